// PoseDetection.h -- headless equivalent of the reference's online pipeline class
//     class PoseDetection            /root/reference/include/PoseDetection.h:18-106, src/PoseDetection.cpp
// over the HighLevelLineMOD facade: class name -> index (:49), principal-point shift of both images (:54-59,192-197),
// detectTemplate (:66), first pose of every group until in_numberOfObjects (:86-92) -- or, with "use icp" set, the ICP branch
// (:70-95): every pose of a group refined on the GPU (HighLevelLinemodIcp), the best one kept when
// estimateBestMatch accepts it (SoftRender stands in for the OpenGL renderer).  The class-list detectBatch, the stream forms and
// detectBatchSlots run the ICP branch on the frames resident in the slots: one batched refinement and one verification call for all
// groups of the batch, the outputs those of detect() frame by frame.  They refuse, with the reason in
// lastError(), on a colour-only detector (its slots keep no depth frame) and with the host colour check (its frames go up
// unshifted); the single-class detectBatch runs no ICP branch and refuses with "use icp" set.  After setupBenchmark (:128-133), detect() scores its
// first final pose with the Hodan error on the GPU (:96-104, Benchmark.h); the batch and stream forms do not score.  imshow (:121)
// needs a display and is out of scope; the drawing in front of it (:105-112, drawCoordinateSystem) is exportResults: the annotated
// frames written to device memory of the caller's on the GPU (Draw.h).
#pragma once
#include <deque>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "Benchmark.h"
#include "Draw.h"
#include "HighLevelLinemod.h"
#include "HighLevelLinemodIcp.h"
#include "TemplateGenerator.h"

namespace lmamd {

class PoseDetection {
public:
    // The reference's constructor reads linemod_settings.yml and the template files itself (:3-18); here the settings
    // are handed in (readSettings() fills them from the same file) and loadTemplates() is readLinemodFromFile (:142-160).
    PoseDetection(CameraParameters const& in_camParams, TemplateGenerationSettings const& in_templateSettings);
    ~PoseDetection();
    PoseDetection(const PoseDetection&) = delete;
    PoseDetection& operator=(const PoseDetection&) = delete;

    void loadTemplates();                                   // readLinemodFromFile: line->readLinemod(), class ids
    HighLevelLineMOD* lineMod() { return line; }            // to add templates in-process instead of reading files
    void refreshClassIds();                                 // after templates were added through lineMod()

    // :45-126.  in_imgs = {colour, depth}.  Like the reference, the poses are appended to in_objPose only when
    // in_displayResults is set (:105-112: the push_back sits inside `if (in_displayResults)`); nothing is drawn here.
    // getFinalObjectPoses() returns them either way.
    void detect(std::vector<Image>& in_imgs, std::string const& in_className, uint16_t const& in_numberOfObjects,
                std::vector<ObjectPose>& in_objPose, bool in_displayResults);
    // The same with Detector::match's per-modality masks (HighLevelLineMOD::detectTemplate with in_masks): in_masks[0] colour,
    // in_masks[1] depth, CV_8UC1 in CAMERA coordinates (those of in_imgs).  They are translated by the principal-point shift exactly
    // like the images; the pixels shifted in are masked out.
    void detect(std::vector<Image>& in_imgs, std::vector<Image> const& in_masks, std::string const& in_className,
                uint16_t const& in_numberOfObjects, std::vector<ObjectPose>& in_objPose, bool in_displayResults);
    // The same for a batch of frames in one pass over the GPU (BASELINE config 5): out[i] = final poses of frame i.
    // Returns false -- with the reason in lastError() -- when the class name is unknown, the batch exceeds the detector's frame
    // slots, or the match fails (capacity overflow, ...): "nothing detected" is true with empty pose lists (r04, ADVICE r3: the
    // reference's void detect cannot tell the two apart; the C ABI underneath can).
    bool detectBatch(std::vector<std::vector<Image>>& in_frames, std::string const& in_className,
                     uint16_t const& in_numberOfObjects, std::vector<std::vector<ObjectPose>>& out_objPoses);
    // Several objects in the same batch of frames (BASELINE config 5: >= 3 models): one upload and one pre-processing per
    // frame for ALL the classes (the reference calls detect once per class name on the same camera frame and pays
    // Detector::match's pyramid each time, PoseDetection.cpp:45-66).  out[c][i] = final poses of class in_classNames[c] in
    // frame i.
    bool detectBatch(std::vector<std::vector<Image>>& in_frames, std::vector<std::string> const& in_classNames,
                     uint16_t const& in_numberOfObjects, std::vector<std::vector<std::vector<ObjectPose>>>& out_objPoses);
    // The several-objects form as a STREAM (r05): Begin hands a batch to the GPU (upload + class-list match on the next free slot set)
    // and returns, End collects the oldest batch begun and runs its post-processing --
    //     detectBatchBegin(b0);  loop { detectBatchBegin(b[k + 1]); detectBatchEnd(n, out[k]); }  detectBatchEnd(n, out[last])
    // overlaps the transfer and the GPU hot path of batch k + 1 with the host's colour / depth checks of batch k.  Up to
    // HighLevelLineMOD::kBatchSets batches in flight; a batch's frames must stay valid until its End has returned.  Same poses, bit
    // for bit, as detectBatch (which is Begin + End).
    bool detectBatchBegin(std::vector<std::vector<Image>>& in_frames, std::vector<std::string> const& in_classNames);
    bool detectBatchEnd(uint16_t const& in_numberOfObjects, std::vector<std::vector<std::vector<ObjectPose>>>& out_objPoses);
    // The several-objects form for frames the caller has ALREADY put into the detector's slots [in_firstSlot, in_firstSlot + in_nFrames) through
    // lineMod()->handle() (lm_upload_* / lm_ingest_*, with the principal-point shift in the ingest's opts): HighLevelLineMOD::detectTemplatesSlots and
    // the final poses on top, as detectBatch sits on detectTemplatesBatch.  No host image is read: with "use depth improvement" the depth statistic
    // must be the sorted one (lineMod()->setDepthStatistic(1) or the settings file's "depth statistic: 1").  Synchronous.  With "use icp" set the
    // groups are refined and checked against the slots' resident depth frames.  out[c][i] = final poses of class in_classNames[c] in the frame of slot in_firstSlot + i.
    bool detectBatchSlots(int in_firstSlot, int in_nFrames, std::vector<std::string> const& in_classNames, uint16_t const& in_numberOfObjects,
                          std::vector<std::vector<std::vector<ObjectPose>>>& out_objPoses);
    // The reference's drawing site (:105-112) for frames resident in slots [in_firstSlot, in_firstSlot + in_nFrames): the coordinate axes (75 mm,
    // drawCoordinateSystem) and the bounding box (yellow, thickness 1) of every pose of in_posesPerFrame[i] drawn onto frame i, then ONE
    // lm_export_frames call: in_dst[i] receives the annotated frame in its format (device memory; an encoder's NV12 surface, a display's
    // buffer), with the ingest options in_undo[i] -- the principal-point shift -- undone (NULL: as the frame lies in the slot).  The
    // primitives of the call are kept in lastExportPrims().  false (lastError) when the call is refused.  Synchronous.
    bool exportResults(int in_firstSlot, int in_nFrames, std::vector<std::vector<ObjectPose>> const& in_posesPerFrame, const lm_image_desc* in_dst,
                       const lm_ingest_opts* in_undo);
    const std::vector<lm_draw_prim>& lastExportPrims() const { return exportPrims; }
    // A match-time gate for detect(), detectBatch and the streamed form (HighLevelLineMOD::setMatchGate): evaluated on the GPU from every
    // frame, in the coordinates of the frame the detector matches (behind the principal-point shift).  Off by default; with "use icp" the
    // refinement sees the same groups it would see with the same masks passed to detect().
    void setMatchGate(const MatchGate& in_gate) { line->setMatchGate(in_gate); }
    void clearMatchGate() { line->clearMatchGate(); }
    const std::vector<ObjectPose>& getFinalObjectPoses() const { return finalObjectPoses; }
    const std::string& lastError() const { return error; }
    // with "use icp" set: the refinement (models are loaded from modelFolder + class id by refreshClassIds; setModel hands one in)
    HighLevelLinemodIcp* icpRefiner() { return icp; }
    // :128-133: from now on detect() scores finalObjectPoses[0] against <groundTruthFolder>pose<counter>.yml (Benchmark::calculateErrorHodan
    // on the principal-point-shifted depth), prints "Error: <e>" and, when in_displayResults is set (like the reference's
    // increaseImgCounter), advances the counter and prints the Hodan score.  The class's mesh is modelFolder + class name (PLY) or
    // in_mesh; it becomes render mesh <class index>.  false (lastError) for an unknown class or an unreadable mesh.  The batch and stream
    // forms (detectBatch*) never score.
    bool setupBenchmark(std::string const& in_className, std::string const& in_groundTruthFolder = "benchmark/");
    bool setupBenchmark(std::string const& in_className, const Mesh& in_mesh, std::string const& in_groundTruthFolder = "benchmark/");
    Benchmark* benchmark() { return bench; }
    float lastBenchmarkError() const { return benchError; }   // NaN before the first scored frame and when scoring failed

private:
    uint16_t findIndexInVector(std::string const& in_stringToFind, std::vector<std::string>& in_vectorToLookIn);   // :134-140
    HighLevelLineMOD* line;
    CameraParameters camParams;
    TemplateGenerationSettings templateSettings;
    std::vector<std::string> ids;
    std::vector<std::vector<ObjectPose>> detectedPoses;
    std::vector<ObjectPose> finalObjectPoses;
    std::string error;
    std::vector<lm_draw_prim> exportPrims;
    // shifted copies of one frame (translateImg works in place on clones, :54-59)
    struct Shifted { std::vector<uint8_t> color; std::vector<uint16_t> depth; };
    std::vector<Shifted> batchBufs;      // detectBatch's shifted frames, kept between calls (6 MB of fresh pages per 1280 x 960 frame otherwise)
    size_t streamBufNext = 0;            // which buffer set the next detectBatchBegin translates into (host colour check only)
    std::deque<std::pair<size_t, size_t>> streamShape;   // (classes, frames) of the batches in flight, oldest first
    std::deque<std::vector<uint16_t>> streamClasses;     // ... and their class indices
    void shiftFrame(const std::vector<Image>& in_imgs, Shifted& buf, std::vector<Image>& out);
    void shiftMasks(const std::vector<Image>& in_masks, std::vector<std::vector<uint8_t>>& buf, std::vector<Image>& out);
    void pickFinal(const std::vector<std::vector<ObjectPose>>& groups, uint16_t nObjects, std::vector<ObjectPose>& out);
    // :70-95 with "use icp": refine, estimateBestMatch, keep the accepted pose of each group (on the shifted depth image)
    void pickFinalIcp(std::vector<std::vector<ObjectPose>>& groups, uint16_t nObjects, const std::vector<Image>& shifted, uint16_t classIndex,
                      std::vector<ObjectPose>& out);
    // the same for a batch whose frames are resident in slots in_firstSlot + i: one refinement and one verification call for all groups
    bool pickFinalIcpSlots(std::vector<std::vector<std::vector<std::vector<ObjectPose>>>>& groups, const std::vector<uint16_t>& classes, int in_firstSlot,
                           uint16_t nObjects, std::vector<std::vector<std::vector<ObjectPose>>>& out);
    std::string icpBatchRefusal() const;
    HighLevelLinemodIcp* icp = nullptr;
    SoftRender* icpRender = nullptr;
    Benchmark* bench = nullptr;
    uint16_t benchClass = 0;
    float benchError = std::numeric_limits<float>::quiet_NaN();
    void score(const std::vector<Image>& shifted, bool in_displayResults);
};

}  // namespace lmamd
