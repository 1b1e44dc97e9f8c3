// PoseDetection.cpp -- see PoseDetection.h.
#include "PoseDetection.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "PostProcess.h"

namespace lmamd {

PoseDetection::PoseDetection(CameraParameters const& cam, TemplateGenerationSettings const& ts)
    : line(new HighLevelLineMOD(cam, ts)), camParams(cam), templateSettings(ts) {
    if (ts.useIcp) {   // :10-11: HighLevelLinemodIcp(6, 0.1f, 2.5f, 8, icpSubsamplingFactor, ...)
        icp = new HighLevelLinemodIcp(line->handle(), 6, 0.1f, 2.5f, 8, ts.icpSubsamplingFactor, {}, ts.modelFolder);
        icpRender = new SoftRender(cam);
    }
}

PoseDetection::~PoseDetection() {
    delete bench;
    delete icp;
    delete icpRender;
    delete line;
}

void PoseDetection::loadTemplates() {
    line->readLinemod();
    refreshClassIds();
    std::printf("Loaded with %d classes and %u templates\n", (int)line->getNumClasses(), (unsigned)line->getNumTemplates());
}

void PoseDetection::refreshClassIds() {
    ids = line->getClassIds();
    if (!icp) return;
    // loadModels: modelFolder + class id (the model file name) for every class; a class whose model cannot be read is refined by no one
    // and reported by detect() through lastError()
    for (size_t k = 0; k < ids.size(); ++k) {
        Mesh m;
        if (load_ply_ascii(templateSettings.modelFolder + ids[k], m)) icp->setModel((uint16_t)k, m);
    }
}

uint16_t PoseDetection::findIndexInVector(std::string const& s, std::vector<std::string>& v) {
    return (uint16_t)std::distance(v.begin(), std::find(v.begin(), v.end(), s));
}

// translateImg(img, -cx + videoWidth / 2, -cy + videoHeight / 2) on clones of both images (:54-59): a pure integer
// shift (the offsets are ints, :192-197), zeros shifted in.  in_imgs[0] must be dense BGR, in_imgs[1] dense depth.
void PoseDetection::shiftFrame(const std::vector<Image>& in, Shifted& buf, std::vector<Image>& out) {
    const int ox = (int)(-camParams.cx + camParams.videoWidth / 2), oy = (int)(-camParams.cy + camParams.videoHeight / 2);
    out = in;
    const int w = in[0].width, h = in[0].height;
    std::vector<uint8_t> dense;
    const uint8_t* src = static_cast<const uint8_t*>(in[0].data);
    if (in[0].stride && in[0].stride != (size_t)w * 3) {
        dense.resize((size_t)w * h * 3);
        for (int y = 0; y < h; ++y) std::memcpy(&dense[(size_t)y * w * 3], src + (size_t)y * in[0].stride, (size_t)w * 3);
        src = dense.data();
    }
    translate_u8c3(src, w, h, ox, oy, buf.color);
    out[0].data = buf.color.data(); out[0].stride = 0;
    if (in.size() >= 2) {
        std::vector<uint16_t> dd;
        const uint16_t* ds = static_cast<const uint16_t*>(in[1].data);
        if (in[1].stride && in[1].stride != (size_t)w * 2) {
            dd.resize((size_t)w * h);
            for (int y = 0; y < h; ++y) std::memcpy(&dd[(size_t)y * w], reinterpret_cast<const uint8_t*>(ds) + (size_t)y * in[1].stride, (size_t)w * 2);
            ds = dd.data();
        }
        translate_u16(ds, w, h, ox, oy, buf.depth);
        out[1].data = buf.depth.data(); out[1].stride = 0;
    }
}

// The masks of a frame through the same translation as shiftFrame's (zeros shifted in: those pixels are not searched).
void PoseDetection::shiftMasks(const std::vector<Image>& in, std::vector<std::vector<uint8_t>>& buf, std::vector<Image>& out) {
    const int ox = (int)(-camParams.cx + camParams.videoWidth / 2), oy = (int)(-camParams.cy + camParams.videoHeight / 2);
    out = in;
    buf.assign(in.size(), std::vector<uint8_t>());
    for (size_t k = 0; k < in.size(); ++k) {
        if (!in[k].data) continue;
        const int w = in[k].width, h = in[k].height;
        const uint8_t* src = static_cast<const uint8_t*>(in[k].data);
        std::vector<uint8_t> dense;
        if (in[k].stride && in[k].stride != (size_t)w) {
            dense.resize((size_t)w * h);
            for (int y = 0; y < h; ++y) std::memcpy(&dense[(size_t)y * w], src + (size_t)y * in[k].stride, (size_t)w);
            src = dense.data();
        }
        translate_u8(src, w, h, ox, oy, buf[k]);
        out[k].data = buf[k].data(); out[k].stride = 0;
    }
}

static const char* kIcpBatchRefusal = "use icp is set: the ICP refinement runs in detect() only, not in the batch and stream forms";

// :70-95 without the ICP branch: the first pose of every group, until in_numberOfObjects poses are collected
void PoseDetection::pickFinal(const std::vector<std::vector<ObjectPose>>& groups, uint16_t nObjects, std::vector<ObjectPose>& out) {
    out.clear();
    for (const auto& g : groups) {
        if (g.empty()) continue;
        out.push_back(g[0]);
        if (out.size() == nObjects) break;
    }
}

void PoseDetection::pickFinalIcp(std::vector<std::vector<ObjectPose>>& groups, uint16_t nObjects, const std::vector<Image>& shifted,
                                 uint16_t classIndex, std::vector<ObjectPose>& out) {
    out.clear();
    if (shifted.size() < 2 || !shifted[1].data) { error = "use icp needs the depth image"; return; }
    const uint16_t* depth = static_cast<const uint16_t*>(shifted[1].data);
    const int w = shifted[1].width, h = shifted[1].height;
    for (auto& g : groups) {
        if (g.empty()) continue;
        uint16_t best = 0;
        icp->prepareDepthForIcp(depth, w, h, camParams, g[0].boundingBox);
        if (!icp->registerToScene(g, classIndex)) { error = icp->lastError(); return; }
        // the best-pose check on the GPU: the means, and so the verdict, are those of estimateBestMatch
        std::vector<double> means;
        if (!icp->meanDepthDifferencesGpu(depth, w, h, g, *icpRender, classIndex, means)) { error = icp->lastError(); return; }
        if (HighLevelLinemodIcp::selectBestMatch(means, best)) out.push_back(g[best]);
        if (out.size() == nObjects) break;
    }
}

// "use icp" in the batch forms: what stands in the way of refining frames in slots (empty: nothing)
std::string PoseDetection::icpBatchRefusal() const {
    if (!line->keepsDepthOnDevice()) return "use icp is set: a colour-only detector keeps no depth frame in its slots, the ICP refinement runs in detect() only";
    if (!line->usesGpuColorCheck()) return "use icp is set: with the host colour check the frames go up unshifted, the ICP refinement needs the shifted frames in the slots";
    return std::string();
}

// :70-95 for a whole batch: one refinement call and one verification call for every non-empty group of every frame
// and class, on the frames resident in slots in_firstSlot + i; then, per frame and class, pickFinalIcp's walk in group order.
bool PoseDetection::pickFinalIcpSlots(std::vector<std::vector<std::vector<std::vector<ObjectPose>>>>& groups, const std::vector<uint16_t>& classes,
                                      int in_firstSlot, uint16_t nObjects, std::vector<std::vector<std::vector<ObjectPose>>>& out) {
    struct Where { size_t c, i, g; };
    std::vector<HighLevelLinemodIcp::SlotGroup> items;
    std::vector<Where> where;
    const size_t nc = std::min(out.size(), groups.size());
    const size_t nf = out.empty() ? 0 : out[0].size();
    for (size_t i = 0; i < nf; ++i)
        for (size_t c = 0; c < nc; ++c) {
            if (i >= groups[c].size()) continue;
            for (size_t g = 0; g < groups[c][i].size(); ++g) {
                std::vector<ObjectPose>& grp = groups[c][i][g];
                if (grp.empty()) continue;
                HighLevelLinemodIcp::SlotGroup e;
                e.slot = in_firstSlot + (int)i; e.modelNumber = classes[c]; e.boundingBox = grp[0].boundingBox; e.poses = &grp;
                items.push_back(e);
                where.push_back({c, i, g});
            }
        }
    std::vector<int32_t> status;
    std::vector<std::vector<double>> means;
    if (!icp->registerToSceneSlots(items, camParams.videoWidth, camParams.videoHeight, camParams, status)) { error = icp->lastError(); return false; }
    if (!icp->meanDepthDifferencesSlots(items, *icpRender, means)) { error = icp->lastError(); return false; }
    for (size_t k = 0; k < items.size(); ++k) {
        const Where& w = where[k];
        std::vector<ObjectPose>& dst = out[w.c][w.i];
        if (dst.size() >= nObjects) continue;            // behind the frame's stop: detect() never looks at these groups
        if (status[k] != LM_OK && status[k] != LM_ERR_INVALID) {       // (LM_ERR_INVALID: a short cloud, the poses stay unrefined)
            error = "frame " + std::to_string(w.i) + ", class " + ids[classes[w.c]] + ", group " + std::to_string(w.g) +
                    ": the ICP refinement failed with code " + std::to_string(status[k]) + " (a scene cloud over the capacity)";
            return false;
        }
        uint16_t best = 0;
        if (HighLevelLinemodIcp::selectBestMatch(means[k], best)) dst.push_back((*items[k].poses)[best]);
    }
    return true;
}

void PoseDetection::detect(std::vector<Image>& in_imgs, std::string const& in_className, uint16_t const& in_numberOfObjects,
                           std::vector<ObjectPose>& in_objPose, bool in_displayResults) {
    const uint16_t numClassIndex = findIndexInVector(in_className, ids);
    Shifted buf;
    std::vector<Image> inputImg;
    shiftFrame(in_imgs, buf, inputImg);
    finalObjectPoses.clear();
    error.clear();
    line->detectTemplate(inputImg, numClassIndex);
    detectedPoses = line->getObjectPoses();
    if (icp) pickFinalIcp(detectedPoses, in_numberOfObjects, inputImg, numClassIndex, finalObjectPoses);
    else pickFinal(detectedPoses, in_numberOfObjects, finalObjectPoses);
    if (in_displayResults)
        for (const ObjectPose& p : finalObjectPoses) in_objPose.push_back(p);
    if (bench) score(inputImg, in_displayResults);
}

void PoseDetection::detect(std::vector<Image>& in_imgs, std::vector<Image> const& in_masks, std::string const& in_className,
                           uint16_t const& in_numberOfObjects, std::vector<ObjectPose>& in_objPose, bool in_displayResults) {
    const uint16_t numClassIndex = findIndexInVector(in_className, ids);
    Shifted buf;
    std::vector<Image> inputImg, inputMasks;
    std::vector<std::vector<uint8_t>> maskBuf;
    shiftFrame(in_imgs, buf, inputImg);
    shiftMasks(in_masks, maskBuf, inputMasks);
    finalObjectPoses.clear();
    error.clear();
    line->detectTemplate(inputImg, numClassIndex, inputMasks);
    detectedPoses = line->getObjectPoses();
    if (icp) pickFinalIcp(detectedPoses, in_numberOfObjects, inputImg, numClassIndex, finalObjectPoses);
    else pickFinal(detectedPoses, in_numberOfObjects, finalObjectPoses);
    if (in_displayResults)
        for (const ObjectPose& p : finalObjectPoses) in_objPose.push_back(p);
    if (bench) score(inputImg, in_displayResults);
}

bool PoseDetection::setupBenchmark(std::string const& in_className, std::string const& in_groundTruthFolder) {
    error.clear();
    Mesh m;
    std::string err;
    if (!load_ply_ascii(templateSettings.modelFolder + in_className, m, &err)) { error = "benchmark model " + in_className + ": " + err; return false; }
    return setupBenchmark(in_className, m, in_groundTruthFolder);
}

bool PoseDetection::setupBenchmark(std::string const& in_className, const Mesh& in_mesh, std::string const& in_groundTruthFolder) {
    error.clear();
    const uint16_t k = findIndexInVector(in_className, ids);
    if (k >= ids.size()) { error = "unknown class name: " + in_className; return false; }
    Benchmark* b = new Benchmark(line->handle(), camParams);
    b->groundTruthFolder = in_groundTruthFolder;
    if (!b->loadModel(in_mesh, k)) { error = b->lastError(); delete b; return false; }
    delete bench;
    bench = b;
    benchClass = k;
    return true;
}

// :96-104, 115-120: the Hodan error of the first final pose on the shifted depth image; the counter advances with in_displayResults
void PoseDetection::score(const std::vector<Image>& shifted, bool in_displayResults) {
    if (!finalObjectPoses.empty()) {
        if (shifted.size() < 2 || !shifted[1].data) { error = "the benchmark needs the depth image"; benchError = std::numeric_limits<float>::quiet_NaN(); }
        else {
            benchError = bench->calculateErrorHodan(static_cast<const uint16_t*>(shifted[1].data), shifted[1].width, shifted[1].height,
                                                    finalObjectPoses[0], benchClass);
            if (!bench->lastError().empty() && std::isnan(benchError)) error = bench->lastError();
            std::printf("Error: %g\n", benchError);
        }
    }
    if (in_displayResults) bench->increaseImgCounter();
}

bool PoseDetection::detectBatch(std::vector<std::vector<Image>>& in_frames, std::string const& in_className,
                                uint16_t const& in_numberOfObjects, std::vector<std::vector<ObjectPose>>& out) {
    error.clear();
    out.assign(in_frames.size(), {});
    if (icp) { error = kIcpBatchRefusal; return false; }
    const uint16_t numClassIndex = findIndexInVector(in_className, ids);
    if (numClassIndex >= ids.size()) { error = "unknown class name: " + in_className; return false; }   // (find's not-found index = ids.size())
    if (in_frames.size() > (size_t)HighLevelLineMOD::kBatchSlots) { error = "batch of " + std::to_string(in_frames.size()) + " frames exceeds the detector's frame slots"; return false; }
    if (batchBufs.size() < in_frames.size()) batchBufs.resize(in_frames.size());
    std::vector<std::vector<Image>> shifted(in_frames.size());
    for (size_t i = 0; i < in_frames.size(); ++i) shiftFrame(in_frames[i], batchBufs[i], shifted[i]);
    std::vector<std::vector<lm_match_t>> m;
    std::vector<std::vector<std::vector<ObjectPose>>> groups;
    line->detectTemplateBatch(shifted, numClassIndex, m, groups);
    if (!line->lastError().empty()) { error = line->lastError(); return false; }     // (the batch entry points clear it on entry)
    for (size_t i = 0; i < in_frames.size() && i < groups.size(); ++i) pickFinal(groups[i], in_numberOfObjects, out[i]);
    finalObjectPoses = out.empty() ? std::vector<ObjectPose>() : out.back();
    return true;
}

bool PoseDetection::detectBatch(std::vector<std::vector<Image>>& in_frames, std::vector<std::string> const& in_classNames,
                                uint16_t const& in_numberOfObjects, std::vector<std::vector<std::vector<ObjectPose>>>& out) {
    out.assign(in_classNames.size(), std::vector<std::vector<ObjectPose>>(in_frames.size()));
    if (line->batchesInFlight() != 0) { error = "batches are in flight: collect them with detectBatchEnd first"; return false; }
    if (!detectBatchBegin(in_frames, in_classNames)) return false;
    return detectBatchEnd(in_numberOfObjects, out);
}

bool PoseDetection::detectBatchSlots(int in_firstSlot, int in_nFrames, std::vector<std::string> const& in_classNames, uint16_t const& in_numberOfObjects,
                                     std::vector<std::vector<std::vector<ObjectPose>>>& out) {
    error.clear();
    out.assign(in_classNames.size(), std::vector<std::vector<ObjectPose>>((size_t)std::max(in_nFrames, 0)));
    if (icp && !icpBatchRefusal().empty()) { error = icpBatchRefusal(); return false; }
    std::vector<uint16_t> idx;
    for (const std::string& nme : in_classNames) {
        const uint16_t k = findIndexInVector(nme, ids);
        if (k >= ids.size()) { error = "unknown class name: " + nme; return false; }
        idx.push_back(k);
    }
    std::vector<std::vector<std::vector<lm_match_t>>> m;
    std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> groups;
    line->detectTemplatesSlots(in_firstSlot, in_nFrames, idx, m, groups);
    if (!line->lastError().empty()) { error = line->lastError(); return false; }
    if (icp) {
        if (!pickFinalIcpSlots(groups, idx, in_firstSlot, in_numberOfObjects, out)) return false;
    } else
    for (size_t c = 0; c < out.size() && c < groups.size(); ++c)
        for (size_t i = 0; i < out[c].size() && i < groups[c].size(); ++i) pickFinal(groups[c][i], in_numberOfObjects, out[c][i]);
    finalObjectPoses = (out.empty() || out.back().empty()) ? std::vector<ObjectPose>() : out.back().back();
    return true;
}

bool PoseDetection::exportResults(int in_firstSlot, int in_nFrames, std::vector<std::vector<ObjectPose>> const& in_posesPerFrame,
                                  const lm_image_desc* in_dst, const lm_ingest_opts* in_undo) {
    error.clear();
    exportPrims.clear();
    for (size_t i = 0; i < in_posesPerFrame.size() && (int)i < in_nFrames; ++i)
        for (const ObjectPose& pose : in_posesPerFrame[i]) {
            drawAxes(pose, camParams, 75.0f, (int)i, exportPrims);
            drawBox(pose.boundingBox, 0, 255, 255, 1, (int)i, exportPrims);
        }
    if (lm_export_frames(line->handle(), in_firstSlot, in_nFrames, in_dst, in_undo, exportPrims.data(), exportPrims.size()) != LM_OK) {
        error = lm_last_error();
        return false;
    }
    return true;
}

bool PoseDetection::detectBatchBegin(std::vector<std::vector<Image>>& in_frames, std::vector<std::string> const& in_classNames) {
    error.clear();
    if (icp && !icpBatchRefusal().empty()) { error = icpBatchRefusal(); return false; }
    std::vector<uint16_t> idx;
    for (const std::string& nme : in_classNames) {
        const uint16_t k = findIndexInVector(nme, ids);
        if (k >= ids.size()) { error = "unknown class name: " + nme; return false; }
        idx.push_back(k);
    }
    if (in_frames.size() > (size_t)HighLevelLineMOD::kBatchSlots) { error = "batch of " + std::to_string(in_frames.size()) + " frames exceeds the detector's frame slots"; return false; }
    // (before anything is translated: a refused Begin must not touch the buffers of a batch in flight)
    if (line->batchesInFlight() >= HighLevelLineMOD::kBatchSets) { error = "all slot sets are in flight: call detectBatchEnd first"; return false; }
    std::vector<std::vector<Image>> shifted(in_frames.size());
    if (line->usesGpuColorCheck()) {
        // r04: nothing is translated on the host -- the frames go up with the shift applied while the staging buffer is filled (or by the
        // DMA engine's row-offset copy for pinned frames) and the host depth check reads the untranslated depth image through the same shift
        const int ox = (int)(-camParams.cx + camParams.videoWidth / 2), oy = (int)(-camParams.cy + camParams.videoHeight / 2);
        for (size_t i = 0; i < in_frames.size(); ++i) {
            shifted[i] = in_frames[i];
            for (Image& im : shifted[i]) { im.shift_x = ox; im.shift_y = oy; }
        }
    } else {
        // host colour check: translated copies, one buffer set per batch in flight (they must outlive the batch's End)
        const size_t base = streamBufNext * (size_t)HighLevelLineMOD::kBatchSlots;
        streamBufNext = (streamBufNext + 1) % (size_t)HighLevelLineMOD::kBatchSets;
        if (batchBufs.size() < (size_t)HighLevelLineMOD::kBatchSlots * HighLevelLineMOD::kBatchSets) batchBufs.resize((size_t)HighLevelLineMOD::kBatchSlots * HighLevelLineMOD::kBatchSets);
        for (size_t i = 0; i < in_frames.size(); ++i) shiftFrame(in_frames[i], batchBufs[base + i], shifted[i]);
    }
    if (!line->detectTemplatesBatchBegin(shifted, idx)) { error = line->lastError(); return false; }
    streamShape.push_back({in_classNames.size(), in_frames.size()});
    streamClasses.push_back(idx);
    return true;
}

bool PoseDetection::detectBatchEnd(uint16_t const& in_numberOfObjects, std::vector<std::vector<std::vector<ObjectPose>>>& out) {
    error.clear();
    if (streamShape.empty()) { error = "no batch in flight"; out.clear(); return false; }
    const std::pair<size_t, size_t> shape = streamShape.front();
    const std::vector<uint16_t> classes = streamClasses.front();
    streamShape.pop_front();
    streamClasses.pop_front();
    out.assign(shape.first, std::vector<std::vector<ObjectPose>>(shape.second));
    std::vector<std::vector<std::vector<lm_match_t>>> m;
    std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> groups;
    line->detectTemplatesBatchEnd(m, groups);
    if (!line->lastError().empty()) { error = line->lastError(); return false; }     // (the batch entry points clear it on entry)
    if (icp) {      // the batch's frames are still resident, shifted, in the slots it was matched on
        if (!pickFinalIcpSlots(groups, classes, line->lastBatchFirstSlot(), in_numberOfObjects, out)) return false;
    } else
    for (size_t c = 0; c < shape.first && c < groups.size(); ++c)
        for (size_t i = 0; i < shape.second && i < groups[c].size(); ++i) pickFinal(groups[c][i], in_numberOfObjects, out[c][i]);
    finalObjectPoses = (out.empty() || out.back().empty()) ? std::vector<ObjectPose>() : out.back().back();
    return true;
}

}  // namespace lmamd
