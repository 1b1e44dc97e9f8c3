// lm_extract.h -- host half of Detector::addTemplate (reference call site
// /root/reference/src/HighLevelLinemod.cpp:93): the quantised images come from the GPU kernels,
// feature selection (a greedy pick) runs here on the host.  This file is the yardstick of the selection on the GPU
// (lm_k_select.hip), which lm_add_templates_slots and lm_add_templates_rendered use.
#pragma once
#include <string>
#include <vector>

#include "lm_host.h"

namespace lmh {

// One pyramid level of the quantised sources of a template image, as read back from the device.
struct ExtractLevel {
    int w = 0, h = 0;
    std::vector<u8> color_q;       // ColorGradient quantised orientations (one-hot)
    std::vector<float> color_mag;  // squared gradient magnitude of the selected channel
    std::vector<u8> depth_q;       // DepthNormal quantised normals (empty for a colour-only detector)
    std::vector<u8> mask;          // object mask at this level (empty = no mask)
};

// Fills tp ([level*M + modality]) from the per-level images; returns false when some level yields
// fewer candidates than requested features (upstream addTemplate then returns -1).
bool extract_pyramid(const std::vector<ExtractLevel>& levels, const lm_config& cfg, TemplatePyramid& tp);

// A feature candidate: position and label at its level, score = squared gradient magnitude (colour) or chessboard distance (depth).
struct Candidate {
    lm_feature f;
    float score;
};
// The selection half of the colour / depth extraction, after the host collection of extract_pyramid (k_select restates both on the
// GPU's candidate lists).  cands must be in row-major order (the stable sort keeps it among equal scores); per_label = the
// candidates per depth label, area = the interior's pixel count (the whole level without a mask).  false: fewer than `want`.
bool select_color(std::vector<Candidate>& cands, size_t want, Template& t);
bool select_depth(std::vector<Candidate>& cands, const int per_label[8], float area, size_t want, Template& t);

// cropTemplates: bounding box over all levels/modalities in level-0 units, features made relative.
lm_rect crop_templates(TemplatePyramid& tp);

}  // namespace lmh
