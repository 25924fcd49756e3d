// uvo_akaze_suppress.h -- host only (no HIP include): what OpenCV's AKAZE does SEQUENTIALLY on the candidate list, for akaze.hip
// (uvo_akaze_set_suppression 0) and for the host test tests/cpp/akaze_suppress_dev_host.cpp.  THE DEFINITION of the device form
// (uvo_akaze_suppress_dev.h): the order the candidates are visited in, find_neighbor_point, FindKeypointsSameScale's sequential half,
// the two cross-scale sweeps of Find_Scale_Space_Extrema and Do_Subpixel_Refinement with solve()'s double determinant.
#pragma once
#include "uvo_akaze_suppress_dev.h"
#include <math.h>
#include <string.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

namespace uvo {
namespace {

struct AksHost {
    AksLevels L;
    std::vector<uint8_t> mask[kAksMaxLevels]; std::vector<float> val[kAksMaxLevels];             // keypoint mask and Ldet at candidates, whole planes
    std::vector<std::vector<AkCand>> cands;                                                      // per level, in visiting order
    std::vector<uint64_t> keys;                                                                  // sort keys of the candidate list
};
inline void aks_host_init(AksHost* s, const AksLevels& L)
{
    s->L = L;
    for (int i = 0; i < L.n; i++) { const size_t n = (size_t)L.lv[i].w * L.lv[i].h; s->mask[i].assign(n, 0); s->val[i].assign(n, 0.f); }
    s->cands.assign(kAksMaxLevels, std::vector<AkCand>());
}
// last frame's keypoint marks (the masks are whole planes: clearing the few thousand marked entries, not 11 MB of planes per frame)
inline void aks_host_clear(AksHost* s)
{
    for (int i = 0; i < s->L.n; i++) { for (const AkCand& cd : s->cands[i]) s->mask[i][(size_t)cd.y * s->L.lv[i].w + cd.x] = 0; s->cands[i].clear(); }
}
// level by level, row-major inside a level -- the order the scans visit them: one sort of 64-bit keys (level, y, x, list position)
inline void aks_host_order(AksHost* s, const AkCand* list, int n_cand)
{
    std::vector<uint64_t>& keys = s->keys;
    keys.resize((size_t)n_cand);
    for (int q = 0; q < n_cand; q++) { const AkCand& cd = list[q]; keys[(size_t)q] = ((uint64_t)cd.pad << 58) | ((uint64_t)cd.y << 40) | ((uint64_t)cd.x << 22) | (uint64_t)q; }
    std::sort(keys.begin(), keys.end());
    for (int q = 0; q < n_cand; q++) { const AkCand& cd = list[keys[(size_t)q] & 0x3fffffu]; s->cands[cd.pad].push_back(cd); }
}
// find_neighbor_point (AKAZEFeatures.cpp): a keypoint of `mask` within search_radius (L2) of (x, y), scanning the square window row-major
inline bool find_neighbor_point(int x, int y, const std::vector<uint8_t>& mask, int cols, int rows, int search_radius, int* idx)
{
    // (the marks are sparse: eight mask bytes are tested at a time and only a non-zero word is walked byte by byte, in the same order)
    const int j0 = std::max(x - search_radius, 0), j1 = std::min(x + search_radius, cols), r2 = search_radius * search_radius;
    for (int i = std::max(y - search_radius, 0); i < std::min(y + search_radius, rows); ++i) {
        const uint8_t* curr = mask.data() + (size_t)i * cols;
        const int dy = i - y;
        for (int j = j0; j < j1;) {
            if (j1 - j >= 8) { uint64_t wd; memcpy(&wd, curr + j, 8); if (wd == 0) { j += 8; continue; } }
            if (curr[j] != 0) { const int dx = j - x; if (dx * dx + dy * dy <= r2) { *idx = i * cols + j; return true; } }
            ++j;
        }
    }
    return false;
}
// ---- FindKeypointsSameScale's sequential half ----
inline void aks_host_within(AksHost* s)
{
    for (int i = 0; i < s->L.n; i++) {
        const AksLevel& lv = s->L.lv[i];
        for (const AkCand& cd : s->cands[i]) {
            const float value = cd.v[4];
            s->val[i][(size_t)cd.y * lv.w + cd.x] = value;
            int idx = 0;
            if (find_neighbor_point(cd.x, cd.y, s->mask[i], lv.w, lv.h, lv.sigma_size, &idx)) {
                if (value > s->val[i][idx]) s->mask[i][idx] = 0;
                else continue;
            }
            s->mask[i][(size_t)cd.y * lv.w + cd.x] = 1;
        }
    }
}
// ---- Find_Scale_Space_Extrema's two sweeps ----
inline void aks_host_sweep_lower(AksHost* s)
{
    for (int i = 1; i < s->L.n; i++) {
        const AksLevel& lv = s->L.lv[i]; const AksLevel& lp = s->L.lv[i - 1];
        const int diff_ratio = (int)lv.octave_ratio / (int)lp.octave_ratio, search_radius = lv.sigma_size * diff_ratio;
        for (const AkCand& cd : s->cands[i]) {
            const size_t j = (size_t)cd.y * lv.w + cd.x;
            if (s->mask[i][j] == 0) continue;
            int idx = 0;
            if (find_neighbor_point(cd.x * diff_ratio, cd.y * diff_ratio, s->mask[i - 1], lp.w, lp.h, search_radius, &idx))
                if (s->val[i][j] > s->val[i - 1][idx]) s->mask[i - 1][idx] = 0;
        }
    }
}
inline void aks_host_sweep_upper(AksHost* s)
{
    for (int i = s->L.n - 2; i >= 0; i--) {
        const AksLevel& lv = s->L.lv[i]; const AksLevel& ln = s->L.lv[i + 1];
        const int diff_ratio = (int)ln.octave_ratio / (int)lv.octave_ratio, search_radius = ln.sigma_size;
        for (const AkCand& cd : s->cands[i]) {
            const size_t j = (size_t)cd.y * lv.w + cd.x;
            if (s->mask[i][j] == 0) continue;
            int idx = 0;
            if (find_neighbor_point(cd.x / diff_ratio, cd.y / diff_ratio, s->mask[i + 1], ln.w, ln.h, search_radius, &idx))
                if (s->val[i][j] > s->val[i + 1][idx]) s->mask[i + 1][idx] = 0;
        }
    }
}
// the mark of every candidate of the list aks_host_order was given, in that list's order (the test hook's `marks`, one phase)
inline void aks_host_marks(const AksHost* s, const AkCand* list, int n_cand, uint8_t* marks, int stride)
{
    for (int q = 0; q < n_cand; q++) marks[(size_t)q * stride] = s->mask[list[q].pad][(size_t)list[q].y * s->L.lv[list[q].pad].w + list[q].x];
}
// ---- Do_Subpixel_Refinement (a 2 x 2 solve per keypoint on the neighbourhood the candidate record carries); KP = uvo_keypoint ----
template <class KP> inline void aks_host_refine(const AksHost* s, std::vector<KP>* out_)
{
    std::vector<KP>& out = *out_;
    out.clear();
    for (int i = 0; i < s->L.n; i++) {
        const AksLevel& e = s->L.lv[i];
        const float ratio = e.octave_ratio;
        for (const AkCand& cd : s->cands[i]) {
            if (s->mask[i][(size_t)cd.y * e.w + cd.x] == 0) continue;
            KP k;
            k.x = cd.x * e.octave_ratio; k.y = cd.y * e.octave_ratio;
            k.size = e.esigma * 1.5f;
            k.angle = -1; k.response = cd.v[4]; k.octave = e.octave; k.class_id = i;
            const float* v = cd.v;                                   // v[3 * (dy + 1) + (dx + 1)]
            const float Dx = 0.5f * (v[5] - v[3]);
            const float Dy = 0.5f * (v[7] - v[1]);
            const float Dxx = v[5] + v[3] - 2.0f * v[4];
            const float Dyy = v[7] + v[1] - 2.0f * v[4];
            const float Dxy = 0.25f * (v[8] + v[0] - v[2] - v[6]);
            // solve(Matx22f, Vec2f, DECOMP_LU): lapack.cpp's 2 x 2 CV_32F branch -- determinant and numerators in double, the result
            // cast to float; a zero determinant leaves dst = 0
            float dx = 0.0f, dy = 0.0f;
            double det = (double)Dxx * Dyy - (double)Dxy * Dxy;
            if (det != 0) { det = 1. / det; dx = (float)(((double)(-Dx) * Dyy - (double)(-Dy) * Dxy) * det); dy = (float)(((double)(-Dy) * Dxx - (double)(-Dx) * Dxy) * det); }
            if (fabsf(dx) > 1.0f || fabsf(dy) > 1.0f) continue;
            k.x += dx * ratio + .5f * (ratio - 1.f);
            k.y += dy * ratio + .5f * (ratio - 1.f);
            k.angle = 0.0f;
            k.size *= 2.0f;
            out.push_back(k);
        }
    }
}

}  // namespace
}  // namespace uvo
