// uvo_akaze_suppress_dev.h -- host AND device (no HIP include): the arithmetic and the decisions of akaze.hip's device form of
// uvo_akaze_suppress.h (k_ak_kcontrast, k_ak_scan, k_ak_refine), so that tests/cpp/akaze_suppress_dev_host.cpp can run the workgroup form
// on a CPU against the sequential scans before any GPU does.
//
// The device form works on the candidate LIST, sorted level by level and row-major inside a level (the order the definition visits), with
// no mark planes: pos[q] = (y << 16) | x ascends inside a level, lvl_start[l] .. lvl_start[l + 1] is level l's range, val[q] the response,
// and a byte per candidate and phase holds its mark.  find_neighbor_point's window -- rows [y - r, y + r), columns [x - r, x + r), clamped,
// "the first marked cell in row-major order that passes dx^2 + dy^2 <= r^2" -- is a walk over the target level's range from the lower
// bound of (y0, x0) to the first row >= y1: list order IS row-major order.
//
// The three phases (within a level; level i against level i - 1; level i against level i + 1) are separated by snapshots: phase p reads
// the scanning level's own marks as phase p - 1 left them and writes the TARGET level's marks of phase p, which no other scan of the
// phase touches; so every scan of a phase is independent of the others and takes one workgroup.  Inside a scan the definition is
// sequential; a candidate's decision reads and writes marks only inside its window (side 2 r around its centre in target coordinates), so
// it may be decided once every EARLIER candidate of the scan whose centre lies within Chebyshev distance 2 r of its own has been (aks_ready):
// nothing earlier can still touch its window, and nothing later whose window meets it can have been decided, by the same rule seen from
// the other side.  A round decides every ready candidate (two ready ones are more than 2 r apart: their windows are disjoint) and the
// rounds repeat until none is left; each round decides at least the earliest undecided candidate, so a scan of m candidates ends within m
// rounds.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define AKS_HD __host__ __device__ inline
#else
#define AKS_HD inline
#endif

namespace uvo {

static const int kAksMaxLevels = 16;
// The list walks below read kAksBatch entries at a time -- independent loads, issued together -- and then test them in order: a walk is a
// chain of dependent trips to L2 otherwise (a few hundred per candidate on a dense level, one workgroup per level), which is what bounded
// k_ak_scan.  An index past the walk's end is clamped to the end and its entry never tested.
static const int kAksBatch = 8;
struct AkCand { int x, y; float v[9]; int pad; };             // a strict maximum and its 3 x 3 neighbourhood (row-major, v[4] = the maximum); pad = its evolution level
struct AksLevel { int w, h, sigma_size, octave; float octave_ratio, esigma; };
struct AksLevels { int n; AksLevel lv[kAksMaxLevels]; };
struct AksKp { float x, y, size, angle, response; int octave, class_id; };      // uvo_keypoint's layout
// one scan: the candidates of level `own` in order, each looking at level `tgt` around (x * mul / div, y * mul / div) with radius r
struct AksScan { int own, tgt, mul, div, r; };
enum { AKS_UNDECIDED = 0, AKS_DECIDED = 1, AKS_READY = 2 };

AKS_HD uint32_t aks_pos(int x, int y) { return ((uint32_t)y << 16) | (uint32_t)x; }
AKS_HD int aks_px(uint32_t p) { return (int)(p & 0xffffu); }
AKS_HD int aks_py(uint32_t p) { return (int)(p >> 16); }
AKS_HD int aks_imin(int a, int b) { return a < b ? a : b; }
AKS_HD int aks_imax(int a, int b) { return a > b ? a : b; }

// compute_kcontrast's last step on the 300-bin histogram (hist[k] = bin k) of the (w - 2) x (h - 2) interior
AKS_HD float aks_kcontrast(float hmax, const int* hist, int total, int nbins)
{
    float kcontrast = 0.03f;
    if (total > 0 && hmax != 0.0f) {
        const int nthreshold = (int)((total - hist[0]) * 0.7f);
        int nelements = 0;
        for (int k = 1; k < nbins; k++) {
            if (nelements >= nthreshold) { kcontrast = (float)hmax * k / nbins; break; }
            nelements = nelements + hist[k];
        }
    }
    return kcontrast;
}

// workgroup wg of phase 0, 1, 2: its scan, or none (own < 0).  *copy_level: the level whose marks of this phase no scan writes and this
// workgroup carries over from the previous phase (-1: none)
AKS_HD AksScan aks_scan_of(int phase, int wg, const AksLevels& L, int* copy_level)
{
    AksScan s = { -1, -1, 1, 1, 0 };
    *copy_level = -1;
    if (phase == 0) { s.own = s.tgt = wg; s.r = L.lv[wg].sigma_size; }
    else if (phase == 1) {
        if (wg == 0) *copy_level = L.n - 1;
        else { s.own = wg; s.tgt = wg - 1; s.mul = (int)L.lv[wg].octave_ratio / (int)L.lv[wg - 1].octave_ratio; s.r = L.lv[wg].sigma_size * s.mul; }
    } else {
        if (wg == L.n - 1) *copy_level = 0;
        else { s.own = wg; s.tgt = wg + 1; s.div = (int)L.lv[wg + 1].octave_ratio / (int)L.lv[wg].octave_ratio; s.r = L.lv[wg + 1].sigma_size; }
    }
    return s;
}
AKS_HD void aks_centre(uint32_t p, const AksScan& s, int* cx, int* cy) { *cx = aks_px(p) * s.mul / s.div; *cy = aks_py(p) * s.mul / s.div; }

AKS_HD int aks_lower_bound(const uint32_t* pos, int a, int b, uint32_t key)
{
    while (a < b) { const int m = a + (b - a) / 2; if (pos[m] < key) a = m + 1; else b = m; }
    return a;
}
// find_neighbor_point on the list range [ta, tb) of a tw x th level: the first marked candidate, in row-major order, inside the window
// around (cx, cy) and within r (L2); -1: none
AKS_HD int aks_find(const uint32_t* pos, const uint8_t* mark, int ta, int tb, int cx, int cy, int r, int tw, int th)
{
    const int j0 = aks_imax(cx - r, 0), j1 = aks_imin(cx + r, tw), i0 = aks_imax(cy - r, 0), i1 = aks_imin(cy + r, th), r2 = r * r;
    if (i0 >= i1 || j0 >= j1) return -1;
    for (int p0 = aks_lower_bound(pos, ta, tb, aks_pos(j0, i0)); p0 < tb; p0 += kAksBatch) {
        uint32_t pp[kAksBatch]; uint8_t mm[kAksBatch];
        for (int k = 0; k < kAksBatch; k++) { const int p = aks_imin(p0 + k, tb - 1); pp[k] = pos[p]; mm[k] = mark[p]; }
        for (int k = 0; k < kAksBatch; k++) {
            if (p0 + k >= tb) return -1;
            const int py = aks_py(pp[k]), px = aks_px(pp[k]);
            if (py >= i1) return -1;
            if (px < j0 || px >= j1 || mm[k] == 0) continue;
            const int dx = px - cx, dy = py - cy;
            if (dx * dx + dy * dy <= r2) return p0 + k;
        }
    }
    return -1;
}
// may candidate q of the scan's range [a, ..) be decided?  No earlier candidate that is still undecided has its centre within 2 r
// (Chebyshev).  (Centres ascend by row with the list, so the walk back ends at the first row further than 2 r.)
AKS_HD bool aks_ready(const uint32_t* pos, const uint8_t* state, int a, int q, const AksScan& s)
{
    int cx, cy;
    aks_centre(pos[q], s, &cx, &cy);
    for (int e0 = q - 1; e0 >= a; e0 -= kAksBatch) {
        uint32_t pp[kAksBatch]; uint8_t ss[kAksBatch];
        for (int k = 0; k < kAksBatch; k++) { const int e = aks_imax(e0 - k, a); pp[k] = pos[e]; ss[k] = state[e]; }
        for (int k = 0; k < kAksBatch; k++) {
            if (e0 - k < a) return true;
            int ex, ey;
            aks_centre(pp[k], s, &ex, &ey);
            if (ey < cy - 2 * s.r) return true;
            if (ss[k] != AKS_DECIDED && ex >= cx - 2 * s.r && ex <= cx + 2 * s.r) return false;
        }
    }
    return true;
}
// the body of the definition's loops for candidate q.  mt: the marks this phase writes ([ta, tb) = the target level's range).
// Phase 0 (FindKeypointsSameScale): a marked neighbour that is not weaker keeps q out; a weaker one loses its mark; q is marked.
// Phases 1, 2 (Find_Scale_Space_Extrema): a marked candidate unmarks the first marked neighbour of the other level when it is stronger.
AKS_HD void aks_decide(int phase, const uint32_t* pos, const float* val, uint8_t* mt, int ta, int tb, int q, const AksScan& s, int tw, int th)
{
    int cx, cy;
    aks_centre(pos[q], s, &cx, &cy);
    const int p = aks_find(pos, mt, ta, tb, cx, cy, s.r, tw, th);
    if (phase == 0) {
        if (p >= 0) { if (val[q] > val[p]) mt[p] = 0; else return; }
        mt[q] = 1;
    } else if (p >= 0 && val[q] > val[p]) mt[p] = 0;
}

// Do_Subpixel_Refinement for one marked candidate of level `level`: false = rejected (|dx| or |dy| above 1)
AKS_HD bool aks_refine(const AkCand& cd, const AksLevel& e, int level, AksKp* out)
{
    const float ratio = e.octave_ratio;
    AksKp k;
    k.x = cd.x * e.octave_ratio; k.y = cd.y * e.octave_ratio;
    k.size = e.esigma * 1.5f;
    k.angle = -1; k.response = cd.v[4]; k.octave = e.octave; k.class_id = level;
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
    if ((dx < 0 ? -dx : dx) > 1.0f || (dy < 0 ? -dy : dy) > 1.0f) return false;
    k.x += dx * ratio + .5f * (ratio - 1.f);
    k.y += dy * ratio + .5f * (ratio - 1.f);
    k.angle = 0.0f;
    k.size *= 2.0f;
    *out = k;
    return true;
}

}  // namespace uvo
