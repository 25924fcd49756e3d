// akaze.hip -- the AKAZE branch of detect_features on gfx950 (uvo_libraries/src/VO_utility.cpp:93-98):
//     Ptr<AKAZE> detector = AKAZE::create();  detector->detectAndCompute(img, noArray(), keypoints, descriptors);
// DESCRIPTOR_MLDB, full length (486 bits = 61 bytes), 3 channels; the detection arguments of AKAZE::create -- threshold, nOctaves,
// nOctaveLayers, diffusivity -- are the context's (uvo_akaze_configure; 0.001f, 4 octaves x 4 sublevels, DIFF_PM_G2 until it is called) -- after
// Alcantarilla, Nuevo, Bartoli, "Fast explicit diffusion for accelerated features in nonlinear scale spaces" (BMVC 2013) in the form
// of OpenCV 4.5's features2d/src/kaze/AKAZEFeatures.cpp as far as it can be recalled (PARITY UNPINNED; the float operation order is
// the scalar one of imgproc's separable filters).
//
// Everything that touches pixels runs on the device, one launch per pass (HBM-bound stencils over float planes, coalesced rows):
//   k_ak_u8_to_f32                 the image in [0, 1]
//   k_ak_blur_rows / _cols         GaussianBlur, BORDER_REPLICATE (9 taps for the base level, 5 for the smoothed copies)
//   k_ak_scharr                    Scharr 3 x 3 (for the conductance), BORDER_REFLECT_101
//   k_ak_gradmax / _gradhist       compute_kcontrast: maximum and 300-bin histogram of the gradient magnitude
//   k_ak_conductance<D>            the conductance of the configured diffusivity: Perona-Malik g1, g2 (the default), Weickert, Charbonnier
//   k_ak_nld_step                  one FED step Lt + step * div(c grad Lt), five-point star, one-sided at the border
//   k_ak_half / k_ak_area          resize INTER_AREA to the next octave (exact halving, or the general table form for odd sizes)
//   k_ak_sep_deriv                 the stretched Scharr pair of compute_derivative_kernels (taps at +-sigma_size)
//   k_ak_det                       determinant of the Hessian x sigma_size^4
//   k_ak_candidates                strict 3 x 3 maxima above the threshold inside the level's border, with their neighbourhood
//   k_ak_orientation               Compute_Main_Orientation, one wave per keypoint (samples, counting sort and window sums in LDS)
//   k_ak_mldb                      the M-LDB descriptor, 32 lanes per keypoint (one per grid cell of the 2x2 + 3x3 + 4x4 grids)
//   k_ak_kcontrast                 compute_kcontrast's last step on the histogram, into the device word the conductance kernels read
//   k_ak_cand_count / _scan / _emit  the same candidates IN ORDER (level by level, row-major): per-workgroup counts, one scan, an ordered scatter
//   k_ak_scan                      one phase of the duplicate suppression, a workgroup per level (uvo_akaze_suppress_dev.h)
//   k_ak_refine                    Do_Subpixel_Refinement per surviving candidate, compacted in candidate order, the count left on the device
// What OpenCV does SEQUENTIALLY -- the row-major scan that suppresses weaker maxima within sigma_size of a stronger one, the two
// sweeps across neighbouring scales (FindKeypointsSameScale, Find_Scale_Space_Extrema), the 2 x 2 sub-pixel solve -- is DEFINED by the
// host scans of uvo_akaze_suppress.h over the candidate list (a few thousand 48-byte records; the planes stay on the device).
// uvo_akaze_set_suppression chooses where it runs: 0 those host scans (three waits of the calling thread per image: histogram, candidate
// count, candidate records), 1 the device form above, which queues without a wait inside the fused steps.  Results do not depend on it.
#include "uvo_ctx.h"
#include "uvo_math.h"
#include "uvo_akaze_suppress.h"
#include "uvo_akaze_plan.h"
#include <float.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <algorithm>

namespace uvo {

double now_us();                                                  // pose.hip / ctx.hip: steady clock, microseconds
static const int kAkMaxLevels = 16, kAkDescBytes = 61, kAkCandCap = 1 << 18;
static const int kAkazeSuppressDefault = 1;                       // uvo_akaze_set_suppression's initial value: the device (124 against 66 stereo pairs/s at depth 6)
struct AkTab { int si; float alpha; };

struct AkazeWs {
    int w = 0, h = 0, n = 0, cap = 0;
    AkazeCfg cfg;                                             // what the plan, the tables and the captured graphs below were made for (uvo_akaze_configure)
    AkLevel lv[kAkMaxLevels];
    float* Lt[kAkMaxLevels] = {nullptr}; float* Lsmooth[kAkMaxLevels] = {nullptr}; float* Lx[kAkMaxLevels] = {nullptr};
    float* Ly[kAkMaxLevels] = {nullptr}; float* Ldet[kAkMaxLevels] = {nullptr};
    float* img = nullptr; float* s[5] = {nullptr};            // full-size scratch planes
    uint8_t* img8 = nullptr;
    int* hist = nullptr;                                      // [0] max bits, [1..300] histogram
    AkCand* cand = nullptr; int* cand_n = nullptr;            // candidates of one level (device), count
    AkCand* h_cand = nullptr; int* h_hist = nullptr;          // pinned
    uvo_keypoint* d_kps = nullptr; uint8_t* d_desc = nullptr; // outputs (cap: max_kpts, grown by the single-image path when a frame has more)
    AkTab* xtab[kAkMaxLevels] = {nullptr}; AkTab* ytab[kAkMaxLevels] = {nullptr}; int* xofs[kAkMaxLevels] = {nullptr}; int* yofs[kAkMaxLevels] = {nullptr};   // general INTER_AREA tables of the octave changes that are not exact halvings (built with the workspace)
    float* d_kc = nullptr; float* h_kc = nullptr;             // compute_kcontrast's result: pinned source, device copy the conductance kernels read
    hipGraph_t graph[2] = {nullptr, nullptr}; hipGraphExec_t exec[2] = {nullptr, nullptr};   // the launch chain from the first evolution step to the last level's candidates, captured once per image size: [0] candidates in atomicAdd order (the host sorts), [1] emitted in order
    AksHost hs;                                               // host: the definition's marks, value planes and per-level candidate lists (uvo_akaze_suppress.h)
    std::vector<uvo_keypoint> out;                            // host: the refined keypoints (source of an asynchronous copy: kept until the next call)
    // ---- the device form (uvo_akaze_set_suppression 1) ----
    AksLevels L;                                              // the plan as the scans read it
    int blk_base[kAkMaxLevels + 1] = {0};                     // ordered emission: the first workgroup of each level's candidate grid; [n] = their number
    int* d_blk = nullptr;                                     // [blk_base[n] + 1] per-workgroup counts, then their exclusive scan
    uint32_t* d_pos = nullptr; float* d_val = nullptr;        // per candidate, in order: (y << 16) | x, the response
    uint8_t* d_mark = nullptr; uint8_t* d_state = nullptr;    // 3 x kAkCandCap marks (one plane per phase), kAkCandCap round states
    int* d_sup = nullptr; int* h_sup = nullptr;               // SUP_* words (h_sup pinned)
    int cand_cap = kAkCandCap;                                // the candidates one image may have (the lists hold kAkCandCap; UVO_AKAZE_CAND_CAP lowers it for tests of the overflow path)
    int stat_ncand = 0, stat_rounds[3] = {0, 0, 0}, stat_waits = 0, stat_dev = 0;    // uvo_akaze_stats: the last detection (stat_dev: the figures are in d_sup)
};
// d_sup: the candidates found (may exceed the list), the candidates listed, the levels' starts in the list, per image slot of a lane the
// keypoint count (what the kernels after the refinement consume: always a count of written keypoints) and, apart from it, the flag "more
// candidates were found than the list holds" (read by k_binary_publish_dev and the host only), the largest round count per phase
enum { SUP_FOUND = 0, SUP_N = 1, SUP_START = 2, SUP_NK = SUP_START + kAkMaxLevels + 1, SUP_OVF = SUP_NK + 2, SUP_ROUNDS = SUP_OVF + 2, SUP_INTS = SUP_ROUNDS + 3 };
static_assert(sizeof(AksKp) == sizeof(uvo_keypoint) && kAksMaxLevels == kAkMaxLevels && kAkPlanMaxLevels == kAkMaxLevels, "AksKp mirrors uvo_keypoint");

// ------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ int ak_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int ak_reflect101(int p, int n) { if (n == 1) return 0; while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; } return p; }

__global__ __launch_bounds__(256) void k_ak_u8_to_f32(const uint8_t* __restrict__ src, int stride, int w, int h, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < w) dst[(size_t)y * w + x] = (float)((double)src[(size_t)y * stride + x] * (1.0 / 255.0));        // convertTo(CV_32F, 1 / 255.)
}
struct AkKernel { float k[16]; int ksize; };
// GaussianBlur rows, BORDER_REPLICATE: 5 taps -> SymmRowSmallFilter (centre, then the mirrored pairs), wider -> the generic RowFilter (left to right)
__global__ __launch_bounds__(256) void k_ak_blur_rows(const float* __restrict__ src, int w, int h, AkKernel kk, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float* s = src + (size_t)y * w;
    const int r = kk.ksize / 2;
    float acc;
    if (kk.ksize <= 5) {
        acc = kk.k[r] * s[x];
        for (int i = 1; i <= r; i++) acc += kk.k[r + i] * (s[ak_clamp(x - i, 0, w - 1)] + s[ak_clamp(x + i, 0, w - 1)]);
    } else {
        acc = kk.k[0] * s[ak_clamp(x - r, 0, w - 1)];
        for (int t = 1; t < kk.ksize; t++) acc += kk.k[t] * s[ak_clamp(x - r + t, 0, w - 1)];
    }
    dst[(size_t)y * w + x] = acc;
}
// columns: SymmColumnFilter (centre, then pairs outward)
__global__ __launch_bounds__(256) void k_ak_blur_cols(const float* __restrict__ src, int w, int h, AkKernel kk, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int r = kk.ksize / 2;
    float acc = kk.k[r] * src[(size_t)y * w + x];
    for (int i = 1; i <= r; i++) acc += kk.k[r + i] * (src[(size_t)ak_clamp(y + i, 0, h - 1) * w + x] + src[(size_t)ak_clamp(y - i, 0, h - 1) * w + x]);
    dst[(size_t)y * w + x] = acc;
}
// Scharr(src, dst, CV_32F, dx, dy, 1, 0, BORDER_DEFAULT): [-1 0 1] along the derivative, [3 10 3] across it; the row pass of the three
// rows a column pass needs is evaluated in place (the same operations as a materialised row pass)
__global__ __launch_bounds__(256) void k_ak_scharr(const float* __restrict__ src, int w, int h, int xorder, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int xm = ak_reflect101(x - 1, w), xp = ak_reflect101(x + 1, w);
    float t[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const float* s = src + (size_t)ak_reflect101(y + q - 1, h) * w;
        const float a = s[xm], b = s[x], c = s[xp];
        t[q] = xorder ? c - a : b * 10.f + (a + c) * 3.f;
    }
    dst[(size_t)y * w + x] = xorder ? (t[0] + t[2]) * 3.f + t[1] * 10.f : t[2] - t[0];
}
// compute_derivative_kernels + sepFilter2D: taps at -r, 0, +r (r = sigma_size; 3 + 2 (r - 1) taps of which three are not zero)
__global__ __launch_bounds__(256) void k_ak_sep_deriv(const float* __restrict__ src, int w, int h, int xorder, int r, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int ksize = 3 + 2 * (r - 1);
    const float ww = 10.0f / 3.0f, nrm = 1.0f / (2.0f * r * (ww + 2.0f)), wn = ww * nrm;
    const int xm = ak_reflect101(x - r, w), xp = ak_reflect101(x + r, w);
    float t[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const float* s = src + (size_t)ak_reflect101(y + (q - 1) * r, h) * w;
        const float a = s[xm], b = s[x], c = s[xp];
        float v;
        if (xorder) v = c - a;
        else if (ksize <= 5) v = wn * b + nrm * (a + c);
        else { v = nrm * a; v += wn * b; v += nrm * c; }
        t[q] = v;
    }
    dst[(size_t)y * w + x] = xorder ? wn * t[1] + nrm * (t[2] + t[0]) : t[2] - t[0];
}
// compute_kcontrast, pass 1: the largest gradient magnitude of the interior (non-negative floats order as their bit patterns)
__global__ __launch_bounds__(256) void k_ak_gradmax(const float* __restrict__ lx, const float* __restrict__ ly, int w, int h, int* __restrict__ hist)
{
    __shared__ float s_m[4];
    const int x = 1 + blockIdx.x * 256 + threadIdx.x;
    float d = 0.f;
    if (x < w - 1)
        for (int y = 1 + blockIdx.y * 16; y < min(h - 1, 1 + (blockIdx.y + 1) * 16); y++) {
            const float a = lx[(size_t)y * w + x], b = ly[(size_t)y * w + x];
            d = fmaxf(d, sqrtf(a * a + b * b));
        }
    for (int o = 32; o > 0; o >>= 1) d = fmaxf(d, __shfl_down(d, o));
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) { d = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3])); if (d > 0.f) atomicMax(&hist[0], __float_as_int(d)); }      // (one atomic per workgroup: 32 000 waves on one address took 206 us)
}
// pass 2: bins (int)(modg * ((nbins - 1) / hmax))
__global__ __launch_bounds__(256) void k_ak_gradhist(const float* __restrict__ lx, const float* __restrict__ ly, int w, int h, int nbins, int* __restrict__ hist)
{
    __shared__ int s_h[512];
    for (int i = threadIdx.x; i < nbins; i += 256) s_h[i] = 0;
    __syncthreads();
    const float hmax = __int_as_float(hist[0]);
    const float sc = (nbins - 1) / hmax;
    const int y = 1 + blockIdx.y;
    for (int x = 1 + blockIdx.x * 1024 + threadIdx.x; x < min(w - 1, 1 + (blockIdx.x + 1) * 1024); x += 256) {
        const float a = lx[(size_t)y * w + x], b = ly[(size_t)y * w + x];
        const float d = sqrtf(a * a + b * b);
        atomicAdd(&s_h[(int)(d * sc)], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += 256) if (s_h[i]) atomicAdd(&hist[1 + i], s_h[i]);
}
// (kcontrast of the frame from device memory -- the launch is part of a captured graph --, x 0.75f once per octave change as
// Create_Nonlinear_Scale_Space does).  One instance per diffusivity of AKAZE::create (nldiffusion_functions.cpp's pm_g1, pm_g2,
// weickert_diffusivity, charbonnier_diffusivity, recalled: DESIGN.md 6), with d = (Lx^2 + Ly^2) / k^2:
//   DIFF_PM_G1 exp(-d) | DIFF_PM_G2 1 / (1 + d) | DIFF_WEICKERT 1 - exp(-3.315 / d^4), 1 where d^4 = 0 | DIFF_CHARBONNIER 1 / sqrt(1 + d)
enum { kAkDiffPmG1 = 0, kAkDiffPmG2 = 1, kAkDiffWeickert = 2, kAkDiffCharbonnier = 3 };
template <int DIFF>
__global__ __launch_bounds__(256) void k_ak_conductance(const float* __restrict__ lx, const float* __restrict__ ly, int n, const float* __restrict__ kc, int octave, float* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float k = *kc;
    for (int o = 0; o < octave; o++) k *= 0.75f;
    const float k2inv = 1.0f / (k * k);
    if constexpr (DIFF == kAkDiffPmG2) dst[i] = 1.0f / (1.0f + ((lx[i] * lx[i] + ly[i] * ly[i]) * k2inv));
    else {
        const float d = (lx[i] * lx[i] + ly[i] * ly[i]) * k2inv;
        if constexpr (DIFF == kAkDiffPmG1) dst[i] = expf(-d);
        else if constexpr (DIFF == kAkDiffCharbonnier) dst[i] = 1.0f / sqrtf(1.0f + d);
        else { const float d2 = d * d, d4 = d2 * d2; dst[i] = d4 > 0.0f ? 1.0f - expf(-3.315f / d4) : 1.0f; }
    }
}
// non_linear_diffusion_step + add: out = Lt + step * div(c grad Lt).  Interior: the five-point star; image border: the one-sided stencil;
// the four corners get a zero step.
__global__ __launch_bounds__(256) void k_ak_nld_step(const float* __restrict__ lt, const float* __restrict__ lf, int w, int h, float step_size, float* __restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (j >= w) return;
    const float* lt_c = lt + (size_t)row * w; const float* lf_c = lf + (size_t)row * w;
    const float c = lt_c[j], f = lf_c[j];
    float step_r;
    const bool top = row == 0, bot = row == h - 1, left = j == 0, right = j == w - 1;
    if ((top || bot) && (left || right)) step_r = 0.0f;
    else if (top || bot) {
        const float* lt_o = top ? lt_c + w : lt_c - w; const float* lf_o = top ? lf_c + w : lf_c - w;
        step_r = (f + lf_c[j + 1]) * (lt_c[j + 1] - c) + (f + lf_c[j - 1]) * (lt_c[j - 1] - c) + (f + lf_o[j]) * (lt_o[j] - c);
    } else if (left) step_r = (f + lf_c[1]) * (lt_c[1] - c) + (f + lf_c[w]) * (lt_c[w] - c) + (f + (lf_c - w)[0]) * ((lt_c - w)[0] - c);
    else if (right) step_r = (f + lf_c[j - 1]) * (lt_c[j - 1] - c) + (f + lf_c[j + w]) * (lt_c[j + w] - c) + (f + lf_c[j - w]) * (lt_c[j - w] - c);
    else step_r = (f + lf_c[j + 1]) * (lt_c[j + 1] - c) + (f + lf_c[j - 1]) * (lt_c[j - 1] - c) + (f + lf_c[j + w]) * (lt_c[j + w] - c) + (f + lf_c[j - w]) * (lt_c[j - w] - c);
    out[(size_t)row * w + j] = c + step_r * step_size;
}
// resize INTER_AREA by exactly two (resizeAreaFast_): (S00 + S01 + S10 + S11) * 0.25f
__global__ __launch_bounds__(256) void k_ak_half(const float* __restrict__ src, int sw, int dw, int dh, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const float* S = src + (size_t)(2 * y) * sw + 2 * x;
    float sum = 0;
    sum += S[0]; sum += S[1]; sum += S[sw]; sum += S[sw + 1];
    dst[(size_t)y * dw + x] = sum * 0.25f;
}
// the general form (resizeArea_): per destination pixel the rows of its y entries in table order, each the sum of its x entries in table order
__global__ __launch_bounds__(256) void k_ak_area(const float* __restrict__ src, int sw, int dw, int dh, const AkTab* __restrict__ xtab, const int* __restrict__ xofs,
                                                 const AkTab* __restrict__ ytab, const int* __restrict__ yofs, float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    float sum = 0.f;
    for (int j = yofs[y]; j < yofs[y + 1]; j++) {
        const float* S = src + (size_t)ytab[j].si * sw;
        float buf = 0.f;
        for (int k = xofs[x]; k < xofs[x + 1]; k++) buf += S[xtab[k].si] * xtab[k].alpha;
        if (j == yofs[y]) sum = ytab[j].alpha * buf; else sum += ytab[j].alpha * buf;
    }
    dst[(size_t)y * dw + x] = sum;
}
__global__ __launch_bounds__(256) void k_ak_det(const float* __restrict__ lxx, const float* __restrict__ lxy, const float* __restrict__ lyy, int n, float sig4, float* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (lxx[i] * lyy[i] - lxy[i] * lxy[i]) * sig4;
}
// FindKeypointsSameScale's parallel half: strict maxima of the 3 x 3 neighbourhood above the threshold inside [border, size - border)
__global__ __launch_bounds__(256) void k_ak_candidates(const float* __restrict__ ldet, int w, int h, int border, float thr, int level, AkCand* __restrict__ out, int* __restrict__ count, int cap)
{
    const int x = border + blockIdx.x * 256 + threadIdx.x, y = border + blockIdx.y;
    if (x >= w - border || y >= h - border) return;
    const float* curr = ldet + (size_t)y * w; const float* prev = curr - w; const float* next = curr + w;
    const float value = curr[x];
    if (value <= thr) return;
    if (value <= curr[x - 1] || value <= curr[x + 1]) return;
    if (value <= prev[x - 1] || value <= prev[x] || value <= prev[x + 1]) return;
    if (value <= next[x - 1] || value <= next[x] || value <= next[x + 1]) return;
    const int slot = atomicAdd(count, 1);
    if (slot >= cap) return;
    AkCand c;
    c.x = x; c.y = y; c.pad = level;
    c.v[0] = prev[x - 1]; c.v[1] = prev[x]; c.v[2] = prev[x + 1]; c.v[3] = curr[x - 1]; c.v[4] = value; c.v[5] = curr[x + 1];
    c.v[6] = next[x - 1]; c.v[7] = next[x]; c.v[8] = next[x + 1];
    out[slot] = c;
}
// ---- the same candidates IN ORDER, level by level and row-major (uvo_akaze_set_suppression 1): every level's candidate grid in one launch,
// workgroup b = 256 consecutive columns of one row of level l (blk_base[l] <= b < blk_base[l + 1]; a level whose border leaves nothing has
// no workgroup), so workgroup order, then thread order, IS the visiting order: count per workgroup, one exclusive scan, ordered scatter ----
struct AkCandPlan { const float* ldet[kAkMaxLevels]; int w[kAkMaxLevels], h[kAkMaxLevels], border[kAkMaxLevels], gx[kAkMaxLevels], blk_base[kAkMaxLevels + 1]; int n; float thr; };
__device__ __forceinline__ bool ak_cand_test(const AkCandPlan& P, int b, int* level, int* xo, int* yo)
{
    int l = 0;
    while (l + 1 < P.n && b >= P.blk_base[l + 1]) l++;
    const int lb = b - P.blk_base[l], border = P.border[l], w = P.w[l], h = P.h[l];
    const int x = border + (lb % P.gx[l]) * 256 + (int)threadIdx.x, y = border + lb / P.gx[l];
    *level = l; *xo = x; *yo = y;
    if (x >= w - border || y >= h - border) return false;
    const float* curr = P.ldet[l] + (size_t)y * w; const float* prev = curr - w; const float* next = curr + w;
    const float value = curr[x];
    if (value <= P.thr) return false;
    if (value <= curr[x - 1] || value <= curr[x + 1]) return false;
    if (value <= prev[x - 1] || value <= prev[x] || value <= prev[x + 1]) return false;
    if (value <= next[x - 1] || value <= next[x] || value <= next[x + 1]) return false;
    return true;
}
__global__ __launch_bounds__(256) void k_ak_cand_count(AkCandPlan P, int* __restrict__ blk)
{
    int l, x, y;
    const int n = __syncthreads_count(ak_cand_test(P, blockIdx.x, &l, &x, &y) ? 1 : 0);
    if (threadIdx.x == 0) blk[blockIdx.x] = n;
}
// one workgroup: blk[0, nblk) -> its exclusive scan, blk[nblk] = the total; the levels' starts, clamped to the list's capacity
__global__ __launch_bounds__(1024) void k_ak_cand_scan(AkCandPlan P, int* blk, int nblk, int cap, int* __restrict__ sup)
{
    __shared__ int s_sum[1024];
    const int t = threadIdx.x, chunk = (nblk + 1023) / 1024, lo = min(t * chunk, nblk), hi = min(lo + chunk, nblk);
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += blk[i];
    s_sum[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                              // inclusive scan of the threads' sums
        const int v = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    int run = s_sum[t] - sum;
    for (int i = lo; i < hi; i++) { const int v = blk[i]; blk[i] = run; run += v; }
    if (t == 1023) blk[nblk] = s_sum[1023];
    __syncthreads();
    const int total = blk[nblk];
    if (t == 0) { sup[SUP_FOUND] = total; sup[SUP_N] = min(total, cap); }
    if (t <= kAkMaxLevels) sup[SUP_START + t] = min(t < P.n ? blk[P.blk_base[t]] : total, cap);
}
__global__ __launch_bounds__(256) void k_ak_cand_emit(AkCandPlan P, const int* __restrict__ blk, AkCand* __restrict__ out, uint32_t* __restrict__ pos, float* __restrict__ val, int cap)
{
    __shared__ int s_w[4];
    int l, x, y;
    const bool is = ak_cand_test(P, blockIdx.x, &l, &x, &y);
    const unsigned long long m = __ballot(is);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_w[wv] = __popcll(m);
    __syncthreads();
    if (!is) return;
    int slot = blk[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < wv; k++) slot += s_w[k];
    if (slot >= cap) return;
    const int w = P.w[l];
    const float* curr = P.ldet[l] + (size_t)y * w; const float* prev = curr - w; const float* next = curr + w;
    AkCand c;
    c.x = x; c.y = y; c.pad = l;
    c.v[0] = prev[x - 1]; c.v[1] = prev[x]; c.v[2] = prev[x + 1]; c.v[3] = curr[x - 1]; c.v[4] = curr[x]; c.v[5] = curr[x + 1];
    c.v[6] = next[x - 1]; c.v[7] = next[x]; c.v[8] = next[x + 1];
    out[slot] = c; pos[slot] = aks_pos(x, y); val[slot] = c.v[4];
}
// compute_kcontrast's last step, where the histogram is
__global__ void k_ak_kcontrast(const int* __restrict__ hist, int total, int nbins, float* __restrict__ kc)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *kc = aks_kcontrast(__int_as_float(hist[0]), hist + 1, total, nbins);
}
// ---- one phase of the duplicate suppression (uvo_akaze_suppress_dev.h): workgroup wg runs the scan of level wg, in rounds; every loop is
// bounded by a list range, and a workgroup waits for nothing but its own barriers.  mark: three planes of kAkCandCap bytes (phase 0, 1, 2);
// a phase reads the scanning level's marks from the previous plane and writes the target level's into its own, which it first fills (zero
// in phase 0, the previous plane's after) -- each level's range of a plane has exactly one writing workgroup. ----
__global__ __launch_bounds__(1024) void k_ak_scan(int phase, AksLevels L, const uint32_t* __restrict__ pos, const float* __restrict__ val, uint8_t* mark, uint8_t* state, int* sup)
{
    __shared__ int s_left;
    const int wg = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    int copy_level;
    const AksScan sc = aks_scan_of(phase, wg, L, &copy_level);
    const int* start = sup + SUP_START;
    const uint8_t* mprev = mark + (size_t)(phase ? phase - 1 : 0) * kAkCandCap;
    uint8_t* mt = mark + (size_t)phase * kAkCandCap;
    if (copy_level >= 0) for (int q = start[copy_level] + tid; q < start[copy_level + 1]; q += nt) mt[q] = mprev[q];
    if (sc.own < 0) return;                                             // (the whole workgroup)
    const int a = start[sc.own], b = start[sc.own + 1], ta = start[sc.tgt], tb = start[sc.tgt + 1];
    const int tw = L.lv[sc.tgt].w, th = L.lv[sc.tgt].h;
    if (tid == 0) s_left = 0;
    __syncthreads();
    int mine = 0;
    if (phase == 0) for (int q = a + tid; q < b; q += nt) { mt[q] = 0; state[q] = AKS_UNDECIDED; mine++; }
    else {
        for (int p = ta + tid; p < tb; p += nt) mt[p] = mprev[p];
        for (int q = a + tid; q < b; q += nt) { const bool act = mprev[q] != 0; state[q] = act ? AKS_UNDECIDED : AKS_DECIDED; mine += act; }
    }
    if (mine) atomicAdd(&s_left, mine);
    __syncthreads();
    int rounds = 0;
    for (int it = 0; it < b - a; ++it) {                                // (each round decides at least the earliest undecided candidate)
        if (s_left == 0) break;                                         // (read by all between two barriers: the same for all)
        for (int q = a + tid; q < b; q += nt) if (state[q] == AKS_UNDECIDED && aks_ready(pos, state, a, q, sc)) state[q] = AKS_READY;     // (READY reads as "not decided" to the others)
        __syncthreads();
        int dec = 0;
        for (int q = a + tid; q < b; q += nt) if (state[q] == AKS_READY) { aks_decide(phase, pos, val, mt, ta, tb, q, sc, tw, th); state[q] = AKS_DECIDED; dec++; }
        if (dec) atomicSub(&s_left, dec);
        __syncthreads();
        rounds++;
    }
    if (tid == 0) atomicMax(&sup[SUP_ROUNDS + phase], rounds);
}
// Do_Subpixel_Refinement per candidate that kept its mark, compacted in candidate order into out[0, cap); the count (also past cap: the
// caller compares) goes to sup[SUP_NK + nk_slot]; sup[SUP_OVF + nk_slot] = more candidates were found than the list (cand_cap) holds
__global__ __launch_bounds__(1024) void k_ak_refine(AksLevels L, const AkCand* __restrict__ cand, const uint8_t* __restrict__ m3, int* sup, uvo_keypoint* __restrict__ out, int cap, int nk_slot, int cand_cap)
{
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = sup[SUP_N];
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < n; q0 += 1024) {
        const int q = q0 + tid;
        bool keep = false;
        AksKp k;
        if (q < n && m3[q] != 0) { const AkCand cd = cand[q]; keep = aks_refine(cd, L.lv[cd.pad], cd.pad, &k); }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_w[wv] = __popcll(m);
        __syncthreads();
        int slot = s_base + __popcll(m & ((1ull << lane) - 1ull)), tot = 0;
        for (int i = 0; i < 16; i++) { if (i < wv) slot += s_w[i]; tot += s_w[i]; }
        if (keep && slot < cap) { uvo_keypoint o; o.x = k.x; o.y = k.y; o.size = k.size; o.angle = k.angle; o.response = k.response; o.octave = k.octave; o.class_id = k.class_id; out[slot] = o; }
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    if (tid == 0) { sup[SUP_NK + nk_slot] = s_base; sup[SUP_OVF + nk_slot] = sup[SUP_FOUND] > cand_cap ? 1 : 0; }
}

__device__ __forceinline__ float ak_atan2_deg(float y, float x)      // cv::fastAtan2 (as surf.hip's fast_atan2_deg)
{
    const float sc = (float)(180 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * sc, p3 = -0.3258083974640975f * sc, p5 = 0.1555786518463281f * sc, p7 = -0.04432655554792128f * sc;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) { c = ay / (ax + (float)DBL_EPSILON); c2 = c * c; a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c; }
    else { c = ax / (ay + (float)DBL_EPSILON); c2 = c * c; a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c; }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}
__device__ const float kGauss25[7][7] = {
    { 0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f },
    { 0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f },
    { 0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f },
    { 0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f },
    { 0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f },
    { 0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f },
    { 0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f } };
struct AkPlanes { const float* Lt[kAkMaxLevels]; const float* Lx[kAkMaxLevels]; const float* Ly[kAkMaxLevels]; int w[kAkMaxLevels], h[kAkMaxLevels]; float ratio[kAkMaxLevels]; };
// Compute_Main_Orientation: 109 Gaussian-weighted derivative samples within 6 scale units, sorted into 42 angular slices (counting
// sort), the 7-slice window with the largest summed vector.  ONE WAVE PER KEYPOINT, everything in LDS (a thread per keypoint kept its
// 109-entry arrays in scratch memory: 3.0 ms for 17 850 keypoints at 1080p): lanes take the samples two at a time; OpenCV's counting
// sort `ang_order[--slice[bin[i]]] = i` puts the members of a slice in DESCENDING sample order, so a sample's place is its slice's start
// plus the number of later samples of the same slice; lane sn sums window sn in that order (a sequential float sum each -- the windows
// are independent); "the first window with the largest norm" is an arg-max with ties to the lower window.  (Windows the reference
// skips because neither end moved hold the previous window's samples, hence its sums: they can never win the strict comparison.)
struct AkOriTab { signed char i[109], j[109]; };
constexpr AkOriTab ak_make_ori_tab()
{
    AkOriTab t{};
    int k = 0;
    for (int i = -6; i <= 6; ++i) for (int j = -6; j <= 6; ++j) if (i * i + j * j < 36) { t.i[k] = (signed char)i; t.j[k] = (signed char)j; ++k; }
    return t;
}
__device__ const AkOriTab kAkOriTab = ak_make_ori_tab();
// (d_n, when given: the count on the device, n its bound -- the grid is sized from n and a workgroup past the count returns at once; only the
// first min(count, n) keypoints were written by k_ak_refine, so nothing else is ever read)
__global__ __launch_bounds__(256) void k_ak_orientation(AkPlanes pl, uvo_keypoint* __restrict__ kps, int n, const int* __restrict__ d_n)
{
    if (d_n) n = min(n, *d_n);
    if ((int)blockIdx.x * 4 >= n) return;
    constexpr int ang_size = 109, slices = 42, win = 7;
    __shared__ float sX[4][ang_size + 3], sY[4][ang_size + 3];
    __shared__ unsigned char sBin[4][ang_size + 3], sOrd[4][ang_size + 3];
    __shared__ int sStart[4][slices + 2];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q_raw = blockIdx.x * 4 + wv;
    const bool live = q_raw < n;
    const int q = live ? q_raw : n - 1;                             // (a ragged tail recomputes the last keypoint and writes nothing)
    const uvo_keypoint kpt = kps[q];
    const int lv = kpt.class_id;
    const float* Lx = pl.Lx[lv]; const float* Ly = pl.Ly[lv];
    const int w = pl.w[lv], h = pl.h[lv];
    const float ratio = pl.ratio[lv];
    const int scale = cv_round_f(0.5f * kpt.size / ratio), x0 = cv_round_f(kpt.x / ratio), y0 = cv_round_f(kpt.y / ratio);
    const float ang_step = (float)(2.0 * 3.14159265358979323846 / slices);
    for (int k = lane; k < ang_size; k += 64) {
        const int i = kAkOriTab.i[k], j = kAkOriTab.j[k];
        const float wgt = kGauss25[i < 0 ? -i : i][j < 0 ? -j : j];
        const int y = ak_clamp(y0 + i * scale, 0, h - 1), x = ak_clamp(x0 + j * scale, 0, w - 1);
        const float rx = wgt * Lx[(size_t)y * w + x], ry = wgt * Ly[(size_t)y * w + x];
        const float ang = ak_atan2_deg(ry, rx) * (float)(3.14159265358979323846 / 180.0);
        int b = (int)(ang / ang_step);
        if (b < 0 || b >= slices) b = 0;
        sX[wv][k] = rx; sY[wv][k] = ry; sBin[wv][k] = (unsigned char)b;
    }
    __syncthreads();
    if (lane <= slices) {                                           // start of slice `lane` = the samples in lower slices; sStart[42] = 109
        int c = 0;
        for (int k = 0; k < ang_size; k++) c += sBin[wv][k] < lane;
        sStart[wv][lane] = c;
    }
    __syncthreads();
    for (int k = lane; k < ang_size; k += 64) {
        const int b = sBin[wv][k];
        int later = 0;
        for (int k2 = k + 1; k2 < ang_size; k2++) later += sBin[wv][k2] == b;
        sOrd[wv][sStart[wv][b] + later] = (unsigned char)k;
    }
    __syncthreads();
    float sumX = 0.0f, sumY = 0.0f, norm = -1.0f;
    if (lane < slices) {
        const int* st = sStart[wv];
        if (lane <= slices - win) { for (int i = st[lane]; i < st[lane + win]; i++) { const int idx = sOrd[wv][i]; sumX += sX[wv][idx]; sumY += sY[wv][idx]; } }
        else {
            const int remain = lane + win - slices;
            for (int i = st[lane]; i < st[slices]; i++) { const int idx = sOrd[wv][i]; sumX += sX[wv][idx]; sumY += sY[wv][idx]; }
            for (int i = st[0]; i < st[remain]; i++) { const int idx = sOrd[wv][i]; sumX += sX[wv][idx]; sumY += sY[wv][idx]; }
        }
        norm = sumX * sumX + sumY * sumY;
    }
    int best = lane;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float on = __shfl_xor(norm, d); const int ob = __shfl_xor(best, d);
        if (on > norm || (on == norm && ob < best)) { norm = on; best = ob; }
    }
    const float maxX = __shfl(sumX, best), maxY = __shfl(sumY, best);
    if (live && lane == 0) kps[q].angle = ak_atan2_deg(maxY, maxX);
}
// MLDB_Full_Descriptor_Invoker: grids of 2 x 2, 3 x 3 and 4 x 4 cells over the rotated 20 x 20-sample pattern (cell sides 10, 7, 5 samples),
// per cell the means of Lt and of the rotated derivatives; every pair of cells of a grid compared channel by channel: 3 (6 + 36 + 120) =
// 486 bits.  Lane c of the keypoint's 32 owns cell c (0..3 | 4..12 | 13..28) and sums its samples in OpenCV's order; lane 0 packs.
// (d_n as k_ak_orientation's; rows of `stride` bytes, zero past the 61)
__global__ __launch_bounds__(256) void k_ak_mldb(AkPlanes pl, const uvo_keypoint* __restrict__ kps, int n, const int* __restrict__ d_n, uint8_t* __restrict__ desc, int stride)
{
    if (d_n) n = min(n, *d_n);
    if ((int)blockIdx.x * 8 >= n) return;
    __shared__ int s_val[8][29 * 3];
    const int g = threadIdx.x >> 5, lane = threadIdx.x & 31, q = blockIdx.x * 8 + g;
    if (q < n && lane < 29) {
        const uvo_keypoint kpt = kps[q];
        const int lv = kpt.class_id;
        const float* Lt = pl.Lt[lv]; const float* Lx = pl.Lx[lv]; const float* Ly = pl.Ly[lv];
        const int w = pl.w[lv], h = pl.h[lv];
        const float ratio = pl.ratio[lv];
        const float scale = (float)cv_round_f(0.5f * kpt.size / ratio);
        const float xf = kpt.x / ratio, yf = kpt.y / ratio;
        const float angle = (kpt.angle * (float)3.14159265358979323846) / 180.f;
        double sd, cd;
        det_sincos((double)angle, &sd, &cd);
        const float co = (float)cd, si = (float)sd;
        const int grid = lane < 4 ? 0 : (lane < 13 ? 1 : 2), cell = lane - (grid == 0 ? 0 : (grid == 1 ? 4 : 13));
        const int side = grid + 2, sample_step = grid == 0 ? 10 : (grid == 1 ? 7 : 5);          // ceil(10 * {1, 2/3, 1/2})
        const int i0 = -10 + (cell / side) * sample_step, j0 = -10 + (cell % side) * sample_step;
        float di = 0.0f, dx = 0.0f, dy = 0.0f;
        int nsamples = 0;
        for (int k = i0; k < i0 + sample_step; k++)
            for (int l = j0; l < j0 + sample_step; l++) {
                const float sample_y = yf + (l * co * scale + k * si * scale);
                const float sample_x = xf + (-l * si * scale + k * co * scale);
                const int y1 = ak_clamp(cv_round_f(sample_y), 0, h - 1), x1 = ak_clamp(cv_round_f(sample_x), 0, w - 1);
                const float ri = Lt[(size_t)y1 * w + x1];
                di += ri;
                const float rx = Lx[(size_t)y1 * w + x1], ry = Ly[(size_t)y1 * w + x1];
                const float rry = rx * co + ry * si, rrx = -rx * si + ry * co;
                dx += rrx; dy += rry;
                nsamples++;
            }
        di /= nsamples; dx /= nsamples; dy /= nsamples;
        const int a = __float_as_int(di), b = __float_as_int(dx), c = __float_as_int(dy);
        s_val[g][lane * 3] = a ^ ((a < 0) ? 0x7fffffff : 0);                                   // CV_TOGGLE_FLT
        s_val[g][lane * 3 + 1] = b ^ ((b < 0) ? 0x7fffffff : 0);
        s_val[g][lane * 3 + 2] = c ^ ((c < 0) ? 0x7fffffff : 0);
    }
    __syncthreads();
    if (q < n && lane == 0) {
        uint8_t d[kAkDescBytes];
        for (int i = 0; i < kAkDescBytes; i++) d[i] = 0;
        int dpos = 0;
        const int first[3] = { 0, 4, 13 };
        for (int lvl = 0; lvl < 3; lvl++) {
            const int val_count = (lvl + 2) * (lvl + 2);
            const int* iv = &s_val[g][first[lvl] * 3];
            for (int pos = 0; pos < 3; pos++)
                for (int i = 0; i < val_count; i++) {
                    const int ival = iv[3 * i + pos];
                    for (int j = i + 1; j < val_count; j++) { d[dpos >> 3] |= (uint8_t)((ival > iv[3 * j + pos]) << (dpos & 7)); dpos++; }
                }
        }
        for (int i = 0; i < kAkDescBytes; i++) desc[(size_t)q * stride + i] = d[i];
        for (int i = kAkDescBytes; i < stride; i++) desc[(size_t)q * stride + i] = 0;
    }
}

// ------------------------------------------------------------------------------------------ host
void akaze_ws_free(Ctx* c)
{
    AkazeWs* s = static_cast<AkazeWs*>(c->akaze_ws);
    if (!s) return;
    for (int i = 0; i < kAkMaxLevels; i++) { (void)hipFree(s->Lt[i]); (void)hipFree(s->Lsmooth[i]); (void)hipFree(s->Lx[i]); (void)hipFree(s->Ly[i]); (void)hipFree(s->Ldet[i]); }
    for (float* p : s->s) (void)hipFree(p);
    (void)hipFree(s->img); (void)hipFree(s->img8); (void)hipFree(s->hist); (void)hipFree(s->cand); (void)hipFree(s->cand_n); (void)hipFree(s->d_kps); (void)hipFree(s->d_desc);
    for (int i = 0; i < kAkMaxLevels; i++) { (void)hipFree(s->xtab[i]); (void)hipFree(s->ytab[i]); (void)hipFree(s->xofs[i]); (void)hipFree(s->yofs[i]); }
    for (int g = 0; g < 2; g++) { if (s->exec[g]) (void)hipGraphExecDestroy(s->exec[g]); if (s->graph[g]) (void)hipGraphDestroy(s->graph[g]); }
    (void)hipFree(s->d_blk); (void)hipFree(s->d_pos); (void)hipFree(s->d_val); (void)hipFree(s->d_mark); (void)hipFree(s->d_state); (void)hipFree(s->d_sup); (void)hipHostFree(s->h_sup);
    (void)hipFree(s->d_kc); (void)hipHostFree(s->h_kc);
    (void)hipHostFree(s->h_cand); (void)hipHostFree(s->h_hist);
    delete s;
    c->akaze_ws = nullptr;
}
static void area_tab(int ssize, int dsize, double scale, std::vector<AkTab>* tab, std::vector<int>* ofs);
static AkazeWs* akaze_ws(Ctx* c, int w, int h)
{
    AkazeWs* s = static_cast<AkazeWs*>(c->akaze_ws);
    const AkazeCfg cfg = c->sh->lanes[0]->akaze_cfg;                // the master context's configuration serves every lane
    if (s && s->w == w && s->h == h && s->cfg == cfg) return s;
    akaze_ws_free(c);
    s = new AkazeWs();
    c->akaze_ws = s;
    s->w = w; s->h = h; s->cap = c->cap; s->cfg = cfg;
    s->n = akaze_plan(w, h, cfg.n_octaves, cfg.n_octave_layers, s->lv);
    if (s->n < 1) {                                                 // (uvo_akaze_configure serves at most 4 x 4: 16 levels, cycles of at most 31 steps)
        c->err = s->n == AK_PLAN_CYCLE_TOO_LONG ? "AKAZE: a FED cycle of the level plan has more steps than a level holds (64)" : "AKAZE: the level plan has more levels than the tables hold (16)";
        akaze_ws_free(c);
        return nullptr;
    }
    if (const char* e = getenv("UVO_AKAZE_CAND_CAP")) s->cand_cap = std::min(std::max(atoi(e), 1), kAkCandCap);      // (read per workspace: tools/probe/README.md)
    bool ok = true;
    auto alloc = [&](float** p, size_t n) { ok = ok && hipMalloc(reinterpret_cast<void**>(p), sizeof(float) * n) == hipSuccess; };
    const size_t npx = (size_t)w * h;
    for (int i = 0; i < s->n; i++) {
        const size_t n = (size_t)s->lv[i].w * s->lv[i].h;
        alloc(&s->Lt[i], n); alloc(&s->Lsmooth[i], n); alloc(&s->Lx[i], n); alloc(&s->Ly[i], n); alloc(&s->Ldet[i], n);
    }
    for (int i = 0; i < s->n; i++) {                                // the plan as the scans read it; the candidate grids of the ordered emission
        const AkLevel& lv = s->lv[i];
        s->L.lv[i] = AksLevel{ lv.w, lv.h, lv.sigma_size, lv.octave, lv.octave_ratio, lv.esigma };
        const bool none = lv.border + 1 >= lv.h || lv.w - 2 * lv.border <= 0 || lv.h - 2 * lv.border <= 0;
        s->blk_base[i + 1] = s->blk_base[i] + (none ? 0 : ((lv.w - 2 * lv.border + 255) / 256) * (lv.h - 2 * lv.border));
    }
    s->L.n = s->n;
    aks_host_init(&s->hs, s->L);
    alloc(&s->img, npx);
    for (float*& p : s->s) alloc(&p, npx);
    ok = ok && hipMalloc(reinterpret_cast<void**>(&s->img8), npx) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->hist), sizeof(int) * 512) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->cand), sizeof(AkCand) * kAkCandCap) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->cand_n), sizeof(int) * kAkMaxLevels) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_kps), sizeof(uvo_keypoint) * (size_t)s->cap) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->d_desc), (size_t)kAkDescBytes * s->cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_kc), sizeof(float)) == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(&s->h_kc), sizeof(float)) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&s->h_cand), sizeof(AkCand) * kAkCandCap) == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(&s->h_hist), sizeof(int) * 512) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_blk), sizeof(int) * ((size_t)s->blk_base[s->n] + 1)) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->d_pos), sizeof(uint32_t) * kAkCandCap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_val), sizeof(float) * kAkCandCap) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->d_mark), (size_t)3 * kAkCandCap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_state), (size_t)kAkCandCap) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->d_sup), sizeof(int) * SUP_INTS) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&s->h_sup), sizeof(int) * SUP_INTS) == hipSuccess && hipMemset(s->d_sup, 0, sizeof(int) * SUP_INTS) == hipSuccess;
    // resize(Lt[i - 1], Lt[i], INTER_AREA) at an octave change: exact halving has a kernel of its own; other size ratios (odd sizes) take
    // resizeArea_'s tables, which depend on the sizes alone
    for (int i = 1; i < s->n && ok; i++) {
        if (!(s->lv[i].octave > s->lv[i - 1].octave)) continue;
        const int lw = s->lv[i].w, lh = s->lv[i].h, sw = s->lv[i - 1].w, sh = s->lv[i - 1].h;
        const double scale_x = 1. / ((double)lw / sw), scale_y = 1. / ((double)lh / sh);
        const int isx = cv_round_d(scale_x), isy = cv_round_d(scale_y);
        if (fabs(scale_x - isx) < DBL_EPSILON && fabs(scale_y - isy) < DBL_EPSILON && isx == 2 && isy == 2) continue;
        std::vector<AkTab> xt, yt; std::vector<int> xo, yo;
        area_tab(sw, lw, scale_x, &xt, &xo); area_tab(sh, lh, scale_y, &yt, &yo);
        ok = hipMalloc(reinterpret_cast<void**>(&s->xtab[i]), sizeof(AkTab) * (xt.size() + 1)) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->ytab[i]), sizeof(AkTab) * (yt.size() + 1)) == hipSuccess &&
             hipMalloc(reinterpret_cast<void**>(&s->xofs[i]), sizeof(int) * xo.size()) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&s->yofs[i]), sizeof(int) * yo.size()) == hipSuccess &&
             hipMemcpy(s->xtab[i], xt.data(), sizeof(AkTab) * xt.size(), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->ytab[i], yt.data(), sizeof(AkTab) * yt.size(), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(s->xofs[i], xo.data(), sizeof(int) * xo.size(), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->yofs[i], yo.data(), sizeof(int) * yo.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { akaze_ws_free(c); c->err = "AKAZE workspace allocation failed"; return nullptr; }
    return s;
}
static void gauss_kernel(int n, double sigma, AkKernel* kk)       // getGaussianKernel(n, sigma, CV_32F): double, normalised, cast
{
    double t[16], sum = 0;
    const double scale2X = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; t[i] = exp(scale2X * x * x); sum += t[i]; }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) kk->k[i] = (float)(t[i] * sum);
    kk->ksize = n;
}
// computeResizeAreaTab (resize.cpp) of one axis -> (si, alpha) entries grouped by destination index, ofs[d] .. ofs[d + 1]
static void area_tab(int ssize, int dsize, double scale, std::vector<AkTab>* tab, std::vector<int>* ofs)
{
    tab->clear(); ofs->assign(dsize + 1, 0);
    for (int dx = 0; dx < dsize; dx++) {
        (*ofs)[dx] = (int)tab->size();
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cellWidth = std::min(scale, ssize - fsx1);
        int sx1 = cv_ceil_d(fsx1), sx2 = cv_floor_d(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) tab->push_back(AkTab{ sx1 - 1, (float)((sx1 - fsx1) / cellWidth) });
        for (int sx = sx1; sx < sx2; sx++) tab->push_back(AkTab{ sx, (float)(1.0 / cellWidth) });
        if (fsx2 - sx2 > 1e-3) tab->push_back(AkTab{ sx2, (float)(std::min(std::min(fsx2 - sx2, 1.), cellWidth) / cellWidth) });
    }
    (*ofs)[dsize] = (int)tab->size();
}
// ordered: the candidates by k_ak_cand_count / _scan / _emit (in visiting order, with pos and val) instead of k_ak_candidates' atomicAdd order
static uvo_status akaze_record(Ctx* c, AkazeWs* s, hipStream_t st, bool ordered)
{
    const dim3 blk(256);
    auto grid = [](int ww, int hh) { return dim3((ww + 255) / 256, hh); };
    AkKernel k5;
    gauss_kernel(5, (double)1.0f, &k5);
    const int diff = s->cfg.diffusivity;
    auto k_cond = diff == kAkDiffPmG1 ? k_ak_conductance<kAkDiffPmG1> : diff == kAkDiffWeickert ? k_ak_conductance<kAkDiffWeickert> : diff == kAkDiffCharbonnier ? k_ak_conductance<kAkDiffCharbonnier> : k_ak_conductance<kAkDiffPmG2>;
    for (int i = 1; i < s->n; i++) {
        const AkLevel& lv = s->lv[i];
        const int lw = lv.w, lh = lv.h;
        if (lv.octave > s->lv[i - 1].octave) {
            const int sw = s->lv[i - 1].w;
            if (!s->xtab[i]) hipLaunchKernelGGL(k_ak_half, grid(lw, lh), blk, 0, st, s->Lt[i - 1], sw, lw, lh, s->Lt[i]);
            else hipLaunchKernelGGL(k_ak_area, grid(lw, lh), blk, 0, st, s->Lt[i - 1], sw, lw, lh, s->xtab[i], s->xofs[i], s->ytab[i], s->yofs[i], s->Lt[i]);
        } else UVO_HIP_TRY(c, hipMemcpyAsync(s->Lt[i], s->Lt[i - 1], sizeof(float) * (size_t)lw * lh, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_ak_blur_rows, grid(lw, lh), blk, 0, st, s->Lt[i], lw, lh, k5, s->s[0]);
        hipLaunchKernelGGL(k_ak_blur_cols, grid(lw, lh), blk, 0, st, s->s[0], lw, lh, k5, s->Lsmooth[i]);
        hipLaunchKernelGGL(k_ak_scharr, grid(lw, lh), blk, 0, st, s->Lsmooth[i], lw, lh, 1, s->s[0]);
        hipLaunchKernelGGL(k_ak_scharr, grid(lw, lh), blk, 0, st, s->Lsmooth[i], lw, lh, 0, s->s[1]);
        hipLaunchKernelGGL(k_cond, dim3((lw * lh + 255) / 256), blk, 0, st, s->s[0], s->s[1], lw * lh, s->d_kc, lv.octave, s->s[2]);
        // Fast Explicit Diffusion: the cycle's steps, ping-pong between Lt[i] and a scratch plane
        float* cur = s->Lt[i]; float* nxt = s->s[3];
        for (int j = 0; j < lv.nsteps; j++) {
            hipLaunchKernelGGL(k_ak_nld_step, grid(lw, lh), blk, 0, st, cur, s->s[2], lw, lh, lv.tau[j] * 0.5f, nxt);
            std::swap(cur, nxt);
        }
        if (cur != s->Lt[i]) UVO_HIP_TRY(c, hipMemcpyAsync(s->Lt[i], cur, sizeof(float) * (size_t)lw * lh, hipMemcpyDeviceToDevice, st));
    }
    if (!ordered) UVO_HIP_TRY(c, hipMemsetAsync(s->cand_n, 0, sizeof(int) * kAkMaxLevels, st));
    for (int i = 0; i < s->n; i++) {
        const AkLevel& lv = s->lv[i];
        const int lw = lv.w, lh = lv.h, r = lv.sigma_size;
        hipLaunchKernelGGL(k_ak_sep_deriv, grid(lw, lh), blk, 0, st, s->Lsmooth[i], lw, lh, 1, r, s->Lx[i]);
        hipLaunchKernelGGL(k_ak_sep_deriv, grid(lw, lh), blk, 0, st, s->Lx[i], lw, lh, 1, r, s->s[0]);        // Lxx
        hipLaunchKernelGGL(k_ak_sep_deriv, grid(lw, lh), blk, 0, st, s->Lx[i], lw, lh, 0, r, s->s[1]);        // Lxy
        hipLaunchKernelGGL(k_ak_sep_deriv, grid(lw, lh), blk, 0, st, s->Lsmooth[i], lw, lh, 0, r, s->Ly[i]);
        hipLaunchKernelGGL(k_ak_sep_deriv, grid(lw, lh), blk, 0, st, s->Ly[i], lw, lh, 0, r, s->s[2]);        // Lyy
        hipLaunchKernelGGL(k_ak_det, dim3((lw * lh + 255) / 256), blk, 0, st, s->s[0], s->s[1], s->s[2], lw * lh, (float)(r * r * r * r), s->Ldet[i]);
        if (ordered || lv.border + 1 >= lh || lw - 2 * lv.border <= 0 || lh - 2 * lv.border <= 0) continue;   // "if border is too big we shouldn't search any keypoints"
        // every level appends to one list (the record carries its level); cand_n[0] counts them all
        hipLaunchKernelGGL(k_ak_candidates, grid(lw - 2 * lv.border, lh - 2 * lv.border), blk, 0, st, s->Ldet[i], lw, lh, lv.border, s->cfg.threshold, i, s->cand, s->cand_n, s->cand_cap);
    }
    if (ordered) {
        AkCandPlan P;
        memset(&P, 0, sizeof(P));
        for (int i = 0; i < s->n; i++) { P.ldet[i] = s->Ldet[i]; P.w[i] = s->lv[i].w; P.h[i] = s->lv[i].h; P.border[i] = s->lv[i].border; P.gx[i] = std::max(1, (s->lv[i].w - 2 * s->lv[i].border + 255) / 256); }
        for (int i = 0; i <= s->n; i++) P.blk_base[i] = s->blk_base[i];
        P.n = s->n; P.thr = s->cfg.threshold;
        const int nblk = s->blk_base[s->n];
        if (nblk > 0) hipLaunchKernelGGL(k_ak_cand_count, dim3(nblk), blk, 0, st, P, s->d_blk);
        hipLaunchKernelGGL(k_ak_cand_scan, dim3(1), dim3(1024), 0, st, P, s->d_blk, nblk, s->cand_cap, s->d_sup);
        if (nblk > 0) hipLaunchKernelGGL(k_ak_cand_emit, dim3(nblk), blk, 0, st, P, s->d_blk, s->cand, s->d_pos, s->d_val, s->cand_cap);
    }
    return UVO_OK;
}
static bool akaze_use_graph()
{
    static const bool on = !(getenv("UVO_AKAZE_GRAPH") && atoi(getenv("UVO_AKAZE_GRAPH")) == 0);      // UVO_AKAZE_GRAPH=0: launch by launch (measurement)
    return on;
}
// the chain captured on stream st (thread-local capture mode) and instantiated, once per workspace
static uvo_status akaze_capture(Ctx* c, AkazeWs* s, hipStream_t st, int ordered)
{
    if (s->exec[ordered]) return UVO_OK;
    UVO_HIP_TRY(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const uvo_status rs = akaze_record(c, s, st, ordered != 0);
    hipGraph_t g = nullptr;
    const hipError_t ee = hipStreamEndCapture(st, &g);
    if (rs != UVO_OK || ee != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); if (rs == UVO_OK) c->err = std::string("AKAZE: graph capture: ") + hipGetErrorString(ee); return rs != UVO_OK ? rs : UVO_HIP_ERROR; }
    s->graph[ordered] = g;
    UVO_HIP_TRY(c, hipGraphInstantiate(&s->exec[ordered], s->graph[ordered], nullptr, nullptr, 0));
    return UVO_OK;
}

// the three scans and the refinement on the ordered list in s->cand / d_pos / d_val with d_sup[SUP_N, SUP_START ..] (left by the ordered
// emission, or uploaded by the test hook): keypoints to dst[0, cap), their count to d_sup[SUP_NK + nk_slot].  Five launches, no wait.
static uvo_status akaze_suppress_launch(Ctx* c, AkazeWs* s, hipStream_t st, uvo_keypoint* dst, int cap, int nk_slot, bool scans = true)
{
    if (scans) {
        UVO_HIP_TRY(c, hipMemsetAsync(s->d_sup + SUP_ROUNDS, 0, sizeof(int) * 3, st));
        for (int ph = 0; ph < 3; ph++) hipLaunchKernelGGL(k_ak_scan, dim3(s->n), dim3(1024), 0, st, ph, s->L, s->d_pos, s->d_val, s->d_mark, s->d_state, s->d_sup);
    }
    hipLaunchKernelGGL(k_ak_refine, dim3(1), dim3(1024), 0, st, s->L, s->cand, s->d_mark + (size_t)2 * kAkCandCap, s->d_sup, dst, cap, nk_slot, s->cand_cap);
    UVO_HIP_TRY(c, hipGetLastError());
    return UVO_OK;
}
// the definition on a candidate list in any order: the host scans of uvo_akaze_suppress.h; marks (n x 3, or null): each candidate's mark after each phase
static void akaze_suppress_host(AkazeWs* s, const AkCand* list, int n_cand, uint8_t* marks)
{
    aks_host_order(&s->hs, list, n_cand);
    aks_host_within(&s->hs);
    if (marks) aks_host_marks(&s->hs, list, n_cand, marks, 3);
    aks_host_sweep_lower(&s->hs);
    if (marks) aks_host_marks(&s->hs, list, n_cand, marks + 1, 3);
    aks_host_sweep_upper(&s->hs);
    if (marks) aks_host_marks(&s->hs, list, n_cand, marks + 2, 3);
    aks_host_refine(&s->hs, &s->out);
}

// where a lane's detection leaves its results under suppression setting 1: the lane's keypoints and 64-byte rows, written straight from the kernels
struct AkLaneOut { uvo_keypoint* kps; uint8_t* rows; int cap, slot; };
// detectAndCompute on `gray` (device or host), *n_out = the count.
//   where = 0 (the host scans): the keypoints and their M-LDB rows are left in s->d_kps / s->d_desc.  When the count exceeds the workspace's
//     capacity, `grow` reallocates the two output buffers to hold it (the single-image operator: AKAZE has no upper bound on its count --
//     17 850 on a 1080p frame); without it nothing past the host stages is computed and the call still returns UVO_OK (the fused steps,
//     whose lane buffers max_kpts sizes).  Three waits.
//   where = 1 (the device form), lane = null: the same outputs and contract, ONE wait (the count, which sizes the output buffers).
//   where = 1, lane given: everything is queued and nothing waited for; the keypoints and padded rows go to the lane's buffers, the count stays in
//     d_sup[SUP_NK + lane->slot] (possibly past lane->cap) and a candidate overflow raises d_sup[SUP_OVF + lane->slot]: nothing is written
//     past either list, and the step's count readback reports UVO_CAPACITY for either, each by its name; *n_out = -1.
static uvo_status akaze_run(Ctx* c, AkazeWs* s, hipStream_t st, const uint8_t* gray, int w, int h, int stride, int mem, bool grow, int where, const AkLaneOut* lane, int* n_out)
{
    *n_out = 0;
    const dim3 blk(256);
    auto grid = [](int ww, int hh) { return dim3((ww + 255) / 256, hh); };
    static const bool dbg = getenv("UVO_DBG_PHASE") != nullptr;                                            // host wall clock of the call's phases
    double tph[8] = {0}; int nph = 0, waits = 0;
    auto stamp = [&]() { if (dbg && nph < 8) tph[nph++] = uvo::now_us(); };     // (at the call's own waits only: the device form has one, for the count, and none inside a fused step)
    auto wait = [&]() { waits++; return hipStreamSynchronize(st); };
    if (where == 1 && (w > 65535 || h > 65535)) { c->err = "AKAZE: the device suppression packs positions into 16 bits a side"; return UVO_INVALID_ARG; }
    stamp();
    // ---- Create_Nonlinear_Scale_Space ----
    const uint8_t* d_img8 = gray;
    int d_stride = stride;
    if (mem != UVO_MEM_DEVICE) {
        UVO_HIP_TRY(c, hipMemcpy2DAsync(s->img8, w, gray, stride, w, h, hipMemcpyHostToDevice, st));
        d_img8 = s->img8; d_stride = w;
    }
    hipLaunchKernelGGL(k_ak_u8_to_f32, grid(w, h), blk, 0, st, d_img8, d_stride, w, h, s->img);
    AkKernel k9, k5;
    { int ks = cv_ceil_d((double)(2.0f * (1.0f + (1.6f - 0.8f) / (0.3f)))); ks |= 1; gauss_kernel(ks, (double)1.6f, &k9); }
    gauss_kernel(5, (double)1.0f, &k5);
    aks_host_clear(&s->hs);
    hipLaunchKernelGGL(k_ak_blur_rows, grid(w, h), blk, 0, st, s->img, w, h, k9, s->s[0]);
    hipLaunchKernelGGL(k_ak_blur_cols, grid(w, h), blk, 0, st, s->s[0], w, h, k9, s->Lsmooth[0]);
    UVO_HIP_TRY(c, hipMemcpyAsync(s->Lt[0], s->Lsmooth[0], sizeof(float) * (size_t)w * h, hipMemcpyDeviceToDevice, st));
    float kcontrast = 0.f;
    bool kc_on_device = false;
    if (s->n > 1) {                                                  // compute_kcontrast on the image blurred with sigma 1
        hipLaunchKernelGGL(k_ak_blur_rows, grid(w, h), blk, 0, st, s->img, w, h, k5, s->s[0]);
        hipLaunchKernelGGL(k_ak_blur_cols, grid(w, h), blk, 0, st, s->s[0], w, h, k5, s->s[1]);
        hipLaunchKernelGGL(k_ak_scharr, grid(w, h), blk, 0, st, s->s[1], w, h, 1, s->s[2]);
        hipLaunchKernelGGL(k_ak_scharr, grid(w, h), blk, 0, st, s->s[1], w, h, 0, s->s[3]);
        const int nbins = 300;
        UVO_HIP_TRY(c, hipMemsetAsync(s->hist, 0, sizeof(int) * 512, st));
        if (w > 2 && h > 2) {
            hipLaunchKernelGGL(k_ak_gradmax, dim3((w - 2 + 255) / 256, (h - 2 + 15) / 16), blk, 0, st, s->s[2], s->s[3], w, h, s->hist);
            hipLaunchKernelGGL(k_ak_gradhist, dim3((w - 2 + 1023) / 1024, h - 2), blk, 0, st, s->s[2], s->s[3], w, h, nbins, s->hist);
        }
        const int total = (w - 2) * (h - 2);
        if (where == 1) { hipLaunchKernelGGL(k_ak_kcontrast, dim3(1), dim3(64), 0, st, s->hist, total, nbins, s->d_kc); kc_on_device = true; }
        else {
            UVO_HIP_TRY(c, hipMemcpyAsync(s->h_hist, s->hist, sizeof(int) * 512, hipMemcpyDeviceToHost, st));
            UVO_HIP_TRY(c, wait());
            float hmax; memcpy(&hmax, &s->h_hist[0], 4);
            kcontrast = aks_kcontrast(hmax, s->h_hist + 1, total, nbins);
        }
    }
    stamp();
    if (!kc_on_device) {
        *s->h_kc = kcontrast;
        UVO_HIP_TRY(c, hipMemcpyAsync(s->d_kc, s->h_kc, sizeof(float), hipMemcpyHostToDevice, st));
    }
    // ---- the evolution (levels 1 ..), Compute_Determinant_Hessian_Response and the candidates of every level: ~600 small launches (166 FED
    // steps, 80 derivative passes at 1080p) whose arguments depend on the image SIZE only -- captured once per workspace as a HIP graph
    // and replayed with one call per frame.  Measured: the chain is bound by the DEVICE (600 kernels of 3-6 us back to back: 3.2 ms at
    // 1080p either way; whole call 1.46 ms as a graph against 1.56 ms launch by launch at 640 x 360, level at 1080p); what the graph
    // buys is the host thread, idle instead of issuing launches for 3 ms. ----
    if (akaze_use_graph()) {
        UVO_TRY(akaze_capture(c, s, st, where));
        UVO_HIP_TRY(c, hipGraphLaunch(s->exec[where], st));
    } else UVO_TRY(akaze_record(c, s, st, where == 1));
    AkPlanes pl;
    memset(&pl, 0, sizeof(pl));
    for (int i = 0; i < s->n; i++) { pl.Lt[i] = s->Lt[i]; pl.Lx[i] = s->Lx[i]; pl.Ly[i] = s->Ly[i]; pl.w[i] = s->lv[i].w; pl.h[i] = s->lv[i].h; pl.ratio[i] = s->lv[i].octave_ratio; }
    s->stat_dev = where;
    int n_cand = 0, n = 0;
    if (where == 1 && lane) {
        // ---- the fused steps: suppression, refinement, orientation and M-LDB by counts read on the device (grids from the lane's capacity) ----
        const int* d_n = s->d_sup + SUP_NK + lane->slot;
        UVO_TRY(akaze_suppress_launch(c, s, st, lane->kps, lane->cap, lane->slot));
        hipLaunchKernelGGL(k_ak_orientation, dim3((lane->cap + 3) / 4), dim3(256), 0, st, pl, lane->kps, lane->cap, d_n);
        hipLaunchKernelGGL(k_ak_mldb, dim3((lane->cap + 7) / 8), dim3(256), 0, st, pl, lane->kps, lane->cap, d_n, lane->rows, 4 * kBinRowWords);
        UVO_HIP_TRY(c, hipGetLastError());
        s->stat_waits = waits;
        *n_out = -1;
        return UVO_OK;
    }
    if (where == 1) {
        UVO_TRY(akaze_suppress_launch(c, s, st, s->d_kps, s->cap, 0));
        UVO_HIP_TRY(c, hipMemcpyAsync(s->h_sup, s->d_sup, sizeof(int) * SUP_INTS, hipMemcpyDeviceToHost, st));
        UVO_HIP_TRY(c, wait());
        n_cand = s->h_sup[SUP_FOUND];
        s->stat_ncand = n_cand; s->stat_waits = waits;
        if (n_cand > s->cand_cap) { c->err = kAkazeCandOverflow; return UVO_CAPACITY; }
        n = s->h_sup[SUP_NK];
        stamp();
    } else {
        UVO_HIP_TRY(c, hipMemcpyAsync(s->h_hist, s->cand_n, sizeof(int), hipMemcpyDeviceToHost, st));
        UVO_HIP_TRY(c, wait());
        n_cand = s->h_hist[0];
        s->stat_ncand = n_cand; s->stat_waits = waits; s->stat_rounds[0] = s->stat_rounds[1] = s->stat_rounds[2] = 0;
        if (n_cand > s->cand_cap) { c->err = kAkazeCandOverflow; return UVO_CAPACITY; }
        if (n_cand) {
            UVO_HIP_TRY(c, hipMemcpyAsync(s->h_cand, s->cand, sizeof(AkCand) * n_cand, hipMemcpyDeviceToHost, st));
            UVO_HIP_TRY(c, wait());
            s->stat_waits = waits;
        }
        UVO_HIP_TRY(c, hipGetLastError());
        stamp();
        // ---- FindKeypointsSameScale's sequential half, Find_Scale_Space_Extrema's two sweeps, Do_Subpixel_Refinement (host, candidate lists) ----
        akaze_suppress_host(s, s->h_cand, n_cand, nullptr);
        n = (int)s->out.size();
        stamp();
    }
    *n_out = n;
    if (n == 0 || (n > s->cap && !grow)) return UVO_OK;
    if (n > s->cap) {                                                // (the stream is idle here: synchronised after the count's copy; the
        (void)hipFree(s->d_kps); (void)hipFree(s->d_desc);          // outputs are not part of the captured graph)
        s->d_kps = nullptr; s->d_desc = nullptr; s->cap = 0;
        const int ncap = (n + 4095) & ~4095;
        if (hipMalloc(reinterpret_cast<void**>(&s->d_kps), sizeof(uvo_keypoint) * (size_t)ncap) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&s->d_desc), (size_t)kAkDescBytes * ncap) != hipSuccess) { c->err = "AKAZE: growing the output buffers failed"; return UVO_HIP_ERROR; }
        s->cap = ncap;
        if (where == 1) UVO_TRY(akaze_suppress_launch(c, s, st, s->d_kps, s->cap, 0, false));         // (the marks are still there: the refinement again, into the buffer that holds them all)
    }
    // ---- Compute_Keypoints_Orientation, MLDB descriptors ----
    if (where == 0) UVO_HIP_TRY(c, hipMemcpyAsync(s->d_kps, s->out.data(), sizeof(uvo_keypoint) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ak_orientation, dim3((n + 3) / 4), dim3(256), 0, st, pl, s->d_kps, n, (const int*)nullptr);
    hipLaunchKernelGGL(k_ak_mldb, dim3((n + 7) / 8), dim3(256), 0, st, pl, s->d_kps, n, (const int*)nullptr, s->d_desc, kAkDescBytes);
    UVO_HIP_TRY(c, hipGetLastError());
    if (dbg) UVO_HIP_TRY(c, hipStreamSynchronize(st));
    stamp();
    if (dbg && where == 1 && nph == 4) fprintf(stderr, "[uvo] akaze phases (ms), device suppression: queueing up to the contrast factor %.3f | evolution + responses + ordered candidates (%d) + suppression + refinement, to the count's wait %.3f | orientation + M-LDB (%d keypoints) %.3f\n",
                                               (tph[1] - tph[0]) * 1e-3, n_cand, (tph[2] - tph[1]) * 1e-3, n, (tph[3] - tph[2]) * 1e-3);
    if (dbg && where == 0 && nph == 5) fprintf(stderr, "[uvo] akaze phases (ms): contrast %.3f | evolution + responses + candidates (%d) %.3f | %s suppression + refinement %.3f | orientation + M-LDB (%d keypoints) %.3f\n",
                                 (tph[1] - tph[0]) * 1e-3, n_cand, (tph[2] - tph[1]) * 1e-3, "host", (tph[3] - tph[2]) * 1e-3, n, (tph[4] - tph[3]) * 1e-3);
    return UVO_OK;
}
static int akaze_suppress_from_env()                                // UVO_AKAZE_SUPPRESS=host|device: the initial setting, for measurements (tools/probe/README.md)
{
    const char* e = getenv("UVO_AKAZE_SUPPRESS");
    if (e && strcmp(e, "host") == 0) return 0;
    if (e && strcmp(e, "device") == 0) return 1;
    return kAkazeSuppressDefault;
}
static int akaze_where(Ctx* c)                                      // the context's setting (-1: not set yet)
{
    if (c->akaze_suppress < 0) c->akaze_suppress = akaze_suppress_from_env();
    return c->akaze_suppress;
}
uvo_status akaze_set_suppression(Ctx* c, int where)
{
    if (where != 0 && where != 1) { c->err = "uvo_akaze_set_suppression: 0 (the host scans of the candidate list) or 1 (the device form: k_ak_scan, k_ak_refine)"; return UVO_INVALID_ARG; }
    c->akaze_suppress = where;
    return UVO_OK;
}
// uvo_akaze_configure.  Everything made for the previous value goes from every lane: the level plan, the INTER_AREA tables and the captured
// evolution graphs (threshold and conductance kernel are launch arguments recorded in them); the next detection makes them again, as
// for a new image size.  The caller holds an idle context whose streams have drained.
uvo_status akaze_configure(Ctx* c, int descriptor_type, int descriptor_size, int descriptor_channels, float threshold, int n_octaves, int n_octave_layers, int diffusivity)
{
    if (descriptor_type >= 2 && descriptor_type <= 4) {
        c->err = "uvo_akaze_configure: descriptor_type 2 (DESCRIPTOR_KAZE_UPRIGHT), 3 (DESCRIPTOR_KAZE) and 4 (DESCRIPTOR_MLDB_UPRIGHT) are not implemented; served is 5 (DESCRIPTOR_MLDB)";
        return UVO_INVALID_ARG;
    }
    if (descriptor_type != 5) { c->err = "uvo_akaze_configure: descriptor_type: served is 5 (DESCRIPTOR_MLDB) only"; return UVO_INVALID_ARG; }
    if (descriptor_size != 0) { c->err = "uvo_akaze_configure: descriptor_size: served is 0 (the full 486 bits) only; descriptor subsets are not implemented"; return UVO_INVALID_ARG; }
    if (descriptor_channels != 3) { c->err = "uvo_akaze_configure: descriptor_channels: served is 3 only; 1- and 2-channel M-LDB are not implemented"; return UVO_INVALID_ARG; }
    if (!(threshold > 0.0f) || !(threshold <= FLT_MAX)) { c->err = "uvo_akaze_configure: threshold: served is any finite value > 0"; return UVO_INVALID_ARG; }
    if (n_octaves < 1 || n_octaves > 4) { c->err = "uvo_akaze_configure: n_octaves: served are 1..4"; return UVO_INVALID_ARG; }
    if (n_octave_layers < 1 || n_octave_layers > 4) { c->err = "uvo_akaze_configure: n_octave_layers: served are 1..4"; return UVO_INVALID_ARG; }
    if (diffusivity < 0 || diffusivity > 3) { c->err = "uvo_akaze_configure: diffusivity: served are 0 (DIFF_PM_G1), 1 (DIFF_PM_G2), 2 (DIFF_WEICKERT) and 3 (DIFF_CHARBONNIER)"; return UVO_INVALID_ARG; }
    AkazeCfg cfg;
    cfg.threshold = threshold; cfg.n_octaves = n_octaves; cfg.n_octave_layers = n_octave_layers; cfg.diffusivity = diffusivity;
    Ctx* m = c->sh->lanes[0];                                        // where akaze_ws reads it, for every lane
    if (cfg == m->akaze_cfg) return UVO_OK;
    m->akaze_cfg = cfg;
    for (Ctx* l : c->sh->lanes) { if (l->akaze_ws && l->stream) (void)hipStreamSynchronize(l->stream); akaze_ws_free(l); }
    return UVO_OK;
}
uvo_status akaze_detect(Ctx* c, const uint8_t* gray, int w, int h, int stride, int mem, uvo_keypoint* kps, uint8_t* desc, int cap, int* n_out)
{
    *n_out = 0;
    if (w < 16 || h < 16 || w > c->max_w || h > c->max_h || stride < w) { c->err = "uvo_akaze_detect: image size outside the context's limits"; return UVO_INVALID_ARG; }
    AkazeWs* s = akaze_ws(c, w, h);
    if (!s) return UVO_HIP_ERROR;                                    // (akaze_ws says why)
    hipStream_t st = c->stream;
    UVO_TRY(akaze_run(c, s, st, gray, w, h, stride, mem, true, akaze_where(c), nullptr, n_out));
    const int n = *n_out;
    if ((kps || desc) && n > cap) { c->err = "uvo_akaze_detect: output capacity too small"; return UVO_CAPACITY; }
    if (n == 0) return UVO_OK;
    if (kps) UVO_HIP_TRY(c, hipMemcpyAsync(kps, s->d_kps, sizeof(uvo_keypoint) * n, hipMemcpyDeviceToHost, st));
    if (desc) UVO_HIP_TRY(c, hipMemcpyAsync(desc, s->d_desc, (size_t)kAkDescBytes * n, hipMemcpyDeviceToHost, st));
    UVO_HIP_TRY(c, hipStreamSynchronize(st));
    return UVO_OK;
}

// ---- detect_features' AKAZE branch inside the fused steps.  The lane's workspace is made (and its evolution graph captured on the
// lane's stream) when a sequence starts, not in it; both images of a pair go through it in turn.  Under suppression setting 0 the host
// stages between the launches (contrast factor, duplicate suppression, refinement) wait for the device; under setting 1 the whole
// detection is queued and the count stays on the device (*d_n), as the SURF branch's does.
uvo_status akaze_prepare_lane(Ctx* c, int w, int h)
{
    AkazeWs* s = akaze_ws(c, w, h);
    if (!s) return UVO_HIP_ERROR;                                    // (akaze_ws says why)
    if (akaze_use_graph()) UVO_TRY(akaze_capture(c, s, c->stream, akaze_where(c->sh->lanes[0])));
    return UVO_OK;
}
uvo_status akaze_detect_lane(Ctx* c, int slot, int* n, const int** d_n, const int** d_ovf)
{
    const int w = c->img_w, h = c->img_h;
    *n = 0; *d_n = nullptr; *d_ovf = nullptr;
    if (w < 16 || h < 16) { c->err = "AKAZE: image too small"; return UVO_INVALID_ARG; }
    UVO_TRY(akaze_prepare_lane(c, w, h));                                    // (a no-op once the lane is primed)
    AkazeWs* s = static_cast<AkazeWs*>(c->akaze_ws);
    const int where = akaze_where(c->sh->lanes[0]);                          // the master context's value serves every lane
    if (where == 1) {
        const AkLaneOut lo = { c->det[slot].kps, reinterpret_cast<uint8_t*>(c->det[slot].desc), c->cap, slot };
        UVO_TRY(akaze_run(c, s, c->stream, c->img[slot], w, h, w, UVO_MEM_DEVICE, false, 1, &lo, n));
        *d_n = s->d_sup + SUP_NK + slot; *d_ovf = s->d_sup + SUP_OVF + slot;
        return UVO_OK;
    }
    UVO_TRY(akaze_run(c, s, c->stream, c->img[slot], w, h, w, UVO_MEM_DEVICE, false, 0, nullptr, n));
    if (*n > c->cap || *n == 0) return UVO_OK;
    UVO_HIP_TRY(c, hipMemcpyAsync(c->det[slot].kps, s->d_kps, sizeof(uvo_keypoint) * (size_t)*n, hipMemcpyDeviceToDevice, c->stream));
    return pad_binary_rows(c, c->stream, s->d_desc, *n, kAkDescBytes, reinterpret_cast<uint8_t*>(c->det[slot].desc));
}
// uvo_akaze_suppress: the scans and the refinement of uvo_akaze_detect on the caller's candidate list (any order), for the plan of a w x h image
uvo_status akaze_suppress(Ctx* c, int w, int h, const int* level, const int* x, const int* y, const float* v9, int n, int where, uint8_t* marks, uvo_keypoint* kps, int cap, int* n_kps)
{
    *n_kps = 0;
    if (where != 0 && where != 1) { c->err = "uvo_akaze_suppress: where = 0 (host) or 1 (device)"; return UVO_INVALID_ARG; }
    if (w < 16 || h < 16 || w > c->max_w || h > c->max_h || w > 65535 || h > 65535) { c->err = "uvo_akaze_suppress: image size outside the context's limits"; return UVO_INVALID_ARG; }
    if (n < 0) { c->err = "uvo_akaze_suppress: a negative candidate count"; return UVO_INVALID_ARG; }
    if (n > kAkCandCap) { c->err = "uvo_akaze_suppress: more candidates than the candidate list holds (262144)"; return UVO_INVALID_ARG; }
    if (n > 0 && (!level || !x || !y || !v9)) { c->err = "uvo_akaze_suppress: level, x, y and v9 are required"; return UVO_INVALID_ARG; }
    AkazeWs* s = akaze_ws(c, w, h);
    if (!s) return UVO_HIP_ERROR;                                    // (akaze_ws says why)
    std::vector<AkCand> list((size_t)n);
    for (int q = 0; q < n; q++) {
        if (level[q] < 0 || level[q] >= s->n) { c->err = "uvo_akaze_suppress: a candidate's level is outside the image's plan"; return UVO_INVALID_ARG; }
        if (x[q] < 0 || y[q] < 0 || x[q] >= s->lv[level[q]].w || y[q] >= s->lv[level[q]].h) { c->err = "uvo_akaze_suppress: a candidate's position is outside its level"; return UVO_INVALID_ARG; }
        AkCand& cd = list[(size_t)q];
        cd.x = x[q]; cd.y = y[q]; cd.pad = level[q];
        memcpy(cd.v, v9 + (size_t)9 * q, sizeof(float) * 9);
    }
    std::vector<uint64_t> keys((size_t)n);                                   // (level, y, x, list position): the visiting order, and duplicates side by side
    for (int q = 0; q < n; q++) keys[(size_t)q] = ((uint64_t)level[q] << 58) | ((uint64_t)y[q] << 40) | ((uint64_t)x[q] << 22) | (uint64_t)q;
    std::sort(keys.begin(), keys.end());
    for (int q = 1; q < n; q++) if ((keys[(size_t)q] >> 22) == (keys[(size_t)q - 1] >> 22)) { c->err = "uvo_akaze_suppress: two candidates on one cell of one level"; return UVO_INVALID_ARG; }
    hipStream_t st = c->stream;
    s->stat_dev = where; s->stat_ncand = n; s->stat_waits = 0;
    s->stat_rounds[0] = s->stat_rounds[1] = s->stat_rounds[2] = 0;
    int nk = 0;
    std::vector<uvo_keypoint> dev_out;
    if (where == 0) {
        aks_host_clear(&s->hs);
        akaze_suppress_host(s, list.data(), n, marks);
        nk = (int)s->out.size();
    } else {
        // the ordered list, as k_ak_cand_emit leaves it
        std::vector<uint32_t> pos((size_t)n); std::vector<float> val((size_t)n);
        int* hs = s->h_sup;
        memset(hs, 0, sizeof(int) * SUP_INTS);
        hs[SUP_FOUND] = hs[SUP_N] = n;
        for (int l = 0; l <= kAkMaxLevels; l++) hs[SUP_START + l] = n;
        for (int q = n - 1; q >= 0; q--) {
            const AkCand& cd = list[keys[(size_t)q] & 0x3fffffu];
            s->h_cand[q] = cd; pos[(size_t)q] = aks_pos(cd.x, cd.y); val[(size_t)q] = cd.v[4];
            for (int l = cd.pad; l >= 0 && hs[SUP_START + l] > q; l--) hs[SUP_START + l] = q;
        }
        const int dcap = std::max(cap, 1);
        uvo_keypoint* d_out = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(uvo_keypoint) * (size_t)dcap) != hipSuccess) { c->err = "uvo_akaze_suppress: allocation failed"; return UVO_HIP_ERROR; }
        bool ok = hipMemcpyAsync(s->d_sup, hs, sizeof(int) * SUP_INTS, hipMemcpyHostToDevice, st) == hipSuccess;
        if (n) ok = ok && hipMemcpyAsync(s->cand, s->h_cand, sizeof(AkCand) * n, hipMemcpyHostToDevice, st) == hipSuccess &&
                    hipMemcpyAsync(s->d_pos, pos.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st) == hipSuccess &&
                    hipMemcpyAsync(s->d_val, val.data(), sizeof(float) * n, hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipStreamSynchronize(st) == hipSuccess;                    // (pos and val are pageable and local)
        const uvo_status rc = ok ? akaze_suppress_launch(c, s, st, d_out, cap, 0) : UVO_HIP_ERROR;
        std::vector<uint8_t> dm((size_t)3 * std::max(n, 1));
        ok = ok && rc == UVO_OK && hipMemcpyAsync(hs, s->d_sup, sizeof(int) * SUP_INTS, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        for (int ph = 0; ph < 3 && ok && n; ph++) ok = hipMemcpy(dm.data() + (size_t)ph * n, s->d_mark + (size_t)ph * kAkCandCap, (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
        nk = ok ? hs[SUP_NK] : 0;
        if (ok && nk > 0 && nk <= cap) { dev_out.resize((size_t)nk); ok = hipMemcpy(dev_out.data(), d_out, sizeof(uvo_keypoint) * (size_t)nk, hipMemcpyDeviceToHost) == hipSuccess; }
        (void)hipFree(d_out);
        if (!ok) { if (rc == UVO_OK) c->err = "uvo_akaze_suppress: a HIP call failed"; return rc != UVO_OK ? rc : UVO_HIP_ERROR; }
        if (marks) for (int q = 0; q < n; q++) for (int ph = 0; ph < 3; ph++) marks[(size_t)3 * (keys[(size_t)q] & 0x3fffffu) + ph] = dm[(size_t)ph * n + q];
    }
    *n_kps = nk;
    if (nk > cap) { c->err = "uvo_akaze_suppress: more keypoints than the output holds"; return UVO_CAPACITY; }
    if (nk) memcpy(kps, where == 0 ? s->out.data() : dev_out.data(), sizeof(uvo_keypoint) * (size_t)nk);
    return UVO_OK;
}
// uvo_akaze_stats: the last detection (or hook call) of this context's workspace
uvo_status akaze_stats(Ctx* c, int* n_candidates, int* rounds, int* host_waits)
{
    AkazeWs* s = static_cast<AkazeWs*>(c->akaze_ws);
    if (!s) { c->err = "uvo_akaze_stats: no AKAZE detection has run on this context"; return UVO_INVALID_ARG; }
    if (s->stat_dev) {
        UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
        UVO_HIP_TRY(c, hipMemcpy(s->h_sup, s->d_sup, sizeof(int) * SUP_INTS, hipMemcpyDeviceToHost));
        s->stat_ncand = s->h_sup[SUP_FOUND];
        for (int p = 0; p < 3; p++) s->stat_rounds[p] = s->h_sup[SUP_ROUNDS + p];
    }
    if (n_candidates) *n_candidates = s->stat_ncand;
    if (rounds) for (int p = 0; p < 3; p++) rounds[p] = s->stat_rounds[p];
    if (host_waits) *host_waits = s->stat_waits;
    return UVO_OK;
}
// intermediates for the parity tests: what = 0 Lt, 1 Lsmooth, 2 Lx, 3 Ly, 4 Ldet of `level` after the last akaze_detect
uvo_status akaze_plane(Ctx* c, int level, int what, float* out, int cap_floats, int* ow, int* oh)
{
    AkazeWs* s = static_cast<AkazeWs*>(c->akaze_ws);
    if (!s || level < 0 || level >= s->n || what < 0 || what > 4) { c->err = "uvo_akaze_plane: no such plane (run uvo_akaze_detect first)"; return UVO_INVALID_ARG; }
    const float* src = what == 0 ? s->Lt[level] : what == 1 ? s->Lsmooth[level] : what == 2 ? s->Lx[level] : what == 3 ? s->Ly[level] : s->Ldet[level];
    *ow = s->lv[level].w; *oh = s->lv[level].h;
    const size_t n = (size_t)*ow * *oh;
    if ((size_t)cap_floats < n) { c->err = "uvo_akaze_plane: output capacity too small"; return UVO_CAPACITY; }
    UVO_HIP_TRY(c, hipMemcpy(out, src, sizeof(float) * n, hipMemcpyDeviceToHost));
    return UVO_OK;
}

}  // namespace uvo
