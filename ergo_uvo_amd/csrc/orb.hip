// orb.hip -- the ORB branch of detect_features on gfx950 (uvo_libraries/src/VO_utility.cpp:100-105):
//     Ptr<ORB> detector = ORB::create(10000, 1.2, 8, 31, 0, 2, ORB::HARRIS_SCORE, 31, 10);
//     detector->detectAndCompute(img, noArray(), keypoints, descriptors);
// oriented FAST + rotated BRIEF (Rublee, Rabaud, Konolige, Bradski, ICCV 2011) in the form of OpenCV 4.5's features2d/src/orb.cpp as far
// as it can be recalled (PARITY UNPINNED).  All of it is integer or byte work on small images -- HBM / L1 bound, no matrix shapes:
//   k_orb_resize       the pyramid: level l = resize(level l - 1, INTER_LINEAR_EXACT): 8.8 fixed-point weights per axis from tables
//                      computed once per image size on the host, two roundings (16-bit row result, then >> 16)
//   k_orb_fast_score   FAST-9/16: per pixel the largest threshold at which nine contiguous circle pixels are all darker / all brighter
//                      (sliding minima and maxima over the ring by doubling: windows of 2, 4, 8, 9), zero where that is below the
//                      threshold -- what FAST_t<16> + cornerScore<16> leave in their score rows
//   k_orb_nms_rows     strict 3 x 3 maxima of the score map inside the edge margin, one wave per image row, in ROW-MAJOR order
//                      (count pass, k_orb_row_scan over every level's rows, write pass): the order retainBest starts from
//   k_orb_harris       HarrisResponses (7 x 7 block of Sobel products, integer sums) for the keypoints the FAST ranking kept
//   k_orb_keypoints    ICAngles (integer moments over the disc of radius 15, 32 lanes per keypoint, fastAtan2) and the KeyPoint fields
//   k_orb_blur         GaussianBlur 7 x 7, sigma 2, as the 8-bit filter engine runs it on a submatrix: integer taps [18 34 49 55 49 34 18],
//                      rows then columns in 32 bits through an LDS tile, one rounding (+ 2^15) >> 16, BORDER_REFLECT_101
//   k_orb_describe     rBRIEF: 32 lanes per keypoint (one per descriptor byte), the sampling table in LDS, rotated by the keypoint's
//                      angle, coordinates rounded half to even
// KeyPointsFilter::retainBest runs twice per level (on the FAST scores for twice the level's share, on the Harris responses for the
// share).  Its surviving SET is a threshold on the n-th largest response, but the ORDER it leaves -- which is the order of the output
// keypoints -- is that of libstdc++'s std::nth_element + std::partition, a sequential algorithm stated pass by pass:
//   k_rb_rank          both rankings, one launch each for all levels (uvo_orb_set_ranking 1, the default): introselect's Hoare passes
//                      as stopper lists + independent swaps + a closed-form cut (uvo_retain_best_dev.h), the tail partition likewise
//   k_orb_harris_cnt, k_orb_keypoints_cnt, k_orb_describe_cnt   with the rankings on the device and uvo_orb_set_counts 1 (the default) the
//                      counts between the launches stay on the device too: fixed grids sized from capacities walk the lists grid-stride up
//                      to lengths read from device memory, and a detection is queued without a stream wait
// or, with uvo_orb_set_ranking 0, the host replays it on the response arrays (uvo_retain_best.h: 4 bytes per keypoint down, 4 bytes per
// survivor up; the images never leave the device), like the RANSAC scans of the pose stages.
// THE SAMPLING TABLE IS AN INPUT (uvo_orb_set_pattern): OpenCV's bit_pattern_31_ (1024 integers learned offline) cannot be restated
// and the reference holds no copy; without a table the detector returns keypoints and refuses descriptors.
#include "uvo_ctx.h"
#include "uvo_math.h"
#define UVO_RB_TRACE           // the header counts rb_heap_select's calls: uvo_retain_best reports them (depth_limit_hits)
#include "uvo_retain_best.h"   // RbItem, retain_best_order: the host replay of KeyPointsFilter::retainBest's order
#include "uvo_retain_best_dev.h"   // the arithmetic of k_rb_rank, the same order on the device
#include <limits.h>
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>

namespace uvo {

static const int kOrbMaxLevels = 16, kOrbDescBytes = 32;
struct OrbParams { int nfeatures = 10000; float scaleFactor = 1.2f; int nlevels = 8, edgeThreshold = 31, patchSize = 31, fastThreshold = 10; };
struct OrbLevels {                                                  // by value into the kernels
    int n;
    int w[kOrbMaxLevels], h[kOrbMaxLevels], stride[kOrbMaxLevels], row0[kOrbMaxLevels + 1];
    const uint8_t* img[kOrbMaxLevels]; uint8_t* blur[kOrbMaxLevels]; uint8_t* score[kOrbMaxLevels];
    float scale[kOrbMaxLevels];
};
struct OrbPrefix { int n; int start[kOrbMaxLevels + 1]; };          // list positions at which each level's keypoints start
static const int kOrbRankDefault = 1;                               // device: profiles/orb_device_rank.json
// d_rank, in ints: k_rb_rank's ticket, counts and flags; the Harris list's OrbPrefix (n, start[17]); the final list's starts; both rankings' flags
enum { RK_META = 0, RK_P1 = 48, RK_P2 = 68, RK_HIT1 = 88, RK_HIT2 = 104, RK_BACK_END = 120, RK_INTS = 128 };
// ... and, past RK_BACK_END, what k_orb_keypoints_cnt leaves (uvo_orb_set_counts 1): per image slot the keypoint count and "more keypoints than the
// list holds" (read by k_binary_publish_dev and the host only), the depth-limit flags summed since the workspace was planned, the FAST corners' count
enum { RK_N = 120, RK_OVF = 122, RK_HITS = 124, RK_NFAST = 125 };
static const int kOrbCountsDefault = 1;                             // the device: profiles/orb_device_counts.json
static const int kOrbGridCap = 1024;                                // the counted launches' largest grid: four workgroups a CU on 256 CUs; the lists are walked grid-stride
struct OrbWs {
    OrbParams p;
    bool has_pattern = false;
    int8_t* d_pattern = nullptr;                                    // 512 x (x, y)
    // sized by (w, h, p):
    int w = 0, h = 0, cap = 0, border = 0, total_rows = 0, fast_cap = 0;
    int want[kOrbMaxLevels] = {0};
    int umax[40] = {0};
    OrbLevels L;
    uint8_t* d_pix = nullptr;                                       // every level's image, blurred copy and score map
    uint16_t* d_tab = nullptr;                                      // resize tables: per level l >= 1: xofs[w], xc1[w], yofs[h], yc1[h]
    size_t tab_off[kOrbMaxLevels] = {0};
    int* d_rows = nullptr;                                          // [total_rows] counts, [total_rows + 1] offsets, [kOrbMaxLevels + 1] level starts
    uint32_t* d_pos = nullptr; float* d_score = nullptr;            // FAST keypoints in row-major order, level after level
    int* d_sel = nullptr; float* d_resp = nullptr; int* d_fin = nullptr;
    uvo_keypoint* d_kps = nullptr; uint8_t* d_desc = nullptr;
    int* h_int = nullptr; float* h_f = nullptr;                     // pinned
    std::vector<int> fin;                                           // host: the final ranking (source of an asynchronous copy: kept until the next call)
    // uvo_orb_set_ranking: 1 = both retainBest rankings by k_rb_rank, 0 = by the host replay (the master context's value serves every lane)
    int rank_dev = kOrbRankDefault;
    RbdItem* d_items = nullptr; int* d_la = nullptr; int* d_lb = nullptr;      // k_rb_rank's items and stopper lists, fast_cap each
    int* d_rank = nullptr;                                          // RK_INTS words: k_rb_rank's own, then what it leaves (level starts, depth-limit flags)
    long depth_limit_hits = 0;                                      // segments that reached introselect's depth limit on the device, since the context was made
    // uvo_orb_set_counts: 1 = with the rankings on the device the counts stay there too and nothing waits, 0 = the host reads them between launches
    int counts_dev = kOrbCountsDefault;
    int hits_seen = 0;                                              // d_rank[RK_HITS] as last added to depth_limit_hits
    int stat_waits = 0, stat_fast = -1, stat_ranked = -1, stat_kps = -1;      // uvo_orb_stats: stream waits since the last call; the last counts that reached the host
};
static int orb_rank_from_env()                                      // UVO_ORB_RANK=host|device: the initial setting, for measurements (tools/probe/README.md)
{
    const char* e = getenv("UVO_ORB_RANK");
    if (e && strcmp(e, "host") == 0) return 0;
    if (e && strcmp(e, "device") == 0) return 1;
    return kOrbRankDefault;
}
static int orb_counts_from_env()                                    // UVO_ORB_COUNTS=host|device, likewise
{
    const char* e = getenv("UVO_ORB_COUNTS");
    if (e && strcmp(e, "host") == 0) return 0;
    if (e && strcmp(e, "device") == 0) return 1;
    return kOrbCountsDefault;
}
static const char* const kOrbNoTable = "uvo_orb_detect: descriptors need the sampling table -- OpenCV's bit_pattern_31_ (orb.cpp), 256 x (x0, y0, x1, y1) -- through uvo_orb_set_pattern; pass desc = NULL for keypoints only";
const char* const kOrbLoopNoTable = "ORB in the fused steps: the descriptors need the sampling table -- OpenCV's bit_pattern_31_ (orb.cpp), 256 x (x0, y0, x1, y1) -- through uvo_orb_set_pattern";

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_orb_resize(const uint8_t* __restrict__ src, int sw, int sh, int sstride, uint8_t* __restrict__ dst, int dw, int dh,
                                                    const uint16_t* __restrict__ xofs, const uint16_t* __restrict__ xc1, const uint16_t* __restrict__ yofs, const uint16_t* __restrict__ yc1)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const int xo = xofs[x], xo1 = min(xo + 1, sw - 1), yo = yofs[y], yo1 = min(yo + 1, sh - 1);
    const uint32_t cx = xc1[x], cy = yc1[y];
    const uint8_t* r0 = src + (size_t)yo * sstride;
    const uint8_t* r1 = src + (size_t)yo1 * sstride;
    const uint32_t h0 = (256u - cx) * r0[xo] + cx * r0[xo1];       // hlineResize: 8.8
    const uint32_t h1 = (256u - cx) * r1[xo] + cx * r1[xo1];
    const uint32_t v = (h0 * (256u - cy) + h1 * cy + 32768u) >> 16; // vlineResize: 16.16, one rounding
    dst[(size_t)y * dw + x] = (uint8_t)min(v, 255u);
}

// FAST-9/16.  ring[k] = v - p_k around the Bresenham circle of radius 3 (fast.cpp makeOffsets); A = max over the 16 arcs of nine of
// min(ring), B = the same for p_k - v; a corner at threshold t iff max(A, B) > t, its score max(A, B) - 1 (cornerScore<16>).
__global__ __launch_bounds__(256) void k_orb_fast_score(const uint8_t* __restrict__ img, int w, int h, int stride, int threshold, uint8_t* __restrict__ score)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    int out = 0;
    if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
        const uint8_t* p = img + (size_t)y * stride + x;
        const int v = p[0];
        int d[16];
        d[0] = v - p[3 * stride];       d[1] = v - p[3 * stride + 1];   d[2] = v - p[2 * stride + 2];   d[3] = v - p[stride + 3];
        d[4] = v - p[3];                d[5] = v - p[-stride + 3];      d[6] = v - p[-2 * stride + 2];  d[7] = v - p[-3 * stride + 1];
        d[8] = v - p[-3 * stride];      d[9] = v - p[-3 * stride - 1];  d[10] = v - p[-2 * stride - 2]; d[11] = v - p[-stride - 3];
        d[12] = v - p[-3];              d[13] = v - p[stride - 3];      d[14] = v - p[2 * stride - 2];  d[15] = v - p[3 * stride - 1];
        int mn[16], mx[16], t0[16], t1[16];
#pragma unroll
        for (int i = 0; i < 16; i++) { t0[i] = min(d[i], d[(i + 1) & 15]); t1[i] = max(d[i], d[(i + 1) & 15]); }          // windows of 2
#pragma unroll
        for (int i = 0; i < 16; i++) { mn[i] = min(t0[i], t0[(i + 2) & 15]); mx[i] = max(t1[i], t1[(i + 2) & 15]); }      // 4
#pragma unroll
        for (int i = 0; i < 16; i++) { t0[i] = min(mn[i], mn[(i + 4) & 15]); t1[i] = max(mx[i], mx[(i + 4) & 15]); }      // 8
        int A = -256, B = -256;
#pragma unroll
        for (int i = 0; i < 16; i++) { A = max(A, min(t0[i], d[(i + 8) & 15])); B = max(B, -max(t1[i], d[(i + 8) & 15])); } // 9
        const int m = max(A, B);
        if (m > threshold) out = m - 1;
    }
    score[(size_t)y * w + x] = (uint8_t)out;
}

// One wave per image row of every level: the strict 3 x 3 maxima of the score map inside the margin (FAST's own 3 pixels and
// KeyPointsFilter::runByImageBorder's edgeThreshold), left to right.  WRITE = false: the row's count; true: positions and scores at
// the row's offset.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_orb_nms_rows(OrbLevels L, int margin, int* __restrict__ rowcount, const int* __restrict__ rowoff,
                                                      uint32_t* __restrict__ pos, float* __restrict__ resp)
{
    const int grow = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (grow >= L.row0[L.n]) return;
    int l = 0;
    while (grow >= L.row0[l + 1]) l++;
    const int y = grow - L.row0[l], w = L.w[l], h = L.h[l];
    int running = 0;
    if (w > 2 * margin && h > 2 * margin && y >= margin && y < h - margin) {
        const uint8_t* s = L.score[l] + (size_t)y * w;
        const int base = WRITE ? rowoff[grow] : 0;
        for (int x0 = margin; x0 < w - margin; x0 += 64) {
            const int x = x0 + lane;
            bool keep = false;
            int sc = 0;
            if (x < w - margin) {
                sc = s[x];
                if (sc) keep = sc > s[x - 1] && sc > s[x + 1] && sc > s[x - w - 1] && sc > s[x - w] && sc > s[x - w + 1] && sc > s[x + w - 1] && sc > s[x + w] && sc > s[x + w + 1];
            }
            const unsigned long long b = __ballot(keep);
            if (WRITE && keep) {
                const int at = base + running + __popcll(b & ((1ull << lane) - 1ull));
                pos[at] = (uint32_t)x | ((uint32_t)y << 16);
                resp[at] = (float)sc;
            }
            running += __popcll(b);
        }
    }
    if (!WRITE && lane == 0) rowcount[grow] = running;
}
// exclusive scan of the row counts (one workgroup); off[n] = the total; lvl[l] = the offset at which level l starts
__global__ __launch_bounds__(1024) void k_orb_row_scan(const int* __restrict__ cnt, int n, int* __restrict__ off, OrbLevels L, int* __restrict__ lvl)
{
    __shared__ int part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024, b = t * per, e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; i++) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { const int v = t >= d ? part[t - d] : 0; __syncthreads(); part[t] += v; __syncthreads(); }
    int run = part[t] - s;
    for (int i = b; i < e; i++) { off[i] = run; run += cnt[i]; }
    if (t == 1023) off[n] = part[1023];
    __syncthreads();
    if (t <= L.n) lvl[t] = t == L.n ? part[1023] : off[L.row0[t]];
}

__device__ __forceinline__ int orb_level_of(const OrbPrefix& P, int j) { int l = 0; while (l + 1 < P.n && j >= P.start[l + 1]) l++; return l; }

// HarrisResponses(pyramid, layers, keypoints, 7, 0.04f) for list entry j (the FAST keypoint sel[j])
__device__ __forceinline__ void orb_harris_at(const OrbLevels& L, const OrbPrefix& P, const int* __restrict__ sel, const uint32_t* __restrict__ pos, float* __restrict__ resp, int j)
{
    const int l = orb_level_of(P, j), step = L.stride[l];
    const uint32_t pp = pos[sel[j]];
    const uint8_t* c0 = L.img[l] + (size_t)(pp >> 16) * step + (pp & 0xffffu);
    int a = 0, b = 0, c = 0;
    for (int i = -3; i <= 3; i++) {
        const uint8_t* rm = c0 + (i - 1) * step; const uint8_t* r0 = c0 + i * step; const uint8_t* rp = c0 + (i + 1) * step;
#pragma unroll
        for (int q = -3; q <= 3; q++) {
            const int Ix = ((int)r0[q + 1] - (int)r0[q - 1]) * 2 + ((int)rm[q + 1] - (int)rm[q - 1]) + ((int)rp[q + 1] - (int)rp[q - 1]);
            const int Iy = ((int)rp[q] - (int)rm[q]) * 2 + ((int)rp[q - 1] - (int)rm[q - 1]) + ((int)rp[q + 1] - (int)rm[q + 1]);
            a += Ix * Ix; b += Iy * Iy; c += Ix * Iy;
        }
    }
    const float scale = 1.f / ((1 << 2) * 7 * 255.f);
    const float scale_sq_sq = scale * scale * scale * scale;
    resp[j] = ((float)a * (float)b - (float)c * (float)c - 0.04f * ((float)a + (float)b) * ((float)a + (float)b)) * scale_sq_sq;
}
__global__ __launch_bounds__(256) void k_orb_harris(OrbLevels L, OrbPrefix P, const int* __restrict__ sel, int n, const uint32_t* __restrict__ pos, float* __restrict__ resp)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    orb_harris_at(L, P, sel, pos, resp, j);
}
// the same with the list's level starts where k_rb_rank left them (device ranking): the grid covers an upper bound of the list
__global__ __launch_bounds__(256) void k_orb_harris_dev(OrbLevels L, const OrbPrefix* __restrict__ Pd, const int* __restrict__ sel, const uint32_t* __restrict__ pos, float* __restrict__ resp)
{
    const OrbPrefix P = *Pd;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P.start[P.n]) return;
    orb_harris_at(L, P, sel, pos, resp, j);
}
// the same with nothing of the list known to the host (uvo_orb_set_counts 1): a grid sized from the list's capacity walks it up to the end
// k_rb_rank left, which every wave reads for itself (one address for the whole wave: the loop's exit does not diverge)
__global__ __launch_bounds__(256) void k_orb_harris_cnt(OrbLevels L, const OrbPrefix* __restrict__ Pd, const int* __restrict__ sel, const uint32_t* __restrict__ pos, float* __restrict__ resp)
{
    const OrbPrefix P = *Pd;
    const int n = P.start[P.n];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) orb_harris_at(L, P, sel, pos, resp, j);
}

__device__ __forceinline__ float orb_atan2_deg(float y, float x)     // cv::fastAtan2 (as surf.hip's fast_atan2_deg)
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
struct OrbUmax { int u[40]; };
// The final keypoints: entry i is Harris-list entry fin[i]; ICAngles over the disc of half_k (32 lanes per keypoint, lane = column),
// pt *= the level's scale, size = patchSize * scale, octave = the level.
__device__ __forceinline__ void orb_keypoint_at(const OrbLevels& L, const OrbPrefix& P, const OrbUmax& um, int half_k, int patch, const int* __restrict__ fin, int i, int lane,
                                                const int* __restrict__ sel, const uint32_t* __restrict__ pos, const float* __restrict__ resp, uvo_keypoint* __restrict__ kps)
{
    const int j = fin[i], l = orb_level_of(P, j), step = L.stride[l];
    const uint32_t pp = pos[sel[j]];
    const int px = (int)(pp & 0xffffu), py = (int)(pp >> 16);
    const uint8_t* c0 = L.img[l] + (size_t)py * step + px;
    int m01 = 0, m10 = 0;
    for (int u = lane - half_k; u <= half_k; u += 32) {
        const int au = u < 0 ? -u : u;
        for (int v = -half_k; v <= half_k; v++) {
            if (au > um.u[v < 0 ? -v : v]) continue;
            const int val = c0[v * step + u];
            m10 += u * val; m01 += v * val;
        }
    }
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) { m01 += __shfl_xor(m01, d, 32); m10 += __shfl_xor(m10, d, 32); }
    if (lane == 0) {
        const float s = L.scale[l];
        uvo_keypoint k;
        k.x = (float)px * s; k.y = (float)py * s;
        k.size = (float)patch * s;
        k.angle = orb_atan2_deg((float)m01, (float)m10);
        k.response = resp[j];
        k.octave = l; k.class_id = -1;
        kps[i] = k;
    }
}
__global__ __launch_bounds__(256) void k_orb_keypoints(OrbLevels L, OrbPrefix P, OrbUmax um, int half_k, int patch, const int* __restrict__ fin, int n,
                                                       const int* __restrict__ sel, const uint32_t* __restrict__ pos, const float* __restrict__ resp, uvo_keypoint* __restrict__ kps)
{
    const int i = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    if (i >= n) return;                                             // (a whole 32-lane group leaves together)
    orb_keypoint_at(L, P, um, half_k, patch, fin, i, lane, sel, pos, resp, kps);
}
__global__ __launch_bounds__(256) void k_orb_keypoints_dev(OrbLevels L, const OrbPrefix* __restrict__ Pd, OrbUmax um, int half_k, int patch, const int* __restrict__ fin, int n,
                                                           const int* __restrict__ sel, const uint32_t* __restrict__ pos, const float* __restrict__ resp, uvo_keypoint* __restrict__ kps)
{
    const OrbPrefix P = *Pd;                                        // the Harris list's level starts, left on the device by the first ranking
    const int i = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    if (i >= n) return;
    orb_keypoint_at(L, P, um, half_k, patch, fin, i, lane, sel, pos, resp, kps);
}
// How many keypoints a counted launch writes: all n of the final list, the first out_cap of them when the output holds fewer (the count
// published downstream is then out_cap, and the caller's overflow check reports n), none when n exceeds the list itself
__device__ __forceinline__ int orb_written(int n, int list_cap, int out_cap) { return n > list_cap ? 0 : min(n, out_cap); }
// k_orb_keypoints_dev with the final list's length read where the second ranking left it (rk[RK_P2 + L.n]), grid-stride; the first thread also
// leaves the count and the overflow flag of image `slot`, the FAST corners' count and the rankings' depth-limit flags for whoever reads them
__global__ __launch_bounds__(256) void k_orb_keypoints_cnt(OrbLevels L, int* rk, OrbUmax um, int half_k, int patch, const int* __restrict__ fin, int list_cap, int out_cap, int slot,
                                                           const int* __restrict__ n_fast, const int* __restrict__ sel, const uint32_t* __restrict__ pos, const float* __restrict__ resp,
                                                           uvo_keypoint* __restrict__ kps)
{
    const OrbPrefix P = *reinterpret_cast<const OrbPrefix*>(rk + RK_P1);
    const int n = rk[RK_P2 + L.n], nw = orb_written(n, list_cap, out_cap), lane = threadIdx.x & 31;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int hits = 0;
        for (int l = 0; l < L.n; l++) hits += rk[RK_HIT1 + l] + rk[RK_HIT2 + l];
        rk[RK_N + slot] = n; rk[RK_OVF + slot] = n > list_cap ? 1 : 0;
        rk[RK_HITS] += hits; rk[RK_NFAST] = *n_fast;
    }
    for (int i = blockIdx.x * 8 + (threadIdx.x >> 5); i < nw; i += gridDim.x * 8)      // (a whole 32-lane group stays or leaves together)
        orb_keypoint_at(L, P, um, half_k, patch, fin, i, lane, sel, pos, resp, kps);
}

struct OrbTaps { int k[7]; };
__device__ __forceinline__ int orb_reflect101(int p, int n) { while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p; return p; }
__global__ __launch_bounds__(256) void k_orb_blur(const uint8_t* __restrict__ src, int w, int h, int stride, OrbTaps kk, uint8_t* __restrict__ dst)
{
    __shared__ uint8_t tile[22][72];
    __shared__ int rowf[22][64];
    const int bx = blockIdx.x * 64, by = blockIdx.y * 16, t = threadIdx.x;
    for (int idx = t; idx < 22 * 70; idx += 256) {
        const int ty = idx / 70, tx = idx - ty * 70;
        tile[ty][tx] = src[(size_t)orb_reflect101(by + ty - 3, h) * stride + orb_reflect101(bx + tx - 3, w)];
    }
    __syncthreads();
    for (int idx = t; idx < 22 * 64; idx += 256) {
        const int r = idx >> 6, x = idx & 63;
        int a = 0;
#pragma unroll
        for (int q = 0; q < 7; q++) a += kk.k[q] * tile[r][x + q];
        rowf[r][x] = a;
    }
    __syncthreads();
    for (int idx = t; idx < 16 * 64; idx += 256) {
        const int y = idx >> 6, x = idx & 63;
        if (bx + x >= w || by + y >= h) continue;
        int a = 0;
#pragma unroll
        for (int q = 0; q < 7; q++) a += kk.k[q] * rowf[y + q][x];
        a = (a + (1 << 15)) >> 16;
        dst[(size_t)(by + y) * w + bx + x] = (uint8_t)min(max(a, 0), 255);
    }
}

// computeOrbDescriptors, WTA_K 2: lane = descriptor byte; bit b = I(p[16 byte + 2 b]) < I(p[16 byte + 2 b + 1]) on the blurred level
__device__ __forceinline__ int orb_describe_at(const OrbLevels& L, const int8_t* pat, const uvo_keypoint& k, int lane)
{
    const int l = k.octave, step = L.w[l];
    const float s = 1.f / L.scale[l];
    float angle = k.angle;
    angle *= (float)(3.1415926535897932384626433832795 / 180.f);
    double sd, cd;
    det_sincos((double)angle, &sd, &cd);                            // (OpenCV: libm's cosf / sinf -- stated departure, as the SIFT and AKAZE branches)
    const float a = (float)cd, b = (float)sd;
    const uint8_t* c0 = L.blur[l] + (size_t)cv_round_f(k.y * s) * step + cv_round_f(k.x * s);
    int val = 0;
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
        int t[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int q = 2 * (16 * lane + 2 * bit + e);
            const float fx = (float)pat[q], fy = (float)pat[q + 1];
            const float x = fx * a - fy * b, y = fx * b + fy * a;
            t[e] = c0[cv_round_f(y) * step + cv_round_f(x)];
        }
        val |= (t[0] < t[1]) << bit;
    }
    return val;
}
__global__ __launch_bounds__(256) void k_orb_describe(OrbLevels L, const int8_t* __restrict__ pattern, const uvo_keypoint* __restrict__ kps, int n, uint8_t* __restrict__ desc)
{
    __shared__ int pat32[256];                                      // the table's 1024 signed bytes, copied a word per thread
    pat32[threadIdx.x] = reinterpret_cast<const int*>(pattern)[threadIdx.x];
    const int8_t* pat = reinterpret_cast<const int8_t*>(pat32);
    __syncthreads();
    const int i = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    if (i >= n) return;
    desc[(size_t)i * kOrbDescBytes + lane] = (uint8_t)orb_describe_at(L, pat, kps[i], lane);
}
// the same for the keypoints k_orb_keypoints_cnt wrote (*n_p: the final list's length), grid-stride, into rows of row_bytes: 32, or the fused
// steps' 64 with the second half zeroed (what k_pad_binary_rows makes of a 32-byte row)
__global__ __launch_bounds__(256) void k_orb_describe_cnt(OrbLevels L, const int8_t* __restrict__ pattern, const uvo_keypoint* __restrict__ kps, const int* __restrict__ n_p,
                                                          int list_cap, int out_cap, uint8_t* __restrict__ desc, int row_bytes)
{
    __shared__ int pat32[256];
    pat32[threadIdx.x] = reinterpret_cast<const int*>(pattern)[threadIdx.x];
    const int8_t* pat = reinterpret_cast<const int8_t*>(pat32);
    __syncthreads();
    const int nw = orb_written(*n_p, list_cap, out_cap), lane = threadIdx.x & 31;
    for (int i = blockIdx.x * 8 + (threadIdx.x >> 5); i < nw; i += gridDim.x * 8) {
        uint8_t* row = desc + (size_t)i * row_bytes;
        row[lane] = (uint8_t)orb_describe_at(L, pat, kps[i], lane);
        if (row_bytes > kOrbDescBytes) row[kOrbDescBytes + lane] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ retainBest on the device
// k_rb_rank: KeyPointsFilter::retainBest's ORDER (uvo_retain_best.h; arithmetic and proof: uvo_retain_best_dev.h) for up to 16 segments in
// one launch, one workgroup of 16 waves per segment: segment l ranks resp[start[l] .. start[l + 1]) for keep.k[l] and leaves the old
// positions (global: start[l] + index) of what retainBest keeps, in its order, compacted at order[out_start[l] ..).  Every introselect
// round is one pass over the (response, index) items in memory: each wave lists the stoppers of its share of the range (ballots), the
// k-th swap pairs the k-th left stopper with the k-th right stopper from the right, and the cut is a closed form.  The median of
// three, the insertion sort of the last three items and -- past the depth limit, which natural images do not reach -- heap select are
// one lane's.  The workgroup that finishes last (one agent-scope release per workgroup, one ticket, one acquire) sums the counts and
// gathers every segment's order.
struct RbKeep { int k[kOrbMaxLevels]; };
struct RbShared { int cntL[kRbdWaves], cntR[kRbdWaves], prefL[kRbdWaves + 1], prefR[kRbdWaves + 1]; int K, last; };
enum { RB_TICKET = 0, RB_COUNT = 4, RB_HIT = 4 + kOrbMaxLevels, RB_META_INTS = 4 + 2 * kOrbMaxLevels };   // the launch's own words (ticket zeroed before every launch)

template <int MODE>
__device__ __forceinline__ int rb_pass(RbdItem* v, int* A, int* B, int lo, int hi, float pv, RbShared& sh)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = rbd_chunk(hi - lo), b = lo + wave * chunk, e = min(b + chunk, hi);
    const unsigned long long below = (1ull << lane) - 1ull;
    int nl = 0, nr = 0;
    for (int p0 = b; p0 < e; p0 += kRbdLanes) {
        const int p = p0 + lane;
        bool sl = false, sr = false;
        if (p < e) { const float x = v[p].r; sl = rbd_left_stop<MODE>(x, pv); sr = rbd_right_stop<MODE>(x, pv); }
        const unsigned long long bl = __ballot(sl), br = __ballot(sr);
        if (sl) A[b + nl + __popcll(bl & below)] = p;                // (rank < the wave's count <= e - b: inside the wave's own share)
        if (sr) B[b + nr + __popcll(br & below)] = p;
        nl += __popcll(bl); nr += __popcll(br);
    }
    if (lane == 0) { sh.cntL[wave] = nl; sh.cntR[wave] = nr; }
    __syncthreads();
    if (tid == 0) {
        int l = 0, r = 0;
        for (int w = 0; w < kRbdWaves; w++) { sh.prefL[w] = l; sh.prefR[w] = r; l += sh.cntL[w]; r += sh.cntR[w]; }
        sh.prefL[kRbdWaves] = l; sh.prefR[kRbdWaves] = r; sh.K = 0;
    }
    __syncthreads();
    const int totL = sh.prefL[kRbdWaves], totR = sh.prefR[kRbdWaves], kmax = min(totL, totR);
    int mine = 0;
    for (int k = tid; k < kmax; k += kRbdThreads) {
        const int pa = A[rbd_list_at(lo, chunk, sh.prefL, k)], pb = B[rbd_list_at(lo, chunk, sh.prefR, totR - 1 - k)];
        if (pa < pb) { const RbdItem x = v[pa], y = v[pb]; v[pa] = y; v[pb] = x; mine++; }
    }
    if (MODE == 1) { __syncthreads(); return totR; }
    if (mine) atomicAdd(&sh.K, mine);
    __syncthreads();
    const int K = sh.K;
    const bool has_a = K < totL, has_b = K > 0;
    const int a_K = has_a ? A[rbd_list_at(lo, chunk, sh.prefL, K)] : INT_MAX, b_Km1 = has_b ? B[rbd_list_at(lo, chunk, sh.prefR, totR - K)] : hi;
    __syncthreads();                                                 // (sh is the next pass's)
    return rbd_cut(has_a, a_K, has_b, b_Km1, hi);
}

__global__ __launch_bounds__(1024) void k_rb_rank(const float* __restrict__ resp, const int* __restrict__ start, RbKeep keep, int nseg, RbdItem* items, int* la, int* lb,
                                                  int* meta, int* order, int cap, int* out_start, int* hits)
{
    __shared__ RbShared sh;
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int s0 = start[seg], n = start[seg + 1] - s0, kp = keep.k[seg];
    RbdItem* v = items + s0;
    for (int q = tid; q < n; q += kRbdThreads) { RbdItem x; x.r = resp[s0 + q]; x.i = q; v[q] = x; }
    int count = n, hit = 0;
    if (n > kp && kp == 0) count = 0;
    else if (n > kp) {
        int* A = la + s0; int* B = lb + s0;
        __syncthreads();
        int first = 0, last = n, depth = rbd_depth(n);
        const int nth = kp - 1;
        while (last - first > 3) {
            if (depth == 0) { hit = 1; break; }
            --depth;
            if (tid == 0) {
                const int at0 = first + 1, at1 = first + (last - first) / 2, at2 = last - 1;
                const int pick = rbd_median_pick(v[at0].r, v[at1].r, v[at2].r);
                rbd_swap(v + first, v + (pick == 0 ? at0 : pick == 1 ? at1 : at2));
            }
            __syncthreads();
            const int cut = rb_pass<0>(v, A, B, first + 1, last, v[first].r, sh);
            if (rbd_take_right(cut, nth)) first = cut; else last = cut;
        }
        if (tid == 0) {
            if (hit) { rbd_heap_select(v + first, v + nth + 1, v + last); rbd_swap(v + first, v + nth); }
            else rbd_insertion(v + first, v + last);
        }
        __syncthreads();
        count = kp + rb_pass<1>(v, A, B, kp, n, v[nth].r, sh);
    }
    // ---- publish this segment; the last workgroup to arrive gathers all of them ----
    if (tid == 0) {
        __hip_atomic_store(meta + RB_COUNT + seg, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(meta + RB_HIT + seg, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // every storing wave, before the barrier
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // (the write-back has landed before the ticket is drawn)
        const int ticket = __hip_atomic_fetch_add(meta + RB_TICKET, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh.last = ticket == nseg - 1;
        if (sh.last) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    }
    __syncthreads();
    if (!sh.last) return;
    int run = 0;
    for (int l = 0; l < nseg; l++) {
        const int c = __hip_atomic_load(meta + RB_COUNT + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), sl = start[l];
        if (tid == 0) { out_start[l] = run; hits[l] = __hip_atomic_load(meta + RB_HIT + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        if (run + c <= cap) for (int q = tid; q < c; q += kRbdThreads) order[run + q] = sl + items[sl + q].i;    // (past cap: the host reads out_start and refuses)
        run += c;
    }
    if (tid == 0) out_start[nseg] = run;
}

// ------------------------------------------------------------------------------------------------ host
namespace {
// resize.cpp interpolationLinear<uint8_t>::getCoeffs over one axis: source offset and the 8.8 weight of the right / lower neighbour.  An
// index left of the first (right of the last) sample centre takes that sample alone: offset at the end, weight 0.
void linear_exact_table(int ssize, int dsize, uint16_t* ofs, uint16_t* c1)
{
    const double inv_scale = (double)dsize / ssize;
    const double scale = 1.0 / inv_scale;
    for (int val = 0; val < dsize; val++) {
        const double fval = scale * ((double)val + 0.5) - 0.5;
        const int ival = cv_floor_d(fval);
        ofs[val] = 0; c1[val] = 0;
        if (ival >= 0 && ssize > 1) {
            if (ival < ssize - 1) { ofs[val] = (uint16_t)ival; c1[val] = (uint16_t)cv_round_d((fval - (double)ival) * 256.0); }
            else ofs[val] = (uint16_t)(ssize - 1);
        }
    }
}
}  // namespace

static void orb_free_sized(OrbWs* s)
{
    int hits = 0;                                                   // (idle here) the depth-limit flags no count readback has carried to the host yet
    if (s->d_rank && hipMemcpy(&hits, s->d_rank + RK_HITS, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) s->depth_limit_hits += hits - s->hits_seen;
    s->hits_seen = 0;
    (void)hipFree(s->d_pix); (void)hipFree(s->d_tab); (void)hipFree(s->d_rows); (void)hipFree(s->d_pos); (void)hipFree(s->d_score); (void)hipFree(s->d_sel);
    (void)hipFree(s->d_resp); (void)hipFree(s->d_fin); (void)hipFree(s->d_kps); (void)hipFree(s->d_desc); (void)hipHostFree(s->h_int); (void)hipHostFree(s->h_f);
    (void)hipFree(s->d_items); (void)hipFree(s->d_la); (void)hipFree(s->d_lb); (void)hipFree(s->d_rank);
    s->d_items = nullptr; s->d_la = nullptr; s->d_lb = nullptr; s->d_rank = nullptr;
    s->d_pix = nullptr; s->d_tab = nullptr; s->d_rows = nullptr; s->d_pos = nullptr; s->d_score = nullptr; s->d_sel = nullptr; s->d_resp = nullptr; s->d_fin = nullptr;
    s->d_kps = nullptr; s->d_desc = nullptr; s->h_int = nullptr; s->h_f = nullptr;
    s->w = s->h = 0;
}
void orb_ws_free(Ctx* c)
{
    OrbWs* s = static_cast<OrbWs*>(c->orb_ws);
    if (!s) return;
    orb_free_sized(s);
    (void)hipFree(s->d_pattern);
    delete s;
    c->orb_ws = nullptr;
}
static OrbWs* orb_state(Ctx* c)
{
    if (!c->orb_ws) { c->orb_ws = new OrbWs(); static_cast<OrbWs*>(c->orb_ws)->rank_dev = orb_rank_from_env(); static_cast<OrbWs*>(c->orb_ws)->counts_dev = orb_counts_from_env(); }
    return static_cast<OrbWs*>(c->orb_ws);
}
// ORB_Impl::detectAndCompute's level geometry and computeKeyPoints' shares (orb.cpp), tables and buffers for one image size
static uvo_status orb_plan(Ctx* c, OrbWs* s, int w, int h)
{
    if (s->w == w && s->h == h && s->d_pix) return UVO_OK;
    orb_free_sized(s);
    const OrbParams& p = s->p;
    const double scaleFactor = (double)p.scaleFactor;               // ORB::create takes a float, ORB_Impl keeps a double
    const int half = p.patchSize / 2;
    s->border = std::max(p.edgeThreshold, std::max(cv_ceil_d(half * sqrt(2.0)), 9 / 2)) + 1;
    OrbLevels& L = s->L;
    memset(&L, 0, sizeof(L));
    L.n = p.nlevels;
    size_t px = 0;
    int rows = 0;
    for (int l = 0; l < L.n; l++) {
        const float sc = (float)pow(scaleFactor, (double)l);        // getScale(level, firstLevel = 0, scaleFactor)
        const float inv = 1.0f / sc;
        L.scale[l] = sc;
        L.w[l] = cv_round_f((float)w * inv); L.h[l] = cv_round_f((float)h * inv);
        if (L.w[l] < 2 || L.h[l] < 2) { c->err = "uvo_orb_detect: the image is too small for this many pyramid levels"; return UVO_INVALID_ARG; }
        L.stride[l] = L.w[l];
        L.row0[l] = rows; rows += L.h[l];
        px += (size_t)L.w[l] * L.h[l];
    }
    L.row0[L.n] = rows;
    s->total_rows = rows;
    const float factor = (float)(1.0 / scaleFactor);
    float ndesired = (float)p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L.n));
    int sum = 0;
    for (int l = 0; l < L.n - 1; l++) { s->want[l] = cv_round_f(ndesired); sum += s->want[l]; ndesired *= factor; }
    s->want[L.n - 1] = std::max(p.nfeatures - sum, 0);
    {   // the disc's row ends (computeKeyPoints: umax)
        const int vmax = cv_floor_d(half * sqrtf(2.f) / 2 + 1), vmin = cv_ceil_d(half * sqrtf(2.f) / 2);
        memset(s->umax, 0, sizeof(s->umax));
        for (int v = 0; v <= vmax; ++v) s->umax[v] = cv_round_d(sqrt((double)half * half - v * v));
        for (int v = half, v0 = 0; v >= vmin; --v) { while (s->umax[v0] == s->umax[v0 + 1]) ++v0; s->umax[v] = v0; ++v0; }
    }
    s->fast_cap = (int)std::min<size_t>(px / 4 + 64, (size_t)1 << 24);      // strict 3 x 3 maxima: at most one per 2 x 2 block
    s->cap = std::max(c->cap, p.nfeatures + p.nfeatures / 4 + 1024);     // retainBest bounds the output by nfeatures, ties at the per-level cuts aside
    bool ok = hipMalloc(reinterpret_cast<void**>(&s->d_pix), 3 * px + 64) == hipSuccess;
    // resize tables
    std::vector<uint16_t> tab;
    for (int l = 1; l < L.n; l++) {
        s->tab_off[l] = tab.size();
        tab.resize(tab.size() + 2 * (size_t)(L.w[l] + L.h[l]));
        uint16_t* t = tab.data() + s->tab_off[l];
        linear_exact_table(L.w[l - 1], L.w[l], t, t + L.w[l]);
        linear_exact_table(L.h[l - 1], L.h[l], t + 2 * L.w[l], t + 2 * L.w[l] + L.h[l]);
    }
    ok = ok && hipMalloc(reinterpret_cast<void**>(&s->d_tab), sizeof(uint16_t) * (tab.size() + 8)) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_rows), sizeof(int) * (2 * (size_t)rows + 2 + kOrbMaxLevels + 1)) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_pos), sizeof(uint32_t) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_score), sizeof(float) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_sel), sizeof(int) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_resp), sizeof(float) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_fin), sizeof(int) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_kps), sizeof(uvo_keypoint) * (size_t)s->cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_desc), (size_t)kOrbDescBytes * s->cap) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&s->h_int), sizeof(int) * ((size_t)s->fast_cap + 64)) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&s->h_f), sizeof(float) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_items), sizeof(RbdItem) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_la), sizeof(int) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_lb), sizeof(int) * (size_t)s->fast_cap) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&s->d_rank), sizeof(int) * RK_INTS) == hipSuccess;
    if (ok) {
        int init[RK_INTS] = {0};
        init[RK_P1] = L.n;                                           // OrbPrefix::n of the Harris list; k_rb_rank writes its starts
        ok = hipMemcpy(s->d_rank, init, sizeof(init), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok && !tab.empty()) ok = hipMemcpy(s->d_tab, tab.data(), sizeof(uint16_t) * tab.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { orb_free_sized(s); c->err = "ORB workspace allocation failed"; return UVO_HIP_ERROR; }
    uint8_t* q = s->d_pix;
    for (int l = 0; l < L.n; l++) { const size_t n = (size_t)L.w[l] * L.h[l]; L.img[l] = q; L.blur[l] = q + px; L.score[l] = q + 2 * px; q += n; }
    s->w = w; s->h = h;
    return UVO_OK;
}

uvo_status orb_configure(Ctx* c, int nfeatures, float scaleFactor, int nlevels, int edgeThreshold, int patchSize, int fastThreshold)
{
    OrbWs* s = orb_state(c);
    const int reach = cv_ceil_d((patchSize / 2) * sqrt(2.0)) + 1;   // the rotated table's reach; OpenCV pads its levels by this much, this build keeps keypoints that far inside
    if (nfeatures < 1 || nlevels < 1 || nlevels > kOrbMaxLevels || !(scaleFactor > 1.0f) || patchSize < 5 || patchSize > 63 || fastThreshold < 1 || fastThreshold > 254 ||
        edgeThreshold < reach || edgeThreshold < 5) {
        c->err = "uvo_orb_configure: nfeatures >= 1, scaleFactor > 1, nlevels 1..16, patchSize 5..63, fastThreshold 1..254, edgeThreshold >= ceil(patchSize / 2 * sqrt 2) + 1";
        return UVO_INVALID_ARG;
    }
    if (patchSize != s->p.patchSize) s->has_pattern = false;        // a table belongs to its patch size
    s->p.nfeatures = nfeatures; s->p.scaleFactor = scaleFactor; s->p.nlevels = nlevels; s->p.edgeThreshold = edgeThreshold; s->p.patchSize = patchSize; s->p.fastThreshold = fastThreshold;
    orb_free_sized(s);
    return UVO_OK;
}
uvo_status orb_set_pattern(Ctx* c, const int* pattern)
{
    OrbWs* s = orb_state(c);
    if (!pattern) { s->has_pattern = false; return UVO_OK; }
    int8_t p8[1024];
    const int half = s->p.patchSize / 2;
    for (int i = 0; i < 1024; i++) {
        if (pattern[i] < -half || pattern[i] > half) { c->err = "uvo_orb_set_pattern: a coordinate lies outside the patch (|x|, |y| <= patchSize / 2)"; return UVO_INVALID_ARG; }
        p8[i] = (int8_t)pattern[i];
    }
    if (!s->d_pattern) UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&s->d_pattern), 1024));
    UVO_HIP_TRY(c, hipMemcpy(s->d_pattern, p8, 1024, hipMemcpyHostToDevice));
    s->has_pattern = true;
    return UVO_OK;
}

// detectAndCompute on `gray` (device or host) with workspace s (planned for w x h) and the sampling table `pattern` (device; null: keypoints
// only): the keypoints and their rows are left in s->d_kps / s->d_desc, *n_out = the count; when it exceeds the list's capacity nothing
// past the host ranking is computed and the call still returns UVO_OK
static OrbTaps orb_blur_taps()
{
    OrbTaps kk;
    // getGaussianKernel(7, 2, CV_32F) x 2^8 rounded: the 8-bit filter engine's integer taps
    double t[7], sum = 0;
    for (int i = 0; i < 7; i++) { const double x = i - 3; t[i] = exp(-0.5 / (2.0 * 2.0) * x * x); sum += t[i]; }
    for (int i = 0; i < 7; i++) kk.k[i] = cv_round_f((float)(t[i] * (1. / sum)) * 256.f);
    return kk;
}
// one launch of k_rb_rank on stream st: segment l = resp[start[l] .. start[l + 1]) (start on the device), keep[l] on the host
static uvo_status rb_launch(Ctx* c, hipStream_t st, const float* resp, const int* d_start, const int* keep, int nseg, RbdItem* items, int* la, int* lb, int* meta,
                            int* order, int cap, int* out_start, int* hits)
{
    RbKeep K; memset(&K, 0, sizeof(K));
    for (int l = 0; l < nseg; l++) K.k[l] = keep[l];
    UVO_HIP_TRY(c, hipMemsetAsync(meta, 0, 16, st));                 // the ticket's block
    hipLaunchKernelGGL(k_rb_rank, dim3(nseg), dim3(kRbdThreads), 0, st, resp, d_start, K, nseg, items, la, lb, meta, order, cap, out_start, hits);
    return UVO_OK;
}
// orb_run from the FAST corners' level starts on, with both rankings on the device: nothing that grows with the number of corners
// crosses to the host; the level starts and the depth-limit flags (RK_P1 .. RK_BACK_END, 288 bytes) come back once, for the grid sizes
static uvo_status orb_run_device(Ctx* c, OrbWs* s, hipStream_t st, const OrbLevels& L, int n_fast, const int8_t* pattern, int* n_out)
{
    const OrbParams& p = s->p;
    if (n_fast == 0) { s->stat_fast = s->stat_ranked = s->stat_kps = 0; return UVO_OK; }
    const int margin = std::max(p.edgeThreshold, 3), R = s->total_rows;
    int* d_cnt = s->d_rows; int* d_off = s->d_rows + R; int* d_lvl = s->d_rows + 2 * R + 1;
    int* rk = s->d_rank;
    OrbPrefix* d_P1 = reinterpret_cast<OrbPrefix*>(rk + RK_P1);
    hipLaunchKernelGGL(k_orb_nms_rows<true>, dim3((R + 3) / 4), dim3(256), 0, st, L, margin, d_cnt, d_off, s->d_pos, s->d_score);
    int keep[kOrbMaxLevels];
    // retainBest(keypoints, 2 * featuresNum) on the FAST scores, every level in one launch: d_sel and the Harris list's starts
    for (int l = 0; l < L.n; l++) keep[l] = 2 * s->want[l];
    UVO_TRY(rb_launch(c, st, s->d_score, d_lvl, keep, L.n, s->d_items, s->d_la, s->d_lb, rk + RK_META, s->d_sel, s->fast_cap, d_P1->start, rk + RK_HIT1));
    hipLaunchKernelGGL(k_orb_harris_dev, dim3((n_fast + 255) / 256), dim3(256), 0, st, L, d_P1, s->d_sel, s->d_pos, s->d_resp);      // (the list is no longer than n_fast)
    // retainBest(keypoints, featuresNum) on the Harris responses: d_fin and the final list's starts
    for (int l = 0; l < L.n; l++) keep[l] = s->want[l];
    UVO_TRY(rb_launch(c, st, s->d_resp, d_P1->start, keep, L.n, s->d_items, s->d_la, s->d_lb, rk + RK_META, s->d_fin, s->fast_cap, rk + RK_P2, rk + RK_HIT2));
    UVO_HIP_TRY(c, hipMemcpyAsync(s->h_int, rk + RK_P1, sizeof(int) * (RK_BACK_END - RK_P1), hipMemcpyDeviceToHost, st));
    if (pattern) {                                                  // (the blurred levels do not wait for the rankings)
        const OrbTaps kk = orb_blur_taps();
        for (int l = 0; l < L.n; l++)
            hipLaunchKernelGGL(k_orb_blur, dim3((L.w[l] + 63) / 64, (L.h[l] + 15) / 16), dim3(256), 0, st, L.img[l], L.w[l], L.h[l], L.stride[l], kk, L.blur[l]);
    }
    s->stat_waits++;
    UVO_HIP_TRY(c, hipStreamSynchronize(st));
    UVO_HIP_TRY(c, hipGetLastError());
    const int* back = s->h_int;
    for (int l = 0; l < L.n; l++) s->depth_limit_hits += back[RK_HIT1 - RK_P1 + l] + back[RK_HIT2 - RK_P1 + l];
    const int n = back[RK_P2 - RK_P1 + L.n];
    *n_out = n;
    s->stat_fast = n_fast; s->stat_ranked = back[1 + L.n]; s->stat_kps = n;
    static const bool dbg = getenv("UVO_DBG_PHASE") != nullptr;      // (as AKAZE's host-clock phases: tools/probe/README.md)
    if (dbg) fprintf(stderr, "orb: %d FAST corners, %d after the first ranking, %d keypoints; %ld ranking segments past the depth limit so far\n", n_fast, back[1 + L.n], n, s->depth_limit_hits);
    if (n > s->cap || n == 0) return UVO_OK;
    OrbUmax um; memcpy(um.u, s->umax, sizeof(um.u));
    hipLaunchKernelGGL(k_orb_keypoints_dev, dim3((n + 7) / 8), dim3(256), 0, st, L, d_P1, um, p.patchSize / 2, p.patchSize, s->d_fin, n, s->d_sel, s->d_pos, s->d_resp, s->d_kps);
    if (pattern) hipLaunchKernelGGL(k_orb_describe, dim3((n + 7) / 8), dim3(256), 0, st, L, pattern, s->d_kps, n, s->d_desc);
    UVO_HIP_TRY(c, hipGetLastError());
    return UVO_OK;
}

// Where a detection whose counts stay on the device (uvo_orb_set_counts 1 with the rankings there) leaves its keypoints and rows: the
// workspace's own lists (the operator: 32-byte rows, wait = true: ONE wait, for the counts that size the caller's copies) or image `slot`
// of a lane (det[slot]: 64-byte zero-padded rows, at most the lane's max_kpts; nothing waits)
struct OrbOut { uvo_keypoint* kps; uint8_t* rows; int row_bytes, cap, slot; bool wait; };
// d_rank as it came back (from RK_P1 on): the counts, the depth-limit flags k_orb_keypoints_cnt summed, UVO_DBG_PHASE's line
static void orb_counts_arrived(OrbWs* s, const int* back, int nlevels)
{
    s->depth_limit_hits += back[RK_HITS - RK_P1] - s->hits_seen;
    s->hits_seen = back[RK_HITS - RK_P1];
    s->stat_fast = back[RK_NFAST - RK_P1]; s->stat_ranked = back[1 + nlevels]; s->stat_kps = back[RK_P2 - RK_P1 + nlevels];
    static const bool dbg = getenv("UVO_DBG_PHASE") != nullptr;
    if (dbg) fprintf(stderr, "orb: %d FAST corners, %d after the first ranking, %d keypoints; %ld ranking segments past the depth limit so far\n", s->stat_fast, s->stat_ranked, s->stat_kps, s->depth_limit_hits);
}
// orb_run from the row scan on with every count left on the device: the ordered maxima, both rankings, the Harris responses, the
// keypoints and their rows are queued with launch shapes that depend on capacities only.  An empty list (no FAST corner, or none
// inside the border on some level) is no special case: k_rb_rank leaves empty segments empty and the grid-stride loops do not start.
// *n_out = the count with out.wait, else -1 (k_orb_keypoints_cnt left it in d_rank[RK_N + out.slot], the overflow flag in RK_OVF + out.slot)
static uvo_status orb_run_counted(Ctx* c, OrbWs* s, hipStream_t st, const OrbLevels& L, const int8_t* pattern, const OrbOut& out, int* n_out)
{
    const OrbParams& p = s->p;
    const int margin = std::max(p.edgeThreshold, 3), R = s->total_rows;
    int* d_cnt = s->d_rows; int* d_off = s->d_rows + R; int* d_lvl = s->d_rows + 2 * R + 1;
    int* rk = s->d_rank;
    OrbPrefix* d_P1 = reinterpret_cast<OrbPrefix*>(rk + RK_P1);
    hipLaunchKernelGGL(k_orb_nms_rows<true>, dim3((R + 3) / 4), dim3(256), 0, st, L, margin, d_cnt, d_off, s->d_pos, s->d_score);
    int keep[kOrbMaxLevels];
    long listed = 0;                                                // the Harris list: twice every level's share, ties at the cuts aside
    for (int l = 0; l < L.n; l++) { keep[l] = 2 * s->want[l]; listed += keep[l]; }
    UVO_TRY(rb_launch(c, st, s->d_score, d_lvl, keep, L.n, s->d_items, s->d_la, s->d_lb, rk + RK_META, s->d_sel, s->fast_cap, d_P1->start, rk + RK_HIT1));
    const int harris_grid = std::max(1, std::min(kOrbGridCap, (int)((std::min<long>(s->fast_cap, listed + 1024) + 255) / 256)));
    hipLaunchKernelGGL(k_orb_harris_cnt, dim3(harris_grid), dim3(256), 0, st, L, d_P1, s->d_sel, s->d_pos, s->d_resp);
    for (int l = 0; l < L.n; l++) keep[l] = s->want[l];
    UVO_TRY(rb_launch(c, st, s->d_resp, d_P1->start, keep, L.n, s->d_items, s->d_la, s->d_lb, rk + RK_META, s->d_fin, s->fast_cap, rk + RK_P2, rk + RK_HIT2));
    if (pattern) {
        const OrbTaps kk = orb_blur_taps();
        for (int l = 0; l < L.n; l++)
            hipLaunchKernelGGL(k_orb_blur, dim3((L.w[l] + 63) / 64, (L.h[l] + 15) / 16), dim3(256), 0, st, L.img[l], L.w[l], L.h[l], L.stride[l], kk, L.blur[l]);
    }
    OrbUmax um; memcpy(um.u, s->umax, sizeof(um.u));
    const int list_cap = s->cap, out_cap = std::min(out.cap, s->cap);
    const int kp_grid = std::max(1, std::min(kOrbGridCap, (out_cap + 7) / 8));
    hipLaunchKernelGGL(k_orb_keypoints_cnt, dim3(kp_grid), dim3(256), 0, st, L, rk, um, p.patchSize / 2, p.patchSize, s->d_fin, list_cap, out_cap, out.slot, d_lvl + L.n,
                       s->d_sel, s->d_pos, s->d_resp, out.kps);
    if (pattern) hipLaunchKernelGGL(k_orb_describe_cnt, dim3(kp_grid), dim3(256), 0, st, L, pattern, out.kps, rk + RK_P2 + L.n, list_cap, out_cap, out.rows, out.row_bytes);
    UVO_HIP_TRY(c, hipGetLastError());
    *n_out = -1;
    static const bool dbg = getenv("UVO_DBG_PHASE") != nullptr;      // (the line needs the counts: with the variable set a lane reads them back too)
    if (!out.wait && !dbg) return UVO_OK;
    UVO_HIP_TRY(c, hipMemcpyAsync(s->h_int, rk + RK_P1, sizeof(int) * (RK_INTS - RK_P1), hipMemcpyDeviceToHost, st));
    s->stat_waits++;
    UVO_HIP_TRY(c, hipStreamSynchronize(st));
    orb_counts_arrived(s, s->h_int, L.n);
    if (out.wait) *n_out = s->stat_kps;
    return UVO_OK;
}

static uvo_status orb_run(Ctx* c, OrbWs* s, hipStream_t st, const uint8_t* gray, int w, int h, int stride, int mem, const int8_t* pattern, int rank_dev, const OrbOut* counted, int* n_out)
{
    *n_out = 0;
    OrbLevels L = s->L;
    const OrbParams& p = s->p;
    // ---- the pyramid ----
    if (mem == UVO_MEM_DEVICE) { L.img[0] = gray; L.stride[0] = stride; }
    else UVO_HIP_TRY(c, hipMemcpy2DAsync(const_cast<uint8_t*>(L.img[0]), w, gray, stride, w, h, hipMemcpyHostToDevice, st));
    for (int l = 1; l < L.n; l++) {
        const uint16_t* t = s->d_tab + s->tab_off[l];
        hipLaunchKernelGGL(k_orb_resize, dim3((L.w[l] + 255) / 256, L.h[l]), dim3(256), 0, st, L.img[l - 1], L.w[l - 1], L.h[l - 1], L.stride[l - 1],
                           const_cast<uint8_t*>(L.img[l]), L.w[l], L.h[l], t, t + L.w[l], t + 2 * L.w[l], t + 2 * L.w[l] + L.h[l]);
    }
    // ---- FAST on every level, maxima in row-major order ----
    for (int l = 0; l < L.n; l++)
        hipLaunchKernelGGL(k_orb_fast_score, dim3((L.w[l] + 63) / 64, (L.h[l] + 3) / 4), dim3(256), 0, st, L.img[l], L.w[l], L.h[l], L.stride[l], p.fastThreshold, L.score[l]);
    const int margin = std::max(p.edgeThreshold, 3), R = s->total_rows;
    int* d_cnt = s->d_rows; int* d_off = s->d_rows + R; int* d_lvl = s->d_rows + 2 * R + 1;
    hipLaunchKernelGGL(k_orb_nms_rows<false>, dim3((R + 3) / 4), dim3(256), 0, st, L, margin, d_cnt, d_off, s->d_pos, s->d_score);
    hipLaunchKernelGGL(k_orb_row_scan, dim3(1), dim3(1024), 0, st, d_cnt, R, d_off, L, d_lvl);
    if (rank_dev && counted) return orb_run_counted(c, s, st, L, pattern, *counted, n_out);
    UVO_HIP_TRY(c, hipMemcpyAsync(s->h_int, d_lvl, sizeof(int) * (L.n + 1), hipMemcpyDeviceToHost, st));
    s->stat_waits++;
    UVO_HIP_TRY(c, hipStreamSynchronize(st));
    int lvl[kOrbMaxLevels + 1];
    memcpy(lvl, s->h_int, sizeof(int) * (L.n + 1));
    const int n_fast = lvl[L.n];
    if (n_fast > s->fast_cap) { c->err = "ORB: more FAST corners than the list holds"; return UVO_CAPACITY; }
    if (rank_dev) return orb_run_device(c, s, st, L, n_fast, pattern, n_out);
    std::vector<int> sel;
    OrbPrefix P1; memset(&P1, 0, sizeof(P1)); P1.n = L.n;
    std::vector<RbItem> tmp;
    if (n_fast > 0) {
        hipLaunchKernelGGL(k_orb_nms_rows<true>, dim3((R + 3) / 4), dim3(256), 0, st, L, margin, d_cnt, d_off, s->d_pos, s->d_score);
        UVO_HIP_TRY(c, hipMemcpyAsync(s->h_f, s->d_score, sizeof(float) * n_fast, hipMemcpyDeviceToHost, st));
        s->stat_waits++;
        UVO_HIP_TRY(c, hipStreamSynchronize(st));
        // retainBest(keypoints, 2 * featuresNum) on the FAST scores (HARRIS_SCORE keeps twice the share for the second ranking)
        for (int l = 0; l < L.n; l++) { P1.start[l] = (int)sel.size(); retain_best_order(s->h_f + lvl[l], lvl[l + 1] - lvl[l], 2 * s->want[l], lvl[l], &tmp, &sel); }
    }
    P1.start[L.n] = (int)sel.size();
    const int n1 = (int)sel.size();
    std::vector<int>& fin = s->fin;
    fin.clear();
    if (n1 > 0) {
        UVO_HIP_TRY(c, hipMemcpyAsync(s->d_sel, sel.data(), sizeof(int) * n1, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_orb_harris, dim3((n1 + 255) / 256), dim3(256), 0, st, L, P1, s->d_sel, n1, s->d_pos, s->d_resp);
        UVO_HIP_TRY(c, hipMemcpyAsync(s->h_f, s->d_resp, sizeof(float) * n1, hipMemcpyDeviceToHost, st));
        s->stat_waits++;
        UVO_HIP_TRY(c, hipStreamSynchronize(st));
        // retainBest(keypoints, featuresNum) on the Harris responses, level by level
        for (int l = 0; l < L.n; l++) retain_best_order(s->h_f + P1.start[l], P1.start[l + 1] - P1.start[l], s->want[l], P1.start[l], &tmp, &fin);
    }
    UVO_HIP_TRY(c, hipGetLastError());
    const int n = (int)fin.size();
    *n_out = n;
    s->stat_fast = n_fast; s->stat_ranked = n1; s->stat_kps = n;
    if (n > s->cap || n == 0) return UVO_OK;
    // ---- ICAngles + the KeyPoint fields; blur; descriptors ----
    OrbUmax um; memcpy(um.u, s->umax, sizeof(um.u));
    UVO_HIP_TRY(c, hipMemcpyAsync(s->d_fin, fin.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_orb_keypoints, dim3((n + 7) / 8), dim3(256), 0, st, L, P1, um, p.patchSize / 2, p.patchSize, s->d_fin, n, s->d_sel, s->d_pos, s->d_resp, s->d_kps);
    if (pattern) {
        const OrbTaps kk = orb_blur_taps();
        for (int l = 0; l < L.n; l++)
            hipLaunchKernelGGL(k_orb_blur, dim3((L.w[l] + 63) / 64, (L.h[l] + 15) / 16), dim3(256), 0, st, L.img[l], L.w[l], L.h[l], L.stride[l], kk, L.blur[l]);
        hipLaunchKernelGGL(k_orb_describe, dim3((n + 7) / 8), dim3(256), 0, st, L, pattern, s->d_kps, n, s->d_desc);
    }
    UVO_HIP_TRY(c, hipGetLastError());
    return UVO_OK;
}

uvo_status orb_detect(Ctx* c, const uint8_t* gray, int w, int h, int stride, int mem, uvo_keypoint* kps, uint8_t* desc, int cap, int* n_out)
{
    *n_out = 0;
    if (w < 16 || h < 16 || w > c->max_w || h > c->max_h || stride < w || w > 65535 || h > 65535) { c->err = "uvo_orb_detect: image size outside the context's limits"; return UVO_INVALID_ARG; }
    OrbWs* s = orb_state(c);
    if (desc && !s->has_pattern) { c->err = kOrbNoTable; return UVO_INVALID_ARG; }
    UVO_TRY(orb_plan(c, s, w, h));
    hipStream_t st = c->stream;
    const OrbOut own = { s->d_kps, s->d_desc, kOrbDescBytes, s->cap, 0, true };
    UVO_TRY(orb_run(c, s, st, gray, w, h, stride, mem, desc ? s->d_pattern : nullptr, s->rank_dev, s->counts_dev ? &own : nullptr, n_out));
    const int n = *n_out;
    if (n > s->cap) { c->err = "ORB: more keypoints tie at the per-level cuts than the output list has room for"; return UVO_CAPACITY; }
    if ((kps || desc) && n > cap) { c->err = "uvo_orb_detect: output capacity too small"; return UVO_CAPACITY; }
    if (n == 0) return UVO_OK;
    if (kps) UVO_HIP_TRY(c, hipMemcpyAsync(kps, s->d_kps, sizeof(uvo_keypoint) * n, hipMemcpyDeviceToHost, st));
    if (desc) UVO_HIP_TRY(c, hipMemcpyAsync(desc, s->d_desc, (size_t)kOrbDescBytes * n, hipMemcpyDeviceToHost, st));
    s->stat_waits++;
    UVO_HIP_TRY(c, hipStreamSynchronize(st));
    return UVO_OK;
}

// ---- detect_features' ORB branch inside the fused steps.  The parameters and the sampling table are lane 0's (uvo_orb_configure /
// uvo_orb_set_pattern); each lane keeps its own level buffers, made when a sequence starts.  Both images of a pair go through them in turn.
// With the rankings on the device and the counts there too (uvo_orb_set_ranking 1, uvo_orb_set_counts 1) the whole detection is queued and
// nothing waits: the keypoints and the padded rows go straight to det[slot], the count stays in the workspace's d_rank (*d_n, possibly
// past max_kpts; *d_ovf raised when more keypoints tie at the cuts than the workspace's list holds -- nothing is written past either list)
// and *n = -1: k_binary_publish_dev and the step's count readback report UVO_CAPACITY for either, as they do for AKAZE's device count.
// With counts 0 the submitting thread waits twice per image, for the level counts; with the rankings on the host, three times.
bool orb_has_pattern(Ctx* c)
{
    const OrbWs* s = static_cast<const OrbWs*>(c->sh->lanes[0]->orb_ws);
    return s && s->has_pattern;
}
uvo_status orb_prepare_lane(Ctx* c, int w, int h)
{
    const OrbWs* ms = orb_state(c->sh->lanes[0]);
    OrbWs* s = orb_state(c);
    if (s != ms && memcmp(&s->p, &ms->p, sizeof(OrbParams)) != 0) { s->p = ms->p; orb_free_sized(s); }     // lane 0's configuration
    return orb_plan(c, s, w, h);
}
uvo_status orb_detect_lane(Ctx* c, int slot, int* n, const int** d_n, const int** d_ovf)
{
    const int w = c->img_w, h = c->img_h;
    *n = 0; *d_n = nullptr; *d_ovf = nullptr;
    if (w < 16 || h < 16 || w > 65535 || h > 65535) { c->err = "ORB: image size outside the detector's limits"; return UVO_INVALID_ARG; }
    if (!orb_has_pattern(c)) { c->err = kOrbLoopNoTable; return UVO_INVALID_ARG; }
    UVO_TRY(orb_prepare_lane(c, w, h));                                       // (a no-op once the lane is primed)
    OrbWs* s = static_cast<OrbWs*>(c->orb_ws);
    const OrbWs* ms = static_cast<const OrbWs*>(c->sh->lanes[0]->orb_ws);
    if (ms->rank_dev && ms->counts_dev) {                                     // the master context's values serve every lane
        const OrbOut lo = { c->det[slot].kps, reinterpret_cast<uint8_t*>(c->det[slot].desc), 4 * kBinRowWords, c->cap, slot, false };
        UVO_TRY(orb_run(c, s, c->stream, c->img[slot], w, h, w, UVO_MEM_DEVICE, ms->d_pattern, 1, &lo, n));
        *d_n = s->d_rank + RK_N + slot; *d_ovf = s->d_rank + RK_OVF + slot;
        return UVO_OK;
    }
    UVO_TRY(orb_run(c, s, c->stream, c->img[slot], w, h, w, UVO_MEM_DEVICE, ms->d_pattern, ms->rank_dev, nullptr, n));
    if (*n > c->cap || *n == 0) return UVO_OK;
    UVO_HIP_TRY(c, hipMemcpyAsync(c->det[slot].kps, s->d_kps, sizeof(uvo_keypoint) * (size_t)*n, hipMemcpyDeviceToDevice, c->stream));
    return pad_binary_rows(c, c->stream, s->d_desc, *n, kOrbDescBytes, reinterpret_cast<uint8_t*>(c->det[slot].desc));
}
// intermediates for the parity tests: what = 0 the level's image, 1 its blurred copy (after a detect with descriptors), 2 its FAST score map
uvo_status orb_level_plane(Ctx* c, int level, int what, uint8_t* out, int cap_bytes, int* ow, int* oh)
{
    OrbWs* s = static_cast<OrbWs*>(c->orb_ws);
    if (!s || !s->d_pix || level < 0 || level >= s->L.n || what < 0 || what > 2 || (what == 0 && level == 0)) {
        c->err = "uvo_orb_plane: no such plane (run uvo_orb_detect first; level 0's image is the caller's)"; return UVO_INVALID_ARG;
    }
    *ow = s->L.w[level]; *oh = s->L.h[level];
    const size_t n = (size_t)*ow * *oh;
    if ((size_t)cap_bytes < n) { c->err = "uvo_orb_plane: output capacity too small"; return UVO_CAPACITY; }
    const uint8_t* src = what == 0 ? s->L.img[level] : what == 1 ? s->L.blur[level] : s->L.score[level];
    UVO_HIP_TRY(c, hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    return UVO_OK;
}


uvo_status orb_set_ranking(Ctx* c, int where)
{
    if (where != 0 && where != 1) { c->err = "uvo_orb_set_ranking: 0 (the host replays retainBest's order) or 1 (k_rb_rank on the device)"; return UVO_INVALID_ARG; }
    orb_state(c)->rank_dev = where;
    return UVO_OK;
}
uvo_status orb_set_counts(Ctx* c, int where)
{
    if (where != 0 && where != 1) { c->err = "uvo_orb_set_counts: 0 (the host reads the counts back between launches) or 1 (they stay on the device)"; return UVO_INVALID_ARG; }
    orb_state(c)->counts_dev = where;
    return UVO_OK;
}
// uvo_orb_stats: the stream waits of every lane's ORB detections since the last call (read and cleared); the counts of this context's own
// workspace as they last reached the host
uvo_status orb_stats(Ctx* c, int* host_waits, int* n_fast, int* n_ranked, int* n_keypoints)
{
    int waits = 0;
    for (Ctx* l : c->sh->lanes)
        if (OrbWs* ls = static_cast<OrbWs*>(l->orb_ws)) { waits += ls->stat_waits; ls->stat_waits = 0; }
    const OrbWs* s = static_cast<const OrbWs*>(c->orb_ws);
    if (host_waits) *host_waits = waits;
    if (n_fast) *n_fast = s ? s->stat_fast : -1;
    if (n_ranked) *n_ranked = s ? s->stat_ranked : -1;
    if (n_keypoints) *n_keypoints = s ? s->stat_kps : -1;
    return UVO_OK;
}
// the test hook behind uvo_retain_best: host buffers in and out; where = 1 is the launch orb_run_device makes
uvo_status orb_retain_best(Ctx* c, const float* responses, const int* start, const int* keep, int nseg, int where, int* order, int cap, int* out_start, int* hits)
{
    if (nseg < 1 || nseg > kOrbMaxLevels) { c->err = "uvo_retain_best: 1 .. 16 segments"; return UVO_INVALID_ARG; }
    if (where != 0 && where != 1) { c->err = "uvo_retain_best: where = 0 (host) or 1 (device)"; return UVO_INVALID_ARG; }
    if (start[0] < 0) { c->err = "uvo_retain_best: start[0] is negative"; return UVO_INVALID_ARG; }
    for (int l = 0; l < nseg; l++) {
        if (start[l + 1] < start[l]) { c->err = "uvo_retain_best: start decreases"; return UVO_INVALID_ARG; }
        if (keep[l] < 0) { c->err = "uvo_retain_best: a negative keep"; return UVO_INVALID_ARG; }
    }
    const int total = start[nseg];
    int hit[kOrbMaxLevels] = {0};
    if (where == 0) {
        std::vector<int> out;
        std::vector<RbItem> tmp;
        for (int l = 0; l < nseg; l++) {
            out_start[l] = (int)out.size();
            const long before = rb_heap_select_calls;
            retain_best_order(responses + start[l], start[l + 1] - start[l], keep[l], start[l], &tmp, &out);
            hit[l] = (int)(rb_heap_select_calls - before);
        }
        out_start[nseg] = (int)out.size();
        if ((int)out.size() > cap) { c->err = "uvo_retain_best: output capacity too small"; return UVO_CAPACITY; }
        if (!out.empty()) memcpy(order, out.data(), sizeof(int) * out.size());
    } else {
        const size_t nn = (size_t)std::max(total, 1), ncap = (size_t)std::max(cap, 1);
        float* d_r = nullptr; RbdItem* d_items = nullptr; int *d_la = nullptr, *d_lb = nullptr, *d_order = nullptr, *d_w = nullptr;
        enum { W_META = 0, W_START = 48, W_OUT = 68, W_HIT = 88, W_INTS = 104 };
        int hw[W_INTS] = {0};
        memcpy(hw + W_START, start, sizeof(int) * (nseg + 1));
        bool ok = hipMalloc(reinterpret_cast<void**>(&d_r), sizeof(float) * nn) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_items), sizeof(RbdItem) * nn) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&d_la), sizeof(int) * nn) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_lb), sizeof(int) * nn) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&d_order), sizeof(int) * ncap) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_w), sizeof(hw)) == hipSuccess;
        hipStream_t st = c->stream;
        ok = ok && hipMemcpyAsync(d_w, hw, sizeof(hw), hipMemcpyHostToDevice, st) == hipSuccess &&
             (total == 0 || hipMemcpyAsync(d_r, responses, sizeof(float) * total, hipMemcpyHostToDevice, st) == hipSuccess);
        uvo_status rc = ok ? rb_launch(c, st, d_r, d_w + W_START, keep, nseg, d_items, d_la, d_lb, d_w + W_META, d_order, cap, d_w + W_OUT, d_w + W_HIT) : UVO_HIP_ERROR;
        ok = ok && rc == UVO_OK && hipGetLastError() == hipSuccess && hipMemcpyAsync(hw, d_w, sizeof(hw), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        const int m = ok ? hw[W_OUT + nseg] : 0;
        if (ok && m > 0 && m <= cap) ok = hipMemcpy(order, d_order, sizeof(int) * m, hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(d_r); (void)hipFree(d_items); (void)hipFree(d_la); (void)hipFree(d_lb); (void)hipFree(d_order); (void)hipFree(d_w);
        if (!ok) { c->err = "uvo_retain_best: a HIP call failed"; return UVO_HIP_ERROR; }
        memcpy(out_start, hw + W_OUT, sizeof(int) * (nseg + 1));
        memcpy(hit, hw + W_HIT, sizeof(int) * nseg);
        if (m > cap) { c->err = "uvo_retain_best: output capacity too small"; return UVO_CAPACITY; }
    }
    if (hits) memcpy(hits, hit, sizeof(int) * nseg);
    return UVO_OK;
}

}  // namespace uvo
