// preproc.hip -- get_image on gfx950 (VO_utility.cpp:337-379): the per-frame preprocessing in
// front of the hot path, so that the colour frame is uploaded once and the grey, undistorted, equalised image the
// detector consumes never leaves HBM:
//     cv::resize(INTER_AREA) -> cv::cvtColor(COLOR_RGB2GRAY) -> cv::undistort -> optional cv::CLAHE::apply.
// Integer / fixed-point stages are exact by construction; the float stages keep OpenCV's operation order (area
// resize: taps accumulated in table order per source row, rows accumulated in order; CLAHE blend: the reference
// expression, no FMA contraction).  The undistortion maps depend only on the camera matrices: they are computed once
// (one thread per image row, because the reference advances its running sums by one addition per column) and cached.
//   k_resize_area_c3   : one thread per destination element and channel
//   k_rgb2gray         : (R*9798 + G*19235 + B*3735 + 2^14) >> 15
//   k_undistort_map    : initUndistortRectifyMap per stripe of undistort (CV_16SC2 + 5+5 fraction bits)
//   k_remap_bilinear   : remap INTER_LINEAR, BORDER_CONSTANT 0, 15-bit weights
//   k_clahe_lut        : one workgroup per tile: histogram, clip + redistribute, cumulative LUT
//   k_clahe_apply      : bilinear blend of the four neighbouring tile LUTs
#include "uvo_ctx.h"
#include "uvo_math.h"
#include "uvo_pix.h"
#include <string.h>
#include <math.h>

namespace uvo {

struct PreWs {
    uint8_t *rgb = nullptr, *small = nullptr, *gray = nullptr, *und = nullptr, *out = nullptr;
    int16_t* map1 = nullptr; uint16_t* map2 = nullptr; uint8_t* lut = nullptr;
    size_t cap_in = 0, cap_out = 0;
    uint8_t *raw = nullptr, *bgr3 = nullptr; size_t cap_raw = 0, cap_bgr3 = 0;      // uvo_get_image_fmt(BGRA8): the staged frame, its three channels
    double mapK[9], mapD[4], mapN[9]; int map_w = 0, map_h = 0; bool map_valid = false;
};

// computeResizeAreaTab for one destination index (same as the descriptor stage's table)
struct PTab { int sx1, sx2; float a_first, a_mid, a_last; int has_first, has_last; };
__device__ __forceinline__ PTab p_area_tab(int dx, int ssize, double scale)
{
    PTab t;
    double fsx1 = dx * scale;
    double fsx2 = fsx1 + scale;
    double cellWidth = scale < ssize - fsx1 ? scale : ssize - fsx1;
    int sx1 = cv_ceil_d(fsx1), sx2 = cv_floor_d(fsx2);
    sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
    sx1 = sx1 < sx2 ? sx1 : sx2;
    t.sx1 = sx1; t.sx2 = sx2;
    t.has_first = sx1 - fsx1 > 1e-3;
    t.a_first = (float)((sx1 - fsx1) / cellWidth);
    t.a_mid = (float)(1.0 / cellWidth);
    t.has_last = fsx2 - sx2 > 1e-3;
    double a = fsx2 - sx2; if (a > 1.) a = 1.; if (a > cellWidth) a = cellWidth;
    t.a_last = (float)(a / cellWidth);
    return t;
}
__device__ __forceinline__ uint8_t p_sat_u8(float v) { int iv = cv_round_f(v); return (uint8_t)(iv < 0 ? 0 : iv > 255 ? 255 : iv); }

__global__ __launch_bounds__(256) void k_resize_area_c3(const uint8_t* __restrict__ src, int sw, int sh, int stride,
                                                        uint8_t* __restrict__ dst, int dw, int dh, double scale_x, double scale_y,
                                                        int iscale_x, int iscale_y, int fast)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dw * 3) return;
    const int dx = e / 3, ch = e - dx * 3, dy = blockIdx.y;
    if (fast) {                                          // resizeAreaFast_: integer block sums
        const uint8_t* S = src + (size_t)(dy * iscale_y) * stride + (size_t)(dx * iscale_x) * 3 + ch;
        int sum = 0;
        for (int sy = 0; sy < iscale_y; sy++) for (int sx = 0; sx < iscale_x; sx++) sum += S[(size_t)sy * stride + sx * 3];
        uint8_t r;
        if (iscale_x == 2 && iscale_y == 2) r = (uint8_t)((sum + 2) >> 2);
        else { float sc = 1.f / (iscale_x * iscale_y); r = p_sat_u8(sum * sc); }
        dst[((size_t)dy * dw + dx) * 3 + ch] = r;
        return;
    }
    const PTab tx = p_area_tab(dx, sw, scale_x), ty = p_area_tab(dy, sh, scale_y);
    const int c_begin = tx.has_first ? tx.sx1 - 1 : tx.sx1, c_end = tx.has_last ? tx.sx2 + 1 : tx.sx2;
    const int r_begin = ty.has_first ? ty.sx1 - 1 : ty.sx1, r_end = ty.has_last ? ty.sx2 + 1 : ty.sx2;
    float sum = 0.f;
    for (int r = r_begin; r < r_end; r++) {
        const uint8_t* S = src + (size_t)r * stride + ch;
        float buf = 0.f;
        for (int cc = c_begin; cc < c_end; cc++) {
            float alpha = cc < tx.sx1 ? tx.a_first : (cc < tx.sx2 ? tx.a_mid : tx.a_last);
            buf += S[cc * 3] * alpha;
        }
        float beta = r < ty.sx1 ? ty.a_first : (r < ty.sx2 ? ty.a_mid : ty.a_last);
        sum += beta * buf;
    }
    dst[((size_t)dy * dw + dx) * 3 + ch] = p_sat_u8(sum);
}

__global__ __launch_bounds__(256) void k_rgb2gray(const uint8_t* __restrict__ rgb, int w, int h, int stride, uint8_t* __restrict__ gray)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* s = rgb + (size_t)y * stride + 3 * x;
    gray[(size_t)y * w + x] = (uint8_t)((s[0] * 9798 + s[1] * 19235 + s[2] * 3735 + (1 << 14)) >> 15);
}

struct CamPar { double A[9], D[4], Ar[9]; };

// one thread per image row; stripes of `stripe0` rows re-derive the inverse with Ar(1,2) = v0 - stripe_start
__global__ __launch_bounds__(64) void k_undistort_map(CamPar cp, int cols, int rows, int stripe0, int16_t* __restrict__ map1, uint16_t* __restrict__ map2)
{
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= rows) return;
    const int ys = (y / stripe0) * stripe0, i = y - ys;
    double S[9];
    for (int k = 0; k < 9; k++) S[k] = cp.Ar[k];
    S[5] = cp.Ar[5] - ys;
    double ir[9];
    {   // cv::invert, 3x3 closed form
        double d = S[0]*(S[4]*S[8] - S[5]*S[7]) - S[1]*(S[3]*S[8] - S[5]*S[6]) + S[2]*(S[3]*S[7] - S[4]*S[6]);
        if (d == 0) { for (int k = 0; k < 9; k++) ir[k] = 0; }
        else {
            d = 1./d;
            ir[0] = (S[4]*S[8] - S[5]*S[7]) * d; ir[1] = (S[2]*S[7] - S[1]*S[8]) * d; ir[2] = (S[1]*S[5] - S[2]*S[4]) * d;
            ir[3] = (S[5]*S[6] - S[3]*S[8]) * d; ir[4] = (S[0]*S[8] - S[2]*S[6]) * d; ir[5] = (S[2]*S[3] - S[0]*S[5]) * d;
            ir[6] = (S[3]*S[7] - S[4]*S[6]) * d; ir[7] = (S[1]*S[6] - S[0]*S[7]) * d; ir[8] = (S[0]*S[4] - S[1]*S[3]) * d;
        }
    }
    const double u0 = cp.A[2], v0 = cp.A[5], fx = cp.A[0], fy = cp.A[4];
    const double k1 = cp.D[0], k2 = cp.D[1], p1 = cp.D[2], p2 = cp.D[3];
    const double k3 = 0, k4 = 0, k5 = 0, k6 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    int16_t* m1 = map1 + (size_t)y * cols * 2;
    uint16_t* m2 = map2 + (size_t)y * cols;
    double _x = i*ir[1] + ir[2], _y = i*ir[4] + ir[5], _w = i*ir[7] + ir[8];
    for (int j = 0; j < cols; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        double w = 1./_w, x = _x*w, yy = _y*w;
        double x2 = x*x, y2 = yy*yy;
        double r2 = x2 + y2, _2xy = 2*x*yy;
        double kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2)/(1 + ((k6*r2 + k5)*r2 + k4)*r2);
        double xd = (x*kr + p1*_2xy + p2*(r2 + 2*x2) + s1*r2 + s2*r2*r2);
        double yd = (yy*kr + p1*(r2 + 2*y2) + p2*_2xy + s3*r2 + s4*r2*r2);
        double invProj = 1.0;
        double u = fx*invProj*xd + u0;
        double v = fy*invProj*yd + v0;
        int iu = cv_round_d(u*32), iv = cv_round_d(v*32);
        m1[j*2] = (int16_t)(iu >> 5); m1[j*2 + 1] = (int16_t)(iv >> 5);
        m2[j] = (uint16_t)((iv & 31)*32 + (iu & 31));
    }
}

__global__ __launch_bounds__(256) void k_remap_bilinear(const uint8_t* __restrict__ src, int sw, int sh, const int16_t* __restrict__ map1,
                                                        const uint16_t* __restrict__ map2, uint8_t* __restrict__ dst, int dw, int dh)
{
    const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
    if (dx >= dw) return;
    const size_t o = (size_t)dy * dw + dx;
    const int sx = map1[o * 2], sy = map1[o * 2 + 1];
    const int f = map2[o], fxi = f & 31, fyi = f >> 5;
    const int w00 = (32 - fxi) * (32 - fyi) * 32, w01 = fxi * (32 - fyi) * 32, w10 = (32 - fxi) * fyi * 32, w11 = fxi * fyi * 32;
    int v00 = 0, v01 = 0, v10 = 0, v11 = 0;
    if (sy >= 0 && sy < sh) { if (sx >= 0 && sx < sw) v00 = src[(size_t)sy * sw + sx]; if (sx + 1 >= 0 && sx + 1 < sw) v01 = src[(size_t)sy * sw + sx + 1]; }
    if (sy + 1 >= 0 && sy + 1 < sh) { if (sx >= 0 && sx < sw) v10 = src[(size_t)(sy + 1) * sw + sx]; if (sx + 1 >= 0 && sx + 1 < sw) v11 = src[(size_t)(sy + 1) * sw + sx + 1]; }
    int val = (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15;
    dst[o] = (uint8_t)(val < 0 ? 0 : val > 255 ? 255 : val);
}

__device__ __forceinline__ int p_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) { if (p < 0) p = -p; else p = 2 * (len - 1) - p; }
    return p;
}

// one workgroup per tile (8 x 8 tiles); the image is extended by BORDER_REFLECT_101 when it does not divide
__global__ __launch_bounds__(256) void k_clahe_lut(const uint8_t* __restrict__ src, int w, int h, int tw, int th, int clipLimit, float lutScale,
                                                   uint8_t* __restrict__ lut)
{
    const int k = blockIdx.x, ty = k / 8, tx = k % 8, tid = threadIdx.x;
    __shared__ int hist[256];
    __shared__ int s_red[256];
    hist[tid] = 0;
    __syncthreads();
    for (int e = tid; e < tw * th; e += 256) {
        int y = e / tw, x = e - y * tw;
        int gy = p_reflect101(ty * th + y, h), gx = p_reflect101(tx * tw + x, w);
        atomicAdd(&hist[src[(size_t)gy * w + gx]], 1);
    }
    __syncthreads();
    int hv = hist[tid];
    if (clipLimit > 0) {
        int over = hv > clipLimit ? hv - clipLimit : 0;
        if (hv > clipLimit) hv = clipLimit;
        s_red[tid] = over;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) s_red[tid] += s_red[tid + o]; __syncthreads(); }
        const int clipped = s_red[0];
        const int redistBatch = clipped / 256;
        int residual = clipped - redistBatch * 256;
        hv += redistBatch;
        if (residual != 0) {
            int step = 256 / residual; if (step < 1) step = 1;
            if (tid % step == 0 && tid / step < residual) hv++;          // for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++
        }
        __syncthreads();
    }
    // inclusive prefix sum (integers: any order)
    s_red[tid] = hv;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        int t = tid >= o ? s_red[tid - o] : 0;
        __syncthreads();
        s_red[tid] += t;
        __syncthreads();
    }
    lut[(size_t)k * 256 + tid] = p_sat_u8(s_red[tid] * lutScale);
}

__global__ __launch_bounds__(256) void k_clahe_apply(const uint8_t* __restrict__ src, int w, int h, int tw, int th, const uint8_t* __restrict__ lut,
                                                     uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float inv_tw = 1.0f / tw, inv_th = 1.0f / th;
    float tyf = y * inv_th - 0.5f;
    int ty1 = (int)floorf(tyf), ty2 = ty1 + 1;
    float ya = tyf - ty1, ya1 = 1.0f - ya;
    ty1 = ty1 > 0 ? ty1 : 0; ty2 = ty2 < 7 ? ty2 : 7;
    float txf = x * inv_tw - 0.5f;
    int tx1 = (int)floorf(txf), tx2 = tx1 + 1;
    float xa = txf - tx1, xa1 = 1.0f - xa;
    tx1 = tx1 > 0 ? tx1 : 0; tx2 = tx2 < 7 ? tx2 : 7;
    const int sv = src[(size_t)y * w + x];
    const uint8_t* p1 = lut + (size_t)ty1 * 8 * 256;
    const uint8_t* p2 = lut + (size_t)ty2 * 8 * 256;
    const int ind1 = tx1 * 256 + sv, ind2 = tx2 * 256 + sv;
    float res = (p1[ind1] * xa1 + p1[ind2] * xa) * ya1 + (p2[ind1] * xa1 + p2[ind2] * xa) * ya;
    dst[(size_t)y * w + x] = p_sat_u8(res);
}

void pre_ws_free(Ctx* c)
{
    PreWs* p = static_cast<PreWs*>(c->pre_ws);
    if (!p) return;
    void* ptrs[] = { p->rgb, p->small, p->gray, p->und, p->out, p->map1, p->map2, p->lut, p->raw, p->bgr3 };
    for (void* q : ptrs) (void)hipFree(q);
    delete p;
    c->pre_ws = nullptr;
}

// get_image: result in ws->out (device), dims returned
uvo_status pre_get_image(Ctx* c, const uint8_t* rgb, int w, int h, int stride, int mem, const double* K, const double* dist4, const double* newK,
                         int desired_width, int clahe_on, int clip_limit, const uint8_t** d_out, int* out_w, int* out_h)
{
    if (w <= 0 || h <= 0 || desired_width <= 0 || stride < 3 * w) { c->err = "get_image: bad geometry"; return UVO_INVALID_ARG; }
    const double ratio = (double)w / (double)desired_width;
    const int dw = desired_width, dh = (int)(h / ratio);
    if (dw > w || dh > h || dh <= 0) { c->err = "get_image: enlarging (OpenCV switches INTER_AREA to bilinear there) is not provided"; return UVO_INVALID_ARG; }
    hipStream_t st = c->stream;
    PreWs* p = static_cast<PreWs*>(c->pre_ws);
    if (!p) { p = new PreWs(); c->pre_ws = p; }
    const size_t n_in = (size_t)h * stride, n_out = (size_t)dw * dh;
    if (n_in > p->cap_in) {
        (void)hipFree(p->rgb); p->rgb = nullptr;
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->rgb), n_in));
        p->cap_in = n_in;
    }
    if (n_out > p->cap_out) {
        void* old[] = { p->small, p->gray, p->und, p->out, p->map1, p->map2 };
        for (void* q : old) (void)hipFree(q);
        p->small = p->gray = p->und = p->out = nullptr; p->map1 = nullptr; p->map2 = nullptr; p->map_valid = false;
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->small), n_out * 3));
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->gray), n_out));
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->und), n_out));
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->out), n_out));
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->map1), n_out * 2 * sizeof(int16_t)));
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->map2), n_out * sizeof(uint16_t)));
        p->cap_out = n_out;
    }
    if (!p->lut) UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->lut), 64 * 256));
    const uint8_t* d_rgb = rgb;
    int d_stride = stride;
    if (mem != UVO_MEM_DEVICE) {
        UVO_HIP_TRY(c, hipMemcpyAsync(p->rgb, rgb, n_in, hipMemcpyHostToDevice, st));
        d_rgb = p->rgb;
    }
    if (w == dw && h == dh) {
        hipLaunchKernelGGL(k_rgb2gray, dim3((dw + 255) / 256, dh), dim3(256), 0, st, d_rgb, dw, dh, d_stride, p->gray);
    } else {
        const double inv_scale_x = (double)dw / w, inv_scale_y = (double)dh / h;
        const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
        const int iscale_x = cv_round_d(scale_x), iscale_y = cv_round_d(scale_y);
        const int fast = fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON;
        hipLaunchKernelGGL(k_resize_area_c3, dim3((dw * 3 + 255) / 256, dh), dim3(256), 0, st, d_rgb, w, h, d_stride, p->small, dw, dh,
                           scale_x, scale_y, iscale_x, iscale_y, fast);
        hipLaunchKernelGGL(k_rgb2gray, dim3((dw + 255) / 256, dh), dim3(256), 0, st, p->small, dw, dh, dw * 3, p->gray);
    }
    if (!p->map_valid || p->map_w != dw || p->map_h != dh || memcmp(p->mapK, K, sizeof(p->mapK)) || memcmp(p->mapD, dist4, sizeof(p->mapD)) ||
        memcmp(p->mapN, newK, sizeof(p->mapN))) {
        CamPar cp;
        memcpy(cp.A, K, sizeof(cp.A)); memcpy(cp.D, dist4, sizeof(cp.D)); memcpy(cp.Ar, newK, sizeof(cp.Ar));
        int stripe0 = (1 << 12) / (dw > 1 ? dw : 1);
        if (stripe0 < 1) stripe0 = 1;
        if (stripe0 > dh) stripe0 = dh;
        hipLaunchKernelGGL(k_undistort_map, dim3((dh + 63) / 64), dim3(64), 0, st, cp, dw, dh, stripe0, p->map1, p->map2);
        memcpy(p->mapK, K, sizeof(p->mapK)); memcpy(p->mapD, dist4, sizeof(p->mapD)); memcpy(p->mapN, newK, sizeof(p->mapN));
        p->map_w = dw; p->map_h = dh; p->map_valid = true;
    }
    hipLaunchKernelGGL(k_remap_bilinear, dim3((dw + 255) / 256, dh), dim3(256), 0, st, p->gray, dw, dh, p->map1, p->map2, p->und, dw, dh);
    const uint8_t* result = p->und;
    if (clahe_on) {
        // clahe.cpp: if either side does not divide into 8 tiles BOTH are extended by 8 - (size % 8) (reflect-101) -- that is
        // a full 8 on the side that did divide
        const bool ext = dw % 8 != 0 || dh % 8 != 0;
        const int ew = ext ? dw + (8 - dw % 8) : dw, eh = ext ? dh + (8 - dh % 8) : dh;
        const int tw = ew / 8, th = eh / 8, total = tw * th;
        const float lutScale = (float)255 / total;
        int clipLimit = 0;
        if ((double)clip_limit > 0.0) { clipLimit = (int)((double)clip_limit * total / 256); if (clipLimit < 1) clipLimit = 1; }
        hipLaunchKernelGGL(k_clahe_lut, dim3(64), dim3(256), 0, st, p->und, dw, dh, tw, th, clipLimit, lutScale, p->lut);
        hipLaunchKernelGGL(k_clahe_apply, dim3((dw + 255) / 256, dh), dim3(256), 0, st, p->und, dw, dh, tw, th, p->lut, p->out);
        result = p->out;
    }
    UVO_HIP_TRY(c, hipGetLastError());
    *d_out = result; *out_w = dw; *out_h = dh;
    return UVO_OK;
}

// uvo_get_image_fmt's BGRA8 frames: the operator composes -- every fourth byte dropped into a tight w x h x 3 picture, then pre_get_image
// (the loop entries read BGRA8 in place instead: k_fr_resize_gray<kPixBGRA8>)
__global__ __launch_bounds__(256) void k_bgra_drop_alpha(const uint8_t* __restrict__ src, int w, int h, int stride, uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* s = src + (size_t)y * stride + 4 * (size_t)x;
    uint8_t* o = dst + ((size_t)y * w + x) * 3;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
}
uvo_status pre_drop_alpha(Ctx* c, const uint8_t* bgra, int w, int h, int stride, int mem, const uint8_t** d_bgr)
{
    PreWs* p = static_cast<PreWs*>(c->pre_ws);
    if (!p) { p = new PreWs(); c->pre_ws = p; }
    const size_t n_raw = mem == UVO_MEM_DEVICE ? 0 : (size_t)h * stride, n3 = (size_t)w * h * 3;
    if (n_raw > p->cap_raw) {
        (void)hipFree(p->raw); p->raw = nullptr; p->cap_raw = 0;
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->raw), n_raw));
        p->cap_raw = n_raw;
    }
    if (n3 > p->cap_bgr3) {
        (void)hipFree(p->bgr3); p->bgr3 = nullptr; p->cap_bgr3 = 0;
        UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&p->bgr3), n3));
        p->cap_bgr3 = n3;
    }
    const uint8_t* d_src = bgra;
    if (mem != UVO_MEM_DEVICE) {
        UVO_HIP_TRY(c, hipMemcpyAsync(p->raw, bgra, n_raw, hipMemcpyHostToDevice, c->stream));
        d_src = p->raw;
    }
    hipLaunchKernelGGL(k_bgra_drop_alpha, dim3((w + 255) / 256, h), dim3(256), 0, c->stream, d_src, w, h, stride, p->bgr3);
    UVO_HIP_TRY(c, hipGetLastError());
    *d_bgr = p->bgr3;
    return UVO_OK;
}

// ------------------------------------------------------------------------------------------ camera frames into the loops' lanes
// get_image in front of detect_features INSIDE a loop entry (uvo_stereo_*_frames / uvo_mono_*_frames): the same four stages, queued on
// the entry's lane's stage-A stream, both cameras of a pair per launch (blockIdx.y = image, as the detector's ImgPair), the last
// kernel writing the lane's detector image (Ctx::d_img).  Every image is addressed as a flat array of w * h bytes and a thread
// owns four consecutive ones, so each store is one aligned dword whatever the width (the buffers come from hipMalloc; the last,
// partial quad of an image is stored bytewise).  Arithmetic per pixel is the single-image kernels' above, statement for statement:
//   k_fr_resize_gray : k_resize_area_c3's three channel values (fast / table path, saturated to u8), then k_rgb2gray's fixed point;
//                      one instance per pixel layout of the frame (uvo_ctx_set_camera_format): BGR8, BGRA8 (three of four bytes) and
//                      BAYER_BGGR8 (the three values of a source pixel demosaiced from the mosaic's 3 x 3 neighbourhood, uvo_pix.h)
//   k_fr_remap       : k_remap_bilinear, maps of the image's camera
//   k_fr_clahe_lut   : k_clahe_lut, 64 workgroups per image
//   k_fr_clahe_apply : k_clahe_apply
// The undistortion maps live in lane 0's workspace, one slot per camera (uvo_ctx_set_camera): built by k_undistort_map on
// lane 0's stream once per (camera parameters, output size) and complete (host sync) before a lane's kernels are queued.
struct FrImg {
    const uint8_t* src; uint8_t* gray;            // the colour frame (device), its grey image at the output size
    const int16_t* map1; const uint16_t* map2;
    uint8_t* und;                                 // the remap's destination: the CLAHE input, or the lane's detector image when CLAHE is off
    uint8_t* lut; uint8_t* out;                   // 64 x 256 tile LUTs; the lane's detector image
    int clahe, clipLimit;
};
struct FrPair { FrImg im[2]; };

struct FrCam {
    bool set = false;
    double K[9], D[4], N[9]; int desired_width = 0, clahe = 0, clip = 0;
    int fmt = kPixBGR8;                           // the layout of this camera's frames (uvo_ctx_set_camera_format); kept whether or not the camera is set
    int16_t* map1 = nullptr; uint16_t* map2 = nullptr; size_t map_cap = 0; int map_w = 0, map_h = 0; bool map_valid = false;
};
struct FramesWs {
    FrCam cam[2];                                 // used in lane 0's workspace only
    uint8_t *rgb[2] = {nullptr, nullptr}, *gray[2] = {nullptr, nullptr}, *und[2] = {nullptr, nullptr}, *lut = nullptr;   // per lane
    size_t cap_in = 0, cap_out = 0;
};

__device__ __forceinline__ void fr_store4(uint8_t* dst, size_t o0, size_t n, const uint8_t* g)
{
    if (o0 + 4 <= n) *reinterpret_cast<uint32_t*>(dst + o0) = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16) | ((uint32_t)g[3] << 24);
    else for (size_t k = 0; o0 + k < n; k++) dst[o0 + k] = g[k];
}
__device__ __forceinline__ uint8_t fr_gray(int r, int g, int b) { return (uint8_t)((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15); }

// The three source samples of source pixel (x, y) that get_image's grey weights 9798 / 19235 / 3735 multiply (channels 0, 1, 2), per
// pixel layout: BGR8 and BGRA8 read them (BGRA8 skips every fourth byte), BAYER_BGGR8 computes them from the mosaic's 3 x 3
// neighbourhood with k_bayer_bggr's own statement (uvo_pix.h) -- no w x h x 3 picture exists on that route.
template <int F> __device__ __forceinline__ void fr_fetch(const uint8_t* __restrict__ src, int sw, int sh, int stride, int x, int y, int& c0, int& c1, int& c2)
{
    if constexpr (F == kPixBayerBGGR8) pix_bayer_bggr(src, sw, sh, stride, x, y, c0, c1, c2);
    else {
        const uint8_t* s = src + (size_t)y * stride + (F == kPixBGRA8 ? 4 : 3) * x;
        c0 = s[0]; c1 = s[1]; c2 = s[2];
    }
}

// mode 0: no resize, 1: resizeAreaFast_ (integer scale), 2: the table path.  One instance per pixel layout F (UVO_PIX_*).  The BGR8
// instance keeps the statements the kernel had before it took a layout (its code is the former kernel's, instruction for instruction);
// the other two go through fr_fetch.
template <int F>
__global__ __launch_bounds__(256) void k_fr_resize_gray(FrPair fp, int sw, int sh, int stride, int dw, int dh, double scale_x, double scale_y,
                                                        int iscale_x, int iscale_y, int mode)
{
    const FrImg& im = fp.im[blockIdx.y];
    const size_t n = (size_t)dw * dh, o0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (o0 >= n) return;
    int dy = (int)(o0 / dw), dx = (int)(o0 - (size_t)dy * dw);
    uint8_t g[4] = {0, 0, 0, 0};
    if constexpr (F == kPixBGR8) {
        if (mode == 0 && dx + 4 <= dw && ((reinterpret_cast<uintptr_t>(im.src) | (unsigned)stride) & 3u) == 0 && (dx & 3) == 0) {
            // twelve bytes of one row, dword aligned
            const uint32_t* s = reinterpret_cast<const uint32_t*>(im.src + (size_t)dy * stride + 3 * dx);
            const uint32_t a = s[0], b = s[1], c = s[2];
            g[0] = fr_gray(a & 255, (a >> 8) & 255, (a >> 16) & 255);
            g[1] = fr_gray(a >> 24, b & 255, (b >> 8) & 255);
            g[2] = fr_gray((b >> 16) & 255, b >> 24, c & 255);
            g[3] = fr_gray((c >> 8) & 255, (c >> 16) & 255, c >> 24);
            fr_store4(im.gray, o0, n, g);
            return;
        }
    }
    if constexpr (F == kPixBGRA8) {
        if (mode == 0 && dx + 4 <= dw && ((reinterpret_cast<uintptr_t>(im.src) | (unsigned)stride) & 3u) == 0) {
            // sixteen bytes of one row, one dword per pixel (4 * dx is a multiple of four whatever dx is)
            const uint32_t* s = reinterpret_cast<const uint32_t*>(im.src + (size_t)dy * stride + 4 * dx);
            for (int k = 0; k < 4; k++) { const uint32_t a = s[k]; g[k] = fr_gray(a & 255, (a >> 8) & 255, (a >> 16) & 255); }
            fr_store4(im.gray, o0, n, g);
            return;
        }
    }
    PTab ty = {};
    int ty_row = -1;
    for (int k = 0; k < 4 && o0 + k < n; k++) {
        int ch3[3];
        if (mode == 0) {
            if constexpr (F == kPixBGR8) {
                const uint8_t* s = im.src + (size_t)dy * stride + 3 * dx;
                ch3[0] = s[0]; ch3[1] = s[1]; ch3[2] = s[2];
            } else fr_fetch<F>(im.src, sw, sh, stride, dx, dy, ch3[0], ch3[1], ch3[2]);
        } else if (mode == 1) {                                  // resizeAreaFast_: integer block sums
            int sum[3] = {0, 0, 0};
            if constexpr (F == kPixBGR8) {
                const uint8_t* S = im.src + (size_t)(dy * iscale_y) * stride + (size_t)(dx * iscale_x) * 3;
                for (int sy = 0; sy < iscale_y; sy++) for (int sx = 0; sx < iscale_x; sx++) {
                    const uint8_t* q = S + (size_t)sy * stride + sx * 3;
                    sum[0] += q[0]; sum[1] += q[1]; sum[2] += q[2];
                }
            } else {
                const int x0 = dx * iscale_x, y0 = dy * iscale_y;
                for (int sy = 0; sy < iscale_y; sy++) for (int sx = 0; sx < iscale_x; sx++) {
                    int q0, q1, q2;
                    fr_fetch<F>(im.src, sw, sh, stride, x0 + sx, y0 + sy, q0, q1, q2);
                    sum[0] += q0; sum[1] += q1; sum[2] += q2;
                }
            }
            if (iscale_x == 2 && iscale_y == 2) for (int ch = 0; ch < 3; ch++) ch3[ch] = (uint8_t)((sum[ch] + 2) >> 2);
            else { const float sc = 1.f / (iscale_x * iscale_y); for (int ch = 0; ch < 3; ch++) ch3[ch] = p_sat_u8(sum[ch] * sc); }
        } else {
            const PTab tx = p_area_tab(dx, sw, scale_x);
            if (ty_row != dy) { ty = p_area_tab(dy, sh, scale_y); ty_row = dy; }
            const int c_begin = tx.has_first ? tx.sx1 - 1 : tx.sx1, c_end = tx.has_last ? tx.sx2 + 1 : tx.sx2;
            const int r_begin = ty.has_first ? ty.sx1 - 1 : ty.sx1, r_end = ty.has_last ? ty.sx2 + 1 : ty.sx2;
            float sum[3] = {0.f, 0.f, 0.f};
            for (int r = r_begin; r < r_end; r++) {
                float buf[3] = {0.f, 0.f, 0.f};
                if constexpr (F == kPixBGR8) {
                    const uint8_t* S = im.src + (size_t)r * stride;
                    for (int cc = c_begin; cc < c_end; cc++) {
                        const float alpha = cc < tx.sx1 ? tx.a_first : (cc < tx.sx2 ? tx.a_mid : tx.a_last);
                        buf[0] += S[cc * 3] * alpha; buf[1] += S[cc * 3 + 1] * alpha; buf[2] += S[cc * 3 + 2] * alpha;
                    }
                } else {
                    for (int cc = c_begin; cc < c_end; cc++) {
                        const float alpha = cc < tx.sx1 ? tx.a_first : (cc < tx.sx2 ? tx.a_mid : tx.a_last);
                        int q0, q1, q2;
                        fr_fetch<F>(im.src, sw, sh, stride, cc, r, q0, q1, q2);
                        buf[0] += q0 * alpha; buf[1] += q1 * alpha; buf[2] += q2 * alpha;
                    }
                }
                const float beta = r < ty.sx1 ? ty.a_first : (r < ty.sx2 ? ty.a_mid : ty.a_last);
                sum[0] += beta * buf[0]; sum[1] += beta * buf[1]; sum[2] += beta * buf[2];
            }
            for (int ch = 0; ch < 3; ch++) ch3[ch] = p_sat_u8(sum[ch]);
        }
        g[k] = fr_gray(ch3[0], ch3[1], ch3[2]);
        if (++dx == dw) { dx = 0; dy++; }
    }
    fr_store4(im.gray, o0, n, g);
}

__global__ __launch_bounds__(256) void k_fr_remap(FrPair fp, int w, int h)
{
    const FrImg& im = fp.im[blockIdx.y];
    const size_t n = (size_t)w * h, o0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (o0 >= n) return;
    const uint8_t* src = im.gray;
    uint8_t g[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4 && o0 + k < n; k++) {
        const size_t o = o0 + k;
        const int sx = im.map1[o * 2], sy = im.map1[o * 2 + 1];
        const int f = im.map2[o], fxi = f & 31, fyi = f >> 5;
        const int w00 = (32 - fxi) * (32 - fyi) * 32, w01 = fxi * (32 - fyi) * 32, w10 = (32 - fxi) * fyi * 32, w11 = fxi * fyi * 32;
        int v00 = 0, v01 = 0, v10 = 0, v11 = 0;
        if (sy >= 0 && sy < h) { if (sx >= 0 && sx < w) v00 = src[(size_t)sy * w + sx]; if (sx + 1 >= 0 && sx + 1 < w) v01 = src[(size_t)sy * w + sx + 1]; }
        if (sy + 1 >= 0 && sy + 1 < h) { if (sx >= 0 && sx < w) v10 = src[(size_t)(sy + 1) * w + sx]; if (sx + 1 >= 0 && sx + 1 < w) v11 = src[(size_t)(sy + 1) * w + sx + 1]; }
        const int val = (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15;
        g[k] = (uint8_t)(val < 0 ? 0 : val > 255 ? 255 : val);
    }
    fr_store4(im.und, o0, n, g);
}

// one workgroup per tile and image
__global__ __launch_bounds__(256) void k_fr_clahe_lut(FrPair fp, int w, int h, int tw, int th, float lutScale)
{
    const FrImg& im = fp.im[blockIdx.y];
    if (!im.clahe) return;
    const uint8_t* src = im.und;
    const int clipLimit = im.clipLimit;
    const int k = blockIdx.x, ty = k / 8, tx = k % 8, tid = threadIdx.x;
    __shared__ int hist[256];
    __shared__ int s_red[256];
    hist[tid] = 0;
    __syncthreads();
    for (int e = tid; e < tw * th; e += 256) {
        int y = e / tw, x = e - y * tw;
        int gy = p_reflect101(ty * th + y, h), gx = p_reflect101(tx * tw + x, w);
        atomicAdd(&hist[src[(size_t)gy * w + gx]], 1);
    }
    __syncthreads();
    int hv = hist[tid];
    if (clipLimit > 0) {
        int over = hv > clipLimit ? hv - clipLimit : 0;
        if (hv > clipLimit) hv = clipLimit;
        s_red[tid] = over;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) s_red[tid] += s_red[tid + o]; __syncthreads(); }
        const int clipped = s_red[0];
        const int redistBatch = clipped / 256;
        int residual = clipped - redistBatch * 256;
        hv += redistBatch;
        if (residual != 0) {
            int step = 256 / residual; if (step < 1) step = 1;
            if (tid % step == 0 && tid / step < residual) hv++;
        }
        __syncthreads();
    }
    s_red[tid] = hv;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        int t = tid >= o ? s_red[tid - o] : 0;
        __syncthreads();
        s_red[tid] += t;
        __syncthreads();
    }
    im.lut[(size_t)k * 256 + tid] = p_sat_u8(s_red[tid] * lutScale);
}

__global__ __launch_bounds__(256) void k_fr_clahe_apply(FrPair fp, int w, int h, int tw, int th)
{
    const FrImg& im = fp.im[blockIdx.y];
    if (!im.clahe) return;
    const size_t n = (size_t)w * h, o0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (o0 >= n) return;
    int y = (int)(o0 / w), x = (int)(o0 - (size_t)y * w);
    const float inv_tw = 1.0f / tw, inv_th = 1.0f / th;
    uint8_t g[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4 && o0 + k < n; k++) {
        float tyf = y * inv_th - 0.5f;
        int ty1 = (int)floorf(tyf), ty2 = ty1 + 1;
        float ya = tyf - ty1, ya1 = 1.0f - ya;
        ty1 = ty1 > 0 ? ty1 : 0; ty2 = ty2 < 7 ? ty2 : 7;
        float txf = x * inv_tw - 0.5f;
        int tx1 = (int)floorf(txf), tx2 = tx1 + 1;
        float xa = txf - tx1, xa1 = 1.0f - xa;
        tx1 = tx1 > 0 ? tx1 : 0; tx2 = tx2 < 7 ? tx2 : 7;
        const int sv = im.und[o0 + k];
        const uint8_t* p1 = im.lut + (size_t)ty1 * 8 * 256;
        const uint8_t* p2 = im.lut + (size_t)ty2 * 8 * 256;
        const int ind1 = tx1 * 256 + sv, ind2 = tx2 * 256 + sv;
        float res = (p1[ind1] * xa1 + p1[ind2] * xa) * ya1 + (p2[ind1] * xa1 + p2[ind2] * xa) * ya;
        g[k] = p_sat_u8(res);
        if (++x == w) { x = 0; y++; }
    }
    fr_store4(im.out, o0, n, g);
}

void frames_ws_free(Ctx* c)
{
    FramesWs* f = static_cast<FramesWs*>(c->frames_ws);
    if (!f) return;
    void* ptrs[] = { f->rgb[0], f->rgb[1], f->gray[0], f->gray[1], f->und[0], f->und[1], f->lut, f->cam[0].map1, f->cam[0].map2, f->cam[1].map1, f->cam[1].map2 };
    for (void* q : ptrs) (void)hipFree(q);
    delete f;
    c->frames_ws = nullptr;
}
static FramesWs* frames_ws(Ctx* c)
{
    if (!c->frames_ws) c->frames_ws = new FramesWs();
    return static_cast<FramesWs*>(c->frames_ws);
}

uvo_status frames_set_camera(Ctx* m, int cam, const double* K, const double* dist4, const double* newK, int desired_width, int clahe, int clip_limit)
{
    FrCam& fc = frames_ws(m)->cam[cam];
    if (fc.set && (memcmp(fc.K, K, sizeof(fc.K)) || memcmp(fc.D, dist4, sizeof(fc.D)) || memcmp(fc.N, newK, sizeof(fc.N)))) fc.map_valid = false;
    memcpy(fc.K, K, sizeof(fc.K)); memcpy(fc.D, dist4, sizeof(fc.D)); memcpy(fc.N, newK, sizeof(fc.N));
    fc.desired_width = desired_width; fc.clahe = clahe != 0; fc.clip = clip_limit;
    fc.set = true;
    return UVO_OK;
}
uvo_status frames_set_camera_format(Ctx* m, int cam, int fmt)
{
    frames_ws(m)->cam[cam].fmt = fmt;
    return UVO_OK;
}

// What a frames entry needs before anything is queued: the cameras (ncam = 1: camera 0 only), get_image's geometry, the output
// against the context's limits, the cameras' maps and every lane's workspace.  Maps and workspaces are made when the first frame of
// a size arrives -- a sequence's synchronous init entry, where prime_lanes makes the lanes' other per-size state -- and never while
// entries are in flight: lanes read the maps.
// *fmt: the layout the frames are read in; kPixOfCamera on entry asks for the cameras' own (one for both cameras of a stereo entry).
uvo_status frames_plan(Ctx* m, int ncam, int* fmt, int w, int h, int stride, int mem, int* out_w, int* out_h)
{
    FramesWs* f = frames_ws(m);
    for (int i = 0; i < ncam; i++)
        if (!f->cam[i].set) { m->err = i == 0 ? "camera 0 is not set (uvo_ctx_set_camera)" : "camera 1 (right) is not set (uvo_ctx_set_camera): the stereo frames calls need both"; return UVO_INVALID_ARG; }
    if (*fmt == kPixOfCamera) {
        if (ncam == 2 && f->cam[0].fmt != f->cam[1].fmt) { m->err = "the two cameras have different pixel formats (uvo_ctx_set_camera_format): a stereo entry reads both frames in one layout"; return UVO_INVALID_ARG; }
        *fmt = f->cam[0].fmt;
    }
    const int bpp = pix_bpp(*fmt);
    int dw = 0, dh = 0;
    for (int i = 0; i < ncam; i++) {
        const int desired_width = f->cam[i].desired_width;
        if (w <= 0 || h <= 0 || desired_width <= 0 || stride < bpp * w) {
            m->err = bpp == 3 ? "get_image: bad geometry (stride < 3 * w?)" : bpp == 4 ? "get_image: bad geometry (BGRA8 frames: stride < 4 * w?)" : "get_image: bad geometry (Bayer mosaics: stride < w?)";
            return UVO_INVALID_ARG;
        }
        const double ratio = (double)w / (double)desired_width;
        const int cw = desired_width, ch = (int)(h / ratio);
        if (cw > w || ch > h || ch <= 0) { m->err = "get_image: enlarging (desired_width > w; OpenCV switches INTER_AREA to bilinear there) is not provided"; return UVO_INVALID_ARG; }
        if (i == 1 && (cw != dw || ch != dh)) { m->err = "left/right image sizes differ (the cameras' desired_width)"; return UVO_INVALID_ARG; }
        dw = cw; dh = ch;
    }
    if (dw > m->max_w || dh > m->max_h) {
        char buf[160];
        snprintf(buf, sizeof(buf), "get_image's output %d x %d exceeds the context's max_w x max_h %d x %d", dw, dh, m->max_w, m->max_h);
        m->err = buf;
        return UVO_INVALID_ARG;
    }
    const size_t n_out = (size_t)dw * dh, n_in = mem == UVO_MEM_DEVICE ? 0 : (size_t)h * stride;
    bool stale = false, grow = false;
    for (int i = 0; i < ncam; i++) stale = stale || !f->cam[i].map_valid || f->cam[i].map_w != dw || f->cam[i].map_h != dh;
    for (Ctx* l : m->sh->lanes) { const FramesWs* lf = static_cast<const FramesWs*>(l->frames_ws); grow = grow || !lf || lf->cap_out < n_out || lf->cap_in < n_in; }
    if (!stale && !grow) { *out_w = dw; *out_h = dh; return UVO_OK; }
    if (m->sh->n_pending != 0) {
        m->err = stale ? "the frame size or a camera changed while entries are in flight: collect first (the lanes read the cameras' maps)"
                       : "the lanes' frame workspaces must grow (first frames from host memory, or a larger frame / stride) while entries are in flight: collect first";
        return UVO_INVALID_ARG;
    }
    for (int i = 0; i < ncam; i++) {
        FrCam& fc = f->cam[i];
        if (fc.map_valid && fc.map_w == dw && fc.map_h == dh) continue;
        if (fc.map_cap < n_out) {
            (void)hipFree(fc.map1); (void)hipFree(fc.map2); fc.map1 = nullptr; fc.map2 = nullptr; fc.map_cap = 0;
            UVO_HIP_TRY(m, hipMalloc(reinterpret_cast<void**>(&fc.map1), n_out * 2 * sizeof(int16_t)));
            UVO_HIP_TRY(m, hipMalloc(reinterpret_cast<void**>(&fc.map2), n_out * sizeof(uint16_t)));
            fc.map_cap = n_out;
        }
        CamPar cp;
        memcpy(cp.A, fc.K, sizeof(cp.A)); memcpy(cp.D, fc.D, sizeof(cp.D)); memcpy(cp.Ar, fc.N, sizeof(cp.Ar));
        int stripe0 = (1 << 12) / (dw > 1 ? dw : 1);
        if (stripe0 < 1) stripe0 = 1;
        if (stripe0 > dh) stripe0 = dh;
        hipLaunchKernelGGL(k_undistort_map, dim3((dh + 63) / 64), dim3(64), 0, m->stream, cp, dw, dh, stripe0, fc.map1, fc.map2);
        UVO_HIP_TRY(m, hipGetLastError());
        fc.map_w = dw; fc.map_h = dh; fc.map_valid = true;
    }
    UVO_HIP_TRY(m, hipStreamSynchronize(m->stream));
    for (Ctx* l : m->sh->lanes) {
        FramesWs* lf = frames_ws(l);
        if (lf->cap_in < n_in) {
            for (int i = 0; i < 2; i++) { (void)hipFree(lf->rgb[i]); lf->rgb[i] = nullptr; }
            lf->cap_in = 0;
            for (int i = 0; i < 2; i++) UVO_HIP_TRY(m, hipMalloc(reinterpret_cast<void**>(&lf->rgb[i]), n_in));
            lf->cap_in = n_in;
        }
        if (lf->cap_out < n_out) {
            for (int i = 0; i < 2; i++) { (void)hipFree(lf->gray[i]); (void)hipFree(lf->und[i]); lf->gray[i] = lf->und[i] = nullptr; }
            lf->cap_out = 0;
            for (int i = 0; i < 2; i++) {
                UVO_HIP_TRY(m, hipMalloc(reinterpret_cast<void**>(&lf->gray[i]), n_out));
                UVO_HIP_TRY(m, hipMalloc(reinterpret_cast<void**>(&lf->und[i]), n_out));
            }
            lf->cap_out = n_out;
        }
        if (!lf->lut) UVO_HIP_TRY(m, hipMalloc(reinterpret_cast<void**>(&lf->lut), 2 * 64 * 256));
    }
    *out_w = dw; *out_h = dh;
    return UVO_OK;
}

// get_image of the entry's ncam frames on lane L's stream, into L->d_img[0 .. ncam-1]: at most four launches, no host sync
uvo_status frames_queue(Ctx* m, Ctx* L, int ncam, int fmt, const uint8_t* const* rgb, int w, int h, int stride, int mem, int dw, int dh)
{
    const FramesWs* f = static_cast<const FramesWs*>(m->frames_ws);
    const FramesWs* lf = static_cast<const FramesWs*>(L->frames_ws);
    hipStream_t st = L->stream;
    const bool ext = dw % 8 != 0 || dh % 8 != 0;                  // clahe.cpp: both sides are extended when either does not divide
    const int ew = ext ? dw + (8 - dw % 8) : dw, eh = ext ? dh + (8 - dh % 8) : dh;
    const int tw = ew / 8, th = eh / 8, total = tw * th;
    const float lutScale = (float)255 / total;
    FrPair fp;
    bool any_clahe = false;
    for (int i = 0; i < 2; i++) {
        const int s = i < ncam ? i : 0;
        const FrCam& fc = f->cam[s];
        FrImg& im = fp.im[i];
        im.src = rgb[s];
        if (mem != UVO_MEM_DEVICE) {
            if (i < ncam) UVO_HIP_TRY(L, hipMemcpyAsync(lf->rgb[i], rgb[i], (size_t)h * stride, hipMemcpyHostToDevice, st));
            im.src = lf->rgb[s];
        }
        im.gray = lf->gray[s]; im.map1 = fc.map1; im.map2 = fc.map2;
        im.lut = lf->lut + (size_t)s * 64 * 256; im.out = L->d_img[s];
        im.clahe = fc.clahe;
        im.und = fc.clahe ? lf->und[s] : L->d_img[s];
        im.clipLimit = 0;
        if ((double)fc.clip > 0.0) { im.clipLimit = (int)((double)fc.clip * total / 256); if (im.clipLimit < 1) im.clipLimit = 1; }
        if (i < ncam) any_clahe = any_clahe || fc.clahe;
    }
    const unsigned quads = (unsigned)(((size_t)dw * dh + 3) / 4), gx = (quads + 255) / 256;
    int mode = 0, iscale_x = 1, iscale_y = 1;
    double scale_x = 1., scale_y = 1.;
    if (!(w == dw && h == dh)) {
        const double inv_scale_x = (double)dw / w, inv_scale_y = (double)dh / h;
        scale_x = 1. / inv_scale_x; scale_y = 1. / inv_scale_y;
        iscale_x = cv_round_d(scale_x); iscale_y = cv_round_d(scale_y);
        mode = (fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON) ? 1 : 2;
    }
    auto k_resize_gray = fmt == kPixBayerBGGR8 ? k_fr_resize_gray<kPixBayerBGGR8> : fmt == kPixBGRA8 ? k_fr_resize_gray<kPixBGRA8> : k_fr_resize_gray<kPixBGR8>;
    hipLaunchKernelGGL(k_resize_gray, dim3(gx, ncam), dim3(256), 0, st, fp, w, h, stride, dw, dh, scale_x, scale_y, iscale_x, iscale_y, mode);
    hipLaunchKernelGGL(k_fr_remap, dim3(gx, ncam), dim3(256), 0, st, fp, dw, dh);
    if (any_clahe) {
        hipLaunchKernelGGL(k_fr_clahe_lut, dim3(64, ncam), dim3(256), 0, st, fp, dw, dh, tw, th, lutScale);
        hipLaunchKernelGGL(k_fr_clahe_apply, dim3(gx, ncam), dim3(256), 0, st, fp, dw, dh, tw, th);
    }
    UVO_HIP_TRY(L, hipGetLastError());
    return UVO_OK;
}

}  // namespace uvo
