// uvo_pix.h -- pixel layouts of a camera frame (UVO_PIX_* of include/uvo_hip.h) and the one statement of the BGGR demosaic.
// k_bayer_bggr (codec.hip: the mosaic to a w x h x 3 picture) and the Bayer instance of k_fr_resize_gray (preproc.hip: the mosaic
// straight to the grey image) both call pix_bayer_bggr, so the two routes cannot drift.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace uvo {

constexpr int kPixBGR8 = 0, kPixBGRA8 = 1, kPixBayerBGGR8 = 2;         // = UVO_PIX_BGR8, UVO_PIX_BGRA8, UVO_PIX_BAYER_BGGR8
__host__ __device__ inline int pix_bpp(int fmt) { return fmt == kPixBGRA8 ? 4 : (fmt == kPixBayerBGGR8 ? 1 : 3); }
inline bool pix_known(int fmt) { return fmt == kPixBGR8 || fmt == kPixBGRA8 || fmt == kPixBayerBGGR8; }

// COLOR_BayerBGGR2BGR (= COLOR_BayerRG2BGR), bilinear ([UPSTREAM] imgproc/src/demosaicing.cpp Bayer2RGB_): B, G, R of pixel (x, y) of a
// w x h mosaic.  Interior pixels from their 3 x 3 neighbourhood; the first / last column copies its neighbour, then the first / last
// row copies its neighbour: a border pixel is the nearest interior pixel's value.  A mosaic with a side below 3 gives zeros.
// Reads rows yy - 1 .. yy + 1 and columns xx - 1 .. xx + 1 of the clamped position only: never outside the mosaic.
__device__ __forceinline__ void pix_bayer_bggr(const uint8_t* __restrict__ bayer, int w, int h, int stride, int x, int y, int& B, int& G, int& R)
{
    if (w < 3 || h < 3) { B = G = R = 0; return; }
    const int yy = y < 1 ? 1 : (y > h - 2 ? h - 2 : y), xx = x < 1 ? 1 : (x > w - 2 ? w - 2 : x);      // the border copies the nearest interior pixel
    const uint8_t* r0 = bayer + (size_t)(yy - 1) * stride; const uint8_t* r1 = r0 + stride; const uint8_t* r2 = r1 + stride;
    const bool ey = (yy & 1) == 0, ex = (xx & 1) == 0;
    const int cross = (r0[xx] + r1[xx - 1] + r1[xx + 1] + r2[xx] + 2) >> 2, diag = (r0[xx - 1] + r0[xx + 1] + r2[xx - 1] + r2[xx + 1] + 2) >> 2;
    const int horz = (r1[xx - 1] + r1[xx + 1] + 1) >> 1, vert = (r0[xx] + r2[xx] + 1) >> 1;
    if (ey && ex) { B = r1[xx]; G = cross; R = diag; }
    else if (!ey && !ex) { R = r1[xx]; G = cross; B = diag; }
    else if (ey) { G = r1[xx]; B = horz; R = vert; }
    else { G = r1[xx]; R = horz; B = vert; }
}

}  // namespace uvo
