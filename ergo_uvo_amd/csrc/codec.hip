// codec.hip -- compressed-image ingest: what from_ros_to_cv_image does before get_image
// (uvo_libraries/src/math_utility.cpp:154-173): cv_bridge::toCvCopy(CompressedImage) = cv::imdecode -> libjpeg, then
// cv::cvtColor(COLOR_BayerBGGR2BGR) when the format string says "bayer".
//
// uvo_decode_image's default entropy decoder runs on the host -- one sequential pass over the compressed bytes into a pinned
// coefficient buffer (variable-length codes, DC prediction).  The compressed loop entries, and uvo_decode_image after
// uvo_ctx_set_jpeg_entropy(c, 1), decode the Huffman stream on the device instead: Huffman streams self-synchronise, so subsequences
// are decoded in parallel and stitched (the k_jh_* kernels below, uvo_jhuff.h).  Everything that is per-block or per-pixel runs on
// the device, HBM-bound byte work with coalesced accesses:
//   k_jpeg_idct    one thread per 8 x 8 block: dequantisation + libjpeg's jpeg_idct_islow (JDCT_ISLOW, libjpeg's and
//                  cv::imdecode's default), the block's 64 samples written to the component plane
//   k_jpeg_colour  one thread per pixel: libjpeg's fancy (triangle) chroma upsampling evaluated at the pixel from the
//                  neighbouring chroma samples + the YCbCr -> RGB fixed-point conversion, B G R interleaved out
//   k_bayer_bggr   COLOR_BayerBGGR2BGR, bilinear, OpenCV's border rule
// Results are byte-identical to libjpeg-turbo's (tests/test_codec.py: fixtures decoded by Pillow's libjpeg-turbo).
// Baseline / extended-sequential Huffman JPEG, 8 bit, 1 or 3 components, sampling factors 1 or 2, restart markers;
// progressive and arithmetic-coded files are refused with UVO_INVALID_ARG (cv::imdecode would decode them on the CPU).
// PNG payloads (round 3; sniffed by signature as cv::imdecode does): zlib inflate and the scanline filters on the host
// (uvo_png.h), k_png_expand on the device: 1 / 2 / 4 / 8-bit grey, palette and RGB(A) samples -> grey / B G R (A) bytes.
#include "uvo_ctx.h"
#include "uvo_png.h"
#include "uvo_jhuff.h"
#include "uvo_pix.h"
#include <string.h>
#include <vector>

namespace uvo {

// ------------------------------------------------------------------------------------------ host: headers + entropy decoding
namespace {

const uint8_t kNatural[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

// canonical Huffman table with a 9-bit first-level lookup (code length + symbol), longer codes by the length walk
struct Huff {
    uint8_t bits[17] = {0}, vals[256] = {0};
    int mincode[18], maxcode[18], valptr[18];
    uint16_t fast[512];                                       // (length << 8) | symbol, 0 = longer than 9 bits
    bool present = false;
    // false: the code lengths do not form a prefix code (more codes of a length than remain): jdhuff.c's JERR_BAD_HUFF_TABLE
    bool build()
    {
        int code = 0, k = 0;
        memset(fast, 0, sizeof(fast));
        present = false;
        for (int l = 1; l <= 16; l++) {
            if (code + bits[l] > (1 << l)) return false;
            valptr[l] = k; mincode[l] = code;
            for (int i = 0; i < bits[l]; i++, k++, code++)
                if (l <= 9) { const int lo = code << (9 - l); for (int f = 0; f < (1 << (9 - l)); f++) fast[lo + f] = (uint16_t)((l << 8) | vals[k]); }
            maxcode[l] = bits[l] ? code - 1 : -1;
            code <<= 1;
        }
        present = true;
        return true;
    }
    bool dc_symbols_ok() const { int cnt = 0; for (int l = 1; l <= 16; l++) cnt += bits[l]; for (int i = 0; i < cnt; i++) if (vals[i] > 15) return false; return true; }
};

struct BitReader {
    const uint8_t* p; const uint8_t* end; uint64_t acc = 0; int nbits = 0; int marker = 0;
    void fill()
    {
        while (nbits <= 48) {
            int c = 0;
            if (!marker && p < end) {
                c = *p++;
                if (c == 0xFF) {
                    const int c2 = p < end ? *p : 0xD9;
                    if (c2 == 0) p++;
                    else { marker = c2; p--; c = 0; }        // a marker ends the segment: zeros from here on (as jdhuff.c)
                }
            }
            acc |= (uint64_t)c << (56 - nbits);
            nbits += 8;
        }
    }
    inline int peek(int n) { if (nbits < n) fill(); return (int)(acc >> (64 - n)); }
    inline void skip(int n) { acc <<= n; nbits -= n; }
    inline int get(int n) { if (n == 0) return 0; const int v = peek(n); skip(n); return v; }
    inline int decode(const Huff& h)
    {
        if (nbits < 16) fill();
        const uint16_t f = h.fast[acc >> 55];
        if (f) { skip(f >> 8); return f & 255; }
        int code = (int)(acc >> 54), l = 10;                 // the first ten bits
        for (; l <= 16; l++) {
            if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) { skip(l); return h.vals[h.valptr[l] + code - h.mincode[l]]; }
            code = (int)(acc >> (63 - l));
        }
        skip(16);
        return 0;                                            // corrupt code: libjpeg warns and goes on with zero
    }
};
inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct Comp { int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0, bw = 0, bh = 0; size_t coef_off = 0; int dc_pred = 0; };
struct Jpeg {
    int w = 0, h = 0, ncomp = 0, hmax = 1, vmax = 1, restart = 0, mcux = 0, mcuy = 0;
    uint16_t quant[4][64];
    Huff dc[4], ac[4];
    Comp comp[3];
    size_t total_blocks = 0;
};
inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

}  // namespace

struct CodecWs {
    int16_t* h_coef = nullptr; int16_t* d_coef = nullptr; size_t coef_cap = 0, coef_cap_dev = 0;      // blocks x 64, pinned / device
    uint8_t* d_planes = nullptr; size_t planes_cap = 0;                                // the three component planes (block-padded)
    uint8_t* d_out = nullptr; size_t out_cap = 0;                                      // decoded image (and the Bayer source)
    uint8_t* d_out2 = nullptr; size_t out2_cap = 0;                                    // demosaiced image
    uint16_t* d_quant = nullptr;                                                       // 4 x 64
    void* jh = nullptr;                                                                // JhWs*: the device entropy decoder's workspaces
};
static void jh_ws_free(CodecWs* w);

void codec_ws_free(Ctx* c)
{
    CodecWs* w = static_cast<CodecWs*>(c->codec_ws);
    if (!w) return;
    jh_ws_free(w);
    (void)hipHostFree(w->h_coef); (void)hipFree(w->d_coef); (void)hipFree(w->d_planes); (void)hipFree(w->d_out); (void)hipFree(w->d_out2); (void)hipFree(w->d_quant);
    delete w;
    c->codec_ws = nullptr;
}

static uvo_status grow(Ctx* c, void** p, size_t* cap, size_t need, bool pinned)
{
    if (*cap >= need) return UVO_OK;
    if (*p) { if (pinned) (void)hipHostFree(*p); else (void)hipFree(*p); *p = nullptr; *cap = 0; }
    const size_t n = need + need / 4 + 4096;
    UVO_HIP_TRY(c, pinned ? hipHostMalloc(p, n) : hipMalloc(p, n));
    *cap = n;
    return UVO_OK;
}

// Parses the headers and decodes every coefficient into ws->h_coef (natural order, component after component,
// blocks in raster order of the MCU-padded component).  Host only.
// headers_only: stop at the first scan header, after every check of the frame, table and scan headers (the size query of
// uvo_decode_image): nothing is allocated and no coefficient is decoded.
// scan_off (with headers_only): where the first scan's entropy-coded bytes begin
static uvo_status jpeg_entropy_decode(Ctx* c, CodecWs* ws, const uint8_t* data, size_t n, Jpeg* j, bool headers_only = false, size_t* scan_off = nullptr)
{
    auto bad = [&](const char* m) { c->err = std::string("JPEG: ") + m; return UVO_INVALID_ARG; };
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return bad("not a JPEG stream (no SOI)");
    size_t pos = 2;
    bool have_sof = false;
    while (pos + 4 <= n) {
        if (data[pos] != 0xFF) { pos++; continue; }
        const int m = data[pos + 1];
        if (m == 0xFF) { pos++; continue; }
        pos += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) break;
        if (pos + 2 > n) return bad("truncated");
        const int len = be16(data + pos);
        if (len < 2 || pos + len > n) return bad("truncated segment");
        const uint8_t* s = data + pos + 2; const int sl = len - 2;
        switch (m) {
        case 0xDB:
            for (int o = 0; o < sl;) {
                const int pq = s[o] >> 4, tq = s[o] & 15; o++;
                if (tq > 3 || o + (pq ? 128 : 64) > sl) return bad("bad quantisation table");
                for (int k = 0; k < 64; k++) j->quant[tq][kNatural[k]] = (uint16_t)(pq ? be16(s + o + 2 * k) : s[o + k]);
                o += pq ? 128 : 64;
            }
            break;
        case 0xC4:
            for (int o = 0; o + 17 <= sl;) {
                const int tc = s[o] >> 4, th = s[o] & 15; o++;
                if (th > 3 || tc > 1) return bad("bad Huffman table id");
                Huff& h = tc ? j->ac[th] : j->dc[th];
                int cnt = 0;
                for (int l = 1; l <= 16; l++) { h.bits[l] = s[o + l - 1]; cnt += h.bits[l]; }
                o += 16;
                if (cnt > 256 || o + cnt > sl) return bad("bad Huffman table");
                memcpy(h.vals, s + o, (size_t)cnt); o += cnt;
                if (!h.build()) return bad("bad Huffman table (not a prefix code)");
            }
            break;
        case 0xC0: case 0xC1: {
            if (have_sof) return bad("second frame header");
            if (sl < 6 || s[0] != 8) return bad("only 8-bit samples are supported");
            j->h = be16(s + 1); j->w = be16(s + 3); j->ncomp = s[5];
            if (j->w <= 0 || j->h <= 0) return bad("empty image");
            if ((long long)j->w * j->h > (1LL << 26)) return bad("images above 64 Mpixel are refused (a damaged header must not ask for gigabytes)");
            if (j->ncomp != 1 && j->ncomp != 3) return bad("only 1 or 3 components are supported");
            if (sl < 6 + 3 * j->ncomp) return bad("truncated frame header");
            j->hmax = j->vmax = 1;
            for (int k = 0; k < j->ncomp; k++) {
                Comp& q = j->comp[k];
                q.id = s[6 + 3 * k]; q.h = s[7 + 3 * k] >> 4; q.v = s[7 + 3 * k] & 15; q.tq = s[8 + 3 * k];
                if (q.h < 1 || q.h > 2 || q.v < 1 || q.v > 2 || q.tq > 3) return bad("sampling factors above 2 are not supported");
                j->hmax = q.h > j->hmax ? q.h : j->hmax; j->vmax = q.v > j->vmax ? q.v : j->vmax;
            }
            if (j->ncomp == 1) { j->comp[0].h = j->comp[0].v = 1; j->hmax = j->vmax = 1; }
            j->mcux = (j->w + 8 * j->hmax - 1) / (8 * j->hmax); j->mcuy = (j->h + 8 * j->vmax - 1) / (8 * j->vmax);
            size_t off = 0;
            for (int k = 0; k < j->ncomp; k++) {
                Comp& q = j->comp[k];
                q.bw = j->mcux * q.h; q.bh = j->mcuy * q.v; q.coef_off = off;
                off += (size_t)q.bw * q.bh;
            }
            j->total_blocks = off;
            if (!headers_only) {
                UVO_TRY(grow(c, reinterpret_cast<void**>(&ws->h_coef), &ws->coef_cap, off * 64 * sizeof(int16_t), true));
                memset(ws->h_coef, 0, off * 64 * sizeof(int16_t));
            }
            have_sof = true;
            break;
        }
        case 0xDD: if (sl < 2) return bad("truncated restart interval"); j->restart = be16(s); break;
        case 0xDA: {
            if (!have_sof) return bad("scan before frame header");
            if (sl < 1 || s[0] != j->ncomp) return bad("non-interleaved scans are not supported");
            if (sl < 1 + 2 * j->ncomp + 3) return bad("truncated scan header");
            for (int i = 0; i < s[0]; i++)
                for (int k = 0; k < j->ncomp; k++)
                    if (j->comp[k].id == s[1 + 2 * i]) { j->comp[k].td = s[2 + 2 * i] >> 4; j->comp[k].ta = s[2 + 2 * i] & 15; }
            for (int k = 0; k < j->ncomp; k++) if (j->comp[k].td > 3 || j->comp[k].ta > 3 || !j->dc[j->comp[k].td].present || !j->ac[j->comp[k].ta].present) return bad("scan refers to a missing Huffman table");
            for (int k = 0; k < j->ncomp; k++) if (!j->dc[j->comp[k].td].dc_symbols_ok()) return bad("bad DC Huffman table (category above 15)");
            if (headers_only) { if (scan_off) *scan_off = pos + len; return UVO_OK; }
            BitReader b; b.p = data + pos + len; b.end = data + n;
            int left = j->restart;
            for (int my = 0; my < j->mcuy; my++)
                for (int mx = 0; mx < j->mcux; mx++) {
                    if (j->restart && left == 0) {           // RSTn: drop the partial byte, skip the marker, reset the predictors
                        b.acc = 0; b.nbits = 0;
                        if (b.marker >= 0xD0 && b.marker <= 0xD7) { b.p += 2; b.marker = 0; }
                        else { while (b.p + 1 < b.end && !(b.p[0] == 0xFF && b.p[1] >= 0xD0 && b.p[1] <= 0xD7)) b.p++; if (b.p + 1 < b.end) b.p += 2; b.marker = 0; }
                        for (int k = 0; k < j->ncomp; k++) j->comp[k].dc_pred = 0;
                        left = j->restart;
                    }
                    for (int k = 0; k < j->ncomp; k++) {
                        Comp& q = j->comp[k];
                        const Huff& hd = j->dc[q.td]; const Huff& ha = j->ac[q.ta];
                        for (int by = 0; by < q.v; by++)
                            for (int bx = 0; bx < q.h; bx++) {
                                int16_t* blk = ws->h_coef + (q.coef_off + (size_t)(my * q.v + by) * q.bw + (mx * q.h + bx)) * 64;
                                const int t = b.decode(hd);
                                q.dc_pred = (int)((unsigned)q.dc_pred + (unsigned)(t ? extend(b.get(t), t) : 0));   // (wraps on damaged streams)
                                blk[0] = (int16_t)q.dc_pred;
                                for (int kk = 1; kk < 64;) {
                                    const int rs = b.decode(ha), r = rs >> 4, sz = rs & 15;
                                    if (sz == 0) { if (r == 15) { kk += 16; continue; } break; }
                                    kk += r;
                                    if (kk > 63) break;
                                    blk[kNatural[kk]] = (int16_t)extend(b.get(sz), sz);
                                    kk++;
                                }
                            }
                    }
                    if (j->restart) left--;
                }
            return UVO_OK;
        }
        default:
            if (m == 0xC2) return bad("progressive JPEG is not supported (baseline / sequential Huffman only)");
            if (m >= 0xC3 && m <= 0xCF && m != 0xC8) return bad("lossless / arithmetic-coded JPEG is not supported");
            break;
        }
        pos += len;
    }
    return bad("no scan found");
}

// ------------------------------------------------------------------------------------------ device
struct IdctComp { size_t coef_off; int bw, bh, tq; size_t plane_off; };
struct IdctArgs { IdctComp comp[3]; int ncomp; size_t total_blocks; };

#define UVO_DESCALE(x, n) ((int)((unsigned)(x) + (1u << ((n) - 1))) >> (n))
__device__ __forceinline__ uint8_t jpeg_range_limit(int x)
{   // libjpeg's post-IDCT range_limit table read at x & 1023 (jdmaster.c prepare_range_limit_table): [0,128) -> v + 128,
    // [128,512) -> 255, [512,896) -> 0, [896,1024) -> v - 896: clamp(x + 128) for |x| < 512, the table's wrap beyond
    const int v = x & 1023;
    return (uint8_t)(v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896)));
}
// jidctint.c's butterfly on eight values (in place); both passes use it with different descaling
// (every add / multiply modulo 2^32: a damaged stream with out-of-range coefficients gives some picture, never undefined behaviour)
__device__ __forceinline__ void islow_1d(const int (&in_s)[8], int (&o)[8])
{
    unsigned in[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = (unsigned)in_s[k];
    unsigned z2 = in[2], z3 = in[6];
    unsigned z1 = (z2 + z3) * 4433u;
    unsigned tmp2 = z1 + z3 * (unsigned)(-15137), tmp3 = z1 + z2 * 6270u;
    unsigned tmp0 = (in[0] + in[4]) * 8192u, tmp1 = (in[0] - in[4]) * 8192u;
    const unsigned tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2; unsigned z4 = tmp1 + tmp3;
    const unsigned z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (unsigned)(-7373); z2 *= (unsigned)(-20995); z3 *= (unsigned)(-16069); z4 *= (unsigned)(-3196);
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = (int)(tmp10 + tmp3); o[7] = (int)(tmp10 - tmp3); o[1] = (int)(tmp11 + tmp2); o[6] = (int)(tmp11 - tmp2);
    o[2] = (int)(tmp12 + tmp1); o[5] = (int)(tmp12 - tmp1); o[3] = (int)(tmp13 + tmp0); o[4] = (int)(tmp13 - tmp0);
}

// Eight threads per block, one column then one row each; the block's workspace lives in LDS ([block in workgroup][8][9] ints)
__global__ __launch_bounds__(256) void k_jpeg_idct(IdctArgs a, const int16_t* __restrict__ coef, const uint16_t* __restrict__ quant, uint8_t* __restrict__ planes)
{
    __shared__ int ws[32][8][9];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const size_t blk = (size_t)blockIdx.x * 32 + lb;
    const bool live = blk < a.total_blocks;
    int ci = 0;
    if (live) { if (a.ncomp == 3 && blk >= a.comp[1].coef_off) ci = blk >= a.comp[2].coef_off ? 2 : 1; }
    const IdctComp cp = a.comp[ci];
    if (live) {
        const int16_t* src = coef + blk * 64;
        const uint16_t* q = quant + cp.tq * 64;
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; r++) in[r] = (int)src[r * 8 + t] * (int)q[r * 8 + t];           // column t, dequantised
        islow_1d(in, o);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[lb][r][t] = UVO_DESCALE(o[r], 11);                       // CONST_BITS - PASS1_BITS
    }
    __syncthreads();
    if (live) {
        int in[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) in[k] = ws[lb][t][k];                                       // row t
        islow_1d(in, o);
        const size_t local = blk - cp.coef_off;
        const int by = (int)(local / cp.bw), bx = (int)(local - (size_t)by * cp.bw);
        uint8_t* dst = planes + cp.plane_off + ((size_t)by * 8 + t) * ((size_t)cp.bw * 8) + (size_t)bx * 8;
        uint2 pk;
        pk.x = jpeg_range_limit(UVO_DESCALE(o[0], 18)) | (jpeg_range_limit(UVO_DESCALE(o[1], 18)) << 8) | (jpeg_range_limit(UVO_DESCALE(o[2], 18)) << 16) | ((unsigned)jpeg_range_limit(UVO_DESCALE(o[3], 18)) << 24);
        pk.y = jpeg_range_limit(UVO_DESCALE(o[4], 18)) | (jpeg_range_limit(UVO_DESCALE(o[5], 18)) << 8) | (jpeg_range_limit(UVO_DESCALE(o[6], 18)) << 16) | ((unsigned)jpeg_range_limit(UVO_DESCALE(o[7], 18)) << 24);
        *reinterpret_cast<uint2*>(dst) = pk;                                                    // 8 samples of row t (8-byte aligned)
    }
}

struct ColourArgs { size_t plane_off[3]; int pw[3]; int dw[3], dh[3]; int hs[3], vs[3]; int ncomp, w, h; };

// libjpeg's fancy upsampling evaluated at one output position (jdsample.c h2v1 / h2v2 / h1v2), replication for 1 x 1
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pw, int dw, int dh, int hs, int vs, int x, int y)
{
    if (hs == 1 && vs == 1) return p[(size_t)y * pw + x];
    const int sy = y / vs, sx = x / hs;
    const uint8_t* r0 = p + (size_t)sy * pw;
    if (vs == 1) {                                            // h2v1: 3/4 nearer + 1/4 farther, bias 1 (even) / 2 (odd); the ends copy
        if ((x & 1) == 0) return sx == 0 ? r0[0] : (3 * r0[sx] + r0[sx - 1] + 1) >> 2;
        return sx == dw - 1 ? r0[sx] : (3 * r0[sx] + r0[sx + 1] + 2) >> 2;
    }
    int oy = (y & 1) ? sy + 1 : sy - 1;
    oy = oy < 0 ? 0 : (oy > dh - 1 ? dh - 1 : oy);
    const uint8_t* r1 = p + (size_t)oy * pw;
    if (hs == 1) return (3 * r0[x] + r1[x] + ((y & 1) ? 2 : 1)) >> 2;                           // h1v2
    const int thiscol = 3 * r0[sx] + r1[sx];                  // h2v2
    if ((x & 1) == 0) return sx == 0 ? (thiscol * 4 + 8) >> 4 : (thiscol * 3 + 3 * r0[sx - 1] + r1[sx - 1] + 8) >> 4;
    return sx == dw - 1 ? (thiscol * 4 + 7) >> 4 : (thiscol * 3 + 3 * r0[sx + 1] + r1[sx + 1] + 7) >> 4;
}

__global__ __launch_bounds__(256) void k_jpeg_colour(ColourArgs a, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const int Y = chroma_at(planes + a.plane_off[0], a.pw[0], a.dw[0], a.dh[0], a.hs[0], a.vs[0], x, y);
    if (a.ncomp == 1) { out[(size_t)y * a.w + x] = (uint8_t)Y; return; }
    const int cb = chroma_at(planes + a.plane_off[1], a.pw[1], a.dw[1], a.dh[1], a.hs[1], a.vs[1], x, y) - 128;
    const int cr = chroma_at(planes + a.plane_off[2], a.pw[2], a.dw[2], a.dh[2], a.hs[2], a.vs[2], x, y) - 128;
    // jdcolor.c: Cr_r_tab, Cb_b_tab, Cb_g_tab + Cr_g_tab (16-bit fixed point, ONE_HALF folded into the Cb table)
    int r = Y + ((91881 * cr + 32768) >> 16);
    int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    int b = Y + ((116130 * cb + 32768) >> 16);
    r = r < 0 ? 0 : (r > 255 ? 255 : r); g = g < 0 ? 0 : (g > 255 ? 255 : g); b = b < 0 ? 0 : (b > 255 ? 255 : b);
    uint8_t* o = out + ((size_t)y * a.w + x) * 3;
    o[0] = (uint8_t)b; o[1] = (uint8_t)g; o[2] = (uint8_t)r;
}

// COLOR_BayerBGGR2BGR (= COLOR_BayerRG2BGR), bilinear ([UPSTREAM] imgproc/src/demosaicing.cpp Bayer2RGB_): interior pixels from
// their 3 x 3 neighbourhood; the first / last column copies its neighbour, then the first / last row copies its neighbour.
__global__ __launch_bounds__(256) void k_bayer_bggr(const uint8_t* __restrict__ bayer, int w, int h, int stride, uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    uint8_t* o = dst + ((size_t)y * w + x) * 3;
    int B, G, R;
    pix_bayer_bggr(bayer, w, h, stride, x, y, B, G, R);                 // uvo_pix.h: the statement the frames entries' Bayer instance shares
    o[0] = (uint8_t)B; o[1] = (uint8_t)G; o[2] = (uint8_t)R;
}

// ------------------------------------------------------------------------------------------ entropy decoding on the device
// The scheme of uvo_jhuff.h as four launches on the lane's stream, every grid-wide seam a kernel boundary (no workgroup waits for another):
//   k_jh_pass1  one thread per subsequence, kJhGroup subsequences per workgroup: decode from (first bit, 0, 0), then again from the
//               left neighbour's exit state until no state in the workgroup changes (at most kJhGroup - 1 rounds: after k rounds the
//               first k subsequences behind a final one are final)
//   k_jh_cross  ONE workgroup, one thread per workgroup boundary: a boundary whose incoming state differs from the state its group
//               was decoded from walks that group until a subsequence's entry state agrees again; rounds until nothing changes (at
//               most the number of boundaries).  Then the segmented exclusive scan of the slot counts: every subsequence's first slot
//   k_jh_emit   one thread per subsequence: decode from the final entry state and scatter the DC differences and AC coefficients
//   k_jh_dc     one workgroup per component: DC differences -> DC values, a scan over the component's blocks in scan order,
//               segmented at restart intervals, modulo 2^32 and narrowed to int16 as the host decoder does
// The Huffman tables are copied to LDS by every workgroup that decodes.  Reads of the staged scan are clamped to its zero padding
// (jhuff::peek32), writes of coefficients are tested against the interval's and the picture's slots, every loop has a trip bound.
constexpr int kJhGroup = 256;
constexpr int kJhWide = 1024;
__device__ const uint8_t kNaturalDev[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
struct JhBufs {
    const jhuff::Table* tabs; int n_tabs;
    const uint8_t* scan; const uint32_t* info;
    jhuff::State* entry; jhuff::State* exit; jhuff::State* incoming;     // per subsequence, per subsequence, per workgroup
    uint32_t* slots; uint32_t* first;
    int* stats;                                                          // [0] rounds inside a workgroup (maximum), [1] rounds across
};

__device__ __forceinline__ void jh_tables_to_lds(jhuff::Table* dst, const jhuff::Table* src, int n_tabs)
{
    const int words = n_tabs * (int)(sizeof(jhuff::Table) / 4);
    static_assert(sizeof(jhuff::Table) % 4 == 0, "tables are copied as words");
    for (int i = threadIdx.x; i < words; i += blockDim.x) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    __syncthreads();
}

__global__ __launch_bounds__(kJhGroup) void k_jh_pass1(jhuff::Scan s, JhBufs b)
{
    __shared__ jhuff::Table tabs[jhuff::kMaxTables];
    __shared__ jhuff::State s_exit[kJhGroup];
    jh_tables_to_lds(tabs, b.tabs, b.n_tabs);
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kJhGroup + tid, sub_bits = s.sub_words * 32;
    const bool live = i < s.n_sub;
    const bool fixed = !live || tid == 0 || (b.info[i] & 1);             // a workgroup's first subsequence is k_jh_cross's
    jhuff::State in = { i * sub_bits, 0 }, out = in;
    uint32_t sl = 0;
    if (live) sl = jhuff::decode_span(tabs, s, b.scan, &out, (i + 1) * sub_bits, jhuff::NoEmit());
    s_exit[tid] = out;
    __syncthreads();
    int rounds = 0;
    for (int r = 0; r < kJhGroup - 1; r++) {
        jhuff::State prev = in;
        if (!fixed) prev = s_exit[tid - 1];
        const int changed = !jhuff::same(prev, in);
        if (!__syncthreads_or(changed)) break;                           // (every thread has read its neighbour before any writes)
        rounds++;
        if (changed) { in = prev; out = in; sl = jhuff::decode_span(tabs, s, b.scan, &out, (i + 1) * sub_bits, jhuff::NoEmit()); s_exit[tid] = out; }
        __syncthreads();
    }
    if (live) { b.entry[i] = in; b.exit[i] = out; b.slots[i] = sl; }
    if (tid == 0) atomicMax(&b.stats[0], rounds);
}

// inclusive scan over the workgroup's (flag, value) pairs with the segmented sum: a flagged right operand replaces, else it adds
__device__ __forceinline__ void jh_seg_scan(uint32_t* s_val, uint32_t* s_flag, uint32_t& val, uint32_t& flag)
{
    const int tid = threadIdx.x;
    s_val[tid] = val; s_flag[tid] = flag;
    __syncthreads();
    for (int o = 1; o < kJhWide; o <<= 1) {
        uint32_t lv = 0, lf = 0;
        if (tid >= o) { lv = s_val[tid - o]; lf = s_flag[tid - o]; }
        __syncthreads();
        if (tid >= o && !flag) { val += lv; flag = lf; }
        s_val[tid] = val; s_flag[tid] = flag;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kJhWide) void k_jh_cross(jhuff::Scan s, JhBufs b, uint32_t n_groups)
{
    __shared__ jhuff::Table tabs[jhuff::kMaxTables];
    __shared__ uint32_t s_val[kJhWide], s_flag[kJhWide];
    jh_tables_to_lds(tabs, b.tabs, b.n_tabs);
    const uint32_t tid = threadIdx.x, sub_bits = s.sub_words * 32;
    int rounds = 0;
    for (uint32_t r = 0; r < n_groups; r++) {                            // (n_groups - 1 boundaries; the last round finds nothing)
        int changed = 0;
        for (uint32_t g = 1 + tid; g < n_groups; g += kJhWide) b.incoming[g] = b.exit[g * kJhGroup - 1];
        __syncthreads();
        for (uint32_t g = 1 + tid; g < n_groups; g += kJhWide) {
            const uint32_t i0 = g * kJhGroup, i1 = i0 + kJhGroup < s.n_sub ? i0 + kJhGroup : s.n_sub;
            if (b.info[i0] & 1) continue;                                // a restart interval begins here: in step from its first bit
            jhuff::State cur = b.incoming[g];
            if (jhuff::same(cur, b.entry[i0])) continue;
            changed = 1;
            for (uint32_t i = i0; i < i1; i++) {
                if (i > i0 && ((b.info[i] & 1) || jhuff::same(cur, b.entry[i]))) break;      // from here on the group already follows
                b.entry[i] = cur;
                b.slots[i] = jhuff::decode_span(tabs, s, b.scan, &cur, (i + 1) * sub_bits, jhuff::NoEmit());
                b.exit[i] = cur;
            }
        }
        if (!__syncthreads_or(changed)) break;
        rounds++;
    }
    if (tid == 0) b.stats[1] = rounds;
    // first slot of every subsequence: its interval's first slot at an interval's start, else the predecessor's first + slots
    const uint32_t per = (s.n_sub + kJhWide - 1) / kJhWide, a = tid * per, e = a + per < s.n_sub ? a + per : s.n_sub;
    const uint32_t iv_slots = s.iv_mcus * s.bpm * 64;
    uint32_t val = 0, flag = 0;
    for (uint32_t i = a; i < e; i++) {
        const uint32_t inf = b.info[i];
        if (inf & 1) { flag = 1; val = (inf >> 1) * iv_slots; }
        val += b.slots[i];
    }
    jh_seg_scan(s_val, s_flag, val, flag);
    uint32_t cur = tid ? s_val[tid - 1] : 0;
    for (uint32_t i = a; i < e; i++) {
        const uint32_t inf = b.info[i];
        if (inf & 1) cur = (inf >> 1) * iv_slots;
        b.first[i] = cur;
        cur += b.slots[i];
    }
}

__global__ __launch_bounds__(kJhGroup) void k_jh_emit(jhuff::Scan s, JhBufs b, int16_t* __restrict__ coef)
{
    __shared__ jhuff::Table tabs[jhuff::kMaxTables];
    jh_tables_to_lds(tabs, b.tabs, b.n_tabs);
    const uint32_t i = blockIdx.x * kJhGroup + threadIdx.x;
    if (i >= s.n_sub) return;
    jhuff::State st = b.entry[i];
    const uint32_t first = b.first[i];
    const unsigned long long total_slots = (unsigned long long)s.total_blocks * 64, iv_end = ((unsigned long long)(b.info[i] >> 1) + 1) * s.iv_mcus * s.bpm * 64;
    const unsigned long long slot_end = iv_end < total_slots ? iv_end : total_slots;       // slots at or beyond it are dropped
    const size_t n_coef = (size_t)s.total_blocks * 64;
    (void)jhuff::decode_span(tabs, s, b.scan, &st, (i + 1) * s.sub_words * 32, [&](uint32_t rel, int v) {
        const uint32_t slot = first + rel;
        if (slot >= slot_end) return;
        const size_t idx = jhuff::slot_block(s, slot >> 6) * 64 + kNaturalDev[slot & 63];
        if (idx < n_coef) coef[idx] = (int16_t)v;
    });
}

// component k = blockIdx.x: element e of its scan order is block (e % hv) of MCU e / hv; a segment begins every iv_mcus * hv elements
__global__ __launch_bounds__(kJhWide) void k_jh_dc(jhuff::Scan s, int16_t* __restrict__ coef)
{
    __shared__ uint32_t s_val[kJhWide], s_flag[kJhWide];
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const uint32_t h = s.comp_h[k], hv = h * s.comp_v[k], n = s.total_mcus * hv, seg = s.iv_mcus * hv;
    const uint32_t per = (n + kJhWide - 1) / kJhWide, a = tid * per, e = a + per < n ? a + per : n;
    const size_t n_coef = (size_t)s.total_blocks * 64;
    auto at = [&](uint32_t el) -> size_t {
        const uint32_t mcu = el / hv, j = el - mcu * hv, by = j / h, bx = j - by * h, my = mcu / s.mcux, mx = mcu - my * s.mcux;
        const size_t idx = ((size_t)s.comp_off[k] + (size_t)(my * s.comp_v[k] + by) * s.comp_bw[k] + (mx * h + bx)) * 64;
        return idx < n_coef ? idx : n_coef;                              // (n_coef: outside the buffer -- read as zero, never written)
    };
    uint32_t val = 0, flag = 0;
    for (uint32_t el = a; el < e; el++) {
        if (el % seg == 0) { flag = 1; val = 0; }
        const size_t idx = at(el);
        val += idx < n_coef ? (uint32_t)(int)coef[idx] : 0u;
    }
    jh_seg_scan(s_val, s_flag, val, flag);
    uint32_t cur = tid ? s_val[tid - 1] : 0;
    for (uint32_t el = a; el < e; el++) {
        if (el % seg == 0) cur = 0;
        const size_t idx = at(el);
        if (idx >= n_coef) continue;
        cur += (uint32_t)(int)coef[idx];
        coef[idx] = (int16_t)(int)cur;
    }
}

// ---- host side of the device entropy decoder
// One image's workspace.  A stereo entry decodes two images on one lane, so a lane has two; uvo_decode_image uses lane 0's first.
// The pinned block h_stage holds what the kernels read besides their by-value arguments -- the Huffman tables, the quantisation
// tables, the staged scan -- and is uploaded once; h_info holds the subsequences' interval words.  Nothing is copied from a stack frame.
struct JhSlot {
    uint8_t* h_stage = nullptr; uint8_t* d_stage = nullptr; size_t h_stage_cap = 0, d_stage_cap = 0;
    uint32_t* h_info = nullptr; size_t h_info_cap = 0;
    uint8_t* d_sub = nullptr; size_t d_sub_cap = 0;
    int16_t* d_coef = nullptr; size_t coef_cap = 0;
    uint8_t* d_planes = nullptr; size_t planes_cap = 0;
    uint8_t* d_out = nullptr; size_t out_cap = 0;
    uint8_t* d_out2 = nullptr; size_t out2_cap = 0;
    int* h_stats = nullptr;                                            // pinned: rounds in group, rounds across (of the last decode with stats)
    int n_sub = 0, n_groups = 0; size_t scan_bytes = 0; bool have_stats = false;
};
constexpr size_t kJhTabBytes = sizeof(jhuff::Table) * jhuff::kMaxTables, kJhQuantBytes = 4 * 64 * sizeof(uint16_t), kJhHeadBytes = (kJhTabBytes + kJhQuantBytes + 15) / 16 * 16;
constexpr int kJhDefaultSubWords = 32;
struct JhNeed { size_t stage = 0, subs = 0, coef = 0, planes = 0, out = 0, out2 = 0; };
// a parsed payload between the entry's checks (nothing queued yet) and its decode
struct JhJob { Jpeg j; const uint8_t* scan = nullptr; size_t scan_n = 0; int bayer = 0, sub_words = kJhDefaultSubWords; jhuff::Scan s; jhuff::Table tabs[jhuff::kMaxTables]; int n_tabs = 0; JhNeed need; };
struct JhWs { JhSlot slot[2]; JhJob job[2]; int where = 0; };

static size_t jh_sub_bytes(size_t subs) { const size_t groups = (subs + kJhGroup - 1) / kJhGroup; return subs * (2 * sizeof(jhuff::State) + 3 * sizeof(uint32_t)) + groups * sizeof(jhuff::State) + 64; }

static JhWs* jh_ws(Ctx* c)
{
    if (!c->codec_ws) c->codec_ws = new CodecWs();
    CodecWs* ws = static_cast<CodecWs*>(c->codec_ws);
    if (!ws->jh) ws->jh = new JhWs();
    return static_cast<JhWs*>(ws->jh);
}
static void jh_ws_free(CodecWs* w)
{
    JhWs* q = static_cast<JhWs*>(w->jh);
    if (!q) return;
    for (JhSlot& s : q->slot) {
        (void)hipHostFree(s.h_stage); (void)hipHostFree(s.h_info); (void)hipHostFree(s.h_stats);
        (void)hipFree(s.d_stage); (void)hipFree(s.d_sub); (void)hipFree(s.d_coef); (void)hipFree(s.d_planes); (void)hipFree(s.d_out); (void)hipFree(s.d_out2);
    }
    delete q;
    w->jh = nullptr;
}

// headers -> job: the scan's layout, its compacted tables and what a workspace must hold.  Refuses what the host JPEG path refuses.
static uvo_status jh_prepare(Ctx* m, const uint8_t* data, size_t n, int bayer, int sub_words, JhJob* job)
{
    Jpeg& j = job->j;
    j = Jpeg();
    memset(j.quant, 0, sizeof(j.quant));
    size_t off = 0;
    UVO_TRY(jpeg_entropy_decode(m, nullptr, data, n, &j, true, &off));
    if (bayer && j.ncomp != 1) { m->err = "a bayer-format message must decode to one channel"; return UVO_INVALID_ARG; }
    if (sub_words <= 0) sub_words = kJhDefaultSubWords;
    if (sub_words > 4096) { m->err = "JPEG: sub_words is 1 .. 4096"; return UVO_INVALID_ARG; }
    if (n - off > ((size_t)1 << 27)) { m->err = "JPEG: scans above 128 MB are refused (bit positions are 32-bit)"; return UVO_INVALID_ARG; }
    job->scan = data + off; job->scan_n = n - off; job->bayer = bayer; job->sub_words = sub_words;
    int map_dc[4] = {-1, -1, -1, -1}, map_ac[4] = {-1, -1, -1, -1}, h[3], v[3], tdc[3], tac[3];
    job->n_tabs = 0;
    for (int k = 0; k < j.ncomp; k++) {
        const Comp& q = j.comp[k];
        if (map_dc[q.td] < 0) { map_dc[q.td] = job->n_tabs; if (!jhuff::build_table(&job->tabs[job->n_tabs++], j.dc[q.td].bits, j.dc[q.td].vals)) { m->err = "JPEG: bad Huffman table"; return UVO_INVALID_ARG; } }
        if (map_ac[q.ta] < 0) { map_ac[q.ta] = job->n_tabs; if (!jhuff::build_table(&job->tabs[job->n_tabs++], j.ac[q.ta].bits, j.ac[q.ta].vals)) { m->err = "JPEG: bad Huffman table"; return UVO_INVALID_ARG; } }
        h[k] = q.h; v[k] = q.v; tdc[k] = map_dc[q.td]; tac[k] = map_ac[q.ta];
    }
    jhuff::make_scan(&job->s, j.ncomp, h, v, tdc, tac, j.mcux, j.mcuy, j.restart);
    job->s.sub_words = (uint32_t)sub_words;
    JhNeed& nd = job->need;
    // bit positions and slot sums are 32-bit: the STAGED scan (every restart interval padded to a subsequence) must stay below 2^32 bits,
    // and so must the picture's slots
    if (jhuff::stage_bound_bytes(job->s, job->scan_n, (uint32_t)sub_words) >= ((size_t)1 << 29) || j.total_blocks >= ((size_t)1 << 25)) {
        m->err = "JPEG: the staged scan (restart intervals padded to subsequences) or the picture exceeds the device decoder's 32-bit positions; decode on the host";
        return UVO_INVALID_ARG;
    }
    nd.stage = kJhHeadBytes + jhuff::stage_bound_bytes(job->s, job->scan_n, (uint32_t)sub_words);
    nd.subs = jhuff::stage_bound_subs(job->s, job->scan_n, (uint32_t)sub_words);
    nd.coef = j.total_blocks * 64 * sizeof(int16_t);
    nd.planes = j.total_blocks * 64;
    nd.out = (size_t)j.w * j.h * j.ncomp;
    nd.out2 = bayer ? (size_t)j.w * j.h * 3 : 0;
    return UVO_OK;
}

static bool jh_fits(const JhSlot& s, const JhNeed& nd)
{
    return s.h_stats && s.h_stage_cap >= nd.stage && s.d_stage_cap >= nd.stage && s.h_info_cap >= nd.subs * sizeof(uint32_t) && s.d_sub_cap >= jh_sub_bytes(nd.subs) &&
           s.coef_cap >= nd.coef && s.planes_cap >= nd.planes && s.out_cap >= nd.out && s.out2_cap >= nd.out2;
}
static uvo_status jh_grow_slot(Ctx* m, JhSlot& s, const JhNeed& nd)
{
    if (!s.h_stats) UVO_HIP_TRY(m, hipHostMalloc(reinterpret_cast<void**>(&s.h_stats), 4 * sizeof(int)));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.h_stage), &s.h_stage_cap, nd.stage, true));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.d_stage), &s.d_stage_cap, nd.stage, false));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.h_info), &s.h_info_cap, nd.subs * sizeof(uint32_t), true));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.d_sub), &s.d_sub_cap, jh_sub_bytes(nd.subs), false));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.d_coef), &s.coef_cap, nd.coef, false));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.d_planes), &s.planes_cap, nd.planes, false));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.d_out), &s.out_cap, nd.out, false));
    UVO_TRY(grow(m, reinterpret_cast<void**>(&s.d_out2), &s.out2_cap, nd.out2, false));
    return UVO_OK;
}
// Workspaces of the first nimg slots of every lane in `lanes`, as frames_plan does: made while nothing is in flight, refused otherwise
static uvo_status jh_plan(Ctx* m, Ctx* const* lanes, size_t n_lanes, int nimg, const JhJob* jobs)
{
    bool fits = true;
    for (size_t l = 0; l < n_lanes; l++) for (int i = 0; i < nimg; i++) fits = fits && jh_fits(jh_ws(lanes[l])->slot[i], jobs[i].need);
    if (fits) return UVO_OK;
    if (m->sh->n_pending != 0) { m->err = "the lanes' JPEG workspaces must grow (a larger payload or picture) while entries are in flight: collect first"; return UVO_CAPACITY; }
    for (size_t l = 0; l < n_lanes; l++) {
        UVO_HIP_TRY(m, hipStreamSynchronize(lanes[l]->stream));
        for (int i = 0; i < nimg; i++) UVO_TRY(jh_grow_slot(m, jh_ws(lanes[l])->slot[i], jobs[i].need));
    }
    return UVO_OK;
}

static void jpeg_pixel_args(const Jpeg& j, IdctArgs* ia, ColourArgs* ca)
{
    memset(ia, 0, sizeof(*ia)); memset(ca, 0, sizeof(*ca));
    size_t poff = 0;
    for (int k = 0; k < j.ncomp; k++) {
        const Comp& q = j.comp[k];
        ia->comp[k] = { q.coef_off, q.bw, q.bh, q.tq, poff };
        ca->plane_off[k] = poff; ca->pw[k] = q.bw * 8;
        ca->dw[k] = (j.w * q.h + j.hmax - 1) / j.hmax; ca->dh[k] = (j.h * q.v + j.vmax - 1) / j.vmax;
        ca->hs[k] = j.hmax / q.h; ca->vs[k] = j.vmax / q.v;
        poff += (size_t)q.bw * q.bh * 64;
    }
    for (int k = j.ncomp; k < 3; k++) ia->comp[k] = ia->comp[0];
    ia->ncomp = j.ncomp; ia->total_blocks = j.total_blocks;
    ca->ncomp = j.ncomp; ca->w = j.w; ca->h = j.h;
}

// Stages the job's scan on the calling thread (the payload is consumed here) and queues the decode on lane L's stream, into L's slot.
// Nothing waits for the device.  pixels: also IDCT, colour and the Bayer step; *d_out is the image (B G R, or grey), on L's stream.
static uvo_status jh_queue(Ctx* m, Ctx* L, int slot, const JhJob& job, bool pixels, bool stats, const uint8_t** d_out)
{
    JhSlot& sl = jh_ws(L)->slot[slot];
    if (!jh_fits(sl, job.need)) { m->err = "JPEG: the lane's workspace was not planned"; return UVO_INVALID_ARG; }
    hipStream_t st = L->stream;
    jhuff::Scan s = job.s;
    memcpy(sl.h_stage, job.tabs, kJhTabBytes);
    memcpy(sl.h_stage + kJhTabBytes, job.j.quant, kJhQuantBytes);
    jhuff::Staged sg;
    if (!jhuff::stage_scan(job.scan, job.scan_n, s.sub_words, jhuff::expected_intervals(s), sl.h_stage + kJhHeadBytes, sl.h_stage_cap - kJhHeadBytes, sl.h_info, sl.h_info_cap / sizeof(uint32_t), &sg)) {
        m->err = "JPEG: staging the scan exceeded its planned workspace"; return UVO_INVALID_ARG;
    }
    s.n_bytes = sg.n_bytes; s.n_sub = sg.n_sub; s.n_iv = sg.n_iv;
    const uint32_t n_groups = (s.n_sub + kJhGroup - 1) / kJhGroup;
    const size_t cap_subs = job.need.subs, cap_groups = (cap_subs + kJhGroup - 1) / kJhGroup;
    if (s.n_sub > cap_subs) { m->err = "JPEG: staging the scan exceeded its planned workspace"; return UVO_INVALID_ARG; }
    JhBufs b;
    b.tabs = reinterpret_cast<const jhuff::Table*>(sl.d_stage); b.n_tabs = job.n_tabs;
    b.scan = sl.d_stage + kJhHeadBytes;
    b.entry = reinterpret_cast<jhuff::State*>(sl.d_sub); b.exit = b.entry + cap_subs; b.incoming = b.exit + cap_subs;
    uint32_t* words = reinterpret_cast<uint32_t*>(b.incoming + cap_groups);
    b.info = words; b.slots = words + cap_subs; b.first = b.slots + cap_subs;
    b.stats = reinterpret_cast<int*>(b.first + cap_subs);
    UVO_HIP_TRY(m, hipMemcpyAsync(sl.d_stage, sl.h_stage, kJhHeadBytes + (size_t)sg.n_bytes + jhuff::kPadBytes, hipMemcpyHostToDevice, st));
    UVO_HIP_TRY(m, hipMemcpyAsync(words, sl.h_info, (size_t)s.n_sub * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    UVO_HIP_TRY(m, hipMemsetAsync(b.stats, 0, 4 * sizeof(int), st));
    UVO_HIP_TRY(m, hipMemsetAsync(sl.d_coef, 0, job.need.coef, st));
    hipLaunchKernelGGL(k_jh_pass1, dim3(n_groups), dim3(kJhGroup), 0, st, s, b);
    hipLaunchKernelGGL(k_jh_cross, dim3(1), dim3(kJhWide), 0, st, s, b, n_groups);
    hipLaunchKernelGGL(k_jh_emit, dim3(n_groups), dim3(kJhGroup), 0, st, s, b, sl.d_coef);
    hipLaunchKernelGGL(k_jh_dc, dim3(job.j.ncomp), dim3(kJhWide), 0, st, s, sl.d_coef);
    UVO_HIP_TRY(m, hipGetLastError());
    sl.have_stats = false;
    if (stats) {
        UVO_HIP_TRY(m, hipMemcpyAsync(sl.h_stats, b.stats, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
        sl.n_sub = (int)s.n_sub; sl.n_groups = (int)n_groups; sl.scan_bytes = sg.consumed; sl.have_stats = true;
    }
    if (!pixels) return UVO_OK;
    const Jpeg& j = job.j;
    IdctArgs ia; ColourArgs ca;
    jpeg_pixel_args(j, &ia, &ca);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((j.total_blocks + 31) / 32)), dim3(256), 0, st, ia, sl.d_coef, reinterpret_cast<const uint16_t*>(sl.d_stage + kJhTabBytes), sl.d_planes);
    hipLaunchKernelGGL(k_jpeg_colour, dim3((j.w + 63) / 64, (j.h + 3) / 4), dim3(256), 0, st, ca, sl.d_planes, sl.d_out);
    *d_out = sl.d_out;
    if (job.bayer) {
        hipLaunchKernelGGL(k_bayer_bggr, dim3((j.w + 63) / 64, (j.h + 3) / 4), dim3(256), 0, st, sl.d_out, j.w, j.h, j.w, sl.d_out2);
        *d_out = sl.d_out2;
    }
    UVO_HIP_TRY(m, hipGetLastError());
    return UVO_OK;
}

uvo_status codec_set_entropy(Ctx* c, int where)
{
    if (where != 0 && where != 1) { c->err = "uvo_ctx_set_jpeg_entropy: where is 0 (host) or 1 (device)"; return UVO_INVALID_ARG; }
    jh_ws(c)->where = where;
    return UVO_OK;
}

// uvo_decode_image's JPEG path with the device entropy decoder: lane 0, slot 0, synchronous
static uvo_status jpeg_decode_device(Ctx* c, const uint8_t* data, size_t n, int bayer, const uint8_t** d_out, int* w, int* h, int* channels)
{
    JhWs* q = jh_ws(c);
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));                     // the pinned block of the previous call is free again
    UVO_TRY(jh_prepare(c, data, n, bayer, 0, &q->job[0]));
    Ctx* lane = c;
    UVO_TRY(jh_plan(c, &lane, 1, 1, q->job));
    UVO_TRY(jh_queue(c, c, 0, q->job[0], true, true, d_out));
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *w = q->job[0].j.w; *h = q->job[0].j.h; *channels = bayer ? 3 : q->job[0].j.ncomp;
    return UVO_OK;
}

// The compressed loop entries, in two steps.  codec_compressed_plan: every refusal by kind and the workspaces of all lanes, before
// anything is queued.  codec_compressed_queue: stage + decode image i on lane L.  Both images' sizes come back from the plan.
uvo_status codec_compressed_plan(Ctx* m, int nimg, const uint8_t* const* data, const size_t* n, const int* bayer, int* w, int* h)
{
    JhWs* q = jh_ws(m);
    for (int i = 0; i < nimg; i++) {
        if (!data[i] || n[i] == 0) { m->err = "compressed entry: empty payload"; return UVO_INVALID_ARG; }
        if (png::is_png(data[i], n[i])) { m->err = "compressed entry: PNG payloads are not decoded on the device; use uvo_decode_image and the frames entries"; return UVO_INVALID_ARG; }
        UVO_TRY(jh_prepare(m, data[i], n[i], bayer[i], 0, &q->job[i]));
        if ((bayer[i] ? 3 : q->job[i].j.ncomp) != 3) { m->err = "compressed entry: the payload does not decode to three channels (a grey stream needs a bayer format)"; return UVO_INVALID_ARG; }
        if (i == 1 && (q->job[1].j.w != q->job[0].j.w || q->job[1].j.h != q->job[0].j.h)) { m->err = "compressed entry: left and right pictures differ in size"; return UVO_INVALID_ARG; }
    }
    *w = q->job[0].j.w; *h = q->job[0].j.h;
    return UVO_OK;
}
uvo_status codec_compressed_workspaces(Ctx* m, int nimg)
{
    return jh_plan(m, m->sh->lanes.data(), m->sh->lanes.size(), nimg, jh_ws(m)->job);
}
uvo_status codec_compressed_queue(Ctx* m, Ctx* L, int i, const uint8_t** d_rgb)
{
    return jh_queue(m, L, i, jh_ws(m)->job[i], true, false, d_rgb);
}

// test hooks: the coefficient buffer of either decoder, and the last device decode's figures (lane 0, slot 0)
uvo_status codec_coefficients(Ctx* c, const uint8_t* data, size_t n, int where, int sub_words, int16_t* out, size_t cap, size_t* n_coefs)
{
    if (!c->codec_ws) c->codec_ws = new CodecWs();
    CodecWs* ws = static_cast<CodecWs*>(c->codec_ws);
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (where == 0) {
        Jpeg j;
        memset(j.quant, 0, sizeof(j.quant));
        UVO_TRY(jpeg_entropy_decode(c, nullptr, data, n, &j, true));       // the size first: a call with too little room decodes nothing
        *n_coefs = j.total_blocks * 64;
        if (*n_coefs > cap) { c->err = "uvo_jpeg_coefficients: output capacity too small"; return UVO_CAPACITY; }
        j = Jpeg();
        memset(j.quant, 0, sizeof(j.quant));
        UVO_TRY(jpeg_entropy_decode(c, ws, data, n, &j));
        memcpy(out, ws->h_coef, *n_coefs * sizeof(int16_t));
        return UVO_OK;
    }
    JhWs* q = jh_ws(c);
    UVO_TRY(jh_prepare(c, data, n, 0, sub_words, &q->job[0]));
    *n_coefs = q->job[0].j.total_blocks * 64;
    if (*n_coefs > cap) { c->err = "uvo_jpeg_coefficients: output capacity too small"; return UVO_CAPACITY; }
    Ctx* lane = c;
    UVO_TRY(jh_plan(c, &lane, 1, 1, q->job));
    const uint8_t* unused = nullptr;
    UVO_TRY(jh_queue(c, c, 0, q->job[0], false, true, &unused));
    UVO_HIP_TRY(c, hipMemcpyAsync(out, q->slot[0].d_coef, *n_coefs * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return UVO_OK;
}
uvo_status codec_entropy_stats(Ctx* c, int* n_sub, int* n_groups, int* rounds_in_group, int* rounds_across, size_t* scan_bytes)
{
    const JhSlot& s = jh_ws(c)->slot[0];
    if (!s.have_stats) { c->err = "uvo_jpeg_entropy_stats: no device decode has run on this context (uvo_decode_image after uvo_ctx_set_jpeg_entropy(c, 1), or uvo_jpeg_coefficients)"; return UVO_INVALID_ARG; }
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_sub) *n_sub = s.n_sub;
    if (n_groups) *n_groups = s.n_groups;
    if (rounds_in_group) *rounds_in_group = s.h_stats[0];
    if (rounds_across) *rounds_across = s.h_stats[1];
    if (scan_bytes) *scan_bytes = s.scan_bytes;
    return UVO_OK;
}

// ------------------------------------------------------------------------------------------ orchestration
// PNG samples -> what cv::imdecode(IMREAD_UNCHANGED) returns: grey (sub-byte depths scaled as png_set_expand_gray_1_2_4_to_8 does,
// v * 255 / (2^d - 1)), palette -> B G R, RGB -> B G R, RGBA -> B G R A.  One thread per pixel.
struct PngArgs { int w, h, depth, ctype, stride; uint8_t pal[256][4]; };
__global__ __launch_bounds__(256) void k_png_expand(PngArgs a, const uint8_t* __restrict__ rows, uint8_t* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const uint8_t* src = rows + (size_t)y * a.stride;
    if (a.ctype == 2) {
        uint8_t* d = out + ((size_t)y * a.w + x) * 3;
        d[0] = src[3 * x + 2]; d[1] = src[3 * x + 1]; d[2] = src[3 * x];
    } else if (a.ctype == 6) {
        uint8_t* d = out + ((size_t)y * a.w + x) * 4;
        d[0] = src[4 * x + 2]; d[1] = src[4 * x + 1]; d[2] = src[4 * x]; d[3] = src[4 * x + 3];
    } else {
        int v;                                                // (a packed row is ~w * depth / 8 bytes: src[x] would read past the last one)
        if (a.depth < 8) { const int per = 8 / a.depth, sh = (per - 1 - x % per) * a.depth; v = (src[x / per] >> sh) & ((1 << a.depth) - 1); }
        else v = src[x];
        if (a.ctype == 0) out[(size_t)y * a.w + x] = (uint8_t)(a.depth < 8 ? v * 255 / ((1 << a.depth) - 1) : v);
        else { uint8_t* d = out + ((size_t)y * a.w + x) * 3; d[0] = a.pal[v][0]; d[1] = a.pal[v][1]; d[2] = a.pal[v][2]; }
    }
}

static uvo_status png_decode(Ctx* c, CodecWs* ws, const uint8_t* data, size_t n, const uint8_t** d_out, int* w, int* h, int* channels)
{
    png::Header hd;
    std::vector<uint8_t> idat;
    std::string err;
    if (!png::parse(data, n, &hd, &idat, false, &err)) { c->err = err; return UVO_INVALID_ARG; }
    const size_t stride = png::row_bytes(hd), raw_bytes = stride * (size_t)hd.h;
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));                     // the pinned staging buffer of the previous call is free again
    UVO_TRY(grow(c, reinterpret_cast<void**>(&ws->h_coef), &ws->coef_cap, raw_bytes, true));        // (the JPEG path's pinned / device staging buffers, reused)
    if (!png::scanlines(hd, idat, reinterpret_cast<uint8_t*>(ws->h_coef), &err)) { c->err = err; return UVO_INVALID_ARG; }
    { void* p = ws->d_coef; size_t cap = ws->coef_cap_dev; UVO_TRY(grow(c, &p, &cap, raw_bytes, false)); ws->d_coef = static_cast<int16_t*>(p); ws->coef_cap_dev = cap; }
    const int ch = png::channels_out(hd);
    { void* p = ws->d_out; UVO_TRY(grow(c, &p, &ws->out_cap, (size_t)hd.w * hd.h * ch, false)); ws->d_out = static_cast<uint8_t*>(p); }
    UVO_HIP_TRY(c, hipMemcpyAsync(ws->d_coef, ws->h_coef, raw_bytes, hipMemcpyHostToDevice, c->stream));
    PngArgs a;
    a.w = hd.w; a.h = hd.h; a.depth = hd.depth; a.ctype = hd.ctype; a.stride = (int)stride;
    memcpy(a.pal, hd.pal, sizeof(a.pal));
    hipLaunchKernelGGL(k_png_expand, dim3((hd.w + 63) / 64, (hd.h + 3) / 4), dim3(256), 0, c->stream, a, reinterpret_cast<const uint8_t*>(ws->d_coef), ws->d_out);
    UVO_HIP_TRY(c, hipGetLastError());
    *w = hd.w; *h = hd.h; *channels = ch; *d_out = ws->d_out;
    return UVO_OK;
}

uvo_status codec_decode(Ctx* c, const uint8_t* data, size_t n, int bayer, const uint8_t** d_out, int* w, int* h, int* channels)
{
    if (!c->codec_ws) c->codec_ws = new CodecWs();
    CodecWs* ws = static_cast<CodecWs*>(c->codec_ws);
    if (png::is_png(data, n)) {
        UVO_TRY(png_decode(c, ws, data, n, d_out, w, h, channels));
        if (bayer) {
            if (*channels != 1) { c->err = "a bayer-format message must decode to one channel"; return UVO_INVALID_ARG; }
            { void* p = ws->d_out2; UVO_TRY(grow(c, &p, &ws->out2_cap, (size_t)*w * *h * 3, false)); ws->d_out2 = static_cast<uint8_t*>(p); }
            hipLaunchKernelGGL(k_bayer_bggr, dim3((*w + 63) / 64, (*h + 3) / 4), dim3(256), 0, c->stream, ws->d_out, *w, *h, *w, ws->d_out2);
            UVO_HIP_TRY(c, hipGetLastError());
            *channels = 3; *d_out = ws->d_out2;
        }
        UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
        return UVO_OK;
    }
    if (ws->jh && static_cast<JhWs*>(ws->jh)->where == 1) return jpeg_decode_device(c, data, n, bayer, d_out, w, h, channels);
    Jpeg j;
    memset(j.quant, 0, sizeof(j.quant));
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));                     // the pinned coefficient buffer of the previous call is free again
    UVO_TRY(jpeg_entropy_decode(c, ws, data, n, &j));
    if (!ws->d_quant) UVO_HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&ws->d_quant), sizeof(j.quant)));
    const size_t coef_bytes = j.total_blocks * 64 * sizeof(int16_t);
    { void* p = ws->d_coef; size_t cap = ws->coef_cap_dev; UVO_TRY(grow(c, &p, &cap, coef_bytes, false)); ws->d_coef = static_cast<int16_t*>(p); ws->coef_cap_dev = cap; }
    IdctArgs ia; ColourArgs ca;
    memset(&ia, 0, sizeof(ia)); memset(&ca, 0, sizeof(ca));
    size_t poff = 0;
    for (int k = 0; k < j.ncomp; k++) {
        const Comp& q = j.comp[k];
        ia.comp[k] = { q.coef_off, q.bw, q.bh, q.tq, poff };
        ca.plane_off[k] = poff; ca.pw[k] = q.bw * 8;
        ca.dw[k] = (j.w * q.h + j.hmax - 1) / j.hmax; ca.dh[k] = (j.h * q.v + j.vmax - 1) / j.vmax;      // jdmaster.c downsampled_width / height
        ca.hs[k] = j.hmax / q.h; ca.vs[k] = j.vmax / q.v;
        poff += (size_t)q.bw * q.bh * 64;
    }
    for (int k = j.ncomp; k < 3; k++) ia.comp[k] = ia.comp[0];
    ia.ncomp = j.ncomp; ia.total_blocks = j.total_blocks;
    ca.ncomp = j.ncomp; ca.w = j.w; ca.h = j.h;
    { void* p = ws->d_planes; UVO_TRY(grow(c, &p, &ws->planes_cap, poff, false)); ws->d_planes = static_cast<uint8_t*>(p); }
    const size_t out_bytes = (size_t)j.w * j.h * j.ncomp;
    { void* p = ws->d_out; UVO_TRY(grow(c, &p, &ws->out_cap, out_bytes, false)); ws->d_out = static_cast<uint8_t*>(p); }
    UVO_HIP_TRY(c, hipMemcpyAsync(ws->d_coef, ws->h_coef, coef_bytes, hipMemcpyHostToDevice, c->stream));
    UVO_HIP_TRY(c, hipMemcpyAsync(ws->d_quant, j.quant, sizeof(j.quant), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((j.total_blocks + 31) / 32)), dim3(256), 0, c->stream, ia, ws->d_coef, ws->d_quant, ws->d_planes);
    hipLaunchKernelGGL(k_jpeg_colour, dim3((j.w + 63) / 64, (j.h + 3) / 4), dim3(256), 0, c->stream, ca, ws->d_planes, ws->d_out);
    UVO_HIP_TRY(c, hipGetLastError());
    *w = j.w; *h = j.h; *channels = j.ncomp; *d_out = ws->d_out;
    if (bayer) {
        if (j.ncomp != 1) { c->err = "a bayer-format message must decode to one channel"; return UVO_INVALID_ARG; }
        { void* p = ws->d_out2; UVO_TRY(grow(c, &p, &ws->out2_cap, (size_t)j.w * j.h * 3, false)); ws->d_out2 = static_cast<uint8_t*>(p); }
        hipLaunchKernelGGL(k_bayer_bggr, dim3((j.w + 63) / 64, (j.h + 3) / 4), dim3(256), 0, c->stream, ws->d_out, j.w, j.h, j.w, ws->d_out2);
        UVO_HIP_TRY(c, hipGetLastError());
        *channels = 3; *d_out = ws->d_out2;
    }
    // j.quant lives on this stack frame and is still being copied: wait for the upload before returning
    UVO_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return UVO_OK;
}

// Size and channel count of what codec_decode would return, from the headers alone (no entropy decoding, no device work)
uvo_status codec_peek(Ctx* c, const uint8_t* data, size_t n, int bayer, int* w, int* h, int* channels)
{
    if (png::is_png(data, n)) {
        png::Header hd; std::string err;
        if (!png::parse(data, n, &hd, nullptr, true, &err)) { c->err = err; return UVO_INVALID_ARG; }
        const int ch = png::channels_out(hd);
        if (bayer && ch != 1) { c->err = "a bayer-format message must decode to one channel"; return UVO_INVALID_ARG; }
        *w = hd.w; *h = hd.h; *channels = bayer ? 3 : ch;
        return UVO_OK;
    }
    Jpeg j;
    memset(j.quant, 0, sizeof(j.quant));
    UVO_TRY(jpeg_entropy_decode(c, nullptr, data, n, &j, true));
    if (bayer && j.ncomp != 1) { c->err = "a bayer-format message must decode to one channel"; return UVO_INVALID_ARG; }
    *w = j.w; *h = j.h; *channels = bayer ? 3 : j.ncomp;
    return UVO_OK;
}

uvo_status codec_bayer(Ctx* c, const uint8_t* bayer, int w, int h, int stride, int mem, const uint8_t** d_out)
{
    if (!c->codec_ws) c->codec_ws = new CodecWs();
    CodecWs* ws = static_cast<CodecWs*>(c->codec_ws);
    { void* p = ws->d_out; UVO_TRY(grow(c, &p, &ws->out_cap, (size_t)w * h, false)); ws->d_out = static_cast<uint8_t*>(p); }
    { void* p = ws->d_out2; UVO_TRY(grow(c, &p, &ws->out2_cap, (size_t)w * h * 3, false)); ws->d_out2 = static_cast<uint8_t*>(p); }
    UVO_HIP_TRY(c, hipMemcpy2DAsync(ws->d_out, w, bayer, stride, w, h, mem == UVO_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bayer_bggr, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, c->stream, ws->d_out, w, h, w, ws->d_out2);
    UVO_HIP_TRY(c, hipGetLastError());
    *d_out = ws->d_out2;
    return UVO_OK;
}

}  // namespace uvo
