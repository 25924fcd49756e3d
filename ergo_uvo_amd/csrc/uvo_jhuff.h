// uvo_jhuff.h -- one statement of baseline-JPEG Huffman decoding for the host and the device: the table build, the staging of a
// scan and the span decoder.  The device entropy decoder's kernels (codec.hip) and its CPU emulation (tests/cpp/jhuff_emulate.cpp)
// both call this code; no HIP header is needed on the host.
//
// The scheme ("JPEG entropy decoding on the device"): the scan is staged without its stuffing bytes and cut into
// subsequences of sub_words 32-bit words.  The state of a decoder between two symbols is (p, b, z): the bit position in the staged
// scan, the index of the current block inside the MCU (it selects the DC / AC tables) and the zigzag position (0: a DC symbol is due).
// Two decoders that agree on a state agree from there on, and Huffman streams self-synchronise, so every subsequence is first decoded
// from (its first bit, 0, 0) and then again from its predecessor's exit state until nothing changes.  A symbol advances the output by
// coefficient SLOTS (DC: 1, AC (r, s): r + 1, ZRL: min(16, 64 - z), EOB: 64 - z; every block is exactly 64 slots), so a scan of the
// slot counts gives every subsequence its first absolute slot, slot / 64 being the block in scan order and slot % 64 == z.
// What the symbol step does on damaged data follows the host decoder in codec.hip: an absent code consumes 16 bits and yields symbol 0,
// a run past position 63 ends the block without reading its extra bits, bits beyond the scan's end are zeros.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define UVO_JH_HD __host__ __device__ inline
#define UVO_JH_H __host__ inline
#else
#define UVO_JH_HD inline
#define UVO_JH_H inline
#endif

namespace uvo {
namespace jhuff {

constexpr int kMaxMcuBlocks = 12;        // three components of at most 2 x 2 blocks
constexpr int kMaxTables = 6;            // the scan's tables, compacted: at most one DC and one AC table per component
constexpr uint32_t kPadBytes = 16;       // zeros behind the staged scan: a reader clamped to the end reads 64 bits of them

// canonical Huffman table: a 9-bit first-level lookup ((length << 8) | symbol, 0: longer than 9 bits), longer codes by the length walk
struct Table {
    uint16_t fast[512];
    int32_t mincode[17], maxcode[17], valptr[17];
    uint8_t vals[256];
};

// bits[1 .. 16]: the number of codes of each length; vals: the symbols in code order.
// false: the lengths do not form a prefix code, or there are more than 256 symbols
UVO_JH_HD bool build_table(Table* t, const uint8_t* bits, const uint8_t* vals)
{
    int code = 0, k = 0, cnt = 0;
    for (int i = 0; i < 512; i++) t->fast[i] = 0;
    for (int l = 1; l <= 16; l++) cnt += bits[l];
    if (cnt > 256) return false;
    for (int i = 0; i < 256; i++) t->vals[i] = i < cnt ? vals[i] : 0;
    t->mincode[0] = 0; t->maxcode[0] = -1; t->valptr[0] = 0;
    for (int l = 1; l <= 16; l++) {
        if (code + bits[l] > (1 << l)) return false;
        t->valptr[l] = k; t->mincode[l] = code;
        for (int i = 0; i < bits[l]; i++, k++, code++)
            if (l <= 9) { const int lo = code << (9 - l); for (int f = 0; f < (1 << (9 - l)); f++) t->fast[lo + f] = (uint16_t)((l << 8) | vals[k]); }
        t->maxcode[l] = bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    return true;
}

// the layout of one interleaved scan: which tables a block of the MCU uses and where its coefficients go.  The coefficient buffer
// holds component after component, each the raster of its MCU-padded blocks, 64 coefficients in natural order per block.
struct Scan {
    uint32_t n_bytes = 0;                // staged bytes holding subsequences (kPadBytes zeros follow)
    uint32_t sub_words = 0, n_sub = 0, n_iv = 0;
    uint32_t bpm = 0;                    // blocks per MCU
    uint32_t mcux = 0, total_mcus = 0, iv_mcus = 0;      // iv_mcus: MCUs per restart interval (total_mcus without restarts)
    uint32_t total_blocks = 0;
    uint32_t comp_off[3] = {0, 0, 0}, comp_bw[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
    uint8_t blk_dc[kMaxMcuBlocks], blk_ac[kMaxMcuBlocks], blk_comp[kMaxMcuBlocks], blk_by[kMaxMcuBlocks], blk_bx[kMaxMcuBlocks];
};

// ncomp components of h[k] x v[k] blocks per MCU, their compact DC / AC table indices, the picture's MCU grid, the restart interval
UVO_JH_HD void make_scan(Scan* s, int ncomp, const int* h, const int* v, const int* dc_tab, const int* ac_tab, int mcux, int mcuy, int restart)
{
    uint32_t b = 0, off = 0;
    for (int i = 0; i < kMaxMcuBlocks; i++) s->blk_dc[i] = s->blk_ac[i] = s->blk_comp[i] = s->blk_by[i] = s->blk_bx[i] = 0;
    for (int k = 0; k < ncomp && k < 3; k++) {
        s->comp_off[k] = off; s->comp_bw[k] = (uint32_t)(mcux * h[k]); s->comp_h[k] = (uint32_t)h[k]; s->comp_v[k] = (uint32_t)v[k];
        off += (uint32_t)(mcux * h[k]) * (uint32_t)(mcuy * v[k]);
        for (int by = 0; by < v[k]; by++)
            for (int bx = 0; bx < h[k]; bx++, b++) {
                if (b >= (uint32_t)kMaxMcuBlocks) continue;
                s->blk_dc[b] = (uint8_t)dc_tab[k]; s->blk_ac[b] = (uint8_t)ac_tab[k]; s->blk_comp[b] = (uint8_t)k; s->blk_by[b] = (uint8_t)by; s->blk_bx[b] = (uint8_t)bx;
            }
    }
    s->bpm = b < (uint32_t)kMaxMcuBlocks ? b : (uint32_t)kMaxMcuBlocks;
    s->mcux = (uint32_t)mcux; s->total_mcus = (uint32_t)mcux * (uint32_t)mcuy;
    s->iv_mcus = restart > 0 && (uint32_t)restart < s->total_mcus ? (uint32_t)restart : s->total_mcus;
    s->total_blocks = off;
}
UVO_JH_HD uint32_t expected_intervals(const Scan& s) { return s.iv_mcus ? (s.total_mcus + s.iv_mcus - 1) / s.iv_mcus : 1; }
// staged bytes and subsequences that a scan of n source bytes can need at most (every interval is padded to a subsequence boundary)
UVO_JH_HD size_t stage_bound_bytes(const Scan& s, size_t n, uint32_t sub_words) { return n + ((size_t)expected_intervals(s) + 1) * 4 * sub_words + kPadBytes; }
UVO_JH_HD size_t stage_bound_subs(const Scan& s, size_t n, uint32_t sub_words) { return n / (4 * (size_t)sub_words) + expected_intervals(s) + 1; }

// index of the coefficient of absolute slot `slot` (scan order) in the coefficient buffer, natural order inside the block
UVO_JH_HD size_t slot_block(const Scan& s, uint32_t blk)
{
    const uint32_t mcu = blk / s.bpm, b = blk - mcu * s.bpm, my = mcu / s.mcux, mx = mcu - my * s.mcux, k = s.blk_comp[b];
    return (size_t)s.comp_off[k] + (size_t)(my * s.comp_v[k] + s.blk_by[b]) * s.comp_bw[k] + (mx * s.comp_h[k] + s.blk_bx[b]);
}

// Stages the entropy-coded bytes src[0 .. n) of a scan: stuffing bytes (FF 00) removed, every restart interval (FF D0 .. FF D7, at
// most max_iv intervals) moved to a subsequence boundary behind zeros, any other marker ends the scan.  No Huffman code is decoded.
// sub_info[i] = (interval << 1) | (1 if subsequence i is its interval's first).  dst is zeroed from the last data byte to
// n_bytes + kPadBytes.  false: a capacity is too small (stage_bound_*).  Host only (it runs on the calling thread).
struct Staged { uint32_t n_bytes = 0, n_sub = 0, n_iv = 0; size_t consumed = 0; };
UVO_JH_H bool stage_scan(const uint8_t* src, size_t n, uint32_t sub_words, uint32_t max_iv, uint8_t* dst, size_t cap_bytes, uint32_t* sub_info, size_t cap_sub, Staged* out)
{
    const size_t sub_bytes = (size_t)sub_words * 4;
    size_t o = 0, iv_begin = 0, pos = 0, n_sub = 0;
    uint32_t iv = 0;
    if (sub_bytes == 0 || max_iv == 0) return false;
    auto close_interval = [&]() -> bool {
        size_t e = (o + sub_bytes - 1) / sub_bytes * sub_bytes;
        if (e == iv_begin) e += sub_bytes;                       // an empty interval is one subsequence of zeros
        if (e + kPadBytes > cap_bytes || n_sub + (e - iv_begin) / sub_bytes > cap_sub) return false;
        memset(dst + o, 0, e - o);
        for (size_t b = iv_begin; b < e; b += sub_bytes) sub_info[n_sub++] = (iv << 1) | (b == iv_begin ? 1u : 0u);
        o = e; iv_begin = e; iv++;
        return true;
    };
    for (;;) {
        const uint8_t* ff = pos < n ? static_cast<const uint8_t*>(memchr(src + pos, 0xFF, n - pos)) : nullptr;
        const size_t run = ff ? (size_t)(ff - (src + pos)) : n - pos;
        if (o + run + 1 + sub_bytes + kPadBytes > cap_bytes) return false;
        memcpy(dst + o, src + pos, run);
        o += run; pos += run;
        if (!ff) break;
        const int c2 = pos + 1 < n ? src[pos + 1] : 0xD9;
        if (c2 == 0) { dst[o++] = 0xFF; pos += 2; continue; }
        if (c2 >= 0xD0 && c2 <= 0xD7 && iv + 1 < max_iv) { if (!close_interval()) return false; pos += 2; continue; }
        break;                                                   // a marker ends the scan: zeros from here on
    }
    if (!close_interval()) return false;
    memset(dst + o, 0, kPadBytes);
    out->n_bytes = (uint32_t)o; out->n_sub = (uint32_t)n_sub; out->n_iv = iv; out->consumed = pos;
    return true;
}

struct State { uint32_t p, bz; };        // bz = (b << 8) | z
UVO_JH_HD bool same(const State& a, const State& b) { return a.p == b.p && a.bz == b.bz; }

UVO_JH_HD uint32_t load_be32(const uint8_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(p));      // (the staged scan is 4-byte aligned, and so is every offset read)
#endif
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
// the 32 bits at bit position p of the staged scan; positions at or beyond n_bytes * 8 read the zeros behind it
UVO_JH_HD uint32_t peek32(const uint8_t* scan, uint32_t n_bytes, uint32_t p)
{
    uint32_t byte = (p >> 5) * 4;
    byte = byte < n_bytes ? byte : n_bytes;                      // (n_bytes is a multiple of 4; kPadBytes zeros follow)
    const uint32_t w0 = load_be32(scan + byte), w1 = load_be32(scan + byte + 4), sh = p & 31;
    return sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;
}
UVO_JH_HD int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Decodes symbols from state *st while the position is before end_bit (a symbol may end behind it); returns the slots advanced.
// emit(slot relative to the span's first, value) is called for every DC difference and every AC coefficient, in order.
// The trip bound: every symbol consumes at least one bit.
template <class Emit>
UVO_JH_HD uint32_t decode_span(const Table* tabs, const Scan& s, const uint8_t* scan, State* st, uint32_t end_bit, Emit&& emit)
{
    uint32_t p = st->p, b = st->bz >> 8, z = st->bz & 255, slots = 0;
    const uint32_t trips = end_bit > p ? end_bit - p : 0;
    if (b >= s.bpm) b = 0;
    if (z > 63) z = 0;
    for (uint32_t it = 0; it < trips && p < end_bit; it++) {
        const uint32_t w = peek32(scan, s.n_bytes, p);
        const Table& t = tabs[z == 0 ? s.blk_dc[b] : s.blk_ac[b]];
        const uint32_t f = t.fast[w >> 23];
        uint32_t len = 16, sym = 0;                              // an absent code consumes 16 bits and yields symbol 0
        if (f) { len = f >> 8; sym = f & 255; }
        else
            for (int l = 10; l <= 16; l++) {
                const int code = (int)(w >> (32 - l));
                if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) { len = (uint32_t)l; sym = t.vals[(t.valptr[l] + code - t.mincode[l]) & 255]; break; }
            }
        p += len;
        uint32_t adv;
        if (z == 0) {
            const uint32_t sz = sym & 15;
            if (sz) { emit(slots, extend((int)((w << len) >> (32 - sz)), (int)sz)); p += sz; }
            adv = 1;
        } else {
            const uint32_t r = sym >> 4, sz = sym & 15;
            if (sz == 0) adv = r == 15 ? (64 - z < 16 ? 64 - z : 16) : 64 - z;
            else if (z + r > 63) adv = 64 - z;                   // the run passes the block's end: no extra bits are read
            else { emit(slots + r, extend((int)((w << len) >> (32 - sz)), (int)sz)); p += sz; adv = r + 1; }
        }
        slots += adv; z += adv;
        if (z >= 64) { z = 0; b = b + 1 >= s.bpm ? 0 : b + 1; }
    }
    st->p = p; st->bz = (b << 8) | z;
    return slots;
}
struct NoEmit { UVO_JH_HD void operator()(uint32_t, int) const {} };

}  // namespace jhuff
}  // namespace uvo
