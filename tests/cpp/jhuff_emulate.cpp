// jhuff_emulate.cpp -- CPU emulation of the device JPEG entropy decoder (ergo_uvo_amd/csrc/uvo_jhuff.h + the k_jh_* kernels of
// codec.hip), the kernels' threads as loops, against a plain sequential decode written here.  Built by tests/test_jpeg_entropy_cpu.py
// with -fsanitize=address,undefined and run as a program of its own.
//   jhuff_emulate FILE.jpg ...   every stream: sub_words 4 / 8 / 32 x workgroups of 16 / 256 subsequences must reproduce the sequential
//                                coefficients; then the stream cut at 1/3 and 2/3 of its scan and with one scan byte inverted must
//                                terminate within the bounds (no comparison: a damaged stream decodes to some picture)
// Prints one line per run with the rounds; exit status 0 when everything held.
#include "../../ergo_uvo_amd/csrc/uvo_jhuff.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

using namespace uvo::jhuff;

static const uint8_t kNatural[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

struct RawTable { uint8_t bits[17] = {0}, vals[256] = {0}; bool present = false; };
struct Picture {
    int w = 0, h = 0, ncomp = 0, restart = 0, mcux = 0, mcuy = 0;
    int ch[3] = {1, 1, 1}, cv[3] = {1, 1, 1}, id[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    RawTable dc[4], ac[4];
    size_t scan_off = 0;
};
static int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

static bool parse(const std::vector<uint8_t>& d, Picture* j)
{
    const size_t n = d.size();
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return false;
    size_t pos = 2;
    while (pos + 4 <= n) {
        if (d[pos] != 0xFF) { pos++; continue; }
        const int m = d[pos + 1];
        if (m == 0xFF) { pos++; continue; }
        pos += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) break;
        const int len = be16(&d[pos]);
        if (len < 2 || pos + len > n) return false;
        const uint8_t* s = &d[pos + 2]; const int sl = len - 2;
        if (m == 0xC4) {
            for (int o = 0; o + 17 <= sl;) {
                const int tc = s[o] >> 4, th = s[o] & 15; o++;
                if (th > 3 || tc > 1) return false;
                RawTable& t = tc ? j->ac[th] : j->dc[th];
                int cnt = 0;
                for (int l = 1; l <= 16; l++) { t.bits[l] = s[o + l - 1]; cnt += t.bits[l]; }
                o += 16;
                if (cnt > 256 || o + cnt > sl) return false;
                memset(t.vals, 0, sizeof(t.vals)); memcpy(t.vals, s + o, (size_t)cnt); o += cnt;
                t.present = true;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            j->h = be16(s + 1); j->w = be16(s + 3); j->ncomp = s[5];
            if (j->ncomp != 1 && j->ncomp != 3) return false;
            int hmax = 1, vmax = 1;
            for (int k = 0; k < j->ncomp; k++) { j->id[k] = s[6 + 3 * k]; j->ch[k] = s[7 + 3 * k] >> 4; j->cv[k] = s[7 + 3 * k] & 15; hmax = j->ch[k] > hmax ? j->ch[k] : hmax; vmax = j->cv[k] > vmax ? j->cv[k] : vmax; }
            if (j->ncomp == 1) { j->ch[0] = j->cv[0] = 1; hmax = vmax = 1; }
            j->mcux = (j->w + 8 * hmax - 1) / (8 * hmax); j->mcuy = (j->h + 8 * vmax - 1) / (8 * vmax);
        } else if (m == 0xDD) j->restart = be16(s);
        else if (m == 0xDA) {
            for (int i = 0; i < s[0]; i++)
                for (int k = 0; k < j->ncomp; k++)
                    if (j->id[k] == s[1 + 2 * i]) { j->td[k] = s[2 + 2 * i] >> 4; j->ta[k] = s[2 + 2 * i] & 15; }
            j->scan_off = pos + len;
            return true;
        }
        pos += len;
    }
    return false;
}

// ---- the plain sequential decode: bit by bit, code by code, one block after the other
struct Bits {
    const uint8_t* p; const uint8_t* end; bool marker = false;
    uint32_t acc = 0; int n = 0;
    int bit()
    {
        if (n == 0) {
            int c = 0;
            if (!marker && p < end) {
                c = *p++;
                if (c == 0xFF) { const int c2 = p < end ? *p : 0xD9; if (c2 == 0) p++; else { marker = true; p--; c = 0; } }
            }
            acc = (uint32_t)c; n = 8;
        }
        return (acc >> --n) & 1;
    }
    int get(int k) { int v = 0; while (k-- > 0) v = (v << 1) | bit(); return v; }
};
static int huff_symbol(Bits& b, const RawTable& t)
{
    int code = 0, first = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        code = (code << 1) | b.bit();
        if (code - first < t.bits[l]) return t.vals[k + code - first];
        k += t.bits[l]; first = (first + t.bits[l]) << 1;
    }
    return 0;
}
static std::vector<int16_t> sequential(const std::vector<uint8_t>& d, const Picture& j, const Scan& s)
{
    std::vector<int16_t> coef((size_t)s.total_blocks * 64, 0);
    Bits b; b.p = &d[0] + j.scan_off; b.end = &d[0] + d.size();
    int left = j.restart;
    unsigned pred[3] = {0, 0, 0};
    uint32_t blk = 0;
    for (int m = 0; m < j.mcux * j.mcuy; m++) {
        if (j.restart && left == 0) {
            b.n = 0;
            if (b.marker) { b.p += 2; b.marker = false; }
            else { while (b.p + 1 < b.end && !(b.p[0] == 0xFF && b.p[1] >= 0xD0 && b.p[1] <= 0xD7)) b.p++; if (b.p + 1 < b.end) b.p += 2; }
            pred[0] = pred[1] = pred[2] = 0;
            left = j.restart;
        }
        for (uint32_t q = 0; q < s.bpm; q++, blk++) {
            const int k = s.blk_comp[q];
            int16_t* out = &coef[slot_block(s, blk) * 64];
            const int t = huff_symbol(b, j.dc[j.td[k]]) & 15;
            pred[k] += (unsigned)(t ? extend(b.get(t), t) : 0);
            out[0] = (int16_t)(int)pred[k];
            for (int kk = 1; kk < 64;) {
                const int rs = huff_symbol(b, j.ac[j.ta[k]]), r = rs >> 4, sz = rs & 15;
                if (sz == 0) { if (r == 15) { kk += 16; continue; } break; }
                kk += r;
                if (kk > 63) break;
                out[kNatural[kk]] = (int16_t)extend(b.get(sz), sz);
                kk++;
            }
        }
        if (j.restart) left--;
    }
    return coef;
}

// ---- the kernels, their threads as loops
struct Emulated { std::vector<int16_t> coef; int rounds_in_group = 0, rounds_across = 0; uint32_t n_sub = 0, n_groups = 0; bool bounded = true; };

// jh_seg_scan of codec.hip: the inclusive scan over kWide (flag, value) partials in log steps, every step reading the state before it
static const uint32_t kWide = 1024;
static void seg_scan(std::vector<uint32_t>& val, std::vector<uint32_t>& flag)
{
    for (uint32_t o = 1; o < kWide; o <<= 1) {
        const std::vector<uint32_t> v0 = val, f0 = flag;
        for (uint32_t t = o; t < kWide; t++) if (!f0[t]) { val[t] = v0[t] + v0[t - o]; flag[t] = f0[t - o]; }
    }
}

static bool emulate(const uint8_t* scan_src, size_t scan_n, Scan s, const Table* tabs, uint32_t sub_words, uint32_t group, Emulated* out)
{
    s.sub_words = sub_words;
    std::vector<uint8_t> stage(stage_bound_bytes(s, scan_n, sub_words));
    std::vector<uint32_t> info(stage_bound_subs(s, scan_n, sub_words));
    Staged sg;
    if (!stage_scan(scan_src, scan_n, sub_words, expected_intervals(s), stage.data(), stage.size(), info.data(), info.size(), &sg)) { fprintf(stderr, "staging failed\n"); return false; }
    s.n_bytes = sg.n_bytes; s.n_sub = sg.n_sub; s.n_iv = sg.n_iv;
    stage.resize((size_t)sg.n_bytes + kPadBytes);                // (so that the sanitizer sees any read behind the padding)
    const uint8_t* scan = stage.data();
    const uint32_t n = s.n_sub, sub_bits = sub_words * 32, n_groups = (n + group - 1) / group;
    std::vector<State> entry(n), exit_(n), incoming(n_groups);
    std::vector<uint32_t> slots(n), first(n);
    // k_jh_pass1
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t i0 = g * group, i1 = i0 + group < n ? i0 + group : n;
        for (uint32_t i = i0; i < i1; i++) { entry[i] = State{ i * sub_bits, 0 }; exit_[i] = entry[i]; slots[i] = decode_span(tabs, s, scan, &exit_[i], (i + 1) * sub_bits, NoEmit()); }
        int rounds = 0;
        uint32_t r = 0;
        for (; r < group - 1; r++) {
            std::vector<State> prev(i1 - i0);
            bool any = false;
            for (uint32_t i = i0; i < i1; i++) {
                const bool fixed = i == i0 || (info[i] & 1);
                prev[i - i0] = fixed ? entry[i] : exit_[i - 1];
                any = any || !same(prev[i - i0], entry[i]);
            }
            if (!any) break;
            rounds++;
            for (uint32_t i = i0; i < i1; i++)
                if (!same(prev[i - i0], entry[i])) { entry[i] = prev[i - i0]; exit_[i] = entry[i]; slots[i] = decode_span(tabs, s, scan, &exit_[i], (i + 1) * sub_bits, NoEmit()); }
        }
        if (r == group - 1) {                                    // the bound was reached: one more look must find nothing to do
            for (uint32_t i = i0 + 1; i < i1; i++) if (!(info[i] & 1) && !same(exit_[i - 1], entry[i])) out->bounded = false;
        }
        out->rounds_in_group = rounds > out->rounds_in_group ? rounds : out->rounds_in_group;
    }
    // k_jh_cross
    {
        uint32_t r = 0;
        bool settled = false;
        for (; r < n_groups; r++) {
            bool changed = false;
            for (uint32_t g = 1; g < n_groups; g++) incoming[g] = exit_[g * group - 1];
            for (uint32_t g = 1; g < n_groups; g++) {
                const uint32_t i0 = g * group, i1 = i0 + group < n ? i0 + group : n;
                if (info[i0] & 1) continue;
                State cur = incoming[g];
                if (same(cur, entry[i0])) continue;
                changed = true;
                for (uint32_t i = i0; i < i1; i++) {
                    if (i > i0 && ((info[i] & 1) || same(cur, entry[i]))) break;
                    entry[i] = cur;
                    slots[i] = decode_span(tabs, s, scan, &cur, (i + 1) * sub_bits, NoEmit());
                    exit_[i] = cur;
                }
            }
            if (!changed) { settled = true; break; }
            out->rounds_across++;
        }
        if (!settled) out->bounded = false;
        const uint32_t iv_slots = s.iv_mcus * s.bpm * 64;
        // the chunked scan as the kernel's 1024 threads run it: a partial per thread, the log-step scan, then every thread's chunk again
        const uint32_t per = (n + kWide - 1) / kWide;
        std::vector<uint32_t> val(kWide, 0), flag(kWide, 0);
        for (uint32_t t = 0; t < kWide; t++)
            for (uint32_t i = t * per; i < (t + 1) * per && i < n; i++) { if (info[i] & 1) { flag[t] = 1; val[t] = (info[i] >> 1) * iv_slots; } val[t] += slots[i]; }
        seg_scan(val, flag);
        for (uint32_t t = 0; t < kWide; t++) {
            uint32_t cur = t ? val[t - 1] : 0;
            for (uint32_t i = t * per; i < (t + 1) * per && i < n; i++) { if (info[i] & 1) cur = (info[i] >> 1) * iv_slots; first[i] = cur; cur += slots[i]; }
        }
        uint32_t cur = 0;                                        // ... and it is the plain sequential scan
        for (uint32_t i = 0; i < n; i++) { if (info[i] & 1) cur = (info[i] >> 1) * iv_slots; if (first[i] != cur) out->bounded = false; cur += slots[i]; }
    }
    // every subsequence must now follow from its predecessor (the fixed point)
    for (uint32_t i = 1; i < n; i++) if (!(info[i] & 1) && !same(exit_[i - 1], entry[i])) out->bounded = false;
    // k_jh_emit
    out->coef.assign((size_t)s.total_blocks * 64, 0);
    const size_t n_coef = out->coef.size();
    const unsigned long long total_slots = (unsigned long long)s.total_blocks * 64;
    for (uint32_t i = 0; i < n; i++) {
        State st = entry[i];
        const unsigned long long iv_end = ((unsigned long long)(info[i] >> 1) + 1) * s.iv_mcus * s.bpm * 64, slot_end = iv_end < total_slots ? iv_end : total_slots;
        const uint32_t f = first[i];
        (void)decode_span(tabs, s, scan, &st, (i + 1) * sub_bits, [&](uint32_t rel, int v) {
            const uint32_t slot = f + rel;
            if (slot >= slot_end) return;
            const size_t idx = slot_block(s, slot >> 6) * 64 + kNatural[slot & 63];
            if (idx < n_coef) out->coef[idx] = (int16_t)v;
        });
    }
    // k_jh_dc
    for (uint32_t k = 0; k < 3 && s.comp_bw[k]; k++) {
        const uint32_t h = s.comp_h[k], hv = h * s.comp_v[k], ne = s.total_mcus * hv, seg = s.iv_mcus * hv;
        auto at = [&](uint32_t el) -> size_t {
            const uint32_t mcu = el / hv, jj = el - mcu * hv, by = jj / h, bx = jj - by * h, my = mcu / s.mcux, mx = mcu - my * s.mcux;
            const size_t idx = ((size_t)s.comp_off[k] + (size_t)(my * s.comp_v[k] + by) * s.comp_bw[k] + (mx * h + bx)) * 64;
            return idx < n_coef ? idx : n_coef;
        };
        const uint32_t per = (ne + kWide - 1) / kWide;           // as k_jh_dc's 1024 threads: partials, the log-step scan, the chunks again
        std::vector<uint32_t> val(kWide, 0), flag(kWide, 0);
        for (uint32_t t = 0; t < kWide; t++)
            for (uint32_t el = t * per; el < (t + 1) * per && el < ne; el++) {
                if (el % seg == 0) { flag[t] = 1; val[t] = 0; }
                const size_t idx = at(el);
                val[t] += idx < n_coef ? (uint32_t)(int)out->coef[idx] : 0u;
            }
        seg_scan(val, flag);
        for (uint32_t t = 0; t < kWide; t++) {
            uint32_t cur = t ? val[t - 1] : 0;
            for (uint32_t el = t * per; el < (t + 1) * per && el < ne; el++) {
                if (el % seg == 0) cur = 0;
                const size_t idx = at(el);
                if (idx >= n_coef) continue;
                cur += (uint32_t)(int)out->coef[idx];
                out->coef[idx] = (int16_t)(int)cur;
            }
        }
    }
    out->n_sub = n; out->n_groups = n_groups;
    return true;
}

int main(int argc, char** argv)
{
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + got);
        fclose(f);
        Picture j;
        if (!parse(d, &j)) { fprintf(stderr, "%s: headers not understood\n", argv[a]); return 2; }
        Table tabs[kMaxTables];
        int map_dc[4] = {-1, -1, -1, -1}, map_ac[4] = {-1, -1, -1, -1}, tdc[3], tac[3], nt = 0;
        for (int k = 0; k < j.ncomp; k++) {
            if (map_dc[j.td[k]] < 0) { map_dc[j.td[k]] = nt; if (!build_table(&tabs[nt++], j.dc[j.td[k]].bits, j.dc[j.td[k]].vals)) return 2; }
            if (map_ac[j.ta[k]] < 0) { map_ac[j.ta[k]] = nt; if (!build_table(&tabs[nt++], j.ac[j.ta[k]].bits, j.ac[j.ta[k]].vals)) return 2; }
            tdc[k] = map_dc[j.td[k]]; tac[k] = map_ac[j.ta[k]];
        }
        Scan s;
        make_scan(&s, j.ncomp, j.ch, j.cv, tdc, tac, j.mcux, j.mcuy, j.restart);
        const std::vector<int16_t> want = sequential(d, j, s);
        const size_t scan_n = d.size() - j.scan_off;
        const uint32_t subs[3] = {4, 8, 32}, groups[2] = {16, 256};
        for (uint32_t sw : subs)
            for (uint32_t g : groups) {
                Emulated e;
                if (!emulate(&d[j.scan_off], scan_n, s, tabs, sw, g, &e)) return 2;
                const bool same_coefs = e.coef == want;
                printf("%s sub_words=%u group=%u n_sub=%u n_groups=%u rounds_in_group=%d rounds_across=%d %s\n", argv[a], sw, g, e.n_sub, e.n_groups, e.rounds_in_group,
                       e.rounds_across, same_coefs && e.bounded ? "ok" : (same_coefs ? "UNBOUNDED" : "MISMATCH"));
                if (!same_coefs || !e.bounded) bad++;
            }
        // damaged streams: termination within the bounds, every index in range (the sanitizers watch)
        for (int v = 0; v < 3; v++) {
            std::vector<uint8_t> x(d.begin() + (long)j.scan_off, d.end());
            if (v == 0) x.resize(scan_n / 3);
            else if (v == 1) x.resize(2 * scan_n / 3);
            else if (scan_n > 2) x[scan_n / 2] = (uint8_t)~x[scan_n / 2];
            x.push_back(0);                                      // (data() of an empty vector may be null)
            for (uint32_t sw : subs)
                for (uint32_t g : groups) {
                    Emulated e;
                    if (!emulate(x.data(), x.size() - 1, s, tabs, sw, g, &e)) return 2;
                    printf("%s damaged=%d sub_words=%u group=%u rounds_in_group=%d rounds_across=%d %s\n", argv[a], v, sw, g, e.rounds_in_group, e.rounds_across, e.bounded ? "ok" : "UNBOUNDED");
                    if (!e.bounded) bad++;
                }
        }
    }
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
