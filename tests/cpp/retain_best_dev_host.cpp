// retain_best_dev_host.cpp -- TEST INFRASTRUCTURE, stand-alone (its own main; built plainly and with -fsanitize=address,undefined by
// tests/test_retain_best_dev_host.py).  The workgroup form of retainBest's order (ergo_uvo_amd/csrc/uvo_retain_best_dev.h: stopper
// lists per wave, swap count, closed-form cut, pivot and side choice, the one-lane ends) run on a CPU -- the 16 waves x 64 lanes of
// k_rb_rank (orb.hip) emulated with plain loops, the independent swaps of a pass taken in DESCENDING k to show that their order does not
// matter -- against the real std::nth_element + std::partition (retain_best_std.cpp), element by element, over the families of
// retain_best_host.cpp (grid, fast-scores, musser, adversary) plus all-equal vectors and EVERY vector of length <= 7 over {0, 1, 2} with
// every keep.  Per case the emulation must reach introselect's depth limit exactly when the host replay (uvo_retain_best.h under
// UVO_RB_TRACE) calls rb_heap_select.  Exit status 0: every permutation equal, every depth-limit decision equal, and both outcomes seen.
#define UVO_RB_TRACE
#include "../../ergo_uvo_amd/csrc/uvo_retain_best.h"
#include "../../ergo_uvo_amd/csrc/uvo_retain_best_dev.h"
#include "retain_best_std.cpp"

#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

namespace {
using uvo::RbdItem;
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

long g_cases = 0, g_failed = 0, g_heap_cases = 0, g_heap_differs = 0;

// one pass of the workgroup over v[lo, hi): Hoare against the value pv (MODE 0; returns the cut) or the tail partition against the
// boundary pv (MODE 1; returns the number of items >= pv)
template <int MODE> int emu_pass(std::vector<RbdItem>& v, std::vector<int>& A, std::vector<int>& B, int lo, int hi, float pv)
{
    const int chunk = uvo::rbd_chunk(hi - lo);
    int prefL[uvo::kRbdWaves + 1], prefR[uvo::kRbdWaves + 1];
    prefL[0] = prefR[0] = 0;
    for (int w = 0; w < uvo::kRbdWaves; w++) {
        const int b = lo + w * chunk, e = std::min(b + chunk, hi);
        int nl = 0, nr = 0;
        for (int p0 = b; p0 < e; p0 += uvo::kRbdLanes)
            for (int lane = 0; lane < uvo::kRbdLanes; lane++) {
                const int p = p0 + lane;
                if (p >= e) continue;
                const float x = v.at((size_t)p).r;
                if (uvo::rbd_left_stop<MODE>(x, pv)) A.at((size_t)(b + nl++)) = p;
                if (uvo::rbd_right_stop<MODE>(x, pv)) B.at((size_t)(b + nr++)) = p;
            }
        prefL[w + 1] = prefL[w] + nl; prefR[w + 1] = prefR[w] + nr;
    }
    const int totL = prefL[uvo::kRbdWaves], totR = prefR[uvo::kRbdWaves], kmax = std::min(totL, totR);
    int K = 0;
    for (int k = kmax - 1; k >= 0; k--) {                                                // every k on its own, as the lanes take them
        const int pa = A.at((size_t)uvo::rbd_list_at(lo, chunk, prefL, k)), pb = B.at((size_t)uvo::rbd_list_at(lo, chunk, prefR, totR - 1 - k));
        if (pa < pb) { uvo::rbd_swap(&v.at((size_t)pa), &v.at((size_t)pb)); K++; }
    }
    if (MODE == 1) return totR;
    const bool has_a = K < totL, has_b = K > 0;
    const int a_K = has_a ? A.at((size_t)uvo::rbd_list_at(lo, chunk, prefL, K)) : INT_MAX;
    const int b_Km1 = has_b ? B.at((size_t)uvo::rbd_list_at(lo, chunk, prefR, totR - K)) : hi;
    return uvo::rbd_cut(has_a, a_K, has_b, b_Km1, hi);
}

// k_rb_rank's segment body; returns the count kept, *hit = the depth limit was reached
int emu_retain_best(const float* r, int n, int keep, std::vector<int>* out, int* hit)
{
    std::vector<RbdItem> v((size_t)n);
    std::vector<int> A((size_t)n), B((size_t)n);
    for (int q = 0; q < n; q++) { v[(size_t)q].r = r[q]; v[(size_t)q].i = q; }
    int count;
    *hit = 0;
    if (!(n > keep)) count = n;
    else if (keep == 0) count = 0;
    else {
        int first = 0, last = n, depth = uvo::rbd_depth(n);
        const int nth = keep - 1;
        bool heap = false;
        while (last - first > 3) {
            if (depth == 0) { heap = true; break; }
            --depth;
            const int at[3] = {first + 1, first + (last - first) / 2, last - 1};
            uvo::rbd_swap(&v.at((size_t)first), &v.at((size_t)at[uvo::rbd_median_pick(v.at((size_t)at[0]).r, v.at((size_t)at[1]).r, v.at((size_t)at[2]).r)]));
            const int cut = emu_pass<0>(v, A, B, first + 1, last, v.at((size_t)first).r);
            if (uvo::rbd_take_right(cut, nth)) first = cut; else last = cut;
        }
        if (heap) { uvo::rbd_heap_select(v.data() + first, v.data() + nth + 1, v.data() + last); uvo::rbd_swap(&v.at((size_t)first), &v.at((size_t)nth)); }
        else uvo::rbd_insertion(v.data() + first, v.data() + last);
        count = keep + emu_pass<1>(v, A, B, keep, n, v.at((size_t)nth).r);
        *hit = heap ? 1 : 0;
    }
    out->clear();
    for (int q = 0; q < count; q++) out->push_back(v[(size_t)q].i);
    return count;
}

void run_case(const std::string& name, const std::vector<float>& r, int keep, bool report_heap)
{
    const int n = (int)r.size();
    std::vector<int> want((size_t)n + 1), got, host;
    const int m = retain_best_std(r.data(), n, keep, want.data());
    std::vector<uvo::RbItem> tmp;
    const long before = uvo::rb_heap_select_calls;
    uvo::retain_best_order(r.data(), n, keep, 0, &tmp, &host);
    const long heap = uvo::rb_heap_select_calls - before;
    int hit = 0;
    emu_retain_best(r.data(), n, keep, &got, &hit);
    g_cases++;
    bool ok = (int)got.size() == m;
    int at = -1;
    for (int i = 0; ok && i < m; i++) if (got[(size_t)i] != want[(size_t)i]) { ok = false; at = i; }
    if (!ok) {
        g_failed++;
        if (g_failed <= 10) fprintf(stderr, "MISMATCH %s n=%d keep=%d: std keeps %d, workgroup form %d, first difference at %d\n", name.c_str(), n, keep, m, (int)got.size(), at);
    }
    if ((long)hit != heap) {
        g_heap_differs++;
        if (g_heap_differs <= 10) fprintf(stderr, "DEPTH LIMIT DIFFERS %s n=%d keep=%d: host replay %ld, workgroup form %d\n", name.c_str(), n, keep, heap, hit);
    }
    if (hit) { g_heap_cases++; if (report_heap) printf("depth limit reached: %s n=%d keep=%d\n", name.c_str(), n, keep); }
}

void order(std::vector<float>* v, int kind)
{
    const size_t n = v->size();
    if (kind == 0) return;
    std::sort(v->begin(), v->end());
    if (kind == 2) std::reverse(v->begin(), v->end());
    if (kind == 3) {
        std::vector<float> o(n);
        size_t a = 0, b = n;
        for (size_t i = 0; i < n; i++) { if (i & 1) o[--b] = (*v)[i]; else o[a++] = (*v)[i]; }
        *v = o;
    }
}

std::vector<float> musser(int k)
{
    std::vector<float> a((size_t)2 * k);
    for (int i = 1; i <= k; i++) {
        if (i & 1) { a[(size_t)i - 1] = (float)i; a[(size_t)i] = (float)(k + i); }
        a[(size_t)k + i - 1] = (float)(2 * i);
    }
    return a;
}
}  // namespace

int main()
{
    static const int sizes[] = {1, 2, 3, 4, 5, 7, 16, 33, 100, 1000, 4097, 60000};
    static const int levels[] = {2, 5, 246, 100000};
    static const char* const kinds[] = {"random", "ascending", "descending", "organ-pipe"};
    for (int n : sizes)
        for (int lv : levels)
            for (int kind = 0; kind < 4; kind++) {
                std::vector<float> r((size_t)n);
                for (float& x : r) x = (float)(rnd() % (uint32_t)lv);
                order(&r, kind);
                const int keeps[] = {1, 2, 3, n / 4, n / 2, n - 3, n - 1, n, n + 1};
                for (int keep : keeps) if (keep >= 1) run_case(std::string("grid ") + kinds[kind] + " levels=" + std::to_string(lv), r, keep, false);
            }
    for (int n : {50, 700, 5000, 40000})
        for (int rep = 0; rep < 4; rep++) {
            std::vector<float> r((size_t)n);
            for (float& x : r) { int s = 9; while (s < 254 && rnd() % 100 < 93) s++; x = (float)s; }
            for (int keep : {1, n / 10, n / 3, n / 2, n - 1}) if (keep >= 1) run_case("fast-scores", r, keep, false);
        }
    for (int k : {8, 32, 100, 512, 2048, 10000}) {
        for (int variant = 0; variant < 4; variant++) {
            std::vector<float> r = musser(k);
            if (variant & 1) for (float& x : r) x = -x;
            if (variant & 2) std::reverse(r.begin(), r.end());
            const int n = 2 * k;
            for (int keep : {1, 2, k / 2, k, n - 2, n - 1}) if (keep >= 1) run_case(std::string("musser variant ") + std::to_string(variant), r, keep, true);
        }
    }
    for (int n : {64, 1000, 4096, 30000})
        for (int keep : {n - 1, n / 2, 3 * n / 4}) {
            std::vector<float> r((size_t)n);
            retain_best_adversary(n, keep, r.data());
            run_case("adversary", r, keep, true);
        }
    const long family_cases = g_cases;
    for (int n : {1, 2, 3, 4, 5, 7, 64, 1023, 1024, 1025, 2049, 20000}) {                // all equal: every item stops both pointers
        const std::vector<float> r((size_t)n, 37.f);
        for (int keep : {0, 1, 2, 3, n / 4, n / 2, n - 3, n - 1, n, n + 1}) if (keep >= 0) run_case("all-equal", r, keep, false);
    }
    for (int n = 1; n <= 7; n++) {                                                       // every vector over {0, 1, 2}, every keep
        int total = 1;
        for (int i = 0; i < n; i++) total *= 3;
        for (int code = 0; code < total; code++) {
            std::vector<float> r((size_t)n);
            for (int i = 0, c = code; i < n; i++, c /= 3) r[(size_t)i] = (float)(c % 3);
            for (int keep = 0; keep <= n + 1; keep++) run_case("alphabet {0,1,2}", r, keep, false);
        }
    }
    printf("%ld cases (%ld in the families of retain_best_host), %ld mismatches, %ld cases reached the depth limit, %ld depth-limit disagreements\n",
           g_cases, family_cases, g_failed, g_heap_cases, g_heap_differs);
    if (g_failed || g_heap_differs) return 1;
    if (g_heap_cases == 0 || g_heap_cases == g_cases) { fprintf(stderr, "the depth limit must be reached by some cases and not by others\n"); return 2; }
    return 0;
}
