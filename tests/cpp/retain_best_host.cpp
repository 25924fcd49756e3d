// retain_best_host.cpp -- TEST INFRASTRUCTURE, stand-alone (its own main; built plainly and with -fsanitize=address,undefined by
// tests/test_retain_best_host.py).  The product's replay of KeyPointsFilter::retainBest's order (ergo_uvo_amd/csrc/uvo_retain_best.h:
// hand-copied introselect, heap select, insertion sort and bidirectional partition) against the real std::nth_element /
// std::partition (retain_best_std.cpp), element by element, over
//   * the grid: sizes 1 .. 60000, 2 .. 100000 distinct values, random / ascending / descending / organ-pipe order, keep 1 .. n + 1;
//   * integer FAST scores: 246 distinct values (9 .. 254) with a geometric distribution, i.e. heavy ties at the low end;
//   * median-of-three killer sequences (D. R. Musser, "Introspective sorting and selection algorithms", 1997), as written, negated,
//     reversed, at several sizes, and an adversary sequence drawn against this library's own std::nth_element.
// UVO_RB_TRACE makes the header count the calls of rb_heap_select: the program FAILS unless some case reached introselect's depth
// limit, and prints which did.  Exit status 0: every permutation equal and the heap fallback proven to have run.
#define UVO_RB_TRACE
#include "../../ergo_uvo_amd/csrc/uvo_retain_best.h"
#include "retain_best_std.cpp"

#include <stdint.h>
#include <stdio.h>
#include <string>

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

long g_cases = 0, g_failed = 0, g_heap_cases = 0;

void run_case(const std::string& name, const std::vector<float>& r, int keep, bool report_heap)
{
    const int n = (int)r.size();
    std::vector<int> want((size_t)n + 1), got;
    const int m = retain_best_std(r.data(), n, keep, want.data());
    std::vector<uvo::RbItem> tmp;
    const long before = uvo::rb_heap_select_calls;
    uvo::retain_best_order(r.data(), n, keep, 0, &tmp, &got);
    const long heap = uvo::rb_heap_select_calls - before;
    g_cases++;
    bool ok = (int)got.size() == m;
    int at = -1;
    for (int i = 0; ok && i < m; i++) if (got[(size_t)i] != want[(size_t)i]) { ok = false; at = i; }
    if (!ok) {
        g_failed++;
        if (g_failed <= 10) fprintf(stderr, "MISMATCH %s n=%d keep=%d: std keeps %d, replay %d, first difference at %d\n", name.c_str(), n, keep, m, (int)got.size(), at);
    }
    if (heap > 0) { g_heap_cases++; if (report_heap) printf("heap fallback reached: %s n=%d keep=%d (%ld calls)\n", name.c_str(), n, keep, heap); }
}

void order(std::vector<float>* v, int kind)
{
    const size_t n = v->size();
    if (kind == 0) return;                                                            // random: as drawn
    std::sort(v->begin(), v->end());                                                  // 1: ascending
    if (kind == 2) std::reverse(v->begin(), v->end());                                // 2: descending
    if (kind == 3) {                                                                  // 3: organ pipe: up, then down
        std::vector<float> o(n);
        size_t a = 0, b = n;
        for (size_t i = 0; i < n; i++) { if (i & 1) o[--b] = (*v)[i]; else o[a++] = (*v)[i]; }
        *v = o;
    }
}

std::vector<float> musser(int k)                                                     // 2k elements: 1, k+1, 3, k+3, ..., 2k-1 | 2, 4, ..., 2k
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
    for (int n : {50, 700, 5000, 40000})                                              // FAST scores: integers 9 .. 254, most of them low
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
    printf("%ld cases, %ld mismatches, %ld cases reached rb_heap_select (%ld calls)\n", g_cases, g_failed, g_heap_cases, uvo::rb_heap_select_calls);
    if (g_failed) return 1;
    if (g_heap_cases == 0) { fprintf(stderr, "no case reached introselect's depth limit: rb_heap_select never ran\n"); return 2; }
    return 0;
}
