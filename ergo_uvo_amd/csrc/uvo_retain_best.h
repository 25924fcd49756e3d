// uvo_retain_best.h -- host only (no HIP include): the order KeyPointsFilter::retainBest leaves, for orb.hip and for the host test
// tests/cpp/retain_best_host.cpp, which compares it with the real std::nth_element / std::partition element by element.
// KeyPointsFilter::retainBest's order: std::nth_element(first, first + n - 1, last, response greater) followed by
// std::partition(first + n, last, response >= boundary) as libstdc++ implements them (introselect: median of three to the front,
// unguarded Hoare partition, heap select after 2 log2(n) bad splits, insertion sort of the last three; the bidirectional partition).
#pragma once
#include <stddef.h>
#include <utility>
#include <vector>

namespace uvo {
namespace {
struct RbItem { float r; int i; };
inline bool rb_gt(const RbItem& a, const RbItem& b) { return a.r > b.r; }
void rb_median_to_first(RbItem* res, RbItem* a, RbItem* b, RbItem* c)
{
    if (rb_gt(*a, *b)) { if (rb_gt(*b, *c)) std::swap(*res, *b); else if (rb_gt(*a, *c)) std::swap(*res, *c); else std::swap(*res, *a); }
    else if (rb_gt(*a, *c)) std::swap(*res, *a);
    else if (rb_gt(*b, *c)) std::swap(*res, *c);
    else std::swap(*res, *b);
}
RbItem* rb_hoare(RbItem* first, RbItem* last, const RbItem* pivot)
{
    for (;;) {
        while (rb_gt(*first, *pivot)) ++first;
        --last;
        while (rb_gt(*pivot, *last)) --last;
        if (!(first < last)) return first;
        std::swap(*first, *last);
        ++first;
    }
}
void rb_sift(RbItem* first, ptrdiff_t hole, ptrdiff_t len, RbItem value)      // __adjust_heap + __push_heap
{
    const ptrdiff_t top = hole;
    ptrdiff_t child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (rb_gt(first[child], first[child - 1])) child--;
        first[hole] = first[child]; hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) { child = 2 * (child + 1); first[hole] = first[child - 1]; hole = child - 1; }
    ptrdiff_t parent = (hole - 1) / 2;
    while (hole > top && rb_gt(first[parent], value)) { first[hole] = first[parent]; hole = parent; parent = (hole - 1) / 2; }
    first[hole] = value;
}
#ifdef UVO_RB_TRACE
long rb_heap_select_calls = 0;                                   // tests/cpp/retain_best_host.cpp: proof that the depth limit was reached; orb.hip: uvo_retain_best's depth_limit_hits
#endif
void rb_heap_select(RbItem* first, RbItem* middle, RbItem* last)
{
#ifdef UVO_RB_TRACE
    ++rb_heap_select_calls;
#endif
    const ptrdiff_t len = middle - first;
    if (len >= 2) for (ptrdiff_t parent = (len - 2) / 2;; parent--) { rb_sift(first, parent, len, first[parent]); if (parent == 0) break; }
    for (RbItem* i = middle; i < last; ++i)
        if (rb_gt(*i, *first)) { const RbItem v = *i; *i = *first; rb_sift(first, 0, len, v); }
}
void rb_nth(RbItem* first, RbItem* nth, RbItem* last)
{
    if (first == last || nth == last) return;
    int depth = 0;
    for (ptrdiff_t n = last - first; n > 1; n >>= 1) depth += 2;
    while (last - first > 3) {
        if (depth == 0) { rb_heap_select(first, nth + 1, last); std::swap(*first, *nth); return; }
        --depth;
        rb_median_to_first(first, first + 1, first + (last - first) / 2, last - 1);
        RbItem* cut = rb_hoare(first + 1, last, first);
        if (cut <= nth) first = cut; else last = cut;
    }
    for (RbItem* i = first + 1; i < last; ++i) {                    // __insertion_sort
        const RbItem v = *i;
        if (rb_gt(v, *first)) { for (RbItem* q = i; q > first; --q) *q = *(q - 1); *first = v; }
        else { RbItem* q = i; while (rb_gt(v, *(q - 1))) { *q = *(q - 1); --q; } *q = v; }
    }
}
// responses r[0 .. n) -> the surviving old indices in retainBest's order, appended to `out` with `base` added
void retain_best_order(const float* r, int n, int n_points, int base, std::vector<RbItem>* tmp, std::vector<int>* out)
{
    if (!(n_points >= 0 && n > n_points)) { for (int i = 0; i < n; i++) out->push_back(base + i); return; }
    if (n_points == 0) return;
    tmp->resize(n);
    RbItem* v = tmp->data();
    for (int i = 0; i < n; i++) { v[i].r = r[i]; v[i].i = i; }
    rb_nth(v, v + n_points - 1, v + n);
    const float amb = v[n_points - 1].r;
    RbItem *first = v + n_points, *last = v + n;
    for (;;) {
        while (first != last && first->r >= amb) ++first;
        if (first == last) break;
        --last;
        while (first != last && !(last->r >= amb)) --last;
        if (first == last) break;
        std::swap(*first, *last);
        ++first;
    }
    for (RbItem* q = v; q < first; ++q) out->push_back(base + q->i);
}
}  // namespace
}  // namespace uvo
