// uvo_retain_best_dev.h -- host AND device (no HIP include): the arithmetic of k_rb_rank (orb.hip), the workgroup form of
// uvo_retain_best.h's replay of KeyPointsFilter::retainBest's order, so that tests/cpp/retain_best_dev_host.cpp can run it on a CPU
// against the real std::nth_element + std::partition before any GPU does.
//
// One pass of libstdc++'s unguarded Hoare partition over v[lo, hi) against a pivot, without walking it:
//   left stoppers  a_0 < a_1 < ...   the positions whose item is NOT greater than the pivot (where `first` stops),
//   right stoppers b_0 > b_1 > ...   the positions whose item is NOT smaller than the pivot (where `last` stops), counted from the right.
//   Swap k exchanges a_k and b_k and happens iff a_k < b_k: before it, everything strictly between a_(k-1) and b_(k-1) is untouched, so
//   `first` stops at min(a_k, b_(k-1)) (position b_(k-1) now holds a_(k-1)'s item, a left stopper) and `last` at max(b_k, a_(k-1)).
//   a ascends and b descends, so the swaps are a prefix k < K and K = the number of k with a_k < b_k; no position is in two swaps
//   (a_k = b_j swapped both ways would need j < k and k < j).  The loop returns `first` = min(a_K, b_(K-1)), with b_(-1) = hi and
//   a_K = +inf when there is no such stopper.
// std::partition's bidirectional loop over the tail is the same shape with disjoint stopper sets (left: r < boundary, right:
// r >= boundary); only the swaps matter there, the returned point is lo + the number of right stoppers.
// The workgroup is kRbdWaves waves of 64 lanes; wave w owns the positions [lo + w * chunk, lo + (w + 1) * chunk) and writes its stoppers,
// ascending, into that same range of two position lists; a 17-entry prefix of the waves' counts finds the k-th of all.
#pragma once
#if defined(__HIPCC__)
#define RBD_HD __host__ __device__ inline
#else
#define RBD_HD inline
#endif

namespace uvo {

struct RbdItem { float r; int i; };
static const int kRbdWaves = 16, kRbdLanes = 64, kRbdThreads = kRbdWaves * kRbdLanes;     // kRbdThreads = the items of one round of a pass

RBD_HD bool rbd_gt(float a, float b) { return a > b; }
// MODE 0: Hoare against the pivot value p; MODE 1: the tail partition against the boundary value p
template <int MODE> RBD_HD bool rbd_left_stop(float x, float p) { return MODE == 0 ? !rbd_gt(x, p) : !(x >= p); }
template <int MODE> RBD_HD bool rbd_right_stop(float x, float p) { return MODE == 0 ? !rbd_gt(p, x) : x >= p; }

RBD_HD int rbd_depth(int n) { int depth = 0; for (; n > 1; n >>= 1) depth += 2; return depth; }          // 2 * floor(log2 n)
// __move_median_to_first(result, a, b, c): which of a, b, c (0, 1, 2) is exchanged with *result
RBD_HD int rbd_median_pick(float a, float b, float c)
{
    if (rbd_gt(a, b)) return rbd_gt(b, c) ? 1 : rbd_gt(a, c) ? 2 : 0;
    return rbd_gt(a, c) ? 0 : rbd_gt(b, c) ? 2 : 1;
}
RBD_HD int rbd_chunk(int m) { return (m + kRbdThreads - 1) / kRbdThreads * kRbdLanes; }                   // positions per wave, a multiple of 64
// where the k-th stopper (ascending, k < pref[kRbdWaves]) sits in the position list: pref = exclusive prefix of the waves' counts
RBD_HD int rbd_list_at(int lo, int chunk, const int* pref, int k)
{
    int w = 0;
    while (w + 1 < kRbdWaves && k >= pref[w + 1]) w++;
    return lo + w * chunk + (k - pref[w]);
}
// the value __unguarded_partition returns after K swaps: a_K (or none) and b_(K-1) (or hi)
RBD_HD int rbd_cut(bool has_a, int a_K, bool has_b, int b_Km1, int hi)
{
    const int b = has_b ? b_Km1 : hi;
    return has_a && a_K < b ? a_K : b;
}
RBD_HD bool rbd_take_right(int cut, int nth) { return cut <= nth; }                                      // first = cut; otherwise last = cut

// ---- the sequential ends, one lane: the insertion sort of at most three items and introselect's heap select ----
RBD_HD void rbd_swap(RbdItem* a, RbdItem* b) { const RbdItem t = *a; *a = *b; *b = t; }
RBD_HD void rbd_insertion(RbdItem* first, RbdItem* last)
{
    for (RbdItem* i = first + 1; i < last; ++i) {
        const RbdItem v = *i;
        if (rbd_gt(v.r, first->r)) { for (RbdItem* q = i; q > first; --q) *q = *(q - 1); *first = v; }
        else { RbdItem* q = i; while (rbd_gt(v.r, (q - 1)->r)) { *q = *(q - 1); --q; } *q = v; }
    }
}
RBD_HD void rbd_sift(RbdItem* first, long hole, long len, RbdItem value)                                 // __adjust_heap + __push_heap
{
    const long top = hole;
    long child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (rbd_gt(first[child].r, first[child - 1].r)) child--;
        first[hole] = first[child]; hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) { child = 2 * (child + 1); first[hole] = first[child - 1]; hole = child - 1; }
    long parent = (hole - 1) / 2;
    while (hole > top && rbd_gt(first[parent].r, value.r)) { first[hole] = first[parent]; hole = parent; parent = (hole - 1) / 2; }
    first[hole] = value;
}
RBD_HD void rbd_heap_select(RbdItem* first, RbdItem* middle, RbdItem* last)
{
    const long len = (long)(middle - first);
    if (len >= 2) for (long parent = (len - 2) / 2;; parent--) { rbd_sift(first, parent, len, first[parent]); if (parent == 0) break; }
    for (RbdItem* i = middle; i < last; ++i)
        if (rbd_gt(i->r, first->r)) { const RbdItem v = *i; *i = *first; rbd_sift(first, 0, len, v); }
}

}  // namespace uvo
