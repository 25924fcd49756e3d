// retain_best_std.cpp -- TEST INFRASTRUCTURE: KeyPointsFilter::retainBest as keypoint.cpp states it, on (response, index) items, with the
// REAL std::nth_element and std::partition of the libstdc++ this file is compiled against.  The product (csrc/uvo_retain_best.h) and
// the oracle (o_orb.c) both replay those two algorithms by hand; this file is what they are compared with, permutation by permutation.
//
//     if (n_points >= 0 && keypoints.size() > (size_t)n_points) {
//         if (n_points == 0) { keypoints.clear(); return; }
//         std::nth_element(keypoints.begin(), keypoints.begin() + n_points - 1, keypoints.end(), KeypointResponseGreater());
//         float ambiguous_response = keypoints[n_points - 1].response;
//         new_end = std::partition(keypoints.begin() + n_points, keypoints.end(), KeypointResponseGreaterThanOrEqualToThreshold(ambiguous_response));
//         keypoints.resize(new_end - keypoints.begin());
//     }
//
// Built as a shared object (loaded through ctypes) and included as text by retain_best_host.cpp.
#include <algorithm>
#include <vector>

namespace rbstd {
struct Item { float response; int index; };
struct ResponseGreater { bool operator()(const Item& a, const Item& b) const { return a.response > b.response; } };
struct ResponseAtLeast { float value; bool operator()(const Item& k) const { return k.response >= value; } };
}  // namespace rbstd

// responses[n] in their current order -> perm[new position] = old index; returns the new count
extern "C" int retain_best_std(const float* responses, int n, int n_points, int* perm)
{
    using namespace rbstd;
    if (!(n_points >= 0 && n > n_points)) { for (int i = 0; i < n; i++) perm[i] = i; return n; }
    if (n_points == 0) return 0;
    std::vector<Item> v((size_t)n);
    for (int i = 0; i < n; i++) { v[(size_t)i].response = responses[i]; v[(size_t)i].index = i; }
    std::nth_element(v.begin(), v.begin() + n_points - 1, v.end(), ResponseGreater());
    const float ambiguous = v[(size_t)n_points - 1].response;
    std::vector<Item>::const_iterator new_end = std::partition(v.begin() + n_points, v.end(), ResponseAtLeast{ambiguous});
    const int m = (int)(new_end - v.begin());
    for (int i = 0; i < m; i++) perm[i] = v[(size_t)i].index;
    return m;
}

// An input on which THIS library's std::nth_element degenerates (M. D. McIlroy, "A killer adversary for quicksort", 1999): the
// comparator decides the values while the algorithm runs -- every element is "gas" until a comparison of two gas elements freezes the
// current pivot candidate to the next small value -- so every partition strips a constant number of elements and introselect's depth
// limit is reached.  responses[i] = -value[i]: "response greater" on the result takes the decisions "value less" took.
namespace rbstd {
struct Adversary {
    std::vector<int> val; int nsolid, candidate, gas;
    bool less(int x, int y)
    {
        if (val[(size_t)x] == gas && val[(size_t)y] == gas) { if (x == candidate) val[(size_t)x] = nsolid++; else val[(size_t)y] = nsolid++; }
        if (val[(size_t)x] == gas) candidate = x; else if (val[(size_t)y] == gas) candidate = y;
        return val[(size_t)x] < val[(size_t)y];
    }
};
}  // namespace rbstd
extern "C" void retain_best_adversary(int n, int n_points, float* responses)
{
    using namespace rbstd;
    Adversary A; A.val.assign((size_t)n, n); A.nsolid = 0; A.candidate = 0; A.gas = n;
    std::vector<int> idx((size_t)n);
    for (int i = 0; i < n; i++) idx[(size_t)i] = i;
    if (n_points >= 1 && n > n_points) std::nth_element(idx.begin(), idx.begin() + n_points - 1, idx.end(), [&A](int a, int b) { return A.less(a, b); });
    for (int i = 0; i < n; i++) responses[i] = -(float)A.val[(size_t)i];      // (what stayed gas ties at -n: below every frozen value)
}
