// uvo_h_vote.h -- host AND device (no HIP include): the two decisions of recover_pose_homography's vote among the candidates of
// decomposeHomographyMat (VO_utility.cpp:581-624), shared by the host-pointer operator, the device-resident chain's pick kernel
// (mono.hip: k_h_pick) and tests/cpp/h_vote_host.cpp, which runs them on a CPU before any GPU does.
//
//   the count      VO_utility.cpp:601-602 reads a row of FLOAT z values through a double pointer: entry j of the reference's loop is the
//                  double whose low word is z[j] and whose high word is z[j + 1] (little endian), counted when it lies in
//                  (0, HOMOGRAPHY_DISTANCE).  The last column, read past the row there, is not counted: pairs j, j + 1 < n only.
//   the choice     the first candidate whose count is strictly greater than a running maximum that starts at 0; -1 when every count is 0
//                  (the reference then leaves R and t unwritten).
// memcpy punning only: no aliasing casts, nothing a sanitizer objects to.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define HV_HD __host__ __device__ inline
#else
#define HV_HD inline
#endif

namespace uvo {

static const int kHVoteMaxCands = 4;          // decomposeHomographyMat returns one or four solutions

// the double the reference reads at column j: low word z[j], high word z[j + 1]
HV_HD double hv_pair_value(float z_lo, float z_hi)
{
    uint32_t lo, hi;
    memcpy(&lo, &z_lo, 4); memcpy(&hi, &z_hi, 4);
    const uint64_t bits = ((uint64_t)hi << 32) | (uint64_t)lo;
    double v;
    memcpy(&v, &bits, 8);
    return v;
}
HV_HD bool hv_pair_good(float z_lo, float z_hi, double distance)
{
    const double v = hv_pair_value(z_lo, z_hi);
    return v > 0 && v < distance;              // NaN fails both
}
// the count of one row, sequentially (the kernel strides the same pairs over its threads and adds)
HV_HD int hv_row_count(const float* z, int n, double distance)
{
    int good = 0;
    for (int j = 0; j + 1 < n; j++) good += hv_pair_good(z[j], z[j + 1], distance) ? 1 : 0;
    return good;
}
// -1: no candidate counted anything
HV_HD int hv_choose(const int* counts, int ncand)
{
    int best = -1, max_good = 0;
    for (int i = 0; i < ncand; i++) if (counts[i] > max_good) { best = i; max_good = counts[i]; }
    return best;
}

}  // namespace uvo
