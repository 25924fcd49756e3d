// h_vote_host.cpp -- TEST INFRASTRUCTURE, stand-alone (its own main; built plainly and with -fsanitize=address,undefined by
// tests/test_mono_h_vote_host.py).  The vote of recover_pose_homography among decomposeHomographyMat's candidates
// (ergo_uvo_amd/csrc/uvo_h_vote.h: the type-punned pair count of VO_utility.cpp:601-602 and the first-strictly-greater choice), run on a
// CPU over rows the Python side wrote, so that numpy can state the expected result independently.
//
// Input (argv[1], text): per case one line  "<ncand> <n> <distance as 16 hex digits of the double>"  followed by ncand * n words of 8 hex
// digits, the float rows bit for bit.  Output: per case  "<count 0> ... <count ncand-1> <choice>".  Each row is copied into a vector of
// exactly n floats, so a read past a row is a heap overflow the sanitizer reports.
#include "../../ergo_uvo_amd/csrc/uvo_h_vote.h"

#include <stdio.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: h_vote_host <cases.txt>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int ncand = 0, n = 0, cases = 0;
    unsigned long long dbits = 0;
    while (fscanf(f, "%d %d %llx", &ncand, &n, &dbits) == 3) {
        if (ncand < 0 || ncand > uvo::kHVoteMaxCands || n < 0) { fprintf(stderr, "bad case header\n"); fclose(f); return 2; }
        double distance;
        const uint64_t db = (uint64_t)dbits;
        memcpy(&distance, &db, 8);
        int counts[uvo::kHVoteMaxCands] = {0, 0, 0, 0};
        for (int c = 0; c < ncand; c++) {
            std::vector<float> row((size_t)n);
            for (int j = 0; j < n; j++) {
                unsigned w = 0;
                if (fscanf(f, "%x", &w) != 1) { fprintf(stderr, "short row\n"); fclose(f); return 2; }
                const uint32_t w32 = (uint32_t)w;
                memcpy(&row[(size_t)j], &w32, 4);
            }
            counts[c] = uvo::hv_row_count(row.data(), n, distance);
            // pair by pair as the kernel's threads take them: the same sum
            int again = 0;
            for (int j = 0; j + 1 < n; j++) again += uvo::hv_pair_good(row[(size_t)j], row[(size_t)j + 1], distance) ? 1 : 0;
            if (again != counts[c]) { fprintf(stderr, "row count and pair sum differ\n"); fclose(f); return 1; }
            printf("%d ", counts[c]);
        }
        printf("%d\n", uvo::hv_choose(counts, ncand));
        cases++;
    }
    fclose(f);
    fprintf(stderr, "%d cases\n", cases);
    return cases > 0 ? 0 : 2;
}
