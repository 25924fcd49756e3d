// akaze_plan_host.cpp -- TEST INFRASTRUCTURE, stand-alone (its own main; built plainly and with -fsanitize=address,undefined by
// tests/test_akaze_plan_host.py, with -ffp-contract=off as the library is).  The level plan of ergo_uvo_amd/csrc/uvo_akaze_plan.h --
// what akaze.hip builds its workspaces, INTER_AREA tables and evolution graphs from -- for all 16 (n_octaves, n_octave_layers) pairs
// uvo_akaze_configure serves, at the image sizes given on the command line (w h pairs).  The table is a heap vector of exactly the
// kAkPlanMaxLevels levels a plan may hold, so a write past it is a heap overflow the sanitizer build reports.
// Output, for the Python side:
//   plan <w> <h> <n_octaves> <n_octave_layers> <levels>
//   level <i> <w> <h> <octave> <sublevel> <sigma_size> <border> <nsteps> <esigma %a> <etime %a> <tau[0 .. nsteps) %a>
//   guard <w> <h> <n_octaves> <n_octave_layers> <akaze_plan's result>      the refusals, asked of the header directly: 6 octaves of 2
//                                                                         sublevels (a FED cycle longer than a level holds), 5 x 4 (more levels than the table)
// Exit status 0: every served plan came back with 1..16 levels and cycles that fit, and both refusals were given.
#include "../../ergo_uvo_amd/csrc/uvo_akaze_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 1) % 2 != 0) { fprintf(stderr, "usage: %s w h [w h ...]\n", argv[0]); return 2; }
    int bad = 0;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int w = atoi(argv[a]), h = atoi(argv[a + 1]);
        if (w < 16 || h < 16) { fprintf(stderr, "size %d x %d\n", w, h); return 2; }
        for (int o = 1; o <= 4; o++)
            for (int l = 1; l <= 4; l++) {
                std::vector<uvo::AkLevel> L((size_t)uvo::kAkPlanMaxLevels);
                const int n = uvo::akaze_plan(w, h, o, l, L.data());
                printf("plan %d %d %d %d %d\n", w, h, o, l, n);
                if (n < 1 || n > uvo::kAkPlanMaxLevels) { printf("FAIL plan %d %d %d %d: %d levels\n", w, h, o, l, n); bad++; continue; }
                for (int i = 0; i < n; i++) {
                    const uvo::AkLevel& v = L[(size_t)i];
                    if (v.nsteps < 0 || v.nsteps > uvo::kAkPlanMaxSteps) { printf("FAIL level %d: %d steps\n", i, v.nsteps); bad++; continue; }
                    printf("level %d %d %d %d %d %d %d %d %a %a", i, v.w, v.h, v.octave, v.sublevel, v.sigma_size, v.border, v.nsteps, (double)v.esigma, (double)v.etime);
                    for (int k = 0; k < v.nsteps; k++) printf(" %a", (double)v.tau[k]);
                    printf("\n");
                }
            }
    }
    // the refusals: an image large enough for six octaves
    const int req[2][2] = { { 6, 2 }, { 5, 4 } }, want[2] = { uvo::AK_PLAN_CYCLE_TOO_LONG, uvo::AK_PLAN_TOO_MANY_LEVELS };
    for (int q = 0; q < 2; q++) {
        std::vector<uvo::AkLevel> L((size_t)uvo::kAkPlanMaxLevels);
        const int n = uvo::akaze_plan(4096, 2048, req[q][0], req[q][1], L.data());
        printf("guard 4096 2048 %d %d %d\n", req[q][0], req[q][1], n);
        if (n != want[q]) { printf("FAIL guard %d %d: %d\n", req[q][0], req[q][1], n); bad++; }
    }
    printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
