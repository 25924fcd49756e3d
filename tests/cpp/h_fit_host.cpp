// h_fit_host.cpp -- TEST INFRASTRUCTURE, stand-alone (its own main; built plainly and with -fsanitize=address,undefined by
// tests/test_h_fit_host.py, with -ffp-contract=off as the library is).  The host policy of ergo_uvo_amd/csrc/uvo_h_fit.h -- findHomography's
// method-0 fit, in the summation order the header writes down -- on the cases of a file written by tests/h_fit_np.py:
//   int32 ncases, then per case: int32 n, int32 degenerate, float32 src[2n], float32 dst[2n].
// Each case's points are copied into vectors of exactly 2n floats, so a read past either end is a heap overflow the sanitizer build
// reports; every case must return (all loops are bounded: the test's time limit is the check); a case that is not marked degenerate
// must report ok = 1 and a finite H with H[8] = 1 (to rounding), a case that reports ok = 0 must leave H = 0.
// Output, one line per case for the Python side:  case <index> n <n> ok <0|1> H <nine %a doubles>
// Exit status 0: every case returned and met the above.
#include "../../ergo_uvo_amd/csrc/uvo_h_fit.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t ncases = 0;
    if (fread(&ncases, sizeof(ncases), 1, f) != 1 || ncases < 1 || ncases > 100000) { fprintf(stderr, "bad case count\n"); return 2; }
    int bad = 0;
    for (int c = 0; c < ncases; c++) {
        int32_t hdr[2];
        if (fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] < 1 || hdr[0] > (1 << 20)) { fprintf(stderr, "case %d: bad header\n", c); return 2; }
        const int n = hdr[0], degenerate = hdr[1];
        std::vector<float> src((size_t)2 * n), dst((size_t)2 * n);
        if (fread(src.data(), sizeof(float), src.size(), f) != src.size() || fread(dst.data(), sizeof(float), dst.size(), f) != dst.size()) { fprintf(stderr, "case %d: short read\n", c); return 2; }
        uvo::HFitWs ws;
        memset(&ws, 0xff, sizeof(ws));                       // the fit must not depend on what the workspace held
        uvo::HFitHost p;
        const int ok = uvo::hf_fit_all(p, src.data(), dst.data(), n, &ws);
        bool finite = true, zero = true;
        for (int k = 0; k < 9; k++) { if (!(fabs(ws.H[k]) <= DBL_MAX)) finite = false; if (ws.H[k] != 0) zero = false; }
        if (ok != 0 && ok != 1) { printf("FAIL case %d: status %d\n", c, ok); bad++; }
        if (!finite) { printf("FAIL case %d: H is not finite\n", c); bad++; }
        // H[8] is runKernel's h8 * (1 / h8), which the refinement leaves alone: 1 to a rounding or two
        if (!degenerate && !(ok == 1 && fabs(ws.H[8] - 1.0) <= 4 * DBL_EPSILON)) { printf("FAIL case %d: a non-degenerate case was not fitted (ok %d, H[8] %g)\n", c, ok, ws.H[8]); bad++; }
        if (!ok && !zero) { printf("FAIL case %d: ok = 0 but H is not zero\n", c); bad++; }
        if (ws.iter < 0 || ws.iter > uvo::kHfLmIters) { if (ok) { printf("FAIL case %d: %d LM iterations\n", c, ws.iter); bad++; } }
        printf("case %d n %d ok %d H", c, n, ok);
        for (int k = 0; k < 9; k++) printf(" %a", ws.H[k]);
        printf("\n");
    }
    fclose(f);
    printf("%d cases, %d failures\n", (int)ncases, bad);
    return bad ? 1 : 0;
}
