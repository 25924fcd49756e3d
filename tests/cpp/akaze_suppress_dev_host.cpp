// akaze_suppress_dev_host.cpp -- stand-alone (no HIP, no GPU): the workgroup form of AKAZE's duplicate suppression and refinement
// (ergo_uvo_amd/csrc/uvo_akaze_suppress_dev.h, the arithmetic and decisions of akaze.hip's k_ak_scan / k_ak_refine) against THE
// DEFINITION, the sequential host scans of ergo_uvo_amd/csrc/uvo_akaze_suppress.h, on candidate lists read from a file.
//
//   akaze_suppress_dev_host <cases.bin> <out.bin>
// cases.bin: int32 ncases, then per case: int32 nlev, nlev x { int32 w, h, sigma_size, octave; float32 octave_ratio, esigma },
//            int32 n, n x int32 level, n x int32 x, n x int32 y, n x 9 float32 v9.
// out.bin:   per case what the DEFINITION leaves: int32 n, n x 3 uint8 marks (the caller's order), int32 nk, nk x 28-byte keypoints,
//            3 x int32 the emulation's largest round count per phase.
// The kernels' workgroup is emulated with plain loops: T "threads" take the candidates of a scan strided, a round is the readiness pass
// over all threads, then the decision pass over all threads; the decision pass runs in ascending AND in descending thread order (two
// emulations: the result may not depend on which ready candidate goes first), with T = 1024 and T = 37.  Every loop carries the kernel's
// bound.  Exit status 1 on any difference in marks (three phases) or keypoints (bit for bit).
#include "../../ergo_uvo_amd/csrc/uvo_akaze_suppress.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace uvo;

struct Case { AksLevels L; std::vector<AkCand> list; };
struct Kp { float x, y, size, angle, response; int octave, class_id; };
static_assert(sizeof(Kp) == 28 && sizeof(AksKp) == 28, "keypoint layout");

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

// the device form on the ordered list; marks_dev: 3 planes of n bytes in list order
static void emulate(const AksLevels& L, const std::vector<AkCand>& sorted, const int* start, int T, bool descending, std::vector<uint8_t>* marks_dev, std::vector<AksKp>* kps, int* rounds_max)
{
    const int n = (int)sorted.size();
    std::vector<uint32_t> pos((size_t)n); std::vector<float> val((size_t)n);
    for (int q = 0; q < n; q++) { pos[(size_t)q] = aks_pos(sorted[(size_t)q].x, sorted[(size_t)q].y); val[(size_t)q] = sorted[(size_t)q].v[4]; }
    std::vector<uint8_t>& mark = *marks_dev;
    mark.assign((size_t)3 * n, 0xcc);                                  // (poison: every byte must be written by the workgroup that owns it)
    std::vector<uint8_t> state((size_t)n, 0xcc);
    for (int phase = 0; phase < 3; phase++) {
        rounds_max[phase] = 0;
        const uint8_t* mprev = mark.data() + (size_t)(phase ? phase - 1 : 0) * n;
        uint8_t* mt = mark.data() + (size_t)phase * n;
        for (int wg = 0; wg < L.n; wg++) {                                                                // the grid: independent workgroups
            int copy_level;
            const AksScan sc = aks_scan_of(phase, wg, L, &copy_level);
            if (copy_level >= 0) for (int tid = 0; tid < T; tid++) for (int q = start[copy_level] + tid; q < start[copy_level + 1]; q += T) mt[q] = mprev[q];
            if (sc.own < 0) continue;
            const int a = start[sc.own], b = start[sc.own + 1], ta = start[sc.tgt], tb = start[sc.tgt + 1];
            const int tw = L.lv[sc.tgt].w, th = L.lv[sc.tgt].h;
            int left = 0;
            for (int tid = 0; tid < T; tid++) {
                if (phase == 0) for (int q = a + tid; q < b; q += T) { mt[q] = 0; state[(size_t)q] = AKS_UNDECIDED; left++; }
                else {
                    for (int p = ta + tid; p < tb; p += T) mt[p] = mprev[p];
                    for (int q = a + tid; q < b; q += T) { const bool act = mprev[q] != 0; state[(size_t)q] = act ? AKS_UNDECIDED : AKS_DECIDED; left += act; }
                }
            }
            int rounds = 0;
            for (int it = 0; it < b - a; ++it) {
                if (left == 0) break;
                for (int tid = 0; tid < T; tid++)
                    for (int q = a + tid; q < b; q += T) if (state[(size_t)q] == AKS_UNDECIDED && aks_ready(pos.data(), state.data(), a, q, sc)) state[(size_t)q] = AKS_READY;
                int dec = 0;
                for (int k = 0; k < T; k++) {
                    const int tid = descending ? T - 1 - k : k;
                    for (int q = a + tid; q < b; q += T) if (state[(size_t)q] == AKS_READY) { aks_decide(phase, pos.data(), val.data(), mt, ta, tb, q, sc, tw, th); state[(size_t)q] = AKS_DECIDED; dec++; }
                }
                if (dec == 0) { fprintf(stderr, "a round decided nothing (phase %d, level %d)\n", phase, wg); exit(2); }
                left -= dec;
                rounds++;
            }
            if (left != 0) { fprintf(stderr, "a scan ended with %d undecided (phase %d, level %d)\n", left, phase, wg); exit(2); }
            if (rounds > rounds_max[phase]) rounds_max[phase] = rounds;
        }
    }
    kps->clear();
    const uint8_t* m3 = mark.data() + (size_t)2 * n;
    for (int q = 0; q < n; q++) { AksKp k; if (m3[q] != 0 && aks_refine(sorted[(size_t)q], L.lv[sorted[(size_t)q].pad], sorted[(size_t)q].pad, &k)) kps->push_back(k); }
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int ncases = 0;
    if (!read_exact(f, &ncases, 4) || ncases < 0) return 2;
    long n_total = 0, bad_marks = 0, bad_kps = 0, longest = 0, rejected = 0, kept = 0;
    for (int ci = 0; ci < ncases; ci++) {
        Case cs;
        int nlev = 0, n = 0;
        if (!read_exact(f, &nlev, 4) || nlev < 1 || nlev > kAksMaxLevels) return 2;
        cs.L.n = nlev;
        for (int l = 0; l < nlev; l++) {
            int iv[4]; float fv[2];
            if (!read_exact(f, iv, 16) || !read_exact(f, fv, 8)) return 2;
            cs.L.lv[l] = AksLevel{ iv[0], iv[1], iv[2], iv[3], fv[0], fv[1] };
        }
        if (!read_exact(f, &n, 4) || n < 0) return 2;
        std::vector<int> lv((size_t)n), x((size_t)n), y((size_t)n); std::vector<float> v9((size_t)9 * n);
        if (!read_exact(f, lv.data(), 4 * (size_t)n) || !read_exact(f, x.data(), 4 * (size_t)n) || !read_exact(f, y.data(), 4 * (size_t)n) || !read_exact(f, v9.data(), 36 * (size_t)n)) return 2;
        cs.list.resize((size_t)n);
        for (int q = 0; q < n; q++) {
            if (lv[(size_t)q] < 0 || lv[(size_t)q] >= nlev || x[(size_t)q] < 0 || y[(size_t)q] < 0 || x[(size_t)q] >= cs.L.lv[lv[(size_t)q]].w || y[(size_t)q] >= cs.L.lv[lv[(size_t)q]].h) return 2;
            AkCand& cd = cs.list[(size_t)q];
            cd.x = x[(size_t)q]; cd.y = y[(size_t)q]; cd.pad = lv[(size_t)q];
            for (int k = 0; k < 9; k++) cd.v[k] = v9[(size_t)9 * q + k];
        }
        // ---- the definition ----
        AksHost hs;
        aks_host_init(&hs, cs.L);
        std::vector<uint8_t> marks((size_t)3 * n + 1, 0);
        std::vector<Kp> def_kps;
        aks_host_order(&hs, cs.list.data(), n);
        aks_host_within(&hs);       aks_host_marks(&hs, cs.list.data(), n, marks.data(), 3);
        aks_host_sweep_lower(&hs);  aks_host_marks(&hs, cs.list.data(), n, marks.data() + 1, 3);
        aks_host_sweep_upper(&hs);  aks_host_marks(&hs, cs.list.data(), n, marks.data() + 2, 3);
        aks_host_refine(&hs, &def_kps);
        // ---- the ordered list the device form works on: the same keys ----
        std::vector<AkCand> sorted((size_t)n);
        std::vector<int> origin((size_t)n);
        int start[kAksMaxLevels + 1];
        for (int l = 0; l <= kAksMaxLevels; l++) start[l] = n;
        for (int q = n - 1; q >= 0; q--) {
            origin[(size_t)q] = (int)(hs.keys[(size_t)q] & 0x3fffffu);
            sorted[(size_t)q] = cs.list[(size_t)origin[(size_t)q]];
            for (int l = sorted[(size_t)q].pad; l >= 0 && start[l] > q; l--) start[l] = q;
        }
        int rounds[3] = {0, 0, 0};
        for (int variant = 0; variant < 4; variant++) {
            std::vector<uint8_t> dm; std::vector<AksKp> dk;
            int r[3];
            emulate(cs.L, sorted, start, variant < 2 ? 1024 : 37, (variant & 1) != 0, &dm, &dk, r);
            for (int p = 0; p < 3; p++) if (r[p] > rounds[p]) rounds[p] = r[p];
            long bm = 0;
            for (int q = 0; q < n; q++) for (int p = 0; p < 3; p++) bm += dm[(size_t)p * n + q] != marks[(size_t)3 * origin[(size_t)q] + p];
            bool same = dk.size() == def_kps.size();
            for (size_t k = 0; same && k < dk.size(); k++) same = memcmp(&dk[k], &def_kps[k], 28) == 0;
            if (bm || !same) fprintf(stderr, "case %d, variant %d: %ld marks differ, keypoints %s (%zu against %zu)\n", ci, variant, bm, same ? "equal" : "DIFFER", dk.size(), def_kps.size());
            bad_marks += bm; bad_kps += !same;
        }
        for (int p = 0; p < 3; p++) if (rounds[p] > longest) longest = rounds[p];
        long m3 = 0;
        for (int q = 0; q < n; q++) m3 += marks[(size_t)3 * q + 2];
        kept += (long)def_kps.size(); rejected += m3 - (long)def_kps.size();
        const int nk = (int)def_kps.size();
        fwrite(&n, 4, 1, g); if (n) fwrite(marks.data(), 1, (size_t)3 * n, g);
        fwrite(&nk, 4, 1, g); if (nk) fwrite(def_kps.data(), 28, (size_t)nk, g);
        fwrite(rounds, 4, 3, g);
        n_total += n;
    }
    fclose(f);
    if (fclose(g) != 0) return 2;
    printf("%d cases, %ld candidates, %ld keypoints kept, %ld rejected by the refinement, %ld mark mismatches, %ld keypoint mismatches, longest scan %ld rounds\n",
           ncases, n_total, kept, rejected, bad_marks, bad_kps, longest);
    return bad_marks || bad_kps ? 1 : 0;
}
