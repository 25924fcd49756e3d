// uvo_h_fit.h -- host AND device: cv::findHomography with method 0 ("regular method using all the points") on n > 4 pairs: the
// normalised DLT over ALL points (HomographyEstimatorCallback::runKernel), then LMSolver's ten Levenberg-Marquardt iterations on the
// reprojection residuals of ALL points (HomographyRefineCallback).  The arithmetic is written once, over a policy, as Epnp<Policy> is:
// k_h_fit_all (mono.hip) runs it with HFitDev, one workgroup of 256 threads; the host route of mono_find_homography and
// tests/cpp/h_fit_host.cpp run it with HFitHost, a plain loop -- and the two give the same bits, because
//
// THE SUMMATION ORDER IS PART OF THE DEFINITION.  Every sum over the points (the 4 + 4 normalisation statistics, LtL's 45 sums, and
// per LM evaluation JtJ's 36, Jte's 8 and |e|^2) is taken as
//   1. lane l of 256 adds the terms of the points l, l + 256, l + 512, ... in that order, in double, starting from +0;
//   2. inside each group of 64 consecutive lanes (a wave), for s = 32, 16, 8, 4, 2, 1: lane j += lane j + s  (j < s);
//   3. the four group totals t0 .. t3 are combined as (t0 + t1) + (t2 + t3).
// The maximum of |e| over the points (LMSolver's second stopping test) takes the same route with "a < b ? b : a", which ignores NaN.
// A term is one expression per point and sum (HfCentroid / HfSpread / HfLtL / HfJtJ / HfErr below); nothing is contracted to FMA:
// the library and the test program are both built with -ffp-contract=off.
//
// What is NOT this header: the refit of methods 4 and 8 (mono.hip: h_compact_refit), whose sums run sequentially over the inliers in
// the CPU restatement's order.  Method 0 has no such twin; its last bits are this header's, not OpenCV's.
// What OpenCV does, as recalled from 4.5's fundam.cpp (medium confidence; the recall lives here and nowhere else): with method == 0
// the mask is all ones and runKernel runs on all points (no sampling, no checkSubset); when it succeeds and npoints > 4, runKernel runs
// again on the mask-compacted points -- the same points -- and LMSolver::create(HomographyRefineCallback, 10)->run(H8) refines the
// first eight entries with H[8] = 1.  The scalar tail of runKernel is homography_tail (uvo_mono.h); the LM state machine and its
// eigen-decomposition solves are lm_refine_homography's (mono.hip), statement for statement, with the sums replaced as above.
// One departure, named: a fit whose H is not finite reports status 0 and H = 0 (OpenCV would hand the non-finite matrix on); NaN
// payloads differ between processors, a status does not.
// Every loop is bounded: 3 + 1 + at most 10 * 2 reductions, Jacobi sweeps by jacobi_eigen's own limit (n * n * 30).
#pragma once
#include "uvo_mono.h"

namespace uvo {

static const int kHfLanes = 256, kHfWave = 64, kHfWaves = kHfLanes / kHfWave;
static const int kHfMaxSums = 45;                       // the widest reduction; slot [K] of a K-sum reduction carries the maximum
static const int kHfLmIters = 10;                       // LMSolver::create(cb, 10)

// the fit's state: one per workgroup in LDS, one on the stack of a host call
struct HFitWs {
    double sums[kHfMaxSums + 1];                        // the last reduction's result
    double part[kHfWaves][kHfMaxSums + 1];              // step 2's group totals
    double st[8];                                       // cMx cMy cmx cmy, then sMx sMy smx smy
    double LtL[81], W[9], V[81];
    double H[9];
    double x[8], xd[8], d[8], v[8], D[8], A[64], Ap[64];
    double ea[64], ew[8], ev[64];                       // the 8 x 8 eigen-solves' scratch
    double S, lambda, lc, rmax;
    int ind[18];
    int iter, ok, improved, proceed;
};

// ---- the per-point terms ----
struct HfCentroid {
    const float *M, *m;
    __host__ __device__ void operator()(int i, double* v) const { v[0] = M[2*i]; v[1] = M[2*i+1]; v[2] = m[2*i]; v[3] = m[2*i+1]; v[4] = 0; }
};
struct HfSpread {
    const float *M, *m; double cMx, cMy, cmx, cmy;
    __host__ __device__ void operator()(int i, double* v) const
    {
        v[0] = fabs(M[2*i] - cMx); v[1] = fabs(M[2*i+1] - cMy); v[2] = fabs(m[2*i] - cmx); v[3] = fabs(m[2*i+1] - cmy); v[4] = 0;
    }
};
// LtL's upper triangle, row by row: (j, k >= j) at j * 9 - j * (j - 1) / 2 + (k - j)
struct HfLtL {
    const float *M, *m; double cMx, cMy, cmx, cmy, sMx, sMy, smx, smy;
    __host__ __device__ void operator()(int i, double* v) const
    {
        const double x = (m[2*i] - cmx)*smx, y = (m[2*i+1] - cmy)*smy;
        const double X = (M[2*i] - cMx)*sMx, Y = (M[2*i+1] - cMy)*sMy;
        const double Lx[9] = { X, Y, 1, 0, 0, 0, -x*X, -x*Y, -x };
        const double Ly[9] = { 0, 0, 0, X, Y, 1, -y*X, -y*Y, -y };
        int o = 0;
#pragma unroll
        for (int j = 0; j < 9; j++)
#pragma unroll
            for (int k = j; k < 9; k++) v[o++] = Lx[j]*Lx[k] + Ly[j]*Ly[k];
        v[45] = 0;
    }
};
// HomographyRefineCallback::compute for one pair: the residual e = (xi - mx, yi - my) and its two Jacobian rows
__host__ __device__ __forceinline__ void hf_project(const float* M, const float* m, int i, const double* h, double* ex, double* ey, double* Jx, double* Jy)
{
    const double Mx = M[2*i], My = M[2*i+1];
    double ww = h[6]*Mx + h[7]*My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1./ww : 0;
    const double xi = (h[0]*Mx + h[1]*My + h[2])*ww;
    const double yi = (h[3]*Mx + h[4]*My + h[5])*ww;
    *ex = xi - m[2*i];
    *ey = yi - m[2*i+1];
    if (Jx) {
        Jx[0] = Mx*ww; Jx[1] = My*ww; Jx[2] = ww; Jx[3] = Jx[4] = Jx[5] = 0.; Jx[6] = -Mx*ww*xi; Jx[7] = -My*ww*xi;
        Jy[0] = Jy[1] = Jy[2] = 0.; Jy[3] = Mx*ww; Jy[4] = My*ww; Jy[5] = ww; Jy[6] = -Mx*ww*yi; Jy[7] = -My*ww*yi;
    }
}
__host__ __device__ __forceinline__ double hf_absmax(double a, double b) { a = fabs(a); b = fabs(b); return a < b ? b : a; }
// |e|^2 at h, and max |e|
struct HfErr {
    const float *M, *m; double h[8];
    __host__ __device__ void operator()(int i, double* v) const
    {
        double ex, ey;
        hf_project(M, m, i, h, &ex, &ey, nullptr, nullptr);
        v[0] = ex*ex + ey*ey; v[1] = hf_absmax(ex, ey);
    }
};
// JtJ's upper triangle (36, row by row as LtL's), Jte (8), |e|^2, and max |e|
struct HfJtJ {
    const float *M, *m; double h[8];
    __host__ __device__ void operator()(int i, double* v) const
    {
        double ex, ey, Jx[8], Jy[8];
        hf_project(M, m, i, h, &ex, &ey, Jx, Jy);
        int o = 0;
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = a; b < 8; b++) v[o++] = Jx[a]*Jx[b] + Jy[a]*Jy[b];
#pragma unroll
        for (int a = 0; a < 8; a++) v[36 + a] = Jx[a]*ex + Jy[a]*ey;
        v[44] = ex*ex + ey*ey; v[45] = hf_absmax(ex, ey);
    }
};

// ---- the host policy: the three steps of the order above, in plain loops ----
struct HFitHost {
    template <int K, class F> void reduce(int n, const F& f, HFitWs* ws)
    {
        double acc[kHfWave][K + 1], v[K + 1];
        for (int w = 0; w < kHfWaves; w++) {
            for (int l = 0; l < kHfWave; l++) {
                for (int k = 0; k <= K; k++) acc[l][k] = 0;
                for (int i = w * kHfWave + l; i < n; i += kHfLanes) {
                    f(i, v);
                    for (int k = 0; k < K; k++) acc[l][k] += v[k];
                    if (acc[l][K] < v[K]) acc[l][K] = v[K];
                }
            }
            for (int s = kHfWave / 2; s > 0; s >>= 1)
                for (int l = 0; l < s; l++) {
                    for (int k = 0; k < K; k++) acc[l][k] += acc[l + s][k];
                    if (acc[l][K] < acc[l + s][K]) acc[l][K] = acc[l + s][K];
                }
            for (int k = 0; k <= K; k++) ws->part[w][k] = acc[0][k];
        }
        for (int k = 0; k < K; k++) ws->sums[k] = (ws->part[0][k] + ws->part[1][k]) + (ws->part[2][k] + ws->part[3][k]);
        const double a = ws->part[0][K] < ws->part[1][K] ? ws->part[1][K] : ws->part[0][K];
        const double b = ws->part[2][K] < ws->part[3][K] ? ws->part[3][K] : ws->part[2][K];
        ws->sums[K] = a < b ? b : a;
    }
    template <class F> void one(const F& f) { f(); }
};

#if defined(__HIPCC__)
// ---- the device policy: one workgroup of kHfLanes threads, ws in LDS; wave shuffles for step 2, 4 x (K + 1) doubles of LDS for step 3.
// reduce() and one() end in a workgroup barrier, so what they wrote into ws is every thread's to read, and every branch taken on it is uniform.
struct HFitDev {
    int tid;
    template <int K, class F> __device__ void reduce(int n, const F& f, HFitWs* ws)
    {
        double acc[K + 1], v[K + 1];
#pragma unroll
        for (int k = 0; k <= K; k++) acc[k] = 0;
        for (int i = tid; i < n; i += kHfLanes) {
            f(i, v);
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] += v[k];
            if (acc[K] < v[K]) acc[K] = v[K];
        }
#pragma unroll
        for (int s = kHfWave / 2; s > 0; s >>= 1) {
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] += __shfl_down(acc[k], s, kHfWave);
            const double o = __shfl_down(acc[K], s, kHfWave);
            if (acc[K] < o) acc[K] = o;
        }
        if ((tid & (kHfWave - 1)) == 0) {
#pragma unroll
            for (int k = 0; k <= K; k++) ws->part[tid / kHfWave][k] = acc[k];
        }
        __syncthreads();
        if (tid < K) ws->sums[tid] = (ws->part[0][tid] + ws->part[1][tid]) + (ws->part[2][tid] + ws->part[3][tid]);
        else if (tid == K) {
            const double a = ws->part[0][K] < ws->part[1][K] ? ws->part[1][K] : ws->part[0][K];
            const double b = ws->part[2][K] < ws->part[3][K] ? ws->part[3][K] : ws->part[2][K];
            ws->sums[K] = a < b ? b : a;
        }
        __syncthreads();
    }
    template <class F> __device__ void one(const F& f) { if (tid == 0) f(); __syncthreads(); }
};
#endif

// ---- the scalar pieces of LMSolver (levmarq.cpp), as mono.hip's solve_eig8 / invert_eig8 state them, on the workspace's scratch ----
__host__ __device__ inline void hf_eig8(HFitWs* ws, const double* A)
{
    for (int i = 0; i < 64; i++) ws->ea[i] = A[i];
    jacobi_eigen(SArr<1>{ws->ea}, 8, SArr<1>{ws->ew}, SArr<1>{ws->ev}, ws->ind, ws->ind + 8);
}
__host__ __device__ inline void hf_solve_eig8(HFitWs* ws, const double* A, const double* b, double* x)
{
    hf_eig8(ws, A);
    const double *w = ws->ew, *v = ws->ev;
    double threshold = 0;
    for (int i = 0; i < 8; i++) { x[i] = 0; threshold += w[i]; }
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < 8; i++) {
        double wi = w[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1/wi;
        double s = 0;
        for (int j = 0; j < 8; j++) s += v[i*8 + j]*b[j];
        s *= wi;
        for (int j = 0; j < 8; j++) x[j] = x[j] + s*v[i*8 + j];
    }
}
// the largest |diagonal entry| of A's pseudo-inverse, floored at DBL_EPSILON (all LMSolver takes from the inverse)
__host__ __device__ inline double hf_inverse_maxdiag(HFitWs* ws, const double* A)
{
    hf_eig8(ws, A);
    const double *w = ws->ew, *v = ws->ev;
    double threshold = 0, diag[8];
    for (int i = 0; i < 8; i++) { diag[i] = 0; threshold += w[i]; }
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < 8; i++) {
        double wi = w[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1/wi;
        for (int k = 0; k < 8; k++) diag[k] = diag[k] + v[i*8 + k]*(v[i*8 + k]*wi);
    }
    double maxval = DBL_EPSILON;
    for (int i = 0; i < 8; i++) { const double a = fabs(diag[i]); if (maxval < a) maxval = a; }
    return maxval;
}
// a 45 + 1 reduction's result into A (symmetric), v and rmax
__host__ __device__ inline void hf_unpack_normal(HFitWs* ws)
{
    int o = 0;
    for (int a = 0; a < 8; a++) for (int b = a; b < 8; b++) { ws->A[a*8 + b] = ws->sums[o]; ws->A[b*8 + a] = ws->sums[o]; o++; }
    for (int a = 0; a < 8; a++) ws->v[a] = ws->sums[36 + a];
    ws->rmax = ws->sums[45];
}

// LMSolver::run on ws->H's first eight entries (H[8] stays as it is), over all n pairs
template <class P>
__host__ __device__ void hf_lm(P& p, const float* M, const float* m, int n, HFitWs* ws)
{
    HfJtJ fj; fj.M = M; fj.m = m;
    HfErr fe; fe.M = M; fe.m = m;
    p.one([&] { for (int i = 0; i < 8; i++) ws->x[i] = ws->H[i]; });
    for (int i = 0; i < 8; i++) fj.h[i] = ws->x[i];
    p.template reduce<45>(n, fj, ws);
    p.one([&] {
        hf_unpack_normal(ws);
        ws->S = ws->sums[44];
        for (int i = 0; i < 8; i++) ws->D[i] = ws->A[i*8 + i];
        ws->lambda = 1; ws->lc = 0.75; ws->iter = 0;
    });
    const double Rlo = 0.25, Rhi = 0.75;
    for (int it = 0; it < kHfLmIters; it++) {
        p.one([&] {
            for (int i = 0; i < 64; i++) ws->Ap[i] = ws->A[i];
            for (int i = 0; i < 8; i++) ws->Ap[i*8 + i] += ws->lambda*ws->D[i];
            hf_solve_eig8(ws, ws->Ap, ws->v, ws->d);
            for (int i = 0; i < 8; i++) ws->xd[i] = ws->x[i] - ws->d[i];
        });
        for (int i = 0; i < 8; i++) fe.h[i] = ws->xd[i];
        p.template reduce<1>(n, fe, ws);
        p.one([&] {
            const double S = ws->S, Sd = ws->sums[0];
            const double *d = ws->d, *v = ws->v;
            double dS = 0;
            {
                double temp_d[8];
                for (int i = 0; i < 8; i++) { double s0 = 0; for (int k = 0; k < 8; k++) s0 += ws->A[i*8 + k]*d[k]; temp_d[i] = s0*-1 + v[i]*2; }
                dS = (d[0]*temp_d[0] + d[1]*temp_d[1] + d[2]*temp_d[2] + d[3]*temp_d[3]) + (d[4]*temp_d[4] + d[5]*temp_d[5] + d[6]*temp_d[6] + d[7]*temp_d[7]);
            }
            const double R = (S - Sd)/(fabs(dS) > DBL_EPSILON ? dS : 1);
            if (R > Rhi) { ws->lambda *= 0.5; if (ws->lambda < ws->lc) ws->lambda = 0; }
            else if (R < Rlo) {
                const double t = (d[0]*v[0] + d[1]*v[1] + d[2]*v[2] + d[3]*v[3]) + (d[4]*v[4] + d[5]*v[5] + d[6]*v[6] + d[7]*v[7]);
                double nu = (Sd - S)/(fabs(t) > DBL_EPSILON ? t : 1) + 2;
                nu = nu > 2. ? nu : 2.; nu = nu < 10. ? nu : 10.;
                if (ws->lambda == 0) {
                    ws->lambda = ws->lc = 1./hf_inverse_maxdiag(ws, ws->A);
                    nu *= 0.5;
                }
                ws->lambda *= nu;
            }
            ws->improved = Sd < S ? 1 : 0;
            if (ws->improved) { ws->S = Sd; for (int i = 0; i < 8; i++) ws->x[i] = ws->xd[i]; }
        });
        if (ws->improved) {
            for (int i = 0; i < 8; i++) fj.h[i] = ws->x[i];
            p.template reduce<45>(n, fj, ws);
        }
        p.one([&] {
            if (ws->improved) hf_unpack_normal(ws);
            ws->iter++;
            double dmax = 0;
            for (int i = 0; i < 8; i++) { const double a = fabs(ws->d[i]); if (dmax < a) dmax = a; }
            ws->proceed = (ws->iter < kHfLmIters && dmax >= (double)FLT_EPSILON && ws->rmax >= (double)FLT_EPSILON) ? 1 : 0;
        });
        if (!ws->proceed) break;
    }
    p.one([&] { for (int i = 0; i < 8; i++) ws->H[i] = ws->x[i]; });
}

// The whole fit.  Returns 1 and leaves H in ws->H, or returns 0 (degenerate points, n < 1 or a non-finite result) with ws->H = 0.
// On the device every thread of the workgroup calls it with the same arguments and gets the same return value.
template <class P>
__host__ __device__ int hf_fit_all(P& p, const float* M, const float* m, int n, HFitWs* ws)
{
    p.one([&] { for (int i = 0; i < 9; i++) ws->H[i] = 0; ws->ok = n >= 1 ? 1 : 0; });
    if (!ws->ok) return 0;
    HfCentroid fc; fc.M = M; fc.m = m;
    p.template reduce<4>(n, fc, ws);
    p.one([&] { for (int k = 0; k < 4; k++) ws->st[k] = ws->sums[k] / n; });
    HfSpread fs; fs.M = M; fs.m = m; fs.cMx = ws->st[0]; fs.cMy = ws->st[1]; fs.cmx = ws->st[2]; fs.cmy = ws->st[3];
    p.template reduce<4>(n, fs, ws);
    p.one([&] {
        const double sMx = ws->sums[0], sMy = ws->sums[1], smx = ws->sums[2], smy = ws->sums[3];
        if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) ws->ok = 0;
        else { ws->st[4] = n/sMx; ws->st[5] = n/sMy; ws->st[6] = n/smx; ws->st[7] = n/smy; }
    });
    if (!ws->ok) return 0;
    HfLtL fl; fl.M = M; fl.m = m;
    fl.cMx = ws->st[0]; fl.cMy = ws->st[1]; fl.cmx = ws->st[2]; fl.cmy = ws->st[3];
    fl.sMx = ws->st[4]; fl.sMy = ws->st[5]; fl.smx = ws->st[6]; fl.smy = ws->st[7];
    p.template reduce<45>(n, fl, ws);
    p.one([&] {
        int o = 0;
        for (int j = 0; j < 9; j++) for (int k = j; k < 9; k++) ws->LtL[j*9 + k] = ws->sums[o++];
        homography_tail(ws->st[0], ws->st[1], ws->st[2], ws->st[3], ws->st[4], ws->st[5], ws->st[6], ws->st[7], ws->H,
                        SArr<1>{ws->LtL}, SArr<1>{ws->W}, SArr<1>{ws->V}, ws->ind);
    });
    hf_lm(p, M, m, n, ws);
    p.one([&] {
        int finite = 1;
        for (int i = 0; i < 9; i++) if (!(fabs(ws->H[i]) <= DBL_MAX)) finite = 0;
        if (!finite) { for (int i = 0; i < 9; i++) ws->H[i] = 0; ws->ok = 0; }
    });
    return ws->ok;
}

}  // namespace uvo
