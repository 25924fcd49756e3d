/* o_akaze.c -- TEST INFRASTRUCTURE (CPU oracle; never linked into the product).
 *
 * The AKAZE branch of detect_features (uvo_libraries/src/VO_utility.cpp:93-98):
 *     Ptr<AKAZE> detector = AKAZE::create();  detector->detectAndCompute(img, noArray(), keypoints, descriptors);
 * i.e. DESCRIPTOR_MLDB, descriptor_size 0 (full length: 486 bits = 61 bytes), 3 channels, threshold 0.001f, 4 octaves of 4 sublevels,
 * DIFF_PM_G2.  Restated from memory of OpenCV 4.5 features2d/src/kaze (AKAZEFeatures.cpp: Allocate_Memory_Evolution,
 * create_nonlinear_scale_space, compute_kcontrast, non_linear_diffusion_step, Compute_Determinant_Hessian_Response,
 * FindKeypointsSameScale, Find_Scale_Space_Extrema, Do_Subpixel_Refinement, Compute_Main_Orientation, MLDB_Full_Descriptor_Invoker;
 * fed.cpp: fed_tau_by_process_time; nldiffusion_functions.cpp: pm_g2, compute_scharr_derivative_kernels) and of the imgproc routines
 * they call (GaussianBlur / Scharr / sepFilter2D through the separable filter engine's SCALAR paths, resize INTER_AREA of CV_32F),
 * after the published method: P. F. Alcantarilla, J. Nuevo, A. Bartoli, "Fast explicit diffusion for accelerated features in
 * nonlinear scale spaces", BMVC 2013; FED: Grewenig, Weickert, Bruhn, DAGM 2010.
 *
 * PARITY UNPINNED, confidence MEDIUM: OpenCV is absent here and the reference holds no AKAZE vectors.  What this file pins is the HIP
 * implementation (ergo_uvo_amd/csrc/akaze.hip) to one fixed operation order, and tests/test_oracle_akaze_kat.py pins this file to
 * the closed forms of its parts (FED cycle times, Scharr on a ramp, the conductance on a step, the Hessian determinant of a Gaussian
 * blob, the descriptor's bit count and comparisons).  Stated departures shared with the HIP path: cos / sin of the keypoint angle are
 * orc_sincos rounded to float (as the SIFT branch); the separable filters take the scalar (non-FMA) operation order. */
#include "uvo_oracle.h"
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int w, h; float* d; } fimg;
static fimg fimg_new(int w, int h) { fimg f; f.w = w; f.h = h; f.d = (float*)calloc((size_t)w * h, sizeof(float)); return f; }
static void fimg_free(fimg* f) { free(f->d); f->d = NULL; }
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int reflect101(int p, int n) { if (n == 1) return 0; while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; } return p; }

/* ---- fed.cpp: fed_tau_by_process_time(T, 1, tau_max, reordering = true, tau) ---- */
static int fed_is_prime(int number)
{
    if (number <= 1) return 0;
    if (number == 1 || number == 2 || number == 3 || number == 5 || number == 7) return 1;
    if ((number % 2) == 0 || (number % 3) == 0 || (number % 5) == 0 || (number % 7) == 0) return 0;
    int upperLimit = (int)sqrt(1.0f + number), divisor = 11;
    while (divisor <= upperLimit) {
        if (number % divisor == 0) return 0;
        divisor += 2;
    }
    return 1;
}
int orc_akaze_fed_tau(float T, float tau_max, float* tau /* >= 256 */)
{
    const float t = T / 1.0f;                                                 /* fed_tau_by_cycle_time(T / M, ...) with M = 1 cycle */
    const int n = orc_cvCeil(sqrtf(3.0f * t / tau_max + 0.25f) - 0.5f - 1.0e-8f);
    const float scale = 3.0f * t / (tau_max * (float)(n * (n + 1)));
    if (n <= 0) return 0;
    float tauh[256];
    const float c = 1.0f / (4.0f * (float)n + 2.0f), d = scale * tau_max / 2.0f;
    for (int k = 0; k < n; ++k) {
        const float hh = cosf((float)3.14159265358979323846 * (2.0f * (float)k + 1.0f) * c);
        tauh[k] = d / (hh * hh);
    }
    const int kappa = n / 2;
    int prime = n + 1;
    while (!fed_is_prime(prime)) prime++;
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index = 0;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return n;
}

/* ---- the separable filters, scalar paths of imgproc's filter engine ---- */
/* getGaussianKernel(n, sigma, CV_32F) as orc_gaussian_kernel_f32 (o_surf.c) */
void orc_gaussian_kernel_f32(int n, double sigma, float* out);
/* GaussianBlur(src, dst, Size(ksize, ksize), sigma, sigma, BORDER_REPLICATE) on CV_32F.  ksize 5: SymmRowSmallFilter (centre first, then the
 * mirrored pairs outward); wider: the generic RowFilter (left to right).  Columns: SymmColumnFilter (centre, then pairs outward). */
static void gaussian_blur_replicate(const fimg* src, fimg* dst, int ksize, float sigma)
{
    float k[64];
    orc_gaussian_kernel_f32(ksize, (double)sigma, k);
    const int r = ksize / 2, w = src->w, h = src->h;
    float* tmp = (float*)malloc(sizeof(float) * (size_t)w * h);
    for (int y = 0; y < h; y++) {
        const float* s = src->d + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            float acc;
            if (ksize <= 5) {
                acc = k[r] * s[x];
                for (int i = 1; i <= r; i++) acc += k[r + i] * (s[clampi(x - i, 0, w - 1)] + s[clampi(x + i, 0, w - 1)]);
            } else {
                acc = k[0] * s[clampi(x - r, 0, w - 1)];
                for (int t = 1; t < ksize; t++) acc += k[t] * s[clampi(x - r + t, 0, w - 1)];
            }
            tmp[(size_t)y * w + x] = acc;
        }
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float acc = k[r] * tmp[(size_t)y * w + x];
            for (int i = 1; i <= r; i++) acc += k[r + i] * (tmp[(size_t)clampi(y + i, 0, h - 1) * w + x] + tmp[(size_t)clampi(y - i, 0, h - 1) * w + x]);
            dst->d[(size_t)y * w + x] = acc;
        }
    free(tmp);
}
static int gaussian_ksize(float sigma) { int k = orc_cvCeil(2.0f * (1.0f + (sigma - 0.8f) / (0.3f))); return k | 1; }

/* Scharr(src, dst, CV_32F, dx, dy, 1, 0, BORDER_DEFAULT): kernels [-1 0 1] along the derivative and [3 10 3] across it, unnormalised;
 * SymmRowSmallFilter / SymmColumnSmallFilter for 3 taps: the difference is S[+1] - S[-1], the smoothing (S[-1] + S[+1]) * 3 + S[0] * 10 */
void orc_akaze_scharr(const float* src, int w, int h, int xorder, float* dst)
{
    float* tmp = (float*)malloc(sizeof(float) * (size_t)w * h);
    for (int y = 0; y < h; y++) {
        const float* s = src + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            const float a = s[reflect101(x - 1, w)], b = s[x], c = s[reflect101(x + 1, w)];
            tmp[(size_t)y * w + x] = xorder ? c - a : b * 10.f + (a + c) * 3.f;
        }
    }
    for (int y = 0; y < h; y++) {
        const float* s0 = tmp + (size_t)reflect101(y - 1, h) * w; const float* s1 = tmp + (size_t)y * w; const float* s2 = tmp + (size_t)reflect101(y + 1, h) * w;
        for (int x = 0; x < w; x++) dst[(size_t)y * w + x] = xorder ? (s0[x] + s2[x]) * 3.f + s1[x] * 10.f : s2[x] - s0[x];
    }
    free(tmp);
}

/* compute_derivative_kernels(kx, ky, dx, dy, scale) + sepFilter2D(src, dst, CV_32F, kx, ky) (BORDER_DEFAULT): the Scharr pair
 * stretched to 3 + 2 (scale - 1) taps -- difference [-1 0 .. 0 1], smoothing [n 0 .. w n .. 0 n] with w = 10 / 3, n = 1 / (2 scale (w + 2)).
 * Rows: 5 taps take SymmRowSmallFilter (centre, then pairs), 7 and 9 the generic RowFilter (left to right; the zero taps add +-0);
 * columns: SymmColumnFilter.  (AKAZE's scales are 2, 3, 4: the scale-1 branch, getDerivKernels, is never taken.) */
static void sep_deriv(const fimg* src, fimg* dst, int xorder, int scale)
{
    const int r = scale, w = src->w, h = src->h, ksize = 3 + 2 * (scale - 1);
    const float ww = 10.0f / 3.0f, nrm = 1.0f / (2.0f * scale * (ww + 2.0f)), wn = ww * nrm;
    float* tmp = (float*)malloc(sizeof(float) * (size_t)w * h);
    for (int y = 0; y < h; y++) {
        const float* s = src->d + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            const float a = s[reflect101(x - r, w)], b = s[x], c = s[reflect101(x + r, w)];
            float v;
            if (xorder) v = c - a;                                                   /* [-1 .. 1] */
            else if (ksize <= 5) v = wn * b + nrm * (a + c);                         /* centre, then the pair */
            else { v = nrm * a; v += wn * b; v += nrm * c; }                        /* left to right */
            tmp[(size_t)y * w + x] = v;
        }
    }
    for (int y = 0; y < h; y++) {
        const float* s0 = tmp + (size_t)reflect101(y - r, h) * w; const float* s1 = tmp + (size_t)y * w; const float* s2 = tmp + (size_t)reflect101(y + r, h) * w;
        for (int x = 0; x < w; x++) dst->d[(size_t)y * w + x] = xorder ? wn * s1[x] + nrm * (s2[x] + s0[x]) : s2[x] - s0[x];
    }
    free(tmp);
}

/* resize(src, dst, dsize, 0, 0, INTER_AREA) of CV_32F, downscaling: exact factor 2 -> resizeAreaFast_ ((S00 + S01 + S10 + S11) * 0.25f), else
 * resizeArea_ with computeResizeAreaTab's float weights (as o_surf.c's 8-bit variant, without the final rounding) */
typedef struct { int si, di; float alpha; } DecAlpha;
static int area_tab(int ssize, int dsize, double scale, DecAlpha* tab)
{
    int k = 0;
    for (int dx = 0; dx < dsize; dx++) {
        double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        double cellWidth = scale < ssize - fsx1 ? scale : ssize - fsx1;
        int sx1 = orc_cvCeil(fsx1), sx2 = orc_cvFloor(fsx2);
        sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
        sx1 = sx1 < sx2 ? sx1 : sx2;
        if (sx1 - fsx1 > 1e-3) { tab[k].di = dx; tab[k].si = sx1 - 1; tab[k++].alpha = (float)((sx1 - fsx1) / cellWidth); }
        for (int sx = sx1; sx < sx2; sx++) { tab[k].di = dx; tab[k].si = sx; tab[k++].alpha = (float)(1.0 / cellWidth); }
        if (fsx2 - sx2 > 1e-3) {
            double a = fsx2 - sx2; if (a > 1.) a = 1.; if (a > cellWidth) a = cellWidth;
            tab[k].di = dx; tab[k].si = sx2; tab[k++].alpha = (float)(a / cellWidth);
        }
    }
    return k;
}
static void resize_area_f32(const fimg* src, fimg* dst)
{
    const int sw = src->w, sh = src->h, dw = dst->w, dh = dst->h;
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    const int iscale_x = orc_cvRound(scale_x), iscale_y = orc_cvRound(scale_y);
    if (fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON && iscale_x == 2 && iscale_y == 2) {
        for (int dy = 0; dy < dh; dy++)
            for (int dx = 0; dx < dw; dx++) {
                const float* S = src->d + (size_t)(2 * dy) * sw + 2 * dx;
                float sum = 0;
                sum += S[0]; sum += S[1]; sum += S[sw]; sum += S[sw + 1];
                dst->d[(size_t)dy * dw + dx] = sum * 0.25f;
            }
        return;
    }
    DecAlpha* xtab = (DecAlpha*)malloc(sizeof(DecAlpha) * (size_t)(sw + sh) * 2);
    DecAlpha* ytab = xtab + sw * 2;
    const int xn = area_tab(sw, dw, scale_x, xtab), yn = area_tab(sh, dh, scale_y, ytab);
    float* buf = (float*)malloc(sizeof(float) * dw * 2);
    float* sum = buf + dw;
    int prev_dy = ytab[0].di;
    for (int dx = 0; dx < dw; dx++) sum[dx] = 0;
    for (int j = 0; j < yn; j++) {
        const float beta = ytab[j].alpha;
        const int dy = ytab[j].di;
        const float* S = src->d + (size_t)ytab[j].si * sw;
        for (int dx = 0; dx < dw; dx++) buf[dx] = 0;
        for (int k = 0; k < xn; k++) buf[xtab[k].di] += S[xtab[k].si] * xtab[k].alpha;
        if (dy != prev_dy) {
            float* D = dst->d + (size_t)prev_dy * dw;
            for (int dx = 0; dx < dw; dx++) { D[dx] = sum[dx]; sum[dx] = beta * buf[dx]; }
            prev_dy = dy;
        } else for (int dx = 0; dx < dw; dx++) sum[dx] += beta * buf[dx];
    }
    { float* D = dst->d + (size_t)prev_dy * dw; for (int dx = 0; dx < dw; dx++) D[dx] = sum[dx]; }
    free(buf); free(xtab);
}

/* ---- nldiffusion_functions.cpp ---- */
void orc_akaze_pm_g2(const float* lx, const float* ly, int n, float k, float* dst)
{
    const float k2inv = 1.0f / (k * k);
    for (int i = 0; i < n; i++) dst[i] = 1.0f / (1.0f + ((lx[i] * lx[i] + ly[i] * ly[i]) * k2inv));
}
/* compute_kcontrast(Lx, Ly, perc, nbins): the perc-quantile of the gradient magnitude histogram over the interior, background bin excluded */
static float compute_kcontrast(const fimg* Lx, const fimg* Ly, float perc, int nbins)
{
    const int rows = Lx->h - 2, cols = Lx->w - 2, total = rows * cols;
    if (total <= 0) return 0.03f;
    float* modg = (float*)malloc(sizeof(float) * (size_t)total);
    float hmax = 0.0f;
    int q = 0;
    for (int i = 1; i < Lx->h - 1; i++)
        for (int j = 0; j < cols; j++) {
            const float lx = Lx->d[(size_t)i * Lx->w + 1 + j], ly = Ly->d[(size_t)i * Lx->w + 1 + j];
            const float dist = sqrtf(lx * lx + ly * ly);
            modg[q++] = dist;
            hmax = hmax > dist ? hmax : dist;
        }
    if (hmax == 0.0f) { free(modg); return 0.03f; }
    const float sc = (nbins - 1) / hmax;                      /* modgs *= (nbins - 1) / hmax */
    int* hist = (int*)calloc((size_t)nbins, sizeof(int));
    for (int i = 0; i < total; i++) hist[(int)(modg[i] * sc)]++;
    const int nthreshold = (int)((total - hist[0]) * perc);
    int nelements = 0;
    float res = 0.03f;
    for (int k = 1; k < nbins; k++) {
        if (nelements >= nthreshold) { res = (float)hmax * k / nbins; break; }
        nelements = nelements + hist[k];
    }
    free(hist); free(modg);
    return res;
}
/* non_linear_diffusion_step: Lstep = step * div(c grad L) on the five-point star with the conductances averaged to the half points; the
 * image border uses the one-sided stencil, its four corners stay 0 */
void orc_akaze_nld_step(const float* lt, const float* lf, int w, int h, float step_size, float* out)
{
    const int cols = w - 2;
    for (int row = 0; row < h; row++) {
        const float* lt_c = lt + (size_t)row * w; const float* lf_c = lf + (size_t)row * w;
        const float* lt_a = row > 0 ? lt_c - w : NULL; const float* lf_a = row > 0 ? lf_c - w : NULL;
        const float* lt_b = row < h - 1 ? lt_c + w : NULL; const float* lf_b = row < h - 1 ? lf_c + w : NULL;
        float* dst = out + (size_t)row * w;
        if (row == 0 || row == h - 1) {
            const float* lt_o = row == 0 ? lt_b : lt_a; const float* lf_o = row == 0 ? lf_b : lf_a;      /* the one neighbouring row */
            dst[0] = 0.0f;
            for (int j = 1; j <= cols; j++) {
                const float step_r = (lf_c[j] + lf_c[j + 1]) * (lt_c[j + 1] - lt_c[j]) +
                                     (lf_c[j] + lf_c[j - 1]) * (lt_c[j - 1] - lt_c[j]) +
                                     (lf_c[j] + lf_o[j]) * (lt_o[j] - lt_c[j]);
                dst[j] = step_r * step_size;
            }
            dst[w - 1] = 0.0f;
            continue;
        }
        {   /* the left-most column */
            const float step_r = (lf_c[0] + lf_c[1]) * (lt_c[1] - lt_c[0]) + (lf_c[0] + lf_b[0]) * (lt_b[0] - lt_c[0]) + (lf_c[0] + lf_a[0]) * (lt_a[0] - lt_c[0]);
            dst[0] = step_r * step_size;
        }
        for (int j = 1; j <= cols; j++) {
            const float step_r = (lf_c[j] + lf_c[j + 1]) * (lt_c[j + 1] - lt_c[j]) +
                                 (lf_c[j] + lf_c[j - 1]) * (lt_c[j - 1] - lt_c[j]) +
                                 (lf_c[j] + lf_b[j]) * (lt_b[j] - lt_c[j]) +
                                 (lf_c[j] + lf_a[j]) * (lt_a[j] - lt_c[j]);
            dst[j] = step_r * step_size;
        }
        {   /* the right-most column */
            const int e = w - 1;
            const float step_r = (lf_c[e] + lf_c[e - 1]) * (lt_c[e - 1] - lt_c[e]) + (lf_c[e] + lf_b[e]) * (lt_b[e] - lt_c[e]) + (lf_c[e] + lf_a[e]) * (lt_a[e] - lt_c[e]);
            dst[e] = step_r * step_size;
        }
    }
}

/* ---- the evolution (Allocate_Memory_Evolution with AKAZE::create()'s defaults) ---- */
#define AKAZE_MAX_LEVELS 16
typedef struct { int w, h, octave, sublevel, sigma_size, border; float esigma, etime, octave_ratio; int nsteps; float tau[64]; } akaze_level;
int orc_akaze_levels(int img_w, int img_h, int* out /* [n][6]: w, h, octave, sigma_size, border, nsteps */, float* esigma)
{
    akaze_level L[AKAZE_MAX_LEVELS];
    extern int orc_akaze_plan(int, int, akaze_level*);
    const int n = orc_akaze_plan(img_w, img_h, L);
    for (int i = 0; i < n; i++) {
        out[6*i] = L[i].w; out[6*i+1] = L[i].h; out[6*i+2] = L[i].octave; out[6*i+3] = L[i].sigma_size; out[6*i+4] = L[i].border; out[6*i+5] = L[i].nsteps;
        if (esigma) esigma[i] = L[i].esigma;
    }
    return n;
}
int orc_akaze_plan(int img_w, int img_h, akaze_level* L)
{
    const int omax = 4, nsublevels = 4;
    const float soffset = 1.6f, derivative_factor = 1.5f, smax = 10.0f * sqrtf(2.0f);
    int n = 0;
    for (int i = 0, power = 1; i <= omax - 1; i++, power *= 2) {
        const float rfactor = 1.0f / power;
        const int level_height = (int)(img_h * rfactor), level_width = (int)(img_w * rfactor);
        if ((level_width < 80 || level_height < 40) && i != 0) break;
        for (int j = 0; j < nsublevels; j++) {
            akaze_level* s = &L[n++];
            s->w = level_width; s->h = level_height;
            s->esigma = soffset * powf(2.f, (float)(j) / (float)(nsublevels) + i);
            s->sigma_size = orc_cvRoundf(s->esigma * derivative_factor / power);
            s->etime = 0.5f * (s->esigma * s->esigma);
            s->octave = i; s->sublevel = j; s->octave_ratio = (float)power;
            s->border = orc_cvRoundf(smax * s->sigma_size) + 1;
            s->nsteps = 0;
        }
    }
    for (int i = 1; i < n; i++) L[i].nsteps = orc_akaze_fed_tau(L[i].etime - L[i - 1].etime, 0.25f, L[i].tau);
    return n;
}

typedef struct { int n; akaze_level lv[AKAZE_MAX_LEVELS]; fimg Lt[AKAZE_MAX_LEVELS], Lsmooth[AKAZE_MAX_LEVELS], Lx[AKAZE_MAX_LEVELS], Ly[AKAZE_MAX_LEVELS], Ldet[AKAZE_MAX_LEVELS];
                 float kcontrast; } akaze_space;

static void akaze_free(akaze_space* s)
{
    for (int i = 0; i < s->n; i++) { fimg_free(&s->Lt[i]); fimg_free(&s->Lsmooth[i]); fimg_free(&s->Lx[i]); fimg_free(&s->Ly[i]); fimg_free(&s->Ldet[i]); }
}
/* Create_Nonlinear_Scale_Space + Compute_Determinant_Hessian_Response */
static void akaze_build(const uint8_t* img8, int w, int h, int stride, akaze_space* s)
{
    memset(s, 0, sizeof(*s));
    s->n = orc_akaze_plan(w, h, s->lv);
    fimg img = fimg_new(w, h);
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) img.d[(size_t)y * w + x] = (float)((double)img8[(size_t)y * stride + x] * (1.0 / 255.0));   /* convertTo(CV_32F, 1 / 255.) */
    for (int i = 0; i < s->n; i++) {
        const akaze_level* lv = &s->lv[i];
        s->Lt[i] = fimg_new(lv->w, lv->h); s->Lsmooth[i] = fimg_new(lv->w, lv->h); s->Lx[i] = fimg_new(lv->w, lv->h); s->Ly[i] = fimg_new(lv->w, lv->h);
        s->Ldet[i] = fimg_new(lv->w, lv->h);
    }
    gaussian_blur_replicate(&img, &s->Lsmooth[0], gaussian_ksize(1.6f), 1.6f);
    memcpy(s->Lt[0].d, s->Lsmooth[0].d, sizeof(float) * (size_t)w * h);
    fimg Lx = fimg_new(w, h), Ly = fimg_new(w, h), Lsm = fimg_new(w, h), Lflow = fimg_new(w, h), Lstep = fimg_new(w, h);
    float kcontrast = 0.f;
    if (s->n > 1) {
        gaussian_blur_replicate(&img, &Lsm, 5, 1.0f);
        orc_akaze_scharr(Lsm.d, w, h, 1, Lx.d);
        orc_akaze_scharr(Lsm.d, w, h, 0, Ly.d);
        kcontrast = compute_kcontrast(&Lx, &Ly, 0.7f, 300);
    }
    s->kcontrast = kcontrast;
    for (int i = 1; i < s->n; i++) {
        const akaze_level* lv = &s->lv[i];
        const int lw = lv->w, lh = lv->h;
        if (lv->octave > s->lv[i - 1].octave) { resize_area_f32(&s->Lt[i - 1], &s->Lt[i]); kcontrast *= 0.75f; }
        else memcpy(s->Lt[i].d, s->Lt[i - 1].d, sizeof(float) * (size_t)lw * lh);
        gaussian_blur_replicate(&s->Lt[i], &s->Lsmooth[i], 5, 1.0f);
        fimg lx = { lw, lh, Lx.d }, ly = { lw, lh, Ly.d };
        orc_akaze_scharr(s->Lsmooth[i].d, lw, lh, 1, lx.d);
        orc_akaze_scharr(s->Lsmooth[i].d, lw, lh, 0, ly.d);
        orc_akaze_pm_g2(lx.d, ly.d, lw * lh, kcontrast, Lflow.d);
        for (int j = 0; j < lv->nsteps; j++) {
            const float step_size = lv->tau[j] * 0.5f;
            orc_akaze_nld_step(s->Lt[i].d, Lflow.d, lw, lh, step_size, Lstep.d);
            for (int q = 0; q < lw * lh; q++) s->Lt[i].d[q] = s->Lt[i].d[q] + Lstep.d[q];
        }
    }
    /* the multiscale derivatives and the determinant of the Hessian scaled by sigma_size^4 */
    for (int i = 0; i < s->n; i++) {
        const akaze_level* lv = &s->lv[i];
        const int lw = lv->w, lh = lv->h, n = lw * lh;
        fimg Lxx = { lw, lh, Lflow.d }, Lxy = { lw, lh, Lstep.d }, Lyy = { lw, lh, Lsm.d };
        sep_deriv(&s->Lsmooth[i], &s->Lx[i], 1, lv->sigma_size);
        sep_deriv(&s->Lx[i], &Lxx, 1, lv->sigma_size);
        sep_deriv(&s->Lx[i], &Lxy, 0, lv->sigma_size);
        sep_deriv(&s->Lsmooth[i], &s->Ly[i], 0, lv->sigma_size);
        sep_deriv(&s->Ly[i], &Lyy, 0, lv->sigma_size);
        const float sig4 = (float)(lv->sigma_size * lv->sigma_size * lv->sigma_size * lv->sigma_size);
        for (int q = 0; q < n; q++) s->Ldet[i].d[q] = (Lxx.d[q] * Lyy.d[q] - Lxy.d[q] * Lxy.d[q]) * sig4;
    }
    fimg_free(&Lx); fimg_free(&Ly); fimg_free(&Lsm); fimg_free(&Lflow); fimg_free(&Lstep); fimg_free(&img);
}
/* intermediates for the parity tests: what = 0 Lt, 1 Lsmooth, 2 Lx, 3 Ly, 4 Ldet of `level`; returns w * h (0: no such level) */
int orc_akaze_plane(const uint8_t* img, int w, int h, int stride, int level, int what, float* out, int* ow, int* oh, float* kcontrast)
{
    akaze_space* s = (akaze_space*)malloc(sizeof(akaze_space));
    akaze_build(img, w, h, stride, s);
    int n = 0;
    if (level >= 0 && level < s->n && what >= 0 && what <= 4) {
        const fimg* f = what == 0 ? &s->Lt[level] : what == 1 ? &s->Lsmooth[level] : what == 2 ? &s->Lx[level] : what == 3 ? &s->Ly[level] : &s->Ldet[level];
        n = f->w * f->h; *ow = f->w; *oh = f->h;
        memcpy(out, f->d, sizeof(float) * (size_t)n);
    }
    if (kcontrast) *kcontrast = s->kcontrast;
    akaze_free(s); free(s);
    return n;
}

/* ---- Find_Scale_Space_Extrema ---- */
static int find_neighbor_point(int x, int y, const uint8_t* mask, int cols, int rows, int search_radius, int* idx)
{
    for (int i = y - search_radius; i < y + search_radius; ++i) {
        if (i < 0 || i >= rows) continue;                      /* (OpenCV's callers keep the window inside the plane through `border`; guarded here) */
        const uint8_t* curr = mask + (size_t)i * cols;
        for (int j = x - search_radius; j < x + search_radius; ++j) {
            if (j < 0 || j >= cols) continue;
            if (curr[j] == 0) continue;
            const int dx = j - x, dy = i - y;
            if (dx * dx + dy * dy <= search_radius * search_radius) { *idx = i * cols + j; return 1; }
        }
    }
    return 0;
}
/* The sequential part on lists of candidates, shared in spirit with the product's host code: `cand` marks the strict 3 x 3 maxima above the
 * threshold inside the border (what a parallel pass can find); the row-major scan with same-scale suppression follows */
static void keypoints_same_scale(const akaze_level* lv, const float* ldet, uint8_t* kpts, float dthreshold)
{
    const int rows = lv->h, cols = lv->w, b = lv->border;
    memset(kpts, 0, (size_t)rows * cols);
    if (b + 1 >= rows) return;
    for (int y = b; y < rows - b; y++) {
        const float* prev = ldet + (size_t)(y - 1) * cols; const float* curr = ldet + (size_t)y * cols; const float* next = ldet + (size_t)(y + 1) * cols;
        for (int x = b; x < cols - b; x++) {
            const float value = curr[x];
            if (value <= dthreshold) continue;
            if (value <= curr[x - 1] || value <= curr[x + 1]) continue;
            if (value <= prev[x - 1] || value <= prev[x] || value <= prev[x + 1]) continue;
            if (value <= next[x - 1] || value <= next[x] || value <= next[x + 1]) continue;
            int idx = 0;
            if (find_neighbor_point(x, y, kpts, cols, rows, lv->sigma_size, &idx)) {
                if (value > ldet[idx]) kpts[idx] = 0;          /* the old point goes: a better candidate is here */
                else continue;                                /* a better keypoint is there already */
            }
            kpts[(size_t)y * cols + x] = 1;
        }
    }
}
static void filter_across_scales(const akaze_space* s, uint8_t** kp)
{
    for (int i = 1; i < s->n; i++) {                            /* against the lower level */
        const akaze_level* lv = &s->lv[i]; const akaze_level* lp = &s->lv[i - 1];
        const int diff_ratio = (int)lv->octave_ratio / (int)lp->octave_ratio;
        const int search_radius = lv->sigma_size * diff_ratio;
        size_t j = 0;
        for (int y = 0; y < lv->h; y++)
            for (int x = 0; x < lv->w; x++, j++) {
                if (kp[i][j] == 0) continue;
                int idx = 0;
                if (find_neighbor_point(x * diff_ratio, y * diff_ratio, kp[i - 1], lp->w, lp->h, search_radius, &idx))
                    if (s->Ldet[i].d[j] > s->Ldet[i - 1].d[idx]) kp[i - 1][idx] = 0;
            }
    }
    for (int i = s->n - 2; i >= 0; i--) {                       /* against the upper level */
        const akaze_level* lv = &s->lv[i]; const akaze_level* ln = &s->lv[i + 1];
        const int diff_ratio = (int)ln->octave_ratio / (int)lv->octave_ratio;
        const int search_radius = ln->sigma_size;
        size_t j = 0;
        for (int y = 0; y < lv->h; y++)
            for (int x = 0; x < lv->w; x++, j++) {
                if (kp[i][j] == 0) continue;
                int idx = 0;
                if (find_neighbor_point(x / diff_ratio, y / diff_ratio, kp[i + 1], ln->w, ln->h, search_radius, &idx))
                    if (s->Ldet[i].d[j] > s->Ldet[i + 1].d[idx]) kp[i + 1][idx] = 0;
            }
    }
}

/* ---- Compute_Main_Orientation ---- */
static const float gauss25[7][7] = {
    { 0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f },
    { 0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f },
    { 0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f },
    { 0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f },
    { 0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f },
    { 0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f },
    { 0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f } };
const float* orc_akaze_gauss25(void) { return &gauss25[0][0]; }
float orc_fast_atan2(float y, float x);
static float main_orientation(const akaze_space* s, const orc_keypoint* kpt)
{
    const akaze_level* e = &s->lv[kpt->class_id];
    const fimg* Lx = &s->Lx[kpt->class_id]; const fimg* Ly = &s->Ly[kpt->class_id];
    const int scale = orc_cvRoundf(0.5f * kpt->size / e->octave_ratio);
    const int x0 = orc_cvRoundf(kpt->x / e->octave_ratio), y0 = orc_cvRoundf(kpt->y / e->octave_ratio);
    enum { ang_size = 109, slices = 42, win = 7 };
    float resX[ang_size], resY[ang_size], Ang[ang_size];
    int k = 0;
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j)
            if (i * i + j * j < 36) {
                const float wgt = gauss25[abs(i)][abs(j)];
                const int y = clampi(y0 + i * scale, 0, Lx->h - 1), x = clampi(x0 + j * scale, 0, Lx->w - 1);      /* (inside the plane by `border`; clamped for safety) */
                resX[k] = wgt * Lx->d[(size_t)y * Lx->w + x]; resY[k] = wgt * Ly->d[(size_t)y * Lx->w + x];
                ++k;
            }
    for (int i = 0; i < ang_size; i++) Ang[i] = orc_fast_atan2(resY[i], resX[i]) * (float)(3.14159265358979323846 / 180.0);     /* hal::fastAtan2(.., false) */
    const float ang_step = (float)(2.0 * 3.14159265358979323846 / slices);
    int slice[slices + 1], ang_order[ang_size];
    memset(slice, 0, sizeof(slice));                                                /* quantized_counting_sort */
    for (int i = 0; i < ang_size; i++) { int b = (int)(Ang[i] / ang_step); if (b < 0 || b >= slices) b = 0; slice[b]++; }
    for (int i = 1; i <= slices; i++) slice[i] += slice[i - 1];
    for (int i = 0; i < ang_size; i++) { int b = (int)(Ang[i] / ang_step); if (b < 0 || b >= slices) b = 0; ang_order[--slice[b]] = i; }
    float maxX = 0.0f, maxY = 0.0f;
    for (int i = slice[0]; i < slice[win]; i++) { const int idx = ang_order[i]; maxX += resX[idx]; maxY += resY[idx]; }
    float maxNorm = maxX * maxX + maxY * maxY;
    for (int sn = 1; sn <= slices - win; sn++) {
        if (slice[sn] == slice[sn - 1] && slice[sn + win] == slice[sn + win - 1]) continue;
        float sumX = 0.0f, sumY = 0.0f;
        for (int i = slice[sn]; i < slice[sn + win]; i++) { const int idx = ang_order[i]; sumX += resX[idx]; sumY += resY[idx]; }
        const float norm = sumX * sumX + sumY * sumY;
        if (norm > maxNorm) { maxNorm = norm; maxX = sumX; maxY = sumY; }
    }
    for (int sn = slices - win + 1; sn < slices; sn++) {
        const int remain = sn + win - slices;
        if (slice[sn] == slice[sn - 1] && slice[remain] == slice[remain - 1]) continue;
        float sumX = 0.0f, sumY = 0.0f;
        for (int i = slice[sn]; i < slice[slices]; i++) { const int idx = ang_order[i]; sumX += resX[idx]; sumY += resY[idx]; }
        for (int i = slice[0]; i < slice[remain]; i++) { const int idx = ang_order[i]; sumX += resX[idx]; sumY += resY[idx]; }
        const float norm = sumX * sumX + sumY * sumY;
        if (norm > maxNorm) { maxNorm = norm; maxX = sumX; maxY = sumY; }
    }
    return orc_fast_atan2(maxY, maxX);
}

/* ---- MLDB_Full_Descriptor_Invoker::Get_MLDB_Full_Descriptor (rotated, 3 channels, pattern 10) ---- */
#define AKAZE_DESC_BYTES 61
static void mldb_descriptor(const akaze_space* s, const orc_keypoint* kpt, uint8_t* desc)
{
    const akaze_level* e = &s->lv[kpt->class_id];
    const fimg* Lt = &s->Lt[kpt->class_id]; const fimg* Lx = &s->Lx[kpt->class_id]; const fimg* Ly = &s->Ly[kpt->class_id];
    const float ratio = e->octave_ratio;
    const float scale = (float)orc_cvRoundf(0.5f * kpt->size / ratio);
    const float xf = kpt->x / ratio, yf = kpt->y / ratio;
    const float angle = (kpt->angle * (float)3.14159265358979323846) / 180.f;
    double sd, cd;
    orc_sincos((double)angle, &sd, &cd);
    const float co = (float)cd, si = (float)sd;
    const int pattern_size = 10;
    static const double size_mult[3] = { 1, 2.0 / 3.0, 1.0 / 2.0 };
    memset(desc, 0, AKAZE_DESC_BYTES);
    int dpos = 0;
    for (int lvl = 0; lvl < 3; lvl++) {
        const int val_count = (lvl + 2) * (lvl + 2);
        const int sample_step = (int)ceil(pattern_size * size_mult[lvl]);
        float values[16 * 3];
        int valpos = 0;
        for (int i = -pattern_size; i < pattern_size; i += sample_step)
            for (int j = -pattern_size; j < pattern_size; j += sample_step) {
                float di = 0.0f, dx = 0.0f, dy = 0.0f;
                int nsamples = 0;
                for (int k = i; k < i + sample_step; k++)
                    for (int l = j; l < j + sample_step; l++) {
                        const float sample_y = yf + (l * co * scale + k * si * scale);
                        const float sample_x = xf + (-l * si * scale + k * co * scale);
                        const int y1 = clampi(orc_cvRoundf(sample_y), 0, Lt->h - 1), x1 = clampi(orc_cvRoundf(sample_x), 0, Lt->w - 1);
                        const float ri = Lt->d[(size_t)y1 * Lt->w + x1];
                        di += ri;
                        const float rx = Lx->d[(size_t)y1 * Lt->w + x1], ry = Ly->d[(size_t)y1 * Lt->w + x1];
                        const float rry = rx * co + ry * si, rrx = -rx * si + ry * co;
                        dx += rrx; dy += rry;
                        nsamples++;
                    }
                di /= nsamples; dx /= nsamples; dy /= nsamples;
                values[valpos] = di; values[valpos + 1] = dx; values[valpos + 2] = dy;
                valpos += 3;
            }
        int ivalues[16 * 3];                                    /* CV_TOGGLE_FLT: the floats as order-preserving integers */
        for (int q = 0; q < val_count * 3; q++) { int v; memcpy(&v, &values[q], 4); ivalues[q] = v ^ ((v < 0) ? 0x7fffffff : 0); }
        for (int pos = 0; pos < 3; pos++)
            for (int i = 0; i < val_count; i++) {
                const int ival = ivalues[3 * i + pos];
                for (int j = i + 1; j < val_count; j++) {
                    const int res = ival > ivalues[3 * j + pos];
                    desc[dpos >> 3] |= (uint8_t)(res << (dpos & 7));
                    dpos++;
                }
            }
    }
}

/* detectAndCompute: keypoints level by level in row-major order (Do_Subpixel_Refinement's order), angle in degrees, 61-byte rows.
 * Returns the count, or -(count) when cap is too small. */
int orc_akaze_detect_and_compute(const uint8_t* img, int w, int h, int stride, orc_keypoint* kps, uint8_t* desc, int cap)
{
    akaze_space* s = (akaze_space*)malloc(sizeof(akaze_space));
    akaze_build(img, w, h, stride, s);
    uint8_t* kp[AKAZE_MAX_LEVELS];
    for (int i = 0; i < s->n; i++) { kp[i] = (uint8_t*)malloc((size_t)s->lv[i].w * s->lv[i].h); keypoints_same_scale(&s->lv[i], s->Ldet[i].d, kp[i], 0.001f); }
    filter_across_scales(s, kp);
    int n = 0;
    for (int i = 0; i < s->n; i++) {                              /* Do_Subpixel_Refinement */
        const akaze_level* e = &s->lv[i];
        const float* ldet = s->Ldet[i].d;
        const float ratio = e->octave_ratio;
        const int cols = e->w;
        size_t j = 0;
        for (int y = 0; y < e->h; y++)
            for (int x = 0; x < e->w; x++, j++) {
                if (kp[i][j] == 0) continue;
                orc_keypoint k;
                k.x = x * e->octave_ratio; k.y = y * e->octave_ratio;
                k.size = e->esigma * 1.5f;
                k.angle = -1; k.response = ldet[j]; k.octave = e->octave; k.class_id = i;
                const float Dx = 0.5f * (ldet[y * cols + x + 1] - ldet[y * cols + x - 1]);
                const float Dy = 0.5f * (ldet[(y + 1) * cols + x] - ldet[(y - 1) * cols + x]);
                const float Dxx = ldet[y * cols + x + 1] + ldet[y * cols + x - 1] - 2.0f * ldet[y * cols + x];
                const float Dyy = ldet[(y + 1) * cols + x] + ldet[(y - 1) * cols + x] - 2.0f * ldet[y * cols + x];
                const float Dxy = 0.25f * (ldet[(y + 1) * cols + x + 1] + ldet[(y - 1) * cols + x - 1] - ldet[(y - 1) * cols + x + 1] - ldet[(y + 1) * cols + x - 1]);
                /* solve(Matx22f(Dxx, Dxy, Dxy, Dyy), Vec2f(-Dx, -Dy), dst, DECOMP_LU): the 2 x 2 CV_32F branch of lapack.cpp's solve --
                 * determinant and numerators in double, the result cast to float; a zero determinant leaves dst = 0 */
                float dx = 0.0f, dy = 0.0f;
                double det = (double)Dxx * Dyy - (double)Dxy * Dxy;
                if (det != 0) { det = 1. / det; dx = (float)(((double)(-Dx) * Dyy - (double)(-Dy) * Dxy) * det); dy = (float)(((double)(-Dy) * Dxx - (double)(-Dx) * Dxy) * det); }
                if (fabsf(dx) > 1.0f || fabsf(dy) > 1.0f) continue;
                k.x += dx * ratio + .5f * (ratio - 1.f);
                k.y += dy * ratio + .5f * (ratio - 1.f);
                k.angle = 0.0f;
                k.size *= 2.0f;
                if (n < cap) kps[n] = k;
                n++;
            }
    }
    if (n <= cap)
        for (int q = 0; q < n; q++) {                             /* Compute_Keypoints_Orientation, then the descriptors */
            kps[q].angle = main_orientation(s, &kps[q]);
            if (desc) mldb_descriptor(s, &kps[q], desc + (size_t)q * AKAZE_DESC_BYTES);
        }
    for (int i = 0; i < s->n; i++) free(kp[i]);
    akaze_free(s); free(s);
    return n <= cap ? n : -n;
}
