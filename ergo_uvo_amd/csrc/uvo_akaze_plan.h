// uvo_akaze_plan.h -- host only: the level plan of AKAZE's non-linear scale space (Allocate_Memory_Evolution of AKAZEFeatures.cpp and
// fed.cpp's fed_tau_by_process_time, as far as they can be recalled), for akaze.hip and for tests/cpp/akaze_plan_host.cpp, which prints
// it on a CPU.  omax and nsublevels are AKAZE::create's nOctaves and nOctaveLayers (uvo_akaze_configure); the arithmetic is float, in
// the reference's order.
#pragma once
#include "uvo_math.h"
#include <math.h>

namespace uvo {

static const int kAkPlanMaxLevels = 16, kAkPlanMaxSteps = 64;       // what a plan may hold: levels, FED steps of one cycle (AkLevel::tau)
enum { AK_PLAN_TOO_MANY_LEVELS = -1, AK_PLAN_CYCLE_TOO_LONG = -2 };  // akaze_plan's refusals
struct AkLevel { int w, h, octave, sublevel, sigma_size, border, nsteps; float esigma, etime, octave_ratio; float tau[kAkPlanMaxSteps]; };

// ---- fed.cpp: fed_tau_by_process_time(T, 1, 0.25f, true, tau) ----
static inline bool fed_is_prime(int number)
{
    if (number <= 1) return false;
    if (number == 1 || number == 2 || number == 3 || number == 5 || number == 7) return true;
    if ((number % 2) == 0 || (number % 3) == 0 || (number % 5) == 0 || (number % 7) == 0) return false;
    int upperLimit = (int)sqrt(1.0f + number), divisor = 11;
    while (divisor <= upperLimit) { if (number % divisor == 0) return false; divisor += 2; }
    return true;
}
// the cycle's step count; tau[0, n) is written only when n <= cap (a longer cycle is the caller's to refuse)
static inline int fed_tau(float T, float tau_max, float* tau, int cap)
{
    const float t = T / 1.0f;
    const int n = cv_ceil_d((double)(sqrtf(3.0f * t / tau_max + 0.25f) - 0.5f - 1.0e-8f));
    const float scale = 3.0f * t / (tau_max * (float)(n * (n + 1)));
    if (n <= 0) return 0;
    if (n > cap || n > kAkPlanMaxSteps) return n;
    float tauh[kAkPlanMaxSteps];
    const float c = 1.0f / (4.0f * (float)n + 2.0f), d = scale * tau_max / 2.0f;
    for (int k = 0; k < n; ++k) { const float hh = cosf((float)3.14159265358979323846 * (2.0f * (float)k + 1.0f) * c); tauh[k] = d / (hh * hh); }
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
// Allocate_Memory_Evolution: the number of levels written to L[0, kAkPlanMaxLevels), or AK_PLAN_TOO_MANY_LEVELS (nothing past the table is
// written) or AK_PLAN_CYCLE_TOO_LONG (a FED cycle of more than kAkPlanMaxSteps steps: with at most 4 octaves the longest has 31)
static inline int akaze_plan(int img_w, int img_h, int omax, int nsublevels, AkLevel* L)
{
    const float soffset = 1.6f, derivative_factor = 1.5f, smax = 10.0f * sqrtf(2.0f);
    int n = 0;
    for (int i = 0, power = 1; i <= omax - 1; i++, power *= 2) {
        const float rfactor = 1.0f / power;
        const int level_height = (int)(img_h * rfactor), level_width = (int)(img_w * rfactor);
        if ((level_width < 80 || level_height < 40) && i != 0) break;
        for (int j = 0; j < nsublevels; j++) {
            if (n >= kAkPlanMaxLevels) return AK_PLAN_TOO_MANY_LEVELS;
            AkLevel* s = &L[n++];
            s->w = level_width; s->h = level_height;
            s->esigma = soffset * powf(2.f, (float)(j) / (float)(nsublevels) + i);
            s->sigma_size = cv_round_f(s->esigma * derivative_factor / power);
            s->etime = 0.5f * (s->esigma * s->esigma);
            s->octave = i; s->sublevel = j; s->octave_ratio = (float)power;
            s->border = cv_round_f(smax * s->sigma_size) + 1;
            s->nsteps = 0;
        }
    }
    for (int i = 1; i < n; i++) {
        L[i].nsteps = fed_tau(L[i].etime - L[i - 1].etime, 0.25f, L[i].tau, kAkPlanMaxSteps);
        if (L[i].nsteps > kAkPlanMaxSteps) return AK_PLAN_CYCLE_TOO_LONG;
    }
    return n;
}

}  // namespace uvo
