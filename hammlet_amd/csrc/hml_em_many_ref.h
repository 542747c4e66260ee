// EM from many starts (hml_em_fit_many, hml_em_starts of include/hml.h): what is defined beside a single fit.  No HIP; compile
// with -ffp-contract=off.  The library calls these very functions.
//
// A member.  Member r of a batch is hml_set_parameters(start_r) followed by hml_em_fit on the same context, word for word:
// hml_em_ref.h and hml_posterior_ref.h are its restatement, and nothing here adds arithmetic to it.
//
// The winner (hml_em_many_best).  The candidates are the members whose reason is not HML_EM_DEGENERATE and whose objective - the
// last trace entry - is finite; the winner is the candidate with the greatest objective, the smallest index among equals; -1
// without a candidate.
//
// Starts (hml_em_many_starts).  Member 0 is the current parameters.  For r >= 1, with P emission parameters, current means mu_p
// and variances var_p (floats, widened exactly), IEEE double, + x / and sqrt only:
//   u_k    = ((double)w + 0.5) 2^-32,  w = word 0 of hml_philox4x32_10(counter (k, r, 0x454D5354, 0), key (seed low, seed high)),
//            k = 0 ... 2 P - 1
//   lo, hi = the least and the greatest mu_p;  c = (lo + hi) / 2;  h = max((hi - lo) / 2, sqrt(max_p var_p));
//   vbar   = (var_0 + var_1 + ... in ascending p, from 0.0) / P
//   mu'_p  = (float)(c + (spread h) (2 u_p - 1)), then the P means sorted ascending as floats: states come out ordered by level,
//            so members do not differ by a permutation of labels
//   var'_p = (float)(vbar (0.25 + 1.75 u_{P+p}))
// A and pi are the current ones for every member.  spread must be finite and positive.
#ifndef HML_EM_MANY_REF_H
#define HML_EM_MANY_REF_H

#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "hml_philox.h"

#ifndef HML_EM_MAX_STEPS
#define HML_EM_MAX_STEPS 0
#define HML_EM_CONVERGED 1
#define HML_EM_DEGENERATE 2
#endif

#define HML_EM_MANY_MAX_R 4096u
#define HML_EM_STARTS_TAG 0x454D5354u   // "EMST"

static inline int64_t hml_em_many_best(uint64_t R, const int* reason, const double* objective) {
    int64_t best = -1;
    for (uint64_t r = 0; r < R; ++r) {
        const double o = objective[r];
        if (reason[r] == HML_EM_DEGENERATE || !(o - o == 0.0)) continue;
        if (best < 0 || o > objective[best]) best = (int64_t)r;
    }
    return best;
}

static inline double hml_em_many_uniform(uint64_t seed, uint32_t k, uint32_t r) {
    const hml_u32x4 w = hml_philox4x32_10(k, r, HML_EM_STARTS_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((double)w.v[0] + 0.5) * (1.0 / 4294967296.0);
}

// cur_mean_var[2 P], cur_A[K K], cur_pi[K] -> mean_var[R][2 P], A[R][K K], pi[R][K]; false if spread is refused
static inline bool hml_em_many_starts(int K, int P, uint64_t R, uint64_t seed, double spread, const float* cur_mean_var, const float* cur_A, const float* cur_pi,
                                      float* mean_var, float* A, float* pi) {
    if (!(spread > 0.0) || !(spread - spread == 0.0)) return false;
    double lo = (double)cur_mean_var[0], hi = lo, vmax = (double)cur_mean_var[1], vsum = 0.0;
    for (int p = 0; p < P; ++p) {
        const double m = (double)cur_mean_var[2 * p], v = (double)cur_mean_var[2 * p + 1];
        lo = m < lo ? m : lo;
        hi = m > hi ? m : hi;
        vmax = v > vmax ? v : vmax;
        vsum = vsum + v;
    }
    const double c = (lo + hi) / 2.0, half = (hi - lo) / 2.0, dev = sqrt(vmax);
    const double h = half > dev ? half : dev;
    const double vbar = vsum / (double)P;
    for (uint64_t r = 0; r < R; ++r) {
        float* const mv = mean_var + r * 2u * (uint64_t)P;
        if (r == 0) {
            for (int i = 0; i < 2 * P; ++i) mv[i] = cur_mean_var[i];
        } else {
            float mean[HML_CAP_K];
            for (int p = 0; p < P; ++p) {
                const double u = hml_em_many_uniform(seed, (uint32_t)p, (uint32_t)r), w = hml_em_many_uniform(seed, (uint32_t)(P + p), (uint32_t)r);
                mean[p] = (float)(c + (spread * h) * (2.0 * u - 1.0));
                mv[2 * p + 1] = (float)(vbar * (0.25 + 1.75 * w));
            }
            std::sort(mean, mean + P);
            for (int p = 0; p < P; ++p) mv[2 * p] = mean[p];
        }
        if (A) for (int i = 0; i < K * K; ++i) A[r * (uint64_t)K * K + i] = cur_A[i];
        if (pi) for (int i = 0; i < K; ++i) pi[r * (uint64_t)K + i] = cur_pi[i];
    }
    return true;
}

#endif
