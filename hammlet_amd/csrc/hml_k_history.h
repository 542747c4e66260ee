// The chain's HISTORY: one row of scalars per sweep - log-likelihood, log-prior, segment count, blocks, threshold - from which
// a user reads burn-in, mixing and whether the chains sit in the same mode (no counterpart in the reference; DESIGN.md 3c''''''').
// A row describes the state of the chain AFTER the sweep: the sweep's states q through their sufficient statistics (the model's
// last_occ / last_trans / last_sum / last_sumsq: the very numbers the conjugate update used, what hml_get_counts returns) under
// the theta, A and pi that the sweep's parameter update has just drawn - the convention of the level recorder (hml_k_levels.h).
// It is the complete-data log-likelihood of the compressed model, not the marginal likelihood of the filter.
// Everything the row needs is reduced by the time the parameter kernel has run, on every sweep path: no kernel of the sweep
// is touched, and this one is compiled into hml_readout.hip's object only.
#ifndef HML_K_HISTORY_H
#define HML_K_HISTORY_H

#include "hml_math.h"
#include "hml_state.h"

#define HML_HIST_COLS 11   // (= HML_HISTORY_COLS, include/hml.h)

// what the history buffer begins with; the rows (HML_HIST_COLS doubles each) follow
struct hml_history_head {
    unsigned long long n_rows;    // rows written so far: where the next one goes
    unsigned long long dropped;   // rows that found the buffer full (the host sizes it ahead of the sweeps: a bug if not 0)
    unsigned long long reserved[2];
};

// One workgroup of one wavefront, behind the sweep's parameter update (and recorders).  K and P are run-time values up to
// 64: lane p holds parameter p, lane s state s and row s of the transition counts.  All arithmetic in double on exactly widened
// floats; a product whose count or zero coefficient is 0 is 0 whatever its logarithm is (0 log 0 is no NaN), everything
// else is kept as IEEE gives it (+inf in lprior_path when a Dirichlet draw underflowed to 0 under a_off < 1).  Sums in a
// fixed order: j ascending inside a row on the row's lane, then lanes ascending on lane 0 - the same bits on every run and
// behind every sweep path.
HML_KERNEL __launch_bounds__(64) void hml_k_history(const hml_model* __restrict__ mdl, const int16_t* __restrict__ q,
                                                    hml_history_head* __restrict__ head, unsigned long long cap,
                                                    unsigned long long every, int mixture, uint32_t chain) {
    __shared__ double sh_em[64], sh_th[64], sh_ll[64], sh_lp[64], sh_lpi[64], sh_mix[64], sh_ppi[64];
    __shared__ unsigned long long sh_occ[64], sh_off[64];
    const int lane = threadIdx.x;
    // ---- the head: every value of the model is requested here, together (hml_pin, hml_common.h) ----
    uint32_t halted = mdl->halted;
    unsigned long long sweeps = mdl->sweeps;
    int32_t K = mdl->K, P = mdl->P, D = mdl->D;
    uint32_t B = mdl->B;
    float thr = mdl->thr;
    float nig[4] = {mdl->nig_prior[0], mdl->nig_prior[1], mdl->nig_prior[2], mdl->nig_prior[3]};
    float a_off = mdl->a_off, a_diag = mdl->a_diag, pi_alpha = mdl->pi_alpha;
    unsigned long long idx = head->n_rows, dropped = head->dropped;
    const int q0 = q[0];
    // (the model's arrays hold HML_CAP_K = 64 entries: a lane's element exists whatever K is)
    const float mu = mdl->mu[lane], var = mdl->var[lane], sx = mdl->last_sum[lane], sxx = mdl->last_sumsq[lane], pi = mdl->pi[lane];
    const unsigned long long occ = mdl->last_occ[lane];
    hml_pin(halted); hml_pin(sweeps); hml_pin(K); hml_pin(P); hml_pin(D); hml_pin(B); hml_pin(thr); hml_pin(nig);
    hml_pin(a_off); hml_pin(a_diag); hml_pin(pi_alpha); hml_pin(idx); hml_pin(dropped);
    if (halted != 0u) return;              // (hml_state.h: the sweep did not happen; its row is written when it runs again)
    if (sweeps % every != 0ull) return;    // not due
    if (K < 1 || K > HML_CAP_K || P < 1 || P > HML_CAP_K) return;
    sh_occ[lane] = lane < K ? occ : 0ull;
    __syncthreads();
    // ---- transitions: row `lane`, j ascending, loads in groups of eight ----
    const double c_off = (double)a_off - 1.0, c_diag = (double)a_diag - 1.0, c_pi = (double)pi_alpha - 1.0;
    double row_ll = 0.0, row_lp = 0.0;
    unsigned long long row_off = 0ull;
    for (int j0 = 0; j0 < K; j0 += 8) {
        float a[8];
        unsigned long long n[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = lane < K && j0 + u < K;
            a[u] = in ? mdl->A[lane * K + j0 + u] : 1.0f;
            n[u] = in ? mdl->last_trans[lane * K + j0 + u] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = lane < K && j0 + u < K;
            if (!in) continue;
            const double lg = hml_log((double)a[u]);
            const double cf = (j0 + u == lane) ? c_diag : c_off;
            if (n[u] != 0ull) row_ll = row_ll + (double)n[u] * lg;
            if (cf != 0.0) row_lp = row_lp + cf * lg;
            if (j0 + u != lane) row_off += n[u];
        }
    }
    sh_ll[lane] = row_ll; sh_lp[lane] = row_lp; sh_off[lane] = row_off;
    // ---- states: log pi ----
    {
        const double lpi = lane < K ? hml_log((double)pi) : 0.0;
        sh_lpi[lane] = lpi;
        sh_mix[lane] = (lane < K && occ != 0ull) ? (double)occ * lpi : 0.0;
        sh_ppi[lane] = (lane < K && c_pi != 0.0) ? c_pi * lpi : 0.0;
    }
    // ---- parameters: emission terms and the prior of theta ----
    {
        // n_p: the (position, dimension) terms that use parameter p - the occupancy of state p when D = 1
        unsigned long long np = 0ull;
        if (D == 1) np = lane < K ? occ : 0ull;
        else if (lane < P)
            for (int s = 0; s < K; ++s)
                for (int d = 0; d < D && d < HML_MAX_D; ++d) if (mdl->map[s][d] == lane) np += sh_occ[s];
        double em = 0.0, th = 0.0;
        if (lane < P) {
            const double m = (double)mu, v = (double)var, n = (double)np;
            const double lv = hml_log(v);
            const double two_pi = 6.283185307179586476925286766559;
            if (np != 0ull) em = 0.5 * n * hml_log(two_pi * v);
            const double nmm = np != 0ull ? n * m * m : 0.0;
            em = em + (((double)sxx - 2.0 * m * (double)sx) + nmm) / (2.0 * v);
            const double alpha = (double)nig[0], beta = (double)nig[1], mu0 = (double)nig[2], nu = (double)nig[3];
            th = -(alpha + 1.0) * lv - beta / v - 0.5 * lv - nu * (m - mu0) * (m - mu0) / (2.0 * v);
        }
        sh_em[lane] = em; sh_th[lane] = th;
    }
    __syncthreads();
    if (lane != 0) return;
    if (idx >= cap) { head->dropped = dropped + 1ull; return; }   // nothing at or beyond the capacity
    double ll_emit = 0.0, lprior_theta = 0.0;
    for (int p = 0; p < P; ++p) { ll_emit = ll_emit + sh_em[p]; lprior_theta = lprior_theta + sh_th[p]; }
    double ll_path = 0.0, lprior_path = 0.0;
    unsigned long long off = 0ull, used = 0ull;
    if (mixture) { for (int s = 0; s < K; ++s) ll_path = ll_path + sh_mix[s]; }
    else {
        ll_path = (q0 >= 0 && q0 < K) ? sh_lpi[q0] : 0.0;
        for (int i = 0; i < K; ++i) ll_path = ll_path + sh_ll[i];
    }
    for (int i = 0; i < K; ++i) { lprior_path = lprior_path + sh_lp[i]; off += sh_off[i]; used += sh_occ[i] != 0ull ? 1ull : 0ull; }
    for (int s = 0; s < K; ++s) lprior_path = lprior_path + sh_ppi[s];
    double* const row = reinterpret_cast<double*>(head + 1) + idx * (unsigned long long)HML_HIST_COLS;
    row[0] = (double)sweeps;
    row[1] = mixture ? 1.0 : 0.0;
    row[2] = -ll_emit;
    row[3] = ll_path;
    row[4] = lprior_theta;
    row[5] = lprior_path;
    row[6] = (double)(1ull + off);
    row[7] = (double)B;
    row[8] = (double)used;
    row[9] = (double)thr;
    row[10] = (double)chain;
    head->n_rows = idx + 1ull;
}

#endif
