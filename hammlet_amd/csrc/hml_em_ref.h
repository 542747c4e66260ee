// Expectation-maximisation over the current blocks (hml_expected_counts, hml_em_step, hml_em_fit of include/hml.h): the
// definition, restated for one host thread.  No HIP; compile with -ffp-contract=off.  The kernels of hml_k_em.h must give the
// E-step's very words; the M-step and the objective below are the functions the library itself calls.
//
// E-step.  e, alpha, beta, gamma, loglik and degenerate exactly as hml_posterior_ref.h gives them.  IEEE double, + x / only, no
// fused multiply-add.  "tree" is that header's fan-in-64 tree sum (value i of the next level is s = v[64 i]; s = s + v[64 i + 1];
// ...), bad(x) its predicate, n_b = (double)(starts[b + 1] - starts[b]).
//   for b = 1 ... B - 1:   v(j) = e_b(j) beta_b(j);  x(i, j) = (alpha_{b-1}(i) A_ij) v(j);
//                          X_b = sum_i sum_j x(i, j), from 0.0, i the outer and j the inner loop;
//                          xi_b(i, j) = x(i, j) / X_b (a division), or 0.0 for all (i, j) if bad(X_b): counted in xi_degenerate
//   xi[i][j]   = tree over b = 1 ... B - 1 of xi_b(i, j) (B - 1 leaves); 0.0 when B = 1
//   first[j]   = gamma_0(j)
//   occ[j]     = tree_b(n_b gamma_b(j))                     (B leaves, as in the three below)
//   stay[j]    = tree_b((n_b - 1.0) gamma_b(j))
//   sx[j][d]   = tree_b(gamma_b(j) (double)Sx_{d,b}),  sxx[j][d] the same with Sxx
// This is the exact E-step of the path weight include/hml.h states for smoothing, pi(q_0) prod exp E_b(q_b) prod A(q_{b-1}, q_b):
// with self-transitions on, (N - 1) log A_jj lies inside E_b, and `stay` is its expected count.
// It is NOT the sampler's count pass: the reference's sweep feeds pi's posterior the full occupancies and books a 0 -> state
// transition for the first block; EM of the weight above takes pi from the first block alone and books no such transition.
//
// M-step (hml_em_mstep).  Per emission parameter p, fold occ, sx, sxx over the (state, dimension) pairs that map to p (ascending
// state, then ascending dimension; the mapping of hml_post_ref_tables): n, S, Q from 0.0.  ss = Q - S S / n, raised to 0.0 if
// negative.
//   use_prior = 0:  mu = S / n;  var = ss / n
//   use_prior = 1:  mu = (nu mu0 + S) / (nu + n);
//                   var = (beta + ss / 2 + (n nu / (n + nu)) (S / n - mu0)^2 / 2) / (alpha + n / 2 + 1.5)
//                   - the joint mode of the normal-inverse-gamma posterior, in the convention of the sweep's parameter kernel
// A parameter keeps its old pair (and is counted in `kept`) if bad(n) or if the values rounded to float are not a finite mean and
// a positive finite variance.
//   rows of A:  r_ij = xi[i][j] + (i == j and self-transitions on ? stay[j] : 0) + (use_prior ? a_ij - 1 : 0), a_ij = a_diag on
//               the diagonal and a_off elsewhere; negative r_ij raised to 0.0; R_i = sum_j r_ij; A_ij = r_ij / R_i; bad(R_i): the
//               row is kept and counted
//   pi:         the same from first and pi_alpha
// Everything is rounded to float.
//
// Objective (hml_em_objective), of float parameters: loglik, and with use_prior = 1 plus
//   sum_p [-(alpha + 1.5) log var_p - beta / var_p - nu (mu_p - mu0)^2 / (2 var_p)] + sum_ij (a_ij - 1) log A_ij
//   + (pi_alpha - 1) sum_j log pi_j,   every term whose exponent a - 1 is exactly 0 skipped, log = hml_log on doubles.
//
// Fit (hml_em_ref_fit).  trace[k] = the objective of the parameters after k M-steps.  Before M-step k + 1 the fit stops if the
// E-step reports degenerate + xi_degenerate > 0 (HML_EM_DEGENERATE), if k >= 1 and trace[k] - trace[k-1] <= rel_tol |trace[k-1]|
// (HML_EM_CONVERGED), or if k == max_steps (HML_EM_MAX_STEPS), tested in this order.  Blocks are never rebuilt.
#ifndef HML_EM_REF_H
#define HML_EM_REF_H

#include "hml_posterior_ref.h"

#ifndef HML_EM_MAX_STEPS
#define HML_EM_MAX_STEPS 0
#define HML_EM_CONVERGED 1
#define HML_EM_DEGENERATE 2
#endif

struct hml_em_counts {
    std::vector<double> xi, first, stay, occ, sx, sxx;   // [K][K], [K], [K], [K], [K][D], [K][D]
    double loglik = 0.0;
    uint64_t degenerate = 0, xi_degenerate = 0;
};

// the chain's priors (hml_set_model), widened exactly
struct hml_em_prior {
    double alpha = 0.0, beta = 0.0, mu0 = 0.0, nu = 0.0;
    double a_off = 1.0, a_diag = 1.0, pi_alpha = 1.0;
};

// the fan-in-64 tree sum of a stream of values, without keeping them
struct hml_em_tree {
    enum { LEVELS = 12 };
    double part[LEVELS];
    uint32_t cnt[LEVELS];
    hml_em_tree() { for (int l = 0; l < LEVELS; ++l) { part[l] = 0.0; cnt[l] = 0; } }
    void add(double v, int l = 0) {
        part[l] = cnt[l] ? part[l] + v : v;
        if (++cnt[l] == 64u) { cnt[l] = 0; add(part[l], l + 1); }
    }
    // (0.0 for no values)
    double finish() {
        for (int l = 0; l < LEVELS; ++l) {
            if (!cnt[l]) continue;
            bool above = false;
            for (int h = l + 1; h < LEVELS; ++h) above = above || cnt[h] != 0;
            if (!above) return part[l];
            const double v = part[l];
            cnt[l] = 0;
            add(v, l + 1);
        }
        return 0.0;
    }
};

static inline int hml_em_ref_map(int s, int d, int P) {
    int div = 1;
    for (int k = 0; k < d; ++k) div *= P;
    return (s / div) % P;
}

// the E-step from a case (B >= 1)
static inline void hml_em_ref_estep(const hml_post_ref_case& c, hml_em_counts& out) {
    const int K = c.K, D = c.D;
    const uint64_t B = c.B;
    hml_post_ref_result r;
    hml_post_ref_tables(c, r.e, r.m);
    hml_post_ref_smooth(c, r);
    out.loglik = r.loglik;
    out.degenerate = r.degenerate;
    out.xi_degenerate = 0;
    std::vector<hml_em_tree> t_xi((size_t)K * K), t_occ(K), t_stay(K), t_sx((size_t)K * D), t_sxx((size_t)K * D);
    std::vector<double> A((size_t)K * K), x((size_t)K * K), v(K);
    for (int i = 0; i < K * K; ++i) A[i] = (double)c.A[i];
    for (uint64_t b = 1; b < B; ++b) {
        const double* const prev = r.alpha.data() + (b - 1) * K;
        for (int j = 0; j < K; ++j) v[j] = (double)r.e[b * K + j] * r.beta[b * K + j];
        double X = 0.0;
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) {
                x[i * K + j] = (prev[i] * A[i * K + j]) * v[j];
                X = X + x[i * K + j];
            }
        const bool bad = hml_post_ref_bad(X);
        if (bad) ++out.xi_degenerate;
        for (int i = 0; i < K * K; ++i) t_xi[i].add(bad ? 0.0 : x[i] / X);
    }
    for (uint64_t b = 0; b < B; ++b) {
        const double n = (double)(c.starts[b + 1] - c.starts[b]);
        for (int j = 0; j < K; ++j) {
            const double g = r.gamma[b * K + j];
            t_occ[j].add(n * g);
            t_stay[j].add((n - 1.0) * g);
            for (int d = 0; d < D; ++d) {
                t_sx[j * D + d].add(g * (double)c.sum[(uint64_t)d * B + b]);
                t_sxx[j * D + d].add(g * (double)c.sum_sq[(uint64_t)d * B + b]);
            }
        }
    }
    out.xi.resize((size_t)K * K); out.first.resize(K); out.stay.resize(K); out.occ.resize(K);
    out.sx.resize((size_t)K * D); out.sxx.resize((size_t)K * D);
    for (int i = 0; i < K * K; ++i) out.xi[i] = t_xi[i].finish();
    for (int j = 0; j < K; ++j) {
        out.first[j] = r.gamma[j];
        out.occ[j] = t_occ[j].finish();
        out.stay[j] = t_stay[j].finish();
    }
    for (int i = 0; i < K * D; ++i) { out.sx[i] = t_sx[i].finish(); out.sxx[i] = t_sxx[i].finish(); }
}

// The M-step: mean_var[2 P], A[K K], pi[K] are the current float parameters and are replaced; returns the number of parameters
// and rows kept.
static inline uint64_t hml_em_mstep(int K, int D, int P, int self_trans, int use_prior, const hml_em_prior& pr, const hml_em_counts& n,
                                    float* mean_var, float* A, float* pi) {
    uint64_t kept = 0;
    for (int p = 0; p < P; ++p) {
        double cnt = 0.0, S = 0.0, Q = 0.0;
        for (int s = 0; s < K; ++s)
            for (int d = 0; d < D; ++d)
                if (hml_em_ref_map(s, d, P) == p) {
                    cnt = cnt + n.occ[s];
                    S = S + n.sx[s * D + d];
                    Q = Q + n.sxx[s * D + d];
                }
        if (hml_post_ref_bad(cnt)) { ++kept; continue; }
        double ss = Q - S * S / cnt;
        if (ss < 0.0) ss = 0.0;
        double mu, var;
        if (!use_prior) {
            mu = S / cnt;
            var = ss / cnt;
        } else {
            const double dx = S / cnt - pr.mu0;
            mu = (pr.nu * pr.mu0 + S) / (pr.nu + cnt);
            var = (pr.beta + ss / 2.0 + (cnt * pr.nu / (cnt + pr.nu)) * (dx * dx) / 2.0) / (pr.alpha + cnt / 2.0 + 1.5);
        }
        const float fm = (float)mu, fv = (float)var;
        if (!(fm - fm == 0.0f) || !(fv > 0.0f && fv < INFINITY)) { ++kept; continue; }
        mean_var[2 * p] = fm;
        mean_var[2 * p + 1] = fv;
    }
    double row[HML_POST_CAP_K];
    for (int i = 0; i <= K; ++i) {   // the rows of A, then pi
        const bool is_pi = i == K;
        double R = 0.0;
        for (int j = 0; j < K; ++j) {
            double r = is_pi ? n.first[j] : n.xi[i * K + j];
            if (!is_pi && i == j && self_trans) r = r + n.stay[j];
            if (use_prior) r = r + ((is_pi ? pr.pi_alpha : (i == j ? pr.a_diag : pr.a_off)) - 1.0);
            if (r < 0.0) r = 0.0;
            row[j] = r;
            R = R + r;
        }
        if (hml_post_ref_bad(R)) { ++kept; continue; }
        for (int j = 0; j < K; ++j) (is_pi ? pi[j] : A[i * K + j]) = (float)(row[j] / R);
    }
    return kept;
}

static inline double hml_em_objective(int K, int P, int use_prior, const hml_em_prior& pr, double loglik, const float* mean_var, const float* A,
                                      const float* pi) {
    if (!use_prior) return loglik;
    double t = 0.0;
    for (int p = 0; p < P; ++p) {
        const double mu = (double)mean_var[2 * p], var = (double)mean_var[2 * p + 1], dm = mu - pr.mu0;
        t = t + ((-(pr.alpha + 1.5) * hml_log(var) - pr.beta / var) - pr.nu * (dm * dm) / (2.0 * var));
    }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            const double a1 = (i == j ? pr.a_diag : pr.a_off) - 1.0;
            if (a1 != 0.0) t = t + a1 * hml_log((double)A[i * K + j]);
        }
    const double p1 = pr.pi_alpha - 1.0;
    if (p1 != 0.0) {
        double u = 0.0;
        for (int j = 0; j < K; ++j) u = u + hml_log((double)pi[j]);
        t = t + p1 * u;
    }
    return loglik + t;
}

// whether the fit stops before M-step k + 1, and why: prev = trace[k - 1] (unused for k = 0), cur = trace[k]
static inline bool hml_em_stops(double prev, double cur, uint64_t k, uint64_t max_steps, double rel_tol, uint64_t n_degenerate, int* reason) {
    if (n_degenerate > 0) { *reason = HML_EM_DEGENERATE; return true; }
    if (k >= 1 && cur - prev <= rel_tol * fabs(prev)) { *reason = HML_EM_CONVERGED; return true; }
    if (k >= max_steps) { *reason = HML_EM_MAX_STEPS; return true; }
    return false;
}

// the fit on a case, whose parameters it replaces; trace receives steps + 1 values; kept sums over the M-steps
static inline void hml_em_ref_fit(hml_post_ref_case& c, int use_prior, const hml_em_prior& pr, uint64_t max_steps, double rel_tol, std::vector<double>& trace,
                                  uint64_t* steps, int* reason, uint64_t* kept) {
    trace.clear();
    *kept = 0;
    for (uint64_t k = 0;; ++k) {
        hml_em_counts n;
        hml_em_ref_estep(c, n);
        trace.push_back(hml_em_objective(c.K, c.P, use_prior, pr, n.loglik, c.mean_var.data(), c.A.data(), c.pi.data()));
        if (hml_em_stops(k ? trace[k - 1] : 0.0, trace[k], k, max_steps, rel_tol, n.degenerate + n.xi_degenerate, reason)) { *steps = k; return; }
        *kept += hml_em_mstep(c.K, c.D, c.P, c.self_trans, use_prior, pr, n, c.mean_var.data(), c.A.data(), c.pi.data());
    }
}

#endif
