// The smoothing read-out of include/hml.h (hml_posterior) restated for one host thread: the float emission tables from block
// statistics, emission parameters and A, the normalised forward and backward recursions in IEEE double, the state posteriors,
// log p(y | theta) and the call per position.  No HIP; compile with -ffp-contract=off.  The kernels of hml_k_posterior.h must
// give these very words.
//
//   weight(q)    = pi(q_0) prod_b exp E_b(q_b) prod_{b > 0} A(q_{b-1}, q_b) over the B blocks
//   E_b(j)       = the float hml_viterbi quantises (hml_viterbi_ref.h): sum_d fl32((2.0 mu_p Sx_d - Sxx_d) / (2.0 var_p))
//                  - N logNs_j [+ (N - 1) logA_j], logNs and logA derived here from the parameters
//   m_b          = max_j E_b(j) as the sweep takes it: m = lowest float; m = (E_j < m) ? m : E_j, j ascending
//   e_b(j)       = hml_expf(E_b(j) - m_b)                                                        (float)
// From here on IEEE double over exactly widened floats (pi, A, e): +, x, / in the order written, no fused multiply-add; every
// sum starts from 0.0 and adds its terms in ascending index.  "bad(x)" = x is not a positive finite number.
//   forward      a_0(j) = pi_j e_0(j);  a_b(j) = e_b(j) sum_i alpha_{b-1}(i) A_ij;  c_b = sum_j a_b(j);  alpha_b = a_b / c_b,
//                or alpha_b(j) = 1.0 / K for all j if bad(c_b): block b is then DEGENERATE (no path reaches it)
//   backward     beta_{B-1}(i) = 1.0 / K;  v(j) = e_{b+1}(j) beta_{b+1}(j);  u(i) = sum_j A_ij v(j);  s = sum_i u(i);
//                beta_b = u / s, or 1.0 / K throughout if bad(s)
//   posterior    g(i) = alpha_b(i) beta_b(i);  S = sum_i g(i);  gamma_b = g / S, or gamma_b = alpha_b if bad(S)
//   degenerate   the number of blocks with bad(c_b).  (bad(s) and bad(S) follow from a degenerate block further on - sums of
//                non-negative terms vanish only with every term - and are not counted a second time.)
//   loglik       l_b = (double)m_b + hml_log(c_b);  log p(y | theta) = the fan-in-64 tree sum of l_0 ... l_{B-1}: value i of the
//                next level is s = v[64 i]; s = s + v[64 i + 1]; ... over at most 64 consecutive values, until one is left
//   call         state_b = the smallest j at the maximum of gamma_b;  adjacent blocks of equal state form a run, whose
//                confidence is the minimum over its blocks of gamma_b(state)
#ifndef HML_POSTERIOR_REF_H
#define HML_POSTERIOR_REF_H

#include <math.h>
#include <stdint.h>

#include <vector>

#include "hml_math.h"

#define HML_POST_CAP_K 64
#define HML_POST_MAX_D 4

struct hml_post_ref_case {
    int K = 0, D = 1, P = 0, self_trans = 1;
    uint64_t B = 0;
    std::vector<uint32_t> starts;          // B + 1
    std::vector<float> sum, sum_sq;        // [D][B]
    std::vector<float> mean_var;           // 2 P: mean0, var0, mean1, ...
    std::vector<float> A, pi;              // K K row-major, K
};

struct hml_post_ref_result {
    std::vector<float> e, m;               // [B][K], [B]
    std::vector<double> alpha, c, beta, gamma;   // [B][K], [B], [B][K], [B][K]
    double loglik = 0.0;
    uint64_t degenerate = 0;
    std::vector<int16_t> state;            // [B]
    std::vector<uint64_t> run_len;         // positions
    std::vector<int32_t> run_state;
    std::vector<double> run_conf;
};

static inline bool hml_post_ref_bad(double x) { return !(x > 0.0 && x < (double)INFINITY); }

// e[B][K], m[B]
static inline void hml_post_ref_tables(const hml_post_ref_case& c, std::vector<float>& e, std::vector<float>& m) {
    const int K = c.K, D = c.D, P = c.P;
    e.resize((size_t)c.B * K); m.resize(c.B);
    int map[HML_POST_CAP_K][HML_POST_MAX_D];
    float logNs[HML_POST_CAP_K], logA[HML_POST_CAP_K], E[HML_POST_CAP_K];
    for (int s = 0; s < K; ++s) {
        int div = 1;
        float r = 0.0f;
        for (int d = 0; d < D; ++d) {
            const int p = (s / div) % P;
            map[s][d] = p;
            div *= P;
            const float mu = c.mean_var[2 * p], v = c.mean_var[2 * p + 1], sd = HML_SQRTF(v);
            r += hml_logf(sd) + mu * mu / (2 * v);
        }
        logNs[s] = r;
        logA[s] = hml_logf(c.A[s * K + s]);
    }
    for (uint64_t b = 0; b < c.B; ++b) {
        const float N = (float)(c.starts[b + 1] - c.starts[b]);
        float top = -3.40282346638528859812e+38f;
        for (int s = 0; s < K; ++s) {
            float r = 0.0f;
            for (int d = 0; d < D; ++d) {
                const int p = map[s][d];
                const float mu = c.mean_var[2 * p], var = c.mean_var[2 * p + 1];
                const float sx = c.sum[(uint64_t)d * c.B + b], sq = c.sum_sq[(uint64_t)d * c.B + b];
                const float ip = (float)((2.0 * (double)mu * (double)sx - (double)sq) / (2.0 * (double)var));
                r += ip;
            }
            float v = r - N * logNs[s];
            if (c.self_trans) v += (N - 1.0f) * logA[s];
            E[s] = v;
            top = (v < top) ? top : v;
        }
        m[b] = top;
        for (int s = 0; s < K; ++s) e[b * K + s] = hml_expf(E[s] - top);
    }
}

// alpha_b and c_b from alpha_{b-1} (prev == nullptr: block 0, from pi); returns whether the block is degenerate
static inline bool hml_post_ref_forward_step(int K, const float* A, const float* pi, const float* e_b, const double* prev, double* alpha, double* c_out) {
    double a[HML_POST_CAP_K];
    double c = 0.0;
    for (int j = 0; j < K; ++j) {
        if (!prev) a[j] = (double)pi[j] * (double)e_b[j];
        else {
            double s = 0.0;
            for (int i = 0; i < K; ++i) s = s + prev[i] * (double)A[i * K + j];
            a[j] = (double)e_b[j] * s;
        }
        c = c + a[j];
    }
    const bool bad = hml_post_ref_bad(c);
    for (int j = 0; j < K; ++j) alpha[j] = bad ? 1.0 / (double)K : a[j] / c;
    *c_out = c;
    return bad;
}

// beta_b from beta_{b+1} and e_{b+1}
static inline void hml_post_ref_backward_step(int K, const float* A, const float* e_next, const double* next, double* beta) {
    double v[HML_POST_CAP_K], u[HML_POST_CAP_K];
    for (int j = 0; j < K; ++j) v[j] = (double)e_next[j] * next[j];
    double s = 0.0;
    for (int i = 0; i < K; ++i) {
        double t = 0.0;
        for (int j = 0; j < K; ++j) t = t + (double)A[i * K + j] * v[j];
        u[i] = t;
        s = s + t;
    }
    const bool bad = hml_post_ref_bad(s);
    for (int i = 0; i < K; ++i) beta[i] = bad ? 1.0 / (double)K : u[i] / s;
}

// gamma_b; returns the called state
static inline int hml_post_ref_combine(int K, const double* alpha, const double* beta, double* gamma) {
    double g[HML_POST_CAP_K];
    double S = 0.0;
    for (int i = 0; i < K; ++i) { g[i] = alpha[i] * beta[i]; S = S + g[i]; }
    const bool bad = hml_post_ref_bad(S);
    int best = 0;
    for (int i = 0; i < K; ++i) {
        gamma[i] = bad ? alpha[i] : g[i] / S;
        if (gamma[i] > gamma[best]) best = i;
    }
    return best;
}

// the fan-in-64 tree sum (n >= 1)
static inline double hml_post_ref_tree_sum(std::vector<double> v) {
    while (v.size() > 1) {
        std::vector<double> w((v.size() + 63) / 64);
        for (size_t i = 0; i < w.size(); ++i) {
            double s = v[64 * i];
            for (size_t k = 64 * i + 1; k < 64 * i + 64 && k < v.size(); ++k) s = s + v[k];
            w[i] = s;
        }
        v.swap(w);
    }
    return v[0];
}

// everything from the tables (B >= 1)
static inline void hml_post_ref_smooth(const hml_post_ref_case& c, hml_post_ref_result& r) {
    const int K = c.K;
    const uint64_t B = c.B;
    r.alpha.assign((size_t)B * K, 0.0); r.beta.assign((size_t)B * K, 0.0); r.gamma.assign((size_t)B * K, 0.0);
    r.c.assign(B, 0.0); r.state.assign(B, 0);
    r.degenerate = 0;
    std::vector<double> ell(B);
    for (uint64_t b = 0; b < B; ++b) {
        if (hml_post_ref_forward_step(K, c.A.data(), c.pi.data(), r.e.data() + b * K, b ? r.alpha.data() + (b - 1) * K : nullptr, r.alpha.data() + b * K, &r.c[b]))
            ++r.degenerate;
        ell[b] = (double)r.m[b] + hml_log(r.c[b]);
    }
    for (int i = 0; i < K; ++i) r.beta[(B - 1) * K + i] = 1.0 / (double)K;
    for (uint64_t b = B - 1; b-- > 0;) hml_post_ref_backward_step(K, c.A.data(), r.e.data() + (b + 1) * K, r.beta.data() + (b + 1) * K, r.beta.data() + b * K);
    r.loglik = hml_post_ref_tree_sum(ell);
    r.run_len.clear(); r.run_state.clear(); r.run_conf.clear();
    for (uint64_t b = 0; b < B; ++b) {
        const int s = hml_post_ref_combine(K, r.alpha.data() + b * K, r.beta.data() + b * K, r.gamma.data() + b * K);
        r.state[b] = (int16_t)s;
        const double conf = r.gamma[b * K + s];
        const uint64_t len = c.starts[b + 1] - c.starts[b];
        if (b > 0 && r.run_state.back() == s) {
            r.run_len.back() += len;
            if (conf < r.run_conf.back()) r.run_conf.back() = conf;
        } else {
            r.run_len.push_back(len); r.run_state.push_back(s); r.run_conf.push_back(conf);
        }
    }
}

#endif
