// The Viterbi decode of include/hml.h (hml_viterbi) restated for one host thread: the fixed-point tables from block
// statistics, emission parameters, A and pi, the sequential max-plus recursion with its back-pointers, the back-track and the
// path score.  No HIP; compile with -ffp-contract=off.  The kernels of hml_k_viterbi.h must give these very words.
//
//   fx(x)        = llrint(clamp(x, -2^38, 2^38) * 2^20), NaN -> -2^38 (the product is exact; ties to even)
//   init[j]      = fx(hml_logf(pi_j)),  trans[i][j] = fx(hml_logf(A_ij))
//   emit[b][j]   = fx(E_b(j)),  E_b(j) = sum_d fl32((2.0 mu_p Sx_d - Sxx_d) / (2.0 var_p)) - N logNs_j [+ (N - 1) logA_j]
//                  in float, p = (j / P^d) % P, with logNs_j = sum_d (hml_logf(sqrtf(var_p)) + mu_p mu_p / (2 var_p)) and
//                  logA_j = hml_logf(A_jj) derived here from the parameters
//   d_0(j)       = init[j] + emit[0][j];  d_b(j) = max_i(d_{b-1}(i) + trans[i][j]) + emit[b][j], psi_b(j) the SMALLEST i that
//                  attains the maximum; max_j d_b(j) is subtracted after every block
//   q_{B-1}      = the smallest j with d_{B-1}(j) = 0,  q_{b-1} = psi_b(q_b)
//   score        = init[q_0] + sum_b emit[b][q_b] + sum_{b > 0} trans[q_{b-1}][q_b] in int64 with wrap-around
#ifndef HML_VITERBI_REF_H
#define HML_VITERBI_REF_H

#include <math.h>
#include <stdint.h>

#include <vector>

#include "hml_math.h"

#define HML_VIT_CAP_K 64
#define HML_VIT_MAX_D 4

static inline int64_t hml_vit_ref_fx(double x) {
    const double lim = 274877906944.0;   // 2^38
    if (x != x) x = -lim;
    if (x < -lim) x = -lim;
    if (x > lim) x = lim;
    return (int64_t)llrint(x * 1048576.0);   // 2^20: exact, |product| <= 2^58
}

struct hml_vit_ref_case {
    int K = 0, D = 1, P = 0, self_trans = 1;
    uint64_t B = 0;
    std::vector<uint32_t> starts;          // B + 1
    std::vector<float> sum, sum_sq;        // [D][B]
    std::vector<float> mean_var;           // 2 P: mean0, var0, mean1, ...
    std::vector<float> A, pi;              // K K row-major, K
};

// emit[B][K], trans[K][K], init[K]
static inline void hml_vit_ref_tables(const hml_vit_ref_case& c, std::vector<int64_t>& emit, std::vector<int64_t>& trans, std::vector<int64_t>& init) {
    const int K = c.K, D = c.D, P = c.P;
    init.resize(K); trans.resize((size_t)K * K); emit.resize((size_t)c.B * K);
    for (int j = 0; j < K; ++j) init[j] = hml_vit_ref_fx((double)hml_logf(c.pi[j]));
    for (int i = 0; i < K * K; ++i) trans[i] = hml_vit_ref_fx((double)hml_logf(c.A[i]));
    int map[HML_VIT_CAP_K][HML_VIT_MAX_D];
    float logNs[HML_VIT_CAP_K], logA[HML_VIT_CAP_K];
    for (int s = 0; s < K; ++s) {
        int div = 1;
        float r = 0.0f;
        for (int d = 0; d < D; ++d) {
            const int p = (s / div) % P;
            map[s][d] = p;
            div *= P;
            const float m = c.mean_var[2 * p], v = c.mean_var[2 * p + 1], sd = HML_SQRTF(v);
            r += hml_logf(sd) + m * m / (2 * v);
        }
        logNs[s] = r;
        logA[s] = hml_logf(c.A[s * K + s]);
    }
    for (uint64_t b = 0; b < c.B; ++b) {
        const float N = (float)(c.starts[b + 1] - c.starts[b]);
        for (int s = 0; s < K; ++s) {
            float r = 0.0f;
            for (int d = 0; d < D; ++d) {
                const int p = map[s][d];
                const float mu = c.mean_var[2 * p], var = c.mean_var[2 * p + 1];
                const float sx = c.sum[(uint64_t)d * c.B + b], sq = c.sum_sq[(uint64_t)d * c.B + b];
                const float ip = (float)((2.0 * (double)mu * (double)sx - (double)sq) / (2.0 * (double)var));
                r += ip;
            }
            float e = r - N * logNs[s];
            if (c.self_trans) e += (N - 1.0f) * logA[s];
            emit[b * K + s] = hml_vit_ref_fx((double)e);
        }
    }
}

// one step of the recursion: `d` (normalised, K words) over block b; psi_row[K] if given
static inline void hml_vit_ref_step(int K, const int64_t* trans, const int64_t* emit_b, int64_t* d, uint8_t* psi_row) {
    int64_t nd[HML_VIT_CAP_K];
    int64_t top = INT64_MIN;
    for (int j = 0; j < K; ++j) {
        int64_t best = d[0] + trans[j];
        int arg = 0;
        for (int i = 1; i < K; ++i) {
            const int64_t v = d[i] + trans[i * K + j];
            if (v > best) { best = v; arg = i; }
        }
        nd[j] = best + emit_b[j];
        if (psi_row) psi_row[j] = (uint8_t)arg;
        if (nd[j] > top) top = nd[j];
    }
    for (int j = 0; j < K; ++j) d[j] = nd[j] - top;
}

// the path q[B] and its score from the tables
static inline void hml_vit_ref_decode(int K, uint64_t B, const std::vector<int64_t>& emit, const std::vector<int64_t>& trans, const std::vector<int64_t>& init,
                                      std::vector<int16_t>& q, int64_t* score) {
    std::vector<uint8_t> psi((size_t)B * K, 0);
    int64_t d[HML_VIT_CAP_K];
    q.assign(B, 0);
    if (B == 0) { *score = 0; return; }
    int64_t top = INT64_MIN;
    for (int j = 0; j < K; ++j) { d[j] = init[j] + emit[j]; if (d[j] > top) top = d[j]; }
    for (int j = 0; j < K; ++j) d[j] -= top;
    for (uint64_t b = 1; b < B; ++b) hml_vit_ref_step(K, trans.data(), emit.data() + b * K, d, psi.data() + b * K);
    int s = 0;
    while (d[s] != 0) ++s;
    for (uint64_t b = B; b-- > 0;) {
        q[b] = (int16_t)s;
        if (b > 0) s = psi[b * K + s];
    }
    uint64_t sum = (uint64_t)init[q[0]];
    for (uint64_t b = 0; b < B; ++b) {
        sum += (uint64_t)emit[b * K + q[b]];
        if (b > 0) sum += (uint64_t)trans[(size_t)q[b - 1] * K + q[b]];
    }
    *score = (int64_t)sum;
}

#endif
