// The pairwise read-outs of the smoothing (hml_posterior_breaks, hml_posterior_regions, hml_posterior_pair_terms of
// include/hml.h): the definition, restated for one host thread.  No HIP; compile with -ffp-contract=off.  The kernels of
// hml_k_pairs.h must give these very words.
//
// e, alpha, beta, gamma exactly as hml_posterior_ref.h gives them; IEEE double, + x / only, no fused multiply-add; every sum
// starts from 0.0 and adds in ascending index; bad(x) is that header's predicate, n_b = starts[b + 1] - starts[b].
//
// Per boundary b = 1 ... B - 1 (between blocks b - 1 and b):
//   v(j)      = e_b(j) beta_b(j);   x(i, j) = (alpha_{b-1}(i) A_ij) v(j)                       (the E-step's terms)
//   d_b       = sum_j x(j, j);   o_b = sum_i sum_{j != i} x(i, j), i the outer and j the inner loop
//   p_b       = o_b / (d_b + o_b): the posterior probability of a change of state at position starts[b].  The off-diagonal mass
//               is summed directly, never formed as 1 - (the diagonal's share): a probability of 1e-20 stays one.
//               bad(d_b + o_b): p_b = 0.0, and the boundary is counted in pair_degenerate
//   u(j)      = sum_k A_jk v(k)                                     (the smoothing's own unnormalised backward vector)
//   r_b(j)    = (A_jj v(j)) / u(j) = p(q_b = j | q_{b-1} = j, y, theta); 0.0 if bad(u(j)) (the quotient would be 0 / 0)
// In fixed point - integers, so that a prefix sum over them is associative and no result can depend on a scan's geometry:
//   pfx_b     = llrint(p_b 2^32)
//   cost_b(j) = CAP = 1023 2^22 if bad(u(j)) or not r_b(j) > 0; else min(llrint(max(-hml_log(r_b(j)), 0) 2^22), CAP): units of
//               2^-22 nat.  hml_exp_nonpos is exactly 0 below -700, so one capped boundary makes a joint probability exactly 0
//   mass_b(j) = n_b llrint(gamma_b(j) 2^32), for b = 0 ... B - 1
// Block 0 has no boundary: p_0 = 0.0, r_0(j) = 0.0, pfx_0 = cost_0(j) = 0.  B and T are below 2^32, so a sum of costs stays
// below 2^32 2^32, a sum of pfx at or below 2^32 2^32 - 2^32 and a sum of mass at or below T 2^32: uint64 holds them.
// Inclusive prefix sums over b: N (of pfx), C_j (of cost(j)), G_j (of mass(j)).
//
// Per region [start, end) - positions, 0 <= start < end <= T:  ba = blk(start), be = blk(end - 1), blk(p) the block that holds p
//   D_j            = C_j[be] - C_j[ba]
//   whole_state[j] = gamma_ba(j) hml_exp_nonpos(-(double)D_j 2^-22): the probability that every position is in state j
//   whole          = sum_j whole_state[j]: the probability of no breakpoint inside the region
//   expected_breaks = (double)(N[be] - N[ba]) 2^-32
//   M_j            = G_j[be] - G_j[ba - 1] (0 for ba = 0) - (start - starts[ba]) fx(gamma_ba(j)) - (starts[be + 1] - end)
//                    fx(gamma_be(j)), fx(g) = llrint(g 2^32): integers throughout
//   share[j]       = ((double)M_j 2^-32) / (double)(end - start): the expected fraction of the region's positions in state j
//   raw            = N[be] - N[ba], then D_0 ... D_{K-1}, then M_0 ... M_{K-1}
// Quantisation ("pairwise read-outs"): a cost is off by at most 2^-23 nat, so whole_state by at most
// (be - ba) 2^-23 relative to first order; expected_breaks by at most (be - ba) 2^-33; share[j] by at most 2^-33.
#ifndef HML_PAIRS_REF_H
#define HML_PAIRS_REF_H

#include "hml_posterior_ref.h"

#define HML_PAIRS_COST_CAP 4290772992ull   // 1023 2^22

struct hml_pairs_ref_result {
    std::vector<double> p, r;                 // [B], [B][K]
    std::vector<uint64_t> pfx, cost, mass;    // [B], [B][K], [B][K]
    std::vector<uint64_t> N, C, G;            // [B], [K][B], [K][B]: the inclusive prefix sums
    std::vector<double> gamma;                // [B][K]
    uint64_t pair_degenerate = 0;
};

struct hml_pairs_ref_region {
    double whole = 0.0, expected_breaks = 0.0;
    std::vector<double> whole_state, share;   // [K]
    std::vector<uint64_t> raw;                // [2 K + 1]
};

// llrint(g 2^32) for 0 <= g <= 1 (the product is exact)
static inline uint64_t hml_pairs_fx32(double g) { return (uint64_t)llrint(g * 4294967296.0); }

static inline uint64_t hml_pairs_cost(double u, double r) {
    if (hml_post_ref_bad(u) || !(r > 0.0)) return HML_PAIRS_COST_CAP;
    double nl = -hml_log(r);
    nl = nl > 0.0 ? nl : 0.0;
    const uint64_t q = (uint64_t)llrint(nl * 4194304.0);   // 2^22: exact, below 2^33
    return q < HML_PAIRS_COST_CAP ? q : HML_PAIRS_COST_CAP;
}

// the terms and their prefix sums from a case (B >= 1)
static inline void hml_pairs_ref_terms(const hml_post_ref_case& c, hml_pairs_ref_result& out) {
    const int K = c.K;
    const uint64_t B = c.B;
    hml_post_ref_result s;
    hml_post_ref_tables(c, s.e, s.m);
    hml_post_ref_smooth(c, s);
    out.gamma = s.gamma;
    out.p.assign(B, 0.0); out.r.assign((size_t)B * K, 0.0);
    out.pfx.assign(B, 0); out.cost.assign((size_t)B * K, 0); out.mass.assign((size_t)B * K, 0);
    out.pair_degenerate = 0;
    std::vector<double> A((size_t)K * K), v(K);
    for (int i = 0; i < K * K; ++i) A[i] = (double)c.A[i];
    for (uint64_t b = 1; b < B; ++b) {
        const double* const prev = s.alpha.data() + (b - 1) * K;
        for (int j = 0; j < K; ++j) v[j] = (double)s.e[b * K + j] * s.beta[b * K + j];
        double d = 0.0, o = 0.0;
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) {
                const double x = (prev[i] * A[i * K + j]) * v[j];
                if (j == i) d = d + x;
                else o = o + x;
            }
        const double X = d + o;
        const bool bad = hml_post_ref_bad(X);
        if (bad) ++out.pair_degenerate;
        out.p[b] = bad ? 0.0 : o / X;
        out.pfx[b] = hml_pairs_fx32(out.p[b]);
        for (int j = 0; j < K; ++j) {
            double u = 0.0;
            for (int k = 0; k < K; ++k) u = u + A[j * K + k] * v[k];
            const double r = hml_post_ref_bad(u) ? 0.0 : (A[j * K + j] * v[j]) / u;
            out.r[b * K + j] = r;
            out.cost[b * K + j] = hml_pairs_cost(u, r);
        }
    }
    for (uint64_t b = 0; b < B; ++b) {
        const uint64_t n = (uint64_t)(c.starts[b + 1] - c.starts[b]);
        for (int j = 0; j < K; ++j) out.mass[b * K + j] = n * hml_pairs_fx32(s.gamma[b * K + j]);
    }
    out.N.assign(B, 0); out.C.assign((size_t)K * B, 0); out.G.assign((size_t)K * B, 0);
    for (uint64_t b = 0; b < B; ++b) {
        out.N[b] = (b ? out.N[b - 1] : 0) + out.pfx[b];
        for (int j = 0; j < K; ++j) {
            out.C[(uint64_t)j * B + b] = (b ? out.C[(uint64_t)j * B + b - 1] : 0) + out.cost[b * K + j];
            out.G[(uint64_t)j * B + b] = (b ? out.G[(uint64_t)j * B + b - 1] : 0) + out.mass[b * K + j];
        }
    }
}

// the last block b of [0, B) with starts[b] <= p (starts[0] = 0)
static inline uint64_t hml_pairs_block_of(const uint32_t* starts, uint64_t B, uint32_t p) {
    uint64_t lo = 0, hi = B;   // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// whether a region is one the calls accept
static inline bool hml_pairs_region_ok(uint32_t start, uint32_t end, uint64_t T) { return start < end && (uint64_t)end <= T; }

// one region from the terms (the region is valid)
static inline void hml_pairs_ref_region_of(const hml_post_ref_case& c, const hml_pairs_ref_result& t, uint32_t start, uint32_t end, hml_pairs_ref_region& out) {
    const int K = c.K;
    const uint64_t B = c.B;
    const uint64_t ba = hml_pairs_block_of(c.starts.data(), B, start), be = hml_pairs_block_of(c.starts.data(), B, end - 1u);
    out.whole_state.assign(K, 0.0); out.share.assign(K, 0.0); out.raw.assign(2 * (size_t)K + 1, 0);
    const uint64_t nb = t.N[be] - t.N[ba];
    out.raw[0] = nb;
    out.expected_breaks = (double)nb * (1.0 / 4294967296.0);
    const uint64_t cut_a = (uint64_t)(start - c.starts[ba]), cut_e = (uint64_t)(c.starts[be + 1] - end);
    const double len = (double)(end - start);
    double whole = 0.0;
    for (int j = 0; j < K; ++j) {
        const double ga = t.gamma[ba * K + j], ge = t.gamma[be * K + j];
        const uint64_t dc = t.C[(uint64_t)j * B + be] - t.C[(uint64_t)j * B + ba];
        const double ws = ga * hml_exp_nonpos(-(double)dc * (1.0 / 4194304.0));
        out.whole_state[j] = ws;
        whole = whole + ws;
        const uint64_t m = t.G[(uint64_t)j * B + be] - (ba ? t.G[(uint64_t)j * B + ba - 1] : 0) - cut_a * hml_pairs_fx32(ga) - cut_e * hml_pairs_fx32(ge);
        out.share[j] = ((double)m * (1.0 / 4294967296.0)) / len;
        out.raw[1 + j] = dc;
        out.raw[1 + K + j] = m;
    }
    out.whole = whole;
}

#endif
