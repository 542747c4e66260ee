// The count read-outs of the smoothing (hml_posterior_region_counts, hml_posterior_count_terms of include/hml.h): per region
// the exact distribution of the number of breakpoints inside it and, per state, the probability that no position of it is in
// that state - the definition, restated for one host thread.  No HIP; compile with -ffp-contract=off.  The kernels of
// hml_k_counts.h must give these very words.
//
// Under fixed parameters the posterior over paths is itself a Markov chain over the blocks, with the transitions
//   p(q_b = j | q_{b-1} = i, y, theta) = A_ij v_b(j) / u_b(i)
// that the pairwise read-outs form (hml_pairs_ref.h).  Both questions are forward recursions over the region's blocks on those
// transitions: the number of breakpoints so far as a second index, or one state struck out.  No draws, no Monte-Carlo error.
//
// e, alpha, beta, gamma exactly as hml_posterior_ref.h gives them; IEEE double, + x / only, no fused multiply-add; every sum
// starts from 0.0 and adds in ascending index; bad(x) is that header's predicate.
//
// Per boundary b = 1 ... B - 1 (between blocks b - 1 and b):
//   v_b(j)   = (double)e_b(j) beta_b(j);   u_b(i) = sum_k A_ik v_b(k)                  (the v and u of hml_pairs_ref.h)
//   rho_b(i) = 1.0 / u_b(i); if u_b(i) is not a finite number of at least 2^-1000: rho_b(i) = 0.0 and the pair (b, i) is counted
//              in count_degenerate - the mass that leaves state i there is lost, not turned into a not-a-number.  (That is
//              bad(u_b(i)) and, with it, a u_b(i) so small that its reciprocal could overflow a later product: a state whose
//              every continuation has underflowed holds no posterior mass worth the name.)
//   After u_b is formed, a v_b(j) that is not a finite non-negative number - e_b(j) is a not-a-number, or infinite beside one -
//   is replaced by 0.0: every u_b(i), formed from it, has then made rho_b(i) = 0.0 already, and the boundary passes no mass.
// Block 0 has no boundary: v_0(j) = rho_0(j) = 0.0.
// So rho_b <= 2^1000 and v_b is finite, and v_b <= 1 wherever some rho_b is not 0; a cell stays at or below 1 up to rounding, so
// no product or sum below can overflow, and none can be 0 x infinity.
//
// Per region [start, end) - positions, 0 <= start < end <= T:  ba = blk(start), be = blk(end - 1) as in hml_pairs_ref.h;
// H = max_breaks, 1 <= H <= 32 and K (H + 1) <= 1024.
//   count cells f(j, h), j a state, h = 0 ... H:
//     start   f(j, 0) = gamma_ba(j) (the degenerate fall-back to alpha_ba included); f(j, h > 0) = 0.0
//     step    for b = ba + 1 ... be:  phi(i, h) = f(i, h) rho_b(i);
//             src(i, h) = phi(i, h - 1) for 1 <= h < H;  src(i, H) = phi(i, H - 1) + phi(i, H): the last bin absorbs - "H or more";
//             s(j, 0) = 0.0;  s(j, h) = sum_{i != j} A_ij src(i, h) for h >= 1;
//             f'(j, h) = (A_jj phi(j, h) + s(j, h)) v_b(j)
//     read    hist[h] = sum_j f(j, h): the probability of exactly h breakpoints inside the region (h = H: of H or more);
//             whole_state[j] = f(j, 0): all of it in state j - the unquantised sibling of hml_posterior_regions' value
//   avoidance cells g_x(i) per struck-out state x:
//     start   g_x(i) = gamma_ba(i) for i != x; g_x(x) = 0.0
//     step    g'_x(i) = (sum_{k != x} A_ki (g_x(k) rho_b(k))) v_b(i) for i != x; g'_x(x) = 0.0
//     read    avoid[x] = sum_{i != x} g_x(i): the posterior probability that no position of the region is in state x
// The probability that the region touches x is 1 - avoid[x], which that subtraction gives exact to 2^-53 absolute; a small
// avoid[x] itself keeps its full relative precision.  Every operation is on non-negative numbers, so nothing cancels: the
// relative error of a cell is bounded by its chain's operation count times 2^-53.  Without degenerate boundaries sum_h hist[h]
// = 1 up to that rounding; with them the shortfall is the lost mass.  No output holds a not-a-number.
//
// Cost: a region is a serial chain of be - ba steps of K^2 (H + 1) and K^3 multiply-adds.  The call is meant for many regions of
// gene or segment size; one region over a whole trace of 10^6 blocks is legal and slow.
#ifndef HML_COUNTS_REF_H
#define HML_COUNTS_REF_H

#include "hml_pairs_ref.h"   // (the block of a position, the check of a region; it brings hml_posterior_ref.h)

#define HML_COUNTS_MAX_H 32u
#define HML_COUNTS_MAX_CELLS 1024u   // K (H + 1): 32 breakpoints up to 31 states, 15 at 64
#define HML_COUNTS_SLICE 16          // struck-out states a workgroup of the avoidance walk holds

// whether max_breaks is one the call accepts for K states
static inline bool hml_counts_h_ok(int K, uint32_t H) { return H >= 1u && H <= HML_COUNTS_MAX_H && (uint64_t)K * (H + 1u) <= HML_COUNTS_MAX_CELLS; }
#define HML_COUNTS_H_RULE "max_breaks must be 1 ... 32 with K (max_breaks + 1) <= 1024"

// whether rho = 1.0 / u is taken: u is a finite number of at least 2^-1000
#define HML_COUNTS_U_MIN 0x1p-1000
#define HML_COUNTS_INF __builtin_inf()
#if defined(__HIPCC__)
#define HML_COUNTS_HD static __host__ __device__ inline
#else
#define HML_COUNTS_HD static inline
#endif
HML_COUNTS_HD bool hml_counts_u_ok(double u) { return u >= HML_COUNTS_U_MIN && u < HML_COUNTS_INF; }
// v as the walks use it: itself if it is a finite non-negative number, else 0.0
HML_COUNTS_HD double hml_counts_v_kept(double v) { return (v >= 0.0 && v < HML_COUNTS_INF) ? v : 0.0; }

struct hml_counts_ref_terms {
    std::vector<double> v, rho, gamma;   // [B][K] each
    uint64_t count_degenerate = 0;
};

struct hml_counts_ref_region {
    std::vector<double> hist, whole_state, avoid;   // [H + 1], [K], [K]
};

// the terms from a case (B >= 1)
static inline void hml_counts_ref_terms_of(const hml_post_ref_case& c, hml_counts_ref_terms& out) {
    const int K = c.K;
    const uint64_t B = c.B;
    hml_post_ref_result s;
    hml_post_ref_tables(c, s.e, s.m);
    hml_post_ref_smooth(c, s);
    out.gamma = s.gamma;
    out.v.assign((size_t)B * K, 0.0); out.rho.assign((size_t)B * K, 0.0);
    out.count_degenerate = 0;
    for (uint64_t b = 1; b < B; ++b) {
        double* const v = out.v.data() + b * K;
        for (int j = 0; j < K; ++j) v[j] = (double)s.e[b * K + j] * s.beta[b * K + j];
        for (int i = 0; i < K; ++i) {
            double u = 0.0;
            for (int k = 0; k < K; ++k) u = u + (double)c.A[i * K + k] * v[k];
            const bool ok = hml_counts_u_ok(u);
            if (!ok) ++out.count_degenerate;
            out.rho[b * K + i] = ok ? 1.0 / u : 0.0;
        }
        for (int j = 0; j < K; ++j) v[j] = hml_counts_v_kept(v[j]);
    }
}

// one region from the terms (the region is valid, H is accepted)
static inline void hml_counts_ref_region_of(const hml_post_ref_case& c, const hml_counts_ref_terms& t, uint32_t start, uint32_t end, uint32_t H,
                                            hml_counts_ref_region& out) {
    const int K = c.K;
    const uint64_t ba = hml_pairs_block_of(c.starts.data(), c.B, start), be = hml_pairs_block_of(c.starts.data(), c.B, end - 1u);
    const size_t W = (size_t)H + 1;
    std::vector<double> A((size_t)K * K), f((size_t)K * W, 0.0), nf((size_t)K * W), g((size_t)K * K, 0.0), ng((size_t)K * K);
    for (int i = 0; i < K * K; ++i) A[i] = (double)c.A[i];
    const double* const ga = t.gamma.data() + ba * K;
    for (int j = 0; j < K; ++j) f[j * W] = ga[j];
    for (int x = 0; x < K; ++x)
        for (int i = 0; i < K; ++i) g[(size_t)x * K + i] = i == x ? 0.0 : ga[i];
    for (uint64_t b = ba + 1; b <= be; ++b) {
        const double* const v = t.v.data() + b * K;
        const double* const rho = t.rho.data() + b * K;
        for (int j = 0; j < K; ++j)
            for (uint32_t h = 0; h <= H; ++h) {
                double s = 0.0;
                if (h >= 1u)
                    for (int i = 0; i < K; ++i) {
                        if (i == j) continue;
                        double src = f[i * W + h - 1u] * rho[i];
                        if (h == H) src = src + f[i * W + h] * rho[i];
                        s = s + A[i * K + j] * src;
                    }
                nf[j * W + h] = (A[j * K + j] * (f[j * W + h] * rho[j]) + s) * v[j];
            }
        f.swap(nf);
        for (int x = 0; x < K; ++x)
            for (int i = 0; i < K; ++i) {
                double s = 0.0;
                for (int k = 0; k < K; ++k)
                    if (k != x) s = s + A[k * K + i] * (g[(size_t)x * K + k] * rho[k]);
                ng[(size_t)x * K + i] = i == x ? 0.0 : s * v[i];
            }
        g.swap(ng);
    }
    out.hist.assign(W, 0.0); out.whole_state.assign(K, 0.0); out.avoid.assign(K, 0.0);
    for (uint32_t h = 0; h <= H; ++h) {
        double s = 0.0;
        for (int j = 0; j < K; ++j) s = s + f[j * W + h];
        out.hist[h] = s;
    }
    for (int j = 0; j < K; ++j) out.whole_state[j] = f[j * W];
    for (int x = 0; x < K; ++x) {
        double s = 0.0;
        for (int i = 0; i < K; ++i)
            if (i != x) s = s + g[(size_t)x * K + i];
        out.avoid[x] = s;
    }
}

// the numbers hml_posterior_counts_info reports for one region: be - ba
static inline uint64_t hml_counts_ref_steps(const hml_post_ref_case& c, uint32_t start, uint32_t end) {
    return hml_pairs_block_of(c.starts.data(), c.B, end - 1u) - hml_pairs_block_of(c.starts.data(), c.B, start);
}

#endif
