// Path sampling under fixed parameters (hml_posterior_sample of include/hml.h) restated for one host thread: independent
// draws of whole state paths from p(q | y, theta) over the blocks, by the backward sampling that follows a forward pass.  No
// HIP; compile with -ffp-contract=off.  The kernels of hml_k_sample.h must give these very words.
//
//   alpha_b(i)   the forward rows of the smoothing (hml_posterior_ref.h), with their degenerate restarts; A widened exactly
//                from float to double.  The backward recursion is not run.
//   uniform      of draw r at block b: o = hml_stream4(hml_make_key(seed, 0), HML_KIND_PSAMPLE, r, b >> 1, 0);
//                (hi, lo) = (o.v[0], o.v[1]) for even b, (o.v[2], o.v[3]) for odd b;
//                u = ((hi >> 5) 2^26 + (lo >> 6)) 2^-53, in [0, 1).  Draw r depends on (seed, r) alone.
//   categorical  over weights w(0 ... K - 1), IEEE double: c_i the running sums from 0.0 in ascending i, S = c_{K-1}, t = u S;
//                the state is the smallest i with t < c_i; if there is none (t rounded up to S) the largest i with w(i) > 0.
//                A state of weight 0 is never drawn.
//   recursion    q_{B-1} from w = alpha_{B-1};  q_b, b = B - 2 ... 0, from w(i) = alpha_b(i) A[i][q_{b+1}] (one multiplication).
//                If S is not a positive finite number the block is DEGENERATE for this draw (counted in sample_degenerate) and
//                the draw uses w = alpha_b; if that sum fails the same test, q_b = 0.
//   per draw     segments = 1 + #{b >= 1 : q_b != q_{b-1}};  score_fixed = init[q_0] + sum_b emit[b][q_b] + sum_{b >= 1}
//                trans[q_{b-1}][q_b] in the int64 tables of hml_viterbi_ref.h (wrap-around), never above the decode's score
//   per call     change_count[b] = #draws with q_b != q_{b-1} (0 at b = 0);  state_count[b][j] = #draws with q_b = j
//   per region   [start, end): ba, be the blocks of start and end - 1;  n_r = #{b in (ba, be] : q_b != q_{b-1}} in draw r;
//                hist[h], h = 0 ... H, counts the draws with n_r = h, the last bin n_r >= H;  whole_state[j] the draws with
//                n_r = 0 and q_ba = j;  breaks_sum = sum_r n_r, breaks_sq = sum_r n_r^2
#ifndef HML_SAMPLE_REF_H
#define HML_SAMPLE_REF_H

#include "hml_philox.h"
#include "hml_posterior_ref.h"
#include "hml_viterbi_ref.h"

// the four words that hold the uniforms of draw r at blocks 2 i and 2 i + 1, and the uniform at block b from them
HML_HD hml_u32x4 hml_sample_words(uint64_t seed, uint64_t r, uint32_t i) { return hml_stream4(hml_make_key(seed, 0), HML_KIND_PSAMPLE, r, i, 0); }
HML_HD double hml_sample_uniform_of(const hml_u32x4& o, uint32_t b) {
    const uint32_t hi = (b & 1u) ? o.v[2] : o.v[0], lo = (b & 1u) ? o.v[3] : o.v[1];
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}
// the uniform of draw r at block b
HML_HD double hml_sample_uniform(uint64_t seed, uint64_t r, uint32_t b) { return hml_sample_uniform_of(hml_sample_words(seed, r, b >> 1), b); }

HML_HD bool hml_sample_bad(double x) { return !(x > 0.0 && x < (double)INFINITY); }

// the categorical rule over w[K] whose sum S is a positive finite number
HML_HD int hml_sample_pick(int K, const double* w, double S, double u) {
    const double t = u * S;
    double c = 0.0;
    int last = 0;
    for (int i = 0; i < K; ++i) {
        c = c + w[i];
        if (t < c) return i;
        if (w[i] > 0.0) last = i;
    }
    return last;
}

// q_b given the successor's state (next < 0: the last block); *degenerate is raised if the block is degenerate for the draw
static inline int hml_sample_ref_step(int K, const float* A, const double* alpha_b, int next, double u, bool* degenerate) {
    double w[HML_POST_CAP_K];
    double S = 0.0;
    for (int i = 0; i < K; ++i) {
        w[i] = next < 0 ? alpha_b[i] : alpha_b[i] * (double)A[i * K + next];
        S = S + w[i];
    }
    if (!hml_sample_bad(S)) return hml_sample_pick(K, w, S, u);
    *degenerate = true;
    S = 0.0;
    for (int i = 0; i < K; ++i) S = S + alpha_b[i];
    if (hml_sample_bad(S)) return 0;
    return hml_sample_pick(K, alpha_b, S, u);
}

struct hml_sample_ref_result {
    std::vector<uint8_t> paths;            // [count][B]
    std::vector<uint64_t> segments;        // [count]
    std::vector<int64_t> score_fixed;      // [count]
    std::vector<uint32_t> change_count;    // [B]
    std::vector<uint32_t> state_count;     // [B][K]
    uint64_t sample_degenerate = 0;
};

// draws first ... first + count - 1 from the rows alpha[B][K]; the score tables as hml_vit_ref_tables gives them
static inline void hml_sample_ref_draw(int K, uint64_t B, const float* A, const double* alpha, const std::vector<int64_t>& emit, const std::vector<int64_t>& trans,
                                       const std::vector<int64_t>& init, uint64_t first, uint64_t count, uint64_t seed, hml_sample_ref_result& out) {
    out.paths.assign((size_t)count * B, 0);
    out.segments.assign(count, 0); out.score_fixed.assign(count, 0);
    out.change_count.assign(B, 0); out.state_count.assign((size_t)B * K, 0);
    out.sample_degenerate = 0;
    for (uint64_t k = 0; k < count; ++k) {
        uint8_t* const q = out.paths.data() + k * B;
        int next = -1;
        for (uint64_t b = B; b-- > 0;) {
            bool deg = false;
            next = hml_sample_ref_step(K, A, alpha + b * K, next, hml_sample_uniform(seed, first + k, (uint32_t)b), &deg);
            if (deg) ++out.sample_degenerate;
            q[b] = (uint8_t)next;
        }
        uint64_t seg = 1, sum = (uint64_t)init[q[0]];
        for (uint64_t b = 0; b < B; ++b) {
            sum += (uint64_t)emit[b * K + q[b]];
            ++out.state_count[b * K + q[b]];
            if (b > 0) {
                sum += (uint64_t)trans[(size_t)q[b - 1] * K + q[b]];
                if (q[b] != q[b - 1]) { ++seg; ++out.change_count[b]; }
            }
        }
        out.segments[k] = seg;
        out.score_fixed[k] = (int64_t)sum;
    }
}

// the block of position t (starts[B + 1], starts[B] = T)
static inline uint64_t hml_sample_ref_block_of(const std::vector<uint32_t>& starts, uint32_t t) {
    uint64_t lo = 0, hi = starts.size() - 1;   // starts[lo] <= t < starts[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (starts[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// the region counts of paths[count][B]: hist[n][H + 1], whole_state[n][K], breaks_sum[n], breaks_sq[n]
static inline void hml_sample_ref_regions(int K, uint64_t B, const std::vector<uint32_t>& starts, const std::vector<uint8_t>& paths, uint64_t count, uint64_t n,
                                          const uint32_t* start, const uint32_t* end, uint32_t H, std::vector<uint32_t>& hist, std::vector<uint32_t>& whole_state,
                                          std::vector<uint64_t>& breaks_sum, std::vector<uint64_t>& breaks_sq) {
    hist.assign((size_t)n * (H + 1u), 0); whole_state.assign((size_t)n * K, 0);
    breaks_sum.assign(n, 0); breaks_sq.assign(n, 0);
    for (uint64_t g = 0; g < n; ++g) {
        const uint64_t ba = hml_sample_ref_block_of(starts, start[g]), be = hml_sample_ref_block_of(starts, end[g] - 1u);
        for (uint64_t k = 0; k < count; ++k) {
            const uint8_t* const q = paths.data() + k * B;
            uint64_t m = 0;
            for (uint64_t b = ba + 1; b <= be; ++b) m += q[b] != q[b - 1];
            ++hist[g * (H + 1u) + (m < H ? m : H)];
            if (m == 0) ++whole_state[g * K + q[ba]];
            breaks_sum[g] += m; breaks_sq[g] += m * m;
        }
    }
}

#endif
