// Posterior - smoothing under the chain's current parameters (include/hml.h, hml_posterior ... hml_posterior_info; no
// counterpart in the reference): the marginal log-likelihood log p(y | theta) of the compressed model, the call per position
// with a confidence per run, and the file the driver writes from them:
//   PREFIXposteriorSUFFIX   `-O PD`: first line "loglik<TAB>degenerate" (%.17g, integer), then "length<TAB>state<TAB>confidence"
//                           per run of equal called state - the maxsegmentation file's columns and, as %.17g, the smallest
//                           posterior of that state over the run's blocks
//   PREFIXposteriorbreaksSUFFIX   `-O PB`: first line "expected_breaks<TAB>pair_degenerate<TAB>min_prob" (%.17g, integer, %.17g),
//                           then "position<TAB>probability" (%.17g) per block boundary whose posterior probability of a change of
//                           state is at least `-pbreak P`, by ascending position (hml_posterior_breaks)
//   PREFIXposteriorregionsSUFFIX  `-O PR`: per region of `-regions FILE`, tab-separated: start, end, whole, expected_breaks,
//                           K whole_state, K share (%.17g), then the region's label (hml_posterior_regions)
// A thin handle over a context that something else owns (the chain's rng_t), next to Viterbi.  Every call computes anew; the
// chain is only read.
#ifndef HAMMLET_POSTERIOR_HPP
#define HAMMLET_POSTERIOR_HPP

#include <stdexcept>
#include <string>
#include <vector>

#include "../hml.h"
#include "TextFile.hpp"

namespace hammlet {

class Posterior {
    hml_ctx* mCtx;
    static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

public:
    struct Runs {
        std::vector<uint64_t> length;   // positions per run
        std::vector<int32_t> state;
        std::vector<double> confidence; // min over the run's blocks of p(q_b = state | y, theta)
    };
    struct Breaks {
        std::vector<uint32_t> position;    // starts[b] of the boundaries with p_b >= minProb, ascending
        std::vector<double> probability;   // p_b
        double expectedBreaks = 0;         // in the whole trace
        uint64_t pairDegenerate = 0;
    };
    struct Regions {
        std::vector<double> whole, expectedBreaks;   // [n]
        std::vector<double> wholeState, share;       // [n][K], row-major
        uint64_t pairDegenerate = 0;
    };
    struct Info { uint64_t chunks = 0, L = 0, W = 0, staleForward = 0, staleBackward = 0, rounds = 0, serialChunks = 0; };

    explicit Posterior(hml_ctx* ctx) : mCtx(ctx) {}
    // launch geometry only (0: the defaults): never part of the result
    void setGeometry(int W, int L, int rounds) {
        check(hml_set_option(mCtx, "posterior_W", W));
        check(hml_set_option(mCtx, "posterior_L", L));
        check(hml_set_option(mCtx, "posterior_rounds", rounds));
    }
    // log p(y | theta); `degenerate` (if given): the blocks no path reaches - the value is then -inf or not a number
    double loglik(uint64_t* degenerate = nullptr) const {
        double l = 0;
        check(hml_posterior(mCtx, nullptr, &l, degenerate));
        return l;
    }
    // gamma[B][K], row-major, for the model's K states
    std::vector<double> gamma(int K) const {
        uint64_t B = 0;
        check(hml_get_num_blocks(mCtx, &B));
        std::vector<double> g(B * (uint64_t)K);
        check(hml_posterior(mCtx, g.data(), nullptr, nullptr));
        return g;
    }
    Runs runs() const {
        Runs r;
        uint64_t n = 0;
        check(hml_posterior_rle(mCtx, &n, nullptr, nullptr, nullptr));
        r.length.resize(n);
        r.state.resize(n);
        r.confidence.resize(n);
        check(hml_posterior_rle(mCtx, &n, r.length.data(), r.state.data(), r.confidence.data()));
        return r;
    }
    // the block boundaries whose posterior probability of a change of state is at least minProb
    Breaks breaks(double minProb) const {
        Breaks b;
        uint64_t n = 0;
        check(hml_get_num_blocks(mCtx, &n));   // (room for every boundary: one call, one computation)
        b.position.resize(n);
        b.probability.resize(n);
        check(hml_posterior_breaks(mCtx, minProb, &n, b.position.data(), b.probability.data(), &b.expectedBreaks, &b.pairDegenerate));
        b.position.resize(n);
        b.probability.resize(n);
        return b;
    }
    // per region [start[r], end[r]): no breakpoint inside, all of it in state j, expected breakpoints, expected share of state j
    Regions regions(const std::vector<uint32_t>& start, const std::vector<uint32_t>& end, int K) const {
        if (start.size() != end.size()) throw std::runtime_error("Posterior::regions: as many starts as ends");
        Regions r;
        const size_t n = start.size();
        r.whole.resize(n); r.expectedBreaks.resize(n); r.wholeState.resize(n * (size_t)K); r.share.resize(n * (size_t)K);
        check(hml_posterior_regions(mCtx, n, start.data(), end.data(), r.whole.data(), r.wholeState.data(), r.expectedBreaks.data(), r.share.data(), nullptr,
                                    &r.pairDegenerate));
        return r;
    }
    Info info() const {
        Info i;
        check(hml_posterior_info(mCtx, &i.chunks, &i.L, &i.W, &i.staleForward, &i.staleBackward, &i.rounds, &i.serialChunks));
        return i;
    }

    void writeFile(const std::string& fn) const {
        uint64_t degenerate = 0;
        const double l = loglik(&degenerate);
        const Runs r = runs();
        TextFile out(fn);
        out.printf("%.17g\t%llu\n", l, (unsigned long long)degenerate);
        for (size_t i = 0; i < r.length.size(); ++i) out.printf("%llu\t%d\t%.17g\n", (unsigned long long)r.length[i], (int)r.state[i], r.confidence[i]);
        out.close();
    }

    void writeBreaksFile(const std::string& fn, double minProb) const {
        const Breaks b = breaks(minProb);
        TextFile out(fn);
        out.printf("%.17g\t%llu\t%.17g\n", b.expectedBreaks, (unsigned long long)b.pairDegenerate, minProb);
        for (size_t i = 0; i < b.position.size(); ++i) out.printf("%u\t%.17g\n", b.position[i], b.probability[i]);
        out.close();
    }

    void writeRegionsFile(const std::string& fn, const std::vector<uint32_t>& start, const std::vector<uint32_t>& end, const std::vector<std::string>& label, int K) const {
        const Regions r = regions(start, end, K);
        TextFile out(fn);
        for (size_t i = 0; i < start.size(); ++i) {
            out.printf("%u\t%u\t%.17g\t%.17g", start[i], end[i], r.whole[i], r.expectedBreaks[i]);
            for (int j = 0; j < K; ++j) out.printf("\t%.17g", r.wholeState[i * (size_t)K + j]);
            for (int j = 0; j < K; ++j) out.printf("\t%.17g", r.share[i * (size_t)K + j]);
            out.printf("\t%s\n", i < label.size() ? label[i].c_str() : "");
        }
        out.close();
    }
};

}  // namespace hammlet

#endif
