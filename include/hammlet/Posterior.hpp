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
//   PREFIXposteriorsampleSUFFIX   `-O PS` with `-psample R [SEED]`: one line per independent draw of a whole path from
//                           p(q | y, theta), tab-separated SIZE:STATE per run - the `sequences` file's line (hml_posterior_sample)
//   PREFIXposteriorsamplesummarySUFFIX  `-O PSS`: "draws<TAB>seed<TAB>viterbi_score<TAB>expected_breaks", then per draw
//                           "index<TAB>segments<TAB>score" (nats); with `-regions FILE`, then per region start, end, the mean number
//                           of breakpoints inside it, its histogram over the draws and the label
//   PREFIXposteriorcountsSUFFIX   `-O PC` with `-pcounts H`: per region of `-regions FILE`, tab-separated: start, end, the H + 1
//                           exact probabilities of 0, 1, ... H - 1 and of H or more breakpoints inside it, then per state the
//                           probability that no position of the region is in it (%.17g) (hml_posterior_region_counts)
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
    struct RegionCounts {
        uint32_t maxBreaks = 0;
        std::vector<double> hist;                 // [n][maxBreaks + 1], row-major: exactly h breakpoints; the last bin: that many or more
        std::vector<double> wholeState, avoid;    // [n][K]: all of it in state j; no position of it in state j
        uint64_t countDegenerate = 0;
    };
    struct CountsInfo { uint64_t regions = 0, steps = 0, longest = 0; };
    struct Info { uint64_t chunks = 0, L = 0, W = 0, staleForward = 0, staleBackward = 0, rounds = 0, serialChunks = 0; };
    struct Sample {
        uint64_t first = 0, blocks = 0;
        std::vector<uint8_t> paths;          // [count][blocks], if asked for
        std::vector<uint64_t> segments;      // [count]
        std::vector<int64_t> scoreFixed;     // [count], units of 2^-20 nat
        std::vector<uint32_t> changeCount;   // [blocks]
        std::vector<uint32_t> stateCount;    // [blocks][K], if asked for
        uint64_t degenerate = 0;
    };
    struct SampleRegions {
        uint32_t maxBreaks = 0;
        std::vector<uint32_t> hist, wholeState;      // [n][maxBreaks + 1], [n][K]
        std::vector<uint64_t> breaksSum, breaksSq;   // [n]
    };
    struct SampleInfo { uint64_t draws = 0, groups = 0, groupSize = 0, chunks = 0, L = 0, W = 0, staleFirst = 0, rounds = 0, serialChunks = 0; };

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
    // per region [start[r], end[r]): the exact distribution of the number of breakpoints inside it, all of it in state j, none of
    // it in state j (hml_posterior_region_counts); maxBreaks 1 ... 32 with K (maxBreaks + 1) <= 1024
    RegionCounts regionCounts(const std::vector<uint32_t>& start, const std::vector<uint32_t>& end, uint32_t maxBreaks, int K) const {
        if (start.size() != end.size()) throw std::runtime_error("Posterior::regionCounts: as many starts as ends");
        RegionCounts r;
        const size_t n = start.size();
        r.maxBreaks = maxBreaks;
        r.hist.resize(n * ((size_t)(maxBreaks <= 32u ? maxBreaks : 32u) + 1)); r.wholeState.resize(n * (size_t)K); r.avoid.resize(n * (size_t)K);
        check(hml_posterior_region_counts(mCtx, n, start.data(), end.data(), maxBreaks, r.hist.data(), r.wholeState.data(), r.avoid.data(), &r.countDegenerate));
        return r;
    }
    CountsInfo countsInfo() const {
        CountsInfo i;
        check(hml_posterior_counts_info(mCtx, &i.regions, &i.steps, &i.longest));
        return i;
    }
    Info info() const {
        Info i;
        check(hml_posterior_info(mCtx, &i.chunks, &i.L, &i.W, &i.staleForward, &i.staleBackward, &i.rounds, &i.serialChunks));
        return i;
    }

    // ---- sampled paths: independent draws from p(q | y, theta) (hml_posterior_sample) ----
    // Draws first ... first + count - 1 under `seed`; draw r depends on (seed, r) alone.  With paths: the states per block,
    // draw-major.
    Sample sample(uint64_t first, uint64_t count, uint64_t seed, bool paths = false, bool stateCounts = false, int K = 0) const {
        Sample s;
        check(hml_get_num_blocks(mCtx, &s.blocks));
        s.first = first;
        s.segments.resize(count); s.scoreFixed.resize(count); s.changeCount.resize(s.blocks);
        if (paths) s.paths.resize(count * s.blocks);
        if (stateCounts) s.stateCount.resize(s.blocks * (uint64_t)K);
        check(hml_posterior_sample(mCtx, first, count, seed, paths ? s.paths.data() : nullptr, s.segments.data(), s.scoreFixed.data(), s.changeCount.data(),
                                   stateCounts ? s.stateCount.data() : nullptr, &s.degenerate));
        return s;
    }
    // per region over the same draws: the histogram of the number of breakpoints inside it, and the draws that hold it whole
    SampleRegions sampleRegions(const std::vector<uint32_t>& start, const std::vector<uint32_t>& end, uint64_t first, uint64_t count, uint64_t seed, uint32_t maxBreaks,
                                int K) const {
        if (start.size() != end.size()) throw std::runtime_error("Posterior::sampleRegions: as many starts as ends");
        SampleRegions r;
        const size_t n = start.size();
        r.maxBreaks = maxBreaks;
        r.hist.resize(n * ((size_t)maxBreaks + 1)); r.wholeState.resize(n * (size_t)K); r.breaksSum.resize(n); r.breaksSq.resize(n);
        check(hml_posterior_sample_regions(mCtx, first, count, seed, n, start.data(), end.data(), maxBreaks, r.hist.data(), r.wholeState.data(), r.breaksSum.data(),
                                           r.breaksSq.data()));
        return r;
    }
    SampleInfo sampleInfo() const {
        SampleInfo i;
        check(hml_posterior_sample_info(mCtx, &i.draws, &i.groups, &i.groupSize, &i.chunks, &i.L, &i.W, &i.staleFirst, &i.rounds, &i.serialChunks));
        return i;
    }
    // the run-length form of draw k of a sample with paths: adjacent blocks of equal state merged, lengths in positions
    static void sampleRuns(const Sample& s, const std::vector<uint32_t>& starts, uint64_t k, std::vector<uint64_t>& length, std::vector<int32_t>& state) {
        length.clear(); state.clear();
        const uint8_t* const q = s.paths.data() + k * s.blocks;
        for (uint64_t b = 0; b < s.blocks; ++b) {
            const uint64_t n = starts[b + 1] - starts[b];
            if (b > 0 && state.back() == (int32_t)q[b]) length.back() += n;
            else { length.push_back(n); state.push_back(q[b]); }
        }
    }
    // the draws of a window whose paths take at most hostBytes on the host (at least one)
    uint64_t sampleWindow(uint64_t hostBytes) const {
        uint64_t B = 0;
        check(hml_get_num_blocks(mCtx, &B));
        const uint64_t per = B + 16u;
        return hostBytes / per > 0 ? hostBytes / per : 1u;
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

    // `-O PS`: one line per draw, tab-separated SIZE:STATE per run of equal state - the line format of the `sequences` file.
    // The draws are read in windows of at most hostBytes of paths.
    void writeSampleFile(const std::string& fn, uint64_t count, uint64_t seed, uint64_t hostBytes = 256ull << 20) const {
        uint64_t B = 0;
        check(hml_get_num_blocks(mCtx, &B));
        std::vector<uint32_t> starts(B + 1);
        check(hml_get_blocks(mCtx, starts.data()));
        const uint64_t window = sampleWindow(hostBytes);
        std::vector<uint64_t> length;
        std::vector<int32_t> state;
        TextFile out(fn);
        for (uint64_t first = 0; first < count; first += window) {
            const uint64_t n = count - first < window ? count - first : window;
            const Sample s = sample(first, n, seed, true);
            for (uint64_t k = 0; k < n; ++k) {
                sampleRuns(s, starts, k, length, state);
                for (size_t i = 0; i < length.size(); ++i) out.printf("%s%llu:%d", i ? "\t" : "", (unsigned long long)length[i], (int)state[i]);
                out.printf("\n");
            }
        }
        out.close();
    }

    // `-O PSS`: first line "draws<TAB>seed<TAB>viterbi_score<TAB>expected_breaks" (integers, %.17g nats, %.17g), then per draw
    // "index<TAB>segments<TAB>score" (%.17g nats); with regions, then per region "start<TAB>end<TAB>mean_breaks<TAB>hist[0 ...
    // maxBreaks]<TAB>label", the histogram in draws (last bin: that many breakpoints or more)
    void writeSampleSummaryFile(const std::string& fn, uint64_t count, uint64_t seed, const std::vector<uint32_t>& start, const std::vector<uint32_t>& end,
                                const std::vector<std::string>& label, int K, uint32_t maxBreaks = 8) const {
        uint64_t nRuns = 0;
        double vitScore = 0;
        check(hml_viterbi(mCtx, &nRuns, nullptr, nullptr, nullptr, &vitScore));
        const Breaks b = breaks(2.0);   // (no boundary is listed: the expectation alone)
        const Sample s = sample(0, count, seed);
        TextFile out(fn);
        out.printf("%llu\t%llu\t%.17g\t%.17g\n", (unsigned long long)count, (unsigned long long)seed, vitScore, b.expectedBreaks);
        for (uint64_t k = 0; k < count; ++k)
            out.printf("%llu\t%llu\t%.17g\n", (unsigned long long)k, (unsigned long long)s.segments[k], (double)s.scoreFixed[k] / 1048576.0);
        if (!start.empty()) {
            const SampleRegions r = sampleRegions(start, end, 0, count, seed, maxBreaks, K);
            for (size_t i = 0; i < start.size(); ++i) {
                out.printf("%u\t%u\t%.17g", start[i], end[i], (double)r.breaksSum[i] / (double)count);
                for (uint32_t h = 0; h <= maxBreaks; ++h) out.printf("\t%u", r.hist[i * ((size_t)maxBreaks + 1) + h]);
                out.printf("\t%s\n", i < label.size() ? label[i].c_str() : "");
            }
        }
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

    // `-O PC`: per region "start<TAB>end<TAB>hist[0 ... maxBreaks]<TAB>avoid[0 ... K - 1]", %.17g
    void writeCountsFile(const std::string& fn, const std::vector<uint32_t>& start, const std::vector<uint32_t>& end, uint32_t maxBreaks, int K) const {
        const RegionCounts r = regionCounts(start, end, maxBreaks, K);
        TextFile out(fn);
        for (size_t i = 0; i < start.size(); ++i) {
            out.printf("%u\t%u", start[i], end[i]);
            for (uint32_t h = 0; h <= maxBreaks; ++h) out.printf("\t%.17g", r.hist[i * ((size_t)maxBreaks + 1) + h]);
            for (int j = 0; j < K; ++j) out.printf("\t%.17g", r.avoid[i * (size_t)K + j]);
            out.printf("\n");
        }
        out.close();
    }
};

}  // namespace hammlet

#endif
