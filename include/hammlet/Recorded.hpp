// Recorded - the read-outs of what a context recorded over its sweeps (include/hml.h, hml_levels_rle ... hml_regions_read; no
// counterpart in the reference), and the files the driver writes from them:
//   PREFIXlevelsSUFFIX        `-O L`: "length mean_0 sd_0 [mean_1 sd_1 ...]" per segment, %.9g
//   PREFIXrhatSUFFIX          `-O R`: "length rhat_0 [rhat_1 ...]" per segment of the union of the chains' level boundaries, from
//                             the chains' levels BEFORE they are merged, %.9g of the double
//   PREFIXbreakpointsSUFFIX   `-O BP`: "position count probability" per listed position, the probability count / N in double, %.9g
//   PREFIXconsensusSUFFIX     `-O CS`: "start length support mean_0 sd_0 [mean_1 sd_1 ...]" per segment between consensus
//                             breakpoints; support = windowed mass / N of the segment's left boundary (1 for the first segment);
//                             mean and standard deviation of the level pooled over the segment's positions and the recorded sweeps
//   PREFIXbandsSUFFIX         `-O LB`: "length c_0 ... c_{n_columns-1}" per band segment, tab-separated like the marginals file;
//                             column d (edges + 1) + b = the recorded sweeps whose level of dimension d lay in band b
//   PREFIXbandcallsSUFFIX     `-O LC`: "start length band_0 [band_1 ...]" per run of equal calls; quantile 0: the most probable band,
//                             0 < P <= 1: the band of the rank max(1, ceil(P N))-th smallest of the N recorded levels
//   PREFIXregionsSUFFIX       `-O RG`: one line per region in the order of the regions file, tab-separated: start end N whole
//                             breaks_mean breaks_sd [level_mean_d level_sd_d per dimension] [inband per dimension and band] label
// Means and standard deviations everywhere by meanSd() below.  A thin handle over a context that something else owns (the
// chain's rng_t), next to Viterbi, Posterior, Fit and History; D is the number of data dimensions of the context's model.
#ifndef HAMMLET_RECORDED_HPP
#define HAMMLET_RECORDED_HPP

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../hml.h"
#include "TextFile.hpp"

namespace hammlet {

// Mean and spread from a sum, a sum of squares and their weight, as every file prints them (the formula of
// hml_levels_dense_device): double arithmetic, the variance clamped at 0, one rounding to float; weight 0 - nothing recorded - nan.
// keepNanVariance: a variance that is not a number stays one (it clamps to 0 otherwise).
struct MeanSd { float mean = NAN, sd = NAN; };
inline MeanSd meanSd(double sum, double sumSq, double weight, bool keepNanVariance = false) {
    MeanSd r;
    if (!(weight > 0)) return r;
    const double m = sum / weight;
    const double var = sumSq / weight - m * m;
    r.mean = (float)m;
    r.sd = (float)std::sqrt(var > 0.0 ? var : 0.0);
    if (keepNanVariance && var != var) r.sd = NAN;
    return r;
}

// the regions of `-regions FILE`, in file order
struct Regions {
    std::vector<uint32_t> start, end;
    std::vector<std::string> label;
};

// `-regions FILE`: "start end [label ...]" per line, 0-based and half-open, within the T positions of the input; lines that
// begin with # and blank lines are skipped
inline Regions readRegions(const std::string& fname, size_t T) {
    using std::string;
    std::ifstream fin(fname);
    if (!fin) throw std::runtime_error("Cannot read from regions file " + fname + "!");
    Regions regions;
    string line;
    size_t lineNo = 0;
    while (std::getline(fin, line)) {
        ++lineNo;
        const string where = "Regions file " + fname + ", line " + std::to_string(lineNo) + ": ";
        size_t i = line.find_first_not_of(" \t\r");
        if (i == string::npos || line[i] == '#') continue;
        unsigned long long v[2];
        for (int k = 0; k < 2; ++k) {
            const size_t j = line.find_first_of(" \t\r", i);
            const string tok = line.substr(i, j == string::npos ? string::npos : j - i);
            char* end = nullptr;
            if (tok.empty() || tok[0] < '0' || tok[0] > '9') throw std::runtime_error(where + "expected \"start end [label]\", two whole numbers, found \"" + tok + "\"!");
            v[k] = strtoull(tok.c_str(), &end, 10);
            if (*end || tok.size() > 18) throw std::runtime_error(where + "expected \"start end [label]\", two whole numbers, found \"" + tok + "\"!");
            i = j == string::npos ? string::npos : line.find_first_not_of(" \t\r", j);
            if (k == 0 && i == string::npos) throw std::runtime_error(where + "expected \"start end [label]\", found one number only!");
        }
        if (v[1] <= v[0]) throw std::runtime_error(where + "the end (" + std::to_string(v[1]) + ") must lie beyond the start (" + std::to_string(v[0]) + ")!");
        if (v[1] > T) throw std::runtime_error(where + "the end (" + std::to_string(v[1]) + ") lies beyond the " + std::to_string(T) + " positions of the input!");
        string label = i == string::npos ? "" : line.substr(i);
        while (!label.empty() && (label.back() == ' ' || label.back() == '\t' || label.back() == '\r')) label.pop_back();
        if (regions.start.size() >= (size_t(1) << 22)) throw std::runtime_error("Regions file " + fname + " holds more than 4194304 regions!");
        regions.start.push_back((uint32_t)v[0]);
        regions.end.push_back((uint32_t)v[1]);
        regions.label.push_back(label);
    }
    if (regions.start.empty()) throw std::runtime_error("Regions file " + fname + " holds no regions!");
    return regions;
}

class Recorded {
    hml_ctx* mCtx;
    static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

public:
    explicit Recorded(hml_ctx* ctx) : mCtx(ctx) {}

    void writeLevelsFile(const std::string& fn, size_t D) const {
        uint64_t M = 0, N = 0;
        check(hml_levels_rle(mCtx, &M, &N, nullptr, nullptr, nullptr));
        std::vector<uint64_t> len(M);
        std::vector<double> s1(M * D), s2(M * D);
        check(hml_levels_rle(mCtx, &M, &N, len.data(), s1.data(), s2.data()));
        TextFile out(fn);
        for (uint64_t i = 0; i < M; ++i) {
            out.printf("%llu", (unsigned long long)len[i]);
            for (size_t d = 0; d < D; ++d) {
                const MeanSd l = meanSd(s1[d * M + i], s2[d * M + i], (double)N);
                out.printf(" %.9g %.9g", (double)l.mean, (double)l.sd);
            }
            out.printf("\n");
        }
        out.close();
    }

    // the agreement of the chains' levels, the chains one by one (a merge changes the first)
    static void writeRhatFile(const std::string& fn, const std::vector<hml_ctx*>& ctxs, size_t D) {
        const int n = (int)ctxs.size();
        uint64_t U = 0, N = 0;
        check(hml_levels_agreement_rle(ctxs.data(), n, &U, &N, nullptr, nullptr, nullptr, nullptr));
        std::vector<uint64_t> len(U);
        std::vector<double> rhat(U * D);
        check(hml_levels_agreement_rle(ctxs.data(), n, &U, &N, len.data(), nullptr, nullptr, rhat.data()));
        TextFile out(fn);
        for (uint64_t i = 0; i < U; ++i) {
            out.printf("%llu", (unsigned long long)len[i]);
            for (size_t d = 0; d < D; ++d) out.printf(" %.9g", rhat[d * U + i]);
            out.printf("\n");
        }
        out.close();
    }

    void writeBreakpointsFile(const std::string& fn) const {
        uint64_t M = 0, N = 0;
        check(hml_breaks_list(mCtx, &M, &N, nullptr, nullptr));
        std::vector<uint32_t> pos(M), cnt(M);
        if (M) check(hml_breaks_list(mCtx, &M, &N, pos.data(), cnt.data()));
        TextFile out(fn);
        for (uint64_t i = 0; i < M; ++i) out.printf("%u %u %.9g\n", pos[i], cnt[i], (double)cnt[i] / (double)N);
        out.close();
    }

    // `-consensus W P` over the T positions: a breakpoint is kept when the sweeps with one within `window` positions of it number
    // at least `share` of the recorded ones (hml_breaks_consensus); the levels on the segments by hml_levels_on_segments
    void writeConsensusFile(const std::string& fn, size_t D, size_t T, uint32_t window, double share) const {
        uint64_t M = 0, N = 0, S = 0, Mlev = 0, Nlev = 0;
        check(hml_breaks_list(mCtx, &M, &N, nullptr, nullptr));
        const double need = std::ceil(share * (double)N);
        const uint64_t minCount = need > 1.0 ? (uint64_t)need : 1;
        check(hml_breaks_consensus(mCtx, window, minCount, &S, nullptr, nullptr, nullptr));
        std::vector<uint32_t> pos(S), peak(S);
        std::vector<uint64_t> mass(S);
        if (S) check(hml_breaks_consensus(mCtx, window, minCount, &S, pos.data(), mass.data(), peak.data()));
        check(hml_levels_rle(mCtx, &Mlev, &Nlev, nullptr, nullptr, nullptr));
        std::vector<double> s1((S + 1) * D), s2((S + 1) * D);
        check(hml_levels_on_segments(mCtx, S, pos.data(), s1.data(), s2.data()));
        TextFile out(fn);
        for (uint64_t k = 0; k <= S; ++k) {
            const uint64_t start = k == 0 ? 0 : pos[k - 1], end = k == S ? T : pos[k];
            out.printf("%llu %llu %.9g", (unsigned long long)start, (unsigned long long)(end - start), k == 0 ? 1.0 : (double)mass[k - 1] / (double)N);
            for (size_t d = 0; d < D; ++d) {
                const MeanSd l = meanSd(s1[d * (S + 1) + k], s2[d * (S + 1) + k], (double)Nlev * (double)(end - start));
                out.printf(" %.9g %.9g", (double)l.mean, (double)l.sd);
            }
            out.printf("\n");
        }
        out.close();
    }

    void writeBandsFile(const std::string& fn) const {
        uint64_t M = 0, N = 0;
        int ncol = 0;
        check(hml_bands_rle(mCtx, &M, &ncol, &N, nullptr, nullptr));
        std::vector<uint64_t> len(M);
        std::vector<int32_t> cnt(M * (size_t)ncol);
        check(hml_bands_rle(mCtx, &M, &ncol, &N, len.data(), cnt.data()));
        TextFile out(fn);
        for (uint64_t i = 0; i < M; ++i) {
            out.printf("%llu", (unsigned long long)len[i]);
            for (int s = 0; s < ncol; ++s) out.printf("\t%d", cnt[i * (size_t)ncol + s]);
            out.printf("\n");
        }
        out.close();
    }

    // quantile: the P of `-bandcall P`
    void writeBandCallsFile(const std::string& fn, size_t D, double quantile) const {
        uint64_t M = 0, N = 0, R = 0;
        int ncol = 0;
        check(hml_bands_rle(mCtx, &M, &ncol, &N, nullptr, nullptr));
        uint64_t rank = 0;
        if (quantile > 0 && N > 0) {
            const double r = std::ceil(quantile * (double)N);
            rank = r > 1.0 ? (uint64_t)r : 1;
            if (rank > N) rank = N;
        }
        check(hml_bands_call(mCtx, rank, &R, nullptr, nullptr));
        std::vector<uint64_t> len(R);
        std::vector<int32_t> band(R * D);
        check(hml_bands_call(mCtx, rank, &R, len.data(), band.data()));
        TextFile out(fn);
        uint64_t start = 0;
        for (uint64_t r = 0; r < R; ++r) {
            out.printf("%llu %llu", (unsigned long long)start, (unsigned long long)len[r]);
            for (size_t d = 0; d < D; ++d) out.printf(" %d", band[d * R + r]);
            out.printf("\n");
            start += len[r];
        }
        out.close();
    }

    // the regions the context was given (hml_set_regions), with their labels.  The spread of the breakpoint count is nan once
    // its sum of squares has saturated.
    void writeRegionsFile(const std::string& fn, size_t D, const Regions& regions) const {
        uint64_t n = 0, N = 0;
        int ncol = 0;
        check(hml_regions_read(mCtx, &n, &ncol, &N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<uint64_t> whole(n), bsum(n), bsq(n), inband(n * (size_t)ncol);
        std::vector<double> lsum(n * D), lsq(n * D);
        check(hml_regions_read(mCtx, &n, &ncol, &N, whole.data(), bsum.data(), bsq.data(), lsum.data(), lsq.data(), inband.data()));
        TextFile out(fn);
        for (uint64_t r = 0; r < n; ++r) {
            MeanSd b = meanSd((double)bsum[r], (double)bsq[r], (double)N, true);
            if (bsq[r] == ~0ull) b.sd = NAN;
            out.printf("%u\t%u\t%llu\t%llu\t%.9g\t%.9g", regions.start[r], regions.end[r], (unsigned long long)N, (unsigned long long)whole[r], (double)b.mean, (double)b.sd);
            for (size_t d = 0; d < D; ++d) {
                const MeanSd l = meanSd(lsum[d * n + r], lsq[d * n + r], (double)N, true);
                out.printf("\t%.9g\t%.9g", (double)l.mean, (double)l.sd);
            }
            for (int j = 0; j < ncol; ++j) out.printf("\t%llu", (unsigned long long)inband[r * (size_t)ncol + j]);
            out.printf("\t%s\n", regions.label[r].c_str());
        }
        out.close();
    }
};

}  // namespace hammlet

#endif
