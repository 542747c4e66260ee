// History - the chain's history (include/hml.h, hml_set_history ... hml_history_summary; no counterpart in the reference): a row
// of scalars per sweep - log-likelihood, log-prior, segments, blocks, threshold - kept on the device, and the files the driver
// writes from it:
//   PREFIXhistorySUFFIX          a header line with the column names, then one line per row, the chains in order; the doubles
//                                with %.17g (they read back to the same bits), the whole-number columns as whole numbers
//   PREFIXhistorysummarySUFFIX   for loglik (ll_emit + ll_path), logpost (... + the two log-priors), segments and blocks: a line
//                                "NAME all RHAT ESS ROWS NONFINITE" - split R-hat and effective sample size over the chains, the
//                                rows used per chain, the values that were not finite - then "NAME CHAIN MEAN SD" per chain
// A thin handle over a context that something else owns (the chain's rng_t), next to Records.
#ifndef HAMMLET_HISTORY_HPP
#define HAMMLET_HISTORY_HPP

#include <stdexcept>
#include <string>
#include <vector>

#include "../hml.h"
#include "TextFile.hpp"

namespace hammlet {

class History {
    hml_ctx* mCtx;
    static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

public:
    explicit History(hml_ctx* ctx) : mCtx(ctx) {}
    // sweeps whose number is a multiple of `every` leave a row from now on
    void enable(uint64_t every = 1) { check(hml_set_history(mCtx, 1, every)); }
    void disable() { check(hml_set_history(mCtx, 0, 1)); }
    void clear() { check(hml_history_clear(mCtx)); }
    uint64_t size() const { uint64_t n = 0; check(hml_history_size(mCtx, &n, nullptr)); return n; }
    uint64_t dropped() const { uint64_t n = 0, d = 0; check(hml_history_size(mCtx, &n, &d)); return d; }
    // the rows so far, HML_HISTORY_COLS doubles each
    std::vector<double> rows() const {
        const uint64_t n = size();
        std::vector<double> r((size_t)n * HML_HISTORY_COLS);
        if (n) check(hml_history_read(mCtx, 0, n, r.data()));
        return r;
    }
    static bool wholeNumberColumn(int col) { return col == 0 || col == 1 || col == 6 || col == 7 || col == 8 || col == 10; }

    // PREFIXhistorySUFFIX of the chains, in order
    static void writeFile(const std::string& fn, const std::vector<hml_ctx*>& ctxs) {
        TextFile out(fn);
        for (int j = 0; j < HML_HISTORY_COLS; ++j) out.printf("%s%s", j ? "\t" : "", hml_history_column(j));
        out.printf("\n");
        for (hml_ctx* ctx : ctxs) {
            const std::vector<double> r = History(ctx).rows();
            for (size_t i = 0; i + HML_HISTORY_COLS <= r.size(); i += HML_HISTORY_COLS) {
                for (int j = 0; j < HML_HISTORY_COLS; ++j) {
                    if (wholeNumberColumn(j)) out.printf("%s%lld", j ? "\t" : "", (long long)r[i + (size_t)j]);
                    else out.printf("%s%.17g", j ? "\t" : "", r[i + (size_t)j]);
                }
                out.printf("\n");
            }
        }
        out.close();
    }

    // PREFIXhistorysummarySUFFIX of the chains: the rows with sweep <= skipSweeps are left out
    static void writeSummaryFile(const std::string& fn, const std::vector<hml_ctx*>& ctxs, uint64_t skipSweeps) {
        TextFile out(fn);
        const struct { const char* name; int col; } what[4] = {{"loglik", HML_HISTORY_LOGLIK}, {"logpost", HML_HISTORY_LOGPOST}, {"segments", 6}, {"blocks", 7}};
        const int n = (int)ctxs.size();
        std::vector<double> mean((size_t)n), sd((size_t)n);
        for (const auto& w : what) {
            double rhat = 0, ess = 0;
            uint64_t used = 0, bad = 0;
            check(hml_history_summary(ctxs.data(), n, w.col, skipSweeps, &rhat, &ess, mean.data(), sd.data(), &used, &bad));
            out.printf("%s\tall\t%.9g\t%.9g\t%llu\t%llu\n", w.name, rhat, ess, (unsigned long long)used, (unsigned long long)bad);
            for (int k = 0; k < n; ++k) out.printf("%s\t%d\t%.17g\t%.17g\n", w.name, k, mean[(size_t)k], sd[(size_t)k]);
        }
        out.close();
    }
};

}  // namespace hammlet

#endif
