// Fit - expectation-maximisation over the chain's current blocks (include/hml.h, hml_expected_counts, hml_em_step, hml_em_fit;
// no counterpart in the reference): the expected counts of the E-step, one step, the fit of theta, A and pi to a mode of
// log p(y | theta) - or of that plus the log density of the chain's own priors -, and the file the driver writes from a fit:
//   PREFIXemSUFFIX   `-O EM`: "step<TAB>objective" (%.17g) per trace entry - the objective of the parameters after that many
//                    M-steps -, then "reason<TAB>max_steps|converged|degenerate", "kept<TAB>n", "means<TAB>...",
//                    "variances<TAB>..." (one value per emission parameter, %.9g), "A<TAB>..." per row and "pi<TAB>..."
//   PREFIXemstartsSUFFIX   `-O EMS`: the batch of `-em-starts` (hml_em_starts, hml_em_fit_many) - one line per member,
//                    tab-separated: index, objective (%.17g), steps, reason, kept, the fitted means, the fitted variances (%.9g),
//                    and "*" as a last field on the winner's line
// A thin handle over a context that something else owns, next to Viterbi and Posterior.  Blocks are never rebuilt inside a
// fit: it is over the context's current block structure; call hml_create_blocks between fits to let the threshold follow.
#ifndef HAMMLET_FIT_HPP
#define HAMMLET_FIT_HPP

#include <stdexcept>
#include <string>
#include <vector>

#include "../hml.h"
#include "TextFile.hpp"

namespace hammlet {

class Fit {
    hml_ctx* mCtx;
    static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }
    // data dimensions D, emission parameters P and states K = P^D of the context's model
    void shape(int* D, int* P, int* K) const {
        check(hml_get_dimensions(mCtx, D, P));
        *K = 1;
        for (int d = 0; d < *D; ++d) *K *= *P;
    }

public:
    struct Counts {
        std::vector<double> xi, first, stay, occ, sum, sumSq;   // [K][K], [K], [K], [K], [K][D], [K][D]
        double loglik = 0;
        uint64_t degenerate = 0, xiDegenerate = 0;
    };
    struct Result {
        std::vector<double> trace;   // steps + 1 values; the last belongs to the installed parameters
        uint64_t steps = 0, kept = 0;
        int reason = HML_EM_MAX_STEPS;
    };

    explicit Fit(hml_ctx* ctx) : mCtx(ctx) {}
    // the E-step alone; the chain is only read
    Counts expectedCounts() const {
        int D = 1, P = 0, K = 0;
        shape(&D, &P, &K);
        Counts n;
        n.xi.resize((size_t)K * K); n.first.resize(K); n.stay.resize(K); n.occ.resize(K);
        n.sum.resize((size_t)K * D); n.sumSq.resize((size_t)K * D);
        check(hml_expected_counts(mCtx, n.xi.data(), n.first.data(), n.stay.data(), n.occ.data(), n.sum.data(), n.sumSq.data(), &n.loglik, &n.degenerate, &n.xiDegenerate));
        return n;
    }
    // one E-step, M-step and installation; returns the objective of the parameters the step started from
    double step(bool usePrior = false, uint64_t* kept = nullptr) {
        double objective = 0;
        check(hml_em_step(mCtx, usePrior ? 1 : 0, &objective, kept));
        return objective;
    }
    Result fit(uint64_t maxSteps, double relTol = 0.0, bool usePrior = false) {
        Result r;
        r.trace.resize(maxSteps + 1);
        check(hml_em_fit(mCtx, usePrior ? 1 : 0, maxSteps, relTol, r.trace.data(), &r.steps, &r.reason, &r.kept));
        r.trace.resize(r.steps + 1);
        return r;
    }
    static const char* reasonName(int reason) {
        return reason == HML_EM_CONVERGED ? "converged" : reason == HML_EM_DEGENERATE ? "degenerate" : "max_steps";
    }

    // ---- EM from many starts (hml_em_starts, hml_em_fit_many): member r is set-parameters(start r) + fit(), word for word ----
    struct Starts {
        std::vector<float> meanVar, A, pi;   // [R][2 P], [R][K][K], [R][K]
        uint64_t n = 0;
    };
    struct ManyResult {
        std::vector<Result> members;         // every member's trace (steps + 1 values), steps, kept, reason
        std::vector<double> objective;       // a member's last trace entry
        Starts fitted;                       // every member's fitted parameters
        int64_t best = -1;                   // -1: no member is a candidate, the chain's parameters were left alone
        // the winner's trace as fit() would have returned it (best >= 0)
        const Result& winner() const { return members.at((size_t)best); }
    };
    // member 0 the current parameters, the others drawn around the current means (spread: finite, positive)
    Starts starts(uint64_t n, uint64_t seed, double spread = 1.0) const {
        int D = 1, P = 0, K = 0;
        shape(&D, &P, &K);
        Starts s;
        s.n = n;
        s.meanVar.resize(n * 2 * P); s.A.resize(n * K * K); s.pi.resize(n * K);
        check(hml_em_starts(mCtx, n, seed, spread, s.meanVar.data(), s.A.data(), s.pi.data()));
        return s;
    }
    ManyResult fitMany(const Starts& s, uint64_t maxSteps, double relTol = 0.0, bool usePrior = false, bool install = true) {
        int D = 1, P = 0, K = 0;
        shape(&D, &P, &K);
        const uint64_t R = s.n;
        ManyResult m;
        m.fitted.n = R;
        m.fitted.meanVar.resize(R * 2 * P); m.fitted.A.resize(R * K * K); m.fitted.pi.resize(R * K);
        m.objective.resize(R);
        std::vector<double> trace(R * (maxSteps + 1));
        std::vector<uint64_t> steps(R), kept(R);
        std::vector<int> reason(R);
        check(hml_em_fit_many(mCtx, R, s.meanVar.data(), s.A.data(), s.pi.data(), usePrior ? 1 : 0, maxSteps, relTol, install ? 1 : 0, trace.data(), steps.data(),
                              reason.data(), kept.data(), m.fitted.meanVar.data(), m.fitted.A.data(), m.fitted.pi.data(), m.objective.data(), &m.best));
        m.members.resize(R);
        for (uint64_t r = 0; r < R; ++r) {
            m.members[r].trace.assign(trace.begin() + r * (maxSteps + 1), trace.begin() + r * (maxSteps + 1) + steps[r] + 1);
            m.members[r].steps = steps[r]; m.members[r].kept = kept[r]; m.members[r].reason = reason[r];
        }
        return m;
    }
    // `-O EMS`: one line per member - index, objective (%.17g), steps, reason, kept, then the fitted means and the fitted
    // variances (%.9g) -, a "*" as the last field of the winner's line
    void writeStartsFile(const std::string& fn, const ManyResult& m) const {
        int D = 1, P = 0, K = 0;
        shape(&D, &P, &K);
        TextFile out(fn);
        for (size_t r = 0; r < m.members.size(); ++r) {
            const Result& f = m.members[r];
            out.printf("%llu\t%.17g\t%llu\t%s\t%llu", (unsigned long long)r, m.objective[r], (unsigned long long)f.steps, reasonName(f.reason), (unsigned long long)f.kept);
            for (int p = 0; p < P; ++p) out.printf("\t%.9g", (double)m.fitted.meanVar[r * 2 * P + 2 * p]);
            for (int p = 0; p < P; ++p) out.printf("\t%.9g", (double)m.fitted.meanVar[r * 2 * P + 2 * p + 1]);
            out.printf((int64_t)r == m.best ? "\t*\n" : "\n");
        }
        out.close();
    }

    // the fit's trace and the context's parameters as they are now
    void writeFile(const std::string& fn, const Result& r) const {
        int D = 1, P = 0, K = 0;
        shape(&D, &P, &K);
        std::vector<float> mv(2 * (size_t)P), A((size_t)K * K), pi(K);
        check(hml_get_theta(mCtx, mv.data()));
        check(hml_get_transitions(mCtx, A.data(), pi.data()));
        TextFile out(fn);
        for (size_t k = 0; k < r.trace.size(); ++k) out.printf("%llu\t%.17g\n", (unsigned long long)k, r.trace[k]);
        out.printf("reason\t%s\nkept\t%llu\n", reasonName(r.reason), (unsigned long long)r.kept);
        out.printf("means");
        for (int p = 0; p < P; ++p) out.printf("\t%.9g", (double)mv[2 * p]);
        out.printf("\nvariances");
        for (int p = 0; p < P; ++p) out.printf("\t%.9g", (double)mv[2 * p + 1]);
        out.printf("\n");
        for (int i = 0; i < K; ++i) {
            out.printf("A");
            for (int j = 0; j < K; ++j) out.printf("\t%.9g", (double)A[(size_t)i * K + j]);
            out.printf("\n");
        }
        out.printf("pi");
        for (int j = 0; j < K; ++j) out.printf("\t%.9g", (double)pi[j]);
        out.printf("\n");
        out.close();
    }
};

}  // namespace hammlet

#endif
