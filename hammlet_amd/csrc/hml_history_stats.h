// Convergence diagnostics of one scalar of the chains' history (hml_history_stats, include/hml.h): split R-hat and the
// effective sample size by Geyer's initial monotone sequence, over n_chains series of n values each.  No HIP in here: a
// host compiler alone builds it (tests/test_history_stats_cpu.py builds it twice, once with the sanitizers).
//
//   every chain is split in halves (n odd: the middle value is dropped): m = 2 n_chains sequences of length h = n / 2
//   W     = mean over the sequences of their sample variances (divisor h - 1)
//   B     = h / (m - 1) sum_j (mean_j - mean)^2,  mean = the mean of the mean_j
//   var+  = (h - 1) / h W + B / h
//   R-hat = sqrt(var+ / W)
//   rho_t = 1 - (W - mean_j acov_j(t)) / var+,  acov_j(t) = 1 / h sum_i (x_i - mean_j) (x_{i + t} - mean_j), direct sums
//   P_0   = 1 + rho_1,  P_k = rho_2k + rho_2k+1; the sum stops before the first P_k < 0 or when 2 k + 1 > h - 1, and P_k is
//           replaced by min(P_k, P_k-1)
//   tau   = -1 + 2 sum P_k,  ESS = m h / tau
//
// Values that are not finite are counted; one of them makes R-hat and ESS not-a-number.  chain_mean / chain_sd (divisor:
// count - 1) are taken over the finite values of a chain.  A constant series (W = 0) gives not-a-number twice.
#ifndef HML_HISTORY_STATS_H
#define HML_HISTORY_STATS_H

#include <math.h>
#include <stdint.h>

#include <vector>

// 0, or 1 with *why set: fewer than one chain, or fewer than four values per half
inline int hml_history_stats_compute(const double* x, int n_chains, uint64_t n, double* rhat, double* ess, double* chain_mean,
                                     double* chain_sd, uint64_t* n_nonfinite, const char** why) {
    const double nan = NAN;
    if (why) *why = nullptr;
    if (!x || n_chains < 1) { if (why) *why = "history statistics: at least one chain"; return 1; }
    const uint64_t h = n / 2;
    if (h < 4) { if (why) *why = "history statistics: at least 8 values per chain (two halves of 4)"; return 1; }
    uint64_t bad = 0;
    for (int c = 0; c < n_chains; ++c) {
        const double* xc = x + (uint64_t)c * n;
        double s = 0.0;
        uint64_t cnt = 0;
        for (uint64_t i = 0; i < n; ++i) if (isfinite(xc[i])) { s += xc[i]; ++cnt; }
        bad += n - cnt;
        const double mean = cnt ? s / (double)cnt : nan;
        double q = 0.0;
        for (uint64_t i = 0; i < n; ++i) if (isfinite(xc[i])) q += (xc[i] - mean) * (xc[i] - mean);
        if (chain_mean) chain_mean[c] = mean;
        if (chain_sd) chain_sd[c] = cnt >= 2 ? sqrt(q / (double)(cnt - 1)) : nan;
    }
    if (n_nonfinite) *n_nonfinite = bad;
    if (rhat) *rhat = nan;
    if (ess) *ess = nan;
    if (bad) return 0;
    const int m = 2 * n_chains;
    const double hd = (double)h;
    std::vector<const double*> seq((size_t)m);
    std::vector<double> mean_j((size_t)m);
    double W = 0.0, grand = 0.0;
    for (int j = 0; j < m; ++j) {
        seq[j] = x + (uint64_t)(j / 2) * n + ((j & 1) ? n - h : 0);
        double s = 0.0;
        for (uint64_t i = 0; i < h; ++i) s += seq[j][i];
        mean_j[j] = s / hd;
        double q = 0.0;
        for (uint64_t i = 0; i < h; ++i) q += (seq[j][i] - mean_j[j]) * (seq[j][i] - mean_j[j]);
        W += q / (hd - 1.0);
        grand += mean_j[j];
    }
    W /= (double)m;
    grand /= (double)m;
    double B = 0.0;
    for (int j = 0; j < m; ++j) B += (mean_j[j] - grand) * (mean_j[j] - grand);
    B *= hd / (double)(m - 1);
    const double var_plus = (hd - 1.0) / hd * W + B / hd;
    if (!(W > 0.0)) return 0;   // a constant series: neither is defined
    if (rhat) *rhat = sqrt(var_plus / W);
    auto rho = [&](uint64_t t) {
        double a = 0.0;
        for (int j = 0; j < m; ++j) {
            double s = 0.0;
            for (uint64_t i = 0; i + t < h; ++i) s += (seq[j][i] - mean_j[j]) * (seq[j][i + t] - mean_j[j]);
            a += s / hd;
        }
        return 1.0 - (W - a / (double)m) / var_plus;
    };
    double sum = 0.0, prev = 0.0;
    for (uint64_t k = 0; 2 * k + 1 <= h - 1; ++k) {
        double P = k == 0 ? 1.0 + rho(1) : rho(2 * k) + rho(2 * k + 1);
        if (P < 0.0) break;
        if (k > 0 && P > prev) P = prev;
        sum += P;
        prev = P;
    }
    const double tau = -1.0 + 2.0 * sum;
    if (ess) *ess = (double)m * hd / tau;
    return 0;
}

#endif
