// TEST INFRASTRUCTURE: hml_history_stats_compute (hammlet_amd/csrc/hml_history_stats.h) as a stand-alone program, for
// tests/test_history_stats_cpu.py - built once plainly and once with the address and undefined-behaviour sanitizers.
// stdin:  n_chains n, then n_chains * n values (chain-major; "inf", "nan" are read by strtod)
// stdout: "ok rhat ess n_nonfinite", then one line "mean sd" per chain, %.17g - or "error <message>" (exit status 2)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hammlet_amd/csrc/hml_history_stats.h"

int main() {
    long long chains = 0, n = 0;
    if (scanf("%lld %lld", &chains, &n) != 2 || chains < 0 || n < 0 || chains > (1 << 20) || n > (1ll << 32)) { printf("error bad header\n"); return 2; }
    std::vector<double> x((size_t)(chains * n));
    char tok[128];
    for (size_t i = 0; i < x.size(); ++i) {
        if (scanf("%127s", tok) != 1) { printf("error short input\n"); return 2; }
        x[i] = strtod(tok, nullptr);
    }
    std::vector<double> mean((size_t)chains), sd((size_t)chains);
    double rhat = 0.0, ess = 0.0;
    uint64_t bad = 0;
    const char* why = nullptr;
    if (hml_history_stats_compute(x.data(), (int)chains, (uint64_t)n, &rhat, &ess, mean.data(), sd.data(), &bad, &why)) {
        printf("error %s\n", why ? why : "?");
        return 2;
    }
    printf("ok %.17g %.17g %llu\n", rhat, ess, (unsigned long long)bad);
    for (long long c = 0; c < chains; ++c) printf("%.17g %.17g\n", mean[(size_t)c], sd[(size_t)c]);
    return 0;
}
