// TEST INFRASTRUCTURE: the count read-outs of the smoothing restated for one host thread (hammlet_amd/csrc/hml_counts_ref.h)
// as a stand-alone program, for tests/test_counts_cpu.py and tests/test_gpu_counts.py - built once plainly and once with the
// address and undefined-behaviour sanitizers.  Floats travel as their 32 bits, doubles as their 64 bits, in hexadecimal.
// stdin:  "counts" K D P self_trans B n_regions H, then starts[B + 1] (decimal), sum[D][B], sum_sq[D][B], mean_var[2 P], A[K K],
//         pi[K], then start[n_regions] and end[n_regions] (decimal)
// stdout: "v ..." [B][K], "rho ..." [B][K], "gamma ..." [B][K], "count_degenerate <n>", then per region in order "hist ..."
//         [n][H + 1], "whole_state ..." [n][K], "avoid ..." [n][K], then "steps <sum of be - ba>", "longest <largest be - ba>" and
//         "seconds <s>"
// anything else: "error <message>", exit status 2
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hammlet_amd/csrc/hml_counts_ref.h"

static bool read_floats(std::vector<float>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i) {
        unsigned int bits = 0;
        if (scanf("%x", &bits) != 1) return false;
        uint32_t u = bits;
        memcpy(&v[i], &u, sizeof u);
    }
    return true;
}

static void print_doubles(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) { uint64_t u; memcpy(&u, &x, sizeof u); printf(" %llx", (unsigned long long)u); }
    printf("\n");
}

int main() {
    char mode[16];
    if (scanf("%15s", mode) != 1 || strcmp(mode, "counts") != 0) { printf("error unknown mode\n"); return 2; }
    hml_post_ref_case c;
    long long B = 0, n_regions = 0, H = 0;
    if (scanf("%d %d %d %d %lld %lld %lld", &c.K, &c.D, &c.P, &c.self_trans, &B, &n_regions, &H) != 7) { printf("error bad header\n"); return 2; }
    if (c.K < 1 || c.K > HML_POST_CAP_K || c.D < 1 || c.D > HML_POST_MAX_D || c.P < 1 || c.P > c.K || B < 1 || B > (1ll << 28) || n_regions < 0 ||
        n_regions > (1ll << 24) || H < 0 || H > (1ll << 31)) {
        printf("error bad sizes\n");
        return 2;
    }
    if (!hml_counts_h_ok(c.K, (uint32_t)H)) { printf("error " HML_COUNTS_H_RULE "\n"); return 2; }
    c.B = (uint64_t)B;
    c.starts.resize(c.B + 1);
    for (uint64_t i = 0; i <= c.B; ++i) {
        unsigned int s = 0;
        if (scanf("%u", &s) != 1) { printf("error short input\n"); return 2; }
        c.starts[i] = s;
        if (i > 0 && c.starts[i] <= c.starts[i - 1]) { printf("error starts not ascending\n"); return 2; }
    }
    if (c.starts[0] != 0) { printf("error starts[0] is not 0\n"); return 2; }
    if (!read_floats(c.sum, (size_t)c.D * c.B) || !read_floats(c.sum_sq, (size_t)c.D * c.B) || !read_floats(c.mean_var, 2 * (size_t)c.P) ||
        !read_floats(c.A, (size_t)c.K * c.K) || !read_floats(c.pi, (size_t)c.K)) { printf("error short input\n"); return 2; }
    std::vector<uint32_t> rs((size_t)n_regions), re((size_t)n_regions);
    for (int part = 0; part < 2; ++part)
        for (long long i = 0; i < n_regions; ++i) {
            unsigned int s = 0;
            if (scanf("%u", &s) != 1) { printf("error short input\n"); return 2; }
            (part ? re : rs)[(size_t)i] = s;
        }
    for (long long i = 0; i < n_regions; ++i)
        if (!hml_pairs_region_ok(rs[(size_t)i], re[(size_t)i], c.starts[c.B])) { printf("error bad region\n"); return 2; }
    hml_counts_ref_terms t;
    const auto t0 = std::chrono::steady_clock::now();
    hml_counts_ref_terms_of(c, t);
    std::vector<double> hist, whole_state, avoid;
    hml_counts_ref_region g;
    uint64_t steps = 0, longest = 0;
    for (long long i = 0; i < n_regions; ++i) {
        hml_counts_ref_region_of(c, t, rs[(size_t)i], re[(size_t)i], (uint32_t)H, g);
        hist.insert(hist.end(), g.hist.begin(), g.hist.end());
        whole_state.insert(whole_state.end(), g.whole_state.begin(), g.whole_state.end());
        avoid.insert(avoid.end(), g.avoid.begin(), g.avoid.end());
        const uint64_t n = hml_counts_ref_steps(c, rs[(size_t)i], re[(size_t)i]);
        steps += n;
        if (n > longest) longest = n;
    }
    const auto t1 = std::chrono::steady_clock::now();
    print_doubles("v", t.v);
    print_doubles("rho", t.rho);
    print_doubles("gamma", t.gamma);
    printf("count_degenerate %llu\n", (unsigned long long)t.count_degenerate);
    print_doubles("hist", hist);
    print_doubles("whole_state", whole_state);
    print_doubles("avoid", avoid);
    printf("steps %llu\n", (unsigned long long)steps);
    printf("longest %llu\n", (unsigned long long)longest);
    printf("seconds %.6f\n", std::chrono::duration<double>(t1 - t0).count());
    return 0;
}
