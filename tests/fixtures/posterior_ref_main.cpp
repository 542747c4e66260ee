// TEST INFRASTRUCTURE: the smoothing restatement for one host thread (hammlet_amd/csrc/hml_posterior_ref.h) as a stand-alone
// program, for tests/test_posterior_cpu.py and tests/test_gpu_posterior.py - built once plainly and once with the address and
// undefined-behaviour sanitizers.  Floats travel as their 32 bits and doubles as their 64 bits in hexadecimal, so not-a-number
// and infinities pass and every comparison is one of words.
// stdin:  "case" K D P self_trans B want_rows, then starts[B + 1] (decimal), sum[D][B], sum_sq[D][B], mean_var[2 P], A[K K], pi[K]
//         -> stdout: lines "m ...", "e ...", "alpha ...", "c ...", "beta ...", "gamma ..." (these six if want_rows), "loglik <word>",
//            "degenerate <n>", "state ...", "run_len ...", "run_state ...", "run_conf ...", "seconds <tables> <smoothing>"
// anything else: "error <message>", exit status 2
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hammlet_amd/csrc/hml_posterior_ref.h"

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

static void print_floats(const char* name, const std::vector<float>& v) {
    printf("%s", name);
    for (float x : v) { uint32_t u; memcpy(&u, &x, sizeof u); printf(" %x", (unsigned)u); }
    printf("\n");
}

static void print_doubles(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) { uint64_t u; memcpy(&u, &x, sizeof u); printf(" %llx", (unsigned long long)u); }
    printf("\n");
}

int main() {
    char mode[16];
    if (scanf("%15s", mode) != 1) { printf("error no mode\n"); return 2; }
    if (strcmp(mode, "case") != 0) { printf("error unknown mode\n"); return 2; }
    hml_post_ref_case c;
    long long B = 0;
    int want_rows = 0;
    if (scanf("%d %d %d %d %lld %d", &c.K, &c.D, &c.P, &c.self_trans, &B, &want_rows) != 6) { printf("error bad header\n"); return 2; }
    if (c.K < 1 || c.K > HML_POST_CAP_K || c.D < 1 || c.D > HML_POST_MAX_D || c.P < 1 || c.P > c.K || B < 1 || B > (1ll << 28)) { printf("error bad sizes\n"); return 2; }
    c.B = (uint64_t)B;
    c.starts.resize(c.B + 1);
    for (uint64_t i = 0; i <= c.B; ++i) {
        unsigned int s = 0;
        if (scanf("%u", &s) != 1) { printf("error short input\n"); return 2; }
        c.starts[i] = s;
        if (i > 0 && c.starts[i] <= c.starts[i - 1]) { printf("error starts not ascending\n"); return 2; }
    }
    if (!read_floats(c.sum, (size_t)c.D * c.B) || !read_floats(c.sum_sq, (size_t)c.D * c.B) || !read_floats(c.mean_var, 2 * (size_t)c.P) ||
        !read_floats(c.A, (size_t)c.K * c.K) || !read_floats(c.pi, (size_t)c.K)) { printf("error short input\n"); return 2; }
    hml_post_ref_result r;
    const auto t0 = std::chrono::steady_clock::now();
    hml_post_ref_tables(c, r.e, r.m);
    const auto t1 = std::chrono::steady_clock::now();
    hml_post_ref_smooth(c, r);
    const auto t2 = std::chrono::steady_clock::now();
    if (want_rows) {
        print_floats("m", r.m);
        print_floats("e", r.e);
        print_doubles("alpha", r.alpha);
        print_doubles("c", r.c);
        print_doubles("beta", r.beta);
        print_doubles("gamma", r.gamma);
    }
    print_doubles("loglik", std::vector<double>(1, r.loglik));
    printf("degenerate %llu\n", (unsigned long long)r.degenerate);
    printf("state");
    for (int16_t s : r.state) printf(" %d", (int)s);
    printf("\nrun_len");
    for (uint64_t l : r.run_len) printf(" %llu", (unsigned long long)l);
    printf("\nrun_state");
    for (int32_t s : r.run_state) printf(" %d", (int)s);
    printf("\n");
    print_doubles("run_conf", r.run_conf);
    printf("seconds %.6f %.6f\n", std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count());
    return 0;
}
