// TEST INFRASTRUCTURE: the expectation-maximisation restatement for one host thread (hammlet_amd/csrc/hml_em_ref.h) as a
// stand-alone program, for tests/test_em_cpu.py and tests/test_gpu_em.py - built once plainly and once with the address and
// undefined-behaviour sanitizers.  Floats travel as their 32 bits and doubles as their 64 bits in hexadecimal.
// stdin:  MODE K D P self_trans B use_prior max_steps rel_tol(word), the prior's seven doubles (alpha beta mu0 nu a_off a_diag
//         pi_alpha, words), then starts[B + 1] (decimal), sum[D][B], sum_sq[D][B], mean_var[2 P], A[K K], pi[K]
// MODE "estep": -> "xi ...", "first ...", "stay ...", "occ ...", "sx ...", "sxx ...", "loglik <word>", "degenerate <n>",
//                  "xi_degenerate <n>", "seconds <s>"
// MODE "step":  one E-step and M-step -> "objective <word>", "kept <n>", "mean_var ...", "A ...", "pi ..."
// MODE "fit":   -> "trace ...", "steps <n>", "reason <n>", "kept <n>", "mean_var ...", "A ...", "pi ..."
// anything else: "error <message>", exit status 2
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hammlet_amd/csrc/hml_em_ref.h"

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

static bool read_double(double* x) {
    unsigned long long bits = 0;
    if (scanf("%llx", &bits) != 1) return false;
    uint64_t u = bits;
    memcpy(x, &u, sizeof u);
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
    const bool estep = strcmp(mode, "estep") == 0, step = strcmp(mode, "step") == 0, fit = strcmp(mode, "fit") == 0;
    if (!estep && !step && !fit) { printf("error unknown mode\n"); return 2; }
    hml_post_ref_case c;
    long long B = 0;
    int use_prior = 0;
    unsigned long long max_steps = 0;
    double rel_tol = 0.0;
    if (scanf("%d %d %d %d %lld %d %llu", &c.K, &c.D, &c.P, &c.self_trans, &B, &use_prior, &max_steps) != 7 || !read_double(&rel_tol)) { printf("error bad header\n"); return 2; }
    if (c.K < 1 || c.K > HML_POST_CAP_K || c.D < 1 || c.D > HML_POST_MAX_D || c.P < 1 || c.P > c.K || B < 1 || B > (1ll << 28) || max_steps > 100000) {
        printf("error bad sizes\n");
        return 2;
    }
    hml_em_prior pr;
    if (!read_double(&pr.alpha) || !read_double(&pr.beta) || !read_double(&pr.mu0) || !read_double(&pr.nu) || !read_double(&pr.a_off) || !read_double(&pr.a_diag) ||
        !read_double(&pr.pi_alpha)) { printf("error bad prior\n"); return 2; }
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
    if (estep) {
        hml_em_counts n;
        const auto t0 = std::chrono::steady_clock::now();
        hml_em_ref_estep(c, n);
        const auto t1 = std::chrono::steady_clock::now();
        print_doubles("xi", n.xi);
        print_doubles("first", n.first);
        print_doubles("stay", n.stay);
        print_doubles("occ", n.occ);
        print_doubles("sx", n.sx);
        print_doubles("sxx", n.sxx);
        print_doubles("loglik", std::vector<double>(1, n.loglik));
        printf("degenerate %llu\nxi_degenerate %llu\n", (unsigned long long)n.degenerate, (unsigned long long)n.xi_degenerate);
        printf("seconds %.6f\n", std::chrono::duration<double>(t1 - t0).count());
        return 0;
    }
    unsigned long long kept = 0;
    if (step) {
        hml_em_counts n;
        hml_em_ref_estep(c, n);
        print_doubles("objective", std::vector<double>(1, hml_em_objective(c.K, c.P, use_prior, pr, n.loglik, c.mean_var.data(), c.A.data(), c.pi.data())));
        kept = hml_em_mstep(c.K, c.D, c.P, c.self_trans, use_prior, pr, n, c.mean_var.data(), c.A.data(), c.pi.data());
    } else {
        std::vector<double> trace;
        uint64_t steps = 0, k = 0;
        int reason = -1;
        hml_em_ref_fit(c, use_prior, pr, max_steps, rel_tol, trace, &steps, &reason, &k);
        kept = k;
        print_doubles("trace", trace);
        printf("steps %llu\nreason %d\n", (unsigned long long)steps, reason);
    }
    printf("kept %llu\n", kept);
    print_floats("mean_var", c.mean_var);
    print_floats("A", c.A);
    print_floats("pi", c.pi);
    return 0;
}
