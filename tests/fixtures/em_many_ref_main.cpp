// TEST INFRASTRUCTURE: EM from many starts (hammlet_amd/csrc/hml_em_many_ref.h over hml_em_ref.h) as a stand-alone program, for
// tests/test_em_many_cpu.py and tests/test_gpu_em_many.py - built once plainly and once with the address and undefined-behaviour
// sanitizers.  Floats travel as their 32 bits and doubles as their 64 bits in hexadecimal.
// stdin, MODE "starts":  K P R seed(word) spread(word), then the current mean_var[2 P], A[K K], pi[K]
//                        -> "ok 1", "mean_var ..." (R 2 P), "A ..." (R K K), "pi ..." (R K); a refused spread: "ok 0"
//        MODE "best":    R, then reason[R] (decimal) and objective[R] (words) -> "best <n>"
//        MODE "fits":    R K D P self_trans B use_prior max_steps rel_tol(word), the prior's seven doubles, starts[B + 1],
//                        sum[D][B], sum_sq[D][B] as tests/fixtures/em_ref_main.cpp takes them, then per member mean_var[2 P],
//                        A[K K], pi[K] -> per member "trace ...", "steps <n>", "reason <n>", "kept <n>", "mean_var ...", "A ...",
//                        "pi ...", and at the end "best <n>": every member is hml_em_ref_fit from its start
// anything else: "error <message>", exit status 2
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hammlet_amd/csrc/hml_em_ref.h"
#include "../../hammlet_amd/csrc/hml_em_many_ref.h"

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

static bool read_word(uint64_t* u) {
    unsigned long long bits = 0;
    if (scanf("%llx", &bits) != 1) return false;
    *u = bits;
    return true;
}

static bool read_double(double* x) {
    uint64_t u = 0;
    if (!read_word(&u)) return false;
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

static int fail(const char* what) { printf("error %s\n", what); return 2; }

int main() {
    char mode[16];
    if (scanf("%15s", mode) != 1) return fail("no mode");
    if (strcmp(mode, "starts") == 0) {
        int K = 0, P = 0;
        unsigned long long R = 0;
        uint64_t seed = 0;
        double spread = 0.0;
        if (scanf("%d %d %llu", &K, &P, &R) != 3 || !read_word(&seed) || !read_double(&spread)) return fail("bad header");
        if (K < 1 || K > HML_CAP_K || P < 1 || P > K || R < 1 || R > HML_EM_MANY_MAX_R) return fail("bad sizes");
        std::vector<float> mv, A, pi;
        if (!read_floats(mv, 2 * (size_t)P) || !read_floats(A, (size_t)K * K) || !read_floats(pi, (size_t)K)) return fail("short input");
        std::vector<float> omv(R * 2 * P), oA(R * K * K), opi(R * K);
        const bool ok = hml_em_many_starts(K, P, R, seed, spread, mv.data(), A.data(), pi.data(), omv.data(), oA.data(), opi.data());
        printf("ok %d\n", ok ? 1 : 0);
        if (!ok) return 0;
        print_floats("mean_var", omv);
        print_floats("A", oA);
        print_floats("pi", opi);
        return 0;
    }
    if (strcmp(mode, "best") == 0) {
        unsigned long long R = 0;
        if (scanf("%llu", &R) != 1 || R < 1 || R > HML_EM_MANY_MAX_R) return fail("bad sizes");
        std::vector<int> reason(R);
        std::vector<double> objective(R);
        for (auto& r : reason)
            if (scanf("%d", &r) != 1) return fail("short input");
        for (auto& o : objective)
            if (!read_double(&o)) return fail("short input");
        printf("best %lld\n", (long long)hml_em_many_best(R, reason.data(), objective.data()));
        return 0;
    }
    if (strcmp(mode, "fits") != 0) return fail("unknown mode");
    hml_post_ref_case c;
    unsigned long long R = 0, max_steps = 0;
    long long B = 0;
    int use_prior = 0;
    double rel_tol = 0.0;
    if (scanf("%llu %d %d %d %d %lld %d %llu", &R, &c.K, &c.D, &c.P, &c.self_trans, &B, &use_prior, &max_steps) != 8 || !read_double(&rel_tol)) return fail("bad header");
    if (R < 1 || R > HML_EM_MANY_MAX_R || c.K < 1 || c.K > HML_POST_CAP_K || c.D < 1 || c.D > HML_POST_MAX_D || c.P < 1 || c.P > c.K || B < 1 || B > (1ll << 28) ||
        max_steps > 100000)
        return fail("bad sizes");
    hml_em_prior pr;
    if (!read_double(&pr.alpha) || !read_double(&pr.beta) || !read_double(&pr.mu0) || !read_double(&pr.nu) || !read_double(&pr.a_off) || !read_double(&pr.a_diag) ||
        !read_double(&pr.pi_alpha))
        return fail("bad prior");
    c.B = (uint64_t)B;
    c.starts.resize(c.B + 1);
    for (uint64_t i = 0; i <= c.B; ++i) {
        unsigned int s = 0;
        if (scanf("%u", &s) != 1) return fail("short input");
        c.starts[i] = s;
        if (i > 0 && c.starts[i] <= c.starts[i - 1]) return fail("starts not ascending");
    }
    if (!read_floats(c.sum, (size_t)c.D * c.B) || !read_floats(c.sum_sq, (size_t)c.D * c.B)) return fail("short input");
    std::vector<int> reasons(R);
    std::vector<double> objectives(R);
    for (unsigned long long r = 0; r < R; ++r) {
        if (!read_floats(c.mean_var, 2 * (size_t)c.P) || !read_floats(c.A, (size_t)c.K * c.K) || !read_floats(c.pi, (size_t)c.K)) return fail("short input");
        std::vector<double> trace;
        uint64_t steps = 0, kept = 0;
        hml_em_ref_fit(c, use_prior, pr, max_steps, rel_tol, trace, &steps, &reasons[r], &kept);
        objectives[r] = trace.back();
        print_doubles("trace", trace);
        printf("steps %llu\nreason %d\nkept %llu\n", (unsigned long long)steps, reasons[r], (unsigned long long)kept);
        print_floats("mean_var", c.mean_var);
        print_floats("A", c.A);
        print_floats("pi", c.pi);
    }
    printf("best %lld\n", (long long)hml_em_many_best(R, reasons.data(), objectives.data()));
    return 0;
}
