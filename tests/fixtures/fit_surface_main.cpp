// TEST INFRASTRUCTURE: hammlet::Fit (include/hammlet/Fit.hpp) from C++, for tests/test_gpu_fit_surface.py: a chain over a
// float32 file, three sweeps, then expectedCounts(), step() and fit(), every double printed as its 64 bits in hexadecimal.
// argv: FILE K SEED.  stdout: "xi ...", "first ...", "stay ...", "occ ...", "sum ...", "sum_sq ...", "loglik <word>",
// "degenerate <n> <n>", "step <objective word> <kept>", "trace ...", "fit <steps> <reason name> <kept>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "hammlet/Fit.hpp"

static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

static void print_doubles(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) { uint64_t u; memcpy(&u, &x, sizeof u); printf(" %llx", (unsigned long long)u); }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: FILE K SEED\n"); return 2; }
    hml_ctx* ctx = nullptr;
    try {
        FILE* in = fopen(argv[1], "rb");
        if (!in) throw std::runtime_error("cannot read the input");
        std::vector<float> x;
        float buf[4096];
        for (size_t n; (n = fread(buf, sizeof(float), 4096, in)) > 0;) x.insert(x.end(), buf, buf + n);
        fclose(in);
        const int K = atoi(argv[2]);
        check(hml_create(&ctx, 0, (uint64_t)atoll(argv[3]), 0, nullptr));
        check(hml_load_observations(ctx, x.data(), x.size()));
        float nig[4];
        check(hml_autoprior(ctx, 0.2f, 0.9f, nig));
        check(hml_set_model(ctx, K, nig, 0.5f, 0.5f, 0.5f, 1));
        check(hml_sample_prior(ctx));
        check(hml_iterate(ctx, 'F', 3, 0));
        check(hml_sync(ctx));
        hammlet::Fit fit(ctx);
        const hammlet::Fit::Counts n = fit.expectedCounts();
        print_doubles("xi", n.xi);
        print_doubles("first", n.first);
        print_doubles("stay", n.stay);
        print_doubles("occ", n.occ);
        print_doubles("sum", n.sum);
        print_doubles("sum_sq", n.sumSq);
        print_doubles("loglik", std::vector<double>(1, n.loglik));
        printf("degenerate %llu %llu\n", (unsigned long long)n.degenerate, (unsigned long long)n.xiDegenerate);
        uint64_t kept = 0;
        const double objective = fit.step(true, &kept);
        uint64_t u;
        memcpy(&u, &objective, sizeof u);
        printf("step %llx %llu\n", (unsigned long long)u, (unsigned long long)kept);
        const hammlet::Fit::Result r = fit.fit(2, -1.0, false);
        print_doubles("trace", r.trace);
        printf("fit %llu %s %llu\n", (unsigned long long)r.steps, hammlet::Fit::reasonName(r.reason), (unsigned long long)r.kept);
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        if (ctx) hml_destroy(ctx);
        return 1;
    }
    hml_destroy(ctx);
    return 0;
}
