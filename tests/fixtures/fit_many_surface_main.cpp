// TEST INFRASTRUCTURE: hammlet::Fit::starts, fitMany and writeStartsFile (include/hammlet/Fit.hpp) from C++, for
// tests/test_gpu_em_many_surface.py: a chain over a float32 file, three sweeps, then a batch of R generated starts, every double
// printed as its 64 bits and every float as its 32 bits in hexadecimal.
// argv: FILE K SEED R STARTS_SEED STEPS OUT.  stdout: "starts ..." (the generated means and variances), per member "trace ...",
// "member <steps> <reason name> <kept>", "mean_var ...", then "best <n>", "installed ..." (the context's theta afterwards); the
// starts file goes to OUT
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

static void print_floats(const char* name, const float* v, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; ++i) { uint32_t u; memcpy(&u, v + i, sizeof u); printf(" %x", (unsigned)u); }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: FILE K SEED R STARTS_SEED STEPS OUT\n"); return 2; }
    hml_ctx* ctx = nullptr;
    try {
        FILE* in = fopen(argv[1], "rb");
        if (!in) throw std::runtime_error("cannot read the input");
        std::vector<float> x;
        float buf[4096];
        for (size_t n; (n = fread(buf, sizeof(float), 4096, in)) > 0;) x.insert(x.end(), buf, buf + n);
        fclose(in);
        const int K = atoi(argv[2]);
        const uint64_t R = (uint64_t)atoll(argv[4]), steps = (uint64_t)atoll(argv[6]);
        check(hml_create(&ctx, 0, (uint64_t)atoll(argv[3]), 0, nullptr));
        check(hml_load_observations(ctx, x.data(), x.size()));
        float nig[4];
        check(hml_autoprior(ctx, 0.2f, 0.9f, nig));
        check(hml_set_model(ctx, K, nig, 0.5f, 0.5f, 0.5f, 1));
        check(hml_sample_prior(ctx));
        check(hml_iterate(ctx, 'F', 3, 0));
        check(hml_sync(ctx));
        hammlet::Fit fit(ctx);
        const hammlet::Fit::Starts s = fit.starts(R, (uint64_t)atoll(argv[5]));
        print_floats("starts", s.meanVar.data(), s.meanVar.size());
        const hammlet::Fit::ManyResult m = fit.fitMany(s, steps, 0.0, false);
        for (uint64_t r = 0; r < R; ++r) {
            print_doubles("trace", m.members[r].trace);
            printf("member %llu %s %llu\n", (unsigned long long)m.members[r].steps, hammlet::Fit::reasonName(m.members[r].reason), (unsigned long long)m.members[r].kept);
            print_floats("mean_var", m.fitted.meanVar.data() + r * 2 * K, 2 * (size_t)K);
        }
        printf("best %lld\n", (long long)m.best);
        std::vector<float> mv(2 * (size_t)K);
        check(hml_get_theta(ctx, mv.data()));
        print_floats("installed", mv.data(), mv.size());
        fit.writeStartsFile(argv[7], m);
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        if (ctx) hml_destroy(ctx);
        return 1;
    }
    hml_destroy(ctx);
    return 0;
}
