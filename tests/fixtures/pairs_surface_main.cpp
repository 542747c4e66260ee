// TEST INFRASTRUCTURE: hammlet::Posterior::breaks and ::regions (include/hammlet/Posterior.hpp) from C++, for
// tests/test_gpu_pairs_surface.py: a chain over a float32 file, three sweeps, then breaks(MIN_PROB) and regions() over five
// regions fixed by T, every double printed as its 64 bits in hexadecimal.
// argv: FILE K SEED MIN_PROB.  stdout: "pos ..." (decimal), "prob ...", "breaks <expected word> <pair_degenerate>",
// "start ...", "end ..." (decimal), "whole ...", "whole_state ...", "expected_breaks ...", "share ...", "degenerate <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "hammlet/Posterior.hpp"

static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

static void print_doubles(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) { uint64_t u; memcpy(&u, &x, sizeof u); printf(" %llx", (unsigned long long)u); }
    printf("\n");
}

static void print_positions(const char* name, const std::vector<uint32_t>& v) {
    printf("%s", name);
    for (uint32_t x : v) printf(" %u", x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: FILE K SEED MIN_PROB\n"); return 2; }
    hml_ctx* ctx = nullptr;
    try {
        FILE* in = fopen(argv[1], "rb");
        if (!in) throw std::runtime_error("cannot read the input");
        std::vector<float> x;
        float buf[4096];
        for (size_t n; (n = fread(buf, sizeof(float), 4096, in)) > 0;) x.insert(x.end(), buf, buf + n);
        fclose(in);
        const int K = atoi(argv[2]);
        const uint32_t T = (uint32_t)x.size();
        check(hml_create(&ctx, 0, (uint64_t)atoll(argv[3]), 0, nullptr));
        check(hml_load_observations(ctx, x.data(), x.size()));
        float nig[4];
        check(hml_autoprior(ctx, 0.2f, 0.9f, nig));
        check(hml_set_model(ctx, K, nig, 0.5f, 0.5f, 0.5f, 1));
        check(hml_sample_prior(ctx));
        check(hml_iterate(ctx, 'F', 3, 0));
        check(hml_sync(ctx));
        hammlet::Posterior post(ctx);
        const hammlet::Posterior::Breaks b = post.breaks(atof(argv[4]));
        print_positions("pos", b.position);
        print_doubles("prob", b.probability);
        uint64_t u;
        memcpy(&u, &b.expectedBreaks, sizeof u);
        printf("breaks %llx %llu\n", (unsigned long long)u, (unsigned long long)b.pairDegenerate);
        const std::vector<uint32_t> start = {0, 0, T / 4, 100, T / 2}, end = {T, 1, 3 * (T / 4), 101, T / 2 + 1000};
        const hammlet::Posterior::Regions r = post.regions(start, end, K);
        print_positions("start", start);
        print_positions("end", end);
        print_doubles("whole", r.whole);
        print_doubles("whole_state", r.wholeState);
        print_doubles("expected_breaks", r.expectedBreaks);
        print_doubles("share", r.share);
        printf("degenerate %llu\n", (unsigned long long)r.pairDegenerate);
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        if (ctx) hml_destroy(ctx);
        return 1;
    }
    hml_destroy(ctx);
    return 0;
}
