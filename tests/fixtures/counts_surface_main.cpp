// TEST INFRASTRUCTURE: hammlet::Posterior::regionCounts, ::countsInfo and ::writeCountsFile (include/hammlet/Posterior.hpp)
// from C++, for tests/test_gpu_counts_surface.py: a chain over a float32 file, three sweeps, then regionCounts() over five
// regions fixed by T, every double printed as its 64 bits in hexadecimal, and the same regions written to a file.
// argv: FILE K SEED MAX_BREAKS OUT.  stdout: "start ...", "end ..." (decimal), "hist ...", "whole_state ...", "avoid ...",
// "degenerate <n>", "info <regions> <steps> <longest>"
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
    if (argc != 6) { fprintf(stderr, "usage: FILE K SEED MAX_BREAKS OUT\n"); return 2; }
    hml_ctx* ctx = nullptr;
    try {
        FILE* in = fopen(argv[1], "rb");
        if (!in) throw std::runtime_error("cannot read the input");
        std::vector<float> x;
        float buf[4096];
        for (size_t n; (n = fread(buf, sizeof(float), 4096, in)) > 0;) x.insert(x.end(), buf, buf + n);
        fclose(in);
        const int K = atoi(argv[2]);
        const uint32_t T = (uint32_t)x.size(), H = (uint32_t)atoi(argv[4]);
        check(hml_create(&ctx, 0, (uint64_t)atoll(argv[3]), 0, nullptr));
        check(hml_load_observations(ctx, x.data(), x.size()));
        float nig[4];
        check(hml_autoprior(ctx, 0.2f, 0.9f, nig));
        check(hml_set_model(ctx, K, nig, 0.5f, 0.5f, 0.5f, 1));
        check(hml_sample_prior(ctx));
        check(hml_iterate(ctx, 'F', 3, 0));
        check(hml_sync(ctx));
        hammlet::Posterior post(ctx);
        const std::vector<uint32_t> start = {0, 0, T / 4, 100, T / 2}, end = {T, 1, 3 * (T / 4), 101, T / 2 + 1000};
        const hammlet::Posterior::RegionCounts r = post.regionCounts(start, end, H, K);
        const hammlet::Posterior::CountsInfo info = post.countsInfo();
        print_positions("start", start);
        print_positions("end", end);
        print_doubles("hist", r.hist);
        print_doubles("whole_state", r.wholeState);
        print_doubles("avoid", r.avoid);
        printf("degenerate %llu\n", (unsigned long long)r.countDegenerate);
        printf("info %llu %llu %llu\n", (unsigned long long)info.regions, (unsigned long long)info.steps, (unsigned long long)info.longest);
        post.writeCountsFile(argv[5], start, end, H, K);
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        if (ctx) hml_destroy(ctx);
        return 1;
    }
    hml_destroy(ctx);
    return 0;
}
