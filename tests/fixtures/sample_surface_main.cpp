// TEST INFRASTRUCTURE: hammlet::Posterior::sample and ::sampleRegions (include/hammlet/Posterior.hpp) from C++, for
// tests/test_gpu_sample_surface.py: a chain over a float32 file, three sweeps, then COUNT draws from FIRST under SAMPLE_SEED with
// paths and state counts, the same draws over five regions fixed by T, and the run-length form of the first draw.
// argv: FILE K SEED FIRST COUNT SAMPLE_SEED.  stdout, all decimal: "paths ..." [COUNT][B], "segments ...", "score_fixed ...",
// "change_count ...", "state_count ...", "degenerate <n>", "start ...", "end ...", "hist ..." [5][4], "whole_state ..." [5][K],
// "breaks_sum ...", "breaks_sq ...", "run_len ...", "run_state ...", "info <draws> <groups> <group size>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "hammlet/Posterior.hpp"

static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

template <class T>
static void print_numbers(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (T x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: FILE K SEED FIRST COUNT SAMPLE_SEED\n"); return 2; }
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
        const uint64_t first = (uint64_t)atoll(argv[4]), count = (uint64_t)atoll(argv[5]), seed = (uint64_t)atoll(argv[6]);
        check(hml_create(&ctx, 0, (uint64_t)atoll(argv[3]), 0, nullptr));
        check(hml_load_observations(ctx, x.data(), x.size()));
        float nig[4];
        check(hml_autoprior(ctx, 0.2f, 0.9f, nig));
        check(hml_set_model(ctx, K, nig, 0.5f, 0.5f, 0.5f, 1));
        check(hml_sample_prior(ctx));
        check(hml_iterate(ctx, 'F', 3, 0));
        check(hml_sync(ctx));
        hammlet::Posterior post(ctx);
        const hammlet::Posterior::Sample s = post.sample(first, count, seed, true, true, K);
        print_numbers("paths", s.paths);
        print_numbers("segments", s.segments);
        print_numbers("score_fixed", s.scoreFixed);
        print_numbers("change_count", s.changeCount);
        print_numbers("state_count", s.stateCount);
        printf("degenerate %llu\n", (unsigned long long)s.degenerate);
        const std::vector<uint32_t> start = {0, 0, T / 4, 100, T / 2}, end = {T, 1, 3 * (T / 4), 101, T / 2 + 1000};
        const hammlet::Posterior::SampleRegions r = post.sampleRegions(start, end, first, count, seed, 3, K);
        print_numbers("start", start);
        print_numbers("end", end);
        print_numbers("hist", r.hist);
        print_numbers("whole_state", r.wholeState);
        print_numbers("breaks_sum", r.breaksSum);
        print_numbers("breaks_sq", r.breaksSq);
        std::vector<uint32_t> starts(s.blocks + 1);
        check(hml_get_blocks(ctx, starts.data()));
        std::vector<uint64_t> length;
        std::vector<int32_t> state;
        hammlet::Posterior::sampleRuns(s, starts, 0, length, state);
        print_numbers("run_len", length);
        print_numbers("run_state", state);
        const hammlet::Posterior::SampleInfo i = post.sampleInfo();
        printf("info %llu %llu %llu\n", (unsigned long long)i.draws, (unsigned long long)i.groups, (unsigned long long)i.groupSize);
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        if (ctx) hml_destroy(ctx);
        return 1;
    }
    hml_destroy(ctx);
    return 0;
}
