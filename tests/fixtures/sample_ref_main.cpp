// TEST INFRASTRUCTURE: path sampling under fixed parameters restated for one host thread (hammlet_amd/csrc/hml_sample_ref.h) as
// a stand-alone program, for tests/test_sample_cpu.py and tests/test_gpu_sample.py - built once plainly and once with the
// address and undefined-behaviour sanitizers.  Floats travel as their 32 bits, doubles as their 64 bits, in hexadecimal.
// argv[1], if given: a file that receives the paths, count * B bytes, draw-major
// stdin:  "sample" K D P self_trans B first count seed n_regions H, then starts[B + 1] (decimal), sum[D][B], sum_sq[D][B],
//         mean_var[2 P], A[K K], pi[K], then start[n_regions] and end[n_regions] (decimal)
//     or  "timing" and the same: only "segments", "score_fixed", "sample_degenerate" and "seconds" are printed
//     or  "pick" K u w[K] (words of doubles): the categorical rule alone; stdout "state <i>"
// stdout: "segments ..." [count], "score_fixed ..." [count], "change_count ..." [B], "state_count ..." [B][K], "hist ..."
//         [n][H + 1], "whole_state ..." [n][K], "breaks_sum ..." [n], "breaks_sq ..." [n] (all decimal), "sample_degenerate <n>",
//         "viterbi_score <s>", "alpha ..." [B][K] (words) and "seconds <tables, forward rows and decode> <draws and counts>"
// anything else: "error <message>", exit status 2
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hammlet_amd/csrc/hml_sample_ref.h"

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

template <class T>
static void print_counts(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (T x : v) printf(" %lld", (long long)x);
    printf("\n");
}

static int pick_mode() {
    int K = 0;
    double u = 0.0;
    if (scanf("%d", &K) != 1 || K < 1 || K > HML_POST_CAP_K || !read_double(&u)) { printf("error bad header\n"); return 2; }
    std::vector<double> w((size_t)K);
    double S = 0.0;
    for (int i = 0; i < K; ++i) {
        if (!read_double(&w[(size_t)i])) { printf("error short input\n"); return 2; }
        S = S + w[(size_t)i];
    }
    if (hml_sample_bad(S)) { printf("error bad sum\n"); return 2; }
    printf("state %d\n", hml_sample_pick(K, w.data(), S, u));
    return 0;
}

int main(int argc, char** argv) {
    char mode[16];
    if (scanf("%15s", mode) != 1) { printf("error no mode\n"); return 2; }
    if (strcmp(mode, "pick") == 0) return pick_mode();
    const bool quiet = strcmp(mode, "timing") == 0;
    if (!quiet && strcmp(mode, "sample") != 0) { printf("error unknown mode\n"); return 2; }
    hml_post_ref_case c;
    long long B = 0, n_regions = 0;
    unsigned long long first = 0, count = 0, seed = 0;
    unsigned int H = 0;
    if (scanf("%d %d %d %d %lld %llu %llu %llu %lld %u", &c.K, &c.D, &c.P, &c.self_trans, &B, &first, &count, &seed, &n_regions, &H) != 10) {
        printf("error bad header\n");
        return 2;
    }
    if (c.K < 1 || c.K > HML_POST_CAP_K || c.D < 1 || c.D > HML_POST_MAX_D || c.P < 1 || c.P > c.K || B < 1 || B > (1ll << 28) || n_regions < 0 ||
        n_regions > (1ll << 24) || count < 1 || count > (1ull << 24) || first + count > (1ull << 48) || (n_regions > 0 && H < 1) || H > (1u << 20)) {
        printf("error bad sizes\n");
        return 2;
    }
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
        if (!(rs[(size_t)i] < re[(size_t)i] && re[(size_t)i] <= c.starts[c.B])) { printf("error bad region\n"); return 2; }

    const auto t0 = std::chrono::steady_clock::now();
    const int K = c.K;
    hml_post_ref_result p;
    hml_post_ref_tables(c, p.e, p.m);
    p.alpha.assign((size_t)c.B * K, 0.0);
    for (uint64_t b = 0; b < c.B; ++b) {
        double cb = 0.0;
        (void)hml_post_ref_forward_step(K, c.A.data(), c.pi.data(), p.e.data() + b * K, b ? p.alpha.data() + (b - 1) * K : nullptr, p.alpha.data() + b * K, &cb);
    }
    hml_vit_ref_case v;
    v.K = c.K; v.D = c.D; v.P = c.P; v.self_trans = c.self_trans; v.B = c.B;
    v.starts = c.starts; v.sum = c.sum; v.sum_sq = c.sum_sq; v.mean_var = c.mean_var; v.A = c.A; v.pi = c.pi;
    std::vector<int64_t> emit, trans, init;
    hml_vit_ref_tables(v, emit, trans, init);
    std::vector<int16_t> vq;
    int64_t vscore = 0;
    hml_vit_ref_decode(K, c.B, emit, trans, init, vq, &vscore);
    const auto tm = std::chrono::steady_clock::now();
    hml_sample_ref_result r;
    hml_sample_ref_draw(K, c.B, c.A.data(), p.alpha.data(), emit, trans, init, first, count, seed, r);
    std::vector<uint32_t> hist, whole_state;
    std::vector<uint64_t> breaks_sum, breaks_sq;
    hml_sample_ref_regions(K, c.B, c.starts, r.paths, count, (uint64_t)n_regions, rs.data(), re.data(), H, hist, whole_state, breaks_sum, breaks_sq);
    const auto t1 = std::chrono::steady_clock::now();

    if (argc > 1) {
        FILE* f = fopen(argv[1], "wb");
        if (!f || fwrite(r.paths.data(), 1, r.paths.size(), f) != r.paths.size() || fclose(f) != 0) { printf("error cannot write the paths\n"); return 2; }
    }
    print_counts("segments", r.segments);
    print_counts("score_fixed", r.score_fixed);
    printf("sample_degenerate %llu\n", (unsigned long long)r.sample_degenerate);
    if (!quiet) {
        print_counts("change_count", r.change_count);
        print_counts("state_count", r.state_count);
        print_counts("hist", hist);
        print_counts("whole_state", whole_state);
        print_counts("breaks_sum", breaks_sum);
        print_counts("breaks_sq", breaks_sq);
        printf("viterbi_score %lld\n", (long long)vscore);
        printf("alpha");
        for (double x : p.alpha) { uint64_t u; memcpy(&u, &x, sizeof u); printf(" %llx", (unsigned long long)u); }
        printf("\n");
    }
    printf("seconds %.6f %.6f\n", std::chrono::duration<double>(tm - t0).count(), std::chrono::duration<double>(t1 - tm).count());
    return 0;
}
