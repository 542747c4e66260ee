// TEST INFRASTRUCTURE: the Viterbi restatement for one host thread (hammlet_amd/csrc/hml_viterbi_ref.h) as a stand-alone
// program, for tests/test_viterbi_cpu.py and tests/test_gpu_viterbi.py - built once plainly and once with the address and
// undefined-behaviour sanitizers.  Floats travel as their 32 bits in hexadecimal, so not-a-number and infinities pass.
// stdin:  "fx" n, then n floats                                   -> stdout: "fx" and the n quantised values
//         "case" K D P self_trans B want_emit, then starts[B + 1] (decimal), sum[D][B], sum_sq[D][B], mean_var[2 P], A[K K], pi[K]
//                                                                 -> stdout: lines "init ...", "trans ...", "emit ..." (if asked),
//                                                                    "path ...", "score <int64>", "seconds <tables> <decode>"
// anything else: "error <message>", exit status 2
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hammlet_amd/csrc/hml_viterbi_ref.h"

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

static void print_words(const char* name, const std::vector<int64_t>& w) {
    printf("%s", name);
    for (int64_t x : w) printf(" %lld", (long long)x);
    printf("\n");
}

int main() {
    char mode[16];
    if (scanf("%15s", mode) != 1) { printf("error no mode\n"); return 2; }
    if (strcmp(mode, "fx") == 0) {
        long long n = 0;
        std::vector<float> x;
        if (scanf("%lld", &n) != 1 || n < 0 || n > (1 << 24) || !read_floats(x, (size_t)n)) { printf("error short input\n"); return 2; }
        std::vector<int64_t> out;
        for (float v : x) out.push_back(hml_vit_ref_fx((double)v));
        print_words("fx", out);
        return 0;
    }
    if (strcmp(mode, "case") != 0) { printf("error unknown mode\n"); return 2; }
    hml_vit_ref_case c;
    long long B = 0;
    int want_emit = 0;
    if (scanf("%d %d %d %d %lld %d", &c.K, &c.D, &c.P, &c.self_trans, &B, &want_emit) != 6) { printf("error bad header\n"); return 2; }
    if (c.K < 1 || c.K > HML_VIT_CAP_K || c.D < 1 || c.D > HML_VIT_MAX_D || c.P < 1 || c.P > c.K || B < 1 || B > (1ll << 28)) { printf("error bad sizes\n"); return 2; }
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
    std::vector<int64_t> emit, trans, init;
    const auto t0 = std::chrono::steady_clock::now();
    hml_vit_ref_tables(c, emit, trans, init);
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int16_t> q;
    int64_t score = 0;
    hml_vit_ref_decode(c.K, c.B, emit, trans, init, q, &score);
    const auto t2 = std::chrono::steady_clock::now();
    print_words("init", init);
    print_words("trans", trans);
    if (want_emit) print_words("emit", emit);
    printf("path");
    for (int16_t s : q) printf(" %d", (int)s);
    printf("\nscore %lld\n", (long long)score);
    printf("seconds %.6f %.6f\n", std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count());
    return 0;
}
