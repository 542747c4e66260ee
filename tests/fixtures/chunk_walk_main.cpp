// The repair walk of the chunked recursions (hammlet_amd/csrc/hml_k_chunks.h) on the host: hml_chunk_same and
// hml_chunk_rerun_walk, exactly as the device kernels instantiate them, around a toy recursion over B blocks on K = 2 words.
//
//   chunk_walk ll|dbl  <  cases        a case per line: seed B L W reset_percent rounds
//
// The toy recursion: block b has an input u[b] in 0 .. 15 and a kind.  R resets the vector from the input alone (block 0 always
// does: the recursion's start is exact); Z zeroes word 0 by a product, so that for doubles the SIGN of the zero depends on
// the predecessor, and keeps word 1; C swaps the words; U updates them from the predecessor, modulo 5 and 3.  All values are
// small integers, exact in both word types.
// The chunk runner follows hml_vit_run_chunk's contract: from == nullptr starts W blocks early from the zero vector (exact
// where that reaches block 0), otherwise from `from`, which becomes the entry; it stores entry, exit and the rows of its blocks.
// Per case: first run of all chunks; verify (match bytes and the list of heads, as hml_chunk_verify defines them); a round -
// the walk from every head - three times on copies of the state, the heads in list order, reversed and shuffled; verify; ...;
// a plain serial finish.  Checked here (a failure prints a line "FAIL ..." and the program exits with 1):
//   (a) after every round the three states are byte-identical: no lane writes what another reads;
//   (b) while chunks are stale every round strictly lowers their number;
//   (c) after the finish the rows are the sequential recursion's, byte for byte;
//   (d) every walk stopped where the rule says it stops (its last steps are traced again on the state it left).
// (a), (b) and (c) are the independent checks.  (d) restates the walk's stopping rule and would share a misreading of it: it
// is there to COUNT the ways on, so that the test can tell that the cases took each of them, and is no oracle for the rule.
// Printed per case, for the test to assert that the cases are not vacuous: the stale chunks after the first run and after
// every round, the longest run of stale chunks, how often each of the walk's ways on was taken, and for doubles the chunks
// whose entry was equal to the predecessor's exit as VALUES (-0.0 against 0.0) and not as words.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hml_k_chunks.h"

static const int K = 2;

struct rng64 {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

static long long toy_mod(long long v, long long m) { return v % m; }
static double toy_mod(double v, double m) { return std::fmod(v, m); }

enum kind : uint8_t { R, Z, C, U };
struct block { uint8_t kind, u; };

template <typename T>
static void toy_step(const block& b, T (&v)[K]) {
    const T u = (T)b.u, v0 = v[0], v1 = v[1];
    switch (b.kind) {
        case R: v[0] = (T)(b.u % 5); v[1] = (T)(b.u % 3); break;
        case Z: v[0] = (v0 - (T)2) * (T)0; break;
        case C: v[0] = v1; v[1] = v0; break;
        default: v[0] = toy_mod(v0 + u, (T)5); v[1] = toy_mod(v1 + v0 + (T)1, (T)3); break;
    }
}

template <typename T>
struct state {
    std::vector<T> entry, exitv, rows;
    bool operator==(const state& o) const {
        return !memcmp(entry.data(), o.entry.data(), entry.size() * sizeof(T)) && !memcmp(exitv.data(), o.exitv.data(), exitv.size() * sizeof(T)) &&
               !memcmp(rows.data(), o.rows.data(), rows.size() * sizeof(T));
    }
};

template <typename T>
struct toy {
    std::vector<block> blocks;
    uint32_t B, L, W, n_chunks;

    void run_chunk(state<T>& s, uint32_t x, const T* from) const {
        const uint32_t lo = x * L, hi = std::min(lo + L, B);
        const uint32_t first = from ? lo : (lo > W ? lo - W : 0u);
        T d[K];
        for (int j = 0; j < K; ++j) d[j] = from ? from[j] : (T)0;
        if (first == lo) memcpy(&s.entry[(size_t)x * K], d, sizeof d);
        for (uint32_t b = first; b < hi; ++b) {
            toy_step(blocks[b], d);
            if (b >= lo) memcpy(&s.rows[(size_t)b * K], d, sizeof d);
            if (b + 1u == lo) memcpy(&s.entry[(size_t)x * K], d, sizeof d);
        }
        memcpy(&s.exitv[(size_t)x * K], d, sizeof d);
    }
    // hml_chunk_verify, serially: the number of stale chunks
    uint32_t verify(const state<T>& s, std::vector<uint8_t>& match, std::vector<uint32_t>& heads) const {
        uint32_t stale = 0;
        heads.clear();
        for (uint32_t x = 0; x < n_chunks; ++x) {
            const bool eq = x == 0u || hml_chunk_same(&s.entry[(size_t)x * K], &s.exitv[(size_t)(x - 1u) * K], K);
            match[x] = eq ? 1 : 0;
            if (!eq) {
                ++stale;
                if (x == 1u || hml_chunk_same(&s.entry[(size_t)(x - 1u) * K], &s.exitv[(size_t)(x - 2u) * K], K)) heads.push_back(x);
            }
        }
        return stale;
    }
};

struct tally { unsigned long long still = 0, stored = 0, other = 0, again = 0, end = 0; };

static bool fail(const char* what, uint64_t seed, long a = -1, long b = -1) {
    printf("FAIL seed=%llu %s %ld %ld\n", (unsigned long long)seed, what, a, b);
    return false;
}

// a round: the walk from every head in this order.  With `t`, every walk's ways on are counted, its stop traced again
template <typename T>
static bool round_of(const toy<T>& g, state<T>& s, const std::vector<uint8_t>& match, const std::vector<uint32_t>& heads, tally* t, uint64_t seed) {
    for (const uint32_t head : heads) {
        std::vector<uint32_t> ran;
        auto run = [&](uint32_t x, const T* from) { ran.push_back(x); g.run_chunk(s, x, from); };
        hml_chunk_rerun_walk(run, s.entry.data(), s.exitv.data(), K, g.n_chunks, head, match.data());
        if (ran.empty() || ran[0] != head) return fail("the walk did not begin at its head", seed, head);
        for (size_t i = 1; i < ran.size(); ++i) {
            if (ran[i] <= ran[i - 1]) return fail("the walk went back", seed, ran[i]);
            for (uint32_t y = ran[i - 1] + 1u; y < ran[i]; ++y)
                if (match[y]) return fail("a matching chunk was stepped over", seed, y);
            if (t) { t->stored += ran[i] - ran[i - 1] - 1u; ++t->again; }
        }
        // nothing was written behind the last run: its steps from there, once more
        for (uint32_t x = ran.back();;) {
            const uint32_t nx = x + 1u;
            if (nx >= g.n_chunks) { if (t) ++t->end; break; }
            const bool listed = match[nx] == 0;
            if (hml_chunk_same(&s.entry[(size_t)nx * K], &s.exitv[(size_t)x * K], K)) {
                if (!listed) { if (t) ++t->still; break; }
                if (t) ++t->stored;
                x = nx;
                continue;
            }
            if (!(!listed && nx + 1u < g.n_chunks && match[nx + 1u] == 0)) return fail("the walk stopped in front of a chunk it had to run", seed, nx);
            if (t) ++t->other;
            break;
        }
    }
    return true;
}

template <typename T>
static bool run_case(uint64_t seed, uint32_t B, uint32_t L, uint32_t W, uint32_t reset_percent, uint32_t rounds) {
    toy<T> g;
    g.B = B; g.L = L; g.W = W; g.n_chunks = (B + L - 1u) / L;
    rng64 rng{seed};
    g.blocks.resize(B);
    for (uint32_t b = 0; b < B; ++b) {
        const uint32_t r = rng.below(100u);
        g.blocks[b].u = (uint8_t)rng.below(16u);
        g.blocks[b].kind = b == 0u || r < reset_percent ? R : r < reset_percent + 12u ? Z : r < reset_percent + 30u ? C : U;
    }
    // the sequential recursion
    std::vector<T> seq((size_t)B * K);
    {
        T d[K] = {(T)0, (T)0};
        for (uint32_t b = 0; b < B; ++b) { toy_step(g.blocks[b], d); memcpy(&seq[(size_t)b * K], d, sizeof d); }
    }
    state<T> s;
    s.entry.assign((size_t)g.n_chunks * K, (T)0); s.exitv.assign((size_t)g.n_chunks * K, (T)0); s.rows.assign((size_t)B * K, (T)0);
    for (uint32_t x = 0; x < g.n_chunks; ++x) g.run_chunk(s, x, nullptr);

    std::vector<uint8_t> match(g.n_chunks);
    std::vector<uint32_t> heads;
    uint32_t stale = g.verify(s, match, heads);
    uint32_t longest = 0, zero_traps = 0;
    for (uint32_t x = 1, len = 0; x < g.n_chunks; ++x) {
        len = match[x] ? 0u : len + 1u;
        longest = std::max(longest, len);
        bool values = true;
        for (int j = 0; j < K; ++j) values = values && s.entry[(size_t)x * K + j] == s.exitv[(size_t)(x - 1u) * K + j];
        if (values && !match[x]) ++zero_traps;
    }
    printf("seed=%llu chunks=%u stale=%u", (unsigned long long)seed, g.n_chunks, stale);
    tally t;
    for (uint32_t round = 0; round < rounds && stale != 0u; ++round) {
        std::vector<uint32_t> rev(heads.rbegin(), heads.rend()), shuf(heads);
        for (size_t i = shuf.size(); i > 1; --i) std::swap(shuf[i - 1], shuf[rng.below((uint32_t)i)]);
        state<T> s_rev = s, s_shuf = s;
        if (!round_of(g, s, match, heads, &t, seed) || !round_of(g, s_rev, match, rev, nullptr, seed) || !round_of(g, s_shuf, match, shuf, nullptr, seed)) return false;
        if (!(s == s_rev) || !(s == s_shuf)) return fail("(a) the order of the heads shows after round", seed, round);
        const uint32_t before = stale;
        stale = g.verify(s, match, heads);
        if (stale >= before) return fail("(b) a round did not lower the number of stale chunks", seed, before, stale);
        printf(",%u", stale);
    }
    // a plain serial finish
    for (uint32_t x = 1; x < g.n_chunks; ++x)
        if (!hml_chunk_same(&s.entry[(size_t)x * K], &s.exitv[(size_t)(x - 1u) * K], K)) g.run_chunk(s, x, &s.exitv[(size_t)(x - 1u) * K]);
    if (g.verify(s, match, heads) != 0u) return fail("stale chunks after the finish", seed);
    if (memcmp(s.rows.data(), seq.data(), seq.size() * sizeof(T))) return fail("(c) the rows are not the sequential recursion's", seed);
    printf(" longest=%u still=%llu stored=%llu other=%llu again=%llu end=%llu zero_traps=%u\n", longest, t.still, t.stored, t.other, t.again, t.end, zero_traps);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2 || (strcmp(argv[1], "ll") && strcmp(argv[1], "dbl"))) { fprintf(stderr, "usage: chunk_walk ll|dbl < cases\n"); return 2; }
    const bool dbl = !strcmp(argv[1], "dbl");
    unsigned long long seed;
    unsigned B, L, W, percent, rounds;
    while (scanf("%llu %u %u %u %u %u", &seed, &B, &L, &W, &percent, &rounds) == 6) {
        if (B < 1u || L < 1u || percent > 70u) { fprintf(stderr, "bad case\n"); return 2; }
        if (!(dbl ? run_case<double>(seed, B, L, W, percent, rounds) : run_case<long long>(seed, B, L, W, percent, rounds))) return 1;
    }
    return 0;
}
