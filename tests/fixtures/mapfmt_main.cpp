// Stand-alone check of the packed maps of the backward pass (hammlet_amd/csrc/hml_maps.h) with a host compiler: the byte
// format of up to 8 states against the 4-bit format and against maps kept as plain arrays, the 4-bit format of 9 to 16
// states against hml_map_compose.  Prints one line per number of states ("K <k> <format> pairs <n> triples <m> ok") and
// returns the number of failed checks (tests/test_mapfmt_cpu.py builds it plain and with sanitizers and runs it).
#include <stdint.h>
#include <stdio.h>

#include "hml_maps.h"

static int failures = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (failures < 20) fprintf(stderr, "%s:%d: K = %d: %s\n", __FILE__, __LINE__, K, #cond); \
            ++failures;                                                                              \
        }                                                                                            \
    } while (0)

struct rng_t {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
};

struct amap { unsigned v[16]; };   // a map as a plain array

template <int K>
static amap a_compose(const amap& f, const amap& g) {
    amap r = {};
    for (int x = 0; x < K; ++x) r.v[x] = f.v[g.v[x]];
    return r;
}
template <int K>
static amap a_random(rng_t& rng) {
    amap r = {};
    for (int x = 0; x < K; ++x) r.v[x] = (unsigned)(rng.next() % (uint64_t)K);
    return r;
}
template <int K>
static amap a_nth(unsigned n) {   // the n-th of the K^K maps
    amap r = {};
    for (int x = 0; x < K; ++x) { r.v[x] = n % (unsigned)K; n /= (unsigned)K; }
    return r;
}
// packed from an array by the format's own empty() and put()
template <class F, int K>
static unsigned long long pack(const amap& a) {
    unsigned long long m = F::empty();
    for (int x = 0; x < K; ++x) m = F::put(m, x, a.v[x]);
    return m;
}
template <class F, int K>
static bool same(unsigned long long m, const amap& a) {
    for (int x = 0; x < K; ++x)
        if (F::get(m, (unsigned)x) != a.v[x]) return false;
    return true;
}
static bool bytes_below_8(unsigned long long m) { return (m & 0xf8f8f8f8f8f8f8f8ull) == 0ull; }

template <int K>
static void check_bytes() {
    using FB = hml_mapfmt<K>;
    using FN = hml_mapfmt_nibbles<K>;
    static_assert(FB::BITS == 8, "up to 8 states: a byte per entry");
    CHECK(FB::identity() == 0x0706050403020100ull);
    CHECK(bytes_below_8(FB::identity()) && bytes_below_8(FB::empty()));
    for (int x = 0; x < 8; ++x) CHECK(FB::get(FB::identity(), (unsigned)x) == (unsigned)x);
    for (int x = K; x < 8; ++x) CHECK(FB::get(FB::empty(), (unsigned)x) == (unsigned)x);   // unused entries: the identity's
    for (unsigned s = 0; s < (unsigned)K; ++s) {
        const unsigned long long b = FB::broadcast(s);
        CHECK(bytes_below_8(b));
        for (int x = 0; x < K; ++x) CHECK(FB::get(b, (unsigned)x) == s && FN::get(FN::broadcast(s), (unsigned)x) == s);
        for (int x = K; x < 8; ++x) CHECK(FB::get(b, (unsigned)x) == (unsigned)x);
        for (int x = 0; x < K; ++x) {
            const unsigned long long m = FB::set(FB::identity(), x, s);
            CHECK(bytes_below_8(m));
            for (int y = 0; y < 8; ++y) CHECK(FB::get(m, (unsigned)y) == (y == x ? s : (unsigned)y));
        }
    }
    long pairs = 0, triples = 0;
    auto pair = [&](const amap& f, const amap& g) {
        const amap r = a_compose<K>(f, g);
        const unsigned long long fb = pack<FB, K>(f), gb = pack<FB, K>(g), rb = FB::compose(fb, gb);
        CHECK(bytes_below_8(fb) && bytes_below_8(gb) && bytes_below_8(rb));
        CHECK((same<FB, K>(rb, r)));
        for (int x = K; x < 8; ++x) CHECK(FB::get(rb, (unsigned)x) == (unsigned)x);
        CHECK((same<FN, K>(FN::compose(pack<FN, K>(f), pack<FN, K>(g)), r)));
        CHECK(FB::compose(fb, FB::identity()) == fb && FB::compose(FB::identity(), fb) == fb);
        ++pairs;
    };
    if (K <= 3) {
        unsigned all = 1;
        for (int i = 0; i < K; ++i) all *= (unsigned)K;
        for (unsigned i = 0; i < all; ++i)
            for (unsigned j = 0; j < all; ++j) pair(a_nth<K>(i), a_nth<K>(j));
    } else {
        rng_t rng = {0x1234u + (uint64_t)K};
        for (int i = 0; i < 100000; ++i) {
            const amap f = a_random<K>(rng), g = a_random<K>(rng);
            pair(f, g);
        }
    }
    rng_t rng = {0x777u + (uint64_t)K};
    for (int i = 0; i < 20000; ++i) {
        const unsigned long long f = pack<FB, K>(a_random<K>(rng)), g = pack<FB, K>(a_random<K>(rng)), h = pack<FB, K>(a_random<K>(rng));
        const unsigned long long l = FB::compose(FB::compose(f, g), h), r = FB::compose(f, FB::compose(g, h));
        CHECK(l == r && bytes_below_8(l));
        ++triples;
    }
    printf("K %d bytes pairs %ld triples %ld %s\n", K, pairs, triples, failures ? "FAILED" : "ok");
}

template <int K>
static void check_nibbles() {
    using F = hml_mapfmt<K>;
    static_assert(F::BITS == 4, "beyond 8 states: 4 bits per entry");
    CHECK(F::identity() == HML_MAP_IDENTITY);
    for (int x = 0; x < 16; ++x) CHECK(F::get(F::identity(), (unsigned)x) == (unsigned)x);
    for (unsigned s = 0; s < (unsigned)K; ++s)
        for (int x = 0; x < K; ++x) CHECK(F::get(F::broadcast(s), (unsigned)x) == s && F::get(F::set(F::identity(), x, s), (unsigned)x) == s);
    long pairs = 0, triples = 0;
    rng_t rng = {0x4321u + (uint64_t)K};
    for (int i = 0; i < 100000; ++i) {
        const amap f = a_random<K>(rng), g = a_random<K>(rng);
        const unsigned long long fp = pack<F, K>(f), gp = pack<F, K>(g);
        CHECK(F::compose(fp, gp) == hml_map_compose<K>(fp, gp));
        CHECK((same<F, K>(F::compose(fp, gp), a_compose<K>(f, g))));
        ++pairs;
    }
    for (int i = 0; i < 20000; ++i) {
        const unsigned long long f = pack<F, K>(a_random<K>(rng)), g = pack<F, K>(a_random<K>(rng)), h = pack<F, K>(a_random<K>(rng));
        CHECK(F::compose(F::compose(f, g), h) == F::compose(f, F::compose(g, h)));
        ++triples;
    }
    printf("K %d nibbles pairs %ld triples %ld %s\n", K, pairs, triples, failures ? "FAILED" : "ok");
}

int main() {
    check_bytes<1>(); check_bytes<2>(); check_bytes<3>(); check_bytes<4>();
    check_bytes<5>(); check_bytes<6>(); check_bytes<7>(); check_bytes<8>();
    check_nibbles<9>(); check_nibbles<10>(); check_nibbles<11>(); check_nibbles<12>();
    check_nibbles<13>(); check_nibbles<14>(); check_nibbles<15>(); check_nibbles<16>();
    return failures ? 1 : 0;
}
