// Maps [K] -> [K] packed into one 64-bit word: what the backward pass composes (hml_k_backward.h).  No HIP in here: a host
// compiler alone builds it and a test walks the formats over all numbers of states (tests/test_mapfmt_cpu.py).
//
// Two formats, chosen by the number of states (hml_mapfmt<K>):
//   up to 8 states  one BYTE per entry, identity 0x0706050403020100.  (f o g)[x] = f[g[x]] is then a byte permute: on the
//                   device two v_perm_b32, one per half of g, with f's eight bytes as the table.
//   9 to 16 states  4 bits per entry, identity HML_MAP_IDENTITY, composed entry by entry (hml_map_compose).
//
// INVARIANT of the byte format: EVERY byte of every map, the unused entries x >= K included, is in 0 .. 7.  The permute's
// selector values from 8 up do not index the table (they replicate sign bits or give constants), so a byte that is 0xff or
// left over from somewhere else would put garbage into the entries that are read.  Maps therefore start from identity() or
// empty() (unused entries = the identity's), broadcast() and set() take a state below K <= 8, and compose() of two maps
// that hold the invariant holds it: each of its bytes is a byte of f.
#ifndef HML_MAPS_H
#define HML_MAPS_H

#include "hml_common.h"

#define HML_MAP_IDENTITY 0xfedcba9876543210ull
#define HML_MAP_IDENTITY_BYTES 0x0706050403020100ull

// (f o g)(x) = f(g(x)) on maps [K]->[K] packed 4 bits per entry
template <int K>
HML_HD unsigned long long hml_map_compose(unsigned long long f, unsigned long long g) {
    unsigned long long r = 0ull;   // entries x >= K are never read
#pragma unroll
    for (int x = 0; x < K; ++x) {
        const unsigned y = (unsigned)(g >> (4 * x)) & 15u;
        const unsigned long long z = (f >> (4 * y)) & 15ull;
        r |= z << (4 * x);
    }
    return r;
}

// 4 bits per entry: entries x >= K of a map are never read and may hold anything
template <int K>
struct hml_mapfmt_nibbles {
    static constexpr int BITS = 4;
    static constexpr unsigned MASK = 15u;
    HML_HDM static unsigned long long identity() { return HML_MAP_IDENTITY; }
    HML_HDM static unsigned long long empty() { return 0ull; }   // to be filled with put()
    HML_HDM static unsigned long long compose(unsigned long long f, unsigned long long g) { return hml_map_compose<K>(f, g); }
    HML_HDM static unsigned get(unsigned long long m, unsigned x) { return (unsigned)(m >> (4u * x)) & 15u; }
    HML_HDM static unsigned long long put(unsigned long long m, int x, unsigned state) { return m | ((unsigned long long)state << (4 * x)); }
    HML_HDM static unsigned long long set(unsigned long long m, int x, unsigned state) {
        return (m & ~(15ull << (4 * x))) | ((unsigned long long)state << (4 * x));
    }
    HML_HDM static unsigned long long broadcast(unsigned state) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int x = 0; x < K; ++x) m |= (unsigned long long)state << (4 * x);
        return m;
    }
};

// a byte per entry (K <= 8); see the invariant at the top
template <int K>
struct hml_mapfmt_bytes {
    static_assert(K >= 1 && K <= 8, "eight bytes in a word");
    static constexpr int BITS = 8;
    static constexpr unsigned MASK = 255u;
    static constexpr unsigned long long USED = K == 8 ? ~0ull : ((1ull << (8 * (K & 7))) - 1ull);   // the bytes of entries x < K
    HML_HDM static unsigned long long identity() { return HML_MAP_IDENTITY_BYTES; }
    HML_HDM static unsigned long long empty() { return HML_MAP_IDENTITY_BYTES & ~USED; }   // entries x < K zero, to be filled with put()
    HML_HDM static unsigned long long compose(unsigned long long f, unsigned long long g) {
#if defined(__HIP_DEVICE_COMPILE__)
        // v_perm_b32: selector bytes 0 .. 3 pick from the second operand, 4 .. 7 from the first
        const unsigned flo = (unsigned)f, fhi = (unsigned)(f >> 32);
        const unsigned lo = __builtin_amdgcn_perm(fhi, flo, (unsigned)g), hi = __builtin_amdgcn_perm(fhi, flo, (unsigned)(g >> 32));
        return ((unsigned long long)hi << 32) | lo;
#else
        unsigned long long r = 0ull;
        for (int x = 0; x < 8; ++x) {
            const unsigned y = (unsigned)(g >> (8 * x)) & 7u;
            r |= ((f >> (8 * y)) & 255ull) << (8 * x);
        }
        return r;
#endif
    }
    HML_HDM static unsigned get(unsigned long long m, unsigned x) { return (unsigned)(m >> (8u * x)) & 255u; }
    HML_HDM static unsigned long long put(unsigned long long m, int x, unsigned state) { return m | ((unsigned long long)state << (8 * x)); }
    HML_HDM static unsigned long long set(unsigned long long m, int x, unsigned state) {
        return (m & ~(255ull << (8 * x))) | ((unsigned long long)(state & 7u) << (8 * x));
    }
    HML_HDM static unsigned long long broadcast(unsigned state) {
        return (((unsigned long long)(state & 7u) * 0x0101010101010101ull) & USED) | (HML_MAP_IDENTITY_BYTES & ~USED);
    }
};

template <int K, bool BYTES = (K <= 8)>
struct hml_mapfmt : hml_mapfmt_bytes<K> {};
template <int K>
struct hml_mapfmt<K, false> : hml_mapfmt_nibbles<K> {};

// entry x of a map whose entries are `bits` wide (hml_mapfmt<K>::BITS), for code that is not compiled per number of states
HML_HD unsigned hml_map_get_bits(unsigned long long m, unsigned x, unsigned bits) { return (unsigned)(m >> (bits * x)) & ((1u << bits) - 1u); }

#endif
