// note_epoch_math.hpp — the order in which an epoch of the note trainer visits its samples (include/pvq.h states the rule in full):
// a counter-based permutation of [0, n), a function of (seed, epoch, n) alone, evaluated per element.  Host (pvq_note_epoch_order)
// and device (note_epoch.hip) include this one statement of it.
//
// A four-round Feistel network over b bits (b even, 2^b >= n, 2^b <= 4 n for n >= 2) is a bijection of [0, 2^b) whatever its round
// function is; walking its cycle from j < n until it returns below n (cycle walking) makes it a bijection of [0, n).  No sort, no
// state, no element depends on another.
#pragma once

#include <cstdint>

#include "note_trainer_plan.hpp"

namespace pvq {

constexpr uint64_t NE_MAX_N = uint64_t(1) << 32;   // an order's elements are uint32
constexpr uint64_t NE_DOMAIN = 0x45504F4348ull;    // keeps an epoch's keys apart from the dropout keys of the same seed and counter

// what every element of one epoch's order shares: made once on the host, passed to the kernel by value
struct NoteEpochKeys {
    uint64_t key[4] = {0, 0, 0, 0};
    uint64_t n = 0;
    uint32_t h = 0;      // bits of a half: b / 2
    uint32_t mask = 0;   // 2^h - 1
};

// b = max(2, bit_length(n - 1)) rounded up to an even number; 1 <= n <= NE_MAX_N gives 2 <= b <= 32
inline uint32_t ne_bits(uint64_t n) {
    uint32_t b = 0;
    for (uint64_t v = n - 1; v; v >>= 1) ++b;
    if (b < 2) b = 2;
    return (b + 1u) & ~1u;
}

inline NoteEpochKeys ne_keys(uint64_t seed, uint64_t epoch, uint64_t n) {
    NoteEpochKeys k;
    k.n = n;
    k.h = ne_bits(n) / 2;
    k.mask = (1u << k.h) - 1u;
    const uint64_t base = nt_mix(nt_mix(seed + 0x9E3779B97F4A7C15ull * (epoch + 1)) ^ NE_DOMAIN);
    for (uint32_t r = 0; r < 4; ++r) k.key[r] = nt_mix(base ^ r);
    return k;
}

// one pass of the network over x < 2^b
PVQ_NT_HD inline uint64_t ne_pass(const NoteEpochKeys& k, uint64_t x) {
    uint32_t l = static_cast<uint32_t>(x >> k.h), r = static_cast<uint32_t>(x) & k.mask;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = l ^ (static_cast<uint32_t>(nt_mix(k.key[i] ^ r)) & k.mask);
        l = r;
        r = t;
    }
    return (static_cast<uint64_t>(l) << k.h) | r;
}

// order(j), j < n.  The walk ends: j lies on a cycle of the network's permutation, and that cycle comes back to j < n at the latest.
PVQ_NT_HD inline uint64_t ne_order(const NoteEpochKeys& k, uint64_t j) {
    if (k.n == 1) return 0;
    uint64_t x = j;
    do x = ne_pass(k, x);
    while (x >= k.n);
    return x;
}

}  // namespace pvq
