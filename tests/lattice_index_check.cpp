// The exact-division lattice index (heavydb_amd/csrc/lattice_index.h) against a 128-bit division: for every (stride, card)
// pair and every d, acceptance ("d is a lattice point of the range") and the index must be what d % stride == 0 and
// d / stride < card say.  Exits non-zero at the first mismatch.  Built and run by tests/test_lattice_index_exact.py with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>

#include "lattice_index.h"

typedef unsigned __int128 u128;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static long n_checked = 0;
static bool check(const mq::LatticeDiv& g, uint64_t stride, uint64_t card, uint64_t d) {
  const bool want_ok = d % stride == 0 && d / stride < card;
  uint32_t idx = 0;
  const bool ok = mq::lattice_index(g, d, &idx);
  ++n_checked;
  if (ok != want_ok || (ok && (uint64_t)idx != d / stride)) {
    std::fprintf(stderr, "MISMATCH stride %llu card %llu d %llu: accepted %d (want %d), index %u (want %llu)\n",
                 (unsigned long long)stride, (unsigned long long)card, (unsigned long long)d, (int)ok, (int)want_ok, idx,
                 (unsigned long long)(d / stride));
    return false;
  }
  return true;
}

int main() {
  const uint64_t strides[] = {1, 2, 3, 12, 4096, 999983, 1000003, 6000018, 3ull << 20, 0xffffffffull, 1ull << 32,
                              (1ull << 32) + 1, (1ull << 33) + 9, 1ull << 40, 3ull << 45, 10000019};
  const uint64_t cards[] = {1, 2, 60001, 100000, 1ull << 24, (1ull << 31) + 5, 0xffffffffull};
  int n_pairs = 0;
  for (uint64_t stride : strides) {
    for (uint64_t card : cards) {
      if ((u128)(card - 1) * stride >= ((u128)1 << 64)) continue;  // no such range of 64-bit keys
      mq::LatticeDiv g{};
      if (!mq::lattice_div_make(stride, card, &g)) {
        std::fprintf(stderr, "lattice_div_make refused stride %llu card %llu\n", (unsigned long long)stride, (unsigned long long)card);
        return 2;
      }
      ++n_pairs;
      uint32_t z = 0;
      while (!((stride >> z) & 1)) ++z;
      const uint64_t odd = stride >> z;
      // (all of these wrap mod 2^64 where they exceed it: a wrapped d is a d like any other)
      const uint64_t edges[] = {0, stride, (card - 1) * stride, card * stride, 0 - stride, ~0ull, stride + 1, stride - 1};
      for (uint64_t d : edges)
        if (!check(g, stride, card, d)) return 1;
      for (int k = 0; k < 3200; ++k) {
        const uint64_t i = rnd() % card;
        const uint64_t at = i * stride;
        const uint64_t ds[] = {at, at + rnd() % stride, (i + (1ull << 32)) * stride, at + stride / 2, at + odd, at + (1ull << z), rnd()};
        for (uint64_t d : ds)
          if (!check(g, stride, card, d)) return 1;
      }
    }
  }
  // more points than a 32-bit index counts: refused
  mq::LatticeDiv g{};
  if (mq::lattice_div_make(1, 1ull << 32, &g) || mq::lattice_div_make(3, ~0ull, &g) || mq::lattice_div_make(0, 1, &g)) {
    std::fprintf(stderr, "lattice_div_make accepted a lattice beyond 2^32 - 1 points (or stride 0)\n");
    return 3;
  }
  std::printf("lattice_index: %d (stride, card) pairs, %ld values, 0 mismatches\n", n_pairs, n_checked);
  return 0;
}
