// lattice_index.h — the lattice member's index of a key, idx = (key - kmin) / stride, as an EXACT division whose quotient
// fits 32 bits (k_part_scatter MODE 3 / 4, kernels_part.hip).  Plain C++ for host and device: the host builds the parameter
// block, the producers of the scatter evaluate it once per record, tests/lattice_index_check.cpp compares both with a
// 128-bit division.
//
// Let d = key - kmin (mod 2^64) and stride = 2^z x s' with s' odd, inv = s'^-1 (mod 2^32), q = low32(low32(d >> z) x inv).
// d is a lattice point of the range (stride | d and d / stride < card, card <= 2^32 - 1) if and only if
//     q < card  and  (uint64) q x stride == d,
// and then q is the index:
//   if:      d = i x stride with i < card gives d >> z = i x s' exactly, and i x s' x inv = i (mod 2^32);
//   only if: (card - 1) x stride <= max - min < 2^64, so for q < card the product q x stride does not wrap and equality
//            with d means d IS q x stride; a key below kmin wraps to a d no q < card reproduces.  (For q >= card the
//            product may wrap — the answer is "no" either way.)
// One 32-bit multiply, one 32 x 32 -> 64 multiply and two compares; a second 32-bit multiply only where the stride has a
// high word (a wave-uniform branch).  No reciprocal, no correction step, no special case for stride 1 (z = 0, inv = 1).
#pragma once

#include <stdint.h>

#include "dev_common.h"

namespace mq {

struct LatticeDiv {
  uint64_t stride;  // >= 1
  uint32_t shift;   // z = ctz(stride)
  uint32_t inv;     // (stride >> z)^-1 mod 2^32
  uint32_t card;    // lattice points of the range, <= 2^32 - 1
};

// false: the lattice has more points than a 32-bit index counts (the caller does not run the member)
inline bool lattice_div_make(uint64_t stride, uint64_t card, LatticeDiv* out) {
  if (stride == 0 || card > 0xffffffffull) return false;
  uint32_t z = 0;
  while (!((stride >> z) & 1)) ++z;
  const uint32_t s = (uint32_t)(stride >> z);  // the odd part (mod 2^32)
  uint32_t x = s;                              // s x s = 1 (mod 8): 3 bits right, every Newton step doubles them
  for (int i = 0; i < 4; ++i) x *= 2u - s * x;
  out->stride = stride;
  out->shift = z;
  out->inv = x;
  out->card = (uint32_t)card;
  return true;
}

// d = key - kmin.  true: d is a lattice point of the range; *idx is its index (set either way, meaningful when true)
MQ_D bool lattice_index(const LatticeDiv& g, uint64_t d, uint32_t* idx) {
  const uint32_t q = (uint32_t)(d >> g.shift) * g.inv;
  uint64_t back = (uint64_t)q * (uint32_t)g.stride;
  const uint32_t s_hi = (uint32_t)(g.stride >> 32);
  if (s_hi) back += (uint64_t)(q * s_hi) << 32;  // (mod 2^64: exact wherever q < card)
  *idx = q;
  return q < g.card && back == d;
}

}  // namespace mq
