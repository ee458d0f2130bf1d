// kernels_filter.hip — the consumers of the two-register programs (regprog.h) that STREAM columns:
//   k_filter_mask, k_filter_mask_i32   the ROW MASK of a filter compiled at plan time whose atoms include programs (round 6)
//   k_scan_agg_prog                    non-grouped aggregates whose ARGUMENTS are programs: SUM(a * b) WHERE c < k in one pass
// (the Projection family evaluates its typed expression targets itself, kernels_proj.hip).  Both run the programs on the
// four rows of a quad together, on values already in registers, with no stack, no scratch and no node decode per row.
// And the other producer of such a row mask, which runs no program: k_join_exists_mask_fast, the join level of a SEMI / ANTI
// step (one plain key column probed in a perfect join table; behind the filter mask's launcher).
//
// ---- the row mask
// The reference compiles a WHERE clause into the row function (Executor::compileBody, NativeCodegen.cpp:3455; arithmetic
// leaves: codegenArith / codegenDiv, ArithmeticIR.cpp:39-560; the short-circuit forms behind prioritizeQuals,
// LogicalIR.cpp:158-297).  Here a filter of comparisons with literals is evaluated INSIDE the consuming kernel (atoms +
// truth table, boolfilter.h).  A filter with PROGRAM atoms — `b <> 0 AND a / b > 3`, `x + y > 100`, `a < b`, DOUBLE
// leaves: two-register programs of typed steps, regprog.h — is evaluated by this pre-pass instead: it streams the
// filter's columns ONCE (16-byte loads, two quads per lane in flight), runs atoms, programs and the truth table on the four
// rows of a quad together and leaves ONE BYTE per row (1 = the row passes).  The step proper then runs without the
// filter's columns and with the qual `mask = 1` on that 1-byte column — which every typed family loads as one 4-byte word
// per quad.  Bytes: the filter's columns are read once either way; the mask adds 1 B/row written + 1 B/row read (the
// interpreter pass of rounds 3-5 wrote and re-read a 4-byte column per expression and ran ~450 wave instructions per 64
// rows).  An error a row raises (error 7 / error 1) ends the step exactly as the row function's would: every row evaluates
// the filter's expressions, whatever the plain quals say of it.
#include <algorithm>
#include <cstring>

#include "boolfilter.h"
#include "fast_common.h"
#include "kernels.h"
#include "regprog.h"

namespace mq {

using namespace fast;

namespace {

constexpr int kFmBlock = 256;

struct FilterMaskArgs {
  int32_t n_flt, n_frags, n_cols_table, pad_;
  int32_t col[kBfMaxCols], width[kBfMaxCols];  // the filter's columns: index in the column table, bytes per value (4 / 8)
  const BoolFilter* bf;                         // DEVICE memory
  const int8_t* const* cols;
  const int64_t* num_rows;
  int8_t* const* mask;                          // per fragment: ceil(n / 4) * 4 bytes, 16-byte aligned
  int32_t* d_err;
};

template <int NF>
MQ_D void fm_load_quad(const FilterMaskArgs& a, const int8_t* const* fc, int64_t quad, v4i32 (&lo)[NF], v4i32 (&hi)[NF]) {
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    if (k >= a.n_flt) break;
    const int8_t* base = fc[a.col[k]];
    if (a.width[k] == 8) {
      lo[k] = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)base + quad * 2);
      hi[k] = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)base + quad * 2 + 1);
    } else {
      lo[k] = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)base + quad);
    }
  }
}
MQ_D int32_t fm_v4(const v4i32& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
template <int NF>
MQ_D void fm_values(const FilterMaskArgs& a, const v4i32 (&lo)[NF], const v4i32 (&hi)[NF], int64_t (&vals)[4][NF]) {
#pragma unroll
  for (int k = 0; k < NF; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (k >= a.n_flt) {
        vals[i][k] = 0;
      } else if (a.width[k] == 8) {
        const v4i32& h = i < 2 ? lo[k] : hi[k];
        const int j = (i & 1) * 2;
        vals[i][k] = (int64_t)(((uint64_t)(uint32_t)fm_v4(h, j + 1) << 32) | (uint64_t)(uint32_t)fm_v4(h, j));
      } else {
        vals[i][k] = (int64_t)fm_v4(lo[k], i);
      }
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#define FM_UNIFORM(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define FM_UNIFORM(x) ((int)(x))
#endif
// what bf_quad_pass (boolfilter.h) reads of the filter per quad, read ONCE per workgroup into scalar registers: every one
// of those reads is an LDS round trip the next one waits for, and a quad's evaluation is a chain of them (the first
// version of this kernel ran 5.3 - 8.0 ms per 1 B rows with 3 waves per SIMD: latency, not bandwidth or arithmetic)
struct FmMeta {
  int n_progs;
  uint32_t atoms_of;   // range atoms of filter column c: byte c
  uint64_t prog_meta;  // program k: 16 bits — operand columns (4 bits each), can_raise (bit 8)
};
template <int NF>
MQ_D uint32_t fm_quad_pass(const BoolFilter& bf, const FmMeta& mt, const int64_t (&vals)[4][NF], uint32_t valid, int32_t* err) {
  uint32_t idx[4] = {0, 0, 0, 0}, mul = 1;
  int ai = 0;
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    const int cnt = (int)((mt.atoms_of >> (8 * c)) & 255u);
    for (int k = 0; k < cnt; ++k) {
      const BoolAtom at = bf.atom[ai];
#pragma unroll
      for (int j = 0; j < 4; ++j) idx[j] += bf_atom_state(at, vals[j][c]) * mul;
      mul *= 3u;
      ++ai;
    }
  }
  uint32_t epack[4] = {0, 0, 0, 0};  // two bits per program atom: the error it raised (ex_err_enc)
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int k = 0; k < mt.n_progs; ++k) {
    const uint32_t pm = (uint32_t)(mt.prog_meta >> (16 * k)) & 0xffffu;
    const int ca = (int)(pm & 15u), cb = (int)((pm >> 4) & 15u);
    int64_t ops[4][2], outv[4];
    int32_t e4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ops[j][0] = vals[j][0];
      ops[j][1] = vals[j][0];
#pragma unroll
      for (int c = 1; c < NF; ++c) {
        if (ca == c) ops[j][0] = vals[j][c];
        if (cb == c) ops[j][1] = vals[j][c];
      }
    }
    rp_eval<4, 2>(bf.prog[k], ops, outv, e4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t st = e4[j] ? 3u : outv[j] == 1 ? 1u : outv[j] == 0 ? 0u : 2u;  // (anything else is the INT8 NULL)
      idx[j] += st * mul;
      epack[j] |= ex_err_enc(e4[j]) << (2 * k);
    }
    mul *= ((pm >> 8) & 1u) ? 4u : 3u;
  }
  uint32_t w4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w4[j] = bf.table[idx[j] >> 5];  // (four independent reads: one round trip)
  uint32_t pass = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t bit = (w4[j] >> (idx[j] & 31u)) & 1u;
    if (epack[j] && ((valid >> j) & 1u)) {  // rare: an atom of this row is in its ERROR state — is it the row's outcome?
      const uint32_t nib = (bf.etable[idx[j] >> 3] >> ((idx[j] & 7u) * 4u)) & 15u;
      if (nib) {
        if (!*err) *err = ex_err_dec((epack[j] >> (2u * (nib - 1u))) & 3u);
        bit = 0;
      }
    }
    pass |= bit << j;
  }
  return pass & valid;
}

// NF: filter columns this member holds registers for
template <int NF>
__global__ __launch_bounds__(kFmBlock) void k_filter_mask(FilterMaskArgs a) {
  __shared__ BoolFilter s_bf;
  bf_load(a.bf, &s_bf, threadIdx.x, kFmBlock);
  __syncthreads();
  FmMeta mt;
  mt.n_progs = FM_UNIFORM(s_bf.n_progs);
  mt.atoms_of = 0;
  mt.prog_meta = 0;
#pragma unroll
  for (int c = 0; c < kBfMaxCols; ++c) mt.atoms_of |= (uint32_t)FM_UNIFORM(c < s_bf.n_cols ? s_bf.atoms_of_col[c] : 0) << (8 * c);
#pragma unroll
  for (int k = 0; k < kBfMaxProgs; ++k)
    mt.prog_meta |= (uint64_t)(uint32_t)FM_UNIFORM((s_bf.prog_op[k][0] & 15) | ((s_bf.prog_op[k][1] & 15) << 4) | (s_bf.prog[k].can_raise ? 256 : 0)) << (16 * k);
  int32_t err = 0;
  const int64_t gtid = (int64_t)blockIdx.x * kFmBlock + threadIdx.x;
  const int64_t gsize = (int64_t)gridDim.x * kFmBlock;
  for (int f = 0; f < a.n_frags; ++f) {
    const int8_t* const* fc = a.cols + (size_t)f * a.n_cols_table;
    const int64_t n = a.num_rows[f];
    const int64_t nq = n >> 2;
    uint32_t* const out = (uint32_t*)a.mask[f];
    // ONE copy of the evaluator in the kernel (the programs' typed members are inlined four rows wide: ~5 K instructions).
    // Every lane walks the fragment's quads with the loads of its NEXT quad in flight while this one's programs run; the
    // fragment's last, partial quad takes the same path with its rows loaded one by one (a row past the end repeats the
    // last one and is not valid).
    const int64_t nq_all = (n + 3) >> 2;
    auto load_vals = [&](int64_t quad, v4i32 (&lo)[NF], v4i32 (&hi)[NF]) {
      if (quad < nq) {
        fm_load_quad<NF>(a, fc, quad, lo, hi);
      } else if (quad < nq_all) {  // (one lane per fragment)
        const int left = (int)(n & 3);
#pragma unroll
        for (int k = 0; k < NF; ++k) {
          if (k >= a.n_flt) break;
          int64_t v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int64_t pos = (nq << 2) + (i < left ? i : left - 1);
            v[i] = a.width[k] == 8 ? load_one<int64_t>(fc[a.col[k]], pos) : (int64_t)load_one<int32_t>(fc[a.col[k]], pos);
          }
          if (a.width[k] == 8) {
            lo[k].x = (int)(uint32_t)v[0]; lo[k].y = (int)(uint32_t)((uint64_t)v[0] >> 32); lo[k].z = (int)(uint32_t)v[1]; lo[k].w = (int)(uint32_t)((uint64_t)v[1] >> 32);
            hi[k].x = (int)(uint32_t)v[2]; hi[k].y = (int)(uint32_t)((uint64_t)v[2] >> 32); hi[k].z = (int)(uint32_t)v[3]; hi[k].w = (int)(uint32_t)((uint64_t)v[3] >> 32);
          } else {
            lo[k].x = (int)v[0]; lo[k].y = (int)v[1]; lo[k].z = (int)v[2]; lo[k].w = (int)v[3];
          }
        }
      }
    };
    v4i32 lo_c[NF], hi_c[NF], lo_n[NF], hi_n[NF];
    int64_t q = gtid;
    load_vals(q, lo_c, hi_c);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (; q < nq_all; q += gsize) {
      load_vals(q + gsize, lo_n, hi_n);
      int64_t vals[4][NF];
      fm_values<NF>(a, lo_c, hi_c, vals);
      const uint32_t valid = q < nq ? 15u : (1u << (int)(n & 3)) - 1u;
      const uint32_t m = fm_quad_pass<NF>(s_bf, mt, vals, valid, &err);
      // one byte per row: 1 = the row passes
      const uint32_t w = (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
      __builtin_nontemporal_store(w, (MQ_GLOBAL uint32_t*)out + q);
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        lo_c[k] = lo_n[k];
        hi_c[k] = hi_n[k];
      }
    }
  }
  if (err) atomicCAS(a.d_err, 0, err);
}

// ---- the LEAN member: every filter column a plain INT32, every program a PairAtom (boolfilter.h): `a <cmp> b`,
// `(a <op> b) <cmp> literal` at INT32.  Values stay 32 bits wide, a program is ONE typed operation per row behind a few
// scalar branches (no steps, no register selects per step), the tile loop is uniform (a workgroup walks tiles of kFmBlock
// quads, the next tile's loads in flight while this one's rows are looked at).
constexpr int kFmHoisted = 2;  // pair atoms kept in scalar registers for the whole kernel (the rest are read per quad)
struct FmPairs {
  PairAtom pa[kFmHoisted];
};
template <int NF>
MQ_D uint32_t fm_quad_pass_i32(const BoolFilter& bf, const FmMeta& mt, const FmPairs& hp, const v4i32 (&col)[NF], uint32_t valid, int32_t* err) {
  uint32_t idx[4] = {0, 0, 0, 0}, mul = 1;
  int ai = 0;
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    const int cnt = (int)((mt.atoms_of >> (8 * c)) & 255u);
    for (int k = 0; k < cnt; ++k) {
      const BoolAtom at = bf.atom[ai];
#pragma unroll
      for (int j = 0; j < 4; ++j) idx[j] += bf_atom_state(at, (int64_t)fm_v4(col[c], j)) * mul;
      mul *= 3u;
      ++ai;
    }
  }
  uint32_t epack[4] = {0, 0, 0, 0};
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int k = 0; k < mt.n_progs; ++k) {
    const uint32_t pm = (uint32_t)(mt.prog_meta >> (16 * k)) & 0xffffu;
    const int ca = (int)(pm & 15u), cb = (int)((pm >> 4) & 15u);
    PairAtom pa;
    if (k == 0) {
      pa = hp.pa[0];
    } else if (k == 1) {
      pa = hp.pa[1];
    } else {
      pa = bf.pair[k];
      pa.op = FM_UNIFORM(pa.op);
      pa.ln = FM_UNIFORM(pa.ln);
      pa.rn = FM_UNIFORM(pa.rn);
      pa.b_is_lit = FM_UNIFORM(pa.b_is_lit);
      pa.b_lit = FM_UNIFORM(pa.b_lit);
      pa.lo = FM_UNIFORM(pa.lo);
      pa.hi = FM_UNIFORM(pa.hi);
      pa.negate = FM_UNIFORM(pa.negate);
      pa.op2 = FM_UNIFORM(pa.op2);
      pa.lit2 = FM_UNIFORM(pa.lit2);
    }
    v4i32 av = col[0], bv = col[0];
#pragma unroll
    for (int c = 1; c < NF; ++c) {
      if (ca == c) av = col[c];
      if (cb == c) bv = col[c];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int32_t e = 0;
      const uint32_t st = pair_eval(pa, fm_v4(av, j), fm_v4(bv, j), e);
      idx[j] += st * mul;
      epack[j] |= ex_err_enc(e) << (2 * k);
    }
    mul *= ((pm >> 8) & 1u) ? 4u : 3u;
  }
  uint32_t w4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w4[j] = bf.table[idx[j] >> 5];  // (four independent reads: one round trip)
  uint32_t pass = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t bit = (w4[j] >> (idx[j] & 31u)) & 1u;
    if (epack[j] && ((valid >> j) & 1u)) {  // rare: an atom of this row is in its ERROR state — is it the row's outcome?
      const uint32_t nib = (bf.etable[idx[j] >> 3] >> ((idx[j] & 7u) * 4u)) & 15u;
      if (nib) {
        if (!*err) *err = ex_err_dec((epack[j] >> (2u * (nib - 1u))) & 3u);
        bit = 0;
      }
    }
    pass |= bit << j;
  }
  return pass & valid;
}

template <int NF>
__global__ __launch_bounds__(kFmBlock) void k_filter_mask_i32(FilterMaskArgs a) {
  __shared__ BoolFilter s_bf;
  bf_load(a.bf, &s_bf, threadIdx.x, kFmBlock);
  __syncthreads();
  FmMeta mt;
  mt.n_progs = FM_UNIFORM(s_bf.n_progs);
  mt.atoms_of = 0;
  mt.prog_meta = 0;
#pragma unroll
  for (int c = 0; c < kBfMaxCols; ++c) mt.atoms_of |= (uint32_t)FM_UNIFORM(c < s_bf.n_cols ? s_bf.atoms_of_col[c] : 0) << (8 * c);
#pragma unroll
  for (int k = 0; k < kBfMaxProgs; ++k)
    mt.prog_meta |= (uint64_t)(uint32_t)FM_UNIFORM((s_bf.prog_op[k][0] & 15) | ((s_bf.prog_op[k][1] & 15) << 4) | (s_bf.prog[k].can_raise ? 256 : 0)) << (16 * k);
  FmPairs hp;
#pragma unroll
  for (int k = 0; k < kFmHoisted; ++k) {
    const PairAtom& src = s_bf.pair[k];
    hp.pa[k] = PairAtom{};
    hp.pa[k].op = FM_UNIFORM(src.op);
    hp.pa[k].ln = FM_UNIFORM(src.ln);
    hp.pa[k].rn = FM_UNIFORM(src.rn);
    hp.pa[k].b_is_lit = FM_UNIFORM(src.b_is_lit);
    hp.pa[k].b_lit = FM_UNIFORM(src.b_lit);
    hp.pa[k].lo = FM_UNIFORM(src.lo);
    hp.pa[k].hi = FM_UNIFORM(src.hi);
    hp.pa[k].negate = FM_UNIFORM(src.negate);
    hp.pa[k].op2 = FM_UNIFORM(src.op2);
    hp.pa[k].lit2 = FM_UNIFORM(src.lit2);
  }
  int32_t err = 0;
  const int tid = threadIdx.x;
  for (int f = 0; f < a.n_frags; ++f) {
    const int8_t* const* fc = a.cols + (size_t)f * a.n_cols_table;
    const int64_t n = a.num_rows[f];
    const int64_t nq = n >> 2;
    uint32_t* const out = (uint32_t*)a.mask[f];
    const int8_t* base[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) base[k] = k < a.n_flt ? fc[a.col[k]] : nullptr;
    const int64_t n_tiles = (nq + kFmBlock - 1) / kFmBlock;
    auto load_tile = [&](int64_t t, v4i32 (&col)[NF]) {
      const int64_t q = t * kFmBlock + tid;
      if (q < nq) {
#pragma unroll
        for (int k = 0; k < NF; ++k)
          if (k < a.n_flt) col[k] = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)base[k] + q);
      }
    };
    v4i32 cur[NF], nxt[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) cur[k] = nxt[k] = v4i32{0, 0, 0, 0};
    int64_t t = (blockIdx.x + (int64_t)f * 7) % gridDim.x;
    if (t < n_tiles) load_tile(t, nxt);
    for (; t < n_tiles; t += gridDim.x) {  // (uniform)
#pragma unroll
      for (int k = 0; k < NF; ++k) cur[k] = nxt[k];
      if (t + gridDim.x < n_tiles) load_tile(t + gridDim.x, nxt);
      const int64_t q = t * kFmBlock + tid;
      const uint32_t m = fm_quad_pass_i32<NF>(s_bf, mt, hp, cur, q < nq ? 15u : 0u, &err);
      const uint32_t w = (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
      if (q < nq) __builtin_nontemporal_store(w, (MQ_GLOBAL uint32_t*)out + q);
    }
    // the fragment's last, partial quad: its rows one by one (a row past the end repeats the last one and is not valid)
    if ((n & 3) && blockIdx.x == (unsigned)(f % (int)gridDim.x) && tid == 0) {
      const int left = (int)(n & 3);
      v4i32 col[NF];
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        col[k] = v4i32{0, 0, 0, 0};
        if (k < a.n_flt) {
          const int64_t p0 = nq << 2;
          col[k].x = load_one<int32_t>(base[k], p0);
          col[k].y = load_one<int32_t>(base[k], p0 + (left > 1 ? 1 : 0));
          col[k].z = load_one<int32_t>(base[k], p0 + (left > 2 ? 2 : left - 1));
          col[k].w = col[k].z;
        }
      }
      const uint32_t m = fm_quad_pass_i32<NF>(s_bf, mt, hp, col, (1u << left) - 1u, &err);
      const uint32_t w = (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
      out[nq] = w;
    }
  }
  if (err) atomicCAS(a.d_err, 0, err);
}

// =========================================================================== scan_agg_prog
// Non-grouped aggregates of EXPRESSIONS — SUM(a * b) WHERE c < k (TPC-H Q6's shape) — in one pass: the scan-aggregate
// skeleton (kernels_fast.hip k_scan_agg: a workgroup walks contiguous tiles of each fragment, every lane keeps UQ 16-byte
// non-temporal loads per column in flight, four rows per lane and load, typed register accumulators per argument, a wave
// shuffle reduce, one LDS fold per workgroup, the partial row merged with reduce_target) with the evaluator of the row
// mask above: the arguments are two-register programs in LDS (regprog.h AggProgArgs), run on the four rows of a quad
// together.  The two-pass path (k_project writes an 8-byte column per expression, k_scan_agg reads it back) moves
// 16 B/row/expression more and synchronises in between.
// Errors: the row function evaluates a target's expression only for a row that passed the quals, so an error (7: overflow,
// a narrowing cast) counts only where the quad's pass bit is set — never for a row the quals drop, never for the
// repeated row behind a fragment's end.  Division is not among the members (rp_eval<.., false>): those plans keep k_project.
constexpr int kSapFlt = 4;
struct ScanAggProgArgs {
  int32_t n_cols, n_args, n_progs, n_frags;
  int32_t n_shared, n_own, n_cols_table, n_targets;
  int32_t slot_count, pad_;
  int32_t col[kApMaxCols], col_w8[kApMaxCols];  // operand slots: index in the column table, 8-byte values (else 4)
  int32_t arg_slot[kApMaxArgs], arg_type[kApMaxArgs], arg_nullable[kApMaxArgs];
  int32_t arg_need[kApMaxArgs];                 // 2 = sum, 4 = min, 8 = max (the count of values is always kept)
  // range quals on an operand column test the values already loaded (sh_slot); the others load their own column
  RangeFilter sh_flt[kSapFlt], own_flt[kSapFlt];
  int32_t sh_slot[kSapFlt], own_type[kSapFlt];  // own_type: MI355Q_INT32 / _INT64 / _INT8 (one word per quad)
  int32_t target_arg[MI355Q_MAX_TARGETS];       // -1 = COUNT(*)
  DevTarget targets[MI355Q_MAX_TARGETS];
  int64_t init_vals[MI355Q_MAX_SLOTS];
  RegProg prog[kApMaxArgs];
  const int8_t* const* cols;
  const int64_t* num_rows;
  int64_t* out;
  int32_t* d_err;
};
static_assert(sizeof(ScanAggProgArgs) <= 3584, "k_scan_agg_prog takes its arguments by value: the kernel argument segment holds 4 KB");

struct SapQuad {
  v4i32 lo, hi;  // four rows of a column as loaded: lo alone (4-byte values; lo.x alone: 1-byte values), lo + hi (8-byte)
};
struct SapAcc {
  unsigned long long cnt;  // rows that passed with a value that is not NULL
  int64_t sum, mn, mx;     // by the argument's type: integers, or the bits of a double
};
MQ_D int64_t sap_i64(const SapQuad& r, int i) {
  const v4i32& h = i < 2 ? r.lo : r.hi;
  const int j = (i & 1) * 2;
  return (int64_t)(((uint64_t)(uint32_t)fm_v4(h, j + 1) << 32) | (uint64_t)(uint32_t)fm_v4(h, j));
}
// four rows loaded one by one (a fragment's last, partial quad) in the registers a 16-byte load would have filled
MQ_D void sap_pack(const int64_t (&v)[4], int width, SapQuad& r) {
  if (width == 8) {
    r.lo.x = (int)(uint32_t)v[0]; r.lo.y = (int)(uint32_t)((uint64_t)v[0] >> 32); r.lo.z = (int)(uint32_t)v[1]; r.lo.w = (int)(uint32_t)((uint64_t)v[1] >> 32);
    r.hi.x = (int)(uint32_t)v[2]; r.hi.y = (int)(uint32_t)((uint64_t)v[2] >> 32); r.hi.z = (int)(uint32_t)v[3]; r.hi.w = (int)(uint32_t)((uint64_t)v[3] >> 32);
  } else if (width == 4) {
    r.lo.x = (int)v[0]; r.lo.y = (int)v[1]; r.lo.z = (int)v[2]; r.lo.w = (int)v[3];
  } else {
    r.lo.x = (int)(((uint32_t)v[0] & 255u) | (((uint32_t)v[1] & 255u) << 8) | (((uint32_t)v[2] & 255u) << 16) | (((uint32_t)v[3] & 255u) << 24));
  }
}
MQ_D double sap_wave_sum_f64(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
template <bool FP, bool MAX>
MQ_D int64_t sap_wave_best(int64_t v) {  // MIN / MAX of integers or of doubles held as their bits
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t o = (int64_t)__shfl_down((long long)v, off, 64);
    bool take;
    if (FP) take = MAX ? bits_dbl(v) < bits_dbl(o) : bits_dbl(o) < bits_dbl(v);
    else take = MAX ? v < o : o < v;
    v = take ? o : v;
  }
  return v;
}

// NC / NF: operand columns / filter-only columns this member holds registers for; UQ: quads per column and lane in flight;
// PF: the next tile's loads are issued before this tile's values are looked at (twice the raw registers).
// Two workgroups per CU (the grid the scan-aggregate family streams best with): 256 VGPRs per lane, which both members
// fill — values and programs are 64 bits wide, four rows at a time — without scratch.
template <int NC, int NF, int UQ, bool PF>
__global__ __launch_bounds__(kBlock, 2) void k_scan_agg_prog(ScanAggProgArgs a) {
  __shared__ RegProg s_prog[kApMaxArgs];
  {
    const int32_t* src = (const int32_t*)a.prog;
    int32_t* dst = (int32_t*)s_prog;
    for (int i = threadIdx.x; i < (int)(sizeof(RegProg) / 4) * a.n_progs; i += kBlock) dst[i] = src[i];
  }
  __syncthreads();
  SapAcc acc[kApMaxArgs];
#pragma unroll
  for (int c = 0; c < kApMaxArgs; ++c) {
    const bool fp = a.arg_type[c] == MI355Q_DOUBLE;
    acc[c].cnt = 0;
    acc[c].sum = 0;  // (the bits of 0.0 as well)
    acc[c].mn = fp ? dbl_bits(1.7976931348623157e308) : INT64_MAX;
    acc[c].mx = fp ? dbl_bits(-1.7976931348623157e308) : INT64_MIN;
  }
  unsigned long long rows_passing = 0;
  int32_t err = 0;
  const int tid = threadIdx.x;
  constexpr int64_t tile_q = (int64_t)kBlock * UQ;

  // one quad of every column: the range quals on the values as loaded (a 4-bit pass mask), the programs on its four rows,
  // the accumulators.  ONE copy in the kernel: the programs' typed members are inlined four rows wide.
  auto quad_rows = [&](const SapQuad (&cq)[NC], const SapQuad (&fq)[NF], uint32_t valid) {
    int64_t vals[4][NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int i = 0; i < 4; ++i) vals[i][k] = k >= a.n_cols ? 0 : a.col_w8[k] ? sap_i64(cq[k], i) : (int64_t)fm_v4(cq[k].lo, i);
    }
    uint32_t pass = valid;
#pragma unroll
    for (int k = 0; k < kSapFlt; ++k) {
      if (k >= a.n_shared) break;
      const int slot = a.sh_slot[k];
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int64_t x = vals[i][0];
#pragma unroll
        for (int c = 1; c < NC; ++c)
          if (slot == c) x = vals[i][c];
        m |= (filter_pass<int64_t>(a.sh_flt[k], x) ? 1u : 0u) << i;
      }
      pass &= m;
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      if (k >= a.n_own) break;
      const int t = a.own_type[k];
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool p = t == MI355Q_INT32  ? filter_pass<int32_t>(a.own_flt[k], fm_v4(fq[k].lo, i))
                       : t == MI355Q_INT8 ? filter_pass<int32_t>(a.own_flt[k], (int32_t)(int8_t)((uint32_t)fq[k].lo.x >> (8 * i)))
                                          : filter_pass<int64_t>(a.own_flt[k], sap_i64(fq[k], i));
        m |= (p ? 1u : 0u) << i;
      }
      pass &= m;
    }
    rows_passing += __popc(pass);
    int64_t av[kApMaxArgs][4];
#pragma unroll
    for (int c = 0; c < kApMaxArgs; ++c) {
      // a plain-column argument: the operand as loaded (wave-uniform selects, never a run-time index into registers)
      const int slot = c >= a.n_progs && c < a.n_args ? a.arg_slot[c] : 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int64_t x = vals[i][0];
#pragma unroll
        for (int k = 1; k < NC; ++k)
          if (slot == k) x = vals[i][k];
        av[c][i] = x;
      }
    }
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int k = 0; k < a.n_progs; ++k) {
      int64_t outv[4];
      int32_t e4[4];
      rp_eval<4, NC, false>(s_prog[k], vals, outv, e4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (e4[i] && ((pass >> i) & 1u) && !err) err = e4[i];
#pragma unroll
      for (int c = 0; c < kApMaxArgs; ++c) {
        if (k != c) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) av[c][i] = outv[i];
      }
    }
#pragma unroll
    for (int c = 0; c < kApMaxArgs; ++c) {
      if (c >= a.n_args) break;
      const int t = a.arg_type[c], need = a.arg_need[c];
      const bool nul = a.arg_nullable[c] != 0;
      SapAcc& r = acc[c];
      if (t == MI355Q_DOUBLE) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double v = bits_dbl(av[c][i]);
          const bool ok = ((pass >> i) & 1u) && !(nul && v == kNullDouble);
          r.cnt += ok ? 1u : 0u;
          if (need & 2) r.sum = ok ? dbl_bits(bits_dbl(r.sum) + v) : r.sum;
          if (need & 4) r.mn = (ok && v < bits_dbl(r.mn)) ? av[c][i] : r.mn;
          if (need & 8) r.mx = (ok && bits_dbl(r.mx) < v) ? av[c][i] : r.mx;
        }
      } else {
        const int64_t null_val = t == MI355Q_INT32 ? (int64_t)INT32_MIN : INT64_MIN;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t x = av[c][i];
          const bool ok = ((pass >> i) & 1u) && !(nul && x == null_val);
          r.cnt += ok ? 1u : 0u;
          if (need & 2) r.sum = (int64_t)((uint64_t)r.sum + (uint64_t)(ok ? x : 0));  // (wraps in 64 bits)
          if (need & 4) r.mn = (ok && x < r.mn) ? x : r.mn;
          if (need & 8) r.mx = (ok && r.mx < x) ? x : r.mx;
        }
      }
    }
  };

  for (int f = 0; f < a.n_frags; ++f) {
    const int8_t* const* fc = a.cols + (size_t)f * a.n_cols_table;
    const int64_t n = a.num_rows[f];
    const int64_t nq = n >> 2;
    // the fragment's quads, its last partial one included: that one's rows are loaded one by one by the lane it falls to (a
    // row past the end repeats the last one and is not valid), so the tile loop below is the only path through the fragment
    const int64_t nq_all = (n + 3) >> 2;
    const int64_t n_tiles = (nq_all + tile_q - 1) / tile_q;
    const int8_t *cbase[NC], *fbase[NF];
#pragma unroll
    for (int k = 0; k < NC; ++k) cbase[k] = k < a.n_cols ? fc[a.col[k]] : nullptr;
#pragma unroll
    for (int k = 0; k < NF; ++k) fbase[k] = k < a.n_own ? fc[a.own_flt[k].col] : nullptr;
    // every load of a step is issued before the first value is looked at
    auto load_tile = [&](int64_t t, SapQuad (&cq)[UQ][NC], SapQuad (&fq)[UQ][NF]) {
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
        const int64_t q = t * tile_q + (int64_t)u * kBlock + tid;
        if (q < nq) {
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            if (k >= a.n_cols) break;
            if (a.col_w8[k]) {
              cq[u][k].lo = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)cbase[k] + q * 2);
              cq[u][k].hi = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)cbase[k] + q * 2 + 1);
            } else {
              cq[u][k].lo = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)cbase[k] + q);
            }
          }
#pragma unroll
          for (int k = 0; k < NF; ++k) {
            if (k >= a.n_own) break;
            if (a.own_type[k] == MI355Q_INT8) {
              fq[u][k].lo.x = (int)__builtin_nontemporal_load((const MQ_GLOBAL uint32_t*)fbase[k] + q);
            } else if (a.own_type[k] == MI355Q_INT32) {
              fq[u][k].lo = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)fbase[k] + q);
            } else {
              fq[u][k].lo = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)fbase[k] + q * 2);
              fq[u][k].hi = __builtin_nontemporal_load((const MQ_GLOBAL v4i32*)fbase[k] + q * 2 + 1);
            }
          }
        } else if (q < nq_all) {  // (one lane per fragment)
          const int left = (int)(n & 3);
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            if (k >= a.n_cols) break;
            int64_t v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int64_t pos = (nq << 2) + (i < left ? i : left - 1);
              v[i] = a.col_w8[k] ? load_one<int64_t>(cbase[k], pos) : (int64_t)load_one<int32_t>(cbase[k], pos);
            }
            sap_pack(v, a.col_w8[k] ? 8 : 4, cq[u][k]);
          }
#pragma unroll
          for (int k = 0; k < NF; ++k) {
            if (k >= a.n_own) break;
            const int t8 = a.own_type[k];
            int64_t v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int64_t pos = (nq << 2) + (i < left ? i : left - 1);
              v[i] = t8 == MI355Q_INT8    ? (int64_t)load_one<int8_t>(fbase[k], pos)
                     : t8 == MI355Q_INT32 ? (int64_t)load_one<int32_t>(fbase[k], pos)
                                          : load_one<int64_t>(fbase[k], pos);
            }
            sap_pack(v, t8 == MI355Q_INT8 ? 1 : t8 == MI355Q_INT32 ? 4 : 8, fq[u][k]);
          }
        }
      }
    };
    auto tile_rows = [&](int64_t t, const SapQuad (&cq)[UQ][NC], const SapQuad (&fq)[UQ][NF]) {
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
        const int64_t q = t * tile_q + (int64_t)u * kBlock + tid;
        const uint32_t valid = q < nq ? 15u : q < nq_all ? (1u << (int)(n & 3)) - 1u : 0u;
        quad_rows(cq[u], fq[u], valid);
      }
    };
    SapQuad cur_c[UQ][NC], cur_f[UQ][NF];
#pragma unroll
    for (int u = 0; u < UQ; ++u) {
#pragma unroll
      for (int k = 0; k < NC; ++k) cur_c[u][k].lo = cur_c[u][k].hi = v4i32{0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < NF; ++k) cur_f[u][k].lo = cur_f[u][k].hi = v4i32{0, 0, 0, 0};
    }
    // (the starting workgroup rotates per fragment so that short fragments still spread over the grid)
    int64_t t = (blockIdx.x + (int64_t)f * 7) % gridDim.x;
    if constexpr (PF) {
      SapQuad nxt_c[UQ][NC], nxt_f[UQ][NF];
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
#pragma unroll
        for (int k = 0; k < NC; ++k) nxt_c[u][k] = cur_c[u][k];
#pragma unroll
        for (int k = 0; k < NF; ++k) nxt_f[u][k] = cur_f[u][k];
      }
      if (t < n_tiles) load_tile(t, nxt_c, nxt_f);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
      for (; t < n_tiles; t += gridDim.x) {  // (uniform)
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
#pragma unroll
          for (int k = 0; k < NC; ++k) cur_c[u][k] = nxt_c[u][k];
#pragma unroll
          for (int k = 0; k < NF; ++k) cur_f[u][k] = nxt_f[u][k];
        }
        if (t + gridDim.x < n_tiles) load_tile(t + gridDim.x, nxt_c, nxt_f);
        tile_rows(t, cur_c, cur_f);
      }
    } else {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
      for (; t < n_tiles; t += gridDim.x) {
        load_tile(t, cur_c, cur_f);
        tile_rows(t, cur_c, cur_f);
      }
    }
  }
  if (err) atomicCAS(a.d_err, 0, err);

  // wave reduce, then one fold per workgroup in LDS (the epilogue of k_scan_agg)
  __shared__ unsigned long long s_rows[kBlock / 64];
  __shared__ SapAcc s_acc[kBlock / 64][kApMaxArgs];
  rows_passing = wave_sum_u64(rows_passing);
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int c = 0; c < kApMaxArgs; ++c) {
    if (c >= a.n_args) break;
    SapAcc r;
    r.cnt = wave_sum_u64(acc[c].cnt);
    if (a.arg_type[c] == MI355Q_DOUBLE) {
      r.sum = dbl_bits(sap_wave_sum_f64(bits_dbl(acc[c].sum)));
      r.mn = sap_wave_best<true, false>(acc[c].mn);
      r.mx = sap_wave_best<true, true>(acc[c].mx);
    } else {
      r.sum = (int64_t)wave_sum_i64((long long)acc[c].sum);
      r.mn = sap_wave_best<false, false>(acc[c].mn);
      r.mx = sap_wave_best<false, true>(acc[c].mx);
    }
    if (lane == 0) s_acc[wave][c] = r;
  }
  if (lane == 0) s_rows[wave] = rows_passing;
  __syncthreads();
  if (tid != 0) return;
  unsigned long long rows = 0;
  for (int w = 0; w < kBlock / 64; ++w) rows += s_rows[w];
  if (!rows) return;  // nothing passed in this workgroup: the slots keep what they have
  // the workgroup's partial row, as the row function would have left it in a private buffer
  int64_t part[MI355Q_MAX_SLOTS];
  for (int j = 0; j < a.slot_count; ++j) part[j] = a.init_vals[j];
  for (int i = 0; i < a.n_targets; ++i) {
    const DevTarget& tg = a.targets[i];
    const int cs = a.target_arg[i];
    if (cs < 0) {
      part[tg.slot] = (int64_t)rows;
      continue;
    }
    const bool fp = a.arg_type[cs] == MI355Q_DOUBLE;
    SapAcc r = s_acc[0][cs];
    for (int w = 1; w < kBlock / 64; ++w) {
      const SapAcc& o = s_acc[w][cs];
      r.cnt += o.cnt;
      if (fp) {
        r.sum = dbl_bits(bits_dbl(r.sum) + bits_dbl(o.sum));
        r.mn = bits_dbl(o.mn) < bits_dbl(r.mn) ? o.mn : r.mn;
        r.mx = bits_dbl(r.mx) < bits_dbl(o.mx) ? o.mx : r.mx;
      } else {
        r.sum = (int64_t)((uint64_t)r.sum + (uint64_t)o.sum);
        r.mn = o.mn < r.mn ? o.mn : r.mn;
        r.mx = r.mx < o.mx ? o.mx : r.mx;
      }
    }
    switch (tg.agg) {
      case MI355Q_COUNT: part[tg.slot] = (int64_t)r.cnt; break;
      case MI355Q_AVG:
        part[tg.slot + 1] = (int64_t)r.cnt;
        [[fallthrough]];
      case MI355Q_SUM:
        if (r.cnt) part[tg.slot] = r.sum;
        break;
      case MI355Q_MIN:
        if (r.cnt) part[tg.slot] = r.mn;
        break;
      default:
        if (r.cnt) part[tg.slot] = r.mx;
    }
  }
  for (int i = 0; i < a.n_targets; ++i) reduce_target<true>(a.targets[i], a.init_vals, a.out, part);
}

// the kernel's arguments from the lowered plan's quals and targets + the arguments' description; false: not this family
bool sap_args(const DevPlan& p, const AggProgArgs& ap, const FragView& fv, ScanAggProgArgs* out) {
  ScanAggProgArgs& a = *out;
  std::memset(&a, 0, sizeof(a));
  if (p.desc_type != MI355Q_NON_GROUPED_AGGREGATE || p.join_col >= 0 || p.bf_active || p.slot_width != 8 || p.n_quals > MI355Q_MAX_QUALS ||
      ap.n_args < 1 || ap.n_args > kApMaxArgs || ap.n_cols < 1 || ap.n_cols > kApMaxCols || p.n_targets > MI355Q_MAX_TARGETS)
    return false;
  a.n_cols = ap.n_cols;
  a.n_args = ap.n_args;
  a.n_progs = ap.n_progs;
  a.n_frags = fv.n_frags;
  a.n_cols_table = fv.n_cols;
  a.n_targets = p.n_targets;
  a.slot_count = p.slot_count;
  for (int k = 0; k < ap.n_cols; ++k) {
    if (!rp_type_ok(ap.col_type[k]) || ap.col[k] < 0 || ap.col[k] >= fv.n_cols || !all_aligned16(fv, ap.col[k])) return false;
    a.col[k] = ap.col[k];
    a.col_w8[k] = ap.col_type[k] == MI355Q_INT32 ? 0 : 1;
  }
  for (int c = 0; c < ap.n_args; ++c) {
    a.arg_slot[c] = c < ap.n_progs ? 0 : ap.arg_slot[c];
    a.arg_type[c] = ap.arg_type[c];
    a.arg_nullable[c] = ap.arg_nullable[c];
    a.prog[c] = ap.prog[c];
  }
  for (int i = 0; i < p.n_targets; ++i) {
    a.targets[i] = p.targets[i];
    a.target_arg[i] = ap.target_arg[i];
    if (ap.target_arg[i] < 0) continue;
    const int agg = p.targets[i].agg;
    a.arg_need[ap.target_arg[i]] |= (agg == MI355Q_SUM || agg == MI355Q_AVG) ? 2 : agg == MI355Q_MIN ? 4 : agg == MI355Q_MAX ? 8 : 0;
  }
  for (int j = 0; j < MI355Q_MAX_SLOTS; ++j) a.init_vals[j] = p.init_vals[j];
  // the range quals, merged per column as k_scan_agg merges them
  RangeFilter flt[MI355Q_MAX_QUALS];
  int32_t flt_type[MI355Q_MAX_QUALS];
  for (int i = 0; i < p.n_quals; ++i) {
    if (p.quals[i].col < 0 || p.quals[i].col >= fv.n_cols || !make_range_filter(p.quals[i], &flt[i], true)) return false;
    flt_type[i] = p.quals[i].type;
    if (!all_aligned16(fv, p.quals[i].col)) return false;
  }
  const int n_flt = merge_range_filters(flt, flt_type, p.n_quals);
  if (n_flt > kSapFlt) return false;
  for (int i = 0; i < n_flt; ++i) {
    int slot = -1;
    for (int k = 0; k < ap.n_cols; ++k)
      if (ap.col[k] == flt[i].col && ap.col_type[k] == flt_type[i]) slot = k;
    if (slot >= 0) {
      a.sh_flt[a.n_shared] = flt[i];
      a.sh_slot[a.n_shared++] = slot;
    } else {
      a.own_flt[a.n_own] = flt[i];
      a.own_type[a.n_own++] = flt_type[i];
    }
  }
  return true;
}

}  // namespace

bool scan_agg_prog_eligible(const DevPlan& p, const AggProgArgs& ap, const FragView& fv) {
  ScanAggProgArgs a;
  return sap_args(p, ap, fv, &a);
}

hipError_t launch_scan_agg_prog(const DevPlan& p, const AggProgArgs& ap, const FragView& fv, int64_t* out, int32_t* d_err, int n_cus,
                                hipStream_t s, LaunchStats* st) {
  ScanAggProgArgs a;
  if (!sap_args(p, ap, fv, &a)) return hipErrorInvalidValue;
  a.cols = fv.d_cols;
  a.num_rows = fv.d_num_rows;
  a.out = out;
  a.d_err = d_err;
  st->kernel_name = "k_scan_agg_prog";
  st->n_launches = 1;
  st->variant = 0;
  // two operand columns and at most one column read for the filter alone (SUM(a * b) WHERE c < k): two quads per column
  // in flight and the next tile's behind them; else one quad of up to four + four columns (no room for the next tile's)
  const bool lean = a.n_cols <= 2 && a.n_own <= 1;
  const int bpc = tune_knobs().blocks_per_cu > 0 ? tune_knobs().blocks_per_cu : 2;
  const int64_t want = (fv.max_frag_rows / 4 + kBlock * (lean ? 2 : 1)) / (kBlock * (lean ? 2 : 1));
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)n_cus * bpc, want));
  rec(st->k_start, s);
  if (lean) hipLaunchKernelGGL((k_scan_agg_prog<2, 1, 2, true>), dim3((unsigned)grid), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((k_scan_agg_prog<kApMaxCols, kSapFlt, 1, false>), dim3((unsigned)grid), dim3(kBlock), 0, s, a);
  rec(st->k_stop, s);
  return hipGetLastError();
}

int64_t filter_mask_chunk_bytes(int64_t n_rows) { return ((((n_rows + 3) >> 2) << 2) + 15) & ~(int64_t)15; }

bool filter_mask_eligible(const BoolFilter& bf, const FragView& fv) {
  if (bf.n_cols < 1 || bf.n_cols > kBfMaxCols) return false;
  for (int k = 0; k < bf.n_cols; ++k) {
    const int t = bf.col_type[k];
    if (t != MI355Q_INT32 && t != MI355Q_INT64 && t != MI355Q_DOUBLE) return false;
    if (!all_aligned16(fv, bf.col[k])) return false;
  }
  return true;
}

// =========================================================================== the join level of a SEMI / ANTI step as a row mask
// k_join_exists_mask_fast (api_routes.cpp execute_exists_join; the general member is kernels_generic.hip k_join_exists_mask):
// ONE plain INT32 / INT64 key column in 16-byte aligned chunks over a PERFECT join table.  The streaming skeleton of
// fast_common.h scan_fragments: a workgroup walks tiles of kBlock x kJxUQ quads, every lane loads its kJxUQ key quads
// (16-byte non-temporal loads) before it looks at the first key, then issues the probes of all its rows — cached loads, the
// table is what should stay in L2 — before it looks at the first answer, and a quad's four result bytes leave as ONE 4-byte
// store (a wave writes 256 contiguous bytes).  The probe of a row: the NULL and range tests, slot = key - min_key, then
//   BITS — a one-to-one table with its presence bitmap: the slot's bit (1/32 of the row-id table: 12.5 MB for 100 M slots, not 400 MB);
//   else the slot's word >= 0: the row id of a one-to-one table without a bitmap, offsets[slot] of a one-to-many table (one test).
// A NULL key and a key outside [min_key, max_key] never touch the table (jx_probe).  ANTI: the inverted byte.  The quads behind a
// fragment's last full tile go one per lane; its last, partial quad goes row by row with BYTE stores: nothing is written
// behind a fragment's last row (the chunk the pass loop carves is padded to a multiple of 16 bytes all the same — the
// consuming families load the mask as one 4-byte word per quad — and those bytes are never looked at).
// No barrier, no LDS, no atomics.
namespace {

constexpr int kJxUQ = 2;

template <bool K64>
MQ_D bool jx_in_range(const JoinExistsArgs& a, int64_t k) {
  constexpr int64_t kNull = K64 ? INT64_MIN : (int64_t)INT32_MIN;
  return k >= a.min_key && k <= a.max_key && !(a.key_nullable && k == kNull);
}
// what the table says of the row's slot, as a word whose top bit is CLEAR when the slot holds a row; -1 for a row that is not `in`
// (NULL key, key outside the range).  The load itself is unconditional — a row that is not `in` reads a word of the row-count
// array instead, never the table — so that a lane's probes are all in flight before the first answer is looked at (behind a
// branch per row the compiler waits for every probe in turn: eight dependent round trips per lane and tile).
template <bool BITS>
MQ_D int32_t jx_probe(const JoinExistsArgs& a, bool in, int64_t off) {
  const int32_t* const idle = (const int32_t*)a.num_rows;
  int32_t w;
  if (BITS) {
    const int32_t* p = in ? (const int32_t*)(a.bitmap + (off >> 5)) : idle;
    w = (int32_t)(~(uint32_t)*(const MQ_GLOBAL int32_t*)p << (31 - (int)(off & 31)));
  } else {
    const int32_t* p = in ? a.table + off : idle;
    w = *(const MQ_GLOBAL int32_t*)p;
  }
  return in ? w : -1;
}

template <bool K64, bool BITS, bool ANTI>
__global__ __launch_bounds__(kBlock) void k_join_exists_mask_fast(JoinExistsArgs a) {
  using KT = typename std::conditional<K64, int64_t, int32_t>::type;
  const int64_t tile_q = (int64_t)kBlock * kJxUQ;
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t gsize = (int64_t)gridDim.x * kBlock;
  for (int f = 0; f < a.n_frags; ++f) {
    const int8_t* kb = a.cols[(size_t)f * a.n_cols_table + a.key_col];
    int8_t* const out = a.mask[f];
    const int64_t n = a.num_rows[f];
    const int64_t nq = n >> 2;
    const int64_t n_tiles = nq / tile_q;
    for (int64_t t = (blockIdx.x + (int64_t)f * 7) % gridDim.x; t < n_tiles; t += gridDim.x) {
      const int64_t q0 = t * tile_q + threadIdx.x;
      Quad<KT> kq[kJxUQ];
#pragma unroll
      for (int u = 0; u < kJxUQ; ++u) load_quad<KT>(kb, q0 + (int64_t)u * kBlock, kq[u]);
      int32_t ans[kJxUQ][4];
#pragma unroll
      for (int u = 0; u < kJxUQ; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t k = (int64_t)kq[u].v[i];
          ans[u][i] = jx_probe<BITS>(a, jx_in_range<K64>(a, k), k - a.min_key);
        }
      }
#pragma unroll
      for (int u = 0; u < kJxUQ; ++u) {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) w |= (uint32_t)((ans[u][i] >= 0) != ANTI) << (8 * i);
        __builtin_nontemporal_store(w, (MQ_GLOBAL uint32_t*)out + q0 + (int64_t)u * kBlock);
      }
    }
    // ragged end of the fragment: whole quads past the last full tile, then < 4 rows (byte stores)
    for (int64_t q = n_tiles * tile_q + gtid; q < nq; q += gsize) {
      Quad<KT> k0;
      load_quad<KT>(kb, q, k0);
      int32_t ans[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t k = (int64_t)k0.v[i];
        ans[i] = jx_probe<BITS>(a, jx_in_range<K64>(a, k), k - a.min_key);
      }
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) w |= (uint32_t)((ans[i] >= 0) != ANTI) << (8 * i);
      __builtin_nontemporal_store(w, (MQ_GLOBAL uint32_t*)out + q);
    }
    const int64_t tail = (nq << 2) + gtid;
    if (tail < n) {
      const int64_t k = (int64_t)load_one<KT>(kb, tail);
      const int32_t ans = jx_probe<BITS>(a, jx_in_range<K64>(a, k), k - a.min_key);
      out[tail] = (int8_t)((ans >= 0) != ANTI);
    }
  }
}

template <bool K64, bool BITS>
void jx_launch(bool anti, int64_t grid, const JoinExistsArgs& a, hipStream_t s) {
  if (anti) hipLaunchKernelGGL((k_join_exists_mask_fast<K64, BITS, true>), dim3((unsigned)grid), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((k_join_exists_mask_fast<K64, BITS, false>), dim3((unsigned)grid), dim3(kBlock), 0, s, a);
}

}  // namespace

bool join_exists_mask_fast_eligible(const DevPlan& p, const FragView& fv) {
  if (tune_knobs().flags & MI355Q_OPT_LDS_GENERIC_MEMBER) return false;  // (the A/B switch of the typed members: the general one)
  if (p.join_n_keys != 1 || (p.join_hash_type != 0 && p.join_hash_type != 2) || !p.join_buf) return false;
  if (p.join_type != MI355Q_INT32 && p.join_type != MI355Q_INT64) return false;  // plain, unencoded
  if (p.join_max < p.join_min || p.join_entries != p.join_max - p.join_min + 1) return false;
  return all_aligned16(fv, p.join_col);
}

hipError_t launch_join_exists_mask(const DevPlan& p, bool anti, const FragView& fv, int8_t* const* d_mask, int n_cus, hipStream_t s) {
  if (fv.n_frags <= 0 || fv.max_frag_rows <= 0) return hipSuccess;
  if (!join_exists_mask_fast_eligible(p, fv)) return launch_join_exists_mask_general(p, anti, fv, d_mask, n_cus, s);
  JoinExistsArgs a{};
  a.cols = fv.d_cols;
  a.num_rows = fv.d_num_rows;
  a.mask = d_mask;
  a.n_frags = fv.n_frags;
  a.n_cols_table = fv.n_cols;
  a.key_col = p.join_col;
  a.key_nullable = p.join_nullable ? 1 : 0;
  a.min_key = p.join_min;
  a.max_key = p.join_max;
  a.table = (const int32_t*)p.join_buf;  // (one-to-many: the offsets lead the buffer)
  a.bitmap = p.join_hash_type == 0 ? p.join_bitmap : nullptr;
  const bool bits = a.bitmap != nullptr;
  // 4 workgroups per CU: a row's probe is a dependent random read behind its key, and more waves hide more of them
  const int bpc = tune_knobs().blocks_per_cu > 0 ? tune_knobs().blocks_per_cu : 4;
  const int64_t want = fv.max_frag_rows / 4 / (kBlock * kJxUQ) + 1;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)n_cus * bpc, want));
  if (p.join_type == MI355Q_INT64) {
    if (bits) jx_launch<true, true>(anti, grid, a, s);
    else jx_launch<true, false>(anti, grid, a, s);
  } else {
    if (bits) jx_launch<false, true>(anti, grid, a, s);
    else jx_launch<false, false>(anti, grid, a, s);
  }
  return hipGetLastError();
}

hipError_t launch_filter_mask(const BoolFilter& bf, const BoolFilter* d_bf, const FragView& fv, int8_t* const* d_mask, int32_t* d_err,
                              int n_cus, hipStream_t s) {
  FilterMaskArgs a{};
  a.n_flt = bf.n_cols;
  a.n_frags = fv.n_frags;
  a.n_cols_table = fv.n_cols;
  for (int k = 0; k < bf.n_cols; ++k) {
    a.col[k] = bf.col[k];
    a.width[k] = bf.col_type[k] == MI355Q_INT32 ? 4 : 8;
  }
  a.bf = d_bf;
  a.cols = fv.d_cols;
  a.num_rows = fv.d_num_rows;
  a.mask = d_mask;
  a.d_err = d_err;
  int64_t want = (fv.max_frag_rows / 4 + kFmBlock - 1) / kFmBlock;
  int64_t grid = (int64_t)n_cus * 8;
  if (grid > want) grid = want;
  if (grid < 1) grid = 1;
  const bool lean = bf.all_lean && bf.all_i32 && !(tune_knobs().flags & MI355Q_OPT_LDS_GENERIC_MEMBER);
  if (lean && bf.n_cols <= 2) hipLaunchKernelGGL(k_filter_mask_i32<2>, dim3((unsigned)grid), dim3(kFmBlock), 0, s, a);
  else if (lean) hipLaunchKernelGGL(k_filter_mask_i32<kBfMaxCols>, dim3((unsigned)grid), dim3(kFmBlock), 0, s, a);
  else if (bf.n_cols <= 2) hipLaunchKernelGGL(k_filter_mask<2>, dim3((unsigned)grid), dim3(kFmBlock), 0, s, a);
  else hipLaunchKernelGGL(k_filter_mask<kBfMaxCols>, dim3((unsigned)grid), dim3(kFmBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace mq

// ---------------------------------------------------------------------------------------------------------------------
// The host simulation WITHOUT the LDS families (tests/hostsim: kernels_lds.hip is not part of that build, its members are
// row-function stand-ins there) still links and takes the route of k_groupby_lds_prog: the member's own description decides
// who is eligible (lds_args.h make_lds_prog_args), and a launch writes the arguments' values into temporary columns — what
// k_project would have left, through this file's evaluator — and runs the lowered plan's row function over them.  An error
// counts only for a row that passes the quals.  The simulation that compiles kernels_lds.hip for the host, and every
// device build, have the kernel itself.
#if defined(HOSTSIM_DEVICE_CODE) && !defined(HOSTSIM_REAL_FAST)
#include <vector>

#include "lds_args.h"

namespace mq {

bool lds_groupby_prog_eligible(const DevPlan& p, const AggProgArgs& ap, const FragView& fv, int n_cus) {
  LdsProgArgs a;
  return make_lds_prog_args(p, ap, fv, n_cus, tune_knobs().flags, &a);
}
hipError_t launch_lds_groupby_prog(const DevPlan& p, const AggProgArgs& ap, const FragView& fv, int64_t* out, int32_t* d_err, int n_cus,
                                   hipStream_t, LaunchStats* st) {
  LdsProgArgs a;
  if (!make_lds_prog_args(p, ap, fv, n_cus, tune_knobs().flags, &a)) return hipErrorInvalidValue;
  st->kernel_name = "k_groupby_lds_prog";
  st->n_launches = 1;
  st->variant = a.l.windows > 1 ? 7 : 6;
  auto value = [](const int8_t* base, int type, int64_t pos) -> int64_t {
    return type == MI355Q_INT32 ? (int64_t)((const int32_t*)base)[pos] : type == MI355Q_INT8 ? (int64_t)base[pos] : ((const int64_t*)base)[pos];
  };
  for (int f = 0; f < fv.n_frags; ++f) {
    const int8_t* const* fc = fv.d_cols + (size_t)f * fv.n_cols;
    const int64_t n = fv.d_num_rows[f];
    std::vector<std::vector<int64_t>> tmp((size_t)a.n_progs, std::vector<int64_t>((size_t)n + 1));
    std::vector<const int8_t*> cols(fc, fc + fv.n_cols);
    for (int k = 0; k < a.n_progs; ++k) cols.push_back((const int8_t*)tmp[(size_t)k].data());
    for (int64_t pos = 0; pos < n; ++pos) {
      bool pass = true;
      for (int i = 0; i < a.l.n_flt; ++i)
        pass = pass && fast::filter_pass<int64_t>(a.l.flt[i], value(fc[a.l.flt[i].col], a.l.flt_type[i], pos));
      int64_t vals[1][kApMaxCols] = {};
      for (int c = 0; c < a.n_cols; ++c) vals[0][c] = value(fc[a.col[c]], a.col_w8[c] ? MI355Q_INT64 : MI355Q_INT32, pos);
      for (int k = 0; k < a.n_progs; ++k) {
        int64_t v[1];
        int32_t e[1];
        rp_eval<1, kApMaxCols, false>(a.prog[k], vals, v, e);
        if (e[0] && pass) {
          atomicCAS(d_err, 0, e[0]);
          return hipSuccess;
        }
        if (a.l.v[k].type == MI355Q_INT32) ((int32_t*)tmp[(size_t)k].data())[pos] = (int32_t)v[0];  // (a plain column of the argument's type)
        else tmp[(size_t)k][(size_t)pos] = v[0];
      }
      if (const int32_t e = process_row<true>(p, cols.data(), pos, out, nullptr)) {
        atomicCAS(d_err, 0, e);
        return hipSuccess;
      }
    }
  }
  return hipSuccess;
}

// ... and of the star member (k_join_group_code + k_star_groupby_lds): the member's own description decides who is eligible
// (lds_args.h make_star_args); a launch gathers the inner columns of a fragment into temporary columns through the join
// table — the column's NULL for the unmatched row a LEFT join keeps, an INNER join's unmatched rows left out — and runs the
// flattened plan's row function over them.
bool star_groupby_eligible(const StarStep& step, const FragView& fv, int n_cus, int64_t* map_bytes) {
  StarCodeArgs c;
  StarArgs a;
  if (!make_star_args(step, fv, n_cus, tune_knobs().flags, &c, &a)) return false;
  *map_bytes = star_map_bytes(c);
  return true;
}
hipError_t launch_star_groupby(const StarStep& step, const FragView& fv, void* code_map, int64_t* out, int32_t* d_err, int n_cus,
                               hipStream_t, LaunchStats* st) {
  StarCodeArgs c;
  StarArgs a;
  if (!make_star_args(step, fv, n_cus, tune_knobs().flags, &c, &a) || !code_map) return hipErrorInvalidValue;
  st->kernel_name = "k_star_groupby_lds";
  st->n_launches = 2;
  st->variant = a.code16 ? 8 : 9;
  const auto null_of = [](int type) -> int64_t {
    return type == MI355Q_DOUBLE ? kNullDoubleBits : plain_int_null(type);
  };
  for (int f = 0; f < fv.n_frags; ++f) {
    const int8_t* const* fc = fv.d_cols + (size_t)f * fv.n_cols;
    const int64_t n = fv.d_num_rows[f];
    std::vector<std::vector<int64_t>> tmp((size_t)step.n_inner, std::vector<int64_t>((size_t)n + 1));
    std::vector<const int8_t*> cols(fc, fc + fv.n_cols);
    for (int j = 0; j < step.n_inner; ++j) cols.push_back((const int8_t*)tmp[(size_t)j].data());
    for (int64_t pos = 0; pos < n; ++pos) {
      const int64_t k = step.key_type == MI355Q_INT32 ? (int64_t)((const int32_t*)fc[step.key_col])[pos] : ((const int64_t*)fc[step.key_col])[pos];
      int64_t row = -1;
      if (!(step.key_nullable && k == plain_int_null(step.key_type)) && k >= step.key_min && k - step.key_min < step.n_slots)
        row = step.table[k - step.key_min];
      if (row >= step.inner_rows) row = -1;
      if (row < 0 && !step.left) continue;
      for (int j = 0; j < step.n_inner; ++j) {
        const int w = plain_width(step.inner_type[j]);
        int64_t v = null_of(step.inner_type[j]);
        if (row >= 0) {
          const int8_t* b = step.inner_base[j];
          v = w == 1 ? (int64_t)b[row] : w == 2 ? (int64_t)((const int16_t*)b)[row] : w == 4 ? (int64_t)((const int32_t*)b)[row] : ((const int64_t*)b)[row];
        }
        int8_t* dst = (int8_t*)tmp[(size_t)j].data();
        if (w == 1) dst[pos] = (int8_t)v;
        else if (w == 2) ((int16_t*)dst)[pos] = (int16_t)v;
        else if (w == 4) ((int32_t*)dst)[pos] = (int32_t)v;
        else ((int64_t*)dst)[pos] = v;
      }
      if (const int32_t e = process_row<true>(step.flat, cols.data(), pos, out, nullptr)) {
        atomicCAS(d_err, 0, e);
        return hipSuccess;
      }
    }
  }
  return hipSuccess;
}

}  // namespace mq
#endif
