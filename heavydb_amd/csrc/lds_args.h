// lds_args.h — the plan as the LDS group-by families see it (kernels_lds.hip: the table replicated / windowed in every
// workgroup's LDS; kernels_idx.hip: perfect-hash tables too large for that, partitioned by entry index).
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "boolfilter.h"
#include "fast_common.h"
#include "regprog.h"

namespace mq {

using namespace fast;

constexpr int kLdsVals = 3;              // value columns
constexpr int kLdsKeys = 3;              // key columns (perfect hash)
constexpr int kLdsGenericFlt = 4;        // filter columns of the run-time-role member's widest instantiation (NF)
constexpr uint32_t kLdsHashSmall = 256;  // slots of one baseline replica, first attempt (many replicas)
constexpr uint32_t kLdsHashMax = 4096;   // ... at most, second attempt
constexpr uint32_t kLdsMaxWindows = 8;   // windows of a table that does not fit one LDS (the columns are read once per window)
constexpr size_t kLdsBudget = 152 * 1024;  // dynamic LDS of one workgroup (one workgroup per CU): replicas + the "full" word

struct LdsVal {
  int32_t col, type, nullable;           // type: MI355Q_INT32 / _INT64 / _DOUBLE (plain)
  int32_t off_cnt, off_sum, off_min, off_max;  // byte offsets of the arrays inside a replica, -1 = not kept
};
struct LdsArgs {
  int32_t n_vals, n_flt, n_keys;
  int32_t baseline;                      // 0: perfect-hash index; 1: open addressing on one 8-byte key
  uint32_t entries;                      // arrays' length: entries of ONE window (perfect), or the hash slots (power of two)
  uint32_t windows;                      // T >= 1: workgroup b keeps the rows of window b % T
  int32_t copies_lg;                     // log2(K)
  uint32_t copy_bytes;                   // bytes of one replica (16-byte multiple)
  int32_t off_rows, off_keys;            // rows[entries] (u32); keys[entries] (int64, baseline)
  LdsVal v[kLdsVals];
  RangeFilter flt[MI355Q_MAX_QUALS];
  int32_t flt_type[MI355Q_MAX_QUALS];
  int32_t key_col[kLdsKeys], key_type[kLdsKeys], key_translate[kLdsKeys];
  int64_t key_min[kLdsKeys], key_card[kLdsKeys], key_mul[kLdsKeys], key_null_key[kLdsKeys];
  int32_t target_v[MI355Q_MAX_TARGETS];  // index into v[] of each target's argument, -1 = none
  // typed members (k_groupby_lds_typed): every value column a plain INT32, no quals; one replica =
  //   keys[E] i64 (baseline) | sum[NV][E] i64 | rows[E] u32 | cnt[NV][E] u32 | min[NV][E] i32 | max[NV][E] i32 (mm only)
  int32_t typed, mm;
  uint32_t xcd_aware;                    // windows: stripe-mates on one XCD (lds_window_map); set by the launcher
  uint32_t t_off_keys, t_off_sum, t_off_rows, t_off_cnt, t_off_min, t_off_max;
  // a filter compiled at plan time (boolfilter.h) instead of range quals: flt[k].col / flt_type[k] name its columns
  int32_t bf_on, pad_bf_;
  const BoolFilter* bf;                  // DEVICE memory
};


// What a few-groups / index-partitioned GROUP BY needs of a plan: quals, key columns (perfect hash: 1 - 3 plain integer columns
// with their ranges; baseline: one 8-byte-wide key), value columns and the accumulators the targets need of each
// (need[c] = {non-NULL count, sum, min, max}).  Perfect-hash tables of more than `max_entries` entries are refused.
// allow_int8_flt: the caller's kernels load 1-byte filter columns (kernels_lds.hip)
// vals_in_table = false: `p` is a plan over LOWERED columns (expression k is column n_cols + k, which the physical column
// table `fv` does not hold): the value columns' chunks are not looked at here — the caller checks the columns its kernel
// really reads (make_lds_prog_args)
inline bool lds_describe(const DevPlan& p, const FragView& fv, int64_t max_entries, uint32_t knob_flags, LdsArgs* out,
                         bool (&need)[kLdsVals][4], bool allow_int8_flt = false, bool vals_in_table = true) {
  LdsArgs& a = *out;
  std::memset(&a, 0, sizeof(a));
  a.windows = 1;
  if (p.desc_type == MI355Q_NON_GROUPED_AGGREGATE || p.join_col >= 0 || p.col0_key_quirk || p.slot_width != 8) return false;
  if (p.n_quals > MI355Q_MAX_QUALS) return false;
  for (int i = 0; i < p.n_quals; ++i) {
    if (!make_range_filter(p.quals[i], &a.flt[i], allow_int8_flt)) return false;
    a.flt_type[i] = p.quals[i].type;
    if (!all_aligned16(fv, p.quals[i].col)) return false;
  }
  a.n_flt = merge_range_filters(a.flt, a.flt_type, p.n_quals);
  if (p.bf_active) {  // the compiled filter's columns take the filter slots
    const BoolFilter* bf = step_bool_filter();
    if (!bf || p.n_quals != 0 || bf->n_cols > 4) return false;
    // program atoms: only in their lean form (PairAtom: INT32 operands, one operation), at most kLdsFusedProgs of them, and
    // only in the typed member (make_lds_args) — everything else takes the row-mask pre-pass (kernels_filter.hip)
    if (bf->n_progs != 0 && !(bf->all_lean && bf->all_i32 && bf->n_progs <= kLdsFusedProgs)) return false;
    for (int k = 0; k < bf->n_cols; ++k) {
      if (!all_aligned16(fv, bf->col[k])) return false;
      a.flt[k] = no_filter();
      a.flt[k].col = bf->col[k];
      a.flt_type[k] = bf->col_type[k];
    }
    a.n_flt = bf->n_cols;
    a.bf_on = 1;
    a.bf = step_bool_filter_dev();
  }
  // keys
  if (p.desc_type == MI355Q_GROUP_BY_PERFECT_HASH) {
    if (p.n_group < 1 || p.n_group > kLdsKeys || p.entry_count < 1 || p.entry_count > max_entries) return false;
    for (int g = 0; g < p.n_group; ++g) {
      if (p.group_types[g] != MI355Q_INT32 && p.group_types[g] != MI355Q_INT64) return false;
      if (p.group_bucket[g] != 0 || !all_aligned16(fv, p.group_cols[g])) return false;
      a.key_col[g] = p.group_cols[g];
      a.key_type[g] = p.group_types[g];
      a.key_translate[g] = p.group_translate[g];
      a.key_min[g] = p.group_min[g];
      a.key_card[g] = p.group_card[g];
      a.key_mul[g] = p.group_mul[g];
      a.key_null_key[g] = p.group_null_key[g];
      if (g > 0 && p.group_mul[g] < p.group_mul[g - 1]) return false;  // (the flush divides in descending order)
    }
    a.n_keys = p.n_group;
    a.entries = (uint32_t)p.entry_count;
  } else if (p.desc_type == MI355Q_GROUP_BY_BASELINE_HASH) {
    // one 8-byte-wide key column (BIGINT, or DOUBLE as its bit pattern); 4-byte integer keys take the value
    // sign-extended, FLOAT keys the bit pattern of the double they widen to
    if (p.n_group != 1) return false;
    const int kt = p.group_types[0];
    if (kt != MI355Q_INT64 && kt != MI355Q_DOUBLE && kt != MI355Q_INT32 && kt != MI355Q_FLOAT) return false;
    if (!all_aligned16(fv, p.group_cols[0])) return false;
    a.key_col[0] = p.group_cols[0];
    a.key_type[0] = kt;
    a.n_keys = 1;
    a.baseline = 1;
    // the group count of a baseline table is only known afterwards: first 256-slot replicas (a table with a handful
    // of groups gets one replica per few lanes), then the largest replica that fits, then kLdsMaxWindows windows (classes
    // of a key hash) of it, then another family.  (Round 4 tried to size the second attempt from the table's entry count
    // — the caller's NDV guess x 2 — and skip the first: the reference's default guess is 16 384 whatever the data holds
    // (g_default_max_groups_buffer_entry_guess, Execute.cpp:111), so BH001's ten groups got three windows and ran 2.4 x
    // slower, 5.5 -> 13.5 ms per 1 B rows, profiles/r04_refbench_sel_call5.jsonl; reverted.)
    // (Also measured: FOUR windows as the third attempt where an NDV estimate says the groups fill them to 0.61 — BH007,
    // 10 K groups: 32.2 ms against 29.6 ms in eight, profiles/r04_refbench_bh007_four_windows_call20.jsonl: the four-window
    // tables overflow their probe limit and the eight-window rung runs after all; reverted.)
    const uint32_t fl = knob_flags;
    a.entries = (fl & (MI355Q_OPT_LDS_BASELINE_LARGE | MI355Q_OPT_LDS_BASELINE_WINDOWS)) ? kLdsHashMax : kLdsHashSmall;
    if (fl & MI355Q_OPT_LDS_BASELINE_WINDOWS) a.windows = kLdsMaxWindows;
  } else {
    return false;
  }
  // targets -> value columns and the accumulators each needs
  for (int c = 0; c < kLdsVals; ++c) a.v[c].off_cnt = a.v[c].off_sum = a.v[c].off_min = a.v[c].off_max = -1;
  for (int c = 0; c < kLdsVals; ++c)
    for (int k = 0; k < 4; ++k) need[c][k] = false;
  for (int i = 0; i < p.n_targets; ++i) {
    const DevTarget& t = p.targets[i];
    a.target_v[i] = -1;
    if (t.agg == MI355Q_PROJECT_KEY) continue;
    if (t.table != 0 || t.arg_f32) return false;
    if (t.agg == MI355Q_COUNT && t.col < 0) continue;
    if (t.agg != MI355Q_COUNT && t.agg != MI355Q_SUM && t.agg != MI355Q_MIN && t.agg != MI355Q_MAX && t.agg != MI355Q_AVG) return false;
    if (t.col < 0) return false;
    if (t.arg_type != MI355Q_INT32 && t.arg_type != MI355Q_INT64 && t.arg_type != MI355Q_DOUBLE) return false;
    int c = -1;
    for (int k = 0; k < a.n_vals; ++k)
      if (a.v[k].col == t.col) c = k;
    if (c < 0) {
      if (a.n_vals >= kLdsVals || (vals_in_table && !all_aligned16(fv, t.col))) return false;
      c = a.n_vals++;
      a.v[c].col = t.col;
      a.v[c].type = t.arg_type;
      a.v[c].nullable = t.skip_null;
    } else if (a.v[c].nullable != t.skip_null) {
      return false;
    }
    a.target_v[i] = c;
    if (t.skip_null) need[c][0] = true;  // (a NOT NULL column's count is the entry's `rows`)
    if (t.agg == MI355Q_SUM || t.agg == MI355Q_AVG) need[c][1] = true;
    if (t.agg == MI355Q_MIN) need[c][2] = true;
    if (t.agg == MI355Q_MAX) need[c][3] = true;
  }
  return true;
}

// one replica of the run-time-role members (k_groupby_lds, k_groupby_lds_prog): 8-byte arrays first — keys (baseline), then
// per value column sum / min / max as needed — then the 4-byte counters: rows, per value column the non-NULL count.
// Sets the offsets for `entries` entries and returns the replica's bytes (a 16-byte multiple).
inline uint32_t lds_lay_out(LdsArgs& a, const bool (&need)[kLdsVals][4], uint32_t entries) {
  uint32_t off = 0;
  a.entries = entries;
  a.off_keys = -1;
  if (a.baseline) {
    a.off_keys = (int32_t)off;
    off += entries * 8;
  }
  for (int c = 0; c < a.n_vals; ++c)
    for (int k = 1; k < 4; ++k) {
      int32_t& o = k == 1 ? a.v[c].off_sum : k == 2 ? a.v[c].off_min : a.v[c].off_max;
      o = -1;
      if (need[c][k]) {
        o = (int32_t)off;
        off += entries * 8;
      }
    }
  a.off_rows = (int32_t)off;
  off += entries * 4;
  for (int c = 0; c < a.n_vals; ++c) {
    a.v[c].off_cnt = -1;
    if (need[c][0]) {
      a.v[c].off_cnt = (int32_t)off;
      off += entries * 4;
    }
  }
  return (off + 15u) & ~15u;
}

// ---- k_groupby_lds_prog (kernels_lds.hip): the few-groups table around aggregate ARGUMENTS that are two-register programs
// (regprog.h AggProgArgs), evaluated on the values the kernel has loaded.  512-lane workgroups, one per CU.
constexpr int kLdsProgBlock = 512;
constexpr int kLdsProgOwnFlt = 2;  // columns read for a qual alone
// columns under range quals, after two quals on one column have become one range.  (Eight — every qual of a plan on a column
// of its own — is what the argument struct could carry; the widest member then holds more uniform state than it has scalar
// registers for and the spill reaches scratch, 12 bytes per lane.  Four, as k_scan_agg_prog has, compiles without.)
constexpr int kLdsProgFlt = 4;
// flt_src: where a range qual finds its value
enum : int32_t { LPS_OPERAND = 0 /* + operand slot */, LPS_KEY = 4 /* + key g */, LPS_OWN = 8 /* + filter-only column k */ };
struct LdsProgArgs {
  LdsArgs l;  // the table side: keys, replica layout, windows; v[] in ARGUMENT order; flt[] / flt_type[]: the merged range quals
  int32_t n_cols, n_args, n_progs, n_own;
  int32_t col[kApMaxCols], col_w8[kApMaxCols];  // operand slots: index in the column table, 8-byte values (else 4)
  int32_t arg_slot[kLdsVals];                   // a plain-column argument's operand slot
  int32_t key_slot[kLdsKeys];                   // the operand slot that holds key g's column; -1: the key is loaded on its own
  int32_t flt_src[MI355Q_MAX_QUALS];            // LPS_*
  int32_t own_col[kLdsProgOwnFlt], own_type[kLdsProgOwnFlt];  // MI355Q_INT32 / _INT64 / _INT8 (one word per quad)
  RegProg prog[kLdsVals];
};

// The kernel's arguments from the plan over the LOWERED columns (keys, quals, targets) + the arguments' description; false:
// not this member.  Nothing past the physical column table is indexed: the alignment of every chunk the kernel reads —
// operand, key and filter-only columns — is checked here, on the columns themselves.
inline bool make_lds_prog_args(const DevPlan& p, const AggProgArgs& ap, const FragView& fv, int n_cus, uint32_t knob_flags,
                               LdsProgArgs* out) {
  LdsProgArgs& a = *out;
  std::memset(&a, 0, sizeof(a));
  if (p.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || p.bf_active || p.n_quals > MI355Q_MAX_QUALS || p.n_group < 1 ||
      p.n_group > kLdsKeys || ap.n_args < 1 || ap.n_args > kLdsVals || ap.n_cols < 1 || ap.n_cols > kApMaxCols)
    return false;
  for (int g = 0; g < p.n_group; ++g)  // (an expression key is a lowered column: not this member's)
    if (p.group_cols[g] < 0 || p.group_cols[g] >= fv.n_cols) return false;
  for (int i = 0; i < p.n_quals; ++i)
    if (p.quals[i].col < 0 || p.quals[i].col >= fv.n_cols) return false;
  bool need[kLdsVals][4] = {};
  LdsArgs& l = a.l;
  if (!lds_describe(p, fv, 65536, knob_flags, &l, need, true, /*vals_in_table=*/false)) return false;
  if (l.baseline || l.bf_on || l.n_vals != ap.n_args || l.n_flt > kLdsProgFlt) return false;
  // value columns in ARGUMENT order (programs first): v[c] is argument c
  {
    LdsVal v2[kLdsVals];
    bool need2[kLdsVals][4];
    int to_arg[kLdsVals];
    for (int c = 0; c < l.n_vals; ++c) {
      int k = -1;
      for (int j = 0; j < ap.n_args; ++j)
        if (ap.arg_col[j] == l.v[c].col) k = j;
      if (k < 0 || ap.arg_type[k] != l.v[c].type || ap.arg_nullable[k] != l.v[c].nullable) return false;
      to_arg[c] = k;
      v2[k] = l.v[c];
      for (int j = 0; j < 4; ++j) need2[k][j] = need[c][j];
    }
    for (int c = 0; c < l.n_vals; ++c) {
      l.v[c] = v2[c];
      for (int j = 0; j < 4; ++j) need[c][j] = need2[c][j];
    }
    for (int i = 0; i < p.n_targets; ++i)
      if (l.target_v[i] >= 0) l.target_v[i] = to_arg[l.target_v[i]];
  }
  a.n_cols = ap.n_cols;
  a.n_args = ap.n_args;
  a.n_progs = ap.n_progs;
  for (int k = 0; k < ap.n_cols; ++k) {
    if (!rp_type_ok(ap.col_type[k]) || ap.col[k] < 0 || ap.col[k] >= fv.n_cols || !all_aligned16(fv, ap.col[k])) return false;
    a.col[k] = ap.col[k];
    a.col_w8[k] = ap.col_type[k] == MI355Q_INT32 ? 0 : 1;
  }
  for (int c = 0; c < ap.n_args; ++c) {
    a.arg_slot[c] = c < ap.n_progs ? 0 : ap.arg_slot[c];
    a.prog[c] = ap.prog[c];
  }
  // a key column that is also an operand column is loaded once
  for (int g = 0; g < l.n_keys; ++g) {
    a.key_slot[g] = -1;
    for (int k = 0; k < ap.n_cols; ++k)
      if (ap.col[k] == l.key_col[g] && ap.col_type[k] == l.key_type[g]) a.key_slot[g] = k;
  }
  // a range qual tests a value already loaded where its column is an operand or key column
  for (int i = 0; i < l.n_flt; ++i) {
    int src = -1;
    for (int k = 0; k < ap.n_cols; ++k)
      if (ap.col[k] == l.flt[i].col && ap.col_type[k] == l.flt_type[i]) src = LPS_OPERAND + k;
    for (int g = 0; g < l.n_keys && src < 0; ++g)
      if (l.key_col[g] == l.flt[i].col && l.key_type[g] == l.flt_type[i]) src = LPS_KEY + g;
    for (int k = 0; k < a.n_own && src < 0; ++k)
      if (a.own_col[k] == l.flt[i].col && a.own_type[k] == l.flt_type[i]) src = LPS_OWN + k;
    if (src < 0) {
      if (a.n_own >= kLdsProgOwnFlt) return false;
      a.own_col[a.n_own] = l.flt[i].col;
      a.own_type[a.n_own] = l.flt_type[i];
      src = LPS_OWN + a.n_own++;
    }
    a.flt_src[i] = src;
  }
  // the replica layout: as many replicas as fit; a table beyond one LDS in the fewest windows whose share fits
  l.copy_bytes = lds_lay_out(l, need, l.entries);
  if (l.copy_bytes > kLdsBudget) {
    const uint32_t total = (uint32_t)p.entry_count;
    for (uint32_t T = 2; T <= kLdsMaxWindows; ++T) {
      const uint32_t share = (total + T - 1) / T;
      if (lds_lay_out(l, need, share) <= kLdsBudget) {
        l.windows = T;
        l.copy_bytes = lds_lay_out(l, need, share);
        break;
      }
    }
    if (l.windows == 1) return false;
  }
  l.copies_lg = 0;
  while (l.copies_lg < 6 && ((size_t)l.copy_bytes << (l.copies_lg + 1)) <= kLdsBudget) ++l.copies_lg;
  // the per-entry counters are 32 bits wide per workgroup: a stripe stays below 2^32 rows (as make_lds_args)
  int64_t stripes = (n_cus > 0 ? n_cus : 1) / (int64_t)l.windows;
  if (stripes < 1) stripes = 1;
  if (fv.total_rows / stripes >= 0xfff00000ll) return false;
  return true;
}

// ---- the star member (kernels_lds.hip k_join_group_code + k_star_groupby_lds; api_routes.cpp execute_inner_refs): a few-groups
// GROUP BY keyed by DIMENSION attributes over fact JOIN dim with a one-to-one perfect join table.  k_join_group_code maps every
// join-table slot to the entry index of its dimension row's group once per step; the hot scan then needs ONE gather per fact
// row — code[key - min_key] — in place of the probe, the attribute loads and the perfect-hash arithmetic, and no temporary
// column.  Codes: >= 0 the entry index; kStarDrop (-1) the row does not count (an inner qual rejects its dimension row, or, as
// `code_unmatched` of an INNER join, it has none); kStarBadKey (-2) an attribute outside its declared range (the row raises
// MI355Q_ERR_OUT_OF_SLOTS, as the family does for such a key).  An EMPTY slot of the join table holds the step's constant
// `code_unmatched` itself — what a NULL fact key and a key outside [min_key, max_key] get without looking at the map: -1 for an
// INNER join, and for a LEFT join the entry of the all-NULL key, or -1 where an inner qual is not TRUE for NULL.
constexpr int kStarBlock = 512;
constexpr int kStarOuterFlt = 2;           // outer columns under range quals
constexpr int32_t kStarDrop = -1, kStarBadKey = -2;
// maps up to here are planned by default; beyond, the member waits behind kernel_variant 2.  2-byte codes: MEASURED at 1 B rows
// with maps of 0.2, 2 and 32 MB — the member beat the flattened route 3.5 - 7.7 x in every class (DESIGN 3.9,
// profiles/star_join_bench_1b.jsonl); 4-byte codes (more than 32 767 entries) are UNMEASURED: one XCD's L2
constexpr int64_t kStarDefaultMapBytes16 = (int64_t)32 << 20, kStarDefaultMapBytes32 = (int64_t)4 << 20;
struct StarCodeArgs {                      // k_join_group_code
  const int32_t* table;                    // the join table: row id per slot, < 0 = empty
  int64_t n_slots, inner_rows;
  int32_t n_keys, n_flt, code16, code_unmatched;
  const int8_t* key_base[kLdsKeys];        // the inner key columns (plain INT32 / INT64)
  int32_t key_type[kLdsKeys], key_translate[kLdsKeys];
  int64_t key_min[kLdsKeys], key_card[kLdsKeys], key_mul[kLdsKeys], key_null_key[kLdsKeys];
  const int8_t* flt_base[MI355Q_MAX_QUALS];  // the inner columns under range quals (plain INT8 / INT32 / INT64)
  int32_t flt_type[MI355Q_MAX_QUALS];
  RangeFilter flt[MI355Q_MAX_QUALS];
  int64_t entry_count;
  void* code;                              // int16 [n_slots] (code16) or int32 [n_slots]
};
struct StarArgs {                          // k_star_groupby_lds
  LdsArgs l;                               // the table side: key_* (for the flush), v[], the replica layout; flt[0 .. n_flt): the OUTER range quals
  int32_t key_col, key_w8, key_nullable, code16;  // the fact's join key column
  int64_t key_min, n_slots;                // slot = key - key_min, 0 <= slot < n_slots
  int32_t code_unmatched, pad_;
  const void* code;
};
// what the host knows of such a step (api_routes.cpp fills it; kernels.h launch_star_groupby takes it)
struct StarStep {
  DevPlan flat;                            // the FLATTENED plan without the matched flag: inner column inner_col[j] is column nc + j
  int32_t nc, n_inner, left, key_col, key_type, key_nullable;
  int32_t inner_col[MI355Q_MAX_COLS], inner_type[MI355Q_MAX_COLS];  // plain types
  const int8_t* inner_base[MI355Q_MAX_COLS];
  int64_t inner_rows;
  const int32_t* table;
  int64_t key_min, n_slots;
};

// The two kernels' arguments from the step; false: not this member (the flattened route runs the step).
inline bool make_star_args(const StarStep& st, const FragView& fv, int n_cus, uint32_t knob_flags, StarCodeArgs* code, StarArgs* out) {
  StarArgs& a = *out;
  StarCodeArgs& c = *code;
  std::memset(&a, 0, sizeof(a));
  std::memset(&c, 0, sizeof(c));
  const DevPlan& p = st.flat;
  const int nc = st.nc, nc2 = st.nc + st.n_inner;
  if (p.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || p.bf_active || p.n_group < 1 || p.n_group > kLdsKeys || fv.n_cols != nc ||
      p.n_quals > MI355Q_MAX_QUALS || st.n_slots < 1 || st.n_slots > (int64_t)INT32_MAX || st.inner_rows < 0 || !st.table ||
      (st.key_type != MI355Q_INT32 && st.key_type != MI355Q_INT64) || !all_aligned16(fv, st.key_col))
    return false;
  // the plan's quals: inner ones for the map, outer ones for the scan
  DevPlan po = p;
  po.n_quals = 0;
  for (int i = 0; i < p.n_quals; ++i) {
    const DevQual& q = p.quals[i];
    if (q.col < nc) {
      po.quals[po.n_quals++] = q;
      continue;
    }
    if (q.col >= nc2 || !make_range_filter(q, &c.flt[c.n_flt], true)) return false;
    c.flt_type[c.n_flt++] = q.type;
  }
  c.n_flt = merge_range_filters(c.flt, c.flt_type, c.n_flt);
  for (int k = 0; k < c.n_flt; ++k) {
    const int j = c.flt[k].col - nc;
    if (st.inner_type[j] != c.flt_type[k]) return false;  // (plain columns: the qual's type is the storage type)
    c.flt_base[k] = st.inner_base[j];
  }
  // the table side, as the family describes it — over a column table in which the inner columns are (aligned) nothings
  std::vector<const void*> h2((size_t)std::max(fv.n_frags, 0) * nc2, nullptr);
  for (int f = 0; f < fv.n_frags; ++f)
    for (int k = 0; k < nc; ++k) h2[(size_t)f * nc2 + k] = fv.h_cols[(size_t)f * nc + k];
  FragView fv2 = fv;
  fv2.h_cols = h2.data();
  fv2.n_cols = nc2;
  bool need[kLdsVals][4] = {};
  LdsArgs& l = a.l;
  if (!lds_describe(po, fv2, 65536, knob_flags, &l, need, false)) return false;
  if (l.baseline || l.bf_on || l.n_flt > kStarOuterFlt) return false;
  for (int k = 0; k < l.n_flt; ++k)
    if (l.flt[k].col >= nc) return false;
  for (int v = 0; v < l.n_vals; ++v)
    if (l.v[v].col >= nc) return false;
  for (int g = 0; g < l.n_keys; ++g) {
    const int j = l.key_col[g] - nc;
    if (j < 0 || j >= st.n_inner || st.inner_type[j] != l.key_type[g]) return false;  // (every key an inner attribute, plain INT32 / INT64)
    c.key_base[g] = st.inner_base[j];
    c.key_type[g] = l.key_type[g];
    c.key_translate[g] = l.key_translate[g];
    c.key_min[g] = l.key_min[g];
    c.key_card[g] = l.key_card[g];
    c.key_mul[g] = l.key_mul[g];
    c.key_null_key[g] = l.key_null_key[g];
  }
  // ONE window under the budget, as many replicas as fit
  l.copy_bytes = lds_lay_out(l, need, l.entries);
  if (l.copy_bytes > kLdsBudget) return false;
  l.copies_lg = 0;
  while (l.copies_lg < 6 && ((size_t)l.copy_bytes << (l.copies_lg + 1)) <= kLdsBudget) ++l.copies_lg;
  if (fv.total_rows / (n_cus > 0 ? n_cus : 1) >= 0xfff00000ll) return false;  // (32-bit counters per workgroup, as make_lds_args)
  // what a row without a dimension row gets
  int32_t unmatched = kStarDrop;
  if (st.left) {
    bool pass = true;
    for (int k = 0; k < c.n_flt; ++k) {  // (filter_pass on the column's NULL, on the host)
      const RangeFilter& f = c.flt[k];
      const int64_t x = int_null_of(c.flt_type[k]);
      bool in = x >= f.lo && x <= f.hi;
      if (f.negate) in = !in;
      pass = pass && in && !(f.nullable && x == f.null_val);
    }
    int64_t idx = 0;
    for (int g = 0; g < l.n_keys && pass; ++g) {
      const int64_t d = l.key_null_key[g] - l.key_min[g];
      if (!l.key_translate[g] || d < 0 || d >= l.key_card[g]) return false;  // (no entry for the NULL key: not this member's plan)
      idx += d * l.key_mul[g];
    }
    if (pass && (idx < 0 || idx >= p.entry_count)) return false;
    if (pass) unmatched = (int32_t)idx;
  }
  c.table = st.table;
  c.n_slots = st.n_slots;
  c.inner_rows = st.inner_rows;
  c.n_keys = l.n_keys;
  c.entry_count = p.entry_count;
  c.code16 = p.entry_count <= 32767;
  c.code_unmatched = unmatched;
  a.key_col = st.key_col;
  a.key_w8 = st.key_type == MI355Q_INT64;
  a.key_nullable = st.key_nullable;
  a.code16 = c.code16;
  a.key_min = st.key_min;
  a.n_slots = st.n_slots;
  a.code_unmatched = unmatched;
  return true;
}
inline int64_t star_map_bytes(const StarCodeArgs& c) { return (c.n_slots * (c.code16 ? 2 : 4) + 255) & ~(int64_t)255; }

}  // namespace mq
