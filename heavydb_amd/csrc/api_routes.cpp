// api_routes.cpp — the derived-plan routes of the step executor (api.cpp execute_impl asks them in turn).  Each route
// rewrites the stated plan into a simpler one, runs that through mi355q_execute and fixes the result up.  What they
// share: RouteScope (api_internal.h: device, context lock, stream, timing events, the common tail), PassLoop (the
// routes that lay temporary columns beside the stated ones, one pass of fragments at a time) and Emission (the routes
// that end by re-emitting a derived table into the stated layout).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "boolfilter.h"
#include "lds_args.h"

namespace mq {
namespace api {
namespace {

// bytes the temporary columns of one pass may take: a third of the free memory (what the workspace already holds counts
// as free), 16 GB at most
int64_t pass_budget(int64_t held_bytes) {
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  return std::min<int64_t>((int64_t)16 << 30, ((int64_t)free_b + held_bytes) / 3);
}

// ------------------------------------------------------------------------------- the pass loop
// The routes whose derived step reads TEMPORARY columns beside the stated ones (join gather: the inner side's columns and
// the matched flag; join expansion: the joined rows, stated columns included; affine twin: lattice indices; projection: the
// expressions' values; mask: the compiled filter's row mask).  The columns of one PASS of fragments live in a DeviceCtx workspace sized from the free memory; per pass the
// route's own pre-pass kernel fills them, the derived plan runs over the pass, and the passes' results are folded with
// the reduce rule.  Workspace layout (every part 256-byte rounded):
//   column chunks | pointer table | bytes_after_tab | row counts | 256 (64 error bytes) | bytes_after_err
struct PassLoop {
  // ---- stated by the route
  Workspace& ws;                   // the DeviceCtx workspace to grow
  int nc;                          // stated columns; the temporary ones follow them in the derived step's table
  int n_extra;                     // temporary columns
  const int32_t* width;            // their widths in bytes
  const mi355q_plan* derived;      // the plan every pass runs
  int64_t bytes_after_tab = 0;     // mask: its second pointer table (the mask chunk of every fragment)
  int64_t bytes_after_err = 0;     // projection: the lowered programs (DevExprSet)
  // mask route only.  One switch with THREE consequences, which come together (a user that wants one of them alone
  // has to split it): (1) padding: 32 bytes per fragment instead of 16 per column and fragment; (2) chunk length:
  // filter_mask_chunk_bytes(rows) instead of (rows x width) rounded to 16; (3) the pointer table the pre-pass reads: the
  // nc STATED columns of every fragment, copied from in->col_buffers, instead of the nc + n_extra columns of cols2
  bool mask_column = false;
  // what a failed workspace allocation answers: kNotTaken (join gather, affine twin: the plain route needs no temporary
  // columns) or MI355Q_ERR_OUT_OF_GPU_MEM with last_hip_error set (projection, mask)
  int32_t alloc_failed = kNotTaken;
  bool clear_err_word = true;          // join gather's pre-pass raises nothing: no word to clear
  bool count_pre_pass = true;          // the pre-pass is a launch of the report: everyone but the projection
  bool first_into_out_buffer = true;   // the first pass writes the caller's buffer: everyone but the affine twin (it emits)
  // affine twin: an inner step that is unsupported, out of memory, out of slots or retrying (< 0) gives the ROUTE up
  // (kNotTaken); everyone else hands the inner step's code on
  bool inner_errors_not_taken = false;
  // affine twin: every pass's result must be the perfect-hash twin that was planned (else kNotTaken); null: no check
  const mi355q_qmd* twin = nullptr;
  // join expansion only: the derived step runs over the JOINED rows.  derived_rows[f] = rows of the derived fragment that
  // outer fragment f becomes: what cuts the passes, sizes the chunks and is the derived step's num_rows (a fragment nothing
  // of which joins is left out of its pass's derived step); stated_tmp_width[c] != 0: stated column c is a temporary column
  // of that storage width too (the pre-pass writes it), 0: the derived step does not read column c — its entry points at the
  // fragment's first temporary chunk, which is valid, aligned and never read.  The pre-pass reads the caller's columns from
  // a table of its own; d_tab is the derived step's table of ALL fragments of the pass, d_rows the OUTER row counts.
  const int64_t* derived_rows = nullptr;
  const int32_t* stated_tmp_width = nullptr;

  // ---- laid out by prepare()
  int nc2 = 0;
  int64_t pass_rows = 0, col_region = 0, tab_bytes = 0, rows_bytes = 0;
  char* base = nullptr;
  const int8_t** d_tab = nullptr;
  char* after_tab = nullptr;
  int64_t* d_rows = nullptr;
  int32_t* d_err = nullptr;
  char* after_err = nullptr;
  std::vector<const void*> cols2;  // the current pass's column table of the derived step (nc2 per fragment)
  // ---- left by run()
  ResultPtr res;                   // all passes folded
  mi355q_exec_report acc{};

  PassLoop(Workspace& ws_, int nc_, int n_extra_, const int32_t* width_, const mi355q_plan* derived_)
      : ws(ws_), nc(nc_), n_extra(n_extra_), width(width_), derived(derived_) {}

  // sizes a pass within `budget` bytes of temporary columns (o.pass_rows: the tests' override): the bytes the workspace must hold
  int64_t lay_out(const mi355q_inputs* in, const mi355q_exec_options& o, int64_t total_rows, int64_t max_frag_rows, int64_t budget) {
    const int nf = in->n_frags;
    nc2 = nc + n_extra;
    int64_t row_bytes = 0;
    for (int k = 0; k < n_extra; ++k) row_bytes += width[k];
    int n_tmp = n_extra;
    for (int c = 0; stated_tmp_width && c < nc; ++c) {
      row_bytes += stated_tmp_width[c];
      n_tmp += stated_tmp_width[c] != 0;
    }
    // every (fragment, column) chunk starts on a 16-byte boundary: the fast families want aligned columns
    // (worst case: every fragment of a pass pads every chunk once)
    const int64_t pad = mask_column ? 32 : 16 * (int64_t)n_tmp;
    pass_rows = std::max<int64_t>(budget / std::max<int64_t>(row_bytes, 1), max_frag_rows);
    if (o.pass_rows > 0) pass_rows = std::max<int64_t>(o.pass_rows, max_frag_rows);  // tests: several passes
    if (pass_rows > total_rows) pass_rows = total_rows;
    tab_bytes = ((int64_t)sizeof(void*) * nf * (mask_column ? nc : nc2) + 255) & ~255ll;
    rows_bytes = ((int64_t)sizeof(int64_t) * nf + 255) & ~255ll;
    col_region = ((pass_rows * row_bytes + pad * nf) + 255) & ~255ll;
    return col_region + tab_bytes + bytes_after_tab + rows_bytes + 256 + bytes_after_err;
  }

  // sizes a pass from the free memory and grows the workspace to hold it
  int32_t prepare(const mi355q_inputs* in, const mi355q_exec_options& o, int64_t total_rows, int64_t max_frag_rows) {
    const int64_t need = lay_out(in, o, total_rows, max_frag_rows, pass_budget(ws.bytes));
    if (const hipError_t he = ws.grow(need)) {
      if (alloc_failed != kNotTaken) last_hip_error = he;
      (void)hipGetLastError();
      return alloc_failed;
    }
    base = (char*)ws.p;
    d_tab = (const int8_t**)(base + col_region);
    after_tab = base + col_region + tab_bytes;
    d_rows = (int64_t*)(after_tab + bytes_after_tab);
    d_err = (int32_t*)((char*)d_rows + rows_bytes);
    after_err = (char*)d_err + 256;
    return MI355Q_OK;
  }

  // pre_pass(f, pnf) -> int32_t: fragments [f, f + pnf) are in cols2 and their pointer table is on its way to d_tab; the
  // route launches its kernel on d_tab / d_rows + f, reads back what it raises and SYNCHRONISES (cols2 is re-used by the
  // next pass).  The timed span of the route starts here, behind the two set-up copies.
  template <class PrePass>
  int32_t run(RouteScope& rs, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_exec_report* report,
              PrePass&& pre_pass) {
    const int nf = in->n_frags;
    hipStream_t s = rs.s;
    if (clear_err_word) HIP_TRY(hipMemsetAsync(d_err, 0, 64, s));
    HIP_TRY(hipMemcpyAsync(d_rows, in->num_rows, sizeof(int64_t) * (size_t)nf, hipMemcpyHostToDevice, s));
    if (!rs.ev0)  // (the join expansion has begun the span already: its count and scan run ahead of the passes)
      if (int32_t e = rs.begin_timing(report)) return e;
    cols2.resize((size_t)nf * nc2);
    const int64_t* frag_rows = derived_rows ? derived_rows : in->num_rows;
    std::vector<int64_t> rows2;  // join expansion: the row counts of the derived fragments a pass runs over
    int pass = 0, f = 0;
    while (f < nf) {
      // a pass holds at least one fragment; the next one joins while the pass stays within pass_rows
      int f1 = f;
      int64_t rows = 0, off = 0;
      while (f1 < nf && (f1 == f || rows + frag_rows[f1] <= pass_rows)) {
        const char* first_tmp = base + off;
        for (int c = 0; c < nc; ++c) {
          const void*& col = cols2[(size_t)(f1 - f) * nc2 + c];
          if (stated_tmp_width && stated_tmp_width[c]) {
            col = base + off;
            off += (frag_rows[f1] * stated_tmp_width[c] + 15) & ~15ll;
          } else {
            col = derived_rows ? (const void*)first_tmp : in->col_buffers[(size_t)f1 * nc + c];
          }
        }
        for (int k = 0; k < n_extra; ++k) {
          cols2[(size_t)(f1 - f) * nc2 + nc + k] = base + off;
          off += mask_column ? filter_mask_chunk_bytes(frag_rows[f1]) : (frag_rows[f1] * width[k] + 15) & ~15ll;
        }
        rows += frag_rows[f1];
        ++f1;
      }
      if (off > col_region) return MI355Q_ERR_OUT_OF_GPU_MEM;  // (cannot happen: the region is sized for it)
      const int pnf = f1 - f;
      if (mask_column)
        HIP_TRY(hipMemcpyAsync(d_tab, in->col_buffers + (size_t)f * nc, sizeof(void*) * (size_t)pnf * nc, hipMemcpyHostToDevice, s));
      else
        HIP_TRY(hipMemcpyAsync(d_tab, cols2.data(), sizeof(void*) * (size_t)pnf * nc2, hipMemcpyHostToDevice, s));
      if (int32_t e = pre_pass(f, pnf)) return e;
      mi355q_inputs in2 = *in;
      in2.n_frags = pnf;
      in2.col_buffers = cols2.data();
      in2.num_rows = in->num_rows + f;
      if (derived_rows) {  // the pass's derived fragments: the ones that have rows (the pre-pass has synchronised: cols2 is ours again)
        rows2.clear();
        for (int i = 0; i < pnf; ++i) {
          if (derived_rows[f + i] <= 0) continue;
          if ((size_t)i != rows2.size()) std::copy_n(&cols2[(size_t)i * nc2], nc2, &cols2[rows2.size() * nc2]);
          rows2.push_back(derived_rows[f + i]);
        }
        in2.n_frags = (int32_t)rows2.size();
        in2.num_rows = rows2.data();
        if (rows2.empty()) {  // (cannot happen while something joins: rowless fragments ride with their neighbours)
          f = f1;
          continue;
        }
      }
      mi355q_exec_options o2 = o;
      o2.stream = s;
      o2.out_buffer = pass == 0 && first_into_out_buffer ? o.out_buffer : nullptr;
      mi355q_result* r2 = nullptr;
      mi355q_exec_report rep2{};
      if (int32_t e2 = mi355q_execute(derived, &in2, &o2, &r2, &rep2)) {
        if (inner_errors_not_taken &&
            (e2 == MI355Q_ERR_UNSUPPORTED || e2 == MI355Q_ERR_OUT_OF_GPU_MEM || e2 < 0 || e2 == MI355Q_ERR_OUT_OF_SLOTS))
          return kNotTaken;
        return e2;
      }
      ResultPtr pass_res(r2);
      if (twin && (r2->qmd.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || r2->qmd.slot_width != 8 || r2->qmd.output_columnar ||
                   r2->qmd.entry_count != twin->entry_count))
        return kNotTaken;
      if (pass == 0) {  // the report names the member the first (a full-sized) pass ran
        res = std::move(pass_res);
        std::snprintf(acc.kernel_name, sizeof(acc.kernel_name), "%s", rep2.kernel_name);
        acc.variant = rep2.variant;
      } else if (int32_t er = mi355q_result_reduce(res.get(), r2, s)) {
        return er;
      }
      acc.kernel_ms += rep2.kernel_ms;
      acc.n_launches += rep2.n_launches + (count_pre_pass ? 1 : 0);
      acc.spilled_rows += rep2.spilled_rows;
      f = f1;
      ++pass;
    }
    return MI355Q_OK;
  }
};

// The emit epilogue of the routes that re-key / zip a derived table into the stated layout: the stated result, initialised
// EMPTY (result_create_impl only allocates; the emit kernels claim their keys with CAS), and a cleared device error word
// for the emit kernel.  RouteScope::finish reads the word back; the route then releases `res` to the caller.
struct Emission {
  ResultPtr res;
  DevWord err;
  int32_t* d_err() const { return (int32_t*)err.p; }
  int32_t create(const mi355q_qmd& q, int32_t device_id, void* out_buffer, hipStream_t s) {
    mi355q_result* r = nullptr;
    if (int32_t e = result_create_impl(&q, device_id, out_buffer, &r)) return e;
    res.reset(r);
    HIP_TRY(launch_init_buffer(res->buf, q.entry_count, make_row_init(q), s));
    HIP_TRY(hipMalloc(&err.p, 64));
    HIP_TRY(hipMemsetAsync(err.p, 0, 64, s));
    return MI355Q_OK;
  }
};

// ------------------------------------------------------------------------------- packed keys
// Baseline-hash GROUP BY over several columns whose ranges together fit 62 bits: pack the key
// columns of every row into one int64 column (one streaming pass), run the step on that column
// with the single-key fast family (partition-then-aggregate), and re-emit the finished table
// with the real key components — MurmurHash3 over the key bytes, the reference's layout.  The
// slots of a row are the same in both tables (key projections take no slot in the baseline
// layout), so the re-emission copies them.  Anything this cannot take (no ranges, too many
// bits, joins, small inputs) stays with the row kernel.
bool pack_spec_of(const mi355q_plan& p, const mi355q_qmd& q, const DevPlan& d, PackSpec* ps) {
  if (p.join_outer_col >= 0 || p.n_group_cols < 1 || d.col0_key_quirk) return false;
  std::memset(ps, 0, sizeof(*ps));
  ps->n = p.n_group_cols;
  // ONE plain FLOAT key on a baseline table: the table stores the double it widens to, so the "packed" column is that
  // double's bit pattern and the single-key families (which read 8-byte keys) take the step — the reference
  // benchmark's GROUP BY cast(x AS FLOAT) (MultiStep/MSBS001-005)
  if (p.n_group_cols == 1 && q.desc_type == MI355Q_GROUP_BY_BASELINE_HASH && p.cols[p.group_cols[0]].type == MI355Q_FLOAT &&
      p.cols[p.group_cols[0]].encoding == MI355Q_ENC_NONE && q.key_width == 8) {
    ps->raw_f32 = 1;
    ps->cols[0] = p.group_cols[0];
    ps->types[0] = d.group_types[0];
    return true;
  }
  for (int g = 0; g < p.n_group_cols; ++g)  // other floating-point keys have no integer range to pack
    if (type_is_fp(p.cols[p.group_cols[g]].type) || type_is_f32(p.cols[p.group_cols[g]].type)) return false;
  if (q.desc_type == MI355Q_GROUP_BY_PERFECT_HASH) {
    // single-column tables that fit LDS already have their kernel; multi-column ones reach it
    // through the packed index (mode 2); bucketed keys cannot be restored from their index
    const bool small = q.entry_count * (int64_t)q.row_size <= 64 * 1024;
    // one plain NOT NULL INT / BIGINT (or FIXED(32)) key: k_perfect_lds reads it natively.  Every other
    // single key — dictionary ids, FIXED(8/16), DATE in days, nullable (translated) keys — reaches the
    // same kernel through the index column the pack kernel decodes it into.
    if (small && p.n_group_cols < 2) {
      const mi355q_col_desc& kc = p.cols[p.group_cols[0]];
      const int tc = d.group_types[0];
      const bool native = !kc.nullable && !q.group_bucket[0] &&
                          (tc == MI355Q_INT32 || tc == MI355Q_INT64 ||
                           (tc_enc(tc) == MI355Q_ENC_FIXED && tc_storage(tc) == MI355Q_INT32));
      if (native) return false;
    }
    if (q.entry_count >= ((int64_t)1 << 31)) return false;
    ps->mode = small ? 2 : 1;
    for (int g = 0; g < p.n_group_cols; ++g) {
      // a bucketed range maps (key - min) / bucket to the index: the key can only be restored from the
      // index when every value is a multiple of the bucket above min — DATE in days decoded to seconds
      if (q.group_bucket[g] &&
          !(tc_enc(d.group_types[g]) == MI355Q_ENC_DATE_IN_DAYS && q.group_bucket[g] == 86400 && q.group_min[g] % 86400 == 0))
        return false;
      ps->bucket[g] = q.group_bucket[g];
      ps->cols[g] = p.group_cols[g];
      ps->types[g] = d.group_types[g];
      ps->translate[g] = d.group_translate[g];
      ps->min[g] = q.group_min[g];
      ps->card[g] = (uint64_t)q.group_card[g];
      ps->mul[g] = d.group_mul[g];
      ps->null_key[g] = q.group_null_key[g];
    }
    return true;
  }
  // baseline layouts: several key columns, or ONE key column whose table has 4-byte key components
  // (pick_baseline_key_width: every key fits int32 — the reference benchmark's x10k_s10k / x100k_s10k BIGINT keys):
  // the partitioned family emits 8-byte keys, so the step runs on the packed (key - min) column into a temporary
  // 8-byte-key table and k_unpack_emit lays the finished groups out with the real 4-byte components
  if (q.desc_type != MI355Q_GROUP_BY_BASELINE_HASH) return false;
  if (p.n_group_cols < 2 && q.key_width != 4) return false;
  int shift = 0;
  for (int g = 0; g < p.n_group_cols; ++g) {
    const int c = p.group_cols[g];
    const mi355q_range& r = p.col_ranges[c];
    if (!r.valid || r.min > r.max) return false;
    const __int128 span = (__int128)r.max - (__int128)r.min + 1 + (p.cols[c].nullable ? 1 : 0);
    if (span > ((__int128)1 << 61)) return false;
    int bits = 1;
    while (((__int128)1 << bits) < span) ++bits;
    if (shift + bits > 62) return false;  // the packed key must stay below EMPTY_KEY_64
    ps->cols[g] = c;
    ps->types[g] = d.group_types[g];
    ps->nullable[g] = p.cols[c].nullable != 0;
    ps->shift[g] = shift;
    ps->min[g] = r.min;
    ps->card[g] = (uint64_t)span;
    ps->mask[g] = (((uint64_t)1) << bits) - 1;
    shift += bits;
  }
  return true;
}

}  // namespace

int32_t execute_packed_multi(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                             const mi355q_qmd& q, const DevPlan& d, int n_cus, mi355q_result** out,
                             mi355q_exec_report* report, int64_t* reserved) {
  PackSpec ps;
  // kernel_variant 1 = "the row kernel / direct members", as everywhere else
  if (o.kernel_variant == 1) return kNotTaken;
  if (!pack_spec_of(*plan, q, d, &ps)) return kNotTaken;
  const int nf = in->n_frags, nc = plan->n_cols;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  // small inputs: the row kernel is as fast (kernel_variant 2 asks for this path regardless, 1 for
  // the row kernel)
  if (o.kernel_variant == 1 || (o.kernel_variant != 2 && total_rows < ((int64_t)8 << 20))) return kNotTaken;

  // derived plan: the packed column (appended, range unknown -> baseline, 8-byte key) is the
  // only group column; key projections are dropped (they own no slot)
  mi355q_plan p2 = *plan;
  // where the packed column sits in the derived step's column table: appended — or, when the table is full
  // (MI355Q_MAX_COLS), in the place of a key column nothing else reads (its only reader, the grouping, is what the packed
  // column replaces; key projections own no slot in the derived plan)
  int pk = nc;
  if (nc >= MI355Q_MAX_COLS) {
    pk = -1;
    for (int g = 0; g < plan->n_group_cols && pk < 0; ++g) {
      const int c = plan->group_cols[g];
      bool used = false;
      for (int t = 0; t < plan->n_targets; ++t) {
        const mi355q_target& tg = plan->targets[t];
        if (tg.agg == MI355Q_PROJECT_KEY) continue;
        used = used || (tg.table == 0 && tg.col == c) ||
               ((tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) && tg.cond.col == c);
      }
      for (int k = 0; k < plan->n_quals; ++k) used = used || plan->quals[k].col == c;
      if (!used) pk = c;
    }
    if (pk < 0) return kNotTaken;
  }
  const int nc2 = pk == nc ? nc + 1 : nc;
  p2.n_cols = nc2;
  p2.cols[pk] = mi355q_col_desc{MI355Q_INT64, 0, MI355Q_ENC_NONE, 0};
  p2.col_ranges[pk] = mi355q_range{};
  p2.n_group_cols = 1;
  p2.group_cols[0] = pk;
  p2.n_targets = 0;
  for (int t = 0; t < plan->n_targets; ++t) {
    if (plan->targets[t].agg != MI355Q_PROJECT_KEY) p2.targets[p2.n_targets++] = plan->targets[t];
  }
  if (p2.n_targets == 0) return kNotTaken;
  if (ps.mode == 1) {  // a baseline table at 50 % fill for the groups of the perfect layout
    const int64_t guess = 2 * q.entry_count;
    if (guess > (int64_t)UINT32_MAX) return kNotTaken;
    p2.max_groups_buffer_entry_guess = guess;
  }
  if (ps.mode == 2) {  // the index is a perfect-hash key itself: range [0, entries)
    p2.col_ranges[pk].valid = 1;
    p2.col_ranges[pk].min = 0;
    p2.col_ranges[pk].max = q.entry_count - 1;
  }
  // the temporary table always has 8-byte slots: k_unpack_emit / k_unpack_perfect read it quad by
  // quad, and a multi-pass run reduces it with 64-bit adds (pick_target_compact_width would narrow a
  // COUNT(*)-only derived plan to 4-byte slots)
  p2.bigint_count = 1;
  mi355q_qmd q2;
  if (qmd_init(p2, &q2) != MI355Q_OK) return kNotTaken;
  if (q2.slot_width != 8 || q2.row_size % 8 != 0) return kNotTaken;
  if (ps.mode == 2) {
    if (q2.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || q2.entry_count != q.entry_count) return kNotTaken;
    ps.tmp_idx_target = q2.idx_target_as_key;
    ps.tmp_init = q2.keyless ? q2.init_vals[q2.idx_target_as_key] : 0;
  } else if (q2.desc_type != MI355Q_GROUP_BY_BASELINE_HASH) {
    return kNotTaken;
  }
  if (ps.mode == 0 && (q2.slot_count != q.slot_count || q2.entry_count != q.entry_count)) return kNotTaken;
  // where every slot of the final row comes from: a slot of the packed step's row, or (perfect
  // layouts: projected keys own a slot) the original value of a key component
  {
    int t2 = 0;
    for (int i = 0; i < MI355Q_MAX_SLOTS; ++i) ps.slot_src[i] = 0;
    for (int t = 0; t < plan->n_targets; ++t) {
      const int sf = q.target_slot[t];
      if (plan->targets[t].agg == MI355Q_PROJECT_KEY) {
        if (sf >= 0) ps.slot_src[sf] = -(1 + q.target_key_idx[t]);
        continue;
      }
      const int st = q2.target_slot[t2++];
      const int ns = plan->targets[t].agg == MI355Q_AVG ? 2 : 1;
      for (int j = 0; j < ns; ++j) {
        if (sf < 0 || st < 0 || q2.init_vals[st + j] != q.init_vals[sf + j]) return kNotTaken;
        ps.slot_src[sf + j] = st + j;
      }
    }
  }

  if (reserved) {  // RESERVE / explain: the derived single-key step over all fragments (one pass), nothing launched
    route_note(ps.raw_f32 ? "k_pack_keys (FLOAT key widened)" : ps.mode == 0 ? "k_pack_keys (bit-packed key)" : ps.mode == 1 ? "k_pack_keys (entry index, baseline temp)"
                                                                             : "k_pack_keys (entry index, perfect temp)");
    std::vector<const void*> cols2((size_t)nf * nc2, nullptr);
    for (int i = 0; i < nf; ++i)
      for (int c = 0; c < nc; ++c)
        if (c != pk) cols2[(size_t)i * nc2 + c] = in->col_buffers[(size_t)i * nc + c];
    mi355q_inputs in2 = *in;
    in2.col_buffers = cols2.data();
    mi355q_exec_options o2 = o;
    o2.out_buffer = nullptr;
    const int32_t e2 = execute_impl(&p2, &in2, &o2, out, report, nullptr, reserved);
    if (e2 == MI355Q_OK) route_note(ps.mode == 2 ? "k_unpack_perfect" : "k_unpack_emit");
    return e2;
  }
  // (this route keeps a pass loop of its own, and uses RouteScope and the result handle only: its passes land in two raw
  // tables of the `aux` workspace that launch_reduce folds, a pass-size override that only ever shrinks the pass, and a pass
  // too small for the padding gives the route up — none of which PassLoop has a knob for)
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  DeviceCtx& ctx = rs.ctx;
  hipStream_t s = rs.s;
  // memory: two temporary tables + the packed column of one pass (a group of fragments)
  const int64_t tmp_bytes = (q2.entry_count * (int64_t)q2.row_size + 255) & ~255ll;
  int64_t pass_rows = pass_budget(ctx.aux.bytes) / 8;
  if (o.pass_rows > 0 && o.pass_rows < pass_rows)  // tests: force several passes
    pass_rows = std::max<int64_t>(o.pass_rows, max_frag_rows);
  if (pass_rows < max_frag_rows + 2 * (int64_t)nf) return kNotTaken;
  if (pass_rows > total_rows) pass_rows = total_rows;
  const int64_t pack_bytes = ((pass_rows + 2 * (int64_t)nf) * 8 + 255) & ~255ll;
  const int64_t tab_bytes = sizeof(void*) * (size_t)nf;
  const int64_t need = pack_bytes + 2 * tmp_bytes + ((tab_bytes + 255) & ~255ll) + 256;
  if (ctx.aux.grow(need) != hipSuccess) {
    (void)hipGetLastError();
    return kNotTaken;
  }
  char* aux = (char*)ctx.aux.p;
  int64_t* packed = (int64_t*)aux;
  int64_t* tmp_a = (int64_t*)(aux + pack_bytes);
  int64_t* tmp_b = (int64_t*)(aux + pack_bytes + tmp_bytes);
  int64_t** d_packed_tab = (int64_t**)(aux + pack_bytes + 2 * tmp_bytes);
  int32_t* d_err = (int32_t*)(aux + pack_bytes + 2 * tmp_bytes + ((tab_bytes + 255) & ~255ll));

  mi355q_result* res_raw = nullptr;
  if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &res_raw)) return e;
  ResultPtr res(res_raw);
  // device copy of the caller's column table (the pack kernel reads the key columns from it)
  DevWord d_tab, d_rows;
  HIP_TRY(hipMalloc(&d_tab.p, sizeof(void*) * (size_t)std::max(1, nf * nc)));
  HIP_TRY(hipMalloc(&d_rows.p, sizeof(int64_t) * (size_t)std::max(1, nf)));
  HIP_TRY(hipMemcpyAsync(d_tab.p, in->col_buffers, sizeof(void*) * (size_t)(nf * nc), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_rows.p, in->num_rows, sizeof(int64_t) * (size_t)nf, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_err, 0, 64, s));

  if (int32_t e = rs.begin_timing(report)) return e;

  std::vector<const void*> cols2((size_t)nf * nc2);
  std::vector<int64_t*> h_packed((size_t)nf);
  mi355q_exec_report acc{};
  int pass = 0;
  int f = 0;
  while (f < nf) {
    int f1 = f;
    int64_t rows = 0, off = 0;
    while (f1 < nf && (f1 == f || rows + in->num_rows[f1] <= pass_rows)) {
      h_packed[f1] = packed + off;
      off += (in->num_rows[f1] + 1) & ~(int64_t)1;  // 16-byte aligned fragment chunks
      rows += in->num_rows[f1];
      ++f1;
    }
    const int pnf = f1 - f;
    HIP_TRY(hipMemcpyAsync(d_packed_tab, h_packed.data() + f, sizeof(void*) * (size_t)pnf, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_pack_keys(ps, (const int8_t* const*)d_tab.p + (size_t)f * nc, (const int64_t*)d_rows.p + f, pnf,
                             nc, max_frag_rows, d_packed_tab, d_err, n_cus, s));
    for (int i = 0; i < pnf; ++i) {
      for (int c = 0; c < nc; ++c) cols2[(size_t)i * nc2 + c] = in->col_buffers[(size_t)(f + i) * nc + c];
      cols2[(size_t)i * nc2 + pk] = h_packed[f + i];
    }
    mi355q_inputs in2 = *in;
    in2.n_frags = pnf;
    in2.col_buffers = cols2.data();
    in2.num_rows = in->num_rows + f;
    mi355q_exec_options o2 = o;
    o2.stream = s;
    o2.out_buffer = pass == 0 ? tmp_a : tmp_b;
    mi355q_result* r2 = nullptr;
    mi355q_exec_report rep2{};
    const int32_t e2 = mi355q_execute(&p2, &in2, &o2, &r2, &rep2);
    if (e2 == MI355Q_ERR_OUT_OF_GPU_MEM || e2 == MI355Q_ERR_UNSUPPORTED) return kNotTaken;
    if (e2) return e2;  // incl. < 0: out of slots -> the caller grows the table
    ResultPtr r2_owner(r2);
    if (pass > 0) {
      HIP_TRY(launch_reduce(r2->dplan, q2.idx_target_as_key, tmp_a, tmp_b, q2.entry_count, d_err, s));
    }
    if (pass == 0) {  // the report names the member the first (a full-sized) pass ran
      std::snprintf(acc.kernel_name, sizeof(acc.kernel_name), "%s", rep2.kernel_name);
      acc.variant = rep2.variant;
    }
    acc.kernel_ms += rep2.kernel_ms;
    acc.n_launches += rep2.n_launches;
    acc.spilled_rows += rep2.spilled_rows;
    f = f1;
    ++pass;
  }
  HIP_TRY(launch_init_buffer(res->buf, q.entry_count, make_row_init(q), s));
  if (nf > 0)
    HIP_TRY(launch_unpack_emit(ps, d, tmp_a, q2.entry_count, q2.row_size / 8, q2.key_bytes / 8, res->buf, d_err, s));
  if (int32_t e = rs.finish(report, acc, 0, *plan, *in, total_rows, d_err))
    return e == MI355Q_ERR_UNSUPPORTED ? kNotTaken : e;  // (unsupported: a key outside its declared range)
  *out = res.release();
  return MI355Q_OK;
}

// Grouped steps whose aggregates read SEVERAL value columns, over inputs large enough for the partitioned / packed
// routes: one run per value column through the single-value families, zipped into the final layout
// (kernels_generic.hip k_zip_targets).  kNotTaken when the shape does not call for it.
int32_t execute_multi_value(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                            const mi355q_qmd& q, const DevPlan& d, mi355q_result** out, mi355q_exec_report* report,
                            int64_t* reserved) {
  if (plan->n_group_cols < 1 || plan->join_outer_col >= 0 || q.slot_width != 8 || q.output_columnar || d.col0_key_quirk)
    return kNotTaken;
  // the value columns, in order of first use
  int vcols[MI355Q_MAX_TARGETS], n_v = 0;
  for (int t = 0; t < plan->n_targets; ++t) {
    const mi355q_target& tg = plan->targets[t];
    if (tg.agg == MI355Q_PROJECT_KEY || tg.col < 0) continue;
    if (tg.table != 0 || tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) return kNotTaken;
    bool seen = false;
    for (int k = 0; k < n_v; ++k) seen = seen || vcols[k] == tg.col;
    if (!seen) vcols[n_v++] = tg.col;
  }
  if (n_v < 2 || n_v > 4) return kNotTaken;
  int64_t total_rows = 0;
  for (int f = 0; f < in->n_frags; ++f) total_rows += in->num_rows[f];
  // small inputs: one pass of the row kernel is as good (kernel_variant 2 = "the large-input members", as for the
  // packed route: how the tests reach this route with small tables)
  if (o.kernel_variant != 2 && total_rows < ((int64_t)8 << 20)) return kNotTaken;

  if (reserved) {  // RESERVE / explain: the run over the first value column (every run has the same shape)
    char note[64];
    std::snprintf(note, sizeof(note), "%d runs (one per value column) + k_zip_targets, each", n_v);
    route_note(note);
    mi355q_plan sp = *plan;
    sp.n_targets = 0;
    for (int t = 0; t < plan->n_targets; ++t) {
      const mi355q_target& tg = plan->targets[t];
      if (tg.agg == MI355Q_PROJECT_KEY || tg.col < 0 || tg.col == vcols[0]) sp.targets[sp.n_targets++] = tg;
    }
    mi355q_exec_options o2 = o;
    o2.out_buffer = nullptr;
    return execute_impl(&sp, in, &o2, out, report, nullptr, reserved);
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  Emission em;  // (ahead of the timed span here: the runs below zip into it one by one)
  if (int32_t e = em.create(q, in->device_id, o.out_buffer, s)) return e;
  if (int32_t e = rs.begin_timing(report)) return e;
  mi355q_exec_report acc{};
  for (int k = 0; k < n_v; ++k) {
    // run k: the targets over value column k; run 0 also carries COUNT(*) and the key projections
    mi355q_plan sp = *plan;
    sp.n_targets = 0;
    int orig_of[MI355Q_MAX_TARGETS];
    for (int t = 0; t < plan->n_targets; ++t) {
      const mi355q_target& tg = plan->targets[t];
      const bool valueless = tg.agg == MI355Q_PROJECT_KEY || tg.col < 0;
      if (valueless ? k == 0 : tg.col == vcols[k]) {
        orig_of[sp.n_targets] = t;
        sp.targets[sp.n_targets++] = tg;
      }
    }
    mi355q_exec_options o2 = o;
    o2.stream = s;
    o2.out_buffer = nullptr;
    mi355q_result* r2 = nullptr;
    mi355q_exec_report rep2{};
    if (int32_t e2 = mi355q_execute(&sp, in, &o2, &r2, &rep2)) return e2;
    ResultPtr r2_owner(r2);
    const mi355q_qmd& q2 = r2->qmd;
    if (q2.desc_type != q.desc_type || q2.entry_count != q.entry_count || q2.slot_width != 8 || q2.output_columnar ||
        (q.desc_type == MI355Q_GROUP_BY_BASELINE_HASH && q2.key_width != q.key_width))
      return MI355Q_ERR_UNSUPPORTED;
    int32_t src[MI355Q_MAX_SLOTS], dst[MI355Q_MAX_SLOTS];
    int n = 0;
    for (int t2 = 0; t2 < sp.n_targets; ++t2) {
      const int t = orig_of[t2];
      const int ss = q2.target_slot[t2], sf = q.target_slot[t];
      if ((ss < 0) != (sf < 0)) return MI355Q_ERR_UNSUPPORTED;   // (a projection read from the key columns on both sides)
      if (ss < 0) continue;
      const int ns = plan->targets[t].agg == MI355Q_AVG ? 2 : 1;
      for (int j = 0; j < ns; ++j) {
        if (q2.init_vals[ss + j] != q.init_vals[sf + j]) return MI355Q_ERR_UNSUPPORTED;
        src[n] = ss + j;
        dst[n] = sf + j;
        ++n;
      }
    }
    HIP_TRY(launch_zip_targets(em.res->dplan, r2->dplan, q2.idx_target_as_key, r2->buf, em.res->buf, src, dst, n, em.d_err(), s));
    HIP_TRY(hipStreamSynchronize(s));   // r2 is freed at the end of this iteration
    if (k == 0) {
      std::snprintf(acc.kernel_name, sizeof(acc.kernel_name), "%s", rep2.kernel_name);
      acc.variant = rep2.variant;
    }
    acc.kernel_ms += rep2.kernel_ms;
    acc.n_launches += rep2.n_launches;
    acc.spilled_rows += rep2.spilled_rows;
  }
  if (int32_t e = rs.finish(report, acc, 0, *plan, *in, total_rows, em.d_err())) return e;
  *out = em.res.release();
  return MI355Q_OK;
}

// Grouped steps over fact JOIN dim (SURVEY f2 + GROUP BY: `SELECT f.g, SUM(d.w), COUNT(*) FROM f JOIN d ON f.k = d.k GROUP BY
// f.g`) with a ONE-TO-ONE join table over a large outer input.  In the row kernel every row probes the table AND updates its
// group with device atomics; here the probe is its own pass (k_join_gather): per outer row, the inner columns the aggregates
// read become dense temporary OUTER columns — the column's NULL where the row has no match — plus, for INNER joins, a 0 / 1
// "matched" column the derived step filters on.  The derived plan has no join, the same targets over those columns and the
// SAME layout (asserted: the descriptor of the derived plan must equal the stated one bit for bit), so its result is the
// step's result and every grouped family applies (LDS members, the partitioned families).  One-to-many tables change the
// row multiplicity: execute_join_expand below.  kNotTaken when the shape does not call for it.
int32_t execute_join_gather(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                            const DevPlan& d, int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  // a plan with inner references (execute_inner_refs) has no row-kernel alternative: every input size, non-grouped aggregate
  // steps and forced variants too; `q` is its flattened plan's descriptor, `d` carries the join alone
  const bool refs = has_inner_refs(*plan);
  if (plan->join_outer_col < 0 || plan->n_exprs != 0 || (d.join_hash_type != 0 && d.join_hash_type != 1)) return kNotTaken;
  if (!refs && (plan->n_group_cols < 1 || o.kernel_variant == 1 || o.force_generic || q.desc_type == MI355Q_NON_GROUPED_AGGREGATE))
    return kNotTaken;
  const int nc = plan->n_cols, nf = in->n_frags;
  const bool inner_join = plan->join_kind != MI355Q_JOIN_LEFT;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (frag_row_totals(*in, &total_rows, &max_frag_rows)) return kNotTaken;  // (a negative count: the plain step's to refuse)
  // (kernel_variant 2 = "the large-input members": how the tests reach this route with small tables)
  if (nf < 1 || (!refs && o.kernel_variant != 2 && total_rows < kIdxPartMinRows)) return kNotTaken;
  // a perfect-hash table of <= 64 KB is aggregated by the row kernel in a per-workgroup LDS copy (launch_generic): probe and
  // update in one pass, nothing gained by splitting them — measured at 1 B rows, 100 groups: 49 ms there, 57 ms here; 10 000
  // groups (global atomics there): 470 / 163 ms there (LEFT / INNER), 69 / 64 ms here (profiles/r04_grouped_join_1b_call16/17.jsonl)
  if (!refs && o.kernel_variant != 2 && q.desc_type == MI355Q_GROUP_BY_PERFECT_HASH && q.entry_count * (int64_t)q.row_size <= 64 * 1024)
    return kNotTaken;
  // the inner columns the plan reads as outer columns behind the stated ones (+ the matched flag): plan.cpp flatten_inner_refs
  mi355q_plan p2;
  InnerFlat fl;
  if (int32_t e = flatten_inner_refs(*plan, true, &p2, &fl)) return refs ? e : kNotTaken;
  const int n_used = fl.n_inner, flag_col = fl.flag_col, nc2 = p2.n_cols;
  const int32_t* used = fl.inner_col;
  int32_t dst[MI355Q_MAX_COLS], width[MI355Q_MAX_COLS];
  int64_t null_pat[MI355Q_MAX_COLS];
  for (int j = 0; j < n_used; ++j) {
    const mi355q_col_desc& cd = plan->inner_cols[used[j]];
    dst[j] = nc + j;
    width[j] = plain_width(cd.type);
    null_pat[j] = cd.type == MI355Q_DOUBLE ? kNullDoubleBits
                  : cd.type == MI355Q_FLOAT ? (int64_t)(uint32_t)kNullFloatBits : plain_int_null(cd.type);
  }
  mi355q_qmd q2;
  if (qmd_init(p2, &q2) != MI355Q_OK || std::memcmp(&q, &q2, sizeof(q)) != 0) return kNotTaken;  // the same layout, or not this way
  if (reserved) {
    route_note(refs ? "inner columns flattened: k_join_gather (inner columns + matched flag as outer columns)"
                    : "k_join_gather (inner columns + matched flag as outer columns)");
    // the derived step's shape: the same fragments with nc2 columns (the pointers are not looked at in reserve mode)
    std::vector<const void*> fake((size_t)nf * nc2, nullptr);
    mi355q_inputs in2 = *in;
    in2.col_buffers = fake.data();
    in2.inner_col_buffers = nullptr;
    return execute_impl(&p2, &in2, &o, out, report, nullptr, reserved);
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  if (inner_join) width[n_used] = 4;  // (the matched flag, behind the gathered columns)
  mi355q_inputs in_outer = *in;       // the derived step has no inner side
  in_outer.inner_col_buffers = nullptr;
  PassLoop pl(rs.ctx.gather, nc, nc2 - nc, width, &p2);
  pl.clear_err_word = false;
  if (int32_t e = pl.prepare(&in_outer, o, total_rows, max_frag_rows)) return e;
  if (int32_t e = pl.run(rs, &in_outer, o, report, [&](int f, int pnf) -> int32_t {
        HIP_TRY(launch_join_gather(d, n_used, used, dst, width, null_pat, flag_col, nc2, pl.d_tab, pl.d_rows + f, pnf, max_frag_rows,
                                   n_cus, s));
        HIP_TRY(hipStreamSynchronize(s));  // (cols2 is re-used by the next pass; the step below synchronises anyway)
        return MI355Q_OK;
      }))
    return e;
  if (int32_t e = rs.finish(report, pl.acc, 0, *plan, *in, total_rows)) return e;
  *out = pl.res.release();
  return MI355Q_OK;
}

// The same steps over a ONE-TO-MANY join table ("real fact JOIN dim workloads have duplicates").  The reference's join
// loop encloses the row function's body, so the step over fact JOIN dim IS the stated step, without the join, over the joined
// rows: k_join_expand_count / _scan count them per tile and fragment, k_join_expand_write lays them down as dense temporary
// columns — the outer columns the derived plan reads copied as stored (every encoding survives: the derived plan keeps the
// descriptors), the inner columns gathered through the payload, NULL for an unmatched LEFT row — and outer fragment f becomes
// one derived fragment of rows2[f] rows, in (outer row, payload) order.  The quals stay in the derived plan: they read outer
// columns only and hold per joined row (rows they drop are expanded and dropped by the derived step; constrained_not_null
// is part of the layout anyway); an INNER join needs no "matched" column, its unmatched rows have no joined row.  The derived
// plan has the SAME layout (asserted bit for bit), so every grouped family applies.  kNotTaken when the shape does not call
// for it.
int32_t execute_join_expand(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                            const DevPlan& d, int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  // (a plan with inner references: as in execute_join_gather — the route at every size, whatever the options say)
  const bool refs = has_inner_refs(*plan);
  if (plan->join_outer_col < 0 || plan->n_exprs != 0 || (d.join_hash_type != 2 && d.join_hash_type != 3)) return kNotTaken;
  if (!refs && (plan->n_group_cols < 1 || o.kernel_variant == 1 || o.force_generic || (o.flags & MI355Q_OPT_NO_JOIN_EXPAND) ||
                q.desc_type == MI355Q_NON_GROUPED_AGGREGATE))
    return kNotTaken;
  const int nc = plan->n_cols, nf = in->n_frags;
  const bool left = plan->join_kind == MI355Q_JOIN_LEFT;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (frag_row_totals(*in, &total_rows, &max_frag_rows)) return kNotTaken;  // (a negative count: the plain step's to refuse)
  // Both thresholds are the gather route's ROUTING CONSTANTS, not crossovers measured for this route: the input size from
  // which the large-input families are planned at all, and the perfect-hash table the row kernel aggregates in a
  // per-workgroup LDS copy (launch_generic).  (kernel_variant 2 = "the large-input members": how the tests reach this route
  // with small tables)
  if (nf < 1 || (!refs && o.kernel_variant != 2 && total_rows < kIdxPartMinRows)) return kNotTaken;
  if (!refs && o.kernel_variant != 2 && q.desc_type == MI355Q_GROUP_BY_PERFECT_HASH && q.entry_count * (int64_t)q.row_size <= 64 * 1024)
    return kNotTaken;
  // the inner columns the plan reads: plain columns, appended behind the stated ones (plan.cpp flatten_inner_refs; no
  // matched flag: an unmatched row of an INNER join has no joined row)
  JoinExpand je{};
  int32_t width[MI355Q_MAX_COLS];
  mi355q_plan p2;
  InnerFlat fl;
  if (int32_t e = flatten_inner_refs(*plan, false, &p2, &fl)) return refs ? e : kNotTaken;
  je.n_inner = fl.n_inner;
  for (int j = 0; j < fl.n_inner; ++j) {
    const mi355q_col_desc& cd = plan->inner_cols[fl.inner_col[j]];
    je.inner_col[j] = fl.inner_col[j];
    je.inner_dst[j] = nc + j;
    je.inner_w[j] = width[j] = plain_width(cd.type);
    je.null_pat[j] = cd.type == MI355Q_DOUBLE ? kNullDoubleBits
                     : cd.type == MI355Q_FLOAT ? (int64_t)(uint32_t)kNullFloatBits : plain_int_null(cd.type);
  }
  const int nc2 = p2.n_cols;
  mi355q_qmd q2;
  if (qmd_init(p2, &q2) != MI355Q_OK || std::memcmp(&q, &q2, sizeof(q)) != 0) return kNotTaken;  // the same layout, or not this way
  if (reserved) {
    // nothing is launched, so no count exists: the derived step over the OUTER fragments' shape (the pointers are not looked at)
    route_note(refs ? "inner columns flattened: k_join_expand (joined rows as dense columns)" : "k_join_expand (joined rows as dense columns)");
    std::vector<const void*> fake((size_t)nf * nc2, nullptr);
    mi355q_inputs in2 = *in;
    in2.col_buffers = fake.data();
    in2.inner_col_buffers = nullptr;
    return execute_impl(&p2, &in2, &o, out, report, nullptr, reserved);
  }
  // the stated columns the derived plan reads: expanded as stored.  The others (the join key, usually) are not.
  int32_t tmp_width[MI355Q_MAX_COLS] = {};
  {
    bool read[MI355Q_MAX_COLS] = {};
    const auto reads = [&](int c) { if (c >= 0 && c < nc) read[c] = true; };
    for (int g = 0; g < plan->n_group_cols; ++g) reads(plan->group_cols[g]);
    for (int t = 0; t < plan->n_targets; ++t) {
      const mi355q_target& tg = p2.targets[t];
      if (tg.agg != MI355Q_PROJECT_KEY && tg.table == 0) reads(tg.col);
      if (tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) reads(tg.cond.col);
    }
    for (int k = 0; k < plan->n_quals; ++k) reads(plan->quals[k].col);
    for (int c = 0; c < nc; ++c) {
      if (!read[c]) continue;
      const int code = col_type_code(plan->cols[c]);
      if (code < 0) return kNotTaken;
      je.outer_col[je.n_outer] = c;
      je.outer_w[je.n_outer++] = tmp_width[c] = type_width(code);
    }
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  // ---- count and scan, once over all fragments: the tiles' and the fragments' joined rows
  const int64_t tile_rows = projection_tile_rows();
  std::vector<int64_t> h_meta((size_t)2 * nf + 1);  // tile_start [nf + 1] | num_rows [nf]
  bool key_aligned = true;
  for (int f = 0; f < nf; ++f) {
    h_meta[f + 1] = h_meta[f] + (in->num_rows[f] + tile_rows - 1) / tile_rows;
    h_meta[(size_t)nf + 1 + f] = in->num_rows[f];
    key_aligned = key_aligned && ((uintptr_t)in->col_buffers[(size_t)f * nc + d.join_cols[0]] & 15) == 0;
  }
  const int64_t n_tiles = h_meta[nf];
  const int64_t meta_bytes = (((int64_t)h_meta.size() * 8) + 255) & ~255ll, tab_bytes = ((int64_t)sizeof(void*) * nf * nc + 255) & ~255ll;
  const int64_t tiles_bytes = (n_tiles * 8 + 255) & ~255ll, frags_bytes = ((int64_t)nf * 8 + 255) & ~255ll;
  DevWord area;  // tile_start | num_rows | the stated columns' table | tile_cnt | tile_base | frag_first | frag_rows
  if (hipMalloc(&area.p, (size_t)(meta_bytes + tab_bytes + 2 * tiles_bytes + 2 * frags_bytes)) != hipSuccess) {
    (void)hipGetLastError();
    return kNotTaken;
  }
  char* ap = (char*)area.p;
  je.tile_start = (const int64_t*)ap;
  je.num_rows = je.tile_start + nf + 1;
  je.src = (const int8_t* const*)(ap + meta_bytes);
  je.tile_cnt = (unsigned long long*)(ap + meta_bytes + tab_bytes);
  je.tile_base = (unsigned long long*)(ap + meta_bytes + tab_bytes + tiles_bytes);
  je.frag_first = (unsigned long long*)(ap + meta_bytes + tab_bytes + 2 * tiles_bytes);
  je.frag_rows = (unsigned long long*)(ap + meta_bytes + tab_bytes + 2 * tiles_bytes + frags_bytes);
  je.n_frags = nf;
  je.nc = nc;
  je.nc2 = nc2;
  je.n_tiles = n_tiles;
  je.left = left;
  je.quad_key = d.join_n_keys == 1 && key_aligned && (d.join_types[0] == MI355Q_INT32 || d.join_types[0] == MI355Q_INT64)
                    ? type_width(d.join_types[0]) : 0;
  HIP_TRY(hipMemcpyAsync(ap, h_meta.data(), h_meta.size() * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ap + meta_bytes, in->col_buffers, sizeof(void*) * (size_t)nf * nc, hipMemcpyHostToDevice, s));
  if (int32_t e = rs.begin_timing(report)) return e;
  HIP_TRY(launch_join_expand_count(d, je, n_cus, s));
  std::vector<int64_t> rows2((size_t)nf);
  HIP_TRY(hipMemcpyAsync(rows2.data(), je.frag_rows, sizeof(int64_t) * (size_t)nf, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // the one synchronisation the sizes cost
  int64_t total2 = 0, max_rows2 = 0;
  for (int f = 0; f < nf; ++f) {
    if (rows2[f] < 0 || rows2[f] >= ((int64_t)1 << 31)) return kNotTaken;
    total2 += rows2[f];
    max_rows2 = std::max(max_rows2, rows2[f]);
  }
  mi355q_inputs in_outer = *in;  // the derived step has no inner side
  in_outer.inner_col_buffers = nullptr;
  if (total2 == 0) {
    // nothing joins at all: the derived step once over one fragment without rows, for the stated, initialised layout
    // (a family that refuses such a step gives the route up)
    if (rs.ctx.gather.grow(256) != hipSuccess) {
      (void)hipGetLastError();
      return kNotTaken;
    }
    std::vector<const void*> cols0((size_t)nc2, rs.ctx.gather.p);
    const int64_t no_rows = 0;
    in_outer.n_frags = 1;
    in_outer.col_buffers = cols0.data();
    in_outer.num_rows = &no_rows;
    mi355q_exec_options o2 = o;
    o2.stream = s;
    mi355q_result* r2 = nullptr;
    mi355q_exec_report acc{};
    if (mi355q_execute(&p2, &in_outer, &o2, &r2, &acc)) return kNotTaken;
    ResultPtr res(r2);
    if (int32_t e = rs.finish(report, acc, 2, *plan, *in, total_rows)) return e;
    *out = res.release();
    return MI355Q_OK;
  }
  PassLoop pl(rs.ctx.gather, nc, je.n_inner, width, &p2);
  pl.clear_err_word = false;
  pl.derived_rows = rows2.data();
  pl.stated_tmp_width = tmp_width;
  if (int32_t e = pl.prepare(&in_outer, o, total2, max_rows2)) return e;
  if (int32_t e = pl.run(rs, &in_outer, o, report, [&](int f, int pnf) -> int32_t {
        je.frag0 = f;
        je.n_pass_frags = pnf;
        je.pass_tile0 = h_meta[f];
        je.pass_tiles = h_meta[f + pnf] - h_meta[f];
        je.dst = (int8_t* const*)pl.d_tab;
        HIP_TRY(launch_join_expand_write(d, je, n_cus, s));
        HIP_TRY(hipStreamSynchronize(s));  // (cols2 is re-used by the next pass; the step below synchronises anyway)
        return MI355Q_OK;
      }))
    return e;
  if (int32_t e = rs.finish(report, pl.acc, 2, *plan, *in, total_rows)) return e;  // (+ 2: count and scan)
  *out = pl.res.release();
  return MI355Q_OK;
}

// The star member behind execute_inner_refs: few groups keyed by dimension attributes, a one-to-one perfect join table over one
// INT32 / INT64 key (lds_args.h make_star_args states the rest).  k_join_group_code maps every join-table slot to its group's
// entry — a dimension-sized pass, once per step, the map is not kept with the join table — and k_star_groupby_lds aggregates the
// fact rows through it: no temporary column.  By default for maps up to kStarDefaultMapBytes16 / 32; kernel_variant 2 takes it at
// every map size, MI355Q_OPT_NO_STAR_GROUPBY never.  kNotTaken: the flattened route runs the step.
int32_t execute_star_groupby(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                             const DevPlan& d, int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  if ((o.flags & MI355Q_OPT_NO_STAR_GROUPBY) || o.force_generic || o.kernel_variant == 1 || in->n_frags < 1 || d.join_hash_type != 0 ||
      d.join_n_keys != 1 || q.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || q.output_columnar || q.slot_width != 8 ||
      plan->n_group_cols < 1 || !d.join_buf || d.join_max < d.join_min || d.join_max - d.join_min + 1 != d.join_entries)
    return kNotTaken;
  for (int g = 0; g < plan->n_group_cols; ++g)
    if (!MI355Q_IS_INNER_COL(plan->group_cols[g])) return kNotTaken;
  for (int t = 0; t < plan->n_targets; ++t)
    if (plan->targets[t].agg != MI355Q_PROJECT_KEY && plan->targets[t].table != 0) return kNotTaken;
  StarStep st{};
  mi355q_plan fp;
  InnerFlat fl;
  if (flatten_inner_refs(*plan, false, &fp, &fl) != MI355Q_OK) return kNotTaken;
  if (build_dev_plan(fp, q, &st.flat) != MI355Q_OK) return kNotTaken;  // (the stated layout over the flattened plan's columns)
  st.nc = plan->n_cols;
  st.n_inner = fl.n_inner;
  st.left = plan->join_kind == MI355Q_JOIN_LEFT;
  st.key_col = d.join_cols[0];
  const mi355q_col_desc& kd = plan->cols[st.key_col];
  if (kd.encoding != MI355Q_ENC_NONE || (kd.logical_type != 0 && kd.logical_type != kd.type)) return kNotTaken;
  st.key_type = kd.type;
  st.key_nullable = kd.nullable != 0;
  for (int j = 0; j < fl.n_inner; ++j) {
    st.inner_col[j] = fl.inner_col[j];
    st.inner_type[j] = plan->inner_cols[fl.inner_col[j]].type;
    st.inner_base[j] = d.inner_cols[fl.inner_col[j]];
    if (!reserved && !st.inner_base[j]) return kNotTaken;
  }
  st.inner_rows = in->inner_num_rows;
  st.table = (const int32_t*)d.join_buf;
  st.key_min = d.join_min;
  st.n_slots = d.join_entries;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (frag_row_totals(*in, &total_rows, &max_frag_rows)) return kNotTaken;
  FragView fv{nullptr, nullptr, in->col_buffers, in->num_rows, in->n_frags, plan->n_cols, total_rows, max_frag_rows};
  int64_t map_bytes = 0;
  if (!star_groupby_eligible(st, fv, n_cus, &map_bytes)) return kNotTaken;
  // the default per (code width, map size) class, as measured (lds_args.h); beyond it: kernel_variant 2
  if (o.kernel_variant != 2 && map_bytes > (q.entry_count <= 32767 ? kStarDefaultMapBytes16 : kStarDefaultMapBytes32)) return kNotTaken;
  if (reserved) {
    route_note("k_join_group_code + k_star_groupby_lds");
    *reserved = 0;
    return MI355Q_OK;
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  if (const hipError_t he = rs.ctx.star.grow(map_bytes)) {
    last_hip_error = he;
    (void)hipGetLastError();
    return kNotTaken;  // (the flattened route sizes its passes from what is free)
  }
  mi355q_result* res = nullptr;
  if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &res)) return e;
  ResultPtr owned(res);
  FragTable ft;
  if (int32_t e = upload_frag_table(rs.ctx, *in, plan->n_cols, s, FragUpload::kAlways, &ft)) return e;
  UploadGuard upload_guard{s, true};
  fv.d_cols = ft.d_cols;
  fv.d_num_rows = ft.d_rows;
  if (int32_t e = rs.begin_timing(report)) return e;
  HIP_TRY(launch_init_buffer(res->buf, q.entry_count, make_row_init(q), s));
  LaunchStats ls;
  HIP_TRY(launch_star_groupby(st, fv, rs.ctx.star.p, res->buf, ft.d_err, n_cus, s, &ls));
  mi355q_exec_report acc{};
  std::snprintf(acc.kernel_name, sizeof(acc.kernel_name), "%s", ls.kernel_name);
  acc.variant = ls.variant;
  acc.n_launches = ls.n_launches;
  if (int32_t e = rs.finish(report, acc, 0, *plan, *in, total_rows, ft.d_err)) return e;  // (synchronises: the upload has landed)
  upload_guard.armed = false;
  if (report) report->kernel_ms = report->total_ms;  // (map + scan: the step has no other launch)
  *out = owned.release();
  return MI355Q_OK;
}

// Star joins: a join step whose quals / group columns name INNER columns (MI355Q_INNER_COL, include/mi355q.h:
// `SELECT d.region, COUNT(*), SUM(f.amount) FROM fact f JOIN dim d ON f.did = d.id WHERE d.segment BETWEEN 2 AND 5 GROUP BY
// d.region`).  The step means what its flattened plan (plan.cpp flatten_inner_refs) means over the joined rows, and that is
// how it runs: k_join_gather (one-to-one tables) or k_join_expand (one-to-many) lay the inner columns down as dense outer
// columns and the flattened, joinless plan runs over them — at every input size and for non-grouped aggregates too, there
// being no row-kernel alternative.  Asked ahead of every other route; never kNotTaken.  The star member
// (execute_star_groupby above) is asked first.
int32_t execute_inner_refs(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                           mi355q_exec_report* report, int64_t* reserved) {
  mi355q_plan flat;
  InnerFlat fl;
  if (int32_t e = flatten_inner_refs(*plan, true, &flat, &fl)) return e;
  mi355q_qmd q;
  if (int32_t e = qmd_init(flat, &q)) return e;
  // the layout twins first, as in execute_impl: they run the same plan with another hint and come back here
  if (q.output_columnar) return execute_columnar_twin(plan, in, o, q, out, report, reserved);
  if (q.slot_width == 4) return execute_wide_slot_twin(plan, in, o, q, out, report, reserved);
  // the join as the device sees it: a carrier plan that keeps the stated columns and the join and nothing else
  mi355q_plan cp = *plan;
  cp.n_quals = 0;
  cp.n_group_cols = 0;
  cp.n_targets = 1;
  cp.targets[0] = mi355q_target{};
  cp.targets[0].agg = MI355Q_COUNT;
  cp.targets[0].col = -1;
  cp.output_columnar_hint = MI355Q_OUTPUT_ROWWISE;
  mi355q_qmd cq;
  if (int32_t e = qmd_init(cp, &cq)) return e;
  DevPlan d;
  if (int32_t e = build_dev_plan(cp, cq, &d)) return e;
  if (int32_t e = attach_join(cp, in, &d)) return e;
  for (int j = 0; j < fl.n_inner; ++j)
    if (!reserved && !d.inner_cols[fl.inner_col[j]] && in->inner_num_rows > 0) return MI355Q_ERR_INVALID_PLAN;
  int n_cus = 0;
  {
    DeviceGuard g(in->device_id);
    if (!g.ok) return MI355Q_ERR_HIP;
    n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);
  }
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  if (total_rows == 0) {  // nothing to join: the flattened plan over no fragments, for the stated, initialised layout
    mi355q_inputs in0 = *in;
    in0.n_frags = 0;
    in0.inner_col_buffers = nullptr;
    return execute_impl(&flat, &in0, &o, out, report, nullptr, reserved);
  }
  const bool one_to_one = d.join_hash_type == 0 || d.join_hash_type == 1;
  if (const int32_t es = try_route(out, [&] { return execute_star_groupby(plan, in, o, q, d, n_cus, out, report, reserved); }); es != kNotTaken)
    return es;
  const int32_t e = one_to_one ? execute_join_gather(plan, in, o, q, d, n_cus, out, report, reserved)
                               : execute_join_expand(plan, in, o, q, d, n_cus, out, report, reserved);
  return e == kNotTaken ? MI355Q_ERR_UNSUPPORTED : e;
}

// Baseline steps over 2 - 3 plain INT key columns that all have ranges — the reference's PerfectHashMultiCol / MultiStep
// shapes beyond g_baseline_groupby_threshold (PHM006, MSPHM005, MSPHM007: ~11 M combinations, Execute.cpp:113,
// GroupByAndAggregate.cpp:232-365) — over a large input: the product of the ranges still indexes a table the
// index-partitioned family (kernels_idx.hip) aggregates in one exchange, so the step runs on a library-owned PERFECT
// twin of the layout and its live entries are re-keyed into the baseline table of the stated plan
// (kernels_generic.hip k_perfect_twin_emit).  kNotTaken when the shape does not call for it.
constexpr int64_t kTwinMaxEntries = (int64_t)32 << 20;
int32_t execute_perfect_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                             int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  if (q.desc_type != MI355Q_GROUP_BY_BASELINE_HASH || plan->n_group_cols < 2 || plan->n_group_cols > 3 ||
      plan->join_outer_col >= 0 || plan->n_exprs != 0 || q.slot_width != 8 || q.output_columnar ||
      plan->output_columnar_hint != 0 || o.kernel_variant == 1 || o.force_generic)
    return kNotTaken;
  __int128 card = 1;
  int32_t translate[MI355Q_MAX_GROUP_COLS], key_type[MI355Q_MAX_GROUP_COLS];
  for (int g = 0; g < plan->n_group_cols; ++g) {
    const int c = plan->group_cols[g];
    if (c < 0 || c >= plan->n_cols) return kNotTaken;
    const mi355q_col_desc& cd = plan->cols[c];
    const mi355q_range& r = plan->col_ranges[c];
    if (cd.type != MI355Q_INT32 || cd.encoding != MI355Q_ENC_NONE || (cd.logical_type != 0 && cd.logical_type != cd.type) ||
        !r.valid || r.bucket != 0 || r.min > r.max || (r.has_nulls && !cd.nullable))
      return kNotTaken;
    card *= (__int128)r.max - (__int128)r.min + 1 + (r.has_nulls ? 1 : 0);
    if (card > (__int128)kTwinMaxEntries) return kNotTaken;
    translate[g] = cd.nullable && r.has_nulls;  // (build_dev_plan's rule for several key columns)
    key_type[g] = col_type_code(cd);
  }
  int64_t total_rows = 0, max_rows = 0;
  for (int f = 0; f < in->n_frags; ++f) {
    total_rows += in->num_rows[f];
    max_rows = std::max(max_rows, in->num_rows[f]);
  }
  // (kernel_variant 2 = "the large-input members": how the tests reach this route with small tables)
  if (o.kernel_variant != 2 && total_rows < kIdxPartMinRows) return kNotTaken;
  PerfectTwinScope twin(kTwinMaxEntries);
  mi355q_qmd q2;
  if (qmd_init(*plan, &q2) != MI355Q_OK) return kNotTaken;
  if (q2.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || q2.slot_width != 8 || q2.output_columnar ||
      q2.entry_count * (int64_t)q2.row_size > ((int64_t)4 << 30))
    return kNotTaken;
  DevPlan d2;
  if (build_dev_plan(*plan, q2, &d2) != MI355Q_OK) return kNotTaken;
  {
    FragView fvh{nullptr, nullptr, in->col_buffers, in->num_rows, in->n_frags, plan->n_cols, total_rows, max_rows};
    if (!idx_part_eligible(d2, fvh, n_cus)) return kNotTaken;
  }
  for (int t = 0; t < plan->n_targets; ++t) {
    const int sf = q.target_slot[t], ss = q2.target_slot[t];
    if (plan->targets[t].agg == MI355Q_PROJECT_KEY) {
      if (sf >= 0) return kNotTaken;  // (baseline: projections are read from the key columns)
      continue;
    }
    if (sf < 0 || ss < 0) return kNotTaken;
    for (int j = 0; j < (plan->targets[t].agg == MI355Q_AVG ? 2 : 1); ++j)
      if (q.init_vals[sf + j] != q2.init_vals[ss + j]) return kNotTaken;
  }
  mi355q_exec_options o2 = o;
  o2.out_buffer = nullptr;
  if (reserved) {
    route_note("perfect-hash twin + k_perfect_twin_emit");
    return execute_impl(plan, in, &o2, out, report, nullptr, reserved);
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  if (int32_t e = rs.begin_timing(report)) return e;
  o2.stream = s;
  mi355q_result* r2 = nullptr;
  mi355q_exec_report rep2{};
  if (int32_t e2 = mi355q_execute(plan, in, &o2, &r2, &rep2)) {
    if (e2 == MI355Q_ERR_UNSUPPORTED || e2 == MI355Q_ERR_OUT_OF_GPU_MEM || e2 < 0) return kNotTaken;
    return e2;
  }
  ResultPtr r2_owner(r2);
  if (r2->qmd.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || r2->qmd.slot_width != 8 || r2->qmd.output_columnar ||
      r2->qmd.entry_count != q2.entry_count)
    return kNotTaken;
  Emission em;
  if (int32_t e = em.create(q, in->device_id, o.out_buffer, s)) return e;
  HIP_TRY(launch_perfect_twin_emit(em.res->dplan, r2->dplan, r2->qmd.idx_target_as_key, plan->n_group_cols, translate, key_type,
                                   q2.group_min, q2.group_card, q2.group_null_key, r2->buf, em.res->buf, em.d_err(), s));
  if (int32_t e = rs.finish(report, rep2, 1, *plan, *in, total_rows, em.d_err())) return e;
  *out = em.res.release();
  return MI355Q_OK;
}

// Baseline steps whose key columns lie on a LATTICE — key = min + stride x i — with few lattice points: the reference
// benchmark's BIGINT columns x10k_s10k / x100k_s10k / x1m_s10k (multiples of 10 000: BaselineHash/BH007-010,
// MultiStep/MSBS006-007).  Their RANGE is far too wide for a perfect hash (GroupByAndAggregate.cpp:232-365 sees max - min),
// so the reference — and the plain route here — hash 8-byte keys.  The stride is found on the first fragment (k_key_gcd), every
// row's key is then rewritten as its lattice index i in a dense INT32 column and CHECKED (k_affine_keys: a key off the
// lattice or outside the range gives the route up, nothing is assumed about the data), the step runs grouped by those
// columns on a library-owned perfect-hash twin (typed LDS members / the index-partitioned family: ONE exchange of 8- or
// 16-byte records instead of 16-byte records per value column), and k_affine_twin_emit re-keys the twin's entries into the
// baseline table of the stated plan.  mi355q_explain cannot see the data and names the plain route for these shapes.
int32_t execute_affine_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                            int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  if (reserved || q.desc_type != MI355Q_GROUP_BY_BASELINE_HASH || plan->n_group_cols < 1 || plan->n_group_cols > 3 ||
      plan->join_outer_col >= 0 || plan->n_exprs != 0 || q.slot_width != 8 || q.output_columnar ||
      plan->output_columnar_hint != 0 || o.kernel_variant == 1 || o.force_generic)
    return kNotTaken;
  const int nc = plan->n_cols, nf = in->n_frags, ng = plan->n_group_cols;
  int64_t total_rows = 0, max_frag_rows = 0;
  int first = -1;
  for (int f = 0; f < nf; ++f) {
    if (in->num_rows[f] < 0) return kNotTaken;
    total_rows += in->num_rows[f];
    max_frag_rows = std::max(max_frag_rows, in->num_rows[f]);
    if (first < 0 && in->num_rows[f] > 0) first = f;
  }
  // (kernel_variant 2 = "the large-input members": how the tests reach this route with small tables)
  if (first < 0 || (o.kernel_variant != 2 && total_rows < kIdxPartMinRows)) return kNotTaken;
  bool proj[MI355Q_MAX_GROUP_COLS];
  int n_proj = 0;
  for (int g = 0; g < ng; ++g) {
    const int c = plan->group_cols[g];
    if (c < 0 || c >= nc) return kNotTaken;
    const mi355q_col_desc& cd = plan->cols[c];
    const mi355q_range& r = plan->col_ranges[c];
    if ((cd.type != MI355Q_INT32 && cd.type != MI355Q_INT64) || cd.encoding != MI355Q_ENC_NONE ||
        (cd.logical_type != 0 && cd.logical_type != cd.type) || !r.valid || r.bucket != 0 || r.min > r.max ||
        (r.has_nulls && !cd.nullable))
      return kNotTaken;
    // BIGINT keys, and INT keys over a range too wide for the twin on their own, are looked at for a stride
    proj[g] = cd.type == MI355Q_INT64 || (__int128)r.max - (__int128)r.min >= ((__int128)1 << 20);
    n_proj += proj[g] ? 1 : 0;
  }
  if (n_proj == 0 || nc + n_proj > MI355Q_MAX_COLS) return kNotTaken;
  // only where the twin's step is the typed LDS members' or the index-partitioned family's work (no qual, plain INT value
  // columns: checked here before anything is launched, and on the derived plan below): every other baseline step — the
  // headline's filtered AVG(double) among them — keeps its own family and pays nothing for this route
  // (a compiled filter travelling beside the plan is a qual too: the `rest` plan of execute_bool_filter has n_quals = 0;
  // ADVICE r05)
  if (plan->n_quals != 0 || step_bool_filter()) return kNotTaken;
  for (int t = 0; t < plan->n_targets; ++t) {
    const mi355q_target& tg = plan->targets[t];
    if (tg.agg == MI355Q_PROJECT_KEY || tg.col < 0) continue;
    if (tg.table != 0 || tg.col >= nc || tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) return kNotTaken;
    const mi355q_col_desc& vd = plan->cols[tg.col];
    if (vd.type != MI355Q_INT32 || vd.encoding != MI355Q_ENC_NONE || (vd.logical_type != 0 && vd.logical_type != vd.type)) return kNotTaken;
  }

  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  // ---- the stride of every looked-at key column, from the first non-empty fragment
  // (a sample: the first 4 M rows — the stride it gives is verified on every row below, a coarser lattice only gives the route up)
  constexpr int kGcdBlocks = 256;  // partial strides per column handed to the host
  constexpr int64_t kGcdScratch = 64 * 256;
  DevWord gw;
  HIP_TRY(hipMalloc(&gw.p, sizeof(unsigned long long) * (kGcdScratch + kGcdBlocks * MI355Q_MAX_GROUP_COLS) + 64));
  unsigned long long* g_scr = (unsigned long long*)gw.p;
  unsigned long long* g_out = g_scr + kGcdScratch;
  std::vector<unsigned long long> h_g((size_t)kGcdBlocks * MI355Q_MAX_GROUP_COLS);
  for (int gcol = 0, k = 0; gcol < ng; ++gcol) {
    if (!proj[gcol]) continue;
    const int c = plan->group_cols[gcol];
    HIP_TRY(launch_key_gcd(in->col_buffers[(size_t)first * nc + c], plain_width(plan->cols[c].type),
                           std::min<int64_t>(in->num_rows[first], (int64_t)4 << 20), plan->col_ranges[c].min, plan->cols[c].nullable, g_scr,
                           g_out + (size_t)k * kGcdBlocks, s));
    ++k;
  }
  HIP_TRY(hipMemcpyAsync(h_g.data(), g_out, sizeof(unsigned long long) * kGcdBlocks * n_proj, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // ---- the derived plan
  mi355q_plan p2 = *plan;
  int32_t src_col[MI355Q_MAX_GROUP_COLS], dst_col[MI355Q_MAX_GROUP_COLS], width[MI355Q_MAX_GROUP_COLS], nullable[MI355Q_MAX_GROUP_COLS];
  int64_t kmin[MI355Q_MAX_GROUP_COLS], stride[MI355Q_MAX_GROUP_COLS], card[MI355Q_MAX_GROUP_COLS];
  int64_t base_of[MI355Q_MAX_GROUP_COLS], stride_of[MI355Q_MAX_GROUP_COLS];
  int32_t translate[MI355Q_MAX_GROUP_COLS], key_type[MI355Q_MAX_GROUP_COLS];
  __int128 entries = 1;
  for (int gcol = 0, k = 0; gcol < ng; ++gcol) {
    const int c = plan->group_cols[gcol];
    const mi355q_col_desc& cd = plan->cols[c];
    const mi355q_range& r = plan->col_ranges[c];
    translate[gcol] = cd.nullable && (ng == 1 || r.has_nulls);  // (build_dev_plan's rule for the twin's keys)
    key_type[gcol] = col_type_code(cd);
    base_of[gcol] = r.min;
    stride_of[gcol] = 1;
    __int128 points = (__int128)r.max - (__int128)r.min + 1;
    if (proj[gcol]) {
      unsigned long long gg = 0;
      for (int b = 0; b < kGcdBlocks; ++b) {
        unsigned long long x = h_g[(size_t)k * kGcdBlocks + b], y = gg;
        while (y) {
          const unsigned long long t = x % y;
          x = y;
          y = t;
        }
        gg = x;
      }
      if (gg == 0) gg = 1;  // (every key of the fragment is the minimum, or NULL)
      if (gg > (unsigned long long)INT64_MAX) return kNotTaken;
      points = ((__int128)r.max - (__int128)r.min) / (__int128)gg + 1;
      if (points >= ((__int128)1 << 30)) return kNotTaken;
      stride_of[gcol] = (int64_t)gg;
      src_col[k] = c;
      dst_col[k] = nc + k;
      width[k] = plain_width(cd.type);
      nullable[k] = cd.nullable;
      kmin[k] = r.min;
      stride[k] = (int64_t)gg;
      card[k] = (int64_t)points;
      p2.cols[nc + k] = mi355q_col_desc{MI355Q_INT32, cd.nullable, MI355Q_ENC_NONE, 0};
      p2.col_ranges[nc + k] = mi355q_range{1, r.has_nulls, 0, (int64_t)points - 1, 0.0, 0.0, 0};
      p2.group_cols[gcol] = nc + k;
      ++k;
    } else if (points >= ((__int128)1 << 30) || r.min <= -((int64_t)1 << 30) || r.min >= ((int64_t)1 << 30)) {
      return kNotTaken;
    }
    entries *= points + (r.has_nulls ? 1 : 0);
    if (entries > (__int128)kTwinMaxEntries) return kNotTaken;
  }
  // one key, one value column, >= 512 K lattice points: the 16-byte partitioned family does this shape as well as the twin's
  // two extra passes allow (BH009 at 1 B rows: 8.6 ms there, 9.9 ms here; 100 K points, BH008: 12.5 -> 8.2 ms;
  // profiles/r04_refbench_lattice_keys_call21.jsonl)
  {
    int vcols[MI355Q_MAX_TARGETS], n_v = 0;
    for (int t = 0; t < plan->n_targets; ++t) {
      const mi355q_target& tg = plan->targets[t];
      if (tg.agg == MI355Q_PROJECT_KEY || tg.col < 0) continue;
      bool seen = false;
      for (int k = 0; k < n_v; ++k) seen = seen || vcols[k] == tg.col;
      if (!seen) vcols[n_v++] = tg.col;
    }
    if (ng == 1 && n_v <= 1 && entries >= ((__int128)1 << 19) && o.kernel_variant != 2) return kNotTaken;
  }
  const int nc2 = nc + n_proj;
  p2.n_cols = nc2;
  PerfectTwinScope twin(kTwinMaxEntries);
  mi355q_qmd q2;
  if (qmd_init(p2, &q2) != MI355Q_OK) return kNotTaken;
  if (q2.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || q2.slot_width != 8 || q2.output_columnar ||
      q2.entry_count * (int64_t)q2.row_size > ((int64_t)4 << 30))
    return kNotTaken;
  for (int t = 0; t < plan->n_targets; ++t) {
    const int sf = q.target_slot[t], ss = q2.target_slot[t];
    if (plan->targets[t].agg == MI355Q_PROJECT_KEY) {
      if (sf >= 0) return kNotTaken;  // (baseline: projections are read from the key columns)
      continue;
    }
    if (sf < 0 || ss < 0) return kNotTaken;
    for (int j = 0; j < (plan->targets[t].agg == MI355Q_AVG ? 2 : 1); ++j)
      if (q.init_vals[sf + j] != q2.init_vals[ss + j]) return kNotTaken;
  }
  {  // the twin's step must be one of the two families this route is for
    DevPlan d2;
    if (build_dev_plan(p2, q2, &d2) != MI355Q_OK) return kNotTaken;
    std::vector<const void*> shape((size_t)nf * nc2);
    for (int f = 0; f < nf; ++f) {
      for (int c = 0; c < nc; ++c) shape[(size_t)f * nc2 + c] = in->col_buffers[(size_t)f * nc + c];
      for (int k = 0; k < n_proj; ++k) shape[(size_t)f * nc2 + nc + k] = (const void*)(uintptr_t)256;  // (16-byte aligned, like the real chunks)
    }
    FragView fvh{nullptr, nullptr, shape.data(), in->num_rows, nf, nc2, total_rows, max_frag_rows};
    if (!lds_groupby_eligible(d2, fvh, n_cus) && !idx_part_eligible(d2, fvh, n_cus)) return kNotTaken;
  }
  // ---- passes: lattice indices of a pass of fragments, the twin step on them
  int32_t w4[MI355Q_MAX_GROUP_COLS];
  for (int k = 0; k < n_proj; ++k) w4[k] = 4;
  PassLoop pl(rs.ctx.lattice, nc, n_proj, w4, &p2);
  pl.first_into_out_buffer = false;
  pl.inner_errors_not_taken = true;
  pl.twin = &q2;
  if (int32_t e = pl.prepare(in, o, total_rows, max_frag_rows)) return e;
  if (int32_t e = pl.run(rs, in, o, report, [&](int f, int pnf) -> int32_t {
        HIP_TRY(launch_affine_keys(n_proj, src_col, dst_col, width, nullable, kmin, stride, card, nc2, pl.d_tab, pl.d_rows + f, pnf,
                                   max_frag_rows, pl.d_err, n_cus, s));
        int32_t h_flag = 0;
        HIP_TRY(hipMemcpyAsync(&h_flag, pl.d_err, sizeof(h_flag), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return h_flag ? kNotTaken : MI355Q_OK;  // a key off the lattice of the first fragment: the plain route
      }))
    return e;
  const mi355q_result* tw = pl.res.get();  // the twin table (all passes folded)
  Emission em;
  if (int32_t e = em.create(q, in->device_id, o.out_buffer, s)) return e;
  HIP_TRY(launch_affine_twin_emit(em.res->dplan, tw->dplan, tw->qmd.idx_target_as_key, ng, translate, key_type, q2.group_min, q2.group_card,
                                  q2.group_null_key, base_of, stride_of, tw->buf, em.res->buf, em.d_err(), s));
  if (int32_t e = rs.finish(report, pl.acc, 1, *plan, *in, total_rows, em.d_err())) return e;
  *out = em.res.release();
  return MI355Q_OK;
}

// Does an expression of the plan read the value of another one (MI355Q_EX_COL with arg >= n_cols)?  The derived-plan routes
// below take expressions out of the plan and renumber the rest: they leave such plans to the projection.
static bool exprs_read_exprs(const mi355q_plan& p) {
  for (int k = 0; k < p.n_exprs && k < MI355Q_MAX_EXPRS; ++k)
    for (int i = 0; i < p.exprs[k].n_nodes && i < MI355Q_MAX_EXPR_NODES; ++i)
      if (p.exprs[k].nodes[i].op == MI355Q_EX_COL && p.exprs[k].nodes[i].arg >= p.n_cols) return true;
  return false;
}

// GROUP BY CAST(<plain integer column> AS DOUBLE | FLOAT) — the reference benchmark's BaselineHash and MultiStep
// BaselineHash shapes (Benchmarks/synthetic_benchmark/queries/BaselineHash/BH001-006.sql, MultiStep/MSBS001-005.sql).  A
// floating-point key always takes the baseline layout (GroupByAndAggregate.cpp:232-365: getExprRangeInfo is FloatingPoint),
// but the groups ARE the integer column's values: the step runs on a derived plan that groups by the integer column
// itself (perfect hash: the LDS / partitioned families, no key expression to project), and its entries are then re-keyed
// with the cast value and merged into the baseline table of the stated plan (kernels_generic.hip k_cast_key_emit).
// kNotTaken when the shape does not call for it.
int32_t execute_cast_key(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                         mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  if (plan->n_group_cols != 1 || plan->join_outer_col >= 0 || plan->output_columnar_hint != 0 || o.kernel_variant == 1 ||
      o.force_generic || exprs_read_exprs(*plan))
    return kNotTaken;
  const int nc = plan->n_cols, gc = plan->group_cols[0];
  if (gc < nc || gc >= nc + plan->n_exprs) return kNotTaken;
  const mi355q_expr& ex = plan->exprs[gc - nc];
  if (ex.n_nodes != 2 || ex.nodes[0].op != MI355Q_EX_COL || ex.nodes[1].op != MI355Q_EX_CAST) return kNotTaken;
  const int to = ex.nodes[1].type, c = ex.nodes[0].arg;
  if ((to != MI355Q_DOUBLE && to != MI355Q_FLOAT) || c < 0 || c >= nc) return kNotTaken;
  const mi355q_col_desc& cd = plan->cols[c];
  const mi355q_range& cr = plan->col_ranges[c];
  if ((cd.type != MI355Q_INT32 && cd.type != MI355Q_INT64) || cd.encoding != MI355Q_ENC_NONE ||
      (cd.logical_type != 0 && cd.logical_type != cd.type) || !cr.valid || cr.bucket != 0 || (cr.has_nulls && !cd.nullable))
    return kNotTaken;
  int64_t total_rows = 0;
  for (int f = 0; f < in->n_frags; ++f) total_rows += in->num_rows[f];
  // (kernel_variant 2 = "the large-input members": how the tests reach this route with small tables)
  if (o.kernel_variant != 2 && total_rows < ((int64_t)4 << 20)) return kNotTaken;
  // the derived plan: the key expression leaves, the expressions behind it move down one column
  mi355q_plan p2 = *plan;
  p2.group_cols[0] = c;
  for (int e = gc - nc; e + 1 < plan->n_exprs; ++e) p2.exprs[e] = plan->exprs[e + 1];
  p2.n_exprs = plan->n_exprs - 1;
  bool key_read = false;
  auto move = [&](int32_t& col) {
    key_read = key_read || col == gc;
    if (col > gc) --col;
  };
  for (int t = 0; t < p2.n_targets; ++t) {
    mi355q_target& tg = p2.targets[t];
    if (tg.agg == MI355Q_PROJECT_KEY) continue;
    if (tg.table == 0 && tg.col >= 0) move(tg.col);
    if (tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) move(tg.cond.col);
  }
  for (int i = 0; i < p2.n_quals; ++i) move(p2.quals[i].col);
  if (key_read) return kNotTaken;  // the cast value itself is aggregated or filtered on
  mi355q_qmd q, q2;
  if (qmd_init(*plan, &q) != MI355Q_OK || qmd_init(p2, &q2) != MI355Q_OK) return kNotTaken;
  if (q.desc_type != MI355Q_GROUP_BY_BASELINE_HASH || q.slot_width != 8 || q.key_width != 8 || q.output_columnar ||
      q2.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || q2.slot_width != 8 || q2.output_columnar)
    return kNotTaken;
  for (int t = 0; t < plan->n_targets; ++t) {
    const int sf = q.target_slot[t], ss = q2.target_slot[t];
    if (plan->targets[t].agg == MI355Q_PROJECT_KEY) {
      if (sf >= 0) return kNotTaken;  // (baseline: projections are read from the key column)
      continue;
    }
    if (sf < 0 || ss < 0) return kNotTaken;
    for (int j = 0; j < (plan->targets[t].agg == MI355Q_AVG ? 2 : 1); ++j)
      if (q.init_vals[sf + j] != q2.init_vals[ss + j]) return kNotTaken;
  }
  mi355q_exec_options o2 = o;
  o2.out_buffer = nullptr;
  if (reserved) {
    route_note("the step grouped by the integer column + k_cast_key_emit");
    return execute_impl(&p2, in, &o2, out, report, nullptr, reserved);
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  if (int32_t e = rs.begin_timing(report)) return e;
  o2.stream = s;
  mi355q_result* r2 = nullptr;
  mi355q_exec_report rep2{};
  if (int32_t e2 = mi355q_execute(&p2, in, &o2, &r2, &rep2)) {
    if (e2 == MI355Q_ERR_UNSUPPORTED || e2 == MI355Q_ERR_OUT_OF_GPU_MEM || e2 < 0) return kNotTaken;
    return e2;
  }
  ResultPtr r2_owner(r2);
  if (r2->qmd.desc_type != MI355Q_GROUP_BY_PERFECT_HASH || r2->qmd.slot_width != 8 || r2->qmd.output_columnar ||
      r2->qmd.entry_count != q2.entry_count || r2->qmd.group_min[0] != q2.group_min[0])
    return kNotTaken;
  Emission em;
  if (int32_t e = em.create(q, in->device_id, o.out_buffer, s)) return e;
  // (NULL keys of a nullable column sit at max + 1: groupByColumnCodegen translate_null_val, as plan.cpp build_dev_plan)
  // every integer of [-2^53, 2^53] is an exact double: a DOUBLE cast of a column inside that range keeps distinct keys distinct
  // (one entry per row of the stated table, plain stores); beyond it, and for FLOAT, entries merge and the emission uses atomics
  const int64_t kExactDouble = (int64_t)1 << 53;
  const bool injective = to == MI355Q_DOUBLE && cr.min >= -kExactDouble && cr.max <= kExactDouble;
  HIP_TRY(launch_cast_key_emit(em.res->dplan, r2->dplan, r2->qmd.idx_target_as_key, to == MI355Q_FLOAT ? 1 : 0, cd.nullable != 0,
                               injective ? 1 : 0, q2.group_min[0], q2.group_null_key[0], r2->buf, em.res->buf, em.d_err(), s));
  if (int32_t e = rs.finish(report, rep2, 1, *plan, *in, total_rows, em.d_err())) return e;
  *out = em.res.release();
  return MI355Q_OK;
}

// Aggregates whose argument is `plain INT column + / - literal` (the reference benchmark's MultiStep shapes:
// MAX(x10 + 1), SUM(x10 + 1) next to MAX(x10)).  The reference compiles the addition into the row function
// (ArithmeticIR.cpp:77-150); materialising it as a projected column costs a pass over the input and a value column of
// the exchange.  Where the column's range says the addition cannot overflow, the step runs on a derived plan that
// aggregates the COLUMN — MIN / MAX / SUM / AVG / COUNT of (x + L) are MIN(x) + L, MAX(x) + L, SUM(x) + L·COUNT(x),
// (SUM(x) + L·COUNT(x)) / COUNT(x), COUNT(x), with NULL rows skipped on both sides and wrapping 64-bit sums — and the
// literal is added while the derived table is copied into the stated layout (k_zip_targets).  The derived plan holds
// every distinct aggregate once, plus COUNT(x) where a sum needs it.  kNotTaken when the shape does not call for it.
int32_t execute_shifted_args(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                             mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  if (plan->n_group_cols < 1 || plan->join_outer_col >= 0 || plan->output_columnar_hint != 0 || o.kernel_variant == 1 ||
      o.force_generic || exprs_read_exprs(*plan))
    return kNotTaken;
  const int nc = plan->n_cols, nx = plan->n_exprs;
  // which expressions are `column +- literal` that cannot overflow
  int src_col[MI355Q_MAX_EXPRS];
  int64_t shift[MI355Q_MAX_EXPRS];
  bool any = false;
  for (int k = 0; k < nx; ++k) {
    src_col[k] = -1;
    const mi355q_expr& ex = plan->exprs[k];
    if (ex.n_nodes != 3 || ex.nodes[0].op != MI355Q_EX_COL || ex.nodes[1].op != MI355Q_EX_LIT || ex.nodes[1].reserved != 0 ||
        (ex.nodes[2].op != MI355Q_EX_ADD && ex.nodes[2].op != MI355Q_EX_SUB))
      continue;
    const int c = ex.nodes[0].arg;
    if (c < 0 || c >= nc) continue;
    const mi355q_col_desc& cd = plan->cols[c];
    const mi355q_range& r = plan->col_ranges[c];
    if ((cd.type != MI355Q_INT32 && cd.type != MI355Q_INT64) || cd.encoding != MI355Q_ENC_NONE ||
        (cd.logical_type != 0 && cd.logical_type != cd.type) || ex.nodes[1].type != cd.type || ex.nodes[2].type != cd.type ||
        !r.valid || r.min > r.max)
      continue;
    const __int128 L = ex.nodes[2].op == MI355Q_EX_ADD ? (__int128)ex.nodes[1].ilit : -(__int128)ex.nodes[1].ilit;
    const __int128 tmax = cd.type == MI355Q_INT32 ? (__int128)INT32_MAX : (__int128)INT64_MAX;
    // (the type's minimum is its NULL; the literal itself must be a value of the type)
    if ((__int128)r.max + L > tmax || (__int128)r.min + L <= -tmax - 1 || L > tmax || L < -tmax) continue;
    src_col[k] = c;
    shift[k] = (int64_t)L;
    any = true;
  }
  if (!any) return kNotTaken;
  // an expression that is also a key, a filter column or a condition stays projected
  for (int g = 0; g < plan->n_group_cols; ++g)
    if (plan->group_cols[g] >= nc && plan->group_cols[g] < nc + nx) src_col[plan->group_cols[g] - nc] = -1;
  for (int i = 0; i < plan->n_quals; ++i)
    if (plan->quals[i].col >= nc && plan->quals[i].col < nc + nx) src_col[plan->quals[i].col - nc] = -1;
  for (int t = 0; t < plan->n_targets; ++t) {
    const mi355q_target& tg = plan->targets[t];
    if ((tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) && tg.cond.col >= nc && tg.cond.col < nc + nx)
      src_col[tg.cond.col - nc] = -1;
    if (tg.agg != MI355Q_PROJECT_KEY && tg.table == 0 && tg.col >= nc && tg.col < nc + nx &&
        (tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF))
      src_col[tg.col - nc] = -1;
  }
  any = false;
  for (int k = 0; k < nx; ++k) any = any || src_col[k] >= 0;
  if (!any) return kNotTaken;
  int64_t total_rows = 0;
  for (int f = 0; f < in->n_frags; ++f) total_rows += in->num_rows[f];
  // (kernel_variant 2 = "the large-input members": how the tests reach this route with small tables)
  if (o.kernel_variant != 2 && total_rows < ((int64_t)4 << 20)) return kNotTaken;

  // the derived plan: the shifted expressions leave (the others move down), every distinct aggregate once
  mi355q_plan p2 = *plan;
  int new_col[MI355Q_MAX_EXPRS];  // column index of a kept expression in the derived plan
  p2.n_exprs = 0;
  for (int k = 0; k < nx; ++k) {
    if (src_col[k] >= 0) {
      new_col[k] = -1;
    } else {
      new_col[k] = nc + p2.n_exprs;
      p2.exprs[p2.n_exprs++] = plan->exprs[k];
    }
  }
  auto moved = [&](int col) { return col >= nc && col < nc + nx ? new_col[col - nc] : col; };
  for (int g = 0; g < p2.n_group_cols; ++g) p2.group_cols[g] = moved(plan->group_cols[g]);
  for (int i = 0; i < p2.n_quals; ++i) p2.quals[i].col = moved(plan->quals[i].col);
  p2.n_targets = 0;
  int t2_of[MI355Q_MAX_TARGETS], cnt_t2[MI355Q_MAX_TARGETS];  // final target -> derived target; -> the derived COUNT(x)
  int64_t lit_of[MI355Q_MAX_TARGETS];
  auto same = [](const mi355q_target& a, const mi355q_target& b) {
    return a.agg == b.agg && a.col == b.col && a.table == b.table && a.cond.col == b.cond.col && a.cond.op == b.cond.op &&
           a.cond.ival == b.cond.ival && a.cond.fval == b.cond.fval;
  };
  auto add_target = [&](const mi355q_target& tg) {
    for (int i = 0; i < p2.n_targets; ++i)
      if (same(p2.targets[i], tg)) return i;
    if (p2.n_targets >= MI355Q_MAX_TARGETS) return -1;
    p2.targets[p2.n_targets] = tg;
    return p2.n_targets++;
  };
  for (int t = 0; t < plan->n_targets; ++t) {
    mi355q_target tg = plan->targets[t];
    lit_of[t] = 0;
    cnt_t2[t] = -1;
    if (tg.agg != MI355Q_PROJECT_KEY && tg.table == 0 && tg.col >= nc && tg.col < nc + nx) {
      const int k = tg.col - nc;
      if (src_col[k] >= 0) {
        tg.col = src_col[k];
        lit_of[t] = shift[k];
      } else {
        tg.col = new_col[k];
      }
    }
    if (tg.agg == MI355Q_COUNT_IF || tg.agg == MI355Q_SUM_IF) tg.cond.col = moved(tg.cond.col);
    t2_of[t] = tg.agg == MI355Q_PROJECT_KEY ? (p2.n_targets < MI355Q_MAX_TARGETS ? (p2.targets[p2.n_targets] = tg, p2.n_targets++) : -1)
                                            : add_target(tg);
    if (t2_of[t] < 0) return kNotTaken;
  }
  for (int t = 0; t < plan->n_targets; ++t) {  // the counts the shifted MIN / MAX / SUM targets need
    const mi355q_target& tg = plan->targets[t];
    if (!lit_of[t] || tg.agg == MI355Q_COUNT || tg.agg == MI355Q_AVG) continue;  // (AVG carries its own count)
    mi355q_target cnt{};
    cnt.agg = MI355Q_COUNT;
    cnt.col = p2.targets[t2_of[t]].col;
    cnt.table = 0;
    cnt_t2[t] = add_target(cnt);
    if (cnt_t2[t] < 0) return kNotTaken;
  }
  mi355q_qmd q, q2;
  if (qmd_init(*plan, &q) != MI355Q_OK || qmd_init(p2, &q2) != MI355Q_OK) return kNotTaken;
  if (q.slot_width != 8 || q2.slot_width != 8 || q.output_columnar || q2.output_columnar || q.desc_type != q2.desc_type ||
      q.entry_count != q2.entry_count || q.desc_type == MI355Q_NON_GROUPED_AGGREGATE ||
      (q.desc_type == MI355Q_GROUP_BY_BASELINE_HASH && q.key_width != q2.key_width))
    return kNotTaken;
  int32_t src[MI355Q_MAX_SLOTS], dst[MI355Q_MAX_SLOTS], kind[MI355Q_MAX_SLOTS], cnt_src[MI355Q_MAX_SLOTS];
  int64_t lit[MI355Q_MAX_SLOTS];
  int n = 0;
  for (int t = 0; t < plan->n_targets; ++t) {
    const int sf = q.target_slot[t], ss = q2.target_slot[t2_of[t]];
    if ((sf < 0) != (ss < 0)) return kNotTaken;  // (a projection read from the key columns on both sides)
    if (sf < 0) continue;
    const int agg = plan->targets[t].agg;
    for (int j = 0; j < (agg == MI355Q_AVG ? 2 : 1); ++j) {
      if (q.init_vals[sf + j] != q2.init_vals[ss + j] || n >= MI355Q_MAX_SLOTS) return kNotTaken;
      src[n] = ss + j;
      dst[n] = sf + j;
      kind[n] = 0;
      cnt_src[n] = 0;
      lit[n] = 0;
      if (lit_of[t] && j == 0 && agg != MI355Q_COUNT) {
        kind[n] = (agg == MI355Q_SUM || agg == MI355Q_AVG) ? 2 : 1;
        cnt_src[n] = agg == MI355Q_AVG ? ss + 1 : q2.target_slot[cnt_t2[t]];
        if (cnt_src[n] < 0) return kNotTaken;
        lit[n] = lit_of[t];
      }
      ++n;
    }
  }
  mi355q_exec_options o2 = o;
  o2.out_buffer = nullptr;
  if (reserved) {
    route_note("aggregates of column + literal from the column's aggregates + k_zip_targets");
    return execute_impl(&p2, in, &o2, out, report, nullptr, reserved);
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  hipStream_t s = rs.s;
  if (int32_t e = rs.begin_timing(report)) return e;
  o2.stream = s;
  mi355q_result* r2 = nullptr;
  mi355q_exec_report rep2{};
  if (int32_t e2 = mi355q_execute(&p2, in, &o2, &r2, &rep2)) {
    if (e2 == MI355Q_ERR_UNSUPPORTED || e2 == MI355Q_ERR_OUT_OF_GPU_MEM) return kNotTaken;
    return e2;  // (out of slots included: the derived table has the stated table's entry count)
  }
  ResultPtr r2_owner(r2);
  if (r2->qmd.desc_type != q.desc_type || r2->qmd.entry_count != q.entry_count || r2->qmd.slot_width != 8 ||
      r2->qmd.output_columnar)
    return kNotTaken;
  for (int t = 0; t < plan->n_targets; ++t)
    if (r2->qmd.target_slot[t2_of[t]] != q2.target_slot[t2_of[t]]) return kNotTaken;
  Emission em;
  if (int32_t e = em.create(q, in->device_id, o.out_buffer, s)) return e;
  HIP_TRY(launch_zip_targets(em.res->dplan, r2->dplan, r2->qmd.idx_target_as_key, r2->buf, em.res->buf, src, dst, n, em.d_err(), s,
                             kind, cnt_src, lit, /*into_empty_table=*/true));
  if (int32_t e = rs.finish(report, rep2, 1, *plan, *in, total_rows, em.d_err())) return e;
  *out = em.res.release();
  return MI355Q_OK;
}

// ---- the two program routes (execute_agg_programs, execute_grouped_agg_programs): aggregates whose arguments are evaluated
// in the kernel's registers.  They share what they refuse, what they derive from the stated plan, and the step itself:
// one kernel over the stated table, one error word back.  Each keeps its own conditions around these.

// An expression a qual or another expression reads is evaluated for every row: the projection pass's business.  So is a
// disjunction among the quals.
static bool program_step_refuses(const mi355q_plan& plan) {
  for (int i = 0; i < plan.n_quals; ++i)
    if (MI355Q_QUAL_OR_GROUP(plan.quals[i].op) != 0) return true;
  return expr_qual_mask(plan) != 0 || exprs_read_exprs(plan);
}

// The stated plan as a program step's kernel takes it: the lowered plan (whose targets give an argument its type and NULL
// rule), the stated plan's layout, the device plan and the arguments' two-register programs.
struct ProgramStep {
  mi355q_plan lp;
  DevExprSet xs;
  mi355q_qmd q;
  DevPlan d;
  AggProgArgs ap;
};
// false: not a step of these routes (the layout is not `desc_type` with 8-byte slots, row-wise; an argument the form does
// not state, regprog.h agg_prog_args_of)
static bool lower_program_step(const mi355q_plan& plan, int32_t desc_type, ProgramStep* ps) {
  if (lower_exprs(plan, &ps->lp, &ps->xs, true) != MI355Q_OK || qmd_init(plan, &ps->q) != MI355Q_OK) return false;
  if (ps->q.desc_type != desc_type || ps->q.slot_width != 8 || ps->q.output_columnar) return false;
  if (build_dev_plan(ps->lp, ps->q, &ps->d) != MI355Q_OK) return false;
  return agg_prog_args_of(ps->d, ps->xs, &ps->ap);
}

// The step of both routes behind their eligibility checks: the fragment table up, the result initialised, ONE launch —
// `launch`, a hipError_t(const FragView&, int64_t* buf, int32_t* d_err, hipStream_t, LaunchStats*) that is handed fv with
// the device's column table — and d_err[0] back; a code there ends the step with no result.  The kernel's event pair is
// the step's time as well.  RESERVE mode (mi355q_reserve_workspace / mi355q_explain) notes the route and its kernel, lays
// the table out, creates the events and launches nothing: there are no temporary columns to reserve.
template <class Launch>
static int32_t run_program_step(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                                FragView fv, const char* route, const char* kernel, Launch&& launch, mi355q_result** out,
                                mi355q_exec_report* report, int64_t* reserved) {
  if (reserved) {
    route_note(route);
    route_note(kernel);
    *reserved = 0;
    if (t_plan_only) return MI355Q_OK;
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  DeviceCtx& ctx = rs.ctx;
  // column table | row counts | error words, one upload out of pinned memory (reserve: laid out only)
  FragTable ft;
  if (int32_t e = upload_frag_table(ctx, *in, fv.n_cols, o.stream, reserved ? FragUpload::kNone : FragUpload::kAlways, &ft)) return e;
  LaunchStats st;
  if (report || reserved) {
    if (int32_t e = grow_events(ctx, 4)) return e;
    st.k_start = ctx.events[2];
    st.k_stop = ctx.events[3];
  }
  if (reserved) return MI355Q_OK;
  hipStream_t s = ft.s;
  UploadGuard upload_guard{s, true};
  mi355q_result* res = nullptr;
  if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &res)) return e;
  ResultPtr owned(res);
  fv.d_cols = ft.d_cols;
  fv.d_num_rows = ft.d_rows;
  HIP_TRY(launch_init_buffer(res->buf, q.entry_count, make_row_init(q), s));
  HIP_TRY(launch(fv, res->buf, ft.d_err, s, &st));
  int32_t* h_ret = (int32_t*)(ctx.h_meta + ctx.meta_bytes);
  HIP_TRY(hipMemcpyAsync(h_ret, ft.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  upload_guard.armed = false;
  const int32_t code = h_ret[0];
  if (report) {
    std::memset(report, 0, sizeof(*report));
    std::snprintf(report->kernel_name, sizeof(report->kernel_name), "%s", st.kernel_name);
    if (hipEventElapsedTime(&report->kernel_ms, st.k_start, st.k_stop) != hipSuccess) report->kernel_ms = 0.f;
    report->total_ms = report->kernel_ms;
    report->n_launches = st.n_launches;
    report->variant = st.variant;
    report->rows_scanned = fv.total_rows;
    report->algorithmic_bytes = algorithmic_bytes(*plan, *in);
  }
  if (code) return code;
  *out = owned.release();
  return MI355Q_OK;
}

// Non-grouped aggregates whose ARGUMENTS are expressions — SUM(a * b) WHERE c < k, TPC-H Q6's shape.  The reference compiles
// the argument into the row function (codegenArith, ArithmeticIR.cpp:39-431) and aggregates it in the kernel's registers
// (query_template, QueryTemplateGenerator.cpp:265-549).  Here every expression that compiles into a two-register program
// (regprog.h) is evaluated by k_scan_agg_prog on the values the scan has loaded: one kernel, no temporary column, no
// synchronisation in between (execute_projected: k_project writes 8 bytes per row and expression, k_scan_agg reads them
// back).  The kernel takes the type and the NULL rule of an argument from the lowered plan's targets — what the plain-column
// step would have applied to the temporary column — so both paths state the same result.  Taken at every input size: a
// non-grouped step has no table to amortise.  kNotTaken: anything the form does not state (regprog.h agg_prog_args_of,
// kernels_filter.hip sap_args); that plan keeps the projection pass.
int32_t execute_agg_programs(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                             mi355q_exec_report* report, int64_t* reserved) {
  if (plan->n_exprs <= 0 || plan->n_group_cols != 0 || plan->join_outer_col >= 0 || plan->output_columnar_hint != 0 || o.force_generic ||
      in->n_frags <= 0 || (o.flags & MI355Q_OPT_NO_AGG_PROGRAMS) || plan->n_quals < 0 || plan->n_quals > MI355Q_MAX_QUALS ||
      plan->n_targets < 1 || plan->n_targets > MI355Q_MAX_TARGETS || program_step_refuses(*plan))
    return kNotTaken;
  ProgramStep ps;
  if (!lower_program_step(*plan, MI355Q_NON_GROUPED_AGGREGATE, &ps)) return kNotTaken;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  // (the kernel reads physical columns only: the table it is handed is the stated one, n_cols columns per fragment)
  FragView fv{nullptr, nullptr, in->col_buffers, in->num_rows, in->n_frags, plan->n_cols, total_rows, max_frag_rows};
  if (!scan_agg_prog_eligible(ps.d, ps.ap, fv)) return kNotTaken;
  const int n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);
  // (the error a passing row raised ends the step with no result, as execute_masked treats its pre-pass's)
  return run_program_step(plan, in, o, ps.q, fv, "aggregate arguments as register programs", "k_scan_agg_prog",
                          [&](const FragView& dv, int64_t* buf, int32_t* d_err, hipStream_t s, LaunchStats* st) {
                            return launch_scan_agg_prog(ps.d, ps.ap, dv, buf, d_err, n_cus, s, st);
                          },
                          out, report, reserved);
}

// The GROUPED half of the route above — SELECT g, SUM(a * b), COUNT(*) FROM t WHERE c < k GROUP BY g — for the few-groups
// shapes: a perfect-hash layout over 1 - 3 plain INT32 / INT64 key columns whose table fits up to 8 windows of LDS.  The
// reference compiles such arguments into the row function all the same (ArithmeticIR.cpp:39-431); here k_groupby_lds_prog
// (kernels_lds.hip) keeps k_groupby_lds's replicated table and evaluates the arguments' programs on the values it has loaded:
// one kernel, no temporary column (8 bytes per row and expression on the two-pass route, which falls back to several passes
// once they exceed a third of the free memory), no synchronisation in between.  Type and NULL rule of an argument come from
// the lowered plan's targets, as above.
// Size rule: from 2^20 rows on, or when kernel_variant 2 asks for the large-input members (how the tests reach this route
// with small tables).  The threshold is a routing constant — the one the compiled filter uses — not a measured crossover:
// below it the two-pass step costs launches, not bandwidth.
// Class rule (grouped_prog_class_on_by_default below): above the threshold a step takes the route BY DEFAULT only if its
// class of arguments beat the two-pass route when measured.  None did, so today the route runs with kernel_variant 2 alone.
// kNotTaken: baseline layouts, expression keys, division / CASE / BOOLEAN results, narrow, FLOAT or encoded operands, _IF
// targets, joins, columnar or 4-byte-slot layouts, a compiled filter, more than 3 arguments, range quals on more than 4
// distinct columns (or on more than 2 that are neither operand nor key columns), tables beyond 8 windows (regprog.h
// agg_prog_args_of, lds_args.h make_lds_prog_args); that plan keeps the projection pass.
//
// A shape class is the type of the program arguments.  1 B rows, one INT32 key with 100 / 1000 groups, 50 % qual, this route
// against the two passes (k_project, then k_perfect_lds), best of 7 steps, three alternating runs each
// (profiles/agg_prog_grouped_bench_1b.jsonl):
//   INT32   SUM(a * b)                                  11.42 - 11.45 ms  against   7.84 -  7.93   LOST
//   INT64   SUM(CAST(a AS BIGINT) * CAST(b AS BIGINT))  13.47 - 13.52     against   9.98 - 10.13   LOST
//   DOUBLE  SUM / MIN / AVG(p * 2.5 - q)                12.48 - 12.53     against  10.93 - 11.21   LOST
// A class that loses stays on k_project by default; what the route removes there — the temporary columns, 8 bytes per row and
// expression — is had by asking for it (kernel_variant 2).
static bool grouped_prog_class_on_by_default(const AggProgArgs& ap) {
  for (int k = 0; k < ap.n_progs; ++k) {
    switch (ap.prog[k].type) {
      case MI355Q_INT32: return false;   // lost by 3.5 ms per 1 B rows
      case MI355Q_INT64: return false;   // lost by 3.4 ms
      case MI355Q_DOUBLE: return false;  // lost by 1.3 ms
      default: return false;
    }
  }
  return false;  // (no program at all: not this route's step)
}

int32_t execute_grouped_agg_programs(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                     mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  if (plan->n_exprs <= 0 || plan->n_group_cols < 1 || plan->n_group_cols > 3 || plan->join_outer_col >= 0 || plan->output_columnar_hint != 0 ||
      o.force_generic || in->n_frags <= 0 || (o.flags & MI355Q_OPT_NO_GROUPED_AGG_PROGRAMS) || plan->n_quals < 0 ||
      plan->n_quals > MI355Q_MAX_QUALS || plan->n_targets < 1 || plan->n_targets > MI355Q_MAX_TARGETS || step_bool_filter() ||
      program_step_refuses(*plan))
    return kNotTaken;
  // (the rows ahead of the lowering here: the size rule spares a small step the lowering)
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  if (o.kernel_variant != 2 && total_rows < ((int64_t)1 << 20)) return kNotTaken;  // (the size rule above)
  ProgramStep ps;
  if (!lower_program_step(*plan, MI355Q_GROUP_BY_PERFECT_HASH, &ps)) return kNotTaken;
  if (o.kernel_variant != 2 && !grouped_prog_class_on_by_default(ps.ap)) return kNotTaken;  // (the class rule above)
  // (the kernel reads physical columns only: the table it is handed is the stated one, n_cols columns per fragment)
  FragView fv{nullptr, nullptr, in->col_buffers, in->num_rows, in->n_frags, plan->n_cols, total_rows, max_frag_rows};
  const int n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);
  if (!lds_groupby_prog_eligible(ps.d, ps.ap, fv, n_cus)) return kNotTaken;
  // (an error a passing row raised (7), or a key outside its declared range, ends the step with no result)
  return run_program_step(plan, in, o, ps.q, fv, "grouped aggregate arguments as register programs", "k_groupby_lds_prog",
                          [&](const FragView& dv, int64_t* buf, int32_t* d_err, hipStream_t s, LaunchStats* st) {
                            return launch_lds_groupby_prog(ps.d, ps.ap, dv, buf, d_err, n_cus, s, st);
                          },
                          out, report, reserved);
}

// Plans with projected expressions (mi355q_expr): scan / filter / PROJECT.  The expressions of a pass of
// fragments are evaluated into dense temporary columns (k_project), the step runs on the lowered plan — where
// those columns are ordinary inputs, so every kernel family applies — and the passes' results are folded with
// the reduce rule (ResultSetStorage::reduce, as for the reference's per-fragment kernels).  One pass when the
// temporary columns fit a third of the free memory (<= 16 GB).
int32_t execute_projected(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                          mi355q_result** out, mi355q_exec_report* report) {
  mi355q_plan lp;
  DevExprSet xs;
  if (int32_t e = lower_exprs(*plan, &lp, &xs, true)) return e;
  mi355q_qmd q;
  if (int32_t e = qmd_init(*plan, &q)) return e;
  DevPlan d;
  if (int32_t e = build_dev_plan(lp, q, &d)) return e;
  if (int32_t e = attach_join(lp, in, &d)) return e;
  const int nf = in->n_frags, nc = plan->n_cols, nx = plan->n_exprs, nc2 = nc + nx;
  if (nf == 0) return mi355q_execute(&lp, in, &o, out, report);
  const uint32_t qual_expr_mask = expr_qual_mask(*plan);
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  int32_t widths[MI355Q_MAX_EXPRS];
  for (int k = 0; k < nx; ++k) widths[k] = plain_width(xs.e[k].store_type);

  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  const int n_cus = cu_count_of(in->device_id);
  hipStream_t s = rs.s;
  PassLoop pl(rs.ctx.proj, nc, nx, widths, &lp);
  pl.bytes_after_err = ((int64_t)sizeof(DevExprSet) + 255) & ~255ll;  // the lowered programs, read by k_project from device memory
  pl.alloc_failed = MI355Q_ERR_OUT_OF_GPU_MEM;
  pl.count_pre_pass = false;
  if (int32_t e = pl.prepare(in, o, total_rows, max_frag_rows)) return e;
  DevExprSet* d_xs = (DevExprSet*)pl.after_err;
  if (int32_t e = pl.run(rs, in, o, report, [&](int f, int pnf) -> int32_t {
        // one-operation expressions over aligned plain columns: the vectorised members (k_project_simple); an overflow there
        // only raises word 2 and the interpreter (which knows whether the offending row counts) runs after all
        bool simple = project_simple_shapes(xs) && !o.force_generic;
        for (size_t i = 0; simple && i < (size_t)pnf * nc2; ++i) simple = ((uintptr_t)pl.cols2[i] & 15) == 0;
        HIP_TRY(launch_project(xs, d_xs, d, qual_expr_mask, pl.d_tab, pl.d_rows + f, pnf, max_frag_rows, pl.d_err, n_cus, s, simple));
        int32_t h_err3[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(h_err3, pl.d_err, sizeof(h_err3), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));  // (cols2 is re-used by the next pass; the step below synchronises anyway)
        if (simple && h_err3[2]) {
          HIP_TRY(hipMemsetAsync(pl.d_err, 0, 64, s));
          HIP_TRY(launch_project(xs, d_xs, d, qual_expr_mask, pl.d_tab, pl.d_rows + f, pnf, max_frag_rows, pl.d_err, n_cus, s, false));
          HIP_TRY(hipMemcpyAsync(h_err3, pl.d_err, sizeof(h_err3), hipMemcpyDeviceToHost, s));
          HIP_TRY(hipStreamSynchronize(s));
        }
        return h_err3[0];
      }))
    return e;
  if (int32_t e = rs.finish_sync_if_timed(report, pl.acc, *plan, *in, total_rows)) return e;
  *out = pl.res.release();
  return MI355Q_OK;
}


// A filter compiled at plan time whose atoms include PROGRAMS (boolfilter.h, regprog.h: `b <> 0 AND a / b > 3`, `x + y > 100`,
// `a < b`, DOUBLE leaves): the pre-pass k_filter_mask streams the filter's columns once and leaves one byte per row, the step
// proper is `rest` (the stated plan without quals and expressions) with ONE more column — the mask, INT8 NOT NULL in [0, 1] —
// and the qual `mask = 1`, which every typed family loads as one 4-byte word per quad.  Errors (7 / 1) surface from the
// pre-pass: every row evaluates the filter's expressions, as the row function does ahead of its quals.
// kNotTaken: unaligned filter columns, no room for one more column (the caller falls through to the interpreter pass).
int32_t execute_masked(const mi355q_plan* plan, const mi355q_plan& rest, const BoolFilterHost& bfh, const mi355q_inputs* in,
                       const mi355q_exec_options& o, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  const int nc = rest.n_cols, nc2 = nc + 1, nf = in->n_frags;
  if (nc2 > MI355Q_MAX_COLS || rest.n_quals != 0 || rest.n_exprs != 0) return kNotTaken;
  // `arg IS NOT NULL` on an aggregate's own argument is part of the LAYOUT (constrained_not_null, plan.cpp resolve_targets: the
  // slot's initial value and its NULL handling), and the masked plan states no quals: its table would not be the stated one
  for (int k = 0; k < plan->n_quals && k < MI355Q_MAX_QUALS; ++k) {
    if (MI355Q_QUAL_OP(plan->quals[k].op) != MI355Q_IS_NOT_NULL) continue;
    for (int t = 0; t < plan->n_targets && t < MI355Q_MAX_TARGETS; ++t) {
      const mi355q_target& tg = plan->targets[t];
      if (tg.agg != MI355Q_PROJECT_KEY && tg.agg != MI355Q_PROJECT && tg.table == 0 && tg.col == plan->quals[k].col) return kNotTaken;
    }
  }
  mi355q_plan mp = rest;
  mp.n_cols = nc2;
  std::memset(&mp.cols[nc], 0, sizeof(mp.cols[nc]));
  mp.cols[nc].type = MI355Q_INT8;
  std::memset(&mp.col_ranges[nc], 0, sizeof(mp.col_ranges[nc]));
  mp.col_ranges[nc].valid = 1;
  mp.col_ranges[nc].min = 0;
  mp.col_ranges[nc].max = 1;
  mp.n_quals = 1;
  std::memset(&mp.quals[0], 0, sizeof(mp.quals[0]));
  mp.quals[0].col = nc;
  mp.quals[0].op = MI355Q_EQ;
  mp.quals[0].ival = 1;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  if (reserved) {  // mi355q_reserve_workspace / mi355q_explain: nothing is launched
    route_note("k_filter_mask (program atoms + truth table -> 1 B/row)");
    return execute_impl(&mp, in, &o, out, report, nullptr, reserved);
  }
  if (nf == 0) return mi355q_execute(&mp, in, &o, out, report);
  {
    FragView hv{nullptr, nullptr, in->col_buffers, in->num_rows, nf, nc, total_rows, max_frag_rows};
    if (!filter_mask_eligible(bfh.bf, hv)) return kNotTaken;
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  const int n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);
  DeviceCtx& ctx = rs.ctx;
  hipStream_t s = rs.s;
  // one pass of fragments = as many as the mask region holds (1 B/row: 16 GB of it cover 16 G rows)
  const int32_t mask_width = 1;
  PassLoop pl(ctx.maskws, nc, 1, &mask_width, &mp);
  pl.mask_column = true;
  pl.bytes_after_tab = ((int64_t)sizeof(void*) * nf + 255) & ~255ll;  // per fragment: its mask chunk
  pl.alloc_failed = MI355Q_ERR_OUT_OF_GPU_MEM;
  if (int32_t e = pl.prepare(in, o, total_rows, max_frag_rows)) return e;
  if (!ctx.bf_table) HIP_TRY(hipMalloc(&ctx.bf_table, sizeof(BoolFilter)));
  HIP_TRY(hipMemcpy(ctx.bf_table, &bfh.bf, sizeof(BoolFilter), hipMemcpyHostToDevice));  // (synchronous: out of the caller's frame)
  int8_t** d_mtab = (int8_t**)pl.after_tab;
  std::vector<const void*> masks((size_t)nf);
  if (int32_t e = pl.run(rs, in, o, report, [&](int f, int pnf) -> int32_t {
        int64_t prows = 0, pmax = 0;
        for (int i = 0; i < pnf; ++i) {
          masks[(size_t)i] = pl.cols2[(size_t)i * nc2 + nc];
          prows += in->num_rows[f + i];
          pmax = std::max(pmax, in->num_rows[f + i]);
        }
        HIP_TRY(hipMemcpyAsync(d_mtab, masks.data(), sizeof(void*) * (size_t)pnf, hipMemcpyHostToDevice, s));
        FragView fv{pl.d_tab, pl.d_rows + f, in->col_buffers + (size_t)f * nc, in->num_rows + f, pnf, nc, prows, pmax};
        HIP_TRY(launch_filter_mask(bfh.bf, (const BoolFilter*)ctx.bf_table, fv, d_mtab, pl.d_err, n_cus, s));
        int32_t h_err = 0;
        // (a filter that cannot raise leaves nothing to look at: only the wait — masks / cols2 are re-used by the next pass)
        if (bfh.bf.any_raise) HIP_TRY(hipMemcpyAsync(&h_err, pl.d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return h_err;
      }))
    return e;
  if (int32_t e = rs.finish_sync_if_timed(report, pl.acc, *plan, *in, total_rows)) return e;
  *out = pl.res.release();
  return MI355Q_OK;
}

// SEMI / ANTI join levels (MI355Q_JOIN_SEMI / _ANTI, include/mi355q.h: `WHERE EXISTS (SELECT 1 FROM d WHERE d.k = f.k)`, `NOT
// EXISTS`, `IN (subquery)`).  Such a level reads no inner column: it is a row mask computed by probing the join table.  The
// pre-pass k_join_exists_mask streams the key column(s) once and leaves one byte per row (1 = the row passes the level); the step
// proper is the stated plan WITHOUT the join plus that INT8 column and the qual `mask = 1` (plan.cpp exists_join_plans), handed
// to execute_impl — so every typed family, the Projection's members and the compiled-quals stage apply, over every kind of join
// table.  Passes as execute_masked sizes them.  The pre-pass raises nothing.  Never kNotTaken.
// (the one class restated as the INNER plan, below: from 100 M slots, and from the input size at which the INNER plan's family
// is k_part_join, api.cpp select_family)
constexpr int64_t kExistsAsInnerMinSlots = 100000000, kExistsAsInnerMinRows = (int64_t)64 << 20;
int32_t execute_exists_join(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                            mi355q_exec_report* report, int64_t* reserved) {
  mi355q_plan jl, mp;
  int mask_col = -1;
  if (int32_t e = exists_join_plans(*plan, &jl, &mp, &mask_col)) return e;
  const bool anti = plan->join_kind == MI355Q_JOIN_ANTI;
  // the derived plan has the stated layout: the mask column is no key and no argument, and the quals stay — an `arg IS NOT NULL`
  // qual on an aggregate's own argument, which is part of the layout (constrained_not_null), among them
  mi355q_qmd q, q2;
  if (int32_t e = qmd_init(jl, &q)) return e;
  if (qmd_init(mp, &q2) != MI355Q_OK || std::memcmp(&q, &q2, sizeof(q)) != 0) return MI355Q_ERR_UNSUPPORTED;
  for (int k = 0; k < plan->n_quals; ++k)
    if (std::memcmp(&mp.quals[k], &plan->quals[k], sizeof(mi355q_qual)) != 0) return MI355Q_ERR_UNSUPPORTED;  // (cannot happen)
  // the join as the device sees it: a carrier plan that keeps the stated columns and the join and nothing else (attach_join
  // knows INNER and LEFT; the probe of an INNER level is the probe of these two)
  mi355q_plan cp = *plan;
  cp.n_quals = 0;
  cp.n_group_cols = 0;
  cp.n_targets = 1;
  cp.targets[0] = mi355q_target{};
  cp.targets[0].agg = MI355Q_COUNT;
  cp.targets[0].col = -1;
  cp.output_columnar_hint = MI355Q_OUTPUT_ROWWISE;
  cp.scan_limit = 0;
  cp.join_kind = MI355Q_JOIN_INNER;
  cp.n_inner_cols = 0;
  mi355q_qmd cq;
  if (int32_t e = qmd_init(cp, &cq)) return e;
  DevPlan d;
  if (int32_t e = build_dev_plan(cp, cq, &d)) return e;
  if (int32_t e = attach_join(cp, in, &d)) return e;
  const int nc = plan->n_cols, nc2 = nc + 1, nf = in->n_frags;
  int64_t total_rows = 0, max_frag_rows = 0;
  if (int32_t e = frag_row_totals(*in, &total_rows, &max_frag_rows)) return e;
  mi355q_inputs in_outer = *in;  // the derived steps have no inner side
  in_outer.inner_col_buffers = nullptr;
  in_outer.inner_num_rows = 0;
  // an empty dimension (a table built from no row), or no fact row: no pre-pass.  SEMI: the joinless plan over no rows; ANTI:
  // the joinless plan itself
  if (plan->join_table->num_rows == 0 || total_rows == 0) {
    if (reserved)
      route_note(anti ? "anti join over an empty dimension (no k_join_exists_mask pre-pass): the joinless plan"
                      : "semi join over an empty dimension (no k_join_exists_mask pre-pass): the joinless plan over no rows");
    if (!anti) in_outer.n_frags = 0;
    return execute_impl(&jl, &in_outer, &o, out, report, nullptr, reserved);
  }
  // SEMI over a ONE-TO-ONE table keeps exactly the rows the INNER join keeps (a row has at most one match).  Measured at 1 B rows
  // (DESIGN 3.10): the non-grouped step over a 100 M-slot table — a 12.5 MB presence map, beyond one XCD's L2 — takes 7.3 ms as
  // the INNER plan (k_part_scatter + k_part_join: the probes partitioned so that a map slice fits LDS) and 13.1 ms through the
  // mask; with 1 M slots the mask route wins (6.7 against 7.4 ms), as it does for grouped steps at both sizes.  So that one
  // class is restated, where the INNER plan's family is the measured one; a forced kernel_variant keeps the mask route.
  if (!anti && o.kernel_variant == 0 && !o.force_generic && d.join_hash_type == 0 && q.desc_type == MI355Q_NON_GROUPED_AGGREGATE &&
      d.join_entries >= kExistsAsInnerMinSlots && total_rows >= kExistsAsInnerMinRows) {
    mi355q_plan ip = *plan;
    ip.join_kind = MI355Q_JOIN_INNER;
    mi355q_qmd iq;
    DevPlan id;
    FragView hv{nullptr, nullptr, in->col_buffers, in->num_rows, nf, nc, total_rows, max_frag_rows};
    if (qmd_init(ip, &iq) == MI355Q_OK && std::memcmp(&iq, &q, sizeof(q)) == 0 && build_dev_plan(ip, iq, &id) == MI355Q_OK &&
        attach_join(ip, in, &id) == MI355Q_OK && join_part_supported(id, hv, cu_count_of(in->device_id))) {
      if (reserved) route_note("semi join over a one-to-one table as the INNER join");
      return execute_impl(&ip, in, &o, out, report, nullptr, reserved);
    }
  }
  const int32_t mask_width = 1;
  const int64_t mtab_bytes = ((int64_t)sizeof(void*) * nf + 255) & ~255ll;  // per fragment: its mask chunk
  if (reserved) {  // mi355q_reserve_workspace / mi355q_explain: nothing is launched
    {
      FragView hv{nullptr, nullptr, in->col_buffers, in->num_rows, nf, nc, total_rows, max_frag_rows};
      const std::string note = std::string(anti ? "anti" : "semi") + " join as a row mask: k_join_exists_mask" +
                               (join_exists_mask_fast_eligible(d, hv) ? " (fast member)" : " (general member)");
      route_note(note.c_str());
    }
    // the derived step's shape: the same fragments with nc2 columns (the pointers are looked at for alignment only)
    std::vector<const void*> cols2((size_t)nf * nc2, nullptr);
    for (int f = 0; f < nf; ++f) std::copy_n(in->col_buffers + (size_t)f * nc, nc, cols2.begin() + (size_t)f * nc2);
    in_outer.col_buffers = cols2.data();
    if (int32_t e = execute_impl(&mp, &in_outer, &o, out, report, nullptr, reserved)) return e;
    // ... and the mask region of the passes, which the derived step knows nothing of: reported, and allocated when reserving
    if (t_plan_only) {
      PassLoop pl(ctx_of(in->device_id).maskws, nc, 1, &mask_width, &mp);
      pl.mask_column = true;
      pl.bytes_after_tab = mtab_bytes;
      *reserved += pl.lay_out(in, o, total_rows, max_frag_rows, (int64_t)16 << 30);
      return MI355Q_OK;
    }
    RouteScope rs(in->device_id, o.stream);
    if (rs.status) return rs.status;
    PassLoop pl(rs.ctx.maskws, nc, 1, &mask_width, &mp);
    pl.mask_column = true;
    pl.bytes_after_tab = mtab_bytes;
    pl.alloc_failed = MI355Q_ERR_OUT_OF_GPU_MEM;
    if (int32_t e = pl.prepare(in, o, total_rows, max_frag_rows)) return e;
    *reserved += rs.ctx.maskws.bytes;
    return MI355Q_OK;
  }
  RouteScope rs(in->device_id, o.stream);
  if (rs.status) return rs.status;
  const int n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);
  hipStream_t s = rs.s;
  // one pass of fragments = as many as the mask region holds (1 B/row: 16 GB of it cover 16 G rows)
  PassLoop pl(rs.ctx.maskws, nc, 1, &mask_width, &mp);
  pl.mask_column = true;
  pl.bytes_after_tab = mtab_bytes;
  pl.alloc_failed = MI355Q_ERR_OUT_OF_GPU_MEM;
  pl.clear_err_word = false;  // (the probe raises nothing)
  if (int32_t e = pl.prepare(&in_outer, o, total_rows, max_frag_rows)) return e;
  int8_t** d_mtab = (int8_t**)pl.after_tab;
  std::vector<const void*> masks((size_t)nf);
  if (int32_t e = pl.run(rs, &in_outer, o, report, [&](int f, int pnf) -> int32_t {
        int64_t prows = 0, pmax = 0;
        for (int i = 0; i < pnf; ++i) {
          masks[(size_t)i] = pl.cols2[(size_t)i * nc2 + mask_col];
          prows += in->num_rows[f + i];
          pmax = std::max(pmax, in->num_rows[f + i]);
        }
        HIP_TRY(hipMemcpyAsync(d_mtab, masks.data(), sizeof(void*) * (size_t)pnf, hipMemcpyHostToDevice, s));
        FragView fv{pl.d_tab, pl.d_rows + f, in->col_buffers + (size_t)f * nc, in->num_rows + f, pnf, nc, prows, pmax};
        HIP_TRY(launch_join_exists_mask(d, anti, fv, d_mtab, n_cus, s));
        HIP_TRY(hipStreamSynchronize(s));  // (masks / cols2 are re-used by the next pass)
        return MI355Q_OK;
      }))
    return e;
  if (int32_t e = rs.finish_sync_if_timed(report, pl.acc, *plan, *in, total_rows)) return e;
  *out = pl.res.release();
  return MI355Q_OK;
}

// ------------------------------------------------------------------------------- the compiled-filter stages
// A filter of comparisons with literals under AND / OR / NOT is compiled into atoms + a truth table and evaluated by
// the consuming kernel on the values it holds in registers (boolfilter.h): no temporary column, no second pass.
namespace {

struct BfScope {  // the compiled filter travels beside the plan for the duration of one inner step
  BfScope(const BoolFilter* host, const BoolFilter* dev) { set_step_bool_filter(host, dev); }
  ~BfScope() { set_step_bool_filter(nullptr, nullptr); }
};

// atoms (and the few lean programs the LDS members evaluate themselves) inside the consuming family: the filter goes to
// ctx.bf_table and `rest` runs with it beside the plan; kNotTaken when no family that takes a filter takes the step
int32_t execute_fused_filter(const mi355q_plan& rest, const BoolFilterHost& bfh, const mi355q_inputs* in, const mi355q_exec_options& o,
                             mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  DeviceGuard gb(in->device_id);
  DeviceCtx& cb = ctx_of(in->device_id);
  std::lock_guard<std::recursive_mutex> lb(cb.mu);
  bool have = true;
  if (!t_plan_only) {
    if (!cb.bf_table) have = gb.ok && hipMalloc(&cb.bf_table, sizeof(BoolFilter)) == hipSuccess;
    // (a synchronous copy out of this frame: atoms + truth table, 1.2 KB)
    have = have && hipMemcpy(cb.bf_table, &bfh.bf, sizeof(BoolFilter), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!have) {
    (void)hipGetLastError();
    return kNotTaken;
  }
  BfScope scope(&bfh.bf, (const BoolFilter*)cb.bf_table);
  route_note("filter compiled (atoms + truth table)");
  return execute_impl(&rest, in, &o, out, report, nullptr, reserved);
}

}  // namespace

// the filter of an aggregate step with expressions: fused into the consuming family where one takes it, else — program
// atoms no family evaluates itself — the row-mask pre-pass, then `mask = 1`
int32_t execute_compiled_filter(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  BoolFilterHost bfh;
  mi355q_plan rest;
  if (!compile_bool_filter(*plan, &bfh, &rest)) return kNotTaken;
  int32_t e = kNotTaken;
  const bool fused_progs = bfh.bf.n_progs == 0 || (bfh.bf.all_lean && bfh.bf.all_i32 && bfh.bf.n_progs <= kLdsFusedProgs &&
                                                   !(o.flags & MI355Q_OPT_FILTER_PREPASS));
  if (fused_progs) e = try_route(out, [&] { return execute_fused_filter(rest, bfh, in, o, out, report, reserved); });
  if (e == kNotTaken && bfh.bf.n_progs != 0)
    e = try_route(out, [&] {
      route_note("filter compiled (atoms + programs + truth table)");
      return execute_masked(plan, rest, bfh, in, o, out, report, reserved);
    });
  if (e == MI355Q_OK && report && !reserved) report->algorithmic_bytes = algorithmic_bytes(*plan, *in);
  return e;
}

// a Projection whose expressions all belong to the FILTER (`SELECT a, b FROM t WHERE x + y > 100`): the filter is compiled,
// the row-mask pre-pass evaluates it, the Projection runs on `mask = 1` — in its fast member where the targets allow —
// instead of evaluating the quals' expressions row by row in the general member.  With a LIMIT only where the filter
// cannot raise: the pre-pass looks at every row, the reference's loop stops at the limit.
int32_t execute_projection_filter(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                  mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  BoolFilterHost bfh;
  mi355q_plan rest;
  if (!compile_bool_filter(*plan, &bfh, &rest) || (bfh.bf.any_raise && plan->scan_limit != 0)) return kNotTaken;
  return try_route(out, [&] {
    route_note("filter compiled (atoms + programs + truth table)");
    return execute_masked(plan, rest, bfh, in, o, out, report, reserved);
  });
}

// SEVERAL plain quals in front of a family that filters on one column (the partitioned GROUP BY, the perfect-hash LDS
// member, the index-partitioned family takes none): instead of the row kernel, the quals become the range atoms of a
// compiled filter, the row-mask pre-pass evaluates them (k_filter_mask: one byte per row) and the step runs on
// `mask = 1` — measured in round 6: `a < K AND b > L` over 10 M INT64 groups went to k_generic at 55 ms per 1 B rows
int32_t execute_compiled_quals(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                               mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  BoolFilterHost bfh;
  mi355q_plan rest;
  if (!compile_bool_filter(*plan, &bfh, &rest)) return kNotTaken;
  return try_route(out, [&] {
    route_note("quals compiled (range atoms + truth table)");
    return execute_masked(plan, rest, bfh, in, o, out, report, reserved);
  });
}

// ------------------------------------------------------------------------------- the layout twins
// Columnar output: the step runs on the row-wise form of the same decisions (same entry count, 8-byte key components,
// same hash, same slots) into a library-owned table, and the finished table is moved column by column into the
// caller-visible buffer.
// Known oddity, kept as it was in execute_impl: unlike every other route this one takes neither the context lock nor
// the context's stream — the inner step locks for itself, and store_row_twin runs on the CALLER's stream, the null
// stream where the caller gave none.
int32_t execute_columnar_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                              mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  mi355q_plan pr = *plan;
  pr.output_columnar_hint = MI355Q_OUTPUT_ROWWISE_COLUMNAR_DECISIONS;
  mi355q_exec_options orw = o;
  orw.out_buffer = nullptr;
  if (reserved) {
    route_note("row-wise twin + k_rows_to_columns");
    return execute_impl(&pr, in, &orw, out, report, nullptr, reserved);
  }
  RowTwin t;
  if (int32_t e = mi355q_execute(&pr, in, &orw, &t.tw, report)) return e;
  const mi355q_qmd& qr = t.tw->qmd;
  if (qr.entry_count != q.entry_count || qr.row_size != q.row_size || qr.key_bytes != q.key_bytes ||
      qr.slot_count != q.slot_count || qr.slot_width != q.slot_width || qr.output_columnar)
    return MI355Q_ERR_UNSUPPORTED;
  mi355q_result* rc = nullptr;
  if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &rc)) return e;
  if (int32_t e = store_row_twin(t, rc, (hipStream_t)o.stream)) {
    mi355q_result_free(rc);
    return e;
  }
  *out = rc;
  return MI355Q_OK;
}

// Compact layout (4-byte slots): the step runs on the 8-byte layout of the same plan — same entry count, same key
// bytes, same hash — into ctx.wide, and the finished table is narrowed row by row.
int32_t execute_wide_slot_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                               mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  int64_t rows = 0;
  for (int f = 0; f < in->n_frags; ++f) rows += in->num_rows[f];
  if (rows > (int64_t)UINT32_MAX) return MI355Q_ERR_INVALID_PLAN;  // a 32-bit COUNT would wrap
  mi355q_plan p8 = *plan;
  p8.bigint_count = 1;  // pick_target_compact_width: g_bigint_count -> 8-byte slots
  mi355q_qmd q8;
  if (int32_t e = qmd_init(p8, &q8)) return e;
  if (q8.slot_width != 8 || q8.entry_count != q.entry_count || q8.key_bytes != q.key_bytes ||
      q8.slot_count != q.slot_count)
    return MI355Q_ERR_UNSUPPORTED;
  if (reserved) {
    route_note("8-byte-slot twin + k_narrow_slots");
    return execute_impl(&p8, in, &o, out, report, nullptr, reserved);
  }
  DeviceCtx& ctx = ctx_of(in->device_id);
  std::lock_guard<std::recursive_mutex> ctx_lock(ctx.mu);
  if (const hipError_t he = ctx.wide.grow(q8.entry_count * (int64_t)q8.row_size)) {
    last_hip_error = he;
    return MI355Q_ERR_OUT_OF_GPU_MEM;
  }
  hipStream_t s4 = nullptr;
  if (int32_t e = launch_stream(ctx, o.stream, &s4)) return e;
  mi355q_exec_options o8 = o;
  o8.stream = s4;
  o8.out_buffer = ctx.wide.p;
  mi355q_result* r8 = nullptr;
  if (int32_t e = mi355q_execute(&p8, in, &o8, &r8, report)) return e;
  mi355q_result_free(r8);
  mi355q_result* res4 = nullptr;
  if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &res4)) return e;
  hipError_t he = launch_narrow_slots((const int64_t*)ctx.wide.p, q8.row_size / 8, q.key_bytes / 8, q.slot_count,
                                      q.row_size / 8, q.entry_count, res4->buf, s4);
  if (he == hipSuccess) he = hipStreamSynchronize(s4);
  if (he != hipSuccess) {
    last_hip_error = he;
    mi355q_result_free(res4);
    return MI355Q_ERR_HIP;
  }
  *out = res4;
  return MI355Q_OK;
}

// An INNER join on ONE key against a dense OneToOne perfect table (mi355q_join_table::dense) whose inner side no target reads:
// a row has a match exactly when its key lies in [min, max] (hash_join_idx, GroupByRuntime.cpp:287-297: in range ->
// the slot, and no slot of a dense table is -1; a NULL key matches nothing, hash_join_idx_nullable :311-318), so the step is
// the same step WITHOUT the join and with the two range quals on the key column — a plain scan for the non-grouped
// shapes (BASELINE cfg4, Query A on the dense dimension).  kNotTaken for everything else.
int32_t execute_dense_join_as_filter(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                     mi355q_result** out, mi355q_exec_report* report, int64_t* reserved) {
  const mi355q_join_table* jt = plan->join_table;
  if (plan->join_outer_col < 0 || !jt || !jt->dense || plan->join_kind != MI355Q_JOIN_INNER || plan->n_join_cols > 1 ||
      plan->n_exprs != 0 || plan->n_quals + 2 > MI355Q_MAX_QUALS || o.force_generic || o.kernel_variant != 0)
    return kNotTaken;
  for (int t = 0; t < plan->n_targets && t < MI355Q_MAX_TARGETS; ++t)
    if (plan->targets[t].table != 0 && plan->targets[t].agg != MI355Q_PROJECT_KEY) return kNotTaken;
  const int kc = plan->join_outer_col;
  if (kc >= plan->n_cols || col_type_code(plan->cols[kc]) < 0) return kNotTaken;
  const int lt = tc_logical(col_type_code(plan->cols[kc]));
  if (lt < MI355Q_INT8 || lt > MI355Q_INT64) return kNotTaken;
  mi355q_plan p2 = *plan;
  p2.join_outer_col = -1;
  p2.join_table = nullptr;
  p2.n_join_cols = 0;
  p2.n_inner_cols = 0;
  p2.quals[p2.n_quals++] = mi355q_qual{kc, MI355Q_GE, jt->min_key, 0.0};
  p2.quals[p2.n_quals++] = mi355q_qual{kc, MI355Q_LE, jt->max_key, 0.0};
  mi355q_qmd qa, qb;   // the layout does not look at the join or at the quals: the derived step's result IS the step's
  if (qmd_init(*plan, &qa) || qmd_init(p2, &qb) || std::memcmp(&qa, &qb, sizeof(qa)) != 0) return kNotTaken;
  route_note("join on a dense one-to-one table = range filter on the key");
  mi355q_inputs in2 = *in;
  in2.inner_col_buffers = nullptr;
  in2.inner_num_rows = 0;
  return execute_impl(&p2, &in2, &o, out, report, nullptr, reserved);
}
}  // namespace api
}  // namespace mq
