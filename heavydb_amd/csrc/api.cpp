// api.cpp — the C-ABI entry points of libmi355q (include/mi355q.h) and the step executor: host C++ that turns a plan
// into a launch sequence over the HIP kernel family (execute_impl: the route order, the plain step, its finish and the
// asynchronous tail).  The derived-plan routes it asks first live in api_routes.cpp.  No torch, no JIT, no CUDA-compat layer.
//
// Shape of one call, against the reference's step executor (heavyai/heavydb):
//   mi355q_execute ~ Executor::executeWorkUnit (Execute.cpp:2144) after fetchChunks:
//     plan -> QueryMemoryDescriptor mirror (plan.cpp) -> output buffer init (K6/K7 analogue,
//     QueryMemoryInitializer.cpp:1144) -> kernel family member chosen at plan time ->
//     error code folded from one device word (QueryExecutionContext.cpp:366 copies one int32
//     per thread; we keep a single word).
// The result stays in HBM; nothing is copied to the host unless the caller asks.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <new>
#include <vector>

#include "api_internal.h"
#include "boolfilter.h"

using namespace mq;

namespace mq {
namespace api {
thread_local std::string* t_route = nullptr;
thread_local bool t_plan_only = false;
void route_note(const char* what) {
  if (!t_route) return;
  if (!t_route->empty()) *t_route += " > ";
  *t_route += what;
}

thread_local hipError_t last_hip_error = hipSuccess;

int cu_count_of(int dev) {
  static std::mutex mu;
  static int cache[64];
  std::lock_guard<std::mutex> lk(mu);
  if (dev < 0 || dev >= 64) return 256;
  if (!cache[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    cache[dev] = v;
  }
  return cache[dev];
}

DeviceCtx& ctx_of(int dev) {
  static DeviceCtx ctxs[64];
  return ctxs[dev < 0 ? 0 : dev % 64];
}

}  // namespace api
}  // namespace mq
using namespace mq::api;

namespace {

// MI355Q_OPT_TRACE: host-side wall-clock marks of one execute call on stderr
struct Trace {
  bool on;
  std::chrono::steady_clock::time_point t0;
  explicit Trace(bool enabled) : on(enabled), t0(std::chrono::steady_clock::now()) {}
  void mark(const char* what) {
    if (!on) return;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[mi355q] %8.3f ms  %s\n", ms, what);
  }
};


void drain_inflight(DeviceCtx& ctx);  // finishes the step mi355q_execute_async left in flight (defined with finish_step)

}  // namespace

int32_t mq::api::attach_join(const mi355q_plan& p, const mi355q_inputs* in, DevPlan* d) {
  if (p.join_outer_col < 0) return MI355Q_OK;
  if (!p.join_table) return MI355Q_ERR_INVALID_PLAN;
  const mi355q_join_table* jt = p.join_table;
  const int n_keys = p.n_join_cols > 1 ? p.n_join_cols : 1;
  if (n_keys > MI355Q_MAX_GROUP_COLS || n_keys != jt->n_keys) return MI355Q_ERR_INVALID_PLAN;
  // (SEMI / ANTI never get here as such: execute_exists_join hands over a carrier plan of kind INNER for the probe alone)
  if (p.join_kind != MI355Q_JOIN_INNER && p.join_kind != MI355Q_JOIN_LEFT) return MI355Q_ERR_UNSUPPORTED;
  for (int i = 0; i < n_keys; ++i) {
    const int c = (i == 0 && p.n_join_cols <= 1) ? p.join_outer_col : p.join_outer_cols[i];
    if (c < 0 || c >= p.n_cols) return MI355Q_ERR_INVALID_PLAN;
    const mi355q_col_desc& jc = p.cols[c];
    if (type_is_fp(jc.type) || type_is_f32(jc.type)) return MI355Q_ERR_UNSUPPORTED;
    d->join_cols[i] = c;
    d->join_types[i] = col_type_code(jc);
    d->join_nullables[i] = jc.nullable != 0;
  }
  d->join_col = d->join_cols[0];
  d->join_type = d->join_types[0];
  d->join_nullable = d->join_nullables[0];
  d->join_n_keys = n_keys;
  d->join_width = jt->width;
  d->join_kind = p.join_kind;
  d->join_hash_type = jt->hash_type;
  d->join_buf = jt->buf;
  d->join_bitmap = (const uint32_t*)jt->bitmap;
  d->join_min = jt->min_key;
  d->join_max = jt->max_key;
  d->join_entries = jt->entry_count;
  for (int i = 0; i < p.n_inner_cols; ++i) {
    d->inner_cols[i] = in && in->inner_col_buffers ? (const int8_t*)in->inner_col_buffers[i] : nullptr;
  }
  for (int i = 0; i < p.n_targets; ++i) {
    // (an empty inner table has no chunks: nothing can match, the pointers are never followed)
    if (d->targets[i].table == 1 && d->targets[i].col >= 0 && !d->inner_cols[d->targets[i].col] &&
        in && in->inner_num_rows > 0)
      return MI355Q_ERR_INVALID_PLAN;
  }
  return MI355Q_OK;
}

int64_t mq::api::algorithmic_bytes(const mi355q_plan& p, const mi355q_inputs& in) {
  // every distinct outer column the plan touches is read once per row
  bool used[MI355Q_MAX_COLS] = {false};
  for (int k = 0; k < p.n_exprs && k < MI355Q_MAX_EXPRS; ++k)  // an expression reads its operand columns
    for (int i = 0; i < p.exprs[k].n_nodes && i < MI355Q_MAX_EXPR_NODES; ++i)
      if (p.exprs[k].nodes[i].op == MI355Q_EX_COL && p.exprs[k].nodes[i].arg >= 0 && p.exprs[k].nodes[i].arg < p.n_cols)
        used[p.exprs[k].nodes[i].arg] = true;
  // (an inner reference of the stated plan of a star join, execute_inner_refs' report: no outer column's bytes)
  for (int i = 0; i < p.n_quals; ++i)
    if (!MI355Q_IS_INNER_COL(p.quals[i].col)) used[p.quals[i].col] = true;
  for (int g = 0; g < p.n_group_cols; ++g)
    if (!MI355Q_IS_INNER_COL(p.group_cols[g])) used[p.group_cols[g]] = true;
  if (p.join_outer_col >= 0) {
    used[p.join_outer_col] = true;
    for (int i = 1; i < p.n_join_cols && i < MI355Q_MAX_GROUP_COLS; ++i) used[p.join_outer_cols[i]] = true;
  }
  for (int i = 0; i < p.n_targets; ++i) {
    if (p.targets[i].table == 0 && p.targets[i].col >= 0 && p.targets[i].agg != MI355Q_PROJECT_KEY)
      used[p.targets[i].col] = true;
    if (p.targets[i].agg == MI355Q_COUNT_IF || p.targets[i].agg == MI355Q_SUM_IF) used[p.targets[i].cond.col] = true;
  }
  int64_t per_row = 0;
  for (int c = 0; c < p.n_cols; ++c) {  // physical columns only (indices >= n_cols are expressions)
    if (used[c]) per_row += type_width(p.cols[c].type);
  }
  int64_t rows = 0;
  for (int f = 0; f < in.n_frags; ++f) rows += in.num_rows[f];
  return per_row * rows;
}


extern "C" {

int32_t mi355q_abi_version(void) { return MI355Q_ABI_VERSION; }

int64_t mi355q_abi_sizeof(int32_t which) {
  switch (which) {
    case 1: return sizeof(mi355q_plan);
    case 2: return sizeof(mi355q_qmd);
    case 3: return sizeof(mi355q_inputs);
    case 4: return sizeof(mi355q_exec_options);
    case 5: return sizeof(mi355q_exec_report);
    case 6: return sizeof(mi355q_join_spec);
    default: return -1;
  }
}

const char* mi355q_error_string(int32_t code) {
  if (code < 0) return "ran out of group slots (negative row position): resize and retry";
  switch (code) {
    case MI355Q_OK: return "No Error";
    case MI355Q_ERR_DIV_BY_ZERO: return "Division by zero";
    case MI355Q_ERR_OUT_OF_GPU_MEM: return "Out of GPU memory";
    case MI355Q_ERR_OUT_OF_SLOTS: return "Out of Slots";
    case MI355Q_ERR_OUT_OF_CPU_MEM: return "Not enough host memory to execute the query";
    case MI355Q_ERR_OVERFLOW_OR_UNDERFLOW: return "Overflow or underflow";
    case MI355Q_ERR_OUT_OF_TIME: return "Query execution has exceeded the time limit";
    case MI355Q_ERR_INTERRUPTED: return "Query execution has been interrupted";
    case MI355Q_ERR_INVALID_PLAN: return "Invalid plan";
    case MI355Q_ERR_UNSUPPORTED: return "Plan shape not supported by this kernel family";
    case MI355Q_ERR_HIP: return hipGetErrorString(last_hip_error);
    case MI355Q_ERR_JOIN_NOT_ONE_TO_ONE: return "Join key column is not unique (one-to-many)";
    case MI355Q_ERR_JOIN_TABLE_FULL: return "Keyed join hash table is full";
    case MI355Q_STEP_RECOMPUTED: return "Step re-run inside mi355q_wait: redo what was enqueued behind it";
    default: return "Unknown error";
  }
}

int32_t mi355q_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t mi355q_device_info(int32_t device_id, char* name, int32_t* cu_count, int64_t* total_mem,
                           int64_t* free_mem, int32_t* mem_clock_khz, int32_t* mem_bus_width) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  if (name) {
    std::snprintf(name, 256, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (cu_count) *cu_count = prop.multiProcessorCount;
  if (mem_clock_khz) *mem_clock_khz = prop.memoryClockRate;
  if (mem_bus_width) *mem_bus_width = prop.memoryBusWidth;
  DeviceGuard g(device_id);
  size_t fr = 0, tot = 0;
  HIP_TRY(hipMemGetInfo(&fr, &tot));
  if (total_mem) *total_mem = (int64_t)tot;
  if (free_mem) *free_mem = (int64_t)fr;
  return MI355Q_OK;
}

int32_t mi355q_release_workspace(int32_t device_id) {
  DeviceCtx& ctx = ctx_of(device_id);
  std::lock_guard<std::recursive_mutex> lk(ctx.mu);
  DeviceGuard g(device_id);
  if (!g.ok) return MI355Q_ERR_HIP;
  // a step left in flight by mi355q_execute_async still points into the workspace (error words, column table,
  // events, the launch stream): finish it before anything is freed
  drain_inflight(ctx);
  ctx.scratch.release();
  if (ctx.meta) (void)hipFree(ctx.meta);
  ctx.meta = nullptr;
  ctx.meta_bytes = 0;
  if (ctx.h_meta) (void)hipHostFree(ctx.h_meta);
  ctx.h_meta = nullptr;
  ctx.aux.release();
  ctx.wide.release();
  ctx.proj.release();
  ctx.gather.release();
  ctx.star.release();
  ctx.lattice.release();
  if (ctx.bf_table) (void)hipFree(ctx.bf_table);
  ctx.bf_table = nullptr;
  ctx.maskws.release();
  ctx.projws.release();
  if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
  ctx.stream = nullptr;
  for (hipEvent_t e : ctx.events) (void)hipEventDestroy(e);
  ctx.events.clear();
  return MI355Q_OK;
}

int32_t mi355q_qmd_init(const mi355q_plan* plan, mi355q_qmd* out) {
  if (!plan || !out) return MI355Q_ERR_INVALID_PLAN;
  return qmd_init(*plan, out);
}

int64_t mi355q_qmd_buffer_bytes(const mi355q_qmd* qmd) { return qmd ? qmd_buffer_bytes(*qmd) : 0; }
int64_t mi355q_qmd_group_col_offset(const mi355q_qmd* qmd, int32_t g) { return qmd ? qmd_group_col_offset(*qmd, g) : -1; }
int64_t mi355q_qmd_slot_col_offset(const mi355q_qmd* qmd, int32_t s) {
  return qmd && s < qmd->slot_count ? qmd_slot_col_offset(*qmd, s) : -1;
}

}  // extern "C"

namespace {

constexpr int32_t kRetryNoIdx = INT32_MIN + 9;  // internal: the index-partitioned family gave up (spill list), plan again without it
constexpr int32_t kRetryNoLds = INT32_MIN + 8;  // internal: the LDS group-by ran out of replica room, plan again without it

// ---------------------------------------------------------------------------------------------------
// The part of a step that needs the host to look at the device: error words, the spill counter, the
// re-run with the direct member when the partitioned family gave up, the report.  mi355q_execute runs it
// right after the launches; mi355q_execute_async parks it in a mi355q_pending until mi355q_wait (or the
// next call on the device) runs it.  Everything it touches is owned here: the caller's host arrays may be
// gone by then.
enum StepKind { K_GENERIC, K_SCAN_COUNT, K_PERFECT_LDS, K_BASELINE_FAST, K_JOIN_SUM, K_JOIN_PART, K_JOIN_PROBE, K_SCAN_AGG, K_LDS_GROUPBY, K_IDX_PART };

// the family as mi355q_explain names it (the partitioned GROUP BY by the member its plan picks)
const char* family_name(StepKind kind, const DevPlan& d, const FragView& fv, int kernel_variant, int n_cus) {
  switch (kind) {
    case K_SCAN_COUNT: return "k_scan_count";
    case K_SCAN_AGG: return "k_scan_agg";
    case K_PERFECT_LDS: return "k_perfect_lds";
    case K_LDS_GROUPBY: return "k_groupby_lds";
    case K_JOIN_SUM: return "k_join_sum";
    case K_JOIN_PART: return "k_part_scatter + k_part_join";
    case K_JOIN_PROBE: return "k_part_scatter + k_part_probe";
    case K_IDX_PART: return "k_idx_scatter + k_idx_aggregate";
    case K_BASELINE_FAST:
      return fv.n_frags > 0 && baseline_fast_variant(d, fv, kernel_variant, n_cus) == 2 ? "k_part_scatter + k_part_aggregate" : "k_baseline_direct";
    default: return "k_generic";
  }
}

struct TailState {
  mi355q_qmd q;
  DevPlan d;
  StepKind kind;
  LaunchStats st;
  mi355q_result* res;
  int32_t* d_err;
  const int8_t* const* d_cols;
  const int64_t* d_rows;
  std::vector<const void*> h_cols;
  std::vector<int64_t> h_rows;
  int nf, nc, n_cus;
  int64_t total_rows, max_frag_rows, alg_bytes;
  hipStream_t s;
  hipEvent_t ev_start, ev_stop;
  hipEvent_t* ev_pool;
  bool trace;
  int32_t* h_ret = nullptr; // 64 pinned bytes the error words (+ the spill counter's copy, word 4) are read back into
  TuneKnobs knobs;          // the knobs the step was planned with: a re-run in mi355q_wait (another thread, another
                            // call's knobs in between) must plan with the same ones
  int32_t* h_ret_dev = nullptr;  // the device's address of h_ret
  bool err_words_zero = false;   // the step left the error words as the upload laid them down
  bool recomputed = false;  // finish_step re-ran the step into res->buf after the first launches had completed
};

struct KnobScope {  // the thread's knobs for the duration of finish_step
  TuneKnobs saved;
  explicit KnobScope(const TuneKnobs& k) : saved(tune_knobs()) { set_tune_knobs(k); }
  ~KnobScope() { set_tune_knobs(saved); }
};

// a partitioned member ran out of spill space (extreme skew): the step again, into the same table, with the member
// `launch` enqueues — error words cleared, table initialised, launched, the words read back, synchronised
template <class Launch>
int32_t redo_step(TailState& t, int32_t (&h_err)[2], Launch&& launch) {
  HIP_TRY(hipMemsetAsync(t.d_err, 0, 64, t.s));
  HIP_TRY(launch_init_buffer(t.res->buf, t.q.entry_count, make_row_init(t.q), t.s));
  HIP_TRY(launch());
  HIP_TRY(hipMemcpyAsync(h_err, t.d_err, sizeof(h_err), hipMemcpyDeviceToHost, t.s));
  HIP_TRY(hipStreamSynchronize(t.s));
  return MI355Q_OK;
}

int32_t finish_step(TailState& t, mi355q_exec_report* report) {
  KnobScope knob_scope(t.knobs);
  hipStream_t s = t.s;
  LaunchStats& st = t.st;
  const mi355q_qmd& q = t.q;
  const DevPlan& d = t.d;
  FragView fv{t.d_cols, t.d_rows, t.h_cols.data(), t.h_rows.data(), t.nf, t.nc, t.total_rows, t.max_frag_rows};
  int32_t h_err[2] = {0, 0};
  uint32_t h_spills = 0;
  if (t.h_ret && (!st.spill_counter32 || st.spill_counter32 == (uint32_t*)(t.d_err + 4))) {
    // error words and the spill counter's copy (word 4) in one read into pinned memory: written there by a one-wave kernel
    // behind the step's kernels (a copy command costs a DMA round trip more than a launch)
    if (t.h_ret_dev) HIP_TRY(launch_words_to_host(t.d_err, t.h_ret_dev, 8, s));
    else HIP_TRY(hipMemcpyAsync(t.h_ret, t.d_err, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h_err[0] = t.h_ret[0];
    h_err[1] = t.h_ret[1];
    if (st.spill_counter32) h_spills = (uint32_t)t.h_ret[4];
    t.err_words_zero = true;
    for (int w = 0; w < 8; ++w) t.err_words_zero = t.err_words_zero && t.h_ret[w] == 0;
  } else {
    HIP_TRY(hipMemcpyAsync(h_err, t.d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    if (st.spill_counter32) {
      HIP_TRY(hipMemcpyAsync(&h_spills, st.spill_counter32, sizeof(h_spills), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
  }
  st.spilled_rows = (int64_t)h_spills;
  if (h_err[1] && (t.kind == K_JOIN_PART || t.kind == K_JOIN_PROBE || t.kind == K_BASELINE_FAST)) t.recomputed = true;
  if (h_err[1] && t.trace) std::fprintf(stderr, "[mi355q] partitioned family gave up (code %d, spills %u): re-running with the direct kernel\n", h_err[1], h_spills);
  // more groups than an LDS replica holds (a baseline table: the group count is only known now): the caller plans
  // the step again without that member (packed route / partitioned family / row kernel, whatever applies)
  if (h_err[1] && t.kind == K_LDS_GROUPBY) return kRetryNoLds;
  if (h_err[1] && t.kind == K_IDX_PART) return kRetryNoIdx;
  if (h_err[1] && t.kind == K_JOIN_PART) {  // the partitioned probe: redo with the direct probe
    if (int32_t e = redo_step(t, h_err, [&] { return launch_join_sum(d, fv, t.res->buf, t.n_cus, s, &st); })) return e;
  } else if (h_err[1] && t.kind == K_JOIN_PROBE) {  // the payload probe: redo with the row kernel, which the report then names
    if (int32_t e = redo_step(t, h_err, [&] {
          const hipError_t he = launch_generic(d, q.idx_target_as_key, make_row_init(q), t.d_cols, t.d_rows, t.nf, t.max_frag_rows,
                                               t.res->buf, t.d_err, t.n_cus, s);
          if (he == hipSuccess) st.kernel_name = "k_generic";
          return he;
        }))
      return e;
  } else if (h_err[1] && t.kind == K_BASELINE_FAST) {  // the partitioned GROUP BY: redo with the direct-atomic member of the same family
    if (int32_t e = redo_step(t, h_err, [&] { return launch_baseline_fast(d, fv, t.res->buf, t.d_err, nullptr, 0, 0, 1, t.n_cus, s, &st); }))
      return e;
  }
  if (report) {
    std::memset(report, 0, sizeof(*report));
    std::snprintf(report->kernel_name, sizeof(report->kernel_name), "%s", st.kernel_name ? st.kernel_name : "");
    if (t.ev_start) (void)hipEventElapsedTime(&report->total_ms, t.ev_start, t.ev_stop);
    if (st.n_events_used > 0) {
      float acc = 0.f;
      for (int i = 0; i + 1 < st.n_events_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.ev_pool[i], t.ev_pool[i + 1]) == hipSuccess) acc += ms;
      }
      report->kernel_ms = acc;
    } else if (st.n_launches > 0 && t.nf > 0) {
      if (hipEventElapsedTime(&report->kernel_ms, st.k_start, st.k_stop) != hipSuccess) report->kernel_ms = 0.f;
    }
    if (!t.ev_start) report->total_ms = report->kernel_ms;  // (a one-kernel scan step: execute_impl)
    report->n_launches = st.n_launches;
    report->variant = st.variant;
    report->rows_scanned = t.total_rows;
    report->algorithmic_bytes = t.alg_bytes;
    report->spilled_rows = st.spilled_rows;
  }
  return h_err[0];
}

}  // namespace

struct mi355q_pending {
  TailState* tail = nullptr;  // null once the step has been finished
  int device_id = 0;
  int32_t code = MI355Q_OK;
  mi355q_exec_report rep{};
};

namespace {

// finishes the step a previous mi355q_execute_async left in flight on this device (ctx.mu held)
void drain_inflight(DeviceCtx& ctx) {
  mi355q_pending* p = ctx.inflight;
  if (!p) return;
  ctx.inflight = nullptr;
  if (p->tail) {
    p->code = finish_step(*p->tail, &p->rep);
    // the step was re-run after the call had returned: a consumer enqueued behind the first launches (pads, slices,
    // a collective) worked on the table the abandoned attempt left — tell the caller to redo it
    if (p->code == MI355Q_OK && p->tail->recomputed) p->code = MI355Q_STEP_RECOMPUTED;
    // the asynchronous call never selects the members that can ask for another plan (execute_impl: `!pend`), and the
    // result has been handed out, so planning again is not possible here: an internal code must not reach the caller
    if (p->code == kRetryNoLds || p->code == kRetryNoIdx || p->code == kNotTaken) p->code = MI355Q_ERR_UNSUPPORTED;
    delete p->tail;
    p->tail = nullptr;
  }
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------- execute
int32_t mi355q_execute(const mi355q_plan* plan, const mi355q_inputs* in,
                       const mi355q_exec_options* opts, mi355q_result** out,
                       mi355q_exec_report* report) {
  return execute_impl(plan, in, opts, out, report, nullptr);
}

}  // extern "C"

namespace {

// mi355q_reserve_workspace / mi355q_explain: the step planned in RESERVE mode.  The planner looks at the pointer table
// for alignment only: a table of NULLs stands in for it (16-byte aligned chunks assumed)
int32_t plan_without_columns(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options* opts, int64_t* bytes) {
  std::vector<const void*> none((size_t)std::max(1, in->n_frags * std::max(plan->n_cols + plan->n_exprs + 1, 1)), nullptr);  // (+ 1: the row mask of a compiled filter, execute_masked)
  mi355q_inputs in2 = *in;
  in2.col_buffers = none.data();
  mi355q_result* r = nullptr;
  const int32_t e = execute_impl(plan, &in2, opts, &r, nullptr, nullptr, bytes);
  if (r) mi355q_result_free(r);
  return e;
}

struct ExplainScope {  // the thread plans only and writes its route down, for the duration of mi355q_explain
  explicit ExplainScope(std::string* text) {
    t_route = text;
    t_plan_only = true;
  }
  ~ExplainScope() {
    t_route = nullptr;
    t_plan_only = false;
  }
};

}  // namespace

extern "C" {

int32_t mi355q_reserve_workspace(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options* opts,
                                 int64_t* reserved_bytes) {
  if (!plan || !in) return MI355Q_ERR_INVALID_PLAN;
  int64_t bytes = 0;
  const int32_t e = plan_without_columns(plan, in, opts, &bytes);
  if (reserved_bytes) *reserved_bytes = bytes;
  return e;
}

// EXPLAIN for one step: the route mi355q_execute would take for this plan over inputs of this shape (fragment row
// counts; the pointer table is not looked at: 16-byte aligned chunks are assumed), as a " > "-separated chain of
// the derived-plan stages and the kernel family that runs the step, e.g.
//   "k_project > k_pack_keys (entry index, baseline temp) > k_part_scatter + k_part_aggregate > k_unpack_emit".
// Nothing is launched and no workspace is allocated; *scratch_bytes = the partition scratch the step would ask for.
int32_t mi355q_explain(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options* opts, char* route,
                       int64_t route_len, int64_t* scratch_bytes) {
  if (!plan || !in || (route_len > 0 && !route)) return MI355Q_ERR_INVALID_PLAN;
  int64_t bytes = 0;
  std::string text;
  int32_t e;
  try {
    ExplainScope scope(&text);
    e = plan_without_columns(plan, in, opts, &bytes);
  } catch (...) {
    return MI355Q_ERR_OUT_OF_CPU_MEM;
  }
  if (route && route_len > 0) std::snprintf(route, (size_t)route_len, "%s", text.c_str());
  if (scratch_bytes) *scratch_bytes = bytes;
  return e;
}

// Stream-ordered form of mi355q_execute: every kernel of the step is enqueued on the stream and the call
// returns without waiting for the device.  *out is valid at once for STREAM-ORDERED use on the same stream
// (mi355q_shard_pads, a collective enqueued behind it, ...); whether the step succeeded — error code, the
// retry with the direct member after a spill overflow, the report — is only known after mi355q_wait.  One step
// per device may be in flight: the next call on the device finishes it first.  Routes that need the host in
// the middle of the step (projected expressions, packed multi-column keys, columnar / 4-byte-slot results,
// the first build of a join payload) run to completion inside this call; mi355q_wait then returns at once.
int32_t mi355q_execute_async(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options* opts,
                             mi355q_result** out, mi355q_pending** pending) {
  if (!pending) return MI355Q_ERR_INVALID_PLAN;
  *pending = nullptr;
  mi355q_pending* p = nullptr;
  mi355q_exec_report rep{};
  const int32_t e = execute_impl(plan, in, opts, out, &rep, &p);
  if (!p) {  // completed (or failed) synchronously
    if (e) return e;  // a failed call leaves no handle behind (*pending stays NULL)
    p = new (std::nothrow) mi355q_pending();
    if (!p) return e ? e : MI355Q_ERR_OUT_OF_CPU_MEM;
    p->device_id = in ? in->device_id : 0;
    p->code = e;
    p->rep = rep;
  }
  *pending = p;
  return p->tail ? MI355Q_OK : e;
}

int32_t mi355q_wait(mi355q_pending* p, mi355q_exec_report* report) {
  if (!p) return MI355Q_ERR_INVALID_PLAN;
  {
    DeviceCtx& ctx = ctx_of(p->device_id);
    std::lock_guard<std::recursive_mutex> lk(ctx.mu);
    if (ctx.inflight == p) {
      DeviceGuard g(p->device_id);
      drain_inflight(ctx);
    }
  }
  if (report) *report = p->rep;
  const int32_t code = p->code;
  delete p->tail;
  delete p;
  return code;
}

}  // extern "C"

int32_t mq::api::upload_frag_table(DeviceCtx& ctx, const mi355q_inputs& in, int nc, void* callers_stream, FragUpload mode,
                                   FragTable* ft) {
  const int nf = in.n_frags;
  const size_t ptr_bytes = sizeof(void*) * (size_t)std::max(1, nf * nc);
  const size_t rows_bytes = sizeof(int64_t) * (size_t)std::max(1, nf);
  const size_t tab_bytes = ptr_bytes + rows_bytes;
  const size_t meta_bytes = tab_bytes + 64;
  if (ctx.meta_bytes < meta_bytes) {
    if (ctx.meta) (void)hipFree(ctx.meta);
    ctx.meta = nullptr;
    ctx.meta_bytes = 0;
    if (ctx.h_meta) (void)hipHostFree(ctx.h_meta);
    ctx.h_meta = nullptr;
    ctx.h_ret_dev = nullptr;
    ctx.meta_shadow.clear();
    HIP_TRY(hipMalloc(&ctx.meta, meta_bytes * 2));
    HIP_TRY(hipHostMalloc((void**)&ctx.h_meta, meta_bytes * 2 + 64, hipHostMallocDefault));
    ctx.meta_bytes = meta_bytes * 2;
  }
  if (!ctx.h_ret_dev && ctx.h_meta) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, ctx.h_meta + ctx.meta_bytes, 0) == hipSuccess) ctx.h_ret_dev = (int32_t*)dp;
    else (void)hipGetLastError();
  }
  if (int32_t e = launch_stream(ctx, callers_stream, &ft->s)) return e;
  char* mp = (char*)ctx.meta;
  char* hm = ctx.h_meta;
  ft->d_cols = (const int8_t* const*)mp;
  ft->d_rows = (const int64_t*)(mp + ptr_bytes);
  ft->d_err = (int32_t*)(mp + tab_bytes);
  // the same table as the last upload, its error words untouched since: nothing to send
  const bool same = mode == FragUpload::kSkipUnchanged && nf > 0 && ctx.meta_err_clean && ctx.meta_shadow.size() == tab_bytes &&
                    !std::memcmp(ctx.meta_shadow.data(), in.col_buffers, sizeof(void*) * (size_t)(nf * nc)) &&
                    !std::memcmp(ctx.meta_shadow.data() + ptr_bytes, in.num_rows, sizeof(int64_t) * (size_t)nf);
  if (mode == FragUpload::kAlways) {
    ctx.meta_shadow.clear();
    ctx.meta_err_clean = false;
  }
  if (mode != FragUpload::kNone && !same) {
    // one copy out of pinned memory: column table | row counts | zeroed error words (the synchronous step of a 60 us scan
    // used to spend ~90 us on a memset and two copies out of pageable memory, each staged by the driver)
    if (nf > 0) {
      std::memcpy(hm, in.col_buffers, sizeof(void*) * (size_t)(nf * nc));
      std::memcpy(hm + ptr_bytes, in.num_rows, sizeof(int64_t) * (size_t)nf);
    }
    std::memset(hm + tab_bytes, 0, 64);
    const size_t lo = nf > 0 ? 0 : tab_bytes;
    HIP_TRY(hipMemcpyAsync(mp + lo, hm + lo, tab_bytes + 64 - lo, hipMemcpyHostToDevice, ft->s));
    if (mode == FragUpload::kSkipUnchanged) {
      if (nf > 0) ctx.meta_shadow.assign(hm, hm + tab_bytes);
      else ctx.meta_shadow.clear();
    }
  }
  ctx.meta_err_clean = false;  // (until a step's words have been read back as zeros: execute_impl)
  return MI355Q_OK;
}

namespace {

void set_step_knobs(const mi355q_exec_options& o) {
  TuneKnobs k;
  k.blocks_per_cu = o.tune_blocks_per_cu;
  k.probe_keyed_passes = o.probe_keyed_passes;
  k.pass_rows = o.pass_rows;
  k.flags = o.flags;
  k.overlap_cus = o.tune_overlap_cus;
  set_tune_knobs(k);
}

// Whether the LDS group-by (lds_direct) or the index-partitioned family (both) is going to take the step: the derived
// routes that would otherwise re-key it are then not asked.  (Small multi-column perfect-hash tables: the LDS group-by
// computes the entry index from the key columns itself, no packed index column needed.)
void members_ahead_of_routes(const mi355q_plan& plan, const mi355q_inputs& in, const mi355q_exec_options& o, const DevPlan& d,
                             int n_cus, bool async, bool* lds_direct, bool* idx_direct) {
  *lds_direct = *idx_direct = false;
  if (o.force_generic || in.n_frags <= 0 || (o.kernel_variant != 0 && o.kernel_variant != 2)) return;
  if (!(d.desc_type == MI355Q_GROUP_BY_PERFECT_HASH ||
        (d.desc_type == MI355Q_GROUP_BY_BASELINE_HASH && d.entry_count <= 65536 && !(o.flags & MI355Q_OPT_NO_LDS_BASELINE) && !async)))
    return;
  int64_t tr = 0, mr = 0;
  for (int f = 0; f < in.n_frags; ++f) {
    tr += in.num_rows[f];
    mr = std::max(mr, in.num_rows[f]);
  }
  FragView fvh{nullptr, nullptr, in.col_buffers, in.num_rows, in.n_frags, plan.n_cols, tr, mr};
  if (o.kernel_variant == 0) *lds_direct = lds_groupby_eligible(d, fvh, n_cus);
  // perfect-hash tables too large for LDS over plain INT keys and values: partitioned by entry index with narrow
  // records (kernels_idx.hip) instead of packed keys + one exchange per value column (kernel_variant 2 = "the
  // large-input members" takes it whatever the input size: tests)
  if (!*lds_direct && !async && d.desc_type == MI355Q_GROUP_BY_PERFECT_HASH && (tr >= kIdxPartMinRows || o.kernel_variant == 2))
    *lds_direct = *idx_direct = idx_part_eligible(d, fvh, n_cus);
}

// ---- plan-time kernel selection (a fixed family; no JIT).  The payload probe is chosen behind this, once its payload
// exists (join_probe_payload)
StepKind select_family(const DevPlan& d, const FragView& fv, const mi355q_exec_options& o, int n_cus, bool bf_step, bool idx_direct,
                       bool async) {
  if (o.force_generic || fv.n_frags <= 0) return K_GENERIC;
  if (bf_step) {  // a compiled filter beside the plan: only the families that take one
    if (scan_agg_eligible(d, fv)) return K_SCAN_AGG;
    if (o.kernel_variant == 0 && lds_groupby_eligible(d, fv, n_cus)) return K_LDS_GROUPBY;
    return K_GENERIC;
  }
  if (scan_count_eligible(d, fv)) return K_SCAN_COUNT;
  if (o.kernel_variant != 1 && scan_agg_eligible(d, fv)) return K_SCAN_AGG;
  // (a 1-byte filter column — the row mask of a compiled filter — in front of a few-groups step: the typed LDS member reads it
  // at 1.98 ms per 1 B rows, k_perfect_lds's 4-byte quad loads at ~3 ms: measured in round 6)
  if (!(d.n_quals == 1 && d.quals[0].type == MI355Q_INT8 && o.kernel_variant == 0 && lds_groupby_typed_eligible(d, fv, n_cus)) &&
      perfect_lds_eligible(d, fv))
    return K_PERFECT_LDS;
  // few groups: the table replicated in every workgroup's LDS (perfect-hash layouts up to 64 K entries that fit;
  // baseline layouts whose entry guess says "small" — if the groups turn out to be too many the step is re-run)
  if (o.kernel_variant == 0 && lds_groupby_eligible(d, fv, n_cus) &&
      (d.desc_type == MI355Q_GROUP_BY_PERFECT_HASH || (d.entry_count <= 65536 && !(o.flags & MI355Q_OPT_NO_LDS_BASELINE) && !async)))
    return K_LDS_GROUPBY;
  if (idx_direct && idx_part_eligible(d, fv, n_cus)) return K_IDX_PART;
  if (baseline_fast_eligible(d, fv)) return K_BASELINE_FAST;
  if (!join_sum_eligible(d, fv)) return K_GENERIC;
  // semi-join + aggregate over a large fact table: radix-partitioned probe (bitmap slices in
  // LDS) instead of one random bitmap read per row; kernel_variant 1 / 2 force either member
  if (o.kernel_variant != 1 && join_part_supported(d, fv, n_cus) && (o.kernel_variant == 2 || fv.total_rows >= ((int64_t)64 << 20)))
    return K_JOIN_PART;
  return K_JOIN_SUM;
}

// The partition scratch of the families that exchange rows: sized by the family's planner under a cap, grown in
// ctx.scratch.  Default cap: kDefaultScratchCap, but never more than 70 % of what the device has free right now
// (counting the scratch this context already holds), halved while the device cannot provide it (the planner then cuts
// the input into more chunks).  A probe that finds no plan within the cap falls back to its direct member (*kind).
int32_t size_scratch(DeviceCtx& ctx, const DevPlan& d, const FragView& fv, const JoinPayloadView& pay, const mi355q_exec_options& o,
                     int n_cus, StepKind* kind, int64_t* scratch_bytes, int64_t* scratch_cap) {
  if (*kind != K_BASELINE_FAST && *kind != K_JOIN_PART && *kind != K_JOIN_PROBE && *kind != K_IDX_PART) return MI355Q_OK;
  if (*scratch_cap <= 0) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const int64_t spare = (int64_t)((double)((int64_t)free_b + ctx.scratch.bytes) * 0.7);
      *scratch_cap = std::max<int64_t>(std::min<int64_t>(kDefaultScratchCap, spare), (int64_t)1 << 30);
    }
  }
  for (;;) {
    *scratch_bytes = *kind == K_JOIN_PART    ? join_part_scratch_bytes(d, fv, n_cus, *scratch_cap)
                     : *kind == K_IDX_PART   ? idx_part_scratch_bytes(d, fv, n_cus, *scratch_cap)
                     : *kind == K_JOIN_PROBE ? join_probe_scratch_bytes(d, fv, pay, probe_cus(n_cus), *scratch_cap)
                                             : baseline_fast_scratch_bytes(d, fv, o.kernel_variant, *scratch_cap, n_cus);
    if (*kind == K_JOIN_PROBE && *scratch_bytes == 0) {  // no plan within this cap: the row kernel
      *kind = join_sum_eligible(d, fv) ? K_JOIN_SUM : K_GENERIC;
      return MI355Q_OK;
    }
    if (*kind == K_IDX_PART && *scratch_bytes == 0) return MI355Q_ERR_OUT_OF_GPU_MEM;  // (eligible means it plans)
    if (*kind == K_JOIN_PART && *scratch_bytes == 0) {  // no plan within this cap: direct probe
      *kind = K_JOIN_SUM;
      return MI355Q_OK;
    }
    if (t_plan_only) return MI355Q_OK;
    const hipError_t e = ctx.scratch.grow(*scratch_bytes);
    if (e == hipSuccess) return MI355Q_OK;
    (void)hipGetLastError();
    const int64_t cur_cap = *scratch_cap > 0 ? *scratch_cap : kDefaultScratchCap;
    if (cur_cap <= ((int64_t)1 << 30)) {
      last_hip_error = e;
      return MI355Q_ERR_OUT_OF_GPU_MEM;
    }
    *scratch_cap = cur_cap / 2;
  }
}

// the events of a timed step, out of the context's pool: the step's pair, the launch functions' pair, their pool
struct StepEvents {
  hipEvent_t start = nullptr, stop = nullptr;
  hipEvent_t* pool = nullptr;
};
int32_t step_events(DeviceCtx& ctx, StepEvents* ev, LaunchStats* st) {
  constexpr int kEvPool = 128;
  if (int32_t e = grow_events(ctx, kEvPool + 4)) return e;
  ev->start = ctx.events[0];
  ev->stop = ctx.events[1];
  st->k_start = ctx.events[2];
  st->k_stop = ctx.events[3];
  ev->pool = ctx.events.data() + 4;
  st->ev_pool = ev->pool;
  st->n_ev = kEvPool;
  return MI355Q_OK;
}

// the launches of the chosen family over the uploaded table (n_frags > 0)
hipError_t launch_family(StepKind kind, const DevPlan& d, const mi355q_qmd& q, const FragView& fv, const JoinPayloadView& pay,
                         int64_t* buf, int32_t* d_err, const Workspace& scratch, int64_t scratch_cap, int kernel_variant, int n_cus,
                         hipStream_t s, LaunchStats* st) {
  switch (kind) {
    case K_SCAN_COUNT: return launch_scan_count(d, fv, buf, n_cus, s, st);
    case K_SCAN_AGG: return launch_scan_agg(d, fv, buf, n_cus, s, st);
    case K_PERFECT_LDS: return launch_perfect_lds(d, fv, buf, d_err, n_cus, s, st);
    case K_LDS_GROUPBY: return launch_lds_groupby(d, fv, buf, d_err, n_cus, s, st);
    case K_BASELINE_FAST: return launch_baseline_fast(d, fv, buf, d_err, scratch.p, scratch.bytes, scratch_cap, kernel_variant, n_cus, s, st);
    case K_IDX_PART: return launch_idx_partitioned(d, fv, buf, d_err, scratch.p, scratch.bytes, scratch_cap, n_cus, s, st);
    case K_JOIN_SUM: return launch_join_sum(d, fv, buf, n_cus, s, st);
    case K_JOIN_PART: return launch_join_partitioned(d, fv, buf, d_err, scratch.p, scratch.bytes, scratch_cap, n_cus, s, st);
    case K_JOIN_PROBE: return launch_join_probe(d, fv, pay, buf, d_err, scratch.p, scratch.bytes, scratch_cap, probe_cus(n_cus), s, st);
    default: break;
  }
  st->kernel_name = "k_generic";
  st->n_launches = 1;
  hipError_t e = st->k_start ? hipEventRecord(st->k_start, s) : hipSuccess;
  if (e == hipSuccess)
    e = launch_generic(d, q.idx_target_as_key, make_row_init(q), fv.d_cols, fv.d_num_rows, fv.n_frags, fv.max_frag_rows, buf, d_err, n_cus, s);
  if (e == hipSuccess && st->k_stop) e = hipEventRecord(st->k_stop, s);
  return e;
}

// what finish_step needs of a launched step, owned (the caller's arrays may be gone when mi355q_wait runs it)
TailState* new_tail(const mi355q_plan& plan, const mi355q_inputs& in, const mi355q_qmd& q, const DevPlan& d, StepKind kind,
                    const LaunchStats& st, mi355q_result* res, const FragTable& ft, const FragView& fv, int n_cus,
                    const StepEvents& ev, bool trace, const DeviceCtx& ctx) {
  TailState* tail = new (std::nothrow) TailState();
  if (!tail) return nullptr;
  tail->q = q;
  tail->d = d;
  tail->kind = kind;
  tail->st = st;
  tail->res = res;
  tail->d_err = ft.d_err;
  tail->d_cols = ft.d_cols;
  tail->d_rows = ft.d_rows;
  tail->h_cols.assign(in.col_buffers, in.col_buffers + (size_t)fv.n_frags * fv.n_cols);
  tail->h_rows.assign(in.num_rows, in.num_rows + fv.n_frags);
  tail->nf = fv.n_frags;
  tail->nc = fv.n_cols;
  tail->n_cus = n_cus;
  tail->total_rows = fv.total_rows;
  tail->max_frag_rows = fv.max_frag_rows;
  tail->alg_bytes = algorithmic_bytes(plan, in);
  tail->s = ft.s;
  tail->ev_start = ev.start;
  tail->ev_stop = ev.stop;
  tail->ev_pool = ev.pool;
  tail->trace = trace;
  tail->knobs = tune_knobs();
  tail->h_ret = (int32_t*)(ctx.h_meta + ctx.meta_bytes);
  tail->h_ret_dev = ctx.h_ret_dev;
  return tail;
}

// the options of the next attempt behind a retry code of finish_step
mi355q_exec_options retry_options(int32_t code, mi355q_exec_options o) {
  if (code == kRetryNoIdx) {
    o.flags |= MI355Q_OPT_NO_IDX_PART;
    return o;
  }
  // kRetryNoLds: small replicas did not hold the groups: the largest replica next, then eight windows of it, then another
  // family (skipping the windows over large inputs was measured and is worse: with <= 65536 entries the families behind
  // them are the direct global-atomic members — BH007 at 1 B rows: 29.6 ms in eight windows, 638 ms without,
  // profiles/r04_refbench_1b_call14.jsonl)
  o.flags |= !(o.flags & MI355Q_OPT_LDS_BASELINE_LARGE)     ? MI355Q_OPT_LDS_BASELINE_LARGE
             : !(o.flags & MI355Q_OPT_LDS_BASELINE_WINDOWS) ? MI355Q_OPT_LDS_BASELINE_WINDOWS
                                                            : MI355Q_OPT_NO_LDS_BASELINE;
  return o;
}

}  // namespace

// The step executor: the routes in the order of DESIGN.md 3.1 (observable through mi355q_explain), then the plain step.
// reserved != nullptr: RESERVE mode — plan the step, size and allocate the per-device workspace it would use,
// launch nothing (mi355q_reserve_workspace); the column pointers are not looked at
int32_t mq::api::execute_impl(const mi355q_plan* plan, const mi355q_inputs* in,
                              const mi355q_exec_options* opts, mi355q_result** out,
                              mi355q_exec_report* report, mi355q_pending** pend, int64_t* reserved) {
  if (!plan || !in || !out) return MI355Q_ERR_INVALID_PLAN;
  if (in->n_frags < 0 || (in->n_frags > 0 && (!in->col_buffers || !in->num_rows)))
    return MI355Q_ERR_INVALID_PLAN;
  *out = nullptr;
  {  // a step left in flight by mi355q_execute_async owns the device workspace: finish it first
    DeviceCtx& c0 = ctx_of(in->device_id);
    std::lock_guard<std::recursive_mutex> lk0(c0.mu);
    if (c0.inflight) {
      DeviceGuard g0(in->device_id);
      drain_inflight(c0);
    }
  }
  mi355q_exec_options o{};
  if (opts) o = *opts;
  for (int i = 0; i < plan->n_quals && i < MI355Q_MAX_QUALS; ++i)
    if (MI355Q_QUAL_OR_GROUP(plan->quals[i].op) != 0) o.force_generic = 1;  // a disjunction among the quals: the row kernel
  set_step_knobs(o);
  // ---- inner columns in the quals / group columns: the flattened plan's routes (the asynchronous call completes here)
  if (plan->abi_version == MI355Q_ABI_VERSION && has_inner_refs(*plan)) return execute_inner_refs(plan, in, o, out, report, reserved);
  // ---- a SEMI / ANTI join level: the join as a row mask, then the joinless plan's routes (the asynchronous call completes here)
  if (plan->abi_version == MI355Q_ABI_VERSION && is_exists_join(*plan))
    return try_route(out, [&] { return execute_exists_join(plan, in, o, out, report, reserved); });
  const bool async = pend != nullptr;
  if (async) {
    TuneKnobs k = tune_knobs();
    k.async_step = true;
    set_tune_knobs(k);
  }
  int32_t e = MI355Q_OK;  // (what the stage or route just asked answered)

  // ---- steps with expressions
  bool proj_step = plan->n_targets > 0;
  for (int i = 0; i < plan->n_targets && i < MI355Q_MAX_TARGETS; ++i) proj_step = proj_step && plan->targets[i].agg == MI355Q_PROJECT;
  if (plan->n_exprs != 0) {
    if (!async && !step_bool_filter() && !o.force_generic && !(o.flags & MI355Q_OPT_NO_COMPILED_FILTER)) {
      // (a Projection evaluates its expressions — filters included — in the compaction kernel's registers, unless they all
      // belong to its filter)
      e = proj_step ? execute_projection_filter(plan, in, o, out, report, reserved)
                    : execute_compiled_filter(plan, in, o, out, report, reserved);
      if (e != kNotTaken) return e;
    }
    if (proj_step) return execute_projection(plan, in, o, out, report, reserved);  // no k_project pass
    if (!async && (e = try_route(out, [&] { return execute_shifted_args(plan, in, o, out, report, reserved); })) != kNotTaken) return e;
    if (!async && (e = try_route(out, [&] { return execute_cast_key(plan, in, o, out, report, reserved); })) != kNotTaken) return e;
    if (!async && (e = try_route(out, [&] { return execute_agg_programs(plan, in, o, out, report, reserved); })) != kNotTaken) return e;
    if (!async && (e = try_route(out, [&] { return execute_grouped_agg_programs(plan, in, o, out, report, reserved); })) != kNotTaken) return e;
    if (reserved) {  // the step proper runs on the lowered plan: reserve for that
      route_note("k_project");
      mi355q_plan lp;
      if ((e = lower_exprs(*plan, &lp, nullptr, true))) return e;
      return execute_impl(&lp, in, &o, out, report, nullptr, reserved);
    }
    return execute_projected(plan, in, o, out, report);
  }

  // ---- the plan as the device sees it
  Trace tr((o.flags & MI355Q_OPT_TRACE) != 0);
  mi355q_qmd q;
  if ((e = qmd_init(*plan, &q))) return e;
  if (q.desc_type == MI355Q_PROJECTION) return execute_projection(plan, in, o, out, report, reserved);
  DevPlan d;
  if ((e = build_dev_plan(*plan, q, &d))) return e;
  if ((e = attach_join(*plan, in, &d))) return e;
  // a compiled filter travels beside the plan (its quals are gone): only the families that take one may run the step —
  // no derived plans, no row kernel; kNotTaken sends the caller back to the projection pass
  d.bf_active = step_bool_filter() != nullptr;
  const bool bf_step = d.bf_active != 0;
  DeviceGuard g(in->device_id);
  if (!g.ok) return MI355Q_ERR_HIP;
  const int n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);

  // ---- the layout twins
  if (q.output_columnar) return execute_columnar_twin(plan, in, o, q, out, report, reserved);
  if (q.slot_width == 4) return execute_wide_slot_twin(plan, in, o, q, out, report, reserved);

  // ---- the derived-plan routes, each asked unless a member that needs none of them is going to take the step
  bool lds_direct = false, idx_direct = false;
  members_ahead_of_routes(*plan, *in, o, d, n_cus, async, &lds_direct, &idx_direct);
  if (bf_step && in->n_frags <= 0) return kNotTaken;
  if (bf_step && q.desc_type != MI355Q_NON_GROUPED_AGGREGATE && (!lds_direct || idx_direct)) return kNotTaken;
  const bool fast = !o.force_generic && in->n_frags > 0;
  const bool join = plan->join_outer_col >= 0 && !bf_step;
  if (!async && join && (e = try_route(out, [&] { return execute_dense_join_as_filter(plan, in, o, out, report, reserved); })) != kNotTaken)
    return e;
  if (fast && !async && join && (e = try_route(out, [&] { return execute_join_gather(plan, in, o, q, d, n_cus, out, report, reserved); })) != kNotTaken)
    return e;
  if (fast && !async && join && (e = try_route(out, [&] { return execute_join_expand(plan, in, o, q, d, n_cus, out, report, reserved); })) != kNotTaken)
    return e;
  if (fast && !lds_direct && !async &&
      (e = try_route(out, [&] { return execute_perfect_twin(plan, in, o, q, n_cus, out, report, reserved); })) != kNotTaken)
    return e;
  // (before the LDS attempt on a small baseline table too: BH007's 10 K lattice points are a typed LDS member's work)
  if (fast && !async && !reserved &&
      (e = try_route(out, [&] { return execute_affine_twin(plan, in, o, q, n_cus, out, report, reserved); })) != kNotTaken)
    return e;
  if (fast && !lds_direct && (e = try_route(out, [&] { return execute_packed_multi(plan, in, o, q, d, n_cus, out, report, reserved); })) != kNotTaken)
    return e;
  // several value columns over a large input, and the LDS group-by is not going to take the step (table too large,
  // a forced variant, or its attempts already failed): one run per value column, zipped
  if (fast && !lds_direct && o.kernel_variant != 1 && d.n_group >= 1 &&
      (e = try_route(out, [&] { return execute_multi_value(plan, in, o, q, d, out, report, reserved); }, /*unsupported_too=*/true)) != kNotTaken)
    return e;

  // ---- the plain step: result, fragment table, family, payload, scratch
  mi355q_result* res = nullptr;
  if ((e = result_create_impl(&q, in->device_id, o.out_buffer, &res))) return e;
  ResultPtr owned(res);
  const int nf = in->n_frags, nc = plan->n_cols;
  int64_t total_rows = 0, max_frag_rows = 0;
  if ((e = frag_row_totals(*in, &total_rows, &max_frag_rows))) return e;
  DeviceCtx& ctx = ctx_of(in->device_id);
  std::lock_guard<std::recursive_mutex> ctx_lock(ctx.mu);
  FragTable ft;  // (reserve / explain launch nothing: no upload to leave in flight)
  if ((e = upload_frag_table(ctx, *in, nc, o.stream, reserved ? FragUpload::kNone : FragUpload::kSkipUnchanged, &ft))) return e;
  hipStream_t s = ft.s;
  UploadGuard upload_guard{s, !reserved};
  StepEvents ev;
  LaunchStats st;
  if (report && (e = step_events(ctx, &ev, &st))) return e;
  FragView fv{ft.d_cols, ft.d_rows, in->col_buffers, in->num_rows, nf, nc, total_rows, max_frag_rows};

  StepKind kind = select_family(d, fv, o, n_cus, bf_step, idx_direct, async);
  if (kind == K_GENERIC && !bf_step && fast && !async && plan->n_quals >= 2 && d.join_col < 0 &&
      (total_rows >= ((int64_t)1 << 20) || o.kernel_variant == 2) && !(o.flags & MI355Q_OPT_NO_COMPILED_FILTER) &&
      (e = execute_compiled_quals(plan, in, o, out, report, reserved)) != kNotTaken)
    return e;
  // joins that read the inner side / one-to-many tables / LEFT joins over a large outer table: the payload probe.  The
  // semi-join shapes keep their 1-bit-per-key member above.
  JoinPayloadView pay{};
  if (fast && kind != K_JOIN_PART && o.kernel_variant != 1 && plan->join_table && !reserved && d.join_col >= 0 &&
      (o.kernel_variant == 3 || total_rows >= ((int64_t)16 << 20)) &&
      join_probe_payload(const_cast<mi355q_join_table*>(plan->join_table), d, fv, in->inner_version, s, n_cus, &pay))
    kind = K_JOIN_PROBE;
  if (bf_step && kind != K_LDS_GROUPBY && kind != K_SCAN_AGG) return kNotTaken;
  tr.mark("setup done");
  int64_t scratch_bytes = 0, scratch_cap = o.scratch_bytes;
  if ((e = size_scratch(ctx, d, fv, pay, o, n_cus, &kind, &scratch_bytes, &scratch_cap))) return e;
  tr.mark("scratch allocated");
  if (reserved) {  // mi355q_reserve_workspace / mi355q_explain: nothing is launched
    route_note(family_name(kind, d, fv, o.kernel_variant, n_cus));
    *reserved = t_plan_only ? scratch_bytes : ctx.scratch.bytes;
    return MI355Q_OK;
  }

  // ---- launch
  // a scan step is ONE kernel of tens of microseconds behind a one-row initialisation: its own event pair (k_start / k_stop,
  // recorded by the launch function) is the step's time as well — two event commands fewer on the stream, ~3 us each
  if (nf > 0 && (kind == K_SCAN_COUNT || kind == K_SCAN_AGG)) ev.start = ev.stop = nullptr;
  if (ev.start) HIP_TRY(hipEventRecord(ev.start, s));
  // the partitioned member writes every row of the table itself (empty rows included)
  const bool self_init = kind == K_BASELINE_FAST && nf > 0 && baseline_fast_variant(d, fv, o.kernel_variant, n_cus) == 2;
  if (!self_init) HIP_TRY(launch_init_buffer(res->buf, q.entry_count, make_row_init(q), s));
  if (nf > 0) HIP_TRY(launch_family(kind, d, q, fv, pay, res->buf, ft.d_err, ctx.scratch, scratch_cap, o.kernel_variant, n_cus, s, &st));
  if (st.spill_counter32) {
    // the counter lives in the partition scratch, which mi355q_shard_merge_slices (or the next call) may reuse or
    // reallocate before mi355q_wait looks at it: keep a copy next to the error words
    HIP_TRY(hipMemcpyAsync(ft.d_err + 4, st.spill_counter32, 4, hipMemcpyDeviceToDevice, s));
    st.spill_counter32 = (uint32_t*)(ft.d_err + 4);
  }
  if (ev.stop) HIP_TRY(hipEventRecord(ev.stop, s));
  tr.mark("launched");

  // ---- the tail: parked for mi355q_wait, or finished here — and the step planned again where a member gave up
  TailState* tail = new_tail(*plan, *in, q, d, kind, st, res, ft, fv, n_cus, ev, tr.on, ctx);
  if (!tail) return MI355Q_ERR_OUT_OF_CPU_MEM;
  upload_guard.armed = false;  // (finish_step synchronises the stream; a pending step is drained before the next call)
  if (pend) {  // mi355q_execute_async: the rest runs in mi355q_wait (or before the next call on this device)
    mi355q_pending* p = new (std::nothrow) mi355q_pending();
    if (!p) {
      delete tail;
      return MI355Q_ERR_OUT_OF_CPU_MEM;
    }
    p->tail = tail;
    p->device_id = in->device_id;
    ctx.inflight = p;
    *pend = p;
    (void)owned.release();
    *out = res;
    return MI355Q_OK;
  }
  const int32_t code = finish_step(*tail, report);
  ctx.meta_err_clean = code == MI355Q_OK && tail->err_words_zero;
  delete tail;
  tr.mark("synchronized");
  if (code == kRetryNoIdx || code == kRetryNoLds) {
    owned.reset();
    const mi355q_exec_options o2 = retry_options(code, o);
    return execute_impl(plan, in, &o2, out, report, nullptr, nullptr);
  }
  if (code) return code;
  (void)owned.release();
  *out = res;
  return MI355Q_OK;
}

extern "C" {

// ------------------------------------------------------------------------------- synth
int32_t mi355q_generate_column(int32_t device_id, void* dst, int64_t n_rows, int64_t row_offset,
                               int32_t kind, uint64_t seed, int64_t a, int64_t b, int64_t c,
                               double a_f, int32_t null_every, void* stream) {
  if (!dst || n_rows < 0 || kind < MI355Q_GEN_I32_UNIFORM31 || kind > MI355Q_GEN_F64_UNIT)
    return MI355Q_ERR_INVALID_PLAN;
  if ((kind == MI355Q_GEN_I32_MOD || kind == MI355Q_GEN_I64_MOD || kind == MI355Q_GEN_I64_MOD_MUL) &&
      a <= 0)
    return MI355Q_ERR_INVALID_PLAN;
  DeviceGuard g(device_id);
  if (!g.ok) return MI355Q_ERR_HIP;
  HIP_TRY(launch_generate(dst, n_rows, row_offset, kind, seed, a, b, c, a_f, null_every,
                          (hipStream_t)stream));
  return MI355Q_OK;
}

}  // extern "C"

#if defined(HOSTSIM_DEVICE_CODE) && !defined(MI355Q_ROUTES_OWN_UNIT)
// Only for a host-simulation recipe written before api_routes.cpp existed (the tests/helpers.py of an older commit, run
// against this tree): its source list names api.cpp alone, so the routes join this unit there and the library still
// links.  Every current build — the device build (heavydb_amd/_build.py SOURCES) and this tree's hostsim_lib, which
// defines MI355Q_ROUTES_OWN_UNIT — compiles api_routes.cpp as a translation unit of its own.
#include "api_routes.cpp"
#endif
