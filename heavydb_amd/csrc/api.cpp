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
  for (int i = 0; i < p.n_quals; ++i) used[p.quals[i].col] = true;
  for (int g = 0; g < p.n_group_cols; ++g) used[p.group_cols[g]] = true;
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
  if (ctx.scratch) (void)hipFree(ctx.scratch);
  if (ctx.meta) (void)hipFree(ctx.meta);
  if (ctx.h_meta) (void)hipHostFree(ctx.h_meta);
  ctx.h_meta = nullptr;
  if (ctx.aux) (void)hipFree(ctx.aux);
  ctx.aux = nullptr;
  ctx.aux_bytes = 0;
  if (ctx.wide) (void)hipFree(ctx.wide);
  ctx.wide = nullptr;
  ctx.wide_bytes = 0;
  if (ctx.proj) (void)hipFree(ctx.proj);
  ctx.proj = nullptr;
  ctx.proj_bytes = 0;
  if (ctx.gather) (void)hipFree(ctx.gather);
  ctx.gather = nullptr;
  ctx.gather_bytes = 0;
  if (ctx.lattice) (void)hipFree(ctx.lattice);
  ctx.lattice = nullptr;
  ctx.lattice_bytes = 0;
  if (ctx.bf_table) (void)hipFree(ctx.bf_table);
  ctx.bf_table = nullptr;
  if (ctx.maskws) (void)hipFree(ctx.maskws);
  ctx.maskws = nullptr;
  ctx.maskws_bytes = 0;
  if (ctx.projws) (void)hipFree(ctx.projws);
  ctx.projws = nullptr;
  ctx.projws_bytes = 0;
  if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
  ctx.stream = nullptr;
  for (hipEvent_t e : ctx.events) (void)hipEventDestroy(e);
  ctx.scratch = ctx.meta = nullptr;
  ctx.scratch_bytes = 0;
  ctx.meta_bytes = 0;
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
  if (h_err[1] && t.kind == K_JOIN_PART) {
    // the partitioned probe ran out of spill space (extreme skew): redo with the direct probe
    HIP_TRY(hipMemsetAsync(t.d_err, 0, 64, s));
    HIP_TRY(launch_init_buffer(t.res->buf, q.entry_count, make_row_init(q), s));
    HIP_TRY(launch_join_sum(d, fv, t.res->buf, t.n_cus, s, &st));
    HIP_TRY(hipMemcpyAsync(h_err, t.d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (h_err[1] && t.kind == K_JOIN_PROBE) {
    // the payload probe ran out of spill space (extreme skew): redo the step with the row kernel
    HIP_TRY(hipMemsetAsync(t.d_err, 0, 64, s));
    HIP_TRY(launch_init_buffer(t.res->buf, q.entry_count, make_row_init(q), s));
    HIP_TRY(launch_generic(d, q.idx_target_as_key, make_row_init(q), t.d_cols, t.d_rows, t.nf, t.max_frag_rows, t.res->buf,
                           t.d_err, t.n_cus, s));
    st.kernel_name = "k_generic";
    HIP_TRY(hipMemcpyAsync(h_err, t.d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  // more groups than an LDS replica holds (a baseline table: the group count is only known now): the caller plans
  // the step again without that member (packed route / partitioned family / row kernel, whatever applies)
  if (h_err[1] && t.kind == K_LDS_GROUPBY) return kRetryNoLds;
  if (h_err[1] && t.kind == K_IDX_PART) return kRetryNoIdx;
  if (h_err[1] && t.kind == K_BASELINE_FAST) {
    // the partitioned family ran out of spill space (extreme skew): redo the step with the
    // direct-atomic member of the same family
    HIP_TRY(hipMemsetAsync(t.d_err, 0, 64, s));
    HIP_TRY(launch_init_buffer(t.res->buf, q.entry_count, make_row_init(q), s));
    HIP_TRY(launch_baseline_fast(d, fv, t.res->buf, t.d_err, nullptr, 0, 0, 1, t.n_cus, s, &st));
    HIP_TRY(hipMemcpyAsync(h_err, t.d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
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

int32_t mi355q_reserve_workspace(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options* opts,
                                 int64_t* reserved_bytes) {
  if (!plan || !in) return MI355Q_ERR_INVALID_PLAN;
  int64_t bytes = 0;
  // the planner looks at the pointer table for alignment only: a table of NULLs stands in for it
  std::vector<const void*> none((size_t)std::max(1, in->n_frags * std::max(plan->n_cols + plan->n_exprs + 1, 1)), nullptr);  // (+ 1: the row mask of a compiled filter, execute_masked)
  mi355q_inputs in2 = *in;
  in2.col_buffers = none.data();
  mi355q_result* r = nullptr;
  const int32_t e = execute_impl(plan, &in2, opts, &r, nullptr, nullptr, &bytes);
  if (r) mi355q_result_free(r);
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
    std::vector<const void*> none((size_t)std::max(1, in->n_frags * std::max(plan->n_cols + plan->n_exprs + 1, 1)), nullptr);  // (+ 1: the row mask of a compiled filter, execute_masked)
    mi355q_inputs in2 = *in;
    in2.col_buffers = none.data();  // (16-byte aligned chunks assumed, as mi355q_reserve_workspace does)
    mi355q_result* r = nullptr;
    t_route = &text;
    t_plan_only = true;
    e = execute_impl(plan, &in2, opts, &r, nullptr, nullptr, &bytes);
    t_route = nullptr;
    t_plan_only = false;
    if (r) mi355q_result_free(r);
  } catch (...) {
    t_route = nullptr;
    t_plan_only = false;
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
  {
    TuneKnobs k;
    k.blocks_per_cu = o.tune_blocks_per_cu;
    k.probe_keyed_passes = o.probe_keyed_passes;
    k.pass_rows = o.pass_rows;
    k.flags = o.flags;
    k.overlap_cus = o.tune_overlap_cus;
    set_tune_knobs(k);
  }
  bool proj_step = plan->n_targets > 0;
  for (int i = 0; i < plan->n_targets && i < MI355Q_MAX_TARGETS; ++i) proj_step = proj_step && plan->targets[i].agg == MI355Q_PROJECT;
  // (a Projection evaluates its expressions — filters included — in the compaction kernel's registers: below)
  if (plan->n_exprs != 0 && !pend && !step_bool_filter() && !o.force_generic && !proj_step && !(o.flags & MI355Q_OPT_NO_COMPILED_FILTER)) {
    // A filter of comparisons with literals under AND / OR / NOT is compiled into atoms + a truth table and evaluated by
    // the consuming kernel on the values it holds in registers (boolfilter.h): no temporary column, no second pass.
    BoolFilterHost bfh;
    mi355q_plan rest;
    if (compile_bool_filter(*plan, &bfh, &rest)) {
      const size_t mark = t_route ? t_route->size() : 0;
      int32_t e = kNotTaken;
      const bool fused_progs = bfh.bf.n_progs == 0 || (bfh.bf.all_lean && bfh.bf.all_i32 && bfh.bf.n_progs <= kLdsFusedProgs &&
                                                       !(o.flags & MI355Q_OPT_FILTER_PREPASS));
      if (fused_progs) {
        DeviceGuard gb(in->device_id);
        DeviceCtx& cb = ctx_of(in->device_id);
        std::lock_guard<std::recursive_mutex> lb(cb.mu);
        bool have = true;
        if (!t_plan_only) {
          if (!cb.bf_table) have = gb.ok && hipMalloc(&cb.bf_table, sizeof(BoolFilter)) == hipSuccess;
          // (a synchronous copy out of this frame: atoms + truth table, 1.2 KB)
          have = have && hipMemcpy(cb.bf_table, &bfh.bf, sizeof(BoolFilter), hipMemcpyHostToDevice) == hipSuccess;
        }
        if (have) {
          struct BfScope {
            BfScope(const BoolFilter* b, const BoolFilter* d) { set_step_bool_filter(b, d); }
            ~BfScope() { set_step_bool_filter(nullptr, nullptr); }
          } scope(&bfh.bf, (const BoolFilter*)cb.bf_table);
          route_note("filter compiled (atoms + truth table)");
          e = execute_impl(&rest, in, &o, out, report, nullptr, reserved);
        } else {
          (void)hipGetLastError();
        }
      }
      if (e == kNotTaken && bfh.bf.n_progs != 0) {  // program atoms no family evaluates itself: the row-mask pre-pass, then `mask = 1`
        if (t_route) t_route->resize(mark);
        *out = nullptr;
        route_note("filter compiled (atoms + programs + truth table)");
        e = execute_masked(plan, rest, bfh, in, o, out, report, reserved);
      }
      if (e != kNotTaken) {
        if (e == MI355Q_OK && report && !reserved) report->algorithmic_bytes = algorithmic_bytes(*plan, *in);
        return e;
      }
      if (t_route) t_route->resize(mark);
      *out = nullptr;
    }
  }
  if (plan->n_exprs != 0 && proj_step && !pend && !step_bool_filter() && !o.force_generic && !(o.flags & MI355Q_OPT_NO_COMPILED_FILTER)) {
    // a Projection whose expressions all belong to the FILTER (`SELECT a, b FROM t WHERE x + y > 100`): the filter is compiled,
    // the row-mask pre-pass evaluates it, the Projection runs on `mask = 1` — in its fast member where the targets allow —
    // instead of evaluating the quals' expressions row by row in the general member.  With a LIMIT only where the filter
    // cannot raise: the pre-pass looks at every row, the reference's loop stops at the limit.
    BoolFilterHost bfh;
    mi355q_plan rest;
    if (compile_bool_filter(*plan, &bfh, &rest) && (!bfh.bf.any_raise || plan->scan_limit == 0)) {
      const size_t mark = t_route ? t_route->size() : 0;
      route_note("filter compiled (atoms + programs + truth table)");
      const int32_t e = execute_masked(plan, rest, bfh, in, o, out, report, reserved);
      if (e != kNotTaken) return e;
      if (t_route) t_route->resize(mark);
      *out = nullptr;
    }
  }
  if (plan->n_exprs != 0) {
    {  // a Projection evaluates its expressions in the compaction kernel's registers: no k_project pass
      if (proj_step) return execute_projection(plan, in, o, out, report, reserved);
    }
    if (!pend) {
      const size_t mark = t_route ? t_route->size() : 0;
      int32_t e = execute_shifted_args(plan, in, o, out, report, reserved);
      if (e != kNotTaken) return e;
      if (t_route) t_route->resize(mark);
      e = execute_cast_key(plan, in, o, out, report, reserved);
      if (e != kNotTaken) return e;
      if (t_route) t_route->resize(mark);
    }
    if (reserved) {  // the step proper runs on the lowered plan: reserve for that
      route_note("k_project");
      mi355q_plan lp;
      if (int32_t e = lower_exprs(*plan, &lp, nullptr, true)) return e;
      return execute_impl(&lp, in, &o, out, report, nullptr, reserved);
    }
    return execute_projected(plan, in, o, out, report);
  }

  Trace tr((o.flags & MI355Q_OPT_TRACE) != 0);
  mi355q_qmd q;
  if (int32_t e = qmd_init(*plan, &q)) return e;
  if (q.desc_type == MI355Q_PROJECTION) return execute_projection(plan, in, o, out, report, reserved);
  DevPlan d;
  if (int32_t e = build_dev_plan(*plan, q, &d)) return e;
  if (int32_t e = attach_join(*plan, in, &d)) return e;
  // a compiled filter travels beside the plan (its quals are gone): only the families that take one may run the step —
  // no derived plans, no row kernel; kNotTaken sends the caller back to the projection pass
  d.bf_active = step_bool_filter() != nullptr;
  const bool bf_step = d.bf_active != 0;

  DeviceGuard g(in->device_id);
  if (!g.ok) return MI355Q_ERR_HIP;
  const int n_cus = o.tune_cus > 0 ? std::min(o.tune_cus, cu_count_of(in->device_id)) : cu_count_of(in->device_id);

  if (q.output_columnar) {
    // Columnar output: the step runs on the row-wise form of the same decisions (same entry
    // count, 8-byte key components, same hash, same slots) into a library-owned table, and the
    // finished table is moved column by column into the caller-visible buffer.
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

  if (q.slot_width == 4) {
    // Compact layout (4-byte slots): the step runs on the 8-byte layout of the same plan — same
    // entry count, same key bytes, same hash — and the finished table is narrowed row by row.
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
    const int64_t need = q8.entry_count * (int64_t)q8.row_size;
    if (ctx.wide_bytes < need) {
      if (ctx.wide) (void)hipFree(ctx.wide);
      ctx.wide = nullptr;
      ctx.wide_bytes = 0;
      hipError_t he = hipMalloc(&ctx.wide, (size_t)need);
      if (he != hipSuccess) {
        last_hip_error = he;
        return MI355Q_ERR_OUT_OF_GPU_MEM;
      }
      ctx.wide_bytes = need;
    }
    hipStream_t s4 = (hipStream_t)o.stream;
    if (!s4) {
      if (!ctx.stream) HIP_TRY(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
      s4 = ctx.stream;
    }
    mi355q_exec_options o8 = o;
    o8.stream = s4;
    o8.out_buffer = ctx.wide;
    mi355q_result* r8 = nullptr;
    if (int32_t e = mi355q_execute(&p8, in, &o8, &r8, report)) return e;
    mi355q_result_free(r8);
    mi355q_result* res4 = nullptr;
    if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &res4)) return e;
    hipError_t he = launch_narrow_slots((const int64_t*)ctx.wide, q8.row_size / 8, q.key_bytes / 8, q.slot_count,
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

  // (small multi-column perfect-hash tables: the LDS group-by computes the entry index from the key columns itself,
  // no packed index column needed)
  bool lds_direct = false, idx_direct = false;
  if (!o.force_generic && in->n_frags > 0 && (o.kernel_variant == 0 || o.kernel_variant == 2) &&
      (d.desc_type == MI355Q_GROUP_BY_PERFECT_HASH ||
       (d.desc_type == MI355Q_GROUP_BY_BASELINE_HASH && d.entry_count <= 65536 && !(o.flags & MI355Q_OPT_NO_LDS_BASELINE) && !pend))) {
    int64_t tr = 0, mr = 0;
    for (int f = 0; f < in->n_frags; ++f) {
      tr += in->num_rows[f];
      mr = std::max(mr, in->num_rows[f]);
    }
    FragView fvh{nullptr, nullptr, in->col_buffers, in->num_rows, in->n_frags, plan->n_cols, tr, mr};
    if (o.kernel_variant == 0) lds_direct = lds_groupby_eligible(d, fvh, n_cus);
    // perfect-hash tables too large for LDS over plain INT keys and values: partitioned by entry index with narrow
    // records (kernels_idx.hip) instead of packed keys + one exchange per value column (kernel_variant 2 = "the
    // large-input members" takes it whatever the input size: tests)
    if (!lds_direct && !pend && d.desc_type == MI355Q_GROUP_BY_PERFECT_HASH && (tr >= kIdxPartMinRows || o.kernel_variant == 2))
      lds_direct = idx_direct = idx_part_eligible(d, fvh, n_cus);
  }
  if (bf_step && in->n_frags <= 0) return kNotTaken;
  if (bf_step && q.desc_type != MI355Q_NON_GROUPED_AGGREGATE && (!lds_direct || idx_direct)) return kNotTaken;
  if (!pend && plan->join_outer_col >= 0 && !bf_step) {
    const size_t mark = t_route ? t_route->size() : 0;
    const int32_t e = execute_dense_join_as_filter(plan, in, o, out, report, reserved);
    if (e != kNotTaken) return e;
    if (t_route) t_route->resize(mark);
    *out = nullptr;
  }
  if (!o.force_generic && in->n_frags > 0 && !pend && plan->join_outer_col >= 0 && !bf_step) {
    const size_t mark = t_route ? t_route->size() : 0;
    const int32_t e = execute_join_gather(plan, in, o, q, d, n_cus, out, report, reserved);
    if (e != kNotTaken) return e;
    if (t_route) t_route->resize(mark);
    *out = nullptr;
  }
  if (!o.force_generic && in->n_frags > 0 && !lds_direct && !pend) {
    const size_t mark = t_route ? t_route->size() : 0;
    const int32_t e = execute_perfect_twin(plan, in, o, q, n_cus, out, report, reserved);
    if (e != kNotTaken) return e;
    if (t_route) t_route->resize(mark);
    *out = nullptr;
  }
  if (!o.force_generic && in->n_frags > 0 && !pend && !reserved) {
    // (before the LDS attempt on a small baseline table too: BH007's 10 K lattice points are a typed LDS member's work)
    const int32_t e = execute_affine_twin(plan, in, o, q, n_cus, out, report, reserved);
    if (e != kNotTaken) return e;
    *out = nullptr;
  }
  if (!o.force_generic && in->n_frags > 0 && !lds_direct) {
    const size_t mark = t_route ? t_route->size() : 0;
    const int32_t e = execute_packed_multi(plan, in, o, q, d, n_cus, out, report, reserved);
    if (e != kNotTaken) return e;
    if (t_route) t_route->resize(mark);
    *out = nullptr;
  }

  if (!o.force_generic && in->n_frags > 0 && !lds_direct && o.kernel_variant != 1 && d.n_group >= 1) {
    // several value columns over a large input, and the LDS group-by is not going to take the step (table too large,
    // a forced variant, or its attempts already failed): one run per value column, zipped
    const size_t mark = t_route ? t_route->size() : 0;
    const int32_t e = execute_multi_value(plan, in, o, q, d, out, report, reserved);
    if (e != kNotTaken && e != MI355Q_ERR_UNSUPPORTED) return e;
    if (t_route) t_route->resize(mark);
    *out = nullptr;
  }

  hipStream_t s = (hipStream_t)o.stream;  // caller's, or the device context's own (below)

  mi355q_result* res = nullptr;
  if (int32_t e = result_create_impl(&q, in->device_id, o.out_buffer, &res)) return e;
  ResultPtr owned(res);

  // device copies of the fragment tables + error word, one allocation
  const int nf = in->n_frags, nc = plan->n_cols;
  int64_t total_rows = 0, max_frag_rows = 0;
  for (int f = 0; f < nf; ++f) {
    if (in->num_rows[f] < 0) return MI355Q_ERR_INVALID_PLAN;
    total_rows += in->num_rows[f];
    max_frag_rows = std::max(max_frag_rows, in->num_rows[f]);
  }
  const size_t ptr_bytes = sizeof(void*) * (size_t)std::max(1, nf * nc);
  const size_t rows_bytes = sizeof(int64_t) * (size_t)std::max(1, nf);
  const size_t meta_bytes = ptr_bytes + rows_bytes + 64;
  DeviceCtx& ctx = ctx_of(in->device_id);
  std::lock_guard<std::recursive_mutex> ctx_lock(ctx.mu);
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
  if (!s) {
    if (!ctx.stream) HIP_TRY(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
    s = ctx.stream;
  }
  char* mp = (char*)ctx.meta;
  const int8_t* const* d_cols = (const int8_t* const*)mp;
  const int64_t* d_rows = (const int64_t*)(mp + ptr_bytes);
  int32_t* d_err = (int32_t*)(mp + ptr_bytes + rows_bytes);
  {
    // one copy out of pinned memory: column table | row counts | zeroed error words (the synchronous step of a 60 us scan
    // used to spend ~90 us on a memset and two copies out of pageable memory, each staged by the driver)
    char* hm = ctx.h_meta;
    const size_t tab_bytes = ptr_bytes + rows_bytes;
    // the same table as the last upload, its error words untouched since: nothing to send
    bool same = !reserved && nf > 0 && ctx.meta_err_clean && ctx.meta_shadow.size() == tab_bytes &&
                !std::memcmp(ctx.meta_shadow.data(), in->col_buffers, sizeof(void*) * (size_t)(nf * nc)) &&
                !std::memcmp(ctx.meta_shadow.data() + ptr_bytes, in->num_rows, sizeof(int64_t) * (size_t)nf);
    if (!same && !reserved) {  // (reserve / explain launch nothing: no upload to leave in flight)
      if (nf > 0) {
        std::memcpy(hm, in->col_buffers, sizeof(void*) * (size_t)(nf * nc));
        std::memcpy(hm + ptr_bytes, in->num_rows, sizeof(int64_t) * (size_t)nf);
      }
      std::memset(hm + ptr_bytes + rows_bytes, 0, 64);
      const size_t lo = nf > 0 ? 0 : ptr_bytes + rows_bytes;
      HIP_TRY(hipMemcpyAsync(mp + lo, hm + lo, ptr_bytes + rows_bytes + 64 - lo, hipMemcpyHostToDevice, s));
      if (nf > 0) ctx.meta_shadow.assign(hm, hm + tab_bytes);
      else ctx.meta_shadow.clear();
    }
    ctx.meta_err_clean = false;  // (until this step's words have been read back as zeros: below)
  }
  // The upload reads the SHARED pinned block: a return that does not reach finish_step (an allocation that fails, a HIP
  // error, kNotTaken) must not leave it in flight — the next call on another stream rewrites h_meta and ctx.meta while
  // the stale copy could still land.  Disarmed where the step synchronises itself or stays in flight by
  // design (mi355q_execute_async: the next call drains it first).
  struct UploadGuard {
    hipStream_t s;
    bool armed;
    ~UploadGuard() {
      if (armed) (void)hipStreamSynchronize(s);
    }
  } upload_guard{s, !reserved};

  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  LaunchStats st;
  constexpr int kEvPool = 128;
  hipEvent_t* ev_pool = nullptr;
  if (report) {
    while ((int)ctx.events.size() < kEvPool + 4) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      ctx.events.push_back(e);
    }
    ev_start = ctx.events[0];
    ev_stop = ctx.events[1];
    st.k_start = ctx.events[2];
    st.k_stop = ctx.events[3];
    ev_pool = ctx.events.data() + 4;
    st.ev_pool = ev_pool;
    st.n_ev = kEvPool;
  }

  FragView fv{d_cols, d_rows, in->col_buffers, in->num_rows, nf, nc, total_rows, max_frag_rows};

  // ---- plan-time kernel selection (a fixed family; no JIT)
  StepKind kind = K_GENERIC;
  JoinPayloadView pay{};
  if (bf_step) {
    if (!o.force_generic && nf > 0 && scan_agg_eligible(d, fv)) kind = K_SCAN_AGG;
    else if (!o.force_generic && nf > 0 && o.kernel_variant == 0 && lds_groupby_eligible(d, fv, n_cus)) kind = K_LDS_GROUPBY;
  } else if (!o.force_generic && nf > 0) {
    if (scan_count_eligible(d, fv)) kind = K_SCAN_COUNT;
    else if (o.kernel_variant != 1 && scan_agg_eligible(d, fv)) kind = K_SCAN_AGG;
    // (a 1-byte filter column — the row mask of a compiled filter — in front of a few-groups step: the typed LDS member reads it
    // at 1.98 ms per 1 B rows, k_perfect_lds's 4-byte quad loads at ~3 ms: measured in round 6)
    else if (!(d.n_quals == 1 && d.quals[0].type == MI355Q_INT8 && o.kernel_variant == 0 && lds_groupby_typed_eligible(d, fv, n_cus)) &&
             perfect_lds_eligible(d, fv))
      kind = K_PERFECT_LDS;
    // few groups: the table replicated in every workgroup's LDS (perfect-hash layouts up to 64 K entries that fit;
    // baseline layouts whose entry guess says "small" — if the groups turn out to be too many the step is re-run)
    else if (o.kernel_variant == 0 && lds_groupby_eligible(d, fv, n_cus) &&
             (d.desc_type == MI355Q_GROUP_BY_PERFECT_HASH ||
              (d.entry_count <= 65536 && !(o.flags & MI355Q_OPT_NO_LDS_BASELINE) && !pend)))
      kind = K_LDS_GROUPBY;
    else if (idx_direct && idx_part_eligible(d, fv, n_cus)) kind = K_IDX_PART;
    else if (baseline_fast_eligible(d, fv)) kind = K_BASELINE_FAST;
    else if (join_sum_eligible(d, fv)) kind = K_JOIN_SUM;
    // semi-join + aggregate over a large fact table: radix-partitioned probe (bitmap slices in
    // LDS) instead of one random bitmap read per row; kernel_variant 1 / 2 force either member
    if (kind == K_JOIN_SUM && o.kernel_variant != 1 && join_part_supported(d, fv, n_cus) &&
        (o.kernel_variant == 2 || total_rows >= ((int64_t)64 << 20)))
      kind = K_JOIN_PART;
  }

  // SEVERAL plain quals in front of a family that filters on one column (the partitioned GROUP BY, the perfect-hash LDS
  // member, the index-partitioned family takes none): instead of the row kernel, the quals become the range atoms of a
  // compiled filter, the row-mask pre-pass evaluates them (k_filter_mask: one byte per row) and the step runs on
  // `mask = 1` — measured in round 6: `a < K AND b > L` over 10 M INT64 groups went to k_generic at 55 ms per 1 B rows
  if (kind == K_GENERIC && !bf_step && !o.force_generic && nf > 0 && !pend && plan->n_exprs == 0 && plan->n_quals >= 2 &&
      d.join_col < 0 && q.desc_type != MI355Q_PROJECTION && (total_rows >= ((int64_t)1 << 20) || o.kernel_variant == 2) &&
      !(o.flags & MI355Q_OPT_NO_COMPILED_FILTER)) {
    BoolFilterHost bfh;
    mi355q_plan rest;
    if (compile_bool_filter(*plan, &bfh, &rest)) {
      const size_t mark = t_route ? t_route->size() : 0;
      route_note("quals compiled (range atoms + truth table)");
      const int32_t e = execute_masked(plan, rest, bfh, in, o, out, report, reserved);
      if (e != kNotTaken) return e;
      if (t_route) t_route->resize(mark);
      *out = nullptr;
    }
  }

  // joins that read the inner side / one-to-many tables / LEFT joins over a large outer table: the
  // payload probe (per-key aggregated payload of the perfect table in LDS).  The semi-join shapes
  // keep their 1-bit-per-key member above.
  // The L2 members of that probe map workgroup b to XCD b % 8 and group b / 8 and walk the runs with stride
  // gridDim / 8: they are planned and launched with a multiple of 8 workgroups, or not at all (found by the host
  // simulation, which first ran them on "4 CUs": gridDim / 8 = 0 never advances — on the device a `tune_cus` below 8
  // would have hung the GPU, and one that is not a multiple of 8 would have read some runs twice).
  const int n_cus_probe = n_cus >= 8 ? (n_cus & ~7) : 0;
  if (!o.force_generic && nf > 0 && kind != K_JOIN_PART && o.kernel_variant != 1 && plan->join_table && !reserved &&
      d.join_col >= 0 && (o.kernel_variant == 3 || total_rows >= ((int64_t)16 << 20))) {
    int wcol = -1, l2 = 0;
    if (n_cus_probe && join_probe_wants(d, fv, n_cus_probe, &wcol, &l2)) {
      mi355q_join_table* jt = const_cast<mi355q_join_table*>(plan->join_table);
      const void* inner = wcol >= 0 ? (const void*)d.inner_cols[wcol] : nullptr;
      std::lock_guard<std::mutex> pl(jt->pay_mu);
      const int64_t entries = jt->entry_count;
      bool ok = !(jt->pay_refused && jt->pay_refused_col == inner && jt->pay_refused_rows == total_rows);
      // a cached payload is only as good as the column it was derived from: same address AND same generation
      const bool have = l2 ? (jt->pay16_built && (!inner || (jt->pay16_col == inner && jt->pay16_version == in->inner_version)))
                           : (jt->pay_col_built && (!inner || (jt->pay_col == inner && jt->pay_version == in->inner_version)));
      if (ok && !have) {
        // (re)build for this inner column, in the layout the chosen mode reads
        hipEvent_t b0 = nullptr, b1 = nullptr;
        (void)hipEventCreate(&b0);
        (void)hipEventCreate(&b1);
        DevWord flags;
        ok = hipMalloc(&flags.p, 64) == hipSuccess;
        if (l2) {
          if (ok && !jt->pay16) ok = hipMalloc(&jt->pay16, (size_t)entries * 16) == hipSuccess;
          // one-to-one tables: the 8-byte payload — interleaved with the slot's key for a keyed table
          if (ok && (jt->hash_type == 0 || jt->hash_type == 1) && !jt->pay8)
            ok = hipMalloc((void**)&jt->pay8, (size_t)entries * (l2 == 2 ? 16 : 8)) == hipSuccess;
          // (one spare key behind the end: the keyed probe reads the keys two at a time)
          if (ok && l2 == 2 && !jt->pay_kkeys) ok = hipMalloc((void**)&jt->pay_kkeys, (size_t)entries * 8 + 16) == hipSuccess;
        } else {
          if (ok && !jt->pay_cnt) ok = hipMalloc((void**)&jt->pay_cnt, (size_t)entries * 4) == hipSuccess;
          if (ok && inner && !jt->pay_wsum) ok = hipMalloc((void**)&jt->pay_wsum, (size_t)entries * 8) == hipSuccess;
          if (ok && inner && !jt->pay_wnn) ok = hipMalloc((void**)&jt->pay_wnn, (size_t)entries * 4) == hipSuccess;
        }
        if (ok) {
          (void)hipMemsetAsync(flags.p, 0, 64, s);
          if (b0) (void)hipEventRecord(b0, s);
          ok = (l2 == 2 ? launch_join_payload_keyed_build(jt->buf, jt->hash_type, entries, inner, jt->pay_kkeys, jt->pay16,
                                                          jt->pay8, (int32_t*)flags.p, n_cus, s)
                        : launch_join_payload_build(jt->buf, jt->hash_type, entries, inner, jt->pay_cnt, jt->pay_wsum,
                                                    jt->pay_wnn, l2 ? jt->pay16 : nullptr, l2 ? jt->pay8 : nullptr,
                                                    (int32_t*)flags.p, n_cus, s)) == hipSuccess;
          if (b1) (void)hipEventRecord(b1, s);
          int32_t h_flags = 0;
          ok = ok && hipMemcpyAsync(&h_flags, flags.p, 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
               hipStreamSynchronize(s) == hipSuccess;
          if (ok) {
            if (l2) {
              jt->pay16_built = true;
              jt->pay16_col = inner;
              jt->pay16_version = in->inner_version;
              jt->pay16_has_nulls = h_flags & 1;
            } else {
              jt->pay_col_built = true;
              jt->pay_col = inner;
              jt->pay_version = in->inner_version;
              jt->pay_has_nulls = h_flags & 1;
            }
            if (b0 && b1) (void)hipEventElapsedTime(&jt->pay_build_ms, b0, b1);
          }
        }
        if (b0) (void)hipEventDestroy(b0);
        if (b1) (void)hipEventDestroy(b1);
        if (!ok) (void)hipGetLastError();
      }
      if (ok) {
        pay.cnt_k = l2 ? nullptr : jt->pay_cnt;
        pay.wsum_k = (!l2 && inner) ? jt->pay_wsum : nullptr;
        pay.wnn_k = (!l2 && inner) ? jt->pay_wnn : nullptr;
        pay.pay16 = l2 ? jt->pay16 : nullptr;
        pay.pay8 = l2 ? jt->pay8 : nullptr;
        pay.kkeys = l2 == 2 ? jt->pay_kkeys : nullptr;
        pay.inner_col = inner;
        pay.entries = entries;
        pay.has_nulls = l2 ? jt->pay16_has_nulls : jt->pay_has_nulls;
        if (join_probe_supported(d, fv, pay, n_cus_probe)) {
          kind = K_JOIN_PROBE;
        } else {
          // the probe plan does not take this payload after all: entries x 16 B of device memory are not kept for a
          // member that will not run (the step falls back to k_join_sum / the row kernel below)
          auto drop = [](auto*& ptr) {
            if (ptr) (void)hipFree((void*)ptr);
            ptr = nullptr;
          };
          if (l2) {
            drop(jt->pay16);
            drop(jt->pay8);
            drop(jt->pay_kkeys);
            jt->pay16_built = false;
            jt->pay16_col = nullptr;
          } else {
            drop(jt->pay_cnt);
            drop(jt->pay_wsum);
            drop(jt->pay_wnn);
            jt->pay_col_built = false;
            jt->pay_col = nullptr;
          }
          pay = JoinPayloadView{};
          jt->pay_refused = true;
          jt->pay_refused_col = inner;
          jt->pay_refused_rows = total_rows;
        }
      }
    }
  }

  if (bf_step && kind != K_LDS_GROUPBY && kind != K_SCAN_AGG) return kNotTaken;
  tr.mark("setup done");
  int64_t scratch_bytes = 0;
  int64_t scratch_cap = o.scratch_bytes;
  if (kind == K_BASELINE_FAST || kind == K_JOIN_PART || kind == K_JOIN_PROBE || kind == K_IDX_PART) {
    // default cap: kDefaultScratchCap, but never more than 70 % of what the device has free right now
    // (counting the scratch this context already holds), halved while the device cannot provide it
    // (the planner then cuts the input into more chunks)
    if (scratch_cap <= 0) {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const int64_t spare = (int64_t)((double)((int64_t)free_b + ctx.scratch_bytes) * 0.7);
        scratch_cap = std::max<int64_t>(std::min<int64_t>(kDefaultScratchCap, spare), (int64_t)1 << 30);
      }
    }
    for (;;) {
      scratch_bytes = kind == K_JOIN_PART    ? join_part_scratch_bytes(d, fv, n_cus, scratch_cap)
                      : kind == K_IDX_PART   ? idx_part_scratch_bytes(d, fv, n_cus, scratch_cap)
                      : kind == K_JOIN_PROBE ? join_probe_scratch_bytes(d, fv, pay, n_cus_probe, scratch_cap)
                                             : baseline_fast_scratch_bytes(d, fv, o.kernel_variant, scratch_cap, n_cus);
      if (kind == K_JOIN_PROBE && scratch_bytes == 0) {  // no plan within this cap: the row kernel
        kind = join_sum_eligible(d, fv) ? K_JOIN_SUM : K_GENERIC;
        break;
      }
      if (kind == K_IDX_PART && scratch_bytes == 0) return MI355Q_ERR_OUT_OF_GPU_MEM;  // (eligible means it plans)
      if (kind == K_JOIN_PART && scratch_bytes == 0) {  // no plan within this cap: direct probe
        kind = K_JOIN_SUM;
        break;
      }
      if (scratch_bytes <= ctx.scratch_bytes || t_plan_only) break;
      if (ctx.scratch) (void)hipFree(ctx.scratch);
      ctx.scratch = nullptr;
      ctx.scratch_bytes = 0;
      hipError_t e = hipMalloc(&ctx.scratch, (size_t)scratch_bytes);
      if (e == hipSuccess) {
        ctx.scratch_bytes = scratch_bytes;
        break;
      }
      (void)hipGetLastError();
      const int64_t cur_cap = scratch_cap > 0 ? scratch_cap : kDefaultScratchCap;
      if (cur_cap <= ((int64_t)1 << 30)) {
        last_hip_error = e;
        return MI355Q_ERR_OUT_OF_GPU_MEM;
      }
      scratch_cap = cur_cap / 2;
    }
  }

  tr.mark("scratch allocated");
  if (reserved) {  // mi355q_reserve_workspace / mi355q_explain: nothing is launched
    if (t_route) {
      char note[96];
      const char* name = kind == K_SCAN_COUNT ? "k_scan_count" : kind == K_SCAN_AGG ? "k_scan_agg"
                         : kind == K_PERFECT_LDS ? "k_perfect_lds" : kind == K_LDS_GROUPBY ? "k_groupby_lds"
                         : kind == K_JOIN_SUM ? "k_join_sum" : kind == K_JOIN_PART ? "k_part_scatter + k_part_join"
                         : kind == K_JOIN_PROBE ? "k_part_scatter + k_part_probe"
                         : kind == K_IDX_PART ? "k_idx_scatter + k_idx_aggregate"
                         : kind == K_BASELINE_FAST
                             ? (nf > 0 && baseline_fast_variant(d, fv, o.kernel_variant, n_cus) == 2 ? "k_part_scatter + k_part_aggregate"
                                                                                                      : "k_baseline_direct")
                             : "k_generic";
      std::snprintf(note, sizeof(note), "%s", name);
      route_note(note);
    }
    *reserved = t_plan_only ? scratch_bytes : ctx.scratch_bytes;
    return MI355Q_OK;
  }
  // a scan step is ONE kernel of tens of microseconds behind a one-row initialisation: its own event pair (k_start / k_stop,
  // recorded by the launch function) is the step's time as well — two event commands fewer on the stream, ~3 us each
  const bool one_kernel_step = nf > 0 && (kind == K_SCAN_COUNT || kind == K_SCAN_AGG);
  if (one_kernel_step) ev_start = ev_stop = nullptr;
  if (ev_start) HIP_TRY(hipEventRecord(ev_start, s));
  // the partitioned member writes every row of the table itself (empty rows included)
  const bool self_init = kind == K_BASELINE_FAST && nf > 0 &&
                         baseline_fast_variant(d, fv, o.kernel_variant, n_cus) == 2;
  if (!self_init) HIP_TRY(launch_init_buffer(res->buf, q.entry_count, make_row_init(q), s));

  if (nf > 0) {
    switch (kind) {
      case K_SCAN_COUNT:
        HIP_TRY(launch_scan_count(d, fv, res->buf, n_cus, s, &st));
        break;
      case K_SCAN_AGG:
        HIP_TRY(launch_scan_agg(d, fv, res->buf, n_cus, s, &st));
        break;
      case K_PERFECT_LDS:
        HIP_TRY(launch_perfect_lds(d, fv, res->buf, d_err, n_cus, s, &st));
        break;
      case K_LDS_GROUPBY:
        HIP_TRY(launch_lds_groupby(d, fv, res->buf, d_err, n_cus, s, &st));
        break;
      case K_BASELINE_FAST:
        HIP_TRY(launch_baseline_fast(d, fv, res->buf, d_err, ctx.scratch, ctx.scratch_bytes,
                                     scratch_cap, o.kernel_variant, n_cus, s, &st));
        break;
      case K_IDX_PART:
        HIP_TRY(launch_idx_partitioned(d, fv, res->buf, d_err, ctx.scratch, ctx.scratch_bytes, scratch_cap, n_cus, s, &st));
        break;
      case K_JOIN_SUM:
        HIP_TRY(launch_join_sum(d, fv, res->buf, n_cus, s, &st));
        break;
      case K_JOIN_PART:
        HIP_TRY(launch_join_partitioned(d, fv, res->buf, d_err, ctx.scratch, ctx.scratch_bytes, scratch_cap, n_cus,
                                        s, &st));
        break;
      case K_JOIN_PROBE:
        HIP_TRY(launch_join_probe(d, fv, pay, res->buf, d_err, ctx.scratch, ctx.scratch_bytes, scratch_cap, n_cus_probe, s,
                                  &st));
        break;
      default:
        st.kernel_name = "k_generic";
        st.n_launches = 1;
        if (st.k_start) HIP_TRY(hipEventRecord(st.k_start, s));
        HIP_TRY(launch_generic(d, q.idx_target_as_key, make_row_init(q), d_cols, d_rows, nf, max_frag_rows,
                               res->buf, d_err, n_cus, s));
        if (st.k_stop) HIP_TRY(hipEventRecord(st.k_stop, s));
    }
  }
  if (st.spill_counter32) {
    // the counter lives in the partition scratch, which mi355q_shard_merge_slices (or the next call) may reuse or
    // reallocate before mi355q_wait looks at it: keep a copy next to the error words
    HIP_TRY(hipMemcpyAsync(d_err + 4, st.spill_counter32, 4, hipMemcpyDeviceToDevice, s));
    st.spill_counter32 = (uint32_t*)(d_err + 4);
  }
  if (ev_stop) HIP_TRY(hipEventRecord(ev_stop, s));
  tr.mark("launched");

  TailState* tail = new (std::nothrow) TailState();
  if (!tail) return MI355Q_ERR_OUT_OF_CPU_MEM;
  tail->q = q;
  tail->d = d;
  tail->kind = kind;
  tail->st = st;
  tail->res = res;
  tail->d_err = d_err;
  tail->d_cols = d_cols;
  tail->d_rows = d_rows;
  tail->h_cols.assign(in->col_buffers, in->col_buffers + (size_t)nf * nc);
  tail->h_rows.assign(in->num_rows, in->num_rows + nf);
  tail->nf = nf;
  tail->nc = nc;
  tail->n_cus = n_cus;
  tail->total_rows = total_rows;
  tail->max_frag_rows = max_frag_rows;
  tail->alg_bytes = algorithmic_bytes(*plan, *in);
  tail->s = s;
  tail->ev_start = ev_start;
  tail->ev_stop = ev_stop;
  tail->ev_pool = ev_pool;
  tail->trace = tr.on;
  tail->knobs = tune_knobs();
  tail->h_ret = (int32_t*)(ctx.h_meta + ctx.meta_bytes);
  tail->h_ret_dev = ctx.h_ret_dev;
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
  if (code == kRetryNoIdx) {
    owned.reset();
    mi355q_exec_options o2 = o;
    o2.flags |= MI355Q_OPT_NO_IDX_PART;
    return execute_impl(plan, in, &o2, out, report, nullptr, nullptr);
  }
  if (code == kRetryNoLds) {
    owned.reset();
    mi355q_exec_options o2 = o;
    // small replicas did not hold the groups: the largest replica next, then eight windows of it, then another family
    // (skipping the windows over large inputs was measured and is worse: with <= 65536 entries the families behind them
    // are the direct global-atomic members — BH007 at 1 B rows: 29.6 ms in eight windows, 638 ms without,
    // profiles/r04_refbench_1b_call14.jsonl)
    o2.flags |= !(o.flags & MI355Q_OPT_LDS_BASELINE_LARGE)     ? MI355Q_OPT_LDS_BASELINE_LARGE
                : !(o.flags & MI355Q_OPT_LDS_BASELINE_WINDOWS) ? MI355Q_OPT_LDS_BASELINE_WINDOWS
                                                               : MI355Q_OPT_NO_LDS_BASELINE;
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
