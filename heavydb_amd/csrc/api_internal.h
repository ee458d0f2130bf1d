// api_internal.h — what the translation units of the C-ABI share (api.cpp, api_routes.cpp, api_projection.cpp,
// api_result.cpp, api_join.cpp): the opaque handle types, the per-device workspace, and the small host-side helpers.
// Internal to libmi355q.
// Out of execute_impl's body since the executor became a list of stages: Workspace (one grow / release for every
// per-device allocation), launch_stream, upload_frag_table (api.cpp, shared with the Projection), try_route; the
// compiled-filter stages and the layout twins (api_routes.cpp); join_probe_payload (api_join.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "plan.h"

struct mi355q_join_table {
  int device_id = 0;
  int hash_type = 0;  // 0 perfect 1:1, 1 keyed 1:1, 2 perfect 1:N, 3 keyed 1:N (mi355q.h)
  int key_type = MI355Q_INT64;
  int n_keys = 1, width = 8;  // key components / component width of keyed tables
  int64_t entry_count = 0;
  int64_t num_rows = 0;  // inner rows the table was built from (0: no slot holds a row)
  int64_t min_key = 0, max_key = 0;
  void* buf = nullptr;
  int64_t bytes = 0;
  void* bitmap = nullptr;  // perfect tables: presence bitmap (1 bit per slot), for probes that
                           // only need to know WHETHER a key matches (no inner column read)
  float build_ms = 0.f;
  // OneToOne perfect table in which EVERY slot holds a row id: the inner key column is NOT NULL, the build met no duplicate
  // and rows == max - min + 1.  hash_join_idx (GroupByRuntime.cpp:287-297) then answers >= 0 exactly for min <= key <= max.
  bool dense = false;
  // perfect tables: per-key aggregated payload for the payload probe (kernels_part.hip), built on
  // first use for one inner column and kept with the table (the inner table does not change under
  // a join table): rows per key, sum of the inner column over them, non-NULL values among them
  std::mutex pay_mu;
  uint32_t* pay_cnt = nullptr;
  int64_t* pay_wsum = nullptr;
  uint32_t* pay_wnn = nullptr;
  void* pay16 = nullptr;         // the same as 16-byte entries (L2 mode of the probe)
  int64_t* pay8 = nullptr;       // one-to-one tables, L2 mode: the inner value per key slot, INT64_MIN = absent
  int64_t* pay_kkeys = nullptr;  // keyed tables: the key of every slot (pay16 / pay8 are then per slot)
  // which inner column (address AND generation: mi355q_inputs.inner_version) each of the two payload layouts was built
  // for — pay_lds: pay_cnt / pay_wsum / pay_wnn; pay_l2: pay16 / pay8 / pay_kkeys (join_probe_payload, api_join.cpp)
  struct PayloadCache {
    bool built = false;
    const void* col = nullptr;
    int64_t version = 0;
    int has_nulls = 0;
    // a cached payload is only as good as the column it was derived from: same address AND same generation
    bool holds(const void* inner, int64_t inner_version) const { return built && (!inner || (col == inner && version == inner_version)); }
    void invalidate() {
      built = false;
      col = nullptr;
    }
  } pay_lds, pay_l2;
  float pay_build_ms = 0.f;
  // a payload the probe plan then refused (built, dropped): not built again for the same column and step shape
  bool pay_refused = false;
  const void* pay_refused_col = nullptr;
  int64_t pay_refused_rows = 0;
};

struct mi355q_result {
  mi355q_qmd qmd{};
  mq::DevPlan dplan{};  // layout + targets for reduce / iteration kernels
  int device_id = 0;
  int64_t* buf = nullptr;
  int64_t bytes = 0;
  bool owns_buf = false;
  int64_t total_matched = -1;  // Projection results: rows that passed the quals; -1 = not known to the host (a wrapped buffer)
  int64_t live_rows = -1;      // Projection results put together by mi355q_result_append: the rows at the front of the buffer
};

namespace mq {
struct BoolFilterHost;  // boolfilter.h
namespace api {

// mi355q_explain: the route of a step, written down while execute_impl plans it in RESERVE mode (nothing is launched,
// nothing is allocated: t_plan_only).  Every derived route (projection, row-wise / 8-byte twins, packed keys, one run
// per value column) notes itself and plans its derived step the same way.
extern thread_local std::string* t_route;
extern thread_local bool t_plan_only;
void route_note(const char* what);


#define HIP_TRY(expr)                                     \
  do {                                                    \
    hipError_t _e = (expr);                               \
    if (_e != hipSuccess) {                               \
      mq::api::last_hip_error = _e;                                \
      return _e == hipErrorOutOfMemory ? MI355Q_ERR_OUT_OF_GPU_MEM : MI355Q_ERR_HIP; \
    }                                                     \
  } while (0)

extern thread_local hipError_t last_hip_error;

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
    // hipGetLastError() is per thread and sticky: another runtime user in this process (torch)
    // may have left an unrelated error behind, which the launch checks would then report
    (void)hipGetLastError();
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int cu_count_of(int dev);

// Per-device workspace kept between calls: the partition scratch (tens of GB for the headline
// workload — hipMalloc/hipFree of that size costs up to a second per call), the fragment
// pointer tables and the timing events.  Calls on one device are serialised by `mu`, like
// the reference's per-device gpu_exec_mutex_ (ExecutionKernel.cpp:216-220).
struct Workspace {
  void* p = nullptr;
  int64_t bytes = 0;
  // at least `need` bytes (what it held is NOT kept when it grows).  A failed allocation leaves it empty and hands back
  // HIP's code: what that means for the step, and whether the sticky error is cleared, is the caller's business
  hipError_t grow(int64_t need) {
    if (bytes >= need) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, (size_t)need);
    if (e == hipSuccess) bytes = need;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct DeviceCtx {
  std::recursive_mutex mu;  // the packed multi-column path re-enters mi355q_execute
  Workspace aux;            // packed key column + temporary tables of that path
  Workspace wide;           // 8-byte-slot table of a step whose result layout has 4-byte slots
  Workspace proj;           // dense temporary columns of projected expressions (one pass of fragments)
  Workspace gather;         // dense temporary columns of a grouped join's inner side (execute_join_gather, and execute_join_expand's joined rows: the two never nest, their derived step has no join; may nest inside proj's step)
  Workspace star;           // the slot -> group entry map of a star join (execute_inner_refs: k_join_group_code writes it, k_star_groupby_lds reads it)
  Workspace lattice;        // dense INT32 key columns of a lattice-keyed step (execute_affine_twin; may nest inside both)
  void* bf_table = nullptr; // a compiled filter in device memory (boolfilter.h BoolFilter: atoms + truth table)
  Workspace maskws;         // the row mask of a compiled filter with program atoms (execute_masked: one pass of fragments)
  Workspace projws;         // Projection family: lowered expressions, ticket / total counters, tile table, tile descriptors
  Workspace scratch;        // the partition scratch
  void* meta = nullptr;
  size_t meta_bytes = 0;
  // pinned host mirror of `meta` (column table, row counts, zeroed error words go to the device as ONE copy that does not
  // stage through a driver buffer) + 64 bytes the error words and the spill counter come back into
  char* h_meta = nullptr;
  // what `meta` holds on the device: the table bytes of the last upload, and whether its error words are still the zeros
  // that upload laid down (a prepared step over resident columns sends the same table every time: the copy — a DMA command
  // ahead of the kernel, ~8 us of a 60 us scan — is then skipped)
  std::vector<char> meta_shadow;
  bool meta_err_clean = false;
  int32_t* h_ret_dev = nullptr;  // the device's address of the 64 return bytes behind h_meta (k_words_to_host writes them)
  std::vector<hipEvent_t> events;
  hipStream_t stream = nullptr;  // library-owned launch stream (when the caller passes none)
  struct mi355q_pending* inflight = nullptr;  // a step enqueued by mi355q_execute_async and not yet waited for
};
DeviceCtx& ctx_of(int dev);

// the stream a step's work goes to: the caller's, else the context's own, created on first use (ctx.mu held)
inline int32_t launch_stream(DeviceCtx& ctx, void* callers_stream, hipStream_t* s) {
  *s = (hipStream_t)callers_stream;
  if (*s) return MI355Q_OK;
  if (!ctx.stream) HIP_TRY(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
  *s = ctx.stream;
  return MI355Q_OK;
}

// The fragment table of a step in ctx.meta: column pointers | row counts | 64 zeroed error bytes, laid out in the pinned
// mirror ctx.h_meta and sent as ONE copy on the launch stream (api.cpp; ctx.mu held).
struct FragTable {
  const int8_t* const* d_cols = nullptr;
  const int64_t* d_rows = nullptr;
  int32_t* d_err = nullptr;
  hipStream_t s = nullptr;  // launch_stream(ctx, callers_stream)
};
enum class FragUpload {
  kAlways,          // the Projection: sends the table every time and forgets what `meta` held
  kSkipUnchanged,   // execute_impl: the same table as the last upload with its error words still zero is not sent again
  kNone,            // execute_impl in RESERVE mode: lay out only, nothing is launched
};
int32_t upload_frag_table(DeviceCtx& ctx, const mi355q_inputs& in, int nc, void* callers_stream, FragUpload mode, FragTable* ft);
// The upload reads the SHARED pinned block: a return that does not reach the step's own synchronisation (an allocation
// that fails, a HIP error, kNotTaken) must not leave it in flight — the next call on another stream rewrites h_meta and
// ctx.meta while the stale copy could still land.  Disarmed where the step synchronises itself or stays in
// flight by design (mi355q_execute_async: the next call drains it first).
struct UploadGuard {
  hipStream_t s;
  bool armed;
  ~UploadGuard() {
    if (armed) (void)hipStreamSynchronize(s);
  }
};

// the rows of a step's fragments: all of them and the largest fragment's (MI355Q_ERR_INVALID_PLAN: a negative count)
inline int32_t frag_row_totals(const mi355q_inputs& in, int64_t* total_rows, int64_t* max_frag_rows) {
  *total_rows = *max_frag_rows = 0;
  for (int f = 0; f < in.n_frags; ++f) {
    if (in.num_rows[f] < 0) return MI355Q_ERR_INVALID_PLAN;
    *total_rows += in.num_rows[f];
    *max_frag_rows = std::max(*max_frag_rows, in.num_rows[f]);
  }
  return MI355Q_OK;
}

// at least n timing events in the context's pool (ctx.mu held); who uses which index is the caller's business
inline int32_t grow_events(DeviceCtx& ctx, int n) {
  while ((int)ctx.events.size() < n) {
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    ctx.events.push_back(ev);
  }
  return MI355Q_OK;
}

// an owned result handle: freed with mi355q_result_free unless released to the caller
struct ResultFree {
  void operator()(mi355q_result* r) const { mi355q_result_free(r); }
};
using ResultPtr = std::unique_ptr<mi355q_result, ResultFree>;

// Small pinned-free device scratch for the error word / counters, one per call.
struct DevWord {
  void* p = nullptr;
  ~DevWord() {
    if (p) (void)hipFree(p);
  }
};

// a result handle over `qmd` (allocates the buffer unless one is given; no initialisation)
int32_t result_create_impl(const mi355q_qmd* qmd, int32_t device_id, void* device_buffer, mi355q_result** out);
// column bytes a plan must read (mi355q_exec_report.algorithmic_bytes)
int64_t algorithmic_bytes(const mi355q_plan& p, const mi355q_inputs& in);

// What every derived-plan route (api_routes.cpp) holds from its eligibility checks to its return: the device, the
// device context under its lock, the launch stream (the caller's, else the library's own) and, once begin_timing has
// run for a call that wants a report, the event pair around the route's work.  `status` is what construction met.
struct RouteScope {
  DeviceGuard dev;
  DeviceCtx& ctx;
  std::lock_guard<std::recursive_mutex> lock;
  hipStream_t s = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int32_t status = MI355Q_OK;
  RouteScope(int32_t device_id, void* stream) : dev(device_id), ctx(ctx_of(device_id)), lock(ctx.mu) {
    status = dev.ok ? launch_stream(ctx, stream, &s) : MI355Q_ERR_HIP;
  }
  RouteScope(const RouteScope&) = delete;
  ~RouteScope() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  // the timed span starts here (every route has its own place for it: behind its workspace set-up)
  int32_t begin_timing(const mi355q_exec_report* report) {
    if (!report) return MI355Q_OK;
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipEventRecord(ev0, s));
    return MI355Q_OK;
  }
  // The common tail: ev1, the route's device error word (d_err != null: read back behind ev1 and returned when set),
  // the synchronisation, the report = acc + extra_launches with the stated plan's figures.
  int32_t finish(mi355q_exec_report* report, const mi355q_exec_report& acc, int32_t extra_launches, const mi355q_plan& plan,
                 const mi355q_inputs& in, int64_t total_rows, const int32_t* d_err = nullptr) {
    return tail(report, acc, extra_launches, plan, in, total_rows, d_err, /*always_sync=*/true);
  }
  // The same tail for the projection and mask routes, which read no error word here and leave an UNTIMED call
  // unsynchronised (their last inner step has synchronised the stream); every other route synchronises always.
  int32_t finish_sync_if_timed(mi355q_exec_report* report, const mi355q_exec_report& acc, const mi355q_plan& plan,
                               const mi355q_inputs& in, int64_t total_rows) {
    return tail(report, acc, 0, plan, in, total_rows, nullptr, /*always_sync=*/false);
  }

 private:
  int32_t tail(mi355q_exec_report* report, const mi355q_exec_report& acc, int32_t extra_launches, const mi355q_plan& plan,
               const mi355q_inputs& in, int64_t total_rows, const int32_t* d_err, bool always_sync) {
    if (ev1) HIP_TRY(hipEventRecord(ev1, s));
    int32_t h_err = 0;
    if (d_err) HIP_TRY(hipMemcpyAsync(&h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    if (ev1 || d_err || always_sync) HIP_TRY(hipStreamSynchronize(s));
    if (h_err) return h_err;
    if (report) {
      *report = acc;
      (void)hipEventElapsedTime(&report->total_ms, ev0, ev1);
      report->n_launches = acc.n_launches + extra_launches;
      report->rows_scanned = total_rows;
      report->algorithmic_bytes = algorithmic_bytes(plan, in);
    }
    return MI355Q_OK;
  }
};

constexpr int32_t kNotTaken = INT32_MIN + 7;           // internal: "use the ordinary path"
constexpr int64_t kIdxPartMinRows = (int64_t)8 << 20;  // below this the row kernel / LDS members are as good
// the L2 members of the payload probe map workgroup b to XCD b % 8 and group b / 8 and walk the runs with stride
// gridDim / 8: they are planned and launched with a multiple of 8 workgroups, or not at all (found by the host
// simulation, which first ran them on "4 CUs": gridDim / 8 = 0 never advances — on the device a `tune_cus` below 8
// would have hung the GPU, and one that is not a multiple of 8 would have read some runs twice)
inline int probe_cus(int n_cus) { return n_cus >= 8 ? (n_cus & ~7) : 0; }

// Asks one route: what it answers, or kNotTaken with everything it noted for mi355q_explain cut back and *out null
// again, so that the next route in the order starts from a clean slate.  unsupported_too: execute_multi_value's one
// extra — its MI355Q_ERR_UNSUPPORTED means "not this way" as well.
// Every route is asked through here, which made three former hand-written undos uniform; none of them changes anything:
//  - execute_shifted_args and execute_cast_key used not to null *out.  Both store to *out only as their last statement
//    before `return MI355Q_OK`, or through an inner execute_impl, which nulls *out on entry and stores to it only where
//    it returns MI355Q_OK: behind a kNotTaken *out still is the null execute_impl laid down on entry.
//  - execute_affine_twin used to take no mark.  It is asked only where `reserved` is null, and t_route is non-null only
//    inside mi355q_explain, which plans with `reserved` set, as does every step a route derives while planning: with
//    t_route null there is nothing to mark or cut.
template <class Route>
int32_t try_route(mi355q_result** out, Route&& route, bool unsupported_too = false) {
  const size_t mark = t_route ? t_route->size() : 0;
  const int32_t e = route();
  if (e != kNotTaken && !(unsupported_too && e == MI355Q_ERR_UNSUPPORTED)) return e;
  if (t_route) t_route->resize(mark);
  *out = nullptr;
  return kNotTaken;
}

// the step executor (api.cpp).  reserved != null: RESERVE mode, plan only; pend != null: mi355q_execute_async
int32_t execute_impl(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options* opts, mi355q_result** out,
                     mi355q_exec_report* report, mi355q_pending** pend, int64_t* reserved = nullptr);
// ---- the derived-plan routes (api_routes.cpp), in execute_impl's order of asking.  Each rewrites the stated plan into a
// simpler one, runs that through mi355q_execute and fixes the result up; kNotTaken when the shape does not call for it.
// (the compiled-filter stages: an aggregate step's filter — fused atoms, else programs through the row mask —, a
// Projection whose expressions all belong to its filter, several plain quals in front of a one-filter family)
int32_t execute_compiled_filter(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_projection_filter(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                  mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_compiled_quals(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                               mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_shifted_args(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                             mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_cast_key(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                         mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
// (non-grouped aggregates whose arguments compile into two-register programs: one kernel, no projection pass)
int32_t execute_agg_programs(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                             mi355q_exec_report* report, int64_t* reserved);
// (... and the few-groups GROUP BY steps of such arguments: k_groupby_lds_prog.  Both lower the plan with
// lower_program_step and run through run_program_step, api_routes.cpp)
int32_t execute_grouped_agg_programs(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                     mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_projected(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                          mi355q_result** out, mi355q_exec_report* report);
// (the layout twins: columnar output through its row-wise form, 4-byte slots through the 8-byte layout)
int32_t execute_columnar_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                              mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_wide_slot_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                               mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_dense_join_as_filter(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                                     mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_join_gather(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                            const DevPlan& d, int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_join_expand(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                            const DevPlan& d, int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
// (inner columns in a join step's quals / group columns: asked ahead of every other route, and answers for good — the
// gather / expand routes above over the flattened plan; no other route meets an inner reference)
int32_t execute_inner_refs(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                           mi355q_exec_report* report, int64_t* reserved);
// (a SEMI / ANTI join level, plan.h is_exists_join: asked directly behind the inner-reference check, and answers for good — the
// join level becomes a row mask, k_join_exists_mask, and the joinless plan runs on `mask = 1`; no other route, no family and
// not the row kernel meet these kinds, attach_join refuses them)
int32_t execute_exists_join(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                            mi355q_exec_report* report, int64_t* reserved);
int32_t execute_perfect_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                             int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_affine_twin(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, const mi355q_qmd& q,
                            int n_cus, mi355q_result** out, mi355q_exec_report* report, int64_t* reserved);
int32_t execute_packed_multi(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                             const mi355q_qmd& q, const DevPlan& d, int n_cus, mi355q_result** out,
                             mi355q_exec_report* report, int64_t* reserved);
int32_t execute_multi_value(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o,
                            const mi355q_qmd& q, const DevPlan& d, mi355q_result** out, mi355q_exec_report* report,
                            int64_t* reserved);
// the Projection family's step (api_projection.cpp); reserved != null: plan only
int32_t execute_projection(const mi355q_plan* plan, const mi355q_inputs* in, const mi355q_exec_options& o, mi355q_result** out,
                           mi355q_exec_report* report, int64_t* reserved);
// ---- shared between api.cpp (the step executor), api_routes.cpp (the derived-plan routes), api_result.cpp (result
// objects, shards) and api_join.cpp
RowInit make_row_init(const mi355q_qmd& q);
ColLayout col_layout_of(const mi355q_qmd& q);
// the device operations that walk rows run on a row-wise twin of a columnar buffer (same entries, same values)
struct RowTwin {
  mi355q_result* tw = nullptr;
  ~RowTwin() {
    if (tw) mi355q_result_free(tw);
  }
};
int32_t make_row_twin(const mi355q_result* r, hipStream_t s, RowTwin* out);
int32_t store_row_twin(const RowTwin& t, mi355q_result* r, hipStream_t s);
int32_t run_reduce(mi355q_result* dst, const int64_t* rows, int64_t n_rows, void* stream);
// (api_join.cpp) the payload of the payload probe for this step, built on first use and cached with the join table:
// true with *pay filled when the probe is to run the step, false when it is not (no such shape, refused, out of memory)
bool join_probe_payload(mi355q_join_table* jt, const DevPlan& d, const FragView& fv, int64_t inner_version, hipStream_t s,
                        int n_cus, JoinPayloadView* pay);
int32_t attach_join(const mi355q_plan& p, const mi355q_inputs* in, DevPlan* d);  // (api.cpp) the join table and the inner columns
int64_t projection_row_count(const mi355q_result* r);
int32_t projection_append(mi355q_result* this_rs, const mi355q_result* that_rs, hipStream_t s);
int32_t projection_fetch_rows(const mi355q_result* r, int64_t max_rows, int64_t* ival, double* dval, int8_t* is_null, int64_t* n_rows);

}  // namespace api
}  // namespace mq
