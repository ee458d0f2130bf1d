// api_join.cpp — join hash tables of the C-ABI (include/mi355q.h): mi355q_join_build (perfect / keyed, OneToOne ->
// OneToMany, the four buffer layouts of the reference's docs hash_joins.rst), payload arrays, info.  Split out of api.cpp
// in round 5.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "api_internal.h"

using namespace mq;
using namespace mq::api;

// ------------------------------------------------------------------------------- the payload probe's payload
// Joins that read the inner side / one-to-many tables / LEFT joins over a large outer table: the payload probe (per-key
// aggregated payload of the perfect table in LDS, or in L2 as 16-byte entries).  The payload is derived from ONE inner
// column on first use and kept with the join table; a payload the probe plan then refuses is dropped and not built
// again for the same column and step shape.  The first build waits for the device (flags read-back).
bool mq::api::join_probe_payload(mi355q_join_table* jt, const DevPlan& d, const FragView& fv, int64_t inner_version,
                                 hipStream_t s, int n_cus, JoinPayloadView* pay) {
  const int n_cus_probe = probe_cus(n_cus);
  int wcol = -1, l2 = 0;
  if (!n_cus_probe || !join_probe_wants(d, fv, n_cus_probe, &wcol, &l2)) return false;
  const void* inner = wcol >= 0 ? (const void*)d.inner_cols[wcol] : nullptr;
  std::lock_guard<std::mutex> pl(jt->pay_mu);
  const int64_t entries = jt->entry_count;
  if (jt->pay_refused && jt->pay_refused_col == inner && jt->pay_refused_rows == fv.total_rows) return false;
  mi355q_join_table::PayloadCache& cache = l2 ? jt->pay_l2 : jt->pay_lds;
  if (!cache.holds(inner, inner_version)) {
    // (re)build for this inner column, in the layout the chosen mode reads
    hipEvent_t b0 = nullptr, b1 = nullptr;
    (void)hipEventCreate(&b0);
    (void)hipEventCreate(&b1);
    DevWord flags;
    bool ok = hipMalloc(&flags.p, 64) == hipSuccess;
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
        cache.built = true;
        cache.col = inner;
        cache.version = inner_version;
        cache.has_nulls = h_flags & 1;
        if (b0 && b1) (void)hipEventElapsedTime(&jt->pay_build_ms, b0, b1);
      }
    }
    if (b0) (void)hipEventDestroy(b0);
    if (b1) (void)hipEventDestroy(b1);
    if (!ok) {
      (void)hipGetLastError();
      return false;
    }
  }
  pay->cnt_k = l2 ? nullptr : jt->pay_cnt;
  pay->wsum_k = (!l2 && inner) ? jt->pay_wsum : nullptr;
  pay->wnn_k = (!l2 && inner) ? jt->pay_wnn : nullptr;
  pay->pay16 = l2 ? jt->pay16 : nullptr;
  pay->pay8 = l2 ? jt->pay8 : nullptr;
  pay->kkeys = l2 == 2 ? jt->pay_kkeys : nullptr;
  pay->inner_col = inner;
  pay->entries = entries;
  pay->has_nulls = cache.has_nulls;
  if (join_probe_supported(d, fv, *pay, n_cus_probe)) return true;
  // the probe plan does not take this payload after all: entries x 16 B of device memory are not kept for a
  // member that will not run (the step falls back to k_join_sum / the row kernel)
  auto drop = [](auto*& ptr) {
    if (ptr) (void)hipFree((void*)ptr);
    ptr = nullptr;
  };
  if (l2) {
    drop(jt->pay16);
    drop(jt->pay8);
    drop(jt->pay_kkeys);
  } else {
    drop(jt->pay_cnt);
    drop(jt->pay_wsum);
    drop(jt->pay_wnn);
  }
  cache.invalidate();
  *pay = JoinPayloadView{};
  jt->pay_refused = true;
  jt->pay_refused_col = inner;
  jt->pay_refused_rows = fv.total_rows;
  return false;
}

// ------------------------------------------------------------------------------- NDV estimate
namespace {

constexpr int kNdvDefaultBits = 11;  // the reference's hll_precision_bits default

// HyperLogLog.h hll_size: the estimate from the registers, in double precision
int64_t hll_estimate(const uint32_t* regs, int bits) {
  const int64_t m = (int64_t)1 << bits;
  const double alpha = m == 16 ? 0.673 : m == 32 ? 0.697 : m == 64 ? 0.709 : 0.7213 / (1.0 + 1.079 / (double)m);
  double sum = 0.0;
  int64_t zeros = 0;
  for (int64_t i = 0; i < m; ++i) {
    sum += std::ldexp(1.0, -(int)regs[i]);
    zeros += regs[i] == 0;
  }
  double e = alpha * (double)m * (double)m / sum;
  if (e <= 2.5 * (double)m && zeros > 0) e = (double)m * std::log((double)m / (double)zeros);
  return (int64_t)e;
}

// The registers of `n_frags` fragments of key columns (h_cols: host array [n_frags][kc.n] of device pointers; kc's own
// column pointers are not read) folded into registers_dev, or into zeroed registers of its own, and the estimate of
// what they then hold.  The arguments have been checked; the device is set.  Waits for the stream.
int32_t ndv_run(const JoinKeyCols& kc, int bits, int n_frags, const void* const* h_cols, const int64_t* h_rows,
                uint32_t* registers_dev, int device_id, hipStream_t s, int64_t* ndv) {
  const size_t reg_bytes = sizeof(uint32_t) << bits;
  DevWord own, table;
  uint32_t* regs = registers_dev;
  if (!regs) {
    HIP_TRY(hipMalloc(&own.p, reg_bytes));
    regs = (uint32_t*)own.p;
    HIP_TRY(hipMemsetAsync(regs, 0, reg_bytes, s));
  }
  // the fragments that have rows: column pointers, then row counts, as one table on the device
  std::vector<int64_t> h_table;
  std::vector<int64_t> rows;
  int64_t total = 0;
  bool vec = true;
  for (int k = 0; k < kc.n; ++k) vec = vec && (kc.type[k] == MI355Q_INT32 || kc.type[k] == MI355Q_INT64);
  for (int f = 0; f < n_frags; ++f) {
    if (h_rows[f] <= 0) continue;
    for (int k = 0; k < kc.n; ++k) {
      const uintptr_t ptr = (uintptr_t)h_cols[(size_t)f * kc.n + k];
      vec = vec && (ptr & 15) == 0;
      h_table.push_back((int64_t)ptr);
    }
    rows.push_back(h_rows[f]);
    total += h_rows[f];
  }
  if (total > 0) {
    static_assert(sizeof(void*) == sizeof(int64_t), "pointer table and row counts share one array");
    const size_t n_ptr = h_table.size();
    h_table.insert(h_table.end(), rows.begin(), rows.end());
    HIP_TRY(hipMalloc(&table.p, h_table.size() * sizeof(int64_t)));
    HIP_TRY(hipMemcpy(table.p, h_table.data(), h_table.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    NdvArgs a{};
    a.cols = (const int8_t* const*)table.p;
    a.rows = (const int64_t*)table.p + n_ptr;
    a.regs = regs;
    a.n_frags = (int32_t)rows.size();
    a.n_keys = kc.n;
    a.width = kc.width;
    a.bits = bits;
    for (int k = 0; k < kc.n; ++k) {
      a.type[k] = kc.type[k];
      a.nullable[k] = kc.nullable[k];
    }
    a.vec = vec ? 1 : 0;
    HIP_TRY(launch_ndv_hll(a, total, cu_count_of(device_id), s));
  }
  std::vector<uint32_t> h_regs((size_t)1 << bits);
  HIP_TRY(hipMemcpyAsync(h_regs.data(), regs, reg_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *ndv = hll_estimate(h_regs.data(), bits);
  return MI355Q_OK;
}

}  // namespace

extern "C" {

int32_t mi355q_estimate_ndv(const mi355q_ndv_spec* spec, uint32_t* registers_dev, void* stream, int64_t* ndv) {
  if (!spec || !ndv) return MI355Q_ERR_INVALID_PLAN;
  if (spec->n_keys < 1 || spec->n_keys > MI355Q_MAX_GROUP_COLS || spec->n_frags < 0) return MI355Q_ERR_INVALID_PLAN;
  const int bits = spec->precision_bits == 0 ? kNdvDefaultBits : spec->precision_bits;
  if (bits < 4 || bits > 13) return MI355Q_ERR_INVALID_PLAN;
  if (spec->n_frags > 0 && !spec->frag_rows) return MI355Q_ERR_INVALID_PLAN;
  for (int f = 0; f < spec->n_frags; ++f) {
    if (spec->frag_rows[f] < 0) return MI355Q_ERR_INVALID_PLAN;
    if (spec->frag_rows[f] == 0) continue;
    if (!spec->key_buffers) return MI355Q_ERR_INVALID_PLAN;
    for (int k = 0; k < spec->n_keys; ++k)
      if (!spec->key_buffers[(size_t)f * spec->n_keys + k]) return MI355Q_ERR_INVALID_PLAN;
  }
  JoinKeyCols kc{};
  kc.n = spec->n_keys;
  kc.width = 4;
  for (int k = 0; k < kc.n; ++k) {
    kc.type[k] = spec->key_types[k];
    kc.nullable[k] = spec->key_nullables[k];
    if (kc.type[k] < MI355Q_INT8 || kc.type[k] > MI355Q_INT64) return MI355Q_ERR_UNSUPPORTED;
    if (type_width(kc.type[k]) > 4) kc.width = 8;  // BaselineJoinHashTable::getKeyComponentWidth
  }
  DeviceGuard g(spec->device_id);
  if (!g.ok) return MI355Q_ERR_HIP;
  return ndv_run(kc, bits, spec->n_frags, spec->key_buffers, spec->frag_rows, registers_dev, spec->device_id,
                 (hipStream_t)stream, ndv);
}

// ------------------------------------------------------------------------------- joins
namespace {

// One attempt at one layout.  `one_to_many` selects hash types 2/3 instead of 0/1.
int32_t join_build_layout(const mi355q_join_spec* spec, bool perfect, bool one_to_many, int64_t keyed_entries,
                          const JoinKeyCols& kc, hipStream_t s, mi355q_join_table* jt, int32_t* d_err) {
  const mi355q_range& r = spec->key_range;
  const int64_t n = spec->num_rows;
  if (jt->buf) (void)hipFree(jt->buf);
  if (jt->bitmap) (void)hipFree(jt->bitmap);
  jt->buf = jt->bitmap = nullptr;
  HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), s));
  jt->n_keys = kc.n;
  jt->width = perfect ? 8 : kc.width;
  auto alloc = [&](int64_t bytes) -> int32_t {
    jt->bytes = bytes;
    hipError_t e = hipMalloc(&jt->buf, (size_t)(bytes > 0 ? bytes : 4));
    if (e != hipSuccess) {
      last_hip_error = e;
      return MI355Q_ERR_OUT_OF_GPU_MEM;
    }
    return MI355Q_OK;
  };
  if (perfect) {
    jt->min_key = r.min;
    jt->max_key = r.max;
    jt->entry_count = r.max - r.min + 1;
  } else {
    jt->min_key = jt->max_key = 0;
    jt->entry_count = keyed_entries;
    if (jt->entry_count > (int64_t)UINT32_MAX) return MI355Q_ERR_UNSUPPORTED;
  }
  const int64_t entries = jt->entry_count;
  if (!one_to_many) {
    if (perfect) {
      jt->hash_type = 0;
      if (int32_t e = alloc(entries * (int64_t)sizeof(int32_t))) return e;
      HIP_TRY(hipMemsetAsync(jt->buf, 0xFF, (size_t)jt->bytes, s));  // init_hash_join_buff: -1
      HIP_TRY(launch_join_fill_perfect(kc.col[0], kc.type[0], kc.nullable[0], n, r.min, r.max,
                                       (int32_t*)jt->buf, d_err, s));
      const size_t bm_bytes = (size_t)((entries + 31) / 32) * 4;
      hipError_t be = hipMalloc(&jt->bitmap, bm_bytes);
      if (be != hipSuccess) {
        last_hip_error = be;
        return MI355Q_ERR_OUT_OF_GPU_MEM;
      }
      HIP_TRY(launch_join_presence_bitmap((const int32_t*)jt->buf, entries, (uint32_t*)jt->bitmap, s));
    } else {
      jt->hash_type = 1;
      const int stride = kc.n + 1;
      if (int32_t e = alloc(entries * stride * kc.width)) return e;
      HIP_TRY(launch_join_init_keyed(jt->buf, entries, kc.n, stride, kc.width, s));
      HIP_TRY(launch_join_fill_keyed(kc, n, jt->buf, entries, stride, true, d_err, s));
    }
    return MI355Q_OK;
  }
  // one-to-many: [keys |] offsets | counts | payloads
  jt->hash_type = perfect ? 2 : 3;
  const int64_t key_bytes = perfect ? 0 : entries * kc.n * kc.width;
  if (int32_t e = alloc(key_bytes + (2 * entries + std::max<int64_t>(n, 1)) * (int64_t)sizeof(int32_t))) return e;
  if (!perfect) {
    HIP_TRY(launch_join_init_keyed(jt->buf, entries, kc.n, kc.n, kc.width, s));
    HIP_TRY(launch_join_fill_keyed(kc, n, jt->buf, entries, kc.n, false, d_err, s));
  }
  int32_t* offsets = (int32_t*)((int8_t*)jt->buf + key_bytes);
  DevWord tiles;
  HIP_TRY(hipMalloc(&tiles.p, sizeof(int64_t) * (size_t)(entries / 2048 + 2)));
  HIP_TRY(launch_join_one_to_many(kc, n, jt->hash_type, jt->buf, entries, jt->min_key, jt->max_key, offsets,
                                  offsets + entries, offsets + 2 * entries, (int64_t*)tiles.p, d_err, s));
  HIP_TRY(hipStreamSynchronize(s));  // tiles is freed on return
  return MI355Q_OK;
}

}  // namespace

int32_t mi355q_join_build(const mi355q_join_spec* spec, void* stream, mi355q_join_table** out) {
  if (!spec || !out || spec->num_rows < 0) return MI355Q_ERR_INVALID_PLAN;
  if (spec->num_rows > (int64_t)INT32_MAX) return MI355Q_ERR_UNSUPPORTED;  // int32 row ids
  const int n_keys = spec->n_keys > 1 ? spec->n_keys : 1;
  if (n_keys > MI355Q_MAX_GROUP_COLS) return MI355Q_ERR_INVALID_PLAN;
  JoinKeyCols kc{};
  kc.n = n_keys;
  kc.width = 4;
  for (int i = 0; i < n_keys; ++i) {
    kc.col[i] = (const int8_t*)(i == 0 ? spec->key_buffer : spec->more_key_buffers[i - 1]);
    kc.type[i] = i == 0 ? spec->key_type : spec->more_key_types[i - 1];
    kc.nullable[i] = i == 0 ? spec->key_nullable : spec->more_key_nullables[i - 1];
    if (kc.type[i] < MI355Q_INT8 || kc.type[i] > MI355Q_INT64) return MI355Q_ERR_UNSUPPORTED;
    if (spec->num_rows > 0 && !kc.col[i]) return MI355Q_ERR_INVALID_PLAN;
    // BaselineJoinHashTable::getKeyComponentWidth: 8 iff an inner key column is wider than 4 bytes
    if (type_width(kc.type[i]) > 4) kc.width = 8;
  }
  *out = nullptr;
  DeviceGuard g(spec->device_id);
  if (!g.ok) return MI355Q_ERR_HIP;
  hipStream_t s = (hipStream_t)stream;
  auto* jt = new (std::nothrow) mi355q_join_table();
  if (!jt) return MI355Q_ERR_OUT_OF_CPU_MEM;
  struct JG {
    mi355q_join_table* j;
    ~JG() { mi355q_join_free(j); }
  } jg{jt};
  jt->device_id = spec->device_id;
  jt->key_type = spec->key_type;
  jt->num_rows = spec->num_rows;
  const mi355q_range& r = spec->key_range;
  // PerfectJoinHashTable::getInstance (PerfectJoinHashTable.cpp:168-246): perfect when there is
  // ONE key column whose range is known and max-min+1 entries fit; else keyed
  // (HashJoin.cpp:340-372).
  int64_t max_entries = spec->max_perfect_entries > 0 ? spec->max_perfect_entries : (int64_t)INT32_MAX;
  const bool perfect = n_keys == 1 && !spec->prefer_baseline && r.valid && r.max >= r.min &&
                       ((__int128)r.max - (__int128)r.min) < (__int128)max_entries;
  DevWord err;
  HIP_TRY(hipMalloc(&err.p, sizeof(int32_t)));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  struct EG {
    hipEvent_t a, b;
    ~EG() {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } eg{e0, e1};
  HIP_TRY(hipEventRecord(e0, s));
  // a keyed table: the caller's entry count, else 2 x rows — or, asked for, 2 x the NDV estimate of the keys, which is
  // what the reference sizes it at (BaselineJoinHashTable.cpp:484-486)
  const int64_t default_entries = 2 * std::max<int64_t>(spec->num_rows, 1);
  int64_t keyed_entries = spec->keyed_entry_count > 0 ? spec->keyed_entry_count : default_entries;
  const bool from_ndv = !perfect && spec->keyed_entry_count == MI355Q_KEYED_ENTRIES_FROM_NDV;
  if (from_ndv) {
    const void* cols[MI355Q_MAX_GROUP_COLS];
    for (int i = 0; i < n_keys; ++i) cols[i] = kc.col[i];
    int64_t ndv = 0;
    if (int32_t e = ndv_run(kc, kNdvDefaultBits, 1, cols, &spec->num_rows, nullptr, spec->device_id, s, &ndv)) return e;
    keyed_entries = 2 * std::max<int64_t>(ndv, 1);
  }
  int32_t h_err = 0;
  for (int sizing = 0; sizing < 2; ++sizing) {
    // the reference tries OneToOne first and rebuilds as OneToMany when the fill reports a
    // duplicate key (PerfectJoinHashTable::reify / BaselineJoinHashTable::reify)
    for (int attempt = spec->one_to_many == 2 ? 1 : 0; attempt < 2; ++attempt) {
      if (int32_t e = join_build_layout(spec, perfect, attempt == 1, keyed_entries, kc, s, jt, (int32_t*)err.p)) return e;
      HIP_TRY(hipMemcpyAsync(&h_err, err.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (h_err != MI355Q_ERR_JOIN_NOT_ONE_TO_ONE || spec->one_to_many == 0) break;
    }
    // an estimate must never turn a buildable table into an error: once more at the size no estimate is behind
    if (!(from_ndv && h_err == MI355Q_ERR_JOIN_TABLE_FULL && keyed_entries < default_entries)) break;
    keyed_entries = default_entries;
  }
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipStreamSynchronize(s));
  (void)hipEventElapsedTime(&jt->build_ms, e0, e1);
  if (h_err) return h_err;
  jt->dense = jt->hash_type == 0 && !spec->key_nullable && spec->num_rows == jt->entry_count;
  jg.j = nullptr;
  *out = jt;
  return MI355Q_OK;
}

int32_t mi355q_join_invalidate_payload(mi355q_join_table* t) {
  if (!t) return MI355Q_ERR_INVALID_PLAN;
  std::lock_guard<std::mutex> pl(t->pay_mu);
  // the buffers are kept (the next build reuses them); only their validity goes
  t->pay_l2.invalidate();
  t->pay_lds.invalidate();
  t->pay_refused = false;
  return MI355Q_OK;
}

int32_t mi355q_join_payload_info(const mi355q_join_table* t, int64_t* bytes, float* build_ms, int64_t* inner_version) {
  if (!t) return MI355Q_ERR_INVALID_PLAN;
  mi355q_join_table* jt = const_cast<mi355q_join_table*>(t);
  std::lock_guard<std::mutex> pl(jt->pay_mu);
  int64_t b = 0;
  const int64_t n = t->entry_count;
  if (t->pay_cnt) b += n * 4;
  if (t->pay_wsum) b += n * 8;
  if (t->pay_wnn) b += n * 4;
  if (t->pay16) b += n * 16;
  if (t->pay8) b += n * (t->pay_kkeys ? 16 : 8);
  if (t->pay_kkeys) b += n * 8;
  if (bytes) *bytes = b;
  if (build_ms) *build_ms = t->pay_build_ms;
  if (inner_version) *inner_version = t->pay_l2.built ? t->pay_l2.version : t->pay_lds.version;
  return MI355Q_OK;
}

int32_t mi355q_join_key_shape(const mi355q_join_table* t, int32_t* key_components, int32_t* component_width) {
  if (!t) return MI355Q_ERR_INVALID_PLAN;
  if (key_components) *key_components = t->n_keys;
  if (component_width) *component_width = t->width;
  return MI355Q_OK;
}

void mi355q_join_free(mi355q_join_table* t) {
  if (!t) return;
  if (t->buf || t->bitmap || t->pay_cnt || t->pay16) {
    DeviceGuard g(t->device_id);
    if (t->buf) (void)hipFree(t->buf);
    if (t->bitmap) (void)hipFree(t->bitmap);
    if (t->pay_cnt) (void)hipFree(t->pay_cnt);
    if (t->pay_wsum) (void)hipFree(t->pay_wsum);
    if (t->pay_wnn) (void)hipFree(t->pay_wnn);
    if (t->pay16) (void)hipFree(t->pay16);
    if (t->pay8) (void)hipFree(t->pay8);
    if (t->pay_kkeys) (void)hipFree(t->pay_kkeys);
  }
  delete t;
}

int32_t mi355q_join_info(const mi355q_join_table* t, int32_t* hash_type, int64_t* entry_count,
                         int64_t* min_key, int64_t* max_key, void** device_ptr, int64_t* bytes,
                         float* build_ms) {
  if (!t) return MI355Q_ERR_INVALID_PLAN;
  if (hash_type) *hash_type = t->hash_type;
  if (entry_count) *entry_count = t->entry_count;
  if (min_key) *min_key = t->min_key;
  if (max_key) *max_key = t->max_key;
  if (device_ptr) *device_ptr = t->buf;
  if (bytes) *bytes = t->bytes;
  if (build_ms) *build_ms = t->build_ms;
  return MI355Q_OK;
}

}  // extern "C"
