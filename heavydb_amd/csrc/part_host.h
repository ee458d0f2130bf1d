// part_host.h — host side shared by the partitioned families (kernels_part.hip: hash-partitioned GROUP BY, radix join,
// payload probe; kernels_idx.hip: index-partitioned GROUP BY).  All four scatter the input into (workgroup, partition)
// runs in a scratch buffer, chunk by chunk, and hand each chunk to a consumer kernel and its spill kernel.  Here: how the
// runs, the spill list and the chunks are sized (size_runs), how the scratch is carved (ScratchCarve), how the fragments
// are cut into chunks (next_chunk) and how a scatter launch is timed and counted (TimedLaunches).  Plain C++, no device code.
#pragma once

#include <cstdint>

#include "kernels.h"

namespace mq {
namespace part_host {

// Where the families differ in sizing their runs.  Every field is a difference that exists today; none is a tuning knob.
struct RunFamily {
  int recs_per_unit;          // records per 16-byte unit: 1 in the hash families, 1 << rs in the index family
  int64_t unit_bytes;         // 16 everywhere (Rec / v4i32)
  double shrink;              // chunk_rows *= shrink until the scratch fits: 0.9 in the index family, 0.97 elsewhere
  uint64_t index_limit;       // P x B x cap stays below it: 2^31 units in the index family, 2^32 records elsewhere
  bool big_cap_refuses;       // cap > 0x7fffffff: the GROUP BY refuses the plan, the others shrink the chunk and retry
  uint32_t spill_min;         // floor of the spill list: kSpillMin, kIdxSpillMin in the index family
  int64_t spill_max;          // its ceiling: 0x3fffffff in the index family, 0x7fffffff elsewhere
  int64_t spill_entry_bytes;  // 8 x (1 + ns_int) in the hash families, 16 in the index family
  int64_t cnt_extra_bytes;    // behind the run lengths: kPairCtrBytes in the GROUP BY, 0 elsewhere
  bool fit_rounded;           // the GROUP BY fits the 256-byte-rounded buffer (buf_bytes) under the cap, the others the plain sum
  bool even_chunks;           // equal-sized chunks once the limit is known: all but the radix join
  int overlap_min_chunks;     // GROUP BY with phase 1 next to phase 2: two buffers of half the cap each, the input cut into
                              // at least this many chunks; 0 = one buffer, start from the whole input
  uint64_t word_weight;       // index family, packed records: recs_per_unit x the largest value code; B x cap x this must stay
                              // below 2^32 (a partition's sum of codes in one word) or the plan is refused; 0 = no such word
};

struct RunSizes {
  uint32_t cap;           // units per (workgroup, partition) run, whole lines
  uint32_t spill_cap;     // spill list entries
  int64_t chunk_rows;     // rows per chunk at most (fragments are not split)
  int64_t rec_bytes;      // runs
  int64_t cnt_bytes;      // run lengths (+ cnt_extra_bytes)
  int64_t buf_bytes;      // runs + run lengths + spill header and list, rounded to 256 bytes
  int64_t scratch_bytes;  // the plain sum, or two buf_bytes when overlapped
};

// Worst case every row survives the filter.  Starts from the whole input (one chunk may not exceed 0xfff00000 rows: 32-bit
// LDS counters) and shrinks the chunk until the runs (1.2 x mean + 6 sigma + a line of slack per run, whole lines), the
// run lengths and the spill list (1/16 of the chunk's rows) fit `scratch_cap` (<= 0: kDefaultScratchCap), never below one
// fragment.  false = the plan is refused.
inline bool size_runs(int64_t total_rows, int64_t max_frag_rows, uint32_t P, int32_t B, uint32_t L, int64_t scratch_cap,
                      const RunFamily& f, RunSizes* out) {
  RunSizes& r = *out;
  if (scratch_cap <= 0) scratch_cap = kDefaultScratchCap;
  int64_t chunk_rows = total_rows > 0 ? total_rows : 1;
  if (f.overlap_min_chunks > 0) {
    scratch_cap /= 2;
    const int64_t want = (total_rows + f.overlap_min_chunks - 1) / f.overlap_min_chunks + max_frag_rows;
    if (want < chunk_rows) chunk_rows = want;
    if (chunk_rows < max_frag_rows) chunk_rows = max_frag_rows;
  }
  if (chunk_rows > 0xfff00000ll) chunk_rows = 0xfff00000ll;
  for (;;) {
    const double per_run = (double)chunk_rows / ((double)P * B);  // records
    uint64_t cap = (uint64_t)((per_run * 1.2 + 6.0 * __builtin_sqrt(per_run + 1.0)) / f.recs_per_unit) + L;
    cap = (cap + L - 1) / L * L;
    if (cap > 0x7fffffffull && f.big_cap_refuses) return false;
    // 32-bit run positions in phase 1
    const bool too_many = cap > 0x7fffffffull || (uint64_t)P * B * cap >= f.index_limit;
    if (!too_many) {
      if (f.word_weight && (uint64_t)B * cap * f.word_weight >= ((uint64_t)1 << 32)) return false;
      int64_t spill_cap = chunk_rows / 16;
      if (spill_cap < (int64_t)f.spill_min) spill_cap = f.spill_min;
      if (spill_cap > f.spill_max) spill_cap = f.spill_max;
      r.cap = (uint32_t)cap;
      r.spill_cap = (uint32_t)spill_cap;
      r.rec_bytes = (int64_t)P * B * (int64_t)cap * f.unit_bytes;
      r.cnt_bytes = (((int64_t)P * B * 4 + 255) & ~255ll) + f.cnt_extra_bytes;
      const int64_t sum = r.rec_bytes + r.cnt_bytes + 256 + spill_cap * f.spill_entry_bytes;
      r.buf_bytes = (sum + 255) & ~255ll;
      r.scratch_bytes = f.overlap_min_chunks > 0 ? 2 * r.buf_bytes : sum;
      if ((f.fit_rounded ? r.buf_bytes : sum) <= scratch_cap || chunk_rows <= max_frag_rows) break;
    }
    if (chunk_rows <= max_frag_rows) return false;
    chunk_rows = (int64_t)(chunk_rows * f.shrink);
    if (chunk_rows < max_frag_rows) chunk_rows = max_frag_rows;
  }
  // equal-sized chunks: 10 B rows under a 3.4 B-row limit are three chunks of 3.3 B, not two full ones and a sliver
  // (every chunk pays the consumer's table re-load, the emission and the launch tails)
  if (f.even_chunks && total_rows > chunk_rows) {
    const int64_t n_chunks = (total_rows + chunk_rows - 1) / chunk_rows;
    const int64_t even = (total_rows + n_chunks - 1) / n_chunks + max_frag_rows;  // fragments are not split
    if (even < chunk_rows) chunk_rows = even;
  }
  r.chunk_rows = chunk_rows;
  return true;
}

// g.P, g.L = units of a staged line, g.lgL = log2 of it, for `stage_units` staged per workgroup
template <typename G>
inline void line_geometry(G& g, uint32_t stage_units, uint32_t P) {
  g.P = (int32_t)P;
  g.L = stage_units / P;
  g.lgL = 0;
  while ((1u << g.lgL) < g.L) ++g.lgL;
}

// whole fragments from f0 on, as many as stay within chunk_rows, at least one; nf == 0 past the last fragment
struct Chunk {
  int f0, nf;
  int64_t rows;
};
inline Chunk next_chunk(const FragView& fv, int f0, int64_t chunk_rows) {
  Chunk c{f0, 0, 0};
  for (int f1 = f0; f1 < fv.n_frags; ++f1) {
    const int64_t n = fv.h_num_rows[f1];
    if (f1 > f0 && c.rows + n > chunk_rows) break;
    c.rows += n;
    c.nf += 1;
  }
  return c;
}

// one buffer set in the scratch: runs, run lengths, the 256-byte spill header (its first word counts the entries), entries
struct ScratchCarve {
  char* recs;
  uint32_t* cnt;
  char* spill_base;
  ScratchCarve(void* scratch, int64_t rec_bytes, int64_t cnt_bytes, int buf = 0, int64_t buf_bytes = 0)
      : recs((char*)scratch + (int64_t)buf * buf_bytes), cnt((uint32_t*)(recs + rec_bytes)), spill_base(recs + rec_bytes + cnt_bytes) {}
  uint32_t* spill_count() const { return (uint32_t*)spill_base; }
  char* spill_entries() const { return spill_base + 256; }
};

// The scatter launches are the ones a step's report times: each takes a (start, stop) pair from LaunchStats::ev_pool while
// pairs last, and is counted either way.  An error from the launch returns before the stop event and the count.
struct TimedLaunches {
  LaunchStats* st;
  hipStream_t s;
  int ev_i = 0;
  template <typename F>
  hipError_t run(F&& launch) {
    const bool timed = st->ev_pool && ev_i + 1 < st->n_ev;
    if (timed) (void)hipEventRecord(st->ev_pool[ev_i], s);
    const hipError_t e = launch();
    if (e != hipSuccess) return e;
    if (timed) {
      (void)hipEventRecord(st->ev_pool[ev_i + 1], s);
      ev_i += 2;
    }
    st->n_launches += 1;
    return hipSuccess;
  }
};

}  // namespace part_host
}  // namespace mq
