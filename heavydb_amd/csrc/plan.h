// plan.h — internal host-side declarations of libmi355q (not part of the C-ABI).
#pragma once

#include "dev_common.h"

namespace mq {

struct ResolvedTarget {
  int agg = 0, col = -1, table = 0;
  int arg_type = 0;  // type code (dev_common.h)
  int key_idx = 0;   // PROJECT_KEY: index into group_cols
  bool cond_nullable = false;  // COUNT_IF / SUM_IF: the condition column is nullable
  bool arg_nullable = false, arg_fp = false, skip_null = false;
  bool arg_f32 = false;  // FLOAT argument: single-precision slot arithmetic
  bool constrained = false;  // constrained_not_null: a qual `arg IS NOT NULL`
  int n_slots = 1;
  const mi355q_range* range = nullptr;
};

int col_type_code(const mi355q_col_desc& c);  // < 0 = invalid
int32_t resolve_targets(const mi355q_plan& p, bool grouped, ResolvedTarget* out);
int32_t qmd_init(const mi355q_plan& p, mi355q_qmd* q);
int32_t qmd_init_projection(const mi355q_plan& p, const ResolvedTarget* ts, mi355q_qmd* q);  // the Projection descriptor
// While one lives (per thread), qmd_init lays multi-column integer keys out as a perfect hash up to `max_entries`
// entries instead of g_baseline_groupby_threshold: the library's own intermediate table of a baseline step (api.cpp
// execute_perfect_twin); never the layout a caller sees.
struct PerfectTwinScope {
  explicit PerfectTwinScope(int64_t max_entries);
  ~PerfectTwinScope();
  int64_t saved;
};
int64_t qmd_buffer_bytes(const mi355q_qmd& q);
int64_t qmd_group_col_offset(const mi355q_qmd& q, int g);  // columnar descriptors; -1 otherwise
int64_t qmd_slot_col_offset(const mi355q_qmd& q, int s);
int32_t build_dev_plan(const mi355q_plan& p, const mi355q_qmd& q, DevPlan* d);
// the layout part of a DevPlan (what reduce / iteration / sort need) from a descriptor alone
void layout_from_qmd(const mi355q_qmd& q, DevPlan* d);
// Projected expressions (mi355q_expr): validates every program and returns the plan in which expression k
// is an ordinary described column n_cols + k (its result type / nullability, the caller's range) and
// n_exprs == 0 — the plan every kernel family and the layout code see after the projection pass
// (kernels_generic.hip k_project) has written the expression's values into a dense temporary column.
// `dev` (optional) receives the lowered programs.
// widen_filter_bools: an INT8 (BOOLEAN) expression that ONLY quals read is described — and stored by the projection pass —
// as an INT32 column (its NULL becomes the INT32 NULL), so that the typed families, which filter on 4- and 8-byte
// columns, take the lowered step
int32_t lower_exprs(const mi355q_plan& p, mi355q_plan* lowered, DevExprSet* dev, bool widen_filter_bools = false);
// Inner columns in a join step's quals and group columns (MI355Q_INNER_COL, include/mi355q.h): the ONE rewrite of such a
// plan into its flattened, joinless form — inner column inner_col[k] becomes outer column n_cols + k, in order of first use
// (targets, quals, group columns); matched_flag: under an INNER join one more INT32 column, flag_col, and the qual
// `flag_col = 1` (a derived step over the joined rows of a one-to-many table needs neither).  A plan WITHOUT inner
// references is rewritten the same way (the inner columns its targets read): execute_join_gather / _expand's derived plan;
// its ranges stay the columns' own.  qmd_init, mi355q_explain, mi355q_reserve_workspace and execute_impl see inner
// references only to hand them here (api_routes.cpp execute_inner_refs); no other code path meets one.
struct InnerFlat {
  int n_inner = 0;
  int32_t inner_col[MI355Q_MAX_COLS] = {};
  int flag_col = -1;
};
bool has_inner_refs(const mi355q_plan& p);
int32_t flatten_inner_refs(const mi355q_plan& p, bool matched_flag, mi355q_plan* flat, InnerFlat* m);
// SEMI / ANTI join levels (MI355Q_JOIN_SEMI / _ANTI, include/mi355q.h): the ONE rewrite of such a plan.  `joinless` is the stated
// plan without the join — what the step means over the rows that pass the join level, and whose descriptor qmd_init returns;
// `masked` is joinless plus one INT8 NOT NULL column in [0, 1] behind the stated ones (mask_col) and the qual `mask_col = 1` as
// the last qual — what api_routes.cpp execute_exists_join runs once k_join_exists_mask has written that column.  The refusals
// are the ones mi355q.h states.
bool is_exists_join(const mi355q_plan& p);
int32_t exists_join_plans(const mi355q_plan& p, mi355q_plan* joinless, mi355q_plan* masked, int* mask_col);
uint32_t expr_qual_mask(const mi355q_plan& p);  // expressions evaluated for every row (read by a qual, directly or through another)
// one initialised row (key quads then slot init values); quad holds row_size / 8 entries
void row_init_image(const mi355q_qmd& q, int64_t* quad);

}  // namespace mq
