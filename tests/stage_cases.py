"""Inputs of the pinned step-executor cases (test_hostsim_real_kernels.py::test_executor_stages_are_the_pinned_ones and
its twin on the device, test_zz_gpu_executor_stages.py): cases of the case matrix, the Projection cases and the reference
benchmark's queries by name, the option sets they are crossed with, and the result layouts derived from a case."""
import copy
import functools

from heavydb_amd import capi

OPTS = {
    "kv0": dict(), "kv2": dict(kernel_variant=2), "kv3": dict(kernel_variant=3),
    "kv2_passes": dict(kernel_variant=2, pass_rows=700),   # (several passes of the routes that lay temporary columns)
}


@functools.lru_cache(maxsize=None)
def by_name(scale=1):
    from oracle import oracle as orc
    from tests import cases as cases_mod, proj_cases
    import tests.test_hostsim_flow as flow
    cs = list(cases_mod.build_cases(scale=scale)) + list(proj_cases.build_cases()) + list(proj_cases.build_join_cases())
    cs += [flow._refbench_case(orc, name, 6000 * scale, 600) for name in flow.QUERIES]
    return {c.name: c for c in cs}


def with_layout(case, layout):
    """the case's plan with the stated layout ("rows"), a columnar table ("columnar"), or the COUNT(*)-only form whose
    table has 4-byte slots ("slot4")"""
    ra = copy.copy(case.ra)
    if layout == "columnar":
        ra.output_columnar_hint = capi.OUTPUT_COLUMNAR
    elif layout == "slot4":
        ra.target_exprs = [t for t in case.ra.target_exprs if t.agg in (capi.PROJECT_KEY, capi.COUNT)] or case.ra.target_exprs
        ra.bigint_count = False
        ra.num_tuples = sum(len(f[0]) for f in case.frags)
    out = copy.copy(case)
    out.ra = ra
    return out


def held_to_oracle(case, layout):
    """whether the pinned test also compares the step's table with the oracle's: the case matrix and the benchmark queries in
    a row-wise layout (Projections and columnar tables have checkers of their own: test_projection.py, test_columnar.py)"""
    return hasattr(case, "fp_rtol") and layout != "columnar"


# (case, layout, option set, mi355q_explain's (code, route, scratch bytes), mi355q_execute's (code, kernel_name, variant,
# n_launches, spilled_rows, rows_scanned, algorithmic_bytes)) of the commit before execute_impl became a list of stage
# functions, through the real-kernel host simulation; one or more per stage function
PINNED = [
    ('MSBS001', 'rows', 'kv2_passes', (0, "aggregates of column + literal from the column's aggregates + k_zip_targets > the step grouped by the integer column + k_cast_key_emit > k_pack_keys (entry index, perfect temp) > 2 runs (one per value column) + k_zip_targets, each > k_generic > k_unpack_perfect", 0), (0, 'k_generic', 0, 4, 0, 6000, 72000)),
    ('MSBS001', 'columnar', 'kv2', (0, 'k_project > row-wise twin + k_rows_to_columns > k_pack_keys (FLOAT key widened) > 3 runs (one per value column) + k_zip_targets, each > k_part_scatter + k_part_aggregate > k_unpack_emit', 169890624), (0, 'k_part_scatter', 2, 3, 0, 6000, 72000)),
    ('expr_filter_guarded_div_columnar', 'rows', 'kv0', (0, 'filter compiled (atoms + programs + truth table) > k_filter_mask (program atoms + truth table -> 1 B/row) > k_proj_compact', 6656), (0, 'k_proj_compact', 0, 2, 0, 21000, 336000)),
    ('S001', 'rows', 'kv0', (0, '8-byte-slot twin + k_narrow_slots > k_groupby_lds', 0), (0, 'k_groupby_lds', 4, 1, 0, 6000, 24000)),
    ('join_1n_buffer_full', 'rows', 'kv0', (100, '', 0), (-26427, 'k_proj_compact', 2, 1, 0, 30000, 480000)),
    ('join_no_match_at_all', 'rows', 'kv0', (0, 'join on a dense one-to-one table = range filter on the key > k_scan_agg', 0), (0, 'k_scan_agg', 0, 1, 0, 20000, 320000)),
    ('expr_is_null_in_case_and_uminus_arguments', 'rows', 'kv2', (0, 'k_project > k_pack_keys (entry index, perfect temp) > 4 runs (one per value column) + k_zip_targets, each > k_perfect_lds > k_unpack_perfect', 0), (0, 'k_perfect_lds', 0, 4, 0, 20000, 640000)),
    ('expr_filter_not_equal_columns_nongrouped', 'rows', 'kv2', (0, 'k_project > quals compiled (range atoms + truth table) > k_filter_mask (program atoms + truth table -> 1 B/row) > k_generic', 0), (0, 'k_generic', 0, 2, 0, 20000, 380000)),
    ('expr_join_groupby_expression_target', 'slot4', 'kv2', (0, 'k_project > k_join_gather (inner columns + matched flag as outer columns) > k_perfect_lds', 0), (0, 'k_perfect_lds', 0, 2, 0, 20000, 480000)),
    ('expr_join_groupby_expression_target', 'slot4', 'kv2_passes', (0, 'k_project > k_join_gather (inner columns + matched flag as outer columns) > k_perfect_lds', 0), (0, 'k_perfect_lds', 0, 8, 0, 20000, 480000)),
    ('BH002', 'rows', 'kv3', (0, 'k_project > k_baseline_direct', 0), (0, 'k_baseline_direct', 1, 1, 0, 6000, 48000)),
    ('BH008', 'rows', 'kv2_passes', (0, 'k_pack_keys (bit-packed key) > k_part_scatter + k_part_aggregate > k_unpack_emit', 136336192), (0, 'k_idx_scatter', 7, 5, 0, 6000, 72000)),
    ('count_star_filter_i64', 'rows', 'kv0', (0, 'k_scan_count', 0), (0, 'k_scan_count', 0, 1, 0, 20000, 160000)),
    ('expr_targets_six_wide', 'rows', 'kv0', (0, 'k_proj_compact (expressions in registers)', 6656), (0, 'k_proj_compact', 1, 1, 0, 21000, 336000)),
    ('join_perfect_sum_fact', 'rows', 'kv3', (0, 'k_join_sum', 0), (0, 'k_part_scatter', 3, 1, 0, 20000, 320000)),
    ('expr_overflow_in_a_qual_counts_for_every_row', 'rows', 'kv0', (0, 'k_project > k_scan_agg', 0), (7, '', 0, 0, 0, 0, 0)),
    ('MSPHM006', 'slot4', 'kv2_passes', (0, 'k_idx_scatter + k_idx_aggregate', 18875200), (0, 'k_idx_scatter', 8, 1, 0, 6000, 72000)),
    ('BH002', 'rows', 'kv0', (0, 'k_project > k_groupby_lds', 0), (0, 'k_groupby_lds', 5, 1, 0, 6000, 48000)),
    ('NGA02', 'rows', 'kv0', (0, 'k_scan_agg', 0), (0, 'k_scan_agg', 5, 1, 0, 6000, 144000)),
    ('join_perfect_sum_fact', 'rows', 'kv2_passes', (0, 'k_part_scatter + k_part_join', 136315712), (0, 'k_part_scatter', 2, 1, 0, 20000, 320000)),
    ('join_outer_columns_only', 'rows', 'kv0', (0, 'k_proj_compact (join probe per row)', 6656), (0, 'k_proj_compact', 2, 1, 0, 30000, 600000)),
    ('join_composite_key64_1to1_sum', 'rows', 'kv0', (100, '', 0), (0, 'k_join_sum', 0, 1, 0, 20000, 480000)),
    ('expr_filter_not_over_a_disjunction', 'rows', 'kv0', (0, 'filter compiled (atoms + truth table) > k_scan_agg', 0), (0, 'k_scan_agg', 0, 1, 0, 20000, 400000)),
]
