"""SEMI and ANTI join levels on the device (k_join_exists_mask, fast and general member, then the joinless plan on `mask = 1`
in whichever family takes it, through the C-ABI): every case of tests/semi_join_cases.py — what tests/test_semi_join.py runs
through the host simulation — as SEMI and as ANTI, by default and with kernel_variant 2, against the oracle on the masked
joinless plan the cases file builds with numpy alone (keys, counts, integer sums, MIN / MAX bit for bit; DOUBLE sums / AVG
within 1e-9 relative) and against SQLite on the query text; the descriptor and the route asserted each time.  The tables go to
the device once per module."""
from __future__ import annotations

import numpy as np
import pytest

from heavydb_amd import capi
from heavydb_amd.executor import Executor, FetchResult
from tests import semi_join_cases as sj
from tests.test_gpu_parity import _build_join, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from tests.test_semi_join import RUN_IDS, RUNS, run_one
from tests.test_zz_gpu_star_join import _unaligned_on_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_tables(torch_cuda):
    """what the cases share, uploaded / built once: the fact fragments (aligned and 4 bytes off) and the join tables"""
    return {}


def _frags(torch, cache, unaligned):
    key = ("frags", unaligned)
    if key not in cache:
        up = (lambda a: _unaligned_on_device(torch, a)) if unaligned else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
        cache[key] = [[up(a) for a in cols] for cols in sj.FRAGS]
    return cache[key]


def _join(torch, cache, sc, case):
    if sc.dim.name not in cache:
        cache[sc.dim.name] = _build_join(torch, case)
    return cache[sc.dim.name]


def _device_run(torch, cache, oracle, sc, kind, opts):
    def make_fetch(c, case):
        frag_t = _frags(torch, cache, c.unaligned)
        return FetchResult([[int(t.data_ptr()) for t in cols] for cols in frag_t], [len(cols[0]) for cols in sj.FRAGS], [], 0, 0, [frag_t])

    return run_one(oracle, sc, kind, opts, make_join=lambda case: _join(torch, cache, sc, case), make_fetch=make_fetch)


@pytest.mark.parametrize("sc,kind,vid,opts", RUNS, ids=RUN_IDS)
def test_semi_and_anti_joins_on_the_device(torch_cuda, device_tables, oracle, sc, kind, vid, opts):
    _device_run(torch_cuda, device_tables, oracle, sc, kind, opts)


def test_the_general_member_agrees_with_the_fast_member_on_the_device(torch_cuda, device_tables, oracle):
    """OPT_LDS_GENERIC_MEMBER (the typed members' A/B switch) sends a fast-member shape to the general member"""
    for name in ("few_groups", "many_non_grouped", "int32_key"):
        sc = next(c for c in sj.CASES if c.name == name)
        for _, kind in sj.KINDS:
            case = sj.stated(sc, kind)
            hj, keep = _join(torch_cuda, device_tables, sc, case)
            case.ra.join_table = hj
            frag_t = _frags(torch_cuda, device_tables, False)
            fr = FetchResult([[int(t.data_ptr()) for t in cols] for cols in frag_t], [len(cols[0]) for cols in sj.FRAGS], [], 0, 0, [frag_t])
            rs = Executor(0).executeWorkUnit(case.ra, fr, allow_retry=False, flags=capi.OPT_LDS_GENERIC_MEMBER)
            sj.check_result(oracle, sc, kind, rs)


def test_the_planner_restates_the_one_measured_class_as_the_inner_join(torch_cuda):
    """non-grouped SEMI over a one-to-one table of 100 M slots and a large input: the INNER plan (k_part_join) by default, the mask
    route under a forced kernel_variant, for ANTI, for a grouped step and for a 1 M-slot table.  Plans only."""
    import os
    if os.environ.get("MI355Q_HOSTSIM"):
        pytest.skip("a 100 M-slot join table is no size for the host simulation")
    from heavydb_amd.executor import ExpressionRange, HashJoin
    torch = torch_cuda
    rows = [250_000_000] * 4
    from heavydb_amd.executor import InputColDescriptor, RelAlgExecutionUnit, TargetExpr
    descs = [InputColDescriptor(capi.INT64, False, ExpressionRange(True, 0, 124_999_999)), InputColDescriptor(capi.INT64, False, ExpressionRange(True, 0, 999)),
             InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 999))]
    ng = RelAlgExecutionUnit(descs, [TargetExpr(capi.SUM, 1), TargetExpr(capi.COUNT)], join_outer_col=0, num_tuples=10**9)
    few = RelAlgExecutionUnit(descs, [TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.SUM, 1)], [], [2], join_outer_col=0,
                              num_tuples=10**9)
    for slots, restated in ((100_000_000, True), (1_000_000, False)):
        keys = torch.arange(slots, dtype=torch.int64).cuda()
        keys = keys[keys % 16 != 0]          # (holes: a dense table's INNER join is a range filter on the key)
        hj = HashJoin.getInstance(int(keys.data_ptr()), int(keys.numel()), capi.INT64, ExpressionRange(True, 0, slots - 1))
        try:
            ng.join_table = few.join_table = hj
            ng.join_kind = few.join_kind = capi.JOIN_SEMI
            route = Executor(0).explain(ng, rows)
            assert route.startswith("semi join"), route
            assert ("as the INNER join" in route and "k_part_join" in route) == restated, route
            assert (sj.KERNEL in route) == (not restated), route
            assert sj.KERNEL in Executor(0).explain(ng, rows, kernel_variant=2)
            assert sj.KERNEL in Executor(0).explain(few, rows)
            ng.join_kind = capi.JOIN_ANTI
            assert sj.KERNEL in Executor(0).explain(ng, rows)
        finally:
            ng.join_table = few.join_table = None
            hj.free()
            del keys
