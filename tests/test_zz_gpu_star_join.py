"""Star joins on the device (k_join_group_code + k_star_groupby_lds, and the flattened route through k_join_gather / k_join_expand,
through the C-ABI): every case of tests/star_join_cases.py — what tests/test_star_join.py runs through the host simulation —
against the oracle on the flattened plan the test builds itself (keys, counts, integer sums, MIN / MAX bit for bit; DOUBLE sums /
AVG within 1e-9 relative) and against SQLite on the query text; every star-shaped case by default, with OPT_NO_STAR_GROUPBY and
with kernel_variant 2, the route and the report's kernel asserted each time.  The tables go to the device once per module."""
from __future__ import annotations

import numpy as np
import pytest

from heavydb_amd import capi
from tests import star_join_cases as sx
from tests.test_gpu_parity import _build_join, _fetch_result, _upload, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from tests.test_star_join import RUN_IDS, RUNS, planned_route, run_one

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_tables(torch_cuda):
    """what the cases share, uploaded / built once: the fact fragments (aligned and 4 bytes off), the two dimensions, the join tables"""
    return {}


def _unaligned_on_device(torch, a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + 32, dtype=torch.uint8).cuda()
    view = buf[4:4 + raw.size]
    view.copy_(torch.from_numpy(raw))
    assert view.data_ptr() % 16 == 4
    return view


def _tables(torch, cache, sc):
    case = sc.case
    key = ("cols", id(case.frags), id(case.inner[0]))
    if key not in cache:
        cache[key] = _upload(torch, case)
    frag_t, inner_t = cache[key]
    if sc.unaligned:
        ukey = ("unaligned", id(case.frags))
        if ukey not in cache:
            cache[ukey] = [[_unaligned_on_device(torch, a) for a in cols] for cols in case.frags]
        frag_t = cache[ukey]
    return frag_t, inner_t


def _join(torch, cache, case):
    key = ("join", id(case.join_keys), case.join_prefer_baseline, case.join_one_to_many)
    if key not in cache:
        cache[key] = _build_join(torch, case)
    return cache[key]


@pytest.mark.parametrize("sc,vid,opts,star_runs", RUNS, ids=RUN_IDS)
def test_star_join_on_the_device(torch_cuda, device_tables, oracle, sc, vid, opts, star_runs):
    torch = torch_cuda

    def make_fetch(c):
        frag_t, inner_t = _tables(torch, device_tables, c)
        from heavydb_amd.executor import FetchResult
        return FetchResult([[int(t.data_ptr()) for t in cols] for cols in frag_t], [len(cols[0]) for cols in c.case.frags],
                           [int(t.data_ptr()) for t in inner_t], int(inner_t[0].numel()), 0, [frag_t, inner_t])

    run_one(oracle, sc, opts, star_runs, make_join=lambda case: _join(torch, device_tables, case), make_fetch=make_fetch)


def test_the_planner_takes_the_star_member_for_a_billion_rows_on_the_device(torch_cuda, device_tables):
    make_join = lambda case: _join(torch_cuda, device_tables, case)  # noqa: E731
    assert sx.STAR_NOTE in planned_route(make_join=make_join)
    route = planned_route(capi.OPT_NO_STAR_GROUPBY, make_join=make_join)
    assert sx.STAR_NOTE not in route and route.startswith(sx.FLAT_NOTE + "k_join_gather"), route
