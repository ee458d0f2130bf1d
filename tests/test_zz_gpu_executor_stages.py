"""The pinned step-executor cases (tests/stage_cases.py) on the device, against the oracle: the executor's stage functions —
workspace growth and reuse, the fragment-table upload, the stream choice, the routes, the families — meet the real runtime,
with fragments of 10^4 - 10^5 rows.  Which member ran is pinned on the CPU (test_executor_stages_are_the_pinned_ones): the
device has other CU counts and plans accordingly, so here only the result is held to the oracle."""
import pytest

from heavydb_amd import capi
from tests import stage_cases
from tests.helpers import compare_buffers, compare_rows, qmd_equal
from tests.test_gpu_parity import _build_join, _fetch_result, _oracle_join, _upload, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

SCALE = 4
STEPS = sorted({(name, layout, opts) for name, layout, opts, _, rep in stage_cases.PINNED
                if rep[0] == 0 and stage_cases.held_to_oracle(stage_cases.by_name()[name], layout)})


@pytest.mark.parametrize("name,layout,opts_name", STEPS, ids=["-".join(s) for s in STEPS])
def test_pinned_executor_steps_match_the_oracle(torch_cuda, oracle, name, layout, opts_name):  # noqa: F811
    from heavydb_amd.executor import Executor
    case = stage_cases.with_layout(stage_cases.by_name(SCALE)[name], layout)
    opts = dict(stage_cases.OPTS[opts_name])
    if "pass_rows" in opts:
        opts["pass_rows"] *= SCALE
    q, want, code = oracle.execute(case.ra.to_plan(), case.frags, case.inner, _oracle_join(oracle, case), n_threads=2)
    assert code == 0
    frag_t, inner_t = _upload(torch_cuda, case)
    hj, keep = _build_join(torch_cuda, case)
    case.ra.join_table = hj
    try:
        ex = Executor(0)
        fr = _fetch_result(case, frag_t, inner_t)
        for _ in range(2):   # the second call runs on the workspace the first one grew
            rs = ex.executeWorkUnit(case.ra, fr, allow_retry=False, **opts)
            qmd_equal(q, rs.getQueryMemDesc())
            compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
            assert rs.rowCount() == oracle.row_count(q, want)
            compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), case.fp_rtol)
        rs_async, pend = ex.executeWorkUnitAsync(case.ra, fr, **{k: v for k, v in opts.items() if k != "pass_rows"})
        done = pend.wait()
        compare_buffers(q, want, done.getStorage(), case.fp_rtol)
    finally:
        case.ra.join_table = None
