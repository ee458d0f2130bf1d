"""k_lattice_emit's claim-and-store emission on the device: the emission cases of tests/part_lattice_tail_cases.py at 1 M
rows against the oracle (compare_buffers, compare_rows, check_probe_invariant).  Every case runs twice on the same
inputs: a race between a lane's claim of a row and its plain stores need not show in one run, and the sequential host
simulation (tests/test_part_lattice_tail.py) cannot show it at all.

The packed walk of k_part_aggregate_idx gets no case of its own here: a 1 M-row input never fills a stage on the device
(256 x 256 runs, about six records each).  Its run and stage edges are walked in the host simulation
(tests/test_part_lattice_tail.py); runs of many stages on the device are the 10 B-row parity test of
tests/test_zz_gpu_baseline_sizes.py.
"""
import numpy as np
import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests import part_lattice_tail_cases as tail
from tests.helpers import check_probe_invariant, compare_buffers, compare_rows, qmd_equal
from tests.test_part_lattice import check_trace

pytestmark = pytest.mark.gpu

CASES = tail.emission_cases(plc.DEVICE_ROWS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load_library()
    return torch


@pytest.mark.parametrize("lc", CASES, ids=[c.name for c in CASES])
def test_emission_on_the_device_twice(torch_cuda, oracle, capfd, lc):
    from heavydb_amd.executor import Executor, FetchResult
    torch = torch_cuda
    q, want, code = oracle.execute(lc.case.ra.to_plan(), lc.case.frags, [], None, n_threads=8)
    assert code == 0
    want_rows, want_count = oracle.fetch_rows(q, want), oracle.row_count(q, want)
    frag_t = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cols] for cols in lc.case.frags]
    fr = FetchResult([[int(t.data_ptr()) for t in cols] for cols in frag_t], [int(cols[0].numel()) for cols in frag_t],
                     [], 0, 0, [frag_t])
    for _ in range(2):
        capfd.readouterr()
        rs = Executor(0).executeWorkUnit(lc.case.ra, fr, allow_retry=False, flags=capi.OPT_TRACE, **lc.opts)
        check_trace(lc, capfd.readouterr().err)
        assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
        assert rs.report.n_launches >= lc.min_launches, rs.report.n_launches
        assert rs.report.rows_scanned == plc.DEVICE_ROWS
        qmd_equal(q, rs.getQueryMemDesc())
        compare_buffers(q, want, rs.getStorage(), lc.case.fp_rtol)
        assert rs.rowCount() == want_count
        compare_rows(q, want_rows, rs.fetch(), lc.case.fp_rtol)
        check_probe_invariant(rs.getQueryMemDesc(), rs.getStorage())
