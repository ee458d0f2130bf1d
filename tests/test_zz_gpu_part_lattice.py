"""The partitioned GROUP BY's lattice member on the device: every case of tests/part_lattice_cases.py at 1 M rows against
the oracle, with the member and with MI355Q_OPT_NO_LATTICE_PART, and the two against each other; the TRACE line says which
phase-2 member ran."""
import numpy as np
import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests.helpers import check_probe_invariant, compare_buffers, compare_rows, qmd_equal
from tests.test_part_lattice import check_trace, units_in_trace

pytestmark = pytest.mark.gpu

DEVICE_PARTITIONS = 256   # P of a 40 K-entry table on 256 CUs
CASES = plc.build_cases(DEVICE_PARTITIONS, plc.DEVICE_ROWS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load_library()
    return torch


@pytest.fixture(scope="module")
def references(oracle):
    """the oracle's table of every case, computed once"""
    memo = {}

    def get(lc):
        if lc.name not in memo:
            q, want, code = oracle.execute(lc.case.ra.to_plan(), lc.case.frags, [], None, n_threads=8)
            assert code == 0
            memo[lc.name] = (q, want, oracle.fetch_rows(q, want), oracle.row_count(q, want))
        return memo[lc.name]
    return get


def _run(torch, lc, frag_t, flags):
    from heavydb_amd.executor import Executor, FetchResult
    bufs = [[int(t.data_ptr()) for t in cols] for cols in frag_t]
    rows = [int(cols[0].numel()) for cols in frag_t]
    fr = FetchResult(bufs, rows, [], 0, 0, [frag_t])
    return Executor(0).executeWorkUnit(lc.case.ra, fr, allow_retry=False, flags=flags, **lc.opts)


@pytest.mark.parametrize("lc", CASES, ids=[c.name for c in CASES])
def test_lattice_member_on_the_device(torch_cuda, references, capfd, lc):
    torch = torch_cuda
    q, want, want_rows, want_count = references(lc)
    frag_t = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cols] for cols in lc.case.frags]
    capfd.readouterr()
    rs = _run(torch, lc, frag_t, capi.OPT_TRACE)
    err = capfd.readouterr().err
    check_trace(lc, err)
    if lc.member is not None:
        assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
        assert rs.report.n_launches >= lc.min_launches, rs.report.n_launches
        assert rs.report.rows_scanned == plc.DEVICE_ROWS
    if lc.name == "few_points_per_unit":
        assert units_in_trace(err) == DEVICE_PARTITIONS, err
    qmd_equal(q, rs.getQueryMemDesc())
    compare_buffers(q, want, rs.getStorage(), lc.case.fp_rtol)
    assert rs.rowCount() == want_count
    if lc.max_groups is not None:
        assert rs.rowCount() < lc.max_groups, rs.rowCount()
    compare_rows(q, want_rows, rs.fetch(), lc.case.fp_rtol)
    check_probe_invariant(rs.getQueryMemDesc(), rs.getStorage())
    plain = _run(torch, lc, frag_t, capi.OPT_TRACE | capi.OPT_NO_LATTICE_PART)
    err = capfd.readouterr().err
    assert plc.TRACE_IDX not in err and plc.TRACE_GAVE_UP not in err, err
    compare_buffers(q, want, plain.getStorage(), lc.case.fp_rtol)
    check_probe_invariant(plain.getQueryMemDesc(), plain.getStorage())
    assert plain.report.kernel_name == rs.report.kernel_name and plain.report.variant == rs.report.variant
    compare_rows(q, plain.fetch(), rs.fetch(), lc.case.fp_rtol)
