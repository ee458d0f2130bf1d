"""The lattice member's exact-division index on the device: every case of tests/part_lattice_index_cases.py at 1 M rows
three ways — packed records (the default), MI355Q_OPT_NO_LATTICE_PACK (the 16-byte records) and the oracle — both device
runs against the oracle and against each other; the TRACE lines say whether the member ran or gave up."""
import numpy as np
import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests import part_lattice_index_cases as pic
from tests.helpers import check_probe_invariant, compare_buffers, compare_rows, qmd_equal
from tests.test_part_lattice import check_trace
from tests.test_part_lattice_pack import check_record_format

pytestmark = pytest.mark.gpu

CASES = pic.build_cases(plc.DEVICE_ROWS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load_library()
    return torch


def _run(torch, lc, frag_t, flags):
    from heavydb_amd.executor import Executor, FetchResult
    bufs = [[int(t.data_ptr()) for t in cols] for cols in frag_t]
    rows = [int(cols[0].numel()) for cols in frag_t]
    fr = FetchResult(bufs, rows, [], 0, 0, [frag_t])
    return Executor(0).executeWorkUnit(lc.case.ra, fr, allow_retry=False, flags=flags, **lc.opts)


@pytest.mark.parametrize("lc", CASES, ids=[c.name for c in CASES])
def test_exact_division_index_on_the_device(torch_cuda, oracle, capfd, lc):
    torch = torch_cuda
    q, want, code = oracle.execute(lc.case.ra.to_plan(), lc.case.frags, [], None, n_threads=8)
    assert code == 0
    want_rows, want_count = oracle.fetch_rows(q, want), oracle.row_count(q, want)
    frag_t = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cols] for cols in lc.case.frags]
    runs = []
    for packed in (True, False):
        capfd.readouterr()
        rs = _run(torch, lc, frag_t, capi.OPT_TRACE | (0 if packed else capi.OPT_NO_LATTICE_PACK))
        err = capfd.readouterr().err
        check_trace(lc, err)
        check_record_format(lc, err, packed)
        assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
        assert rs.report.rows_scanned == plc.DEVICE_ROWS
        qmd_equal(q, rs.getQueryMemDesc())
        compare_buffers(q, want, rs.getStorage(), lc.case.fp_rtol)
        assert rs.rowCount() == want_count
        compare_rows(q, want_rows, rs.fetch(), lc.case.fp_rtol)
        check_probe_invariant(rs.getQueryMemDesc(), rs.getStorage())
        runs.append(rs)
    packed, wide = runs
    assert wide.report.kernel_name == packed.report.kernel_name and wide.report.variant == packed.report.variant
    assert wide.report.n_launches == packed.report.n_launches
    compare_rows(q, wide.fetch(), packed.fetch(), lc.case.fp_rtol)
