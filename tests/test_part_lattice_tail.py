"""The tail of the lattice member in the host simulation (the real kernels_part.hip compiled for the CPU, as
tests/test_part_lattice.py runs it): the cases of tests/part_lattice_tail_cases.py at 250 K rows against the oracle.

The emission cases check the VALUES of k_lattice_emit's two paths: blocks run one after the other here, so a race between
the claim and the stores cannot show; the device test runs the same cases for that.

The run-edge case walks runs of 0, 1, a stage - 1, a stage, a stage + 1, two stages and two stages and an odd bit through
the packed walk of k_part_aggregate_idx (clamped loads, the half pair of an odd count, the stage loaded ahead past the end
of a run).  A unit has 8 runs here and 16 waves, so every wave takes at most one run; the device gives a wave sixteen, short
and empty ones in every 1 M-row lattice case and long ones in the 10 B-row parity test of
tests/test_zz_gpu_baseline_sizes.py.
"""
import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests import part_lattice_tail_cases as tail
from tests import test_hostsim_flow as flow
from tests.helpers import check_probe_invariant
from tests.test_part_lattice import check_trace, sim, units_in_trace  # noqa: F401  (sim: the module's fixture)

EMISSION = tail.emission_cases(plc.SIM_ROWS)
TRACE_PACKED = "lattice records: 12 per 128-byte segment"


def _run(oracle, capfd, lc):
    """flow._check compares the table and the rows with the oracle's (compare_buffers, compare_rows)"""
    capfd.readouterr()
    rs = flow._check(oracle, lc.case, flags=capi.OPT_TRACE, **lc.opts)
    err = capfd.readouterr().err
    check_trace(lc, err)
    assert TRACE_PACKED in err, err
    assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
    assert rs.report.n_launches >= lc.min_launches, rs.report.n_launches
    assert rs.report.rows_scanned == plc.SIM_ROWS
    check_probe_invariant(rs.getQueryMemDesc(), rs.getStorage())
    return rs, err


@pytest.mark.parametrize("lc", EMISSION, ids=[c.name for c in EMISSION])
def test_emission_stores_what_the_merge_leaves(sim, oracle, capfd, lc):
    _run(oracle, capfd, lc)


def test_packed_walk_at_the_edges_of_runs_and_stages(sim, oracle, capfd):
    lc, want = tail.run_edge_case()
    stage = tail.pack_stage_records()
    assert {0, 1, stage - 1, stage, stage + 1, 2 * stage, 2 * stage + 21} <= set(want.ravel().tolist())
    assert (2 * stage + 21) % 2 == 1
    rs, err = _run(oracle, capfd, lc)
    assert units_in_trace(err) == tail.SIM_PARTITIONS, err
    assert rs.report.spilled_rows == 0, rs.report.spilled_rows   # no run overflowed: the runs hold the counts asked for
