"""The NDV estimate and the join tables sized by it on the CPU: k_ndv_hll (kernels_generic.hip) and the host code of
api_join.cpp compiled into both host simulations (tests/hostsim), against the numpy restatement of tests/ndv_cases.py.
The same cases run on the device in tests/test_zz_gpu_ndv.py."""
import ctypes as C

import numpy as np
import pytest

from heavydb_amd import capi
from tests import ndv_cases as nc
from tests.helpers import hostsim_lib

CASES = nc.build_cases()
MEM = nc.HostMem()


@pytest.fixture(scope="module", params=[False, True], ids=["hostsim", "hostsim_real"])
def sim(request):
    lib = capi.load_library(hostsim_lib(request.param))
    lib.hostsim_live_allocations.restype = C.c_int
    saved = capi._lib
    capi._lib = lib
    yield lib
    capi._lib = saved


def test_the_restatement_on_hand_computed_values():
    """MurmurHash64A of the 4 bytes 01 00 00 00 and of the 8 bytes 01 00 .. 00, seed 0, worked step by step with Python
    integers; ranks and the estimate's two branches from the definitions"""
    m, mask = nc.MUL, nc.MASK

    def fin(h):
        h ^= h >> 47
        h = (h * m) & mask
        return h ^ (h >> 47)
    assert int(nc.murmur64a([np.array([1], np.int32)])[0]) == fin((((4 * m) & mask) ^ 1) * m & mask)
    k = m
    k ^= k >> 47
    k = (k * m) & mask
    assert int(nc.murmur64a([np.array([1], np.int64)])[0]) == fin(((((8 * m) & mask) ^ k) * m) & mask)
    # (INT32 -1, INT16 -1): sign-extended 4-byte components FFFFFFFF FFFFFFFF = one block of all ones
    k = (mask * m) & mask
    k ^= k >> 47
    k = (k * m) & mask
    assert int(nc.murmur64a([np.array([-1], np.int32), np.array([-1], np.int16)])[0]) == fin(((((8 * m) & mask) ^ k) * m) & mask)
    assert nc.clz64(np.array([0, 1, 2**63, 2**40 + 5], np.uint64)).tolist() == [64, 63, 0, 23]
    regs = np.zeros(2048, np.uint32)
    assert nc.estimate(regs) == 0
    regs[5] = 9
    assert nc.estimate(regs) == 1                      # 2048 ln(2048 / 2047) = 1.0002
    regs[:] = 10                                       # no zero register: 0.7213 / (1 + 1.079 / 2048) x 2048 x 2^10
    assert nc.estimate(regs) == int(0.7213 / (1 + 1.079 / 2048) * 2048 * 1024)
    assert nc.unmix_block(int(nc.murmur64a([np.array([123456789], np.int64)])[0])) == 123456789


@pytest.mark.parametrize("which,distinct", [("few", 1000), ("all", nc.BIG_N)])
def test_the_restatement_is_accurate_for_the_fixed_seeds(which, distinct):
    """|restated ndv - exact distinct| <= 4 x 1.04 / sqrt(M) x distinct at b = 11"""
    case = nc.big_case(which, 0)
    assert exact_distinct(case) == distinct
    ndv = nc.estimate(nc.registers(case.frags, case.types, case.nullables, 11))
    print(which, "restated ndv", ndv, "exact", distinct)
    assert abs(ndv - distinct) <= 4 * 1.04 / np.sqrt(2048) * distinct
    # both branches of the estimate are taken: linear counting for the few, the raw estimate for the many
    regs = nc.registers(case.frags, case.types, case.nullables, 11)
    assert (np.count_nonzero(regs == 0) > 0) == (which == "few")


def exact_distinct(case):
    return nc.exact_distinct(case.frags, case.types, case.nullables)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_ndv_case_on_the_host_simulation(sim, case):
    nc.check_case(MEM, case)


@pytest.mark.parametrize("bits", [0, 4, 13])
def test_registers_accumulate_on_the_host_simulation(sim, bits):
    nc.check_accumulation(MEM, nc.big_case("all", bits))


def test_hostile_specs_on_the_host_simulation(sim):
    nc.check_hostile(sim, sim.hostsim_live_allocations)


def test_hostile_specs_answer_before_the_device_is_touched():
    """the product library on a machine that may have no GPU: the codes of the checks, not MI355Q_ERR_HIP"""
    nc.check_hostile(capi.load_library())


def test_abi_sizes_are_untouched():
    lib = capi.load_library()
    assert lib.mi355q_abi_version() == 7
    # (mi355q_abi_sizeof answers for the six structs it always has; the new spec is not among them)
    assert [lib.mi355q_abi_sizeof(i) for i in range(8)] == [-1] + [C.sizeof(s) for s in (
        capi.Plan, capi.QMD, capi.Inputs, capi.ExecOptions, capi.ExecReport, capi.JoinSpec)] + [-1]
    assert C.sizeof(capi.NdvSpec) == 64


@pytest.mark.parametrize("which", ["one_to_many", "composite"])
def test_join_table_sized_by_the_estimate_on_the_host_simulation(sim, oracle, which):
    jc = nc.one_to_many_case() if which == "one_to_many" else nc.composite_case()
    nc.check_ndv_sized_table(oracle, MEM, jc, smaller_than_rows=which == "one_to_many")


def test_a_full_table_is_rebuilt_at_the_default_size_on_the_host_simulation(sim, oracle):
    nc.check_fallback(oracle, MEM)


def test_other_entry_counts_are_as_before_on_the_host_simulation(sim):
    nc.check_other_counts_are_as_before(MEM)
