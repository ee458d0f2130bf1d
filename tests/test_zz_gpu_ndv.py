"""The NDV estimate (k_ndv_hll) and the join tables sized by it on the device: the cases of tests/ndv_cases.py against
its numpy restatement — registers bit for bit, the estimate within 1 — and, for the tables, the oracle on a table of
the entry count the product reports.  Also passes under MI355Q_HOSTSIM=real."""
import ctypes as C
import os

import numpy as np
import pytest

from heavydb_amd import capi
from tests import ndv_cases as nc
from tests import test_gpu_parity as gp

pytestmark = pytest.mark.gpu

CASES = nc.build_cases()
SIMULATED = os.environ.get("MI355Q_HOSTSIM") in ("1", "real")


class TorchMem:
    """device memory through torch tensors"""

    def __init__(self, torch):
        self.torch = torch

    def put(self, a, offset=0):
        a = np.ascontiguousarray(a)
        if a.size == 0:
            t = self.torch.zeros(16, dtype=self.torch.uint8, device="cuda")   # (an empty tensor has no address)
            return t, int(t.data_ptr())
        if offset:
            assert offset % a.dtype.itemsize == 0
            lead = offset // a.dtype.itemsize
            t = self.torch.from_numpy(np.concatenate([np.zeros(lead, a.dtype), a])).cuda()[lead:]
            assert int(t.data_ptr()) % 16 == offset
            return t, int(t.data_ptr())
        t = self.torch.from_numpy(a).cuda()
        return t, int(t.data_ptr())

    def zeros_u32(self, n):
        t = self.torch.zeros(n, dtype=self.torch.int32, device="cuda")
        return t, int(t.data_ptr())

    def get_u32(self, handle):
        self.torch.cuda.synchronize()
        return handle.cpu().numpy().view(np.uint32).copy()

    def read(self, ptr, nbytes):
        if SIMULATED:
            return C.string_at(ptr, nbytes)
        out = np.empty(nbytes, np.uint8)
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
        return out.tobytes()


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load_library()
    return TorchMem(torch)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_ndv_case_on_the_device(mem, case):
    nc.check_case(mem, case)


@pytest.mark.parametrize("bits", [0, 4, 13])
def test_registers_accumulate_on_the_device(mem, bits):
    nc.check_accumulation(mem, nc.big_case("all", bits))


def test_hostile_specs_on_the_device(mem):
    nc.check_hostile(capi.load_library())


@pytest.mark.parametrize("which", ["one_to_many", "composite"])
def test_join_table_sized_by_the_estimate_on_the_device(mem, oracle, which):
    jc = nc.one_to_many_case() if which == "one_to_many" else nc.composite_case()
    nc.check_ndv_sized_table(oracle, mem, jc, smaller_than_rows=which == "one_to_many")
    # the table the existing helpers build (keyed_entry_count 0) is the default 2 x rows, and the oracle's with it
    hj, keep = gp._build_join(mem.torch, jc.agg)
    assert hj.info()["entry_count"] == 2 * jc.rows == gp._oracle_join(oracle, jc.agg).info()["entry_count"]


def test_a_full_table_is_rebuilt_at_the_default_size_on_the_device(mem, oracle):
    nc.check_fallback(oracle, mem)


def test_other_entry_counts_are_as_before_on_the_device(mem):
    nc.check_other_counts_are_as_before(mem)
