"""Inputs of the lattice member's exact-division index (heavydb_amd/csrc/lattice_index.h, evaluated per record by
k_part_scatter MODE 3 / 4), shared by the host simulation (tests/test_part_lattice_index.py, 250 K rows) and the device
(tests/test_zz_gpu_part_lattice_index.py, 1 M rows).

Built with tests/part_lattice_cases.py's `_build` (four fragments, the cfg3f filter, kernel_variant 2).  The index is
q = low32(low32(d >> z) x inv) for stride = 2^z x odd, accepted when q < card and q x stride == d; every case is the
smallest input that reaches one way this can go wrong: an even stride with an odd part, a shift of 20 and one of 40 (>= 32),
a stride with a high word; and keys that are NOT lattice points in each way the test of the index could miss them.  Each
runs packed (the default), with MI355Q_OPT_NO_LATTICE_PACK and in the oracle.
"""
from __future__ import annotations

import numpy as np

from tests.part_lattice_cases import _build

SUPER_TILE = 12 * 64 * 4   # rows one scatter workgroup takes in one step (12 producer waves x 64 lanes x 4 rows)


def _both_ends(rng, card, n):
    idx = rng.integers(0, card, n)
    idx[:2] = [0, card - 1]
    return idx


def _refragment(lc, sizes):
    """the case's rows in fragments of `sizes` rows and the rest"""
    cols = [np.concatenate([f[c] for f in lc.case.frags]) for c in range(len(lc.case.frags[0]))]
    n = len(cols[0])
    cuts = [0] + list(np.cumsum(sizes)) + [n]
    assert cuts[-2] <= n
    lc.case.frags = [[np.ascontiguousarray(col[a:b]) for col in cols] for a, b in zip(cuts[:-1], cuts[1:])]
    return lc


def build_cases(n_rows: int):
    n = n_rows
    cases = []
    rng = np.random.default_rng(20263)

    # ---- strides the division must get right, both ends of every lattice present
    # z = 1 and an odd part that is not 1, a negative minimum
    cases.append(_build("stride_6000018_negative_min", _both_ends(rng, 60_001, n), 6_000_018, -(10**12) - 11, 60_001, "idx", rng=rng))
    # z = 20, odd part 3
    cases.append(_build("stride_3_x_2_20", _both_ends(rng, 120_000, n), 3 << 20, 7, 120_000, "idx", rng=rng))
    # a stride with a high word: the product q x stride needs its second multiply
    cases.append(_build("stride_2_33_plus_9", _both_ends(rng, 100_000, n), 2**33 + 9, 7, 100_000, "idx", rng=rng))
    # a shift of 32 or more: the index comes from the high word of d alone
    cases.append(_build("stride_2_40_negative_min", _both_ends(rng, 100_000, n), 2**40, -(2**50), 100_000, "idx", rng=rng))

    # ---- one key that is no lattice point of the range, in the last fragment, on a row that passes the filter: the member
    # gives up and the plain member computes the step
    def one_key(at, f):
        def override(key):
            key = key.copy()
            key[at] = f(int(key[at]))
            return key
        return override
    row = n - 5
    card = 50_000
    for name, stride, f in [
            # divisible by 2^z but not by the odd part
            ("off_by_2", 6_000_018, lambda k: k + 2),
            # divisible by the odd part but not by 2^z
            ("off_by_the_odd_part", 6_000_018, lambda k: k + 3_000_009),
            # a lattice point 2^32 indexes beyond: the low 32 bits of its quotient are an index of the range
            ("index_aliases_mod_2_32", 1_000_003, lambda k: k + 2**32 * 1_000_003),
            # the lattice point before the first and the one after the last
            ("below_the_minimum", 1_000_003, lambda k: 7 - 1_000_003),
            ("past_the_maximum", 1_000_003, lambda k: 7 + card * 1_000_003)]:
        cases.append(_build(name, rng.integers(0, card, n), stride, 7, card, "gave_up", rng=rng,
                            key_override=one_key(row, f), pass_row=row))

    # ---- ragged tiles: fragments of a single row, three rows (less than a quad), none, one row short of a super-tile,
    # exactly one, one more, and the rest.  (The stride is sampled from the first fragment that has rows: its one key is the
    # lattice's second point.)
    idx = rng.integers(0, card, n)
    idx[0] = 1
    lc = _build("ragged_tiles", idx, 1_000_003, 7, card, "idx", rng=rng)
    cases.append(_refragment(lc, [1, 3, 0, SUPER_TILE - 1, SUPER_TILE, SUPER_TILE + 1]))
    return cases
