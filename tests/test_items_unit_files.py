"""CPU tests of lcfir_items_unit_files (include/lcfir.h): the file of every
entry of the fused item launch's per-unit table, a pure function, against a
restatement over lcfir_items_plan and lcfir_items_unit_table; its declaration
in the header and its signature in the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import lcfir
from test_items_units import BS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(B, n, nch):
    """The files with rows in arena order (the plan's offsets, ascending), file
    f repeated nch[f] * ceil(n[f] / B) times."""
    n, nch = np.asarray(n, np.int64), np.asarray(nch, np.int64)
    plan = lcfir.ItemSet.plan(B, n, nch)
    live = [f for f in range(n.size) if plan["file_group"][f] >= 0]
    live.sort(key=lambda f: int(plan["file_offset"][f]))
    out = []
    for f in live:
        out += [f] * (int(nch[f]) * -(-int(n[f]) // B))
    return np.array(out, np.int32), plan


def check(B, n, nch):
    n, nch = np.asarray(n, np.int64), np.asarray(nch, np.int32)
    got = lcfir.ItemSet.unit_files(B, n, nch)
    want, plan = restate(B, n, nch)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # the unit table's total and order: entry u's row lies inside the block the plan gives file[u]
    table = lcfir.ItemSet.unit_table(B, n, nch)
    assert got.size == table.size == int(np.sum(nch.astype(np.int64) * -(-n // B)))
    lo = plan["file_offset"][got]
    hi = lo + nch[got].astype(np.int64) * plan["file_stride"][got]
    assert np.all((lo <= table["off"]) & (table["off"] < hi))
    assert np.array_equal(table["n"], n[got].astype(np.int32))
    # files without rows contribute nothing, every other file is there
    assert set(got.tolist()) == {f for f in range(n.size) if n[f] > 0 and nch[f] > 0}
    return got


@pytest.mark.parametrize("B", BS)
def test_boundary_lengths(B):
    n = [0, 1, B - 1, B, B + 1, 5, 2 * B, 2 * B + 1, 3 * B - 1, 7, B, 0]
    nch = [2, 1, 2, 3, 1, 0, 2, 1, 3, 2, 0, 0]
    got = check(B, n, nch)
    assert got.size == 1 + 2 + 3 + 2 + 4 + 3 + 9 + 2
    assert np.bincount(got, minlength=12).tolist() == [0, 1, 2, 3, 2, 0, 4, 3, 9, 2, 0, 0]
    assert check(B, [], []).size == 0
    assert check(B, [0, 9], [3, 0]).size == 0  # n = 0 or nch = 0: no entry


@pytest.mark.parametrize("seed", range(6))
def test_seeded_random_lists(seed):
    rng = np.random.default_rng(100 + seed)
    B = BS[seed % len(BS)]
    nf = int(rng.integers(1, 60))
    n = rng.integers(0, 5 * B, nf)
    n[rng.integers(0, nf, 3)] = rng.choice([0, 1, B - 1, B, B + 1], 3)
    nch = rng.integers(0, 5, nf)
    check(B, n, nch)


def test_cap_too_small_is_reported_without_writing():
    lib = lcfir.load()
    n = np.array([10000, 3], np.int64)
    nch = np.array([2, 1], np.int32)
    total = ctypes.c_int64(-1)
    buf = np.full(8, -7, np.int32)
    rc = lib.lcfir_items_unit_files(4096, 2, n.ctypes.data, nch.ctypes.data, ctypes.byref(total), buf.ctypes.data, 6)
    assert rc == lcfir.EINVAL and total.value == 7 and b"cap" in lib.lcfir_last_error()
    assert np.all(buf == -7)
    with pytest.raises(lcfir.LcfirError):
        lcfir.ItemSet.unit_files(4096, n, nch, cap=6)
    # arena order: the one-unit file (k = 1) before the three-unit one
    assert lcfir.ItemSet.unit_files(4096, n, nch, cap=9).tolist() == [1] + [0] * 6
    rc = lib.lcfir_items_unit_files(4096, 2, n.ctypes.data, nch.ctypes.data, ctypes.byref(total), None, 0)
    assert rc == lcfir.EINVAL and total.value == 7
    assert lib.lcfir_items_unit_files(4096, 2, n.ctypes.data, nch.ctypes.data, None, None, 0) == lcfir.EINVAL
    assert lib.lcfir_items_unit_files(0, 2, n.ctypes.data, nch.ctypes.data, ctypes.byref(total), None, 0) \
        == lcfir.EINVAL
    big, one = np.array([2**31], np.int64), np.array([1], np.int32)
    assert lib.lcfir_items_unit_files(4096, 1, big.ctypes.data, one.ctypes.data, ctypes.byref(total), None, 0) \
        == lcfir.EINVAL
    assert b"frames" in lib.lcfir_last_error()


def test_the_header_declares_and_the_binding_binds_it():
    text = open(os.path.join(ROOT, "include", "lcfir.h")).read()
    assert re.search(r"^int lcfir_items_unit_files\(", text, re.M)
    assert "lcfir_items_unit_files" in lcfir.header_symbols()
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    assert lcfir._SIGNATURES["lcfir_items_unit_files"] == ([i64, i32, vp, vp, ctypes.POINTER(i64), vp, i64],
                                                          ctypes.c_int)
    assert callable(lcfir.ItemSet.unit_files)
