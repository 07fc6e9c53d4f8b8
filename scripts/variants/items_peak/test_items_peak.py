"""CPU tests of the item sets' fused per-file peak, host side (include/lcfir.h):
lcfir_items_unit_files, a pure function, against a restatement over
lcfir_items_plan and lcfir_items_unit_table; the three new entry points in the
header and the binding; batch.ItemBatch's fuse_peak; and the peak-carrying item
kernels in the last build's resource remarks."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch
import check_resources
import lcfir
from test_items_batch import StubBackend, make_files
from test_items_units import BS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMARKS = os.path.join(ROOT, "audio-fir-filter_amd", "liblcfir.remarks")
NEW = ["lcfir_items_unit_files", "lcfir_items_set_peak_fusion", "lcfir_items_peak_launches"]


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
    # files without rows contribute nothing
    assert all(n[f] > 0 and nch[f] > 0 for f in set(got.tolist()))
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


def test_the_header_declares_and_the_binding_binds_the_three_functions():
    text = open(os.path.join(ROOT, "include", "lcfir.h")).read()
    for name in NEW:
        assert re.search(rf"^int {name}\(", text, re.M), name
        assert name in lcfir.header_symbols() and name in lcfir._SIGNATURES, name
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    assert lcfir._SIGNATURES["lcfir_items_unit_files"] == ([i64, i32, vp, vp, ctypes.POINTER(i64), vp, i64],
                                                          ctypes.c_int)
    assert lcfir._SIGNATURES["lcfir_items_set_peak_fusion"] == ([vp, ctypes.c_int], ctypes.c_int)
    assert lcfir._SIGNATURES["lcfir_items_peak_launches"] == ([vp, ctypes.POINTER(i32)], ctypes.c_int)
    lib = lcfir.load()
    assert lib.lcfir_items_set_peak_fusion(None, 1) == lcfir.EINVAL
    assert lib.lcfir_items_peak_launches(None, None) == lcfir.EINVAL
    for m in ("set_peak_fusion", "peak_launches", "unit_files"):
        assert callable(getattr(lcfir.ItemSet, m))


class PeakStub(StubBackend):
    def set_peak_fusion(self, on):
        self.calls.append(("peak_fusion", on))


def test_item_batch_switches_peak_fusion_on_only_when_asked():
    be = PeakStub()
    ib = batch.ItemBatch(be, make_files(), fuse_peak=True)
    assert ib.fuse_peak is True and be.calls[0] == ("peak_fusion", True)  # before the arena is loaded
    ib.step()
    assert [c for c in be.calls if isinstance(c, tuple) and c[0] == "peak_fusion"] == [("peak_fusion", True)]
    be = PeakStub()
    ib = batch.ItemBatch(be, make_files())
    ib.step()
    assert ib.fuse_peak is False and not any(isinstance(c, tuple) and c[0] == "peak_fusion" for c in be.calls)
    # a backend written before the switch: the base class's no-op
    assert batch.ItemBackend().set_peak_fusion(True) is None
    batch.ItemBatch(StubBackend(), make_files(), fuse_peak=True).step()


def test_peak_item_entry_points_in_the_build_remarks():
    """The peak-carrying item form has entry points of its own, one instance
    per output mode that rounds to f32 (general, last, zero-phase = 0, 3, 4) for
    each LDS-column kernel; the L = 16 384 ones use no scratch and spill no
    VGPR, as their plain peak-carrying counterparts."""
    lcfir.load()  # the library's own make writes the remarks next to it
    assert os.path.exists(REMARKS), "liblcfir.so without its remarks: rebuild with make -C audio-fir-filter_amd"
    k = check_resources.parse(open(REMARKS).read())
    l16 = {n: f for n, f in k.items() if "fir_fft_items_peak_kernel" in n}
    park = {n: f for n, f in k.items() if "fir_fft32_items_peak_kernel" in n}
    for got in (l16, park):
        assert len(got) == 3, sorted(got)
        assert all(sum(f"kernelILi{m}EEEv" in n for n in got) == 1 for m in (0, 3, 4)), sorted(got)
    for n, f in l16.items():
        assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0, (n, f)
    for kernel, flags in (("fir_fft_f64_kernel", "Lb0ELb0E"), ("fir_fft32_f64_kernel", "Lb0E")):
        for m in (0, 3, 4):  # the plain counterparts
            plain = [f for n, f in k.items() if kernel in n and f"ILi{m}E{flags}EEv" in n]
            assert len(plain) == 1, (kernel, m)
            if kernel == "fir_fft_f64_kernel":
                assert plain[0]["ScratchSize"] == 0 and plain[0]["VGPRs Spill"] == 0, (m, plain[0])
