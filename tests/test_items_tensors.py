"""CPU tests of the item set's tensor path (lcfir_items_gather_dev,
lcfir_items_scatter_scaled_dev, batch.TensorBatch): the tile -> (channel,
position) decode the two kernels do, restated in numpy over the library's own
layout; TensorBatch's argument checks and call order against a stub backend;
the new symbols in the header, the library and the binding; the two kernels'
resources as built."""
import os
import subprocess

import numpy as np
import pytest

import batch
import check_resources
import lcfir

ROW_TILE = 4096  # csrc/items.hpp, kItemRowTile
LENGTHS = [0, 1, 3, 4095, 4096, 4097, 9000]


def row_tiles(plan, nframes, nch):
    """lcfir_items_create's row tile table over a plan: (first, count, file)."""
    tiles = []
    for f, (n, c) in enumerate(zip(nframes, nch)):
        if plan["file_group"][f] < 0:
            continue
        off, stride = int(plan["file_offset"][f]), int(plan["file_stride"][f])
        for ch in range(c):
            for t0 in range(0, n, ROW_TILE):
                tiles.append((off + ch * stride + t0, min(ROW_TILE, n - t0), f))
    return tiles


@pytest.mark.parametrize("unit", [4096, 16184, 28768])
def test_tile_decode_covers_every_row_exactly_once(unit):
    """rel = first - off_f, c = rel / stride_f, t0 = rel - c stride_f (items.hpp,
    item_span_ptr): over every tile, every float of every [0, n_f) of every
    channel is covered exactly once and nothing else is."""
    nframes = [n for n in LENGTHS for _ in range(3)]
    nch = [1 + k % 3 for k in range(len(nframes))]
    plan = lcfir.ItemSet.plan(unit, nframes, nch)
    cover = [np.zeros((c, n), np.int32) for n, c in zip(nframes, nch)]
    tiles = row_tiles(plan, nframes, nch)
    assert len(tiles) == sum(c * -(-n // ROW_TILE) for n, c in zip(nframes, nch))
    for first, count, f in tiles:
        off, stride = int(plan["file_offset"][f]), int(plan["file_stride"][f])
        assert first % 4 == 0 and 0 < count <= ROW_TILE and stride >= nframes[f]
        rel = first - off
        c = rel // stride
        t0 = rel - c * stride
        assert 0 <= c < nch[f], (f, c)
        assert 0 <= t0 and t0 + count <= nframes[f], (f, c, t0, count)  # nothing outside [0, n_f)
        cover[f][c, t0:t0 + count] += 1
    for f, cv in enumerate(cover):
        assert np.all(cv == 1), f
    # the arena side of the same tiles: rows' [0, n_f) and nothing of the padding
    arena = np.zeros(plan["arena_floats"], np.int32)
    for first, count, f in tiles:
        arena[first:first + count] += 1
    assert arena.max() <= 1 and arena.sum() == sum(n * c for n, c in zip(nframes, nch))


class StubFilter:
    device = 0


class StubBackend(batch.ItemBackend):
    def __init__(self):
        self.calls = []

    def create(self, nframes, nch):
        self.plan = lcfir.ItemSet.plan(4096, nframes, nch)
        self.calls.append(("create", list(nframes), list(nch)))
        return {k: self.plan[k] for k in ("file_offset", "file_stride", "arena_floats", "groups", "launches")}

    def set_fusion(self, mode):
        self.calls.append(("fusion", mode))

    def new_peaks(self, nfiles):
        return np.zeros(max(1, nfiles), np.float32)

    def zero_peaks(self, peaks):
        self.calls.append("zero")

    def filter(self, peaks):
        self.calls.append("filter")

    def gather(self, ptrs, strides):
        self.calls.append(("gather", list(ptrs), list(strides)))

    def scatter(self, peaks, force, ptrs, strides):
        self.calls.append(("scatter", bool(force), list(ptrs), list(strides)))


def test_tensor_batch_rejects_what_the_kernels_cannot_read():
    import torch
    # every tensor here is a host tensor (no device in this test), so the bad
    # one comes first: the checks run tensor by tensor, the device check last
    good = torch.zeros(2, 100)
    cases = {
        "float32": torch.zeros(2, 100, dtype=torch.float64),          # wrong dtype
        r"\[nch, n\] or \[n\]": torch.zeros(2, 3, 100),                # 3-D
        "stride 1": torch.zeros(2, 200)[:, ::2],                       # strided last dimension
        "channel stride": torch.zeros(1, 100).expand(2, 100),          # channels closer than n
        "is on cpu": good,                                             # a host tensor
    }
    for match, bad in cases.items():
        be = StubBackend()
        with pytest.raises(ValueError, match=match) as e:
            batch.TensorBatch(StubFilter(), [bad, good], backend=be)
        assert "tensor 0" in str(e.value), (match, str(e.value))
        assert be.calls == []  # nothing was planned or allocated
    with pytest.raises(ValueError, match="float32"):
        batch.TensorBatch(StubFilter(), [np.zeros((1, 4), np.float32)], backend=StubBackend())
    with pytest.raises(ValueError, match="fusion"):
        batch.TensorBatch(StubFilter(), [], fusion="all", backend=StubBackend())


def test_tensor_batch_of_nothing_plans_nothing_and_steps():
    be = StubBackend()
    tb = batch.TensorBatch(StubFilter(), [], normalize=True, backend=be)
    tb.step()
    assert tb.outputs == [] and tb.layout["arena_floats"] == 0 and tb.steps == 1
    assert be.calls == [("create", [], []), ("fusion", "groups"), ("gather", [], []), "zero", "filter",
                        ("scatter", True, [], [])]


def test_new_symbols_in_header_library_and_binding():
    new = ["lcfir_items_gather_dev", "lcfir_items_scatter_scaled_dev"]
    declared = lcfir.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", lcfir.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in new:
        assert s in declared and s in exported and s in lcfir._SIGNATURES, s
    assert hasattr(lcfir.ItemSet, "gather_dev") and hasattr(lcfir.ItemSet, "scatter_scaled_dev")
    assert lcfir.load().lcfir_abi_version() == 1
    # null arguments are refused before any device is touched
    lib = lcfir.load()
    assert lib.lcfir_items_gather_dev(None, None, None, None) == lcfir.EINVAL
    assert lib.lcfir_items_scatter_scaled_dev(None, None, 0, None, None, None) == lcfir.EINVAL


def test_built_tensor_kernels_resources():
    """As built: no scratch, no VGPR spill, and the occupancy of the other row
    passes (8 waves per SIMD)."""
    pkg = os.path.dirname(lcfir.LIB_PATH)
    remarks = os.path.join(pkg, "liblcfir.remarks")
    if not os.path.exists(remarks):
        subprocess.run(["make", "-C", pkg, "liblcfir.so"], check=True, capture_output=True)
    k = check_resources.parse(open(remarks).read())
    for name in ("items_gather_kernel", "items_scatter_scaled_kernel"):
        found = [f for n, f in k.items() if name in n]
        assert len(found) == 1, (name, sorted(k))
        f = found[0]
        assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0 and f["Occupancy"] >= 8, (name, f)
    peak = next(f for n, f in k.items() if "items_peak_kernel" in n)
    assert peak["Occupancy"] == 8
