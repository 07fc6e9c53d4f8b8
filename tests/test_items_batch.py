"""batch.ItemBatch: its bookkeeping against a stub backend (CPU), and on the
device against BatchRunner for the same files, bit for bit."""
import numpy as np
import pytest

import batch
import lcfir

UNIT = 4096


class StubBackend(batch.ItemBackend):
    """The item set's layout from the pure planner, the passes in numpy: the
    'filter' doubles every sample of the arena (padding included, as a
    launch writes its rows' tails), so the bookkeeping is what is tested."""

    def __init__(self):
        self.calls = []

    def create(self, nframes, nch):
        self.n, self.nch = list(nframes), list(nch)
        self.plan = lcfir.ItemSet.plan(UNIT, nframes, nch)
        self.x = None
        self.y = np.full(self.plan["arena_floats"], np.float32(np.nan))
        return {k: self.plan[k] for k in ("file_offset", "file_stride", "arena_floats", "groups", "launches")}

    def load(self, arena):
        assert arena.dtype == np.float32 and arena.shape == (self.plan["arena_floats"],)
        self.x = arena.copy()
        self.calls.append("load")

    def new_peaks(self, nfiles):
        return np.zeros(max(1, nfiles), np.float32)

    def zero_peaks(self, peaks):
        peaks[:] = 0
        self.calls.append("zero")

    def _blocks(self):
        for f, (o, s) in enumerate(zip(self.plan["file_offset"], self.plan["file_stride"])):
            if s:
                yield f, self.y[o:o + self.nch[f] * s].reshape(self.nch[f], s)[:, :self.n[f]]

    def filter(self, peaks):
        self.y[:] = 2 * self.x + np.float32(1e-3) * (self.x == 0)  # tails are not zero
        for f, blk in self._blocks():
            peaks[f] = max(peaks[f], np.abs(blk).max())
        self.calls.append("filter")

    def normalize(self, peaks, force):
        for f, blk in self._blocks():
            if (peaks[f] > 1 or force) and peaks[f] > 0:
                blk[:] = (blk.astype(np.float64) * (1.0 / float(peaks[f]))).astype(np.float32)
        self.calls.append(("normalize", bool(force)))

    def rows(self, offset, nch, stride, n):
        return self.y[offset:offset + nch * stride].reshape(nch, stride)[:, :n]


def make_files(seed=1):
    rng = np.random.default_rng(seed)
    shapes = [(2, UNIT + 5), (1, 0), (3, 17), (1, 2 * UNIT), (0, 100), (2, UNIT + 5), (1, UNIT - 1)]
    files = [(rng.uniform(-0.4, 0.4, s)).astype(np.float32) for s in shapes]
    files[3] *= np.float32(2.0)  # doubled by the stub filter: the one peak above 1
    return files


@pytest.mark.parametrize("normalize", [False, True])
def test_item_batch_bookkeeping(normalize):
    files = make_files()
    be = StubBackend()
    ib = batch.ItemBatch(be, files, normalize=normalize)
    assert ib.nframes == [f.shape[1] for f in files] and ib.nch == [f.shape[0] for f in files]
    assert ib.layout["groups"] == 2 and ib.layout["launches"] == 2  # one- and two-unit files
    # the arena as loaded: every row in place, everything else zero
    mask = np.zeros(be.x.size, bool)
    for f, x in enumerate(files):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = ib.offset[f] + c * ib.stride[f]
            assert np.array_equal(be.x[o:o + x.shape[1]], x[c])
            mask[o:o + x.shape[1]] = True
    assert not be.x[~mask].any() and mask.sum() == sum(f.size for f in files)
    ib.step()
    ib.step()
    assert ib.steps == 2
    assert be.calls == ["load"] + ["zero", "filter", ("normalize", normalize)] * 2
    res = ib.results()
    assert [r is None for r in res] == [f.size == 0 for f in files]
    for f, x in enumerate(files):
        if x.size == 0:
            assert ib.peaks[f] == 0
            continue
        y = 2 * x
        pk = np.abs(y).max()
        assert ib.peaks[f] == pk  # the tails (1e-3 in the stub) never enter a file's peak
        if (pk > 1 or normalize) and pk > 0:
            y = (y.astype(np.float64) * (1.0 / float(pk))).astype(np.float32)
        assert res[f].shape == x.shape and np.array_equal(res[f], y), f
    assert [f for f in range(len(files)) if ib.peaks[f] > 1] == [3]


def test_item_batch_accepts_torch_tensors_and_rejects_other_shapes():
    import torch
    files = make_files(2)
    a = batch.ItemBatch(StubBackend(), files)
    b = batch.ItemBatch(StubBackend(), [torch.from_numpy(f) for f in files])
    assert np.array_equal(a.b.x, b.b.x)
    with pytest.raises(ValueError, match="file 1"):
        batch.ItemBatch(StubBackend(), [files[0], files[0][0]])
    with pytest.raises(ValueError, match="float32"):
        batch.ItemBatch(StubBackend(), [files[0].astype(np.float64)])
    empty = batch.ItemBatch(StubBackend(), [])
    empty.step()
    assert empty.results() == [] and empty.layout["arena_floats"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("method,ntaps", [("direct", 801), ("fft", 4001)])
@pytest.mark.parametrize("normalize", [False, True])
def test_item_batch_equals_batch_runner(oracle_mod, method, ntaps, normalize):
    """Three stereo files of different lengths, one of them loud, no peak
    exchange: ItemBatch's outputs and peaks are BatchRunner's bit for bit."""
    import torch
    import synth
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    taps = oracle_mod.design_lowcut(20.0, 48000.0, ntaps)
    files = [synth.file_buffer(2, n, 48000.0, file=f, bits=24) for f, n in enumerate([20_000, 61_001, 3_777])]
    files[1] = (files[1] * np.float32(3.0)).astype(np.float32)
    flt = lcfir.Filter(taps, method=method)
    be = batch.DeviceBackend(flt, dev)
    r = batch.BatchRunner(be, 0, 1, [f.shape[1] for f in files], 2, (ntaps - 1) // 2, normalize, "file")
    r.prepare(lambda f, lo, hi: files[f][:, lo:hi])
    assert not r.exchange
    r.step()
    want = {sh.file: y.cpu().numpy() for sh, y in r.results()}
    want_pk = r.peaks.cpu().numpy()[:3]
    ibe = batch.DeviceItemBackend(flt, dev)
    ib = batch.ItemBatch(ibe, files, normalize=normalize)
    for _ in range(2):  # steps are repeatable
        ib.step()
        torch.cuda.synchronize()
        got_pk = ib.peaks.cpu().numpy()
        assert np.array_equal(got_pk.view(np.uint32), want_pk.view(np.uint32))
        for f, y in enumerate(ib.results()):
            assert np.array_equal(y.cpu().numpy().view(np.uint32), want[f].view(np.uint32)), f
    assert want_pk[1] > 1.0 and want_pk[0] <= 1.0 and want_pk[2] <= 1.0
    ibe.close()
