"""GPU tests of the PCM encode through every entry point of its one kernel per
layout (lcfir_encode_pcm_dev, _scaled_dev and _dither_dev;
lcfir_items_encode_pcm_scaled_dev and _dither_dev; lowcut --dither) against the
numpy restatement in dither_ref.py.  The noise is a pure function of (seed,
channel, frame) and every step but one f64 add is exact, so bytes are compared
with bytes: no tolerance anywhere."""
import numpy as np
import pytest

import dither_ref as dr
import pcm_ref

pytestmark = pytest.mark.gpu

FORMATS = dr.FORMATS
SENTINEL = 0xA5
SEED = 0x5EED5EED5EED5EED


@pytest.fixture(scope="module")
def lc():
    import lcfir
    assert lcfir.device_count() >= 1
    return lcfir


@pytest.fixture(scope="module")
def src():
    """[8][4099 + 6] floats in (-1.1, 1.1), shared and read-only: every grid case
    takes its channels and frames from the front."""
    x = np.random.default_rng(20).uniform(-1.1, 1.1, (8, 4105)).astype(np.float32)
    x.setflags(write=False)
    return x


def run_encode(lc, x, stride, fmt, dither, seed, frame0, out_off=0, peak=None, force=False, in_off=0,
               entry="dither"):
    """x: planar [nch][frames]; the call's input has `stride` floats between
    channels and starts in_off floats into its buffer, d_out starts out_off
    bytes into a sentinel-filled one.  entry: "dither" (lcfir_encode_pcm_dither_dev),
    "scaled" (lcfir_encode_pcm_scaled_dev; no dither, frame0 unused) or "plain"
    (lcfir_encode_pcm_dev; no peak either).  Returns the payload after checking
    that the sentinel around it is intact."""
    nch, frames = x.shape
    nb = dr.NB[fmt[:3]] * nch * frames
    xin = np.full(in_off + nch * stride, np.float32(np.nan), np.float32)
    for c in range(nch):
        xin[in_off + c * stride:in_off + c * stride + frames] = x[c]
    d_x = lc.DeviceBuffer.from_array(xin)
    d_o = lc.DeviceBuffer.from_array(np.full(nb + 24, SENTINEL, np.uint8))
    d_pk = lc.DeviceBuffer.from_array(np.asarray(peak, np.float32)) if peak is not None else None
    d_in, d_out, npeak = d_x.ptr + 4 * in_off, d_o.ptr + out_off, 0 if peak is None else len(peak)
    if entry == "dither":
        lc.encode_pcm_dither_dev(d_in, stride, nch, frames, fmt, d_pk, npeak, force, dither, seed, frame0, d_out)
    elif entry == "scaled":
        assert dither == "none"
        lc._check(lc.load().lcfir_encode_pcm_scaled_dev(d_in, stride, nch, frames, lc.PCM_FORMATS[fmt],
                                                        d_pk.ptr if d_pk else None, npeak, 1 if force else 0,
                                                        d_out, None))
    else:
        assert entry == "plain" and dither == "none" and peak is None and not force
        lc.encode_pcm_dev(d_in, stride, nch, frames, fmt, d_out)
    lc.sync()
    got = d_o.download(nb + 24, np.uint8)
    assert np.all(got[:out_off] == SENTINEL) and np.all(got[out_off + nb:] == SENTINEL)
    return got[out_off:out_off + nb].tobytes()


@pytest.mark.parametrize("dither", ["tpdf", "none"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_grid(lc, src, fmt, dither):
    """Every format x channel count x length x d_out alignment, with an odd and
    an even input stride above the length (the even one lets one- and
    two-channel rows load as float4 / float2).  Without dither the two older
    entry points give the same bytes, each pinned on the helper's directly."""
    for nch in (1, 2, 3, 8):
        for frames in (1, 3, 4, 5, 257, 4099):
            x = src[:nch, :frames]
            want = dr.encode(x, fmt, dr.noise(SEED, nch, frames) if dither == "tpdf" else None)
            for stride in (frames + 3, (frames + 5) & ~1):
                for off in range(4):
                    if stride != frames + 3 and off not in (0, 3):
                        continue
                    for entry in ("dither", "scaled", "plain") if dither == "none" else ("dither",):
                        got = run_encode(lc, x, stride, fmt, dither, SEED, 0, out_off=off, entry=entry)
                        assert got == want, (nch, frames, stride, off, entry)


@pytest.mark.parametrize("nch", [1, 2])
def test_unaligned_input_rows(lc, src, nch):
    """Rows that start one float off a 16-byte boundary take the scalar loads."""
    x = src[:nch, :4099]
    want = dr.encode(x, "s24le", dr.noise(SEED, nch, 4099))
    assert run_encode(lc, x, 4100, "s24le", "tpdf", SEED, 0, in_off=1) == want


@pytest.mark.parametrize("frame0", [0, 1, 2 ** 32 - 2, 2 ** 40 + 7])
def test_frame0(lc, src, frame0):
    """The noise follows the absolute frame index; 2^32 - 2 crosses the 32-bit carry inside the call."""
    x = src[:2, :4099]
    for fmt in ("s16le", "s24be"):
        assert run_encode(lc, x, 4102, fmt, "tpdf", 3, frame0) == dr.encode_file(x, fmt, 3, frame0)
    if frame0:
        assert dr.encode_file(x, "s16le", 3, frame0) != dr.encode_file(x, "s16le", 3, 0)


@pytest.mark.parametrize("fmt", ["s16be", "s24le", "s32le"])
def test_split_invariance(lc, src, fmt):
    """A file encoded whole equals the file encoded in two ranges."""
    x = src[:3, :4099]
    whole = run_encode(lc, x, 4105, fmt, "tpdf", SEED, 0)
    a = run_encode(lc, x[:, :1000], 4105, fmt, "tpdf", SEED, 0)
    b = run_encode(lc, x[:, 1000:], 4105, fmt, "tpdf", SEED, 1000, out_off=2)
    assert a + b == whole and whole == dr.encode_file(x, fmt, SEED)


@pytest.mark.parametrize("fmt", FORMATS)
def test_rescale_none_and_tpdf(lc, src, fmt):
    """With the normalize folded in: NONE is lcfir_encode_pcm_scaled_dev byte for
    byte, TPDF is the helper applied after the f64 rescale.  The decision comes
    from the largest of the peak slots; d_peak NULL means none."""
    x = np.ascontiguousarray(src[:3, :4099] * np.float32(2.2))
    for peak in (0.5, 1.0, 2.5):
        for force in (False, True):
            slots = [peak * 0.75, peak]
            ref = run_encode(lc, x, 4099, fmt, "none", SEED, 0, peak=slots, force=force, entry="scaled")
            assert run_encode(lc, x, 4099, fmt, "none", SEED, 0, peak=slots, force=force) == ref
            y = dr.rescale(x, peak, force)
            assert ref == dr.encode(y, fmt)
            assert run_encode(lc, x, 4099, fmt, "tpdf", SEED, 0, peak=slots, force=force) == \
                dr.encode_file(y, fmt, SEED)
    assert run_encode(lc, x, 4099, fmt, "none", SEED, 7) == \
        run_encode(lc, x, 4099, fmt, "none", SEED, 0, force=True, entry="scaled")
    assert run_encode(lc, x, 4099, fmt, "tpdf", SEED, 0, force=True) == dr.encode_file(x, fmt, SEED)


@pytest.mark.parametrize("fmt", FORMATS)
def test_value_domain(lc, fmt):
    bits = 8 * dr.NB[fmt[:3]]
    top = np.float32(1.0) - np.float32(2.0 ** -min(bits - 1, 24))  # full scale minus one LSB (f32's nearest for 32 bits)
    pat = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, -0.0, 0.0, 1e-40, -1e-40, top, -top,
                    np.float32(2.0 ** -126), 0.5 / 2 ** (bits - 1), 3.0e38], np.float32)
    x = np.resize(pat, (2, 4099)).astype(np.float32)
    x[1] = np.roll(x[1], 5)
    got = run_encode(lc, x, 4100, fmt, "tpdf", 1, 0)
    assert got == dr.encode_file(x, fmt, 1)
    if fmt.startswith("f32"):  # the input's bits, NaN payloads and -0.0 included
        want = np.ascontiguousarray(x.T).reshape(-1)
        assert got == (want.byteswap() if fmt.endswith("be") else want).tobytes()
        return
    q = dr.decode_ints(got, fmt).reshape(-1, 2).T.astype(np.float64)  # exact: |q| <= 2^31
    hi, lo = 2.0 ** (bits - 1) - 1, -2.0 ** (bits - 1)
    d = dr.noise(1, 2, 4099)
    assert np.all(q[np.isnan(x)] == 0)
    assert np.all(q[(x == np.inf) | (x == 1.0) | (x > 1e38)] == hi) and np.all(q[x == -np.inf] == lo)
    # -1.0 is the lowest code itself: negative noise clamps to it, noise above half an LSB lifts it by one
    m = x == -1.0
    assert np.all((q[m] == lo) | ((q[m] == lo + 1) & (d[m] > 0.5))) and np.all(q[m & (d < 0.5)] == lo)
    assert np.all(np.abs(q[np.abs(x) < 1e-30]) <= 1)  # zeros and subnormals: the noise alone
    if bits <= 24:  # one LSB below full scale and noise above half an LSB: clamped, never wrapped
        m = (x == top) & (d > 0.5)
        assert m.sum() > 50 and np.all(q[m] == hi)
    assert np.all(q[x == top] > 0) and np.all(q[x == -top] < 0)


def test_grid_stride(lc):
    """More quads than the launch has threads: the grid-stride loop's second round."""
    nch, frames = 2, (1 << 21) + 3
    x = np.random.default_rng(21).uniform(-1.0, 1.0, (nch, frames)).astype(np.float32)
    assert run_encode(lc, x, frames + 1, "s24le", "tpdf", SEED, 0) == dr.encode_file(x, "s24le", SEED)


ITEM_FILES = [(1, 0), (1, 1), (2, 1024), (3, 1367), (2, 4099)]  # (3, 1367): a PCM tile ends inside a frame
ITEM_FMTS = ["s16le", "s24be", "s24le", "s16be", "s32le"]
# payload offsets modulo 8: odd ones and a 2 keep the byte stores; the 0s and 4s put, in turn, the
# two-channel file (float2 loads), the file with the split frame and the three-tile file on the dword path
ITEM_ALIGNS = [[1, 3, 0, 4, 2], [3, 1, 5, 7, 4]]


@pytest.mark.parametrize("dither", ["tpdf", "none"])
@pytest.mark.parametrize("aligns", ITEM_ALIGNS)
@pytest.mark.parametrize("force,with_peak", [(False, True), (True, True), (False, False)])
def test_items(lc, src, dither, aligns, force, with_peak):
    """Every file's bytes equal the per-file call's, whatever the batch; the
    bytes between the payloads stay as they were.  With a peak and no dither
    lcfir_items_encode_pcm_scaled_dev is held to the same helper bytes."""
    flt = lc.Filter(np.array([1.0]), device=0, method="direct")
    items = lc.ItemSet(flt, [n for _, n in ITEM_FILES], [c for c, _ in ITEM_FILES])
    files, offs, pos = [], [], 7
    for f, (nch, n) in enumerate(ITEM_FILES):
        x = np.ascontiguousarray(src[f:f + nch, :n] * np.float32(1.0 + 0.5 * f))
        files.append(x)
        _, dy, stride = items.file(f)
        for c in range(nch if n else 0):
            lc._check(lc.load().lcfir_memcpy_h2d(dy + 4 * c * stride, x[c].ctypes.data, x[c].nbytes, None))
        pos += (aligns[f] - pos) % 8 + 8
        offs.append(pos)
        pos += dr.NB[ITEM_FMTS[f][:3]] * nch * n + 5
    lc.sync()
    peaks = np.array([max(float(np.abs(x).max()) if x.size else 0.0, 0.0) for x in files], np.float32)
    d_pk = lc.DeviceBuffer.from_array(peaks) if with_peak else None
    d_blob = lc.DeviceBuffer.from_array(np.full(pos, SENTINEL, np.uint8))
    items.encode_pcm_dither_dev(d_pk, force, dither, SEED, d_blob, offs, ITEM_FMTS)
    lc.sync()
    got = d_blob.download(pos, np.uint8)
    untouched = np.ones(pos, bool)
    for f, x in enumerate(files):
        nch, n = x.shape
        nb = dr.NB[ITEM_FMTS[f][:3]] * nch * n
        untouched[offs[f]:offs[f] + nb] = False
        if nb == 0:
            continue
        pk = [peaks[f]] if with_peak else None
        want = run_encode(lc, x, n, ITEM_FMTS[f], dither, SEED, 0, peak=pk, force=force)
        assert got[offs[f]:offs[f] + nb].tobytes() == want, f
        y = dr.rescale(x, peaks[f], force) if with_peak else x
        assert want == dr.encode_file(y, ITEM_FMTS[f], SEED, dither=dither == "tpdf"), f
    assert np.all(got[untouched] == SENTINEL)
    if with_peak and dither == "none":
        d_sc = lc.DeviceBuffer.from_array(np.full(pos, SENTINEL, np.uint8))
        items.encode_pcm_scaled_dev(d_pk, force, d_sc, offs, ITEM_FMTS)
        lc.sync()
        got = d_sc.download(pos, np.uint8)
        for f, x in enumerate(files):
            if x.size:
                want = dr.encode_file(dr.rescale(x, peaks[f], force), ITEM_FMTS[f], SEED, dither=False)
                assert got[offs[f]:offs[f] + len(want)].tobytes() == want, f
        assert np.all(got[untouched] == SENTINEL)
    if with_peak and dither == "tpdf" and not force:
        sc = lc.DeviceBuffer.from_array(np.full(pos, SENTINEL, np.uint8))
        items.encode_pcm_dither_dev(d_pk, force, "none", SEED, sc, offs, ITEM_FMTS)
        ref = lc.DeviceBuffer.from_array(np.full(pos, SENTINEL, np.uint8))
        items.encode_pcm_scaled_dev(d_pk, force, ref, offs, ITEM_FMTS)
        lc.sync()
        assert np.array_equal(sc.download(pos, np.uint8), ref.download(pos, np.uint8))
    items.close()
    flt.close()


@pytest.mark.parametrize("container,fmt", [("wav", "s16le"), ("aif", "s24be")])
def test_tool(lc, oracle_mod, tmp_path, container, fmt):
    """lowcut --dither / --dither-seed: -f 100 -s 4000 at 48 kHz is 49 taps, which
    AUTO gives to the direct kernel, bit-exact with the oracle's fma mode; so
    the payload is the helper's encode of the oracle's output, every other byte
    of the file is kept, and without the option nothing changes."""
    from test_gpu_lowcut_cli import info, lowcut, tone
    nch, n, rate = 2, 6000, 48000
    x = tone(nch, n, rate, amp=0.45, bits=16 if fmt == "s16le" else 24)
    p = tmp_path / f"in.{container}"
    if container == "wav":
        pcm_ref.write_wave(p, x, rate, fmt, extra_chunks=[(b"LIST", b"INFOICMT\x04\x00\x00\x00dith")])
    else:
        pcm_ref.write_aiff(p, x, rate, fmt, extra_chunks=[(b"ANNO", b"lcfir!")])
    raw = open(p, "rb").read()
    meta = info(p)
    off, nbytes = int(meta["data_offset"]), int(meta["data_bytes"])
    xq = pcm_ref.np_decode(raw[off:off + nbytes], fmt, nch)
    taps = lc.design_lowcut(100.0, 4000.0, float(rate))
    assert taps.size == 49
    y = np.stack([np.asarray(oracle_mod.filter_channel(xq[c], taps, oracle_mod.MODE_FMA), np.float32)
                  for c in range(nch)])
    peak = np.abs(y).max()
    assert 0 < peak <= 1.0
    cases = [([], y, None), (["--dither"], y, 0), (["--dither-seed", 7], y, 7), (["--dither-seed=7"], y, 7),
             (["-n", "--dither"], dr.rescale(y, peak, True), 0), (["-n"], dr.rescale(y, peak, True), None)]
    outs = {}
    for i, (args, yy, seed) in enumerate(cases):
        q = tmp_path / f"out{i}.{container}"
        text = lowcut("-v", *args, "-f", 100, "-s", 4000, p, q)
        assert "49 taps (direct)" in text
        b = open(q, "rb").read()
        assert len(b) == len(raw) and b[:off] == raw[:off] and b[off + nbytes:] == raw[off + nbytes:]
        want = dr.encode(yy, fmt) if seed is None else dr.encode_file(yy, fmt, seed)
        assert b[off:off + nbytes] == want, args
        outs[i] = b
    assert outs[2] == outs[3] and outs[1] != outs[0] and outs[1] != outs[2]


def test_tool_float_file_unchanged_by_dither(lc, tmp_path):
    """--dither on a float file is accepted and changes nothing; a bad seed is a usage error."""
    import subprocess
    from test_gpu_lowcut_cli import LOWCUT, lowcut, tone
    p = tmp_path / "f.wav"
    pcm_ref.write_wave(p, tone(1, 3000, 48000), 48000, "f32le")
    lowcut("-f", 100, "-s", 4000, p, tmp_path / "a.wav")
    lowcut("--dither-seed", 2 ** 64 - 1, "-f", 100, "-s", 4000, p, tmp_path / "b.wav")
    assert open(tmp_path / "a.wav", "rb").read() == open(tmp_path / "b.wav", "rb").read()
    r = subprocess.run([LOWCUT, "--dither-seed", "-3", str(p), str(tmp_path / "c.wav")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and not (tmp_path / "c.wav").exists()
