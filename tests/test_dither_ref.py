"""CPU tests of the TPDF dither: the numpy restatement (dither_ref.py) against
the values pinned in include/lcfir.h's definition and against the library's
host function lcfir_dither_tpdf, bit for bit; the noise's statistics and what
it does to the quantiser; the new entry points' argument checks; the two new
kernels' resources as built.  No device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import check_resources
import dither_ref as dr
import lcfir

# seed, ch, frame -> z, d
PINNED = [
    (0, 0, 0, 0x8209B480FAED1B10, -0.4722198583185673),
    (0, 0, 1, 0x2D0F28C7E7E786B2, -0.7298639963846654),
    (0, 1, 0, 0x6C23AACCA1387409, -0.20734842051751912),
    (1, 0, 0, 0x01D60447FEA35413, -0.9875078080222011),
    (0x123456789ABCDEF0, 2, 2 ** 33 + 5, 0x455892673477D3C2, 0.06592933204956353),
    (0xFFFFFFFFFFFFFFFF, 65534, 2 ** 62, 0x729BFD5937B2C4DB, 0.23012116504833102),
]

N = 1 << 20


@pytest.mark.parametrize("seed,ch,frame,z,d", PINNED)
def test_pinned_values(seed, ch, frame, z, d):
    assert int(dr.hash64(seed, ch, frame)) == z
    assert float(dr.tpdf(seed, ch, frame)) == d
    got = lcfir.dither_tpdf(seed, ch, frame, 1)
    assert got.shape == (1,) and got.dtype == np.float64 and got[0] == d


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
@pytest.mark.parametrize("ch", [0, 1, 65534])
@pytest.mark.parametrize("frame0", [0, 2 ** 32 - 2, 2 ** 40 + 7])
def test_helper_equals_library(seed, ch, frame0):
    """Identical as f64 bit patterns; the middle frame0 crosses the 32-bit carry."""
    want = dr.tpdf(seed, ch, dr.frames_from(frame0, 4096))
    got = lcfir.dither_tpdf(seed, ch, frame0, 4096)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.fixture(scope="module")
def d00():
    """Channel 0, seed 0, frames [0, N + 1): shared, read-only."""
    d = dr.tpdf(0, 0, np.arange(N + 1, dtype=np.uint64))
    d.setflags(write=False)
    return d


def _corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)))


def test_noise_statistics(d00):
    """d = (U1 - U2) for two independent uniforms on [0, 1): mean 0, variance
    1/6, fourth moment 1/15.  Each bound is five standard deviations of the
    estimator at N = 2^20 samples:
      mean:         sigma = sqrt(var / N)             = sqrt(1 / 6N)
      variance:     sigma = sqrt((E d^4 - var^2) / N) = sqrt((1/15 - 1/36) / N) = sqrt(7 / 180N)
      correlation of two independent streams: sigma = 1 / sqrt(N)."""
    d = d00[:N]
    assert abs(d.mean()) <= 5 * np.sqrt(1 / (6 * N))                 # 2.0e-3
    assert abs(d.var() - 1 / 6) <= 5 * np.sqrt(7 / (180 * N))        # 9.6e-4
    assert d.min() > -1.0 and d.max() < 1.0
    fr = np.arange(N, dtype=np.uint64)
    bound = 5 / np.sqrt(N)                                           # 4.9e-3
    assert abs(_corr(d, dr.tpdf(0, 1, fr))) <= bound                 # channel 0 against 1
    assert abs(_corr(d, dr.tpdf(1, 0, fr))) <= bound                 # seed 0 against 1
    assert abs(_corr(d, d00[1:])) <= bound                           # lag 1


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("lsb", [0.3, -0.45, 0.5])
def test_quantiser_constant_input(d00, bits, lsb):
    """A constant below one LSB: plain rounding loses it, TPDF dither keeps its
    mean.  With +-1 LSB triangular noise the error e = q - x has mean 0 and
    variance 1/4 whatever x is, so mean(q) is within 5 * 0.5 / sqrt(N) of x;
    |e| < 3/2 gives e^2 <= 9/4, so var(e^2) <= (9/4) * E e^2 = 9/16 and
    mean(e^2) is within 5 * 0.75 / sqrt(N) = 3.7e-3 < 5.5e-3 of 1/4."""
    v = np.full(N, lsb / (1 << (bits - 1)), np.float32)
    x = float(v[0]) * (1 << (bits - 1))  # the input in LSB, as the f32 holds it
    assert not dr.quantise(v, bits).any()
    q = dr.quantise(v, bits, d00[:N]).astype(np.float64)
    assert abs(q.mean() - x) <= 5 * 0.5 / np.sqrt(N)                 # 2.4e-3
    e = q - x
    assert np.abs(e).max() < 1.5
    assert abs(np.mean(e * e) - 0.25) <= 5.5e-3


def test_quantiser_sine_below_one_lsb(d00):
    """997 Hz at 0.4 LSB of int16, 48 kHz, ten seconds (997 whole cycles a
    second): undithered it is digital silence; dithered, the projection onto
    the sine gives the amplitude back (the estimator's sigma is
    0.5 * sqrt(2 / n) = 1.0e-3 LSB)."""
    n = 480_000
    s = np.sin(2 * np.pi * 997.0 * np.arange(n) / 48000.0)
    v = (0.4 / 32768.0 * s).astype(np.float32)
    assert not dr.quantise(v, 16).any()
    q = dr.quantise(v, 16, d00[:n]).astype(np.float64)
    amp = 2.0 * np.dot(q, s) / n
    assert abs(amp - 0.4) <= 0.02
    assert dr.encode(v[None, :], "s16le") == bytes(2 * n)


def test_encode_helper_formats():
    """The helper's byte layout: both endians, the clamp, NaN and the float pass-through."""
    v = np.array([[0.5, -1.0, 1.0, np.nan, -0.0]], np.float32)
    assert dr.encode(v, "s16le") == bytes([0x00, 0x40, 0x00, 0x80, 0xFF, 0x7F, 0, 0, 0, 0])
    assert dr.encode(v, "s24be") == bytes([0x40, 0, 0, 0x80, 0, 0, 0x7F, 0xFF, 0xFF, 0, 0, 0, 0, 0, 0])
    d = np.full(v.shape, 0.75)
    assert dr.encode(v, "s16le", d)[:6] == bytes([0x01, 0x40, 0x01, 0x80, 0xFF, 0x7F])
    assert dr.encode(v, "f32le", d) == v.tobytes() and dr.encode(v, "f32be", d) == v.byteswap().tobytes()


def _einval(rc):
    assert rc == lcfir.EINVAL
    assert lcfir.load().lcfir_last_error()


def test_argument_checks():
    """Refused before any device is touched, each with a message."""
    lib = lcfir.load()
    out = np.zeros(4, np.float64)
    big = 2 ** 63 - 1
    _einval(lib.lcfir_dither_tpdf(0, 0, -1, 4, out.ctypes.data))           # negative frame0
    _einval(lib.lcfir_dither_tpdf(0, 0, 0, -1, out.ctypes.data))           # negative count
    _einval(lib.lcfir_dither_tpdf(0, -1, 0, 4, out.ctypes.data))           # negative channel
    _einval(lib.lcfir_dither_tpdf(0, 0, big - 2, 4, out.ctypes.data))      # frame0 + count overflows
    _einval(lib.lcfir_dither_tpdf(0, 0, 0, 4, None))                       # NULL output, count > 0
    assert lib.lcfir_dither_tpdf(0, 0, 0, 0, None) == lcfir.OK
    assert lcfir.dither_tpdf(5, 3, 9, 0).shape == (0,)
    with pytest.raises(lcfir.LcfirError):
        lcfir.dither_tpdf(0, 0, -1, 4)
    fake = out.ctypes.data  # never dereferenced: every call below fails its checks
    s16 = lcfir.PCM_FORMATS["s16le"]
    enc = lib.lcfir_encode_pcm_dither_dev
    _einval(enc(fake, 4, 1, 4, s16, None, 0, 0, 2, 0, 0, fake, None))      # unknown mode
    _einval(enc(fake, 4, 1, 4, s16, None, 0, 0, -1, 0, 0, fake, None))
    _einval(enc(fake, 4, 1, 4, s16, None, 0, 0, 1, 0, -1, fake, None))     # negative frame0
    _einval(enc(fake, 4, 1, 4, s16, None, 0, 0, 1, 0, big - 2, fake, None))  # frame0 + frames overflows
    _einval(enc(fake, 4, 1, 4, s16, None, 0, 0, 0, 0, -1, fake, None))     # checked with NONE too
    _einval(enc(fake, 4, 1, 4, 99, None, 0, 0, 1, 0, 0, fake, None))       # the existing rules
    _einval(enc(fake, 4, 1, 4, s16, None, 1, 0, 1, 0, 0, fake, None))      # npeak > 0, d_peak NULL
    _einval(enc(fake, 4, 1, 4, s16, None, 0, 0, 1, 0, 0, None, None))      # NULL output
    _einval(enc(fake, 3, 2, 4, s16, None, 0, 0, 1, 0, 0, fake, None))      # stride < frames
    _einval(lib.lcfir_items_encode_pcm_dither_dev(None, None, 0, 1, 0, None, None, None, None))
    with pytest.raises(KeyError):
        lcfir.encode_pcm_dither_dev(fake, 4, 1, 4, "s16le", None, 0, False, "rect", 0, 0, fake)


def test_abi_lists_the_dither_calls():
    new = ["lcfir_dither_tpdf", "lcfir_encode_pcm_dither_dev", "lcfir_items_encode_pcm_dither_dev"]
    declared = lcfir.header_symbols()
    lib = lcfir.load()
    for s in new:
        assert s in declared and s in lcfir._SIGNATURES and hasattr(lib, s), s
    text = open(lcfir.HEADER_PATH).read()
    assert "#define LCFIR_DITHER_NONE 0" in text and "#define LCFIR_DITHER_TPDF 1" in text
    assert lcfir.DITHER_MODES == {"none": 0, "tpdf": 1}
    assert hasattr(lcfir.ItemSet, "encode_pcm_dither_dev")


def test_built_dither_kernels_resources():
    """As built: both forms of both new kernels without scratch or spills."""
    pkg = os.path.dirname(lcfir.LIB_PATH)
    remarks = os.path.join(pkg, "liblcfir.remarks")
    if not os.path.exists(remarks):
        subprocess.run(["make", "-C", pkg, "liblcfir.so"], check=True, capture_output=True)
    k = check_resources.parse(open(remarks).read())
    for name in ("encode_pcm_dither_kernel", "items_encode_dither_kernel"):
        found = [f for n, f in k.items() if name in n]
        assert len(found) == 2, (name, sorted(k))  # NONE and TPDF
        for f in found:
            assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (name, f)
