"""numpy restatement of the TPDF dither and the dithered PCM encode
(include/lcfir.h, LCFIR_DITHER_TPDF): test infrastructure, numpy only.

The noise is a pure function of (seed, channel, absolute frame index):

    s = seed ^ ((ch + 1) * 0xD1B54A32D192ED03)            all modulo 2^64
    z = s + frame * 0x9E3779B97F4A7C15
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z =  z ^ (z >> 31)
    d = (f64(z >> 32) - f64(z & 0xFFFFFFFF)) * 2^-32      in (-1, 1) LSB

and a b-bit integer sample of a float v is clamp(rint(f64(v) * 2^(b-1) + d)),
NaN -> 0; float formats pass their bits through.  Every step is exact in f64
but the one add, so the bytes are pinned without a tolerance."""
import numpy as np

NB = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}
FORMATS = ["s16le", "s24le", "s32le", "f32le", "s16be", "s24be", "s32be", "f32be"]
INT_FORMATS = [f for f in FORMATS if not f.startswith("f32")]

_M64 = (1 << 64) - 1
_K_CH = np.uint64(0xD1B54A32D192ED03)
_K_FR = np.uint64(0x9E3779B97F4A7C15)
_K_1 = np.uint64(0xBF58476D1CE4E5B9)
_K_2 = np.uint64(0x94D049BB133111EB)


def _u64(a):
    """Integers of any sign or size (scalars or arrays) as uint64, modulo 2^64."""
    if isinstance(a, np.ndarray) and a.dtype == np.uint64:
        return a
    if isinstance(a, np.ndarray) and a.dtype.kind in "iu":
        return a.astype(np.uint64)
    return np.asarray([int(v) & _M64 for v in np.atleast_1d(np.asarray(a, dtype=object)).ravel()],
                      dtype=np.uint64).reshape(np.shape(a))


def hash64(seed, ch, frame):
    """z of (seed, ch, frame); ch and frame broadcast against each other."""
    with np.errstate(over="ignore"):
        s = _u64(seed) ^ ((_u64(ch) + np.uint64(1)) * _K_CH)
        z = s + _u64(frame) * _K_FR
        z = (z ^ (z >> np.uint64(30))) * _K_1
        z = (z ^ (z >> np.uint64(27))) * _K_2
        return z ^ (z >> np.uint64(31))


def tpdf(seed, ch, frame):
    """d of (seed, ch, frame) in LSB, float64."""
    z = hash64(seed, ch, frame)
    hi = (z >> np.uint64(32)).astype(np.float64)
    lo = (z & np.uint64(0xFFFFFFFF)).astype(np.float64)
    return (hi - lo) * 2.0 ** -32


def frames_from(frame0: int, count: int) -> np.ndarray:
    """frame0 + [0, count) as uint64 (frame0 up to 2^63)."""
    return np.uint64(int(frame0)) + np.arange(count, dtype=np.uint64)


def noise(seed: int, nch: int, frames: int, frame0: int = 0) -> np.ndarray:
    """[nch][frames] noise of one file's frames frame0 + [0, frames)."""
    fr = frames_from(frame0, frames)
    return np.stack([tpdf(seed, c, fr) for c in range(nch)]) if nch else np.zeros((0, frames))


def quantise(v: np.ndarray, bits: int, d=None) -> np.ndarray:
    """The integer a float sample encodes to (int64), d in LSB or None."""
    scale = float(1 << (bits - 1))
    t = np.asarray(v, dtype=np.float32).astype(np.float64) * scale
    if d is not None:
        t = t + d
    with np.errstate(invalid="ignore"):
        q = np.rint(t)
        q = np.where(q < -scale, -scale, np.where(q > scale - 1, scale - 1, q))
    return np.where(np.isnan(q), 0.0, q).astype(np.int64)


def encode(v: np.ndarray, fmt: str, d=None) -> bytes:
    """Planar [nch][frames] float32 -> interleaved bytes; d: same shape, LSB, or
    None for the plain encode."""
    nb = NB[fmt[:3]]
    v = np.asarray(v, dtype=np.float32)
    inter = np.ascontiguousarray(v.T).reshape(-1)
    if fmt.startswith("f32"):
        u = inter.view(np.uint32)
    else:
        di = None if d is None else np.ascontiguousarray(np.asarray(d, dtype=np.float64).T).reshape(-1)
        u = quantise(inter, 8 * nb, di).astype(np.uint32)
    b = np.stack([(u >> np.uint32(8 * i)) & np.uint32(0xFF) for i in range(nb)], 1).astype(np.uint8)
    if fmt.endswith("be"):
        b = b[:, ::-1]
    return b.tobytes()


def decode_ints(raw: bytes, fmt: str) -> np.ndarray:
    """Interleaved bytes of an integer format -> the integers (int64), in stream order."""
    nb = NB[fmt[:3]]
    b = np.frombuffer(raw, np.uint8).reshape(-1, nb).astype(np.int64)
    if fmt.endswith("be"):
        b = b[:, ::-1]
    u = sum(b[:, i] << (8 * i) for i in range(nb))
    return (u << (64 - 8 * nb)) >> (64 - 8 * nb)


def rescale(v: np.ndarray, peak: float, force: bool) -> np.ndarray:
    """The normalize rule folded into the encode: (float)((double)v * (1 / (double)peak))
    iff (peak > 1 or force) and peak > 0."""
    pk = np.float32(peak)
    if (pk > 1.0 or force) and pk > 0.0:
        return (np.asarray(v, np.float32).astype(np.float64) * (1.0 / float(pk))).astype(np.float32)
    return np.asarray(v, np.float32)


def encode_file(v: np.ndarray, fmt: str, seed: int, frame0: int = 0, dither: bool = True) -> bytes:
    """A file's frames frame0 + [0, frames) (planar [nch][frames]) as the library encodes them."""
    nch, frames = v.shape
    return encode(v, fmt, noise(seed, nch, frames, frame0) if dither else None)
