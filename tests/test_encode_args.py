"""The three per-file encode calls are one function's callers, and the two item
calls another's: every refusal below happens before a device is touched, with
the same code and text whichever entry point is used (CPU)."""
import numpy as np
import pytest

import lcfir

S16 = lcfir.PCM_FORMATS["s16le"]
BIG = 2 ** 63 - 1


def refused(rc):
    assert rc == lcfir.EINVAL
    return lcfir.load().lcfir_last_error().decode()


def per_file_calls():
    """name -> call(d_in, stride, nch, frames, format, d_out) with no peak, no dither."""
    lib = lcfir.load()
    return {
        "plain": lambda i, st, c, n, f, o: lib.lcfir_encode_pcm_dev(i, st, c, n, f, o, None),
        "scaled": lambda i, st, c, n, f, o: lib.lcfir_encode_pcm_scaled_dev(i, st, c, n, f, None, 0, 0, o, None),
        "dither": lambda i, st, c, n, f, o: lib.lcfir_encode_pcm_dither_dev(i, st, c, n, f, None, 0, 0, 0, 0, 0, o,
                                                                             None),
    }


@pytest.mark.parametrize("entry", ["plain", "scaled", "dither"])
def test_per_file_refusals(entry):
    fake = np.zeros(4, np.float64).ctypes.data  # never dereferenced: every call fails its checks or is empty
    enc = per_file_calls()[entry]
    assert refused(enc(fake, 4, 1, 4, 99, fake)) == "unknown PCM format 99"
    assert refused(enc(fake, 4, -1, 4, S16, fake)) == "negative size"
    assert refused(enc(fake, 4, 1, -4, S16, fake)) == "negative size"
    assert enc(None, 4, 0, 4, S16, None) == lcfir.OK and enc(None, 4, 1, 0, S16, None) == lcfir.OK
    assert refused(enc(None, 4, 1, 4, S16, fake)) == "null argument"
    assert refused(enc(fake, 4, 1, 4, S16, None)) == "null argument"
    assert refused(enc(fake, 3, 2, 4, S16, fake)) == "channel stride < frames"
    # frames * nch * 4 bytes of input cannot exist; before the fold the two older calls let the product overflow
    assert refused(enc(fake, BIG, 2, BIG // 4, S16, fake)) == "frames * nch too large"
    assert refused(enc(fake, BIG, 1, BIG // 4 + 1, S16, fake)) == "frames * nch too large"


def test_scaled_peak_refusals():
    lib = lcfir.load()
    fake = np.zeros(4, np.float64).ctypes.data
    assert refused(lib.lcfir_encode_pcm_scaled_dev(fake, 4, 1, 4, S16, fake, -1, 0, fake, None)) == "negative size"
    assert refused(lib.lcfir_encode_pcm_scaled_dev(fake, 4, 1, 4, S16, None, 1, 0, fake, None)) == "null argument"


def test_items_null_set():
    lib = lcfir.load()
    assert refused(lib.lcfir_items_encode_pcm_scaled_dev(None, None, 0, None, None, None, None)) == "items is null"
    assert refused(lib.lcfir_items_encode_pcm_dither_dev(None, None, 0, 0, 0, None, None, None, None)) == \
        "items is null"
