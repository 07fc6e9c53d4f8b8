"""GPU tap domain: every kernel form on known-answer taps and on tap families
no designed low-cut belongs to, checked at every output.

lcfir_ctx_create takes any finite doubles, and fft_plan_tables /
r32_plan_tables (fir_fft.hpp) turn them into the pair tables every FFT kernel
multiplies by.  The rest of the suite feeds the kernels designed low-cuts and
standard_normal / sqrt(T), and beyond the small goldens compares sampled
positions.  Here (include/lcfir.h, "the taps' value domain"):

  1. delays (h = e_k) on the general and partitioned forms, k at both ends of
     the filter, around its centre and at the first and last tap of every
     partition: y[n] = x[n + k - half] bit for bit (known_answer.py);
  2. pairs (h[half -+ d] = 0.5) on the zero-phase forms, then the general
     table on the same, truly symmetric taps;
  3. the direct kernel (16 taps per block, stages of 256 taps) at tap counts
     on every side of a block and a stage, delays at those boundaries; zeros
     exact, and bit for bit against the oracle's fma chain;
  4. dense parity with the long-double oracle (RMS <= 1e-9, <= 1 f32 ulp with
     the 1e-12 floor, peak == max |y|) for designed, random, antisymmetric
     (type III) and one-sided taps;
  5. taps either side of fft_sym_eligible's 2^-50 threshold;
  6. scale invariance in the taps: y(2^s h) = 2^s y(h) bit for bit, same plan;
  7. all-zero taps: zeros, peak 0.

Forms are test_gpu_persistent_rounds.FORMS (plus the direct kernel); every
case asserts the plan it runs (kernel, segment length, partitions, zero-phase
form).  Shapes: two channels of different data, n = max(2 B + B // 3 + 1, T + B
// 2) with B the plan's outputs per segment -- two whole segments and a partial
one, and long enough that the largest shift (half) leaves outputs to compare;
at most ~108 000 samples (100 001 taps).  The direct kernel: n = 2 x 4096 + 777.
Samples sit on the 16-bit grid (known_answer.grid16).
"""
import time

import numpy as np
import pytest

import known_answer as ka
from test_gpu_parity import RMS_TOL, gpu_filter_channels, max_ulps, rms
from test_gpu_persistent_rounds import FORMS, _taps

pytestmark = pytest.mark.gpu

FS = 48000.0
N_DIRECT = 2 * 4096 + 777
GENERAL = ["l16_general", "l32_park_general", "l16_parts", "l32_park_parts"]
ZERO_PHASE = [("l16_sym", 4001), ("l16_sym", 4003), ("l32_park_sym", 8001), ("l32_reg", 4001), ("l32_reg", 4003),
              ("l32_reg", 19201)]
FAMILIES = ["designed", "normal", "antisym", "one_sided"]
# the zero-phase forms take symmetric taps: the designed low-cut alone
DENSE = [(form, family) for form in FORMS for family in FAMILIES
         if family == "designed" or not FORMS[form]["zero_phase"]]
DIRECT_TAPS = [1, 3, 15, 17, 31, 33, 255, 257, 271, 273, 513, 801]


@pytest.fixture(scope="module")
def lc():
    import lcfir
    assert lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


def _plan_filter(lc, taps, form, zero_phase=None):
    """A Filter of `taps` tuned as FORMS[form], the plan it claims asserted.
    zero_phase: None = what the form says (the general forms always pass
    zero_phase off: a delay at k = half is symmetric); False = the general
    table at the form's segment length (the register kernel's forms then run
    the park-slab kernel); True = the zero-phase form, by the taps' symmetry."""
    f = FORMS[form]
    tune = dict(f["tune"])
    kernel, zp = f["kernel"], f["zero_phase"] if zero_phase is None else zero_phase
    if taps.size != f["ntaps"] or zero_phase is False:
        tune["seg_len"] = f["seg_len"]
    if not zp:
        tune["zero_phase"] = False
        if kernel == "l32_reg":
            kernel = "l32_park"
    flt = lc.Filter(taps, method="fft")
    flt.set_fft_tuning(**tune)
    if f.get("family"):
        flt.set_fft_family(f["family"])
    info, units = flt.fft_info, flt.fft_units
    assert units["kernel"] == kernel, (form, units)
    assert info["seg_len"] == f["seg_len"] and info["zero_phase"] == zp and info["parts"] == f["parts"], (form, info)
    tp = ka.partition_taps(taps.size, info["parts"])
    assert units["outputs"] == f["seg_len"] - tp + 1, (form, units, tp)
    return flt, units["outputs"], tp


def _length(T, B):
    return max(2 * B + B // 3 + 1, T + B // 2)


_X = {}


def _input(n, nch=2):
    """The same two channels for every case of a length (seeded by it)."""
    if n not in _X:
        _X[n] = ka.grid16(np.random.default_rng(n), nch, n)
        assert not np.array_equal(_X[n][0], _X[n][1])
    return _X[n]


def _run(lc, flt, x):
    y, pk = gpu_filter_channels(lc, flt, x)
    assert np.array_equal(pk, np.abs(y).max(axis=1)), (pk, np.abs(y).max(axis=1))
    return y, pk


def _known(failures, y, want, exact_zero, where):
    """assert_known, collected: one case's wrong lane or slot should not hide the next case's."""
    assert np.count_nonzero(want) >= want.size // 4, where  # the shift leaves outputs to check
    try:
        ka.assert_known(y, want, exact_zero, where)
    except AssertionError as e:
        failures.append(str(e))


def _geometry(B, tp, parts, half):
    return f"[segment = index // {B}, {parts} partition(s) of {tp} taps, half {half}]"


# ---- 1: delays on the general forms ---------------------------------------------
@pytest.mark.parametrize("form", GENERAL)
def test_delays_general_forms(lc, form):
    T, parts = FORMS[form]["ntaps"], FORMS[form]["parts"]
    half = (T - 1) // 2
    tp = ka.partition_taps(T, parts)
    ks = ka.delay_ks(T, ka.partition_edges(T, tp, parts))
    assert {0, half, T - 1} <= set(ks)
    assert all(p * tp - 1 in ks and p * tp in ks for p in range(1, parts)) and (parts - 1) * tp < T
    failures, x = [], None
    for k in ks:
        flt, B, tp_plan = _plan_filter(lc, ka.delay_taps(T, k), form)
        assert tp_plan == tp
        x = _input(_length(T, B))
        assert x.shape[1] >= 2 * B + 2 and x.shape[1] % B  # two seams and a partial tail
        y, _ = _run(lc, flt, x)
        _known(failures, y, ka.expect_delay(x, T, k), False, f"{form} delay k={k} (partition {k // tp}, tap {k % tp})")
        flt.close()
    assert not failures, _geometry(B, tp, parts, half) + "\n" + "\n".join(failures)


# ---- 2: pairs on the zero-phase forms, then the general table on the same taps ----
@pytest.mark.parametrize("form,T", ZERO_PHASE)
def test_pairs_zero_phase_forms(lc, form, T):
    half = (T - 1) // 2
    ds = ka.pair_ds(T)
    assert {0, 1, half} <= set(ds) and (2047 in ds) == (half >= 2047) and FORMS[form]["parts"] == 1
    failures = []
    for zero_phase in (True, False):
        for d in ds:
            flt, B, _ = _plan_filter(lc, ka.pair_taps(T, d), form, zero_phase=zero_phase)
            x = _input(_length(T, B))
            y, _ = _run(lc, flt, x)
            _known(failures, y, ka.expect_pair(x, T, d), False,
                   f"{form} T={T} pair d={d} {'zero-phase' if zero_phase else 'general table'}")
            flt.close()
    assert not failures, _geometry(B, T, 1, half) + "\n" + "\n".join(failures)


# ---- 3: the direct kernel -----------------------------------------------------------
@pytest.mark.parametrize("T", DIRECT_TAPS)
def test_delays_direct_kernel(lc, oracle_mod, T):
    x = _input(N_DIRECT)
    ks = ka.direct_ks(T)
    assert {0, T - 1} <= set(ks)
    failures = []
    for k in ks:
        taps = ka.delay_taps(T, k)
        flt = lc.Filter(taps, method="direct")
        assert flt.method == "direct"
        y, _ = _run(lc, flt, x)
        want = ka.expect_delay(x, T, k)
        assert np.count_nonzero(want) > want.size // 2
        try:
            ka.assert_known(y, want, True, f"direct T={T} delay k={k} (block {k // 16}, stage {k // 256})")
        except AssertionError as e:
            failures.append(str(e))
        for c in range(2):
            ref = oracle_mod.filter_channel(x[c], taps, oracle_mod.MODE_FMA)
            if not np.array_equal(y[c].view(np.int32), ref.view(np.int32)):
                failures.append(f"direct T={T} k={k} channel {c}: differs from the fma chain at "
                                f"{np.nonzero(y[c].view(np.int32) != ref.view(np.int32))[0][:8].tolist()}")
        flt.close()
    assert not failures, "\n".join(failures)


# ---- 4: dense oracle parity per tap family ------------------------------------------
def _family_taps(oracle_mod, form, family, T):
    if family == "designed":
        return _taps(oracle_mod, form)  # the general park form's carries its 1e-9 ramp
    if family == "normal":
        return np.random.default_rng(T).standard_normal(T) / np.sqrt(T)
    return {"antisym": ka.antisym_taps, "one_sided": ka.one_sided_taps}[family](T)


def _dense(oracle_mod, taps, x, y, where):
    """Every output of every channel against the threaded long-double oracle."""
    t0 = time.perf_counter()
    for c in range(x.shape[0]):
        ref = oracle_mod.filter_channel_mt(x[c], taps, 16, oracle_mod.MODE_LD)
        r, u = rms(y[c], ref), max_ulps(y[c], ref)
        print(f"{where} channel {c}: n={x.shape[1]} rms={r:.3e} max_ulps={u}")
        assert r <= RMS_TOL, (where, c, r)
        assert u <= 1, (where, c, u)
    print(f"{where}: oracle {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("form,family", DENSE)
def test_dense_oracle_parity(lc, oracle_mod, form, family):
    T = FORMS[form]["ntaps"]
    taps = _family_taps(oracle_mod, form, family, T)
    if family == "antisym":  # nothing symmetric about it: the general table without being told
        auto = lc.Filter(taps, method="fft")
        assert auto.fft_info["zero_phase"] is False
        auto.close()
    flt, B, _ = _plan_filter(lc, taps, form)
    x = _input(_length(T, B))
    y, _ = _run(lc, flt, x)
    assert np.isfinite(y).all()
    _dense(oracle_mod, taps, x, y, f"{form} {family}")


# ---- 5: the symmetry threshold ------------------------------------------------------
@pytest.mark.parametrize("exp,zero_phase", [(-52, True), (-48, False)])
def test_symmetry_threshold(lc, oracle_mod, exp, zero_phase):
    """An antisymmetric part of 2^-52 |h|_1 runs the zero-phase form (default
    tuning: the register kernel), 2^-48 the general table; both against the
    oracle run on the given taps, not the symmetrised ones."""
    sym = oracle_mod.design_lowcut(20.0, FS, 4001)
    sym = 0.5 * (sym + sym[::-1])
    taps = ka.threshold_taps(sym, 2.0 ** exp)
    anti, norm = ka.sym_ratio(taps)
    assert (anti <= norm * np.longdouble(2.0) ** -50) == zero_phase
    flt = lc.Filter(taps, method="fft")
    info, units = flt.fft_info, flt.fft_units
    assert info["zero_phase"] == zero_phase and info["parts"] == 1, info
    assert units["kernel"] == ("l32_reg" if zero_phase else "l16"), units
    x = _input(_length(4001, units["outputs"]))
    y, _ = _run(lc, flt, x)
    _dense(oracle_mod, taps, x, y, f"threshold 2^{exp}")


# ---- 6: scale invariance in the taps -------------------------------------------------
_TINY = np.finfo(np.float32).tiny


@pytest.mark.parametrize("form", list(FORMS) + ["direct"])
def test_tap_scaling(lc, oracle_mod, form):
    """y(2^s h) = ldexp(y(h), s) bit for bit, peaks too, under the same plan:
    every operation on the taps is linear and fft_sym_eligible's rule is
    relative, so a difference means an absolute threshold crept in."""
    def make(h):
        if form == "direct":
            return lc.Filter(h, method="direct"), None
        return _plan_filter(lc, h, form)[:2]

    taps = oracle_mod.design_lowcut(20.0, FS, 801) if form == "direct" else _taps(oracle_mod, form)
    flt, B = make(taps)
    x = _input(N_DIRECT if form == "direct" else _length(taps.size, B))
    y0, pk0 = _run(lc, flt, x)
    assert np.isfinite(y0).all() and np.all(pk0 > 0.1)
    for s in (-40, 40):
        scaled, Bs = make(np.ldexp(taps, s))
        assert Bs == B
        if form != "direct":
            assert scaled.fft_info == flt.fft_info and scaled.fft_units == flt.fft_units
        y, pk = _run(lc, scaled, x)
        want = np.ldexp(y0, s)
        assert want.dtype == np.float32
        normal = (np.abs(y0) >= _TINY) & (np.abs(want) >= _TINY) & np.isfinite(want)
        assert normal.mean() > 0.999, (s, normal.mean())
        bad = normal & (y.view(np.int32) != want.view(np.int32))
        assert not bad.any(), (form, s, int(bad.sum()), np.argwhere(bad)[:8].tolist())
        assert np.array_equal(pk, np.ldexp(pk0, s)), (form, s, pk, pk0)
        scaled.close()


# ---- 7: all-zero taps ---------------------------------------------------------------
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_all_zero_taps(lc, method):
    flt = lc.Filter(np.zeros(4001), method=method)
    if method == "fft":
        info, units = flt.fft_info, flt.fft_units
        assert info["parts"] == 1 and info["zero_phase"] is False and units["kernel"] is not None, (info, units)
        x = _input(_length(4001, units["outputs"]))
    else:
        assert flt.method == "direct"
        x = _input(N_DIRECT)
    y, pk = _run(lc, flt, x)
    assert not np.isnan(y).any()
    assert np.all(y == 0.0) and np.all(pk == 0.0)
