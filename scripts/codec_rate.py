#!/usr/bin/env python3
"""Time of the PCM encode pass alone through its entry points, on one device in
one process.  Two families, four arrangements each:

  per-file  (a) scaled        lcfir_encode_pcm_scaled_dev
            (b) dither_none   lcfir_encode_pcm_dither_dev, LCFIR_DITHER_NONE
            (c) dither_tpdf   the same call with LCFIR_DITHER_TPDF: the 64-bit
                              hash and one f64 add per sample on top
            (d) scaled_again  (a) once more, placed last in the alternation
  item set  the same four through ItemSet.encode_pcm_scaled_dev and
            ItemSet.encode_pcm_dither_dev on one ragged set of 64 files.

(a) and (b) are one kernel behind two entry points (four samples a lane, whole
dwords stored where d_out allows; codec.hpp, items.hpp), so this script has two
floors: |(a) - (d)|, the same call twice, and |(a) - (b)|, the same kernel
through two calls.  A distance between builds or modes below either says
nothing.  On a library from before the fold (a) was a kernel of its own, one
sample a lane with byte stores; profiles/codec_rate_parent.json is this script
on that library, and its `fold` verdicts are the rule the fold was held to:
(b)'s median at most (a)'s plus |(a) - (d)| at every workload of a family.

Per-file workloads: BASELINE config 2's shape (2 channels x 28.8 M frames, int24
LE) and config 1's (1 x 48 000, int16 LE) as the lowcut tool calls the pass; six
channels (the general row walk); two channels with rows one float off
alignment (scalar loads); one channel of float32; and config 2's shape with
d_out one byte off a dword (byte stores throughout).  One peak slot per
channel, the peak below 1, no forced normalize.  The item sets take 64 files of
1 or 2 channels, 4 800 to 28.8 M frames, int16 and int24 LE mixed, once with
every payload on a dword and once with every payload at an odd offset.

Each arrangement is warmed, the device pre-rolled, then the arrangements are
timed in alternation (--rounds windows each, HIP events around the window's
calls on the stream that runs them); the figure is the median window.  Before
timing, (b)'s bytes are compared with (a)'s and (c)'s with neither, and the
script fails if (b)'s differ.  Prints a table and one JSON line; not part of
bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-fir-filter_amd"))

# name, channels, frames, format, calls a window, floats d_in is off 16 bytes, bytes d_out is off a dword
WORKLOADS = [("config2_2x28.8M_s24le", 2, 28_800_000, "s24le", 20, 0, 0),
             ("config1_1x48000_s16le", 1, 48_000, "s16le", 400, 0, 0),
             ("6x9.6M_s24le", 6, 9_600_000, "s24le", 20, 0, 0),
             ("2x28.8M_s16le_rows_off_1_float", 2, 28_800_000, "s16le", 20, 1, 0),
             ("1x57.6M_f32le", 1, 57_600_000, "f32le", 20, 0, 0),
             ("2x28.8M_s24le_out_off_1_byte", 2, 28_800_000, "s24le", 20, 0, 1)]
# name, payload offset modulo 4 per file (cycled), calls a window
ITEM_WORKLOADS = [("items_64_files_dword_offsets", (0,), 5),
                  ("items_64_files_odd_offsets", (1, 3), 5)]
ITEM_FILES, ITEM_MIN, ITEM_MAX = 64, 4_800, 28_800_000
ARRANGEMENTS = ("scaled", "dither_none", "dither_tpdf", "scaled_again")


def window(torch, stream, fn, calls):
    """Event ms of `calls` calls of fn between two events on the stream that runs them."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(args, torch, stream, arrangements, outs, calls, samples, moved, head):
    """Warm, compare the bytes, pre-roll, then time the arrangements in alternation."""
    for fn in arrangements.values():
        fn()
    torch.cuda.synchronize()
    out = dict(head, calls_per_window=calls, rounds=args.rounds, bytes_moved=moved,
               none_equals_scaled=bool(torch.equal(outs["scaled"], outs["dither_none"])),
               tpdf_differs=not bool(torch.equal(outs["scaled"], outs["dither_tpdf"])))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.preroll_s:
        for fn in arrangements.values():
            window(torch, stream, fn, max(1, calls // 4))
    ms = {k: [] for k in arrangements}
    for _ in range(args.rounds):
        for k, fn in arrangements.items():
            ms[k].append(window(torch, stream, fn, calls) / calls)
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"call_us_median": round(1e3 * med, 3), "call_us_min": round(1e3 * min(v), 3),
                  "call_us_max": round(1e3 * max(v), 3), "gsamples_per_s": round(samples / med / 1e6, 3),
                  "gbytes_per_s": round(moved / med / 1e6, 1)}
    a, b, c, d = (out[k]["call_us_median"] for k in ARRANGEMENTS)
    floor = abs(a - d)
    out["comparisons"] = {"floor_us": round(floor, 3), "floor_rel": round(floor / min(a, d), 4),
                          "none_minus_scaled_us": round(b - a, 3), "scaled_over_none": round(a / b, 3),
                          "none_within_floor_or_faster": bool(b - a <= floor),
                          "tpdf_minus_none_us": round(c - b, 3), "tpdf_over_none": round(c / b, 3)}
    return out


def measure(args, torch, lcfir, name, nch, frames, fmt, calls, in_off, out_off, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    buf = (torch.rand(in_off + nch * frames, generator=gen, device=dev, dtype=torch.float32) - 0.5) * 0.8
    x = buf.data_ptr() + 4 * in_off
    peak = torch.full((nch,), 0.4, device=dev, dtype=torch.float32)
    nbytes = lcfir.pcm_bytes(fmt) * nch * frames
    outs = {k: torch.zeros(out_off + nbytes, device=dev, dtype=torch.uint8) for k in ARRANGEMENTS[:3]}
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def scaled():
        lcfir.encode_pcm_scaled_dev(x, frames, nch, frames, fmt, peak, nch, False, outs["scaled"].data_ptr() + out_off, s)

    def dither(mode):
        d_out = outs["dither_" + mode].data_ptr() + out_off
        return lambda: lcfir.encode_pcm_dither_dev(x, frames, nch, frames, fmt, peak, nch, False, mode, args.dither_seed,
                                                   0, d_out, s)

    arrangements = {"scaled": scaled, "dither_none": dither("none"), "dither_tpdf": dither("tpdf"),
                    "scaled_again": scaled}
    samples = nch * frames
    head = {"workload": name, "family": "per_file", "nch": nch, "frames": frames, "format": fmt,
            "in_off_floats": in_off, "out_off_bytes": out_off, "tpdf_should_differ": not fmt.startswith("f32")}
    return timed(args, torch, stream, arrangements, outs, calls, samples, 4 * samples + nbytes, head)


def measure_items(args, torch, lcfir, name, aligns, calls, dev):
    import numpy as np
    n = [min(ITEM_MAX, round(ITEM_MIN * (ITEM_MAX / ITEM_MIN) ** (f / (ITEM_FILES - 1)))) for f in range(ITEM_FILES)]
    nch = [1 + f % 2 for f in range(ITEM_FILES)]
    fmts = ["s16le" if (f // 2) % 2 == 0 else "s24le" for f in range(ITEM_FILES)]
    flt = lcfir.Filter(np.array([1.0]), device=0, method="direct")
    items = lcfir.ItemSet(flt, n, nch)
    row = ((np.random.default_rng(args.seed).random(ITEM_MAX, dtype=np.float32) - np.float32(0.5)) * np.float32(0.8))
    offs, pos = [], 0
    for f in range(ITEM_FILES):  # every output row: the first n_f floats of one random row
        _, dy, stride = items.file(f)
        for c in range(nch[f]):
            lcfir._check(lcfir.load().lcfir_memcpy_h2d(dy + 4 * c * stride, row.ctypes.data, 4 * n[f], None))
        pos += (aligns[f % len(aligns)] - pos) % 4 + 4
        offs.append(pos)
        pos += lcfir.pcm_bytes(fmts[f]) * nch[f] * n[f]
    lcfir.sync()
    peak = torch.full((ITEM_FILES,), 0.4, device=dev, dtype=torch.float32)
    outs = {k: torch.zeros(pos + 4, device=dev, dtype=torch.uint8) for k in ARRANGEMENTS[:3]}
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def scaled():
        items.encode_pcm_scaled_dev(peak, False, outs["scaled"], offs, fmts, s)

    def dither(mode):
        return lambda: items.encode_pcm_dither_dev(peak, False, mode, args.dither_seed, outs["dither_" + mode], offs,
                                                   fmts, s)

    arrangements = {"scaled": scaled, "dither_none": dither("none"), "dither_tpdf": dither("tpdf"),
                    "scaled_again": scaled}
    samples = sum(c * k for c, k in zip(nch, n))
    nbytes = sum(lcfir.pcm_bytes(m) * c * k for m, c, k in zip(fmts, nch, n))
    head = {"workload": name, "family": "items", "files": ITEM_FILES, "samples": samples,
            "offsets_mod_4": list(aligns), "tpdf_should_differ": True}
    out = timed(args, torch, stream, arrangements, outs, calls, samples, 4 * samples + nbytes, head)
    items.close()
    flt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per arrangement, alternating")
    ap.add_argument("--preroll-s", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--dither-seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("codec_rate.py needs a GPU: a rate measured anywhere else says nothing")
    import lcfir
    dev = torch.device("cuda", 0)
    results = []
    jobs = [lambda w=w: measure(args, torch, lcfir, *w, dev) for w in WORKLOADS]
    jobs += [lambda w=w: measure_items(args, torch, lcfir, *w, dev) for w in ITEM_WORKLOADS]
    for job in jobs:
        r = job()
        results.append(r)
        print(f"{r['workload']}: {r['bytes_moved'] / 1e6:.1f} MB a call, {r['calls_per_window']} calls a window, "
              f"NONE == scaled: {r['none_equals_scaled']}, TPDF differs: {r['tpdf_differs']}", flush=True)
        for k in ARRANGEMENTS:
            v = r[k]
            print(f"  {k:13s} {v['call_us_median']:10.3f} us/call (min {v['call_us_min']:.3f}, max {v['call_us_max']:.3f})"
                  f"  {v['gsamples_per_s']:8.3f} Gsamples/s  {v['gbytes_per_s']:8.1f} GB/s")
        c = r["comparisons"]
        print(f"  floor (scaled against scaled_again): {c['floor_us']:.3f} us ({100 * c['floor_rel']:.1f} %); "
              f"dither_none - scaled: {c['none_minus_scaled_us']:+.3f} us (scaled / none = x{c['scaled_over_none']:.2f}, "
              f"within the floor or faster: {c['none_within_floor_or_faster']}); "
              f"dither_tpdf / dither_none = x{c['tpdf_over_none']:.2f}", flush=True)
    fold = {fam: all(r["comparisons"]["none_within_floor_or_faster"] for r in results if r["family"] == fam)
            for fam in ("per_file", "items")}
    print("dither_none within the floor of scaled, or faster, at every workload of the family: " +
          ", ".join(f"{k}: {v}" for k, v in fold.items()))
    line = json.dumps({"codec_rate": results, "build_id": lcfir.build_id(), "fold": fold})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["none_equals_scaled"] and r["tpdf_differs"] == r["tpdf_should_differ"] for r in results):
        raise SystemExit("the NONE bytes differ from the scaled call's, or TPDF changed nothing (or a float file)")


if __name__ == "__main__":
    main()
