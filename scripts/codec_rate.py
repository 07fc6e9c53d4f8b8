#!/usr/bin/env python3
"""Time of the PCM encode pass alone, four ways, on one device in one process:

  (a) scaled        lcfir_encode_pcm_scaled_dev: one thread per sample, byte stores;
  (b) dither_none   lcfir_encode_pcm_dither_dev with LCFIR_DITHER_NONE: the same
                    bytes, four samples a lane stored as whole dwords;
  (c) dither_tpdf   the same call with LCFIR_DITHER_TPDF: (b) plus the 64-bit
                    hash and one f64 add per sample;
  (d) scaled_again  (a) once more, placed last in the alternation: the distance
                    between (a) and (d) is the floor of every comparison of this
                    run and is printed with them.

Workloads: BASELINE config 2's shape (2 channels x 28.8 M frames, int24 LE) and
config 1's (1 x 48 000, int16 LE), as the lowcut tool calls the pass: one peak
slot per channel, the peak below 1, no forced normalize.  Each arrangement is
warmed, the device pre-rolled, then the arrangements are timed in alternation
(--rounds windows each, HIP events around the window's calls on the stream
that runs them); the figure is the median window.  Before timing, (b)'s bytes
are compared with (a)'s and (c)'s with neither.
Prints a table and one JSON line; not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-fir-filter_amd"))

WORKLOADS = [("config2_2x28.8M_s24le", 2, 28_800_000, "s24le", 20),
             ("config1_1x48000_s16le", 1, 48_000, "s16le", 400)]


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


def measure(args, torch, lcfir, name, nch, frames, fmt, calls, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    x = (torch.rand((nch, frames), generator=gen, device=dev, dtype=torch.float32) - 0.5) * 0.8
    peak = torch.full((nch,), 0.4, device=dev, dtype=torch.float32)
    nbytes = lcfir.pcm_bytes(fmt) * nch * frames
    outs = {k: torch.zeros(nbytes, device=dev, dtype=torch.uint8) for k in ("scaled", "dither_none", "dither_tpdf")}
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def scaled():
        lcfir.encode_pcm_scaled_dev(x, frames, nch, frames, fmt, peak, nch, False, outs["scaled"], s)

    def dither(mode):
        return lambda: lcfir.encode_pcm_dither_dev(x, frames, nch, frames, fmt, peak, nch, False, mode, args.dither_seed,
                                                   0, outs["dither_" + mode], s)

    arrangements = {"scaled": scaled, "dither_none": dither("none"), "dither_tpdf": dither("tpdf"),
                    "scaled_again": scaled}
    for fn in arrangements.values():
        fn()
    torch.cuda.synchronize()
    none_equal = bool(torch.equal(outs["scaled"], outs["dither_none"]))
    tpdf_differs = not bool(torch.equal(outs["scaled"], outs["dither_tpdf"]))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.preroll_s:
        for fn in arrangements.values():
            window(torch, stream, fn, max(1, calls // 4))
    ms = {k: [] for k in arrangements}
    for _ in range(args.rounds):
        for k, fn in arrangements.items():
            ms[k].append(window(torch, stream, fn, calls) / calls)
    samples = nch * frames
    moved = 4 * samples + nbytes  # f32 read once, payload written once
    out = {"workload": name, "nch": nch, "frames": frames, "format": fmt, "calls_per_window": calls,
           "rounds": args.rounds, "bytes_moved": moved, "none_equals_scaled": none_equal,
           "tpdf_differs": tpdf_differs}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"call_us_median": round(1e3 * med, 3), "call_us_min": round(1e3 * min(v), 3),
                  "call_us_max": round(1e3 * max(v), 3), "gsamples_per_s": round(samples / med / 1e6, 3),
                  "gbytes_per_s": round(moved / med / 1e6, 1)}
    a, b, c, d = (out[k]["call_us_median"] for k in arrangements)
    floor = abs(a - d)
    out["comparisons"] = {"floor_us": round(floor, 3), "floor_rel": round(floor / min(a, d), 4),
                          "none_minus_scaled_us": round(b - a, 3), "scaled_over_none": round(a / b, 3),
                          "none_within_floor_or_faster": bool(b - a <= floor),
                          "tpdf_minus_none_us": round(c - b, 3), "tpdf_over_none": round(c / b, 3)}
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
    for name, nch, frames, fmt, calls in WORKLOADS:
        r = measure(args, torch, lcfir, name, nch, frames, fmt, calls, dev)
        results.append(r)
        print(f"{name}: {r['bytes_moved'] / 1e6:.1f} MB a call, {calls} calls a window, "
              f"NONE == scaled: {r['none_equals_scaled']}, TPDF differs: {r['tpdf_differs']}")
        for k in ("scaled", "dither_none", "dither_tpdf", "scaled_again"):
            v = r[k]
            print(f"  {k:13s} {v['call_us_median']:10.3f} us/call (min {v['call_us_min']:.3f}, max {v['call_us_max']:.3f})"
                  f"  {v['gsamples_per_s']:8.3f} Gsamples/s  {v['gbytes_per_s']:8.1f} GB/s")
        c = r["comparisons"]
        print(f"  floor (scaled against scaled_again): {c['floor_us']:.3f} us ({100 * c['floor_rel']:.1f} %); "
              f"dither_none - scaled: {c['none_minus_scaled_us']:+.3f} us (scaled / none = x{c['scaled_over_none']:.2f}, "
              f"within the floor or faster: {c['none_within_floor_or_faster']}); "
              f"dither_tpdf / dither_none = x{c['tpdf_over_none']:.2f}")
    line = json.dumps({"codec_rate": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["none_equals_scaled"] and r["tpdf_differs"] for r in results):
        raise SystemExit("the NONE bytes differ from lcfir_encode_pcm_scaled_dev's, or TPDF changed nothing")


if __name__ == "__main__":
    main()
