#!/usr/bin/env python3
"""Rate of a batch of short files eight ways, on one device in one process:

  (a) eager    per-file lcfir_filter_window_dev calls on one stream
               (batch.BatchRunner, one lane: fused peak, the normalize riding
               in the next file's launch);
  (b) graphed  the same steps on ten lanes replayed from a HIP graph, as
               `bench.py --config 1` arranges them (batch.GraphedSteps);
  (c) items    one item set (batch.ItemBatch, fusion="auto"): one filter
               launch for all groups over the per-unit table where the plan's
               kernel has an item form (the L = 16 384 and the park kernel; a
               register-kernel plan, as 19 201 linear-phase taps give by
               default, stays on the per-group launches: see "filter_launches"
               in the output, and --family lds), one ragged peak launch, one
               ragged normalize;
  (d) items_groups  a second item set with fusion="groups": one filter launch
               per group of equal unit count, then the same two ragged passes;
  (e) items_parts   a third item set with fusion="parts": (c)'s launch for a
               single-partition plan, and for a partitioned plan on an
               LDS-column kernel (--fs 96000: 38 401 taps, two partitions on
               the park kernel) one launch per partition for all groups, where
               (c) and (d) both run groups x partitions launches;
  (f) tensors       the files as float32 tensors in device memory through
               batch.TensorBatch: one gather launch, (d)'s filter step, one
               scatter launch that rescales on the way out into the caller's
               output tensors;
  (g) tensors_copies  the same tensors in, the same output tensors filled, by
               what the library offered before (f): one copy_ per row into the
               arena, (d)'s step with its in-place normalize, one copy_ per row
               out;
  (h) groups_again  (d) once more, on an item set of its own, placed last in
               the alternation: the spread between (d) and (h) is the floor of
               every comparison of this run and is printed with them.  (f) is
               compared with (g).

A step is filter + per-file peak + the per-file normalize decision for every
file of the batch.  Workloads: BASELINE config 1's shape repeated (--files
mono files of 1 s at 48 kHz, 19 201 taps), then the same number of files with
lengths drawn uniformly from 0.1-3 s (seeded).  Each arrangement is warmed,
the device pre-rolled, then the arrangements are timed in alternation
(--rounds windows each, HIP events around --steps steps on the stream that
runs them, and a host clock that stops after a device synchronise beside
them); the rate is the batch's samples x steps / the window's event time.
Before and after timing, the outputs and peaks of (c) to (h) are compared
with (a)'s bit for bit.
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


def build(torch, lcfir, batch, flt, files, dev, lanes):
    half = (flt.ntaps - 1) // 2
    nframes = [f.shape[1] for f in files]
    be_a = batch.DeviceBackend(flt, dev)
    run_a = batch.BatchRunner(be_a, 0, 1, nframes, 1, half, False, "file")
    run_a.prepare(lambda f, lo, hi: files[f][:, lo:hi])
    be_b = batch.DeviceBackend(flt, dev, lanes=lanes, own_streams=True)
    run_b = batch.BatchRunner(be_b, 0, 1, nframes, 1, half, False, "file", lanes=lanes)
    run_b.prepare(lambda f, lo, hi: files[f][:, lo:hi])
    ibe = batch.DeviceItemBackend(flt, dev)
    ib = batch.ItemBatch(ibe, files, fusion="auto")
    ibe_g = batch.DeviceItemBackend(flt, dev)
    ib_g = batch.ItemBatch(ibe_g, files, fusion="groups")
    ibe_p = batch.DeviceItemBackend(flt, dev)
    ib_p = batch.ItemBatch(ibe_p, files, fusion="parts")
    return be_a, run_a, be_b, run_b, ibe, ib, ibe_g, ib_g, ibe_p, ib_p


def window(torch, stream, fn, calls):
    """(event ms, host ms) of `calls` calls of fn issued with `stream` current,
    between two events on it; the host clock stops after a device synchronise.
    (BatchRunner steps leave another stream current, so every window sets its
    own: events on a stream the work does not run on bracket nothing.)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(calls):
            fn()
    with torch.cuda.stream(stream):
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def measure(args, torch, lcfir, batch, np, name, files, taps, dev):
    flt = lcfir.Filter(taps, device=dev.index or 0, method="auto")
    if args.family != "default":
        flt.set_fft_family(args.family)
    be_a, run_a, be_b, run_b, ibe, ib, ibe_g, ib_g, ibe_p, ib_p = build(torch, lcfir, batch, flt, files, dev, args.lanes)
    samples = sum(f.size for f in files)
    ibe_2 = batch.DeviceItemBackend(flt, dev)
    ib_2 = batch.ItemBatch(ibe_2, files, fusion="groups")
    sets = {"items": ib, "items_groups": ib_g, "items_parts": ib_p, "groups_again": ib_2}
    launched = {k: v.b.items.filter_launches() for k, v in sets.items()}
    # the files as tensors in device memory, and the two ways to filter them
    d_files = [torch.from_numpy(f).to(dev) for f in files]
    tb = batch.TensorBatch(flt, d_files, normalize=False, fusion="groups")
    ibe_c = batch.DeviceItemBackend(flt, dev)
    ib_c = batch.ItemBatch(ibe_c, [np.zeros_like(f) for f in files], fusion="groups")
    rows_in = [ibe_c.x[o:o + c * st].view(c, st)[:, :n] if st else None
               for o, c, st, n in zip(ib_c.offset, ib_c.nch, ib_c.stride, ib_c.nframes)]
    rows_out = ib_c.results()
    outs_c = [torch.empty_like(t) for t in d_files]

    def copies_step():
        for t, v in zip(d_files, rows_in):
            if v is not None:
                for c in range(t.shape[0]):
                    v[c].copy_(t[c])
        ib_c.step()
        for o, v in zip(outs_c, rows_out):
            if v is not None:
                for c in range(o.shape[0]):
                    o[c].copy_(v[c])

    def same_as_eager():
        """every item set against the per-file calls, outputs and peaks"""
        run_a.step()
        for v in sets.values():
            v.step()
        tb.step()
        copies_step()
        torch.cuda.synchronize()
        want = {sh.file: y.cpu().numpy() for sh, y in run_a.results()}
        pk_a = run_a.peaks.cpu().numpy()[:len(files)]
        ok = {}
        for k, v in sets.items():
            pk_c = v.peaks.cpu().numpy()[:len(files)]
            ok[k] = bool(np.array_equal(pk_a.view(np.uint32), pk_c.view(np.uint32)))
            for f, y in enumerate(v.results()):
                ok[k] = ok[k] and bool(np.array_equal(y.cpu().numpy().view(np.uint32), want[f].view(np.uint32)))
        for k, outs, pk in (("tensors", tb.outputs, tb.peaks), ("tensors_copies", outs_c, ib_c.peaks)):
            ok[k] = bool(np.array_equal(pk_a.view(np.uint32), pk.cpu().numpy()[:len(files)].view(np.uint32)))
            for f, y in enumerate(outs):
                ok[k] = ok[k] and bool(np.array_equal(y.cpu().numpy().view(np.uint32), want[f].view(np.uint32)))
        return ok

    # same bytes first
    same = same_as_eager()
    for _ in range(3):
        run_b.step()
    graphed = batch.GraphedSteps(run_b, be_b)
    graphed.replay()
    torch.cuda.synchronize()
    per_replay = graphed.per_replay
    replays = max(1, -(-args.steps // per_replay))
    s_a = be_a.streams[0]  # the eager runner's stream; the item set's steps go to it too
    arrangements = {
        "eager": (s_a, run_a.step, args.steps, args.steps),
        "graphed": (be_b.streams[0], graphed.replay, replays, replays * per_replay),
        "items": (s_a, ib.step, args.steps, args.steps),
        "items_groups": (s_a, ib_g.step, args.steps, args.steps),
        "items_parts": (s_a, ib_p.step, args.steps, args.steps),
        "tensors": (s_a, tb.step, args.steps, args.steps),
        "tensors_copies": (s_a, copies_step, args.steps, args.steps),
        "groups_again": (s_a, ib_2.step, args.steps, args.steps),
    }
    # pre-roll: untimed work until the clock has settled, every arrangement warm
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.preroll_s:
        for stream, fn, _, _ in arrangements.values():
            window(torch, stream, fn, 4)
    ms = {k: [] for k in arrangements}
    host = {k: [] for k in arrangements}
    for _ in range(args.rounds):
        for k, (stream, fn, calls, steps) in arrangements.items():
            ev, wall = window(torch, stream, fn, calls)
            ms[k].append(ev / steps)
            host[k].append(wall / steps)
    # the timed steps computed what the first ones did
    with torch.cuda.stream(s_a):
        again = same_as_eager()
    same = {k: same[k] and again[k] for k in same}
    cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    out = {"workload": name, "files": len(files), "samples_per_step": samples, "ntaps": int(flt.ntaps),
           "fft": flt.fft_info, "unit": flt.fft_units["outputs"], "kernel": flt.fft_units["kernel"], "groups": ib.layout["groups"],
           "launches": ib.layout["launches"], "items_equal_per_file_calls": all(same.values()),
           "equal_per_file_calls": same, "filter_launches": {k: v[0] for k, v in launched.items()},
           "fused_units": launched["items"][1], "cus": cus, "grid_rounds": -(-launched["items"][1] // cus),
           "fused_units_parts": launched["items_parts"][1],
           "rounds": args.rounds,
           "steps_per_window": {k: v[3] for k, v in arrangements.items()}}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"step_ms_median": round(med, 4), "step_ms_min": round(min(v), 4), "step_ms_max": round(max(v), 4),
                  "host_step_ms_median": round(statistics.median(host[k]), 4),
                  "gsamples_per_s": round(samples / med / 1e6, 3)}
    # the floor of this run's comparisons: the same step on two item sets, at
    # two places of the alternation
    g, g2 = out["items_groups"]["step_ms_median"], out["groups_again"]["step_ms_median"]
    floor = abs(g - g2)
    tens, cop = out["tensors"]["step_ms_median"], out["tensors_copies"]["step_ms_median"]
    out["comparisons"] = {"floor_ms": round(floor, 4), "floor_rel": round(floor / min(g, g2), 4),
                          "tensors_copies_minus_tensors_ms": round(cop - tens, 4),
                          "tensors_copies_over_tensors": round(cop / tens, 3),
                          "tensors_beyond_floor": bool(cop - tens > floor)}
    run_a.close()
    run_b.close()
    torch.cuda.synchronize()
    tb.close()
    for be in (ibe, ibe_g, ibe_p, ibe_2, ibe_c):
        be.close()
    flt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--fs", type=float, default=48000.0)
    ap.add_argument("--slope", type=float, default=10.0, help="transition width in Hz (10 Hz at 48 kHz: 19 201 taps)")
    ap.add_argument("--steps", type=int, default=60, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per arrangement, alternating")
    ap.add_argument("--lanes", type=int, default=10)
    ap.add_argument("--preroll-s", type=float, default=1.0)
    ap.add_argument("--family", choices=["default", "lds"], default="default",
                    help="lcfir_ctx_set_fft_family: lds runs the LDS-column kernels, which have the item form")
    ap.add_argument("--seed", type=int, default=20260206)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("items_rate.py needs a GPU: a rate measured anywhere else says nothing")
    import lcfir
    import batch
    dev = torch.device("cuda", 0)
    taps = lcfir.design_lowcut(20.0, args.slope, args.fs)
    rng = np.random.default_rng(args.seed)

    def noise(n):
        return (rng.integers(-2**23, 2**23, size=(1, n)) / 2.0**23 * 0.4).astype(np.float32)

    one_s = int(round(args.fs))
    workloads = [("equal_1s", [one_s] * args.files),
                 ("uniform_0.1_3s", rng.integers(one_s // 10, 3 * one_s + 1, args.files).tolist())]
    results = []
    for name, lengths in workloads:
        files = [noise(int(n)) for n in lengths]
        r = measure(args, torch, lcfir, batch, np, name, files, taps, dev)
        results.append(r)
        print(f"{name}: {r['files']} files, {r['samples_per_step']} samples/step, {r['ntaps']} taps, "
              f"unit {r['unit']} ({r['kernel']}), {r['groups']} groups, filter launches {r['filter_launches']}, "
              f"{r['fused_units']} fused units = {r['grid_rounds']} rounds of {r['cus']} CUs "
              f"({r['fused_units_parts']} under parts), "
              f"same bytes: {r['equal_per_file_calls']}")
        for k in ("eager", "graphed", "items", "items_groups", "items_parts", "tensors", "tensors_copies",
                  "groups_again"):
            v = r[k]
            print(f"  {k:14s} {v['step_ms_median']:9.4f} ms/step (min {v['step_ms_min']:.4f}, max "
                  f"{v['step_ms_max']:.4f}; host clock {v['host_step_ms_median']:.4f})  "
                  f"{v['gsamples_per_s']:8.3f} Gsamples/s")
        c = r["comparisons"]
        print(f"  floor (items_groups against groups_again): {c['floor_ms']:.4f} ms ({100 * c['floor_rel']:.1f} %); "
              f"tensors_copies - tensors: {c['tensors_copies_minus_tensors_ms']:+.4f} ms, "
              f"x{c['tensors_copies_over_tensors']:.2f} (beyond the floor: {c['tensors_beyond_floor']})")
    line = json.dumps({"items_rate": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["items_equal_per_file_calls"] for r in results):
        raise SystemExit("the item set's bytes differ from the per-file calls'")


if __name__ == "__main__":
    main()
