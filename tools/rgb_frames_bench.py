#!/usr/bin/env python3
"""Times batched RGB frames against the frame-by-frame calls, 4K and 8K, 5/3 (wl 5) and 9/7 (wl 5, qs 0.5), as ms per frame:
  (a) a loop of n picsong_encode_rgb_frame calls on one stream -- measured TWICE per round (legs a1, a2), so the run
      carries its own spread: max - min over all of (a)'s round values;
  (b) one picsong_encode_rgb_frames call of n;
  (c), (d) the same pair for decode (picsong_decode_rgb_frame / picsong_decode_rgb_frames; (c) twice as well).
n in {1, 2, 4} at both sizes and 8 at 4K.  HIP events bracket `calls` calls, the legs alternate within a round, the median
of the rounds is reported.  Device-resident frames (and streams) rotate over --pool MB of distinct buffers, past the 256
MiB Infinity Cache.  Before timing, the batched calls' streams and planes are checked against the single-frame calls'.
Conditions (margin = the spread of (a)): n = 1: (b) within the spread of (a); 4K, n = 4: (b) below (a) by more than it.
One JSON line.

    python tools/rgb_frames_bench.py [--rounds=5] [--pool=320] [--sizes=4k,8k] [--modes=53,97] [--n=1,2,4,8] [--legs=all|batched]

--legs=batched runs only (b) and (d): what a kernel-trace run wants (one n a run, so the kernels' totals are that n's)."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-image-and-video-codec_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import oracle_lib as orc
import picsong_amd as pa

opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
rounds = int(opts.get("rounds", 5))
pool = int(opts.get("pool", 320)) * 1000 * 1000
sizes = [s for s in opts.get("sizes", "4k,8k").split(",") if s]
modes = [m for m in opts.get("modes", "53,97").split(",") if m]
ns = [int(x) for x in opts.get("n", "1,2,4,8").split(",")]
only_batched = opts.get("legs", "all") == "batched"
DIMS = {"4k": (3840, 2160), "8k": (7680, 4320)}
assert torch.cuda.is_available(), "no GPU: nothing to time"


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_legs(legs, calls, frames_per_call):
    """{name: fn(i)} -> {name: [ms per frame of every round]}, the legs alternating within a round"""
    for fn in legs.values():                                 # warm-up: code objects, the context's buffers
        fn(0)
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(timed(fn, calls) / (calls * frames_per_call))
    return out


def case(size, mode, n):
    W, H = DIMS[size]
    lossy = mode == "97"
    wl, qs = 5, (0.5 if lossy else 1.0)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless"), rgb=True)
    P, ms = c.P, c.max_stream_shorts()
    # groups of n frames, R, G, B back to back per frame: enough of them to leave the Infinity Cache between two uses
    G = max(2, -(-pool // (3 * P * n)))
    contents = [torch.from_numpy(np.stack([orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + k)) for k in range(3)])).cuda() for f in range(4)]
    frames = torch.empty((G, n, 3, c.ah, c.aw), dtype=torch.uint8, device="cuda")
    for g in range(G):
        for f in range(n):
            frames[g, f] = contents[(g * n + f) % 4]
    streams = torch.zeros((G, 3 * n, ms), dtype=torch.int16, device="cuda")
    planes = torch.empty((G, n, 3, c.ah, c.aw), dtype=torch.uint8, device="cuda")
    L, h, s, vp = c.L, c.h, c._stream(), C.c_void_p

    def at(t, *idx):
        return vp(t[idx].data_ptr())

    def enc_loop(i):
        g = i % G
        for f in range(n):
            pa._check(L.picsong_encode_rgb_frame(h, at(frames, g, f, 0), at(frames, g, f, 1), at(frames, g, f, 2), 7 if f == 0 else 0,
                                                 at(streams, g, 3 * f), ms, s))

    def enc_batch(i):
        g = i % G
        pa._check(L.picsong_encode_rgb_frames(h, n, at(frames, g, 0, 0), at(frames, g, 0, 1), at(frames, g, 0, 2), 3 * P, 0, 7,
                                              at(streams, g, 0), ms, s))

    def dec_loop(i):
        g = i % G
        for f in range(n):
            pa._check(L.picsong_decode_rgb_frame(h, at(streams, g, 3 * f), ms, at(planes, g, f, 0), at(planes, g, f, 1), at(planes, g, f, 2), s))

    def dec_batch(i):
        g = i % G
        pa._check(L.picsong_decode_rgb_frames(h, n, at(streams, g, 0), ms, at(planes, g, 0, 0), at(planes, g, 0, 1), at(planes, g, 0, 2),
                                              3 * P, s))

    # ---- the results must not differ: group 0 through both forms, streams and planes compared; then every group's streams
    # (a kernel-trace run launches the batched calls only, so that a kernel's total is theirs)
    if not only_batched:
        enc_loop(0)
        torch.cuda.synchronize()
        want = streams[0].clone()
        streams[0].zero_()
        enc_batch(0)
        totals = c.last_totals(3 * n)
        for z in range(3 * n):
            assert torch.equal(streams[0, z, :totals[z]], want[z, :totals[z]]), f"{size} {mode} n={n}: stream {z} differs"
        dec_loop(0)
        torch.cuda.synchronize()
        want_px = planes[0].clone()
        planes[0].zero_()
        dec_batch(0)
        torch.cuda.synchronize()
        assert torch.equal(planes[0], want_px), f"{size} {mode} n={n}: decoded planes differ"
    for g in range(0 if only_batched else 1, G):
        enc_batch(g)
    if only_batched:
        dec_batch(0)
    torch.cuda.synchronize()
    if not lossy:
        assert torch.equal(planes[0], frames[0]), "5/3 round trip is not the identity"

    calls = max(4, 32 // n)
    if only_batched:
        r = run_legs({"b": enc_batch, "d": dec_batch}, calls, n)
        res = {k: round(statistics.median(v), 4) for k, v in r.items()}
        # every launch of the run is one of these calls' (the kernels' totals of a trace divide by these)
        res.update(encode_calls=G + 1 + rounds * calls, decode_calls=2 + rounds * calls)
    else:
        e = run_legs({"a1": enc_loop, "b": enc_batch, "a2": enc_loop}, calls, n)
        d = run_legs({"c1": dec_loop, "d": dec_batch, "c2": dec_loop}, calls, n)
        res = {}
        for lo, one, two, r in (("encode", "a1", "a2", e), ("decode", "c1", "c2", d)):
            single = r[one] + r[two]
            batch = r["b" if lo == "encode" else "d"]
            a, b = statistics.median(single), statistics.median(batch)
            res[lo] = {"single_ms": round(a, 4), "single_legs_ms": [round(statistics.median(r[one]), 4), round(statistics.median(r[two]), 4)],
                       "spread_ms": round(max(single) - min(single), 4), "batched_ms": round(b, 4),
                       "batched_range_ms": [round(min(batch), 4), round(max(batch), 4)], "batched_over_single": round(b / a, 4)}
    res.update(groups_rotated=G, calls_per_round=calls, megapixels_per_frame=round(W * H / 1e6, 3))
    c.close()
    del frames, streams, planes, contents
    torch.cuda.empty_cache()
    return res


results, conditions = {}, []
for size in sizes:
    for mode in modes:
        for n in ns:
            if n == 8 and size != "4k":
                continue
            key = f"{size}/{'9/7' if mode == '97' else '5/3'}/n={n}"
            results[key] = r = case(size, mode, n)
            if only_batched:
                continue
            for lo in ("encode", "decode"):
                x = r[lo]
                if n == 1:
                    conditions.append({"case": key, "leg": lo, "what": "n = 1: batched within the spread of single",
                                       "holds": abs(x["batched_ms"] - x["single_ms"]) <= x["spread_ms"]})
                if n == 4 and size == "4k":
                    conditions.append({"case": key, "leg": lo, "what": "4K, n = 4: batched below single by more than the spread",
                                       "holds": x["single_ms"] - x["batched_ms"] > x["spread_ms"]})

print(json.dumps({"gpu": torch.cuda.get_device_name(0), "rounds": rounds, "pool_mbytes": pool // 1000000, "wl": 5, "qs_97": 0.5,
                  "results": results, "conditions": conditions}))
