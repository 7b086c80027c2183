#!/usr/bin/env python3
"""Times the reduced-quality decode (picsong_ctx_set_decode_drop): ms per 8K grey frame of picsong_decode_frames -- three
frames a call, and a lone frame -- for drop = 0..6, with the PSNR of each against the source (picsong_frames_sse), on

  53    5/3 (lossless), wl 5
  97    9/7, qs 0.5, wl 6

A leg is `calls` decode calls on resident streams between two device synchronisations (host clock).  The legs of a round
run one after the other -- drop 0 (d0a), the parent commit's library at drop 0 (--parent=<its libpicsong_hip.so>; without
it: this library once more), drop 1 .. 6, drop 0 again (d0b) -- and the median over the rounds is reported.  The run's own
spread is max - min over all d0a and d0b values.  What must hold, and is reported as booleans: this library at drop 0 is
within the spread of the parent, and the time does not rise with drop (beyond the spread).

Before timing, drop = 0 is checked to give the parent's bytes, and the three frames of a call the lone frame's.
One JSON object, printed and written to --out.

    python tools/drop_bench.py [--parent=build/parent/libpicsong_hip.so] [--rounds=7] [--calls=40] [--size=8k]
                               [--modes=53,97] [--out=profiles/drop_bench.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-image-and-video-codec_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import oracle_lib as orc
import picsong_amd as pa

opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
rounds = int(opts.get("rounds", 7))
calls = int(opts.get("calls", 40))
size = opts.get("size", "8k")
modes = [m for m in opts.get("modes", "53,97").split(",") if m]
parent_so = opts.get("parent", "")
out_path = opts.get("out", os.path.join(ROOT, "profiles", "drop_bench.json"))
DIMS = {"8k": (7680, 4320), "4k": (3840, 2160), "tiny": (704, 512)}
MODES = {"53": dict(lossy=False, qs=1.0, wl=5), "97": dict(lossy=True, qs=0.5, wl=6)}
DROPS = list(range(7))
N = 3
assert torch.cuda.is_available(), "no GPU: nothing to time"

pa.load()                                                   # this tree's library
if parent_so:                                               # ... and the parent's beside it: contexts keep the one they were made with
    this_lib, pa._lib, pa.SO_PATH = pa._lib, None, os.path.abspath(parent_so)
    parent_lib = pa.load()
    pa._lib = this_lib
else:
    parent_lib = None


def codec(W, H, m, lib=None):
    keep = pa._lib
    if lib is not None:
        pa._lib = lib
    try:
        return pa.Codec(W, H, wl=m["wl"], lossy=m["lossy"], qs=m["qs"], lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if m["lossy"] else "n1_lossless"))
    finally:
        pa._lib = keep


def med(x):
    return round(statistics.median(x), 4)


def mode(name):
    m = MODES[name]
    W, H = DIMS[size]
    if size == "tiny":
        m = dict(m, wl=3)
    mine = codec(W, H, m)
    theirs = codec(W, H, m, parent_lib) if parent_lib else codec(W, H, m)
    frames = torch.from_numpy(orc.pad_frame(orc.gen_frame(W, H, 0))).cuda().reshape(1, -1).repeat(N, 1)
    s = mine.encode_frame(frames[0].view(mine.ah, mine.aw)).clone()
    streams = torch.stack([torch.nn.functional.pad(s, (0, mine.max_stream_shorts() - s.numel())) for _ in range(N)])
    out3 = torch.empty((N, mine.ah, mine.aw), dtype=torch.uint8, device="cuda")
    out1 = torch.empty((1, mine.ah, mine.aw), dtype=torch.uint8, device="cuda")

    def leg(c, drop, n):
        """ms per frame of `calls` decode calls of n frames under `drop`"""
        if drop is not None:
            c.set_decode_drop(drop)
        o, st = (out3, streams) if n == N else (out1, streams[:1])
        c.decode_frames(st, o)                              # warm-up: the code object of this drop's kernels, the buffers
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            c.decode_frames(st, o)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (calls * n)

    # what the legs decode: the PSNR by drop, drop 0 against the parent, a call's three frames against the lone frame
    psnr = {}
    for d in DROPS:
        mine.set_decode_drop(d)
        mine.decode_frames(streams, out3)
        mine.decode_frames(streams[:1], out1)
        assert all(torch.equal(out3[f], out1[0]) for f in range(N)), d
        sse = int(mine.frames_sse(out1.view(1, -1), frames[:1])[0].item())
        psnr[d] = round(pa.sse_to_psnr(sse, W * H), 3) if sse else None     # None: exact
        if d == 0:
            ref = theirs.decode_frames(streams[:1]).clone()
            assert torch.equal(ref, out1), "drop 0 is not the parent's decode"
    doc = {"psnr_db": psnr, "stream_shorts": int(s.numel())}
    for n, key in ((N, "three_frames_a_call"), (1, "lone_frame")):
        legs = [("d0a", mine, 0), ("parent", theirs, None if parent_lib else 0)] + [(f"d{d}", mine, d) for d in DROPS[1:]] + [("d0b", mine, 0)]
        ms = {k: [] for k, _, _ in legs}
        for _ in range(rounds):
            for k, c, d in legs:
                ms[k].append(leg(c, d, n))
        zero = ms["d0a"] + ms["d0b"]
        spread = max(zero) - min(zero)
        by_drop = [med(zero)] + [med(ms[f"d{d}"]) for d in DROPS[1:]]
        doc[key] = {"ms_per_frame_by_drop": by_drop, "drop0_a_ms": med(ms["d0a"]), "drop0_b_ms": med(ms["d0b"]),
                    "parent_is": "the parent commit's library" if parent_lib else "this library, drop 0",
                    "parent_ms": med(ms["parent"]), "spread_ms": round(spread, 4),
                    "drop0_minus_parent_ms": round(med(zero) - med(ms["parent"]), 4),
                    "drop0_within_spread_of_parent": abs(med(zero) - med(ms["parent"])) <= spread,
                    "time_does_not_rise_with_drop": all(by_drop[i + 1] <= by_drop[i] + spread for i in range(len(by_drop) - 1)),
                    "ranges_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}
    mine.close()
    theirs.close()
    return doc


results = {}
for name in modes:
    results[name] = mode(name)
    print(name, json.dumps(results[name]), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()

doc = json.dumps({"gpu": torch.cuda.get_device_name(0), "size": size, "rounds": rounds, "calls_per_leg": calls, "frames_a_call": N,
                  "parent_library": bool(parent_lib), "modes": {k: MODES[k] for k in modes}, "results": results})
print(doc)
with open(out_path, "w") as f:
    f.write(doc + "\n")
