#!/usr/bin/env python3
"""Times the rate calls on one 8K 9/7 frame (wl 6, whole grid), the legs alternating in one process:
  (a) the rate call as shipped (picsong_encode_frame_rate / picsong_encode_rgb_frame_rate);
  (b) the same with one candidate a round (PICSONG_RATE_K=1);
  (c) the loop a user could write without the rate calls: per probe of the same bisection picsong_ctx_set_qs +
      picsong_encode_frame + picsong_last_total (the fused transform, a lone-frame coder and a pack, every probe);
  (d) one plain picsong_encode_frame (+ picsong_last_total) at the chosen qs.
Every leg ends in a device synchronise (the calls are synchronous); host wall clock, median of the rounds.  Checks that
(a), (b) and (c) choose the same j and produce the same stream before timing.  One JSON line.

    python tools/rate_bench.py [grey|rgb] [--bpp=2.0] [--rounds=R] [--calls=C]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-image-and-video-codec_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import oracle_lib as orc
import picsong_amd as pa
import rate_ref as rr

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
mode = args[0] if args else "grey"
rgb = mode == "rgb"
bpp, rounds, calls = float(opts.get("bpp", 2.0)), int(opts.get("rounds", 7)), int(opts.get("calls", 5))
W, H, wl = int(opts.get("w", 7680)), int(opts.get("h", 4320)), int(opts.get("wl", 6))
assert torch.cuda.is_available(), "no GPU: nothing to time"
target = int(bpp * W * H / 16)
GRID = rr.grid()

lut = os.path.join(orc.LUT_DIR, "n1_lossy")
c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=lut, rgb=rgb)
naive = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=lut, rgb=rgb)
planes = [torch.from_numpy(orc.pad_frame(orc.gen_frame(W, H, i))).cuda() for i in range(3 if rgb else 1)]
out = torch.empty((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
out_n = torch.empty((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")


def rate_call(k):
    if k == 1:
        os.environ["PICSONG_RATE_K"] = "1"
    else:
        os.environ.pop("PICSONG_RATE_K", None)
    if rgb:
        j, s = c.encode_rgb_frame_rate(*planes, target)
        return j, [x.numel() for x in s]
    j, s = c.encode_frame_rate(planes[0], target, out=out[0])
    return j, [s.numel()]


def plain(codec, buf):
    if rgb:
        pa._check(codec.L.picsong_encode_rgb_frame(codec.h, *[codec._p(p) for p in planes], 1, codec._p(buf), buf.stride(0),
                                                   codec._stream()))
        return codec.last_totals(3)
    codec.encode_frame_async(planes[0], buf[0], 0)
    return [codec.last_total()]


def naive_loop():
    """The procedure of rate_ref.bisect, a context re-tuned and a whole encode per probe."""
    lo, hi, probes = -1, len(GRID), 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        naive.set_qs(pa.rate_qs(GRID[mid]))
        probes += 1
        if sum(plain(naive, out_n)) <= target:
            lo = mid
        else:
            hi = mid
    if lo < 0:
        return 0, [], probes
    naive.set_qs(pa.rate_qs(GRID[lo]))                     # the final stream: the last fitting probe's, coded once more
    return GRID[lo], plain(naive, out_n), probes + 1


# ---- the three ways agree before anything is timed
ja, ta = rate_call(3)
sa = [out[k, :ta[k]].clone() for k in range(len(ta))] if not rgb else None
jb, tb = rate_call(1)
jc, tc, encodes = naive_loop()
assert ja == jb == jc and ta == tb == tc, (ja, jb, jc, ta, tb, tc)
if not rgb:
    assert torch.equal(sa[0], out_n[0, :tc[0]]), "the rate call's stream differs from the plain encode at the chosen qs"
c.set_qs(pa.rate_qs(ja))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


legs = {"a_rate_call": lambda: rate_call(3), "b_rate_call_k1": lambda: rate_call(1), "c_naive_loop": naive_loop,
        "d_plain_encode": lambda: plain(c, out)}
for fn in legs.values():
    fn()
ms = {k: [] for k in legs}
for r in range(rounds):                                    # the legs alternate: drift hits them alike
    for k, fn in legs.items():
        ms[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in ms.items()}
print(json.dumps({
    "mode": mode, "gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "wl": wl, "bpp": bpp, "target_shorts": target,
    "j": ja, "stream_shorts": ta, "probes": 14 if ja else 13, "naive_encodes": encodes,
    "rounds": rounds, "calls_per_round": calls,
    "ms_per_call": {k: round(v, 3) for k, v in med.items()},
    "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}}))
