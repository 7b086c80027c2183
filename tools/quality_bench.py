#!/usr/bin/env python3
"""Times the quality calls on one 8K 9/7 frame (wl 6, whole grid), the legs alternating in one process:
  (a) the quality call as shipped (picsong_encode_frame_quality / picsong_encode_rgb_frame_quality);
  (b) one rate call (picsong_encode_frame_rate / picsong_encode_rgb_frame_rate) for the size (a) produced;
  (c) one plain picsong_encode_frame (+ picsong_last_total) at the quantiser (a) chose.
Every leg ends in a device synchronise (the calls are synchronous); host wall clock, median of the rounds.  Then, with the
context's stage timers armed (picsong_profile_begin), one more quality call: per probe the HIP-event times of the quantise
pass, the synthesis and the SSE, their medians over the call's probes.  Last, sse_kernel alone (picsong_frames_sse over two
frames, HIP events around `calls` launches) as bytes per second.  Checks the stream against the plain encode at the chosen
quantiser, and the SSE against the library's own decode, before timing.  One JSON line.

    python tools/quality_bench.py [grey|rgb] [--psnr=40] [--rounds=R] [--calls=C]"""
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
mode = args[0] if args else "grey"
rgb = mode == "rgb"
psnr, rounds, calls = float(opts.get("psnr", 40.0)), int(opts.get("rounds", 7)), int(opts.get("calls", 5))
W, H, wl = int(opts.get("w", 7680)), int(opts.get("h", 4320)), int(opts.get("wl", 6))
assert torch.cuda.is_available(), "no GPU: nothing to time"
ncomp = 3 if rgb else 1
limit = pa.psnr_to_sse(psnr, W * H * ncomp)

lut = os.path.join(orc.LUT_DIR, "n1_lossy")
c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=lut, rgb=rgb)
planes = [torch.from_numpy(orc.pad_frame(orc.gen_frame(W, H, i))).cuda() for i in range(ncomp)]
out = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
out_p = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")


def quality_call():
    if rgb:
        j, s, e = c.encode_rgb_frame_quality(*planes, limit)
        return j, [x.numel() for x in s], e, s
    j, s, e = c.encode_frame_quality(planes[0], limit, out=out[0])
    return j, [s.numel()], [e], [s]


def rate_call(target):
    if rgb:
        return c.encode_rgb_frame_rate(*planes, target)[0]
    return c.encode_frame_rate(planes[0], target, out=out_p[0])[0]


def plain(codec, buf):
    if rgb:
        pa._check(codec.L.picsong_encode_rgb_frame(codec.h, *[codec._p(p) for p in planes], 1, codec._p(buf), buf.stride(0),
                                                   codec._stream()))
        return codec.last_totals(3)
    codec.encode_frame_async(planes[0], buf[0], 0)
    return [codec.last_total()]


# ---- the result is what the plain calls give at the chosen quantiser, before anything is timed
j, totals, sse, streams = quality_call()
streams = [s.clone() for s in streams]
at_j = pa.Codec(W, H, wl=wl, lossy=True, qs=min(pa.rate_qs(j), 1.0), lut_folder=lut, rgb=rgb)
if pa.rate_qs(j) > 1.0:
    at_j.set_qs(pa.rate_qs(j))
assert plain(at_j, out_p) == totals
assert all(torch.equal(streams[k], out_p[k, :totals[k]]) for k in range(ncomp)), "the stream differs from the plain encode at the chosen qs"
if rgb:
    dec = at_j.decode_rgb_frame(out_p)
    own = at_j.frames_sse(torch.stack([d.view(-1) for d in dec]), torch.stack([p.view(-1) for p in planes]))
else:
    own = at_j.frames_sse(at_j.decode_frame(out_p[0]).view(-1), planes[0].view(-1))
assert [int(v) for v in own] == sse and sum(sse) <= limit, (own, sse, limit)
target = sum(totals)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


legs = {"a_quality_call": quality_call, "b_rate_call": lambda: rate_call(target), "c_plain_encode": lambda: plain(at_j, out_p)}
for fn in legs.values():
    fn()
ms = {k: [] for k in legs}
for r in range(rounds):                                    # the legs alternate: drift hits them alike
    for k, fn in legs.items():
        ms[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in ms.items()}

# ---- the probes' stages, by the context's HIP-event timers
c.profile_begin(64)
quality_call()
stages = c.profile_read(64).astype(np.float64)
c.profile_begin(0)
probe = {k: round(float(np.median(stages[:, i])), 4) for i, k in enumerate(("quantise_ms", "synthesis_ms", "sse_ms"))}
probe["probe_ms"] = round(float(np.median(stages.sum(axis=1))), 4)

# ---- sse_kernel alone
a = planes[0].view(-1)
b = torch.roll(a, 1).contiguous()
res = torch.empty(1, dtype=torch.int64, device="cuda")
for _ in range(3):
    c.frames_sse(a, b, out=res)
sse_ms = []
for r in range(rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        c.frames_sse(a, b, out=res)
    e1.record()
    torch.cuda.synchronize()
    sse_ms.append(e0.elapsed_time(e1) / calls)
sse_med = statistics.median(sse_ms)
# (the bytes the kernel has to read: the visible part of both frames, whole 16-byte vectors a row)
sse_bytes = 2 * H * ((W + 15) // 16 * 16)

print(json.dumps({
    "mode": mode, "gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "wl": wl, "psnr": psnr, "max_sse": limit,
    "j": j, "sse": sse, "stream_shorts": totals, "probes_recorded": int(stages.shape[0]),
    "rounds": rounds, "calls_per_round": calls,
    "ms_per_call": {k: round(v, 3) for k, v in med.items()},
    "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
    "per_probe_ms": probe,
    "sse_kernel": {"ms": round(sse_med, 4), "spread_ms": [round(min(sse_ms), 4), round(max(sse_ms), 4)],
                   "bytes": sse_bytes, "gbytes_per_s": round(sse_bytes / sse_med / 1e6, 1)}}))
