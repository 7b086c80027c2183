#!/usr/bin/env python3
"""Times the SSIM measure and the SSIM search call on 8K frames (9/7, wl 6, whole grid), in one process.
  1. ssim_kernel alone: picsong_frames_dssim over three 8K frame pairs a launch, HIP events around `calls` launches, beside
     sse_kernel (picsong_frames_sse over the same pairs) timed TWICE a round -- before and after it -- so that the run's own
     spread stands next to the difference.  ms a frame and bytes per second (the bytes each kernel has to read: the
     visible part of both frames for the SSE; the rows and columns that carry windows for the SSIM).
  2. the search calls, the legs alternating: (a) picsong_encode_frame_ssim at the SSIM target, (b)
     picsong_encode_frame_quality at the PSNR target, (c) one plain picsong_encode_frame (+ picsong_last_total) at the
     quantiser (a) chose.  Host wall clock around synchronous calls, median of the rounds.
  3. with the context's stage timers armed (picsong_profile_begin), one more SSIM call: per probe the HIP-event times of
     the quantise pass, the synthesis and the SSIM kernel, their medians over the call's probes; the same for a PSNR call.
Checks the stream against the plain encode at the chosen quantiser, and the DSSIM sum against the library's own decode,
before timing.  One JSON line.

    python tools/ssim_bench.py [--ssim=0.98] [--psnr=40] [--rounds=R] [--calls=C] [--kernel-calls=K]"""
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

opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ssim, psnr = float(opts.get("ssim", 0.98)), float(opts.get("psnr", 40.0))
rounds, calls, kcalls = int(opts.get("rounds", 7)), int(opts.get("calls", 3)), int(opts.get("kernel-calls", 200))
W, H, wl = int(opts.get("w", 7680)), int(opts.get("h", 4320)), int(opts.get("wl", 6))
assert torch.cuda.is_available(), "no GPU: nothing to time"
windows = pa.ssim_windows(W, H)
limit = pa.ssim_to_dssim(ssim, windows)
max_sse = pa.psnr_to_sse(psnr, W * H)

lut = os.path.join(orc.LUT_DIR, "n1_lossy")
c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=lut)
frame = torch.from_numpy(orc.pad_frame(orc.gen_frame(W, H, 0))).cuda()
out = torch.zeros((2, c.max_stream_shorts()), dtype=torch.int16, device="cuda")

# ---- the result is what the plain call gives at the chosen quantiser, before anything is timed
j, stream, dssim = c.encode_frame_ssim(frame, limit, out=out[0])
stream = stream.clone()
at_j = pa.Codec(W, H, wl=wl, lossy=True, qs=min(pa.rate_qs(j), 1.0), lut_folder=lut)
if pa.rate_qs(j) > 1.0:
    at_j.set_qs(pa.rate_qs(j))


def plain():
    at_j.encode_frame_async(frame, out[1], 0)
    return at_j.last_total()


total = plain()
assert total == stream.numel() and torch.equal(stream, out[1, :total]), "the stream differs from the plain encode at the chosen qs"
own = at_j.frames_dssim(at_j.decode_frame(out[1]).view(-1), frame.view(-1))
assert int(own[0]) == dssim <= limit, (own, dssim, limit)
jq, _, sse = c.encode_frame_quality(frame, max_sse, out=out[0])

# ---- 1. the kernels alone, three frames a launch
a = torch.stack([torch.from_numpy(orc.pad_frame(orc.gen_frame(W, H, i))).view(-1) for i in range(3)]).cuda()
b = torch.roll(a, 1, dims=1).contiguous()
res = torch.empty(3, dtype=torch.int64, device="cuda")


def kernel_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(kcalls):
        fn(a, b, out=res)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / kcalls / 3.0              # a frame


for fn in (c.frames_sse, c.frames_dssim):
    for _ in range(3):
        fn(a, b, out=res)
k_ms = {"sse_first": [], "ssim": [], "sse_second": []}
for r in range(rounds):
    k_ms["sse_first"].append(kernel_ms(c.frames_sse))
    k_ms["ssim"].append(kernel_ms(c.frames_dssim))
    k_ms["sse_second"].append(kernel_ms(c.frames_sse))
k_med = {k: statistics.median(v) for k, v in k_ms.items()}
sse_bytes = 2 * H * ((W + 15) // 16 * 16)
nx, ny = (W - 8) // 4 + 1, (H - 8) // 4 + 1
ssim_bytes = 2 * 4 * (ny + 1) * 4 * (nx + 1)


# ---- 2. the calls
def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


legs = {"a_ssim_call": lambda: c.encode_frame_ssim(frame, limit, out=out[0]),
        "b_psnr_call": lambda: c.encode_frame_quality(frame, max_sse, out=out[0]),
        "c_plain_encode": plain}
for fn in legs.values():
    fn()
ms = {k: [] for k in legs}
for r in range(rounds):                                    # the legs alternate: drift hits them alike
    for k, fn in legs.items():
        ms[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in ms.items()}


# ---- 3. the probes' stages, by the context's HIP-event timers
def stages_of(fn, last):
    c.profile_begin(64)
    fn()
    st = c.profile_read(64).astype(np.float64)
    c.profile_begin(0)
    d = {k: round(float(np.median(st[:, i])), 4) for i, k in enumerate(("quantise_ms", "synthesis_ms", last))}
    d["probe_ms"] = round(float(np.median(st.sum(axis=1))), 4)
    d["probes_recorded"] = int(st.shape[0])
    return d


print(json.dumps({
    "gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "wl": wl, "ssim": ssim, "windows": windows, "max_dssim": limit,
    "j": j, "dssim": dssim, "ssim_achieved": round(pa.dssim_to_ssim(dssim, windows), 6), "stream_shorts": total,
    "psnr": psnr, "max_sse": max_sse, "psnr_j": jq, "psnr_sse": sse,
    "rounds": rounds, "calls_per_round": calls, "kernel_calls_per_round": kcalls, "frames_per_launch": 3,
    "kernels_ms_per_frame": {k: round(v, 4) for k, v in k_med.items()},
    "kernels_spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in k_ms.items()},
    "sse_kernel": {"bytes": sse_bytes, "gbytes_per_s": round(sse_bytes / min(k_med["sse_first"], k_med["sse_second"]) / 1e6, 1)},
    "ssim_kernel": {"bytes": ssim_bytes, "gbytes_per_s": round(ssim_bytes / k_med["ssim"] / 1e6, 1),
                    "windows_per_s": round(windows / k_med["ssim"] * 1e3),
                    "over_sse": round(k_med["ssim"] / min(k_med["sse_first"], k_med["sse_second"]), 3)},
    "ms_per_call": {k: round(v, 3) for k, v in med.items()},
    "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
    "per_probe_ms_ssim": stages_of(legs["a_ssim_call"], "ssim_ms"),
    "per_probe_ms_psnr": stages_of(legs["b_psnr_call"], "sse_ms")}))
