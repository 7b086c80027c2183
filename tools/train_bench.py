#!/usr/bin/env python3
"""Times picsong_train_frames (transform + statistics kernel) beside picsong_encode_frames (transform + coder + pack)
at n = 3 on the bench's device-resident frames, the two alternating in one process; prints ms per frame of each, their
ratio, and the statistics kernel alone (picsong_train_coeffs on one frame's resident coefficients) as one JSON line.
The encode path is the library's own: this tool changes nothing in it.

    python tools/train_bench.py [8k_lossless|8k_lossy|4k_lossless] [--rounds=R] [--calls=C]"""
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

# bench.py's workloads: (W, H, wl, lossy, qs)
WORKLOADS = {"8k_lossless": (7680, 4320, 5, False, 1.0), "4k_lossless": (3840, 2160, 5, False, 1.0),
             "8k_lossy": (7680, 4320, 6, True, 0.5)}

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
workload = args[0] if args else "8k_lossless"
rounds, calls, n = int(opts.get("rounds", 7)), int(opts.get("calls", 20)), 3
W, H, wl, lossy, qs = WORKLOADS[workload]
assert torch.cuda.is_available(), "no GPU: nothing to time"

lut = os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
enc = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=lut)
trn = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs)
trn.train_begin()
pool = torch.from_numpy(np.stack([orc.pad_frame(orc.gen_frame(W, H, i)).reshape(-1) for i in range(2 * n)])).cuda()
out = torch.empty((n, enc.max_stream_shorts()), dtype=torch.int16, device="cuda")
coef = trn.dwt_forward(pool[0])[:trn.P].clone()            # one frame's Mallat array, 32-bit


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


legs = {
    "train_frames": lambda i: trn.train_frames(pool[(i % 2) * n:(i % 2) * n + n]),
    "encode_frames": lambda i: enc.encode_frames_async(pool[(i % 2) * n:(i % 2) * n + n], out, 1),
    "train_coeffs": lambda i: trn.train_coeffs(coef),
}
for fn in legs.values():                                   # warm every shape the timed windows use
    for i in range(3):
        fn(i)
torch.cuda.synchronize()
ms = {k: [] for k in legs}
for r in range(rounds):                                    # the legs alternate: drift hits them alike
    for k, fn in legs.items():
        ms[k].append(timed(fn) / (1 if k == "train_coeffs" else n))
med = {k: statistics.median(v) for k, v in ms.items()}
symbols = int(trn.train_counts(0).sum())
print(json.dumps({
    "workload": workload, "frames_per_call": n, "rounds": rounds, "calls_per_round": calls,
    "train_frames_ms_per_frame": round(med["train_frames"], 4), "encode_frames_ms_per_frame": round(med["encode_frames"], 4),
    "train_over_encode": round(med["train_frames"] / med["encode_frames"], 3),
    "stats_kernel_ms_per_frame": round(med["train_coeffs"], 4),
    "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
    "symbols_counted": symbols, "range_flag": trn.range_flag()}))
