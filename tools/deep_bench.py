#!/usr/bin/env python3
"""Times the deep contexts' frame calls on 8K 12-bit frames, three a call: picsong_encode_frames16 and
picsong_decode_frames16 (HIP events around `calls` calls, median of the rounds, ms per FRAME), beside
  - the same calls under PICSONG_DEEP_NOFUSE=1 (element-wise level shift / clamp passes instead of the kernels' uint16
    load and store stages), and
  - picsong_encode_frames / picsong_decode_frames of an 8-bit context created under PICSONG_C16=0 (the 32-bit coefficient
    form: the comparable path) on the frames' top 8 bits, timed TWICE a round: the difference of the two is the run's own
    spread, the yardstick for "not slower than".
The legs alternate within a round.  5/3 wl 5 and 9/7 wl 6; the frames are deep_ref's `smooth` content.  Before anything is
timed the CPU oracle transforms one frame: a configuration whose coefficients reach 2^15 (the coders' range) is not run.
Streams and decoded samples of the two deep routes are compared before timing.  One JSON line.

    python tools/deep_bench.py [--rounds=R] [--calls=C] [--w=7680] [--h=4320] [--bd=12] [--qs=0.25]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-image-and-video-codec_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import deep_ref as D
import oracle_lib as orc
import picsong_amd as pa

opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
rounds, calls = int(opts.get("rounds", 7)), int(opts.get("calls", 5))
W, H, bd, N = int(opts.get("w", 7680)), int(opts.get("h", 4320)), int(opts.get("bd", 12)), 3
qs97 = float(opts.get("qs", 0.25))
assert torch.cuda.is_available(), "no GPU: nothing to time"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls / N


def nofuse(fn):
    def call():
        os.environ["PICSONG_DEEP_NOFUSE"] = "1"
        try:
            fn()
        finally:
            del os.environ["PICSONG_DEEP_NOFUSE"]
    return call


def legs_alternating(legs):
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}


pads = [D.mirror_pad(D.inputs("smooth", bd, 5 + f, W, H)) for f in range(N)]
results = {}
for name, lossy, wl, qs in (("5/3", False, 5, 1.0), ("9/7", True, 6, qs97)):
    peak = D.max_coef(D.forward(pads[0], bd, wl, lossy, qs)[:pads[0].size])
    if peak >= 32768:
        results[name] = {"skipped": f"max |coefficient| {peak} on the CPU oracle reaches 2^15: not run"}
        continue
    lut = os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    deep = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=lut, bit_depth=bd)
    os.environ["PICSONG_C16"] = "0"
    os.environ["PICSONG_DEC_C16"] = "0"
    flat = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=lut)
    del os.environ["PICSONG_C16"], os.environ["PICSONG_DEC_C16"]
    f16 = torch.from_numpy(np.stack(pads).view(np.int16)).cuda().view(N, -1)
    f8 = torch.from_numpy(np.stack([(p >> (bd - 8)).astype(np.uint8) for p in pads])).cuda().view(N, -1)
    s16 = torch.zeros((N, deep.max_stream_shorts()), dtype=torch.int16, device="cuda")
    s8 = torch.zeros_like(s16)
    o16 = torch.zeros((N, deep.P), dtype=torch.int16, device="cuda")
    o8 = torch.zeros((N, deep.P), dtype=torch.uint8, device="cuda")
    st = deep._stream()

    def enc16():
        pa._check(deep.L.picsong_encode_frames16(deep.h, N, deep._p(f16), f16.stride(0) * 2, 0, deep._p(s16), s16.stride(0), st))

    def dec16():
        pa._check(deep.L.picsong_decode_frames16(deep.h, N, deep._p(s16), s16.stride(0), deep._p(o16), o16.stride(0) * 2, st))

    def enc8():
        flat.encode_frames_async(f8, s8, 0)

    def dec8():
        flat.decode_frames(s8, out=o8.view(N, flat.ah, flat.aw))

    # the two deep routes give the same bytes; the in-kernel route's streams decode to the oracle's samples (5/3: the input)
    enc16()
    totals = deep.last_totals(N)
    a = [s16[f, :totals[f]].clone() for f in range(N)]
    nofuse(enc16)()
    assert deep.last_totals(N) == totals and all(torch.equal(a[f], s16[f, :totals[f]]) for f in range(N)), "NOFUSE streams differ"
    dec16()
    b = o16.clone()
    nofuse(dec16)()
    assert torch.equal(b, o16), "NOFUSE samples differ"
    if not lossy:
        assert torch.equal(o16, f16), "the 5/3 round trip is not exact"
    assert deep.range_flag() == 0
    enc8()
    totals8 = flat.last_totals(N)
    med_e, spread_e = legs_alternating({"encode_frames16": enc16, "u8_c32_a": enc8, "encode_frames16_nofuse": nofuse(enc16), "u8_c32_b": enc8})
    med_d, spread_d = legs_alternating({"decode_frames16": dec16, "u8_c32_a": dec8, "decode_frames16_nofuse": nofuse(dec16), "u8_c32_b": dec8})
    results[name] = {
        "wl": wl, "qs": qs, "max_abs_coefficient_cpu": peak,
        "stream_shorts_per_frame": {"deep": int(sum(totals) / N), "u8": int(sum(totals8) / N)},
        "encode_ms_per_frame": med_e, "encode_spread_ms": spread_e,
        "decode_ms_per_frame": med_d, "decode_spread_ms": spread_d,
        "encode_run_spread_ms": round(abs(med_e["u8_c32_a"] - med_e["u8_c32_b"]), 4),
        "decode_run_spread_ms": round(abs(med_d["u8_c32_a"] - med_d["u8_c32_b"]), 4),
        "encode_in_kernel_minus_nofuse_ms": round(med_e["encode_frames16"] - med_e["encode_frames16_nofuse"], 4),
        "decode_in_kernel_minus_nofuse_ms": round(med_d["decode_frames16"] - med_d["decode_frames16_nofuse"], 4),
    }
    deep.close()
    flat.close()
    del f16, f8, s16, s8, o16, o8
    torch.cuda.empty_cache()

print(json.dumps({"gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "bit_depth": bd, "frames_per_call": N, "rounds": rounds,
                  "calls_per_round": calls, "results": results}))
