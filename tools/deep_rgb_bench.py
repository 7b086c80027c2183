#!/usr/bin/env python3
"""Times the deep RGB contexts' frame calls on 4K 12-bit RGB frames, n = 1 and 4 a call: picsong_encode_rgb_frames16 and
picsong_decode_rgb_frames16 (HIP events around `calls` calls, median of the rounds, ms per FRAME), in three legs:
  1. the default route (the colour transform in level 0's load stage);
  2. PICSONG_DEEP_NOFUSE=1 (the colour transform as a launch of its own, the component planes written and read back);
  3. picsong_encode_rgb_frames / picsong_decode_rgb_frames of an 8-bit RGB context created under PICSONG_C16=0 (the 32-bit
     coefficient form: the comparable path) on the frames' top 8 bits with PICSONG_RGB_NOFUSE=1 read per call (its fused
     head and tails want 16-bit coefficients anyway), timed TWICE a round: the difference of the two is the run's own
     spread, the yardstick for "faster than".
The decode has one deep route (the synthesis writes the T planes, one inverse-transform launch follows): legs 1 and 3.
The legs alternate within a round.  5/3 wl 5 and 9/7 wl 6; the frames are deep_rgb_ref's `smooth` content.  Before anything
is timed the CPU oracle transforms one frame's components: a configuration whose coefficients reach 2^15 (the coders'
range) is not run.  Streams of the two encode routes are compared before timing.  One JSON line.

    python tools/deep_rgb_bench.py [--rounds=R] [--calls=C] [--w=3840] [--h=2160] [--bd=12] [--qs=0.25]"""
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
import deep_rgb_ref as R
import oracle_lib as orc
import picsong_amd as pa

opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
rounds, calls = int(opts.get("rounds", 7)), int(opts.get("calls", 5))
W, H, bd = int(opts.get("w", 3840)), int(opts.get("h", 2160)), int(opts.get("bd", 12))
qs97 = float(opts.get("qs", 0.25))
assert torch.cuda.is_available(), "no GPU: nothing to time"


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls / n


def with_env(name, fn):
    def call():
        os.environ[name] = "1"
        try:
            fn()
        finally:
            del os.environ[name]
    return call


def legs_alternating(legs, n):
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn, n))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}


NMAX = 4
pads = [[D.mirror_pad(R.inputs("smooth", bd, 5 + f, c, W, H)) for c in range(3)] for f in range(NMAX)]
results = {}
for name, lossy, wl, qs in (("5/3", False, 5, 1.0), ("9/7", True, 6, qs97)):
    comp = R.forward(pads[0][0], pads[0][1], pads[0][2], bd, lossy)
    peak = max(D.max_coef(orc.dwt_forward(np.ascontiguousarray(c), wl, qs)[:c.size]) for c in comp)
    if peak >= 32768:
        results[name] = {"skipped": f"max |coefficient| {peak} on the CPU oracle reaches 2^15: not run"}
        continue
    lut = os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    deep = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=lut, bit_depth=bd, is_rgb=True)
    os.environ["PICSONG_C16"] = "0"
    os.environ["PICSONG_DEC_C16"] = "0"
    flat = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=lut, rgb=True)
    del os.environ["PICSONG_C16"], os.environ["PICSONG_DEC_C16"]
    P = deep.P
    # frame f's R, G, B planes back to back: [NMAX, 3, P]
    f16 = torch.from_numpy(np.stack([np.stack(p) for p in pads]).view(np.int16)).cuda().view(NMAX, 3, P)
    f8 = torch.from_numpy(np.stack([np.stack([(x >> (bd - 8)).astype(np.uint8) for x in p]) for p in pads])).cuda().view(NMAX, 3, P)
    s16 = torch.zeros((3 * NMAX, deep.max_stream_shorts()), dtype=torch.int16, device="cuda")
    s8 = torch.zeros_like(s16)
    o16 = torch.zeros_like(f16)
    o8 = torch.zeros_like(f8)
    st = deep._stream()
    per_n = {}
    for n in (1, NMAX):
        def enc16():
            pa._check(deep.L.picsong_encode_rgb_frames16(deep.h, n, deep._p(f16[0, 0]), deep._p(f16[0, 1]), deep._p(f16[0, 2]), 6 * P, 0, 7,
                                                         deep._p(s16), s16.stride(0), st))

        def dec16():
            pa._check(deep.L.picsong_decode_rgb_frames16(deep.h, n, deep._p(s16), s16.stride(0), deep._p(o16[0, 0]), deep._p(o16[0, 1]),
                                                         deep._p(o16[0, 2]), 6 * P, st))

        def enc8():
            pa._check(flat.L.picsong_encode_rgb_frames(flat.h, n, flat._p(f8[0, 0]), flat._p(f8[0, 1]), flat._p(f8[0, 2]), 3 * P, 0, 7,
                                                       flat._p(s8), s8.stride(0), st))

        def dec8():
            pa._check(flat.L.picsong_decode_rgb_frames(flat.h, n, flat._p(s8), s8.stride(0), flat._p(o8[0, 0]), flat._p(o8[0, 1]),
                                                       flat._p(o8[0, 2]), 3 * P, st))

        enc8, dec8 = with_env("PICSONG_RGB_NOFUSE", enc8), with_env("PICSONG_RGB_NOFUSE", dec8)
        # the two deep encode routes give the same bytes; 5/3 decodes to the input
        enc16()
        totals = deep.last_totals(3 * n)
        a = [s16[z, :totals[z]].clone() for z in range(3 * n)]
        with_env("PICSONG_DEEP_NOFUSE", enc16)()
        assert deep.last_totals(3 * n) == totals and all(torch.equal(a[z], s16[z, :totals[z]]) for z in range(3 * n)), "NOFUSE streams differ"
        dec16()
        if not lossy:
            assert torch.equal(o16[:n], f16[:n]), "the 5/3 round trip is not exact"
        assert deep.range_flag() == 0
        enc8()
        totals8 = flat.last_totals(3 * n)
        med_e, spread_e = legs_alternating({"encode_rgb_frames16": enc16, "u8_c32_a": enc8,
                                            "encode_rgb_frames16_nofuse": with_env("PICSONG_DEEP_NOFUSE", enc16), "u8_c32_b": enc8}, n)
        med_d, spread_d = legs_alternating({"decode_rgb_frames16": dec16, "u8_c32_a": dec8, "u8_c32_b": dec8}, n)
        per_n[f"n={n}"] = {
            "stream_shorts_per_frame": {"deep": int(sum(totals) / n), "u8": int(sum(totals8) / n)},
            "encode_ms_per_frame": med_e, "encode_spread_ms": spread_e,
            "decode_ms_per_frame": med_d, "decode_spread_ms": spread_d,
            "encode_run_spread_ms": round(abs(med_e["u8_c32_a"] - med_e["u8_c32_b"]), 4),
            "decode_run_spread_ms": round(abs(med_d["u8_c32_a"] - med_d["u8_c32_b"]), 4),
            "encode_in_kernel_minus_nofuse_ms": round(med_e["encode_rgb_frames16"] - med_e["encode_rgb_frames16_nofuse"], 4),
        }
    results[name] = {"wl": wl, "qs": qs, "max_abs_coefficient_cpu": peak, **per_n}
    deep.close()
    flat.close()
    del f16, f8, s16, s8, o16, o8
    torch.cuda.empty_cache()

print(json.dumps({"gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "bit_depth": bd, "rounds": rounds,
                  "calls_per_round": calls, "results": results}))
