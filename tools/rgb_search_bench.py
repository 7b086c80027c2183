#!/usr/bin/env python3
"""Times the quantiser search over n RGB frames (picsong_encode_rgb_frames_rate / _quality) and the tail of an RGB quality
probe, 9/7, wl 5:

  tail   per size (4K, 8K), one frame: a probe's stage times through picsong_profile_begin / picsong_profile_read --
         {quantise, synthesis, SSE} -- of picsong_encode_rgb_frame_quality over a one-entry range (one probe a call).
         Compared is synthesis + SSE SUMMED: the unfused tail has the colour transform in the second stage, the fused one
         in the third.  Legs: the parent commit's library (--parent=<its libpicsong_hip.so>) TWICE (p1, p2: the run's own
         spread is max - min over all of their values), this library with rgb_sse_kernel (fused) and this library with
         PICSONG_RGB_SSE_FUSED=0 (unfused); the legs alternate within a round; the median over the rounds is reported.
         Without --parent the two spread legs are this library's unfused tail (the parent's launches).
  calls  4K, n = 1, 4, 7: ms per call (host clock around the synchronous call) of the n-frame rate call at 1.0 bpp and of
         the n-frame quality call at 40 dB, beside a loop of n single-frame calls (measured twice, for the spread), and a
         probe's stage times of the n-frame quality call.

Before timing, the fused and the unfused tail are checked to give the same j, sums and streams.  One JSON object, printed and
written to --out.

    python tools/rgb_search_bench.py [--parent=build/parent/libpicsong_hip.so] [--rounds=5] [--sizes=4k,8k] [--n=1,4,7]
                                     [--out=profiles/rgb_search_bench.json]"""
import ctypes as C
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
rounds = int(opts.get("rounds", 5))
sizes = [s for s in opts.get("sizes", "4k,8k").split(",") if s]
ns = [int(x) for x in opts.get("n", "1,4,7").split(",") if x]
parent_so = opts.get("parent", "")
out_path = opts.get("out", os.path.join(ROOT, "profiles", "rgb_search_bench.json"))
DIMS = {"4k": (3840, 2160), "8k": (7680, 4320), "tiny": (200, 136)}
WL, PROBE_J, CALLS = 5, 5000, 8
LUTS = os.path.join(orc.LUT_DIR, "n1_lossy")
assert torch.cuda.is_available(), "no GPU: nothing to time"

pa.load()                                                   # this tree's library
if parent_so:                                               # ... and the parent's beside it: contexts keep the one they were made with
    this_lib, pa._lib, pa.SO_PATH = pa._lib, None, os.path.abspath(parent_so)
    parent_lib = pa.load()
    pa._lib = this_lib
else:
    parent_lib = None


def codec(W, H, lib=None):
    keep = pa._lib
    if lib is not None:
        pa._lib = lib
    try:
        return pa.Codec(W, H, wl=WL, lossy=True, qs=0.5, lut_folder=LUTS, rgb=True)
    finally:
        pa._lib = keep


def planes(W, H, n):
    """three uint8 [n, AH, AW] device arrays"""
    return [torch.from_numpy(np.stack([orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + c)) for f in range(n)])).cuda() for c in range(3)]


def fused_env(on):
    if on:
        os.environ.pop("PICSONG_RGB_SSE_FUSED", None)
    else:
        os.environ["PICSONG_RGB_SSE_FUSED"] = "0"


def med(x):
    return round(statistics.median(x), 4)


# ---- the probe's tail, one frame ----------------------------------------------------------------------------------------
def tail(size):
    W, H = DIMS[size]
    rgb = planes(W, H, 1)
    mine, theirs = codec(W, H), codec(W, H, parent_lib) if parent_lib else None
    out = torch.empty((3, mine.max_stream_shorts()), dtype=torch.int16, device="cuda")

    def probe_stages(c, fused):
        """CALLS single-probe quality calls; [quantise, synthesis, sse] ms, the median over the calls' probes"""
        fused_env(fused)
        c.profile_begin(CALLS)
        j, t, e = C.c_int(), (C.c_int * 3)(), (C.c_uint64 * 3)()
        for _ in range(CALLS):
            pa._check(c.L.picsong_encode_rgb_frame_quality(c.h, c._p(rgb[0]), c._p(rgb[1]), c._p(rgb[2]), 1, 1 << 60, PROBE_J, PROBE_J,
                                                           c._p(out), out.stride(0), c._stream(), C.byref(j), t, e))
        ms = c.profile_read(CALLS)
        fused_env(True)
        assert ms.shape[0] == CALLS and j.value == PROBE_J
        return [float(np.median(ms[:, k])) for k in range(3)], (list(t), [int(v) for v in e], out.clone())

    old = theirs if theirs else mine
    legs = {"p1": (old, False), "fused": (mine, True), "unfused": (mine, False), "p2": (old, False)}
    res = {k: probe_stages(c, f)[1] for k, (c, f) in legs.items()}          # warm-up, and the results must not differ
    for k in ("unfused", "p1"):
        assert res["fused"][0] == res[k][0] and res["fused"][1] == res[k][1] and torch.equal(res["fused"][2], res[k][2]), k
    stages = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (c, f) in legs.items():
            stages[k].append(probe_stages(c, f)[0])
    doc = {}
    for k, v in stages.items():
        doc[k] = {"quantise_ms": med([x[0] for x in v]), "synthesis_ms": med([x[1] for x in v]), "sse_ms": med([x[2] for x in v]),
                  "synthesis_plus_sse_ms": med([x[1] + x[2] for x in v])}
    par = [x[1] + x[2] for k in ("p1", "p2") for x in stages[k]]
    doc["parent_is"] = "the parent commit's library" if theirs else "this library, PICSONG_RGB_SSE_FUSED=0"
    doc["spread_ms"] = round(max(par) - min(par), 4)
    doc["parent_ms"] = med(par)
    doc["fused_minus_parent_ms"] = round(doc["fused"]["synthesis_plus_sse_ms"] - doc["parent_ms"], 4)
    doc["fused_not_slower_than_parent_plus_spread"] = doc["fused_minus_parent_ms"] <= doc["spread_ms"]
    doc["bytes_moved_model"] = {"fused": 15 * mine.P, "unfused": 21 * mine.P}
    mine.close()
    if theirs:
        theirs.close()
    return doc


# ---- the calls, 4K ------------------------------------------------------------------------------------------------------
def calls(size, n):
    W, H = DIMS[size]
    rgb = planes(W, H, n)
    c = codec(W, H)
    target, limit = int(1.0 * W * H / 16), pa.psnr_to_sse(40.0, 3 * W * H)
    one = [[rgb[k][f] for k in range(3)] for f in range(n)]

    def loop_rate():
        return [c.encode_rgb_frame_rate(*one[f], target)[0] for f in range(n)]

    def frames_rate():
        return c.encode_rgb_frames_rate(*rgb, target * n)[0]

    def loop_quality():
        return [c.encode_rgb_frame_quality(*one[f], limit)[0] for f in range(n)]

    def frames_quality():
        return c.encode_rgb_frames_quality(*rgb, limit * n)[0]

    legs = {"loop_rate_1": loop_rate, "frames_rate": frames_rate, "loop_quality_1": loop_quality, "frames_quality": frames_quality,
            "loop_rate_2": loop_rate, "loop_quality_2": loop_quality}
    chosen = {k: fn() for k, fn in legs.items()}           # warm-up: code objects, the context's buffers
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    doc = {"j": {k: chosen[k] for k in ("loop_rate_1", "frames_rate", "loop_quality_1", "frames_quality")}}
    for kind in ("rate", "quality"):
        loop = ms[f"loop_{kind}_1"] + ms[f"loop_{kind}_2"]
        doc[kind] = {"loop_of_single_frame_calls_ms": med(loop), "loop_spread_ms": round(max(loop) - min(loop), 4),
                     "frames_call_ms": med(ms[f"frames_{kind}"]),
                     "frames_call_range_ms": [round(min(ms[f"frames_{kind}"]), 4), round(max(ms[f"frames_{kind}"]), 4)]}
    # a probe's stages of the n-frame quality call, both tails
    for name, fused in (("fused", True), ("unfused", False)):
        fused_env(fused)
        c.profile_begin(64)
        frames_quality()
        st = c.profile_read(64)
        fused_env(True)
        doc[f"probe_stages_{name}"] = {"probes": int(st.shape[0]), "quantise_ms": med(st[:, 0].tolist()), "synthesis_ms": med(st[:, 1].tolist()),
                                       "sse_ms": med(st[:, 2].tolist()), "synthesis_plus_sse_ms": med((st[:, 1] + st[:, 2]).tolist())}
    c.close()
    return doc


results = {"tail": {}, "calls": {}}
for size in sizes:
    results["tail"][size] = tail(size)
    print("tail", size, json.dumps(results["tail"][size]), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
for n in ns:
    size = "4k" if "4k" in sizes else sizes[0]
    results["calls"][f"{size}/n={n}"] = calls(size, n)
    print("calls", size, n, json.dumps(results["calls"][f"{size}/n={n}"]), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()

doc = json.dumps({"gpu": torch.cuda.get_device_name(0), "rounds": rounds, "wl": WL, "probe_j": PROBE_J, "calls_per_tail_leg": CALLS,
                  "parent_library": bool(parent_lib), "results": results})
print(doc)
with open(out_path, "w") as f:
    f.write(doc + "\n")
