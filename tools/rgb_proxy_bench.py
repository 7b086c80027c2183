#!/usr/bin/env python3
"""Times colour proxies -- RGBA thumbnails of 4K and 8K RGB streams at 1/4 and 1/8 size, and a 512 x 512 RGBA window at
full size -- 5/3 (wl 5) and 9/7 (wl 5, qs 0.5), as ms per frame, n = 1, 4, 8 and 21 frames:
  (a) the parent commit's way: a loop of n picsong_decode_rgb_frame_reduced (picsong_decode_rgb_frame_window) calls, each
      followed by the caller's own planar-to-RGBA step, a torch.stack of the visible pixels and a constant alpha plane
      -- measured TWICE per round (legs a1, a2), so the run carries its own spread: max - min over all of (a)'s values;
  (b) one picsong_decode_rgb_images_reduced (picsong_decode_rgb_images_window) call of n into RGBA32;
  (p) the loop of (a) without the RGBA step, and (q) one picsong_decode_rgb_frames_reduced (_window) call of n into planar
      planes: the decode alone, single-frame against batched.
HIP events bracket `calls` calls, the legs alternate within a round, the median of the rounds is reported.  The streams
rotate over `groups` distinct buffers.  Before timing, (b)'s pixels are checked against (a)'s.
Recorded, not gated: n = 1, does (b) cost no more than (a) plus its spread, and (q) no more than (p) plus it?  One JSON object, printed and written
to --out.

    python tools/rgb_proxy_bench.py [--rounds=5] [--sizes=4k,8k] [--modes=53,97] [--n=1,4,8,21] [--reduce=2,3]
                                    [--out=profiles/rgb_proxy_bench.json]"""
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
sizes = [s for s in opts.get("sizes", "4k,8k").split(",") if s]
modes = [m for m in opts.get("modes", "53,97").split(",") if m]
ns = [int(x) for x in opts.get("n", "1,4,8,21").split(",")]
reduces = [int(x) for x in opts.get("reduce", "2,3").split(",")]
out_path = opts.get("out", os.path.join(ROOT, "profiles", "rgb_proxy_bench.json"))
DIMS = {"4k": (3840, 2160), "8k": (7680, 4320)}
WIN = 512
GROUPS = 3
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


def summary(r, n):
    single, plain = r["a1"] + r["a2"], r["p"]
    a, b, p, q = (statistics.median(x) for x in (single, r["b"], plain, r["q"]))
    return {"loop_rgba_ms": round(a, 4), "loop_legs_ms": [round(statistics.median(r["a1"]), 4), round(statistics.median(r["a2"]), 4)],
            "spread_ms": round(max(single) - min(single), 4), "images_call_ms": round(b, 4),
            "images_call_range_ms": [round(min(r["b"]), 4), round(max(r["b"]), 4)], "images_over_loop": round(b / a, 4),
            "loop_planar_ms": round(p, 4), "frames_call_ms": round(q, 4), "frames_over_loop": round(q / p, 4)}


def setup(size, mode):
    """one context, 21 frames' streams in GROUPS rotating buffers"""
    W, H = DIMS[size]
    lossy = mode == "97"
    wl, qs = 5, (0.5 if lossy else 1.0)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless"), rgb=True)
    ms = c.max_stream_shorts()
    nmax = max(ns)
    coded = []
    for f in range(4):                                       # four distinct frames, coded once
        planes = [torch.from_numpy(orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + k))).cuda() for k in range(3)]
        coded.append([s.clone() for s in c.encode_rgb_frame(*planes, header_mask=0)])
        del planes
    streams = torch.zeros((GROUPS, 3 * nmax, ms), dtype=torch.int16, device="cuda")
    for g in range(GROUPS):
        for f in range(nmax):
            for k in range(3):
                s = coded[(g * nmax + f) % 4][k]
                streams[g, 3 * f + k, :s.numel()] = s
    return c, streams, wl


def case(c, streams, n, r, window):
    """r > 0: the reduced image; window: (x, y, w, h) at r = 0"""
    ms = c.max_stream_shorts()
    L, h, s, vp = c.L, c.h, c._stream(), C.c_void_p
    if window:
        x, y, w, hh = window
        pw, ph, vw, vh = w, hh, w, hh
    else:
        vw, vh, pw, ph = c.reduced_dims(r)[:4]
    planes = torch.empty((n, 3, ph, pw), dtype=torch.uint8, device="cuda")
    alpha = torch.full((vh, vw), 255, dtype=torch.uint8, device="cuda")
    rgba_loop = torch.zeros((n, vh, vw, 4), dtype=torch.uint8, device="cuda")
    rgba_call = torch.zeros((n, vh, vw, 4), dtype=torch.uint8, device="cuda")
    img = c.image(rgba_call, pa.LAYOUT_RGBA32, 4 * vw)
    fs = vh * vw * 4

    def at(t, *idx):
        return vp(t[idx].data_ptr())

    def single(g, f):
        if window:
            pa._check(L.picsong_decode_rgb_frame_window(h, at(streams, g, 3 * f), ms, 0, x, y, w, hh, at(planes, f, 0), at(planes, f, 1),
                                                        at(planes, f, 2), pw, s))
        else:
            pa._check(L.picsong_decode_rgb_frame_reduced(h, at(streams, g, 3 * f), ms, r, at(planes, f, 0), at(planes, f, 1), at(planes, f, 2), s))

    def loop_rgba(i):
        g = i % GROUPS
        for f in range(n):
            single(g, f)
            torch.stack((planes[f, 0, :vh, :vw], planes[f, 1, :vh, :vw], planes[f, 2, :vh, :vw], alpha), dim=-1, out=rgba_loop[f])

    def loop_planar(i):
        g = i % GROUPS
        for f in range(n):
            single(g, f)

    def images_call(i):
        g = i % GROUPS
        if window:
            pa._check(L.picsong_decode_rgb_images_window(h, n, at(streams, g, 0), ms, 0, x, y, w, hh, C.byref(img), fs, s))
        else:
            pa._check(L.picsong_decode_rgb_images_reduced(h, n, at(streams, g, 0), ms, r, C.byref(img), fs, s))

    def frames_call(i):
        g = i % GROUPS
        if window:
            pa._check(L.picsong_decode_rgb_frames_window(h, n, at(streams, g, 0), ms, 0, x, y, w, hh, at(planes, 0, 0), at(planes, 0, 1),
                                                         at(planes, 0, 2), pw, 3 * pw * ph, s))
        else:
            pa._check(L.picsong_decode_rgb_frames_reduced(h, n, at(streams, g, 0), ms, r, at(planes, 0, 0), at(planes, 0, 1), at(planes, 0, 2),
                                                          3 * pw * ph, s))

    # ---- the results must not differ
    loop_rgba(0)
    images_call(0)
    torch.cuda.synchronize()
    assert torch.equal(rgba_loop, rgba_call), "the image call's pixels differ from the loop's"
    want = planes.clone()
    planes.zero_()
    frames_call(0)
    torch.cuda.synchronize()
    assert torch.equal(planes, want), "the frames call's planes differ from the loop's"

    calls = max(4, 64 // n)
    res = summary(run_legs({"a1": loop_rgba, "b": images_call, "p": loop_planar, "q": frames_call, "a2": loop_rgba}, calls, n), n)
    res.update(calls_per_round=calls, pixels=[vw, vh])
    return res


results, notes = {}, []
for size in sizes:
    for mode in modes:
        c, streams, wl = setup(size, mode)
        W, H = DIMS[size]
        what = [(f"r={r}", r, None) for r in reduces] + [(f"window{WIN}", 0, ((W - WIN) // 2 + 1, (H - WIN) // 2 + 3, WIN, WIN))]
        for name, r, window in what:
            for n in ns:
                key = f"{size}/{'9/7' if mode == '97' else '5/3'}/{name}/n={n}"
                results[key] = x = case(c, streams, n, r, window)
                print(key, x["loop_rgba_ms"], x["images_call_ms"], file=sys.stderr, flush=True)
                if n == 1:
                    notes.append({"case": key, "what": "n = 1: the image call costs no more than the loop with its RGBA step, plus the loop's spread",
                                  "holds": x["images_call_ms"] - x["loop_rgba_ms"] <= x["spread_ms"]})
                    notes.append({"case": key, "what": "n = 1: the frames call costs no more than the single-frame call, plus the loop's spread",
                                  "holds": x["frames_call_ms"] - x["loop_planar_ms"] <= x["spread_ms"]})
        c.close()
        del streams
        torch.cuda.empty_cache()

doc = json.dumps({"gpu": torch.cuda.get_device_name(0), "rounds": rounds, "groups_rotated": GROUPS, "wl": 5, "qs_97": 0.5,
                  "results": results, "recorded_not_gated": notes})
print(doc)
with open(out_path, "w") as f:
    f.write(doc + "\n")
