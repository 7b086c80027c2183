#!/usr/bin/env python3
"""Times the proxies of deep frames -- RGBA64 thumbnails of 4K 12-bit RGB streams at 1/4 and 1/8 size, a 512 x 512 RGBA64
window of them at full size, and 8K 12-bit grey frames at 1/4 size -- `smooth` content, 5/3 (wl 5) and 9/7 (wl 5, qs 0.25: deep_bench.py found qs 0.5 out of the coders' range on this content at 8K),
as ms per frame, n = 1, 4 and 21 frames (grey: 1 and 3):
  (f) the full decode of the same n, picsong_decode_rgb_frames16 (picsong_decode_frames16) -- what a caller had to run before
      these calls existed, measured TWICE per round (legs f1, f2), so the run carries its own spread: max - min over all of
      (f)'s values;
  (p) one picsong_decode_rgb_images_reduced / picsong_decode_rgb_images_window call of n into RGBA64
      (grey: picsong_decode_frames16_reduced).
HIP events bracket `calls` calls, the legs alternate within a round, the median of the rounds is reported.  The streams
rotate over `groups` distinct buffers.  Before timing, the proxy's samples are checked against the planar proxy call's.
Recorded, not gated: is the proxy call faster than the full decode by more than the spread?  One JSON object, printed and
written to --out.

    python tools/deep_proxy_bench.py [--rounds=5] [--modes=53,97] [--n=1,4,21] [--grey_n=1,3] [--out=profiles/deep_proxy_bench.json]"""
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
modes = [m for m in opts.get("modes", "53,97").split(",") if m]
ns = [int(x) for x in opts.get("n", "1,4,21").split(",")]
grey_ns = [int(x) for x in opts.get("grey_n", "1,3").split(",")]
out_path = opts.get("out", os.path.join(ROOT, "profiles", "deep_proxy_bench.json"))
BD, WL, WIN, GROUPS, DISTINCT = 12, 5, 512, 3, 4
MX = (1 << BD) - 1
assert torch.cuda.is_available(), "no GPU: nothing to time"


def smooth(w, h, seed):
    """deep_ref's `smooth` content at any size: a slow wave at 45 % of the range with noise of 1/32 of it"""
    rng = np.random.default_rng(seed)
    a = max(1, MX >> 5)
    y, x = np.mgrid[0:h, 0:w]
    x, y = x + 11 * seed, y + 7 * seed
    v = np.clip((MX * (0.5 + 0.45 * np.sin(x / 17.0) * np.cos(y / 23.0))).astype(np.int64) + rng.integers(-a, a + 1, (h, w)), 0, MX)
    return v.astype(np.uint16)


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_legs(legs, calls, frames_per_call):
    for fn in legs.values():                                 # warm-up: code objects, the context's buffers
        fn(0)
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(timed(fn, calls) / (calls * frames_per_call))
    return out


def summary(r):
    full = r["f1"] + r["f2"]
    f, p = statistics.median(full), statistics.median(r["p"])
    spread = max(full) - min(full)
    return {"full_ms": round(f, 4), "full_legs_ms": [round(statistics.median(r["f1"]), 4), round(statistics.median(r["f2"]), 4)],
            "spread_ms": round(spread, 4), "proxy_ms": round(p, 4), "proxy_range_ms": [round(min(r["p"]), 4), round(max(r["p"]), 4)],
            "proxy_over_full": round(p / f, 4), "faster_by_more_than_the_spread": bool(f - p > spread)}


def setup(W, H, mode, rgb, nmax):
    """one context, nmax frames' streams in GROUPS rotating buffers, DISTINCT frames coded once"""
    lossy = mode == "97"
    qs = 0.25 if lossy else 1.0
    c = pa.Codec(W, H, wl=WL, lossy=lossy, qs=qs, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless"), bit_depth=BD,
                 is_rgb=rgb)
    ms = c.max_stream_shorts()
    comps = 3 if rgb else 1
    coded = []
    for f in range(DISTINCT):
        planes = [dev16(pa.pad_frame16(smooth(W, H, comps * f + k), c.aw, c.ah)).reshape(1, c.ah, c.aw) for k in range(comps)]
        got = c.encode_rgb_frames16(*planes, header_mask=0) if rgb else c.encode_frames16(planes[0], first_iter=1)
        coded.append([s.clone() for s in got])
        del planes
    assert c.range_flag() == 0, "the content left the coder's range"
    streams = torch.zeros((GROUPS, comps * nmax, ms), dtype=torch.int16, device="cuda")
    for g in range(GROUPS):
        for f in range(nmax):
            for k in range(comps):
                s = coded[(g * nmax + f) % DISTINCT][k]
                streams[g, comps * f + k, :s.numel()] = s
    return c, streams


def rgb_case(c, streams, n, r, window):
    """r > 0: the visible thumbnail; window: (x, y, w, h) at r = 0"""
    ms = c.max_stream_shorts()
    L, h, s, vp = c.L, c.h, c._stream(), C.c_void_p
    if window:
        x, y, w, hh = window
        vw, vh = w, hh
    else:
        vw, vh = c.reduced_dims(r)[:2]
        x = y = 0
    full = torch.empty((n, 3, c.ah, c.aw), dtype=torch.int16, device="cuda")
    rgba = torch.zeros((n, vh, vw, 4), dtype=torch.int16, device="cuda")
    img = c.image(rgba, pa.LAYOUT_RGBA64, 8 * vw)
    fs = vh * vw * 8

    def at(t, *idx):
        return vp(t[idx].data_ptr())

    def full_call(i):
        pa._check(L.picsong_decode_rgb_frames16(h, n, at(streams, i % GROUPS, 0), ms, at(full, 0, 0), at(full, 0, 1), at(full, 0, 2),
                                                6 * c.P, s))

    def proxy_call(i):
        if window:
            pa._check(L.picsong_decode_rgb_images_window(h, n, at(streams, i % GROUPS, 0), ms, 0, x, y, vw, vh, C.byref(img), fs, s))
        else:
            pa._check(L.picsong_decode_rgb_images_reduced(h, n, at(streams, i % GROUPS, 0), ms, r, C.byref(img), fs, s))

    # ---- the image call's samples are the planar window call's
    proxy_call(0)
    planes = c.decode_rgb_frames16_window(streams[0, :3 * n], x, y, vw, vh, r=r)
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(rgba[..., k], planes[k]), "the image call's samples differ from the planar call's"
    assert bool((rgba[..., 3] == MX).all()), "alpha = mx"
    if window:                                               # ... and, at full size, the full decode's
        full_call(0)
        torch.cuda.synchronize()
        assert torch.equal(full[:, 0, y:y + vh, x:x + vw], planes[0]), "the window differs from the full decode's rectangle"

    calls = max(4, 64 // n)
    res = summary(run_legs({"f1": full_call, "p": proxy_call, "f2": full_call}, calls, n))
    res.update(calls_per_round=calls, samples=[vw, vh])
    return res


def grey_case(c, streams, n, r):
    ms = c.max_stream_shorts()
    L, h, s, vp = c.L, c.h, c._stream(), C.c_void_p
    paw, pah = c.aw >> r, c.ah >> r
    full = torch.empty((n, c.ah, c.aw), dtype=torch.int16, device="cuda")
    small = torch.zeros((n, pah, paw), dtype=torch.int16, device="cuda")

    def full_call(i):
        pa._check(L.picsong_decode_frames16(h, n, vp(streams[i % GROUPS].data_ptr()), ms, vp(full.data_ptr()), 2 * c.P, s))

    def proxy_call(i):
        pa._check(L.picsong_decode_frames16_reduced(h, n, vp(streams[i % GROUPS].data_ptr()), ms, r, vp(small.data_ptr()), 2 * paw * pah, s))

    proxy_call(0)
    win = c.decode_frames16_window(streams[0, :n], 0, 0, paw, pah, r=r)
    torch.cuda.synchronize()
    assert torch.equal(small, win), "the reduced call's samples differ from the whole-image window's"
    calls = max(4, 64 // n)
    res = summary(run_legs({"f1": full_call, "p": proxy_call, "f2": full_call}, calls, n))
    res.update(calls_per_round=calls, samples=[paw, pah])
    return res


results = {}
for mode in modes:
    name = "9/7" if mode == "97" else "5/3"
    W, H = 3840, 2160
    c, streams = setup(W, H, mode, True, max(ns))
    what = [("r=2", 2, None), ("r=3", 3, None), (f"window{WIN}", 0, ((W - WIN) // 2 + 1, (H - WIN) // 2 + 3, WIN, WIN))]
    for label, r, window in what:
        for n in ns:
            key = f"4k-rgb/{name}/{label}/n={n}"
            results[key] = x = rgb_case(c, streams, n, r, window)
            print(key, x["full_ms"], x["proxy_ms"], x["spread_ms"], file=sys.stderr, flush=True)
    c.close()
    del streams
    torch.cuda.empty_cache()
    c, streams = setup(7680, 4320, mode, False, max(grey_ns))
    for n in grey_ns:
        key = f"8k-grey/{name}/r=2/n={n}"
        results[key] = x = grey_case(c, streams, n, 2)
        print(key, x["full_ms"], x["proxy_ms"], x["spread_ms"], file=sys.stderr, flush=True)
    c.close()
    del streams
    torch.cuda.empty_cache()

doc = json.dumps({"gpu": torch.cuda.get_device_name(0), "rounds": rounds, "groups_rotated": GROUPS, "bit_depth": BD, "wl": WL, "qs_97": 0.25,
                  "content": "smooth", "results": results})
print(doc)
with open(out_path, "w") as f:
    f.write(doc + "\n")
