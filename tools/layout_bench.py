#!/usr/bin/env python3
"""Times the pixel-layout kernels on one 8K frame, per layout: picsong_ingest_frames and picsong_emit_frames (HIP events
around `calls` launches, median of the rounds) as ms per frame and as bytes per second -- the bytes the kernel has to read
plus the bytes it has to write -- and beside each, IN THE SAME ROUND, a device-to-device copy_ of the same byte total
(half read, half written): the yardstick is a flat copy, not the kernel's earlier self.  Packed rows (pitch = W * bpp),
256-byte aligned buffers: the vector forms.  Every leg rotates over enough distinct buffers (--pool MB of them, 640 by
default) that no call finds its bytes in the 256 MiB Infinity Cache: the figures are HBM figures.
Then picsong_encode_images on raw grey frames beside picsong_encode_frames on the pre-padded ones, lossless and 9/7, legs
alternating, inputs rotating likewise.  Checks every kernel's output against the host pad / numpy before timing.  One
JSON line.

    python tools/layout_bench.py [--rounds=R] [--calls=C] [--pool=640] [--w=7680] [--h=4320] [--wl=6]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-image-and-video-codec_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import layout_ref as lr
import oracle_lib as orc
import picsong_amd as pa

opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
rounds, calls = int(opts.get("rounds", 7)), int(opts.get("calls", 10))
W, H, wl = int(opts.get("w", 7680)), int(opts.get("h", 4320)), int(opts.get("wl", 6))
pool = int(opts.get("pool", 640)) * 1000 * 1000
assert torch.cuda.is_available(), "no GPU: nothing to time"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def rotating(fn, sets):
    """fn over the next of `sets` at every call."""
    state = [0]

    def call():
        fn(*sets[state[0] % len(sets)])
        state[0] += 1
    return call


def legs_alternating(legs):
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):                                  # the legs alternate: drift hits them alike
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}


planes3 = [orc.gen_frame(W, H, i) for i in range(3)]
layouts = {}
for layout in lr.LAYOUTS:
    rgb = layout != lr.GREY8
    c = pa.Codec(W, H, wl=wl, rgb=rgb)
    nplanes, bpp = lr.PLANES[layout], lr.BPP[layout]
    planes = planes3[:nplanes]
    pitch, ps = W * bpp, W * H
    host = lr.pack(planes, layout, pitch, ps, alpha=0x80)
    d_img = torch.from_numpy(host).cuda()
    img = c.image(d_img, layout, pitch, ps)
    padded = c.ingest_frames(img)
    want = np.concatenate([orc.pad_frame(p).ravel() for p in planes])
    assert np.array_equal(padded.cpu().numpy().ravel(), want), "ingest differs from the host pad"
    d_back = torch.zeros_like(d_img)
    back = c.image(d_back, layout, pitch, ps)
    c.emit_frames(padded, back)
    assert np.array_equal(d_back.cpu().numpy(), lr.pack(planes, layout, pitch, ps, alpha=255)), "emit differs from numpy's interleave"
    # bytes: the image's pixel bytes on one side; on the other the whole padded planes (ingest writes them) or their
    # visible W x H part in whole 16-byte (4-pixel) groups (emit reads those)
    img_bytes = host.size
    grp = 4 if layout >= lr.RGB24 else 16
    ingest_bytes = img_bytes + nplanes * c.P
    emit_bytes = img_bytes + nplanes * H * ((W + grp - 1) // grp * grp)
    K = max(2, -(-pool // ingest_bytes))
    d_imgs = [d_img.clone() for _ in range(K)]
    sets = [(c.image(t, layout, pitch, ps), padded.clone()) for t in d_imgs]
    res = {}
    for name, fn, nbytes in (("ingest", lambda im, pd: c.ingest_frames(im, out=pd), ingest_bytes),
                             ("emit", lambda im, pd: c.emit_frames(pd, im), emit_bytes)):
        pairs = [(torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"))
                 for _ in range(K)]
        med, spread = legs_alternating({"kernel": rotating(fn, sets), "copy": rotating(lambda a, b: b.copy_(a), pairs)})
        res[name] = {"ms": round(med["kernel"], 4), "spread_ms": spread["kernel"], "bytes": nbytes,
                     "gbytes_per_s": round(nbytes / med["kernel"] / 1e6, 1),
                     "copy_ms": round(med["copy"], 4), "copy_spread_ms": spread["copy"],
                     "copy_gbytes_per_s": round(2 * (nbytes // 2) / med["copy"] / 1e6, 1),
                     "of_copy": round(med["copy"] / med["kernel"], 3)}
        del pairs
    res["buffers_rotated"] = K
    layouts[lr.NAMES[layout]] = res
    c.close()
    del d_img, d_back, padded, d_imgs, sets
    torch.cuda.empty_cache()

# ---- picsong_encode_images on the raw frame beside picsong_encode_frames on the pre-padded one
encode = {}
for lossy in (False, True):
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=0.5 if lossy else 1.0, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless"))
    K = max(2, -(-pool // (W * H + c.P)))
    raws = [torch.from_numpy(orc.gen_frame(W, H, 20 + i % 4)).cuda() for i in range(K)]       # (distinct buffers, four contents)
    pres = [(torch.from_numpy(orc.pad_frame(r.cpu().numpy())).cuda().view(1, -1),) for r in raws]
    imgs = [(c.image(r, lr.GREY8),) for r in raws]
    out = torch.zeros((1, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    s = c._stream()

    def images(img):
        pa._check(c.L.picsong_encode_images(c.h, 1, img, 0, 0, c._p(out), out.stride(0), s))

    def frames(pre):
        c.encode_frames_async(pre, out, 0)

    images(*imgs[0])
    t = c.last_totals(1)[0]
    a = out[0, :t].clone()
    frames(*pres[0])
    assert c.last_totals(1)[0] == t and torch.equal(a, out[0, :t]), "encode_images differs from encode_frames on the padded frame"
    med, spread = legs_alternating({"encode_images": rotating(images, imgs), "encode_frames_prepadded": rotating(frames, pres)})
    encode["9/7" if lossy else "5/3"] = {"ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": spread,
                                         "ingest_share": round(1.0 - med["encode_frames_prepadded"] / med["encode_images"], 4)}
    c.close()
    del raws, pres, imgs

print(json.dumps({"gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "wl": wl, "rounds": rounds, "calls_per_round": calls,
                  "pool_mbytes": pool // 1000000, "layouts": layouts, "encode": encode}))
