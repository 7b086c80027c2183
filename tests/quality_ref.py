"""Reference model of the quality calls (picsong_encode_frame_quality and its mirrors).  TEST INFRASTRUCTURE ONLY.

The grid is the rate calls' (rate_ref.grid).  bisect(): the procedure that DEFINES the result (SSE against j is not
monotone, so "the coarsest j that meets the limit" is not defined without an exhaustive scan).  The SSE functions are
defined through the CPU oracle's decode of its own encode, never through the code under test; the coder-free route the
library's probes take (quantise, truncate, synthesise, clamp) is asserted equal to it at every evaluation."""
import collections

import numpy as np

import oracle_lib as orc
import rate_ref as rr

q = rr.q
grid = rr.grid


def limit(psnr_db, samples):
    """picsong_psnr_to_sse."""
    return int(65025.0 * samples / 10 ** (psnr_db / 10))


def sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


Result = collections.namedtuple("Result", "j sse prev_j prev_sse probes")
Result.__doc__ = """j: the result (None: nothing meets the limit); sse: sse(j); prev_j / prev_sse: G'[hi - 1] and its SSE
where the procedure probed it (None at the bottom of the range); probes: [(j, sse)] in the procedure's order."""


def bisect(sse_fn, max_sse, j_min=0, j_max=0):
    g = grid(j_min, j_max)
    assert g, "the range holds no grid entry"
    seen = {}
    probes = []
    lo, hi = -1, len(g)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if g[mid] not in seen:
            seen[g[mid]] = int(sse_fn(g[mid]))
        s = seen[g[mid]]
        probes.append((g[mid], s))
        if s <= max_sse:
            hi = mid
        else:
            lo = mid
    prev = g[hi - 1] if hi >= 1 else None
    return Result(g[hi] if hi < len(g) else None, seen[g[hi]] if hi < len(g) else None, prev,
                  seen.get(prev) if prev is not None else None, probes)


def rounds3(sse_fn, max_sse, j_min=0, j_max=0):
    """The K = 3 round of the quality calls: rate_ref.rounds3 with a pass moving hi."""
    return rr.rounds3(sse_fn, max_sse, j_min, j_max, pass_moves_lo=False)


def coder_free_frame(img, wl, j):
    """The decoder's pixels without the coder: the oracle's fused transform at q(j), truncated toward zero, its
    synthesis at q(j), level shift and clamp; the visible part."""
    H, W = img.shape
    pad = orc.pad_frame(img)
    AH, AW = pad.shape
    coef = np.trunc(orc.dwt_forward(orc.level_shift_fwd(pad, True), wl, q(j))[:AW * AH]).astype(np.int32).reshape(AH, AW)
    out, extra = orc.dwt_inverse(coef, wl, True, q(j))
    return orc.level_shift_inv(out[extra:]).reshape(AH, AW)[:H, :W].astype(np.uint8)


def frames_sse_list(imgs, wl, lut, j, k=0.0):
    """The per-frame SSE of grey frames at q(j): the oracle's decode of its encode against the input."""
    out = []
    for img in imgs:
        H, W = img.shape
        dec = orc.decode_frame(orc.encode_frame(img, wl, True, q(j), lut, k=k), W, H, wl, True, q(j), lut, k=k)
        s = sse(img, dec)
        assert s == sse(img, coder_free_frame(img, wl, j)), ("the coder-free route differs", j)
        out.append(s)
    return out


def frames_sse_fn(imgs, wl, lut, k=0.0):
    return lambda j: sum(frames_sse_list(imgs, wl, lut, j, k))


def rgb_sse_list(planes, wl, luts, j):
    """The SSE of the R, G and B planes of an RGB frame at q(j): per-component streams (rate_ref.rgb_streams), the oracle's
    decode_plane and inverse ICT."""
    H, W = planes[0].shape
    comps = rr.rgb_components(*planes)
    AH, AW = comps[0].shape
    streams = rr.rgb_streams(comps, wl, j, luts)
    dec = orc.rgb_inverse(*[orc.decode_plane(streams[c], AW, AH, wl, True, q(j), luts[c]) for c in range(3)])
    free = []
    for c in range(3):
        coef = np.trunc(orc.dwt_forward(comps[c], wl, q(j))[:AW * AH]).astype(np.int32).reshape(AH, AW)
        out, extra = orc.dwt_inverse(coef, wl, True, q(j))
        free.append(out[extra:].reshape(AH, AW))
    free = orc.rgb_inverse(*free)
    out = [sse(planes[c], dec[c].reshape(AH, AW)[:H, :W]) for c in range(3)]
    assert out == [sse(planes[c], free[c].reshape(AH, AW)[:H, :W]) for c in range(3)], ("the coder-free route differs", j)
    return out


def rgb_sse_fn(planes, wl, luts):
    return lambda j: sum(rgb_sse_list(planes, wl, luts, j))


# ---- the cases recorded on the oracle when the feature was specified (limit = limit(dB, samples)):
# name -> (W, H, wl, frames, rgb, dB, j_min, j_max, limit, j, per-frame / per-plane sse(j), previous grid value, its sse)
CASES = {
    "200x136-wl3-40dB": (200, 136, 3, 1, False, 40, 0, 0, 176868, 1865, [176463], 1864, 176935),
    "320x192-wl5-30dB": (320, 192, 5, 1, False, 30, 0, 0, 3995136, 77, [3950171], 76, 4029937),
    "700x500-wl5-40dB": (700, 500, 5, 1, False, 40, 0, 0, 2275875, 1873, [2274469], 1872, 2276625),
    "700x500-wl6-50dB": (700, 500, 6, 1, False, 50, 0, 0, 227587, 5190, [227536], 5189, 227668),
    "700x500-wl6-40dB-sub": (700, 500, 6, 1, False, 40, 1000, 3000, 2275875, 1873, [2274694], 1872, 2277067),
    "3x320x192-wl5-40dB": (320, 192, 5, 3, False, 40, 0, 0, 1198540, 1874, [398534, 400970, 399018], 1873, 1199911),
    "rgb-200x136-wl3-40dB": (200, 136, 3, 1, True, 40, 0, 0, 530604, 3128, [178524, 105882, 246045], 3127, 531445),
}
_cache = {}


def case_inputs(name):
    """(images or the R, G, B planes, table(s)) of a case."""
    W, H, wl, frames, rgb = CASES[name][:5]
    if rgb:
        return [orc.gen_frame(W, H, 60 + c) for c in range(3)], [orc.lut_for_component(True, wl, c) for c in range(3)]
    return [orc.gen_frame(W, H, f) for f in range(frames)], orc.lut_for(True, wl)


def case_sse_fn(name):
    W, H, wl, frames, rgb = CASES[name][:5]
    imgs, lut = case_inputs(name)
    return rgb_sse_fn(imgs, wl, lut) if rgb else frames_sse_fn(imgs, wl, lut)


def case_result(name, max_sse=None, j_min=None, j_max=None):
    """The procedure's Result for a case (its own limit and range unless given), computed once."""
    c = CASES[name]
    key = (name, c[8] if max_sse is None else max_sse, c[6] if j_min is None else j_min, c[7] if j_max is None else j_max)
    if key not in _cache:
        if name not in _cache:
            fn, seen = case_sse_fn(name), {}
            _cache[name] = lambda j: seen[j] if j in seen else seen.setdefault(j, fn(j))
        _cache[key] = bisect(_cache[name], *key[1:])
    return _cache[key]
