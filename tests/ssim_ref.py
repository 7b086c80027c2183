"""Reference model of the SSIM calls (picsong_frames_dssim, picsong_encode_frame_ssim and its mirrors).  TEST
INFRASTRUCTURE ONLY.

The measure is x264 / ffmpeg's integer 8 x 8 SSIM as include/picsong_hip.h defines it: windows of 8 x 8 samples at the
origins (4 x, 4 y) over the visible W x H part, exact integer sums per window, three IEEE double operations and a floor
to 24 fractional bits; the DSSIM sum is windows * 2^24 - sum q.  numpy's float64 arithmetic is IEEE double, each
operation rounded once, so this model is the definition bit for bit.

The grid and the procedure are the quality calls' (quality_ref.bisect, quality_ref.rounds3).  dssim(j) is defined through
the CPU oracle's decode of its own encode, never through the code under test; the coder-free route the library's probes
take is asserted equal to it at every evaluation."""
import math

import numpy as np

import oracle_lib as orc
import quality_ref as qr
import rate_ref as rr

q = rr.q
grid = rr.grid
bisect = qr.bisect
rounds3 = qr.rounds3
C1, C2 = 416, 235963
ONE = 1 << 24
X264_K1 = (0.01 * 255) ** 2 / 64


def windows(W, H):
    """picsong_ssim_windows."""
    assert W >= 8 and H >= 8
    return ((W - 8) // 4 + 1) * ((H - 8) // 4 + 1)


def ssim_to_dssim(ssim, n_windows):
    """picsong_ssim_to_dssim: floor(((1 - ssim) * windows) * 2^24), double arithmetic in that order."""
    return int(math.floor(((1.0 - float(ssim)) * float(n_windows)) * 16777216.0))


def dssim_to_ssim(dssim, n_windows):
    """picsong_dssim_to_ssim."""
    return 1.0 - float(dssim) / (float(n_windows) * 16777216.0)


def window_sums(a, b):
    """(s1, s2, ss, s12): int64 [ny, nx] arrays of the windows' sums over the visible planes a, b (uint8 [H, W])."""
    H, W = a.shape
    assert b.shape == a.shape and W >= 8 and H >= 8
    nx, ny = (W - 8) // 4 + 1, (H - 8) // 4 + 1
    A = a[:4 * (ny + 1), :4 * (nx + 1)].astype(np.int64)
    B = b[:4 * (ny + 1), :4 * (nx + 1)].astype(np.int64)

    def win(x):
        blk = x.reshape(ny + 1, 4, nx + 1, 4).sum(axis=(1, 3))
        return blk[:-1, :-1] + blk[:-1, 1:] + blk[1:, :-1] + blk[1:, 1:]
    return win(A), win(B), win(A * A + B * B), win(A * B)


def window_q(a, b):
    """int64 [ny, nx]: q = floor(v * 2^24) of every window."""
    s1, s2, ss, s12 = window_sums(a, b)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    cov = 64 * s12 - s1 * s2
    fa, fb, fc, fe = 2 * s1 * s2 + C1, 2 * cov + C2, s1 * s1 + s2 * s2 + C1, vars_ + C2
    for t in (fa, fb, fc, fe):
        assert np.abs(t).max() < 1 << 30
    v = (fa.astype(np.float64) * fb.astype(np.float64)) / (fc.astype(np.float64) * fe.astype(np.float64))
    return np.floor(v * 16777216.0).astype(np.int64)


def dssim(a, b):
    """The DSSIM sum of two visible planes: windows * 2^24 - sum q."""
    qs = window_q(a, b)
    out = qs.size * ONE - int(qs.sum())
    assert out >= 0
    return out


def textbook_ssim(a, b, k1=(0.01 * 255) ** 2):
    """float64 [ny, nx]: the textbook SSIM of the same windows -- uniform 8 x 8 weights, unbiased variances, C1 = k1 =
    (0.01 * 255)^2, C2 = (0.03 * 255)^2 -- computed sample by sample in floating point.  (x264's c1 = 416 stands beside
    the SUMS' product, 64^2 times the means': its luminance constant is the textbook's / 64, X264_K1.)"""
    H, W = a.shape
    nx, ny = (W - 8) // 4 + 1, (H - 8) // 4 + 1
    k2 = (0.03 * 255) ** 2
    out = np.empty((ny, nx))
    A, B = a.astype(np.float64), b.astype(np.float64)
    for y in range(ny):
        for x in range(nx):
            wa, wb = A[4 * y:4 * y + 8, 4 * x:4 * x + 8], B[4 * y:4 * y + 8, 4 * x:4 * x + 8]
            ma, mb = wa.mean(), wb.mean()
            va, vb = wa.var(ddof=1), wb.var(ddof=1)
            cab = ((wa - ma) * (wb - mb)).sum() / 63.0
            out[y, x] = (2 * ma * mb + k1) * (2 * cab + k2) / ((ma * ma + mb * mb + k1) * (va + vb + k2))
    return out


def frames_dssim_list(imgs, wl, lut, j, k=0.0):
    """The per-frame DSSIM sum of grey frames at q(j): the oracle's decode of its encode against the input."""
    out = []
    for img in imgs:
        H, W = img.shape
        dec = orc.decode_frame(orc.encode_frame(img, wl, True, q(j), lut, k=k), W, H, wl, True, q(j), lut, k=k)
        d = dssim(img, dec)
        assert d == dssim(img, qr.coder_free_frame(img, wl, j)), ("the coder-free route differs", j)
        out.append(d)
    return out


def rgb_dssim_list(planes, wl, luts, j):
    """The DSSIM sums of the R, G and B planes of an RGB frame at q(j) (quality_ref.rgb_sse_list's two routes)."""
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
    vis = lambda p: np.ascontiguousarray(np.asarray(p).reshape(AH, AW)[:H, :W]).astype(np.uint8)
    out = [dssim(planes[c], vis(dec[c])) for c in range(3)]
    assert out == [dssim(planes[c], vis(free[c])) for c in range(3)], ("the coder-free route differs", j)
    return out


# ---- the cases recorded on the oracle when the feature was specified (inputs: quality_ref.case_inputs of `inputs`;
# limit = ssim_to_dssim(target, planes * windows(W, H))):
# name -> (inputs, target SSIM, limit, j, dssim(j), previous grid value, its dssim)
CASES = {
    "200x136-wl3-0.98": ("200x136-wl3-40dB", 0.98, 542575165, 2963, 542507941, 2962, 543839825),
    "320x192-wl5-0.90": ("320x192-wl5-30dB", 0.90, 6229380300, 1432, 6222148695, 1430, 6241176044),
    "3x320x192-wl5-0.98": ("3x320x192-wl5-40dB", 0.98, 3737628180, 2964, 3737215569, 2963, 3740858679),
    "rgb-200x136-wl3-0.98": ("rgb-200x136-wl3-40dB", 0.98, 1627725496, 4965, 1627476481, 4964, 1628170251),
}
_cache = {}


def case_geometry(name):
    """(W, H, wl, frames, rgb) of a case."""
    return qr.CASES[CASES[name][0]][:5]


def case_inputs(name):
    return qr.case_inputs(CASES[name][0])


def case_limit(name):
    W, H, wl, frames, rgb = case_geometry(name)
    return ssim_to_dssim(CASES[name][1], (3 if rgb else frames) * windows(W, H))


def case_list_fn(name):
    """j -> the per-frame / per-plane DSSIM sums of a case, each j computed once."""
    key = ("list", name)
    if key not in _cache:
        W, H, wl, frames, rgb = case_geometry(name)
        imgs, lut = case_inputs(name)
        seen = {}

        def fn(j):
            if j not in seen:
                seen[j] = rgb_dssim_list(imgs, wl, lut, j) if rgb else frames_dssim_list(imgs, wl, lut, j)
            return seen[j]
        _cache[key] = fn
    return _cache[key]


def case_dssim_fn(name):
    fn = case_list_fn(name)
    return lambda j: sum(fn(j))


def case_result(name, max_dssim=None, j_min=0, j_max=0):
    """The procedure's Result for a case (its own limit unless given), computed once."""
    key = (name, CASES[name][2] if max_dssim is None else max_dssim, j_min, j_max)
    if key not in _cache:
        _cache[key] = bisect(case_dssim_fn(name), *key[1:])
    return _cache[key]


# ---- n RGB frames (rgb_search_ref.frames: frame f = the planes oracle.gen_frame(W, H, 60 + 3 f + c), the shipped tables)
def rgb_frames_lists(W, H, wl, n, j):
    """[frame][plane] DSSIM sums at q(j), each (geometry, j) computed once."""
    import rgb_search_ref as rs
    key = ("rgbn", W, H, wl, n, j)
    if key not in _cache:
        tabs = rs.luts(wl)
        _cache[key] = [rgb_dssim_list(fr, wl, tabs, j) for fr in rs.frames(W, H, n)]
    return _cache[key]


def rgb_frames_limit(W, H, n, target):
    return ssim_to_dssim(target, 3 * n * windows(W, H))


def rgb_frames_result(W, H, wl, n, max_dssim, j_min=0, j_max=0):
    key = ("rgbn-result", W, H, wl, n, max_dssim, j_min, j_max)
    if key not in _cache:
        _cache[key] = bisect(lambda j: sum(sum(p) for p in rgb_frames_lists(W, H, wl, n, j)), max_dssim, j_min, j_max)
    return _cache[key]
