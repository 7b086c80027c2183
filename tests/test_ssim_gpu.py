"""-m gpu: picsong_frames_dssim against the numpy model of the definition (ssim_ref.dssim), and the SSIM calls
(picsong_encode_frame_ssim and its mirrors) against the reference procedure (ssim_ref.bisect) over the CPU oracle's
decode of its own encode: the chosen quantiser, the streams byte for byte, the DSSIM sums reported and those of this
library's own decode -- never against the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as orc
import rate_ref as rr
import rgb_search_ref as rs
import ssim_ref as sr

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_QUALITY = -1, -8
SENTINEL = 0x5A5A
MARK = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return t


@pytest.fixture(scope="module")
def pa():
    import picsong_amd
    picsong_amd.load()
    return picsong_amd


def _lutdir(lossy=True):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _np_dssim(a, b, W, H):
    return sr.dssim(a[:H, :W], b[:H, :W])


# ---- picsong_frames_dssim -------------------------------------------------------------------------------------------
def _dssim_call(torch, c, a, a_stride, b, b_stride, n):
    """The raw call into a buffer with marks on both sides of d_dssim[0 .. n)."""
    out = torch.full((n + 2,), MARK, dtype=torch.int64, device="cuda")
    assert c.L.picsong_frames_dssim(c.h, n, c._p(a), a_stride, c._p(b), b_stride, c._p(out[1:]), c._stream()) == 0, c.L.picsong_last_error()
    got = out.cpu().numpy()
    assert got[0] == MARK and got[n + 1] == MARK
    return [int(v) for v in got[1:n + 1]]


@pytest.mark.parametrize("W,H", [(33, 32), (203, 139), (1100, 40)])
def test_frames_dssim_against_the_model(pa, torch, W, H):
    c = pa.Codec(W, H, wl=3, lossy=False)                    # a lossless context: only the geometry is used
    AW, AH, P = c.aw, c.ah, c.P
    rng = np.random.default_rng(W + H)
    a = rng.integers(0, 256, (AH, AW), dtype=np.uint8)
    b = a.copy()
    b[:H, :W] = (a[:H, :W].astype(np.int32) + rng.integers(-30, 31, (H, W))).clip(0, 255)
    b[:, W:] ^= 0xFF                                         # padding that differs does not count
    b[H:, :] ^= 0xFF
    noise = rng.integers(0, 256, (AH, AW), dtype=np.uint8)
    want, want_noise, want_neg = _np_dssim(a, b, W, H), _np_dssim(a, noise, W, H), _np_dssim(a, 255 - a, W, H)
    assert 0 < want < want_noise
    da, db = _dev(torch, a), _dev(torch, b)
    assert _dssim_call(torch, c, da, 0, db, 0, 1) == [want]
    assert _dssim_call(torch, c, da, 0, da, 0, 1) == [0]                        # equal images: every window once
    assert _dssim_call(torch, c, da, 0, _dev(torch, noise), 0, 1) == [want_noise]
    assert _dssim_call(torch, c, da, 0, _dev(torch, 255 - a), 0, 1) == [want_neg]
    assert int(c.frames_dssim(da.view(-1), db.view(-1))[0]) == want             # the binding
    # n = 3 with gaps between the frames
    za, zb = P + 4096, P + 12
    fa = rng.integers(0, 256, 3 * za, dtype=np.uint8)
    fb = rng.integers(0, 256, 3 * zb, dtype=np.uint8)
    fb[zb:zb + P] = fa[za:za + P]
    fb[2 * zb:2 * zb + P] = (fa[2 * za:2 * za + P].astype(np.int32) + rng.integers(-9, 10, P)).clip(0, 255)
    wants = [_np_dssim(fa[f * za:f * za + P].reshape(AH, AW), fb[f * zb:f * zb + P].reshape(AH, AW), W, H) for f in range(3)]
    assert wants[1] == 0 and wants[0] > wants[2] > 0
    dfa, dfb = _dev(torch, fa), _dev(torch, fb)
    assert _dssim_call(torch, c, dfa, za, dfb, zb, 3) == wants
    assert [int(v) for v in _dssim_call(torch, c, dfa, za, dfb, zb, 3)] == wants          # the same from run to run
    # misaligned: pointers offset by one byte, and an odd frame stride -- the per-byte form
    ua = torch.zeros(P + 16, dtype=torch.uint8, device="cuda")
    ub = torch.zeros(P + 16, dtype=torch.uint8, device="cuda")
    ua[1:1 + P].copy_(da.view(-1))
    ub[1:1 + P].copy_(db.view(-1))
    assert _dssim_call(torch, c, ua[1:], 0, ub[1:], 0, 1) == [want]
    assert _dssim_call(torch, c, ua[1:], 0, db, 0, 1) == [want]
    zc = P + 13
    fc = np.zeros(3 * zc, np.uint8)
    for f in range(3):
        fc[f * zc:f * zc + P] = fb[f * zb:f * zb + P]
    assert _dssim_call(torch, c, dfa, za, _dev(torch, fc), zc, 3) == wants
    # refusals: nothing launched
    out = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    L = c.L
    assert L.picsong_frames_dssim(c.h, 1, None, 0, c._p(db), 0, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_dssim(c.h, 1, c._p(da), 0, None, 0, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_dssim(c.h, 1, c._p(da), 0, c._p(db), 0, None, c._stream()) == ERR_ARG
    assert L.picsong_frames_dssim(None, 1, c._p(da), 0, c._p(db), 0, c._p(out), c._stream()) == ERR_ARG
    for n in (0, -1, 65):
        assert L.picsong_frames_dssim(c.h, n, c._p(da), P, c._p(db), P, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_dssim(c.h, 2, c._p(dfa), P - 1, c._p(dfb), zb, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_dssim(c.h, 2, c._p(dfa), za, c._p(dfb), P - 1, c._p(out), c._stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    c.close()


def test_frames_dssim_on_an_rgb_context_and_refusals_by_context(pa, torch):
    W, H = 200, 136
    c = pa.Codec(W, H, wl=3, lossy=True, qs=0.5, rgb=True)
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (3, c.ah, c.aw), dtype=np.uint8)
    b = rng.integers(0, 256, (3, c.ah, c.aw), dtype=np.uint8)
    got = c.frames_dssim(_dev(torch, a).view(3, -1), _dev(torch, b).view(3, -1))
    assert [int(v) for v in got] == [_np_dssim(a[k], b[k], W, H) for k in range(3)]
    c.close()
    out = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    deep = pa.Codec(W, H, wl=3, lossy=False, bit_depth=12)
    x = torch.zeros(2 * deep.P, dtype=torch.uint8, device="cuda")
    assert deep.L.picsong_frames_dssim(deep.h, 1, deep._p(x), 0, deep._p(x), 0, deep._p(out), deep._stream()) == ERR_ARG
    deep.close()
    # a geometry below 8 x 8: the helper refuses it, and so does the call where such a context exists
    assert pa.load().picsong_ssim_windows(7, 136, C.byref(C.c_uint64())) == ERR_ARG
    for w, h in ((7, 136), (200, 7)):
        try:
            small = pa.Codec(w, h, wl=1, lossy=False)
        except pa.PicsongError:
            continue
        y = torch.zeros(small.P, dtype=torch.uint8, device="cuda")
        assert small.L.picsong_frames_dssim(small.h, 1, small._p(y), 0, small._p(y), 0, small._p(out), small._stream()) == ERR_ARG
        small.close()
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- the search calls -----------------------------------------------------------------------------------------------
def _decoder(pa, W, H, wl, j, rgb=False):
    """A context at q(j) (picsong_ctx_create keeps (0, 1]: a gain above it through set_qs)."""
    d = pa.Codec(W, H, wl=wl, lossy=True, qs=min(rr.q(j), 1.0), lut_folder=_lutdir(), rgb=rgb)
    if rr.q(j) > 1.0:
        d.set_qs(rr.q(j))
    return d


def _frame_call(torch, c, frame, max_dssim, j_min=0, j_max=0, iter_=0):
    """picsong_encode_frame_ssim into a buffer with sentinel shorts behind picsong_max_stream_shorts; returns
    (rc, j, total, dssim, stream buffer)."""
    n = c.max_stream_shorts()
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    j, t, e = C.c_int(77), C.c_int(-5), C.c_uint64(99)
    rc = c.L.picsong_encode_frame_ssim(c.h, c._p(frame), iter_, max_dssim, j_min, j_max, c._p(buf), c._stream(), C.byref(j),
                                       C.byref(t), C.byref(e))
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "shorts behind picsong_max_stream_shorts were written"
    return rc, j.value, t.value, e.value, buf


def test_one_grey_frame(pa, torch, monkeypatch):
    name = "200x136-wl3-0.98"
    W, H, wl, frames, rgb = sr.case_geometry(name)
    _, _, limit, want_j, want_d, prev_j, prev_d = sr.CASES[name]
    res = sr.case_result(name)
    assert (res.j, res.sse, res.prev_sse) == (want_j, want_d, prev_d) and want_d <= limit < prev_d
    (img,), lut = sr.case_inputs(name)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    frame = _dev(torch, orc.pad_frame(img))
    rc, j, total, e, buf = _frame_call(torch, c, frame, limit)
    assert rc == 0, c.L.picsong_last_error()
    assert j == want_j and e == want_d
    want = orc.encode_frame(img, wl, True, rr.q(j), lut)
    assert total == want.size and np.array_equal(_u16(buf[:total]), want)
    assert c.last_total() == total and c.range_flag() == 0
    d = _decoder(pa, W, H, wl, j)
    got = d.decode_frame(buf[:c.max_stream_shorts()]).cpu().numpy()
    assert _np_dssim(got, orc.pad_frame(img), W, H) == e     # the DSSIM sum of this library's own decode
    d.close()
    # one candidate a round: the same result
    monkeypatch.setenv("PICSONG_RATE_K", "1")
    rc1, j1, total1, e1, buf1 = _frame_call(torch, c, frame, limit)
    monkeypatch.delenv("PICSONG_RATE_K")
    assert (rc1, j1, total1, e1) == (0, j, total, e) and torch.equal(buf1, buf)
    # max_dssim = 0 is a legal request that nothing meets; an unreachable limit inside a sub-range
    assert sr.case_result(name, 0).j is None
    rc, j0, _, _, _ = _frame_call(torch, c, frame, 0)
    assert rc == ERR_QUALITY and j0 == 0
    sub = sr.case_result(name, limit, 1000, 2500)
    assert sub.j is None
    rc, j0, _, _, _ = _frame_call(torch, c, frame, limit, 1000, 2500)
    assert rc == ERR_QUALITY and j0 == 0
    with pytest.raises(pa.QualityError):
        c.encode_frame_ssim(frame, limit, 1000, 2500)
    # a sub-range that holds the result, through the binding; and an unaligned frame takes the per-byte kernel
    assert sr.case_result(name, limit, 2900, 3000).j == want_j
    jb, sb, eb = c.encode_frame_ssim(frame, limit, 2900, 3000)
    assert (jb, eb) == (want_j, want_d) and np.array_equal(_u16(sb), want)
    big = torch.zeros(c.P + 64, dtype=torch.uint8, device="cuda")
    un = big[1:1 + c.P]
    un.copy_(frame.view(-1))
    ju, su, eu = c.encode_frame_ssim(un, limit, 2900, 3000)
    assert (ju, eu) == (want_j, want_d) and np.array_equal(_u16(su), want)
    c.close()


def test_three_grey_frames(pa, torch, monkeypatch):
    name = "3x320x192-wl5-0.98"
    W, H, wl, n, rgb = sr.case_geometry(name)
    _, _, limit, want_j, want_d, prev_j, prev_d = sr.CASES[name]
    res = sr.case_result(name)
    per = sr.case_list_fn(name)(want_j)
    assert (res.j, res.sse) == (want_j, want_d) == (want_j, sum(per)) and want_d <= limit < res.prev_sse == prev_d
    imgs, lut = sr.case_inputs(name)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=0.5, lut_folder=_lutdir())
    frames = _dev(torch, np.stack([orc.pad_frame(im).ravel() for im in imgs]))
    j, streams, e = c.encode_frames_ssim(frames, limit)
    assert j == want_j and e == per
    want = [orc.encode_frame(imgs[f], wl, True, rr.q(j), lut, iter_=f) for f in range(n)]
    for f in range(n):
        assert np.array_equal(_u16(streams[f]), want[f]), f
    assert c.last_totals(n) == [w.size for w in want]
    d = _decoder(pa, W, H, wl, j)
    for f in range(n):
        full = torch.zeros(c.max_stream_shorts(), dtype=torch.int16, device="cuda")
        full[:streams[f].numel()] = streams[f]
        assert _np_dssim(d.decode_frame(full).cpu().numpy(), orc.pad_frame(imgs[f]), W, H) == per[f]
    d.close()
    monkeypatch.setenv("PICSONG_RATE_K", "1")
    j1, s1, e1 = c.encode_frames_ssim(frames, limit)
    monkeypatch.delenv("PICSONG_RATE_K")
    assert j1 == j and e1 == per and all(np.array_equal(_u16(s1[f]), want[f]) for f in range(n))
    with pytest.raises(pa.QualityError):
        c.encode_frames_ssim(frames, 0)
    # the context's own qs is unchanged
    assert np.array_equal(_u16(c.encode_frame(frames[0])), orc.encode_frame(imgs[0], wl, True, 0.5, lut))
    c.close()


def _rgb_header(W, H, wl, j):
    return orc.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=8, lossy=1, qs_1e4=j, components=3,
                           is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=0)


def _rgb_call(torch, c, rgb, n, limit, j_min=0, j_max=0, first_iter=0, mask=7):
    ms = c.max_stream_shorts()
    buf = torch.full((3 * n, ms + 64), SENTINEL, dtype=torch.int16, device="cuda")
    j, t, e = C.c_int(77), (C.c_int * (3 * n))(*([-5] * (3 * n))), (C.c_uint64 * (3 * n))(*([99] * (3 * n)))
    rc = c.L.picsong_encode_rgb_frames_ssim(c.h, n, c._p(rgb[0]), c._p(rgb[1]), c._p(rgb[2]), rgb[0].stride(0) if n > 1 else 0,
                                            first_iter, mask, limit, j_min, j_max, c._p(buf), buf.stride(0), c._stream(),
                                            C.byref(j), t, e)
    torch.cuda.synchronize()
    assert bool((buf[:, ms:] == SENTINEL).all()), "shorts behind picsong_max_stream_shorts were written"
    return rc, j.value, list(t), [int(v) for v in e], buf


@pytest.mark.parametrize("W,H,wl,n", [(200, 136, 3, 1), (320, 192, 5, 2)])
def test_rgb_frames(pa, torch, monkeypatch, W, H, wl, n):
    limit = sr.rgb_frames_limit(W, H, n, 0.98)
    res = sr.rgb_frames_result(W, H, wl, n, limit)
    assert res.j is not None and res.sse <= limit < res.prev_sse
    if n == 1:                                               # frame 0 is the recorded case's
        assert (limit, res.j, res.sse, res.prev_j, res.prev_sse) == sr.CASES["rgb-200x136-wl3-0.98"][2:]
    per = [v for fr in sr.rgb_frames_lists(W, H, wl, n, res.j) for v in fr]
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=0.75, lut_folder=_lutdir(), rgb=True)
    rgb = [_dev(torch, p) for p in rs.padded_stack(W, H, n)]
    rc, j, totals, e, buf = _rgb_call(torch, c, rgb, n, limit)
    assert rc == 0, c.L.picsong_last_error()
    assert j == res.j and e == per and sum(e) == res.sse
    want = rs.streams(W, H, wl, n, j, _rgb_header(W, H, wl, j), 0, 7)
    assert totals == [w.size for w in want]
    for z, w in enumerate(want):
        assert np.array_equal(_u16(buf[z, :totals[z]]), w), z
    assert c.last_totals(3 * n) == totals
    d = _decoder(pa, W, H, wl, j, rgb=True)
    back = d.decode_rgb_frames(buf[:, :c.max_stream_shorts()])
    host = [p.cpu().numpy() for p in rgb]
    assert [_np_dssim(back[k][f].cpu().numpy(), host[k][f], W, H) for f in range(n) for k in range(3)] == e
    d.close()
    monkeypatch.setenv("PICSONG_RATE_K", "1")
    rc1, j1, totals1, e1, buf1 = _rgb_call(torch, c, rgb, n, limit)
    monkeypatch.delenv("PICSONG_RATE_K")
    assert (rc1, j1, totals1, e1) == (0, j, totals, e) and torch.equal(buf1, buf)
    rc0, j0, _, _, _ = _rgb_call(torch, c, rgb, n, 0)
    assert rc0 == ERR_QUALITY and j0 == 0
    assert sr.rgb_frames_result(W, H, wl, n, limit, 1000, 2500).j is None
    rc0, j0, _, _, _ = _rgb_call(torch, c, rgb, n, limit, 1000, 2500)
    assert rc0 == ERR_QUALITY and j0 == 0
    jb, streams, eb = c.encode_rgb_frames_ssim(*rgb, limit)                            # the binding
    assert jb == j and eb == e and [s.numel() for s in streams] == totals
    c.close()


def test_refusals_launch_nothing(pa, torch):
    W, H, wl = 200, 136, 3
    img = orc.pad_frame(orc.gen_frame(W, H))
    frame = _dev(torch, img)
    limit = 542575165

    def refused(c, call):
        """`call(stream buffer, j, totals, dssim)` -> rc: PICSONG_ERR_ARG, the outputs and the range flag untouched."""
        n = c.max_stream_shorts()
        buf = torch.full((3, n), SENTINEL, dtype=torch.int16, device="cuda")
        j, t, e = C.c_int(77), (C.c_int * 16)(*([-5] * 16)), (C.c_uint64 * 16)(*([99] * 16))
        assert call(buf, j, t, e) == ERR_ARG
        torch.cuda.synchronize()
        assert j.value == 77 and list(t) == [-5] * 16 and list(e) == [99] * 16 and bool((buf == SENTINEL).all())
        if c.bit_depth == 8:
            assert c.range_flag() == 0

    def grey(c, j_min=0, j_max=0, fr=frame):
        return lambda buf, j, t, e: c.L.picsong_encode_frame_ssim(c.h, c._p(fr) if fr is not None else None, 0, limit, j_min,
                                                                  j_max, c._p(buf), c._stream(), C.byref(j), t, e)

    def batch(c, n=2, stride=None, fr=None, sstride=None):
        fr2 = torch.stack([frame.view(-1)] * 2) if fr is None else fr
        return lambda buf, j, t, e: c.L.picsong_encode_frames_ssim(c.h, n, c._p(fr2), c.P if stride is None else stride, 0, 2 * limit,
                                                                   0, 0, c._p(buf), buf.stride(0) if sstride is None else sstride,
                                                                   c._stream(), C.byref(j), t, e)

    def rgb(c, planes=(frame, frame, frame), n=1):
        return lambda buf, j, t, e: c.L.picsong_encode_rgb_frames_ssim(c.h, n, c._p(planes[0]), c._p(planes[1]), c._p(planes[2]), 0,
                                                                       0, 7, 3 * limit, 0, 0, c._p(buf), buf.stride(0), c._stream(),
                                                                       C.byref(j), t, e)

    lossless = pa.Codec(W, H, wl=wl, lossy=False, lut_folder=_lutdir(False))
    refused(lossless, grey(lossless))
    refused(lossless, batch(lossless))
    lossless.close()
    cp3 = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, cp=3)
    refused(cp3, grey(cp3))
    cp3.close()
    col = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir(), rgb=True)
    refused(col, grey(col))
    refused(col, batch(col))
    big3 = torch.zeros(3 * col.P + 64, dtype=torch.uint8, device="cuda")
    refused(col, rgb(col, (big3[1:], frame, frame)))                            # a plane not 4-byte aligned
    refused(col, rgb(col, n=0))
    refused(col, rgb(col, n=22))
    col.close()
    deep = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, bit_depth=12)
    refused(deep, grey(deep))
    refused(deep, batch(deep))
    deep.close()
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    refused(c, rgb(c))
    for lo, hi in ((0, 5), (5, 0), (3, 2), (-1, 4), (1, 16384), (7, 7)):       # (7, 7): a range without a grid entry
        refused(c, grey(c, j_min=lo, j_max=hi))
    refused(c, grey(c, fr=None))
    call = c.L.picsong_encode_frame_ssim
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, limit, 0, 0, c._p(buf), c._stream(), None, t, e))
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, limit, 0, 0, c._p(buf), c._stream(), C.byref(j), None, e))
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, limit, 0, 0, c._p(buf), c._stream(), C.byref(j), t, None))
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, limit, 0, 0, None, c._stream(), C.byref(j), t, e))
    refused(c, batch(c, n=0))
    refused(c, batch(c, n=17))
    refused(c, batch(c, stride=c.P - 16))
    refused(c, batch(c, sstride=c.max_stream_shorts() - 1))
    big = torch.zeros(2 * c.P + 64, dtype=torch.uint8, device="cuda")
    refused(c, batch(c, fr=big[1:]))                                            # frames not 16-byte aligned
    c.close()
    nolut = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0)
    refused(nolut, grey(nolut))
    nolut.close()
    # a geometry below 8 x 8, where such a context exists
    for w, h in ((7, 136), (200, 7)):
        try:
            small = pa.Codec(w, h, wl=1, lossy=True, qs=1.0)
        except pa.PicsongError:
            continue
        y = torch.zeros(small.P, dtype=torch.uint8, device="cuda")
        refused(small, grey(small, fr=y))
        small.close()
