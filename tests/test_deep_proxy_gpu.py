"""-m gpu: the deep proxy calls -- picsong_decode_frames16_reduced / _window, picsong_decode_rgb_frames16_reduced / _window and
the 16-bit layouts of picsong_decode_rgb_images_reduced / _window -- through the C ABI and picsong_amd.Codec, against
deep_proxy_ref (the CPU oracle's LL_r between numpy ends), never against the code under test.  Every output lies in a device
buffer of sentinel bytes that must survive around it; every comparison is byte for byte.  No out-of-range input here."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import deep_proxy_ref as X
import deep_ref as D
import deep_rgb_ref as R
import oracle_lib as orc
import reduced_ref as rr
import window_ref as wr

pytestmark = pytest.mark.gpu
ERR_ARG = -1
W, H, AW, AH = D.W, D.H, D.AW, D.AH
P = AW * AH
BS = 0xA5
P3_16, RGB48, RGBA64 = 7, 8, 9
SPP = {P3_16: 1, RGB48: 3, RGBA64: 4}

GREY = [(False, 12, "saw", 5, 1.0, 0), (False, 9, "saw", 2, 1.0, 0), (False, 12, "noise", 5, 1.0, 9), (True, 12, "smooth", 3, 1.0, 0),
        (True, 16, "noise", 3, 0.25, 12)]
RGB = [R.row(False, 12, "saw"), R.row(False, 9, "saw"), R.row(False, 12, "noise"), R.row(True, 12, "saw"), R.row(True, 16, "noise")]
GREY_IDS = [f"{'97' if c[0] else '53'}-{c[1]}-{c[2]}" for c in GREY]
RGB_IDS = [R.row_id(r) for r in RGB]


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


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _lutdir(lossy):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _codec(pa, bd, wl, lossy, qs=1.0, k=0.0, rgb=False):
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), k=k, bit_depth=bd, is_rgb=rgb)


def _streams(torch, c, streams):
    sb = np.full((len(streams), c.max_stream_shorts()), 0xFFFF, np.uint16)
    for z, s in enumerate(streams):
        sb[z, :s.size] = s
    return torch.from_numpy(sb.view(np.int16)).cuda()


class Out:
    """n frames of `planes` planes of h rows of `row` bytes at `pitch` in a device buffer of sentinel bytes, `off` bytes behind a
    256-byte boundary: plane c of frame f at f * fs + c * pstep, pstep = span + pgap, fs = planes * pstep + gap."""

    def __init__(self, torch, n, planes, h, row, pitch=None, off=0, pgap=0, gap=0):
        self.n, self.planes, self.h, self.row = n, planes, h, row
        self.pitch = row if pitch is None else pitch
        self.span = (h - 1) * self.pitch + row
        self.pstep = self.span + pgap
        self.fs = planes * self.pstep + gap
        self.base = 256 + off
        self.t = torch.full((self.base + n * self.fs + 256,), BS, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0

    def ptr(self, c=0):
        return C.c_void_p(self.t.data_ptr() + self.base + c * self.pstep)

    def fetch(self):
        """the planes [n][planes] as uint16 (h, row / 2), after checking that nothing else was written"""
        raw = self.t.cpu().numpy()
        mask = np.ones(raw.size, bool)
        out = []
        for f in range(self.n):
            planes = []
            for c in range(self.planes):
                o = self.base + f * self.fs + c * self.pstep
                rows = []
                for y in range(self.h):
                    rows.append(raw[o + y * self.pitch:o + y * self.pitch + self.row].copy().view(np.uint16))
                    mask[o + y * self.pitch:o + y * self.pitch + self.row] = False
                planes.append(np.stack(rows))
            out.append(planes)
        assert (raw[mask] == BS).all(), "a byte outside the documented rows was written"
        return out

    def untouched(self):
        return bool((self.t == BS).all().item())


def grey(torch, c, d_s, n, r, win=None, extra=0, off=0, gap=0):
    x, y, w, h = win if win else (0, 0, AW >> r, AH >> r)
    out = Out(torch, n, 1, h, 2 * w, 2 * w + (extra if win else 0), off, 0, gap)
    if win:
        rc = c.L.picsong_decode_frames16_window(c.h, n, c._p(d_s), d_s.stride(0), r, x, y, w, h, out.ptr(), out.pitch, out.fs, c._stream())
    else:
        rc = c.L.picsong_decode_frames16_reduced(c.h, n, c._p(d_s), d_s.stride(0), r, out.ptr(), out.fs, c._stream())
    assert rc == 0, c.L.picsong_last_error()
    return [f[0] for f in out.fetch()]


def rgb(torch, c, d_s, n, r, win=None, layout=P3_16, images=False, extra=0, off=0, pgap=0, gap=0, bd=12, pa=None):
    x, y, w, h = win if win else (0, 0, AW >> r, AH >> r)
    spp, planes = SPP[layout], 3 if layout == P3_16 else 1
    out = Out(torch, n, planes, h, 2 * w * spp, 2 * w * spp + (extra if win else 0), off, pgap, gap)
    if images:
        img = pa.Image(data=out.ptr().value, pitch=out.pitch, plane_stride=out.pstep if planes == 3 else 0, layout=layout)
        if win:
            rc = c.L.picsong_decode_rgb_images_window(c.h, n, c._p(d_s), d_s.stride(0), r, x, y, w, h, C.byref(img), out.fs, c._stream())
        else:
            rc = c.L.picsong_decode_rgb_images_reduced(c.h, n, c._p(d_s), d_s.stride(0), r, C.byref(img), out.fs, c._stream())
    elif win:
        rc = c.L.picsong_decode_rgb_frames16_window(c.h, n, c._p(d_s), d_s.stride(0), r, x, y, w, h, out.ptr(0), out.ptr(1), out.ptr(2), out.pitch,
                                                    out.fs, c._stream())
    else:
        rc = c.L.picsong_decode_rgb_frames16_reduced(c.h, n, c._p(d_s), d_s.stride(0), r, out.ptr(0), out.ptr(1), out.ptr(2), out.fs, c._stream())
    assert rc == 0, c.L.picsong_last_error()
    frames = []
    for f in out.fetch():
        if planes == 3:
            frames.append(f)
        else:
            px = f[0].reshape(h, w, spp)
            if spp == 4:
                assert (px[:, :, 3] == (1 << bd) - 1).all(), "alpha = mx"
            frames.append([np.ascontiguousarray(px[:, :, k]) for k in range(3)])
    return frames


def _all(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---- expected output, computed once and left unchanged -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grey_streams(case):
    """the row's stream first (its precondition asserted on the oracle alone), then the other kinds of the same parameters that
    stay in range, up to three frames"""
    lossy, bd, kind, wl, qs, raw = case
    img, pad, coef, sizes, stream = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, raw)
    out = [stream]
    for other in ("saw", "smooth", "noise"):
        if other != kind and len(out) < 3:
            e = D.encode(other, bd, wl, lossy, qs)
            if D.max_coef(e[2]) < 32768:
                out.append(e[4])
    while len(out) < 3:
        out.append(stream)
    return out


@functools.lru_cache(maxsize=None)
def grey_want(case, f, r, drop=0):
    lossy, bd, kind, wl, qs, raw = case
    out = X.grey_reduced(grey_streams(case)[f], bd, wl, lossy, qs, r, drop=drop)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rgb_streams(case):
    lossy, bd, kind, wl, qs, want_max, want_raw = case
    img, pad, comp, coef, sizes, streams = R.encode(kind, bd, wl, lossy, qs)
    R.check_precondition(coef, sizes, want_max, want_raw)
    out = [list(streams)]
    for other in ("saw", "smooth", "noise"):
        if other != kind and len(out) < 3:
            e = R.encode(other, bd, wl, lossy, qs)
            if max(R.max_coef(e[3])) < 32768:
                out.append(list(e[5]))
    while len(out) < 3:
        out.append(list(streams))
    return out


@functools.lru_cache(maxsize=None)
def rgb_want(case, f, r, drop=0):
    lossy, bd, kind, wl, qs = case[:5]
    out = X.rgb_reduced(rgb_streams(case)[f], bd, wl, lossy, qs, r, drop=drop)
    for o in out:
        o.setflags(write=False)
    return out


def six_windows(r):
    """six of window_ref.windows: a corner, an edge, 1 x 1, the odd one, the one reaching into the padding, the whole image"""
    vw, vh = rr.visible(W, H, r)
    ws = wr.windows(AW >> r, AH >> r, vw, vh)
    return [ws[3], ws[4], ws[9], ws[10], ws[12] if len(ws) > 12 else ws[8], ws[11]]


VARIATION = ((0, 0), (2, 0), (6, 2), (16, 0), (0, 2), (6, 0))      # (pitch excess, misalignment) of the six windows


# ---- the rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GREY, ids=GREY_IDS)
def test_grey_rows(pa, torch, case):
    lossy, bd, kind, wl, qs, raw = case
    c = _codec(pa, bd, wl, lossy, qs)
    d3 = _streams(torch, c, grey_streams(case))
    for r in sorted({0, 1, wl - 1}):
        want = [grey_want(case, f, r) for f in range(3)]
        ones = [grey(torch, c, d3[f:f + 1], 1, r)[0] for f in range(3)]
        assert _all(ones, want), r
        for gap, off in ((0, 0), (6, 2), (32, 0)):           # aligned (the fused store), misaligned (the clamp pass)
            assert _all(grey(torch, c, d3, 3, r, gap=gap, off=off), ones), (r, gap, off)
        if r == 0:
            assert np.array_equal(c.decode_frames16(d3[:1]).cpu().numpy().view(np.uint16)[0], ones[0]), "reduce = 0 is picsong_decode_frames16"
        for i, win in enumerate(six_windows(r)):
            extra, off = VARIATION[i]
            wants = [X.window(w_, *win) for w_ in want]
            assert _all(grey(torch, c, d3[:1], 1, r, win, extra=extra, off=off), wants[:1]), (r, win)
            if i % 3 == 0:
                assert _all(grey(torch, c, d3, 3, r, win, extra=extra, off=off, gap=6), wants), (r, win)
            assert c.window_codeblocks(*win, r=r) == len(wr.window_codeblocks(AW, AH, wl, lossy, r, *win))
    assert c.reduced_dims(1)[:4] == (*rr.visible(W, H, 1), AW >> 1, AH >> 1)
    assert c.range_flag() == 0
    # the binding
    got = c.decode_frames16_reduced(d3, 1).cpu().numpy().view(np.uint16)
    assert _all(list(got), [grey_want(case, f, 1) for f in range(3)])
    got = c.decode_frames16_window(d3, 3, 5, 17, 11, r=1).cpu().numpy().view(np.uint16)
    assert _all(list(got), [X.window(grey_want(case, f, 1), 3, 5, 17, 11) for f in range(3)])
    c.close()


@pytest.mark.parametrize("case", RGB, ids=RGB_IDS)
def test_rgb_rows(pa, torch, case):
    lossy, bd, kind, wl, qs = case[:5]
    c = _codec(pa, bd, wl, lossy, qs, rgb=True)
    d9 = _streams(torch, c, sum(rgb_streams(case), []))
    for r in sorted({0, 1, wl - 1}):
        want = [rgb_want(case, f, r) for f in range(3)]
        ones = [rgb(torch, c, d9[3 * f:3 * f + 3], 1, r)[0] for f in range(3)]
        assert all(_all(o, w_) for o, w_ in zip(ones, want)), r
        for gap, pgap, off in ((0, 0, 0), (6, 10, 2), (32, 16, 0)):
            got = rgb(torch, c, d9, 3, r, gap=gap, pgap=pgap, off=off)
            assert all(_all(g, o) for g, o in zip(got, ones)), (r, gap, pgap, off)
        if r == 0:
            full = c.decode_rgb_frames16(d9[:3])
            assert _all([t[0].cpu().numpy().view(np.uint16) for t in full], ones[0]), "reduce = 0 is picsong_decode_rgb_frames16"
        for i, win in enumerate(six_windows(r)):
            extra, off = VARIATION[i]
            wants = [X.window(w_, *win) for w_ in want]
            assert _all(rgb(torch, c, d9[:3], 1, r, win, extra=extra, off=off, pgap=2 * (i % 2))[0], wants[0]), (r, win)
            if i % 3 == 0:
                got = rgb(torch, c, d9, 3, r, win, extra=extra, off=off, gap=6, pgap=4)
                assert all(_all(g, w_) for g, w_ in zip(got, wants)), (r, win)
            assert c.window_codeblocks(*win, r=r) == len(wr.window_codeblocks(AW, AH, wl, lossy, r, *win))
    assert c.range_flag() == 0
    # the three layouts at pitches packed and + 6 (the vector and the per-sample form), n = 1 and 3
    r = 1
    vw, vh = rr.visible(W, H, r)
    for layout in (P3_16, RGB48, RGBA64):
        for win in ((8, 4, 40, 9), (5, 3, 5, 4), (0, 0, AW >> r, AH >> r)):
            for extra in (0, 6):
                got = rgb(torch, c, d9, 3, r, win, layout=layout, images=True, extra=extra, gap=2 * extra, bd=bd, pa=pa)
                assert all(_all(g, X.window(rgb_want(case, f, r), *win)) for f, g in enumerate(got)), (layout, win, extra)
        got = rgb(torch, c, d9[:3], 1, r, (0, 0, vw, vh), layout=layout, images=True, bd=bd, pa=pa)
        assert _all(got[0], X.window(rgb_want(case, 0, r), 0, 0, vw, vh))
        out = Out(torch, 1, 3 if layout == P3_16 else 1, vh, 2 * vw * SPP[layout], 2 * vw * SPP[layout] + 6)
        c.decode_rgb_images_reduced(d9[:3], r, pa.Image(data=out.ptr().value, pitch=out.pitch, plane_stride=out.pstep, layout=layout))
        f = out.fetch()[0]
        planes = f if layout == P3_16 else [np.ascontiguousarray(f[0].reshape(vh, vw, SPP[layout])[:, :, k]) for k in range(3)]
        assert _all(planes, X.window(rgb_want(case, 0, r), 0, 0, vw, vh)), "images_reduced = the window (0, 0, rw, rh)"
    # the binding
    got = c.decode_rgb_frames16_reduced(d9, 1)
    for f in range(3):
        assert _all([t[f].cpu().numpy().view(np.uint16) for t in got], rgb_want(case, f, 1))
    mine = [torch.zeros((3, (AH >> 1) + 2, AW >> 1), dtype=torch.int16, device="cuda")[:, :AH >> 1] for _ in range(3)]
    c.decode_rgb_frames16_reduced(d9, 1, outs=mine)          # (the caller's planes: the frame stride is theirs)
    for f in range(3):
        assert _all([t[f].cpu().numpy().view(np.uint16) for t in mine], rgb_want(case, f, 1))
    got = c.decode_rgb_frames16_window(d9, 3, 5, 17, 11, r=1)
    for f in range(3):
        assert _all([t[f].cpu().numpy().view(np.uint16) for t in got], X.window(rgb_want(case, f, 1), 3, 5, 17, 11))
    c.close()


def test_nofuse_gives_the_same_bytes(pa, torch):
    case, row = GREY[3], RGB[3]
    c = _codec(pa, case[1], case[3], case[0], case[4])
    d3 = _streams(torch, c, grey_streams(case))
    cc = _codec(pa, row[1], row[3], row[0], row[4], rgb=True)
    d9 = _streams(torch, cc, sum(rgb_streams(row), []))
    with env(PICSONG_DEEP_NOFUSE=1):
        for r in (0, 1):
            assert _all(grey(torch, c, d3, 3, r), [grey_want(case, f, r) for f in range(3)])
            got = rgb(torch, cc, d9, 3, r)
            assert all(_all(g, rgb_want(row, f, r)) for f, g in enumerate(got))
    c.close()
    cc.close()


# ---- both clamp ends -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [9, 12])
@pytest.mark.parametrize("lossy", [False, True])
def test_both_clamp_ends(pa, torch, bd, lossy):
    """A hand-built Mallat array whose LL band alternates between values past both ends, coded by the context's own coder
    (picsong_bpc_encode + picsong_bitstream_pack), then the window call.  bd = 16 is the emulator's alone: +-(2^15 + 100) is no
    magnitude the coder takes."""
    wl, r = 2, 0
    off, mx = 1 << (bd - 1), (1 << bd) - 1
    amp = (off + 100) * (8 if lossy else 1)
    assert amp < 32768
    coef = np.zeros((AH, AW), np.int32)
    yy, xx = np.mgrid[0:AH >> wl, 0:AW >> wl]
    coef[:AH >> wl, :AW >> wl] = np.where(((xx // 4) + (yy // 4)) % 2 == 0, amp, -amp)
    want = X.synthesis_grey(coef, bd, wl, lossy, 1.0, r)
    assert want.min() == 0 and want.max() == mx
    c = _codec(pa, bd, wl, lossy)
    dc = torch.from_numpy(coef.astype(np.float32) if lossy else coef).cuda().reshape(-1)
    st, sz = c.bpc_encode(dc)
    stream = c.bitstream_pack(st, sz).cpu().numpy().view(np.uint16)
    d_s = _streams(torch, c, [stream])
    win = (5, 3, 201, 150)
    assert np.array_equal(grey(torch, c, d_s, 1, r, win, extra=6)[0], X.window(want, *win))
    c.close()
    coefs = [coef, -coef, coef]
    want3 = X.synthesis_rgb(coefs, bd, wl, lossy, 1.0, r)
    assert min(p.min() for p in want3) == 0 and max(p.max() for p in want3) == mx
    cc = _codec(pa, bd, wl, lossy, rgb=True)
    streams = []
    for k in range(3):
        dk = torch.from_numpy(coefs[k].astype(np.float32) if lossy else coefs[k]).cuda().reshape(-1)
        st = torch.empty(cc.P, dtype=torch.int32, device=cc.dev)
        sz = torch.empty(cc.ncb, dtype=torch.int32, device=cc.dev)
        assert cc.L.picsong_bpc_encode_component(cc.h, k, cc._p(dk), cc._p(st), cc._p(sz), cc._stream()) == 0, cc.L.picsong_last_error()
        streams.append(cc.bitstream_pack(st, sz).cpu().numpy().view(np.uint16))
    d_s = _streams(torch, cc, streams)
    for layout, images in ((P3_16, False), (RGBA64, True)):
        got = rgb(torch, cc, d_s, 1, r, win, layout=layout, images=images, extra=6 if not images else 0, bd=bd, pa=pa)
        assert _all(got[0], X.window(want3, *win))
    cc.close()


def test_drop_composes(pa, torch):
    case, row = GREY[3], R.row(True, 12, "smooth")
    lossy, bd, kind, wl, qs, raw = case
    c = _codec(pa, bd, wl, lossy, qs)
    d3 = _streams(torch, c, grey_streams(case))
    c.set_decode_drop(2)
    want = grey_want(case, 0, 1, 2)
    assert not np.array_equal(want, grey_want(case, 0, 1)), "drop = 2 changes the picture"
    assert np.array_equal(grey(torch, c, d3[:1], 1, 1)[0], want)
    win = (9, 13, 51, 30)
    assert np.array_equal(grey(torch, c, d3[:1], 1, 1, win, extra=2)[0], X.window(want, *win))
    c.close()
    cc = _codec(pa, row[1], row[3], row[0], row[4], rgb=True)
    streams = list(R.encode(row[2], row[1], row[3], row[0], row[4])[5])
    d_s = _streams(torch, cc, streams)
    cc.set_decode_drop(2)
    want3 = X.rgb_reduced(streams, row[1], row[3], row[0], row[4], 1, drop=2)
    assert _all(rgb(torch, cc, d_s, 1, 1)[0], want3)
    assert _all(rgb(torch, cc, d_s, 1, 1, win)[0], X.window(want3, *win))
    cc.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(pa, torch):
    bd, wl = 12, 3
    lut = _lutdir(False)
    g16 = _codec(pa, bd, wl, False)
    c16 = _codec(pa, bd, wl, False, rgb=True)
    g8 = pa.Codec(W, H, wl=wl, lut_folder=lut)
    c8 = pa.Codec(W, H, wl=wl, lut_folder=lut, rgb=True)
    g16cp3 = pa.Codec(W, H, wl=wl, cp=3, bit_depth=bd)
    c16cp3 = pa.Codec(W, H, wl=wl, cp=3, bit_depth=bd, is_rgb=True)
    L, s, vp = g16.L, g16._stream(), C.c_void_p
    ms = g16.max_stream_shorts()
    out = torch.full((1 << 20,), BS, dtype=torch.uint8, device="cuda")
    st = torch.full((9, ms), 0x5A5A, dtype=torch.int16, device="cuda")
    o, ps = out.data_ptr(), st.data_ptr()
    pp = 2 * (AW >> 1) * (AH >> 1)
    r_, g_, b_ = vp(o), vp(o + pp), vp(o + 2 * pp)
    rw, gw_, bw = vp(o), vp(o + 4096), vp(o + 8192)

    def img(layout, pitch, plane_stride=0, data=None):
        return pa.Image(data=o if data is None else data, pitch=pitch, plane_stride=plane_stride, layout=layout)

    GR, GW = L.picsong_decode_frames16_reduced, L.picsong_decode_frames16_window
    CR, CW = L.picsong_decode_rgb_frames16_reduced, L.picsong_decode_rgb_frames16_window
    IR, IW = L.picsong_decode_rgb_images_reduced, L.picsong_decode_rgb_images_window
    g, c = g16.h, c16.h
    # what works, so that the refusals below are refusals of the one thing each changes (streams of 0x5A5A decode to rubbish:
    # only the argument checks matter here, and nothing is launched by a refused call)
    def refused(rc, name=None):
        assert rc == ERR_ARG, (rc, name)
        if name:
            assert name in L.picsong_last_error(), (name, L.picsong_last_error())

    # the kind of context, the message naming the call to use instead
    refused(GR(g8.h, 1, vp(ps), ms, 1, vp(o), 0, s), b"picsong_decode_frames_reduced")
    refused(GW(g8.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 32, 0, s), b"picsong_decode_frames_window")
    refused(CR(c8.h, 1, vp(ps), ms, 1, r_, g_, b_, 0, s), b"picsong_decode_rgb_frames_reduced")
    refused(CW(c8.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 0, s), b"picsong_decode_rgb_frames_window")
    refused(GR(c, 1, vp(ps), ms, 1, vp(o), 0, s), b"picsong_decode_rgb_frames16_reduced")
    refused(GW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 32, 0, s), b"picsong_decode_rgb_frames16_window")
    refused(CR(g, 1, vp(ps), ms, 1, r_, g_, b_, 0, s), b"picsong_decode_frames16_reduced")
    refused(CW(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 0, s), b"picsong_decode_frames16_window")
    refused(GR(g8.h, 1, vp(ps), ms, 1, vp(o), 0, s))
    refused(CR(g8.h, 1, vp(ps), ms, 1, r_, g_, b_, 0, s))
    for rc in (
        # null pointers, n, reduce
        GR(g, 1, None, ms, 1, vp(o), 0, s), GR(g, 1, vp(ps), ms, 1, None, 0, s), GR(None, 1, vp(ps), ms, 1, vp(o), 0, s),
        GW(g, 1, None, ms, 1, 0, 0, 16, 16, vp(o), 32, 0, s), GW(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, None, 32, 0, s),
        CR(c, 1, None, ms, 1, r_, g_, b_, 0, s), CR(c, 1, vp(ps), ms, 1, r_, None, b_, 0, s), CR(c, 1, vp(ps), ms, 1, r_, g_, None, 0, s),
        CW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, None, gw_, bw, 32, 0, s), CW(c, 1, None, ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 0, s),
        GR(g, 0, vp(ps), ms, 1, vp(o), pp, s), GR(g, 65, vp(ps), ms, 1, vp(o), pp, s), GW(g, 65, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 32, 4096, s),
        CR(c, 0, vp(ps), ms, 1, r_, g_, b_, 3 * pp, s), CR(c, 22, vp(ps), ms, 1, r_, g_, b_, 3 * pp, s),
        CW(c, 22, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 3 * 4096, s),
        GR(g, 1, vp(ps), ms, -1, vp(o), 0, s), GR(g, 1, vp(ps), ms, wl, vp(o), 0, s), GW(g, 1, vp(ps), ms, wl, 0, 0, 16, 16, vp(o), 32, 0, s),
        CR(c, 1, vp(ps), ms, wl, r_, g_, b_, 0, s), CW(c, 1, vp(ps), ms, -1, 0, 0, 16, 16, rw, gw_, bw, 32, 0, s),
        # windows
        GW(g, 1, vp(ps), ms, 1, 0, 0, 0, 16, vp(o), 32, 0, s), GW(g, 1, vp(ps), ms, 1, 0, 0, 16, 0, vp(o), 32, 0, s),
        GW(g, 1, vp(ps), ms, 1, -1, 0, 16, 16, vp(o), 32, 0, s), GW(g, 1, vp(ps), ms, 1, 120, 0, 9, 16, vp(o), 32, 0, s),
        GW(g, 1, vp(ps), ms, 1, 0, 90, 16, 7, vp(o), 32, 0, s),
        CW(c, 1, vp(ps), ms, 1, 0, 0, 0, 16, rw, gw_, bw, 32, 0, s), CW(c, 1, vp(ps), ms, 1, 120, 0, 9, 16, rw, gw_, bw, 32, 0, s),
        CW(c, 1, vp(ps), ms, 1, 0, 90, 16, 7, rw, gw_, bw, 32, 0, s),
        # odd pointers, pitches, strides; out_pitch < 2 w
        GR(g, 1, vp(ps), ms, 1, vp(o + 1), 0, s), GR(g, 1, vp(ps + 1), ms, 1, vp(o), 0, s), GR(g, 2, vp(ps), ms, 1, vp(o), pp + 1, s),
        GW(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o + 1), 32, 0, s), GW(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 33, 0, s),
        GW(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 30, 0, s), GW(g, 2, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 32, 4097, s),
        CR(c, 1, vp(ps), ms, 1, vp(o + 1), g_, b_, 0, s), CR(c, 2, vp(ps), ms, 1, r_, g_, b_, 3 * pp + 1, s),
        CW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, vp(o + 4097), bw, 32, 0, s), CW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 33, 0, s),
        CW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 30, 0, s), CW(c, 2, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 3 * 4096 + 1, s),
        # n > 1: a frame_stride below a plane's span, or one that makes a frame's planes overlap the next frame's; stream strides
        GR(g, 2, vp(ps), ms, 1, vp(o), pp - 2, s), GW(g, 2, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 32, 15 * 32 + 30, s),
        CR(c, 2, vp(ps), ms, 1, r_, g_, b_, pp - 2, s), CR(c, 2, vp(ps), ms, 1, r_, g_, b_, 2 * pp, s),
        CW(c, 2, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 15 * 32 + 30, s), CW(c, 2, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 4096, s),
        GR(g, 2, vp(ps), ms - 1, 1, vp(o), pp, s), GW(g, 2, vp(ps), ms - 1, 1, 0, 0, 16, 16, vp(o), 32, 4096, s),
        CR(c, 1, vp(ps), ms - 1, 1, r_, g_, b_, 0, s), CW(c, 1, vp(ps), ms - 1, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 0, s),
        # the 8-bit layouts on a deep RGB context
        IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB24, 48)), 0, s), IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_PLANAR3, 16, 4096)), 0, s),
        IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGBA32, 64)), 0, s), IR(c, 1, vp(ps), ms, 1, C.byref(img(pa.LAYOUT_RGB24, 3 * W)), 0, s),
        IR(c, 1, vp(ps), ms, 1, C.byref(img(pa.LAYOUT_BGRA32, 4 * W)), 0, s),
        # the 16-bit layouts' own rules there
        IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 94)), 0, s), IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 97)), 0, s),
        IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGBA64, 128, data=o + 1)), 0, s),
        IW(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_PLANAR3_16, 32, 15 * 32 + 30)), 0, s),
        IW(c, 2, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 96)), 15 * 96 + 94, s), IW(c, 22, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 96)), 4096, s),
        IR(c, 1, vp(ps), ms, wl, C.byref(img(pa.LAYOUT_RGB48, 6 * W)), 0, s), IR(c, 1, vp(ps), ms - 1, 1, C.byref(img(pa.LAYOUT_RGB48, 6 * W)), 0, s),
        # the 16-bit layouts on 8-bit, deep grey and 8-bit RGB contexts
        IW(g8.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 96)), 0, s), IW(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 96)), 0, s),
        IW(c8.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGB48, 96)), 0, s), IW(c8.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_RGBA64, 128)), 0, s),
        IW(c8.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, C.byref(img(pa.LAYOUT_PLANAR3_16, 32, 4096)), 0, s),
        IR(c8.h, 1, vp(ps), ms, 1, C.byref(img(pa.LAYOUT_RGBA64, 8 * W)), 0, s), IR(g, 1, vp(ps), ms, 1, C.byref(img(pa.LAYOUT_PLANAR3_16, 2 * W, 2 * W * H)), 0, s),
        IR(g8.h, 1, vp(ps), ms, 1, C.byref(img(pa.LAYOUT_RGB48, 6 * W)), 0, s),
        # the uint8_t proxy calls stay refused on deep contexts
        L.picsong_decode_frames_reduced(g, 1, vp(ps), ms, 1, vp(o), 0, s), L.picsong_decode_frames_window(g, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 16, 0, s),
        L.picsong_decode_frame_reduced(g, vp(ps), 1, vp(o), s), L.picsong_decode_frame_window(g, vp(ps), 1, 0, 0, 16, 16, vp(o), 16, s),
        L.picsong_decode_rgb_frames_reduced(c, 1, vp(ps), ms, 1, r_, g_, b_, 0, s),
        L.picsong_decode_rgb_frames_window(c, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 16, 0, s),
        L.picsong_decode_rgb_frame_reduced(c, vp(ps), ms, 1, r_, g_, b_, s), L.picsong_decode_rgb_frame_window(c, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 16, s),
    ):
        refused(rc)
    refused(GR(g16cp3.h, 1, vp(ps), ms, 1, vp(o), 0, s), b"-cp 3")
    refused(GW(g16cp3.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, vp(o), 32, 0, s), b"-cp 3")
    refused(CR(c16cp3.h, 1, vp(ps), ms, 1, r_, g_, b_, 0, s), b"-cp 3")
    refused(CW(c16cp3.h, 1, vp(ps), ms, 1, 0, 0, 16, 16, rw, gw_, bw, 32, 0, s), b"-cp 3")
    # geometry only: they answer on deep contexts
    d = [C.c_int() for _ in range(5)]
    for h in (g, c):
        assert L.picsong_reduced_dims(h, 1, *[C.byref(x) for x in d]) == 0 and (d[2].value, d[3].value) == (AW >> 1, AH >> 1)
        assert L.picsong_window_codeblocks(h, 1, 0, 0, 16, 16, C.byref(d[4])) == 0 and d[4].value >= 1
    torch.cuda.synchronize()
    assert bool((out == BS).all().item()) and bool((st == 0x5A5A).all().item()), "a refused call wrote something"
    for x in (g16, c16, g8, c8, g16cp3, c16cp3):
        x.close()
