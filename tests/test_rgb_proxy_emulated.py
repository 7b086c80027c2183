"""Colour proxies on the CPU wave emulator (tests/hipemu/emu_rgb_proxy_driver.cpp): the launch sequences of
picsong_decode_rgb_frames_reduced / _window and picsong_decode_rgb_images_reduced / _window -- n RGB frames at 1/2^r, or a
window of them, every stage ONE launch over 3 n planes -- and the epilogue kernel that stores the window in the caller's
pixel layout, against the oracle; the argument checks through the shared functions.

Frame f's component c is oracle.gen_frame(W, H, 60 + 3 f + c) and the three tables are the shipped R / G / B files, so a
swapped frame / component index, a wrong table or a wrong stride shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import layout_ref as lr
import oracle_lib as orc
import reduced_ref as rr
from emu_lib import _geo, _p, aligned_zeros, driver_lib

_lib = None
ULL = C.c_ulonglong
SENTINEL = 0xA5
W, H, WL, N = 192, 128, 3, 2
# (lossy, qs, k)
MODES = [(False, 1.0, 0.0), (True, 0.5, 0.0), (False, 1.0, 0.5)]
MODE_IDS = ["53", "97", "53-k0.5"]
COLOUR = (lr.PLANAR3, lr.RGB24, lr.BGR24, lr.RGBA32, lr.BGRA32)


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_rgb_proxy.so", ("emu_rgb_proxy_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
    return _lib


def _max_stream(AW, AH):
    return 9 + 2 * (AW // 64) * (AH // 64) + AW * AH + 1


@functools.lru_cache(maxsize=None)
def _luts(lossy, k):
    return tuple(orc.lut_for_component(lossy, WL, c, k=k) for c in range(3))


@functools.lru_cache(maxsize=None)
def _streams(lossy, qs, k):
    """(the 3 N oracle streams, the same in one array max_stream shorts apart)"""
    out = []
    for f in range(N):
        comps = orc.rgb_forward(*[orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + c)) for c in range(3)], lossy)
        out += [orc.encode_plane(comps[c], WL, lossy, qs, _luts(lossy, k)[c], None, k=k) for c in range(3)]
    AH, AW = comps[0].shape
    stride = _max_stream(AW, AH)
    flat = np.zeros(3 * N * stride, np.uint16)
    for z, s in enumerate(out):
        flat[z * stride:z * stride + s.size] = s
    return tuple(out), flat, AW, AH


@functools.lru_cache(maxsize=None)
def _want(lossy, qs, k, r):
    """[f][c]: the oracle's plane of frame f at 1/2^r, (AH >> r, AW >> r) uint8"""
    streams, _, AW, AH = _streams(lossy, qs, k)
    return [[np.asarray(p, np.uint8).reshape(AH >> r, AW >> r)
             for p in rr.reduced_rgb(streams[3 * f:3 * f + 3], AW, AH, WL, lossy, qs, _luts(lossy, k), r, k)] for f in range(N)]


def _tables(lossy, k):
    luts = _luts(lossy, k)
    return [np.ascontiguousarray(t.table, np.int32) for t in luts], _geo(luts[0]), int(luts[0].n_tables)


def _reduced(lossy, qs, k, r, fuse=1, offset=0, gap=0):
    """the reduced call into R, G, B back to back per frame, `offset` bytes off alignment, `gap` bytes between frames"""
    _, flat, AW, AH = _streams(lossy, qs, k)
    pp = (AW >> r) * (AH >> r)
    fs = 3 * pp + gap
    buf = aligned_zeros(N * fs + offset + 16, np.uint8)
    buf[:] = SENTINEL
    out = buf[offset:]
    tabs, geo, nt = _tables(lossy, k)
    flag = np.zeros(1, np.int32)
    rc = lib().emu_rgbp_decode_reduced(N, _p(flat), ULL(_max_stream(AW, AH)), r, _p(out), _p(out[pp:]), _p(out[2 * pp:]), ULL(fs), AW, AH, WL,
                                       int(lossy), C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(geo), C.c_float(k), nt, fuse, _p(flag))
    assert rc >= 0 and not rc & 8 and flag[0] == 0
    return rc, buf, fs, pp


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("lossy,qs,k", MODES, ids=MODE_IDS)
def test_reduced_frames_equal_the_oracle(lossy, qs, k, r):
    """decode_rgb_frames_reduced with n = 2: the fused tail (grid.z = frame) where the plan has it, and the separate inverse
    colour transform -- asked for, and forced by planes one byte off -- give the oracle's planes and touch nothing else."""
    want = _want(lossy, qs, k, r)
    lib().emu_rgbp_reset()
    rc, buf, fs, pp = _reduced(lossy, qs, k, r)
    fused_launches = lib().emu_rgbp_launches()
    for fuse, offset, gap in [(1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 4)]:
        if (fuse, offset, gap) != (1, 0, 0):
            lib().emu_rgbp_reset()
            rc2, buf, fs, pp = _reduced(lossy, qs, k, r, fuse, offset, gap)
            assert (rc2 & 1) == (rc & 1 if (fuse and not offset) else 0)
            if not rc2 & 1 and rc & 1:
                assert lib().emu_rgbp_launches() > fused_launches              # (a level and one transform a frame for the tail)
        expect = np.full(buf.size, SENTINEL, np.uint8)
        for f in range(N):
            for c in range(3):
                at = offset + f * fs + c * pp
                expect[at:at + pp] = want[f][c].ravel()
        assert np.array_equal(buf, expect), (fuse, offset, gap)


def _windows(AW, AH, r):
    paw, pah = AW >> r, AH >> r
    return [(0, 0, paw, pah), (1, 2, 33, 21), (paw - 5, pah - 3, 5, 3)]


def _window(lossy, qs, k, r, win, layout, offset, pitch_pad, gap):
    """the window call in `layout` into a sentinel-filled buffer; returns (rc, buffer, expected buffer)"""
    streams, flat, AW, AH = _streams(lossy, qs, k)
    x, y, w, h = win
    bpp = lr.BPP[layout]
    pitch = w * bpp + pitch_pad
    plane = lr.plane_span(layout, w, h, pitch)
    ps = plane + 3 if layout == lr.PLANAR3 else 0
    span = lr.frame_span(layout, w, h, pitch, ps)
    fs = span + gap
    buf = aligned_zeros(offset + N * fs + 16, np.uint8)
    buf[:] = SENTINEL
    out = buf[offset:]
    tabs, geo, nt = _tables(lossy, k)
    flag = np.zeros(1, np.int32)
    rc = lib().emu_rgbp_decode_window(N, _p(flat), ULL(_max_stream(AW, AH)), r, x, y, w, h, layout, _p(out), _p(out[ps:]), _p(out[2 * ps:]),
                                      ULL(pitch), ULL(fs), AW, AH, WL, int(lossy), C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]),
                                      _p(geo), C.c_float(k), nt, _p(flag))
    assert rc >= 0 and not rc & 8 and flag[0] == 0
    expect = np.full(buf.size, SENTINEL, np.uint8)
    want = _want(lossy, qs, k, r)
    for f in range(N):
        crop = [p[y:y + h, x:x + w] for p in want[f]]
        at = offset + f * fs
        expect[at:at + span] = lr.pack(crop, layout, pitch, ps, alpha=255, fill=SENTINEL)
    return rc, buf, expect


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("lossy,qs,k", MODES, ids=MODE_IDS)
def test_window_frames_equal_the_oracles_crop(lossy, qs, k, r):
    """decode_rgb_frames_window with n = 2 (the decoder over the rectangle table of 6 planes, run_window with frames = 6, the
    epilogue with grid.z = frame into three planes): the whole image, an odd window and the bottom-right corner; only the
    window's bytes are written."""
    _, _, AW, AH = _streams(lossy, qs, k)
    for win in _windows(AW, AH, r):
        rc, buf, expect = _window(lossy, qs, k, r, win, lr.PLANAR3, 0, 0, 0)
        assert np.array_equal(buf, expect), win
    # the planes at an odd address, a pitch gap and a gap between frames: the per-byte form
    rc, buf, expect = _window(lossy, qs, k, r, (1, 2, 33, 21), lr.PLANAR3, 1, 6, 5)
    assert not rc & 1
    assert np.array_equal(buf, expect)


@pytest.mark.parametrize("layout", COLOUR, ids=[lr.NAMES[l] for l in COLOUR])
@pytest.mark.parametrize("lossy,qs,k", MODES[:2], ids=MODE_IDS[:2])
def test_every_layout_at_an_aligned_and_an_odd_destination(lossy, qs, k, layout):
    """the epilogue's vector form (destination, pitch and frame stride multiples of 16 / of 4) and its per-byte form (an odd
    offset; an odd pitch) store the same pixels: the oracle's crop packed by layout_ref, alpha 255, the sentinel everywhere
    else.  w = 33: eight whole groups and a ragged tail of one pixel a row."""
    r, win = 1, (1, 2, 33, 21)
    bpp = lr.BPP[layout]
    pad16 = (-33 * bpp) % 16
    for offset, pitch_pad, gap, vec in [(0, pad16, 16 + (-(20 * (33 * bpp + pad16) + 33 * bpp)) % 16, True), (0, pad16 + 4, 0, None),
                                        (3, pad16, 0, False), (0, 7, 0, False)]:
        if layout == lr.PLANAR3 and vec:
            continue                                       # (PLANAR3's aligned case: below, with an aligned plane stride)
        rc, buf, expect = _window(lossy, qs, k, r, win, layout, offset, pitch_pad, gap)
        if vec is not None and layout != lr.PLANAR3:
            assert bool(rc & 1) == vec, (offset, pitch_pad, gap)
        assert np.array_equal(buf, expect), (offset, pitch_pad, gap)
    # the whole reduced image (w a multiple of 4: dwordx4 loads, no tail), packed rows
    _, _, AW, AH = _streams(lossy, qs, k)
    rc, buf, expect = _window(lossy, qs, k, 2, (0, 0, AW >> 2, AH >> 2), layout, 0, 0, 0)
    assert np.array_equal(buf, expect)


def test_planar_vector_form():
    """PLANAR3 with planes, pitch and frame stride 4-byte aligned takes the dword stores"""
    lossy, qs, k = False, 1.0, 0.0
    streams, flat, AW, AH = _streams(lossy, qs, k)
    x, y, w, h = 1, 2, 33, 21
    pitch, ps = 36, 36 * 21
    fs = 3 * ps + 4
    buf = aligned_zeros(N * fs + 16, np.uint8)
    buf[:] = SENTINEL
    tabs, geo, nt = _tables(lossy, k)
    flag = np.zeros(1, np.int32)
    rc = lib().emu_rgbp_decode_window(N, _p(flat), ULL(_max_stream(AW, AH)), 1, x, y, w, h, lr.PLANAR3, _p(buf), _p(buf[ps:]), _p(buf[2 * ps:]),
                                      ULL(pitch), ULL(fs), AW, AH, WL, 0, C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(geo),
                                      C.c_float(k), nt, _p(flag))
    assert rc == 1
    expect = np.full(buf.size, SENTINEL, np.uint8)
    for f in range(N):
        for c in range(3):
            rows = np.lib.stride_tricks.as_strided(expect[f * fs + c * ps:], (h, w), (pitch, 1))
            rows[...] = _want(lossy, qs, k, 1)[f][c][y:y + h, x:x + w]
    assert np.array_equal(buf, expect)


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("lossy,qs,k", MODES[:2], ids=MODE_IDS[:2])
def test_reduced_images_through_the_reduced_sequence_and_one_emit(lossy, qs, k, r):
    """decode_rgb_images_reduced (192 >> r is a multiple of 16: the reduced sequence into aligned planes + emit_frames with the
    geometry (rw, rh, paw, pah)): the visible pixels of both frames in every layout, aligned and odd, equal the oracle's and
    what the window (0, 0, rw, rh) stores."""
    _, flat, AW, AH = _streams(lossy, qs, k)
    rw, rh = rr.visible(W, H, r)
    tabs, geo, nt = _tables(lossy, k)
    want = _want(lossy, qs, k, r)
    for layout in COLOUR:
        bpp = lr.BPP[layout]
        for offset, pitch_pad in [(0, (-rw * bpp) % 16), (1, 7)]:
            pitch = rw * bpp + pitch_pad
            plane = lr.plane_span(layout, rw, rh, pitch)
            ps = 0 if layout != lr.PLANAR3 else (plane + 15) // 16 * 16 if not offset else plane + 3
            span = lr.frame_span(layout, rw, rh, pitch, ps)
            fs = (span + 15) // 16 * 16 if not offset else span + 5
            buf = aligned_zeros(offset + N * fs + 16, np.uint8)
            buf[:] = SENTINEL
            flag = np.zeros(1, np.int32)
            rc = lib().emu_rgbp_images_reduced(N, _p(flat), ULL(_max_stream(AW, AH)), r, rw, rh, layout, _p(buf[offset:]), ULL(pitch), ULL(ps),
                                               ULL(fs), AW, AH, WL, int(lossy), C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(geo),
                                               C.c_float(k), nt, 1, _p(flag))
            assert rc == 0 and flag[0] == 0
            expect = np.full(buf.size, SENTINEL, np.uint8)
            for f in range(N):
                at = offset + f * fs
                expect[at:at + span] = lr.pack([p[:rh, :rw] for p in want[f]], layout, pitch, ps, alpha=255, fill=SENTINEL)
            assert np.array_equal(buf, expect), (layout, offset)
            if layout != lr.PLANAR3:                       # (the window route packs the same bytes: _window's plane stride differs)
                _, wbuf, wexpect = _window(lossy, qs, k, r, (0, 0, rw, rh), layout, offset, pitch_pad, fs - span)
                assert np.array_equal(wbuf, wexpect) and np.array_equal(wbuf[:buf.size], buf[:wbuf.size])


# ---- the argument checks, through the shared functions -------------------------------------------------------------------
def _refusal(fn, *args):
    """"" when the arguments pass, else the shared function's message"""
    msg = C.create_string_buffer(256)
    return (msg.value.decode() or "refused") if fn(*args, msg, len(msg)) else ""


def test_refusals():
    AW, AH, wl = 192, 128, 3
    ms = _max_stream(AW, AH)
    base = 1 << 20
    vp = C.c_void_p

    def red(ctx_rgb=1, cp=2, same=1, n=2, planes=None, null=None, st=base, fs=None, stride=ms, reduce=1):
        rc = max(0, min(reduce, wl - 1))
        pp = (AW >> rc) * (AH >> rc)
        fs = 3 * pp if fs is None else fs
        p = list(planes or (base, base + pp, base + 2 * pp))           # R, G, B back to back per frame
        if null is not None:
            p[null] = None
        return _refusal(lib().emu_rgbp_reduced_refusal, ctx_rgb, cp, same, n, vp(p[0]), vp(p[1]), vp(p[2]), vp(st), ULL(fs), ULL(stride), AW, AH,
                        wl, reduce)

    pp = (AW >> 1) * (AH >> 1)
    assert red() == "" and red(n=1, fs=0) == "" and red(n=21) == "" and red(reduce=0) == "" and red(reduce=2) == ""
    for kw in [dict(ctx_rgb=0), dict(cp=3), dict(same=0), dict(n=0), dict(n=22), dict(null=0), dict(null=1), dict(null=2), dict(st=None),
               dict(stride=ms - 1), dict(reduce=-1), dict(reduce=3), dict(fs=pp - 1), dict(fs=pp), dict(fs=3 * pp - 1)]:
        assert red(**kw) != "", kw
    # three separate arrays of n planes: frame_stride = a plane
    assert red(planes=(base, base + 2 * pp, base + 4 * pp), fs=pp) == ""

    def win(ctx_rgb=1, cp=2, same=1, n=2, r_=base, st=base, pitch=40, fs=None, stride=ms, reduce=1, x=1, y=2, w=33, h=21, null=None):
        span = (h - 1) * pitch + w
        fs = 3 * span if fs is None else fs
        p = [r_, r_ + span, r_ + 2 * span]
        if null is not None:
            p[null] = None
        return _refusal(lib().emu_rgbp_window_refusal, ctx_rgb, cp, same, n, vp(p[0]), vp(p[1]), vp(p[2]), vp(st), ULL(pitch), ULL(fs),
                        ULL(stride), AW, AH, wl, reduce, x, y, w, h)

    span = 20 * 40 + 33
    assert win() == "" and win(n=1, fs=0) == "" and win(pitch=33) == "" and win(x=96 - 33, y=64 - 21) == ""
    for kw in [dict(ctx_rgb=0), dict(cp=3), dict(same=0), dict(n=0), dict(n=22), dict(null=0), dict(null=1), dict(null=2), dict(st=None),
               dict(stride=ms - 1), dict(reduce=-1), dict(reduce=3), dict(w=0), dict(h=0), dict(x=-1), dict(y=-1), dict(x=96 - 32),
               dict(y=64 - 20), dict(pitch=32), dict(fs=span - 1), dict(fs=span), dict(fs=3 * span - 1)]:
        assert win(**kw) != "", kw

    def img(ctx_rgb=1, cp=2, same=1, n=2, st=base, stride=ms, reduce=1, x=1, y=2, w=33, h=21, layout=lr.RGB24, data=base, pitch=None, ps=0,
            fs=None):
        pitch = w * lr.BPP.get(layout, 3) + 1 if pitch is None else pitch
        if layout == lr.PLANAR3 and ps == 0:
            ps = h * pitch
        fs = (h * pitch + 2 * ps) if fs is None else fs
        return _refusal(lib().emu_rgbp_images_refusal, ctx_rgb, cp, same, n, vp(st), ULL(stride), AW, AH, wl, reduce, x, y, w, h, layout,
                        vp(data), ULL(pitch), ULL(ps), ULL(fs))

    for layout in COLOUR:
        assert img(layout=layout) == "", layout
    assert img(n=1, fs=0) == "" and img(n=21) == ""
    for kw in [dict(ctx_rgb=0), dict(cp=3), dict(same=0), dict(n=0), dict(n=22), dict(st=None), dict(data=None), dict(stride=ms - 1),
               dict(reduce=-1), dict(reduce=3), dict(w=0), dict(x=96 - 32), dict(layout=lr.GREY8), dict(layout=6), dict(layout=-1),
               dict(pitch=3 * 33 - 1), dict(layout=lr.RGBA32, pitch=4 * 33 - 1), dict(layout=lr.PLANAR3, ps=20 * 34 + 32),
               dict(fs=20 * 100 + 98), dict(layout=lr.PLANAR3, fs=3 * 21 * 34 - 2)]:
        assert img(**kw) != "", kw
