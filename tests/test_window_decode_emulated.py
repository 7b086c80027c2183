"""The window decode on the CPU wave emulator (tests/hipemu/emu_window_driver.cpp): the decoder over the window's
codeblock table and the cone's synthesis (dwt_window_kernel), against the oracle's crop of LL_r."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
import reduced_ref as rr
import window_ref as wr
from emu_lib import _geo, _p, driver_lib

FILL = 0x3A5A5A5A
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_window.so", ("emu_window_driver.cpp", "emu_runtime.cpp"))
    return _lib


def plan(AW, AH, wl, lossy, r, x, y, w, h):
    """(distinct codeblocks, rectangles [(x0, y0, x1, y1)], listed codeblocks, waves, waves cap) of window_plan."""
    rects = np.zeros(4 * 22, np.int32)
    n = np.zeros(4, np.int32)
    ncb = lib().emu_window_plan(AW, AH, wl, int(lossy), r, x, y, w, h, _p(rects), _p(n))
    return ncb, [tuple(rects[4 * i:4 * i + 4]) for i in range(n[0])], int(n[1]), int(n[2]), int(n[3])


def decode_window(stream, AW, AH, wl, lossy, qs, lut, r, x, y, w, h, k=0.0, staging=False, misalign=0, pad=5,
                  seed=0):
    """Returns (window (h, w), flags, range flag, decoder output (AH, AW)); the coefficient array starts random."""
    stream = np.ascontiguousarray(stream, np.uint16)
    rng = np.random.default_rng(seed)
    coef = rng.integers(-(1 << 20), 1 << 20, (AH, AW), dtype=np.int32)
    coef[::7, ::5] = FILL
    before = coef.copy()
    pitch = w + pad
    n = (h - 1) * pitch + w
    buf = np.full(n + 128 + misalign, 0xA5, np.uint8)
    flag = np.zeros(1, np.int32)
    tab = np.ascontiguousarray(lut.table, np.int32)
    res = lib().emu_decode_window(_p(stream), int(stream.size), AW, AH, wl, int(lossy), C.c_float(qs), _p(tab),
                                  _p(_geo(lut)), C.c_float(k), int(lut.n_tables), int(staging), r, x, y, w, h, _p(coef),
                                  C.c_void_p(buf.ctypes.data + misalign), C.c_size_t(pitch), _p(flag), 1, C.c_size_t(0))
    full = np.full((h, pitch), 0xA5, np.uint8).reshape(-1)[:n].copy()
    got = buf[misalign:misalign + n]
    mask = np.zeros(n, bool)
    for i in range(h):
        mask[i * pitch:i * pitch + w] = True
    assert np.all(got[~mask] == 0xA5) and np.all(buf[:misalign] == 0xA5) and np.all(buf[misalign + n:] == 0xA5), \
        "bytes written outside the window"
    del full
    win = np.stack([got[i * pitch:i * pitch + w] for i in range(h)])
    return win, res, int(flag[0]), coef, before


def _stream(W, H, wl, lossy, qs, k, seed=0):
    lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
    img = orc.gen_frame(W, H, seed)
    return orc.encode_frame(img, wl, lossy, qs, lut, k=k), lut


def _written_cbs(coef, before, AW, AH):
    d = (coef != before).reshape(AH // 64, 64, AW // 64, 64).any(axis=(1, 3))
    return {(int(cx), int(cy)) for cy, cx in zip(*np.nonzero(d))}


@pytest.mark.parametrize("AW,AH,wl,lossy", [(704, 512, 5, False), (704, 512, 6, True), (1024, 320, 4, True),
                                            (7680, 4352, 5, False), (16384, 16384, 7, True), (832, 320, 4, False)])
def test_rule_matches_plan(AW, AH, wl, lossy):
    """The library's plan lists exactly the rule's codeblocks; the whole padded reduced image is the reduced corner."""
    rng = np.random.default_rng(AW + wl)
    for r in range(wl):
        paw, pah = AW >> r, AH >> r
        ws = wr.windows(paw, pah)
        for _ in range(6):
            x, y = int(rng.integers(0, paw)), int(rng.integers(0, pah))
            ws.append((x, y, int(rng.integers(1, paw - x + 1)), int(rng.integers(1, pah - y + 1))))
        for (x, y, w, h) in ws:
            want = wr.window_codeblocks(AW, AH, wl, lossy, r, x, y, w, h)
            ncb, rects, listed, waves, cap = plan(AW, AH, wl, lossy, r, x, y, w, h)
            got = set()
            for (x0, y0, x1, y1) in rects:
                got |= {(cx, cy) for cy in range(y0, y1) for cx in range(x0, x1)}
            assert got == want and ncb == len(want), (r, x, y, w, h)
            assert len(rects) == 3 * (wl - r) + 1 and listed >= ncb and waves == (listed + 1) // 2 and waves <= cap
        ncb, _, _, _, _ = plan(AW, AH, wl, lossy, r, 0, 0, paw, pah)
        assert ncb == -(-paw // 64) * -(-pah // 64)


def test_window_ok():
    f = lib().emu_window_ok
    assert f(100, 50, 0, 0, 100, 50) == 1 and f(100, 50, 99, 49, 1, 1) == 1
    assert [f(100, 50, *a) for a in [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (99, 0, 2, 1),
                                     (0, 49, 1, 2), (2**31 - 2, 0, 5, 1)]] == [0] * 7


CASES = [(704, 512, 5, False, 1.0, 0.0), (704, 512, 6, True, 0.5, 0.0), (704, 512, 6, True, 0.3, 0.0),
         (576, 320, 3, False, 1.0, 0.5)]


@pytest.mark.parametrize("W,H,wl,lossy,qs,k", CASES)
def test_window_matches_oracle(W, H, wl, lossy, qs, k):
    stream, lut = _stream(W, H, wl, lossy, qs, k)
    for r in range(wl):
        full = rr.reduced_pixels(stream, W, H, wl, lossy, qs, lut, r, k=k)
        pah, paw = full.shape
        ws = wr.windows(paw, pah, W, H)
        # crossing a coarse level's straddling codeblocks: around the middle of LL_r's subband boundary
        ws.append((max(0, paw // 2 - 3), max(0, pah // 2 - 2), min(7, paw - max(0, paw // 2 - 3)), min(5, pah - max(0, pah // 2 - 2))))
        for i, (x, y, w, h) in enumerate(ws):
            got, res, flag, coef, before = decode_window(stream, W, H, wl, lossy, qs, lut, r, x, y, w, h, k=k,
                                                         misalign=i % 4, seed=i)
            assert flag == 0 and not res & 8
            assert np.array_equal(got, full[y:y + h, x:x + w]), (r, x, y, w, h)
            want = wr.window_codeblocks(W, H, wl, lossy, r, x, y, w, h)
            assert _written_cbs(coef, before, W, H) <= want, (r, x, y, w, h)


def test_window_staging_form():
    W, H, wl = 704, 512, 4
    stream, lut = _stream(W, H, wl, True, 0.5, 0.0)
    for r in (0, 2):
        full = rr.reduced_pixels(stream, W, H, wl, True, 0.5, lut, r)
        pah, paw = full.shape
        for (x, y, w, h) in [(0, 0, 40, 30), (paw - 33, pah - 9, 33, 9), (paw // 3, pah // 3, 21, 13)]:
            got, _, flag, _, _ = decode_window(stream, W, H, wl, True, 0.5, lut, r, x, y, w, h, staging=True)
            assert flag == 0 and np.array_equal(got, full[y:y + h, x:x + w]), (r, x, y, w, h)


@pytest.mark.parametrize("k", [0.0, 0.5])
def test_window_decoder_touches_only_the_set(k):
    """A codeblock just outside the rule's set whose MSB is out of range is never looked at: range flag clear, pixels
    those of the clean stream, no coefficient outside the set written.  The same damage inside raises the flag."""
    W, H, wl, r = 704, 512, 4, 0
    stream, lut = _stream(W, H, wl, False, 1.0, k)
    x, y, w, h = 300, 200, 40, 30
    want_cbs = wr.window_codeblocks(W, H, wl, False, r, x, y, w, h)
    ncx, ncy = W // 64, H // 64
    outside = [(cx, cy) for cy in range(ncy) for cx in range(ncx) if (cx, cy) not in want_cbs
               and any((cx + dx, cy + dy) in want_cbs for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))]
    assert outside
    want = wr.window_pixels(stream, W, H, wl, False, 1.0, lut, r, x, y, w, h, k=k)
    cx, cy = outside[0]
    bad = stream.copy()
    bad[9 + 2 * (cy * ncx + cx)] = 20
    got, _, flag, coef, before = decode_window(bad, W, H, wl, False, 1.0, lut, r, x, y, w, h, k=k)
    assert flag == 0 and np.array_equal(got, want)
    assert _written_cbs(coef, before, W, H) <= want_cbs
    cx, cy = sorted(want_cbs)[len(want_cbs) // 2]
    bad = stream.copy()
    bad[9 + 2 * (cy * ncx + cx)] = 20
    _, _, flag, _, _ = decode_window(bad, W, H, wl, False, 1.0, lut, r, x, y, w, h, k=k)
    assert flag == 1


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_window_two_grey_frames(lossy, qs):
    """picsong_decode_frames_window's n = 2 path through the library's sequence, on the smallest frame of the reduced
    tests (9 codeblock columns) at r = 1, a window that crosses codeblock boundaries in both directions: each frame's
    window against the oracle's crop, no byte outside the windows written, and the launches counted -- the intake (1),
    the decoder (1), a level of the cone a launch (wl - r), whatever n."""
    W, H, wl, r, n = 576, 320, 3, 1, 2
    x, y, w, h = 50, 50, 40, 30
    pairs = [_stream(W, H, wl, lossy, qs, 0.0, seed=s) for s in range(n)]
    lut = pairs[0][1]
    stride = max(p[0].size for p in pairs)
    streams = np.zeros((n, stride), np.uint16)
    for i, p in enumerate(pairs):
        streams[i, :p[0].size] = p[0]
    cbs = wr.window_codeblocks(W, H, wl, lossy, r, x, y, w, h)
    assert len({cx for cx, _ in cbs}) > 1 and len({cy for _, cy in cbs}) > 1
    pitch = w + 5
    span = (h - 1) * pitch + w
    fs = span + 7
    coef = np.full((n, H, W), FILL, np.int32)
    buf = np.full(n * fs + 64, 0xA5, np.uint8)
    flag = np.zeros(1, np.int32)
    tab = np.ascontiguousarray(lut.table, np.int32)
    lib().emu_window_reset()
    res = lib().emu_decode_window(_p(streams), stride, W, H, wl, int(lossy), C.c_float(qs), _p(tab), _p(_geo(lut)), C.c_float(0.0),
                                  int(lut.n_tables), 0, r, x, y, w, h, _p(coef), _p(buf), C.c_size_t(pitch), _p(flag), n,
                                  C.c_size_t(fs))
    assert res == 0 and flag[0] == 0
    expect = np.full(buf.size, 0xA5, np.uint8)
    for f in range(n):
        full = rr.reduced_pixels(pairs[f][0], W, H, wl, lossy, qs, lut, r)
        for i in range(h):
            expect[f * fs + i * pitch:f * fs + i * pitch + w] = full[y + i, x:x + w]
    assert np.array_equal(buf, expect)
    for f in range(n):
        written = (coef[f] != FILL).reshape(H // 64, 64, W // 64, 64).any(axis=(1, 3))
        assert {(int(cx), int(cy)) for cy, cx in zip(*np.nonzero(written))} <= cbs
    assert lib().emu_window_launches() == 2 + (wl - r)
