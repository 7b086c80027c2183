"""The reduced-quality decode (picsong_ctx_set_decode_drop) on the CPU wave emulator (tests/hipemu/emu_drop_driver.cpp):
the library's own sequences with BpcArgs::drop set, byte for byte / coefficient for coefficient against drop_ref -- the
oracle's full decode truncated in numpy by the rule d(cb) = max(0, drop - level(cb)), midpoint reconstruction.

The driver's context poisons the plane scratch (0xDEADBEEF) and the tests poison the coefficient arrays: a result equal to
the expected one read no plane the decoder did not write, and wrote no codeblock outside the launch."""
import ctypes as C
import functools

import numpy as np
import pytest

import drop_ref as dr
import oracle_lib as orc
import reduced_ref as rr
from emu_lib import _geo, _p, driver_lib

_lib = None
POISON = 0x7A5A5A5A
ULL = C.c_ulonglong


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_drop.so", ("emu_drop_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
    return _lib


# ---- the rule ------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(704, 512), (576, 320), (832, 320)]


def test_drop_planes_rule_matches_the_reference_and_the_kernels_subband_search():
    """drop_planes_of (picsong_drop_planes' rule) against drop_ref.drop_planes, and the level under it against the kernels'
    own find_subband at the codeblock's corner and the oracle's, for every codeblock of the three geometries, wl 1..5."""
    lv, sb = C.c_int(), C.c_int()
    for AW, AH in GEOMETRIES:
        for wl in range(1, 6):
            for cb in range((AW // 64) * (AH // 64)):
                level = dr.cb_level(AW, AH, wl, cb)
                assert lib().emu_drop_kernel_level(AW, AH, wl, cb) == level, (AW, AH, wl, cb)
                orc.lib().po_find_subband((cb % (AW // 64)) * 64, (cb // (AW // 64)) * 64, AW, AH, wl, C.byref(lv), C.byref(sb))
                assert lv.value == level, (AW, AH, wl, cb)
                for drop in (0, 1, 2, 3, wl, wl + 1, 9, 15):
                    assert lib().emu_drop_planes(AW, AH, wl, drop, cb) == dr.drop_planes(AW, AH, wl, drop, cb) == max(0, drop - level)
    assert [lib().emu_drop_ok(d) for d in (-1, 0, 15, 16)] == [0, 1, 1, 0]
    # 704 wide, wl 3: AW >> 1 = 352 is no multiple of 64 -- codeblock column 5 straddles LL1 | HL0 and takes its corner's level
    assert dr.cb_level(704, 512, 3, 5) == 1 and dr.cb_level(704, 512, 3, 6) == 0


def test_selector_keeps_its_choice_without_drop():
    """select_decoder(.., drop = false) is select_decoder(..) -- the function pointer, grid and scratch -- for the three
    k = 0 forms, -k > 0 and -cp 3; drop = true gives three other kernels on the same grid and scratch, and refuses -k > 0
    and -cp 3."""
    for waves in (1, 4, 23):
        assert lib().emu_drop_selector(waves) == 0b0111_0111_0011_0111, waves


# ---- coefficients --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep():
    W, H, wl = 576, 320, 3
    lut = orc.lut_for(False, wl)
    coef = orc.deep_coeffs(W, H, 5, raw_cb=7)
    st, sz = orc.bpc_encode(coef, wl, lut)
    assert np.array_equal(orc.bpc_decode(st, sz, W, H, wl, lut), coef), "the fixture round-trips"
    assert sz[7] == 4096, "codeblock 7 is raw"
    msbs = {int(st[cb * 4096]) for cb in range(sz.size) if sz[cb] != 4096}
    assert {8, 12, 15} <= msbs, msbs
    stream = orc.bitstream_pack(st, sz)
    return W, H, wl, lut, coef, st, sz, stream


@pytest.mark.parametrize("drop", [1, 3, 4, 9, 15])
@pytest.mark.parametrize("form", ["staging", "stream"])
def test_deep_coefficients(drop, form):
    """MSBs 8, 12 and 15 (the sixteen-plane epilogue), a raw codeblock (copied whole), and at drop 9 / 15 codeblocks with
    MSB < d (all zero, no plane iteration) beside ones that decode partially."""
    W, H, wl, lut, coef, st, sz, stream = _deep()
    want = dr.truncate(coef, sz, W, H, wl, drop)
    ds = [dr.drop_planes(W, H, wl, drop, cb) for cb in range(sz.size)]
    assert np.array_equal(want[0:64, 448:512], coef[0:64, 448:512]), "the raw codeblock (7: row 0, column 7) stays whole"
    if drop >= 9:
        assert any(int(st[cb * 4096]) < ds[cb] for cb in range(sz.size) if sz[cb] != 4096), "a codeblock with MSB < d"
    got = np.full((H, W), POISON, np.int32)
    flag = np.zeros(1, np.int32)
    tab, geo = np.ascontiguousarray(lut.table, np.int32), _geo(lut)
    if form == "staging":
        rc = lib().emu_drop_decode_coeffs(_p(np.ascontiguousarray(st, np.int32)), _p(np.ascontiguousarray(sz, np.int32)), None, 0, W, H, wl,
                                          _p(tab), _p(geo), drop, _p(got), _p(flag))
    else:
        s = np.ascontiguousarray(stream, np.uint16)
        rc = lib().emu_drop_decode_coeffs(None, None, _p(s), int(s.size), W, H, wl, _p(tab), _p(geo), drop, _p(got), _p(flag))
    assert rc == 0 and flag[0] == 0
    assert np.array_equal(got, want), (drop, form, np.argwhere(got != want)[:4])


def test_deep_coefficients_partial_launch_writes_only_its_codeblocks():
    """A reduced launch (r = 1) under drop: the codeblocks outside the rectangle keep the poison."""
    W, H, wl = 832, 320, 4
    stream, lut = _stream(W, H, wl, False, 1.0)
    _, res, coef = _decode(stream, W, H, wl, False, 1.0, lut, 2, r=1, c16=False)
    ncx, ncy = W // 64, H // 64
    ncx_r, ncy_r = -(-(W >> 1) // 64), -(-(H >> 1) // 64)
    inside = np.zeros((ncy, ncx), bool)
    inside[:ncy_r, :ncx_r] = True
    written = (coef != POISON).reshape(ncy, 64, ncx, 64).any(axis=(1, 3))
    assert not (written & ~inside).any()
    want = dr.drop_coefficients(stream, W, H, wl, lut, 2)
    for cy in range(ncy_r):
        for cx in range(ncx_r):
            assert np.array_equal(coef[cy * 64:cy * 64 + 64, cx * 64:cx * 64 + 64], want[cy * 64:cy * 64 + 64, cx * 64:cx * 64 + 64]), (cx, cy)


# ---- frames --------------------------------------------------------------------------------------------------------------
# 704x512 wl 3: codeblocks straddle subbands; 576x320 wl 3: odd codeblock columns (a wave's halves in two rows); 832x320 wl 4
FRAMES = [(704, 512, 3), (576, 320, 3), (832, 320, 4)]


@functools.lru_cache(maxsize=None)
def _stream(W, H, wl, lossy, qs, seed=0):
    lut = orc.lut_for(lossy, wl)
    return orc.encode_frame(orc.gen_frame(W, H, seed), wl, lossy, qs, lut), lut


def _decode(stream, AW, AH, wl, lossy, qs, lut, drop, r=0, c16=True, win=None, pitch=None):
    """Returns (pixels, flags of emu_drop_decode, the decoder's output (AH, AW) int32)."""
    stream = np.ascontiguousarray(stream, np.uint16)
    coef = np.full((AH, AW), POISON, np.int32)
    x, y, w, h = win if win else (0, 0, AW >> r, AH >> r)
    pitch = pitch if pitch else w
    n = (h - 1) * pitch + w
    buf = np.full(n + 128, 0xA5, np.uint8)
    base = (-buf.ctypes.data) % 64
    flag = np.zeros(1, np.int32)
    tab, geo = np.ascontiguousarray(lut.table, np.int32), _geo(lut)
    res = lib().emu_drop_decode(_p(stream), int(stream.size), AW, AH, wl, int(lossy), C.c_float(qs), _p(tab), _p(geo), int(c16), drop, r,
                                int(win is not None), x, y, w, h, _p(coef), C.c_void_p(buf.ctypes.data + base), C.c_size_t(pitch if win else 0),
                                _p(flag), 1, C.c_size_t(0))
    assert res >= 0 and not res & 8 and flag[0] == 0
    assert np.all(buf[:base] == 0xA5) and np.all(buf[base + n:] == 0xA5), "bytes written outside the image"
    rows = np.lib.stride_tricks.as_strided(buf[base:], (h, w), (pitch, 1))
    if pitch > w:
        gaps = np.lib.stride_tricks.as_strided(buf[base + w:], (h - 1, pitch - w), (pitch, 1))
        assert np.all(gaps == 0xA5), "bytes written between the window's rows"
    return rows.copy(), res, coef


@pytest.mark.parametrize("W,H,wl", FRAMES)
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_frames_match_the_truncated_oracle(W, H, wl, lossy, qs):
    stream, lut = _stream(W, H, wl, lossy, qs)
    coef, sz = dr.full_decode(stream, W, H, wl, lut)
    st, _ = orc.bitstream_unpack(stream, sz.size)
    msb = [int(st[cb * 4096]) if sz[cb] not in (0, 4096) else None for cb in range(sz.size)]
    for drop in (1, 2, wl + 1, 6):
        ds = [dr.drop_planes(W, H, wl, drop, cb) for cb in range(sz.size)]
        if drop == wl + 1:
            assert ds[0] == 1, "the LL codeblock drops a plane"
        if drop == 6 and not lossy:
            zeroed = [cb for cb in range(sz.size) if msb[cb] is not None and msb[cb] < ds[cb]]
            partial = [cb for cb in range(sz.size) if msb[cb] is not None and 0 < ds[cb] <= msb[cb]]
            assert zeroed and partial, "level-0 codeblocks become all-zero while others decode partially"
        want = dr.drop_pixels(stream, W, H, wl, lossy, qs, lut, drop)
        want_coef = dr.drop_coefficients(stream, W, H, wl, lut, drop)
        for c16 in (True, False):
            got, res, dec = _decode(stream, W, H, wl, lossy, qs, lut, drop, c16=c16)
            assert np.array_equal(got, want), (drop, c16, res)
            if not c16:                                      # the 32-bit form: the coefficients are in the caller's array
                assert not res & 2 and np.array_equal(dec, want_coef), (drop, res)
            elif not lossy:
                assert res & 2, (drop, res)                  # the int16 form ran (the midpoint keeps coef16_ok's bound)
    assert not np.array_equal(dr.drop_pixels(stream, W, H, wl, lossy, qs, lut, 2), rr.reduced_pixels(stream, W, H, wl, lossy, qs, lut, 0))


# ---- composition ---------------------------------------------------------------------------------------------------------
COMP = (832, 320, 4)


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_composes_with_reduce_and_window(lossy, qs):
    W, H, wl = COMP
    drop = 2
    stream, lut = _stream(W, H, wl, lossy, qs)
    for r in (1, 2):
        want = dr.drop_pixels(stream, W, H, wl, lossy, qs, lut, drop, r)
        for c16 in (True, False):
            got, res, _ = _decode(stream, W, H, wl, lossy, qs, lut, drop, r=r, c16=c16)
            assert np.array_equal(got, want), (r, c16, res)
        # (LL_r is made of levels r and coarser: drop 2 takes a plane off level 1, none off level 2 and beyond)
        assert np.array_equal(want, rr.reduced_pixels(stream, W, H, wl, lossy, qs, lut, r)) == (r >= drop), r
    for r, win in ((0, (50, 40, 150, 100)), (1, (25, 20, 75, 50))):         # crosses codeblock borders in x and y
        x, y, w, h = win
        want = dr.drop_window(stream, W, H, wl, lossy, qs, lut, drop, r, x, y, w, h)
        got, _, _ = _decode(stream, W, H, wl, lossy, qs, lut, drop, r=r, win=win, pitch=w + 5)
        assert np.array_equal(got, want), (r, win)


def test_two_grey_frames_with_an_odd_frame_stride():
    W, H, wl = COMP
    n, drop = 2, 2
    pairs = [_stream(W, H, wl, False, 1.0, seed=s) for s in range(n)]
    lut = pairs[0][1]
    stride = max(p[0].size for p in pairs)
    streams = np.zeros((n, stride), np.uint16)
    for i, p in enumerate(pairs):
        streams[i, :p[0].size] = p[0]
    want = [dr.drop_pixels(p[0], W, H, wl, False, 1.0, lut, drop) for p in pairs]
    assert not np.array_equal(want[0], want[1])
    px = W * H
    fs = px + 3
    coef = np.full((n, H, W), POISON, np.int32)
    buf = np.full(n * fs + 128, 0xA5, np.uint8)
    base = (-buf.ctypes.data) % 64
    flag = np.zeros(1, np.int32)
    tab, geo = np.ascontiguousarray(lut.table, np.int32), _geo(lut)
    res = lib().emu_drop_decode(_p(streams), stride, W, H, wl, 0, C.c_float(1.0), _p(tab), _p(geo), 1, drop, 0, 0, 0, 0, W, H, _p(coef),
                                C.c_void_p(buf.ctypes.data + base), C.c_size_t(0), _p(flag), n, C.c_size_t(fs))
    assert res >= 0 and not res & 8 and flag[0] == 0
    expect = np.full(buf.size, 0xA5, np.uint8)
    for f in range(n):
        expect[base + f * fs:base + f * fs + px] = want[f].ravel()
    assert np.array_equal(buf, expect), res


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_two_rgb_frames(lossy, qs):
    """n = 2 RGB frames, the three components' tables on one grid, the same drop for the three components."""
    W, H, wl = COMP
    n, drop = 2, 2
    luts = [orc.lut_for_component(lossy, wl, c) for c in range(3)]
    planes = [[orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + c)) for c in range(3)] for f in range(n)]
    per = []
    for f in range(n):
        comps = orc.rgb_forward(*planes[f], lossy)
        per += [orc.encode_plane(comps[c], wl, lossy, qs, luts[c], None) for c in range(3)]
    stride = 9 + 2 * (W // 64) * (H // 64) + W * H + 1
    streams = np.zeros((3 * n, stride), np.uint16)
    for z, s in enumerate(per):
        streams[z, :s.size] = s
    P = W * H
    buf = np.full(3 * n * P + 128, 0xA5, np.uint8)
    base = (-buf.ctypes.data) % 64
    out = buf[base:base + 3 * n * P]
    flag = np.zeros(1, np.int32)
    tabs = [np.ascontiguousarray(t.table, np.int32) for t in luts]
    res = lib().emu_drop_decode_rgb(n, _p(streams), ULL(stride), _p(out), _p(out[P:]), _p(out[2 * P:]), ULL(3 * P), W, H, wl, int(lossy),
                                    C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])), drop, 0, _p(flag))
    assert res >= 0 and flag[0] == 0
    assert np.all(buf[:base] == 0xA5) and np.all(buf[base + 3 * n * P:] == 0xA5)
    for f in range(n):
        want = dr.drop_rgb(per[3 * f:3 * f + 3], W, H, wl, lossy, qs, luts, drop)
        plain = rr.reduced_rgb(per[3 * f:3 * f + 3], W, H, wl, lossy, qs, luts, 0)
        for c in range(3):
            assert np.array_equal(out[(3 * f + c) * P:(3 * f + c + 1) * P].reshape(H, W), want[c]), (f, c, res)
        assert any(not np.array_equal(want[c], plain[c]) for c in range(3))


# ---- drop = 0 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_drop_zero_is_the_plain_decode(lossy, qs):
    """The output is the full decode's and the launches are the plain sequence's: the intake, the decoder, a synthesis level
    a launch (one fewer where two ran fused), a clamp where the finest level did not write the pixels."""
    W, H, wl = 576, 320, 3
    stream, lut = _stream(W, H, wl, lossy, qs)
    for r in (0, 1):
        want = rr.reduced_pixels(stream, W, H, wl, lossy, qs, lut, r)
        assert np.array_equal(dr.drop_pixels(stream, W, H, wl, lossy, qs, lut, 0, r), want), "drop_ref at drop 0 is reduced_ref"
        counts = {}
        for drop in (0, 2):
            lib().emu_drop_reset()
            got, res, _ = _decode(stream, W, H, wl, lossy, qs, lut, drop, r=r)
            counts[drop] = lib().emu_drop_launches()
            assert counts[drop] == 2 + (wl - r) - (1 if res & 4 else 0) + (0 if res & 1 else 1), (drop, r, res)
            if drop == 0:
                assert np.array_equal(got, want), r
        assert counts[0] == counts[2]
