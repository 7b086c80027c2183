"""The reduced-resolution decode on the CPU wave emulator (tests/hipemu/emu_reduce_driver.cpp): the decoder over the
codeblock rectangle of the 1/2^r image and the synthesis stopped at level r, against the oracle's LL_r."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
import reduced_ref as rr
from emu_lib import _geo, _p, driver_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_reduce.so", ("emu_reduce_driver.cpp", "emu_runtime.cpp"))
    return _lib


def decode_reduced(stream, AW, AH, wl, lossy, qs, lut, r, k=0.0, c16=True, staging=False, misalign=0, coef_fill=0x7A5A5A5A):
    """Returns (pixels (AH >> r, AW >> r), flags of emu_decode_reduced, range flag, decoder output (AH, AW))."""
    stream = np.ascontiguousarray(stream, np.uint16)
    coef = np.full((AH, AW), coef_fill, np.int32)
    n = (AW >> r) * (AH >> r)
    buf = np.full(n + 128, 0xA5, np.uint8)
    base = (-buf.ctypes.data) % 64 + misalign
    flag = np.zeros(1, np.int32)
    tab = np.ascontiguousarray(lut.table, np.int32)
    geo = _geo(lut)
    res = lib().emu_decode_reduced(_p(stream), int(stream.size), AW, AH, wl, int(lossy), C.c_float(qs), _p(tab), _p(geo),
                                   C.c_float(k), int(lut.n_tables), int(c16), int(staging), r, _p(coef),
                                   C.c_void_p(buf.ctypes.data + base), _p(flag), 1, C.c_size_t(0))
    assert np.all(buf[:base] == 0xA5) and np.all(buf[base + n:] == 0xA5), "bytes written outside the reduced image"
    return buf[base:base + n].reshape(AH >> r, AW >> r), res, int(flag[0]), coef


def stack_streams(streams):
    """The streams as rows of one array, its row length their stride: (array, stride in shorts)."""
    stride = max(s.size for s in streams)
    out = np.zeros((len(streams), stride), np.uint16)
    for i, s in enumerate(streams):
        out[i, :s.size] = s
    return out, stride


def _stream(W, H, wl, lossy, qs, k, seed=0):
    lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
    img = orc.gen_frame(W, H, seed)
    return orc.encode_frame(img, wl, lossy, qs, lut, k=k), lut


def test_reduced_dims_arithmetic():
    d = (C.c_int * 5)()
    cases = [(700, 500, 704, 512, 0, (700, 500, 704, 512, 88)), (700, 500, 704, 512, 1, (350, 250, 352, 256, 24)),
             (700, 500, 704, 512, 3, (88, 63, 88, 64, 2)), (7680, 4320, 7680, 4352, 1, (3840, 2160, 3840, 2176, 2040)),
             (7680, 4320, 7680, 4352, 2, (1920, 1080, 1920, 1088, 510)), (832, 320, 832, 320, 1, (416, 160, 416, 160, 21)),
             (1000, 300, 1024, 320, 4, (63, 19, 64, 20, 1))]
    for W, H, AW, AH, r, want in cases:
        lib().emu_reduced_dims(W, H, AW, AH, r, d)
        assert tuple(d) == want, (W, H, r)
    assert [lib().emu_reduce_ok(5, r) for r in (-1, 0, 4, 5)] == [0, 1, 1, 0]


# 704x512 wl 3: the rectangle straddles subbands; 576x320 wl 3: 5 codeblock columns at r = 1; 832x320 wl 4: 7 at r = 1
# (odd ncx_r: a wave's halves lie in two codeblock rows)
FRAMES = [(704, 512, 3), (576, 320, 3), (832, 320, 4)]


@pytest.mark.parametrize("W,H,wl", FRAMES)
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5), (True, 0.3)])
def test_reduced_matches_oracle_ll(W, H, wl, lossy, qs):
    stream, lut = _stream(W, H, wl, lossy, qs, 0.0)
    for r in range(wl):
        want = rr.reduced_pixels(stream, W, H, wl, lossy, qs, lut, r)
        for c16 in (True, False):
            got, res, flag, _ = decode_reduced(stream, W, H, wl, lossy, qs, lut, r, c16=c16)
            assert flag == 0 and not res & 8
            assert np.array_equal(got, want), (r, c16, res)
            if c16 and not lossy and r <= wl - 2:
                assert res & 2, (r, res)            # the 16-bit form over the levels that run


@pytest.mark.parametrize("W,H,wl", FRAMES)
def test_reduced_k_mode_matches_oracle_ll(W, H, wl):
    k = 0.5
    stream, lut = _stream(W, H, wl, False, 1.0, k)
    for r in range(wl):
        want = rr.reduced_pixels(stream, W, H, wl, False, 1.0, lut, r, k=k)
        for c16 in (True, False):
            got, res, flag, _ = decode_reduced(stream, W, H, wl, False, 1.0, lut, r, k=k, c16=c16)
            assert flag == 0
            assert np.array_equal(got, want), (r, c16, res)


def test_reduced_staging_and_misaligned_output():
    W, H, wl = 832, 320, 4
    stream, lut = _stream(W, H, wl, True, 0.5, 0.0)
    for r in range(wl):
        want = rr.reduced_pixels(stream, W, H, wl, True, 0.5, lut, r)
        got, res, _, _ = decode_reduced(stream, W, H, wl, True, 0.5, lut, r, staging=True)
        assert np.array_equal(got, want) and not res & 2, r
        got, res, _, _ = decode_reduced(stream, W, H, wl, True, 0.5, lut, r, misalign=3)
        assert np.array_equal(got, want) and not res & 1, r


@pytest.mark.parametrize("k", [0.0, 0.5])
def test_reduced_decoder_touches_only_the_rectangle(k):
    """Coefficients outside the rectangle are not written, and a codeblock there whose MSB is out of range is never
    looked at: the range flag stays clear and the pixels are those of the clean stream."""
    W, H, wl, r = 832, 320, 4, 1
    stream, lut = _stream(W, H, wl, False, 1.0, k)
    ncx, ncy = W // 64, H // 64
    ncx_r, ncy_r = -(-(W >> r) // 64), -(-(H >> r) // 64)
    want = rr.reduced_pixels(stream, W, H, wl, False, 1.0, lut, r, k=k)
    bad = stream.copy()
    outside = (ncy_r - 1) * ncx + ncx_r            # first codeblock right of the rectangle's last row
    assert outside % ncx >= ncx_r
    bad[9 + 2 * outside] = 20
    got, _, flag, coef = decode_reduced(bad, W, H, wl, False, 1.0, lut, r, k=k, c16=False)
    assert flag == 0 and np.array_equal(got, want)
    inside = np.zeros((ncy, ncx), bool)
    inside[:ncy_r, :ncx_r] = True
    written = (coef != 0x7A5A5A5A).reshape(ncy, 64, ncx, 64).any(axis=(1, 3))
    assert not (written & ~inside).any()
    _, _, flag0, _ = decode_reduced(bad, W, H, wl, False, 1.0, lut, 0, k=k, c16=False)
    assert flag0 == 1                                 # the full decode reads that codeblock


# The smallest frame of FRAMES, 9 codeblock columns (every frame of FRAMES is a padded size, a multiple of 64): an odd
# count, so a wave's two codeblocks straddle codeblock rows and frames; the frame stride is not the frame's size.
N_FRAMES = (576, 320, 3)


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
@pytest.mark.parametrize("r", [0, 1])
def test_reduced_two_grey_frames(lossy, qs, r):
    """picsong_decode_frames_reduced's n = 2 path through the library's sequence: each frame against the oracle, nothing
    written between the frames, and the launches counted -- the intake (1), the decoder (1), a synthesis level a launch
    (wl - r; one fewer where levels r + 1 and r ran as one), and a clamp a frame where level r did not write the
    pixels itself (a frame stride that is no multiple of 4)."""
    W, H, wl = N_FRAMES
    n = 2
    pairs = [_stream(W, H, wl, lossy, qs, 0.0, seed=s) for s in range(n)]
    lut = pairs[0][1]
    streams, stride = stack_streams([p[0] for p in pairs])
    want = [rr.reduced_pixels(p[0], W, H, wl, lossy, qs, lut, r) for p in pairs]
    assert not np.array_equal(want[0], want[1])
    px = (W >> r) * (H >> r)
    tab, geo = np.ascontiguousarray(lut.table, np.int32), _geo(lut)
    for gap in (64, 3):
        fs = px + gap
        coef = np.full((n, H, W), 0x7A5A5A5A, np.int32)
        buf = np.full(n * fs + 128, 0xA5, np.uint8)
        base = (-buf.ctypes.data) % 64
        flag = np.zeros(1, np.int32)
        lib().emu_reduce_reset()
        res = lib().emu_decode_reduced(_p(streams), stride, W, H, wl, int(lossy), C.c_float(qs), _p(tab), _p(geo), C.c_float(0.0),
                                       int(lut.n_tables), 1, 0, r, _p(coef), C.c_void_p(buf.ctypes.data + base), _p(flag), n,
                                       C.c_size_t(fs))
        assert res >= 0 and not res & 8 and flag[0] == 0
        expect = np.full(buf.size, 0xA5, np.uint8)
        for f in range(n):
            expect[base + f * fs:base + f * fs + px] = want[f].ravel()
        assert np.array_equal(buf, expect), (gap, res)
        assert bool(res & 1) == (gap % 4 == 0), (gap, res)      # both forms are taken: these levels take the vector kernels
        assert lib().emu_reduce_launches() == 2 + (wl - r) - (1 if res & 4 else 0) + (0 if res & 1 else n), (gap, res)
