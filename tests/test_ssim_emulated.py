"""The SSIM calls' pieces on the CPU wave emulator (tests/hipemu/emu_ssim_driver.cpp): ssim_kernel, both forms, bit-exact
against the numpy model of the definition (ssim_ref.dssim); the probe sequence of launch_seq.hpp (unit transform,
quantise, synthesis, SSIM), grey and RGB, against the oracle's decode of its own encode; and a search over such probes
against the reference procedure."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
import ssim_ref as sr
from emu_lib import _p, driver_lib

_lib = None
ULL = C.c_ulonglong
SENTINEL = 0xABCDEF0123456789


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_ssim.so", ("emu_ssim_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
    return _lib


def shape():
    s = np.zeros(2, np.int32)
    lib().emu_ssim_shape(_p(s))
    return int(s[0]), int(s[1])


def _emu_dssim(a, b, W, H, n=1, a_pitch=None, b_pitch=None, a_z=0, b_z=0, max_wgs=0, want_vec=None):
    """a, b: flat u8 views whose first byte is frame 0's first sample."""
    out = np.full(n + 1, SENTINEL, np.uint64)
    vec = lib().emu_dssim(_p(a), ULL(a_pitch), ULL(a_z), _p(b), ULL(b_pitch), ULL(b_z), W, H, n, _p(out), max_wgs)
    assert out[n] == SENTINEL                                # nothing behind out[n)
    if want_vec is not None:
        assert bool(vec) == want_vec
    return [int(v) for v in out[:n]]


def _ref(a, b, W, H, pitch_a, pitch_b):
    A = a[:H * pitch_a].reshape(H, pitch_a)[:, :W]
    B = b[:H * pitch_b].reshape(H, pitch_b)[:, :W]
    return sr.dssim(A, B)


def _padded(vis, AW, AH, fill):
    """The visible plane set into an aligned padded one whose padding holds `fill` (it must not count)."""
    H, W = vis.shape
    out = E.aligned_zeros(AW * AH, np.uint8).reshape(AH, AW)
    out[:] = fill
    out[:H, :W] = vis
    return out.ravel()


# 33 x 32: 7 x 7 windows, the eighth block column a lane of its own with one neighbour; 203 x 139: trailing columns and
# rows in no window, three bands; 1100 x 40: five strips of 63 window columns; 40 x 300: one strip, five bands
SHAPES = [(33, 32), (200, 136), (203, 139), (1100, 40), (40, 300)]


def test_shapes_cross_the_kernels_cuts():
    strip, band = shape()
    nx = lambda W: (W - 8) // 4 + 1
    assert nx(1100) > 2 * strip and nx(203) <= strip and nx(40) + 1 < 64
    assert nx(300) > 2 * band and nx(139) > 2 * band and nx(40) <= band      # (ny of a height H is nx(H))
    assert (33 - 8) // 4 + 1 == 7 and 4 * (nx(203) + 1) < 203 and 4 * (nx(139) + 1) < 139


@pytest.mark.parametrize("W,H", SHAPES)
def test_dssim_is_bit_exact_on_the_content_kinds(W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    rng = np.random.default_rng(W * 7 + H)
    va = rng.integers(0, 256, (H, W)).astype(np.uint8)
    vb = rng.integers(0, 256, (H, W)).astype(np.uint8)
    a, b = _padded(va, AW, AH, 0x11), _padded(vb, AW, AH, 0xEE)
    # identical images: exactly 0 -- every window counted once gives windows * 2^24 on both sides of the subtraction;
    # a window counted twice or missed leaves a multiple of 2^24 only where its q is 2^24, so noise is checked too
    same = _padded(va, AW, AH, 0x77)
    for mw in (0, 1):
        assert _emu_dssim(a, same, W, H, a_pitch=AW, b_pitch=AW, max_wgs=mw, want_vec=True) == [0]
    want = _ref(a, b, W, H, AW, AW)
    assert want > 0
    assert _emu_dssim(a, b, W, H, a_pitch=AW, b_pitch=AW, want_vec=True) == [want]
    assert _emu_dssim(a, b, W, H, a_pitch=AW, b_pitch=AW, max_wgs=1, want_vec=True) == [want]     # one workgroup, every tile
    assert _emu_dssim(b, a, W, H, a_pitch=AW, b_pitch=AW, max_wgs=2) == [want]                    # the measure is symmetric
    # an image against its negative: negative q, a sum above windows * 2^24
    smooth = (np.add.outer(np.arange(H) * 3, np.arange(W) * 5) % 256).astype(np.uint8)
    smooth[::7, ::5] ^= 0x80
    c, d = _padded(smooth, AW, AH, 0), _padded(255 - smooth, AW, AH, 0)
    assert sr.window_q(smooth, 255 - smooth).min() < 0
    want_neg = _ref(c, d, W, H, AW, AW)
    assert _emu_dssim(c, d, W, H, a_pitch=AW, b_pitch=AW, want_vec=True) == [want_neg]
    # all 0 against all 255
    z, f = _padded(np.zeros((H, W), np.uint8), AW, AH, 0x55), _padded(np.full((H, W), 255, np.uint8), AW, AH, 0x55)
    want_flat = _ref(z, f, W, H, AW, AW)
    assert want_flat == sr.windows(W, H) * ((1 << 24) - 26)          # q = 26 a window (2106 over the 81 windows of 40 x 40)
    assert _emu_dssim(z, f, W, H, a_pitch=AW, b_pitch=AW, want_vec=True) == [want_flat]


@pytest.mark.parametrize("W,H", [(33, 32), (203, 139), (1100, 40)])
def test_per_byte_form_gives_the_same_result(W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    rng = np.random.default_rng(H)
    va = rng.integers(0, 256, (H, W)).astype(np.uint8)
    vb = (va.astype(np.int32) + rng.integers(-20, 21, (H, W))).clip(0, 255).astype(np.uint8)
    a, b = _padded(va, AW, AH, 1), _padded(vb, AW, AH, 2)
    want = _ref(a, b, W, H, AW, AW)
    assert _emu_dssim(a, b, W, H, a_pitch=AW, b_pitch=AW, want_vec=True) == [want]
    # pointers offset by one byte
    ua, ub = E.aligned_zeros(AW * AH + 16, np.uint8), E.aligned_zeros(AW * AH + 16, np.uint8)
    ua[1:1 + a.size] = a
    ub[1:1 + b.size] = b
    assert _emu_dssim(ua[1:], ub[1:], W, H, a_pitch=AW, b_pitch=AW, want_vec=False) == [want]
    assert _emu_dssim(ua[1:], b, W, H, a_pitch=AW, b_pitch=AW, max_wgs=1, want_vec=False) == [want]
    # an odd row stride on one side
    op = AW + 3
    o = E.aligned_zeros(op * AH, np.uint8)
    o.reshape(AH, op)[:, :AW] = b.reshape(AH, AW)
    assert _emu_dssim(a, o, W, H, a_pitch=AW, b_pitch=op, want_vec=False) == [want]


@pytest.mark.parametrize("W,H", [(203, 139), (1100, 40)])
def test_three_frames_a_launch_with_gaps_between_them(W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    P = AW * AH
    za, zb = P + 4096, P + 12                               # 4-byte aligned strides above P
    rng = np.random.default_rng(W)
    a, b = E.aligned_zeros(3 * za, np.uint8), E.aligned_zeros(3 * zb, np.uint8)
    a[:] = rng.integers(0, 256, a.size)
    b[:] = rng.integers(0, 256, b.size)
    b[zb:zb + P] = a[za:za + P]                             # frame 1 equal in all but its padding
    b[zb:zb + P].reshape(AH, AW)[:, W:] ^= 0x55
    b[2 * zb:2 * zb + P] = (a[2 * za:2 * za + P].astype(np.int32) + rng.integers(-9, 10, P)).clip(0, 255)
    want = [_ref(a[f * za:], b[f * zb:], W, H, AW, AW) for f in range(3)]
    assert want[1] == 0 and want[0] > want[2] > 0
    for max_wgs in (0, 1, 3):
        assert _emu_dssim(a, b, W, H, 3, AW, AW, za, zb, max_wgs, want_vec=True) == want
    # a stride that is no multiple of 4: the per-byte form
    zc = P + 13
    c = E.aligned_zeros(3 * zc, np.uint8)
    for f in range(3):
        c[f * zc:f * zc + P] = b[f * zb:f * zb + P]
    assert _emu_dssim(a, c, W, H, 3, AW, AW, za, zc, 1, want_vec=False) == want
    assert _emu_dssim(a, c, W, H, 3, AW, AW, za, zc, 0, want_vec=False) == want


# ---- the probe sequence ---------------------------------------------------------------------------------------------
def _grey_src(imgs):
    pads = [orc.pad_frame(im) for im in imgs]
    AH, AW = pads[0].shape
    P = AW * AH
    src = E.aligned_zeros(len(pads) * P, np.uint8)
    for f, im in enumerate(pads):
        src[f * P:(f + 1) * P] = im.ravel()
    return src, AW, AH


def _probe(name, js):
    W, H, wl, frames, rgb = sr.case_geometry(name)
    imgs, _ = sr.case_inputs(name)
    nf = 3 if rgb else frames
    out = np.zeros(len(js) * nf, np.uint64)
    jarr = np.array(js, np.int32)
    if rgb:
        src = [E.aligned_copy(orc.pad_frame(p)) for p in imgs]
        AH, AW = src[0].shape
        rc = lib().emu_ssim_probe(_p(src[0]), ULL(0), _p(src[1]), _p(src[2]), W, H, AW, AH, wl, 3, _p(jarr), len(js), _p(out))
    else:
        src, AW, AH = _grey_src(imgs)
        rc = lib().emu_ssim_probe(_p(src), ULL(AW * AH), None, None, W, H, AW, AH, wl, nf, _p(jarr), len(js), _p(out))
    assert rc == 0
    return [[int(v) for v in out[i * nf:(i + 1) * nf]] for i in range(len(js))]


@pytest.mark.parametrize("name", ["200x136-wl3-0.98", "rgb-200x136-wl3-0.98"])
def test_probe_sequence_equals_the_reference_dssim(name):
    j = sr.CASES[name][3]
    js = [j, 1021]
    fn = sr.case_list_fn(name)
    assert sum(fn(j)) == sr.CASES[name][4]
    assert _probe(name, js) == [fn(v) for v in js]


# ---- a search over probes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_search_in_a_range_around_the_recorded_result(K):
    name = "200x136-wl3-0.98"
    W, H, wl, frames, rgb = sr.case_geometry(name)
    _, _, limit, j, d, prev_j, prev_d = sr.CASES[name]
    j_min, j_max = j - 12, j + 12                           # 25 values of j: five probes
    ref = sr.case_result(name, limit, j_min, j_max)
    assert (ref.j, ref.sse, ref.prev_j, ref.prev_sse) == (j, d, prev_j, prev_d) and 4 <= len(ref.probes) <= 5
    imgs, _ = sr.case_inputs(name)
    src, AW, AH = _grey_src(imgs)
    res = np.zeros(1, np.uint64)
    stats, probed = np.zeros(3, np.int32), np.zeros(64, np.int32)
    got = lib().emu_ssim_search(_p(src), ULL(AW * AH), None, None, W, H, AW, AH, wl, 1, ULL(limit), j_min, j_max, K, _p(res),
                                _p(stats), _p(probed))
    assert got == j and int(res[0]) == d
    made = [int(v) for v in probed[:stats[2]]]
    if K == 1:
        assert made == [p[0] for p in ref.probes]
    else:
        assert made == sr.rounds3(sr.case_dssim_fn(name), limit, j_min, j_max) and stats[0] == (len(ref.probes) + 1) // 2
    assert stats[1] == len(ref.probes)
