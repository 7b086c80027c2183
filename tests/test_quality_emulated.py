"""The quality calls' pieces on the CPU wave emulator (tests/hipemu/emu_quality_driver.cpp): sse_kernel against numpy,
the search of rate_search.hpp (bisect_walk, smallest passing index) against the reference procedure (quality_ref.bisect),
quantise_kernel's int32 form against the oracle's fused transform truncated, and the probe sequence of launch_seq.hpp
(unit transform, quantise, synthesis, SSE) against the oracle's decode of its own encode."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
import quality_ref as qr
import rate_ref as rr
from emu_lib import _p, driver_lib

_lib = None
ULL = C.c_ulonglong


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_quality.so", ("emu_quality_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
    return _lib


# ---- sse_kernel -----------------------------------------------------------------------------------------------------
def _emu_sse(a, b, W, H, n=1, a_pitch=None, b_pitch=None, a_z=0, b_z=0, max_wgs=0, want_vec=None):
    """a, b: flat u8 views whose first byte is frame 0's first sample."""
    out = np.full(n + 1, 0xABCDEF0123456789, np.uint64)
    vec = lib().emu_sse(_p(a), ULL(a_pitch), ULL(a_z), _p(b), ULL(b_pitch), ULL(b_z), W, H, n, _p(out), max_wgs)
    assert out[n] == 0xABCDEF0123456789                     # nothing behind out[n)
    if want_vec is not None:
        assert bool(vec) == want_vec
    return [int(v) for v in out[:n]]


def _np_sse(a, b, W, H, pitch_a, pitch_b):
    A = a[:H * pitch_a].reshape(H, pitch_a)[:, :W].astype(np.int64)
    B = b[:H * pitch_b].reshape(H, pitch_b)[:, :W].astype(np.int64)
    return int(((A - B) ** 2).sum())


SHAPES = [(200, 136), (700, 500), (201, 137)]


@pytest.mark.parametrize("W,H", SHAPES)
def test_sse_of_random_pairs(W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    if W == 700:
        assert W % 16 == 12
    rng = np.random.default_rng(W)
    a, b = E.aligned_zeros(AW * AH, np.uint8), E.aligned_zeros(AW * AH, np.uint8)
    a[:] = rng.integers(0, 256, a.size)
    b[:] = rng.integers(0, 256, b.size)
    want = _np_sse(a, b, W, H, AW, AW)
    assert want > 0
    assert _emu_sse(a, b, W, H, a_pitch=AW, b_pitch=AW, want_vec=True) == [want]
    assert _emu_sse(a, b, W, H, a_pitch=AW, b_pitch=AW, max_wgs=1, want_vec=True) == [want]   # one workgroup, every tile
    assert _emu_sse(a, a, W, H, a_pitch=AW, b_pitch=AW) == [0]                                # equal images
    # padding that differs does not count: the columns [W, AW) and the rows [H, AH)
    c = a.copy().reshape(AH, AW)
    c[:, W:] ^= 0xFF
    c[H:, :] ^= 0xFF
    c = E.aligned_copy(c).ravel()
    assert _emu_sse(a, c, W, H, a_pitch=AW, b_pitch=AW, want_vec=True) == [0]
    assert _emu_sse(b, c, W, H, a_pitch=AW, b_pitch=AW) == [want]
    # pointers offset by one byte: the per-byte form, the same result
    ua, ub = E.aligned_zeros(AW * AH + 16, np.uint8), E.aligned_zeros(AW * AH + 16, np.uint8)
    ua[1:1 + a.size] = a
    ub[1:1 + b.size] = b
    assert _emu_sse(ua[1:], ub[1:], W, H, a_pitch=AW, b_pitch=AW, want_vec=False) == [want]
    assert _emu_sse(ua[1:], b, W, H, a_pitch=AW, b_pitch=AW, max_wgs=1, want_vec=False) == [want]


@pytest.mark.parametrize("W,H", SHAPES)
def test_sse_of_three_frames_with_strides_above_a_frame(W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    P = AW * AH
    za, zb = P + 4096, P + 160                              # 16-byte aligned strides above P
    rng = np.random.default_rng(H)
    a, b = E.aligned_zeros(3 * za, np.uint8), E.aligned_zeros(3 * zb, np.uint8)
    a[:] = rng.integers(0, 256, a.size)
    b[:] = rng.integers(0, 256, b.size)
    b[zb:zb + P] = a[za:za + P]                             # frame 1 equal in all but its padding
    b[zb:zb + P].reshape(AH, AW)[:, W:] ^= 0x55
    want = [_np_sse(a[f * za:], b[f * zb:], W, H, AW, AW) for f in range(3)]
    assert want[1] == 0 and want[0] > 0 and want[2] > 0
    for max_wgs in (0, 1, 3):
        assert _emu_sse(a, b, W, H, 3, AW, AW, za, zb, max_wgs, want_vec=True) == want
    # a stride that is no multiple of 16: the per-byte form
    zc = P + 161
    c = E.aligned_zeros(3 * zc, np.uint8)
    for f in range(3):
        c[f * zc:f * zc + P] = b[f * zb:f * zb + P]
    assert _emu_sse(a, c, W, H, 3, AW, AW, za, zc, 1, want_vec=False) == want


def test_sse_widens_before_a_lanes_32_bit_sum_overflows():
    """One 4224 x 4160 frame of 0 against 255 on ONE workgroup: 264 * 4160 vectors over 256 lanes are 4290 loads a lane,
    beyond the 4128 a 32-bit run may hold -- each lane's own sum passes 2^32, the total 2^40."""
    W, H = 4224, 4160
    a, b = E.aligned_zeros(W * H, np.uint8), E.aligned_zeros(W * H, np.uint8)
    b[:] = 255
    want = W * H * 65025
    assert (W // 16) * H // 256 * 16 * 65025 > 1 << 32 and want > 1 << 40
    assert _emu_sse(a, b, W, H, a_pitch=W, b_pitch=W, max_wgs=1, want_vec=True) == [want]


# ---- the stepper ----------------------------------------------------------------------------------------------------
def emu_search(table, limit, j_min, j_max, K):
    stats = np.zeros(3, np.int32)
    probed = np.zeros(64, np.int32)
    j = lib().emu_quality_search(_p(np.ascontiguousarray(table, np.uint64)), ULL(limit), j_min, j_max, K, _p(stats), _p(probed))
    return j, tuple(int(v) for v in stats), [int(v) for v in probed[:stats[2]]]


def _ramp():
    """A monotone distortion: 0 at the finest quantiser j = 16383, rising towards j = 1."""
    j = np.arange(rr.J_MAX + 1, dtype=np.int64)
    return (rr.J_MAX - j) * 7 + (rr.J_MAX - j) ** 2 // 1000


def _noisy():
    rng = np.random.default_rng(30)
    return _ramp() * 3 + rng.integers(0, 400, rr.J_MAX + 1)


def _oracle_window():
    """The oracle's SSE at j = 1830..1899 (200 x 136, wl 3: rising steps among them) set into a ramp that meets both ends."""
    fn = qr.case_sse_fn("200x136-wl3-40dB")
    win = np.array([fn(j) for j in range(1830, 1900)], np.int64)
    assert np.any(np.diff(win) > 0), "the fixture's point: a distortion that rises as j grows"
    j = np.arange(rr.J_MAX + 1, dtype=np.int64)
    t = np.empty(rr.J_MAX + 1, np.int64)
    t[:1830] = win[0] + (1830 - j[:1830]) * 500
    t[1830:1900] = win
    t[1900:] = np.maximum(win[-1] - (j[1900:] - 1899) * 20, 0)
    return t, win


def _check(table, limit, j_min=0, j_max=0):
    ref = qr.bisect(lambda j: table[j], limit, j_min, j_max)
    for K in (1, 3):
        j, (rounds, used, made), probed = emu_search(table, limit, j_min, j_max, K)
        assert j == (ref.j or 0), (K, limit, j_min, j_max)
        assert used == len(ref.probes)
        if K == 1:
            assert rounds == made == used and probed == [p[0] for p in ref.probes]
        else:
            want = qr.rounds3(lambda j: table[j], limit, j_min, j_max)
            assert rounds == (used + 1) // 2 and made == len(want) <= 3 * rounds
            assert probed == want and set(p[0] for p in ref.probes) <= set(probed)
    return ref


def test_stepper_on_a_monotone_function_over_the_whole_grid():
    t = _ramp()
    g = rr.grid()
    for limit in (int(t[g[-1]]), int(t[g[-1]]) + 1, 1000, 50000, int(t[1]) - 1, int(t[1])):
        ref = _check(t, limit)
        assert ref.j is not None and len(ref.probes) in (13, 14)
        assert ref.j == min(j for j in g if t[j] <= limit)           # monotone: the procedure finds the coarsest
    j, (rounds, used, made), _ = emu_search(t, 50000, 0, 0, 3)
    assert rounds == (used + 1) // 2 == 7                            # two bisection levels a round


def test_stepper_on_the_oracles_non_monotone_window():
    t, win = _oracle_window()
    for limit in sorted(set(int(v) for v in win)) + [int(win.min()) - 1, int(win.max()) + 1]:
        _check(t, limit)
        _check(t, limit, 1830, 1899)
        _check(t, limit, 1000, 3000)


def test_stepper_on_noisy_functions_and_sub_ranges():
    t = _noisy()
    rng = np.random.default_rng(31)
    for _ in range(40):
        a, b = sorted(int(v) for v in rng.integers(1, rr.J_MAX + 1, 2))
        if not rr.grid(a, b):
            continue
        _check(t, int(t[int(rng.integers(a, b + 1))]) + int(rng.integers(-3, 4)), a, b)
    for a, b in ((1, 1), (6, 8), (8, 9), (16382, 16383), (1000, 3000)):
        for limit in (int(t[b]) - 1, int(t[b]), int(t[a]), int(t[(a + b) // 2])):
            _check(t, max(limit, 0), a, b)


def test_nothing_meets_and_everything_meets():
    t = _ramp() + 5
    for a, b in ((0, 0), (1000, 3000), (5, 5)):
        g = rr.grid(a, b)
        none = _check(t, int(min(t[j] for j in g)) - 1, a, b)
        assert none.j is None
        top = _check(t, 1 << 50, a, b)
        assert top.j == g[0] and top.prev_j is None
    j, (rounds, used, made), _ = emu_search(t, 0, 0, 0, 3)
    assert j == 0 and used == 14 and rounds == 7
    assert emu_search(t, 100, 7, 7, 3)[0] == -1                      # a range without a grid entry
    assert emu_search(t, 100, 5, 0, 3)[0] == -1 and emu_search(t, 100, 1, 16384, 1)[0] == -1


# ---- quantise_kernel, int32 form ------------------------------------------------------------------------------------
def _unit(imgs, wl):
    AH, AW = imgs[0].shape
    P = AW * AH
    stride = (P + orc.dwt_extra(AW, AH, wl) + 3) // 4 * 4
    src = E.aligned_zeros(len(imgs) * P, np.uint8)
    for f, im in enumerate(imgs):
        src[f * P:(f + 1) * P] = im.ravel()
    out = E.aligned_zeros(len(imgs) * stride, np.float32)
    lib().emu_quality_unit_forward(_p(src), ULL(P), _p(out), ULL(stride * 4), AW, AH, wl, len(imgs))
    return out, stride


@pytest.mark.parametrize("W,H,wl,js", [(200, 136, 3, (1, 1865, 16382)), (700, 500, 6, (77, 5190))])
def test_int32_quantise_equals_the_truncated_fused_transform(W, H, wl, js):
    imgs = [orc.pad_frame(orc.gen_frame(W, H, f)) for f in range(2)]
    AH, AW = imgs[0].shape
    P = AW * AH
    unit, stride = _unit(imgs, wl)
    for j in js:
        dst = E.aligned_zeros(2 * P + 4, np.int32)
        dst[:] = 0x5EADBEEF
        lib().emu_quality_quantise_i32(_p(unit), ULL(stride * 4), _p(dst), ULL(P * 4), AW, AH, wl, 2, j)
        assert np.all(dst[2 * P:] == 0x5EADBEEF)
        for f in range(2):
            ref = orc.dwt_forward(orc.level_shift_fwd(imgs[f], True), wl, rr.q(j))[:P]
            assert np.array_equal(dst[f * P:(f + 1) * P], np.trunc(ref).astype(np.int32)), (j, f)


# ---- the probe sequence ---------------------------------------------------------------------------------------------
def _probe(planes, W, H, wl, j, rgb):
    AH, AW = planes[0].shape
    P = AW * AH
    n = len(planes)
    out = np.zeros(n, np.uint64)
    if rgb:
        src = [E.aligned_copy(p) for p in planes]
        rc = lib().emu_quality_probe(_p(src[0]), ULL(0), _p(src[1]), _p(src[2]), W, H, AW, AH, wl, 3, j, _p(out))
    else:
        src = E.aligned_zeros(n * P, np.uint8)
        for f, im in enumerate(planes):
            src[f * P:(f + 1) * P] = im.ravel()
        rc = lib().emu_quality_probe(_p(src), ULL(P), None, None, W, H, AW, AH, wl, n, j, _p(out))
    assert rc == 0
    return [int(v) for v in out]


@pytest.mark.parametrize("j", [77, 1865, 16382])
def test_probe_sequence_equals_the_reference_sse(j):
    W, H, wl = 200, 136, 3
    imgs = [orc.gen_frame(W, H, f) for f in range(2)]
    want = qr.frames_sse_list(imgs, wl, orc.lut_for(True, wl), j)
    if j == 1865:
        assert want[0] == qr.CASES["200x136-wl3-40dB"][10][0]
    assert _probe([orc.pad_frame(im) for im in imgs], W, H, wl, j, False) == want


def test_probe_sequence_of_an_rgb_frame():
    name = "rgb-200x136-wl3-40dB"
    W, H, wl = qr.CASES[name][:3]
    j, per = qr.CASES[name][9], qr.CASES[name][10]
    planes, luts = qr.case_inputs(name)
    assert qr.rgb_sse_list(planes, wl, luts, j) == per
    assert _probe([orc.pad_frame(p) for p in planes], W, H, wl, j, True) == per
