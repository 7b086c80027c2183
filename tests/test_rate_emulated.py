"""The rate calls' pieces on the CPU wave emulator (tests/hipemu/emu_rate_driver.cpp): the search stepper of
rate_search.hpp against the reference procedure (rate_ref.bisect), and the unquantised forward transform followed by
quantise_kernel against the oracle's fused transform at q(j), bit for bit in both coefficient forms."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
import rate_ref as rr
from emu_lib import _p, driver_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_rate.so", ("emu_rate_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
        _lib.emu_rate_q.restype = C.c_float
    return _lib


# ---- the search -----------------------------------------------------------------------------------------------------
def emu_search(table, target, j_min, j_max, K):
    stats = np.zeros(3, np.int32)
    probed = np.zeros(64, np.int32)
    j = lib().emu_rate_search(_p(table), C.c_longlong(target), j_min, j_max, K, _p(stats), _p(probed))
    return j, tuple(int(v) for v in stats), [int(v) for v in probed[:stats[2]]]


def _ramp():
    """A monotone size function: 34 shorts at j = 1, about a short per step."""
    j = np.arange(rr.J_MAX + 1, dtype=np.int64)
    return 33 + j + j * j // 40000


def _oracle_window():
    """The oracle's sizes at j = 4990..5029 (200 x 136, wl 3: not monotone) set into a ramp that meets both ends."""
    size = rr.frames_size_fn([orc.gen_frame(200, 136)], 3, orc.lut_for(True, 3))
    win = np.array([size(j) for j in range(4990, 5030)], np.int64)
    assert np.any(np.diff(win) < 0), "the fixture's point: sizes that fall as j grows"
    t = np.empty(rr.J_MAX + 1, np.int64)
    j = np.arange(rr.J_MAX + 1, dtype=np.int64)
    t[:4990] = win[0] - (4990 - j[:4990])
    t[4990:5030] = win
    t[5030:] = win[-1] + (j[5030:] - 5029)
    return t, win


def _noisy():
    rng = np.random.default_rng(20)
    return _ramp() * 3 + rng.integers(-40, 41, rr.J_MAX + 1)


def _check(table, target, j_min=0, j_max=0):
    ref = rr.bisect(lambda j: table[j], target, j_min, j_max)
    for K in (1, 3):
        j, (rounds, used, made), probed = emu_search(table, target, j_min, j_max, K)
        assert j == (ref.j or 0), (K, target, j_min, j_max)
        assert used == len(ref.probes)
        if K == 1:
            assert rounds == made == used and probed == [p[0] for p in ref.probes]
        else:
            want = rr.rounds3(lambda j: table[j], target, j_min, j_max)
            assert rounds == (used + 1) // 2 and made == len(want) <= 3 * rounds
            assert probed == want and set(p[0] for p in ref.probes) <= set(probed)
    return ref


def test_stepper_on_a_monotone_function_over_the_whole_grid():
    t = _ramp()
    g = rr.grid()
    for target in (34, 35, 1000, 5000, int(t[g[-1]]) - 1, int(t[g[-1]])):
        ref = _check(t, target)
        assert ref.j is not None and len(ref.probes) == 14
        assert ref.j == max(j for j in g if t[j] <= target)          # monotone: the procedure finds the maximum
    j, (rounds, used, made), _ = emu_search(t, 5000, 0, 0, 3)
    assert (rounds, used) == (7, 14)                                 # two bisection levels a round


def test_stepper_on_the_oracles_non_monotone_window():
    t, win = _oracle_window()
    for target in sorted(set(int(v) for v in win)) + [int(win.min()) - 1, int(win.max()) + 1]:
        _check(t, target)
        _check(t, target, 4990, 5029)
        _check(t, target, 4000, 6000)


def test_stepper_on_noisy_functions_and_sub_ranges():
    t = _noisy()
    rng = np.random.default_rng(21)
    for _ in range(40):
        a, b = sorted(int(v) for v in rng.integers(1, rr.J_MAX + 1, 2))
        if not rr.grid(a, b):
            continue
        target = int(t[int(rng.integers(a, b + 1))]) + int(rng.integers(-3, 4))
        _check(t, target, a, b)
    for a, b in ((1, 1), (6, 8), (8, 9), (16382, 16383), (1000, 3000)):
        for target in (int(t[a]) - 1, int(t[a]), int(t[b]), int(t[(a + b) // 2])):
            _check(t, target, a, b)


def test_nothing_fits_and_everything_fits():
    t = _ramp()
    for a, b in ((0, 0), (1000, 3000), (5, 5)):
        g = rr.grid(a, b)
        lowest = int(min(t[j] for j in g))
        ref = _check(t, lowest - 1 if (a, b) != (0, 0) else 33, a, b)
        assert ref.j is None and ref.first_size > (lowest - 1)
        top = _check(t, 1 << 40, a, b)
        assert top.j == g[-1] and top.next_j is None
    j, (rounds, used, made), _ = emu_search(t, 33, 0, 0, 3)
    assert j == 0 and used == 13 and rounds == 7


def test_ranges():
    t = _ramp()
    stats = np.zeros(3, np.int32)
    assert lib().emu_rate_search(_p(t), C.c_longlong(100), 7, 7, 3, _p(stats), None) == -1        # no grid entry
    out = np.zeros(20000, np.int32)
    for a, b in ((0, 5), (5, 0), (3, 2), (-1, 4), (1, 16384)):
        assert lib().emu_rate_grid(a, b, _p(out), out.size) == -1
    n = lib().emu_rate_grid(0, 0, _p(out), out.size)
    assert [int(v) for v in out[:n]] == rr.grid()
    n = lib().emu_rate_grid(1000, 3000, _p(out), out.size)
    assert [int(v) for v in out[:n]] == rr.grid(1000, 3000)
    for j in (1, 7, 5000, 16382):
        assert np.float32(lib().emu_rate_q(j)).tobytes() == np.float32(rr.q(j)).tobytes()


# ---- unit-step transform + quantise_kernel --------------------------------------------------------------------------
def _unit_forward(imgs, wl):
    """imgs: padded u8 frames of one size.  Returns (float buffer [n, stride], fused flag)."""
    AH, AW = imgs[0].shape
    stride = (AW * AH + orc.dwt_extra(AW, AH, wl) + 3) // 4 * 4
    src = E.aligned_zeros(len(imgs) * AW * AH, np.uint8)
    for f, im in enumerate(imgs):
        src[f * AW * AH:(f + 1) * AW * AH] = im.ravel()
    out = E.aligned_zeros(len(imgs) * stride, np.float32)
    fused = lib().emu_rate_unit_forward(_p(src), 1, C.c_ulonglong(AW * AH), _p(out), C.c_ulonglong(stride * 4), AW, AH, wl,
                                        len(imgs))
    return out.reshape(len(imgs), stride), bool(fused)


def _quantise(unit, AW, AH, wl, js, c16, max_wgs=0):
    """Returns out[c][f]: int16 or float32 (AH, AW) arrays."""
    n, stride = unit.shape
    K = len(js)
    P = AW * AH
    dst = E.aligned_zeros(K * n * P, np.float32)
    dst.view(np.uint32)[:] = 0xDEADBEEF
    lib().emu_rate_quantise(_p(unit), C.c_ulonglong(stride * 4), _p(dst), C.c_ulonglong(P * 4), AW, AH, wl, n, K,
                            _p(np.array(js, np.int32)), _p(np.array(c16, np.int32)), max_wgs)
    out = []
    for c in range(K):
        row = []
        for f in range(n):
            a = dst[(c * n + f) * P:(c * n + f + 1) * P]
            if c16[c]:
                assert np.all(a.view(np.uint32)[P // 2:] == 0xDEADBEEF)        # an int16 array: the first half only
                row.append(a.view(np.int16)[:P].reshape(AH, AW).copy())
            else:
                row.append(a.reshape(AH, AW).copy())
        out.append(row)
    return out


def _oracle_coef(img, wl, j):
    AH, AW = img.shape
    return orc.dwt_forward(orc.level_shift_fwd(img, True), wl, rr.q(j))[:AW * AH].reshape(AH, AW)


def _assert_forms(got, ref, c16):
    if c16:
        assert np.abs(ref).max() < 32768
        assert np.array_equal(got, np.trunc(ref).astype(np.int16))
    else:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("W,H,wl,js,max_wgs", [
    (200, 136, 3, (9, 2829, 16382), 0),
    (700, 500, 6, (1000, 3098, 9999), 0),          # AW = 704: a subband edge at column 11, inside a group of four
    (1000, 300, 5, (1407, 5000, 16382), 37),       # a capped grid: a workgroup takes several rows
])
def test_quantise_equals_the_fused_transform(W, H, wl, js, max_wgs):
    imgs = [orc.pad_frame(orc.gen_frame(W, H, f)) for f in range(2)]
    AH, AW = imgs[0].shape
    if (W, wl) == (700, 6):
        assert AW == 704 and (AW >> 6) == 11
    unit, fused = _unit_forward(imgs, wl)
    # no grid value makes coef16_ok false at these wl (<= 6, grey; asked at a geometry every level of which takes the
    # vector kernels): one candidate is forced into the float form
    assert all(lib().emu_rate_coef16_ok(wl, j, 128, 1024, 1024) for j in (1, 16382) + tuple(js))
    for forms in ((1, 0, 1), (0, 1, 0)):
        out = _quantise(unit, AW, AH, wl, js, forms, max_wgs)
        for c, j in enumerate(js):
            for f in range(2):
                _assert_forms(out[c][f], _oracle_coef(imgs[f], wl, j), forms[c])
    for K in (1, 2):                                # the one- and two-candidate instantiations
        out = _quantise(unit[:1], AW, AH, wl, js[:K], (1, 0)[:K])
        for c in range(K):
            _assert_forms(out[c][0], _oracle_coef(imgs[0], wl, js[c]), (1, 0)[c])


def test_coef16_ok_false_is_honoured_by_the_c16_switch():
    """PICSONG_C16=0, the existing switch, makes coef16_ok false for every candidate; at wl = 7 the bound itself does for
    the top of the grid."""
    assert lib().emu_rate_coef16_ok(7, 16382, 128, 1024, 1024) == 0 and lib().emu_rate_coef16_ok(7, 5000, 128, 1024, 1024) == 1
    os.environ["PICSONG_C16"] = "0"
    try:
        assert lib().emu_rate_coef16_ok(3, 9, 128, 256, 192) == 0
    finally:
        del os.environ["PICSONG_C16"]


def test_rgb_unit_forward_through_the_fused_ict_head():
    W, H, wl, j = 256, 192, 3, 2829
    planes = [orc.pad_frame(orc.gen_frame(W, H, 60 + c)) for c in range(3)]
    AH, AW = planes[0].shape
    stride = (AW * AH + orc.dwt_extra(AW, AH, wl) + 3) // 4 * 4
    src = [E.aligned_copy(p) for p in planes]
    unit = E.aligned_zeros(3 * stride, np.float32)
    assert lib().emu_rate_unit_forward_rgb(_p(src[0]), _p(src[1]), _p(src[2]), _p(unit), C.c_ulonglong(stride * 4), AW, AH, wl)
    out = _quantise(unit.reshape(3, stride), AW, AH, wl, (j,), (0,))
    comps = orc.rgb_forward(*planes, True)
    for c in range(3):
        ref = orc.dwt_forward(comps[c], wl, rr.q(j))[:AW * AH].reshape(AH, AW)
        assert np.array_equal(out[0][c].view(np.uint32), ref.view(np.uint32)), c


@pytest.mark.parametrize("c16", [1, 0])
def test_coder_and_pack_of_a_candidate_equal_the_oracle_stream(c16):
    W, H, wl, j = 200, 136, 3, 2829
    img = orc.gen_frame(W, H)
    pad = orc.pad_frame(img)
    AH, AW = pad.shape
    lut = orc.lut_for(True, wl)
    unit, _ = _unit_forward([pad], wl)
    coef = _quantise(unit, AW, AH, wl, (1000, j, 9999), (c16,) * 3)[1][0]
    staging, sizes, flag = E.bpc_encode(coef.astype(np.int32) if c16 else coef, wl, lut)
    assert flag == 0
    hdr = orc.header_pack(n_samples=W * H, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=8, lossy=1, qs_1e4=j,
                          components=1, is_rgb=0, height=H, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=0)
    ref = orc.encode_frame(img, wl, True, rr.q(j), lut)
    assert np.array_equal(E.pack(staging, sizes, hdr), ref) and ref.size == 8000
