"""The pieces of the n-frame RGB search calls on the CPU wave emulator (tests/hipemu/emu_rgb_search_driver.cpp):
rgb_sse_kernel -- the inverse ICT and the SSE in one pass -- against the oracle's inverse ICT and numpy, the probe
sequence of launch_seq.hpp over n RGB frames against the oracle's decode of its own encode, the candidate-count function
and the size walk of rate_search.hpp."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
import quality_ref as qr
import rate_ref as rr
import rgb_search_ref as ref
from emu_lib import _p, driver_lib

_lib = None
ULL = C.c_ulonglong
CANARY = 0xABCDEF0123456789


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_rgb_search.so", ("emu_rgb_search_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
    return _lib


# ---- rgb_sse_kernel -------------------------------------------------------------------------------------------------
# (W, H) in padded arrays of AW x AH: a whole last group, W % 4 = 1, and an image smaller than a tile
SHAPES = [(200, 136, 256, 192), (201, 137, 256, 192), (7, 5, 64, 64)]


def _data(W, H, AW, AH, n, c_extra, in_extra, seed):
    """n frames of random float components (most pixels inside 0..255, some far outside at both ends) and random input
    planes.  Returns (comp, c_stride, rgb, in_stride): comp a flat float32 array, plane z at z * c_stride floats; rgb three
    flat u8 arrays, frame f at f * in_stride bytes."""
    P = AW * AH
    rng = np.random.default_rng(seed)
    cz, iz = P + c_extra, P + in_extra
    comp = E.aligned_zeros(3 * n * cz, np.float32)
    comp[:] = rng.normal(0.0, 60.0, comp.size).astype(np.float32)
    for z in range(3 * n):
        if z % 3:
            comp[z * cz:z * cz + P] *= np.float32(0.5)
    far = rng.integers(0, comp.size, comp.size // 50)
    comp[far] = rng.choice(np.array([-900.0, 900.0, -131.4, 127.6], np.float32), far.size)
    for f in range(n):                                      # ... and in every frame's first and last visible pixel
        y = comp[3 * f * cz:3 * f * cz + P].reshape(AH, AW)
        y[0, 0], y[H - 1, W - 1] = -900.0, 900.0
    rgb = [E.aligned_zeros(n * iz, np.uint8) for _ in range(3)]
    for p in rgb:
        p[:] = rng.integers(0, 256, p.size)
    return comp, cz, rgb, iz


def _model(comp, cz, rgb, iz, W, H, AW, AH, n):
    """[3 n] sums: the oracle's inverse ICT of every frame, quality_ref.sse over the visible part."""
    P = AW * AH
    out = []
    for f in range(n):
        pix = orc.rgb_inverse(*[comp[(3 * f + k) * cz:(3 * f + k) * cz + P] for k in range(3)])
        for k in range(3):
            out.append(qr.sse(pix[k].reshape(AH, AW)[:H, :W], rgb[k][f * iz:f * iz + P].reshape(AH, AW)[:H, :W]))
    return out


def _emu(comp, cz, rgb, iz, W, H, AW, n, max_wgs=0, short_run=0, fused=1, want_ran=True):
    out = np.full(3 * n + 1, CANARY, np.uint64)
    ran = lib().emu_rgb_sse(_p(comp), ULL(cz * 4), ULL(AW), _p(rgb[0]), _p(rgb[1]), _p(rgb[2]), ULL(iz), ULL(AW), W, H, n, 128, _p(out),
                            max_wgs, short_run, fused)
    assert out[3 * n] == CANARY                             # nothing behind out[3 n)
    assert bool(ran) == want_ran
    return [int(v) for v in out[:3 * n]]


def _unfused(comp, cz, rgb, iz, W, H, AW, AH, n):
    out = np.full(3 * n + 1, CANARY, np.uint64)
    pix = E.aligned_zeros(3 * n * AW * AH, np.uint8)
    assert lib().emu_rgb_sse_unfused(_p(comp), ULL(cz * 4), _p(rgb[0]), _p(rgb[1]), _p(rgb[2]), ULL(iz), W, H, AW, AH, n, 128, _p(pix),
                                     _p(out)) == 0
    assert out[3 * n] == CANARY
    return [int(v) for v in out[:3 * n]]


@pytest.mark.parametrize("W,H,AW,AH", SHAPES)
def test_rgb_sse_of_three_frames_equals_the_model_and_the_unfused_launches(W, H, AW, AH):
    n = 3
    comp, cz, rgb, iz = _data(W, H, AW, AH, n, 4096, 160, W)          # strides above P
    want = _model(comp, cz, rgb, iz, W, H, AW, AH, n)
    assert min(want) > 0 and len(set(want)) == 3 * n
    # values that clamp at both ends are among the visible pixels
    P = AW * AH
    vis = np.concatenate([comp[z * cz:z * cz + P].reshape(AH, AW)[:H, :W].ravel() for z in range(0, 3 * n, 3)])
    assert (vis < -200).any() and (vis > 200).any()
    for max_wgs in (0, 1, 2):                               # one workgroup spans the frames
        assert _emu(comp, cz, rgb, iz, W, H, AW, n, max_wgs) == want, max_wgs
    assert _emu(comp, cz, rgb, iz, W, H, AW, n, 1, short_run=1) == want
    assert _unfused(comp, cz, rgb, iz, W, H, AW, AH, n) == want
    # padding that differs counts for nothing: the columns [W, AW) and the rows [H, AH) of both sides
    comp2, rgb2 = comp.copy(), [p.copy() for p in rgb]
    comp2, rgb2 = E.aligned_copy(comp2), [E.aligned_copy(p) for p in rgb2]
    for z in range(3 * n):
        a = comp2[z * cz:z * cz + P].reshape(AH, AW)
        a[:, W:] += np.float32(77.0)
        a[H:, :] -= np.float32(55.0)
    for p in rgb2:
        for f in range(n):
            b = p[f * iz:f * iz + P].reshape(AH, AW)
            b[:, W:] ^= 0xFF
            b[H:, :] ^= 0xFF
    assert _emu(comp2, cz, rgb2, iz, W, H, AW, n, 2) == want


def test_rgb_sse_widens_before_a_run_overflows():
    """The short-run instantiation on ONE workgroup: 64 x 192 groups over 256 lanes are 48 groups a lane, six runs of two
    tiles; the pixels 0 against 255 on every channel, so that a wrong run boundary would show in every lane's sum."""
    W, H, AW, AH = 256, 192, 256, 192
    P = AW * AH
    comp = E.aligned_zeros(3 * P, np.float32)
    comp[:P] = -500.0                                       # Y far below: R = G = B = 0
    rgb = [E.aligned_zeros(P, np.uint8) for _ in range(3)]
    for p in rgb:
        p[:] = 255
    want = [W * H * 65025] * 3
    assert _emu(comp, P, rgb, P, W, H, AW, 1, 1, short_run=1) == want
    assert _emu(comp, P, rgb, P, W, H, AW, 1, 1) == want


def test_selector_refuses_what_the_loads_cannot_take():
    W, H, AW, AH = 200, 136, 256, 192
    n = 2
    comp, cz, rgb, iz = _data(W, H, AW, AH, n, 4, 4, 5)
    want = _model(comp, cz, rgb, iz, W, H, AW, AH, n)
    assert _emu(comp, cz, rgb, iz, W, H, AW, n) == want
    # the switch off, float planes 4 bytes off, a plane stride that is no multiple of 16 bytes, an input plane 1 byte off,
    # an input stride that is no multiple of 4: no launch, the caller runs the unfused sequence
    assert _emu(comp, cz, rgb, iz, W, H, AW, n, fused=0, want_ran=False) == [CANARY] * (3 * n)
    assert _emu(comp[1:], cz, rgb, iz, W, H, AW, 1, want_ran=False) == [CANARY] * 3
    assert _emu(comp, cz + 1, rgb, iz, W, H, AW, 1, want_ran=False) == [CANARY] * 3
    assert _emu(comp, cz, [rgb[0][1:], rgb[1], rgb[2]], iz, W, H, AW, 1, want_ran=False) == [CANARY] * 3
    assert _emu(comp, cz, rgb, iz + 1, W, H, AW, n, want_ran=False) == [CANARY] * (3 * n)
    # an input stride is not looked at for one frame; input planes 4 bytes off are fine
    off4 = [E.aligned_zeros(p.size + 16, np.uint8) for p in rgb]
    for o, p in zip(off4, rgb):
        o[4:4 + p.size] = p
    assert _emu(comp, cz, [o[4:] for o in off4], iz, W, H, AW, n) == want


# ---- the probe sequence over n RGB frames ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(200, 136), (201, 137)])
def test_probe_of_two_rgb_frames_equals_the_reference_sse(W, H):
    wl, n = 3, 2
    limit, j, per = ref.check_quality(W, H, wl, n)
    assert per == ref.CASES[(W, H, wl, n)][12]
    stack = [E.aligned_copy(p) for p in ref.padded_stack(W, H, n)]
    AH, AW = stack[0].shape[1:]
    want = [v for fr in per for v in fr]
    for fused in (1, 0):
        out = np.full(3 * n + 1, CANARY, np.uint64)
        took = lib().emu_rgb_probe(_p(stack[0]), _p(stack[1]), _p(stack[2]), ULL(AW * AH), W, H, AW, AH, wl, n, j, _p(out), fused)
        assert took == fused, "the driver's buffers allow the fused tail; the switch turns it off"
        assert out[3 * n] == CANARY and [int(v) for v in out[:3 * n]] == want, fused


# ---- candidates a round, and the walk -------------------------------------------------------------------------------
def test_candidates_a_round():
    f = lib().emu_rgb_search_candidates
    for n in range(1, 22):
        assert f(1, n, 0) == (3 if n <= 7 else 1), n       # a size round: 3 * 3 n planes in one coder launch of 64
        assert f(0, n, 0) == 3                              # a quality round launches no coder
        assert f(1, n, 1) == 1 and f(0, n, 1) == 1          # PICSONG_RATE_K=1


def _walk(table, limit, j_min, j_max, K):
    stats = np.zeros(3, np.int32)
    j = lib().emu_rgb_size_walk(_p(np.ascontiguousarray(table, np.uint64)), ULL(limit), j_min, j_max, K, _p(stats))
    return j, tuple(int(v) for v in stats)


def test_size_walk_gives_the_procedures_result_for_one_and_three_candidates():
    rng = np.random.default_rng(77)
    j = np.arange(rr.J_MAX + 1, dtype=np.int64)
    table = 200 + j * 5 + rng.integers(0, 60, j.size)      # rising, not monotone
    assert np.any(np.diff(table) < 0)
    cases = [(int(table[5000]), 0, 0), (int(table[5000]) + 3, 0, 0), (199, 0, 0), (1 << 40, 0, 0), (int(table[2000]), 1000, 3000),
             (int(table[1000]) - 100, 1000, 3000), (int(table[8]), 8, 9), (int(table[6]), 6, 8)]
    for limit, a, b in cases:
        want = rr.bisect(lambda v: table[v], limit, a, b)
        j1, (rounds1, used1, made1) = _walk(table, limit, a, b, 1)
        j3, (rounds3, used3, made3) = _walk(table, limit, a, b, 3)
        assert j1 == j3 == (want.j or 0), (limit, a, b)
        assert used1 == used3 == len(want.probes) == rounds1 == made1
        assert rounds3 == (used3 + 1) // 2 and made3 <= 3 * rounds3
