"""The fused 5/3 head (dwt_fwd2_kernel, csrc/dwt_kernels.hpp) on the CPU wave emulator, u8 in, int16 out, against the
oracle's transform, at the geometries where its two newer forms can go wrong:

* the interior strips' instantiation without edge selects (PICSONG_DWT_F2_EDGE53): a wave whose 256 columns hold neither
  column 0 nor column W - 4.  Padded width 704 is four strips with exactly one interior, 960 five with three, 192 one strip
  and no interior one (every wave through the instantiation with the selects);
* the 16-pair bands of a call that carries several frames (PICSONG_DWT_F2_PAIRS_BATCH=16: not the library's default, so
  the driver of this file, tests/hipemu/emu_fwd2_driver.cpp, is compiled with it; three frames) beside the lone frame's
  8-pair bands (emu_lib.dwt_forward): height 64 is one 16-pair band that holds both mirrors, 128 two, 192 three, the
  middle one with neither mirror.

wl 2 (level 1 is the transform's last: its LL is a coded int16 subband) and wl 3 (its LL goes on to level 2 as 32 bits)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
from emu_lib import _p, driver_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_fwd2.so", ("emu_fwd2_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes", "-DPICSONG_DWT_F2_PAIRS_BATCH=16"))
    return _lib


WIDTHS = {704: 1, 960: 3, 192: 0}                            # padded width -> interior strips
HEIGHTS = (64, 128, 192)
FRAMES = (31, 32, 33)                                        # gen_frame numbers of the batched call (the lone one: the first)


def interior_strips(W):
    """Strips of the head whose 256 columns hold neither column 0 nor column W - 4 (dwt_fwd2_kernel's test)."""
    useful = lib().emu_f2_useful_cols()
    edge = (256 - useful) // 2
    strips = (W + useful - 1) // useful
    return sum(1 for s in range(strips) if s * useful - edge > 0 and s * useful - edge + 256 < W)


_refs = {}


def oracle_coeffs(W, H, wl, frame):
    key = (W, H, wl, frame)
    if key not in _refs:
        img = orc.gen_frame(W, H, frame)
        assert img.shape == (H, W)
        c = orc.dwt_forward(orc.level_shift_fwd(img, False), wl)[:W * H].reshape(H, W).astype(np.int32)
        assert np.abs(c).max() < 32768
        img.setflags(write=False)
        c.setflags(write=False)
        _refs[key] = (img, c)
    return _refs[key]


@pytest.mark.parametrize("W", sorted(WIDTHS))
def test_geometries_reach_the_interior_instantiation(W):
    assert interior_strips(W) == WIDTHS[W]
    assert lib().emu_f2_pairs_batch() == 16


@pytest.mark.parametrize("wl", [2, 3])
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", sorted(WIDTHS))
def test_lone_frame_equals_oracle(monkeypatch, W, H, wl):
    monkeypatch.delenv("PICSONG_DWT_NOFUSE01", raising=False)
    img, ref = oracle_coeffs(W, H, wl, FRAMES[0])
    E.set_c16(True)
    try:
        buf = E.dwt_forward(np.array(img), wl, False, extra=orc.dwt_extra(W, H, wl))
        assert E.dwt_forward.fused01
        got = E.mallat16(buf, W, H).astype(np.int32)
    finally:
        E.set_c16(False)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("wl", [2, 3])
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", sorted(WIDTHS))
def test_three_frames_in_one_call_equal_oracle(monkeypatch, W, H, wl):
    monkeypatch.delenv("PICSONG_DWT_NOFUSE01", raising=False)
    n = len(FRAMES)
    P, extra = W * H, orc.dwt_extra(W, H, wl)
    frames = E.aligned_zeros(n * P, np.uint8)
    for z, f in enumerate(FRAMES):
        frames[z * P:(z + 1) * P] = oracle_coeffs(W, H, wl, f)[0].ravel()
    out = E.aligned_zeros(n * (P + extra), np.int32)
    flags = lib().emu_dwt_forward_frames(_p(frames), C.c_ulonglong(P), _p(out), C.c_ulonglong((P + extra) * 4), W, H, wl, 0,
                                         C.c_float(1.0), n)
    assert flags & 4, "the 16-bit form applies to these geometries"
    assert flags & 1, "levels 0 and 1 as one launch"
    assert flags & 2, "H is a multiple of 64: whole 16-pair bands, the batched call's own instantiation"
    for z, f in enumerate(FRAMES):
        got = E.mallat16(out[z * (P + extra):(z + 1) * (P + extra)], W, H).astype(np.int32)
        assert np.array_equal(got, oracle_coeffs(W, H, wl, f)[1]), f"frame {z}"
