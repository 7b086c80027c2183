"""The training statistics kernel (bpc_stats_kernel, picsong_train_coeffs) on the CPU wave emulator
(tests/hipemu/emu_train_driver.cpp) against the reference model (train_ref.py): equal counts, [entry][2], exactly."""
import ctypes as C

import numpy as np
import pytest

import train_cases as tc
import train_ref as tr
from emu_lib import _p, driver_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_train.so", ("emu_train_driver.cpp", "emu_runtime.cpp"))
    return _lib


def _geo9(geo, wl, sized=False):
    n = tr.sections(geo, wl) if sized else (0, 0, 0)
    return np.array([geo["n_bitplanes"], geo["n_subbands"], geo["ctx_ref"], geo["ctx_sign"], geo["ctx_sig"],
                     geo["precision"], *n], np.int32)


def emu_counts(coef, wl, geo=tc.GEO, into=None, max_wgs=0, frames=1):
    """coef: (AH, AW) or (frames, AH, AW) int32 / float32 / int16.  Returns (counts, range flag)."""
    coef = np.ascontiguousarray(coef)
    AH, AW = coef.shape[-2:]
    form = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.int16): 2}[coef.dtype]
    total = sum(tr.sections(geo, wl))
    cnt = np.zeros((total, 2), np.uint64) if into is None else into
    flag = np.zeros(1, np.int32)
    n = lib().emu_train_counts(_p(coef), form, AW, AH, wl, _p(_geo9(geo, wl)), frames,
                               C.c_ulonglong(AW * AH * coef.dtype.itemsize), _p(cnt), _p(flag), max_wgs)
    assert n == total
    return cnt, int(flag[0])


@pytest.mark.parametrize("name", tc.CASES)
def test_kernel_equals_model(name):
    coef, wl = tc.case(name)
    want, wflag = tc.model(name)
    got, flag = emu_counts(coef, wl)
    assert want.sum() > 0
    assert np.array_equal(got, want)
    assert flag == wflag == (1 if name == "zero_and_over" else 0)


def test_deep_case_reaches_plane_15_and_aliases():
    """deep_coeffs has MSB 15: with 15 bit-planes a group, plane 15 of a group is read at plane 0 of the next group --
    no symbol is lost, the entries differ from a 16-plane geometry's."""
    coef, wl = tc.case("deep")
    assert int(np.abs(coef).max()).bit_length() - 1 == 15
    cnt15, _ = tc.model("deep")
    cnt16, _ = tr.counts(coef, wl, dict(tc.GEO, n_bitplanes=16))
    assert cnt15.sum() == cnt16.sum()
    n15, n16 = tr.sections(tc.GEO, wl)[0], tr.sections(dict(tc.GEO, n_bitplanes=16), wl)[0]
    ref15, ref16 = cnt15[:n15].sum(axis=1).reshape(-1, 15), cnt16[:n16].sum(axis=1).reshape(-1, 16)
    assert ref16[:, 15].sum() == 0                       # plane 15 is never refined ...
    sig16 = cnt16[n16:n16 + ref16.size * 9].sum(axis=1).reshape(-1, 16, 9)
    assert sig16[:, 15].sum() > 0                        # ... but its significance is coded: the aliasing index


def test_int16_form_equals_int32():
    coef, wl = tc.case("frame2")
    assert np.abs(coef).max() < 32768
    got, _ = emu_counts(coef.astype(np.int16), wl)
    assert np.array_equal(got, tc.model("frame2")[0])


def test_two_calls_accumulate():
    c0, wl = tc.case("frame1")
    c1, _ = tc.case("zero_and_over")
    cnt, _ = emu_counts(c0, wl)
    cnt, flag = emu_counts(c1, wl, into=cnt)
    assert np.array_equal(cnt, tc.model("frame1")[0] + tc.model("zero_and_over")[0])
    assert flag == 1


def test_persistent_grid_and_frames():
    """Two frames in one launch on a grid of one workgroup: every wave takes several codeblock pairs."""
    c0, wl = tc.case("frame2")
    c1 = tc.frame_coeffs(256, 192, 3, False, 1)
    got, _ = emu_counts(np.stack([c0, c1]), wl, max_wgs=1, frames=2)
    assert np.array_equal(got, tc.model("frame2")[0] + tc.model_of_frame(256, 192, 3, False, 1)[0])


def test_other_geometry():
    """A geometry that is not the shipped one: 12 bit-planes, 5 significance contexts (contexts above 4 alias)."""
    geo = dict(n_bitplanes=12, n_subbands=3, ctx_ref=2, ctx_sign=4, ctx_sig=5, precision=7)
    coef, wl = tc.case("frame1")
    want, _ = tr.counts(coef, wl, geo)
    got, _ = emu_counts(coef, wl, geo)
    assert np.array_equal(got, want)


def test_geometry_beyond_the_lds_copy_is_reported():
    geo = dict(tc.GEO, n_bitplanes=200)
    n = lib().emu_train_counts(None, 0, 128, 128, 1, _p(_geo9(geo, 1)), 1, C.c_ulonglong(0), None, None, 0)
    assert n == -1 and sum(tr.sections(geo, 1)) > lib().emu_train_max_entries()
