"""The register diet of the k = 0 two-pass encoder (csrc/bpc_kernels.hpp, PICSONG_ENC_OCC8): a lane no longer holds its
plane's probabilities through the plane but the byte offset of the plane's record in the LDS image, read at the head of
every 4-row group of the significance pass and of every refinement half-pass; the neighbour lanes' columns are moved a
half-pass at a time; the next plane's words are loaded after the refinement's first half.

Every case runs the kernel on the CPU wave emulator -- emu_lib.driver_lib's build of the encoder driver with the switch at 1
(columns and plane load only) and at 2 (the record reads too), whatever the library's default -- and compares staging and
sizes bit for bit with the oracle's bpc_encode.  The cases are the places where such a diet goes wrong: an
idle upper half (its lanes read a record they must not use), halves at different bit-planes in one step, lanes of one
wave in different subbands (different records in one read), more than eight plane steps, a half that drops out for the
raw fallback, dense and generic half-passes in one plane, and a 9/7 frame.

The last test is a guard on the compiled gfx950 text of bpc_encode_kernel<false, false> with the whole diet (=2) at eight waves
a SIMD: 64 registers, and the plane loops still free of scratch traffic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
from test_encoder_spp_dense import check_branch, synth
from test_isa_guards import CSRC, _compile, _kernel_body


def _noise(seed, H, W, top=31):
    return np.random.default_rng(seed).integers(-top, top + 1, (H, W)).astype(np.int32)


def _groups(AW, AH, wl, cb):
    """The (level, subband) of the 32 lanes of codeblock `cb`, as the coder looks them up: at the lane's first column,
    the codeblock's first row."""
    L = orc.lib()
    ncx = AW // 64
    out = []
    for t in range(32):
        lv, sb = C.c_int(), C.c_int()
        L.po_find_subband((cb % ncx) * 64 + 2 * t, (cb // ncx) * 64, AW, AH, wl, C.byref(lv), C.byref(sb))
        out.append((lv.value, sb.value))
    return out


def _one_codeblock():
    return _noise(41, 64, 64), 1


def _msb_apart_by_2():
    c = _noise(42, 64, 128)
    c[:, :64] = _noise(43, 64, 64, top=7)                      # the lower half two planes below the upper one
    m = [int(np.abs(c[:, 64 * h:64 * h + 64]).max()).bit_length() for h in range(2)]
    assert m[1] - m[0] == 2
    return c, 1


def _boundary_between_halves():
    AW, AH, wl = 128, 128, 1
    g0, g1 = set(_groups(AW, AH, wl, 0)), set(_groups(AW, AH, wl, 1))
    assert len(g0) == 1 and len(g1) == 1 and g0 != g1         # one wave, its halves in two subbands
    return _noise(44, AH, AW), wl


def _boundary_inside_codeblock():
    AW, AH, wl = 192, 128, 1
    assert len(set(_groups(AW, AH, wl, 1))) == 2              # x = 96 splits codeblock 1: its lanes read two records
    return _noise(45, AH, AW), wl


def _deep():
    c = orc.deep_coeffs(128, 128, 17)
    assert int(np.abs(c[:64, :64]).max()).bit_length() - 1 >= 8
    return c, 1


def _raw_beside_normal():
    return orc.deep_coeffs(128, 128, 18, raw_cb=1), 1


def _mixed_one():
    c = synth("mixed_one")
    check_branch("mixed_one", c)                              # a dense and a generic half-pass in one plane
    return c, 1


CASES = {"one_codeblock": _one_codeblock, "msb_apart_by_2": _msb_apart_by_2,
         "boundary_between_halves": _boundary_between_halves, "boundary_inside_codeblock": _boundary_inside_codeblock,
         "deep": _deep, "raw_beside_normal": _raw_beside_normal, "mixed_one": _mixed_one}


_libs = {}


def _emu(level):
    """The encoder driver of the emulator, built (emu_lib.driver_lib) with PICSONG_ENC_OCC8=`level`: 1 = the neighbour
    columns a half-pass at a time and the late plane load, 2 = also the plane's record read where it is used."""
    if level not in _libs:
        _libs[level] = E.driver_lib(f"libpicsong_emu_occ8_{level}.so", ("emu_driver.cpp", "emu_runtime.cpp"),
                                    (f"-DPICSONG_ENC_OCC8={level}",))
    return _libs[level]


def _emu_encode(level, coef, wl, lut):
    AH, AW = coef.shape
    coef = np.ascontiguousarray(coef)
    staging = np.empty(AW * AH, np.int32)
    sizes = np.empty((AW // 64) * (AH // 64), np.int32)
    flag = np.zeros(1, np.int32)
    tab = np.ascontiguousarray(lut.table, np.int32)
    geo = E._geo(lut)
    _emu(level).emu_bpc_encode(E._p(coef), int(coef.dtype == np.float32), AW, AH, wl, E._p(tab), E._p(geo),
                               E._p(staging), E._p(sizes), E._p(flag), C.c_float(0.0), 1)
    return staging, sizes, int(flag[0])


def _compare(level, coef, wl, lut):
    st_ref, sz_ref = orc.bpc_encode(coef, wl, lut)
    st, sz, flag = _emu_encode(level, coef, wl, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    for cb in range(sz_ref.size):                             # (past a codeblock's size the staging is not defined)
        n = sz_ref[cb]
        assert np.array_equal(st[cb * 4096:cb * 4096 + n], st_ref[cb * 4096:cb * 4096 + n]), cb
    return st_ref, sz_ref


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_case_equals_oracle(name, level):
    coef, wl = CASES[name]()
    st_ref, sz_ref = _compare(level, np.ascontiguousarray(coef), wl, orc.lut_for(False, wl))
    if name == "raw_beside_normal":
        assert sz_ref[1] == 4096 and sz_ref[0] < 4096
    elif name == "deep":
        assert sz_ref.max() < 4096 and st_ref[0] >= 8
    else:
        assert sz_ref.max() < 4096


@pytest.mark.parametrize("level", [1, 2])
def test_emulated_97_frame_equals_oracle(level):
    """One 9/7 frame, 256 x 128, wl 2, qs 0.5: float coefficients, four waves, LL and detail subbands."""
    AW, AH, wl, qs = 256, 128, 2, 0.5
    x = orc.level_shift_fwd(orc.gen_frame(AW, AH, 0), True)
    coef = np.ascontiguousarray(orc.dwt_forward(x, wl, qs)[:AW * AH].reshape(AH, AW))
    _compare(level, coef, wl, orc.lut_for(True, wl))


def test_compiled_encoder_fits_eight_waves(tmp_path_factory):
    """bpc_encode_kernel<false, false> with the diet on and eight waves a SIMD asked for: at most 64 vector registers, and
    at most 8 scratch instructions from the first interval update (v_mul_u32_u24) on -- the bound tests/test_isa_guards.py
    holds the plane loops to."""
    asm = _compile(tmp_path_factory, "occ8", os.path.join(CSRC, "picsong_hip.hip"),
                   ["-DPICSONG_ENC_OCC8=2", "-DPICSONG_BPC_ENC_WAVES=8"])
    key = "17bpc_encode_kernelILb0ELb0E"
    body = _kernel_body(asm, key)
    i0 = next(i for i, ln in enumerate(body) if "v_mul_u32_u24" in ln)
    tail = [ln for ln in body[i0:] if re.match(r"^\s*scratch_", ln)]
    assert len(tail) <= 8, f"{len(tail)} scratch instructions after the first v_mul_u32_u24"
    name, vgprs = None, None
    for line in asm:
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"^\s*\.amdhsa_next_free_vgpr (\d+)", line)
        if m and name and key in name:
            vgprs = int(m.group(1))
    assert vgprs is not None and vgprs <= 64, vgprs
