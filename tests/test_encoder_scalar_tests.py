"""The k = 0 encoder's wave-uniform tests kept scalar in its carry-read bodies (csrc/bpc_kernels.hpp):
PICSONG_ENC_SIGN_TEST_SCALAR -- the test around a carry-read coefficient's sign site is a scalar compare;
PICSONG_ENC_SPP_ONM_CARRY -- the dense significance body shifts the bit-reversed COMPLEMENT of A, so a carry is the site's
lane mask itself; PICSONG_ENC_REF_SCALAR_COUNT -- the dense refinement loops count their rows in an SGPR;
PICSONG_ENC_RESERVE_ONE_TEST -- a site enters the reservation without a scalar pre-test of its mask, an empty mask opens an
empty region.

Every case runs the kernel on the CPU wave emulator -- emu_lib.driver_lib's build of the encoder driver with all four
switches at 1, whatever the library's defaults -- and compares staging and sizes bit for bit with the oracle's bpc_encode.
The second and the fourth switch change C++ that the emulator runs (the complemented word and its idle half; a
reservation entered with no lane); the first and the third are forms of unchanged logic that exist on the GPU alone, and
what can be held of them without one is the compiled text: test_compiled_encoder_holds_the_static_conditions.

The synthetic frames are single waves.  Which body a half-pass takes is computed from the coefficients
(test_encoder_spp_near.half_passes; with PICSONG_ENC_SPP_NEAR off a nearly full half-pass is a generic one), and
test_every_body_is_entered asserts that the cases between them reach the first plane's body, the dense significance body,
both dense refinement loops and the generic bodies.

Wrong variants, each run once through this file and not kept (profiles/NOTES.md has the outcomes): the complement left
out of the dense body's word; the lanes outside an entered reservation left switched off for the site's update; the
dense refinement loops a row short."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
import test_encoder_spp_dense as D
import test_encoder_spp_near as N
from test_isa_guards import CSRC, _compile, _kernel_body

SWITCHES = ("PICSONG_ENC_SIGN_TEST_SCALAR", "PICSONG_ENC_SPP_ONM_CARRY", "PICSONG_ENC_REF_SCALAR_COUNT",
            "PICSONG_ENC_RESERVE_ONE_TEST")
FLAGS = tuple(f"-D{s}=1" for s in SWITCHES)
_lib = None


def _emu():
    global _lib
    if _lib is None:
        _lib = E.driver_lib("libpicsong_emu_scalar_tests.so", ("emu_driver.cpp", "emu_runtime.cpp"), FLAGS)
    return _lib


def _emu_encode(coef, wl, lut):
    AH, AW = coef.shape
    coef = np.ascontiguousarray(coef)
    staging = np.empty(AW * AH, np.int32)
    sizes = np.empty((AW // 64) * (AH // 64), np.int32)
    flag = np.zeros(1, np.int32)
    tab = np.ascontiguousarray(lut.table, np.int32)
    geo = E._geo(lut)
    _emu().emu_bpc_encode(E._p(coef), int(coef.dtype == np.float32), AW, AH, wl, E._p(tab), E._p(geo),
                          E._p(staging), E._p(sizes), E._p(flag), C.c_float(0.0), 1)
    return staging, sizes, int(flag[0])


def _compare(coef, wl, lut):
    st_ref, sz_ref = orc.bpc_encode(coef, wl, lut)
    st, sz, flag = _emu_encode(coef, wl, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    for cb in range(sz_ref.size):                             # (past a codeblock's size the staging is not defined)
        n = sz_ref[cb]
        assert np.array_equal(st[cb * 4096:cb * 4096 + n], st_ref[cb * 4096:cb * 4096 + n]), cb
    return st_ref, sz_ref


# ---- inputs: 128 x 64, one wave of two codeblocks --------------------------------------------------------------------
# dense: noise, every half-pass below the first plane full;  empty_sign: the left column of row 9 significant from step 0
# in every lane -- in a full half-pass that site has no lane, so its sign mask is empty and the sign site is skipped;
# ref_hole: row 44 of magnitude <= 1, a dense refinement half-pass with a row without work beside one without such a
# row;  zero_lower / zero_upper: a zero codeblock as one half (its complemented word is 0);  raw: the second codeblock
# passes 4094 codewords and ends as raw words beside one that codes;  mixed_one: a full and a generic significance
# half-pass in one plane;  sparse_ref: refinement half-passes with few rows.
def _sparse_ref():
    """Magnitudes <= 1 but for five rows of noise: the refinement passes find three rows of 32 with work in the lower
    half-pass and two in the upper one -- too few for the dense loops, the generic refinement body."""
    c = np.random.default_rng(82).integers(-1, 2, (64, 128)).astype(np.int32)
    c[[3, 20, 31, 35, 60]] = D._noise(83)[[3, 20, 31, 35, 60]]
    return c


SYNTH = {"dense": D._dense, "empty_sign": N._empty_sig_site, "ref_hole": N._ref_hole, "zero_lower": D._zero_lower,
         "zero_upper": D._zero_upper, "raw": N._raw, "mixed_one": D._mixed_one, "sparse_ref": _sparse_ref}
_made = {}


def synth(name):
    if name not in _made:
        c = np.ascontiguousarray(SYNTH[name]())
        c.setflags(write=False)
        _made[name] = (c, N.half_passes(c))
    return _made[name]


def bodies(cls):
    """The bodies the half-passes of N.half_passes' classes take in this build (PICSONG_ENC_SPP_NEAR off)."""
    sig = {"full": "dense", "near": "generic", "near_group": "generic", "generic": "generic", None: None}
    return {sig[v[0]] for v in cls.values()} - {None}, {v[1] for v in cls.values()} - {None}


def check_branch(name, coef, cls, empty):
    """The input reaches the branch it is there for."""
    if name == "dense":
        steps = sorted({p for p, _ in cls})
        assert all(cls[(p, hw)][0] == "full" for p in steps[:3] for hw in (0, 1))
    if name == "empty_sign":
        assert sum(e[0] for e in empty.values()) >= 3        # row 9's left site in every plane below the first
    if name == "ref_hole":
        assert any(cls[(p, 0)][1] == "notest" and cls[(p, 1)][1] == "dense" for p, _ in cls)
    if name in ("zero_lower", "zero_upper"):
        assert (np.abs(coef[:, :64]).max() == 0) != (np.abs(coef[:, 64:]).max() == 0)
        assert any(v[0] == "full" for v in cls.values())
    if name == "sparse_ref":
        assert any(v[1] == "generic" for v in cls.values())
    if name == "mixed_one":
        assert any(cls[(p, 0)][0] == "full" and cls[(p, 1)][0] not in ("full", None) for p, _ in cls)


@pytest.mark.parametrize("name", sorted(SYNTH))
def test_emulated_synthetic_equals_oracle(name):
    coef, (cls, empty) = synth(name)
    check_branch(name, coef, cls, empty)
    st_ref, sz_ref = _compare(coef, 1, orc.lut_for(False, 1))
    if name == "raw":
        assert sz_ref[1] == 4096 and sz_ref[0] < 4096         # (all 4096 words of the raw codeblock are compared)
    else:
        assert sz_ref.max() < 4096                           # (no raw fallback: half_passes does not model it)


def test_every_body_is_entered():
    seen_sig, seen_ref = set(), set()
    for name in SYNTH:
        if name == "raw":
            continue
        coef, (cls, _) = synth(name)
        assert np.abs(coef).max() > 0                        # step 0: the first plane's body
        s, r = bodies(cls)
        seen_sig |= s
        seen_ref |= r
    assert {"dense", "generic"} <= seen_sig
    assert {"notest", "dense", "generic"} <= seen_ref


def test_emulated_single_codeblock_equals_oracle():
    """64 x 64: one wave whose upper half is no codeblock -- idle from the first plane on."""
    coef = np.random.default_rng(81).integers(-31, 32, (64, 64)).astype(np.int32)
    _, sz_ref = _compare(coef, 1, orc.lut_for(False, 1))
    assert sz_ref.size == 1 and sz_ref[0] < 4096


def test_emulated_97_frame_equals_oracle():
    """One 9/7 frame, 256 x 128, wl 2, qs 0.5: float coefficients, four waves, LL and detail subbands."""
    AW, AH, wl, qs = 256, 128, 2, 0.5
    x = orc.level_shift_fwd(orc.gen_frame(AW, AH, 0), True)
    coef = np.ascontiguousarray(orc.dwt_forward(x, wl, qs)[:AW * AH].reshape(AH, AW))
    _compare(coef, wl, orc.lut_for(True, wl))


def test_compiled_encoder_holds_the_static_conditions(tmp_path_factory):
    """bpc_encode_kernel<false, false> with all four switches on, in the compiled gfx950 text: no 64-bit vector compare;
    no s_not_b64 of a v_add_co_u32's carry; no row counter in a vector register (v_add_co_u32_e32 v, vcc, 1, v); at most
    72 vector registers and seven waves a SIMD; at most 2 scratch instructions from the first interval update on."""
    asm = _compile(tmp_path_factory, "scalar_tests", os.path.join(CSRC, "picsong_hip.hip"), list(FLAGS))
    key = "17bpc_encode_kernelILb0ELb0E"
    start = next(i for i, ln in enumerate(asm) if re.match(r"^_ZN7picsong\S*" + key + r"\S*:", ln))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    assert len(_kernel_body(asm, key)) > (end - start) // 2   # (the kernel's one exit is at its end)
    body = [ln.split(";")[0].strip() for ln in asm[start:end]]
    body = [ln for ln in body if ln]
    assert not [ln for ln in body if re.match(r"v_cmp_(eq|ne)_u64", ln)]
    assert not [ln for ln in body if re.match(r"v_add_co_u32_e32 v\d+, vcc, 1, v\d+$", ln)]
    for i, ln in enumerate(body):
        m = re.match(r"s_not_b64 s\[\d+:\d+\], (s\[\d+:\d+\])$", ln)
        if not m:
            continue
        # the instruction that wrote the complemented pair: the nearest one above that names it as a destination
        src = re.escape(m.group(1))
        w = next((x for x in reversed(body[:i]) if re.match(r"\S+ (v\d+, )?" + src + r"(,|$)", x)), "")
        assert not w.startswith("v_add_co_u32"), f"'{ln}' complements the carry of '{w}'"
    i0 = next(i for i, ln in enumerate(body) if "v_mul_u32_u24" in ln)
    tail = [ln for ln in body[i0:] if ln.startswith("scratch_")]
    assert len(tail) <= 2, f"{len(tail)} scratch instructions after the first v_mul_u32_u24"
    occ = next(int(m.group(1)) for m in (re.match(r"^; Occupancy: (\d+)", ln) for ln in asm[start:]) if m)
    assert occ == 7, occ
    name, vgprs = None, None
    for line in asm:
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"^\s*\.amdhsa_next_free_vgpr (\d+)", line)
        if m and name and key in name:
            vgprs = int(m.group(1))
    assert vgprs is not None and vgprs <= 72, vgprs
