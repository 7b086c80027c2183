"""The k = 0 encoder's carry-read bodies around their edges (csrc/bpc_kernels.hpp): PICSONG_ENC_SPP_NEAR -- a significance
half-pass with at most PICSONG_ENC_SPP_NEAR_MAX rows without work takes the dense body, a 4-row group with no row set only
shifts its words; PICSONG_ENC_DENSE_NOTEST -- where every visited row has work (rows == 0xFFFFFFFF in the significance
pass, popcount(rows) == last in a dense refinement half-pass) a column's site is not tested for being empty;
PICSONG_ENC_RESET64 -- a fresh codeword's S and L are reset by one 64-bit move.

Every case runs the kernel on the CPU wave emulator -- emu_lib.driver_lib's build of the encoder driver with all three
switches at 1 and NEAR_MAX = 4, whatever the library's defaults -- and compares staging and sizes bit for bit with the
oracle's bpc_encode.  The synthetic frames are 128 x 64, one wave of two codeblocks.  Which body a half-pass takes is
computed here from the coefficients (half_passes), and test_every_new_body_is_entered asserts that the cases between them
reach each new body; the cases that are there for one body assert that they reach it.

Wrong variants run once through this file and not kept: the words of a skipped group not shifted fails empty_group, the
one case with such a group; the pair's halves swapped (S = 0, L = 0xFFFF) fails all eleven encodes; the sign site's test
dropped with the others fails NOTHING, and cannot: a sign site with no lane is as much a no-op as an empty significance
site -- that test is kept for its speed (it skips a whole update and is taken), not for the result."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc

ALL = 0xFFFFFFFF
NEAR_MAX = 4
FLAGS = ("-DPICSONG_ENC_SPP_NEAR=1", f"-DPICSONG_ENC_SPP_NEAR_MAX={NEAR_MAX}", "-DPICSONG_ENC_DENSE_NOTEST=1",
         "-DPICSONG_ENC_RESET64=1")
_lib = None


def _emu():
    global _lib
    if _lib is None:
        _lib = E.driver_lib("libpicsong_emu_spp_near.so", ("emu_driver.cpp", "emu_runtime.cpp"), FLAGS)
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


def half_passes(coef):
    """The half-passes of the one wave of a 128 x 64 array at steps >= 1, as the kernel classes them:
    {(step, hw): (sig, ref)}.  sig: 'full' (every row has work: no empty-site tests), 'near' (1 .. NEAR_MAX rows
    without), 'near_group' (near, and a whole 4-row group without), 'generic', None (no row has work); ref: 'notest'
    (dense, every visited row has work), 'dense', 'generic', None.  Then the empty column sites met: {(step, hw): (in a
    'full' significance half-pass, in a 'notest' refinement half-pass)}."""
    mag = np.abs(np.trunc(np.asarray(coef, np.float64))).astype(np.int64)
    assert mag.shape == (64, 128)
    msb = [int(mag[:, 64 * h:64 * h + 64].max()).bit_length() - 1 for h in range(2)]
    cls, empty = {}, {}
    for p in range(1, max(msb) + 1):
        ins = np.zeros((64, 2), bool)                        # row, column of a lane: some lane has an insignificant coefficient
        sg = np.zeros((64, 2), bool)                         # ... a significant one
        for h in range(2):
            bp = msb[h] - p
            if msb[h] >= 0 and bp >= 0:
                s = (mag[:, 64 * h:64 * h + 64] >> (bp + 1)) != 0
                for col in range(2):
                    ins[:, col] |= (~s[:, col::2]).any(axis=1)
                    sg[:, col] |= s[:, col::2].any(axis=1)
        for hw in range(2):
            w = ins[32 * hw:32 * hw + 32]
            rows = w.any(axis=1)
            nwo = 32 - int(rows.sum())
            if nwo == 32:
                sig = None
            elif nwo == 0:
                sig = "full"
            elif nwo <= NEAR_MAX:
                sig = "near_group" if (~rows.reshape(8, 4).any(axis=1)).any() else "near"
            else:
                sig = "generic"
            r = sg[32 * hw:32 * hw + 32]
            rrows = r.any(axis=1)
            pop = int(rrows.sum())
            last = 0 if pop == 0 else 32 - int(np.argmax(rrows[::-1]))
            if pop == 0:
                ref = None
            elif 5 * pop >= 3 * last:
                ref = "notest" if pop == last else "dense"
            else:
                ref = "generic"
            cls[(p, hw)] = (sig, ref)
            empty[(p, hw)] = (int((~w).sum()) if sig == "full" else 0, int((~r[:last]).sum()) if ref == "notest" else 0)
    return cls, empty


# ---- inputs ------------------------------------------------------------------------------------------------------

def _noise(seed, top=31):
    return np.random.default_rng(seed).integers(-top, top + 1, (64, 128)).astype(np.int32)


def _force(c, rows, cols=slice(None), seed=52):
    """Magnitude 16 .. 31 at `cols` of `rows`: significant from step 0 of a block whose msb is 4."""
    rng = np.random.default_rng(seed)
    for r in rows:
        n = c[r, cols].size
        c[r, cols] = rng.integers(16, 32, n) * rng.choice([-1, 1], n)
    return c


def _near_1():
    return _force(_noise(61), (40,))


def _near_max():
    return _force(_noise(62), (34, 40, 45, 51))              # four rows of the upper half-pass, no two in one group


def _near_max_plus_1():
    return _force(_noise(63), (34, 40, 45, 51, 57))


def _empty_group():
    return _force(_noise(64), (40, 41, 42, 43))              # group 2 of the upper half-pass has no row with work


def _empty_sig_site():
    """Row 9: the left column of every lane significant from step 0, the right ones noise -- the row has work, its left
    site has no lane."""
    return _force(_noise(65), (9,), slice(0, None, 2))


def _empty_ref_site():
    """Row 20: every left coefficient of magnitude <= 1 -- significant at no refinement pass -- the right ones noise."""
    c = _noise(66)
    c[20, 0::2] = np.random.default_rng(67).integers(-1, 2, 64)
    return c


def _ref_hole():
    """Row 44 of magnitude <= 1 in every column: the refinement's upper half-pass is dense with a row without work, so it
    keeps its empty tests beside the lower one's untested loop."""
    c = _noise(72)
    c[44] = np.random.default_rng(73).integers(-1, 2, 128)
    return c


def _zero_upper():
    c = _force(_noise(68), (40,))
    c[:, 64:] = 0
    return c


def _zero_lower():
    c = _force(_noise(69), (9,), slice(0, None, 2))
    c[:, :64] = 0
    return c


def _raw():
    """The second codeblock runs out of codeword slots and ends as raw words; the first one codes beside it."""
    c = _noise(70)
    c[:, 64:] = np.random.default_rng(71).integers(-30000, 30001, (64, 64))
    return c


SYNTH = {"near_1": _near_1, "near_max": _near_max, "near_max_plus_1": _near_max_plus_1, "empty_group": _empty_group,
         "empty_sig_site": _empty_sig_site, "empty_ref_site": _empty_ref_site, "ref_hole": _ref_hole, "zero_upper": _zero_upper,
         "zero_lower": _zero_lower, "raw": _raw}
_made = {}


def synth(name):
    if name not in _made:
        c = np.ascontiguousarray(SYNTH[name]())
        c.setflags(write=False)
        _made[name] = (c, half_passes(c))
    return _made[name]


def check_branch(name, cls, empty):
    """The input reaches the branch it is there for."""
    sigs = {k: v[0] for k, v in cls.items()}
    if name in ("near_1", "near_max"):
        assert any(v == "near" for v in sigs.values()) and "generic" not in sigs.values()
        assert any(sigs[(p, 0)] == "full" and sigs[(p, 1)] == "near" for p, _ in sigs)
    if name == "near_max_plus_1":
        assert all(v == "generic" for (p, hw), v in sigs.items() if hw == 1)
        assert all(v == "full" for (p, hw), v in sigs.items() if hw == 0 and p <= 3)
    if name == "empty_group":
        assert any(v == "near_group" for v in sigs.values())
    if name in ("empty_sig_site", "zero_lower"):
        assert sum(e[0] for e in empty.values()) >= 3        # row 9's left site in every plane below the first
    if name == "empty_ref_site":
        assert sum(e[1] for e in empty.values()) >= 3        # row 20's left site in every refinement pass
    if name == "zero_upper":
        assert any(v == "near" for v in sigs.values())
    if name == "ref_hole":
        assert any(cls[(p, 0)][1] == "notest" and cls[(p, 1)][1] == "dense" for p, _ in cls)


@pytest.mark.parametrize("name", sorted(SYNTH))
def test_emulated_synthetic_equals_oracle(name):
    coef, (cls, empty) = synth(name)
    check_branch(name, cls, empty)
    if name in ("zero_upper", "zero_lower"):
        assert (np.abs(coef[:, :64]).max() == 0) != (np.abs(coef[:, 64:]).max() == 0)
    st_ref, sz_ref = _compare(coef, 1, orc.lut_for(False, 1))
    if name == "raw":
        assert sz_ref[1] == 4096 and sz_ref[0] < 4096         # (all 4096 words of the raw codeblock are compared)
    else:
        assert sz_ref.max() < 4096                           # (no raw fallback: half_passes does not model it)


def test_every_new_body_is_entered():
    seen_sig, seen_ref = set(), set()
    e_sig = e_ref = 0
    for name in SYNTH:
        if name == "raw":
            continue
        _, (cls, empty) = synth(name)
        seen_sig |= {v[0] for v in cls.values()}
        seen_ref |= {v[1] for v in cls.values()}
        e_sig += sum(e[0] for e in empty.values())
        e_ref += sum(e[1] for e in empty.values())
    assert {"full", "near", "near_group", "generic"} <= seen_sig
    assert {"notest", "dense"} <= seen_ref
    assert e_sig > 0 and e_ref > 0


def test_emulated_97_frame_equals_oracle():
    """One 9/7 frame, 256 x 128, wl 2, qs 0.5: float coefficients, four waves, LL and detail subbands."""
    AW, AH, wl, qs = 256, 128, 2, 0.5
    x = orc.level_shift_fwd(orc.gen_frame(AW, AH, 0), True)
    coef = np.ascontiguousarray(orc.dwt_forward(x, wl, qs)[:AW * AH].reshape(AH, AW))
    _compare(coef, wl, orc.lut_for(True, wl))
