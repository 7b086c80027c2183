"""The k = 0 encoder's fully visited significance half-passes (csrc/bpc_kernels.hpp, PICSONG_ENC_SPP_DENSE): a half-pass
(32 rows of a wave's two codeblocks) in which every row has a lane with an insignificant coefficient visits its rows in
order and reads a row's three lane masks -- significant before, becomes significant, becomes significant and negative --
off the carries of the columns' bit-reversed words; every other half-pass takes the generic body with its row-bit tests.
The first plane's body reads its two masks the same way.

Every case runs the kernel on the CPU wave emulator and compares staging and sizes bit for bit with the oracle's
bpc_encode.  The frames are 128 x 64 -- one wave of two codeblocks -- unless they say otherwise.  Which body a half-pass
takes is computed here from the coefficients (half_pass_rows: a row has work if some lane has an insignificant coefficient
in either column before the plane, in a codeblock that codes a plane at that step), and the cases that are there for a
branch assert that they reach it.

`mixed` is two inputs.  One row of EACH 32-row half forced significant from step 0 leaves no dense half-pass at all
(mixed_both: the generic body beside the first plane's carries); a dense and a generic half-pass in ONE plane needs the
hole in one half only (mixed_one, the hole in the lower half; lower_only has its holes in the upper one)."""
import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc

ALL = 0xFFFFFFFF


def half_pass_rows(coef):
    """{(step, hw): rows} of the one wave of a 128 x 64 array, steps >= 1 (step 0 is the first plane's body): bit i of
    rows is set when row 32 hw + i has work."""
    mag = np.abs(np.trunc(np.asarray(coef, np.float64))).astype(np.int64)
    assert mag.shape == (64, 128)
    msb = [int(mag[:, 64 * h:64 * h + 64].max()).bit_length() - 1 for h in range(2)]
    out = {}
    for p in range(1, max(msb) + 1):
        work = np.zeros(64, bool)
        for h in range(2):
            bp = msb[h] - p
            if msb[h] >= 0 and bp >= 0:
                work |= ((mag[:, 64 * h:64 * h + 64] >> (bp + 1)) == 0).any(axis=1)
        for hw in range(2):
            out[(p, hw)] = sum(1 << i for i in range(32) if work[32 * hw + i])
    return out


def ctx8_sites_in_dense(coef):
    """Coefficients coded at a step >= 1 whose eight neighbours are all significant before that step, in a dense
    half-pass (both codeblocks of the input have the same msb)."""
    mag = np.abs(np.asarray(coef)).astype(np.int64)
    rows = half_pass_rows(coef)
    msb = int(mag.max()).bit_length() - 1
    n = 0
    for p in range(1, msb + 1):
        sig = np.zeros((66, 66 + 64), bool)
        for h in range(2):                                   # (a codeblock's neighbours outside it count as zero)
            s = (mag[:, 64 * h:64 * h + 64] >> (msb - p + 1)) != 0
            pad = np.zeros((66, 66), bool)
            pad[1:65, 1:65] = s
            nb = sum(pad[1 + dy:65 + dy, 1 + dx:65 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
            hit = (nb == 8) & ~s
            for hw in range(2):
                if rows[(p, hw)] == ALL:
                    n += int(hit[32 * hw:32 * hw + 32].sum())
    return n


# ---- inputs ------------------------------------------------------------------------------------------------------

def _noise(seed=31, top=31):
    return np.random.default_rng(seed).integers(-top, top + 1, (64, 128)).astype(np.int32)


def _force_rows(c, rows, seed=32):
    """Magnitude 16 .. 31 in all 128 columns of `rows`: significant from step 0 of a block whose msb is 4."""
    rng = np.random.default_rng(seed)
    for r in rows:
        c[r] = rng.integers(16, 32, 128) * rng.choice([-1, 1], 128)
    return c


def _dense():
    return _noise()


def _mixed_both():
    return _force_rows(_noise(), (5, 40))


def _mixed_one():
    return _force_rows(_noise(), (40,))


def _zero_upper():
    c = _noise(33)
    c[:, 64:] = 0
    return c


def _zero_lower():
    c = _noise(34)
    c[:, :64] = 0
    return c


def _two_msb():
    c = _noise(35)
    c[:, 64:] = np.random.default_rng(36).integers(-7, 8, (64, 64))
    return c


def _lower_only():
    return _force_rows(_noise(37), range(0, 32, 2))


def _ctx8():
    """Small coefficients at (r, c), c = 2 (r & 1) mod 4, everything else of magnitude 16 .. 31: every small one has
    eight neighbours significant from step 0 (no two small ones touch), and every row has small ones.  Rows 16 .. 31
    and 48 .. 63 are plain noise, so a half-pass has groups with the gate shut by construction beside the open ones."""
    rng = np.random.default_rng(38)
    c = (rng.integers(16, 32, (64, 128)) * rng.choice([-1, 1], (64, 128))).astype(np.int32)
    small = rng.integers(-15, 16, (64, 128)).astype(np.int32)
    r, x = np.mgrid[0:64, 0:128]
    at = (x % 4) == 2 * (r & 1)
    c[at] = small[at]
    plain = _noise(39)
    for r0 in (16, 48):
        c[r0:r0 + 16] = plain[r0:r0 + 16]
    return c


SYNTH = {"dense": _dense, "mixed_both": _mixed_both, "mixed_one": _mixed_one, "zero_upper": _zero_upper,
         "zero_lower": _zero_lower, "two_msb": _two_msb, "lower_only": _lower_only, "ctx8": _ctx8}
_made = {}


def synth(name):
    if name not in _made:
        c = np.ascontiguousarray(SYNTH[name]())
        c.setflags(write=False)
        _made[name] = c
    return _made[name]


def check_branch(name, coef):
    """The input reaches the branch it is there for."""
    rows = half_pass_rows(coef)
    steps = sorted({p for p, _ in rows})
    dense = {k for k, v in rows.items() if v == ALL}
    generic = {k for k, v in rows.items() if v != ALL and v != 0}
    if name == "dense":
        assert all((p, hw) in dense for p in steps[:3] for hw in (0, 1))      # (the last plane has rows with no zero left)
    if name == "mixed_both":
        assert generic and not dense
    if name == "mixed_one":
        assert any((p, 0) in dense and (p, 1) in generic for p in steps)
    if name == "lower_only":
        assert all((p, 0) not in dense for p in steps) and any((p, 0) in generic and (p, 1) in dense for p in steps)
    if name in ("zero_upper", "zero_lower"):
        assert dense and (np.abs(coef[:, :64]).max() == 0) != (np.abs(coef[:, 64:]).max() == 0)
    if name == "two_msb":
        m = [int(np.abs(coef[:, 64 * h:64 * h + 64]).max()).bit_length() for h in range(2)]
        assert abs(m[0] - m[1]) == 2 and dense
    if name == "ctx8":
        assert ctx8_sites_in_dense(coef) >= 64


@pytest.mark.parametrize("name", sorted(SYNTH))
def test_emulated_synthetic_equals_oracle(name):
    coef = synth(name)
    check_branch(name, coef)
    lut = orc.lut_for(False, 1)
    st_ref, sz_ref = orc.bpc_encode(coef, 1, lut)
    assert sz_ref.max() < 4096                               # (no raw fallback: half_pass_rows does not model it)
    st, sz, flag = E.bpc_encode(coef, 1, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)


def test_emulated_97_frame_equals_oracle():
    """One 9/7 frame, 256 x 128, wl 2, qs 0.5: float coefficients, four waves, LL and detail subbands."""
    AW, AH, wl, qs = 256, 128, 2, 0.5
    x = orc.level_shift_fwd(orc.gen_frame(AW, AH, 0), True)
    coef = np.ascontiguousarray(orc.dwt_forward(x, wl, qs)[:AW * AH].reshape(AH, AW))
    lut = orc.lut_for(True, wl)
    st_ref, sz_ref = orc.bpc_encode(coef, wl, lut)
    st, sz, flag = E.bpc_encode(coef, wl, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)
