"""The k = 0 encoder's prologue on the frame paths' int16 array (enc_transpose_pass<2>, csrc/bpc_kernels.hpp,
PICSONG_ENC_PROLOGUE_PK16): a row's dword is the lane's two coefficients, and the magnitudes, their plane bytes, the OR of
the magnitudes and the signs are all taken from the packed halves.  Each input is one at which that form can go wrong,
and each is compared whole with the oracle's output:

* 5/3 and 9/7 coefficients of a photographic frame, the 9/7 ones at a quantiser step that leaves codeblocks with MSB >= 8,
  so that the second transposition pass (planes 8..15: byte 1 of the left half, byte 3 of the right) runs -- asserted from
  the MSB words (word 0 of a codeblock's staging: short 9 + 2 cb of the stream);
* codeblocks in which both of a lane's coefficients are negative, only the left one, only the right one (bits 15 and 31
  of the raw word), with magnitudes on both sides of 256;
* a codeblock holding -32768, whose magnitude does not fit a signed half: bit 15, as the 32-bit form gives it.

Without a GPU the encoder runs on the CPU wave emulator; with one (-m gpu) the frames go through picsong_encode_frame and
picsong_encode_frames, whose coder reads the int16 array."""
import os

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc

PHOTO = (256, 256, 3)                                        # AW, AH, wl
QS97 = 1.0                                                   # (a context takes qs in (0, 1])
_made = {}


def photo_coeffs(lossy, frame=9):
    """Truncated toward zero, as the coder reads them (and as the head writes the int16 array)."""
    key = ("photo", lossy, frame)
    if key not in _made:
        AW, AH, wl = PHOTO
        x = orc.level_shift_fwd(orc.gen_frame(AW, AH, frame), lossy)
        c = orc.dwt_forward(x, wl, QS97 if lossy else 1.0)[:AW * AH].reshape(AH, AW)
        c = np.ascontiguousarray(np.trunc(c).astype(np.int32))
        c.setflags(write=False)
        _made[key] = c
    return _made[key]


def sign_cases():
    """256 x 64, two waves.  Codeblock 0: every coefficient <= 0 (both halves of every word negative or zero), magnitudes
    below 256; codeblock 1: the left (even) columns <= 0, the right ones >= 0; codeblock 2: the other way round; codeblock 3:
    mixed.  Codeblocks 1-3 have sparse spikes up to 30000 (MSB 14: both passes)."""
    if "signs" not in _made:
        rng = np.random.default_rng(41)
        mag = rng.integers(0, 4, (64, 256)) * (rng.random((64, 256)) < 0.4)
        mag[:, :64] += (rng.random((64, 64)) < 0.02) * rng.integers(0, 200, (64, 64))
        mag[:, 64:] += (rng.random((64, 192)) < 0.01) * rng.integers(256, 30001, (64, 192))
        sgn = rng.choice([-1, 1], (64, 256))
        sgn[:, 0:64] = -1
        sgn[:, 64:128:2] = -1; sgn[:, 65:128:2] = 1
        sgn[:, 128:192:2] = 1; sgn[:, 129:192:2] = -1
        c = np.ascontiguousarray((mag * sgn).astype(np.int32))
        assert (c[:, :64] <= 0).all() and (c[:, :64] < 0).sum() > 1000 and np.abs(c[:, :64]).max() < 256
        assert (c[:, 64:128:2] <= 0).all() and (c[:, 65:128:2] >= 0).all() and (c[:, 64:128:2] < 0).any() and (c[:, 65:128:2] > 0).any()
        assert (c[:, 128:192:2] >= 0).all() and (c[:, 129:192:2] <= 0).all() and (c[:, 129:192:2] < 0).any()
        assert all(np.abs(c[:, 64 * k:64 * k + 64]).max() >= 256 for k in (1, 2, 3))
        c.setflags(write=False)
        _made["signs"] = c
    return _made["signs"]


def min16_case():
    """128 x 64, one wave: -32768 as a left coefficient of codeblock 0 and as a right one of codeblock 1, among small ones."""
    if "min16" not in _made:
        rng = np.random.default_rng(42)
        c = (rng.integers(-3, 4, (64, 128)) * (rng.random((64, 128)) < 0.3)).astype(np.int32)
        c[9, 20] = -32768
        c[40, 64 + 33] = -32768
        c[41, 64 + 32] = 32767
        c = np.ascontiguousarray(c)
        c.setflags(write=False)
        _made["min16"] = c
    return _made["min16"]


_refs = {}


def oracle_ref(key, coef, wl, lut):
    if key not in _refs:
        _refs[key] = orc.bpc_encode(coef, wl, lut)
    return _refs[key]


def msb_words(staging, sizes):
    """A coded codeblock's MSB: word 0 of its staging (the stream's short 9 + 2 cb)."""
    return [int(staging[cb * 4096]) for cb in range(sizes.size)]


def emu_encode16(coef, wl, lut):
    assert np.abs(coef).max() <= 32768 and coef.max() <= 32767
    E.set_c16(True)
    try:
        return E.bpc_encode(np.ascontiguousarray(coef.astype(np.int16)), wl, lut)
    finally:
        E.set_c16(False)


# ---- emulated ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lossy", [False, True])
def test_emulated_photographic_int16_equals_oracle(lossy):
    AW, AH, wl = PHOTO
    coef = photo_coeffs(lossy)
    lut = orc.lut_for(lossy, wl)
    st_ref, sz_ref = oracle_ref(("photo", lossy), coef, wl, lut)
    msbs = msb_words(st_ref, sz_ref)
    if lossy:
        assert E.coef16_ok(True, wl, QS97, 255, AW, AH)
        assert any(8 <= m <= 15 for m in msbs), "a codeblock for the second pass"
    assert any(m < 8 for m in msbs)
    st, sz, flag = emu_encode16(coef, wl, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)


def test_emulated_sign_cases_equal_oracle():
    coef = sign_cases()
    lut = orc.lut_for(False, 1)
    st_ref, sz_ref = oracle_ref("signs", coef, 1, lut)
    msbs = msb_words(st_ref, sz_ref)
    assert msbs[0] < 8 and all(m >= 8 for m in msbs[1:])
    st, sz, flag = emu_encode16(coef, 1, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)


def test_emulated_minus_32768_as_the_32_bit_form_gives_it():
    """Magnitude 32768, bit 15: the stream and the range flag of the 32-bit array's coder (modes 0 of the same kernel), and
    the oracle's stream."""
    coef = min16_case()
    lut = orc.lut_for(False, 1)
    st32, sz32, flag32 = E.bpc_encode(coef, 1, lut)
    st_ref, sz_ref = oracle_ref("min16", coef, 1, lut)
    assert msb_words(st_ref, sz_ref) == [15, 15]
    assert np.array_equal(sz32, sz_ref) and np.array_equal(st32, st_ref)
    st, sz, flag = emu_encode16(coef, 1, lut)
    assert flag == flag32 == 0
    assert np.array_equal(sz, sz32)
    assert np.array_equal(st, st32)


# ---- GPU --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return t


@pytest.fixture(scope="module")
def pa():
    import picsong_amd
    picsong_amd.load()
    return picsong_amd


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("lossy", [False, True])
def test_gpu_frame_paths_equal_oracle(pa, torch, lossy):
    """256 x 256, wl 3, 5/3 and 9/7 (the step of the emulated case: codeblocks with MSB >= 8): picsong_encode_frame and a
    three-frame picsong_encode_frames call, whose coder reads the int16 array."""
    AW, AH, wl = PHOTO
    qs = QS97 if lossy else 1.0
    lut = orc.lut_for(lossy, wl)
    imgs = [orc.gen_frame(AW, AH, f) for f in (9, 10, 11)]
    c = pa.Codec(AW, AH, wl=wl, lossy=lossy, qs=qs,
                 lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless"))
    ref = orc.encode_frame(imgs[0], wl, lossy, qs, lut)
    n_cb = (AW // 64) * (AH // 64)
    if lossy:
        assert any(8 <= int(m) <= 15 for m in ref[9:9 + 2 * n_cb:2])
    got = c.encode_frame(_dev(torch, imgs[0]), 0).cpu().numpy().view(np.uint16)
    assert c.range_flag() == 0
    assert got.size == ref.size and np.array_equal(got, ref)
    batch = c.encode_frames(_dev(torch, np.stack([i.reshape(-1) for i in imgs])), 0)
    for f, img in enumerate(imgs):
        ref = orc.encode_frame(img, wl, lossy, qs, lut, f, 0)
        g = batch[f].cpu().numpy().view(np.uint16)
        assert g.size == ref.size and np.array_equal(g, ref), f
    c.close()
