"""The k = 0 encoder codes a codeblock's first bit-plane (step 0 of its wave: plane `msb` of each half's own codeblock) in
a body of its own (csrc/bpc_kernels.hpp, PICSONG_ENC_FIRST_PLANE): nothing is significant before that plane, so the lanes
of a significance site are one wave-constant mask, a left coefficient's context is the count of its three neighbours
above, a right one's at most five, context 8 cannot occur and the refinement pass is empty.

Every input is one at which that body can go wrong -- halves of a wave with different first planes, an invalid or an
all-zero half, blocks whose first plane is their only one, a first plane in which every coefficient becomes significant,
photographic frames (5/3 and 9/7 coefficients, 32-bit, float and 16-bit), and the wl = 6 table's zero-probability groups,
which send a codeblock to the raw fallback from its first plane on -- and every one is compared whole with the oracle's
output.  What step 0 codes is counted from the coefficients beside each input (first_plane_sites), so no case passes
without its step-0 sign sites, the dense case not without a right-column symbol of context 5 and a left-column symbol of
context 3, the first case not without two different first planes in one wave.

Without a GPU the encoder runs on the CPU wave emulator; with one (-m gpu) the same coefficients go through the stage
API, the same inputs as pixels through picsong_encode_frame, and three of them through one picsong_encode_frames call."""
import os

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc


# ---- what step 0 codes ------------------------------------------------------------------------------------------

def first_plane_sites(coef):
    """Per codeblock (None for an all-zero one): its msb, the number of step-0 sign sites (coefficients with bit msb
    set), and the sets of significance contexts its left (even) and right (odd) columns code at step 0.  Nothing is
    significant before the plane, so a neighbour counts when it becomes significant in it and is visited earlier: the
    three above for every coefficient, and for a right coefficient the two beside it (the lanes' left coefficients come
    first in a row)."""
    mag = np.abs(np.trunc(np.asarray(coef, np.float64))).astype(np.int64)
    AH, AW = mag.shape
    out = []
    for cb in range((AW // 64) * (AH // 64)):
        cby, cbx = divmod(cb, AW // 64)
        m = mag[cby * 64:cby * 64 + 64, cbx * 64:cbx * 64 + 64]
        if m.max() == 0:
            out.append(None)
            continue
        msb = min(int(m.max()).bit_length() - 1, 15)
        p = np.zeros((66, 66), np.int64)
        p[1:65, 1:65] = (m >> msb) & 1
        above = p[0:64, 0:64] + p[0:64, 1:65] + p[0:64, 2:66]
        beside = p[1:65, 0:64] + p[1:65, 2:66]
        out.append({"msb": msb, "signs": int(p.sum()), "left": set(above[:, 0::2].ravel().tolist()),
                    "right": set((above + beside)[:, 1::2].ravel().tolist())})
    return out


# ---- inputs: coefficient arrays (wl 1 unless they say otherwise) ------------------------------------------------

def _two_msb():
    """128 x 64, one wave: its two codeblocks' first planes are different bit-planes (the left one scaled by 8)."""
    c = np.random.default_rng(21).integers(-3, 4, (64, 128)).astype(np.int32)
    c[:, :64] *= 8
    return c


def _three_cb():
    """192 x 64: the second wave's upper half is no codeblock."""
    return np.random.default_rng(22).integers(-40, 41, (64, 192)).astype(np.int32) * \
        (np.random.default_rng(23).random((64, 192)) < 0.4)


def _zero_half():
    """256 x 64, two waves: a zero codeblock as the lower half of the first and as the upper half of the second."""
    c = np.random.default_rng(24).integers(-20, 21, (64, 256)).astype(np.int32)
    c[:, 0:64] = 0
    c[:, 192:256] = 0
    return c


def _ones():
    """256 x 64, magnitudes 0 and 1 only -- the first plane is the whole block: mixed, a single coefficient, every
    coefficient, sparse non-negative."""
    rng = np.random.default_rng(25)
    c = np.zeros((64, 256), np.int32)
    c[:, 0:64] = rng.integers(-1, 2, (64, 64))
    c[37, 64 + 22] = -1
    c[:, 128:192] = rng.choice([-1, 1], (64, 64))
    c[:, 192:256] = rng.random((64, 64)) < 0.1
    return c


def _dense():
    """128 x 64: every magnitude in [2^k, 2^(k+1)), k = 3 | 2, random signs: every coefficient becomes significant in the
    first plane and has a sign site, rows 31 / 32 and the edge lanes included."""
    rng = np.random.default_rng(26)
    c = np.empty((64, 128), np.int32)
    c[:, :64] = rng.integers(8, 16, (64, 64))
    c[:, 64:] = rng.integers(4, 8, (64, 64))
    return c * rng.choice([-1, 1], (64, 128))


SYNTH = {"two_msb": _two_msb, "three_cb": _three_cb, "zero_half": _zero_half, "ones": _ones, "dense": _dense}
PHOTO = (256, 256, 3)                                        # AW, AH, wl
QS = 0.5
_made = {}


def synth(name):
    if name not in _made:
        c = np.ascontiguousarray(SYNTH[name]().astype(np.int32))
        c.setflags(write=False)
        _made[name] = c
    return _made[name]


def photo_coeffs(lossy, frame=5):
    key = ("photo", lossy, frame)
    if key not in _made:
        AW, AH, wl = PHOTO
        x = orc.level_shift_fwd(orc.gen_frame(AW, AH, frame), lossy)
        c = np.ascontiguousarray(orc.dwt_forward(x, wl, QS if lossy else 1.0)[:AW * AH].reshape(AH, AW))
        c.setflags(write=False)
        _made[key] = c
    return _made[key]


def check_sites(name, coef):
    """The input reaches what it is there for."""
    s = first_plane_sites(coef)
    coded = [x for x in s if x is not None]
    assert coded and all(x["signs"] > 0 for x in coded), "step-0 sign sites"
    if name == "photo_lossy":
        # (a 5/3 frame's first planes are sparse: no context above 3; the 9/7 frame's LL block is what reaches bit n2)
        assert any(max(x["right"]) >= 4 for x in coded)
    if name == "two_msb":
        assert len(s) == 2 and s[0]["msb"] != s[1]["msb"]
    if name == "three_cb":
        assert len(s) == 3 and None not in s
    if name == "zero_half":
        assert [x is None for x in s] == [True, False, False, True]
    if name == "ones":
        assert all(x["msb"] == 0 for x in s) and s[1]["signs"] == 1 and s[2]["signs"] == 4096
    if name == "dense":
        assert s[0]["msb"] != s[1]["msb"]
        for x in s:
            assert x["signs"] == 4096 and 5 in x["right"] and 3 in x["left"]
            assert max(x["right"]) == 5 and max(x["left"]) == 3


_refs = {}


def oracle_ref(key, coef, wl, lut):
    if key not in _refs:
        _refs[key] = orc.bpc_encode(coef, wl, lut)
    return _refs[key]


# ---- emulated ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SYNTH))
def test_emulated_synthetic_equals_oracle(name):
    coef = synth(name)
    check_sites(name, coef)
    lut = orc.lut_for(False, 1)
    st_ref, sz_ref = oracle_ref(name, coef, 1, lut)
    st, sz, flag = E.bpc_encode(coef, 1, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)


@pytest.mark.parametrize("form", ["int32", "int16", "float"])
def test_emulated_photographic_equals_oracle(form):
    """256 x 256, wl 3: the 5/3 coefficients as 32-bit and as the frame paths' 16-bit array, the 9/7 ones as floats."""
    AW, AH, wl = PHOTO
    lossy = form == "float"
    coef = photo_coeffs(lossy)
    check_sites("photo_lossy" if lossy else "photo", coef)
    lut = orc.lut_for(lossy, wl)
    st_ref, sz_ref = oracle_ref(("photo", lossy), coef, wl, lut)
    if form == "int16":
        assert np.abs(coef).max() < 32768
        E.set_c16(True)
        try:
            st, sz, flag = E.bpc_encode(np.ascontiguousarray(coef.astype(np.int16)), wl, lut)
        finally:
            E.set_c16(False)
    else:
        st, sz, flag = E.bpc_encode(coef, wl, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)


HOLES = (2048, 2048, 6)                                      # test_gpu_parity.py::test_wl6_lut_holes_behaviour


def holes_coeffs():
    if "holes" not in _made:
        W, H, wl = HOLES
        x = orc.level_shift_fwd(orc.gen_frame(W, H, 0), True)
        _made["holes"] = np.ascontiguousarray(orc.dwt_forward(x, wl, QS)[:W * H].reshape(H, W))
    return _made["holes"]


def test_emulated_wl6_zero_probability_groups():
    """9/7, wl 6, 2048 x 2048: codeblock 0 holds LL and level 5, three of whose groups the wl = 6 table never wrote
    (probability 0: every 0 coded there ends a codeword).  The block ends as raw words, and its slots run out from the
    first plane on.  The first wave (codeblocks 0 and 1) on the emulator against the oracle."""
    W, H, wl = HOLES
    coef = holes_coeffs()
    lut = orc.lut_for(True, wl)
    st_ref, sz_ref = oracle_ref("holes", coef, wl, lut)
    assert sz_ref[0] == 4096 and sz_ref[1] < 4096
    s = first_plane_sites(coef[:64, :128])
    assert s[0]["signs"] > 0 and s[1]["signs"] > 0
    st, sz, flag = E.bpc_encode_range(coef, wl, lut, 0, 2)
    assert flag == 0
    assert np.array_equal(sz[:2], sz_ref[:2])
    assert np.array_equal(st[:2 * 4096], st_ref[:2 * 4096])


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
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared inputs are read-only)


def _lutdir(lossy):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def pixels_of(coef, wl):
    """The frame whose 5/3 coefficients are `coef` (the integer transform is reversible; the inputs are small enough for
    8-bit samples), and the coefficients that frame really has."""
    AH, AW = coef.shape
    inv, extra = orc.dwt_inverse(coef, wl, False)
    img = np.clip(orc.level_shift_inv(inv[extra:]).reshape(AH, AW), 0, 255).astype(np.uint8)
    back = orc.dwt_forward(orc.level_shift_fwd(img, False), wl)[:AW * AH].reshape(AH, AW)
    return img, back


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SYNTH))
def test_gpu_synthetic_equals_oracle(pa, torch, name):
    """The stage API on the 32-bit coefficients, and picsong_encode_frame on the frame that has them (16-bit array)."""
    coef = synth(name)
    AH, AW = coef.shape
    lut = orc.lut_for(False, 1)
    st_ref, sz_ref = oracle_ref(name, coef, 1, lut)
    img, back = pixels_of(coef, 1)
    assert np.array_equal(back, coef)
    check_sites(name, back)
    c = pa.Codec(AW, AH, wl=1, lut_folder=_lutdir(False))
    assert (c.aw, c.ah) == (AW, AH)
    st, sz = c.bpc_encode(_dev(torch, coef.reshape(-1)))
    assert c.range_flag() == 0
    assert np.array_equal(sz.cpu().numpy(), sz_ref)
    assert np.array_equal(st.cpu().numpy(), st_ref)
    ref = orc.encode_frame(img, 1, False, 1.0, lut)
    got = c.encode_frame(_dev(torch, img), 0).cpu().numpy().view(np.uint16)
    assert c.range_flag() == 0
    c.close()
    assert got.size == ref.size and np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("lossy", [False, True])
def test_gpu_photographic_equals_oracle(pa, torch, lossy):
    """256 x 256, wl 3, 5/3 and 9/7: the stage API (32-bit / float coefficients), the frame path (16-bit) and a
    three-frame batched call."""
    AW, AH, wl = PHOTO
    qs = QS if lossy else 1.0
    lut = orc.lut_for(lossy, wl)
    coef = photo_coeffs(lossy)
    st_ref, sz_ref = oracle_ref(("photo", lossy), coef, wl, lut)
    c = pa.Codec(AW, AH, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy))
    assert (c.aw, c.ah) == (AW, AH)
    st, sz = c.bpc_encode(_dev(torch, coef.reshape(-1)))
    assert np.array_equal(sz.cpu().numpy(), sz_ref)
    assert np.array_equal(st.cpu().numpy(), st_ref)
    imgs = [orc.gen_frame(AW, AH, f) for f in (5, 6, 7)]
    got = c.encode_frame(_dev(torch, imgs[0]), 0).cpu().numpy().view(np.uint16)
    ref = orc.encode_frame(imgs[0], wl, lossy, qs, lut)
    assert got.size == ref.size and np.array_equal(got, ref)
    batch = c.encode_frames(_dev(torch, np.stack([i.reshape(-1) for i in imgs])), 0)
    for f, img in enumerate(imgs):
        ref = orc.encode_frame(img, wl, lossy, qs, lut, f, 0)
        g = batch[f].cpu().numpy().view(np.uint16)
        assert g.size == ref.size and np.array_equal(g, ref), f
    c.close()


@pytest.mark.gpu
def test_gpu_wl6_zero_probability_groups(pa, torch):
    """The coefficients of the emulated case, all codeblocks, through the stage API."""
    W, H, wl = HOLES
    coef = holes_coeffs()
    lut = orc.lut_for(True, wl)
    st_ref, sz_ref = oracle_ref("holes", coef, wl, lut)
    assert sz_ref[0] == 4096
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=QS, lut_folder=_lutdir(True))
    st, sz = c.bpc_encode(_dev(torch, coef.reshape(-1)))
    c.close()
    assert np.array_equal(sz.cpu().numpy(), sz_ref)
    assert np.array_equal(st.cpu().numpy(), st_ref)
