"""-m gpu: the per-level transform kernels' 8-, 16- and 32-row band instantiations as hipcc builds them for gfx950,
through the C ABI, bit for bit against the CPU oracle.  launch_plan.hpp takes bands taller than 4 rows only from 1 Mi
samples a level on, so outside the full-size 4K / 8K / 16K tests nothing ran them; here PICSONG_DWT_BANDS, the per-level
override the plans read at every call, puts them on small frames whose levels are ragged against the band, on the
per-column kernels, on restricted level-0 launches and on every frame-path form.  tests/test_dwt_bands.py is the same
matrix on the CPU wave emulator.

Which kernel a launch takes cannot be read back through the ABI; the emulator's library includes the same launch_plan.hpp,
so every case first asserts through it (host code only) that its environment plans the bands it means to run."""
import os

import numpy as np
import pytest

import emu_lib as E

pytestmark = pytest.mark.gpu

# (W, H, wl) -> padded (AW, AH): 320 x 192 (level 2: 24 row pairs, ragged at 16- and 32-row bands), 704 x 320 (four strips
# across; level 2: 40 pairs), 1000 x 300 padded to 1024 x 320 (wl 4: 20 pairs on level 3)
GEOMS = [(320, 192, 3), (704, 320, 3), (1000, 300, 4)]
BAND_LISTS = {"8": "8,8,8,8", "16": "16,16,16,16", "32": "32,32,32,32", "mixed": "32,16,8,4"}
TRANSFORMS = {"53": (False, 1.0), "97q05": (True, 0.5), "97q03": (True, 0.3)}      # qs = 0.5: the one_div forms
SWITCHES = ("PICSONG_DWT_BANDS", "PICSONG_DWT_NOVEC", "PICSONG_DWT_NOFUSE01", "PICSONG_DWT_FUSE01", "PICSONG_DWT_EXACTDIV",
            "PICSONG_DWT_NOFUSE_INV", "PICSONG_DWT_FUSE_INV97", "PICSONG_DWT_EXACT_REPLAY", "PICSONG_C16", "PICSONG_DEC_C16",
            "PICSONG_RGB_NOFUSE")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return t


@pytest.fixture(scope="module")
def pa():
    import picsong_amd
    picsong_amd.load()          # raises if the extension is missing
    return picsong_amd


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _lutdir(oracle, lossy):
    return os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the cached references are read-only)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def use_bands(monkeypatch, bands, AW, AH, wl, lossy, novec=False):
    """Set the override and prove, through the plans themselves, that every level of this geometry takes the band meant
    for it (and the kernel family meant)."""
    monkeypatch.setenv("PICSONG_DWT_BANDS", BAND_LISTS[bands])
    if novec:
        monkeypatch.setenv("PICSONG_DWT_NOVEC", "1")
    want = [int(v) for v in BAND_LISTS[bands].split(",")][:wl]
    for fast in (False, True):
        fwd, inv = E.dwt_plan_bands(AW, AH, wl, lossy, fast)
        assert [b for b, _ in fwd] == want and [b for b, _ in inv] == want, (bands, AW, AH, wl, fast)
        assert all(v != novec for _, v in fwd + inv), "every level of these geometries is on the vector kernels unless told otherwise"


_refs = {}


def stage_reference(oracle, W, H, wl, tf):
    """The oracle's transform of the padded frame and its synthesis of the coded integers, computed once."""
    key = ("stage", W, H, wl, tf)
    if key not in _refs:
        lossy, qs = TRANSFORMS[tf]
        img = oracle.pad_frame(oracle.gen_frame(W, H, 1))
        AH, AW = img.shape
        x = oracle.level_shift_fwd(img, lossy)
        fwd = oracle.dwt_forward(x, wl, qs)[:AW * AH].copy()
        coef = np.trunc(fwd).astype(np.int32).reshape(AH, AW)
        inv, ex = oracle.dwt_inverse(coef, wl, lossy, qs)
        _refs[key] = (img, x, fwd, coef, inv[ex:].copy())
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def frame_reference(oracle, W, H, wl, tf, seed):
    """The oracle's codestream of a frame and its decode of it, computed once."""
    key = ("frame", W, H, wl, tf, seed)
    if key not in _refs:
        lossy, qs = TRANSFORMS[tf]
        img = oracle.gen_frame(W, H, seed)
        lut = oracle.lut_for(lossy, wl)
        stream = oracle.encode_frame(img, wl, lossy, qs, lut, 0, 0)
        pix = oracle.decode_frame(stream, W, H, wl, lossy, qs, lut)
        _refs[key] = (img, oracle.pad_frame(img), stream, pix)
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def _codec(oracle, pa, W, H, wl, tf, **kw):
    lossy, qs = TRANSFORMS[tf]
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), **kw)


# ---- stage calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", sorted(TRANSFORMS))
@pytest.mark.parametrize("path", ["vec", "novec"])
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("W,H,wl", GEOMS)
def test_stage_calls_equal_oracle(oracle, pa, torch, monkeypatch, W, H, wl, bands, path, tf):
    """Codec.dwt_forward from u8 (the fused head, and one launch a level) and from shifted samples, Codec.dwt_inverse --
    9/7 with the context's reciprocal divisions and with the dividing kernels -- on the vector and the per-column
    kernels."""
    lossy, qs = TRANSFORMS[tf]
    img, x, fwd, coef, inv = stage_reference(oracle, W, H, wl, tf)
    AH, AW = img.shape
    P = AW * AH
    use_bands(monkeypatch, bands, AW, AH, wl, lossy, novec=path == "novec")
    c = _codec(oracle, pa, W, H, wl, tf)
    assert (c.aw, c.ah) == (AW, AH)
    d_img, d_x, d_coef = _dev(torch, img), _dev(torch, x), _dev(torch, coef)
    for nofuse in (None, "1"):
        if nofuse:
            monkeypatch.setenv("PICSONG_DWT_NOFUSE01", nofuse)
        got = c.dwt_forward(d_img).cpu().numpy()
        assert np.array_equal(_bits(got[:P]), _bits(fwd)), f"forward from u8, nofuse01={nofuse}"
    got = c.dwt_forward(d_x).cpu().numpy()
    assert np.array_equal(_bits(got[:P]), _bits(fwd)), "forward from shifted samples"
    got = c.dwt_inverse(d_coef).cpu().numpy()
    assert np.array_equal(_bits(got[c.extra:]), _bits(inv)), "synthesis"
    c.close()
    if lossy:
        monkeypatch.setenv("PICSONG_DWT_EXACTDIV", "1")         # read when the context is made
        c = _codec(oracle, pa, W, H, wl, tf)
        got = c.dwt_inverse(d_coef).cpu().numpy()
        assert np.array_equal(_bits(got[c.extra:]), _bits(inv)), "synthesis, dividing kernels"
        c.close()


# ---- frame calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c16", ["unset", "0"])
@pytest.mark.parametrize("tf", sorted(TRANSFORMS))
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("W,H,wl", GEOMS)
def test_frame_calls_equal_oracle(oracle, pa, torch, monkeypatch, W, H, wl, bands, tf, c16):
    """encode_frame / decode_frame with levels 0 and 1 through the per-level kernels (PICSONG_DWT_NOFUSE01=1,
    PICSONG_DWT_NOFUSE_INV=1), coefficients as int16 (the default) and as 32-bit arrays (PICSONG_C16=0, PICSONG_DEC_C16=0):
    the oracle's stream, the oracle's pixels."""
    lossy, qs = TRANSFORMS[tf]
    img, pad, stream, pix = frame_reference(oracle, W, H, wl, tf, 2)
    AH, AW = pad.shape
    use_bands(monkeypatch, bands, AW, AH, wl, lossy)
    monkeypatch.setenv("PICSONG_DWT_NOFUSE01", "1")
    monkeypatch.setenv("PICSONG_DWT_NOFUSE_INV", "1")
    if c16 == "0":
        monkeypatch.setenv("PICSONG_C16", "0")
        monkeypatch.setenv("PICSONG_DEC_C16", "0")
    c = _codec(oracle, pa, W, H, wl, tf)
    got = _u16(c.encode_frame(_dev(torch, pad), 0))
    assert c.range_flag() == 0
    assert got.size == stream.size and np.array_equal(got, stream)
    dec = c.decode_frame(_dev(torch, stream.view(np.int16))).cpu().numpy()[:H, :W]
    assert np.array_equal(dec, pix)
    if not lossy:
        assert np.array_equal(dec, img)
    c.close()


@pytest.mark.parametrize("tf", sorted(TRANSFORMS))
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("W,H,wl", GEOMS)
def test_three_frames_a_call_and_the_reduced_decode(oracle, pa, torch, monkeypatch, W, H, wl, bands, tf):
    """encode_frames / decode_frames with n = 3 (grid.z = frame) and decode_frame_reduced with r = 1 (the synthesis plan cut
    after level 1: plan_dwt_inverse_reduced), one launch a level."""
    import reduced_ref
    lossy, qs = TRANSFORMS[tf]
    refs = [frame_reference(oracle, W, H, wl, tf, seed) for seed in (2, 3, 4)]
    AH, AW = refs[0][1].shape
    use_bands(monkeypatch, bands, AW, AH, wl, lossy)
    monkeypatch.setenv("PICSONG_DWT_NOFUSE01", "1")
    monkeypatch.setenv("PICSONG_DWT_NOFUSE_INV", "1")
    c = _codec(oracle, pa, W, H, wl, tf)
    frames = _dev(torch, np.stack([r[1].reshape(-1) for r in refs]))
    got = c.encode_frames(frames, 0)
    assert c.range_flag() == 0
    streams = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for i, r in enumerate(refs):
        g = _u16(got[i])
        assert g.size == r[2].size and np.array_equal(g[9:], r[2][9:]), f"frame {i}"      # (the header: on frame 0 alone)
        streams[i, :r[2].size] = _dev(torch, r[2].view(np.int16))
    assert np.array_equal(_u16(got[0]), refs[0][2])
    out = c.decode_frames(streams).cpu().numpy()
    for i, r in enumerate(refs):
        assert np.array_equal(out[i, :H, :W], r[3]), f"frame {i}"
    small = c.decode_frame_reduced(streams[0, :refs[0][2].size].clone(), 1).cpu().numpy()
    want = reduced_ref.reduced_pixels(refs[0][2], AW, AH, wl, lossy, qs, oracle.lut_for(lossy, wl), 1)
    assert small.shape == want.shape and np.array_equal(small, want)
    c.close()


@pytest.mark.parametrize("tf", ["53", "97q05"])
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("W,H,wl", GEOMS[1:])
def test_unaligned_frame_pointer_takes_the_per_column_kernels(oracle, pa, torch, monkeypatch, W, H, wl, bands, tf):
    """A frame pointer off 16-byte alignment sends the call to the per-column kernels (VEC = false) with the 32-bit arrays,
    at whatever band height the levels have: the same codestream.  (The plan is asserted for an aligned pointer; what an
    unaligned one changes is vec alone -- dwt_vec_ok.)"""
    lossy, qs = TRANSFORMS[tf]
    img, pad, stream, pix = frame_reference(oracle, W, H, wl, tf, 2)
    AH, AW = pad.shape
    use_bands(monkeypatch, bands, AW, AH, wl, lossy)
    c = _codec(oracle, pa, W, H, wl, tf)
    for off in (1, 4, 8):
        buf = torch.zeros(pad.size + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + pad.size]
        view.copy_(_dev(torch, pad).view(-1))
        assert np.array_equal(_u16(c.encode_frame(view, 0)), stream), off
    c.close()


# ---- RGB ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", sorted(TRANSFORMS))
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("W,H,wl", [GEOMS[0], GEOMS[2]])
def test_rgb_frame_equals_oracle(oracle, pa, torch, monkeypatch, W, H, wl, bands, tf):
    """encode_rgb_frame / decode_rgb_frame: the per-level kernels over the three components (grid.z) and the fused tails
    (dwt_inv_rgb_kernel; dwt_inv97_rgb_kernel in both one_div forms) -- every component's stream is the oracle's, the planes
    are the oracle's decode of them through its inverse colour transform."""
    lossy, qs = TRANSFORMS[tf]
    planes = [oracle.pad_frame(oracle.gen_frame(W, H, 20 + k)) for k in range(3)]
    AH, AW = planes[0].shape
    use_bands(monkeypatch, bands, AW, AH, wl, lossy)
    monkeypatch.setenv("PICSONG_DWT_NOFUSE01", "1")
    c = _codec(oracle, pa, W, H, wl, tf, rgb=True)
    hdr = pa.header_pack(c.params)
    got = [g.clone() for g in c.encode_rgb_frame(*[_dev(torch, p) for p in planes], header_mask=1)]
    comps = oracle.rgb_forward(*planes, lossy)
    luts = [oracle.lut_for_component(lossy, wl, k) for k in range(3)]
    streams = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    back = []
    for k in range(3):
        ref = oracle.encode_plane(comps[k], wl, lossy, qs, luts[k], hdr if k == 0 else None)
        assert np.array_equal(_u16(got[k]), ref), f"component {k}"
        streams[k, :got[k].numel()] = got[k]
        back.append(oracle.decode_plane(ref, AW, AH, wl, lossy, qs, luts[k]))
    want = oracle.rgb_inverse(*back)
    dec = c.decode_rgb_frame(streams)
    for k in range(3):
        assert np.array_equal(dec[k].cpu().numpy().reshape(AH, AW), want[k]), f"plane {k}"
        if not lossy:
            assert np.array_equal(want[k], planes[k])
    c.close()


# ---- sharding: level 0 restricted to a slice of rows ----------------------------------------------------------------------
# the first slicing divides into 8-row bands and not into taller ones (its last slice into all); the second into none,
# 4-row bands included: 22, 45 and 29 row pairs
SLICINGS = {"40+88+64": ((0, 40), (40, 88), (128, 64)), "44+90+58": ((0, 44), (44, 90), (134, 58))}


@pytest.mark.parametrize("tf", ["53", "97q05"])
@pytest.mark.parametrize("path", ["vec", "novec"])
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("slicing", sorted(SLICINGS))
def test_restricted_level_0_slices_equal_the_whole_transform(oracle, pa, torch, monkeypatch, slicing, bands, path, tf):
    """dwt_forward_band over three slices of a 320 x 192 frame's rows, each from a buffer that holds nothing but the slice
    and its 4-row halo, then dwt_forward_tail: the oracle's coefficients."""
    W, H, wl = GEOMS[0]
    lossy, qs = TRANSFORMS[tf]
    img, x, fwd, coef, inv = stage_reference(oracle, W, H, wl, tf)
    AH, AW = img.shape
    use_bands(monkeypatch, bands, AW, AH, wl, lossy, novec=path == "novec")
    c = _codec(oracle, pa, W, H, wl, tf)
    out = c.new_coef_buffer()
    out.fill_(12345)
    for row0, rows in SLICINGS[slicing]:
        part = np.full((AH, AW), 0xA5, np.uint8)
        lo, hi = max(0, row0 - 4), min(AH, row0 + rows + 4)
        part[lo:hi] = img[lo:hi]
        c.dwt_forward_band(_dev(torch, part).view(-1), row0, rows, out)
    c.dwt_forward_tail(out)
    assert np.array_equal(_bits(out.cpu().numpy()[:AW * AH]), _bits(fwd))
    c.close()


# ---- the policy's own choice ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", ["53", "97q05"])
def test_2048_square_takes_8_row_bands_by_itself(oracle, pa, torch, tf):
    """No override: level 0 of 2048 x 2048 is 9 strips x 248 columns x 2048 rows = 4.6 Mi samples, where fwd_band_rows gives
    8 rows (and inv97_band_rows 16, with 8 on level 1) -- the stage calls and the frame calls against the oracle."""
    W, H, wl = 2048, 2048, 3
    lossy, qs = TRANSFORMS[tf]
    fwd_plan, inv_plan = E.dwt_plan_bands(W, H, wl, lossy, lossy)
    assert [b for b, _ in fwd_plan] == [8, 4, 4]
    assert [b for b, _ in inv_plan] == ([16, 8, 4] if lossy else [8, 4, 4])
    oracle.set_threads(oracle.usable_threads())
    try:
        img = oracle.gen_frame(W, H, 5)
        x = oracle.level_shift_fwd(img, lossy)
        fwd = oracle.dwt_forward(x, wl, qs)[:W * H]
        coef = np.trunc(fwd).astype(np.int32).reshape(H, W)
        inv, ex = oracle.dwt_inverse(coef, wl, lossy, qs)
        lut = oracle.lut_for(lossy, wl)
        stream = oracle.encode_frame(img, wl, lossy, qs, lut, 0, 0)
        pix = oracle.decode_frame(stream, W, H, wl, lossy, qs, lut)
    finally:
        oracle.set_threads(1)
    c = _codec(oracle, pa, W, H, wl, tf)
    assert (c.aw, c.ah) == (W, H)
    d_img = _dev(torch, img)
    assert np.array_equal(_bits(c.dwt_forward(_dev(torch, x)).cpu().numpy()[:W * H]), _bits(fwd))      # one launch a level
    assert np.array_equal(_bits(c.dwt_forward(d_img).cpu().numpy()[:W * H]), _bits(fwd))
    assert np.array_equal(_bits(c.dwt_inverse(_dev(torch, coef)).cpu().numpy()[c.extra:]), _bits(inv[ex:]))
    assert np.array_equal(_u16(c.encode_frame(d_img, 0)), stream)
    assert np.array_equal(c.decode_frame(_dev(torch, stream.view(np.int16))).cpu().numpy(), pix)
    c.close()
