"""-m gpu: the reduced-quality decode (Codec.set_decode_drop / picsong_ctx_set_decode_drop) against drop_ref -- the oracle's
full decode truncated in numpy by d(cb) = max(0, drop - level(cb)) with midpoint reconstruction: the decoder alone, whole
frames in both coefficient forms, the composition with n frames, reduce, windows, RGB and the image calls, the setting as
state, and what the setter refuses."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import drop_ref as dr

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                      # PICSONG_ERR_ARG


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


def _lutdir(oracle, lossy):
    return os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _codec(pa, oracle, W, H, wl, lossy, qs, k=0.0, rgb=False, cp=2):
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=None if cp == 3 else _lutdir(oracle, lossy), k=k, rgb=rgb, cp=cp)


def _encode(torch, oracle, c, W, H, seed):
    frame = torch.from_numpy(oracle.pad_frame(oracle.gen_frame(W, H, seed))).cuda()
    return c.encode_frame(frame).clone()


def _rows(torch, c, streams):
    sb = torch.zeros((len(streams), c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for f, s in enumerate(streams):
        sb[f, :s.numel()] = s
    return sb


def _u16(s):
    return s.cpu().numpy().view(np.uint16)


# ---- the decoder alone ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep(oracle):
    W, H, wl = 576, 320, 3
    lut = oracle.lut_for(False, wl)
    coef = oracle.deep_coeffs(W, H, 5, raw_cb=7)
    st, sz = oracle.bpc_encode(coef, wl, lut)
    assert sz[7] == 4096 and np.array_equal(oracle.bpc_decode(st, sz, W, H, wl, lut), coef)
    return W, H, wl, coef, st, sz


@pytest.mark.parametrize("drop", [1, 4, 9])
def test_bpc_decode_deep_coefficients(oracle, pa, torch, drop):
    """picsong_bpc_decode (the staging form) on MSBs 8, 12 and 15, a raw codeblock and, at drop 9, codeblocks with MSB < d."""
    W, H, wl, coef, st, sz = _deep(oracle)
    c = _codec(pa, oracle, W, H, wl, False, 1.0)
    c.set_decode_drop(drop)
    assert c.decode_drop() == drop
    staging = torch.from_numpy(np.ascontiguousarray(st, np.int32)).cuda()
    sizes = torch.from_numpy(np.ascontiguousarray(sz, np.int32)).cuda()
    got = c.bpc_decode(staging, sizes).cpu().numpy().reshape(H, W)
    want = dr.truncate(coef, sz, W, H, wl, drop)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(got[0:64, 448:512], coef[0:64, 448:512]), "the raw codeblock stays whole"
    assert c.range_flag() == 0
    c.close()


# ---- frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
@pytest.mark.parametrize("c16", [True, False])
def test_decode_frame_matches_the_truncated_oracle(oracle, pa, torch, monkeypatch, lossy, qs, c16):
    """704 x 512, wl 3: codeblocks straddle subbands (AW >> 1 = 352).  Both coefficient forms: the context's own choice, and
    the 32-bit form of a context created under PICSONG_DEC_C16=0."""
    if not c16:
        monkeypatch.setenv("PICSONG_DEC_C16", "0")
    W, H, wl = 704, 512, 3
    c = _codec(pa, oracle, W, H, wl, lossy, qs)
    s = _encode(torch, oracle, c, W, H, 0)
    lut = oracle.lut_for(lossy, wl)
    plain = c.decode_frame(s).clone()
    for drop in (1, 2, 4, 6):
        c.set_decode_drop(drop)
        got = c.decode_frame(s).cpu().numpy()
        want = dr.drop_pixels(_u16(s), W, H, wl, lossy, qs, lut, drop)
        assert np.array_equal(got, want), (drop, int((got != want).sum()))
        assert not np.array_equal(got, plain.cpu().numpy()), drop
    assert c.range_flag() == 0
    c.close()


def test_composition_on_grey_frames(oracle, pa, torch):
    """832 x 320, wl 4, drop 2: n = 3 frames a call equal three single calls (and drop_ref); reduce 1; a window that crosses
    codeblock borders."""
    W, H, wl, drop = 832, 320, 4, 2
    for lossy, qs in ((False, 1.0), (True, 0.5)):
        c = _codec(pa, oracle, W, H, wl, lossy, qs)
        lut = oracle.lut_for(lossy, wl)
        ss = [_encode(torch, oracle, c, W, H, 20 + f) for f in range(3)]
        sb = _rows(torch, c, ss)
        c.set_decode_drop(drop)
        single = [c.decode_frame(s).clone() for s in ss]
        batch = c.decode_frames(sb)
        for f in range(3):
            assert torch.equal(batch[f], single[f]), f
            assert np.array_equal(single[f].cpu().numpy(), dr.drop_pixels(_u16(ss[f]), W, H, wl, lossy, qs, lut, drop)), f
        got = c.decode_frame_reduced(ss[0], 1).cpu().numpy()
        assert np.array_equal(got, dr.drop_pixels(_u16(ss[0]), W, H, wl, lossy, qs, lut, drop, 1))
        for r, (x, y, w, h) in ((0, (50, 40, 150, 100)), (1, (25, 20, 75, 50))):
            got = c.decode_frame_window(ss[0], x, y, w, h, r).cpu().numpy()
            assert np.array_equal(got, dr.drop_window(_u16(ss[0]), W, H, wl, lossy, qs, lut, drop, r, x, y, w, h)), (r, x, y)
        c.close()


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_composition_on_rgb_frames(oracle, pa, torch, lossy, qs):
    """832 x 320, wl 4, drop 2 (the same for the three components): decode_rgb_frames n = 2, and decode_rgb_images_reduced
    into RGBA at r = 1."""
    W, H, wl, drop, n = 832, 320, 4, 2, 2
    c = _codec(pa, oracle, W, H, wl, lossy, qs, rgb=True)
    planes = [torch.from_numpy(np.stack([oracle.pad_frame(oracle.gen_frame(W, H, 60 + 3 * f + k)) for f in range(n)])).cuda() for k in range(3)]
    got = [g.clone() for g in c.encode_rgb_frames(*planes)]
    sb = _rows(torch, c, got)
    luts = [oracle.lut_for_component(lossy, wl, k) for k in range(3)]
    c.set_decode_drop(drop)
    outs = c.decode_rgb_frames(sb)
    want = [dr.drop_rgb([_u16(g) for g in got[3 * f:3 * f + 3]], W, H, wl, lossy, qs, luts, drop) for f in range(n)]
    for f in range(n):
        for k in range(3):
            assert np.array_equal(outs[k][f].cpu().numpy(), want[f][k]), (f, k)
    r = 1
    rw, rh, paw, pah, _ = c.reduced_dims(r)
    rgba = torch.full((n, rh, rw, 4), 0x5A, dtype=torch.uint8, device="cuda")
    c.decode_rgb_images_reduced(sb, r, c.image(rgba, pa.LAYOUT_RGBA32, pitch=rw * 4), frame_stride=rgba.stride(0))
    px = rgba.cpu().numpy()
    for f in range(n):
        red = dr.drop_rgb([_u16(g) for g in got[3 * f:3 * f + 3]], W, H, wl, lossy, qs, luts, drop, r)
        for k in range(3):
            assert np.array_equal(px[f, :, :, k], red[k][:rh, :rw]), (f, k)
        assert (px[f, :, :, 3] == 255).all()
    c.close()


# ---- the setting is state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_drop_zero_after_a_drop_is_the_fresh_contexts_decode(oracle, pa, torch, lossy, qs):
    W, H, wl = 704, 512, 3
    c, fresh = _codec(pa, oracle, W, H, wl, lossy, qs), _codec(pa, oracle, W, H, wl, lossy, qs)
    s = _encode(torch, oracle, c, W, H, 3)
    want = fresh.decode_frame(s).clone()
    assert c.decode_drop() == 0
    c.set_decode_drop(5)
    assert not torch.equal(c.decode_frame(s), want)
    c.set_decode_drop(0)
    assert c.decode_drop() == 0
    assert torch.equal(c.decode_frame(s), want)
    if not lossy:
        assert np.array_equal(want.cpu().numpy()[:H, :W], oracle.gen_frame(W, H, 3))
    c.close()
    fresh.close()


def test_refusals_keep_the_setting(oracle, pa, torch):
    W, H, wl = 704, 512, 3
    c = _codec(pa, oracle, W, H, wl, False, 1.0)
    s = _encode(torch, oracle, c, W, H, 4)
    c.set_decode_drop(2)
    want = c.decode_frame(s).clone()
    for bad in (-1, 16):
        assert c.L.picsong_ctx_set_decode_drop(c.h, bad) == ERR_ARG
        assert b"set_decode_drop" in c.L.picsong_last_error()
        with pytest.raises(pa.PicsongError):
            c.set_decode_drop(bad)
        assert c.decode_drop() == 2
        assert torch.equal(c.decode_frame(s), want)
    c.close()
    for kw in (dict(k=0.5), dict(cp=3)):
        c = _codec(pa, oracle, W, H, wl, False, 1.0, **kw)
        for d in (1, 0, 15):
            assert c.L.picsong_ctx_set_decode_drop(c.h, d) == ERR_ARG, (kw, d)
        d = C.c_int(-1)
        assert c.L.picsong_ctx_get_decode_drop(c.h, C.byref(d)) == 0 and d.value == 0
        c.close()
