"""The k = 0 two-pass encoder after its register diet (csrc/bpc_kernels.hpp, PICSONG_ENC_OCC8) on the GPU: small frames
through the frame calls, every codestream compared with the oracle's.  (tests/test_encoder_occ8.py runs the diet's edge
cases on the emulator.)"""
import os

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu
QS = 0.5


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


def _lutdir(lossy):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _stream(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("lossy", [False, True], ids=["53", "97"])
def test_photographic_frames_equal_oracle(pa, torch, lossy):
    """gen_frame(256, 256, f), f = 0, 1, wl 3: lossless with the round trip, and 9/7 at qs 0.5."""
    W, H, wl = 256, 256, 3
    qs = QS if lossy else 1.0
    lut = orc.lut_for(lossy, wl)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy))
    for f in (0, 1):
        img = orc.gen_frame(W, H, f)
        ref = orc.encode_frame(img, wl, lossy, qs, lut)
        got = c.encode_frame(_dev(torch, orc.pad_frame(img)), 0)
        g = _stream(got)
        assert g.size == ref.size and np.array_equal(g, ref), f
        if not lossy:
            assert np.array_equal(c.decode_frame(got).cpu().numpy()[:H, :W], img), f
    assert c.range_flag() == 0
    c.close()


def test_one_codeblock_frame_equals_oracle(pa, torch):
    """64 x 64: one codeblock, the upper half of its wave idle."""
    W, H, wl = 64, 64, 1
    lut = orc.lut_for(False, wl)
    img = orc.gen_frame(W, H, 2)
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False))
    assert (c.aw, c.ah, c.ncb) == (64, 64, 1)
    got = c.encode_frame(_dev(torch, orc.pad_frame(img)), 0)
    ref = orc.encode_frame(img, wl, False, 1.0, lut)
    g = _stream(got)
    assert g.size == ref.size and np.array_equal(g, ref)
    assert np.array_equal(c.decode_frame(got).cpu().numpy()[:H, :W], img)
    c.close()


def test_two_frame_batch_equals_oracle(pa, torch):
    W, H, wl = 256, 256, 3
    lut = orc.lut_for(False, wl)
    imgs = [orc.gen_frame(W, H, f) for f in (0, 1)]
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False))
    batch = c.encode_frames(_dev(torch, np.stack([orc.pad_frame(i).reshape(-1) for i in imgs])), 0)
    for f, img in enumerate(imgs):
        ref = orc.encode_frame(img, wl, False, 1.0, lut, f, 0)
        g = _stream(batch[f])
        assert g.size == ref.size and np.array_equal(g, ref), f
    c.close()


def test_rgb_frame_equals_oracle(pa, torch):
    """128 x 128 RGB: three components, each with its table, in one coder launch."""
    W, H, wl = 128, 128, 2
    planes = [orc.pad_frame(orc.gen_frame(W, H, 10 + k)) for k in range(3)]
    c = pa.Codec(W, H, wl=wl, rgb=True, lut_folder=_lutdir(False))
    got = [g.clone() for g in c.encode_rgb_frame(*[_dev(torch, p) for p in planes], header_mask=0)]
    comps = orc.rgb_forward(*planes, False)
    for k in range(3):
        ref = orc.encode_plane(comps[k], wl, False, 1.0, orc.lut_for_component(False, wl, k), None)
        g = _stream(got[k])
        assert g.size == ref.size and np.array_equal(g, ref), f"component {k}"
    c.close()
