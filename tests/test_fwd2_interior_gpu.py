"""The geometries of test_fwd2_interior.py on the GPU: picsong_encode_frame (a lone frame: the fused 5/3 head's 8-pair
bands) and a three-frame picsong_encode_frames call (the band length of batched calls, PICSONG_DWT_F2_PAIRS_BATCH), both
with interior strips where the width has them, against the oracle's codestream."""
import os

import numpy as np
import pytest

import oracle_lib as orc
from test_fwd2_interior import FRAMES, HEIGHTS, WIDTHS

_refs = {}


def oracle_stream(W, H, wl, frame, iter_):
    key = (W, H, wl, frame, iter_)
    if key not in _refs:
        _refs[key] = orc.encode_frame(orc.gen_frame(W, H, frame), wl, False, 1.0, orc.lut_for(False, wl), iter_, 0)
    return _refs[key]


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


@pytest.mark.gpu
@pytest.mark.parametrize("wl", [2, 3])
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", sorted(WIDTHS))
def test_gpu_encode_frame_and_frames_equal_oracle(pa, torch, W, H, wl):
    imgs = [orc.gen_frame(W, H, f) for f in FRAMES]
    c = pa.Codec(W, H, wl=wl, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossless"))
    assert (c.aw, c.ah) == (W, H)
    ref = oracle_stream(W, H, wl, FRAMES[0], 0)
    got = c.encode_frame(torch.from_numpy(imgs[0]).cuda(), 0).cpu().numpy().view(np.uint16)
    assert c.range_flag() == 0
    assert got.size == ref.size and np.array_equal(got, ref)
    batch = c.encode_frames(torch.from_numpy(np.stack([i.reshape(-1) for i in imgs])).cuda(), 0)
    for z, f in enumerate(FRAMES):
        ref = oracle_stream(W, H, wl, f, z)
        g = batch[z].cpu().numpy().view(np.uint16)
        assert g.size == ref.size and np.array_equal(g, ref), f"frame {z}"
    c.close()
