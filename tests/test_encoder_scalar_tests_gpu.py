"""The k = 0 encoder's scalar forms of its wave-uniform tests on the GPU (csrc/bpc_kernels.hpp,
PICSONG_ENC_SIGN_TEST_SCALAR, PICSONG_ENC_SPP_ONM_CARRY, PICSONG_ENC_REF_SCALAR_COUNT, PICSONG_ENC_RESERVE_ONE_TEST; the
emulated cases and what the switches do: tests/test_encoder_scalar_tests.py): whole frames through picsong_amd.Codec with
the library as it is built, the codestream compared bit for bit with the oracle's, the lossless ones decoded back to the
frame.  What the emulator cannot show is here: the sign site's scalar compare and the refinement loops' scalar counter
exist in the compiled kernel alone, and a reservation entered with an empty mask is an exec region that no lane enters --
its store, its LDS atomic and its wait are skipped by the region's own branch."""
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


def _roundtrip(pa, torch, W, H, wl, lossy, frame):
    qs = QS if lossy else 1.0
    img = orc.gen_frame(W, H, frame)
    lut = orc.lut_for(lossy, wl)
    ref = orc.encode_frame(img, wl, lossy, qs, lut)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs,
                 lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless"))
    got = c.encode_frame(torch.from_numpy(orc.pad_frame(img)).cuda(), 0)
    assert c.range_flag() == 0
    g = got.cpu().numpy().view(np.uint16)
    assert g.size == ref.size and np.array_equal(g, ref)
    if not lossy:
        dec = c.decode_frame(got).cpu().numpy()[:H, :W]
        assert np.array_equal(dec, img)
    c.close()


@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("frame", [0, 1])
def test_gpu_frame_equals_oracle(pa, torch, frame, lossy):
    """gen_frame(256, 256, f), wl 3: 5/3 lossless (and its round trip) and 9/7 at qs 0.5."""
    _roundtrip(pa, torch, 256, 256, 3, lossy, frame)


def test_gpu_single_codeblock_equals_oracle(pa, torch):
    """64 x 64, wl 1: one wave whose upper half is no codeblock."""
    _roundtrip(pa, torch, 64, 64, 1, False, 0)


def test_gpu_single_wave_equals_oracle(pa, torch):
    """128 x 64, wl 1: one wave, two codeblocks in lock step."""
    _roundtrip(pa, torch, 128, 64, 1, False, 0)
