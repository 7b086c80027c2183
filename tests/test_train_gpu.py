"""-m gpu: the training calls (picsong_train_*) against the reference model (train_ref.py) on the oracle's coefficients,
and what a trained table buys: smaller streams that equal the oracle's with the same table and still round-trip."""
import numpy as np
import pytest

import train_cases as tc
import train_ref as tr

pytestmark = pytest.mark.gpu
ERR_ARG = -1


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


def _frames(torch, oracle, W, H, seeds):
    return torch.from_numpy(np.stack([oracle.pad_frame(oracle.gen_frame(W, H, f)) for f in seeds])).cuda()


@pytest.mark.parametrize("name", tc.CASES)
def test_train_coeffs_equals_model(oracle, pa, torch, name):
    coef, wl = tc.case(name)
    AH, AW = coef.shape
    c = pa.Codec(AW, AH, wl=wl, lossy=coef.dtype == np.float32, qs=0.5)        # (no table set)
    info = c.train_begin()
    want, wflag = tc.model(name)
    assert info.n_ref + info.n_sig + info.n_sign == len(want)
    c.train_coeffs(torch.from_numpy(coef).cuda())
    assert np.array_equal(c.train_counts(0), want)
    assert c.range_flag() == wflag and c.range_flag() == 0
    assert not c.train_counts(1).any() and not c.train_counts(2).any()
    c.train_coeffs(torch.from_numpy(coef).cuda(), component=2)                 # accumulates, slot by slot
    c.train_coeffs(torch.from_numpy(coef).cuda(), component=2)
    assert np.array_equal(c.train_counts(2), 2 * want) and np.array_equal(c.train_counts(0), want)
    c.train_end()
    c.close()


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_train_frames(oracle, pa, torch, lossy, qs):
    W, H, wl = 256, 192, 3
    want = sum(tc.model_of_frame(W, H, wl, lossy, f, qs)[0] for f in range(3))
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs)
    c.train_begin()
    fr = _frames(torch, oracle, W, H, range(3))
    c.train_frames(fr.view(3, -1))
    got = c.train_counts(0)
    assert np.array_equal(got, want)                       # the model over the oracle's coefficients of the three frames
    c.train_reset()
    assert not c.train_counts(0).any()
    for f in range(3):                                     # three n = 1 calls
        c.train_frames(fr[f].view(1, -1))
    assert np.array_equal(c.train_counts(0), want)
    c.train_reset()
    # frames at an odd address (a view one byte into a larger buffer): the per-column kernels, the same counts
    buf = torch.zeros(3 * c.P + 64, dtype=torch.uint8, device="cuda")
    un = buf[1:1 + 3 * c.P].view(3, c.P)
    un.copy_(fr.view(3, -1))
    assert un.data_ptr() % 16 == 1
    c.train_frames(un)
    assert np.array_equal(c.train_counts(0), want)
    assert c.range_flag() == 0
    c.close()                                              # (without train_end: the context frees the counters)


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_train_rgb_frame(oracle, pa, torch, lossy, qs):
    W, H, wl = 128, 128, 2
    planes = [oracle.pad_frame(oracle.gen_frame(W, H, 40 + k)) for k in range(3)]
    comps = oracle.rgb_forward(*planes, lossy)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, rgb=True)
    c.train_begin()
    c.train_rgb_frame(*[torch.from_numpy(p).cuda() for p in planes])
    for k in range(3):
        AH, AW = planes[0].shape
        coef = oracle.dwt_forward(comps[k].reshape(AH, AW), wl, qs)[:AW * AH].reshape(AH, AW)
        want, _ = tr.counts(coef, wl, tc.GEO)
        assert np.array_equal(c.train_counts(k), want), k
    c.close()


def test_persistent_grid_takes_several_pairs_a_wave(oracle, pa, torch):
    """32 frames of 1024 x 1024 are 4096 codeblock pairs, more than the persistent grid has waves: a wave then takes
    several pairs, reusing its plane scratch and its LDS columns.  One launch equals the frames' single-frame calls."""
    W = H = 1024
    c = pa.Codec(W, H, wl=4)
    c.train_begin()
    four = _frames(torch, oracle, W, H, range(4)).view(4, -1)
    single = []
    for f in range(4):
        c.train_reset()
        c.train_frames(four[f:f + 1])
        single.append(c.train_counts(0))
    assert 32 * ((c.ncb + 1) // 2) > 768 * 4
    c.train_reset()
    c.train_frames(four.repeat(8, 1))
    assert np.array_equal(c.train_counts(0), 8 * sum(single))
    assert int(single[0].sum()) > W * H
    c.close()


def test_refusals(oracle, pa, torch):
    W, H, wl = 128, 128, 2
    import ctypes as C
    fr = _frames(torch, oracle, W, H, [0])
    p = C.c_void_p(fr.data_ptr())
    geo = pa.LutInfo(**pa.TRAIN_GEOMETRY)
    c = pa.Codec(W, H, wl=wl)
    L = c.L
    assert L.picsong_train_frames(c.h, 1, p, 0, None) == ERR_ARG and b"picsong_train_begin" in L.picsong_last_error()
    assert L.picsong_train_coeffs(c.h, 0, p, None) == ERR_ARG
    assert L.picsong_train_counts(c.h, 0, None, None, 0) == ERR_ARG
    assert L.picsong_train_reset(c.h) == ERR_ARG and L.picsong_train_end(c.h) == ERR_ARG
    for bad in (dict(n_bitplanes=0), dict(ctx_sig=0), dict(ctx_ref=0), dict(ctx_sign=-1), dict(n_subbands=0), dict(n_bitplanes=400)):
        assert L.picsong_train_begin(c.h, C.byref(pa.LutInfo(**dict(pa.TRAIN_GEOMETRY, **bad)))) == ERR_ARG, bad
    assert L.picsong_train_begin(c.h, None) == ERR_ARG
    c.train_begin()
    assert L.picsong_train_frames(c.h, 0, p, c.P, None) == ERR_ARG and L.picsong_train_frames(c.h, 65, p, c.P, None) == ERR_ARG
    assert L.picsong_train_frames(c.h, 2, p, c.P - 16, None) == ERR_ARG
    assert L.picsong_train_frames(c.h, 1, None, c.P, None) == ERR_ARG
    assert L.picsong_train_coeffs(c.h, 3, p, None) == ERR_ARG and L.picsong_train_coeffs(c.h, 0, None, None) == ERR_ARG
    assert L.picsong_train_rgb_frame(c.h, p, p, p, None) == ERR_ARG          # a grey context
    n = L.picsong_train_counts(c.h, 0, None, None, 0)
    assert n == sum(tr.sections(tc.GEO, wl))
    small = np.zeros((n - 1, 2), np.uint64)
    assert L.picsong_train_counts(c.h, 0, None, small.ctypes.data_as(C.c_void_p), n - 1) == ERR_ARG
    assert not c.train_counts(0).any()                      # nothing was launched
    c.close()
    for kw in (dict(cp=3), dict(k=0.5)):
        c = pa.Codec(W, H, wl=wl, **kw)
        assert c.L.picsong_train_begin(c.h, C.byref(geo)) == ERR_ARG, kw
        c.close()
    c = pa.Codec(W, H, wl=wl, rgb=True)
    c.train_begin()
    assert c.L.picsong_train_frames(c.h, 1, p, c.P, None) == ERR_ARG          # an RGB context
    assert c.L.picsong_train_rgb_frame(c.h, p, None, p, None) == ERR_ARG
    c.close()


# the streams of frames 0, 1, 2 in shorts: golden table -> table trained on frames 0 and 1 (the reference model and the
# oracle on the CPU; the rule is deterministic)
GAIN = {False: [(79048, 75425), (79074, 75459), (79160, 75521)], True: [(57548, 54756), (57510, 54725), (57645, 54778)]}


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_trained_table_gain(oracle, pa, torch, lossy, qs):
    W = H = 512
    wl = 3
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs)
    info = c.train_begin()
    fr = _frames(torch, oracle, W, H, range(3))
    c.train_frames(fr[:2].view(2, -1))                     # frame 2 is held out
    table = pa.lut_from_counts(info, c.train_counts(0))    # no prior
    c.train_end()
    assert table.min() >= 1 and table.max() <= 127
    c.set_lut(info, table)
    geo = dict(tc.GEO, n_ref=info.n_ref, n_sig=info.n_sig, n_sign=info.n_sign)
    trained, golden = oracle.CallerLut(table, geo), oracle.lut_for(lossy, wl)
    for f in range(3):
        img = oracle.gen_frame(W, H, f)
        got = c.encode_frame(fr[f]).clone()
        want = oracle.encode_frame(img, wl, lossy, qs, trained)
        assert np.array_equal(got.cpu().numpy().view(np.uint16), want), f      # the oracle's stream with the same table
        dec = c.decode_frame(got).cpu().numpy()[:H, :W]
        if lossy:
            assert np.array_equal(dec, oracle.decode_frame(want, W, H, wl, lossy, qs, trained))
            assert np.array_equal(dec, oracle.decode_frame(oracle.encode_frame(img, wl, lossy, qs, golden), W, H, wl, lossy, qs, golden))
        else:
            assert np.array_equal(dec, img)
        base = oracle.encode_frame(img, wl, lossy, qs, golden).size
        print(f"lossy {lossy} frame {f}: golden {base} -> trained {want.size} shorts ({want.size / base:.4f})")
        assert want.size <= 0.97 * base
        assert (base, want.size) == GAIN[lossy][f]
    c.close()
