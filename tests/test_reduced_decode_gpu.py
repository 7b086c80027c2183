"""-m gpu: the reduced-resolution decode (picsong_decode_frame_reduced, _frames_reduced, _rgb_frame_reduced) against the
oracle's level-shifted LL_r, byte-identity with the full-size calls at r = 0, the output bound, and the codeblocks a
reduced call never reads."""
import os

import numpy as np
import pytest

import reduced_ref as rr

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


def _lut(oracle, lossy, wl, k, comp=0):
    return oracle.lut_for_component(lossy, wl, comp, k=k)


def _codec(pa, oracle, W, H, wl, lossy, qs, k=0.0, rgb=False):
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), k=k, rgb=rgb)


def _encode(torch, oracle, c, W, H, seed):
    frame = torch.from_numpy(oracle.pad_frame(oracle.gen_frame(W, H, seed))).cuda()
    return c.encode_frame(frame).clone()


@pytest.mark.parametrize("W,H,wl,lossy,qs,k", [
    (700, 500, 5, False, 1.0, 0.0), (1000, 300, 5, False, 1.0, 0.0),
    (700, 500, 6, True, 0.5, 0.0), (1000, 300, 6, True, 0.3, 0.0),
    (700, 500, 5, False, 1.0, 0.5), (1000, 300, 6, True, 0.5, 1.5), (700, 500, 6, True, 0.3, 0.5),
    (3840, 2160, 5, False, 1.0, 0.0), (3840, 2160, 6, True, 0.3, 0.0),       # odd ncx_r at r = 2 (15 columns)
    (7680, 4320, 5, False, 1.0, 0.0), (7680, 4320, 6, True, 0.5, 0.0),
])
def test_reduced_matches_oracle_ll(oracle, pa, torch, W, H, wl, lossy, qs, k):
    c = _codec(pa, oracle, W, H, wl, lossy, qs, k)
    s = _encode(torch, oracle, c, W, H, 5)
    sh = s.cpu().numpy().view(np.uint16)
    lut = _lut(oracle, lossy, wl, k)
    full = c.decode_frame(s).clone()
    for r in range(wl):
        got = c.decode_frame_reduced(s, r)
        assert tuple(got.shape) == (c.ah >> r, c.aw >> r)
        want = rr.reduced_pixels(sh, c.aw, c.ah, wl, lossy, qs, lut, r, k=k)
        assert np.array_equal(got.cpu().numpy(), want), f"r = {r}"
        rw, rh, paw, pah, ncb = c.reduced_dims(r)
        assert (rw, rh) == rr.visible(W, H, r) and (paw, pah) == (c.aw >> r, c.ah >> r)
        assert ncb == -(-paw // 64) * -(-pah // 64)
    assert torch.equal(c.decode_frame_reduced(s, 0), full)
    c.close()


@pytest.mark.parametrize("lossy,qs,k", [(False, 1.0, 0.0), (True, 0.5, 0.0), (False, 1.0, 0.5)])
def test_r0_is_the_full_decode_and_batches_equal_single_calls(oracle, pa, torch, lossy, qs, k):
    W, H, wl = 1000, 300, 5
    c = _codec(pa, oracle, W, H, wl, lossy, qs, k)
    ss = [_encode(torch, oracle, c, W, H, 20 + f) for f in range(5)]
    S = c.max_stream_shorts() + 40                               # strides larger than the minimum
    sb = torch.zeros((5, S), dtype=torch.int16, device="cuda")
    for f, s in enumerate(ss):
        sb[f, :s.numel()] = s
    full = [c.decode_frame(s).clone() for s in ss]
    assert torch.equal(c.decode_frames_reduced(sb, 0), c.decode_frames(sb))
    for r in range(wl):
        single = [c.decode_frame_reduced(s, r).clone() for s in ss]
        if r == 0:
            assert all(torch.equal(a, b) for a, b in zip(single, full))
        for n in (1, 3, 5):
            out = torch.full((n, (c.ah >> r) + 3, c.aw >> r), 0xA5, dtype=torch.uint8, device="cuda")
            c.decode_frames_reduced(sb[:n], r, out)
            for f in range(n):
                assert torch.equal(out[f, :c.ah >> r], single[f]), (r, n, f)
                assert bool((out[f, c.ah >> r:] == 0xA5).all())
    c.close()


@pytest.mark.parametrize("lossy,qs,k", [(False, 1.0, 0.0), (True, 0.5, 0.0), (True, 0.3, 0.0), (False, 1.0, 0.5)])
@pytest.mark.parametrize("nofuse", [False, True])
def test_rgb_reduced_matches_oracle(oracle, pa, torch, monkeypatch, lossy, qs, k, nofuse):
    if nofuse:
        monkeypatch.setenv("PICSONG_RGB_NOFUSE", "1")          # (read at every call)
    W, H, wl = 700, 500, 5
    planes = [oracle.pad_frame(oracle.gen_frame(W, H, 70 + i)) for i in range(3)]
    c = _codec(pa, oracle, W, H, wl, lossy, qs, k, rgb=True)
    got = [g.clone() for g in c.encode_rgb_frame(*[torch.from_numpy(p).cuda() for p in planes])]
    streams = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for i in range(3):
        streams[i, :got[i].numel()] = got[i]
    shs = [g.cpu().numpy().view(np.uint16) for g in got]
    luts = [_lut(oracle, lossy, wl, k, i) for i in range(3)]
    full = c.decode_rgb_frame(streams)
    for r in range(wl):
        back = c.decode_rgb_frame_reduced(streams, r)
        want = rr.reduced_rgb(shs, c.aw, c.ah, wl, lossy, qs, luts, r, k=k)
        for i in range(3):
            assert np.array_equal(back[i].cpu().numpy(), want[i]), (r, i)
            if r == 0:
                assert torch.equal(back[i], full[i])
    c.close()


def test_output_bound_and_odd_offset(oracle, pa, torch):
    W, H, wl = 700, 500, 5
    for lossy, qs in ((False, 1.0), (True, 0.5)):
        c = _codec(pa, oracle, W, H, wl, lossy, qs)
        s = _encode(torch, oracle, c, W, H, 9)
        for r in range(wl):
            n = (c.aw >> r) * (c.ah >> r)
            ref = c.decode_frame_reduced(s, r).view(-1).clone()
            for off in (0, 1, 3):
                buf = torch.full((n + 4096 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                view = buf[off:]
                assert c.L.picsong_decode_frame_reduced(c.h, c._p(s), r, c._p(view), c._stream()) == 0
                torch.cuda.synchronize()
                assert torch.equal(view[:n], ref), (lossy, r, off)
                assert bool((buf[:off] == 0xA5).all()) and bool((view[n:] == 0xA5).all()), (lossy, r, off)
        c.close()


@pytest.mark.parametrize("k", [0.0, 0.5])
def test_codeblocks_outside_the_rectangle_are_not_read(oracle, pa, torch, k):
    W, H, wl, r = 1000, 300, 5, 1
    c = _codec(pa, oracle, W, H, wl, False, 1.0, k)
    s = _encode(torch, oracle, c, W, H, 11)
    clean = c.decode_frame_reduced(s, r).clone()
    c.range_flag()
    ncx = c.aw // 64
    ncx_r, ncy_r = -(-(c.aw >> r) // 64), -(-(c.ah >> r) // 64)
    cb = (ncy_r - 1) * ncx + ncx_r                                # right of the rectangle
    bad = s.clone()
    bad[9 + 2 * cb] = 20                                          # MSB 20, length untouched
    c.decode_frame(bad)
    assert c.range_flag() == 1
    got = c.decode_frame_reduced(bad, r)
    assert c.range_flag() == 0
    assert torch.equal(got, clean)
    sb = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for f in range(3):
        sb[f, :bad.numel()] = bad
    out = c.decode_frames_reduced(sb, r)
    assert c.range_flag() == 0 and all(torch.equal(out[f], clean) for f in range(3))
    c.close()


def test_refusals(oracle, pa, torch):
    W, H, wl = 700, 500, 5
    c = _codec(pa, oracle, W, H, wl, False, 1.0)
    s = _encode(torch, oracle, c, W, H, 1)
    sb = torch.zeros((2, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    out = torch.empty(c.P * 2, dtype=torch.uint8, device="cuda")
    L = c.L
    for r in (-1, wl):
        assert L.picsong_decode_frame_reduced(c.h, c._p(s), r, c._p(out), c._stream()) == ERR_ARG
        assert b"reduce" in L.picsong_last_error()
        assert L.picsong_decode_frames_reduced(c.h, 2, c._p(sb), sb.stride(0), r, c._p(out), c.P, c._stream()) == ERR_ARG
        with pytest.raises(pa.PicsongError):
            c.reduced_dims(r)
    assert L.picsong_decode_frame_reduced(c.h, None, 1, c._p(out), c._stream()) == ERR_ARG
    # frame stride below the reduced image's bytes
    n1 = (c.aw >> 1) * (c.ah >> 1)
    assert L.picsong_decode_frames_reduced(c.h, 2, c._p(sb), sb.stride(0), 1, c._p(out), n1 - 1, c._stream()) == ERR_ARG
    assert L.picsong_decode_frames_reduced(c.h, 2, c._p(sb), 16, 1, c._p(out), n1, c._stream()) == ERR_ARG
    c.close()
    g = pa.Codec(W, H, wl=wl, lut_folder=os.path.join(oracle.LUT_CP3_DIR, "n1_lossless"), cp=3)
    assert g.L.picsong_decode_frame_reduced(g.h, g._p(s), 1, g._p(out), g._stream()) == ERR_ARG
    assert g.L.picsong_decode_frame_reduced(g.h, g._p(s), 0, g._p(out), g._stream()) == ERR_ARG
    g.close()
    rc = _codec(pa, oracle, W, H, wl, False, 1.0, rgb=True)
    s3 = torch.zeros((3, rc.max_stream_shorts()), dtype=torch.int16, device="cuda")
    o3 = [torch.empty(rc.P, dtype=torch.uint8, device="cuda") for _ in range(3)]
    assert rc.L.picsong_decode_rgb_frame_reduced(rc.h, rc._p(s3), s3.stride(0), wl, *[rc._p(o) for o in o3],
                                                 rc._stream()) == ERR_ARG
    rc.close()
