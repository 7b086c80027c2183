"""-m gpu: the rate calls (picsong_encode_frame_rate and its mirrors) against the reference procedure (rate_ref.bisect)
over the CPU oracle's own codestream sizes: the chosen quantiser, the streams byte for byte, their decode -- never
against the code under test."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as orc
import rate_ref as rr

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_RATE = -1, -7
SENTINEL = 0x5A5A


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


def _lutdir(lossy=True):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _ref(W, H, wl, target, j_min=0, j_max=0, k=0.0, frames=1):
    """The reference result, computed once a case: (Result, images, lut)."""
    imgs = [orc.gen_frame(W, H, f) for f in range(frames)]
    lut = orc.lut_for_k(True, wl) if k > 0 else orc.lut_for(True, wl)
    return rr.bisect(rr.frames_size_fn(imgs, wl, lut, k=k), target, j_min, j_max), imgs, lut


def _assert_interior(res, target, j_min=0, j_max=0):
    """The reference's own preconditions: a result strictly inside the range, the next grid value too large."""
    g = rr.grid(j_min, j_max)
    assert res.j is not None and g[0] < res.j < g[-1]
    assert res.size <= target < res.next_size


def _rate_call(pa, torch, c, frame, target, j_min=0, j_max=0, iter_=0):
    """picsong_encode_frame_rate into a buffer with sentinel shorts behind picsong_max_stream_shorts; returns
    (rc, j, total, stream buffer)."""
    n = c.max_stream_shorts()
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    j, t = C.c_int(77), C.c_int(-5)
    rc = c.L.picsong_encode_frame_rate(c.h, c._p(frame), iter_, target, j_min, j_max, c._p(buf), c._stream(), C.byref(j),
                                       C.byref(t))
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "shorts behind picsong_max_stream_shorts were written"
    return rc, j.value, t.value, buf


def _check_grey(pa, torch, W, H, wl, target, j_min=0, j_max=0, k=0.0):
    res, (img,), lut = _ref(W, H, wl, target, j_min, j_max, k)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir(), k=k)
    rc, j, total, buf = _rate_call(pa, torch, c, _dev(torch, orc.pad_frame(img)), target, j_min, j_max)
    assert rc == 0, c.L.picsong_last_error()
    assert j == res.j
    want = orc.encode_frame(img, wl, True, rr.q(j), lut, k=k)
    assert total == want.size == res.size and total <= target
    assert np.array_equal(_u16(buf[:total]), want)
    assert c.last_total() == total                      # ... and where picsong_encode_frame leaves its length
    # the decode on a context made from the stream's own header
    hp = pa.header_unpack(want[:9])
    assert np.float32(hp.qs) == np.float32(rr.q(j)) and (hp.wl, hp.lossy, hp.height, hp.width) == (wl, 1, H, W)
    # (picsong_ctx_create keeps the launcher's -qs range (0, 1]: a gain above it, the top of the grid, through set_qs)
    d = pa.Codec(hp.width, hp.height, wl=hp.wl, lossy=True, qs=min(hp.qs, 1.0), lut_folder=_lutdir(), k=hp.k)
    if hp.qs > 1.0:
        d.set_qs(hp.qs)
    got = d.decode_frame(buf[:c.max_stream_shorts()]).cpu().numpy()[:H, :W]
    assert np.array_equal(got, orc.decode_frame(want, W, H, wl, True, rr.q(j), lut, k=k))
    d.close()
    c.close()
    return res


@pytest.mark.parametrize("W,H,wl,target,want_j", [(200, 136, 3, 8000, 2829), (320, 192, 5, 6000, 1407), (700, 500, 5, 60000, 3098)])
def test_interior_results(pa, torch, W, H, wl, target, want_j):
    res, _, _ = _ref(W, H, wl, target)
    _assert_interior(res, target)
    assert res.j == want_j and len(res.probes) == 14
    _check_grey(pa, torch, W, H, wl, target)


def test_top_of_the_grid(pa, torch):
    res, _, _ = _ref(200, 136, 3, 20000)
    assert res.j == rr.grid()[-1] == 16382 and res.next_j is None and res.size == 16949 <= 20000
    _check_grey(pa, torch, 200, 136, 3, 20000)


def test_lowest_sizes(pa, torch):
    """34 shorts: the stream of an all-zero frame (9 + 2 * 12 + 1) fits from j = 9 down; 33: nothing does."""
    res, (img,), _ = _ref(200, 136, 3, 34)
    assert res.j == 9 and res.size == 34 and res.next_size == 323
    _check_grey(pa, torch, 200, 136, 3, 34)
    none, _, _ = _ref(200, 136, 3, 33)
    assert none.j is None and none.first_size == 34 > 33        # really below size(G'[0])
    c = pa.Codec(200, 136, wl=3, lossy=True, qs=1.0, lut_folder=_lutdir())
    rc, j, total, _ = _rate_call(pa, torch, c, _dev(torch, orc.pad_frame(img)), 33)
    assert rc == ERR_RATE and j == 0
    with pytest.raises(pa.RateError):
        c.encode_frame_rate(_dev(torch, orc.pad_frame(img)), 33)
    c.close()


def test_sub_range(pa, torch):
    W, H, wl, target, lo, hi = 700, 500, 6, 45000, 1000, 3000
    res, _, _ = _ref(W, H, wl, target, lo, hi)
    _assert_interior(res, target, lo, hi)
    assert res.first_size <= target
    _check_grey(pa, torch, W, H, wl, target, lo, hi)
    # nothing of the sub-range fits while lower quantisers outside it would
    low = res.first_size - 1
    none, (img,), _ = _ref(W, H, wl, low, lo, hi)
    assert none.j is None and none.first_size > low
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    rc, j, _, _ = _rate_call(pa, torch, c, _dev(torch, orc.pad_frame(img)), low, lo, hi)
    assert rc == ERR_RATE and j == 0
    c.close()


def test_complexity_scalable_context(pa, torch):
    W, H, wl, target, k = 320, 192, 5, 6000, 0.5
    res, _, _ = _ref(W, H, wl, target, k=k)
    _assert_interior(res, target)
    _check_grey(pa, torch, W, H, wl, target, k=k)


def test_batched_frames(pa, torch):
    W, H, wl, n, target = 320, 192, 5, 3, 18000
    res, imgs, lut = _ref(W, H, wl, target, frames=n)
    _assert_interior(res, target)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    frames = _dev(torch, np.stack([orc.pad_frame(im).ravel() for im in imgs]))
    j, streams = c.encode_frames_rate(frames, target)
    assert j == res.j
    want = [orc.encode_frame(imgs[f], wl, True, rr.q(j), lut, iter_=f) for f in range(n)]
    assert sum(w.size for w in want) == res.size <= target
    for f in range(n):
        assert np.array_equal(_u16(streams[f]), want[f]), f
        assert bool((want[f][:9] == 0xFFFF).all()) == (f != 0)      # the header on frame 0 only
    assert c.last_totals(n) == [w.size for w in want]
    # first_iter > 0: no frame carries the header, the same result
    j2, s2 = c.encode_frames_rate(frames, target, first_iter=5)
    assert j2 == j and all(np.array_equal(_u16(s2[f])[9:], want[f][9:]) and (_u16(s2[f])[:9] == 0xFFFF).all() for f in range(n))
    c.close()


def test_rgb_frame(pa, torch):
    W, H, wl, target = 200, 136, 3, 20000
    planes = [orc.gen_frame(W, H, 60 + c) for c in range(3)]
    comps = rr.rgb_components(*planes)
    luts = [orc.lut_for_component(True, wl, c) for c in range(3)]
    res = rr.bisect(rr.rgb_size_fn(comps, wl, luts), target)
    _assert_interior(res, target)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir(), rgb=True)
    d = [_dev(torch, orc.pad_frame(p)) for p in planes]
    j, streams = c.encode_rgb_frame_rate(*d, target, header_mask=1)
    assert j == res.j
    hdr = orc.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=8, lossy=1, qs_1e4=j,
                          components=3, is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=0)
    want = rr.rgb_streams(comps, wl, j, luts, hdr)
    assert sum(w.size for w in want) == res.size <= target
    for k in range(3):
        assert np.array_equal(_u16(streams[k]), want[k]), k
    # a 4-byte aligned view of the planes takes the separate colour transform: the same streams
    big = torch.zeros(3 * c.P + 64, dtype=torch.uint8, device="cuda")
    un = [big[4 + k * c.P:4 + (k + 1) * c.P] for k in range(3)]
    for k in range(3):
        un[k].copy_(d[k].view(-1))
    j2, s2 = c.encode_rgb_frame_rate(*un, target, header_mask=1)
    assert j2 == j and all(np.array_equal(_u16(s2[k]), want[k]) for k in range(3))
    c.close()


def test_set_qs_and_the_contexts_own_qs(pa, torch):
    W, H, wl, target = 200, 136, 3, 8000
    res, (img,), lut = _ref(W, H, wl, target)
    frame = _dev(torch, orc.pad_frame(img))
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=0.5, lut_folder=_lutdir())
    before = c.encode_frame(frame).clone()
    assert np.array_equal(_u16(before), orc.encode_frame(img, wl, True, 0.5, lut))
    j, _ = c.encode_frame_rate(frame, target)
    assert j == res.j
    assert torch.equal(c.encode_frame(frame), before)           # a rate call leaves the context's qs alone
    c.set_qs(pa.rate_qs(j))
    fresh = pa.Codec(W, H, wl=wl, lossy=True, qs=pa.rate_qs(j), lut_folder=_lutdir())
    got = c.encode_frame(frame)
    assert torch.equal(got, fresh.encode_frame(frame))
    assert np.array_equal(_u16(got), orc.encode_frame(img, wl, True, rr.q(j), lut))
    # ... and the decode side re-derived too
    full = torch.zeros(c.max_stream_shorts(), dtype=torch.int16, device="cuda")
    full[:got.numel()] = got
    assert torch.equal(c.decode_frame(full), fresh.decode_frame(full))
    assert c.L.picsong_ctx_set_qs(c.h, C.c_float(0.0)) == ERR_ARG and c.L.picsong_ctx_set_qs(c.h, C.c_float(-1.0)) == ERR_ARG
    assert c.L.picsong_ctx_set_qs(c.h, C.c_float(1.64)) == ERR_ARG and c.L.picsong_ctx_set_qs(None, C.c_float(0.5)) == ERR_ARG
    assert torch.equal(c.encode_frame(frame), got)              # a refused value changes nothing
    # a gain above 1 (the grid's upper part): the plain call equals the oracle there too
    c.set_qs(pa.rate_qs(16382))
    assert np.array_equal(_u16(c.encode_frame(frame)), orc.encode_frame(img, wl, True, rr.q(16382), lut))
    fresh.close()
    c.close()


def test_refusals_launch_nothing(pa, torch):
    W, H, wl = 200, 136, 3
    img = orc.pad_frame(orc.gen_frame(W, H))
    frame = _dev(torch, img)
    n_max = None

    def refused(c, call):
        """`call(stream buffer, j, totals)` -> rc: PICSONG_ERR_ARG, the outputs and the range flag untouched."""
        n = c.max_stream_shorts()
        buf = torch.full((3, n), SENTINEL, dtype=torch.int16, device="cuda")
        j, t = C.c_int(77), (C.c_int * 16)(*([-5] * 16))
        assert call(buf, j, t) == ERR_ARG
        torch.cuda.synchronize()
        assert j.value == 77 and list(t) == [-5] * 16 and bool((buf == SENTINEL).all())
        assert c.range_flag() == 0

    def grey(c, target=8000, j_min=0, j_max=0, fr=frame):
        return lambda buf, j, t: c.L.picsong_encode_frame_rate(c.h, c._p(fr) if fr is not None else None, 0, target, j_min, j_max,
                                                               c._p(buf), c._stream(), C.byref(j), t)

    def batch(c, n=2, stride=None, fr=None):
        fr2 = torch.stack([frame.view(-1)] * 2) if fr is None else fr
        return lambda buf, j, t: c.L.picsong_encode_frames_rate(c.h, n, c._p(fr2), c.P if stride is None else stride, 0, 16000, 0, 0,
                                                                c._p(buf), buf.stride(0), c._stream(), C.byref(j), t)

    def rgb(c):
        return lambda buf, j, t: c.L.picsong_encode_rgb_frame_rate(c.h, c._p(frame), c._p(frame), c._p(frame), 1, 20000, 0, 0,
                                                                   c._p(buf), buf.stride(0), c._stream(), C.byref(j), t)

    lossless = pa.Codec(W, H, wl=wl, lossy=False, lut_folder=_lutdir(False))
    refused(lossless, grey(lossless))
    refused(lossless, batch(lossless))
    lossless.close()
    cp3 = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, cp=3)
    refused(cp3, grey(cp3))
    cp3.close()
    col = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir(), rgb=True)
    refused(col, grey(col))
    refused(col, batch(col))
    col.close()
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    refused(c, rgb(c))
    refused(c, grey(c, target=0))
    for lo, hi in ((0, 5), (5, 0), (3, 2), (-1, 4), (1, 16384), (7, 7)):       # (7, 7): a range without a grid entry
        refused(c, grey(c, j_min=lo, j_max=hi))
    refused(c, grey(c, fr=None))
    refused(c, lambda buf, j, t: c.L.picsong_encode_frame_rate(c.h, c._p(frame), 0, 8000, 0, 0, c._p(buf), c._stream(), None, t))
    refused(c, lambda buf, j, t: c.L.picsong_encode_frame_rate(c.h, c._p(frame), 0, 8000, 0, 0, c._p(buf), c._stream(), C.byref(j), None))
    refused(c, batch(c, n=0))
    refused(c, batch(c, n=17))
    refused(c, batch(c, stride=c.P - 16))
    big = torch.zeros(2 * c.P + 64, dtype=torch.uint8, device="cuda")
    refused(c, batch(c, fr=big[1:]))                                            # frames not 16-byte aligned
    refused(c, lambda buf, j, t: c.L.picsong_encode_frames_rate(c.h, 2, c._p(torch.stack([frame.view(-1)] * 2)), c.P, 0, 16000, 0, 0,
                                                                c._p(buf), c.max_stream_shorts() - 1, c._stream(), C.byref(j), t))
    # the context still works, and an unaligned single frame is accepted as picsong_encode_frame accepts it
    res, _, _ = _ref(W, H, wl, 8000)
    un = big[1:1 + c.P]
    un.copy_(frame.view(-1))
    assert c.encode_frame_rate(un, 8000)[0] == res.j
    c.close()
    nolut = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0)
    refused(nolut, grey(nolut))
    nolut.close()
