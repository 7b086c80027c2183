"""-m gpu: picsong_frames_sse against numpy, and the quality calls (picsong_encode_frame_quality and its mirrors) against
the reference procedure (quality_ref.bisect) over the CPU oracle's decode of its own encode: the chosen quantiser, the
streams byte for byte, the distortion reported and the distortion of this library's own decode -- never against the
code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as orc
import quality_ref as qr
import rate_ref as rr

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_QUALITY = -1, -8
SENTINEL = 0x5A5A
GREY_CASES = [n for n, c in sorted(qr.CASES.items()) if c[3] == 1 and not c[4]]


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


def _np_sse(a, b, W, H):
    return qr.sse(a[:H, :W], b[:H, :W])


# ---- picsong_frames_sse ---------------------------------------------------------------------------------------------
def _sse_call(torch, c, a, a_stride, b, b_stride, n):
    """The raw call into a buffer with a sentinel behind d_sse[n]."""
    out = torch.full((n + 1,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    assert c.L.picsong_frames_sse(c.h, n, c._p(a), a_stride, c._p(b), b_stride, c._p(out), c._stream()) == 0, c.L.picsong_last_error()
    got = out.cpu().numpy()
    assert got[n] == 0x0123456789ABCDEF
    return [int(v) for v in got[:n]]


@pytest.mark.parametrize("W,H", [(200, 136), (700, 500), (201, 137)])
def test_frames_sse_against_numpy(pa, torch, W, H):
    c = pa.Codec(W, H, wl=3, lossy=False)                    # a lossless context: only the geometry is used
    AW, AH, P = c.aw, c.ah, c.P
    rng = np.random.default_rng(W + H)
    a = rng.integers(0, 256, (AH, AW), dtype=np.uint8)
    b = rng.integers(0, 256, (AH, AW), dtype=np.uint8)
    want = _np_sse(a, b, W, H)
    da, db = _dev(torch, a), _dev(torch, b)
    assert _sse_call(torch, c, da, 0, db, 0, 1) == [want]
    assert _sse_call(torch, c, da, 0, da, 0, 1) == [0]                          # equal images
    pad = a.copy()
    pad[:, W:] ^= 0xFF
    pad[H:, :] ^= 0xFF
    assert _sse_call(torch, c, da, 0, _dev(torch, pad), 0, 1) == [0]            # padding that differs does not count
    assert int(c.frames_sse(da.view(-1), db.view(-1))[0]) == want               # the binding
    # n = 3 with strides above P
    za, zb = P + 4096, P + 160
    fa = rng.integers(0, 256, 3 * za, dtype=np.uint8)
    fb = rng.integers(0, 256, 3 * zb, dtype=np.uint8)
    fb[zb:zb + P] = fa[za:za + P]
    wants = [_np_sse(fa[f * za:f * za + P].reshape(AH, AW), fb[f * zb:f * zb + P].reshape(AH, AW), W, H) for f in range(3)]
    assert wants[1] == 0 and wants[0] > 0
    assert _sse_call(torch, c, _dev(torch, fa), za, _dev(torch, fb), zb, 3) == wants
    # pointers offset by one byte: the per-byte form
    ua = torch.zeros(P + 16, dtype=torch.uint8, device="cuda")
    ub = torch.zeros(P + 16, dtype=torch.uint8, device="cuda")
    ua[1:1 + P].copy_(da.view(-1))
    ub[1:1 + P].copy_(db.view(-1))
    assert _sse_call(torch, c, ua[1:], 0, ub[1:], 0, 1) == [want]
    assert _sse_call(torch, c, ua[1:], 0, db, 0, 1) == [want]
    # refusals: nothing launched
    out = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    L = c.L
    assert L.picsong_frames_sse(c.h, 1, None, 0, c._p(db), 0, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_sse(c.h, 1, c._p(da), 0, None, 0, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_sse(c.h, 1, c._p(da), 0, c._p(db), 0, None, c._stream()) == ERR_ARG
    assert L.picsong_frames_sse(None, 1, c._p(da), 0, c._p(db), 0, c._p(out), c._stream()) == ERR_ARG
    for n in (0, -1, 65):
        assert L.picsong_frames_sse(c.h, n, c._p(da), P, c._p(db), P, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_sse(c.h, 2, c._p(_dev(torch, fa)), P - 1, c._p(_dev(torch, fb)), zb, c._p(out), c._stream()) == ERR_ARG
    assert L.picsong_frames_sse(c.h, 2, c._p(_dev(torch, fa)), za, c._p(_dev(torch, fb)), P - 1, c._p(out), c._stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    c.close()


def test_frames_sse_beyond_32_bits(pa, torch):
    c = pa.Codec(2048, 2048, wl=5, lossy=False)
    a = torch.zeros(c.P, dtype=torch.uint8, device="cuda")
    b = torch.full((c.P,), 255, dtype=torch.uint8, device="cuda")
    want = 65025 * (1 << 22)
    assert want > 1 << 32
    assert _sse_call(torch, c, a, 0, b, 0, 1) == [want]
    assert [int(v) for v in c.frames_sse(a, b)] == [want]                       # the same from run to run
    c.close()


def test_frames_sse_on_an_rgb_context(pa, torch):
    W, H = 200, 136
    c = pa.Codec(W, H, wl=3, lossy=True, qs=0.5, rgb=True)
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (3, c.ah, c.aw), dtype=np.uint8)
    b = rng.integers(0, 256, (3, c.ah, c.aw), dtype=np.uint8)
    got = c.frames_sse(_dev(torch, a).view(3, -1), _dev(torch, b).view(3, -1))
    assert [int(v) for v in got] == [_np_sse(a[k], b[k], W, H) for k in range(3)]
    c.close()


# ---- the quality calls ----------------------------------------------------------------------------------------------
def _quality_call(torch, c, frame, max_sse, j_min=0, j_max=0, iter_=0):
    """picsong_encode_frame_quality into a buffer with sentinel shorts behind picsong_max_stream_shorts; returns
    (rc, j, total, sse, stream buffer)."""
    n = c.max_stream_shorts()
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    j, t, e = C.c_int(77), C.c_int(-5), C.c_uint64(99)
    rc = c.L.picsong_encode_frame_quality(c.h, c._p(frame), iter_, max_sse, j_min, j_max, c._p(buf), c._stream(), C.byref(j),
                                          C.byref(t), C.byref(e))
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "shorts behind picsong_max_stream_shorts were written"
    return rc, j.value, t.value, e.value, buf


def _decoder(pa, W, H, wl, j, k=0.0, rgb=False):
    """A context at q(j) (picsong_ctx_create keeps (0, 1]: a gain above it through set_qs)."""
    d = pa.Codec(W, H, wl=wl, lossy=True, qs=min(rr.q(j), 1.0), lut_folder=_lutdir(), k=k, rgb=rgb)
    if rr.q(j) > 1.0:
        d.set_qs(rr.q(j))
    return d


def _check_grey(pa, torch, name, max_sse=None, j_min=None, j_max=None, k=0.0):
    W, H, wl = qr.CASES[name][:3]
    res = qr.case_result(name, max_sse, j_min, j_max)
    limit = qr.CASES[name][8] if max_sse is None else max_sse
    lo = qr.CASES[name][6] if j_min is None else j_min
    hi = qr.CASES[name][7] if j_max is None else j_max
    (img,), _ = qr.case_inputs(name)
    lut = orc.lut_for_k(True, wl) if k > 0 else orc.lut_for(True, wl)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir(), k=k)
    rc, j, total, e, buf = _quality_call(torch, c, _dev(torch, orc.pad_frame(img)), limit, lo, hi)
    assert rc == 0, c.L.picsong_last_error()
    assert j == res.j
    want = orc.encode_frame(img, wl, True, rr.q(j), lut, k=k)
    assert total == want.size and np.array_equal(_u16(buf[:total]), want)
    assert e == res.sse <= limit
    assert c.last_total() == total                      # ... and where picsong_encode_frame leaves its length
    assert c.range_flag() == 0
    d = _decoder(pa, W, H, wl, j, k)
    got = d.decode_frame(buf[:c.max_stream_shorts()]).cpu().numpy()
    assert _np_sse(got, orc.pad_frame(img), W, H) == e  # the distortion of this library's own decode
    d.close()
    c.close()
    return res


@pytest.mark.parametrize("name", GREY_CASES)
def test_table_cases_of_one_grey_frame(pa, torch, name):
    W, H, wl, frames, rgb, db, j_min, j_max, limit, j, per, prev_j, prev_sse = qr.CASES[name]
    res = _check_grey(pa, torch, name)
    assert (res.j, res.sse) == (j, per[0]) and res.prev_sse == prev_sse > limit


def test_edges_of_the_grid(pa, torch):
    name = "200x136-wl3-40dB"
    assert _check_grey(pa, torch, name, max_sse=10 ** 12).j == 1
    assert _check_grey(pa, torch, name, max_sse=339).j == 16374
    assert qr.case_result(name, max_sse=0).j is None
    (img,), _ = qr.case_inputs(name)
    c = pa.Codec(200, 136, wl=3, lossy=True, qs=1.0, lut_folder=_lutdir())
    frame = _dev(torch, orc.pad_frame(img))
    rc, j, _, _, _ = _quality_call(torch, c, frame, 0)             # max_sse = 0: a legal request that nothing meets
    assert rc == ERR_QUALITY and j == 0
    with pytest.raises(pa.QualityError):
        c.encode_frame_quality(frame, 0)
    assert c.encode_frame_quality(frame, 176868)[0] == 1865          # the context still works
    c.close()


def test_sub_range_pair(pa, torch):
    name = "700x500-wl6-40dB-sub"
    W, H, wl = qr.CASES[name][:3]
    assert qr.case_result(name, max_sse=778017).j is None
    (img,), _ = qr.case_inputs(name)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    rc, j, _, _, _ = _quality_call(torch, c, _dev(torch, orc.pad_frame(img)), 778017, 1000, 3000)
    assert rc == ERR_QUALITY and j == 0
    c.close()
    assert _check_grey(pa, torch, name, max_sse=778017, j_min=0, j_max=0).j == 3001


def test_complexity_scalable_context(pa, torch):
    """The distortion does not depend on -k: the same j, the stream the oracle's at that k."""
    name = "320x192-wl5-30dB"
    assert _check_grey(pa, torch, name, k=0.5).j == qr.CASES[name][9]


def test_batched_frames(pa, torch):
    name = "3x320x192-wl5-40dB"
    W, H, wl, n = qr.CASES[name][:4]
    limit, want_j, per = qr.CASES[name][8:11]
    res = qr.case_result(name)
    assert (res.j, res.sse) == (want_j, sum(per)) and res.sse <= limit < res.prev_sse
    imgs, lut = qr.case_inputs(name)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=0.5, lut_folder=_lutdir())
    frames = _dev(torch, np.stack([orc.pad_frame(im).ravel() for im in imgs]))
    j, streams, sse = c.encode_frames_quality(frames, limit)
    assert j == res.j and sse == per
    want = [orc.encode_frame(imgs[f], wl, True, rr.q(j), lut, iter_=f) for f in range(n)]
    for f in range(n):
        assert np.array_equal(_u16(streams[f]), want[f]), f
        assert bool((want[f][:9] == 0xFFFF).all()) == (f != 0)      # the header on frame 0 only
    assert c.last_totals(n) == [w.size for w in want]
    d = _decoder(pa, W, H, wl, j)
    for f in range(n):
        full = torch.zeros(c.max_stream_shorts(), dtype=torch.int16, device="cuda")
        full[:streams[f].numel()] = streams[f]
        assert _np_sse(d.decode_frame(full).cpu().numpy(), orc.pad_frame(imgs[f]), W, H) == per[f]
    d.close()
    # first_iter > 0: no frame carries the header, the same result
    j2, s2, sse2 = c.encode_frames_quality(frames, limit, first_iter=5)
    assert j2 == j and sse2 == per
    assert all(np.array_equal(_u16(s2[f])[9:], want[f][9:]) and (_u16(s2[f])[:9] == 0xFFFF).all() for f in range(n))
    # the context's own qs is unchanged
    assert np.array_equal(_u16(c.encode_frame(frames[0])), orc.encode_frame(imgs[0], wl, True, 0.5, lut))
    c.close()


def test_rgb_frame(pa, torch):
    name = "rgb-200x136-wl3-40dB"
    W, H, wl = qr.CASES[name][:3]
    limit, want_j, per = qr.CASES[name][8:11]
    res = qr.case_result(name)
    assert (res.j, res.sse) == (want_j, sum(per)) and res.sse <= limit < res.prev_sse
    planes, luts = qr.case_inputs(name)
    comps = rr.rgb_components(*planes)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir(), rgb=True)
    d = [_dev(torch, orc.pad_frame(p)) for p in planes]
    n = c.max_stream_shorts()
    buf = torch.full((3, n + 64), SENTINEL, dtype=torch.int16, device="cuda")
    j, t, e = C.c_int(), (C.c_int * 3)(), (C.c_uint64 * 3)()
    rc = c.L.picsong_encode_rgb_frame_quality(c.h, c._p(d[0]), c._p(d[1]), c._p(d[2]), 1, limit, 0, 0, c._p(buf), buf.stride(0),
                                              c._stream(), C.byref(j), t, e)
    torch.cuda.synchronize()
    assert rc == 0, c.L.picsong_last_error()
    assert bool((buf[:, n:] == SENTINEL).all())
    assert j.value == res.j and [int(v) for v in e] == per
    hdr = orc.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=8, lossy=1, qs_1e4=j.value,
                          components=3, is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=0)
    want = rr.rgb_streams(comps, wl, j.value, luts, hdr)
    for k in range(3):
        assert t[k] == want[k].size and np.array_equal(_u16(buf[k, :t[k]]), want[k]), k
    assert c.last_totals(3) == [w.size for w in want]
    dec = _decoder(pa, W, H, wl, j.value, rgb=True)
    out = dec.decode_rgb_frame(buf[:, :n].contiguous())
    assert [_np_sse(out[k].cpu().numpy(), orc.pad_frame(planes[k]), W, H) for k in range(3)] == per
    dec.close()
    # a 4-byte aligned view of the planes takes the separate colour transform: the same result
    big = torch.zeros(3 * c.P + 64, dtype=torch.uint8, device="cuda")
    un = [big[4 + k * c.P:4 + (k + 1) * c.P] for k in range(3)]
    for k in range(3):
        un[k].copy_(d[k].view(-1))
    j2, s2, sse2 = c.encode_rgb_frame_quality(*un, limit, header_mask=1)
    assert j2 == res.j and sse2 == per and all(np.array_equal(_u16(s2[k]), want[k]) for k in range(3))
    c.close()


def test_refusals_launch_nothing(pa, torch):
    W, H, wl = 200, 136, 3
    img = orc.pad_frame(orc.gen_frame(W, H))
    frame = _dev(torch, img)

    def refused(c, call):
        """`call(stream buffer, j, totals, sse)` -> rc: PICSONG_ERR_ARG, the outputs and the range flag untouched."""
        n = c.max_stream_shorts()
        buf = torch.full((3, n), SENTINEL, dtype=torch.int16, device="cuda")
        j, t, e = C.c_int(77), (C.c_int * 16)(*([-5] * 16)), (C.c_uint64 * 16)(*([99] * 16))
        assert call(buf, j, t, e) == ERR_ARG
        torch.cuda.synchronize()
        assert j.value == 77 and list(t) == [-5] * 16 and list(e) == [99] * 16 and bool((buf == SENTINEL).all())
        assert c.range_flag() == 0

    def grey(c, j_min=0, j_max=0, fr=frame):
        return lambda buf, j, t, e: c.L.picsong_encode_frame_quality(c.h, c._p(fr) if fr is not None else None, 0, 176868, j_min,
                                                                     j_max, c._p(buf), c._stream(), C.byref(j), t, e)

    def batch(c, n=2, stride=None, fr=None, sstride=None):
        fr2 = torch.stack([frame.view(-1)] * 2) if fr is None else fr
        return lambda buf, j, t, e: c.L.picsong_encode_frames_quality(c.h, n, c._p(fr2), c.P if stride is None else stride, 0, 400000,
                                                                      0, 0, c._p(buf), buf.stride(0) if sstride is None else sstride,
                                                                      c._stream(), C.byref(j), t, e)

    def rgb(c, planes=(frame, frame, frame)):
        return lambda buf, j, t, e: c.L.picsong_encode_rgb_frame_quality(c.h, c._p(planes[0]), c._p(planes[1]), c._p(planes[2]), 1,
                                                                         530604, 0, 0, c._p(buf), buf.stride(0), c._stream(),
                                                                         C.byref(j), t, e)

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
    big3 = torch.zeros(3 * col.P + 64, dtype=torch.uint8, device="cuda")
    refused(col, rgb(col, (big3[1:], frame, frame)))                            # a plane not 4-byte aligned
    col.close()
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0, lut_folder=_lutdir())
    refused(c, rgb(c))
    for lo, hi in ((0, 5), (5, 0), (3, 2), (-1, 4), (1, 16384), (7, 7)):       # (7, 7): a range without a grid entry
        refused(c, grey(c, j_min=lo, j_max=hi))
    refused(c, grey(c, fr=None))
    call = c.L.picsong_encode_frame_quality
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, 176868, 0, 0, c._p(buf), c._stream(), None, t, e))
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, 176868, 0, 0, c._p(buf), c._stream(), C.byref(j), None, e))
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, 176868, 0, 0, c._p(buf), c._stream(), C.byref(j), t, None))
    refused(c, lambda buf, j, t, e: call(c.h, c._p(frame), 0, 176868, 0, 0, None, c._stream(), C.byref(j), t, e))
    refused(c, batch(c, n=0))
    refused(c, batch(c, n=17))
    refused(c, batch(c, stride=c.P - 16))
    refused(c, batch(c, sstride=c.max_stream_shorts() - 1))
    big = torch.zeros(2 * c.P + 64, dtype=torch.uint8, device="cuda")
    refused(c, batch(c, fr=big[1:]))                                            # frames not 16-byte aligned
    # the context still works, and an unaligned single frame is accepted as picsong_encode_frame accepts it
    un = big[1:1 + c.P]
    un.copy_(frame.view(-1))
    j, _, sse = c.encode_frame_quality(un, 176868)
    assert (j, sse) == (1865, 176463)
    c.close()
    nolut = pa.Codec(W, H, wl=wl, lossy=True, qs=1.0)
    refused(nolut, grey(nolut))
    nolut.close()
