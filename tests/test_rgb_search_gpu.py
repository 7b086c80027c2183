"""-m gpu: the quantiser search over n RGB frames (picsong_encode_rgb_frames_rate / _quality) and picsong_train_rgb_frames
through the C ABI, against the reference procedures over the CPU oracle (rgb_search_ref.py): the chosen quantiser, the
3 n streams byte for byte, the lengths, the distortion reported and that of this library's own decode -- never against
the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as orc
import quality_ref as qr
import rate_ref as rr
import rgb_search_ref as ref
import train_cases as tc
import train_ref as tr

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_RATE, ERR_QUALITY = -1, -7, -8
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


LUTS = os.path.join(orc.LUT_DIR, "n1_lossy")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _codec(pa, W, H, wl, k=0.0, qs=0.75):
    return pa.Codec(W, H, wl=wl, lossy=True, qs=qs, lut_folder=LUTS, rgb=True, k=k)


def _header(pa, W, H, wl, j, k=0.0):
    """the oracle's nine header shorts carrying q(j)"""
    return orc.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=8, lossy=1, qs_1e4=j, components=3,
                           is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=int(round(k * 1000)))


def _planes(torch, W, H, n):
    """three [n, AH, AW] device arrays"""
    return [_dev(torch, p) for p in ref.padded_stack(W, H, n)]


def _call(torch, c, rgb, n, limit, quality, j_min=0, j_max=0, first_iter=0, mask=7, frame_stride=None):
    """The raw call into 3 n stream buffers with sentinel shorts behind picsong_max_stream_shorts each; returns
    (rc, j, totals, sse, the [3 n, stride] buffer)."""
    ms = c.max_stream_shorts()
    buf = torch.full((3 * n, ms + 64), SENTINEL, dtype=torch.int16, device="cuda")
    j, t, e = C.c_int(77), (C.c_int * (3 * n))(*([-5] * (3 * n))), (C.c_uint64 * (3 * n))(*([99] * (3 * n)))
    fs = (rgb[0].stride(0) if n > 1 else 0) if frame_stride is None else frame_stride
    head = (c.h, n, c._p(rgb[0]), c._p(rgb[1]), c._p(rgb[2]), fs, first_iter, mask, limit, j_min, j_max, c._p(buf), buf.stride(0),
            c._stream(), C.byref(j), t)
    rc = c.L.picsong_encode_rgb_frames_quality(*head, e) if quality else c.L.picsong_encode_rgb_frames_rate(*head)
    torch.cuda.synchronize()
    assert bool((buf[:, ms:] == SENTINEL).all()), "shorts behind picsong_max_stream_shorts were written"
    return rc, j.value, list(t), [int(v) for v in e], buf


def _assert_streams(buf, totals, want):
    assert totals == [w.size for w in want]
    for z, w in enumerate(want):
        assert np.array_equal(_u16(buf[z, :totals[z]]), w), f"frame {z // 3} component {z % 3}"


# ---- rate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n", [(200, 136, 2), (200, 136, 3), (201, 137, 2)])
def test_rate_table_rows(pa, torch, W, H, n):
    wl = 3
    target, j_want = ref.check_rate(W, H, wl, n)
    c = _codec(pa, W, H, wl)
    rgb = _planes(torch, W, H, n)
    rc, j, totals, _, buf = _call(torch, c, rgb, n, target, False)
    assert rc == 0, c.L.picsong_last_error()
    assert j == j_want
    hdr = _header(pa, W, H, wl, j)
    _assert_streams(buf, totals, ref.streams(W, H, wl, n, j, hdr, 0, 7))      # the header on all three components of frame 0
    assert sum(totals) == ref.CASES[(W, H, wl, n)][3] <= target
    assert c.last_totals(3 * n) == totals
    d_tot = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    assert c.L.picsong_copy_last_totals(c.h, c._stream(), 3 * n, C.c_void_p(d_tot.data_ptr())) == 0
    assert d_tot.cpu().tolist() == totals
    assert c.range_flag() == 0
    assert abs(c.params.qs - 0.75) < 1e-7
    # the context's own qs is unchanged: a plain call still codes at 0.75
    plain = c.encode_rgb_frames(*rgb, first_iter=0, header_mask=1)
    assert np.array_equal(_u16(plain[0])[:9], pa.header_pack(c.params))
    # ... and no header where the call does not hold the video's frame 0
    rc, j5, totals5, _, buf5 = _call(torch, c, rgb, n, target, False, first_iter=5)
    assert rc == 0 and j5 == j_want
    _assert_streams(buf5, totals5, ref.streams(W, H, wl, n, j, hdr, 5, 7))
    for z in range(3 * n):
        assert (_u16(buf5[z, :9]) == 0xFFFF).all()
    # the binding
    jb, streams = c.encode_rgb_frames_rate(*rgb, target)
    assert jb == j_want and [s.numel() for s in streams] == totals
    c.close()


def test_rate_of_eight_frames_codes_one_candidate_a_round(pa, torch):
    W, H, wl, n = 200, 136, 3, 8
    target, j_want = ref.check_rate(W, H, wl, n)
    c = _codec(pa, W, H, wl)
    rc, j, totals, _, buf = _call(torch, c, _planes(torch, W, H, n), n, target, False)
    assert rc == 0, c.L.picsong_last_error()
    assert j == j_want and sum(totals) == ref.CASES[(W, H, wl, n)][3]
    c.close()


def test_rate_with_one_candidate_a_round_forced(pa, torch, monkeypatch):
    W, H, wl, n = 200, 136, 3, 2
    target, j_want = ref.check_rate(W, H, wl, n)
    c = _codec(pa, W, H, wl)
    rgb = _planes(torch, W, H, n)
    rc3, j3, totals3, _, buf3 = _call(torch, c, rgb, n, target, False)
    monkeypatch.setenv("PICSONG_RATE_K", "1")
    rc1, j1, totals1, _, buf1 = _call(torch, c, rgb, n, target, False)
    assert rc1 == rc3 == 0 and j1 == j3 == j_want and totals1 == totals3
    assert torch.equal(buf1, buf3)
    _assert_streams(buf1, totals1, ref.streams(W, H, wl, n, j1, _header(pa, W, H, wl, j1), 0, 7))
    c.close()


def test_rate_of_one_frame_equals_the_single_frame_result(pa, torch):
    W, H, wl, n = 200, 136, 3, 1
    target, j_want = ref.check_rate(W, H, wl, n)
    assert j_want == 564
    c = _codec(pa, W, H, wl)
    rgb = _planes(torch, W, H, n)
    rc, j, totals, _, buf = _call(torch, c, rgb, n, target, False, mask=1)
    assert rc == 0 and j == j_want
    _assert_streams(buf, totals, ref.streams(W, H, wl, n, j, _header(pa, W, H, wl, j), 0, 1))
    j1, one = c.encode_rgb_frame_rate(rgb[0][0], rgb[1][0], rgb[2][0], target)       # (the single-frame call: header_mask = 1)
    assert j1 == j and [s.numel() for s in one] == totals
    for k in range(3):
        assert torch.equal(one[k], buf[k, :totals[k]])
    c.close()


# ---- quality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n", [(200, 136, 2), (201, 137, 2), (200, 136, 3)])
def test_quality_table_rows(pa, torch, W, H, n, monkeypatch):
    wl = 3
    limit, j_want, per = ref.check_quality(W, H, wl, n)
    flat = [v for fr in per for v in fr]
    c = _codec(pa, W, H, wl)
    rgb = _planes(torch, W, H, n)
    rc, j, totals, sse, buf = _call(torch, c, rgb, n, limit, True)
    assert rc == 0, c.L.picsong_last_error()
    assert j == j_want
    assert sse == flat and sum(sse) <= limit
    want = ref.streams(W, H, wl, n, j, _header(pa, W, H, wl, j), 0, 7)
    _assert_streams(buf, totals, want)
    assert c.last_totals(3 * n) == totals
    assert abs(c.params.qs - 0.75) < 1e-7
    # the distortion of this library's own decode at q(j)
    d = _codec(pa, W, H, wl, qs=rr.q(j))
    back = d.decode_rgb_frames(buf[:, :c.max_stream_shorts()])
    host = [p.cpu().numpy() for p in rgb]
    assert [qr.sse(back[k][f].cpu().numpy()[:H, :W], host[k][f][:H, :W]) for f in range(n) for k in range(3)] == sse
    d.close()
    # the unfused tail: the same j, sums and bytes
    monkeypatch.setenv("PICSONG_RGB_SSE_FUSED", "0")
    rc0, j0, totals0, sse0, buf0 = _call(torch, c, rgb, n, limit, True)
    assert rc0 == 0 and (j0, totals0, sse0) == (j, totals, sse) and torch.equal(buf0, buf)
    monkeypatch.delenv("PICSONG_RGB_SSE_FUSED")
    jb, streams, e = c.encode_rgb_frames_quality(*rgb, limit)                          # the binding
    assert jb == j and e == sse and [s.numel() for s in streams] == totals
    c.close()


def test_planes_at_a_four_byte_offset(pa, torch):
    """R, G, B back to back per frame, 4 bytes off their 16-byte alignment: the separate colour transform ahead of the
    unit-step transform, dword loads of the input in the fused tail; the same results."""
    W, H, wl, n = 200, 136, 3, 2
    target, j_rate = ref.check_rate(W, H, wl, n)
    limit, j_q, per = ref.check_quality(W, H, wl, n)
    c = _codec(pa, W, H, wl)
    P = c.P
    stack = ref.padded_stack(W, H, n)
    flat = np.concatenate([np.zeros(4, np.uint8)] + [stack[k][f].ravel() for f in range(n) for k in range(3)])
    t = _dev(torch, flat)
    assert t.data_ptr() % 16 == 0
    rgb = [t[4:], t[4 + P:], t[4 + 2 * P:]]
    rc, j, totals, _, buf = _call(torch, c, rgb, n, target, False, frame_stride=3 * P)
    assert rc == 0 and j == j_rate
    _assert_streams(buf, totals, ref.streams(W, H, wl, n, j, _header(pa, W, H, wl, j), 0, 7))
    rc, j, totals, sse, buf = _call(torch, c, rgb, n, limit, True, frame_stride=3 * P)
    assert rc == 0 and j == j_q and sse == [v for fr in per for v in fr]
    _assert_streams(buf, totals, ref.streams(W, H, wl, n, j, _header(pa, W, H, wl, j), 0, 7))
    c.close()


def test_complexity_scalable_context(pa, torch):
    """-k 0.5: the coder changes, the quantised coefficients and so the distortion do not -- the quality result is the
    table's, the streams the oracle's at that k; the rate result is the procedure's over the oracle's sizes at that k."""
    W, H, wl, n, k = 200, 136, 3, 2, 0.5
    limit, j_q, per = ref.check_quality(W, H, wl, n)
    c = _codec(pa, W, H, wl, k=k)
    rgb = _planes(torch, W, H, n)
    rc, j, totals, sse, buf = _call(torch, c, rgb, n, limit, True)
    assert rc == 0, c.L.picsong_last_error()
    assert j == j_q and sse == [v for fr in per for v in fr]
    _assert_streams(buf, totals, ref.streams(W, H, wl, n, j, _header(pa, W, H, wl, j, k), 0, 7, k=k))
    target = ref.CASES[(W, H, wl, n)][1]
    res = ref.rate_result(W, H, wl, n, k=k)
    assert res.j is not None and res.size <= target and (res.next_size is None or res.next_size > target)
    rc, j, totals, _, buf = _call(torch, c, rgb, n, target, False)
    assert rc == 0 and j == res.j and sum(totals) == res.size
    _assert_streams(buf, totals, ref.streams(W, H, wl, n, j, _header(pa, W, H, wl, j, k), 0, 7, k=k))
    c.close()


def test_nothing_fits(pa, torch):
    W, H, wl, n = 200, 136, 3, 2
    res = ref.rate_result(W, H, wl, n, target=203)
    assert res.first_size == 204 and res.j is None         # the oracle's size(G'[0]) is one short above the target
    c = _codec(pa, W, H, wl)
    rgb = _planes(torch, W, H, n)
    rc, j, _, _, _ = _call(torch, c, rgb, n, 203, False)
    assert rc == ERR_RATE and j == 0
    rc, j, _, _, _ = _call(torch, c, rgb, n, 0, True)      # max_sse = 0: a legal request that nothing meets
    assert rc == ERR_QUALITY and j == 0
    with pytest.raises(pa.RateError):
        c.encode_rgb_frames_rate(*rgb, 203)
    with pytest.raises(pa.QualityError):
        c.encode_rgb_frames_quality(*rgb, 0)
    target, j_want = ref.check_rate(W, H, wl, n)           # the context still works
    assert c.encode_rgb_frames_rate(*rgb, target)[0] == j_want
    c.close()


# ---- refusals: PICSONG_ERR_ARG, nothing launched, the outputs untouched ------------------------------------------------------
def test_refusals_leave_the_outputs_alone(pa, torch):
    W, H, wl, n = 200, 136, 3, 2
    r = _codec(pa, W, H, wl)
    grey = pa.Codec(W, H, wl=wl, lossy=True, qs=0.75, lut_folder=LUTS)
    cp3 = pa.Codec(W, H, wl=wl, lossy=True, qs=0.75, rgb=True, cp=3)
    lossless = pa.Codec(W, H, wl=wl, lossy=False, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossless"), rgb=True)
    bare = pa.Codec(W, H, wl=wl, lossy=True, qs=0.75, rgb=True)
    P, ms = r.P, r.max_stream_shorts()
    planes = torch.full((22 * 3 * P + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    streams = torch.full((3 * n, ms), SENTINEL, dtype=torch.int16, device="cuda")
    vp = C.c_void_p
    pr, st = planes.data_ptr(), streams.data_ptr()
    assert pr % 16 == 0
    j, t, e = C.c_int(77), (C.c_int * 66)(*([-5] * 66)), (C.c_uint64 * 66)(*([99] * 66))

    def call(quality, c=r, n_=n, r_=pr, g_=pr + P, b_=pr + 2 * P, fs=3 * P, st_=st, stride=ms, limit=5000, lo=0, hi=0, hj=True, ht=True,
             he=True):
        head = (c.h, n_, vp(r_), vp(g_), vp(b_), fs, 0, 7, limit, lo, hi, vp(st_), stride, c._stream(), C.byref(j) if hj else None,
                t if ht else None)
        if quality:
            return c.L.picsong_encode_rgb_frames_quality(*head, e if he else None)
        return c.L.picsong_encode_rgb_frames_rate(*head)

    bad = [dict(c=lossless), dict(c=cp3), dict(c=grey), dict(c=bare), dict(n_=0), dict(n_=22), dict(fs=P - 4), dict(fs=3 * P + 2),
           dict(fs=3 * P - 16), dict(r_=pr + 1), dict(g_=pr + P + 2), dict(b_=pr + 2 * P + 3), dict(stride=ms - 1), dict(r_=None),
           dict(g_=None), dict(b_=None), dict(st_=None), dict(hj=False), dict(ht=False), dict(lo=5, hi=4), dict(lo=0, hi=9),
           dict(lo=1, hi=16384), dict(lo=7, hi=7)]
    for kw in bad:
        assert call(False, **kw) == ERR_ARG, ("rate", kw)
        assert call(True, **kw) == ERR_ARG, ("quality", kw)
    assert call(False, limit=0) == ERR_ARG                 # target_shorts = 0 (max_sse = 0 is a legal request)
    assert call(True, he=False) == ERR_ARG
    # picsong_train_rgb_frames: the refusals of the single-frame call, the n and the stride checks
    r.train_begin()
    grey.train_begin()
    s = r._stream()
    tcall = r.L.picsong_train_rgb_frames
    assert tcall(grey.h, n, vp(pr), vp(pr + P), vp(pr + 2 * P), 3 * P, s) == ERR_ARG
    assert tcall(bare.h, n, vp(pr), vp(pr + P), vp(pr + 2 * P), 3 * P, s) == ERR_ARG        # no picsong_train_begin
    for kw in (dict(n_=0), dict(n_=22), dict(fs=P - 4), dict(fs=3 * P + 2), dict(r_=pr + 1), dict(g_=None)):
        a = dict(n_=n, r_=pr, g_=pr + P, b_=pr + 2 * P, fs=3 * P)
        a.update(kw)
        assert tcall(r.h, a["n_"], vp(a["r_"]), vp(a["g_"]), vp(a["b_"]), a["fs"], s) == ERR_ARG, kw
    assert not r.train_counts(0).any() and not r.train_counts(2).any()
    torch.cuda.synchronize()
    assert bool((streams == SENTINEL).all()) and bool((planes == 0xA5).all())
    assert j.value == 77 and list(t) == [-5] * 66 and list(e) == [99] * 66
    for c in (r, grey, cp3, lossless, bare):
        c.close()


# ---- training -----------------------------------------------------------------------------------------------------------
def test_train_rgb_frames_equals_the_single_frame_calls_and_the_model(pa, torch):
    W, H, wl, n, qs = 128, 128, 2, 3, 0.5
    stack = ref.padded_stack(W, H, n)
    rgb = [_dev(torch, p) for p in stack]
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=qs, rgb=True)
    c.train_begin()
    c.train_rgb_frames(*rgb)
    got = [c.train_counts(k).copy() for k in range(3)]
    c.train_reset()
    for f in range(n):
        c.train_rgb_frame(*[rgb[k][f] for k in range(3)])
    AH, AW = stack[0].shape[1:]
    for k in range(3):
        assert got[k].any()
        assert np.array_equal(got[k], c.train_counts(k)), k
        want = 0
        for f in range(n):
            comp = orc.rgb_forward(*[stack[x][f] for x in range(3)], True)[k]
            coef = orc.dwt_forward(comp.reshape(AH, AW), wl, qs)[:AW * AH].reshape(AH, AW)
            want = want + tr.counts(coef, wl, tc.GEO)[0]
        assert np.array_equal(got[k], want), k
    c.close()
