"""-m gpu: deep contexts (bit_depth 9..16, uint16 samples) through the C ABI and picsong_amd.Codec(bit_depth=...), against
deep_ref -- the CPU oracle's stage functions between a numpy level shift and a numpy clamp -- never against the code under
test.  No out-of-range input here (the range flag's cases run on the emulator)."""
import ctypes as C
import os

import numpy as np
import pytest

import deep_ref as D
import drop_ref as dr
import oracle_lib as orc

pytestmark = pytest.mark.gpu
ERR_ARG = -1
W, H, AW, AH = D.W, D.H, D.AW, D.AH
P = AW * AH
SENT = 0xA5C3


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


def _lutdir(lossy):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _codec(pa, bd, wl, lossy, qs=1.0, k=0.0, **kw):
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), k=k, bit_depth=bd, **kw)


def _dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _frames_at(torch, frames, gap=0, off=0):
    """n padded frames 2 P + gap bytes apart, the first `off` bytes behind a 16-byte boundary, sentinel everywhere else:
    (device tensor int16, element offset of frame 0, stride in bytes)."""
    n = len(frames)
    stride = 2 * P + gap
    host = np.full(32 + (off + (n - 1) * stride + 2 * P) // 2 + 32, SENT, np.uint16)
    for f, x in enumerate(frames):
        o = 32 + (off + f * stride) // 2
        host[o:o + P] = x.ravel()
    t = _dev16(torch, host)
    assert t.data_ptr() % 16 == 0
    return t, 32 + off // 2, stride


def _encode(c, torch, frames, gap=0, off=0, first_iter=0):
    t, at, stride = _frames_at(torch, frames, gap, off)
    n = len(frames)
    out = torch.full((n, c.max_stream_shorts()), 0x5A5A, dtype=torch.int16, device=c.dev)
    rc = c.L.picsong_encode_frames16(c.h, n, C.c_void_p(t.data_ptr() + 2 * at), stride, first_iter, C.c_void_p(out.data_ptr()),
                                     out.stride(0), c._stream())
    assert rc == 0, c.L.picsong_last_error()
    totals = c.last_totals(n)
    return [_u16(out[f, :totals[f]]) for f in range(n)]


def _decode(c, torch, streams, gap=0, off=0):
    n = len(streams)
    sb = np.full((n, c.max_stream_shorts()), 0xFFFF, np.uint16)
    for f, s in enumerate(streams):
        sb[f, :s.size] = s
    d_s = _dev16(torch, sb)
    t, at, stride = _frames_at(torch, [np.full((AH, AW), SENT, np.uint16)] * n, gap, off)
    rc = c.L.picsong_decode_frames16(c.h, n, C.c_void_p(d_s.data_ptr()), d_s.stride(0), C.c_void_p(t.data_ptr() + 2 * at), stride,
                                     c._stream())
    assert rc == 0, c.L.picsong_last_error()
    host = _u16(t)
    outs, mask = [], np.ones(host.size, bool)
    for f in range(n):
        o = at + f * stride // 2
        outs.append(host[o:o + P].reshape(AH, AW).copy())
        mask[o:o + P] = False
    assert (host[mask] == SENT).all(), "decoding writes exactly the 2 P bytes of each frame"
    return outs


CASES = [(False, 10, "saw", 5, 1.0, 0), (False, 12, "saw", 5, 1.0, 0), (False, 14, "saw", 5, 1.0, 0),
         (True, 12, "saw", 3, 1.0, 0), (True, 14, "saw", 3, 0.25, 0), (False, 12, "noise", 5, 1.0, 9)]


@pytest.mark.parametrize("lossy,bd,kind,wl,qs,raw", CASES, ids=[f"{'97' if c[0] else '53'}-{c[1]}-{c[2]}" for c in CASES])
def test_frame_sequences_match_the_composed_reference(pa, torch, lossy, bd, kind, wl, qs, raw):
    img, pad, coef, sizes, stream0 = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, raw)
    stream1 = D.encode(kind, bd, wl, lossy, qs, with_header=False)[4]
    want = D.decode(stream0, bd, wl, lossy, qs)
    c = _codec(pa, bd, wl, lossy, qs)
    got = _encode(c, torch, [pad, pad, pad])
    assert np.array_equal(got[0], stream0) and np.array_equal(got[1], stream1) and np.array_equal(got[2], stream1)
    dec = _decode(c, torch, got)
    for f in range(3):
        assert np.array_equal(dec[f], want), f
    if not lossy:
        assert np.array_equal(dec[0], pad), "the 5/3 round trip is exact"
    assert c.range_flag() == 0
    # the Codec's own methods: tensors in, tensors out
    s = c.encode_frames16(_dev16(torch, np.stack([pad, pad])))
    assert np.array_equal(_u16(s[0]), stream0) and np.array_equal(_u16(s[1]), stream1)
    sb = torch.full((1, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    sb[0, :stream0.size] = _dev16(torch, stream0)
    assert np.array_equal(_u16(c.decode_frames16(sb))[0], want)
    c.close()


@pytest.mark.parametrize("lossy,bd,kind,wl,qs", [(False, 12, "saw", 5, 1.0), (True, 12, "saw", 3, 1.0)])
def test_misaligned_pointers_and_the_element_wise_route_give_the_same_bytes(pa, torch, monkeypatch, lossy, bd, kind, wl, qs):
    img, pad, coef, sizes, stream0 = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, 0)
    want = D.decode(stream0, bd, wl, lossy, qs)
    c = _codec(pa, bd, wl, lossy, qs)
    for nofuse in (None, "1"):
        if nofuse:
            monkeypatch.setenv("PICSONG_DEEP_NOFUSE", nofuse)
        for gap, off in ((0, 2), (6, 0), (48, 0), (0, 8)):
            got = _encode(c, torch, [pad, pad], gap, off)
            assert np.array_equal(got[0], stream0), (nofuse, gap, off)
            dec = _decode(c, torch, got, gap, off)
            assert np.array_equal(dec[0], want) and np.array_equal(dec[1], want), (nofuse, gap, off)
    c.close()


def test_complexity_scalable_mode_and_decode_drop(pa, torch):
    img, pad, coef, sizes, stream = D.encode("saw", 12, 5, False, 1.0, k=0.5)
    assert D.max_coef(coef) < 32768
    c = _codec(pa, 12, 5, False, k=0.5)
    got = _encode(c, torch, [pad])
    assert np.array_equal(got[0], stream)
    assert np.array_equal(_decode(c, torch, got)[0], pad)
    c.close()
    lossy, bd, wl, qs = True, 12, 3, 1.0
    img, pad, coef, sizes, stream = D.encode("smooth", bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, 0)
    want = D.inverse(dr.drop_coefficients(stream, AW, AH, wl, orc.lut_for(lossy, wl), 2), bd, wl, lossy, qs)
    c = _codec(pa, bd, wl, lossy, qs)
    c.set_decode_drop(2)
    assert np.array_equal(_decode(c, torch, [stream])[0], want)
    c.close()


def test_images_in_the_grey16_layout(pa, torch):
    lossy, bd, kind, wl, qs = False, 12, "saw", 5, 1.0
    img, pad, coef, sizes, stream0 = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, 0)
    stream1 = D.encode(kind, bd, wl, lossy, qs, with_header=False)[4]
    c = _codec(pa, bd, wl, lossy, qs)
    pitch = 2 * W + 2
    span = (H - 1) * pitch + 2 * W
    fs = span + 6
    host = np.full(64 + fs + span + 64, 0xA5, np.uint8)
    for f in range(2):
        for y in range(H):
            o = 64 + f * fs + y * pitch
            host[o:o + 2 * W] = img[y].view(np.uint8)
    d = torch.from_numpy(host).cuda()
    im = c.image(d, pa.LAYOUT_GREY16, pitch, offset=64)
    got = c.encode_images(im, 2, fs)
    assert np.array_equal(_u16(got[0]), stream0) and np.array_equal(_u16(got[1]), stream1)
    # ingest on its own: the host pad's samples
    padded = c.ingest_frames(im, 2, fs)
    assert np.array_equal(_u16(padded)[0, 0], pad) and np.array_equal(_u16(padded)[1, 0], pad)
    assert np.array_equal(pa.pad_frame16(img, AW, AH), pad)
    # decode into a sentinel-filled image: the W x H samples and nothing else
    sb = torch.full((2, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    for f, s in enumerate((stream0, stream1)):
        sb[f, :s.size] = _dev16(torch, s)
    out = torch.full((host.size,), 0xA5, dtype=torch.uint8, device=c.dev)
    c.decode_images(sb, c.image(out, pa.LAYOUT_GREY16, pitch, offset=64), fs)
    assert np.array_equal(out.cpu().numpy(), host)
    c.close()


@pytest.mark.parametrize("lossy", [False, True])
def test_stage_seam(pa, torch, lossy):
    bd, wl, qs = 12, 3, 1.0
    pad = D.mirror_pad(D.inputs("smooth", bd, wl))
    c = _codec(pa, bd, wl, lossy, qs)
    d = _dev16(torch, pad)
    shifted = c.level_shift_fwd16(d)
    assert np.array_equal(shifted.cpu().numpy().view(np.uint32), D.level_shift(pad, bd, lossy).ravel().view(np.uint32))
    a = c.dwt_forward(shifted).cpu().numpy()
    b = c.dwt_forward_u16(d).cpu().numpy()
    want = D.forward(pad, bd, wl, lossy, qs)
    assert np.array_equal(a[:P].view(np.uint32), want[:P].view(np.uint32)) and np.array_equal(b[:P].view(np.uint32), want[:P].view(np.uint32))
    # the inverse seam: picsong_dwt_inverse, then picsong_level_shift_inv clamps at 2^bd - 1
    coef = np.trunc(want[:P]).astype(np.int64) * 5 // 4
    coef = coef.astype(np.int32).reshape(AH, AW)
    out = c.dwt_inverse(torch.from_numpy(coef).cuda())[c.extra:].clone()
    got = c.level_shift_inv(out).cpu().numpy()
    ref = D.inverse(coef, bd, wl, lossy, qs)
    assert ref.max() == (1 << bd) - 1 and ref.min() == 0
    assert np.array_equal(got.astype(np.uint16).reshape(AH, AW), ref)
    c.close()


def test_refusals_leave_the_outputs_untouched(pa, torch):
    bd, wl = 12, 3
    lut = _lutdir(False)
    deep = _codec(pa, bd, wl, False)
    shallow = pa.Codec(W, H, wl=wl, lut_folder=lut)
    L, s, vp = deep.L, deep._stream(), C.c_void_p
    ms = deep.max_stream_shorts()
    f16 = torch.full((3, P + 8), 0x1234, dtype=torch.int16, device=deep.dev)
    f8 = torch.full((3, P), 0x5A, dtype=torch.uint8, device=deep.dev)
    st = torch.full((3, ms), 0x5A5A, dtype=torch.int16, device=deep.dev)
    work = torch.full((P + deep.extra,), 0x5A5A5A5A, dtype=torch.int32, device=deep.dev)
    sse = torch.zeros(4, dtype=torch.int64, device=deep.dev)
    p16, p8, pst, pw = f16.data_ptr(), f8.data_ptr(), st.data_ptr(), work.data_ptr()
    fs16 = f16.stride(0) * 2
    j, tot, e = C.c_int(), (C.c_int * 4)(), (C.c_uint64 * 4)()

    def img(t, layout, pitch):
        return pa.Image(data=t.data_ptr(), pitch=pitch, plane_stride=0, layout=layout)

    with pytest.raises(pa.PicsongError):                    # deep + RGB at create
        pa.Codec(W, H, wl=wl, rgb=True, bit_depth=12)
    for bad in (7, 17):
        with pytest.raises(pa.PicsongError):
            pa.Codec(W, H, wl=wl, bit_depth=bad)
    d = deep.h
    refused = [
        # 8-bit frame calls on a deep context
        L.picsong_encode_frame(d, vp(p8), 0, vp(pst), s), L.picsong_encode_frames(d, 2, vp(p8), P, 0, vp(pst), ms, s),
        L.picsong_decode_frame(d, vp(pst), vp(p8), s), L.picsong_decode_frames(d, 2, vp(pst), ms, vp(p8), P, s),
        L.picsong_decode_frame_reduced(d, vp(pst), 1, vp(p8), s), L.picsong_decode_frames_reduced(d, 2, vp(pst), ms, 1, vp(p8), P, s),
        L.picsong_decode_frame_window(d, vp(pst), 0, 0, 0, 16, 16, vp(p8), 16, s),
        L.picsong_decode_frames_window(d, 2, vp(pst), ms, 0, 0, 0, 16, 16, vp(p8), 16, P, s),
        L.picsong_encode_frame_stripe(d, vp(p8), 0, 2, vp(pst), s), L.picsong_dwt_forward_band(d, vp(p8), 0, 64, vp(pw), s),
        L.picsong_train_frames(d, 1, vp(p8), P, s), L.picsong_frames_sse(d, 1, vp(p8), P, vp(p8), P, vp(sse.data_ptr()), s),
        L.picsong_level_shift_fwd(d, vp(p8), vp(pw), s), L.picsong_dwt_forward_u8(d, vp(p8), vp(pw), s),
        L.picsong_encode_frame_rate(d, vp(p8), 0, 1000, 0, 0, vp(pst), s, C.byref(j), tot),
        L.picsong_encode_frames_rate(d, 2, vp(p8), P, 0, 1000, 0, 0, vp(pst), ms, s, C.byref(j), tot),
        L.picsong_encode_frame_quality(d, vp(p8), 0, 1000, 0, 0, vp(pst), s, C.byref(j), tot, e),
        L.picsong_encode_frames_quality(d, 2, vp(p8), P, 0, 1000, 0, 0, vp(pst), ms, s, C.byref(j), tot, e),
        L.picsong_encode_rgb_frame(d, vp(p8), vp(p8 + P), vp(p8 + 2 * P), 1, vp(pst), ms, s),
        # the 8-bit layouts on a deep context
        L.picsong_encode_images(d, 1, C.byref(img(f8, pa.LAYOUT_GREY8, W)), 0, 0, vp(pst), ms, s),
        L.picsong_decode_images(d, 1, vp(pst), ms, C.byref(img(f8, pa.LAYOUT_GREY8, W)), 0, s),
        L.picsong_ingest_frames(d, 1, C.byref(img(f8, pa.LAYOUT_GREY8, W)), 0, vp(p16), 0, s),
        L.picsong_emit_frames(d, 1, vp(p16), 0, C.byref(img(f8, pa.LAYOUT_RGB24, 3 * W)), 0, s),
        # the *16 frame calls' own rules
        L.picsong_encode_frames16(d, 0, vp(p16), fs16, 0, vp(pst), ms, s), L.picsong_encode_frames16(d, 65, vp(p16), fs16, 0, vp(pst), ms, s),
        L.picsong_decode_frames16(d, 0, vp(pst), ms, vp(p16), fs16, s), L.picsong_decode_frames16(d, 65, vp(pst), ms, vp(p16), fs16, s),
        L.picsong_encode_frames16(d, 2, vp(p16), 2 * P - 2, 0, vp(pst), ms, s), L.picsong_decode_frames16(d, 2, vp(pst), ms, vp(p16), 2 * P - 2, s),
        L.picsong_encode_frames16(d, 2, vp(p16), 2 * P + 1, 0, vp(pst), ms, s),
        L.picsong_encode_frames16(d, 1, vp(p16 + 1), 0, 0, vp(pst), ms, s), L.picsong_decode_frames16(d, 1, vp(pst), ms, vp(p16 + 1), 0, s),
        L.picsong_encode_frames16(d, 2, vp(p16), fs16, 0, vp(pst), ms - 1, s),
        L.picsong_encode_frames16(d, 1, None, 0, 0, vp(pst), ms, s), L.picsong_decode_frames16(d, 1, vp(pst), ms, None, 0, s),
        L.picsong_level_shift_fwd16(d, vp(p16 + 1), vp(pw), s), L.picsong_dwt_forward_u16(d, vp(p16 + 1), vp(pw), s),
        # GREY16's alignment rules
        L.picsong_ingest_frames(d, 1, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W + 1)), 0, vp(p16), 0, s),
        L.picsong_ingest_frames(d, 1, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W - 2)), 0, vp(p16), 0, s),
        L.picsong_encode_images(d, 1, C.byref(pa.Image(data=p16 + 1, pitch=2 * W, plane_stride=0, layout=pa.LAYOUT_GREY16)), 0, 0, vp(pst), ms, s),
    ]
    h8 = shallow.h
    refused += [
        # ... and the uint16 calls and GREY16 on an 8-bit context
        L.picsong_encode_frames16(h8, 1, vp(p16), 0, 0, vp(pst), ms, s), L.picsong_decode_frames16(h8, 1, vp(pst), ms, vp(p16), 0, s),
        L.picsong_level_shift_fwd16(h8, vp(p16), vp(pw), s), L.picsong_dwt_forward_u16(h8, vp(p16), vp(pw), s),
        L.picsong_encode_images(h8, 1, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, 0, vp(pst), ms, s),
        L.picsong_decode_images(h8, 1, vp(pst), ms, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, s),
        L.picsong_ingest_frames(h8, 1, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, vp(p16), 0, s),
        L.picsong_emit_frames(h8, 1, vp(p16), 0, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, s),
    ]
    assert refused == [ERR_ARG] * len(refused), refused
    # -cp 3 in the frame calls
    cp3 = pa.Codec(W, H, wl=wl, cp=3, bit_depth=bd)
    assert L.picsong_encode_frames16(cp3.h, 1, vp(p16), 0, 0, vp(pst), ms, s) == ERR_ARG
    assert L.picsong_decode_frames16(cp3.h, 1, vp(pst), ms, vp(p16), 0, s) == ERR_ARG
    cp3.close()
    torch.cuda.synchronize()
    assert bool((f16 == 0x1234).all()) and bool((f8 == 0x5A).all()) and bool((st == 0x5A5A).all()) and bool((work == 0x5A5A5A5A).all())
    assert bool((sse == 0).all())
    deep.close()
    shallow.close()
