"""-m gpu: deep RGB contexts (bit_depth 9..16, components 3, is_rgb 1: three uint16 planes a frame) through the C ABI and
picsong_amd.Codec(bit_depth=, is_rgb=True), against deep_rgb_ref -- the CPU oracle's stage functions between a numpy colour
transform and a numpy inverse -- never against the code under test.  No out-of-range input here."""
import ctypes as C
import os

import numpy as np
import pytest

import deep_ref as D
import deep_rgb_ref as R
import drop_ref as dr
import oracle_lib as orc

pytestmark = pytest.mark.gpu
ERR_ARG = -1
W, H, AW, AH = R.W, R.H, R.AW, R.AH
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
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), k=k, bit_depth=bd, is_rgb=True, **kw)


def _dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _planes_at(torch, frames, gap=0, pgap=0, off=0):
    """n frames' padded R, G, B planes: plane c of frame f at byte off + f * stride + c * (2 P + pgap) behind a 16-byte
    boundary, stride = 3 (2 P + pgap) + gap, the sentinel everywhere else.  (device tensor int16, the three element offsets
    of frame 0's planes, the stride in bytes)"""
    n = len(frames)
    pstep = 2 * P + pgap
    stride = 3 * pstep + gap
    host = np.full(32 + (off + n * stride) // 2 + 32, SENT, np.uint16)
    for f, planes in enumerate(frames):
        for c in range(3):
            o = 32 + (off + f * stride + c * pstep) // 2
            host[o:o + P] = np.asarray(planes[c]).ravel()
    t = _dev16(torch, host)
    assert t.data_ptr() % 16 == 0
    return t, [32 + (off + c * pstep) // 2 for c in range(3)], stride


def _encode(c, torch, frames, gap=0, pgap=0, off=0, first_iter=0, header_mask=7):
    t, at, stride = _planes_at(torch, frames, gap, pgap, off)
    n = len(frames)
    out = torch.full((3 * n, c.max_stream_shorts()), 0x5A5A, dtype=torch.int16, device=c.dev)
    p = [C.c_void_p(t.data_ptr() + 2 * a) for a in at]
    rc = c.L.picsong_encode_rgb_frames16(c.h, n, p[0], p[1], p[2], stride, first_iter, header_mask, C.c_void_p(out.data_ptr()),
                                         out.stride(0), c._stream())
    assert rc == 0, c.L.picsong_last_error()
    totals = c.last_totals(3 * n)
    return [_u16(out[z, :totals[z]]) for z in range(3 * n)]


def _decode(c, torch, streams, gap=0, pgap=0, off=0):
    """streams: 3 n of them; the n frames' planes, and the proof that nothing but their 2 P bytes each was written."""
    n = len(streams) // 3
    sb = np.full((3 * n, c.max_stream_shorts()), 0xFFFF, np.uint16)
    for z, s in enumerate(streams):
        sb[z, :s.size] = s
    d_s = _dev16(torch, sb)
    blank = [np.full((AH, AW), SENT, np.uint16)] * 3
    t, at, stride = _planes_at(torch, [blank] * n, gap, pgap, off)
    p = [C.c_void_p(t.data_ptr() + 2 * a) for a in at]
    rc = c.L.picsong_decode_rgb_frames16(c.h, n, C.c_void_p(d_s.data_ptr()), d_s.stride(0), p[0], p[1], p[2], stride, c._stream())
    assert rc == 0, c.L.picsong_last_error()
    host = _u16(t)
    outs, mask = [], np.ones(host.size, bool)
    for f in range(n):
        planes = []
        for k in range(3):
            o = at[k] + f * stride // 2
            planes.append(host[o:o + P].reshape(AH, AW).copy())
            mask[o:o + P] = False
        outs.append(planes)
    assert (host[mask] == SENT).all(), "decoding writes exactly the 2 P bytes of each plane"
    return outs


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


CASES = [R.row(False, 10, "saw"), R.row(False, 12, "saw"), R.row(False, 12, "noise"), R.row(True, 12, "saw"), R.row(True, 16, "noise")]


@pytest.mark.parametrize("case", CASES, ids=[R.row_id(r) for r in CASES])
def test_frame_sequences_match_the_composed_reference(pa, torch, case):
    lossy, bd, kind, wl, qs, want_max, want_raw = case
    img, pad, comp, coef, sizes, with_hdr = R.encode(kind, bd, wl, lossy, qs)
    R.check_precondition(coef, sizes, want_max, want_raw)
    bare = R.encode(kind, bd, wl, lossy, qs, header_mask=0)[5]
    want = R.decode(with_hdr, bd, wl, lossy, qs)
    c = _codec(pa, bd, wl, lossy, qs)
    one = _encode(c, torch, [pad])
    assert _same(one, with_hdr)
    three = _encode(c, torch, [pad, pad, pad])
    assert _same(three, list(with_hdr) + list(bare) * 2)
    for streams in (one, three):
        for planes in _decode(c, torch, streams):
            assert _same(planes, want)
    if not lossy:
        assert _same(want, pad), "the 5/3 round trip is exact"
    assert c.range_flag() == 0
    # the Codec's own methods: tensors in, tensors out
    planes = [_dev16(torch, np.stack([pad[k], pad[k]])) for k in range(3)]
    s = c.encode_rgb_frames16(*planes)
    assert _same([_u16(x) for x in s], list(with_hdr) + list(bare))
    sb = torch.full((3, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    for k in range(3):
        sb[k, :with_hdr[k].size] = _dev16(torch, with_hdr[k])
    assert _same([_u16(o)[0] for o in c.decode_rgb_frames16(sb)], want)
    c.close()


def _other_frame(bd, wl):
    """A second and third frame that differ from the first: its planes rotated."""
    pad = R.encode("saw", bd, wl, False)[1]
    return [pad[1], pad[2], pad[0]], [pad[2], pad[0], pad[1]]


@pytest.mark.parametrize("lossy,wl", [(False, 5), (True, 3)])
def test_three_frames_a_call_against_three_calls(pa, torch, lossy, wl):
    bd = 12
    f0 = R.encode("saw", bd, wl, False)[1]
    f1, f2 = _other_frame(bd, wl)
    c = _codec(pa, bd, wl, lossy)
    singles = [_encode(c, torch, [f], first_iter=i) for i, f in enumerate((f0, f1, f2))]
    batch = _encode(c, torch, [f0, f1, f2])
    assert _same(batch, singles[0] + singles[1] + singles[2])
    dec = _decode(c, torch, batch, gap=32)
    for f in range(3):
        assert _same(dec[f], _decode(c, torch, batch[3 * f:3 * f + 3])[0]), f
    if not lossy:
        assert _same(dec[0], f0) and _same(dec[1], f1) and _same(dec[2], f2)
    c.close()


@pytest.mark.parametrize("lossy,wl", [(False, 5), (True, 3)])
def test_frame_calls_against_the_stage_calls(pa, torch, lossy, wl):
    bd, kind = 12, "saw"
    img, pad, comp, coef, sizes, streams = R.encode(kind, bd, wl, lossy, header_mask=1)
    c = _codec(pa, bd, wl, lossy)
    d = [_dev16(torch, p) for p in pad]
    planes = c.rgb_forward16(*d)
    for k in range(3):
        assert np.array_equal(planes[k].cpu().numpy().view(np.uint32), comp[k].ravel().view(np.uint32)), k
    staged = [_u16(c.encode_plane(planes[k], k, k == 0)).copy() for k in range(3)]
    assert _same(staged, streams)
    assert _same(_encode(c, torch, [pad], header_mask=1), staged)
    # ... and the mirror: 3 x picsong_decode_plane + picsong_rgb_inverse16
    sb = torch.full((3, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    for k in range(3):
        sb[k, :streams[k].size] = _dev16(torch, streams[k])
    outs = [c.decode_plane(sb[k], k).clone() for k in range(3)]
    want_c = R.synthesis([R.decode_coefficients(streams[k], wl, lossy, k) for k in range(3)], wl, lossy)
    for k in range(3):
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), want_c[k].ravel().view(np.uint32)), k
    got = [_u16(o) for o in c.rgb_inverse16(*outs)]
    assert _same(got, R.decode(streams, bd, wl, lossy))
    assert _same(got, _decode(c, torch, streams)[0])
    c.close()


def test_colour_transforms_at_the_ends_of_the_range(pa, torch):
    """0 and 65535 forced into every plane (read unsigned), and both clamp ends of the inverse."""
    rng = np.random.default_rng(5)
    for bd in (9, 12, 16):
        for lossy in (False, True):
            c = _codec(pa, bd, 3, lossy)
            pad = [rng.integers(0, 1 << bd, (AH, AW)).astype(np.uint16) for _ in range(3)]
            for k in range(3):
                pad[k][k, :8] = [0, 65535, 0, 65535, (1 << bd) - 1, 1 << (bd - 1), 65535, 0]
            want = R.forward(pad[0], pad[1], pad[2], bd, lossy)
            got = c.rgb_forward16(*[_dev16(torch, p) for p in pad])
            for k in range(3):
                assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want[k].ravel().view(np.uint32)), (bd, lossy, k)
            # components scaled past the range: both clamp ends occur
            comp = [(w.astype(np.float64) * 1.5).astype(w.dtype) for w in want]
            ref = R.inverse(comp[0], comp[1], comp[2], bd)
            assert min(r.min() for r in ref) == 0 and max(r.max() for r in ref) == (1 << bd) - 1
            out = c.rgb_inverse16(*[torch.from_numpy(x).cuda() for x in comp])
            assert _same([_u16(o) for o in out], ref), (bd, lossy)
            c.close()


@pytest.mark.parametrize("lossy,wl", [(False, 5), (True, 3)])
def test_misaligned_planes_and_nofuse_give_the_same_bytes(pa, torch, monkeypatch, lossy, wl):
    bd, kind = 12, "saw"
    img, pad, comp, coef, sizes, with_hdr = R.encode(kind, bd, wl, lossy)
    bare = R.encode(kind, bd, wl, lossy, header_mask=0)[5]
    want = R.decode(with_hdr, bd, wl, lossy)
    c = _codec(pa, bd, wl, lossy)
    for nofuse in (None, "1"):
        if nofuse:
            monkeypatch.setenv("PICSONG_DEEP_NOFUSE", nofuse)
        for gap, pgap, off in ((0, 0, 2), (6, 0, 0), (0, 2, 0), (48, 16, 0), (0, 0, 8), (2, 6, 4)):
            got = _encode(c, torch, [pad, pad], gap, pgap, off)
            assert _same(got, list(with_hdr) + list(bare)), (nofuse, gap, pgap, off)
            dec = _decode(c, torch, got, gap, pgap, off)
            assert _same(dec[0], want) and _same(dec[1], want), (nofuse, gap, pgap, off)
    c.close()


def test_header_mask_and_first_iter_place_the_header(pa, torch):
    lossy, bd, kind, wl = False, 10, "saw", 5
    pad = R.encode(kind, bd, wl, lossy)[1]
    c = _codec(pa, bd, wl, lossy)
    for first_iter, mask in ((0, 7), (0, 1), (0, 5), (-1, 7), (-2, 2), (1, 7), (-3, 7), (0, 0)):
        want = []
        for f in range(3):
            want += list(R.encode(kind, bd, wl, lossy, header_mask=mask if first_iter + f == 0 else 0)[5])
        assert _same(_encode(c, torch, [pad] * 3, first_iter=first_iter, header_mask=mask), want), (first_iter, mask)
    c.close()


def test_complexity_scalable_mode_and_decode_drop(pa, torch):
    lossy, bd, kind, wl = False, 12, "saw", 5
    img, pad, comp, coef, sizes, streams = R.encode(kind, bd, wl, lossy, k=0.5)
    assert max(R.max_coef(coef)) < 32768
    c = _codec(pa, bd, wl, lossy, k=0.5)
    got = _encode(c, torch, [pad])
    assert _same(got, streams)
    assert _same(_decode(c, torch, got)[0], pad)
    c.close()
    lossy, bd, kind, wl, qs = R.row(True, 12, "smooth")[:5]
    streams = R.encode(kind, bd, wl, lossy, qs)[5]
    comps = R.synthesis([dr.drop_coefficients(streams[k], AW, AH, wl, R.lut(lossy, wl, k), 2) for k in range(3)], wl, lossy, qs)
    want = R.inverse(comps[0], comps[1], comps[2], bd)
    c = _codec(pa, bd, wl, lossy, qs)
    c.set_decode_drop(2)
    assert _same(_decode(c, torch, streams)[0], want)
    c.close()


def _image_host(planes, layout, pitch, fs, n, alpha):
    """n copies of a frame in a 16-bit colour layout: (bytes, offset of frame 0, plane_stride), 0xA5 around every row."""
    spp = {7: 1, 8: 3, 9: 4}[layout]
    row = 2 * W * spp
    span = (H - 1) * pitch + row
    ps = span + 8 if layout == 7 else 0
    host = np.full(64 + (n - 1) * fs + span + 2 * ps + 64, 0xA5, np.uint8)
    for f in range(n):
        for y in range(H):
            if layout == 7:
                for c in range(3):
                    o = 64 + f * fs + c * ps + y * pitch
                    host[o:o + row] = planes[c][y].view(np.uint8)
            else:
                px = np.full((W, spp), alpha, np.uint16)
                for c in range(3):
                    px[:, c] = planes[c][y]
                o = 64 + f * fs + y * pitch
                host[o:o + row] = px.reshape(-1).view(np.uint8)
    return host, 64, ps


@pytest.mark.parametrize("layout,extra", [(7, 4), (8, 2), (9, 0), (8, 4)], ids=["planar3_16", "rgb48-2byte", "rgba64", "rgb48-dwords"])
def test_images_in_the_16_bit_colour_layouts(pa, torch, layout, extra):
    lossy, bd, kind, wl = False, 12, "saw", 5
    mx = (1 << bd) - 1
    img, pad, comp, coef, sizes, with_hdr = R.encode(kind, bd, wl, lossy)
    bare = R.encode(kind, bd, wl, lossy, header_mask=0)[5]
    assert (pa.LAYOUT_PLANAR3_16, pa.LAYOUT_RGB48, pa.LAYOUT_RGBA64) == (7, 8, 9)
    c = _codec(pa, bd, wl, lossy)
    spp = {7: 1, 8: 3, 9: 4}[layout]
    pitch = 2 * W * spp + extra
    span = (H - 1) * pitch + 2 * W * spp
    fs = (3 * (span + 8) if layout == 7 else span) + 12
    host, at, ps = _image_host(img, layout, pitch, fs, 2, 0x1357)
    d = torch.from_numpy(host).cuda()
    im = c.image(d, layout, pitch, plane_stride=ps, offset=at)
    got = c.encode_rgb_images(im, 2, fs)
    assert _same([_u16(g) for g in got], list(with_hdr) + list(bare)), "byte-identical to the frame call on host-padded planes"
    # ingest on its own: the host pad's samples, three planes a frame
    padded = _u16(c.ingest_frames(im, 2, fs))
    for f in range(2):
        for k in range(3):
            assert np.array_equal(padded[f, k], pad[k]), (f, k)
            assert np.array_equal(pa.pad_frame16(img[k], AW, AH), pad[k])
    # decode into a sentinel-filled image: the W x H pixels and nothing else, alpha = 2^bd - 1
    want, _, _ = _image_host(img, layout, pitch, fs, 2, mx)
    sb = torch.full((6, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    for z, s in enumerate(list(with_hdr) + list(bare)):
        sb[z, :s.size] = _dev16(torch, s)
    out = torch.full((host.size,), 0xA5, dtype=torch.uint8, device=c.dev)
    c.decode_rgb_images(sb, c.image(out, layout, pitch, plane_stride=ps, offset=at), fs)
    assert np.array_equal(out.cpu().numpy(), want)
    # ... and emit on its own
    out2 = torch.full((host.size,), 0xA5, dtype=torch.uint8, device=c.dev)
    c.emit_frames(_dev16(torch, padded), c.image(out2, layout, pitch, plane_stride=ps, offset=at), 2, fs)
    assert np.array_equal(out2.cpu().numpy(), want)
    c.close()


def test_refusals_leave_the_outputs_untouched(pa, torch):
    bd, wl = 12, 3
    lut = _lutdir(False)
    deep = _codec(pa, bd, wl, False)
    grey16 = pa.Codec(W, H, wl=wl, lut_folder=lut, bit_depth=bd)
    rgb8 = pa.Codec(W, H, wl=wl, lut_folder=lut, rgb=True)
    grey8 = pa.Codec(W, H, wl=wl, lut_folder=lut)
    L, s, vp = deep.L, deep._stream(), C.c_void_p
    ms = deep.max_stream_shorts()
    f16 = torch.full((9, P + 8), 0x1234, dtype=torch.int16, device=deep.dev)
    f8 = torch.full((9, P), 0x5A, dtype=torch.uint8, device=deep.dev)
    st = torch.full((9, ms), 0x5A5A, dtype=torch.int16, device=deep.dev)
    work = torch.full((3, P + deep.extra), 0x5A5A5A5A, dtype=torch.int32, device=deep.dev)
    sse = torch.zeros(16, dtype=torch.int64, device=deep.dev)
    p16, p8, pst, pw = f16.data_ptr(), f8.data_ptr(), st.data_ptr(), work.data_ptr()
    row16 = f16.stride(0) * 2
    r16, g16, b16 = vp(p16), vp(p16 + row16), vp(p16 + 2 * row16)
    r8, g8, b8 = vp(p8), vp(p8 + P), vp(p8 + 2 * P)
    w0, w1, w2 = vp(pw), vp(pw + work.stride(0) * 4), vp(pw + 2 * work.stride(0) * 4)
    fs16 = 3 * row16
    j, tot, e = C.c_int(), (C.c_int * 16)(), (C.c_uint64 * 16)()

    def img(t, layout, pitch, plane_stride=0):
        return pa.Image(data=t.data_ptr(), pitch=pitch, plane_stride=plane_stride, layout=layout)

    # Codec(rgb=True) stays the 8-bit RGB context: with a deeper bit_depth it is refused as ever (the deep one: is_rgb=True)
    with pytest.raises(pa.PicsongError):
        pa.Codec(W, H, wl=wl, rgb=True, bit_depth=12)
    # components 3 without is_rgb stays refused at creation, at any depth
    h = C.c_void_p()
    for depth in (8, 12):
        prm = pa.make_params(W, H, wl=wl, bit_depth=depth)
        prm.components = 3
        assert L.picsong_ctx_create(C.byref(prm), 0, C.byref(h)) == ERR_ARG
    d = deep.h
    refused = [
        # every call that takes or returns uint8_t frames, the 8-bit RGB calls included
        L.picsong_encode_rgb_frame(d, r8, g8, b8, 1, vp(pst), ms, s), L.picsong_encode_rgb_frames(d, 2, r8, g8, b8, 3 * P, 0, 7, vp(pst), ms, s),
        L.picsong_decode_rgb_frame(d, vp(pst), ms, r8, g8, b8, s), L.picsong_decode_rgb_frames(d, 2, vp(pst), ms, r8, g8, b8, 3 * P, s),
        L.picsong_decode_rgb_frame_reduced(d, vp(pst), ms, 1, r8, g8, b8, s),
        L.picsong_decode_rgb_frames_reduced(d, 2, vp(pst), ms, 1, r8, g8, b8, 3 * P, s),
        L.picsong_decode_rgb_frame_window(d, vp(pst), ms, 0, 0, 0, 16, 16, r8, g8, b8, 16, s),
        L.picsong_decode_rgb_frames_window(d, 2, vp(pst), ms, 0, 0, 0, 16, 16, r8, g8, b8, 16, 3 * P, s),
        L.picsong_rgb_forward(d, r8, g8, b8, w0, w1, w2, s), L.picsong_rgb_inverse(d, w0, w1, w2, r8, g8, b8, s),
        L.picsong_encode_frame(d, r8, 0, vp(pst), s), L.picsong_encode_frames(d, 2, r8, P, 0, vp(pst), ms, s),
        L.picsong_decode_frame(d, vp(pst), r8, s), L.picsong_decode_frames(d, 2, vp(pst), ms, r8, P, s),
        L.picsong_encode_frame_stripe(d, r8, 0, 2, vp(pst), s), L.picsong_dwt_forward_band(d, r8, 0, 64, w0, s),
        L.picsong_level_shift_fwd(d, r8, w0, s), L.picsong_dwt_forward_u8(d, r8, w0, s),
        L.picsong_frames_sse(d, 1, r8, P, r8, P, vp(sse.data_ptr()), s),
        # the searches, training on frames
        L.picsong_encode_rgb_frame_rate(d, r8, g8, b8, 1, 1000, 0, 0, vp(pst), ms, s, C.byref(j), tot),
        L.picsong_encode_rgb_frames_rate(d, 2, r8, g8, b8, 3 * P, 0, 7, 1000, 0, 0, vp(pst), ms, s, C.byref(j), tot),
        L.picsong_encode_rgb_frame_quality(d, r8, g8, b8, 1, 1000, 0, 0, vp(pst), ms, s, C.byref(j), tot, e),
        L.picsong_encode_rgb_frames_quality(d, 2, r8, g8, b8, 3 * P, 0, 7, 1000, 0, 0, vp(pst), ms, s, C.byref(j), tot, e),
        L.picsong_train_frames(d, 1, r8, P, s), L.picsong_train_rgb_frames(d, 1, r8, g8, b8, 0, s),
        # the grey *16 frame calls
        L.picsong_encode_frames16(d, 1, r16, 0, 0, vp(pst), ms, s), L.picsong_decode_frames16(d, 1, vp(pst), ms, r16, 0, s),
        # the 8-bit layouts and GREY16 in the layout and image calls, the grey and single-frame image calls whatever the layout
        L.picsong_encode_rgb_images(d, 1, C.byref(img(f8, pa.LAYOUT_RGB24, 3 * W)), 0, 0, 7, vp(pst), ms, s),
        L.picsong_decode_rgb_images(d, 1, vp(pst), ms, C.byref(img(f8, pa.LAYOUT_RGB24, 3 * W)), 0, s),
        L.picsong_encode_rgb_image(d, C.byref(img(f8, pa.LAYOUT_PLANAR3, W, P)), 1, vp(pst), ms, s),
        L.picsong_decode_rgb_image(d, vp(pst), ms, C.byref(img(f8, pa.LAYOUT_PLANAR3, W, P)), s),
        L.picsong_decode_rgb_images_reduced(d, 1, vp(pst), ms, 1, C.byref(img(f8, pa.LAYOUT_RGB24, 3 * W)), 0, s),
        L.picsong_decode_rgb_images_window(d, 1, vp(pst), ms, 0, 0, 0, 16, 16, C.byref(img(f8, pa.LAYOUT_RGB24, 48)), 0, s),
        L.picsong_encode_images(d, 1, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, 0, vp(pst), ms, s),
        L.picsong_decode_images(d, 1, vp(pst), ms, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, s),
        L.picsong_ingest_frames(d, 1, C.byref(img(f16, pa.LAYOUT_GREY16, 2 * W)), 0, r16, 0, s),
        L.picsong_emit_frames(d, 1, r16, 0, C.byref(img(f8, pa.LAYOUT_RGB24, 3 * W)), 0, s),
        L.picsong_encode_images(d, 1, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 0, 0, vp(pst), ms, s),
        L.picsong_decode_images(d, 1, vp(pst), ms, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 0, s),
        L.picsong_encode_rgb_image(d, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 1, vp(pst), ms, s),
        L.picsong_decode_rgb_image(d, vp(pst), ms, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), s),
        # the 16-bit colour layouts' alignment and size rules
        L.picsong_ingest_frames(d, 1, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W + 1)), 0, r16, 0, s),
        L.picsong_ingest_frames(d, 1, C.byref(img(f16, pa.LAYOUT_RGBA64, 8 * W - 2)), 0, r16, 0, s),
        L.picsong_emit_frames(d, 1, r16, 0, C.byref(pa.Image(data=p16 + 1, pitch=6 * W, plane_stride=0, layout=pa.LAYOUT_RGB48)), 0, s),
        L.picsong_emit_frames(d, 1, r16, 0, C.byref(img(f16, pa.LAYOUT_PLANAR3_16, 2 * W, 2 * W * H - 2)), 0, s),
        L.picsong_emit_frames(d, 2, r16, 6 * P - 2, C.byref(img(f16, pa.LAYOUT_PLANAR3_16, 2 * W, 2 * W * H)), 6 * W * H, s),
        L.picsong_encode_rgb_images(d, 22, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 6 * W * H, 0, 7, vp(pst), ms, s),
        L.picsong_encode_rgb_images(d, 1, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 0, 0, 7, vp(pst), ms - 1, s),
        L.picsong_decode_rgb_images(d, 1, vp(pst), ms, C.byref(pa.Image(data=p16 + 1, pitch=6 * W, plane_stride=0, layout=pa.LAYOUT_RGB48)), 0, s),
        # the *16 RGB frame calls' own rules
        L.picsong_encode_rgb_frames16(d, 0, r16, g16, b16, fs16, 0, 7, vp(pst), ms, s),
        L.picsong_encode_rgb_frames16(d, 22, r16, g16, b16, fs16, 0, 7, vp(pst), ms, s),
        L.picsong_decode_rgb_frames16(d, 0, vp(pst), ms, r16, g16, b16, fs16, s),
        L.picsong_decode_rgb_frames16(d, 22, vp(pst), ms, r16, g16, b16, fs16, s),
        L.picsong_encode_rgb_frames16(d, 2, r16, g16, b16, 2 * P - 2, 0, 7, vp(pst), ms, s),          # below a plane
        L.picsong_decode_rgb_frames16(d, 2, vp(pst), ms, r16, g16, b16, 2 * P - 2, s),
        L.picsong_encode_rgb_frames16(d, 2, r16, g16, b16, row16, 0, 7, vp(pst), ms, s),             # frame 1's R on frame 0's G
        L.picsong_decode_rgb_frames16(d, 2, vp(pst), ms, r16, g16, b16, row16, s),
        L.picsong_encode_rgb_frames16(d, 2, r16, g16, b16, fs16 + 1, 0, 7, vp(pst), ms, s),           # odd
        L.picsong_encode_rgb_frames16(d, 1, vp(p16 + 1), g16, b16, 0, 0, 7, vp(pst), ms, s),
        L.picsong_decode_rgb_frames16(d, 1, vp(pst), ms, r16, vp(p16 + row16 + 1), b16, 0, s),
        L.picsong_encode_rgb_frames16(d, 1, r16, g16, b16, 0, 0, 7, vp(pst), ms - 1, s),
        L.picsong_encode_rgb_frames16(d, 1, r16, None, b16, 0, 0, 7, vp(pst), ms, s),
        L.picsong_decode_rgb_frames16(d, 1, vp(pst), ms, r16, g16, None, 0, s),
        L.picsong_rgb_forward16(d, vp(p16 + 1), g16, b16, w0, w1, w2, s), L.picsong_rgb_inverse16(d, w0, w1, w2, r16, g16, vp(p16 + 1), s),
        L.picsong_rgb_forward16(d, r16, g16, b16, w0, None, w2, s),
        L.picsong_rgb_forward16(d, r16, g16, b16, w0, vp(pw + 4), w2, s), L.picsong_rgb_inverse16(d, vp(pw + 8), w1, w2, r16, g16, b16, s),
    ]
    # ... and the four new calls on every other context
    for other in (grey16.h, rgb8.h, grey8.h):
        refused += [
            L.picsong_encode_rgb_frames16(other, 1, r16, g16, b16, 0, 0, 7, vp(pst), ms, s),
            L.picsong_decode_rgb_frames16(other, 1, vp(pst), ms, r16, g16, b16, 0, s),
            L.picsong_rgb_forward16(other, r16, g16, b16, w0, w1, w2, s), L.picsong_rgb_inverse16(other, w0, w1, w2, r16, g16, b16, s),
            # ... and the 16-bit colour layouts
            L.picsong_ingest_frames(other, 1, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 0, r16, 0, s),
            L.picsong_emit_frames(other, 1, r16, 0, C.byref(img(f16, pa.LAYOUT_RGBA64, 8 * W)), 0, s),
            L.picsong_encode_rgb_images(other, 1, C.byref(img(f16, pa.LAYOUT_PLANAR3_16, 2 * W, 2 * W * H)), 0, 0, 7, vp(pst), ms, s),
            L.picsong_decode_rgb_images(other, 1, vp(pst), ms, C.byref(img(f16, pa.LAYOUT_RGB48, 6 * W)), 0, s),
        ]
    assert refused == [ERR_ARG] * len(refused), [i for i, rc in enumerate(refused) if rc != ERR_ARG]
    assert L.picsong_encode_rgb_frames16(grey8.h, 1, r16, g16, b16, 0, 0, 7, vp(pst), ms, s) == ERR_ARG
    assert b"deep RGB" in L.picsong_last_error()
    L.picsong_encode_rgb_frame(d, r8, g8, b8, 1, vp(pst), ms, s)
    assert b"picsong_encode_rgb_frames16" in L.picsong_last_error(), "the refusal names the *16 RGB calls"
    # -cp 3 in the frame calls
    cp3 = pa.Codec(W, H, wl=wl, cp=3, bit_depth=bd, is_rgb=True)
    assert L.picsong_encode_rgb_frames16(cp3.h, 1, r16, g16, b16, 0, 0, 7, vp(pst), ms, s) == ERR_ARG
    assert L.picsong_decode_rgb_frames16(cp3.h, 1, vp(pst), ms, r16, g16, b16, 0, s) == ERR_ARG
    cp3.close()
    torch.cuda.synchronize()
    assert bool((f16 == 0x1234).all()) and bool((f8 == 0x5A).all()) and bool((st == 0x5A5A).all()) and bool((work == 0x5A5A5A5A).all())
    assert bool((sse == 0).all())
    for c in (deep, grey16, rgb8, grey8):
        c.close()


def test_the_other_contexts_give_the_bytes_they_gave(pa, torch):
    """An 8-bit RGB context and a deep grey context, one case each against the reference."""
    wl, lossy = 3, False
    rgb = [orc.gen_frame(W, H, k) for k in range(3)]
    pad = [orc.pad_frame(x) for x in rgb]
    comp = orc.rgb_forward(pad[0], pad[1], pad[2], lossy)
    hdr = orc.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=8, lossy=0, qs_1e4=10000, components=3,
                          is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=0)
    want = [orc.encode_plane(comp[k], wl, lossy, 1.0, orc.lut_for_component(lossy, wl, k), hdr if k == 0 else None) for k in range(3)]
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(lossy), rgb=True)
    got = c.encode_rgb_frame(*[torch.from_numpy(p).cuda() for p in pad], header_mask=1)
    assert _same([_u16(g) for g in got], want)
    sb = torch.full((3, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    for k in range(3):
        sb[k, :want[k].size] = _dev16(torch, want[k])
    assert _same([o.cpu().numpy() for o in c.decode_rgb_frame(sb)], pad)
    c.close()
    bd, wl = 12, 5
    img, pad16, coef, sizes, stream = D.encode("saw", bd, wl, lossy)
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(lossy), bit_depth=bd)
    s = c.encode_frames16(_dev16(torch, pad16[None]))
    assert np.array_equal(_u16(s[0]), stream)
    sb = torch.full((1, c.max_stream_shorts()), -1, dtype=torch.int16, device=c.dev)
    sb[0, :stream.size] = _dev16(torch, stream)
    assert np.array_equal(_u16(c.decode_frames16(sb))[0], pad16)
    c.close()
