"""-m gpu: frames as applications hold them.  picsong_ingest_frames / picsong_emit_frames against oracle_lib.pad_frame and
numpy's split / interleave (layout_ref), the whole-frame image calls against the CPU oracle's streams and decodes and
against the plain frame calls on host-padded input, and every refusal -- never against the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import layout_ref as lr
import oracle_lib as orc

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENTINEL = 0xA5
SHAPES = [(201, 137), (33, 40), (192, 128)]
IDS = [lr.NAMES[x] for x in lr.LAYOUTS]


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


def _up(v, m):
    return (v + m - 1) // m * m


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _guarded(torch, data, off=0, guard=64):
    """`data` on the device with `guard` sentinel bytes on both sides, its first byte `off` bytes behind a 16-byte boundary;
    returns (whole tensor, byte offset of the data)."""
    at = guard + off
    host = np.full(at + data.size + guard, SENTINEL, np.uint8)
    host[at:at + data.size] = data
    t = _dev(torch, host)
    assert t.data_ptr() % 16 == 0 and guard % 16 == 0
    return t, at


def _want_padded(planes):
    return np.concatenate([orc.pad_frame(p).ravel() for p in planes])


# ---- the stage seam -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", lr.LAYOUTS, ids=IDS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_ingest_and_emit_on_the_device(pa, torch, W, H, layout):
    rgb = layout != lr.GREY8
    c = pa.Codec(W, H, wl=1, rgb=rgb)                         # only the geometry is used: no table
    frame = lr.PLANES[layout] * c.P
    planes = lr.random_planes(layout, W, H, seed=W + layout)
    want = _want_padded(planes)
    row = W * lr.BPP[layout]
    # (pitch, offset of the first pixel, padded side's offset): the vector form, an unaligned pitch, an odd pointer, an
    # odd padded side
    for pitch, off, pad_off in ((row, 0, 0), (_up(row, 256), 0, 0), (row + 3, 0, 0), (_up(row, 16), 1, 0), (_up(row, 16), 0, 1)):
        ps = _up(lr.plane_span(layout, W, H, pitch), 16) + (16 if pitch % 4 == 0 else 3) if layout == lr.PLANAR3 else 0
        src = lr.pack(planes, layout, pitch, ps, alpha=0x3C, seed=pitch)
        d_src, at = _guarded(torch, src, off)
        d_pad, pat = _guarded(torch, np.full(frame, SENTINEL, np.uint8), pad_off)
        img = c.image(d_src, layout, pitch, ps, offset=at)
        assert c.L.picsong_ingest_frames(c.h, 1, C.byref(img), 0, C.c_void_p(d_pad.data_ptr() + pat), 0, c._stream()) == 0, \
            c.L.picsong_last_error()
        got = d_pad.cpu().numpy()
        assert np.array_equal(got[pat:pat + frame], want), (pitch, off, pad_off)
        assert (got[:pat] == SENTINEL).all() and (got[pat + frame:] == SENTINEL).all()
        # ---- and back: into a sentinel-filled image, from padded planes whose padding is not the mirror
        rng = np.random.default_rng(pitch)
        full = [rng.integers(0, 256, (c.ah, c.aw), dtype=np.uint8) for _ in range(lr.PLANES[layout])]
        d_full, fat = _guarded(torch, np.concatenate([p.ravel() for p in full]), pad_off)
        d_out, oat = _guarded(torch, np.full(src.size, SENTINEL, np.uint8), off)
        out_img = c.image(d_out, layout, pitch, ps, offset=oat)
        assert c.L.picsong_emit_frames(c.h, 1, C.c_void_p(d_full.data_ptr() + fat), 0, C.byref(out_img), 0, c._stream()) == 0, \
            c.L.picsong_last_error()
        want_img = lr.pack_into(np.full(src.size, SENTINEL, np.uint8), [p[:H, :W] for p in full], layout, pitch, ps, alpha=255)
        got = d_out.cpu().numpy()
        assert np.array_equal(got[oat:oat + src.size], want_img), (pitch, off, pad_off)     # pixels, alpha, untouched gaps
        assert (got[:oat] == SENTINEL).all() and (got[oat + src.size:] == SENTINEL).all()
    c.close()


@pytest.mark.parametrize("layout", [lr.GREY8, lr.RGB24, lr.BGRA32], ids=["grey", "rgb", "bgra"])
def test_ingest_and_emit_of_three_frames_through_the_binding(pa, torch, layout):
    W, H = 201, 137
    c = pa.Codec(W, H, wl=1, rgb=layout != lr.GREY8)
    pitch = _up(W * lr.BPP[layout], 4) + 4
    span = lr.frame_span(layout, W, H, pitch)
    fs = _up(span, 4) + 20
    frames = [lr.random_planes(layout, W, H, seed=f) for f in range(3)]
    src = np.full(2 * fs + span, SENTINEL, np.uint8)
    for f in range(3):
        lr.pack_into(src[f * fs:], frames[f], layout, pitch, alpha=f)
    d_src = _dev(torch, src)
    padded = c.ingest_frames(c.image(d_src, layout, pitch), n=3, frame_stride=fs)
    assert tuple(padded.shape) == (3, lr.PLANES[layout], c.ah, c.aw)
    for f in range(3):
        assert np.array_equal(padded[f].cpu().numpy().ravel(), _want_padded(frames[f])), f
    d_out = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    c.emit_frames(padded, c.image(d_out, layout, pitch), n=3, frame_stride=fs)
    want = np.full(src.size, SENTINEL, np.uint8)
    for f in range(3):
        lr.pack_into(want[f * fs:], frames[f], layout, pitch, alpha=255)
    assert np.array_equal(d_out.cpu().numpy(), want)
    c.close()


# ---- grey: picsong_encode_images / picsong_decode_images ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)], ids=["5/3", "9/7"])
def test_grey_images_code_as_host_padded_frames_do(pa, torch, lossy, qs, n):
    W, H, wl = 201, 137, 3
    lut = orc.lut_for(lossy, wl)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy))
    imgs = [orc.gen_frame(W, H, 10 + f) for f in range(n)]
    pitch = W + 3
    span = lr.frame_span(lr.GREY8, W, H, pitch)
    fs = span + 7
    src = np.full((n - 1) * fs + span, SENTINEL, np.uint8)
    for f in range(n):
        lr.pack_into(src[f * fs:], [imgs[f]], lr.GREY8, pitch)
    d_src = _dev(torch, src)
    got = c.encode_images(c.image(d_src, lr.GREY8, pitch), n=n, frame_stride=fs)
    got = [g.clone() for g in got]
    # ... the oracle's streams of the frames (frame 0 carries the header), and the plain call on host-padded input
    plain = c.encode_frames(_dev(torch, np.stack([orc.pad_frame(i).ravel() for i in imgs])))
    for f in range(n):
        ref = orc.encode_frame(imgs[f], wl, lossy, qs, lut, iter_=f)
        assert np.array_equal(_u16(got[f]), ref), f
        assert torch.equal(got[f], plain[f]), f
    # ---- decode into a sentinel-filled pitched buffer: the oracle's decode, cropped; nothing else written
    streams = torch.zeros((n, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for f in range(n):
        streams[f, :got[f].numel()] = got[f]
    d_out = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    c.decode_images(streams, c.image(d_out, lr.GREY8, pitch), frame_stride=fs)
    want = np.full(src.size, SENTINEL, np.uint8)
    for f in range(n):
        dec = orc.decode_frame(_u16(got[f]), W, H, wl, lossy, qs, lut)
        if not lossy:
            assert np.array_equal(dec, imgs[f])
        lr.pack_into(want[f * fs:], [dec], lr.GREY8, pitch)
    assert np.array_equal(d_out.cpu().numpy(), want)
    c.close()


# ---- colour: picsong_encode_rgb_image / picsong_decode_rgb_image --------------------------------------------------------
@pytest.fixture(scope="module")
def rgb_case():
    """The oracle's three component streams of one RGB frame, computed once."""
    W, H, wl, lossy, qs = 201, 137, 3, False, 1.0
    planes = [orc.gen_frame(W, H, 60 + k) for k in range(3)]
    comps = orc.rgb_forward(*[orc.pad_frame(p) for p in planes], lossy)
    return dict(W=W, H=H, wl=wl, lossy=lossy, qs=qs, planes=planes, comps=comps)


@pytest.mark.parametrize("layout", [lr.RGB24, lr.BGRA32, lr.PLANAR3], ids=["rgb", "bgra", "planar"])
def test_rgb_image_codes_as_the_oracle_codes_its_planes(pa, torch, rgb_case, layout):
    k = rgb_case
    W, H, wl, lossy, qs = k["W"], k["H"], k["wl"], k["lossy"], k["qs"]
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), rgb=True)
    hdr = pa.header_pack(c.params)
    # RGB24: an unaligned pitch, the per-byte form; the others the vector one
    pitch = {lr.RGB24: 3 * W + 1, lr.BGRA32: 4 * W + 4, lr.PLANAR3: _up(W, 16)}[layout]
    ps = _up(lr.plane_span(layout, W, H, pitch), 16) + 32 if layout == lr.PLANAR3 else 0
    d_src = _dev(torch, lr.pack(k["planes"], layout, pitch, ps, alpha=7))
    got = [g.clone() for g in c.encode_rgb_image(c.image(d_src, layout, pitch, ps), header_mask=1)]
    plain = c.encode_rgb_frame(*[_dev(torch, orc.pad_frame(p)) for p in k["planes"]], header_mask=1)
    for comp in range(3):
        ref = orc.encode_plane(k["comps"][comp], wl, lossy, qs, orc.lut_for_component(lossy, wl, comp), hdr if comp == 0 else None)
        assert np.array_equal(_u16(got[comp]), ref), comp
        assert torch.equal(got[comp], plain[comp]), comp
    # ---- decode into RGBA32: the oracle's planes interleaved, alpha 255, the gaps and the tail untouched
    streams = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for comp in range(3):
        streams[comp, :got[comp].numel()] = got[comp]
    opitch = W * 4 + 12
    span = lr.frame_span(lr.RGBA32, W, H, opitch)
    d_out = torch.full((span + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    c.decode_rgb_image(streams, c.image(d_out, lr.RGBA32, opitch))
    AW, AH = c.aw, c.ah
    back = orc.rgb_inverse(*[orc.decode_plane(_u16(got[comp]), AW, AH, wl, lossy, qs, orc.lut_for_component(lossy, wl, comp))
                             for comp in range(3)])
    crop = [b.reshape(AH, AW)[:H, :W] for b in back]
    for comp in range(3):
        assert np.array_equal(crop[comp], k["planes"][comp])               # (lossless)
    want = lr.pack_into(np.full(span + 64, SENTINEL, np.uint8), crop, lr.RGBA32, opitch, alpha=255)
    assert np.array_equal(d_out.cpu().numpy(), want)
    c.close()


# ---- refusals: PICSONG_ERR_ARG, outputs at their sentinel ----------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(pa, torch):
    W, H, wl = 201, 137, 3
    g = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False))
    r = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False), rgb=True)
    P, ms = g.P, g.max_stream_shorts()
    buf = torch.full((4 * W * H * 3,), SENTINEL, dtype=torch.uint8, device="cuda")          # image side, read or written
    pad = torch.full((3 * 3 * P,), SENTINEL, dtype=torch.uint8, device="cuda")
    streams = torch.full((3, ms), 0x5A5A, dtype=torch.int16, device="cuda")
    s = g._stream()
    vp = C.c_void_p

    def img(layout, pitch=None, ps=0, data=True):
        i = g.image(buf, layout, 3 * W if pitch is None and layout not in lr.LAYOUTS else pitch, ps)
        if not data:
            i.data = None
        return i

    def ingest(c, i, n=1, fs=0, out=pad, pstride=0):
        return c.L.picsong_ingest_frames(c.h, n, C.byref(i) if i is not None else None, fs, vp(out.data_ptr()) if out is not None else None,
                                         pstride, s)

    def emit(c, i, n=1, fs=0, src=pad, pstride=0):
        return c.L.picsong_emit_frames(c.h, n, vp(src.data_ptr()) if src is not None else None, pstride, C.byref(i) if i is not None else None,
                                       fs, s)

    span24 = lr.frame_span(lr.RGB24, W, H, 3 * W)
    plane = lr.plane_span(lr.PLANAR3, W, H, W)
    bad = [
        lambda f, c: f(c, None),                                                   # null image
        lambda f, c: f(c, img(lr.RGB24, data=False)),                              # null data
        lambda f, c: f(c, img(lr.RGB24), 1, 0, None),                              # null padded side
        lambda f, c: f(c, img(6)), lambda f, c: f(c, img(-1)),                     # unknown layout
        lambda f, c: f(c, img(lr.RGB24, 3 * W - 1)),                               # pitch < W * bpp
        lambda f, c: f(c, img(lr.GREY8, W - 1)),
        lambda f, c: f(c, img(lr.RGBA32, 4 * W - 1)),
        lambda f, c: f(c, img(lr.PLANAR3, W, plane - 1)),                          # plane_stride too small
        lambda f, c: f(c, img(lr.RGB24), 2, span24 - 1, pad, 3 * P),               # frame_stride too small
        lambda f, c: f(c, img(lr.RGB24), 2, span24, pad, 3 * P - 1),               # padded_stride too small
        lambda f, c: f(c, img(lr.RGB24), 0), lambda f, c: f(c, img(lr.RGB24), 65, span24, pad, 3 * P),   # n outside 1..64
    ]
    for k, call in enumerate(bad):
        for f in (ingest, emit):
            for c in (g, r):
                assert call(f, c) == ERR_ARG, (k, f.__name__)
    # what is fine: one frame looks at no stride; two frames at their smallest strides
    assert ingest(g, img(lr.RGB24), 1, 0, pad, 0) == 0 and ingest(g, img(lr.PLANAR3, W, plane)) == 0
    assert ingest(g, img(lr.RGB24), 2, span24, pad, 3 * P) == 0
    torch.cuda.synchronize()
    pad.fill_(SENTINEL)
    # ---- the whole-frame calls: the layout against the context, and the plain calls' own checks
    L = g.L
    st = vp(streams.data_ptr())
    whole = [
        L.picsong_encode_images(g.h, 1, C.byref(img(lr.RGB24)), 0, 0, st, ms, s),              # a colour layout on a grey context
        L.picsong_encode_images(g.h, 1, C.byref(img(lr.PLANAR3, W, plane)), 0, 0, st, ms, s),
        L.picsong_decode_images(g.h, 1, st, ms, C.byref(img(lr.BGRA32)), 0, s),
        L.picsong_encode_rgb_image(r.h, C.byref(img(lr.GREY8)), 1, st, ms, s),                 # GREY8 on an RGB context
        L.picsong_decode_rgb_image(r.h, st, ms, C.byref(img(lr.GREY8)), s),
        L.picsong_encode_images(r.h, 1, C.byref(img(lr.GREY8)), 0, 0, st, ms, s),              # the grey calls on an RGB context
        L.picsong_encode_rgb_image(g.h, C.byref(img(lr.RGB24)), 1, st, ms, s),                 # ... and the RGB calls on a grey one
        L.picsong_decode_rgb_image(g.h, st, ms, C.byref(img(lr.RGB24)), s),
        L.picsong_encode_images(g.h, 1, None, 0, 0, st, ms, s),                                # null pointers
        L.picsong_encode_images(g.h, 1, C.byref(img(lr.GREY8)), 0, 0, None, ms, s),
        L.picsong_encode_images(g.h, 1, C.byref(img(lr.GREY8, data=False)), 0, 0, st, ms, s),
        L.picsong_decode_images(g.h, 1, None, ms, C.byref(img(lr.GREY8)), 0, s),
        L.picsong_encode_rgb_image(r.h, None, 1, st, ms, s),
        L.picsong_decode_rgb_image(r.h, st, ms, None, s),
        L.picsong_encode_images(g.h, 1, C.byref(img(7)), 0, 0, st, ms, s),                     # unknown layout
        L.picsong_encode_images(g.h, 1, C.byref(img(lr.GREY8, W - 1)), 0, 0, st, ms, s),       # pitch
        L.picsong_decode_rgb_image(r.h, st, ms, C.byref(img(lr.RGBA32, 4 * W - 1)), s),
        L.picsong_encode_rgb_image(r.h, C.byref(img(lr.PLANAR3, W, plane - 1)), 1, st, ms, s),   # plane_stride
        L.picsong_encode_images(g.h, 2, C.byref(img(lr.GREY8)), plane - 1, 0, st, ms, s),      # frame_stride
        L.picsong_decode_images(g.h, 2, st, ms, C.byref(img(lr.GREY8)), plane - 1, s),
        L.picsong_encode_images(g.h, 0, C.byref(img(lr.GREY8)), plane, 0, st, ms, s),          # n
        L.picsong_encode_images(g.h, 65, C.byref(img(lr.GREY8)), plane, 0, st, ms, s),
        L.picsong_encode_images(g.h, 2, C.byref(img(lr.GREY8)), plane, 0, st, ms - 1, s),      # the plain call's stream stride
        L.picsong_encode_rgb_image(r.h, C.byref(img(lr.RGB24)), 1, st, ms - 1, s),
    ]
    assert whole == [ERR_ARG] * len(whole), whole
    # a context without its table refuses before anything runs
    bare = pa.Codec(W, H, wl=wl)
    assert L.picsong_encode_images(bare.h, 1, C.byref(img(lr.GREY8)), 0, 0, st, ms, s) == ERR_ARG
    bare.close()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((pad == SENTINEL).all()) and bool((streams == 0x5A5A).all())
    # the frame too small to be mirror-padded (AW - W > W) never becomes a context: the rule is picsong_pad_frame_host's
    with pytest.raises(pa.PicsongError):
        pa.Codec(31, 40, wl=1)
    g.close()
    r.close()
