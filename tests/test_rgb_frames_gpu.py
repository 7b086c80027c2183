"""-m gpu: batched RGB frames through the C ABI.  picsong_encode_rgb_frames / picsong_decode_rgb_frames -- n colour frames,
ONE launch per stage over 3 n planes -- against the CPU oracle plane by plane and against n calls of the single-frame
calls; the two plane addressings, the unfused paths, the header rule, the image calls, the refusals.

Frame f's component c is oracle.gen_frame(W, H, 60 + 3 f + c) and the three tables are the shipped R / G / B files, so a
swapped frame / component index, a wrong table or a wrong plane stride shows; with n = 2 the 6 planes are no square."""
import ctypes as C
import os

import numpy as np
import pytest

import layout_ref as lr
import oracle_lib as orc

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENTINEL = 0xA5

# (W, H, wl, lossy, qs, k, pipelined hint, n, header mask)
CASES = [(320, 192, 3, False, 1.0, 0.0, False, 2, 1),        # 15 codeblocks a plane; head grid 1 x 6 tiles: launch order
         (512, 256, 3, True, 0.5, 0.0, False, 3, 7),         # head grid 1 x 8 tiles: the components re-indexed per frame
         (1000, 300, 3, False, 1.0, 0.4, True, 2, 0),        # ragged: mirror padding, two strip columns, 10 bands
         (512, 256, 4, True, 0.5, 1.5, False, 2, 7)]
IDS = ["320x192-53-n2", "512x256-97-n3", "1000x300-53-k0.4-n2", "512x256-97-k1.5-n2"]


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _stack(torch, c, streams):
    """codestreams -> int16 [len, max_stream_shorts()] rows, zero behind each stream"""
    out = torch.zeros((len(streams), c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for k, s in enumerate(streams):
        out[k, :s.numel()] = s
    return out


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request, pa, torch):
    """One context, the n frames on the device as three separate arrays, the oracle's 3 n streams and the batched call's --
    computed once per case, read by every test."""
    W, H, wl, lossy, qs, k, hint, n, mask = request.param
    frames = [[orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + c)) for c in range(3)] for f in range(n)]
    luts = [orc.lut_for_component(lossy, wl, c, k=k) for c in range(3)]
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), rgb=True, k=k, pipelined=hint)
    hdr = pa.header_pack(c.params)
    oracle = []
    for f in range(n):
        comps = orc.rgb_forward(*frames[f], lossy)
        for comp in range(3):
            with_hdr = f == 0 and (mask >> comp) & 1
            oracle.append(orc.encode_plane(comps[comp], wl, lossy, qs, luts[comp], hdr if with_hdr else None, k=k))
    rgb = [_dev(torch, np.stack([frames[f][comp] for f in range(n)])) for comp in range(3)]        # three [n, AH, AW] arrays
    got = [g.clone() for g in c.encode_rgb_frames(*rgb, first_iter=0, header_mask=mask)]
    totals = c.last_totals(3 * n)
    d = dict(W=W, H=H, wl=wl, lossy=lossy, qs=qs, k=k, n=n, mask=mask, frames=frames, luts=luts, c=c, hdr=hdr, oracle=oracle, rgb=rgb,
             got=got, totals=totals)
    yield d
    c.close()


def test_streams_equal_the_oracle_and_the_single_frame_call(case, torch):
    c, n = case["c"], case["n"]
    assert case["totals"] == [g.numel() for g in case["got"]] == [o.size for o in case["oracle"]]
    for z in range(3 * n):
        assert np.array_equal(_u16(case["got"][z]), case["oracle"][z]), f"frame {z // 3} component {z % 3} against the oracle"
    for f in range(n):
        one = c.encode_rgb_frame(*[case["rgb"][comp][f] for comp in range(3)], header_mask=case["mask"] if f == 0 else 0)
        for comp in range(3):
            assert torch.equal(one[comp], case["got"][3 * f + comp]), f"frame {f} component {comp} against encode_rgb_frame"
    # the call of n leaves the lengths where the plain calls leave theirs, on the device too
    case["c"].encode_rgb_frames(*case["rgb"], first_iter=0, header_mask=case["mask"])
    d_tot = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    assert c.L.picsong_copy_last_totals(c.h, c._stream(), 3 * n, C.c_void_p(d_tot.data_ptr())) == 0
    assert d_tot.cpu().tolist() == case["totals"]


def test_decode_equals_single_frame_calls_and_the_oracle(case, torch):
    c, n, lossy, wl, qs, k = case["c"], case["n"], case["lossy"], case["wl"], case["qs"], case["k"]
    AW, AH = c.aw, c.ah
    streams = _stack(torch, c, case["got"])
    back = c.decode_rgb_frames(streams)                       # three [n, AH, AW]
    for f in range(n):
        one = c.decode_rgb_frame(streams[3 * f:3 * f + 3])
        ob = orc.rgb_inverse(*[orc.decode_plane(_u16(case["got"][3 * f + comp]), AW, AH, wl, lossy, qs, case["luts"][comp], k=k)
                               for comp in range(3)])
        for comp in range(3):
            assert torch.equal(back[comp][f], one[comp]), f"frame {f} plane {comp} against decode_rgb_frame"
            assert np.array_equal(back[comp][f].cpu().numpy(), ob[comp].reshape(AH, AW)), f"frame {f} plane {comp} against the oracle"
            if not lossy:
                assert np.array_equal(back[comp][f].cpu().numpy(), case["frames"][f][comp])


def test_plane_addressings_and_the_unfused_head_give_the_same_streams(case, torch):
    c, n, mask = case["c"], case["n"], case["mask"]
    P = c.P
    # R, G, B back to back per frame: frame_stride = 3 P
    flat = np.concatenate([case["frames"][f][comp].ravel() for f in range(n) for comp in range(3)])
    t = _dev(torch, flat)
    got = c.encode_rgb_frames(t[0:], t[P:], t[2 * P:], n=n, frame_stride=3 * P, first_iter=0, header_mask=mask)
    for z in range(3 * n):
        assert torch.equal(got[z], case["got"][z]), f"back to back: plane {z}"
    # planes 4 bytes off their alignment: the separate colour-transform kernel, one launch a frame
    t4 = _dev(torch, np.concatenate([np.zeros(4, np.uint8), flat]))
    assert t4.data_ptr() % 16 == 0
    got = c.encode_rgb_frames(t4[4:], t4[4 + P:], t4[4 + 2 * P:], n=n, frame_stride=3 * P, first_iter=0, header_mask=mask)
    for z in range(3 * n):
        assert torch.equal(got[z], case["got"][z]), f"4 bytes off: plane {z}"


def test_output_planes_at_an_odd_address(case, torch):
    c, n = case["c"], case["n"]
    P = c.P
    streams = _stack(torch, c, case["got"])
    want = c.decode_rgb_frames(streams)
    out = torch.full((1 + 3 * n * P + 15,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    c.decode_rgb_frames(streams, outs=[out[1:], out[1 + P:], out[1 + 2 * P:]], frame_stride=3 * P)
    host = out.cpu().numpy()
    assert host[0] == SENTINEL and (host[1 + 3 * n * P:] == SENTINEL).all()
    for f in range(n):
        for comp in range(3):
            at = 1 + (3 * f + comp) * P
            assert np.array_equal(host[at:at + P], want[comp][f].cpu().numpy().ravel()), f"frame {f} plane {comp}"


def test_no_header_when_the_call_does_not_hold_frame_zero(case, torch):
    c, n = case["c"], case["n"]
    got = c.encode_rgb_frames(*case["rgb"], first_iter=5, header_mask=7)
    for z in range(3 * n):
        s = _u16(got[z])
        assert (s[:9] == 0xFFFF).all(), f"plane {z}"
        assert np.array_equal(s[9:], case["oracle"][z][9:])
    # ... and the frame that is the video's frame 0 may be any of the call's: first_iter = -(n - 1)
    got = c.encode_rgb_frames(*case["rgb"], first_iter=-(n - 1), header_mask=5)
    for z in range(3 * n):
        has = z // 3 == n - 1 and (5 >> (z % 3)) & 1
        assert np.array_equal(_u16(got[z])[:9], case["hdr"] if has else np.full(9, 0xFFFF, np.uint16)), f"plane {z}"


# ---- picsong_encode_rgb_images / picsong_decode_rgb_images ---------------------------------------------------------------
@pytest.mark.parametrize("layout", [lr.RGB24, lr.BGRA32], ids=["rgb", "bgra"])
def test_images_code_as_host_padded_planes_do(pa, torch, layout):
    W, H, wl, lossy, qs, n = 201, 137, 3, False, 1.0, 3
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), rgb=True)
    imgs = [[orc.gen_frame(W, H, 60 + 3 * f + comp) for comp in range(3)] for f in range(n)]
    pitch = W * lr.BPP[layout] + (5 if layout == lr.RGB24 else 8)               # above W * bpp: per byte / vector
    span = lr.frame_span(layout, W, H, pitch)
    fs = span + (7 if layout == lr.RGB24 else 24)                               # above a frame
    src = np.full((n - 1) * fs + span, SENTINEL, np.uint8)
    for f in range(n):
        lr.pack_into(src[f * fs:], imgs[f], layout, pitch, alpha=f)
    got = [g.clone() for g in c.encode_rgb_images(c.image(_dev(torch, src), layout, pitch), n=n, frame_stride=fs, first_iter=0, header_mask=1)]
    rgb = [_dev(torch, np.stack([orc.pad_frame(imgs[f][comp]) for f in range(n)])) for comp in range(3)]
    plain = c.encode_rgb_frames(*rgb, first_iter=0, header_mask=1)
    hdr = pa.header_pack(c.params)
    for f in range(n):
        comps = orc.rgb_forward(*[orc.pad_frame(p) for p in imgs[f]], lossy)
        for comp in range(3):
            z = 3 * f + comp
            assert torch.equal(got[z], plain[z]), f"frame {f} component {comp} against encode_rgb_frames"
            ref = orc.encode_plane(comps[comp], wl, lossy, qs, orc.lut_for_component(lossy, wl, comp), hdr if z == 0 else None)
            assert np.array_equal(_u16(got[z]), ref), f"frame {f} component {comp} against the oracle"
    # ---- decode into a sentinel-filled pitched buffer: the crop re-interleaved; the pitch gap and the tail keep the sentinel
    d_out = torch.full((src.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    c.decode_rgb_images(_stack(torch, c, got), c.image(d_out, layout, pitch), frame_stride=fs)
    want = np.full(src.size + 64, SENTINEL, np.uint8)
    for f in range(n):
        lr.pack_into(want[f * fs:], imgs[f], layout, pitch, alpha=255)           # (lossless: the crop is the input)
    assert np.array_equal(d_out.cpu().numpy(), want)
    c.close()


# ---- refusals: PICSONG_ERR_ARG, nothing launched, the outputs at their sentinel -------------------------------------------
def test_refusals_leave_the_outputs_alone(pa, torch):
    W, H, wl, n = 320, 192, 3, 2
    r = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False), rgb=True)
    g = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False))
    cp3 = pa.Codec(W, H, wl=wl, rgb=True, cp=3)
    P, ms = r.P, r.max_stream_shorts()
    planes = torch.full((3 * n * P,), SENTINEL, dtype=torch.uint8, device="cuda")
    streams = torch.full((3 * n, ms), 0x5A5A, dtype=torch.int16, device="cuda")
    buf = torch.full((n * 4 * W * H,), SENTINEL, dtype=torch.uint8, device="cuda")
    vp = C.c_void_p
    s = r._stream()
    L = r.L
    pr, pg, pb, st = planes.data_ptr(), planes.data_ptr() + P, planes.data_ptr() + 2 * P, streams.data_ptr()

    def enc(c=r, n_=n, r_=pr, g_=pg, b_=pb, fs=3 * P, st_=st, stride=ms):
        return L.picsong_encode_rgb_frames(c.h, n_, vp(r_), vp(g_), vp(b_), fs, 0, 7, vp(st_), stride, s)

    def dec(c=r, n_=n, r_=pr, g_=pg, b_=pb, fs=3 * P, st_=st, stride=ms):
        return L.picsong_decode_rgb_frames(c.h, n_, vp(st_), stride, vp(r_), vp(g_), vp(b_), fs, s)

    bad = [dict(c=g), dict(c=cp3), dict(n_=0), dict(n_=22), dict(fs=P - 1), dict(fs=P), dict(fs=3 * P - 16), dict(stride=ms - 1),
           dict(r_=None), dict(g_=None), dict(b_=None), dict(st_=None)]
    for kw in bad:
        assert enc(**kw) == ERR_ARG, ("encode", kw)
        assert dec(**kw) == ERR_ARG, ("decode", kw)

    def img(layout, pitch=None, data=True):
        i = r.image(buf, layout, 3 * W if pitch is None and layout not in lr.LAYOUTS else pitch)
        if not data:
            i.data = None
        return i

    span = lr.frame_span(lr.RGB24, W, H, 3 * W)

    def enc_i(c=r, n_=n, i=None, fs=span, st_=st, stride=ms, null_img=False):
        i = img(lr.RGB24) if i is None else i
        return L.picsong_encode_rgb_images(c.h, n_, None if null_img else C.byref(i), fs, 0, 7, vp(st_), stride, s)

    def dec_i(c=r, n_=n, i=None, fs=span, st_=st, stride=ms, null_img=False):
        i = img(lr.RGB24) if i is None else i
        return L.picsong_decode_rgb_images(c.h, n_, vp(st_), stride, None if null_img else C.byref(i), fs, s)

    bad = [dict(c=g), dict(c=cp3), dict(n_=0), dict(n_=22), dict(fs=span - 1), dict(stride=ms - 1), dict(st_=None), dict(null_img=True),
           dict(i=img(lr.RGB24, data=False)), dict(i=img(lr.GREY8), fs=W * H), dict(i=img(7)), dict(i=img(lr.RGB24, 3 * W - 1)),
           dict(i=img(lr.BGRA32, 4 * W - 1), fs=4 * W * H)]
    for k, kw in enumerate(bad):
        assert enc_i(**kw) == ERR_ARG, ("encode_rgb_images", k)
        assert dec_i(**kw) == ERR_ARG, ("decode_rgb_images", k)
    # a context without its tables refuses before anything runs
    bare = pa.Codec(W, H, wl=wl, rgb=True)
    assert enc(c=bare) == ERR_ARG and dec(c=bare) == ERR_ARG
    bare.close()
    torch.cuda.synchronize()
    assert bool((planes == SENTINEL).all()) and bool((streams == 0x5A5A).all()) and bool((buf == SENTINEL).all())
    # what is fine: the largest call's arguments pass the check (n = 21 needs its buffers: only the smallest strides here)
    assert enc(fs=3 * P) == 0 and enc(n_=1, fs=0) == 0
    torch.cuda.synchronize()
    for c in (r, g, cp3):
        c.close()
