"""-m gpu: colour proxies through the C ABI.  picsong_decode_rgb_frames_reduced / _window and picsong_decode_rgb_images_reduced /
_window -- n RGB frames at 1/2^r, or a window of them, ONE launch per stage over 3 n planes -- against the CPU oracle and
against n calls of the single-frame calls; every colour layout at an aligned and an odd destination with sentinels around
every written byte; the unfused tail; the refusals.

Ground truth is the oracle: frame f's component c is oracle.gen_frame(W, H, 60 + 3 f + c), coded by the oracle with the
shipped R / G / B tables; the expected planes at level r are reduced_ref.reduced_rgb's, a window is its crop, a layout is
layout_ref.pack of the crop."""
import ctypes as C
import os

import numpy as np
import pytest

import layout_ref as lr
import oracle_lib as orc
import reduced_ref as rr
import window_ref as wr

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENTINEL = 0xA5
COLOUR = (lr.PLANAR3, lr.RGB24, lr.BGR24, lr.RGBA32, lr.BGRA32)

# (W, H, wl, lossy, qs, k, n)
CASES = [(320, 192, 3, False, 1.0, 0.0, 2),         # 5 x 3 codeblocks a plane; odd rectangles at r = 1, 2
         (1000, 300, 3, True, 0.5, 0.0, 3),         # ragged; rw x rh = 250 x 75 at r = 2: odd rows, widths no multiple of 4
         (512, 256, 4, True, 1.0, 1.5, 2),
         (128, 64, 2, False, 1.0, 0.0, 21)]         # 63 planes, one codeblock a plane at r = 1
IDS = ["320x192-53-n2", "1000x300-97-n3", "512x256-97-k1.5-n2", "128x64-53-n21"]


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


class Case:
    """One context, the oracle's 3 n streams on the device, the oracle's planes at every level (made on first use)"""

    def __init__(self, pa, torch, W, H, wl, lossy, qs, k, n):
        self.W, self.H, self.wl, self.lossy, self.qs, self.k, self.n = W, H, wl, lossy, qs, k, n
        self.torch = torch
        self.luts = [orc.lut_for_component(lossy, wl, c, k=k) for c in range(3)]
        self.c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(lossy), rgb=True, k=k)
        self.AW, self.AH = self.c.aw, self.c.ah
        self.host = []
        for f in range(n):
            comps = orc.rgb_forward(*[orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + c)) for c in range(3)], lossy)
            self.host += [orc.encode_plane(comps[c], wl, lossy, qs, self.luts[c], None, k=k) for c in range(3)]
        ms = self.c.max_stream_shorts()
        flat = np.zeros((3 * n, ms), np.uint16)
        for z, s in enumerate(self.host):
            flat[z, :s.size] = s
        self.streams = torch.from_numpy(flat.view(np.int16)).cuda()
        # another set of streams for the same context: the frames in another order (every component keeps its table)
        self.other = torch.roll(self.streams, 3, 0).contiguous()
        self._want = {}

    def want(self, r):
        """[f][c]: the oracle's plane of frame f at 1/2^r, (AH >> r, AW >> r) uint8"""
        if r not in self._want:
            self._want[r] = [[np.asarray(p, np.uint8).reshape(self.AH >> r, self.AW >> r)
                              for p in rr.reduced_rgb(self.host[3 * f:3 * f + 3], self.AW, self.AH, self.wl, self.lossy, self.qs, self.luts,
                                                      r, self.k)] for f in range(self.n)]
        return self._want[r]

    def windows(self, r):
        paw, pah = self.AW >> r, self.AH >> r
        out = [(0, 0, paw, pah), (1, 2, min(33, paw - 1), min(21, pah - 2)), (paw - 5, pah - 3, 5, 3)]
        if paw >= 130:
            out.append((60, 1, 70, min(40, pah - 1)))         # crosses a 64-sample tile edge, wider than a tile
        return out


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request, pa, torch):
    d = Case(pa, torch, *request.param)
    yield d
    d.c.close()


def test_reduced_frames_equal_the_oracle_and_the_single_frame_call(case, torch):
    c, n = case.c, case.n
    for r in range(case.wl):
        got = c.decode_rgb_frames_reduced(case.streams, r)             # three [n, AH >> r, AW >> r]
        want = case.want(r)
        for f in range(n):
            one = c.decode_rgb_frame_reduced(case.streams[3 * f:3 * f + 3], r)
            for comp in range(3):
                assert torch.equal(got[comp][f], one[comp]), f"r {r} frame {f} plane {comp} against decode_rgb_frame_reduced"
                assert np.array_equal(got[comp][f].cpu().numpy(), want[f][comp]), f"r {r} frame {f} plane {comp} against the oracle"
    full = c.decode_rgb_frames(case.streams)
    got = c.decode_rgb_frames_reduced(case.streams, 0)
    for comp in range(3):
        assert torch.equal(got[comp], full[comp]), "reduce = 0 is decode_rgb_frames"
    assert c.range_flag() == 0


def test_reduced_frames_write_nothing_else_and_take_any_alignment(case, torch):
    """R, G, B back to back per frame with a gap between frames: aligned (the fused tail where the plan has it) and one byte
    off (the separate inverse colour transform); the sentinel survives around every plane."""
    c, n, r = case.c, case.n, 1
    pp = (case.AW >> r) * (case.AH >> r)
    want = case.want(r)
    for offset, gap in [(0, 4), (1, 3)]:
        fs = 3 * pp + gap
        out = torch.full((offset + n * fs + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0
        c.decode_rgb_frames_reduced(case.streams, r, outs=[out[offset:], out[offset + pp:], out[offset + 2 * pp:]], frame_stride=fs)
        expect = np.full(out.numel(), SENTINEL, np.uint8)
        for f in range(n):
            for comp in range(3):
                at = offset + f * fs + comp * pp
                expect[at:at + pp] = want[f][comp].ravel()
        assert np.array_equal(out.cpu().numpy(), expect), (offset, gap)


def test_unfused_tail_gives_the_same_planes(case, torch, monkeypatch):
    c = case.c
    for r in range(case.wl):
        fused = [g.clone() for g in c.decode_rgb_frames_reduced(case.streams, r)]
        monkeypatch.setenv("PICSONG_RGB_NOFUSE", "1")
        plain = c.decode_rgb_frames_reduced(case.streams, r)
        monkeypatch.delenv("PICSONG_RGB_NOFUSE")
        for comp in range(3):
            assert torch.equal(fused[comp], plain[comp]), f"r {r} plane {comp}"


def test_window_frames_equal_the_oracles_crop_and_the_single_frame_call(case, torch):
    c, n = case.c, case.n
    for r in range(case.wl):
        want = case.want(r)
        for (x, y, w, h) in case.windows(r):
            assert c.window_codeblocks(x, y, w, h, r) == len(wr.window_codeblocks(case.AW, case.AH, case.wl, case.lossy, r, x, y, w, h))
            c.decode_rgb_frames_window(case.other, x, y, w, h, r)        # other coefficients in the buffers: stale ones would show
            got = c.decode_rgb_frames_window(case.streams, x, y, w, h, r)                      # three [n, h, w]
            for f in range(n if n <= 3 else 2):
                one = c.decode_rgb_frame_window(case.streams[3 * f:3 * f + 3], x, y, w, h, r)
                for comp in range(3):
                    assert torch.equal(got[comp][f], one[comp]), f"r {r} window {(x, y, w, h)} frame {f} plane {comp} against the single-frame call"
            for f in range(n):
                for comp in range(3):
                    assert np.array_equal(got[comp][f].cpu().numpy(), want[f][comp][y:y + h, x:x + w]), \
                        f"r {r} window {(x, y, w, h)} frame {f} plane {comp} against the oracle"
    assert c.range_flag() == 0


def test_window_frames_at_a_pitch_write_only_the_window(case, torch):
    """the three planes row-pitched at an odd address, a gap between frames: the pitch gap, the space between the frames
    and the bytes behind the last row keep the sentinel"""
    c, n, r = case.c, case.n, 1
    x, y, w, h = case.windows(r)[1]
    for offset, pitch, gap in [(1, w + 6, 5), (0, (w + 3) // 4 * 4 + 4, 4)]:
        span = (h - 1) * pitch + w
        ps = span + (3 if offset else (-span) % 4)
        fs = 3 * ps + gap
        out = torch.full((offset + n * fs + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        planes = [torch.as_strided(out, (n, h, w), (fs, pitch, 1), offset + comp * ps) for comp in range(3)]
        c.decode_rgb_frames_window(case.other, x, y, w, h, r)
        c.decode_rgb_frames_window(case.streams, x, y, w, h, r, outs=planes)
        expect = np.full(out.numel(), SENTINEL, np.uint8)
        for f in range(n):
            for comp in range(3):
                rows = np.lib.stride_tricks.as_strided(expect[offset + f * fs + comp * ps:], (h, w), (pitch, 1))
                rows[...] = case.want(r)[f][comp][y:y + h, x:x + w]
        assert np.array_equal(out.cpu().numpy(), expect), (offset, pitch, gap)


def _image_buffer(torch, layout, w, h, n, aligned):
    """(buffer, offset, pitch, plane_stride, frame_stride, a frame's span): pitch = w * bpp + 7 at an odd base, or a 16-byte
    aligned pitch at an aligned base"""
    bpp = lr.BPP[layout]
    offset = 0 if aligned else 1
    pitch = (w * bpp + 15) // 16 * 16 + 16 if aligned else w * bpp + 7
    plane = lr.plane_span(layout, w, h, pitch)
    ps = 0 if layout != lr.PLANAR3 else (plane + 15) // 16 * 16 if aligned else plane + 5
    span = lr.frame_span(layout, w, h, pitch, ps)
    fs = (span + 15) // 16 * 16 + 16 if aligned else span + 9
    buf = torch.full((offset + n * fs + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, offset, pitch, ps, fs, span


def _image_expect(size, planes_of, layout, n, offset, pitch, ps, fs, span):
    expect = np.full(size, SENTINEL, np.uint8)
    for f in range(n):
        at = offset + f * fs
        expect[at:at + span] = lr.pack(planes_of(f), layout, pitch, ps, alpha=255, fill=SENTINEL)
    return expect


@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
@pytest.mark.parametrize("layout", COLOUR, ids=[lr.NAMES[l] for l in COLOUR])
def test_image_calls_write_the_layout_and_nothing_else(case, torch, layout, aligned):
    """every byte of the destination: the oracle's crop packed by layout_ref (alpha 255) and the 0xA5 sentinel in every pitch
    gap, behind the last row and between the frames"""
    c, n = case.c, case.n
    r = 1
    x, y, w, h = case.windows(r)[1]
    buf, offset, pitch, ps, fs, span = _image_buffer(torch, layout, w, h, n, aligned)
    c.decode_rgb_frames_window(case.other, x, y, w, h, r)
    c.decode_rgb_images_window(case.streams, x, y, w, h, c.image(buf, layout, pitch, ps, offset), r=r, frame_stride=fs)
    want = case.want(r)
    expect = _image_expect(buf.numel(), lambda f: [p[y:y + h, x:x + w] for p in want[f]], layout, n, offset, pitch, ps, fs, span)
    assert np.array_equal(buf.cpu().numpy(), expect), "images_window"
    # ---- the reduced image call: the visible rw x rh pixels, = the window (0, 0, rw, rh)
    r = case.wl - 1
    rw, rh = c.reduced_dims(r)[:2]
    want = case.want(r)
    buf, offset, pitch, ps, fs, span = _image_buffer(torch, layout, rw, rh, n, aligned)
    c.decode_rgb_images_reduced(case.streams, r, c.image(buf, layout, pitch, ps, offset), frame_stride=fs)
    expect = _image_expect(buf.numel(), lambda f: [p[:rh, :rw] for p in want[f]], layout, n, offset, pitch, ps, fs, span)
    assert np.array_equal(buf.cpu().numpy(), expect), "images_reduced"
    other = torch.full_like(buf, SENTINEL)
    c.decode_rgb_images_window(case.streams, 0, 0, rw, rh, c.image(other, layout, pitch, ps, offset), r=r, frame_stride=fs)
    assert torch.equal(buf, other), "images_reduced against images_window (0, 0, rw, rh)"
    assert c.range_flag() == 0


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)], ids=["53", "97"])
def test_reduced_images_on_rows_emit_cannot_group(pa, torch, lossy, qs):
    """320 x 192, wl 4, r = 3: the reduced rows are 40 bytes, no multiple of 16, so picsong_decode_rgb_images_reduced takes the
    window (0, 0, rw, rh) instead of the reduced sequence + emit; r = 2 (80 bytes) takes the latter.  The same checks."""
    d = Case(pa, torch, 320, 192, 4, lossy, qs, 0.0, 2)
    c, n = d.c, d.n
    for r in (3, 2):
        rw, rh = c.reduced_dims(r)[:2]
        want = d.want(r)
        for layout in COLOUR:
            for aligned in (False, True):
                buf, offset, pitch, ps, fs, span = _image_buffer(torch, layout, rw, rh, n, aligned)
                c.decode_rgb_images_reduced(d.streams, r, c.image(buf, layout, pitch, ps, offset), frame_stride=fs)
                expect = _image_expect(buf.numel(), lambda f: [p[:rh, :rw] for p in want[f]], layout, n, offset, pitch, ps, fs, span)
                assert np.array_equal(buf.cpu().numpy(), expect), (r, layout, aligned)
    assert c.range_flag() == 0
    c.close()


# ---- refusals: PICSONG_ERR_ARG, nothing launched, the outputs at their sentinel -------------------------------------------
def test_refusals_leave_the_outputs_alone(pa, torch):
    W, H, wl, n, red = 320, 192, 3, 2, 1
    r = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False), rgb=True)
    g = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(False))
    cp3 = pa.Codec(W, H, wl=wl, rgb=True, cp=3)
    bare = pa.Codec(W, H, wl=wl, rgb=True)
    ms = r.max_stream_shorts()
    pp = (r.aw >> red) * (r.ah >> red)
    planes = torch.full((3 * n * pp,), SENTINEL, dtype=torch.uint8, device="cuda")
    streams = torch.full((3 * n, ms), 0x5A5A, dtype=torch.int16, device="cuda")
    vp = C.c_void_p
    s = r._stream()
    L = r.L
    pr, st = planes.data_ptr(), streams.data_ptr()
    x, y, w, h, pitch = 1, 2, 33, 21, 40
    span = (h - 1) * pitch + w

    def reduced(c=r, n_=n, null=None, fs=3 * pp, st_=st, stride=ms, reduce=red):
        p = [pr, pr + pp, pr + 2 * pp]
        if null is not None:
            p[null] = None
        return L.picsong_decode_rgb_frames_reduced(c.h, n_, vp(st_), stride, reduce, vp(p[0]), vp(p[1]), vp(p[2]), fs, s)

    for kw in [dict(c=g), dict(c=cp3), dict(c=bare), dict(n_=0), dict(n_=22), dict(null=0), dict(null=1), dict(null=2), dict(st_=None),
               dict(stride=ms - 1), dict(reduce=-1), dict(reduce=wl), dict(fs=pp - 1), dict(fs=pp), dict(fs=3 * pp - 16)]:
        assert reduced(**kw) == ERR_ARG, ("frames_reduced", kw)

    def window(c=r, n_=n, null=None, fs=3 * span, st_=st, stride=ms, reduce=red, x_=x, y_=y, w_=w, h_=h, pitch_=pitch):
        p = [pr, pr + span, pr + 2 * span]
        if null is not None:
            p[null] = None
        return L.picsong_decode_rgb_frames_window(c.h, n_, vp(st_), stride, reduce, x_, y_, w_, h_, vp(p[0]), vp(p[1]), vp(p[2]), pitch_, fs, s)

    paw, pah = r.aw >> red, r.ah >> red
    for kw in [dict(c=g), dict(c=cp3), dict(c=bare), dict(n_=0), dict(n_=22), dict(null=0), dict(null=1), dict(null=2), dict(st_=None),
               dict(stride=ms - 1), dict(reduce=-1), dict(reduce=wl), dict(w_=0), dict(h_=0), dict(x_=-1), dict(y_=-1), dict(x_=paw - w + 1),
               dict(y_=pah - h + 1), dict(pitch_=w - 1), dict(fs=span - 1), dict(fs=span), dict(fs=3 * span - 8)]:
        assert window(**kw) == ERR_ARG, ("frames_window", kw)

    def img(layout=lr.RGB24, pitch_=None, ps=0, data=True):
        i = r.image(planes, layout, (3 * w if layout not in lr.BPP else w * lr.BPP[layout]) if pitch_ is None else pitch_, ps)
        if not data:
            i.data = None
        return i

    ispan = lr.frame_span(lr.RGB24, w, h, 3 * w)

    def images_window(c=r, n_=n, i=None, fs=ispan, st_=st, stride=ms, reduce=red, x_=x, y_=y, w_=w, h_=h, null_img=False):
        i = img() if i is None else i
        return L.picsong_decode_rgb_images_window(c.h, n_, vp(st_), stride, reduce, x_, y_, w_, h_, None if null_img else C.byref(i), fs, s)

    rw, rh = r.reduced_dims(red)[:2]
    rspan = lr.frame_span(lr.RGB24, rw, rh, 3 * rw)
    small = torch.full((n * rspan,), SENTINEL, dtype=torch.uint8, device="cuda")

    def images_reduced(c=r, n_=n, i=None, fs=rspan, st_=st, stride=ms, reduce=red, null_img=False):
        i = r.image(small, lr.RGB24, 3 * rw) if i is None else i
        return L.picsong_decode_rgb_images_reduced(c.h, n_, vp(st_), stride, reduce, None if null_img else C.byref(i), fs, s)

    common = [dict(c=g), dict(c=cp3), dict(c=bare), dict(n_=0), dict(n_=22), dict(st_=None), dict(null_img=True), dict(stride=ms - 1),
              dict(reduce=-1), dict(reduce=wl), dict(i=img(data=False)), dict(i=img(lr.GREY8)), dict(i=img(7))]
    for k, kw in enumerate(common + [dict(w_=0), dict(x_=paw - w + 1), dict(i=img(lr.RGB24, 3 * w - 1)), dict(i=img(lr.BGRA32, 4 * w - 1), fs=4 * w * h),
                                     dict(i=img(lr.PLANAR3, w, (h - 1) * w + w - 1), fs=3 * w * h), dict(fs=ispan - 1)]):
        assert images_window(**kw) == ERR_ARG, ("images_window", k)
    for k, kw in enumerate(common + [dict(i=r.image(small, lr.RGB24, 3 * rw - 1)), dict(fs=rspan - 1),
                                     dict(i=r.image(small, lr.PLANAR3, rw, rw * rh - 1), fs=3 * rw * rh)]):
        assert images_reduced(**kw) == ERR_ARG, ("images_reduced", k)
    torch.cuda.synchronize()
    assert bool((planes == SENTINEL).all()) and bool((streams == 0x5A5A).all()) and bool((small == SENTINEL).all())
    for c in (r, g, cp3, bare):
        c.close()
