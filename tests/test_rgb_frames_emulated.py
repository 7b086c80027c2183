"""Batched RGB frames on the CPU wave emulator (tests/hipemu/emu_rgb_frames_driver.cpp): the launch sequences of
picsong_encode_rgb_frames / picsong_decode_rgb_frames -- every stage ONE launch over 3 n planes, plane z component z % 3 of
frame z / 3, component c coding with table c -- against the oracle plane by plane and against the same sequences on one
frame; the pack's header mask; the separate-kernel path; the argument checks.

Frame f's component c is oracle.gen_frame(W, H, 60 + 3 f + c) and the three tables are the shipped R / G / B files (they
differ), so a swapped frame / component index, a wrong table or a wrong plane stride shows as a mismatch; n = 2 makes the
6 planes no square, so a transposed z / 3 <-> z % 3 cannot pass."""
import ctypes as C
import functools

import numpy as np
import pytest

import emu_lib as E
import layout_ref as lr
import oracle_lib as orc
from emu_lib import _geo, _p, driver_lib

_lib = None
ULL = C.c_ulonglong
SENTINEL = 0xA5
HEADER = np.arange(0x1101, 0x110A, dtype=np.uint16)         # nine shorts no stream holds by accident


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_rgb_frames.so", ("emu_rgb_frames_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
    return _lib


def _max_stream(AW, AH):
    return 9 + 2 * (AW // 64) * (AH // 64) + AW * AH + 1


@functools.lru_cache(maxsize=None)
def _frames(W, H, n):
    """[n][3] padded planes: frame f's component c from seed 60 + 3 f + c"""
    return tuple(tuple(orc.pad_frame(orc.gen_frame(W, H, 60 + 3 * f + c)) for c in range(3)) for f in range(n))


@functools.lru_cache(maxsize=None)
def _luts(lossy, wl, k):
    return tuple(orc.lut_for_component(lossy, wl, c, k=k) for c in range(3))


@functools.lru_cache(maxsize=None)
def _oracle_planes(W, H, wl, lossy, qs, k, n):
    """per plane z = 3 f + c: (coefficients as the coder reads them, staging, sizes) of the oracle, table c"""
    out = []
    for f in range(n):
        comps = orc.rgb_forward(*_frames(W, H, n)[f], lossy)
        for c in range(3):
            AH, AW = comps[c].shape
            coef = orc.dwt_forward(comps[c], wl, qs)[:AW * AH].reshape(AH, AW)
            st, sz = orc.bpc_encode(coef, wl, _luts(lossy, wl, k)[c], k=k)
            out.append((np.trunc(coef).astype(np.int32), st, sz))
    return out


def _planes_buffer(frames, back_to_back, offset=0):
    """The n frames' planes in one 64-byte aligned buffer (+ offset): three arrays of n planes (frame_stride = P), or R, G, B
    back to back per frame (frame_stride = 3 P).  Returns (buffer, [r, g, b] views of frame 0, frame_stride)."""
    n = len(frames)
    P = frames[0][0].size
    buf = E.aligned_zeros(3 * n * P + offset, np.uint8)[offset:]
    for f in range(n):
        for c in range(3):
            at = (3 * f + c) * P if back_to_back else (c * n + f) * P
            buf[at:at + P] = frames[f][c].ravel()
    starts = [c * P for c in range(3)] if back_to_back else [c * n * P for c in range(3)]
    return buf, [buf[s:] for s in starts], (3 * P if back_to_back else P)


def _encode(W, H, wl, lossy, qs, k, n, first_iter=0, mask=7, fuse=1, stages=3, back_to_back=True, offset=0, frames=None):
    frames = frames if frames is not None else _frames(W, H, n)
    AH, AW = frames[0][0].shape
    P, ncb, extra = AW * AH, (AW // 64) * (AH // 64), orc.dwt_extra(AW, AH, wl)
    luts = _luts(lossy, wl, k)
    buf, rgb, fs = _planes_buffer(frames, back_to_back, offset)
    stride = _max_stream(AW, AH)
    streams = np.full(3 * n * stride, 0x7E7E, np.uint16)
    totals = np.zeros(3 * n, np.int32)
    coef = E.aligned_zeros(3 * n * (P + extra), np.int32)
    st16 = np.zeros(3 * n * P, np.uint16)
    sizes = np.zeros(3 * n * ncb, np.int32)
    flag = np.zeros(1, np.int32)
    tabs = [np.ascontiguousarray(t.table, np.int32) for t in luts]
    rc = lib().emu_rgbf_encode(1, 2, n, _p(rgb[0]), _p(rgb[1]), _p(rgb[2]), ULL(fs), first_iter, mask, _p(streams), ULL(stride), AW, AH, wl,
                               int(lossy), C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])), C.c_float(k),
                               int(luts[0].n_tables), _p(HEADER), fuse, stages, _p(totals), _p(coef), _p(st16), _p(sizes), _p(flag))
    assert rc >= 0 and flag[0] == 0
    return dict(rc=rc, streams=streams.reshape(3 * n, stride), totals=totals, coef=coef.reshape(3 * n, P + extra),
                st16=st16.reshape(3 * n, P), sizes=sizes.reshape(3 * n, ncb), AW=AW, AH=AH)


def _coef_of(res, z):
    """plane z's coefficients as the coder reads them"""
    assert res["rc"] & 2, "16-bit coefficients"
    return E.mallat16(res["coef"][z], res["AW"], res["AH"]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _encoded(W, H, wl, lossy, qs, k, n):
    return _encode(W, H, wl, lossy, qs, k, n)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
@pytest.mark.parametrize("W,H", [(320, 192), (512, 256)])
def test_forward_sequence_over_3n_planes(W, H, lossy, qs, n):
    """rgb_forward_transform with n: the fused head with grid.z = 3 n (320x192: 6 tiles, launch order; 512x256: 8 tiles, the
    three components of a tile re-indexed 8 apart within each frame), the levels above it over 3 n planes -- every plane's
    coefficients equal the oracle's colour transform + transform and those of the same sequence on that frame alone."""
    wl = 3
    res = _encode(W, H, wl, lossy, qs, 0.0, n, stages=1)
    assert res["rc"] == 3, "the fused 16-bit head ran"
    want = _oracle_planes(W, H, wl, lossy, qs, 0.0, n)
    for f in range(n):
        one = _encode(W, H, wl, lossy, qs, 0.0, 1, stages=1, frames=(_frames(W, H, n)[f],))
        assert one["rc"] == 3
        for c in range(3):
            got = _coef_of(res, 3 * f + c)
            assert np.array_equal(got, want[3 * f + c][0]), f"frame {f} component {c} against the oracle"
            assert np.array_equal(got, _coef_of(one, c)), f"frame {f} component {c} against the single-frame sequence"


CODED = [(320, 192, False, 1.0, 0.0, 2), (320, 192, True, 0.5, 0.0, 3), (512, 256, False, 1.0, 0.0, 3), (320, 192, False, 1.0, 0.6, 2),
         (320, 192, True, 0.5, 0.6, 2)]


@pytest.mark.parametrize("W,H,lossy,qs,k,n", CODED)
def test_encoder_launch_over_3n_planes(W, H, lossy, qs, k, n):
    """ONE coder launch over 3 n planes, plane z with table z % 3 (k = 0: four-wave workgroups, 15 codeblocks a plane leave
    the last one of every plane half empty; -k 0.6: the BULK instantiation): staging and sizes of every plane are the
    oracle's with table c, and the packed streams are oracle.encode_plane's."""
    wl = 3
    res = _encoded(W, H, wl, lossy, qs, k, n)
    want = _oracle_planes(W, H, wl, lossy, qs, k, n)
    for z in range(3 * n):
        _, st, sz = want[z]
        assert np.array_equal(res["sizes"][z], sz), f"plane {z}: sizes"
        for cb in range(sz.size):
            assert np.array_equal(res["st16"][z][cb * 4096:cb * 4096 + sz[cb]], (st[cb * 4096:cb * 4096 + sz[cb]] & 0xFFFF).astype(np.uint16)), \
                f"plane {z} codeblock {cb}"
        hdr = HEADER if z < 3 else None                      # (first_iter 0, mask 7)
        ref = orc.bitstream_pack(st, sz, hdr)
        assert res["totals"][z] == ref.size
        assert np.array_equal(res["streams"][z][:ref.size], ref), f"plane {z}: stream"
        comps = orc.rgb_forward(*_frames(W, H, n)[z // 3], lossy)
        assert np.array_equal(ref, orc.encode_plane(comps[z % 3], wl, lossy, qs, _luts(lossy, wl, k)[z % 3], hdr, k=k))


@pytest.mark.parametrize("first_iter,mask", [(0, 1), (0, 7), (0, 0), (1, 7), (-1, 5), (-2, 7), (5, 7)])
def test_pack_header_mask(first_iter, mask):
    """The populated header on exactly the masked components of the frame with first_iter + f == 0, 0xFFFF elsewhere --
    and nothing else of any stream depends on where it lands."""
    W, H, wl, n = 320, 192, 3, 2
    base = _encoded(W, H, wl, False, 1.0, 0.0, n)
    res = _encode(W, H, wl, False, 1.0, 0.0, n, first_iter=first_iter, mask=mask)
    for z in range(3 * n):
        t = res["totals"][z]
        assert t == base["totals"][z]
        has = (z // 3) + first_iter == 0 and (mask >> (z % 3)) & 1
        assert np.array_equal(res["streams"][z][:9], HEADER if has else np.full(9, 0xFFFF, np.uint16)), f"plane {z}"
        assert np.array_equal(res["streams"][z][9:t], base["streams"][z][9:t])
        assert (res["streams"][z][t:] == 0x7E7E).all()


def test_single_frame_pack_is_unchanged():
    """n = 1: the header argument of a lone RGB frame names its three planes as before (base 0)."""
    W, H, wl = 320, 192, 3
    for mask in (0, 1, 2, 7):
        res = _encode(W, H, wl, False, 1.0, 0.0, 1, mask=mask)
        for c in range(3):
            has = (mask >> c) & 1
            assert np.array_equal(res["streams"][c][:9], HEADER if has else np.full(9, 0xFFFF, np.uint16))


def _decode(res, W, H, wl, lossy, qs, k, n, fuse=1, offset=0, back_to_back=True):
    AW, AH = res["AW"], res["AH"]
    P = AW * AH
    luts = _luts(lossy, wl, k)
    tabs = [np.ascontiguousarray(t.table, np.int32) for t in luts]
    buf = E.aligned_zeros(3 * n * P + 64, np.uint8)
    buf[:] = SENTINEL
    out = buf[offset:offset + 3 * n * P]
    starts = [c * P for c in range(3)] if back_to_back else [c * n * P for c in range(3)]
    fs = 3 * P if back_to_back else P
    flag = np.zeros(1, np.int32)
    streams = np.ascontiguousarray(res["streams"])
    rc = lib().emu_rgbf_decode(1, 2, n, _p(streams), ULL(streams.shape[1]), _p(out[starts[0]:]), _p(out[starts[1]:]), _p(out[starts[2]:]),
                               ULL(fs), AW, AH, wl, int(lossy), C.c_float(qs), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])),
                               C.c_float(k), int(luts[0].n_tables), fuse, _p(flag))
    assert rc >= 0 and flag[0] == 0
    assert (buf[:offset] == SENTINEL).all() and (buf[offset + 3 * n * P:] == SENTINEL).all()
    planes = [[out[((3 * f + c) if back_to_back else (c * n + f)) * P:][:P].reshape(AH, AW) for c in range(3)] for f in range(n)]
    return rc, planes


def _oracle_decode(res, wl, lossy, qs, k, n):
    AW, AH = res["AW"], res["AH"]
    out = []
    for f in range(n):
        comps = [orc.decode_plane(res["streams"][3 * f + c][:res["totals"][3 * f + c]], AW, AH, wl, lossy, qs, _luts(lossy, wl, k)[c], k=k)
                 for c in range(3)]
        out.append(orc.rgb_inverse(*comps))
    return out


@pytest.mark.parametrize("W,H,lossy,qs,k,n", CODED)
def test_decoder_launch_and_fused_tails(W, H, lossy, qs, k, n):
    """stream_intake over 3 n streams, ONE decoder launch (plane z with table z % 3), the levels above the finest over 3 n
    planes, the fused tail with grid.z = frame (5/3: dwt_inv_rgb_kernel, 9/7: dwt_inv97_rgb_kernel) -- the oracle's decode
    through its inverse colour transform, and for 5/3 the input."""
    wl = 3
    res = _encoded(W, H, wl, lossy, qs, k, n)
    rc, planes = _decode(res, W, H, wl, lossy, qs, k, n, back_to_back=(n == 2))
    assert rc == 3, "a fused tail over 16-bit coefficients ran"
    want = _oracle_decode(res, wl, lossy, qs, k, n)
    for f in range(n):
        for c in range(3):
            assert np.array_equal(planes[f][c], want[f][c]), f"frame {f} plane {c}"
            if not lossy:
                assert np.array_equal(planes[f][c], _frames(W, H, n)[f][c])


def test_97_tail_replay_takes_its_workgroup_only(monkeypatch):
    """The 9/7 tail's second pass with true divisions (every workgroup through it: PICSONG_DWT_EXACT_REPLAY=1) gives the
    same planes with a frame axis."""
    W, H, wl, n = 320, 192, 3, 3
    res = _encoded(W, H, wl, True, 0.5, 0.0, n)
    _, planes = _decode(res, W, H, wl, True, 0.5, 0.0, n)
    monkeypatch.setenv("PICSONG_DWT_EXACT_REPLAY", "1")
    rc, again = _decode(res, W, H, wl, True, 0.5, 0.0, n)
    assert rc == 3
    for f in range(n):
        for c in range(3):
            assert np.array_equal(planes[f][c], again[f][c])


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_separate_kernel_path(lossy, qs):
    """Unfused (the caller's switch, or planes off their alignment): the separate colour transform, one launch a frame, and
    the levels of all 3 n planes -- the same streams; the separate inverse transform, one launch a frame, the same planes
    (also at an odd address)."""
    W, H, wl, n = 320, 192, 3, 2
    base = _encoded(W, H, wl, lossy, qs, 0.0, n)
    for kw in (dict(fuse=0), dict(offset=4), dict(fuse=0, back_to_back=False)):
        res = _encode(W, H, wl, lossy, qs, 0.0, n, **kw)
        assert not res["rc"] & 1, "the separate colour-transform kernel ran"
        assert np.array_equal(res["totals"], base["totals"])
        for z in range(3 * n):
            assert np.array_equal(res["streams"][z], base["streams"][z]), f"plane {z}"
    _, want = _decode(base, W, H, wl, lossy, qs, 0.0, n)
    for kw in (dict(fuse=0), dict(offset=1), dict(fuse=0, back_to_back=False)):
        rc, planes = _decode(base, W, H, wl, lossy, qs, 0.0, n, **kw)
        assert not rc & 1, "the separate inverse colour transform ran"
        for f in range(n):
            for c in range(3):
                assert np.array_equal(planes[f][c], want[f][c]), f"frame {f} plane {c}"


# ---- the argument checks ----
def _refusal(**kw):
    AW, AH = 320, 192
    P = AW * AH
    a = dict(ctx_rgb=1, cp=2, same=1, n=2, r=4096, g=4096 + P, b=4096 + 2 * P, streams=1 << 30, frame_stride=3 * P,
             stream_stride=_max_stream(AW, AH))
    a.update(kw)
    msg = C.create_string_buffer(256)
    rc = lib().emu_rgbf_refusal(a["ctx_rgb"], a["cp"], a["same"], a["n"], C.c_void_p(a["r"]), C.c_void_p(a["g"]), C.c_void_p(a["b"]),
                                C.c_void_p(a["streams"]), ULL(a["frame_stride"]), ULL(a["stream_stride"]), AW, AH, msg, len(msg))
    return msg.value.decode() if rc else None


def test_refusals():
    AW, AH = 320, 192
    P = AW * AH
    assert _refusal() is None
    for name in ("r", "g", "b", "streams"):
        assert "null" in _refusal(**{name: 0})
    assert "not an RGB" in _refusal(ctx_rgb=0)
    assert "-cp 3" in _refusal(cp=3)
    for n in (0, -1, 22):
        assert "n outside" in _refusal(n=n)
    assert _refusal(n=21) is None and _refusal(n=1, frame_stride=0) is None
    assert "stream stride" in _refusal(stream_stride=_max_stream(AW, AH) - 1)
    assert "geometry" in _refusal(same=0)
    # strides: below a padded plane; back-to-back planes whose frames are less than three planes apart overlap the next
    # frame's; three separate arrays take any stride from a plane on
    assert "frame_stride" in _refusal(frame_stride=P - 1)
    assert "overlap" in _refusal(frame_stride=P) and "overlap" in _refusal(frame_stride=3 * P - 1)
    far = dict(r=1 << 24, g=2 << 24, b=3 << 24)
    assert _refusal(frame_stride=P, n=21, **far) is None
    assert "overlap" in _refusal(frame_stride=1 << 23, n=3, **far)       # frame 2 of R lands on frame 0 of G
    assert _refusal(frame_stride=1 << 23, n=2, **far) is None


def _images_refusal(**kw):
    W, H, AW, AH = 300, 180, 320, 192
    a = dict(layout=lr.RGB24, data=4096, pitch=3 * W, plane_stride=0, frame_stride=3 * W * H, n=2)
    a.update(kw)
    msg = C.create_string_buffer(256)
    rc = lib().emu_rgbf_images_refusal(a["layout"], C.c_void_p(a["data"]), ULL(a["pitch"]), ULL(a["plane_stride"]), ULL(a["frame_stride"]),
                                       a["n"], W, H, AW, AH, msg, len(msg))
    return msg.value.decode() if rc else None


def test_image_refusals():
    W, H = 300, 180
    assert _images_refusal() is None
    assert "grey" in _images_refusal(layout=lr.GREY8, pitch=W, frame_stride=W * H)
    assert "null" in _images_refusal(data=0)
    assert "layout" in _images_refusal(layout=9)
    assert "pitch" in _images_refusal(pitch=3 * W - 1)
    assert "frame_stride" in _images_refusal(frame_stride=3 * W * H - 1)
    assert "plane_stride" in _images_refusal(layout=lr.PLANAR3, pitch=W, plane_stride=W * H - 1)
    for n in (0, 22, 64):
        assert "n outside" in _images_refusal(n=n)
    assert _images_refusal(n=21) is None


def test_refused_calls_run_nothing():
    W, H, wl, n = 320, 192, 3, 2
    frames = _frames(W, H, n)
    AH, AW = frames[0][0].shape
    P = AW * AH
    luts = _luts(False, wl, 0.0)
    tabs = [np.ascontiguousarray(t.table, np.int32) for t in luts]
    buf, rgb, fs = _planes_buffer(frames, True)
    stride = _max_stream(AW, AH)
    streams = np.full(3 * n * stride, 0x7E7E, np.uint16)
    totals = np.full(3 * n, -7, np.int32)
    flag = np.zeros(1, np.int32)
    lib().emu_rgbf_reset()

    def enc(ctx_rgb=1, cp=2, n_=n, fs_=fs, stride_=stride, r=rgb[0]):
        return lib().emu_rgbf_encode(ctx_rgb, cp, n_, _p(r) if r is not None else None, _p(rgb[1]), _p(rgb[2]), ULL(fs_), 0, 7, _p(streams),
                                     ULL(stride_), AW, AH, wl, 0, C.c_float(1.0), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])),
                                     C.c_float(0.0), 1, _p(HEADER), 1, 3, _p(totals), None, None, None, _p(flag))

    for kw in (dict(ctx_rgb=0), dict(cp=3), dict(n_=0), dict(n_=22), dict(fs_=P - 1), dict(fs_=P), dict(stride_=stride - 1), dict(r=None)):
        assert enc(**kw) == -1, kw
    assert lib().emu_rgbf_launches() == 0
    assert (streams == 0x7E7E).all() and (totals == -7).all()

    out = np.full(3 * n * P, SENTINEL, np.uint8)

    def dec(ctx_rgb=1, cp=2, n_=n, fs_=3 * P, stride_=stride, s=streams):
        return lib().emu_rgbf_decode(ctx_rgb, cp, n_, _p(s) if s is not None else None, ULL(stride_), _p(out), _p(out[P:]), _p(out[2 * P:]),
                                     ULL(fs_), AW, AH, wl, 0, C.c_float(1.0), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])),
                                     C.c_float(0.0), 1, 1, _p(flag))

    for kw in (dict(ctx_rgb=0), dict(cp=3), dict(n_=0), dict(n_=22), dict(fs_=P - 1), dict(fs_=2 * P), dict(stride_=stride - 1), dict(s=None)):
        assert dec(**kw) == -1, kw
    assert lib().emu_rgbf_launches() == 0
    assert (out == SENTINEL).all()
    # ... and an accepted call counts its launches: the head, wl - 2 levels, the coder, scan and pack
    assert enc() >= 0 and lib().emu_rgbf_launches() == 1 + (wl - 2) + 1 + 2
