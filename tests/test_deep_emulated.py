"""Deep contexts (bit_depth 9..16, uint16 samples) on the CPU wave emulator (tests/hipemu/emu_deep_driver.cpp): the
library's own plans, selectors and launch sequences over the kernel sources, against deep_ref -- the oracle's stage
functions between a numpy level shift and a numpy clamp.  Every comparison is bit for bit / byte for byte."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import deep_ref as D
import drop_ref as dr
import emu_lib as E
import oracle_lib as orc
from emu_lib import _geo, _p, driver_lib

_lib = None
ULL = C.c_ulonglong
SENT = 0xA5C3


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_deep.so", ("emu_deep_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
        _lib.emu_deep_level_shift_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
        _lib.emu_deep_level_shift_inv.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    return _lib


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def frames_buffer(frames, gap=0, off=0):
    """n padded uint16 frames laid frame_stride = 2 P + gap bytes apart, the first `off` bytes behind a 64-byte boundary,
    gaps (and the bytes before and after) filled with the sentinel.  Returns (whole buffer u16, view at frame 0, stride)."""
    n, P = len(frames), frames[0].size
    stride = 2 * P + gap
    assert off % 2 == 0 and gap % 2 == 0
    raw = E.aligned_zeros((off + (n - 1) * stride + 2 * P) // 2 + 32, np.uint16)
    raw[:] = SENT
    for f, x in enumerate(frames):
        o = (off + f * stride) // 2
        raw[o:o + P] = x.ravel()
    return raw, raw[off // 2:], stride


def forward(frames, bd, wl, lossy, qs=1.0, gap=0, off=0):
    """emu_deep_forward over n frames; returns (list of (AH, AW) Mallat arrays, bits)."""
    ah, aw = frames[0].shape
    P, extra = aw * ah, orc.dwt_extra(aw, ah, wl)
    raw, view, stride = frames_buffer(frames, gap, off)
    before = raw.copy()
    coef = E.aligned_zeros(len(frames) * (P + extra), np.float32 if lossy else np.int32)
    bits = lib().emu_deep_forward(_p(view), ULL(stride), len(frames), _p(coef), aw, ah, wl, int(lossy), C.c_float(qs), bd)
    assert bits >= 0
    assert np.array_equal(raw, before), "the input is read only"
    return [coef[f * (P + extra):f * (P + extra) + P].reshape(ah, aw) for f in range(len(frames))], bits


def inverse(coefs, bd, wl, lossy, qs=1.0, gap=0, off=0):
    """emu_deep_inverse over n int32 Mallat arrays; returns (list of uint16 (AH, AW), fused flag); the sentinel around and
    between the frames must survive."""
    ah, aw = coefs[0].shape
    P = aw * ah
    n = len(coefs)
    cin = E.aligned_copy(np.concatenate([np.ascontiguousarray(c, np.int32).ravel() for c in coefs]))
    raw, view, stride = frames_buffer([np.full((ah, aw), SENT, np.uint16)] * n, gap, off)
    fused = lib().emu_deep_inverse(_p(cin), _p(view), ULL(stride), n, aw, ah, wl, int(lossy), C.c_float(qs), bd)
    assert fused >= 0
    outs = []
    mask = np.ones(raw.size, bool)
    for f in range(n):
        o = (off + f * stride) // 2
        outs.append(raw[o:o + P].reshape(ah, aw).copy())
        mask[o:o + P] = False
    assert (raw[mask] == SENT).all(), "a byte outside the frames' 2 P bytes was written"
    return outs, bool(fused)


def padded_input(kind, bd, wl):
    return D.mirror_pad(D.inputs(kind, bd, wl))


FWD_CASES = [(lossy, qs, bd, wl) for lossy, qs in ((False, 1.0), (True, 1.0), (True, 0.25)) for bd in (9, 12, 16) for wl in (2, 5)]


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("lossy,qs,bd,wl", FWD_CASES)
def test_forward_transform_of_uint16_frames(lossy, qs, bd, wl):
    pad = padded_input("saw" if bd < 16 else "noise", bd, wl).copy()
    if bd == 16:
        pad[0, 0], pad[0, 1], pad[5, 7], pad[-1, -1] = 0, 65535, 65535, 0       # the unsigned read: 65535 is never -1
    want = D.forward(pad, bd, wl, lossy, qs)[:pad.size].reshape(pad.shape)
    got, bits = forward([pad], bd, wl, lossy, qs)
    assert bits == 3 and _same(got[0], want)


@pytest.mark.parametrize("lossy,qs,bd,wl", [(False, 1.0, 12, 5), (True, 0.25, 16, 2), (True, 1.0, 9, 5)])
def test_forward_transform_variations(lossy, qs, bd, wl):
    pads = [padded_input(k, bd, wl) for k in ("saw", "noise", "smooth")]
    wants = [D.forward(p, bd, wl, lossy, qs)[:p.size].reshape(p.shape) for p in pads]
    # the pointer 2 bytes off a 16-byte boundary: level 0's per-column form
    got, bits = forward(pads[:1], bd, wl, lossy, qs, off=2)
    assert bits == 1 and _same(got[0], wants[0])
    with env(PICSONG_DEEP_NOFUSE=1):
        for off in (0, 2):
            got, bits = forward(pads[:1], bd, wl, lossy, qs, off=off)
            assert bits == 0 and _same(got[0], wants[0])
    for bands in ("32,16,8", "8,8,8"):
        with env(PICSONG_DWT_BANDS=bands):
            for off in (0, 2):
                got, bits = forward(pads[:1], bd, wl, lossy, qs, off=off)
                assert bits == (3 if off == 0 else 1) and _same(got[0], wants[0]), bands
    # three frames with gaps: a 16-byte multiple keeps the vector form, another even gap takes the per-column one
    for gap, bit in ((48, 3), (6, 1)):
        got, bits = forward(pads, bd, wl, lossy, qs, gap=gap)
        assert bits == bit
        for f in range(3):
            assert _same(got[f], wants[f]), (gap, f)
    with env(PICSONG_DEEP_NOFUSE=1):
        got, bits = forward(pads, bd, wl, lossy, qs, gap=6)
        assert bits == 0 and all(_same(got[f], wants[f]) for f in range(3))


def clamp_coefficients(bd, wl, lossy, qs):
    """Coded coefficients of `noise` (samples over the whole range), scaled by 5/4 about the mid level so that the decoded
    samples pass both clamp ends and hit 2^bd - 1 exactly.  (No coder here: their magnitudes may pass 2^15.)"""
    pad = padded_input("noise", bd, wl)
    c = np.trunc(D.forward(pad, bd, wl, lossy, qs)[:pad.size]).astype(np.int64).reshape(pad.shape)
    return np.clip(c * 5 // 4, -(1 << 20), 1 << 20).astype(np.int32)


@pytest.mark.parametrize("lossy,qs,bd,wl", FWD_CASES)
def test_inverse_transform_to_uint16_samples(lossy, qs, bd, wl):
    mx = (1 << bd) - 1
    pad = padded_input("saw", bd, wl)
    coef = np.trunc(D.forward(pad, bd, wl, lossy, qs)[:pad.size]).astype(np.int32).reshape(pad.shape)
    for c in (coef, clamp_coefficients(bd, wl, lossy, qs)):
        want = D.inverse(c, bd, wl, lossy, qs)
        got, fused = inverse([c], bd, wl, lossy, qs)
        assert fused and np.array_equal(got[0], want)
    assert want.min() == 0 and want.max() == mx, "the scaled array passes both clamp ends"
    if not lossy:
        assert np.array_equal(D.inverse(coef, bd, wl, lossy), pad), "5/3 is exact"


@pytest.mark.parametrize("lossy,qs,bd,wl", [(False, 1.0, 12, 5), (True, 0.25, 16, 2), (True, 1.0, 9, 5)])
def test_inverse_transform_variations(lossy, qs, bd, wl):
    coefs = [clamp_coefficients(bd, wl, lossy, qs)]
    for kind in ("noise", "smooth"):
        p = padded_input(kind, bd, wl)
        coefs.append(np.trunc(D.forward(p, bd, wl, lossy, qs)[:p.size]).astype(np.int32).reshape(p.shape))
    wants = [D.inverse(c, bd, wl, lossy, qs) for c in coefs]
    got, fused = inverse(coefs[:1], bd, wl, lossy, qs, off=2)          # the separate clamp pass, per sample
    assert not fused and np.array_equal(got[0], wants[0])
    got, fused = inverse(coefs[:1], bd, wl, lossy, qs, off=8)          # ... its 8-byte form
    assert not fused and np.array_equal(got[0], wants[0])
    with env(PICSONG_DEEP_NOFUSE=1):
        got, fused = inverse(coefs[:1], bd, wl, lossy, qs)
        assert not fused and np.array_equal(got[0], wants[0])
    for bands in ("32,16,8", "8,8,8"):
        with env(PICSONG_DWT_BANDS=bands):
            got, fused = inverse(coefs[:1], bd, wl, lossy, qs)
            assert fused and np.array_equal(got[0], wants[0]), bands
    if lossy:
        with env(PICSONG_DWT_EXACTDIV=1):                              # the dividing kernels
            got, fused = inverse(coefs[:1], bd, wl, lossy, qs)
            assert fused and np.array_equal(got[0], wants[0])
    for gap, f_want in ((48, True), (6, False)):
        got, fused = inverse(coefs, bd, wl, lossy, qs, gap=gap)
        assert fused == f_want
        for f in range(3):
            assert np.array_equal(got[f], wants[f]), (gap, f)


def test_element_wise_ends():
    rng = np.random.default_rng(1)
    for bd in (9, 16):
        off, mx = 1 << (bd - 1), (1 << bd) - 1
        v = rng.integers(0, mx + 1, 4096).astype(np.uint16)
        v[:4] = (0, mx, mx, 0)
        for lossy in (False, True):
            for o in (0, 1):
                src = E.aligned_zeros(4096 + 8, np.uint16)[o:o + 4096]
                src[:] = v
                out = E.aligned_zeros(4096, np.float32 if lossy else np.int32)
                assert lib().emu_deep_level_shift_fwd(_p(src), _p(out), 1024, int(lossy), bd) == 0
                assert _same(out, D.level_shift(v, bd, lossy))
            x = (rng.integers(-3 * off, 3 * off, 4096)).astype(np.float32 if lossy else np.int32)
            if lossy:
                x += np.float32(0.49)
                x[7] = np.nan
            y = x.copy()
            assert lib().emu_deep_level_shift_inv(_p(y), y.size, int(lossy), bd) == 0
            assert np.array_equal(y.astype(np.uint16), D.clamp(x, bd))


# ---- frame sequences -----------------------------------------------------------------------------------------------------
def encode(frames, bd, wl, lossy, qs, k=0.0, first_iter=0, gap=0, off=0):
    ah, aw = frames[0].shape
    n = len(frames)
    lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
    tab = np.ascontiguousarray(lut.table, np.int32)
    stride = 9 + 2 * (aw // 64) * (ah // 64) + aw * ah + 1
    streams = np.full(n * stride, 0x7777, np.uint16)
    totals = np.zeros(n, np.int32)
    flag = np.zeros(1, np.int32)
    raw, view, fs = frames_buffer(frames, gap, off)
    hdr = D.header(D.W, D.H, bd, wl, lossy, qs, k)
    bits = lib().emu_deep_encode(_p(view), ULL(fs), n, first_iter, _p(streams), ULL(stride), _p(totals), aw, ah, wl, int(lossy),
                                 C.c_float(qs), bd, _p(tab), _p(_geo(lut)), C.c_float(k), int(getattr(lut, "n_tables", 1)), _p(hdr), _p(flag))
    assert bits >= 0
    return [streams[f * stride:f * stride + totals[f]].copy() for f in range(n)], int(flag[0]), bits


def decode(streams, bd, wl, lossy, qs, k=0.0, drop=0, gap=0, off=0):
    ah, aw = D.AH, D.AW
    n = len(streams)
    lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
    tab = np.ascontiguousarray(lut.table, np.int32)
    stride = 9 + 2 * (aw // 64) * (ah // 64) + aw * ah + 1
    sbuf = np.full(n * stride, 0xFFFF, np.uint16)
    for f, s in enumerate(streams):
        sbuf[f * stride:f * stride + s.size] = s
    flag = np.zeros(1, np.int32)
    raw, view, fs = frames_buffer([np.full((ah, aw), SENT, np.uint16)] * n, gap, off)
    bits = lib().emu_deep_decode(_p(sbuf), ULL(stride), n, _p(view), ULL(fs), aw, ah, wl, int(lossy), C.c_float(qs), bd, _p(tab),
                                 _p(_geo(lut)), C.c_float(k), int(getattr(lut, "n_tables", 1)), drop, _p(flag))
    assert bits >= 0 and not bits & 8
    outs, mask = [], np.ones(raw.size, bool)
    for f in range(n):
        o = (off + f * fs) // 2
        outs.append(raw[o:o + aw * ah].reshape(ah, aw).copy())
        mask[o:o + aw * ah] = False
    assert (raw[mask] == SENT).all()
    return outs, int(flag[0]), bits


@pytest.mark.parametrize("lossy,bd,kind,wl,qs,raw", D.IN_RANGE, ids=[f"{'97' if c[0] else '53'}-{c[1]}-{c[2]}" for c in D.IN_RANGE])
def test_frame_sequences_match_the_composed_reference(lossy, bd, kind, wl, qs, raw):
    img, pad, coef, sizes, stream0 = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, raw)
    stream1 = D.encode(kind, bd, wl, lossy, qs, with_header=False)[4]
    assert (stream1[:9] == 0xFFFF).all() and np.array_equal(stream1[9:], stream0[9:])
    got, flag, bits = encode([pad, pad], bd, wl, lossy, qs)
    assert flag == 0 and bits == 3
    assert np.array_equal(got[0], stream0) and np.array_equal(got[1], stream1)
    want = D.decode(stream0, bd, wl, lossy, qs)
    dec, flag, bits = decode(got, bd, wl, lossy, qs)
    assert flag == 0 and bits & 1
    assert np.array_equal(dec[0], want) and np.array_equal(dec[1], want)
    if not lossy:
        assert np.array_equal(dec[0], pad), "the 5/3 round trip is exact"


def test_frame_sequences_on_the_other_routes():
    lossy, bd, kind, wl, qs, raw = D.IN_RANGE[6]            # 9/7, 12-bit saw
    img, pad, coef, sizes, stream0 = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, raw)
    want = D.decode(stream0, bd, wl, lossy, qs)
    for nofuse in (None, 1):
        with env(PICSONG_DEEP_NOFUSE=nofuse):
            got, flag, bits = encode([pad], bd, wl, lossy, qs, off=2)
            assert flag == 0 and bits == (0 if nofuse else 1) and np.array_equal(got[0], stream0)
            dec, flag, bits = decode(got, bd, wl, lossy, qs, off=2)
            assert flag == 0 and not bits & 1 and np.array_equal(dec[0], want)
    # first_iter = -1: the header on the call's second frame
    got, flag, _ = encode([pad, pad], bd, wl, lossy, qs, first_iter=-1)
    assert np.array_equal(got[1], stream0) and (got[0][:9] == 0xFFFF).all() and np.array_equal(got[0][9:], stream0[9:])


def test_complexity_scalable_mode():
    lossy, bd, kind, wl, qs = False, 12, "saw", 5, 1.0
    img, pad, coef, sizes, stream = D.encode(kind, bd, wl, lossy, qs, k=0.5)
    assert D.max_coef(coef) < 32768
    got, flag, _ = encode([pad], bd, wl, lossy, qs, k=0.5)
    assert flag == 0 and np.array_equal(got[0], stream)
    dec, flag, _ = decode(got, bd, wl, lossy, qs, k=0.5)
    assert flag == 0 and np.array_equal(dec[0], D.decode(stream, bd, wl, lossy, qs, k=0.5)) and np.array_equal(dec[0], pad)


def test_decode_drop_on_a_deep_context():
    lossy, bd, kind, wl, qs = True, 12, "smooth", 3, 1.0
    img, pad, coef, sizes, stream = D.encode(kind, bd, wl, lossy, qs)
    D.check_precondition(coef, sizes, 0)
    c = dr.drop_coefficients(stream, D.AW, D.AH, wl, orc.lut_for(lossy, wl), 2)
    want = D.inverse(c, bd, wl, lossy, qs)
    dec, flag, _ = decode([stream], bd, wl, lossy, qs, drop=2)
    assert flag == 0 and np.array_equal(dec[0], want)
    assert not np.array_equal(want, D.decode(stream, bd, wl, lossy, qs)), "drop = 2 changes the picture"


@pytest.mark.parametrize("lossy,bd,kind,wl,qs", D.OUT_OF_RANGE)
def test_out_of_range_frames_raise_the_range_flag(lossy, bd, kind, wl, qs):
    pad = padded_input(kind, bd, wl)
    assert D.max_coef(D.forward(pad, bd, wl, lossy, qs)[:pad.size]) >= 32768
    _, flag, _ = encode([pad], bd, wl, lossy, qs)
    assert flag != 0


# ---- GREY16 layouts ------------------------------------------------------------------------------------------------------
SHAPES = [(201, 137), (33, 40), (192, 128), (700, 500)]


def _up(v, m):
    return (v + m - 1) // m * m


def _at_offset(data_u8, off):
    raw = E.aligned_zeros(off + data_u8.size, np.uint8)
    raw[off:] = data_u8
    return raw[off:]


def _pack16(frames, pitch, fs, rng):
    """n (H, W) uint16 frames at `pitch`, fs bytes apart, in a buffer that ends with the last addressed byte."""
    h, w = frames[0].shape
    span = (h - 1) * pitch + 2 * w
    buf = rng.integers(0, 256, (len(frames) - 1) * fs + span, dtype=np.uint8)
    for f, x in enumerate(frames):
        for y in range(h):
            o = f * fs + y * pitch
            buf[o:o + 2 * w] = x[y].view(np.uint8)
    return buf


@pytest.mark.parametrize("W,H", SHAPES)
def test_grey16_ingest_and_emit(W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    P = AW * AH
    rng = np.random.default_rng(W)
    msg = C.create_string_buffer(256)
    for n in (1, 2):
        frames = [rng.integers(0, 65536, (H, W)).astype(np.uint16) for _ in range(n)]
        wants = [D.mirror_pad(x, AW, AH) for x in frames]
        for pitch in (2 * W, 2 * W + 2, _up(2 * W, 256)):
            span = (H - 1) * pitch + 2 * W
            fs = _up(span, 4) + 8 if pitch % 4 == 0 else span + 6
            for off in (0, 2):
                src = _at_offset(_pack16(frames, pitch, fs, rng), off)
                pad_stride = 2 * P + 64
                raw = E.aligned_zeros(((n - 1) * pad_stride + 2 * P) // 2 + 32, np.uint16)
                raw[:] = SENT
                vec = lib().emu_deep_ingest(_p(src), ULL(pitch), ULL(fs), _p(raw), ULL(pad_stride), n, W, H, AW, AH, msg, 256)
                assert vec >= 0, msg.value
                assert bool(vec) == (off == 0 and pitch % 4 == 0), (pitch, off)
                for f in range(n):
                    o = f * pad_stride // 2
                    assert np.array_equal(raw[o:o + P].reshape(AH, AW), wants[f]), (pitch, off, f)
                    assert (raw[o + P:o + pad_stride // 2][:32] == SENT).all()
                # emit: padded planes whose padding is NOT the mirror -- it must crop -- into a sentinel-filled buffer
                full = [rng.integers(0, 65536, (AH, AW)).astype(np.uint16) for _ in range(n)]
                padded = E.aligned_zeros(n * pad_stride // 2, np.uint16)
                for f in range(n):
                    padded[f * pad_stride // 2:f * pad_stride // 2 + P] = full[f].ravel()
                out = _at_offset(np.full((n - 1) * fs + span, 0xA5, np.uint8), off)
                vec = lib().emu_deep_emit(_p(padded), ULL(pad_stride), _p(out), ULL(pitch), ULL(fs), n, W, H, AW, AH, msg, 256)
                assert vec >= 0 and bool(vec) == (off == 0 and pitch % 4 == 0)
                want = np.full(out.size, 0xA5, np.uint8)
                for f in range(n):
                    for y in range(H):
                        want[f * fs + y * pitch:f * fs + y * pitch + 2 * W] = full[f][y, :W].view(np.uint8)
                assert np.array_equal(out, want), (pitch, off)
    # the padded side off its 16-byte boundary: the per-sample form, the same samples
    src = _at_offset(_pack16(frames[:1], 2 * W, 0, rng), 0)
    raw = E.aligned_zeros(P + 16, np.uint16)
    raw[:] = SENT
    assert lib().emu_deep_ingest(_p(src), ULL(2 * W), ULL(0), _p(raw[1:]), ULL(0), 1, W, H, AW, AH, msg, 256) == 0
    assert np.array_equal(raw[1:1 + P].reshape(AH, AW), wants[0]) and raw[0] == SENT and (raw[1 + P:] == SENT).all()


def test_grey16_refusals():
    W, H, AW, AH = 201, 137, 256, 192
    msg = C.create_string_buffer(256)
    buf = E.aligned_zeros(4 * AW * AH, np.uint8)
    pad = E.aligned_zeros(2 * AW * AH, np.uint16)
    ok = dict(pitch=2 * W, fs=2 * W * H, ps=2 * AW * AH, n=1, data=buf, padded=pad)

    def run(**kw):
        a = dict(ok, **kw)
        return lib().emu_deep_ingest(_p(a["data"]), ULL(a["pitch"]), ULL(a["fs"]), _p(a["padded"]), ULL(a["ps"]), a["n"], W, H, AW, AH, msg, 256)

    assert run() >= 0
    assert run(pitch=2 * W - 2) == -1 and b"pitch" in msg.value
    assert run(pitch=2 * W + 1) == -1 and b"2-byte" in msg.value
    assert run(data=buf[1:]) == -1 and b"2-byte" in msg.value
    assert run(padded=pad.view(np.uint8)[1:]) == -1
    assert run(n=2, ps=2 * AW * AH - 2) == -1 and b"padded_stride" in msg.value
    assert run(n=2, fs=2 * W * H - 2) == -1
    assert run(n=65) == -1


def test_every_deep_selector_kernel_was_launched():
    """The driver's own enumeration of every kernel the selectors can return for a DEEP launch -- 16 forward (band x
    transform x vec), 12 synthesis (band x 5/3, 9/7 dividing, 9/7 FAST), 4 layout -- each launched at least once here."""
    cap, nb = 128, 96
    ptrs = (C.c_void_p * cap)()
    labels = C.create_string_buffer(cap * nb)
    n = lib().emu_deep_selector_kernels(ptrs, labels, nb, cap)
    assert n == 32
    want = {int(ptrs[i]): labels.raw[i * nb:(i + 1) * nb].split(b"\0", 1)[0].decode() for i in range(n)}
    lib().emu_deep_log_reset()
    bd, wl = 10, 2
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1 << bd, (64, 128)).astype(np.uint16)
    for band in (4, 8, 16, 32):
        with env(PICSONG_DWT_BANDS=f"{band},4"):
            for lossy in (False, True):
                ref = D.forward(x, bd, wl, lossy)[:x.size].reshape(x.shape)
                for off in (0, 2):
                    got, _ = forward([x], bd, wl, lossy, off=off)
                    assert _same(got[0], ref)
                c = np.trunc(ref).astype(np.int32)
                for exact in ((None, 1) if lossy else (None,)):
                    with env(PICSONG_DWT_EXACTDIV=exact):
                        got, fused = inverse([c], bd, wl, lossy)
                        assert fused and np.array_equal(got[0], D.inverse(c, bd, wl, lossy))
    msg = C.create_string_buffer(64)
    img = E.aligned_zeros(64 * 128 + 8, np.uint16)
    pad = E.aligned_zeros(64 * 128, np.uint16)
    for off in (0, 1):
        assert lib().emu_deep_ingest(_p(img[off:]), ULL(256), ULL(0), _p(pad), ULL(0), 1, 128, 64, 128, 64, msg, 64) == 1 - off
        assert lib().emu_deep_emit(_p(pad), ULL(0), _p(img[off:]), ULL(256), ULL(0), 1, 128, 64, 128, 64, msg, 64) == 1 - off
    got = (C.c_void_p * cap)()
    m = lib().emu_deep_log_read(got, cap)
    launched = set(int(p or 0) for p in got[:min(m, cap)])
    missing = [lab for p, lab in want.items() if p not in launched]
    assert not missing, missing
