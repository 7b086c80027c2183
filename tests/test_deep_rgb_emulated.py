"""Deep RGB contexts (bit_depth 9..16, three uint16 planes a frame) on the CPU wave emulator
(tests/hipemu/emu_deep_rgb_driver.cpp): the library's own plans, selectors and launch sequences over the kernel sources,
against deep_rgb_ref -- the oracle's stage functions between a numpy colour transform and a numpy inverse.  Every
comparison is bit for bit / byte for byte."""
import ctypes as C

import numpy as np
import pytest

import deep_ref as D
import deep_rgb_ref as R
import drop_ref as dr
import emu_lib as E
import oracle_lib as orc
from emu_lib import _geo, _p, driver_lib
from test_deep_emulated import env

_lib = None
ULL = C.c_ulonglong
SENT = 0xA5C3
AW, AH = R.AW, R.AH
P = AW * AH


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_deep_rgb.so", ("emu_deep_rgb_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
        vp = C.c_void_p
        _lib.emu_drgb_transform_fwd.argtypes = [vp] * 6 + [C.c_size_t, C.c_int, C.c_int, C.c_int, ULL, ULL]
        _lib.emu_drgb_transform_inv.argtypes = [vp] * 6 + [C.c_size_t, C.c_int, C.c_int, C.c_int, ULL, ULL]
    return _lib


def planes_buffer(frames, gap=0, pgap=0, off=0):
    """n frames' padded planes: plane c of frame f at byte off + f * stride + c * (2 P + pgap) behind a 64-byte boundary,
    stride = 3 (2 P + pgap) + gap, the sentinel everywhere else.  (whole buffer, the three views at frame 0's planes, the
    planes' element offsets, stride)"""
    n = len(frames)
    pstep = 2 * P + pgap
    stride = 3 * pstep + gap
    assert off % 2 == 0 and gap % 2 == 0 and pgap % 2 == 0
    raw = E.aligned_zeros((off + n * stride) // 2 + 32, np.uint16)
    raw[:] = SENT
    at = [(off + c * pstep) // 2 for c in range(3)]
    for f, planes in enumerate(frames):
        for c in range(3):
            o = at[c] + f * stride // 2
            raw[o:o + P] = np.asarray(planes[c]).ravel()
    return raw, [raw[a:] for a in at], at, stride


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _all(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the colour transforms -----------------------------------------------------------------------------------------------
def _ends_frame(bd, seed):
    rng = np.random.default_rng(seed)
    pad = [rng.integers(0, 1 << bd, (64, 64)).astype(np.uint16) for _ in range(3)]
    for k in range(3):
        pad[k][k, :8] = [0, 65535, 0, 65535, (1 << bd) - 1, 1 << (bd - 1), 65535, 0]        # (read unsigned: 65535 is never -1)
    return pad


@pytest.mark.parametrize("bd", [9, 12, 16])
@pytest.mark.parametrize("lossy", [False, True])
def test_colour_transforms_bit_for_bit(bd, lossy):
    n4 = 64 * 64 // 4
    T = np.float32 if lossy else np.int32
    frames = [_ends_frame(bd, s) for s in (1, 2)]
    wants = [R.forward(f[0], f[1], f[2], bd, lossy) for f in frames]
    for off in (0, 2):                                      # 8-byte accesses, 2-byte accesses
        src = [E.aligned_zeros(2 * 4096 + 64, np.uint16)[off // 2:] for _ in range(3)]
        for k in range(3):
            src[k][:4096] = frames[0][k].ravel()
            src[k][4096 + 16:2 * 4096 + 16] = frames[1][k].ravel()
        out = [E.aligned_zeros(2 * 4096, T) for _ in range(3)]
        assert lib().emu_drgb_transform_fwd(_p(src[0]), _p(src[1]), _p(src[2]), _p(out[0]), _p(out[1]), _p(out[2]), n4, int(lossy), bd, 2,
                                            2 * (4096 + 16), 4 * 4096) == 0
        for f in range(2):
            for k in range(3):
                assert _same(out[k][f * 4096:(f + 1) * 4096], wants[f][k].ravel()), (off, f, k)
        # the inverse, components scaled past the range: both clamp ends occur
        comp = [np.concatenate([(wants[f][k].astype(np.float64) * 1.5).astype(T).ravel() for f in range(2)]) for k in range(3)]
        cin = [E.aligned_copy(c) for c in comp]
        dst = [E.aligned_zeros(2 * 4096 + 64, np.uint16) for _ in range(3)]
        for d in dst:
            d[:] = SENT
        view = [d[off // 2:] for d in dst]
        assert lib().emu_drgb_transform_inv(_p(cin[0]), _p(cin[1]), _p(cin[2]), _p(view[0]), _p(view[1]), _p(view[2]), n4, int(lossy), bd, 2,
                                            4 * 4096, 2 * (4096 + 16)) == 0
        for f in range(2):
            ref = R.inverse(*[comp[k][f * 4096:(f + 1) * 4096] for k in range(3)], bd)
            assert min(r.min() for r in ref) == 0 and max(r.max() for r in ref) == (1 << bd) - 1
            for k in range(3):
                o = f * (4096 + 16)
                assert np.array_equal(view[k][o:o + 4096], ref[k]), (off, f, k)
        for k in range(3):                                   # nothing but the 2 x 4096 samples a plane was written
            mask = np.ones(dst[k].size, bool)
            for f in range(2):
                o = off // 2 + f * (4096 + 16)
                mask[o:o + 4096] = False
            assert (dst[k][mask] == SENT).all()


# ---- level 0 with the colour transform in its load stage -----------------------------------------------------------------
def forward(frames, bd, wl, lossy, qs=1.0, gap=0, pgap=0, off=0):
    """emu_drgb_forward over n frames; (the 3 n (AH, AW) Mallat arrays, bits)."""
    n = len(frames)
    extra = orc.dwt_extra(AW, AH, wl)
    raw, views, at, stride = planes_buffer(frames, gap, pgap, off)
    before = raw.copy()
    coef = E.aligned_zeros(3 * n * (P + extra), np.float32 if lossy else np.int32)
    bits = lib().emu_drgb_forward(_p(views[0]), _p(views[1]), _p(views[2]), ULL(stride), n, _p(coef), AW, AH, wl, int(lossy), C.c_float(qs), bd)
    assert bits >= 0
    assert np.array_equal(raw, before), "the input is read only"
    return [coef[z * (P + extra):z * (P + extra) + P].reshape(AH, AW) for z in range(3 * n)], bits


def _pads(kind, bd, wl):
    return [D.mirror_pad(R.inputs(kind, bd, wl, c)) for c in range(3)]


def _want_coef(pad, bd, wl, lossy, qs):
    comp = R.forward(pad[0], pad[1], pad[2], bd, lossy)
    return [orc.dwt_forward(np.ascontiguousarray(c), wl, qs)[:P].reshape(AH, AW) for c in comp]


@pytest.mark.parametrize("lossy,qs,bd,wl", [(False, 1.0, 12, 5), (True, 0.25, 16, 2), (True, 1.0, 9, 5), (False, 1.0, 16, 2)])
def test_fused_level_0_against_the_separate_transform(lossy, qs, bd, wl):
    frames = [_pads(k, bd, wl) for k in ("saw", "noise", "smooth")]
    frames[1][0] = frames[1][0].copy()
    frames[1][0][0, :4] = [0, 65535, 65535, 0]
    wants = [_want_coef(f, bd, wl, lossy, qs) for f in frames]

    def check(got, nf, what):
        for z in range(3 * nf):
            assert _same(got[z], wants[z // 3][z % 3]), (what, z)

    got, bits = forward(frames[:1], bd, wl, lossy, qs)
    assert bits & 3 == 3
    check(got, 1, "vector")
    for off, pgap in ((2, 0), (0, 2)):                       # a plane at an odd 2-byte offset: the per-column form
        got, bits = forward(frames[:1], bd, wl, lossy, qs, off=off, pgap=pgap)
        assert bits & 3 == 1
        check(got, 1, ("per column", off, pgap))
    with env(PICSONG_DEEP_NOFUSE=1):
        for off in (0, 2):
            got, bits = forward(frames[:1], bd, wl, lossy, qs, off=off)
            assert bits == 0
            check(got, 1, ("nofuse", off))
    for band in (4, 8, 16, 32):                              # every band height the selector can return
        with env(PICSONG_DWT_BANDS=f"{band},8,8"):
            for off in (0, 2):
                got, bits = forward(frames[:1], bd, wl, lossy, qs, off=off)
                # (the per-column form takes bands of at most 8 rows: the plan gives it the next smaller one)
                assert bits & 3 == (3 if off == 0 else 1) and bits >> 8 == (band if off == 0 else min(band, 8))
                check(got, 1, ("band", band, off))
    # three frames with sentinel gaps between planes and frames: 16-byte multiples keep the vector form
    for gap, pgap, vec in ((48, 32, True), (6, 0, False), (0, 6, False)):
        got, bits = forward(frames, bd, wl, lossy, qs, gap=gap, pgap=pgap)
        assert bits & 3 == (3 if vec else 1)
        check(got, 3, (gap, pgap))
    with env(PICSONG_DEEP_NOFUSE=1):
        got, bits = forward(frames, bd, wl, lossy, qs, gap=6, pgap=2)
        assert bits == 0
        check(got, 3, "nofuse, 3 frames")


# ---- frame sequences -----------------------------------------------------------------------------------------------------
def _tables(lossy, wl, k):
    luts = [R.lut(lossy, wl, c, k) for c in range(3)]
    return luts, [np.ascontiguousarray(t.table, np.int32) for t in luts]


def encode(frames, bd, wl, lossy, qs, k=0.0, first_iter=0, header_mask=7, gap=0, pgap=0, off=0):
    n = len(frames)
    luts, tabs = _tables(lossy, wl, k)
    stride = 9 + 2 * (AW // 64) * (AH // 64) + P + 1
    streams = np.full(3 * n * stride, 0x7777, np.uint16)
    totals = np.zeros(3 * n, np.int32)
    flag = np.zeros(1, np.int32)
    raw, views, at, fs = planes_buffer(frames, gap, pgap, off)
    hdr = R.header(R.W, R.H, bd, wl, lossy, qs, k)
    bits = lib().emu_drgb_encode(_p(views[0]), _p(views[1]), _p(views[2]), ULL(fs), n, first_iter, header_mask, _p(streams), ULL(stride),
                                 _p(totals), AW, AH, wl, int(lossy), C.c_float(qs), bd, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])),
                                 C.c_float(k), int(getattr(luts[0], "n_tables", 1)), _p(hdr), _p(flag))
    assert bits >= 0
    return [streams[z * stride:z * stride + totals[z]].copy() for z in range(3 * n)], int(flag[0]), bits


def decode(streams, bd, wl, lossy, qs, k=0.0, drop=0, gap=0, pgap=0, off=0):
    n = len(streams) // 3
    luts, tabs = _tables(lossy, wl, k)
    stride = 9 + 2 * (AW // 64) * (AH // 64) + P + 1
    sbuf = np.full(3 * n * stride, 0xFFFF, np.uint16)
    for z, s in enumerate(streams):
        sbuf[z * stride:z * stride + s.size] = s
    flag = np.zeros(1, np.int32)
    blank = [np.full((AH, AW), SENT, np.uint16)] * 3
    raw, views, at, fs = planes_buffer([blank] * n, gap, pgap, off)
    bits = lib().emu_drgb_decode(_p(sbuf), ULL(stride), n, _p(views[0]), _p(views[1]), _p(views[2]), ULL(fs), AW, AH, wl, int(lossy),
                                 C.c_float(qs), bd, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(_geo(luts[0])), C.c_float(k),
                                 int(getattr(luts[0], "n_tables", 1)), drop, _p(flag))
    assert bits >= 0 and not bits & 8
    outs, mask = [], np.ones(raw.size, bool)
    for f in range(n):
        planes = []
        for c in range(3):
            o = at[c] + f * fs // 2
            planes.append(raw[o:o + P].reshape(AH, AW).copy())
            mask[o:o + P] = False
        outs.append(planes)
    assert (raw[mask] == SENT).all(), "decoding writes exactly the 2 P bytes of each plane"
    return outs, int(flag[0]), bits


@pytest.mark.parametrize("case", R.IN_RANGE, ids=[R.row_id(r) for r in R.IN_RANGE])
def test_frame_sequences_match_the_composed_reference(case):
    lossy, bd, kind, wl, qs, want_max, want_raw = case
    img, pad, comp, coef, sizes, with_hdr = R.encode(kind, bd, wl, lossy, qs)
    R.check_precondition(coef, sizes, want_max, want_raw)
    bare = R.encode(kind, bd, wl, lossy, qs, header_mask=0)[5]
    for c in range(3):
        assert (bare[c][:9] == 0xFFFF).all() and np.array_equal(bare[c][9:], with_hdr[c][9:])
    got, flag, bits = encode([pad, pad], bd, wl, lossy, qs)
    assert flag == 0 and bits & 3 == 3
    assert _all(got, list(with_hdr) + list(bare))
    want = R.decode(with_hdr, bd, wl, lossy, qs)
    dec, flag, bits = decode(got, bd, wl, lossy, qs)
    assert flag == 0 and bits == 0
    assert _all(dec[0], want) and _all(dec[1], want)
    if not lossy:
        assert _all(dec[0], pad), "the 5/3 round trip is exact"


def test_frame_sequences_on_the_other_routes():
    lossy, bd, kind, wl, qs = R.row(True, 12, "saw")[:5]
    img, pad, comp, coef, sizes, with_hdr = R.encode(kind, bd, wl, lossy, qs)
    want = R.decode(with_hdr, bd, wl, lossy, qs)
    for nofuse in (None, 1):
        with env(PICSONG_DEEP_NOFUSE=nofuse):
            for off, pgap in ((0, 0), (2, 0), (0, 6)):
                got, flag, bits = encode([pad], bd, wl, lossy, qs, off=off, pgap=pgap)
                assert flag == 0 and bits & 3 == (0 if nofuse else (3 if (off, pgap) == (0, 0) else 1)) and _all(got, with_hdr)
                dec, flag, bits = decode(got, bd, wl, lossy, qs, off=off, pgap=pgap)
                assert flag == 0 and _all(dec[0], want)
    # first_iter = -1, header_mask = 5: the header on components 0 and 2 of the call's second frame
    bare = R.encode(kind, bd, wl, lossy, qs, header_mask=0)[5]
    m5 = R.encode(kind, bd, wl, lossy, qs, header_mask=5)[5]
    got, flag, _ = encode([pad, pad], bd, wl, lossy, qs, first_iter=-1, header_mask=5)
    assert _all(got, list(bare) + list(m5))


def test_complexity_scalable_mode():
    lossy, bd, kind, wl, qs = R.row(False, 12, "saw")[:5]
    img, pad, comp, coef, sizes, streams = R.encode(kind, bd, wl, lossy, qs, k=0.5)
    assert max(R.max_coef(coef)) < 32768
    got, flag, _ = encode([pad], bd, wl, lossy, qs, k=0.5)
    assert flag == 0 and _all(got, streams)
    dec, flag, _ = decode(got, bd, wl, lossy, qs, k=0.5)
    assert flag == 0 and _all(dec[0], R.decode(streams, bd, wl, lossy, qs, k=0.5)) and _all(dec[0], pad)


def test_decode_drop_is_the_same_for_the_three_components():
    lossy, bd, kind, wl, qs = R.row(True, 12, "smooth")[:5]
    streams = R.encode(kind, bd, wl, lossy, qs)[5]
    comps = R.synthesis([dr.drop_coefficients(streams[c], AW, AH, wl, R.lut(lossy, wl, c), 2) for c in range(3)], wl, lossy, qs)
    want = R.inverse(comps[0], comps[1], comps[2], bd)
    dec, flag, _ = decode(streams, bd, wl, lossy, qs, drop=2)
    assert flag == 0 and _all(dec[0], want)
    assert not _all(want, R.decode(streams, bd, wl, lossy, qs)), "drop = 2 changes the picture"


@pytest.mark.parametrize("lossy,bd,kind,wl,qs", R.OUT_OF_RANGE)
def test_out_of_range_frames_raise_the_range_flag(lossy, bd, kind, wl, qs):
    pad = _pads(kind, bd, wl)
    assert max(D.max_coef(c) for c in _want_coef(pad, bd, wl, lossy, qs)) >= 32768
    _, flag, _ = encode([pad], bd, wl, lossy, qs)
    assert flag != 0


# ---- every selector kernel -----------------------------------------------------------------------------------------------
def test_every_new_selector_kernel_is_launched():
    cap = 64
    ptrs = (C.c_void_p * cap)()
    labels = C.create_string_buffer(cap * 64)
    n = lib().emu_drgb_selector_kernels(ptrs, labels, 64, cap)
    assert n == 12 + 12 + 4          # level 0: four vector bands and two per-column ones, 5/3 and 9/7; the layouts; the transforms
    want = {ptrs[i]: labels.raw[i * 64:(i + 1) * 64].split(b"\0")[0].decode() for i in range(n)}
    lib().emu_drgb_log_reset()
    bd, wl = 10, 2
    pad = _pads("saw", bd, wl)
    for lossy in (False, True):
        for band in (4, 8, 16, 32):
            with env(PICSONG_DWT_BANDS=f"{band},8"):
                forward([pad], bd, wl, lossy)
                forward([pad], bd, wl, lossy, off=2)
        with env(PICSONG_DEEP_NOFUSE=1):
            streams, _, _ = encode([pad], bd, wl, lossy, 1.0)
        decode(streams, bd, wl, lossy, 1.0)
    for layout in (P3_16, RGB48, RGBA64):                   # (ingest and emit, both forms)
        test_16_bit_colour_layouts(layout, 33, 40)
    got = (C.c_void_p * 256)()
    m = lib().emu_drgb_log_read(got, 256)
    launched = {got[i] for i in range(min(m, 256))}
    missing = [label for p, label in want.items() if p not in launched]
    assert not missing, missing


# ---- the 16-bit colour layouts -------------------------------------------------------------------------------------------
P3_16, RGB48, RGBA64 = 7, 8, 9
SPP = {P3_16: 1, RGB48: 3, RGBA64: 4}
BYTE_SENT = 0xA5


def _up(v, m):
    return (v + m - 1) // m * m


def image_bytes(planes, layout, pitch, off, alpha=None):
    """One frame's W x H pixels in `layout` at `pitch`, `off` bytes behind a 64-byte boundary, the byte sentinel around
    every row.  (whole buffer u8, byte offset of the image, plane_stride, span)"""
    h, w = planes[0].shape
    spp = SPP[layout]
    row = 2 * w * spp
    span = (h - 1) * pitch + row
    plane_stride = (_up(span + 6, 4) if pitch % 4 == 0 else _up(span + 6, 2)) if layout == P3_16 else 0      # (dwords only at a 4-byte pitch)
    total = span + 2 * plane_stride
    raw = E.aligned_zeros(64 + off + total + 64, np.uint8)
    raw[:] = BYTE_SENT
    for y in range(h):
        if layout == P3_16:
            for c in range(3):
                o = 64 + off + c * plane_stride + y * pitch
                raw[o:o + row] = planes[c][y].view(np.uint8)
        else:
            px = np.empty((w, spp), np.uint16)
            for c in range(3):
                px[:, c] = planes[c][y]
            if spp == 4:
                px[:, 3] = 0x1357 if alpha is None else alpha
            o = 64 + off + y * pitch
            raw[o:o + row] = px.reshape(-1).view(np.uint8)
    return raw, 64 + off, plane_stride, total


@pytest.mark.parametrize("layout", [P3_16, RGB48, RGBA64])
@pytest.mark.parametrize("w,h", [(200, 136), (201, 137), (33, 40)])
def test_16_bit_colour_layouts(layout, w, h):
    bd = 12
    mx = (1 << bd) - 1
    aw, ah = orc.pad_dim(w), orc.pad_dim(h)
    PP = aw * ah
    rng = np.random.default_rng(w + layout)
    planes = [rng.integers(0, mx + 1, (h, w)).astype(np.uint16) for _ in range(3)]
    pads = [D.mirror_pad(p, aw, ah) for p in planes]
    msg = C.create_string_buffer(160)
    row = 2 * w * SPP[layout]
    for extra in (0, 2, 14, 16):                             # packed, +2, +14 bytes (2-byte accesses), +16 (dwords)
        pitch = row + extra
        for off in (0, 2):                                   # both forms
            vec = off == 0 and pitch % 4 == 0
            raw, at, ps, total = image_bytes(planes, layout, pitch, off)
            before = raw.copy()
            padded = E.aligned_zeros(3 * PP + 64, np.uint16)
            padded[:] = SENT
            rc = lib().emu_drgb_ingest(layout, C.c_void_p(raw.ctypes.data + at), ULL(pitch), ULL(ps), ULL(0), _p(padded), ULL(0), 1, w, h, aw, ah,
                                       bd, msg, 160)
            assert rc == (1 if vec else 0), (extra, off, msg.value)
            assert np.array_equal(raw, before), "the image is read only"
            for c in range(3):
                assert np.array_equal(padded[c * PP:(c + 1) * PP].reshape(ah, aw), pads[c]), (extra, off, c)
            assert (padded[3 * PP:] == SENT).all()
            # emit into a sentinel-filled image: the W x H pixels and nothing else, alpha = 2^bd - 1
            want, _, _, _ = image_bytes(planes, layout, pitch, off, alpha=mx)
            out = E.aligned_zeros(want.size, np.uint8)
            out[:] = BYTE_SENT
            src = E.aligned_copy(np.concatenate([p.ravel() for p in pads]))
            rc = lib().emu_drgb_emit(layout, _p(src), ULL(0), C.c_void_p(out.ctypes.data + at), ULL(pitch), ULL(ps), ULL(0), 1, w, h, aw, ah, bd,
                                     msg, 160)
            assert rc == (1 if vec else 0), (extra, off, msg.value)
            assert np.array_equal(out, want), (extra, off)


def test_16_bit_colour_layouts_of_three_frames_with_gaps():
    layout, w, h, bd = RGB48, 201, 137, 10
    aw, ah = orc.pad_dim(w), orc.pad_dim(h)
    PP = aw * ah
    rng = np.random.default_rng(9)
    frames = [[rng.integers(0, 1 << bd, (h, w)).astype(np.uint16) for _ in range(3)] for _ in range(3)]
    pitch = 6 * w + 2
    span = (h - 1) * pitch + 6 * w
    fs, pstride = span + 10, 6 * PP + 32
    raw = E.aligned_zeros(64 + 3 * fs + 64, np.uint8)
    raw[:] = BYTE_SENT
    for f in range(3):
        one, at, _, total = image_bytes(frames[f], layout, pitch, 0)
        img = one[at:at + total]
        keep = img != BYTE_SENT
        raw[64 + f * fs:64 + f * fs + total][keep] = img[keep]
        for y in range(h):                                  # (a sample byte may equal the sentinel: copy the rows whole)
            raw[64 + f * fs + y * pitch:64 + f * fs + y * pitch + 6 * w] = img[y * pitch:y * pitch + 6 * w]
    padded = E.aligned_zeros(3 * pstride // 2 + 64, np.uint16)
    padded[:] = SENT
    msg = C.create_string_buffer(160)
    rc = lib().emu_drgb_ingest(layout, C.c_void_p(raw.ctypes.data + 64), ULL(pitch), ULL(0), ULL(fs), _p(padded), ULL(pstride), 3, w, h, aw, ah, bd,
                               msg, 160)
    assert rc == 1, msg.value                                # (pitch, frame stride and padded stride allow the vector form)
    mask = np.ones(padded.size, bool)
    for f in range(3):
        for c in range(3):
            o = f * pstride // 2 + c * PP
            assert np.array_equal(padded[o:o + PP].reshape(ah, aw), D.mirror_pad(frames[f][c], aw, ah)), (f, c)
            mask[o:o + PP] = False
    assert (padded[mask] == SENT).all()
    out = E.aligned_zeros(raw.size, np.uint8)
    out[:] = BYTE_SENT
    rc = lib().emu_drgb_emit(layout, _p(padded), ULL(pstride), C.c_void_p(out.ctypes.data + 64), ULL(pitch), ULL(0), ULL(fs), 3, w, h, aw, ah, bd,
                             msg, 160)
    assert rc == 1 and np.array_equal(out, raw)


def test_layout_refusals_by_kind_of_context():
    buf = E.aligned_zeros(1 << 16, np.uint8)
    msg = C.create_string_buffer(160)

    def refused(layout, deep, deep_rgb, data_off=0, pitch=None, plane_stride=1 << 14, n=1, fs=0, ps=0):
        bpp = {0: 1, 1: 1, 2: 3, 4: 4, 6: 2, 7: 2, 8: 6, 9: 8}[layout]
        return lib().emu_drgb_layout_refusal(layout, C.c_void_p(buf.ctypes.data + data_off), ULL(33 * bpp if pitch is None else pitch),
                                             ULL(plane_stride), ULL(fs), _p(buf), ULL(ps), n, 33, 40, 64, 64, int(deep), int(deep_rgb), msg, 160)

    for layout in (P3_16, RGB48, RGBA64):
        assert refused(layout, True, True) == 0, msg.value
        assert refused(layout, False, False) == 1 and refused(layout, True, False) == 1      # an 8-bit context, a deep grey one
        assert refused(layout, True, True, data_off=1) == 1 and refused(layout, True, True, pitch=33 * SPP[layout] * 2 + 1) == 1
        assert refused(layout, True, True, pitch=33 * SPP[layout] * 2 - 2) == 1
        assert refused(layout, True, True, n=2, fs=1 << 16, ps=6 * 64 * 64) == 0, msg.value
        assert refused(layout, True, True, n=2, fs=1 << 16, ps=6 * 64 * 64 - 2) == 1 and refused(layout, True, True, n=2, fs=(1 << 16) + 1, ps=6 * 64 * 64) == 1
    assert refused(P3_16, True, True, plane_stride=(1 << 14) + 1) == 1 and refused(P3_16, True, True, plane_stride=100) == 1
    for layout in (0, 1, 2, 4, 6):                           # the 8-bit layouts and GREY16 on a deep RGB context
        assert refused(layout, True, True) == 1 and b"PLANAR3_16" in msg.value
    assert refused(6, True, False) == 0 and refused(2, False, False) == 0
