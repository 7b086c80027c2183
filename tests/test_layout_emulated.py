"""The pixel-layout kernels on the CPU wave emulator (tests/hipemu/emu_layout_driver.cpp): ingest_kernel against
oracle_lib.pad_frame of the numpy-split planes, emit_kernel against numpy's interleave of the crop inside a
sentinel-filled buffer, both forms (vector and per byte), every layout, and the argument check of the calls."""
import ctypes as C

import numpy as np
import pytest

import emu_lib as E
import layout_ref as lr
import oracle_lib as orc
from emu_lib import _p, driver_lib

_lib = None
ULL = C.c_ulonglong
SENTINEL = 0xA5

# (201,137): odd width, 3 W no multiple of 4; (33,40): AW - W = 31 <= W, almost every padded column mirrored;
# (130,70): AW - W = 62, AH - H = 58; (192,128): no padding; (700,500): several row batches, W % 16 = 12
SHAPES = [(201, 137), (33, 40), (130, 70), (192, 128), (700, 500)]


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_layout.so", ("emu_layout_driver.cpp", "emu_runtime.cpp"), ("-Wno-attributes",))
        _lib.emu_guard_alloc.restype = C.c_void_p
        _lib.emu_guard_alloc.argtypes = [ULL]
        _lib.emu_guard_free.argtypes = [C.c_void_p, ULL]
    return _lib


def _up(v, m):
    return (v + m - 1) // m * m


def _at_offset(data, off):
    """A copy of `data` whose first byte lies `off` bytes behind a 64-byte boundary, in a buffer that ends with it."""
    raw = E.aligned_zeros(off + data.size, np.uint8)
    raw[off:] = data
    return raw[off:]


def _pitches(layout, W):
    row = W * lr.BPP[layout]
    return [row, row + 3, _up(row, 256)]


def _plane_stride(layout, W, H, pitch):
    """Planar: planes a little more than a plane apart, 4-byte aligned exactly when the pitch is."""
    if layout != lr.PLANAR3:
        return 0
    span = lr.plane_span(layout, W, H, pitch)
    return _up(span, 4) + 8 if pitch % 4 == 0 else (span + 5) | 1


def _want_padded(planes):
    return np.concatenate([orc.pad_frame(p).ravel() for p in planes])


def _ingest(layout, buf, pitch, plane_stride, frame_stride, n, W, H, pad_stride=None, pad_off=0):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    frame = lr.PLANES[layout] * AW * AH
    pad_stride = frame if pad_stride is None else pad_stride
    raw = E.aligned_zeros(pad_off + (n - 1) * pad_stride + frame + 64, np.uint8)
    raw[:] = SENTINEL
    out = raw[pad_off:]
    vec = lib().emu_ingest(layout, _p(buf), ULL(pitch), ULL(plane_stride), ULL(frame_stride), _p(out), ULL(pad_stride), n, W, H, AW, AH)
    assert vec >= 0, "refused"
    assert (raw[:pad_off] == SENTINEL).all()
    return out, bool(vec), frame, pad_stride


@pytest.mark.parametrize("layout", lr.LAYOUTS, ids=[lr.NAMES[x] for x in lr.LAYOUTS])
@pytest.mark.parametrize("W,H", SHAPES)
def test_ingest_pads_and_splits(W, H, layout):
    planes = lr.random_planes(layout, W, H, seed=W * 7 + layout)
    want = _want_padded(planes)
    for pitch in _pitches(layout, W):
        ps = _plane_stride(layout, W, H, pitch)
        src = lr.pack(planes, layout, pitch, ps, alpha=0x3C, seed=pitch)          # exactly as long as the last addressed byte
        assert src.size == lr.frame_span(layout, W, H, pitch, ps)
        for off in (0, 1):
            buf = _at_offset(src, off)
            got, vec, frame, _ = _ingest(layout, buf, pitch, ps, 0, 1, W, H)
            assert vec == (off == 0 and pitch % 4 == 0), (pitch, off)
            assert np.array_equal(got[:frame], want), (pitch, off)
            assert (got[frame:] == SENTINEL).all()
    # the padded side at an odd address: the per-byte form, the same bytes
    pitch = _pitches(layout, W)[2]
    ps = _up(lr.plane_span(layout, W, H, pitch), 16) if layout == lr.PLANAR3 else 0
    buf = _at_offset(lr.pack(planes, layout, pitch, ps), 0)
    got, vec, frame, _ = _ingest(layout, buf, pitch, ps, 0, 1, W, H, pad_off=1)
    assert not vec and np.array_equal(got[:frame], want) and (got[frame:] == SENTINEL).all()


@pytest.mark.parametrize("layout", lr.LAYOUTS, ids=[lr.NAMES[x] for x in lr.LAYOUTS])
@pytest.mark.parametrize("W,H", [(201, 137), (130, 70)])
def test_ingest_of_three_frames_with_strides_above_a_frame(W, H, layout):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    for pitch, extra in ((_up(W * lr.BPP[layout], 16), 48), (W * lr.BPP[layout] + 3, 5)):
        ps = (lr.plane_span(layout, W, H, pitch) + 12) if layout == lr.PLANAR3 else 0
        span = lr.frame_span(layout, W, H, pitch, ps)
        fs = (_up(span, 16) if extra == 48 else span) + extra
        frames = [lr.random_planes(layout, W, H, seed=100 + f) for f in range(3)]
        src = np.random.default_rng(3).integers(0, 256, 2 * fs + span, dtype=np.uint8)     # ends with frame 2's last byte
        for f in range(3):
            lr.pack_into(src[f * fs:], frames[f], layout, pitch, ps, alpha=f)
        buf = _at_offset(src, 0)
        pad_stride = lr.PLANES[layout] * AW * AH + 64
        got, vec, frame, _ = _ingest(layout, buf, pitch, ps, fs, 3, W, H, pad_stride=pad_stride)
        assert vec == (extra == 48 and ps % 4 == 0)
        for f in range(3):
            assert np.array_equal(got[f * pad_stride:f * pad_stride + frame], _want_padded(frames[f])), f
            assert (got[f * pad_stride + frame:(f + 1) * pad_stride] == SENTINEL).all()


def _emit(layout, padded, pad_stride, out, pitch, plane_stride, frame_stride, n, W, H):
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    vec = lib().emu_emit(layout, _p(padded), ULL(pad_stride), _p(out), ULL(pitch), ULL(plane_stride), ULL(frame_stride), n, W, H, AW, AH)
    assert vec >= 0, "refused"
    return bool(vec)


def _padded_random(layout, W, H, seed):
    """Padded planes whose padding is NOT the mirror of the image: emit must crop, not look at it."""
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    rng = np.random.default_rng(seed)
    full = [rng.integers(0, 256, (AH, AW), dtype=np.uint8) for _ in range(lr.PLANES[layout])]
    return full, [p[:H, :W] for p in full]


@pytest.mark.parametrize("layout", lr.LAYOUTS, ids=[lr.NAMES[x] for x in lr.LAYOUTS])
@pytest.mark.parametrize("W,H", SHAPES)
def test_emit_crops_and_interleaves_inside_its_rows(W, H, layout):
    full, crop = _padded_random(layout, W, H, seed=W + 31 * layout)
    padded = E.aligned_copy(np.concatenate([p.ravel() for p in full]))
    for pitch in _pitches(layout, W):
        ps = _plane_stride(layout, W, H, pitch)
        span = lr.frame_span(layout, W, H, pitch, ps)
        want = lr.pack_into(np.full(span + 40, SENTINEL, np.uint8), crop, layout, pitch, ps, alpha=255)
        for off in (0, 1):
            out = _at_offset(np.full(span + 40, SENTINEL, np.uint8), off)
            vec = _emit(layout, padded, 0, out, pitch, ps, 0, 1, W, H)
            assert vec == (off == 0 and pitch % 4 == 0), (pitch, off)
            # the pixels, alpha = 255, and every other byte -- the gaps, everything behind the last row -- still the sentinel
            assert np.array_equal(out, want), (pitch, off)


@pytest.mark.parametrize("layout", lr.LAYOUTS, ids=[lr.NAMES[x] for x in lr.LAYOUTS])
def test_emit_of_three_frames(layout):
    W, H = 201, 137
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    pad_stride = lr.PLANES[layout] * AW * AH + 32
    padded = E.aligned_zeros(3 * pad_stride, np.uint8)
    crops = []
    for f in range(3):
        full, crop = _padded_random(layout, W, H, seed=f)
        padded[f * pad_stride:f * pad_stride + pad_stride - 32] = np.concatenate([p.ravel() for p in full])
        crops.append(crop)
    pitch = _up(W * lr.BPP[layout], 4) + 4
    ps = _plane_stride(layout, W, H, pitch)
    span = lr.frame_span(layout, W, H, pitch, ps)
    fs = _up(span, 4) + 20
    want = np.full(2 * fs + span + 16, SENTINEL, np.uint8)
    for f in range(3):
        lr.pack_into(want[f * fs:], crops[f], layout, pitch, ps)
    out = _at_offset(np.full(want.size, SENTINEL, np.uint8), 0)
    assert _emit(layout, padded, pad_stride, out, pitch, ps, fs, 3, W, H)
    assert np.array_equal(out, want)


def _guarded(n):
    p = lib().emu_guard_alloc(n)
    assert p
    return p, np.ctypeslib.as_array((C.c_uint8 * n).from_address(p))


@pytest.mark.parametrize("layout", lr.LAYOUTS, ids=[lr.NAMES[x] for x in lr.LAYOUTS])
@pytest.mark.parametrize("W,H", [(201, 137), (192, 128), (33, 40)])
def test_no_access_behind_the_last_addressed_byte(W, H, layout):
    """The image side ends where an inaccessible page begins: a byte read (ingest) or written (emit) behind the last row's
    last pixel is a fault."""
    AW, AH = orc.pad_dim(W), orc.pad_dim(H)
    for pitch in (W * lr.BPP[layout], _up(W * lr.BPP[layout], 256)):
        ps = _up(lr.plane_span(layout, W, H, pitch), 16) if layout == lr.PLANAR3 else 0
        planes = lr.random_planes(layout, W, H, seed=5)
        src = lr.pack(planes, layout, pitch, ps)
        p, g = _guarded(src.size)
        try:
            g[:] = src
            got, _, frame, _ = _ingest(layout, g, pitch, ps, 0, 1, W, H)
            assert np.array_equal(got[:frame], _want_padded(planes))
            g[:] = SENTINEL
            full, crop = _padded_random(layout, W, H, seed=6)
            _emit(layout, E.aligned_copy(np.concatenate([x.ravel() for x in full])), 0, g, pitch, ps, 0, 1, W, H)
            assert np.array_equal(g, lr.pack_into(np.full(src.size, SENTINEL, np.uint8), crop, layout, pitch, ps))
        finally:
            del g
            lib().emu_guard_free(C.c_void_p(p), src.size)


# ---- the argument check of picsong_ingest_frames / picsong_emit_frames (layout_refusal, kernel_select.hpp) --------------
def _refusal(layout=lr.RGB24, data=1, pitch=None, plane_stride=0, frame_stride=0, padded=1, padded_stride=0, n=1, W=201, H=137,
             AW=None, AH=None):
    AW = orc.pad_dim(W) if AW is None else AW
    AH = orc.pad_dim(H) if AH is None else AH
    pitch = W * lr.BPP.get(layout, 1) if pitch is None else pitch
    buf = np.zeros(16, np.uint8)
    msg = C.create_string_buffer(256)
    r = lib().emu_layout_refusal(layout, _p(buf) if data else None, ULL(pitch), ULL(plane_stride), ULL(frame_stride),
                                 _p(buf) if padded else None, ULL(padded_stride), n, W, H, AW, AH, msg, len(msg))
    return msg.value.decode() if r else None


def test_refusals():
    W, H = 201, 137
    P = orc.pad_dim(W) * orc.pad_dim(H)
    assert _refusal() is None
    assert "null" in _refusal(data=0)
    assert "null" in _refusal(padded=0)
    for bad in (-1, 6, 99):
        assert "layout" in _refusal(layout=bad)
    for layout in lr.LAYOUTS:
        row = W * lr.BPP[layout]
        ps = lr.plane_span(layout, W, H, row) if layout == lr.PLANAR3 else 0
        assert _refusal(layout=layout, pitch=row, plane_stride=ps) is None
        assert "pitch" in _refusal(layout=layout, pitch=row - 1, plane_stride=ps)
        span = lr.frame_span(layout, W, H, row, ps)
        frame = lr.PLANES[layout] * P
        assert _refusal(layout=layout, plane_stride=ps, n=2, frame_stride=span, padded_stride=frame) is None
        assert "frame_stride" in _refusal(layout=layout, plane_stride=ps, n=2, frame_stride=span - 1, padded_stride=frame)
        assert "padded_stride" in _refusal(layout=layout, plane_stride=ps, n=2, frame_stride=span, padded_stride=frame - 1)
        # one frame addresses no second one: its strides are not looked at
        assert _refusal(layout=layout, plane_stride=ps, n=1, frame_stride=0, padded_stride=0) is None
    span = lr.plane_span(lr.PLANAR3, W, H, W + 3)
    assert _refusal(layout=lr.PLANAR3, pitch=W + 3, plane_stride=span) is None
    assert "plane_stride" in _refusal(layout=lr.PLANAR3, pitch=W + 3, plane_stride=span - 1)
    for n in (0, -1, 65):
        assert "n outside" in _refusal(n=n, frame_stride=1 << 20, padded_stride=1 << 24)
    assert _refusal(n=64, frame_stride=1 << 20, padded_stride=1 << 24) is None
    # the rule picsong_pad_frame_host refuses: more added columns / rows than the frame has
    assert _refusal(W=32, H=40, AW=64, AH=64) is None
    assert "mirror" in _refusal(W=31, H=40, AW=64, AH=64)
    assert "mirror" in _refusal(W=40, H=31, AW=64, AH=64)
    with pytest.raises(ValueError):
        orc.pad_frame(np.zeros((40, 31), np.uint8))


def test_refused_calls_run_nothing():
    W, H = 33, 40
    out = np.full(64 * 64, SENTINEL, np.uint8)
    src = np.zeros(W * H, np.uint8)
    assert lib().emu_ingest(lr.GREY8, _p(src), ULL(W - 1), ULL(0), ULL(0), _p(out), ULL(0), 1, W, H, 64, 64) == -1
    assert lib().emu_ingest(7, _p(src), ULL(W), ULL(0), ULL(0), _p(out), ULL(0), 1, W, H, 64, 64) == -1
    assert (out == SENTINEL).all()
    assert lib().emu_emit(lr.GREY8, _p(src), ULL(0), _p(out), ULL(W - 1), ULL(0), ULL(0), 1, W, H, 64, 64) == -1
    assert (out == SENTINEL).all()
