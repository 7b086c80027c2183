"""numpy reference of the pixel layouts (picsong_image, include/picsong_hip.h): W x H pixels at a byte pitch, one byte a
pixel or interleaved RGB(A), to and from R, G, B planes.  TEST INFRASTRUCTURE ONLY -- shared by the emulated, GPU and
command-line layout tests; never the code under test."""
import numpy as np

GREY8, PLANAR3, RGB24, BGR24, RGBA32, BGRA32 = range(6)
LAYOUTS = (GREY8, PLANAR3, RGB24, BGR24, RGBA32, BGRA32)
NAMES = {GREY8: "grey", PLANAR3: "planar", RGB24: "rgb", BGR24: "bgr", RGBA32: "rgba", BGRA32: "bgra"}
BPP = {GREY8: 1, PLANAR3: 1, RGB24: 3, BGR24: 3, RGBA32: 4, BGRA32: 4}
PLANES = {GREY8: 1, PLANAR3: 3, RGB24: 3, BGR24: 3, RGBA32: 3, BGRA32: 3}
# the byte of R, G, B in a pixel of the interleaved layouts
CHAN = {RGB24: (0, 1, 2), BGR24: (2, 1, 0), RGBA32: (0, 1, 2), BGRA32: (2, 1, 0)}


def plane_span(layout, W, H, pitch):
    """Bytes from a plane's (an interleaved frame's) first to its last addressed byte."""
    return (H - 1) * pitch + W * BPP[layout]


def frame_span(layout, W, H, pitch, plane_stride=0):
    """Bytes one frame addresses: the smallest buffer that holds it."""
    return plane_span(layout, W, H, pitch) + (2 * plane_stride if layout == PLANAR3 else 0)


def _rows(buf, off, W_bytes, H, pitch):
    """A (H, W_bytes) view of the rows at buf[off + y * pitch]."""
    return np.lib.stride_tricks.as_strided(buf[off:], (H, W_bytes), (pitch, 1))


def pack_into(buf, planes, layout, pitch, plane_stride=0, alpha=255):
    """Write the (H, W) planes into the flat uint8 `buf` as a frame of `layout`: only pixel bytes are touched."""
    H, W = planes[0].shape
    assert len(planes) == PLANES[layout] and buf.size >= frame_span(layout, W, H, pitch, plane_stride)
    if layout in (GREY8, PLANAR3):
        for c, p in enumerate(planes):
            _rows(buf, c * plane_stride, W, H, pitch)[...] = p
        return buf
    bpp = BPP[layout]
    for y in range(H):
        row = buf[y * pitch:y * pitch + W * bpp].reshape(W, bpp)
        for c in range(3):
            row[:, CHAN[layout][c]] = planes[c][y]
        if bpp == 4:
            row[:, 3] = alpha
    return buf


def pack(planes, layout, pitch, plane_stride=0, alpha=255, fill=None, seed=0):
    """A buffer EXACTLY as long as the frame addresses; the bytes between rows random (or `fill`)."""
    H, W = planes[0].shape
    n = frame_span(layout, W, H, pitch, plane_stride)
    buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if fill is None else np.full(n, fill, np.uint8)
    return pack_into(buf, planes, layout, pitch, plane_stride, alpha)


def unpack(buf, layout, W, H, pitch, plane_stride=0):
    """The R, G, B (or the one grey) planes of a frame of `layout` in the flat uint8 `buf`."""
    if layout in (GREY8, PLANAR3):
        return [_rows(buf, c * plane_stride, W, H, pitch).copy() for c in range(PLANES[layout])]
    bpp = BPP[layout]
    out = [np.empty((H, W), np.uint8) for _ in range(3)]
    for y in range(H):
        row = buf[y * pitch:y * pitch + W * bpp].reshape(W, bpp)
        for c in range(3):
            out[c][y] = row[:, CHAN[layout][c]]
    return out


def random_planes(layout, W, H, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(PLANES[layout])]
