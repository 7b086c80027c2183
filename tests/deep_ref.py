"""Expected output of the deep contexts (bit_depth 9..16, uint16 samples), composed from the CPU oracle's STAGE functions.
TEST INFRASTRUCTURE ONLY.  The oracle's frame functions are 8-bit; here the two ends are numpy -- the mirror pad on 2-byte
samples, the level shift with the depth as a parameter, the clamp with 255 replaced by 2^bd - 1 -- and everything between
(transform, coder, pack) is the oracle's own."""
import numpy as np

import oracle_lib as orc

W, H = 200, 136                     # the tests' frame: AW x AH = 256 x 192, 12 codeblocks
AW, AH = 256, 192


def mirror_pad(img, aw=None, ah=None):
    """Column W + j = column W - 1 - j, padded row H + r = padded row H - 1 - r (picsong_pad_frame_host's rule)."""
    h, w = img.shape
    aw = orc.pad_dim(w) if aw is None else aw
    ah = orc.pad_dim(h) if ah is None else ah
    assert aw - w <= w and ah - h <= h
    out = np.empty((ah, aw), img.dtype)
    out[:h, :w] = img
    out[:h, w:] = img[:, ::-1][:, :aw - w]
    out[h:] = out[:h][::-1][:ah - h]
    return out


def inputs(kind, bd, wl, w=W, h=H):
    """The issue's inputs: `noise`, `saw`, `smooth`; rng = default_rng(7 bd + wl); uint16 (h, w)."""
    rng = np.random.default_rng(7 * bd + wl)
    mx = (1 << bd) - 1
    a = max(1, mx >> 5)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        v = rng.integers(0, mx + 1, (h, w))
    elif kind == "saw":
        v = np.clip(((37 * x + 53 * y) % (mx + 1)) + rng.integers(-a, a + 1, (h, w)), 0, mx)
    elif kind == "smooth":
        v = np.clip((mx * (0.5 + 0.45 * np.sin(x / 17.0) * np.cos(y / 23.0))).astype(np.int64) + rng.integers(-a, a + 1, (h, w)), 0, mx)
    else:
        raise ValueError(kind)
    return v.astype(np.uint16)


def level_shift(padded_u16, bd, lossy):
    off = 1 << (bd - 1)
    if lossy:
        return padded_u16.astype(np.float32) - np.float32(off)
    return padded_u16.astype(np.int32) - np.int32(off)


def clamp(x, bd):
    """5/3: clamp(x + off, 0, 2^bd - 1); 9/7: clamp(rint((x + off) + 0.01f), 0, 2^bd - 1) in float32, NaN -> 0."""
    off, mx = 1 << (bd - 1), (1 << bd) - 1
    if x.dtype == np.float32:
        t = (x + np.float32(off)) + np.float32(0.01)
        r = np.clip(np.nan_to_num(np.rint(t), nan=0.0), 0.0, float(mx))
        return r.astype(np.uint16)
    return np.clip(x.astype(np.int64) + off, 0, mx).astype(np.uint16)


def forward(padded_u16, bd, wl, lossy, qs=1.0):
    """The flat P + extra buffer of orc.dwt_forward over the level-shifted samples."""
    return orc.dwt_forward(level_shift(padded_u16, bd, lossy), wl, qs)


def header(w, h, bd, wl, lossy, qs=1.0, k=0.0, frames=0):
    return orc.header_pack(n_samples=w * h, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=bd, lossy=int(lossy),
                           qs_1e4=int(qs * 10000), components=1, is_rgb=0, height=h, endianess=0, bps=bd, is_signed=0,
                           frames=frames, k_1e3=int(k * 1000))


_enc = {}       # computed once per case, never modified


def encode(kind, bd, wl, lossy, qs=1.0, k=0.0, with_header=True):
    """(visible uint16 frame, padded frame, Mallat coefficients (AH, AW), sizes, stream) of an input of the issue."""
    key = (kind, bd, wl, lossy, qs, k, with_header)
    if key not in _enc:
        img = inputs(kind, bd, wl)
        pad = mirror_pad(img)
        ah, aw = pad.shape
        coef = forward(pad, bd, wl, lossy, qs)[:aw * ah].reshape(ah, aw)
        lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
        st, sz = orc.bpc_encode(coef, wl, lut, k=k)
        stream = orc.bitstream_pack(st, sz, header(img.shape[1], img.shape[0], bd, wl, lossy, qs, k) if with_header else None)
        for a in (img, pad, coef, sz, stream):
            a.setflags(write=False)
        _enc[key] = (img, pad, coef, sz, stream)
    return _enc[key]


def max_coef(coef):
    return int(np.abs(np.trunc(coef)).max())


def decode_coefficients(stream, aw, ah, wl, lossy, k=0.0):
    lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
    st, sz = orc.bitstream_unpack(stream, (aw // 64) * (ah // 64))
    return orc.bpc_decode(st, sz, aw, ah, wl, lut, k=k)


def inverse(coef_i32, bd, wl, lossy, qs=1.0):
    """The padded uint16 frame of an (AH, AW) int32 Mallat array."""
    ah, aw = coef_i32.shape
    out, extra = orc.dwt_inverse(coef_i32, wl, lossy, qs)
    return clamp(out[extra:].reshape(ah, aw), bd)


def decode(stream, bd, wl, lossy, qs=1.0, k=0.0, aw=AW, ah=AH):
    return inverse(decode_coefficients(stream, aw, ah, wl, lossy, k), bd, wl, lossy, qs)


# the in-range rows of the issue's table: (lossy, bd, kind, wl, qs, raw codeblocks)
IN_RANGE = [
    (False, 9, "saw", 2, 1.0, 0), (False, 10, "saw", 5, 1.0, 0), (False, 12, "saw", 5, 1.0, 0), (False, 14, "saw", 5, 1.0, 0),
    (False, 12, "noise", 5, 1.0, 9),
    (True, 10, "saw", 3, 1.0, 0), (True, 12, "saw", 3, 1.0, 0), (True, 12, "smooth", 3, 1.0, 0), (True, 14, "saw", 3, 0.25, 0),
    (True, 16, "noise", 3, 0.25, 12),
]
# out of range on purpose (the range flag; emulator only)
OUT_OF_RANGE = [(False, 16, "noise", 5, 1.0), (True, 14, "saw", 3, 1.0)]


def check_precondition(coef, sizes, raw):
    """What every coder-level test asserts on the oracle alone first."""
    assert max_coef(coef) < 32768
    assert int((np.asarray(sizes) == 4096).sum()) == raw
