"""Expected output of the reduced-quality decode (picsong_ctx_set_decode_drop), from the CPU oracle alone.
TEST INFRASTRUCTURE ONLY.  The oracle decodes every plane; `truncate` then states the semantics in numpy: codeblock cb,
whose top-left sample lies in level lv (0 the finest, wl the LL band), keeps the planes above d = max(0, drop - lv) of its
magnitudes; a coefficient with a bit left gets the midpoint 1 << (d - 1) below them, every other one is 0; raw codeblocks
(length 4096) stay whole.  Everything after the coder is the oracle's own."""
import numpy as np

import oracle_lib as orc


def cb_level(AW, AH, wl, cb):
    """The level of raster codeblock cb's top-left sample: the smallest a in 1..wl with x >= AW >> a or y >= AH >> a gives
    a - 1; none: wl (the LL band)."""
    ncx = AW // 64
    x, y = (cb % ncx) * 64, (cb // ncx) * 64
    for a in range(1, wl + 1):
        if x >= (AW >> a) or y >= (AH >> a):
            return a - 1
    return wl


def drop_planes(AW, AH, wl, drop, cb):
    return max(0, drop - cb_level(AW, AH, wl, cb))


def truncate(coef, sizes, AW, AH, wl, drop):
    """`coef`: the (AH, AW) int32 Mallat array of the full decode; `sizes`: the codeblocks' lengths.  Returns the array the
    decode under `drop` gives."""
    out = np.array(coef, np.int32).reshape(AH, AW).copy()
    ncx = AW // 64
    for cb in range(ncx * (AH // 64)):
        d = drop_planes(AW, AH, wl, drop, cb)
        if d == 0 or sizes[cb] == 4096:
            continue
        ys, xs = (cb // ncx) * 64, (cb % ncx) * 64
        blk = out[ys:ys + 64, xs:xs + 64].astype(np.int64)
        m = np.abs(blk)
        kept = (m >> d) << d
        m = np.where(kept != 0, kept | (1 << (d - 1)), 0)
        out[ys:ys + 64, xs:xs + 64] = (np.sign(blk) * m).astype(np.int32)
    return out


_full = {}      # the oracle's full decode of a stream, computed once: (coefficients, sizes), never modified


def full_decode(stream, AW, AH, wl, lut):
    stream = np.ascontiguousarray(stream, np.uint16)
    key = (hash(stream.tobytes()), stream.size, AW, AH, wl, hash(lut.table.tobytes()))
    if key not in _full:
        st, sz = orc.bitstream_unpack(stream, (AW // 64) * (AH // 64))
        coef = orc.bpc_decode(st, sz, AW, AH, wl, lut)
        coef.setflags(write=False)
        sz.setflags(write=False)
        _full[key] = (coef, sz)
    return _full[key]


def drop_coefficients(stream, AW, AH, wl, lut, drop):
    """The (AH, AW) int32 coefficients a component's codestream decodes to under `drop`."""
    coef, sz = full_decode(stream, AW, AH, wl, lut)
    return truncate(coef, sz, AW, AH, wl, drop)


def drop_ll(stream, AW, AH, wl, lossy, qs, lut, drop, r=0):
    """LL_r of the decode under `drop`, before the level shift (reduced_ref.coded_ll with the truncation in it)."""
    out, extra = orc.dwt_inverse(drop_coefficients(stream, AW, AH, wl, lut, drop), wl, lossy, qs)
    o = extra - orc.dwt_extra(AW, AH, r + 1)
    return out[o:o + (AW >> r) * (AH >> r)].reshape(AH >> r, AW >> r)


def drop_pixels(stream, AW, AH, wl, lossy, qs, lut, drop, r=0):
    """The grey image at 1/2^r under `drop`, padded: uint8 (AH >> r, AW >> r)."""
    return orc.level_shift_inv(drop_ll(stream, AW, AH, wl, lossy, qs, lut, drop, r)).astype(np.uint8)


def drop_rgb(streams, AW, AH, wl, lossy, qs, luts, drop, r=0):
    """The RGB image at 1/2^r under `drop`: three uint8 (AH >> r, AW >> r)."""
    return orc.rgb_inverse(*[drop_ll(s, AW, AH, wl, lossy, qs, lut, drop, r) for s, lut in zip(streams, luts)])


def drop_window(stream, AW, AH, wl, lossy, qs, lut, drop, r, x, y, w, h):
    return drop_pixels(stream, AW, AH, wl, lossy, qs, lut, drop, r)[y:y + h, x:x + w]


def drop_window_rgb(streams, AW, AH, wl, lossy, qs, luts, drop, r, x, y, w, h):
    return [p[y:y + h, x:x + w] for p in drop_rgb(streams, AW, AH, wl, lossy, qs, luts, drop, r)]
