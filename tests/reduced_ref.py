"""Expected output of the reduced-resolution decode (picsong_decode_frame_reduced and its mirrors), from the CPU oracle.
TEST INFRASTRUCTURE ONLY.  The oracle's inverse transform keeps every intermediate LL packed in its output buffer, as
the reference's DWTDecode does: LL_r starts at dwt_extra(AW, AH, wl) - dwt_extra(AW, AH, r + 1) and holds
(AW >> r) x (AH >> r) samples."""
import numpy as np

import oracle_lib as orc


def coded_ll(stream, AW, AH, wl, lossy, qs, lut, r, k=0.0):
    """LL_r of a component's codestream, before the level shift: (AH >> r, AW >> r) int32 (5/3) or float32 (9/7)."""
    st, sz = orc.bitstream_unpack(stream, (AW // 64) * (AH // 64))
    coef = orc.bpc_decode(st, sz, AW, AH, wl, lut, k=k)
    out, extra = orc.dwt_inverse(coef, wl, lossy, qs)
    o = extra - orc.dwt_extra(AW, AH, r + 1)
    return out[o:o + (AW >> r) * (AH >> r)].reshape(AH >> r, AW >> r)


def reduced_pixels(stream, AW, AH, wl, lossy, qs, lut, r, k=0.0):
    """The grey reduced image, padded: the level-shifted, clamped LL_r as uint8 (AH >> r, AW >> r)."""
    return orc.level_shift_inv(coded_ll(stream, AW, AH, wl, lossy, qs, lut, r, k)).astype(np.uint8)


def reduced_rgb(streams, AW, AH, wl, lossy, qs, luts, r, k=0.0):
    """The RGB reduced image: the inverse RCT / ICT of the three components' LL_r, three uint8 (AH >> r, AW >> r)."""
    ll = [coded_ll(s, AW, AH, wl, lossy, qs, lut, r, k) for s, lut in zip(streams, luts)]
    return orc.rgb_inverse(*ll)


def visible(W, H, r):
    """ceil(W / 2^r) x ceil(H / 2^r): the part of the padded reduced image that shows the frame."""
    return -(-W // (1 << r)), -(-H // (1 << r))
