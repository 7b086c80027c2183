"""Expected output of the deep proxy calls (picsong_decode_frames16_reduced / _window, picsong_decode_rgb_frames16_reduced /
_window and the 16-bit layouts of the image proxy calls), composed from reduced_ref, window_ref's slicing, deep_ref and
deep_rgb_ref -- the CPU oracle's stage functions between numpy ends.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import deep_ref as D
import deep_rgb_ref as R
import drop_ref as dr
import oracle_lib as orc
import reduced_ref as rr

AW, AH = D.AW, D.AH


def _ll_of(coef, wl, lossy, qs, r):
    """LL_r of an (AH, AW) int32 Mallat array, before the level shift (reduced_ref.coded_ll's slice)."""
    ah, aw = coef.shape
    out, extra = orc.dwt_inverse(coef, wl, lossy, qs)
    o = extra - orc.dwt_extra(aw, ah, r + 1)
    return np.ascontiguousarray(out[o:o + (aw >> r) * (ah >> r)].reshape(ah >> r, aw >> r))


def grey_reduced(stream, bd, wl, lossy, qs, r, k=0.0, drop=0, aw=AW, ah=AH):
    """The padded reduced frame, uint16 (ah >> r, aw >> r): deep_ref.clamp of reduced_ref.coded_ll; under `drop` the
    coefficients follow drop_ref's rule."""
    lut = orc.lut_for_k(lossy, wl) if k > 0 else orc.lut_for(lossy, wl)
    if drop:
        return D.clamp(dr.drop_ll(stream, aw, ah, wl, lossy, qs, lut, drop, r), bd)
    return D.clamp(rr.coded_ll(stream, aw, ah, wl, lossy, qs, lut, r, k), bd)


def rgb_reduced(streams, bd, wl, lossy, qs, r, k=0.0, drop=0, aw=AW, ah=AH):
    """The three padded reduced planes: deep_rgb_ref.inverse of the components' LL_r, component c with table c."""
    if drop:
        ll = [np.ascontiguousarray(dr.drop_ll(streams[c], aw, ah, wl, lossy, qs, R.lut(lossy, wl, c, k), drop, r)) for c in range(3)]
    else:
        ll = [np.ascontiguousarray(rr.coded_ll(streams[c], aw, ah, wl, lossy, qs, R.lut(lossy, wl, c, k), r, k)) for c in range(3)]
    return R.inverse(ll[0], ll[1], ll[2], bd)


def window(planes, x, y, w, h):
    """A window is a slice of the reduced output."""
    if isinstance(planes, (list, tuple)):
        return [p[y:y + h, x:x + w] for p in planes]
    return planes[y:y + h, x:x + w]


def synthesis_grey(coef, bd, wl, lossy, qs, r):
    """... of a hand-built Mallat array: the oracle's inverse, then deep_ref.clamp."""
    return D.clamp(_ll_of(coef, wl, lossy, qs, r), bd)


def synthesis_rgb(coefs, bd, wl, lossy, qs, r):
    ll = [_ll_of(c, wl, lossy, qs, r) for c in coefs]
    return R.inverse(ll[0], ll[1], ll[2], bd)


def interleave(planes, layout_spp, alpha):
    """(h, w, spp) uint16 pixels of three planes; spp = 4: alpha in the fourth sample."""
    h, w = planes[0].shape
    px = np.empty((h, w, layout_spp), np.uint16)
    for c in range(3):
        px[:, :, c] = planes[c]
    if layout_spp == 4:
        px[:, :, 3] = alpha
    return px
