"""Expected output of the window decode (picsong_decode_frame_window and its mirrors), from the CPU oracle, and an
independent restatement of the rule that picks the window's codeblocks.  TEST INFRASTRUCTURE ONLY."""
import reduced_ref as rr


def window_pixels(stream, AW, AH, wl, lossy, qs, lut, r, x, y, w, h, k=0.0):
    """The grey window: rows [y, y + h), columns [x, x + w) of the reduced image at 1/2^r."""
    return rr.reduced_pixels(stream, AW, AH, wl, lossy, qs, lut, r, k)[y:y + h, x:x + w]


def window_rgb(streams, AW, AH, wl, lossy, qs, luts, r, x, y, w, h, k=0.0):
    return [p[y:y + h, x:x + w] for p in rr.reduced_rgb(streams, AW, AH, wl, lossy, qs, luts, r, k)]


def window_codeblocks(AW, AH, wl, lossy, r, x, y, w, h):
    """The set of (cx, cy) codeblocks the window [x, x + w) x [y, y + h) of LL_r depends on: per synthesis level
    l = r .. wl - 1 the subband rectangle S_l of R_l (R_r the window, R_{l+1} = S_l), per axis
    [max(0, a // 2 - e), min(K, ceil(b / 2) + e)), e = 1 (5/3) or 2 (9/7); the codeblocks meeting S_l moved to HL, LH
    and HH of level l, and S_{wl-1} itself (LL_wl)."""
    e = 2 if lossy else 1
    cbs = set()

    def add(x0, y0, x1, y1):
        for cy in range(y0 // 64, -(-y1 // 64)):
            for cx in range(x0 // 64, -(-x1 // 64)):
                cbs.add((cx, cy))

    rx, ry = (x, x + w), (y, y + h)
    for l in range(r, wl):
        hw, hh = (AW >> l) // 2, (AH >> l) // 2
        sx = (max(0, rx[0] // 2 - e), min(hw, -(-rx[1] // 2) + e))
        sy = (max(0, ry[0] // 2 - e), min(hh, -(-ry[1] // 2) + e))
        add(sx[0] + hw, sy[0], sx[1] + hw, sy[1])
        add(sx[0], sy[0] + hh, sx[1], sy[1] + hh)
        add(sx[0] + hw, sy[0] + hh, sx[1] + hw, sy[1] + hh)
        if l == wl - 1:
            add(sx[0], sy[0], sx[1], sy[1])
        rx, ry = sx, sy
    return cbs


def windows(paw, pah, W=None, H=None, ncx_straddle=None):
    """Windows of a paw x pah padded reduced image: every corner and edge, the centre, 1 x 1, odd x / y / w / h, one
    reaching into the padding (W, H: the visible size), the whole image."""
    cw, ch = max(1, min(37, paw // 3)), max(1, min(29, pah // 3))
    out = [(0, 0, cw, ch), (paw - cw, 0, cw, ch), (0, pah - ch, cw, ch), (paw - cw, pah - ch, cw, ch),
           ((paw - cw) // 2, 0, cw, ch), ((paw - cw) // 2, pah - ch, cw, ch), (0, (pah - ch) // 2, cw, ch),
           (paw - cw, (pah - ch) // 2, cw, ch), ((paw - cw) // 2, (pah - ch) // 2, cw, ch), (paw // 2, pah // 3, 1, 1),
           (min(3, paw - 1), min(5, pah - 1), min(17, paw - min(3, paw - 1)), min(11, pah - min(5, pah - 1))),
           (0, 0, paw, pah)]
    if W is not None and (W < paw or H < pah):
        out.append((max(0, W - 9), max(0, H - 7), paw - max(0, W - 9), pah - max(0, H - 7)))
    return out
