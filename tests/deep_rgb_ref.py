"""Expected output of the deep RGB contexts (bit_depth 9..16, components 3, is_rgb 1: three uint16 planes a frame), composed
from deep_ref.py / the CPU oracle's STAGE functions between a numpy colour transform and a numpy inverse.  TEST
INFRASTRUCTURE ONLY.  The oracle's colour transforms are 8-bit; here they are numpy on 16-bit samples, and everything
between (transform, coder, pack) is the oracle's own, a component at a time with table c.

Forward ICT.  c = fmaf(m2, B', fmaf(m1, G', m0 * R')) in float32.  Here every step is m * x + t in float64 followed by ONE
rounding to float32, which is exactly fmaf: m is a float32 of magnitude >= 2^-4, so a multiple of 2^-27; x is an integer
below 2^17; t is a float32 that was itself rounded from a multiple of 2^-27 and so is one (rounding to float32 moves a
value to a coarser or equal grid, never a finer one that the value does not lie on).  Product and sum are therefore
multiples of 2^-27 below 2^18: at most 45 significant bits, exact in float64's 53.

Inverse ICT.  Its inputs are arbitrary floats (the synthesis' output), where float64 emulation can double-round; it uses
the true fmaf of libm through a few lines of C that this file builds with the host compiler."""
import ctypes as C
import os
import subprocess

import numpy as np

import deep_ref as D
import oracle_lib as orc

W, H, AW, AH = D.W, D.H, D.AW, D.AH

M_FWD = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], np.float32)
M_INV = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], np.float32)

_FMAF_C = """
#include <math.h>
#include <stddef.h>
void fmaf_n(const float *a, const float *b, const float *c, float *out, size_t n)
{
    for (size_t i = 0; i < n; i++) out[i] = fmaf(a[i], b[i], c[i]);
}
"""
_fmaf_lib = None


def _fmaf(a, b, c):
    """fmaf(a, b, c) element by element: libm's, one rounding."""
    global _fmaf_lib
    if _fmaf_lib is None:
        out_dir = os.path.join(orc.ROOT, "tests", "hipemu", "_build")
        so = os.path.join(out_dir, "libdeep_rgb_fmaf.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(__file__):
            os.makedirs(out_dir, exist_ok=True)
            tmp = f"{so}.{os.getpid()}"                      # (several test processes may build it at once)
            subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, "-x", "c", "-", "-lm"],
                           input=_FMAF_C.encode(), check=True)
            os.replace(tmp, so)
        _fmaf_lib = C.CDLL(so)
        # is it fused?  (1 + 2^-12)^2 - 1 = 2^-11 + 2^-24 exactly; a product rounded to float32 first loses the 2^-24
        x = np.array([1.0 + 2.0 ** -12], np.float32)
        assert _fmaf_run(x, x, np.array([-1.0], np.float32))[0] == np.float32(2.0 ** -11 + 2.0 ** -24)
    return _fmaf_run(a, b, c)


def _fmaf_run(a, b, c):
    a, b, c = (np.ascontiguousarray(np.broadcast_to(x, np.broadcast(a, b, c).shape), np.float32) for x in (a, b, c))
    out = np.empty(a.shape, np.float32)
    _fmaf_lib.fmaf_n(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                     out.ctypes.data_as(C.c_void_p), C.c_size_t(a.size))
    return out


def inputs(kind, bd, wl, c, w=W, h=H):
    """Plane c of an input of the issue: deep_ref.inputs' formula with rng = default_rng(7 bd + wl + 1000 c) and x, y
    shifted by 11 c, 7 c; uint16 (h, w)."""
    rng = np.random.default_rng(7 * bd + wl + 1000 * c)
    mx = (1 << bd) - 1
    a = max(1, mx >> 5)
    y, x = np.mgrid[0:h, 0:w]
    x, y = x + 11 * c, y + 7 * c
    if kind == "noise":
        v = rng.integers(0, mx + 1, (h, w))
    elif kind == "saw":
        v = np.clip(((37 * x + 53 * y) % (mx + 1)) + rng.integers(-a, a + 1, (h, w)), 0, mx)
    elif kind == "smooth":
        v = np.clip((mx * (0.5 + 0.45 * np.sin(x / 17.0) * np.cos(y / 23.0))).astype(np.int64) + rng.integers(-a, a + 1, (h, w)), 0, mx)
    else:
        raise ValueError(kind)
    return v.astype(np.uint16)


def forward(r, g, b, bd, lossy):
    """The three component planes (int32 / float32) of uint16 planes: RCT / ICT on the level-shifted samples, read unsigned."""
    off = 1 << (bd - 1)
    if not lossy:
        R, G, B = (np.asarray(x).astype(np.int64) - off for x in (r, g, b))
        return [((R + 2 * G + B) >> 2).astype(np.int32), (B - G).astype(np.int32), (R - G).astype(np.int32)]
    R, G, B = (np.asarray(x).astype(np.float64) - float(off) for x in (r, g, b))
    m = M_FWD.astype(np.float64)
    out = []
    for k in range(3):
        t = (m[k, 0] * R).astype(np.float32)
        t = (m[k, 1] * G + t.astype(np.float64)).astype(np.float32)
        t = (m[k, 2] * B + t.astype(np.float64)).astype(np.float32)
        out.append(t)
    return out


def inverse(c0, c1, c2, bd):
    """The three uint16 planes of component planes: inverse RCT / ICT, level shift, clamp to [0, 2^bd - 1]."""
    off, mx = 1 << (bd - 1), (1 << bd) - 1
    if c0.dtype != np.float32:
        y, cb, cr = (np.asarray(x).astype(np.int64) for x in (c0, c1, c2))
        G = y - ((cb + cr) >> 2)
        return [np.clip(v + off, 0, mx).astype(np.uint16) for v in (cr + G, G, cb + G)]
    out = []
    for k in range(3):
        t = M_INV[k, 0] * c0                                     # (float32 * float32: one rounding)
        t = _fmaf(M_INV[k, 1], c1, t)
        t = _fmaf(M_INV[k, 2], c2, t)
        x = np.rint(t + np.float32(0.01)).astype(np.int64)
        out.append(np.clip(x + off, 0, mx).astype(np.uint16))
    return out


def header(w, h, bd, wl, lossy, qs=1.0, k=0.0, frames=0):
    return orc.header_pack(n_samples=w * h * 3, cp=2, cb_height=18, cb_width=64, wl=wl, bit_depth=bd, lossy=int(lossy),
                           qs_1e4=int(qs * 10000), components=3, is_rgb=1, height=h, endianess=0, bps=bd, is_signed=0,
                           frames=frames, k_1e3=int(k * 1000))


def lut(lossy, wl, c, k=0.0):
    return orc.lut_for_component(lossy, wl, c, k=k)


_enc = {}       # computed once per case, never modified


def encode(kind, bd, wl, lossy, qs=1.0, k=0.0, header_mask=7):
    """(visible planes [3], padded planes [3], component planes [3], Mallat coefficients [3] (AH, AW), sizes [3],
    streams [3]) of an input of the issue; the populated header on the components of header_mask."""
    key = (kind, bd, wl, lossy, qs, k, header_mask)
    if key not in _enc:
        img = [inputs(kind, bd, wl, c) for c in range(3)]
        pad = [D.mirror_pad(x) for x in img]
        comp = forward(pad[0], pad[1], pad[2], bd, lossy)
        hdr = header(W, H, bd, wl, lossy, qs, k)
        coef, sizes, streams = [], [], []
        for c in range(3):
            cf = orc.dwt_forward(np.ascontiguousarray(comp[c]), wl, qs)[:AW * AH].reshape(AH, AW)
            st, sz = orc.bpc_encode(cf, wl, lut(lossy, wl, c, k), k=k)
            coef.append(cf); sizes.append(sz)
            streams.append(orc.bitstream_pack(st, sz, hdr if header_mask >> c & 1 else None))
        for a in img + pad + comp + coef + sizes + streams:
            a.setflags(write=False)
        _enc[key] = (img, pad, comp, coef, sizes, streams)
    return _enc[key]


def decode_coefficients(stream, wl, lossy, c, k=0.0):
    """Component c's (AH, AW) int32 Mallat array of its stream (table c)."""
    st, sz = orc.bitstream_unpack(stream, (AW // 64) * (AH // 64))
    return orc.bpc_decode(st, sz, AW, AH, wl, lut(lossy, wl, c, k), k=k)


def synthesis(coefs, wl, lossy, qs=1.0):
    """The three (AH, AW) component planes of three int32 Mallat arrays."""
    out = []
    for cf in coefs:
        o, extra = orc.dwt_inverse(cf, wl, lossy, qs)
        out.append(np.ascontiguousarray(o[extra:].reshape(AH, AW)))
    return out


def decode(streams, bd, wl, lossy, qs=1.0, k=0.0):
    """The three padded uint16 planes of a frame's three streams."""
    c = synthesis([decode_coefficients(streams[i], wl, lossy, i, k) for i in range(3)], wl, lossy, qs)
    return inverse(c[0], c[1], c[2], bd)


def max_coef(coef):
    return [D.max_coef(c) for c in coef]


def raw_codeblocks(sizes):
    return [int((np.asarray(s) == 4096).sum()) for s in sizes]


# the in-range rows: (lossy, bd, kind, wl, qs, max|c| per component, raw codeblocks per component) -- measured with this
# generator on the CPU oracle; check_precondition holds every run to them
IN_RANGE = [
    (False, 9, "saw", 2, 1.0, (312, 576, 610), (0, 1, 0)),
    (False, 10, "saw", 5, 1.0, (725, 2498, 1956), (0, 0, 0)),
    (False, 12, "saw", 5, 1.0, (2565, 7051, 7511), (0, 0, 0)),
    (False, 12, "smooth", 5, 1.0, (2103, 1520, 1528), (0, 0, 0)),
    (False, 12, "noise", 5, 1.0, (4008, 12005, 9454), (1, 10, 8)),
    (False, 14, "saw", 5, 1.0, (7406, 2096, 2304), (0, 0, 0)),
    (True, 10, "saw", 3, 1.0, (1678, 2123, 2357), (0, 0, 0)),
    (True, 12, "saw", 3, 1.0, (11743, 13727, 14132), (0, 0, 0)),
    (True, 12, "smooth", 5, 0.5, (23139, 10229, 8814), (0, 0, 0)),
    (True, 14, "saw", 3, 0.25, (15504, 1276, 1138), (0, 0, 0)),
    (True, 16, "noise", 3, 0.25, (14222, 12828, 15359), (11, 12, 12)),
]


def row(lossy, bd, kind):
    return next(r for r in IN_RANGE if r[:3] == (lossy, bd, kind))


def row_id(r):
    return f"{'97' if r[0] else '53'}-{r[1]}-{r[2]}"
# out of range on purpose (the range flag)
OUT_OF_RANGE = [(False, 16, "noise", 5, 1.0)]


def check_precondition(coef, sizes, want_max, want_raw):
    """What every coder-level test asserts on the oracle alone first."""
    assert max(max_coef(coef)) < 32768
    assert max_coef(coef) == list(want_max) and raw_codeblocks(sizes) == list(want_raw)
