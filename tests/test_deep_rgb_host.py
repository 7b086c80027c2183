"""Deep RGB contexts (bit_depth 9..16, components 3, is_rgb 1): the host-side functions, no GPU -- the range rule
picsong_depth_range_guaranteed_rgb, the header of such a context, and the reference's own colour transforms."""
import ctypes as C

import numpy as np

import deep_rgb_ref as R
import picsong_amd as pa


def test_depth_range_guaranteed_rgb():
    # 5/3: the RCT's chroma differences span +-(2^bd - 1): max|sample| = 2^bd, 2^bd x 2.8601^2 + 64 < 30000 up to bd = 11
    for wl in (1, 5, 7):
        got = [pa.depth_range_guaranteed_rgb(bd, False, wl) for bd in range(9, 17)]
        assert got == [(1 << bd) * 2.8601 * 2.8601 + 64.0 < 30000.0 for bd in range(9, 17)] == [True] * 3 + [False] * 5
        # ... which is the grey rule one bit deeper
        assert got[:7] == [pa.depth_range_guaranteed(bd + 1, False, wl) for bd in range(9, 16)]
    # 9/7: the ICT's rows have absolute sum 1, so max|sample| = 2^(bd-1): the grey rule of that depth
    for bd in range(9, 17):
        for wl, qs in ((3, 1.0), (3, 0.25), (7, 1.0), (5, 0.5), (1, 0.05)):
            assert pa.depth_range_guaranteed_rgb(bd, True, wl, qs) == pa.depth_range_guaranteed(bd, True, wl, qs), (bd, wl, qs)
    assert pa.depth_range_guaranteed_rgb(10, True, 3, 0.25) and not pa.depth_range_guaranteed_rgb(16, True, 3, 1.0)
    L = pa.load()
    yes = C.c_int(7)
    assert L.picsong_depth_range_guaranteed_rgb(12, 0, 5, 1.0, None) == -1
    # what the grey helper refuses, and bit_depth 8
    for bd, lossy, wl, qs in ((7, 0, 5, 1.0), (8, 0, 5, 1.0), (8, 1, 3, 0.5), (17, 0, 5, 1.0), (12, 0, 0, 1.0), (12, 0, 8, 1.0),
                              (12, 1, 5, 0.0), (12, 1, 5, 1.5)):
        assert L.picsong_depth_range_guaranteed_rgb(bd, lossy, wl, qs, C.byref(yes)) == -1, (bd, lossy, wl, qs)
    assert yes.value == 7, "a refused call leaves *yes alone"
    assert b"depth_range_guaranteed_rgb" in L.picsong_last_error()


def test_depth_range_rgb_ignores_the_coefficient_form_switch(monkeypatch):
    monkeypatch.setenv("PICSONG_C16", "0")
    assert pa.depth_range_guaranteed_rgb(11, False, 5)


def test_header_of_a_deep_rgb_context(oracle):
    p = pa.make_params(200, 136, wl=5, lossy=True, qs=0.25, frames=3, bit_depth=12, rgb=True)
    s = pa.header_pack(p)
    ref = oracle.header_pack(n_samples=200 * 136 * 3, cp=2, cb_height=18, cb_width=64, wl=5, bit_depth=12, lossy=1, qs_1e4=2500,
                             components=3, is_rgb=1, height=136, endianess=0, bps=12, is_signed=0, frames=3, k_1e3=0)
    assert np.array_equal(s, ref)
    assert np.array_equal(s, R.header(200, 136, 12, 5, True, 0.25, frames=3))
    assert (int(s[3]) >> 3) & 127 == 12 and (int(s[6]) >> 9) & 31 == 12
    q = pa.header_unpack(s)
    assert (q.width, q.height, q.wl, q.lossy, q.bit_depth, q.frames, q.components, q.is_rgb) == (200, 136, 5, 1, 12, 3, 3, 1)
    assert np.array_equal(pa.header_pack(q)[:8], s[:8])
    h = oracle.header_unpack(s)
    assert h["bit_depth"] == 12 and h["bps"] == 12 and h["components"] == 3 and h["is_rgb"] == 1


def test_the_reference_transforms_at_8_bits_are_the_oracles(oracle):
    """deep_rgb_ref's numpy RCT / ICT and their inverses with bd = 8 against the CPU oracle's 8-bit ones, bit for bit."""
    rng = np.random.default_rng(3)
    r, g, b = (rng.integers(0, 256, (64, 64)).astype(np.uint8) for _ in range(3))
    for lossy in (False, True):
        want = oracle.rgb_forward(r, g, b, lossy)
        got = R.forward(r, g, b, 8, lossy)
        for k in range(3):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (lossy, k)
        comp = [(w.astype(np.float64) * 1.25).astype(w.dtype) for w in want]          # (both clamp ends occur)
        back, ref = R.inverse(comp[0], comp[1], comp[2], 8), oracle.rgb_inverse(*comp)
        for k in range(3):
            assert np.array_equal(back[k], ref[k]), (lossy, k)
        assert min(x.min() for x in back) == 0 and max(x.max() for x in back) == 255


def test_the_reference_round_trip_is_exact_for_5_3():
    for bd in (9, 12, 16):
        planes = [R.inputs("noise", bd, 3, c, 64, 64) for c in range(3)]
        planes[0][0, :2] = [0, (1 << bd) - 1]
        comp = R.forward(planes[0], planes[1], planes[2], bd, False)
        assert max(int(np.abs(c).max()) for c in comp[1:]) <= (1 << bd) - 1
        back = R.inverse(comp[0], comp[1], comp[2], bd)
        assert all(np.array_equal(back[c], planes[c]) for c in range(3))
