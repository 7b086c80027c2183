"""Deep contexts (bit_depth 9..16): the host-side functions, no GPU -- the mirror padding on 2-byte samples, the header's two
depth fields, and the range rule picsong_depth_range_guaranteed."""
import ctypes as C

import numpy as np
import pytest

import deep_ref as D
import picsong_amd as pa


@pytest.mark.parametrize("w,h", [(201, 137), (33, 40), (192, 128)])
def test_pad_frame16_is_the_numpy_mirror(w, h):
    img = np.random.default_rng(w).integers(0, 65536, (h, w)).astype(np.uint16)
    aw, ah = pa.pad_dim(w), pa.pad_dim(h)
    assert np.array_equal(pa.pad_frame16(img, aw, ah), D.mirror_pad(img, aw, ah))


def test_pad_frame16_refusals():
    L = pa.load()
    img = np.zeros((40, 31), np.uint16)
    out = np.full((64, 64), 0x5A5A, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.picsong_pad_frame16_host(p(img), 31, 40, p(out), 64, 64) == -1          # aw - w = 33 > w = 31
    assert b"more columns" in L.picsong_last_error()
    assert L.picsong_pad_frame16_host(p(img[:31, :]), 31, 31, p(out), 32, 64) == -1      # ah - h = 33 > h
    assert L.picsong_pad_frame16_host(None, 31, 40, p(out), 64, 64) == -1
    assert L.picsong_pad_frame16_host(p(img), 31, 40, p(out), 30, 64) == -1
    assert (out == 0x5A5A).all(), "a refused call writes nothing"


def test_header_carries_the_depth_twice(oracle):
    p = pa.make_params(200, 136, wl=5, lossy=True, qs=0.25, frames=3, bit_depth=12)
    s = pa.header_pack(p)
    ref = oracle.header_pack(n_samples=200 * 136, cp=2, cb_height=18, cb_width=64, wl=5, bit_depth=12, lossy=1, qs_1e4=2500,
                             components=1, is_rgb=0, height=136, endianess=0, bps=12, is_signed=0, frames=3, k_1e3=0)
    assert np.array_equal(s, ref)
    assert (int(s[3]) >> 3) & 127 == 12 and (int(s[6]) >> 9) & 31 == 12
    q = pa.header_unpack(s)
    assert (q.width, q.height, q.wl, q.lossy, q.bit_depth, q.frames, q.components, q.is_rgb) == (200, 136, 5, 1, 12, 3, 1, 0)
    assert np.array_equal(pa.header_pack(q)[:8], s[:8])
    h = oracle.header_unpack(s)
    assert h["bit_depth"] == 12 and h["bps"] == 12


def test_depth_range_guaranteed():
    for wl in (1, 5, 7):
        assert [pa.depth_range_guaranteed(bd, False, wl) for bd in range(9, 17)] == [True] * 4 + [False] * 4
    assert pa.depth_range_guaranteed(8, False, 5)
    # 9/7: the bound grows with wl and qs -- 8-bit samples at qs = 1 fit three levels, 16-bit ones never at qs = 1
    assert pa.depth_range_guaranteed(8, True, 3, 1.0)
    assert not pa.depth_range_guaranteed(16, True, 3, 1.0)
    assert pa.depth_range_guaranteed(10, True, 3, 0.25) and not pa.depth_range_guaranteed(10, True, 7, 1.0)
    L = pa.load()
    yes = C.c_int(7)
    assert L.picsong_depth_range_guaranteed(12, 0, 5, 1.0, None) == -1
    for bd, lossy, wl, qs in ((7, 0, 5, 1.0), (17, 0, 5, 1.0), (12, 0, 0, 1.0), (12, 0, 8, 1.0), (12, 1, 5, 0.0), (12, 1, 5, 1.5)):
        assert L.picsong_depth_range_guaranteed(bd, lossy, wl, qs, C.byref(yes)) == -1, (bd, lossy, wl, qs)
    assert yes.value == 7, "a refused call leaves *yes alone"


def test_depth_range_ignores_the_coefficient_form_switch(monkeypatch):
    monkeypatch.setenv("PICSONG_C16", "0")
    assert pa.depth_range_guaranteed(12, False, 5)
