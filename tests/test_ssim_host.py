"""Host-side SSIM calls of the C ABI (no GPU): picsong_ssim_windows, picsong_ssim_to_dssim and picsong_dssim_to_ssim
against the reference model (ssim_ref.py), and their refusals."""
import ctypes as C

import picsong_amd as pa
import ssim_ref as sr

ERR_ARG = -1


def test_windows():
    for w, h in ((8, 8), (11, 15), (33, 32), (200, 136), (203, 139), (1100, 40), (7680, 4320), (16384, 16384)):
        assert pa.ssim_windows(w, h) == sr.windows(w, h), (w, h)
    assert pa.ssim_windows(8, 8) == 1 and pa.ssim_windows(12, 8) == 2 and pa.ssim_windows(200, 136) == 1617


def test_ssim_to_dssim_is_the_models():
    for windows in (1, 49, 1617, 3 * 1617, 3 * 4503, 1919 * 1079 * 63):
        for ssim in (1.0, 0.999, 0.98, 0.95, 0.9, 0.5, 0.1, 0.0, -0.25, -1.0, 0.123456789):
            assert pa.ssim_to_dssim(ssim, windows) == sr.ssim_to_dssim(ssim, windows), (ssim, windows)
    assert pa.ssim_to_dssim(0.98, 1617) == 542575165 and pa.ssim_to_dssim(0.90, 3713) == 6229380300
    assert pa.ssim_to_dssim(1.0, 77) == 0 and pa.ssim_to_dssim(0.0, 77) == 77 << 24 and pa.ssim_to_dssim(-1.0, 77) == 154 << 24


def test_dssim_to_ssim_is_the_models():
    for windows in (1, 1617, 3 * 4503):
        for d in (0, 1, 12345, windows << 23, windows << 24, (windows << 24) + 999, windows << 25):
            assert pa.dssim_to_ssim(d, windows) == sr.dssim_to_ssim(d, windows), (d, windows)
    assert pa.dssim_to_ssim(0, 9) == 1.0 and pa.dssim_to_ssim(9 << 24, 9) == 0.0 and pa.dssim_to_ssim(9 << 25, 9) == -1.0
    # the two are inverse to each other up to the floor
    lim = pa.ssim_to_dssim(0.98, 1617)
    assert pa.dssim_to_ssim(lim, 1617) >= 0.98 - 1e-12 > pa.dssim_to_ssim(lim + 1617, 1617)


def test_refusals():
    L = pa.load()
    s, d = C.c_uint64(77), C.c_double(77.0)
    for w, h in ((7, 8), (8, 7), (0, 100), (-5, 100), (100, -5), (7, 7)):
        assert L.picsong_ssim_windows(w, h, C.byref(s)) == ERR_ARG, (w, h)
    assert L.picsong_ssim_windows(8, 8, None) == ERR_ARG
    assert L.picsong_ssim_to_dssim(0.9, 100, None) == ERR_ARG
    assert L.picsong_ssim_to_dssim(0.9, 0, C.byref(s)) == ERR_ARG
    for bad in (1.0000001, -1.0000001, float("nan"), float("inf"), float("-inf")):
        assert L.picsong_ssim_to_dssim(bad, 100, C.byref(s)) == ERR_ARG, bad
    assert L.picsong_dssim_to_ssim(5, 100, None) == ERR_ARG
    assert L.picsong_dssim_to_ssim(5, 0, C.byref(d)) == ERR_ARG
    assert s.value == 77 and d.value == 77.0                     # outputs untouched
