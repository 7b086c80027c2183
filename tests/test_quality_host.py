"""Host-side quality calls of the C ABI (no GPU): the PSNR <-> SSE helpers where the power of ten is exact, their
refusals, and sse = 0."""
import ctypes as C
import math

import picsong_amd as pa
import quality_ref as qr

ERR_ARG = -1


def test_psnr_to_sse_where_the_power_of_ten_is_exact():
    for samples in (1, 200 * 136, 700 * 500, 3 * 320 * 192, 7680 * 4320 * 16 * 3):
        for db in (10, 20, 30, 40, 50):
            want = 65025 * samples // 10 ** (db // 10)           # exact integer arithmetic
            assert pa.psnr_to_sse(float(db), samples) == want == qr.limit(db, samples), (db, samples)
    assert pa.psnr_to_sse(40.0, 200 * 136) == 176868 and pa.psnr_to_sse(30.0, 320 * 192) == 3995136
    assert pa.psnr_to_sse(0.0, 10) == 650250


def test_sse_to_psnr_where_the_logarithm_is_exact():
    for samples in (1, 200 * 136, 700 * 500):
        for db in (10, 20, 30, 40, 50):
            # sse = 65025 * samples / 10^(dB / 10) exactly where that is an integer: scale the samples so that it is
            s = samples * 10 ** (db // 10)
            assert pa.sse_to_psnr(65025 * samples, s) == float(db), (db, samples)
    assert pa.sse_to_psnr(65025, 1) == 0.0
    # the two are inverse to each other up to the floor
    lim = pa.psnr_to_sse(40.0, 700 * 500)
    assert pa.sse_to_psnr(lim, 700 * 500) >= 40.0 > pa.sse_to_psnr(lim + 1, 700 * 500)


def test_sse_zero_is_infinite_psnr():
    assert pa.sse_to_psnr(0, 100) == math.inf
    v = C.c_double(1.0)
    assert pa.load().picsong_sse_to_psnr(0, 1, C.byref(v)) == 0 and v.value == float("inf")


def test_refusals():
    L = pa.load()
    s, d = C.c_uint64(77), C.c_double(77.0)
    assert L.picsong_psnr_to_sse(40.0, 100, None) == ERR_ARG
    assert L.picsong_psnr_to_sse(40.0, 0, C.byref(s)) == ERR_ARG
    assert L.picsong_psnr_to_sse(float("nan"), 100, C.byref(s)) == ERR_ARG
    assert L.picsong_psnr_to_sse(float("inf"), 100, C.byref(s)) == ERR_ARG
    assert L.picsong_psnr_to_sse(float("-inf"), 100, C.byref(s)) == ERR_ARG
    assert L.picsong_sse_to_psnr(5, 100, None) == ERR_ARG
    assert L.picsong_sse_to_psnr(5, 0, C.byref(d)) == ERR_ARG
    assert s.value == 77 and d.value == 77.0                     # outputs untouched
    assert L.picsong_psnr_to_sse(-400.0, 1 << 40, C.byref(s)) == 0 and s.value == (1 << 64) - 1    # saturates
