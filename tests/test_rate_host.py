"""Host-side rate calls of the C ABI (no GPU): picsong_rate_qs over every j against the model's grid, and the header
round trip of every grid value."""
import ctypes as C

import numpy as np

import picsong_amd as pa
import rate_ref as rr

ERR_ARG = -1


def test_rate_qs_succeeds_exactly_on_the_grid():
    L = pa.load()
    g = set(rr.grid())
    q = C.c_float()
    for j in range(1, rr.J_MAX + 1):
        rc = L.picsong_rate_qs(j, C.byref(q))
        assert rc == (0 if j in g else ERR_ARG), j
        if rc == 0:
            assert np.float32(q.value).tobytes() == np.float32(j / 10000.0).tobytes(), j
    for j in (0, -1, rr.J_MAX + 1, 1 << 20):
        assert L.picsong_rate_qs(j, C.byref(q)) == ERR_ARG
    assert L.picsong_rate_qs(5, None) == ERR_ARG
    assert pa.rate_qs(5000) == 0.5


def test_header_round_trip_of_every_grid_value():
    p = pa.make_params(700, 500, wl=5, lossy=True)
    for j in rr.grid():
        p.qs = pa.rate_qs(j)
        back = pa.header_unpack(pa.header_pack(p))
        assert np.float32(back.qs).tobytes() == np.float32(p.qs).tobytes(), j


def test_a_value_off_the_grid_is_stored_as_another():
    """Existing behaviour, and why the search keeps to the grid: q(7) * 10000 truncates to 6."""
    p = pa.make_params(700, 500, wl=5, lossy=True, qs=rr.q(7))
    assert np.float32(pa.header_unpack(pa.header_pack(p)).qs) == np.float32(rr.q(6))
