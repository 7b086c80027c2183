"""The reference model of the quality calls (quality_ref.py) against the oracle results recorded when the feature was
specified: the procedure over the oracle's own decode of its own encode, the coder-free route asserted equal to it at
every probe (quality_ref.frames_sse_list / rgb_sse_list)."""
import pytest

import oracle_lib as orc
import quality_ref as qr

# whole-grid probe counts measured when the feature was specified (the others were not)
PROBES = {"200x136-wl3-40dB": 13, "320x192-wl5-30dB": 14, "700x500-wl5-40dB": 14, "700x500-wl6-50dB": 14}


def test_limit_is_the_documented_formula():
    for name, c in qr.CASES.items():
        W, H, wl, frames, rgb, db = c[:6]
        assert qr.limit(db, W * H * frames * (3 if rgb else 1)) == c[8], name


@pytest.mark.parametrize("name", sorted(qr.CASES))
def test_model_reproduces_the_oracle_results(name):
    W, H, wl, frames, rgb, db, j_min, j_max, limit, j, per, prev_j, prev_sse = qr.CASES[name]
    res = qr.case_result(name)
    g = qr.grid(j_min, j_max)
    assert res.j == j and g[0] < j < g[-1]                                   # interior
    assert res.sse == sum(per) <= limit
    assert res.prev_j == prev_j and res.prev_sse == prev_sse > limit         # a probe the procedure itself made
    if name in PROBES:
        assert len(res.probes) == PROBES[name]
    imgs, lut = qr.case_inputs(name)
    got = qr.rgb_sse_list(imgs, wl, lut, j) if rgb else qr.frames_sse_list(imgs, wl, lut, j)
    assert got == per


def test_sse_is_not_monotone_in_j():
    """Why the result is a procedure: rising steps among the grid values around the 40 dB result, and the top of the grid."""
    fn = qr.case_sse_fn("200x136-wl3-40dB")
    g = [j for j in qr.grid() if 1825 <= j <= 1905][:81]
    v = [fn(j) for j in g]
    assert sum(1 for a, b in zip(v, v[1:]) if b > a) >= 1
    assert fn(16374) == 332 and fn(16382) == 339


def test_edges_of_the_grid():
    name = "200x136-wl3-40dB"
    top = qr.case_result(name, max_sse=10 ** 12)
    assert top.j == 1 and top.prev_j is None
    low = qr.case_result(name, max_sse=339)
    assert low.j == 16374 and low.sse == 332                 # not 16382 (339 as well): a procedure, not an argmin
    none = qr.case_result(name, max_sse=0)
    assert none.j is None and len(none.probes) == 14


def test_edge_of_a_sub_range():
    name = "700x500-wl6-40dB-sub"
    fn = qr.case_sse_fn(name)
    assert fn(3000) == 778018
    assert qr.case_result(name, max_sse=778017).j is None
    assert qr.case_result(name, max_sse=778017, j_min=0, j_max=0).j == 3001
