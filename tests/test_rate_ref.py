"""The reference model of the rate calls (rate_ref.py) against the oracle results recorded when the feature was specified:
the grid, and the procedure over the whole grid on the oracle's own codestream sizes."""
import pytest

import oracle_lib as orc
import rate_ref as rr

# (W, H, wl, target shorts) -> (result j, size, size at the next grid entry); None: nothing fits
ORACLE_RESULTS = [
    (200, 136, 3, 8000, (2829, 8000, 8001)),
    (200, 136, 3, 34, (9, 34, 323)),
    (200, 136, 3, 33, None),
    (200, 136, 3, 20000, (16382, 16949, None)),
    (320, 192, 5, 6000, (1407, 5999, 6003)),
    (700, 500, 5, 60000, (3098, 59995, 60016)),
]


def test_grid():
    g = rr.grid()
    assert len(g) == 15240
    assert g[:8] == [1, 2, 3, 4, 5, 6, 8, 9] and g[-1] == 16382
    missing = sorted(set(range(1, 16384)) - set(g))
    assert len(missing) == 1143 and missing[:6] == [7, 14, 28, 45, 56, 90] and missing[-1] == 16383
    assert rr.grid(1000, 3000) == [j for j in g if 1000 <= j <= 3000]
    assert rr.grid(7, 7) == []


def test_size_is_not_monotone_in_j():
    """Why the result is a procedure: the oracle's sizes at j = 4990..4993."""
    size = rr.frames_size_fn([orc.gen_frame(200, 136)], 3, orc.lut_for(True, 3))
    assert [size(j) for j in range(4990, 4994)] == [10847, 10845, 10845, 10844]


@pytest.mark.parametrize("W,H,wl,target,want", ORACLE_RESULTS)
def test_model_reproduces_the_oracle_results(W, H, wl, target, want):
    res = rr.bisect(rr.frames_size_fn([orc.gen_frame(W, H)], wl, orc.lut_for(True, wl)), target)
    assert len(res.probes) == (13 if want is None else 14)
    if want is None:
        assert res.j is None and res.first_size > target
        return
    j, size, next_size = want
    assert (res.j, res.size) == (j, size) and size <= target
    if next_size is None:
        assert res.next_j is None and res.j == rr.grid()[-1]
    else:
        assert res.next_size == next_size > target
