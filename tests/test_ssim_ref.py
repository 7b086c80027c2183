"""The reference model of the SSIM calls (ssim_ref.py) against the numbers recorded when the feature was specified, the
textbook formula, and the recorded search cases on the CPU oracle."""
import numpy as np
import pytest

import ssim_ref as sr


def test_identical_images_give_exactly_the_full_sum():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (139, 203)).astype(np.uint8)
    q = sr.window_q(a, a)
    assert q.shape == (33, 49) and np.all(q == 1 << 24)
    assert sr.dssim(a, a) == 0
    flat = np.full((40, 40), 77, np.uint8)
    assert sr.dssim(flat, flat) == 0


def test_recorded_numbers():
    z, f = np.zeros((40, 40), np.uint8), np.full((40, 40), 255, np.uint8)
    q = sr.window_q(z, f)
    assert q.size == 81 == sr.windows(40, 40) and int(q.sum()) == 2106
    assert sr.dssim(z, f) == 81 * (1 << 24) - 2106
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (139, 203)).astype(np.uint8)
    assert sr.window_q(a, 255 - a).min() < 0                 # anti-correlated content: negative q
    x, y = np.meshgrid(np.arange(64), np.arange(64))
    g = ((x * 37 + y * 91) % 256).astype(np.uint8)
    assert sr.window_q(g, 255 - g).min() < -(1 << 22)
    assert sr.window_q(a, rng.integers(0, 256, a.shape).astype(np.uint8)).max() <= 1 << 24
    assert sr.windows(33, 32) == 49 and sr.windows(8, 8) == 1 and sr.windows(11, 15) == 2 and sr.windows(7680, 4320) == 1919 * 1079


def test_trailing_columns_and_rows_belong_to_no_window():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (139, 203)).astype(np.uint8)
    b = rng.integers(0, 256, (139, 203)).astype(np.uint8)
    c = b.copy()
    c[:, 200:] ^= 0xFF                                      # 4 (nx + 1) = 200, 4 (ny + 1) = 136
    c[136:, :] ^= 0xFF
    assert sr.dssim(a, b) == sr.dssim(a, c)
    c[135, 199] ^= 1
    assert sr.dssim(a, b) != sr.dssim(a, c)


def test_agreement_with_the_textbook_formula():
    """Per window |q / 2^24 - textbook SSIM| <= 1e-6 on a 203 x 139 noisy frame (an image and the image with noise added).
    Measured maximum: 8.3e-7 (the floor to 24 bits gives up to 6e-8; the rest is x264's luminance constant, below).
    x264's c1 is the textbook's C1 / 64 (ssim_ref.textbook_ssim), which moves the luminance term by about 6e-9 d^2 where
    the windows' means differ by d: on noise against noise (d up to 30) the textbook value with C1 = 6.5025 lies up to
    3.1e-6 away -- measured and printed here, not asserted -- and the textbook formula with x264's luminance constant
    within the same 1e-6 (measured 5.5e-8)."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (139, 203)).astype(np.uint8)
    b = (a.astype(np.int32) + rng.integers(-40, 41, a.shape)).clip(0, 255).astype(np.uint8)
    err = np.abs(sr.window_q(a, b) / float(1 << 24) - sr.textbook_ssim(a, b)).max()
    print("noisy frame: max |q / 2^24 - textbook| =", err)
    assert err <= 1e-6
    c = rng.integers(0, 256, a.shape).astype(np.uint8)
    qc = sr.window_q(a, c) / float(1 << 24)
    print("noise against noise, textbook C1:", np.abs(qc - sr.textbook_ssim(a, c)).max())
    err2 = np.abs(qc - sr.textbook_ssim(a, c, sr.X264_K1)).max()
    print("noise against noise, x264's C1:", err2)
    assert err2 <= 1e-6


def test_conversions():
    assert sr.ssim_to_dssim(0.98, 1617) == 542575165 and sr.ssim_to_dssim(0.98, 3 * 1617) == 1627725496
    assert sr.ssim_to_dssim(1.0, 1000) == 0 and sr.ssim_to_dssim(0.0, 3) == 3 << 24 and sr.ssim_to_dssim(-1.0, 1) == 2 << 24
    assert sr.dssim_to_ssim(0, 5) == 1.0 and sr.dssim_to_ssim(5 << 24, 5) == 0.0
    lim = sr.ssim_to_dssim(0.9, 4503)
    assert sr.dssim_to_ssim(lim, 4503) >= 0.9 - 1e-12 > sr.dssim_to_ssim(lim + 4503, 4503)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_recorded_search_cases(name):
    inputs, target, limit, j, d, prev_j, prev_d = sr.CASES[name]
    assert sr.case_limit(name) == limit
    res = sr.case_result(name)
    assert (res.j, res.sse, res.prev_j, res.prev_sse) == (j, d, prev_j, prev_d)
    assert d <= limit < prev_d, "the case's point: the result meets the limit and its neighbour does not"
    assert len(res.probes) == 14 and sum(sr.case_list_fn(name)(j)) == d
