"""Reference model of the n-frame RGB search calls (picsong_encode_rgb_frames_rate / _quality).  TEST INFRASTRUCTURE ONLY.

Frame f is the planes oracle.gen_frame(W, H, 60 + 3 f + c), c = 0..2, the tables the shipped R / G / B files.  size(j) is
the sum of the 3 n stream lengths, sse(j) the sum over the 3 n planes, both through the CPU oracle (rate_ref.rgb_streams,
quality_ref.rgb_sse_list), never through the code under test; the results are the procedures' (rate_ref.bisect,
quality_ref.bisect).  The rate target is floor(bpp W H / 16) n shorts, the quality limit quality_ref.limit(dB, 3 W H n).

CASES records what the oracle gave when the feature was specified; check() recomputes a row and asserts it, with the
precondition every test stands on: the result passes and its neighbour on the grid fails the limit."""
import numpy as np

import oracle_lib as orc
import quality_ref as qr
import rate_ref as rr

# (W, H, wl, n) -> bpp, rate target, j, size(j), next j, its size; dB, limit, j, sse(j), previous j, its sse, per plane sse or None
CASES = {
    (200, 136, 3, 1): (1.0, 1700, 564, 1538, 565, 1730, 35, 1677917, 1340, 1677600, 1339, 1679346, None),
    (200, 136, 3, 2): (2.0, 6800, 824, 6720, 825, 6850, 40, 1061208, 3128, 1060326, 3127, 1061383,
                       [[178524, 105882, 246045], [180509, 104129, 245237]]),
    (200, 136, 3, 3): (1.0, 5100, 567, 4802, 568, 5122, 35, 5033751, 1347, 5029620, 1346, 5035513, None),
    (200, 136, 3, 8): (2.0, 27200, 811, 27128, 812, 27296, 40, 4244832, 3128, 4243102, 3127, 4246782, None),
    (201, 137, 3, 2): (2.0, 6884, 828, 6854, 829, 7001, 40, 1074356, 3123, 1073700, 3122, 1074510,
                       [[181170, 105784, 249997], [181873, 106061, 248815]]),
    (320, 192, 5, 2): (1.5, 11520, 930, 11504, 932, 11664, 38, 3799118, 2489, 3796761, 2488, 3800206, None),
}
_cache = {}


def frames(W, H, n):
    """[frame][component] unpadded planes."""
    return [[orc.gen_frame(W, H, 60 + 3 * f + c) for c in range(3)] for f in range(n)]


def luts(wl, k=0.0):
    return [orc.lut_for_component(True, wl, c, k=k) for c in range(3)]


def rate_target(W, H, n, bpp):
    return int(bpp * W * H / 16) * n


def quality_limit(W, H, n, dB):
    return qr.limit(dB, 3 * W * H * n)


def components(W, H, n):
    key = ("comps", W, H, n)
    if key not in _cache:
        _cache[key] = [rr.rgb_components(*fr) for fr in frames(W, H, n)]
    return _cache[key]


def size_fn(W, H, wl, n, k=0.0):
    comps, tabs = components(W, H, n), luts(wl, k)
    seen = _cache.setdefault(("size", W, H, wl, n, k), {})

    def fn(j):
        if j not in seen:
            seen[j] = sum(orc.encode_plane(comps[f][c], wl, True, rr.q(j), tabs[c], None, k=k).size for f in range(n) for c in range(3))
        return seen[j]
    return fn


def sse_lists(W, H, wl, n, j):
    """[frame][plane] at q(j)."""
    key = ("sse", W, H, wl, n, j)
    if key not in _cache:
        tabs = luts(wl)
        _cache[key] = [qr.rgb_sse_list(fr, wl, tabs, j) for fr in frames(W, H, n)]
    return _cache[key]


def sse_fn(W, H, wl, n):
    return lambda j: sum(sum(p) for p in sse_lists(W, H, wl, n, j))


def rate_result(W, H, wl, n, target=None, j_min=0, j_max=0, k=0.0):
    target = CASES[(W, H, wl, n)][1] if target is None else target
    key = ("rate", W, H, wl, n, target, j_min, j_max, k)
    if key not in _cache:
        _cache[key] = rr.bisect(size_fn(W, H, wl, n, k), target, j_min, j_max)
    return _cache[key]


def quality_result(W, H, wl, n, limit=None, j_min=0, j_max=0):
    limit = CASES[(W, H, wl, n)][7] if limit is None else limit
    key = ("quality", W, H, wl, n, limit, j_min, j_max)
    if key not in _cache:
        _cache[key] = qr.bisect(sse_fn(W, H, wl, n), limit, j_min, j_max)
    return _cache[key]


def check_rate(W, H, wl, n):
    """Asserts the table's rate columns on the oracle and the precondition; returns (target, j)."""
    bpp, target, j, size, next_j, next_size = CASES[(W, H, wl, n)][:6]
    assert rate_target(W, H, n, bpp) == target
    ref = rate_result(W, H, wl, n)
    assert (ref.j, ref.size, ref.next_j, ref.next_size) == (j, size, next_j, next_size), ref[:4]
    assert size <= target < next_size, "the case's point: the result fits and its neighbour does not"
    return target, j


def check_quality(W, H, wl, n):
    """Asserts the table's quality columns on the oracle and the precondition; returns (limit, j, [frame][plane] sse)."""
    dB, limit, j, sse, prev_j, prev_sse, per = CASES[(W, H, wl, n)][6:]
    assert quality_limit(W, H, n, dB) == limit
    ref = quality_result(W, H, wl, n)
    assert (ref.j, ref.sse, ref.prev_j, ref.prev_sse) == (j, sse, prev_j, prev_sse), ref[:4]
    assert sse <= limit < prev_sse, "the case's point: the result meets the limit and its neighbour does not"
    planes = sse_lists(W, H, wl, n, j)
    if per is not None:
        assert planes == per
    return limit, j, planes


def streams(W, H, wl, n, j, header, first_iter=0, header_mask=7, k=0.0):
    """The oracle's 3 n codestreams at q(j): `header` (nine shorts carrying q(j)) on the components of header_mask of the
    frame with first_iter + f == 0."""
    comps, tabs = components(W, H, n), luts(wl, k)
    out = []
    for f in range(n):
        for c in range(3):
            has = first_iter + f == 0 and (header_mask >> c) & 1
            out.append(orc.encode_plane(comps[f][c], wl, True, rr.q(j), tabs[c], header if has else None, k=k))
    return out


def padded_stack(W, H, n):
    """Three uint8 [n, AH, AW] arrays: the R, G and B planes of the n frames, padded."""
    fr = frames(W, H, n)
    return [np.stack([orc.pad_frame(fr[f][c]) for f in range(n)]) for c in range(3)]
