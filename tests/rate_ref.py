"""Reference model of the rate calls (picsong_encode_frame_rate and its mirrors).  TEST INFRASTRUCTURE ONLY.

The header stores qs as int(qs * 10000) (float32 arithmetic) in 14 bits and a decoder reads q(j) = float32(j / 10000.0).
grid(): the j the header stores unchanged.  bisect(): the procedure that DEFINES the result (size against j is not
monotone, so "the largest j that fits" is not defined without an exhaustive scan).  The size functions code with the
CPU oracle, never with the code under test."""
import collections

import numpy as np

import oracle_lib as orc

J_MAX = 16383


def q(j):
    """What picsong_header_unpack returns for a stored j, as a Python float holding the float32 value."""
    return float(np.float32(j / 10000.0))


def grid(j_min=0, j_max=0):
    """G' ascending: the header-exact j inside [j_min, j_max]; 0, 0 = the whole grid G."""
    if j_min == 0 and j_max == 0:
        j_min, j_max = 1, J_MAX
    j = np.arange(j_min, j_max + 1, dtype=np.int64)
    qv = (j / 10000.0).astype(np.float32)
    stored = (qv * np.float32(10000)).astype(np.int32)          # float32 product, truncated: picsong_header_pack
    return [int(v) for v in j[stored == j]]


Result = collections.namedtuple("Result", "j size next_j next_size probes first_size")
Result.__doc__ = """j: the result (None: nothing fits); size: size(j); next_j / next_size: G'[lo + 1] and its size where
the procedure probed it (None at the top of the range); probes: [(j, size)] in the procedure's order; first_size:
size(G'[0]) (computed besides the procedure's probes, for the tests' preconditions)."""


def bisect(size_fn, target, j_min=0, j_max=0):
    g = grid(j_min, j_max)
    assert g, "the range holds no grid entry"
    seen = {}
    probes = []

    def size(j):
        if j not in seen:
            seen[j] = int(size_fn(j))
        return seen[j]

    lo, hi = -1, len(g)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        s = size(g[mid])
        probes.append((g[mid], s))
        if s <= target:
            lo = mid
        else:
            hi = mid
    probed = dict(probes)
    nxt = g[lo + 1] if lo + 1 < len(g) else None
    return Result(g[lo] if lo >= 0 else None, probed[g[lo]] if lo >= 0 else None, nxt,
                  probed.get(nxt) if nxt is not None else None, probes, size(g[0]))


def rounds3(value_fn, limit, j_min=0, j_max=0, pass_moves_lo=True):
    """The K = 3 round: every j probed, round by round.  A round's candidates, ascending, are (lo+mid)//2 when
    mid - lo > 1, mid, and (mid+hi)//2 when hi - mid > 1; then two levels of the procedure are applied (the midpoint,
    and the candidate its outcome leads to where there is one).  A pass (value <= limit) moves lo (the rate calls) or
    hi (the quality calls, pass_moves_lo = False)."""
    g = grid(j_min, j_max)
    lo, hi = -1, len(g)
    probed = []

    def level(i):
        nonlocal lo, hi
        if (int(value_fn(g[i])) <= limit) == pass_moves_lo:
            lo = i
        else:
            hi = i

    while hi - lo > 1:
        mid = (lo + hi) // 2
        left = (lo + mid) // 2 if mid - lo > 1 else None
        right = (mid + hi) // 2 if hi - mid > 1 else None
        probed += [g[i] for i in (left, mid, right) if i is not None]
        level(mid)
        second = right if lo == mid else left
        if second is not None:
            level(second)
    return probed


def frames_size_fn(imgs, wl, lut, k=0.0):
    """size(j) of grey frames: the sum of the oracle's codestream lengths (shorts, header and terminator included)."""
    def fn(j):
        return sum(orc.encode_frame(img, wl, True, q(j), lut, iter_=f, k=k).size for f, img in enumerate(imgs))
    return fn


def rgb_components(r, g, b):
    """The oracle's ICT (level shift fused) of the padded planes of an RGB frame."""
    return orc.rgb_forward(orc.pad_frame(r), orc.pad_frame(g), orc.pad_frame(b), True)


def rgb_streams(comps, wl, j, luts, header=None):
    """The three codestreams of an RGB frame at q(j): per-component encode_plane with the component tables; `header`
    (nine shorts) on component 0 only (header_mask = 1)."""
    return [orc.encode_plane(comps[c], wl, True, q(j), luts[c], header if c == 0 else None) for c in range(3)]


def rgb_size_fn(comps, wl, luts):
    def fn(j):
        return sum(s.size for s in rgb_streams(comps, wl, j, luts))
    return fn
