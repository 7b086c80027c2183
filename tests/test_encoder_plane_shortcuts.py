"""The k = 0 encoder's two shortcuts around its call sites (csrc/bpc_kernels.hpp): find_subband as selects over the
levels (PICSONG_ENC_SUBBAND_SELECT) and the context-8 lookup of a 4-row group run only where some lane of the wave has
all eight neighbours visibly significant (PICSONG_ENC_CTX8_GATE).

Without a GPU: find_subband through a small emulator driver (tests/hipemu/emu_subband_driver.cpp) against the search
restated in Python, and the encoder on the CPU wave emulator against the oracle on three inputs -- a photographic
frame, a dense one in which many groups hold context 8, and a sparse one in which a single lane of the wave opens the
gate.  The context-8 sites of the dense and the sparse input are counted from the oracle's coefficients beside it, so a
test cannot pass by never reaching the gated lookup, or by never skipping it.  With one (-m gpu): the same inputs as
pixels through picsong_encode_frame / picsong_encode_frames against the oracle's codestreams, and one 9/7 frame."""
import os

import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc
from emu_lib import _p, driver_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        orc.lib()
        _lib = driver_lib("libpicsong_emu_subband.so", ("emu_subband_driver.cpp", "emu_runtime.cpp"))
    return _lib


# ---- subband search ---------------------------------------------------------------------------------------------

def subband_search(x, y, AW, AH, wl):
    """The search as the reference states it: the first a in 1..wl with x >= AW >> a or y >= AH >> a."""
    level = np.full(x.shape, wl, np.int32)
    sb = np.zeros(x.shape, np.int32)
    found = np.zeros(x.shape, bool)
    for a in range(1, wl + 1):
        cx, cy = x >= (AW >> a), y >= (AH >> a)
        hit = (cx | cy) & ~found
        level[hit] = a - 1
        sb[hit] = np.where(cx, np.where(cy, 2, 0), 1)[hit]
        found |= hit
    return level, sb


@pytest.mark.parametrize("wl", [1, 3, 5, 6])
@pytest.mark.parametrize("AW,AH", [(64, 64), (448, 320), (960, 576), (7680, 4352)])
def test_find_subband_every_lane_start(AW, AH, wl):
    """Every position a lane asks about: x = cbx * 64 + 2 t, y = cby * 64.  (448 x 320: subband widths of 56, 28, ...
    -- lanes of one codeblock in different subbands; 64 x 64 at wl 6: subbands a sample wide.)"""
    xs = np.arange(0, AW, 2, dtype=np.int32)
    ys = np.arange(0, AH, 64, dtype=np.int32)
    x = np.ascontiguousarray(np.tile(xs, ys.size))
    y = np.ascontiguousarray(np.repeat(ys, xs.size))
    level = np.full(x.size, -7, np.int32)
    sb = np.full(x.size, -7, np.int32)
    lib().emu_find_subband(_p(x), _p(y), int(x.size), AW, AH, wl, _p(level), _p(sb))
    level_ref, sb_ref = subband_search(x, y, AW, AH, wl)
    assert np.array_equal(level, level_ref) and np.array_equal(sb, sb_ref)
    assert level[0] == wl and sb[0] == 0                       # the LL band
    if (AW, AH) == (448, 320) and wl >= 3:                     # 448 >> 3 = 56: the first codeblock's lanes differ
        assert level[0] != level[31]


# ---- the three inputs -------------------------------------------------------------------------------------------

def ctx8_sites(coef):
    """(codeblock, bit-plane, row, column) of every significance symbol the lock-step scan codes with context 8: the
    coefficient insignificant before the plane and all eight neighbours VISIBLY significant -- significant before
    the plane (A), or becoming so in it (N) and visited earlier: the row above sees A | N, the row below A, the same
    row A for an even column (the lanes' left coefficients come first) and A | N for an odd one.  Neighbours outside
    the codeblock count as insignificant."""
    mag = np.abs(np.trunc(np.asarray(coef, np.float64))).astype(np.int64)
    AH, AW = mag.shape
    even = np.zeros((64, 64), bool)
    even[:, 0::2] = True
    sites = []

    def at(a, dy, dx):                                         # a[r + dy, c + dx], False outside the block
        p = np.zeros((66, 66), bool)
        p[1:65, 1:65] = a
        return p[1 + dy:65 + dy, 1 + dx:65 + dx]

    for cb in range((AW // 64) * (AH // 64)):
        cby, cbx = divmod(cb, AW // 64)
        m = mag[cby * 64:cby * 64 + 64, cbx * 64:cbx * 64 + 64]
        if m.max() == 0:
            continue
        for bp in range(min(int(m.max()).bit_length() - 1, 15), -1, -1):
            A = (m >> (bp + 1)) != 0
            A2 = A | (((m >> bp) & 1) != 0)
            cnt = sum(at(A2, -1, dx).astype(int) + at(A, 1, dx) for dx in (-1, 0, 1))
            cnt = cnt + sum(np.where(even, at(A, 0, dx), at(A2, 0, dx)) for dx in (-1, 1))
            sites += [(cb, bp, int(r), int(c)) for r, c in np.argwhere((cnt == 8) & ~A)]
    return sites


def patch_places(AW, AH):
    """Two planted context-8 sites (codeblock, row, column inside it): an odd codeblock (the upper half of its wave),
    rows 0..31, row 1 of its 4-row group, a right column; an even one, rows 32..63, row 2 of its group, a left column."""
    ncb = (AW // 64) * (AH // 64)
    return [(1, 21, 37), (2 * (ncb // 3), 46, 10)]


def dense_coeffs(AW, AH, seed=11):
    """oracle_lib.deep_coeffs (spikes up to bit-plane 15 in every subband) with rows 16..47 of every codeblock filled: a
    field in which coefficients of every magnitude below 64 lie side by side, so that from plane 4 down most 4-row groups
    of those rows hold a coefficient with eight significant neighbours."""
    rng = np.random.default_rng(seed)
    coef = orc.deep_coeffs(AW, AH, seed)
    for y0 in range(16, AH, 64):
        coef[y0:y0 + 32] = rng.integers(-63, 64, (32, AW))
    return coef


def sparse_coeffs(AW, AH, seed=12):
    """Zeros, isolated +-1 (no two closer than three samples), and at each of patch_places a 3 x 3 patch of +-2 around a
    centre of 1 / 0: at bit-plane 0 the centre is insignificant with all eight neighbours significant, nothing else is."""
    rng = np.random.default_rng(seed)
    coef = np.zeros((AH, AW), np.int32)
    lat = (rng.random((AH // 3, AW // 3)) < 0.08) * rng.choice([-1, 1], (AH // 3, AW // 3))
    coef[1:AH // 3 * 3:3, 1:AW // 3 * 3:3] = lat
    for i, (cb, r, c) in enumerate(patch_places(AW, AH)):
        cby, cbx = divmod(cb, AW // 64)
        y, x = cby * 64 + r, cbx * 64 + c
        coef[y - 3:y + 4, x - 3:x + 4] = 0
        coef[y - 1:y + 2, x - 1:x + 2] = 2 * rng.choice([-1, 1], (3, 3))
        coef[y, x] = 1 - i
    return coef


def planted(AW, AH):
    return sorted((cb, 0, r, c) for cb, r, c in patch_places(AW, AH))


def frame_coeffs(AW, AH, wl, frame):
    x = orc.level_shift_fwd(orc.gen_frame(AW, AH, frame), False)
    return orc.dwt_forward(x, wl)[:AW * AH].reshape(AH, AW)


_inputs = {}


def coeff_inputs(AW, AH, wl):
    """The three coefficient arrays of a geometry, made once, with what ctx8_sites finds in the made-up two."""
    key = (AW, AH, wl)
    if key not in _inputs:
        d = {"frame": frame_coeffs(AW, AH, wl, 5), "dense": dense_coeffs(AW, AH), "sparse": sparse_coeffs(AW, AH)}
        for v in d.values():
            v.setflags(write=False)
        _inputs[key] = (d, {k: ctx8_sites(d[k]) for k in ("dense", "sparse")})
    return _inputs[key]


def check_ctx8_sites(sites, name, AW, AH):
    if name == "sparse":
        assert sorted(sites) == planted(AW, AH)
    if name == "dense":
        # the filled rows of every codeblock hold such sites, in both 32-row halves, both columns of a lane, both halves
        # of a wave and every row of a 4-row group
        ncb = (AW // 64) * (AH // 64)
        assert {s[0] for s in sites} == set(range(ncb))
        assert {(s[2] >= 32, s[3] & 1, s[0] & 1) for s in sites} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        assert {s[2] & 3 for s in sites} == {0, 1, 2, 3}
        groups = {(s[0], s[1], s[2] >> 2) for s in sites if s[1] <= 4}
        assert len(groups) > (ncb * 5 * 8) // 2, "most 4-row groups of the filled rows, planes 4..0"


@pytest.mark.parametrize("name", ["frame", "dense", "sparse"])
@pytest.mark.parametrize("AW,AH,wl", [(128, 128, 2), (448, 320, 3)])
def test_emulated_encoder_equals_oracle(AW, AH, wl, name):
    inputs, sites = coeff_inputs(AW, AH, wl)
    if name in sites:
        check_ctx8_sites(sites[name], name, AW, AH)
    coef = inputs[name]
    lut = orc.lut_for(False, wl)
    st_ref, sz_ref = orc.bpc_encode(coef, wl, lut)
    st, sz, flag = E.bpc_encode(coef, wl, lut)
    assert flag == 0
    assert np.array_equal(sz, sz_ref)
    assert np.array_equal(st, st_ref)


# ---- GPU --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return t


@pytest.fixture(scope="module")
def pa():
    import picsong_amd
    picsong_amd.load()
    return picsong_amd


def pixels_of(coef, wl):
    """The frame whose 5/3 coefficients are `coef` wherever its samples fit 8 bits (the integer transform is
    reversible), clamped where they do not; and the coefficients that frame really has."""
    AH, AW = coef.shape
    inv, extra = orc.dwt_inverse(coef, wl, False)
    img = np.clip(orc.level_shift_inv(inv[extra:]).reshape(AH, AW), 0, 255).astype(np.uint8)
    back = orc.dwt_forward(orc.level_shift_fwd(img, False), wl)[:AW * AH].reshape(AH, AW)
    return img, back


_frames = {}


def pixel_inputs(AW, AH, wl):
    """The three inputs as frames.  The sparse one's coefficients come back exactly; the dense one is scaled to the
    range of 8-bit pixels first and its context-8 sites are counted on the coefficients the clamped frame really has."""
    key = (AW, AH, wl)
    if key not in _frames:
        sparse, back = pixels_of(sparse_coeffs(AW, AH), wl)
        assert np.array_equal(back, sparse_coeffs(AW, AH))
        assert sorted(ctx8_sites(back)) == planted(AW, AH)
        dense, back = pixels_of(np.clip(dense_coeffs(AW, AH), -63, 63), wl)
        sites = ctx8_sites(back)
        assert len({s[0] for s in sites}) > (AW // 64) * (AH // 64) // 2, "context-8 sites in most codeblocks"
        _frames[key] = {"frame": orc.gen_frame(AW, AH, 5), "dense": dense, "sparse": sparse}
    return _frames[key]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frame", "dense", "sparse"])
def test_gpu_frame_equals_oracle(pa, torch, name):
    AW, AH, wl = 448, 320, 3
    img = pixel_inputs(AW, AH, wl)[name]
    lut = orc.lut_for(False, wl)
    ref = orc.encode_frame(img, wl, False, 1.0, lut)
    c = pa.Codec(AW, AH, wl=wl, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossless"))
    assert (c.aw, c.ah) == (AW, AH)
    got = c.encode_frame(_dev(torch, img), 0).cpu().numpy().view(np.uint16)
    assert c.range_flag() == 0
    c.close()
    assert got.size == ref.size and np.array_equal(got, ref)


@pytest.mark.gpu
def test_gpu_batched_frames_equal_oracle(pa, torch):
    """The three inputs as the three frames of one picsong_encode_frames launch."""
    AW, AH, wl = 960, 576, 5
    imgs = pixel_inputs(AW, AH, wl)
    lut = orc.lut_for(False, wl)
    c = pa.Codec(AW, AH, wl=wl, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossless"))
    assert (c.aw, c.ah) == (AW, AH)
    names = ["frame", "dense", "sparse"]
    got = c.encode_frames(_dev(torch, np.stack([imgs[n].reshape(-1) for n in names])), 0)
    assert c.range_flag() == 0
    for f, n in enumerate(names):
        ref = orc.encode_frame(imgs[n], wl, False, 1.0, lut, f, 0)
        g = got[f].cpu().numpy().view(np.uint16)
        assert g.size == ref.size and np.array_equal(g, ref), n
    c.close()


@pytest.mark.gpu
def test_gpu_lossy_wl6_frame_equals_oracle(pa, torch):
    """9/7, qs 0.5, wl 6: the float prologue, and the wl = 6 tables' unwritten groups (probability 0)."""
    AW, AH, wl, qs = 448, 320, 6, 0.5
    img = orc.gen_frame(AW, AH, 5)
    lut = orc.lut_for(True, wl)
    ref = orc.encode_frame(img, wl, True, qs, lut)
    c = pa.Codec(AW, AH, wl=wl, lossy=True, qs=qs, lut_folder=os.path.join(orc.LUT_DIR, "n1_lossy"))
    assert (c.aw, c.ah) == (AW, AH)
    got = c.encode_frame(_dev(torch, img), 0).cpu().numpy().view(np.uint16)
    c.close()
    assert got.size == ref.size and np.array_equal(got, ref)
