"""The per-level transform kernels' 8-, 16- and 32-row band instantiations (dwt_fwd_kernel, dwt_inv_kernel,
dwt_inv97_kernel, dwt_inv_rgb_kernel, dwt_inv97_rgb_kernel; csrc/dwt_kernels.hpp) on the CPU wave emulator, bit for bit
against the oracle.  launch_plan.hpp picks the band height from a level's sample count -- 4 rows below 1 Mi (9/7
synthesis) / 4 Mi samples, which is every shape the emulator can afford -- so the cases here set PICSONG_DWT_BANDS, the
per-level override the plans read at every call.

The shapes give a ragged last band ((H >> 1) % (BAND / 2) != 0) at every height on some level; 704 x 192 is four strips
across.  Every case runs the vector and the per-column kernels; the frame paths' forms (int16 coefficients, pixel output,
the RGB head and tails, three frames a call) run where their geometry rules admit them.  The last test holds the file to
its purpose: every kernel the selectors of kernel_select.hpp can return has been launched by the cases above."""
import numpy as np
import pytest

import emu_lib as E
import oracle_lib as orc

# (W, H, wl): level heights 200/100/50, 72/36, 40, 24/12, 136/68/34, 104/52/26, 192/96/48 -- row pairs 100/50/25, 36/18,
# 20, 12/6, 68/34/17, 52/26/13, 96/48/24
SHAPES = [(320, 200, 3), (264, 72, 2), (512, 40, 1), (64, 24, 2), (576, 136, 3), (448, 104, 3), (704, 192, 3)]
# every level of these on the vector kernels and wl >= 2: the 16-bit coefficient forms apply (dwt_c16_geometry_ok, dec_c16_ok)
C16_SHAPES = [s for s in SHAPES if s not in ((264, 72, 2), (512, 40, 1))]
# "default": no override, the policy's own 4-row bands -- the band-4 instantiations belong to the selectors' list too
BAND_LISTS = {"8": "8,8,8", "16": "16,16,16", "32": "32,32,32", "mixed": "32,16,8,4", "default": None}
TRANSFORMS = {"53": (False, 1.0), "97q05": (True, 0.5), "97q03": (True, 0.3)}      # qs = 0.5: one_div
SWITCHES = ("PICSONG_DWT_BANDS", "PICSONG_DWT_NOVEC", "PICSONG_DWT_NOFUSE01", "PICSONG_DWT_FUSE01", "PICSONG_DWT_EXACTDIV",
            "PICSONG_DWT_INV97", "PICSONG_DWT_NOFUSE_INV", "PICSONG_DWT_FUSE_INV97", "PICSONG_DWT_EXACT_REPLAY", "PICSONG_C16",
            "PICSONG_DEC_C16")


@pytest.fixture(scope="module", autouse=True)
def launch_log():
    """The coverage assertion counts this file's launches alone."""
    E.lib()
    E.launch_log_reset()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def set_bands(monkeypatch, bands):
    if BAND_LISTS[bands] is not None:
        monkeypatch.setenv("PICSONG_DWT_BANDS", BAND_LISTS[bands])


def planned(bands, wl):
    """The band a list gives level l: its l-th value, 4 (every shape of this file by itself) where it has none."""
    vals = [int(v) for v in BAND_LISTS[bands].split(",")] if BAND_LISTS[bands] else []
    return [vals[l] if l < len(vals) else 4 for l in range(wl)]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_refs = {}


def reference(W, H, wl, tf, seed=3):
    """The oracle's side of a shape, computed once: the frame, its shifted samples, the transform, the coded integers (with
    two spikes that drive the pixels into the clamp at both ends), their synthesis and its pixels."""
    key = (W, H, wl, tf, seed)
    if key not in _refs:
        lossy, qs = TRANSFORMS[tf]
        img = orc.gen_frame(W, H, seed)
        assert img.shape == (H, W)
        x = orc.level_shift_fwd(img, lossy)
        fwd = orc.dwt_forward(x, wl, qs)[:W * H].copy()
        coef = np.trunc(fwd).astype(np.int32).reshape(H, W)
        coef[3, 5] += 4000
        coef[9, 70 % W] -= 4000
        assert np.abs(coef).max() < 32768
        inv, ex = orc.dwt_inverse(coef, wl, lossy, qs)
        inv = inv[ex:].copy()
        pix = orc.level_shift_inv(inv).reshape(H, W).astype(np.uint8)
        assert (pix == 0).any() and (pix == 255).any()
        _refs[key] = frozen(img, x, fwd, coef, inv, pix)
    return _refs[key]


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


# ---- the override itself ------------------------------------------------------------------------------------------------
def test_band_override_reaches_the_plans(monkeypatch):
    shapes = SHAPES + [(320, 192, 3)]
    for W, H, wl in shapes:                                   # without it: 4 rows everywhere -- why the override is needed
        for fast in (False, True):
            fwd, inv = E.dwt_plan_bands(W, H, wl, True, fast)
            assert [b for b, _ in fwd] == [4] * wl and [b for b, _ in inv] == [4] * wl, (W, H, wl, fast)
    monkeypatch.setenv("PICSONG_DWT_BANDS", "32,16,8")         # level l takes the l-th value
    for W, H, wl in shapes:
        for fast in (False, True):
            fwd, inv = E.dwt_plan_bands(W, H, wl, True, fast)
            assert [b for b, _ in fwd] == [32, 16, 8][:wl] and [b for b, _ in inv] == [32, 16, 8][:wl]
    for text, want in (("8,5,32", [8, 4, 32]), ("16", [16, 4, 4]), ("8,,32", [8, 4, 32]), ("64,2,0", [4, 4, 4]), ("", [4, 4, 4]),
                       ("4,8,16,32", [4, 8, 16])):             # a value outside {4, 8, 16, 32}, or none: the level's default
        monkeypatch.setenv("PICSONG_DWT_BANDS", text)
        for fast in (False, True):
            fwd, inv = E.dwt_plan_bands(320, 200, 3, True, fast)
            assert [b for b, _ in fwd] == want and [b for b, _ in inv] == want, text
    # the vec flags are the geometry's, whatever the bands: 200 -> 100 -> 50, a width that is no multiple of 4 (level 2 per
    # column both ways)
    monkeypatch.setenv("PICSONG_DWT_BANDS", "16,16,16")
    fwd, inv = E.dwt_plan_bands(200, 64, 3)
    assert [v for _, v in fwd] == [True, True, False] and [v for _, v in inv] == [True, True, False]
    monkeypatch.setenv("PICSONG_DWT_NOVEC", "1")
    fwd, inv = E.dwt_plan_bands(200, 64, 3)
    assert not any(v for _, v in fwd + inv)


def test_inv97_band_policy_is_consulted_only_with_fast_divisions(monkeypatch):
    """2048 x 2048: level 0 is 9 strips x 248 columns x 2048 rows = 4.6 Mi samples, level 1 1.3 Mi -- fwd_band_rows gives
    8 / 4 / 4, inv97_band_rows 16 / 8 / 4, and the synthesis plan takes the latter only for a context whose reciprocal
    divisions verified (host code only: nothing is launched)."""
    fwd, inv = E.dwt_plan_bands(2048, 2048, 3, True, False)
    assert [b for b, _ in fwd] == [8, 4, 4] and [b for b, _ in inv] == [8, 4, 4]
    fwd, inv = E.dwt_plan_bands(2048, 2048, 3, True, True)
    assert [b for b, _ in fwd] == [8, 4, 4] and [b for b, _ in inv] == [16, 8, 4]
    fwd, inv = E.dwt_plan_bands(2048, 2048, 3, False, True)    # 5/3: no such thing as fast
    assert [b for b, _ in inv] == [8, 4, 4]
    monkeypatch.setenv("PICSONG_DWT_BANDS", "32,32,32")
    for fast in (False, True):
        fwd, inv = E.dwt_plan_bands(2048, 2048, 3, True, fast)
        assert [b for b, _ in fwd] == [32] * 3 and [b for b, _ in inv] == [32] * 3


# ---- the parity matrix --------------------------------------------------------------------------------------------------
# The cases are functions of their parameters so that the coverage assertion at the end can run whichever of them a
# partial selection (-k, a single node id) left out.
_done = set()


def stage_case(monkeypatch, shape, bands, path, tf):
    """The stage calls: forward from u8 (fused head where it applies, and two launches) and from shifted samples, synthesis
    to 32 bits and to pixels; 9/7 synthesis also through the dividing kernels and dwt_inv_kernel's FAST instantiations."""
    W, H, wl = shape
    lossy, qs = TRANSFORMS[tf]
    img, x, fwd, coef, inv, pix = reference(W, H, wl, tf)
    extra = orc.dwt_extra(W, H, wl)
    set_bands(monkeypatch, bands)
    if path == "novec":
        monkeypatch.setenv("PICSONG_DWT_NOVEC", "1")
    want = planned(bands, wl)
    got_fwd, got_inv = E.dwt_plan_bands(W, H, wl, lossy, lossy)
    assert [b for b, _ in got_fwd] == want and [b for b, _ in got_inv] == want
    for nofuse in (None, "1"):
        if nofuse:
            monkeypatch.setenv("PICSONG_DWT_NOFUSE01", nofuse)
        got = E.dwt_forward(np.array(img), wl, lossy, qs, extra=extra)
        assert not (nofuse and E.dwt_forward.fused01)
        assert np.array_equal(bits(got[:W * H]), bits(fwd)), f"forward from u8, nofuse01={nofuse}"
        if not E.dwt_forward.fused01:                           # (the head refused by itself: the two launches have run)
            break
    monkeypatch.delenv("PICSONG_DWT_NOFUSE01", raising=False)
    got = E.dwt_forward(np.array(x), wl, lossy, qs, extra=extra)
    assert np.array_equal(bits(got[:W * H]), bits(fwd)), "forward from shifted samples"
    modes = [{}] + ([{"PICSONG_DWT_EXACTDIV": "1"}, {"PICSONG_DWT_INV97": "0"}] if lossy else [])
    for env in modes:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = E.dwt_inverse(np.array(coef), wl, lossy, qs, extra=extra)
        assert np.array_equal(bits(got[extra:]), bits(inv)), f"synthesis {env}"
        got, fused = E.dwt_inverse_u8(np.array(coef), wl, lossy, qs, extra=extra)
        # the per-column path has no pixel store (fused = False: the caller clamps the samples, which the comparison above
        # has covered); its pixels are not compared and not counted
        assert fused == (path == "vec"), env
        if fused:
            assert np.array_equal(got, pix), f"pixels {env}"
        for k in env:
            monkeypatch.delenv(k)


def rgb_reference(W, H, wl, tf):
    key = ("rgb", W, H, wl, tf)
    if key not in _refs:
        lossy, qs = TRANSFORMS[tf]
        planes = [orc.gen_frame(W, H, 90 + c) for c in range(3)]
        planes[0][:11, :7] = 255; planes[1][:11, :7] = 0; planes[2][-9:, -6:] = 255; planes[0][-9:, -6:] = 0
        comps = orc.rgb_forward(*planes, lossy)
        coefs = [np.trunc(orc.dwt_forward(comps[k], wl, qs)[:W * H]).astype(np.int32).reshape(H, W) for k in range(3)]
        assert max(np.abs(c).max() for c in coefs) < 32768
        back = []
        for k in range(3):
            s, ex = orc.dwt_inverse(coefs[k], wl, lossy, qs)
            back.append(s[ex:].reshape(H, W))
        pix = orc.rgb_inverse(*back)
        assert (pix[0] == 0).any() and (pix[0] == 255).any()
        _refs[key] = (frozen(*planes), frozen(*coefs), frozen(*pix))
    return _refs[key]


def frame_case(monkeypatch, shape, bands, tf):
    """The frame paths' forms, which exist on the vector kernels only: int16 coefficients out of the forward transform and
    into the synthesis that writes pixels, and the RGB head and tails."""
    W, H, wl = shape
    lossy, qs = TRANSFORMS[tf]
    img, x, fwd, coef, inv, pix = reference(W, H, wl, tf)
    extra = orc.dwt_extra(W, H, wl)
    set_bands(monkeypatch, bands)
    monkeypatch.setenv("PICSONG_DWT_NOFUSE_INV", "1")           # levels 1 and 0 through the per-level kernels
    assert E.coef16_ok(lossy, wl, qs, 255, W, H)
    E.set_c16(True)
    try:
        for nofuse in (None, "1"):
            if nofuse:
                monkeypatch.setenv("PICSONG_DWT_NOFUSE01", nofuse)
            got = E.mallat16(E.dwt_forward(np.array(img), wl, lossy, qs, extra=extra), W, H)
            assert not (nofuse and E.dwt_forward.fused01)
            assert np.array_equal(got.astype(np.int32), np.trunc(fwd).astype(np.int32).reshape(H, W)), f"int16 forward, nofuse01={nofuse}"
            if not E.dwt_forward.fused01:
                break
        monkeypatch.delenv("PICSONG_DWT_NOFUSE01", raising=False)
    finally:
        E.set_c16(False)
    got, flags = E.dwt_inverse_u8_c16(coef.astype(np.int16), wl, lossy, qs, extra=extra)
    assert flags == 5, flags                                    # the 16-bit form, pixels from the finest level, one launch a level
    assert np.array_equal(got, pix), "int16 synthesis to pixels"
    planes, coefs, rgb_pix = rgb_reference(W, H, wl, tf)
    for nofuse in (None, "1"):
        if nofuse:
            monkeypatch.setenv("PICSONG_DWT_NOFUSE01", nofuse)
        got, fused = E.dwt_forward_rgb_forms(*[np.array(p) for p in planes], wl, extra, lossy, qs)
        assert not (nofuse and fused)
        for k in range(3):
            assert got[k].dtype == np.int16 and np.array_equal(got[k].astype(np.int32), coefs[k]), f"RGB forward, component {k}, nofuse01={nofuse}"
        if not fused:
            break
    got = E.dwt_inverse_rgb([c.astype(np.int16) for c in coefs], wl, extra, lossy, qs)
    assert got is not None
    for k in range(3):
        assert np.array_equal(got[k], rgb_pix[k]), f"RGB tail, plane {k}"


STAGE_CASES = [(s, b, p, t) for s in SHAPES for b in BAND_LISTS for p in ("vec", "novec") for t in TRANSFORMS]
FRAME_CASES = [(s, b, t) for s in C16_SHAPES for b in BAND_LISTS for t in TRANSFORMS]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape,bands,path,tf", STAGE_CASES, ids=_id)
def test_stage_calls_equal_oracle(monkeypatch, shape, bands, path, tf):
    stage_case(monkeypatch, shape, bands, path, tf)
    _done.add(("stage", shape, bands, path, tf))


@pytest.mark.parametrize("shape,bands,tf", FRAME_CASES, ids=_id)
def test_frame_path_forms_equal_oracle(monkeypatch, shape, bands, tf):
    frame_case(monkeypatch, shape, bands, tf)
    _done.add(("frame", shape, bands, tf))


@pytest.mark.parametrize("tf", ["53", "97q03"])
@pytest.mark.parametrize("bands", ["16", "mixed"])
def test_three_frames_in_one_call(monkeypatch, bands, tf):
    """grid.z = 3: frame z's arrays z strides on (dwt_fwd_select_frame / dwt_inv_select_frame), ragged tall bands."""
    W, H, wl = 320, 200, 3
    lossy, qs = TRANSFORMS[tf]
    refs = [reference(W, H, wl, tf, seed) for seed in (3, 4, 5)]
    extra = orc.dwt_extra(W, H, wl)
    set_bands(monkeypatch, bands)
    monkeypatch.setenv("PICSONG_DWT_NOFUSE01", "1")
    got = E.dwt_forward_n(np.stack([r[0] for r in refs]), wl, lossy, qs, extra)
    for z, r in enumerate(refs):
        assert np.array_equal(bits(got[z, :W * H]), bits(r[2])), f"forward, frame {z}"
    pix, fused = E.dwt_inverse_u8_n(np.stack([r[3] for r in refs]), wl, lossy, qs, extra)
    assert fused
    for z, r in enumerate(refs):
        assert np.array_equal(pix[z], r[5]), f"pixels, frame {z}"


# ---- level 0 restricted to a slice of rows (plan_restrict_band) ---------------------------------------------------------
# the first slicing divides into 8-row bands and not into taller ones (its last slice into all); the second into none,
# 4-row bands included: 22, 45 and 29 row pairs
SLICINGS = {"40+88+64": ((0, 40), (40, 88), (128, 64)), "44+90+58": ((0, 44), (44, 90), (134, 58))}


@pytest.mark.parametrize("tf", sorted(TRANSFORMS))
@pytest.mark.parametrize("path", ["vec", "novec"])
@pytest.mark.parametrize("bands", sorted(BAND_LISTS))
@pytest.mark.parametrize("slicing", sorted(SLICINGS))
def test_restricted_level_0_slices_equal_the_whole_transform(monkeypatch, slicing, bands, path, tf):
    """dwt_forward_band over three slices of the rows (pair_base / pair_end: the bands start at the slice, not at multiples
    of the band height, and the last one is clamped at the slice's end), then dwt_forward_tail: the unrestricted
    transform's words, which are the oracle's.  Rows outside a slice and its four-row halo are poison."""
    W, H, wl = 320, 192, 3
    lossy, qs = TRANSFORMS[tf]
    img, x, fwd, _, _, _ = reference(W, H, wl, tf)
    extra = orc.dwt_extra(W, H, wl)
    set_bands(monkeypatch, bands)
    if path == "novec":
        monkeypatch.setenv("PICSONG_DWT_NOVEC", "1")
    assert [b for b, _ in E.dwt_plan_bands(W, H, wl)[0]] == planned(bands, wl)
    monkeypatch.setenv("PICSONG_DWT_NOFUSE01", "1")
    whole = E.dwt_forward(np.array(img), wl, lossy, qs, extra=extra)
    out = E.aligned_zeros(W * H + extra, np.float32 if lossy else np.int32)
    out[:] = 12345
    for row0, rows in SLICINGS[slicing]:
        part = np.full((H, W), 0xA5, np.uint8)
        lo, hi = max(0, row0 - 4), min(H, row0 + rows + 4)
        part[lo:hi] = img[lo:hi]
        E.dwt_forward_band(E.aligned_copy(part), out, wl, lossy, qs, row0, rows)
    E.dwt_forward_tail(out, W, H, wl, lossy, qs)
    assert np.array_equal(bits(out[:W * H]), bits(whole[:W * H]))
    assert np.array_equal(bits(out[:W * H]), bits(fwd))


# ---- every kernel the selectors can return has been launched ------------------------------------------------------------
# label (emu_dwt_selector_kernels) -> why no launch of a plan can reach it.  Only unreachable combinations belong here; a
# reachable instantiation that the matrix misses fails the test below by its label.
UNREACHABLE = {}


def test_every_selector_kernel_was_launched(monkeypatch):
    for case in STAGE_CASES:                                    # (a partial selection: what it left out runs here)
        if ("stage",) + case not in _done:
            with monkeypatch.context() as m:
                stage_case(m, *case)
            _done.add(("stage",) + case)
    for case in FRAME_CASES:
        if ("frame",) + case not in _done:
            with monkeypatch.context() as m:
                frame_case(m, *case)
            _done.add(("frame",) + case)
    kernels = E.dwt_selector_kernels()
    # 32 forward (band x lossy x vec x u8) + 44 dwt_inv_kernel + 48 dwt_inv97_kernel + 12 RGB tails
    assert len(kernels) == 136, sorted(kernels.values())
    assert set(UNREACHABLE) <= set(kernels.values())
    launched = E.launch_log()
    missing = sorted(label for ptr, label in kernels.items() if ptr not in launched and label not in UNREACHABLE)
    assert not missing, "never launched: " + "; ".join(missing)
    stale = sorted(label for ptr, label in kernels.items() if ptr in launched and label in UNREACHABLE)
    assert not stale, "declared unreachable, yet launched: " + "; ".join(stale)
