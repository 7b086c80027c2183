"""The k = 0 encoder's plane records (an image of plane_lut<true> built once per table: bpc_kernels.hpp, plane_record)
and the one-wave-a-codeblock pack of the encoders' 16-bit staging.

On the CPU wave emulator (tests/hipemu/emu_plane_img_driver.cpp): the image against plane_lut<true> entry for entry, the
encoder reading the image against the oracle, the pack against po_bitstream_pack.  On the GPU (-m gpu): the context's
own images -- host tables, caller device tables, three tables in one launch, a table replaced between calls."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
from emu_lib import _geo, _p, driver_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = driver_lib("libpicsong_emu_plane_img.so", ("emu_plane_img_driver.cpp", "emu_runtime.cpp"))
    return _lib


WL = 2
# the shipped tables and the caller tables of oracle_lib.lut_shorten_sections / lut_cut_bitplanes (sections that end
# early: the clamp of an index past the table is part of what a record holds), a table short by a level and one with a
# single subband a level (its groups are not the image's slots)
TABLES = ["n1_lossless", "n1_lossy", "short4", "bp8", "wl-1", "nsub1"]


def _table(name, wl=WL):
    if name == "n1_lossless":
        return orc.lut_for(False, wl)
    if name == "n1_lossy":
        return orc.lut_for(True, wl)
    return orc.caller_table("k0", name, wl)


def _tab(lut):
    return np.ascontiguousarray(lut.table[:lut.total], np.int32)


def _image(lut, wl, by_kernel):
    img = np.full(4 * lib().emu_plane_img_recs(wl), 0xA5A5A5A5, np.uint32)
    tab, geo = _tab(lut), _geo(lut)
    lib().emu_plane_img_build(_p(tab), _p(geo), wl, int(by_kernel), _p(img))
    return img


@pytest.mark.parametrize("by_kernel", [False, True], ids=["host", "kernel"])
@pytest.mark.parametrize("wl", [2, 5])
@pytest.mark.parametrize("name", TABLES)
def test_image_equals_plane_lut_entry_for_entry(name, wl, by_kernel):
    """Every (group, bit-plane) the encoder can ask for -- level 0 .. wl, subband 0 .. 2, bit-plane 0 .. 15 -- read from
    the image is what plane_lut<true> returns from the byte table, field for field: built on the host (the context's
    own tables) and by plane_img_kernel (a caller's device table)."""
    lut = _table(name, wl)
    tab, geo = _tab(lut), _geo(lut)
    nsub = int(geo[1])
    img = _image(lut, wl, by_kernel)
    assert img.size == 4 * (3 * wl + 1) * 16
    want, got = np.zeros(6, np.uint32), np.zeros(6, np.uint32)
    for slot in range(3 * wl + 1):
        grp = (slot // 3) * nsub + slot % 3
        for bp in range(16):
            lib().emu_plane_lut_ref(_p(tab), _p(geo), grp, bp, _p(want))
            lib().emu_plane_lut_img(_p(img), slot, bp, _p(got))
            assert np.array_equal(want, got), (name, slot, bp, want, got)
            r = img[4 * (slot * 16 + bp):4 * (slot * 16 + bp) + 4]
            assert (r[0], r[1], r[2], r[3]) == (want[0], want[1], want[3], want[4] | (want[2] << 8))


def _encode_img(coefs, wl, luts):
    """k = 0 encode of len(coefs) frames in one launch, frame f with luts[f] through its image."""
    n = len(coefs)
    AH, AW = coefs[0].shape
    ncb = (AW // 64) * (AH // 64)
    coef = np.ascontiguousarray(np.stack(coefs), np.int32)
    tabs = [_tab(l) for l in luts]
    ptrs = (C.c_void_p * n)(*[t.ctypes.data for t in tabs])
    geo = _geo(luts[0])
    staging = np.empty(n * AW * AH, np.int32)
    sizes = np.zeros(n * ncb, np.int32)
    flag = np.zeros(1, np.int32)
    lib().emu_bpc_encode_img(_p(coef), AW, AH, wl, ptrs, _p(geo), n, _p(staging), _p(sizes), _p(flag))
    assert int(flag[0]) == 0
    return staging.reshape(n, AW * AH), sizes.reshape(n, ncb)


def _assert_staging(st, sz, st_o, sz_o):
    assert np.array_equal(sz, sz_o)
    for cb in range(sz_o.size):
        n = sz_o[cb]
        assert np.array_equal(st[cb * 4096:cb * 4096 + n], st_o[cb * 4096:cb * 4096 + n]), cb
        assert np.all(st[cb * 4096 + n:(cb + 1) * 4096] == -1), cb


@pytest.mark.parametrize("name", TABLES)
def test_encoder_reading_the_image_equals_oracle(name):
    """Codeblocks whose MSB reaches 15 in every subband (the bit-planes past a cut table's last, the groups past a short
    table's sections) and one raw block, coded through the image."""
    wl = 1 if name == "nsub1" else WL
    lut = _table(name, wl)
    coef = orc.deep_coeffs(256, 256, 17, raw_cb=15)
    st_o, sz_o = orc.bpc_encode(coef, wl, lut)
    st, sz = _encode_img([coef], wl, [lut])
    _assert_staging(st[0], sz[0], st_o, sz_o)


def test_three_tables_in_one_launch_equal_oracle():
    """The batched launch of an RGB frame's components: frame f codes with table f and ITS image."""
    luts = [orc.lut_for_component(False, WL, 0), orc.lut_for(True, WL), orc.lut_for_component(False, WL, 2)]
    assert len({tuple(_geo(l)) for l in luts}) == 1 and not np.array_equal(luts[0].table, luts[2].table)
    coefs = [orc.deep_coeffs(256, 192, 30 + f, raw_cb=3 + f) for f in range(3)]
    st, sz = _encode_img(coefs, WL, luts)
    for f in range(3):
        st_o, sz_o = orc.bpc_encode(coefs[f], WL, luts[f])
        _assert_staging(st[f], sz[f], st_o, sz_o)


# ---- pack ------------------------------------------------------------------------------------------------------------
# lengths 1, 2, 3, odd, even and 4096 (a raw block), each met at an even and at an odd stream offset (a codeblock's payload
# starts at short 9 + 2 n + sum of the lengths - 1 before it): chunk counts 0, 1, exactly n, n + a tail, two rounds
PACK_LENS = [1, 2, 3, 4096, 10, 9, 1, 2, 3, 4096, 2, 8, 10, 9, 17, 18, 4095, 2049, 2050, 2051, 1001, 1000, 4094, 4096, 7, 1, 3,
             513, 520, 4096, 16, 25, 24]


def _pack_case(seed, lens):
    rng = np.random.default_rng(seed)
    n = len(lens)
    st16 = rng.integers(0, 65536, n * 4096, dtype=np.uint32).astype(np.uint16)
    staging = np.full(n * 4096, -1, np.int32)
    for cb, ln in enumerate(lens):
        staging[cb * 4096:cb * 4096 + ln] = st16[cb * 4096:cb * 4096 + ln]
    return st16, staging, np.asarray(lens, np.int32)


def test_pack_lengths_cover_both_offset_parities():
    off, seen = 0, set()
    for ln in PACK_LENS:
        kind = ln if ln in (1, 2, 3, 4096) else ("odd" if ln & 1 else "even")
        seen.add((kind, off & 1))
        off += ln - 1
    assert seen == {(k, p) for k in (1, 2, 3, 4096, "odd", "even") for p in (0, 1)}


@pytest.mark.parametrize("with_header", [False, True])
def test_pack16_one_wave_a_codeblock_equals_oracle(with_header):
    """Two frames in one launch (blockIdx.y), the library's grid of four codeblocks a workgroup, against
    po_bitstream_pack; nothing is written past a stream's total."""
    lens1 = PACK_LENS[::-1] + [4096, 5]
    n = len(lens1)
    lens0 = PACK_LENS + [1] * (n - len(PACK_LENS))          # (one launch has one codeblock count)
    cases = [_pack_case(5, lens0), _pack_case(6, lens1)]
    hdr = orc.header_pack(n_samples=640 * 384, cp=2, cb_height=64, cb_width=64, wl=3, bit_depth=8, components=1,
                          height=384, bps=1, frames=7) if with_header else None
    stride = 9 + 2 * n + n * 4095 + 1 + 3                   # (odd: frame 1's stream starts at an odd short)
    out = np.full(2 * stride, 0x5A5A, np.uint16)
    st16 = np.concatenate([c[0] for c in cases])
    sizes = np.concatenate([c[2] for c in cases])
    totals = np.zeros(2, np.int32)
    hp = _p(np.ascontiguousarray(hdr, np.uint16)) if hdr is not None else None
    lib().emu_pack16_frames(_p(st16), _p(sizes), n, 2, hp, _p(out), C.c_size_t(stride), _p(totals))
    for f in range(2):
        ref = orc.bitstream_pack(cases[f][1], cases[f][2], hdr if f == 0 else None)
        assert totals[f] == ref.size
        assert np.array_equal(out[f * stride:f * stride + ref.size], ref), f
        assert np.all(out[f * stride + ref.size:(f + 1) * stride] == 0x5A5A), f


def test_pack16_from_a_workgroup_a_codeblock_grid_equals_oracle():
    """The kernel under a grid of one workgroup per codeblock (tests/hipemu/emu_driver.cpp launches it so): the waves
    past the last codeblock do nothing."""
    import emu_lib
    st16, staging, sizes = _pack_case(9, PACK_LENS)
    assert np.array_equal(emu_lib.pack16(st16, sizes), orc.bitstream_pack(staging, sizes))


# ---- GPU: the context's own images -----------------------------------------------------------------------------------
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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _info(pa, lut):
    info = pa.LutInfo()
    for k, v in lut.geometry().items():
        setattr(info, k, v)
    info.n_tables, info.cp = lut.n_tables, lut.cp
    return info


def _set(pa, torch, c, lut, setter, comp=0):
    """Returns the device table a "device" setter borrowed (the caller keeps it alive), else None."""
    info = _info(pa, lut)
    if setter == "host":
        pa._check(c.L.picsong_ctx_set_lut_component(c.h, comp, C.byref(info), _tab(lut).ctypes.data_as(C.c_void_p)))
        return None
    d = _dev(torch, _tab(lut))
    pa._check(c.L.picsong_ctx_set_lut_device(c.h, comp, C.byref(info), C.c_void_p(d.data_ptr())))
    return d


def _gpu_parity(torch, c, coef, img, wl, lut):
    st_o, sz_o = orc.bpc_encode(coef, wl, lut)
    st, sz = c.bpc_encode(_dev(torch, coef))
    st, sz = st.cpu().numpy(), sz.cpu().numpy()
    assert np.array_equal(sz, sz_o)
    for cb in range(sz_o.size):
        n = sz_o[cb]
        assert np.array_equal(st[cb * 4096:cb * 4096 + n], st_o[cb * 4096:cb * 4096 + n]), cb
    s = c.encode_frame(_dev(torch, orc.pad_frame(img)), 0)
    ref = orc.encode_frame(img, wl, False, 1.0, lut, 0, 0)
    assert np.array_equal(s.cpu().numpy().view(np.uint16), ref)
    assert c.range_flag() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("setter", ["host", "device"])
@pytest.mark.parametrize("name", TABLES)
def test_gpu_frame_with_each_table_equals_oracle(pa, torch, name, setter):
    wl = 1 if name == "nsub1" else WL
    lut = _table(name, wl)
    c = pa.Codec(256, 256, wl=wl)
    keep = _set(pa, torch, c, lut, setter)
    _gpu_parity(torch, c, orc.deep_coeffs(256, 256, 17, raw_cb=15), orc.gen_frame(256, 256, 3), wl, lut)
    torch.cuda.synchronize()
    c.close()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("setter", ["host", "device"])
def test_gpu_three_tables_in_one_launch_equal_oracle(pa, torch, setter):
    """picsong_encode_rgb_frame: component f with table f -- three different ones -- in one coder launch."""
    W, H, wl = 320, 192, 3
    luts = [orc.lut_for_component(False, wl, 2), orc.lut_for(True, wl), orc.lut_for_component(False, wl, 0)]
    planes = [orc.pad_frame(orc.gen_frame(W, H, 70 + k)) for k in range(3)]
    c = pa.Codec(W, H, wl=wl, rgb=True)
    keep = [_set(pa, torch, c, luts[k], setter, k) for k in range(3)]
    got = [g.clone() for g in c.encode_rgb_frame(*[_dev(torch, p) for p in planes], header_mask=0)]
    comps = orc.rgb_forward(*planes, False)
    for k in range(3):
        ref = orc.encode_plane(comps[k], wl, False, 1.0, luts[k], None)
        assert np.array_equal(got[k].cpu().numpy().view(np.uint16), ref), f"component {k}"
    torch.cuda.synchronize()
    c.close()
    del keep


@pytest.mark.gpu
def test_gpu_batched_frames_equal_oracle(pa, torch):
    """picsong_encode_frames: three frames of one launch, one table (and its one image)."""
    W, H, wl = 320, 192, 3
    lut = orc.lut_for(False, wl)
    imgs = [orc.gen_frame(W, H, 80 + f) for f in range(3)]
    c = pa.Codec(W, H, wl=wl)
    _set(pa, torch, c, lut, "host")
    frames = _dev(torch, np.stack([orc.pad_frame(i) for i in imgs]).reshape(3, -1))
    got = c.encode_frames(frames, 0)
    for f in range(3):
        ref = orc.encode_frame(imgs[f], wl, False, 1.0, lut, f, 0)
        assert np.array_equal(got[f].cpu().numpy().view(np.uint16), ref), f
    c.close()


@pytest.mark.gpu
def test_gpu_table_changed_between_calls(pa, torch):
    """A context codes with the table it holds NOW: replaced by either setter, and a caller's device table rewritten in
    place, as it could always be."""
    wl = WL
    a, b, s4 = orc.lut_for(False, wl), orc.lut_for(True, wl), orc.caller_table("k0", "short4", wl)
    coef, img = orc.deep_coeffs(256, 256, 21, raw_cb=7), orc.gen_frame(256, 256, 5)
    c = pa.Codec(256, 256, wl=wl)
    _set(pa, torch, c, a, "host")
    _gpu_parity(torch, c, coef, img, wl, a)
    _set(pa, torch, c, b, "host")
    _gpu_parity(torch, c, coef, img, wl, b)
    d = _set(pa, torch, c, s4, "device")
    _gpu_parity(torch, c, coef, img, wl, s4)
    _set(pa, torch, c, a, "host")
    _gpu_parity(torch, c, coef, img, wl, a)
    d = _set(pa, torch, c, a, "device")
    _gpu_parity(torch, c, coef, img, wl, a)
    assert _tab(a).size == _tab(b).size
    d.copy_(torch.from_numpy(_tab(b)))                       # the same device table, other entries
    torch.cuda.synchronize()
    _gpu_parity(torch, c, coef, img, wl, b)
    torch.cuda.synchronize()
    c.close()
    del d
