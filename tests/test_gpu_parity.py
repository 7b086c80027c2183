"""-m gpu: the HIP path (through the C ABI) against the CPU oracle, bit-exact for integer work and
for the fp32 9/7 path (explicit fmaf on both sides, contraction off), plus size-independent
properties at BASELINE.json's full sizes."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return t


@pytest.fixture(scope="module")
def pa():
    import picsong_amd
    picsong_amd.load()          # raises if the extension is missing
    return picsong_amd


def _lutdir(oracle, lossy):
    return os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("W,H,wl,lossy,qs", [
    (512, 512, 3, False, 1.0),        # BASELINE config 1 geometry
    (320, 192, 3, False, 1.0),
    (1000, 300, 4, False, 1.0),       # ragged -> padded 1024x320
    (512, 512, 3, True, 0.5),
    (832, 192, 4, True, 1.0),         # (AW >> 3)/2 odd: scalar store paths
])
def test_stage_by_stage_parity(oracle, pa, torch, W, H, wl, lossy, qs):
    img = oracle.pad_frame(oracle.gen_frame(W, H, 1))
    AH, AW = img.shape
    lut = oracle.lut_for(lossy, wl)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
    assert (c.aw, c.ah) == (AW, AH)
    d_img = _dev(torch, img)
    # level shift
    x_ref = oracle.level_shift_fwd(img, lossy)
    x = c.level_shift_fwd(d_img)
    assert np.array_equal(x.cpu().numpy().reshape(AH, AW), x_ref)
    # DWT forward (separate shift and fused u8 ingest)
    f_ref = oracle.dwt_forward(x_ref, wl, qs)
    P = AW * AH
    view = np.uint32 if lossy else np.int32
    for src in (x, d_img):
        f = c.dwt_forward(src).cpu().numpy()
        assert np.array_equal(f[:P].view(view), f_ref[:P].view(view))
    coef_ref = f_ref[:P].reshape(AH, AW)
    # BPC encode: staging + sizes
    st_ref, sz_ref = oracle.bpc_encode(coef_ref, wl, lut)
    st, sz = c.bpc_encode(_dev(torch, f_ref[:P]))
    assert c.range_flag() == 0
    assert np.array_equal(sz.cpu().numpy(), sz_ref)
    assert np.array_equal(st.cpu().numpy(), st_ref)
    # pack
    hdr = pa.header_pack(c.params)
    s_ref = oracle.bitstream_pack(st_ref, sz_ref, hdr)
    s = c.bitstream_pack(st, sz, hdr).cpu().numpy().view(np.uint16)
    assert np.array_equal(s, s_ref)
    s2 = c.bitstream_pack(st, sz, None).cpu().numpy().view(np.uint16)
    assert (s2[:9] == 0xFFFF).all() and np.array_equal(s2[9:], s_ref[9:])
    # unpack
    st2, sz2 = c.bitstream_unpack(_dev(torch, s_ref.view(np.int16)))
    assert np.array_equal(sz2.cpu().numpy(), sz_ref) and np.array_equal(st2.cpu().numpy(), st_ref)
    # BPC decode
    ci = np.trunc(coef_ref).astype(np.int32)
    dec = c.bpc_decode(st2, sz2).cpu().numpy().reshape(AH, AW)
    assert np.array_equal(dec, ci)
    # DWT inverse + inverse level shift
    inv_ref, extra = oracle.dwt_inverse(ci, wl, lossy, qs)
    inv = c.dwt_inverse(_dev(torch, ci))
    assert np.array_equal(inv.cpu().numpy()[extra:].view(view), inv_ref[extra:].view(view))
    pix_ref = oracle.level_shift_inv(inv_ref[extra:])
    pix = c.level_shift_inv(inv[extra:].clone()).cpu().numpy()
    assert np.array_equal(pix.view(view), pix_ref.view(view))
    c.close()


@pytest.mark.parametrize("W,H,wl,lossy,qs", [(512, 512, 3, False, 1.0), (700, 500, 4, False, 1.0),
                                             (512, 512, 5, True, 0.5), (640, 384, 3, True, 1.0)])
def test_frame_codestream_identical_to_oracle(oracle, pa, torch, W, H, wl, lossy, qs):
    img = oracle.gen_frame(W, H, 2)
    lut = oracle.lut_for(lossy, wl)
    ref = oracle.encode_frame(img, wl, lossy, qs, lut, 0, 0)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
    got = c.encode_frame(_dev(torch, oracle.pad_frame(img)), 0).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref)
    dec = c.decode_frame(_dev(torch, ref.view(np.int16))).cpu().numpy()[:H, :W]
    assert np.array_equal(dec, oracle.decode_frame(ref, W, H, wl, lossy, qs, lut))
    if not lossy:
        assert np.array_equal(dec, img)
    else:
        mse = np.mean((dec.astype(np.float64) - img) ** 2)
        assert 10 * np.log10(255 ** 2 / mse) > 40.0        # oracle and HIP are bit-identical; sanity
    c.close()


@pytest.mark.parametrize("name", ["zeros", "c255", "random", "impulse"])
def test_edge_inputs_roundtrip_and_oracle_parity(oracle, pa, torch, name):
    W, H, wl = 256, 192, 2
    rng = np.random.default_rng(9)
    img = {"zeros": np.zeros((H, W), np.uint8), "c255": np.full((H, W), 255, np.uint8),
           "random": rng.integers(0, 256, (H, W), dtype=np.uint8), "impulse": np.zeros((H, W), np.uint8)}[name]
    if name == "impulse":
        img[100, 77] = 255
    lut = oracle.lut_for(False, wl)
    ref = oracle.encode_frame(img, wl, False, 1.0, lut)
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    got = c.encode_frame(_dev(torch, oracle.pad_frame(img))).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref)
    assert np.array_equal(c.decode_frame(_dev(torch, got.view(np.int16))).cpu().numpy()[:H, :W], img)
    c.close()


@pytest.mark.parametrize("qs", [0.5, 0.3, 0.05])
def test_lossy_pixels_clamp_like_the_oracle(oracle, pa, torch, qs):
    """9/7 reconstruction of a frame of 0 / 255 pixels overshoots the pixel range on both sides all over the
    frame: the fused pixel store of the finest inverse level (v_cvt_pk_u8_f32's saturation) must clamp like
    removeOffsetAndApplyMaxMinLossy + the u8 conversion do (oracle), pixel for pixel; qs = 0.5 is the
    one-division form of the lean 9/7 kernel, 0.3 the two-division form, 0.05 coarse enough for big overshoots."""
    W, H, wl = 512, 320, 3
    rng = np.random.default_rng(31)
    img = (rng.integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8)
    img[:, :W // 2] = np.where(np.arange(W // 2)[None, :] // 7 % 2 == 0, 0, 255)     # hard vertical edges too
    lut = oracle.lut_for(True, wl)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=qs, lut_folder=_lutdir(oracle, True))
    s = c.encode_frame(_dev(torch, oracle.pad_frame(img))).cpu().numpy().view(np.uint16)
    assert np.array_equal(s, oracle.encode_frame(img, wl, True, qs, lut))
    want = oracle.decode_frame(s, W, H, wl, True, qs, lut)
    got = c.decode_frame(_dev(torch, s.view(np.int16))).cpu().numpy()
    assert np.array_equal(got[:H, :W], np.asarray(want)[:H, :W])
    assert (got == 0).mean() > 0.05 and (got == 255).mean() > 0.05
    c.close()


def test_raw_fallback_and_mixed_blocks(oracle, pa, torch):
    rng = np.random.default_rng(4)
    coef = np.zeros((64, 256), np.int32)
    coef[:, 0:64] = rng.integers(-30000, 30000, (64, 64))
    coef[:, 128:192] = rng.integers(-1, 2, (64, 64))
    coef[:, 192:256] = (rng.standard_normal((64, 64)) * 600).astype(np.int32)
    lut = oracle.lut_for(False, 1)
    st_ref, sz_ref = oracle.bpc_encode(coef, 1, lut)
    c = pa.Codec(256, 64, wl=1, lut_folder=_lutdir(oracle, False))
    st, sz = c.bpc_encode(_dev(torch, coef))
    assert np.array_equal(sz.cpu().numpy(), sz_ref) and np.array_equal(st.cpu().numpy(), st_ref)
    assert np.array_equal(c.bpc_decode(st, sz).cpu().numpy().reshape(64, 256), coef)
    c.close()


def test_wl6_lut_holes_behaviour(oracle, pa, torch):
    """BASELINE config 3 geometry in miniature (wl = 6, lossy): the three never-written LUT groups
    (zero-filled) drive level-5 LH/HH and LL codeblocks into the raw fallback; HIP == oracle."""
    W, H, wl, qs = 2048, 2048, 6, 0.5
    img = oracle.gen_frame(W, H, 0)
    lut = oracle.lut_for(True, wl)
    ref = oracle.encode_frame(img, wl, True, qs, lut)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=qs, lut_folder=_lutdir(oracle, True))
    got = c.encode_frame(_dev(torch, img)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref)
    dec = c.decode_frame(_dev(torch, got.view(np.int16))).cpu().numpy()
    assert np.array_equal(dec, oracle.decode_frame(ref, W, H, wl, True, qs, lut))
    c.close()


def test_repeated_decodes_leave_the_same_pixels(oracle, pa, torch):
    """Forty decodes of one 9/7 wl = 6 codestream, each compared with the oracle's pixels.  A hazard between a wide
    buffer store and the next vector instruction (the compiler's hazard recognizer exempts buffer
    stores with a scalar offset, gfx950 does not) showed as a few wrong samples in one decode of fifteen, never in the
    first one of a process: a single comparison per test does not see that kind of fault."""
    W, H, wl, qs = 2048, 2048, 6, 0.5
    img = oracle.gen_frame(W, H, 0)
    lut = oracle.lut_for(True, wl)
    ref = oracle.encode_frame(img, wl, True, qs, lut)
    want = oracle.decode_frame(ref, W, H, wl, True, qs, lut)
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=qs, lut_folder=_lutdir(oracle, True))
    s = _dev(torch, ref.view(np.int16))
    d_want = _dev(torch, np.ascontiguousarray(want))
    bad = [i for i in range(40) if not torch.equal(c.decode_frame(s)[:H, :W], d_want)]
    assert bad == []
    # the 5/3 path the same way
    lut0 = oracle.lut_for(False, 5)
    c0 = pa.Codec(W, H, wl=5, lut_folder=_lutdir(oracle, False))
    d_img = _dev(torch, oracle.pad_frame(img))
    s0 = c0.encode_frame(d_img).clone()
    bad = [i for i in range(40) if not torch.equal(c0.decode_frame(s0), d_img.view(c0.ah, c0.aw))]
    assert bad == []
    c.close(); c0.close()


def test_missing_lut_is_an_error(pa, torch):
    c = pa.Codec(256, 256, wl=2)
    with pytest.raises(pa.PicsongError):
        c.bpc_encode(torch.zeros(256 * 256, dtype=torch.int32, device="cuda"))
    c.close()


# ---- full BASELINE sizes: the whole codestream against the oracle (OpenMP over codeblocks and DWT
# rows on all of the box's cores: well under a second per 8K frame), then size-independent properties
def _gen_device(torch, oracle, W, H, f=0):
    return _dev(torch, oracle.pad_frame(oracle.gen_frame(W, H, f)))


@pytest.mark.parametrize("W,H,wl,lossy,qs", [
    (3840, 2160, 5, False, 1.0),      # BASELINE configs[1]: 4K, -type 0, wl 5
    (7680, 4320, 5, False, 1.0),      # the metric's workload: 8K, -type 0, wl 5
    (7680, 4320, 6, True, 0.5),       # BASELINE configs[2]: 8K, -type 1, qs 0.5, wl 6
])
def test_full_size_codestream_equals_oracle(oracle, pa, torch, W, H, wl, lossy, qs):
    """Every BASELINE single-frame configuration at its full size: header, per-codeblock (MSB, length)
    table, payload and the trailing short of the HIP codestream equal the oracle's, and the HIP decode of
    it equals the oracle's decode (CodingEngine::runImage Engines/CodingEngine.cu:634-674,713-751;
    DecodingEngine::runImage Engines/DecodingEngine.cu:770-794)."""
    oracle.set_threads(oracle.usable_threads())
    try:
        img = oracle.gen_frame(W, H, 0)
        lut = oracle.lut_for(lossy, wl)
        ref = oracle.encode_frame(img, wl, lossy, qs, lut)
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
        frame = _dev(torch, oracle.pad_frame(img))
        s = c.encode_frame(frame, 0)
        got = s.cpu().numpy().view(np.uint16)
        ncb = c.ncb
        assert got.size == ref.size
        assert np.array_equal(got[:9], ref[:9])                                            # header
        assert np.array_equal(got[9:9 + 2 * ncb:2], ref[9:9 + 2 * ncb:2])                  # MSB per codeblock
        assert np.array_equal(got[10:10 + 2 * ncb:2], ref[10:10 + 2 * ncb:2])              # sizeArray
        assert np.array_equal(got, ref)                                                    # everything
        dec = c.decode_frame(s).cpu().numpy()
        ref_dec = oracle.decode_frame(ref, W, H, wl, lossy, qs, lut)
        assert np.array_equal(dec[:H, :W], ref_dec[:H, :W])
        if not lossy:
            assert np.array_equal(dec[:H, :W], img)
        c.close()
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("W,H,wl,lossy,qs,n,first", [
    (640, 448, 3, False, 1.0, 5, 0),       # frame 0 of the video in the batch: header on it alone
    (640, 448, 3, False, 1.0, 3, 7),       # later frames: no header
    (576, 320, 3, False, 1.0, 4, -2),      # 45 codeblocks (odd: the last wave of a frame is half empty), frame 0 third
    (512, 512, 4, True, 0.5, 2, 0),
    (3840, 2160, 5, False, 1.0, 4, 0),     # BASELINE configs[3]'s frames, four to a launch
])
def test_batched_frames_equal_oracle(oracle, pa, torch, W, H, wl, lossy, qs, n, first):
    """picsong_encode_frames: n frames through one launch per stage == the oracle's frame-by-frame streams
    (CodingEngine::runVideo Engines/CodingEngine.cu:819-872; header on the video's frame 0 only,
    BitStreamBuilder.cu:277-278)."""
    oracle.set_threads(oracle.usable_threads())
    try:
        lut = oracle.lut_for(lossy, wl)
        imgs = [oracle.gen_frame(W, H, 20 + i) for i in range(n)]
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
        frames = _dev(torch, np.stack([oracle.pad_frame(im).reshape(-1) for im in imgs]))
        got = c.encode_frames(frames, first)
        assert c.range_flag() == 0
        for i in range(n):
            ref = oracle.encode_frame(imgs[i], wl, lossy, qs, lut, 0 if first + i == 0 else 1)
            g = got[i].cpu().numpy().view(np.uint16)
            assert g.size == ref.size and np.array_equal(g, ref), f"frame {i} of the batch differs from the oracle"
        # a smaller batch on the same context afterwards, and the single-frame path, still agree
        one = c.encode_frame(frames[1], 1).cpu().numpy().view(np.uint16)
        two = c.encode_frames(frames[:2], 5)
        assert np.array_equal(two[1].cpu().numpy().view(np.uint16), one)
        c.close()
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("W,H,wl,lossy", [(512, 512, 3, False), (1000, 300, 4, False), (832, 192, 4, True),
                                          (3840, 2160, 5, False)])
def test_three_coding_passes_equal_oracle(oracle, pa, torch, W, H, wl, lossy):
    """-cp 3 (kernelBPCCoder3CP / kernelBPCDecoder3CP BPC/BPCEngine.cu:2029-2121,2221-2299): the HIP codestream
    equals the oracle's, and the HIP decode of it the oracle's decode."""
    oracle.set_threads(oracle.usable_threads())
    try:
        qs = 0.5 if lossy else 1.0
        img = oracle.gen_frame(W, H, 3)
        lut = oracle.lut_for_cp3(lossy, wl)
        ref = oracle.encode_frame(img, wl, lossy, qs, lut)
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, cp=3,
                     lut_folder=os.path.join(oracle.LUT_CP3_DIR, "n1_lossy" if lossy else "n1_lossless"))
        s = c.encode_frame(_dev(torch, oracle.pad_frame(img)), 0)
        got = s.cpu().numpy().view(np.uint16)
        assert c.range_flag() == 0
        assert got.size == ref.size and np.array_equal(got, ref)
        dec = c.decode_frame(s).cpu().numpy()
        assert np.array_equal(dec[:H, :W], oracle.decode_frame(ref, W, H, wl, lossy, qs, lut))
        c.close()
    finally:
        oracle.set_threads(1)


def test_lds_atomic_reservation_order(pa, torch):
    """The coder takes codeword slots with one LDS atomic add per requesting lane; lanes of one instruction
    that hit one counter must be served in ascending lane order (== v_mbcnt rank).  16 M random lane masks."""
    import ctypes as C
    bad = C.c_int(-1)
    assert pa.load().picsong_selftest_lds_order(0, C.byref(bad)) == 0
    assert bad.value == 0


@pytest.mark.parametrize("W,H,wl,lossy,qs,n", [
    (640, 448, 3, False, 1.0, 5),
    (576, 320, 3, False, 1.0, 4),        # 45 codeblocks: the last wave of a frame is half empty
    (512, 512, 4, True, 0.5, 2),
    (3840, 2160, 5, False, 1.0, 4),      # BASELINE configs[3]'s frames, four to a launch
    (1000, 300, 4, True, 0.7, 3),        # padded width not a multiple of 4 levels' vector widths at every level
])
def test_batched_decode_equals_frame_by_frame_and_oracle(oracle, pa, torch, W, H, wl, lossy, qs, n):
    """picsong_decode_frames: n codestreams through one launch per stage give the frames of n picsong_decode_frame
    calls -- and, lossless, the original frames; 9/7: the oracle's decode of the same streams."""
    oracle.set_threads(oracle.usable_threads())
    try:
        lut = oracle.lut_for(lossy, wl)
        imgs = [oracle.gen_frame(W, H, 40 + i) for i in range(n)]
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
        frames = _dev(torch, np.stack([oracle.pad_frame(im).reshape(-1) for im in imgs]))
        streams = torch.full((n, c.max_stream_shorts()), -1, dtype=torch.int16, device="cuda")
        c.encode_frames_async(frames, streams, 0)
        totals = c.last_totals(n)
        got = c.decode_frames(streams)
        assert c.range_flag() == 0
        for i in range(n):
            one = c.decode_frame(streams[i, :totals[i]].clone())
            assert torch.equal(got[i], one), f"frame {i}: batched decode differs from the single-frame decode"
            if lossy:
                ref = oracle.decode_frame(streams[i, :totals[i]].cpu().numpy().view(np.uint16), W, H, wl, lossy, qs, lut)
                assert np.array_equal(got[i].cpu().numpy()[:H, :W], ref)
            else:
                assert np.array_equal(got[i].cpu().numpy()[:H, :W], imgs[i])
        # a smaller batch on the same context afterwards
        two = c.decode_frames(streams[:2])
        assert torch.equal(two[1], got[1])
        with pytest.raises(pa.PicsongError):
            c.decode_frames(torch.zeros((2, 100), dtype=torch.int16, device="cuda"))     # too short a stride
        c.close()
    finally:
        oracle.set_threads(1)


def test_copy_last_totals_matches_the_waited_for_lengths(oracle, pa, torch):
    """picsong_copy_last_totals: the lengths of the most recent single-frame / batched call, copied on the device
    without a wait, are the ones picsong_last_total(s) returns after one; the count is checked against the call."""
    W, H, wl = 640, 448, 3
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    frames = _dev(torch, np.stack([oracle.pad_frame(oracle.gen_frame(W, H, 30 + i)).reshape(-1) for i in range(3)]))
    out = torch.empty((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    d = torch.zeros(4, dtype=torch.int32, device="cuda")
    c.encode_frame_async(frames[0], out[0], 0)
    c.copy_last_totals(1, d[3:4])
    assert c.last_total() == int(d[3].item())
    c.encode_frames_async(frames, out, 1)
    c.copy_last_totals(3, d)
    assert c.last_totals(3) == d[:3].tolist() and int(d[3].item()) != 0
    with pytest.raises(pa.PicsongError):
        c.copy_last_totals(4, torch.zeros(4, dtype=torch.int32, device="cuda"))     # the batch had three
    c.encode_frame_async(frames[1], out[1], 1)                                       # a single frame again
    c.copy_last_totals(1, d[0:1])
    assert c.last_total() == int(d[0].item())
    c.close()


@pytest.mark.parametrize("W,H,wl,lossy,qs,k,n,hint", [(576, 320, 3, False, 1.0, 0.5, 3, False), (512, 512, 5, False, 1.0, 1.5, 2, True),
                                                      (640, 384, 3, True, 0.5, 0.7, 4, True)])
def test_batched_frames_of_a_complexity_scalable_context(oracle, pa, torch, W, H, wl, lossy, qs, k, n, hint):
    """picsong_encode_frames / picsong_decode_frames of a -k > 0 context: the BULK coder instantiations over the n frames
    of one launch (both of the encoder's; 45 codeblocks: the last wave of a frame half empty) -- the oracle's streams
    frame by frame, header on the video's frame 0 only, and the decode the single-frame decode's and the oracle's."""
    oracle.set_threads(oracle.usable_threads())
    try:
        lut = oracle.lut_for_k(lossy, wl)
        imgs = [oracle.gen_frame(W, H, 70 + i) for i in range(n)]
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), k=k, pipelined=hint)
        frames = _dev(torch, np.stack([oracle.pad_frame(im).reshape(-1) for im in imgs]))
        streams = torch.full((n, c.max_stream_shorts()), -1, dtype=torch.int16, device="cuda")
        c.encode_frames_async(frames, streams, 0)
        totals = c.last_totals(n)
        assert c.range_flag() == 0
        refs = [oracle.encode_frame(imgs[i], wl, lossy, qs, lut, 0 if i == 0 else 1, 0, k=k) for i in range(n)]
        for i in range(n):
            g = streams[i, :totals[i]].cpu().numpy().view(np.uint16)
            assert g.size == refs[i].size and np.array_equal(g, refs[i]), f"frame {i} of the batch differs from the oracle"
        got = c.decode_frames(streams)
        for i in range(n):
            assert torch.equal(got[i], c.decode_frame(streams[i, :totals[i]].clone())), f"frame {i}: batched decode"
            ref = oracle.decode_frame(refs[i], W, H, wl, lossy, qs, lut, k=k)
            assert np.array_equal(got[i].cpu().numpy()[:H, :W], ref)
        c.close()
    finally:
        oracle.set_threads(1)


def test_batched_frames_argument_checks(oracle, pa, torch):
    c = pa.Codec(256, 256, wl=2, lut_folder=_lutdir(oracle, False))
    frames = torch.zeros((2, c.P), dtype=torch.uint8, device="cuda")
    out = torch.empty((2, c.max_stream_shorts() - 1), dtype=torch.int16, device="cuda")      # too short a stride
    with pytest.raises(pa.PicsongError):
        c.encode_frames_async(frames, out, 0)
    with pytest.raises(pa.PicsongError):
        c.last_totals(3)
    c.close()
    # an RGB context codes component by component (picsong_encode_plane): the batched grey path refuses it
    c = pa.Codec(256, 256, wl=2, lut_folder=_lutdir(oracle, False), rgb=True)
    out = torch.empty((2, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    with pytest.raises(pa.PicsongError):
        c.encode_frames_async(frames, out, 0)
    c.close()


def test_copy_last_totals_follows_every_call_that_packs_a_stream(oracle, pa, torch):
    """After a batched encode, a stripe (or any other single-stream pack) makes ITS length the most recent total --
    not the stale first length of the batch --, and a batched decode leaves no encode totals to hand out."""
    W, H, wl = 512, 320, 3
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    frames = _dev(torch, np.stack([oracle.pad_frame(oracle.gen_frame(W, H, 40 + i)).reshape(-1) for i in range(2)]))
    out = torch.empty((2, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    d = torch.zeros(2, dtype=torch.int32, device="cuda")
    c.encode_frames_async(frames, out, 1)
    batch = c.last_totals(2)
    mini = c.encode_frame_stripe(frames[1], 3, 5)
    c.copy_last_totals(1, d[0:1])
    assert int(d[0].item()) == mini.numel() != batch[0]
    with pytest.raises(pa.PicsongError):
        c.copy_last_totals(2, d)                                                      # the batch is no longer the last call
    c.encode_frames_async(frames, out, 1)
    streams = torch.stack([out[0], out[1]])
    dec = c.decode_frames(streams)
    assert torch.equal(dec[0].view(-1), frames[0]) and torch.equal(dec[1].view(-1), frames[1])
    with pytest.raises(pa.PicsongError):
        c.copy_last_totals(2, d)
    c.close()


def test_borrowed_device_table_follows_the_contexts_coding_passes(oracle, pa, torch):
    """picsong_ctx_set_lut_device: a -cp 3 context takes a five-section device table (and codes with it like the host
    path's copy); a table declared for the other mode is refused instead of being read out of bounds."""
    import ctypes as C
    W, H, wl = 256, 192, 2
    img = oracle.gen_frame(W, H, 50)
    frame = _dev(torch, oracle.pad_frame(img))
    lut3 = os.path.join(oracle.LUT_CP3_DIR, "n1_lossless")
    info3, table3 = pa.lut_load(lut3, wl, 1, 0, 1, 3)
    c = pa.Codec(W, H, wl=wl, cp=3)
    d_table = torch.from_numpy(np.ascontiguousarray(table3, np.int32)).cuda()
    pa._check(c.L.picsong_ctx_set_lut_device(c.h, 0, C.byref(info3), C.c_void_p(d_table.data_ptr())))
    got = c.encode_frame(frame, 0)
    ref = pa.Codec(W, H, wl=wl, cp=3, lut_folder=lut3)
    assert torch.equal(got, ref.encode_frame(frame, 0))
    info2, table2 = pa.lut_load(_lutdir(oracle, False), wl, 1, 0, 1, 2)
    d2 = torch.from_numpy(np.ascontiguousarray(table2, np.int32)).cuda()
    with pytest.raises(pa.PicsongError):
        pa._check(c.L.picsong_ctx_set_lut_device(c.h, 0, C.byref(info2), C.c_void_p(d2.data_ptr())))
    c.close(); ref.close()


@pytest.mark.parametrize("W,H,wl", [(3840, 2160, 5), (7680, 4320, 5)])
def test_full_size_lossless_roundtrip(oracle, pa, torch, W, H, wl):
    """configs[1] (4K) and the headline 8K lossless workload: encode -> decode is the identity."""
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    frame = _gen_device(torch, oracle, W, H)
    s = c.encode_frame(frame)
    assert c.range_flag() == 0
    sn = s.cpu().numpy().view(np.uint16)
    ncb = c.ncb
    assert sn[-1] == 0xFFFF
    assert sn.size == 9 + 2 * ncb + int((sn[10:10 + 2 * ncb:2].astype(np.int64) - 1).sum()) + 1
    hp = pa.header_unpack(sn[:9])
    assert (hp.width, hp.height, hp.wl, hp.lossy) == (W, H, wl, 0)
    dec = c.decode_frame(s)
    assert torch.equal(dec, frame.view(c.ah, c.aw))
    # determinism: a second encode of the same frame gives the same bytes
    s2 = c.encode_frame(frame)
    assert zlib.crc32(s2.cpu().numpy().tobytes()) == zlib.crc32(sn.tobytes())
    c.close()


def test_full_size_8k_lossy_psnr(oracle, pa, torch):
    """configs[2]: 8K, 9/7, qs = 0.5, wl = 6.  Stated tolerance: PSNR >= 40 dB on the synthetic
    frame (the oracle gives 49.6 dB at 512^2 with these settings; HIP is bit-identical to it)."""
    W, H, wl, qs = 7680, 4320, 6, 0.5
    c = pa.Codec(W, H, wl=wl, lossy=True, qs=qs, lut_folder=_lutdir(oracle, True))
    frame = _gen_device(torch, oracle, W, H)
    s = c.encode_frame(frame)
    dec = c.decode_frame(s)
    a = dec[:H, :W].float()
    b = frame.view(c.ah, c.aw)[:H, :W].float()
    mse = torch.mean((a - b) ** 2).item()
    assert 10 * np.log10(255 ** 2 / mse) >= 40.0
    assert s.numel() * 2 < W * H           # it compresses
    c.close()


def test_dwt_linearity_full_size(pa, torch, oracle):
    """5/3 without rounding effects: DWT(2^k * x) of a smooth input scales exactly for the
    constant image; and DWT of constant c has LL = c, all detail = 0 at 8K."""
    W, H, wl = 7680, 4352, 5
    c = pa.Codec(W, H, wl=wl)
    x = torch.full((H * W,), 37, dtype=torch.int32, device="cuda")
    f = c.dwt_forward(x)[:H * W].view(H, W)
    assert (f[:H >> wl, :W >> wl] == 37).all()
    assert (f[H >> wl:, :] == 0).all() and (f[:, W >> wl:] == 0).all()
    c.close()


def test_codeblock_stripes_equal_full_frame(oracle, pa, torch):
    """Intra-frame sharding on one GPU: the frame coded as 3 uneven stripes and spliced by
    picsong_dist.splice_stripes is byte-identical to the whole-frame codestream."""
    import picsong_dist as pd
    W, H, wl = 640, 448, 3
    img = oracle.gen_frame(W, H, 4)
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    frame = _dev(torch, oracle.pad_frame(img))
    full = c.encode_frame(frame, 0)
    ranges = pd.stripe_ranges(c.ncb, 3)
    minis = [c.encode_frame_stripe(frame, b, n).clone() for b, n in ranges]
    hdr = torch.from_numpy(pa.header_pack(c.params).view(np.int16).copy()).cuda()
    spliced = pd.splice_stripes(hdr, minis, [n for _, n in ranges])
    assert torch.equal(spliced, full)
    ref = oracle.encode_frame(img, wl, False, 1.0, oracle.lut_for(False, wl))
    assert np.array_equal(spliced.cpu().numpy().view(np.uint16), ref)
    with pytest.raises(pa.PicsongError):
        c.encode_frame_stripe(frame, c.ncb - 1, 2)
    c.close()


def test_config5_16k_single_frame_roundtrip(oracle, pa, torch):
    """BASELINE config 5 geometry on one GPU: 16384 x 16384, -type 0, wl 5, 65,536 codeblocks."""
    W = H = 16384
    c = pa.Codec(W, H, wl=5, lut_folder=_lutdir(oracle, False))
    assert c.ncb == 65536
    tile = torch.from_numpy(oracle.gen_frame(2048, 2048, 1)).cuda()
    frame = tile.repeat(8, 8).contiguous()
    frame[5000:5064, 7000:7064] = torch.randint(0, 256, (64, 64), dtype=torch.uint8, device="cuda")
    s = c.encode_frame(frame)
    assert c.range_flag() == 0
    # the WHOLE codestream against the oracle at full size (header, MSB / length table, payload): the oracle's
    # OpenMP loops on all of the box's cores take a few seconds for the 268 Mpixel frame
    oracle.set_threads(oracle.usable_threads())
    ref = oracle.encode_frame(frame.cpu().numpy(), 5, False, 1.0, oracle.lut_for(False, 5))
    oracle.set_threads(1)
    assert ref.size == s.numel()
    assert np.array_equal(s.cpu().numpy().view(np.uint16), ref)
    del ref
    dec = c.decode_frame(s)
    assert torch.equal(dec, frame)
    # two stripes of the same frame splice to the same bytes
    import picsong_dist as pd
    ranges = pd.stripe_ranges(c.ncb, 2)
    minis = [c.encode_frame_stripe(frame, b, n).clone() for b, n in ranges]
    hdr = torch.from_numpy(pa.header_pack(c.params).view(np.int16).copy()).cuda()
    assert torch.equal(pd.splice_stripes(hdr, minis, [n for _, n in ranges]), s)
    c.close()


@pytest.mark.parametrize("W,H,wl,lossy,world", [(512, 512, 3, False, 4), (384, 256, 2, True, 2), (16384, 16384, 5, False, 8)])
def test_banded_transform_sharding_equals_full_frame(oracle, pa, torch, W, H, wl, lossy, world):
    """SURVEY 8e / BASELINE config 5 with the transform sharded too, the `world` ranks played one after the
    other on one GPU: rank k transforms only its row band (picsong_dwt_forward_band) from a buffer that holds
    nothing but the band and its 4-row halo, the LL1 bands are exchanged (here: device copies, on a node:
    one all-gather), every rank runs levels >= 1 (picsong_dwt_forward_tail) and codes its two stripes
    (picsong_encode_stripe_coded); the splice equals picsong_encode_frame's stream byte for byte."""
    import picsong_dist as pd
    qs = 0.5 if lossy else 1.0
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
    AW, AH, P = c.aw, c.ah, c.P
    if W * H > (1 << 24):
        tile = torch.from_numpy(oracle.gen_frame(2048, 2048, 1)).cuda()
        frame = tile.repeat(AH // 2048, AW // 2048).contiguous()
    else:
        frame = _dev(torch, oracle.pad_frame(oracle.gen_frame(W, H, 6)))
    full = c.encode_frame(frame.view(-1), 0).clone()
    plan = pd.band_plan(AW, AH, world)
    assert plan is not None
    n_ll1 = (AW // 2) * (AH // 2)
    coefs = []
    for k, p in enumerate(plan):
        x = torch.full((AH, AW), 0xA5, dtype=torch.uint8, device="cuda")
        lo, hi = max(0, p["row0"] - 4), min(AH, p["row0"] + p["rows"] + 4)
        x[lo:hi] = frame.view(AH, AW)[lo:hi]
        coef = c.new_coef_buffer()
        c.dwt_forward_band(x.view(-1), p["row0"], p["rows"], coef)
        torch.cuda.synchronize()
        coefs.append(coef)
    ll1 = torch.cat([coefs[k][P + p["ll1_begin"]:P + p["ll1_begin"] + p["ll1_count"]] for k, p in enumerate(plan)])
    minis = [[], []]
    for k, p in enumerate(plan):
        coefs[k][P:P + n_ll1] = ll1                              # the all-gather
        c.dwt_forward_tail(coefs[k])
        for h, (b, n) in enumerate(p["stripes"]):
            minis[h].append(c.encode_stripe_coded(coefs[k], b, n).clone())
        coefs[k] = None
    hdr = torch.from_numpy(pa.header_pack(c.params).view(np.int16).copy()).cuda()
    counts = [p["stripes"][0][1] for p in plan] + [p["stripes"][1][1] for p in plan]
    spliced = pd.splice_stripes(hdr, minis[0] + minis[1], counts)
    assert torch.equal(spliced, full)
    # ... and the oracle's stream for the same frame, not only HIP's own (config 5 at full size included)
    oracle.set_threads(oracle.usable_threads())
    ref = oracle.encode_frame(frame.view(AH, AW)[:H, :W].cpu().numpy(), wl, lossy, qs, oracle.lut_for(lossy, wl))
    oracle.set_threads(1)
    assert np.array_equal(spliced.cpu().numpy().view(np.uint16), ref)
    c.close()


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_rgb_components_parity(oracle, pa, torch, lossy, qs):
    """RGB row: colour transform + per-component LUT streams identical to the oracle, decode_plane +
    inverse transform returns the planes (exactly for RCT)."""
    W, H, wl = 320, 192, 3
    planes = [oracle.pad_frame(oracle.gen_frame(W, H, 20 + c)) for c in range(3)]
    AH, AW = planes[0].shape
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), rgb=True)
    d = [_dev(torch, p) for p in planes]
    comps = c.rgb_forward(*d)
    ref_comps = oracle.rgb_forward(*planes, lossy)
    view = np.uint32 if lossy else np.int32
    hdr = pa.header_pack(c.params)
    assert pa.header_unpack(hdr).is_rgb == 1 and pa.header_unpack(hdr).components == 3
    decoded = []
    for k in range(3):
        assert np.array_equal(comps[k].cpu().numpy().view(view), ref_comps[k].ravel().view(view))
        ref = oracle.encode_plane(ref_comps[k], wl, lossy, qs, oracle.lut_for_component(lossy, wl, k),
                                  hdr if k == 0 else None)
        got = c.encode_plane(comps[k], k, k == 0)
        assert np.array_equal(got.cpu().numpy().view(np.uint16), ref)
        dp = c.decode_plane(got.clone(), k).clone()
        ref_dp = oracle.decode_plane(ref, AW, AH, wl, lossy, qs, oracle.lut_for_component(lossy, wl, k))
        assert np.array_equal(dp.cpu().numpy().view(view), ref_dp.ravel().view(view))
        decoded.append(dp)
    back = c.rgb_inverse(*decoded)
    ref_back = oracle.rgb_inverse(*[x.cpu().numpy().reshape(AH, AW) for x in decoded])
    for k in range(3):
        assert np.array_equal(back[k].cpu().numpy(), ref_back[k])
        if not lossy:
            assert np.array_equal(back[k].cpu().numpy(), planes[k])
    c.close()


@pytest.mark.parametrize("W,H,wl,lossy,qs", [(3840, 2160, 5, False, 1.0), (1280, 704, 6, True, 0.5), (700, 500, 4, False, 1.0)])
def test_16_bit_and_32_bit_coefficient_forms_agree(oracle, pa, torch, monkeypatch, W, H, wl, lossy, qs):
    """The encode frame paths carry their coded coefficients as int16 between transform and coder (default) or as the
    reference's 32-bit arrays (PICSONG_C16=0): same codestream -- the oracle's --, single frames and batched calls."""
    img = oracle.gen_frame(W, H, 70)
    frame = _dev(torch, oracle.pad_frame(img))
    ref = oracle.encode_frame(img, wl, lossy, qs, oracle.lut_for(lossy, wl))
    results = []
    for c16 in ("1", "0"):
        monkeypatch.setenv("PICSONG_C16", c16)
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
        s = c.encode_frame(frame, 0).clone()
        assert np.array_equal(s.cpu().numpy().view(np.uint16), ref), c16
        two = torch.stack([frame.view(-1), frame.view(-1)])
        out = torch.empty((2, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
        c.encode_frames_async(two, out, 0)
        t = c.last_totals(2)
        assert t[0] == s.numel() and torch.equal(out[0, :t[0]], s) and torch.equal(out[1, 9:t[1]], s[9:])
        pix = c.decode_frame(s).clone()
        both = c.decode_frames(out)
        assert torch.equal(both[0], pix) and torch.equal(both[1], pix) and c.range_flag() == 0
        results.append(pix)
        c.close()
    assert torch.equal(results[0], results[1])
    assert np.array_equal(results[0].cpu().numpy()[:H, :W], oracle.decode_frame(ref, W, H, wl, lossy, qs, oracle.lut_for(lossy, wl)))


@pytest.mark.parametrize("W,H,wl,lossy,qs", [(3840, 2160, 5, False, 1.0), (1920, 1080, 6, True, 0.5), (700, 500, 4, False, 1.0),
                                             (1000, 300, 3, True, 0.5), (512, 512, 2, False, 1.0)])
def test_decode_forms_agree_16_bit_fused_and_32_bit(oracle, pa, torch, monkeypatch, W, H, wl, lossy, qs):
    """The decode frame paths carry their coefficients as int16 between decoder and synthesis and run synthesis levels
    1 + 0 as one launch (5/3 by default, 9/7 with PICSONG_DWT_FUSE_INV97=1); PICSONG_DWT_NOFUSE_INV=1 keeps one launch per
    level, PICSONG_DEC_C16=0 the reference's 32-bit arrays: the oracle's pixels in every form, single frames and batched
    calls, from an exact-length buffer."""
    img = oracle.gen_frame(W, H, 72)
    lut = oracle.lut_for(lossy, wl)
    ref = oracle.encode_frame(img, wl, lossy, qs, lut)
    want = oracle.decode_frame(ref, W, H, wl, lossy, qs, lut)
    s = _dev(torch, ref.view(np.int16))
    for env in ({}, {"PICSONG_DWT_FUSE_INV97": "1"}, {"PICSONG_DWT_NOFUSE_INV": "1"}, {"PICSONG_DEC_C16": "0"},
                {"PICSONG_DWT_FUSE_INV97": "1", "PICSONG_DWT_EXACT_REPLAY": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
        pix = c.decode_frame(s.clone())
        assert np.array_equal(pix.cpu().numpy()[:H, :W], want), env
        three = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
        three[:, :s.numel()] = s
        out = c.decode_frames(three)
        assert all(torch.equal(out[j], pix) for j in range(3)) and c.range_flag() == 0, env
        c.close()
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("W,H,wl,lossy,qs", [(1280, 704, 5, False, 1.0), (640, 384, 4, True, 0.5)])
def test_unaligned_frame_pointer_and_late_novec_fall_back_to_the_32_bit_form(oracle, pa, torch, monkeypatch, W, H, wl, lossy, qs):
    """A context chooses the 16-bit coefficient form from its geometry; whether a CALL can use it also depends on the
    caller's frame pointer (the vector kernels want 16-byte alignment) and on PICSONG_DWT_NOVEC at call time.  Such a
    call takes the per-column kernels with the 32-bit arrays -- same codestream, no error (the header states no
    alignment requirement for picsong_encode_frame)."""
    img = oracle.gen_frame(W, H, 71)
    ref = oracle.encode_frame(img, wl, lossy, qs, oracle.lut_for(lossy, wl))
    pad = oracle.pad_frame(img)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
    for off in (1, 2, 4, 8):                                   # a view at an odd / a 2- / 4- / 8-byte offset
        buf = torch.zeros(pad.size + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + pad.size]
        view.copy_(_dev(torch, pad).view(-1))
        got = c.encode_frame(view, 0).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, ref), off
    frame = _dev(torch, pad)
    assert np.array_equal(c.encode_frame(frame, 0).cpu().numpy().view(np.uint16), ref)
    monkeypatch.setenv("PICSONG_DWT_NOVEC", "1")               # after the context was created
    assert np.array_equal(c.encode_frame(frame, 0).cpu().numpy().view(np.uint16), ref)
    monkeypatch.delenv("PICSONG_DWT_NOVEC")
    assert np.array_equal(c.encode_frame(frame, 0).cpu().numpy().view(np.uint16), ref)
    c.close()


@pytest.mark.parametrize("W,H,wl,lossy,qs,mask,kk,hint", [(320, 192, 3, False, 1.0, 1, 0.0, False), (704, 448, 4, True, 0.5, 7, 0.0, False),
                                                          (1000, 300, 3, False, 1.0, 0, 0.0, False), (704, 448, 4, False, 1.0, 1, 0.6, False),
                                                          (512, 512, 5, True, 0.5, 7, 1.5, True), (1000, 300, 3, False, 1.0, 2, 0.4, True)])
def test_rgb_frame_through_the_batched_grid_equals_oracle(oracle, pa, torch, W, H, wl, lossy, qs, mask, kk, hint):
    """picsong_encode_rgb_frame / picsong_decode_rgb_frame: the three components of an RGB frame as the three frames
    of ONE launch per stage (component c with table c; the colour transform inside the transform's first and last
    launches) -- every component's codestream equals the oracle's and the plane-by-plane calls', the header lands on the
    components of the mask, and the decode returns the planes.  -k > 0 too (the BULK coder instantiations over the
    three components, both of the encoder's, the decoder's int16 form)."""
    planes = [oracle.pad_frame(oracle.gen_frame(W, H, 60 + c)) for c in range(3)]
    AH, AW = planes[0].shape
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), rgb=True, k=kk, pipelined=hint)
    d = [_dev(torch, p) for p in planes]
    hdr = pa.header_pack(c.params)
    got = [g.clone() for g in c.encode_rgb_frame(*d, header_mask=mask)]
    ref_comps = oracle.rgb_forward(*planes, lossy)
    comps = c.rgb_forward(*d)
    for k in range(3):
        with_hdr = (mask >> k) & 1
        ref = oracle.encode_plane(ref_comps[k], wl, lossy, qs, oracle.lut_for_component(lossy, wl, k, k=kk), hdr if with_hdr else None, k=kk)
        assert np.array_equal(got[k].cpu().numpy().view(np.uint16), ref), f"component {k}"
        assert torch.equal(got[k], c.encode_plane(comps[k], k, bool(with_hdr)))
    streams = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for k in range(3):
        streams[k, :got[k].numel()] = got[k]
    back = c.decode_rgb_frame(streams)
    dec = [c.decode_plane(got[k].clone(), k).clone() for k in range(3)]
    ref_back = c.rgb_inverse(*dec)
    for k in range(3):
        assert torch.equal(back[k].view(-1), ref_back[k].view(-1))
        if not lossy:
            assert np.array_equal(back[k].cpu().numpy(), planes[k])
    # ... and the oracle's own decode of the three streams, through its inverse colour transform
    ob = oracle.rgb_inverse(*[oracle.decode_plane(got[k].cpu().numpy().view(np.uint16), AW, AH, wl, lossy, qs,
                                                  oracle.lut_for_component(lossy, wl, k, k=kk), k=kk) for k in range(3)])
    for k in range(3):
        assert np.array_equal(back[k].cpu().numpy().reshape(AH, AW), ob[k]), f"plane {k} against the oracle's decode"
    # a grey context refuses the call
    g = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    with pytest.raises(pa.PicsongError):
        g.encode_rgb_frame(*d)
    g.close()
    c.close()


# ---- complexity-scalable mode -k > 0 -------------------------------------------
@pytest.mark.parametrize("W,H,wl,lossy,qs,k", [(512, 512, 3, False, 1.0, 0.3), (700, 500, 4, False, 1.0, 1.5),
                                               (512, 384, 3, False, 1.0, 65.0), (640, 384, 3, True, 0.5, 0.7)])
def test_complexity_scalable_codestream_identical_to_oracle(oracle, pa, torch, W, H, wl, lossy, qs, k):
    img = oracle.gen_frame(W, H, 4)
    lut = oracle.lut_for_k(lossy, wl)
    ref = oracle.encode_frame(img, wl, lossy, qs, lut, 0, 0, k=k)
    c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), k=k)
    got = c.encode_frame(_dev(torch, oracle.pad_frame(img)), 0).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref)
    dec = c.decode_frame(_dev(torch, ref.view(np.int16))).cpu().numpy()[:H, :W]
    assert np.array_equal(dec, oracle.decode_frame(ref, W, H, wl, lossy, qs, lut, k=k))
    if not lossy:
        assert np.array_equal(dec, img)
    c.close()


def test_complexity_scalable_full_size_roundtrip(oracle, pa, torch):
    """8K, k = 0.5: size-independent property (decode(encode(x)) == x) + the stream differs from k = 0."""
    W, H, wl = 7680, 4320, 5
    frame = _dev(torch, oracle.pad_frame(oracle.gen_frame(W, H, 0)))
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False), k=0.5)
    s = c.encode_frame(frame, 0)
    assert torch.equal(c.decode_frame(s), frame.view(c.ah, c.aw))
    c0 = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    assert c0.encode_frame(frame, 0).numel() != s.numel()
    c.close(); c0.close()


@pytest.mark.parametrize("k", [0.0, 0.4])
def test_deep_planes_beyond_the_register_file(oracle, pa, torch, k):
    """Codeblocks with MSB 8..15: the encoder keeps 8 planes in registers, the deeper ones go through
    its HBM scratch; paired in one wave with shallow and empty codeblocks."""
    rng = np.random.default_rng(23)
    W, H, wl = 256, 128, 1
    peak = np.array([[6000, 5, 300, 0], [40000, 1000, 2, 200]])
    coef = np.zeros((H, W), np.int32)
    for by in range(2):
        for bx in range(4):
            s = int(peak[by, bx])
            if not s:
                continue
            blk = rng.integers(-2, 3, (64, 64))
            ys, xs = rng.integers(0, 64, 60), rng.integers(0, 64, 60)
            blk[ys, xs] = rng.integers(-s, s + 1, 60)
            coef[by * 64:by * 64 + 64, bx * 64:bx * 64 + 64] = blk
    coef[70, 3] = 65535
    lut = oracle.lut_for_k(False, wl) if k > 0 else oracle.lut_for(False, wl)
    st_ref, sz_ref = oracle.bpc_encode(coef, wl, lut, k=k)
    assert (sz_ref < 4096).all() and st_ref[::4096][st_ref[::4096] != 32].max() == 15
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False), k=k)
    st, sz = c.bpc_encode(_dev(torch, coef))
    st, sz = st.cpu().numpy(), sz.cpu().numpy()
    assert np.array_equal(sz, sz_ref)
    for cb in range(sz_ref.size):
        n = sz_ref[cb]
        assert np.array_equal(st[cb * 4096:cb * 4096 + n], st_ref[cb * 4096:cb * 4096 + n]), cb
    back = c.bpc_decode(_dev(torch, st_ref), _dev(torch, sz_ref)).cpu().numpy().reshape(H, W)
    assert np.array_equal(back, coef)
    c.close()


def test_pipelined_hint_changes_launches_not_results(oracle, pa, torch):
    """picsong_ctx_set_pipelined is a hint: the codestream is the same with and without it, and equals the
    oracle's (until round 2 the hint selected two launches for DWT levels 0 and 1)."""
    for (W, H, wl, lossy, qs) in ((1920, 1080, 5, False, 1.0), (1024, 768, 4, True, 0.5)):
        img = oracle.gen_frame(W, H, 9)
        ref = oracle.encode_frame(img, wl, lossy, qs, oracle.lut_for(lossy, wl), 0, 0)
        frame = _dev(torch, oracle.pad_frame(img))
        got = []
        for hint in (False, True):
            c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), pipelined=hint)
            got.append(c.encode_frame(frame, 0).cpu().numpy().view(np.uint16))
            c.close()
        assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref)


@pytest.mark.parametrize("W,H,wl,k", [(1920, 1080, 5, 0.5), (512, 512, 5, 1.5)])
def test_complexity_scalable_instantiations_agree(oracle, pa, torch, monkeypatch, W, H, wl, k):
    """-k > 0: the encoder's two instantiations (the hint picks: compact table copies and six waves a SIMD for frames in
    flight, whole tables and more registers for a lone frame), the whole-table forms of both coders
    (PICSONG_BULK_FULLTAB=1; the 512 x 512 wl 5 geometry has a codeblock that spans 13 table groups and takes them by
    itself), the decoder's int16 and 32-bit coefficient forms -- one codestream, the oracle's, and its decode the frame."""
    img = oracle.gen_frame(W, H, 33)
    lut = oracle.lut_for_k(False, wl)
    ref = oracle.encode_frame(img, wl, False, 1.0, lut, 0, 0, k=k)
    frame = _dev(torch, oracle.pad_frame(img))
    for hint, fulltab, dec32 in ((False, False, False), (True, False, False), (True, True, False), (False, False, True),
                                 (False, True, True)):
        if fulltab:
            monkeypatch.setenv("PICSONG_BULK_FULLTAB", "1")
        if dec32:                      # the decoder's 32-bit coefficient form (the default is int16 where the geometry allows)
            monkeypatch.setenv("PICSONG_DEC_C16", "0")
        c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False), k=k, pipelined=hint)
        s = c.encode_frame(frame, 0)
        assert np.array_equal(s.cpu().numpy().view(np.uint16), ref), (hint, fulltab, dec32)
        assert np.array_equal(c.decode_frame(s.clone()).cpu().numpy()[:H, :W], img), (hint, fulltab, dec32)
        assert c.range_flag() == 0
        c.close()
        if fulltab:
            monkeypatch.delenv("PICSONG_BULK_FULLTAB")
        if dec32:
            monkeypatch.delenv("PICSONG_DEC_C16")


def test_random_geometries_through_the_frame_paths(oracle, pa, torch):
    """Seeded random W x H, wl, transform and content (synthetic, noise = raw blocks, flat = empty blocks, mixed) through
    the frame paths: the codestream is the oracle's, the decode -- which reads it straight from an EXACT-length buffer --
    the oracle's pixels, and a three-frame batched call writes the same payload (tools/fuzz_parity.py is the longer run)."""
    rng = np.random.default_rng(11)
    oracle.set_threads(oracle.usable_threads())
    try:
        for case in range(10):
            W, H = int(rng.integers(65, 1500)), int(rng.integers(65, 900))
            lossy = bool(rng.integers(0, 2))
            wl = int(rng.integers(1, 7))
            while (oracle.pad_dim(W) >> wl) < 2 or (oracle.pad_dim(H) >> wl) < 2:
                wl -= 1
            qs = float(rng.choice([1.0, 0.5])) if lossy else 1.0
            kind = case % 4
            img = oracle.gen_frame(W, H, case)
            if kind == 1:
                img = rng.integers(0, 256, (H, W), dtype=np.uint8)
            elif kind == 2:
                img = np.full((H, W), 77, np.uint8)
            elif kind == 3:
                img[: H // 2] = rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
            lut = oracle.lut_for(lossy, wl)
            ref = oracle.encode_frame(img, wl, lossy, qs, lut)
            c = pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy))
            frame = _dev(torch, oracle.pad_frame(img))
            s = c.encode_frame(frame)
            what = f"case {case}: {W}x{H} wl {wl} lossy {lossy} qs {qs} kind {kind}"
            assert s.numel() == ref.size and np.array_equal(s.cpu().numpy().view(np.uint16), ref), what
            got = c.decode_frame(s.clone()).cpu().numpy()[:H, :W]
            want = img if not lossy else oracle.decode_frame(ref, W, H, wl, lossy, qs, lut)
            assert np.array_equal(got, want), what
            frames = torch.stack([frame.view(-1)] * 3)
            out = torch.empty((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
            c.encode_frames_async(frames, out, 1)
            torch.cuda.synchronize()
            assert torch.equal(out[2, 9:s.numel()], s[9:]), what   # (frames 1.. of a video carry no header)
            c.close()
    finally:
        oracle.set_threads(1)


def test_damaged_streams_decode_without_leaving_their_buffers(oracle, pa, torch):
    """Garbage in: every length is clamped into 1..4096 and every MSB into 0..15 (range flag set), the
    decoder's loops are bounded by 16 planes x 64 rows, codeword slots by 4094 -- so a damaged stream
    decodes to SOMETHING and returns; it must not fault or hang.  Payload-only damage (table intact)
    keeps the flag clear."""
    W, H, wl = 256, 192, 2
    c = pa.Codec(W, H, wl=wl, lut_folder=_lutdir(oracle, False))
    rng = np.random.default_rng(12)
    n = c.max_stream_shorts()
    junk = torch.from_numpy(rng.integers(-32768, 32768, n, dtype=np.int16)).cuda()
    out = c.decode_frame(junk)
    torch.cuda.synchronize()
    assert out.shape == (c.ah, c.aw) and c.range_flag() == 1
    img = oracle.gen_frame(W, H, 4)
    good = c.encode_frame(_dev(torch, oracle.pad_frame(img)), 0).cpu().numpy().copy()
    bad = np.zeros(n, np.int16)
    bad[:good.size] = good
    first_payload = 9 + 2 * c.ncb
    idx = rng.integers(first_payload, good.size, 200)
    bad[idx] = rng.integers(-32768, 32768, idx.size, dtype=np.int16)
    out = c.decode_frame(torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    assert c.range_flag() == 0 and out.shape == (c.ah, c.aw)
    # and the context is still good for a clean stream
    assert np.array_equal(c.decode_frame(torch.from_numpy(good).cuda()).cpu().numpy()[:H, :W], img)
    c.close()


# ---- caller tables whose geometry is not the context's: taken and coded as the oracle codes, or refused ---------------
def _lut_info(pa, lut):
    info = pa.LutInfo()
    for k, v in lut.geometry().items():
        setattr(info, k, v)
    info.n_tables, info.cp = lut.n_tables, lut.cp
    return info


def _set_caller_table(pa, torch, c, lut, setter):
    """picsong_ctx_set_lut_component (a host copy) or picsong_ctx_set_lut_device (the caller's device table, which must
    outlive its use: returned); returns (rc, device table or None)."""
    import ctypes as C
    info = _lut_info(pa, lut)
    if setter == "component":
        tab = np.ascontiguousarray(lut.table[:lut.total * lut.n_tables], np.int32)
        return c.L.picsong_ctx_set_lut_component(c.h, 0, C.byref(info), tab.ctypes.data_as(C.c_void_p)), None
    d = _dev(torch, lut.table[:lut.total * lut.n_tables])
    return c.L.picsong_ctx_set_lut_device(c.h, 0, C.byref(info), C.c_void_p(d.data_ptr())), d


def _stage_parity(oracle, torch, c, coef, wl, lut, k):
    H, W = coef.shape
    st_o, sz_o = oracle.bpc_encode(coef, wl, lut, k=k)
    st, sz = c.bpc_encode(_dev(torch, coef))
    st, sz = st.cpu().numpy(), sz.cpu().numpy()
    assert np.array_equal(sz, sz_o)
    for cb in range(sz_o.size):
        n = sz_o[cb]
        assert np.array_equal(st[cb * 4096:cb * 4096 + n], st_o[cb * 4096:cb * 4096 + n]), cb
    ref = oracle.bpc_decode(st_o, sz_o, W, H, wl, lut, k=k)
    back = c.bpc_decode(_dev(torch, st_o), _dev(torch, sz_o)).cpu().numpy().reshape(H, W)
    assert np.array_equal(back, ref)
    assert c.range_flag() == 0


_GPU_CT_CASES = ([("k0", t, True) for t in ("wl-1", "wl+1", "bp8", "short4", "nsub1")] + [("k0", "ntab15", False)]
                 + [("cp3", t, True) for t in ("wl-1", "bp8", "nsub1")]
                 + [(m, t, ok) for m in ("k", "k-hint", "k-fulltab", "wholegeo")
                    for t, ok in (("wl-1", False), ("wl+1", True), ("bp12", True), ("bp11", False), ("bp8", False),
                                  ("short3", True), ("short4", False), ("ntab4", True), ("nsub1", False),
                                  ("nsub1+", True))])


@pytest.mark.parametrize("setter", ["component", "device"])
@pytest.mark.parametrize("mode,table,accepted", _GPU_CT_CASES)
def test_caller_table_lut_geometry_taken_or_refused(oracle, pa, torch, monkeypatch, mode, table, accepted, setter):
    """Both setters with a caller's table of another geometry (tests/test_kernels_emulated.py has the same matrix on the
    emulator).  Taken: the stage coders and the frame paths give the oracle's staging, sizes, codestream and decode.
    Refused: PICSONG_ERR_ARG naming the geometry, and the context keeps coding with the table it held.  -k > 0 runs the
    lone-frame encoder (whole tables), the pipelined one (compact copies where the geometry allows), the whole-table
    coders by PICSONG_BULK_FULLTAB=1, and a geometry whose codeblocks take whole tables by themselves."""
    W, H, wl = (128, 128, 5) if mode == "wholegeo" else (256, 256, 2)
    if table.startswith("nsub1") and mode != "wholegeo":
        W, H, wl = 256, 256, 1          # level 0's HH group (2, past LL's 1) has coded codeblocks at MSB 15
    layout = {"k0": "k0", "cp3": "cp3"}.get(mode, "k")
    k = 0.7 if layout == "k" else 0.0
    if mode == "k-fulltab":
        monkeypatch.setenv("PICSONG_BULK_FULLTAB", "1")
    load = {"k0": oracle.lut_for, "cp3": oracle.lut_for_cp3, "k": oracle.lut_for_k}[layout]
    good = load(False, wl)
    lut = oracle.caller_table(layout, table, wl)
    coef = oracle.deep_coeffs(W, H, 17, raw_cb=(W // 64) * (H // 64) - 1)
    img = oracle.gen_frame(W, H, 3)
    c = pa.Codec(W, H, wl=wl, k=k, cp=3 if layout == "cp3" else 2, pipelined=(mode == "k-hint"))
    rc, d_good = _set_caller_table(pa, torch, c, good, setter)
    assert rc == 0
    rc, d_lut = _set_caller_table(pa, torch, c, lut, setter)
    if accepted:
        assert rc == 0, c.L.picsong_last_error().decode()
        _stage_parity(oracle, torch, c, coef, wl, lut, k)
        s = c.encode_frame(_dev(torch, oracle.pad_frame(img)), 0)
        ref = oracle.encode_frame(img, wl, False, 1.0, lut, 0, 0, k=k)
        assert np.array_equal(s.cpu().numpy().view(np.uint16), ref)
        want = oracle.decode_frame(ref, W, H, wl, False, 1.0, lut, k=k)
        assert np.array_equal(c.decode_frame(s.clone()).cpu().numpy()[:H, :W], want)
    else:
        assert rc == -1                                               # PICSONG_ERR_ARG
        msg = c.L.picsong_last_error().decode()
        g = lut.geometry()
        assert (f"n_bitplanes {g['n_bitplanes']}" in msg and f"wl {wl}" in msg) or "bit-plane tables" in msg, msg
        _stage_parity(oracle, torch, c, coef, wl, good, k)           # the context still codes with its previous table
    torch.cuda.synchronize()
    c.close()
    del d_good, d_lut
