"""-m gpu: the window decode (picsong_decode_frame_window, _frames_window, _rgb_frame_window) against the oracle's crop
of LL_r, identities with the reduced and batched calls, the output bound, the codeblocks a window call never reads,
the refusals, and a 1920 x 1080 window of a 16K frame."""
import ctypes
import os

import numpy as np
import pytest

import reduced_ref as rr
import window_ref as wr

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                      # PICSONG_ERR_ARG


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


def _lutdir(oracle, lossy):
    return os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _codec(pa, oracle, W, H, wl, lossy, qs, k=0.0, rgb=False):
    return pa.Codec(W, H, wl=wl, lossy=lossy, qs=qs, lut_folder=_lutdir(oracle, lossy), k=k, rgb=rgb)


def _encode(torch, oracle, c, W, H, seed):
    frame = torch.from_numpy(oracle.pad_frame(oracle.gen_frame(W, H, seed))).cuda()
    return c.encode_frame(frame).clone()


def _windows(paw, pah, W, H, r, rng):
    ws = wr.windows(paw, pah, -(-W // (1 << r)), -(-H // (1 << r)))
    for _ in range(2):
        x, y = int(rng.integers(0, paw)), int(rng.integers(0, pah))
        ws.append((x, y, int(rng.integers(1, min(300, paw - x) + 1)), int(rng.integers(1, min(200, pah - y) + 1))))
    return ws


@pytest.mark.parametrize("W,H,wl,lossy,qs,k", [
    (700, 500, 5, False, 1.0, 0.0), (1000, 300, 5, False, 1.0, 0.0),
    (700, 500, 6, True, 0.5, 0.0), (1000, 300, 6, True, 0.3, 0.0),
    (700, 500, 5, False, 1.0, 0.5), (1000, 300, 6, True, 0.5, 1.5), (700, 500, 6, True, 0.3, 0.5),
    (3840, 2160, 5, False, 1.0, 0.0), (3840, 2160, 6, True, 0.3, 0.0),
    (7680, 4320, 5, False, 1.0, 0.0), (7680, 4320, 6, True, 0.5, 0.0),
])
def test_window_matches_oracle(oracle, pa, torch, W, H, wl, lossy, qs, k):
    c = _codec(pa, oracle, W, H, wl, lossy, qs, k)
    s = _encode(torch, oracle, c, W, H, 5)
    other = _encode(torch, oracle, c, W, H, 6)                   # decoded before every window: no stale coefficients
    sh = s.cpu().numpy().view(np.uint16)
    lut = oracle.lut_for_component(lossy, wl, 0, k=k)
    rng = np.random.default_rng(W + wl)
    for r in range(wl):
        full = rr.reduced_pixels(sh, c.aw, c.ah, wl, lossy, qs, lut, r, k=k)
        pah, paw = full.shape
        for (x, y, w, h) in _windows(paw, pah, W, H, r, rng):
            c.decode_frame(other)
            got = c.decode_frame_window(s, x, y, w, h, r)
            assert np.array_equal(got.cpu().numpy(), full[y:y + h, x:x + w]), (r, x, y, w, h)
            assert c.window_codeblocks(x, y, w, h, r) == len(wr.window_codeblocks(c.aw, c.ah, wl, lossy, r, x, y, w, h))
        assert c.range_flag() == 0
    c.close()


@pytest.mark.parametrize("lossy,qs,k", [(False, 1.0, 0.0), (True, 0.5, 0.0), (False, 1.0, 0.5)])
def test_whole_window_and_batches(oracle, pa, torch, lossy, qs, k):
    W, H, wl = 1000, 300, 5
    c = _codec(pa, oracle, W, H, wl, lossy, qs, k)
    ss = [_encode(torch, oracle, c, W, H, 20 + f) for f in range(5)]
    S = c.max_stream_shorts() + 40
    sb = torch.zeros((5, S), dtype=torch.int16, device="cuda")
    for f, s in enumerate(ss):
        sb[f, :s.numel()] = s
    for r in range(wl):
        paw, pah = c.aw >> r, c.ah >> r
        assert torch.equal(c.decode_frame_window(ss[0], 0, 0, paw, pah, r), c.decode_frame_reduced(ss[0], r))
        assert c.window_codeblocks(0, 0, paw, pah, r) == c.reduced_dims(r)[4]
        for (x, y, w, h) in [(3, 5, min(41, paw - 3), min(17, pah - 5)), (paw - 64, pah // 2, 64, pah - pah // 2)]:
            single = [c.decode_frame_window(s, x, y, w, h, r).clone() for s in ss]
            for n in (1, 2, 5):
                out = torch.full((n, h + 2, w + 7), 0xA5, dtype=torch.uint8, device="cuda")
                c.decode_frames_window(sb[:n], x, y, w, h, r, out[:, :h, :w])
                for f in range(n):
                    assert torch.equal(out[f, :h, :w], single[f]), (r, n, f)
                assert bool((out[:, h:] == 0xA5).all()) and bool((out[:, :, w:] == 0xA5).all())
    c.close()


@pytest.mark.parametrize("lossy,qs,k", [(False, 1.0, 0.0), (True, 0.5, 0.0), (True, 0.3, 0.0)])
def test_rgb_window_matches_oracle(oracle, pa, torch, lossy, qs, k):
    W, H, wl = 700, 500, 5
    planes = [oracle.pad_frame(oracle.gen_frame(W, H, 70 + i)) for i in range(3)]
    c = _codec(pa, oracle, W, H, wl, lossy, qs, k, rgb=True)
    got = [g.clone() for g in c.encode_rgb_frame(*[torch.from_numpy(p).cuda() for p in planes])]
    streams = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for i in range(3):
        streams[i, :got[i].numel()] = got[i]
    shs = [g.cpu().numpy().view(np.uint16) for g in got]
    luts = [oracle.lut_for_component(lossy, wl, i, k=k) for i in range(3)]
    for r in range(wl):
        want = rr.reduced_rgb(shs, c.aw, c.ah, wl, lossy, qs, luts, r, k=k)
        paw, pah = c.aw >> r, c.ah >> r
        for (x, y, w, h) in [(0, 0, paw, pah), (1, 2, min(33, paw - 1), min(21, pah - 2)), (paw - 5, pah - 3, 5, 3)]:
            back = c.decode_rgb_frame_window(streams, x, y, w, h, r)
            for i in range(3):
                assert np.array_equal(back[i].cpu().numpy(), want[i][y:y + h, x:x + w]), (r, i, x, y, w, h)
    c.close()


def test_output_bound_and_odd_offset(oracle, pa, torch):
    W, H, wl = 700, 500, 5
    for lossy, qs in ((False, 1.0), (True, 0.5)):
        c = _codec(pa, oracle, W, H, wl, lossy, qs)
        s = _encode(torch, oracle, c, W, H, 9)
        for r in (0, 2):
            x, y, w, h = 13, 7, 51, 23
            ref = c.decode_frame_window(s, x, y, w, h, r).clone()
            pitch = w + 29
            for off in (0, 1, 3):
                buf = torch.full((h * pitch + 256,), 0xA5, dtype=torch.uint8, device="cuda")
                view = buf[off:]
                assert c.L.picsong_decode_frame_window(c.h, c._p(s), r, x, y, w, h, c._p(view), pitch, c._stream()) == 0
                torch.cuda.synchronize()
                img = view[:h * pitch].view(h, pitch)
                assert torch.equal(img[:, :w], ref), (lossy, r, off)
                assert bool((img[:, w:] == 0xA5).all()) and bool((buf[:off] == 0xA5).all())
                assert bool((view[h * pitch:] == 0xA5).all())
        c.close()


@pytest.mark.parametrize("k", [0.0, 0.5])
def test_codeblocks_outside_the_set_are_not_read(oracle, pa, torch, k):
    W, H, wl, r = 1000, 300, 5, 0
    c = _codec(pa, oracle, W, H, wl, False, 1.0, k)
    s = _encode(torch, oracle, c, W, H, 11)
    x, y, w, h = 400, 100, 90, 60
    clean = c.decode_frame_window(s, x, y, w, h, r).clone()
    want = wr.window_codeblocks(c.aw, c.ah, wl, False, r, x, y, w, h)
    ncx = c.aw // 64
    outside = sorted((cx, cy) for cy in range(c.ah // 64) for cx in range(ncx) if (cx, cy) not in want and
                     any((cx + dx, cy + dy) in want for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))))
    cx, cy = outside[0]
    bad = s.clone()
    bad[9 + 2 * (cy * ncx + cx)] = 20                             # MSB 20, length untouched
    c.range_flag()
    assert torch.equal(c.decode_frame_window(bad, x, y, w, h, r), clean) and c.range_flag() == 0
    sb = torch.zeros((3, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    for f in range(3):
        sb[f, :bad.numel()] = bad
    out = c.decode_frames_window(sb, x, y, w, h, r)
    assert c.range_flag() == 0 and all(torch.equal(out[f], clean) for f in range(3))
    cx, cy = sorted(want)[len(want) // 2]
    bad = s.clone()
    bad[9 + 2 * (cy * ncx + cx)] = 20
    c.decode_frame_window(bad, x, y, w, h, r)
    assert c.range_flag() == 1
    c.close()


def test_refusals(oracle, pa, torch):
    W, H, wl = 700, 500, 5
    c = _codec(pa, oracle, W, H, wl, False, 1.0)
    s = _encode(torch, oracle, c, W, H, 1)
    sb = torch.zeros((2, c.max_stream_shorts()), dtype=torch.int16, device="cuda")
    out = torch.full((c.P * 2,), 0xA5, dtype=torch.uint8, device="cuda")
    L, p, st = c.L, c._p, c._stream()
    one = lambda r, x, y, w, h, pitch, ptr=p(out), sp=p(s): L.picsong_decode_frame_window(c.h, sp, r, x, y, w, h, ptr, pitch, st)
    bat = lambda r, x, y, w, h, pitch, fs, n=2, ss=sb.stride(0): L.picsong_decode_frames_window(
        c.h, n, p(sb), ss, r, x, y, w, h, p(out), pitch, fs, st)
    paw, pah = c.aw, c.ah
    cases = [((-1, 0, 0, 8, 8, 8), b"reduce"), ((wl, 0, 0, 8, 8, 8), b"reduce"), ((0, 0, 0, 0, 8, 8), b"empty"),
             ((0, 0, 0, 8, 0, 8), b"empty"), ((0, -1, 0, 8, 8, 8), b"not inside"), ((0, 0, -1, 8, 8, 8), b"not inside"),
             ((0, paw - 7, 0, 8, 8, 8), b"not inside"), ((0, 0, pah - 7, 8, 8, 8), b"not inside"),
             ((1, (paw >> 1) - 7, 0, 8, 8, 8), b"not inside"), ((0, 0, 0, 8, 8, 7), b"out_pitch")]
    for args, word in cases:
        assert one(*args) == ERR_ARG, args
        assert word in L.picsong_last_error(), (args, L.picsong_last_error())
        assert bat(*args, fs=1 << 20) == ERR_ARG, args
    assert one(0, 0, 0, 8, 8, 8, ptr=None) == ERR_ARG and one(0, 0, 0, 8, 8, 8, sp=None) == ERR_ARG
    assert bat(0, 0, 0, 8, 8, 16, fs=7 * 16 + 7) == ERR_ARG                 # frame stride < (h - 1) * pitch + w
    assert bat(0, 0, 0, 8, 8, 16, fs=1 << 16, ss=16) == ERR_ARG              # stream stride
    assert bat(0, 0, 0, 8, 8, 16, fs=1 << 16, n=0) == ERR_ARG and bat(0, 0, 0, 8, 8, 16, fs=1 << 16, n=65) == ERR_ARG
    n = ctypes.c_int(-5)
    assert L.picsong_window_codeblocks(c.h, wl, 0, 0, 8, 8, ctypes.byref(n)) == ERR_ARG and n.value == -5
    assert L.picsong_window_codeblocks(c.h, 0, 0, 0, 8, 8, None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                                           # refused calls launched nothing
    assert bat(0, 0, 0, 8, 8, 16, fs=7 * 16 + 8) == 0
    c.close()
    g = pa.Codec(W, H, wl=wl, lut_folder=os.path.join(oracle.LUT_CP3_DIR, "n1_lossless"), cp=3)
    assert g.L.picsong_decode_frame_window(g.h, g._p(s), 0, 0, 0, 8, 8, g._p(out), 8, g._stream()) == ERR_ARG
    assert b"-cp 3" in g.L.picsong_last_error()
    g.close()
    rc = _codec(pa, oracle, W, H, wl, False, 1.0, rgb=True)
    s3 = torch.zeros((3, rc.max_stream_shorts()), dtype=torch.int16, device="cuda")
    o3 = [torch.empty(rc.P, dtype=torch.uint8, device="cuda") for _ in range(3)]
    R = lambda *a, ss=s3.stride(0), ptrs=None: rc.L.picsong_decode_rgb_frame_window(
        rc.h, rc._p(s3), ss, *a[:5], *(ptrs or [rc._p(o) for o in o3]), a[5], rc._stream())
    assert R(wl, 0, 0, 8, 8, 8) == ERR_ARG and R(0, 0, 0, 8, 8, 7) == ERR_ARG and R(0, 0, 0, 8, 8, 8, ss=16) == ERR_ARG
    assert R(0, 0, 0, 8, 8, 8, ptrs=[None, rc._p(o3[1]), rc._p(o3[2])]) == ERR_ARG
    rc.close()


def test_16k_window(oracle, pa, torch):
    W = H = 16384
    wl = 5                                                        # bench.py's 16k_intra: 5/3, wl 5
    c = _codec(pa, oracle, W, H, wl, False, 1.0)
    s = _encode(torch, oracle, c, W, H, 3)
    full = c.decode_frame(s).clone()
    for r, (x, y) in ((0, (7000, 9001)), (1, (2049, 3001))):
        ref = full if r == 0 else c.decode_frame_reduced(s, r).clone()
        got = c.decode_frame_window(s, x, y, 1920, 1080, r)
        assert torch.equal(got, ref[y:y + 1080, x:x + 1920]), r
        assert c.window_codeblocks(x, y, 1920, 1080, r) == len(wr.window_codeblocks(c.aw, c.ah, wl, False, r, x, y, 1920, 1080))
    c.close()
