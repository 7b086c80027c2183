"""PICSONG -cd 1 -drop d on a GPU: the files written for a small grey image and a small RGB video equal drop_ref -- the
oracle's full decode of the file's own streams, truncated by d(cb) = max(0, d - level(cb)) with the midpoint -- alone and
with -reduce 1; -drop 0 writes the plain decode's bytes.  (The refusals that need no GPU: tests/test_drop_host.py.)"""
import os
import subprocess

import numpy as np
import pytest

import drop_ref as dr
import reduced_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def _pgm(path, w, h):
    data = open(path, "rb").read()
    head = f"P5\n{w} {h}\n255\n".encode()
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w)


@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_grey_image(oracle, tmp_path, lossy, qs):
    W, H, wl, drop = 700, 500, 4, 2
    lutdir = os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    raw, enc = tmp_path / "in.raw", tmp_path / "out.enc"
    oracle.gen_frame(W, H, 30).tofile(raw)
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", int(lossy), "-qs", qs, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    AW, AH = oracle.pad_dim(W), oracle.pad_dim(H)
    stream, lut = np.fromfile(enc, np.uint16), oracle.lut_for(lossy, wl)
    outs = {}
    for name, flags in (("plain", ()), ("d0", ("-drop", 0)), ("d2", ("-drop", drop)), ("d2r1", ("-drop", drop, "-reduce", 1))):
        dec = tmp_path / f"{name}.pgm"
        r = _run("-cd", 1, "-i", enc, "-o", dec, "-LUTFolder", lutdir, *flags)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = dec
    assert outs["d0"].read_bytes() == outs["plain"].read_bytes()
    assert np.array_equal(_pgm(outs["d2"], W, H), dr.drop_pixels(stream, AW, AH, wl, lossy, qs, lut, drop)[:H, :W])
    rw, rh = rr.visible(W, H, 1)
    assert np.array_equal(_pgm(outs["d2r1"], rw, rh), dr.drop_pixels(stream, AW, AH, wl, lossy, qs, lut, drop, 1)[:rh, :rw])
    assert outs["d2"].read_bytes() != outs["plain"].read_bytes()
    # -compare composes: the PSNR of the quick decode against the original
    r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "c.pgm", "-LUTFolder", lutdir, "-drop", drop, "-compare", raw)
    assert r.returncode == 0 and "Compare: PSNR" in r.stdout, r.stdout + r.stderr


def test_rgb_video(oracle, tmp_path):
    W, H, wl, F, drop = 320, 192, 3, 3, 2
    lossy, qs = False, 1.0
    lutdir = os.path.join(oracle.LUT_DIR, "n1_lossless")
    planes = [[oracle.gen_frame(W, H, 60 + 3 * f + c) for c in range(3)] for f in range(F)]
    raw, enc = tmp_path / "v.raw", tmp_path / "v.enc"
    np.concatenate([p.ravel() for fr in planes for p in fr]).tofile(raw)
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", 0, "-isRGB", 1, "-components", 3, "-video", 1,
             "-frames", F, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    AW, AH = oracle.pad_dim(W), oracle.pad_dim(H)
    sizes = [int(x) for x in open(str(enc) + "_SIZE").read().split(",") if x]
    allsh = np.fromfile(enc, np.uint16)
    at = np.concatenate([[0], np.cumsum(sizes)])
    luts = [oracle.lut_for_component(lossy, wl, c) for c in range(3)]
    per = [[allsh[at[3 * f + c]:at[3 * f + c + 1]] for c in range(3)] for f in range(F)]
    for red in (0, 1):
        rw, rh = rr.visible(W, H, red)
        want = [dr.drop_rgb(per[f], AW, AH, wl, lossy, qs, luts, drop, red) for f in range(F)]
        expect = np.concatenate([np.asarray(want[f][c], np.uint8)[:rh, :rw].ravel() for f in range(F) for c in range(3)]).tobytes()
        dec = tmp_path / f"v_r{red}.dec"
        flags = ("-reduce", red) if red else ()
        r = _run("-cd", 1, "-i", enc, "-o", dec, "-video", 1, "-LUTFolder", lutdir, "-framesPerLaunch", 2, "-drop", drop, *flags)
        assert r.returncode == 0, r.stdout + r.stderr
        assert dec.read_bytes() == expect, red
    plain, d0 = tmp_path / "plain.dec", tmp_path / "d0.dec"
    for dec, flags in ((plain, ()), (d0, ("-drop", 0))):
        r = _run("-cd", 1, "-i", enc, "-o", dec, "-video", 1, "-LUTFolder", lutdir, *flags)
        assert r.returncode == 0, r.stdout + r.stderr
    assert d0.read_bytes() == plain.read_bytes() != (tmp_path / "v_r0.dec").read_bytes()
