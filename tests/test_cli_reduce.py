"""PICSONG -cd 1 -reduce r: flag validation on CPU, and on a GPU the reduced images written for a grey image (P5 PGM),
a grey video (raw frames) and an RGB image (planar planes), against the oracle's LL_r."""
import json
import os
import subprocess

import numpy as np
import pytest

import reduced_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def test_reduce_flag_help_and_encode_refusal():
    assert "-reduce r" in _run("-h").stdout
    r = _run("-cd", 0, "-i", "/etc/hostname", "-o", "/tmp/x", "-xSize", 64, "-ySize", 64, "-reduce", 1)
    assert r.returncode == 255 and "Incorrect parameters" in r.stdout


def _encode_grey(oracle, tmp_path, W, H, wl, lossy, qs, F=0):
    frames = [oracle.gen_frame(W, H, 30 + f) for f in range(max(F, 1))]
    lutdir = os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    raw, enc = tmp_path / "in.raw", tmp_path / "out.enc"
    np.concatenate([f.ravel() for f in frames]).tofile(raw)
    args = ["-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", int(lossy), "-qs", qs,
            "-LUTFolder", lutdir]
    if F:
        args += ["-video", 1, "-frames", F]
    r = _run(*args)
    assert r.returncode == 0, r.stdout + r.stderr
    return enc, lutdir


@pytest.mark.gpu
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_grey_image_reduce(oracle, tmp_path, lossy, qs):
    W, H, wl, red = 700, 500, 4, 2
    enc, lutdir = _encode_grey(oracle, tmp_path, W, H, wl, lossy, qs)
    dec = tmp_path / "out.pgm"
    r = _run("-cd", 1, "-i", enc, "-o", dec, "-LUTFolder", lutdir, "-reduce", red, "--metrics", tmp_path / "m.json")
    assert r.returncode == 0, r.stdout + r.stderr
    rw, rh = rr.visible(W, H, red)
    data = open(dec, "rb").read()
    head = f"P5\n{rw} {rh}\n255\n".encode()
    assert data.startswith(head)
    AW, AH = oracle.pad_dim(W), oracle.pad_dim(H)
    want = rr.reduced_pixels(np.fromfile(enc, np.uint16), AW, AH, wl, lossy, qs, oracle.lut_for(lossy, wl), red)
    assert np.array_equal(np.frombuffer(data[len(head):], np.uint8).reshape(rh, rw), want[:rh, :rw])
    m = json.load(open(tmp_path / "m.json"))
    assert (m["width"], m["height"], m["reduce"]) == (rw, rh, red)
    # outside 0 .. wl - 1 (the stream's wl): refused
    for bad in (-1, wl):
        r = _run("-cd", 1, "-i", enc, "-o", dec, "-LUTFolder", lutdir, "-reduce", bad)
        assert r.returncode == 255 and "Incorrect parameters" in r.stdout


@pytest.mark.gpu
def test_grey_video_reduce(oracle, tmp_path):
    W, H, wl, F, red = 700, 500, 4, 6, 2
    enc, lutdir = _encode_grey(oracle, tmp_path, W, H, wl, False, 1.0, F)
    dec = tmp_path / "v.dec"
    r = _run("-cd", 1, "-i", enc, "-o", dec, "-video", 1, "-LUTFolder", lutdir, "-reduce", red)
    assert r.returncode == 0, r.stdout + r.stderr
    rw, rh = rr.visible(W, H, red)
    got = np.fromfile(dec, np.uint8)
    assert got.size == F * rw * rh
    AW, AH = oracle.pad_dim(W), oracle.pad_dim(H)
    sizes = [int(x) for x in open(str(enc) + "_SIZE").read().split(",") if x]
    allsh = np.fromfile(enc, np.uint16)
    off = 0
    for f in range(F):
        want = rr.reduced_pixels(allsh[off:off + sizes[f]], AW, AH, wl, False, 1.0, oracle.lut_for(False, wl), red)
        off += sizes[f]
        assert np.array_equal(got[f * rw * rh:(f + 1) * rw * rh].reshape(rh, rw), want[:rh, :rw]), f


@pytest.mark.gpu
@pytest.mark.parametrize("lossy,qs", [(False, 1.0), (True, 0.5)])
def test_rgb_image_reduce(oracle, tmp_path, lossy, qs):
    W, H, wl, red = 700, 500, 4, 2
    lutdir = os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    planes = [oracle.gen_frame(W, H, 80 + c) for c in range(3)]
    raw, enc, dec = tmp_path / "rgb.raw", tmp_path / "rgb.enc", tmp_path / "rgb.dec"
    np.concatenate([p.ravel() for p in planes]).tofile(raw)
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", int(lossy), "-qs", qs,
             "-isRGB", 1, "-components", 3, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run("-cd", 1, "-i", enc, "-o", dec, "-LUTFolder", lutdir, "-reduce", red)
    assert r.returncode == 0, r.stdout + r.stderr
    rw, rh = rr.visible(W, H, red)
    got = np.fromfile(dec, np.uint8)
    assert got.size == 3 * rw * rh
    AW, AH = oracle.pad_dim(W), oracle.pad_dim(H)
    sizes = [int(x) for x in open(str(enc) + "_SIZE").read().split(",") if x]
    allsh = np.fromfile(enc, np.uint16)
    streams = [allsh[sum(sizes[:c]):sum(sizes[:c + 1])] for c in range(3)]
    want = rr.reduced_rgb(streams, AW, AH, wl, lossy, qs, [oracle.lut_for_component(lossy, wl, c) for c in range(3)], red)
    for c in range(3):
        assert np.array_equal(got[c * rw * rh:(c + 1) * rw * rh].reshape(rh, rw), want[c][:rh, :rw]), c
