"""PICSONG -cd 1 -isRGB video with -reduce and / or -window: the frames go through groups of -framesPerLaunch frames, one
call a group (picsong_decode_rgb_frames_reduced / picsong_decode_rgb_frames_window).  Whatever the group size -- 4 (the
last group short) or 1 -- the decoded file is the same bytes: the oracle's reduced planes, or their crop, frame by frame,
planar."""
import os
import subprocess

import numpy as np
import pytest

import reduced_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")
W, H, WL, F, RED = 320, 192, 3, 6, 1
WINDOW = (3, 5, 40, 20)


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def test_help_names_the_grouped_proxies():
    assert "an RGB video\n                     goes through groups of -framesPerLaunch frames" in _run("-h").stdout


@pytest.mark.gpu
@pytest.mark.parametrize("lossy", [False, True], ids=["5/3", "9/7"])
def test_rgb_video_reduced_and_windowed_in_groups(oracle, tmp_path, lossy):
    qs = 0.5 if lossy else 1.0
    lutdir = os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    planes = [[oracle.gen_frame(W, H, 60 + 3 * f + c) for c in range(3)] for f in range(F)]
    raw, enc = tmp_path / "v.raw", tmp_path / "v.enc"
    np.concatenate([p.ravel() for fr in planes for p in fr]).tofile(raw)
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", WL, "-type", int(lossy), "-qs", qs, "-isRGB", 1,
             "-components", 3, "-video", 1, "-frames", F, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    # the oracle's planes at 1/2^RED from the file's own streams
    AW, AH = oracle.pad_dim(W), oracle.pad_dim(H)
    sizes = [int(x) for x in open(str(enc) + "_SIZE").read().split(",") if x]
    assert len(sizes) == 3 * F
    allsh = np.fromfile(enc, np.uint16)
    at = np.concatenate([[0], np.cumsum(sizes)])
    luts = [oracle.lut_for_component(lossy, WL, c) for c in range(3)]
    want = [rr.reduced_rgb([allsh[at[3 * f + c]:at[3 * f + c + 1]] for c in range(3)], AW, AH, WL, lossy, qs, luts, RED) for f in range(F)]
    rw, rh = rr.visible(W, H, RED)
    x, y, w, h = WINDOW
    for name, flags, crop in [("reduced", ("-reduce", RED), (0, 0, rw, rh)),
                              ("window", ("-reduce", RED, "-window", ",".join(map(str, WINDOW))), (x, y, w, h))]:
        cx, cy, cw, ch = crop
        expect = np.concatenate([np.asarray(want[f][c], np.uint8).reshape(AH >> RED, AW >> RED)[cy:cy + ch, cx:cx + cw].ravel()
                                 for f in range(F) for c in range(3)]).tobytes()
        for group in (4, 1):
            dec = tmp_path / f"{name}_b{group}.dec"
            r = _run("-cd", 1, "-i", enc, "-o", dec, "-video", 1, "-LUTFolder", lutdir, "-framesPerLaunch", group, *flags)
            assert r.returncode == 0, r.stdout + r.stderr
            assert dec.read_bytes() == expect, (name, group)
