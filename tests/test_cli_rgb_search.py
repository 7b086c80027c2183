"""PICSONG -searchFrames N (cuda-image-and-video-codec_amd/host): the -rate / -psnr search of a video over its first N
frames -- an RGB video through the n-frame search calls -- against the reference procedures over the CPU oracle
(rgb_search_ref): the chosen quantiser on the console, the output file and its _SIZE sidecar, and the refusals."""
import json
import os
import subprocess

import numpy as np
import pytest

import layout_ref as lr
import oracle_lib as orc
import rgb_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")
LUTDIR = os.path.join(orc.LUT_DIR, "n1_lossy")
W, H, WL, F = 200, 136, 3, 3


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def test_refused_flag_combinations(tmp_path):
    base = ("-cd", 0, "-i", "/etc/hostname", "-o", tmp_path / "x", "-xSize", 64, "-ySize", 64, "-wl", 1, "-type", 1, "-LUTFolder", LUTDIR)
    rgb = ("-isRGB", 1, "-components", 3)
    for extra, msg in ((("-rate", 1.0, "-searchFrames", 2), "-video 1"),
                       (("-video", 1, "-frames", 4, "-searchFrames", 2), "-rate or -psnr"),
                       (("-video", 1, "-frames", 4, "-rate", 1.0, "-searchFrames", 0), "1 or more"),
                       (("-video", 1, "-frames", 30, "-rate", 1.0, "-searchFrames", 22, *rgb), "1..21"),
                       (("-video", 1, "-frames", 30, "-psnr", 35, "-searchFrames", 17), "1..16")):
        r = _run(*base, *extra)
        assert r.returncode != 0 and "Incorrect parameters." in r.stdout and msg in r.stdout, (extra, r.stdout)
    r = _run("-cd", 1, "-i", "/etc/hostname", "-o", tmp_path / "x", "-LUTFolder", LUTDIR, "-searchFrames", 2)
    assert r.returncode != 0 and "Incorrect parameters." in r.stdout and "-cd 0" in r.stdout
    assert not os.path.exists(tmp_path / "x")


def _video(tmp_path):
    frames = ref.frames(W, H, F)
    raw = tmp_path / "v.raw"
    np.concatenate([p.ravel() for fr in frames for p in fr]).tofile(raw)
    return frames, raw


def _header(j):
    return orc.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=WL, bit_depth=8, lossy=1, qs_1e4=j, components=3,
                           is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=F, k_1e3=0)


def _encode(raw, enc, *extra):
    return _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", WL, "-type", 1, "-isRGB", 1, "-components", 3,
                "-video", 1, "-frames", F, "-LUTFolder", LUTDIR, *extra)


def _assert_file(enc, j):
    want = ref.streams(W, H, WL, F, j, _header(j), 0, 7)
    assert np.array_equal(np.fromfile(enc, np.uint16), np.concatenate(want))
    assert open(str(enc) + "_SIZE").read() == ",".join(str(x.size) for x in want)


@pytest.mark.gpu
def test_rate_over_three_frames_and_over_the_first_alone(tmp_path):
    target3, j3 = ref.check_rate(W, H, WL, 3)
    target1, j1 = ref.check_rate(W, H, WL, 1)
    assert (j3, j1) == (567, 564)
    frames, raw = _video(tmp_path)
    enc, met = tmp_path / "s3.enc", tmp_path / "m.json"
    r = _encode(raw, enc, "-rate", 1.0, "-searchFrames", 3, "--metrics", met)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"(j = {j3}) chosen for {target3} shorts over 3 frame(s)" in r.stdout
    _assert_file(enc, j3)
    assert json.load(open(met))["search_frames"] == 3
    # more frames asked for than there are: the search takes the video's
    enc9 = tmp_path / "s9.enc"
    r = _encode(raw, enc9, "-rate", 1.0, "-searchFrames", 9)
    assert r.returncode == 0 and f"(j = {j3}) chosen for {target3} shorts over 3 frame(s)" in r.stdout
    assert open(enc9, "rb").read() == open(enc, "rb").read()
    # without the flag: the first frame, today's file
    enc1 = tmp_path / "s1.enc"
    r = _encode(raw, enc1, "-rate", 1.0)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"(j = {j1}) chosen for {target1} shorts over 1 frame(s)" in r.stdout
    _assert_file(enc1, j1)
    # the frames as an application holds them: one ingest of the searched frames, the same file
    inter = tmp_path / "v.rgb"
    buf = np.zeros(F * lr.frame_span(lr.RGB24, W, H, 3 * W), np.uint8)
    for f in range(F):
        lr.pack_into(buf[f * lr.frame_span(lr.RGB24, W, H, 3 * W):], frames[f], lr.RGB24, 3 * W)
    buf.tofile(inter)
    encl = tmp_path / "sl.enc"
    r = _encode(inter, encl, "-rate", 1.0, "-searchFrames", 3, "-layout", "rgb")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(encl, "rb").read() == open(enc, "rb").read()
    assert open(str(encl) + "_SIZE").read() == open(str(enc) + "_SIZE").read()


@pytest.mark.gpu
def test_psnr_over_three_frames(tmp_path):
    limit, j, per = ref.check_quality(W, H, WL, 3)
    assert j == 1347
    frames, raw = _video(tmp_path)
    enc = tmp_path / "q3.enc"
    r = _encode(raw, enc, "-psnr", 35, "-searchFrames", 3)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"(j = {j}) chosen for an SSE of at most {limit} over 3 frame(s)" in r.stdout
    assert f"(SSE {sum(sum(p) for p in per)})" in r.stdout
    _assert_file(enc, j)
