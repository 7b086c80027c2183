"""PICSONG -isRGB 1 -components 3 -video 1: an RGB video coded and decoded in groups of -framesPerLaunch frames through
one call a group (picsong_encode_rgb_frames / picsong_decode_rgb_frames; with -layout the image calls).  Whatever the
group size -- 1, 2 (the last group short) or the default -- the .enc, the _SIZE file and the decoded file are the same
bytes, and the streams are the oracle's plane by plane."""
import os
import subprocess

import numpy as np
import pytest

import layout_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")
W, H, WL, F = 320, 192, 3, 5
GROUPS = (("b1", ("-framesPerLaunch", 1)), ("b2", ("-framesPerLaunch", 2)), ("default", ()))


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def test_flag_is_documented():
    assert "an RGB video" in _run("-h").stdout


@pytest.fixture(scope="module")
def video(oracle):
    """The 5 frames' planes and, per transform, the oracle's 15 streams (frame 0's three components carry the header)."""
    planes = [[oracle.gen_frame(W, H, 60 + 3 * f + c) for c in range(3)] for f in range(F)]
    ref = {}
    for lossy in (False, True):
        qs = 0.5 if lossy else 1.0
        hdr = oracle.header_pack(n_samples=W * H * 3, cp=2, cb_height=18, cb_width=64, wl=WL, bit_depth=8, lossy=int(lossy),
                                 qs_1e4=int(qs * 10000), components=3, is_rgb=1, height=H, endianess=0, bps=8, is_signed=0, frames=F, k_1e3=0)
        streams = []
        for f in range(F):
            comps = oracle.rgb_forward(*[oracle.pad_frame(p) for p in planes[f]], lossy)
            for c in range(3):
                streams.append(oracle.encode_plane(comps[c], WL, lossy, qs, oracle.lut_for_component(lossy, WL, c), hdr if f == 0 else None))
        ref[lossy] = streams
    return planes, ref


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [None, "rgb"], ids=["planar", "layout-rgb"])
@pytest.mark.parametrize("lossy", [False, True], ids=["5/3", "9/7"])
def test_rgb_video_in_groups_changes_no_file(oracle, video, tmp_path, lossy, layout):
    planes, ref = video
    qs = 0.5 if lossy else 1.0
    lutdir = os.path.join(oracle.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")
    raw = tmp_path / "v.raw"
    if layout is None:
        data = np.concatenate([p.ravel() for fr in planes for p in fr])
    else:
        data = np.concatenate([lr.pack(fr, lr.RGB24, 3 * W) for fr in planes])
    data.tofile(raw)
    extra = () if layout is None else ("-layout", layout)
    want = np.concatenate(ref[lossy])
    want_sizes = ",".join(str(x.size) for x in ref[lossy])
    decs = []
    for name, group in GROUPS:
        enc, dec = tmp_path / (name + ".enc"), tmp_path / (name + ".dec")
        r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", WL, "-type", int(lossy), "-qs", qs, "-isRGB", 1,
                 "-components", 3, "-video", 1, "-frames", F, "-LUTFolder", lutdir, *group, *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.fromfile(enc, np.uint16), want), name
        assert open(str(enc) + "_SIZE").read() == want_sizes, name
        r = _run("-cd", 1, "-i", enc, "-o", dec, "-video", 1, "-LUTFolder", lutdir, *group, *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        decs.append(dec.read_bytes())
        assert len(decs[-1]) == F * 3 * W * H, name
        assert decs[-1] == decs[0], name
    if not lossy:
        assert decs[0] == data.tobytes()
