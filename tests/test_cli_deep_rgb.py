"""PICSONG command-line tool with -bps 9..16 -isRGB 1 -components 3: one RGB still image or a video of 16-bit samples, raw
files in -layout planar (default), rgb or rgba.  On a GPU the file-level contract -- the .enc is the composed reference's
streams (deep_rgb_ref) back to back with their lengths in _SIZE, a lossless round trip is exact, a 9/7 one the reference
decode; without one, the flag combinations that are not built say what is."""
import os
import subprocess

import numpy as np
import pytest

import deep_ref as D
import deep_rgb_ref as R
import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")
BUILT = "it codes one RGB still image or a video"
W, H, AW, AH = R.W, R.H, R.AW, R.AH
RGB = ("-isRGB", 1, "-components", 3)


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def _lutdir(lossy):
    return os.path.join(orc.LUT_DIR, "n1_lossy" if lossy else "n1_lossless")


def _frames(bd, wl, n):
    """n frames' visible planes: the issue's saw input, its planes rotated from frame to frame."""
    img = [R.inputs("saw", bd, wl, c) for c in range(3)]
    return [[img[(c + f) % 3] for c in range(3)] for f in range(n)]


def _file_bytes(frames, layout, alpha=0x1357):
    if layout == "planar":
        return np.concatenate([p.ravel() for fr in frames for p in fr]).astype("<u2").tobytes()
    out = []
    for fr in frames:
        px = np.full((H, W, 3 if layout == "rgb" else 4), alpha, np.uint16)
        for c in range(3):
            px[:, :, c] = fr[c]
        out.append(px.ravel())
    return np.concatenate(out).astype("<u2").tobytes()


def _reference(frames, bd, wl, lossy, qs, video):
    """The streams of the frames, 3 a frame: the populated header on component 0 of an image, on frame 0's three of a video."""
    hdr = R.header(W, H, bd, wl, lossy, qs, frames=len(frames) if video else 0)
    streams = []
    for f, fr in enumerate(frames):
        pad = [D.mirror_pad(p) for p in fr]
        comp = R.forward(pad[0], pad[1], pad[2], bd, lossy)
        for c in range(3):
            cf = orc.dwt_forward(np.ascontiguousarray(comp[c]), wl, qs)[:AW * AH].reshape(AH, AW)
            assert D.max_coef(cf) < 32768
            st, sz = orc.bpc_encode(cf, wl, R.lut(lossy, wl, c))
            streams.append(orc.bitstream_pack(st, sz, hdr if f == 0 and (video or c == 0) else None))
    return streams


def test_flag_combinations_that_are_not_built_name_what_is(tmp_path):
    raw = tmp_path / "in.raw"
    raw.write_bytes(_file_bytes(_frames(12, 3, 2), "planar"))
    base = ("-cd", 0, "-i", raw, "-o", tmp_path / "x.enc", "-xSize", W, "-ySize", H, "-wl", 3, "-bps", 12, *RGB, "-LUTFolder", _lutdir(False))
    for extra in (("-layout", "bgr"), ("-layout", "bgra"), ("-layout", "grey"), ("-type", 1, "-rate", 2.0), ("-type", 1, "-psnr", 40),
                  ("-type", 1, "-ssim", 0.97), ("-train", tmp_path / "t"), ("-gpus", 2), ("-cp", 3), ("-signedOrUnsigned", 1),
                  ("-video", 1, "-frames", 2, "-framesPerLaunch", 22), ("-video", 1, "-frames", 3), ("-layout", "rgba", "-video", 1, "-frames", 2)):
        r = _run(*base, *extra)                              # (the last two: the file is shorter than the frames asked for)
        assert r.returncode != 0 and BUILT in r.stdout, (extra, r.stdout)
    pgm = tmp_path / "in.pgm"
    pgm.write_bytes(f"P5\n{W} {H}\n4095\n".encode() + _file_bytes(_frames(12, 3, 1), "planar"))
    r = _run("-cd", 0, "-i", pgm, "-o", tmp_path / "x.enc", "-wl", 3, "-bps", 12, *RGB, "-LUTFolder", _lutdir(False))
    assert r.returncode != 0 and BUILT in r.stdout
    assert "rgba" in _run("-h").stdout and "-bps" in _run("-h").stdout
    assert not os.path.exists(tmp_path / "x.enc")


@pytest.mark.gpu
@pytest.mark.parametrize("lossy,bd,wl,qs,layout,video", [(False, 12, 5, 1.0, "planar", 0), (True, 12, 3, 1.0, "rgb", 0),
                                                         (False, 10, 5, 1.0, "rgb", 3), (True, 12, 3, 1.0, "planar", 3)],
                         ids=["53-still-planar", "97-still-rgb", "53-video-rgb", "97-video-planar"])
def test_still_image_and_video_files(tmp_path, lossy, bd, wl, qs, layout, video):
    n = video or 1
    frames = _frames(bd, wl, n)
    ref = _reference(frames, bd, wl, lossy, qs, bool(video))
    raw, enc, dec = tmp_path / "in.raw", tmp_path / "out.enc", tmp_path / "out.raw"
    raw.write_bytes(_file_bytes(frames, layout))
    lay = () if layout == "planar" else ("-layout", layout)
    vid = ("-video", 1, "-frames", video, "-framesPerLaunch", 2) if video else ()
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", int(lossy), "-qs", qs, "-bps", bd, *RGB, *lay, *vid,
             "-LUTFolder", _lutdir(lossy))
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(enc, np.uint16), np.concatenate(ref))
    sizes = [int(t) for t in open(str(enc) + "_SIZE").read().split(",") if t.strip()]
    assert sizes == [s.size for s in ref]
    r = _run("-cd", 1, "-i", enc, "-o", dec, "-LUTFolder", _lutdir(lossy), *lay, *(("-video", 1, "-framesPerLaunch", 2) if video else ()))
    assert r.returncode == 0, r.stdout + r.stderr
    if lossy:                                                # the reference decode, cropped
        want = [[p[:H, :W] for p in R.decode(ref[3 * f:3 * f + 3], bd, wl, lossy, qs)] for f in range(n)]
    else:
        want = frames                                        # lossless: exact
    assert open(dec, "rb").read() == _file_bytes(want, layout), "the decoded file"
    if layout == "rgb" and not video:
        # ... and into another layout, alpha 2^bd - 1; -drop works; -reduce and -window are not built
        r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "a.raw", "-LUTFolder", _lutdir(lossy), "-layout", "rgba")
        assert r.returncode == 0 and open(tmp_path / "a.raw", "rb").read() == _file_bytes(want, "rgba", alpha=(1 << bd) - 1)
        r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "d.raw", "-LUTFolder", _lutdir(lossy), "-drop", 2)
        assert r.returncode == 0 and os.path.getsize(tmp_path / "d.raw") == 6 * W * H, r.stdout + r.stderr
        for extra in (("-reduce", 1), ("-window", "8,8,64,40"), ("-layout", "bgra")):
            r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "r.raw", "-LUTFolder", _lutdir(lossy), *extra)
            assert r.returncode != 0 and BUILT in r.stdout, extra


@pytest.mark.gpu
def test_a_raised_range_flag_fails_the_encode(tmp_path):
    bd, wl = 16, 5
    planes = [R.inputs("noise", bd, wl, c) for c in range(3)]
    raw, enc = tmp_path / "in.raw", tmp_path / "out.enc"
    raw.write_bytes(_file_bytes([planes], "planar"))
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", 0, "-bps", bd, *RGB, "-LUTFolder", _lutdir(False))
    assert r.returncode != 0 and "2^15" in r.stdout
    assert not os.path.exists(enc) and not os.path.exists(str(enc) + "_SIZE")
