"""PICSONG command-line tool with -bps 9..16: one grey still image of 16-bit samples.  On a GPU the file-level contract --
the .enc equals the composed reference's stream (deep_ref) and the C ABI call's, the decode is a P5 with maxval 2^bd - 1
whose big-endian samples are the input; without one, the modes that are not built say what is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deep_ref as D
import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")
BUILT = "this build codes one grey still image"


def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def test_modes_that_are_not_built_name_what_is(tmp_path):
    raw = tmp_path / "in.raw"
    D.inputs("saw", 12, 5).tofile(raw)
    lutdir = os.path.join(orc.LUT_DIR, "n1_lossless")
    base = ("-cd", 0, "-i", raw, "-o", tmp_path / "x.enc", "-xSize", D.W, "-ySize", D.H, "-wl", 5, "-bps", 12, "-LUTFolder", lutdir)
    for extra in (("-video", 1, "-frames", 2), ("-isRGB", 1, "-components", 3), ("-type", 1, "-rate", 2.0), ("-type", 1, "-psnr", 40),
                  ("-train", tmp_path / "t"), ("-gpus", 2), ("-layout", "rgb", "-isRGB", 1, "-components", 3), ("-signedOrUnsigned", 1)):
        r = _run(*base, *extra)
        assert r.returncode != 0 and BUILT in r.stdout, (extra, r.stdout)
    assert "-bps" in _run("-h").stdout
    for bad in (7, 17):
        r = _run(*base[:-4], "-bps", bad, "-LUTFolder", lutdir)
        assert r.returncode != 0 and BUILT in r.stdout
    assert not os.path.exists(tmp_path / "x.enc")


@pytest.mark.gpu
def test_twelve_bit_image_files(tmp_path):
    import picsong_amd as pa
    import torch
    bd, wl, W, H = 12, 5, D.W, D.H
    img, pad, coef, sizes, ref = D.encode("saw", bd, wl, False)
    D.check_precondition(coef, sizes, 0)
    lutdir = os.path.join(orc.LUT_DIR, "n1_lossless")
    raw, enc, dec = tmp_path / "in.raw", tmp_path / "out.enc", tmp_path / "out.pgm"
    img.astype("<u2").tofile(raw)
    r = _run("-cd", 0, "-i", raw, "-o", enc, "-xSize", W, "-ySize", H, "-wl", wl, "-type", 0, "-bps", bd, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(enc, np.uint16)
    assert np.array_equal(got, ref)
    # ... which is the ABI call's stream
    c = pa.Codec(W, H, wl=wl, lut_folder=lutdir, bit_depth=bd)
    s = c.encode_frames16(torch.from_numpy(np.ascontiguousarray(pad).view(np.int16)[None]).cuda())
    assert np.array_equal(s[0].cpu().numpy().view(np.uint16), got)
    c.close()
    r = _run("-cd", 1, "-i", enc, "-o", dec, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(dec, "rb").read()
    head = f"P5\n{W} {H}\n4095\n".encode()
    assert data.startswith(head) and len(data) == len(head) + 2 * W * H
    assert np.array_equal(np.frombuffer(data[len(head):], ">u2").reshape(H, W), img)
    # the same from a 16-bit PGM: sizes from its header, big-endian samples
    pgm, enc2 = tmp_path / "in.pgm", tmp_path / "out2.enc"
    pgm.write_bytes(head + img.astype(">u2").tobytes())
    r = _run("-cd", 0, "-i", pgm, "-o", enc2, "-wl", wl, "-bps", bd, "-LUTFolder", lutdir)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(enc2, np.uint16), ref)
    # -drop is a context setting and works; -reduce is not built
    r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "d.pgm", "-LUTFolder", lutdir, "-drop", 2)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "r.pgm", "-LUTFolder", lutdir, "-reduce", 1)
    assert r.returncode != 0 and BUILT in r.stdout
    for extra in (("-video", 1, "-frames", 2), ("-isRGB", 1, "-components", 3)):
        r = _run("-cd", 0, "-i", raw, "-o", tmp_path / "y.enc", "-xSize", W, "-ySize", H, "-wl", wl, "-bps", bd, "-LUTFolder", lutdir, *extra)
        assert r.returncode != 0 and BUILT in r.stdout
