"""The reduced-quality decode's host side, no GPU needed: picsong_drop_planes through the real library -- its values
against drop_ref for every codeblock, and what it refuses -- and the command-line tool's -drop refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import drop_ref as dr
import picsong_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host", "PICSONG")
ERR_ARG = -1                                                      # PICSONG_ERR_ARG


def test_drop_planes_values():
    for AW, AH in ((704, 512), (576, 320), (832, 320), (7680, 4352)):
        for wl in range(1, 8 if AW > 1000 else 6):
            for cb in range((AW // 64) * (AH // 64)):
                for drop in (0, 1, wl, wl + 1, 15):
                    assert pa.drop_planes(AW, AH, wl, drop, cb) == dr.drop_planes(AW, AH, wl, drop, cb), (AW, AH, wl, drop, cb)
    # the LL codeblock of a five-level frame keeps every plane up to drop 5; a finest-level one loses `drop` planes
    assert [pa.drop_planes(7680, 4352, 5, d, 0) for d in (0, 5, 6, 15)] == [0, 0, 1, 10]
    assert [pa.drop_planes(7680, 4352, 5, d, 119) for d in (0, 1, 6, 15)] == [0, 1, 6, 15]


@pytest.mark.parametrize("aw,ah,wl,drop,cb", [
    (0, 512, 3, 1, 0), (704, 0, 3, 1, 0), (700, 512, 3, 1, 0), (704, 500, 3, 1, 0), (-64, 64, 1, 1, 0),      # geometry
    (704, 512, 0, 1, 0), (704, 512, 8, 1, 0),                                                                # wl
    (704, 512, 3, -1, 0), (704, 512, 3, 16, 0),                                                              # drop
    (704, 512, 3, 1, -1), (704, 512, 3, 1, 88),                                                              # index
])
def test_drop_planes_refusals(aw, ah, wl, drop, cb):
    L = pa.load()
    d = C.c_int(-77)
    assert L.picsong_drop_planes(aw, ah, wl, drop, cb, C.byref(d)) == ERR_ARG
    assert d.value == -77 and b"drop_planes" in L.picsong_last_error()
    with pytest.raises(pa.PicsongError):
        pa.drop_planes(aw, ah, wl, drop, cb)


def test_drop_planes_null_and_last_codeblock():
    L = pa.load()
    assert L.picsong_drop_planes(704, 512, 3, 1, 0, None) == ERR_ARG
    assert pa.drop_planes(704, 512, 3, 3, 87) == 3
    assert L.picsong_ctx_set_decode_drop(None, 1) == ERR_ARG
    assert L.picsong_ctx_get_decode_drop(None, None) == ERR_ARG


# ---- the command-line tool ----------------------------------------------------------------------------------------------
def _run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN)])


def test_cli_help_and_argument_refusals(built, tmp_path):
    assert "-drop d" in _run("-h").stdout
    r = _run("-cd", 0, "-i", "/etc/hostname", "-o", tmp_path / "x", "-xSize", 64, "-ySize", 64, "-drop", 1)
    assert r.returncode == 255 and "Incorrect parameters. -drop applies to decoding" in r.stdout
    for bad in (-1, 16):
        r = _run("-cd", 1, "-i", "/etc/hostname", "-o", tmp_path / "x", "-drop", bad)
        assert r.returncode == 255 and "Incorrect parameters. -drop takes a number of bit-planes in 0..15" in r.stdout


@pytest.mark.parametrize("cp,k_1e3", [(2, 500), (3, 0)])
def test_cli_refuses_streams_coded_otherwise(built, oracle, tmp_path, cp, k_1e3):
    """A stream whose header says -k > 0 or -cp 3: refused from the header alone, before any device is touched."""
    hdr = oracle.header_pack(n_samples=128 * 128, cp=cp, cb_height=18, cb_width=64, wl=2, bit_depth=8, lossy=0, qs_1e4=10000,
                             components=1, is_rgb=0, height=128, endianess=0, bps=8, is_signed=0, frames=0, k_1e3=k_1e3)
    enc = tmp_path / "s.enc"
    np.concatenate([hdr, np.zeros(40, np.uint16)]).tofile(enc)
    r = _run("-cd", 1, "-i", enc, "-o", tmp_path / "s.pgm", "-LUTFolder", os.path.join(oracle.LUT_DIR, "n1_lossless"), "-drop", 2)
    assert r.returncode == 255 and "Incorrect parameters. -drop applies to -cp 2 streams coded at -k 0" in r.stdout
