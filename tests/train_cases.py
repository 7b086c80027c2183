"""Coefficient arrays the training-statistics tests share (emulated and GPU), with the reference model's counts of each
computed once per process."""
import functools

import numpy as np

import oracle_lib as orc
import train_ref as tr

SHAPES = [(128, 128, 1), (192, 128, 2), (256, 192, 3)]       # 192 x 128 wl 2: codeblocks that straddle subbands
GEO = dict(tr.GEO_DEFAULT)


def coeffs_of(img, wl, lossy, qs=0.5):
    """The oracle's transform of a frame: (AH, AW) int32 (5/3) or float32 (9/7 at qs) Mallat array."""
    x = orc.level_shift_fwd(orc.pad_frame(img), lossy)
    AH, AW = x.shape
    return np.ascontiguousarray(orc.dwt_forward(x, wl, qs)[:AW * AH].reshape(AH, AW))


@functools.lru_cache(maxsize=None)
def frame_coeffs(W, H, wl, lossy, frame=0, qs=0.5):
    return coeffs_of(orc.gen_frame(W, H, frame), wl, lossy, qs)


@functools.lru_cache(maxsize=None)
def case(name):
    """(coefficients (AH, AW), wl) of a named case."""
    if name.startswith("frame"):
        W, H, wl = SHAPES[int(name[5:])]
        return frame_coeffs(W, H, wl, False), wl
    if name == "deep":                                       # MSB up to 15: the index of bit-plane 15 aliases into the next group
        return orc.deep_coeffs(192, 128, 7), 2
    if name == "float97":                                    # float coefficients, truncated by the coder
        return frame_coeffs(256, 192, 3, True), 3
    if name == "zero_and_over":                              # an all-zero codeblock, and one of MSB 16 (skipped, flag raised)
        c = frame_coeffs(192, 128, 2, False).copy()
        c[0:64, 64:128] = 0
        c[64:128, 0:64] = 0
        c[70, 9] = -(1 << 16)
        return c, 2
    raise ValueError(name)


CASES = ["frame0", "frame1", "frame2", "deep", "float97", "zero_and_over"]


@functools.lru_cache(maxsize=None)
def model(name):
    """(counts[entries][2] uint64, range flag) of the reference model; do not modify."""
    c, wl = case(name)
    cnt, flag = tr.counts(c, wl, GEO)
    cnt.setflags(write=False)
    return cnt, flag


@functools.lru_cache(maxsize=None)
def model_of_frame(W, H, wl, lossy, frame, qs=0.5):
    cnt, flag = tr.counts(frame_coeffs(W, H, wl, lossy, frame, qs), wl, GEO)
    cnt.setflags(write=False)
    return cnt, flag
