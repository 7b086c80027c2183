"""Host-side training calls of the C ABI (no GPU): the counts -> table rule, the LUT folder writer against both loaders,
and the refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as orc
import picsong_amd as pa
import train_ref as tr

ERR_ARG, ERR_IO = -1, -3


def _info(wl, **geo):
    g = dict(tr.GEO_DEFAULT, **geo)
    n_ref, n_sig, n_sign = tr.sections(g, wl)
    return pa.LutInfo(n_files=3, n_bp_files=1, n_ref=n_ref, n_sig=n_sig, n_sign=n_sign, n_tables=1, cp=2, **g)


def test_table_rule_on_hand_made_counts():
    info = _info(1)
    n = info.n_ref + info.n_sig + info.n_sign
    cnt = np.zeros((n, 2), np.uint64)
    cnt[1] = (10, 0)              # only zeros: clamped to 2^7 - 1
    cnt[2] = (0, 10)              # only ones: clamped to 1
    cnt[3] = (3, 253)             # 3 * 128 / 256 = 1.5: rounds up
    cnt[4] = (5, 251)             # 2.5 -> 3
    cnt[5] = (1, 1)               # 64
    cnt[6] = (1, 2)               # 128 / 3 = 42.67 -> 43
    cnt[7] = (1 << 40, 3 << 40)   # large counts: 32
    cnt[8] = (1, 1000)            # 0.128 -> 0, clamped to 1
    t = pa.lut_from_counts(info, cnt)
    assert list(t[:9]) == [64, 127, 1, 2, 3, 64, 43, 32, 1]
    assert np.all(t[9:] == 64)                                   # unseen, no prior: 2^(precision - 1)
    prior = np.arange(n, dtype=np.int32) % 200
    tp = pa.lut_from_counts(info, cnt, prior)
    assert list(tp[1:9]) == list(t[1:9]) and tp[0] == prior[0] and np.array_equal(tp[9:], prior[9:])
    # the rule against its restatement, random counts, another precision
    rng = np.random.default_rng(5)
    cnt = rng.integers(0, 1000, (n, 2)).astype(np.uint64) * (rng.integers(0, 3, (n, 1)) > 0).astype(np.uint64)
    for prec in (7, 5):
        info.precision = prec
        assert np.array_equal(pa.lut_from_counts(info, cnt), tr.table_from_counts(cnt, prec))


@pytest.mark.parametrize("wl", [1, 5])
@pytest.mark.parametrize("component", [0, 1])
def test_save_then_load_is_the_identity(tmp_path, wl, component):
    info = _info(wl)
    n = info.n_ref + info.n_sig + info.n_sign
    table = np.random.default_rng(wl * 4 + component).integers(0, 256, n).astype(np.int32)
    folder = str(tmp_path / "trained")                         # (absent: created)
    pa.lut_save(folder, component, info, wl, table)
    stems = ["", "R"][component]
    assert sorted(os.listdir(folder)) == sorted(["header.txt"] + [f"{s}{stems}.txt_0" for s in ("ref", "sig", "sign")])
    assert open(os.path.join(folder, "header.txt")).read().split() == [
        "LUT_N_BITPLANES;15", "LUT_N_SUBBANDS;3", "N_CONTEXT_REFINEMENT;1", "N_CONTEXT_SIGN;4", "N_CONTEXT_SIGNIFICANCE;9",
        "MULT_PRECISION;7", "LUT_N_FILES;3", "AMOUNT_OF_BITPLANE_FILES;1"]
    first = open(os.path.join(folder, f"sig{stems}.txt_0")).readline().split()
    assert first[:4] == ["0", "0", "0", ":"] and [int(x) for x in first[4:]] == list(table[info.n_ref:info.n_ref + 9])
    for fill in (0, 77):
        got_info, got = pa.lut_load(folder, wl, component=component, fill=fill)
        assert np.array_equal(got, table)
        assert (got_info.n_ref, got_info.n_sig, got_info.n_sign) == (info.n_ref, info.n_sig, info.n_sign)
        assert np.array_equal(orc.Lut(folder, wl, component, fill).table, table)       # the oracle's loader
    pa.lut_save(folder + "/", component, info, wl, table)      # (present: overwritten)


def test_save_other_geometry(tmp_path):
    info = _info(2, n_bitplanes=12, ctx_ref=2, ctx_sig=5)
    n = info.n_ref + info.n_sig + info.n_sign
    table = np.random.default_rng(1).integers(1, 128, n).astype(np.int32)
    pa.lut_save(str(tmp_path / "g"), 2, info, 2, table)
    assert np.array_equal(pa.lut_load(str(tmp_path / "g"), 2, component=2, fill=9)[1], table)
    assert np.array_equal(orc.Lut(str(tmp_path / "g"), 2, 2, 9).table, table)


def test_refusals_without_a_device(tmp_path):
    L = pa.load()
    info = _info(2)
    n = info.n_ref + info.n_sig + info.n_sign
    table = np.full(n, 64, np.int32)
    cnt = np.zeros((n, 2), np.uint64)
    tp, cp = table.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)
    # training calls on no context
    assert L.picsong_train_begin(None, C.byref(info)) == ERR_ARG
    assert L.picsong_train_reset(None) == ERR_ARG and L.picsong_train_end(None) == ERR_ARG
    assert L.picsong_train_coeffs(None, 0, tp, None) == ERR_ARG
    assert L.picsong_train_frames(None, 1, tp, 0, None) == ERR_ARG
    assert L.picsong_train_rgb_frame(None, tp, tp, tp, None) == ERR_ARG
    assert L.picsong_train_counts(None, 0, None, None, 0) == ERR_ARG
    assert L.picsong_train_info(None, C.byref(info)) == ERR_ARG
    assert b"train" in L.picsong_last_error()
    # the rule: null arguments, a geometry without section sizes, a precision the coder cannot use
    assert L.picsong_lut_from_counts(None, cp, None, tp) == ERR_ARG
    assert L.picsong_lut_from_counts(C.byref(info), None, None, tp) == ERR_ARG
    bare = pa.LutInfo(**tr.GEO_DEFAULT)
    assert L.picsong_lut_from_counts(C.byref(bare), cp, None, tp) == ERR_ARG
    assert L.picsong_lut_from_counts(C.byref(_info(2, precision=0)), cp, None, tp) == ERR_ARG
    # the writer: sections of another wl, component / wl out of range, nothing written
    out = str(tmp_path / "no")
    assert L.picsong_lut_save(out.encode(), 1, C.byref(info), 3, tp) == ERR_ARG
    assert L.picsong_lut_save(out.encode(), 4, C.byref(info), 2, tp) == ERR_ARG
    assert L.picsong_lut_save(out.encode(), 1, C.byref(info), 0, tp) == ERR_ARG
    assert L.picsong_lut_save(None, 1, C.byref(info), 2, tp) == ERR_ARG
    assert not os.path.exists(out)
    # a folder that cannot be created: PICSONG_ERR_IO
    blocker = tmp_path / "file"
    blocker.write_text("x")
    assert L.picsong_lut_save(str(blocker / "sub").encode(), 1, C.byref(info), 2, tp) == ERR_IO
    assert L.picsong_lut_save(str(blocker).encode(), 1, C.byref(info), 2, tp) == ERR_IO
    assert blocker.read_text() == "x"
