"""The reference model of the training statistics (train_ref.py) checked against the coder itself: the ideal code length
of the counted symbols under the golden table, -sum log2 p, predicts the codewords the oracle writes with that table."""
import pytest

import oracle_lib as orc
import train_cases as tc
import train_ref as tr


@pytest.mark.parametrize("W,H,wl", tc.SHAPES)
def test_counts_predict_the_oracles_codewords(W, H, wl):
    coef = tc.frame_coeffs(W, H, wl, False)
    lut = orc.lut_for(False, wl)
    assert {k: v for k, v in lut.geometry().items() if not k.startswith("n_r") and not k.startswith("n_si")} == tc.GEO
    cnt, flag = tc.model_of_frame(W, H, wl, False, 0)
    assert flag == 0 and len(cnt) == lut.total
    _, sizes = orc.bpc_encode(coef, wl, lut)
    codewords = int(sizes.sum()) - sizes.size            # a codeblock's size counts its MSB word
    ratio = tr.ideal_codewords(cnt, lut.table) / codewords
    print(f"{W}x{H} wl {wl}: ideal / coded = {ratio:.4f}")
    # an arithmetic coder cannot beat the ideal length, and 16-bit codewords with a flush a lane lose a few percent
    assert 0.95 <= ratio <= 1.00


def test_every_symbol_is_counted_once():
    """A block's coefficients: one significance symbol a plane until significant, one sign, one refinement a plane after."""
    coef, wl = tc.case("frame0")
    cnt, _ = tc.model("frame0")
    n_ref, n_sig, n_sign = tr.sections(tc.GEO, wl)
    assert int(cnt[n_ref + n_sig:].sum()) == int((coef != 0).sum())          # a sign per non-zero coefficient
    assert int(cnt[n_ref:n_ref + n_sig, 1].sum()) == int((coef != 0).sum())  # ... and one significance 1
