"""Reference model of the training statistics (picsong_train_*): a numpy restatement of what the two-pass coder
(-cp 2, k = 0) codes -- every call site of the oracle's po_cb_encode at cbp = 0 as one increment at
counts[entry][symbol], entry = the index po_lut_at reads (raw index, clamped to the table).  No arithmetic coder: at
k = 0 the sequence of (entry, symbol) pairs depends on the coefficients alone.

TEST INFRASTRUCTURE ONLY, and independent of the kernel: the significance pass is walked site by site in the coder's
order (rows 0..63; in a row the 32 even columns, then the 32 odd ones), contexts taken from the state before the site.
All codeblocks of the array advance together; a site is vectorised over its 32 columns."""
import numpy as np

GEO_DEFAULT = dict(n_bitplanes=15, n_subbands=3, ctx_ref=1, ctx_sign=4, ctx_sig=9, precision=7)

# po_sign_ctx_hv (computeSignContext): index (h + 2) * 5 + (v + 2), h and v in -2..2 taken by their sign
_SIGN_CTX = np.zeros(25, np.int64)
for _h in range(-2, 3):
    for _v in range(-2, 3):
        if _h == 0:
            _c = 0 if _v == 0 else (2 if _v > 0 else 3)
        elif _h > 0:
            _c = 4 if _v == 0 else (6 if _v > 0 else 0)
        else:
            _c = 5 if _v == 0 else (1 if _v > 0 else 7)
        _SIGN_CTX[(_h + 2) * 5 + (_v + 2)] = _c


def sections(geo, wl):
    """(n_ref, n_sig, n_sign) as picsong_lut_load derives them for `wl`; values given in `geo` win."""
    nB, nS = geo["n_bitplanes"], geo["n_subbands"]
    out = []
    for key, ctx in (("n_ref", "ctx_ref"), ("n_sig", "ctx_sig"), ("n_sign", "ctx_sign")):
        v = geo.get(key, 0)
        out.append(v if v > 0 else nS * nB * geo[ctx] * wl + nB * geo[ctx])
    return tuple(out)


def find_subband(x, y, AW, AH, wl):
    for a in range(1, wl + 1):
        cx, cy = x >= (AW >> a), y >= (AH >> a)
        if cx or cy:
            return a - 1, (2 if cy else 0) if cx else 1
    return wl, 0


def counts(coef, wl, geo=GEO_DEFAULT):
    """coef: (AH, AW) int32 or float32 Mallat array.  Returns (uint64 counts[n_ref + n_sig + n_sign][2], range flag)."""
    AH, AW = coef.shape
    ncx, ncy = AW // 64, AH // 64
    ncb = ncx * ncy
    nB, nS = geo["n_bitplanes"], geo["n_subbands"]
    c_ref, c_sig, c_sign = geo["ctx_ref"], geo["ctx_sig"], geo["ctx_sign"]
    n_ref, n_sig, n_sign = sections(geo, wl)
    total = n_ref + n_sig + n_sign
    v = np.trunc(coef).astype(np.int64) if coef.dtype.kind == "f" else coef.astype(np.int64)   # (int) truncation
    v = v.reshape(ncy, 64, ncx, 64).transpose(0, 2, 1, 3).reshape(ncb, 64, 64)
    mag, neg = np.abs(v), v < 0
    top = mag.reshape(ncb, -1).max(axis=1)
    msb = np.array([int(m).bit_length() - 1 for m in top])          # -1: an all-zero block
    flag = int(np.any(msb > 15))
    coded = (msb >= 0) & (msb <= 15)
    # the lane's group, from its own first column
    G = np.zeros((ncb, 32), np.int64)
    for cb in range(ncb):
        for t in range(32):
            lv, sb = find_subband((cb % ncx) * 64 + 2 * t, (cb // ncx) * 64, AW, AH, wl)
            G[cb, t] = lv * nS * nB + sb * nB
    hist = np.zeros(total * 2, np.int64)

    def add(entry, sym, where):
        e = np.clip(entry[where], 0, total - 1)
        hist[:] += np.bincount(e * 2 + sym[where], minlength=total * 2)

    sig = np.zeros((ncb, 66, 66), bool)                  # one sample of border: outside the block counts as 0
    con = np.zeros((ncb, 66, 66), np.int64)              # a significant coefficient's contribution: -1 negative, +1 positive
    sgn = np.where(neg, -1, 1)
    lanes = np.arange(32)
    for bp in range(int(msb[coded].max()) if coded.any() else -1, -1, -1):
        act = coded & (msb >= bp)
        before = sig[:, 1:65, 1:65].copy()
        bit = (mag >> bp) & 1
        for i in range(64):
            r = i + 1
            for par in (0, 1):
                c = 2 * lanes + par + 1
                cand = act[:, None] & ~sig[:, r, c]
                if not cand.any():
                    continue
                ctx = (sig[:, r - 1, c - 1].astype(np.int64) + sig[:, r - 1, c] + sig[:, r - 1, c + 1] + sig[:, r, c - 1] +
                       sig[:, r, c + 1] + sig[:, r + 1, c - 1] + sig[:, r + 1, c] + sig[:, r + 1, c + 1])
                h = np.sign(con[:, r, c - 1] + con[:, r, c + 1])
                w = np.sign(con[:, r - 1, c] + con[:, r + 1, c])
                sctx = _SIGN_CTX[(h + 2) * 5 + (w + 2)]
                b = bit[:, i, c - 1]
                add(n_ref + (G + bp) * c_sig + ctx, b, cand)
                new = cand & (b == 1)
                if new.any():
                    s = neg[:, i, c - 1]
                    add(n_ref + n_sig + (G + bp) * c_sign + (sctx >> 1), (s != ((sctx & 1) == 1)).astype(np.int64), new)
                    sig[:, r, c] |= new
                    con[:, r, c] = np.where(new, sgn[:, i, c - 1], con[:, r, c])
        # refinement: significant before this plane's significance pass
        m = before & act[:, None, None]
        Gc = np.repeat(G, 2, axis=1)[:, None, :]
        add(np.broadcast_to((Gc + bp) * c_ref, m.shape), bit, m)
    return hist.reshape(total, 2).astype(np.uint64), flag


def table_from_counts(cnt, precision=7, prior=None):
    """The rule of picsong_lut_from_counts."""
    z, o = cnt[:, 0].astype(object), cnt[:, 1].astype(object)
    out = np.empty(len(cnt), np.int32)
    for i in range(len(cnt)):
        t = int(z[i]) + int(o[i])
        if t == 0:
            out[i] = (1 << (precision - 1)) if prior is None else prior[i]
        else:
            out[i] = min(max(((int(z[i]) << precision) + t // 2) // t, 1), (1 << precision) - 1)
    return out


def ideal_codewords(cnt, table, precision=7):
    """Ideal code length of the counted symbols under `table`, in 16-bit codewords: -sum log2 p / 16.  A probability
    the 16-bit interval cannot hold costs a whole codeword."""
    p0 = np.clip(table[:len(cnt)].astype(np.float64) / (1 << precision), 2.0 ** -16, 1.0 - 2.0 ** -16)
    bits = -(cnt[:, 0].astype(np.float64) * np.log2(p0) + cnt[:, 1].astype(np.float64) * np.log2(1.0 - p0))
    return float(bits.sum()) / 16.0
