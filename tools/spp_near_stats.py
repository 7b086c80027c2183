#!/usr/bin/env python3
"""What the k = 0 encoder's carry-read bodies meet on a frame (CPU count over the oracle's coefficients, test
infrastructure): per plane step of a wave (two codeblocks, 32 lanes each, two columns a lane),

  * the significance half-passes (32 rows) by the number of rows WITHOUT work -- 0 is the fully dense body
    (PICSONG_ENC_SPP_DENSE), 1 .. PICSONG_ENC_SPP_NEAR_MAX the near-dense one (PICSONG_ENC_SPP_NEAR), 32 is skipped --
    and, in the near-dense ones, the 4-row groups with no row set;
  * the column sites (a row of one column: 64 a half-pass) of the fully dense significance half-passes at which no lane
    codes: what PICSONG_ENC_DENSE_NOTEST no longer tests for;
  * the same for the dense refinement half-passes (5 popcount(rows) >= 3 last), apart for those in which every visited
    row has work (popcount(rows) == last: the untested loop) and the others.

A row has work in the significance pass if some lane of a codeblock that codes a plane at that step has an insignificant
coefficient in it, in the refinement pass if some lane has a significant one.  Step 0 (the first plane's body) and the raw
fallback are not modelled.
usage: tools/spp_near_stats.py [W H wl [near_max]]   (default: the bench's 8K lossless frame, 4)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as orc

W, H, wl = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (7680, 4320, 5)
NEAR = int(sys.argv[4]) if len(sys.argv) >= 5 else 4
orc.set_threads(orc.usable_threads())
img = orc.pad_frame(orc.gen_frame(W, H, 0))
AH, AW = img.shape
coef = orc.dwt_forward(orc.level_shift_fwd(img, False), wl)[:AW * AH].reshape(AH, AW)
mag = np.abs(np.trunc(np.asarray(coef, np.float64))).astype(np.int32)
ncx, ncy = AW // 64, AH // 64
blk = mag.reshape(ncy, 64, ncx, 64).transpose(0, 2, 1, 3).reshape(ncx * ncy, 64, 64)
if blk.shape[0] & 1:
    blk = np.concatenate([blk, np.zeros((1, 64, 64), np.int32)])
nw = blk.shape[0] // 2
wv = blk.reshape(nw, 2, 64, 32, 2)                            # wave, half, row, lane, column of the lane
msb = np.array([int(v).bit_length() - 1 for v in blk.reshape(2 * nw, -1).max(axis=1)]).reshape(nw, 2)
steps = int(msb.max()) + 1
print(f"{W}x{H} wl {wl}: {nw} waves, near_max {NEAR}; per plane step, half-passes of the frame")
print("step | sig half-passes: 0 rows without work / 1 / 2 / 3 / 4 / 5-8 / 9-31 / 32 (skipped) | near: empty rows per pass,"
      " empty groups | dense sig sites: empty / all | ref dense, all rows with work: passes, sites empty / all | ref dense,"
      " other: passes, sites empty / all | ref generic passes")
tot = np.zeros(12, np.int64)
hist_all = np.zeros(33, np.int64)
for p in range(1, steps):
    bp = msb - p                                             # the plane each half codes at this step
    act = (msb >= 0) & (bp >= 0)
    sh = np.where(act, bp + 1, 0).astype(np.int32)
    sig = ((wv >> sh[:, :, None, None, None]) != 0)
    a = act[:, :, None, None, None]
    ins = (~sig & a).any(axis=(1, 3))                        # wave, row, column: some lane has an insignificant coefficient
    sg = (sig & a).any(axis=(1, 3))                          # ... a significant one
    # significance
    work = ins.any(axis=2).reshape(nw, 2, 32)
    nwo = 32 - work.sum(axis=2)
    hist = np.bincount(nwo.ravel(), minlength=33)
    hist_all += hist
    full = nwo == 0
    near = (nwo >= 1) & (nwo <= NEAR)
    site = ins.reshape(nw, 2, 32, 2)
    d_all = int(full.sum()) * 64
    d_empty = int((~site[full]).sum())
    n_rows = int(nwo[near].sum())
    n_grp = int((~work.reshape(nw, 2, 8, 4).any(axis=3))[near].sum())
    # refinement
    rw = sg.any(axis=2).reshape(nw, 2, 32)
    pop = rw.sum(axis=2)
    last = np.where(pop > 0, 32 - np.argmax(rw[:, :, ::-1], axis=2), 0)
    dense = (5 * pop >= 3 * last) & (last > 0)
    allw = dense & (pop == last)
    oth = dense & (pop != last)
    vis = np.arange(32)[None, None, :] < last[:, :, None]
    rsite = sg.reshape(nw, 2, 32, 2)
    r_emp = vis[:, :, :, None] & ~rsite
    ra_all, ra_emp = 2 * int(last[allw].sum()), int(r_emp[allw].sum())
    ro_all, ro_emp = 2 * int(last[oth].sum()), int(r_emp[oth].sum())
    gen = int(((pop > 0) & ~dense).sum())
    h = hist
    print(f"{p:4d} | {h[0]} / {h[1]} / {h[2]} / {h[3]} / {h[4]} / {h[5:9].sum()} / {h[9:32].sum()} / {h[32]} | "
          f"{n_rows / max(int(near.sum()), 1):.2f}, {n_grp} | {d_empty} / {d_all} | {int(allw.sum())}, {ra_emp} / {ra_all} | "
          f"{int(oth.sum())}, {ro_emp} / {ro_all} | {gen}")
    tot += np.array([d_empty, d_all, int(allw.sum()), ra_emp, ra_all, int(oth.sum()), ro_emp, ro_all, gen,
                     int(near.sum()), n_rows, n_grp])
print(f"all steps: sig half-passes by rows without work 0: {hist_all[0]}, 1: {hist_all[1]}, 2: {hist_all[2]}, 3: {hist_all[3]}, "
      f"4: {hist_all[4]}, 5-8: {hist_all[5:9].sum()}, 9-31: {hist_all[9:32].sum()}, 32: {hist_all[32]}")
print(f"near-dense (1..{NEAR}): {tot[9]} half-passes, {tot[10]} rows without work, {tot[11]} empty groups")
print(f"dense sig sites empty: {tot[0]} of {tot[1]} ({100.0 * tot[0] / max(tot[1], 1):.2f} %)")
print(f"dense ref, every visited row with work: {tot[2]} half-passes, sites empty {tot[3]} of {tot[4]} "
      f"({100.0 * tot[3] / max(tot[4], 1):.2f} %)")
print(f"dense ref, other: {tot[5]} half-passes, sites empty {tot[6]} of {tot[7]} ({100.0 * tot[6] / max(tot[7], 1):.2f} %); "
      f"generic ref half-passes: {tot[8]}")
