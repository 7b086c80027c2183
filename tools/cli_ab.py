#!/usr/bin/env python3
"""A/B of two builds of the PICSONG command-line tool: cli_ab.py <old binary> <new binary> [--out profiles/cli_ab.json].

Both binaries run over ONE list of command lines, one process at a time, each in a folder of its own with the same
relative file names.  Compared per command: the exit status, stdout (the numbers of the timing lines masked), every file
the command left in the folder byte for byte (outputs, _SIZE sidecars, trained LUT folders) and the --metrics JSON (its
keys in order; the values of seconds, mpixels_per_s and *_ms masked).  Exit status 1 on any difference; 2 where a run
ended by a signal or its time limit -- nothing is started after that.

The inputs are the CLI tests' own: tests/oracle_lib.gen_frame frames, tests/layout_ref.pack for the interleaved layouts,
the LUT folders under tests/golden.  Small shapes only: 200 x 136 (padded to 256 x 192) and 128 x 128 (padded already)."""
import argparse
import filecmp
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import layout_ref as lr          # noqa: E402
import oracle_lib as orc         # noqa: E402

LOSSLESS, LOSSY = os.path.join(orc.LUT_DIR, "n1_lossless"), os.path.join(orc.LUT_DIR, "n1_lossy")
CP3 = os.path.join(orc.LUT_CP3_DIR, "n1_lossless")
TIMING = re.compile(r"^(The time spent with the app[^:]*is: |BPC acum time is: )\S+$", re.M)
PIPELINE = re.compile(r"((?:readers\)|for frames|launching|for the GPU|writing) )[-+.e0-9]+")
MASKED_KEYS = ("seconds", "mpixels_per_s")


def make_inputs(d):
    """The raw files every command reads, by name."""
    os.makedirs(d)
    for tag, (W, H) in (("a", (200, 136)), ("b", (128, 128))):
        grey = [orc.gen_frame(W, H, f) for f in range(9)]
        np.concatenate([g.ravel() for g in grey]).tofile(os.path.join(d, f"grey_{tag}.raw"))
        planes = [[orc.gen_frame(W, H, 10 * f + c) for c in range(3)] for f in range(5)]
        np.concatenate([p.ravel() for fr in planes for p in fr]).tofile(os.path.join(d, f"planar_{tag}.raw"))
        for layout in (lr.RGB24, lr.BGRA32):
            data = [lr.pack(fr, layout, W * lr.BPP[layout], W * H, alpha=9) for fr in planes]
            np.concatenate(data).tofile(os.path.join(d, f"{lr.NAMES[layout]}_{tag}.raw"))
    W, H = 200, 136
    deep = (orc.gen_frame(W, H, 5).astype(np.uint16) * 16 + orc.gen_frame(W, H, 6) % 16).astype(">u2")
    with open(os.path.join(d, "deep12.pgm"), "wb") as f:
        f.write(f"P5\n# 12 bits\n{W} {H}\n4095\n".encode() + deep.tobytes())
    # three 12-bit RGB frames: planar (R, G, B planes a frame) and interleaved, 6 bytes a pixel
    deep_rgb = [[(orc.gen_frame(W, H, 20 * f + c).astype(np.uint16) * 16 + orc.gen_frame(W, H, 20 * f + c + 7) % 16).astype("<u2")
                 for c in range(3)] for f in range(3)]
    np.concatenate([p.ravel() for fr in deep_rgb for p in fr]).tofile(os.path.join(d, "deep12_planar.raw"))
    np.concatenate([np.stack(fr, axis=-1).ravel() for fr in deep_rgb]).tofile(os.path.join(d, "deep12_rgb48.raw"))
    raw = open(os.path.join(d, "grey_a.raw"), "rb").read()
    open(os.path.join(d, "grey_a_5.raw"), "wb").write(raw[:5 * W * H])                   # (-compare: the frames coded)
    open(os.path.join(d, "grey_a_truncated.raw"), "wb").write(raw[:2 * W * H + 1000])    # short within the first group
    # (the -cp 3 folder has the R tables only: an RGB run gets a folder with them under the G and B names too)
    shutil.copytree(CP3, os.path.join(d, "lut_cp3_rgb"))
    for f in os.listdir(CP3):
        for c in "GB":
            if "R.txt" in f:
                shutil.copy(os.path.join(CP3, f), os.path.join(d, "lut_cp3_rgb", f.replace("R.txt", c + ".txt")))
    open(os.path.join(d, "planar_a_1.raw"), "wb").write(open(os.path.join(d, "planar_a.raw"), "rb").read()[:3 * W * H])


def commands():
    """(name, argv, prepare) in running order; a decode reads what an earlier encode of the same folder wrote.  `prepare`
    (or None) names a step done in the folder before the command."""
    A, B = ("-xSize", 200, "-ySize", 136), ("-xSize", 128, "-ySize", 128)
    RGB = ("-isRGB", 1, "-components", 3)
    out = []
    encoded = []                                   # (name, is video, decode LUT folder)

    def enc(name, inp, lut, *args, video=0, ok=True):
        v = ("-video", 1, "-frames", video) if video else ()
        out.append((name, ["-cd", 0, "-i", f"../in/{inp}", "-o", f"{name}.enc", "-LUTFolder", lut, *v, *args], None))
        if ok:
            encoded.append((name, bool(video), lut))

    # ---- images and videos, grey and RGB, 5/3 and 9/7, -k 0 and 0.5, -cp 3
    enc("img_grey_a_53", "grey_a.raw", LOSSLESS, *A, "-wl", 3, "-type", 0, "--metrics", "img_grey_a_53.json")
    enc("img_grey_a_97_k", "grey_a.raw", LOSSY, *A, "-wl", 3, "-type", 1, "-qs", 0.5, "-k", 0.5)
    enc("img_grey_b_53", "grey_b.raw", LOSSLESS, *B, "-wl", 2, "-type", 0)
    enc("img_rgb_a_53", "planar_a.raw", LOSSLESS, *A, *RGB, "-wl", 3, "-type", 0)
    enc("img_rgb_a_97_k", "planar_a.raw", LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-qs", 0.5, "-k", 0.5, "--metrics", "img_rgb_a_97_k.json")
    enc("img_grey_a_cp3", "grey_a.raw", CP3, *A, "-wl", 3, "-type", 0, "-cp", 3)
    enc("vid_grey_a_cp3", "grey_a.raw", CP3, *A, "-wl", 3, "-type", 0, "-cp", 3, video=3)
    enc("vid_grey_a_9_b1", "grey_a.raw", LOSSLESS, *A, "-wl", 3, "-type", 0, "-framesPerLaunch", 1, video=9)      # 6 slots, reused
    enc("vid_grey_a_5_b2", "grey_a.raw", LOSSY, *A, "-wl", 3, "-type", 1, "-qs", 0.5, "-framesPerLaunch", 2, video=5)
    enc("vid_grey_a_5_k", "grey_a.raw", LOSSY, *A, "-wl", 3, "-type", 1, "-qs", 0.5, "-k", 0.5, video=5)
    enc("vid_grey_b_5", "grey_b.raw", LOSSLESS, *B, "-wl", 2, "-type", 0, "--metrics", "vid_grey_b_5.json", video=5)   # the direct read
    enc("vid_grey_a_dev00", "grey_a.raw", LOSSLESS, *A, "-wl", 3, "-type", 0, "--devices", "0,0", "-framesPerLaunch", 2, video=9)
    enc("vid_rgb_a_5", "planar_a.raw", LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-qs", 0.5, video=5)
    enc("vid_rgb_a_5_b2", "planar_a.raw", LOSSLESS, *A, *RGB, "-wl", 3, "-type", 0, "-framesPerLaunch", 2, video=5)
    enc("vid_rgb_b_5", "planar_b.raw", LOSSLESS, *B, *RGB, "-wl", 2, "-type", 0, "--metrics", "vid_rgb_b_5.json", video=5)
    enc("img_rgb_a_cp3", "planar_a.raw", "../in/lut_cp3_rgb", *A, *RGB, "-wl", 3, "-type", 0, "-cp", 3)
    enc("vid_rgb_a_cp3", "planar_a.raw", "../in/lut_cp3_rgb", *A, *RGB, "-wl", 3, "-type", 0, "-cp", 3, video=2)
    # ---- -rate, -psnr, -ssim: a grey image, an RGB image, a grey video and an RGB video, with and without -searchFrames 3
    for flag, val in (("-rate", 2.0), ("-psnr", 38), ("-ssim", 0.97)):
        t = flag[1:]
        lossy = ("-wl", 3, "-type", 1, flag, val)
        enc(f"img_grey_a_{t}", "grey_a.raw", LOSSY, *A, *lossy, "--metrics", f"img_grey_a_{t}.json")
        enc(f"img_rgb_a_{t}", "planar_a.raw", LOSSY, *A, *RGB, *lossy, "--metrics", f"img_rgb_a_{t}.json")
        enc(f"vid_grey_a_{t}", "grey_a.raw", LOSSY, *A, *lossy, "--metrics", f"vid_grey_a_{t}.json", video=5)
        enc(f"vid_grey_a_{t}_sf3", "grey_a.raw", LOSSY, *A, *lossy, "-searchFrames", 3, video=5)
        enc(f"vid_rgb_a_{t}", "planar_a.raw", LOSSY, *A, *RGB, *lossy, video=5)
        enc(f"vid_rgb_a_{t}_sf3", "planar_a.raw", LOSSY, *A, *RGB, *lossy, "-searchFrames", 3, "--metrics", f"vid_rgb_a_{t}_sf3.json", video=5)
    # ---- -layout grey, planar, rgb, bgra: coding, alone and under a search
    enc("lay_img_grey_a", "grey_a.raw", LOSSLESS, *A, "-wl", 3, "-type", 0, "-layout", "grey")
    enc("lay_vid_grey_a", "grey_a.raw", LOSSLESS, *A, "-wl", 3, "-type", 0, "-layout", "grey", video=5)
    enc("lay_vid_grey_b_rate", "grey_b.raw", LOSSY, *B, "-wl", 2, "-type", 1, "-rate", 2.0, "-layout", "grey", video=5)
    for name in ("planar", "rgb", "bgra"):
        inp = "planar_a.raw" if name == "planar" else f"{name}_a.raw"
        enc(f"lay_img_{name}_a", inp, LOSSLESS, *A, *RGB, "-wl", 3, "-type", 0, "-layout", name)
        enc(f"lay_vid_{name}_a", inp, LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-qs", 0.5, "-layout", name, video=5)
    enc("lay_img_rgb_a_psnr", "rgb_a.raw", LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-psnr", 38, "-layout", "rgb")
    enc("lay_vid_bgra_a_rate", "bgra_a.raw", LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-rate", 2.0, "-layout", "bgra", video=5)
    enc("lay_vid_rgb_b_ssim_sf3", "rgb_b.raw", LOSSY, *B, *RGB, "-wl", 2, "-type", 1, "-ssim", 0.97, "-searchFrames", 3, "-layout", "rgb",
        video=5)
    # ---- one -bps 12 PGM; -train (a grey video, an RGB image)
    enc("deep12", "deep12.pgm", LOSSLESS, "-wl", 3, "-type", 0, "-bps", 12)
    # ---- -bps 12 RGB: an image from planar planes, a video from interleaved pixels, two frames a launch
    enc("deep12_rgb_img", "deep12_planar.raw", LOSSLESS, *A, *RGB, "-wl", 3, "-type", 0, "-bps", 12)
    enc("deep12_rgb_vid", "deep12_rgb48.raw", LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-qs", 0.25, "-bps", 12, "-layout", "rgb",
        "-framesPerLaunch", 2, video=3)
    out.append(("train_grey", ["-cd", 0, "-i", "../in/grey_a.raw", *A, "-wl", 3, "-video", 1, "-frames", 9, "-framesPerLaunch", 4,
                               "-train", "train_grey"], None))
    out.append(("train_rgb", ["-cd", 0, "-i", "../in/planar_b.raw", *B, *RGB, "-wl", 2, "-train", "train_rgb", "-LUTFolder", LOSSLESS], None))
    # ---- every encoded file decoded at full size, with -reduce 1, with -window 8,8,64,40 and with -drop 2 (what a mode
    # refuses, it refuses the same)
    for name, video, lut in encoded:
        v = ("-video", 1) if video else ()
        for tag, extra in (("full", ()), ("reduce", ("-reduce", 1)), ("window", ("-window", "8,8,64,40")), ("drop", ("-drop", 2))):
            if name.startswith("deep12") and tag in ("reduce", "window"):
                continue                                          # (refused before the stream is opened: nothing to compare)
            m = ("--metrics", f"{name}.{tag}.json") if name in ("vid_grey_b_5", "img_rgb_a_53", "vid_rgb_a_5") else ()
            out.append((f"{name}.{tag}", ["-cd", 1, "-i", f"{name}.enc", "-o", f"{name}.{tag}.dec", "-LUTFolder", lut, *v, *extra, *m], None))
    # ---- -layout, decoding; -framesPerLaunch, decoding; -compare
    for name, src, video in (("grey", "lay_img_grey_a", 0), ("grey", "lay_vid_grey_a", 1), ("planar", "lay_img_planar_a", 0),
                             ("rgb", "lay_vid_rgb_a", 1), ("bgra", "lay_img_bgra_a", 0), ("bgra", "vid_rgb_a_5_b2", 1)):
        lut = LOSSY if src == "lay_vid_rgb_a" else LOSSLESS
        out.append((f"{src}.as_{name}", ["-cd", 1, "-i", f"{src}.enc", "-o", f"{src}.as_{name}.dec", "-LUTFolder", lut,
                                         *(("-video", 1) if video else ()), "-layout", name, "-drop", 1], None))
    out.append(("vid_grey_a_9_b1.b2", ["-cd", 1, "-i", "vid_grey_a_9_b1.enc", "-o", "vid_grey_a_9_b1.b2.dec", "-LUTFolder", LOSSLESS, "-video", 1,
                                       "-framesPerLaunch", 2], None))
    out.append(("vid_rgb_a_5.b2", ["-cd", 1, "-i", "vid_rgb_a_5.enc", "-o", "vid_rgb_a_5.b2.dec", "-LUTFolder", LOSSY, "-video", 1,
                                   "-framesPerLaunch", 2, "-reduce", 1], None))
    out.append(("compare_grey", ["-cd", 1, "-i", "vid_grey_a_5_b2.enc", "-o", "compare_grey.dec", "-LUTFolder", LOSSY, "-video", 1,
                                 "-compare", "../in/grey_a_5.raw"], None))
    out.append(("compare_rgb", ["-cd", 1, "-i", "img_rgb_a_rate.enc", "-o", "compare_rgb.dec", "-LUTFolder", LOSSY,
                                "-compare", "../in/planar_a_1.raw"], None))
    # ---- what must fail, and fail the same: a truncated input (grey, RGB groups), an unreachable -rate, a _SIZE sidecar
    # with an entry too few
    enc("fail_truncated", "grey_a_truncated.raw", LOSSLESS, *A, "-wl", 3, "-type", 0, video=9, ok=False)
    enc("fail_truncated_rgb", "grey_a_truncated.raw", LOSSLESS, *A, *RGB, "-wl", 3, "-type", 0, video=2, ok=False)
    enc("fail_rate", "grey_a.raw", LOSSY, *A, "-wl", 3, "-type", 1, "-rate", 0.001, ok=False)
    enc("fail_rate_rgb_sf", "planar_a.raw", LOSSY, *A, *RGB, "-wl", 3, "-type", 1, "-rate", 0.001, "-searchFrames", 2, video=3, ok=False)
    out.append(("fail_short_size", ["-cd", 1, "-i", "short_size.enc", "-o", "short_size.dec", "-LUTFolder", LOSSLESS, "-video", 1], "short_size"))
    return out


def prepare(step, folder):
    if step == "short_size" and os.path.exists(os.path.join(folder, "vid_grey_a_9_b1.enc_SIZE")):
        # a video's stream with the last entry of its sidecar gone
        shutil.copy(os.path.join(folder, "vid_grey_a_9_b1.enc"), os.path.join(folder, "short_size.enc"))
        sizes = open(os.path.join(folder, "vid_grey_a_9_b1.enc_SIZE")).read().split(",")
        open(os.path.join(folder, "short_size.enc_SIZE"), "w").write(",".join(sizes[:-1]))


def tree(folder):
    return sorted(os.path.relpath(os.path.join(r, f), folder) for r, _, fs in os.walk(folder) for f in fs)


def masked_metrics(path):
    m = json.load(open(path))
    return [(k, None if k in MASKED_KEYS or k.endswith("_ms") else v) for k, v in m.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cli_ab.json"))
    ap.add_argument("--timeout", type=int, default=60, help="seconds a run may take (small shapes: a run takes about one)")
    ap.add_argument("--keep", action="store_true", help="keep the work folder")
    a = ap.parse_args()
    work = tempfile.mkdtemp(prefix="cli_ab_")
    make_inputs(os.path.join(work, "in"))
    sides = {"old": os.path.abspath(a.old), "new": os.path.abspath(a.new)}
    for side in sides:
        os.makedirs(os.path.join(work, side))
    report = {"old": a.old, "new": a.new, "commands": 0, "differences": [], "not_ok": [], "stopped": None, "seconds": {"old": 0.0, "new": 0.0}}
    status = 0
    for name, argv, step in commands():
        got = {}
        for side, binary in sides.items():
            folder = os.path.join(work, side)
            if step:
                prepare(step, folder)
            before = set(tree(folder))
            t0 = time.time()
            r = subprocess.run(["timeout", "-k", "10", str(a.timeout), binary, *map(str, argv)], cwd=folder, capture_output=True, text=True)
            report["seconds"][side] += time.time() - t0
            # a signal (128 + n from timeout's child, negative from timeout itself) or the time limit: nothing runs after it
            if r.returncode < 0 or r.returncode in (124, 137) or 128 < r.returncode < 255:
                report["stopped"] = {"command": name, "side": side, "status": r.returncode, "argv": list(map(str, argv)),
                                     "stdout": r.stdout[-2000:], "stderr": r.stderr[-2000:]}
                status = 2
                break
            got[side] = (r.returncode, PIPELINE.sub(r"\1#", TIMING.sub(r"\1#", r.stdout)), r.stderr, sorted(set(tree(folder)) - before))
        if status == 2:
            break
        report["commands"] += 1
        if got["new"][0] != 0:                     # what was refused, or failed, and how
            said = [ln for ln in got["new"][1].split("\n") if ln and not ln.startswith(("User entered", "The time spent"))]
            report["not_ok"].append({"command": name, "status": got["new"][0], "said": said[-1][:200] if said else ""})
        why = []
        (rc_o, out_o, err_o, new_o), (rc_n, out_n, err_n, new_n) = got["old"], got["new"]
        if rc_o != rc_n:
            why.append(f"exit status {rc_o} != {rc_n}")
        if out_o != out_n:
            why.append("stdout differs: " + repr([(x, y) for x, y in zip(out_o.split("\n"), out_n.split("\n")) if x != y][:3]))
        if err_o != err_n:
            why.append("stderr differs")
        if new_o != new_n:
            why.append(f"files written differ: {new_o} != {new_n}")
        for f in new_o:
            fo, fn = os.path.join(work, "old", f), os.path.join(work, "new", f)
            if not os.path.exists(fn):
                continue
            if f.endswith(".json"):
                if masked_metrics(fo) != masked_metrics(fn):
                    why.append(f"{f}: metrics differ: {masked_metrics(fo)} != {masked_metrics(fn)}")
            elif not filecmp.cmp(fo, fn, shallow=False):
                why.append(f"{f}: bytes differ")
        if why:
            report["differences"].append({"command": name, "argv": list(map(str, argv)), "why": why})
            status = 1
        print(f"{'DIFF' if why else 'same'} {rc_o:3d} {name}" + "".join("\n     " + w for w in why), flush=True)
    report["files_compared"] = len(tree(os.path.join(work, "new")))
    report["seconds"] = {k: round(v, 1) for k, v in report["seconds"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"{report['commands']} commands, {len(report['differences'])} with differences, {report['files_compared']} files; "
          f"stopped: {report['stopped'] and report['stopped']['command']}; {a.out}")
    if a.keep:
        print("work folder kept:", work)
    else:
        shutil.rmtree(work, ignore_errors=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
