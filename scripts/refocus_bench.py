"""Refocus against defocus (include/rtdd.h rtdd_simulate_refocus, rtdd_simulate_defocus) at 1080p, 4K and 8K, automatic path: a smooth
depth map and a real one (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size); refocus at f = 0, at
f = 128 and in the pixel form (the focal depth read on the device).  Microseconds per call, host clock around a device synchronise,
the four calls alternated over several rounds: the median and the spread of the rounds.

    python scripts/refocus_bench.py [--out profiles/r07_refocus.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt
from realtimedepthdiffusion_amd.synth import make_problem

ROUNDS, CALLS = 7, 20


def timeit(f, n=CALLS):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6


def dog_depth():
    g = np.load(os.path.join(ROOT, "tests", "golden", "Dog_full.npz"), allow_pickle=False)
    bgr, ann = g["bgr"], g["annotation"]
    rows, cols = ann.shape
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4); c.pyramid_create(rows, cols)
        c.pyramid_set_image(rt.device_image(bgr)); c.pyramid_set_annotation(rt.device_image(ann))
        c.estimate_depth(1000); c.synchronize()
        return c.pyramid_download(rt.IMG_DEPTH, 0)


def tile(a, rows, cols):
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    return np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# refocus vs defocus, automatic path, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds)"]

    def say(s):
        print(s, flush=True); lines.append(s)

    dog = dog_depth()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K")):
        p = make_problem(rows, cols, seed=1)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        c = rt.Context(0)
        o = rt.device_image(orig); art = rt.device_image(np.zeros_like(orig))
        maps = {"smooth": rt.device_image(p["gray"].astype(np.float32)), "Dog tiled": rt.device_image(tile(dog, rows, cols))}
        x, y = cols // 2, rows // 2
        for mname, d in maps.items():
            calls = {"defocus": lambda: c.GPUSimulateDefocus(o, d, art, rows, cols),
                     "refocus f=0": lambda: c.simulate_refocus(o, d, art, rows, cols, 0.025, 0.0, -1, -1),
                     "refocus f=128": lambda: c.simulate_refocus(o, d, art, rows, cols, 0.025, 128.0, -1, -1),
                     "refocus pixel": lambda: c.simulate_refocus(o, d, art, rows, cols, 0.025, 0.0, x, y)}
            for f in calls.values():            # warm-up: code objects, the table's allocation
                for _ in range(3): f()
            t = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, f in calls.items():
                    t[k].append(timeit(f))
            med = {k: float(np.median(v)) for k, v in t.items()}
            line = f"{name:5s} {mname:9s} path {c.get_option(rt.OPT_DEFOCUS_LAST_PATH)}:"
            for k, v in t.items():
                line += f"  {k} {med[k]:7.1f} ({min(v):.1f}-{max(v):.1f})"
            line += f"  | refocus f=0 / defocus = {med['refocus f=0'] / med['defocus']:.3f}"
            say(line)
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
