"""Stereo against haze_ex (include/rtdd.h rtdd_simulate_stereo, rtdd_simulate_haze_ex) at 1080p, 4K and 8K: a smooth depth map and a
real one (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size); disparities of 1 % and 3 % of the width
and 256 (the largest admitted), zero parallax at 128.  haze_ex is the streaming effect that moves the same 10 B/px.
Microseconds per call, host clock around a device synchronise, the calls alternated over several rounds: the median and the spread.

    python scripts/stereo_bench.py [--out profiles/r08_stereo.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt

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
    lines = [f"# stereo vs haze_ex, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); z0 = 128, view mode"]

    def say(s):
        print(s, flush=True); lines.append(s)

    dog = dog_depth()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K")):
        yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
        smooth = (127.5 + 120 * np.sin(xx / 301.0) * np.cos(yy / 207.0)).astype(np.float32)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        c = rt.Context(0)
        o = rt.device_image(orig); art = rt.device_image(np.zeros_like(orig))
        for mname, dh in (("smooth", smooth), ("Dog tiled", tile(dog, rows, cols))):
            d = rt.device_image(dh)
            ds = (cols // 100, 3 * cols // 100, 256)
            calls = {"haze_ex": lambda: c.simulate_haze_ex(o, d, art, rows, cols, 2.0, (255, 255, 255))}
            for D in ds:
                calls[f"stereo D={D}"] = (lambda D=D: c.simulate_stereo(o, d, art, rows, cols, D, 128.0, -1, -1, rt.STEREO_VIEW))
            for f in calls.values():
                for _ in range(3): f()
            t = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, f in calls.items():
                    t[k].append(timeit(f))
            med = {k: float(np.median(v)) for k, v in t.items()}
            line = f"{name:5s} {mname:9s}:"
            for k, v in t.items():
                line += f"  {k} {med[k]:7.1f} ({min(v):.1f}-{max(v):.1f})"
            line += "  | / haze_ex: " + " ".join(f"{med[f'stereo D={D}'] / med['haze_ex']:.2f}" for D in ds)
            say(line)
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
