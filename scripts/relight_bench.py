"""Relight against haze_ex (include/rtdd.h rtdd_simulate_relight, rtdd_simulate_haze_ex) at 1080p, 4K and 8K, in one process: a smooth
depth map and a real one (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size); a directional light
and a point light anchored at the centre pixel.  haze_ex is the streaming effect that moves the same 10 B/px.
Microseconds per call, host clock around a device synchronise, the calls alternated over several rounds: the median and the spread.

    python scripts/relight_bench.py [--out profiles/r11_relight.txt]"""
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
    lines = [f"# relight vs haze_ex, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); relief 2, ambient 0.25, diffuse 1"]

    def say(s):
        print(s, flush=True); lines.append(s)

    dog = dog_depth()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K")):
        yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
        smooth = (127.5 + 120 * np.sin(xx / 301.0) * np.cos(yy / 207.0)).astype(np.float32)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        c = rt.Context(0)
        o = rt.device_image(orig); art = rt.device_image(np.zeros_like(orig))
        directional = rt.Light(rt.LIGHT_DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.25, diffuse=1)
        point = rt.Light(rt.LIGHT_POINT, cols * 0.4, rows * 0.3, 100, anchorX=cols // 2, anchorY=rows // 2, radius=cols / 4, relief=2, ambient=0.25,
                         diffuse=1)
        for mname, dh in (("smooth", smooth), ("Dog tiled", tile(dog, rows, cols))):
            d = rt.device_image(dh)
            calls = {"haze_ex": lambda: c.simulate_haze_ex(o, d, art, rows, cols, 2.0, (255, 255, 255)),
                     "relight directional": lambda: c.simulate_relight(o, d, art, rows, cols, directional),
                     "relight point": lambda: c.simulate_relight(o, d, art, rows, cols, point)}
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
            line += "  | / haze_ex: " + " ".join(f"{med[k] / med['haze_ex']:.2f}" for k in ("relight directional", "relight point"))
            say(line)
        c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
