"""The parallax view against stereo (include/rtdd.h rtdd_simulate_parallax, rtdd_simulate_stereo) at 1080p, 4K and 8K on a real depth
map (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size), zero parallax at 128:
  horizontal   shiftX = D = 3 % of the width (at most 256), shiftY = 0, dolly = 0: stereo's bytes -- timed in alternating order with
               rtdd_simulate_stereo at the same D and reported as a ratio to it
  mixed        shiftX = D, shiftY = -D / 2
  dolly        no shift, the dolly at its bound (|dolly| * (cols - 1) / 2 = 256)
Microseconds per call, host clock around a device synchronise, the calls alternated over several rounds: the median and the spread.
Per case the share of holes and the mean number of keys a hole's marches look at, from the restatement (tests/parallax_ref.py), which
also checks the bytes of every case once.

    python scripts/parallax_bench.py [--out profiles/r13_parallax.txt] [--no-stats]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt
from parallax_ref import parallax

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


def dolly_bound(rows, cols):
    span = max(cols - 1, rows - 1)
    d = np.float32(512.0 / span)
    if float(d) * span / 2.0 > 256.0:
        d = np.nextafter(d, np.float32(0))
    return float(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-stats", action="store_true", help="leave out the restatement: no hole statistics, no check of the bytes")
    args = ap.parse_args()
    lines = [f"# parallax vs stereo, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); the tiled Dog map, z0 = 128",
             "# holes: share of targets no source lands on; march: mean number of keys a hole's marches read (tests/parallax_ref.py)"]

    def say(s):
        print(s, flush=True); lines.append(s)

    dog = dog_depth()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K")):
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        dh = tile(dog, rows, cols)
        c = rt.Context(0)
        o = rt.device_image(orig); art = rt.device_image(np.zeros_like(orig)); d = rt.device_image(dh)
        D = min(3 * cols // 100, 256)
        views = {"horizontal": (D, 0, 0.0), "mixed": (D, -(D // 2), 0.0), "dolly": (0, 0, dolly_bound(rows, cols))}
        calls = {"stereo": lambda: c.simulate_stereo(o, d, art, rows, cols, D, 128.0, -1, -1, rt.STEREO_VIEW)}
        for k, v in views.items():
            calls[k] = (lambda v=v: c.simulate_parallax(o, d, art, rows, cols, rt.Parallax(v[0], v[1], v[2], 128.0)))
        for f in calls.values():
            for _ in range(3): f()
        t = {k: [] for k in calls}
        for r in range(ROUNDS):
            order = list(calls.items())
            if r % 2: order.reverse()                       # alternating order
            for k, f in order:
                t[k].append(timeit(f))
        med = {k: float(np.median(v)) for k, v in t.items()}
        say(f"{name:5s} D = {D}:  " + "  ".join(f"{k} {med[k]:8.1f} ({min(v):.1f}-{max(v):.1f})" for k, v in t.items()))
        say(f"{name:5s} / stereo:  " + "  ".join(f"{k} {med[k] / med['stereo']:.2f}" for k in views))
        if not args.no_stats:
            for k, v in views.items():
                st = {}
                want = parallax(orig, dh, v[0], v[1], v[2], 128.0, stats=st)
                calls[k](); c.synchronize()
                same = np.array_equal(rt.to_host(art), want)
                say(f"{name:5s} {k:10s} view {v}: holes {100 * st['holes']:.2f} %, march {st['march']:.2f} keys per hole, bytes {'equal' if same else 'DIFFER'}")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
