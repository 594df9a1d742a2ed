"""Brush strokes and the annotation rebuild (include/rtdd.h rtdd_paint_strokes, rtdd_pyramid_annotation_rebuild), timed.

1. A 300-segment round polyline of radius 21 across a 1080p and a 4K image: ONE rtdd_paint_strokes call against the rtdd_paint_image
   stamps, one call each, that leave no gap along the same polyline (one per pixel step of each segment's longer axis), and against one
   rtdd_paint_image call (the floor a launch has).
2. The first estimate after a change at 1080p: a stamp + estimate with the accumulating annotation kernel (what every build before this
   one ran: those kernels are unchanged), the same with rtdd_pyramid_annotation_rebuild in front, and an estimate with no change.
Microseconds per call, host clock around a device synchronise, the variants alternated over several rounds: the median and the spread.

    python scripts/strokes_bench.py [--out profiles/r09_strokes.txt]"""
import argparse
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt
from realtimedepthdiffusion_amd.synth import make_problem

ROUNDS, CALLS = 9, 10


def timeit(f, n=CALLS):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6


def polyline(rows, cols, n=300):
    return [(int(cols * (0.05 + 0.9 * i / n)), int(rows * (0.5 + 0.35 * math.sin(i / 9.0)))) for i in range(n + 1)]


def stamps_along(line):
    out = []
    for (x0, y0), (x1, y1) in zip(line[:-1], line[1:]):
        k = max(abs(x1 - x0), abs(y1 - y0), 1)
        for i in range(k + 1):
            p = (x0 + (x1 - x0) * i // k, y0 + (y1 - y0) * i // k)
            if not out or out[-1] != p:
                out.append(p)
    return out


def fmt(v):
    return f"{float(np.median(v)):9.1f} ({min(v):.1f}-{max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# brush strokes, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); host clock around a device synchronise"]

    def say(s):
        print(s, flush=True); lines.append(s)

    L = rt.lib()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        c = rt.Context(0)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        e = rt.device_image(orig); s = rt.device_image(np.zeros((rows, cols), np.uint8))
        ep, epitch = C.c_void_p(e.data_ptr()), C.c_size_t(e.stride(0)); sp, spitch = C.c_void_p(s.data_ptr()), C.c_size_t(s.stride(0))
        line = polyline(rows, cols)
        arr = (rt.Stroke * 300)(*[rt.Stroke(a[0], a[1], b[0], b[1], 21, rt.BRUSH_ROUND, 200) for a, b in zip(line[:-1], line[1:])])
        stamps = stamps_along(line)

        def strokes():
            assert L.rtdd_paint_strokes(c._h, arr, 300, ep, epitch, sp, spitch, None, C.c_size_t(0), rows, cols) == 0

        def all_stamps():
            for x, y in stamps:
                L.rtdd_paint_image(c._h, x, y, 200, 21, ep, epitch, sp, spitch, rows, cols)

        def one_stamp():
            L.rtdd_paint_image(c._h, cols // 2, rows // 2, 200, 21, ep, epitch, sp, spitch, rows, cols)
        calls = {"strokes": (strokes, CALLS), "stamps": (all_stamps, 2), "one stamp": (one_stamp, 50)}
        for f, _ in calls.values():
            f(); f()
        t = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, (f, n) in calls.items():
                t[k].append(timeit(f, n))
        m = {k: float(np.median(v)) for k, v in t.items()}
        say(f"{name:5s} 300 round segments, radius 21: one rtdd_paint_strokes call {fmt(t['strokes'])}  |  the {len(stamps)} rtdd_paint_image stamps that leave no gap "
            f"{fmt(t['stamps'])}  |  one rtdd_paint_image call {fmt(t['one stamp'])}  |  stamps / strokes {m['stamps'] / m['strokes']:.1f}, strokes / one stamp {m['strokes'] / m['one stamp']:.2f}")
        c.close()

    rows, cols = 1080, 1920
    p = make_problem(rows, cols, seed=1234)
    bgr = np.repeat(p["gray"][..., None], 3, -1)
    ann = np.where(p["mask"] == 255, p["edited"][..., 0], 32).astype(np.uint8)
    c = rt.Context(0)
    c.GPULoadWeights(0.4); c.pyramid_create(rows, cols)
    c.pyramid_set_image(rt.device_image(bgr)); c.pyramid_set_annotation(rt.device_image(ann))
    sptr = c.pyramid_image(rt.IMG_SCRIBBLE, 0); eptr = c.pyramid_image(rt.IMG_EDITED, 0)
    stamp = lambda: c.GPUPaintImage(700, 500, 128, 21, (eptr[0], eptr[1]), (sptr[0], sptr[1]), rows, cols)

    def accumulate():
        stamp(); c.estimate_depth(1000)

    def rebuild():
        stamp(); c.pyramid_annotation_rebuild(); c.estimate_depth(1000)

    def unchanged():
        c.estimate_depth(1000)
    calls = {"stamp + estimate (accumulate)": accumulate, "stamp + rebuild + estimate": rebuild, "estimate, nothing changed": unchanged}
    for f in calls.values():
        for _ in range(5): f()
    c.synchronize()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            t[k].append(timeit(f))
    for k, v in t.items():
        say(f"1080p {k:32s} {fmt(v)}")
    a, r = float(np.median(t["stamp + estimate (accumulate)"])), float(np.median(t["stamp + rebuild + estimate"]))
    sa = t["stamp + estimate (accumulate)"]
    say(f"1080p rebuild - accumulate: {r - a:+.1f} us; run-to-run spread of the accumulating figure {max(sa) - min(sa):.1f} us")
    c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
