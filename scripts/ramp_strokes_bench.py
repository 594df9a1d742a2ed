"""Depth-ramp strokes (include/rtdd.h rtdd_paint_ramp_strokes, rtdd_ramp_polyline), timed against the constant-label call.

1. The same geometry through both calls: scripts/strokes_bench.py's 300-segment round polyline of radius 21 across a 1080p and a 4K
   image, through rtdd_paint_ramp_strokes with the labels rtdd_ramp_polyline spreads from 20 to 240 along it, and through
   rtdd_paint_strokes with one label.
2. A floor: ONE square stroke of radius 1024 across the image.  Every covered pixel evaluates the label rule, so this is the ramp's worst
   ratio to the constant call.
3. With --parent LIB (a librtdd.so built from the parent commit): rtdd_paint_strokes of that library on the same polyline in the same
   session (the constant-label kernel's code is meant to be what it was: a confirmation).
Microseconds per call, host clock around a device synchronise, the variants alternated over the rounds: the median and the spread.

    python scripts/ramp_strokes_bench.py [--parent path/to/parent/librtdd.so] [--out profiles/r18_ramp_strokes.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt
from strokes_bench import polyline

ROUNDS, CALLS = 7, 20


def timeit(f, n=CALLS):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6


def fmt(v):
    return f"{float(np.median(v)):8.1f} ({min(v):.1f}-{max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a librtdd.so built from the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# depth-ramp strokes, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); host clock around a device synchronise; "
             "the variants of a row alternate within every round"]

    def say(s):
        print(s, flush=True); lines.append(s)

    L = rt.lib()
    parent = pctx = None
    if args.parent:
        parent = C.CDLL(os.path.abspath(args.parent))
        pctx = C.c_void_p()
        assert parent.rtdd_ctx_create(C.c_int(0), C.byref(pctx)) == 0
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        c = rt.Context(0)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        e = rt.device_image(orig); s = rt.device_image(np.zeros((rows, cols), np.uint8))
        ep, epitch = C.c_void_p(e.data_ptr()), C.c_size_t(e.stride(0)); sp, spitch = C.c_void_p(s.data_ptr()), C.c_size_t(s.stride(0))
        line = polyline(rows, cols)
        ramp = rt.ramp_polyline(line, 21, rt.BRUSH_ROUND, 20, 240)
        assert len(ramp) == 300 and ramp[0][6] == 20 and ramp[-1][7] == 240
        geometry = {
            "300 round segments, radius 21": (ramp, [q[:6] + (200,) for q in ramp]),
            "one square stroke, radius 1024": ([(-100, rows // 3, cols + 100, 2 * rows // 3, 1024, rt.BRUSH_SQUARE, 0, 255)],
                                               [(-100, rows // 3, cols + 100, 2 * rows // 3, 1024, rt.BRUSH_SQUARE, 200)]),
        }
        for what, (ramps, plain) in geometry.items():
            n = len(ramps)
            rarr = (rt.RampStroke * n)(*[rt.RampStroke(*q) for q in ramps])
            parr = (rt.Stroke * n)(*[rt.Stroke(*q) for q in plain])

            def ramp_call():
                assert L.rtdd_paint_ramp_strokes(c._h, rarr, n, ep, epitch, sp, spitch, None, C.c_size_t(0), rows, cols) == 0

            def plain_call():
                assert L.rtdd_paint_strokes(c._h, parr, n, ep, epitch, sp, spitch, None, C.c_size_t(0), rows, cols) == 0

            def parent_call():
                assert parent.rtdd_paint_strokes(pctx, parr, n, ep, epitch, sp, spitch, None, C.c_size_t(0), rows, cols) == 0
            calls = {"ramp": ramp_call, "constant": plain_call}
            if parent is not None:
                calls["parent"] = parent_call
            for f in calls.values():
                f(); f()
            t = {k: [] for k in calls}
            for r in range(ROUNDS):
                order = list(calls) if r % 2 == 0 else list(calls)[::-1]
                for k in order:
                    t[k].append(timeit(calls[k]))
            m = {k: float(np.median(v)) for k, v in t.items()}
            row = (f"{name:5s} {what:31s} rtdd_paint_ramp_strokes {fmt(t['ramp'])}  |  rtdd_paint_strokes {fmt(t['constant'])}  |  ramp / constant {m['ramp'] / m['constant']:.2f}")
            if parent is not None:
                inside = min(t["parent"]) <= m["constant"] <= max(t["parent"])
                row += f"  |  the parent commit's rtdd_paint_strokes {fmt(t['parent'])}: this commit's median {'inside' if inside else 'OUTSIDE'} its min-max"
            say(row)
        c.close()
    if parent is not None:
        parent.rtdd_ctx_destroy(pctx)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
