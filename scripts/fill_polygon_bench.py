"""rtdd_fill_polygon (include/rtdd.h), timed.

1. Fill against a stroke: a rectangle against the ONE horizontal square stroke of radius 1024 that covers the same pixels (a band of 1025
   rows across the image), constant and ramp (the fill's axis is the stroke's segment, so both write the same bytes: checked).
2. A 768-vertex lasso: a wobbly circle whose radius is 0.4 of the image's height, constant, ramp and erase; microseconds per call and per
   million covered pixels, and the share of the launch's tiles without a live edge (counted on the host with tests/polygon_ref.py's
   restated classification).
3. The same number of vertices enclosing next to nothing: a sliver along the image's diagonal, there and one pixel lower back -- the cost
   of the cull when almost every tile of the launch has live edges.
Microseconds per call, host clock around a device synchronise, the variants of a row alternated over the rounds: the median and the spread.

    python scripts/fill_polygon_bench.py [--out profiles/r19_fill_polygon.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import polygon_ref as pr
import realtimedepthdiffusion_amd as rt

ROUNDS, CALLS = 7, 20


def timeit(f, n=CALLS):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6


def fmt(v):
    return f"{float(np.median(v)):7.1f} ({min(v):.1f}-{max(v):.1f})"


def rounds(calls):
    for f in calls.values():
        f(); f()
    t = {k: [] for k in calls}
    for r in range(ROUNDS):
        for k in (list(calls) if r % 2 == 0 else list(calls)[::-1]):
            t[k].append(timeit(calls[k]))
    return t


def sliver(n, rows, cols):
    half = n // 2
    out = [(int(round(i * (cols - 1) / (half - 1))), int(round(i * (rows - 2) / (half - 1)))) for i in range(half)]
    return out + [(x, y + 1) for x, y in out[::-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# rtdd_fill_polygon, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); host clock around a device synchronise; "
             "the variants of a row alternate within every round"]

    def say(s):
        print(s, flush=True); lines.append(s)

    L = rt.lib()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        c = rt.Context(0)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        o = rt.device_image(orig); e = rt.device_image(orig); s = rt.device_image(np.zeros((rows, cols), np.uint8))
        e2 = rt.device_image(orig); s2 = rt.device_image(np.zeros((rows, cols), np.uint8))
        img = lambda t: (C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(0)))
        (ep, epitch), (sp, spitch), (op, opitch) = img(e), img(s), img(o)

        def fill_call(V, fill, ed=None, sc=None):
            xy = (C.c_int * (2 * len(V)))(*[v for p in V for v in p]); f = rt.Fill(*fill); n = len(V)
            e_, ei = img(ed) if ed is not None else (ep, epitch); s_, si = img(sc) if sc is not None else (sp, spitch)

            def call():
                assert L.rtdd_fill_polygon(c._h, xy, n, C.byref(f), e_, ei, s_, si, op, opitch, rows, cols) == 0
            return call

        def covered(V, fill):
            s.zero_(); fill_call(V, (fill[0], 0, 0, 0, 0, 1, 1))(); torch.cuda.synchronize()
            return int((s[:, :cols] == 255).sum().item())

        # 1. a rectangle against the square stroke that covers the same pixels
        y = rows // 2
        rect = [(-612, y - 512), (cols + 612, y - 512), (cols + 612, y + 512), (-612, y + 512)]
        for what, l0, l1 in (("constant", 200, 200), ("ramp", 0, 255)):
            q = (rt.RampStroke * 1)(rt.RampStroke(-100, y, cols + 100, y, 1024, rt.BRUSH_SQUARE, l0, l1))
            p = (rt.Stroke * 1)(rt.Stroke(-100, y, cols + 100, y, 1024, rt.BRUSH_SQUARE, l0))
            e2p, e2i = img(e2); s2p, s2i = img(s2)

            def stroke_call():
                if l0 == l1:
                    assert L.rtdd_paint_strokes(c._h, p, 1, e2p, e2i, s2p, s2i, None, C.c_size_t(0), rows, cols) == 0
                else:
                    assert L.rtdd_paint_ramp_strokes(c._h, q, 1, e2p, e2i, s2p, s2i, None, C.c_size_t(0), rows, cols) == 0
            f = fill_call(rect, (pr.FILL_NONZERO, -100, y, cols + 100, y, l0, l1))
            f(); stroke_call(); torch.cuda.synchronize()
            assert torch.equal(e, e2) and torch.equal(s, s2), "the fill and the stroke should write the same bytes"
            t = rounds({"fill": f, "stroke": stroke_call})
            say(f"{name:5s} rectangle of 1025 rows, {what:8s}  rtdd_fill_polygon {fmt(t['fill'])}  |  the square stroke of radius 1024 {fmt(t['stroke'])}  |  "
                f"fill / stroke {np.median(t['fill']) / np.median(t['stroke']):.2f}")
        # 2. and 3. 768 vertices: a wobbly circle, and a sliver
        shapes = {"wobbly circle, radius 0.4 x height": pr.wobbly_circle(768, cols // 2, rows // 2, 0.4 * rows),
                  "sliver along the diagonal": sliver(768, rows, cols)}
        for what, V in shapes.items():
            assert len(V) == 768
            tiles = pr.tile_classes(V, rows, cols)
            uniform = sum(1 for t_ in tiles if not t_[5])
            px = covered(V, pr.constant(1))
            axis = (cols // 2, rows // 10, cols // 2, 9 * rows // 10)
            t = rounds({"constant": fill_call(V, pr.constant(200)), "ramp": fill_call(V, (pr.FILL_NONZERO, *axis, 20, 240)), "erase": fill_call(V, pr.erase())})
            say(f"{name:5s} 768 vertices, {what:35s} constant {fmt(t['constant'])}  |  ramp {fmt(t['ramp'])}  |  erase {fmt(t['erase'])}  |  {px} pixels covered: "
                f"{np.median(t['constant']) / px * 1e6:.1f} / {np.median(t['ramp']) / px * 1e6:.1f} / {np.median(t['erase']) / px * 1e6:.1f} us per million covered pixels  |  "
                f"{len(tiles)} tiles, {uniform} without a live edge ({100.0 * uniform / len(tiles):.1f} %)")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
