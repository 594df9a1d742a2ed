"""rtdd_fill_surface (include/rtdd.h), timed against rtdd_fill_similar selecting the SAME pixels.  Both calls synchronise, so a call's time
is the host's clock around it (scripts/wand_bench.py's protocol: medians of 7 rounds of 20 calls, the variants alternating in one session).

The image of the colour wand is tests/wand_ref.py from_mask(mask); the depth map of the surface wand is 60 inside the mask and 200 outside.
(a) A flat band of 1025 rows across the image, clicked at its left end: the selection travels the image's width.
(b) A flat disc of radius 0.4 x height, clicked at its centre.
Each also with the global flag of either call (no grow pass).  Both outputs are compared byte for byte before anything is timed.

From the code the two calls run the same number of passes; the links pass reads 4 bytes per pixel where the mask pass reads 3 and writes
three planes where it writes two; a grow pass loads three words per row where the wand's loads two.  No threshold is set on the ratio.

    python scripts/surface_wand_bench.py [--out profiles/r25_surface_wand.txt] [--sizes 1080p,4K]"""
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

import realtimedepthdiffusion_amd as rt
import wand_ref as wr

ROUNDS, CALLS = 7, 20


def timeit(f, n=CALLS):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6


def fmt(v):
    return f"{float(np.median(v)):8.1f} ({min(v):.1f}-{max(v):.1f})"


def rounds(calls):
    for f in calls.values():
        f(); f()
    t = {k: [] for k in calls}
    for r in range(ROUNDS):
        for k in (list(calls) if r % 2 == 0 else list(calls)[::-1]):
            t[k].append(timeit(calls[k]))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1080p,4K")
    args = ap.parse_args()
    lines = [f"# rtdd_fill_surface against rtdd_fill_similar on the same selection, us per call INCLUDING the call's synchronisations: median of {ROUNDS} rounds of "
             f"{CALLS} calls each (min-max of the rounds); host clock; the variants of a row alternate within every round; a round of the host loop is "
             f"{rt.WAND_ROUND} passes"]

    def say(s):
        print(s, flush=True); lines.append(s)

    L = rt.lib()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        if name not in args.sizes.split(","):
            continue
        c = rt.Context(0)
        img = lambda t: (C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(0) * t.element_size()))
        pairs = [(rt.device_image(np.zeros((rows, cols, 3), np.uint8)), rt.device_image(np.zeros((rows, cols), np.uint8))) for _ in range(2)]
        yy, xx = np.mgrid[:rows, :cols]
        y = rows // 2
        shapes = (("flat band of 1025 rows, clicked at its left end", (yy >= y - 512) & (yy <= y + 512), (5, y)),
                  ("flat disc, radius 0.4 x height, clicked at its centre", ((yy - rows // 2) ** 2 + (xx - cols // 2) ** 2) <= (0.4 * rows) ** 2, (cols // 2, rows // 2)))
        for what, mask, (sx, sy) in shapes:
            o = rt.device_image(wr.from_mask(mask)); d = rt.device_image(np.where(mask, np.float32(60), np.float32(200)).astype(np.float32))
            (op, opitch), (dp, dpitch) = img(o), img(d)
            axis = (cols // 2, 0, cols // 2, rows - 1, 20, 240)
            for kind, wflags, sflags in (("connected", 0, 0), ("global", rt.WAND_GLOBAL, rt.SURFACE_GLOBAL)):
                w = rt.Wand(sx, sy, 5, wflags, *axis); s = rt.SurfaceWand(sx, sy, 4.0, 30.0, 30.0, sflags, *axis)      # (the band keeps the 200 outside out of the global selection)
                wi, si = rt.WandInfo(), rt.WandInfo()
                e0, e1 = (img(p[0]) + img(p[1]) for p in pairs)         # (edited, its pitch, scribble, its pitch) of either call's pair

                def similar():
                    assert L.rtdd_fill_similar(c._h, C.byref(w), *e0, op, opitch, rows, cols, C.byref(wi)) == 0

                def surface():
                    assert L.rtdd_fill_surface(c._h, C.byref(s), *e1, None, C.c_size_t(0), dp, dpitch, rows, cols, C.byref(si)) == 0

                for p in pairs:
                    p[0].zero_(); p[1].zero_()
                similar(); surface(); torch.cuda.synchronize()
                assert torch.equal(pairs[0][0], pairs[1][0]) and torch.equal(pairs[0][1], pairs[1][1]), "the two wands should write the same bytes"
                assert wi.pixels == si.pixels == int(mask.sum()) and (wi.x0, wi.y0, wi.x1, wi.y1) == (si.x0, si.y0, si.x1, si.y1)
                t = rounds({"similar": similar, "surface": surface})
                ratios = [b / a for a, b in zip(t["similar"], t["surface"])]
                say(f"{name:5s} {what}, {kind}: rtdd_fill_similar {fmt(t['similar'])} ({wi.passes} passes)  |  rtdd_fill_surface {fmt(t['surface'])} ({si.passes} passes)  |  "
                    f"{si.pixels} pixels  |  surface / similar {np.median(t['surface']) / np.median(t['similar']):.2f} (per round {min(ratios):.2f}-{max(ratios):.2f})")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
