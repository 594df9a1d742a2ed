"""rtdd_fill_similar (include/rtdd.h), timed.  The call synchronises, so a call's time is the host's clock around it.

(a) A flat rectangle across the image (a band of 1025 rows) against the rtdd_fill_polygon call that writes the same bytes (checked first;
    the polygon call is asynchronous: its time is the host clock around 20 calls and one synchronise).
(b) A flat disc of radius 0.4 x height, clicked in its centre.
(c) A click in the sky of a dataset photograph tiled to the size, tolerance 12, 4- and 8-connected.
(d) RTDD_WAND_GLOBAL on (c): no grow pass at all -- the mask, the paint and the one synchronisation.
For each: the passes the call reports, and (time - time of (d)'s kind of call on the same image) / passes as the time per pass.
Microseconds per call, the variants of a row alternated over the rounds: the median and the spread.

    python scripts/wand_bench.py [--out profiles/r20_wand.txt] [--label TEXT] [--append]

The round length (csrc/fill_similar.hip: kWandRound) is a constant; its alternatives were measured with libraries built from a copy of
that file with another value (scripts/build_variant.sh's recipe), selected with RTDD_LIBRARY, one run of this script each (--label, --append)."""
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
from dataset_util import load_pair

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
    ap.add_argument("--label", default="")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--sizes", default="1080p,4K")
    args = ap.parse_args()
    lines = [f"# rtdd_fill_similar{' [' + args.label + ']' if args.label else ''}, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); host clock; "
             f"the variants of a row alternate within every round; a round of the host loop is {rt.WAND_ROUND} passes unless the label says otherwise"]

    def say(s):
        print(s, flush=True); lines.append(s)

    L = rt.lib()
    photo = load_pair("Dog")[0]
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        if name not in args.sizes.split(","):
            continue
        c = rt.Context(0)
        img = lambda t: (C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(0)))
        blank = np.zeros((rows, cols, 3), np.uint8)
        e = rt.device_image(blank); s = rt.device_image(np.zeros((rows, cols), np.uint8))
        e2 = rt.device_image(blank); s2 = rt.device_image(np.zeros((rows, cols), np.uint8))
        (ep, epitch), (sp, spitch) = img(e), img(s)

        def wand_call(o, wand, info=None):
            w = rt.Wand(*wand); op, opitch = img(o); out = info if info is not None else rt.WandInfo()

            def call():
                assert L.rtdd_fill_similar(c._h, C.byref(w), ep, epitch, sp, spitch, op, opitch, rows, cols, C.byref(out)) == 0
            return call

        def row(what, o, seed, tol, label=(200, 200), flags_list=((0, "4-connected"), (rt.WAND_CONNECT_8, "8-connected"))):
            x, y = seed
            infos = {k: rt.WandInfo() for _, k in flags_list}
            calls = {k: wand_call(o, (x, y, tol, f, cols // 2, 0, cols // 2, rows - 1, *label), infos[k]) for f, k in flags_list}
            calls["global"] = wand_call(o, (x, y, tol, rt.WAND_GLOBAL, cols // 2, 0, cols // 2, rows - 1, *label))
            t = rounds(calls)
            base = float(np.median(t["global"]))
            for _, k in flags_list:
                i = infos[k]; m = float(np.median(t[k]))
                say(f"{name:5s} {what:38s} {k}: {fmt(t[k])}  |  {i.pixels} pixels, box {i.x0},{i.y0}..{i.x1},{i.y1}  |  {i.passes} passes, "
                    f"{(m - base) / max(i.passes, 1):.1f} us per pass over the global call's {base:.1f}")
            say(f"{name:5s} {what:38s} RTDD_WAND_GLOBAL (no grow pass): {fmt(t['global'])}")
            return t

        # (a) a flat band across the image against the polygon that writes the same bytes
        y = rows // 2
        band = np.full((rows, cols, 3), 40, np.uint8); band[y - 512:y + 513] = (90, 100, 110)
        o = rt.device_image(band); op, opitch = img(o)
        rect = [(-612, y - 512), (cols + 612, y - 512), (cols + 612, y + 512), (-612, y + 512)]
        for what, l0, l1 in (("constant", 200, 200), ("ramp", 0, 255)):
            fill = rt.Fill(pr.FILL_NONZERO, -100, y, cols + 100, y, l0, l1)
            xy = (C.c_int * 8)(*[v for p in rect for v in p]); e2p, e2i = img(e2); s2p, s2i = img(s2)

            def polygon_call():
                assert L.rtdd_fill_polygon(c._h, xy, 4, C.byref(fill), e2p, e2i, s2p, s2i, op, opitch, rows, cols) == 0
            info = rt.WandInfo()
            w = wand_call(o, (5, y, 0, 0, -100, y, cols + 100, y, l0, l1), info)
            e.zero_(); s.zero_(); e2.zero_(); s2.zero_()
            w(); polygon_call(); torch.cuda.synchronize()
            assert torch.equal(e, e2) and torch.equal(s, s2), "the wand and the polygon should write the same bytes"
            t = rounds({"wand": w, "polygon": polygon_call})
            say(f"{name:5s} (a) flat band of 1025 rows, {what:8s}  rtdd_fill_similar {fmt(t['wand'])} ({info.passes} passes, {info.pixels} pixels)  |  "
                f"the rtdd_fill_polygon that writes the same bytes {fmt(t['polygon'])}  |  wand / polygon {np.median(t['wand']) / np.median(t['polygon']):.1f}")
        row("(a) the same band, clicked at its left end", o, (5, y), 0)
        # (b) a flat disc
        yy, xx = np.mgrid[:rows, :cols]
        disc = np.where((((yy - rows // 2) ** 2 + (xx - cols // 2) ** 2) <= (0.4 * rows) ** 2)[..., None], np.uint8(120), np.uint8(30)).repeat(3, -1)
        row("(b) flat disc, radius 0.4 x height", rt.device_image(disc), (cols // 2, rows // 2), 0)
        # (c), (d) the sky of a photograph tiled to the size
        ph, pw = photo.shape[:2]
        tiled = np.ascontiguousarray(np.tile(photo, ((rows + ph - 1) // ph, (cols + pw - 1) // pw, 1))[:rows, :cols])
        row("(c) sky of the tiled Dog photograph, tolerance 12; (d)", rt.device_image(tiled), (pw // 2, ph // 12), 12, label=(20, 240))
        c.close()
    if args.out:
        with open(args.out, "a" if args.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
