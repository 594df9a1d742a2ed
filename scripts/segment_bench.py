"""rtdd_segment_surfaces (include/rtdd.h), timed against rtdd_fill_surface selecting ONE of its components.  Both calls synchronise, so a
call's time is the host's clock around it (scripts/wand_bench.py's protocol: medians of 7 rounds of 20 calls, the variants alternating in
one session; the device is drained at the end of every round, so the segmentation's queued paint pass is counted).

The maps are scripts/surface_wand_bench.py's -- (a) a flat band of 1025 rows across the image, (b) a flat disc of radius 0.4 x height, 60
inside and 200 outside -- and (c) the library's own estimate of the dataset's Dog pair, resampled bilinearly to the size.  The wand clicks
the band's left end, the disc's centre, the middle of the Dog map; the segmentation labels everything.  Variants: with the pair, the label
map and the records; the pair alone (no label map, no records); the label map and records alone (no pair: five launches); minPixels 64.
Before anything is timed the region that holds the click is compared with the wand's selection: pixel count, box, and the painted bytes.

The yardstick is the wand's cost for ONE component (profiles/r25_surface_wand.txt).  No threshold is set.

    python scripts/segment_bench.py [--out profiles/r26_segment.txt] [--sizes 1080p,4K]"""
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


def dog_depth():
    """the library's estimate of the Dog pair at its own size (f32, host)"""
    from dataset_util import load_pair
    bgr, ann, _ = load_pair("Dog")
    rows, cols = ann.shape
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(rt.device_image(bgr)); c.pyramid_set_annotation(rt.device_image(ann))
        c.estimate_depth(1000); c.synchronize()
        return c.pyramid_download(rt.IMG_DEPTH, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1080p,4K")
    args = ap.parse_args()
    lines = [f"# rtdd_segment_surfaces (every component) against rtdd_fill_surface (the one under a click), us per call INCLUDING the call's synchronisations and, for the "
             f"segmentation, its queued paint pass: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); host clock; the variants of a row alternate "
             f"within every round; tile {rt.SEGMENT_TILE_W} x {rt.SEGMENT_TILE_H}, {rt.SEGMENT_HEAD} candidates per first read-back"]

    def say(s):
        print(s, flush=True); lines.append(s)

    L = rt.lib()
    dog = torch.from_numpy(dog_depth())[None, None]
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        if name not in args.sizes.split(","):
            continue
        c = rt.Context(0)
        img = lambda t: (C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(0) * t.element_size()))
        none = (None, C.c_size_t(0))
        pairs = [(rt.device_image(np.zeros((rows, cols, 3), np.uint8)), rt.device_image(np.zeros((rows, cols), np.uint8))) for _ in range(2)]
        labels = torch.zeros((rows, cols), dtype=torch.int32, device="cuda:0")
        yy, xx = np.mgrid[:rows, :cols]
        y = rows // 2
        two = lambda mask: np.where(mask, np.float32(60), np.float32(200)).astype(np.float32)
        maps = (("flat band of 1025 rows, clicked at its left end", two((yy >= y - 512) & (yy <= y + 512)), (5, y), 4.0),
                ("flat disc, radius 0.4 x height, clicked at its centre", two(((yy - rows // 2) ** 2 + (xx - cols // 2) ** 2) <= (0.4 * rows) ** 2), (cols // 2, rows // 2), 4.0),
                ("Dog estimate resampled, clicked in the middle", torch.nn.functional.interpolate(dog, (rows, cols), mode="bilinear", align_corners=False)[0, 0].numpy().copy(),
                 (cols // 2, rows // 2), 0.25))
        for what, depth, (sx, sy), step in maps:
            d = rt.device_image(depth)
            dp, dpitch = img(d)
            e0, e1 = (img(p[0]) + img(p[1]) for p in pairs)             # (edited, its pitch, scribble, its pitch) of either call's pair
            wi, si = rt.WandInfo(), rt.SegmentInfo()
            records = (rt.Segment * 255)()

            def segment(min_pixels=1, pair=True, lab=True, rec=True):
                g = rt.Segmentation(step, 0.0, 255.0, min_pixels, 255, 1, 0)
                assert L.rtdd_segment_surfaces(c._h, C.byref(g), *(e1 if pair else none + none), dp, dpitch, *(img(labels) if lab else none), rows, cols,
                                               records if rec else None, C.byref(si)) == 0

            # what the click selects, from the label map; then the wand with that region's code
            for p in pairs:
                p[0].zero_(); p[1].zero_()
            segment(); torch.cuda.synchronize()
            root = int(labels[sy, sx])
            mine = [r for r in records[:si.regions] if r.rootY * cols + r.rootX == root]
            if not mine:                                                # (a click outside the 255 largest components: the largest one's root instead)
                mine, sx, sy = [records[0]], records[0].rootX, records[0].rootY
                root = sy * cols + sx
            mine = mine[0]
            w = rt.SurfaceWand(sx, sy, step, 255.0, 255.0, 0, 0, 0, 0, 0, mine.code, mine.code)

            def wand():
                assert L.rtdd_fill_surface(c._h, C.byref(w), *e0, None, C.c_size_t(0), dp, dpitch, rows, cols, C.byref(wi)) == 0

            wand(); torch.cuda.synchronize()
            assert (wi.pixels, wi.x0, wi.y0, wi.x1, wi.y1) == (mine.pixels, mine.x0, mine.y0, mine.x1, mine.y1), "the wand and the segmentation disagree"
            sel = labels == root
            assert int(sel.sum()) == wi.pixels and torch.equal(pairs[0][1] == 255, sel) and torch.equal(pairs[0][0][sel], pairs[1][0][sel])
            info = (si.components, si.candidates, si.regions, si.pixels)
            segment(64); torch.cuda.synchronize()
            info64 = (si.components, si.candidates, si.regions, si.pixels)
            t = rounds({"wand": wand, "all": segment, "pair": lambda: segment(1, True, False, False), "labels": lambda: segment(1, False, True, True),
                        "min64": lambda: segment(64)})
            ratios = [b / a for a, b in zip(t["wand"], t["all"])]
            say(f"{name:5s} {what}, step {step:g}: rtdd_fill_surface {fmt(t['wand'])} ({wi.passes} passes, {wi.pixels} pixels)  |  rtdd_segment_surfaces pair + labels + records "
                f"{fmt(t['all'])}  |  pair alone {fmt(t['pair'])}  |  labels + records alone {fmt(t['labels'])}  |  minPixels 64 {fmt(t['min64'])}  |  components, candidates, "
                f"regions, pixels {info}, with minPixels 64 {info64}  |  all / wand {np.median(t['all']) / np.median(t['wand']):.2f} (per round {min(ratios):.2f}-{max(ratios):.2f})")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
