"""The mask refinement (include/rtdd.h rtdd_mask_distance, rtdd_refine_mask) at 1080p and 4K against two calls measured in the same
session: rtdd_lift_layer of the whole image's box -- one pass over the bytes: the floor -- and rtdd_remove_object with grow = 8 on the
same mask, the only other call that widens a selection.  Masks: a disc of radius 0.1 x and one of 0.4 x the height; the code plane
rtdd_segment_surfaces paints for the library's estimate of the bundled Dog pair tiled to the size, read under the code of the region
whose size is nearest a tenth of the image (the largest region is nearly all of it: no object selection); the empty
and the full mask.  Reaches 8, 64 and 1024: the distance at that reach, grow / shrink / outline at its square, the feather lo = 0.5 -
reach, hi = 0.  Microseconds per call from HIP events around CALLS calls on the context's stream, the variants alternated over ROUNDS rounds
in one process after a warm-up: the median and the spread (min-max) of the rounds, and the ratios to the floor and to the removal.  No
ratio is fixed in advance: the profile records what was measured.

    python scripts/mask_distance_bench.py [--out profiles/r27_mask_distance.txt] [--sizes 1080p,4K] [--reaches 8,64,1024] [--masks empty,full]

(the last three narrow the run, e.g. to one mask at one reach under `rocprofv3 --kernel-trace --stats --output-format csv`: which pass a
case spends its time in -- the second section of the profile)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from lens_blur_bench import dog_depth, event_us, tile
from remove_bench import disc

ROUNDS, CALLS = 7, 20
SIZES = {"1080p": (1080, 1920), "4K": (2160, 3840)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1080p,4K")
    ap.add_argument("--reaches", default="8,64,1024")
    ap.add_argument("--masks", default=None, help="a comma-separated subset of the masks' names, '_' for a space (default: all)")
    args = ap.parse_args()
    import torch
    import realtimedepthdiffusion_amd as rt
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"# rtdd_mask_distance / rtdd_refine_mask, us per call (HIP events around {CALLS} calls): median of {ROUNDS} alternated rounds (min-max) "
        "| ratio to rtdd_lift_layer of the image's box (the floor) | ratio to rtdd_remove_object, grow 8, on the same mask")
    dog = dog_depth(rt)
    reaches = [int(v) for v in args.reaches.split(",")]
    for name in args.sizes.split(","):
        rows, cols = SIZES[name]
        depth = tile(dog, rows, cols)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        c = rt.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        o, d = rt.device_image(orig), rt.device_image(depth)
        art, z = rt.device_image(np.zeros_like(orig)), rt.device_image(np.zeros_like(depth))
        sprite = rt.device_image(np.zeros((rows, cols, 4), np.uint8))
        out, d2 = rt.device_image(np.zeros((rows, cols), np.uint8)), rt.device_image(np.zeros((rows, cols), np.int32))
        ed, scr = rt.device_image(np.zeros((rows, cols, 3), np.uint8)), rt.device_image(np.zeros((rows, cols), np.uint8))
        info, segs = c.segment_surfaces((2.0, 0.0, 255.0, 64, 8, 1, 0), ed, scr, rows, cols, d)
        codes = np.where(rt.to_host(scr) == 255, rt.to_host(ed)[..., 0], 0).astype(np.uint8)
        pick = min(segs, key=lambda q: abs(q.pixels - rows * cols // 10))      # a mid-sized region: an object, not the background
        masks = {"disc 0.1 h": (disc(rows, cols, 0.1), 0), "disc 0.4 h": (disc(rows, cols, 0.4), 0), "segment codes": (codes, pick.code),
                 "empty": (np.zeros((rows, cols), np.uint8), 0), "full": (np.ones((rows, cols), np.uint8), 0)}
        say(f"{name}: {rt.mask_distance_plan(rows, cols, 8)['words'] * 4} B of the table buffer; segment codes: {info.regions} regions of {[q.pixels for q in segs]} pixels, region {pick.code} selected ({int((codes == pick.code).sum())} pixels)")
        wanted = [v.replace("_", " ") for v in args.masks.split(",")] if args.masks else list(masks)
        for mname, (m, select) in ((k, masks[k]) for k in wanted):
            mi = rt.device_image(m)
            calls = {"floor: lift, the image's box": lambda: c.lift_layer(o, mi, rows, cols, select, 0, 0, sprite, rows, cols),
                     "remove, grow 8": lambda: c.remove_object(o, d, mi, art, z, rows, cols, rt.Removal(select, 8, 0.0))}
            for r in reaches:
                r2 = r * r
                calls[f"distance, reach {r}"] = lambda r=r: c.mask_distance(mi, rows, cols, select, r, d2)
                calls[f"grow, outer2 {r2}"] = lambda r2=r2: c.refine_mask(mi, rows, cols, rt.MaskRefine(select, rt.REFINE_GROW, 0, r2), out)
                calls[f"shrink, inner2 {r2}"] = lambda r2=r2: c.refine_mask(mi, rows, cols, rt.MaskRefine(select, rt.REFINE_SHRINK, r2, 0), out)
                calls[f"outline, {r2} both sides"] = lambda r2=r2: c.refine_mask(mi, rows, cols, rt.MaskRefine(select, rt.REFINE_OUTLINE, r2, r2), out)
                calls[f"feather, {r - 0.5} px inwards"] = lambda r=r: c.refine_mask(mi, rows, cols, rt.MaskRefine(select, rt.REFINE_FEATHER, 0, 0, 0.5 - r, 0.0), out)
            for fn in calls.values():                    # warm-up: code objects, the table buffer
                for _ in range(2): fn()
            t = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, fn in calls.items():
                    t[k].append(event_us(torch, fn, CALLS))
            med = {k: float(np.median(v)) for k, v in t.items()}
            floor, removal = med["floor: lift, the image's box"], med["remove, grow 8"]
            for k, v in t.items():
                say(f"{name:5s} {mname:14s} {k:30s} {med[k]:9.1f} ({min(v):.1f}-{max(v):.1f})  | / floor = {med[k] / floor:6.2f} | / remove = {med[k] / removal:5.2f}")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
