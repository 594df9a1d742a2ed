"""The removed object (include/rtdd.h rtdd_remove_object) against rtdd_composite_layer with its sprite off screen -- the copy of both images
any such call must make: the floor -- on the same images: a random photograph and the library's estimate of the bundled Dog pair tiled to
the size, at 1080p and 4K.  Cases: an empty mask; a disc of radius 0.1 x the height and one of 0.4 x the height (grow 0); the small disc
with grow 8; the small disc with depthOut NULL; rtdd_lift_layer of the whole image's box.  Microseconds per call from HIP events around
CALLS calls on the context's stream, the variants alternated over ROUNDS rounds in one process after a warm-up: the median and the spread
(min-max) of the rounds and the ratio to the floor; the launches per call and the bytes of the table buffer the coarse levels take.  No
ratio is fixed in advance: the profile records what was measured.

    python scripts/remove_bench.py [--out profiles/r23_remove.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from lens_blur_bench import dog_depth, event_us, tile

ROUNDS, CALLS = 7, 20
SIZES = ((1080, 1920, "1080p"), (2160, 3840, "4K"))


def disc(rows, cols, frac):
    yy, xx = np.mgrid[0:rows, 0:cols]
    r = frac * rows
    return ((yy - rows // 2) ** 2 + (xx - cols // 2) ** 2 <= r * r).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import realtimedepthdiffusion_amd as rt
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"# rtdd_remove_object vs rtdd_composite_layer off screen (the floor), random photograph, Dog map tiled, us per call (HIP events around {CALLS} calls): median of {ROUNDS} alternated rounds (min-max)")
    dog = dog_depth(rt)
    for rows, cols, name in SIZES:
        depth = tile(dog, rows, cols)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        plan = rt.remove_plan(rows, cols)
        say(f"{name}: {2 * len(plan) + 1} launches per call, stored levels {[p[1:] for p in plan]}, {sum(16 * r * k for _, r, k in plan)} B of the table buffer")
        c = rt.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        o, d = rt.device_image(orig), rt.device_image(depth)
        art, z = rt.device_image(np.zeros_like(orig)), rt.device_image(np.zeros_like(depth))
        sprite = rt.device_image(np.zeros((rows, cols, 4), np.uint8))
        one = rt.device_image(np.zeros((1, 1, 4), np.uint8))
        masks = {k: rt.device_image(m) for k, m in (("empty", np.zeros((rows, cols), np.uint8)), ("small", disc(rows, cols, 0.1)), ("large", disc(rows, cols, 0.4)))}
        off = rt.Layer(1, 1, -16384, 0, 256, rt.LAYER_NEAREST, 255)
        calls = {"floor: composite off screen": lambda: c.composite_layer(o, d, one, art, z, rows, cols, off),
                 "empty mask": lambda: c.remove_object(o, d, masks["empty"], art, z, rows, cols, rt.Removal(0, 0, 0.0)),
                 "disc 0.1 h": lambda: c.remove_object(o, d, masks["small"], art, z, rows, cols, rt.Removal(0, 0, 0.0)),
                 "disc 0.4 h": lambda: c.remove_object(o, d, masks["large"], art, z, rows, cols, rt.Removal(0, 0, 0.0)),
                 "disc 0.1 h, grow 8": lambda: c.remove_object(o, d, masks["small"], art, z, rows, cols, rt.Removal(0, 8, 0.0)),
                 "disc 0.1 h, no depthOut": lambda: c.remove_object(o, d, masks["small"], art, None, rows, cols, rt.Removal(0, 0, 0.0)),
                 "lift, the image's box": lambda: c.lift_layer(o, masks["large"], rows, cols, 0, 0, 0, sprite, rows, cols)}
        for fn in calls.values():                    # warm-up: code objects, the table buffer
            for _ in range(3): fn()
        t = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                t[k].append(event_us(torch, fn, CALLS))
        med = {k: float(np.median(v)) for k, v in t.items()}
        floor = med["floor: composite off screen"]
        for k, v in t.items():
            say(f"{name:5s} {k:28s} {med[k]:8.1f} ({min(v):.1f}-{max(v):.1f})  | / floor = {med[k] / floor:.2f}")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
