"""The composited layer (include/rtdd.h rtdd_composite_layer) against rtdd_simulate_haze_ex -- the library's plain streaming effect, 3 B + 4 B
read and 3 B written per pixel -- on the same images: a random photograph and the library's estimate of the bundled Dog pair tiled to the
size, at 1080p and 4K.  The layer's depth is a plane from 60 at the left edge to 200 at the right, feather 8, so it wins and loses all over
the footprint; depthOut is written (3 B + 4 B more per pixel than the haze).  Cases: no sprite on screen (the copy path alone); a 512 x 512
sprite at scale 256 with each filter; the same sprite at scale 1024 (2048 x 2048 pixels: most of the frame) with each filter.
Microseconds per call from HIP events around CALLS calls on the context's stream, the variants alternated over ROUNDS rounds in one process
after a warm-up: the median and the spread (min-max) of the rounds, the ratio to the haze, and the bytes moved per second counting 14 B
per pixel (the sprite's texels not counted).  No ratio is fixed in advance: the profile records what was measured.

    python scripts/composite_bench.py [--out profiles/r22_composite.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import realtimedepthdiffusion_amd as rt
    from composite_ref import random_sprite
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"# rtdd_composite_layer vs rtdd_simulate_haze_ex, random photograph, Dog map tiled, us per call (HIP events around {CALLS} calls): median of {ROUNDS} alternated rounds (min-max)")
    dog = dog_depth(rt)
    sprite = random_sprite(512, 512, 1, "ramp")
    for rows, cols, name in SIZES:
        depth = tile(dog, rows, cols)
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        c = rt.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        o, d, s = rt.device_image(orig), rt.device_image(depth), rt.device_image(sprite)
        art, z = rt.device_image(np.zeros_like(orig)), rt.device_image(np.zeros_like(depth))

        def layer(x, y, scale, filt):
            return rt.Layer(512, 512, x, y, scale, filt, 255, 0, 0, cols, 0, 60.0, 200.0, 8.0)

        layers = {"off screen": layer(-16384, 0, 256, rt.LAYER_NEAREST),
                  "512^2 x1 nearest": layer(cols // 3, rows // 4, 256, rt.LAYER_NEAREST), "512^2 x1 bilinear": layer(cols // 3, rows // 4, 256, rt.LAYER_BILINEAR),
                  "512^2 x4 nearest": layer(-60, -500, 1024, rt.LAYER_NEAREST), "512^2 x4 bilinear": layer(-60, -500, 1024, rt.LAYER_BILINEAR)}
        calls = {"haze_ex": lambda: c.simulate_haze_ex(o, d, art, rows, cols, 3.0, (200, 180, 160))}
        for k, L in layers.items():
            calls[k] = lambda L=L: c.composite_layer(o, d, s, art, z, rows, cols, L)
        for fn in calls.values():                    # warm-up: code objects
            for _ in range(3): fn()
        t = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                t[k].append(event_us(torch, fn, CALLS))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, v in t.items():
            bytes_moved = rows * cols * (10 if k == "haze_ex" else 14)
            say(f"{name:5s} {k:18s} {med[k]:8.1f} ({min(v):.1f}-{max(v):.1f})  | / haze_ex = {med[k] / med['haze_ex']:.2f}  | {bytes_moved / med[k] / 1e6:.2f} TB/s")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
