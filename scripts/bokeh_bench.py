"""The occlusion-aware lens blur against the disc gather (include/rtdd.h rtdd_simulate_bokeh, rtdd_simulate_lens_blur RTDD_APERTURE_DISC)
with the same window scale K, on the library's estimate of the bundled Dog pair tiled to the size, focus at the map's median: 1080p with
K = 55 and 27, 4K with K = 110 and 55.  Microseconds per call from HIP events around CALLS calls on the context's stream, disc and bokeh
alternated over ROUNDS rounds in one process after a warm-up: the median and the spread (min-max) of the rounds, the ratio to the disc,
and the samples per second -- a sample is one (source, target) pair of the window the kernel walks, pi / 4 * (largest |s| of a tile)^2 of
them per pixel, counted here from the map as the kernel bounds it (per 64 x 16 tile with its halo of K / 2).

    python scripts/bokeh_bench.py [--out profiles/r16_bokeh.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from lens_blur_bench import dog_depth, event_us, tile

ROUNDS, CALLS = 7, 20
CASES = ((1080, 1920, "1080p", (55, 27)), (2160, 3840, "4K", (110, 55)))


def aperture_for(rows, cols, K):
    a = (K + 0.5) / float(np.sqrt(np.float32(rows * rows + cols * cols)))
    assert int(a * float(np.sqrt(np.float32(rows * rows + cols * cols)))) == K
    return a


def samples_walked(depth, f, K):
    """The (source, target) pairs k_bokeh's window loop visits: per tile of 64 x 16 the disc of the largest |s| within the tile and its
    halo of K / 2, for each of the tile's pixels inside the image."""
    from bokeh_ref import signed_coc
    from lens_blur_ref import disc_points
    k = np.abs(signed_coc(depth, f, K))
    rows, cols = k.shape
    h = K // 2
    n = {kk: disc_points(kk) for kk in range(K + 1)}
    total = 0
    for y0 in range(0, rows, 16):
        for x0 in range(0, cols, 64):
            hw = int(k[max(y0 - h, 0):y0 + 16 + h, max(x0 - h, 0):x0 + 64 + h].max())
            if hw > 1:
                total += n[hw] * (min(y0 + 16, rows) - y0) * (min(x0 + 64, cols) - x0)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import realtimedepthdiffusion_amd as rt
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"# bokeh vs disc gather, Dog map tiled, focus at the map's median, us per call (HIP events around {CALLS} calls): median of {ROUNDS} alternated rounds (min-max)")
    dog = dog_depth(rt)
    for rows, cols, name, Ks in CASES:
        depth = tile(dog, rows, cols)
        f = float(np.median(depth))
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        c = rt.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        o, d, art = rt.device_image(orig), rt.device_image(depth), rt.device_image(np.zeros_like(orig))
        for K in Ks:
            a = aperture_for(rows, cols, K)
            calls = {"disc": lambda: c.simulate_lens_blur(o, d, art, rows, cols, a, f, -1, -1, rt.APERTURE_DISC),
                     "bokeh": lambda: c.simulate_bokeh(o, d, art, rows, cols, a, f, -1, -1)}
            for fn in calls.values():                # warm-up: code objects, the table's allocation
                for _ in range(3): fn()
            t = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, fn in calls.items():
                    t[k].append(event_us(torch, fn, CALLS))
            med = {k: float(np.median(v)) for k, v in t.items()}
            n = samples_walked(depth, f, K)
            line = f"{name:5s} K={K:3d}:"
            for k, v in t.items():
                line += f"  {k} {med[k]:9.1f} ({min(v):.1f}-{max(v):.1f})"
            say(line + f"  | bokeh / disc = {med['bokeh'] / med['disc']:.1f}  | {n / 1e9:.2f} G samples per call, {n / med['bokeh'] / 1e6:.2f} T samples/s")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
