"""The colour guide's cost (include/rtdd.h rtdd_solve_guided, rtdd_pyramid_set_guide), in one process:

  * the prepare pass alone at 1080p, 4K and 8K -- a solve of 0 sweeps, the device time between the events in front of and behind its
    prepare launch (rtdd_profile.prepare_ms) -- for a gray and a BGR guide, each in an aligned allocation (the four-pixel kernels) and as a
    region of interest (pointer off by one byte, odd pitch: the scalar kernels);
  * rtdd_pyramid_set_image and the whole estimate (1000 iterations) under RTDD_GUIDE_GRAY and RTDD_GUIDE_BGR on the bundled Dog pair at
    its own size and tiled with mirroring to 1080p and 4K: host clock around a device synchronise.

The two guides alternate round by round on the same device: the median of the rounds and their spread.

    python scripts/color_guide_bench.py [--out profiles/r17_color_guide.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt

ROUNDS, CALLS = 7, 20


def tile(a, rows, cols):
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    return np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])


def roi(host):
    """The image inside a larger allocation: base pointer off by one byte, a pitch that is no multiple of 4.  Returns (keep-alive, (ptr, pitch))."""
    rows = host.shape[0]
    width = host.size // rows
    pitch = (width + 64) // 4 * 4 + 3
    base = torch.zeros(pitch * (rows + 1) + 16, dtype=torch.uint8, device="cuda:0")
    view = torch.as_strided(base, (rows, width), (pitch, 1), 1)
    view.copy_(torch.from_numpy(host.reshape(rows, width)).to("cuda:0"))
    return base, (base.data_ptr() + 1, pitch)


def spread(v):
    return f"{float(np.median(v)):8.1f} ({min(v):.1f}-{max(v):.1f})"


def prepare_pass(say):
    say(f"# prepare pass alone, us of device time per call: median of {ROUNDS} rounds of {CALLS} solves of 0 sweeps (min-max of the rounds)")
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K")):
        rng = np.random.default_rng(0)
        bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        gray = np.ascontiguousarray(bgr[..., 1])
        depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
        mask = np.where(rng.random((rows, cols)) < 0.01, 255, 0).astype(np.uint8)
        with rt.Context(0) as c:
            c.GPULoadWeights(0.4); c.GPUAllocateDeviceMemory(rows, cols, 1)
            d, m = rt.device_image(depth), rt.device_image(mask)
            keep_g, roi_g = roi(gray); keep_c, roi_c = roi(bgr)
            guides = {"gray aligned": (rt.device_image(gray), rt.GUIDE_GRAY), "bgr aligned": (rt.device_image(bgr), rt.GUIDE_BGR),
                      "gray roi": (roi_g, rt.GUIDE_GRAY), "bgr roi": (roi_c, rt.GUIDE_BGR)}
            c.profile_enable(True)
            t = {k: [] for k in guides}
            for r in range(ROUNDS + 1):                                 # (round 0 warms up)
                for k, (g, kind) in guides.items():
                    c.profile()
                    for _ in range(CALLS):
                        c.solve_guided(d, m, g, kind, rows, cols, 0, maxIterations=0)
                    us = c.profile().prepare_ms / CALLS * 1e3
                    if r:
                        t[k].append(us)
            med = {k: float(np.median(v)) for k, v in t.items()}
            say(f"{name:5s}: " + "  ".join(f"{k} {spread(v)}" for k, v in t.items()) +
                f"  | bgr / gray: aligned {med['bgr aligned'] / med['gray aligned']:.2f}, roi {med['bgr roi'] / med['gray roi']:.2f}")
            del keep_g, keep_c


def estimates(say):
    say(f"# rtdd_pyramid_set_image and the whole estimate (1000 iterations), us per call by the host clock around a synchronise: median of "
        f"{ROUNDS} rounds of {CALLS} calls, the guides alternating (min-max of the rounds)")
    g = np.load(os.path.join(ROOT, "tests", "golden", "Dog_full.npz"), allow_pickle=False)
    dog, dog_ann = g["bgr"], g["annotation"]
    sizes = [(dog.shape[0], dog.shape[1], "Dog"), (1080, 1920, "Dog tiled to 1080p"), (2160, 3840, "Dog tiled to 4K")]
    for rows, cols, name in sizes:
        bgr, ann = tile(dog, rows, cols), tile(dog_ann, rows, cols)
        ctxs = {}
        for kind, label in ((rt.GUIDE_GRAY, "gray"), (rt.GUIDE_BGR, "bgr")):
            c = rt.Context(0)
            c.GPULoadWeights(0.4); c.pyramid_create(rows, cols); c.pyramid_set_guide(kind)
            ctxs[label] = c
        b, a = rt.device_image(bgr), rt.device_image(ann)

        def timed(f, c, n):
            c.synchronize(); t0 = time.perf_counter()
            for _ in range(n):
                f()
            c.synchronize(); return (time.perf_counter() - t0) / n * 1e6
        t = {(k, w): [] for k in ctxs for w in ("set_image", "estimate")}
        for r in range(ROUNDS + 1):
            for k, c in ctxs.items():
                si = timed(lambda: c.pyramid_set_image(b), c, CALLS)
                c.pyramid_set_annotation(a)
                es = timed(lambda: c.estimate_depth(1000), c, CALLS)
                if r:
                    t[(k, "set_image")].append(si); t[(k, "estimate")].append(es)
        med = {k: float(np.median(v)) for k, v in t.items()}
        say(f"{name} ({cols} x {rows}): " + "  ".join(f"{w} {k} {spread(t[(k, w)])}" for w in ("set_image", "estimate") for k in ctxs) +
            f"  | bgr / gray: set_image {med[('bgr', 'set_image')] / med[('gray', 'set_image')]:.2f}, estimate {med[('bgr', 'estimate')] / med[('gray', 'estimate')]:.3f}")
        for c in ctxs.values():
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    prepare_pass(say)
    estimates(say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
