"""Ambient occlusion against relight (include/rtdd.h rtdd_simulate_ambient_occlusion, rtdd_simulate_relight) at 1080p, 4K and 8K on a
real depth map (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size): rtdd_simulate_relight under a
directional light -- the yardstick -- and the occlusion at radius 8 / 16 / 64 with 4 and 8 directions, without a light and under the
yardstick's light, all in ONE process per size.  Microseconds per call, host clock around a device synchronise, the calls alternated
over several rounds: the median and the spread, the ratio to the yardstick, and the height samples the kernel takes per second (it
takes no early exit: directions * radius LDS reads per pixel, whatever the map holds).

Each size runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/ambient_occlusion_bench.py [--out profiles/r14_ambient_occlusion.txt]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, CALLS = 7, 20
SIZES = {"1080p": (1080, 1920), "4K": (2160, 3840), "8K": (4320, 7680)}
LIMIT_S = {"1080p": 120, "4K": 150, "8K": 240}
RADII, DIRECTIONS = (8, 16, 64), (4, 8)


def measure(name):
    import numpy as np
    import torch

    import realtimedepthdiffusion_amd as rt

    def timeit(f, n=CALLS):
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(n): f()
        torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6

    g = np.load(os.path.join(ROOT, "tests", "golden", "Dog_full.npz"), allow_pickle=False)
    bgr, ann = g["bgr"], g["annotation"]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4); c.pyramid_create(*ann.shape)
        c.pyramid_set_image(rt.device_image(bgr)); c.pyramid_set_annotation(rt.device_image(ann))
        c.estimate_depth(1000); c.synchronize()
        a = c.pyramid_download(rt.IMG_DEPTH, 0)
    rows, cols = SIZES[name]
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    dh = np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])
    orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    c = rt.Context(0)
    o = rt.device_image(orig); art = rt.device_image(np.zeros_like(orig)); d = rt.device_image(dh)
    L = rt.Light(rt.LIGHT_DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.5, diffuse=1)
    calls, samples = {"relight directional": lambda: c.simulate_relight(o, d, art, rows, cols, L)}, {}
    for lname, light in (("no light", None), ("directional", L)):
        for radius in RADII:
            for directions in DIRECTIONS:
                A = rt.AmbientOcclusion(rt.AO_SHADE, directions, radius, 2.0, 0.5, 1.0)
                key = f"ao {lname} radius {radius} x {directions}"
                calls[key] = lambda A=A, light=light: c.simulate_ambient_occlusion(o, d, art, rows, cols, A, light)
                samples[key] = rows * cols * directions * radius
    for f in calls.values():
        for _ in range(3): f()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            t[k].append(timeit(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    yard = med["relight directional"]
    for k, v in t.items():
        line = f"{name:5s} {k:32s} {med[k]:9.1f} us ({min(v):.1f}-{max(v):.1f}, spread {100 * (max(v) - min(v)) / med[k]:.1f} %)  x {med[k] / yard:6.2f} relight"
        if k in samples:
            rate = samples[k] / (med[k] * 1e-6)
            line += f"  | {samples[k] / (rows * cols):4.0f} samples/px, {rate / 1e12:.3f} Tsamples/s = {4 * rate / 1e12:.2f} TB/s from LDS"
        print(line, flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default=None, help="(internal) measure this size in this process")
    args = ap.parse_args()
    if args.size:
        measure(args.size)
        return 0
    lines = [f"# ambient occlusion vs relight on the tiled Dog map, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds, "
             "their spread over the median); relief 2, ambient 0.5, diffuse 1, bias 0.5, strength 1; the light: directional (-1, -1, 1)",
             "# samples: directions * radius height reads per pixel from LDS (the kernel takes no early exit); TB/s = 4 B per sample"]
    rc = 0
    for name in SIZES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", name], capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result inside {LIMIT_S[name]} s; the run ends here"); rc = 124; break
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            print(r.stderr[-2000:], file=sys.stderr)
            lines.append(f"{name}: exit status {r.returncode}; the run ends here"); rc = r.returncode; break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
