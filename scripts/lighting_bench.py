"""The whole lighting model in one call against the two calls it replaces (include/rtdd.h rtdd_simulate_lighting against
rtdd_simulate_relight_shadowed followed by rtdd_simulate_ambient_occlusion under the same light) at 1080p, 4K and 8K on a real depth
map (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size), all in ONE process per size: a directional
and a point light, 64 and 256 steps, hard and soft shadows, radius 8 / 16 / 64 with 8 directions.  The baseline is the pair back to
back on the same images; the fused call and the pair take turns at going first, round by round.  Microseconds, host clock around a
device synchronise: the median of the rounds and their min-max, the ratio fused / pair, and whether the fused call is slower than the
pair BEYOND the rounds' own spread (its fastest round slower than the pair's slowest).  Then the call with a term disabled against the
kernel it dispatches to: it is that kernel.

Each size runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/lighting_bench.py [--out profiles/r15_lighting.txt]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, CALLS = 7, 20
SIZES = {"1080p": (1080, 1920), "4K": (2160, 3840), "8K": (4320, 7680)}
LIMIT_S = {"1080p": 150, "4K": 240, "8K": 420}
STEPS, SOFTNESS, RADII = (64, 256), (0.0, 1.0), (8, 16, 64)


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
    lights = {"directional": rt.Light(rt.LIGHT_DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.5, diffuse=1),
              "point": rt.Light(rt.LIGHT_POINT, cols * 0.4, rows * 0.3, 120, anchorX=cols // 2, anchorY=rows // 2, radius=cols / 4, relief=2, ambient=0.5, diffuse=1)}

    def shadowed(L, S): return lambda: c.simulate_relight_shadowed(o, d, art, rows, cols, L, S)
    def occluded(L, A): return lambda: c.simulate_ambient_occlusion(o, d, art, rows, cols, A, L)
    def fused(L, S, A): return lambda: c.simulate_lighting(o, d, art, rows, cols, L, S, A)

    def pair(L, S, A):
        f1, f2 = shadowed(L, S), occluded(L, A)
        def both(): f1(); f2()
        return both

    def compare(key, new, old, old_name):
        """new against old, taking turns at going first; prints the medians, the spreads and the verdict"""
        for f in (new, old):
            for _ in range(3): f()
        tn, to = [], []
        for r in range(ROUNDS):
            if r % 2: tn.append(timeit(new)); to.append(timeit(old))
            else: to.append(timeit(old)); tn.append(timeit(new))
        mn, mo = float(np.median(tn)), float(np.median(to))
        verdict = "SLOWER beyond the spread" if min(tn) > max(to) else "faster beyond the spread" if max(tn) < min(to) else "within the spread"
        print(f"{name:5s} {key:52s} lighting {mn:9.1f} us ({min(tn):.1f}-{max(tn):.1f})  {old_name} {mo:9.1f} us ({min(to):.1f}-{max(to):.1f})  "
              f"x {mn / mo:5.2f}  {verdict}", flush=True)

    for lname, L in lights.items():
        for steps in STEPS:
            for softness in SOFTNESS:
                for radius in RADII:
                    S = rt.Shadow(steps, 0.5, softness, 1.0)
                    A = rt.AmbientOcclusion(rt.AO_SHADE, 8, radius, 2.0, 0.5, 1.0)
                    compare(f"{lname} {steps} steps {'soft' if softness else 'hard'} radius {radius} x 8", fused(L, S, A), pair(L, S, A), "the pair")
    # a term disabled: the launch is the remaining kernel's own
    L = lights["directional"]
    S, A = rt.Shadow(256, 0.5, 0.0, 1.0), rt.AmbientOcclusion(rt.AO_SHADE, 8, 16, 2.0, 0.5, 1.0)
    S0, A0 = rt.Shadow(0, 0.5, 0.0, 1.0), rt.AmbientOcclusion(rt.AO_SHADE, 8, 0, 2.0, 0.5, 1.0)
    compare("no shadows (0 steps), radius 16 x 8", fused(L, S0, A), occluded(L, A), "ambient_occlusion")
    compare("256 steps hard, no occlusion (radius 0)", fused(L, S, A0), shadowed(L, S), "relight_shadowed")
    compare("neither term", fused(L, S0, A0), lambda: c.simulate_relight(o, d, art, rows, cols, L), "relight")
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default=None, help="(internal) measure this size in this process")
    args = ap.parse_args()
    if args.size:
        measure(args.size)
        return 0
    lines = [f"# rtdd_simulate_lighting against rtdd_simulate_relight_shadowed + rtdd_simulate_ambient_occlusion(light) back to back on the tiled Dog map, us: "
             f"median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); the two take turns at going first",
             "# relief 2, ambient 0.5, diffuse 1; shadows: bias 0.5, softness 0 (hard) or 1 (soft), strength 1; occlusion: 8 directions, bias 0.5, strength 1",
             "# the lights: directional (-1, -1, 1); point at (0.4 cols, 0.3 rows), 120 above the centre pixel, radius cols / 4",
             "# verdict: SLOWER beyond the spread = the fused call's fastest round is slower than the baseline's slowest"]
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
