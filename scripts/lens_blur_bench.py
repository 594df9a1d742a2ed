"""The round-aperture lens blur against the box (include/rtdd.h rtdd_simulate_lens_blur RTDD_APERTURE_DISC, rtdd_simulate_refocus) at
1080p, 4K and 8K, automatic path, default aperture, f = 0 and f = 128, on the three depth maps of bench.py's effects leg: smooth, the
library's estimate of the bundled Dog pair tiled to the size, and a random depth per pixel.  Microseconds per call from HIP events
around CALLS calls on the context's stream, box and disc alternated over ROUNDS rounds in one process after a warm-up: the median and
the spread (min-max) of the rounds.

    python scripts/lens_blur_bench.py [--out profiles/r10_lens_blur.txt]

--ab OTHER.so: no regression of the existing effects -- rtdd_simulate_defocus and rtdd_simulate_refocus with this tree's library and with
OTHER.so (the parent commit's build), one child process per library and round, alternated.
--disc-only SIZE: one size's disc calls and nothing else (the kernel to count under a profiler)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ROUNDS, CALLS = 5, 20
SIZES = ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K"))


def event_us(torch, f, n=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n): f()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / n * 1e3


def dog_depth(rt):
    g = np.load(os.path.join(ROOT, "tests", "golden", "Dog_full.npz"), allow_pickle=False)
    bgr, ann = g["bgr"], g["annotation"]
    rows, cols = ann.shape
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4); c.pyramid_create(rows, cols)
        c.pyramid_set_image(rt.device_image(bgr)); c.pyramid_set_annotation(rt.device_image(ann))
        c.estimate_depth(1000); c.synchronize()
        return c.pyramid_download(rt.IMG_DEPTH, 0)


def tile(a, rows, cols):
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    return np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])


def setup(rt, torch, rows, cols, dog):
    from realtimedepthdiffusion_amd.synth import make_problem
    p = make_problem(rows, cols, seed=1)
    rng = np.random.default_rng(0)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    rnd = (p["depth"] * rng.uniform(0, 1, (rows, cols))).astype(np.float32)
    c = rt.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    o = rt.device_image(orig); art = rt.device_image(np.zeros_like(orig))
    maps = {"smooth": rt.device_image(p["gray"].astype(np.float32)), "Dog tiled": rt.device_image(tile(dog, rows, cols)), "random": rt.device_image(rnd)}
    return c, o, art, maps


def run_rounds(torch, calls):
    for f in calls.values():                # warm-up: code objects, the table's allocation
        for _ in range(3): f()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            t[k].append(event_us(torch, f))
    return t


def disc_vs_box(say):
    import torch
    import realtimedepthdiffusion_amd as rt
    say(f"# disc vs box, automatic path, aperture 0.025, us per call (HIP events around {CALLS} calls): median of {ROUNDS} alternated rounds (min-max)")
    dog = dog_depth(rt)
    for rows, cols, name in SIZES:
        c, o, art, maps = setup(rt, torch, rows, cols, dog)
        for mname, d in maps.items():
            for f in (0.0, 128.0):
                calls = {"box": lambda: c.simulate_refocus(o, d, art, rows, cols, 0.025, f, -1, -1),
                         "disc": lambda: c.simulate_lens_blur(o, d, art, rows, cols, 0.025, f, -1, -1, rt.APERTURE_DISC)}
                t = run_rounds(torch, calls)
                med = {k: float(np.median(v)) for k, v in t.items()}
                line = f"{name:5s} {mname:9s} f={f:5.1f} path {c.get_option(rt.OPT_DEFOCUS_LAST_PATH)}:"
                for k, v in t.items():
                    line += f"  {k} {med[k]:8.1f} ({min(v):.1f}-{max(v):.1f})"
                say(line + f"  | disc / box = {med['disc'] / med['box']:.2f}")
        c.close()


def existing_effects():
    """One child of --ab: defocus and refocus (f = 128) on the smooth map at every size, one JSON line."""
    import torch
    import realtimedepthdiffusion_amd as rt
    if os.environ.get("RTDD_LIBRARY"):      # (a build from before the lens blur: the binding would refuse to load it)
        rt.C_ABI_SYMBOLS.remove("rtdd_simulate_lens_blur")
    out = {}
    dog = np.zeros((8, 8), np.float32)      # (the Dog map is not measured here)
    for rows, cols, name in SIZES:
        c, o, art, maps = setup(rt, torch, rows, cols, dog)
        d = maps["smooth"]
        t = run_rounds(torch, {"defocus": lambda: c.GPUSimulateDefocus(o, d, art, rows, cols),
                               "refocus": lambda: c.simulate_refocus(o, d, art, rows, cols, 0.025, 128.0, -1, -1)})
        for k, v in t.items():
            out[f"{name} {k}"] = float(np.median(v))
        c.close()
    print("AB " + json.dumps(out), flush=True)


def ab(say, other, rounds=2):
    say(f"# no regression: defocus / refocus f=128 on the smooth map, us per call, this tree's library (new) against {os.path.basename(os.path.dirname(os.path.abspath(other)))}/"
        f"{os.path.basename(other)} (old): {rounds} child processes each, alternated; median (min-max) of the processes' medians")
    res = {"new": [], "old": []}
    for _ in range(rounds):
        for which, lib in (("old", other), ("new", None)):
            env = dict(os.environ)
            if lib: env["RTDD_LIBRARY"] = os.path.abspath(lib)
            else: env.pop("RTDD_LIBRARY", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                say(f"child ({which}) failed with status {r.returncode}: {r.stderr[-400:]}")
                return 1                            # nothing more is started on the GPU
            res[which].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    for key in res["new"][0]:
        n = [x[key] for x in res["new"]]; o = [x[key] for x in res["old"]]
        say(f"{key:14s} old {np.median(o):8.1f} ({min(o):.1f}-{max(o):.1f})  new {np.median(n):8.1f} ({min(n):.1f}-{max(n):.1f})  | new / old = {np.median(n) / np.median(o):.3f}")
    return 0


def disc_only(size):
    import torch
    import realtimedepthdiffusion_amd as rt
    rows, cols, _ = [s for s in SIZES if s[2] == size][0]
    c, o, art, maps = setup(rt, torch, rows, cols, dog_depth(rt))
    for d in maps.values():
        for _ in range(5):
            c.simulate_lens_blur(o, d, art, rows, cols, 0.025, 128.0, -1, -1, rt.APERTURE_DISC)
    c.synchronize(); c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--disc-only", default=None)
    args = ap.parse_args()
    if args.child:
        return existing_effects()
    if args.disc_only:
        return disc_only(args.disc_only)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    rc = ab(say, args.ab) if args.ab else disc_vs_box(say)
    if args.out:
        with open(args.out, "a" if args.ab else "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
