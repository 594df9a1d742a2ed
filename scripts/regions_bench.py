"""The depth regions' cost (include/rtdd.h rtdd_solve_regions, rtdd_pyramid_set_regions), in one session:

  * the prepare pass alone at 1080p, 4K and 8K -- a solve of 0 sweeps, the device time between the events in front of and behind its
    prepare launch (rtdd_profile.prepare_ms) -- without and with region codes (cut and smooth), for a gray and a BGR guide, aligned
    allocations (the four-pixel kernels);
  * k_region_codes alone -- rtdd_region_codes for level 0 of a 1080p / 4K / 8K pair, host clock around a device synchronise -- and the
    pyramid's own launch (every level at once) as the difference of a 1080p estimate of 0 iterations with and without a changed pair;
  * whole 1080p estimates (1000 iterations, the bundled Dog pair tiled with mirroring) with regions off, cut, and cut plus smooth, the
    three alternating round by round;
  * with --parent-tree DIR (a built checkout of the parent commit): the 1080p estimate with regions off in child processes, this tree
    and the parent's alternating, and whether this tree's median lies inside the parent's min-max of rounds; then bench.py of both trees,
    alternating, five runs each, and the same statement.

    python scripts/regions_bench.py [--parent-tree DIR] [--out profiles/r21_regions.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if "--tree" in sys.argv:                                    # (a child: the package and the golden pair of that checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
import numpy as np

import realtimedepthdiffusion_amd as rt

ROUNDS, CALLS = 7, 20
SIZES = ((1080, 1920, "1080p"), (2160, 3840, "4K"), (4320, 7680, "8K"))


def tile(a, rows, cols):
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    return np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])


def spread(v):
    return f"{float(np.median(v)):8.1f} ({min(v):.1f}-{max(v):.1f})"


def timed(f, c, n):
    c.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        f()
    c.synchronize(); return (time.perf_counter() - t0) / n * 1e6


def region_image(rows, cols):
    """Rectangles of 64 x 48 pixels with ids 0..3: long runs of equal codes, a cut every 64 pixels."""
    yy, xx = np.mgrid[:rows, :cols]
    return np.ascontiguousarray(((yy // 48 + xx // 64) % 4).astype(np.uint8))


def prepare_pass(say):
    say(f"# prepare pass alone, us of device time per call: median of {ROUNDS} rounds of {CALLS} solves of 0 sweeps (min-max of the rounds)")
    for rows, cols, name in SIZES:
        rng = np.random.default_rng(0)
        bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        gray = np.ascontiguousarray(bgr[..., 1])
        depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
        mask = np.where(rng.random((rows, cols)) < 0.01, 255, 0).astype(np.uint8)
        with rt.Context(0) as c:
            c.GPULoadWeights(0.4); c.GPUAllocateDeviceMemory(rows, cols, 1)
            d, m, r = rt.device_image(depth), rt.device_image(mask), rt.device_image(region_image(rows, cols))
            guides = {"gray": (rt.device_image(gray), rt.GUIDE_GRAY), "bgr": (rt.device_image(bgr), rt.GUIDE_BGR)}
            cases = {(k, w): None for k in guides for w in ("plain", "regions")}
            c.profile_enable(True)
            t = {k: [] for k in cases}
            for rnd in range(ROUNDS + 1):                               # (round 0 warms up)
                for (k, w) in cases:
                    g, kind = guides[k]
                    c.profile()
                    for _ in range(CALLS):
                        c.solve_regions(d, m, g, kind, r if w == "regions" else None, 3 if w == "regions" else 0, rows, cols, 0, maxIterations=0)
                    us = c.profile().prepare_ms / CALLS * 1e3
                    if rnd:
                        t[(k, w)].append(us)
            med = {k: float(np.median(v)) for k, v in t.items()}
            say(f"{name:5s}: " + "  ".join(f"{k} {w} {spread(v)}" for (k, w), v in t.items()) +
                f"  | regions / plain: gray {med[('gray', 'regions')] / med[('gray', 'plain')]:.2f}, bgr {med[('bgr', 'regions')] / med[('bgr', 'plain')]:.2f}")


def codes_pass(say):
    say(f"# k_region_codes alone (rtdd_region_codes, level 0), us per call by the host clock around a synchronise: median of {ROUNDS} rounds of {CALLS} calls")
    for rows, cols, name in SIZES:
        rng = np.random.default_rng(1)
        edited = np.repeat(region_image(rows, cols)[..., None], 3, axis=2)
        mask = np.where(rng.random((rows, cols)) < 0.7, 255, 0).astype(np.uint8)
        with rt.Context(0) as c:
            e, m, out = rt.device_image(edited), rt.device_image(mask), rt.device_image(np.zeros((rows, cols), np.uint8))
            t = [timed(lambda: c.region_codes(e, m, rows, cols, 0, out), c, CALLS) for _ in range(ROUNDS + 1)][1:]
            say(f"{name:5s}: {spread(t)}  ({rows * cols * 5 / float(np.median(t)) / 1e6:.2f} TB/s of 4 B read + 1 written per pixel)")


def dog_pair(rows, cols):
    g = np.load(os.path.join(ROOT, "tests", "golden", "Dog_full.npz"), allow_pickle=False)
    return tile(g["bgr"], rows, cols), tile(g["annotation"], rows, cols)


def estimates(say):
    rows, cols = 1080, 1920
    say(f"# whole 1080p estimates (1000 iterations, Dog tiled), us per call by the host clock around a synchronise: median of {ROUNDS} rounds of "
        f"{CALLS} calls, the three alternating (min-max of the rounds)")
    bgr, ann = dog_pair(rows, cols)
    ctxs = {}
    b, a = rt.device_image(bgr), rt.device_image(ann)
    for label, flags in (("off", 0), ("cut", rt.REGION_CUT), ("cut+smooth", rt.REGION_CUT | rt.REGION_SMOOTH)):
        c = rt.Context(0)
        c.GPULoadWeights(0.4); c.pyramid_create(rows, cols)
        c.pyramid_set_regions(rt.REGION_CUT)                            # (every context holds the images; "off" has the flags at 0)
        c.pyramid_set_image(b); c.pyramid_set_annotation(a)
        e, m = c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2]
        for i, (x0, y0, x1, y1) in enumerate(((200, 150, 900, 700), (1000, 300, 1700, 1000), (100, 800, 800, 1050))):
            c.fill_polygon([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], (0, 0, 0, 0, 0, i + 1, i + 1), e, m, rows, cols)
        c.pyramid_set_regions(flags)
        ctxs[label] = c
    t = {k: [] for k in ctxs}
    for rnd in range(ROUNDS + 1):
        for k, c in ctxs.items():
            us = timed(lambda: c.estimate_depth(1000), c, CALLS)
            if rnd:
                t[k].append(us)
    med = {k: float(np.median(v)) for k, v in t.items()}
    say("1080p: " + "  ".join(f"{k} {spread(v)}" for k, v in t.items()) + f"  | cut / off {med['cut'] / med['off']:.3f}, cut+smooth / off {med['cut+smooth'] / med['off']:.3f}")
    # the pyramid's own k_region_codes launch (every level): estimates of 0 iterations with and without a changed pair in front
    c = ctxs["cut"]
    plain = [timed(lambda: c.estimate_depth(0), c, CALLS) for _ in range(ROUNDS + 1)][1:]

    def changed():
        c.pyramid_regions_changed(); c.estimate_depth(0)
    dirty = [timed(changed, c, CALLS) for _ in range(ROUNDS + 1)][1:]
    say(f"1080p estimate of 0 iterations: {spread(plain)}; with rtdd_pyramid_regions_changed in front (k_region_codes, every level, behind the synchronisation that settles the logged estimates): {spread(dirty)}")
    for c in ctxs.values():
        c.close()


def child_estimate():
    """(a child process, this tree or the parent's: nothing but calls the parent has too)  Prints the rounds as JSON."""
    rows, cols = 1080, 1920
    bgr, ann = dog_pair(rows, cols)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4); c.pyramid_create(rows, cols)
        b, a = rt.device_image(bgr), rt.device_image(ann)
        c.pyramid_set_image(b); c.pyramid_set_annotation(a)
        t = [timed(lambda: c.estimate_depth(1000), c, CALLS) for _ in range(ROUNDS + 1)][1:]
    print(json.dumps(t))


def against_parent(say, parent):
    say(f"# 1080p estimate (1000 iterations, Dog tiled), regions off, this tree against the parent commit's: child processes alternating, "
        f"{ROUNDS} rounds of {CALLS} calls each, twice per tree; us per call")
    t = {"parent": [], "this": []}
    for _ in range(2):
        for k, tree in (("parent", parent), ("this", HERE)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-estimate", "--tree", tree], capture_output=True, text=True, timeout=300, check=True)
            t[k] += json.loads(out.stdout.strip().splitlines()[-1])
    med = float(np.median(t["this"]))
    inside = min(t["parent"]) <= med <= max(t["parent"])
    say(f"parent {spread(t['parent'])}  this tree {spread(t['this'])}  | this tree's median {'lies inside' if inside else 'LIES OUTSIDE'} the parent's min-max of rounds")


def bench_py(say, parent):
    args = ["--gpus", "1", "--steps", "20", "--warmup", "3"]
    say(f"# bench.py {' '.join(args)} (1080p_jacobi1000, regions off: the benchmark knows none), the parent commit's tree and this one alternating, "
        "five runs each; ms per step")
    t = {"parent": [], "this": []}
    for _ in range(5):
        for k, tree in (("parent", parent), ("this", HERE)):
            out = subprocess.run([sys.executable, "bench.py"] + args, cwd=tree, capture_output=True, text=True, timeout=300, check=True)
            t[k].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
    med = float(np.median(t["this"]))
    inside = min(t["parent"]) <= med <= max(t["parent"])
    say("  ".join(f"{name} {float(np.median(v)):.4f} ({min(v):.4f}-{max(v):.4f})" for name, v in (("parent", t["parent"]), ("this tree", t["this"]))) +
        f"  | this tree's median {'lies inside' if inside else 'LIES OUTSIDE'} the parent's min-max of runs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-estimate", action="store_true")
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    if args.child_estimate:
        return child_estimate()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    prepare_pass(say)
    codes_pass(say)
    estimates(say)
    if args.parent_tree:
        against_parent(say, args.parent_tree)
        bench_py(say, args.parent_tree)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
