"""The two-layer parallax view (include/rtdd.h rtdd_simulate_parallax_layered) against rtdd_simulate_parallax at 1080p and 4K on a real
depth map (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size).  A disc of 0.2 x the height in the
middle of the image is selected and removed (rtdd_remove_object, grow 2) as the plate; the view is (shiftX, shiftY, dolly) =
(30, -12, 0.05), zero parallax at 128.  Timed, in alternating order in one session:
  single       rtdd_simulate_parallax (its own cost is recorded here too)
  bare         the layered call with plate, depthOut and coverage NULL: the same launches -- its median should lie inside single's min-max
  plate        the layered call with the plate
  plate+outs   the layered call with the plate, depthOut and coverage
Microseconds per call, host clock around a device synchronise: the median of the rounds and their min-max.  From the restatement
(tests/parallax_layers_ref.py), which also checks every output once: the share of holes before and after, the share of cracks, and the
number of plate atomics actually issued (plate sources whose d' differs from the front's at their own pixel and that land inside).

    python scripts/parallax_layered_bench.py [--out profiles/r24_parallax_layered.txt] [--no-stats]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import realtimedepthdiffusion_amd as rt
from parallax_layers_ref import parallax_layers
from parallax_bench import dog_depth, tile

ROUNDS, CALLS = 7, 20
VIEW = (30, -12, 0.05)


def timeit(f, n=CALLS):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-stats", action="store_true", help="leave out the restatement: no hole and crack statistics, no check of the outputs")
    args = ap.parse_args()
    lines = [f"# layered parallax vs parallax, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds); the tiled Dog map,",
             f"# a disc of 0.2 x the height removed as the plate (grow 2), view {VIEW}, z0 = 128"]

    def say(s):
        print(s, flush=True); lines.append(s)

    dog = dog_depth()
    for rows, cols, name in ((1080, 1920, "1080p"), (2160, 3840, "4K")):
        orig = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        dh = tile(dog, rows, cols)
        yy, xx = np.mgrid[0:rows, 0:cols]
        r = 0.1 * rows                                      # a disc 0.2 x the height across
        mask = (((xx - cols // 2) ** 2 + (yy - rows // 2) ** 2) <= r * r).astype(np.uint8)
        c = rt.Context(0)
        up = rt.device_image
        o, d, m = up(orig), up(dh), up(mask)
        plate, pz = up(np.zeros_like(orig)), up(np.zeros_like(dh))
        c.remove_object(o, d, m, plate, pz, rows, cols, rt.Removal(0, 2, 0.0))
        c.synchronize()
        art, z, cv = up(np.zeros_like(orig)), up(np.zeros_like(dh)), up(np.zeros((rows, cols), np.uint8))
        view = rt.Parallax(VIEW[0], VIEW[1], VIEW[2], 128.0)
        calls = {"single": lambda: c.simulate_parallax(o, d, art, rows, cols, view),
                 "bare": lambda: c.simulate_parallax_layered(o, d, None, None, art, None, None, rows, cols, view),
                 "plate": lambda: c.simulate_parallax_layered(o, d, plate, pz, art, None, None, rows, cols, view),
                 "plate+outs": lambda: c.simulate_parallax_layered(o, d, plate, pz, art, z, cv, rows, cols, view)}
        for f in calls.values():
            for _ in range(3): f()
        t = {k: [] for k in calls}
        for rnd in range(ROUNDS):
            order = list(calls.items())
            if rnd % 2: order.reverse()                     # alternating order
            for k, f in order:
                t[k].append(timeit(f))
        med = {k: float(np.median(v)) for k, v in t.items()}
        say(f"{name:5s}:  " + "  ".join(f"{k} {med[k]:8.1f} ({min(v):.1f}-{max(v):.1f})" for k, v in t.items()))
        say(f"{name:5s} / single:  " + "  ".join(f"{k} {med[k] / med['single']:.2f}" for k in calls if k != "single") +
            f"   (bare inside single's min-max: {'yes' if min(t['single']) <= med['bare'] <= max(t['single']) else 'NO'})")
        if not args.no_stats:
            ph, pd = rt.to_host(plate), rt.to_host(pz)
            before, after = {}, {}
            parallax_layers(orig, dh, None, None, *VIEW, 128.0, stats=before)
            want = parallax_layers(orig, dh, ph, pd, *VIEW, 128.0, stats=after)
            calls["plate+outs"](); c.synchronize()
            same = (np.array_equal(rt.to_host(art), want[0]) and np.array_equal(rt.to_host(z).view(np.uint32), want[1].view(np.uint32)) and
                    np.array_equal(rt.to_host(cv), want[2]))
            say(f"{name:5s} holes {100 * before['holes']:.3f} % with one layer, {100 * after['holes']:.3f} % with the plate; cracks {100 * after['cracks']:.3f} %; "
                f"plate atomics issued {after['plate_atomics']} of {rows * cols} plate pixels ({int(mask.sum())} selected); outputs {'equal' if same else 'DIFFER'}")
        c.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
