#!/usr/bin/env python3
"""Count, on the CPU, how often the persistent 1080p sweep's row groups meet a tiny numerator on the bench image -- and how many of those
groups div_tiny's guard would still send to the IEEE divide.

    python3 scripts/count_tiny_groups.py [--seed 1234] [--rows 1080 --cols 1920] [--sweeps 1000]        (about a minute per seed)

The iterates are the oracle's own sweeps (bit-exact).  At every sweep the weighted sums are formed again in numpy (fma emulated in
float64: the count depends on their magnitude only) and the kernels' test 0 < |sum| < 2^-100 is mapped to (tile, wave, row group) of
k_sweep_blocked<32, 1024, 3>: tiles of 112 x 80 pixels extended by a halo of 8 to 128 x 96, thread row tr owns rows 3 tr .. 3 tr + 2, a wave
is two thread rows, and row group g of wave w is rows 6 w + g and 6 w + 3 + g.  Halo rows are counted with the true iterate (the kernel's
halo drifts from it inside a block of sweeps; the count is a census, not a replay).  A pixel is `suspect` when its scaled quotient
Q = RN24(sum 2^64 / cnt) lies on a midpoint of the 2^-149 grid (sweep_common.hpp div_tiny)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import oracle  # noqa: E402
from realtimedepthdiffusion_amd.synth import make_problem  # noqa: E402

TW, TH, HALO, G = 112, 80, 8, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--sweeps", type=int, default=1000)
    ap.add_argument("--threads", type=int, default=oracle.max_threads())
    args = ap.parse_args()
    rows, cols = args.rows, args.cols
    p = make_problem(rows, cols, seed=args.seed)
    lut = oracle.load_weights(0.4)
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    w = [lut[idx[..., 0] // 1000], lut[idx[..., 0] % 1000], lut[idx[..., 1] // 1000], lut[idx[..., 1] % 1000]]      # left, right, up, down
    cnt = np.float32(0)
    for k in range(4):
        cnt = (cnt + w[k]).astype(np.float32)
    cnt = np.where(cnt == 0, np.float32(1), cnt).astype(np.float64)
    w = [a.astype(np.float64) for a in w]
    gx, gy = -(-cols // TW), -(-rows // TH)
    ew, eh = TW + 2 * HALO, TH + 2 * HALO
    nwaves = eh // (2 * G)
    omegas = oracle.omega_schedule(args.sweeps)
    x = p["depth"].copy()
    prev = np.zeros_like(x)                    # the reference's x_{-1} is 0 on free pixels (src/GPUSolver.cu:290)
    first = None
    per_tile, per_tile_fallback = {}, {}
    groups = fallback = 0
    pad_t = np.zeros((gy * TH + 2 * HALO, gx * TW + 2 * HALO), bool)
    pad_s = np.zeros_like(pad_t)
    for s in range(args.sweeps):
        x64 = x.astype(np.float64)
        z = np.zeros_like(x64)
        nb = [z.copy(), z.copy(), z.copy(), z.copy()]
        nb[0][:, 1:] = x64[:, :-1]; nb[1][:, :-1] = x64[:, 1:]; nb[2][1:] = x64[:-1]; nb[3][:-1] = x64[1:]
        sm = np.zeros_like(x)
        for k in range(4):
            sm = (w[k] * nb[k] + sm.astype(np.float64)).astype(np.float32)
        tiny = (np.abs(sm) < np.float32(2.0 ** -100)) & (sm != 0)
        if tiny.any():
            if first is None:
                first = s
            N = sm.astype(np.float64) * 2.0 ** 64
            with np.errstate(all="ignore"):
                Q = np.where(tiny, N / cnt, 0.0).astype(np.float32)
                q = (Q * np.float32(2.0 ** -64)).astype(np.float32)
                sus = tiny & (np.abs(Q.astype(np.float64) - q.astype(np.float64) * 2.0 ** 64) == 2.0 ** -86)
            pad_t[:] = False; pad_s[:] = False
            pad_t[HALO:HALO + rows, HALO:HALO + cols] = tiny
            pad_s[HALO:HALO + rows, HALO:HALO + cols] = sus
            ys, xs = np.nonzero(tiny)
            cand = set()
            for by in range(gy):
                in_y = (ys >= by * TH - HALO) & (ys < by * TH + TH + HALO)
                if not in_y.any():
                    continue
                for bx in range(gx):
                    if (in_y & (xs >= bx * TW - HALO) & (xs < bx * TW + TW + HALO)).any():
                        cand.add((by, bx))
            for by, bx in cand:
                t = pad_t[by * TH:by * TH + eh, bx * TW:bx * TW + ew].reshape(nwaves, 2, G, ew).any(axis=(1, 3))      # [wave, group]
                u = pad_s[by * TH:by * TH + eh, bx * TW:bx * TW + ew].reshape(nwaves, 2, G, ew).any(axis=(1, 3))
                n, f = int(t.sum()), int((t & u).sum())
                groups += n; fallback += f
                per_tile[(by, bx)] = per_tile.get((by, bx), 0) + n
                per_tile_fallback[(by, bx)] = per_tile_fallback.get((by, bx), 0) + f
        x = oracle.sweep(x, idx, p["mask"], prev, omegas[s], lut, 1, threads=args.threads)
    busiest = max(per_tile, key=per_tile.get) if per_tile else None
    print(f"seed {args.seed} {cols}x{rows} {args.sweeps} sweeps: first sweep with a tiny numerator {first}, redo groups {groups}, "
          f"of them with a suspect lane {fallback}; busiest tile {busiest}: {per_tile.get(busiest, 0)} groups, {per_tile_fallback.get(busiest, 0)} with a suspect "
          f"(of {nwaves * G} groups x {args.sweeps} sweeps); tiles ever hit {len(per_tile)} of {gx * gy}; smallest |iterate| > 0 at the end "
          f"{np.abs(x[x != 0]).min() if (x != 0).any() else 0:.3g}")


if __name__ == "__main__":
    main()
