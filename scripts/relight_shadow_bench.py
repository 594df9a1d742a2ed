"""Relight with cast shadows against relight (include/rtdd.h rtdd_simulate_relight_shadowed, rtdd_simulate_relight) at 1080p, 4K and 8K
on a real depth map (the library's own estimate of the bundled Dog pair, tiled with mirroring to the size): rtdd_simulate_relight -- the
yardstick -- and the shadowed call with maxSteps 0 (the same kernel) and 64 / 256 / 1024, hard and soft, under a directional light and a
point light anchored at the centre pixel, all in ONE process per size.  Microseconds per call, host clock around a device synchronise,
the calls alternated over several rounds: the median and the spread (relight and maxSteps 0 as a pair of their own, the order of
the two reversed every round).  Beside each time the depth samples the kernel actually takes
(its exits counted: full shadow, the ray above every height, the image's edge, the light's column or row -- a torch restatement of
the kernel's groups of four steps) and the rate that makes, set against the L2 gather rate of MI355X_MICROARCH.md.

Each size runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/relight_shadow_bench.py [--out profiles/r12_relight_shadow.txt]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, CALLS = 7, 20
PAIR_ROUNDS = 14                     # relight and maxSteps 0, timed as a pair: 7 rounds in each order
SIZES = {"1080p": (1080, 1920), "4K": (2160, 3840), "8K": (4320, 7680)}
LIMIT_S = {"1080p": 240, "4K": 300, "8K": 420}
L2_GATHER_TBS = (16.8, 18.8)         # MI355X_MICROARCH.md, "Indexed rows": rows shared by every workgroup, served by the XCD's L2, chip-wide
GROUP = 4                            # relight_shadow.hip kShGroup


def samples_taken(torch, depth, light, steps, bias, softness, anchor):
    """The depth samples k_relight_shadow loads for this call: per pixel, groups of four steps until the group's last step is out (k > n,
    outside the image), q == 1, or (rise >= 0) the ray stands above relief * 255.  f32 on the device; a count, not a bit-exact image."""
    import math
    rows, cols = depth.shape
    relief = light.relief
    H = relief * (255.0 - depth.clamp(0.0, 255.0).nan_to_num(0.0))
    ys, xs = torch.meshgrid(torch.arange(rows, device=depth.device), torch.arange(cols, device=depth.device), indexing="ij")
    if light.kind == 0:
        n3 = math.sqrt(light.x ** 2 + light.y ** 2 + light.z ** 2)
        m = max(abs(light.x), abs(light.y)) / n3
        sx = torch.full_like(H, light.x / n3 / m); sy = torch.full_like(H, light.y / n3 / m); rise = torch.full_like(H, light.z / n3 / m)
        n = torch.full_like(xs, steps)
    else:
        Lz = relief * (255.0 - anchor) + light.z
        vx, vy, vz = light.x - xs.float(), light.y - ys.float(), Lz - H
        m = torch.maximum(vx.abs(), vy.abs())
        lit = m < 1
        m = m.clamp_min(1.0)
        sx, sy, rise = vx / m, vy / m, vz / m
        n = torch.where(lit, torch.zeros_like(xs), torch.minimum(torch.full_like(xs, steps), m.int()))
    h0, hmax = H + bias, relief * 255.0
    q = torch.zeros_like(H)
    alive = n >= 1
    total = 0
    for k0 in range(1, steps + 1, GROUP):
        if not bool(alive.any()):
            break
        for k in range(k0, k0 + GROUP):
            px, py = xs + torch.round(k * sx).long(), ys + torch.round(k * sy).long()
            inside = alive & (n >= k) & (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
            total += int(inside.sum())
            ray = h0 + k * rise
            occ = H[py.clamp(0, rows - 1), px.clamp(0, cols - 1)] - ray
            hit = inside & (occ > 0)
            qk = torch.ones_like(q) if softness == 0 else (occ / (k * softness)).clamp_max(1.0)
            q = torch.where(hit, torch.maximum(q, qk), q)
        alive = inside & (q < 1) & ~((rise >= 0) & (ray > hmax))
    return total, float((q > 0).float().mean())


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
    lights = {"directional": rt.Light(rt.LIGHT_DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.25, diffuse=1),
              "point": rt.Light(rt.LIGHT_POINT, cols * 0.4, rows * 0.3, 100, anchorX=cols // 2, anchorY=rows // 2, radius=cols / 4, relief=2,
                                ambient=0.25, diffuse=1)}
    anchor = float(min(max(dh[rows // 2, cols // 2], 0.0), 255.0))
    calls, shadows = {}, {}
    for lname, L in lights.items():
        calls[f"relight {lname}"] = lambda L=L: c.simulate_relight(o, d, art, rows, cols, L)
        for steps in (0, 64, 256, 1024):
            for sname, soft in (("hard", 0.0), ("soft", 0.5)):
                if steps == 0 and soft:
                    continue
                S = rt.Shadow(steps, 0.5, soft, 1.0)
                key = f"shadowed {lname} {steps}" + (f" {sname}" if steps else "")
                calls[key] = lambda L=L, S=S: c.simulate_relight_shadowed(o, d, art, rows, cols, L, S)
                shadows[key] = (L, steps, soft)
    for f in calls.values():
        for _ in range(3): f()
    t = {k: [] for k in calls}
    # The yardstick and the maxSteps-0 call launch the same kernel, so they are timed as a pair on their own, before the marches (a
    # 17 ms march just before a 10 us call moves it by more than the two differ), in PAIR_ROUNDS rounds whose order alternates:
    # yardstick first in the even rounds, maxSteps 0 first in the odd ones.
    pairs = [(f"relight {lname}", f"shadowed {lname} 0") for lname in lights]
    for r in range(PAIR_ROUNDS):
        for pair in pairs:
            for k in (pair if r % 2 == 0 else pair[::-1]):
                t[k].append(timeit(calls[k]))
    paired = {k for pair in pairs for k in pair}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            if k not in paired:
                t[k].append(timeit(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    dt = torch.from_numpy(dh).cuda()
    for k, v in t.items():
        yard = med["relight " + k.split()[1]]
        line = f"{name:5s} {k:32s} {med[k]:9.1f} us ({min(v):.1f}-{max(v):.1f}, spread {100 * (max(v) - min(v)) / med[k]:.1f} %)  x {med[k] / yard:6.2f} relight"
        if k in shadows and shadows[k][1] > 0:
            L, steps, soft = shadows[k]
            n, share = samples_taken(torch, dt, L, steps, 0.5, soft, anchor)
            rate = n / (med[k] * 1e-6)
            line += (f"  | {share:.3f} shadowed, {n / (rows * cols):7.1f} samples/px, {rate / 1e12:.3f} Tsamples/s = {4 * rate / 1e12:.2f} TB/s"
                     f" = {4 * rate / 1e12 / L2_GATHER_TBS[0]:.2f} of the L2 gather rate")
        print(line, flush=True)
    for lname in lights:                                  # maxSteps 0 launches k_relight itself: it must cost what the yardstick costs
        yard, zero = t[f"relight {lname}"], med[f"shadowed {lname} 0"]
        verdict = ("inside the yardstick's spread" if min(yard) <= zero <= max(yard) else
                   f"{100 * (min(yard) - zero) / min(yard):.1f} % BELOW the yardstick's fastest round" if zero < min(yard) else
                   f"{100 * (zero - max(yard)) / max(yard):.1f} % ABOVE the yardstick's slowest round")
        print(f"{name:5s} maxSteps 0 ({lname}) {zero:.1f} us against relight's {min(yard):.1f}-{max(yard):.1f} us: {verdict}", flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default=None, help="(internal) measure this size in this process")
    args = ap.parse_args()
    if args.size:
        measure(args.size)
        return 0
    lines = [f"# relight with cast shadows vs relight on the tiled Dog map, us per call: median of {ROUNDS} rounds of {CALLS} calls each (min-max of the rounds, "
             f"their spread over the median); relight and maxSteps 0: {PAIR_ROUNDS} rounds as a pair before the marches, the order of the two reversed every round; relief 2, ambient 0.25, diffuse 1, bias 0.5, soft = softness 0.5",
             f"# samples: the depth loads of the march, the kernel's exits counted; TB/s = 4 B per sample; L2 gather rate {L2_GATHER_TBS[0]}-{L2_GATHER_TBS[1]} TB/s "
             "chip-wide (MI355X_MICROARCH.md, 'Indexed rows: gather into LDS', rows served by the XCD's L2)"]
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
