"""Where a rtdd_remove_object call spends its time, kernel by kernel (the second section of profiles/r23_remove.txt).  Two steps:

    rocprofv3 --kernel-trace -d DIR -o t -- python scripts/remove_trace.py run empty|disc GROW     # 30 calls at 1080p under the tracer
    python scripts/remove_trace.py report LABEL=DIR/t_results.db ...                                # per kernel: calls, mean and min us

`run` uses the images of scripts/remove_bench.py's 1080p case with a random depth map: an empty mask, or a disc of 0.1 x the height.
`report` reads the tracer's database (its `kernels` view) and prints the library's kernels only."""
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CALLS = 30


def run(case, grow):
    import numpy as np
    import realtimedepthdiffusion_amd as rt
    from remove_bench import disc
    rows, cols = 1080, 1920
    rng = np.random.default_rng(0)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    mask = np.zeros((rows, cols), np.uint8) if case == "empty" else disc(rows, cols, 0.1)
    with rt.Context(0) as c:
        o, d, m = rt.device_image(orig), rt.device_image(depth), rt.device_image(mask)
        art, z = rt.device_image(np.zeros_like(orig)), rt.device_image(np.zeros_like(depth))
        for _ in range(CALLS):
            c.remove_object(o, d, m, art, z, rows, cols, rt.Removal(0, grow, 0.0))
        c.synchronize()


def report(pairs):
    print(f"# kernel trace, 1080p, {CALLS} calls each: per kernel the mean (min) us, in launch order of a call")
    for pair in pairs:
        label, path = pair.split("=", 1)
        db = sqlite3.connect(path)
        rows = db.execute("select name, count(*), avg(end - start) / 1000.0, min(end - start) / 1000.0, min(start) from kernels "
                          "where name like '%rtdd::k_remove%' group by name order by 5").fetchall()
        total = sum(r[2] for r in rows)
        print(f"{label}: sum of the means {total:.1f} us")
        for name, n, mean, lo, _ in rows:
            short = name.replace("void ", "").replace("rtdd::", "").split("(")[0]
            print(f"    {short:42s} {n:3d} calls  {mean:6.1f} ({lo:.1f})")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "report":
        report(sys.argv[2:])
    else:
        sys.exit(__doc__)
