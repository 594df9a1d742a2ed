"""Restatement of the colour-guided edge weights (include/rtdd.h, rtdd_solve_guided) in whole-array numpy (test infrastructure).

The rule: for two 4-neighbours p, q of a BGR guide, index(p, q) = max(|B_p - B_q|, |G_p - G_q|, |R_p - R_q|), an integer in [0, 255];
256 outside the image; where level != max_level the index is 0 unless the saturated u8 depths of p and q differ by more than the
threshold (0 on level 0, 4 otherwise).  The sweeps are np_restatement's, which tests/test_oracle.py pins against the oracle; the colour
pyramid is oracle.pyrdown_u8 applied to each channel plane (cv::pyrDown filters channels independently)."""
import numpy as np

import np_restatement as npr
from cascade_ref import Cascade

GRAY, BGR = 0, 1


def index_maps_bgr(bgr, depth, level, max_level):
    """left/right/up/down index maps (int32, 256 = no neighbour) of a rows x cols x 3 guide."""
    c = bgr.astype(np.int32)
    rows, cols = c.shape[:2]
    gh = np.abs(c[:, 1:] - c[:, :-1]).max(axis=2)        # between x - 1 and x: the largest channel difference
    gv = np.abs(c[1:, :] - c[:-1, :]).max(axis=2)        # between y - 1 and y
    if level != max_level:
        with np.errstate(invalid="ignore"):
            d = np.trunc(np.clip(np.nan_to_num(depth.astype(np.float64), nan=0.0, posinf=255.0, neginf=0.0), 0, 255)).astype(np.int32)
        thr = 0 if level == 0 else 4
        gh = np.where(np.abs(d[:, 1:] - d[:, :-1]) > thr, gh, 0)
        gv = np.where(np.abs(d[1:, :] - d[:-1, :]) > thr, gv, 0)
    out = {k: np.full((rows, cols), 256, np.int32) for k in ("left", "right", "up", "down")}
    out["left"][:, 1:] = gh
    out["right"][:, :-1] = gh
    out["up"][1:, :] = gv
    out["down"][:-1, :] = gv
    return out


def solve_bgr(depth, mask, bgr, iters, level, max_level, lut, contract):
    """np_restatement.solve with the indices of the colour rule; returns the result (depth is not modified)."""
    maps = index_maps_bgr(bgr, depth, level, max_level)
    x = depth.astype(np.float32).copy()
    prev = np.zeros_like(x)
    for om in npr.omega_schedule(iters):
        x, prev = npr.sweep(x, maps, mask, prev, om, lut, contract)
    return x


def color_chain(oracle, bgr, levels):
    """Level 0 is the image; level l is pyrDown of level l - 1, channel by channel (the ceil-sized chain of the gray pyramid)."""
    chain = [np.ascontiguousarray(bgr)]
    for _ in range(1, levels):
        prev = chain[-1]
        chain.append(np.stack([oracle.pyrdown_u8(prev[..., ch].copy()) for ch in range(3)], axis=-1))
    return chain


class ColorCascade(Cascade):
    """cascade_ref.Cascade whose per-level solve is solve_bgr on the colour chain while `guide` is BGR (GRAY: Cascade's own solve); the
    guide may be changed between estimates, which continue from each other's depth pyramid as the library's do."""

    def __init__(self, oracle, bgr, annotation, lut, contract=1, threads=1, guide=BGR):
        super().__init__(oracle, bgr, annotation, lut, contract, threads)
        self.guide = guide
        self.color = color_chain(oracle, bgr, self.P)

    def estimate(self, max_iterations=1000):
        if self.guide == GRAY:
            return super().estimate(max_iterations)
        o, P = self.o, self.P
        for l in range(1, P):
            o.pyrdown_annotation(self.scribble[l - 1], self.edited[l - 1], self.scribble[l], self.edited[l])
        o.convert_to_float(self.edited[P - 1], self.depth[P - 1], self.scribble[P - 1])
        for l in range(P - 1, -1, -1):
            iters = int(np.float32(max_iterations) / np.float32(2.0) ** ((P - 1) - l))
            r, c = self.size[l]
            if r > 0 and c > 0:
                self.depth[l] = solve_bgr(self.depth[l], self.scribble[l], self.color[l][:r, :c], iters, l, P - 1, self.lut, self.contract)
            if l > 0:
                self.depth[l - 1] = o.pyrup_f32(self.depth[l], *self.size[l - 1], contract=self.contract)
                o.convert_to_float(self.edited[l - 1], self.depth[l - 1], self.scribble[l - 1])
        self.depth_u8 = o.depth_to_u8(self.depth[0])
        return self.depth[0]


# ---- the isoluminant pair of the issue: two colours the reference cannot tell apart -----------------------------------------------------
GREEN, RED = (0, 100, 0), (0, 0, 196)         # (B, G, R): both give gray 59 under cv::cvtColor's fixed-point rule


def isoluminant_image(rows, cols):
    """Left half GREEN, right half RED."""
    img = np.empty((rows, cols, 3), np.uint8)
    img[:, :cols // 2] = GREEN
    img[:, cols // 2:] = RED
    return img
