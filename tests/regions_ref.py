"""Restatement of the depth regions (include/rtdd.h, rtdd_solve_regions) in whole-array numpy (test infrastructure).

The rule works on the index maps the existing rule gives (np_restatement.index_maps for the gray guide, color_guide_ref.index_maps_bgr for
the colour one: guide, then gate): for two 4-neighbours p, q inside the image with region codes rp, rq (u8, 0 = unassigned)

    CUT set and rp != rq              -> 255
    else SMOOTH set and rp == rq != 0 -> 0
    else                              -> the index as it was

and outside the image the index stays 256.  The sweeps are np_restatement's.  The codes of pyramid level l are the level-0 codes sampled
at (y << l, x << l), and a level-0 code is the label where the mask says painted (255), else 0."""
import numpy as np

import np_restatement as npr
from color_guide_ref import BGR, GRAY, ColorCascade, index_maps_bgr

CUT, SMOOTH = 1, 2


def index_maps_regions(maps, codes, flags):
    """New left/right/up/down maps: the rule applied on top of `maps` (which is not modified)."""
    r = np.asarray(codes).astype(np.int32)
    out = {k: v.copy() for k, v in maps.items()}
    if flags == 0:
        return out

    def rule(i, rp, rq):
        cut = (rp != rq) if flags & CUT else np.zeros(rp.shape, bool)
        smooth = ((rp == rq) & (rp != 0)) if flags & SMOOTH else np.zeros(rp.shape, bool)
        return np.where(cut, 255, np.where(smooth, 0, i)).astype(np.int32)

    h = rule(maps["left"][:, 1:], r[:, 1:], r[:, :-1])      # the edge between x - 1 and x (left of x is right of x - 1: the rule is symmetric)
    v = rule(maps["up"][1:, :], r[1:, :], r[:-1, :])
    assert np.array_equal(maps["left"][:, 1:], maps["right"][:, :-1]) and np.array_equal(maps["up"][1:, :], maps["down"][:-1, :])
    out["left"][:, 1:] = h; out["right"][:, :-1] = h
    out["up"][1:, :] = v; out["down"][:-1, :] = v
    return out


def base_maps(guide, guide_kind, depth, level, max_level):
    return index_maps_bgr(guide, depth, level, max_level) if guide_kind == BGR else npr.index_maps(guide, depth, level, max_level)


def solve_maps(depth, mask, maps, iters, lut, contract):
    """np_restatement.solve on given index maps; returns the result (depth is not modified)."""
    x = depth.astype(np.float32).copy()
    prev = np.zeros_like(x)
    for om in npr.omega_schedule(iters):
        x, prev = npr.sweep(x, maps, mask, prev, om, lut, contract)
    return x


def solve_regions(depth, mask, guide, guide_kind, codes, flags, iters, level, max_level, lut, contract):
    maps = index_maps_regions(base_maps(guide, guide_kind, depth, level, max_level), codes, flags)
    return solve_maps(depth, mask, maps, iters, lut, contract)


def region_codes(edited, mask, level):
    """The codes of pyramid level `level` (floor(rows / 2^level) x floor(cols / 2^level)) of a level-0 region pair."""
    code0 = np.where(mask == 255, edited[..., 0], 0).astype(np.uint8)
    rows, cols = code0.shape
    return np.ascontiguousarray(code0[::1 << level, ::1 << level][:rows >> level, :cols >> level])


class RegionCascade(ColorCascade):
    """color_guide_ref.ColorCascade (either guide) whose per-level solve applies `flags` with level l's codes of the region pair
    (region_edited, region_mask: level 0, what the paint calls write).  flags 0: ColorCascade's own estimate."""

    def __init__(self, oracle, bgr, annotation, lut, contract=1, threads=1, guide=GRAY, flags=0):
        super().__init__(oracle, bgr, annotation, lut, contract, threads, guide)
        self.flags = flags
        rows, cols = bgr.shape[:2]
        self.region_edited = np.zeros((rows, cols, 3), np.uint8)
        self.region_mask = np.zeros((rows, cols), np.uint8)

    def codes(self, l):
        return region_codes(self.region_edited, self.region_mask, l)

    def estimate(self, max_iterations=1000):
        if self.flags == 0:
            return super().estimate(max_iterations)
        o, P = self.o, self.P
        for l in range(1, P):
            o.pyrdown_annotation(self.scribble[l - 1], self.edited[l - 1], self.scribble[l], self.edited[l])
        o.convert_to_float(self.edited[P - 1], self.depth[P - 1], self.scribble[P - 1])
        for l in range(P - 1, -1, -1):
            iters = int(np.float32(max_iterations) / np.float32(2.0) ** ((P - 1) - l))
            r, c = self.size[l]
            if r > 0 and c > 0:
                guide = self.color[l][:r, :c] if self.guide == BGR else self.gray[l][:r, :c]
                assert self.codes(l).shape == (r, c)
                self.depth[l] = solve_regions(self.depth[l], self.scribble[l], guide, self.guide, self.codes(l), self.flags, iters, l, P - 1,
                                              self.lut, self.contract)
            if l > 0:
                self.depth[l - 1] = o.pyrup_f32(self.depth[l], *self.size[l - 1], contract=self.contract)
                o.convert_to_float(self.edited[l - 1], self.depth[l - 1], self.scribble[l - 1])
        self.depth_u8 = o.depth_to_u8(self.depth[0])
        return self.depth[0]
