"""The shapes, masks and reaches that tests/test_gpu_mask_distance.py runs the kernels on and tests/test_mask_distance_cpu.py checks the
reference on: derived from the geometry realtimedepthdiffusion_amd exports (importable without a GPU), the smallest at which a pass of
csrc/mask_distance.hip can go wrong.  A plain module -- no fixtures, no pytest settings."""
import numpy as np

import mask_distance_ref as mr
from realtimedepthdiffusion_amd import EDT_BAND, EDT_LDS_REACH, EDT_TILE_H, EDT_TILE_W
from remove_ref import CODE, OTHER, mask_pattern

W, H, B, L = EDT_TILE_W, EDT_TILE_H, EDT_BAND, EDT_LDS_REACH
# tiny; one tile and one more each way; one band of the column pass, two and a row; the widest row segment LDS stages and a column; many
SHAPES = [(1, 1), (1, 7), (9, 1), (37, 53), (H, W), (H + 1, W + 1), (B, 70), (2 * B + 1, 70), (9, W + 2 * L + 1), (257, 513)]
MASKS = ["empty", "full", "corners", "edges", "random50", "random1", "checker", "disc", "borders", "allbut", "random"]
REACHES = [1, 2, 5, 63, 64, 65, L, L + 1, 1024]
SELECTS = [0, CODE]
# the reaches at which an "edges" mask is built: REACHES, and 6, which the refine tests' thresholds 26 derive
EDGE_REACHES = sorted(set(REACHES) | {6})


def make_mask(name, rows, cols, reach):
    """The issue's masks.  "edges": single pixels 0, 1, reach - 1, reach and reach + 1 away from the first tile border (x: W, y: H) and
    the first band border (y: B), on both sides, in x and in y.  Every mask but the empty and the full one also carries OTHER pixels: selected
    with the rest under select = 0, not selected under select = CODE."""
    rng = np.random.default_rng(rows * 1000 + cols)
    if name == "empty":
        return np.zeros((rows, cols), np.uint8)
    if name == "full":
        return np.full((rows, cols), CODE, np.uint8)
    if name == "corners":
        m = mr.single_pixels(rows, cols, [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)], CODE)
    elif name == "edges":
        m = np.zeros((rows, cols), np.uint8)
        for i, k in enumerate((0, 1, reach - 1, reach, reach + 1)):
            for p in (W - 1 - k, W + k):
                if 0 <= p < cols:
                    m[(5 + 7 * i) % rows, p] = CODE
            for p in (H - 1 - k, H + k, B - 1 - k, B + k):
                if 0 <= p < rows:
                    m[p, (9 + 11 * i) % cols] = CODE
    elif name == "random50":
        m = np.where(rng.random((rows, cols)) < 0.5, CODE, 0).astype(np.uint8)
    elif name == "random1":
        m = np.where(rng.random((rows, cols)) < 0.01, CODE, 0).astype(np.uint8)
    else:
        m = mask_pattern(name, rows, cols, seed=2)
    m[rows // 3, cols // 3] = OTHER
    return m
