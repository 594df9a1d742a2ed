"""realtimedepthdiffusion_amd -- host-side Python mirror of librtdd.so's C ABI.

The product is the HIP library (csrc/ -> librtdd.so, declared in include/rtdd.h).  This
module is plumbing: it loads the library with ctypes and mirrors the reference's interface
for the hot path -- the ten ``GPU*`` functions of /root/reference/include/GPUSolver.h:6-10,
GPUImageProcessing.h:4-10 and GPUDepthEffect.h:4-9 -- with the same names, argument order
and meaning, so parity tests read like calls into the reference.  Image arguments are
*pitched device buffers*: anything with ``data_ptr()`` and ``stride()`` (a torch CUDA tensor
whose rows may be padded) or an explicit ``(ptr, pitch_bytes)`` pair.

There is NO CPU fallback: if librtdd.so is missing or no HIP device is present every entry
point raises.  Nothing here imports ``oracle``.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("RTDD_LIBRARY") or os.path.join(_HERE, "librtdd.so")     # RTDD_LIBRARY: developer knob for A/B builds (scripts/build_variant.sh)
_CSRC = os.path.join(_HERE, "csrc")

RTDD_OK = 0
METHOD_CHEBYSHEV_JACOBI = 0
METHOD_RED_BLACK_GS = 1
METHOD_MULTIGRID = 2
METHOD_AUTO = 3
RELAXATION_AUTO = -1.0                     # rtdd_solve_params.relaxation: SOR cycles (include/rtdd.h)
OPT_FP_CONTRACT, OPT_SWEEP_KERNEL, OPT_TEMPORAL_DEPTH, OPT_DEFOCUS_PATH, OPT_ROWS_PER_WAVE, OPT_TILE, OPT_PERSISTENT = 0, 1, 2, 3, 4, 5, 6
OPT_DEBUG_WITHHOLD_TILE, OPT_DEBUG_POLL_LIMIT_US = 7, 8
OPT_AUTO_CYCLE_FIXED_NS, OPT_AUTO_CYCLE_FS_PER_PX, OPT_AUTO_SWEEP_FS_PER_PX, OPT_AUTO_SWEEP_FLOOR_NS = 9, 10, 11, 12
OPT_DEBUG_FORCE_STATUS = 13
OPT_TIMEOUT_HEALS = 14                     # read only
OPT_DEFOCUS_LAST_PATH = 15                 # read only: 1 the global table, 2 the tile kernel
OPT_TIMEOUT_HEAL, OPT_PERSISTENT_REARM_AFTER, OPT_PERSISTENT_SUSPENDED, OPT_PENDING_CALLS = 16, 17, 18, 19
OPT_LIVE_ZERO_COPY = 20
OPT_ANNOTATION_LDS = 21
OPT_DEFOCUS_STRIPS = 22
OPT_DEFOCUS_LAST_SLICES = 23              # read only
OPT_DEFOCUS_SLICE_MB = 24
RTDD_ERR_TIMEOUT = 6

# every symbol include/rtdd.h declares (checked by tests/test_abi.py against the header)
C_ABI_SYMBOLS = [
    "rtdd_ctx_create", "rtdd_ctx_destroy", "rtdd_ctx_set_stream", "rtdd_ctx_synchronize", "rtdd_set_option",
    "rtdd_get_option", "rtdd_last_error", "rtdd_status_string", "rtdd_version", "rtdd_allocate", "rtdd_free",
    "rtdd_load_weights", "rtdd_matrix_free_solver", "rtdd_solve_ex", "rtdd_last_solve_info", "rtdd_scaled_mode_waves", "rtdd_multigrid_level", "rtdd_index_to_weight", "rtdd_convert_to_float",
    "rtdd_pyrdown_annotation", "rtdd_paint_image", "rtdd_simulate_defocus", "rtdd_simulate_desaturation",
    "rtdd_simulate_haze", "rtdd_profile_enable", "rtdd_profile_get",
    "rtdd_pyramid_levels", "rtdd_pyramid_create", "rtdd_pyramid_destroy", "rtdd_pyramid_set_image",
    "rtdd_pyramid_set_annotation", "rtdd_pyramid_image", "rtdd_pyramid_annotation_changed", "rtdd_estimate_depth", "rtdd_refine_depth", "rtdd_bgr2gray", "rtdd_pyrdown_gray",
    "rtdd_pyrup_depth", "rtdd_depth_to_u8", "rtdd_upload", "rtdd_download",
    "rtdd_live_submit", "rtdd_live_wait", "rtdd_live_pending", "rtdd_host_alloc", "rtdd_host_free",
    "rtdd_pyramid_create_batch", "rtdd_pyramid_select", "rtdd_pyramid_batch", "rtdd_estimate_depth_batch", "rtdd_pyramid_level_info", "rtdd_live_submit_ex",
    "rtdd_simulate_refocus", "rtdd_simulate_haze_ex", "rtdd_simulate_stereo", "rtdd_simulate_lens_blur",
    "rtdd_paint_strokes", "rtdd_pyramid_annotation_rebuild", "rtdd_paint_ramp_strokes", "rtdd_ramp_polyline", "rtdd_fill_polygon", "rtdd_fill_similar", "rtdd_fill_surface", "rtdd_segment_surfaces",
    "rtdd_simulate_relight", "rtdd_simulate_relight_shadowed", "rtdd_simulate_parallax", "rtdd_simulate_ambient_occlusion",
    "rtdd_simulate_lighting", "rtdd_simulate_bokeh", "rtdd_composite_layer", "rtdd_remove_object", "rtdd_lift_layer",
    "rtdd_simulate_parallax_layered", "rtdd_mask_distance", "rtdd_refine_mask", "rtdd_lift_layer_matte",
    "rtdd_solve_guided", "rtdd_index_to_weight_guided", "rtdd_pyrdown_bgr", "rtdd_pyramid_set_guide", "rtdd_pyramid_guide",
    "rtdd_solve_regions", "rtdd_index_to_weight_regions", "rtdd_region_codes", "rtdd_pyramid_set_regions", "rtdd_pyramid_regions",
    "rtdd_pyramid_regions_changed",
]
IMG_ORIGINAL, IMG_GRAY, IMG_SCRIBBLE, IMG_EDITED, IMG_DEPTH, IMG_DEPTH_U8, IMG_ARTISTIC, IMG_GUIDE_BGR = range(8)
IMG_REGION_EDITED, IMG_REGION_MASK, IMG_REGION_CODE = 8, 9, 10    # the depth regions' level-0 pair and per-level codes (rtdd_pyramid_set_regions)
REGION_CUT, REGION_SMOOTH = 1, 2              # rtdd_region_flags: edges between different codes are cut, edges inside one region are smoothed
GUIDE_GRAY, GUIDE_BGR = 0, 1                  # rtdd_guide: what the edge weights are read from (rtdd_solve_guided, rtdd_pyramid_set_guide)
EFFECT_NONE, EFFECT_DEFOCUS, EFFECT_DESATURATION, EFFECT_HAZE = range(4)
STEREO_VIEW, STEREO_ANAGLYPH = 0, 1           # rtdd_simulate_stereo's modes
APERTURE_BOX, APERTURE_DISC = 0, 1            # rtdd_simulate_lens_blur's shapes
LIGHT_DIRECTIONAL, LIGHT_POINT = 0, 1         # rtdd_light.kind
AO_SHADE, AO_MAP = 0, 1                       # rtdd_ambient_occlusion.mode
LAYER_NEAREST, LAYER_BILINEAR = 0, 1          # rtdd_layer.filter
BRUSH_SQUARE, BRUSH_ROUND = 0, 1              # rtdd_stroke.brush
STROKE_ERASE = -1                             # rtdd_stroke.label: remove the annotation
FILL_NONZERO, FILL_EVEN_ODD = 0, 1            # rtdd_fill.rule
WAND_CONNECT_8, WAND_GLOBAL = 1, 2            # rtdd_wand.flags
SURFACE_GLOBAL = 1                            # rtdd_surface_wand.flags
SEGMENT_TILE_W, SEGMENT_TILE_H = 64, 16       # the tile rtdd_segment_surfaces labels in LDS before it merges across borders (csrc/segment.hip: kPaintTileW, kPaintTileH)
SEGMENT_HEAD = 1024                           # candidates it reads back with the counters; more take a second copy (csrc/segment.hip: kSegHead)
WAND_ROUND = 8                                # grow passes rtdd_fill_similar queues between two synchronisations (csrc/fill_similar.hip: kWandRound)
# rtdd_remove_object's grouping (csrc/rtdd_internal.hpp: kRemoveTile, kRemoveGroup, kRemoveApex, kRemoveApexChain): a workgroup owns a
# REMOVE_TILE-square tile of a level and takes REMOVE_GROUP levels in LDS; one workgroup takes a level of at most REMOVE_APEX samples
# (its chain up to 1 x 1 at most REMOVE_APEX_CHAIN) to the top and back
REMOVE_TILE, REMOVE_GROUP, REMOVE_APEX = 64, 3, 8192
REMOVE_APEX_CHAIN = REMOVE_APEX + REMOVE_APEX // 2 + 64


def remove_plan(rows, cols):
    """The levels rtdd_remove_object stores for a rows x cols image (csrc/remove.hip remove_plan): [(levels taken, rows, cols of the level
    stored), ...], one entry per pull group; the apex takes the last.  2 * len + 1 launches."""
    def chain(r, c):
        n = r * c
        while r > 1 or c > 1:
            r, c = (r + 1) // 2, (c + 1) // 2
            n += r * c
        return n
    plan, r, c = [], rows, cols
    while True:
        g = 0
        while g < REMOVE_GROUP and (r > 1 or c > 1):
            r, c, g = (r + 1) // 2, (c + 1) // 2, g + 1
        plan.append((g, r, c))
        if r * c <= REMOVE_APEX and chain(r, c) <= REMOVE_APEX_CHAIN:
            return plan


# rtdd_mask_distance / rtdd_refine_mask (csrc/rtdd_internal.hpp: kEdtTileW, kEdtTileH, kEdtBand, kEdtLdsReach): the column pass works on
# words of EDT_BAND rows of a column and flags blocks of EDT_TILE_W columns; a workgroup of the row pass owns EDT_TILE_W x EDT_TILE_H
# pixels and stages a row segment with its halo in LDS up to a reach of EDT_LDS_REACH
EDT_TILE_W, EDT_TILE_H, EDT_BAND, EDT_LDS_REACH = 64, 4, 64, 224
REFINE_GROW, REFINE_SHRINK, REFINE_OUTLINE, REFINE_FEATHER = range(4)    # rtdd_mask_refine.op
DISTANCE_FAR = 0x7FFFFFFF                     # rtdd_mask_distance: |dist2| of a pixel whose E lies beyond the reach


def mask_distance_plan(rows, cols, reach):
    """What rtdd_mask_distance does for a rows x cols mask at `reach` (csrc/mask_distance.hip edt_plan and launch_rows): the row pass's
    path ("lds": the halo is staged; "l2": read through the caches), the bands of the column pass and how many neighbouring words a carry
    may read each way, the blocks of columns, the row pass's grid and the u32 words of the table buffer."""
    bands, blocks = (rows + EDT_BAND - 1) // EDT_BAND, (cols + EDT_TILE_W - 1) // EDT_TILE_W
    return dict(path="lds" if reach <= EDT_LDS_REACH else "l2", bands=bands, blocks=blocks, carry_words=(reach + EDT_BAND - 1) // EDT_BAND,
                grid=(blocks, (rows + EDT_TILE_H - 1) // EDT_TILE_H), words=2 * bands * cols + rows * cols + rows * blocks)


def refine_reach(op, inner2=0, outer2=0, lo=0.0, hi=0.0):
    """The reach rtdd_refine_mask derives on the host (include/rtdd.h): the smallest R with R^2 >= the largest threshold the op reads, or
    for the feather the smallest integer R >= max(|lo|, |hi|) + 0.5."""
    import math
    if op == REFINE_FEATHER:
        return math.ceil(max(abs(lo), abs(hi)) + 0.5)
    most = {REFINE_GROW: outer2, REFINE_SHRINK: inner2}.get(op, max(inner2, outer2))
    return max(1, math.isqrt(max(most - 1, 0)) + 1 if most > 0 else 1)


# Itanium-mangled names of the reference's ten free functions
DROPIN_SYMBOLS = [
    "_Z23GPUAllocateDeviceMemoryiii", "_Z19GPUFreeDeviceMemoryi", "_Z14GPULoadWeightsf",
    "_Z19GPUMatrixFreeSolverPfmPhmS0_miififi", "_Z17GPUConvertToFloatPhmPfmS_mii",
    "_Z20GPUPyrDownAnnotationPhmS_miiS_mS_mii", "_Z13GPUPaintImageiiiiPhmS_mii",
    "_Z18GPUSimulateDefocusPhmPfmS_mii", "_Z23GPUSimulateDesaturationPhmS_mPfmS_mii", "_Z15GPUSimulateHazePhmPfmS_mii",
]


class RtddError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"rtdd status {status}: {message}")
        self.status = status


class SolveParams(C.Structure):
    _fields_ = [("method", C.c_int), ("maxIterations", C.c_int), ("tolerance", C.c_float), ("checkEvery", C.c_int), ("relaxation", C.c_float)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("residual", C.c_float), ("cycles", C.c_int), ("kernel", C.c_int), ("tile", C.c_int),
                ("temporal_depth", C.c_int), ("persistent", C.c_int), ("fp_contract", C.c_int), ("launches", C.c_int)]

    def describe(self):
        return (f"kernel {self.kernel} tile {self.tile} depth {self.temporal_depth} persistent {self.persistent} contract {self.fp_contract} "
                f"launches {self.launches} iterations {self.iterations} cycles {self.cycles} residual {self.residual:.3g}")


class Stroke(C.Structure):
    """rtdd_stroke: the segment (x0, y0)-(x1, y1), `radius` (the reference's scribbleRadius: a diameter), BRUSH_*, label 0..255 or STROKE_ERASE."""
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("radius", C.c_int), ("brush", C.c_int), ("label", C.c_int)]


class RampStroke(C.Structure):
    """rtdd_ramp_stroke: a Stroke whose label runs linearly from label0 at (x0, y0) to label1 at (x1, y1) (both STROKE_ERASE: an eraser)."""
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("radius", C.c_int), ("brush", C.c_int),
                ("label0", C.c_int), ("label1", C.c_int)]


class Fill(C.Structure):
    """rtdd_fill: FILL_*, the ramp's axis (label0 at (ax0, ay0), label1 at (ax1, ay1); ignored when the labels are equal), the two labels
    (both STROKE_ERASE: the polygon erases)."""
    _fields_ = [("rule", C.c_int), ("ax0", C.c_int), ("ay0", C.c_int), ("ax1", C.c_int), ("ay1", C.c_int), ("label0", C.c_int), ("label1", C.c_int)]


class Wand(C.Structure):
    """rtdd_wand: the clicked pixel (x, y), the tolerance 0..255, WAND_* flags, and rtdd_fill's axis and two labels (both STROKE_ERASE: the
    selection is erased)."""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("tolerance", C.c_int), ("flags", C.c_int), ("ax0", C.c_int), ("ay0", C.c_int), ("ax1", C.c_int),
                ("ay1", C.c_int), ("label0", C.c_int), ("label1", C.c_int)]


class SurfaceWand(C.Structure):
    """rtdd_surface_wand: the clicked pixel (x, y), the largest depth step between two joined neighbours, the band [ds - below, ds + above]
    around the clicked depth ds (255: no limit on that side), SURFACE_* flags, and rtdd_fill's axis and two labels."""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("step", C.c_float), ("below", C.c_float), ("above", C.c_float), ("flags", C.c_int),
                ("ax0", C.c_int), ("ay0", C.c_int), ("ax1", C.c_int), ("ay1", C.c_int), ("label0", C.c_int), ("label1", C.c_int)]


class WandInfo(C.Structure):
    """rtdd_wand_info: the covered pixels, their inclusive bounding box, and the grow passes that ran (a diagnostic: not deterministic)."""
    _fields_ = [("pixels", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("passes", C.c_int)]


class Segmentation(C.Structure):
    """rtdd_segmentation: the largest depth step between two joined neighbours, the absolute band [lo, hi] of depths that take part, the
    smallest component that is a candidate, the number of regions wanted (1..255), the first region's code, flags (0)."""
    _fields_ = [("step", C.c_float), ("lo", C.c_float), ("hi", C.c_float), ("minPixels", C.c_int), ("maxRegions", C.c_int), ("firstCode", C.c_int),
                ("flags", C.c_int)]


class Segment(C.Structure):
    """rtdd_segment: a region's code, size, root, inclusive bounding box and the smallest and largest clamped depth in it."""
    _fields_ = [("code", C.c_int), ("pixels", C.c_int), ("rootX", C.c_int), ("rootY", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int),
                ("y1", C.c_int), ("dmin", C.c_float), ("dmax", C.c_float)]


class SegmentInfo(C.Structure):
    """rtdd_segment_info: all components, those of at least minPixels pixels, the regions numbered, and the pixels in them."""
    _fields_ = [("components", C.c_int), ("candidates", C.c_int), ("regions", C.c_int), ("pixels", C.c_int)]


def ramp_polyline(points, radius, brush, label0, label1):
    """rtdd_ramp_polyline: the points [(x, y), ...] of a drag as a list of 8-tuples (x0, y0, x1, y1, radius, brush, label0, label1) for
    Context.paint_ramp_strokes, the labels spread from label0 to label1 by arc length.  Host arithmetic: needs no context and no device."""
    n = len(points)
    xy = (C.c_int * max(2 * n, 1))(*[int(v) for p in points for v in p])
    out = (RampStroke * max(n - 1, 1))()
    rc = lib().rtdd_ramp_polyline(xy, C.c_int(n), C.c_int(radius), C.c_int(brush), C.c_int(label0), C.c_int(label1), out)
    if rc != RTDD_OK:
        raise RtddError(rc, lib().rtdd_status_string(rc).decode() + " -- rtdd_ramp_polyline")
    return [(q.x0, q.y0, q.x1, q.y1, q.radius, q.brush, q.label0, q.label1) for q in out]


class Light(C.Structure):
    """rtdd_light: LIGHT_DIRECTIONAL with (x, y, z) the direction towards the light, or LIGHT_POINT at pixel (x, y), z pixels above the
    surface point of depth `anchorDepth` or (anchorX >= 0) of the depth map's value at (anchorX, anchorY), read on the device; `radius`
    the distance of half intensity; `relief` pixels of height per unit of depth; gain = ambient + diffuse * colour * shade."""
    _fields_ = [("kind", C.c_int), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("anchorDepth", C.c_float),
                ("anchorX", C.c_int), ("anchorY", C.c_int), ("radius", C.c_float), ("relief", C.c_float), ("ambient", C.c_float),
                ("diffuse", C.c_float), ("colorB", C.c_uint8), ("colorG", C.c_uint8), ("colorR", C.c_uint8)]

    def __init__(self, kind=LIGHT_DIRECTIONAL, x=0.0, y=0.0, z=1.0, anchorDepth=0.0, anchorX=-1, anchorY=-1, radius=1.0, relief=1.0,
                 ambient=0.0, diffuse=1.0, color=(255, 255, 255)):
        b, g, r = color
        super().__init__(kind, x, y, z, anchorDepth, anchorX, anchorY, radius, relief, ambient, diffuse, b, g, r)


class Shadow(C.Structure):
    """rtdd_shadow: every pixel marches up to `maxSteps` pixels towards the light (0: no shadows) from `bias` above the surface;
    `softness` 0 gives hard shadows, > 0 a penumbra that widens with the blocker's distance; `strength` is the share of the diffuse
    term a full shadow removes."""
    _fields_ = [("maxSteps", C.c_int), ("bias", C.c_float), ("softness", C.c_float), ("strength", C.c_float)]

    def __init__(self, maxSteps=256, bias=0.0, softness=0.0, strength=1.0):
        super().__init__(maxSteps, bias, softness, strength)


class Parallax(C.Structure):
    """rtdd_parallax: the camera moved by (shiftX, shiftY) -- pixels of shift of a point 255 depth units behind the zero-parallax depth --
    and forward by `dolly` (< 0: back); zero parallax at `zeroParallaxDepth` or (zeroX >= 0) at the depth map's value at (zeroX, zeroY),
    read on the device."""
    _fields_ = [("shiftX", C.c_int), ("shiftY", C.c_int), ("dolly", C.c_float), ("zeroParallaxDepth", C.c_float), ("zeroX", C.c_int),
                ("zeroY", C.c_int)]

    def __init__(self, shiftX=0, shiftY=0, dolly=0.0, zeroParallaxDepth=0.0, zeroX=-1, zeroY=-1):
        super().__init__(shiftX, shiftY, dolly, zeroParallaxDepth, zeroX, zeroY)


class AmbientOcclusion(C.Structure):
    """rtdd_ambient_occlusion: the horizon of the height field relief * (255 - depth) along `directions` (4 or 8) compass directions
    over `radius` pixels (0: no occlusion); a horizon counts once it clears `bias`; `strength` is the share of the ambient light a fully
    occluded pixel loses.  mode AO_SHADE darkens the original (or, under a light, relight's ambient term), AO_MAP renders the occlusion
    itself as a gray image.  Under a light `relief` must be the light's."""
    _fields_ = [("mode", C.c_int), ("directions", C.c_int), ("radius", C.c_int), ("relief", C.c_float), ("bias", C.c_float),
                ("strength", C.c_float)]

    def __init__(self, mode=AO_SHADE, directions=8, radius=16, relief=1.0, bias=0.0, strength=1.0):
        super().__init__(mode, directions, radius, relief, bias, strength)


class Layer(C.Structure):
    """rtdd_layer: a sprite of rows x cols texels whose top-left corner lands at image pixel (x, y), `scale` / 256 pixels per texel,
    LAYER_NEAREST or LAYER_BILINEAR, `opacity` 0..255; its depth is a plane, depth0 at (x0, y0) and depth1 at (x1, y1) (the same point:
    the constant depth0); `feather` is the depth interval over which the scene takes over from the layer (0: a hard edge)."""
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("x", C.c_int), ("y", C.c_int), ("scale", C.c_int), ("filter", C.c_int),
                ("opacity", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("depth0", C.c_float),
                ("depth1", C.c_float), ("feather", C.c_float)]

    def __init__(self, rows=1, cols=1, x=0, y=0, scale=256, filter=LAYER_NEAREST, opacity=255, x0=0, y0=0, x1=0, y1=0, depth0=0.0,
                 depth1=0.0, feather=0.0):
        super().__init__(rows, cols, x, y, scale, filter, opacity, x0, y0, x1, y1, depth0, depth1, feather)


class Removal(C.Structure):
    """rtdd_removal: a pixel is selected iff its mask byte != 0 (`select` 0) or == select (1..255, a region code); the hole also takes
    the eligible pixels within Chebyshev distance `grow` (0..8) of a selected one; only pixels at least `sourceMinDepth` far are sources
    of the fill (0: every pixel)."""
    _fields_ = [("select", C.c_int), ("grow", C.c_int), ("sourceMinDepth", C.c_float)]

    def __init__(self, select=0, grow=0, sourceMinDepth=0.0):
        super().__init__(select, grow, sourceMinDepth)


class MaskRefine(C.Structure):
    """rtdd_mask_refine: `select` as Removal's; REFINE_GROW (out to squared distance outer2), REFINE_SHRINK (in by inner2),
    REFINE_OUTLINE (the selected pixels within inner2 of the boundary and the unselected ones within outer2; 0: that side is empty) or
    REFINE_FEATHER (255 at `lo` pixels from the boundary, 0 at `hi`, linear between; negative is inside)."""
    _fields_ = [("select", C.c_int), ("op", C.c_int), ("inner2", C.c_int), ("outer2", C.c_int), ("lo", C.c_float), ("hi", C.c_float)]

    def __init__(self, select=0, op=REFINE_GROW, inner2=0, outer2=0, lo=0.0, hi=0.0):
        super().__init__(select, op, inner2, outer2, lo, hi)


class Profile(C.Structure):
    _fields_ = [("sweep_ms", C.c_double), ("launches", C.c_int), ("sweeps", C.c_int),
                ("prepare_ms", C.c_double), ("finish_ms", C.c_double)]


def build(force=False):
    """Compile librtdd.so for gfx950 (hipcc cross-compiles without a GPU).

    The persistent kernels' hand-off reads its halo with sc1 loads and NO agent-scope acquire; that is only right if the compiler put
    nothing between those loads and the wait behind them (csrc/sweep_common.hpp).  scripts/isa_check.py checks exactly that on the
    objects just built -- every path, spills included.  If the check fails, or cannot run (no llvm-objdump), the two kernels are
    rebuilt with -DRTDD_EXCHANGE_ACQUIRE=1 (one acquire per exchange, plain loads: ~0.8 us per exchange slower, no such dependence) and
    a warning says so: a compiler bump can cost speed, never silently a wrong depth map."""
    import sys
    args = ["make", "-C", _CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    stamp = os.path.join(_CSRC, ".exchange_variant")
    try:
        sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "scripts"))
        import isa_check
        isa_check.check_build(_CSRC)
        variant = "sc1"
    except Exception as e:      # AssertionError (the check failed), FileNotFoundError (no objdump), ...
        already = os.path.exists(stamp) and open(stamp).read().strip() == "acquire" and os.path.getmtime(stamp) >= os.path.getmtime(os.path.join(_CSRC, "sweep_blocked.o"))
        if not already:
            print(f"[rtdd build] the structural check of the no-acquire hand-off did not pass ({type(e).__name__}: {e}): rebuilding the persistent "
                  "kernels with -DRTDD_EXCHANGE_ACQUIRE=1", file=sys.stderr)
            for f in ("sweep_blocked.o", "rbgs_blocked.o"):
                if os.path.exists(os.path.join(_CSRC, f)):
                    os.remove(os.path.join(_CSRC, f))
            subprocess.check_call(["make", "-C", _CSRC, "-j4", "CXXFLAGS_EXTRA=-DRTDD_EXCHANGE_ACQUIRE=1"], stdout=subprocess.DEVNULL)
        variant = "acquire"
    with open(stamp, "w") as f:
        f.write(variant + "\n")
    return _SO


_lib = None


def lib():
    """The loaded librtdd.so.  Raises (never falls back) when the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RtddError(-1, f"{_SO} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is no CPU fallback)")
        try:
            # torch wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7, NEEDED as plain
            # "libamdhip64.so").  If librtdd.so pulled in /opt/rocm's copy first, torch would load a
            # SECOND HIP runtime into the process and find no GPUs.  Loading torch first makes the
            # dynamic linker satisfy librtdd's libamdhip64.so.7 with the runtime torch already holds.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_SO)
        L.rtdd_last_error.restype = C.c_char_p
        L.rtdd_status_string.restype = C.c_char_p
        for name in C_ABI_SYMBOLS:
            getattr(L, name)        # fail at load time, not at first use, if a symbol is missing
        if L.rtdd_version() // 100 != 2:    # SolveInfo below is the 36-byte rtdd_solve_info of ABI 2xx
            raise RtddError(-1, f"{_SO} has ABI version {L.rtdd_version()}, this binding needs 2xx: rebuild")
        _lib = L
    return _lib


def _img(t):
    """(pointer, pitch in bytes) of a pitched device image."""
    if isinstance(t, tuple):
        return C.c_void_p(t[0]), C.c_size_t(t[1])
    assert t.stride(-1) == 1 or (t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]), "pixels must be contiguous within a row"
    return C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(0) * t.element_size())


def _paint_images(edited, scribble, original):
    """The six image arguments of the paint calls: edited, scribble and the optional original, each as (pointer, pitch)."""
    return (*_img(edited), *_img(scribble), *(_img(original) if original is not None else (None, C.c_size_t(0))))


class Context:
    """One solver context per GPU (handle of the C ABI).  Methods carry the reference's names."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        rc = lib().rtdd_ctx_create(C.c_int(device), C.byref(self._h))
        if rc != RTDD_OK:
            raise RtddError(rc, lib().rtdd_status_string(rc).decode())
        self.device = device
        self.last_cycles = 0                    # V-cycles of the last solve_ex / refine_depth (rtdd_solve_info.cycles)
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().rtdd_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != RTDD_OK:
            raise RtddError(rc, lib().rtdd_status_string(rc).decode() + " -- " + lib().rtdd_last_error(self._h).decode())

    # ---- context plumbing
    def set_stream(self, stream):
        """stream: a raw hipStream_t value (e.g. torch.cuda.current_stream().cuda_stream) or 0."""
        self._check(lib().rtdd_ctx_set_stream(self._h, C.c_void_p(int(stream))))

    def synchronize(self):
        self._check(lib().rtdd_ctx_synchronize(self._h))

    def set_option(self, key, value):
        self._check(lib().rtdd_set_option(self._h, C.c_int(key), C.c_int(value)))

    def get_option(self, key):
        v = C.c_int()
        self._check(lib().rtdd_get_option(self._h, C.c_int(key), C.byref(v)))
        return v.value

    def auto_model(self, rows, cols):
        """(seconds RTDD_METHOD_AUTO prices its SOR-cycle alternative at, seconds per V-cycle): csrc/api.cpp Solve::automatic(),
        from the RTDD_OPT_AUTO_* constants the library holds."""
        px = float(rows * cols)
        sweep = max(px * self.get_option(OPT_AUTO_SWEEP_FS_PER_PX) * 1e-15, self.get_option(OPT_AUTO_SWEEP_FLOOR_NS) * 1e-9)
        sor = (((max(rows, cols) + 1) // 2) * 1.25 + 20.0) * sweep
        cycle = self.get_option(OPT_AUTO_CYCLE_FIXED_NS) * 1e-9 + px * self.get_option(OPT_AUTO_CYCLE_FS_PER_PX) * 1e-15
        return sor, cycle

    def profile_enable(self, on=True):
        self._check(lib().rtdd_profile_enable(self._h, C.c_int(1 if on else 0)))

    def profile(self):
        p = Profile()
        self._check(lib().rtdd_profile_get(self._h, C.byref(p)))
        return p

    # ---- include/GPUSolver.h
    def GPUAllocateDeviceMemory(self, rows, cols, levels):
        self._check(lib().rtdd_allocate(self._h, C.c_int(rows), C.c_int(cols), C.c_int(levels)))

    def GPUFreeDeviceMemory(self, levels=0):
        self._check(lib().rtdd_free(self._h))

    def GPULoadWeights(self, beta):
        self._check(lib().rtdd_load_weights(self._h, C.c_float(beta)))

    def GPUMatrixFreeSolver(self, depthImage, scribbleImage, grayImage, rows, cols, beta, maxIterations, tolerance, level):
        dp, dpitch = _img(depthImage); sp, spitch = _img(scribbleImage); gp, gpitch = _img(grayImage)
        self._check(lib().rtdd_matrix_free_solver(self._h, dp, dpitch, sp, spitch, gp, gpitch, C.c_int(rows), C.c_int(cols),
                                                  C.c_float(beta), C.c_int(maxIterations), C.c_float(tolerance), C.c_int(level)))

    def solve_ex(self, depthImage, scribbleImage, grayImage, rows, cols, level, method=METHOD_CHEBYSHEV_JACOBI,
                 maxIterations=1000, tolerance=0.0, checkEvery=0, relaxation=0.0):
        dp, dpitch = _img(depthImage); sp, spitch = _img(scribbleImage); gp, gpitch = _img(grayImage)
        params = SolveParams(method, maxIterations, tolerance, checkEvery, relaxation)
        info = SolveInfo()
        self._check(lib().rtdd_solve_ex(self._h, dp, dpitch, sp, spitch, gp, gpitch, C.c_int(rows), C.c_int(cols), C.c_int(level),
                                        C.byref(params), C.byref(info)))
        self.last_cycles = info.cycles          # V-cycles of the last solve (METHOD_MULTIGRID / METHOD_AUTO)
        return info.iterations, info.residual

    def solve_guided(self, depthImage, scribbleImage, guideImage, guideKind, rows, cols, level, method=METHOD_CHEBYSHEV_JACOBI,
                     maxIterations=1000, tolerance=0.0, checkEvery=0, relaxation=0.0):
        """rtdd_solve_guided: solve_ex with the edge weights read from `guideImage` as `guideKind` says -- GUIDE_GRAY (solve_ex itself) or
        GUIDE_BGR (an interleaved colour image: the index of an edge is the largest channel difference)."""
        dp, dpitch = _img(depthImage); sp, spitch = _img(scribbleImage); gp, gpitch = _img(guideImage)
        params = SolveParams(method, maxIterations, tolerance, checkEvery, relaxation)
        info = SolveInfo()
        self._check(lib().rtdd_solve_guided(self._h, dp, dpitch, sp, spitch, gp, gpitch, C.c_int(guideKind), C.c_int(rows), C.c_int(cols),
                                            C.c_int(level), C.byref(params), C.byref(info)))
        self.last_cycles = info.cycles
        return info.iterations, info.residual

    def solve_regions(self, depthImage, scribbleImage, guideImage, guideKind, regionImage, regionFlags, rows, cols, level,
                      method=METHOD_CHEBYSHEV_JACOBI, maxIterations=1000, tolerance=0.0, checkEvery=0, relaxation=0.0):
        """rtdd_solve_regions: solve_guided with the region rule on top -- `regionImage` holds one u8 code per pixel (0: unassigned; None
        with regionFlags 0: solve_guided itself), `regionFlags` REGION_CUT | REGION_SMOOTH."""
        dp, dpitch = _img(depthImage); sp, spitch = _img(scribbleImage); gp, gpitch = _img(guideImage)
        rp, rpitch = _img(regionImage) if regionImage is not None else (None, C.c_size_t(0))
        params = SolveParams(method, maxIterations, tolerance, checkEvery, relaxation)
        info = SolveInfo()
        self._check(lib().rtdd_solve_regions(self._h, dp, dpitch, sp, spitch, gp, gpitch, C.c_int(guideKind), rp, rpitch, C.c_int(regionFlags),
                                             C.c_int(rows), C.c_int(cols), C.c_int(level), C.byref(params), C.byref(info)))
        self.last_cycles = info.cycles
        return info.iterations, info.residual

    def last_solve_info(self):
        """What the most recent solve on this context actually ran (kernel, tile, depth, persistence, contraction, counts)."""
        info = SolveInfo()
        self._check(lib().rtdd_last_solve_info(self._h, C.byref(info)))
        return info

    def scaled_mode_waves(self):
        """How many waves of this context's persistent Jacobi launches have entered scaled mode so far (rtdd_scaled_mode_waves; synchronises)."""
        n = C.c_int(0)
        self._check(lib().rtdd_scaled_mode_waves(self._h, C.byref(n)))
        return n.value

    def multigrid_level(self, level, which):
        """Diagnostic: plane `which` of hierarchy level `level` after a METHOD_MULTIGRID solve, as a numpy array."""
        import numpy as np
        r = C.c_int(0); c = C.c_int(0)
        self._check(lib().rtdd_multigrid_level(self._h, C.c_int(level), C.c_int(which), None, C.byref(r), C.byref(c)))
        out = np.zeros((r.value, c.value), np.float32)
        self._check(lib().rtdd_multigrid_level(self._h, C.c_int(level), C.c_int(which), out.ctypes.data_as(C.c_void_p), C.byref(r), C.byref(c)))
        return out

    def index_to_weight(self, grayImage, depthImage, index2, level, rows, cols):
        gp, gpitch = _img(grayImage); dp, dpitch = _img(depthImage)
        self._check(lib().rtdd_index_to_weight(self._h, gp, gpitch, dp, dpitch, C.c_void_p(index2.data_ptr()), C.c_int(level),
                                               C.c_int(rows), C.c_int(cols)))

    def index_to_weight_guided(self, guideImage, guideKind, depthImage, index2, level, rows, cols):
        gp, gpitch = _img(guideImage); dp, dpitch = _img(depthImage)
        self._check(lib().rtdd_index_to_weight_guided(self._h, gp, gpitch, C.c_int(guideKind), dp, dpitch, C.c_void_p(index2.data_ptr()),
                                                      C.c_int(level), C.c_int(rows), C.c_int(cols)))

    def index_to_weight_regions(self, guideImage, guideKind, regionImage, regionFlags, depthImage, index2, level, rows, cols):
        gp, gpitch = _img(guideImage); dp, dpitch = _img(depthImage)
        rp, rpitch = _img(regionImage) if regionImage is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_index_to_weight_regions(self._h, gp, gpitch, C.c_int(guideKind), rp, rpitch, C.c_int(regionFlags), dp, dpitch,
                                                       C.c_void_p(index2.data_ptr()), C.c_int(level), C.c_int(rows), C.c_int(cols)))

    def region_codes(self, edited, mask, rows, cols, level, codes):
        """rtdd_region_codes: the codes of pyramid level `level` from a rows x cols level-0 region pair, into `codes`."""
        e, ep = _img(edited); m, mp = _img(mask); c, cp = _img(codes)
        self._check(lib().rtdd_region_codes(self._h, e, ep, m, mp, C.c_int(rows), C.c_int(cols), C.c_int(level), c, cp))

    # ---- include/GPUImageProcessing.h
    def GPUConvertToFloat(self, src, dst, mask, rows, cols):
        s, sp = _img(src); d, dp = _img(dst); m, mp = _img(mask)
        self._check(lib().rtdd_convert_to_float(self._h, s, sp, d, dp, m, mp, C.c_int(rows), C.c_int(cols)))

    def GPUPyrDownAnnotation(self, prevScribbleImage, prevEditedImage, previousRows, previousCols,
                             currScribbleImage, currEditedImage, currentRows, currentCols):
        a, ap = _img(prevScribbleImage); b, bp = _img(prevEditedImage); c, cp = _img(currScribbleImage); d, dp = _img(currEditedImage)
        self._check(lib().rtdd_pyrdown_annotation(self._h, a, ap, b, bp, C.c_int(previousRows), C.c_int(previousCols),
                                                  c, cp, d, dp, C.c_int(currentRows), C.c_int(currentCols)))

    def GPUPaintImage(self, x, y, scribbleColor, scribbleRadius, editedImage, scribbleImage, rows, cols):
        e, ep = _img(editedImage); s, sp = _img(scribbleImage)
        self._check(lib().rtdd_paint_image(self._h, C.c_int(x), C.c_int(y), C.c_int(scribbleColor), C.c_int(scribbleRadius),
                                           e, ep, s, sp, C.c_int(rows), C.c_int(cols)))

    def paint_strokes(self, strokes, edited, scribble, rows, cols, original=None):
        """rtdd_paint_strokes: `strokes` (Stroke objects or 7-tuples x0, y0, x1, y1, radius, brush, label) in order, one call; `original`
        is needed when a stroke erases."""
        arr = (Stroke * max(len(strokes), 1))(*[q if isinstance(q, Stroke) else Stroke(*q) for q in strokes])
        self._check(lib().rtdd_paint_strokes(self._h, arr, C.c_int(len(strokes)), *_paint_images(edited, scribble, original), C.c_int(rows), C.c_int(cols)))

    def paint_ramp_strokes(self, strokes, edited, scribble, rows, cols, original=None):
        """rtdd_paint_ramp_strokes: `strokes` (RampStroke objects or 8-tuples x0, y0, x1, y1, radius, brush, label0, label1) in order, one
        call; `original` is needed when a stroke erases."""
        arr = (RampStroke * max(len(strokes), 1))(*[q if isinstance(q, RampStroke) else RampStroke(*q) for q in strokes])
        self._check(lib().rtdd_paint_ramp_strokes(self._h, arr, C.c_int(len(strokes)), *_paint_images(edited, scribble, original), C.c_int(rows), C.c_int(cols)))

    def fill_polygon(self, points, fill, edited, scribble, rows, cols, original=None):
        """rtdd_fill_polygon: the closed contour through `points` [(x, y), ...] (at most 768) filled by `fill` (a Fill or a 7-tuple rule,
        ax0, ay0, ax1, ay1, label0, label1); `original` is needed when it erases."""
        n = len(points)
        xy = (C.c_int * max(2 * n, 1))(*[int(v) for p in points for v in p])
        f = fill if isinstance(fill, Fill) else Fill(*fill)
        self._check(lib().rtdd_fill_polygon(self._h, xy, C.c_int(n), C.byref(f), *_paint_images(edited, scribble, original), C.c_int(rows), C.c_int(cols)))

    def fill_similar(self, wand, edited, scribble, rows, cols, original):
        """rtdd_fill_similar: everything joined to the clicked pixel whose colour in `original` is within the tolerance of the clicked colour
        is filled by `wand` (a Wand or a 10-tuple x, y, tolerance, flags, ax0, ay0, ax1, ay1, label0, label1).  SYNCHRONISES; returns the
        WandInfo."""
        w = wand if isinstance(wand, Wand) else Wand(*wand)
        info = WandInfo()
        self._check(lib().rtdd_fill_similar(self._h, C.byref(w), *_paint_images(edited, scribble, original), C.c_int(rows), C.c_int(cols), C.byref(info)))
        return info

    def fill_surface(self, wand, edited, scribble, rows, cols, depth, original=None):
        """rtdd_fill_surface: everything joined to the clicked pixel through neighbours whose depths in `depth` (f32) differ by at most the
        step, inside the band around the clicked depth, is filled by `wand` (a SurfaceWand or a 12-tuple x, y, step, below, above, flags,
        ax0, ay0, ax1, ay1, label0, label1); `original` is needed when it erases.  SYNCHRONISES; returns the WandInfo."""
        w = wand if isinstance(wand, SurfaceWand) else SurfaceWand(*wand)
        info = WandInfo()
        d, dp = _img(depth)
        self._check(lib().rtdd_fill_surface(self._h, C.byref(w), *_paint_images(edited, scribble, original), d, dp, C.c_int(rows), C.c_int(cols), C.byref(info)))
        return info

    def segment_surfaces(self, seg, edited, scribble, rows, cols, depth, labels=None):
        """rtdd_segment_surfaces: every component of rtdd_fill_surface's link graph over `depth` (f32) under `seg` (a Segmentation or a
        7-tuple step, lo, hi, minPixels, maxRegions, firstCode, flags); the largest are painted into the pair as codes firstCode, ...
        (edited and scribble both None: nothing is painted) and `labels` (int32, optional) gets every pixel's root or -1.  SYNCHRONISES;
        returns (SegmentInfo, [Segment, ...] in rank order)."""
        g = seg if isinstance(seg, Segmentation) else Segmentation(*seg)
        info = SegmentInfo()
        records = (Segment * max(g.maxRegions, 1))()
        none = (None, C.c_size_t(0))
        self._check(lib().rtdd_segment_surfaces(self._h, C.byref(g), *(_img(edited) if edited is not None else none),
                                                *(_img(scribble) if scribble is not None else none), *_img(depth),
                                                *(_img(labels) if labels is not None else none), C.c_int(rows), C.c_int(cols), records, C.byref(info)))
        return info, [records[k] for k in range(info.regions)]

    # ---- include/GPUDepthEffect.h
    def GPUSimulateDefocus(self, originalImage, depthImage, artisticImage, rows, cols):
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_defocus(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols)))

    def GPUSimulateDesaturation(self, originalImage, grayImage, depthImage, artisticImage, rows, cols):
        o, op = _img(originalImage); g, gp = _img(grayImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_desaturation(self._h, o, op, g, gp, d, dp, a, ap, C.c_int(rows), C.c_int(cols)))

    def GPUSimulateHaze(self, originalImage, depthImage, artisticImage, rows, cols):
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_haze(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols)))

    # ---- aimed depth effects (extensions, include/rtdd.h)
    def simulate_refocus(self, originalImage, depthImage, artisticImage, rows, cols, aperture=0.025, focusDepth=0.0, focusX=-1, focusY=-1):
        """Defocus sharp at depth `focusDepth`, or (focusX >= 0) at the depth map's value at (focusX, focusY), read on the device."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_refocus(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols), C.c_double(aperture),
                                                C.c_float(focusDepth), C.c_int(focusX), C.c_int(focusY)))

    def simulate_lens_blur(self, originalImage, depthImage, artisticImage, rows, cols, aperture=0.025, focusDepth=0.0, focusX=-1, focusY=-1,
                           shape=APERTURE_DISC):
        """Refocus through a round aperture (shape APERTURE_DISC: disc windows) or a square one (APERTURE_BOX: simulate_refocus itself)."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_lens_blur(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols), C.c_double(aperture),
                                                  C.c_float(focusDepth), C.c_int(focusX), C.c_int(focusY), C.c_int(shape)))

    def simulate_bokeh(self, originalImage, depthImage, artisticImage, rows, cols, aperture=0.025, focusDepth=0.0, focusX=-1, focusY=-1):
        """The occlusion-aware lens blur: every pixel spreads its colour over its own circle of confusion (the disc of simulate_lens_blur),
        and a pixel behind the target spreads no wider than the target's own circle -- a sharp subject gets no halo, a blurred one a soft
        edge.  The focus as simulate_refocus's; the window scale (int)(aperture * diagonal) must be <= 127."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_bokeh(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols), C.c_double(aperture),
                                              C.c_float(focusDepth), C.c_int(focusX), C.c_int(focusY)))

    def simulate_haze_ex(self, originalImage, depthImage, artisticImage, rows, cols, beta=2.0, air=(255, 255, 255)):
        """Haze with density `beta` and airlight `air` = (b, g, r)."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        b, g, r = air
        self._check(lib().rtdd_simulate_haze_ex(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols), C.c_float(beta),
                                                C.c_uint8(b), C.c_uint8(g), C.c_uint8(r)))

    def simulate_stereo(self, originalImage, depthImage, artisticImage, rows, cols, disparity, zeroParallaxDepth=0.0, zeroX=-1, zeroY=-1,
                        mode=STEREO_VIEW):
        """A second eye's view with `disparity` pixels between depths 0 and 255, zero parallax at `zeroParallaxDepth` or (zeroX >= 0) at
        the depth map's value at (zeroX, zeroY), read on the device; mode STEREO_ANAGLYPH: a red-cyan anaglyph of it with the original."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_stereo(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols), C.c_int(disparity),
                                               C.c_float(zeroParallaxDepth), C.c_int(zeroX), C.c_int(zeroY), C.c_int(mode)))

    def simulate_relight(self, originalImage, depthImage, artisticImage, rows, cols, light):
        """The depth map as a surface under `light` (a Light, or None for the C call's null pointer): a directional light, or a point
        light anchored to the surface that falls off with distance."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_relight(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols),
                                                C.byref(light) if light is not None else None))

    def simulate_relight_shadowed(self, originalImage, depthImage, artisticImage, rows, cols, light, shadow):
        """simulate_relight with cast shadows: a height-field march per pixel towards `light`, as `shadow` (a Shadow, or None for the C
        call's null pointer) says."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_relight_shadowed(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols),
                                                         C.byref(light) if light is not None else None,
                                                         C.byref(shadow) if shadow is not None else None))

    def simulate_parallax(self, originalImage, depthImage, artisticImage, rows, cols, view):
        """The view of a camera moved sideways, up or forward as `view` (a Parallax, or None for the C call's null pointer) says: a
        forward warp over the whole image, the nearest source wins, holes filled from the background side."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_parallax(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols),
                                                 C.byref(view) if view is not None else None))

    def simulate_parallax_layered(self, originalImage, depthImage, plateImage, plateDepthImage, artisticImage, depthOutImage, coverageImage,
                                  rows, cols, view):
        """simulate_parallax over two layers: the plate (plateImage u8 x 3 and plateDepthImage f32, both or neither None: the scene without
        the object, as remove_object writes it) fills what the camera's move uncovers.  depthOutImage (f32) and coverageImage (u8: 0
        front-won, 1 back-won, 2 a crack, 3 a hole filled by a march, 4 a hole left as the original) receive the view's depth map and its
        coverage; each may be None for the C call's null pointer."""
        null = (None, C.c_size_t(0))
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        p, pp = _img(plateImage) if plateImage is not None else null
        q, qp = _img(plateDepthImage) if plateDepthImage is not None else null
        z, zp = _img(depthOutImage) if depthOutImage is not None else null
        c, cp = _img(coverageImage) if coverageImage is not None else null
        self._check(lib().rtdd_simulate_parallax_layered(self._h, o, op, d, dp, p, pp, q, qp, a, ap, z, zp, c, cp, C.c_int(rows), C.c_int(cols),
                                                         C.byref(view) if view is not None else None))

    def simulate_ambient_occlusion(self, originalImage, depthImage, artisticImage, rows, cols, ao, light=None):
        """Ambient occlusion from the depth map as `ao` (an AmbientOcclusion, or None for the C call's null pointer) says: alone
        (light None: the original darkened, or AO_MAP's gray map), or as the ambient term of simulate_relight under `light`."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_ambient_occlusion(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols),
                                                          C.byref(ao) if ao is not None else None,
                                                          C.byref(light) if light is not None else None))

    def simulate_lighting(self, originalImage, depthImage, artisticImage, rows, cols, light, shadow, ao):
        """The whole lighting model in one call: simulate_relight's shade under `light`, simulate_relight_shadowed's cast shadows as
        `shadow` says and simulate_ambient_occlusion's occlusion of the ambient term as `ao` (AO_SHADE, relief the light's) says.  Each
        may be None for the C call's null pointer."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        self._check(lib().rtdd_simulate_lighting(self._h, o, op, d, dp, a, ap, C.c_int(rows), C.c_int(cols),
                                                 C.byref(light) if light is not None else None,
                                                 C.byref(shadow) if shadow is not None else None,
                                                 C.byref(ao) if ao is not None else None))

    def composite_layer(self, originalImage, depthImage, spriteImage, artisticImage, depthOutImage, rows, cols, layer):
        """A sprite (u8 x 4: B, G, R, A; straight alpha) inserted into the scene as `layer` (a Layer, or None for the C call's null
        pointer) says: the depth map hides what lies behind nearer things.  depthOutImage (None: not written) receives the composite's
        depth map -- the layer's depth where the layer won, the scene's elsewhere -- for the effects that follow."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        s, sp = _img(spriteImage) if spriteImage is not None else (None, C.c_size_t(0))
        z, zp = _img(depthOutImage) if depthOutImage is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_composite_layer(self._h, o, op, d, dp, s, sp, a, ap, z, zp, C.c_int(rows), C.c_int(cols),
                                               C.byref(layer) if layer is not None else None))

    def remove_object(self, originalImage, depthImage, maskImage, artisticImage, depthOutImage, rows, cols, removal):
        """The pixels `maskImage` (u8, rows x cols) selects as `removal` (a Removal, or None for the C call's null pointer) says are filled,
        colour and depth, from what lies around them (a push-pull over a pyramid).  depthOutImage (None: not written) receives the depth
        map without the object, for the effects that follow."""
        o, op = _img(originalImage); d, dp = _img(depthImage); a, ap = _img(artisticImage)
        m, mp = _img(maskImage) if maskImage is not None else (None, C.c_size_t(0))
        z, zp = _img(depthOutImage) if depthOutImage is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_remove_object(self._h, o, op, d, dp, m, mp, a, ap, z, zp, C.c_int(rows), C.c_int(cols),
                                             C.byref(removal) if removal is not None else None))

    def lift_layer(self, originalImage, maskImage, rows, cols, select, x, y, spriteImage, spriteRows, spriteCols):
        """The selected pixels (mask byte != 0, or == select) of the box whose corner is image pixel (x, y) cut out as a u8 x 4 sprite
        (B, G, R, 255; everything else 0, 0, 0, 0) for composite_layer."""
        o, op = _img(originalImage); m, mp = _img(maskImage); s, sp = _img(spriteImage)
        self._check(lib().rtdd_lift_layer(self._h, o, op, m, mp, C.c_int(rows), C.c_int(cols), C.c_int(select), C.c_int(x), C.c_int(y),
                                          s, sp, C.c_int(spriteRows), C.c_int(spriteCols)))

    def mask_distance(self, maskImage, rows, cols, select, reach, dist2Image):
        """The exact squared Euclidean distance of every pixel of `maskImage` (u8, rows x cols; selected: byte != 0, or == select) to the
        nearest pixel of the other class, into dist2Image (int32, rows x cols): negative inside the selection, positive outside, never 0;
        +-DISTANCE_FAR where it exceeds reach * reach (reach 1..1024) or the other class is empty."""
        m, mp = _img(maskImage) if maskImage is not None else (None, C.c_size_t(0))
        d, dp = _img(dist2Image) if dist2Image is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_mask_distance(self._h, m, mp, C.c_int(rows), C.c_int(cols), C.c_int(select), C.c_int(reach), d, dp))

    def refine_mask(self, maskImage, rows, cols, refine, outImage):
        """`maskImage` grown, shrunk, outlined or feathered as `refine` (a MaskRefine, or None for the C call's null pointer) says, by the
        exact Euclidean distance, into outImage (u8, rows x cols): 0 / 255, or the feather's ramp."""
        m, mp = _img(maskImage) if maskImage is not None else (None, C.c_size_t(0))
        o, op = _img(outImage) if outImage is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_refine_mask(self._h, m, mp, C.c_int(rows), C.c_int(cols), C.byref(refine) if refine is not None else None, o, op))

    def lift_layer_matte(self, originalImage, alphaImage, rows, cols, x, y, spriteImage, spriteRows, spriteCols):
        """lift_layer with an alpha image (u8, rows x cols, e.g. a feathered mask) in place of the mask: texel (B, G, R, alpha) where
        alpha != 0, everything else 0, 0, 0, 0.  Composited back where it came from it gives the original byte for byte."""
        o, op = _img(originalImage); m, mp = _img(alphaImage); s, sp = _img(spriteImage)
        self._check(lib().rtdd_lift_layer_matte(self._h, o, op, m, mp, C.c_int(rows), C.c_int(cols), C.c_int(x), C.c_int(y),
                                                s, sp, C.c_int(spriteRows), C.c_int(spriteCols)))

    # ---- whole-estimate driver (src/main.cpp:92-155, 232-295)
    def pyramid_create(self, rows, cols):
        self._check(lib().rtdd_pyramid_create(self._h, C.c_int(rows), C.c_int(cols)))
        return int(lib().rtdd_pyramid_levels(C.c_int(rows), C.c_int(cols)))

    def pyramid_create_batch(self, rows, cols, images):
        """`images` pyramids of one size on this context (rtdd_estimate_depth_batch runs them in the same launches)."""
        self._check(lib().rtdd_pyramid_create_batch(self._h, C.c_int(rows), C.c_int(cols), C.c_int(images)))
        return int(lib().rtdd_pyramid_levels(C.c_int(rows), C.c_int(cols)))

    def pyramid_select(self, index):
        self._check(lib().rtdd_pyramid_select(self._h, C.c_int(index)))

    def estimate_depth_batch(self, maxIterations=1000):
        self._check(lib().rtdd_estimate_depth_batch(self._h, C.c_int(maxIterations)))

    def pyramid_level_info(self, level):
        """(SolveInfo, images per sweep launch) of what the most recent estimate ran on pyramid level `level`."""
        info = SolveInfo(); n = C.c_int()
        self._check(lib().rtdd_pyramid_level_info(self._h, C.c_int(level), C.byref(info), C.byref(n)))
        return info, n.value

    def pyramid_destroy(self):
        self._check(lib().rtdd_pyramid_destroy(self._h))

    def pyramid_set_image(self, bgr):
        p, pitch = _img(bgr)
        self._check(lib().rtdd_pyramid_set_image(self._h, p, pitch))

    def pyramid_set_guide(self, guideKind):
        """GUIDE_GRAY (the default, the reference's behaviour) or GUIDE_BGR: the estimates' per-level solves read the colour pyramid."""
        self._check(lib().rtdd_pyramid_set_guide(self._h, C.c_int(guideKind)))

    def pyramid_guide(self):
        return int(lib().rtdd_pyramid_guide(self._h))

    def pyramid_set_regions(self, flags):
        """REGION_CUT | REGION_SMOOTH: the estimates apply the region rule with the codes painted into IMG_REGION_EDITED / IMG_REGION_MASK
        (the first non-zero call allocates them); 0 switches the effect off and keeps the images."""
        self._check(lib().rtdd_pyramid_set_regions(self._h, C.c_int(flags)))

    def pyramid_regions(self):
        return int(lib().rtdd_pyramid_regions(self._h))

    def pyramid_regions_changed(self):
        """The host wrote the region pair through the raw pointers: the code planes are filled again before the next estimate."""
        self._check(lib().rtdd_pyramid_regions_changed(self._h))

    def pyramid_set_annotation(self, annotation):
        p, pitch = _img(annotation)
        self._check(lib().rtdd_pyramid_set_annotation(self._h, p, pitch))

    def pyramid_annotation_changed(self):
        self._check(lib().rtdd_pyramid_annotation_changed(self._h))

    def pyramid_annotation_rebuild(self):
        """Labels were removed from the level-0 annotation: the next estimate builds the coarse levels afresh instead of adding to them."""
        self._check(lib().rtdd_pyramid_annotation_rebuild(self._h))

    def pyramid_image(self, kind, level=0):
        """(ptr, pitch_bytes, rows, cols) of a context-owned pyramid image."""
        ptr = C.c_void_p(); pitch = C.c_size_t(); rows = C.c_int(); cols = C.c_int()
        self._check(lib().rtdd_pyramid_image(self._h, C.c_int(kind), C.c_int(level), C.byref(ptr), C.byref(pitch), C.byref(rows), C.byref(cols)))
        return ptr.value, pitch.value, rows.value, cols.value

    def pyramid_download(self, kind, level=0):
        import numpy as np
        ptr, pitch, rows, cols = self.pyramid_image(kind, level)
        dtype, ch = (np.float32, 1) if kind == IMG_DEPTH else (np.uint8, 3 if kind in (IMG_ORIGINAL, IMG_EDITED, IMG_ARTISTIC, IMG_GUIDE_BGR, IMG_REGION_EDITED) else 1)
        out = np.empty((rows, cols, ch) if ch == 3 else (rows, cols), dtype)
        if rows and cols:
            w = cols * ch * out.itemsize
            self._check(lib().rtdd_download(self._h, C.c_void_p(out.ctypes.data), C.c_size_t(w), C.c_void_p(ptr), C.c_size_t(pitch), C.c_size_t(w), C.c_int(rows)))
        return out

    def estimate_depth(self, maxIterations=1000):
        self._check(lib().rtdd_estimate_depth(self._h, C.c_int(maxIterations)))

    # ---- live mode (src/main.cpp:232-295 pipelined): host images are numpy views of page-locked memory (host_image)
    def live_submit(self, scribble, edited, depth_u8, maxIterations=1000):
        sp = (C.c_void_p(scribble.ctypes.data), C.c_size_t(scribble.strides[0])) if scribble is not None else (None, C.c_size_t(0))
        ep = (C.c_void_p(edited.ctypes.data), C.c_size_t(edited.strides[0])) if edited is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_live_submit(self._h, sp[0], sp[1], ep[0], ep[1], C.c_int(maxIterations),
                                           C.c_void_p(depth_u8.ctypes.data), C.c_size_t(depth_u8.strides[0])))

    def live_submit_ex(self, scribble, edited, depth_u8, effect, artistic, maxIterations=1000):
        """rtdd_live_submit_ex: the frame with a sticky depth effect (EFFECT_*), its artistic image into the host array `artistic`."""
        sp = (C.c_void_p(scribble.ctypes.data), C.c_size_t(scribble.strides[0])) if scribble is not None else (None, C.c_size_t(0))
        ep = (C.c_void_p(edited.ctypes.data), C.c_size_t(edited.strides[0])) if edited is not None else (None, C.c_size_t(0))
        ap = (C.c_void_p(artistic.ctypes.data), C.c_size_t(artistic.strides[0])) if artistic is not None else (None, C.c_size_t(0))
        self._check(lib().rtdd_live_submit_ex(self._h, sp[0], sp[1], ep[0], ep[1], C.c_int(maxIterations),
                                              C.c_void_p(depth_u8.ctypes.data), C.c_size_t(depth_u8.strides[0]), C.c_int(effect), ap[0], ap[1]))

    def live_wait(self):
        self._check(lib().rtdd_live_wait(self._h))

    def live_pending(self):
        return int(lib().rtdd_live_pending(self._h))

    def refine_depth(self, method=METHOD_RED_BLACK_GS, maxIterations=200000, tolerance=1e-4, checkEvery=0, relaxation=RELAXATION_AUTO):
        """rtdd_refine_depth: converge the finest level of the last estimate in place.  Returns (iterations, residual)."""
        params = SolveParams(method, maxIterations, tolerance, checkEvery, relaxation if method == METHOD_RED_BLACK_GS else 0.0)
        info = SolveInfo()
        self._check(lib().rtdd_refine_depth(self._h, C.byref(params), C.byref(info)))
        self.last_cycles = info.cycles
        return info.iterations, info.residual

    def bgr2gray(self, bgr, gray, rows, cols):
        b, bp = _img(bgr); g, gp = _img(gray)
        self._check(lib().rtdd_bgr2gray(self._h, b, bp, g, gp, C.c_int(rows), C.c_int(cols)))

    def pyrdown_gray(self, src, rows, cols, dst):
        s, sp = _img(src); d, dp = _img(dst)
        self._check(lib().rtdd_pyrdown_gray(self._h, s, sp, C.c_int(rows), C.c_int(cols), d, dp))

    def pyrdown_bgr(self, src, rows, cols, dst):
        s, sp = _img(src); d, dp = _img(dst)
        self._check(lib().rtdd_pyrdown_bgr(self._h, s, sp, C.c_int(rows), C.c_int(cols), d, dp))

    def pyrup_depth(self, src, rows, cols, dst, drows, dcols):
        s, sp = _img(src); d, dp = _img(dst)
        self._check(lib().rtdd_pyrup_depth(self._h, s, sp, C.c_int(rows), C.c_int(cols), d, dp, C.c_int(drows), C.c_int(dcols)))

    def depth_to_u8(self, src, dst, rows, cols):
        s, sp = _img(src); d, dp = _img(dst)
        self._check(lib().rtdd_depth_to_u8(self._h, s, sp, d, dp, C.c_int(rows), C.c_int(cols)))


# ---- pitched device images (torch is plumbing for device memory only) ----------------------------
def device_image(host, device="cuda:0", align=512):
    """Upload a numpy image [rows, cols] or [rows, cols, 3] into a PITCHED device tensor whose row
    stride is padded to `align` bytes, like cudaMallocPitch / cv::cuda::GpuMat in the reference
    (/root/reference/src/main.cpp:117-137).  Returns the logical view (use .stride(0) for the pitch)."""
    import numpy as np
    import torch
    host = np.ascontiguousarray(host)
    rows = host.shape[0]
    row_elems = int(np.prod(host.shape[1:]))
    item = host.itemsize
    pitch_elems = ((row_elems * item + align - 1) // align * align) // item
    base = torch.zeros((rows, pitch_elems), dtype=torch.from_numpy(host[:0]).dtype, device=device)
    view = base[:, :row_elems]
    view.copy_(torch.from_numpy(host.reshape(rows, row_elems)).to(device))
    if host.ndim == 3:
        view = view.unflatten(1, host.shape[1:])
    return view


class host_image:
    """A numpy array over page-locked host memory (rtdd_host_alloc), so that live-mode copies are asynchronous.  `.a` is the array;
    free() or the garbage collector releases the memory (keep the object alive while frames that use it are in flight)."""

    def __init__(self, shape, dtype="uint8"):
        import numpy as np
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = C.c_void_p()
        rc = lib().rtdd_host_alloc(C.byref(self._p), C.c_size_t(n))
        if rc != RTDD_OK:
            raise RtddError(rc, "rtdd_host_alloc")
        self.a = np.frombuffer((C.c_char * n).from_address(self._p.value), dtype=dtype).reshape(shape)

    def free(self):
        if self._p is not None and self._p.value:
            self.a = None
            lib().rtdd_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def to_host(view):
    return view.cpu().contiguous().numpy()
