"""ctypes loader for the reference's own GPU code, built by oracle/ref.mk into oracle/_ref/ (TEST INFRASTRUCTURE ONLY: the product
never imports it, tests/test_abi.py).

``RefLib(contract)`` loads ``libref_c{contract}.so`` -- the reference's three .cu files, hipified and compiled for gfx950 with
FP contraction off (0) or on (1) -- and offers its ten functions under their own names, taking torch device tensors (pitched views
as ``tests/gpu_util.up`` makes them) like ``realtimedepthdiffusion_amd.Context`` does.  Each of the two libraries holds its own copy
of the reference's global state (device buffers, weight LUT, maxLevel).

What the wrapper adds, because the reference checks nothing:
  * bounds, on the host, before every launch: every image must hold the rows x cols (x 3) the call names, and a solver call must fit
    the buffers GPUAllocateDeviceMemory made for its level -- int(rows / powf(2, level)) x int(cols / powf(2, level))
    (src/GPUSolver.cu:35-49); the solver works densely on whatever size it is given and would write past them.  To run level l of
    maxLevel at (r, c), allocate (r << l, c << l, maxLevel + 1).  Calls of size 0 are refused too (a launch of an empty grid).
  * ``allocated(rows, cols, levels)`` pairs every GPUAllocateDeviceMemory with GPUFreeDeviceMemory, so device memory does not grow
    across tests; a second allocation while one is live is refused.
  * the reference launches on the null stream and synchronises only inside its GPUCheckError (the solver-side functions): every
    call here is fenced by torch.cuda.synchronize() on both sides.
  * the reference reports errors only by ``printf("%s: %s\\n", ...)`` on stdout; stdout is flushed after every call so that a test's
    ``capfd`` sees them (``ERROR_LINE`` matches such a line).
Inputs: the reference's float -> unsigned char casts of values outside [0, 255] are undefined behaviour, which the product defines;
every comparison against the product keeps depths in [0, 255]."""
import contextlib
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
CONTRACTS = (0, 1)
ERROR_LINE = re.compile(r"^GPU\w+: ", re.M)          # GPUCheckError's report (src/GPUSolver.cu:20-26)

vp, sz, i32, f32 = C.c_void_p, C.c_size_t, C.c_int, C.c_float
_SYMBOLS = {                                          # the reference's ten functions, Itanium-mangled (tests/golden/reference_mangled_symbols.txt)
    "GPUAllocateDeviceMemory": ("_Z23GPUAllocateDeviceMemoryiii", [i32, i32, i32]),
    "GPUFreeDeviceMemory": ("_Z19GPUFreeDeviceMemoryi", [i32]),
    "GPULoadWeights": ("_Z14GPULoadWeightsf", [f32]),
    "GPUMatrixFreeSolver": ("_Z19GPUMatrixFreeSolverPfmPhmS0_miififi", [vp, sz, vp, sz, vp, sz, i32, i32, f32, i32, f32, i32]),
    "GPUConvertToFloat": ("_Z17GPUConvertToFloatPhmPfmS_mii", [vp, sz, vp, sz, vp, sz, i32, i32]),
    "GPUPyrDownAnnotation": ("_Z20GPUPyrDownAnnotationPhmS_miiS_mS_mii", [vp, sz, vp, sz, i32, i32, vp, sz, vp, sz, i32, i32]),
    "GPUPaintImage": ("_Z13GPUPaintImageiiiiPhmS_mii", [i32, i32, i32, i32, vp, sz, vp, sz, i32, i32]),
    "GPUSimulateDefocus": ("_Z18GPUSimulateDefocusPhmPfmS_mii", [vp, sz, vp, sz, vp, sz, i32, i32]),
    "GPUSimulateDesaturation": ("_Z23GPUSimulateDesaturationPhmS_mPfmS_mii", [vp, sz, vp, sz, vp, sz, vp, sz, i32, i32]),
    "GPUSimulateHaze": ("_Z15GPUSimulateHazePhmPfmS_mii", [vp, sz, vp, sz, vp, sz, i32, i32]),
}


def path(contract):
    return os.path.join(REF_DIR, f"libref_c{contract}.so")


def available():
    return all(os.path.exists(path(c)) for c in CONTRACTS)


def level_shape(rows, cols, level):
    """The size GPUAllocateDeviceMemory(rows, cols, ...) gives level `level`: int / powf in binary32, truncated."""
    s = np.float32(2.0) ** np.float32(level)
    return int(np.float32(rows) / s), int(np.float32(cols) / s)


def _img(t, rows, cols, dtype, channels, what):
    """(pointer, pitch in bytes) of a pitched device image that holds at least rows x cols (x channels) pixels."""
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda, f"{what}: a device tensor is required"
    assert t.dtype == dtype, f"{what}: {t.dtype}, expected {dtype}"
    if channels == 1:
        assert t.dim() == 2 and t.stride(1) == 1, f"{what}: rows must be contiguous"
    else:
        assert t.dim() == 3 and t.shape[2] == channels and t.stride(2) == 1 and t.stride(1) == channels, f"{what}: pixels must be interleaved"
    assert 0 < rows <= t.shape[0] and 0 < cols <= t.shape[1], f"{what}: {rows}x{cols} does not fit a {tuple(t.shape)} image"
    return vp(t.data_ptr()), sz(t.stride(0) * t.element_size())


class RefLib:
    def __init__(self, contract, library=None):
        """`library`: another loaded library exporting the same ten symbols (librtdd.so's drop-in shim), driven through the same
        checks; by default libref_c{contract}.so."""
        import torch   # noqa: F401 -- torch's HIP runtime first, so the library binds to it (as realtimedepthdiffusion_amd.lib() does)
        if library is None and not os.path.exists(path(contract)):
            raise FileNotFoundError(f"{path(contract)} is not built (oracle.build_ref needs the reference tree)")
        self.contract = contract
        self._L = library if library is not None else C.CDLL(path(contract))
        self._libc = C.CDLL(None)
        self._f = {}
        for name, (sym, args) in _SYMBOLS.items():
            f = getattr(self._L, sym)
            f.argtypes = args; f.restype = None
            self._f[name] = f
        self.alloc = None                             # (rows, cols, levels) of the live allocation

    def _call(self, name, *args):
        import torch
        torch.cuda.synchronize()                      # inputs written on torch's stream are complete
        self._f[name](*args)
        torch.cuda.synchronize()                      # the reference's launches on the null stream are complete
        self._libc.fflush(None)                       # its printf'd errors reach the test's capfd now

    # ---- include/GPUSolver.h
    @contextlib.contextmanager
    def allocated(self, rows, cols, levels):
        assert self.alloc is None, f"an allocation {self.alloc} is live: the reference would leak it"
        assert rows > 0 and cols > 0 and levels > 0
        self._call("GPUAllocateDeviceMemory", rows, cols, levels)
        self.alloc = (rows, cols, levels)
        try:
            yield self
        finally:
            self._call("GPUFreeDeviceMemory", levels)
            self.alloc = None

    def GPULoadWeights(self, beta):
        self._call("GPULoadWeights", beta)

    def GPUMatrixFreeSolver(self, depthImage, scribbleImage, grayImage, rows, cols, beta, maxIterations, tolerance, level):
        import torch
        assert self.alloc is not None, "GPUMatrixFreeSolver outside allocated()"
        R, Cc, levels = self.alloc
        assert 0 <= level < levels, f"level {level} of an allocation of {levels}"
        lr, lc = level_shape(R, Cc, level)
        assert 0 < rows <= lr and 0 < cols <= lc, f"{rows}x{cols} exceeds level {level}'s buffers ({lr}x{lc}) of the allocation {self.alloc}"
        self._call("GPUMatrixFreeSolver", *_img(depthImage, rows, cols, torch.float32, 1, "depth"),
                   *_img(scribbleImage, rows, cols, torch.uint8, 1, "scribble"), *_img(grayImage, rows, cols, torch.uint8, 1, "gray"),
                   rows, cols, beta, maxIterations, tolerance, level)

    # ---- include/GPUImageProcessing.h
    def GPUConvertToFloat(self, src, dst, mask, rows, cols):
        import torch
        self._call("GPUConvertToFloat", *_img(src, rows, cols, torch.uint8, 3, "src"), *_img(dst, rows, cols, torch.float32, 1, "dst"),
                   *_img(mask, rows, cols, torch.uint8, 1, "mask"), rows, cols)

    def GPUPyrDownAnnotation(self, prevScribbleImage, prevEditedImage, previousRows, previousCols,
                             currScribbleImage, currEditedImage, currentRows, currentCols):
        import torch
        self._call("GPUPyrDownAnnotation", *_img(prevScribbleImage, previousRows, previousCols, torch.uint8, 1, "prev scribble"),
                   *_img(prevEditedImage, previousRows, previousCols, torch.uint8, 3, "prev edited"), previousRows, previousCols,
                   *_img(currScribbleImage, currentRows, currentCols, torch.uint8, 1, "curr scribble"),
                   *_img(currEditedImage, currentRows, currentCols, torch.uint8, 3, "curr edited"), currentRows, currentCols)

    def GPUPaintImage(self, x, y, scribbleColor, scribbleRadius, editedImage, scribbleImage, rows, cols):
        import torch
        self._call("GPUPaintImage", x, y, scribbleColor, scribbleRadius, *_img(editedImage, rows, cols, torch.uint8, 3, "edited"),
                   *_img(scribbleImage, rows, cols, torch.uint8, 1, "scribble"), rows, cols)

    # ---- include/GPUDepthEffect.h
    def GPUSimulateDefocus(self, originalImage, depthImage, artisticImage, rows, cols):
        import torch
        self._call("GPUSimulateDefocus", *_img(originalImage, rows, cols, torch.uint8, 3, "original"),
                   *_img(depthImage, rows, cols, torch.float32, 1, "depth"), *_img(artisticImage, rows, cols, torch.uint8, 3, "artistic"), rows, cols)

    def GPUSimulateDesaturation(self, originalImage, grayImage, depthImage, artisticImage, rows, cols):
        import torch
        self._call("GPUSimulateDesaturation", *_img(originalImage, rows, cols, torch.uint8, 3, "original"),
                   *_img(grayImage, rows, cols, torch.uint8, 1, "gray"), *_img(depthImage, rows, cols, torch.float32, 1, "depth"),
                   *_img(artisticImage, rows, cols, torch.uint8, 3, "artistic"), rows, cols)

    def GPUSimulateHaze(self, originalImage, depthImage, artisticImage, rows, cols):
        import torch
        self._call("GPUSimulateHaze", *_img(originalImage, rows, cols, torch.uint8, 3, "original"),
                   *_img(depthImage, rows, cols, torch.float32, 1, "depth"), *_img(artisticImage, rows, cols, torch.uint8, 3, "artistic"), rows, cols)
