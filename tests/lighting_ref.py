"""Two restatements of rtdd_simulate_lighting (include/rtdd.h) for the tests, composed of the restatements of the calls it fuses:
`lighting` in vectorised numpy float32 from relight_ref.shade, shadow_ref.visibility, ao_ref.ambient and relight_ref.channel_gains, and
`lighting_literal`, a per-pixel loop over the header's output line, every intermediate an np.float32 scalar, from
relight_shadowed_literal's vis and ambient_literal's ao.  Every operation is one f32 operation rounded once, in the header's order:
    out_c = (uchar) fminf(o_c * ((ambient * ao) + (k_c * (shade * vis))), 255)
Neither knows about the kernel.  `rows=(y0, y1)` restates a band of rows only, on the whole map.  Test infrastructure."""
import numpy as np

from ao_ref import SHADE, ambient, ambient_literal
from relight_ref import F, channel_gains, shade
from shadow_ref import relight_shadowed_literal, visibility


def lighting(orig, depth, L, S, A, rows=None):
    """rtdd_simulate_lighting's image (rows=None), or its rows [y0, y1)."""
    depth = np.asarray(depth, F)
    assert A["mode"] == SHADE and F(L["relief"]) == F(A["relief"])
    y0, y1 = rows if rows is not None else (0, depth.shape[0])
    lit = shade(depth, L)[y0:y1] * visibility(depth, L, S, rows)
    amb = F(L["ambient"]) * ambient(depth, A, rows)
    assert lit.dtype == F and amb.dtype == F
    out = np.empty((y1 - y0, depth.shape[1], 3), np.uint8)
    for c, k in enumerate(channel_gains(L)):
        v = np.fmin(orig[y0:y1, :, c].astype(F) * (amb + (k * lit)), F(255))
        assert v.dtype == F
        out[..., c] = v.astype(np.int32).astype(np.uint8)
    return out


def lighting_literal(orig, depth, L, S, A):
    """The header's output line, one pixel at a time; vis and ao are the literal restatements' of the two calls."""
    depth = np.asarray(depth, F)
    assert A["mode"] == SHADE and F(L["relief"]) == F(A["relief"])
    rows, cols = depth.shape
    vis = np.empty((rows, cols), F)
    relight_shadowed_literal(orig, depth, L, S, vis_out=vis)
    ao = ambient_literal(depth, A)
    s_all = shade(depth, L)                                       # relight's shade (pinned against its own literal loop by test_relight_cpu.py)
    amb0, ks = F(L["ambient"]), channel_gains(L)
    out = np.empty((rows, cols, 3), np.uint8)
    for y in range(rows):
        for x in range(cols):
            lit = F(F(s_all[y, x]) * F(vis[y, x]))
            amb = F(amb0 * F(ao[y, x]))
            for c in range(3):
                v = F(F(orig[y, x, c]) * F(amb + F(ks[c] * lit)))
                out[y, x, c] = int(min(v, F(255)))
    return out
