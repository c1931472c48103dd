"""The reference side of adaptive supersampling (rtc_ctx_render_adaptive, include/rtc.h): the mask of contrast
edges and the composition of the base frame with the supersampled one, in numpy.

    M[p] = any over the up to four neighbours n of p inside the frame (x +- 1, y +- 1) and the channels c of
           fabsf(B[p][c] - B[n][c]) > threshold
    O[p] = S[p] where M[p], else B[p]

Written with explicit float32 slice operations, as supersample_helpers.box_filter is: numpy subtracts two float32 arrays
element by element in float32, one rounding per subtraction; `>` with a NaN on either side is False, so a NaN difference
(NaN operands, inf - inf) never flags.  The k x k value S itself is box_filter's -- DESIGN.md 8b item (3), the one
definition of the reduction's order."""
import numpy as np

f32 = np.float32


def edge_mask(B, threshold):
    """(H, W, C) float32 -> (H, W) bool."""
    B = np.ascontiguousarray(B, dtype=f32)
    assert B.ndim == 3 and B.dtype == f32  # (float32 in, float32 differences out)
    t = f32(threshold)
    M = np.zeros(B.shape[:2], dtype=bool)
    with np.errstate(invalid="ignore"):  # inf - inf
        dx = (np.abs(B[:, 1:] - B[:, :-1]) > t).any(axis=2)  # pixel (y, x) against (y, x + 1)
        dy = (np.abs(B[1:] - B[:-1]) > t).any(axis=2)        # pixel (y, x) against (y + 1, x)
    # symmetric: both pixels of a contrasting pair
    M[:, :-1] |= dx
    M[:, 1:] |= dx
    M[:-1] |= dy
    M[1:] |= dy
    return M


def compose(B, S, M):
    """O = S where M, else B (a copy)."""
    B, S = np.asarray(B, dtype=f32), np.asarray(S, dtype=f32)
    assert B.shape == S.shape and M.shape == B.shape[:2] and M.dtype == bool
    out = B.copy()
    out[M] = S[M]
    return out
