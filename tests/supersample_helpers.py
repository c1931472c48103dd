"""The reference side of supersampled rendering (rtc_ctx_set_scene_ss, include/rtc.h): the fixed-order f32 box filter that
defines the supersampled frame.  Output pixel (X, Y), per channel, is a pairwise tree over its k x k block of the fine
frame F, along x first, then along y:

    k = 2: ((F[2Y][2X] + F[2Y][2X+1]) + (F[2Y+1][2X] + F[2Y+1][2X+1])) * 0.25f
    k = 4: per row r = (a0 + a1) + (a2 + a3), then ((r0 + r1) + (r2 + r3)) * 0.0625f

Written with explicit float32 slice additions: numpy adds two float32 arrays element by element in float32, one rounding per
addition, nothing fused.  (np.sum is NOT this: its order is pairwise over the flattened axis, or sequential, as it sees fit.)"""
import numpy as np

f32 = np.float32


def box_filter(fine, k):
    """(k H, k W, C) float32 -> (H, W, C) float32, in the contract's order."""
    F = np.ascontiguousarray(fine, dtype=f32)
    assert k in (1, 2, 4), k
    assert F.ndim == 3 and F.shape[0] % k == 0 and F.shape[1] % k == 0, (F.shape, k)
    if k == 1:
        return F.copy()
    a = [F[:, i::k] for i in range(k)]  # along x
    r = a[0] + a[1] if k == 2 else (a[0] + a[1]) + (a[2] + a[3])
    b = [r[j::k] for j in range(k)]  # then along y
    s = b[0] + b[1] if k == 2 else (b[0] + b[1]) + (b[2] + b[3])
    out = s * f32(0.25 if k == 2 else 0.0625)
    assert out.dtype == f32
    return out


def assemble_partitions(parts, height, band_rows, n_parts):
    """The whole frame from the compact rows of its partitions (band b belongs to part b mod n_parts)."""
    width = parts[0].shape[1]
    out = np.zeros((height, width, 3), dtype=f32)
    used = [0] * n_parts
    for b, y0 in enumerate(range(0, height, band_rows)):
        p, n = b % n_parts, min(band_rows, height - y0)
        out[y0:y0 + n] = parts[p][used[p]:used[p] + n]
        used[p] += n
    assert all(used[p] == parts[p].shape[0] for p in range(n_parts)), (used, [q.shape for q in parts])
    return out
