"""Ray generators for Renderer.trace / trace_hits: projections the reference's pinhole camera does not have, and the
bounce step from a set of first-hit planes to the next stream (reflected, at the end).

Plain torch, on any device (CPU included).  Each projection returns (origins, directions): (height * width, 4) float32 in image
order -- ray y * width + x is pixel (x, y) -- origins with w = 1, directions with w = 0 and of unit length to within f32
rounding.  The angles and offsets are formed in float64 and rounded once; the directions are then normalised in float32
(three products, two sums, a square root, a division each).

They are inputs, not part of the arithmetic contract: whatever they produce, trace() colours exactly as World::color_at
colours those very rays.
"""
import math

import torch


def _normalize(v):
    """float32 (n, 3) -> unit vectors: v / sqrt((x x + y y) + z z), every operation rounded to float32."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    m = torch.sqrt((x * x + y * y) + z * z)
    return v / m[:, None]


def _pack(origins3, directions3):
    n = directions3.shape[0]
    origins = torch.ones((n, 4), dtype=torch.float32, device=directions3.device)
    origins[:, :3] = origins3
    directions = torch.zeros((n, 4), dtype=torch.float32, device=directions3.device)
    directions[:, :3] = directions3
    return origins, directions


def orthographic(width, height, view_width, transform, device=None):
    """Parallel rays along the camera's -z.  `transform`: the view transform (world -> camera space, what
    scenes.view_transform makes, 4 x 4); the image plane is z = 0 of camera space, view_width world units wide and
    view_width * height / width high, x to the left and y up as the reference's camera has them.  Pixel (x, y) starts at
    the centre of its square."""
    width, height = int(width), int(height)
    if width <= 0 or height <= 0 or not view_width > 0:
        raise ValueError("orthographic: empty view")
    inv = torch.linalg.inv(torch.as_tensor(transform, dtype=torch.float64).reshape(4, 4).cpu()).to(device)
    step = float(view_width) / width
    xs = 0.5 * float(view_width) - (torch.arange(width, dtype=torch.float64, device=device) + 0.5) * step
    ys = 0.5 * step * height - (torch.arange(height, dtype=torch.float64, device=device) + 0.5) * step
    cam = torch.zeros((height, width, 4), dtype=torch.float64, device=device)
    cam[..., 0] = xs[None, :]
    cam[..., 1] = ys[:, None]
    cam[..., 3] = 1.0
    origins3 = (cam.reshape(-1, 4) @ inv.T)[:, :3].to(torch.float32)
    forward = (inv @ torch.tensor([0.0, 0.0, -1.0, 0.0], dtype=torch.float64, device=device))[:3].to(torch.float32)
    direction = _normalize(forward[None, :])  # one vector, normalised once: every ray carries the same bits
    return _pack(origins3, direction.expand(height * width, 3))


def equirectangular(width, height, position, device=None):
    """A full panorama from `position` (x, y, z): longitude along the image's x, from -pi to pi in `width` steps, latitude
    along y from pi / 2 (up, +y) to -pi / 2 in `height` steps, each pixel looking through the centre of its cell.  The
    middle of the image looks along +z, longitude grows towards +x."""
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("equirectangular: empty image")
    lon = -math.pi + (torch.arange(width, dtype=torch.float64, device=device) + 0.5) * (2.0 * math.pi / width)
    lat = 0.5 * math.pi - (torch.arange(height, dtype=torch.float64, device=device) + 0.5) * (math.pi / height)
    d = torch.empty((height, width, 3), dtype=torch.float64, device=device)
    d[..., 0] = torch.cos(lat)[:, None] * torch.sin(lon)[None, :]
    d[..., 1] = torch.sin(lat)[:, None]
    d[..., 2] = torch.cos(lat)[:, None] * torch.cos(lon)[None, :]
    directions3 = _normalize(d.reshape(-1, 3).to(torch.float32))
    p = torch.as_tensor([float(c) for c in list(position)[:3]], dtype=torch.float32, device=device)
    return _pack(p[None, :].expand(height * width, 3), directions3)


def reflected(hits, directions=None):
    """The bounce step: from a dict of first-hit planes (Renderer.trace_hits / render_hits, flattened to one element per ray)
    holding `object`, `over_point` and `reflectv`, the reflection rays of the rays that hit something, compacted in index
    order.  -> (origins (m, 4): over_point, directions (m, 4): reflectv, index (m,) int64: the ray each came from), on the
    planes' device, as they were stored (w included; trace() and trace_hits() read x, y, z).
    `directions` ((n, 4), optional: the directions of the rays that made the hits) is only checked against the planes'
    length; the reflected direction is the stored `reflectv` (world.rs:220), not recomputed from it."""
    for k in ("object", "over_point", "reflectv"):
        if k not in hits:
            raise ValueError("reflected: the planes need %r" % k)
    obj = hits["object"].reshape(-1)
    over, refl = hits["over_point"].reshape(-1, 4), hits["reflectv"].reshape(-1, 4)
    n = obj.shape[0]
    if over.shape[0] != n or refl.shape[0] != n or (directions is not None and directions.reshape(-1, 4).shape[0] != n):
        raise ValueError("reflected: planes and directions of %d rays expected" % n)
    index = torch.nonzero(obj >= 0).reshape(-1)  # int64, ascending
    return over[index].contiguous(), refl[index].contiguous(), index
