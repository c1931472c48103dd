"""Worlds, cameras and reference values for the sweep of rectangle-light grids (tests/test_gpu_light_grids.py).

Every shortcut of the light sample loop works on the light's u_steps x v_steps grid: the whole-light cull (from 8 cells), the block
cones (both counts even, any number of cells), own-sphere blocks, lanes sharing a shade point's cells, the supersampled and the
adaptive refinement.  The shapes below sit on every such property: a step count of 1, the 8-cell threshold from both sides with a
1 in it, odd and even counts, grids longer than a wave's share of cells, more cells than any other test has.

The worlds are built through the product API and mirrored with tests.helpers.oracle_world; the oracle's frames are rendered
once per (world, shape, frame) and handed out read-only."""
import os

import numpy as np

import ray_tracer_challenge_amd as P
from tests import helpers as H
from tests import hits_helpers as HH
from tests.supersample_helpers import box_filter

f32 = np.float32
THREADS = min(16, len(os.sched_getaffinity(0)))

SHAPES = [(1, 1), (1, 7), (7, 1), (1, 8), (8, 1), (2, 4), (4, 2), (2, 2), (3, 3), (5, 2), (1, 64), (64, 1), (16, 16), (2, 130), (130, 2),
          (33, 32), (64, 64)]
SHORT = [(1, 8), (8, 1), (3, 3), (1, 64), (16, 16), (2, 130)]
FRAME, SMALL_FRAME = (24, 16), (8, 8)
DEPTH, MIRROR_DEPTH = 5, 7  # the reference's default (constants.rs:4); the mirrors: 8 shade points per pixel
FAR = 1000.0
JITTER = ("hashed", 0x51DE)
CULL_THRESHOLD = 8  # cells from which the whole-light cull and lane sharing apply (rtc_kernel_core.h light_cull_mask, rtc_scene_prep.h choose_share_log2)


def shape_id(shape):
    return "%dx%d" % shape


def cells(shape):
    return shape[0] * shape[1]


def light(shape, dx=0.0, jitter=JITTER):
    """2 x 2 units, 4 above the floor, centred over (dx, 0)."""
    return P.RectangleLight(P.color(1.1, 1.0, 0.9), P.point(dx - 1.0, 4.0, -1.0), P.vector(2.0, 0.0, 0.0), shape[0], P.vector(0.0, 0.0, 2.0), shape[1], jitter)


def _matte(r, g, b, **kw):
    return P.Material(color=(r, g, b), ambient=0.1, diffuse=0.8, specular=0.0, **kw)


def spheres(shape, dx=0.0, jitter=JITTER):
    """A non-casting matte floor and two casting, uniformly scaled spheres, one of them mirrored: the unrolled flat kernel with the
    fast shadow decision, block cones (even grids) and own-sphere blocks."""
    floor = P.Plane(None, _matte(0.9, 0.9, 0.85), casts_shadow=False)
    ball = P.Sphere(P.translation(dx, 1.0, 0.0), _matte(0.8, 0.3, 0.3))
    mirrored = P.Sphere(P.chain(P.translation(dx + 1.7, 0.6, 1.3), P.scaling(-0.6, -0.6, -0.6)), _matte(0.3, 0.4, 0.8))
    return P.World([floor, ball, mirrored], light(shape, dx, jitter))


def medley(shape, dx=0.0, jitter=JITTER):
    """Casters that are not all spheres -- a cube, a bounded cylinder, a cone (which the cull always keeps: casters_left) -- on a
    casting floor: no block cones, the general kernel's exact shadow decision."""
    floor = P.Plane(None, _matte(0.85, 0.9, 0.85))
    cube = P.Cube(P.chain(P.translation(dx - 1.3, 0.5, 0.4), P.rotation_y(0.5), P.scaling(0.5, 0.5, 0.5)), _matte(0.8, 0.6, 0.2))
    cyl = P.Cylinder(P.chain(P.translation(dx + 1.4, 0.0, 0.9), P.scaling(0.5, 1.0, 0.5)), _matte(0.2, 0.7, 0.5), minimum_y=0.0, maximum_y=1.3, closed=True)
    cone = P.Cone(P.chain(P.translation(dx + 0.1, 1.4, -0.5), P.scaling(0.6, 1.4, 0.6)), _matte(0.6, 0.3, 0.7), minimum_y=-1.0, maximum_y=0.0, closed=True)
    return P.World([floor, cube, cyl, cone], light(shape, dx, jitter))


def group(shape, dx=0.0, jitter=JITTER):
    """A GroupShape of four spheres over the floor: the traversal kernel."""
    kids = [P.Sphere(P.chain(P.translation(dx + x, y, z), P.scaling(r, r, r)), _matte(*c))
            for x, y, z, r, c in ((-1.1, 0.7, 0.2, 0.7, (0.8, 0.3, 0.3)), (0.9, 0.5, -0.6, 0.5, (0.3, 0.8, 0.3)), (0.4, 1.6, 0.8, 0.4, (0.3, 0.3, 0.8)),
                                  (1.9, 0.3, 1.2, 0.3, (0.8, 0.8, 0.3)))]
    floor = P.Plane(None, _matte(0.9, 0.85, 0.9))
    return P.World([floor, P.GroupShape.with_children(kids)], light(shape, dx, jitter))


def casterless(shape, dx=0.0, jitter=JITTER):
    """The floor alone, non-casting: every shade point's samples are answered at once (LIGHT_CULL_ALL_CASTERS)."""
    return P.World([P.Plane(None, _matte(0.9, 0.9, 0.9), casts_shadow=False)], light(shape, dx, jitter))


def mirrors(shape, dx=0.0, jitter=JITTER):
    """Two facing, non-casting, fully reflective planes with the light between them: every ray is reflected until the depth runs
    out -- depth + 1 shade points per pixel."""
    mirror = _matte(0.9, 0.9, 0.9, reflective=1.0)
    return P.World([P.Plane(None, mirror, casts_shadow=False), P.Plane(P.translation(0.0, 6.0, 0.0), mirror, casts_shadow=False)], light(shape, dx, jitter))


# ("spheres_open": the spheres' world seen by a camera that looks at open floor only, ten units to their right)
WORLDS = {"spheres": (spheres, 0.0), "spheres_far": (spheres, FAR), "spheres_open": (spheres, 0.0), "medley": (medley, 0.0), "group": (group, 0.0),
          "casterless": (casterless, 0.0), "mirrors": (mirrors, 0.0)}
# the kernel family of each world: the ahead-of-time kernel's template arguments (rtc_scene_prep.h KernelFamily::name).  A tree as
# small as `group` would be rendered by the unrolled flat kernel with its group as a gate: the sweep switches the gates off
# (RTC_AMD_GATES=0, SWITCHES_OF) and so walks the traversal stream.
FAMILY = {"spheres": "4,simple", "spheres_far": "4,simple", "spheres_open": "4,simple", "medley": "4,general", "group": "tree", "casterless": "4,simple",
          "mirrors": "4,simple"}
SWITCHES_OF = {"group": {"GATES": 0}}


def world(name, shape, jitter=JITTER):
    make, dx = WORLDS[name]
    return make(shape, dx, jitter)


def camera(name, size=FRAME):
    """From above and in front, every pixel floor or object.  At 24 x 16 the objects and their shadows fill the left two thirds of
    the frame -- a fifth of the pixels of `spheres` lie in a penumbra -- and the two wave tiles on the right are open floor, where
    the whole-light cull and the block cones answer for the whole wave."""
    dx = WORLDS[name][1]
    if name == "mirrors":  # between the planes, looking down at an angle: every ray meets the floor, then the ceiling, ...
        return P.Camera(size[0], size[1], 0.8, P.view_transform(P.point(dx, 3.0, -4.0), P.point(dx, 0.0, 0.0), P.vector(0, 1, 0)))
    if name == "spheres_open":  # every pixel open floor from which the whole light is seen clear of both spheres, by a wide margin
        return P.Camera(size[0], size[1], 0.6, P.view_transform(P.point(dx + 10.0, 4.0, -3.0), P.point(dx + 10.0, 0.0, 0.5), P.vector(0, 1, 0)))
    return P.Camera(size[0], size[1], 1.0, P.view_transform(P.point(dx + 1.5, 4.5, -5.0), P.point(dx + 1.5, 0.3, 0.6), P.vector(0, 1, 0)))


def assert_kernel(name, kernel_name, specialised, prefix="render_kernel"):
    """The kernel family that ran, from its name -- so that a cell of the sweep cannot silently test another kernel.
    prefix: render_kernel, ss_render_kernel, trace_kernel or adaptive_refine_kernel."""
    family = FAMILY[name]
    if specialised:  # render_kernel_spec[<the objects' words, or tree...>;simple...]
        assert kernel_name.startswith(prefix + "_spec[" + ("tree" if family == "tree" else "0x")), (name, kernel_name)
        assert (";simple" in kernel_name) == family.endswith("simple"), (name, kernel_name)
    else:            # render_kernel<4,simple> (supersampled: <4,simple;ss=2>)
        head = prefix + "<" + family
        assert kernel_name.startswith(head) and kernel_name[len(head):len(head) + 1] in (">", ";"), (name, kernel_name)


# ---------------------------------------------------------------- the oracle's frames, once each
_frames = {}


def oracle_frame(name, shape, size=FRAME, depth=DEPTH, k=1):
    """-> (frame, rays) of the oracle for `camera(name, size)` (k > 1: its fine camera, camera.supersampled(k)); read-only."""
    key = (name, shape, size, depth, k)
    if key not in _frames:
        cam = camera(name, size)
        img, rays = H.oracle_camera(cam if k == 1 else cam.supersampled(k)).render(H.oracle_world(world(name, shape)), depth, threads=THREADS)
        img.setflags(write=False)
        _frames[key] = (img, rays)
    return _frames[key]


def oracle_filtered(name, shape, k, size=FRAME, depth=DEPTH):
    fine, rays = oracle_frame(name, shape, size, depth, k)
    return box_filter(fine, k), rays


def traced_pixels(size):
    """camera.rs:80-81: the last row and column are never traced"""
    return (size[0] - 1) * (size[1] - 1)


def oracle_shaded_hits(name, shape, size=FRAME, depth=DEPTH):
    """shade_hit evaluations of the oracle's frame, from its ray count alone (the oracle counts rays, not shade points).  Every
    color_at is one ray and every shade point adds one ray per cell: rays = calls + shaded x cells.  A world in which nothing
    reflects or transmits makes one call per traced pixel.  Between the mirrors no ray misses -- every call is a shade point, depth + 1
    of them per traced pixel -- so rays = shaded x (cells + 1): the division must come out even, and at that count."""
    _, rays = oracle_frame(name, shape, size, depth)
    n = cells(shape)
    if name == "mirrors":
        shaded, rest = divmod(rays, n + 1)
        assert rest == 0 and shaded == (depth + 1) * traced_pixels(size), (name, shape, rays, shaded, rest)
        return shaded
    shaded, rest = divmod(rays - traced_pixels(size), n)
    assert rest == 0 and 0 <= shaded <= traced_pixels(size), (name, shape, rays, shaded, rest)
    return shaded


# ---------------------------------------------------------------- the condition that keeps the sweep honest
def probe_points(name):
    """24 x 16 points over the floor rectangle -3 <= x <= 3, -2 <= z <= 4 (x offset by the world's translation), 1e-3 above the plane:
    a point exactly on a non-casting plane is always lit by the reference's nearest-hit rule."""
    dx = WORLDS[name][1]
    xs, zs = np.linspace(-3.0, 3.0, 24), np.linspace(-2.0, 4.0, 16)
    return np.array([[dx + x, 1e-3, z, 1.0] for z in zs for x in xs], dtype=f32)


_penumbra = {}


def oracle_light_at_probes(name, shape):
    """The oracle's intensity_at of every probe point, point i drawing as pixel i; read-only."""
    if (name, shape) not in _penumbra:
        own, pts = H.oracle_world(world(name, shape)), probe_points(name)
        out = np.zeros(len(pts), dtype=f32)
        for i in range(len(pts)):
            own.set_pixel(i)
            out[i] = own.intensity_at(pts[i])
        out.setflags(write=False)
        _penumbra[name, shape] = out
    return _penumbra[name, shape]


def assert_penumbra(name, shape):
    """On the oracle alone: at least a tenth of the probe points have a light fraction strictly between 0 and 1 (every shape but
    1 x 1, whose fraction is 0 or 1 by construction).  A world whose points are all fully lit or fully dark proves nothing about
    the sample loop."""
    li = oracle_light_at_probes(name, shape)
    partial = int(((li > 0.0) & (li < 1.0)).sum())
    if shape != (1, 1):
        assert 10 * partial >= len(li), "%s %s: only %d of %d probe points lie in a penumbra" % (name, shape_id(shape), partial, len(li))
    assert (li == 1.0).any() and (li < 1.0).any(), (name, shape)
    return partial


def oracle_light_plane(name, shape, size=FRAME):
    """The oracle's intensity_at(over_point) of every pixel's first hit, as Renderer.render_hits' light plane has it ((h, w);
    the untraced last row and column and the misses hold 0), and the object plane beside it."""
    cam = camera(name, size)
    o, d = HH.camera_rays(cam)
    w, h = size
    traced = np.array([y * w + x for y in range(h - 1) for x in range(w - 1)], dtype=np.int64)
    exp = HH.empty_planes(w * h, ("object", "light"))
    part = HH.oracle_first_hits(H.oracle_world(world(name, shape)), o[traced], d[traced], pixels=traced)
    exp["object"][traced], exp["light"][traced] = part["object"], part["light"]
    return exp["light"].reshape(h, w), exp["object"].reshape(h, w)


def check_counts(st, shape, what=""):
    """What holds in every test of the sweep: of the rays, shade points x cells are shadow rays, and of those some were answered
    without a test."""
    assert st["culled_shadow_rays"] <= st["shaded_hits"] * cells(shape) <= st["rays"], (what, st)
