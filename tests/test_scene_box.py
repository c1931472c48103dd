"""Two shortcuts for primary rays of fully bounded scenes (rtc_scene_prep.h / render_body): the SCENE BOX -- a ray that
misses the padded box around everything is black after one counted ray, without the exact normalisation and the walk --
and the SCENE RECTANGLE -- where the pixels that can see anything (that box, and the near side of every top-level plane's
horizon) lie within a rectangle smaller than the frame, only that rectangle's blocks are rendered, other workgroups of the
same launch zero-fill the rest, and the rays of the pixels outside are added to the count.  Neither is part of the reference's
semantics (camera.rs:76-91 traces every pixel the same way): every pixel, the ray count and the shaded-hit count must
equal the oracle's and those of a render with the shortcut switched off -- whole frames, ragged sizes, cameras that put
the scene at an edge, partly outside or behind, and the band partitions of the multi-GPU split."""
import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H

pytestmark = pytest.mark.gpu
f32 = np.float32


def _world(n=5, mirror=True):
    objs = []
    rng = np.random.default_rng(n)
    for i in range(n):
        m = P.Material(color=tuple(map(float, rng.uniform(0.2, 1.0, 3))), reflective=0.4 if (mirror and i % 2) else 0.0)
        shape = P.Cube if i % 3 == 2 else P.Sphere
        objs.append(shape(P.chain(P.translation(float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1, 1)), float(rng.uniform(-1.5, 1.5))),
                                  P.scaling(*map(float, rng.uniform(0.3, 0.7, 3)))), m))
    return P.World(objs, P.PointLight(P.point(-6, 8, -9), P.color(1, 1, 1)))


CAMERAS = {
    # (size, from, to, field of view): where the scene's rectangle falls
    "centre": ((401, 297), (0, 1, -14), (0, 0, 0), np.pi / 3),
    "corner": ((390, 310), (0, 1, -14), (6.5, -4.5, 0), np.pi / 3),          # the scene in the upper left corner, cut by the frame
    "edge_strip": ((640, 130), (0, 0.5, -20), (9.0, 0, 0), np.pi / 2.5),     # a wide frame, the scene at its left edge
    "tiny": ((333, 333), (0, 2, -60), (0, 0, 0), np.pi / 4),                 # a few tiles in the middle
    "inside": ((200, 150), (0.1, 0.2, 0.0), (1, 0.3, 1), np.pi / 2),         # the camera inside the box: no rectangle
    "looking_away": ((260, 200), (0, 1, -6), (0, 1, -20), np.pi / 3),        # everything behind the camera: all black
}


def _render(world, camera, depth, env, monkeypatch, parts=None):
    for k in ("RTC_AMD_SCENE_BOX", "RTC_AMD_SCENE_RECT", "RTC_AMD_SCENE_TILES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = Renderer(world, camera, device=0)
    if parts is None:
        img = r.render(depth).cpu().numpy()
        st = r.stats()
        counts = (st["rays"], st["shaded_hits"])
    else:
        n, band = parts
        img = np.zeros((camera.height, camera.width, 3), f32)
        rays = shaded = 0
        for p in range(n):
            got = r.render(depth, part=Renderer.partition(band, n, p)).cpu().numpy()
            st = r.stats()
            rays += st["rays"]
            shaded += st["shaded_hits"]
            cursor = 0
            for b in range(p, (camera.height + band - 1) // band, n):
                y0, y1 = b * band, min((b + 1) * band, camera.height)
                img[y0:y1] = got[cursor:cursor + (y1 - y0)]
                cursor += y1 - y0
        counts = (rays, shaded)
    r.close()
    return img, counts


@pytest.mark.parametrize("specialise", ["0", "1"])
@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_scene_box_and_rectangle_change_nothing(cam, specialise, monkeypatch):
    (w, h), frm, to, fov = CAMERAS[cam]
    world = _world()
    camera = P.Camera(w, h, float(fov), P.view_transform(P.point(*frm), P.point(*to), P.vector(0, 1, 0)))
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), 3, threads=8)
    base, base_counts = _render(world, camera, 3, {"RTC_AMD_SCENE_BOX": "0", "RTC_AMD_SCENE_RECT": "0"}, monkeypatch)
    H.assert_images_equal(base, exp, "%s: no shortcuts" % cam)
    assert base_counts[0] == rays
    for name, env in (("box only", {"RTC_AMD_SCENE_RECT": "0", "RTC_AMD_SCENE_TILES": "0"}), ("default", {}), ("no tile lists", {"RTC_AMD_SCENE_TILES": "0"}),
                      ("rectangle whatever its size", {"RTC_AMD_SCENE_RECT": "2", "RTC_AMD_SCENE_TILES": "0"})):
        img, counts = _render(world, camera, 3, env, monkeypatch)
        H.assert_images_equal(img, exp, "%s: %s" % (cam, name))
        assert counts == base_counts, (cam, name)
    # the multi-GPU split: rows dealt out in bands, every part launches its own share of the rectangle
    for parts in ((3, 16), (2, 64), (5, 48)):
        for env in ({"RTC_AMD_SCENE_RECT": "2", "RTC_AMD_SCENE_TILES": "0"}, {}):  # (the rectangle per part; tile lists per part where the scene has them)
            img, counts = _render(world, camera, 3, env, monkeypatch, parts=parts)
            H.assert_images_equal(img, exp, "%s: %d parts of %d-row bands %s" % ((cam,) + parts + (env,)))
            assert counts == base_counts, (cam, parts, env)


PLANE_CAMERAS = {
    # (size, from, to, up, field of view) over a floor (and for some a wall) plane: where the horizon falls
    "horizon_mid": ((402, 300), (0, 2, -10), (0, 1.5, 0), (0, 1, 0), np.pi / 3),
    "rolled": ((391, 283), (0, 2, -10), (0, 1.0, 0), (0.5, 1, 0.1), np.pi / 3),        # the horizon is a slanted line
    "looking_up": ((300, 220), (0, 1, -6), (0, 9, 0), (0, 1, 0), np.pi / 4),          # the floor below the frame: only the box
    "looking_down": ((280, 260), (0, 8, -3), (0, 0, 0), (0, 0, 1), np.pi / 3),        # floor everywhere
    "under_the_floor": ((260, 200), (0, -3, -8), (0, 2, 0), (0, 1, 0), np.pi / 3),    # camera on the floor's other side
    "grazing": ((420, 120), (0, 0.02, -10), (0, 0.02, 0), (0, 1, 0), np.pi / 2.2),    # eye almost in the plane
}


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("cam", sorted(PLANE_CAMERAS))
def test_rectangle_with_planes_changes_nothing(cam, wall, monkeypatch):
    """Top-level planes: a primary ray sees a plane only on one side of its horizon, so the scene rectangle is the box of
    the bounded objects plus that side (mark_plane_side).  A rolled camera, a camera under the floor, one that looks away
    from it, one almost in it; a second plane (a tilted wall) whose horizon crosses the first's."""
    (w, h), frm, to, up, fov = PLANE_CAMERAS[cam]
    world = _world(4)
    objs = list(world.objects)
    objs.insert(1, P.Plane(P.identity_4x4(), P.Material(color=(0.7, 0.7, 0.6), reflective=0.3)))
    if wall:
        objs.append(P.Plane(P.chain(P.translation(0, 0, 6), P.rotation_y(f32(0.4)), P.rotation_x(f32(np.pi / 2.3))), P.Material(color=(0.3, 0.5, 0.8))))
    world = P.World(objs, world.light)
    camera = P.Camera(w, h, float(fov), P.view_transform(P.point(*frm), P.point(*to), P.vector(*up)))
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), 3, threads=8)
    off, off_counts = _render(world, camera, 3, {"RTC_AMD_SCENE_RECT": "0"}, monkeypatch)
    H.assert_images_equal(off, exp, "%s: whole grid" % cam)
    assert off_counts[0] == rays
    # (RTC_AMD_SCENE_RECT=2: the rectangle is launched whatever its share of the frame -- by default only under half of it)
    for env in ({}, {"RTC_AMD_SCENE_RECT": "2"}):
        on, on_counts = _render(world, camera, 3, env, monkeypatch)
        H.assert_images_equal(on, exp, "%s: rectangle %s" % (cam, env))
        assert on_counts == off_counts
    for parts in ((3, 16), (2, 64)):
        img, counts = _render(world, camera, 3, {"RTC_AMD_SCENE_RECT": "2"}, monkeypatch, parts=parts)
        H.assert_images_equal(img, exp, "%s: %d parts of %d-row bands" % ((cam,) + parts))
        assert counts == off_counts, (cam, parts)


def test_rectangle_with_the_librarys_own_hierarchy(monkeypatch):
    """C5's shape at a ragged size: 64 spheres (flat world, internal hierarchy, scene box, scene rectangle) from far away."""
    from ray_tracer_challenge_amd import scenes
    world, _, depth = scenes.sphere_grid(64, 64)
    camera = P.Camera(517, 389, float(np.pi / 3), P.view_transform(P.point(0, 30, -40), P.point(4, 0, 7), P.vector(0, 1, 0)))
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=8)
    off, off_counts = _render(world, camera, depth, {"RTC_AMD_SCENE_RECT": "0", "RTC_AMD_SCENE_TILES": "0"}, monkeypatch)
    rect, rect_counts = _render(world, camera, depth, {"RTC_AMD_SCENE_TILES": "0"}, monkeypatch)
    on, on_counts = _render(world, camera, depth, {}, monkeypatch)
    H.assert_images_equal(off, exp, "whole grid")
    H.assert_images_equal(rect, exp, "rectangle")
    H.assert_images_equal(on, exp, "tile list (zero-fill + the tiles the spheres project to)")
    assert on_counts == off_counts == rect_counts and on_counts[0] == rays
    for parts in ((4, 32), (3, 64), (2, 16)):
        img, counts = _render(world, camera, depth, {}, monkeypatch, parts=parts)
        H.assert_images_equal(img, exp, "tile lists, %d parts of %d-row bands" % parts)
        assert counts == on_counts


@pytest.mark.parametrize("specialise", ["0", "1"])
def test_thin_discs_seen_from_thousands_of_their_own_units(specialise, monkeypatch):
    """ERROR_BUDGET.md B8 / E2: a sphere scaled 1e-2 .. 1e-3 across, seen from twenty units, is thousands of its OWN units from the
    camera, and the reference's f32 quadratic reports hits for lines that pass radii away from it -- two thirds of this frame's lit
    pixels lie outside the discs' true silhouettes.  A world-space padding cannot hold those (round 4's wide fuzz found three such
    worlds, all cured by RTC_AMD_SCENE_BOX=0); the box, the rectangle and the tile list now stand down for a leaf the camera
    is more than ~100 of its own units from.  Whatever is switched on or off, the frame is the oracle's."""
    m = P.Material(color=(0.3, 0.9, 0.3), ambient=0.3, diffuse=0.7, specular=0.0)
    objs = [P.Sphere(P.chain(P.translation(0.0, 0.0, 0.0), P.rotation_y(0.9), P.rotation_x(0.4), P.scaling(0.6, 0.6, 0.007)), m),
            P.Sphere(P.chain(P.translation(2.5, 1.0, 1.0), P.rotation_x(1.2), P.scaling(0.6, 0.0024, 0.6)), m),
            P.Cube(P.chain(P.translation(-2.5, -1.0, 0.5), P.rotation_y(0.3), P.scaling(0.6, 0.55, 0.007)), m)]
    world = P.World(objs, P.PointLight(P.point(-5, 8, -20), P.color(1, 1, 1)))
    camera = P.Camera(160, 120, 0.7, P.view_transform(P.point(-5, 5, -20), P.point(0, 0, 0), P.vector(0, 1, 0)))
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), 1, threads=8)
    assert (exp.sum(axis=2) > 0).sum() > 500  # (the discs' true silhouettes cover 176 pixels, the plate some 150)
    for env in ({}, {"RTC_AMD_SCENE_BOX": "0", "RTC_AMD_SCENE_RECT": "0", "RTC_AMD_SCENE_TILES": "0"}, {"RTC_AMD_SCENE_RECT": "2"}):
        img, counts = _render(world, camera, 1, env, monkeypatch)
        H.assert_images_equal(img, exp, "thin discs %s" % env)
        assert counts[0] == rays
    # ... and the same discs many to a frame (the library's own hierarchy asks for a scene within 100 of its SMALLEST half-axis: not built)
    many = [P.Sphere(P.chain(P.translation(float(i % 5) - 2.0, float(i // 5) - 1.5, 0.0), P.rotation_y(0.2 * i), P.scaling(0.3, 0.3, 0.004)), m) for i in range(20)]
    world = P.World(many, world.light)
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), 1, threads=8)
    img, counts = _render(world, camera, 1, {}, monkeypatch)
    H.assert_images_equal(img, exp, "twenty thin discs")
    assert counts[0] == rays
