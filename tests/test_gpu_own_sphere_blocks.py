"""Own-sphere light blocks (rtc_kernel_core.h intensity_at, ERROR_BUDGET.md B11, RTC_AMD_OWN_BLOCKS): a 2 x 2 block of an area
light's cells is called LIT against the sphere a shade point sits on when the whole block lies above that sphere's tangent plane.
It may not change an answer.  The worlds here put shade points on the rule's boundaries: the light stands BESIDE a uniformly scaled
casting sphere, at its height, 1.05 - 6 radii from its centre, so that the tangent planes of the visible points cut the light -- for
radii 1e-2 .. 1e2 (one mirrored), at the origin and a thousand units away, lights of 10 x 10, 4 x 4, 2 x 8 and (blocks must not
apply) 5 x 4 cells, hashed jitter and the constant jitters 0.0 and 1.0 that put samples on cell edges, a light almost touching the
sphere, two touching spheres, a non-casting cube between sphere and light, a squashed sphere, reflective spheres.  Every frame is
compared with the oracle bit for bit and ray for ray, with the rule on and off, with RTC_AMD_DARK=0, ahead-of-time and scene-compiled
kernels.

Skipped cases: 0 of 16.  (tests/test_gpu_shortcut_matrix.py's criterion -- f32 must resolve a twentieth of the object at the scene's
offset -- holds for every world here: the worst is `tiny_far_4x4_hashed`, radius 0.013 at offset 1e3, 1.2e-4 against 6.5e-4.)"""
import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from tests import helpers as H

pytestmark = pytest.mark.gpu
f32 = np.float32
DEPTH = 3
W, HGT = 128, 96
FOV = 0.9

# name: radius (negative: mirrored), offset of the scene from the origin, light (u cells, v cells), jitter, distance of the light's
# centre from the sphere's in radii, and what else is in the world; `band`: built to have a terminator band the rule must shorten.
# A shade point on a sphere of radius R lies 1.19e-3 / R radii off it (world.rs:210 over_point), so it "sits on" the sphere in the
# rule's sense (1e-4 < c_own, oo <= 1.21) for R between 0.0119 and 23.8: radii 0.013 and 20 are just inside, 1e-2 and 1e2 just
# outside, where the rule must say nothing (oo = 1.25: the cone speaks; c_own = 2.4e-5: the lane stays mute).  At 0.013 the lane sits
# on the sphere but B10's cone is not mute (oo = 1.19 > 1.062) and speaks for itself: no band is claimed there either; from
# R = 0.04 up the cone is mute and the rule is what speaks (0.05: `small`).
CASES = {
    "unit_10x10_hashed": dict(r=1.0, off=0.0, cells=(10, 10), jitter=("hashed", 7), dist=2.5, band=True),
    "tiny_4x4_jitter0": dict(r=1e-2, off=0.0, cells=(4, 4), jitter=("constant", 0.0), dist=1.5, band=False),
    "huge_far_2x8_jitter1": dict(r=1e2, off=1e3, cells=(2, 8), jitter=("constant", 1.0), dist=6.0, band=False),
    "small_4x4_jitter0": dict(r=0.05, off=0.0, cells=(4, 4), jitter=("constant", 0.0), dist=4.0, band=True),
    "large_far_2x8_jitter1": dict(r=20.0, off=1e3, cells=(2, 8), jitter=("constant", 1.0), dist=6.0, band=True),
    "mirrored_far_10x10_hashed": dict(r=-0.5, off=1e3, cells=(10, 10), jitter=("hashed", 11), dist=3.0, band=True),
    "tiny_far_4x4_hashed": dict(r=0.013, off=1e3, cells=(4, 4), jitter=("hashed", 3), dist=2.0, band=False),
    "huge_10x10_jitter0": dict(r=1e2, off=0.0, cells=(10, 10), jitter=("constant", 0.0), dist=1.5, band=False),
    "unit_2x8_jitter1": dict(r=1.0, off=0.0, cells=(2, 8), jitter=("constant", 1.0), dist=4.0, band=True),
    "odd_light_5x4": dict(r=1.0, off=0.0, cells=(5, 4), jitter=("hashed", 5), dist=2.5, band=False),
    "light_almost_touching": dict(r=1.0, off=0.0, cells=(4, 4), jitter=("hashed", 9), dist=1.05, size=0.4, ysize=0.4, band=False),
    "two_touching_spheres": dict(r=1.0, off=0.0, cells=(10, 10), jitter=("hashed", 13), dist=3.0, extra="touching", band=True),
    "non_casting_cube_between": dict(r=1.0, off=0.0, cells=(4, 4), jitter=("hashed", 15), dist=3.5, extra="ghost_cube", band=False),
    "squashed_sphere": dict(r=1.0, off=0.0, cells=(4, 4), jitter=("hashed", 17), dist=2.5, extra="squashed", band=False),
    "reflective_pair_far": dict(r=0.1, off=1e3, cells=(10, 10), jitter=("hashed", 19), dist=3.0, extra="reflective_pair", band=True),
    "reflective_pair_jitter0": dict(r=1.0, off=0.0, cells=(4, 4), jitter=("constant", 0.0), dist=3.0, extra="reflective_pair", band=True),
}


def geometry(r, off, cells, jitter, dist, size=1.6, ysize=0.4, extra=None):
    """The sphere at C; the light's centre at C + (dist |r|, 0, 0) -- beside the sphere, at its height -- with the rectangle spanning
    `ysize` radii in y and `size` radii in z; the floor 1.2 radii below C; the camera in front (-z), towards the light and below the
    sphere's centre, looking at its lower half.  (The floor casts: it stays in play, and the blocks out of use, for every shade point
    higher than the light's lowest point -- light_cull_mask's plane rule -- hence a light that is low and a camera that looks at what lies
    below it: there the tangent planes of the visible points cut the light with the floor culled.)"""
    a = abs(r)
    C = np.array([0.6, 0.0, 0.8]) * off
    at = lambda dx, dy, dz: C + a * np.array([dx, dy, dz], dtype=np.float64)
    spheres = [(at(0, 0, 0), r)]
    if extra == "touching":        # a neighbour of half the size touching on the side away from the light and towards the camera
        spheres.append((at(*(np.array([-0.6, 0.0, -0.8]) * 1.5)), 0.5 * a))
    if extra == "reflective_pair":  # a second mirror ball: shade points on either sphere reached by reflection in the other
        spheres.append((at(-1.3, -0.3, -1.6), 0.6 * a))
    return dict(a=a, at=at, spheres=spheres, floor_y=float(C[1] - 1.2 * a), corner=at(dist, -0.5 * ysize, -0.5 * size),
                uvec=np.array([0.0, ysize * a / cells[0], 0.0]), vvec=np.array([0.0, 0.0, size * a / cells[1]]), cells=cells,
                cam_from=at(1.0, -0.5, -3.2), cam_to=at(-0.2, -0.3, 0.0))


def build_world(r, off, cells, jitter, dist, band, size=1.6, ysize=0.4, extra=None):
    g = geometry(r, off, cells, jitter, dist, size, ysize, extra)
    a, at = g["a"], g["at"]
    mat = P.Material(color=(0.8, 0.5, 0.4), specular=0.0, reflective=0.5 if extra == "reflective_pair" else 0.0)
    objs = [P.Plane(P.translation(0.0, g["floor_y"], 0.0), P.Material(color=(0.9, 0.9, 0.8), specular=0.0))]
    for k, (c, rad) in enumerate(g["spheres"]):
        s = (rad, 0.7 * rad, 1.3 * rad) if extra == "squashed" and k == 0 else (rad, rad, rad)
        objs.append(P.Sphere(P.chain(P.translation(*[float(x) for x in c]), P.scaling(*[float(x) for x in s])), mat))
    if extra == "ghost_cube":       # half-way to the light, casting nothing: may be hit first, BLOCKED must stay silent
        objs.append(P.Cube(P.chain(P.translation(*[float(x) for x in at(0.5 * dist + 0.5, 0.0, 0.0)]), P.scaling(0.05 * a, 0.8 * a, 0.8 * a)), P.Material(), casts_shadow=False))
    light = P.RectangleLight(P.color(1.2, 1.1, 1.0), P.point(*[float(x) for x in g["corner"]]), P.vector(*[float(x) * cells[0] for x in g["uvec"]]), cells[0],
                             P.vector(*[float(x) * cells[1] for x in g["vvec"]]), cells[1], jitter)
    cam = P.Camera(W, HGT, FOV, P.view_transform(P.point(*[float(x) for x in g["cam_from"]]), P.point(*[float(x) for x in g["cam_to"]]), P.vector(0, 1, 0)))
    return P.World(objs, light), cam


_oracle = {}


def oracle_frame(name):
    """The reference's frame and ray count, rendered once per world and shared."""
    if name not in _oracle:
        world, cam = build_world(**CASES[name])
        _oracle[name] = H.oracle_camera(cam).render(H.oracle_world(world), DEPTH, threads=8)
    return _oracle[name]


@pytest.mark.parametrize("name", list(CASES))
def test_own_sphere_blocks_change_nothing(name, monkeypatch):
    from ray_tracer_challenge_amd.renderer import Renderer
    case = CASES[name]
    world, cam = build_world(**case)
    exp, rays = oracle_frame(name)
    monkeypatch.setenv("RTC_AMD_SHARE_LOG2", "0")  # one lane per pixel: the kernels that have the block loop, at this size
    culled = {}
    for spec in ("0", "1"):
        for own in ("1", "0"):
            for dark in ("1", "0"):
                monkeypatch.setenv("RTC_AMD_SPECIALIZE", spec)
                monkeypatch.setenv("RTC_AMD_OWN_BLOCKS", own)
                monkeypatch.setenv("RTC_AMD_DARK", dark)
                r = Renderer(world, cam, device=0)
                got = r.render(DEPTH).cpu().numpy()
                st = r.stats()
                r.close()
                H.assert_images_equal(got, exp, "%s specialise=%s own=%s dark=%s" % (name, spec, own, dark))
                assert st["rays"] == rays, (name, spec, own, dark)
                culled[(spec, own, dark)] = st["culled_shadow_rays"]
    print(name, "rays", rays, "culled", culled)
    for spec in ("0", "1"):
        for dark in ("1", "0"):
            assert culled[(spec, "1", dark)] >= culled[(spec, "0", dark)], culled
            if case["band"]:
                assert culled[(spec, "1", dark)] > culled[(spec, "0", dark)], culled
        if case["cells"][0] % 2:  # an odd count: no blocks, hence no rule
            assert culled[(spec, "1", "1")] == culled[(spec, "0", "1")], culled
