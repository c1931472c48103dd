"""What tests/test_gpu_lens.py and the child processes it starts share: the cases -- world, camera, depth, factor, lens, switches --
and the oracle side of a lens frame.  By definition (include/rtc.h, rtc_ctx_set_scene_lens) the frame is the box filter of the fine
frame whose pixel is World::color_at of the ray rtc_lens_rays gives it, with the fine pixel index as its jitter key and a black
last row and column."""
import os

import numpy as np

from ray_tracer_challenge_amd import Camera, Lens, api, point, scenes, vector, view_transform
from ray_tracer_challenge_amd.obj_parser import parse_obj
from tests.supersample_helpers import box_filter

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
PI = f32(np.pi)


def golden_mesh(camera):
    """tests/golden/triangles.obj, three copies of it, as one divided GroupShape over a mirror floor: the traversal kernel, with
    triangle pre-culling boxes"""
    text = open(os.path.join(HERE, "golden", "triangles.obj")).read()
    mesh = api.GroupShape()
    for k in range(3):
        part = parse_obj(text, api).take_all_as_group()
        part.set_material(api.Material(color=(0.9 - 0.3 * k, 0.3, 0.2 + 0.3 * k), reflective=0.2 * k))
        part.set_transformation(api.chain(api.translation(-1.5 + 1.5 * k, 1.0, 0.5 * k), api.rotation_y(f32(0.3 * k))))
        mesh.add_child(part)
    mesh.divide(4)
    floor = api.Plane(api.identity_4x4(), api.Material(color=(0.8, 0.8, 0.75), specular=0.0, reflective=0.3))
    world = api.World([floor, mesh], api.PointLight(point(-6, 8, -8), api.color(1, 1, 1)))
    return world, camera, 5


# The glass sphere of reflect_refract nearest its camera: centre (-0.5, 1, 0.5), radius 1 (scenes.reflect_refract: `middle`)
GLASS_CENTRE, GLASS_RADIUS = np.array([-0.5, 1.0, 0.5]), 1.0


def _reflect_refract_beside_the_glass():
    """A lens lies in the plane through the camera perpendicular to its line of sight, and the demo's own camera looks AT the glass
    sphere from 5.5 units away: no aperture puts a lens point inside it.  This camera stands beside the sphere and looks past it; the
    sphere's centre is 0.91 in front of the lens's plane and 1.29 beside the camera, so the plane cuts the sphere in a disc of radius
    sqrt(1 - 0.91^2) = 0.41 whose nearest point is 0.88 from the camera: R = 1.5 reaches well into it."""
    world, _, depth = scenes.reflect_refract(24, 16)
    camera = Camera(24, 16, PI / f32(3.0), view_transform(point(1.0, 1.0, 0.0), point(-0.2, 1.0, 4.0), vector(0, 1, 0)))
    return world, camera, depth


def _with_depth(triple, depth):
    return triple[0], triple[1], depth


# name -> (world, camera, depth), k, lens, switches of the library beyond RTC_AMD_SPECIALIZE.  Output sizes: the smallest that reach
# each path -- 26 x 18 is no multiple of 8 either way, 20 x 16 under an area light shares lanes in the scene's own kernel.
CASES = {
    "sphere_grid_k2": (lambda: _with_depth(scenes.sphere_grid(26, 18), 5), 2, Lens(0.6, 20.0, seed=1), {}),
    "sphere_grid_k4": (lambda: _with_depth(scenes.sphere_grid(26, 18), 5), 4, Lens(0.6, 20.0, seed=1), {}),
    "soft_shadows_k2": (lambda: scenes.soft_shadows(20, 16), 2, Lens(0.15, 3.9, seed=2), {}),
    "soft_shadows_k4": (lambda: scenes.soft_shadows(20, 16), 4, Lens(0.15, 3.9, seed=2), {}),
    "soft_shadows_k2_one_lane": (lambda: scenes.soft_shadows(20, 16), 2, Lens(0.15, 3.9, seed=2), {"RTC_AMD_SHARE_LOG2": "0"}),
    "soft_shadows_k4_one_lane": (lambda: scenes.soft_shadows(20, 16), 4, Lens(0.15, 3.9, seed=2), {"RTC_AMD_SHARE_LOG2": "0"}),
    "reflect_refract": (lambda: _with_depth(scenes.reflect_refract(24, 16), 5), 2, Lens(0.3, 5.5, seed=3), {}),
    "reflect_refract_inside_the_glass": (_reflect_refract_beside_the_glass, 2, Lens(1.5, 3.0, seed=3), {}),
    "golden_mesh": (lambda: golden_mesh(Camera(24, 16, PI / f32(3.0), view_transform(point(0.2, 2.0, -5.0), point(0, 0.8, 0), vector(0, 1, 0)))),
                    2, Lens(0.2, 5.2, seed=4), {}),
    # the camera far away in a corner of the scene's box, an aperture of 10: lens points leave the ball the pre-culling boxes are padded for
    "golden_mesh_outside_the_cull_ball": (lambda: golden_mesh(Camera(24, 16, f32(0.12), view_transform(point(9, 9, -40), point(0, 0.8, 0), vector(0, 1, 0)))),
                                          2, Lens(10.0, 41.0, seed=5), {}),
}
# the cases whose oracle frame and whose switches are another case's
SAME_FRAME = {"soft_shadows_k2_one_lane": "soft_shadows_k2", "soft_shadows_k4_one_lane": "soft_shadows_k4"}


def zero_last_row_and_column(fine):
    fine = fine.copy()
    fine[-1] = 0.0
    fine[:, -1] = 0.0
    return fine


def oracle_lens_frame(own, camera, depth, k, lens):
    """own: the oracle's world (tests.helpers.oracle_world) -> (the lens frame, rays traced, the fine frame)."""
    o, d = camera.lens_rays(k, lens)
    fw, fh = k * camera.width, k * camera.height
    fine = np.zeros((fh, fw, 3), dtype=f32)
    before = own.ray_count
    for y in range(fh - 1):  # camera.rs:80-81 at the fine resolution: the last row and column are not traced
        for x in range(fw - 1):
            key = y * fw + x
            own.set_pixel(key)
            fine[y, x] = own.color_at(o[key], d[key], depth)
    return box_filter(fine, k), own.ray_count - before, fine
