"""Test-only glue for the ray-stream first hits and occlusion queries (tests/test_gpu_trace_hits.py,
tests/test_trace_hits_boundary.py): the worlds of every ahead-of-time kernel family under small cameras, and the second
bounce the tests trace -- built with torch from a dict of first-hit planes, so that the same function makes it on the device
from Renderer.trace_hits' result and on the host from the oracle's."""
import os

import numpy as np
import torch

from ray_tracer_challenge_amd import api, rays, scenes
from ray_tracer_challenge_amd.obj_parser import parse_obj
from ray_tracer_challenge_amd.scenes import PI, Camera, f32, point, vector, view_transform

HERE = os.path.dirname(os.path.abspath(__file__))


def camera(w, h):
    """Low over sphere_grid: the rows of spheres overlap, the sky above sees nothing (tests/test_gpu_primary_ray.py's)."""
    return Camera(w, h, PI / f32(5.0), view_transform(point(1, 0.8, -2.5), point(0, 0.4, 7), vector(0, 1, 0)))


def spheres(n):
    """sphere_grid's first n x n spheres (a flat world) under a camera of their own"""
    world, _, depth = scenes.sphere_grid(40, 30, n=n)
    c = f32(-7.0 + (n - 1))  # the grid's centre: x = -7 + 2 i, z = 2 j
    cam = Camera(40, 30, PI / f32(3.0), view_transform(point(c, 4.5, -6.0), point(c, 0.0, n - 1.0), vector(0, 1, 0)))
    return world, cam, depth


def golden_mesh():
    """tests/golden/triangles.obj, three copies of it, as one divided GroupShape over a mirror floor"""
    text = open(os.path.join(HERE, "golden", "triangles.obj")).read()
    mesh = api.GroupShape()
    for k in range(3):
        part = parse_obj(text, api).take_all_as_group()
        part.set_material(api.Material(color=(0.9 - 0.3 * k, 0.3, 0.2 + 0.3 * k), reflective=0.2 * k))
        part.set_transformation(api.chain(api.translation(-1.5 + 1.5 * k, 1.0, 0.5 * k), api.rotation_y(f32(0.3 * k))))
        mesh.add_child(part)
    mesh.divide(1)
    floor = api.Plane(api.identity_4x4(), api.Material(color=(0.8, 0.8, 0.75), specular=0.0, reflective=0.3))
    world = api.World([floor, mesh], api.PointLight(point(-6, 8, -8), api.color(1, 1, 1)))
    cam = Camera(40, 30, PI / f32(3.0), view_transform(point(0.2, 2.0, -5.0), point(0, 0.8, 0), vector(0, 1, 0)))
    return world, cam, 5


# One world per ahead-of-time kernel family and object-loop shape, all at 40 x 30.  (Depth plays no part in a first hit.)
FAMILIES = {
    "simple_le4": lambda: scenes.glass_and_mirror(40, 30),
    "general_le8": lambda: scenes.first_scene(40, 30),
    "flat_gt8": lambda: spheres(3),
    "flat_bvh_16": lambda: spheres(4),
    "hexagons": lambda: scenes.hexagons(40, 30),
    "golden_mesh": golden_mesh,
    "textured": lambda: scenes.first_textures(40, 30),
    "soft_shadows": lambda: scenes.soft_shadows(40, 30),
    "reflect_refract": lambda: scenes.reflect_refract(40, 30),
}
# The scenes whose second bounce is traced: glass, mirrors, a group tree, nested refractive indices, textures.
BOUNCE_SCENES = {
    "glass_and_mirror": lambda: scenes.glass_and_mirror(40, 30),
    "first_scene": lambda: scenes.first_scene(40, 30),
    "hexagons": lambda: scenes.hexagons(40, 30),
    "reflect_refract": lambda: scenes.reflect_refract(40, 30),
    "first_textures": lambda: scenes.first_textures(40, 30),
}


def scrambled_keys(n):
    """2654435761 * i mod 2^32: no key is its ray's index past 0, half of them are >= 2^31."""
    return ((2654435761 * np.arange(n, dtype=np.uint64)) % (1 << 32)).astype(np.uint32)


def as_tensors(planes, device=None):
    """{plane: numpy array} -> {plane: tensor}"""
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) if device else torch.from_numpy(np.ascontiguousarray(v)) for k, v in planes.items()}


def second_stream(hits, directions):
    """The rays that leave the first hits, on the planes' device: the reflections (rays.reflected: over_point, reflectv),
    followed by the straight-through rays (under_point, the ray's own direction) of the same hits, both in index order.
    -> (origins (2 m, 4), directions (2 m, 4))."""
    o_r, d_r, index = rays.reflected(hits, directions)
    o_t = hits["under_point"].reshape(-1, 4)[index]
    d_t = directions.reshape(-1, 4)[index]
    return torch.cat([o_r, o_t]).contiguous(), torch.cat([d_r, d_t]).contiguous()


def visibility_pairs(origins):
    """Pair i of the mutual-visibility test: (origin (7919 i + 13) mod n, origin i) -- surface points, no light involved."""
    n = origins.shape[0]
    j = (7919 * torch.arange(n, dtype=torch.int64, device=origins.device) + 13) % max(n, 1)
    return origins[j].contiguous(), origins
