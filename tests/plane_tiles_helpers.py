"""The worlds and cameras of tests/test_plane_tiles_plan.py (CPU, the mask against the oracle) and tests/test_gpu_plane_tiles.py (the
frames drawn from the mask's list): worlds with top-level planes, whose sky tiles the scene-tile mask leaves out."""
import numpy as np

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import scenes

f32 = np.float32
UP = (0, 1, 0)


def _camera(size, frm, to, up=UP, fov=np.pi / 3):
    return P.Camera(size[0], size[1], float(fov), P.view_transform(P.point(*frm), P.point(*to), P.vector(*up)))


def _floor(**kw):
    return P.Plane(P.identity_4x4(), P.Material(color=(0.8, 0.8, 0.7), specular=0.0, **kw))


def _light():
    return P.PointLight(P.point(-6, 8, -9), P.color(1, 1, 1))


def _ball(reflective=0.3):
    return P.Sphere(P.chain(P.translation(0.3, 1.0, 0.0), P.scaling(0.8, 0.8, 0.8)), P.Material(color=(0.9, 0.3, 0.2), reflective=reflective))


def _rolled_up(deg=30.0):
    a = np.deg2rad(deg)
    return (float(np.sin(a)), float(np.cos(a)), 0.0)


def case(name, size):
    """-> (world, camera, depth) of a named case at a frame size."""
    if name in ("soft_shadows", "glass_and_mirror"):
        return getattr(scenes, name)(*size)
    if name == "plane_only":
        return P.World([_floor(reflective=0.2)], _light()), _camera(size, (0, 2, -8), (0, 1.5, 0)), 3
    if name == "floor_and_wall":  # a horizontal and a vertical plane: the wall is seen only by the rays that point to the right, the floor at the horizon
        wall = P.Plane(P.chain(P.translation(4.0, 0, 0), P.rotation_z(f32(np.pi / 2))), P.Material(color=(0.3, 0.5, 0.8), specular=0.0))
        return P.World([_floor(), wall, _ball()], _light()), _camera(size, (0, 2, -8), (-2, 4.0, 0)), 3
    if name == "rolled":  # a sphere over a plane, the camera rolled 30 degrees: a slanted horizon
        return P.World([_floor(reflective=0.2), _ball()], _light()), _camera(size, (0, 2, -9), (0, 2.5, 0), up=_rolled_up()), 3
    if name == "under_the_floor":  # the camera below the floor, looking up: the plane is seen from its other side, above the horizon
        return P.World([_floor(), _ball()], _light()), _camera(size, (0, -2, -8), (0, -1.5, 0)), 3
    if name == "straight_down":  # floor everywhere: nothing is unseen
        return P.World([_floor(), _ball()], _light()), _camera(size, (0, 9, 0), (0, 0, 0), up=(0, 0, 1)), 3
    if name == "in_the_plane":  # the camera's origin in the floor plane: the horizon decides nothing -- everything
        return P.World([_floor(), _ball()], _light()), _camera(size, (0, 0, -8), (0, 1.0, 0)), 3
    raise KeyError(name)


def two_far_balls():
    """-> (world, camera, depth): a world without planes whose two balls, far away and apart, lie on a seventh of a 320 x 256 frame's tiles
    and under two thirds of their rectangle: the sparse bounded kind, which gets its list by the policy, through the one-call seam too."""
    world = P.World([_ball(), P.Sphere(P.translation(6.0, 3.5, 0.0), P.Material(color=(0.2, 0.4, 0.9), reflective=0.3))], _light())
    return world, _camera((320, 256), (0, 1, -14), (3.0, 2, 0)), 3


def mirror_balls_at_the_horizon():
    """-> (world, camera, depth): 1280 x 960, the camera upside down over a matt floor, so that the floor fills the top of the image and
    the list ends with what is dear -- three mirror balls standing at the horizon.  More listed tiles (3 120) than an MI355X has
    workgroup slots in the feedback's model (0.85 x 256 x 6 = 1 305): in list order the balls' tiles start in the third round and
    end the frame a ball's time later, longest first they start at once.  With a ball tile 1.3 to 48 times a floor tile the
    model's gain is far above its 3 %."""
    floor = P.Plane(P.identity_4x4(), P.Material(color=(0.8, 0.8, 0.7), specular=0.0))
    balls = [P.Sphere(P.chain(P.translation(x, 0.6, 3.0), P.scaling(0.6, 0.6, 0.6)), P.Material(color=(0.9, 0.3, 0.2), reflective=0.9))
             for x in (-2.5, 0.0, 2.5)]
    return P.World([floor] + balls, _light()), _camera((1280, 960), (0, 1.5, -5), (0, 0.9, 0), up=(0, -1, 0)), 3


# (name, frame size, the least share of the frame's tiles the mask must leave out -- None: it must leave none out)
CASES = [("soft_shadows", (256, 256), 0.2), ("soft_shadows", (96, 96), 0.0), ("glass_and_mirror", (192, 128), 0.0), ("plane_only", (96, 64), 0.0),
         ("floor_and_wall", (160, 112), 0.0), ("rolled", (320, 256), 0.0), ("under_the_floor", (128, 96), 0.0), ("straight_down", (96, 64), None),
         ("in_the_plane", (112, 80), None)]
