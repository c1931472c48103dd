"""Test-only glue for the first-hit buffers (tests/test_gpu_hits.py, tools/explain_pixel.py): what the ORACLE says a
ray's first hit is -- World::intersect -> Intersection::hit -> precompute_values -> set_pixel + intensity_at(over_point) --
laid out like rtc_hit_planes, and the camera's rays as the render kernels form them."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from ray_tracer_challenge_amd import _lib as L

f32 = np.float32
PLANES = tuple(L.HIT_PLANES)
GEOMETRY = tuple(k for k in PLANES if k != "light")


def empty_planes(n, planes=PLANES):
    """The record of n misses."""
    out = {}
    for k in planes:
        is_int, per = L.HIT_PLANES[k]
        out[k] = np.zeros((n, per) if per > 1 else n, dtype=np.int32 if is_int else f32)
    if "object" in out:
        out["object"][:] = -1
    return out


_arena_leaf_nodes = []  # node ids of the oracle arena's leaves, in creation order: entry k is the node of leaf k


def _object_index(own):
    """Oracle object id -> index into the flattened world (rtc_scene.objects: the leaves in depth-first order).  A flat
    oracle world numbers its objects by list position.  A world of group trees reports ARENA leaf ids: the arena is
    process-wide, a leaf's id is its rank among all leaf nodes ever made (rtco_node_shape pushes one leaf and one node)."""
    if not any(isinstance(o, O.NodeRef) for o in own.objects):
        return None
    own._handle()  # (plain shapes at the top level become nodes here)
    order = []

    def walk(node):
        if O.lib().rtco_node_is_group(node):
            for c in O.GroupShape(node).get_children():
                walk(c.node)
        else:
            order.append(node)
    for o in own.objects:
        walk(O._node_of(o))
    top = max(order) if order else -1
    k = _arena_leaf_nodes[-1] + 1 if _arena_leaf_nodes else 0
    while k <= top:
        if not O.lib().rtco_node_is_group(k):
            _arena_leaf_nodes.append(k)
        k += 1
    leaf_of_node = {node: leaf for leaf, node in enumerate(_arena_leaf_nodes)}
    return {leaf_of_node[node]: i for i, node in enumerate(order)}


def oracle_first_hits(own, origins, directions, pixels=None, light=True):
    """own: an oracle World.  -> {plane: array} for the rays, ray i drawing its light samples as pixel pixels[i] (default i)."""
    o = np.ascontiguousarray(np.asarray(origins, dtype=f32).reshape(-1, 4))
    d = np.ascontiguousarray(np.asarray(directions, dtype=f32).reshape(-1, 4))
    n = o.shape[0]
    out = empty_planes(n, PLANES if light else GEOMETRY)
    lib, h, index = O.lib(), own._handle(), _object_index(own)
    cap = 256
    ts, objs = (C.c_float * cap)(), (C.c_int * cap)()
    comps = O._Comps()
    for i in range(n):
        po, pd = O._p(o[i]), O._p(d[i])
        cnt = lib.rtco_intersect(h, po, pd, ts, objs, cap)
        if cnt > cap:
            cap = 2 * cnt
            ts, objs = (C.c_float * cap)(), (C.c_int * cap)()
            cnt = lib.rtco_intersect(h, po, pd, ts, objs, cap)
        j = lib.rtco_hit(ts, cnt)
        if j < 0:
            continue
        lib.rtco_precompute(h, po, pd, j, ts, objs, cnt, C.byref(comps))
        out["object"][i] = comps.object if index is None else index[comps.object]
        out["distance"][i] = comps.distance
        out["point"][i] = comps.point
        out["eye"][i] = comps.eye
        out["normal"][i] = comps.normal
        out["reflectv"][i] = comps.reflectv
        out["over_point"][i] = comps.over_point
        out["under_point"][i] = comps.under_point
        out["inside"][i] = comps.inside
        out["n1n2"][i] = (comps.n1, comps.n2)
        if light:
            lib.rtco_world_set_pixel(h, C.c_uint32(i if pixels is None else int(pixels[i])))
            out["light"][i] = lib.rtco_intensity_at(h, comps.over_point)
    return out


def camera_rays(camera, ys=None):
    """ray_for_pixel (camera.rs:60-74) for every pixel of rows `ys` (default: all), in image order, with the render
    kernels' arithmetic: (n, 4) origins, (n, 4) directions.  f32 throughout, one rounding per operation."""
    cam = camera._cam
    c = np.array(list(cam.inv), dtype=f32)
    ps, hw, hh = f32(cam.pixel_size), f32(cam.half_width), f32(cam.half_height)
    ys = np.arange(camera.height) if ys is None else np.asarray(ys)
    wx = (hw - (np.arange(camera.width, dtype=f32) + f32(0.5)) * ps)[None, :]
    wy = (hh - (ys.astype(f32) + f32(0.5)) * ps)[:, None]
    origin = np.array([c[3], c[7], c[11]], dtype=f32)  # transform_inverse * point(0, 0, 0)
    comp = [(c[4 * r] * wx + c[4 * r + 1] * wy + c[4 * r + 2] * f32(-1.0) + c[4 * r + 3]) - origin[r] for r in range(3)]
    m = np.sqrt(comp[0] * comp[0] + comp[1] * comp[1] + comp[2] * comp[2])
    n = len(ys) * camera.width
    directions = np.zeros((n, 4), dtype=f32)
    for r in range(3):
        directions[:, r] = (comp[r] / m).reshape(-1)
    origins = np.zeros((n, 4), dtype=f32)
    origins[:, :3] = origin
    origins[:, 3] = 1.0
    return origins, directions


def same(a, b):
    """Elementwise == as tests/helpers.py::assert_images_equal has it: +0.0 equals -0.0, NaN equals NaN; integers exactly."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "iu":
        return a == b
    return (a == b) | (np.isnan(a) & np.isnan(b))


def first_difference(got, exp, planes=None):
    """(plane, element index, got, expected) of the first plane -- in rtc_hit_planes' order -- that differs, or None."""
    for k in (planes or [k for k in PLANES if k in got and k in exp]):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, (k, g.shape, e.shape)
        bad = ~same(g, e)
        if bad.any():
            i = int(np.argwhere(bad.reshape(bad.shape[0], -1).any(axis=1))[0][0]) if bad.ndim > 1 else int(np.argwhere(bad)[0][0])
            return k, i, g[i], e[i], int(bad.reshape(bad.shape[0], -1).any(axis=1).sum())
    return None


def assert_planes_equal(got, exp, what="", planes=None):
    diff = first_difference(got, exp, planes)
    if diff is not None:
        k, i, g, e, n_bad = diff
        raise AssertionError("%s: plane %r differs in %d elements (first: element %d, got %r, expected %r)" % (what, k, n_bad, i, g, e))
