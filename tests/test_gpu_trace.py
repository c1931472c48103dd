"""Ray streams (-m gpu): Renderer.trace colours the caller's rays against the resident scene exactly as the oracle's
World::color_at colours them -- and, for the camera's own rays, exactly as the render kernels do -- whichever 64 rays share a
wave, in every kernel family, and without leaving a trace in the context's render state (rtc_ctx_trace, csrc/rtc_trace.h).

Base case: the world and camera of tests/test_gpu_primary_ray.py -- sphere_grid at 52 x 36, 1872 rays: no multiple of a wave
(64) or a workgroup (256), a tree world, a good quarter of the rays hit and a good quarter miss.  Every comparison is
bit-exact (tests.helpers.assert_images_equal)."""
import os

import numpy as np
import pytest
import torch

from ray_tracer_challenge_amd import api, rays, scenes
from ray_tracer_challenge_amd.obj_parser import parse_obj
from ray_tracer_challenge_amd.renderer import Renderer
from ray_tracer_challenge_amd.scenes import PI, Camera, f32, point, vector, view_transform
from tests import helpers as H
from tests import hits_helpers as HH

pytestmark = pytest.mark.gpu
W, HEIGHT = 52, 36
N = W * HEIGHT
HERE = os.path.dirname(os.path.abspath(__file__))


def _camera(w, h):
    # tests/test_gpu_primary_ray.py's: low over the grid, the rows of spheres overlap, the sky above sees nothing
    return Camera(w, h, PI / f32(5.0), view_transform(point(1, 0.8, -2.5), point(0, 0.4, 7), vector(0, 1, 0)))


def _oracle_colors(own, origins, directions, keys, depth):
    """World::color_at ray by ray, ray i drawing as pixel keys[i] -> ((n, 3) colours, rays traced)."""
    out = np.zeros((len(origins), 3), dtype=np.float32)
    before = own.ray_count
    for i in range(len(origins)):
        own.set_pixel(int(keys[i]))
        out[i] = own.color_at(origins[i], directions[i], depth)
    return out, own.ray_count - before


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") if dtype is None else torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to("cuda:0")


def _keys_tensor(keys):
    """uint32 keys as the int32 tensor that carries their bits."""
    return _dev(np.asarray(keys, dtype=np.uint32), np.int32)


def _equal(got, exp, what):
    """bit-exact comparison of (n, 3) colour lists"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    H.assert_images_equal(got.reshape(1, -1, 3), exp.reshape(1, -1, 3), what)


def _trace(r, o, d, depth, keys=None, **kw):
    out = r.trace(o, d, depth, keys=keys, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def case():
    """World, camera, depth; the camera's rays and keys on the host; the oracle's colour of every one of the 1872 rays -- the last
    row and column included, which no render traces -- and its ray count over them.  Computed once, left unchanged."""
    world, _, depth = scenes.sphere_grid(W, HEIGHT)
    camera = _camera(W, HEIGHT)
    own = H.oracle_world(world)
    origins, directions = HH.camera_rays(camera)
    keys = np.arange(N, dtype=np.uint32)
    hits = HH.oracle_first_hits(own, origins, directions, light=False)
    obj = hits["object"].reshape(HEIGHT, W).copy()
    obj[-1, :] = -1  # camera.rs:80-81: the last row and column are never traced
    obj[:, -1] = -1
    n_miss, n_hit = int((obj < 0).sum()), int((obj >= 0).sum())
    assert 4 * n_miss >= N and 4 * n_hit >= N, (n_miss, n_hit)  # (a camera change must not hollow the tests out)
    colors, n_rays = _oracle_colors(own, origins, directions, keys, depth)
    return {"world": world, "camera": camera, "depth": depth, "own": own, "o": origins, "d": directions, "keys": keys, "hits": hits,
            "colors": colors, "rays": n_rays}


@pytest.fixture(scope="module")
def traced(case):
    """The base case on the device: the render, the camera's rays as the library makes them, and their trace."""
    r = Renderer(case["world"], case["camera"], device=0)
    frame = r.render(case["depth"])
    torch.cuda.synchronize()
    o, d, k = r.camera_rays()
    colors = r.trace(o, d, case["depth"], keys=k)
    stats = r.stats()
    out = {"frame": frame.cpu().numpy(), "o": o, "d": d, "k": k, "colors": colors.cpu().numpy(), "stats": stats, "name": r.trace_kernel_name,
           "id": r.trace_kernel_id, "render_name": r.kernel_name}
    yield out
    r.close()


# ---- 1. the camera's rays ----------------------------------------------------------
def test_camera_rays_are_the_render_kernels_rays(case, traced):
    o, d, k = (t.cpu().numpy() for t in (traced["o"], traced["d"], traced["k"]))
    assert o.shape == (N, 4) and d.shape == (N, 4) and k.shape == (N,)
    HH.assert_planes_equal({"origin": o, "direction": d}, {"origin": case["o"], "direction": case["d"]}, "camera_rays()", planes=("origin", "direction"))
    assert (o[:, 3] == 1.0).all() and (d[:, 3] == 0.0).all()
    ys, xs = np.divmod(np.arange(N), W)
    assert (k.view(np.uint32) == (ys * W + xs).astype(np.uint32)).all()
    r = Renderer(case["world"], case["camera"], device=0)
    o2, d2, k2 = (t.cpu().numpy() for t in r.camera_rays(y0=7, n_rows=9))
    eo, ed = HH.camera_rays(case["camera"], ys=np.arange(7, 16))
    r.close()
    assert o2.shape == (9 * W, 4)
    HH.assert_planes_equal({"origin": o2, "direction": d2}, {"origin": eo, "direction": ed}, "camera_rays(y0=7, n_rows=9)", planes=("origin", "direction"))
    assert (k2.view(np.uint32) == np.arange(7 * W, 16 * W, dtype=np.uint32)).all()
    # another camera than the context's: an argument, not the resident one
    other = _camera(20, 10)
    r = Renderer(case["world"], case["camera"], device=0)
    o3, d3, k3 = (t.cpu().numpy() for t in r.camera_rays(other))
    r.close()
    eo, ed = HH.camera_rays(other)
    HH.assert_planes_equal({"origin": o3, "direction": d3}, {"origin": eo, "direction": ed}, "camera_rays(other)", planes=("origin", "direction"))
    assert (k3 == np.arange(200)).all()


# ---- 2. trace equals render ----------------------------------------------------------
def test_trace_of_the_cameras_rays_is_the_render_and_the_oracle(case, traced):
    assert traced["name"].startswith("trace_kernel"), traced["name"]
    assert traced["id"].startswith(("aot_trace_", "spec_")), traced["id"]
    got = traced["colors"].reshape(HEIGHT, W, 3)
    H.assert_images_equal(got[:-1, :-1], traced["frame"][:-1, :-1], "trace against render, the traced pixels")
    assert not traced["frame"][-1].any() and not traced["frame"][:, -1].any()  # (what a render leaves black ...)
    exp = case["colors"].reshape(HEIGHT, W, 3)
    edge = np.concatenate([got[-1], got[:-1, -1]]), np.concatenate([exp[-1], exp[:-1, -1]])
    assert edge[0].shape == (W + HEIGHT - 1, 3)  # 87 rays
    _equal(edge[0], edge[1], "trace against the oracle, last row and column")  # (... a trace colours)
    H.assert_images_equal(got, exp, "trace against the oracle, every ray")
    st = traced["stats"]
    assert st["rays"] == case["rays"], (st["rays"], case["rays"])
    assert st["pixels"] == N and st["rows"] == 0 and st["launches"] == 1, st
    assert st["shaded_hits"] > 0 and st["kernel_ms"] > 0.0, st


# ---- 3. rays that no camera makes ----------------------------------------------------
def test_reflection_rays_from_the_first_hits_match_the_oracle(case):
    hit = case["hits"]["object"] >= 0
    origins = np.ascontiguousarray(case["hits"]["over_point"][hit])
    directions = np.ascontiguousarray(case["hits"]["reflectv"][hit])
    n = origins.shape[0]
    assert n >= 468, n
    keys = ((2654435761 * np.arange(n, dtype=np.uint64)) % (1 << 32)).astype(np.uint32)
    exp, exp_rays = _oracle_colors(case["own"], origins, directions, keys, case["depth"])
    r = Renderer(case["world"], case["camera"], device=0)
    got = _trace(r, _dev(origins), _dev(directions), case["depth"], keys=_keys_tensor(keys))
    st = r.stats()
    r.close()
    _equal(got, exp, "reflection rays against the oracle")
    assert st["rays"] == exp_rays and st["pixels"] == n, (st, exp_rays)
    assert len(np.unique(got, axis=0)) > 16  # (they do see the scene)


# ---- 3a. the keys reach the arithmetic -------------------------------------------------
# Only a hashed-jitter area light reads a ray's key (the light's sample points are drawn from seed, key and path), so the keys
# are tested where they matter: soft_shadows under its rectangle light, 40 x 30, with keys that are not the rays' indices.
@pytest.fixture(scope="module")
def jittered():
    """soft_shadows 40 x 30 (hashed jitter): world, camera, depth, its oracle world, the camera's rays on the host, and keys that differ
    from every index -- a multiplicative scramble, a third of them >= 2^31, the largest ones pinned."""
    world, camera, depth = scenes.soft_shadows(40, 30)
    origins, directions = HH.camera_rays(camera)
    n = origins.shape[0]
    keys = ((2654435761 * (np.arange(n, dtype=np.uint64) + 1)) % (1 << 32)).astype(np.uint32)
    keys[5], keys[700] = 0xffffffff, 0x80000000
    assert (keys != np.arange(n)).all() and int((keys >= 1 << 31).sum()) >= n // 3
    own = H.oracle_world(world)
    return {"world": world, "camera": camera, "depth": depth, "own": own, "o": origins, "d": directions, "keys": keys}


def test_keys_choose_the_light_samples_as_set_pixel_does(jittered):
    j = jittered
    n = len(j["keys"])
    exp, exp_rays = _oracle_colors(j["own"], j["o"], j["d"], j["keys"], j["depth"])
    by_index, _ = _oracle_colors(j["own"], j["o"], j["d"], np.arange(n), j["depth"])
    differ = int((exp != by_index).any(axis=1).sum())
    # the keys do reach the colours here -- in the penumbra, where some of a point's samples are blocked, and in what reflects it: one
    # such ray is enough to tell a trace that ignored its keys, since every comparison below is bit-exact over all rays
    print("rays whose colour depends on the key: %d of %d" % (differ, n))
    assert differ > 0
    r = Renderer(j["world"], j["camera"], device=0)
    o, d = _dev(j["o"]), _dev(j["d"])
    k = _keys_tensor(j["keys"])
    assert k.dtype == torch.int32 and int((k < 0).sum()) >= n // 3  # keys of 2^31 and more, carried in an int32 tensor
    got = _trace(r, o, d, j["depth"], keys=k)
    st = r.stats()
    none = _trace(r, o, d, j["depth"])
    r.close()
    _equal(got, exp, "scrambled keys under a hashed-jitter light against the oracle's set_pixel(key)")
    assert st["rays"] == exp_rays, (st["rays"], exp_rays)
    _equal(none, by_index, "keys=None under a hashed-jitter light against the oracle's set_pixel(i)")


def test_a_permutation_with_its_keys_permutes_the_colours_under_an_area_light(jittered):
    """The wave-voted light culls and block cones on waves of 64 unrelated rays, each ray carrying its own key."""
    j = jittered
    n = len(j["keys"])
    perm = np.random.RandomState(4321).permutation(n)
    r = Renderer(j["world"], j["camera"], device=0)
    o, d, k = _dev(j["o"]), _dev(j["d"]), _keys_tensor(j["keys"])
    straight = _trace(r, o, d, j["depth"], keys=k)
    tp = torch.from_numpy(perm).to("cuda:0")
    shuffled = _trace(r, o[tp].contiguous(), d[tp].contiguous(), j["depth"], keys=k[tp].contiguous())
    # ... and with the camera's own keys: the render's bits, in the permuted order
    cam_keys = torch.arange(n, dtype=torch.int32, device="cuda:0")
    frame = r.render(j["depth"])
    torch.cuda.synchronize()
    shuffled_cam = _trace(r, o[tp].contiguous(), d[tp].contiguous(), j["depth"], keys=cam_keys[tp].contiguous())
    r.close()
    _equal(shuffled, straight[perm], "permuted rays with their scrambled keys")
    h, w = j["camera"].height, j["camera"].width
    inner = (perm // w < h - 1) & (perm % w < w - 1)  # the pixels a render traces
    _equal(shuffled_cam[inner], frame.cpu().numpy().reshape(-1, 3)[perm][inner], "permuted rays with the camera's keys against the render")


# ---- 3b. a context without a scene, a real context's depth range ------------------------
def test_a_real_context_refuses_no_scene_and_depths_out_of_range(case, traced):
    import ctypes as C

    from ray_tracer_challenge_amd import _lib as L
    lib = L.lib()
    ctx = C.c_void_p()
    L.check(lib.rtc_ctx_create(0, C.byref(ctx)))
    o, d, out = traced["o"], traced["d"], torch.full((N, 3), -7.0, dtype=torch.float32, device="cuda:0")
    args = (C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), None, N, C.c_void_p(out.data_ptr()), None)
    try:
        assert lib.rtc_ctx_trace(ctx, 5, *args) == L.RTC_ERR_INVALID_ARG
        assert b"no scene" in lib.rtc_last_error()
        assert lib.rtc_ctx_trace_kernel_name(ctx) == b"" and lib.rtc_ctx_trace_kernel_id(ctx) == b""
    finally:
        lib.rtc_ctx_destroy(ctx)
    r = Renderer(case["world"], case["camera"], device=0)
    for depth in (-1, L.RTC_MAX_DEPTH + 1):
        assert lib.rtc_ctx_trace(r._ctx, depth, *args) == L.RTC_ERR_INVALID_ARG
        assert b"depth" in lib.rtc_last_error()
        with pytest.raises(L.RtcError):
            r.trace(o, d, depth)
    assert r.trace_kernel_name == ""  # nothing was launched
    r.close()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # ... and nothing written


# ---- 4. a wave is any 64 rays --------------------------------------------------------
def test_a_permutation_of_the_rays_permutes_the_colours(case, traced):
    perm = torch.from_numpy(np.random.RandomState(1234).permutation(N)).to("cuda:0")
    r = Renderer(case["world"], case["camera"], device=0)
    got = _trace(r, traced["o"][perm].contiguous(), traced["d"][perm].contiguous(), case["depth"], keys=traced["k"][perm].contiguous())
    st = r.stats()
    r.close()
    _equal(got, traced["colors"][perm.cpu().numpy()], "permuted rays")
    assert st["rays"] == case["rays"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_the_first_n_rays_give_the_first_n_colours(case, traced, n):
    r = Renderer(case["world"], case["camera"], device=0)
    o, d = traced["o"][:n].contiguous(), traced["d"][:n].contiguous()
    guard = torch.full((n + 64, 3), -7.0, dtype=torch.float32, device="cuda:0")
    out = r.trace(o, d, case["depth"], keys=traced["k"][:n].contiguous(), out=guard[:n])
    torch.cuda.synchronize()
    assert out.data_ptr() == guard.data_ptr()
    assert bool((guard[n:] == -7.0).all())  # nothing is written past ray n - 1
    _equal(guard[:n].cpu().numpy(), traced["colors"][:n], "the first %d rays" % n)
    assert r.stats()["pixels"] == n
    # keys = None: ray i draws as pixel i
    none = _trace(r, o, d, case["depth"])
    explicit = _trace(r, o, d, case["depth"], keys=torch.arange(n, dtype=torch.int32, device="cuda:0"))
    r.close()
    _equal(none, explicit, "keys=None against arange(%d)" % n)
    _equal(none, traced["colors"][:n], "keys=None: the camera's keys are 0 .. n - 1 here")


# ---- 5. every kernel family ----------------------------------------------------------
def _spheres(n):
    """sphere_grid's first n x n spheres (a flat world) under a camera of their own"""
    world, _, depth = scenes.sphere_grid(40, 30, n=n)
    c = f32(-7.0 + (n - 1))  # the grid's centre: x = -7 + 2 i, z = 2 j
    camera = Camera(40, 30, PI / f32(3.0), view_transform(point(c, 4.5, -6.0), point(c, 0.0, n - 1.0), vector(0, 1, 0)))
    return world, camera, depth


def _golden_mesh():
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
    camera = Camera(40, 30, PI / f32(3.0), view_transform(point(0.2, 2.0, -5.0), point(0, 0.8, 0), vector(0, 1, 0)))
    return world, camera, 5


FAMILIES = {
    "simple_le4": lambda: scenes.glass_and_mirror(40, 30),
    "general_le8": lambda: scenes.first_scene(40, 30),
    "flat_gt8": lambda: _spheres(3),
    "flat_bvh_16": lambda: _spheres(4),
    "hexagons": lambda: scenes.hexagons(40, 30),
    "golden_mesh": _golden_mesh,
    "textured": lambda: scenes.first_textures(40, 30),
    "soft_shadows": lambda: scenes.soft_shadows(40, 30),
    "reflect_refract": lambda: scenes.reflect_refract(40, 30),
    "reflect_refract_deep": lambda: scenes.reflect_refract(40, 30)[:2] + (12,),
}


def _trace_and_render(world, camera, depth):
    """-> (trace of the camera's rays as a frame, the render, trace kernel name, trace kernel id, render kernel id before and after the trace)"""
    r = Renderer(world, camera, device=0)
    frame = r.render(depth)
    torch.cuda.synchronize()
    rid = r.kernel_id
    o, d, k = r.camera_rays()
    got = _trace(r, o, d, depth, keys=k).reshape(camera.height, camera.width, 3)
    out = got, frame.cpu().numpy(), r.trace_kernel_name, r.trace_kernel_id, rid, r.kernel_id
    r.close()
    return out


@pytest.mark.parametrize("name", list(FAMILIES))
def test_every_family_traces_what_it_renders(name, monkeypatch):
    monkeypatch.delenv("RTC_AMD_SPECIALIZE", raising=False)
    world, camera, depth = FAMILIES[name]()
    got, frame, tname, tid, rid0, rid1 = _trace_and_render(world, camera, depth)
    print(name, tname, tid)
    assert tname.startswith("trace_kernel"), tname
    assert tid and rid0 == rid1
    assert frame[:-1, :-1].any()  # (the camera sees the scene)
    H.assert_images_equal(got[:-1, :-1], frame[:-1, :-1], "%s: trace against render" % name)
    if name == "reflect_refract_deep":
        assert tname.startswith("trace_kernel_spec"), tname  # depth 12: the deep-stack variant is a scene kernel


@pytest.mark.parametrize("name", ["soft_shadows", "reflect_refract"])
def test_the_scenes_own_kernel_and_the_ahead_of_time_one_trace_the_same_bits(name, monkeypatch):
    world, camera, depth = FAMILIES[name]()
    res = {}
    for policy in ("0", "1"):
        monkeypatch.setenv("RTC_AMD_SPECIALIZE", policy)
        res[policy] = _trace_and_render(world, camera, depth)
        got, frame, tname, tid, rid0, rid1 = res[policy]
        assert rid0 == rid1, (rid0, rid1)  # the render's kernel id is unchanged by the trace
        H.assert_images_equal(got[:-1, :-1], frame[:-1, :-1], "%s, RTC_AMD_SPECIALIZE=%s: trace against render" % (name, policy))
    assert res["0"][2].startswith("trace_kernel<") and res["0"][3].startswith("aot_trace_"), res["0"][2:4]
    assert res["1"][2].startswith("trace_kernel_spec[") and res["1"][3].startswith("spec_"), res["1"][2:4]
    assert res["0"][3] != res["1"][3]
    assert res["1"][3] != res["1"][4]  # ... and the scene's trace kernel is not its render kernel
    H.assert_images_equal(res["0"][0], res["1"][0], "%s: ahead-of-time against scene kernel" % name)


# ---- 6. a trace leaves the context alone -----------------------------------------------
def test_a_trace_between_two_renders_leaves_no_trace(case, traced):
    def run(with_trace):
        r = Renderer(case["world"], case["camera"], device=0)
        a = r.render(case["depth"]).clone()
        ident = r.kernel_name, r.kernel_id
        if with_trace:
            r.trace(traced["o"], traced["d"], case["depth"], keys=traced["k"])
            assert r.trace_kernel_name.startswith("trace_kernel")
            assert (r.kernel_name, r.kernel_id) == ident
        b = r.render(case["depth"])
        st = r.stats()
        assert (r.kernel_name, r.kernel_id) == ident
        out = a.cpu().numpy(), b.cpu().numpy(), st, ident
        r.close()
        return out
    a1, b1, st1, id1 = run(True)
    a0, b0, st0, id0 = run(False)
    H.assert_images_equal(a1, b1, "render, trace, render: the two frames")
    H.assert_images_equal(b1, b0, "the frame after a trace against a fresh context's")
    assert id1 == id0
    st1.pop("kernel_ms"), st0.pop("kernel_ms")
    assert st1 == st0, (st1, st0)
    assert st1["launches"] == 2 and st1["rows"] == HEIGHT


# ---- 7. supersampled context ----------------------------------------------------------
def test_a_supersampled_context_traces_like_a_plain_one(case, traced):
    r = Renderer(case["world"], _camera(W // 2, HEIGHT // 2), device=0, supersample=2)
    assert r.kernel_name.startswith("ss_render_kernel")
    got = _trace(r, traced["o"], traced["d"], case["depth"], keys=traced["k"])
    name = r.trace_kernel_name
    r.close()
    assert name.startswith("trace_kernel"), name
    _equal(got, traced["colors"], "supersample=2 context")


# ---- 8. streams ---------------------------------------------------------------------
def test_a_trace_on_another_stream(case, traced):
    r = Renderer(case["world"], case["camera"], device=0)
    s = torch.cuda.Stream(device="cuda:0")
    s.wait_stream(torch.cuda.current_stream("cuda:0"))
    out = r.trace(traced["o"], traced["d"], case["depth"], keys=traced["k"], stream=s)
    s.synchronize()
    got = out.cpu().numpy()
    r.close()
    _equal(got, traced["colors"], "a trace on a stream of its own")


# ---- 9. the generators ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["equirectangular", "orthographic"])
def test_generated_rays_are_coloured_as_the_oracle_colours_them(case, which):
    if which == "equirectangular":
        o, d = rays.equirectangular(48, 24, point(1, 0.8, -2.5), device="cuda:0")
    else:
        o, d = rays.orthographic(40, 30, 9.0, view_transform(point(1, 6, -4), point(0, 0.4, 7), vector(0, 1, 0)), device="cuda:0")
    n = o.shape[0]
    keys = np.arange(n, dtype=np.uint32)
    ho, hd = o.cpu().numpy(), d.cpu().numpy()  # the very bits the device traces
    exp, exp_rays = _oracle_colors(case["own"], ho, hd, keys, case["depth"])
    r = Renderer(case["world"], case["camera"], device=0)
    got = _trace(r, o, d, case["depth"])
    st = r.stats()
    r.close()
    _equal(got, exp, "%s rays against the oracle" % which)
    assert st["rays"] == exp_rays, (st["rays"], exp_rays)
    assert len(np.unique(got, axis=0)) > 16  # (they see the scene)


# ---- arguments ------------------------------------------------------------------------
def test_trace_checks_its_tensors(case, traced):
    r = Renderer(case["world"], case["camera"], device=0)
    o, d, k = traced["o"], traced["d"], traced["k"]
    bad = [
        (o.cpu(), d, None, None), (o, d[:-1], None, None), (o[:, :3].contiguous(), d, None, None), (o.double(), d, None, None),
        (o.t().contiguous().t(), d, None, None),                              # not contiguous
        (torch.cat([o.reshape(-1)[:1], o.reshape(-1)])[1:].reshape(-1, 4), d, None, None),  # 4-byte aligned only
        (o, d, k[:-1], None), (o, d, k.float(), None), (o, d, k.cpu(), None),
        (o, d, k, torch.empty((N, 4), dtype=torch.float32, device="cuda:0")), (o, d, k, torch.empty((N, 3), dtype=torch.float32)),
    ]
    for oo, dd, kk, out in bad:
        with pytest.raises(ValueError):
            r.trace(oo, dd, case["depth"], keys=kk, out=out)
    with pytest.raises(ValueError):
        r.camera_rays(y0=30, n_rows=7)
    # nothing to trace: an empty answer, no launch
    empty = r.trace(o[:0].contiguous(), d[:0].contiguous(), case["depth"])
    assert empty.shape == (0, 3)
    assert r.trace_kernel_name == ""  # no trace of this scene has been launched
    r.close()
