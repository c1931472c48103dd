"""First-hit buffers on the device (-m gpu): World.hit_at (rtc_hit_at) and Renderer.render_hits (rtc_ctx_render_hits)
against the reference's own known-answer vectors, against the oracle field by field, against each other on whole
frames, and against the render they are the front half of.  Every comparison is bit-exact with == semantics
(tests/hits_helpers.py::same: +0.0 equals -0.0, NaN equals NaN; integers exactly).

"First hit": xs = World::intersect(ray); hit = Intersection::hit(xs); comps = precompute_values(ray, hit, xs) for every
hit, opaque or not; light = intensity_at(comps.over_point) drawn as (pixel index, path 1)."""
import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests import hits_helpers as HH
from tests import kat as K
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL = HH.PLANES


def _device_planes(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _flat(planes):
    """(rows, w[, k]) planes as (rows * w[, k]): image order, the order of hits_helpers.camera_rays."""
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in planes.items()}


# ---------------------------------------------------------------- 1. the reference's own vectors, on the device
def test_precompute_vectors_of_the_reference(kat):  # world.rs:334-381
    w = P.World([P.Sphere()], P.PointLight(P.point(0, 0, 0), P.color(1, 1, 1)))
    for key in ("precompute_state", "precompute_inside"):
        c = kat["world"][key]
        r = w.hit_at(K.point(c["ray"][0]), K.vector(c["ray"][1]))
        assert r.object[0] == 0
        assert r.distance[0] == f32(c["t"])
        K.assert_exact(r.point[0], c["point"])
        K.assert_exact(r.eye[0], c["eye"])
        K.assert_exact(r.normal[0], c["normal"])
        assert bool(r.inside[0]) == c["inside"]
    c = kat["world"]["precompute_reflection_vector"]
    w = P.World([P.Plane()], P.PointLight(P.point(0, 0, 0), P.color(1, 1, 1)))
    r = w.hit_at(K.point(c["ray"][0]), K.vector(c["ray"][1]))
    assert r.object[0] == 0
    K.assert_exact(r.reflectv[0], K.vec(c["reflectv"]))


def test_intersect_world_with_ray_vector_of_the_reference(kat):  # world.rs:322-332
    c = kat["world"]["intersect_world_with_ray"]
    r = P.default_world().hit_at(K.point(c["ray"][0]), K.vector(c["ray"][1]))
    assert r.distance[0] == f32(c["expect_exact"][0]) == f32(4.0) and r.object[0] == 0


def test_find_n1_and_n2_vector_of_the_reference(kat):  # world.rs:396-451
    """The vector asks precompute_values about each of six intersections of ONE ray.  A ray that starts 0.125 before
    entry k on the same line has exactly the entries before k behind its origin (z = -4 + t - 0.125 is exact in f32), and
    entry k as its first hit."""
    c = kat["world"]["find_n1_and_n2"]

    def glass(transform, ri):
        return P.Sphere(transform, P.Material(transparency=1.0, refractive_index=ri))
    w = P.World([glass(P.scaling(2.0, 2.0, 2.0), 1.5), glass(P.translation(0.0, 0.0, -0.25), 2.0),
                 glass(P.translation(0.0, 0.0, 0.25), 2.5)], P.PointLight(P.point(0, 0, 0), P.color(1, 1, 1)))
    assert c["ray"] == [[0, 0, -4], [0, 0, 1]]
    o = np.array([[0.0, 0.0, -4.0 + t - 0.125, 1.0] for t, _ in c["xs"]], dtype=f32)
    d = np.tile(np.array([0, 0, 1, 0], dtype=f32), (len(c["xs"]), 1))
    r = w.hit_at(o, d)
    assert list(r.object) == [obj for _, obj in c["xs"]]
    assert (r.distance == f32(0.125)).all()
    for i, (n1, n2) in enumerate(c["expect_exact"]):
        assert r.n1n2[i, 0] == f32(n1) and r.n1n2[i, 1] == f32(n2), (i, r.n1n2[i])


def test_a_cycled_jitter_light_is_refused_for_the_light_plane_only():
    """RTC_JITTER_SEQUENCE (test/utils.rs hardcoded_jitter) is state carried from call to call: the light plane would draw from
    it and is refused as a render is; the geometry planes draw nothing and are answered."""
    w = P.default_world()
    w.light = P.RectangleLight(P.color(1, 1, 1), P.point(-0.5, -0.5, -5), P.vector(1, 0, 0), 2, P.vector(0, 1, 0), 2, ("cycle", [0.7, 0.3]))
    o, d = np.array([[0, 0, -5, 1]], dtype=f32), np.array([[0, 0, 1, 0]], dtype=f32)
    with pytest.raises(P.RtcError) as e:
        w.hit_at(o, d)
    assert "sequence jitter" in str(e.value)
    with pytest.raises(P.RtcError):
        w.hit_at(o, d, planes=("light",))
    r = w.hit_at(o, d, light=False)
    assert r.light is None and r.object[0] == 0 and r.distance[0] == f32(4.0) and r.inside[0] == 0
    HH.assert_planes_equal(r.planes(), HH.oracle_first_hits(H.oracle_world(P.default_world()), o, d, light=False), "cycled light", planes=HH.GEOMETRY)


# ---------------------------------------------------------------- 2. batched rays against the oracle, every field
SMALL = (56, 36)
SCENES = {
    "C1_C3_soft_shadows": lambda: scenes.soft_shadows(*SMALL), "C2_single_sphere": lambda: scenes.single_sphere(*SMALL),
    "C4_glass_and_mirror": lambda: scenes.glass_and_mirror(*SMALL), "C5_sphere_grid": lambda: scenes.sphere_grid(*SMALL),
    "first_scene": lambda: scenes.first_scene(*SMALL), "first_plane": lambda: scenes.first_plane(*SMALL),
    "first_patterns": lambda: scenes.first_patterns(*SMALL), "reflect_refract": lambda: scenes.reflect_refract(*SMALL),
    "patterns_medley": lambda: scenes.patterns_medley(*SMALL), "hexagons": lambda: scenes.hexagons(*SMALL),
    "grouped_grid": lambda: scenes.grouped_grid(*SMALL), "groups_medley": lambda: scenes.groups_medley(*SMALL),
    "mesh": lambda: scenes.mesh(*SMALL), "here_be_dragons": lambda: scenes.here_be_dragons(*SMALL, nu=24, nv=16),
    "first_textures": lambda: scenes.first_textures(*SMALL), "skybox": lambda: scenes.skybox(*SMALL),
    "shapes_medley": lambda: scenes.shapes_medley(*SMALL),
}
N_INSIDE = 400  # rays that start inside the scene, per world


def _inside_rays(seed, points):
    """Seeded rays whose origins lie in the bounds of `points` (first hits the camera sees) and point anywhere: inside hits,
    containers behind the origin, overlapping glass."""
    rng = np.random.default_rng(seed)
    pts = points[np.isfinite(points).all(axis=1)][:, :3].astype(np.float64)
    lo, hi = (pts.min(axis=0), pts.max(axis=0)) if len(pts) else (-np.ones(3), np.ones(3))
    pad = 0.1 * np.maximum(hi - lo, 1e-3)
    o = np.ones((N_INSIDE, 4), dtype=f32)
    o[:, :3] = rng.uniform(lo - pad, hi + pad, (N_INSIDE, 3))
    v = rng.normal(size=(N_INSIDE, 3))
    d = np.zeros((N_INSIDE, 4), dtype=f32)
    d[:, :3] = v / np.linalg.norm(v, axis=1)[:, None]
    return o, d


def _check_rays_against_the_oracle(world, own, camera, seed, what):
    o, d = HH.camera_rays(camera)
    # (the rays are the camera's: rtc_ray_for_pixel on the host agrees with the kernels' arithmetic)
    for x, y in ((0, 0), (camera.width - 2, camera.height - 2), (camera.width // 2, camera.height // 3)):
        ho, hd = camera.ray_for_pixel(x, y)
        assert HH.same(ho, o[y * camera.width + x]).all() and HH.same(hd, d[y * camera.width + x]).all(), (x, y)
    exp = HH.oracle_first_hits(own, o, d)
    got = world.hit_at(o, d).planes()
    HH.assert_planes_equal(got, exp, what + ": camera rays")
    hits = exp["object"] >= 0
    io, idr = _inside_rays(seed, exp["point"][hits])
    exp_in = HH.oracle_first_hits(own, io, idr)
    got_in = world.hit_at(io, idr).planes()
    HH.assert_planes_equal(got_in, exp_in, what + ": rays from inside")
    # geometry only: the same values without the light plane, which is then not there
    geo = world.hit_at(io, idr, light=False)
    assert geo.light is None
    HH.assert_planes_equal(geo.planes(), exp_in, what + ": rays from inside, light=False", planes=HH.GEOMETRY)
    return int(hits.sum()), int((exp_in["object"] >= 0).sum()), int(exp_in["inside"].sum())


@pytest.mark.parametrize("name", list(SCENES))
def test_batched_rays_match_the_oracle_in_every_field(name):
    world, camera, _ = SCENES[name]()
    n_hit, n_in_hit, n_inside = _check_rays_against_the_oracle(world, H.oracle_world(world), camera, 1000 + len(name), name)
    assert n_hit > 0 and n_in_hit > 0, (name, n_hit, n_in_hit)  # (the comparison is not one of misses with misses)


@pytest.mark.parametrize("seed", range(24))
def test_batched_rays_of_wide_worlds_match_the_oracle_in_every_field(seed):
    world, cam, _, style = W.world(seed, P)
    own, _, _, _ = W.world(seed, O)
    camera = P.Camera(SMALL[0], SMALL[1], cam[2], cam[3])
    _check_rays_against_the_oracle(world, own, camera, seed, "wide seed %d [%s]" % (seed, style))


# ---------------------------------------------------------------- 3. frame planes
def _frame(world, camera, planes=ALL, part=None):
    r = Renderer(world, camera, device=0)
    got = _device_planes(r.render_hits(planes=planes, part=part))
    r.close()
    return got


def _oracle_frame(own, camera):
    """The oracle's planes for a whole frame -- the last row and column as misses."""
    o, d = HH.camera_rays(camera)
    w, h = camera.width, camera.height
    traced = np.array([y * w + x for y in range(h - 1) for x in range(w - 1)], dtype=np.int64)
    exp = HH.empty_planes(w * h)
    if len(traced):
        part = HH.oracle_first_hits(own, o[traced], d[traced], pixels=traced)
        for k in exp:
            exp[k][traced] = part[k]
    return exp


@pytest.mark.parametrize("name,size", [("soft_shadows", (37, 23)), ("soft_shadows", (17, 3)), ("soft_shadows", (2, 2)),
                                       ("groups_medley", (37, 23)), ("groups_medley", (17, 3)), ("groups_medley", (2, 2)),
                                       ("reflect_refract", (37, 23)), ("sphere_grid", (37, 23)), ("mesh", (37, 23))])
def test_whole_small_frames_match_the_oracle(name, size):
    world, camera, _ = getattr(scenes, name)(*size)
    got = _flat(_frame(world, camera))
    exp = _oracle_frame(H.oracle_world(world), camera)
    HH.assert_planes_equal(got, exp, "%s %dx%d" % (name, size[0], size[1]))
    w, h = size
    last = np.zeros((h, w), dtype=bool)
    last[-1, :] = last[:, -1] = True
    assert (got["object"][last.reshape(-1)] == -1).all()
    for k in ALL:
        if k != "object":
            assert not got[k][last.reshape(-1)].any(), k


BIG = {
    # name -> (scene, planes compared device against device on every pixel)
    "C3_4096": (lambda: scenes.CONFIGS["C3"](), ("object", "distance", "normal", "inside", "light")),
    "C4_1024": (lambda: scenes.glass_and_mirror(1024, 1024), ALL),
    "mesh_1024": (lambda: scenes.mesh(1024, 1024), ALL),
}


@pytest.mark.parametrize("name", list(BIG))
def test_every_pixel_of_a_full_frame_equals_hit_at_on_the_cameras_rays(name, monkeypatch):
    """render_hits against hit_at on the camera's own rays, every pixel (device against device: two kernel families, two
    launch shapes), and both against the oracle on a seeded sample of 5 000 pixels.  hit_at's ray index is its jitter key:
    the rays go in image order, in one call."""
    make, planes = BIG[name]
    world, camera, _ = make()
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", "0")  # (no render follows: the scene's render kernel need not be compiled)
    w, h = camera.width, camera.height
    got = _flat(_frame(world, camera, planes=planes))
    o, d = HH.camera_rays(camera)
    ref = world.hit_at(o, d, planes=planes).planes()
    assert len(o) == w * h and all(got[k].shape[0] == w * h for k in planes)
    print("\n%s: %d x %d, %d rays, %d of them hits" % (name, w, h, len(o), int((got["object"] >= 0).sum())), flush=True)
    # the last row and column are not traced: misses in the frame, whatever their rays would hit
    untraced = np.zeros((h, w), dtype=bool)
    untraced[-1, :] = untraced[:, -1] = True
    untraced = untraced.reshape(-1)
    miss = HH.empty_planes(1, planes)
    for k in planes:
        ref[k][untraced] = miss[k][0]
    HH.assert_planes_equal(got, ref, name + ": render_hits against hit_at")
    del ref
    rng = np.random.default_rng(5000)
    ys, xs = rng.integers(0, h - 1, 5000), rng.integers(0, w - 1, 5000)
    idx = ys.astype(np.int64) * w + xs
    exp = HH.oracle_first_hits(H.oracle_world(world), o[idx], d[idx], pixels=idx)
    HH.assert_planes_equal({k: got[k][idx] for k in planes}, exp, name + ": render_hits against the oracle, 5 000 pixels", planes=planes)
    print("%s: %d oracle samples compared, %d of them hits" % (name, len(idx), int((exp["object"] >= 0).sum())), flush=True)
    assert (exp["object"] >= 0).sum() > 500


@pytest.mark.parametrize("name,size", [("soft_shadows", (150, 200)), ("groups_medley", (97, 161))])
@pytest.mark.parametrize("band_rows", [64, 7])
@pytest.mark.parametrize("n_parts", [2, 3])
def test_the_parts_of_a_frame_put_back_together_are_the_frame(name, size, band_rows, n_parts):
    world, camera, _ = getattr(scenes, name)(*size)
    r = Renderer(world, camera, device=0)
    whole = _device_planes(r.render_hits(planes=ALL))
    h = camera.height
    n_bands = (h + band_rows - 1) // band_rows
    for part in range(n_parts):
        q = Renderer.partition(band_rows, n_parts, part)
        got = _device_planes(r.render_hits(planes=ALL, part=q))
        rows = [y for b in range(part, n_bands, n_parts) for y in range(b * band_rows, min(h, (b + 1) * band_rows))]
        assert r.rows(q) == len(rows)
        HH.assert_planes_equal(got, {k: whole[k][rows] for k in ALL}, "%s part %d of %d, bands of %d" % (name, part, n_parts, band_rows))
    r.close()


@pytest.mark.parametrize("subset", [("distance",), ("object", "distance", "normal"), ("light",), ("n1n2", "inside"), ("reflectv", "under_point", "light")])
def test_a_subset_of_planes_has_the_same_values_and_leaves_the_other_buffers_alone(subset):
    world, camera, _ = scenes.groups_medley(90, 70)
    r = Renderer(world, camera, device=0)
    whole = _device_planes(r.render_hits(planes=ALL))
    bufs = {}
    for k in ALL:
        is_int, per = L.HIT_PLANES[k]
        shape = (camera.height, camera.width, per) if per > 1 else (camera.height, camera.width)
        bufs[k] = torch.full(shape, -77, dtype=torch.int32 if is_int else torch.float32, device="cuda:0")
    res = r.render_hits(planes=subset, out=bufs)
    assert set(res) == set(subset)
    got = _device_planes(bufs)
    for k in ALL:
        if k in subset:
            assert res[k] is bufs[k]
            assert HH.same(got[k], whole[k]).all(), k
        else:
            assert (got[k] == -77).all(), k
    # the same for the batched call
    o, d = HH.camera_rays(camera)
    full = world.hit_at(o, d).planes()
    part = world.hit_at(o, d, planes=subset).planes()
    assert set(part) == set(subset)
    HH.assert_planes_equal(part, full, "hit_at subset", planes=subset)
    with pytest.raises(ValueError):
        r.render_hits(planes=())
    r.close()


def test_caller_supplied_tensors_are_checked_like_renders():
    world, camera, _ = scenes.soft_shadows(40, 30)
    r = Renderer(world, camera, device=0)
    ok = torch.empty((30, 40, 4), dtype=torch.float32, device="cuda:0")
    r.render_hits(planes=("normal",), out={"normal": ok})
    for bad in (torch.empty((30, 40, 3), dtype=torch.float32, device="cuda:0"), torch.empty((30, 40, 4), dtype=torch.float64, device="cuda:0"),
                torch.empty((30, 40, 4), dtype=torch.float32), torch.empty((30, 40, 8), dtype=torch.float32, device="cuda:0")[:, :, ::2]):
        with pytest.raises(ValueError):
            r.render_hits(planes=("normal",), out={"normal": bad})
    with pytest.raises(ValueError):
        r.render_hits(planes=("object",), out={"object": torch.empty((30, 40), dtype=torch.float32, device="cuda:0")})
    with pytest.raises(ValueError):
        r.render_hits(planes=("colour",))
    r.close()


# ---------------------------------------------------------------- 4. the planes are what the render used
@pytest.mark.parametrize("name,size", [("soft_shadows", (100, 40)), ("reflect_refract", (100, 50)), ("shapes_medley", (96, 72))])
def test_the_surface_colour_of_the_planes_is_the_depth_0_render(name, size):
    """At depth 0 both recursive terms of shade_hit are black (world.rs:62-86): the pixel is phong_lighting of the planes."""
    world, camera, _ = getattr(scenes, name)(*size)
    r = Renderer(world, camera, device=0)
    pl = _flat(_device_planes(r.render_hits(planes=("object", "over_point", "eye", "normal", "light"))))
    img = r.render(0).cpu().numpy().reshape(-1, 3)
    r.close()
    own = H.oracle_world(world)
    leaves = [H.oracle_shape(s) for s in world._c().leaves]
    exp = np.zeros_like(img)
    for i in np.flatnonzero(pl["object"] >= 0):
        s = leaves[pl["object"][i]]
        exp[i] = own.phong_lighting(s.material, pl["over_point"][i], pl["eye"][i], pl["normal"][i], pl["light"][i], shape=s)
    assert (pl["object"] >= 0).sum() > size[0] * size[1] // 4
    H.assert_images_equal(img.reshape(size[1], size[0], 3), exp.reshape(size[1], size[0], 3), name + " depth 0 from its planes")
    assert not img[pl["object"] < 0].any()  # misses are black


# ---------------------------------------------------------------- 5. same bits under every policy
POLICIES = [{}, {"RTC_AMD_LIGHT_CULL": "0", "RTC_AMD_FAST_SHADOW": "0", "RTC_AMD_CELL_CULL": "0", "RTC_AMD_DARK": "0"},
            {"RTC_AMD_PRUNE": "0", "RTC_AMD_BVH": "0", "RTC_AMD_GATES": "0", "RTC_AMD_TRI_PRECULL": "0", "RTC_AMD_CLUSTERS": "0"}]


@pytest.mark.parametrize("name", ["C1", "groups_medley"])
def test_the_planes_are_the_same_bits_under_every_policy(name, monkeypatch):
    world, camera, _ = scenes.CONFIGS["C1"]() if name == "C1" else scenes.groups_medley()
    o, d = HH.camera_rays(camera, ys=range(0, camera.height, 7))
    frames, batches = [], []
    for env in POLICIES:  # (the environment is read when a context is created, and by every batched call)
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            frames.append(_frame(world, camera))
            batches.append(world.hit_at(o, d).planes())
    for i in (1, 2):
        HH.assert_planes_equal(frames[i], frames[0], "%s render_hits under %r" % (name, POLICIES[i]))
        HH.assert_planes_equal(batches[i], batches[0], "%s hit_at under %r" % (name, POLICIES[i]))
    assert (frames[0]["object"] >= 0).sum() > 1000


# ---------------------------------------------------------------- 6. nothing existing moves
@pytest.mark.parametrize("name", ["C1", "mesh"])
def test_a_render_after_render_hits_is_the_render_it_would_have_been(name):
    """Frame, kernel id, kernel name and counters of four renders on one context (the second and later are scheduled by
    what the ones before measured) are the same with a render_hits in front of each as without."""
    world, camera, depth = scenes.CONFIGS["C1"]() if name == "C1" else scenes.mesh()

    def four_frames(with_hits):
        r = Renderer(world, camera, device=0)
        seen = []
        for frame in range(4):
            if with_hits:
                r.render_hits(planes=ALL if frame % 2 else ("object", "light"))
            img = r.render(depth).cpu().numpy()
            st = r.stats()
            seen.append((img, r.kernel_id, r.kernel_name, st["rays"], st["shaded_hits"], st["launches"], st["rows"], st["pixels"]))
            assert st["rays"] > camera.width * camera.height and img.any()
        r.close()
        return seen
    plain, mixed = four_frames(False), four_frames(True)
    for frame, (a, b) in enumerate(zip(plain, mixed)):
        H.assert_images_equal(b[0], a[0], "%s frame %d after render_hits" % (name, frame))
        assert a[1:] == b[1:], (name, frame, a[1:], b[1:])
        assert a[5] == 1
