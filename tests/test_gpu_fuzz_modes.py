"""Random worlds through every mode (-m gpu): the worlds of tests/test_gpu_fuzz.py and tests/wide_worlds.py -- all six shape kinds
under shears and negative scales, nested and divided groups, small meshes, non-casters, planes inside groups, thin discs 1e4 from
the origin, lights that touch casters -- through the kernels that have only ever seen the named demo scenes: the supersampling
kernel, the lens kernel, adaptive refinement and its mask, ray streams plain and reordered, first hits and occlusion, and the
one-call seam's siblings of the first three.  Every one of them has an entry point, a stash layout, header tweaks, ahead-of-time
instantiations and a scene-compiled variant of its own; what they share is color_at<NOBJ, SIMPLE>.

Every comparison is bit-exact against the CPU oracle (tests.helpers.assert_images_equal, tests.hits_helpers.assert_planes_equal),
ray counts included.  The oracle side of each mode is what the mode's own test file uses.  The seed list, and the kernel family each
seed gets, live in tests/fuzz_modes_helpers.py; tests/test_fuzz_modes_plan.py asserts without a GPU that every ahead-of-time family
is there at least twice and that the adaptive thresholds flag a useful share of pixels.

Each (seed, mode) runs under RTC_AMD_SPECIALIZE=0; the first seed of each family runs under =1 as well (at most two scene
kernels compiled per test).

The second half is a directed test of ray streams that start far from a world with the library's own hierarchy (ERROR_BUDGET.md
B9): origins up to 1e4 radii from the objects, where the f32 quadratic reports hits for lines that miss the padded boxes."""
import functools

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import rays
from ray_tracer_challenge_amd.renderer import Renderer
from tests import fuzz_modes_helpers as FM
from tests import helpers as H
from tests import hits_helpers as HH
from tests import lens_helpers as LH
from tests import trace_hits_helpers as TH
from tests.adaptive_helpers import compose, edge_mask
from tests.supersample_helpers import box_filter
from tests.test_flat_bvh import _cloud

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
ALL = HH.PLANES
MODES = ("supersample", "lens", "adaptive", "trace", "hits", "seam_supersample", "seam_lens", "seam_adaptive")
# the seeds that also run under RTC_AMD_SPECIALIZE=1: the first of each family in the list's order (tests/test_fuzz_modes_plan.py
# asserts that these are they)
SPECIALISED = FM.SPECIALISED
CASES = [(gen, seed, mode, "0") for gen, seed in FM.all_seeds() for mode in MODES] + \
        [(gen, seed, mode, "1") for gen, seed in SPECIALISED for mode in MODES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _keys_tensor(keys):
    """uint32 keys as the int32 tensor that carries their bits"""
    return _dev(np.asarray(keys, dtype=np.uint32).view(np.int32).copy())


def _host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _oracle_colors(own, origins, directions, keys, depth):
    """World::color_at ray by ray, ray i drawing as pixel keys[i] -> ((n, 3) colours, rays traced)."""
    out = np.zeros((len(origins), 3), dtype=f32)
    before = own.ray_count
    for i in range(len(origins)):
        own.set_pixel(int(keys[i]))
        out[i] = own.color_at(origins[i], directions[i], depth)
    return out, own.ray_count - before


def _colours_equal(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    H.assert_images_equal(got.reshape(1, -1, 3), exp.reshape(1, -1, 3), what)  # ("x" in the message is the ray's index)


def _seam_kernel():
    """The render kernel's name in the seam's first context (for messages)."""
    lib = P.lib()
    try:
        return lib.rtc_ctx_kernel_name(lib.rtc_diag_seam_ctx(0)).decode()
    except Exception:  # noqa: BLE001 -- a message must not hide the failure it describes
        return "?"


# ---------------------------------------------------------------- the modes
def _supersample(b, what, gen, seed):
    for k in (2, 4):
        fine, rays_exp = FM.oracle_frame(gen, seed, k)
        camera = b["camera"]
        r = Renderer(b["world"], camera, device=0, supersample=k)
        try:
            got = _np(r.render(b["depth"]))
            st = r.stats()
            w = "%s k=%d (%s)" % (what, k, r.kernel_name)
            assert r.kernel_name.startswith("ss_render_kernel"), w
            H.assert_images_equal(got, box_filter(fine, k), w)
            assert st["rays"] == rays_exp, (w, st["rays"], rays_exp)
            assert st["pixels"] == (k * camera.width - 1) * (k * camera.height - 1), (w, st["pixels"])
        finally:
            r.close()


@functools.lru_cache(maxsize=None)
def _lens_oracle(gen, seed):
    camera, lens = FM.lens_case(gen, seed)
    b = FM.build(gen, seed)
    frame, n_rays, _ = LH.oracle_lens_frame(b["own"], camera, b["depth"], 2, lens)
    frame.setflags(write=False)
    return frame, n_rays


def _lens(b, what, gen, seed):
    camera, lens = FM.lens_case(gen, seed)
    exp, rays_exp = _lens_oracle(gen, seed)
    r = Renderer(b["world"], camera, device=0, supersample=2, lens=lens)
    try:
        got = _np(r.render(b["depth"]))
        st = r.stats()
        w = "%s %r (%s)" % (what, lens, r.kernel_name)
        assert r.kernel_name.startswith("lens_render_kernel"), w
        H.assert_images_equal(got, exp, w)
        assert st["rays"] == rays_exp, (w, st["rays"], rays_exp)
        assert st["pixels"] == (2 * camera.width - 1) * (2 * camera.height - 1), (w, st["pixels"])
    finally:
        r.close()


def _adaptive_expected(gen, seed):
    B, base_rays = FM.oracle_frame(gen, seed, 1)
    fine, _ = FM.oracle_frame(gen, seed, 2)
    t = FM.threshold_of(B)
    M = edge_mask(B, t)
    return compose(B, box_filter(fine, 2), M), M, t, base_rays


def _adaptive(b, what, gen, seed):
    exp, M, t, base_rays = _adaptive_expected(gen, seed)
    r = Renderer(b["world"], b["camera"], device=0)
    try:
        res = r.render_adaptive(b["depth"], k=2, threshold=t, mask=True)
        got, mask = _np(res[0]), _np(res[1])
        w = "%s threshold=%r (%s, %s)" % (what, t, r.kernel_name, r.adaptive_kernel_name)
        assert mask.shape == M.shape, w
        bad = mask != M.astype(np.uint8)
        assert not bad.any(), "%s: the mask differs at %d pixels (first: y, x = %s)" % (w, int(bad.sum()), np.argwhere(bad)[0])
        H.assert_images_equal(got, exp, w)
        assert r.adaptive_stats()["refined_pixels"] == int(M.sum()), w
        assert r.stats()["rays"] == base_rays, (w, r.stats()["rays"], base_rays)
    finally:
        r.close()


def _permutation(n):
    return np.random.RandomState(4321).permutation(n)


def _trace(b, what, gen, seed):
    own, depth = b["own"], b["depth"]
    r = Renderer(b["world"], b["camera"], device=0)
    try:
        o, d, k = r.camera_rays()
        ho, hd = _np(o), _np(d)  # the very bits the device traces
        n = ho.shape[0]
        # 1. the camera's own rays, keys=None: ray i draws as pixel i
        exp, rays_exp = _oracle_colors(own, ho, hd, np.arange(n), depth)
        got = _np(r.trace(o, d, depth))
        w = "%s (%s)" % (what, r.trace_kernel_name)
        assert r.trace_kernel_name.startswith("trace_kernel"), w
        _colours_equal(got, exp, w + ": the camera's rays, keys=None")
        assert r.stats()["rays"] == rays_exp, (w, r.stats()["rays"], rays_exp)
        # 2. the same rays shuffled, with scrambled keys: plain and reordered on the device
        perm, keys = _permutation(n), TH.scrambled_keys(n)
        tp = _dev(perm)
        po, pd, pk = o[tp].contiguous(), d[tp].contiguous(), _keys_tensor(keys)
        exp, rays_exp = _oracle_colors(own, ho[perm], hd[perm], keys, depth)
        for reorder in (False, True):
            got = _np(r.trace(po, pd, depth, keys=pk, reorder=reorder))
            _colours_equal(got, exp, "%s: shuffled rays, scrambled keys, reorder=%r" % (w, reorder))
            assert r.stats()["rays"] == rays_exp, (w, reorder, r.stats()["rays"], rays_exp)
        # 3. the second bounce, made on the device from the device's own first hits
        first = r.trace_hits(o, d, keys=k, planes=ALL)
        so, sd, _ = rays.reflected(first, d)
        m = int(so.shape[0])
        if m:
            keys = TH.scrambled_keys(m)
            exp, rays_exp = _oracle_colors(own, _np(so), _np(sd), keys, depth)
            got = _np(r.trace(so, sd, depth, keys=_keys_tensor(keys)))
            _colours_equal(got, exp, "%s: the reflected stream (%d rays)" % (w, m))
            assert r.stats()["rays"] == rays_exp, (w, r.stats()["rays"], rays_exp)
    finally:
        r.close()


def _inner(planes, h, w):
    """flat planes of an h x w frame -> the pixels a render traces (camera.rs:80-81)"""
    return {k: np.asarray(v).reshape((h, w) + tuple(np.asarray(v).shape[1:]))[:-1, :-1] for k, v in planes.items()}


def _hits(b, what, gen, seed):
    own, camera = b["own"], b["camera"]
    h, wd = camera.height, camera.width
    r = Renderer(b["world"], camera, device=0)
    try:
        w = "%s (%s)" % (what, r.kernel_name)
        o, d, k = r.camera_rays()
        ho, hd = _np(o), _np(d)
        n = ho.shape[0]
        exp = HH.oracle_first_hits(own, ho, hd)
        frame = _host(r.render_hits(planes=ALL))
        flat = {p: v.reshape((-1,) + tuple(v.shape[2:])) for p, v in frame.items()}
        HH.assert_planes_equal(_inner(flat, h, wd), _inner(exp, h, wd), w + ": render_hits, the traced pixels")
        perm, keys = _permutation(n), TH.scrambled_keys(n)
        tp = _dev(perm)
        got_dev = r.trace_hits(o[tp].contiguous(), d[tp].contiguous(), keys=_keys_tensor(keys), planes=ALL)
        got = _host(got_dev)
        exp_p = HH.oracle_first_hits(own, ho[perm], hd[perm], pixels=keys)
        HH.assert_planes_equal(got, exp_p, w + ": trace_hits of the shuffled rays, scrambled keys")
        # mutual visibility of the hit points (over_point of every hit, as the device has them)
        hit = got_dev["object"] >= 0
        points = got_dev["over_point"][hit].contiguous()
        m = int(points.shape[0])
        if m:
            lights, pts = TH.visibility_pairs(points)
            hl, hp = _np(lights), _np(pts)
            exp_s = np.array([own.is_shadowed(hl[i], hp[i]) for i in range(m)], dtype=np.int32)
            got_s = _np(r.is_shadowed(lights, pts))
            bad = got_s != exp_s
            assert not bad.any(), "%s: is_shadowed differs for %d of %d pairs (first: pair %d)" % (w, int(bad.sum()), m, int(np.argmax(bad)))
    finally:
        r.close()


def _seam(b, what, camera, exp, rays_exp, **kw):
    """One call each: f32 and quantized, whole and in 7-row bands dealt over two entries of device 0."""
    exp8 = O.quantize(exp)
    for band in (0, 7):
        for quantize in (False, True):
            got = camera.render(b["world"], b["depth"], devices=[0, 0], band_rows=band, quantize=quantize, **kw)
            w = "%s band_rows=%d quantize=%r (%s)" % (what, band, quantize, _seam_kernel())
            if quantize:
                bad = got != exp8
                assert not bad.any(), "%s: %d bytes differ (first: y, x, c = %s)" % (w, int(bad.sum()), np.argwhere(bad)[0])
            else:
                H.assert_images_equal(got.data, exp, w)
            assert camera.last_stats["rays"] == rays_exp, (w, camera.last_stats["rays"], rays_exp)


def _seam_supersample(b, what, gen, seed):
    fine, rays_exp = FM.oracle_frame(gen, seed, 2)
    _seam(b, what, b["camera"], box_filter(fine, 2), rays_exp, supersample=2)


def _seam_lens(b, what, gen, seed):
    camera, lens = FM.lens_case(gen, seed)
    exp, rays_exp = _lens_oracle(gen, seed)
    _seam(b, what, camera, exp, rays_exp, supersample=2, lens=lens)


def _seam_adaptive(b, what, gen, seed):
    exp, M, t, base_rays = _adaptive_expected(gen, seed)
    _seam(b, "%s threshold=%r" % (what, t), b["camera"], exp, base_rays, supersample=2, adaptive=t)


RUN = {"supersample": _supersample, "lens": _lens, "adaptive": _adaptive, "trace": _trace, "hits": _hits,
       "seam_supersample": _seam_supersample, "seam_lens": _seam_lens, "seam_adaptive": _seam_adaptive}


@pytest.mark.parametrize("gen,seed,mode,specialise", CASES, ids=["%s%d-%s-spec%s" % c for c in CASES])
def test_random_worlds_through_every_mode(gen, seed, mode, specialise, monkeypatch):
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
    b = FM.build(gen, seed)
    what = "%s seed %d [%s] %s specialise=%s" % (gen, seed, b["style"], mode, specialise)
    try:
        RUN[mode](b, what, gen, seed)
    finally:
        if mode.startswith("seam"):
            P.lib().rtc_render_release()  # (the seam keeps its contexts between calls; they read the switch when created)


# ---------------------------------------------------------------- ray streams that start far from a flat-BVH world
DISTANCES = (30.0, 300.0, 3000.0, 10000.0)  # in radii of the object aimed at
RAYS_PER = 64


def _far_worlds():
    world, camera, depth = TH.spheres(4)
    cloud, cloud_camera = _cloud(7, 20)
    return {"spheres4": (world, camera, depth), "cloud": (cloud, cloud_camera, 4)}


def _centre_and_half(obj):
    """World-space centre and half extents of a scale + translate-only sphere or cube, in double precision."""
    m = np.asarray(obj.transform, dtype=np.float64).reshape(4, 4)
    assert np.count_nonzero(m[:3, :3] - np.diag(np.diag(m[:3, :3]))) == 0
    return m[:3, 3].copy(), np.abs(np.diag(m[:3, :3]))


@functools.lru_cache(maxsize=None)
def _far_case(name):
    """The rays, on the host: for each object and each D, RAYS_PER oblique rays whose line passes m in [0.9, 2.0] radii (of the
    object's smallest half extent) from the object's centre, the origin D radii back along the ray; the oracle's answers for them;
    and which of their lines miss the padded box of the object the oracle says they hit."""
    world, camera, depth = _far_worlds()[name]
    own = H.oracle_world(world)
    rng = np.random.default_rng(20240 + len(name))
    boxes = [_centre_and_half(ob) for ob in world.objects]
    os_, ds_, dist, beyond = [], [], [], []
    for c, h in boxes:
        rad = float(h.min())
        for D in DISTANCES:
            for _ in range(RAYS_PER):
                u = rng.normal(size=3)
                u /= np.linalg.norm(u)
                v = np.cross(u, rng.normal(size=3))
                v /= np.linalg.norm(v)
                near = c + v * rng.uniform(0.9, 2.0) * rad  # the line's closest point to the centre
                os_.append(near - u * D * rad)
                ds_.append(u)
                dist.append(D)
                beyond.append(near + u * 2.0 * rad)  # 2 radii beyond the object along the ray
    n = len(os_)
    o = np.concatenate([np.array(os_), np.ones((n, 1))], axis=1).astype(f32)
    d = np.concatenate([np.array(ds_), np.zeros((n, 1))], axis=1).astype(f32)
    p = np.concatenate([np.array(beyond), np.ones((n, 1))], axis=1).astype(f32)
    dist = np.array(dist)
    keys = TH.scrambled_keys(n)
    hits = HH.oracle_first_hits(own, o, d, pixels=keys)
    colours, n_rays = _oracle_colors(own, o, d, keys, depth)
    shadowed = np.array([own.is_shadowed(o[i], p[i]) for i in range(n)], dtype=np.int32)
    # not hollow: rays the oracle gives a hit although their line (the f32 ray's, in double precision) misses the hit object's box
    # with the library's own padding, 0.1 h + 1e-4 (|c| + h) per axis
    outside = np.zeros(n, dtype=bool)
    o64, d64 = o[:, :3].astype(np.float64), d[:, :3].astype(np.float64)
    for i in np.nonzero(hits["object"] >= 0)[0]:
        c, h = boxes[int(hits["object"][i])]
        pad = 0.1 * h + 1e-4 * (np.abs(c) + h)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (c - h - pad - o64[i]) / d64[i], (c + h + pad - o64[i]) / d64[i]
        lo, hi = np.fmax.reduce(np.minimum(t0, t1)), np.fmin.reduce(np.maximum(t0, t1))
        outside[i] = not (hi >= lo)  # the LINE: no t >= 0 restriction
    return {"world": world, "camera": camera, "depth": depth, "o": o, "d": d, "p": p, "keys": keys, "dist": dist, "hits": hits,
            "colours": colours, "rays": n_rays, "shadowed": shadowed, "outside": outside}


@pytest.mark.parametrize("switches", [{"RTC_AMD_SPECIALIZE": "0"}, {"RTC_AMD_SPECIALIZE": "1"}, {"RTC_AMD_SPECIALIZE": "0", "RTC_AMD_BVH": "0"}],
                         ids=["aot", "scene_compiled", "bvh_off"])
@pytest.mark.parametrize("name", ["spheres4", "cloud"])
def test_ray_streams_that_start_far_from_a_flat_bvh_world(name, switches, monkeypatch):
    for key, value in switches.items():
        monkeypatch.setenv(key, value)
    c = _far_case(name)
    far = c["dist"] >= 3000.0
    share = float(c["outside"][far].mean())
    print("%s: %d rays, %d hits by the oracle, %d of them on lines that miss the hit object's padded box (%.1f %% of the rays at D >= 3000)"
          % (name, len(c["dist"]), int((c["hits"]["object"] >= 0).sum()), int(c["outside"].sum()), 100.0 * share))
    assert share >= 0.01, share
    r = Renderer(c["world"], c["camera"], device=0)
    try:
        assert ("bvh" in r.kernel_name) == ("RTC_AMD_BVH" not in switches), r.kernel_name
        o, d, p, k = _dev(c["o"]), _dev(c["d"]), _dev(c["p"]), _keys_tensor(c["keys"])
        w = "%s %s (%s)" % (name, switches, r.kernel_name)
        got = _host(r.trace_hits(o, d, keys=k, planes=ALL))
        HH.assert_planes_equal(got, c["hits"], w + ": trace_hits")
        got_s = _np(r.is_shadowed(o, p))
        bad = got_s != c["shadowed"]
        assert not bad.any(), "%s: is_shadowed differs for %d of %d pairs (first: pair %d)" % (w, int(bad.sum()), bad.size, int(np.argmax(bad)))
        for reorder in (False, True):
            got_c = _np(r.trace(o, d, c["depth"], keys=k, reorder=reorder))
            _colours_equal(got_c, c["colours"], "%s: trace, reorder=%r (%s)" % (w, reorder, r.trace_kernel_name))
            assert r.stats()["rays"] == c["rays"], (w, reorder, r.stats()["rays"], c["rays"])
    finally:
        r.close()
