"""Adaptive supersampling on the device (-m gpu): Renderer.render_adaptive (rtc_ctx_render_adaptive, csrc/rtc_adaptive.h).

By definition (include/rtc.h) the frame is the plain render B with, at every pixel one of whose four neighbours
differs from it by more than the threshold, the supersampled frame's value S instead.  B and S are frames the CPU oracle
renders (the coarse and the fine camera), the mask and the composition are tests/adaptive_helpers.py, the k x k reduction is
tests/supersample_helpers.box_filter: every comparison here is bit-exact (helpers.assert_images_equal).

Wall time of this module on an MI355X: see DESIGN.md 8e."""
import os

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests.adaptive_helpers import compose, edge_mask
from tests.supersample_helpers import box_filter

pytestmark = pytest.mark.gpu
f32 = np.float32
THREADS = min(16, len(os.sched_getaffinity(0)))
SWITCHES = ("RTC_AMD_SPECIALIZE", "RTC_AMD_BLOCK_FEEDBACK", "RTC_AMD_SHARE_LOG2", "RTC_AMD_BLOCK_LIST")
THRESHOLD = 0.1


@pytest.fixture
def env():
    """Sets / restores the library's switches (read when a context is created)."""
    saved = {k: os.environ.get(k) for k in SWITCHES}

    def set_(**kw):
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            os.environ["RTC_AMD_" + k] = str(v)
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _adaptive(r, depth, k, threshold, mask=True):
    res = r.render_adaptive(depth, k=k, threshold=threshold, mask=mask)
    torch.cuda.synchronize()
    if mask is None:
        return res.cpu().numpy()
    return res[0].cpu().numpy(), res[1].cpu().numpy()


def _plain(r, depth):
    out = r.render(depth)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# the oracle's frames, rendered once per module and left unchanged: (case, depth, k) -> (frame, rays); k = 1 is the base frame
_oracle_frames = {}


def _oracle(key, world, camera, depth, k):
    if (key, depth, k) not in _oracle_frames:
        cam = camera if k == 1 else camera.supersampled(k)
        frame, rays = H.oracle_camera(cam).render(H.oracle_world(world), depth, threads=THREADS)
        frame.setflags(write=False)
        _oracle_frames[key, depth, k] = (frame, rays)
    return _oracle_frames[key, depth, k]


def _expected(key, world, camera, depth, k, threshold):
    """-> (expected frame, expected mask, B, the oracle's ray count of B)"""
    B, rays = _oracle(key, world, camera, depth, 1)
    fine, _ = _oracle(key, world, camera, depth, k)
    assert not np.isnan(B).any() and not np.isnan(fine).any()
    M = edge_mask(B, threshold)
    return compose(B, box_filter(fine, k), M), M, B, rays


# ---------------------------------------------------------------- 1. against the oracle
# the scenes and sizes of test_gpu_supersample.ORACLE_CASES; (factors, scene-compiled kernels too?)
ORACLE_CASES = {
    "C1_like_constant_jitter": (lambda: scenes.soft_shadows(50, 20, jitter=("constant", 0.5)), (2, 4), True),
    "soft_shadows_odd": (lambda: scenes.soft_shadows(45, 31), (2, 4), True),
    "reflect_refract": (lambda: scenes.reflect_refract(75, 41), (2, 4), True),
    "first_textures": (lambda: scenes.first_textures(62, 35), (2,), False),
    "hexagons": (lambda: scenes.hexagons(70, 37), (2,), False),
    "mesh": (lambda: scenes.mesh(53, 39), (2, 4), True),
    "sphere_grid": (lambda: scenes.sphere_grid(64, 48), (2,), True),
}
RUNS = [(name, 0) for name in ORACLE_CASES] + [(name, 1) for name, case in ORACLE_CASES.items() if case[2]]


def _check_against_oracle(name, world, camera, depth, k, threshold, specialise, share=(0.05, 0.95)):
    exp, M, B, base_rays = _expected(name, world, camera, depth, k, threshold)
    # a mask that is empty or full shows nothing
    assert share[0] <= M.mean() <= share[1], (name, threshold, M.mean())
    r = Renderer(world, camera, device=0)
    got, mask = _adaptive(r, depth, k, threshold)
    what = "%s k=%d threshold=%g specialise=%r depth=%d" % (name, k, threshold, specialise, depth)
    assert mask.dtype == np.uint8 and mask.shape == (camera.height, camera.width)
    assert np.array_equal(mask, M.astype(np.uint8)), (what, int(mask.sum()), int(M.sum()))
    H.assert_images_equal(got, exp, what)
    ad = r.adaptive_stats()
    assert ad["refined_pixels"] == int(M.sum()), what
    assert 0 < ad["rays"] and ad["culled_shadow_rays"] <= ad["rays"] and 0 < ad["shaded_hits"] <= ad["rays"]
    # which refinement kernel ran
    if specialise or depth > 8:
        assert r.adaptive_kernel_name.startswith("adaptive_refine_kernel_spec["), r.adaptive_kernel_name
        assert r.adaptive_kernel_id.startswith("spec_"), r.adaptive_kernel_id
    else:
        assert r.adaptive_kernel_name.startswith("adaptive_refine_kernel<"), r.adaptive_kernel_name
        assert r.adaptive_kernel_id.startswith("aot_adaptive%d_" % k), r.adaptive_kernel_id
    assert r.adaptive_kernel_name.endswith(";ss=%d%s" % (k, r.adaptive_kernel_name[-1])), r.adaptive_kernel_name
    assert r.adaptive_kernel_id not in (r.kernel_id, r.trace_kernel_id)
    # rtc_ctx_stats reports the base pass as after a render
    st = r.stats()
    assert st["rays"] == base_rays and st["pixels"] == (camera.width - 1) * (camera.height - 1) and st["rows"] == camera.height, what
    r.close()


@pytest.mark.parametrize("name,specialise", RUNS)
def test_against_the_oracle(name, specialise, env):
    make, ks, _ = ORACLE_CASES[name]
    world, camera, depth = make()
    for k in ks:
        env(SPECIALIZE=specialise)
        _check_against_oracle(name, world, camera, depth, k, THRESHOLD, specialise)


# ---------------------------------------------------------------- 2. limits
def test_a_threshold_nothing_exceeds_gives_the_plain_render(env):
    env()
    world, camera, depth = scenes.soft_shadows(45, 31)
    r = Renderer(world, camera, device=0)
    plain = _plain(r, depth)
    for k in (2, 4):
        got, mask = _adaptive(r, depth, k, 10.0)
        H.assert_images_equal(got, plain, "threshold 10, k=%d" % k)
        assert not mask.any()
        ad = r.adaptive_stats()
        assert (ad["refined_pixels"], ad["rays"], ad["shaded_hits"], ad["culled_shadow_rays"]) == (0, 0, 0, 0)  # no step taken
    H.assert_images_equal(plain, _oracle("soft_shadows_odd", world, camera, depth, 1)[0], "the base frame is the oracle's")
    r.close()


@pytest.mark.parametrize("specialise", [0, 1])
def test_threshold_zero_refines_wherever_neighbours_differ_at_all(specialise, env):
    env(SPECIALIZE=specialise)
    world, camera, depth = scenes.soft_shadows(45, 31)
    _check_against_oracle("soft_shadows_odd", world, camera, depth, 2, 0.0, specialise)  # (the oracle's mask flags 74 % here)


# ---------------------------------------------------------------- 3. against the library's own parts, at size
def _torch_mask(B, threshold):
    """Rule 2 of the contract on the device: f32 subtraction, abs, a strict compare; both pixels of a pair."""
    t = torch.tensor(threshold, dtype=torch.float32, device=B.device)
    M = torch.zeros(B.shape[:2], dtype=torch.bool, device=B.device)
    dx = ((B[:, 1:] - B[:, :-1]).abs() > t).any(dim=2)
    dy = ((B[1:] - B[:-1]).abs() > t).any(dim=2)
    M[:, :-1] |= dx
    M[:, 1:] |= dx
    M[:-1] |= dy
    M[1:] |= dy
    return M


def _composed(r, camera, depth, k, threshold):
    """render -> mask -> the fine camera's rays of the flagged pixels -> trace with the fine pixels' keys -> box_filter's order
    -> scatter: the adaptive frame from calls that existed before it.  -> (frame, mask, the trace's stats)"""
    B = r.render(depth)
    M = _torch_mask(B, threshold)
    fine_cam = camera.supersampled(k)
    fw, fh = fine_cam.width, fine_cam.height
    origins, directions, keys = r.camera_rays(fine_cam)
    ys, xs = M.nonzero(as_tuple=True)  # (n,)
    sub = torch.arange(k, device=B.device)
    fy = (ys[:, None, None] * k + sub[None, :, None]).expand(-1, k, k)  # (n, sy, sx)
    fx = (xs[:, None, None] * k + sub[None, None, :]).expand(-1, k, k)
    traced = (fx < fw - 1) & (fy < fh - 1)  # the fine frame's last row and column are black
    idx = (fy * fw + fx)[traced]
    cols = r.trace(origins[idx].contiguous(), directions[idx].contiguous(), depth, keys=keys[idx].contiguous())
    st = r.stats()
    v = torch.zeros(fy.shape + (3,), dtype=torch.float32, device=B.device)
    v[traced] = cols
    # DESIGN.md 8b item (3), box_filter's order: along x first, then along y
    if k == 2:
        rows = v[:, :, 0] + v[:, :, 1]
        S = (rows[:, 0] + rows[:, 1]) * 0.25
    else:
        rows = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
        S = ((rows[:, 0] + rows[:, 1]) + (rows[:, 2] + rows[:, 3])) * 0.0625
    out = B.clone()
    out[ys, xs] = S
    torch.cuda.synchronize()
    return out.cpu().numpy(), M.cpu().numpy(), st


def test_against_the_librarys_own_parts_at_size(env):
    env()
    k = 2
    world, camera, depth = scenes.soft_shadows(512, 384)
    r = Renderer(world, camera, device=0)
    exp, M, trace_stats = _composed(r, camera, depth, k, THRESHOLD)
    # enough flagged pixels that many waves take a step (1000 pixels are 4000 lane slots, 63 steps of 64), and unflagged ones left
    assert 1000 <= M.sum() <= M.size - 1000, M.sum()
    for frame in range(3):  # the first frame, and the frames whose base pass is scheduled by what the frames before measured
        got, mask = _adaptive(r, depth, k, THRESHOLD)
        assert np.array_equal(mask.astype(bool), M), frame
        H.assert_images_equal(got, exp, "soft_shadows 512 x 384 k=2 frame %d" % frame)
        ad = r.adaptive_stats()
        assert ad["refined_pixels"] == int(M.sum())
        assert ad["rays"] == trace_stats["rays"] and ad["shaded_hits"] == trace_stats["shaded_hits"], (frame, ad, trace_stats)
        assert ad["culled_shadow_rays"] <= ad["rays"]  # (voted by whichever lanes share a wave)
        assert ad["mask_ms"] > 0.0 and ad["refine_ms"] > 0.0
    # the specialisation policy is asked with the frame's pixels, as the base pass asks it: both scene-compiled or both ahead-of-time
    assert r.adaptive_kernel_name.startswith("adaptive_refine_kernel_spec[") == r.kernel_name.startswith("render_kernel_spec["), (r.adaptive_kernel_name, r.kernel_name)
    r.close()


# ---------------------------------------------------------------- 4. independence of order and state
def test_state_before_and_after(env):
    env()
    world, camera, depth = scenes.reflect_refract(96, 56)
    r = Renderer(world, camera, device=0)
    before = _plain(r, depth)
    before_stats, before_name, before_id = r.stats(), r.kernel_name, r.kernel_id
    first, mask1 = _adaptive(r, depth, 2, THRESHOLD)
    assert 0 < mask1.sum() < mask1.size
    again, mask2 = _adaptive(r, depth, 2, THRESHOLD)  # (the list's order is whatever the waves' atomics made it, twice)
    H.assert_images_equal(again, first, "the same call twice")
    assert np.array_equal(mask1, mask2)
    # unflagged pixels are the plain render's, flagged ones are not all
    assert np.array_equal(first[mask1 == 0], before[mask1 == 0]) and not np.array_equal(first[mask1 == 1], before[mask1 == 1])
    # a plain render after it is the plain render before it, reported and named as before
    H.assert_images_equal(_plain(r, depth), before, "plain render after an adaptive one")
    st = r.stats()
    assert (st["rays"], st["shaded_hits"], st["pixels"], st["rows"]) == tuple(before_stats[key] for key in ("rays", "shaded_hits", "pixels", "rows"))
    assert (r.kernel_name, r.kernel_id) == (before_name, before_id)
    # after a trace: the trace's stats are the trace's until the adaptive call's base pass renders
    origins, directions, keys = r.camera_rays()
    r.trace(origins, directions, depth, keys=keys)
    assert r.stats()["pixels"] == camera.width * camera.height
    trace_name = r.trace_kernel_name
    H.assert_images_equal(_adaptive(r, depth, 2, THRESHOLD, mask=None), first, "after a trace, without a mask")
    assert r.stats()["pixels"] == (camera.width - 1) * (camera.height - 1) and r.trace_kernel_name == trace_name
    # k = 4 on the same context, then 2 again
    four, mask4 = _adaptive(r, depth, 4, THRESHOLD)
    assert np.array_equal(mask4, mask1) and not np.array_equal(four, first)
    assert ";ss=4" in r.adaptive_kernel_name
    H.assert_images_equal(_adaptive(r, depth, 2, THRESHOLD, mask=None), first, "k = 2 after k = 4")
    # into caller tensors
    out, mask = r.alloc(), torch.full((camera.height, camera.width), 7, dtype=torch.uint8, device=r.device)
    res = r.render_adaptive(depth, out=out, mask=mask)
    torch.cuda.synchronize()
    assert res[0] is out and res[1] is mask and np.array_equal(mask.cpu().numpy(), mask1)
    H.assert_images_equal(out.cpu().numpy(), first, "caller tensors, default k and threshold")
    r.close()


def test_after_set_camera(env):
    env()
    world, camera, depth = scenes.reflect_refract(96, 56)
    other = P.Camera(88, 60, camera.field_of_view, P.view_transform(P.point(-2.0, 2.0, -4.5), P.point(-0.6, 1, -0.8), P.vector(0, 1, 0)))
    r = Renderer(world, camera, device=0)
    _adaptive(r, depth, 2, THRESHOLD)
    r.set_camera(other)
    assert r.adaptive_kernel_name == ""  # (of the current scene)
    got, mask = _adaptive(r, depth, 2, THRESHOLD)
    assert got.shape == (60, 88, 3) and mask.shape == (60, 88)
    r.close()
    fresh = Renderer(world, other, device=0)
    B = _plain(fresh, depth)
    fresh.close()
    ss = Renderer(world, other, device=0, supersample=2)
    S = _plain(ss, depth)
    ss.close()
    M = edge_mask(B, THRESHOLD)
    assert np.array_equal(mask.astype(bool), M) and 0.05 < M.mean() < 0.95
    H.assert_images_equal(got, compose(B, S, M), "after set_camera")


def test_refusals_that_need_a_context(env):
    env()
    world, camera, depth = scenes.first_scene(64, 48)
    r = Renderer(world, camera, device=0, supersample=2)
    with pytest.raises(P.RtcError) as e:
        r.render_adaptive(depth)
    assert e.value.status == L.RTC_ERR_UNSUPPORTED and "supersampled" in str(e.value)
    r.set_scene(world, camera)  # leaves supersampled mode
    exp = _adaptive(r, depth, 2, THRESHOLD, mask=None)
    for bad in (dict(k=3), dict(threshold=-1.0), dict(threshold=float("nan")), dict(depth=-1), dict(depth=256)):
        with pytest.raises(P.RtcError) as e:
            r.render_adaptive(**dict(dict(depth=depth), **bad))
        assert e.value.status == L.RTC_ERR_INVALID_ARG, bad
    H.assert_images_equal(_adaptive(r, depth, 2, THRESHOLD, mask=None), exp, "after refused arguments")
    r.close()
    # a fine frame beyond rtc_camera_supersampled's limits: 4 x 40000 rows are 160000 >= 2^17 (k = 2: 80000, fine -- not rendered here)
    tall = P.Camera(4, 40000, camera.field_of_view, camera.transform)
    r = Renderer(world, tall, device=0)
    with pytest.raises(P.RtcError) as e:
        r.render_adaptive(depth, k=4)
    assert e.value.status == L.RTC_ERR_INVALID_ARG and "2^17 rows" in str(e.value)
    r.close()


# ---------------------------------------------------------------- 5. one deep case
def test_a_deep_frame_takes_the_deep_stack_kernel(env):
    env(SPECIALIZE=1)
    world, camera, _ = scenes.reflect_refract(75, 41)
    _check_against_oracle("reflect_refract", world, camera, 12, 2, THRESHOLD, 1)
