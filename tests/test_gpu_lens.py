"""The thin-lens camera on the device (-m gpu): Renderer(world, camera, supersample=k, lens=lens) -- depth of field sampled inside
the supersampling kernel (rtc_ctx_set_scene_lens, csrc/rtc_lens.h).

By definition a lens frame is the fixed-order box filter of the fine frame whose pixel (x, y) is World::color_at of the ray
rtc_lens_rays gives it, jitter key y * k W + x, last row and column zero (tests/lens_helpers.py::oracle_lens_frame).  So every
comparison here is bit-exact: against the CPU oracle, against the composed path (Renderer.trace of the same rays), and against
itself however it is launched.  The oracle counts rays; shade_hit evaluations are compared with the trace of the same rays.

Sections 1 renders every case of lens_helpers.CASES in two child processes -- RTC_AMD_SPECIALIZE=0, the ahead-of-time lens
kernels, and =1 with an empty cache directory, the scene-compiled one -- once each (a module fixture: the first test that asks
pays for the child's start and, for =1, ten compiles)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import demo, scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests import lens_helpers as LH
from tests.supersample_helpers import assemble_partitions, box_filter

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(r, depth, part=None):
    out = r.render(depth, part=part)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _composed(r, camera, depth, k, lens):
    """The lens frame put together by hand on renderer `r` (any context of the same world): trace of rtc_lens_rays' rays with their
    keys, the last fine row and column zeroed, box filter -> (frame, stats of the trace of the rays a lens frame traces)."""
    o, d = camera.lens_rays(k, lens)
    fw, fh = k * camera.width, k * camera.height
    keys = np.arange(fw * fh, dtype=np.uint32)
    traced = (keys // fw < fh - 1) & (keys % fw < fw - 1)
    col = r.trace(_dev(o[traced]), _dev(d[traced]), depth, keys=_dev(keys[traced].view(np.int32)))
    torch.cuda.synchronize()
    st = r.stats()
    fine = np.zeros((fh * fw, 3), dtype=f32)
    fine[traced] = col.cpu().numpy()
    return box_filter(fine.reshape(fh, fw, 3), k), st


# ---------------------------------------------------------------- 1. against the oracle, both kinds of kernel
_CHILD = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %(root)r)
    import numpy as np
    import torch
    from ray_tracer_challenge_amd.renderer import Renderer
    from tests import lens_helpers as LH
    out, seen = {}, {}
    for name, (make, k, lens, switches) in LH.CASES.items():
        for key, value in switches.items():
            os.environ[key] = value
        world, camera, depth = make()
        plan = world.scene_plan(camera)[1]
        r = Renderer(world, camera, device=0, supersample=k, lens=lens)
        frame = r.render(depth)
        torch.cuda.synchronize()
        out[name] = frame.cpu().numpy()
        seen[name] = {"stats": r.stats(), "kernel_name": r.kernel_name, "kernel_id": r.kernel_id, "jit_status": r.jit_status,
                      "share_log2": int(r._lib.rtc_diag_ctx_share_log2(r._ctx)),
                      "plan": {key: plan["lens%%d_%%s" %% (k, key)] for key in ("family_name", "spec_name", "cache_file", "aot_id")}}
        r.close()
        for key in switches:
            del os.environ[key]
    cache = os.environ["RTC_AMD_JIT_CACHE"]
    seen["files"] = sorted(os.listdir(cache)) if os.path.isdir(cache) else []
    np.savez(sys.argv[1], **out)
    print(json.dumps(seen))
""")


@pytest.fixture(scope="module", params=[0, 1], ids=["ahead_of_time", "scene_compiled"])
def rendered(request, tmp_path_factory):
    """Every case rendered by one child process under RTC_AMD_SPECIALIZE = the parameter -> (mode, frames by case, what it saw)."""
    tmp = tmp_path_factory.mktemp("lens%d" % request.param)
    script, frames, cache = tmp / "render.py", tmp / "frames.npz", tmp / "cache"
    script.write_text(_CHILD % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTC_AMD_")}
    env["RTC_AMD_JIT_CACHE"], env["RTC_AMD_SPECIALIZE"] = str(cache), str(request.param)
    p = subprocess.run([sys.executable, str(script), str(frames)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return request.param, dict(np.load(frames)), json.loads(p.stdout.strip().splitlines()[-1])


_oracle = {}  # case -> the oracle's lens frame, its ray count and the fine frame: computed once, compared with both children


def _oracle_of(name):
    name = LH.SAME_FRAME.get(name, name)
    if name not in _oracle:
        make, k, lens, _ = LH.CASES[name]
        world, camera, depth = make()
        _oracle[name] = LH.oracle_lens_frame(H.oracle_world(world), camera, depth, k, lens)
    return _oracle[name]


@pytest.mark.parametrize("name", list(LH.CASES))
def test_against_the_oracle(name, rendered):
    mode, frames, seen = rendered
    make, k, lens, switches = LH.CASES[name]
    world, camera, depth = make()
    exp, exp_rays, fine = _oracle_of(name)
    got, saw = frames[name], seen[name]
    assert got.shape == exp.shape == (camera.height, camera.width, 3)
    # which kernel ran, and that it is the planned one
    assert saw["jit_status"] == ""
    if mode:
        assert saw["kernel_name"] == saw["plan"]["spec_name"] and saw["kernel_name"].startswith("lens_render_kernel_spec[") and saw["kernel_name"].endswith(";ss=%d;lens]" % k)
        assert saw["kernel_id"].partition(".")[0] + ".hsaco" == saw["plan"]["cache_file"] and saw["plan"]["cache_file"] in seen["files"]
    else:
        assert saw["kernel_name"] == saw["plan"]["family_name"] and saw["kernel_name"].startswith("lens_render_kernel<") and saw["kernel_name"].endswith(";ss=%d>" % k)
        assert saw["kernel_id"] == saw["plan"]["aot_id"] and saw["kernel_id"].startswith("aot_lens%d_" % k)
        assert seen["files"] == []
    if "RTC_AMD_SHARE_LOG2" in switches:
        assert saw["share_log2"] == int(switches["RTC_AMD_SHARE_LOG2"])
    H.assert_images_equal(got, exp, "%s specialise=%d" % (name, mode))
    st = saw["stats"]
    assert st["rays"] == exp_rays, (name, mode, st["rays"], exp_rays)
    assert st["pixels"] == (k * camera.width - 1) * (k * camera.height - 1) and st["rows"] == camera.height
    assert not fine[-1].any() and not fine[:, -1].any() and fine.any()
    # shade_hit evaluations: those of the same rays as a stream (the oracle counts rays only)
    plain = Renderer(world, camera, device=0)
    composed, trace_stats = _composed(plain, camera, depth, k, lens)
    plain.close()
    H.assert_images_equal(composed, exp, "%s composed" % name)
    assert (st["rays"], st["shaded_hits"]) == (trace_stats["rays"], trace_stats["shaded_hits"])


def test_lane_sharing_is_reached_and_switched_off():
    """soft_shadows 20 x 16 under its area light: the scene's own kernel shares lanes (the planning code's choice), and
    RTC_AMD_SHARE_LOG2=0 is the same frame with one lane per pixel -- test_against_the_oracle compares both with one oracle frame."""
    os.environ["RTC_AMD_SPECIALIZE"] = "1"
    try:
        make, k, lens, _ = LH.CASES["soft_shadows_k2"]
        world, camera, depth = make()
        r = Renderer(world, camera, device=0, supersample=k, lens=lens)
        _frame(r, depth)
        assert r._lib.rtc_diag_ctx_share_log2(r._ctx) > 0
        r.close()
    finally:
        del os.environ["RTC_AMD_SPECIALIZE"]


def test_lens_origins_inside_the_glass_sphere_and_outside_the_cull_ball():
    """What two of the cases are there for, asserted on the host: some o' lies inside reflect_refract's glass sphere, and some o' of the
    far mesh camera lies outside the ball triangle pre-culling is argued for (rtc_diag_scene_plan's tri_cull line: has_tbox, centre, r^2)."""
    make, k, lens, _ = LH.CASES["reflect_refract_inside_the_glass"]
    _, camera, _ = make()
    o, _ = camera.lens_rays(k, lens)
    inside = np.linalg.norm(o[:, :3].astype(np.float64) - LH.GLASS_CENTRE, axis=1) < LH.GLASS_RADIUS
    assert inside.sum() >= 10, int(inside.sum())
    for name, some_outside in (("golden_mesh", False), ("golden_mesh_outside_the_cull_ball", True)):
        make, k, lens, _ = LH.CASES[name]
        world, camera, _ = make()
        cull = world.scene_plan(camera.supersampled(k))[1]["tri_cull"].split()
        assert int(cull[0]) == 1  # the triangles carry pre-culling boxes
        centre, r2 = np.array([float(v) for v in cull[1:4]]), float(cull[4])
        o, _ = camera.lens_rays(k, lens)
        outside = ((o[:, :3].astype(np.float64) - centre) ** 2).sum(axis=1) > r2
        assert (outside.sum() >= 10) == some_outside, (name, int(outside.sum()))


# ---------------------------------------------------------------- 2. partitions
def test_partitions_count_output_rows():
    make, k, lens, _ = LH.CASES["sphere_grid_k2"]
    world, camera, depth = make()
    band_rows, n_parts = 4, 3
    r = Renderer(world, camera, device=0, supersample=k, lens=lens)
    whole = _frame(r, depth)
    whole_stats = r.stats()
    parts, rays, pixels, rows = [], 0, 0, 0
    for p in range(n_parts):
        part = r.partition(band_rows, n_parts, p)
        buf = _frame(r, depth, part=part)
        assert buf.shape == (r.rows(part), camera.width, 3)
        parts.append(buf)
        st = r.stats()
        rays, pixels, rows = rays + st["rays"], pixels + st["pixels"], rows + st["rows"]
    r.close()
    H.assert_images_equal(assemble_partitions(parts, camera.height, band_rows, n_parts), whole, "bands of 4 output rows over 3 parts")
    assert (rays, pixels, rows) == (whole_stats["rays"], whole_stats["pixels"], camera.height)
    H.assert_images_equal(whole, _oracle_of("sphere_grid_k2")[0], "the whole frame")


# ---------------------------------------------------------------- 3. against the composed path, at a size the oracle is not asked for
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", ["soft_shadows", "reflect_refract"])
def test_against_the_composed_path(name, k):
    world, camera, depth = getattr(scenes, name)(128, 80)
    lens = P.Lens(0.2, 4.5, seed=9)
    r = Renderer(world, camera, device=0, supersample=k, lens=lens)
    for frame in range(3):  # the first frame, and the frames scheduled by what the frames before measured
        got = _frame(r, depth)
        st = r.stats()
        if frame == 0:
            exp, trace_stats = _composed(r, camera, depth, k, lens)  # (a lens context traces like any other)
        H.assert_images_equal(got, exp, "%s k=%d frame %d" % (name, k, frame))
        assert (st["rays"], st["shaded_hits"]) == (trace_stats["rays"], trace_stats["shaded_hits"])
        assert st["pixels"] == (k * 128 - 1) * (k * 80 - 1) == trace_stats["pixels"]
    r.close()


# ---------------------------------------------------------------- 4. state
def test_a_focus_pull_uploads_nothing_and_set_camera_keeps_the_lens():
    world, camera, depth = scenes.reflect_refract(96, 56)
    near, far = P.Lens(0.25, 3.0, seed=1), P.Lens(0.25, 9.0, seed=1)
    r = Renderer(world, camera, device=0, supersample=2, lens=near)
    a = _frame(r, depth)
    name, kid = r.kernel_name, r.kernel_id
    assert name.startswith("lens_render_kernel")
    r.set_lens(far)
    b = _frame(r, depth)
    assert r.lens is far and (r.kernel_name, r.kernel_id) == (name, kid)
    assert not np.array_equal(a, b)
    fresh = Renderer(world, camera, device=0, supersample=2, lens=far)
    H.assert_images_equal(b, _frame(fresh, depth), "after set_lens against a fresh context")
    # (nothing was planned or compiled again either: the kernel and its id are the ones the first lens got)
    r.set_lens(near)
    H.assert_images_equal(_frame(r, depth), a, "back to the first lens")
    other = P.Camera(88, 60, camera.field_of_view, P.view_transform(P.point(-2.0, 2.0, -4.5), P.point(-0.6, 1, -0.8), P.vector(0, 1, 0)))
    r.set_camera(other)
    assert r.lens is near and r.supersample == 2 and (r.width, r.height) == (88, 60) and r.kernel_name.startswith("lens_render_kernel")
    got = _frame(r, depth)
    fresh.set_scene(world, other, supersample=2, lens=near)
    H.assert_images_equal(got, _frame(fresh, depth), "set_camera under a lens")
    H.assert_images_equal(got, _composed(fresh, other, depth, 2, near)[0], "set_camera under a lens, composed")
    r.close()
    fresh.close()


def test_leaving_lens_mode_gives_the_supersampled_frame_again():
    world, camera, depth = scenes.soft_shadows(64, 40)
    ss = Renderer(world, camera, device=0, supersample=2)
    exp, exp_name, exp_id = _frame(ss, depth), ss.kernel_name, ss.kernel_id
    ss.close()
    r = Renderer(world, camera, device=0, supersample=2, lens=P.Lens(0.2, 3.9))
    through = _frame(r, depth)
    assert r.kernel_name.startswith("lens_") and r.kernel_id != exp_id
    r.set_scene(world, camera, supersample=2)
    assert r.lens is None and (r.kernel_name, r.kernel_id) == (exp_name, exp_id)
    H.assert_images_equal(_frame(r, depth), exp, "supersampled after the lens")
    assert not np.array_equal(through, exp)
    r.set_scene(world, camera, supersample=2, lens=P.Lens(0.2, 3.9))
    H.assert_images_equal(_frame(r, depth), through, "the lens again")
    r.set_scene(world, camera)  # ... and a plain set_scene leaves both modes
    plain = _frame(r, depth)
    assert r.supersample == 1 and r.kernel_name.startswith("render_kernel") and not plain[-1].any()
    r.close()


def test_hits_and_adaptive_are_refused_and_trace_is_untouched():
    world, camera, depth = scenes.first_scene(64, 48)
    plain = Renderer(world, camera, device=0)
    o, d, keys = plain.camera_rays()
    exp = plain.trace(o, d, depth, keys=keys).cpu().numpy()
    r = Renderer(world, camera, device=0, supersample=2, lens=P.Lens(0.1, 5.0))
    for call in (lambda: r.render_hits(planes=("object",)), lambda: r.render_adaptive(depth, k=2, threshold=0.1)):
        with pytest.raises(P.RtcError) as e:
            call()
        assert e.value.status == L.RTC_ERR_UNSUPPORTED and "lens" in str(e.value)
    got = r.trace(o, d, depth, keys=keys).cpu().numpy()
    H.assert_images_equal(got.reshape(1, -1, 3), exp.reshape(1, -1, 3), "trace on a lens context")
    assert r.trace_kernel_name == plain.trace_kernel_name and r.trace_kernel_id == plain.trace_kernel_id
    for bad in (P.Lens(-1.0, 5.0), P.Lens(0.1, 0.0)):  # a refused lens leaves the context as it was
        with pytest.raises(P.RtcError) as e:
            r.set_lens(bad)
        assert e.value.status == L.RTC_ERR_INVALID_ARG
    assert r.lens.aperture_radius == f32(0.1)
    r.close()
    plain.close()


# ---------------------------------------------------------------- 5. the demo
def test_the_demo_prints_the_renderers_frame(tmp_path):
    out = tmp_path / "lens.ppm"
    assert demo.main(["first_scene", "--size", "40x20", "--supersample", "2", "--aperture", "0.2", "--focus", "5.0", "--out", str(out)]) == 0
    world, camera, depth = scenes.first_scene(40, 20)
    r = Renderer(world, camera, device=0, supersample=2, lens=P.Lens(0.2, 5.0))
    frame = r.render(depth)
    assert out.read_bytes() == r.to_ppm(frame) + b"\n"
    r.close()
    with pytest.raises(SystemExit):
        demo.main(["first_scene", "--aperture", "0.2", "--focus", "5.0"])  # no lens without supersampling
    with pytest.raises(SystemExit):
        demo.main(["first_scene", "--supersample", "2", "--aperture", "0.2"])
