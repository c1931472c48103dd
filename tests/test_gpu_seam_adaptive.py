"""rtc_render_adaptive on the device (-m gpu): adaptive supersampling through the one-call seam (csrc/rtc_adaptive_seam.h).

By definition (include/rtc.h) the frame is rtc_ctx_render_adaptive's whatever the split: the plain frame B with, at every
pixel one of whose four neighbours IN THE WHOLE FRAME differs from it by more than the threshold, the supersampled frame's value
instead.  B and the fine frame are the CPU oracle's, the mask and the composition tests/adaptive_helpers.py, the k x k reduction
tests/supersample_helpers.box_filter; every comparison is bit-exact.  The cases are chosen so that a mask computed band by band without
halo rows is wrong: each has, at band_rows 7 and 1, a flagged pixel whose only contrasting neighbour lies across a band edge that
another entry owns (checked on the CPU, with the oracle's frame, before anything is rendered).

Wall time of this module on an MI355X: see DESIGN.md 8e."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import demo, scenes
from ray_tracer_challenge_amd.renderer import Renderer
from oracle import oracle as O
from tests import helpers as H
from tests.adaptive_helpers import compose, edge_mask
from tests.supersample_helpers import box_filter

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, len(os.sched_getaffinity(0)))
THRESHOLD = 0.1
# the small sizes of tests/test_gpu_adaptive.ORACLE_CASES: name -> (scene, factors)
CASES = {
    "soft_shadows": (lambda: scenes.soft_shadows(45, 31), (2, 4)),
    "reflect_refract": (lambda: scenes.reflect_refract(75, 41), (2,)),
    "mesh": (lambda: scenes.mesh(53, 39), (2, 4)),
    "sphere_grid": (lambda: scenes.sphere_grid(64, 48), (2,)),
}
SPLITS = [(n, band_rows) for n in (1, 2, 5) for band_rows in (64, 7, 1)]


@pytest.fixture
def env():
    """Sets / restores RTC_AMD_SPECIALIZE (Camera.render drops the seam's contexts when the environment has changed)."""
    saved = os.environ.get("RTC_AMD_SPECIALIZE")

    def set_(specialise=None):
        P.lib().rtc_render_release()  # (contexts read the switch when they are created)
        os.environ.pop("RTC_AMD_SPECIALIZE", None)
        if specialise is not None:
            os.environ["RTC_AMD_SPECIALIZE"] = str(specialise)
    yield set_
    os.environ.pop("RTC_AMD_SPECIALIZE", None)
    if saved is not None:
        os.environ["RTC_AMD_SPECIALIZE"] = saved
    P.lib().rtc_render_release()


# the oracle's frames, rendered once per module and left unchanged
_oracle_frames = {}


def _oracle(name, world, camera, depth, k):
    if (name, depth, k) not in _oracle_frames:
        cam = camera if k == 1 else camera.supersampled(k)
        frame, rays = H.oracle_camera(cam).render(H.oracle_world(world), depth, threads=THREADS)
        frame.setflags(write=False)
        _oracle_frames[name, depth, k] = (frame, rays)
    return _oracle_frames[name, depth, k]


def _expected(name, world, camera, depth, k, threshold):
    """-> (O, M, B, B's rays)"""
    B, rays = _oracle(name, world, camera, depth, 1)
    fine, _ = _oracle(name, world, camera, depth, k)
    M = edge_mask(B, threshold)
    return compose(B, box_filter(fine, k), M), M, B, rays


def _scale(frame):
    """canvas.rs:39-43 per channel, the arithmetic of every u8 canvas here: f32 product, clamp, truncation."""
    return np.maximum(np.minimum(frame.astype(f32) * f32(255.0), f32(255.0)), f32(0.0)).astype(np.uint8)


def _needs_a_halo(B, threshold, band_rows, n_parts):
    """Is there a flagged pixel whose ONLY contrasting neighbour lies across a band edge that another part owns?"""
    if n_parts == 1 or band_rows >= B.shape[0]:
        return False
    t = f32(threshold)
    dx = (np.abs(B[:, 1:] - B[:, :-1]) > t).any(axis=2)
    dy = (np.abs(B[1:] - B[:-1]) > t).any(axis=2)  # row y against y + 1
    crossing = (np.arange(1, B.shape[0]) % band_rows) == 0  # y + 1 starts a band
    inside = np.zeros(B.shape[:2], dtype=bool)
    inside[:, :-1] |= dx
    inside[:, 1:] |= dx
    own = dy & ~crossing[:, None]
    inside[:-1] |= own
    inside[1:] |= own
    return bool((edge_mask(B, threshold) & ~inside).any())


def _halo_rows(height, band_rows, n_parts):
    """Halo rows of all parts together, by the library's host-only plan (tests/test_seam_adaptive_boundary.py restates it)."""
    total = 0
    for part in range(n_parts):
        counts = (C.c_uint32 * 2)()
        assert P.lib().rtc_diag_adaptive_bands(height, band_rows, n_parts, part, None, 0, None, 0, counts) == 1
        total += counts[1]
    return total


def _call(world, camera, depth, k, threshold, devices=(0,), band_rows=0, quantize=0, on_device=0, out=None, mask=None):
    """The ctypes call -> (frame, mask, rtc_stats, rtc_seam_adaptive_stats); out / mask: raw addresses, or None for fresh pageable arrays."""
    cs = world._c()
    arr = (C.c_int32 * len(devices))(*devices)
    opts = L.rtc_opts(arr, len(devices), band_rows, quantize, on_device)
    frame = m = None
    if out is None:
        frame = np.full((camera.height, camera.width, 3), 7, dtype=np.uint8 if quantize else f32)
        m = np.full((camera.height, camera.width), 9, dtype=np.uint8)
        out, mask = frame.ctypes.data, m.ctypes.data
    st, ad = L.rtc_stats(), L.rtc_seam_adaptive_stats()
    L.check(P.lib().rtc_render_adaptive(C.byref(cs.scene), C.byref(camera._cam), depth, k, f32(threshold), C.byref(opts), C.c_void_p(out),
                                        C.c_void_p(mask) if mask else None, C.byref(st), C.byref(ad)))
    return frame, m, st, ad


def _seam_kernels(entry=0):
    lib = P.lib()
    ctx = lib.rtc_diag_seam_ctx(entry)
    return [lib.rtc_diag_ctx_adaptive_seam_kernel(ctx, what).decode() for what in range(4)]


# ---------------------------------------------------------------- 1. against the oracle, over the splits
@pytest.mark.parametrize("name,k", [(name, k) for name, case in CASES.items() for k in case[1]])
def test_every_split_gives_the_whole_frames_picture(name, k, env):
    env(0)  # (the matrix runs the ahead-of-time kernels; the scene-compiled ones: below)
    world, camera, depth = CASES[name][0]()
    exp, M, B, base_rays = _expected(name, world, camera, depth, k, THRESHOLD)
    assert 0.05 <= M.mean() <= 0.95, (name, M.mean())
    for n in (2, 5):
        for band_rows in (7, 1):
            assert _needs_a_halo(B, THRESHOLD, band_rows, n), (name, n, band_rows)
    ex = L.rtc_stats()
    plain = np.zeros((camera.height, camera.width, 3), dtype=f32)
    L.check(P.lib().rtc_render_ex(C.byref(world._c().scene), C.byref(camera._cam), depth, None, plain.ctypes.data_as(C.c_void_p), C.byref(ex)))
    assert ex.rays == base_rays
    exp_u8 = _scale(exp)
    for n, band_rows in SPLITS:
        for quantize in (0, 1):
            what = "%s k=%d entries=%d band_rows=%d quantize=%d" % (name, k, n, band_rows, quantize)
            got, mask, st, ad = _call(world, camera, depth, k, THRESHOLD, [0] * n, band_rows, quantize)
            assert np.array_equal(mask, M.astype(np.uint8)), (what, int(mask.sum()), int(M.sum()))
            if quantize:
                assert np.array_equal(got, exp_u8), what
            else:
                H.assert_images_equal(got, exp, what)
            assert ad.refined_pixels == int(M.sum()), what
            assert (st.rays, st.shaded_hits, st.pixels, st.rows) == (base_rays, ex.shaded_hits, ex.pixels, camera.height), what
            assert ad.halo_pixels == _halo_rows(camera.height, band_rows, n) * camera.width, what
            assert (ad.halo_pixels == 0) == (n == 1 or band_rows >= camera.height) and (ad.halo_rays > 0) == (ad.halo_pixels > 0), what
            assert 0 < ad.refine_rays, what
            names = _seam_kernels()
            assert names[0].startswith("adaptive_seam_kernel<") and names[0].endswith(";ss=%d>" % k) and names[1].startswith("aot_adaptive_seam%d_" % k), names
            if ad.halo_pixels:
                assert names[2].startswith("adaptive_seam_kernel<") and names[2].endswith(";halo>") and names[3].startswith("aot_adaptive_seam1_"), names
            else:
                assert names[2:] == ["", ""], names


def test_a_band_edge_at_the_last_row(env):
    """soft_shadows 45 x 31 at band_rows 5: the last band is the single row 30 -- the frame's black last row is a halo row of the part
    that owns rows 25 .. 29, and the row 29 a halo row of the part that owns the last."""
    env(0)
    world, camera, depth = CASES["soft_shadows"][0]()
    exp, M, B, base_rays = _expected("soft_shadows", world, camera, depth, 2, THRESHOLD)
    assert camera.height == 31 and not B[30].any() and M[29].any()
    for n in (2, 3):
        halo = (C.c_uint32 * 64)()
        counts = (C.c_uint32 * 2)()
        assert P.lib().rtc_diag_adaptive_bands(31, 5, n, 5 % n, None, 0, halo, 64, counts) == 1 and 30 in list(halo[:counts[1]])
        for quantize in (0, 1):
            got, mask, st, ad = _call(world, camera, depth, 2, THRESHOLD, [0] * n, 5, quantize)
            assert np.array_equal(mask, M.astype(np.uint8)) and ad.refined_pixels == int(M.sum())
            assert np.array_equal(got, _scale(exp)) if quantize else np.array_equal(got.view(np.uint32), exp.view(np.uint32))
            assert st.rays == base_rays


# ---------------------------------------------------------------- 2. thresholds
def test_thresholds(env):
    env(0)
    world, camera, depth = CASES["reflect_refract"][0]()
    _, _, B, base_rays = _expected("reflect_refract", world, camera, depth, 2, THRESHOLD)
    plain = np.zeros((camera.height, camera.width, 3), dtype=f32)
    L.check(P.lib().rtc_render_ex(C.byref(world._c().scene), C.byref(camera._cam), depth, None, plain.ctypes.data_as(C.c_void_p), None))
    for n, band_rows in ((1, 64), (2, 7), (5, 1)):
        got, mask, st, ad = _call(world, camera, depth, 2, 1e30, [0] * n, band_rows)  # nothing exceeds it
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)) and not mask.any()
        assert ad.refined_pixels == 0 and ad.refine_rays == 0 and st.rays == base_rays
        exp, M, _, _ = _expected("reflect_refract", world, camera, depth, 2, 0.0)
        got, mask, st, ad = _call(world, camera, depth, 2, 0.0, [0] * n, band_rows)
        assert np.array_equal(mask, M.astype(np.uint8)) and ad.refined_pixels == int(M.sum())
        H.assert_images_equal(got, exp, "threshold 0, %d entries" % n)


# ---------------------------------------------------------------- 3. which kernels run (child processes, an empty cache)
_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L, scenes
world, camera, depth = scenes.soft_shadows(45, 31)
lib = P.lib()
seen = []
for call in range(2):
    mask = np.zeros((31, 45), dtype=np.uint8)
    img = camera.render(world, depth, devices=[0, 0], band_rows=7, supersample=2, adaptive=0.1, mask=mask)
    ctx = lib.rtc_diag_seam_ctx(1)
    seen.append({"names": [lib.rtc_diag_ctx_adaptive_seam_kernel(ctx, w).decode() for w in range(4)], "base": lib.rtc_ctx_kernel_name(ctx).decode(),
                 "refined": camera.last_adaptive_stats["refined_pixels"], "rays": camera.last_stats["rays"]})
    np.save(sys.argv[1] + "/frame%d.npy" % call, img.data)
    np.save(sys.argv[1] + "/mask%d.npy" % call, mask)
print(json.dumps(seen))
"""


@pytest.mark.parametrize("specialise", ["0", "1"])
def test_ahead_of_time_and_scene_compiled_kernels(specialise, tmp_path):
    env = dict(os.environ, RTC_AMD_SPECIALIZE=specialise, RTC_AMD_JIT_CACHE=str(tmp_path / "cache"), PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    seen = json.loads(p.stdout.strip().splitlines()[-1])
    world, camera, depth = CASES["soft_shadows"][0]()
    exp, M, _, base_rays = _expected("soft_shadows", world, camera, depth, 2, THRESHOLD)
    for call, s in enumerate(seen):
        H.assert_images_equal(np.load(tmp_path / ("frame%d.npy" % call)), exp, "specialise=%s call %d" % (specialise, call))
        assert np.array_equal(np.load(tmp_path / ("mask%d.npy" % call)), M.astype(np.uint8))
        assert s["refined"] == int(M.sum()) and s["rays"] == base_rays
        if specialise == "1":
            assert s["names"][0].startswith("adaptive_seam_kernel_spec[") and s["names"][0].endswith(";ss=2]") and s["names"][1].startswith("spec_"), s
            assert s["names"][2].startswith("adaptive_seam_kernel_spec[") and s["names"][2].endswith(";halo]") and s["names"][3].startswith("spec_"), s
            assert len({s["names"][1], s["names"][3]}) == 2 and s["base"].startswith("render_kernel_spec["), s
        else:
            assert s["names"][0].startswith("adaptive_seam_kernel<") and s["names"][1].startswith("aot_adaptive_seam2_"), s
            assert s["names"][2].endswith(";halo>") and s["names"][3].startswith("aot_adaptive_seam1_") and s["base"].startswith("render_kernel<"), s


def test_depth_12_takes_the_deep_stack_kernels(env):
    env()
    world, camera, _ = CASES["reflect_refract"][0]()
    exp, M, _, base_rays = _expected("reflect_refract", world, camera, 12, 2, THRESHOLD)
    got, mask, st, ad = _call(world, camera, 12, 2, THRESHOLD, [0, 0], 7)
    assert np.array_equal(mask, M.astype(np.uint8)) and st.rays == base_rays
    H.assert_images_equal(got, exp, "depth 12")
    names = _seam_kernels()
    assert names[0].startswith("adaptive_seam_kernel_spec[") and names[1].startswith("spec_") and names[3].startswith("spec_"), names


# ---------------------------------------------------------------- 4. where the frame and the mask go
def test_device_pageable_and_page_locked_output(env):
    env(0)
    world, camera, depth = CASES["sphere_grid"][0]()
    W, Hh = camera.width, camera.height
    exp, M, _, base_rays = _expected("sphere_grid", world, camera, depth, 2, THRESHOLD)
    lib = P.lib()
    pinned, pinned_mask = lib.rtc_host_alloc(W * Hh * 12), lib.rtc_host_alloc(W * Hh)
    assert pinned and pinned_mask
    try:
        for devices in ([0], [0, 0, 0]):
            for quantize in (0, 1):
                want = _scale(exp) if quantize else exp.view(np.uint32)
                t = torch.full((Hh, W, 3), 7, dtype=torch.uint8 if quantize else torch.float32, device="cuda:0")
                tm = torch.full((Hh, W), 7, dtype=torch.uint8, device="cuda:0")
                _, _, st, ad = _call(world, camera, depth, 2, THRESHOLD, devices, 7, quantize, 1, t.data_ptr(), tm.data_ptr())
                got = t.cpu().numpy()
                assert np.array_equal(got if quantize else got.view(np.uint32), want) and np.array_equal(tm.cpu().numpy(), M.astype(np.uint8)), (devices, quantize)
                assert st.rays == base_rays and ad.refined_pixels == int(M.sum())
                C.memset(pinned, 0xAB, W * Hh * 12)
                C.memset(pinned_mask, 0xAB, W * Hh)
                _, _, st, ad = _call(world, camera, depth, 2, THRESHOLD, devices, 7, quantize, 0, pinned, pinned_mask)
                view = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8 if quantize else C.c_uint32)), shape=(W * Hh * 3,)).reshape(Hh, W, 3)
                assert np.array_equal(view, want), (devices, quantize, "page-locked")
                assert np.array_equal(np.ctypeslib.as_array(C.cast(pinned_mask, C.POINTER(C.c_uint8)), shape=(Hh * W,)).reshape(Hh, W), M.astype(np.uint8))
                got, mask, st, ad = _call(world, camera, depth, 2, THRESHOLD, devices, 7, quantize)  # pageable
                assert np.array_equal(got if quantize else got.view(np.uint32), want) and np.array_equal(mask, M.astype(np.uint8))
                # no mask asked for: the frame is the same
                frame = np.zeros((Hh, W, 3), dtype=np.uint8 if quantize else f32)
                _call(world, camera, depth, 2, THRESHOLD, devices, 7, quantize, 0, frame.ctypes.data, None)
                assert np.array_equal(frame if quantize else frame.view(np.uint32), want)
    finally:
        lib.rtc_host_free(pinned)
        lib.rtc_host_free(pinned_mask)
        lib.rtc_render_release()


# ---------------------------------------------------------------- 5. the seam's state
def test_the_four_seam_calls_alternate_on_one_scene(env):
    env(0)
    world, camera, depth = CASES["sphere_grid"][0]()
    exp, M, B, base_rays = _expected("sphere_grid", world, camera, depth, 2, THRESHOLD)
    fine, fine_rays = _oracle("sphere_grid", world, camera, depth, 2)
    lens = P.Lens(0.3, 6.0, seed=3)
    r = Renderer(world, camera, device=0, supersample=2, lens=lens)
    lens_frame = r.render(depth)
    torch.cuda.synchronize()
    lens_frame = lens_frame.cpu().numpy()
    r.close()
    for again in range(2):
        H.assert_images_equal(camera.render(world, depth).data, B, "rtc_render_ex in the sequence")
        H.assert_images_equal(camera.render(world, depth, supersample=2, adaptive=THRESHOLD, devices=[0, 0], band_rows=7).data, exp, "adaptive")
        assert camera.last_stats["rays"] == base_rays and camera.last_adaptive_stats["refined_pixels"] == int(M.sum())
        H.assert_images_equal(camera.render(world, depth, supersample=2).data, box_filter(fine, 2), "rtc_render_ss in the sequence")
        assert camera.last_stats["rays"] == fine_rays and camera.last_adaptive_stats is None
        H.assert_images_equal(camera.render(world, depth, supersample=2, adaptive=THRESHOLD).data, exp, "adaptive after ss")
        H.assert_images_equal(camera.render(world, depth, supersample=2, lens=lens).data, lens_frame, "rtc_render_lens in the sequence")
        assert np.array_equal(camera.render(world, depth, supersample=2, adaptive=THRESHOLD, quantize=True), _scale(exp))
        P.lib().rtc_render_release()


# ---------------------------------------------------------------- 6. the Python and C++ surfaces, the demo
def test_python_surface_is_the_ctypes_call(env):
    env(0)
    world, camera, depth = CASES["soft_shadows"][0]()
    for quantize in (0, 1):
        raw, raw_mask, st, ad = _call(world, camera, depth, 4, THRESHOLD, [0, 0], 7, quantize)
        mask = np.zeros((camera.height, camera.width), dtype=np.uint8)
        got = camera.render(world, depth, devices=[0, 0], band_rows=7, quantize=bool(quantize), supersample=4, adaptive=THRESHOLD, mask=mask)
        got = got if quantize else got.data
        assert got.dtype == raw.dtype and np.array_equal(got.view(np.uint8), raw.view(np.uint8)) and np.array_equal(mask, raw_mask)
        assert camera.last_stats["rays"] == st.rays and camera.last_stats["pixels"] == st.pixels
        mine = camera.last_adaptive_stats
        assert (mine["refined_pixels"], mine["refine_rays"], mine["halo_pixels"], mine["halo_rays"]) == (ad.refined_pixels, ad.refine_rays, ad.halo_pixels, ad.halo_rays)


def test_cpp_surface_prints_the_oracles_ppm():
    """demos/adaptive.cpp: first_scene through Camera::render_adaptive (include/rtc.hpp)."""
    demos = os.path.join(ROOT, "demos")
    subprocess.check_call(["make", "-C", demos, "-s"], timeout=300)
    exe = os.path.join(demos, "adaptive")
    world, camera, depth = scenes.first_scene(40, 20)
    exp, M, _, _ = _expected("first_scene", world, camera, depth, 2, THRESHOLD)
    p = subprocess.run([exe, "40x20", "2", "0.1"], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stdout == O.to_ppm(exp) + b"\n"
    assert ("refined %d " % int(M.sum())).encode() in p.stderr, p.stderr
    bad = subprocess.run([exe, "40x20", "3", "0.1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "factor 3" in bad.stderr and bad.stdout == "", bad.stderr
    bad = subprocess.run([exe, "40x20", "2", "-1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "threshold" in bad.stderr and bad.stdout == "", bad.stderr


def test_the_demo_goes_through_the_seam_and_writes_the_same_ppm(tmp_path):
    out = tmp_path / "adaptive.ppm"
    assert demo.main(["first_scene", "--size", "40x20", "--supersample", "2", "--adaptive", "0.1", "--out", str(out)]) == 0
    assert _seam_kernels()[0].startswith(("adaptive_seam_kernel<", "adaptive_seam_kernel_spec["))
    world, camera, depth = scenes.first_scene(40, 20)
    exp, _, _, _ = _expected("first_scene", world, camera, depth, 2, THRESHOLD)
    assert out.read_bytes() == O.to_ppm(exp) + b"\n"
    with pytest.raises(SystemExit):
        demo.main(["first_scene", "--size", "40x20", "--adaptive", "0.1", "--out", str(out)])  # no --supersample
    P.lib().rtc_render_release()
