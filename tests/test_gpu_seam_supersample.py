"""Supersampling through the one-call seam (-m gpu): rtc_render_ss / Camera.render(..., supersample=k) / Camera::render_supersampled.

The expected frame is the one rtc_ctx_set_scene_ss defines: box_filter (tests/supersample_helpers.py) of the oracle's render of
camera.supersampled(k); for bytes, O.quantize of that.  f32 frames are compared bit for bit, bytes for equality.  Where a test
is about the transport (rows leaving while later rows render) the expectation is the persistent context's frame,
Renderer(world, camera, supersample=k), which tests/test_gpu_supersample.py ties to the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests.supersample_helpers import box_filter

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, len(os.sched_getaffinity(0)))
SWITCHES = ("RTC_AMD_SPECIALIZE", "RTC_AMD_SHARE_LOG2")


@pytest.fixture
def env():
    """Sets / restores the library's switches; the seam's contexts read them when they are created, so they are dropped."""
    saved = {k: os.environ.get(k) for k in SWITCHES}

    def set_(**kw):
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            os.environ["RTC_AMD_" + k] = str(v)
        P.lib().rtc_render_release()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    P.lib().rtc_render_release()


SCENES = {
    "soft_shadows": lambda: scenes.soft_shadows(100, 66, jitter=("hashed", scenes.DEFAULT_SEED)),  # height no multiple of the bands; lanes share pixels
    "glass_and_mirror": lambda: scenes.glass_and_mirror(49, 32),
    "sphere_grid": lambda: scenes.sphere_grid(128, 150),
    "hexagons": lambda: scenes.hexagons(80, 50),
    "first_scene": lambda: scenes.first_scene(100, 50),
}
_made, _expected = {}, {}


def _scene(name):
    if name not in _made:
        _made[name] = SCENES[name]()
    return _made[name]


def _oracle(key, world, camera, depth, k):
    """(expected f32 frame, its bytes, the fine frame's rays): rendered once per scene and factor, never changed."""
    if (key, k) not in _expected:
        fine, rays = H.oracle_camera(camera.supersampled(k)).render(H.oracle_world(world), depth, threads=THREADS)
        exp = box_filter(fine, k)
        exp.setflags(write=False)
        _expected[key, k] = (exp, O.quantize(exp), rays)
    return _expected[key, k]


def _render_ss(world, camera, depth, k, devices, out_ptr, band_rows=0, quantize=0, on_device=0, entry="rtc_render_ss"):
    """The ctypes call itself -> rtc_stats."""
    lib, cs = P.lib(), world._c()
    arr = (C.c_int32 * len(devices))(*devices)
    opts = L.rtc_opts(arr, len(devices), band_rows, quantize, on_device)
    st = L.rtc_stats()
    if entry == "rtc_render_ss":
        L.check(lib.rtc_render_ss(C.byref(cs.scene), C.byref(camera._cam), depth, k, C.byref(opts), C.c_void_p(out_ptr), C.byref(st)))
    else:
        L.check(lib.rtc_render_ex(C.byref(cs.scene), C.byref(camera._cam), depth, C.byref(opts), C.c_void_p(out_ptr), C.byref(st)))
    return st


def _owners(height, band_rows, n_entries):
    """Entries of opts->devices that own at least one band of output rows: each of them launches once, the others have nothing to
    launch (rtc_stats.launches counts launches, as for rtc_render_ex)."""
    band = band_rows or 64
    return min(n_entries, -(-height // band))


def _progress(entry):
    out = (C.c_uint32 * 2)()
    assert P.lib().rtc_diag_seam_progress(entry, out) == 1
    return bool(out[0]), int(out[1])


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("specialise", [0, 1])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", ["soft_shadows", "glass_and_mirror", "sphere_grid", "hexagons"])
def test_against_the_oracle(name, k, specialise, env):
    world, camera, depth = _scene(name)
    exp, exp_u8, exp_rays = _oracle(name, world, camera, depth, k)
    W, Hh = camera.width, camera.height
    env(SPECIALIZE=specialise)
    for devices, bands in (([0], (0, 16, 7)), ([0, 0], (0, 16, 7)), ([0, 0, 0], (0, 16, 7)), ([0] * 5, (0, 16, 7))):  # (five entries at 64-row bands: some own no row)
        for band_rows in bands:
            what = "%s k=%d specialise=%d devices=%s band_rows=%d" % (name, k, specialise, devices, band_rows)
            canvas = camera.render(world, depth, devices=devices, band_rows=band_rows, supersample=k)
            H.assert_images_equal(canvas.data, exp, what)
            st = camera.last_stats
            assert st["rays"] == exp_rays and st["pixels"] == (k * W - 1) * (k * Hh - 1), (what, st, exp_rays)
            assert st["launches"] == _owners(Hh, band_rows, len(devices)) and st["flags"] == 0, (what, st)
            q = camera.render(world, depth, devices=devices, band_rows=band_rows, quantize=True, supersample=k)
            assert q.dtype == np.uint8 and q.shape == (Hh, W, 3) and np.array_equal(q, exp_u8), what
            st = camera.last_stats
            assert st["rays"] == exp_rays and st["launches"] == _owners(Hh, band_rows, len(devices)) and st["flags"] == 0, (what, st)
    name_of = P.lib().rtc_ctx_kernel_name(P.lib().rtc_diag_seam_ctx(0)).decode()
    # the seam's contexts launch the variant of the supersampling kernels that stores bytes and reports its rows: the name says so
    assert name_of.startswith("ss_render_kernel_spec[" if specialise else "ss_seam_render_kernel<") and ";ss=%d" % k in name_of, name_of
    assert name_of.endswith(";seam]") if specialise else True, name_of
    kid = P.lib().rtc_ctx_kernel_id(P.lib().rtc_diag_seam_ctx(0)).decode()
    assert kid.startswith("spec_") if specialise else (kid.startswith("aot_ss%d_" % k) and kid.endswith(".seam")), kid
    r = Renderer(world, camera, device=0, supersample=k)  # ... and a persistent context's kernel is another one
    assert r.kernel_id != kid and "seam" not in r.kernel_name and "seam" not in r.kernel_id, (r.kernel_name, r.kernel_id)
    r.close()


# ---------------------------------------------------------------- 2. lanes per pixel: both reduces in front of the new stores
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("pinned", [0, 1, 2, 3])
def test_lanes_per_pixel(pinned, k, env):
    """One lane per pixel reduces with DPP, several with __shfl_xor; k = 4 caps eight lanes per pixel at four."""
    world, camera, depth = _scene("soft_shadows")
    exp, exp_u8, exp_rays = _oracle("soft_shadows", world, camera, depth, k)
    env(SPECIALIZE=1, SHARE_LOG2=pinned)
    lib = P.lib()
    for devices in ([0], [0, 0]):
        canvas = camera.render(world, depth, devices=devices, supersample=k)
        H.assert_images_equal(canvas.data, exp, "pinned %d k=%d devices=%s" % (pinned, k, devices))
        assert camera.last_stats["rays"] == exp_rays
        assert lib.rtc_diag_ctx_share_log2(lib.rtc_diag_seam_ctx(0)) == (min(pinned, 2) if k == 4 else pinned)
        assert _progress(0)[0], "a pinned lane count is launched as the plain grid, which reports"
        q = camera.render(world, depth, devices=devices, quantize=True, supersample=k)
        assert np.array_equal(q, exp_u8), (pinned, k, devices)
        assert _progress(0)[0]


@pytest.mark.parametrize("k", [2, 4])
def test_a_block_list_launch_does_not_report_and_gives_the_same_frame(k, env):
    """A divided mesh under a point light: the scene's own kernel shares lanes and is launched from a block list, which cannot
    report its rows -- its chunks leave when the stream is done; the ahead-of-time kernels render the plain grid, which reports.
    Same frame and bytes either way, one entry and two."""
    if "mesh" not in _made:
        _made["mesh"] = scenes.mesh(53, 39)
    world, camera, depth = _made["mesh"]
    exp, exp_u8, exp_rays = _oracle("mesh", world, camera, depth, k)
    for specialise in (1, 0):
        env(SPECIALIZE=specialise)
        for devices in ([0], [0, 0]):
            canvas = camera.render(world, depth, devices=devices, band_rows=16, supersample=k)
            H.assert_images_equal(canvas.data, exp, "mesh k=%d specialise=%d devices=%s" % (k, specialise, devices))
            assert camera.last_stats["rays"] == exp_rays
            assert _progress(0)[0] == (specialise == 0), (k, specialise, devices, _progress(0))
            q = camera.render(world, depth, devices=devices, band_rows=16, quantize=True, supersample=k)
            assert np.array_equal(q, exp_u8), (k, specialise, devices)
            assert _progress(0)[0] == (specialise == 0), (k, specialise, devices, _progress(0))


# ---------------------------------------------------------------- 3. rows leave while later rows render
def _want_chunks(rows, width, px_bytes):
    return min(24, max(1, -(-rows * width * px_bytes // (4 << 20))))  # about 4 MB of OUTPUT a chunk, at most 24 (rtc_oneshot.hip)


@pytest.mark.parametrize("size,k", [((2048, 1536), 2), ((1024, 768), 4)])
def test_rows_leave_while_later_rows_render(size, k, env):
    """Two different frames alternate in the same persistent buffers, three rounds: a chunk copied before its rows were in memory
    would carry the other frame's pixels.  f32 and u8, pageable output and page-locked output pre-filled with 0xAB, one device
    and a device listed twice; and the launch must have REPORTED its chunks -- a launch that fell back to "finished when the
    stream is" would pass every comparison."""
    env()
    W, Hh = size
    frames = []
    for make in (scenes.first_scene, scenes.glass_and_mirror):
        world, camera, depth = make(W, Hh)
        r = Renderer(world, camera, device=0, supersample=k)
        img_t = r.render(depth)
        torch.cuda.synchronize()
        st = r.stats()
        frames.append((world, camera, depth, img_t.cpu().numpy(), r.quantize(img_t).cpu().numpy(), st["rays"]))
        r.close()
    assert not np.array_equal(frames[0][3], frames[1][3])
    lib = P.lib()
    n = W * Hh * 3
    pinned = lib.rtc_host_alloc(n * 4)
    assert pinned
    try:
        for rep in range(3):
            for world, camera, depth, want, want_u8, rays in frames:
                for devices in ([0], [0, 0]):
                    share_rows = Hh if len(devices) == 1 else Hh // 2  # 64-row bands dealt over two entries: half each
                    for quantize in (0, 1):
                        expect_chunks = _want_chunks(share_rows, W, 3 if quantize else 12)
                        # pageable
                        got = camera.render(world, depth, devices=devices, quantize=bool(quantize), supersample=k)
                        got = got if quantize else got.data
                        assert np.array_equal(got, want_u8) if quantize else np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rep, devices, quantize)
                        assert camera.last_stats["rays"] == rays and camera.last_stats["launches"] == len(devices)
                        for e in range(len(devices)):
                            reported, chunks = _progress(e)
                            assert reported and (chunks > 1) == (expect_chunks > 1) and chunks <= expect_chunks, (e, devices, quantize, chunks, expect_chunks)
                        # page-locked: DMA straight into `out`
                        C.memset(pinned, 0xAB, n * 4)
                        st = _render_ss(world, camera, depth, k, devices, pinned, quantize=quantize)
                        view = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8 if quantize else C.c_uint32)), shape=(n,)).reshape(Hh, W, 3)
                        assert np.array_equal(view, want_u8 if quantize else want.view(np.uint32)), (rep, devices, quantize, "page-locked")
                        assert st.rays == rays and st.launches == len(devices) and st.rows == Hh
                        for e in range(len(devices)):
                            reported, chunks = _progress(e)
                            assert reported and (chunks > 1) == (expect_chunks > 1), (e, devices, quantize, chunks, expect_chunks)
    finally:
        lib.rtc_host_free(pinned)
        lib.rtc_render_release()
    # what the sizes say: 2048 x 1536 at k = 2 is about 9 chunks of f32 and 3 of bytes on one device, 1024 x 768 at k = 4 is 3 of f32
    if k == 2:
        assert _want_chunks(Hh, W, 12) == 9 and _want_chunks(Hh, W, 3) == 3
    else:
        assert _want_chunks(Hh, W, 12) == 3


# ---------------------------------------------------------------- 4. device output
@pytest.mark.parametrize("k", [2, 4])
def test_device_output(k, env):
    env()
    world, camera, depth = _scene("soft_shadows")
    exp, exp_u8, exp_rays = _oracle("soft_shadows", world, camera, depth, k)
    for devices in ([0], [0, 0]):
        for quantize in (0, 1):
            t = torch.full((camera.height, camera.width, 3), 7, dtype=torch.uint8 if quantize else torch.float32, device="cuda:0")
            st = _render_ss(world, camera, depth, k, devices, t.data_ptr(), band_rows=16, quantize=quantize, on_device=1)
            got = t.cpu().numpy()
            if quantize:
                assert np.array_equal(got, exp_u8), (k, devices)
            else:
                H.assert_images_equal(got, exp, "device output k=%d devices=%s" % (k, devices))
            assert st.rays == exp_rays and st.rows == camera.height and st.launches == len(devices)


# ---------------------------------------------------------------- 5. state shared with rtc_render_ex
def test_factors_alternate_in_the_seams_state(env):
    """k = 1, 2, 4, 2, 1 of one scene in one process, then another camera, then another scene -- each call gives its own frame,
    the k = 1 frames are rtc_render_ex's and the oracle's plain frame -- and all of it again after rtc_render_release."""
    env()
    world, camera, depth = _scene("glass_and_mirror")
    plain, plain_rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=THREADS)
    other = P.Camera(40, 30, camera.field_of_view, P.view_transform(P.point(1.0, 2.5, -6.0), P.point(0.0, 1.0, 0.0), P.vector(0, 1, 0)))
    world2, camera2, depth2 = _scene("hexagons")
    for again in range(2):
        for k in (1, 2, 4, 2, 1):
            out = np.full((camera.height, camera.width, 3), 9.0, dtype=f32)
            st = _render_ss(world, camera, depth, k, [0], out.ctypes.data)
            if k == 1:
                H.assert_images_equal(out, plain, "k=1 through rtc_render_ss")
                assert st.rays == plain_rays and st.pixels == (camera.width - 1) * (camera.height - 1)
                ex = np.zeros_like(out)
                _render_ss(world, camera, depth, 1, [0], ex.ctypes.data, entry="rtc_render_ex")
                H.assert_images_equal(ex, out, "rtc_render_ex")
            else:
                exp, _, rays = _oracle("glass_and_mirror", world, camera, depth, k)
                H.assert_images_equal(out, exp, "k=%d in the sequence" % k)
                assert st.rays == rays and st.pixels == (k * camera.width - 1) * (k * camera.height - 1) and st.rows == camera.height
        for k in (2, 4, 1):  # another camera
            exp, exp_u8, rays = _oracle("glass_and_mirror/other", world, other, depth, k)
            H.assert_images_equal(other.render(world, depth, supersample=k).data, exp, "other camera k=%d" % k)
            assert other.last_stats["rays"] == rays
        for k in (4, 2):  # another scene
            exp, exp_u8, rays = _oracle("hexagons", world2, camera2, depth2, k)
            assert np.array_equal(camera2.render(world2, depth2, supersample=k, quantize=True), exp_u8), k
            H.assert_images_equal(camera2.render(world2, depth2, supersample=k).data, exp, "other scene k=%d" % k)
        P.lib().rtc_render_release()


# ---------------------------------------------------------------- 6. the Python and C++ surfaces
@pytest.mark.parametrize("k", [2, 4])
def test_python_surface_is_the_ctypes_call(k, env):
    env()
    world, camera, depth = _scene("hexagons")
    for quantize in (0, 1):
        raw = np.zeros((camera.height, camera.width, 3), dtype=np.uint8 if quantize else f32)
        st = _render_ss(world, camera, depth, k, [0, 0], raw.ctypes.data, band_rows=16, quantize=quantize)
        got = camera.render(world, depth, devices=[0, 0], band_rows=16, quantize=bool(quantize), supersample=k)
        got = got if quantize else got.data
        assert got.dtype == raw.dtype and np.array_equal(got.view(np.uint8), raw.view(np.uint8))
        assert camera.last_stats["rays"] == st.rays and camera.last_stats["pixels"] == st.pixels
    # out=: the caller's array is filled and returned
    mine = np.zeros((camera.height, camera.width, 3), dtype=np.uint8)
    assert camera.render(world, depth, quantize=True, supersample=k, out=mine) is mine and np.array_equal(mine, raw)


@pytest.mark.parametrize("k", [2, 4])
def test_cpp_surface_prints_the_oracles_ppm(k):
    """demos/supersampled.cpp: first_scene through Camera::render_supersampled (include/rtc.hpp)."""
    demos = os.path.join(ROOT, "demos")
    subprocess.check_call(["make", "-C", demos, "-s", "supersampled"])
    p = subprocess.run([os.path.join(demos, "supersampled"), "100x50", str(k)], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    world, camera, depth = _scene("first_scene")
    exp, _, _ = _oracle("first_scene", world, camera, depth, k)
    assert p.stdout == O.to_ppm(exp) + b"\n"
    bad = subprocess.run([os.path.join(demos, "supersampled"), "100x50", "3"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "factor 3" in bad.stderr
