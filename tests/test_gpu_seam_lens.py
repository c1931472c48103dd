"""Depth of field through the one-call seam (-m gpu): rtc_render_lens / Camera.render(..., lens=) / Camera::render_lens /
demos/depth_of_field / demo.py --aperture.

The expected frame is the one rtc_ctx_set_scene_lens defines: tests/lens_helpers.py::oracle_lens_frame -- the box filter of the fine
frame whose pixel is the oracle's color_at of the ray rtc_lens_rays gives it; for bytes, O.quantize of that.  f32 frames are compared
bit for bit, bytes for equality.  The oracle's side is a Python loop over fine pixels, so each frame is computed once and shared.
Where a test is about the transport (rows leaving while later rows render) the expectation is the persistent context's frame,
Renderer(world, camera, supersample=k, lens=lens), which tests/test_gpu_lens.py ties to the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import demo, scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests import lens_helpers as LH
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


_made, _expected = {}, {}


def _case(name):
    """(world, camera, depth), k, lens of a case of lens_helpers.CASES: made once."""
    if name not in _made:
        make, k, lens, _ = LH.CASES[name]
        _made[name] = (make(), k, lens)
    return _made[name]


def _oracle(key, world, camera, depth, k, lens):
    """(expected f32 frame, its bytes, the rays traced): computed once per key, never changed."""
    if key not in _expected:
        exp, rays, _ = LH.oracle_lens_frame(H.oracle_world(world), camera, depth, k, lens)
        exp.setflags(write=False)
        _expected[key] = (exp, O.quantize(exp), rays)
    return _expected[key]


def _oracle_of(name):
    (world, camera, depth), k, lens = _case(name)
    return _oracle(name, world, camera, depth, k, lens)


def _render_lens(world, camera, depth, k, lens, devices, out_ptr, band_rows=0, quantize=0, on_device=0):
    """The ctypes call itself -> rtc_stats."""
    lib, cs = P.lib(), world._c()
    arr = (C.c_int32 * len(devices))(*devices)
    opts = L.rtc_opts(arr, len(devices), band_rows, quantize, on_device)
    st = L.rtc_stats()
    L.check(lib.rtc_render_lens(C.byref(cs.scene), C.byref(camera._cam), depth, k, C.byref(lens._c), C.byref(opts), C.c_void_p(out_ptr), C.byref(st)))
    return st


def _render_other(world, camera, depth, k, out_ptr):
    """rtc_render_ex (k = 1) / rtc_render_ss on entry 0 -> rtc_stats."""
    lib, cs = P.lib(), world._c()
    arr = (C.c_int32 * 1)(0)
    opts = L.rtc_opts(arr, 1, 0, 0, 0)
    st = L.rtc_stats()
    if k == 1:
        L.check(lib.rtc_render_ex(C.byref(cs.scene), C.byref(camera._cam), depth, C.byref(opts), C.c_void_p(out_ptr), C.byref(st)))
    else:
        L.check(lib.rtc_render_ss(C.byref(cs.scene), C.byref(camera._cam), depth, k, C.byref(opts), C.c_void_p(out_ptr), C.byref(st)))
    return st


def _owners(height, band_rows, n_entries):
    """Entries of opts->devices that own at least one band of output rows: each of them launches once."""
    band = band_rows or 64
    return min(n_entries, -(-height // band))


def _progress(entry):
    out = (C.c_uint32 * 2)()
    assert P.lib().rtc_diag_seam_progress(entry, out) == 1
    return bool(out[0]), int(out[1])


def _seam_kernel():
    lib = P.lib()
    ctx = lib.rtc_diag_seam_ctx(0)
    return lib.rtc_ctx_kernel_name(ctx).decode(), lib.rtc_ctx_kernel_id(ctx).decode()


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("specialise", [0, 1])
@pytest.mark.parametrize("name", ["sphere_grid_k2", "sphere_grid_k4", "soft_shadows_k2", "soft_shadows_k4", "reflect_refract_inside_the_glass", "golden_mesh"])
def test_against_the_oracle(name, specialise, env):
    (world, camera, depth), k, lens = _case(name)
    exp, exp_u8, exp_rays = _oracle_of(name)
    W, Hh = camera.width, camera.height
    env(SPECIALIZE=specialise)
    # (a band height of 7 over 16 - 18 rows puts band edges inside the k x k blocks' tiles; five entries leave some owning no row)
    for devices in ([0], [0, 0], [0] * 5):
        for band_rows in (0, 16, 7):
            what = "%s specialise=%d devices=%s band_rows=%d" % (name, specialise, devices, band_rows)
            canvas = camera.render(world, depth, devices=devices, band_rows=band_rows, supersample=k, lens=lens)
            H.assert_images_equal(canvas.data, exp, what)
            st = camera.last_stats
            assert st["rays"] == exp_rays and st["pixels"] == (k * W - 1) * (k * Hh - 1), (what, st, exp_rays)
            assert st["launches"] == _owners(Hh, band_rows, len(devices)) and st["flags"] == 0, (what, st)
            q = camera.render(world, depth, devices=devices, band_rows=band_rows, quantize=True, supersample=k, lens=lens)
            assert q.dtype == np.uint8 and q.shape == (Hh, W, 3) and np.array_equal(q, exp_u8), what
            st = camera.last_stats
            assert st["rays"] == exp_rays and st["launches"] == _owners(Hh, band_rows, len(devices)) and st["flags"] == 0, (what, st)
            raw = np.zeros((Hh, W, 3), dtype=f32)
            assert _render_lens(world, camera, depth, k, lens, devices, raw.ctypes.data, band_rows=band_rows).rows == Hh
    # the seam's contexts launch the variant of the lens kernels that stores bytes and reports its rows: name and id say so
    name_of, kid = _seam_kernel()
    if specialise:
        assert name_of.startswith("lens_render_kernel_spec[") and name_of.endswith(";ss=%d;lens;seam]" % k), name_of
        assert kid.startswith("spec_"), kid
    else:
        assert name_of.startswith("lens_seam_render_kernel<") and name_of.endswith(";ss=%d>" % k), name_of
        assert kid.startswith("aot_lens%d_" % k) and kid.endswith(".seam"), kid
    plan = world.scene_plan(camera)[1]
    assert name_of == plan["lens%d_seam_%s" % (k, "spec_name" if specialise else "family_name")]
    assert (kid.partition(".")[0] + ".hsaco" == plan["lens%d_seam_cache_file" % k]) if specialise else (kid == plan["lens%d_seam_aot_id" % k])
    r = Renderer(world, camera, device=0, supersample=k, lens=lens)  # ... and a persistent context's kernel is another one
    assert r.kernel_id != kid and "seam" not in r.kernel_name and "seam" not in r.kernel_id, (r.kernel_name, r.kernel_id)
    assert r.kernel_id.partition(".")[0] != kid.partition(".")[0]
    r.close()


# ---------------------------------------------------------------- 2. lanes per pixel: both reduces in front of the new stores
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("pinned", [0, 1, 2, 3])
def test_lanes_per_pixel(pinned, k, env):
    """One lane per pixel reduces with DPP, several with __shfl_xor; k = 4 caps eight lanes per pixel at four."""
    (world, camera, depth), _, lens = _case("soft_shadows_k%d" % k)
    exp, exp_u8, exp_rays = _oracle_of("soft_shadows_k%d" % k)
    env(SPECIALIZE=1, SHARE_LOG2=pinned)
    lib = P.lib()
    for devices in ([0], [0, 0]):
        canvas = camera.render(world, depth, devices=devices, band_rows=8, supersample=k, lens=lens)
        H.assert_images_equal(canvas.data, exp, "pinned %d k=%d devices=%s" % (pinned, k, devices))
        assert camera.last_stats["rays"] == exp_rays
        assert lib.rtc_diag_ctx_share_log2(lib.rtc_diag_seam_ctx(0)) == (min(pinned, 2) if k == 4 else pinned)
        assert _progress(0)[0], "a pinned lane count is launched as the plain grid, which reports"
        q = camera.render(world, depth, devices=devices, band_rows=8, quantize=True, supersample=k, lens=lens)
        assert np.array_equal(q, exp_u8), (pinned, k, devices)
        assert _progress(0)[0]


@pytest.mark.parametrize("name", ["golden_mesh", "mesh"])
def test_a_block_list_launch_does_not_report_and_gives_the_same_frame(name, env):
    """A divided mesh under a point light whose scene kernel shares lanes is launched from a block list, which cannot report its rows --
    its chunks leave when the stream is done; the ahead-of-time kernels render the plain grid, which reports.  Same frame and bytes
    either way, one entry and two.
    Which launches come from a block list is the planning code's choice, the same for a persistent context (rtc_diag_scene_plan:
    spec_shares and heavy_tiles): golden_mesh's 22 triangles are no heavy tile at 48 x 32 fine pixels, its kernel does not share lanes
    and its launch is the plain grid, which reports under either switch -- measured: (reported, chunks) = (True, 1) with
    RTC_AMD_SPECIALIZE=1.  So `mesh` (scenes.mesh, 32 x 24: heavy tiles, lane sharing) stands beside it: the smallest frame that does
    reach the block list, with the expectation in full -- 1 does not report, 0 reports."""
    if name == "mesh":
        if name not in _made:
            _made[name] = (scenes.mesh(32, 24), 2, P.Lens(0.2, 5.6, seed=4))
    (world, camera, depth), k, lens = _case(name)
    exp, exp_u8, exp_rays = _oracle(name, world, camera, depth, k, lens)
    plan = world.scene_plan(camera.supersampled(k))[1]
    listed = plan["spec_shares"] == "1" and not plan["heavy_tiles"].startswith("0 ")
    assert listed == (name == "mesh")
    for specialise in (1, 0):
        env(SPECIALIZE=specialise)
        for devices in ([0], [0, 0]):
            reports = not (specialise == 1 and listed)
            canvas = camera.render(world, depth, devices=devices, band_rows=8, supersample=k, lens=lens)
            H.assert_images_equal(canvas.data, exp, "%s specialise=%d devices=%s" % (name, specialise, devices))
            assert camera.last_stats["rays"] == exp_rays
            assert _progress(0)[0] == reports, (name, specialise, devices, _progress(0))
            q = camera.render(world, depth, devices=devices, band_rows=8, quantize=True, supersample=k, lens=lens)
            assert np.array_equal(q, exp_u8), (name, specialise, devices)
            assert _progress(0)[0] == reports, (name, specialise, devices, _progress(0))


# ---------------------------------------------------------------- 3. rows leave while later rows render
def _want_chunks(rows, width, px_bytes):
    return min(24, max(1, -(-rows * width * px_bytes // (4 << 20))))  # about 4 MB of OUTPUT a chunk, at most 24 (rtc_oneshot.hip)


def test_rows_leave_while_later_rows_render(env):
    """1024 x 512 at k = 2: 6.3 MB of f32 are two chunks on one device, the bytes one -- the smallest shape at which a chunk copied
    before its rows were in memory would show.  Two different frames alternate in the same persistent buffers, three rounds, pageable
    output and page-locked output pre-filled with 0xAB; and the f32 launch must have REPORTED its chunks -- a launch that fell back to
    "finished when the stream is" would pass every comparison."""
    env()
    W, Hh, k = 1024, 512, 2
    assert _want_chunks(Hh, W, 12) == 2 and _want_chunks(Hh, W, 3) == 1
    lens = P.Lens(0.15, 5.0, seed=6)
    frames = []
    for make in (scenes.first_scene, scenes.glass_and_mirror):
        world, camera, depth = make(W, Hh)
        r = Renderer(world, camera, device=0, supersample=k, lens=lens)
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
    pageable = {0: np.zeros((Hh, W, 3), dtype=f32), 1: np.zeros((Hh, W, 3), dtype=np.uint8)}
    try:
        for rep in range(3):
            for world, camera, depth, want, want_u8, rays in frames:
                for quantize in (0, 1):
                    expect_chunks = _want_chunks(Hh, W, 3 if quantize else 12)
                    got = camera.render(world, depth, quantize=bool(quantize), supersample=k, lens=lens, out=pageable[quantize])
                    got = got if quantize else got.data
                    assert np.array_equal(got, want_u8) if quantize else np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rep, quantize)
                    assert camera.last_stats["rays"] == rays and camera.last_stats["launches"] == 1
                    reported, chunks = _progress(0)
                    assert reported and chunks == expect_chunks, (quantize, chunks, expect_chunks)
                    # page-locked: DMA straight into `out`
                    C.memset(pinned, 0xAB, n * 4)
                    st = _render_lens(world, camera, depth, k, lens, [0], pinned, quantize=quantize)
                    view = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8 if quantize else C.c_uint32)), shape=(n,)).reshape(Hh, W, 3)
                    assert np.array_equal(view, want_u8 if quantize else want.view(np.uint32)), (rep, quantize, "page-locked")
                    assert st.rays == rays and st.launches == 1 and st.rows == Hh
                    reported, chunks = _progress(0)
                    assert reported and chunks == expect_chunks and (quantize or chunks > 1), (quantize, chunks, expect_chunks)
    finally:
        lib.rtc_host_free(pinned)
        lib.rtc_render_release()


# ---------------------------------------------------------------- 4. device output
@pytest.mark.parametrize("k", [2, 4])
def test_device_output(k, env):
    env()
    (world, camera, depth), _, lens = _case("soft_shadows_k%d" % k)
    exp, exp_u8, exp_rays = _oracle_of("soft_shadows_k%d" % k)
    for devices in ([0], [0, 0]):
        for quantize in (0, 1):
            t = torch.full((camera.height, camera.width, 3), 7, dtype=torch.uint8 if quantize else torch.float32, device="cuda:0")
            st = _render_lens(world, camera, depth, k, lens, devices, t.data_ptr(), band_rows=16, quantize=quantize, on_device=1)
            got = t.cpu().numpy()
            if quantize:
                assert np.array_equal(got, exp_u8), (k, devices)
            else:
                H.assert_images_equal(got, exp, "device output k=%d devices=%s" % (k, devices))
            assert st.rays == exp_rays and st.rows == camera.height and st.launches == _owners(camera.height, 16, len(devices))


# ---------------------------------------------------------------- 5. state shared with rtc_render_ex and rtc_render_ss
def test_calls_alternate_in_the_seams_state(env):
    """rtc_render_ex, rtc_render_ss k = 2, rtc_render_lens k = 2, rtc_render_lens k = 4, rtc_render_ss k = 4, rtc_render_lens k = 2 with
    another lens twice over (a focus pull), rtc_render_ex: one scene, one process, each call its own frame.  Then another camera, then
    another scene -- and all of it again after rtc_render_release."""
    env()
    (world, camera, depth), _, lens = _case("sphere_grid_k2")
    W, Hh = camera.width, camera.height
    own = H.oracle_world(world)
    plain = {kk: H.oracle_camera(camera.supersampled(kk) if kk != 1 else camera).render(own, depth, threads=THREADS) for kk in (1, 2, 4)}
    pulled = P.Lens(0.6, 9.0, seed=1)
    other = P.Camera(20, 12, camera.field_of_view, P.view_transform(P.point(1.0, 2.5, -6.0), P.point(0.0, 1.0, 0.0), P.vector(0, 1, 0)))
    (world2, camera2, depth2), k2, lens2 = _case("soft_shadows_k2")

    def lens_call(kk, ln, key):
        exp, _, rays = _oracle(key, world, camera, depth, kk, ln)
        out = np.full((Hh, W, 3), 9.0, dtype=f32)
        st = _render_lens(world, camera, depth, kk, ln, [0], out.ctypes.data)
        H.assert_images_equal(out, exp, "rtc_render_lens %s in the sequence" % key)
        assert st.rays == rays and st.pixels == (kk * W - 1) * (kk * Hh - 1) and st.rows == Hh and st.launches == 1
        return out

    def other_call(kk):
        fine, rays = plain[kk]
        out = np.full((Hh, W, 3), 9.0, dtype=f32)
        st = _render_other(world, camera, depth, kk, out.ctypes.data)
        H.assert_images_equal(out, fine if kk == 1 else box_filter(fine, kk), "k=%d without a lens in the sequence" % kk)
        assert st.rays == rays
        return out

    for again in range(2):
        other_call(1)
        ss2 = other_call(2)
        a = lens_call(2, lens, "sphere_grid_k2")
        assert not np.array_equal(a, ss2)
        lens_call(4, _case("sphere_grid_k4")[2], "sphere_grid_k4")
        other_call(4)
        first = lens_call(2, lens, "sphere_grid_k2")
        name_of, kid = _seam_kernel()
        b = lens_call(2, pulled, "sphere_grid_k2/pulled")  # the focus pull: the resident scene, camera and factor, another lens
        assert _seam_kernel() == (name_of, kid), "a focus pull plans and compiles nothing: the kernel and its id are the first lens's"
        assert not np.array_equal(first, b)
        lens_call(2, lens, "sphere_grid_k2")  # ... and back
        assert _seam_kernel() == (name_of, kid)
        other_call(1)
        # another camera
        exp, exp_u8, rays = _oracle("sphere_grid/other", world, other, depth, 2, lens)
        H.assert_images_equal(other.render(world, depth, supersample=2, lens=lens).data, exp, "another camera")
        assert other.last_stats["rays"] == rays
        assert np.array_equal(other.render(world, depth, supersample=2, lens=lens, quantize=True), exp_u8)
        # another scene
        exp, exp_u8, rays = _oracle_of("soft_shadows_k2")
        assert np.array_equal(camera2.render(world2, depth2, supersample=k2, lens=lens2, quantize=True), exp_u8)
        H.assert_images_equal(camera2.render(world2, depth2, supersample=k2, lens=lens2).data, exp, "another scene")
        assert camera2.last_stats["rays"] == rays
        P.lib().rtc_render_release()


# ---------------------------------------------------------------- 6. the Python and C++ surfaces, the demo
@pytest.mark.parametrize("k", [2, 4])
def test_python_surface_is_the_ctypes_call(k, env):
    env()
    (world, camera, depth), _, lens = _case("sphere_grid_k%d" % k)
    for quantize in (0, 1):
        raw = np.zeros((camera.height, camera.width, 3), dtype=np.uint8 if quantize else f32)
        st = _render_lens(world, camera, depth, k, lens, [0, 0], raw.ctypes.data, band_rows=7, quantize=quantize)
        got = camera.render(world, depth, devices=[0, 0], band_rows=7, quantize=bool(quantize), supersample=k, lens=lens)
        got = got if quantize else got.data
        assert got.dtype == raw.dtype and np.array_equal(got.view(np.uint8), raw.view(np.uint8))
        assert camera.last_stats["rays"] == st.rays and camera.last_stats["pixels"] == st.pixels
    # out=: the caller's array is filled and returned
    mine = np.zeros((camera.height, camera.width, 3), dtype=np.uint8)
    assert camera.render(world, depth, quantize=True, supersample=k, lens=lens, out=mine) is mine and np.array_equal(mine, raw)
    assert np.array_equal(mine, _oracle_of("sphere_grid_k%d" % k)[1])


_first_scene = {}


def _first_scene_oracle(k, lens):
    if k not in _first_scene:
        world, camera, depth = scenes.first_scene(40, 20)
        _first_scene[k] = _oracle("first_scene/%d" % k, world, camera, depth, k, lens)
    return _first_scene[k]


@pytest.mark.parametrize("k", [2, 4])
def test_cpp_surface_prints_the_oracles_ppm(k):
    """demos/depth_of_field.cpp: first_scene through Camera::render_lens (include/rtc.hpp)."""
    demos = os.path.join(ROOT, "demos")
    subprocess.check_call(["make", "-C", demos, "-s"], timeout=300)
    exe = os.path.join(demos, "depth_of_field")
    p = subprocess.run([exe, "40x20", str(k), "0.2", "5.0", "11"], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    exp, _, _ = _first_scene_oracle(k, P.Lens(0.2, 5.0, seed=11))
    assert p.stdout == O.to_ppm(exp) + b"\n"
    if k == 2:
        bad = subprocess.run([exe, "40x20", "3", "0.2", "5.0"], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "factor 3" in bad.stderr and bad.stdout == "", bad.stderr
        bad = subprocess.run([exe, "40x20", "2", "-0.2", "5.0"], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "aperture" in bad.stderr and bad.stdout == "", bad.stderr


def test_the_demo_goes_through_the_seam_and_writes_the_same_ppm(tmp_path, monkeypatch):
    out = tmp_path / "lens.ppm"
    made = []
    monkeypatch.setattr(Renderer, "__init__", lambda self, *a, **kw: made.append(1))  # (no persistent context any more)
    assert demo.main(["first_scene", "--size", "40x20", "--supersample", "2", "--aperture", "0.2", "--focus", "5.0", "--out", str(out)]) == 0
    assert not made
    name_of, _ = _seam_kernel()
    assert name_of.startswith(("lens_seam_render_kernel<", "lens_render_kernel_spec[")) and "seam" in name_of
    monkeypatch.undo()
    world, camera, depth = scenes.first_scene(40, 20)
    r = Renderer(world, camera, device=0, supersample=2, lens=P.Lens(0.2, 5.0))
    frame = r.render(depth)
    assert out.read_bytes() == r.to_ppm(frame) + b"\n"  # what the demo wrote when it built a Renderer itself
    r.close()
    P.lib().rtc_render_release()


# ---------------------------------------------------------------- 7. a persistent lens context is what it was
def test_a_persistent_lens_context_still_refuses_hits_and_adaptive():
    world, camera, depth = scenes.first_scene(64, 48)
    r = Renderer(world, camera, device=0, supersample=2, lens=P.Lens(0.1, 5.0))
    for call in (lambda: r.render_hits(planes=("object",)), lambda: r.render_adaptive(depth, k=2, threshold=0.1)):
        with pytest.raises(P.RtcError) as e:
            call()
        assert e.value.status == L.RTC_ERR_UNSUPPORTED and "lens" in str(e.value)
    assert r.kernel_name.startswith("lens_render_kernel") and "seam" not in r.kernel_name
    r.close()
