"""rtc_render_lens without a device: the one-call seam's lens entry point exists and is declared, answers its argument errors on the
host -- before any device call, rtc_render_ss's checks first and then the lens's, in check_lens_args' order --, the Python surface
refuses what it can refuse itself, and the seam's lens kernels (csrc/rtc_lens_seam.h) are planned by the formula of every scene
kernel: the persistent lens kernel's options with one more last, three headers behind the key, names, ids and cache files of
their own -- while every entry the plan had before keeps its value."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "csrc")
# hiprtc's options in front of a variant's own (csrc/rtc_jit.h plan_jit)
FIXED = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize"]
# the bad lenses of tests/test_lens_boundary.py, restated: (aperture_radius, focal_distance, a word of the message)
BAD_LENSES = [(-0.5, 1.0, b"aperture"), (float("nan"), 1.0, b"aperture"), (float("inf"), 1.0, b"aperture"), (-0.0001, 1.0, b"aperture"),
              (0.1, 0.0, b"focal"), (0.1, -2.0, b"focal"), (0.1, float("nan"), b"focal"), (0.1, float("inf"), b"focal")]


def fnv1a(data, h=1469598103934665603):  # (the library's offset basis, csrc/rtc_internal.h)
    for byte in data:
        h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


_texts = {}


def source_hash(name, h=None):
    """FNV-1a over csrc/<name>, continued from h."""
    if name not in _texts:
        with open(os.path.join(CSRC, name), "rb") as f:
            _texts[name] = f.read()
    return fnv1a(_texts[name]) if h is None else fnv1a(_texts[name], h)


def _call(cs, cam, depth, k, lens, out, opts=None):
    lib = P.lib()
    st = L.rtc_stats()
    rc = lib.rtc_render_lens(C.byref(cs.scene), C.byref(cam) if cam is not None else None, depth, k, C.byref(lens) if lens is not None else None,
                             C.byref(opts) if opts is not None else None, out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(st))
    return rc, lib.rtc_last_error()


# ---- 1. the symbol, its declarations, the ABI -----------------------------------------------------------------------------
def test_the_symbol_exists_and_is_declared():
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "rtc_render_lens") and "rtc_render_lens" in L.SIGNATURES
    assert P.lib().rtc_render_lens.restype is C.c_int and len(P.lib().rtc_render_lens.argtypes) == 8
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert ("rtc_status rtc_render_lens(const rtc_scene* scene, const rtc_camera* output_camera, int32_t depth, uint32_t k, const rtc_lens* lens,\n"
            "                           const rtc_opts* opts, void* out, rtc_stats* stats);") in header
    assert "#define RTC_ABI_VERSION 8" in header and P.lib().rtc_abi_version() == 8
    assert "lens" in inspect.signature(P.Camera.render).parameters
    hpp = open(os.path.join(ROOT, "include", "rtc.hpp")).read()
    assert "struct Lens {" in hpp and "Canvas render_lens(World world, int16_t reflection_recursion_depth, uint32_t k, Lens lens," in hpp
    # what is still not offered, in the three places that say it (its "Declined" sentence)
    for path, section, marker in (("include/rtc.h", "void rtc_render_release(void);", "Not offered"), ("README.md", "**Depth of field**", "Not offered"),
                                  ("DESIGN.md", "## 8g.", "**Declined**")):
        text = open(os.path.join(ROOT, path)).read()
        at = text.index(marker, text.index(section))
        sentence = " ".join(text[at:at + 500].replace(" * ", " ").split())
        assert "daptive lens frames" in sentence[:200] and "dist.py" in sentence, (path, sentence)
        upto = sentence[:min(sentence.index("daptive lens frames"), sentence.index("dist.py"))]
        assert "rtc_render" not in upto and "rtc.hpp" not in upto and "one-call seam" not in upto, (path, sentence)


# ---- 2. argument errors, without a device ---------------------------------------------------------------------------------
def test_argument_errors_are_decided_on_the_host_in_order():
    world, camera, depth = scenes.single_sphere(32, 32)
    cs, cam = world._c(), camera._cam
    out = np.zeros((32, 32, 3), dtype=f32)
    good = L.rtc_lens(0.1, 5.0, 0)
    bad = L.rtc_lens(-1.0, -1.0, 0)
    # rtc_render_ss's checks first -- null `out`, null camera, an empty canvas --, whatever the factor and the lens are
    for k in (1, 2, 3, 4):
        for lens in (good, bad, None):
            rc, msg = _call(cs, cam, depth, k, lens, None)
            assert rc == L.RTC_ERR_INVALID_ARG and b"null argument" in msg, (k, msg)
            rc, msg = _call(cs, None, depth, k, lens, out)
            assert rc == L.RTC_ERR_INVALID_ARG and b"null argument" in msg, (k, msg)
            empty = L.rtc_camera()
            C.memmove(C.byref(empty), C.byref(cam), C.sizeof(L.rtc_camera))
            empty.width = 0
            rc, msg = _call(cs, empty, depth, k, lens, out)
            assert rc == L.RTC_ERR_INVALID_ARG and b"empty canvas" in msg, (k, msg)
    # then check_lens_args' order.  A null lens: an error whatever else is wrong, never rtc_render_ss's frame
    for k in (1, 2, 3, 4):
        rc, msg = _call(cs, cam, depth, k, None, out)
        assert rc == L.RTC_ERR_INVALID_ARG and b"rtc_render_lens" in msg and b"lens is NULL" in msg, (k, msg)
    # the factor, in front of the lens's values: k = 1 with a lens is an error, and so is every factor but 2 and 4
    for k in (0, 1, 3, 5, 8):
        for lens in (good, bad):
            rc, msg = _call(cs, cam, depth, k, lens, out)
            assert rc == L.RTC_ERR_INVALID_ARG and b"factor %d" % k in msg and b"2 or 4" in msg, (k, msg)
    # the aperture in front of the focal distance
    for k in (2, 4):
        rc, msg = _call(cs, cam, depth, k, bad, out)
        assert rc == L.RTC_ERR_INVALID_ARG and b"aperture" in msg and b"focal" not in msg, msg
        for radius, focal, word in BAD_LENSES:
            rc, msg = _call(cs, cam, depth, k, L.rtc_lens(radius, focal, 0), out)
            assert rc == L.RTC_ERR_INVALID_ARG and word in msg and b"rtc_render_lens" in msg, (radius, focal, msg)
    # the lens in front of the fine frame; a fine frame beyond 2^32 pixels or 2^17 rows is refused with nothing written
    for w, h, k in ((40000, 40000, 4), (8, 40000, 4), (8, 70000, 2)):
        big = L.rtc_camera()
        L.check(P.lib().rtc_camera_new(w, h, f32(0.9), camera.transform.ctypes.data_as(L.FP), C.byref(big)))
        one = np.zeros(3, dtype=f32)
        rc, msg = _call(cs, big, depth, k, bad, one)
        assert rc == L.RTC_ERR_INVALID_ARG and b"aperture" in msg, msg
        rc, msg = _call(cs, big, depth, k, good, one)
        assert rc == L.RTC_ERR_INVALID_ARG and b"by %d" % k in msg and b"%d x %d" % (w, h) in msg, (w, h, k, msg)
        assert not one.any()
    assert not out.any()  # no refused call has written anything
    P.lib().rtc_render_release()


def test_a_valid_call_without_a_device_is_no_device():
    """... and where there is one, tests/test_gpu_seam_lens.py renders through the same call and compares the frame."""
    world, camera, depth = scenes.single_sphere(32, 32)
    out = np.zeros((32, 32, 3), dtype=f32)
    if P.device_count() != 0:
        return
    for k in (2, 4):
        for lens in (L.rtc_lens(0.1, 5.0, 0), L.rtc_lens(0.0, 1.0, 9)):  # (a pinhole's aperture is a valid lens)
            rc, msg = _call(world._c(), camera._cam, depth, k, lens, out)
            assert rc == L.RTC_ERR_NO_DEVICE and msg != b"", (k, rc, msg)
    with pytest.raises(P.RtcError) as e:
        camera.render(world, depth, supersample=2, lens=P.Lens(0.1, 5.0))
    assert e.value.status == L.RTC_ERR_NO_DEVICE
    assert not out.any()


# ---- 3. the Python surface ------------------------------------------------------------------------------------------------
def test_python_surface_refuses_a_lens_without_a_factor_of_2_or_4(monkeypatch):
    world, camera, depth = scenes.single_sphere(16, 16)
    called = []
    monkeypatch.setattr(P.World, "_c", lambda self: called.append(1))  # (the library is not reached: the scene is not even packed)
    lens = P.Lens(0.1, 5.0)
    with pytest.raises(ValueError):
        camera.render(world, depth, lens=lens)  # supersample defaults to 1
    with pytest.raises(ValueError):
        camera.render(world, depth, supersample=1, lens=lens)
    for k in (0, 3, 8):
        with pytest.raises(ValueError):
            camera.render(world, depth, supersample=k, lens=lens)
    with pytest.raises(TypeError):
        camera.render(world, depth, supersample=2, lens=(0.1, 5.0))
    assert not called


def test_the_library_refuses_a_bad_lens_given_through_python():
    world, camera, depth = scenes.single_sphere(16, 16)
    for radius, focal, word in BAD_LENSES:
        with pytest.raises(P.RtcError) as e:
            camera.render(world, depth, supersample=2, lens=P.Lens(radius, focal))
        assert e.value.status == L.RTC_ERR_INVALID_ARG and word.decode() in str(e.value), (radius, focal, str(e.value))


# ---- 4. the seam's lens kernels in the plan --------------------------------------------------------------------------------
@pytest.fixture
def _library_defaults(monkeypatch):
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)


# a flat world, an area-light world whose kernel shares lanes, a divided mesh
@pytest.mark.parametrize("name", ["reflect_refract", "soft_shadows", "mesh"])
def test_the_seams_lens_kernels_are_planned_by_the_formula(name, _library_defaults):
    world, camera, _ = getattr(scenes, name)(64, 48)
    plan = world.scene_plan(camera)[1]
    core = source_hash("rtc_kernel_core.h")
    tail = "hiprtc %s abi 8 args %s\n" % (plan["hiprtc"], plan["render_args"])
    if name == "soft_shadows":
        assert "-DRTC_SPEC_SHARE=1" in plan["lens2_seam_spec_defs"].split()
    if name == "mesh":
        assert plan["lens2_seam_family_name"].startswith("lens_seam_render_kernel<tree")
    seen = set()
    for k in (2, 4):
        seam, lens, ss = "lens%d_seam_" % k, "lens%d_" % k, "ss%d_" % k
        assert plan[seam + "entry"] == "lens_render_kernel_spec" == plan[lens + "entry"]
        assert (plan[seam + "header"], plan[seam + "header_below"], plan[seam + "header_below2"]) == ("rtc_lens_seam.h", "rtc_lens.h", "rtc_supersample.h")
        # names: what rtc_ctx_kernel_name reports on a context of the seam
        assert plan[seam + "family_name"] == plan[lens + "family_name"].replace("lens_render_kernel<", "lens_seam_render_kernel<")
        assert plan[seam + "family_name"].startswith("lens_seam_render_kernel<") and plan[seam + "family_name"].endswith(";ss=%d>" % k)
        assert plan[seam + "spec_name"] == plan[lens + "spec_name"][:-1] + ";seam]"
        assert plan[seam + "spec_name"].startswith("lens_render_kernel_spec[") and plan[seam + "spec_name"].endswith(";ss=%d;lens;seam]" % k)
        # options: the persistent lens kernel's and one more, last -- not stacked on the supersampling seam's
        defs = plan[seam + "spec_defs"].split()
        assert defs == plan[lens + "spec_defs"].split() + ["-DRTC_SPEC_LENS_SEAM=1"]
        assert defs[-2:] == ["-DRTC_SPEC_LENS=1", "-DRTC_SPEC_LENS_SEAM=1"] and "-DRTC_SPEC_SS=%d" % k in defs
        assert not any(d.startswith("-DRTC_SPEC_SS_SEAM") for d in defs)
        options = FIXED + defs + ([] if any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in defs) else ["-DRTC_WAVES_PER_SIMD=7"])
        assert plan[seam + "options"].split() == options
        assert plan[seam + "args"] == plan[lens + "args"]  # one argument block: LensRenderArgs
        # the cache file and the ahead-of-time id: three headers' bytes behind the key, rtc_supersample.h, rtc_lens.h, rtc_lens_seam.h
        key = "".join(o + "\n" for o in options) + tail + "lens args %s\n" % plan[seam + "args"]
        h = source_hash("rtc_lens_seam.h", source_hash("rtc_lens.h", source_hash("rtc_supersample.h", fnv1a(key.encode(), core))))
        assert plan[seam + "cache_file"] == "spec_%016x.hsaco" % h
        own = source_hash("rtc_lens_seam.h", source_hash("rtc_lens.h", source_hash("rtc_supersample.h", core)))
        assert plan[seam + "aot_id"] == "aot_lens%d_%016x.seam" % (k, own)
        # ... other ones than the persistent lens kernel's and than the supersampling kernels', the seam's variant of those among them
        # (rtc_scene_prep.h plan_supersampled(seam): -DRTC_SPEC_SS_SEAM=1 last, the persistent kernel's id + ".seam")
        ss_defs = plan[ss + "spec_defs"].split() + ["-DRTC_SPEC_SS_SEAM=1"]
        ss_options = FIXED + ss_defs + ([] if any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in ss_defs) else ["-DRTC_WAVES_PER_SIMD=7"])
        ss_seam_file = "spec_%016x.hsaco" % source_hash("rtc_supersample.h", fnv1a(("".join(o + "\n" for o in ss_options) + tail).encode(), core))
        ss_seam_id = plan[ss + "aot_id"] + ".seam"
        ids = [plan[seam + "aot_id"], plan[lens + "aot_id"], plan[ss + "aot_id"], ss_seam_id]
        files = [plan[seam + "cache_file"], plan[lens + "cache_file"], plan[ss + "cache_file"], ss_seam_file]
        assert len(set(ids)) == 4 and len(set(files)) == 4, (ids, files)
        seen |= set(ids) | set(files)
        # what the plan had before is what it was: the persistent lens kernel's entries by the formula of tests/test_lens_boundary.py
        lens_defs = plan[lens + "spec_defs"].split()
        assert lens_defs == plan[ss + "spec_defs"].split() + ["-DRTC_SPEC_LENS=1"]
        lens_options = FIXED + lens_defs + ([] if any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in lens_defs) else ["-DRTC_WAVES_PER_SIMD=7"])
        lens_key = "".join(o + "\n" for o in lens_options) + tail + "lens args %s\n" % plan[lens + "args"]
        assert plan[lens + "cache_file"] == "spec_%016x.hsaco" % source_hash("rtc_lens.h", source_hash("rtc_supersample.h", fnv1a(lens_key.encode(), core)))
        assert plan[lens + "aot_id"] == "aot_lens%d_%016x" % (k, source_hash("rtc_lens.h", source_hash("rtc_supersample.h", core)))
        assert plan[ss + "aot_id"] == "aot_ss%d_%016x" % (k, source_hash("rtc_supersample.h", core))
        assert lens + "header_below2" not in plan and ss + "header_below" not in plan
    assert len(seen) == 16 and plan["cache_file"] not in seen and plan["aot_id"] not in seen
    assert plan["aot_id"] == "aot_%016x" % core


def test_the_new_entries_leave_every_other_entry_alone(_library_defaults):
    """The plan's text without its lens<k>_seam_ lines is a plan of the earlier form: the same keys in the same order, none of them
    between two lines that belong together, and every kernel text that identifies an earlier kernel is untouched by the new header
    (its hash does not depend on rtc_lens_seam.h: the formulas above and in tests/test_jit_plan.py / test_lens_boundary.py)."""
    world, camera, _ = scenes.reflect_refract(64, 48)
    cs = world._c()
    text, digests = C.create_string_buffer(1 << 16), (C.c_uint64 * 4)()
    L.check(P.lib().rtc_diag_scene_plan(C.byref(cs.scene), C.byref(camera._cam), text, len(text), digests))
    lines = text.value.decode().splitlines()
    new = [i for i, ln in enumerate(lines) if ln.startswith(("lens2_seam_", "lens4_seam_"))]
    per_kernel = ["family_name", "spec_name", "spec_defs", "header_below", "header_below2", "entry", "header", "options", "cache_file", "aot_id", "args"]
    assert len(new) == 2 * len(per_kernel) and new == list(range(new[0], new[0] + len(new))) and new[-1] == len(lines) - 1, new  # one run, at the end
    keys = [ln.split("=", 1)[0] for ln in lines]
    assert len(set(keys)) == len(keys)
    assert keys[new[0]:] == ["lens%d_seam_%s" % (k, what) for k in (2, 4) for what in per_kernel]
