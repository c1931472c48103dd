"""rtc_render_adaptive without a device: the one-call seam's adaptive entry point exists and is declared, answers its argument errors on
the host -- before any device call, rtc_render_ss's checks first, then the threshold, the factor, the fine frame --, the Python surface
refuses what it can refuse itself, the host-only plan of a part's bands and halo rows (rtc_diag_adaptive_bands) is what a restatement
in Python gives, and the seam's adaptive kernels (csrc/rtc_adaptive_seam.h) are planned by the formula of every scene kernel while every
entry the plan had before keeps its bytes (tests/golden/scene_plan_before_adaptive_seam.json: the plan's text of five scenes at 64 x 48
as the commit before this entry point printed it under the library's defaults -- a change of a kernel header or of hiprtc moves the
hashes in it, and whoever makes one prints it again: world.scene_plan's text without its adaptive_seam<k>_ lines)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import demo, scenes

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "csrc")
FIXED = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize"]
PER_KERNEL = ["family_name", "spec_name", "spec_defs", "header_below", "entry", "header", "options", "cache_file", "aot_id", "args"]


def fnv1a(data, h=1469598103934665603):
    for byte in data:
        h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


def source_hash(name, h=None):
    with open(os.path.join(CSRC, name), "rb") as f:
        text = f.read()
    return fnv1a(text) if h is None else fnv1a(text, h)


def _call(cs, cam, depth, k, threshold, out, mask=None, opts=None):
    lib = P.lib()
    st, ad = L.rtc_stats(), L.rtc_seam_adaptive_stats()
    rc = lib.rtc_render_adaptive(C.byref(cs.scene), C.byref(cam) if cam is not None else None, depth, k, f32(threshold), C.byref(opts) if opts is not None else None,
                                 out.ctypes.data_as(C.c_void_p) if out is not None else None, mask.ctypes.data_as(C.c_void_p) if mask is not None else None,
                                 C.byref(st), C.byref(ad))
    return rc, lib.rtc_last_error()


# ---- 1. the symbol, its declarations, the struct, the ABI ----------------------------------------------------------------
def test_the_symbol_exists_and_is_declared():
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "rtc_render_adaptive") and "rtc_render_adaptive" in L.SIGNATURES
    assert hasattr(raw, "rtc_diag_adaptive_bands") and "rtc_diag_adaptive_bands" in L.EXTRA
    assert P.lib().rtc_render_adaptive.restype is C.c_int and len(P.lib().rtc_render_adaptive.argtypes) == 10
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert ("rtc_status rtc_render_adaptive(const rtc_scene* scene, const rtc_camera* camera, int32_t depth, uint32_t k, float threshold,\n"
            "                               const rtc_opts* opts, void* out, void* mask_u8, rtc_stats* stats,\n"
            "                               rtc_seam_adaptive_stats* ad);") in header
    assert "#define RTC_ABI_VERSION 8" in header and P.lib().rtc_abi_version() == 8
    # the new struct: four 64-bit sums and two times; rtc_adaptive_stats keeps its layout
    S = L.rtc_seam_adaptive_stats
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("refined_pixels", 0), ("refine_rays", 8), ("halo_pixels", 16), ("halo_rays", 24),
                                                                 ("mask_ms", 32), ("refine_ms", 36)] and C.sizeof(S) == 40
    for name, _ in S._fields_:
        assert name in header[header.index("typedef struct rtc_seam_adaptive_stats {"):header.index("} rtc_seam_adaptive_stats;")]
    A = L.rtc_adaptive_stats
    assert [(n, getattr(A, n).offset) for n, _ in A._fields_] == [("refined_pixels", 0), ("rays", 8), ("shaded_hits", 16), ("culled_shadow_rays", 24),
                                                                 ("mask_ms", 32), ("refine_ms", 36)] and C.sizeof(A) == 40
    params = inspect.signature(P.Camera.render).parameters
    assert "adaptive" in params and "mask" in params
    hpp = open(os.path.join(ROOT, "include", "rtc.hpp")).read()
    assert "Canvas render_adaptive(World world, int16_t reflection_recursion_depth, uint32_t k, float threshold," in hpp
    # what is still not offered, where the header and DESIGN say it
    for path in ("include/rtc.h", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().replace(" * ", " ").split())
        assert "adaptive frames in dist.py" in text and "partitioned rtc_ctx_render_adaptive" in text, path


# ---- 2. argument errors, without a device ---------------------------------------------------------------------------------
def test_argument_errors_are_decided_on_the_host_in_order():
    world, camera, depth = scenes.single_sphere(32, 32)
    cs, cam = world._c(), camera._cam
    out = np.zeros((32, 32, 3), dtype=f32)
    mask = np.zeros((32, 32), dtype=np.uint8)
    nan, inf = float("nan"), float("inf")
    # rtc_render_ss's checks first -- null `out`, null camera, an empty canvas --, whatever the threshold and the factor are
    for k in (1, 2, 3, 4):
        for threshold in (0.1, -1.0, nan):
            rc, msg = _call(cs, cam, depth, k, threshold, None, mask)
            assert rc == L.RTC_ERR_INVALID_ARG and b"rtc_render_adaptive: null argument" in msg, (k, msg)
            rc, msg = _call(cs, None, depth, k, threshold, out, mask)
            assert rc == L.RTC_ERR_INVALID_ARG and b"null argument" in msg, (k, msg)
            empty = L.rtc_camera()
            C.memmove(C.byref(empty), C.byref(cam), C.sizeof(L.rtc_camera))
            empty.height = 0
            rc, msg = _call(cs, empty, depth, k, threshold, out, mask)
            assert rc == L.RTC_ERR_INVALID_ARG and b"empty canvas" in msg, (k, msg)
    # then the threshold, in front of the factor
    for threshold in (-1.0, -1e-30, nan, inf, -inf):
        for k in (0, 1, 2, 3, 4, 8):
            rc, msg = _call(cs, cam, depth, k, threshold, out, mask)
            assert rc == L.RTC_ERR_INVALID_ARG and b"rtc_render_adaptive" in msg and b"threshold" in msg and b"factor" not in msg, (threshold, k, msg)
    # then the factor: 2 or 4
    for k in (0, 1, 3, 5, 8):
        rc, msg = _call(cs, cam, depth, k, 0.1, out, mask)
        assert rc == L.RTC_ERR_INVALID_ARG and b"factor %d" % k in msg and b"2 or 4" in msg, (k, msg)
    # then the fine frame: beyond 2^32 pixels or 2^17 rows it is refused with nothing written
    for w, h, k in ((40000, 40000, 4), (8, 40000, 4), (8, 70000, 2)):
        big = L.rtc_camera()
        L.check(P.lib().rtc_camera_new(w, h, f32(0.9), camera.transform.ctypes.data_as(L.FP), C.byref(big)))
        one = np.zeros(3, dtype=f32)
        rc, msg = _call(cs, big, depth, k, -1.0, one)
        assert rc == L.RTC_ERR_INVALID_ARG and b"threshold" in msg, msg
        rc, msg = _call(cs, big, depth, 3, 0.1, one)
        assert rc == L.RTC_ERR_INVALID_ARG and b"factor 3" in msg, msg
        rc, msg = _call(cs, big, depth, k, 0.1, one)
        assert rc == L.RTC_ERR_INVALID_ARG and b"by %d" % k in msg and b"%d x %d" % (w, h) in msg, (w, h, k, msg)
        assert not one.any()
    assert not out.any() and not mask.any()  # no refused call has written anything
    P.lib().rtc_render_release()


def test_a_valid_call_without_a_device_is_no_device():
    """... and where there is one, tests/test_gpu_seam_adaptive.py renders through the same call and compares the frame."""
    world, camera, depth = scenes.single_sphere(32, 32)
    out = np.zeros((32, 32, 3), dtype=f32)
    if P.device_count() != 0:
        return
    for k in (2, 4):
        for threshold in (0.0, 0.1, 1e30):
            rc, msg = _call(world._c(), camera._cam, depth, k, threshold, out)
            assert rc == L.RTC_ERR_NO_DEVICE and msg != b"", (k, rc, msg)
    with pytest.raises(P.RtcError) as e:
        camera.render(world, depth, supersample=2, adaptive=0.1)
    assert e.value.status == L.RTC_ERR_NO_DEVICE
    assert not out.any()


# ---- 3. the Python surface and the command line ---------------------------------------------------------------------------
def test_python_surface_refuses_adaptive_with_a_lens_or_without_a_factor(monkeypatch):
    world, camera, depth = scenes.single_sphere(16, 16)
    called = []
    monkeypatch.setattr(P.World, "_c", lambda self: called.append(1))  # (the library is not reached: the scene is not even packed)
    with pytest.raises(ValueError):
        camera.render(world, depth, adaptive=0.1)  # supersample defaults to 1
    with pytest.raises(ValueError):
        camera.render(world, depth, supersample=1, adaptive=0.1)
    for k in (0, 3, 8):
        with pytest.raises(ValueError):
            camera.render(world, depth, supersample=k, adaptive=0.1)
    with pytest.raises(ValueError):
        camera.render(world, depth, supersample=2, adaptive=0.1, lens=P.Lens(0.1, 5.0))
    with pytest.raises(ValueError):
        camera.render(world, depth, supersample=2, mask=np.zeros((16, 16), dtype=np.uint8))  # a mask without adaptive
    for bad in (np.zeros((16, 15), dtype=np.uint8), np.zeros((16, 16), dtype=f32), np.zeros((16, 32), dtype=np.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            camera.render(world, depth, supersample=2, adaptive=0.1, mask=bad)
    assert not called


def test_the_library_refuses_a_bad_threshold_given_through_python():
    world, camera, depth = scenes.single_sphere(16, 16)
    for threshold in (-0.5, float("nan"), float("inf")):
        with pytest.raises(P.RtcError) as e:
            camera.render(world, depth, supersample=2, adaptive=threshold)
        assert e.value.status == L.RTC_ERR_INVALID_ARG and "threshold" in str(e.value)


def test_the_command_line_wants_a_factor_with_adaptive(capsys):
    for argv, why in ((["first_scene", "--adaptive", "0.1"], "--adaptive needs --supersample 2 or 4"),
                      (["first_scene", "--supersample", "1", "--adaptive", "0.1"], "--adaptive needs --supersample 2 or 4"),
                      (["first_scene", "--supersample", "2", "--adaptive", "0.1", "--aperture", "0.1", "--focus", "5"], "--adaptive takes no lens")):
        with pytest.raises(SystemExit) as e:
            demo.main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and why in err and "unrecognized" not in err, err


# ---- 4. a part's bands and halo rows --------------------------------------------------------------------------------------
def _bands(height, band_rows, n_parts, part):
    """The restatement: bands part, part + n_parts, ... of band_rows rows; for every band edge whose neighbouring row belongs to another
    part, that row -- above the band first, then below it, band after band."""
    rows, halo = [], []
    n_bands = (height + band_rows - 1) // band_rows
    for b in range(part, n_bands, n_parts):
        y0, y1 = b * band_rows, min((b + 1) * band_rows, height)
        rows += list(range(y0, y1))
        if n_parts > 1:  # (one part: the band above and the band below are its own)
            halo += ([y0 - 1] if y0 > 0 else []) + ([y1] if y1 < height else [])
    return rows, halo


def _diag(height, band_rows, n_parts, part, cap=1 << 12):
    rows, halo, counts = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * 2)()
    ok = P.lib().rtc_diag_adaptive_bands(height, band_rows, n_parts, part, rows, cap, halo, cap, counts)
    return ok, list(rows[:counts[0]]), list(halo[:counts[1]])


@pytest.mark.parametrize("height,band_rows,n_parts", [(31, 7, 2), (31, 7, 5), (31, 1, 2), (31, 1, 5), (31, 5, 2), (31, 5, 3), (48, 64, 1), (48, 64, 3), (48, 100, 2),
                                                      (41, 7, 1), (41, 1, 1), (1, 1, 2), (2, 1, 2), (130, 64, 2), (129, 64, 3), (1000, 16, 7), (10, 3, 64)])
def test_bands_and_halo_rows_against_a_restatement(height, band_rows, n_parts):
    owners, total_halo = np.full(height, -1), 0
    for part in range(n_parts):
        ok, rows, halo = _diag(height, band_rows, n_parts, part)
        want_rows, want_halo = _bands(height, band_rows, n_parts, part)
        assert ok == 1 and rows == want_rows and halo == want_halo, (part, rows, halo, want_rows, want_halo)
        assert all(0 <= y < height and y not in want_rows for y in halo)  # rows of the frame, other parts' rows
        assert len(halo) <= 2 * max(1, len(range(part, (height + band_rows - 1) // band_rows, n_parts)))
        owners[rows] = part
        total_halo += len(halo)
    assert (owners >= 0).all()
    if n_parts == 1 or band_rows >= height:
        assert total_halo == 0  # one part, or one band: nothing across an edge
    else:
        assert total_halo == 2 * ((height + band_rows - 1) // band_rows - 1)  # every inner edge, from both sides


def test_bands_named_cases():
    # a part that owns no row
    assert _diag(10, 64, 3, 1) == (1, [], []) and _diag(10, 3, 64, 40) == (1, [], [])
    # a band edge at row H - 1: the frame's black last row is a halo row, and the last band's only halo row is H - 2
    assert _diag(31, 5, 2, 1)[2][-1] == 30 and _diag(31, 5, 2, 0)[1][-1] == 30 and _diag(31, 5, 2, 0)[2][-1] == 29
    # defaults (band_rows 0 -> 64, n_parts 0 -> 1), and what is no part
    assert _diag(100, 0, 0, 0) == (1, list(range(100)), [])
    assert _diag(100, 0, 2, 1) == (1, list(range(64, 100)), [63])
    assert _diag(100, 7, 2, 2)[0] == 0 and _diag(0, 7, 2, 0)[0] == 0
    # the caps are kept
    rows, halo, counts = (C.c_uint32 * 4)(), (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
    assert P.lib().rtc_diag_adaptive_bands(31, 1, 2, 1, rows, 3, halo, 1, counts) == 1 and list(counts) == [15, 30]
    assert list(rows) == [1, 3, 5, 0] and list(halo) == [0, 0]


# ---- 5. the seam's adaptive kernels in the plan ---------------------------------------------------------------------------
@pytest.fixture
def _library_defaults(monkeypatch):
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)


def _plan_lines(world, camera):
    cs = world._c()
    text, digests = C.create_string_buffer(1 << 16), (C.c_uint64 * 4)()
    L.check(P.lib().rtc_diag_scene_plan(C.byref(cs.scene), C.byref(camera._cam), text, len(text), digests))
    return text.value.decode().splitlines()


@pytest.mark.parametrize("name", ["reflect_refract", "soft_shadows", "mesh"])
def test_the_seams_adaptive_kernels_are_planned_by_the_formula(name, _library_defaults):
    world, camera, _ = getattr(scenes, name)(64, 48)
    plan = world.scene_plan(camera)[1]
    core = source_hash("rtc_kernel_core.h")
    tail = "hiprtc %s abi 8 args %s\n" % (plan["hiprtc"], plan["render_args"])
    own = source_hash("rtc_adaptive_seam.h", source_hash("rtc_adaptive.h", core))
    trace_defs = plan["trace_spec_defs"].split()
    assert trace_defs[-1] == "-DRTC_SPEC_TRACE=1"
    seen = set()
    for k in (1, 2, 4):
        seam = "adaptive_seam%d_" % k
        tag = ";halo" if k == 1 else ";ss=%d" % k
        assert plan[seam + "entry"] == "adaptive_seam_kernel_spec"
        assert (plan[seam + "header"], plan[seam + "header_below"]) == ("rtc_adaptive_seam.h", "rtc_adaptive.h") and seam + "header_below2" not in plan
        # names: a ray stream's, renamed, with the factor (or "halo") last
        assert plan[seam + "family_name"] == plan["trace_family_name"].replace("trace_kernel<", "adaptive_seam_kernel<")[:-1] + tag + ">"
        assert plan[seam + "spec_name"] == plan["trace_spec_name"].replace("trace_kernel_spec[", "adaptive_seam_kernel_spec[")[:-1] + tag + "]"
        # options: a ray stream's with the kind's own option in the place of its last
        defs = plan[seam + "spec_defs"].split()
        assert defs == trace_defs[:-1] + ["-DRTC_SPEC_ADAPTIVE_SEAM=%d" % k]
        assert "-DRTC_SPEC_SHARE=0" in defs and not any(d.startswith(("-DRTC_SPEC_ADAPTIVE=", "-DRTC_SPEC_SS")) for d in defs)
        options = FIXED + defs + ([] if any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in defs) else ["-DRTC_WAVES_PER_SIMD=7"])
        assert plan[seam + "options"].split() == options
        # the cache file and the ahead-of-time id: two headers' bytes behind the key, rtc_adaptive.h and then rtc_adaptive_seam.h
        key = "".join(o + "\n" for o in options) + tail + "adaptive seam args %s\n" % plan[seam + "args"]
        assert plan[seam + "cache_file"] == "spec_%016x.hsaco" % source_hash("rtc_adaptive_seam.h", source_hash("rtc_adaptive.h", fnv1a(key.encode(), core)))
        assert plan[seam + "aot_id"] == "aot_adaptive_seam%d_%016x" % (k, own)
        seen |= {plan[seam + "cache_file"], plan[seam + "aot_id"]}
    assert len(seen) == 6
    # the persistent context's refinement kernels keep theirs, by the formula they had
    for k in (2, 4):
        old = "adaptive%d_" % k
        assert plan[old + "aot_id"] == "aot_adaptive%d_%016x" % (k, source_hash("rtc_adaptive.h", core)) and plan[old + "aot_id"] not in seen
        assert plan[old + "spec_defs"].split() == trace_defs[:-1] + ["-DRTC_SPEC_ADAPTIVE=%d" % k] and plan[old + "cache_file"] not in seen
    assert plan["aot_id"] == "aot_%016x" % core


def test_every_earlier_entry_keeps_its_bytes(_library_defaults):
    """The plan's text without its adaptive_seam<k>_ lines is, line by line, what the commit before printed -- for five scenes.
    (The ray-stream kernel's own five lines -- trace_args, trace_cache_file, trace_aot_id, trace_deep16_ / trace_deep32_cache_file --
    stand in the stored text as they are since rtc_trace.h's per-ray guard of the flat hierarchy gave TraceArgs its StreamGuard;
    every other kernel's lines, the render kernels' ids among them, are still that commit's.)"""
    with open(os.path.join(ROOT, "tests", "golden", "scene_plan_before_adaptive_seam.json")) as f:
        golden = json.load(f)
    assert len(golden["plans"]) == 5
    for name, before in golden["plans"].items():
        world, camera, _ = getattr(scenes, name)(*golden["size"])
        lines = _plan_lines(world, camera)
        new = [i for i, ln in enumerate(lines) if ln.startswith("adaptive_seam")]
        assert len(new) == 3 * len(PER_KERNEL) and new == list(range(new[0], new[0] + len(new))), (name, new)  # one run
        assert [ln.split("=", 1)[0] for ln in lines[new[0]:new[-1] + 1]] == ["adaptive_seam%d_%s" % (k, what) for k in (1, 2, 4) for what in PER_KERNEL]
        # ... in front of the seam's lens kernels, the only entries behind it (tests/test_seam_lens_boundary.py pins those as the last)
        assert all(ln.startswith(("lens2_seam_", "lens4_seam_")) for ln in lines[new[-1] + 1:]) and lines[new[0] - 1].startswith("lens4_args=")
        assert lines[:new[0]] + lines[new[-1] + 1:] == before, name
