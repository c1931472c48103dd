"""The limits on a rectangle light's grid, enforced on the host (no GPU needed).

RTC_LIGHT_CELLS_MAX (include/rtc.h): u_steps x v_steps <= 2^24.  rectangle_light.rs:76-88 adds 1.0 per lit sample in f32, and an
f32 sum of ones stops at 2^24, so above it the reference itself answers a fully lit point with 2^24 / cells -- pinned below on the
oracle, which restates the reference and keeps accepting such lights.  None of the library's ways of answering samples
without tracing them reproduces that, so rtc_rectangle_light, pack_light (every call that takes a scene) and rtc_scene_validate
refuse such a light, with the product formed in 64 bits.

The packed work counter (rtc_kernel_core.h Counters, rtc_launch_plan.h culled_count_fits): the rule by which a launch either
counts its culled shadow rays exactly or runs with the culls off, at its boundaries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import _lib as L
from tests import helpers as H

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = [(4096, 4096), (1, 1 << 24), (1 << 24, 1)]
REFUSED = [(4096, 4097), (4097, 4096), (65536, 65536), (46341, 46341), (2 ** 31 - 1, 2 ** 31 - 1), (1, (1 << 24) + 1)]


def _c_light(u_steps, v_steps):
    light = L.rtc_light()
    args = [np.array(v, dtype=f32) for v in ((1, 1, 1), (-1, 4, -1, 1), (2, 0, 0, 0), (0, 0, 2, 0))]
    st = L.lib().rtc_rectangle_light(args[0].ctypes.data_as(L.FP), args[1].ctypes.data_as(L.FP), args[2].ctypes.data_as(L.FP), u_steps,
                                     args[3].ctypes.data_as(L.FP), v_steps, L.RTC_JITTER_HASHED, 0.0, 7, C.byref(light))
    return st, light


def _world(u_steps, v_steps):
    floor = P.Plane(None, P.Material(specular=0.0), casts_shadow=False)
    return P.World([floor], P.RectangleLight(P.color(1, 1, 1), P.point(-1, 4, -1), P.vector(2, 0, 0), u_steps, P.vector(0, 0, 2), v_steps, ("hashed", 7)))


def _camera():
    return P.Camera(8, 8, 1.0, P.view_transform(P.point(0, 3, -6), P.point(0, 0, 0), P.vector(0, 1, 0)))


def test_the_limit_is_a_constant_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert "#define RTC_LIGHT_CELLS_MAX %d" % L.RTC_LIGHT_CELLS_MAX in hdr
    assert L.RTC_LIGHT_CELLS_MAX == 2 ** 24
    assert "#define RTC_JITTER_SEQUENCE_MAX %d" % L.RTC_JITTER_SEQUENCE_MAX in hdr


@pytest.mark.parametrize("steps", ACCEPTED)
def test_lights_of_up_to_2_to_the_24_cells_are_accepted(steps):
    st, light = _c_light(*steps)
    assert st == L.RTC_OK and (light.u_steps, light.v_steps) == steps
    world = _world(*steps)
    world.validate()
    world.validate(_camera())
    world.scene_plan(_camera())


@pytest.mark.parametrize("steps", REFUSED)
def test_larger_lights_are_refused_by_all_three_entry_points(steps):
    # 1. rtc_rectangle_light
    st, _ = _c_light(*steps)
    assert st == L.RTC_ERR_UNSUPPORTED, (steps, st)
    msg = L.lib().rtc_last_error().decode()
    assert "RTC_LIGHT_CELLS_MAX" in msg and str(2 ** 24) in msg, msg
    # 2. pack_light and 3. rtc_scene_validate, given a light that did not come from rtc_rectangle_light: a valid one with the
    # step counts written into the struct, as a C caller filling rtc_light by hand would
    cs = _world(2, 2)._c()
    cam = _camera()
    assert L.lib().rtc_scene_validate(C.byref(cs.scene), C.byref(cam._cam)) == L.RTC_OK
    cs.light.u_steps, cs.light.v_steps = steps
    for camera in (C.byref(cam._cam), None):
        assert L.lib().rtc_scene_validate(C.byref(cs.scene), camera) == L.RTC_ERR_UNSUPPORTED, steps
        msg = L.lib().rtc_last_error().decode()
        assert "RTC_LIGHT_CELLS_MAX" in msg and str(2 ** 24) in msg, msg
    text, digests = C.create_string_buffer(1 << 16), (C.c_uint64 * 4)()  # (pack_light through another door: the scene's plan)
    assert L.lib().rtc_diag_scene_plan(C.byref(cs.scene), C.byref(cam._cam), text, len(text), digests) == L.RTC_ERR_UNSUPPORTED
    # the batched entry points flatten the scene too; without a GPU the missing device is reported first
    out, pt = np.zeros(1, dtype=f32), P.point(0, 1e-3, 0).reshape(1, 4)
    assert L.lib().rtc_intensity_at(C.byref(cs.scene), pt.ctypes.data_as(L.FP), 1, 0, out.ctypes.data_as(L.FP)) in (L.RTC_ERR_UNSUPPORTED, L.RTC_ERR_NO_DEVICE)


def test_zero_and_negative_steps_are_still_invalid_arguments():
    for steps in ((0, 4), (4, 0), (-1, -1), (-65536, -65536)):
        st, _ = _c_light(*steps)
        assert st == L.RTC_ERR_INVALID_ARG, steps


@pytest.mark.parametrize("steps", [(4096, 4097), (65536, 65536)])
def test_the_python_light_surfaces_the_error(steps):
    world = _world(*steps)
    with pytest.raises(P.RtcError) as e:
        world.light._c()
    assert e.value.status == L.RTC_ERR_UNSUPPORTED and "RTC_LIGHT_CELLS_MAX" in str(e.value)
    with pytest.raises(P.RtcError) as e:
        world.validate(_camera())
    assert e.value.status == L.RTC_ERR_UNSUPPORTED
    with pytest.raises(P.RtcError) as e:
        world.light.position
    assert e.value.status == L.RTC_ERR_UNSUPPORTED


CPP = r"""
#include <cstdio>
#include "rtc.hpp"
int main() {
    const rtc::Color white = rtc::color(1.0f, 1.0f, 1.0f);
    rtc::RectangleLight ok(white, rtc::point(-1, 4, -1), rtc::vector(2, 0, 0), 4096, rtc::vector(0, 0, 2), 4096);
    std::printf("accepted %d x %d\n", ok.l.u_steps, ok.l.v_steps);
    const int refused[2][2] = {{4096, 4097}, {65536, 65536}};
    for (const auto& s : refused) {
        try {
            rtc::RectangleLight bad(white, rtc::point(-1, 4, -1), rtc::vector(2, 0, 0), s[0], rtc::vector(0, 0, 2), s[1]);
            std::printf("NOT refused %d x %d\n", s[0], s[1]);
            return 1;
        } catch (const rtc::Error& e) {
            std::printf("refused %d x %d: status %d: %s\n", s[0], s[1], e.status, e.what());
            if (e.status != RTC_ERR_UNSUPPORTED) return 2;
        }
    }
    static_assert(RTC_LIGHT_CELLS_MAX == 16777216, "the limit of include/rtc.h");
    return 0;
}
"""


def test_the_cpp_mirror_surfaces_the_error(tmp_path):
    (tmp_path / "limit.cpp").write_text(CPP)
    libdir = os.path.dirname(L.LIB_PATH)
    exe = str(tmp_path / "limit")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "limit.cpp"),
                           "-L" + libdir, "-lrtc_amd", "-Wl,-rpath," + libdir])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "accepted 4096 x 4096" in p.stdout
    assert p.stdout.count("refused") == 2 and "NOT refused" not in p.stdout and "RTC_LIGHT_CELLS_MAX" in p.stdout, p.stdout


def test_the_reason_above_2_to_the_24_cells_the_references_own_sum_saturates():
    """Oracle only: a casterless world under a 4096 x 4097 light.  Every one of the 16 781 312 samples is lit, the f32 sum of
    ones stops at 2^24, and intensity_at is 2^24 / cells -- not the 1.0 every shortcut of the library would give."""
    cells = 4096 * 4097
    own = H.oracle_world(_world(4096, 4097))
    own.set_pixel(3)
    got = own.intensity_at(P.point(0.25, 1e-3, 0.5))
    assert got == f32(2 ** 24) / f32(cells), got
    assert got < f32(1.0)
    # ... and at the limit itself the sum is still exact
    own = H.oracle_world(_world(4096, 4096))
    own.set_pixel(3)
    assert own.intensity_at(P.point(0.25, 1e-3, 0.5)) == f32(1.0)


# ---------------------------------------------------------------- the packed counter's capacity
def _fits(u, v, depth, refl, refr, rays_per_lane=1):
    return bool(L.lib().rtc_diag_culled_count_fits(u, v, depth, int(refl), int(refr), rays_per_lane))


def test_culled_count_capacity_rule():
    """cells x (shade points one lane can make) <= 2^20 - 1, the shade points being 1 / depth + 1 / 2^(depth + 1) - 1 per ray for
    worlds that do not recurse / reflect or transmit / do both, times the rays a lane traces, and never more than the 4 095
    the shade-point field itself holds."""
    cap = 2 ** 20 - 1
    # a world that does not recurse: one shade point per ray whatever the depth -- 1023 x 1025 = 2^20 - 1 is the largest light
    for depth in (0, 5, 8):
        assert _fits(1023, 1025, depth, False, False) and _fits(1, cap, depth, False, False)
        assert not _fits(1024, 1024, depth, False, False) and not _fits(1, cap + 1, depth, False, False)
    # mirrors only (or glass only): a chain of depth + 1 shade points
    for refl, refr in ((True, False), (False, True)):
        assert _fits(1, 131071, 7, refl, refr) and not _fits(512, 256, 7, refl, refr)   # 8 x 2^17 = 2^20
        assert _fits(512, 256, 6, refl, refr)                                           # 7 x 2^17
        assert _fits(1, cap // 9, 8, refl, refr) and not _fits(1, cap // 9 + 1, 8, refl, refr)
    # both: a binary tree, 2^(depth + 1) - 1; depth 5 (the reference's default): 63
    assert _fits(1, cap // 63, 5, True, True) and not _fits(1, cap // 63 + 1, 5, True, True)
    assert _fits(129, 129, 5, True, True) and not _fits(129, 130, 5, True, True)        # 16 641 / 16 770 cells against 16 644
    assert _fits(1, cap // 511, 8, True, True) and not _fits(1, cap // 511 + 1, 8, True, True)
    # several rays per lane (blocks per workgroup), capped by what the shade-point field holds
    assert _fits(1, cap // 4, 3, False, False, 4) and not _fits(1, cap // 4 + 1, 3, False, False, 4)
    assert _fits(16, 16, 8, True, True, 8) and not _fits(1, 257, 8, True, True, 9)      # 4 095 x 256 fits, 4 095 x 257 does not
    assert _fits(1, 256, 8, True, True, 2 ** 31)
    # what the suite and the demos use -- 100 cells at depth 5 -- is far inside
    assert _fits(10, 10, 8, True, True, 8)
