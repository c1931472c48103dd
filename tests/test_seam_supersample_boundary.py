"""rtc_render_ss without a device: the one-call seam's supersampled entry point answers its argument errors on the host, before
any device call and in the order rtc_render_ex checks its arguments; and the arithmetic that turns a reporting launch's chunks
of fine block rows into chunks of OUTPUT rows (csrc/rtc_launch_plan.h plan_ss_chunks / chunk_output_rows, through
rtc_diag_ss_chunks) cuts every partition into whole output rows."""
import ctypes as C

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes

f32 = np.float32


def _call(lib, cs, cam, depth, k, out):
    st = L.rtc_stats()
    rc = lib.rtc_render_ss(C.byref(cs.scene), C.byref(cam) if cam is not None else None, depth, k, None,
                           out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(st))
    return rc, lib.rtc_last_error().decode()


def test_render_ss_argument_errors_are_decided_on_the_host():
    world, camera, depth = scenes.single_sphere(32, 32)
    cs, lib = world._c(), P.lib()
    out = np.zeros((32, 32, 3), dtype=f32)
    # null `out`, null camera: whatever k is
    for k in (1, 2, 4, 3):
        assert _call(lib, cs, camera._cam, depth, k, None)[0] == L.RTC_ERR_INVALID_ARG
        assert _call(lib, cs, None, depth, k, out)[0] == L.RTC_ERR_INVALID_ARG
    # a factor that is not 1, 2 or 4: INVALID_ARG (not NO_DEVICE on a machine without one), the factor named
    for k in (0, 3, 8):
        rc, msg = _call(lib, cs, camera._cam, depth, k, out)
        assert rc == L.RTC_ERR_INVALID_ARG, (k, rc, msg)
        assert "factor %d" % k in msg, msg
    # a fine frame beyond 2^32 pixels (40000^2 x 16) or 2^17 rows (8 x 40000 x 4): refused with the factor named
    for w, h, k in ((40000, 40000, 4), (8, 40000, 4), (8, 70000, 2)):
        big = L.rtc_camera()
        L.check(lib.rtc_camera_new(w, h, f32(0.9), camera.transform.ctypes.data_as(L.FP), C.byref(big)))
        one = np.zeros(3, dtype=f32)  # never written: the call is refused before anything is
        rc, msg = _call(lib, cs, big, depth, k, one)
        assert rc == L.RTC_ERR_INVALID_ARG, (w, h, k, rc, msg)
        assert "by %d" % k in msg and "%d x %d" % (w, h) in msg, msg
        assert not one.any()
    # k = 1 is rtc_render_ex: with valid arguments and no device it says so (and k = 2, 4 likewise: nothing else was wrong)
    if lib.rtc_device_count() == 0:
        for k in (1, 2, 4):
            assert _call(lib, cs, camera._cam, depth, k, out)[0] == L.RTC_ERR_NO_DEVICE
    lib.rtc_render_release()


def test_python_surface_refuses_other_factors():
    world, camera, depth = scenes.single_sphere(16, 16)
    for k in (0, 3, 8):
        with pytest.raises(ValueError):
            camera.render(world, depth, supersample=k)


def _cap(k):
    return 2 if k == 4 else 4  # rtc_launch_plan.h ss_max_share_log2


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("width", [17, 64, 1000])
def test_chunks_of_a_supersampled_launch_are_whole_output_rows(width, k):
    lib = P.lib()
    out = (C.c_uint32 * 8)()
    for rows in (1, 7, 66, 1536):
        for s in range(_cap(k) + 1):
            for swizzle in (0, 1):
                for want in (1, 3, 24, 200):
                    whole = lib.rtc_diag_ss_chunks(width, rows, k, s, swizzle, want, out)
                    grid_x, grid_y, block_h, cbr, n_chunks, chunk_rows, planned_s, max_chunks = list(out)
                    what = (width, rows, k, s, swizzle, want, list(out))
                    assert planned_s == s and max_chunks == 64, what
                    # the fine grid: blocks of 16 >> ceil(s / 2) fine rows, 16 >> floor(s / 2) fine columns
                    assert block_h == 16 >> ((s + 1) >> 1) and block_h % k == 0, what
                    gy = -(-rows * k // block_h)
                    gx = -(-width * k // (16 >> (s >> 1)))
                    assert (grid_x, grid_y) == (((gx + 1) & ~1, (gy + 3) & ~3) if swizzle else (gx, gy)), what
                    # a chunk is a whole number of output rows
                    assert whole == 1 and cbr * block_h == chunk_rows * k and chunk_rows >= 1, what
                    # no more chunks than there are words, no more than asked for
                    assert 1 <= n_chunks <= min(max_chunks, max(want, 1)), what
                    # swizzled grids finish block rows four at a time: chunks start at multiples of four block rows
                    if swizzle:
                        assert cbr % 4 == 0, what
                    # chunk j = output rows [j * chunk_rows, min(rows, (j + 1) * chunk_rows)): the chunks tile [0, rows) without a gap
                    # or an overlap, none of them empty, and the counters' chunks are the same ones (every block row in one chunk)
                    edges = [min(rows, j * chunk_rows) for j in range(n_chunks + 1)]
                    assert edges[0] == 0 and edges[-1] == rows and all(a < b for a, b in zip(edges, edges[1:])), what
                    assert (n_chunks - 1) * cbr < grid_y <= n_chunks * cbr, what
                    # every fine row of output row y lies in block rows of y's chunk
                    for j in range(n_chunks):
                        y0, y1 = edges[j], edges[j + 1]
                        assert (y0 * k) // block_h // cbr == j and ((y1 * k - 1) // block_h) // cbr == j, what


def test_a_factor_of_zero_is_answered_not_divided_by():
    out = (C.c_uint32 * 8)()
    assert P.lib().rtc_diag_ss_chunks(64, 66, 0, 0, 1, 24, out) == 0 and out[5] == 0


def test_lanes_per_pixel_are_capped_before_the_chunks_are_cut():
    """k = 4 with eight or sixteen lanes per pixel asked for is planned with four (8 x 4 tiles: blocks of 8 fine rows, two output rows)."""
    lib = P.lib()
    out = (C.c_uint32 * 8)()
    for s in (3, 4):
        assert lib.rtc_diag_ss_chunks(64, 66, 4, s, 1, 24, out) == 1
        assert out[6] == 2 and out[2] == 8
    assert lib.rtc_diag_ss_chunks(64, 66, 2, 4, 1, 24, out) == 1
    assert out[6] == 4 and out[2] == 4
