"""CPU-only checks of supersampled rendering's boundary (rtc_camera_supersampled, rtc_ctx_set_scene_ss): the symbols exist and
are declared, the ABI version has not moved, the fine camera is Camera::new(k W, k H, fov, T) bit for bit, argument errors are
decided on the host, the lanes-per-pixel cap keeps a k x k group inside one wave's tile, and the numpy reference filter
(tests/supersample_helpers.py) adds in the contract's order."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import renderer as R
from tests.supersample_helpers import assemble_partitions, box_filter

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_exist_and_are_declared():
    raw = C.CDLL(L.LIB_PATH)
    for name in ("rtc_camera_supersampled", "rtc_ctx_set_scene_ss"):
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert getattr(P.lib(), name).restype is C.c_int
    assert hasattr(raw, "rtc_diag_ss_plan") and "rtc_diag_ss_plan" in L.EXTRA
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert "rtc_status rtc_camera_supersampled(const rtc_camera* camera, uint32_t k, rtc_camera* fine);" in header
    assert "rtc_status rtc_ctx_set_scene_ss(rtc_ctx* ctx, const rtc_scene* scene, const rtc_camera* output_camera, uint32_t k);" in header
    assert "#define RTC_ABI_VERSION 8" in header
    assert P.lib().rtc_abi_version() == 8
    assert "supersample" in inspect.signature(R.Renderer.__init__).parameters
    assert "supersample" in inspect.signature(R.Renderer.set_scene).parameters


def _transforms():
    ident = np.eye(4, dtype=f32)
    moved = P.view_transform(P.point(-2.6, 1.5, -3.9), P.point(-0.6, 1, -0.8), P.vector(0, 1, 0))
    rotated = (P.rotation_z(0.7) @ P.rotation_x(-0.3) @ P.translation(1.5, -2.25, 7.0)).astype(f32)
    return {"identity": ident, "view": np.asarray(moved, dtype=f32), "rotated+translated": rotated}


SIZES = [(1001, 333), (333, 1001), (125, 200), (201, 101), (64, 64), (7, 7), (1, 1), (400, 200), (200, 400), (4096, 4096), (3, 1000)]


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("size", SIZES)
def test_the_fine_camera_is_camera_new_at_k_times_the_size(k, size):
    lib = P.lib()
    w, h = size
    for name, t in _transforms().items():
        for fov in (math.pi / 3, 0.45, 1.2, 2.5):
            t = np.ascontiguousarray(t, dtype=f32)
            out_cam, want, got = L.rtc_camera(), L.rtc_camera(), L.rtc_camera()
            assert lib.rtc_camera_new(w, h, fov, t.ctypes.data_as(L.FP), C.byref(out_cam)) == L.RTC_OK
            assert lib.rtc_camera_new(k * w, k * h, fov, t.ctypes.data_as(L.FP), C.byref(want)) == L.RTC_OK
            assert lib.rtc_camera_supersampled(C.byref(out_cam), k, C.byref(got)) == L.RTC_OK, lib.rtc_last_error()
            assert bytes(got) == bytes(want), (name, fov, size, k)
            # the aspect branch and the half extents are the output camera's, bit for bit; only the pixel is smaller
            assert f32(got.half_width).tobytes() == f32(out_cam.half_width).tobytes()
            assert f32(got.half_height).tobytes() == f32(out_cam.half_height).tobytes()
            assert list(got.inv) == list(out_cam.inv)
            assert f32(got.pixel_size) == f32(f32(f32(got.half_width) * f32(2.0)) / f32(k * w))


def test_factor_one_is_the_camera_itself_and_the_python_camera_follows():
    cam = P.Camera(125, 200, math.pi / 3, _transforms()["view"])
    same = cam.supersampled(1)
    assert bytes(same._cam) == bytes(cam._cam)
    fine = cam.supersampled(4)
    ref = P.Camera(500, 800, math.pi / 3, _transforms()["view"])
    assert bytes(fine._cam) == bytes(ref._cam)
    assert (fine.width, fine.height) == (500, 800) and fine.field_of_view == cam.field_of_view
    assert (fine.transform == cam.transform).all()


def _camera(w, h):
    cam = L.rtc_camera()
    t = np.eye(4, dtype=f32)
    assert P.lib().rtc_camera_new(w, h, 1.0, t.ctypes.data_as(L.FP), C.byref(cam)) == L.RTC_OK
    return cam


@pytest.mark.parametrize("k", [0, 3, 5, 8])
def test_other_factors_are_invalid_arguments(k):
    lib = P.lib()
    cam, fine = _camera(100, 50), L.rtc_camera()
    assert lib.rtc_camera_supersampled(C.byref(cam), k, C.byref(fine)) == L.RTC_ERR_INVALID_ARG
    assert b"factor %d" % k in lib.rtc_last_error()
    with pytest.raises(P.RtcError) as e:
        P.Camera(100, 50, 1.0, np.eye(4, dtype=f32)).supersampled(k)
    assert e.value.status == L.RTC_ERR_INVALID_ARG


@pytest.mark.parametrize("size,k", [((40000, 40000), 4), ((65536, 20000), 4), ((50000, 50000), 2), ((10, 32768), 4), ((10, 65536), 2)])
def test_an_oversize_fine_frame_is_an_invalid_argument(size, k):
    lib = P.lib()
    cam, fine = _camera(*size), L.rtc_camera()
    assert lib.rtc_camera_supersampled(C.byref(cam), k, C.byref(fine)) == L.RTC_ERR_INVALID_ARG
    assert b"exceeds" in lib.rtc_last_error()
    # ... and the largest frames that fit are accepted: local rows below 2^17, the pixel index in 32 bits
    ok = _camera(10, (1 << 17) // k - 1)
    assert lib.rtc_camera_supersampled(C.byref(ok), k, C.byref(fine)) == L.RTC_OK
    assert fine.height == k * ok.height < (1 << 17)


def test_set_scene_ss_argument_errors_come_before_any_device_call():
    lib = P.lib()
    cs = P.default_world()._c()
    cam = _camera(100, 50)
    for k in (0, 3, 5, 8):  # the factor is checked first: no context is needed to learn that it is wrong
        assert lib.rtc_ctx_set_scene_ss(None, C.byref(cs.scene), C.byref(cam), k) == L.RTC_ERR_INVALID_ARG
        assert b"factor %d" % k in lib.rtc_last_error()
    big = _camera(40000, 40000)
    assert lib.rtc_ctx_set_scene_ss(None, C.byref(cs.scene), C.byref(big), 4) == L.RTC_ERR_INVALID_ARG
    assert b"exceeds" in lib.rtc_last_error()
    assert lib.rtc_ctx_set_scene_ss(None, C.byref(cs.scene), None, 2) == L.RTC_ERR_INVALID_ARG
    assert lib.rtc_last_error() != b""
    for k in (1, 2, 4):  # a good factor, no context
        assert lib.rtc_ctx_set_scene_ss(None, C.byref(cs.scene), C.byref(cam), k) == L.RTC_ERR_INVALID_ARG
        assert b"ctx is NULL" in lib.rtc_last_error()


# ---- the lanes-per-pixel cap -------------------------------------------------------------------------------------------
def _tile_dims(s):  # a wave's tile at 2^s lanes per pixel: 8 x 8, 8 x 4, 4 x 4, 4 x 2, 2 x 2
    return 8 >> (s >> 1), 8 >> ((s + 1) >> 1)


def _block_dims(s):  # a workgroup's block: 2 x 2 wave tiles
    w, h = _tile_dims(s)
    return 2 * w, 2 * h


def _tile_word(s, x0, y0):
    return (s & 3) << 30 | (x0 // 4) << 16 | (s >> 2) << 15 | (y0 // 4)


def _decode(t):
    return (t >> 30) | ((t >> 13) & 4), ((t >> 16) & 0x3FFF) << 2, (t & 0x7FFF) << 2


def _ss_plan(k, s, list_=None, ticks=None, width=0, rows=0, wave_slots=1.0):
    lib = P.lib()
    cap = 1 << 16
    out = (C.c_uint32 * cap)()
    n_out = C.c_uint32(0)
    if list_ is None:
        got = lib.rtc_diag_ss_plan(k, s, None, None, 0, width, rows, wave_slots, out, cap, C.byref(n_out))
    else:
        la, ta = (C.c_uint32 * len(list_))(*list_), (C.c_uint32 * len(ticks))(*ticks)
        got = lib.rtc_diag_ss_plan(k, s, la, ta, len(list_), width, rows, wave_slots, out, cap, C.byref(n_out))
    assert n_out.value <= cap
    return got, [out[i] for i in range(n_out.value)]


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_the_planned_lanes_per_pixel_never_split_a_group_across_waves(k, s):
    width, rows = 96 * k, 40 * k  # (a fine frame: multiples of k)
    planned, blocks = _ss_plan(k, s, width=width, rows=rows)
    assert planned == (min(s, 2) if k == 4 else s)
    tw, th = _tile_dims(planned)
    assert tw % k == 0 and th % k == 0, (k, s, planned, tw, th)
    # the uniform list such a frame starts from: every block at the capped count, at origins that keep groups whole, covering the frame
    bw, bh = _block_dims(planned)
    covered = np.zeros((rows, width), dtype=np.int32)
    for t in blocks:
        bs, x0, y0 = _decode(t)
        assert bs == planned and x0 % k == 0 and y0 % k == 0 and x0 % tw == 0 and y0 % th == 0
        covered[y0:y0 + bh, x0:x0 + bw] += 1
    assert (covered == 1).all()


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("s_in", [3, 4])
@pytest.mark.parametrize("pressure", ["waves far too long", "waves far too short"])
def test_a_block_list_with_more_lanes_than_the_cap_comes_back_capped(k, s_in, pressure):
    width, rows = 64, 48
    bw, bh = _block_dims(s_in)
    list_ = [_tile_word(s_in, x0, y0) for y0 in range(0, rows, bh) for x0 in range(0, width, bw)]
    ticks = [1000 + (i % 7) for i in range(4 * len(list_))]
    # few wave slots: the frame's throughput time dwarfs every wave, the feedback wants fewer lanes; many: it wants more
    slots = 1e9 if pressure == "waves far too long" else 1e-3
    _, out = _ss_plan(k, s_in, list_, ticks, width, rows, slots)
    cap = 2 if k == 4 else 4
    covered = np.zeros((rows, width), dtype=np.int32)
    for t in out:
        s, x0, y0 = _decode(t)
        assert s <= cap, (s, cap)
        tw, th = _tile_dims(s)
        assert tw % k == 0 and th % k == 0
        w, h = _block_dims(s)
        covered[y0:y0 + h, x0:x0 + w] += 1
    assert (covered == 1).all()
    if pressure == "waves far too long":
        assert all(_decode(t)[0] == cap for t in out)  # as many lanes as the cap allows, and no more


# ---- the numpy reference filter ----------------------------------------------------------------------------------------
BIG, EVEN = f32(1e8), f32(16777216.0)  # ulp(1e8) = 8, ulp(2^24) = 2: adding 1 to either changes nothing


def test_box_filter_factor_two_is_pinned_by_hand():
    F = np.zeros((4, 4, 3), dtype=f32)
    # block (0, 0): (1e8 + 1) + (-1e8 + 1) = 1e8 + -1e8 = 0; y first would give (1e8 + -1e8) + (1 + 1) = 2, sequential 1
    F[0:2, 0:2, 0] = [[BIG, 1], [-BIG, 1]]
    # block (1, 0): (2^24 + 1) + (1 + 1) = 2^24 + 2; sequential ((2^24 + 1) + 1) + 1 = 2^24
    F[0:2, 2:4, 0] = [[EVEN, 1], [1, 1]]
    F[2:4, 0:2, 0] = [[1, 2], [3, 4]]          # 10 / 4
    F[2:4, 2:4, 0] = [[0.5, 0.25], [0.125, 0]]  # 0.875 / 4
    F[..., 1] = 1.0
    F[..., 2] = np.arange(16, dtype=f32).reshape(4, 4)
    got = box_filter(F, 2)
    assert got.dtype == f32 and got.shape == (2, 2, 3)
    assert got[..., 0].tolist() == [[0.0, 4194304.5], [2.5, 0.21875]]
    assert got[..., 1].tolist() == [[1.0, 1.0], [1.0, 1.0]]
    assert got[..., 2].tolist() == [[2.5, 4.5], [10.5, 12.5]]
    # the case distinguishes orders on this CPU: the same four values added another way give other bits
    a, b, c, d = F[0, 0, 0], F[0, 1, 0], F[1, 0, 0], F[1, 1, 0]
    assert f32(f32(a + b) + f32(c + d)) * f32(0.25) == f32(0.0)
    assert f32(f32(a + c) + f32(b + d)) * f32(0.25) == f32(0.5)          # along y first
    assert f32(f32(f32(a + b) + c) + d) * f32(0.25) == f32(0.25)         # sequential
    a, b, c, d = F[0, 2, 0], F[0, 3, 0], F[1, 2, 0], F[1, 3, 0]
    assert f32(f32(f32(a + b) + c) + d) * f32(0.25) == f32(4194304.0)    # sequential: one ulp-pair lost


def test_box_filter_factor_four_is_pinned_by_hand():
    F = np.zeros((4, 4, 3), dtype=f32)
    F[..., 0] = [[BIG, 1, -BIG, 1],     # (1e8 + 1) + (-1e8 + 1) = 0       (sequential: 1)
                 [1, 1, 1, 1],          # 4
                 [EVEN, 1, 1, 1],       # (2^24 + 1) + (1 + 1) = 2^24 + 2  (sequential: 2^24)
                 [-EVEN, 0, 0, 0]]      # -2^24
    F[..., 1] = 0.5
    F[..., 2] = np.arange(16, dtype=f32).reshape(4, 4)
    got = box_filter(F, 4)
    assert got.dtype == f32 and got.shape == (1, 1, 3)
    # (0 + 4) + ((2^24 + 2) + -2^24) = 4 + 2 = 6; 6 / 16
    assert got[0, 0].tolist() == [0.375, 0.5, 7.5]
    ch = F[..., 0]
    # along y first: columns (1e8 + 1) + (2^24 - 2^24) = 1e8, 3, -1e8, 3; (1e8 + 3) + (-1e8 + 3) = 0
    cols = [f32(f32(ch[0, x] + ch[1, x]) + f32(ch[2, x] + ch[3, x])) for x in range(4)]
    assert f32(f32(cols[0] + cols[1]) + f32(cols[2] + cols[3])) * f32(0.0625) == f32(0.0)
    # sequential, row by row: ((((1e8 + 1) + -1e8) + 1) ... loses other bits
    acc = f32(0.0)
    for v in ch.reshape(-1):
        acc = f32(acc + v)
    assert f32(acc * f32(0.0625)) != got[0, 0, 0]


def test_box_filter_blocks_are_independent_and_factor_one_is_the_frame():
    rng = np.random.default_rng(7)
    F = (rng.standard_normal((24, 40, 3)) * 10.0 ** rng.integers(-3, 8, (24, 40, 3))).astype(f32)
    assert (box_filter(F, 1) == F).all()
    for k in (2, 4):
        got = box_filter(F, k)
        for (X, Y) in ((0, 0), (3, 2), (40 // k - 1, 24 // k - 1)):
            assert (got[Y, X] == box_filter(F[k * Y:k * Y + k, k * X:k * X + k], k)[0, 0]).all()


def test_assemble_partitions_puts_bands_back_in_image_order():
    frame = np.arange(23 * 5 * 3, dtype=f32).reshape(23, 5, 3)
    for band_rows, n_parts in ((7, 3), (16, 2), (4, 1)):
        parts = []
        for p in range(n_parts):
            rows = [frame[y0:y0 + band_rows] for b, y0 in enumerate(range(0, 23, band_rows)) if b % n_parts == p]
            parts.append(np.concatenate(rows) if rows else np.zeros((0, 5, 3), dtype=f32))
        assert (assemble_partitions(parts, 23, band_rows, n_parts) == frame).all()
