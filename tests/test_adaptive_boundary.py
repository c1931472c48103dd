"""CPU-only checks of adaptive supersampling's boundary (rtc_ctx_render_adaptive): the symbols exist and are
declared, the ABI version has not moved, the numpy mask (tests/adaptive_helpers.py) is the contract's rule on hand-computed
frames, argument errors are decided on the host, and the refinement's slot mapping (csrc/rtc_adaptive.h adaptive_slot, the function the kernel calls) puts a pixel's k x k
samples where the lane reduce adds them in box_filter's order."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import renderer as R
from tests.adaptive_helpers import compose, edge_mask
from tests.supersample_helpers import box_filter

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_exist_and_are_declared():
    raw = C.CDLL(L.LIB_PATH)
    for name in ("rtc_ctx_render_adaptive", "rtc_ctx_adaptive_stats", "rtc_ctx_adaptive_kernel_name", "rtc_ctx_adaptive_kernel_id"):
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
    assert hasattr(raw, "rtc_diag_adaptive_plan") and "rtc_diag_adaptive_plan" in L.EXTRA
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert "rtc_status rtc_ctx_render_adaptive(rtc_ctx* ctx, int32_t depth, uint32_t k, float threshold, void* d_out_rgb," in header
    assert "rtc_status rtc_ctx_adaptive_stats(rtc_ctx* ctx, rtc_adaptive_stats* out);" in header
    assert "} rtc_adaptive_stats;" in header
    assert "#define RTC_ABI_VERSION 8" in header
    assert P.lib().rtc_abi_version() == 8
    # the struct as the header lays it out: four u64 and two f32
    assert C.sizeof(L.rtc_adaptive_stats) == 40
    assert [f[0] for f in L.rtc_adaptive_stats._fields_] == ["refined_pixels", "rays", "shaded_hits", "culled_shadow_rays", "mask_ms", "refine_ms"]
    params = inspect.signature(R.Renderer.render_adaptive).parameters
    assert list(params)[1:] == ["depth", "k", "threshold", "out", "mask", "stream"]
    assert params["k"].default == 2 and params["threshold"].default == 0.1
    assert hasattr(R.Renderer, "adaptive_stats")


# ---------------------------------------------------------------- the mask, by hand
def _frame(rows):
    """rows of grey values -> (H, W, 3) float32"""
    g = np.asarray(rows, dtype=f32)
    return np.repeat(g[:, :, None], 3, axis=2).copy()


def test_the_compare_is_strict_at_exactly_the_threshold():
    B = _frame([[0.0, 0.5, 0.5, 1.25]])  # differences 0.5, 0, 0.75: all exact in f32
    assert edge_mask(B, 0.5).tolist() == [[False, False, True, True]]
    assert edge_mask(B, np.nextafter(f32(0.5), f32(0))).tolist() == [[True, True, True, True]]
    assert edge_mask(B, 0.75).tolist() == [[False, False, False, False]]
    assert edge_mask(B, 0.0).tolist() == [[True, True, True, True]]
    assert not edge_mask(_frame([[0.25, 0.25], [0.25, 0.25]]), 0.0).any()  # 0 > 0 is false: a flat frame flags nothing at threshold 0
    # the subtraction and the compare are f32: 1 - (1 - 2^-24) is 2^-24 exactly, and the threshold 0.1 is 0.1f
    a, b = f32(1.0), np.nextafter(f32(1.0), f32(0))
    assert edge_mask(_frame([[a, b]]), 2.0 ** -24).tolist() == [[False, False]] and edge_mask(_frame([[a, b]]), 2.0 ** -25).all()
    assert not edge_mask(_frame([[0.0, f32(0.1)]]), 0.1).any()  # (as doubles, 0.1f > 0.1)


def test_four_neighbours_not_eight_and_both_pixels_of_a_pair():
    # one bright pixel: itself and its four neighbours, not the diagonals
    B = _frame(np.zeros((5, 5)))
    B[2, 2] = 1.0
    exp = np.zeros((5, 5), dtype=bool)
    exp[2, 2] = exp[1, 2] = exp[3, 2] = exp[2, 1] = exp[2, 3] = True
    assert np.array_equal(edge_mask(B, 0.1), exp)
    # a diagonal contrast alone: (0, 0) and (1, 1) differ, but each 4-neighbour pair is within the threshold
    D = _frame([[0.0, 0.1], [0.1, 0.2]])
    assert abs(D[0, 0, 0] - D[1, 1, 0]) > f32(0.15)
    assert not edge_mask(D, 0.15).any()
    # both pixels of a pair, and only they
    assert edge_mask(_frame([[0.0, 0.0, 1.0, 1.0]]), 0.5).tolist() == [[False, True, True, False]]
    assert edge_mask(_frame([[0.0], [0.0], [1.0], [1.0]]), 0.5)[:, 0].tolist() == [False, True, True, False]


def test_corners_and_one_pixel_wide_frames():
    B = _frame(np.zeros((3, 4)))
    B[0, 0] = B[2, 3] = 1.0
    exp = np.zeros((3, 4), dtype=bool)
    exp[0, 0] = exp[0, 1] = exp[1, 0] = exp[2, 3] = exp[2, 2] = exp[1, 3] = True
    assert np.array_equal(edge_mask(B, 0.1), exp)
    assert edge_mask(_frame([[3.0]]), 0.0).tolist() == [[False]]  # 1 x 1: no neighbour
    assert edge_mask(_frame([[0.0, 1.0, 1.0]]), 0.5).tolist() == [[True, True, False]]  # one row
    assert edge_mask(_frame([[0.0], [1.0], [1.0]]), 0.5)[:, 0].tolist() == [True, True, False]  # one column
    # the black last row and column take part like any pixel: a lit frame flags them and their neighbours
    lit = _frame(np.full((3, 3), 0.8))
    lit[-1] = 0.0
    lit[:, -1] = 0.0
    assert np.array_equal(edge_mask(lit, 0.1), np.array([[0, 1, 1], [1, 1, 1], [1, 1, 0]], dtype=bool))


def test_nan_and_inf_minus_inf_never_flag_and_one_channel_is_enough():
    inf, nan = f32(np.inf), f32(np.nan)
    assert not edge_mask(_frame([[nan, 0.0, nan]]), 0.0).any()
    assert not edge_mask(_frame([[inf, inf]]), 0.0).any()  # inf - inf is NaN
    assert edge_mask(_frame([[inf, 0.0]]), 1e30).all()     # inf - 0 is inf > anything finite
    assert edge_mask(_frame([[inf, -inf]]), 1e30).all()
    B = _frame([[0.5, 0.5]])
    for c in range(3):
        one = B.copy()
        one[0, 1, c] = 0.75
        assert edge_mask(one, 0.2).all() and not edge_mask(one, 0.25).any()
    # a NaN in one channel does not hide a contrast in another
    mixed = B.copy()
    mixed[0, 0, 0] = nan
    mixed[0, 1, 2] = 1.0
    assert edge_mask(mixed, 0.1).all()


def test_compose_takes_s_where_flagged_and_b_elsewhere():
    B, S = _frame([[0.0, 0.0, 1.0]]), _frame([[7.0, 8.0, 9.0]])
    M = edge_mask(B, 0.5)
    out = compose(B, S, M)
    assert out[:, :, 0].tolist() == [[0.0, 8.0, 9.0]] and B[0, 1, 0] == 0.0  # (a copy)
    assert np.array_equal(compose(B, S, np.zeros((1, 3), dtype=bool)), B)


# ---------------------------------------------------------------- argument errors, on the host
def test_argument_errors_are_decided_before_any_device_call():
    """A null context is the LAST of the argument checks: each wrong argument is reported by name with no context at all, on
    a machine without a device (a device call would answer RTC_ERR_NO_DEVICE or fault on the null context)."""
    lib = P.lib()
    buf = (C.c_float * 16)()
    out = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(out.value + 1)

    def call(depth=5, k=2, threshold=0.1, o=out, mask=None):
        st = lib.rtc_ctx_render_adaptive(None, depth, k, threshold, o, mask, None)
        return st, lib.rtc_last_error().decode()

    for bad in (float("nan"), float("inf"), -float("inf"), -0.5, -1e-30):
        st, msg = call(threshold=bad)
        assert st == L.RTC_ERR_INVALID_ARG and "threshold" in msg, (bad, msg)
    for bad in (0, 1, 3, 5, 8, 16):
        st, msg = call(k=bad)
        assert st == L.RTC_ERR_INVALID_ARG and "factor %d" % bad in msg, (bad, msg)
    st, msg = call(o=None)
    assert st == L.RTC_ERR_INVALID_ARG and "null output" in msg
    st, msg = call(o=odd)
    assert st == L.RTC_ERR_INVALID_ARG and "aligned" in msg
    for bad in (-1, 256, 1000):
        st, msg = call(depth=bad)
        assert st == L.RTC_ERR_INVALID_ARG and "depth %d" % bad in msg, (bad, msg)
    # everything right but the context: named last; threshold 0 and -0.0 are thresholds
    for ok in (0.0, -0.0, 0.1, 3e38):
        st, msg = call(threshold=ok)
        assert st == L.RTC_ERR_INVALID_ARG and "ctx is NULL" in msg, (ok, msg)
    # the order: threshold, factor, pointers, depth
    assert "threshold" in call(threshold=-1.0, k=3, o=None, depth=-1)[1]
    assert "factor" in call(k=3, o=None, depth=-1)[1]
    assert "null output" in call(o=None, depth=-1)[1]
    st = L.rtc_adaptive_stats()
    assert lib.rtc_ctx_adaptive_stats(None, C.byref(st)) == L.RTC_ERR_INVALID_ARG
    assert lib.rtc_ctx_adaptive_kernel_name(None) == b"" and lib.rtc_ctx_adaptive_kernel_id(None) == b""


# ---------------------------------------------------------------- the refinement's plan
def _plan(k, first, n, width=64, height=64, n_cus=256, wgs_per_cu=6):
    out = (C.c_uint32 * (4 * n))()
    grid = C.c_uint32()
    chunk = P.lib().rtc_diag_adaptive_plan(k, width, height, n_cus, wgs_per_cu, first, n, out, C.byref(grid))
    return chunk, np.array(out, dtype=np.int64).reshape(n, 4), grid.value


@pytest.mark.parametrize("k", [2, 4])
def test_every_slot_of_a_chunk_maps_to_its_entry_and_sample(k):
    kk = k * k
    for first in (0, 256, 5 * 256, (1 << 32) - 256, (1 << 33) + 3 * 256):
        chunk, m, _ = _plan(k, first, 256)  # four waves' steps
        assert chunk == 64  # a wave's step: one slot per lane
        for i in range(256):
            slot = first + i
            entry, sx, sy, lane = m[i]
            assert entry == (slot // kk) & 0xffffffff and sx == (slot % kk) % k and sy == (slot % kk) // k and lane == i % 64, (k, slot)
            assert lane % kk == sy * k + sx  # sx in the low log2 k bits of the lane, sy in the next
        # a k x k group never straddles a wave: the k^2 lanes of an entry are consecutive and start at a multiple of k^2
        for w in range(4):
            wave = m[64 * w:64 * w + 64]
            for g in range(64 // kk):
                grp = wave[g * kk:(g + 1) * kk]
                assert len(set(grp[:, 0])) == 1 and grp[0, 3] % kk == 0
                assert sorted((int(a), int(b)) for a, b in grp[:, 1:3]) == [(x, y) for x in range(k) for y in range(k)]
    assert P.lib().rtc_diag_adaptive_plan(3, 64, 64, 256, 6, 0, 0, None, None) == 0


def test_the_grid_does_not_depend_on_the_flagged_count():
    """As many workgroups as the device holds, capped by what a fully flagged frame could feed (one step of 64 slots for each of a workgroup's four waves)."""
    for k in (2, 4):
        assert _plan(k, 0, 1, 4096, 4096, 256, 6)[2] == 256 * 6
        assert _plan(k, 0, 1, 1, 1, 256, 6)[2] == 1
        assert _plan(k, 0, 1, 50, 20, 256, 6)[2] == min(256 * 6, -(-50 * 20 * k * k // 256))
        assert _plan(k, 0, 1, 64, 64, 0, 0)[2] == 1
        assert _plan(k, 0, 1, 65535, 16383, 256, 2)[2] == 512


@pytest.mark.parametrize("k", [2, 4])
def test_the_lane_reduce_over_the_mapping_is_box_filters_order(k):
    """One wave's 64 lanes hold 64 / k^2 flagged pixels.  Walking lanes ^ 1, ^ 2 (k = 4: then ^ 4, ^ 8) -- for k = 2 that is
    ^ 1 then ^ k -- adds each pixel's k x k samples in the order of box_filter, on values where
    another order gives other bits."""
    kk, n = k * k, 64 // (k * k)
    rng = np.random.default_rng(7 + k)
    # magnitudes spread over 2^-12 .. 2^12: every partial sum rounds, and differently in another order
    fine = (rng.standard_normal((k, k * n, 3)) * np.exp2(rng.integers(-12, 13, (k, k * n, 3)))).astype(f32)
    _, m, _ = _plan(k, 13 * 64, 64)  # some wave's step
    lanes = np.zeros((64, 3), dtype=f32)
    first_entry = m[0, 0]
    for entry, sx, sy, lane in m:
        lanes[lane] = fine[sy, (entry - first_entry) * k + sx]
    v = lanes.copy()
    for mask in ((1, 2) if k == 2 else (1, 2, 4, 8)):
        v = v + v[np.arange(64) ^ mask]
        assert v.dtype == f32
    v = v * f32(1.0 / kk)
    exp = box_filter(fine, k)  # (1, n, 3)
    for g in range(n):
        for lane in range(g * kk, (g + 1) * kk):  # every lane of a group ends with the group's value
            assert v[lane].tobytes() == exp[0, g].tobytes(), (k, g, lane)
    # ... and the values tell orders apart: along y first gives other bits somewhere
    w = lanes.copy()
    for mask in ((2, 1) if k == 2 else (4, 8, 1, 2)):
        w = w + w[np.arange(64) ^ mask]
    w = w * f32(1.0 / kk)
    assert w[::kk].tobytes() != exp[0].tobytes()
