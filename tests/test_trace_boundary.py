"""CPU-only checks of the ray-stream entry points' boundary (rtc_ctx_trace, rtc_ctx_camera_rays, rtc_ctx_trace_kernel_name /
_id): the symbols exist and are declared, the ABI version has not moved, the argument errors that need no device are decided
before any device call, and the two ray generators (ray_tracer_challenge_amd/rays.py) make what they say on CPU tensors."""
import ctypes as C
import math
import os

import numpy as np
import torch

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import rays
from ray_tracer_challenge_amd.scenes import PI, Camera, f32, point, vector, view_transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtc_ctx_trace", "rtc_ctx_camera_rays", "rtc_ctx_trace_kernel_name", "rtc_ctx_trace_kernel_id")
# Pointers that are never followed: every call below is refused before the library looks behind them.
ALIGNED, BY_FOUR, BY_ONE = C.c_void_p(0x10000), C.c_void_p(0x10004), C.c_void_p(0x10001)
# No context can be made without a device, so every call here passes a null one.  The entry points check their other arguments
# first and say which one they refuse: the message, not only the status, tells a pointer error from the null context's.  (No scene
# set and a real context's depth range: tests/test_gpu_trace.py.)
NO_CTX = None


def test_the_symbols_exist_and_are_declared():
    raw = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert " %s(" % name in header, name
    assert P.lib().rtc_ctx_trace.restype is C.c_int and P.lib().rtc_ctx_camera_rays.restype is C.c_int
    assert P.lib().rtc_ctx_trace_kernel_name.restype is C.c_char_p and P.lib().rtc_ctx_trace_kernel_id.restype is C.c_char_p
    assert "#define RTC_ABI_VERSION 8" in header
    assert P.lib().rtc_abi_version() == 8


def _refused(status, lib, *words):
    assert status == L.RTC_ERR_INVALID_ARG, status
    msg = lib.rtc_last_error()
    assert msg != b""
    for w in words:
        assert w in msg, (w, msg)


def test_trace_argument_errors_come_before_any_device_call():
    lib = P.lib()
    # a null context (everything else in order)
    _refused(lib.rtc_ctx_trace(None, 5, ALIGNED, ALIGNED, None, 4, ALIGNED, None), lib, b"rtc_ctx_trace", b"ctx")
    _refused(lib.rtc_ctx_trace(None, 5, ALIGNED, ALIGNED, BY_FOUR, 4, BY_FOUR, None), lib, b"ctx")
    # null ray or output pointers with n > 0
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, None, ALIGNED, None, 4, ALIGNED, None), lib, b"null ray")
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, ALIGNED, None, None, 4, ALIGNED, None), lib, b"null ray")
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, ALIGNED, ALIGNED, None, 4, None, None), lib, b"null output")
    # misaligned: 16 bytes for the rays, 4 for keys and output
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, BY_FOUR, ALIGNED, None, 4, ALIGNED, None), lib, b"16-byte")
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, ALIGNED, BY_FOUR, None, 4, ALIGNED, None), lib, b"16-byte")
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, ALIGNED, ALIGNED, BY_ONE, 4, ALIGNED, None), lib, b"4-byte")
    _refused(lib.rtc_ctx_trace(NO_CTX, 5, ALIGNED, ALIGNED, None, 4, BY_ONE, None), lib, b"4-byte")
    # depth out of range
    _refused(lib.rtc_ctx_trace(NO_CTX, -1, ALIGNED, ALIGNED, None, 4, ALIGNED, None), lib, b"depth")
    _refused(lib.rtc_ctx_trace(NO_CTX, L.RTC_MAX_DEPTH + 1, ALIGNED, ALIGNED, None, 4, ALIGNED, None), lib, b"depth")
    # ... and a null context with nothing to trace is still a null context
    _refused(lib.rtc_ctx_trace(None, 5, None, None, None, 0, None, None), lib, b"ctx")


def test_camera_rays_argument_errors_come_before_any_device_call():
    lib = P.lib()
    cam = Camera(40, 30, PI / f32(3.0), view_transform(point(0, 1, -5), point(0, 1, 0), vector(0, 1, 0)))._cam
    _refused(lib.rtc_ctx_camera_rays(None, C.byref(cam), 0, 30, ALIGNED, ALIGNED, BY_FOUR, None), lib, b"rtc_ctx_camera_rays", b"ctx")
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, None, 0, 30, ALIGNED, ALIGNED, BY_FOUR, None), lib, b"camera")
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, C.byref(cam), 0, 30, BY_FOUR, ALIGNED, None, None), lib, b"16-byte")
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, C.byref(cam), 0, 30, None, BY_FOUR, None, None), lib, b"16-byte")
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, C.byref(cam), 0, 30, None, None, BY_ONE, None), lib, b"4-byte")
    # y0 + n_rows > height, also where the sum wraps 32 bits
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, C.byref(cam), 7, 24, ALIGNED, ALIGNED, BY_FOUR, None), lib, b"rows")
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, C.byref(cam), 31, 0, ALIGNED, ALIGNED, BY_FOUR, None), lib, b"rows")
    _refused(lib.rtc_ctx_camera_rays(NO_CTX, C.byref(cam), 2, 0xffffffff, ALIGNED, ALIGNED, BY_FOUR, None), lib, b"rows")


def test_the_names_of_no_context_are_empty():
    assert P.lib().rtc_ctx_trace_kernel_name(None) == b"" and P.lib().rtc_ctx_trace_kernel_id(None) == b""


# ---- the generators ---------------------------------------------------------------
# |d| of a direction normalised in float32 as rays._normalize does, u = 2^-24 (round to nearest), first order in u:
#   the three products carry (1 + e), |e| <= u each; the first sum another, the second sum another: the sum of squares is
#   s (1 + t) with |t| <= 3 u (a term passes through its product and at most two sums);
#   the square root halves that and adds its own rounding: m^ = |v| (1 + t'), |t'| <= 1.5 u + u = 2.5 u;
#   each component is divided by m^ and rounded once more: +- u on the length.
# So | |d| - 1 | <= 3.5 u (1 + O(u)): within 4 u = 2 ulp of 1.0 (ulp(1) = 2^-23).  The check measures |d| in float64, whose
# own rounding (2^-53) is nine orders below.
UNIT_BOUND = 4.0 * 2.0 ** -24


def _lengths(directions):
    d = directions.to(torch.float64)[:, :3]
    return torch.sqrt((d * d).sum(dim=1))


def _check_layout(o, d, n):
    assert o.shape == (n, 4) and d.shape == (n, 4), (o.shape, d.shape)
    assert o.dtype == torch.float32 and d.dtype == torch.float32
    assert o.device.type == "cpu" and d.device.type == "cpu"
    assert o.is_contiguous() and d.is_contiguous()
    assert bool((o[:, 3] == 1.0).all()) and bool((d[:, 3] == 0.0).all())
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(d).all())
    worst = float((_lengths(d) - 1.0).abs().max())
    assert worst <= UNIT_BOUND, (worst, UNIT_BOUND)


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def test_orthographic_rays():
    w, h, view = 40, 30, 8.0
    # (a level view: the reference's view_transform is orthonormal only where `up` is perpendicular to the line of sight, and the
    # grid's steps are checked in world units below)
    t = view_transform(point(1, 2, -6), point(0.5, 2, 0), vector(0, 1, 0))
    o, d = rays.orthographic(w, h, view, t)
    _check_layout(o, d, w * h)
    o2, d2 = rays.orthographic(w, h, view, t)
    assert _same_bits(o, o2) and _same_bits(d, d2)
    # parallel: one vector, the camera's -z in world space
    assert bool((d.view(torch.int32) == d[0].view(torch.int32)[None, :]).all())
    inv = np.linalg.inv(np.asarray(t, dtype=np.float64).reshape(4, 4))
    fwd = inv @ np.array([0.0, 0.0, -1.0, 0.0])
    fwd = fwd[:3] / np.linalg.norm(fwd[:3])
    assert np.abs(d[0, :3].numpy().astype(np.float64) - fwd).max() <= 4 * 2.0 ** -24
    # the origins: a w x h grid of view / w steps in the plane through the camera's position, perpendicular to the direction
    og = o[:, :3].numpy().astype(np.float64).reshape(h, w, 3)
    assert np.abs((og - np.array([1.0, 2.0, -6.0])) @ fwd).max() <= 1e-5
    step = view / w
    assert np.abs(np.linalg.norm(og[:, 1:] - og[:, :-1], axis=2) - step).max() <= 1e-5
    assert np.abs(np.linalg.norm(og[1:] - og[:-1], axis=2) - step).max() <= 1e-5
    assert np.abs(og.mean(axis=(0, 1)) - np.array([1.0, 2.0, -6.0])).max() <= 1e-5  # centred on the camera
    assert og[0, 0, 1] > og[-1, 0, 1]  # image rows run downwards


def test_equirectangular_rays():
    w, h = 48, 24
    o, d = rays.equirectangular(w, h, point(0.5, 1.0, -2.0))
    _check_layout(o, d, w * h)
    o2, d2 = rays.equirectangular(w, h, point(0.5, 1.0, -2.0))
    assert _same_bits(o, o2) and _same_bits(d, d2)
    assert bool((o[:, :3] == torch.tensor([0.5, 1.0, -2.0])).all())
    dg = d[:, :3].numpy().astype(np.float64).reshape(h, w, 3)
    lon = np.arctan2(dg[..., 0], dg[..., 2])
    lat = np.arcsin(np.clip(dg[..., 1], -1.0, 1.0))
    step = 2.0 * math.pi / w
    # longitude along x: the same in every row, `step` from column to column, first and last one step short of the full turn
    assert np.abs(lon - lon[0][None, :]).max() <= 1e-5
    assert np.abs((lon[:, 1:] - lon[:, :-1]) - step).max() <= 1e-5
    assert np.abs((lon[:, -1] - lon[:, 0]) - (2.0 * math.pi - step)).max() <= 1e-5
    assert abs(lon[0, 0] - (-math.pi + 0.5 * step)) <= 1e-5
    # latitude along y: the same in every column, from just under the zenith to just over the nadir
    assert np.abs(lat - lat[:, :1]).max() <= 1e-5
    assert np.abs((lat[:-1] - lat[1:]) - math.pi / h).max() <= 1e-5
    assert abs(lat[0, 0] - (0.5 * math.pi - 0.5 * math.pi / h)) <= 1e-5
