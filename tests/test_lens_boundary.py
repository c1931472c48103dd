"""CPU-only checks of the thin-lens camera's boundary (rtc_lens, rtc_lens_rays, rtc_ctx_set_scene_lens): the symbols exist and are
declared, the ABI version has not moved, argument errors are decided on the host, rtc_lens_rays -- the contract's executable
form (include/rtc.h) -- is the contract bit for bit against an independent numpy-f32 restatement, its rays have the properties a
lens's rays must have, and the lens kernel's names, ids and cache files are planned by the formula of every scene kernel."""
import ctypes as C
import ctypes.util
import inspect
import os

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import renderer as R
from ray_tracer_challenge_amd import scenes
from tests.test_jit_plan import FIXED, fnv1a, source_hash

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 26, 18

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sqrtf.restype = C.c_float
_libm.cosf.argtypes = _libm.sqrtf.argtypes = [C.c_float]


def _elementwise(fn, a):
    return np.array([fn(float(v)) for v in a.reshape(-1)], dtype=f32).reshape(a.shape)


def _cameras():
    view = P.view_transform(P.point(-2.6, 1.5, -3.9), P.point(-0.6, 1, -0.8), P.vector(0, 1, 0))
    # scaling after the view transform: the inverse's first two columns -- the lens's axes -- stay perpendicular, with lengths 1 / 1.5 and 1 / 0.75
    scaled = (P.scaling(1.5, 0.75, 2.0) @ np.asarray(view, dtype=f32)).astype(f32)
    return {"view": P.Camera(W, H, np.pi / 3, view), "non-uniform": P.Camera(W, H, 0.9, scaled)}


def _lens_rays(camera, k, lens, y0=0, n_rows=None):
    o, d = camera.lens_rays(k, lens, y0, n_rows)
    return o, d


# ---- the contract, restated: explicit float32 operations on arrays, one rounding each, nothing fused ----------------------
def _mix32(x):
    x = x.astype(u32)
    x = x ^ (x >> u32(16))
    x = x * u32(0x7feb352d)
    x = x ^ (x >> u32(15))
    x = x * u32(0x846ca68b)
    x = x ^ (x >> u32(16))
    return x


def _jitter(seed, key, path):
    h = _mix32(_mix32(key ^ u32(seed)) + u32((path * 0x9E3779B9) & 0xFFFFFFFF))
    return ((h >> u32(9)) + u32(1)).astype(f32) * f32(2.0 ** -23)  # (h >> 9) + 1 <= 2^23: exact in f32, and so is the product


def restated(camera, k, lens):
    """Steps 1 - 5 of include/rtc.h's rtc_lens_rays for the whole fine frame -> (o' (n, 3), d (n, 3), o (3,), P (n, 3), (ci, cj))."""
    fine = camera.supersampled(k)._cam
    inv = np.array(list(fine.inv), dtype=f32).reshape(4, 4)
    fw, fh = int(fine.width), int(fine.height)
    assert (fw, fh) == (k * camera.width, k * camera.height)
    x = np.tile(np.arange(fw, dtype=u32), fh)
    y = np.repeat(np.arange(fh, dtype=u32), fw)
    ps, hw, hh = f32(fine.pixel_size), f32(fine.half_width), f32(fine.half_height)
    # 1. camera.rs:60-70: the pixel point and the origin, matrix.rs:73-84 row by row, left to right
    wx = hw - (x.astype(f32) + f32(0.5)) * ps
    wy = hh - (y.astype(f32) + f32(0.5)) * ps
    p = np.stack([((inv[r, 0] * wx + inv[r, 1] * wy) + inv[r, 2] * f32(-1.0)) + inv[r, 3] * f32(1.0) for r in range(3)], axis=1)
    o = np.array([((inv[r, 0] * f32(0.0) + inv[r, 1] * f32(0.0)) + inv[r, 2] * f32(0.0)) + inv[r, 3] * f32(1.0) for r in range(3)], dtype=f32)
    # 2. key and jitter
    key = y * u32(fw) + x
    ju, jv = _jitter(lens.seed, key, 1), _jitter(lens.seed, key, 2)
    # 3. the lens cell, the sub-pixel cell turned by a quarter, and the point
    i, j = x % u32(k), y % u32(k)
    ci, cj = j, u32(k - 1) - i
    u = (ci.astype(f32) + ju) / f32(k)
    v = (cj.astype(f32) + jv) / f32(k)
    r = f32(lens.aperture_radius) * _elementwise(_libm.sqrtf, u)
    theta = f32(6.2831855) * v
    lx = r * _elementwise(_libm.cosf, theta)
    ly = r * _elementwise(_libm.cosf, theta - f32(1.5707964))
    # 4. the origin on the lens
    right, up = inv[:3, 0], inv[:3, 1]
    lo = np.stack([(o[a] + right[a] * lx) + up[a] * ly for a in range(3)], axis=1)
    # 5. through the focus point
    focus = np.stack([o[a] + (p[:, a] - o[a]) * f32(lens.focal_distance) for a in range(3)], axis=1)
    dv = focus - lo
    m = _elementwise(_libm.sqrtf, (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    d = dv / m[:, None]
    for a in (p, lo, focus, dv, d, u, v, lx, ly):
        assert a.dtype == f32
    return lo, d, o, focus, (ci, cj)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


LENSES = [P.Lens(0.35, 4.25, seed=0), P.Lens(0.0, 2.0, seed=7), P.Lens(2.5, 0.75, seed=0xDEADBEEF)]


# ---- 1. symbols, declarations, the ABI ----------------------------------------------------------------------------------
def test_the_symbols_exist_and_are_declared():
    raw = C.CDLL(L.LIB_PATH)
    for name in ("rtc_lens_rays", "rtc_ctx_set_scene_lens"):
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert getattr(P.lib(), name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert "typedef struct rtc_lens {" in header and "} rtc_lens;" in header
    assert "rtc_status rtc_lens_rays(const rtc_camera* output_camera, uint32_t k, const rtc_lens* lens, uint32_t y0, uint32_t n_rows," in header
    assert "rtc_status rtc_ctx_set_scene_lens(rtc_ctx* ctx, const rtc_scene* scene, const rtc_camera* output_camera, uint32_t k," in header
    assert "#define RTC_ABI_VERSION 8" in header
    assert P.lib().rtc_abi_version() == 8
    assert [n for n, _ in L.rtc_lens._fields_] == ["aperture_radius", "focal_distance", "seed"] and C.sizeof(L.rtc_lens) == 12
    assert "lens" in inspect.signature(R.Renderer.__init__).parameters
    assert "lens" in inspect.signature(R.Renderer.set_scene).parameters
    assert hasattr(R.Renderer, "set_lens") and hasattr(P.Camera, "lens_rays")
    lens = P.Lens(0.25, 3.0)
    assert (lens.aperture_radius, lens.focal_distance, lens.seed) == (0.25, 3.0, 0)


# ---- 2. argument errors, without a device -------------------------------------------------------------------------------
BAD_LENSES = [(-0.5, 1.0, b"aperture"), (float("nan"), 1.0, b"aperture"), (float("inf"), 1.0, b"aperture"), (-0.0001, 1.0, b"aperture"),
              (0.1, 0.0, b"focal"), (0.1, -2.0, b"focal"), (0.1, float("nan"), b"focal"), (0.1, float("inf"), b"focal")]


def _both_entry_points(cs, cam, k, lens):
    """The two entry points with the same lens arguments, no context and no buffers -> their (status, message)."""
    lib = P.lib()
    cam_p = C.byref(cam) if cam is not None else None
    lens_p = C.byref(lens) if lens is not None else None
    out = []
    st = lib.rtc_ctx_set_scene_lens(None, C.byref(cs.scene), cam_p, k, lens_p)
    out.append((st, lib.rtc_last_error()))
    st = lib.rtc_lens_rays(cam_p, k, lens_p, 0, 0, None, None)
    out.append((st, lib.rtc_last_error()))
    return out


def test_argument_errors_come_before_any_device_call():
    cs = P.default_world()._c()
    cam = P.Camera(100, 50, 1.0, np.eye(4, dtype=f32))._cam
    good = L.rtc_lens(0.1, 5.0, 0)
    for st, msg in _both_entry_points(cs, cam, 2, None):
        assert st == L.RTC_ERR_INVALID_ARG and b"lens is NULL" in msg
    for st, msg in _both_entry_points(cs, None, 2, good):
        assert st == L.RTC_ERR_INVALID_ARG and b"camera is NULL" in msg
    for k in (0, 1, 3, 5, 8):
        for st, msg in _both_entry_points(cs, cam, k, good):
            assert st == L.RTC_ERR_INVALID_ARG and b"factor %d" % k in msg, (k, msg)
    for radius, focal, word in BAD_LENSES:
        for st, msg in _both_entry_points(cs, cam, 4, L.rtc_lens(radius, focal, 0)):
            assert st == L.RTC_ERR_INVALID_ARG and word in msg, (radius, focal, msg)
    big = P.Camera(40000, 40000, 1.0, np.eye(4, dtype=f32))._cam  # what rtc_camera_supersampled refuses
    for st, msg in _both_entry_points(cs, big, 4, good):
        assert st == L.RTC_ERR_INVALID_ARG and b"exceeds" in msg
    # rows beyond the fine frame
    o = np.zeros((4, 4), dtype=f32)
    assert P.lib().rtc_lens_rays(C.byref(cam), 2, C.byref(good), 100, 1, o.ctypes.data_as(L.FP), None) == L.RTC_ERR_INVALID_ARG
    assert b"rows" in P.lib().rtc_last_error() and not o.any()
    with pytest.raises(P.RtcError) as e:
        P.Camera(10, 10, 1.0, np.eye(4, dtype=f32)).lens_rays(3, P.Lens(0.1, 1.0))
    assert e.value.status == L.RTC_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        P.Camera(10, 10, 1.0, np.eye(4, dtype=f32)).lens_rays(2, P.Lens(0.1, 1.0), y0=19, n_rows=2)


def test_a_valid_call_without_a_device_is_no_device():
    """Valid arguments and no context: where there is no device to have made one on, that is what the call reports; where there is
    one (tests/test_gpu_lens.py renders through the lens there), the missing context is the argument error."""
    cs = P.default_world()._c()
    cam = P.Camera(100, 50, 1.0, np.eye(4, dtype=f32))
    lens = P.Lens(0.1, 5.0)
    st = P.lib().rtc_ctx_set_scene_lens(None, C.byref(cs.scene), C.byref(cam._cam), 2, C.byref(lens._c))
    assert P.lib().rtc_last_error() != b""
    if P.device_count() == 0:
        assert st == L.RTC_ERR_NO_DEVICE
        with pytest.raises(P.RtcError) as e:
            R.Renderer(P.default_world(), cam, supersample=2, lens=lens)
        assert e.value.status == L.RTC_ERR_NO_DEVICE
    else:
        assert st == L.RTC_ERR_INVALID_ARG and b"ctx is NULL" in P.lib().rtc_last_error()
    o, d = cam.lens_rays(2, lens, 0, 1)  # ... and the rays need none
    assert o.shape == d.shape == (200, 4)


# ---- 3. rtc_lens_rays is the contract, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", ["view", "non-uniform"])
def test_lens_rays_equal_the_restated_contract(name, k):
    camera = _cameras()[name]
    for lens in LENSES:
        o, d = _lens_rays(camera, k, lens)
        exp_o, exp_d, _, _, _ = restated(camera, k, lens)
        assert o.shape == d.shape == (k * W * k * H, 4) and o.dtype == d.dtype == f32
        assert (_bits(o[:, :3]) == _bits(exp_o)).all(), (name, k, lens, int((_bits(o[:, :3]) != _bits(exp_o)).sum()))
        assert (_bits(d[:, :3]) == _bits(exp_d)).all(), (name, k, lens, int((_bits(d[:, :3]) != _bits(exp_d)).sum()))
        assert (o[:, 3] == 1.0).all() and (d[:, 3] == 0.0).all()  # rtc_ctx_trace's layout


# ---- 4. properties of the rays --------------------------------------------------------------------------------------------
U = 2.0 ** -24  # the unit roundoff of f32


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", ["view", "non-uniform"])
def test_origins_stay_on_the_lens(name, k):
    """|o' - o| <= R max(|right|, |up|): the lens point is r (right cos(theta) + up cos(theta - pi / 2)) with r <= R, and the two axes
    of these cameras are perpendicular.  Rounding: lx and ly carry the roundings of sqrtf, cosf, the product and of theta (whose
    error moves the point ALONG the circle, not outward, to first order), each component of o' two products and two sums of values
    no larger than |o|_max + R |axis|: a few ulp of that magnitude -- eight allowed."""
    camera = _cameras()[name]
    for lens in LENSES:
        o, _ = _lens_rays(camera, k, lens)
        _, _, origin, _, _ = restated(camera, k, lens)
        inv = camera.transform_inverse.astype(np.float64)
        right, up = inv[:3, 0], inv[:3, 1]
        assert abs(right @ up) <= 1e-6 * np.linalg.norm(right) * np.linalg.norm(up)  # (the cameras are what the bound is argued for)
        axis = max(np.linalg.norm(right), np.linalg.norm(up))
        off = np.linalg.norm(o[:, :3].astype(np.float64) - origin.astype(np.float64), axis=1)
        tol = 8 * 2 * U * (np.abs(origin).max() + lens.aperture_radius * axis)
        assert off.max() <= lens.aperture_radius * axis + tol, (name, k, lens, off.max())
        if lens.aperture_radius == 0.0:
            assert (_bits(o[:, :3]) == _bits(origin)[None, :]).all()  # a pinhole: every ray leaves the camera's origin
        else:
            assert off.max() > 0.5 * lens.aperture_radius * min(np.linalg.norm(right), np.linalg.norm(up))  # (the lens is used)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", ["view", "non-uniform"])
def test_every_ray_passes_through_its_focus_point(name, k):
    """With v = P - o' in exact arithmetic (P, o': the f32 values of steps 4 and 5), the code forms fl(P - o') -- each component
    v_a (1 + e1), |e1| <= u --, the length m of that, and fl(fl(v_a) / m) = v_a (1 + e1)(1 + e2) / m, |e2| <= u.  So d is a positive
    multiple of v + e with |e_a| <= (2 u + u^2) |v_a|, hence |e| <= (2 u + u^2) |v|, and the sine of the angle between d and v is at most
    |e| / |v|: |cross(v, d)| <= (2 u + u^2) |v| |d|, |d| <= 1 + 4 u (tests/test_trace_boundary.py).  Bound: 2.5 u |v|.  The
    check is made in float64, whose own rounding is nine orders below."""
    camera = _cameras()[name]
    for lens in LENSES:
        o, d = _lens_rays(camera, k, lens)
        _, _, _, focus, _ = restated(camera, k, lens)
        v = focus.astype(np.float64) - o[:, :3].astype(np.float64)
        miss = np.linalg.norm(np.cross(v, d[:, :3].astype(np.float64)), axis=1)
        assert (miss <= 2.5 * U * np.linalg.norm(v, axis=1)).all(), (name, k, lens, (miss / np.linalg.norm(v, axis=1)).max() / U)
        assert (np.einsum("ij,ij->i", v, d[:, :3].astype(np.float64)) > 0).all()  # ... towards it, not away
        assert np.abs(np.linalg.norm(d[:, :3].astype(np.float64), axis=1) - 1.0).max() <= 4 * U


@pytest.mark.parametrize("k", [2, 4])
def test_the_samples_of_a_pixel_fall_in_distinct_lens_cells(k):
    """The cell is read back from the ray's own origin: o' - o = right lx + up ly, u = (|l| / R)^2, v = angle / 2 pi."""
    camera, lens = _cameras()["view"], LENSES[0]
    o, _ = _lens_rays(camera, k, lens)
    _, _, origin, _, (ci, cj) = restated(camera, k, lens)
    inv = camera.transform_inverse.astype(np.float64)
    off = o[:, :3].astype(np.float64) - origin.astype(np.float64)
    # (perpendicular axes, not unit ones: the reference's view_transform does not normalise `left` where `up` leans)
    lx, ly = off @ inv[:3, 0] / (inv[:3, 0] @ inv[:3, 0]), off @ inv[:3, 1] / (inv[:3, 1] @ inv[:3, 1])
    u = (lx * lx + ly * ly) / lens.aperture_radius ** 2
    v = (np.arctan2(ly, lx) / (2 * np.pi)) % 1.0
    cell_u, cell_v = np.minimum((u * k).astype(int), k - 1), np.minimum((v * k).astype(int), k - 1)
    # read back through f32 roundings (o' carries half an ulp of |o| ~ 4, 2.4e-7, against a lens of 0.35): a point within 1e-4 of a
    # cell's border may land next door, and the angle of a point at the lens's very centre is not known; those are not judged
    near = (np.abs(u * k - np.round(u * k)) < 1e-4) | (np.abs(v * k - np.round(v * k)) < 1e-4) | (u < 1e-3)
    assert near.sum() <= 0.01 * near.size
    assert ((cell_u == ci) & (cell_v == cj) | near).all()
    # ... and by construction: the k x k (ci, cj) of an output pixel are all different, and not aligned with the sub-pixel offsets
    fw = k * W
    cells = (ci.astype(int) * k + cj.astype(int)).reshape(k * H, fw)
    for Y in range(H):
        for X in range(W):
            block = cells[k * Y:k * Y + k, k * X:k * X + k]
            assert len(set(block.reshape(-1).tolist())) == k * k
    x, y = np.tile(np.arange(fw), k * H), np.repeat(np.arange(k * H), fw)
    assert not ((ci == x % k) & (cj == y % k)).all()


def test_rays_are_deterministic_and_rows_are_rows_of_the_frame():
    camera, lens, k = _cameras()["view"], LENSES[0], 2
    o, d = _lens_rays(camera, k, lens)
    o2, d2 = _lens_rays(camera, k, P.Lens(lens.aperture_radius, lens.focal_distance, lens.seed))
    assert (_bits(o) == _bits(o2)).all() and (_bits(d) == _bits(d2)).all()
    fw = k * W
    for y0, n in ((0, 1), (5, 7), (k * H - 3, 3), (k * H, 0)):
        po, pd = _lens_rays(camera, k, lens, y0, n)
        assert po.shape == (n * fw, 4)
        assert (_bits(po) == _bits(o[y0 * fw:(y0 + n) * fw])).all() and (_bits(pd) == _bits(d[y0 * fw:(y0 + n) * fw])).all()
    # only the directions are asked for, only the origins
    only_d = np.zeros((fw, 4), dtype=f32)
    assert P.lib().rtc_lens_rays(C.byref(camera._cam), k, C.byref(lens._c), 3, 1, None, only_d.ctypes.data_as(L.FP)) == L.RTC_OK
    assert (_bits(only_d) == _bits(d[3 * fw:4 * fw])).all()


def test_another_seed_moves_the_lens_points():
    camera, k = _cameras()["view"], 4
    a, _ = _lens_rays(camera, k, P.Lens(0.35, 4.25, seed=1))
    b, _ = _lens_rays(camera, k, P.Lens(0.35, 4.25, seed=2))
    moved = (_bits(a[:, :3]) != _bits(b[:, :3])).any(axis=1)
    assert moved.mean() > 0.99


# ---- 5. the lens kernel's plan ------------------------------------------------------------------------------------------
@pytest.fixture
def _library_defaults(monkeypatch):
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)


@pytest.mark.parametrize("name", ["soft_shadows", "reflect_refract", "mesh"])
def test_the_lens_kernels_are_planned_by_the_formula(name, _library_defaults):
    """Names, options, cache file and ahead-of-time id of the lens kernels of a scene (rtc_diag_scene_plan's lens2_ / lens4_ lines): the
    supersampling kernel's, with the lens's option last, and both headers' bytes -- rtc_supersample.h, then rtc_lens.h -- behind the key."""
    world, camera, _ = getattr(scenes, name)(64, 48)
    plan = world.scene_plan(camera)[1]
    core = source_hash("rtc_kernel_core.h")
    tail = "hiprtc %s abi 8 args %s\n" % (plan["hiprtc"], plan["render_args"])
    seen = set()
    for k in (2, 4):
        lens, ss = "lens%d_" % k, "ss%d_" % k
        assert plan[lens + "entry"] == "lens_render_kernel_spec" and plan[lens + "header"] == "rtc_lens.h" and plan[lens + "header_below"] == "rtc_supersample.h"
        assert plan[lens + "family_name"] == plan[ss + "family_name"].replace("ss_render_kernel<", "lens_render_kernel<")
        assert plan[lens + "family_name"].startswith("lens_render_kernel<") and plan[lens + "family_name"].endswith(";ss=%d>" % k)
        assert plan[lens + "spec_name"] == plan[ss + "spec_name"].replace("ss_render_kernel_spec[", "lens_render_kernel_spec[")[:-1] + ";lens]"
        assert plan[lens + "spec_name"].endswith(";ss=%d;lens]" % k)
        defs = plan[lens + "spec_defs"].split()
        assert defs == plan[ss + "spec_defs"].split() + ["-DRTC_SPEC_LENS=1"] and "-DRTC_SPEC_SS=%d" % k in defs
        options = FIXED + defs + ([] if any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in defs) else ["-DRTC_WAVES_PER_SIMD=7"])
        assert plan[lens + "options"].split() == options
        assert int(plan[lens + "args"]) == int(plan["render_args"]) + 8 + 16  # SsRenderArgs' two words, the lens's three, padded to 8 bytes
        key = "".join(o + "\n" for o in options) + tail + "lens args %s\n" % plan[lens + "args"]
        h = source_hash("rtc_lens.h", source_hash("rtc_supersample.h", fnv1a(key.encode(), core)))
        assert plan[lens + "cache_file"] == "spec_%016x.hsaco" % h
        assert plan[lens + "aot_id"] == "aot_lens%d_%016x" % (k, source_hash("rtc_lens.h", source_hash("rtc_supersample.h", core)))
        seen |= {plan[lens + "cache_file"], plan[ss + "cache_file"], plan[lens + "aot_id"], plan[ss + "aot_id"]}
    assert len(seen) == 8 and plan["cache_file"] not in seen and plan["aot_id"] not in seen


# ---------------------------------------------------------------- the lens and the library's own hierarchy (ERROR_BUDGET.md B9)
def test_a_lens_too_wide_for_the_flat_hierarchy_drops_it(monkeypatch):
    """build_flat_bvh pads its boxes for rays that start within 100 of the smallest half-axis of everything, and a lens frame's
    primary rays start on the lens disc: cam_origin +- R along the camera's two axes belongs to the hull the plan tests.  Restated
    here in double precision for tests/test_flat_bvh.py's cloud, and asked of the library a tenth below and above the radius at
    which the restatement turns."""
    from tests.test_flat_bvh import _cloud
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", "0")
    world, camera = _cloud(7, 20)
    assert "bvh" in world.scene_plan(camera)[1]["family_name"]
    cs = world._c()

    def library(lens):
        return L.lib().rtc_diag_flat_bvh(C.byref(cs.scene), C.byref(camera._cam), C.byref(lens._c) if lens is not None else None)

    lo, hi, r_min = np.full(3, np.inf), np.full(3, -np.inf), np.inf
    for ob in world.objects:
        m = np.asarray(ob.transform, dtype=np.float64).reshape(4, 4)
        c, h = m[:3, 3], np.abs(np.diag(m[:3, :3]))
        lo, hi, r_min = np.minimum(lo, c - h), np.maximum(hi, c + h), min(r_min, float(h.min()))
    inv = camera.transform_inverse.astype(np.float64)
    origin, axes = inv[:3, 3], np.abs(inv[:3, :2]).max(axis=1)  # per world axis: the larger of the two camera axes' components

    def restated(R):
        l, h = np.minimum(lo, origin - R * axes), np.maximum(hi, origin + R * axes)
        return bool(np.linalg.norm(h - l) < 100.0 * r_min and max(np.abs(l).max(), np.abs(h).max()) <= 2.5e3 * r_min)

    assert restated(0.0) and not restated(1e3)
    a, b = 0.0, 1e3
    for _ in range(60):
        mid = 0.5 * (a + b)
        a, b = (mid, b) if restated(mid) else (a, mid)
    assert 0.5 < a < 100.0, a  # (a lens of a useful size keeps the hierarchy; one as wide as the scene does not)
    assert library(None) == 1
    assert library(P.Lens(0.0, 14.0)) == 1
    assert library(P.Lens(0.9 * a, 14.0)) == 1
    assert library(P.Lens(1.1 * a, 14.0)) == 0
    assert library(P.Lens(1e3, 14.0)) == 0
    monkeypatch.setenv("RTC_AMD_BVH", "0")
    assert library(None) == 0
