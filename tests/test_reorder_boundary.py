"""CPU-only checks of ray reordering's boundary (rtc_ctx_ray_order, rtc_ctx_trace_reordered, rtc_ctx_reorder_stats; csrc/rtc_reorder.h):
the symbols exist and are declared, the ABI version has not moved, the argument errors that need no device come by name and in
rtc_ctx_trace's order, and the coherence key -- one function, host and device -- is what include/rtc.h says it is: the numpy
restatement below is written from that comment, not from the code."""
import ctypes as C
import os

import numpy as np

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd.scenes import PI, Camera, f32, point, vector, view_transform
from tests import hits_helpers as HH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtc_ctx_ray_order", "rtc_ctx_trace_reordered", "rtc_ctx_reorder_stats")
DIAG = ("rtc_diag_ray_keys", "rtc_diag_reorder_plan")
# Pointers that are never followed: every call below is refused before the library looks behind them.
ALIGNED, BY_FOUR, BY_ONE = C.c_void_p(0x10000), C.c_void_p(0x10004), C.c_void_p(0x10001)
NO_CTX = None  # no context can be made without a device; the entry points check their other arguments first and say which they refuse
F = np.float32
U32P = C.POINTER(C.c_uint32)


def test_the_symbols_exist_and_are_declared():
    raw = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert " %s(" % name in header, name
        assert getattr(P.lib(), name).restype is C.c_int
    for name in DIAG:
        assert hasattr(raw, name), name
        assert name in L.EXTRA and name not in header, name
    assert "} rtc_reorder_stats;" in header
    assert [f[0] for f in L.rtc_reorder_stats._fields_] == ["n", "keys_ms", "sort_ms", "gather_ms", "trace_ms", "scatter_ms"]
    assert C.sizeof(L.rtc_reorder_stats) == 32
    assert L.SIGNATURES["rtc_ctx_trace_reordered"] == L.SIGNATURES["rtc_ctx_trace"]  # rtc_ctx_trace's arguments
    assert "#define RTC_ABI_VERSION 8" in header
    assert P.lib().rtc_abi_version() == 8


def _refused(status, lib, *words):
    assert status == L.RTC_ERR_INVALID_ARG, status
    msg = lib.rtc_last_error()
    assert msg != b""
    for w in words:
        assert w in msg, (w, msg)


def test_trace_reordered_argument_errors_are_rtc_ctx_traces():
    """tests/test_trace_boundary.py's list, call for call: the same refusals in the same order, under the entry point's own name."""
    lib = P.lib()
    f = lib.rtc_ctx_trace_reordered
    _refused(f(None, 5, ALIGNED, ALIGNED, None, 4, ALIGNED, None), lib, b"rtc_ctx_trace_reordered", b"ctx")
    _refused(f(None, 5, ALIGNED, ALIGNED, BY_FOUR, 4, BY_FOUR, None), lib, b"ctx")
    _refused(f(NO_CTX, 5, None, ALIGNED, None, 4, ALIGNED, None), lib, b"rtc_ctx_trace_reordered", b"null ray")
    _refused(f(NO_CTX, 5, ALIGNED, None, None, 4, ALIGNED, None), lib, b"null ray")
    _refused(f(NO_CTX, 5, ALIGNED, ALIGNED, None, 4, None, None), lib, b"null output")
    _refused(f(NO_CTX, 5, BY_FOUR, ALIGNED, None, 4, ALIGNED, None), lib, b"16-byte")
    _refused(f(NO_CTX, 5, ALIGNED, BY_FOUR, None, 4, ALIGNED, None), lib, b"16-byte")
    _refused(f(NO_CTX, 5, ALIGNED, ALIGNED, BY_ONE, 4, ALIGNED, None), lib, b"4-byte")
    _refused(f(NO_CTX, 5, ALIGNED, ALIGNED, None, 4, BY_ONE, None), lib, b"4-byte")
    _refused(f(NO_CTX, -1, ALIGNED, ALIGNED, None, 4, ALIGNED, None), lib, b"depth")
    _refused(f(NO_CTX, L.RTC_MAX_DEPTH + 1, ALIGNED, ALIGNED, None, 4, ALIGNED, None), lib, b"depth")
    # the order: pointers before alignment before depth before the context
    _refused(f(NO_CTX, -1, None, BY_FOUR, BY_ONE, 4, ALIGNED, None), lib, b"null ray")
    _refused(f(NO_CTX, -1, ALIGNED, BY_FOUR, BY_ONE, 4, ALIGNED, None), lib, b"16-byte")
    _refused(f(NO_CTX, -1, ALIGNED, ALIGNED, BY_ONE, 4, ALIGNED, None), lib, b"4-byte")
    # ... and, as for rtc_ctx_trace, a null context with nothing to trace is still a null context
    _refused(f(None, 5, None, None, None, 0, None, None), lib, b"ctx")
    # the very same calls are refused alike by rtc_ctx_trace
    for args in ((NO_CTX, -1, None, BY_FOUR, BY_ONE, 4, ALIGNED, None), (NO_CTX, -1, ALIGNED, BY_FOUR, BY_ONE, 4, ALIGNED, None),
                 (NO_CTX, -1, ALIGNED, ALIGNED, BY_ONE, 4, ALIGNED, None), (NO_CTX, -1, ALIGNED, ALIGNED, None, 4, ALIGNED, None)):
        assert lib.rtc_ctx_trace(*args) == f(*args) == L.RTC_ERR_INVALID_ARG
        a = lib.rtc_ctx_trace(*args), lib.rtc_last_error()
        b = f(*args), lib.rtc_last_error()
        assert b[1] == a[1].replace(b"rtc_ctx_trace:", b"rtc_ctx_trace_reordered:"), (a, b)


def test_ray_order_argument_errors_and_nothing_to_order():
    lib = P.lib()
    f = lib.rtc_ctx_ray_order
    _refused(f(None, ALIGNED, ALIGNED, 4, ALIGNED, None), lib, b"rtc_ctx_ray_order", b"ctx")
    _refused(f(NO_CTX, None, ALIGNED, 4, ALIGNED, None), lib, b"rtc_ctx_ray_order", b"null ray")
    _refused(f(NO_CTX, ALIGNED, None, 4, ALIGNED, None), lib, b"null ray")
    _refused(f(NO_CTX, ALIGNED, ALIGNED, 4, None, None), lib, b"null output")
    _refused(f(NO_CTX, BY_FOUR, ALIGNED, 4, ALIGNED, None), lib, b"16-byte")
    _refused(f(NO_CTX, ALIGNED, BY_FOUR, 4, ALIGNED, None), lib, b"16-byte")
    _refused(f(NO_CTX, ALIGNED, ALIGNED, 4, BY_ONE, None), lib, b"4-byte")
    _refused(f(NO_CTX, None, BY_FOUR, 4, BY_ONE, None), lib, b"null ray")  # pointers before alignment
    _refused(f(NO_CTX, BY_FOUR, ALIGNED, 0, ALIGNED, None), lib, b"16-byte")  # alignment is checked whatever n
    # n = 0: RTC_OK, nothing launched, the context not looked at
    assert f(NO_CTX, None, None, 0, None, None) == L.RTC_OK
    assert f(NO_CTX, ALIGNED, ALIGNED, 0, BY_FOUR, None) == L.RTC_OK
    st = L.rtc_reorder_stats()
    _refused(lib.rtc_ctx_reorder_stats(None, C.byref(st)), lib, b"rtc_ctx_reorder_stats")


# ---- the key, restated from include/rtc.h ------------------------------------------------
def _cell(t, cells, last):
    """last if t >= cells, (int)t if t > 0, else 0 -- a NaN fails both compares"""
    with np.errstate(invalid="ignore"):
        top = t >= F(cells)
        inside = (t > F(0.0)) & ~top
        return np.where(top, last, np.trunc(np.where(inside, t, F(0.0)))).astype(np.uint32)


def _spread(c, step, bits):
    r = np.zeros(c.shape, dtype=np.uint32)
    for k in range(bits):
        r |= ((c >> np.uint32(k)) & np.uint32(1)) << np.uint32(step * k)
    return r


def _finite(x):
    fmax = np.finfo(F).max
    with np.errstate(invalid="ignore"):
        return (x >= -fmax) & (x <= fmax)


def numpy_box(origins):
    lo, hi = np.full(3, np.inf, dtype=F), np.full(3, -np.inf, dtype=F)
    for a in range(3):
        x = origins[:, a]
        x = x[_finite(x)]
        if len(x):
            lo[a], hi[a] = x.min(), x.max()
    return lo, hi


def numpy_keys(origins, directions):
    """include/rtc.h "The coherence key of a ray" in float32 numpy: one rounding per operation, nothing fused."""
    origins, directions = np.asarray(origins, dtype=F), np.asarray(directions, dtype=F)
    lo, hi = numpy_box(origins)
    origin = np.zeros(len(origins), dtype=np.uint32)
    with np.errstate(all="ignore"):
        for a in range(3):
            x = origins[:, a]
            if hi[a] > lo[a]:
                t = (x - lo[a]) * (F(16.0) / (hi[a] - lo[a]))
                cell = np.where(_finite(x), _cell(t, 16.0, 15), 0).astype(np.uint32)
            else:
                cell = np.zeros(len(x), dtype=np.uint32)
            origin |= _spread(cell, 3, 4) << np.uint32(a)
        dx, dy, dz = directions[:, 0], directions[:, 1], directions[:, 2]
        ab = lambda v: np.where(v < F(0.0), -v, v)
        sign = lambda v: np.where(v >= F(0.0), F(1.0), F(-1.0)).astype(F)
        s = (ab(dx) + ab(dy)) + ab(dz)
        ok = (s > F(0.0)) & _finite(s)
        px, py = dx / s, dy / s
        fx, fy = (F(1.0) - ab(py)) * sign(px), (F(1.0) - ab(px)) * sign(py)
        px, py = np.where(dz < F(0.0), fx, px), np.where(dz < F(0.0), fy, py)
        u = np.where(ok, _cell((px * F(0.5) + F(0.5)) * F(1024.0), 1024.0, 1023), 0).astype(np.uint32)
        v = np.where(ok, _cell((py * F(0.5) + F(0.5)) * F(1024.0), 1024.0, 1023), 0).astype(np.uint32)
    direction = _spread(u, 2, 10) | (_spread(v, 2, 10) << np.uint32(1))
    return (origin << np.uint32(20)) | direction


def diag_keys(origins, directions):
    """rtc_diag_ray_keys: the library's key function on the host -> (box (6,), keys (n,))."""
    o = np.ascontiguousarray(origins, dtype=F)
    d = np.ascontiguousarray(directions, dtype=F)
    n = o.shape[0]
    assert o.shape == (n, 4) and d.shape == (n, 4)
    box, keys = np.zeros(6, dtype=F), np.zeros(max(n, 1), dtype=np.uint32)
    P.lib().rtc_diag_ray_keys(o.ctypes.data_as(L.FP), d.ctypes.data_as(L.FP), n, box.ctypes.data_as(L.FP), keys.ctypes.data_as(U32P))
    return box, keys[:n]


def seeded_rays(n=4096, seed=20240607):
    """Origins in a box, directions over the whole sphere (both signs of z), not normalised alike."""
    rng = np.random.RandomState(seed)
    o = np.ones((n, 4), dtype=F)
    o[:, :3] = (rng.uniform(-1.0, 1.0, (n, 3)) * np.array([3.0, 0.5, 40.0]) + np.array([1.0, 2.0, -7.0])).astype(F)
    d = np.zeros((n, 4), dtype=F)
    v = rng.normal(size=(n, 3))
    d[:, :3] = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.25, 4.0, (n, 1))).astype(F)
    assert n < 64 or ((d[:, 2] < 0).sum() > n // 3 and (d[:, 2] > 0).sum() > n // 3)
    return o, d


def non_finite_rays():
    """seeded_rays with a handful of NaN, +-inf and zero components in origins and directions (never traced: ordered only)."""
    o, d = seeded_rays(3000, seed=77)
    o[3, 0], o[17, 1], o[99, 2] = np.nan, np.inf, -np.inf
    o[100, :3] = np.nan
    o[5, 0] = 0.0
    o[6, 1] = -0.0
    d[4, 0], d[18, 1], d[98, 2] = np.nan, np.inf, -np.inf
    d[200, :3] = 0.0
    d[201, :3] = (-0.0, 0.0, -0.0)
    d[202, :2] = 0.0
    d[203, 2] = 0.0
    d[204, :3] = (np.finfo(F).max, np.finfo(F).max, 1.0)  # |x| + |y| overflows
    return o, d


def test_the_host_key_is_the_headers_formula():
    for what, (o, d) in (("box", seeded_rays()), ("non-finite", non_finite_rays())):
        box, keys = diag_keys(o, d)
        lo, hi = numpy_box(o)
        assert (box[:3] == lo).all() and (box[3:] == hi).all(), (what, box, lo, hi)
        exp = numpy_keys(o, d)
        bad = np.flatnonzero(keys != exp)
        assert len(bad) == 0, (what, len(bad), bad[:5], keys[bad[:5]], exp[bad[:5]])
        assert len(np.unique(keys >> 20)) > 1000 and len(np.unique(keys & 0xfffff)) > 1000  # (all of the key is in use)
    # one origin for all rays -- a camera's -- is a degenerate box: origin bits 0, the key is the direction's
    o, d = seeded_rays()
    o[:, :3] = (1.0, 0.8, -2.5)
    box, keys = diag_keys(o, d)
    assert (box[:3] == box[3:]).all()
    assert (keys == numpy_keys(o, d)).all() and (keys >> 20 == 0).all() and len(np.unique(keys)) > 1000
    # no ray, one ray
    assert diag_keys(np.zeros((0, 4)), np.zeros((0, 4)))[1].shape == (0,)
    box, keys = diag_keys(o[:1], d[:1])
    assert keys[0] == numpy_keys(o[:1], d[:1])[0] and keys[0] >> 20 == 0


def _ray(o, d):
    return np.array([list(o) + [1.0]], dtype=F), np.array([list(d) + [0.0]], dtype=F)


def test_what_the_key_means():
    # the eight corners of the stream's box: the eight octants in the top three origin bits, x lowest
    corners = [(x, y, z) for z in (-7.0, 5.0) for y in (2.0, 2.5) for x in (-1.0, 9.0)]
    o = np.array([list(c) + [1.0] for c in corners], dtype=F)
    d = np.tile(np.array([[0.0, 0.0, 1.0, 0.0]], dtype=F), (8, 1))
    _, keys = diag_keys(o, d)
    assert (keys >> 29 == np.arange(8)).all(), keys >> 29
    # (cells 0 and 15 on every axis; 15's four bits land on bits 0, 3, 6, 9 of the axis' lane: 0x249)
    assert (keys >> 20 == np.array([sum(((i >> a) & 1) * (0x249 << a) for a in range(3)) for i in range(8)])).all()
    # the six axis directions: six known cells (u, v) of the 1024 x 1024 octahedral grid
    axes = {(1, 0, 0): (1023, 512), (-1, 0, 0): (0, 512), (0, 1, 0): (512, 1023), (0, -1, 0): (512, 0), (0, 0, 1): (512, 512), (0, 0, -1): (1023, 1023)}
    seen = set()
    for axis, (u, v) in axes.items():
        for scale in (1.0, 0.125, 3.0):  # the direction's length does not matter
            _, k = diag_keys(*_ray((0, 0, 0), tuple(scale * a for a in axis)))
            exp = sum(((u >> b) & 1) << (2 * b) | ((v >> b) & 1) << (2 * b + 1) for b in range(10))
            assert k[0] == exp, (axis, scale, hex(k[0]), hex(exp))
        seen.add(int(k[0]))
    assert len(seen) == 6
    # two rays in one origin cell and one direction cell: equal keys; a third elsewhere: another
    o = np.array([[0, 0, 0, 1], [16, 16, 16, 1], [5.1, 5.2, 5.3, 1], [5.9, 5.01, 5.6, 1], [5.1, 6.2, 5.3, 1]], dtype=F)
    d = np.array([[0, 0, 1, 0], [0, 0, 1, 0], [0.3, 0.2, 0.5, 0], [0.3001, 0.2001, 0.5, 0], [0.3, 0.2, 0.5, 0]], dtype=F)
    _, k = diag_keys(o, d)
    assert k[2] == k[3] and k[4] != k[2], [hex(x) for x in k]
    assert k[2] >> 20 == 0x1c7 and k[4] >> 20 == 0x1c7 ^ 0x12, [hex(x) for x in k]  # cells (5, 5, 5) and (5, 6, 5): y's bits are 1, 4, 7, 10


def test_sorting_by_key_brings_a_shuffled_frames_rays_together():
    """The camera's rays of a 64 x 64 frame (tests/test_gpu_trace.py's camera), shuffled, then ordered by key: the 64 rays of a wave
    cover a far smaller patch of the image than image order's 64 x 1 rows (width + height = 65).  The figure is a fact about the
    key (DESIGN.md 8f quotes it), not a tuned bound."""
    w = h = 64
    camera = Camera(w, h, PI / f32(5.0), view_transform(point(1, 0.8, -2.5), point(0, 0.4, 7), vector(0, 1, 0)))
    o, d = HH.camera_rays(camera)
    perm = np.random.RandomState(99).permutation(w * h)
    _, keys = diag_keys(o[perm], d[perm])
    order = np.argsort(keys, kind="stable")

    def mean_extent(pixels):
        runs = pixels.reshape(-1, 64)
        xs, ys = runs % w, runs // w
        return float(((xs.max(axis=1) - xs.min(axis=1) + 1) + (ys.max(axis=1) - ys.min(axis=1) + 1)).mean())
    image, shuffled, by_key = mean_extent(np.arange(w * h)), mean_extent(perm), mean_extent(perm[order])
    print("mean width + height of a wave's pixels: image order %.2f, shuffled %.2f, by key %.2f" % (image, shuffled, by_key))
    assert image == 65.0
    assert shuffled > 100.0
    assert by_key < 65.0


def _plan(n, n_cus):
    out = (C.c_uint32 * 3)()
    grid = P.lib().rtc_diag_reorder_plan(n, n_cus, out)
    assert grid == out[0]
    return int(out[0]), int(out[1]), int(out[2])


def test_the_sorts_plan_tiles_the_stream():
    assert _plan(0, 256)[0] == 0
    assert _plan(1, 256) == (1, 256, 256)
    for n_cus in (1, 8, 256, 304):
        for n in (1, 255, 256, 257, 1872, 65536, 65537, 1000003, 2 ** 24, 2 ** 31 + 5, 2 ** 32 - 1):
            grid, segment, tile = _plan(n, n_cus)
            assert tile == 256 and segment % tile == 0 and segment > 0
            assert 1 <= grid <= (n + tile - 1) // tile
            # workgroup w owns [w * segment, min(n, (w + 1) * segment)): no gap, no overlap, none empty, all of [0, n)
            assert (grid - 1) * segment < n <= grid * segment, (n, n_cus, grid, segment)
