"""CPU-only checks of the first-hit entry points' boundary (rtc_hit_at, rtc_ctx_render_hits): the symbols exist and are
declared, the ABI version has not moved, rtc_hit_planes is eleven pointers, and the argument errors are decided before any
device call -- so they come back as RTC_ERR_INVALID_ARG on a machine without a GPU too."""
import ctypes as C
import os

import numpy as np

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rays(n=2):
    o = np.tile(np.array([0, 0, -5, 1], dtype=f32), (n, 1))
    d = np.tile(np.array([0, 0, 1, 0], dtype=f32), (n, 1))
    return o, d


def _fp(a):
    return a.ctypes.data_as(L.FP)


def test_the_symbols_exist_and_are_declared():
    raw = C.CDLL(L.LIB_PATH)
    for name in ("rtc_hit_at", "rtc_ctx_render_hits"):
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert getattr(P.lib(), name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert "rtc_status rtc_hit_at(" in header and "rtc_status rtc_ctx_render_hits(" in header
    assert "#define RTC_ABI_VERSION 8" in header
    assert P.lib().rtc_abi_version() == 8


def test_hit_planes_is_eleven_pointers_in_the_headers_order():
    assert C.sizeof(L.rtc_hit_planes) == 11 * C.sizeof(C.c_void_p)
    names = [f[0] for f in L.rtc_hit_planes._fields_]
    assert names == ["object", "distance", "point", "eye", "normal", "reflectv", "over_point", "under_point", "inside", "n1n2", "light"]
    assert list(L.HIT_PLANES) == names
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    body = header[header.index("typedef struct rtc_hit_planes {"):header.index("} rtc_hit_planes;")]
    at = [body.index(" %s;" % n) for n in names]
    assert at == sorted(at)


def test_hit_at_argument_errors_come_before_any_device_call():
    lib = P.lib()
    cs = P.default_world()._c()
    o, d = _rays()
    obj = np.zeros(2, dtype=np.int32)
    hp = L.rtc_hit_planes()
    # no plane requested
    assert lib.rtc_hit_at(C.byref(cs.scene), _fp(o), _fp(d), 2, 0, C.byref(hp)) == L.RTC_ERR_INVALID_ARG
    assert b"no plane" in lib.rtc_last_error()
    assert lib.rtc_hit_at(C.byref(cs.scene), _fp(o), _fp(d), 2, 0, None) == L.RTC_ERR_INVALID_ARG
    assert lib.rtc_last_error() != b""
    # a null ray pointer with n > 0
    hp.object = obj.ctypes.data
    assert lib.rtc_hit_at(C.byref(cs.scene), None, _fp(d), 2, 0, C.byref(hp)) == L.RTC_ERR_INVALID_ARG
    assert b"null ray" in lib.rtc_last_error()
    assert lib.rtc_hit_at(C.byref(cs.scene), _fp(o), None, 2, 0, C.byref(hp)) == L.RTC_ERR_INVALID_ARG
    assert b"null ray" in lib.rtc_last_error()
    # ... but not with n == 0: nothing to do
    assert lib.rtc_hit_at(C.byref(cs.scene), None, None, 0, 0, C.byref(hp)) == L.RTC_OK
    # rays as rtc_color_at wants them: origin.w 1, direction.w 0
    bad = d.copy()
    bad[1, 3] = 1.0
    assert lib.rtc_hit_at(C.byref(cs.scene), _fp(o), _fp(bad), 2, 0, C.byref(hp)) == L.RTC_ERR_INVALID_ARG
    assert b"ray 1" in lib.rtc_last_error()
    assert (obj == 0).all()  # nothing was written


def test_render_hits_argument_errors_come_before_any_device_call():
    lib = P.lib()
    obj = np.zeros(4, dtype=np.int32)
    hp = L.rtc_hit_planes()
    hp.object = obj.ctypes.data
    assert lib.rtc_ctx_render_hits(None, None, C.byref(hp), None) == L.RTC_ERR_INVALID_ARG
    assert b"rtc_ctx_render_hits" in lib.rtc_last_error()
    assert lib.rtc_ctx_render_hits(None, None, None, None) == L.RTC_ERR_INVALID_ARG
    assert (obj == 0).all()


def test_world_hit_at_names_its_planes():
    w = P.default_world()
    o, d = _rays()
    try:
        w.hit_at(o, d, planes=("object", "colour"))
    except KeyError as e:
        assert "colour" in str(e)
    else:
        raise AssertionError("an unknown plane was accepted")
    if P.device_count() == 0:  # no GPU: an error, not a fallback
        try:
            w.hit_at(o, d)
        except P.RtcError as e:
            assert e.status == L.RTC_ERR_NO_DEVICE
        else:
            raise AssertionError("hit_at answered without a device")
