"""The scene-kernel JIT's host side (csrc/rtc_jit.h, and rtc_scene_prep.h's deep_variant) -- no device needed.

rtc_diag_scene_plan prints, for every kernel variant of a scene, what the JIT would make of it: entry point, the header beside the
core, hiprtc's option list, the cache file's name and the ahead-of-time id.  The key's format -- the options one per line, then
"hiprtc M.m abi A args S" and the kind's own argument size, hashed after rtc_kernel_core.h's text and before the header's -- is
restated here in Python: it is what keeps every disk cache and every profile keyed by a kernel id matched to its kernel, so it is
pinned to the formula and not to the code under test.  The cache's entries -- the one piece of host code that reads files it did
not write -- go through rtc_diag_jit_cache_publish / _read.
"""
import os
import struct

import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from tests.test_scene_prep import _scene

CSRC = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "csrc")
PREFIXES = ["", "trace_", "adaptive2_", "adaptive4_", "ss2_", "ss4_"]
FIXED = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize"]
# prefix -> (entry point, header beside the core, "aot_..." prefix, the key's own argument line: (name, plan key) or None)
KINDS = {
    "": ("render_kernel_spec", "", "aot_", None),
    "trace_": ("trace_kernel_spec", "rtc_trace.h", "aot_trace_", ("trace args", "trace_args")),
    "adaptive2_": ("adaptive_refine_kernel_spec", "rtc_adaptive.h", "aot_adaptive2_", ("adaptive args", "adaptive_args")),
    "adaptive4_": ("adaptive_refine_kernel_spec", "rtc_adaptive.h", "aot_adaptive4_", ("adaptive args", "adaptive_args")),
    "ss2_": ("ss_render_kernel_spec", "rtc_supersample.h", "aot_ss2_", None),
    "ss4_": ("ss_render_kernel_spec", "rtc_supersample.h", "aot_ss4_", None),
}
THREE = ["soft_shadows", "hexagons", "mesh"]


@pytest.fixture(autouse=True)
def _library_defaults(monkeypatch):
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)


def fnv1a(data, h=1469598103934665603):  # (the library's offset basis: the standard one without its last digit -- part of every id)
    for byte in data:
        h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


_hashes = {}


def source_hash(name, h=None):
    """FNV-1a over csrc/<name>, continued from h; the core's own is computed once."""
    if (name, h) not in _hashes:
        with open(os.path.join(CSRC, name), "rb") as f:
            _hashes[(name, h)] = fnv1a(f.read()) if h is None else fnv1a(f.read(), h)
    return _hashes[(name, h)]


def plan_of(name, size=(64, 48)):
    world, camera = _scene(name, size)
    return world.scene_plan(camera)[1]


# ---------------------------------------------------------------------------------------------- kinds, options, key
@pytest.mark.parametrize("name", THREE)
def test_entry_point_and_header_of_every_kind(name):
    plan = plan_of(name)
    for prefix, (entry, header, _, _) in KINDS.items():
        assert (plan[prefix + "entry"], plan[prefix + "header"]) == (entry, header), prefix


@pytest.mark.parametrize("name", THREE)
def test_option_list(name):
    """The five fixed options, the variant's own in order, seven waves per SIMD where the variant names no number: once in all."""
    plan = plan_of(name)
    given = set()
    for prefix in PREFIXES:
        defs, options = plan[prefix + "spec_defs"].split(), plan[prefix + "options"].split()
        assert defs and options[:5] == FIXED and options[5:5 + len(defs)] == defs, prefix
        waves = [o for o in options if o.startswith("-DRTC_WAVES_PER_SIMD=")]
        assert len(waves) == 1, options
        own = any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in defs)
        assert options[5 + len(defs):] == ([] if own else ["-DRTC_WAVES_PER_SIMD=7"]), prefix
        given.add(own)
    assert given == {name != "soft_shadows"}  # (an area light's flat kernel takes the default, a tree kernel names its own)


@pytest.mark.parametrize("name", THREE)
def test_key_restated(name):
    """cache_file and aot_id by the formula: FNV-1a over rtc_kernel_core.h's bytes, the options one per line, the key's tail, and --
    not for the frame's own kernel -- the bytes of the header beside the core."""
    plan = plan_of(name)
    tail = "hiprtc %s abi 8 args %s\n" % (plan["hiprtc"], plan["render_args"])
    assert plan["key_tail"] + "\n" == tail
    major, minor = plan["hiprtc"].split(".")
    assert int(major) > 0 and str(int(major)) == major and str(int(minor)) == minor
    assert all(int(plan[k]) > 0 for k in ("render_args", "trace_args", "adaptive_args"))
    files = set()
    for prefix, (_, header, aot, own_args) in KINDS.items():
        defs = plan[prefix + "spec_defs"].split()
        options = FIXED + defs + ([] if any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in defs) else ["-DRTC_WAVES_PER_SIMD=7"])
        key = "".join(o + "\n" for o in options) + tail + ("%s %s\n" % (own_args[0], plan[own_args[1]]) if own_args else "")
        h = fnv1a(key.encode(), source_hash("rtc_kernel_core.h"))
        if header:
            h = source_hash(header, h)
        assert plan[prefix + "cache_file"] == "spec_%016x.hsaco" % h, prefix
        aot_hash = source_hash(header, source_hash("rtc_kernel_core.h")) if header else source_hash("rtc_kernel_core.h")
        assert plan[prefix + "aot_id"] == aot + "%016x" % aot_hash, prefix
        files.add(plan[prefix + "cache_file"])
    assert len(files) == len(KINDS)


# ---------------------------------------------------------------------------------------------- deep variants
def test_deep_stack_caps():
    """16, 32, ... up to RTC_MAX_DEPTH."""
    assert L.RTC_STACK_DEPTH_BASE == 8 and L.RTC_MAX_DEPTH == 255
    assert [P.deep_stack_cap(d) for d in (9, 16, 17, 32, 33, 128, 129, L.RTC_MAX_DEPTH)] == [16, 16, 32, 32, 64, 128, 255, 255]


def test_deep_variants_drop_the_lds_frames_and_name_the_stack_last():
    """glass_and_mirror: a point light over scale + translate objects that reflect, whose kernel keeps five recursion frames in LDS
    (-DRTC_SPEC_LDS_FRAMES=5); soft_shadows has no such option.  The frames of a deeper stack all live in scratch."""
    for name, lds in (("glass_and_mirror", True), ("soft_shadows", False), ("mesh", False)):
        plan = plan_of(name)
        for prefix in ("", "trace_"):
            defs = plan[prefix + "spec_defs"].split()
            assert ("-DRTC_SPEC_LDS_FRAMES=5" in defs) == lds, (name, prefix)
            kept = [d for d in defs if not d.startswith("-DRTC_SPEC_LDS_FRAMES=")]
            assert len(kept) == len(defs) - (1 if lds else 0)
            for cap in (16, 32):
                deep = plan["%sdeep%d_spec_defs" % (prefix, cap)].split()
                assert deep == kept + ["-DRTC_SPEC_MAX_DEPTH=%d" % cap], (name, prefix, cap)
        assert not any(key.startswith(("adaptive2_deep", "ss2_deep")) for key in plan)


def test_deep_variant_of_a_world_without_objects():
    world, camera = _scene("soft_shadows")
    plan = P.World([], world.light).scene_plan(camera)[1]
    for prefix in ("", "trace_"):
        for cap in (16, 32):
            assert plan["%sdeep%d_error" % (prefix, cap)] == "%d depth %d: no kernel options recorded for this scene" % (L.RTC_ERR_INVALID_ARG, cap)
            assert "%sdeep%d_spec_defs" % (prefix, cap) not in plan


# ---------------------------------------------------------------------------------------------- cache entries
HEADER = 24  # {char magic[8]; uint64 size, checksum}
PAYLOAD = bytes((i * 2654435761 >> 13) & 0xff for i in range(5003))  # arbitrary, no code object
NAME = "spec_0123456789abcdef.hsaco"


@pytest.fixture
def entry(tmp_path):
    """(path, bytes) of a published entry."""
    assert P.jit_cache_publish(str(tmp_path), NAME, PAYLOAD)
    path = tmp_path / NAME
    return path, path.read_bytes()


def test_publish_then_read(tmp_path, entry):
    path, raw = entry
    assert P.jit_cache_read(str(path)) == PAYLOAD
    assert sorted(os.listdir(tmp_path)) == [NAME]  # no .<pid> file is left
    assert raw == b"RTCJIT1\0" + struct.pack("<QQ", len(PAYLOAD), fnv1a(PAYLOAD)) + PAYLOAD and len(raw) == HEADER + len(PAYLOAD)
    assert P.jit_cache_publish(str(tmp_path), NAME, PAYLOAD[:100]) and P.jit_cache_read(str(path)) == PAYLOAD[:100]  # replaced whole


def test_every_truncation_is_rejected(entry):
    path, raw = entry
    for n in (0, 1, HEADER - 1, HEADER, HEADER + 1, len(raw) // 3, len(raw) - 1):
        path.write_bytes(raw[:n])
        assert P.jit_cache_read(str(path)) is None, n
    path.write_bytes(raw)
    assert P.jit_cache_read(str(path)) == PAYLOAD


def test_damaged_and_foreign_files_are_rejected(tmp_path, entry):
    path, raw = entry
    for what, at in (("magic", 3), ("size", 9), ("checksum", 17), ("payload", HEADER + 1234)):
        damaged = bytearray(raw)
        damaged[at] ^= 0x10
        path.write_bytes(bytes(damaged))
        assert P.jit_cache_read(str(path)) is None, what
    path.write_bytes(raw[:8] + struct.pack("<Q", 1 << 63) + raw[16:])
    assert P.jit_cache_read(str(path)) is None
    path.write_bytes(raw + b"\0")  # (one byte more than the size field says)
    assert P.jit_cache_read(str(path)) is None
    for foreign in (b"\x7fELF" + PAYLOAD, PAYLOAD, b"RTCJIT2\0" + raw[8:]):
        path.write_bytes(foreign)
        assert P.jit_cache_read(str(path)) is None
    assert P.jit_cache_read(str(tmp_path / "nothing.hsaco")) is None
    assert P.jit_cache_read(str(tmp_path)) is None  # a directory


def test_publish_creates_a_missing_directory_and_refuses_a_file(tmp_path):
    fresh = tmp_path / "cache"
    assert P.jit_cache_publish(str(fresh), NAME, PAYLOAD)
    assert os.listdir(fresh) == [NAME] and P.jit_cache_read(str(fresh / NAME)) == PAYLOAD
    plain = tmp_path / "plain"
    plain.write_bytes(b"x")
    assert not P.jit_cache_publish(str(plain), NAME, PAYLOAD)
    assert plain.read_bytes() == b"x" and sorted(os.listdir(tmp_path)) == ["cache", "plain"]
    assert not P.jit_cache_publish(str(tmp_path / "a" / "b"), NAME, PAYLOAD)  # (one level only, as the library's own directory needs)
    assert sorted(os.listdir(tmp_path)) == ["cache", "plain"]
