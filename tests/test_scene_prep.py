"""Getting a scene ready, on the host (csrc/rtc_scene_prep.h) -- no device needed.

rtc_diag_scene_plan runs what rtc_ctx_set_scene runs before it touches the device -- flatten, then plan_scene -- under the
environment's policy and returns digests of what was packed (header, records, texels, tile masks) and the plan as text.
Which kernel a scene gets is asserted here on the plan's names; tests/test_flat_bvh.py::test_flat_bvh_eligibility checks on
the device that a context's kernel_name is the one the plan predicts.  Digests are only ever compared between two calls of
one library: the packing uses the C library's double-precision atan2 / acos / sin, so no expected values are stored.
"""
import os

import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes
from tests.test_flat_bvh import _cloud
from tests.test_groups import _small_tree_world

SCENES = ["soft_shadows", "single_sphere", "glass_and_mirror", "sphere_grid", "first_scene", "first_plane", "first_patterns",
          "reflect_refract", "patterns_medley", "hexagons", "grouped_grid", "groups_medley", "mesh", "here_be_dragons",
          "first_textures", "skybox", "shapes_medley"]
HDR, RECORDS, TEXELS, MASKS = range(4)  # the four digests


@pytest.fixture(autouse=True)
def _library_defaults(monkeypatch):
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)


_worlds = {}


def _scene(name, size=(64, 48)):
    """(world, camera at `size`) of a scenes.py constructor; the world is built once."""
    if name not in _worlds:
        _worlds[name] = getattr(scenes, name)(64, 48)[:2]
    world, camera = _worlds[name]
    return world, P.Camera(size[0], size[1], camera.field_of_view, camera.transform)


def kernel_name(world, camera):
    """The name a context (not a one-shot one: nothing is deferred) reports for this scene under the current environment."""
    plan = world.scene_plan(camera)[1]
    return plan["spec_name"] if plan["compile_now"] == "1" else plan["family_name"]


# ---------------------------------------------------------------------------------------------- kernel choice without a GPU
def flat_bvh_eligibility_cases():
    """(what, world, expected) of tests/test_flat_bvh.py::test_flat_bvh_eligibility, which asserts the same on a device;
    expected: (RTC_AMD_SPECIALIZE, predicate on the kernel's name)."""
    world, camera = _cloud(7, 20)
    balls = P.World([o for o in world.objects if o.kind == world.objects[0].kind] * 2, world.light)
    few = P.World(world.objects[:15], world.light)
    floor = P.World(world.objects + [P.Plane()], world.light)
    tilted = P.World(list(world.objects), world.light)
    tilted.objects[3] = P.Sphere(P.chain(P.rotation_z(0.3), P.scaling(1, 2, 1)), world.objects[3].material)
    speck = P.World(list(world.objects), world.light)
    speck.objects[5] = P.Sphere(P.scaling(0.01, 0.01, 0.01), world.objects[5].material)
    cyl = P.World(list(world.objects), world.light)
    cyl.objects[0] = P.Cylinder(P.identity_4x4(), world.objects[0].material, minimum_y=0.0, maximum_y=1.0)
    no_bvh = lambda name: name.find("bvh") < 0
    return camera, [("cloud", world, "0", lambda name: name == "render_kernel<tree,bvh>"),
                    ("cloud", world, "1", lambda name: name == "render_kernel_spec[tree,bvh]"),
                    ("balls", balls, "1", lambda name: name.startswith("render_kernel_spec[tree,bvh;all 0x")),
                    ("few", few, "0", no_bvh), ("floor", floor, "0", no_bvh), ("tilted", tilted, "0", no_bvh),
                    ("speck", speck, "0", no_bvh), ("cylinder", cyl, "0", no_bvh)]


def test_flat_bvh_eligibility_on_the_plan(monkeypatch):
    monkeypatch.setenv("RTC_AMD_BVH", "1")
    camera, cases = flat_bvh_eligibility_cases()
    for what, world, _, expected in cases:
        for specialise in ("0", "1"):
            monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
            name = kernel_name(world, camera)
            if specialise == "0":
                assert name.startswith("render_kernel<"), (what, name)
            assert ("bvh" in name) == (what in ("cloud", "balls")), (what, specialise, name)
    for what, world, specialise, expected in cases:
        monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
        assert expected(kernel_name(world, camera)), (what, specialise, kernel_name(world, camera))


def test_group_kernel_selection_on_the_plan():
    """The three names of tests/test_groups.py::test_group_kernel_selection_and_flat_equivalence."""
    world, camera, _ = scenes.hexagons(64, 32)
    assert kernel_name(world, camera) == "render_kernel<tree>"
    flat_world, camera2, _ = scenes.first_scene(64, 32)
    assert kernel_name(flat_world, camera2).startswith("render_kernel<")
    w = P.World([P.GroupShape()] + list(flat_world.objects), flat_world.light)  # empty groups are ignored
    assert kernel_name(w, camera2) != "render_kernel<tree>"
    assert kernel_name(w, camera2) == kernel_name(flat_world, camera2)


@pytest.mark.parametrize("seed", range(10))
def test_small_trees_are_gated_on_the_plan(seed, monkeypatch):
    world, camera = _small_tree_world(seed, area_light=seed % 2 == 0)
    if not any(isinstance(o, P.GroupShape) and o.leaves() for o in world.objects):
        return  # (a world of leaves only: nothing to gate)
    for specialise in ("0", "1"):
        monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
        for gates in ("1", "0"):
            monkeypatch.setenv("RTC_AMD_GATES", gates)
            name = kernel_name(world, camera)
            assert ("tree" in name) == (gates == "0"), (gates, name)
            if specialise == "1" and gates == "1":
                assert ";gates" in name, name


def test_specialisation_policy_and_name_tags(monkeypatch):
    """tests/test_gpu_parity.py::test_specialisation_policy_defaults, and the tags of a scene kernel's name."""
    assert kernel_name(*_scene("soft_shadows", (64, 64))) == "render_kernel<4,simple>"  # thumbnail: ahead-of-time
    assert kernel_name(*_scene("soft_shadows", (1024, 512))).startswith("render_kernel_spec[")  # >= 2^18 pixels
    world, camera, _ = scenes.sphere_grid(1024, 512)
    assert kernel_name(world, camera) == "render_kernel_spec[tree,bvh;all 0x500]"
    monkeypatch.setenv("RTC_AMD_BVH", "0")
    assert kernel_name(world, camera) == "render_kernel_spec[all 0x500]"
    world.objects[3].casts_shadow = False  # ... no longer alike
    assert kernel_name(world, camera) == "render_kernel<0,general>"
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", "1")
    assert kernel_name(world, camera) == "render_kernel<0,general>"  # a mixed list is left to the ahead-of-time loop
    assert world.scene_plan(camera)[1]["spec_name"] == "render_kernel_spec[any]"
    for name, simple, patterns in (("single_sphere", True, False), ("soft_shadows", True, False), ("first_scene", False, False),
                                   ("first_patterns", False, True)):  # (first_scene's walls are rotated: not scale + translate)
        spec, plan = kernel_name(*_scene(name)), _scene(name)[0].scene_plan(_scene(name)[1])[1]
        assert spec.startswith("render_kernel_spec[0x") and spec == plan["spec_name"], spec
        assert (";simple" in spec) == simple == (plan["simple"] == "1"), spec
        assert (";patterns" in spec) == patterns, spec
        assert ("simple>" in plan["family_name"]) == simple, plan["family_name"]


# ------------------------------------------------------------------------------------------------- option lists
ONCE = ["RTC_SPEC_LIST", "RTC_SPEC_NOBJ", "RTC_SPEC_SHARE", "RTC_SPEC_BLOCKS_Y", "RTC_SPEC_RECT", "RTC_SPEC_LIGHT_KIND", "RTC_SPEC_JITTER",
        "RTC_SPEC_PATTERNS", "RTC_SPEC_LIGHT_ZEROS", "RTC_SPEC_ANY_REFL", "RTC_SPEC_ANY_REFR", "RTC_SPEC_REG_LEVELS", "RTC_SPEC_ANY_SPECULAR"]


@pytest.mark.parametrize("specialise", ["0", "1", "2"])
@pytest.mark.parametrize("name", SCENES)
def test_option_lists_are_well_formed(name, specialise, monkeypatch):
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
    for size in ((64, 48), (1024, 512)):
        world, camera = _scene(name, size)
        plan = world.scene_plan(camera)[1]
        options = plan["spec_defs"].split()
        assert options, (name, size)  # every demo scene has objects
        assert all(o.startswith("-D") for o in options), options
        names = [o[2:].split("=", 1)[0] for o in options]
        assert len(set(names)) == len(names), options
        for must in ONCE:
            assert names.count(must) == 1, (must, options)
        assert names.count("RTC_WAVES_PER_SIMD") <= 1
        if specialise == "0":
            assert plan["compile_now"] == "0"
        if specialise == "1":
            assert plan["compile_now"] == "1" or plan["spec_name"] == "render_kernel_spec[any]", plan


# ------------------------------------------------------------------------------------------------- kernel variants
# (rtc_scene_prep.h render_variant / trace_variant / refine_variant: the options are the JIT cache key, in order, and what
# rtc_ctx_*_kernel_id names; the names are what rtc_ctx_*_kernel_name reports)
def _switched_off(options, shapes):
    on = ["-DRTC_SPEC_%s=1" % s for s in shapes]
    return [o[:-1] + "0" if o in on else o for o in options]


def _variant(plan, prefix):
    return plan[prefix + "spec_defs"].split(), plan[prefix + "family_name"], plan[prefix + "spec_name"]


def _with_factor(name, k):
    return name and name[:-1] + ";ss=%d" % k + name[-1]


def _assert_variants_follow(plan, what):
    render, family, spec = _variant(plan, "")
    trace, trace_family, trace_spec = _variant(plan, "trace_")
    assert trace == (_switched_off(render, ("BLOCKS_Y", "RECT", "SHARE")) + ["-DRTC_SPEC_TRACE=1"] if render else []), what
    for name, traced in ((family, trace_family), (spec, trace_spec)):
        assert name == "" or name.startswith("render_kernel"), (what, name)
        assert traced == name.replace("render_", "trace_", 1), (what, traced)
    for k in (2, 4):
        refine, refine_family, refine_spec = _variant(plan, "adaptive%d_" % k)
        assert refine == (trace[:-1] + ["-DRTC_SPEC_ADAPTIVE=%d" % k] if trace else []), (what, k)
        assert refine_family == _with_factor(trace_family.replace("trace_", "adaptive_refine_", 1), k), (what, k, refine_family)
        assert refine_spec == _with_factor(trace_spec.replace("trace_", "adaptive_refine_", 1), k), (what, k, refine_spec)
        ss, ss_family, ss_spec = _variant(plan, "ss%d_" % k)
        assert ss == (_switched_off(render, ("BLOCKS_Y", "RECT")) + ["-DRTC_SPEC_SS=%d" % k] if render else []), (what, k)
        assert ss_family == "ss_" + _with_factor(family, k), (what, k, ss_family)
        assert ss_spec == (spec and "ss_" + _with_factor(spec, k)), (what, k, ss_spec)


@pytest.mark.parametrize("specialise", ["0", "1"])
@pytest.mark.parametrize("name", SCENES)
def test_kernel_variants_follow_the_render_kernel(name, specialise, monkeypatch):
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", specialise)
    world, camera = _scene(name)
    _assert_variants_follow(world.scene_plan(camera)[1], name)


def test_kernel_variants_of_every_launch_shape_and_of_no_objects(monkeypatch):
    """The frames above are thumbnails: the scene rectangle and several blocks per workgroup are for larger ones, and lane
    sharing is not for all.  A world without objects has no options and no scene kernel's name: neither have its variants."""
    seen = set()
    for name, size in (("sphere_grid", (2048, 1536)), ("soft_shadows", (64, 48)), ("sphere_grid", (64, 48))):
        world, camera = _scene(name, size)
        plan = world.scene_plan(camera)[1]
        seen |= {s for s in ("SHARE", "BLOCKS_Y", "RECT") if "-DRTC_SPEC_%s=1" % s in plan["spec_defs"].split()}
        seen |= {"not " + s for s in ("SHARE", "BLOCKS_Y", "RECT") if "-DRTC_SPEC_%s=0" % s in plan["spec_defs"].split()}
        _assert_variants_follow(plan, (name, size))
    assert seen == {"SHARE", "BLOCKS_Y", "RECT", "not SHARE", "not BLOCKS_Y", "not RECT"}, seen
    plan = P.World([], _scene("soft_shadows")[0].light).scene_plan(_scene("soft_shadows")[1])[1]
    assert _variant(plan, "") == ([], "render_kernel<4,simple>", "")
    assert _variant(plan, "trace_") == ([], "trace_kernel<4,simple>", "")
    assert _variant(plan, "adaptive2_") == ([], "adaptive_refine_kernel<4,simple;ss=2>", "")
    assert _variant(plan, "ss4_") == ([], "ss_render_kernel<4,simple;ss=4>", "")
    _assert_variants_follow(plan, "no objects")


def test_kernel_variant_names_of_three_scenes():
    """... and literally, so that the rule above is not only restated."""
    expected = {
        "soft_shadows": ("<4,simple", ">", "_spec[0x402,0x1501,0x1500,0x1500;simple", "]"),
        "hexagons": ("<tree", ">", "_spec[tree;patterns", "]"),
        "mesh": ("<tree", ">", "_spec[tree;patterns", "]"),
    }
    for name, (family, family_end, spec, spec_end) in expected.items():
        world, camera = _scene(name)
        plan = world.scene_plan(camera)[1]
        assert (plan["family_name"], plan["spec_name"]) == ("render_kernel" + family + family_end, "render_kernel" + spec + spec_end)
        assert (plan["trace_family_name"], plan["trace_spec_name"]) == ("trace_kernel" + family + family_end, "trace_kernel" + spec + spec_end)
        for k in ("2", "4"):
            tag = ";ss=" + k
            assert plan["adaptive%s_family_name" % k] == "adaptive_refine_kernel" + family + tag + family_end
            assert plan["adaptive%s_spec_name" % k] == "adaptive_refine_kernel" + spec + tag + spec_end
            assert plan["ss%s_family_name" % k] == "ss_render_kernel" + family + tag + family_end
            assert plan["ss%s_spec_name" % k] == "ss_render_kernel" + spec + tag + spec_end
    world, camera = _scene("soft_shadows")
    plan = world.scene_plan(camera)[1]  # one of them in full
    assert plan["adaptive4_spec_name"] == "adaptive_refine_kernel_spec[0x402,0x1501,0x1500,0x1500;simple;ss=4]"
    assert plan["ss2_family_name"] == "ss_render_kernel<4,simple;ss=2>"
    assert plan["trace_spec_defs"] == (
        "-DRTC_SPEC_LIST=0x402,0x1501,0x1500,0x1500 -DRTC_SPEC_NOBJ=4 -DRTC_SPEC_SIMPLE=1 -DRTC_SPEC_LIGHT_KIND=1 -DRTC_SPEC_JITTER=2 "
        "-DRTC_SPEC_PATTERNS=0 -DRTC_SPEC_GATES=0 -DRTC_LIGHT_VGPRS -DRTC_SPEC_SHARE=0 -DRTC_SPEC_BLOCKS_Y=0 -DRTC_SPEC_RECT=0 "
        "-DRTC_SPEC_LIGHT_ZEROS=46 -DRTC_SPEC_ANY_REFL=1 -DRTC_SPEC_ANY_REFR=0 -DRTC_SPEC_REG_LEVELS=0 -DRTC_SPEC_ANY_SPECULAR=0 -DRTC_SPEC_TRACE=1")


# ---------------------------------------------------------------------------------------- policy switches reach the packing
def _tree_world():
    for seed in range(10):
        world, camera = _small_tree_world(seed, area_light=False)
        if any(isinstance(o, P.GroupShape) and o.leaves() for o in world.objects):
            return world, camera


# switch -> (a scene it governs, the digests that must change there; a scene it has nothing to say about)
SWITCHES = {
    "RTC_AMD_BVH": (lambda: _scene("sphere_grid"), (HDR, RECORDS), lambda: _scene("first_scene")),             # 64 bounded objects / 6
    "RTC_AMD_TRI_PRECULL": (lambda: _scene("mesh"), (HDR, RECORDS), lambda: _scene("hexagons")),               # triangles under groups / none
    "RTC_AMD_PRUNE": (lambda: _scene("hexagons"), (RECORDS,), lambda: _scene("first_scene")),                  # a traversal stream / none
    "RTC_AMD_SCENE_BOX": (lambda: _scene("single_sphere"), (HDR,), lambda: _scene("first_plane")),             # bounded / a plane
    "RTC_AMD_GATES": (_tree_world, (HDR, RECORDS), lambda: _scene("first_scene")),                             # a small tree / no group
    "RTC_AMD_LIGHT_CULL": (lambda: _scene("soft_shadows"), (HDR,), None),                                      # (a header flag in every scene)
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_policy_switches_reach_the_packing(switch, monkeypatch):
    governed, must_change, untouched = SWITCHES[switch]
    world, camera = governed()
    on = world.scene_plan(camera)
    monkeypatch.setenv(switch, "0")
    off = world.scene_plan(camera)
    for k in must_change:
        assert on[0][k] != off[0][k], (switch, k)
    if untouched is not None:
        world, camera = untouched()
        off = world.scene_plan(camera)
        monkeypatch.delenv(switch)
        assert world.scene_plan(camera) == off, switch


# -------------------------------------------------------------------------------------------------- determinism, null camera
@pytest.mark.parametrize("name", SCENES)
def test_two_calls_agree(name):
    """(a stage reading an uninitialised local would show here; the header's padding bytes are part of the contract: the
    context compares headers with memcmp)"""
    for size in ((64, 48), (2048, 1536)):
        world, camera = _scene(name, size)
        assert world.scene_plan(camera) == world.scene_plan(camera)
    assert _scene(name)[0].scene_plan(None) == _scene(name)[0].scene_plan(None)


def _status_and_error(call):
    try:
        call()
        return L.RTC_OK, ""
    except L.RtcError as e:
        return e.status, str(e)


@pytest.mark.parametrize("name", SCENES)
def test_null_camera_follows_scene_validate(name):
    world, _ = _scene(name)
    assert _status_and_error(lambda: world.scene_plan(None)) == _status_and_error(lambda: world.validate(None))
    digests, plan = world.scene_plan(None)
    assert plan == {} and digests[MASKS] == 0
    assert digests[HDR] != 0 and digests[RECORDS] != 0 and digests[TEXELS] != 0


def test_null_camera_refuses_sequence_jitter():
    world, camera, _ = scenes.soft_shadows(64, 48, jitter=("cycle", [0.3, 0.7]))
    for cam in (None, camera):
        got = _status_and_error(lambda: world.scene_plan(cam))
        assert got == _status_and_error(lambda: world.validate(cam))
        assert got[0] == L.RTC_ERR_UNSUPPORTED and "sequence jitter (hardcoded_jitter) is serial across pixels and rays" in got[1], got
