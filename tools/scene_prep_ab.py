"""Scene preparation, two builds side by side: do both libraries pack the same bytes and choose the same kernel?

    python tools/scene_prep_ab.py LIB_A LIB_B            (two librtc_amd*.so that export rtc_diag_scene_plan)

For every environment below, each library is loaded in a child process of its own and asked for rtc_diag_scene_plan
(digests of the SceneHdr, the records, the texels, the three tile masks; the plan's text) of: every scene constructor of
scenes.py at four frame sizes and without a camera, the worlds of tests/wide_worlds.py for the seeds
tests/test_gpu_fuzz_wide.py uses (at their own size, and the seeds it also renders at 512 x 384 and 800 x 400), and the
clouds of tests/test_flat_bvh.py.  No GPU is needed.  The two builds must run on ONE machine: the packing calls atan2,
acos, asin, sin, cos in double precision, whose last bit may differ between C libraries, so the digests are compared,
never stored as expected values.  Two development builds (-DRTC_DEV_SWITCHES) also get the development switches.
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ["soft_shadows", "single_sphere", "glass_and_mirror", "sphere_grid", "first_scene", "first_plane", "first_patterns",
          "reflect_refract", "patterns_medley", "hexagons", "grouped_grid", "groups_medley", "mesh", "here_be_dragons",
          "first_textures", "skybox", "shapes_medley"]
SIZES = [(64, 48), (1000, 400), (2048, 1536), (4096, 2048)]
ENVS = [{}, {"RTC_AMD_SPECIALIZE": "0"}, {"RTC_AMD_SPECIALIZE": "1"}, {"RTC_AMD_BVH": "0"}, {"RTC_AMD_TRI_PRECULL": "0"},
        {"RTC_AMD_PRUNE": "0"}, {"RTC_AMD_SCENE_BOX": "0"}, {"RTC_AMD_GATES": "0"}, {"RTC_AMD_LIGHT_CULL": "0"}]
DEV_ENVS = [{"RTC_AMD_CLUSTERS": "1"}, {"RTC_AMD_TREE_WAVES": "6"}, {"RTC_AMD_REG_LEVELS": "2"}, {"RTC_AMD_BLOCKS_Y": "2"}]


def cases():
    """(name, world, camera or None) of everything that is compared."""
    import ray_tracer_challenge_amd as P
    from ray_tracer_challenge_amd import scenes
    from tests import test_flat_bvh as B
    from tests import wide_worlds as W
    for name in SCENES:
        world, camera, _ = getattr(scenes, name)(*SIZES[0])
        yield name + " no camera", world, None
        for w, h in SIZES:
            yield "%s %dx%d" % (name, w, h), world, P.Camera(w, h, camera.field_of_view, camera.transform)
    # tests/test_gpu_fuzz_wide.py: seeds 0 .. 279 at their own size (its first and third test), and the seeds its second and third
    # test also render at 512 x 384 / 800 x 400 -- written inside its parametrize decorators, so copied here: keep them in step
    for seed in range(280):
        world, cam, _, _ = W.world(seed, P)
        yield "wide %d" % seed, world, P.Camera(*cam)
        for seeds, size in (((1, 9, 18, 27, 43, 52, 70, 86), (512, 384)), ((3, 12, 21, 30, 39, 45, 54, 63), (800, 400))):
            if seed in seeds:
                yield "wide %d %dx%d" % ((seed,) + size), world, P.Camera(size[0], size[1], cam[2], cam[3])
    # tests/test_flat_bvh.py: the parameters of its first test, then the clouds its other tests build (copied likewise)
    clouds = [((s, n), dict(duplicates=d, rect_light=r)) for s, n, d, r in
              [(1, 16, 0, False), (2, 23, 4, False), (3, 40, 8, False), (4, 64, 0, True), (5, 31, 6, True), (6, 100, 10, False)]]
    clouds += [((7, 20), {}), ((11, 24), dict(glass=0.6, mirror=0.2, cubes=0.0)), ((21, 80), dict(duplicates=6))]
    for args, kw in clouds:
        world, camera = B._cloud(*args, **kw)
        for w, h in [(camera.width, camera.height)] + ([(1024, 1024), (2048, 1536)] if args[0] == 21 else []):
            yield "cloud %d %dx%d" % (args[0], w, h), world, P.Camera(w, h, camera.field_of_view, camera.transform)


def child(path):
    """One line per case: name | status | the four digests | sha256 of the plan's text | family and kernel names."""
    import ctypes as C
    from ray_tracer_challenge_amd import _lib as L
    lib = L.load(path)
    print("dev_switches %d" % lib.rtc_dev_switches())
    text, digests = C.create_string_buffer(1 << 16), (C.c_uint64 * 4)()
    for name, world, camera in cases():
        cs = world._c()
        st = lib.rtc_diag_scene_plan(C.byref(cs.scene), C.byref(camera._cam) if camera is not None else None, text, len(text), digests)
        plan = dict(ln.split("=", 1) for ln in text.value.decode().splitlines())
        err = lib.rtc_last_error().decode(errors="replace") if st else ""
        print(" | ".join([name, "%d %s" % (st, err), " ".join("%016x" % d for d in digests), hashlib.sha256(text.value).hexdigest()[:16],
                          plan.get("family_name", "-"), plan.get("spec_name", "-"), plan.get("compile_now", "-")]))


def run(path, env):
    e = dict(os.environ)
    for k in list(e):
        if k.startswith("RTC_AMD_"):
            del e[k]
    e.update(env)
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", path], env=e, stdout=subprocess.PIPE, text=True)


def main(a, b):
    print("scene preparation, %s against %s" % (a, b))
    envs, all_equal, e = list(ENVS), True, 0
    while e < len(envs):
        pa, pb = run(a, envs[e]), run(b, envs[e])
        la, lb = pa.communicate()[0].splitlines(), pb.communicate()[0].splitlines()
        assert pa.returncode == 0 and pb.returncode == 0, (pa.returncode, pb.returncode)
        if e == 0 and la[0] == lb[0] == "dev_switches 1":
            envs += DEV_ENVS
        la, lb = la[1:], lb[1:]
        diff = [(x, y) for x, y in zip(la, lb) if x != y]
        equal = len(la) == len(lb) and not diff
        all_equal = all_equal and equal
        with_camera = [ln for ln in la if " no camera" not in ln.split(" | ")[0]]
        print("%-24s %4d cases (%d refused, %d compile_now)  equal: %s  sha256 of A's lines %s" % (
            " ".join("%s=%s" % kv for kv in envs[e].items()) or "default", len(la), sum(not ln.split(" | ")[1].startswith("0") for ln in la),
            sum(ln.endswith("| 1") for ln in with_camera), "yes" if equal else "NO", hashlib.sha256("\n".join(la).encode()).hexdigest()[:16]))
        if len(la) != len(lb):
            print("    A has %d lines, B %d" % (len(la), len(lb)))
        for x, y in diff[:10]:
            print("    A: %s\n    B: %s" % (x, y))
        e += 1
    print("all equal: %s" % all_equal)
    return 0 if all_equal else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) == 3:
        sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])))
    else:
        sys.exit(__doc__)
