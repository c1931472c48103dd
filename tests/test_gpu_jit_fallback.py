"""A ray stream's and a refinement's scene kernel that hiprtc does not deliver (rtc_device.hip scene_kernel_for), as
tests/test_seam.py::test_failed_scene_compile_is_reported_not_hidden has it for the frame's: under the default policy the call
succeeds with the ahead-of-time kernel -- same image, its name reported, one line on stderr per process unless RTC_AMD_QUIET --
and under RTC_AMD_SPECIALIZE=1 it returns the error.

The compile is made to fail with the development library's RTC_AMD_JIT_FLAGS, by a definition that breaks rtc_trace.h's or
rtc_adaptive.h's text only: the frame's kernel still compiles, so that the context exists and the base frame is rendered.  The
scene is an area light over divided meshes: those are compiled whatever the number of rays (ScenePlan::compile_any_size), 32 x 32
included.  A context reads the environment when it is created, so one child process -- the warning is once per process -- makes
one context per setting.
"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ray_tracer_challenge_amd import _lib as L

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %(root)r)
    import numpy as np
    import ray_tracer_challenge_amd as P
    from ray_tracer_challenge_amd import api, scenes
    from ray_tracer_challenge_amd.renderer import Renderer
    from ray_tracer_challenge_amd.scenes import RectangleLight, color, point, vector
    mode, out_dir = sys.argv[1], sys.argv[2]
    light = RectangleLight(color(1.5, 1.5, 1.5), point(-1, 4, -4), vector(2, 0, 0), 4, vector(0, 2, 0), 4, ("hashed", scenes.DEFAULT_SEED))
    world = P.World(scenes.mesh_objects(api), light)
    camera, depth = scenes.mesh(32, 32)[1:]
    seen = []
    for phase, env in enumerate([{}] + json.loads(sys.argv[3])):
        for name in ("RTC_AMD_SPECIALIZE", "RTC_AMD_QUIET"):
            os.environ.pop(name, None)
        os.environ.update(env)
        if not seen:  # (the default policy's plan, before any context)
            seen.append({"compile_now": world.scene_plan(camera)[1]["compile_now"]})
            continue
        phase -= 1
        sys.stderr.write("\\n== phase %%d\\n" %% phase)
        sys.stderr.flush()
        r = Renderer(world, camera, device=0)
        try:
            if mode == "trace":
                o, d, k = r.camera_rays()
                img = r.trace(o, d, depth, keys=k).cpu().numpy()
                info = {"kernel": r.trace_kernel_name, "flags": r.stats()["flags"]}
            else:
                img = r.render_adaptive(depth, k=2, threshold=0.05).cpu().numpy()
                info = {"kernel": r.adaptive_kernel_name, "refined": r.adaptive_stats()["refined_pixels"]}
            np.save(os.path.join(out_dir, "%%d.npy" %% phase), img)
            info.update({"render": r.kernel_name, "jit_status": r.jit_status})
        except P.RtcError as e:
            info = {"error": str(e)[:300]}
        seen.append(info)
        r.close()
    print(json.dumps(seen))
""")
# (one context each, in this order: the quiet one must not use the process's one warning up)
PHASES = [{"RTC_AMD_QUIET": "1"}, {}, {}, {"RTC_AMD_SPECIALIZE": "1"}, {"RTC_AMD_SPECIALIZE": "0"}]
QUIET, DEFAULT, AGAIN, FORCED, NEVER = range(5)


def _run(tmp_path, mode, breaks):
    script = tmp_path / "fallback.py"
    script.write_text(_CHILD % {"root": ROOT})
    env = dict(os.environ, RTC_AMD_LIB=L.DEV_LIB_PATH, RTC_AMD_JIT_FLAGS="-D%s=:" % breaks, RTC_AMD_JIT_CACHE=str(tmp_path / "cache"))
    p = subprocess.run([sys.executable, str(script), mode, str(tmp_path), json.dumps(PHASES)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    seen = json.loads(p.stdout.strip().splitlines()[-1])
    assert seen[0]["compile_now"] == "1", seen[0]  # the policy wants this scene's kernels at any size
    stderr = p.stderr.split("\n== phase ")[1:]
    assert len(stderr) == len(PHASES)
    images = [np.load(tmp_path / ("%d.npy" % i)) if (tmp_path / ("%d.npy" % i)).exists() else None for i in range(len(PHASES))]
    return seen[1:], stderr, images


def _check(seen, stderr, images, doing, family):
    line = "librtc_amd: scene specialisation unavailable, %s the slower ahead-of-time kernel" % doing
    for phase in (QUIET, DEFAULT, AGAIN, NEVER):
        assert "error" not in seen[phase], (phase, seen[phase])
        assert seen[phase]["kernel"] == family, (phase, seen[phase])                   # the ahead-of-time family's name
        assert seen[phase]["render"] == "render_kernel_spec[tree;patterns]" or phase == NEVER, seen[phase]   # (the frame's kernel compiled)
        assert seen[phase]["jit_status"] == "", seen[phase]                            # ... and rtc_ctx_jit_status speaks of that one only
        assert images[phase] is not None and np.isfinite(images[phase]).all() and images[phase].any()
        assert np.array_equal(images[phase].view(np.uint32), images[NEVER].view(np.uint32)), phase
    assert stderr[DEFAULT].count(line) == 1 and "failed to compile" in stderr[DEFAULT], stderr[DEFAULT][-600:]
    for phase in (QUIET, AGAIN, FORCED, NEVER):                                        # silence under the quiet policy; once per process
        assert "librtc_amd:" not in stderr[phase], (phase, stderr[phase][-600:])
    assert "failed to compile" in seen[FORCED].get("error", ""), seen[FORCED]          # explicitly requested: an error
    assert images[FORCED] is None


@gpu
def test_a_ray_streams_failed_scene_compile_is_reported_not_hidden(tmp_path):
    seen, stderr, images = _run(tmp_path, "trace", "TraceArgs")
    _check(seen, stderr, images, "tracing with", "trace_kernel<tree>")
    assert "trace_kernel<tree>: " in stderr[DEFAULT]                                   # the line names the kernel that traces instead
    for phase in (QUIET, DEFAULT, AGAIN):
        assert seen[phase]["flags"] & L.RTC_STATS_JIT_FALLBACK, (phase, seen[phase])   # rtc_ctx_stats after a trace: the trace's note
    assert seen[NEVER]["flags"] == 0


@gpu
def test_a_refinements_failed_scene_compile_is_reported_not_hidden(tmp_path):
    seen, stderr, images = _run(tmp_path, "adaptive", "AdaptiveRefineArgs")
    _check(seen, stderr, images, "refining with", "adaptive_refine_kernel<tree;ss=2>")
    assert seen[DEFAULT]["refined"] > 0 and seen[DEFAULT]["refined"] == seen[NEVER]["refined"], seen  # (the refinement has work to do)
