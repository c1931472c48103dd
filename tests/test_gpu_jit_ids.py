"""The ids and cache files of a scene's kernels on the device are those the host plans (csrc/rtc_jit.h plan_jit, printed by
rtc_diag_scene_plan; tests/test_jit_plan.py pins their formula without a GPU).

One child process -- compiled kernels are remembered per process, and only a process that has none writes every one of them into
its cache directory -- with RTC_AMD_SPECIALIZE=1 and an empty RTC_AMD_JIT_CACHE: a frame of 64 x 48 soft_shadows at depth 5, its
camera's rays as a stream, an adaptive frame at k = 2 and a frame at depth 12, i.e. four compiles of that scene's kernel.
rtc_ctx_kernel_id keeps naming the frame's own kernel after the depth-12 frame, so that frame's kernel -- the same options with a
stack of 16 levels -- is identified by its cache file, whose stem is an id's first half.  Then RTC_AMD_SPECIALIZE=0.
"""
import json
import os
import subprocess
import sys
import textwrap

import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %(root)r)
    from ray_tracer_challenge_amd import scenes
    from ray_tracer_challenge_amd.renderer import Renderer
    world, camera, depth = scenes.soft_shadows(64, 48)
    assert depth == 5
    seen = {}
    os.environ["RTC_AMD_SPECIALIZE"] = "1"
    seen["plan"] = world.scene_plan(camera)[1]
    r = Renderer(world, camera, device=0)
    r.render(depth)
    seen["render"] = r.kernel_id
    o, d, k = r.camera_rays()
    r.trace(o, d, depth, keys=k)
    seen["trace"] = r.trace_kernel_id
    r.render_adaptive(depth, k=2, threshold=0.05)
    seen["adaptive2"], seen["refined"] = r.adaptive_kernel_id, r.adaptive_stats()["refined_pixels"]
    r.render(12).cpu()
    seen["after_deep"] = r.kernel_id
    seen["files"] = sorted(os.listdir(os.environ["RTC_AMD_JIT_CACHE"]))
    r.close()
    os.environ["RTC_AMD_SPECIALIZE"] = "0"
    seen["plan0"] = world.scene_plan(camera)[1]
    r = Renderer(world, camera, device=0)
    r.render(depth).cpu()
    seen["aot"], seen["aot_name"] = r.kernel_id, r.kernel_name
    r.close()
    seen["files0"] = sorted(os.listdir(os.environ["RTC_AMD_JIT_CACHE"]))
    print(json.dumps(seen))
""")


@gpu
def test_ids_and_cache_files_are_the_planned_ones(tmp_path):
    script = tmp_path / "ids.py"
    script.write_text(_CHILD % {"root": ROOT})
    cache = tmp_path / "cache"
    cache.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTC_AMD_")}
    env["RTC_AMD_JIT_CACHE"] = str(cache)
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    seen = json.loads(p.stdout.strip().splitlines()[-1])
    plan = seen["plan"]
    stem = lambda key: plan[key][:-len(".hsaco")]
    planned = [plan[key] for key in ("cache_file", "trace_cache_file", "adaptive2_cache_file", "deep16_cache_file")]
    assert all(f.startswith("spec_") and f.endswith(".hsaco") and len(f) == 27 for f in planned) and len(set(planned)) == 4, planned
    for what, key in (("render", "cache_file"), ("trace", "trace_cache_file"), ("adaptive2", "adaptive2_cache_file"), ("after_deep", "cache_file")):
        first, _, second = seen[what].partition(".")
        assert first == stem(key), (what, seen[what], plan[key])
        assert len(second) == 8 and int(second, 16) >= 0, seen[what]  # the code object's checksum
    assert seen["refined"] > 0  # (the refinement had work to do)
    assert seen["files"] == sorted(planned), (seen["files"], planned)  # the depth-12 frame's kernel among them, by its name
    # never: the ahead-of-time kernel, named by its source
    assert seen["aot_name"] == seen["plan0"]["family_name"] == "render_kernel<4,simple>"
    assert seen["aot"] == seen["plan0"]["aot_id"] == plan["aot_id"] and seen["aot"].startswith("aot_") and len(seen["aot"]) == 20
    assert seen["files0"] == seen["files"]
