"""One context across changes of mode and scene (-m gpu): what a context keeps for life and what a scene replaces
(csrc/rtc_device.hip, the inventory at the head of rtc_ctx; DESIGN.md "What a context keeps").

A characterisation test: one Renderer is driven through plain -> trace (plain and reordered) -> adaptive k=2 ->
set_scene_ss k=2 -> set_scene_lens k=2 -> a plain scene with an area light.  After every step the result is bit-equal to the
same call on a fresh context, and after every set_scene the context reports exactly what it reported when this test was written:
the per-scene names are empty again, and the statistics are the ones the last launches before the scene change left behind (they
outlive the scene -- on purpose or not, they are pinned here as they are).  Times (the *_ms fields) are not compared.

Two 32 x 32 scenes, one process, about two seconds on an MI355X."""
import os

import numpy as np
import pytest
import torch

from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.api import Lens
from ray_tracer_challenge_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
SWITCHES = ("RTC_AMD_SPECIALIZE", "RTC_AMD_BLOCK_FEEDBACK", "RTC_AMD_SHARE_LOG2", "RTC_AMD_BLOCK_LIST")
SIZE = 32
K = 2
THRESHOLD = 0.1
LENS = Lens(0.05, 4.0, seed=7)


@pytest.fixture
def default_switches():
    """The library's switches at their defaults (they are read when a context is created)."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def _bits(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d words differ from a fresh context's" % (what, int((got != want).sum()))


def _counts(stats):
    return {k: v for k, v in stats.items() if not k.endswith("_ms")}


def _state(r):
    return {"trace_kernel_name": r.trace_kernel_name, "adaptive_kernel_name": r.adaptive_kernel_name, "adaptive": _counts(r.adaptive_stats()),
            "reorder": _counts(r.reorder_stats()), "stats": _counts(r.stats())}


# What the context reports right after each rtc_ctx_set_scene* of the sequence, recorded from the code as it stood when the test was
# written.  The adaptive and reorder statistics are those of the calls made under the FIRST scene setting; rtc_ctx_stats reports the
# last render before the change (its rows, pixels and counters) and the launches since the statistics were last read.
ADAPTIVE_LEFT = {"refined_pixels": 277, "rays": 8906, "shaded_hits": 3457, "culled_shadow_rays": 0}
REORDER_LEFT = {"n": SIZE * SIZE}
EXPECTED = {
    # the adaptive call's base frame: its rows and traced pixels (31 x 31), two launches since the statistics were last read
    "set_scene_ss": {"trace_kernel_name": "", "adaptive_kernel_name": "", "adaptive": ADAPTIVE_LEFT, "reorder": REORDER_LEFT,
                     "stats": {"rays": 5473, "shaded_hits": 1986, "pixels": 961, "launches": 2, "rows": 32, "culled_shadow_rays": 0, "flags": 0}},
    # the supersampled frame: output rows, but the FINE frame's traced pixels (63 x 63)
    "set_scene_lens": {"trace_kernel_name": "", "adaptive_kernel_name": "", "adaptive": ADAPTIVE_LEFT, "reorder": REORDER_LEFT,
                       "stats": {"rays": 22847, "shaded_hits": 8318, "pixels": 3969, "launches": 1, "rows": 32, "culled_shadow_rays": 0, "flags": 0}},
    # the lens frame
    "set_scene": {"trace_kernel_name": "", "adaptive_kernel_name": "", "adaptive": ADAPTIVE_LEFT, "reorder": REORDER_LEFT,
                  "stats": {"rays": 22890, "shaded_hits": 8336, "pixels": 3969, "launches": 1, "rows": 32, "culled_shadow_rays": 0, "flags": 0}},
}


def _check_state(r, step):
    got = _state(r)
    print("state after %s: %r" % (step, got))
    assert got == EXPECTED[step], step


def test_one_context_through_modes_and_scenes(default_switches):
    world_a, camera_a, depth_a = scenes.glass_and_mirror(SIZE, SIZE)  # flat, a point light, reflection and refraction
    world_b, camera_b, depth_b = scenes.soft_shadows(SIZE, SIZE)      # an area light
    r = Renderer(world_a, camera_a, device=0)

    # plain
    fresh = Renderer(world_a, camera_a, device=0)
    _same(r.render(depth_a), fresh.render(depth_a), "plain")
    # trace: the camera's own rays, as they are and reordered
    fresh = Renderer(world_a, camera_a, device=0)
    origins, directions, keys = fresh.camera_rays()
    want = fresh.trace(origins, directions, depth_a, keys=keys)
    _same(r.trace(origins, directions, depth_a, keys=keys), want, "trace")
    assert r.trace_kernel_name != ""
    _same(r.trace(origins, directions, depth_a, keys=keys, reorder=True), want, "reordered trace")
    # adaptive k = 2
    fresh = Renderer(world_a, camera_a, device=0)
    want, want_mask = fresh.render_adaptive(depth_a, k=K, threshold=THRESHOLD, mask=True)
    got, got_mask = r.render_adaptive(depth_a, k=K, threshold=THRESHOLD, mask=True)
    _same(got, want, "adaptive")
    torch.cuda.synchronize()
    assert torch.equal(got_mask, want_mask)
    assert r.adaptive_kernel_name != "" and r.adaptive_kernel_name == fresh.adaptive_kernel_name
    # supersampled k = 2
    r.set_scene(world_a, camera_a, supersample=K)
    _check_state(r, "set_scene_ss")
    fresh = Renderer(world_a, camera_a, device=0, supersample=K)
    _same(r.render(depth_a), fresh.render(depth_a), "supersampled")
    # through a lens, k = 2
    r.set_scene(world_a, camera_a, supersample=K, lens=LENS)
    _check_state(r, "set_scene_lens")
    fresh = Renderer(world_a, camera_a, device=0, supersample=K, lens=LENS)
    _same(r.render(depth_a), fresh.render(depth_a), "lens")
    # another scene, plain
    r.set_scene(world_b, camera_b)
    _check_state(r, "set_scene")
    fresh = Renderer(world_b, camera_b, device=0)
    _same(r.render(depth_b), fresh.render(depth_b), "plain, the second scene")
    assert r.kernel_name == fresh.kernel_name and r.kernel_id == fresh.kernel_id
    assert _counts(r.stats()) == _counts(fresh.stats())
