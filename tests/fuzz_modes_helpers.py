"""What tests/test_gpu_fuzz_modes.py (-m gpu) and tests/test_fuzz_modes_plan.py (no GPU) share: the seed list of the random worlds
that go through every mode, the ahead-of-time kernel family the host-only plan gives each of them, and the inputs derived from a
seed -- the adaptive threshold, the lens.  The generators are tests/test_gpu_fuzz.py::_world and tests/wide_worlds.py::world; nothing
of them is copied here."""
import functools
import os

import numpy as np

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from tests import helpers as H
from tests import hits_helpers as HH
from tests import wide_worlds as W
from tests.test_gpu_fuzz import _world

f32 = np.float32
THREADS = min(16, len(os.sched_getaffinity(0)))

# (generator, seed).  The issue's starting list -- fuzz 0..15 and the pinned finds of test_gpu_fuzz.py, wide 0..15: two of each of
# the eight styles -- and the smallest further seeds that bring every ahead-of-time family to two per list (test_fuzz_modes_plan.py
# asserts that on the plan, so that a change of the generators cannot hollow the file out).
FUZZ_SEEDS = list(range(16)) + [2133, 4002, 4003, 9007, 14005]
WIDE_SEEDS = list(range(16))
EXTRA_SEEDS = [("wide", 23)]  # 4,simple: the starting list has wide 7 only
FAMILIES = ("4,simple", "4or8,general", "0,general", "tree", "tree,bvh", "gated")
# the first seed of each family, in the list's order: these run under RTC_AMD_SPECIALIZE=1 as well
SPECIALISED = [("fuzz", 0), ("fuzz", 1), ("fuzz", 2), ("fuzz", 3), ("fuzz", 9007), ("wide", 7)]


def all_seeds():
    return [("fuzz", s) for s in FUZZ_SEEDS] + [("wide", s) for s in WIDE_SEEDS] + list(EXTRA_SEEDS)


@functools.lru_cache(maxsize=None)
def build(gen, seed):
    """One seed, built once for the product's API and once for the oracle's, as the fuzz tests do
    -> {"world", "camera", "own", "depth", "style"}; left unchanged by every test."""
    if gen == "fuzz":
        world, cam, depth = _world(seed, P)
        own, cam_o, _ = _world(seed, O)
        style = "-"
    else:
        world, cam, depth, style = W.world(seed, P)
        own, cam_o, _, _ = W.world(seed, O)
    assert np.array_equal(np.asarray(cam[3], dtype=f32), np.asarray(cam_o[3], dtype=f32))
    return {"world": world, "camera": P.Camera(*cam), "own": own, "depth": depth, "style": style}


def family_of(plan):
    """The ahead-of-time family of a host-only plan made under RTC_AMD_SPECIALIZE=0, as one of FAMILIES."""
    name = plan["family_name"]
    inner = name[name.index("<") + 1:name.rindex(">")]
    if inner.startswith("tree"):
        return inner  # "tree" or "tree,bvh"
    if ";gates" in plan["spec_name"]:
        return "gated"  # a small tree in an unrolled kernel, its group boxes as gates
    if inner in ("4,general", "8,general"):
        return "4or8,general"
    return inner  # "4,simple", "8,simple", "0,general", ...


def plan_family(gen, seed):
    """(RTC_AMD_SPECIALIZE must be 0 in the environment: the caller sets it.)"""
    b = build(gen, seed)
    return family_of(b["world"].scene_plan(b["camera"])[1])


# ---- oracle frames, rendered once per process and left unchanged ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_frame(gen, seed, k):
    """The oracle's frame of the seed's camera (k = 1) or of camera.supersampled(k) -> (frame, rays)."""
    b = build(gen, seed)
    cam = b["camera"] if k == 1 else b["camera"].supersampled(k)
    frame, rays = H.oracle_camera(cam).render(b["own"], b["depth"], threads=THREADS)
    frame.setflags(write=False)
    return frame, rays


def threshold_of(B):
    """The median of the nonzero neighbour differences of a frame, per channel, in f32 as adaptive_helpers.edge_mask takes them;
    0.1 for a frame that has none."""
    B = np.ascontiguousarray(B, dtype=f32)
    with np.errstate(invalid="ignore"):
        d = np.concatenate([np.abs(B[:, 1:] - B[:, :-1]).reshape(-1), np.abs(B[1:] - B[:-1]).reshape(-1)])
    d = d[np.isfinite(d) & (d > 0)]
    return float(np.median(d)) if d.size else 0.1


# ---- the lens of a seed ------------------------------------------------------------------------------------------------------
LENS_SIZE = (24, 16)  # the lens oracle is a Python loop of one color_at per fine ray


@functools.lru_cache(maxsize=None)
def lens_case(gen, seed):
    """-> (camera at LENS_SIZE with the seed's field of view and transform, Lens).  The camera-to-target distance D is the distance
    from the camera to what it looks at: the median first-hit distance of that camera's rays by the oracle (test_gpu_fuzz's cameras
    look at the world's origin, the wide ones at their scene: both are where the hits are), or the camera's distance from the world's
    origin where no ray hits anything.  R = D * 10^u, u uniform so that R / D lies in [0.02, 0.5]; the lens focuses at D."""
    b = build(gen, seed)
    cam = b["camera"]
    camera = P.Camera(LENS_SIZE[0], LENS_SIZE[1], cam.field_of_view, cam.transform)
    o, d = HH.camera_rays(camera)
    hits = HH.oracle_first_hits(b["own"], o, d, light=False)
    dist = hits["distance"][(hits["object"] >= 0) & np.isfinite(hits["distance"]) & (hits["distance"] > 0)]
    D = float(np.median(dist)) if dist.size else float(np.linalg.norm(o[0, :3]))
    if not (np.isfinite(D) and D > 0.0):
        D = 1.0
    rng = np.random.default_rng(555000 + seed + (100000 if gen == "wide" else 0))
    R = D * float(10.0 ** rng.uniform(np.log10(0.02), np.log10(0.5)))
    return camera, P.Lens(R, D, seed=seed)
