"""What every wave does in front of and behind color_at (-m gpu): the pixel's place and image row, the late-loaded arguments of
the canvas store, the DPP sum of the wave's counters and the lane it is stored from (rtc_kernel_core.h: where_is_lane,
image_row, late_args, reduce_wave_counts, store_wave_counts).

Small frames whose tiles are partial -- 13 x 11, 70 x 50, 129 x 65: lanes outside the image, more than one workgroup, no multiple
of a tile -- of soft_shadows (area light: a hundred rays per shade point) and glass_and_mirror (depth 5: lanes of one wave count
very different numbers of rays), and a tree world.  Every frame is compared bit for bit with the oracle's, `rays` and `pixels`
with the oracle's counts, through the scene-compiled kernel as the library chooses it, the same pinned to one lane per pixel (the short form of the wave's
fixed part, whatever the frame's size), the ahead-of-time kernel and a scene kernel pinned to four lanes per pixel (both the earlier
form, RTC_WAVE_FIXED_SHORT 0).
The oracle counts rays, not shade points.  `shaded_hits` is compared with SHADED below: the counts that the library of commit
14c3938 -- the parent of the change this file came with, whose reduce was eighteen __shfl_down -- reported for these frames, the same
from its ahead-of-time and its scene-compiled kernels.  first_scene's count also follows from the oracle's rays (nothing reflects
under a point light: rays = pixels + shaded).

The oracle's frames are rendered once per session and never changed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests import hits_helpers as HH
from tests.supersample_helpers import box_filter

pytestmark = pytest.mark.gpu
f32 = np.float32
THREADS = min(16, len(os.sched_getaffinity(0)))
SWITCHES = ("RTC_AMD_SPECIALIZE", "RTC_AMD_SHARE_LOG2")
SIZES = [(13, 11), (70, 50), (129, 65)]
# "single": small frames under an area light share lanes by the library's own choice, and the lane-sharing kernels keep the earlier
# form -- pinned to one lane per pixel, soft_shadows runs the short form as the large frames do
PATHS = {"scene": {"SPECIALIZE": 1}, "single": {"SPECIALIZE": 1, "SHARE_LOG2": 0}, "aot": {"SPECIALIZE": 0}, "shared": {"SPECIALIZE": 1, "SHARE_LOG2": 2}}
# shade points per frame, recorded from the library of commit 14c3938 (see the head of this file)
SHADED = {("soft_shadows", 13, 11): 80, ("soft_shadows", 70, 50): 2621, ("soft_shadows", 129, 65): 7231,
          ("glass_and_mirror", 13, 11): 319, ("glass_and_mirror", 70, 50): 7942, ("glass_and_mirror", 129, 65): 21346,
          ("hexagons", 64, 32): 2919, ("first_scene", 70, 50): 3381}


@pytest.fixture
def env():
    """Sets / restores the library's switches (read when a context is created; the seam's contexts are dropped)."""
    saved = {k: os.environ.get(k) for k in SWITCHES}

    def set_(**kw):
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            os.environ["RTC_AMD_" + k] = str(v)
        P.lib().rtc_render_release()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    P.lib().rtc_render_release()


_made, _frames = {}, {}


def _scene(name, w, h):
    if (name, w, h) not in _made:
        kw = {"jitter": ("hashed", scenes.DEFAULT_SEED)} if name == "soft_shadows" else {}
        _made[name, w, h] = getattr(scenes, name)(w, h, **kw)
    return _made[name, w, h]


def _oracle(name, w, h, k=1):
    """(frame, rays) of the oracle, k x k box-filtered for k > 1: rendered once, read-only."""
    if (name, w, h, k) not in _frames:
        world, camera, depth = _scene(name, w, h)
        cam = camera.supersampled(k) if k > 1 else camera
        img, rays = H.oracle_camera(cam).render(H.oracle_world(world), depth, threads=THREADS)
        img = box_filter(img, k) if k > 1 else img
        img.setflags(write=False)
        _frames[name, w, h, k] = (img, rays)
    return _frames[name, w, h, k]


def _render_all_paths(name, w, h, env):
    world, camera, depth = _scene(name, w, h)
    exp, rays = _oracle(name, w, h)
    pixels = (w - 1) * (h - 1)
    shaded = {}
    for path, switches in PATHS.items():
        env(**switches)
        r = Renderer(world, camera, device=0)
        for frame in range(3):  # a scene's first frame, and two scheduled by the frames before
            img = r.render(depth).cpu().numpy()
            st = r.stats()
            what = "%s %dx%d %s (%s) frame %d" % (name, w, h, path, r.kernel_name, frame)
            H.assert_images_equal(img, exp, what)
            assert (st["rays"], st["pixels"], st["flags"]) == (rays, pixels, 0), (what, st, rays, pixels)
            shaded[path, frame] = st["shaded_hits"]
            share = int(r._lib.rtc_diag_ctx_share_log2(r._ctx))  # (what the launch took)
            if path == "shared" and name == "soft_shadows":  # (lanes share a pixel's light cells: only under an area light)
                assert share == 2, (what, share)
            if path == "single":
                assert share == 0, (what, share)
        assert ("_spec[" in r.kernel_name) == (switches["SPECIALIZE"] == 1), (path, r.kernel_name)
        r.close()
    assert set(shaded.values()) == {SHADED[name, w, h]}, (shaded, SHADED[name, w, h])
    return rays, pixels, shaded["scene", 0]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["soft_shadows", "glass_and_mirror"])
def test_partial_tiles_on_every_kernel_path(name, size, env):
    _render_all_paths(name, size[0], size[1], env)


def test_shaded_hits_follow_from_the_oracles_rays_where_nothing_reflects(env):
    """first_scene's spheres neither reflect nor transmit, and its light is a point: every traced pixel is one call, every shade
    point one shadow ray -- rays = pixels + shaded, so the oracle's ray count gives its shade points."""
    rays, pixels, shaded = _render_all_paths("first_scene", 70, 50, env)
    assert shaded == rays - pixels


def test_a_tree_world_on_every_kernel_path(env):
    _render_all_paths("hexagons", 64, 32, env)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("band", [1, 3, 8, 24, 64])
@pytest.mark.parametrize("name", ["soft_shadows", "glass_and_mirror"])
def test_partitions_give_the_oracles_rows(name, band, n, env):
    """image_row's three forms -- one part, a band of 2^k rows, any band -- in both kernels: each part's compact rows are those rows
    of the oracle's frame, and the parts' rays add up to the frame's."""
    w, h = 70, 50
    world, camera, depth = _scene(name, w, h)
    exp, rays = _oracle(name, w, h)
    for path in ("scene", "single", "aot"):
        env(**PATHS[path])
        r = Renderer(world, camera, device=0)
        total = 0
        for p in range(n):
            part = r.partition(band, n, p)
            want = [exp[b * band:min((b + 1) * band, h)] for b in range(p, (h + band - 1) // band, n)]
            assert r.rows(part) == sum(len(x) for x in want), (band, n, p)
            if not want:  # (a part that owns no band: nothing is launched)
                continue
            want = np.concatenate(want)
            rows = r.render(depth, part=part).cpu().numpy()
            total += r.stats()["rays"]
            assert rows.shape == want.shape, (path, band, n, p, rows.shape, want.shape)
            H.assert_images_equal(rows, want, "%s %s band %d part %d of %d" % (name, path, band, p, n))
        assert total == rays, (name, path, band, n, total, rays)
        r.close()


@pytest.mark.parametrize("name", ["soft_shadows", "glass_and_mirror"])
def test_the_one_call_seam_reads_its_late_arguments(name, env):
    """rtc_render_ex, f32 and bytes (the progress words, `done`, out_u8), and rtc_render_ss at k = 2, scene kernel and ahead-of-time."""
    w, h = 70, 50
    world, camera, depth = _scene(name, w, h)
    exp, rays = _oracle(name, w, h)
    exp2, rays2 = _oracle(name, w, h, 2)
    for path in ("scene", "aot"):
        env(**PATHS[path])
        for devices, band_rows in (([0], 0), ([0, 0], 16)):
            what = "%s %s devices=%s" % (name, path, devices)
            canvas = camera.render(world, depth, devices=devices, band_rows=band_rows)
            H.assert_images_equal(canvas.data, exp, what)
            assert camera.last_stats["rays"] == rays and camera.last_stats["pixels"] == (w - 1) * (h - 1), (what, camera.last_stats)
            q = camera.render(world, depth, devices=devices, band_rows=band_rows, quantize=True)
            assert q.dtype == np.uint8 and np.array_equal(q, O.quantize(exp)), what
            assert camera.last_stats["rays"] == rays, (what, camera.last_stats)
            canvas = camera.render(world, depth, devices=devices, band_rows=band_rows, supersample=2)
            H.assert_images_equal(canvas.data, exp2, what + " k=2")
            assert camera.last_stats["rays"] == rays2 and camera.last_stats["pixels"] == (2 * w - 1) * (2 * h - 1), (what, camera.last_stats)
            q = camera.render(world, depth, devices=devices, band_rows=band_rows, quantize=True, supersample=2)
            assert np.array_equal(q, O.quantize(exp2)), what + " k=2 bytes"


def test_render_hits_of_the_same_frame(env):
    """rtc_ctx_render_hits: image_row and the primary ray of the core, planes against the oracle's first hits, whole and in bands."""
    w, h = 70, 50
    world, camera, depth = _scene("soft_shadows", w, h)
    o, d = HH.camera_rays(camera)
    traced = np.array([y * w + x for y in range(h - 1) for x in range(w - 1)], dtype=np.int64)
    planes = ("object", "distance", "normal", "light")
    exp = HH.empty_planes(w * h, planes)
    part = HH.oracle_first_hits(H.oracle_world(world), o[traced], d[traced], pixels=traced)
    for k in planes:
        exp[k][traced] = part[k]
    env()
    r = Renderer(world, camera, device=0)
    got = r.render_hits(planes=planes)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().reshape((-1,) + tuple(v.shape[2:])) for k, v in got.items()}
    HH.assert_planes_equal(got, exp, "render_hits 70x50", planes=planes)
    for band, n in ((8, 3), (24, 2)):
        for p in range(n):
            rows = np.concatenate([np.arange(b * band, min((b + 1) * band, h)) for b in range(p, (h + band - 1) // band, n)])
            got = r.render_hits(planes=planes, part=r.partition(band, n, p))
            torch.cuda.synchronize()
            for k in planes:
                g = got[k].cpu().numpy()
                e = exp[k].reshape((h, w) + exp[k].shape[1:])[rows]
                assert g.shape == e.shape and HH.same(g, e).all(), (k, band, n, p)
    r.close()
