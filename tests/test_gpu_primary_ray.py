"""One world, four kernels, one primary ray per pixel (-m gpu): render_body, wf_trace_kernel<true>, hits_kernel and
ss_render_body all take a pixel's ray and the scene-box early-out from the same device function, and its image row from
the same expression (csrc/rtc_kernel_core.h: primary_ray, image_row -- written out in ss_render_body), and must agree on every
pixel -- whole frames and partitions.

sphere_grid is fully bounded (has_scene_box is set: the early-out is live) and a tree world (RTC_AMD_WAVEFRONT=1 applies).
The frame is 52 x 36: no multiple of the 16 x 16 block, divisible by 2 and 4."""
import os

import numpy as np
import pytest
import torch

from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.renderer import Renderer
from ray_tracer_challenge_amd.scenes import PI, Camera, f32, point, vector, view_transform
from tests import helpers as H
from tests import hits_helpers as HH
from tests.supersample_helpers import assemble_partitions, box_filter

pytestmark = pytest.mark.gpu
W, HEIGHT, BAND_ROWS, N_PARTS = 52, 36, 7, 3
THREADS = min(16, len(os.sched_getaffinity(0)))


def _camera(w, h):
    # low over the grid, so that the rows of spheres overlap: well over a third of the pixels see a sphere, the sky above sees nothing
    return Camera(w, h, PI / f32(5.0), view_transform(point(1, 0.8, -2.5), point(0, 0.4, 7), vector(0, 1, 0)))


@pytest.fixture(scope="module")
def case():
    """World, camera, depth; the oracle's frame, ray count and object plane (-1: a miss).  Computed once, left unchanged."""
    world, _, depth = scenes.sphere_grid(W, HEIGHT)
    camera = _camera(W, HEIGHT)
    own = H.oracle_world(world)
    frame, rays = H.oracle_camera(camera).render(own, depth, threads=THREADS)
    origins, directions = HH.camera_rays(camera)
    obj = HH.oracle_first_hits(own, origins, directions, light=False)["object"].reshape(HEIGHT, W).copy()
    obj[-1, :] = -1  # camera.rs:80-81: the last row and column are never traced
    obj[:, -1] = -1
    misses, hits = int((obj < 0).sum()), int((obj >= 0).sum())
    assert 4 * misses >= W * HEIGHT and 4 * hits >= W * HEIGHT, (misses, hits)  # (a camera change must not hollow the test out)
    return world, camera, depth, frame, rays, obj


def _parts():
    return [None] + [[Renderer.partition(BAND_ROWS, N_PARTS, p) for p in range(N_PARTS)]]


def _render(world, camera, depth, parts, wavefront, monkeypatch, supersample=1):
    """-> (frame, rays, kernel name): whole (parts None), or every partition rendered and put back together."""
    monkeypatch.setenv("RTC_AMD_WAVEFRONT", "1" if wavefront else "0")
    r = Renderer(world, camera, device=0, supersample=supersample)
    rays = 0
    if parts is None:
        frame = r.render(depth).cpu().numpy()
        rays = r.stats()["rays"]
    else:
        pieces = []
        for part in parts:
            if r.rows(part) == 0:  # (the 9-row frame has two bands: the third partition owns nothing)
                pieces.append(np.zeros((0, r.width, 3), dtype=np.float32))
                continue
            pieces.append(r.render(depth, part=part).cpu().numpy())
            rays += r.stats()["rays"]
        frame = assemble_partitions(pieces, camera.height, BAND_ROWS, N_PARTS)
    name = r.kernel_name
    r.close()
    return frame, rays, name


@pytest.mark.parametrize("parts", _parts(), ids=["whole", "parts"])
def test_per_pixel_and_wavefront_frames_are_the_oracles(case, parts, monkeypatch):
    world, camera, depth, exp, exp_rays, _ = case
    pp, pp_rays, pp_name = _render(world, camera, depth, parts, False, monkeypatch)
    wf, wf_rays, wf_name = _render(world, camera, depth, parts, True, monkeypatch)
    assert wf_name.startswith("wavefront[") and not pp_name.startswith("wavefront["), (pp_name, wf_name)
    H.assert_images_equal(pp, wf, "per-pixel against wavefront")
    H.assert_images_equal(pp, exp, "per-pixel against the oracle")
    H.assert_images_equal(wf, exp, "wavefront against the oracle")
    assert pp_rays == wf_rays, (pp_rays, wf_rays)
    if parts is None:
        assert pp_rays == exp_rays, (pp_rays, exp_rays)


@pytest.mark.parametrize("parts", _parts(), ids=["whole", "parts"])
def test_the_object_plane_misses_exactly_where_the_oracle_does(case, parts, monkeypatch):
    world, camera, _, _, _, exp_obj = case
    monkeypatch.delenv("RTC_AMD_WAVEFRONT", raising=False)
    r = Renderer(world, camera, device=0)
    if parts is None:
        got = r.render_hits(planes=("object",))["object"]
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    else:
        got = np.full((HEIGHT, W), -2, dtype=np.int32)
        bands = [range(y0, min(y0 + BAND_ROWS, HEIGHT)) for y0 in range(0, HEIGHT, BAND_ROWS)]
        for p, part in enumerate(parts):
            plane = r.render_hits(planes=("object",), part=part)["object"]
            torch.cuda.synchronize()
            rows = [y for b, band in enumerate(bands) if b % N_PARTS == p for y in band]  # band b belongs to part b mod N_PARTS
            assert plane.shape == (len(rows), W), (plane.shape, len(rows))
            got[rows] = plane.cpu().numpy()
        assert (got != -2).all()
    r.close()
    assert ((got == -1) == (exp_obj == -1)).all(), np.argwhere((got == -1) != (exp_obj == -1))[:8]


@pytest.mark.parametrize("parts", _parts(), ids=["whole", "parts"])
@pytest.mark.parametrize("k", [2, 4])
def test_supersampled_frames_are_the_box_filter_of_the_per_pixel_frame(case, k, parts, monkeypatch):
    world, camera, depth, _, _, _ = case
    fine, fine_rays, _ = _render(world, camera, depth, None, False, monkeypatch)
    got, rays, name = _render(world, _camera(W // k, HEIGHT // k), depth, parts, False, monkeypatch, supersample=k)
    assert name.startswith("ss_render_kernel"), name
    H.assert_images_equal(got, box_filter(fine, k), "supersample=%d against the filtered per-pixel frame" % k)
    assert rays == fine_rays, (rays, fine_rays)
