"""Frames of worlds with planes, drawn from a scene-tile list (rtc_device.hip use_scene_tile_list): one workgroup per 16 x 16 tile in which
a primary ray can see anything, a zero-fill of the others, one counted ray for each of their traced pixels.  None of it is part of
the reference's semantics: every frame -- the first of a scene (the list in the grid's permuted order), the later ones (longest
first), whole frames and band partitions, after a change of camera -- is bit-equal to the oracle's and to the same context's with
RTC_AMD_SCENE_TILES=0, with the same ray, shaded-hit and pixel counts; and the context says that tiles were in fact left out."""
import ctypes as C

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from oracle import oracle as O
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests.plane_tiles_helpers import case, mirror_balls_at_the_horizon, two_far_balls

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = ["soft_shadows", "glass_and_mirror", "plane_only", "floor_and_wall", "rolled", "under_the_floor", "straight_down", "in_the_plane"]
SIZES = [(192, 128), (320, 256)]
# the first frame in the permuted image order, the second leaves its counts, the third judges them.  (These frames have fewer tiles
# than the device has workgroup slots, so the judgement is "leave the list alone": the order itself is
# test_the_feedback_reorders_a_list_longer_than_the_device_holds's.)
FRAMES = 4
PARTS = (16, 3)


def _env(monkeypatch, tiles):
    for k in ("RTC_AMD_SCENE_BOX", "RTC_AMD_SCENE_RECT", "RTC_AMD_BLOCK_FEEDBACK", "RTC_AMD_GRID_FEEDBACK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", tiles)
    monkeypatch.setenv("RTC_AMD_SHARE_LOG2", "0")  # one lane per pixel: the area light's small frames would share lanes, and lists are for one


def _listed(r, part=None, feedback=False):
    """(tiles listed, fill runs) of the context's list for a partition -- (0, 0): there is none; feedback: ... and how far its feedback is."""
    out = (C.c_uint32 * 3)()
    r._lib.rtc_diag_ctx_scene_tiles(r._ctx, C.byref(part) if part is not None else None, out)
    return (int(out[0]), int(out[1]), int(out[2])) if feedback else (int(out[0]), int(out[1]))


def _frames(r, depth, part=None, n=FRAMES):
    """n frames in a row of one context -> [(image, (rays, shaded hits, pixels))]."""
    got = []
    for _ in range(n):
        img = r.render(depth, part=part).cpu().numpy()
        st = r.stats()
        got.append((img, (st["rays"], st["shaded_hits"], st["pixels"])))
    return got


def _part_rows(height, band, n, p):
    return np.concatenate([np.arange(b * band, min((b + 1) * band, height)) for b in range(p, (height + band - 1) // band, n)] or [np.zeros(0, int)])


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", NAMES)
def test_tile_lists_change_nothing(name, size, monkeypatch):
    world, camera, depth = case(name, size)
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=8)
    everything = name in ("straight_down", "in_the_plane")
    band, n_parts = PARTS
    results = {}
    for tiles in ("0", "2"):
        _env(monkeypatch, tiles)
        r = Renderer(world, camera, device=0)
        whole = _frames(r, depth)
        n_listed, n_fill, feedback = _listed(r, feedback=True)
        parts = []
        for p in range(n_parts):
            q = Renderer.partition(band, n_parts, p)
            parts.append((_frames(r, depth, part=q), _listed(r, q)))
        r.close()
        results[tiles] = (whole, parts)
        tw, th = (size[0] + 15) // 16, (size[1] + 15) // 16
        if tiles == "0" or everything:
            assert (n_listed, n_fill) == (0, 0), (name, tiles)
        else:  # the path was taken: a list shorter than the frame, and runs of tiles to fill
            assert 0 < n_listed < tw * th and n_fill > 0, (name, n_listed, n_fill)
            assert feedback == 2  # the second frame's counts have been read and judged: all tiles start at once, the list stays
            assert sum(l[0] for _, l in parts) == n_listed
        for i, (img, counts) in enumerate(whole):
            H.assert_images_equal(img, exp, "%s tiles=%s frame %d" % (name, tiles, i))
            assert counts[0] == rays and counts == whole[0][1], (name, tiles, i, counts, rays)
        part_rays = 0
        for p, (frames, _) in enumerate(parts):
            ys = _part_rows(size[1], band, n_parts, p)
            for i, (img, counts) in enumerate(frames):
                H.assert_images_equal(img, exp[ys], "%s tiles=%s part %d frame %d" % (name, tiles, p, i))
                assert counts == frames[0][1]
            part_rays += frames[0][1][0]
        assert part_rays == rays
    # ... and the two contexts agree count by count
    assert results["0"][0][0][1] == results["2"][0][0][1]
    for a, b in zip(results["0"][1], results["2"][1]):
        assert a[0][0][1] == b[0][0][1]


def _seam_listed():
    """_listed for the context the one-call seam keeps for its first device (its frames are the partition {64, 1, 0})."""
    lib = L.lib()
    out = (C.c_uint32 * 3)()
    lib.rtc_diag_ctx_scene_tiles(lib.rtc_diag_seam_ctx(0), None, out)
    return int(out[0]), int(out[1]), int(out[2])


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", NAMES)
def test_quantized_frames(name, size, monkeypatch):
    """Frames of bytes leave through the one-call seam, whose rows are reported chunk by chunk: worlds with planes stay on the grid
    there whatever RTC_AMD_SCENE_TILES says, and the bytes are the oracle's, four frames in a row."""
    world, camera, depth = case(name, size)
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=8)
    want = np.asarray(O.quantize(exp)).reshape(size[1], size[0], 3)
    counts = set()
    for tiles in ("0", "2"):
        _env(monkeypatch, tiles)
        for i in range(FRAMES):
            img = camera.render(world, depth, quantize=True)
            assert (img == want).all(), (name, tiles, i)
            counts.add((camera.last_stats["rays"], camera.last_stats["shaded_hits"], camera.last_stats["pixels"]))
        assert _seam_listed()[:2] == (0, 0)
    assert len(counts) == 1 and counts.pop()[0] == rays


@pytest.mark.parametrize("quantize", [True, False], ids=["u8", "f32"])
def test_seam_frames_drawn_from_a_list(quantize, monkeypatch):
    """A sparse bounded world (plane_tiles_helpers.two_far_balls) IS drawn from its list through the seam: bytes and floats, four
    frames, the list in the permuted order, no feedback where rows are reported (its state stays 0)."""
    world, camera, depth = two_far_balls()
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=8)
    want = np.asarray(O.quantize(exp)).reshape(exp.shape) if quantize else exp
    for tiles in ("0", "1"):
        _env(monkeypatch, tiles)
        for i in range(FRAMES):
            got = camera.render(world, depth, quantize=quantize)
            img = got if quantize else got.data
            H.assert_images_equal(img, want, "tiles=%s frame %d" % (tiles, i))
            assert camera.last_stats["rays"] == rays
        n_listed, n_fill, feedback = _seam_listed()
        if tiles == "0":
            assert (n_listed, n_fill) == (0, 0)
        else:
            assert 0 < n_listed < 20 * 16 // 3 and n_fill > 0 and feedback == 0, (n_listed, n_fill, feedback)


def test_the_list_follows_the_camera(monkeypatch):
    """Renderer.set_camera between frames: the mask, the list and its order are the new camera's."""
    world, camera, depth = case("rolled", (320, 256))
    _, other, _ = case("under_the_floor", (320, 256))
    _, down, _ = case("straight_down", (320, 256))
    _env(monkeypatch, "2")
    r = Renderer(world, camera, device=0)
    ow = H.oracle_world(world)
    seen = []
    for cam in (camera, other, camera, down, other):
        r.set_camera(cam)
        exp, rays = H.oracle_camera(cam).render(ow, depth, threads=8)
        for i, (img, counts) in enumerate(_frames(r, depth, n=3)):
            H.assert_images_equal(img, exp, "camera %d frame %d" % (len(seen), i))
            assert counts[0] == rays
        seen.append(_listed(r))
    r.close()
    assert seen[0] == seen[2] and seen[1] == seen[4] and seen[0] != seen[1]
    assert seen[3] == (0, 0) and seen[0][0] > 0 and seen[1][0] > 0


def test_the_feedback_reorders_a_list_longer_than_the_device_holds(monkeypatch):
    """plane_tiles_helpers.mirror_balls_at_the_horizon: the second frame's counts make the third and fourth start their tiles longest
    first (feedback state 3: the list on the device was replaced), and they are the same frames, count for count."""
    world, camera, depth = mirror_balls_at_the_horizon()
    exp, rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=8)
    _env(monkeypatch, "2")
    r = Renderer(world, camera, device=0)
    states, frames = [], []
    for _ in range(FRAMES):
        frames += _frames(r, depth, n=1)
        states.append(_listed(r, feedback=True))
    r.close()
    print("(listed, fill runs, feedback) after each frame:", states)
    assert [s[2] for s in states] == [0, 1, 3, 3] and len({s[:2] for s in states}) == 1 and 2610 < states[0][0] < 80 * 60
    for i, (img, counts) in enumerate(frames):
        H.assert_images_equal(img, exp, "frame %d" % i)
        assert counts[0] == rays and counts == frames[0][1]
