"""Scene tiles for worlds with planes, on the host (csrc/rtc_scene_prep.h plan_coverage, csrc/rtc_launch_plan.h) -- no device needed.

The scene-tile mask says in which 16 x 16 tiles of the frame a primary ray can see anything: the tiles some bounded entry's padded box
projects to, and for every top-level plane the tiles with a corner on the side of its horizon where rays point towards it
(mark_plane_tiles).  Frames are then one workgroup per listed tile and a zero-fill of the others, whose pixels are counted as one ray
each.  That is right exactly if the reference renders every traced pixel of an unseen tile black after a single ray, which is what
the oracle is asked here, pixel by pixel.  The list's two orders (first frame: the grid's permutation; later frames: longest first)
must be permutations of the image-order list, and list + fill runs must cover a partition's pixels exactly once."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_tracer_challenge_amd as P
from ray_tracer_challenge_amd import _lib as L
from tests import helpers as H
from tests.plane_tiles_helpers import CASES, _ball, case, two_far_balls

U32P = C.POINTER(C.c_uint32)


@pytest.fixture(autouse=True)
def _library_defaults(monkeypatch):
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "2")  # whenever the mask leaves any tile out: these frames are small


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a):
    return a.ctypes.data_as(U32P)


_oracle = {}


def oracle_frame(name, size):
    """(image, rays) of a case, rendered once."""
    if (name, size) not in _oracle:
        world, camera, depth = case(name, size)
        img, rays = H.oracle_camera(camera).render(H.oracle_world(world), depth, threads=8)
        img.setflags(write=False)
        _oracle[(name, size)] = (img, rays)
    return _oracle[(name, size)]


@pytest.mark.parametrize("name,size,least", CASES, ids=["%s-%dx%d" % (n, s[0], s[1]) for n, s, _ in CASES])
def test_unseen_tiles_are_black_after_one_ray(name, size, least):
    world, camera, depth = case(name, size)
    mask = world.scene_tile_mask(camera)
    if least is None:  # nothing can be left out: no mask at all, or one that marks everything
        assert mask is None or mask.all(), name
        return
    assert mask is not None, name
    w, h = size
    unseen_tiles = int((~mask).sum())
    print("%s %dx%d: %d of %d tiles unseen" % (name, w, h, unseen_tiles, mask.size))
    assert unseen_tiles >= 1 and unseen_tiles >= least * mask.size, (name, unseen_tiles, mask.size)
    img, _ = oracle_frame(name, size)
    unseen = np.repeat(np.repeat(~mask, 16, axis=0), 16, axis=1)[:h, :w].copy()
    unseen[h - 1:, :] = False  # the last row and column are not traced (camera.rs:80-81)
    unseen[:, w - 1:] = False
    assert not img[unseen].any(), "%s: %d channel values of unseen tiles are not black" % (name, int((img[unseen] != 0).sum()))
    # ... and each of those pixels is exactly one ray: the frame's count is the listed tiles' rays + one per traced pixel outside them
    ow, oc = H.oracle_world(world), H.oracle_camera(camera)
    for y, x in np.argwhere(unseen):
        before = ow.ray_count
        ow.set_pixel(int(y) * w + int(x))
        o, d = oc.ray_for_pixel(int(x), int(y))
        assert not ow.color_at(o, d, depth).any()
        assert ow.ray_count - before == 1, (name, x, y)


def test_the_mask_marks_every_tile_the_oracle_lights():
    """The other direction, as a sanity check of the cases themselves: the frames are not black."""
    for name, size, least in CASES:
        img, _ = oracle_frame(name, size)
        assert img.any(), name


def test_plane_side_follows_the_camera():
    """A rolled camera's horizon is a slanted line: the unseen tiles are not a rectangle's complement -- some tile row has both."""
    world, camera, _ = case("rolled", (320, 256))
    mask = world.scene_tile_mask(camera)
    rows_with_both = [r for r in range(mask.shape[0]) if mask[r].any() and not mask[r].all()]
    assert len(rows_with_both) >= 3
    firsts = {int(np.argmax(mask[r])) if mask[r][0] == 0 else int(np.argmin(mask[r])) for r in rows_with_both}
    assert len(firsts) >= 3  # the boundary moves from row to row


def test_policy_switch(monkeypatch):
    world, camera, _ = case("soft_shadows", (256, 256))
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "0")
    assert world.scene_tile_mask(camera) is None
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "2")
    two = world.scene_tile_mask(camera)
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "1")  # the policy: this frame has more unseen tiles than the threshold asks for
    one = world.scene_tile_mask(camera)
    assert one is not None and (one == two).all()
    # the scene rectangle is not the mask's business: the same with and without
    for v in ("0", "2"):
        monkeypatch.setenv("RTC_AMD_SCENE_TILES", v)
        plan = world.scene_plan(camera)[1]
        assert plan["scene_rect"] == "0 16 0 16", plan["scene_rect"]
    # a frame that is nearly all floor stays on the grid under the policy, and gets its list when asked for one
    world, camera, _ = case("rolled", (320, 256))
    down = P.Camera(320, 256, camera.field_of_view, P.view_transform(P.point(0, 6, -6), P.point(0, 4.0, 0), P.vector(0, 1, 0)))
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "2")
    m = world.scene_tile_mask(down)
    assert m is not None and 0 < (~m).sum() < 0.1 * m.size, (~m).sum()
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "1")
    assert world.scene_tile_mask(down) is None
    # a world without planes keeps its rule -- entries on under a third of the frame and under two thirds of their rectangle: a
    # ball on 45 % of the frame's tiles gets a list only when asked for one, two balls far away and apart get theirs by the policy
    ball = P.World([_ball()], world.light)
    two, far, _ = two_far_balls()
    near = P.Camera(320, 256, camera.field_of_view, P.view_transform(P.point(0, 1.5, -3.6), P.point(0.3, 1.6, 0), P.vector(0, 1, 0)))
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "1")
    assert world.scene_tile_mask(near) is not None  # (with the floor: by its unseen share)
    assert ball.scene_tile_mask(near) is None and two.scene_tile_mask(far) is not None
    monkeypatch.setenv("RTC_AMD_SCENE_TILES", "2")
    m = ball.scene_tile_mask(near)
    assert m is not None and 0.33 < m.mean() < 0.8, m.mean()


# ------------------------------------------------------------------------------------------------------------- list arithmetic
def _tile_list(mask, width, height, part):
    th, tw = mask.shape
    cap = tw * th + 64
    tiles, fill, counts = np.zeros(cap, np.uint32), np.zeros(2 * cap, np.uint32), np.zeros(2, np.uint32)
    flat = np.ascontiguousarray(mask.astype(np.uint8).ravel())
    traced = L.lib().rtc_diag_scene_tiles(flat.ctypes.data_as(C.POINTER(C.c_uint8)), tw, th, width, height, C.byref(part), _p(tiles), _p(fill), cap, _p(counts))
    return tiles[:counts[0]].copy(), fill[:2 * counts[1]].reshape(-1, 2).copy(), int(traced)


def _xy(words):
    words = np.asarray(words, dtype=np.uint64)
    return ((words >> 16) & 0x3fff) << 2, (words & 0x7fff) << 2


def _order(tiles, width, rows, ticks=None):
    out = np.zeros(len(tiles) + 8, np.uint32)
    n = L.lib().rtc_diag_tile_order(_p(_u32(tiles)), _p(_u32(ticks)) if ticks is not None else None, len(tiles), width, rows, _p(out), len(out))
    return out[:n].copy()


PARTITIONS = [(16, 3), (64, 2)]


@pytest.mark.parametrize("name,size", [("soft_shadows", (256, 256)), ("rolled", (320, 256)), ("floor_and_wall", (160, 112)), ("plane_only", (96, 64))])
def test_list_orders_and_cover(name, size):
    world, camera, _ = case(name, size)
    mask = world.scene_tile_mask(camera)
    w, h = size
    rng = np.random.default_rng(5)
    for band, n_parts in PARTITIONS + [(16, 1)]:
        for part in range(n_parts):
            q = L.rtc_partition(band, n_parts, part)
            rows = int(L.lib().rtc_partition_rows(h, C.byref(q)))
            tiles, fill, traced = _tile_list(mask, w, h, q)
            # tiles + fill runs cover every pixel of the partition exactly once
            cover = np.zeros((rows, w), np.int32)
            for x0, y0 in zip(*_xy(tiles)):
                cover[int(y0):int(y0) + 16, int(x0):int(x0) + 16] += 1
            for x0_n, row in fill:
                x0, n = int(x0_n) & 0xffff, int(x0_n) >> 16
                assert 1 <= n <= 64
                cover[int(row):int(row) + 16, 16 * x0:16 * (x0 + n)] += 1
            assert (cover == 1).all(), (name, band, n_parts, part)
            if len(tiles) == 0:
                continue
            # the first frame's order: a permutation of the image-order list, tiles of four tile rows still together
            first = _order(tiles, w, rows)
            assert sorted(first.tolist()) == sorted(tiles.tolist())
            fy = _xy(first)[1] // 64
            assert (np.diff(fy.astype(np.int64)) >= 0).all()
            if len(tiles) > 8 and rows >= 32:
                assert first.tolist() != tiles.tolist()
            # the feedback's order: a permutation sorted by the key -- the longest of a tile's four waves -- equal ones in list order
            ticks = rng.integers(0, 50, size=(len(first), 4)).astype(np.uint32)
            again = _order(first, w, rows, ticks)
            assert sorted(again.tolist()) == sorted(first.tolist())
            key = dict(zip(first.tolist(), ticks.max(axis=1).tolist()))
            pos = {t: i for i, t in enumerate(first.tolist())}
            keys = [key[t] for t in again.tolist()]
            assert keys == sorted(keys, reverse=True)
            for a, b in zip(again.tolist(), again.tolist()[1:]):
                if key[a] == key[b]:
                    assert pos[a] < pos[b]


def test_wave_work_and_the_rule():
    lib = L.lib()
    # rays that met objects (rays less those the cull resolved) + 16 x shade points (+ an eighth of the culled ones): the grid feedback's key
    assert lib.rtc_diag_wave_work(100, 3, 0) == 100 + 48
    assert lib.rtc_diag_wave_work(100, 3, 40) == 60 + 48 + 5
    assert lib.rtc_diag_wave_work(10, 0, 40) == 5
    # even waves: no list; a few long waves at the end of the list: longest first pays
    even = np.full(4 * 4096, 7, np.uint32)
    assert lib.rtc_diag_longest_first_pays(_p(even), 4096, 256) == 0
    tail = even.copy()
    tail[-4 * 64:] = 400
    assert lib.rtc_diag_longest_first_pays(_p(tail), 4096, 256) == 1
