"""Rectangle lights over the whole range of grid shapes (-m gpu).  tests/light_grids.py has the shapes, the worlds and the
oracle's side; every comparison is bit-exact against the oracle (tests.helpers.assert_images_equal), ray counts and shade points
included, and every cell asserts from the kernel's name which kernel family ran.

(a) every shape x {spheres, spheres 1 000 units from the origin, medley, group} x the ahead-of-time kernel, the scene-compiled kernel
    with one lane per pixel, and the scene-compiled kernel as the library launches it -- with what the code prescribes for the
    culled-ray count on either side of the 8-cell threshold and of the block cones' evenness rule;
(b) spheres x every shape x each shortcut switched off in turn;
(c) a short list of shapes x spheres and group x the other ways to reach the light: lanes sharing a pixel, supersampled and
    adaptive frames, first-hit light planes, shuffled ray streams, batched intensity_at with hashed and with cycled jitter;
(d) the culled-ray counter against an independent count, up to the packed counter's capacity and on both sides of it."""
import numpy as np
import pytest
import torch

from ray_tracer_challenge_amd import _lib as L
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests import hits_helpers as HH
from tests import light_grids as G
from tests.adaptive_helpers import compose, edge_mask

pytestmark = pytest.mark.gpu
f32 = np.float32
SWITCHES = ("SPECIALIZE", "SHARE_LOG2", "LIGHT_CULL", "CELL_CULL", "OWN_BLOCKS", "FAST_SHADOW", "DARK", "GATES", "BLOCK_FEEDBACK", "BLOCK_LIST", "WAVEFRONT")
# the three ways a frame is rendered in (a): the ahead-of-time kernel; the scene's own kernel with one lane per pixel (the block
# cones are compiled into such a kernel only); the scene's own kernel as the library launches a frame this small (8 lanes per pixel
# from CULL_THRESHOLD cells on)
KERNEL_CONFIGS = {"aot": dict(SPECIALIZE=0), "spec": dict(SPECIALIZE=1, SHARE_LOG2=0), "spec_shared": dict(SPECIALIZE=1)}
ids = G.shape_id


@pytest.fixture
def env(monkeypatch):
    """Sets the library's switches (read when a context is created): all of SWITCHES unset, then the world's own (G.SWITCHES_OF) and
    the given ones."""
    def set_(name=None, **kw):
        for k in SWITCHES:
            monkeypatch.delenv("RTC_AMD_" + k, raising=False)
        for k, v in dict(G.SWITCHES_OF.get(name, {}), **kw).items():
            assert k in SWITCHES, k
            monkeypatch.setenv("RTC_AMD_" + k, str(v))
    set_()
    return set_


def _render(name, shape, depth=G.DEPTH, size=G.FRAME, supersample=1):
    """-> (frame, stats, kernel name, lanes per pixel (log2) of the launch)"""
    r = Renderer(G.world(name, shape), G.camera(name, size), device=0, supersample=supersample)
    out = r.render(depth)
    torch.cuda.synchronize()
    st, kernel, share = r.stats(), r.kernel_name, int(L.lib().rtc_diag_ctx_share_log2(r._ctx))
    assert r.jit_status == "", r.jit_status
    r.close()
    return out.cpu().numpy(), st, kernel, share


def _check_frame(name, shape, got, st, what, size=G.FRAME, depth=G.DEPTH):
    """image, rays and shade points are the oracle's; the counters are consistent"""
    exp, rays = G.oracle_frame(name, shape, size, depth)
    H.assert_images_equal(got, exp, what)
    assert st["rays"] == rays, (what, st["rays"], rays)
    assert st["shaded_hits"] == G.oracle_shaded_hits(name, shape, size, depth), (what, st)
    assert st["pixels"] == G.traced_pixels(size), (what, st)
    G.check_counts(st, shape, what)


def _blocks_apply(name, shape):
    """rtc_kernel_core.h blocks_usable: both step counts even, every caster a uniformly scaled sphere, an unrolled flat kernel with
    one lane per pixel -- and NO minimum number of cells."""
    return name.startswith("spheres") and shape[0] % 2 == 0 and shape[1] % 2 == 0


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("config", list(KERNEL_CONFIGS))
@pytest.mark.parametrize("shape", G.SHAPES, ids=ids)
@pytest.mark.parametrize("name", ["spheres", "spheres_far", "medley", "group"])
def test_every_shape_renders_like_the_oracle(name, shape, config, env):
    G.assert_penumbra(name, shape)
    env(name, **KERNEL_CONFIGS[config])
    got, st, kernel, share = _render(name, shape)
    what = "%s %s %s" % (name, ids(shape), config)
    print(what, kernel, "share", share, st)
    G.assert_kernel(name, kernel, config != "aot")
    # lanes per pixel: only the library's own choice shares, and only from the threshold on (choose_share_log2)
    assert share == (3 if config == "spec_shared" and G.cells(shape) >= G.CULL_THRESHOLD else 0), (what, share)
    _check_frame(name, shape, got, st, what)
    culled = st["culled_shadow_rays"]
    if G.cells(shape) < G.CULL_THRESHOLD and not _blocks_apply(name, shape):
        # (1, 1), (1, 7), (7, 1) everywhere, (2, 2) where the casters are not all spheres: under 8 cells the whole-light cull stands down
        # (light_cull_mask) and nothing else answers a sample without a test
        assert culled == 0, (what, st)
    elif name.startswith("spheres") and G.cells(shape) >= G.CULL_THRESHOLD:
        assert culled > 0, (what, st)  # the open floor of the right-hand wave tiles sees the light clear of both spheres
    elif name.startswith("spheres"):
        # (2, 2): 4 cells, so the whole-light cull is off and the mask of culled objects is 0 -- but block cones need even step counts,
        # not 8 cells: the light's one 2 x 2 block is called lit, four rays at a time, by every wave ALL of whose lanes see its cone
        # clear of the spheres.  The cone of a block that is the whole 2 x 2-unit light is 14 - 17 degrees wide from this floor, and no
        # wave tile of this frame lies that far from the spheres: what the count is HERE follows from the geometry, and
        # test_on_open_floor_every_rule_answers_all_or_nothing pins the rule where every lane agrees.
        assert shape == (2, 2) and culled % 4 == 0, (what, st)


OPEN_FLOOR = {  # shape -> (what answers the open floor's samples: the whole-light cull, the block cones), from the code:
    (1, 1): (False, False), (1, 7): (False, False), (7, 1): (False, False),  # under 8 cells no cull (light_cull_mask); an odd count: no blocks (blocks_usable)
    (2, 2): (False, True),                                                   # under 8 cells no cull -- but blocks need even counts, not 8 cells
    (1, 8): (True, False), (8, 1): (True, False), (3, 3): (True, False), (5, 2): (True, False),  # from 8 cells the cull; an odd count: no blocks
    (2, 4): (True, True), (4, 2): (True, True), (16, 16): (True, True)}      # both


@pytest.mark.parametrize("config", list(KERNEL_CONFIGS))
@pytest.mark.parametrize("shape", list(OPEN_FLOOR), ids=ids)
def test_on_open_floor_every_rule_answers_all_or_nothing(shape, config, env):
    """One wave of open floor ten units beside the spheres: every lane sees the whole light clear of both by a wide margin, so
    whichever rule applies to a shape answers ALL of the wave's samples without a test -- and where none applies, none is.  The
    8-cell threshold of the whole-light cull, the evenness rule of the block cones and the fact that they need no 8 cells, each
    with its own switch: a change of any of them turns a row of this table red."""
    name, size = "spheres_open", G.SMALL_FRAME
    cull, blocks = OPEN_FLOOR[shape]
    assert cull == (G.cells(shape) >= G.CULL_THRESHOLD) and blocks == _blocks_apply(name, shape)
    light, obj = G.oracle_light_plane(name, shape, size)
    assert (obj[:-1, :-1] == 0).all() and (light[:-1, :-1] == 1.0).all()  # every traced pixel: floor, fully lit
    every = G.traced_pixels(size) * G.cells(shape)
    for off in ((), ("LIGHT_CULL",), ("CELL_CULL",), ("LIGHT_CULL", "CELL_CULL")):
        env(name, **dict(KERNEL_CONFIGS[config], **{k: 0 for k in off}))
        got, st, kernel, share = _render(name, shape, size=size)
        what = "open floor %s %s without %s" % (ids(shape), config, "+".join(off) or "nothing")
        print(what, kernel, "share", share, st)
        G.assert_kernel(name, kernel, config != "aot")
        assert share == (3 if config == "spec_shared" and cull else 0), (what, share)
        _check_frame(name, shape, got, st, what, size)
        # (lanes sharing a pixel walk the cells themselves: the block cones are a path of kernels with one lane per pixel)
        answered = (cull and "LIGHT_CULL" not in off) or (blocks and "CELL_CULL" not in off and share == 0)
        assert st["culled_shadow_rays"] == (every if answered else 0), (what, st, every)


# ---------------------------------------------------------------- (b)
SWITCHED_OFF = [("LIGHT_CULL",), ("CELL_CULL",), ("OWN_BLOCKS",), ("FAST_SHADOW",), ("DARK",), ("LIGHT_CULL", "CELL_CULL")]


@pytest.mark.parametrize("config", ["aot", "spec"])
@pytest.mark.parametrize("shape", G.SHAPES, ids=ids)
def test_each_shortcut_switched_off_changes_nothing_but_the_count(shape, config, env):
    name = "spheres"
    env(name, **KERNEL_CONFIGS[config])
    got, on, kernel, _ = _render(name, shape)
    G.assert_kernel(name, kernel, config != "aot")
    _check_frame(name, shape, got, on, "%s %s all on" % (ids(shape), config))
    for off in SWITCHED_OFF:
        env(name, **dict(KERNEL_CONFIGS[config], **{k: 0 for k in off}))
        got, st, kernel, share = _render(name, shape)
        what = "%s %s without %s" % (ids(shape), config, "+".join(off))
        print(what, kernel, st)
        G.assert_kernel(name, kernel, config != "aot")
        assert share == 0
        _check_frame(name, shape, got, st, what)
        culled = st["culled_shadow_rays"]
        assert culled <= on["culled_shadow_rays"], (what, st, on)
        if "LIGHT_CULL" in off and ("CELL_CULL" in off or not _blocks_apply(name, shape)):
            assert culled == 0, (what, st)  # with the cull off nothing is answered without a test -- but for the block cones, a switch of their own
        elif "LIGHT_CULL" in off:
            assert culled % 4 == 0, (what, st)  # block cones alone: four rays at a time
        if off == ("CELL_CULL",) and G.cells(shape) < G.CULL_THRESHOLD:
            assert culled == 0, (what, st)  # (2, 2) and the odd shapes under the threshold


# ---------------------------------------------------------------- (c)
C_CASES = [(name, shape) for name in ("spheres", "group") for shape in G.SHORT]
c_ids = ["%s-%s" % (n, ids(s)) for n, s in C_CASES]


@pytest.mark.parametrize("name,shape", C_CASES, ids=c_ids)
def test_lanes_sharing_a_pixel(name, shape, env):
    """2, 4 and 8 lanes of a scene-compiled kernel walk the cells of one shade point with stride 2, 4, 8 (a 1 x n light wraps a row at
    every step): the image, the rays and the shade points of the single-lane render, which are the oracle's."""
    env(name, SPECIALIZE=1, SHARE_LOG2=0)
    got, single, kernel, share = _render(name, shape)
    assert share == 0
    _check_frame(name, shape, got, single, "%s %s one lane" % (name, ids(shape)))
    for s in (1, 2, 3):
        env(name, SPECIALIZE=1, SHARE_LOG2=s)
        got, st, kernel, share = _render(name, shape)
        what = "%s %s %d lanes per pixel" % (name, ids(shape), 1 << s)
        print(what, kernel, st)
        G.assert_kernel(name, kernel, True)
        assert share == s, (what, share)
        _check_frame(name, shape, got, st, what)
        assert (st["rays"], st["shaded_hits"]) == (single["rays"], single["shaded_hits"]), (what, st, single)


@pytest.mark.parametrize("specialise", [0, 1])
@pytest.mark.parametrize("name,shape", C_CASES, ids=c_ids)
def test_supersampled_frames(name, shape, specialise, env):
    """k x k rays per pixel reduced in the kernel, against the box filter of the oracle's fine frame (tests/test_gpu_supersample.py);
    the scene's own kernel shares lanes here too, up to 16 per pixel."""
    for k in (2, 4):
        exp, rays = G.oracle_filtered(name, shape, k)
        env(name, SPECIALIZE=specialise)
        got, st, kernel, share = _render(name, shape, supersample=k)
        what = "%s %s supersample %d specialise %d" % (name, ids(shape), k, specialise)
        print(what, kernel, "share", share, st)
        G.assert_kernel(name, kernel, bool(specialise), "ss_render_kernel")
        assert ";ss=%d" % k in kernel, kernel
        H.assert_images_equal(got, exp, what)
        assert st["rays"] == rays, (what, st, rays)
        assert st["pixels"] == (k * G.FRAME[0] - 1) * (k * G.FRAME[1] - 1)
        assert (st["rays"] - st["pixels"]) == st["shaded_hits"] * G.cells(shape), (what, st)  # (no world of the sweep recurses)
        G.check_counts(st, shape, what)


@pytest.mark.parametrize("name,shape", C_CASES, ids=c_ids)
def test_adaptive_frames(name, shape, env):
    """render_adaptive(k = 2): the plain frame with the 2 x 2 value wherever a neighbour differs by more than the threshold."""
    k, threshold = 2, 0.1
    B, base_rays = G.oracle_frame(name, shape)
    M = edge_mask(B, threshold)
    assert 0.05 <= M.mean() <= 0.95, M.mean()
    exp = compose(B, G.oracle_filtered(name, shape, k)[0], M)
    env(name, SPECIALIZE=0)
    r = Renderer(G.world(name, shape), G.camera(name), device=0)
    out, mask = r.render_adaptive(G.DEPTH, k=k, threshold=threshold, mask=True)
    torch.cuda.synchronize()
    what = "%s %s adaptive" % (name, ids(shape))
    assert np.array_equal(mask.cpu().numpy(), M.astype(np.uint8)), what
    H.assert_images_equal(out.cpu().numpy(), exp, what)
    ad, st = r.adaptive_stats(), r.stats()
    print(what, r.adaptive_kernel_name, ad, st)
    G.assert_kernel(name, r.kernel_name, False)
    G.assert_kernel(name, r.adaptive_kernel_name, False, "adaptive_refine_kernel")
    assert ";ss=%d" % k in r.adaptive_kernel_name
    assert ad["refined_pixels"] == int(M.sum()) and st["rays"] == base_rays
    assert 0 < ad["shaded_hits"] and ad["culled_shadow_rays"] <= ad["shaded_hits"] * G.cells(shape) <= ad["rays"], (what, ad)
    G.check_counts(st, shape, what)
    r.close()


def _traced_rays(r, size):
    """the camera's rays of the traced pixels (the last row and column are never traced), with their keys"""
    o, d, keys = r.camera_rays()
    w, h = size
    traced = torch.tensor([y * w + x for y in range(h - 1) for x in range(w - 1)], dtype=torch.int64, device=o.device)
    return o[traced].contiguous(), d[traced].contiguous(), keys[traced].contiguous(), traced.cpu().numpy()


@pytest.mark.parametrize("name,shape", C_CASES, ids=c_ids)
def test_first_hit_light_planes(name, shape, env):
    """render_hits' light plane, and trace_hits' for the same rays in a shuffled order with their keys, against the oracle's
    intensity_at of every pixel's first hit."""
    exp_light, exp_obj = G.oracle_light_plane(name, shape)
    assert ((exp_light > 0) & (exp_light < 1)).sum() >= (0 if shape == (1, 1) else 8)
    env(name, SPECIALIZE=0)
    r = Renderer(G.world(name, shape), G.camera(name), device=0)
    G.assert_kernel(name, r.kernel_name, False)  # (the first-hit kernels are the ahead-of-time family's)
    got = r.render_hits(planes=("object", "light"))
    torch.cuda.synchronize()
    what = "%s %s" % (name, ids(shape))
    assert np.array_equal(got["object"].cpu().numpy(), exp_obj), what
    assert HH.same(got["light"].cpu().numpy(), exp_light).all(), (what, int((~HH.same(got["light"].cpu().numpy(), exp_light)).sum()))
    o, d, keys, traced = _traced_rays(r, G.FRAME)
    perm = torch.randperm(len(traced), generator=torch.Generator().manual_seed(11)).to(o.device)
    res = r.trace_hits(o[perm].contiguous(), d[perm].contiguous(), keys=keys[perm].contiguous(), planes=("object", "light"))
    torch.cuda.synchronize()
    back = np.empty(len(traced), dtype=np.int64)
    back[perm.cpu().numpy()] = np.arange(len(traced))
    assert np.array_equal(res["object"].cpu().numpy()[back], exp_obj.reshape(-1)[traced]), what
    assert HH.same(res["light"].cpu().numpy()[back], exp_light.reshape(-1)[traced]).all(), what
    r.close()


@pytest.mark.parametrize("name,shape", C_CASES, ids=c_ids)
def test_shuffled_ray_streams(name, shape, env):
    """trace() of the camera's rays shuffled by a fixed permutation, each ray with its pixel's key: the oracle's frame, ray counts
    and shade points -- whichever 64 rays share a wave and vote on a light block together."""
    exp, rays = G.oracle_frame(name, shape)
    env(name, SPECIALIZE=0)
    r = Renderer(G.world(name, shape), G.camera(name), device=0)
    o, d, keys, traced = _traced_rays(r, G.FRAME)
    perm = torch.randperm(len(traced), generator=torch.Generator().manual_seed(5)).to(o.device)
    out = r.trace(o[perm].contiguous(), d[perm].contiguous(), G.DEPTH, keys=keys[perm].contiguous())
    torch.cuda.synchronize()
    st, what = r.stats(), "%s %s shuffled trace" % (name, ids(shape))
    print(what, r.trace_kernel_name, st)
    G.assert_kernel(name, r.trace_kernel_name, False, "trace_kernel")
    got = np.zeros((G.FRAME[1] * G.FRAME[0], 3), dtype=f32)
    got[traced[perm.cpu().numpy()]] = out.cpu().numpy()
    H.assert_images_equal(got.reshape(G.FRAME[1], G.FRAME[0], 3), exp, what)
    assert st["rays"] == rays and st["shaded_hits"] == G.oracle_shaded_hits(name, shape), (what, st, rays)
    G.check_counts(st, shape, what)
    r.close()


CYCLE = [0.0, 1.0, 0.5, 0.25, 0.75, 0.125, 0.875, 0.375, 0.625, 0.0625, 0.9375, 0.3125, 0.6875, 0.4375, 0.5625, 0.1875]


@pytest.mark.parametrize("name,shape", C_CASES + [("spheres", (64, 1)), ("group", (64, 1))], ids=c_ids + ["spheres-64x1", "group-64x1"])
def test_batched_intensity_at(name, shape):
    """rtc_intensity_at for a batch of 64 probe points, point i drawing as pixel i: with the hashed jitter, and with a cycle of 16
    values -- whose draws are numbered in the reference's order, v outer and u inner, two per cell (1 x 64 against 64 x 1 tells a
    transposed walk apart).  The oracle's cycle is state of its light: a fresh world per point."""
    pts = G.probe_points(name)[::6]
    assert len(pts) == 64
    world = G.world(name, shape)
    own = H.oracle_world(world)
    exp = np.zeros(64, dtype=f32)
    for i in range(64):
        own.set_pixel(i)
        exp[i] = own.intensity_at(pts[i])
    assert ((exp > 0) & (exp < 1)).sum() >= 6, exp  # (a tenth of the points, as of the whole probe grid)
    got = world.intensity_at(pts)
    assert HH.same(got, exp).all(), (name, shape, "hashed", got, exp)
    cycled = G.world(name, shape, jitter=("cycle", CYCLE))
    exp = np.array([H.oracle_world(cycled).intensity_at(p) for p in pts], dtype=f32)
    assert ((exp > 0) & (exp < 1)).sum() >= 6, exp
    got = cycled.intensity_at(pts)
    assert HH.same(got, exp).all(), (name, shape, "cycle", got, exp)


# ---------------------------------------------------------------- (d)
CAPACITY = 2 ** 20 - 1  # culled shadow rays one lane of a kernel of up to 8 levels can count (rtc_launch_plan.h CULLED_COUNT_MAX)
# casterless, one shade point per pixel: 1023 x 1025 = 2^20 - 1 cells is the largest light that still counts, 1024 x 1024 the smallest
# that does not; 1024 x 1025 is no multiple of 2^20 (a counter that wrapped would show it, not a 0)
CASTERLESS_SHAPES = [(1, 8), (16, 16), (64, 64), (512, 256), (1023, 1025), (1024, 1024), (1024, 1025)]
# the mirrors at depth 7, eight shade points per pixel: 8 x 131 071 = 2^20 - 8 fits, 8 x 512 x 256 = 2^20 does not
MIRROR_SHAPES = [(16, 16), (1, 131071), (512, 256)]


def _check_counter(name, shape, st, points_per_lane, what):
    """culled_shadow_rays == shaded_hits x cells up to the capacity -- every sample of these worlds is answered without a test --
    and 0 beyond it, where the launch runs with the culls off"""
    n = G.cells(shape)
    assert st["shaded_hits"] > 0
    if n * points_per_lane <= CAPACITY:
        assert st["culled_shadow_rays"] == st["shaded_hits"] * n, (what, st, n)
    else:
        assert st["culled_shadow_rays"] == 0, (what, st, n)


def _counter_case(name, shape, depth, config, env):
    size, what = G.SMALL_FRAME, "%s %s %s" % (name, ids(shape), config)
    points_per_lane = depth + 1 if name == "mirrors" else 1
    if config == "trace":
        env(name, SPECIALIZE=0)
        r = Renderer(G.world(name, shape), G.camera(name, size), device=0)
        o, d, keys, traced = _traced_rays(r, size)
        out = r.trace(o, d, depth, keys=keys)
        torch.cuda.synchronize()
        st = r.stats()
        G.assert_kernel(name, r.trace_kernel_name, False, "trace_kernel")
        got = np.zeros((size[0] * size[1], 3), dtype=f32)
        got[traced] = out.cpu().numpy()
        got = got.reshape(size[1], size[0], 3)
        st["pixels"] = G.traced_pixels(size)
        r.close()
    else:
        env(name, **KERNEL_CONFIGS[config])
        got, st, kernel, share = _render(name, shape, depth, size)
        G.assert_kernel(name, kernel, config != "aot")
        assert share == (3 if config == "spec_shared" else 0)
    print(what, st)
    _check_frame(name, shape, got, st, what, size, depth)
    _check_counter(name, shape, st, points_per_lane, what)


@pytest.mark.parametrize("config", ["aot", "spec_shared", "trace"])
@pytest.mark.parametrize("shape", CASTERLESS_SHAPES, ids=ids)
def test_the_culled_count_of_a_casterless_world(shape, config, env):
    _counter_case("casterless", shape, G.DEPTH, config, env)


@pytest.mark.parametrize("config", ["aot", "spec_shared", "trace"])
@pytest.mark.parametrize("shape", MIRROR_SHAPES, ids=ids)
def test_the_culled_count_between_two_mirrors(shape, config, env):
    """depth 7: eight shade points per pixel, so that the capacity is reached by accumulation only"""
    assert G.oracle_shaded_hits("mirrors", shape, G.SMALL_FRAME, G.MIRROR_DEPTH) == 8 * G.traced_pixels(G.SMALL_FRAME)
    _counter_case("mirrors", shape, G.MIRROR_DEPTH, config, env)
