#!/usr/bin/env python3
"""Ray-stream first hits and occlusion (Renderer.trace_hits, Renderer.is_shadowed) against what the same user had before
them, one process, the routes alternating -- every other round in the reverse order, two untimed launches after every change
of kernel (tools/time_supersample.py says why).

    python tools/time_trace_hits.py --parent-lib PATH/librtc_amd.so [--out profiles/trace_hits_times.txt] [--rounds 5] [--frames 10]
                                    [--quick] [--cases C3,mesh] [--no-host]

Per scene, for the camera's own rays:
  (a) rtc_ctx_render_hits of the frame by the parent commit's library (--parent-lib: built from a checkout of the parent), with
      the planes (object, distance, normal) and with (light);
  (b) World.hit_at by the parent's library for the same rays from host arrays, wall time: the only route from caller rays to
      first hits before;
  (c) trace_hits of the camera's rays in image order and in the render's order (8 x 8 tiles, 2 x 2 of them to a workgroup's
      16 x 16 block, blocks row by row), with the same two sets of planes; and a device-to-device torch copy of 32 B per ray,
      what a stream reads that a frame does not;
  (d) is_shadowed for every first hit's over_point against the scene's light position (a rectangle light's corner), beside the
      parent's World.is_shadowed for the same pairs, wall time;
  (e) rtc_ctx_render and rtc_ctx_trace (image order) by the parent's library and by this tree's: both paths are untouched and
      must reproduce the parent within its spread, with the same code objects (the ids are compared).
ms: HIP events around each call, mean over a round's launches; median (min .. max) over the rounds."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
ap.add_argument("--cases", default=None, help="comma-separated labels (default: all)")
ap.add_argument("--no-host", action="store_true", help="leave out the host routes (b) and (d)'s World.is_shadowed")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ray_tracer_challenge_amd import _lib as L  # noqa: E402
from ray_tracer_challenge_amd import scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402

CASES = [("C3", "soft_shadows", 4096, 4096), ("reflect_refract", "reflect_refract", 1000, 500), ("mesh", "mesh", 1024, 768),
         ("C5", "sphere_grid", 8192, 8192)]
GEOMETRY, LIGHT = ("object", "distance", "normal"), ("light",)
NEW = ("rtc_ctx_trace_hits", "rtc_ctx_is_shadowed")
DEV = "cuda:0"
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))


class parent_library:
    """with parent_library(): ... -- the package's calls go to the parent's library, which lacks this tree's new symbols"""

    def __enter__(self):
        self.own = {k: L.SIGNATURES.pop(k) for k in NEW if k in L.SIGNATURES}
        self.use = L.use_library(args.parent_lib)
        return self.use.__enter__()

    def __exit__(self, *exc):
        try:
            return self.use.__exit__(*exc)
        finally:
            L.SIGNATURES.update(self.own)


def timed(call, frames):
    """two untimed launches, then `frames` of them, an event pair around each -> mean ms"""
    for _ in range(2):
        call()
    pairs = []
    for _ in range(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / frames


def tile_order(w, h):
    """The pixels in the render's order: blocks of 16 x 16 row by row, a block's four 8 x 8 tiles 2 x 2, a tile's pixels row by row."""
    y, x = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
    block = (y >> 4) * ((w + 15) >> 4) + (x >> 4)
    wave = ((y >> 3) & 1) * 2 + ((x >> 3) & 1)
    lane = (y & 7) * 8 + (x & 7)
    return torch.argsort(((block * 4 + wave) * 64 + lane).reshape(-1), stable=True)


def take(t, perm, piece=1 << 24):
    """t[perm], gathered in pieces (one indexing kernel over the 67 M rays of an 8192^2 frame is more than a launch takes)"""
    return torch.cat([t[perm[i:i + piece]] for i in range(0, perm.numel(), piece)]).contiguous()


def planes_out(n, planes):
    return {k: torch.empty((n, L.HIT_PLANES[k][1]) if L.HIT_PLANES[k][1] > 1 else (n,), dtype=torch.int32 if L.HIT_PLANES[k][0] else torch.float32,
                           device=DEV) for k in planes}


def wall_ms(fn, times):
    out = []
    for _ in range(times):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def time_case(label, name, w, h):
    if args.quick:
        w, h = w // 4, h // 4
    kw = {"jitter": ("hashed", scenes.DEFAULT_SEED)} if name == "soft_shadows" else {}
    world, camera, depth = getattr(scenes, name)(w, h, **kw)
    n = w * h
    branch = Renderer(world, camera, device=0)
    with parent_library():
        parent = Renderer(world, camera, device=0)
    frame = branch.alloc()
    colors = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    image = branch.camera_rays()
    torch.cuda.synchronize()
    perm = tile_order(w, h)
    tiled = tuple(take(t, perm) for t in image)
    del perm
    outs = {GEOMETRY: planes_out(n, GEOMETRY), LIGHT: planes_out(n, LIGHT)}
    frames_out = {p: {k: v.reshape((h, w) + tuple(v.shape[1:])) for k, v in o.items()} for p, o in outs.items()}
    # (d): the first hits' over_points against the light's position
    first = branch.trace_hits(image[0], image[1], keys=image[2], planes=("object", "over_point"))
    points = first["over_point"][first["object"] >= 0].contiguous()
    del first
    light = world.light
    lpos = np.asarray(light.corner if hasattr(light, "corner") else light.position, dtype=np.float32)
    lights = torch.from_numpy(lpos).to(DEV)[None, :].expand(points.shape[0], 4).contiguous()
    shadowed = torch.empty((points.shape[0],), dtype=torch.int32, device=DEV)

    routes = []
    for planes, tag in ((GEOMETRY, "geometry"), (LIGHT, "light")):
        routes.append(("render_hits, parent, " + tag, lambda planes=planes: timed(lambda: parent.render_hits(planes=planes, out=frames_out[planes]), args.frames)))
        routes.append(("render_hits, branch, " + tag, lambda planes=planes: timed(lambda: branch.render_hits(planes=planes, out=frames_out[planes]), args.frames)))
        for what, rays in (("image order", image), ("tile order", tiled)):
            routes.append(("trace_hits, %s, %s" % (what, tag),
                           lambda planes=planes, rays=rays: timed(lambda: branch.trace_hits(rays[0], rays[1], keys=rays[2], planes=planes, out=outs[planes]), args.frames)))
    src, dst = torch.empty(n * 8, dtype=torch.float32, device=DEV), torch.empty(n * 8, dtype=torch.float32, device=DEV)  # 32 B per ray
    routes.append(("copy 32 B per ray", lambda: timed(lambda: dst.copy_(src), args.frames)))
    routes.append(("is_shadowed", lambda: timed(lambda: branch.is_shadowed(lights, points, out=shadowed), args.frames)))
    for who, r in (("parent", parent), ("branch", branch)):
        routes.append(("render, " + who, lambda r=r: timed(lambda: r.render(depth, out=frame), args.frames)))
        routes.append(("trace, " + who, lambda r=r: timed(lambda: r.trace(image[0], image[1], depth, keys=image[2], out=colors), args.frames)))
    t = {r[0]: [] for r in routes}
    for _, fn in routes:  # warm-up: compiles, schedules
        fn()
    for rnd in range(args.rounds):
        for what, fn in (routes if rnd % 2 == 0 else routes[::-1]):
            t[what].append(fn())
    ids = {who: (r.kernel_id, r.trace_kernel_id) for who, r in (("parent", parent), ("branch", branch))}
    # what the stream gives is what the frame gives (tests/test_gpu_trace_hits.py is the contract; this is a report)
    same = True
    for planes in (GEOMETRY, LIGHT):
        a = {k: v.clone() for k, v in branch.render_hits(planes=planes).items()}
        b = branch.trace_hits(image[0], image[1], keys=image[2], planes=planes)
        torch.cuda.synchronize()
        same = same and all(torch.equal(a[k][:-1, :-1], b[k].reshape(a[k].shape)[:-1, :-1]) for k in planes)
        del a, b

    say("%s: %s %d x %d, %d rays, %d first hits; median (min .. max) of %d rounds x %d launches, ms" % (label, name, w, h, n, points.shape[0], args.rounds, args.frames))
    for what, _ in routes:
        say("  %-36s %s" % (what, spread(t[what])))
    host = {}
    if not args.no_host:
        ho, hd = image[0].cpu().numpy(), image[1].cpu().numpy()
        hl, hp = lights.cpu().numpy(), points.cpu().numpy()
        times = 3 if n <= (1 << 22) else 1
        with parent_library():
            host["geometry"] = wall_ms(lambda: world.hit_at(ho, hd, planes=GEOMETRY), times)
            host["light"] = wall_ms(lambda: world.hit_at(ho, hd, planes=LIGHT), times)
            host["shadowed"] = wall_ms(lambda: world.is_shadowed(hl, hp), times)
        del ho, hd, hl, hp
        say("  %-36s %s   (wall time, host arrays in and out, %d call%s)" % ("World.hit_at, parent, geometry", spread(host["geometry"]), times, "s" if times > 1 else ""))
        say("  %-36s %s   (likewise)" % ("World.hit_at, parent, light", spread(host["light"])))
        say("  %-36s %s   (likewise)" % ("World.is_shadowed, parent", spread(host["shadowed"])))
        for tag in ("geometry", "light"):
            say("  (b) / (c, image order), %s: %.1f" % (tag, med(host[tag]) / med(t["trace_hits, image order, " + tag])))
        say("  World.is_shadowed / is_shadowed: %.1f" % (med(host["shadowed"]) / med(t["is_shadowed"])))
    c = med(t["copy 32 B per ray"])
    for tag in ("geometry", "light"):
        a, tr = med(t["render_hits, parent, " + tag]), med(t["trace_hits, tile order, " + tag])
        say("  (c, tile order) / ((a) + copy), %s: %.3f / (%.3f + %.3f) = %.3f      (c, image order) / (c, tile order) = %.3f"
            % (tag, tr, a, c, tr / (a + c), med(t["trace_hits, image order, " + tag]) / tr))
    for what in ("render_hits, %s, geometry", "render_hits, %s, light", "render, %s", "trace, %s"):
        p, b = t[what % "parent"], t[what % "branch"]
        say("  %s - parent: %+.3f ms; the branch's median is %s the parent's min .. max (%.3f .. %.3f)"
            % (what % "branch", med(b) - med(p), "inside" if min(p) <= med(b) <= max(p) else "OUTSIDE", min(p), max(p)))
    say("  render kernel id: parent %s, branch %s: %s" % (ids["parent"][0], ids["branch"][0], "the same" if ids["parent"][0] == ids["branch"][0] else "DIFFERENT"))
    say("  trace kernel id:  parent %s, branch %s: %s" % (ids["parent"][1], ids["branch"][1], "the same" if ids["parent"][1] == ids["branch"][1] else "DIFFERENT"))
    say("  trace_hits in image order == render_hits on the traced pixels, bit for bit: %s" % same)
    branch.close()
    parent.close()
    torch.cuda.empty_cache()


if not args.parent_lib:
    sys.exit("--parent-lib is needed: rows (a), (b), (d) and (e) are the parent's")
say("device: %s" % torch.cuda.get_device_name(0))
wanted = args.cases.split(",") if args.cases else [c[0] for c in CASES]
for case in CASES:
    if case[0] in wanted:
        time_case(*case)
        say()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.cases else "w") as f:
        f.write("\n".join(lines) + "\n")
