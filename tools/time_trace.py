#!/usr/bin/env python3
"""Ray streams (Renderer.trace) against what the same user had before them, one process, the routes alternating -- every
other round in the reverse order, two untimed launches after every change of kernel (tools/time_supersample.py says why).

    python tools/time_trace.py [--parent-lib PATH/librtc_amd.so] [--out profiles/trace_times.txt] [--rounds 8] [--frames 10] [--quick]

Per scene, for the camera's own rays at the scene's depth:
  (a) rtc_ctx_render's kernel ms of the frame -- by the parent commit's library (--parent-lib: built from a checkout of the
      parent) and by this tree's, alternating: the render path is untouched and must reproduce the parent within its spread;
  (b) World.color_at's wall time for the same rays from host arrays (depth <= 8): the only route to caller rays before;
  (c) a device-to-device torch copy of as many bytes as a trace moves: 16 + 16 + 4 B in, 12 B out per ray;
  (d) the trace's kernel ms (rtc_stats.kernel_ms) with the rays in image order, in the render's order -- 8 x 8 tiles, 2 x 2 of
      them to a workgroup's 16 x 16 block, blocks row by row -- and in a fixed random order.
kernel ms: the library's HIP-event time, mean over a round's launches; median (min .. max) over the rounds."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ray_tracer_challenge_amd import _lib as L  # noqa: E402
from ray_tracer_challenge_amd import scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402

CASES = [("C3", "soft_shadows", 4096, 4096), ("reflect_refract", "reflect_refract", 1000, 500), ("mesh", "mesh", 1024, 768),
         ("C5", "sphere_grid", 8192, 8192)]
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))


def med(v):
    return sorted(v)[len(v) // 2]


def render_ms(r, depth, out, frames):
    for _ in range(2):
        r.render(depth, out=out)
    r.stats()
    for _ in range(frames):
        r.render(depth, out=out)
    return r.stats()["kernel_ms"]


def trace_ms(r, depth, rays, out, frames):
    o, d, k = rays
    for _ in range(2):
        r.trace(o, d, depth, keys=k, out=out)
    r.stats()
    for _ in range(frames):
        r.trace(o, d, depth, keys=k, out=out)
    return r.stats()["kernel_ms"]


def copy_ms(n, frames):
    src, dst = torch.empty(n * 12, dtype=torch.float32, device="cuda:0"), torch.empty(n * 12, dtype=torch.float32, device="cuda:0")  # 48 B per ray
    for _ in range(2):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(frames):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / frames


def tile_order(w, h):
    """The pixels in the render's order: blocks of 16 x 16 row by row, a block's four 8 x 8 tiles 2 x 2, a tile's pixels row by row."""
    y, x = torch.meshgrid(torch.arange(h, device="cuda:0"), torch.arange(w, device="cuda:0"), indexing="ij")
    block = (y >> 4) * ((w + 15) >> 4) + (x >> 4)
    wave = ((y >> 3) & 1) * 2 + ((x >> 3) & 1)
    lane = (y & 7) * 8 + (x & 7)
    return torch.argsort(((block * 4 + wave) * 64 + lane).reshape(-1), stable=True)


def take(t, perm, piece=1 << 24):
    """t[perm], gathered in pieces (one indexing kernel over the 67 M rays of an 8192^2 frame is more than a launch takes)"""
    return torch.cat([t[perm[i:i + piece]] for i in range(0, perm.numel(), piece)]).contiguous()


def time_case(label, name, w, h):
    if args.quick:
        w, h = w // 4, h // 4
    kw = {"jitter": ("hashed", scenes.DEFAULT_SEED)} if name == "soft_shadows" else {}
    world, camera, depth = getattr(scenes, name)(w, h, **kw)
    n = w * h
    branch = Renderer(world, camera, device=0)
    parent = None
    if args.parent_lib:
        # (the parent's library has no ray-stream symbols to declare: this tree's has been loaded, with all of them, above)
        own = {k: L.SIGNATURES.pop(k) for k in list(L.SIGNATURES) if k.startswith(("rtc_ctx_trace", "rtc_ctx_camera_rays"))}
        try:
            with L.use_library(args.parent_lib):
                parent = Renderer(world, camera, device=0)
        finally:
            L.SIGNATURES.update(own)
    frame = branch.alloc()
    image = branch.camera_rays()
    torch.cuda.synchronize()
    orders = {"image order": image}
    for what, perm in (("tile order", tile_order(w, h)), ("random order", torch.randperm(n, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1)))):
        orders[what] = tuple(take(t, perm) for t in image)
        del perm
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    routes = [("render, branch", lambda: render_ms(branch, depth, frame, args.frames))]
    if parent is not None:
        routes.insert(0, ("render, parent", lambda: render_ms(parent, depth, frame, args.frames)))
    for what in orders:
        routes.append(("trace, " + what, lambda what=what: trace_ms(branch, depth, orders[what], out, args.frames)))
    routes.append(("copy 48 B per ray", lambda: copy_ms(n, args.frames)))
    t = {r[0]: [] for r in routes}
    for _, fn in routes:  # warm-up: compiles, schedules
        fn()
    for rnd in range(args.rounds):
        order = list(routes)
        if parent is not None and (rnd // 2) % 2 == 1:  # ... and the two renders change places every two rounds: neither is always the one
            order[0], order[1] = order[1], order[0]     # that follows the other, or the copy
        for what, fn in (order if rnd % 2 == 0 else order[::-1]):
            t[what].append(fn())
    # the trace in image order is the render, pixel for pixel (tests/test_gpu_trace.py is the contract; this is a report)
    branch.render(depth, out=frame)
    branch.trace(*image[:2], depth, keys=image[2], out=out)
    torch.cuda.synchronize()
    same = torch.equal(out.reshape(h, w, 3)[:-1, :-1], frame[:-1, :-1])
    say("%s: %s %d x %d, depth %d, %d rays; median (min .. max) of %d rounds x %d launches, ms" % (label, name, w, h, depth, n, args.rounds, args.frames))
    say("  render kernel  %s" % branch.kernel_name[:90])
    say("  trace kernel   %s  %s" % (branch.trace_kernel_name[:90], branch.trace_kernel_id))
    for what, _ in routes:
        say("  %-22s %s" % (what, spread(t[what])))
    if depth <= L.RTC_STACK_DEPTH_BASE:
        ho, hd = image[0].cpu().numpy(), image[1].cpu().numpy()
        walls = []
        for _ in range(3 if n <= (1 << 24) else 2):
            t0 = time.perf_counter()
            world.color_at(ho, hd, depth)
            walls.append(1e3 * (time.perf_counter() - t0))
        say("  %-22s %s   (wall time, host arrays in and out)" % ("World.color_at", spread(walls)))
        say("  World.color_at / trace, image order: %.1f" % (med(walls) / med(t["trace, image order"])))
        del ho, hd
    a = med(t["render, parent"]) if parent is not None else med(t["render, branch"])
    c = med(t["copy 48 B per ray"])
    say("  (d, tile order) / ((a) + (c)) = %.3f / (%.3f + %.3f) = %.3f" % (med(t["trace, tile order"]), a, c, med(t["trace, tile order"]) / (a + c)))
    say("  (d, image order) / (d, tile order) = %.3f      (d, random order) / (d, tile order) = %.3f"
        % (med(t["trace, image order"]) / med(t["trace, tile order"]), med(t["trace, random order"]) / med(t["trace, tile order"])))
    if parent is not None:
        p, b = t["render, parent"], t["render, branch"]
        say("  render, branch - parent: %+.3f ms; the branch's median is %s the parent's min .. max (%.3f .. %.3f)"
            % (med(b) - med(p), "inside" if min(p) <= med(b) <= max(p) else "OUTSIDE", min(p), max(p)))
    say("  trace in image order == render on the traced pixels, bit for bit: %s" % same)
    branch.close()
    if parent is not None:
        parent.close()
    del orders, image, out, frame
    torch.cuda.empty_cache()


say("device: %s" % torch.cuda.get_device_name(0))
for case in CASES:
    time_case(*case)
    say()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
