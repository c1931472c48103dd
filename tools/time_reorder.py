#!/usr/bin/env python3
"""Ray reordering (Renderer.trace(reorder=True)) against the plain trace, one process per scene, the routes alternating -- every
other round in the reverse order, two untimed launches after every change of kernel (tools/time_supersample.py says why).

    python tools/time_reorder.py --case C3 [--parent-lib PATH/librtc_amd.so] [--out profiles/reorder_times.txt] [--rounds 5] [--frames 10]
                                 [--quick] [--keys-out FILE] [--yardstick tools/sort_yardstick]

Per scene, at the scene's depth:
  (a) the plain trace of the camera's rays in tile, image and a fixed random order (tools/time_trace.py's three), by the parent
      commit's library (--parent-lib) and by this tree's: the plain path is untouched and must lie in the parent's range;
  (b) the reordered trace of the same three streams: the whole call, and rtc_ctx_reorder_stats' phases of the last launch;
  (c) the second bounce -- rays.reflected of the tile-ordered first hits -- plain and reordered;
  (d) the key layout, origin-major against direction-major (librtc_amd_dev.so, RTC_AMD_REORDER_DIR_MAJOR), on (b)-random and (c).
ms per call between two events on the stream (the whole call: for a plain trace the kernel and its counter sum), mean over a round's
launches; median (min .. max) over the rounds.  --keys-out: the random-order stream's coherence keys as raw u32, for
tools/sort_yardstick (rocPRIM's radix_sort_pairs on the same keys; --yardstick runs it and quotes its line)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"C3": ("soft_shadows", 4096, 4096), "reflect_refract": ("reflect_refract", 1000, 500), "mesh": ("mesh", 1024, 768),
         "C5": ("sphere_grid", 8192, 8192)}
ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=list(CASES))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None, help="appended to: one process per scene")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
ap.add_argument("--keys-out", default=None)
ap.add_argument("--yardstick", default=None)
args = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ray_tracer_challenge_amd import _lib as L  # noqa: E402
from ray_tracer_challenge_amd import rays, scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402

NEW = ("rtc_ctx_ray_order", "rtc_ctx_trace_reordered", "rtc_ctx_reorder_stats", "rtc_diag_ray_keys", "rtc_diag_reorder_plan")
PHASES = ("keys_ms", "sort_ms", "gather_ms", "trace_ms", "scatter_ms")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))


def call_ms(r, depth, stream, out, frames, reorder):
    o, d, k = stream
    for _ in range(2):
        r.trace(o, d, depth, keys=k, out=out, reorder=reorder)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(frames):
        r.trace(o, d, depth, keys=k, out=out, reorder=reorder)
    e1.record()
    torch.cuda.synchronize()
    r.stats()
    return e0.elapsed_time(e1) / frames


def tile_order(w, h):
    """The pixels in the render's order (tools/time_trace.py)."""
    y, x = torch.meshgrid(torch.arange(h, device="cuda:0"), torch.arange(w, device="cuda:0"), indexing="ij")
    block = (y >> 4) * ((w + 15) >> 4) + (x >> 4)
    wave = ((y >> 3) & 1) * 2 + ((x >> 3) & 1)
    lane = (y & 7) * 8 + (x & 7)
    return torch.argsort(((block * 4 + wave) * 64 + lane).reshape(-1), stable=True)


def take(t, perm, piece=1 << 24):
    return torch.cat([t[perm[i:i + piece]] for i in range(0, perm.numel(), piece)]).contiguous()


def other_library(path, world, camera, env=None):
    """A renderer of another library beside this tree's (the parent's has none of the new symbols to declare)."""
    hidden = {k: (L.SIGNATURES if k in L.SIGNATURES else L.EXTRA).pop(k) for k in NEW} if env is None else {}
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        with L.use_library(path):
            return Renderer(world, camera, device=0)
    finally:
        for k, v in hidden.items():
            (L.EXTRA if k.startswith("rtc_diag") else L.SIGNATURES)[k] = v
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


name, w, h = CASES[args.case]
if args.quick:
    w, h = w // 4, h // 4
kw = {"jitter": ("hashed", scenes.DEFAULT_SEED)} if name == "soft_shadows" else {}
world, camera, depth = getattr(scenes, name)(w, h, **kw)
n = w * h
branch = Renderer(world, camera, device=0)
parent = other_library(args.parent_lib, world, camera) if args.parent_lib else None
dev = {}
if os.path.exists(L.DEV_LIB_PATH):
    dev = {"origin-major": other_library(L.DEV_LIB_PATH, world, camera, {"RTC_AMD_REORDER_DIR_MAJOR": "0"}),
           "direction-major": other_library(L.DEV_LIB_PATH, world, camera, {"RTC_AMD_REORDER_DIR_MAJOR": "1"})}
image = branch.camera_rays()
torch.cuda.synchronize()
streams = {"image": image}
for what, perm in (("tile", tile_order(w, h)), ("random", torch.randperm(n, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1)))):
    streams[what] = tuple(take(t, perm) for t in image)
    del perm
hits = branch.trace_hits(*streams["tile"][:2], keys=streams["tile"][2], planes=("object", "over_point", "reflectv"))
o2, d2, index = rays.reflected(hits, streams["tile"][1])
streams["bounce"] = (o2.contiguous(), d2.contiguous(), streams["tile"][2].index_select(0, index).contiguous())
del hits, o2, d2, index
n2 = int(streams["bounce"][0].shape[0])
out = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")


def route(r, what, reorder):
    m = int(streams[what][0].shape[0])
    return lambda: call_ms(r, depth, streams[what], out[:m], args.frames, reorder)


routes = []
for what in ("tile", "image", "random"):
    if parent is not None:
        routes.append(("plain, %s, parent" % what, route(parent, what, False)))
    routes.append(("plain, %s" % what, route(branch, what, False)))
    routes.append(("reordered, %s" % what, route(branch, what, True)))
routes.append(("plain, bounce", route(branch, "bounce", False)))
routes.append(("reordered, bounce", route(branch, "bounce", True)))
for layout, r in dev.items():
    routes.append(("%s, random" % layout, route(r, "random", True)))
    routes.append(("%s, bounce" % layout, route(r, "bounce", True)))
t = {what: [] for what, _ in routes}
for _, fn in routes:  # warm-up: compiles, scratch
    fn()
for rnd in range(args.rounds):
    for what, fn in (routes if rnd % 2 == 0 else routes[::-1]):
        t[what].append(fn())
say("%s: %s %d x %d, depth %d, %d camera rays, %d second-bounce rays; median (min .. max) of %d rounds x %d launches, ms per call"
    % (args.case, name, w, h, depth, n, n2, args.rounds, args.frames))
say("  trace kernel   %s  %s" % (branch.trace_kernel_name[:90], branch.trace_kernel_id))
for what, _ in routes:
    say("  %-28s %s" % (what, spread(t[what])))
for what in ("tile", "image", "random", "bounce"):
    m = int(streams[what][0].shape[0])
    branch.trace(*streams[what][:2], depth, keys=streams[what][2], out=out[:m], reorder=True)
    rs = branch.reorder_stats()
    whole = sum(rs[p] for p in PHASES)
    plain, re = med(t["plain, %s" % what]), med(t["reordered, %s" % what])
    say("  %-7s phases of one call: %s = %.3f    reordered / plain = %.3f / %.3f = %.2f"
        % (what, "  ".join("%s %.3f" % (p[:-3], rs[p]) for p in PHASES), whole, re, plain, re / plain))
    same = branch.trace(*streams[what][:2], depth, keys=streams[what][2], reorder=False)
    torch.cuda.synchronize()
    say("          reordered == plain, bit for bit: %s" % torch.equal(out[:m], same))
    del same
if parent is not None:
    for what in ("tile", "image", "random"):
        p, b = t["plain, %s, parent" % what], t["plain, %s" % what]
        say("  plain, %s, branch - parent: %+.3f ms; the branch's median is %s the parent's min .. max (%.3f .. %.3f)"
            % (what, med(b) - med(p), "inside" if min(p) <= med(b) <= max(p) else "OUTSIDE", min(p), max(p)))
if dev:
    for what in ("random", "bounce"):
        a, b = med(t["origin-major, %s" % what]), med(t["direction-major, %s" % what])
        say("  key layout on %s: origin-major %.3f, direction-major %.3f (%+.1f %%)" % (what, a, b, 100.0 * (b - a) / a))
if args.keys_out or args.yardstick:
    import tempfile  # noqa: E402
    path = args.keys_out or os.path.join(tempfile.gettempdir(), "reorder_keys_%s_%d.u32" % (args.case, os.getpid()))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    o, d = streams["random"][0].cpu().numpy(), streams["random"][1].cpu().numpy()
    keys = np.zeros(n, dtype=np.uint32)
    import ctypes as C  # noqa: E402
    L.lib().rtc_diag_ray_keys(o.ctypes.data_as(L.FP), d.ctypes.data_as(L.FP), n, None, keys.ctypes.data_as(C.POINTER(C.c_uint32)))
    keys.tofile(path)
    del o, d
    if args.yardstick:
        for r in [branch, parent] + list(dev.values()):
            if r is not None:
                r.close()
        torch.cuda.empty_cache()
        res = subprocess.run([args.yardstick, path], capture_output=True, text=True, timeout=300)  # a fresh child process
        say("  %s" % (res.stdout.strip() or "sort_yardstick failed: " + res.stderr.strip()[-200:]))
        if not args.keys_out:
            os.remove(path)
say()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
