#!/usr/bin/env python3
"""Adaptive supersampling (Renderer.render_adaptive) against what the same user had before it.  Four routes per configuration,
in one process, alternating -- every other round in the reverse order, and two untimed frames after every change of kernel
(tools/time_supersample.py says why) -- after warm-up (the schedule settles by the third frame):

  (a) render_adaptive: the base render, the mask and list kernel, the refinement kernel
  (b) the plain render
  (c) uniform supersampling, Renderer(..., supersample=k)
  (d) the composed route from the calls that existed before: render -> a torch mask -> camera_rays of the fine camera ->
      gather the flagged pixels' rays -> trace with keys -> reduce -> scatter (tests/test_gpu_adaptive.py section 3)

    python tools/time_adaptive.py [--out profiles/adaptive_times.txt] [--rounds 5] [--frames 10] [--quick] [--threshold 0.1]

Every route is timed the same way: HIP events on the stream around `frames` whole calls, divided by `frames` -- what a caller
waits for, the launches' gaps included.  (a)'s own mask_ms and refine_ms (rtc_adaptive_stats) are the last frame's.  (d) is
timed twice: with the fine camera's rays made once outside the loop (they do not change while the camera stands still: 32 B per
fine ray stay resident), and made anew every frame.  Peak memory: torch's allocator (canvases, rays, temporaries); the library's
own buffers -- (a)'s list of W x H words among them -- are reported from the frame size."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--threshold", type=float, default=0.1)
ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
ap.add_argument("--only", type=int, default=None, help="one configuration, by index")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ray_tracer_challenge_amd import scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402

# (scene, output size, k): tools/time_supersample.py's configurations
CASES = [("soft_shadows", 4096, 2), ("soft_shadows", 2048, 4), ("reflect_refract", 2048, 2), ("mesh", 2048, 2), ("sphere_grid", 4096, 2)]
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def event_ms(fn, frames):
    for _ in range(2):  # untimed: the device goes from the work before to this kernel
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(frames):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / frames


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))


def torch_mask(B, t):
    M = torch.zeros(B.shape[:2], dtype=torch.bool, device=B.device)
    dx = ((B[:, 1:] - B[:, :-1]).abs() > t).any(dim=2)
    dy = ((B[1:] - B[:-1]).abs() > t).any(dim=2)
    M[:, :-1] |= dx
    M[:, 1:] |= dx
    M[:-1] |= dy
    M[1:] |= dy
    return M


class Composed:
    """Route (d)."""

    def __init__(self, r, camera, depth, k, threshold, out):
        self.r, self.depth, self.k, self.out = r, depth, k, out
        self.fine = camera.supersampled(k)
        self.t = torch.tensor(threshold, dtype=torch.float32, device=out.device)
        self.sub = torch.arange(k, device=out.device)
        self.rays = None

    def make_rays(self):
        self.rays = self.r.camera_rays(self.fine)

    def frame(self, fresh_rays=False):
        r, k, fw, fh = self.r, self.k, self.fine.width, self.fine.height
        if fresh_rays or self.rays is None:
            self.make_rays()
        origins, directions, keys = self.rays
        B = r.render(self.depth, out=self.out)
        ys, xs = torch_mask(B, self.t).nonzero(as_tuple=True)
        fy = (ys[:, None, None] * k + self.sub[None, :, None]).expand(-1, k, k)
        fx = (xs[:, None, None] * k + self.sub[None, None, :]).expand(-1, k, k)
        traced = (fx < fw - 1) & (fy < fh - 1)
        idx = (fy * fw + fx)[traced]
        cols = r.trace(origins[idx], directions[idx], self.depth, keys=keys[idx])
        v = torch.zeros(fy.shape + (3,), dtype=torch.float32, device=B.device)
        v[traced] = cols
        if k == 2:
            rows = v[:, :, 0] + v[:, :, 1]
            S = (rows[:, 0] + rows[:, 1]) * 0.25
        else:
            rows = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
            S = ((rows[:, 0] + rows[:, 1]) + (rows[:, 2] + rows[:, 3])) * 0.0625
        B[ys, xs] = S
        return B


def time_case(name, size, k):
    if args.quick:
        size //= 4
    world, camera, depth = getattr(scenes, name)(size, size)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    r = Renderer(world, camera, device=0)           # (a), (b) and (d): one context, as one user has
    uniform = Renderer(world, camera, device=0, supersample=k)  # (c)
    out_a, out_b, out_c, out_d = r.alloc(), r.alloc(), uniform.alloc(), r.alloc()
    mask = torch.empty((size, size), dtype=torch.uint8, device=out_a.device)
    composed = Composed(r, camera, depth, k, args.threshold, out_d)
    routes = {
        "a": lambda: r.render_adaptive(depth, k=k, threshold=args.threshold, out=out_a),
        "b": lambda: r.render(depth, out=out_b),
        "c": lambda: uniform.render(depth, out=out_c),
        "d": lambda: composed.frame(),
        "d+rays": lambda: composed.frame(fresh_rays=True),
    }
    peaks = {}
    for key, fn in routes.items():  # warm-up: kernels compiled, schedules settled; and each route's peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
    times = {key: [] for key in routes}
    order = list(routes)
    for rnd in range(args.rounds):
        for key in (order if rnd % 2 == 0 else order[::-1]):
            times[key].append(event_ms(routes[key], args.frames))
    # what (a) did, and that (a) and (d) agree
    r.render_adaptive(depth, k=k, threshold=args.threshold, out=out_a, mask=mask)
    ad = r.adaptive_stats()
    composed.frame()
    torch.cuda.synchronize()
    share = ad["refined_pixels"] / float(size * size)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rng = lambda v: max(v) - min(v)  # noqa: E731
    say("%s %dx%d k=%d threshold %g: %.1f %% of the pixels flagged (%d); median (min .. max) of %d rounds x %d frames, ms per frame"
        % (name, size, size, k, args.threshold, 100.0 * share, ad["refined_pixels"], args.rounds, args.frames))
    say("  (a) render_adaptive      %s    base %s" % (spread(times["a"]), r.kernel_name[:50]))
    say("      of the last frame: mask %.3f, refinement %.3f (%s), %d rays" % (ad["mask_ms"], ad["refine_ms"], r.adaptive_kernel_name[:50], ad["rays"]))
    say("  (b) plain render         %s" % spread(times["b"]))
    say("  (c) uniform supersample  %s    %s" % (spread(times["c"]), uniform.kernel_name[:50]))
    say("  (d) composed, rays kept  %s    trace %s" % (spread(times["d"]), r.trace_kernel_name[:50]))
    say("      composed, rays made  %s" % spread(times["d+rays"]))
    say("  (a) - (b): %+.3f ms    (a) / (c): %.3f    (a) / (d): %.3f" % (med(times["a"]) - med(times["b"]), med(times["a"]) / med(times["c"]), med(times["a"]) / med(times["d"])))
    for other in ("c", "d"):
        gap, bar = med(times[other]) - med(times["a"]), max(rng(times["a"]), rng(times[other]))
        say("  (%s) - (a) = %+.3f ms against the larger spread of the two routes' rounds, %.3f ms: (a) is %s"
            % (other, gap, bar, "faster" if gap > bar else "slower" if -gap > bar else "within the spread"))
    say("  peak device memory beyond the canvas (torch allocator): (a) %.1f MB + the library's list %.1f MB, (c) %.1f MB, (d) %.1f MB of which rays %.1f MB"
        % (peaks["a"] / 1e6, size * size * 4 / 1e6, peaks["c"] / 1e6, (peaks["d+rays"]) / 1e6, (k * size) ** 2 * 36 / 1e6))
    say("  (a) == (d), bit for bit: %s" % torch.equal(out_a, out_d))
    r.close(), uniform.close()


say("device: %s" % torch.cuda.get_device_name(0))
for i, case in enumerate(CASES):
    if args.only is not None and i != args.only:
        continue
    time_case(*case)
    say()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.only is not None else "w") as f:
        f.write("\n".join(lines) + "\n")
