#!/usr/bin/env python3
"""Supersampled rendering against what the same user had before it: the plain render of the fine camera plus a filter pass
over the fine tensor in torch.  Both routes in one process, alternating -- every other round in the reverse order, and two
untimed frames after every change of kernel: the first frames after another kind of work (the memory-bound filter, the other
kernel) run up to 8 % slower, whichever kernel they are -- after warm-up (the schedule settles by the third frame).

    python tools/time_supersample.py [--out profiles/supersample_times.txt] [--rounds 5] [--frames 10] [--quick]

kernel ms: the library's HIP-event time of the render kernel (rtc_stats.kernel_ms), mean over a round's frames; filter ms: HIP
events around the torch pass, the faster of reshape/sum and avg_pool2d.  Peak memory: torch's allocator (the canvases and the
filter's temporaries; the library's own buffers -- records, counters, lists -- are the same order for both routes and not in it).
compile s: the scene's kernel is compiled in this process (RTC_AMD_JIT_CACHE=0 unless the caller sets it): wall time of making the
context the first time minus the second time, when the kernel is in the process's memory."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
args = ap.parse_args()
sys.path.insert(0, ROOT)
os.environ.setdefault("RTC_AMD_JIT_CACHE", "0")  # every scene kernel is compiled here, once: its compile time is part of the report
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ray_tracer_challenge_amd import scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402

# (scene, output size, k): C3 at 4096^2 x 2 and 2048^2 x 4, reflect_refract and mesh 2048^2 x 2; C5 for what declining the scene
# tiles / scene rectangle costs a supersampled context
CASES = [("soft_shadows", 4096, 2), ("soft_shadows", 2048, 4), ("reflect_refract", 2048, 2), ("mesh", 2048, 2), ("sphere_grid", 4096, 2)]
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def kernel_ms(r, depth, out, frames):
    for _ in range(2):  # untimed: the device goes from the work before to this kernel
        r.render(depth, out=out)
    r.stats()
    for _ in range(frames):
        r.render(depth, out=out)
    return r.stats()["kernel_ms"]


def filter_sum(fine, k):
    h, w = fine.shape[0] // k, fine.shape[1] // k
    return fine.reshape(h, k, w, k, 3).sum(dim=(1, 3)) * (1.0 / (k * k))


def filter_pool(fine, k):
    return F.avg_pool2d(fine.permute(2, 0, 1).unsqueeze(0), k).squeeze(0).permute(1, 2, 0).contiguous()


def event_ms(fn, frames):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(frames):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / frames


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))


def make(world, camera, k):
    """The context, made twice: (renderer, seconds the first making spent on what the second did not -- the kernel's compile)."""
    t0 = time.perf_counter()
    Renderer(world, camera, device=0, supersample=k).close()
    t1 = time.perf_counter()
    r = Renderer(world, camera, device=0, supersample=k)
    return r, (t1 - t0) - (time.perf_counter() - t1)


def time_case(name, size, k):
    if args.quick:
        size //= 4
    world, camera, depth = getattr(scenes, name)(size, size)
    fine_camera = camera.supersampled(k)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fused, c_fused = make(world, camera, k)
    out = fused.alloc()
    kernel_ms(fused, depth, out, 4)
    peak_fused = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    plain, c_plain = make(world, fine_camera, 1)
    fine = plain.alloc()
    kernel_ms(plain, depth, fine, 4)
    filters = {"reshape/sum": filter_sum, "avg_pool2d": filter_pool}
    for f in filters.values():
        f(fine, k)
    torch.cuda.synchronize()
    peak_plain = torch.cuda.max_memory_allocated() - base - out.numel() * 4
    t_fused, t_plain, t_filter = [], [], {n: [] for n in filters}
    for rnd in range(args.rounds):
        for which in ((0, 1) if rnd % 2 == 0 else (1, 0)):
            if which == 0:
                t_fused.append(kernel_ms(fused, depth, out, args.frames))
            else:
                t_plain.append(kernel_ms(plain, depth, fine, args.frames))
    for _ in range(args.rounds):
        for n, f in filters.items():
            f(fine, k)
            t_filter[n].append(event_ms(lambda: f(fine, k), args.frames))
    best = min(t_filter, key=lambda n: sorted(t_filter[n])[len(t_filter[n]) // 2])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    say("%s %dx%d k=%d (fine %dx%d)  median (min .. max) of %d rounds x %d frames, ms" % (name, size, size, k, k * size, k * size, args.rounds, args.frames))
    say("  fused      %-60s kernel %s" % (fused.kernel_name[:60], spread(t_fused)))
    say("  plain fine %-60s kernel %s" % (plain.kernel_name[:60], spread(t_plain)))
    for n in filters:
        say("  filter     %-60s        %s%s" % (n, spread(t_filter[n]), "  <- the faster" if n == best else ""))
    say("  fused / plain fine render alone: %.3f     fused / (render + filter): %.3f" % (med(t_fused) / med(t_plain), med(t_fused) / (med(t_plain) + med(t_filter[best]))))
    say("  fused - plain fine: %+.3f ms; the plain fine render's own spread over the rounds: %.3f ms" % (med(t_fused) - med(t_plain), max(t_plain) - min(t_plain)))
    say("  scene kernel compile: fused %.2f s, plain fine %.2f s" % (c_fused, c_plain))
    say("  peak device memory (torch allocator): fused %.1f MB, render + filter %.1f MB" % (peak_fused / 1e6, peak_plain / 1e6))
    same = torch.equal(out, filter_sum(fine, k))  # (torch's sum order is its own: a report, not the contract -- tests/test_gpu_supersample.py is)
    say("  fused == torch reshape/sum of the fine frame, bit for bit: %s" % same)
    fused.close(), plain.close()


say("device: %s" % torch.cuda.get_device_name(0))
for case in CASES:
    time_case(*case)
    say()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
