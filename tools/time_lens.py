#!/usr/bin/env python3
"""The thin-lens camera (Renderer(..., supersample=k, lens=...)) against the two things it can be compared with on one commit:
the supersampled frame of the same k -- the price of per-lane origins and incoherent primary rays, at an aperture of zero and
at a visible one -- and the composed path a user had before it: the lens rays resident on the device (rtc_lens_rays makes them
on the host, untimed), Renderer.trace of them, and the reduce in torch.  All routes in one process, alternating, every other
round in the reverse order, two untimed frames after every change of kernel (tools/time_supersample.py says why).

    python tools/time_lens.py [--out profiles/lens_times.txt] [--rounds 5] [--frames 10] [--quick] [--cases soft_shadows:4096:2,...]

kernel ms: the library's HIP-event time of the render / trace kernel (rtc_stats.kernel_ms), mean over a round's frames; reduce
ms: HIP events around the torch pass.  Device memory: torch's allocator -- the canvas for the lens frame; rays (32 B), keys (4 B),
colours (12 B) per fine pixel and the canvas for the composed path."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
ap.add_argument("--cases", default=None, help="scene:size:k,... instead of the default list")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ray_tracer_challenge_amd import Lens, scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402

# (scene, output size, k, focal distance, visible aperture): C3 at 4096^2 x 2 and 2048^2 x 4, reflect_refract and mesh 2048^2 x 2, C5
FOCUS = {"soft_shadows": (3.9, 0.15), "reflect_refract": (5.5, 0.2), "mesh": (5.6, 0.2), "sphere_grid": (20.0, 0.6)}
CASES = [("soft_shadows", 4096, 2), ("soft_shadows", 2048, 4), ("reflect_refract", 2048, 2), ("mesh", 2048, 2), ("sphere_grid", 4096, 2)]
if args.cases:
    CASES = [(n, int(s), int(k)) for n, s, k in (c.split(":") for c in args.cases.split(","))]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()


def say(text=""):
    print(text, flush=True)
    if args.out:  # (line by line: a long run that is cut short keeps what it measured)
        with open(args.out, "a") as f:
            f.write(text + "\n")


def kernel_ms(fn, stats, frames):
    for _ in range(2):  # untimed: the device goes from the work before to this kernel
        fn()
    stats()
    for _ in range(frames):
        fn()
    return stats()["kernel_ms"]


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


def resident_rays(camera, k, lens, device):
    """rtc_lens_rays' rays on the device, made in bands of fine rows (the host never holds the whole stream), and their keys."""
    fw, fh = k * camera.width, k * camera.height
    o = torch.empty((fw * fh, 4), dtype=torch.float32, device=device)
    d = torch.empty((fw * fh, 4), dtype=torch.float32, device=device)
    for y0 in range(0, fh, 256):
        n = min(256, fh - y0)
        ho, hd = camera.lens_rays(k, lens, y0, n)
        o[y0 * fw:(y0 + n) * fw] = torch.from_numpy(ho).to(device)
        d[y0 * fw:(y0 + n) * fw] = torch.from_numpy(hd).to(device)
    keys = torch.arange(fw * fh, dtype=torch.int64, device=device).to(torch.int32)  # (bits of the uint32 index)
    return o, d, keys


def reduce_(colours, fh, fw, k):
    fine = colours.reshape(fh, fw, 3).clone()
    fine[-1] = 0.0
    fine[:, -1] = 0.0
    return fine.reshape(fh // k, k, fw // k, k, 3).sum(dim=(1, 3)) * (1.0 / (k * k))


def time_case(name, size, k):
    if args.quick:
        size //= 4
    world, camera, depth = getattr(scenes, name)(size, size)
    focus, aperture = FOCUS.get(name, (5.0, 0.2))
    fw = fh = k * size
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    routes = {"supersampled": Renderer(world, camera, device=0, supersample=k),
              "lens R=0": Renderer(world, camera, device=0, supersample=k, lens=Lens(0.0, focus)),
              "lens R=%g" % aperture: Renderer(world, camera, device=0, supersample=k, lens=Lens(aperture, focus))}
    out = routes["supersampled"].alloc()
    for r in routes.values():
        kernel_ms(lambda: r.render(depth, out=out), r.stats, 4)
    peak_lens = torch.cuda.max_memory_allocated() - base
    lens_frame = out.clone()  # (the last route's: the visible aperture)
    torch.cuda.reset_peak_memory_stats()
    tracer = routes["lens R=%g" % aperture]
    o, d, keys = resident_rays(camera, k, tracer.lens, tracer.device)
    colours = torch.empty((fw * fh, 3), dtype=torch.float32, device=tracer.device)
    trace = lambda: tracer.trace(o, d, depth, keys=keys, out=colours)  # noqa: E731
    kernel_ms(trace, tracer.stats, 2)
    composed = reduce_(colours, fh, fw, k)
    torch.cuda.synchronize()
    peak_composed = torch.cuda.max_memory_allocated() - base - out.numel() * 4 - lens_frame.numel() * 4
    times = {n: [] for n in routes}
    times["trace of resident lens rays"] = []
    order = list(times)
    for rnd in range(args.rounds):
        for n in (order if rnd % 2 == 0 else order[::-1]):
            if n in routes:
                r = routes[n]
                times[n].append(kernel_ms(lambda: r.render(depth, out=out), r.stats, args.frames))
            else:
                times[n].append(kernel_ms(trace, tracer.stats, max(2, args.frames // 2)))
    t_reduce = [event_ms(lambda: reduce_(colours, fh, fw, k), args.frames) for _ in range(args.rounds)]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    say("%s %dx%d k=%d (fine %dx%d), focus %g  median (min .. max) of %d rounds x %d frames, ms" % (name, size, size, k, fw, fh, focus, args.rounds, args.frames))
    for n in order:
        kn = routes[n].kernel_name if n in routes else tracer.trace_kernel_name
        say("  %-28s %-58s kernel %s" % (n, kn[:58], spread(times[n])))
    say("  %-28s %-58s        %s" % ("torch reduce", "zero last row / column, reshape / sum", spread(t_reduce)))
    ss, l0, lr, tr = (med(times[n]) for n in order)
    say("  lens R=0 / supersampled: %.3f     lens R=%g / supersampled: %.3f     lens R=%g / (trace + reduce): %.3f"
        % (l0 / ss, aperture, lr / ss, aperture, lr / (tr + med(t_reduce))))
    say("  peak device memory (torch allocator): lens frame %.1f MB, composed path %.1f MB" % (peak_lens / 1e6, peak_composed / 1e6))
    say("  lens frame == torch reduce of the traced rays, bit for bit: %s   (torch's sum order is its own: a report; tests/test_gpu_lens.py is the contract)"
        % torch.equal(lens_frame, composed))
    for r in routes.values():
        r.close()


say("device: %s" % torch.cuda.get_device_name(0))
for case in CASES:
    time_case(*case)
    say()
