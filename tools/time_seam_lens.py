#!/usr/bin/env python3
"""Depth of field through the one-call seam (rtc_render_lens): what the one call costs against the route a caller had before it.

    python tools/time_seam_lens.py [--out profiles/seam_lens_times.txt] [--append] [--rounds 5] [--quick] [--cases soft_shadows:4096:2,...]

The cases are those of tools/time_lens.py (profiles/lens_times.txt): C3 at 4096^2 x 2 and 2048^2 x 4, reflect_refract and the mesh at
2048^2 x 2, C5 at 4096^2 x 2, each at R = 0 and at the visible aperture used there; f32 and bytes; page-locked output.  Per row:
  (a) the wall time of one rtc_render_lens call, and the render kernel's time inside it (rtc_stats.kernel_ms: write-through stores,
      progress counters).  The first three calls are not timed: the scene's own kernel is compiled when the scene comes a second time;
  (b) the only route to the same host frame before rtc_render_lens: Renderer(..., lens=).render, quantize for bytes, and a
      synchronous device-to-host copy into page-locked memory, on one stream -- no overlap of render and transfer; wall time;
  (c) the persistent lens kernel's time (the kernel of (b)).
Reported: (a) / (b), and kernel-in-call / (c).  Every figure is the median (min .. max) of --rounds calls in one process, the routes'
calls interleaved; --append adds a run (another process, possibly another machine) to the file instead of replacing it, so that the
spread between runs can be read beside the spread within one."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lines = []

# (scene, output size, k); focal distance and visible aperture of a scene: tools/time_lens.py's
FOCUS = {"soft_shadows": (3.9, 0.15), "reflect_refract": (5.5, 0.2), "mesh": (5.6, 0.2), "sphere_grid": (20.0, 0.6)}
CASES = [("soft_shadows", 4096, 2), ("soft_shadows", 2048, 4), ("reflect_refract", 2048, 2), ("mesh", 2048, 2), ("sphere_grid", 4096, 2)]


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return "%8.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))


def main(args):
    sys.path.insert(0, ROOT)
    import torch

    import ray_tracer_challenge_amd as P
    from ray_tracer_challenge_amd import _lib as L
    from ray_tracer_challenge_amd import scenes
    from ray_tracer_challenge_amd.renderer import Renderer

    lib = P.lib()
    cases = CASES if not args.cases else [(n, int(s), int(k)) for n, s, k in (c.split(":") for c in args.cases.split(","))]
    say("device: %s" % torch.cuda.get_device_name(0))
    say("--rounds %d%s: three untimed calls of each route, then %d timed ones, the routes alternating; page-locked output" % (
        args.rounds, " --quick" if args.quick else "", args.rounds))
    say("ms, median (min .. max); (a) rtc_render_lens, wall; (b) Renderer(lens=).render (+ quantize) + synchronous copy to the host, wall; "
        "(c) the persistent lens kernel")
    dev = (C.c_int32 * 1)(0)
    worst = 0.0

    def seam(cs, cam, depth, k, lens, quantize, ptr):
        st = L.rtc_stats()
        opts = L.rtc_opts(dev, 1, 0, quantize, 0)
        t0 = time.perf_counter()
        L.check(lib.rtc_render_lens(C.byref(cs.scene), C.byref(cam._cam), depth, k, C.byref(lens._c), C.byref(opts), C.c_void_p(ptr), C.byref(st)))
        return (time.perf_counter() - t0) * 1e3, st.kernel_ms

    for name, size, k in cases:
        if args.quick:
            size //= 4
        world, camera, depth = getattr(scenes, name)(size, size)
        cs = world._c()
        focus, aperture = FOCUS[name]
        say("%s %dx%d k=%d (fine %dx%d)" % (name, size, size, k, k * size, k * size))
        for radius in (0.0, aperture):
            lens = P.Lens(radius, focus)
            r = Renderer(world, camera, device=0, supersample=k, lens=lens)
            d_out = r.alloc()
            for quantize in (0, 1):
                host = torch.empty((size, size, 3), dtype=torch.uint8 if quantize else torch.float32, pin_memory=True)
                mine = torch.empty_like(host, pin_memory=True)
                lib.rtc_render_release()
                t_a, k_a, t_b, k_c = [], [], [], []
                for i in range(3 + args.rounds):
                    ms, kms = seam(cs, camera, depth, k, lens, quantize, host.data_ptr())
                    torch.cuda.synchronize()
                    r.stats()
                    t0 = time.perf_counter()
                    img = r.render(depth, out=d_out)
                    mine.copy_(r.quantize(img) if quantize else img)  # synchronous: device -> page-locked host memory
                    ms_b = (time.perf_counter() - t0) * 1e3
                    kc = r.stats()["kernel_ms"]
                    if i >= 3:
                        t_a.append(ms), k_a.append(kms), t_b.append(ms_b), k_c.append(kc)
                reported, chunks = (C.c_uint32 * 2)(), 0
                if lib.rtc_diag_seam_progress(0, reported) == 1:
                    chunks = int(reported[1]) if reported[0] else 0
                seam_name = lib.rtc_ctx_kernel_name(lib.rtc_diag_seam_ctx(0)).decode()
                same = bool((host.numpy() == mine.numpy()).all())
                ratio = med(k_a) / med(k_c)
                worst = max(worst, ratio)
                say("  R=%-4g %-3s (a) %s   (b) %s   (a)/(b) %.2f   kernel in the call %s   (c) %s   ratio %.2f   %s   frames equal: %s" % (
                    radius, "u8" if quantize else "f32", spread(t_a), spread(t_b), med(t_a) / med(t_b), spread(k_a), spread(k_c), ratio,
                    "%d chunk(s) reported" % chunks if chunks else "not reported (block list)", same))
                if quantize:
                    say("         seam kernel: %s" % seam_name[:110])
                del host, mine
            r.close()
        lib.rtc_render_release()
        say()
    say("worst kernel-in-call / (c) of this run: %.2f" % worst)
    say()
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add this run to --out instead of replacing it")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
    ap.add_argument("--cases", default=None, help="scene:size:k,... instead of the five cases")
    a = ap.parse_args()
    rc = main(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(rc)
