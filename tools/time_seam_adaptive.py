#!/usr/bin/env python3
"""Adaptive supersampling through the one-call seam (rtc_render_adaptive): what the one call costs against the routes a caller had.

    python tools/time_seam_adaptive.py [--out profiles/seam_adaptive_times.txt] [--append] [--rounds 5] [--quick] [--cases soft_shadows:4096:2,...]

The cases are those of tools/time_adaptive.py (profiles/adaptive_times.txt): C3 at 4096^2 x 2 and 2048^2 x 4, reflect_refract and the
mesh at 2048^2 x 2, C5 at 4096^2 x 2, threshold 0.1; f32 and bytes; page-locked output.  Per row, wall times:
  (a) one rtc_render_adaptive call, one entry;
  (b) the only route to that host frame before: Renderer.render_adaptive, quantize for bytes, and a synchronous device-to-host copy
      into page-locked memory, on one stream -- one device, no overlap, no bands;
  (c) rtc_render_ss at the same k: uniform supersampling through the seam.
Then the halo cost: (a) with two and five entries of device 0 at band_rows 64 and 16, against one entry, with the halo pixels and rays.
The first three calls of every route are not timed (the scene's own kernels are compiled when the scene comes a second time); every
figure is the median (min .. max) of --rounds calls in one process, the routes' calls interleaved.  Ratios are reported as measured."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lines = []
THRESHOLD = 0.1
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
    say("--rounds %d%s: three untimed calls of each route, then %d timed ones, the routes alternating; threshold %g; page-locked output" % (
        args.rounds, " --quick" if args.quick else "", args.rounds, THRESHOLD))
    say("ms, median (min .. max), wall; (a) rtc_render_adaptive; (b) Renderer.render_adaptive (+ quantize) + synchronous copy to the host; (c) rtc_render_ss")

    def seam(cs, cam, depth, k, quantize, ptr, entries=1, band_rows=0, uniform=False):
        st, ad = L.rtc_stats(), L.rtc_seam_adaptive_stats()
        dev = (C.c_int32 * entries)(*([0] * entries))
        opts = L.rtc_opts(dev, entries, band_rows, quantize, 0)
        t0 = time.perf_counter()
        if uniform:
            L.check(lib.rtc_render_ss(C.byref(cs.scene), C.byref(cam._cam), depth, k, C.byref(opts), C.c_void_p(ptr), C.byref(st)))
        else:
            L.check(lib.rtc_render_adaptive(C.byref(cs.scene), C.byref(cam._cam), depth, k, THRESHOLD, C.byref(opts), C.c_void_p(ptr), None, C.byref(st), C.byref(ad)))
        return (time.perf_counter() - t0) * 1e3, st, ad

    for name, size, k in cases:
        if args.quick:
            size //= 4
        world, camera, depth = getattr(scenes, name)(size, size)
        cs = world._c()
        say("%s %dx%d k=%d" % (name, size, size, k))
        r = Renderer(world, camera, device=0)
        for quantize in (0, 1):
            host = torch.empty((size, size, 3), dtype=torch.uint8 if quantize else torch.float32, pin_memory=True)
            mine = torch.empty_like(host, pin_memory=True)
            other = torch.empty_like(host, pin_memory=True)
            lib.rtc_render_release()
            t_a, t_b, t_c, last = [], [], [], None
            for i in range(3 + args.rounds):
                ms_a, st, ad = seam(cs, camera, depth, k, quantize, host.data_ptr())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                img = r.render_adaptive(depth, k=k, threshold=THRESHOLD, mask=None)
                mine.copy_(r.quantize(img) if quantize else img)  # synchronous: device -> page-locked host memory
                ms_b = (time.perf_counter() - t0) * 1e3
                ms_c, _, _ = seam(cs, camera, depth, k, quantize, other.data_ptr(), uniform=True)
                if i >= 3:
                    t_a.append(ms_a), t_b.append(ms_b), t_c.append(ms_c)
                last = (st, ad)
            st, ad = last
            same = bool((host.numpy() == mine.numpy()).all())
            say("  %-3s (a) %s   (b) %s   (c) %s   (a)/(b) %.2f   (a)/(c) %.2f   flagged %.2f %%   base kernel %.3f mask %.3f refine %.3f ms   frames equal: %s" % (
                "u8" if quantize else "f32", spread(t_a), spread(t_b), spread(t_c), med(t_a) / med(t_b), med(t_a) / med(t_c),
                100.0 * ad.refined_pixels / (size * size), st.kernel_ms, ad.mask_ms, ad.refine_ms, same))
            one = med(t_a)
            for entries in (2, 5):
                for band_rows in (64, 16):
                    t_h = []
                    for i in range(3 + args.rounds):
                        ms, st, ad = seam(cs, camera, depth, k, quantize, other.data_ptr(), entries, band_rows)
                        if i >= 3:
                            t_h.append(ms)
                    say("      %d entries, band_rows %-2d: %s   / one entry %.2f   halo pixels %d (%.2f %% of the frame) rays %d   frames equal: %s" % (
                        entries, band_rows, spread(t_h), med(t_h) / one, ad.halo_pixels, 100.0 * ad.halo_pixels / (size * size), ad.halo_rays,
                        bool((other.numpy() == host.numpy()).all())))
            del host, mine, other
        r.close()
        lib.rtc_render_release()
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
