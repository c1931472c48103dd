#!/usr/bin/env python3
"""Supersampling through the one-call seam (rtc_render_ss): what it buys, and what it must not cost.

    python tools/time_seam_supersample.py times [--out profiles/seam_supersample_times.txt] [--rounds 5] [--quick]
    python tools/time_seam_supersample.py ab --parent TREE [--out profiles/seam_supersample_ab.txt] [--rounds 5] [--frames 10] [--quick]

times: the wall time of one rtc_render_ss call (the first three calls are not timed: the scene's own kernel is compiled when the
scene comes a second time; --rounds calls from the fourth on) against the two routes a caller had before it, for f32 and bytes, pageable and page-locked output:
  (a) the persistent context, Renderer(supersample=k).render, then a synchronous copy of the frame to the host (plus the
      quantize pass for bytes) -- no overlap of render and transfer, one device;
  (b) rtc_render_ex of the FINE frame (k^2 times the traffic), then the box filter on the host (numpy, the contract's order)
      and, for bytes, scale_color on the host.
Also the render kernel's own time inside the seam call (rtc_stats.kernel_ms: write-through stores, progress counters) against
the persistent context's kernel.

ab: the kernel time of Renderer(supersample=k).render -- no progress words, f32: the launches the persistent context made before
the kernel learnt to report -- with this tree's library against a built checkout of the parent commit (TREE: its root, library
built in place), one process per measurement, the two interleaved, every other round in reverse order.  The margin is the
spread the parent shows against itself."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return "%8.3f (%.3f .. %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))


def med(v):
    return sorted(v)[len(v) // 2]


# ------------------------------------------------------------------------------------------------ ab
def ab_child(scene, size, k, frames):
    """Runs with the tree under test first on sys.path (PYTHONPATH), so the package, its Renderer and its library are that tree's."""
    from ray_tracer_challenge_amd import scenes
    from ray_tracer_challenge_amd.renderer import Renderer
    world, camera, depth = getattr(scenes, scene)(size, size)
    r = Renderer(world, camera, device=0, supersample=k)
    out = r.alloc()
    for _ in range(5):
        r.render(depth, out=out)
    r.stats()
    for _ in range(frames):
        r.render(depth, out=out)
    st = r.stats()
    digest = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:16]
    print(json.dumps({"kernel_ms": st["kernel_ms"], "rays": st["rays"], "hash": digest, "kernel": r.kernel_name, "id": r.kernel_id}))


AB_CASES = [("soft_shadows", 4096, 2), ("soft_shadows", 2048, 4), ("reflect_refract", 2048, 2), ("mesh", 2048, 2)]


def ab(args):
    say("ab --rounds %d --frames %d%s" % (args.rounds, args.frames, " --quick" if args.quick else ""))
    trees = [("parent", os.path.abspath(args.parent)), ("this", ROOT), ("parent again", os.path.abspath(args.parent))]
    for scene, size, k in AB_CASES:
        if args.quick:
            size //= 4
        res, info = {n: [] for n, _ in trees}, {}
        for rnd in range(args.rounds):
            for name, tree in (trees if rnd % 2 == 0 else trees[::-1]):
                env = dict(os.environ)
                env["PYTHONPATH"] = tree
                env.pop("RTC_AMD_LIB", None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "ab-child", scene, str(size), str(k), str(args.frames)], env=env, cwd=tree,
                                   capture_output=True, text=True, timeout=180)  # (a child is seconds: compile, fifteen frames)
                if p.returncode != 0:
                    say("%s FAILED (exit %d) %s" % (name, p.returncode, p.stderr[-600:]))
                    return 1  # (nothing more is started on the device after a failure)
                d = json.loads(p.stdout.strip().splitlines()[-1])
                res[name].append(d["kernel_ms"])
                info[name] = d
        say("%s %dx%d k=%d  Renderer(supersample=k).render kernel ms, median (min .. max) of %d processes x %d frames" % (scene, size, size, k, args.rounds, args.frames))
        for name, _ in trees:
            d = info[name]
            same = (d["hash"], d["rays"]) == (info["parent"]["hash"], info["parent"]["rays"])
            say("  %-13s %s  hash %s %s %s" % (name, spread(res[name]), d["hash"], "" if same else "<-- DIFFERS", d["kernel"][:70]))
        both = res["parent"] + res["parent again"]
        margin = max(abs(med(res["parent"]) - med(res["parent again"])), max(both) - min(both))
        delta = med(res["this"]) - med(both)
        say("  this - parent: %+.4f ms (%+.2f %%); the parent against itself: medians %.4f apart, all runs within %.4f ms -> %s" % (
            delta, 100.0 * delta / med(both), abs(med(res["parent"]) - med(res["parent again"])), max(both) - min(both),
            "within the margin" if delta <= margin else "EXCEEDS the margin"))
        say()
    return 0


# ------------------------------------------------------------------------------------------------ times
TIMES_CASES = [("soft_shadows", 4096, 2), ("soft_shadows", 2048, 4), ("reflect_refract", 2048, 2), ("sphere_grid", 8192, 2)]


def times(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import ray_tracer_challenge_amd as P
    from ray_tracer_challenge_amd import _lib as L
    from ray_tracer_challenge_amd import scenes
    from ray_tracer_challenge_amd.renderer import Renderer
    from tests.supersample_helpers import box_filter

    lib = P.lib()
    say("device: %s" % torch.cuda.get_device_name(0))
    say("times --rounds %d%s: three untimed calls, then %d timed ones" % (args.rounds, " --quick" if args.quick else "", args.rounds))
    say("wall ms of one call, median (min .. max); seam: rtc_render_ss; (a) persistent context + synchronous copy (+ quantize); (b) rtc_render_ex of the fine frame + host box filter")
    dev = (C.c_int32 * 1)(0)

    def seam(cs, cam, depth, k, quantize, ptr):
        st = L.rtc_stats()
        opts = L.rtc_opts(dev, 1, 0, quantize, 0)
        t0 = time.perf_counter()
        if k == 1:
            L.check(lib.rtc_render_ex(C.byref(cs.scene), C.byref(cam._cam), depth, C.byref(opts), C.c_void_p(ptr), C.byref(st)))
        else:
            L.check(lib.rtc_render_ss(C.byref(cs.scene), C.byref(cam._cam), depth, k, C.byref(opts), C.c_void_p(ptr), C.byref(st)))
        return (time.perf_counter() - t0) * 1e3, st.kernel_ms

    for name, size, k in TIMES_CASES:
        if args.quick:
            size //= 4
        world, camera, depth = getattr(scenes, name)(size, size)
        fine_camera = camera.supersampled(k)
        cs = world._c()
        say("%s %dx%d k=%d (fine %dx%d)" % (name, size, size, k, k * size, k * size))
        r = Renderer(world, camera, device=0, supersample=k)
        d_out = r.alloc()
        for _ in range(3):
            r.render(depth, out=d_out)
        torch.cuda.synchronize()
        r.stats()
        ctx_kernel = []
        for _ in range(args.rounds):
            r.render(depth, out=d_out)
            torch.cuda.synchronize()
            ctx_kernel.append(r.stats()["kernel_ms"])
        rounds_b = 1 if k * size > 8192 else max(2, args.rounds // 2)  # (the host filter of a 16384^2 frame takes seconds)
        for quantize in (0, 1):
            for pinned in (0, 1):
                dtype = torch.uint8 if quantize else torch.float32
                host = torch.empty((size, size, 3), dtype=dtype, pin_memory=bool(pinned))
                fine_host = torch.empty((k * size, k * size, 3), dtype=torch.float32, pin_memory=bool(pinned))
                lib.rtc_render_release()
                t_seam, k_seam, t_a, t_b = [], [], [], []
                for i in range(3 + args.rounds):  # (first call: ahead-of-time kernels; second: compiles; then the compiled kernel)
                    ms, kms = seam(cs, camera, depth, k, quantize, host.data_ptr())
                    if i >= 3:
                        t_seam.append(ms), k_seam.append(kms)
                seam_frame = host.numpy().copy()
                for i in range(1 + args.rounds):
                    t0 = time.perf_counter()
                    img = r.render(depth, out=d_out)
                    host.copy_(r.quantize(img) if quantize else img)  # synchronous: device -> host, page-locked or pageable
                    if i:
                        t_a.append((time.perf_counter() - t0) * 1e3)
                same_a = bool((host.numpy() == seam_frame).all())
                lib.rtc_render_release()
                for i in range(3):
                    seam(cs, fine_camera, depth, 1, 0, fine_host.data_ptr())
                for i in range(rounds_b):
                    t0 = time.perf_counter()
                    seam(cs, fine_camera, depth, 1, 0, fine_host.data_ptr())
                    img = box_filter(fine_host.numpy(), k)
                    if quantize:
                        img = np.maximum(np.minimum(img * np.float32(255.0), np.float32(255.0)), np.float32(0.0)).astype(np.uint8)
                    t_b.append((time.perf_counter() - t0) * 1e3)
                same_b = bool((img == seam_frame).all())
                say("  %-3s %-11s seam %s   (a) %s   (b) %s   seam/(a) %.2f  seam/(b) %.3f  frames equal: (a) %s (b) %s" % (
                    "u8" if quantize else "f32", "page-locked" if pinned else "pageable", spread(t_seam), spread(t_a), spread(t_b),
                    med(t_seam) / med(t_a), med(t_seam) / med(t_b), same_a, same_b))
                say("      kernel ms inside the seam call %s   persistent context %s   ratio %.2f" % (spread(k_seam), spread(ctx_kernel), med(k_seam) / med(ctx_kernel)))
                del host, fine_host
        r.close()
        lib.rtc_render_release()
        say()
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ab-child":
        ab_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        sys.exit(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("times", "ab"))
    ap.add_argument("--parent", help="ab: the root of a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="a quarter of the sizes (a rehearsal)")
    a = ap.parse_args()
    if a.mode == "ab" and not a.parent:
        ap.error("ab needs --parent TREE")
    rc = ab(a) if a.mode == "ab" else times(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(rc)
