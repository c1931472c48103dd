#!/usr/bin/env python3
"""development (no GPU needed): what the compiler makes of every kernel, from one csrc directory or from two side by side.

    python tools/codegen_table.py CSRC [OTHER_CSRC] [--out FILE]

Per kernel: VGPRs, SGPRs, scratch bytes per lane, LDS bytes (the code object's metadata), instructions, `scratch_`
instructions, v_writelane_b32 + v_readlane_b32 instructions -- SGPR spills into VGPR lanes -- and how many of those stand in front of the
kernel's first v_sqrt_f32 / v_rsq_f32, the primary ray's normalisation in the per-pixel kernels (counted in the assembly, in program order).  Covered: every kernel of the ahead-of-time library (rtc_device.hip, rtc_oneshot.hip,
build.py's flags, device only); the scene kernels of the eight profiled workloads (tools/check_profile_ids.sh), their options
taken from World.scene_plan(camera) and compiled as tools/spec_asm.sh does; C3's supersampling scene kernel at k = 2
(the fine camera's options as rtc_ctx_set_scene_ss rewrites them); and, where the directory has rtc_trace.h, the same eight
scenes' ray-stream kernels (the options as rtc_ctx_set_scene rewrites them for rtc_ctx_trace).  With two directories the rows
are compared and every figure that differs is marked.  --trace-pairs FILE: every ray-stream kernel of the first directory next
to its render sibling (profiles/trace_codegen.txt).  --hits-pairs FILE: every ray-stream first-hit and occlusion kernel
(csrc/rtc_hits.h: trace_hits_kernel, shadowed_kernel) next to its sibling, hits_kernel of the same instantiation or the batched
is_shadowed_kernel (profiles/trace_hits_codegen.txt); given alone, only rtc_device.hip is compiled.

Build first (python -m ray_tracer_challenge_amd.build --all, in this tree and in the tree of any other directory named): the
scenes' option lists come from this tree's library, and rtc_device.hip includes the literal the build generates beside it.
The figures are read from the assembly as this compiler writes it: one metadata entry per kernel, opening with .agpr_count,
and a kernel's instructions between its label and its .Lfunc_end."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ray_tracer_challenge_amd import scenes  # noqa: E402

SCENES = [("C3", "soft_shadows", 4096, 4096), ("C4", "glass_and_mirror", 4096, 4096), ("C5", "sphere_grid", 8192, 8192),
          ("hexagons", "hexagons", 4096, 2048), ("mesh", "mesh", 2048, 2048), ("dragons", "here_be_dragons", 1000, 400),
          ("reflect_refract", "reflect_refract", 4096, 2048), ("first_textures", "first_textures", 4096, 2048)]
FIGURES = ("vgpr", "sgpr", "scratch", "lds", "insts", "scratch_insts", "lane_insts", "lane_front")
PAIR_FIGURES = FIGURES[:6]  # (--trace-pairs, --hits-pairs: the six their files have had from the start)


def scene_defs(name, w, h, ss=0, trace=False):
    kw = {"jitter": ("hashed", scenes.DEFAULT_SEED)} if name == "soft_shadows" else {}
    world, camera, _ = getattr(scenes, name)(w, h, **kw)
    if ss:
        camera = camera.supersampled(ss)
    defs = world.scene_plan(camera)[1]["spec_defs"].split()
    if ss or trace:
        off = ("-DRTC_SPEC_BLOCKS_Y=1", "-DRTC_SPEC_RECT=1") + (("-DRTC_SPEC_SHARE=1",) if trace else ())  # (a stream: one lane per ray)
        defs = [d[:-1] + "0" if d in off else d for d in defs]
        defs.append("-DRTC_SPEC_SS=%d" % ss if ss else "-DRTC_SPEC_TRACE=1")
    if not any(d.startswith("-DRTC_WAVES_PER_SIMD=") for d in defs):
        defs.append("-DRTC_WAVES_PER_SIMD=7")
    return defs


def compile_asm(csrc, source, defs, out):
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-I" + csrc,
           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", out, source] + defs
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def read_asm(path):
    """{kernel: figures} of one assembly file."""
    text = open(path).read()
    rows = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        f = dict(re.findall(r"^\s+\.(\w+):\s+(.*)$", m.group(0), re.M))
        rows[f["name"].strip("'")] = {"vgpr": int(f["vgpr_count"]), "sgpr": int(f["sgpr_count"]), "scratch": int(f["private_segment_fixed_size"]),
                                      "lds": int(f["group_segment_fixed_size"])}
    for name, r in rows.items():
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        insts = [ln.split()[0] for ln in body.splitlines() if re.match(r"^\t[a-z]", ln)]
        r["insts"], r["scratch_insts"] = len(insts), sum(1 for i in insts if i.startswith("scratch_"))
        lane = [i in ("v_writelane_b32", "v_readlane_b32") for i in insts]  # SGPRs spilled into VGPR lanes, and read back
        # ... of them, those in front of the kernel's first v_sqrt_f32 / v_rsq_f32 in program order: for the per-pixel kernels that is the
        # primary ray's normalisation, so the figure is what stands between a wave's entry and its first ray (all of them where there is no such instruction)
        first_root = next((n for n, i in enumerate(insts) if i.startswith(("v_sqrt_f32", "v_rsq_f32"))), len(insts))
        r["lane_insts"], r["lane_front"] = sum(lane), sum(lane[:first_root])
    return rows


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void rtc::|\(rtc::\w+\)$|\(.*\)$", "", d) for n, d in zip(names, out)}


def table(csrc, tmp, tag, device_only=False):
    jobs = [("aot " + s, os.path.join(csrc, s), []) for s in ("rtc_device.hip", "rtc_oneshot.hip")[:1 if device_only else 2]]
    spec, ss = os.path.join(tmp, "spec.hip"), os.path.join(tmp, "ss.hip")
    open(spec, "w").write('#include "rtc_kernel_core.h"\n')
    open(ss, "w").write('#include "rtc_supersample.h"\n')
    for scene, name, w, h in ([] if device_only else SCENES):
        jobs.append(("scene " + scene, spec, scene_defs(name, w, h)))
    if not device_only:
        jobs.append(("scene C3 ss=2", ss, scene_defs("soft_shadows", 4096, 4096, ss=2)))
    if os.path.exists(os.path.join(csrc, "rtc_trace.h")) and not device_only:
        trace = os.path.join(tmp, "trace.hip")
        open(trace, "w").write('#include "rtc_trace.h"\n')
        for scene, name, w, h in SCENES:
            jobs.append(("scene %s trace" % scene, trace, scene_defs(name, w, h, trace=True)))
    with ThreadPoolExecutor(8) as ex:
        files = list(ex.map(lambda j: compile_asm(csrc, j[1], j[2], os.path.join(tmp, "%s_%s.s" % (tag, j[0].replace(" ", "_").replace("=", "")))), jobs))
    rows = {}
    for (kind, _, _), f in zip(jobs, files):
        r = read_asm(f)
        pretty = demangle(list(r))
        for k, v in r.items():
            if kind.endswith(" trace") and not pretty[k].startswith("trace_"):
                continue  # (the core's render_kernel_spec is in that compile as well: not a kernel anything launches)
            rows["%s: %s" % (kind, pretty[k])] = v
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csrc", nargs="+")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-pairs", default=None, help="write the ray-stream kernels next to their render siblings here")
    ap.add_argument("--hits-pairs", default=None, help="write the ray-stream first-hit and occlusion kernels next to their siblings here")
    args = ap.parse_args()
    device_only = bool(args.hits_pairs) and not args.out and not args.trace_pairs and len(args.csrc) == 1
    own = os.path.join(ROOT, "ray_tracer_challenge_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        tables = [table(os.path.abspath(c), tmp, "t%d" % i, device_only) for i, c in enumerate(args.csrc)]
    lines = ["figures per kernel: VGPRs / SGPRs / scratch bytes per lane / LDS bytes / instructions / scratch_ instructions / "
             "v_writelane_b32 + v_readlane_b32 instructions / those of them in front of the first v_sqrt_f32 or v_rsq_f32 (the primary ray's normalisation)"]
    if len(tables) == 2:
        lines.append("first: %s   second: %s   (* a figure that differs)" % tuple(os.path.relpath(os.path.abspath(c), ROOT) if os.path.abspath(c) == own else "the parent's csrc" for c in args.csrc))
    differing = []
    for k in sorted(set().union(*tables)):
        cells = [" / ".join(str(t[k][f]) for f in FIGURES) if k in t else "-" for t in tables]
        mark = ""
        if len(tables) == 2 and cells[0] != cells[1]:
            which = [f for f in FIGURES if k not in tables[0] or k not in tables[1] or tables[0][k][f] != tables[1][k][f]]
            mark = "   * " + ", ".join(which)
            differing.append((k, which))
        lines.append("%-110s %s%s" % (k, "   |   ".join("%-48s" % c for c in cells), mark))
    if len(tables) == 2:
        hard = [k for k, which in differing if set(which) & {"vgpr", "scratch", "lds"}]
        lines.append("kernels with a differing figure: %d of %d; with differing VGPRs, scratch bytes or LDS bytes: %d%s"
                     % (len(differing), len(set().union(*tables)), len(hard), "".join("\n    " + k for k in hard)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        open(args.out, "w").write(text)
    if args.trace_pairs:
        t = tables[0]
        pairs = ["ray-stream kernels (csrc/rtc_trace.h) next to their render siblings: VGPRs / SGPRs / scratch bytes per lane / LDS bytes / "
                 "instructions / scratch_ instructions", "%-62s %-36s   |   %-36s %s" % ("kernel", "trace", "render sibling", "scratch, trace - render")]
        for k in sorted(t):
            if ": trace_kernel" not in k:
                continue
            sib = k.replace(" trace: trace_kernel_spec", ": render_kernel_spec").replace(": trace_kernel<", ": render_kernel<")
            cells = [" / ".join(str(t[n][f]) for f in PAIR_FIGURES) if n in t else "-" for n in (k, sib)]
            pairs.append("%-62s %-36s   |   %-36s %+d B" % (k, cells[0], cells[1], t[k]["scratch"] - t[sib]["scratch"] if sib in t else 0))
        open(args.trace_pairs, "w").write("\n".join(pairs) + "\n")
    if args.hits_pairs:
        t = tables[0]
        pairs = ["ray-stream first-hit and occlusion kernels (csrc/rtc_hits.h) next to their siblings: VGPRs / SGPRs / scratch bytes per lane / "
                 "LDS bytes / instructions / scratch_ instructions", "%-58s %-32s   |   %-32s %-32s %s" % ("kernel", "stream", "sibling", "", "scratch, stream - sibling")]
        for k in sorted(t):
            if ": trace_hits_kernel<" in k:
                sib = k.replace(": trace_hits_kernel<", ": hits_kernel<")
            elif ": shadowed_kernel<" in k:
                sib = k[:k.index(": ")] + ": rtc::is_shadowed_kernel"  # (not a template: the mangled name carries no return type)
            else:
                continue
            cells = [" / ".join(str(t[n][f]) for f in PAIR_FIGURES) if n in t else "-" for n in (k, sib)]
            pairs.append("%-58s %-32s   |   %-32s %-32s %+d B" % (k, cells[0], sib.split(": ")[1].replace("rtc::", ""), cells[1], t[k]["scratch"] - t[sib]["scratch"] if sib in t else 0))
        open(args.hits_pairs, "w").write("\n".join(pairs) + "\n")


if __name__ == "__main__":
    main()
