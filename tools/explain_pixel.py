#!/usr/bin/env python3
"""development: the first-hit record of some pixels, device and oracle side by side, and the first field that differs.

    python tools/explain_pixel.py soft_shadows 100x40 12,7 55,30      # a scene of scenes.py, width x height, x,y ...
    python tools/explain_pixel.py wide:84 - 3,3                       # a tests/wide_worlds.py seed at its own size
    python tools/explain_pixel.py wide:84 640x420 --differing 5       # ... the first five pixels whose rendered colour differs

A pixel whose colour differs from the oracle's is attributed directly: wrong object, wrong distance, wrong normal, wrong
containers (n1n2), wrong light fraction -- or "geometry and light equal: the shading differs".  The device's record comes
from Renderer.render_hits (the kernel family a render of the scene takes) and from World.hit_at on the pixel's ray (the
generic loops); the oracle's from World::intersect -> Intersection::hit -> precompute_values -> intensity_at."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import ray_tracer_challenge_amd as P
from oracle import oracle as O
from ray_tracer_challenge_amd import scenes
from ray_tracer_challenge_amd.renderer import Renderer
from tests import helpers as H
from tests import hits_helpers as HH
from tests import wide_worlds as W


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    what, size = argv[0], None if argv[1] == "-" else tuple(int(v) for v in argv[1].split("x"))
    if what.startswith("wide:"):
        seed = int(what[5:])
        world, cam, depth, style = W.world(seed, P)
        own = W.world(seed, O)[0]
        camera = P.Camera(*cam) if size is None else P.Camera(size[0], size[1], cam[2], cam[3])
        what += " [%s]" % style
    else:
        world, camera, depth = getattr(scenes, what)(*(size or ()))
        own = H.oracle_world(world)
    w, h = camera.width, camera.height
    r = Renderer(world, camera, device=0)
    frame = {k: v.cpu().numpy().reshape((h * w,) + tuple(v.shape[2:])) for k, v in r.render_hits(planes=HH.PLANES).items()}
    if argv[2] == "--differing":
        img = r.render(depth).cpu().numpy()
        exp, _ = H.oracle_camera(camera).render(own, depth, threads=min(16, len(os.sched_getaffinity(0))))
        ys, xs = np.nonzero(~((img == exp) | (np.isnan(img) & np.isnan(exp))).all(axis=2))
        print("%s %dx%d depth %d (%s): %d pixels differ" % (what, w, h, depth, r.kernel_name, len(ys)))
        pixels = list(zip(xs, ys))[:int(argv[3]) if len(argv) > 3 else 4]
    else:
        pixels = [tuple(int(v) for v in a.split(",")) for a in argv[2:]]
    o, d = HH.camera_rays(camera)
    for x, y in pixels:
        i = int(y) * w + int(x)
        traced = x < w - 1 and y < h - 1
        exp = HH.oracle_first_hits(own, o[i:i + 1], d[i:i + 1], pixels=[i]) if traced else HH.empty_planes(1)
        batch = world.hit_at(o[i:i + 1], d[i:i + 1]).planes()  # (a single ray's jitter key is pixel 0: its light plane is only the frame's where the jitter is constant)
        print("pixel (%d, %d)%s  ray %s -> %s" % (x, y, "" if traced else " -- last row / column: never traced", o[i, :3], d[i, :3]))
        print("  %-12s %-44s %-44s %s" % ("plane", "render_hits", "oracle", "hit_at (generic loops)"))
        first = None
        for k in HH.PLANES:
            g, e, b = frame[k][i], exp[k][0], batch[k][0]
            ok = bool(np.all(HH.same(g, e)))
            if not ok and first is None:
                first = k
            note = "" if k == "light" or bool(np.all(HH.same(b, g))) else "   <- differs from render_hits"
            print("  %-12s %-44s %-44s %s%s%s" % (k, np.array2string(np.asarray(g), precision=9), np.array2string(np.asarray(e), precision=9),
                                                np.array2string(np.asarray(b), precision=9), note, "" if ok else "   <== DIFFERS"))
        print("  first field that differs: %s" % (first or "none -- geometry and light are equal: a colour difference here is in the shading"))
    r.close()


if __name__ == "__main__":
    main(sys.argv[1:])
