#!/usr/bin/env python3
"""A full equirectangular panorama of a scene from its camera's position: rays the reference's pinhole camera cannot make,
traced against the resident scene on the device (Renderer.trace), formatted as PPM on the device.

    python tools/panorama.py SCENE WxH > out.ppm        e.g.  python tools/panorama.py reflect_refract 1024x512

SCENE: a function of ray_tracer_challenge_amd/scenes.py (soft_shadows, reflect_refract, hexagons, mesh, ...)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ray_tracer_challenge_amd import rays, scenes  # noqa: E402
from ray_tracer_challenge_amd.renderer import Renderer  # noqa: E402


def main():
    if len(sys.argv) != 3 or "x" not in sys.argv[2] or not hasattr(scenes, sys.argv[1]):
        sys.exit(__doc__)
    width, height = (int(v) for v in sys.argv[2].split("x"))
    world, camera, depth = getattr(scenes, sys.argv[1])()
    r = Renderer(world, camera, device=0)
    # where the scene's own camera stands: transform_inverse * point(0, 0, 0), camera.rs:70
    position = np.asarray(camera.transform_inverse, dtype=np.float32).reshape(4, 4)[:3, 3]
    origins, directions = rays.equirectangular(width, height, position, device=r.device)
    colors = r.trace(origins, directions, depth)  # ray i draws its light samples as pixel i of the panorama
    sys.stdout.buffer.write(r.to_ppm(colors.reshape(height, width, 3)))
    print("%s: %d rays, %s" % (sys.argv[1], width * height, r.trace_kernel_name), file=sys.stderr)
    r.close()


if __name__ == "__main__":
    main()
