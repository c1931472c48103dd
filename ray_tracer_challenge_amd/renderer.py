"""Device-resident rendering: scene uploaded once, output left in HBM.

`Renderer` wraps the persistent-context half of the C ABI (rtc_ctx_*).
PyTorch appears here only as plumbing -- it owns the output tensor and the
stream, and (in dist.py) carries the RCCL gather.  The kernel launch itself goes
through librtc_amd.so with raw device pointers.
"""
import ctypes as C

import torch

from . import _lib as L


class Renderer:
    """supersample = k (1, 2 or 4): k x k rays per pixel of `camera`, reduced in the render kernel (rtc_ctx_set_scene_ss).
    width / height, alloc() and rows() speak of the output frame -- `camera`'s -- whatever k is.
    lens = api.Lens(...) with supersample = 2 or 4: depth of field -- the k x k rays of a pixel leave from k x k points of the
    lens (rtc_ctx_set_scene_lens); render_hits and render_adaptive are refused on such a renderer."""

    def __init__(self, world, camera, device=None, supersample=1, lens=None):
        if not torch.cuda.is_available():
            raise L.RtcError(L.RTC_ERR_NO_DEVICE, "no GPU visible to torch; the render path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.width, self.height = camera.width, camera.height
        self._ctx = C.c_void_p()
        self._lib = L.lib()  # the library that owns this context (tests load a second one beside it: _lib.use_library)
        L.check(self._lib.rtc_ctx_create(self.device.index, C.byref(self._ctx)))
        self._keep = None
        self.supersample = 1
        self.lens = None
        self.set_scene(world, camera, supersample=supersample, lens=lens)

    def _set(self, cs, camera, k, lens=None):
        if lens is not None:  # (the library checks the factor: a lens frame takes 2 or 4)
            L.check(self._lib.rtc_ctx_set_scene_lens(self._ctx, C.byref(cs.scene), C.byref(camera._cam), k, C.byref(lens._c)), self._lib)
        elif k == 1:
            L.check(self._lib.rtc_ctx_set_scene(self._ctx, C.byref(cs.scene), C.byref(camera._cam)), self._lib)
        else:
            L.check(self._lib.rtc_ctx_set_scene_ss(self._ctx, C.byref(cs.scene), C.byref(camera._cam), k), self._lib)
        self._keep = (cs, camera)
        self.supersample = k
        self.lens = lens
        self.width, self.height = camera.width, camera.height

    def set_scene(self, world, camera, supersample=1, lens=None):
        """supersample=1 (the default) leaves supersampled mode, lens=None (the default) lens mode."""
        self._set(world._c(), camera, int(supersample), lens)

    def set_camera(self, camera):
        """Another camera on the world that is resident (an animation's usual frame): the world is not flattened again on the
        Python side, and the library, finding the records unchanged, uploads none of them.
        The supersampling factor and the lens stay."""
        self._set(self._keep[0], camera, self.supersample, self.lens)

    def set_lens(self, lens):
        """Another lens on the resident world and camera (a focus pull): nothing is flattened or uploaded.  The renderer must be
        supersampled (2 or 4); lens=None leaves lens mode for the plain supersampled frame."""
        self._set(self._keep[0], self._keep[1], self.supersample, lens)

    def close(self):
        if self._ctx:
            self._lib.rtc_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def partition(band_rows=64, n_parts=1, part=0):
        return L.rtc_partition(band_rows, n_parts, part)

    def rows(self, part=None):
        return int(self._lib.rtc_partition_rows(self.height, C.byref(part) if part is not None else None))

    def alloc(self, part=None):
        return torch.empty((self.rows(part), self.width, 3), dtype=torch.float32, device=self.device)

    def render(self, depth, out=None, part=None, stream=None):
        """Launches the render kernel on `stream` (default: torch's current stream); asynchronous."""
        if out is None:
            out = self.alloc(part)
        # (checked, not asserted: the raw pointer goes to a kernel that writes rows x width x 3 floats through it)
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.rows(part) * self.width * 3):
            raise ValueError("out must be a contiguous float32 CUDA tensor of %d x %d x 3" % (self.rows(part), self.width))
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_render(self._ctx, int(depth), C.byref(part) if part is not None else None,
                                       C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)))
        return out

    def render_adaptive(self, depth, k=2, threshold=0.1, out=None, mask=None, stream=None):
        """Adaptive supersampling (rtc_ctx_render_adaptive) on `stream` (default: torch's current stream); asynchronous.  The
        frame is render()'s, except that every pixel one of whose four neighbours differs from it by more than `threshold` in
        some channel holds the k x k supersampled value instead (k = 2 or 4).  mask: None -> the frame; True -> (frame, mask)
        with a fresh (height, width) uint8 tensor, 1 = refined; a tensor -> written and returned likewise."""
        if out is None:
            out = self.alloc()
        # (checked, not asserted: the raw pointers go to kernels that write height x width x 3 floats / height x width bytes through them)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.float32 and out.is_contiguous()
                and out.numel() == self.height * self.width * 3):
            raise ValueError("out must be a contiguous float32 CUDA tensor of %d x %d x 3 on %s" % (self.height, self.width, self.device))
        if mask is True:
            mask = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        elif mask is False:
            mask = None
        if mask is not None and not (torch.is_tensor(mask) and mask.is_cuda and mask.device == self.device and mask.dtype == torch.uint8
                                     and mask.is_contiguous() and mask.numel() == self.height * self.width):
            raise ValueError("mask must be a contiguous uint8 CUDA tensor of %d x %d on %s" % (self.height, self.width, self.device))
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_render_adaptive(self._ctx, int(depth), int(k), float(threshold), C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(mask.data_ptr()) if mask is not None else None, C.c_void_p(s.cuda_stream)),
                self._lib)
        return out if mask is None else (out, mask)

    def adaptive_stats(self):
        """Synchronises with the last render_adaptive() and returns what its mask and refinement passes did."""
        st = L.rtc_adaptive_stats()
        L.check(self._lib.rtc_ctx_adaptive_stats(self._ctx, C.byref(st)), self._lib)
        return {"refined_pixels": int(st.refined_pixels), "rays": int(st.rays), "shaded_hits": int(st.shaded_hits),
                "culled_shadow_rays": int(st.culled_shadow_rays), "mask_ms": float(st.mask_ms), "refine_ms": float(st.refine_ms)}

    @property
    def adaptive_kernel_name(self):
        """The refinement kernel of the last render_adaptive() ("" before the first of the current scene)."""
        return self._lib.rtc_ctx_adaptive_kernel_name(self._ctx).decode()

    @property
    def adaptive_kernel_id(self):
        """Names the code object of the last render_adaptive()'s refinement, as kernel_id does for renders."""
        return self._lib.rtc_ctx_adaptive_kernel_id(self._ctx).decode()

    def render_hits(self, planes=("object", "distance", "normal", "light"), out=None, part=None, stream=None):
        """The first hit of every pixel's ray (rtc_ctx_render_hits) on `stream` (default: torch's current stream);
        asynchronous.  -> {plane: tensor}: int32 (rows, w) for object / inside, float32 (rows, w) for distance / light,
        float32 (rows, w, 4) for the vector planes, (rows, w, 2) for n1n2.  `out`: tensors to write into, by plane."""
        rows, planes = self.rows(part), tuple(planes)
        if not planes:
            raise ValueError("no plane requested")
        res, hp = {}, L.rtc_hit_planes()
        for k in planes:
            if k not in L.HIT_PLANES:
                raise ValueError("%r is not a plane (%s)" % (k, ", ".join(L.HIT_PLANES)))
            is_int, per = L.HIT_PLANES[k]
            dtype = torch.int32 if is_int else torch.float32
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty((rows, self.width, per) if per > 1 else (rows, self.width), dtype=dtype, device=self.device)
            # (checked, not asserted: the raw pointer goes to a kernel that writes rows x width elements through it, 16 bytes at a time)
            if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == rows * self.width * per and t.data_ptr() % 16 == 0):
                raise ValueError("out[%r] must be a contiguous, 16-byte aligned %s CUDA tensor of %d x %d%s"
                                 % (k, "int32" if is_int else "float32", rows, self.width, " x %d" % per if per > 1 else ""))
            res[k] = t
            setattr(hp, k, t.data_ptr())
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_render_hits(self._ctx, C.byref(part) if part is not None else None, C.byref(hp),
                                              C.c_void_p(s.cuda_stream)), self._lib)
        return res

    def _ray_tensor(self, t, what, n=None):
        # (checked, not asserted: the raw pointer goes to a kernel that reads n x 16 bytes through it, 16 at a time)
        if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 4
                and t.is_contiguous() and t.data_ptr() % 16 == 0 and (n is None or t.shape[0] == n)):
            raise ValueError("%s must be a contiguous, 16-byte aligned float32 CUDA tensor (n, 4) on %s" % (what, self.device))
        return int(t.shape[0])

    def _key_tensor(self, keys, n):
        if keys is not None:
            ok = torch.is_tensor(keys) and keys.is_cuda and keys.device == self.device and keys.dim() == 1 and keys.shape[0] == n and keys.is_contiguous()
            if not (ok and keys.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and keys.data_ptr() % 4 == 0):
                raise ValueError("keys must be a contiguous int32 or uint32 CUDA tensor (n,) on %s" % self.device)

    def trace(self, origins, directions, depth, keys=None, out=None, stream=None, reorder=False):
        """World::color_at for the caller's rays against the resident scene (rtc_ctx_trace) on `stream` (default: torch's
        current stream); asynchronous.  origins, directions: (n, 4) float32 on the renderer's device (x, y, z are read); the
        direction is used as given.  keys: (n,) int32 / uint32 -- ray i draws its light samples as pixel keys[i] (None: i).
        -> (n, 3) float32.
        With `stream` given and no `out`, the result is allocated by torch on its CURRENT stream and written on `stream`: keep it
        alive until `stream` has been waited for (or pass an `out` made on `stream`, or call out.record_stream(stream)).  One
        stream at a time per renderer: two traces in flight on different streams race on what stats() reports.
        reorder=True (rtc_ctx_trace_reordered): the stream is sorted by a coherence key on the device, traced in that order and
        answered in the caller's -- the same bits, element i still ray i's, keys=None still drawing as pixel i.  For streams whose
        neighbours in memory are not neighbours in space (second bounces, shuffled or gathered rays); a coherent stream only pays
        for the sort.  trace_hits() and is_shadowed() do not take the flag: compose them from ray_order() and
        index_select."""
        n = self._ray_tensor(origins, "origins")
        self._ray_tensor(directions, "directions", n)
        self._key_tensor(keys, n)
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.float32 and out.is_contiguous()
                and out.numel() == 3 * n):
            raise ValueError("out must be a contiguous float32 CUDA tensor of %d x 3 on %s" % (n, self.device))
        if not 0 <= n < 2 ** 32:
            raise ValueError("at most 2^32 - 1 rays a call")
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        entry = self._lib.rtc_ctx_trace_reordered if reorder else self._lib.rtc_ctx_trace
        L.check(entry(self._ctx, int(depth), C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                      C.c_void_p(keys.data_ptr()) if keys is not None else None, n, C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)),
                self._lib)
        return out

    def ray_order(self, origins, directions, out=None, stream=None):
        """The coherence order of the caller's rays (rtc_ctx_ray_order) on `stream` (default: torch's current stream);
        asynchronous.  origins, directions: as trace() takes them.  -> (n,) int32: out[j] is the index of the ray that comes j-th
        by key (include/rtc.h spells the key out), ties by index -- origins.index_select(0, order) is the stream trace(reorder=True)
        traces, and what trace_hits() / is_shadowed(), which have no flag of their own, can be given.  No scene is read.
        With `stream` given and no `out`, keep the result alive as for trace()."""
        n = self._ray_tensor(origins, "origins")
        self._ray_tensor(directions, "directions", n)
        if n > 2 ** 31 - 1:
            raise ValueError("at most 2^31 - 1 rays a call (the order is int32)")
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.int32 and out.is_contiguous()
                and tuple(out.shape) == (n,) and out.data_ptr() % 4 == 0):
            raise ValueError("out must be a contiguous int32 CUDA tensor (%d,) on %s" % (n, self.device))
        if n == 0:  # (an empty tensor has no address to give)
            return out
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_ray_order(self._ctx, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()), n,
                                            C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)), self._lib)
        return out

    def reorder_stats(self):
        """Synchronises with the last trace(reorder=True) and returns its phases' HIP-event times (all zero before the first)."""
        st = L.rtc_reorder_stats()
        L.check(self._lib.rtc_ctx_reorder_stats(self._ctx, C.byref(st)), self._lib)
        return {"n": int(st.n), "keys_ms": float(st.keys_ms), "sort_ms": float(st.sort_ms), "gather_ms": float(st.gather_ms),
                "trace_ms": float(st.trace_ms), "scatter_ms": float(st.scatter_ms)}

    def trace_hits(self, origins, directions, keys=None, planes=("object", "distance", "normal", "light"), out=None, stream=None):
        """The first hit of each of the caller's rays against the resident scene (rtc_ctx_trace_hits) on `stream` (default:
        torch's current stream); asynchronous.  origins, directions, keys: as trace() takes them.  -> {plane: tensor}, element
        i belonging to ray i: int32 (n,) for object / inside, float32 (n,) for distance / light, float32 (n, 4) for the vector
        planes, (n, 2) for n1n2; a miss is object -1 and zeros.  `out`: tensors to write into, by plane.
        With `stream` given, a plane that is not in `out` is allocated by torch on its CURRENT stream and written on `stream`:
        keep it alive until `stream` has been waited for (or pass an `out` made on `stream`, or call record_stream(stream) on
        it).  Leaves stats() and the kernel names alone."""
        n = self._ray_tensor(origins, "origins")
        self._ray_tensor(directions, "directions", n)
        self._key_tensor(keys, n)
        planes = tuple(planes)
        if not planes:
            raise ValueError("no plane requested")
        res, hp = {}, L.rtc_hit_planes()
        for k in planes:
            if k not in L.HIT_PLANES:
                raise ValueError("%r is not a plane (%s)" % (k, ", ".join(L.HIT_PLANES)))
            is_int, per = L.HIT_PLANES[k]
            dtype = torch.int32 if is_int else torch.float32
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty((n, per) if per > 1 else (n,), dtype=dtype, device=self.device)
            # (checked, not asserted: the raw pointer goes to a kernel that writes n elements through it, up to 16 bytes at a time)
            if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()
                    and tuple(t.shape) == ((n, per) if per > 1 else (n,)) and t.data_ptr() % (4 * per) == 0):
                raise ValueError("out[%r] must be a contiguous, %d-byte aligned %s CUDA tensor of %d%s on %s"
                                 % (k, 4 * per, "int32" if is_int else "float32", n, " x %d" % per if per > 1 else "", self.device))
            res[k] = t
            setattr(hp, k, t.data_ptr())
        if not 0 <= n < 2 ** 32:
            raise ValueError("at most 2^32 - 1 rays a call")
        if n == 0:  # (an empty tensor has no address to give: nothing to trace, no call)
            return res
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_trace_hits(self._ctx, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                             C.c_void_p(keys.data_ptr()) if keys is not None else None, n, C.byref(hp),
                                             C.c_void_p(s.cuda_stream)), self._lib)
        return res

    def is_shadowed(self, light_positions, points, out=None, stream=None):
        """World::is_shadowed(light_position, point) pair by pair against the resident scene (rtc_ctx_is_shadowed) on `stream`
        (default: torch's current stream); asynchronous.  light_positions, points: (n, 4) float32 on the renderer's device (x,
        y, z are read).  -> (n,) int32, 1: the nearest thing between the two is a shadow caster.
        With `stream` given and no `out`, the result is allocated by torch on its CURRENT stream and written on `stream`: keep
        it alive until `stream` has been waited for (or pass an `out` made on `stream`, or call out.record_stream(stream)).
        Leaves stats() and the kernel names alone."""
        n = self._ray_tensor(light_positions, "light_positions")
        self._ray_tensor(points, "points", n)
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.int32 and out.is_contiguous()
                and tuple(out.shape) == (n,) and out.data_ptr() % 4 == 0):
            raise ValueError("out must be a contiguous int32 CUDA tensor (%d,) on %s" % (n, self.device))
        if not 0 <= n < 2 ** 32:
            raise ValueError("at most 2^32 - 1 pairs a call")
        if n == 0:
            return out
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_is_shadowed(self._ctx, C.c_void_p(light_positions.data_ptr()), C.c_void_p(points.data_ptr()), n,
                                              C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)), self._lib)
        return out

    def camera_rays(self, camera=None, y0=0, n_rows=None, stream=None):
        """ray_for_pixel of `camera` (default: the camera last set) for image rows [y0, y0 + n_rows) (default: to the last),
        made on the device by the render kernels' own function (rtc_ctx_camera_rays), in image order and in trace()'s
        layout.  -> (origins (n, 4), directions (n, 4), keys (n,) int32: y * width + x)."""
        camera = self._keep[1] if camera is None else camera
        y0 = int(y0)
        n_rows = camera.height - y0 if n_rows is None else int(n_rows)
        if y0 < 0 or n_rows < 0 or y0 + n_rows > camera.height:
            raise ValueError("rows [%d, %d) of a camera of %d" % (y0, y0 + n_rows, camera.height))
        n = n_rows * camera.width
        origins = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        directions = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        keys = torch.empty((n,), dtype=torch.int32, device=self.device)
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_camera_rays(self._ctx, C.byref(camera._cam), y0, n_rows, C.c_void_p(origins.data_ptr()),
                                              C.c_void_p(directions.data_ptr()), C.c_void_p(keys.data_ptr()), C.c_void_p(s.cuda_stream)),
                self._lib)
        return origins, directions, keys

    @property
    def trace_kernel_name(self):
        """The kernel of the last trace() ("" before the first trace of the current scene)."""
        return self._lib.rtc_ctx_trace_kernel_name(self._ctx).decode()

    @property
    def trace_kernel_id(self):
        """Names the code object of the last trace(), as kernel_id does for renders."""
        return self._lib.rtc_ctx_trace_kernel_id(self._ctx).decode()

    @property
    def kernel_name(self):
        return self._lib.rtc_ctx_kernel_name(self._ctx).decode()

    @property
    def kernel_id(self):
        """Names the code object that renders the current scene (rtc_ctx_kernel_id)."""
        return self._lib.rtc_ctx_kernel_id(self._ctx).decode()

    @property
    def jit_status(self):
        """"" when the scene's kernel is what the specialisation policy asked for, else the reason (rtc_ctx_jit_status)."""
        return self._lib.rtc_ctx_jit_status(self._ctx).decode(errors="replace")

    def stats(self):
        """Synchronises with the last render and returns its counters."""
        st = L.rtc_stats()
        L.check(self._lib.rtc_ctx_stats(self._ctx, C.byref(st)))
        return {"rays": int(st.rays), "shaded_hits": int(st.shaded_hits), "pixels": int(st.pixels),
                "kernel_ms": float(st.kernel_ms), "launches": int(st.launches), "rows": int(st.rows),
                "culled_shadow_rays": int(st.culled_shadow_rays), "flags": int(st.flags)}

    def to_ppm(self, rgb, stream=None):
        """Canvas::to_ppm (canvas.rs:58-96) formatted on the device from an (h, w, 3) f32 tensor -> bytes."""
        if not (rgb.is_cuda and rgb.dtype == torch.float32 and rgb.is_contiguous() and rgb.dim() == 3):
            raise ValueError("rgb must be a contiguous float32 CUDA tensor (rows, width, 3)")
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        cap = int(self._lib.rtc_ppm_max_bytes(w, h))
        text = torch.empty(cap, dtype=torch.uint8, device=rgb.device)
        n = C.c_uint64()
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_to_ppm(self._ctx, C.c_void_p(rgb.data_ptr()), w, h, C.c_void_p(text.data_ptr()), cap,
                                       C.byref(n), C.c_void_p(s.cuda_stream)))
        return text[: n.value].cpu().numpy().tobytes()

    def quantize(self, rgb, stream=None, out=None):
        """canvas.rs:39-43 scale_color on the device: f32 tensor -> u8 tensor of the same shape."""
        if out is None:
            out = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
        if not (rgb.is_cuda and rgb.dtype == torch.float32 and rgb.is_contiguous() and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and
                out.numel() == rgb.numel()):
            raise ValueError("rgb: a contiguous float32 CUDA tensor; out: a contiguous uint8 CUDA tensor with one byte per colour value of rgb")
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        L.check(self._lib.rtc_ctx_quantize(self._ctx, C.c_void_p(rgb.data_ptr()), rgb.numel(),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)))
        return out
