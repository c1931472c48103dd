// rtc_trace.h -- ray streams (rtc_ctx_trace, rtc_ctx_camera_rays): World::color_at (world.rs:88-101) for rays the CALLER
// brings, against the context's resident scene, on the device.
//
// The render kernels make their rays from the reference's pinhole camera (primary_ray); everything after that -- color_at
// and all it calls, with every shortcut the host switches on in the SceneHdr -- does not know where a ray came from.  Here the
// rays are read from memory instead: one lane per ray, ray i in thread i of a 1-D grid, so a wave is 64 consecutive rays --
// whichever 64 the caller put side by side.  A lane loads 16 bytes of origin, 16 of direction (a wave: two contiguous runs of
// 1 KiB) and its jitter key -- the pixel index whose light samples the ray draws, or i -- calls color_at and stores three
// dwords at render_body's 12-byte stride.
//
// Included by rtc_device.hip after rtc_kernel_core.h (ahead-of-time instantiations) and handed to hiprtc beside it
// (-DRTC_SPEC_TRACE=1: trace_kernel_spec), as rtc_supersample.h is.  Not here, because a ray stream has no frame: block
// lists, scene tiles and rectangles, the swizzle, several blocks per workgroup, progress words, the u8 canvas, lanes sharing
// a ray (the host switches lane sharing off in a scene's ray-stream kernel), and the scene-box early-out of primary_ray, whose
// padding is argued from the camera's distance to the scene.
#ifndef RTC_TRACE_H
#define RTC_TRACE_H

#include "rtc_kernel_core.h"

namespace rtc {

struct TraceArgs {
    SceneHdr hdr;
    SceneSoA soa;
    const float4* origins;     // [n] x, y, z read; w ignored
    const float4* directions;  // [n] likewise; used as given (world.rs:88 does not normalise either)
    const uint32_t* keys;      // [n] jitter keys, or nullptr: ray i draws as pixel i (wave-uniform: a kernel argument)
    float* out;                // [n][3]
    uint4* wave_counts;        // one partial {rays, shaded hits, culled shadow rays, 0} per wave: [4 * gridDim.x]
    unsigned long long* total; // zeroed here, accumulated by sum_counts_kernel
    uint32_t n;
    int32_t depth;
};

// store_wave_counts for a 1-D grid: one partial per wave, no workgroup barrier (a finished wave leaves).
DI void store_trace_counts(const TraceArgs& A, const Counters& cnt) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint4 counts = reduce_wave_counts(cnt);
    if (blockIdx.x == 0 && threadIdx.x < 3) A.total[threadIdx.x] = 0ull;  // for sum_counts_kernel's atomics
    if (lane == COUNTS_LANE) A.wave_counts[(size_t)blockIdx.x * 4u + wave] = counts;
}

template <int NOBJ, bool SIMPLE>
DI void trace_body(const TraceArgs& A) {
    const SceneHdr& H = A.hdr;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (the host launches ceil(n / 256) workgroups: no wrap below 2^32 rays)
    Counters cnt = {0u, 0u, 0u};  // one lane per ray (sl = 0, should a kernel ever be compiled for lane sharing)
    __shared__ float stash_lds[LDS_SLOTS * 256];
    const LaneStash stash = {stash_lds + threadIdx.x, 256u};
    // (what stands in front of color_at is kept to three plain loads: render_body's comments say why)
    if (i < A.n) {
        const float4 o4 = A.origins[i], d4 = A.directions[i];
        const uint32_t key = A.keys != nullptr ? A.keys[i] : i;
        const V3 col = color_at<NOBJ, SIMPLE>(H, A.soa, v3(o4.x, o4.y, o4.z), v3(d4.x, d4.y, d4.z), A.depth, key, cnt, stash);
        float* dst = A.out + (size_t)i * 3;
        dst[0] = col.x;
        dst[1] = col.y;
        dst[2] = col.z;
    }
    // after the divergent region: lanes past n have traced nothing and take part in the reduce
    store_trace_counts(A, cnt);
}

#ifdef RTC_SPEC_LIST
#ifdef RTC_SPEC_TRACE
}  // namespace rtc
// The ray-stream kernel of a scene-specialised (hiprtc) build.
extern "C" __global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void trace_kernel_spec(rtc::TraceArgs A) {
    rtc::trace_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0>(A);
}
namespace rtc {
#endif
#else
template <int NOBJ, bool SIMPLE>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void trace_kernel(TraceArgs A) {
    trace_body<NOBJ, SIMPLE>(A);
}

// rtc_ctx_camera_rays: ray_for_pixel (camera.rs:60-74) for rows [y0, y0 + n_rows) of a camera, in image order, in
// trace_body's layout.  The ray is the core's primary_ray and norm3 -- what render_body traces, by construction.  `hdr`
// carries the camera's fields only (has_scene_box = 0: primary_ray's answer is not asked for).
struct CameraRaysArgs {
    SceneHdr hdr;
    float4* origins;     // any of the three may be nullptr (wave-uniform)
    float4* directions;
    uint32_t* keys;
    uint32_t y0, n_rows;
};
__global__ __launch_bounds__(256) void camera_rays_kernel(CameraRaysArgs A) {
    const SceneHdr& H = A.hdr;
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;  // (the host refuses n_rows * width >= 2^32)
    if ((unsigned long long)j >= (unsigned long long)A.n_rows * H.width) return;
    const uint32_t row = j / H.width, x = j - row * H.width, y = A.y0 + row;
    V3 origin, pixel;
    (void)primary_ray(H, x, y, origin, pixel);
    const V3 direction = norm3(pixel - origin);
    if (A.origins) A.origins[j] = make_float4(origin.x, origin.y, origin.z, 1.0f);
    if (A.directions) A.directions[j] = make_float4(direction.x, direction.y, direction.z, 0.0f);
    if (A.keys) A.keys[j] = y * H.width + x;
}
#endif

}  // namespace rtc
#endif  // RTC_TRACE_H
