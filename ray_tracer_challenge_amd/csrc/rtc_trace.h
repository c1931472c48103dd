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

// ERROR_BUDGET.md B9, per ray.  The library's own hierarchy over a flat world (rtc_scene_prep.h build_flat_bvh) turns a ray away
// from a box padded by 10 % of the object, which is safe while the ray starts within 100 of the smallest half-axis of everything
// (E2(i)) and no coordinate exceeds 2.5e3 of it (E1).  The host checks that for the camera; a stream's rays start where the caller
// says.  So the stream kernels check it for the ray they trace: a wave one of whose origins fails walks `open_trav` instead -- the
// same entry list with every box of the library's own opened (infinite bounds, infinite slack: aabb_hit holds for every finite
// ray, nothing is pruned), i.e. every object in turn, the flat list's answer.  Rays that start on the objects -- the secondary
// rays of such a lane -- would not need it and walk the open list too: correct, only slower.  A wave's choice, not a lane's: the
// walk's entry index and records are wave-uniform.  GroupShape boxes are the reference's semantics and are never opened
// (open_trav is null for every scene but a flat one with a hierarchy).
struct StreamGuard {
    const float4* open_trav;  // nullptr: nothing to guard
    float lo[3], hi[3];       // the hull of the objects' bounds, as build_flat_bvh takes it
    float r_min;              // the smallest half-axis
};
// build_flat_bvh's own condition with `p` in the camera's place, in its arithmetic; false for a NaN coordinate's comparison
DI bool within_flat_bvh_reach(const StreamGuard& G, V3 p) {
    const float lx = fminf(G.lo[0], p.x), ly = fminf(G.lo[1], p.y), lz = fminf(G.lo[2], p.z);
    const float hx = fmaxf(G.hi[0], p.x), hy = fmaxf(G.hi[1], p.y), hz = fmaxf(G.hi[2], p.z);
    const float diag2 = (hx - lx) * (hx - lx) + (hy - ly) * (hy - ly) + (hz - lz) * (hz - lz);
    const float far_coord = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
    const bool finite = p.x - p.x == 0.0f && p.y - p.y == 0.0f && p.z - p.z == 0.0f;
    return finite && sqrtf(diag2) < 100.0f * G.r_min && far_coord <= 2.5e3f * G.r_min;
}
// The scene's records as this wave walks them.  Call it where every lane that will trace is active.
DI SceneSoA guarded_soa(const StreamGuard& G, const SceneSoA& S, bool within_reach) {
    SceneSoA s = S;
    if (G.open_trav != nullptr && __any(!within_reach)) s.trav = G.open_trav;  // wave-uniform
    return s;
}

struct TraceArgs {
    SceneHdr hdr;
    SceneSoA soa;
    StreamGuard guard;
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
        const V3 origin = v3(o4.x, o4.y, o4.z);
        V3 col;
        if constexpr (NOBJ < 0) {  // (the other families walk no boxes of the library's own)
            const SceneSoA soa = guarded_soa(A.guard, A.soa, within_flat_bvh_reach(A.guard, origin));
            col = color_at<NOBJ, SIMPLE>(H, soa, origin, v3(d4.x, d4.y, d4.z), A.depth, key, cnt, stash);
        } else {
            col = color_at<NOBJ, SIMPLE>(H, A.soa, origin, v3(d4.x, d4.y, d4.z), A.depth, key, cnt, stash);
        }
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
