// rtc_hits.h -- first-hit buffers (rtc_hit_at, rtc_ctx_render_hits): what the render path knows about a ray's first hit
// before it turns it into a colour, one plane per field of PrecomputedValues (world.rs:165-182) plus the light fraction.
//
// "First hit" is, in this order: xs = World::intersect(ray) (world.rs:52-60); hit = Intersection::hit(xs)
// (intersection.rs:30-35); comps = precompute_values(ray, hit, xs) (world.rs:212-283) for EVERY hit, opaque or not; and
// light = world.light.intensity_at(comps.over_point, world) (world.rs:75) with the jitter key (pixel index, path 1) -- the
// key color_at gives a pixel's primary hit.
//
// Ahead-of-time only, included by rtc_device.hip after rtc_kernel_core.h.  A pixel's ray is the core's (image_row,
// primary_ray: what render_body calls); first_hit below is either one of the core's device functions or restates a line of
// color_at (rtc_kernel_core.h) with the same operations in the same order, so the planes hold the bits the render used.
#ifndef RTC_HITS_H
#define RTC_HITS_H

#include "rtc_kernel_core.h"
#include "rtc_trace.h"

namespace rtc {

// Device view of rtc_hit_planes (include/rtc.h).  nullptr: not wanted -- wave-uniform, a kernel argument.
struct HitPlanes {
    int32_t* object;
    float* distance;
    float4* point;
    float4* eye;
    float4* normal;
    float4* reflectv;
    float4* over_point;
    float4* under_point;
    int32_t* inside;
    float2* n1n2;
    float* light;
};

// One dword store per lane for a scalar plane, one 16-byte store per lane for a vector plane.
DI void store_miss(const HitPlanes& P, size_t i) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (P.object) P.object[i] = -1;
    if (P.distance) P.distance[i] = 0.0f;
    if (P.point) P.point[i] = z;
    if (P.eye) P.eye[i] = z;
    if (P.normal) P.normal[i] = z;
    if (P.reflectv) P.reflectv[i] = z;
    if (P.over_point) P.over_point[i] = z;
    if (P.under_point) P.under_point[i] = z;
    if (P.inside) P.inside[i] = 0;
    if (P.n1n2) P.n1n2[i] = make_float2(0.0f, 0.0f);
    if (P.light) P.light[i] = 0.0f;
}

// The first hit of ray (o, d) into element i of the planes.  NOBJ / SIMPLE: the render kernels' families (for_each_object);
// LIGHT: a template flag, so that a geometry-only pass does not carry the sampling loop's registers.
template <int NOBJ, bool SIMPLE, bool LIGHT>
DI void first_hit(const SceneHdr& H, const SceneSoA& S, V3 o, V3 d, uint32_t pixel, const HitPlanes& P, size_t i) {
    Counters cnt = {0u, 0u, 0u, 0u};
    const bool want_n12 = P.n1n2 != nullptr;  // wave-uniform
    Hit h;
    float kt1 = 0.0f, kt2 = 0.0f;  // tree worlds: the ray's containers from the same walk, as color_at takes them
    int kc1 = -1, kc2 = -1;
    bool k_inside = false;
    if constexpr (NOBJ < 0) {
        if (want_n12) h = nearest_hit_and_containers<NOBJ>(H, S, o, d, cnt, kt1, kc1, kt2, kc2, k_inside);
        else h = nearest_hit<NOBJ, true>(H, S, o, d, cnt);
    } else {
        h = nearest_hit<NOBJ, true>(H, S, o, d, cnt);
    }
    if (h.obj < 0) {
        store_miss(P, i);
        return;
    }
    // precompute_values, world.rs:212-233 (color_at's expressions)
    const int ob = h.obj;
    const Obj rec = load_obj(S, ob);
    const V3 point = o + d * h.t;
    const V3 op = obj_point(rec, point);
    const V3 n0 = obj_normal_to_world(rec, local_normal(rec.bits & SHAPE_KIND_MASK, rec.min_y(), rec.max_y(), S.tri + 3 * ob, op));
    const bool inside = dot3(n0, -d) < 0.0f;
    const V3 n = inside ? -n0 : n0;
    const V3 over_point = point + n * SELF_EPS;
    const V3 under_point = point - n * SELF_EPS;
    const V3 eye = -d;
    const V3 reflectv = reflect3(d, n0);  // world.rs:220: from the normal before the inside flip
    // The reference's Tuples carry w: 1 for points, 0 for vectors -- except that normal_at (shape.rs:72-154) sets the
    // normal's w to 0 BEFORE it normalises, so a normal of magnitude 0 or NaN (the apex of a cone) has w = 0 / m = NaN
    // like its other three components, and what is derived from the normal inherits it.
    const float nw = (n.x != n.x && n.y != n.y && n.z != n.z) ? RTC_NAN : 0.0f;
    const float pw = 1.0f + nw;  // over_point.w = 1 + n.w * eps, under_point.w = 1 - n.w * eps
    if (P.object) P.object[i] = ob;
    if (P.distance) P.distance[i] = h.t;
    if (P.point) P.point[i] = make_float4(point.x, point.y, point.z, 1.0f);
    if (P.eye) P.eye[i] = make_float4(eye.x, eye.y, eye.z, 0.0f);
    if (P.normal) P.normal[i] = make_float4(n.x, n.y, n.z, nw);
    if (P.reflectv) P.reflectv[i] = make_float4(reflectv.x, reflectv.y, reflectv.z, nw);
    if (P.over_point) P.over_point[i] = make_float4(over_point.x, over_point.y, over_point.z, pw);
    if (P.under_point) P.under_point[i] = make_float4(under_point.x, under_point.y, under_point.z, pw);
    if (P.inside) P.inside[i] = inside ? 1 : 0;
    if (want_n12) {  // world.rs:234-263, for every hit: the reference does not look at the material first
        float n1, n2;
        if constexpr (NOBJ < 0) {  // (what refraction_indices derives from the same containers)
            const float own = S.mat_c[ob].y;
            n1 = kc1 >= 0 ? S.mat_c[kc1].y : 1.0f;  // REFRACTION_VACCUM, constants.rs:6
            n2 = !k_inside ? own : kc1 == ob ? (kc2 >= 0 ? S.mat_c[kc2].y : 1.0f) : n1;
        } else {
            refraction_indices<NOBJ>(H, S, o, d, ob, n1, n2, cnt);
        }
        P.n1n2[i] = make_float2(n1, n2);
    }
    if constexpr (LIGHT) {
        if (P.light) P.light[i] = intensity_at<NOBJ, SIMPLE>(H, S, over_point, pixel, 1u, cnt);  // world.rs:75
    }
}

// rtc_hit_at: one lane per caller ray, the generic loops -- as color_at_kernel.  Ray i uses pixel index i as its jitter key.
__global__ void hit_at_kernel(SceneHdr H, SceneSoA S, const float4* __restrict__ origins, const float4* __restrict__ directions, uint32_t n,
                              HitPlanes P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 o4 = origins[i], d4 = directions[i];
    const V3 o = v3(o4.x, o4.y, o4.z), d = v3(d4.x, d4.y, d4.z);
    if (H.n_trav) first_hit<-1, false, true>(H, S, o, d, i, P, i);
    else first_hit<0, false, true>(H, S, o, d, i, P, i);
}

struct HitsArgs {
    SceneHdr hdr;
    SceneSoA soa;
    HitPlanes planes;  // compact rows of this partition: element (yl, x) at index yl * width + x
    uint32_t rows;     // rows in the planes
    uint32_t band_rows, n_parts, part;
    // A wave's tile is 2^tile_w_log2 pixels wide and 64 >> tile_w_log2 high (8 x 8, 32 x 2 or 64 x 1); a workgroup's four waves
    // sit 2 x 2 for the square tile and one below the other for the wide ones.  Changes which lane has which pixel: time only.
    uint32_t tile_w_log2;
};

// Waves per SIMD the kernels with the light plane are compiled for.  Measured on C3 4096^2 / C1 1000 x 400, planes = (light),
// hits_kernel<4, simple, light> (profiles/hits_times.txt): left to the compiler (131 VGPRs, 3 waves) 1018 / 134 us; 6 waves as the
// render kernels (80 VGPRs, 244 B of spills per lane) 1018 / 184 us; 4 waves (128 VGPRs, no spill) 830 / 140 us.  Unlike
// color_at, nothing but the hit's few values is live across the sampling loop here, so the loop fits 128 registers whole.
// (The geometry-only kernels need under 40 registers: whatever the compiler takes.)
#ifndef RTC_HITS_LIGHT_WAVES
#define RTC_HITS_LIGHT_WAVES 4
#endif
// rtc_ctx_render_hits: one lane per pixel, render_body's primary ray (image_row, primary_ray).
template <int NOBJ, bool SIMPLE, bool LIGHT>
__global__ __launch_bounds__(256, LIGHT ? RTC_HITS_LIGHT_WAVES : 1) void hits_kernel(HitsArgs A) {
    const SceneHdr& H = A.hdr;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t twl = A.tile_w_log2, thl = 6u - twl;
    const bool square = twl == 3u;
    const uint32_t bx0 = blockIdx.x << (square ? 4u : twl), by0 = blockIdx.y << (square ? 4u : thl + 2u);
    const uint32_t x = bx0 + (square ? (wave & 1u) << 3 : 0u) + (lane & ((1u << twl) - 1u));
    const uint32_t yl = by0 + ((square ? wave >> 1 : wave) << thl) + (lane >> twl);
    if (!(x < H.width && yl < A.rows)) return;
    const size_t idx = (size_t)yl * H.width + x;
    const uint32_t y = image_row(yl, A.band_rows, A.n_parts, A.part);
    // camera.rs:80-81: `0..height-1` x `0..width-1` -- the last row and column are never traced: misses
    if (!(x < H.width - 1u && y < H.height - 1u)) {
        store_miss(A.planes, idx);
        return;
    }
    V3 origin, pixel;
    if (primary_ray(H, x, y, origin, pixel)) {  // misses the padded box around everything: hits nothing
        store_miss(A.planes, idx);
        return;
    }
    V3 direction = norm3(pixel - origin);
    first_hit<NOBJ, SIMPLE, LIGHT>(H, A.soa, origin, direction, y * H.width + x, A.planes, idx);
}

// ---- ray streams: first hits and occlusion for rays the caller brings (rtc_ctx_trace_hits, rtc_ctx_is_shadowed) ----------
// What rtc_trace.h is to render_body these are to hits_kernel and is_shadowed_kernel: the rays are read from memory instead
// of made from the camera, one lane per ray, ray i in thread i of a 1-D grid, so a wave is whichever 64 rays the caller put
// side by side.  Everything behind the loads is first_hit / is_shadowed as the resident scene's SceneHdr switches them.
// Not here, because a stream has no frame: tiles, the scene-box early-out of primary_ray, block lists, lane sharing.
// `guard` (rtc_trace.h StreamGuard): ERROR_BUDGET.md B9 for rays that start where the caller says.
struct TraceHitsArgs {
    SceneHdr hdr;
    SceneSoA soa;
    StreamGuard guard;
    const float4* origins;     // [n] x, y, z read; w ignored (as trace_body)
    const float4* directions;  // [n] likewise; used as given
    const uint32_t* keys;      // [n] jitter keys, or nullptr: ray i draws as pixel i (wave-uniform: a kernel argument)
    HitPlanes planes;          // element i: ray i
    uint32_t n;
};

// rtc_ctx_trace_hits.  hits_kernel's launch bounds: behind the loads the two kernels are the same code.
template <int NOBJ, bool SIMPLE, bool LIGHT>
__global__ __launch_bounds__(256, LIGHT ? RTC_HITS_LIGHT_WAVES : 1) void trace_hits_kernel(TraceHitsArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (the host launches ceil(n / 256) workgroups: no wrap below 2^32 rays)
    if (i >= A.n) return;
    const float4 o4 = A.origins[i], d4 = A.directions[i];
    const uint32_t key = A.keys != nullptr ? A.keys[i] : i;
    const V3 origin = v3(o4.x, o4.y, o4.z);
    if constexpr (NOBJ < 0) {
        const SceneSoA soa = guarded_soa(A.guard, A.soa, within_flat_bvh_reach(A.guard, origin));
        first_hit<NOBJ, SIMPLE, LIGHT>(A.hdr, soa, origin, v3(d4.x, d4.y, d4.z), key, A.planes, i);
    } else {
        first_hit<NOBJ, SIMPLE, LIGHT>(A.hdr, A.soa, origin, v3(d4.x, d4.y, d4.z), key, A.planes, i);
    }
}

struct ShadowedArgs {
    SceneHdr hdr;
    SceneSoA soa;
    StreamGuard guard;              // for both ends of a pair: either may be anywhere
    const float4* light_positions;  // [n] x, y, z read
    const float4* points;           // [n] likewise
    int32_t* out;                   // [n] 0 / 1
    uint32_t n;
};

// rtc_ctx_is_shadowed: World::is_shadowed (world.rs:104-119) pair by pair, with the object loop of the scene's family.
template <int NOBJ>
__global__ __launch_bounds__(256) void shadowed_kernel(ShadowedArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const float4 l = A.light_positions[i], p = A.points[i];
    Counters cnt = {0u, 0u, 0u, 0u};
    const V3 light = v3(l.x, l.y, l.z), point = v3(p.x, p.y, p.z);
    if constexpr (NOBJ < 0) {
        const SceneSoA soa = guarded_soa(A.guard, A.soa, within_flat_bvh_reach(A.guard, light) && within_flat_bvh_reach(A.guard, point));
        A.out[i] = is_shadowed<NOBJ>(A.hdr, soa, light, point, cnt) ? 1 : 0;
    } else {
        A.out[i] = is_shadowed<NOBJ>(A.hdr, A.soa, light, point, cnt) ? 1 : 0;
    }
}

}  // namespace rtc
#endif  // RTC_HITS_H
