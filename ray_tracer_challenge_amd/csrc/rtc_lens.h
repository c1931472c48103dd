// rtc_lens.h -- a thin-lens camera (rtc_ctx_set_scene_lens): depth of field inside the supersampling kernel.
//
// A lens frame is a supersampled frame (rtc_supersample.h) whose K x K samples of an output pixel leave from K x K different
// points of a lens of radius R around the pinhole and meet again at the focal distance f: objects there are sharp, everything
// nearer or farther is blurred.  By definition (include/rtc.h spells it out ray by ray) the sample of fine pixel (x, y) is
//   * the pinhole pair o, p of primary_ray for the FINE camera,
//   * two keyed jitter draws ju, jv = jitter_value(jitter_base(seed, key, 1 / 2)), key = y * K W + x,
//   * the lens cell (ci, cj) = (y mod K, K - 1 - x mod K) -- the sub-pixel cell turned by a quarter --, the point
//     u = (ci + ju) / K, v = (cj + jv) / K of the unit square, r = R sqrtf(u), theta = 2 pi v, lx = r cosf(theta),
//     ly = r cosf(theta - pi / 2) on the lens,
//   * the origin o' = (o + right lx) + up ly along the camera's axes, the direction norm3((o + (p - o) f) - o'),
// and its colour color_at(o', d, depth, key).  Everything after that is ss_render_body's: the last fine row and column
// contribute zero, ss_reduce adds the block up in the contract's order, one lane per output pixel stores.
//
// A kernel of its own beside rtc_supersample.h, which it includes and whose device functions it calls: no existing kernel gains a
// branch, an argument or a template parameter (rtc_supersample.h says what one shared call did to ten instantiations), and no
// existing header's text -- so no existing kernel's id -- changes.  lens_render_body is ss_render_body<..., SEAM = false> with
// lens_ray between primary_ray and color_at; the one-call seam's bytes and progress words are not here.  Lanes that share a
// pixel compute the same ray from the same (x, y), as they do in ss_render_body.
// The host sets has_scene_box = 0 in a lens launch's header (the early-out's padding is argued for rays from the camera's
// origin; rtc_trace.h and rtc_adaptive.h do the same), so primary_ray's answer is constant false here.  Triangle pre-culling
// tests each ray's own origin (world_ray), whatever it is.
//
// Included by rtc_device.hip after rtc_supersample.h (ahead-of-time instantiations) and handed to hiprtc beside it and the core
// (-DRTC_SPEC_SS=K -DRTC_SPEC_LENS=1: lens_render_kernel_spec).
#ifndef RTC_LENS_H
#define RTC_LENS_H

// A scene-compiled lens kernel takes its factor from -DRTC_SPEC_SS=K, as the supersampling kernel does -- and must not compile
// that kernel's entry point a second time beside its own (rtc_supersample.h defines it wherever RTC_SPEC_SS is): the factor is
// kept as a constant, the macro is gone when the header below is read.
#if defined(RTC_SPEC_LENS) && defined(RTC_SPEC_SS)
namespace rtc {
constexpr int LENS_SPEC_K = RTC_SPEC_SS;
}
#undef RTC_SPEC_SS
#endif

#include "rtc_supersample.h"

namespace rtc {

// SsRenderArgs first: late_args<SsRenderArgs>() reads it at offset 0 of the kernel-argument segment, as ss_render_body does.
struct LensRenderArgs {
    SsRenderArgs ss;
    float aperture_radius, focal_distance;  // R >= 0, f > 0, both finite (the host has checked)
    uint32_t seed;
};

// Steps 2 - 5 of the contract: the pinhole pair (o, p) of fine pixel (x, y) -> the sample's ray.  f32, nothing fused, operands
// in the order written; sqrtf is IEEE, the cosine is glibc's cosf restated (rtc_cosf_dev).  rtc_lens_rays (rtc_host.cpp) is
// the same arithmetic on the host.
template <int K>
DI void lens_ray(const SceneHdr& H, const LensRenderArgs& A, uint32_t x, uint32_t y, uint32_t key, V3 o, V3 p, V3& origin, V3& direction) {
    const float ju = jitter_value(jitter_base(A.seed, key, 1u)), jv = jitter_value(jitter_base(A.seed, key, 2u));
    const uint32_t i = x & (uint32_t)(K - 1), j = y & (uint32_t)(K - 1);
    const uint32_t ci = j, cj = (uint32_t)(K - 1) - i;
    const float u = ((float)ci + ju) / (float)K, v = ((float)cj + jv) / (float)K;
    const float r = A.aperture_radius * sqrtf(u), theta = 6.2831855f * v;
    const float lx = r * rtc_cosf_dev(theta), ly = r * rtc_cosf_dev(theta - 1.5707964f);
    const float* c = H.cam;  // rows 0..2 of transform_inverse: its first two columns are the camera's x and y axes
    const V3 right = v3(c[0], c[4], c[8]), up = v3(c[1], c[5], c[9]);
    origin = (o + right * lx) + up * ly;
    const V3 focus = o + (p - o) * A.focal_distance;
    direction = norm3(focus - origin);
}

template <int NOBJ, bool SIMPLE, int K>
DI void lens_render_body(const LensRenderArgs& LA) {
    const RenderArgs& A = LA.ss.fine;
    const SceneHdr& H = A.hdr;
    // Where this lane's fine pixel is: regular grid (swizzled or not) or block list
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const Where w = where_is_lane<false>(A, lane, wave, 1u, 0u);
    const uint32_t sl = w.sl, x = w.x, yl = w.yl;
    const uint32_t tw_log2 = 3u - (sl >> 1), q = lane >> sl;  // the tile's width and the fine pixel's slot in it, as where_is_lane has them
    const uint32_t qx = q & ((1u << tw_log2) - 1u), qy = q >> tw_log2;
    Counters cnt = {0u, 0u, sl};
    const bool timed = Counters::SHARE_LANES && A.wave_ticks != nullptr;  // wave-uniform
    uint32_t ticks0 = 0u;
    if (timed) ticks0 = (uint32_t)wall_clock64();
    __shared__ float stash_lds[LDS_SLOTS * 256];
    const LaneStash stash = {stash_lds + threadIdx.x, 256u};
    // A lane outside the fine frame contributes zero; such lanes only ever form whole K x K blocks (ss_render_body).
    V3 col = v3(0.0f, 0.0f, 0.0f);
    if (x < H.width && yl < A.rows) {
        // compact local row -> global row of the fine image: image_row's expression, written out as ss_render_body writes it
        const uint32_t band = yl / A.band_rows;
        const uint32_t y = (band * A.n_parts + A.part) * A.band_rows + (yl - band * A.band_rows);
        // camera.rs:80-81 at the fine resolution: the fine frame's last row and column stay black, so the output's are dimmed
        if (x < H.width - 1u && y < H.height - 1u) {
            V3 o, p, origin, direction;
            (void)primary_ray(H, x, y, o, p);  // (has_scene_box is 0 in this launch's header: the answer is false)
            const uint32_t key = y * H.width + x;  // the fine pixel index: the lens's jitter key and the area light's
            lens_ray<K>(H, LA, x, y, key, o, p, origin, direction);
            col = color_at<NOBJ, SIMPLE>(H, A.soa, origin, direction, A.depth, key, cnt, stash);
        }
    }
    // The reduction, after the divergent region: every lane of the wave takes part (ss_render_body).
    col.x = ss_reduce<K>(col.x, sl, tw_log2);
    col.y = ss_reduce<K>(col.y, sl, tw_log2);
    col.z = ss_reduce<K>(col.z, sl, tw_log2);
    // One lane per output pixel stores: the block's first slot, the lead lane of a pixel's lanes.
    // (short form, RTC_WAVE_FIXED_SHORT: the arguments as late_args hands them out; earlier form: the arguments as they are)
#if RTC_WAVE_FIXED_SHORT
    const SsRenderArgs& LS = late_args<SsRenderArgs>();
#else
    const SsRenderArgs& LS = LA.ss;
#endif
    const RenderArgs& L = LS.fine;
    if (cnt.lead() && (qx & (uint32_t)(K - 1)) == 0u && (qy & (uint32_t)(K - 1)) == 0u) {
        const uint32_t ox = x / (uint32_t)K, oy = yl / (uint32_t)K;
        if (ox < LS.out_width && oy < LS.out_rows) {
            float* dst = L.out + ((size_t)oy * LS.out_width + ox) * 3;
            dst[0] = col.x;
            dst[1] = col.y;
            dst[2] = col.z;
        }
    }
    store_wave_counts(L, cnt, timed, ticks0);
}

#ifdef RTC_SPEC_LIST
#ifdef RTC_SPEC_LENS
}  // namespace rtc
// The lens kernel of a scene-specialised (hiprtc) build.
// (A is the kernel's first and only argument: lens_render_body's late_args reads it at offset 0 of the kernel-argument segment)
extern "C" __global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void lens_render_kernel_spec(rtc::LensRenderArgs A) {
    rtc::lens_render_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0, rtc::LENS_SPEC_K>(A);
}
namespace rtc {
#endif
#else
template <int NOBJ, bool SIMPLE, int K>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void lens_render_kernel(LensRenderArgs A) {
    lens_render_body<NOBJ, SIMPLE, K>(A);
}
#endif

}  // namespace rtc
#endif  // RTC_LENS_H
