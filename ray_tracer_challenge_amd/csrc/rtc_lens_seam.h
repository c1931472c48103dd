// rtc_lens_seam.h -- the lens kernel of the one-call seam (rtc_render_lens): lens_render_body with what the seam asks of the one
// lane per output pixel that stores after the reduce.
//
// It stands to rtc_lens.h as ss_render_body<..., SEAM = true> stands to ss_render_body<..., SEAM = false>: the same lane
// placement (where_is_lane), the same pinhole pair (primary_ray), the same lens ray (lens_ray<K>), the same keys -- the fine pixel
// index y * K W + x is the lens's jitter key and the area light's --, the same black last fine row and column, the same reduce
// (ss_reduce<K>).  Added, all of it after the reduce but one barrier:
//   * RenderArgs::out_u8: three bytes, scale_color of the reduced colour, in ss_render_body's arithmetic;
//   * write-through (system scope) stores when the launch reports its rows (RenderArgs::progress);
//   * the progress tail: waves_done in LDS -- one barrier in front of all work, and only when reporting --, fence and s_waitcnt,
//     the block row's counter, the chunk's counter, done[ch] = epoch.  gridDim.y counts FINE block rows, a chunk is
//     chunk_block_rows of them; the host turns them into output rows (rtc_launch_plan.h chunk_output_rows).
// A COMPILE-TIME variant, and a header of its own beside rtc_lens.h, which it includes and whose device functions it calls: the
// persistent context's lens kernels (lens_render_kernel<...>, -DRTC_SPEC_LENS=1 alone) keep their text, so their ids, and their
// code -- rtc_supersample.h's head says what the seam's paths did to the register allocation of the supersampling kernels when they
// were run-time branches of one body (profiles/lens_seam_codegen.txt: the persistent lens kernels' figures at both commits).
// Within the variant, u8 and reporting are wave-uniform run-time branches on kernel arguments, as in ss_render_body.  The tail is
// written out a third time, not shared, for the reason rtc_supersample.h gives: a function of the core would change every plain
// kernel's id.  No workgroup barrier after color_at: a finished wave must be able to leave (store_wave_counts says why).
//
// Included by rtc_device.hip after rtc_lens.h (ahead-of-time instantiations: lens_seam_render_kernel<NOBJ, SIMPLE, K>) and handed
// to hiprtc beside it, rtc_supersample.h and the core (-DRTC_SPEC_SS=K -DRTC_SPEC_LENS=1 -DRTC_SPEC_LENS_SEAM=1: the entry point
// is lens_render_kernel_spec, as the persistent context's is -- the variant is an option of the compile).
#ifndef RTC_LENS_SEAM_H
#define RTC_LENS_SEAM_H

// A scene-compiled seam kernel defines lens_render_kernel_spec itself: rtc_lens.h must not define it a second time (nor
// rtc_supersample.h its own entry point), so the factor is kept as a constant and both macros are gone when the headers below are
// read -- rtc_lens.h does the same to rtc_supersample.h.
#if defined(RTC_SPEC_LENS_SEAM) && defined(RTC_SPEC_LENS) && defined(RTC_SPEC_SS)
namespace rtc {
constexpr int LENS_SEAM_SPEC_K = RTC_SPEC_SS;
}
#undef RTC_SPEC_SS
#undef RTC_SPEC_LENS
#endif

#include "rtc_lens.h"

namespace rtc {

template <int NOBJ, bool SIMPLE, int K>
DI void lens_seam_render_body(const LensRenderArgs& LA) {
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
    // progress reporting: how many of this workgroup's waves have stored their pixels
    __shared__ uint32_t waves_done_lds;
    uint32_t* const waves_done = &waves_done_lds;
    if (A.progress != nullptr) {  // wave-uniform (a kernel argument); the one barrier, in front of all work
        if (threadIdx.x == 0) waves_done_lds = 0u;
        __syncthreads();
    }
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
    // The reduction, after the divergent region: every lane of the wave takes part (ss_render_body).  No LDS round trip and no
    // workgroup barrier -- a finished wave must be able to leave.
    col.x = ss_reduce<K>(col.x, sl, tw_log2);
    col.y = ss_reduce<K>(col.y, sl, tw_log2);
    col.z = ss_reduce<K>(col.z, sl, tw_log2);
    // One lane per output pixel stores: the block's first slot, the lead lane of a pixel's lanes.  Three dword stores -- or three
    // bytes, scale_color of the reduced colour (render_body's arithmetic) --, write-through (system scope) when the launch reports.
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
            const bool through = L.progress != nullptr;  // wave-uniform
            const size_t at = ((size_t)oy * LS.out_width + ox) * 3;
            if (L.out_u8 != nullptr) {  // wave-uniform
                uint8_t* dst = L.out_u8 + at;
                const uint8_t r = (uint8_t)fmaxf(fminf(col.x * 255.0f, 255.0f), 0.0f), g = (uint8_t)fmaxf(fminf(col.y * 255.0f, 255.0f), 0.0f),
                              b = (uint8_t)fmaxf(fminf(col.z * 255.0f, 255.0f), 0.0f);
                if (through) {
                    __hip_atomic_store(dst, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dst + 1, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dst + 2, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    dst[0] = r, dst[1] = g, dst[2] = b;
                }
            } else {
                float* dst = L.out + at;
                if (through) {
                    __hip_atomic_store(dst, col.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dst + 1, col.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dst + 2, col.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    dst[0] = col.x;
                    dst[1] = col.y;
                    dst[2] = col.z;
                }
            }
        }
    }
    store_wave_counts(L, cnt, timed, ticks0);
    // ss_render_body's progress tail (see RenderArgs::progress): the wave's stores are acknowledged -- write-through: in memory --
    // before it counts itself done; the workgroup's last wave (the fourth of 256 threads) counts the block row, the row's last
    // workgroup the chunk, the chunk's last row writes the host's word.
    if (L.progress != nullptr) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        uint32_t last = 0u;
        if (lane == 0) last = __hip_atomic_fetch_add(waves_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 3u ? 1u : 0u;
        if (__builtin_amdgcn_readfirstlane((int)last) != 0 && lane == 0) {
            const uint32_t row = blockIdx.y;
            if (__hip_atomic_fetch_add(&L.progress[row * PROGRESS_STRIDE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == gridDim.x) {
                const uint32_t ch = row / L.chunk_block_rows;
                const uint32_t in_chunk = min(L.chunk_block_rows, gridDim.y - ch * L.chunk_block_rows);
                if (__hip_atomic_fetch_add(&L.progress[(gridDim.y + ch) * PROGRESS_STRIDE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == in_chunk)
                    __hip_atomic_store(&L.done[ch], L.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

#ifdef RTC_SPEC_LIST
#ifdef RTC_SPEC_LENS_SEAM
}  // namespace rtc
// The seam's lens kernel of a scene-specialised (hiprtc) build.
// (A is the kernel's first and only argument: the body's late_args reads it at offset 0 of the kernel-argument segment)
extern "C" __global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void lens_render_kernel_spec(rtc::LensRenderArgs A) {
    rtc::lens_seam_render_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0, rtc::LENS_SEAM_SPEC_K>(A);
}
namespace rtc {
#endif
#else
template <int NOBJ, bool SIMPLE, int K>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void lens_seam_render_kernel(LensRenderArgs A) {
    lens_seam_render_body<NOBJ, SIMPLE, K>(A);
}
#endif

}  // namespace rtc
#endif  // RTC_LENS_SEAM_H
