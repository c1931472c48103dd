// rtc_supersample.h -- supersampled rendering (rtc_ctx_set_scene_ss): K x K rays per output pixel, reduced in the kernel.
//
// By definition the supersampled frame is a fixed-order f32 box filter of the frame the render path produces for the FINE
// camera (Camera::new(K W, K H, fov, transform), camera.rs:23-56): output pixel (X, Y) is a pairwise tree over its K x K block
// of that frame, along x first, then along y, times 1 / K^2 -- see include/rtc.h.  The K x K samples of an output pixel sit
// in neighbouring lanes of one wave's tile, so the fine frame never exists in memory: every lane traces its fine pixel as
// render_body does, an xor-butterfly across the lanes adds the block up (IEEE addition is commutative: every lane of the
// block ends with the same bits), and one lane per output pixel stores.
//
// Included by rtc_device.hip after rtc_kernel_core.h (ahead-of-time instantiations) and handed to hiprtc beside it
// (-DRTC_SPEC_SS=K: ss_render_kernel_spec).  Everything up to the reduce is the core's own device functions, the ones
// render_body calls: where_is_lane (never a scene rectangle launch, one block per workgroup), primary_ray, color_at,
// store_wave_counts -- all but image_row, whose two lines are written out below.  Not supported, because the host never
// asks a supersampled launch for them: scene rectangle launches and their zero-filling workgroups, several blocks per
// workgroup.
// The one-call seam (rtc_render_ss) asks for what it asks of render_body, of the one lane per output pixel that stores after the
// reduce: the u8 canvas (RenderArgs::out_u8: [out_rows][out_width][3] bytes) and progress words (RenderArgs::progress, regular
// grid only: gridDim.y counts FINE block rows, a chunk is chunk_block_rows of them, the host turns them into output rows).
// render_body's write-through stores and its progress tail are repeated here, not shared: a scene's plain render kernel is
// identified by the TEXT of rtc_kernel_core.h (JitKind::RENDER hashes the core alone), so moving them into a function of the
// core would change every plain kernel's id -- the ones profiles/*_pmc.json and bench.py match -- for no change in code.
// Both are a COMPILE-TIME variant (SEAM; ss_seam_render_kernel<...>, -DRTC_SPEC_SS_SEAM=1), launched by the seam's contexts alone:
// as wave-uniform run-time branches on the kernel's arguments -- render_body's way -- they moved the register allocation of the
// kernels the persistent context launches (four of the twelve ahead-of-time instantiations spilled 18 to 40 VGPRs more, DESIGN.md
// 8b).  With SEAM = false this body compiles to what it was.  Within the variant, u8 and reporting are run-time, wave-uniform.
#ifndef RTC_SUPERSAMPLE_H
#define RTC_SUPERSAMPLE_H

#include "rtc_kernel_core.h"

namespace rtc {

// The fine frame's RenderArgs -- its SceneHdr is the fine camera's, rows / band_rows count fine rows, tiles / share_log2 /
// swizzle / wave_ticks / block_counts are what render_body takes -- except that `out` is the OUTPUT canvas:
// [out_rows][out_width][3] f32, out_width = hdr.width / K, out_rows = rows / K.
struct SsRenderArgs {
    RenderArgs fine;
    uint32_t out_width, out_rows;
};

// How a lane reads another lane's value.  With lanes-per-pixel a run-time value (the lane-sharing kernels) the masks are run-time
// shifts: __shfl_xor (ds_bpermute_b32) takes any mask.
DI float ss_xor_lane(float v, uint32_t mask) { return __shfl_xor(v, (int)mask, 64); }
// With one lane per pixel the masks are 1, 2, 8 and 16: the first three are DPP controls, folded into the v_add_f32 itself --
// quad_perm:[1,0,3,2], quad_perm:[2,3,0,1], row_ror:8 (a rotation by 8 within a row of 16 lanes is the xor) -- and the fourth,
// which crosses rows of 16, is ds_swizzle_b32 in bit mode (and 0x1f, or 0, xor 0x10).  Measured against ds_bpermute:
// profiles/supersample_xlane_ab.txt.
template <int CTRL>
DI float ss_dpp(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
DI float ss_swizzle_xor16(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401f)); }

// One channel of the K x K block this lane's fine pixel belongs to, in the contract's order: pixel slots q ^ 1 (and q ^ 2)
// along x, then q ^ tile width (and twice it) along y, each shifted by the wave's lanes-per-pixel.  Every lane of the wave
// takes part; the K^2 lanes of a block (times 2^sl: a pixel's lanes hold the same bits) all end with the block's value.
template <int K>
DI float ss_reduce(float v, uint32_t sl, uint32_t tw_log2) {
    static_assert(K == 2 || K == 4, "supersampling factor");
    if (!Counters::SHARE_LANES) {  // sl = 0, an 8 x 8 tile: slots are lanes, the steps are lanes ^ 1, 2, 8, 16
        v = v + ss_dpp<0xB1>(v);
        if constexpr (K == 4) v = v + ss_dpp<0x4E>(v);
        v = v + ss_dpp<0x128>(v);
        if constexpr (K == 4) v = v + ss_swizzle_xor16(v);
        return v * (1.0f / (float)(K * K));
    }
    const uint32_t sx = 1u << sl, sy = 1u << (sl + tw_log2);
    v = v + ss_xor_lane(v, sx);
    if constexpr (K == 4) v = v + ss_xor_lane(v, 2u * sx);
    v = v + ss_xor_lane(v, sy);
    if constexpr (K == 4) v = v + ss_xor_lane(v, 2u * sy);
    return v * (1.0f / (float)(K * K));  // 0.25f / 0.0625f: exact constants
}

template <int NOBJ, bool SIMPLE, int K, bool SEAM>
DI void ss_render_body(const SsRenderArgs& SA) {
    const RenderArgs& A = SA.fine;
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
    [[maybe_unused]] uint32_t* waves_done = nullptr;  // progress reporting: how many of this workgroup's waves have stored their pixels
    if constexpr (SEAM) {
        __shared__ uint32_t waves_done_lds;
        waves_done = &waves_done_lds;
        if (A.progress != nullptr) {  // wave-uniform (a kernel argument); the one barrier, in front of all work
            if (threadIdx.x == 0) waves_done_lds = 0u;
            __syncthreads();
        }
    }
    // A lane outside the fine frame contributes zero.  Such lanes only ever form whole K x K blocks: the fine width, the fine
    // rows of a partition and every band are multiples of K, and so is every tile's origin.
    V3 col = v3(0.0f, 0.0f, 0.0f);
    if (x < H.width && yl < A.rows) {
        // compact local row -> global row of the fine image: image_row's expression, written out.  The one shared call that is not
        // neutral here: with image_row called, ten of the twelve ahead-of-time instantiations of this body spill differently (4 - 8 B
        // of scratch per lane either way) and <4, simple, 4> runs 6 % slower; written out, all twelve have the figures they had
        // before (LABNOTES.md, "one definition of the primary ray").
        const uint32_t band = yl / A.band_rows;
        const uint32_t y = (band * A.n_parts + A.part) * A.band_rows + (yl - band * A.band_rows);
        // camera.rs:80-81 at the fine resolution: the fine frame's last row and column stay black, so the output's are dimmed
        if (x < H.width - 1u && y < H.height - 1u) {
            V3 origin, pixel;
            const bool sees_nothing = primary_ray(H, x, y, origin, pixel);
            if (sees_nothing) {
                cnt.rays += cnt.lead();
            } else {
                V3 direction = norm3(pixel - origin);
                col = color_at<NOBJ, SIMPLE>(H, A.soa, origin, direction, A.depth, y * H.width + x, cnt, stash);  // jitter key: the FINE pixel index
            }
        }
    }
    // The reduction, after the divergent region: every lane of the wave takes part.  No LDS round trip and no workgroup
    // barrier -- a finished wave must be able to leave (store_wave_counts says why).
    col.x = ss_reduce<K>(col.x, sl, tw_log2);
    col.y = ss_reduce<K>(col.y, sl, tw_log2);
    col.z = ss_reduce<K>(col.z, sl, tw_log2);
    // One lane per output pixel stores: the block's first slot, the lead lane of a pixel's lanes.  Three dword stores, 1 / K^2 of
    // the fine frame's -- or three bytes, scale_color of the reduced colour (render_body's arithmetic), and write-through
    // (system scope) when the launch reports its rows (RenderArgs::progress).
    // (short form, RTC_WAVE_FIXED_SHORT: the arguments as late_args hands them out -- what the stores and the counters need is loaded here,
    // behind color_at; earlier form: the arguments as they are)
#if RTC_WAVE_FIXED_SHORT
    const SsRenderArgs& LS = late_args<SsRenderArgs>();
#else
    const SsRenderArgs& LS = SA;
#endif
    const RenderArgs& L = LS.fine;
    if (cnt.lead() && (qx & (uint32_t)(K - 1)) == 0u && (qy & (uint32_t)(K - 1)) == 0u) {
        const uint32_t ox = x / (uint32_t)K, oy = yl / (uint32_t)K;
        if (ox < LS.out_width && oy < LS.out_rows) {
            const bool through = SEAM && L.progress != nullptr;  // wave-uniform
            const size_t at = ((size_t)oy * LS.out_width + ox) * 3;
            if (SEAM && L.out_u8 != nullptr) {  // wave-uniform
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
    // render_body's progress tail (see RenderArgs::progress, and the head of this file for why it is written out a second
    // time): the wave's stores are acknowledged -- write-through: in memory -- before it counts itself done; the workgroup's last
    // wave counts the block row, the row's last workgroup the chunk, the chunk's last row writes the host's word.
    if (SEAM && L.progress != nullptr) {
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
#ifdef RTC_SPEC_SS
}  // namespace rtc
// The supersampling kernel of a scene-specialised (hiprtc) build.
// (A is the kernel's first and only argument: ss_render_body's late_args reads it at offset 0 of the kernel-argument segment)
extern "C" __global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void ss_render_kernel_spec(rtc::SsRenderArgs A) {
#if defined(RTC_SPEC_SS_SEAM) && RTC_SPEC_SS_SEAM
    rtc::ss_render_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0, RTC_SPEC_SS, true>(A);  // a context of the one-call seam
#else
    rtc::ss_render_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0, RTC_SPEC_SS, false>(A);
#endif
}
namespace rtc {
#endif
#else
template <int NOBJ, bool SIMPLE, int K>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void ss_render_kernel(SsRenderArgs A) {
    ss_render_body<NOBJ, SIMPLE, K, false>(A);
}
// ... and the one the one-call seam's contexts launch: bytes, write-through stores and progress words on request
template <int NOBJ, bool SIMPLE, int K>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void ss_seam_render_kernel(SsRenderArgs A) {
    ss_render_body<NOBJ, SIMPLE, K, true>(A);
}
#endif

}  // namespace rtc
#endif  // RTC_SUPERSAMPLE_H
