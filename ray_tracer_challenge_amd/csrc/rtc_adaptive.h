// rtc_adaptive.h -- adaptive supersampling (rtc_ctx_render_adaptive): K x K rays only for the pixels of a rendered frame
// that differ from a neighbour.
//
// Two kernels behind the context's normal render of the frame B.  The mask kernel reads B, flags every pixel one of whose
// 4-neighbours differs from it by more than the threshold in some channel, and appends the flagged pixels' indices to a
// device list, one contiguous run per 8 x 8 tile: the list stays tile-compact, which is the order ray streams want.  The
// refinement kernel gives every entry of that list K^2 neighbouring lanes of one wave, one lane per fine sample: each
// builds its ray of the FINE camera with the core's primary_ray, calls color_at with the fine pixel index as jitter key --
// what ss_render_body does for the same fine pixel -- and an xor-butterfly adds the K^2 samples up in the order of
// include/rtc.h's supersampling contract (tests/supersample_helpers.box_filter is the same order
// in numpy).  One lane per entry stores three dwords over B's pixel.
//
// How many pixels are flagged never reaches the host: both kernels are launched as a fixed number of workgroups whose
// waves stride through the work -- tiles of B, steps of 64 lane slots of the list -- until it is exhausted.
//
// Included by rtc_device.hip after rtc_kernel_core.h (ahead-of-time instantiations) and handed to hiprtc beside it
// (-DRTC_SPEC_ADAPTIVE=K: adaptive_refine_kernel_spec), as rtc_supersample.h and rtc_trace.h are.  Like a ray stream the
// refinement has no frame of its own: no block lists, tiles, rectangles, swizzle, lane sharing, progress words, u8 canvas.
#ifndef RTC_ADAPTIVE_H
#define RTC_ADAPTIVE_H

#include "rtc_kernel_core.h"

namespace rtc {

// What the two kernels share on the device, zeroed by the host in front of the mask kernel: the number of flagged pixels
// and the refinement's {rays, shaded hits, culled shadow rays}, 64 bits each (a wave of a small grid may serve millions of
// samples of a large frame).
struct AdaptiveQueue {
    uint32_t n_flagged, pad;
    unsigned long long total[3];
};

// The refinement's lane slots.  Slot j serves entry j / K^2 of the flagged-pixel list and fine sample j mod K^2 of that
// pixel, sx in the low log2 K bits and sy in the next; a wave's step is ADAPTIVE_STEP consecutive slots, one per lane, so a
// pixel's K^2 samples are K^2 consecutive lanes and never straddle a wave.  The one definition: the kernel below calls it,
// and the CPU tests reach it through rtc_diag_adaptive_plan.
constexpr uint32_t ADAPTIVE_STEP = 64u;
struct AdaptiveSlot {
    uint32_t entry, sx, sy, lane;
};
template <int K>
__host__ __device__ inline AdaptiveSlot adaptive_slot(unsigned long long slot) {
    static_assert(K == 2 || K == 4, "supersampling factor");
    constexpr uint32_t KK = (uint32_t)(K * K), K_LOG2 = K == 4 ? 2u : 1u;
    const uint32_t sub = (uint32_t)slot & (KK - 1u);
    return {(uint32_t)(slot / KK), sub & (uint32_t)(K - 1), sub >> K_LOG2, (uint32_t)slot & (ADAPTIVE_STEP - 1u)};
}

struct AdaptiveRefineArgs {
    SceneHdr hdr;               // the scene's, with the FINE camera's width, height and pixel_size; has_scene_box = 0 (see below)
    SceneSoA soa;
    const uint32_t* list;       // flagged pixels of the W x H frame, y * W + x
    AdaptiveQueue* queue;
    float* out;                 // [H][W][3]: B, overwritten at the flagged pixels
    uint32_t out_width;         // W
    int32_t depth;
    uint32_t warm;              // a code object's first launch on a queue: no step is taken
};

// One channel of the K x K block whose samples sit in K^2 consecutive lanes, sx in the low log2 K bits of the lane, sy in
// the next: lanes ^ 1 (^ 2) along x, then ^ K (^ 2 K) along y -- the contract's ((a + b) + (c + d)) and its K = 4 form.  All
// four steps stay inside a row of 16 lanes.  ^ 1, ^ 2 and ^ 8 are DPP controls folded into the v_add_f32 itself
// (quad_perm:[1,0,3,2], quad_perm:[2,3,0,1], row_ror:8), as rtc_supersample.h has them; ^ 4 has no DPP control on gfx9 and is
// ds_swizzle_b32 in bit mode (and 0x1f, or 0, xor 4).  Not measured for this kernel: the choice follows
// profiles/supersample_xlane_ab.txt, which measured DPP and the xor-16 swizzle against ds_bpermute for rtc_supersample.h; the
// three or twelve cross-lane adds of a step stand behind a color_at.
template <int CTRL>
DI float adaptive_dpp(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
DI float adaptive_swizzle_xor4(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x101f)); }
template <int K>
DI float adaptive_reduce(float v) {
    static_assert(K == 2 || K == 4, "supersampling factor");
    v = v + adaptive_dpp<0xB1>(v);
    v = v + adaptive_dpp<0x4E>(v);
    if constexpr (K == 4) {
        v = v + adaptive_swizzle_xor4(v);
        v = v + adaptive_dpp<0x128>(v);
    }
    return v * (1.0f / (float)(K * K));  // 0.25f / 0.0625f: exact constants
}

template <int NOBJ, bool SIMPLE, int K>
DI void adaptive_refine_body(const AdaptiveRefineArgs& A) {
    constexpr uint32_t KK = (uint32_t)(K * K);
    const SceneHdr& H = A.hdr;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ float stash_lds[LDS_SLOTS * 256];
    const LaneStash stash = {stash_lds + threadIdx.x, 256u};
    // The wave's counter partial lives in LDS between steps, not in registers across color_at, in 64 bits.  (A pixel's packed
    // counters are sized for one pixel -- Counters::shaded -- so they are unpacked after every step.)
    __shared__ unsigned long long acc[4][3];
    if (lane == 0u) acc[wave][0] = acc[wave][1] = acc[wave][2] = 0ull;
    const unsigned long long n_slots = A.warm ? 0ull : (unsigned long long)A.queue->n_flagged * KK;  // wave-uniform: a scalar load
    // Wave w of the grid's n takes steps w, w + n, w + 2 n, ... of 64 slots: a short list -- the usual one, edges are a few
    // per cent of a frame -- is spread one step per wave over the whole device, a long one evenly, with no counter to pull
    // from.  (Waves that pulled 256 slots from a device head counter and worked through them in four steps left most of
    // the device idle behind a short list: profiles/adaptive_chunk_ab.txt.)
    const unsigned long long n_waves = (unsigned long long)gridDim.x * 4u;
    for (unsigned long long base = ((unsigned long long)blockIdx.x * 4u + wave) * ADAPTIVE_STEP; base < n_slots; base += n_waves * ADAPTIVE_STEP) {
        const unsigned long long slot = base + lane;
        Counters cnt = {0u, 0u, 0u};
        V3 col = v3(0.0f, 0.0f, 0.0f);
        uint32_t p = 0u;
        const bool listed = slot < n_slots;  // lanes past the end of the list contribute zero; they only ever form whole groups
        const AdaptiveSlot s = adaptive_slot<K>(slot);
        if (listed) {
            p = A.list[s.entry];
            const uint32_t oy = p / A.out_width, ox = p - oy * A.out_width;
            const uint32_t x = ox * (uint32_t)K + s.sx, y = oy * (uint32_t)K + s.sy;
            // camera.rs:80-81 at the fine resolution: the fine frame's last row and column are black
            if (x < H.width - 1u && y < H.height - 1u) {
                // (has_scene_box is 0 in this header: the early-out's padding is argued for the camera the scene was planned
                // with, and a miss costs color_at one counted ray either way -- the colours and the counts are the same)
                V3 origin, pixel;
                (void)primary_ray(H, x, y, origin, pixel);
                const V3 direction = norm3(pixel - origin);
                col = color_at<NOBJ, SIMPLE>(H, A.soa, origin, direction, A.depth, y * H.width + x, cnt, stash);  // jitter key: the FINE pixel index
            }
        }
        // after the divergent region: every lane of the wave takes part
        col.x = adaptive_reduce<K>(col.x);
        col.y = adaptive_reduce<K>(col.y);
        col.z = adaptive_reduce<K>(col.z);
        if (listed && s.sx == 0u && s.sy == 0u) {
            float* dst = A.out + (size_t)p * 3;
            dst[0] = col.x;
            dst[1] = col.y;
            dst[2] = col.z;
        }
        const uint4 counts = reduce_wave_counts(cnt);
        if (lane == COUNTS_LANE) acc[wave][0] += counts.x, acc[wave][1] += counts.y, acc[wave][2] += counts.z;
    }
    // one partial per wave, added to the totals the host zeroed; no workgroup barrier (a finished wave leaves); a wave that
    // took no step adds nothing
    if (lane < 3u && acc[wave][0] != 0ull) atomicAdd(&A.queue->total[lane], acc[wave][lane]);
}

#ifdef RTC_SPEC_LIST
#ifdef RTC_SPEC_ADAPTIVE
}  // namespace rtc
// The refinement kernel of a scene-specialised (hiprtc) build.
extern "C" __global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void adaptive_refine_kernel_spec(rtc::AdaptiveRefineArgs A) {
    rtc::adaptive_refine_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0, RTC_SPEC_ADAPTIVE>(A);
}
namespace rtc {
#endif
#else
template <int NOBJ, bool SIMPLE, int K>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void adaptive_refine_kernel(AdaptiveRefineArgs A) {
    adaptive_refine_body<NOBJ, SIMPLE, K>(A);
}

// The mask and the list.  One wave per 8 x 8 tile of B at a time, 2 x 2 waves per 16 x 16 block (render_body's layout); a
// workgroup strides through the blocks, b = blockIdx.x, + gridDim.x, ...: no barrier, no LDS.  (A workgroup per block was
// bound by starting its waves: 262 144 of them at 4096^2, 0.34 ms for traffic HBM serves in 0.05 --
// profiles/adaptive_chunk_ab.txt.)  A pixel is flagged when |B[p][c] - B[n][c]| > threshold for one of its up to four
// neighbours n inside the frame and one channel c: f32 subtraction, fabsf, a strict compare -- a NaN difference (NaN
// operands, inf - inf) compares false and never flags.  The rule is symmetric, so both pixels of a contrasting pair flag
// themselves.
struct AdaptiveMaskArgs {
    const float* frame;  // B: [height][width][3]
    uint8_t* mask;       // [height][width], 1 = flagged; or nullptr (wave-uniform)
    uint32_t* list;      // [width * height]
    AdaptiveQueue* queue;
    uint32_t width, height;
    uint32_t blocks_x, n_blocks;  // 16 x 16 blocks across, and in all
    float threshold;
};
DI bool adaptive_differs(const float* a, const float* b, float threshold) {
    return fabsf(a[0] - b[0]) > threshold || fabsf(a[1] - b[1]) > threshold || fabsf(a[2] - b[2]) > threshold;
}
__global__ __launch_bounds__(256) void adaptive_mask_kernel(AdaptiveMaskArgs A) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lx = (wave & 1u) * 8u + (lane & 7u), ly = (wave >> 1) * 8u + (lane >> 3);
    for (uint32_t b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {  // uniform over the workgroup
        const uint32_t by = b / A.blocks_x, bx = b - by * A.blocks_x;
        const uint32_t x = bx * 16u + lx, y = by * 16u + ly;
        bool flagged = false;
        if (x < A.width && y < A.height) {
            const size_t i = (size_t)y * A.width + x;
            const float* p = A.frame + i * 3;
            if (x > 0u) flagged = flagged || adaptive_differs(p, p - 3, A.threshold);
            if (x + 1u < A.width) flagged = flagged || adaptive_differs(p, p + 3, A.threshold);
            if (y > 0u) flagged = flagged || adaptive_differs(p, p - (size_t)A.width * 3, A.threshold);
            if (y + 1u < A.height) flagged = flagged || adaptive_differs(p, p + (size_t)A.width * 3, A.threshold);
            if (A.mask != nullptr) A.mask[i] = flagged ? 1 : 0;
        }
        // the wave's flagged pixels as one contiguous run of the list: one ballot, the lane's rank among the set bits, one
        // device-scope atomic per wave on the list's length
        const unsigned long long votes = __ballot(flagged);
        if (votes != 0ull) {  // wave-uniform
            const uint32_t rank = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(&A.queue->n_flagged, (uint32_t)__popcll(votes));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (flagged) A.list[base + rank] = y * A.width + x;
        }
    }
}
#endif

}  // namespace rtc
#endif  // RTC_ADAPTIVE_H
