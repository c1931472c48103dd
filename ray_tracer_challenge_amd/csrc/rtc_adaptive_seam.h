// rtc_adaptive_seam.h -- adaptive supersampling of the one-call seam (rtc_render_adaptive): rtc_adaptive.h's frame for ONE PART of
// a frame whose 64-row bands are dealt round-robin over the entries of opts->devices (DESIGN.md 8e "one-call seam").
//
// An entry holds its share of the base frame B compactly, band after band (rtc_internal.h for_each_band).  The mask's rule looks at a
// pixel's four neighbours in the WHOLE frame, and with more than one part the rows above a band's first row and below its last
// belong to another entry: the halo rows, at most two per band.  The entry traces them itself, on its own device -- a halo pixel is
// exactly B's pixel: primary_ray + norm3 of the plain camera, color_at with key y W + x, zero in the frame's last row and column --
// into a halo buffer of its own, halo row after halo row in the order seam_halo_row defines.  Three kernels, in this order on one
// stream:
//   * the halo pass: adaptive_seam_body<..., K = 1>, one lane per halo pixel, the plain camera's header;
//   * adaptive_seam_mask_kernel: rtc_adaptive.h's rule (adaptive_differs) on the share, a band's outer neighbours read from the halo
//     buffer; flagged pixels are appended as SHARE-LOCAL indices ly * W + x, one contiguous run per 8 x 8 tile, as
//     adaptive_mask_kernel does; in byte mode it also stores scale_color(B) for every pixel it leaves unflagged, so no quantize pass
//     follows;
//   * the refinement: adaptive_seam_body<..., K = 2, 4>, adaptive_refine_body with the entry's local row turned into the global
//     output row for the fine rays (oy = seam_global_row(ly)), the same lane slots (adaptive_slot) and the same reduce
//     (adaptive_reduce): DESIGN.md 8b's order stays the one definition.  It stores f32 over the share's B, or three bytes.
// None of it reports progress: a share's chunks leave when its stream is done.
//
// Included by rtc_device.hip after rtc_adaptive.h, which it includes and which keeps its text (so every kernel there keeps its id),
// and handed to hiprtc beside it and the core (-DRTC_SPEC_ADAPTIVE_SEAM=K, K = 1, 2, 4: adaptive_seam_kernel_spec).
#ifndef RTC_ADAPTIVE_SEAM_H
#define RTC_ADAPTIVE_SEAM_H

#include "rtc_adaptive.h"

namespace rtc {

// One part's share of a W x H frame: `rows` compact rows, bands part, part + n_parts, ... of band_rows rows.
struct AdaptiveShare {
    uint32_t width, height, rows;
    uint32_t band_rows, n_parts, part;
};
// compact row -> row of the frame (rtc_internal.h global_row, restated for the device)
__host__ __device__ inline uint32_t seam_global_row(const AdaptiveShare& s, uint32_t ly) {
    const uint32_t band = ly / s.band_rows;
    return (band * s.n_parts + s.part) * s.band_rows + (ly - band * s.band_rows);
}
// The halo rows of a part, n_parts > 1 (with one part consecutive bands are adjacent and there are none).  Every band of the part has
// a row above it but the frame's first band -- band 0 of part 0 -- and a row below it but the frame's last, which is the last of
// its part: local band j's upper halo row is number 2 j - z and its lower one 2 j + 1 - z, z = 1 for part 0, else 0.
__host__ __device__ inline uint32_t seam_halo_above(const AdaptiveShare& s, uint32_t local_band) { return 2u * local_band - (s.part == 0u ? 1u : 0u); }
__host__ __device__ inline uint32_t seam_halo_below(const AdaptiveShare& s, uint32_t local_band) { return seam_halo_above(s, local_band) + 1u; }
// ... and the frame's row that halo row h holds
__host__ __device__ inline uint32_t seam_halo_row(const AdaptiveShare& s, uint32_t h) {
    const uint32_t t = h + (s.part == 0u ? 1u : 0u), band = (t >> 1) * s.n_parts + s.part;
    return (t & 1u) ? (band + 1u) * s.band_rows : band * s.band_rows - 1u;
}

struct AdaptiveSeamArgs {
    SceneHdr hdr;               // K = 2, 4: the scene's with the FINE camera's width, height and pixel_size; K = 1: the plain camera's
    SceneSoA soa;
    const uint32_t* list;       // K = 2, 4: flagged pixels of the share, ly * W + x
    AdaptiveQueue* queue;       // the list's length (K = 2, 4) and this launch's {rays, shaded hits, culled shadow rays}
    float* out;                 // K = 2, 4: the share's B, [rows][W][3], overwritten at the flagged pixels; K = 1: the halo buffer
    uint8_t* out_u8;            // K = 2, 4, byte mode (wave-uniform): [rows][W][3] bytes instead; else nullptr
    AdaptiveShare share;        // (width and height: the OUTPUT frame's)
    uint32_t n_halo;            // K = 1: halo rows
    int32_t depth;
    uint32_t warm;              // a code object's first launch on a queue: no step is taken
};

DI uint8_t seam_scale_color(float v) { return (uint8_t)fmaxf(fminf(v * 255.0f, 255.0f), 0.0f); }  // canvas.rs:39-43, render_body's arithmetic

template <int NOBJ, bool SIMPLE, int K>
DI void adaptive_seam_body(const AdaptiveSeamArgs& A) {
    static_assert(K == 1 || K == 2 || K == 4, "halo pass or supersampling factor");
    constexpr uint32_t KK = (uint32_t)(K * K);
    const SceneHdr& H = A.hdr;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ float stash_lds[LDS_SLOTS * 256];
    const LaneStash stash = {stash_lds + threadIdx.x, 256u};
    // the wave's counter partial, in LDS between steps and in 64 bits (adaptive_refine_body)
    __shared__ unsigned long long acc[4][3];
    if (lane == 0u) acc[wave][0] = acc[wave][1] = acc[wave][2] = 0ull;
    const uint32_t W = A.share.width;
    unsigned long long n_slots = 0ull;  // wave-uniform
    if (!A.warm) n_slots = K == 1 ? (unsigned long long)A.n_halo * W : (unsigned long long)A.queue->n_flagged * KK;
    const unsigned long long n_waves = (unsigned long long)gridDim.x * 4u;
    for (unsigned long long base = ((unsigned long long)blockIdx.x * 4u + wave) * ADAPTIVE_STEP; base < n_slots; base += n_waves * ADAPTIVE_STEP) {
        const unsigned long long slot = base + lane;
        Counters cnt = {0u, 0u, 0u};
        V3 col = v3(0.0f, 0.0f, 0.0f);
        const bool listed = slot < n_slots;  // lanes past the end contribute zero; K > 1: they only ever form whole groups
        uint32_t p = 0u, sx = 0u, sy = 0u;
        if (listed) {
            uint32_t x, y;
            if constexpr (K == 1) {
                // halo pixel: halo row slot / W of the part, column slot mod W -- B's pixel (x, y) of the plain camera
                const uint32_t hr = (uint32_t)(slot / W);
                x = (uint32_t)(slot - (unsigned long long)hr * W), y = seam_halo_row(A.share, hr);
            } else {
                const AdaptiveSlot s = adaptive_slot<K>(slot);
                sx = s.sx, sy = s.sy;
                p = A.list[s.entry];
                const uint32_t ly = p / W, ox = p - ly * W;
                x = ox * (uint32_t)K + sx, y = seam_global_row(A.share, ly) * (uint32_t)K + sy;
            }
            // camera.rs:80-81 at the header's resolution: the last row and column are black
            if (x < H.width - 1u && y < H.height - 1u) {
                // (has_scene_box is 0 in this header, as in rtc_adaptive.h's: the colours and the counts are the same)
                V3 origin, pixel;
                (void)primary_ray(H, x, y, origin, pixel);
                const V3 direction = norm3(pixel - origin);
                col = color_at<NOBJ, SIMPLE>(H, A.soa, origin, direction, A.depth, y * H.width + x, cnt, stash);  // jitter key: the header's pixel index
            }
        }
        if constexpr (K == 1) {
            if (listed) {
                float* dst = A.out + (size_t)slot * 3;
                dst[0] = col.x;
                dst[1] = col.y;
                dst[2] = col.z;
            }
        } else {
            // after the divergent region: every lane of the wave takes part
            col.x = adaptive_reduce<K>(col.x);
            col.y = adaptive_reduce<K>(col.y);
            col.z = adaptive_reduce<K>(col.z);
            if (listed && sx == 0u && sy == 0u) {
                if (A.out_u8 != nullptr) {  // wave-uniform
                    uint8_t* dst = A.out_u8 + (size_t)p * 3;
                    dst[0] = seam_scale_color(col.x), dst[1] = seam_scale_color(col.y), dst[2] = seam_scale_color(col.z);
                } else {
                    float* dst = A.out + (size_t)p * 3;
                    dst[0] = col.x;
                    dst[1] = col.y;
                    dst[2] = col.z;
                }
            }
        }
        const uint4 counts = reduce_wave_counts(cnt);
        if (lane == COUNTS_LANE) acc[wave][0] += counts.x, acc[wave][1] += counts.y, acc[wave][2] += counts.z;
    }
    // one partial per wave, added to the totals the host zeroed; a wave that took no step adds nothing (adaptive_refine_body)
    if (lane < 3u && acc[wave][0] != 0ull) atomicAdd(&A.queue->total[lane], acc[wave][lane]);
}

#ifdef RTC_SPEC_LIST
#ifdef RTC_SPEC_ADAPTIVE_SEAM
}  // namespace rtc
// The seam's refinement kernel (2, 4) or halo pass (1) of a scene-specialised (hiprtc) build.
extern "C" __global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void adaptive_seam_kernel_spec(rtc::AdaptiveSeamArgs A) {
    rtc::adaptive_seam_body<RTC_SPEC_NOBJ, RTC_SPEC_SIMPLE != 0, RTC_SPEC_ADAPTIVE_SEAM>(A);
}
namespace rtc {
#endif
#else
template <int NOBJ, bool SIMPLE, int K>
__global__ __launch_bounds__(256, RTC_WAVES_PER_SIMD) void adaptive_seam_kernel(AdaptiveSeamArgs A) {
    adaptive_seam_body<NOBJ, SIMPLE, K>(A);
}

// The banded mask and list.  adaptive_mask_kernel's layout -- one wave per 8 x 8 tile, 2 x 2 waves per 16 x 16 block, a workgroup
// strides through the blocks -- over the share's compact rows.  Left and right neighbours are the share's; the row above a band's
// first row and the one below its last are halo rows when the frame has several parts (seam_halo_above / _below), the share's
// own neighbouring compact rows when it has one.  Whether a neighbour exists is decided with the WHOLE frame's coordinates.
struct AdaptiveSeamMaskArgs {
    const float* frame;  // the share's B: [rows][W][3]
    const float* halo;   // [halo rows][W][3] (never read when n_parts == 1)
    uint8_t* mask;       // [rows][W], 1 = flagged; or nullptr (wave-uniform)
    uint8_t* out_u8;     // byte mode: [rows][W][3], scale_color(B) where the pixel is NOT flagged; else nullptr (wave-uniform)
    uint32_t* list;      // [rows * W]
    AdaptiveQueue* queue;
    AdaptiveShare share;
    uint32_t blocks_x, n_blocks;  // 16 x 16 blocks across the share, and in all
    float threshold;
};
__global__ __launch_bounds__(256) void adaptive_seam_mask_kernel(AdaptiveSeamMaskArgs A) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lx = (wave & 1u) * 8u + (lane & 7u), lyb = (wave >> 1) * 8u + (lane >> 3);
    const AdaptiveShare& S = A.share;
    const uint32_t W = S.width;
    const bool split = S.n_parts > 1u;  // uniform
    for (uint32_t b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {  // uniform over the workgroup
        const uint32_t by = b / A.blocks_x, bx = b - by * A.blocks_x;
        const uint32_t x = bx * 16u + lx, ly = by * 16u + lyb;
        bool flagged = false;
        if (x < W && ly < S.rows) {
            const uint32_t band = ly / S.band_rows, r = ly - band * S.band_rows;
            const uint32_t y = (band * S.n_parts + S.part) * S.band_rows + r;  // seam_global_row
            const size_t i = (size_t)ly * W + x;
            const float* p = A.frame + i * 3;
            if (x > 0u) flagged = flagged || adaptive_differs(p, p - 3, A.threshold);
            if (x + 1u < W) flagged = flagged || adaptive_differs(p, p + 3, A.threshold);
            if (y > 0u) {
                const float* n = (r > 0u || !split) ? p - (size_t)W * 3 : A.halo + ((size_t)seam_halo_above(S, band) * W + x) * 3;
                flagged = flagged || adaptive_differs(p, n, A.threshold);
            }
            if (y + 1u < S.height) {
                const float* n = (r + 1u < S.band_rows || !split) ? p + (size_t)W * 3 : A.halo + ((size_t)seam_halo_below(S, band) * W + x) * 3;
                flagged = flagged || adaptive_differs(p, n, A.threshold);
            }
            if (A.mask != nullptr) A.mask[i] = flagged ? 1 : 0;
            if (A.out_u8 != nullptr && !flagged) {
                uint8_t* dst = A.out_u8 + i * 3;
                dst[0] = seam_scale_color(p[0]), dst[1] = seam_scale_color(p[1]), dst[2] = seam_scale_color(p[2]);
            }
        }
        // the wave's flagged pixels as one contiguous run of the list (adaptive_mask_kernel)
        const unsigned long long votes = __ballot(flagged);
        if (votes != 0ull) {  // wave-uniform
            const uint32_t rank = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(&A.queue->n_flagged, (uint32_t)__popcll(votes));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (flagged) A.list[base + rank] = ly * W + x;
        }
    }
}
#endif

}  // namespace rtc
#endif  // RTC_ADAPTIVE_SEAM_H
