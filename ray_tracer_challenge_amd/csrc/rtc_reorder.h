// Device-side ray reordering (rtc_ctx_ray_order, rtc_ctx_trace_reordered).
//
// A ray stream is traced one lane per ray, ray i in thread i, so a wave's 64 rays are whichever the caller put side by side.
// This file sorts a stream by a coherence key, so that a wave's rays start close together and point the same way:
//   * reorder_key: the one definition of a ray's key, host and device (the formulas are include/rtc.h's, word for word);
//   * the stream box, reduced on the device (reorder_box_kernel) and read on the device (reorder_keys_kernel);
//   * a stable least-significant-digit radix sort of (key, index) pairs, 8-bit digits, four passes over ping-pong buffers:
//     count -> scan -> scatter per pass.  No float arithmetic and no global atomics on element positions: the permutation is
//     np.argsort(keys, kind="stable"), the same on every run;
//   * gather (rays and jitter keys into sorted order) and scatter (colours back into the caller's order).
// The trace between gather and scatter is rtc_trace.h's, untouched.
#pragma once
#include <stdint.h>

// ---- the key ---------------------------------------------------------------------------------------------------------
// f32 + - * /, compares and float-to-int conversions only, nothing fused (-ffp-contract=off), no libm call: the host's
// result (rtc_diag_ray_keys) is the device's bit for bit.
constexpr uint32_t REORDER_ORIGIN_BITS = 12u;  // three 4-bit cells of the stream box, interleaved, x lowest
constexpr uint32_t REORDER_DIR_BITS = 20u;     // two 10-bit octahedral coordinates, interleaved, u lowest
// Which of the two is the major sort order (the key's top bits).  Origin-major: a wave's rays share a cell of the stream's box
// first, then a direction; the direction-major alternative is RTC_AMD_REORDER_DIR_MAJOR=1 in librtc_amd_dev.so (A/B:
// profiles/reorder_times.txt).
constexpr bool REORDER_ORIGIN_MAJOR = true;
static_assert(REORDER_ORIGIN_BITS + REORDER_DIR_BITS == 32u, "a key is one 32-bit word");
constexpr float REORDER_FLT_MAX = 3.402823466e+38f;

struct ReorderBox {  // per axis, over the origin components that are finite; lo = +inf, hi = -inf where there is none
    float lo[3], hi[3];
};

__host__ __device__ inline bool reorder_finite(float x) { return x >= -REORDER_FLT_MAX && x <= REORDER_FLT_MAX; }  // (false for a NaN)
__host__ __device__ inline float reorder_abs(float x) { return x < 0.0f ? -x : x; }
// t -> 0 .. cells - 1; a NaN fails both compares and is cell 0
__host__ __device__ inline uint32_t reorder_cell(float t, float cells, uint32_t last) { return t >= cells ? last : t > 0.0f ? (uint32_t)(int)t : 0u; }
__host__ __device__ inline uint32_t reorder_origin_cell(float x, float lo, float hi) {
    if (!reorder_finite(x) || !(hi > lo)) return 0u;  // (a camera's rays all leave one point: hi == lo on every axis)
    const float t = (x - lo) * (16.0f / (hi - lo));
    return reorder_cell(t, 16.0f, 15u);
}
// bit k of c to bit STEP * k
template <uint32_t STEP, uint32_t BITS>
__host__ __device__ inline uint32_t reorder_spread(uint32_t c) {
    uint32_t r = 0u;
    for (uint32_t k = 0; k < BITS; k++) r |= ((c >> k) & 1u) << (STEP * k);
    return r;
}

__host__ __device__ inline uint32_t reorder_key(const ReorderBox& box, float ox, float oy, float oz, float dx, float dy, float dz, bool dir_major) {
    const uint32_t origin = reorder_spread<3, 4>(reorder_origin_cell(ox, box.lo[0], box.hi[0])) |
                            reorder_spread<3, 4>(reorder_origin_cell(oy, box.lo[1], box.hi[1])) << 1 |
                            reorder_spread<3, 4>(reorder_origin_cell(oz, box.lo[2], box.hi[2])) << 2;
    // the octahedral map: the direction projected on |x| + |y| + |z| = 1, the lower half folded over the upper one's corners
    uint32_t u = 0u, v = 0u;
    const float s = (reorder_abs(dx) + reorder_abs(dy)) + reorder_abs(dz);
    if (s > 0.0f && reorder_finite(s)) {
        float px = dx / s, py = dy / s;
        if (dz < 0.0f) {
            const float qx = (1.0f - reorder_abs(py)) * (px >= 0.0f ? 1.0f : -1.0f);
            const float qy = (1.0f - reorder_abs(px)) * (py >= 0.0f ? 1.0f : -1.0f);
            px = qx, py = qy;
        }
        u = reorder_cell((px * 0.5f + 0.5f) * 1024.0f, 1024.0f, 1023u);
        v = reorder_cell((py * 0.5f + 0.5f) * 1024.0f, 1024.0f, 1023u);
    }
    const uint32_t dir = reorder_spread<2, 10>(u) | reorder_spread<2, 10>(v) << 1;
    return dir_major ? (dir << REORDER_ORIGIN_BITS | origin) : (origin << REORDER_DIR_BITS | dir);
}

// ---- the sort's plan (host) --------------------------------------------------------------------------------------------
constexpr uint32_t REORDER_TILE = 256u;        // a workgroup's sub-tile: one element per thread
constexpr uint32_t REORDER_WGS_PER_CU = 2u;    // a fixed grid, a few workgroups per compute unit ...
constexpr uint32_t REORDER_MAX_GRID = 512u;    // ... capped: the [digit][workgroup] table is scanned by one workgroup
constexpr uint32_t REORDER_DIGITS = 256u, REORDER_PASSES = 4u;
struct ReorderPlan {
    uint32_t grid;     // workgroups of the count and scatter kernels; 0: nothing to sort
    uint32_t segment;  // elements a workgroup owns: workgroup w sorts [w * segment, min(n, (w + 1) * segment)), a multiple of REORDER_TILE
};
inline ReorderPlan reorder_plan(uint32_t n, uint32_t n_cus) {
    ReorderPlan p = {0u, 0u};
    if (n == 0u) return p;
    const uint64_t tiles = ((uint64_t)n + REORDER_TILE - 1u) / REORDER_TILE;
    uint64_t grid = (uint64_t)(n_cus ? n_cus : 1u) * REORDER_WGS_PER_CU;
    if (grid > REORDER_MAX_GRID) grid = REORDER_MAX_GRID;
    if (grid > tiles) grid = tiles;
    const uint64_t tiles_per_wg = (tiles + grid - 1u) / grid;
    p.segment = (uint32_t)(tiles_per_wg * REORDER_TILE);        // (<= 2^32 / grid + 256: fits)
    p.grid = (uint32_t)((tiles + tiles_per_wg - 1u) / tiles_per_wg);  // no workgroup without an element
    return p;
}

#ifdef __HIPCC__
// ---- the stream box --------------------------------------------------------------------------------------------------
// An order-preserving image of a float in the unsigned integers: min and max of the images are the images of min and max,
// whatever the order they are taken in, so one integer atomic per wave and axis gives the exact box.
__device__ inline uint32_t reorder_float_image(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float reorder_image_float(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
constexpr uint32_t REORDER_IMAGE_POS_INF = 0xff800000u, REORDER_IMAGE_NEG_INF = 0x007fffffu;

// box: {lo x, y, z, hi x, y, z} as images; an empty box is {+inf ..., -inf ...}
__global__ void reorder_box_init_kernel(uint32_t* __restrict__ box) {
    if (threadIdx.x < 6u) box[threadIdx.x] = threadIdx.x < 3u ? REORDER_IMAGE_POS_INF : REORDER_IMAGE_NEG_INF;
}

__global__ __launch_bounds__(256) void reorder_box_kernel(const float4* __restrict__ origins, uint32_t n, uint32_t* __restrict__ box) {
    uint32_t lo[3] = {REORDER_IMAGE_POS_INF, REORDER_IMAGE_POS_INF, REORDER_IMAGE_POS_INF};
    uint32_t hi[3] = {REORDER_IMAGE_NEG_INF, REORDER_IMAGE_NEG_INF, REORDER_IMAGE_NEG_INF};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float4 o = origins[i];
        const float x[3] = {o.x, o.y, o.z};
        for (int a = 0; a < 3; a++)
            if (reorder_finite(x[a])) {
                const uint32_t m = reorder_float_image(x[a]);
                lo[a] = m < lo[a] ? m : lo[a];
                hi[a] = m > hi[a] ? m : hi[a];
            }
    }
    for (int a = 0; a < 3; a++) {
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t l = (uint32_t)__shfl_xor((int)lo[a], d), h = (uint32_t)__shfl_xor((int)hi[a], d);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
        if ((threadIdx.x & 63u) == 0u) {
            atomicMin(&box[a], lo[a]);
            atomicMax(&box[3 + a], hi[a]);
        }
    }
}

__global__ __launch_bounds__(256) void reorder_keys_kernel(const float4* __restrict__ origins, const float4* __restrict__ directions, uint32_t n,
                                                           const uint32_t* __restrict__ box_images, uint32_t* __restrict__ keys, bool dir_major) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ReorderBox box;
    for (int a = 0; a < 3; a++) box.lo[a] = reorder_image_float(box_images[a]), box.hi[a] = reorder_image_float(box_images[3 + a]);
    const float4 o = origins[i], d = directions[i];
    keys[i] = reorder_key(box, o.x, o.y, o.z, d.x, d.y, d.z, dir_major);
}

// ---- the sort: one pass = count, scan, scatter ---------------------------------------------------------------------------
// table[digit * gridDim.x + workgroup]: how many elements of the workgroup's segment carry the digit
__global__ __launch_bounds__(256) void reorder_count_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t segment, uint32_t shift,
                                                            uint32_t* __restrict__ table) {
    __shared__ uint32_t hist[REORDER_DIGITS];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * segment;
    const uint64_t end = first + segment < n ? first + segment : n;
    for (uint64_t i = first + threadIdx.x; i < end; i += REORDER_TILE) atomicAdd(&hist[(keys[i] >> shift) & 0xffu], 1u);
    __syncthreads();
    table[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

// The table's exclusive prefix sum in place, digit-major: afterwards table[digit][workgroup] is where the workgroup's first element
// with that digit goes.  One workgroup of 1024: every thread sums a contiguous piece, the 1024 sums are scanned in LDS.
__global__ __launch_bounds__(1024) void reorder_scan_kernel(uint32_t* __restrict__ table, uint32_t entries) {
    __shared__ uint32_t sums[1024];
    const uint32_t piece = (entries + 1023u) / 1024u;
    const uint32_t first = threadIdx.x * piece < entries ? threadIdx.x * piece : entries;
    const uint32_t end = first + piece < entries ? first + piece : entries;
    uint32_t sum = 0u;
    for (uint32_t i = first; i < end; i++) sum += table[i];
    sums[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {  // (Hillis-Steele, inclusive)
        const uint32_t below = threadIdx.x >= d ? sums[threadIdx.x - d] : 0u;
        __syncthreads();
        sums[threadIdx.x] += below;
        __syncthreads();
    }
    uint32_t run = sums[threadIdx.x] - sum;
    for (uint32_t i = first; i < end; i++) {
        const uint32_t c = table[i];
        table[i] = run;
        run += c;
    }
}

// Elements keep their order within a digit: lanes within a wave (a rank from eight ballots), waves within a sub-tile, sub-tiles
// within a segment (the running base), segments within the stream (the table).  idx_in == nullptr: the first pass, element i is ray i.
__global__ __launch_bounds__(256) void reorder_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in, uint32_t n,
                                                              uint32_t segment, uint32_t shift, const uint32_t* __restrict__ table,
                                                              uint32_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
    __shared__ uint32_t base[REORDER_DIGITS];          // where the workgroup's next element of each digit goes
    __shared__ uint32_t wave_off[4][REORDER_DIGITS];   // per wave: first the digit's count in this sub-tile, then its offset
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    base[threadIdx.x] = table[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x];
    const uint64_t first = (uint64_t)blockIdx.x * segment;
    const uint64_t end = first + segment < n ? first + segment : n;
    for (uint64_t tile = first; tile < end; tile += REORDER_TILE) {  // (uniform in the workgroup)
        for (uint32_t w = 0; w < 4u; w++) wave_off[w][threadIdx.x] = 0u;
        __syncthreads();
        const uint64_t i = tile + threadIdx.x;
        const bool valid = i < end;
        const uint32_t key = valid ? keys_in[i] : 0u;
        const uint32_t idx = valid ? (idx_in ? idx_in[i] : (uint32_t)i) : 0u;
        const uint32_t digit = (key >> shift) & 0xffu;
        unsigned long long same = __ballot(valid);  // the lanes of this wave that hold this lane's digit
        for (uint32_t b = 0; b < 8u; b++) {
            const unsigned long long set = __ballot((digit >> b) & 1u);
            same &= ((digit >> b) & 1u) ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wave_off[wave][digit] = (uint32_t)__popcll(same);
        __syncthreads();
        {
            uint32_t run = base[threadIdx.x];
            for (uint32_t w = 0; w < 4u; w++) {
                const uint32_t c = wave_off[w][threadIdx.x];
                wave_off[w][threadIdx.x] = run;
                run += c;
            }
            base[threadIdx.x] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t pos = wave_off[wave][digit] + rank;
            if (pos < n) keys_out[pos] = key, idx_out[pos] = idx;  // (always: the counts are of these very digits)
        }
        __syncthreads();
    }
}

// ---- gather and scatter around the trace -------------------------------------------------------------------------------
// The j-th ray by key, and its jitter key: the caller's, or -- where the caller gave none -- the ray's index in the caller's order,
// which is what an unsorted trace would have drawn its light samples with.
__global__ __launch_bounds__(256) void reorder_gather_kernel(const float4* __restrict__ origins, const float4* __restrict__ directions,
                                                             const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t n,
                                                             float4* __restrict__ out_origins, float4* __restrict__ out_directions,
                                                             uint32_t* __restrict__ out_keys) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = order[j];
    out_origins[j] = origins[i];
    out_directions[j] = directions[i];
    out_keys[j] = keys ? keys[i] : i;
}

__global__ __launch_bounds__(256) void reorder_scatter_colours_kernel(const float* __restrict__ colours, const uint32_t* __restrict__ order, uint32_t n,
                                                                      float* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t i = order[j];
    out[3u * i] = colours[3u * j], out[3u * i + 1u] = colours[3u * j + 1u], out[3u * i + 2u] = colours[3u * j + 2u];
}
#endif  // __HIPCC__
