// rtc_launch_plan.h -- how a partition's rows become workgroups: block lists, scene-tile lists, scene-rectangle launches,
// the regular grid with its padding and progress chunks.  Integer arithmetic on the frame size, the partition and the
// scene's tile masks: no device, no context (rtc_device.hip's ctx_render_slot owns those and fills RenderArgs from a
// LaunchPlan).  tests/test_block_lists.py and tests/test_launch_plan.py reach these functions through rtc_diag_* entry points.
#ifndef RTC_LAUNCH_PLAN_H
#define RTC_LAUNCH_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <queue>
#include <vector>

#include "rtc_internal.h"

namespace rtc {

// a row-major map of 16 x 16 pixel tiles of the frame
struct TileMask {
    const uint8_t* bits;
    uint32_t w, h;
};

// RenderArgs::tiles' words: lanes per pixel 2^s (s = 0 .. 4), pixel origin (multiples of 4; local rows below 2^17)
inline uint32_t tile_word(uint32_t s, uint32_t x0, uint32_t y0) { return (s & 3u) << 30 | (x0 / 4u) << 16 | (s >> 2) << 15 | (y0 / 4u); }
inline uint32_t tile_s(uint32_t t) { return (t >> 30) | ((t >> 13) & 4u); }
inline uint32_t tile_x0(uint32_t t) { return ((t >> 16) & 0x3fffu) << 2; }
inline uint32_t tile_y0(uint32_t t) { return (t & 0x7fffu) << 2; }
// Supersampled frames (rtc_supersample.h): the k x k fine pixels of an output pixel are added up across the lanes of ONE wave, so a
// k x k group must lie in one wave's tile.  Wave tiles are 8 x 8, 8 x 4, 4 x 4, 4 x 2 and 2 x 2 pixels for s = 0 .. 4 lanes per
// pixel (log2), at origins that are multiples of their size: any s serves k = 2, k = 4 needs s <= 2.  (Block origins are
// multiples of 4 pixels: groups never straddle blocks.)  k = 1: no cap.
inline uint32_t ss_max_share_log2(uint32_t k) { return k == 4u ? 2u : 4u; }
// Adaptive supersampling (rtc_adaptive.h; the slot -> (entry, sx, sy) mapping is that header's adaptive_slot).  The refinement's
// grid: how many workgroups of four waves the device holds at once (the kernel's occupancy), and no more than a fully flagged
// frame could give one step of ADAPTIVE_STEP_SLOTS slots per wave -- never a function of how many pixels ARE flagged, which the
// host does not know.  The waves stride through the list's steps.
constexpr uint32_t ADAPTIVE_STEP_SLOTS = 64u;
inline uint32_t adaptive_grid(uint32_t n_cus, uint32_t wgs_per_cu, uint32_t width, uint32_t height, uint32_t k) {
    const uint64_t slots = (uint64_t)width * height * k * k, per_wg = 4ull * ADAPTIVE_STEP_SLOTS;
    const uint64_t resident = (uint64_t)std::max(1u, n_cus) * std::max(1u, wgs_per_cu);
    return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(resident, (slots + per_wg - 1u) / per_wg));
}
// ... and the mask kernel's: workgroups striding through the frame's 16 x 16 blocks, eight per compute unit at the most
inline uint32_t adaptive_mask_grid(uint32_t n_cus, uint32_t n_blocks) { return std::max(1u, std::min(n_blocks, std::max(1u, n_cus) * 8u)); }
// the blocks of the 16 x 16 tile at (x0, y0) at 2^s lanes per pixel, clipped to the partition
inline void push_tile_blocks(std::vector<uint32_t>* out, uint32_t s, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows) {
    const uint32_t hbw = 16u >> (s >> 1), hbh = 16u >> ((s + 1u) >> 1);
    for (uint32_t dy = 0; dy < 16u && y0 + dy < rows; dy += hbh)
        for (uint32_t dx = 0; dx < 16u && x0 + dx < width; dx += hbw) out->push_back(tile_word(s, x0 + dx, y0 + dy));
}
// The block list of one partition (RenderArgs::tiles): the 16 x 16 tiles of the partition's compact rows, those a mesh
// projects to first and cut into blocks of 2^mesh_share_log2 lanes per pixel (8 x 8 or 8 x 4 pixels), the others after
// them, whole, one lane per pixel.
// block_order, block_s, block_s_top: the policy's switches of those names.
inline void build_block_list(bool block_order, int block_s, int block_s_top, const TileMask& T, uint32_t width, uint32_t mesh_share_log2, uint32_t rows,
                             const Partition& q, std::vector<uint32_t>* out, uint32_t cap_s = 4u /* ss_max_share_log2 */) {
    out->clear();
    std::vector<uint32_t> light;
    uint32_t hs = mesh_share_log2;  // lanes per pixel (log2) in the mesh tiles; RTC_AMD_BLOCK_S=0..3: development
    // the dearest tiles first (rank 3: glass that also reflects), or the frame ends waiting for a few waves that started
    // late (RTC_AMD_BLOCK_ORDER=0: image order; RTC_AMD_BLOCK_S_TOP=0..3: lanes per pixel of rank 3 alone -- development)
    const bool ordered = block_order;
    uint32_t hs_top = hs;
    // large frames at two lanes: only the glass keeps them, the other meshes' tiles take one (first frames of here_be_dragons
    // 4000 x 1600 2.87 -> 2.68 ms, mesh 2048^2 3.47 -> 3.24; at 1024^2 and below the other way round: 2.38 -> 2.70,
    // profiles/r03_ab_first_frame_lanes.txt)
    if (hs == 1u && ((uint64_t)width * rows + 63u) / 64u > 60000u) hs = 0u;
    if (block_s >= 0) hs = hs_top = (uint32_t)block_s;
    if (block_s_top >= 0) hs_top = (uint32_t)block_s_top;
    hs = std::min(hs, cap_s), hs_top = std::min(hs_top, cap_s);
    for (uint32_t rank = 3u; rank >= 1u; rank--) {
        const uint32_t s = rank == 3u ? hs_top : hs;
        for (uint32_t yl0 = 0; yl0 < rows; yl0 += 16u) {
            const uint32_t y = global_row(q, yl0);  // of the tile's first row
            for (uint32_t x0 = 0; x0 < width; x0 += 16u) {
                const uint32_t ty = std::min(y / 16u, T.h - 1u), tx = std::min(x0 / 16u, T.w - 1u);
                const uint32_t r = T.bits[(size_t)ty * T.w + tx];
                if (r != 0u && (ordered ? r == rank : rank == 1u)) push_tile_blocks(out, s, x0, yl0, width, rows);
                else if (rank == 1u && r == 0u) light.push_back(tile_word(0u, x0, yl0));
            }
        }
    }
    out->insert(out->end(), light.begin(), light.end());
}

// Feedback for block lists.  The list a scene starts with knows three kinds of tile (build_block_list) and nothing of what a tile
// costs; the frame it schedules ends with a tail -- here_be_dragons 4000 x 1600: waves of 2.3 ms that started at 0.8 ms of a 3.1 ms
// frame; mesh 2048^2: the machine runs out of waves at 2.2 ms, the longest (two lanes per pixel, the centre of the glass mesh)
// run to 3.4.  The first launch of a list therefore times its waves (RenderArgs::wave_ticks), and the list of every later frame
// of this scene and partition is made from those times: a 16 x 16 tile whose longest wave ran more than half of the frame's
// throughput time (the sum of all waves' times over the wave slots of the device) gets more lanes per pixel, each doubling
// taken to shorten its waves to 0.7 (measured: tools/ab_env.py over RTC_AMD_BLOCK_S), and the tiles start in the order of their predicted
// longest wave.  Which lanes trace a pixel and when changes nothing about its value (tests/test_gpu_fullsize.py compares first
// and later frames with the oracle).
inline void refine_block_list(const std::vector<uint32_t>& list, const uint32_t* ticks /* [4 list.size()] */, uint32_t width, uint32_t rows, double wave_slots,
                              double threshold, double down, std::vector<uint32_t>* out, uint32_t max_s = 4u, double* throughput_ticks = nullptr,
                              uint32_t cap_s = 4u /* ss_max_share_log2: entries above it come back capped */) {
    struct Tile {
        uint32_t x0, y0, s;
        uint64_t longest = 0;
        double predicted = 0.0;
    };
    const uint32_t tw = (width + 15u) / 16u;
    std::vector<Tile> tiles;
    std::vector<int32_t> index((size_t)tw * ((rows + 15u) / 16u), -1);
    uint64_t total = 0u;  // (an integer: a chain of double additions, four per block, was most of this loop's time)
    for (size_t b = 0; b < list.size(); b++) {
        const uint32_t t = list[b], x0 = tile_x0(t), y0 = tile_y0(t);
        if (x0 >= width || y0 >= rows) continue;  // (a padded grid's blocks outside the image)
        int32_t& slot = index[(size_t)(y0 / 16u) * tw + x0 / 16u];
        if (slot < 0) {
            slot = (int32_t)tiles.size();
            Tile n;
            n.x0 = x0 & ~15u, n.y0 = y0 & ~15u, n.s = std::min(tile_s(t), cap_s);
            tiles.push_back(n);
        }
        Tile& tile = tiles[(size_t)slot];
        const uint32_t* d = ticks + 4u * b;  // (the block's four waves)
        tile.longest = std::max<uint64_t>(tile.longest, std::max(std::max(d[0], d[1]), std::max(d[2], d[3])));
        total += (uint64_t)d[0] + d[1] + d[2] + d[3];
    }
    const double throughput = (double)total / std::max(1.0, wave_slots);  // ticks the frame takes if the work were spread evenly
    if (throughput_ticks) *throughput_ticks = throughput;
    for (Tile& t : tiles) {
        t.predicted = (double)t.longest;
        while (t.s < std::min(max_s, cap_s) && t.predicted > threshold * throughput) t.s++, t.predicted *= 0.7;  // (up to sixteen lanes per pixel)
        while (t.s > 0u && t.predicted / 0.7 < down * throughput) t.s--, t.predicted /= 0.7;
    }
    // the tiles by predicted longest wave, longest first, equal ones in list order: a radix sort of the (non-negative) doubles' bit
    // patterns, 16 bits a pass, passes whose digit is the same everywhere skipped -- a comparison sort of 16 384 tiles cost the host
    // 2 ms in front of the frame that waits for the list, this a tenth of that
    std::vector<uint32_t> order(tiles.size()), other(tiles.size());
    {
        std::vector<uint64_t> key(tiles.size());
        uint64_t all_or = 0u, all_and = ~(uint64_t)0u;
        for (uint32_t i = 0; i < order.size(); i++) {
            const double pr = tiles[i].predicted > 0.0 ? tiles[i].predicted : 0.0;
            uint64_t k;
            std::memcpy(&k, &pr, sizeof(k));
            key[i] = ~k;  // (ascending in ~k = descending in the prediction)
            all_or |= key[i], all_and &= key[i];
            order[i] = i;
        }
        std::vector<uint32_t> count(65537u);
        for (uint32_t shift = 0u; shift < 64u; shift += 16u) {
            if ((((all_or ^ all_and) >> shift) & 0xffffu) == 0u) continue;
            std::fill(count.begin(), count.end(), 0u);
            for (uint32_t i : order) count[((key[i] >> shift) & 0xffffu) + 1u]++;
            for (uint32_t d = 0u; d < 65536u; d++) count[d + 1u] += count[d];
            for (uint32_t i : order) other[count[(key[i] >> shift) & 0xffffu]++] = i;
            order.swap(other);
        }
    }
    out->clear();
    for (uint32_t i : order) push_tile_blocks(out, tiles[i].s, tiles[i].x0, tiles[i].y0, width, rows);
}

// How long a frame takes whose blocks start in the given order: every block goes to the workgroup slot that is free first and
// keeps it for as long as its longest wave ran (what the dispatcher does, with costs in whatever unit `cost` is in).
inline double simulate_dispatch(const std::vector<uint32_t>& cost, size_t slots) {
    std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
    for (size_t i = 0; i < std::max<size_t>(1, slots); i++) free_at.push(0.0);
    double end = 0.0;
    for (uint32_t c : cost) {
        const double t = free_at.top() + (double)c;
        free_at.pop();
        free_at.push(t);
        end = std::max(end, t);
    }
    return end;
}

// The block list of a frame that shares an area light's cells between a pixel's lanes: every tile with the frame's lane
// count, in image order (the feedback then gives the tiles in the penumbra more lanes, the lit and the empty ones fewer).
inline void uniform_block_list(uint32_t share_log2, uint32_t width, uint32_t rows, std::vector<uint32_t>* out) {
    out->clear();
    for (uint32_t y0 = 0; y0 < rows; y0 += 16u)
        for (uint32_t x0 = 0; x0 < width; x0 += 16u) push_tile_blocks(out, share_log2, x0, y0, width, rows);
}

// the traced rows (global row < h - 1) among a partition's local rows [l0, l1)
inline uint64_t traced_rows(uint32_t height, const Partition& q, uint32_t l0 = 0u, uint32_t l1 = ~0u) {
    uint64_t n = 0;
    const uint32_t lim = height - 1u;
    for_each_band(height, q, [&](uint32_t y0, uint32_t y1, uint32_t local0) {
        const uint32_t a = std::max(local0, l0), e = std::min(local0 + (y1 - y0), l1);
        if (a < e) n += std::min(y0 + (e - local0), lim) - std::min(y0 + (a - local0), lim);
    });
    return n;
}
// traced pixels among a partition's rows: x < w - 1, y < h - 1
inline uint64_t traced_pixels(uint32_t width, uint32_t height, const Partition& q) { return traced_rows(height, q) * (uint64_t)(width - 1u); }

// A scene-tile launch of one partition (band_rows a multiple of 16): one workgroup per 16 x 16 tile of the mask (`tiles`,
// by local row), and the tiles that are NOT in the mask as runs of at most 64 within a tile row, for the zero-fill
// (fill_tiles_kernel reads them as uint2).
struct FillRun {
    uint32_t x0_n;  // first tile | number of tiles << 16
    uint32_t row;   // local pixel row of the tiles' first row
};
struct SceneTilePlan {
    std::vector<uint32_t> tiles;
    std::vector<FillRun> fill;
    unsigned long long traced_pixels = 0ull;  // traced pixels (x < w - 1, y < h - 1) inside the listed tiles
};
inline void plan_scene_tiles(const TileMask& mask, uint32_t width, uint32_t height, const Partition& q, SceneTilePlan* out) {
    out->tiles.clear(), out->fill.clear(), out->traced_pixels = 0ull;
    for_each_band(height, q, [&](uint32_t y0, uint32_t y1, uint32_t local0) {
        for (uint32_t ty = y0 / 16u; ty * 16u < y1; ty++) {
            const uint32_t yl = local0 + (ty * 16u - y0);
            uint32_t run0 = 0u, run = 0u;  // the current run of unlisted tiles: [run0, run0 + run)
            auto close_run = [&]() {
                for (uint32_t k = 0; k < run; k += 64u) out->fill.push_back({(run0 + k) | (std::min(64u, run - k) << 16), yl});
                run = 0u;
            };
            for (uint32_t tx = 0; tx < mask.w; tx++) {
                if (!mask.bits[(size_t)ty * mask.w + tx]) {
                    if (run == 0u) run0 = tx;
                    run++;
                    continue;
                }
                close_run();
                out->tiles.push_back(tile_word(0u, tx * 16u, yl));
                const uint32_t px1 = std::min(width - 1u, tx * 16u + 16u), py1 = std::min(std::min(height - 1u, y1), ty * 16u + 16u);
                if (px1 > tx * 16u && py1 > ty * 16u) out->traced_pixels += (unsigned long long)(px1 - tx * 16u) * (py1 - ty * 16u);
            }
            close_run();
        }
    });
}

// Scheduling for scene-tile lists: what the regular grid has (RenderArgs::swizzle for a first frame, the grid feedback's order for
// the later ones), as arithmetic on the list.
// What a wave cost, from what it counted (RenderArgs::block_counts: rays, shade points, shadow rays the light-cone cull resolved):
// rays that met objects, and shade points (each a light-cone cull, a Phong evaluation, a push or pop of the recursion) at sixteen
// rays apiece.
inline uint32_t wave_work(uint32_t rays, uint32_t shade_points, uint32_t culled) { return (rays - std::min(rays, culled)) + 16u * shade_points + culled / 8u; }
// Is the longest-first order worth a list?  Both orders go through a model of the dispatcher with the blocks' costs (ticks: four
// waves per block): yes when it ends the frame at least 3 % earlier.
inline bool longest_first_pays(const uint32_t* ticks, size_t n_blocks, size_t wg_slots, double* in_order = nullptr, double* longest_first = nullptr) {
    std::vector<uint32_t> block_cost(n_blocks), sorted_cost;
    for (size_t b = 0; b < n_blocks; b++) block_cost[b] = std::max(std::max(ticks[4 * b], ticks[4 * b + 1]), std::max(ticks[4 * b + 2], ticks[4 * b + 3]));
    sorted_cost = block_cost;
    std::sort(sorted_cost.begin(), sorted_cost.end(), std::greater<uint32_t>());
    const double a = simulate_dispatch(block_cost, wg_slots), b = simulate_dispatch(sorted_cost, wg_slots);
    if (in_order) *in_order = a;
    if (longest_first) *longest_first = b;
    return b < 0.97 * a;
}
// A scene-tile list's first frame: the list is in image order (plan_scene_tiles); the regular grid starts its blocks permuted within
// four block rows -- workgroup j of such a group renders block (2 (j >> 3) + (j & 1), (j & 7) >> 1) of it -- and so does the list:
// its tiles in the order in which that walk meets them.  (Tiles are whole, one lane per pixel: `list` holds one word per tile.)
inline void swizzle_tile_list(const std::vector<uint32_t>& list, uint32_t width, uint32_t rows, std::vector<uint32_t>* out) {
    const uint32_t tw = (width + 15u) / 16u, th = (rows + 15u) / 16u, gx = (tw + 1u) & ~1u;
    std::vector<int32_t> index((size_t)tw * th, -1);
    out->clear();
    for (size_t i = 0; i < list.size(); i++) {
        const uint32_t tx = tile_x0(list[i]) / 16u, ty = tile_y0(list[i]) / 16u;
        if (tx >= tw || ty >= th || index[(size_t)ty * tw + tx] >= 0) return (void)(*out = list);  // (not a tile list of this frame: as it is)
        index[(size_t)ty * tw + tx] = (int32_t)i;
    }
    out->reserve(list.size());
    for (uint32_t ty0 = 0; ty0 < th; ty0 += 4u)
        for (uint32_t j = 0; j < 4u * gx; j++) {
            const uint32_t tx = 2u * (j >> 3) + (j & 1u), ty = ty0 + ((j & 7u) >> 1);
            if (tx < tw && ty < th && index[(size_t)ty * tw + tx] >= 0) out->push_back(list[(size_t)index[(size_t)ty * tw + tx]]);
        }
}
// ... and its later frames: the tiles by the longest of their four waves' costs in the frame before (ticks: [4 list.size()], in
// the order of `list`), longest first, equal ones in list order.
inline void order_tile_list(const std::vector<uint32_t>& list, const uint32_t* ticks, uint32_t width, uint32_t rows, std::vector<uint32_t>* out) {
    refine_block_list(list, ticks, width, rows, 1.0, INFINITY, 0.0, out);
}

// The packed work counter's capacity (rtc_kernel_core.h Counters).  A kernel of up to RTC_STACK_DEPTH_BASE levels counts, per lane,
// its shade points in bits 0..11 of one word and the shadow rays it answered without a test in bits 12..31: 2^20 - 1 of them at the
// most, one more carries out of the word and the frame's culled_shadow_rays loses 2^20.  A lane adds at most the light's cell
// count per shade point, so the count is exact while cells x (shade points a lane can make in the launch) <= 2^20 - 1.  A launch
// for which that does not hold runs with the whole-light cull and the block cones switched off in its copy of the scene's
// header (rtc_device.hip launch_hdr): every sample is traced, the image is the same (each switch has its on / off tests) and
// culled_shadow_rays is honestly 0.  Kernels with a longer stack count in a word of their own and are never limited.
// (This rule is what holds.  The comment at Counters still speaks of "<= 255 shade points, <= 255 x 128 cells", which nothing ever
// enforced and which is wrong twice -- depth 8 shades up to 511 points a ray, 8 blocks per workgroup make that 4 088 a lane.  It
// is left as it is for now: the compiled kernel depends on the TEXT of rtc_kernel_core.h, comments included, so touching it would
// change every scene kernel's id for no change in code.  LABNOTES.md "Light grids".)
constexpr uint64_t CULLED_COUNT_MAX = (1ull << 20) - 1ull;
constexpr uint64_t SHADED_COUNT_MAX = (1ull << 12) - 1ull;  // what bits 0..11 hold: no launch lets a lane make more shade points
// The shade points of one ray traced at `depth` (world.rs:121-162: a child is traced while remaining >= 1, so levels depth, depth - 1,
// ... 0 shade): one where no material reflects or transmits, a chain where only one of the two occurs in the scene, a full binary tree
// otherwise.
inline uint64_t shade_points_per_ray(int32_t depth, bool any_refl, bool any_refr) {
    const uint32_t levels = (uint32_t)std::min(std::max(depth, 0), RTC_STACK_DEPTH_BASE) + 1u;
    if (!any_refl && !any_refr) return 1ull;
    if (any_refl != any_refr) return levels;
    return (1ull << levels) - 1ull;
}
// `rays_per_lane`: how many rays a lane of the launch traces into one counter (blocks per workgroup; 1 for ray streams)
inline bool culled_count_fits(int64_t cells, int32_t depth, bool any_refl, bool any_refr, uint32_t rays_per_lane) {
    const uint64_t points = std::min(SHADED_COUNT_MAX, shade_points_per_ray(depth, any_refl, any_refr) * std::max(1u, rays_per_lane));
    return cells >= 0 && (uint64_t)cells <= CULLED_COUNT_MAX / points;
}

// What RenderArgs and the launch need to know of a frame's geometry.  `shape` says which of the mutually exclusive ways
// of launching was chosen; the regular grid alone can be swizzled, re-ordered by the grid feedback or cut into progress
// chunks, and only while it is the plain one (plain_grid()).
struct LaunchPlan {
    enum Shape { GRID, BLOCK_LIST, SCENE_TILES, SCENE_RECT } shape = GRID;
    uint32_t grid_x = 0u, grid_y = 0u;
    uint32_t block_h = 16u;                 // pixel rows of a block of the regular grid
    uint32_t blocks_y = 1u;                 // blocks per workgroup (RenderArgs::blocks_y)
    uint32_t block_x0 = 0u, block_y0 = 0u;  // SCENE_RECT: the launched blocks' origin, in blocks
    bool swizzle = false;
    uint32_t fill_wg_rows = 0u, fill_rows = 0u, fill_period = 1u, fill_rect[4] = {0u, 0u, 0u, 0u};  // SCENE_RECT: the zero-filling workgroups
    unsigned long long extra_rays = 0ull;  // the pixels no workgroup is launched for: one ray each that sees nothing
    uint32_t chunk_block_rows = 1u, n_chunks = 0u;  // progress chunks (n_chunks == 0: this launch does not report)

    bool plain_grid() const { return shape == GRID && blocks_y == 1u; }
    void run_list(size_t n_blocks) { shape = BLOCK_LIST, grid_x = (uint32_t)n_blocks, grid_y = 1u, swizzle = false; }
    // scene tiles: one workgroup per listed tile; the pixels of the other tiles (`unlaunched`) are one ray each
    void run_scene_tiles(size_t n_tiles, unsigned long long unlaunched) { shape = SCENE_TILES, grid_x = (uint32_t)n_tiles, grid_y = 1u, blocks_y = 1u, extra_rays = unlaunched; }
    // the plain regular grid: blocks permuted within four rows (RenderArgs::swizzle), the grid padded to what that needs --
    // workgroups of the padding find no pixel of theirs inside the image
    void pad_for_swizzle() { swizzle = true, grid_x = (grid_x + 1u) & ~1u, grid_y = (grid_y + 3u) & ~3u; }
    size_t n_workgroups() const { return (size_t)grid_x * grid_y; }
    size_t progress_words(uint32_t stride) const { return ((size_t)grid_y + n_chunks) * stride; }
};

// The regular grid of blocks of 2^share_log2 lanes per pixel.  Frames of very many very short waves get several blocks per
// workgroup -- where the kernel was compiled to loop over them (`can_loop`); blocks_y_override: 1..8, or 0 for the library's choice.
inline LaunchPlan plan_grid(uint32_t width, uint32_t rows, uint32_t share_log2, bool can_loop, uint32_t blocks_y_override) {
    const uint32_t bw = 16u >> (share_log2 >> 1), bh = 16u >> ((share_log2 + 1u) >> 1);  // pixels per workgroup (2x2 wave tiles)
    LaunchPlan p;
    p.block_h = bh;
    p.grid_x = (width + bw - 1) / bw, p.grid_y = (rows + bh - 1) / bh;
    if (!can_loop) {
        // (only kernels compiled for it loop over blocks)
    } else if (blocks_y_override != 0u) {
        p.blocks_y = blocks_y_override;
    } else if ((uint64_t)p.grid_x * p.grid_y >= (1u << 15)) {
        // most workgroups see nothing but the sky: C5 8192^2 0.51 -> 0.43 ms, single_sphere 4096^2 0.088 -> 0.061 ms.  (Where the
        // waves have work -- hexagons, grouped_grid, whose boxes fill the frame -- four blocks per workgroup cost 8 ... 17 %.)
        p.blocks_y = 4u;
    }
    p.grid_y = (p.grid_y + p.blocks_y - 1) / p.blocks_y;
    return p;
}

// Scene rectangle (`rect`: 16 x 16 tiles [x0, x1) x [y0, y1) outside which no primary ray sees anything): the kernel is
// launched over the rectangle's blocks only, preceded by workgroups that zero-fill the rest at memory speed while the
// others render; the rays of the pixels outside are added to the count.  blocks_y: what a workgroup of this launch
// loops over (every one of them has work: callers pass 1 unless told otherwise -- C5 0.395 / 0.407 / 0.427 / 0.46 ms
// with 1 / 2 / 4 / 8 blocks per workgroup).  out_u8: a frame of bytes is zeroed by the caller's memset in front of
// the launch (the kernel's filling workgroups write f32 rows): no fill workgroups.
// partition_traced: traced_pixels() of the partition.
inline void plan_rect_launch(LaunchPlan* p, uint32_t width, uint32_t height, const Partition& q, uint32_t rows, uint64_t partition_traced,
                             const uint32_t rect[4], uint32_t blocks_y, bool out_u8, uint32_t fill_wgs_override) {
    // local rows of this partition whose global row lies in the rectangle's rows
    const uint32_t gy0 = rect[2] * 16u, gy1 = std::min(height, rect[3] * 16u);
    uint32_t yl0 = rows, yl1 = 0u;
    for_each_band(height, q, [&](uint32_t y0, uint32_t y1, uint32_t local0) {
        const uint32_t lo = std::max(y0, gy0), hi = std::min(y1, gy1);
        if (lo < hi) yl0 = std::min(yl0, local0 + (lo - y0)), yl1 = std::max(yl1, local0 + (hi - y0));
    });
    p->shape = LaunchPlan::SCENE_RECT;
    p->block_x0 = rect[0];
    if (yl0 < yl1) {
        p->block_y0 = yl0 / 16u;
        const uint32_t block_rows = (yl1 - p->block_y0 * 16u + 15u) / 16u;
        p->blocks_y = blocks_y;
        p->grid_x = rect[1] - rect[0], p->grid_y = (block_rows + blocks_y - 1u) / blocks_y;
    } else {  // none of this partition's rows: one block of the rectangle's columns, for the launch's bookkeeping
        p->block_y0 = 0u;
        p->blocks_y = 1u;
        p->grid_x = p->grid_y = 1u;
    }
    // traced pixels (x < w - 1, y < h - 1) inside the launched blocks
    const uint32_t lx0 = p->block_x0 * 16u, lx1 = std::min(width - 1u, (p->block_x0 + p->grid_x) * 16u);
    const uint32_t ly0 = p->block_y0 * 16u, ly1 = std::min(rows, (p->block_y0 + p->grid_y * p->blocks_y) * 16u);
    p->extra_rays = partition_traced - traced_rows(height, q, ly0, ly1) * (uint64_t)(lx1 > lx0 ? lx1 - lx0 : 0u);
    // what the launched blocks do not cover is zero-filled by the launch's first workgroups (the kernel's fill_outside):
    // about a thousand of them, a share of the rows each
    p->fill_rect[0] = p->block_x0 * 16u, p->fill_rect[1] = std::min(width, (p->block_x0 + p->grid_x) * 16u);
    p->fill_rect[2] = ly0, p->fill_rect[3] = ly1;
    if (out_u8) return;
    // about 160 KB of zeros per workgroup -- C5 (805 MB): 0.350 / 0.329 / 0.313 / 0.329 ms with 256 / 2048 / 4096 / 16384 of
    // them; a frame of 4096 blocks must not get as many again (fill_wgs_override: development)
    const uint64_t frame_bytes = (uint64_t)rows * width * 12u;
    uint32_t fill_wgs = (uint32_t)std::min<uint64_t>(4096u, std::max<uint64_t>(16u, frame_bytes / (160u << 10)));
    if (fill_wgs_override != 0u) fill_wgs = fill_wgs_override;
    p->fill_wg_rows = std::max(1u, (fill_wgs + p->grid_x - 1u) / p->grid_x);
    p->fill_rows = (rows + p->fill_wg_rows * p->grid_x - 1u) / (p->fill_wg_rows * p->grid_x);
    p->fill_period = std::max(1u, (p->grid_y + p->fill_wg_rows) / p->fill_wg_rows);  // spread among the rendering rows: the fill shares the memory system with them
    p->grid_y += p->fill_wg_rows;
}

// progress reporting: the plain regular grid's block rows in at most `want_chunks` chunks (max_chunks: the words there are)
inline void plan_chunks(LaunchPlan* p, uint32_t want_chunks, uint32_t max_chunks) {
    const uint32_t want = std::max(1u, std::min(want_chunks, max_chunks));
    p->chunk_block_rows = (p->grid_y + want - 1u) / want;
    if (p->swizzle) p->chunk_block_rows = (p->chunk_block_rows + 3u) & ~3u;  // (block rows finish four at a time)
    p->n_chunks = (p->grid_y + p->chunk_block_rows - 1u) / p->chunk_block_rows;
}
// ... and what a chunk is to the caller of a supersampled launch (rtc_render_ss), whose buffer holds OUTPUT rows: the plan is the
// fine frame's, a chunk is chunk_block_rows blocks of block_h fine rows, k fine rows make an output row.  block_h is 16, 8 or 4
// and never below k -- the lanes per pixel are capped by ss_max_share_log2(k): k = 4 stops at 8 x 4 tiles, blocks of 8 rows -- so
// the division is exact and a chunk ends between two output rows.  false: it would not be (the caller asserts; k = 1: as it is).
inline bool chunk_output_rows(const LaunchPlan& p, uint32_t k, uint32_t* out_rows) {
    *out_rows = 0u;
    if (k == 0u) return false;
    const uint64_t fine = (uint64_t)p.chunk_block_rows * p.block_h;
    *out_rows = (uint32_t)(fine / k);
    return fine % k == 0u && fine / k <= 0xffffffffull;
}
// The progress chunks of a supersampled partition of `out_rows` rows of `out_width` output pixels, as ctx_render_slot plans them
// for the plain regular grid (tests/test_seam_supersample_boundary.py through rtc_diag_ss_chunks): the fine grid at
// min(share_log2, cap) lanes per pixel, padded where it is swizzled, cut by plan_chunks.
inline LaunchPlan plan_ss_chunks(uint32_t out_width, uint32_t out_rows, uint32_t k, uint32_t share_log2, bool swizzle, uint32_t want_chunks,
                                 uint32_t max_chunks) {
    LaunchPlan p = plan_grid(out_width * std::max(k, 1u), out_rows * std::max(k, 1u), std::min(share_log2, ss_max_share_log2(k)), false, 0u);
    if (swizzle) p.pad_for_swizzle();
    plan_chunks(&p, want_chunks, max_chunks);
    return p;
}

}  // namespace rtc

#endif
