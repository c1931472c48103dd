// rtc_device.hip -- the MI355X (gfx950 / CDNA4) render path of librtc_amd.so.
//
// This translation unit holds the HOST side of the device path: the persistent context, kernel
// launches, the batched test entry points and the device part of the scene-specialising JIT
// (compile, load, remember).  Scene validation, flattening and the choice of a scene's kernels are
// rtc_scene_prep.h, what a compile is made of and the disk cache's entries rtc_jit.h, how a launch
// is cut rtc_launch_plan.h (all host-only); the device code itself lives in rtc_kernel_core.h
// (shared with the hiprtc compile).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <unistd.h>

#include <chrono>

#include <algorithm>
#include <array>
#include <functional>
#include <queue>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <set>
#include <vector>

#include "rtc_internal.h"
#include "rtc_owned.h"
#include "rtc_launch_plan.h"
#include "rtc_kernel_core.h"
#include "rtc_hits.h"
#include "rtc_supersample.h"
#include "rtc_lens.h"
#include "rtc_lens_seam.h"
#include "rtc_trace.h"
#include "rtc_adaptive.h"
#include "rtc_adaptive_seam.h"
#include "rtc_reorder.h"
#include "rtc_wavefront.h"
#include "rtc_scene_prep.h"

namespace rtc {

// Host copies of the same tables (rtc_powf_host, used by CPU tests to pin the
// restatement against the C library without a GPU).
static const PowLog2Entry h_pow_log2_tab[16] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2},
};
static const uint64_t h_exp2f_tab[32] = {
    0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51, 0x3fef72b83c7d517b,
    0x3fef54873168b9aa, 0x3fef387a6e756238, 0x3fef1e9df51fdee1, 0x3fef06fe0a31b715, 0x3feef1a7373aa9cb,
    0x3feedea64c123422, 0x3feece086061892d, 0x3feebfdad5362a27, 0x3feeb42b569d4f82, 0x3feeab07dd485429,
    0x3feea47eb03a5585, 0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13,
    0x3feeace5422aa0db, 0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d, 0x3feee89f995ad3ad,
    0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069, 0x3fef5818dcfba487, 0x3fef7c97337b9b5f,
    0x3fefa4afa2a490da, 0x3fefd0765b6e4540,
};
static const SinCosTab h_sincosf_tab[2] = RTC_SINCOSF_TAB_INIT;
static const uint32_t h_inv_pio4[24] = RTC_INV_PIO4_INIT;

// ============================================================================
//  Host side of the device path
// ============================================================================
#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(RTC_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static int usable_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static rtc_status select_device(int32_t device) {
    int nd = usable_devices();
    if (nd <= 0) return fail(RTC_ERR_NO_DEVICE, "no HIP device visible; librtc_amd has no CPU fallback");
    if (device < 0 || device >= nd) return fail(RTC_ERR_INVALID_ARG, "device %d out of range (have %d)", device, nd);
    HIP_TRY(hipSetDevice(device));
    return RTC_OK;
}

}  // namespace rtc

using namespace rtc;

namespace {  // (the context's parts: this file's alone)
struct BlockList {  // RenderArgs::tiles of one partition (build_block_list), resident on the device
    DeviceArray<uint32_t> d;     // grown, never shrunk (hipMalloc / hipFree cost the animation's frames milliseconds)
    size_t n = 0, n_listed = 0;  // (n_listed: a grid's list leaves the padding out)
    // feedback (refine_block_list): the list as built, where its first launch leaves its waves' running times, and how far it is
    std::vector<uint32_t> host;
    DeviceArray<uint32_t> d_ticks;  // [4 n] wave times -- or, for kernels that do not time their waves, [4 n] uint4 work counts (a copy of block_counts)
    bool counts = false, swizzled = false, listed = false;  // (listed: a grid whose frames run from `d`, its blocks in order)
    // IDLE (regular grids): a scene's first frame -- nothing is measured before a second frame of the SAME scene shows that frames repeat
    enum { FRESH, TIMED, REFINED, IDLE } state = FRESH;
    uint32_t passes = 0;  // refinements so far
    // Scenes that change (restart_block_lists): once a scene has changed under a refined list, every frame from it leaves its waves'
    // times and is bracketed by the list's own events; what the frames since the last re-cut took beyond the best of them adds up
    // (loss_ms), and when that reaches what a re-cut costs the host (recut_host_ms, measured) the next frame re-cuts the list from
    // the times of the frame before it -- at the latest after sixteen scenes.
    uint32_t scene_changes = 0;
    bool animated = false, ev_recorded = false;
    Event ev0, ev1;
    double best_ms = 0.0, loss_ms = 0.0, recut_host_ms = 0.5;
};
// Scene tiles: the 16 x 16 tiles in which a primary ray can see anything (ScenePlan::scene_tile_mask) -- those some bounded entry's
// padded box projects to (C5: 64 spheres, 7 % of 8192^2) and the near side of every top-level plane's horizon (C3: two thirds of the
// frame).  Frames of such a scene are a zero-fill of the other tiles and one workgroup per listed tile (ctx_render_slot).
struct SceneTileList {
    DeviceArray<uint32_t> d;
    size_t n = 0;
    unsigned long long traced_pixels = 0ull;  // traced pixels (x < w - 1, y < h - 1) inside the listed tiles
    DeviceArray<uint2> d_fill;  // the runs of tiles that are NOT listed, at most 64 tiles each: {x0 | n << 16, local row} (fill_tiles_kernel)
    size_t n_fill = 0;
    // feedback (order_scene_tiles): the list as launched, and where its first frame leaves its waves' work counts ([4 n] uint4, a
    // copy of block_counts).  IDLE: a scene's first frame -- as for a regular grid, nothing is measured (or allocated) before a
    // second frame of the same scene shows that frames repeat; FRESH: the next frame leaves its counts; TIMED: they are on the
    // device; SETTLED: ordered, or left as it is
    std::vector<uint32_t> host;
    DeviceArray<uint4> d_counts;
    enum { IDLE, FRESH, TIMED, SETTLED } state = IDLE;
    bool ordered = false;  // SETTLED, and the list was re-ordered
};
// One kernel of the resident scene as the context keeps it -- the frame's, the ray streams', the refinement's of one factor:
// what rtc_scene_prep.h planned for it, the scene-compiled kernel (scene_kernel_for) and, for recursion deeper than
// RTC_STACK_DEPTH_BASE, the same kernel compiled once more with a longer frame stack on first use (deep_kernel).
struct SceneKernel {
    KernelVariant variant;        // options (written down whatever the policy says: deep_kernel may need them) and the two names
    hipFunction_t fn = nullptr;   // scene-specialised kernel (hiprtc), or null: the ahead-of-time family
    std::string fn_id;
    std::map<int, std::pair<hipFunction_t, std::string>> deep;  // by stack depth: the kernel and its id
    bool failed = false;          // hiprtc did not deliver fn: the ahead-of-time family from then on (note says why)
    std::string note;
};
// ... and what outlives the scene beside it: the (kernel, stream) pairs launched once (warm_up).  One set per slot:
// KernelFamily::key() is one value for the render and the ray-stream kernel of a family.
typedef std::set<std::pair<const void*, const void*>> Warmed;
typedef std::vector<std::pair<Event, Event>> EventPairs;
}  // namespace

// The context.  Its fields are two groups, and which group a field is in says how long it lives:
//
// (a) `scene`, the resident scene: replaced WHOLE, by one assignment, when rtc_ctx_set_scene* takes another scene, camera, factor
//     or lens, and filled from the new plan.  `ready` is false from that assignment until the new scene is fully resident, and again
//     when its kernel could not be compiled under RTC_AMD_SPECIALIZE=1.  Setting the very scene that is resident replaces nothing
//     (a focus pull writes `lens`, a deferred compile `render` and the names).
//       hdr, camera, ss_k, lens_mode, lens, stream_guard          what the launches take
//       plan                                                      ScenePlan as plan_scene / plan_supersampled / plan_lens left it
//                                                                 (spec_shares is cleared in it when the compile fails)
//       render, kernel_name, kernel_id, jit_deferred              the frame's kernel slot and what is reported of it
//       wf_disabled                                               a frame of this scene overflowed the level-by-level pools
//       trace.{kernel, name, id, last}                            the ray streams' slot, the last trace's names, "the last launch was
//                                                                 a trace" (a new scene reports renders again)
//       adaptive.{kernel[2], failed, note, name, id}              the refinement's slots and names
//       adaptive_seam.{kernel[3], failed, note, name, id, halo_*} ... and the one-call seam's
//
// (b) everything else, kept for the context's life.  Set once: device, policy, n_cus, lazy_jit, seam_kernels, reorder.dir_major.
//     Grow-only memory and lazily made events and streams (rtc_owned.h), freed by the destructor: every d_* array, h_feedback, the
//     event pairs, fill_stream, ev_fork / ev_join, the refinement's and the reordering's ev[].
//     The records' host mirror (soa_host, texels_host) lives with d_soa / d_texels: a camera-only change keeps all four.
//     Bookkeeping about the PROCESS, not the scene: the warmed sets (code objects launched once per queue), wgs_per_cu (occupancy of a
//     code object).
//     The lists: block_lists survive a scene of the same frame, factor and mode under restart_block_lists' rule and are dropped
//     otherwise; scene_tile_lists are dropped by every scene; both are dropped when a deferred compile delivers the scene's kernel.
//     And the record of the last launches, which a new scene does NOT reset -- each is written by the call it describes and read by
//     the statistics, whatever scene has been set in between (tests/test_gpu_ctx_lifetime.py pins what they report):
//       tree_waves        the last TREE scene's waves per SIMD: recut_block_list reads it for the area-light lists of flat scenes too
//       rendered, events_used, last_rows, last_pixels, last_share_log2, wf_last
//                         rtc_ctx_stats / rtc_ctx_kernel_name / rtc_diag_ctx_share_log2 after a set_scene still report the frame before
//       trace.last_n, trace.events_used
//                         likewise for the traces (trace.last itself is the scene's)
//       adaptive.ran, adaptive_seam.ran, adaptive_seam.halo_pixels, reorder.ran, reorder.last_n
//                         rtc_ctx_adaptive_stats / rtc_ctx_reorder_stats after a set_scene report the last call under the scene before
struct rtc_ctx {
    // ---- (a) the resident scene
    struct Scene {
        bool ready = false;  // fully resident: the render paths may use it
        SceneHdr hdr = {};
        rtc_camera camera = {};  // as rtc_ctx_set_scene took it
        // Supersampling (rtc_ctx_set_scene_ss; rtc_supersample.h): 1, or k = 2 / 4 -- `hdr` is then the FINE camera's, and everything that
        // plans, schedules and feeds back does so in fine space; only the canvas and rtc_stats.rows speak of the output frame
        uint32_t ss_k = 1u;
        // A thin lens (rtc_ctx_set_scene_lens; rtc_lens.h): the context is a supersampled one in every respect but its kernel -- the
        // lens kernel of the same factor -- and the three words that kernel takes; a focus pull replaces the words and nothing else
        bool lens_mode = false;
        rtc_lens lens = {0.0f, 1.0f, 0u};
        // Ray streams on a flat world with a hierarchy of the library's own (rtc_trace.h StreamGuard, ERROR_BUDGET.md B9): what tells a
        // ray that needs the entry list with every box opened (d_open_trav); open_trav is null for every other scene
        StreamGuard stream_guard = {nullptr, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
        // Which kernel renders the scene and how its frames are cut (rtc_scene_prep.h): the block-list bitmap (heavy_tiles), the scene
        // box's coverage, the scene rectangle, the scene-tile mask, what the scene's kernel was compiled with (spec_*)
        ScenePlan plan;
        SceneKernel render;               // compiled by rtc_ctx_set_scene (or deferred: lazy_jit); note: rtc_ctx_jit_status
        std::string kernel_name;          // what rtc_ctx_render launches, for rtc_ctx_kernel_name()
        std::string kernel_id;            // rtc_ctx_kernel_id(): names the code object (source + options + compiler), not the scene
        bool jit_deferred = false;  // the kernel was left uncompiled by the scene's first sighting: the next render of this scene compiles it
        bool wf_disabled = false;   // a frame overflowed the level-by-level renderer's pools: per-pixel kernels from then on
        struct Trace {
            SceneKernel kernel;    // trace_variant's, compiled by the first trace that asks for it
            std::string name, id;  // of the last trace's kernel ("" before the first trace of the current scene)
            bool last = false;     // the context's last launch was a trace: rtc_ctx_stats reports it
        } trace;
        struct Refine {
            bool failed = false;   // hiprtc did not deliver one of the path's kernels: the ahead-of-time ones from then on, for all (note says why)
            std::string note;
            std::string name, id;  // of the last call's refinement kernel ("" before the first of the current scene)
        };
        struct Adaptive : Refine {
            SceneKernel kernel[2];  // refine_variant's of k = 2, 4, compiled by the first call that asks for it
        } adaptive;
        struct AdaptiveSeam : Refine {
            SceneKernel kernel[3];           // seam_refine_variant's of k = 1 (the halo pass), 2, 4
            std::string halo_name, halo_id;  // of the last call's halo pass ("": the last call had no halo row)
        } adaptive_seam;
    } scene;

    // ---- (b) kept for life
    int device = 0;
    Policy policy;  // the environment's switches as they were when the context was created
    int n_cus = 0;  // compute_units()
    bool lazy_jit = false;      // a context of the one-call seam (rtc::ctx_mark_one_shot): see jit_get
    // ... and what else such a context is: supersampled, its kernels are the variant that stores bytes and reports its rows
    // (rtc_supersample.h SEAM: ss_seam_render_kernel<...>, -DRTC_SPEC_SS_SEAM=1; with a lens rtc_lens_seam.h: lens_seam_render_kernel<...>,
    // -DRTC_SPEC_LENS_SEAM=1), and ctx_render_slot accepts out_u8 / progress
    bool seam_kernels = false;
    // the records on the device, and as last uploaded: an identical scene (rtc_render_ex called again for the next frame) is not uploaded twice
    DeviceArray<float4> d_soa;
    DeviceArray<float> d_texels;        // UVImage canvases (RGB f32)
    DeviceArray<float4> d_open_trav;    // Scene::stream_guard's entry list
    std::vector<float4> soa_host;
    std::vector<float> texels_host;
    Warmed render_warmed;
    int tree_waves = 6;  // waves per SIMD the last tree scene's kernel was compiled for (a flat scene leaves it: see above)
    // Block lists (RenderArgs::tiles) -- key: band_rows, n_parts, part, lanes per pixel (log2; ~0: a regular grid's order), depth (what
    // a block costs depends on it) -- and scene-tile lists per partition {band_rows, n_parts, part}
    std::map<std::array<uint32_t, 5>, BlockList> block_lists;
    std::map<std::array<uint32_t, 3>, SceneTileList> scene_tile_lists;
    Stream fill_stream;  // the zero-fill of a tile launch runs beside the render kernel (fork / join by events)
    Event ev_fork, ev_join;
    DeviceArray<uint4> d_block_counts;
    // pinned host memory through which the feedback reads wave times back and sends lists out (through pageable vectors the two
    // copies of a 2048^2 frame's re-cut took longer than the frame)
    PinnedBuffer h_feedback;
    // workspace of rtc_ctx_to_ppm
    DeviceArray<unsigned long long> d_ppm_rows;  // per-row length, then offset; [h] is the total
    DeviceArray<uint32_t> d_ppm_bits;
    // the level-by-level renderer (rtc_wavefront.h): ray lists (two levels x reflection / refraction, one capacity), the node pool, counters
    DeviceArray<WfRay> d_wf_rays[4];
    DeviceArray<WfNode> d_wf_nodes;
    DeviceArray<uint32_t> d_wf_ctr;
    bool wf_last = false;      // the last frame was rendered level by level (rtc_ctx_kernel_name says so)
    std::string wf_name;
    DeviceArray<uint32_t> d_progress;  // RenderArgs::progress counters (rtc_render_ex)
    // {rays, shaded hits, culled shadow rays} per counter slot: slot 0 = the last rtc_ctx_render launch; rtc_render_ex
    // renders a frame in several launches (row chunks in flight while earlier ones travel) and gives each its own
    DeviceArray<unsigned long long> d_total;
    // HIP-event pairs around the render kernel, one per launch since the last rtc_ctx_stats
    EventPairs events;
    size_t events_used = 0;
    bool rendered = false;
    uint32_t last_rows = 0;
    uint32_t last_share_log2 = 0;  // lanes per pixel (log2) the last launch was planned with (rtc_diag_ctx_share_log2)
    uint64_t last_pixels = 0;
    // Ray streams (rtc_ctx_trace; rtc_trace.h).  Everything a trace needs it has of its own -- kernel, names, counters, events,
    // warm-up bookkeeping -- so that the frame schedule and what rtc_ctx_render reports never see it.
    struct Trace {
        Warmed warmed;
        DeviceArray<uint4> d_counts;              // one partial per wave
        DeviceArray<unsigned long long> d_total;  // {rays, shaded hits, culled shadow rays} of the last trace
        EventPairs events;                        // around the trace kernels since the last rtc_ctx_stats that reported a trace
        size_t events_used = 0;
        uint64_t last_n = 0;
    } trace;
    // What the two refinement paths keep: the mask and the refinement have everything of their own, as a trace has, so that the
    // frame schedule and rtc_ctx_stats never see them.
    struct Refine {
        DeviceArray<uint32_t> d_list;        // flagged pixel indices (the seam's: of the share, share-local)
        DeviceArray<AdaptiveQueue> d_queue;  // the list's length and the last refinement's {rays, shaded hits, culled shadow rays}; the seam's [2]: ... and the halo pass's
        Event ev[3];                         // before the mask kernel (the seam's: the halo pass), between the two, after the refinement
        bool ran = false;                    // the events have been recorded
        std::map<const void*, int> wgs_per_cu;  // occupancy of a refinement kernel, asked once
    };
    // Adaptive supersampling (rtc_ctx_render_adaptive; rtc_adaptive.h).  The base frame is the context's normal render.
    struct Adaptive : Refine {
        Warmed warmed[2];  // by Scene::Adaptive::kernel
    } adaptive;
    // Adaptive supersampling of the one-call seam (rtc_render_adaptive; rtc_adaptive_seam.h): one part's halo pass, banded mask and
    // refinement behind a base pass that is ctx_render_slot's.
    struct AdaptiveSeam : Refine {
        Warmed warmed[3];
        DeviceArray<float> d_halo;    // [halo rows][W][3]
        DeviceArray<uint8_t> d_mask;  // [rows][W]
        uint64_t halo_pixels = 0;     // of the last call: halo rows x W
    } adaptive_seam;
    // Ray reordering (rtc_ctx_ray_order, rtc_ctx_trace_reordered; rtc_reorder.h).  The sort's and the gather's buffers, events of
    // its own; the trace in the middle is rtc_ctx_trace's and is reported as one.
    struct Reorder {
        bool dir_major = !REORDER_ORIGIN_MAJOR;  // RTC_AMD_REORDER_DIR_MAJOR (development): the direction in the key's top bits
        DeviceArray<uint8_t> d_scratch;  // bytes: sort ping-pong (16 B a ray; the colours reuse 12 of them) + gathered rays and keys (36 B a ray)
        DeviceArray<uint32_t> d_table;   // the sort's [digit][workgroup] table, then the stream box (REORDER_TABLE_WORDS, allocated once)
        Event ev[6];                     // around keys + box, sort, gather, trace, scatter
        bool ran = false;                // the events have been recorded (by a reordered trace)
        uint64_t last_n = 0;
    } reorder;
};

// A new scene of the same frame size (an animation: the camera or an object has moved): what a tile cost in the frame before is
// still the best guess for what it costs now, and any list is a valid tiling for any scene.  The lists that cut tiles into lanes
// (divided meshes, lane-sharing area lights) stay, and from then on every frame from a refined list leaves its waves' times and is
// bracketed by the list's own events: what the frames since the last re-cut took beyond the best of them adds up, and when that
// reaches what a re-cut costs the host (a read-back, a sort, an upload: 0.2 - 0.5 ms, measured) the next frame starts with a re-cut
// from the times of the frame before it -- rent until the rent equals the price.  Lists age at their own pace (mesh 2048^2, a
// quarter of a degree per frame: 0.1 - 0.3 ms per frame, re-cut every 2 - 9 scenes, kernel 3.85 -> 2.97 ms; soft_shadows 2048^2:
// hardly, every sixteenth -- the cap); a fixed period was wrong for one or the other (every eighth: mesh 3.57 with frames of 5).  A list whose timed frame belonged to the old scene is re-cut from that: it is the frame before.  A regular grid's
// ORDER does not survive: a stale order was slightly worse than the permuted image order (reflect_refract 0.839 -> 0.860 ms).
static void restart_block_lists(rtc_ctx* c) {
    for (auto it = c->block_lists.begin(); it != c->block_lists.end();) {
        BlockList& bl = it->second;
        if (it->first[3] == 0xffffffffu) {  // (its buffers stay for the next scene that repeats)
            bl.state = BlockList::IDLE;
            bl.listed = false;
            ++it;
            continue;
        }
        if (bl.state == BlockList::REFINED) {
            bl.animated = true;
            bool recut = ++bl.scene_changes >= 16u, timed = false;
            if (bl.ev_recorded) {  // the frame before ran from this list (rtc_ctx_set_scene has waited for it)
                bl.ev_recorded = false;
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, bl.ev0, bl.ev1) == hipSuccess && ms > 0.0f) {
                    timed = true;
                    if (bl.best_ms == 0.0 || ms < bl.best_ms) bl.best_ms = ms;
                    bl.loss_ms += ms - bl.best_ms;
                    if (bl.loss_ms >= bl.recut_host_ms) recut = true;
                }
            }
            if (recut) {
                bl.scene_changes = 0u;
                bl.best_ms = bl.loss_ms = 0.0;
                // (timed: that frame's times are on the device -- the next frame starts with the re-cut; else it is timed first)
                bl.state = timed ? BlockList::TIMED : BlockList::FRESH;
                bl.passes = c->policy.feedback_passes ? c->policy.feedback_passes - 1u : 0u;
            }
        }
        ++it;
    }
}
// ============================================================================
//  Scene-specialised kernels (hiprtc)
//
//  The generic kernels decide each object's shape kind and flags with wave-uniform branches inside the
//  unrolled object loops.  For a given scene those words are constants, so rtc_ctx_set_scene compiles
//  rtc_kernel_core.h once more with them baked in (-DRTC_SPEC_LIST=...): no kind switches, dead
//  shape code removed, tighter scheduling -- C3 4.06 -> 3.13 ms with bit-identical output.  Only the
//  scene's *shape* (object count, kinds, flags, light kind, jitter mode) is specialised; all values
//  stay run-time data.  Compiled code is cached in-process and on disk (<lib dir>/jit_cache/);
//  options, key, cache file name and the cache's entries are rtc_jit.h's (host-only).
//  Policy: RTC_AMD_SPECIALIZE=0 never, =1 always; default: scenes of <= 8 objects rendered at >= 2^18
//  pixels (a 0.7 s compile is not worth it for thumbnails; the AOT kernels produce the same bits).
// ============================================================================
namespace {

struct JitModule {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    std::string id;  // "spec_<hash of source, options, compiler version>.<checksum of the code object>": names the code that runs (rtc_ctx_kernel_id)
};
std::mutex g_jit_mutex;
std::map<std::string, JitModule> g_jit_cache;  // key: "<device>|<defines>"

std::string lib_dir() {
    Dl_info info;
    if (dladdr((const void*)&rtc_abi_version, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        size_t k = p.find_last_of('/');
        return k == std::string::npos ? std::string(".") : p.substr(0, k);
    }
    return ".";
}

// The kernel source travels inside the library: rtc_kernel_core_embed.inc is rtc_kernel_core.h as a string literal,
// written by ray_tracer_challenge_amd/build.py before every compile (under hiprtc the header needs no other file).  A
// deployment is librtc_amd.so alone -- no csrc/ or include/ beside it.  RTC_AMD_JIT_SOURCE=<path> (development) reads
// the header from disk instead, so a kernel experiment needs no rebuild of the library.
#include "rtc_kernel_core_embed.inc"

std::string jit_cache_dir(const Policy& P) {  // RTC_AMD_JIT_CACHE=<dir>, or 0 / off to keep compiled kernels in memory only; default <lib dir>/jit_cache
    if (!P.jit_cache.empty()) return (P.jit_cache == "0" || P.jit_cache == "off") ? std::string() : P.jit_cache;
    return lib_dir() + "/jit_cache";
}

// The text of the header beside the core that a kind's kernel includes ("" for the frame's own) -- the lens kernel's: of the two,
// rtc_supersample.h and then rtc_lens.h, which includes it; the seam's lens kernel's: of the three, rtc_lens_seam.h last
// (rtc_jit.h: what a hash folds in)
std::string beside_text(JitKind kind) {
    if (kind == JitKind::LENS) return std::string(k_ss_src) + k_lens_src;
    if (kind == JitKind::LENS_SEAM) return std::string(k_ss_src) + k_lens_src + k_lens_seam_src;
    if (kind == JitKind::ADAPTIVE_SEAM) return std::string(k_adaptive_src) + k_adaptive_seam_src;
    return kind == JitKind::SS ? k_ss_src : kind == JitKind::TRACE ? k_trace_src : kind == JitKind::ADAPTIVE ? k_adaptive_src : "";
}
// The sizes of the kernels' argument blocks, which a key carries
constexpr JitArgSizes k_jit_arg_sizes = {sizeof(RenderArgs), sizeof(TraceArgs), sizeof(AdaptiveRefineArgs), sizeof(LensRenderArgs), sizeof(AdaptiveSeamArgs)};
// identifies the ahead-of-time kernels of this build: the source they were compiled from
std::string aot_kernel_id(JitKind kind, uint32_t k = 1u) { return rtc::aot_kernel_id(kind, k, k_core_src, beside_text(kind)); }

// Compiles (or fetches) the specialised kernel of variant `v` on the current device: what rtc_jit.h plans, compiled by hiprtc,
// loaded and remembered.
// `lazy` (the one-call seam, rtc_render_ex: the reference renders ONE frame per process): a kernel that is neither in this process's
// memory nor in the disk cache is not compiled the first time its scene is seen -- *out stays null and the frame is rendered by the
// ahead-of-time kernel: a compile is 0.5 - 2 s, the frame it speeds up a few milliseconds (tools/first_call.py: C3's first call 693 ms
// with the compile, 121 with a filled cache, 123 ahead-of-time).  The second time the process asks for the same kernel -- frames
// repeat -- it is compiled, and cached on disk for every process after it.
std::set<std::string> g_jit_seen;
rtc_status jit_get(const Policy& P, int device, const KernelVariant& v, hipFunction_t* out, std::string* id, bool lazy = false) {
    std::string key = std::to_string(device) + "|";
    for (const auto& d : v.defs) key += d + " ";
    key += "|" + P.jit_source + "|" + P.jit_flags;  // (development builds: another source or other flags are another kernel)
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    auto it = g_jit_cache.find(key);
    if (it != g_jit_cache.end()) {
        *out = it->second.fn;
        *id = it->second.id;
        return RTC_OK;
    }
    const JitKindFacts& kind = jit_kind_facts(v.kind);
    // (`beside`: the header the kind's kernel includes; `below`: the header that one includes -- the lens kernel's rtc_supersample.h;
    // the seam's lens kernel: rtc_lens_seam.h, rtc_lens.h below it and rtc_supersample.h below that, `below2`;
    // the seam's adaptive kernels: rtc_adaptive_seam.h, rtc_adaptive.h below it)
    const bool lens_seam = v.kind == JitKind::LENS_SEAM, adaptive_seam = v.kind == JitKind::ADAPTIVE_SEAM;
    std::string core = k_core_src, beside = lens_seam ? k_lens_seam_src : adaptive_seam ? k_adaptive_seam_src : v.kind == JitKind::LENS ? k_lens_src : beside_text(v.kind);
    std::string below = lens_seam ? k_lens_src : adaptive_seam ? k_adaptive_src : *kind.header_below ? k_ss_src : "", below2 = *kind.header_below2 ? k_ss_src : "";
    if (!P.jit_source.empty()) {  // development builds only (Policy)
        if (!read_file(P.jit_source, &core)) return fail(RTC_ERR_DEVICE, "scene specialisation: cannot read the kernel source %s", P.jit_source.c_str());
        // (... and the headers beside it from the same directory, when they are there: an experiment in any of them needs no rebuild)
        const size_t slash = P.jit_source.find_last_of('/');
        const std::string dir = slash == std::string::npos ? std::string() : P.jit_source.substr(0, slash + 1);
        std::string text;
        if (*kind.header && read_file(dir + kind.header, &text)) beside = text;
        if (*kind.header_below && read_file(dir + kind.header_below, &text)) below = text;
        if (*kind.header_below2 && read_file(dir + kind.header_below2, &text)) below2 = text;
    }
    int rtc_major = 0, rtc_minor = 0;
    (void)hiprtcVersion(&rtc_major, &rtc_minor);
    const JitPlan plan = plan_jit(v.defs, v.kind, P.jit_flags, rtc_major, rtc_minor, k_jit_arg_sizes, core, below2 + below + beside);
    if (P.jit_print) {  // development: the options, one line, as tools/spec_asm.sh takes them
        std::string line;
        for (size_t i = 5; i < plan.opts.size(); i++) line += " " + plan.opts[i];
        std::fprintf(stderr, "librtc_amd: scene kernel options:%s\n", line.c_str());
    }
    const std::string cache_dir = jit_cache_dir(P), cache_path = cache_dir + "/" + plan.cache_file;
    auto compile = [&](std::string* code) -> rtc_status {
        hiprtcProgram prog;
        const char* headers[] = {core.c_str(), beside.c_str(), below.c_str(), below2.c_str()};
        const char* header_names[] = {"rtc_kernel_core.h", kind.header, kind.header_below, kind.header_below2};
        if (hiprtcCreateProgram(&prog, kind.program, "rtc_scene_spec.hip", *kind.header_below2 ? 4 : *kind.header_below ? 3 : *kind.header ? 2 : 1, headers, header_names) != HIPRTC_SUCCESS)
            return fail(RTC_ERR_DEVICE, "hiprtcCreateProgram failed");
        std::vector<const char*> copts;
        for (const auto& o : plan.opts) copts.push_back(o.c_str());
        hiprtcResult r = hiprtcCompileProgram(prog, (int)copts.size(), copts.data());
        if (r != HIPRTC_SUCCESS) {
            size_t n = 0;
            hiprtcGetProgramLogSize(prog, &n);
            std::string log(n, '\0');
            if (n) hiprtcGetProgramLog(prog, &log[0]);
            hiprtcDestroyProgram(&prog);
            return fail(RTC_ERR_DEVICE, "scene specialisation failed to compile: %s\n%.1500s", hiprtcGetErrorString(r), log.c_str());
        }
        size_t n = 0;
        hiprtcGetCodeSize(prog, &n);
        code->resize(n);
        hiprtcGetCode(prog, &(*code)[0]);
        hiprtcDestroyProgram(&prog);
        (void)publish_cache_entry(cache_dir, cache_path, *code);
        return RTC_OK;
    };
    std::string code;
    const bool cached = !cache_dir.empty() && read_cache_entry(cache_path, &code);
    if (!cached && lazy && g_jit_seen.insert(key).second) {  // (first sighting: see above)
        *out = nullptr;
        return RTC_OK;
    }
    if (!cached) RTC_TRY(compile(&code));
    JitModule m;
    hipError_t le = hipModuleLoadData(&m.mod, code.data());
    if (le == hipSuccess) le = hipModuleGetFunction(&m.fn, m.mod, plan.entry);
    if (le != hipSuccess && cached) {
        // a cached code object that does not load (truncated, or from another toolchain): drop it and compile once
        (void)hipGetLastError();
        (void)::unlink(cache_path.c_str());
        RTC_TRY(compile(&code));
        le = hipModuleLoadData(&m.mod, code.data());
        if (le == hipSuccess) le = hipModuleGetFunction(&m.fn, m.mod, plan.entry);
    }
    if (le != hipSuccess) return fail(RTC_ERR_DEVICE, "scene specialisation: the compiled kernel does not load: %s", hipGetErrorString(le));
    m.id = code_object_id(plan.cache_file, code);
    g_jit_cache[key] = m;
    *out = m.fn;
    *id = m.id;
    return RTC_OK;
}

}  // namespace

// rtc_hit_planes as the kernels take it; false: no plane requested
static bool hit_planes_view(const rtc_hit_planes* p, HitPlanes* v) {
    v->object = p->object, v->distance = p->distance, v->inside = p->inside, v->light = p->light;
    v->point = (float4*)p->point, v->eye = (float4*)p->eye, v->normal = (float4*)p->normal, v->reflectv = (float4*)p->reflectv;
    v->over_point = (float4*)p->over_point, v->under_point = (float4*)p->under_point, v->n1n2 = (float2*)p->n1n2;
    return p->object || p->distance || p->point || p->eye || p->normal || p->reflectv || p->over_point || p->under_point || p->inside || p->n1n2 || p->light;
}

static KernelFamily aot_family(const rtc_ctx* c) { return aot_family(c->scene.hdr.n_trav, c->scene.hdr.n_objects, c->scene.plan.simple); }
// f(NOBJ, SIMPLE) with the family as compile-time constants
template <class F>
static void dispatch_family(KernelFamily k, F&& f) {
    if (k.nobj < 0) f(std::integral_constant<int, -1>(), std::false_type());
    else if (k.nobj == 4 && k.simple) f(std::integral_constant<int, 4>(), std::true_type());
    else if (k.nobj == 4) f(std::integral_constant<int, 4>(), std::false_type());
    else if (k.nobj == 8 && k.simple) f(std::integral_constant<int, 8>(), std::true_type());
    else if (k.nobj == 8) f(std::integral_constant<int, 8>(), std::false_type());
    else f(std::integral_constant<int, 0>(), std::false_type());
}
// One launch of a slot's kernel (SceneKernel): `fn`, the scene-compiled one, takes `args` as its one parameter; null: `aot`
// dispatches to the ahead-of-time family.
template <class Args, class Aot>
static hipError_t launch_scene_kernel(hipFunction_t fn, dim3 grid, hipStream_t stream, Args& args, Aot&& aot) {
    if (fn) {
        void* params[] = {&args};
        return hipModuleLaunchKernel(fn, grid.x, grid.y, 1, 256, 1, 1, 0, stream, params, nullptr);
    }
    aot();
    return hipGetLastError();
}

extern "C" {

int32_t rtc_device_count(void) { return usable_devices(); }

// Diagnostic (not in rtc.h): the level-by-level renderer's counters after the context's last frame (rtc_wavefront.h: nodes,
// overflow, then per level {reflection rays, refraction rays, nodes so far}); returns the number of words written.
uint32_t rtc_ctx_wavefront_counters(rtc_ctx* c, uint32_t* out, uint32_t cap) {
    if (!c || !out || !c->d_wf_ctr) return 0u;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const uint32_t n = std::min<uint32_t>(cap, WF_CTR_WORDS);
    if (hipMemcpy(out, c->d_wf_ctr, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0u;
    return n;
}

// Diagnostic (not in rtc.h): was this library built with the development switches (Policy, -DRTC_DEV_SWITCHES)?
int32_t rtc_dev_switches(void) {
#ifdef RTC_DEV_SWITCHES
    return 1;
#else
    return 0;
#endif
}

rtc_status rtc_scene_validate(const rtc_scene* scene, const rtc_camera* camera) {
    SceneHdr hdr;
    std::vector<float4> soa;
    std::vector<float> texels;
    return flatten(Policy::from_env(), scene, camera, &hdr, &soa, &texels);
}

rtc_status rtc_ctx_create(int32_t device, rtc_ctx** out) {
    if (!out) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_create: out is NULL");
    int n = usable_devices();
    if (n <= 0) return fail(RTC_ERR_NO_DEVICE, "no HIP device visible; librtc_amd has no CPU fallback");
    if (device < 0 || device >= n) return fail(RTC_ERR_INVALID_ARG, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rtc_ctx> c(new rtc_ctx());  // (a failure below frees it, with its device current)
    c->device = device;
    c->policy = Policy::from_env();  // the one place a context looks at the environment
    if (const char* e = RTC_DEV_ENV("RTC_AMD_REORDER_DIR_MAJOR")) c->reorder.dir_major = *e && e[0] != '0';
    HIP_TRY(c->d_total.grow(3 * CTX_TOTAL_SLOTS));
    HIP_TRY(hipMemset(c->d_total, 0, 3 * CTX_TOTAL_SLOTS * sizeof(unsigned long long)));
    *out = c.release();
    return RTC_OK;
}

void rtc_ctx_destroy(rtc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);  // (rtc_owned.h: every release with the context's device current)
    delete c;
}

// ... and what the pairs in use measured, added up
static hipError_t sum_event_ms(const EventPairs& events, size_t used, double* sum_ms) {
    for (size_t i = 0; i < used; i++) {
        float ms = 0.0f;
        const hipError_t e = hipEventElapsedTime(&ms, events[i].first, events[i].second);
        if (e != hipSuccess) return e;
        *sum_ms += ms;
    }
    return hipSuccess;
}
static hipError_t sum_event_ms(const rtc_ctx* c, double* sum_ms) { return sum_event_ms(c->events, c->events_used, sum_ms); }
// the next HIP-event pair of the launches since the last rtc_ctx_stats (the renders' pairs, or the traces')
static hipError_t next_event_pair(EventPairs& events, size_t& used, std::pair<Event, Event>** out) {
    if (used == events.size()) {
        if (events.size() >= 4096) {
            used = 0;  // nobody is reading the timings: recycle
        } else {
            std::pair<Event, Event> e;
            hipError_t err = e.first.create();
            if (err == hipSuccess) err = e.second.create();
            if (err != hipSuccess) return err;
            events.push_back(std::move(e));
        }
    }
    *out = &events[used++];
    return hipSuccess;
}
static hipError_t next_event_pair(rtc_ctx* c, std::pair<Event, Event>** out) { return next_event_pair(c->events, c->events_used, out); }
static hipError_t feedback_staging(rtc_ctx* c, size_t bytes, void** p) {  // (the caller has synchronised the device: nothing is using the old one)
    const hipError_t e = c->h_feedback.grow(bytes);
    *p = c->h_feedback.get();
    return e;
}
static int compute_units(rtc_ctx* c) {  // of the context's device (asked once: the query takes a fraction of a millisecond)
    if (c->n_cus == 0) {
        hipDeviceProp_t prop;
        c->n_cus = hipGetDeviceProperties(&prop, c->device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    return c->n_cus;
}

// A block list's first launch has left its waves' times (BlockList::TIMED): the list of this and every later frame is made from
// them (refine_block_list); feedback_passes times over.
static rtc_status recut_block_list(rtc_ctx* c, BlockList& bl, uint32_t rows) {
    const Policy& P = c->policy;
    HIP_TRY(hipDeviceSynchronize());  // (once per scene, partition and pass; the launch may be on any stream)
    const auto host_t0 = std::chrono::steady_clock::now();  // (after the wait for the frame, which the caller's next step would have had anyway)
    std::vector<uint32_t> refined;
    double throughput_ticks = 0.0;
    void* staging = nullptr;
    HIP_TRY(feedback_staging(c, 4u * bl.n * sizeof(uint32_t), &staging));
    const uint32_t* ticks = (const uint32_t*)staging;
    HIP_TRY(hipMemcpy(staging, bl.d_ticks, 4u * bl.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    refine_block_list(bl.host, ticks, c->scene.hdr.width, rows, 0.85 * 4.0 * compute_units(c) * c->tree_waves, 0.01 * P.feedback_pct, 0.01 * P.feedback_down_pct,
                      &refined, P.feedback_max_s, &throughput_ticks, ss_max_share_log2(c->scene.ss_k));
    if (P.jit_print) {
        size_t by_s[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};  // blocks by lanes per pixel (log2), before and after
        for (uint32_t t : bl.host.empty() ? refined : bl.host) by_s[0][tile_s(t)]++;
        for (uint32_t t : refined) by_s[1][tile_s(t)]++;
        std::fprintf(stderr, "librtc_amd: block list made from the frame before's wave times: %zu blocks; pixels by lanes per pixel 1/2/4/8/16: "
                             "%zu/%zu/%zu/%zu/%zu -> %zu/%zu/%zu/%zu/%zu k\n", bl.n, by_s[0][0] * 256 / 1000, by_s[0][1] * 128 / 1000, by_s[0][2] * 64 / 1000,
                     by_s[0][3] * 32 / 1000, by_s[0][4] * 16 / 1000, by_s[1][0] * 256 / 1000, by_s[1][1] * 128 / 1000, by_s[1][2] * 64 / 1000, by_s[1][3] * 32 / 1000,
                     by_s[1][4] * 16 / 1000);
    }
    HIP_TRY(bl.d.grow(refined.size(), true));  // (nothing is in flight: the synchronisation above)
    HIP_TRY(feedback_staging(c, refined.size() * sizeof(uint32_t), &staging));  // (the times have been used)
    std::memcpy(staging, refined.data(), refined.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpy(bl.d, staging, refined.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    bl.n = refined.size();
    bl.passes++;
    bl.host = refined;  // (kept: a later scene of this size starts from it, restart_block_lists)
    bl.state = bl.passes < P.feedback_passes ? BlockList::FRESH /* time this list's first launch as well */ : BlockList::REFINED;
    // How often scenes that change (restart_block_lists) may have the list re-cut: what this re-cut cost the host may be a
    // sixteenth of the frames between -- their time taken from below: the waves' times over the device's wave slots (the timer runs
    // at 100 MHz).
    const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
    const double frame_ms = std::max(1e-3, throughput_ticks * 1e-5);
    bl.recut_host_ms = std::max(0.05, host_ms);
    if (P.jit_print) std::fprintf(stderr, "librtc_amd: the re-cut took the host %.3f ms (a frame takes %.3f ms or more)\n", host_ms, frame_ms);
    return RTC_OK;
}

// A regular grid's first frame has left what its waves cost (BlockList::TIMED): their times, or -- kernels that do not time
// their waves -- their work counts.  Is the order worth a list?  Both orders go through a model of the dispatcher with the blocks'
// costs: the list is taken when it ends the frame at least 3 % earlier (reflect_refract 9 %, first_textures 20 %, hexagons 8 %:
// yes; the frames of short, even waves -- C3 1 %, first_scene 0 % -- no: there a list's scalar load and the lost neighbourhood of
// the blocks in flight cost more than the order gives).  gx x gy: the launched (padded) grid.
static rtc_status order_grid(rtc_ctx* c, BlockList& bl, uint32_t gx, uint32_t gy, uint32_t rows) {
    const Policy& P = c->policy;
    HIP_TRY(hipDeviceSynchronize());  // (once per scene and partition)
    const size_t nt = bl.n;  // the blocks of the timed launch: the (padded) grid's
    std::vector<uint32_t> launched(nt), ordered;
    void* staging = nullptr;
    HIP_TRY(feedback_staging(c, 4u * nt * sizeof(uint4), &staging));
    uint32_t* ticks = (uint32_t*)staging;
    if (bl.counts) {
        // what a wave cost, from what it counted: rays that met objects, and shade points (each a light-cone cull, a Phong
        // evaluation, a push or pop of the recursion) at sixteen rays apiece
        const uint4* counts = (const uint4*)staging;
        HIP_TRY(hipMemcpy(staging, bl.d_ticks, 4u * nt * sizeof(uint4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 4u * nt; i++) {  // (in place: ticks[i] overwrites a word of counts[i / 4], which has been read)
            const uint4 n = counts[i];
            ticks[i] = wave_work(n.x, n.y, n.z);
        }
    } else {
        HIP_TRY(hipMemcpy(staging, bl.d_ticks, 4u * nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (uint32_t by = 0; by < gy; by++)
        for (uint32_t bx = 0; bx < gx; bx++) {  // the block workgroup (bx, by) rendered: the kernel's permutation
            uint32_t x = bx, y = by;
            if (bl.swizzled) {
                const uint32_t j = (by & 3u) * gx + bx, r = j & 7u;
                y = (by & ~3u) + (r >> 1);
                x = 2u * (j >> 3) + (r & 1u);
            }
            launched[(size_t)by * gx + bx] = tile_word(0u, 16u * x, 16u * y);
        }
    const double wave_slots = 0.85 * 4.0 * compute_units(c) * 6.0;
    bl.state = BlockList::REFINED;
    bl.listed = false;
    {
        double in_order = 0.0, longest_first = 0.0;
        const bool pays = longest_first_pays(ticks, nt, (size_t)(wave_slots / 4.0), &in_order, &longest_first);
        if (P.jit_print) std::fprintf(stderr, "librtc_amd: grid of %zu blocks: modelled frame %.4g in image order, %.4g longest first\n", nt, in_order, longest_first);
        if (!pays) return RTC_OK;  // (the grid stays)
    }
    refine_block_list(launched, ticks, c->scene.hdr.width, rows, wave_slots, INFINITY, 0.0, &ordered);
    if (ordered.empty() || ordered.size() > bl.n) return RTC_OK;
    HIP_TRY(bl.d.grow(ordered.size(), true));  // (nothing is in flight: the synchronisation above)
    std::memcpy(staging, ordered.data(), ordered.size() * sizeof(uint32_t));  // (the times have been used; ordered.size() <= nt)
    HIP_TRY(hipMemcpy(bl.d, staging, ordered.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    bl.n_listed = ordered.size();
    bl.listed = true;
    return RTC_OK;
}

// One launch of the scene's render kernel: the scene-compiled one, or the context's ahead-of-time family.
static hipError_t launch_render(rtc_ctx* c, hipFunction_t spec_fn, dim3 grid, hipStream_t stream, RenderArgs& a) {
    if (c->scene.ss_k != 1u) {  // a supersampled context: `a` is the fine frame's, a.out the output canvas (rtc_supersample.h)
        SsRenderArgs sa;
        sa.fine = a;
        sa.out_width = a.hdr.width / c->scene.ss_k, sa.out_rows = a.rows / c->scene.ss_k;
        if (c->scene.lens_mode) {  // ... whose rays leave from a lens (rtc_lens.h)
            LensRenderArgs la;
            la.ss = sa;
            // the scene-box early-out is argued for rays from the camera's origin (primary_ray): not for these
            la.ss.fine.hdr.has_scene_box = 0u;
            la.aperture_radius = c->scene.lens.aperture_radius, la.focal_distance = c->scene.lens.focal_distance, la.seed = c->scene.lens.seed;
            return launch_scene_kernel(spec_fn, grid, stream, la, [&] {
                dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
                    // (a context of the one-call seam launches the variant that stores bytes and reports its rows: rtc_lens_seam.h)
                    if (c->seam_kernels && c->scene.ss_k == 2u) hipLaunchKernelGGL((lens_seam_render_kernel<decltype(nobj)::value, decltype(simple)::value, 2>), grid, dim3(256), 0, stream, la);
                    else if (c->seam_kernels) hipLaunchKernelGGL((lens_seam_render_kernel<decltype(nobj)::value, decltype(simple)::value, 4>), grid, dim3(256), 0, stream, la);
                    else if (c->scene.ss_k == 2u) hipLaunchKernelGGL((lens_render_kernel<decltype(nobj)::value, decltype(simple)::value, 2>), grid, dim3(256), 0, stream, la);
                    else hipLaunchKernelGGL((lens_render_kernel<decltype(nobj)::value, decltype(simple)::value, 4>), grid, dim3(256), 0, stream, la);
                });
            });
        }
        return launch_scene_kernel(spec_fn, grid, stream, sa, [&] {
            dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
                // (a context of the one-call seam launches the variant that stores bytes and reports its rows: rtc_supersample.h SEAM)
                if (c->seam_kernels && c->scene.ss_k == 2u) hipLaunchKernelGGL((ss_seam_render_kernel<decltype(nobj)::value, decltype(simple)::value, 2>), grid, dim3(256), 0, stream, sa);
                else if (c->seam_kernels) hipLaunchKernelGGL((ss_seam_render_kernel<decltype(nobj)::value, decltype(simple)::value, 4>), grid, dim3(256), 0, stream, sa);
                else if (c->scene.ss_k == 2u) hipLaunchKernelGGL((ss_render_kernel<decltype(nobj)::value, decltype(simple)::value, 2>), grid, dim3(256), 0, stream, sa);
                else hipLaunchKernelGGL((ss_render_kernel<decltype(nobj)::value, decltype(simple)::value, 4>), grid, dim3(256), 0, stream, sa);
            });
        });
    }
    return launch_scene_kernel(spec_fn, grid, stream, a, [&] {
        dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
            hipLaunchKernelGGL((render_kernel<decltype(nobj)::value, decltype(simple)::value>), grid, dim3(256), 0, stream, a);
        });
    });
}

// A slot's kernel with a frame stack of at least `depth` levels (rtc_scene_prep.h deep_variant of the slot's own).  Always a
// scene-compiled kernel, whatever RTC_AMD_SPECIALIZE says: the ahead-of-time kernels stop at RTC_STACK_DEPTH_BASE.
static rtc_status deep_kernel(rtc_ctx* c, int32_t depth, SceneKernel& s, hipFunction_t* out, std::string* out_id = nullptr) {
    auto it = s.deep.find(deep_stack_cap(depth));
    if (it == s.deep.end()) {
        KernelVariant deep;
        RTC_TRY(deep_variant(s.variant, depth, &deep));
        hipFunction_t fn = nullptr;
        std::string id;
        RTC_TRY(jit_get(c->policy, c->device, deep, &fn, &id));  // (the message is hiprtc's)
        it = s.deep.emplace(deep_stack_cap(depth), std::make_pair(fn, id)).first;
    }
    *out = it->second.first;
    if (out_id) *out_id = it->second.second;
    return RTC_OK;
}
// The kernel to launch for a slot at this depth, or null: the ahead-of-time family.  `want`: the specialisation policy asks for the
// scene's own kernel, which is compiled on first use (`lazy`: as jit_get's); deeper than the ahead-of-time stack it is always a
// scene kernel (deep_kernel).  When the policy wanted the scene's kernel and hiprtc did not deliver it, `failed` and `note`
// remember that (the slot's own; the two refinement slots share theirs).  RTC_AMD_SPECIALIZE=1: an error.  Default policy: the
// ahead-of-time kernel computes the same image -- several times slower on area-light scenes -- so say so: the note
// (rtc_ctx_jit_status(), rtc_stats.flags) and one line on stderr per process and `doing` ("rendering with", "tracing with",
// "refining with"; `named`: ... and the family's name).
static rtc_status scene_kernel_for(rtc_ctx* c, SceneKernel& s, int32_t depth, bool want, bool lazy, bool& failed, std::string& note,
                                   const char* doing, bool named, hipFunction_t* fn, std::string* id) {
    *fn = nullptr;
    if (depth > RTC_STACK_DEPTH_BASE) return deep_kernel(c, depth, s, fn, id);
    if (!want || failed) return RTC_OK;
    if (s.fn == nullptr) {
        const rtc_status jst = jit_get(c->policy, c->device, s.variant, &s.fn, &s.fn_id, lazy);
        if (jst != RTC_OK) {
            s.fn = nullptr;
            failed = true;
            note = rtc_last_error();
            if (c->policy.specialise == 1) return jst;
            static std::set<std::string> warned;
            if (!c->policy.quiet && warned.insert(doing).second)
                std::fprintf(stderr, "librtc_amd: scene specialisation unavailable, %s the slower ahead-of-time kernel%s%s: %.300s\n", doing,
                             named ? " " : "", named ? s.variant.family_name.c_str() : "", note.c_str());
            return RTC_OK;
        }
    }
    *fn = s.fn, *id = s.fn_id;
    return RTC_OK;
}

// The frame's kernel: compiled when the scene is set (or, lazy, when it comes again: compile_deferred), not by the first frame.
// RTC_AMD_SPECIALIZE=1 and no kernel: the context has no scene.
// (the one-call seam's variant of the supersampling kernels is a code object of its own: "aot_ss<k>_<hash>.seam"; its variant of the
// lens kernels is a kind of its own, JitKind::LENS_SEAM, whose id says so itself: "aot_lens<k>_<hash of its own>.seam")
static std::string ctx_aot_id(const rtc_ctx* c) {
    return aot_kernel_id(c->scene.render.variant.kind, c->scene.render.variant.k) + (c->seam_kernels && c->scene.render.variant.kind == JitKind::SS ? ".seam" : "");
}
static rtc_status compile_render_kernel(rtc_ctx* c, bool lazy) {
    SceneKernel& r = c->scene.render;
    hipFunction_t fn = nullptr;
    std::string id;
    const rtc_status jst = scene_kernel_for(c, r, 0, true, lazy, r.failed, r.note, "rendering with", true, &fn, &id);
    c->scene.kernel_name = fn ? r.variant.spec_name : r.variant.family_name;
    c->scene.kernel_id = fn ? id : ctx_aot_id(c);
    c->scene.jit_deferred = !fn && !r.failed;  // (lazy: this frame by the ahead-of-time kernel)
    if (r.failed) c->scene.plan.spec_shares = false;
    if (jst != RTC_OK) {
        c->scene.ready = false;
        c->soa_host.clear();
    }
    return jst;
}

// are these the records (and texels) that are resident on the device?
static bool same_records(const rtc_ctx* c, const std::vector<float4>& soa, const std::vector<float>& texels) {
    return c->scene.ready && soa.size() == c->soa_host.size() && texels.size() == c->texels_host.size() &&
           std::memcmp(soa.data(), c->soa_host.data(), soa.size() * sizeof(float4)) == 0 &&
           (texels.empty() || std::memcmp(texels.data(), c->texels_host.data(), texels.size() * sizeof(float)) == 0);
}
// The resident scene's kernel was left uncompiled the first time (jit_get, lazy): frames repeat, so now it pays.
static rtc_status compile_deferred(rtc_ctx* c) {
    c->scene.jit_deferred = false;
    HIP_TRY(hipDeviceSynchronize());  // (nothing of this context may be in flight while its kernel and lists change)
    RTC_TRY(compile_render_kernel(c, false));
    if (!c->scene.render.fn) return RTC_OK;
    c->block_lists.clear();  // (lists of the ahead-of-time launches: the scene's kernel takes other ones)
    c->scene_tile_lists.clear();
    c->scene.render.deep.clear();
    return RTC_OK;
}

}  // extern "C"

// rtc_ctx_set_scene (k = 1), and rtc_ctx_set_scene_ss with the FINE camera (k = 2, 4; rtc_camera_supersampled has checked it):
// a supersampled context flattens, plans, schedules and feeds back in fine space, with the code that exists.
// `lens` (rtc_ctx_set_scene_lens has checked it; k = 2, 4): the same, with the lens kernel in the supersampling kernel's place.
static rtc_status set_scene(rtc_ctx* c, const rtc_scene* scene, const rtc_camera* camera, uint32_t k, const rtc_lens* lens = nullptr) {
    if (!c) return fail(RTC_ERR_INVALID_ARG, "ctx is NULL");
    SceneHdr hdr;
    std::vector<float4> soa;
    std::vector<float> texels;
    std::vector<float> heavy_boxes;
    SceneRegion region;
    const Policy& P = c->policy;
    FlatHull flat_hull;
    rtc_status st = flatten(P, scene, camera, &hdr, &soa, &texels, &heavy_boxes, &region, false, &flat_hull, lens ? lens->aperture_radius : 0.0f);
    if (st != RTC_OK) return st;
    HIP_TRY(hipSetDevice(c->device));
    const bool resident = same_records(c, soa, texels);
    // the very scene that is resident (records, camera, light; the switches are the context's for life): nothing to replace
    // (another lens on it -- a focus pull: three words of the next launch's arguments)
    if (resident && c->scene.ss_k == k && c->scene.lens_mode == (lens != nullptr) && std::memcmp(&hdr, &c->scene.hdr, sizeof(hdr)) == 0) {
        if (lens) c->scene.lens = *lens;
        return c->scene.jit_deferred ? compile_deferred(c) : RTC_OK;
    }
    // Renders are asynchronous on caller streams (torch's are non-blocking: the null-stream copies below do not order
    // against them), and a render still in flight reads the records and the counters this call replaces.  Wait for
    // everything the context has launched before touching them.  (rtc.h: one stream at a time per context.)
    HIP_TRY(hipDeviceSynchronize());
    // (block lists: below; another factor is another kernel and other lane caps -- its lists start afresh)
    const bool same_frame = c->scene.ready && c->scene.hdr.width == hdr.width && c->scene.hdr.height == hdr.height && c->scene.ss_k == k && c->scene.lens_mode == (lens != nullptr);
    // until the new scene is fully resident the context has none (Scene::ready): nothing of the old one is left for a render path
    // to believe in, whatever fails below
    // (only the camera has moved -- an animation's usual frame: the records and texels that are resident stay)
    c->scene = rtc_ctx::Scene();
    rtc_ctx::Scene& s = c->scene;
    if (!resident) {
        c->soa_host.clear();
        c->texels_host.clear();
        if (!texels.empty()) {
            HIP_TRY(c->d_texels.grow(texels.size()));
            HIP_TRY(hipMemcpy(c->d_texels, texels.data(), texels.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (!soa.empty()) HIP_TRY(c->d_soa.grow(soa.size()));
        HIP_TRY(hipMemcpy(c->d_soa, soa.data(), soa.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    // the stream kernels' guard (nothing is in flight: the synchronisation above)
    if (hdr.internal_boxes && hdr.n_trav) {
        const std::vector<float4> open = open_flat_bvh(soa.data() + soa_index(SOA_COLUMNS, padded_count(hdr.n_objects), 0), hdr.n_trav);
        HIP_TRY(c->d_open_trav.grow(open.size()));
        HIP_TRY(hipMemcpy(c->d_open_trav, open.data(), open.size() * sizeof(float4), hipMemcpyHostToDevice));
        for (int a = 0; a < 3; a++) s.stream_guard.lo[a] = flat_hull.lo[a], s.stream_guard.hi[a] = flat_hull.hi[a];
        s.stream_guard.r_min = flat_hull.r_min;
        s.stream_guard.open_trav = c->d_open_trav;
    }
    s.plan = plan_scene(P, hdr, soa, scene, camera, heavy_boxes, region);  // which kernel will render this scene
    // Ray streams (rtc_ctx_trace) and the refinement of an adaptive frame: kernels of their own, none compiled yet -- the first call
    // that wants the scene's kernel compiles it
    s.trace.kernel.variant = trace_variant(s.plan);
    for (uint32_t i = 0; i < 2u; i++) s.adaptive.kernel[i].variant = refine_variant(s.plan, i ? 4u : 2u);
    for (uint32_t i = 0; i < 3u; i++) s.adaptive_seam.kernel[i].variant = seam_refine_variant(s.plan, 1u << i);
    if (k != 1u) plan_supersampled(&s.plan, k, c->seam_kernels && !lens);  // (the lens kernel's seam variant is derived from the non-seam plan)
    if (lens) plan_lens(&s.plan, c->seam_kernels);
    s.hdr = hdr;
    s.camera = *camera;
    s.ss_k = k;
    s.lens_mode = lens != nullptr;
    if (lens) s.lens = *lens;
    s.ready = true;
    if (!resident) {
        c->soa_host.swap(soa);
        c->texels_host.swap(texels);
    }
    if (same_frame && P.block_feedback) restart_block_lists(c);
    else c->block_lists.clear();  // (nothing is in flight any more: the synchronisation above)
    c->scene_tile_lists.clear();
    if (s.plan.tree_waves) c->tree_waves = s.plan.tree_waves;
    s.render.variant = render_variant(s.plan);
    s.kernel_name = s.plan.family_name;
    s.kernel_id = ctx_aot_id(c);
    if (s.plan.compile_now && !s.plan.spec_defs.empty()) return compile_render_kernel(c, c->lazy_jit && P.specialise == 2);
    return RTC_OK;
}

extern "C" {
rtc_status rtc_ctx_set_scene(rtc_ctx* c, const rtc_scene* scene, const rtc_camera* camera) { return set_scene(c, scene, camera, 1u); }

// The argument checks come first, the context's among them: all of them are decided on the host, before any device call.
rtc_status rtc_ctx_set_scene_ss(rtc_ctx* c, const rtc_scene* scene, const rtc_camera* output_camera, uint32_t k) {
    if (k == 1u) return set_scene(c, scene, output_camera, 1u);
    rtc_camera fine;
    RTC_TRY(rtc_camera_supersampled(output_camera, k, &fine));
    return set_scene(c, scene, &fine, k);
}

// The argument checks come first (rtc::check_lens_args, host only: the lens, the factor, the fine frame), then the context: all of
// them are decided before any device call.  Without a context: RTC_ERR_NO_DEVICE where there is no device to have made one on.
rtc_status rtc_ctx_set_scene_lens(rtc_ctx* c, const rtc_scene* scene, const rtc_camera* output_camera, uint32_t k, const rtc_lens* lens) {
    rtc_camera fine;
    RTC_TRY(check_lens_args("rtc_ctx_set_scene_lens", output_camera, k, lens, &fine));
    if (!c && usable_devices() <= 0) return fail(RTC_ERR_NO_DEVICE, "no HIP device visible; librtc_amd has no CPU fallback");
    return set_scene(c, scene, &fine, k, lens);
}
}  // extern "C"

// The scene's header as a launch of up to RTC_STACK_DEPTH_BASE levels takes it: where the packed counter of such a kernel cannot hold
// the culled shadow rays one lane may answer (rtc_launch_plan.h culled_count_fits), the whole-light cull and the block cones are off
// in the launch's copy -- the only two places that count one (Counters::add_culled).  `rays_per_lane`: the rays a lane traces into one
// counter; 0: unknown (the level-by-level renderer's lanes draw rays from a queue), every shade point the word can count.
// (Lights of up to 256 cells, the usual ones, fit whatever the launch is and are not looked at further.)
static SceneHdr launch_hdr(const rtc_ctx* c, int32_t depth, uint32_t rays_per_lane) {
    SceneHdr h = c->scene.hdr;
    const int64_t cells = (int64_t)h.u_steps * (int64_t)h.v_steps;
    if (h.light_kind != RTC_LIGHT_RECT || depth > RTC_STACK_DEPTH_BASE || cells * (int64_t)SHADED_COUNT_MAX <= (int64_t)CULLED_COUNT_MAX) return h;
    bool any_refl = rays_per_lane == 0u, any_refr = rays_per_lane == 0u;
    const uint32_t stride = padded_count(h.n_objects);
    for (uint32_t i = 0; i < h.n_objects && !(any_refl && any_refr); i++) {  // (as scene_recurses; NaN: recurses)
        any_refl = any_refl || !(c->soa_host[soa_index(COL_MAT_B, stride, i)].w == 0.0f);
        any_refr = any_refr || !(c->soa_host[soa_index(COL_MAT_C, stride, i)].x == 0.0f);
    }
    if (!culled_count_fits(cells, depth, any_refl, any_refr, rays_per_lane == 0u ? (uint32_t)SHADED_COUNT_MAX : rays_per_lane))
        h.cull_flags &= ~(CULL_ENABLED | CULL_CELLS);
    return h;
}

// The frame level by level (rtc_wavefront.h): one lane per ray, suspended shade_hits as nodes in HBM.  *used: false when the
// frame was not rendered this way (pools could not be allocated, or ran full: the caller renders it with the per-pixel kernel).
static rtc_status render_wavefront(rtc_ctx* c, int32_t depth, const Partition& q, uint32_t rows, void* d_out, bool out_u8, hipStream_t stream,
                                   uint32_t slot, bool* used) {
    *used = false;
    const size_t pixels = (size_t)rows * c->scene.hdr.width;
    // pools: a level's two ray lists hold up to two rays per pixel each, the node pool six suspended hits per pixel (a glass
    // mesh filling a quarter of the frame at depth 5 needs about one and three); a frame that needs more is rendered again
    const size_t cap_rays = std::max<size_t>(1024, 2 * pixels), cap_nodes = std::max<size_t>(1024, 6 * pixels);
    if (cap_nodes > 0x7fffffffull) return RTC_OK;
    if (cap_rays > c->d_wf_rays[0].capacity() || cap_nodes > c->d_wf_nodes.capacity() || !c->d_wf_ctr) {
        HIP_TRY(hipDeviceSynchronize());  // (the pools may be in use by a frame in flight)
        auto free_pools = [c]() {
            for (auto& r : c->d_wf_rays) r.release();
            c->d_wf_nodes.release();
        };
        free_pools();
        bool ok = true;
        for (auto& r : c->d_wf_rays) ok = ok && r.grow(cap_rays) == hipSuccess;
        ok = ok && c->d_wf_nodes.grow(cap_nodes) == hipSuccess;
        if (ok && !c->d_wf_ctr) ok = c->d_wf_ctr.grow(WF_CTR_WORDS) == hipSuccess;
        if (!ok) {  // not enough memory for the pools: the per-pixel kernel needs none
            (void)hipGetLastError();
            free_pools();
            return RTC_OK;
        }
    }
    WfArgs a;
    a.hdr = launch_hdr(c, depth, 0u);
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.out = out_u8 ? nullptr : (float*)d_out;
    a.out_u8 = out_u8 ? (uint8_t*)d_out : nullptr;
    a.rows = rows, a.band_rows = q.band_rows, a.n_parts = q.n_parts, a.part = q.part;
    a.depth = depth;
    a.nodes = c->d_wf_nodes;
    a.ctr = c->d_wf_ctr;
    a.cap_rays = (uint32_t)c->d_wf_rays[0].capacity(), a.cap_nodes = (uint32_t)c->d_wf_nodes.capacity();
    // (levels after the first and the combining passes draw their work from counters: a launch that fills the chip once)
    const uint32_t ray_wgs = 256u * 6u, node_wgs = 256u * 4u;
    const dim3 primary_grid((c->scene.hdr.width + 15u) / 16u, (rows + 15u) / 16u);
    const size_t n_counts = ((size_t)primary_grid.x * primary_grid.y + (size_t)depth * ray_wgs) * 4;  // one partial per wave of every tracing launch
    if (n_counts > c->d_block_counts.capacity()) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(c->d_block_counts.grow(n_counts));
    }
    a.wave_counts = c->d_block_counts;
    unsigned long long* total = c->d_total + 3 * (size_t)slot;
    HIP_TRY(hipMemsetAsync(c->d_wf_ctr, 0, WF_CTR_WORDS * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(total, 0, 3 * sizeof(unsigned long long), stream));
    std::pair<Event, Event>* ev = nullptr;
    HIP_TRY(next_event_pair(c, &ev));
    HIP_TRY(hipEventRecord(ev->first, stream));
    for (int32_t level = 0; level <= depth; level++) {
        a.level = (uint32_t)level;
        a.in_refl = c->d_wf_rays[2 * ((level + 1) & 1)], a.in_refr = c->d_wf_rays[2 * ((level + 1) & 1) + 1];
        a.out_refl = c->d_wf_rays[2 * (level & 1)], a.out_refr = c->d_wf_rays[2 * (level & 1) + 1];
        a.count_base = level == 0 ? 0u : (uint32_t)(((size_t)primary_grid.x * primary_grid.y + (size_t)(level - 1) * ray_wgs) * 4);
        if (level == 0)
            hipLaunchKernelGGL(wf_trace_kernel<true>, primary_grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL(wf_trace_kernel<false>, dim3(ray_wgs), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(wf_snapshot_kernel, dim3(1), dim3(1), 0, stream, c->d_wf_ctr.get(), (uint32_t)level, a.cap_nodes);
    }
    for (int32_t level = depth; level >= 0; level--) {
        a.level = (uint32_t)level;
        hipLaunchKernelGGL(wf_combine_kernel, dim3(node_wgs), dim3(256), 0, stream, a);
    }
    HIP_TRY(hipEventRecord(ev->second, stream));
    hipLaunchKernelGGL(sum_counts_kernel, dim3((uint32_t)((n_counts + SUM_COUNTS_SLICE - 1) / SUM_COUNTS_SLICE)), dim3(1024), 0, stream, c->d_block_counts.get(),
                       (uint32_t)n_counts, total, 0ull);
    HIP_TRY(hipGetLastError());
    // did everything fit?  (One small read-back: the call returns when the frame is done -- these frames take milliseconds.)
    uint32_t overflow = 0u;
    HIP_TRY(hipMemcpyAsync(&overflow, c->d_wf_ctr + WF_CTR_OVERFLOW, sizeof(overflow), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (overflow) {
        c->scene.wf_disabled = true;  // this scene needs more than the pools hold: per-pixel kernels from now on
        c->events_used--;
        return RTC_OK;
    }
    c->rendered = true;
    c->wf_last = true;
    *used = true;
    return RTC_OK;
}

// What the context's cached lists add to a launch (ctx_render_slot).
struct LaunchLists {
    const uint32_t* d_tiles = nullptr;  // RenderArgs::tiles
    uint32_t* d_ticks = nullptr;        // RenderArgs::wave_ticks
    BlockList* timed_list = nullptr;    // a list whose own events bracket this launch
    void* copy_counts_to = nullptr;     // where the launch's wave counts go afterwards, on its stream
    SceneTileList* scene_tiles = nullptr;
};

// (a world in which nothing reflects or transmits -- an empty world among them, which the reference renders black at any
// depth -- never suspends a shade_hit: whatever the depth asked for, the base kernels trace it as they trace depth 8)
static bool scene_recurses(const rtc_ctx* c) {
    const uint32_t stride = padded_count(c->scene.hdr.n_objects);
    for (uint32_t i = 0; i < c->scene.hdr.n_objects; i++) {
        const float4 mb = c->soa_host[soa_index(COL_MAT_B, stride, i)], mc = c->soa_host[soa_index(COL_MAT_C, stride, i)];
        if (!(mb.w == 0.0f) || !(mc.x == 0.0f)) return true;  // reflective, transparency (NaN: recurses)
    }
    return false;
}

// room for one more of the context's block lists (a caller cycling through partitions without end: start over -- nothing may be in flight)
static rtc_status block_list_room(rtc_ctx* c) {
    if (c->block_lists.size() >= 256u) {
        HIP_TRY(hipDeviceSynchronize());
        c->block_lists.clear();
    }
    return RTC_OK;
}

// Tree worlds with meshes: a block list instead of the regular grid -- the tiles a mesh projects to first, eight
// lanes per pixel there and one elsewhere (build_block_list).
// ... and frames that share an area light's cells between a pixel's lanes (small frames: choose_share_log2), when there is a
// frame before to go by: the list starts with the frame's one lane count everywhere, and the feedback gives the tiles in the
// penumbra more lanes, the lit and the empty ones fewer (refine_block_list).
// One list per partition, built on first use and kept until the scene changes: rtc_render_ex renders a frame as
// several partitions of one context, frame after frame (a single cached list meant a device synchronisation, a
// rebuild and a blocking copy per chunk launch).
static rtc_status use_block_list(rtc_ctx* c, const Partition& q, uint32_t rows, int32_t depth, uint32_t share_log2, bool mesh_list, hipStream_t stream,
                                 LaunchPlan* lp, LaunchLists* L) {
    const Policy& P = c->policy;
    const std::array<uint32_t, 5> key = {q.band_rows, q.n_parts, q.part, share_log2, P.block_feedback ? (uint32_t)depth : 0u};
    auto it = c->block_lists.find(key);
    if (it == c->block_lists.end()) {
        RTC_TRY(block_list_room(c));
        std::vector<uint32_t> host;
        if (mesh_list) build_block_list(P.block_order, P.block_s, P.block_s_top, TileMask{c->scene.plan.heavy_tiles.data(), c->scene.plan.heavy_w, c->scene.plan.heavy_h}, c->scene.hdr.width, share_log2, rows, q, &host,
                                        ss_max_share_log2(c->scene.ss_k));
        else uniform_block_list(share_log2, c->scene.hdr.width, rows, &host);
        BlockList bl;
        bl.n = host.size();
        if (P.block_feedback) bl.host = host;
        HIP_TRY(bl.d.grow(host.size(), true));
        // (a new buffer: no launch in flight can be reading it; the copy is complete when the call returns)
        hipError_t ce = hipMemcpy(bl.d, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (ce != hipSuccess) return fail(RTC_ERR_DEVICE, "block list upload failed: %s", hipGetErrorString(ce));
        it = c->block_lists.emplace(key, std::move(bl)).first;
    }
    BlockList& bl = it->second;
    if (P.block_feedback && bl.state == BlockList::TIMED) RTC_TRY(recut_block_list(c, bl, rows));
    // (a refined list under scenes that change: every frame is timed -- restart_block_lists decides from them when to re-cut)
    if (P.block_feedback && (bl.state == BlockList::FRESH || (bl.state == BlockList::REFINED && bl.animated)) && bl.n != 0) {
        HIP_TRY(bl.d_ticks.grow(4u * bl.n, true));
        HIP_TRY(hipMemsetAsync(bl.d_ticks, 0, 4u * bl.n * sizeof(uint32_t), stream));
        L->d_ticks = bl.d_ticks;
        if (bl.state == BlockList::FRESH) {
            bl.state = BlockList::TIMED;
        } else {
            HIP_TRY(bl.ev0.create());
            HIP_TRY(bl.ev1.create());
            L->timed_list = &bl;
        }
    }
    L->d_tiles = bl.d;
    lp->run_list(bl.n);
    return RTC_OK;
}

// A scene-tile list's second frame has left what its waves counted (SceneTileList::TIMED): as order_grid, for a list -- the same
// cost of a wave, the same model of the dispatcher, the same 3 %.  The tiles stay whole and the fill runs as they are.
static rtc_status order_scene_tiles(rtc_ctx* c, SceneTileList& tl, uint32_t rows) {
    HIP_TRY(hipDeviceSynchronize());  // (once per scene and partition)
    tl.state = SceneTileList::SETTLED;
    void* staging = nullptr;
    HIP_TRY(feedback_staging(c, 4u * tl.n * sizeof(uint4), &staging));
    HIP_TRY(hipMemcpy(staging, tl.d_counts, 4u * tl.n * sizeof(uint4), hipMemcpyDeviceToHost));
    const uint4* counts = (const uint4*)staging;
    uint32_t* ticks = (uint32_t*)staging;
    for (size_t i = 0; i < 4u * tl.n; i++) {  // (in place: ticks[i] overwrites a word of counts[i / 4], which has been read)
        const uint4 n = counts[i];
        ticks[i] = wave_work(n.x, n.y, n.z);
    }
    double in_order = 0.0, longest_first = 0.0;
    const bool pays = longest_first_pays(ticks, tl.n, (size_t)(0.85 * compute_units(c) * 6.0), &in_order, &longest_first);
    if (c->policy.jit_print)
        std::fprintf(stderr, "librtc_amd: scene tiles: list of %zu: modelled frame %.4g in list order, %.4g longest first\n", tl.n, in_order, longest_first);
    if (!pays) return RTC_OK;  // (the list stays)
    std::vector<uint32_t> ordered;
    order_tile_list(tl.host, ticks, c->scene.hdr.width, rows, &ordered);
    if (ordered.size() != tl.n) return RTC_OK;
    HIP_TRY(hipMemcpy(tl.d, ordered.data(), tl.n * sizeof(uint32_t), hipMemcpyHostToDevice));  // (nothing is in flight: the synchronisation above)
    tl.host.swap(ordered);
    tl.ordered = true;
    return RTC_OK;
}

// Scene tiles (ScenePlan::scene_tile_mask): the canvas is zero-filled at memory speed (805 MB of an 8192^2 frame: 0.12 ms) and
// only the tiles some entry of the world projects to get a workgroup -- C5: 18 k of 262 k, where the bounding rectangle of
// them all has 60 k, and a frame of such short waves costs what starting them costs (0.78 waves per ns).  The partition's
// list, built and uploaded on first use (an empty one: nothing of the scene in this partition's rows).
// The list's first frame starts its tiles in the grid's permuted order (swizzle_tile_list); the second of the same scene leaves its
// waves' work counts, and the frames after it start the tiles longest first where the grid feedback's model says that pays
// (order_scene_tiles).
static rtc_status use_scene_tile_list(rtc_ctx* c, const Partition& q, uint32_t rows, bool feedback, hipStream_t stream, LaunchLists* L) {
    const Policy& P = c->policy;
    const std::array<uint32_t, 3> key = {q.band_rows, q.n_parts, q.part};
    auto it = c->scene_tile_lists.find(key);
    if (it == c->scene_tile_lists.end()) {
        // (a caller cycling through partitions without end: start over -- nothing may be in flight)
        if (c->scene_tile_lists.size() >= 256u) {
            HIP_TRY(hipDeviceSynchronize());
            c->scene_tile_lists.clear();
        }
        SceneTilePlan host;
        plan_scene_tiles(TileMask{c->scene.plan.scene_tile_mask.data(), c->scene.plan.scene_tiles_w, c->scene.plan.scene_tiles_h}, c->scene.hdr.width, c->scene.hdr.height, q, &host);
        if (P.swizzle) {
            std::vector<uint32_t> permuted;
            swizzle_tile_list(host.tiles, c->scene.hdr.width, rows, &permuted);
            host.tiles.swap(permuted);
        }
        static_assert(sizeof(FillRun) == sizeof(uint2), "fill_tiles_kernel reads the runs as uint2");
        SceneTileList tl;
        tl.n = host.tiles.size();
        tl.n_fill = host.fill.size();
        tl.traced_pixels = host.traced_pixels;
        if (tl.n) {
            HIP_TRY(tl.d.grow(tl.n));
            HIP_TRY(hipMemcpyAsync(tl.d, host.tiles.data(), tl.n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            if (tl.n_fill) {
                HIP_TRY(tl.d_fill.grow(tl.n_fill));
                HIP_TRY(hipMemcpyAsync(tl.d_fill, host.fill.data(), tl.n_fill * sizeof(uint2), hipMemcpyHostToDevice, stream));
            }
            HIP_TRY(hipStreamSynchronize(stream));  // (the host vectors go out of scope)
        }
        tl.host.swap(host.tiles);
        it = c->scene_tile_lists.emplace(key, std::move(tl)).first;
    }
    SceneTileList& tl = it->second;
    if (tl.n && feedback) {
        if (tl.state == SceneTileList::TIMED) RTC_TRY(order_scene_tiles(c, tl, rows));
        if (tl.state == SceneTileList::IDLE) {
            tl.state = SceneTileList::FRESH;
        } else if (tl.state == SceneTileList::FRESH) {
            if (!tl.d_counts) HIP_TRY(tl.d_counts.grow(4u * tl.n));
            L->copy_counts_to = tl.d_counts;
            tl.state = SceneTileList::TIMED;
        }
    }
    if (it->second.n && !c->fill_stream) {  // the zero-fill runs beside the render kernel (fork / join by events)
        HIP_TRY(c->fill_stream.create(hipStreamNonBlocking));
        HIP_TRY(c->ev_fork.create(hipEventDisableTiming));
        HIP_TRY(c->ev_join.create(hipEventDisableTiming));
    }
    L->scene_tiles = &it->second;
    return RTC_OK;
}

// A regular grid's frames after the first: the same 16 x 16 blocks, started in the order of their longest wave in the frame
// before (refine_block_list: a list of one lane per pixel throughout).  Where the grid is the plain one -- one block per
// workgroup, no scene rectangle, nobody waiting for rows in image order (rtc_render_ex's progress words) -- and the frame
// has a tail worth the list: a model of the dispatcher ends it at least 3 % earlier longest first (order_grid).
// timed_waves: the kernel leaves its waves' times (else their work counts are taken).
static rtc_status use_grid_feedback(rtc_ctx* c, const Partition& q, uint32_t rows, int32_t depth, bool timed_waves, hipStream_t stream, LaunchPlan* lp,
                                    LaunchLists* L) {
    const std::array<uint32_t, 5> key = {q.band_rows, q.n_parts, q.part, 0xffffffffu, (uint32_t)depth};
    auto it = c->block_lists.find(key);
    if (it == c->block_lists.end()) {
        RTC_TRY(block_list_room(c));
        BlockList bl;
        bl.n = lp->n_workgroups();
        bl.state = BlockList::IDLE;
        it = c->block_lists.emplace(key, std::move(bl)).first;
    }
    BlockList& bl = it->second;
    if (bl.state == BlockList::TIMED) RTC_TRY(order_grid(c, bl, lp->grid_x, lp->grid_y, rows));
    if (bl.state == BlockList::IDLE) {
        bl.state = BlockList::FRESH;  // (the next frame of this scene, if there is one, is measured)
    } else if (bl.state == BlockList::FRESH && bl.n == lp->n_workgroups()) {
        bl.counts = !timed_waves;
        bl.swizzled = lp->swizzle;
        HIP_TRY(bl.d_ticks.grow(4u * bl.n * (bl.counts ? sizeof(uint4) / sizeof(uint32_t) : 1u), true));
        if (bl.counts) {
            L->copy_counts_to = bl.d_ticks;
        } else {
            HIP_TRY(hipMemsetAsync(bl.d_ticks, 0, 4u * bl.n * sizeof(uint32_t), stream));
            L->d_ticks = bl.d_ticks;
        }
        bl.state = BlockList::TIMED;
    } else if (bl.state == BlockList::REFINED && bl.listed) {
        L->d_tiles = bl.d;
        lp->run_list(bl.n_listed);
    }
    return RTC_OK;
}

// The FIRST launch of a code object on a queue pays what is not the kernel's: the runtime moves the code to the device and
// sizes the queue's scratch for it -- 6 to 11 ms in a fresh process for these kernels (tools/first_frame_probe.py: C3's first
// frame 0.95 ms cold, 0.71 once any context of the process has launched the same code; mesh 11.2 / 3.4).  It is paid once per
// process and queue, here: one workgroup of the same kernel over zero rows (it finds no pixel of its own and writes only
// the counters the real launch overwrites), in front of the events that time the frame.
// (`kernel`: the slot's kernel this launch runs -- `fn`, or the ahead-of-time family's key; `launch_no_op`: one workgroup of it over the
// caller's no-op variant of its arguments)
template <class Launch>
static rtc_status warm_up(Warmed& warmed, const void* kernel, hipStream_t stream, Launch&& launch_no_op) {
    if (warmed.insert(std::make_pair(kernel, (const void*)stream)).second) HIP_TRY(launch_no_op());
    return RTC_OK;
}

// A scene-tile launch's zero-fill of the unlisted tiles runs beside the render kernel, on the context's fill stream: memory-bound
// work under arithmetic.  (The caller joins: the frame's stream waits for ev_join after the render kernel.)
static rtc_status fork_tile_fill(rtc_ctx* c, const SceneTileList& tl, void* d_out, uint32_t rows, bool out_u8, hipStream_t stream) {
    HIP_TRY(hipEventRecord(c->ev_fork, stream));
    HIP_TRY(hipStreamWaitEvent(c->fill_stream, c->ev_fork, 0));
    // 96 workgroups share the jobs: enough to move 690 MB in the time C5's tiles take to render, few enough to leave the chip's wave
    // slots to the render kernel (C5 8192^2, whole frame: 0.84 / 0.46 / 0.33 / 0.294 / 0.30 / 0.36 / 0.38 ms with 16 / 32 / 64 / 96 /
    // 128 / 512 / 4096 of them; the bounding rectangle with its interleaved fill: 0.335; profiles/r04_c5_tile_fill.txt)
    const uint32_t fill_wgs = c->policy.tile_fill_wgs ? c->policy.tile_fill_wgs : 96u;
    hipLaunchKernelGGL(fill_tiles_kernel, dim3((uint32_t)std::min<size_t>(tl.n_fill, fill_wgs)), dim3(256), 0, c->fill_stream.get(), tl.d_fill.get(),
                       (uint32_t)tl.n_fill, (uint8_t*)d_out, c->scene.hdr.width, rows, out_u8 ? 3u : 12u);
    HIP_TRY(hipEventRecord(c->ev_join, c->fill_stream));
    return RTC_OK;
}

// RenderArgs of a frame: the one place where a LaunchPlan and the lists' device pointers become kernel arguments
static RenderArgs render_args(const rtc_ctx* c, const Partition& q, uint32_t rows, int32_t depth, uint32_t share_log2, void* d_out_rgb, bool out_u8,
                              unsigned long long* total, const ProgressPlan* progress, const LaunchPlan& lp, const LaunchLists& L) {
    RenderArgs a;
    a.hdr = launch_hdr(c, depth, lp.blocks_y);
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.out = out_u8 ? nullptr : (float*)d_out_rgb;
    a.out_u8 = out_u8 ? (uint8_t*)d_out_rgb : nullptr;
    a.progress = lp.n_chunks ? c->d_progress.get() : nullptr;
    a.done = lp.n_chunks ? progress->d_done : nullptr;
    a.chunk_block_rows = lp.chunk_block_rows;
    a.epoch = progress ? progress->epoch : 0u;
    a.block_counts = c->d_block_counts;
    a.total = total;
    a.rows = rows, a.band_rows = q.band_rows, a.n_parts = q.n_parts, a.part = q.part;
    a.depth = depth;
    a.share_log2 = share_log2;
    a.tiles = L.d_tiles;
    a.wave_ticks = L.d_ticks;
    a.blocks_y = lp.blocks_y;
    a.swizzle = lp.swizzle ? 1u : 0u;
    a.block_x0 = lp.block_x0, a.block_y0 = lp.block_y0;
    a.fill_wg_rows = lp.fill_wg_rows, a.fill_rows = lp.fill_rows, a.fill_period = lp.fill_period;
    a.fill_x0 = lp.fill_rect[0], a.fill_x1 = lp.fill_rect[1], a.fill_y0 = lp.fill_rect[2], a.fill_y1 = lp.fill_rect[3];
    return a;
}

// Level by level instead of pixel by pixel (rtc_wavefront.h): only on request (RTC_AMD_WAVEFRONT=1).  Built in round 3 for
// the frames whose time is their longest wave (glass meshes), bit-identical -- and measured slower everywhere: mesh 2048^2
// 8.0 ms against 3.8, here_be_dragons 4000 x 1600 9.6 against 3.0 (profiles/r03_wavefront_ab.txt).  A level is a launch, a
// launch ends with ITS longest wave -- one packet walk over a divided mesh is hundreds of microseconds -- and a frame of
// depth 5 pays six of those tails where the per-pixel kernel pays one; its walks are also the generic ones (no lanes
// splitting leaf runs, no per-scene compile).  What the finding asks for is a single persistent launch with a queue of rays
// and continuation frames, not level-synchronous passes.  Kept as a verified alternative, not a default.
static bool wavefront_wanted(const rtc_ctx* c, uint32_t rows, int32_t depth) {
    return c->scene.hdr.n_trav != 0u && rows > 0u && depth >= 1 && depth <= RTC_STACK_DEPTH_BASE && (int)depth < (int)WF_MAX_LEVELS && !c->scene.wf_disabled &&
           (size_t)rows * c->scene.hdr.width <= (16u << 20) && c->policy.wavefront == 1 && c->scene.ss_k == 1u;
}

// What a partition with rows that is not run from a mesh / area-light block list is launched as: scene tiles, else the scene
// rectangle, else the regular grid -- which alone, and only while it is one block per workgroup (plain_grid), is swizzled,
// re-ordered by the grid feedback or cut into progress chunks.
static rtc_status settle_shape(rtc_ctx* c, const Partition& q, uint32_t rows, int32_t depth, uint32_t share_log2, hipFunction_t spec_fn, void* d_out_rgb,
                               bool out_u8, const ProgressPlan* progress, hipStream_t stream, LaunchPlan* lp, LaunchLists* L) {
    const Policy& P = c->policy;
    const bool list_words_fit = c->scene.hdr.width <= 65532u && rows <= 131068u;  // (tile_word)
    if (lp->shape == LaunchPlan::GRID && share_log2 == 0u && !c->scene.plan.scene_tile_mask.empty() && (q.band_rows & 15u) == 0u && list_words_fit &&
        (progress == nullptr || c->scene.plan.scene_tiles_sparse)) {
        // (the feedback: as for the grid, not where rows are reported chunk by chunk -- the seam's frames pay no wait for it)
        RTC_TRY(use_scene_tile_list(c, q, rows, P.block_feedback && P.grid_feedback && progress == nullptr, stream, L));
        if (L->scene_tiles->n) {
            lp->run_scene_tiles(L->scene_tiles->n, c->last_pixels - L->scene_tiles->traced_pixels);
            L->d_tiles = L->scene_tiles->d;
        }
    }
    // Scene rectangle: every primary ray outside the rectangle the scene's box projects to (project_heavy_boxes: exact
    // camera arithmetic in double, 8 pixels of padding, "everything" if the box reaches behind the camera) sees nothing --
    // black, one ray.  Where that rectangle is under half the frame: plan_rect_launch.  RTC_AMD_SCENE_RECT=0: the whole grid.
    if (lp->shape == LaunchPlan::GRID && share_log2 == 0u && c->scene.plan.scene_rect[0] < c->scene.plan.scene_rect[1] && c->scene.plan.scene_rect_coverage < P.scene_rect_threshold() &&
        (spec_fn == nullptr || c->scene.plan.spec_rect)) {
        plan_rect_launch(lp, c->scene.hdr.width, c->scene.hdr.height, q, rows, c->last_pixels, c->scene.plan.scene_rect, P.blocks_y == 0 ? 1u : lp->blocks_y, out_u8, P.fill_wgs);
        // a frame of bytes: the zeros outside the rectangle are one asynchronous memset in front of the launch
        if (out_u8) HIP_TRY(hipMemsetAsync(d_out_rgb, 0, (size_t)rows * c->scene.hdr.width * 3u, stream));
    }
    if (P.swizzle && lp->plain_grid()) lp->pad_for_swizzle();
    if (lp->plain_grid() && P.block_feedback && P.grid_feedback && progress == nullptr && share_log2 == 0u && list_words_fit &&
        !(c->scene.hdr.n_trav != 0u && P.wavefront))
        RTC_TRY(use_grid_feedback(c, q, rows, depth, spec_fn && c->scene.plan.spec_shares, stream, lp, L));
    // progress reporting: a regular grid only (one workgroup per block, every block of the partition launched)
    if (progress && progress->d_done && lp->plain_grid()) plan_chunks(lp, progress->want_chunks, PROGRESS_MAX_CHUNKS);
    return RTC_OK;
}

// rtc_ctx_render with a counter slot of the caller's choosing (rtc_internal.h)
rtc_status rtc::ctx_render_slot(rtc_ctx* c, int32_t depth, const rtc_partition* part, void* d_out_rgb, void* stream_, uint32_t slot,
                                ProgressPlan* progress, bool out_u8) {
    // ---- arguments
    if (progress) progress->n_chunks = 0u, progress->chunk_rows = 0u;
    if (!c) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render: null argument");
    if (slot >= CTX_TOTAL_SLOTS) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render: counter slot %u", slot);
    if (!c->scene.ready || c->scene.hdr.width == 0) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render: no scene/camera set");
    // A supersampled context: the caller's partition counts OUTPUT rows -- bands of band_rows output rows are k * band_rows fine
    // rows -- and from here on everything is the fine frame's: c->scene.hdr, `rows`, the launch's shape, its lists and their feedback.
    const uint32_t ss_k = c->scene.ss_k;
    rtc_partition fine_part;
    if (ss_k != 1u) {
        // progress words and the u8 canvas (rtc_render_ss): the plain grid reports, a block-list launch is finished when its stream
        // is.  Only the kernels of the one-call seam's contexts have those paths (rtc_supersample.h SEAM, rtc_lens_seam.h).
        if ((progress || out_u8) && !c->seam_kernels)
            return fail(RTC_ERR_UNSUPPORTED, "rtc_ctx_render: a supersampled context renders f32 frames without progress words (bytes and progress words: rtc_render_ss)");
        const Partition o = resolve(part);
        if (o.band_rows > 0xffffffffu / ss_k) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render: band_rows %u times the supersampling factor %u", o.band_rows, ss_k);
        fine_part.band_rows = o.band_rows * ss_k, fine_part.n_parts = o.n_parts, fine_part.part = o.part;
        part = &fine_part;
    }
    const uint32_t rows = partition_rows(c->scene.hdr.height, part);
    // a partition that owns no band (height < band_rows * n_parts) has nothing to write and may pass a null buffer
    if (!d_out_rgb && rows != 0) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render: null output buffer");
    if (depth < 0 || depth > RTC_MAX_DEPTH)
        return fail(RTC_ERR_INVALID_ARG, "depth %d outside [0, %d]", depth, RTC_MAX_DEPTH);
    const Partition q = resolve(part);
    if (q.part >= q.n_parts) return fail(RTC_ERR_INVALID_ARG, "partition %u of %u", q.part, q.n_parts);
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const Policy& P = c->policy;
    const uint32_t width = c->scene.hdr.width, height = c->scene.hdr.height;
    // ---- depth and kernel
    // camera.rs:76 takes any depth; the kernels' frame stack (one suspended shade_hit per level, world.rs:62-86) holds
    // RTC_STACK_DEPTH_BASE levels.  Deeper than that, the scene's kernel is compiled once more with a longer stack -- 16, 32,
    // ... RTC_MAX_DEPTH levels of per-lane scratch -- on first use, and kept with the context.
    hipFunction_t spec_fn = c->scene.render.fn;
    if (depth > RTC_STACK_DEPTH_BASE && !scene_recurses(c)) depth = RTC_STACK_DEPTH_BASE;
    if (depth > RTC_STACK_DEPTH_BASE && rows > 0u) RTC_TRY(deep_kernel(c, depth, c->scene.render, &spec_fn));
    const bool shares = spec_fn && c->scene.plan.spec_shares;  // only kernels compiled for it share lanes
    // (supersampled: capped so that a k x k group lies in one wave's tile, rtc_launch_plan.h)
    const uint32_t share_log2 = shares ? std::min(choose_share_log2(c->scene.hdr, rows, P, progress == nullptr), ss_max_share_log2(ss_k)) : 0u;
    // ---- the launch's shape, and the cached list that goes with it
    LaunchPlan lp = plan_grid(width, rows, share_log2, spec_fn && c->scene.plan.spec_blocks_y && ss_k == 1u, (uint32_t)P.blocks_y);
    LaunchLists L;
    // (block lists: not when RTC_AMD_SHARE_LOG2 pins one value for all; an area light's not for rtc_render_ex, whose rows leave in order)
    const bool mesh_list = shares && !c->scene.plan.heavy_tiles.empty() && c->scene.hdr.light_kind == RTC_LIGHT_POINT;
    const bool area_list = shares && c->scene.hdr.light_kind == RTC_LIGHT_RECT && share_log2 != 0u && P.block_feedback && progress == nullptr;
    const bool list_words_fit = width <= 65532u && rows <= 131068u;  // (tile_word)
    if ((mesh_list || area_list) && P.share_log2 < 0 && list_words_fit && rows > 0u) RTC_TRY(use_block_list(c, q, rows, depth, share_log2, mesh_list, stream, &lp, &L));
    c->scene.trace.last = false;  // (rtc_ctx_stats reports renders again)
    c->last_rows = rows / ss_k;  // (rows written to the caller's buffer)
    c->last_share_log2 = share_log2;
    c->last_pixels = traced_pixels(width, height, q);
    if (wavefront_wanted(c, rows, depth)) {
        bool used = false;
        RTC_TRY(render_wavefront(c, depth, q, rows, d_out_rgb, out_u8, stream, slot, &used));
        if (used) return RTC_OK;
    }
    c->wf_last = false;
    unsigned long long* const total = c->d_total + 3 * (size_t)slot;
    if (rows == 0) {  // nothing to launch: the slot's counters read zero
        HIP_TRY(hipMemsetAsync(total, 0, 3 * sizeof(unsigned long long), stream));
        if (slot == 0) c->rendered = false;
        return RTC_OK;
    }
    RTC_TRY(settle_shape(c, q, rows, depth, share_log2, spec_fn, d_out_rgb, out_u8, progress, stream, &lp, &L));
    // ---- workspaces (grow-only: first call / larger image only)
    const size_t n_blocks = lp.n_workgroups() * 4;  // partial counts: one per wave
    HIP_TRY(c->d_block_counts.grow(n_blocks));
    if (lp.n_chunks) {
        const size_t words = lp.progress_words(PROGRESS_STRIDE);
        HIP_TRY(c->d_progress.grow(words));
        HIP_TRY(hipMemsetAsync(c->d_progress, 0, words * sizeof(uint32_t), stream));
        // (the counters are the FINE grid's, one per block row of lp.grid_y; the caller's rows are output rows)
        uint32_t chunk_rows = 0u;
        if (!chunk_output_rows(lp, ss_k, &chunk_rows))
            return fail(RTC_ERR_DEVICE, "rtc_ctx_render: chunks of %u blocks of %u fine rows do not end between output rows (factor %u)", lp.chunk_block_rows, lp.block_h, ss_k);
        progress->n_chunks = lp.n_chunks;
        progress->chunk_rows = chunk_rows;
    }
    RenderArgs a = render_args(c, q, rows, depth, share_log2, d_out_rgb, out_u8, total, progress, lp, L);
    // ---- warm up, time, launch, sum
    std::pair<Event, Event>* ev = nullptr;
    HIP_TRY(next_event_pair(c, &ev));
    RTC_TRY(warm_up(c->render_warmed, spec_fn ? (const void*)spec_fn : aot_family(c).key(ss_k, ss_k != 1u && c->seam_kernels, c->scene.lens_mode), stream, [&] {
        RenderArgs w = a;
        w.rows = 0u, w.tiles = nullptr, w.wave_ticks = nullptr, w.progress = nullptr, w.done = nullptr, w.fill_wg_rows = 0u, w.swizzle = 0u, w.blocks_y = 1u;
        return launch_render(c, spec_fn, dim3(1, 1), stream, w);
    }));
    HIP_TRY(hipEventRecord(ev->first, stream));
    const bool tile_fill = lp.shape == LaunchPlan::SCENE_TILES && L.scene_tiles->n_fill != 0;
    if (tile_fill) RTC_TRY(fork_tile_fill(c, *L.scene_tiles, d_out_rgb, rows, out_u8, stream));
    if (L.timed_list) HIP_TRY(hipEventRecord(L.timed_list->ev0, stream));
    HIP_TRY(launch_render(c, spec_fn, dim3(lp.grid_x, lp.grid_y), stream, a));
    if (tile_fill) HIP_TRY(hipStreamWaitEvent(stream, c->ev_join, 0));
    HIP_TRY(hipEventRecord(ev->second, stream));
    if (L.timed_list) {
        HIP_TRY(hipEventRecord(L.timed_list->ev1, stream));
        L.timed_list->ev_recorded = true;
    }
    if (L.copy_counts_to) HIP_TRY(hipMemcpyAsync(L.copy_counts_to, c->d_block_counts, n_blocks * sizeof(uint4), hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(sum_counts_kernel, dim3((uint32_t)((n_blocks + SUM_COUNTS_SLICE - 1) / SUM_COUNTS_SLICE)), dim3(1024), 0, stream,
                       c->d_block_counts.get(), (uint32_t)n_blocks, total, lp.extra_rays);
    HIP_TRY(hipGetLastError());
    c->rendered = true;
    return RTC_OK;
}

// After the caller has synchronised with every launch: counters summed over slots [0, n_slots), kernel_ms = the SUM
// of the launches' HIP-event times since the last stats call (the launches of one frame run back to back).
void rtc::ctx_mark_one_shot(rtc_ctx* c) {
    if (c) c->lazy_jit = c->seam_kernels = true;
}

rtc_status rtc::ctx_collect(rtc_ctx* c, uint32_t n_slots, rtc_stats* out) {
    std::memset(out, 0, sizeof(*out));
    if (n_slots > CTX_TOTAL_SLOTS) n_slots = CTX_TOTAL_SLOTS;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<unsigned long long> total(3 * (size_t)n_slots, 0ull);
    if (n_slots) HIP_TRY(hipMemcpy(total.data(), c->d_total, total.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < n_slots; s++) {
        out->rays += total[3 * s];
        out->shaded_hits += total[3 * s + 1];
        out->culled_shadow_rays += total[3 * s + 2];
    }
    double sum_ms = 0.0;
    HIP_TRY(sum_event_ms(c, &sum_ms));
    out->kernel_ms = (float)sum_ms;
    out->launches = (uint32_t)c->events_used;
    out->flags = c->scene.render.note.empty() ? 0u : RTC_STATS_JIT_FALLBACK;
    c->events_used = 0;
    return RTC_OK;
}

extern "C" {

// Diagnostics (not in rtc.h; tests/test_block_lists.py, no device needed): refine_block_list and simulate_dispatch as
// rtc_ctx_render uses them.  -> the number of blocks of the new list (its first min(that, cap) are written to `out`).
uint32_t rtc_diag_refine_block_list(const uint32_t* list, const uint32_t* ticks, uint32_t n, uint32_t width, uint32_t rows, double wave_slots,
                                    double threshold, double down, uint32_t* out, uint32_t cap) {
    std::vector<uint32_t> l(list, list + n), refined;
    refine_block_list(l, ticks, width, rows, wave_slots, threshold, down, &refined);
    for (size_t i = 0; i < refined.size() && i < cap; i++) out[i] = refined[i];
    return (uint32_t)refined.size();
}
double rtc_diag_simulate_dispatch(const uint32_t* cost, uint32_t n, uint32_t slots) {
    return simulate_dispatch(std::vector<uint32_t>(cost, cost + n), slots);
}
// ... and rtc_launch_plan.h's arithmetic (tests/test_launch_plan.py).  The band walk: {y0, y1, local0} per band into `bands`
// (the first min(n, cap) of them; -> n), `facts` = {partition_rows, traced_pixels, does global_row give every local row the
// row the walk gave it}.
uint32_t rtc_diag_band_walk(uint32_t height, uint32_t width, const rtc_partition* part, uint32_t* bands, uint32_t cap, uint64_t facts[3]) {
    const Partition q = resolve(part);
    uint32_t n = 0;
    bool inverts = true;
    for_each_band(height, q, [&](uint32_t y0, uint32_t y1, uint32_t local0) {
        if (n < cap) bands[3 * n] = y0, bands[3 * n + 1] = y1, bands[3 * n + 2] = local0;
        n++;
        for (uint32_t y = y0; y < y1; y++) inverts = inverts && global_row(q, local0 + (y - y0)) == y;
    });
    facts[0] = partition_rows(height, part), facts[1] = traced_pixels(width, height, q), facts[2] = inverts ? 1u : 0u;
    return n;
}
// The scene-tile list of a partition: counts = {tiles, fill runs}; -> traced pixels inside the listed tiles.
uint64_t rtc_diag_scene_tiles(const uint8_t* mask, uint32_t mask_w, uint32_t mask_h, uint32_t width, uint32_t height, const rtc_partition* part,
                              uint32_t* tiles, uint32_t* fill /* pairs */, uint32_t cap, uint32_t counts[2]) {
    SceneTilePlan plan;
    plan_scene_tiles(TileMask{mask, mask_w, mask_h}, width, height, resolve(part), &plan);
    for (size_t i = 0; i < plan.tiles.size() && i < cap; i++) tiles[i] = plan.tiles[i];
    for (size_t i = 0; i < plan.fill.size() && i < cap; i++) fill[2 * i] = plan.fill[i].x0_n, fill[2 * i + 1] = plan.fill[i].row;
    counts[0] = (uint32_t)plan.tiles.size(), counts[1] = (uint32_t)plan.fill.size();
    return plan.traced_pixels;
}
// A scene-tile list's orders (tests/test_plane_tiles_plan.py): ticks == NULL: the first frame's (swizzle_tile_list); else the
// feedback's from four wave costs per tile (order_tile_list).  -> the new list's length (its first min(that, cap) words in `out`).
uint32_t rtc_diag_tile_order(const uint32_t* list, const uint32_t* ticks, uint32_t n, uint32_t width, uint32_t rows, uint32_t* out, uint32_t cap) {
    std::vector<uint32_t> l(list, list + n), made;
    if (ticks) order_tile_list(l, ticks, width, rows, &made);
    else swizzle_tile_list(l, width, rows, &made);
    for (size_t i = 0; i < made.size() && i < cap; i++) out[i] = made[i];
    return (uint32_t)made.size();
}
// ... and the cost of a wave that counted {rays, shade points, culled shadow rays}, and whether longest first is worth a list
uint32_t rtc_diag_wave_work(uint32_t rays, uint32_t shade_points, uint32_t culled) { return wave_work(rays, shade_points, culled); }
int32_t rtc_diag_longest_first_pays(const uint32_t* ticks, uint32_t n_blocks, uint32_t wg_slots) { return longest_first_pays(ticks, n_blocks, wg_slots) ? 1 : 0; }
// The scene-tile mask of a scene and camera under the environment's policy: -> the number of tiles written (w * h; 0: the scene has
// no mask -- not known, or the policy does not want it), dims = {w, h}.
uint32_t rtc_diag_scene_tile_mask(const rtc_scene* scene, const rtc_camera* camera, uint8_t* mask, uint32_t cap, uint32_t dims[2]) {
    dims[0] = dims[1] = 0u;
    if (!scene || !camera) return 0u;
    const Policy P = Policy::from_env();
    SceneHdr hdr;
    std::vector<float4> soa;
    std::vector<float> texels, heavy_boxes;
    SceneRegion region;
    if (flatten(P, scene, camera, &hdr, &soa, &texels, &heavy_boxes, &region) != RTC_OK) return 0u;
    ScenePlan p;
    plan_coverage(P, hdr, camera, region, &p);
    if (p.scene_tile_mask.empty() || p.scene_tile_mask.size() > cap) return 0u;
    std::memcpy(mask, p.scene_tile_mask.data(), p.scene_tile_mask.size());
    dims[0] = p.scene_tiles_w, dims[1] = p.scene_tiles_h;
    return (uint32_t)p.scene_tile_mask.size();
}
// What the context's last rtc_ctx_render left out: {tiles listed, fill runs, feedback} of the partition's scene-tile list (0, 0: the
// frame was not drawn from one); feedback: 0 the list has not been launched with feedback, 1 its counts are on the device, 2 they
// have been judged and the list stays, 3 ... and the list was re-ordered.
void rtc_diag_ctx_scene_tiles(rtc_ctx* c, const rtc_partition* part, uint32_t out[3]) {
    out[0] = out[1] = out[2] = 0u;
    if (!c) return;
    const Partition q = resolve(part);
    auto it = c->scene_tile_lists.find({q.band_rows, q.n_parts, q.part});
    if (it == c->scene_tile_lists.end()) return;
    const SceneTileList& tl = it->second;
    out[0] = (uint32_t)tl.n, out[1] = (uint32_t)tl.n_fill;
    out[2] = tl.state <= SceneTileList::FRESH ? 0u : tl.state == SceneTileList::TIMED ? 1u : tl.ordered ? 3u : 2u;
}
// A scene-rectangle launch of a partition: out = {grid_x, grid_y, blocks_y, block_x0, block_y0, fill_wg_rows, fill_rows, fill_period,
// fill_rect[4]}; -> extra_rays.
uint64_t rtc_diag_rect_launch(uint32_t width, uint32_t height, const rtc_partition* part, const uint32_t rect[4], uint32_t blocks_y, int32_t out_u8,
                              uint32_t fill_wgs, uint32_t out[12]) {
    const Partition q = resolve(part);
    LaunchPlan lp;
    plan_rect_launch(&lp, width, height, q, partition_rows(height, part), traced_pixels(width, height, q), rect, blocks_y, out_u8 != 0, fill_wgs);
    const uint32_t v[12] = {lp.grid_x, lp.grid_y, lp.blocks_y, lp.block_x0, lp.block_y0, lp.fill_wg_rows, lp.fill_rows, lp.fill_period,
                            lp.fill_rect[0], lp.fill_rect[1], lp.fill_rect[2], lp.fill_rect[3]};
    std::memcpy(out, v, sizeof(v));
    return lp.extra_rays;
}
// The packed counter's capacity (tests/test_light_grid_limits.py): does a launch of `depth` levels whose lanes trace `rays_per_lane` rays
// each count the culled shadow rays of a light of u_steps x v_steps cells exactly (1), or does it run with the culls off (0)?
int32_t rtc_diag_culled_count_fits(int32_t u_steps, int32_t v_steps, int32_t depth, int32_t any_refl, int32_t any_refr, uint32_t rays_per_lane) {
    return culled_count_fits((int64_t)u_steps * (int64_t)v_steps, depth, any_refl != 0, any_refr != 0, rays_per_lane) ? 1 : 0;
}

// The lanes per pixel (log2) the context's last rtc_ctx_render was planned with -- a block list's entries may differ per tile, under
// the same cap (tests/test_gpu_supersample.py: the cap in effect under a pinned RTC_AMD_SHARE_LOG2).
uint32_t rtc_diag_ctx_share_log2(rtc_ctx* c) { return c ? c->last_share_log2 : 0u; }
// Supersampled frames (tests/test_supersample_boundary.py): -> the lanes per pixel (log2) a frame of factor k is planned with when the
// frame's own choice is share_log2; and, with a list, that list re-cut from `ticks` as a supersampled context re-cuts it (the
// first min(*n_out, cap) blocks into `out`) -- list == NULL: the uniform list a lane-sharing frame starts from.
uint32_t rtc_diag_ss_plan(uint32_t k, uint32_t share_log2, const uint32_t* list, const uint32_t* ticks, uint32_t n, uint32_t width, uint32_t rows,
                          double wave_slots, uint32_t* out, uint32_t cap, uint32_t* n_out) {
    const uint32_t max_s = ss_max_share_log2(k), s = std::min(share_log2, max_s);
    std::vector<uint32_t> made;
    if (list && ticks) refine_block_list(std::vector<uint32_t>(list, list + n), ticks, width, rows, wave_slots, 0.85, 0.40, &made, 4u, nullptr, max_s);
    else uniform_block_list(s, width, rows, &made);
    for (size_t i = 0; out && i < made.size() && i < cap; i++) out[i] = made[i];
    if (n_out) *n_out = (uint32_t)made.size();
    return s;
}
// The progress chunks of a supersampled launch that reports (rtc_render_ss; tests/test_seam_supersample_boundary.py): a partition of
// out_rows rows of out_width output pixels at factor k, the frame's own choice of lanes per pixel share_log2 (capped as the launch caps
// it), swizzled or not, want_chunks asked for.  out = {grid_x, grid_y, block_h, chunk_block_rows, n_chunks, chunk rows in OUTPUT rows,
// lanes per pixel (log2) planned with, PROGRESS_MAX_CHUNKS}; -> 1 when a chunk is a whole number of output rows, else 0.
int32_t rtc_diag_ss_chunks(uint32_t out_width, uint32_t out_rows, uint32_t k, uint32_t share_log2, int32_t swizzle, uint32_t want_chunks, uint32_t out[8]) {
    const LaunchPlan lp = plan_ss_chunks(out_width, out_rows, k, share_log2, swizzle != 0, want_chunks, PROGRESS_MAX_CHUNKS);
    uint32_t chunk_rows = 0u;
    const bool whole = chunk_output_rows(lp, k, &chunk_rows);
    const uint32_t v[8] = {lp.grid_x, lp.grid_y, lp.block_h, lp.chunk_block_rows, lp.n_chunks, chunk_rows, std::min(share_log2, ss_max_share_log2(k)), PROGRESS_MAX_CHUNKS};
    std::memcpy(out, v, sizeof(v));
    return whole ? 1 : 0;
}

// A scene's preparation on the host, under the environment's policy (as rtc_scene_validate): flatten, then plan_scene.
// digests: FNV-1a of the SceneHdr's bytes, of the records, of the texels, and of the plan's three tile masks together; text: the
// plan, one key=value per line.  A null camera (the batched entry points' case): the first three digests only.
rtc_status rtc_diag_scene_plan(const rtc_scene* scene, const rtc_camera* camera, char* text, uint32_t cap, uint64_t digests[4]) {
    if (!text || !cap || !digests) return fail(RTC_ERR_INVALID_ARG, "rtc_diag_scene_plan: null argument");
    text[0] = 0;
    digests[0] = digests[1] = digests[2] = digests[3] = 0u;
    const Policy P = Policy::from_env();
    SceneHdr hdr;
    std::vector<float4> soa;
    std::vector<float> texels, heavy_boxes;
    SceneRegion region;
    RTC_TRY(flatten(P, scene, camera, &hdr, &soa, &texels, &heavy_boxes, &region));
    digests[0] = rtc::fnv1a(&hdr, sizeof(hdr));
    digests[1] = rtc::fnv1a(soa.data(), soa.size() * sizeof(float4));
    digests[2] = rtc::fnv1a(texels.data(), texels.size() * sizeof(float));
    if (!camera) return RTC_OK;
    const ScenePlan p = plan_scene(P, hdr, soa, scene, camera, heavy_boxes, region);
    digests[3] = rtc::fnv1a(p.scene_tile_mask.data(), p.scene_tile_mask.size(),
                            rtc::fnv1a(p.scene_rect_tiles.data(), p.scene_rect_tiles.size(), rtc::fnv1a(p.heavy_tiles.data(), p.heavy_tiles.size())));
    char b[512];
    snprintf(b, sizeof(b), "simple=%d\nheavy_tiles=%zu %u %u\nscene_box_coverage=%.9g\nscene_rect=%u %u %u %u\nscene_rect_coverage=%.9g\n"
             "scene_tile_mask=%zu %u %u\nspec_shares=%d\nspec_blocks_y=%d\nspec_rect=%d\ntree_waves=%d\nwf_pays=%d\ncompile_now=%d\n",
             (int)p.simple, p.heavy_tiles.size(), p.heavy_w, p.heavy_h, (double)p.scene_box_coverage, p.scene_rect[0], p.scene_rect[1], p.scene_rect[2],
             p.scene_rect[3], (double)p.scene_rect_coverage, p.scene_tile_mask.size(), p.scene_tiles_w, p.scene_tiles_h, (int)p.spec_shares,
             (int)p.spec_blocks_y, (int)p.spec_rect, p.tree_waves, (int)p.wf_pays, (int)p.compile_now);
    std::string out = b;
    // the ball triangle pre-culling is argued for (SceneHdr::has_tbox, cull_c, cull_r2): rays that start outside it do not pre-cull
    snprintf(b, sizeof(b), "tri_cull=%u %.9g %.9g %.9g %.9g\n", hdr.has_tbox, (double)hdr.cull_c[0], (double)hdr.cull_c[1], (double)hdr.cull_c[2],
             (double)hdr.cull_r2);
    out += b;
    // ... and what the JIT makes of every variant (rtc_jit.h), with this process's hiprtc and the embedded source
    int major = 0, minor = 0;
    (void)hiprtcVersion(&major, &minor);
    const JitArgSizes sizes = k_jit_arg_sizes;
    out += "hiprtc=" + std::to_string(major) + "." + std::to_string(minor) + "\nkey_tail=" + jit_key_tail(JitKind::RENDER, major, minor, sizes) +
           "render_args=" + std::to_string(sizes.render) + "\ntrace_args=" + std::to_string(sizes.trace) + "\nadaptive_args=" + std::to_string(sizes.adaptive) + "\n";
    auto joined = [](const std::vector<std::string>& defs) {
        std::string line;
        for (size_t i = 0; i < defs.size(); i++) line += (i ? " " : "") + defs[i];
        return line + "\n";
    };
    // <prefix>family_name, spec_name, spec_defs, entry, header, options (hiprtc's), cache_file, aot_id; `deep`: <prefix>deep16_spec_defs, deep16_cache_file, deep32_
    // (a world without objects: <prefix>deep16_error = status and message)
    auto add = [&](const std::string& prefix, const KernelVariant& v, bool deep = false) {
        const JitKindFacts& kind = jit_kind_facts(v.kind);
        out += prefix + "family_name=" + v.family_name + "\n" + prefix + "spec_name=" + v.spec_name + "\n" + prefix + "spec_defs=" + joined(v.defs);
        const JitPlan jit = plan_jit(v.defs, v.kind, P.jit_flags, major, minor, sizes, k_core_src, beside_text(v.kind));
        if (*kind.header_below) out += prefix + "header_below=" + kind.header_below + "\n";
        if (*kind.header_below2) out += prefix + "header_below2=" + kind.header_below2 + "\n";
        out += prefix + "entry=" + jit.entry + "\n" + prefix + "header=" + kind.header + "\n" + prefix + "options=" + joined(jit.opts) + prefix + "cache_file=" +
               jit.cache_file + "\n" + prefix + "aot_id=" + aot_kernel_id(v.kind, v.k) + "\n";
        for (int depth : {16, 32}) {
            KernelVariant d;
            if (!deep) continue;
            const std::string name = prefix + "deep" + std::to_string(depth);
            const rtc_status st = deep_variant(v, depth, &d);
            if (st != RTC_OK) out += name + "_error=" + std::to_string((int)st) + " " + rtc_last_error() + "\n";
            else out += name + "_spec_defs=" + joined(d.defs) + name + "_cache_file=" + plan_jit(d.defs, d.kind, P.jit_flags, major, minor, sizes, k_core_src, beside_text(d.kind)).cache_file + "\n";
        }
    };
    add("", render_variant(p), true);
    add("trace_", trace_variant(p), true);
    for (uint32_t k : {2u, 4u}) add("adaptive" + std::to_string(k) + "_", refine_variant(p, k));
    for (uint32_t k : {2u, 4u}) add("ss" + std::to_string(k) + "_", render_variant(p, k));  // (of this camera as the fine one)
    for (uint32_t k : {2u, 4u}) {  // ... and the lens kernels of a lens context (rtc_ctx_set_scene_lens), likewise
        ScenePlan lens_plan = p;
        plan_supersampled(&lens_plan, k);
        plan_lens(&lens_plan);
        add("lens" + std::to_string(k) + "_", render_variant(lens_plan), false);
        out += "lens" + std::to_string(k) + "_args=" + std::to_string(sizes.lens) + "\n";
    }
    // ... and the adaptive kernels of the one-call seam's contexts (rtc_render_adaptive; rtc_adaptive_seam.h): the halo pass, then the
    // refinements.  (In front of the seam's lens kernels, which tests/test_seam_lens_boundary.py pins as the text's last lines.)
    for (uint32_t k : {1u, 2u, 4u}) {
        add("adaptive_seam" + std::to_string(k) + "_", seam_refine_variant(p, k));
        out += "adaptive_seam" + std::to_string(k) + "_args=" + std::to_string(sizes.adaptive_seam) + "\n";
    }
    for (uint32_t k : {2u, 4u}) {  // ... and the lens kernels of the one-call seam's contexts (rtc_render_lens; rtc_lens_seam.h)
        ScenePlan lens_plan = p;
        plan_supersampled(&lens_plan, k);
        plan_lens(&lens_plan, true);
        add("lens" + std::to_string(k) + "_seam_", render_variant(lens_plan), false);
        out += "lens" + std::to_string(k) + "_seam_args=" + std::to_string(sizes.lens) + "\n";
    }
    if (out.size() >= cap) return fail(RTC_ERR_INVALID_ARG, "rtc_diag_scene_plan: the text needs %zu bytes", out.size() + 1);
    std::memcpy(text, out.c_str(), out.size() + 1);
    return RTC_OK;
}

// Does a context of this scene and camera -- under this lens, or none (null) -- get a hierarchy of the library's own (build_flat_bvh)?
// Host only, under the environment's policy: 1 / 0, or -1 where the scene is refused.  (A lens widens where primary rays start.)
int32_t rtc_diag_flat_bvh(const rtc_scene* scene, const rtc_camera* camera, const rtc_lens* lens) {
    SceneHdr hdr;
    std::vector<float4> soa;
    std::vector<float> texels;
    if (flatten(Policy::from_env(), scene, camera, &hdr, &soa, &texels, nullptr, nullptr, false, nullptr, lens ? lens->aperture_radius : 0.0f) != RTC_OK) return -1;
    return hdr.internal_boxes ? 1 : 0;
}

// rtc_jit.h's cache entries and rtc_scene_prep.h's stack cap, as they are (tests/test_jit_plan.py).  _read: the code's length, or -1.
int32_t rtc_diag_jit_cache_publish(const char* dir, const char* file, const void* bytes, uint64_t n) {
    return publish_cache_entry(dir, std::string(dir) + "/" + file, std::string((const char*)bytes, (size_t)n)) ? 1 : 0;
}
int64_t rtc_diag_jit_cache_read(const char* path, void* out, uint64_t cap) {
    std::string code;
    if (!read_cache_entry(path, &code)) return -1;
    if (out) std::memcpy(out, code.data(), std::min<size_t>(code.size(), (size_t)cap));
    return (int64_t)code.size();
}
int32_t rtc_diag_deep_stack_cap(int32_t depth) { return deep_stack_cap(depth); }

rtc_status rtc_ctx_render(rtc_ctx* c, int32_t depth, const rtc_partition* part, void* d_out_rgb, void* stream) {
    return rtc::ctx_render_slot(c, depth, part, d_out_rgb, stream, 0u);
}

// The context's scene and camera, none of its render state: no counters, no events, no block or tile lists, no compiled
// kernel -- a render after this call finds the context as the render before it left it.
rtc_status rtc_ctx_render_hits(rtc_ctx* c, const rtc_partition* part, const rtc_hit_planes* d_out, void* stream_) {
    if (!c || !d_out) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_hits: null argument");
    HitPlanes planes;
    if (!hit_planes_view(d_out, &planes)) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_hits: no plane requested");
    if (!c->scene.ready || c->scene.hdr.width == 0) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_hits: no scene/camera set");
    if (c->scene.lens_mode) return fail(RTC_ERR_UNSUPPORTED, "rtc_ctx_render_hits: the context renders through a lens (%u x %u rays per pixel): a first hit per output pixel is not defined", c->scene.ss_k, c->scene.ss_k);
    if (c->scene.ss_k != 1u) return fail(RTC_ERR_UNSUPPORTED, "rtc_ctx_render_hits: the context is supersampled (%u x %u rays per pixel): a first hit per output pixel is not defined", c->scene.ss_k, c->scene.ss_k);
    const Partition q = resolve(part);
    if (q.part >= q.n_parts) return fail(RTC_ERR_INVALID_ARG, "partition %u of %u", q.part, q.n_parts);
    // (rtc_ctx_set_scene refuses RTC_JITTER_SEQUENCE lights: no resident scene has one)
    const uint32_t rows = partition_rows(c->scene.hdr.height, part);
    if (rows == 0) return RTC_OK;  // a partition that owns no band has nothing to write
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    HitsArgs a;
    a.hdr = c->scene.hdr;
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.planes = planes;
    a.rows = rows;
    a.band_rows = q.band_rows, a.n_parts = q.n_parts, a.part = q.part;
    const bool light = planes.light != nullptr;
    // A wave's tile (HitsArgs::tile_w_log2), geometry only (profiles/hits_times.txt, planes = object, distance, normal; 8 x 8 / 32 x 2 /
    // 64 x 1): C3 4096^2 233 / 232 / 232 us -- neither the walk nor the stores: a quarter of a million waves of a few hundred
    // instructions each; mesh 2048^2 167 / 197 / 266 us -- the walk, which wants a wave's rays close together; C5 8192^2 516 / 450 /
    // 450 us -- 95 % of its pixels miss the scene's box and store zeros, 24 B each: there the stores bind, and a wave that writes
    // 128 contiguous bytes of a dword plane per row beats one that writes eight pieces of 32.  So: the compact tile, but the
    // 32 x 2 one where most of the frame is sky (the share below which the render puts several blocks into a workgroup).
    // With the light plane always the compact tile: intensity_at's wave votes (block cones, culls) decide more when a wave's
    // pixels are close together.  RTC_AMD_HITS_TILE (development) pins one.
    a.tile_w_log2 = (!light && c->scene.plan.scene_box_coverage < 0.25f) ? 5u : 3u;
    if (c->policy.hits_tile == 3 || c->policy.hits_tile == 5 || c->policy.hits_tile == 6) a.tile_w_log2 = (uint32_t)c->policy.hits_tile;
    const uint32_t bw = a.tile_w_log2 == 3u ? 16u : 1u << a.tile_w_log2, bh = 256u / bw;
    const dim3 grid((c->scene.hdr.width + bw - 1) / bw, (rows + bh - 1) / bh), block(256);
    // the families rtc_ctx_render's ahead-of-time branch chooses from (SIMPLE is a property of intensity_at alone: the
    // geometry-only kernels exist once per object-loop family)
    dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
        if (light) hipLaunchKernelGGL((hits_kernel<decltype(nobj)::value, decltype(simple)::value, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((hits_kernel<decltype(nobj)::value, false, false>), grid, block, 0, stream, a);
    });
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

}  // extern "C"

// ---- ray streams (rtc_trace.h) ---------------------------------------------------
static hipError_t launch_trace(rtc_ctx* c, hipFunction_t fn, uint32_t n_workgroups, hipStream_t stream, TraceArgs& a) {
    return launch_scene_kernel(fn, dim3(n_workgroups), stream, a, [&] {
        dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
            hipLaunchKernelGGL((trace_kernel<decltype(nobj)::value, decltype(simple)::value>), dim3(n_workgroups), dim3(256), 0, stream, a);
        });
    });
}

// rtc_ctx_trace's and rtc_ctx_trace_reordered's argument checks, the context's last among them: all are decided on the host, before
// any device call.
static rtc_status trace_args_ok(const char* who, const rtc_ctx* c, int32_t depth, const void* d_origins, const void* d_directions, const void* d_keys,
                                uint32_t n, const void* d_out_rgb) {
    if (n > 0u && (!d_origins || !d_directions)) return fail(RTC_ERR_INVALID_ARG, "%s: null ray buffer", who);
    if (n > 0u && !d_out_rgb) return fail(RTC_ERR_INVALID_ARG, "%s: null output buffer", who);
    if (((uintptr_t)d_origins & 15u) || ((uintptr_t)d_directions & 15u))
        return fail(RTC_ERR_INVALID_ARG, "%s: origins and directions must be 16-byte aligned", who);
    if (((uintptr_t)d_keys & 3u) || ((uintptr_t)d_out_rgb & 3u)) return fail(RTC_ERR_INVALID_ARG, "%s: keys and output must be 4-byte aligned", who);
    if (depth < 0 || depth > RTC_MAX_DEPTH) return fail(RTC_ERR_INVALID_ARG, "%s: depth %d outside [0, %d]", who, depth, RTC_MAX_DEPTH);
    if (!c) return fail(RTC_ERR_INVALID_ARG, "%s: ctx is NULL", who);
    if (!c->scene.ready) return fail(RTC_ERR_INVALID_ARG, "%s: no scene set", who);
    return RTC_OK;
}

// The trace itself, n > 0 rays whose arguments have been checked: the kernel's choice, its workspaces, the launch between the
// trace's events, the counters.  (The device is the context's already.)
static rtc_status trace_launch(rtc_ctx* c, int32_t depth, const void* d_origins, const void* d_directions, const void* d_keys, uint32_t n,
                               void* d_out_rgb, hipStream_t stream) {
    // (rtc_ctx_set_scene refuses RTC_JITTER_SEQUENCE lights: no resident scene has one)
    rtc_ctx::Trace& t = c->trace;
    rtc_ctx::Scene::Trace& st = c->scene.trace;
    const Policy& P = c->policy;
    if (depth > RTC_STACK_DEPTH_BASE && !scene_recurses(c)) depth = RTC_STACK_DEPTH_BASE;  // (as rtc_ctx_render)
    // (rtc_ctx_set_scene's policy with the number of rays in the place of the frame's pixels)
    const bool want = !st.kernel.variant.defs.empty() && wants_scene_kernel(P, n, c->scene.plan.compile_any_size, c->scene.plan.compile_never);
    hipFunction_t fn = nullptr;
    std::string id;
    RTC_TRY(scene_kernel_for(c, st.kernel, depth, want, false, st.kernel.failed, st.kernel.note, "tracing with", true, &fn, &id));
    st.name = fn ? st.kernel.variant.spec_name : st.kernel.variant.family_name;
    st.id = fn ? id : aot_kernel_id(JitKind::TRACE);
    // workspaces (grow-only; a trace in flight on this stream may still be writing the old partials: grow frees, which waits)
    const uint32_t n_workgroups = (uint32_t)(((uint64_t)n + 255u) / 256u);
    const size_t n_counts = (size_t)n_workgroups * 4u;
    HIP_TRY(t.d_counts.grow(n_counts));
    if (!t.d_total) HIP_TRY(t.d_total.grow(3));
    TraceArgs a;
    a.hdr = launch_hdr(c, depth, 1u);
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.guard = c->scene.stream_guard;
    a.origins = (const float4*)d_origins, a.directions = (const float4*)d_directions, a.keys = (const uint32_t*)d_keys;
    a.out = (float*)d_out_rgb;
    a.wave_counts = t.d_counts;
    a.total = t.d_total;
    a.n = n;
    a.depth = depth;
    // warm up (warm_up: a code object's first launch on a queue, in front of the events), time, launch, sum
    RTC_TRY(warm_up(t.warmed, fn ? (const void*)fn : aot_family(c).key(), stream, [&] {
        TraceArgs w = a;
        w.n = 0u;
        return launch_trace(c, fn, 1u, stream, w);
    }));
    std::pair<Event, Event>* ev = nullptr;
    HIP_TRY(next_event_pair(t.events, t.events_used, &ev));
    HIP_TRY(hipEventRecord(ev->first, stream));
    HIP_TRY(launch_trace(c, fn, n_workgroups, stream, a));
    HIP_TRY(hipEventRecord(ev->second, stream));
    hipLaunchKernelGGL(sum_counts_kernel, dim3((uint32_t)((n_counts + SUM_COUNTS_SLICE - 1) / SUM_COUNTS_SLICE)), dim3(1024), 0, stream, t.d_counts.get(),
                       (uint32_t)n_counts, t.d_total.get(), 0ull);
    HIP_TRY(hipGetLastError());
    t.last_n = n;
    st.last = true;
    return RTC_OK;
}

// ---- ray reordering (rtc_reorder.h) ------------------------------------------------
constexpr size_t REORDER_TABLE_WORDS = (size_t)REORDER_DIGITS * REORDER_MAX_GRID + 6u;
constexpr size_t REORDER_SORT_BYTES = 16u, REORDER_GATHER_BYTES = 36u;  // per ray: DESIGN.md 8f
struct ReorderBuffers {  // the scratch block of a stream of n rays
    uint32_t *idx_a, *keys_a, *keys_b, *idx_b;  // the sort's ping-pong: the last pass leaves keys in keys_a (and the order where it is told to)
    float* colours;                             // n x 3 f32 over keys_a, keys_b, idx_b: free once the order stands in idx_a
    float4 *origins, *directions;               // gathered
    uint32_t* keys;
};
static ReorderBuffers reorder_buffers(uint8_t* base, uint32_t n) {
    ReorderBuffers b;
    b.idx_a = (uint32_t*)base, b.keys_a = b.idx_a + n, b.keys_b = b.keys_a + n, b.idx_b = b.keys_b + n;
    b.colours = (float*)b.keys_a;
    b.origins = (float4*)(base + REORDER_SORT_BYTES * n), b.directions = b.origins + n;  // (16 n bytes in: 16-byte aligned)
    b.keys = (uint32_t*)(b.directions + n);
    return b;
}
// The scratch block (grow-only; a call in flight on this stream may still be using the old one: grow frees, which waits) and the table.
static rtc_status reorder_room(rtc_ctx* c, uint32_t n, bool gathered) {
    rtc_ctx::Reorder& r = c->reorder;
    if (!r.d_table) HIP_TRY(r.d_table.grow(REORDER_TABLE_WORDS));
    const hipError_t e = r.d_scratch.grow((size_t)n * (REORDER_SORT_BYTES + (gathered ? REORDER_GATHER_BYTES : 0u)));
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (the context stays usable: the next call allocates again)
        return fail(RTC_ERR_DEVICE, "ray reordering: %zu bytes of scratch for %u rays: %s", (size_t)n * (REORDER_SORT_BYTES + REORDER_GATHER_BYTES), n,
                    hipGetErrorString(e));
    }
    return RTC_OK;
}
// Keys of the stream (box, then keys: after_keys is recorded behind them if given), then the sort: d_order[j] = the ray that comes
// j-th by key, ties by index.  Everything on `stream`, nothing read by the host.
static rtc_status reorder_sort(rtc_ctx* c, const void* d_origins, const void* d_directions, uint32_t n, const ReorderBuffers& b, uint32_t* d_order,
                               hipStream_t stream, hipEvent_t after_keys) {
    rtc_ctx::Reorder& r = c->reorder;
    uint32_t* const box = r.d_table + (size_t)REORDER_DIGITS * REORDER_MAX_GRID;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + 255u) / 256u);
    hipLaunchKernelGGL(reorder_box_init_kernel, dim3(1), dim3(64), 0, stream, box);
    hipLaunchKernelGGL(reorder_box_kernel, dim3(std::min<uint32_t>(n_tiles, 2048u)), dim3(256), 0, stream, (const float4*)d_origins, n, box);
    hipLaunchKernelGGL(reorder_keys_kernel, dim3(n_tiles), dim3(256), 0, stream, (const float4*)d_origins, (const float4*)d_directions, n, box, b.keys_a,
                       r.dir_major);
    HIP_TRY(hipGetLastError());
    if (after_keys) HIP_TRY(hipEventRecord(after_keys, stream));
    const ReorderPlan plan = reorder_plan(n, (uint32_t)compute_units(c));
    const uint32_t* keys_in = b.keys_a;
    const uint32_t* idx_in = nullptr;  // (the first pass: element i is ray i)
    for (uint32_t pass = 0; pass < REORDER_PASSES; pass++) {
        const bool to_b = (pass & 1u) == 0u;
        uint32_t* const keys_out = to_b ? b.keys_b : b.keys_a;
        uint32_t* const idx_out = pass + 1u == REORDER_PASSES ? d_order : to_b ? b.idx_b : b.idx_a;
        hipLaunchKernelGGL(reorder_count_kernel, dim3(plan.grid), dim3(256), 0, stream, keys_in, n, plan.segment, 8u * pass, r.d_table.get());
        hipLaunchKernelGGL(reorder_scan_kernel, dim3(1), dim3(1024), 0, stream, r.d_table.get(), REORDER_DIGITS * plan.grid);
        hipLaunchKernelGGL(reorder_scatter_kernel, dim3(plan.grid), dim3(256), 0, stream, keys_in, idx_in, n, plan.segment, 8u * pass,
                           (const uint32_t*)r.d_table.get(), keys_out, idx_out);
        keys_in = keys_out, idx_in = idx_out;
    }
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

extern "C" {

rtc_status rtc_ctx_trace(rtc_ctx* c, int32_t depth, const void* d_origins, const void* d_directions, const void* d_keys, uint32_t n,
                         void* d_out_rgb, void* stream_) {
    RTC_TRY(trace_args_ok("rtc_ctx_trace", c, depth, d_origins, d_directions, d_keys, n, d_out_rgb));
    if (n == 0u) return RTC_OK;
    HIP_TRY(hipSetDevice(c->device));
    return trace_launch(c, depth, d_origins, d_directions, d_keys, n, d_out_rgb, (hipStream_t)stream_);
}

rtc_status rtc_ctx_ray_order(rtc_ctx* c, const void* d_origins, const void* d_directions, uint32_t n, void* d_order_u32, void* stream_) {
    if (n > 0u && (!d_origins || !d_directions)) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_ray_order: null ray buffer");
    if (n > 0u && !d_order_u32) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_ray_order: null output buffer");
    if (((uintptr_t)d_origins & 15u) || ((uintptr_t)d_directions & 15u))
        return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_ray_order: origins and directions must be 16-byte aligned");
    if ((uintptr_t)d_order_u32 & 3u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_ray_order: output must be 4-byte aligned");
    if (n == 0u) return RTC_OK;  // nothing to order, whatever the context
    if (!c) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_ray_order: ctx is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    RTC_TRY(reorder_room(c, n, false));
    return reorder_sort(c, d_origins, d_directions, n, reorder_buffers(c->reorder.d_scratch, n), (uint32_t*)d_order_u32, stream, nullptr);
}

rtc_status rtc_ctx_trace_reordered(rtc_ctx* c, int32_t depth, const void* d_origins, const void* d_directions, const void* d_keys, uint32_t n,
                                   void* d_out_rgb, void* stream_) {
    RTC_TRY(trace_args_ok("rtc_ctx_trace_reordered", c, depth, d_origins, d_directions, d_keys, n, d_out_rgb));
    if (n == 0u) return RTC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    rtc_ctx::Reorder& r = c->reorder;
    RTC_TRY(reorder_room(c, n, true));
    for (Event& e : r.ev) HIP_TRY(e.create());
    const ReorderBuffers b = reorder_buffers(r.d_scratch, n);
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u)), block(256);
    HIP_TRY(hipEventRecord(r.ev[0], stream));
    RTC_TRY(reorder_sort(c, d_origins, d_directions, n, b, b.idx_a, stream, r.ev[1]));
    HIP_TRY(hipEventRecord(r.ev[2], stream));
    hipLaunchKernelGGL(reorder_gather_kernel, grid, block, 0, stream, (const float4*)d_origins, (const float4*)d_directions, (const uint32_t*)d_keys,
                       (const uint32_t*)b.idx_a, n, b.origins, b.directions, b.keys);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r.ev[3], stream));
    RTC_TRY(trace_launch(c, depth, b.origins, b.directions, b.keys, n, b.colours, stream));
    HIP_TRY(hipEventRecord(r.ev[4], stream));
    hipLaunchKernelGGL(reorder_scatter_colours_kernel, grid, block, 0, stream, (const float*)b.colours, (const uint32_t*)b.idx_a, n, (float*)d_out_rgb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r.ev[5], stream));
    r.last_n = n;
    r.ran = true;
    return RTC_OK;
}

// Waits for the device, as rtc_ctx_stats does.
rtc_status rtc_ctx_reorder_stats(rtc_ctx* c, rtc_reorder_stats* out) {
    if (!c || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_reorder_stats: null argument");
    std::memset(out, 0, sizeof(*out));
    const rtc_ctx::Reorder& r = c->reorder;
    if (!r.ran) return RTC_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    out->n = r.last_n;
    float* const ms[5] = {&out->keys_ms, &out->sort_ms, &out->gather_ms, &out->trace_ms, &out->scatter_ms};
    for (int k = 0; k < 5; k++) HIP_TRY(hipEventElapsedTime(ms[k], r.ev[k], r.ev[k + 1]));
    return RTC_OK;
}

// Diagnostic (not in rtc.h; tests/test_reorder_boundary.py, no device needed): rtc_reorder.h's reorder_key -- the function the key
// kernel calls -- on host buffers in rtc_ctx_trace's layout (n x 4 f32), with the stream box it is taken against in box_out
// {lo x, y, z, hi x, y, z}.  Either output may be NULL.
void rtc_diag_ray_keys(const float* origins, const float* directions, uint32_t n, float* box_out, uint32_t* keys_out) {
    const float inf = REORDER_FLT_MAX * 2.0f;
    ReorderBox box = {{inf, inf, inf}, {-inf, -inf, -inf}};
    for (uint64_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const float x = origins[4u * i + a];
            if (!reorder_finite(x)) continue;
            if (x < box.lo[a]) box.lo[a] = x;
            if (x > box.hi[a]) box.hi[a] = x;
        }
    for (int a = 0; box_out && a < 3; a++) box_out[a] = box.lo[a], box_out[3 + a] = box.hi[a];
    bool dir_major = !REORDER_ORIGIN_MAJOR;
    if (const char* e = RTC_DEV_ENV("RTC_AMD_REORDER_DIR_MAJOR")) dir_major = *e && e[0] != '0';
    for (uint64_t i = 0; keys_out && i < n; i++)
        keys_out[i] = reorder_key(box, origins[4u * i], origins[4u * i + 1u], origins[4u * i + 2u], directions[4u * i], directions[4u * i + 1u],
                                  directions[4u * i + 2u], dir_major);
}

// Diagnostic (not in rtc.h): the sort's plan for n rays on a device of n_cus compute units, out = {grid, segment, sub-tile}: workgroup
// w of `grid` owns elements [w * segment, min(n, (w + 1) * segment)) and walks them `sub-tile` at a time.  -> grid.
uint32_t rtc_diag_reorder_plan(uint32_t n, uint32_t n_cus, uint32_t* out) {
    const ReorderPlan p = reorder_plan(n, n_cus);
    if (out) out[0] = p.grid, out[1] = p.segment, out[2] = REORDER_TILE;
    return p.grid;
}

rtc_status rtc_ctx_camera_rays(rtc_ctx* c, const rtc_camera* camera, uint32_t y0, uint32_t n_rows, void* d_origins, void* d_directions, void* d_keys,
                               void* stream_) {
    if (!camera) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: camera is NULL");
    if (((uintptr_t)d_origins & 15u) || ((uintptr_t)d_directions & 15u))
        return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: origins and directions must be 16-byte aligned");
    if ((uintptr_t)d_keys & 3u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: keys must be 4-byte aligned");
    if (camera->width == 0 || camera->height == 0) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: empty canvas");
    if ((uint64_t)y0 + n_rows > camera->height) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: rows [%u, %u + %u) of %u", y0, y0, n_rows, camera->height);
    if ((uint64_t)n_rows * camera->width > 0xffffffffull) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: %u rows of %u rays are more than 2^32 - 1", n_rows, camera->width);
    if (!is_affine(camera->inv)) return fail(RTC_ERR_UNSUPPORTED, "camera inverse transform is not affine");
    if (!c) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_camera_rays: ctx is NULL");
    if (n_rows == 0u || (!d_origins && !d_directions && !d_keys)) return RTC_OK;
    HIP_TRY(hipSetDevice(c->device));
    CameraRaysArgs a;
    std::memset(&a.hdr, 0, sizeof(a.hdr));  // (has_scene_box = 0)
    // the camera as flatten packs it (rtc_scene_prep.h pack_camera)
    a.hdr.width = camera->width, a.hdr.height = camera->height;
    a.hdr.half_w = camera->half_width, a.hdr.half_h = camera->half_height, a.hdr.pixel_size = camera->pixel_size;
    std::memcpy(a.hdr.cam, camera->inv, sizeof(float) * 12);
    const float zero[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    float cam_origin[4];
    mat_vec4(camera->inv, zero, cam_origin);
    for (int k = 0; k < 3; k++) a.hdr.cam_origin[k] = cam_origin[k];
    a.origins = (float4*)d_origins, a.directions = (float4*)d_directions, a.keys = (uint32_t*)d_keys;
    a.y0 = y0, a.n_rows = n_rows;
    const uint64_t n = (uint64_t)n_rows * camera->width;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream_, a);
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

// First hits of the caller's rays (rtc_hits.h trace_hits_kernel).  As rtc_ctx_render_hits: the context's scene, none of its
// render or trace state -- no counters, no events, no warm-up bookkeeping, no names.  The argument checks in the header's
// order, all on the host.
rtc_status rtc_ctx_trace_hits(rtc_ctx* c, const void* d_origins, const void* d_directions, const void* d_keys, uint32_t n,
                              const rtc_hit_planes* d_out, void* stream_) {
    if (n > 0u && (!d_origins || !d_directions)) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: null ray buffer");
    if (n > 0u && !d_out) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: null output (no rtc_hit_planes)");
    HitPlanes planes;
    std::memset(&planes, 0, sizeof(planes));
    if (d_out && !hit_planes_view(d_out, &planes)) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: no plane requested");
    if (((uintptr_t)d_origins & 15u) || ((uintptr_t)d_directions & 15u))
        return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: origins and directions must be 16-byte aligned");
    const void* const vector_planes[] = {planes.point, planes.eye, planes.normal, planes.reflectv, planes.over_point, planes.under_point};
    for (const void* p : vector_planes)
        if ((uintptr_t)p & 15u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: the vector planes must be 16-byte aligned");
    if ((uintptr_t)planes.n1n2 & 7u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: n1n2 must be 8-byte aligned");
    const void* const scalars[] = {d_keys, planes.object, planes.distance, planes.inside, planes.light};
    for (const void* p : scalars)
        if ((uintptr_t)p & 3u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: keys and the scalar planes must be 4-byte aligned");
    if (n == 0u) return RTC_OK;  // nothing to trace, whatever the context
    if (!c) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: ctx is NULL");
    if (!c->scene.ready) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_trace_hits: no scene set");
    // (rtc_ctx_set_scene refuses RTC_JITTER_SEQUENCE lights: no resident scene has one)
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    TraceHitsArgs a;
    a.hdr = c->scene.hdr;
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.guard = c->scene.stream_guard;
    a.origins = (const float4*)d_origins, a.directions = (const float4*)d_directions, a.keys = (const uint32_t*)d_keys;
    a.planes = planes;
    a.n = n;
    const bool light = planes.light != nullptr;
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u)), block(256);
    // rtc_ctx_render_hits' families (the geometry-only kernels exist once per object-loop family)
    dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
        if (light) hipLaunchKernelGGL((trace_hits_kernel<decltype(nobj)::value, decltype(simple)::value, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((trace_hits_kernel<decltype(nobj)::value, false, false>), grid, block, 0, stream, a);
    });
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

// World::is_shadowed for the caller's pairs (rtc_hits.h shadowed_kernel); leaves the context as rtc_ctx_trace_hits does.
rtc_status rtc_ctx_is_shadowed(rtc_ctx* c, const void* d_light_positions, const void* d_points, uint32_t n, void* d_out_i32, void* stream_) {
    if (n > 0u && (!d_light_positions || !d_points)) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_is_shadowed: null pair buffer");
    if (n > 0u && !d_out_i32) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_is_shadowed: null output buffer");
    if (((uintptr_t)d_light_positions & 15u) || ((uintptr_t)d_points & 15u))
        return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_is_shadowed: light positions and points must be 16-byte aligned");
    if ((uintptr_t)d_out_i32 & 3u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_is_shadowed: output must be 4-byte aligned");
    if (n == 0u) return RTC_OK;  // nothing to answer, whatever the context
    if (!c) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_is_shadowed: ctx is NULL");
    if (!c->scene.ready) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_is_shadowed: no scene set");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    ShadowedArgs a;
    a.hdr = c->scene.hdr;
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.guard = c->scene.stream_guard;
    a.light_positions = (const float4*)d_light_positions, a.points = (const float4*)d_points;
    a.out = (int32_t*)d_out_i32;
    a.n = n;
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u)), block(256);
    dispatch_family(aot_family(c), [&](auto nobj, auto) {  // (SIMPLE is a property of intensity_at alone)
        hipLaunchKernelGGL((shadowed_kernel<decltype(nobj)::value>), grid, block, 0, stream, a);
    });
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

const char* rtc_ctx_trace_kernel_name(rtc_ctx* c) { return c ? c->scene.trace.name.c_str() : ""; }
const char* rtc_ctx_trace_kernel_id(rtc_ctx* c) { return c ? c->scene.trace.id.c_str() : ""; }

}  // extern "C"

// ---- adaptive supersampling (rtc_adaptive.h) ---------------------------------------
static_assert(ADAPTIVE_STEP == ADAPTIVE_STEP_SLOTS, "the kernel's step is the plan's");
// f(the ahead-of-time refinement kernel of the context's family and factor k)
template <class F>
static void dispatch_adaptive(rtc_ctx* c, uint32_t k, F&& f) {
    dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
        if (k == 4u) f(adaptive_refine_kernel<decltype(nobj)::value, decltype(simple)::value, 4>);
        else f(adaptive_refine_kernel<decltype(nobj)::value, decltype(simple)::value, 2>);
    });
}
// One launch of a refinement kernel, of either path: `fn`, or the ahead-of-time one `aot` names -- aot(f) calls f(that kernel), as
// [&](auto&& f) { dispatch_adaptive(c, k, f); } does
template <class Args, class Aot>
static hipError_t launch_refine(hipFunction_t fn, uint32_t n_workgroups, hipStream_t stream, Args& a, Aot&& aot) {
    return launch_scene_kernel(fn, dim3(n_workgroups), stream, a, [&] {
        aot([&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(n_workgroups), dim3(256), 0, stream, a); });
    });
}
// workgroups of the refinement kernel a compute unit holds at once (asked once per kernel, `known` by `key`; 0 from the runtime: one)
template <class Aot>
static int wgs_per_cu(std::map<const void*, int>& known, hipFunction_t fn, const void* key, Aot&& aot) {
    auto it = known.find(key);
    if (it != known.end()) return it->second;
    int n = 0;
    hipError_t e = hipSuccess;
    if (fn) e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, 0);
    else aot([&](auto kernel) { e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0); });
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || n < 1) n = 1;
    if (n > 8) n = 8;  // (a compute unit holds 32 waves)
    known[key] = n;
    return n;
}

extern "C" {

// The argument checks come first, the context's last among them: all are decided on the host, before any device call.  Between
// the three passes -- the base frame, the mask, the refinement -- nothing comes back to the host: the mask kernel is ordered
// behind the base pass by being launched on `stream` (ctx_render_slot has joined its zero-fill stream back), the refinement's
// grid does not depend on how many pixels were flagged.
rtc_status rtc_ctx_render_adaptive(rtc_ctx* c, int32_t depth, uint32_t k, float threshold, void* d_out_rgb, void* d_mask_u8, void* stream_) {
    if (!(threshold >= 0.0f) || !std::isfinite(threshold)) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: the threshold must be finite and >= 0");
    if (k != 2u && k != 4u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: supersampling factor %u: 2 or 4 rays per pixel side", k);
    if (!d_out_rgb) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: null output buffer");
    if ((uintptr_t)d_out_rgb & 3u) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: the output must be 4-byte aligned");
    if (depth < 0 || depth > RTC_MAX_DEPTH) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: depth %d outside [0, %d]", depth, RTC_MAX_DEPTH);
    if (!c) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: ctx is NULL");
    if (!c->scene.ready || c->scene.hdr.width == 0) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_render_adaptive: no scene/camera set");
    if (c->scene.lens_mode) return fail(RTC_ERR_UNSUPPORTED, "rtc_ctx_render_adaptive: a lens context renders every pixel with k x k lens rays already (adaptive lens frames are not defined)");
    if (c->scene.ss_k != 1u) return fail(RTC_ERR_UNSUPPORTED, "rtc_ctx_render_adaptive: a supersampled context renders every pixel with k x k rays already");
    rtc_camera fine;
    RTC_TRY(rtc_camera_supersampled(&c->scene.camera, k, &fine));  // (the fine frame's limits: 2^32 pixels, 2^17 rows)
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    rtc_ctx::Adaptive& ad = c->adaptive;
    rtc_ctx::Scene::Adaptive& sa = c->scene.adaptive;
    const Policy& P = c->policy;
    const uint32_t width = c->scene.hdr.width, height = c->scene.hdr.height;
    const size_t n_pixels = (size_t)width * height;
    // ---- the refinement kernel: the policy's question is asked with the frame's pixels, as the base pass asks it
    int32_t refine_depth = depth;
    if (refine_depth > RTC_STACK_DEPTH_BASE && !scene_recurses(c)) refine_depth = RTC_STACK_DEPTH_BASE;  // (as rtc_ctx_render)
    const int slot_i = k == 4u ? 1 : 0;
    SceneKernel& slot = sa.kernel[slot_i];
    const auto aot = [&](auto&& f) { dispatch_adaptive(c, k, f); };
    const bool want = !slot.variant.defs.empty() && wants_scene_kernel(P, n_pixels, c->scene.plan.compile_any_size, c->scene.plan.compile_never);
    hipFunction_t fn = nullptr;
    std::string id;
    RTC_TRY(scene_kernel_for(c, slot, refine_depth, want, false, sa.failed, sa.note, "refining with", false, &fn, &id));
    // ---- workspaces (the list: first use / a larger frame only)
    HIP_TRY(ad.d_list.grow(n_pixels));
    if (!ad.d_queue) HIP_TRY(ad.d_queue.grow(1));
    for (Event& e : ad.ev) HIP_TRY(e.create());
    const void* const kernel_key = fn ? (const void*)fn : aot_family(c).key(k);
    const uint32_t n_workgroups = adaptive_grid((uint32_t)compute_units(c), (uint32_t)wgs_per_cu(ad.wgs_per_cu, fn, kernel_key, aot), width, height, k);
    AdaptiveRefineArgs a;
    a.hdr = launch_hdr(c, refine_depth, 1u);  // (a step's counters are unpacked before the next: one ray per lane and counter)
    a.hdr.width = fine.width, a.hdr.height = fine.height, a.hdr.pixel_size = fine.pixel_size;  // (half extents and transform: the same, checked)
    a.hdr.has_scene_box = 0u;  // (rtc_adaptive.h)
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.list = ad.d_list, a.queue = ad.d_queue;
    a.out = (float*)d_out_rgb;
    a.out_width = width;
    a.depth = refine_depth;
    a.warm = 0u;
    // ---- the base frame B: the context's normal render, with its tiles, lists, feedback and stats
    RTC_TRY(rtc_ctx_render(c, depth, nullptr, d_out_rgb, stream_));
    // ---- warm up (in front of the events), mask, refinement, sum
    RTC_TRY(warm_up(ad.warmed[slot_i], kernel_key, stream, [&] {
        AdaptiveRefineArgs w = a;
        w.warm = 1u;
        return launch_refine(fn, 1u, stream, w, aot);
    }));
    HIP_TRY(hipMemsetAsync(ad.d_queue, 0, sizeof(AdaptiveQueue), stream));
    HIP_TRY(hipEventRecord(ad.ev[0], stream));
    AdaptiveMaskArgs m;
    m.frame = (const float*)d_out_rgb, m.mask = (uint8_t*)d_mask_u8, m.list = ad.d_list, m.queue = ad.d_queue;
    m.width = width, m.height = height, m.threshold = threshold;
    m.blocks_x = (width + 15u) / 16u, m.n_blocks = m.blocks_x * ((height + 15u) / 16u);
    hipLaunchKernelGGL(adaptive_mask_kernel, dim3(adaptive_mask_grid((uint32_t)compute_units(c), m.n_blocks)), dim3(256), 0, stream, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ad.ev[1], stream));
    HIP_TRY(launch_refine(fn, n_workgroups, stream, a, aot));
    HIP_TRY(hipEventRecord(ad.ev[2], stream));
    // (named once it has been launched: a call that failed on the way names no kernel it did not run)
    sa.name = fn ? slot.variant.spec_name : slot.variant.family_name;
    sa.id = fn ? id : aot_kernel_id(JitKind::ADAPTIVE, k);
    ad.ran = true;
    return RTC_OK;
}

// Waits for the device, as rtc_ctx_stats does.
rtc_status rtc_ctx_adaptive_stats(rtc_ctx* c, rtc_adaptive_stats* out) {
    if (!c || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_adaptive_stats: null argument");
    std::memset(out, 0, sizeof(*out));
    const rtc_ctx::Adaptive& ad = c->adaptive;
    if (!ad.ran) return RTC_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    AdaptiveQueue q;
    HIP_TRY(hipMemcpy(&q, ad.d_queue, sizeof(q), hipMemcpyDeviceToHost));
    out->refined_pixels = q.n_flagged;
    out->rays = q.total[0], out->shaded_hits = q.total[1], out->culled_shadow_rays = q.total[2];
    HIP_TRY(hipEventElapsedTime(&out->mask_ms, ad.ev[0], ad.ev[1]));
    HIP_TRY(hipEventElapsedTime(&out->refine_ms, ad.ev[1], ad.ev[2]));
    return RTC_OK;
}

const char* rtc_ctx_adaptive_kernel_name(rtc_ctx* c) { return c ? c->scene.adaptive.name.c_str() : ""; }
const char* rtc_ctx_adaptive_kernel_id(rtc_ctx* c) { return c ? c->scene.adaptive.id.c_str() : ""; }

// Diagnostic (not in rtc.h; tests/test_adaptive_boundary.py, no device needed): rtc_adaptive.h's adaptive_slot -- the function the
// refinement kernel calls -- for slots [first_slot, first_slot + n), {entry, sx, sy, lane} per slot into `out`, and
// rtc_launch_plan.h's adaptive_grid into *grid.  -> a wave's step, in slots; 0: k is neither 2 nor 4.
uint32_t rtc_diag_adaptive_plan(uint32_t k, uint32_t width, uint32_t height, uint32_t n_cus, uint32_t wgs_per_cu, uint64_t first_slot, uint32_t n,
                                uint32_t* out, uint32_t* grid) {
    if (k != 2u && k != 4u) return 0u;
    for (uint32_t i = 0; out && i < n; i++) {
        const AdaptiveSlot s = k == 4u ? adaptive_slot<4>(first_slot + i) : adaptive_slot<2>(first_slot + i);
        out[4 * i] = s.entry, out[4 * i + 1] = s.sx, out[4 * i + 2] = s.sy, out[4 * i + 3] = s.lane;
    }
    if (grid) *grid = adaptive_grid(n_cus, wgs_per_cu, width, height, k);
    return ADAPTIVE_STEP_SLOTS;
}

}  // extern "C"

// ---- adaptive supersampling of the one-call seam (rtc_adaptive_seam.h; rtc_render_adaptive) ---------------------
// The host-only plan of one part: its share, and how many halo rows it has -- counted band by band, not from seam_halo_row's closed
// form, which the kernels use and rtc_diag_adaptive_bands lists beside it.  One part: consecutive bands are adjacent, no halo.
static AdaptiveShare adaptive_seam_share(uint32_t width, uint32_t height, const Partition& q, uint32_t* n_halo) {
    AdaptiveShare s = {width, height, 0u, q.band_rows, q.n_parts, q.part};
    uint32_t halo = 0u;
    for_each_band(height, q, [&](uint32_t y0, uint32_t y1, uint32_t) {
        s.rows += y1 - y0;
        if (q.n_parts > 1u) halo += (y0 > 0u ? 1u : 0u) + (y1 < height ? 1u : 0u);
    });
    *n_halo = halo;
    return s;
}
// f(the ahead-of-time seam kernel of the context's family: k = 2, 4 the refinement, 1 the halo pass)
template <class F>
static void dispatch_adaptive_seam(rtc_ctx* c, uint32_t k, F&& f) {
    dispatch_family(aot_family(c), [&](auto nobj, auto simple) {
        if (k == 4u) f(adaptive_seam_kernel<decltype(nobj)::value, decltype(simple)::value, 4>);
        else if (k == 2u) f(adaptive_seam_kernel<decltype(nobj)::value, decltype(simple)::value, 2>);
        else f(adaptive_seam_kernel<decltype(nobj)::value, decltype(simple)::value, 1>);
    });
}
static std::string adaptive_seam_aot_id(uint32_t k) { return aot_kernel_id(JitKind::ADAPTIVE_SEAM, k); }  // (rtc::ctx_adaptive_seam sees rtc::aot_kernel_id first)

// Behind a base pass that ctx_render_slot has queued on `stream` for the same partition into d_share_f32: halo pass, banded mask,
// refinement, nothing coming back to the host in between.  d_out_u8 (byte mode): the share's bytes, every one of them written by the
// mask kernel or the refinement; null: the refinement writes f32 over d_share_f32.  *d_mask: the share's mask, compact like the share
// (null when not wanted or the part owns no row).  The checks of k, the threshold and the fine frame are the caller's (rtc_oneshot.hip).
rtc_status rtc::ctx_adaptive_seam(rtc_ctx* c, int32_t depth, uint32_t k, float threshold, const rtc_partition* part, void* d_share_f32, void* d_out_u8,
                                  bool want_mask, void* stream_, void** d_mask) {
    if (d_mask) *d_mask = nullptr;
    if (!c || !c->scene.ready || c->scene.ss_k != 1u || c->scene.lens_mode) return fail(RTC_ERR_INVALID_ARG, "rtc_render_adaptive: the context holds no plain scene");
    if (k != 2u && k != 4u) return fail(RTC_ERR_INVALID_ARG, "rtc_render_adaptive: supersampling factor %u: 2 or 4 rays per pixel side", k);
    rtc_camera fine;
    RTC_TRY(rtc_camera_supersampled(&c->scene.camera, k, &fine));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    rtc_ctx::AdaptiveSeam& ad = c->adaptive_seam;
    rtc_ctx::Scene::AdaptiveSeam& sa = c->scene.adaptive_seam;
    const Policy& P = c->policy;
    const Partition q = resolve(part);
    const uint32_t width = c->scene.hdr.width, height = c->scene.hdr.height;
    uint32_t n_halo = 0u;
    const AdaptiveShare share = adaptive_seam_share(width, height, q, &n_halo);
    ad.ran = false;
    ad.halo_pixels = 0u;
    if (share.rows == 0u) return RTC_OK;  // (a part that owns no row: nothing to launch, its statistics read zero)
    if (!d_share_f32) return fail(RTC_ERR_INVALID_ARG, "rtc_render_adaptive: null share buffer");
    const size_t n_share = (size_t)width * share.rows, n_halo_px = (size_t)width * n_halo;
    // ---- the kernels: the policy's question is asked with the whole frame's pixels, as the base pass asks it; the seam's rule for a
    // scene's first sighting (jit_get, lazy) as for its frame kernel
    int32_t refine_depth = depth;
    if (refine_depth > RTC_STACK_DEPTH_BASE && !scene_recurses(c)) refine_depth = RTC_STACK_DEPTH_BASE;
    const int slot_i = k == 4u ? 2 : 1;
    SceneKernel& slot = sa.kernel[slot_i];
    SceneKernel& halo_slot = sa.kernel[0];
    const auto aot = [&](auto&& f) { dispatch_adaptive_seam(c, k, f); };
    const auto halo_aot = [&](auto&& f) { dispatch_adaptive_seam(c, 1u, f); };
    const bool want = !slot.variant.defs.empty() && wants_scene_kernel(P, (uint64_t)width * height, c->scene.plan.compile_any_size, c->scene.plan.compile_never);
    const bool lazy = c->lazy_jit && P.specialise == 2;
    hipFunction_t fn = nullptr, halo_fn = nullptr;
    std::string id, halo_id;
    RTC_TRY(scene_kernel_for(c, slot, refine_depth, want, lazy, sa.failed, sa.note, "refining with", false, &fn, &id));
    if (n_halo) RTC_TRY(scene_kernel_for(c, halo_slot, refine_depth, want, lazy, sa.failed, sa.note, "refining with", false, &halo_fn, &halo_id));
    // ---- workspaces (grow-only; the caller's stream is the only one that has used them, and it is ordered)
    HIP_TRY(ad.d_list.grow(n_share));
    if (n_halo) HIP_TRY(ad.d_halo.grow(n_halo_px * 3));
    if (want_mask) HIP_TRY(ad.d_mask.grow(n_share));
    if (!ad.d_queue) HIP_TRY(ad.d_queue.grow(2));
    for (Event& e : ad.ev) HIP_TRY(e.create());
    const void* const kernel_key = fn ? (const void*)fn : aot_family(c).key(k);
    const void* const halo_key = halo_fn ? (const void*)halo_fn : aot_family(c).key(1u);
    const uint32_t n_cus = (uint32_t)compute_units(c);
    AdaptiveSeamArgs a;
    a.hdr = launch_hdr(c, refine_depth, 1u);
    a.hdr.has_scene_box = 0u;  // (rtc_adaptive.h)
    a.soa = soa_view(c->d_soa, c->scene.hdr, c->d_texels);
    a.share = share;
    a.depth = refine_depth;
    a.warm = 0u;
    AdaptiveSeamArgs h = a;  // the halo pass: the plain camera's header
    h.list = nullptr, h.queue = ad.d_queue + 1, h.out = ad.d_halo, h.out_u8 = nullptr, h.n_halo = n_halo;
    a.hdr.width = fine.width, a.hdr.height = fine.height, a.hdr.pixel_size = fine.pixel_size;
    a.list = ad.d_list, a.queue = ad.d_queue, a.out = (float*)d_share_f32, a.out_u8 = (uint8_t*)d_out_u8, a.n_halo = 0u;
    // ---- warm up (in front of the events), halo, mask, refinement
    RTC_TRY(warm_up(ad.warmed[slot_i], kernel_key, stream, [&] {
        AdaptiveSeamArgs w = a;
        w.warm = 1u;
        return launch_refine(fn, 1u, stream, w, aot);
    }));
    if (n_halo)
        RTC_TRY(warm_up(ad.warmed[0], halo_key, stream, [&] {
            AdaptiveSeamArgs w = h;
            w.warm = 1u;
            return launch_refine(halo_fn, 1u, stream, w, halo_aot);
        }));
    HIP_TRY(hipMemsetAsync(ad.d_queue, 0, 2 * sizeof(AdaptiveQueue), stream));
    HIP_TRY(hipEventRecord(ad.ev[0], stream));
    if (n_halo)
        HIP_TRY(launch_refine(halo_fn, adaptive_grid(n_cus, (uint32_t)wgs_per_cu(ad.wgs_per_cu, halo_fn, halo_key, halo_aot), width, n_halo, 1u), stream, h, halo_aot));
    AdaptiveSeamMaskArgs m;
    m.frame = (const float*)d_share_f32, m.halo = ad.d_halo, m.mask = want_mask ? ad.d_mask.get() : nullptr, m.out_u8 = (uint8_t*)d_out_u8;
    m.list = ad.d_list, m.queue = ad.d_queue, m.share = share, m.threshold = threshold;
    m.blocks_x = (width + 15u) / 16u, m.n_blocks = m.blocks_x * ((share.rows + 15u) / 16u);
    hipLaunchKernelGGL(adaptive_seam_mask_kernel, dim3(adaptive_mask_grid(n_cus, m.n_blocks)), dim3(256), 0, stream, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ad.ev[1], stream));
    HIP_TRY(launch_refine(fn, adaptive_grid(n_cus, (uint32_t)wgs_per_cu(ad.wgs_per_cu, fn, kernel_key, aot), width, share.rows, k), stream, a, aot));
    HIP_TRY(hipEventRecord(ad.ev[2], stream));
    sa.name = fn ? slot.variant.spec_name : slot.variant.family_name;
    sa.id = fn ? id : adaptive_seam_aot_id(k);
    sa.halo_name = !n_halo ? std::string() : halo_fn ? halo_slot.variant.spec_name : halo_slot.variant.family_name;
    sa.halo_id = !n_halo ? std::string() : halo_fn ? halo_id : adaptive_seam_aot_id(1u);
    ad.halo_pixels = n_halo_px;
    ad.ran = true;
    if (d_mask && want_mask) *d_mask = ad.d_mask;
    return RTC_OK;
}

// After the caller has synchronised with the stream: what the last ctx_adaptive_seam of this context did (all zero: its part owned no row).
rtc_status rtc::ctx_adaptive_seam_collect(rtc_ctx* c, rtc_seam_adaptive_stats* out) {
    std::memset(out, 0, sizeof(*out));
    const rtc_ctx::AdaptiveSeam& ad = c->adaptive_seam;
    if (!ad.ran) return RTC_OK;
    HIP_TRY(hipSetDevice(c->device));
    AdaptiveQueue q[2];
    HIP_TRY(hipMemcpy(q, ad.d_queue, sizeof(q), hipMemcpyDeviceToHost));
    out->refined_pixels = q[0].n_flagged;
    out->refine_rays = q[0].total[0];
    out->halo_pixels = ad.halo_pixels;
    out->halo_rays = q[1].total[0];
    HIP_TRY(hipEventElapsedTime(&out->mask_ms, ad.ev[0], ad.ev[1]));
    HIP_TRY(hipEventElapsedTime(&out->refine_ms, ad.ev[1], ad.ev[2]));
    return RTC_OK;
}

extern "C" {
// Diagnostics (not in rtc.h): the seam's adaptive kernels of a context's last rtc_render_adaptive -- what = 0, 1: the refinement's
// name and id; 2, 3: the halo pass's ("": no halo row) -- tests/test_gpu_seam_adaptive.py, through rtc_diag_seam_ctx.
const char* rtc_diag_ctx_adaptive_seam_kernel(rtc_ctx* c, uint32_t what) {
    if (!c) return "";
    const rtc_ctx::Scene::AdaptiveSeam& ad = c->scene.adaptive_seam;
    return what == 0u ? ad.name.c_str() : what == 1u ? ad.id.c_str() : what == 2u ? ad.halo_name.c_str() : what == 3u ? ad.halo_id.c_str() : "";
}
// ... and the host-only plan of a part (tests/test_seam_adaptive_boundary.py, no device needed): the compact-row -> frame-row map
// (seam_global_row, what the kernels call) into rows_out and the frame rows of its halo rows (seam_halo_row) into halo_out, as
// far as the caps go; counts = {rows, halo rows}, the halo rows counted band by band as the launch counts them.  band_rows 0 -> 64,
// n_parts 0 -> 1.  -> 1; 0: no such part, or an empty frame.
int32_t rtc_diag_adaptive_bands(uint32_t height, uint32_t band_rows, uint32_t n_parts, uint32_t part, uint32_t* rows_out, uint32_t rows_cap,
                                uint32_t* halo_out, uint32_t halo_cap, uint32_t counts[2]) {
    if (counts) counts[0] = counts[1] = 0u;
    const rtc_partition p = {band_rows, n_parts, part};
    const Partition q = resolve(&p);
    if (height == 0u || q.part >= q.n_parts || !counts) return 0;
    uint32_t n_halo = 0u;
    const AdaptiveShare s = adaptive_seam_share(1u, height, q, &n_halo);
    counts[0] = s.rows, counts[1] = n_halo;
    for (uint32_t i = 0; rows_out && i < s.rows && i < rows_cap; i++) rows_out[i] = seam_global_row(s, i);
    for (uint32_t i = 0; halo_out && i < n_halo && i < halo_cap; i++) halo_out[i] = seam_halo_row(s, i);
    return 1;
}
}  // extern "C"

// rtc_ctx_stats' read-out, of the renders or of the traces: waits for the device, the last launch's counters (`total`), the mean
// kernel time of the launches since the last read-out (`events`, which start over)
static rtc_status read_launch_stats(rtc_ctx* c, const unsigned long long* d_total, const EventPairs& events, size_t& events_used, const std::string& note,
                                    rtc_stats* out) {
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long total[3] = {0, 0, 0};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(total, d_total, sizeof(total), hipMemcpyDeviceToHost));
    double sum_ms = 0.0;
    HIP_TRY(sum_event_ms(events, events_used, &sum_ms));
    out->rays = total[0];
    out->shaded_hits = total[1];
    out->culled_shadow_rays = total[2];
    out->launches = (uint32_t)events_used;
    out->kernel_ms = events_used ? (float)(sum_ms / (double)events_used) : 0.0f;
    out->flags = note.empty() ? 0u : RTC_STATS_JIT_FALLBACK;
    events_used = 0;
    return RTC_OK;
}
extern "C" {
rtc_status rtc_ctx_stats(rtc_ctx* c, rtc_stats* out) {
    if (!c || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_stats: null argument");
    std::memset(out, 0, sizeof(*out));
    if (c->scene.trace.last) {  // the last launch was rtc_ctx_trace: its counters, and the traces' own events
        rtc_ctx::Trace& t = c->trace;
        out->pixels = t.last_n;
        return read_launch_stats(c, t.d_total, t.events, t.events_used, c->scene.trace.kernel.note, out);
    }
    out->rows = c->last_rows;
    out->pixels = c->last_pixels;
    if (!c->rendered) return RTC_OK;
    return read_launch_stats(c, c->d_total, c->events, c->events_used, c->scene.render.note, out);
}

const char* rtc_ctx_kernel_name(rtc_ctx* c) {
    if (!c) return "";
    if (c->wf_last) {  // the frame before this call was rendered by rtc_wavefront.h's kernels, not by the scene's per-pixel kernel
        c->wf_name = "wavefront[tree walk of " + c->scene.kernel_name + "]";
        return c->wf_name.c_str();
    }
    return c->scene.kernel_name.c_str();
}
const char* rtc_ctx_jit_status(rtc_ctx* c) { return c ? c->scene.render.note.c_str() : ""; }
const char* rtc_ctx_kernel_id(rtc_ctx* c) { return c ? c->scene.kernel_id.c_str() : ""; }

rtc_status rtc_ctx_quantize(rtc_ctx* c, const void* d_rgb, uint64_t n, void* d_out_u8, void* stream_) {
    if (!c || !d_rgb || !d_out_u8) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_quantize: null argument");
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(c->device));
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(quantize_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream_, (const float*)d_rgb, n,
                       (uint8_t*)d_out_u8);
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

uint64_t rtc_ppm_max_bytes(uint32_t width, uint32_t height) {
    // header "P3\n<w> <h>\n255\n" (<= 32 bytes) + at most 4 bytes per colour channel
    return 32ull + (uint64_t)width * height * 12ull;
}

rtc_status rtc_ctx_to_ppm(rtc_ctx* c, const void* d_rgb, uint32_t width, uint32_t height, void* d_text, uint64_t cap,
                          uint64_t* out_len, void* stream_) {
    if (!c || !d_rgb || !d_text || !out_len) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_to_ppm: null argument");
    if (width == 0 || height == 0) return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_to_ppm: empty canvas");
    if (cap < rtc_ppm_max_bytes(width, height))
        return fail(RTC_ERR_INVALID_ARG, "rtc_ctx_to_ppm: text buffer must hold rtc_ppm_max_bytes() = %llu bytes",
                    (unsigned long long)rtc_ppm_max_bytes(width, height));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t words = (3u * width + 31u) / 32u;
    HIP_TRY(c->d_ppm_rows.grow((size_t)height + 1));
    HIP_TRY(c->d_ppm_bits.grow((size_t)height * words));
    char head[40];
    const int head_len = snprintf(head, sizeof(head), "P3\n%u %u\n255\n", width, height);  // canvas.rs:60-63
    HIP_TRY(hipMemcpyAsync(d_text, head, (size_t)head_len, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(ppm_row_scan_kernel, dim3((height + 63) / 64), dim3(64), 0, stream, (const float*)d_rgb, width, height,
                       c->d_ppm_rows.get(), c->d_ppm_bits.get(), words);
    hipLaunchKernelGGL(ppm_row_offsets_kernel, dim3(1), dim3(1024), 0, stream, c->d_ppm_rows.get(), height,
                       (unsigned long long)head_len, c->d_ppm_rows + height);
    hipLaunchKernelGGL(ppm_emit_kernel, dim3((height + 3) / 4), dim3(256), 0, stream, (const float*)d_rgb, width, height,
                       c->d_ppm_rows.get(), c->d_ppm_bits.get(), words, (char*)d_text);
    HIP_TRY(hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, c->d_ppm_rows + height, sizeof(total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // `head` and `total` are host stack memory
    *out_len = total;
    return RTC_OK;
}

// ---- batched test/utility entry points (host buffers) ---------------------------
namespace {
struct DevBuf : DeviceArray<uint8_t> {  // bytes, allocated once
    hipError_t alloc(size_t n) { return grow(n ? n : 1); }
};
rtc_status begin_batch(const rtc_scene* scene, int32_t device, SceneHdr* hdr, DevBuf* soa_buf, DevBuf* tex_buf, bool allow_sequence = false) {
    int n = usable_devices();
    if (n <= 0) return fail(RTC_ERR_NO_DEVICE, "no HIP device visible; librtc_amd has no CPU fallback");
    if (device < 0 || device >= n) return fail(RTC_ERR_INVALID_ARG, "device %d out of range (have %d)", device, n);
    std::vector<float4> soa;
    std::vector<float> texels;
    rtc_status st = flatten(Policy::from_env(), scene, nullptr, hdr, &soa, &texels, nullptr, nullptr, allow_sequence);
    if (st != RTC_OK) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(soa_buf->alloc(soa.size() * sizeof(float4)));
    HIP_TRY(hipMemcpy(soa_buf->get(), soa.data(), soa.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(tex_buf->alloc(texels.size() * sizeof(float)));
    if (!texels.empty()) HIP_TRY(hipMemcpy(tex_buf->get(), texels.data(), texels.size() * sizeof(float), hipMemcpyHostToDevice));
    return RTC_OK;
}
}  // namespace

rtc_status rtc_color_at(const rtc_scene* scene, const float* origins, const float* directions, uint32_t n,
                        int32_t depth, int32_t device, float* out_rgb) {
    if (!origins || !directions || !out_rgb) return fail(RTC_ERR_INVALID_ARG, "rtc_color_at: null argument");
    if (depth < 0 || depth > RTC_STACK_DEPTH_BASE) return fail(RTC_ERR_INVALID_ARG, "rtc_color_at: depth %d outside [0, %d]", depth, RTC_STACK_DEPTH_BASE);
    if (n == 0) return RTC_OK;
    for (uint32_t i = 0; i < n; i++) {
        if (origins[i * 4 + 3] != 1.0f || directions[i * 4 + 3] != 0.0f)
            return fail(RTC_ERR_INVALID_ARG, "ray %u: origin.w must be 1 and direction.w 0", i);
    }
    SceneHdr hdr;
    DevBuf soa, tex, d_o, d_d, d_out;
    rtc_status st = begin_batch(scene, device, &hdr, &soa, &tex);
    if (st != RTC_OK) return st;
    HIP_TRY(d_o.alloc((size_t)n * 16));
    HIP_TRY(d_d.alloc((size_t)n * 16));
    HIP_TRY(d_out.alloc((size_t)n * 12));
    HIP_TRY(hipMemcpy(d_o.get(), origins, (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.get(), directions, (size_t)n * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(color_at_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, hdr,
                       soa_view((const float4*)soa.get(), hdr, (const float*)tex.get()), (const float4*)d_o.get(), (const float4*)d_d.get(), n,
                       depth, (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_rgb, d_out.get(), (size_t)n * 12, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_hit_at(const rtc_scene* scene, const float* origins, const float* directions, uint32_t n, int32_t device,
                      const rtc_hit_planes* out) {
    if (!scene || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_hit_at: null argument");
    HitPlanes host;
    if (!hit_planes_view(out, &host)) return fail(RTC_ERR_INVALID_ARG, "rtc_hit_at: no plane requested");
    if (n > 0 && (!origins || !directions)) return fail(RTC_ERR_INVALID_ARG, "rtc_hit_at: null ray buffer");
    if (n == 0) return RTC_OK;
    for (uint32_t i = 0; i < n; i++) {
        if (origins[i * 4 + 3] != 1.0f || directions[i * 4 + 3] != 0.0f)
            return fail(RTC_ERR_INVALID_ARG, "ray %u: origin.w must be 1 and direction.w 0", i);
    }
    SceneHdr hdr;
    DevBuf soa, tex, d_o, d_d, d_planes[11];
    // (a sequence-jitter light is refused by the flattening where the light plane would draw from it)
    rtc_status st = begin_batch(scene, device, &hdr, &soa, &tex, /*allow_sequence=*/host.light == nullptr);
    if (st != RTC_OK) return st;
    HIP_TRY(d_o.alloc((size_t)n * 16));
    HIP_TRY(d_d.alloc((size_t)n * 16));
    HIP_TRY(hipMemcpy(d_o.get(), origins, (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.get(), directions, (size_t)n * 16, hipMemcpyHostToDevice));
    // the planes in rtc_hit_planes' order: host pointer, bytes per element, where the device view keeps its pointer
    HitPlanes dev;
    std::memset(&dev, 0, sizeof(dev));
    struct PlaneCopy {
        void* host;
        size_t bytes;
        void** dev;
    } planes[11] = {{host.object, 4, (void**)&dev.object},      {host.distance, 4, (void**)&dev.distance},
                    {host.point, 16, (void**)&dev.point},       {host.eye, 16, (void**)&dev.eye},
                    {host.normal, 16, (void**)&dev.normal},     {host.reflectv, 16, (void**)&dev.reflectv},
                    {host.over_point, 16, (void**)&dev.over_point}, {host.under_point, 16, (void**)&dev.under_point},
                    {host.inside, 4, (void**)&dev.inside},      {host.n1n2, 8, (void**)&dev.n1n2},
                    {host.light, 4, (void**)&dev.light}};
    for (int k = 0; k < 11; k++) {
        if (!planes[k].host) continue;
        HIP_TRY(d_planes[k].alloc((size_t)n * planes[k].bytes));
        *planes[k].dev = d_planes[k].get();
    }
    hipLaunchKernelGGL(hit_at_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, hdr, soa_view((const float4*)soa.get(), hdr, (const float*)tex.get()),
                       (const float4*)d_o.get(), (const float4*)d_d.get(), n, dev);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < 11; k++)
        if (planes[k].host) HIP_TRY(hipMemcpy(planes[k].host, d_planes[k].get(), (size_t)n * planes[k].bytes, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_intensity_at(const rtc_scene* scene, const float* points, uint32_t n, int32_t device, float* out) {
    if (!points || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_intensity_at: null argument");
    if (n == 0) return RTC_OK;
    SceneHdr hdr;
    DevBuf soa, tex, d_p, d_out;
    rtc_status st = begin_batch(scene, device, &hdr, &soa, &tex, /*allow_sequence=*/true);
    if (st != RTC_OK) return st;
    HIP_TRY(d_p.alloc((size_t)n * 16));
    HIP_TRY(d_out.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_p.get(), points, (size_t)n * 16, hipMemcpyHostToDevice));
    bool simple = !hdr.has_patterns && hdr.n_objects <= 4 && !hdr.n_trav;  // (as rtc_ctx_set_scene decides it for the render kernels)
    for (uint32_t i = 0; simple && i < hdr.n_objects; i++) simple = simple_shape(shape_bits(scene->objects[i]));
    const auto kernel = simple ? intensity_at_kernel_simple : (hdr.n_objects <= 4 && !hdr.n_trav) ? intensity_at_kernel : intensity_at_kernel_generic;
    hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, hdr, soa_view((const float4*)soa.get(), hdr, (const float*)tex.get()),
                       (const float4*)d_p.get(), n, (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_point_on_light(const rtc_light* light, const int32_t* cells_uv, uint32_t n, int32_t device, float* out) {
    if (!light || !cells_uv || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_point_on_light: null argument");
    if (light->kind != RTC_LIGHT_RECT) return fail(RTC_ERR_INVALID_ARG, "rtc_point_on_light: not a rectangle light");
    if (n == 0) return RTC_OK;
    for (uint32_t i = 0; i < n; i++)
        if (cells_uv[2 * i] < 0 || cells_uv[2 * i] >= light->u_steps || cells_uv[2 * i + 1] < 0 || cells_uv[2 * i + 1] >= light->v_steps)
            return fail(RTC_ERR_INVALID_ARG, "rtc_point_on_light: cell %u (%d, %d) outside the light's %d x %d", i, cells_uv[2 * i], cells_uv[2 * i + 1],
                        light->u_steps, light->v_steps);
    rtc_scene sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.light = light;
    SceneHdr hdr;
    DevBuf soa, tex, d_c, d_out;
    rtc_status st = begin_batch(&sc, device, &hdr, &soa, &tex, /*allow_sequence=*/true);
    if (st != RTC_OK) return st;
    HIP_TRY(d_c.alloc((size_t)n * 8));
    HIP_TRY(d_out.alloc((size_t)n * 16));
    HIP_TRY(hipMemcpy(d_c.get(), cells_uv, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(point_on_light_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, hdr, (const int2*)d_c.get(), n, (float4*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 16, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_is_shadowed(const rtc_scene* scene, const float* light_positions, const float* points, uint32_t n,
                           int32_t device, int32_t* out) {
    if (!light_positions || !points || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_is_shadowed: null argument");
    if (n == 0) return RTC_OK;
    SceneHdr hdr;
    DevBuf soa, tex, d_l, d_p, d_out;
    rtc_status st = begin_batch(scene, device, &hdr, &soa, &tex);
    if (st != RTC_OK) return st;
    HIP_TRY(d_l.alloc((size_t)n * 16));
    HIP_TRY(d_p.alloc((size_t)n * 16));
    HIP_TRY(d_out.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_l.get(), light_positions, (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_p.get(), points, (size_t)n * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(is_shadowed_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, hdr,
                       soa_view((const float4*)soa.get(), hdr, (const float*)tex.get()), (const float4*)d_l.get(), (const float4*)d_p.get(), n,
                       (int32_t*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_powf(const float* x, const float* y, uint32_t n, int32_t device, float* out) {
    if (!x || !y || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_powf: null argument");
    if (n == 0) return RTC_OK;
    int nd = usable_devices();
    if (nd <= 0) return fail(RTC_ERR_NO_DEVICE, "no HIP device visible; librtc_amd has no CPU fallback");
    if (device < 0 || device >= nd) return fail(RTC_ERR_INVALID_ARG, "device %d out of range (have %d)", device, nd);
    HIP_TRY(hipSetDevice(device));
    DevBuf d_x, d_y, d_out;
    HIP_TRY(d_x.alloc((size_t)n * 4));
    HIP_TRY(d_y.alloc((size_t)n * 4));
    HIP_TRY(d_out.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_x.get(), x, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_y.get(), y, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(powf_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d_x.get(), (const float*)d_y.get(), n,
                       (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_cosf(const float* x, uint32_t n, int32_t device, float* out) {
    if (!x || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_cosf: null argument");
    if (n == 0) return RTC_OK;
    rtc_status st = select_device(device);
    if (st != RTC_OK) return st;
    DevBuf d_x, d_out;
    HIP_TRY(d_x.alloc((size_t)n * 4));
    HIP_TRY(d_out.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_x.get(), x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(cosf_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d_x.get(), n, (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_atan2f(const float* y, const float* x, uint32_t n, int32_t device, float* out) {
    if (!x || !y || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_atan2f: null argument");
    if (n == 0) return RTC_OK;
    rtc_status st = select_device(device);
    if (st != RTC_OK) return st;
    DevBuf d_x, d_y, d_out;
    HIP_TRY(d_x.alloc((size_t)n * 4));
    HIP_TRY(d_y.alloc((size_t)n * 4));
    HIP_TRY(d_out.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_x.get(), x, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_y.get(), y, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(atan2f_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d_y.get(), (const float*)d_x.get(), n,
                       (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}
rtc_status rtc_acosf(const float* x, uint32_t n, int32_t device, float* out) {
    if (!x || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_acosf: null argument");
    if (n == 0) return RTC_OK;
    rtc_status st = select_device(device);
    if (st != RTC_OK) return st;
    DevBuf d_x, d_out;
    HIP_TRY(d_x.alloc((size_t)n * 4));
    HIP_TRY(d_out.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_x.get(), x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(acosf_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d_x.get(), n, (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}

// One object's geometry as a kernel argument for the batched shape / pattern entry points.
static rtc_status object_arg(const rtc_object* object, const char* who, Obj* ob, DevBuf* d_tri) {
    rtc_object unit;
    if (!object) {  // an untransformed unit sphere
        std::memset(&unit, 0, sizeof(unit));
        unit.kind = RTC_SPHERE;
        unit.casts_shadow = 1;
        unit.min_y = -INFINITY;
        unit.max_y = INFINITY;
        for (int i = 0; i < 4; i++) unit.inv[i * 5] = 1.0f;
        object = &unit;
    }
    if (object->kind < RTC_SPHERE || object->kind > RTC_TRIANGLE)
        return fail(RTC_ERR_UNSUPPORTED, "%s: shape kind %d is not on the device path", who, object->kind);
    if (!is_affine(object->inv)) return fail(RTC_ERR_UNSUPPORTED, "%s: inverse transform is not affine", who);
    float4 g[4];
    pack_geometry(*object, g);
    ob->geo = g[0];
    ob->off0 = g[1];
    ob->off1 = g[2];
    ob->off2 = g[3];
    ob->trn = make_float4(object->inv[3], object->inv[7], object->inv[11], 0.0f);
    std::memcpy(&ob->bits, &g[0].w, 4);
    float4 tri[3] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
    if (object->kind == RTC_TRIANGLE) pack_triangle(*object, tri);
    HIP_TRY(d_tri->alloc(sizeof(tri)));
    HIP_TRY(hipMemcpy(d_tri->get(), tri, sizeof(tri), hipMemcpyHostToDevice));
    return RTC_OK;
}

rtc_status rtc_local_intersect(const rtc_object* object, const float* origins, const float* directions, uint32_t n,
                               int32_t device, float* out_t, int32_t* out_count) {
    if (!object || !origins || !directions || !out_t || !out_count)
        return fail(RTC_ERR_INVALID_ARG, "rtc_local_intersect: null argument");
    Obj ob;
    DevBuf d_tri;
    rtc_status st = select_device(device);
    if (st != RTC_OK) return st;
    if ((st = object_arg(object, "rtc_local_intersect", &ob, &d_tri)) != RTC_OK) return st;
    if (n == 0) return RTC_OK;
    DevBuf d_o, d_d, d_t, d_c;
    HIP_TRY(d_o.alloc((size_t)n * 16));
    HIP_TRY(d_d.alloc((size_t)n * 16));
    HIP_TRY(d_t.alloc((size_t)n * 16));
    HIP_TRY(d_c.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_o.get(), origins, (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.get(), directions, (size_t)n * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(local_intersect_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, ob, (const float4*)d_tri.get(), (const float4*)d_o.get(),
                       (const float4*)d_d.get(), n, (float4*)d_t.get(), (int32_t*)d_c.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_t, d_t.get(), (size_t)n * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_count, d_c.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_normal_at(const rtc_object* object, const float* world_points, uint32_t n, int32_t device, float* out) {
    if (!object || !world_points || !out) return fail(RTC_ERR_INVALID_ARG, "rtc_normal_at: null argument");
    Obj ob;
    DevBuf d_tri;
    rtc_status st = select_device(device);
    if (st != RTC_OK) return st;
    if ((st = object_arg(object, "rtc_normal_at", &ob, &d_tri)) != RTC_OK) return st;
    if (n == 0) return RTC_OK;
    DevBuf d_p, d_out;
    HIP_TRY(d_p.alloc((size_t)n * 16));
    HIP_TRY(d_out.alloc((size_t)n * 16));
    HIP_TRY(hipMemcpy(d_p.get(), world_points, (size_t)n * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(normal_at_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, ob, (const float4*)d_tri.get(), (const float4*)d_p.get(), n,
                       (float4*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 16, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_pattern_color_at(const rtc_pattern* pattern, const rtc_object* object, const float* world_points,
                                uint32_t n, int32_t device, float* out_rgb) {
    if (!pattern || !world_points || !out_rgb) return fail(RTC_ERR_INVALID_ARG, "rtc_pattern_color_at: null argument");
    if (pattern->kind < RTC_PATTERN_STRIPES || pattern->kind > RTC_PATTERN_CUBE_MAP)
        return fail(RTC_ERR_UNSUPPORTED, "rtc_pattern_color_at: pattern kind %d is not on the device path", pattern->kind);
    if (!is_affine(pattern->inv)) return fail(RTC_ERR_UNSUPPORTED, "rtc_pattern_color_at: pattern inverse transform is not affine");
    Obj ob;
    DevBuf d_tri;
    rtc_status st = select_device(device);
    if (st != RTC_OK) return st;
    if ((st = object_arg(object, "rtc_pattern_color_at", &ob, &d_tri)) != RTC_OK) return st;
    if (n == 0) return RTC_OK;
    float4 rec[5];
    pack_pattern(*pattern, rec);
    std::vector<float4> uvrec;
    std::vector<float> texels;
    std::vector<std::pair<const float*, size_t>> seen;
    if (pattern->kind >= RTC_PATTERN_TEXTURE_MAP && (st = pack_texture_map(*pattern, rec, &uvrec, &texels, &seen)) != RTC_OK) return st;
    DevBuf d_pat, d_p, d_out, d_uv, d_tex;
    HIP_TRY(d_uv.alloc(uvrec.size() * sizeof(float4)));
    HIP_TRY(d_tex.alloc(texels.size() * sizeof(float)));
    if (!uvrec.empty()) HIP_TRY(hipMemcpy(d_uv.get(), uvrec.data(), uvrec.size() * sizeof(float4), hipMemcpyHostToDevice));
    if (!texels.empty()) HIP_TRY(hipMemcpy(d_tex.get(), texels.data(), texels.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(d_pat.alloc(sizeof(rec)));
    HIP_TRY(d_p.alloc((size_t)n * 16));
    HIP_TRY(d_out.alloc((size_t)n * 12));
    HIP_TRY(hipMemcpy(d_pat.get(), rec, sizeof(rec), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_p.get(), world_points, (size_t)n * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pattern_color_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, ob, (const float4*)d_pat.get(),
                       (const float4*)d_uv.get(), (const float*)d_tex.get(), (const float4*)d_p.get(), n, (float*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_rgb, d_out.get(), (size_t)n * 12, hipMemcpyDeviceToHost));
    return RTC_OK;
}

// Host compile of the same powf restatement (diagnostic: lets the CPU test
// suite pin the algorithm against the C library without a GPU).  Not used by
// any render path.
void rtc_powf_host(const float* x, const float* y, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; i++) out[i] = powf_glibc(x[i], y[i], h_pow_log2_tab, h_exp2f_tab);
}

// Same for the cosf restatement (pattern/sine_2d.rs:40).
void rtc_cosf_host(const float* x, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; i++) out[i] = cosf_glibc(x[i], h_sincosf_tab, h_inv_pio4);
}

// Same for atan2f / acosf (pattern/uv.rs:108,115).
void rtc_atan2f_host(const float* y, const float* x, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; i++) out[i] = atan2f_glibc(y[i], x[i]);
}
void rtc_acosf_host(const float* x, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; i++) out[i] = acosf_glibc(x[i]);
}

// Diagnostic (not in rtc.h): runs fastmath_selftest_kernel on n host vectors (n*3 f32);
// counts[0] = vectors inside the core range, counts[1] = mismatches against sqrtf and '/'.
rtc_status rtc_selftest_fastmath(const float* vectors, uint32_t n, int32_t device, uint32_t counts[2]) {
    if (!vectors || !counts) return fail(RTC_ERR_INVALID_ARG, "rtc_selftest_fastmath: null argument");
    int nd = usable_devices();
    if (nd <= 0) return fail(RTC_ERR_NO_DEVICE, "no HIP device visible; librtc_amd has no CPU fallback");
    if (device < 0 || device >= nd) return fail(RTC_ERR_INVALID_ARG, "device %d out of range (have %d)", device, nd);
    HIP_TRY(hipSetDevice(device));
    DevBuf d_v, d_out;
    HIP_TRY(d_v.alloc((size_t)n * 12));
    HIP_TRY(d_out.alloc(8));
    HIP_TRY(hipMemcpy(d_v.get(), vectors, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_out.get(), 0, 8));
    if (n)
        hipLaunchKernelGGL(fastmath_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d_v.get(), n,
                           (uint32_t*)d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(counts, d_out.get(), 8, hipMemcpyDeviceToHost));
    return RTC_OK;
}

}  // extern "C"
