// rtc_scene_prep.h -- getting a scene ready, on the host: rtc_scene + rtc_camera become the kernel's header and records
// (flatten and its stages: object records, triangle pre-culling boxes, the traversal stream, scene box and region, light,
// camera), and the resident records decide which kernel renders them (plan_scene: tile coverages, scene rectangle, the
// option list and name of the scene's kernel; render_variant / trace_variant / refine_variant / deep_variant: those of the
// supersampling, ray-stream, refinement and deep-recursion kernels derived from it).  This is where the arguments of ERROR_BUDGET.md (B6, B7, B8, B10, E1, E2)
// become numbers.  No device, no context: rtc_device.hip's rtc_ctx_set_scene uploads what flatten packed and copies a
// ScenePlan into the context; tests/test_scene_prep.py reaches both through rtc_diag_scene_plan.
// Included after rtc_kernel_core.h (SceneHdr, SceneSoA, the SHAPE_* / TRAV_* constants).
#ifndef RTC_SCENE_PREP_H
#define RTC_SCENE_PREP_H

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rtc_internal.h"
#include "rtc_jit.h"

namespace rtc {

#define RTC_TRY(expr)                \
    do {                             \
        rtc_status s_ = (expr);      \
        if (s_ != RTC_OK) return s_; \
    } while (0)

inline uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
inline float float_of(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

inline uint32_t padded_count(uint32_t n) { return n ? (n + 7u) & ~7u : 8u; }

inline rtc_status check_tuple(const float v[4], float w, const char* what) {
    if (v[3] != w) return fail(RTC_ERR_INVALID_ARG, "%s: w component must be %g (got %g)", what, (double)w, (double)v[3]);
    return RTC_OK;
}

// The four geometry records of one object (see SceneSoA).
inline uint32_t shape_bits(const rtc_object& o) {  // an object's kind / flags word (geo[i].w)
    uint32_t bits = (uint32_t)o.kind | (o.casts_shadow ? SHAPE_CASTS : 0u) | (o.closed ? SHAPE_CLOSED : 0u);
    if (o.inv[1] == 0.0f && o.inv[2] == 0.0f && o.inv[4] == 0.0f && o.inv[6] == 0.0f && o.inv[8] == 0.0f &&
        o.inv[9] == 0.0f) {
        bits |= SHAPE_DIAG;
        if (o.inv[0] == o.inv[5] && o.inv[5] == o.inv[10]) bits |= SHAPE_UNIFORM;  // a uniform scale (shadow_fast)
    }
    return bits;
}
// what the SIMPLE kernels take: scale+translate-only, no cylinder / cone / triangle
inline bool simple_shape(uint32_t bits) {
    const uint32_t kind = bits & SHAPE_KIND_MASK;
    return (bits & SHAPE_DIAG) && kind != RTC_CYLINDER && kind != RTC_CONE && kind != RTC_TRIANGLE;
}
inline void pack_geometry(const rtc_object& o, float4 g[4]) {
    const uint32_t bits = shape_bits(o);
    g[0] = make_float4(o.inv[0], o.inv[5], o.inv[10], float_of(bits));
    g[1] = make_float4(o.inv[1], o.inv[2], o.inv[3], o.min_y);
    g[2] = make_float4(o.inv[4], o.inv[6], o.inv[7], o.max_y);
    g[3] = make_float4(o.inv[8], o.inv[9], o.inv[11], 0.0f);
}
// The three triangle records of one object (see SceneSoA::tri); e1, e2, normal as Triangle::new derives them.
inline void pack_triangle(const rtc_object& o, float4 rec[3]) {
    float e1[3], e2[3], nrm[3];
    rtc_triangle_fields(o.p1, o.p2, o.p3, e1, e2, nrm);
    rec[0] = make_float4(o.p1[0], o.p1[1], o.p1[2], nrm[0]);
    rec[1] = make_float4(e1[0], e1[1], e1[2], nrm[1]);
    rec[2] = make_float4(e2[0], e2[1], e2[2], nrm[2]);
}

// ---- triangle pre-culling (kernel side and error analysis: rtc_kernel_core.h tri_precull) ------------------------
// world = F * object + f for an object whose (affine) inverse is `inv`; false if the 3x3 part is singular
inline bool forward_affine(const float inv[16], double F[9], double f[3]) {
    const double a[9] = {inv[0], inv[1], inv[2], inv[4], inv[5], inv[6], inv[8], inv[9], inv[10]};
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    F[0] = (a[4] * a[8] - a[5] * a[7]) / det, F[1] = (a[2] * a[7] - a[1] * a[8]) / det, F[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    F[3] = (a[5] * a[6] - a[3] * a[8]) / det, F[4] = (a[0] * a[8] - a[2] * a[6]) / det, F[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    F[6] = (a[3] * a[7] - a[4] * a[6]) / det, F[7] = (a[1] * a[6] - a[0] * a[7]) / det, F[8] = (a[0] * a[4] - a[1] * a[3]) / det;
    const double t[3] = {inv[3], inv[7], inv[11]};
    for (int r = 0; r < 3; r++) f[r] = -(F[3 * r] * t[0] + F[3 * r + 1] * t[1] + F[3 * r + 2] * t[2]);
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(F[k])) return false;
    return std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]);
}
// largest and smallest singular value of a 3x3 matrix (cyclic Jacobi on A^T A)
inline void singular_range(const double a[9], double* s_max, double* s_min) {
    double m[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[3 * r + c] = a[r] * a[c] + a[3 + r] * a[3 + c] + a[6 + r] * a[6 + c];
    for (int sweep = 0; sweep < 12; sweep++)
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                if (std::fabs(m[3 * p + q]) < 1e-300) continue;
                const double th = 0.5 * std::atan2(2.0 * m[3 * p + q], m[3 * q + q] - m[3 * p + p]), c = std::cos(th), sn = std::sin(th);
                double r[9];
                for (int k = 0; k < 9; k++) r[k] = m[k];
                for (int k = 0; k < 3; k++) {  // columns p, q
                    r[3 * k + p] = c * m[3 * k + p] - sn * m[3 * k + q];
                    r[3 * k + q] = sn * m[3 * k + p] + c * m[3 * k + q];
                }
                for (int k = 0; k < 9; k++) m[k] = r[k];
                for (int k = 0; k < 3; k++) {  // rows p, q
                    r[3 * p + k] = c * m[3 * p + k] - sn * m[3 * q + k];
                    r[3 * q + k] = sn * m[3 * p + k] + c * m[3 * q + k];
                }
                for (int k = 0; k < 9; k++) m[k] = r[k];
            }
    const double e0 = std::fmax(m[0], 0.0), e1 = std::fmax(m[4], 0.0), e2 = std::fmax(m[8], 0.0);
    *s_max = std::sqrt(std::fmax(e0, std::fmax(e1, e2)));
    *s_min = std::sqrt(std::fmin(e0, std::fmin(e1, e2)));
}
// World-space extent of a bounded object; false for unbounded / unsupported ones.  `grow_y` (object units): a cylinder's
// y range widened by that much at either end (scene box: ERROR_BUDGET.md B8).
inline bool world_extent(const rtc_object& o, double lo[3], double hi[3], double grow_y = 0.0) {
    double F[9], f[3];
    if (!forward_affine(o.inv, F, f)) return false;
    double pts[8][3];
    int n = 0;
    if (o.kind == RTC_TRIANGLE) {
        for (const float* p : {o.p1, o.p2, o.p3}) pts[n][0] = p[0], pts[n][1] = p[1], pts[n][2] = p[2], n++;
    } else {
        double y0 = -1.0, y1 = 1.0;
        if (o.kind == RTC_CYLINDER || o.kind == RTC_CONE) {
            if (!std::isfinite(o.min_y) || !std::isfinite(o.max_y)) return false;
            y0 = o.min_y - grow_y, y1 = o.max_y + grow_y;
        } else if (o.kind != RTC_SPHERE && o.kind != RTC_CUBE) {
            return false;  // planes
        }
        const double rxz = o.kind == RTC_CONE ? std::fmax(std::fabs(y0), std::fabs(y1)) : 1.0;
        for (int k = 0; k < 8; k++) pts[n][0] = (k & 1) ? rxz : -rxz, pts[n][1] = (k & 2) ? y1 : y0, pts[n][2] = (k & 4) ? rxz : -rxz, n++;
    }
    for (int a = 0; a < 3; a++) lo[a] = INFINITY, hi[a] = -INFINITY;
    for (int k = 0; k < n; k++)
        for (int a = 0; a < 3; a++) {
            const double w = F[3 * a] * pts[k][0] + F[3 * a + 1] * pts[k][1] + F[3 * a + 2] * pts[k][2] + f[a];
            if (!std::isfinite(w)) return false;
            lo[a] = std::fmin(lo[a], w), hi[a] = std::fmax(hi[a], w);
        }
    return true;
}
// The pre-culling box of one triangle (see tri_precull for the derivation of P); `d_world`: bound on the distance
// between a pre-culling ray's origin and the triangle.  Leaves rec[0].w = 0 when no safe box exists.
struct TransformFacts {  // of the last object's inverse transform: the triangles of a mesh share theirs
    float inv[16];
    bool valid = false, usable = false;
    double F[9], f[3], s_max, s_min;  // object = A * world: object lengths are within [s_min, s_max] times world lengths
};
inline void triangle_box(const rtc_object& o, const float4 tri[3], double d_world, double guard, double pad_scale, TransformFacts* tf,
                         float4 rec[3]) {
    rec[0] = rec[1] = rec[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!tf->valid || std::memcmp(tf->inv, o.inv, sizeof(tf->inv)) != 0) {
        std::memcpy(tf->inv, o.inv, sizeof(tf->inv));
        tf->valid = true;
        tf->usable = forward_affine(o.inv, tf->F, tf->f);
        if (tf->usable) {
            const double A[9] = {o.inv[0], o.inv[1], o.inv[2], o.inv[4], o.inv[5], o.inv[6], o.inv[8], o.inv[9], o.inv[10]};
            singular_range(A, &tf->s_max, &tf->s_min);
            tf->usable = tf->s_min > 0.0 && std::isfinite(tf->s_max);
        }
    }
    if (!tf->usable) return;
    const double *F = tf->F, *f = tf->f, s_max = tf->s_max, s_min = tf->s_min;
    const double kappa = s_max / s_min;
    // the triangle the kernel intersects: p1, p1 + e1, p1 + e2 with the stored (f32) edges
    const double p[3][3] = {{tri[0].x, tri[0].y, tri[0].z},
                            {(double)tri[0].x + tri[1].x, (double)tri[0].y + tri[1].y, (double)tri[0].z + tri[1].z},
                            {(double)tri[0].x + tri[2].x, (double)tri[0].y + tri[2].y, (double)tri[0].z + tri[2].z}};
    auto len = [](const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    const double e1[3] = {tri[1].x, tri[1].y, tri[1].z}, e2[3] = {tri[2].x, tri[2].y, tri[2].z};
    const double e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    const double l1 = len(e1), l2 = len(e2), l3 = len(e3);
    if (!(l1 > 0.0 && l2 > 0.0 && l3 > 0.0)) return;
    auto angle_sin_half = [](double a, double b, double c) {  // sin(angle/2) at the vertex between sides a, b opposite c
        const double cosv = std::fmax(-1.0, std::fmin(1.0, (a * a + b * b - c * c) / (2.0 * a * b)));
        return std::sqrt(std::fmax(0.0, (1.0 - cosv) / 2.0));
    };
    const double sh = std::fmin(angle_sin_half(l1, l2, l3), std::fmin(angle_sin_half(l1, l3, l2), angle_sin_half(l2, l3, l1)));
    if (!(sh > 1e-3)) return;  // a sliver: its rejections are not robust at any useful padding
    const double rho = std::fmax(1.0, (l1 + l2) / l3), s_obj = std::fmax(l1, std::fmax(l2, l3));
    const double eps = 5.9604644775390625e-08;  // 2^-24
    const double d_obj = s_max * d_world;
    const double pad_obj = 4.0 * eps * rho * kappa * (8.0 * d_obj + 10.0 * s_obj) / (guard * sh);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, w[3][3];
    for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++) {
            w[k][a] = F[3 * a] * p[k][0] + F[3 * a + 1] * p[k][1] + F[3 * a + 2] * p[k][2] + f[a];
            lo[a] = std::fmin(lo[a], w[k][a]), hi[a] = std::fmax(hi[a], w[k][a]);
        }
    const double u[3] = {w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2]}, v[3] = {w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2]};
    double nrm[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double nl = len(nrm);
    if (!(nl > 0.0) || !std::isfinite(nl)) return;
    double big = 0.0;
    for (int a = 0; a < 3; a++) big = std::fmax(big, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
    // object distance >= s_min * world distance; 1e-5 of the coordinates covers the slab test's own rounding in f32
    const double pad = pad_scale * (pad_obj / s_min + 1e-5 * (big + d_world));
    if (!std::isfinite(pad)) return;
    rec[0] = make_float4((float)(lo[0] - pad), (float)(lo[1] - pad), (float)(lo[2] - pad), 1.0f);
    rec[1] = make_float4((float)(hi[0] + pad), (float)(hi[1] + pad), (float)(hi[2] + pad), 0.0f);
    rec[2] = make_float4((float)(nrm[0] / nl), (float)(nrm[1] / nl), (float)(nrm[2] / nl), 0.0f);
}

// ---- environment switches --------------------------------------------------------------------------------------------
// Every switch the library takes from the environment, read ONCE -- when a context is created (rtc_ctx_create; the
// stateless batched entry points read them per call) -- and kept with the context: a switch changed later does not reach
// a context that exists, and nothing on the launch path calls getenv.  Two classes:
//   * policy switches (always compiled in): on / off of a shortcut or a choice the library makes by itself.  None of them
//     can change an image -- every one has a whole-frame on / off test -- only how fast it is produced;
//   * development switches (RTC_DEV_ENV: compiled in only with -DRTC_DEV_SWITCHES, i.e. into librtc_amd_dev.so, which the
//     tools and a few tests load): substitute kernel source or compiler flags, pin tuning constants, or -- RTC_AMD_TRI_NAIVE --
//     deliberately break a guarantee so that a test can show it notices.  The shipped library does not even hold their names.
#ifdef RTC_DEV_SWITCHES
#define RTC_DEV_ENV(name) std::getenv(name)
#else
#define RTC_DEV_ENV(name) ((const char*)nullptr)
#endif
// Scene tiles (plan_coverage): the share of the 16 x 16 tiles of a frame of a world with planes, in percent, that must be unseen for
// the frame to be drawn from a tile list instead of the regular grid or the scene's rectangle (profiles/plane_tiles_ab.txt has the sweep).
constexpr uint32_t SCENE_TILES_UNSEEN_PCT = 20u;
struct Policy {
    int specialise = 2;  // RTC_AMD_SPECIALIZE: 0 never, 1 always (a failed compile is an error), 2 by frame size
    bool light_cull = true, dark = true, fast_shadow = true, cell_cull = true, own_blocks = true;  // RTC_AMD_LIGHT_CULL / _DARK / _FAST_SHADOW / _CELL_CULL / _OWN_BLOCKS (SceneHdr::cull_flags)
    bool bvh = true, scene_box = true, gates = true, tri_precull = true, block_list = true, quiet = false;
    // RTC_AMD_SCENE_TILES: frames as a zero-fill of the tiles nothing can be seen in + one workgroup for each of the others
    // (rtc_ctx::scene_tile_mask): 0 never, 1 where it pays (plan_coverage: SCENE_TILES_UNSEEN_PCT; sparse bounded worlds), 2 whenever any
    // tile is unseen
    int scene_tiles = 1;
    bool prune = true;    // RTC_AMD_PRUNE: groups / nodes a ray enters beyond what it still wants are left closed (for_each_object, ERROR_BUDGET.md B6)
    int clusters = -1;    // RTC_AMD_CLUSTERS: nodes over long triangle runs -- 0 never, 1 always, -1 by frame size
    int share_log2 = -1;  // RTC_AMD_SHARE_LOG2 = 0..3: lanes per pixel (log2) pinned for every frame; -1: by frame size
    int scene_rect = 1;   // RTC_AMD_SCENE_RECT: 0 never launch the scene's rectangle only, 2 whenever there is one, 1 under half the frame
    bool swizzle = true;         // RTC_AMD_SWIZZLE: a regular grid's blocks permuted within four rows (RenderArgs::swizzle)
    bool grid_feedback = true;   // RTC_AMD_GRID_FEEDBACK: ... and so do the frames of a regular grid: their blocks start longest first
    bool block_feedback = true;  // RTC_AMD_BLOCK_FEEDBACK: a block list's second and later frames go by the first one's wave times (refine_block_list)
    int wavefront = 0;    // RTC_AMD_WAVEFRONT=1: tree worlds are rendered by the level-by-level renderer (rtc_wavefront.h); default: never
    std::string jit_cache;  // RTC_AMD_JIT_CACHE=<dir>; "0" / "off": compiled kernels stay in memory; empty: <library dir>/jit_cache
    // development
    std::string jit_source, jit_flags;  // RTC_AMD_JIT_SOURCE=<path of rtc_kernel_core.h>, RTC_AMD_JIT_FLAGS="-D... -m..."
    bool jit_print = false, cluster_stats = false, tri_naive = false, block_order = true;
    int tree_waves = 0, reg_levels = 0, blocks_y = 0, block_s = -1, block_s_top = -1;  // (0 / -1: the library's own choice)
    uint32_t fill_wgs = 0u, tile_fill_wgs = 0u, cluster_min_run = 0u, cluster_leaf = 0u, area_share_waves = 0u, feedback_pct = 85u, feedback_down_pct = 40u, feedback_passes = 2u, feedback_max_s = 4u;
    double cluster_gmax = -1.0;
    int hits_tile = 0;  // RTC_AMD_HITS_TILE = 3 / 5 / 6: a wave's tile in rtc_ctx_render_hits is 8 x 8 / 32 x 2 / 64 x 1 pixels (0: the library's own choice)

    static Policy from_env() {
        Policy p;
        auto flag = [](const char* e, bool dflt) { return (e && *e) ? e[0] != '0' : dflt; };
        auto digit = [](const char* e, int lo, int hi, int dflt) { return (e && e[0] >= '0' + lo && e[0] <= '0' + hi && !e[1]) ? e[0] - '0' : dflt; };
        if (const char* e = std::getenv("RTC_AMD_SPECIALIZE")) p.specialise = !*e ? 2 : e[0] == '0' ? 0 : e[0] == '1' ? 1 : 2;
        p.light_cull = flag(std::getenv("RTC_AMD_LIGHT_CULL"), true);
        p.dark = flag(std::getenv("RTC_AMD_DARK"), true);
        p.fast_shadow = flag(std::getenv("RTC_AMD_FAST_SHADOW"), true);
        p.cell_cull = flag(std::getenv("RTC_AMD_CELL_CULL"), true);
        p.own_blocks = flag(std::getenv("RTC_AMD_OWN_BLOCKS"), true);
        p.bvh = flag(std::getenv("RTC_AMD_BVH"), true);
        p.scene_box = flag(std::getenv("RTC_AMD_SCENE_BOX"), true);
        p.gates = flag(std::getenv("RTC_AMD_GATES"), true);
        p.tri_precull = flag(std::getenv("RTC_AMD_TRI_PRECULL"), true);
        p.prune = flag(std::getenv("RTC_AMD_PRUNE"), true);
        if (const char* e = std::getenv("RTC_AMD_SCENE_TILES")) p.scene_tiles = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
        p.block_list = flag(std::getenv("RTC_AMD_BLOCK_LIST"), true);
        p.block_feedback = flag(std::getenv("RTC_AMD_BLOCK_FEEDBACK"), true);
        p.grid_feedback = flag(std::getenv("RTC_AMD_GRID_FEEDBACK"), true);
        p.swizzle = flag(std::getenv("RTC_AMD_SWIZZLE"), true);
        p.quiet = flag(std::getenv("RTC_AMD_QUIET"), false);
        if (const char* e = std::getenv("RTC_AMD_CLUSTERS")) p.clusters = *e ? (e[0] != '0' ? 1 : 0) : -1;
        p.share_log2 = digit(std::getenv("RTC_AMD_SHARE_LOG2"), 0, 3, -1);
        if (const char* e = std::getenv("RTC_AMD_SCENE_RECT")) p.scene_rect = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
        if (const char* e = std::getenv("RTC_AMD_WAVEFRONT")) p.wavefront = (*e && e[0] != '0') ? 1 : 0;
        if (const char* e = std::getenv("RTC_AMD_JIT_CACHE")) p.jit_cache = e;
        if (const char* e = RTC_DEV_ENV("RTC_AMD_JIT_SOURCE")) p.jit_source = e;
        if (const char* e = RTC_DEV_ENV("RTC_AMD_JIT_FLAGS")) p.jit_flags = e;
        p.jit_print = flag(RTC_DEV_ENV("RTC_AMD_JIT_PRINT"), false);
        p.cluster_stats = flag(RTC_DEV_ENV("RTC_AMD_CLUSTER_STATS"), false);
        p.tri_naive = flag(RTC_DEV_ENV("RTC_AMD_TRI_NAIVE"), false);
        p.block_order = flag(RTC_DEV_ENV("RTC_AMD_BLOCK_ORDER"), true);
        p.tree_waves = digit(RTC_DEV_ENV("RTC_AMD_TREE_WAVES"), 1, 8, 0);  // (0: by the scene and the frame, rtc_ctx_set_scene)
        p.reg_levels = digit(RTC_DEV_ENV("RTC_AMD_REG_LEVELS"), 0, 8, 0);
        p.blocks_y = digit(RTC_DEV_ENV("RTC_AMD_BLOCKS_Y"), 1, 8, 0);
        p.block_s = digit(RTC_DEV_ENV("RTC_AMD_BLOCK_S"), 0, 3, -1);
        p.block_s_top = digit(RTC_DEV_ENV("RTC_AMD_BLOCK_S_TOP"), 0, 3, -1);
        if (const char* e = RTC_DEV_ENV("RTC_AMD_FEEDBACK_PCT")) p.feedback_pct = std::max(1u, (uint32_t)std::atoi(e));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_FEEDBACK_DOWN_PCT")) p.feedback_down_pct = (uint32_t)std::atoi(e);
        if (const char* e = RTC_DEV_ENV("RTC_AMD_FEEDBACK_PASSES")) p.feedback_passes = std::max(1u, (uint32_t)std::atoi(e));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_AREA_SHARE_WAVES")) p.area_share_waves = (uint32_t)std::atoi(e);
        if (const char* e = RTC_DEV_ENV("RTC_AMD_FEEDBACK_MAX_S")) p.feedback_max_s = std::min(4u, (uint32_t)std::atoi(e));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_FILL_WGS")) p.fill_wgs = std::max(1u, (uint32_t)std::atoi(e));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_TILE_FILL_WGS")) p.tile_fill_wgs = std::max(1u, (uint32_t)std::atoi(e));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_CLUSTER_MIN_RUN")) p.cluster_min_run = std::max(3u, (uint32_t)std::atoi(e));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_CLUSTER_LEAF")) p.cluster_leaf = std::min(64u, std::max(2u, (uint32_t)std::atoi(e)));
        if (const char* e = RTC_DEV_ENV("RTC_AMD_CLUSTER_GMAX")) p.cluster_gmax = std::atof(e);
        p.hits_tile = digit(RTC_DEV_ENV("RTC_AMD_HITS_TILE"), 3, 6, 0);
        return p;
    }
    // The share of the frame below which a scene's rectangle is launched instead of the whole grid (rtc_ctx_render).
    float scene_rect_threshold() const { return scene_rect == 0 ? 0.0f : scene_rect == 2 ? 1.01f : 0.5f; }
};

// Lanes per pixel (RenderArgs::share_log2).  Two kinds of work can be shared between the lanes of a pixel: an area light's
// cells (intensity_at), while the frame would otherwise be fewer than ~4 waves per SIMD; and, in a tree walk, the long
// runs of leaves a divided mesh leaves at every level (for_each_leaf_shared) -- there a frame's time is that of its
// slowest wave, whatever the frame's size.  RTC_AMD_SHARE_LOG2=0..3 overrides.
// (beyond 200 k waves a first frame is better off with one lane everywhere -- mesh 4096^2, 262 k: 8.1 ms with two lanes in the mesh
// tiles, 6.3 with one; here_be_dragons 4000 x 1600, 100 k: 2.9 / 3.8 -- and the feedback finds the few tiles that want more)
inline uint32_t choose_share_log2_runs(uint64_t waves) { return waves <= 12000u ? 3u : waves <= 40000u ? 2u : waves <= 200000u ? 1u : 0u; }
inline bool has_leaf_runs(const SceneHdr& hdr) {  // a tree walk with the long runs of leaves a divided mesh leaves: lanes can split them
    return hdr.n_trav != 0u && hdr.max_leaf_run >= 16u && !(hdr.light_kind == RTC_LIGHT_RECT && hdr.u_steps * hdr.v_steps >= 8);
}
inline uint32_t choose_share_log2(const SceneHdr& hdr, uint32_t rows, const Policy& P, bool lists = true) {
    const bool area = hdr.light_kind == RTC_LIGHT_RECT && hdr.u_steps * hdr.v_steps >= 8;
    const bool runs = has_leaf_runs(hdr);
    if (!area && !runs) return 0u;
    if (P.share_log2 >= 0) return (uint32_t)P.share_log2;
    const uint64_t waves = ((uint64_t)hdr.width * rows + 63) / 64;
    // measured (tools/ab_env.py over RTC_AMD_BLOCK_S, round 3), ms with 2 / 4 / 8 lanes per pixel in the mesh tiles: here_be_dragons 1000 x 400 (6 k
    // waves) 1.33 / 0.93 / 0.77, 2000 x 800 (25 k) 1.61 / 1.41 / 1.50, 4000 x 1600 (100 k) 3.25 / 3.57 / 4.80; mesh 512 x 384
    // (3 k) 3.81 / 2.54 / 2.05, 1024^2 (16 k) 3.12 / 2.58 / 3.13, 2048^2 (65 k) 3.65 / 4.37 / 5.86, 4096^2 (262 k) 8.5 / 11.1 / 16.8
    if (runs) return choose_share_log2_runs(waves);
    // area lights, measured on soft_shadows (ms with 1 / 2 / 4 / 8 lanes per pixel): 512^2 (4 k waves) - / - / 0.119 / 0.084;
    // 1000 x 400 (6 k) - / 0.193 / 0.134 / 0.145; 700^2 (8 k) 0.396 / 0.242 / 0.158 / 0.130; 1024^2 (16 k) 0.317 / 0.204 / 0.150 / -;
    // 1536^2 (37 k) 0.346 / 0.248 / 0.308 / 0.49; 2048^2 (66 k) 0.366 / 0.38 / 0.50 / 0.81: a frame's time is its throughput or
    // its longest wave, whichever is longer, and a wave of 64 pixels x 100 samples is long
    // (`lists`: the frame's lane count is only where the feedback starts from -- rtc_device.hip refine_block_list cuts it per tile
    // from the second frame on, which pays up to larger frames: 2048^2 0.288 -> 0.250 ms, 3072^2 0.511 -> 0.525)
    const uint32_t one_lane_from = P.area_share_waves ? P.area_share_waves : (lists && P.block_feedback) ? 100000u : 50000u;
    return waves < 6144u ? 3u : waves < 24000u ? 2u : waves < one_lane_from ? 1u : 0u;
}

// An internal bounding-volume hierarchy for FLAT worlds (World.objects without GroupShapes) of many bounded objects:
// the object list is left as it is, and a traversal stream with groups of the library's own making is laid over it,
// walked by the same packet kernel as real GroupShapes.  Unlike a GroupShape's box -- which is part of the
// reference's semantics -- these boxes must never change an answer.  They cannot: every box is the hull of its
// objects' world-space bounds INFLATED by 10 % (plus an absolute epsilon), so a ray that misses a box passes at
// least 0.1 radius away from every object inside, where the exact intersection test reports a miss with a margin far
// above its rounding error -- the same argument, and the same proviso, as for light-cone culling: the
// quadratic's cancellation error grows with the ray origin's distance in radii, so the hierarchy is only built when
// no PRIMARY ray of the frame can start more than 100 radii from any object: the hull below holds the objects and the
// camera -- and, under a thin lens, the lens disc (`lens_radius` along the camera's two axes, `cam_inv` the camera's
// inverse transform).  Secondary rays start on the objects, inside the hull.  Rays that a caller brings (ray streams)
// start anywhere: the stream kernels test this very condition for each ray and open every box for a ray that fails it
// (`hull`: what they need for that -- the objects' own hull and the smallest half-axis; rtc_trace.h StreamGuard).  Ties in
// hit distance go by object index in the tree kernels, so the visiting order does not matter either.
// Eligible: scale+translate-only spheres and cubes, all of them (a plane's bounds are infinite).
struct FlatHull {
    float lo[3], hi[3], r_min;
};
inline bool build_flat_bvh(const rtc_scene* scene, const float cam_origin[4], std::vector<float4>* trav, FlatHull* hull = nullptr,
                           float lens_radius = 0.0f, const float* cam_inv = nullptr) {
    const uint32_t n = scene->n_objects;
    struct Box {
        float lo[3], hi[3];
    };
    std::vector<Box> box(n);
    float obj_lo[3] = {INFINITY, INFINITY, INFINITY}, obj_hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float r_min = INFINITY;
    for (uint32_t i = 0; i < n; i++) {
        const rtc_object& o = scene->objects[i];
        if (o.kind != RTC_SPHERE && o.kind != RTC_CUBE) return false;
        const float* m = o.inv;
        if (!(m[1] == 0.0f && m[2] == 0.0f && m[4] == 0.0f && m[6] == 0.0f && m[8] == 0.0f && m[9] == 0.0f)) return false;
        for (int a = 0; a < 3; a++) {
            const float g = m[5 * a], t = m[4 * a + 3];  // x_obj = g * x_world + t, |x_obj| <= 1 (sphere and cube alike)
            if (!(std::fabs(g) > 1e-20f) || !std::isfinite(g) || !std::isfinite(t)) return false;
            const float c = -t / g, h = 1.0f / std::fabs(g);  // world centre and half extent along this axis
            const float pad = 0.1f * h + 1e-4f * (std::fabs(c) + h);
            box[i].lo[a] = c - h - pad;
            box[i].hi[a] = c + h + pad;
            obj_lo[a] = std::fmin(obj_lo[a], c - h);
            obj_hi[a] = std::fmax(obj_hi[a], c + h);
            r_min = std::fmin(r_min, h);
        }
    }
    if (hull) {
        for (int a = 0; a < 3; a++) hull->lo[a] = obj_lo[a], hull->hi[a] = obj_hi[a];
        hull->r_min = r_min;
    }
    float all_lo[3], all_hi[3];
    for (int a = 0; a < 3; a++) {
        // where primary rays start: the camera, or the four points of the lens's rim on its axes (a NaN or infinite radius: no hierarchy)
        float reach = 0.0f;
        if (lens_radius != 0.0f && cam_inv) reach = std::fabs(lens_radius) * std::fmax(std::fabs(cam_inv[4 * a]), std::fabs(cam_inv[4 * a + 1]));
        if (!std::isfinite(reach)) return false;
        all_lo[a] = std::fmin(obj_lo[a], cam_origin[a] - reach);
        all_hi[a] = std::fmax(obj_hi[a], cam_origin[a] + reach);
    }
    float diag2 = 0.0f;
    for (int a = 0; a < 3; a++) diag2 += (all_hi[a] - all_lo[a]) * (all_hi[a] - all_lo[a]);
    // ERROR_BUDGET.md B9: a ray is turned away from a box when it misses the box padded by 10 % of the object.  That is safe
    // while (E2) no ray starts more than 100 radii -- of the object's SMALLEST axis: object-space units -- from an object, and
    // (E1) the object-space origin M p + t is good to a hundredth of the padding: 3 u (|p| + |centre|) / r <= 1e-3.
    if (!(std::sqrt(diag2) < 100.0f * r_min)) return false;
    float far_coord = 0.0f;
    for (int a = 0; a < 3; a++) far_coord = std::fmax(far_coord, std::fmax(std::fabs(all_lo[a]), std::fabs(all_hi[a])));
    if (!(far_coord <= 2.5e3f * r_min)) return false;  // 3 u * 2 * 2.5e3 = 9e-4
    // median split of the centres along the widest axis, down to two objects per group
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    struct Rec {
        static void go(std::vector<uint32_t>& ord, size_t b, size_t e, const std::vector<Box>& box, std::vector<float4>* out) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (size_t k = b; k < e; k++)
                for (int a = 0; a < 3; a++) {
                    lo[a] = std::fmin(lo[a], box[ord[k]].lo[a]);
                    hi[a] = std::fmax(hi[a], box[ord[k]].hi[a]);
                }
            const size_t head = out->size();
            float big = 0.0f;
            for (int a = 0; a < 3; a++) big = std::fmax(big, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
            out->push_back(make_float4(lo[0], lo[1], lo[2], 0.0f));
            out->push_back(make_float4(hi[0], hi[1], hi[2], 4e-3f * big));  // pruning slack, ERROR_BUDGET.md B6
            out->push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            if (e - b <= 2) {
                for (size_t k = b; k < e; k++) {
                    out->push_back(make_float4(0.0f, 0.0f, 0.0f, float_of(ord[k])));
                    out->push_back(make_float4(0.0f, 0.0f, 0.0f, TRAV_LEAF_TAG));
                    out->push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                }
            } else {
                int axis = 0;
                for (int a = 1; a < 3; a++)
                    if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
                const size_t mid = b + (e - b) / 2;
                std::nth_element(ord.begin() + b, ord.begin() + mid, ord.begin() + e, [&](uint32_t x, uint32_t y) {
                    return box[x].lo[axis] + box[x].hi[axis] < box[y].lo[axis] + box[y].hi[axis];
                });
                go(ord, b, mid, box, out);
                go(ord, mid, e, box, out);
            }
            (*out)[head].w = float_of((uint32_t)(out->size() / TRAV_STRIDE));  // skip: the entry after this subtree
        }
    };
    Rec::go(order, 0, n, box, trav);
    return true;
}

// build_flat_bvh's entry list with every box opened, for the rays of a stream that start beyond the hierarchy's reach (rtc_trace.h
// StreamGuard): infinite bounds -- aabb_hit holds for every ray of finite origin and direction, +-inf times a reciprocal that may
// itself be infinite keeps its sign -- an infinite slack and no q, so that nothing is pruned by distance either.  Skip indices, leaf
// entries and their run lengths stay: the same walk, every leaf visited.  `trav`: the list as it stands in the scene's records.
inline std::vector<float4> open_flat_bvh(const float4* trav, uint32_t n_trav) {
    std::vector<float4> open(trav, trav + (size_t)n_trav * TRAV_STRIDE);
    for (uint32_t k = 0; k < n_trav; k++) {
        float4* e = &open[(size_t)k * TRAV_STRIDE];
        if (e[1].w < 0.0f) continue;  // a leaf
        e[0].x = e[0].y = e[0].z = -INFINITY;
        e[1].x = e[1].y = e[1].z = INFINITY;
        e[1].w = INFINITY;
        e[2].x = 0.0f;
    }
    return open;
}

// A hierarchy of the library's own over every long run of boxed triangle leaves (the rings divide() leaves behind, group.rs:
// 46-73: 168 / 48 / 63 / 27 ... direct children per level of a 3 k-triangle mesh, thousands for a scanned one), written into
// the entry list as NODES -- group-like entries the kernel tells from GroupShapes by e2.w > 0 and tests with node_precull.  A
// node never changes an answer: it is passed by only when tri_precull would have skipped each triangle under it, i.e. the
// ray's line misses the hull of their padded boxes AND the ray is at more than asin(TRI_GUARD) from every one of their
// planes, which the node knows through a cone around their normals (axis a, half-angle phi: |d.a| >= sin(phi +
// asin(TRI_GUARD)) |d| implies |d.n| >= TRI_GUARD |d| for every n within phi of +-a).  The run's leaves are re-ordered
// (median splits of their boxes' centres): the tree kernels resolve equal distances by object index, not by position.
// `trav` must carry the run lengths of mark_leaf_runs; the caller marks the new list again.
inline void cluster_leaf_runs(std::vector<float4>* trav, double tri_guard, const Policy& P) {
    // (RTC_AMD_CLUSTER_MIN_RUN, _LEAF, _GMAX: development and tests)
    const uint32_t MIN_RUN = P.cluster_min_run ? P.cluster_min_run : 24u;
    const uint32_t LEAF = P.cluster_leaf ? P.cluster_leaf : 8u;  // triangles under a node of the lowest level, at most
    const double g_max = P.cluster_gmax >= 0.0 ? P.cluster_gmax : 0.85;  // a node whose cone lets fewer than ~15 % of all directions pass is not worth its test
    const size_t ne = trav->size() / TRAV_STRIDE;
    const std::vector<float4>& in = *trav;
    std::vector<float4> out;
    out.reserve(in.size() + in.size() / 4);
    std::vector<uint32_t> new_index(ne + 1, 0);
    std::vector<size_t> groups;  // new positions of the copied group entries (their skip indices are mapped at the end)
    struct Build {
        const std::vector<float4>& in;
        std::vector<float4>& out;
        double tri_guard, g_max;
        uint32_t LEAF;
        void go(std::vector<size_t>& ord, size_t b, size_t e) {
            if (e - b <= LEAF) {
                for (size_t k = b; k < e; k++)
                    for (uint32_t r = 0; r < TRAV_STRIDE; r++) out.push_back(in[TRAV_STRIDE * ord[k] + r]);
                return;
            }
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            double axis[3] = {0.0, 0.0, 0.0};
            for (size_t k = b; k < e; k++) {
                const float4 &mn = in[TRAV_STRIDE * ord[k]], &mx = in[TRAV_STRIDE * ord[k] + 1], &nr = in[TRAV_STRIDE * ord[k] + 2];
                const double a[3] = {mn.x, mn.y, mn.z}, c[3] = {mx.x, mx.y, mx.z}, n[3] = {nr.x, nr.y, nr.z};
                for (int j = 0; j < 3; j++) {
                    lo[j] = std::fmin(lo[j], a[j]), hi[j] = std::fmax(hi[j], c[j]);
                    clo[j] = std::fmin(clo[j], a[j] + c[j]), chi[j] = std::fmax(chi[j], a[j] + c[j]);
                }
                const double sgn = (n[0] * axis[0] + n[1] * axis[1] + n[2] * axis[2]) < 0.0 ? -1.0 : 1.0;  // n and -n are one plane
                for (int j = 0; j < 3; j++) axis[j] += sgn * n[j];
            }
            const double al = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
            double g = 2.0;  // sin(phi + asin(tri_guard)), or "no node"
            if (al > 1e-6) {
                double cmin = 1.0;  // cosine of the cone's half-angle
                for (size_t k = b; k < e; k++) {
                    const float4& nr = in[TRAV_STRIDE * ord[k] + 2];
                    const double nl = std::sqrt((double)nr.x * nr.x + (double)nr.y * nr.y + (double)nr.z * nr.z);
                    const double c = std::fabs(nr.x * axis[0] + nr.y * axis[1] + nr.z * axis[2]) / (al * nl);
                    cmin = std::fmin(cmin, nl > 0.5 ? c : 0.0);
                }
                const double phi = std::acos(std::fmin(1.0, cmin)) + 1e-3;  // 1e-3 rad: the records' normals are f32, so is the kernel's dot product
                const double lim = phi + std::asin(std::fmin(1.0, tri_guard));
                if (lim < 1.5) g = std::sin(lim);
            }
            const bool node = g <= g_max && std::isfinite(lo[0] + lo[1] + lo[2] + hi[0] + hi[1] + hi[2]);
            const size_t head = out.size();
            if (node) {
                float big = 0.0f;
                for (int j = 0; j < 3; j++) big = std::fmax(big, (float)std::fmax(std::fabs(lo[j]), std::fabs(hi[j])));
                // hull of boxes that are f32 already: exact.  The third record: |d.a'| >= tri_guard |d| <=> |d.a| >= g |d|
                const double scale = (tri_guard > 0.0 ? tri_guard : 1.0) / (g * al);
                out.push_back(make_float4((float)lo[0], (float)lo[1], (float)lo[2], 0.0f));
                out.push_back(make_float4((float)hi[0], (float)hi[1], (float)hi[2], 1e-3f * big));
                out.push_back(make_float4((float)(axis[0] * scale), (float)(axis[1] * scale), (float)(axis[2] * scale), 1.0f));
            }
            int ax = 0;
            for (int j = 1; j < 3; j++)
                if (chi[j] - clo[j] > chi[ax] - clo[ax]) ax = j;
            const size_t mid = b + (e - b) / 2;
            std::nth_element(ord.begin() + b, ord.begin() + mid, ord.begin() + e, [&](size_t x, size_t y) {
                const float4 &xa = in[TRAV_STRIDE * x], &xb = in[TRAV_STRIDE * x + 1], &ya = in[TRAV_STRIDE * y], &yb = in[TRAV_STRIDE * y + 1];
                const float cx = ax == 0 ? xa.x + xb.x : ax == 1 ? xa.y + xb.y : xa.z + xb.z;
                const float cy = ax == 0 ? ya.x + yb.x : ax == 1 ? ya.y + yb.y : ya.z + yb.z;
                return cx < cy || (cx == cy && x < y);
            });
            go(ord, b, mid);
            go(ord, mid, e);
            if (node) out[head].w = float_of((uint32_t)(out.size() / TRAV_STRIDE));
        }
    };
    Build build = {in, out, tri_guard, g_max, LEAF};
    for (size_t e = 0; e < ne;) {
        new_index[e] = (uint32_t)(out.size() / TRAV_STRIDE);
        if (!(in[TRAV_STRIDE * e + 1].w < 0.0f)) {  // a group
            groups.push_back(out.size() / TRAV_STRIDE);
            for (uint32_t r = 0; r < TRAV_STRIDE; r++) out.push_back(in[TRAV_STRIDE * e + r]);
            e++;
            continue;
        }
        const uint32_t w = (uint32_t)in[TRAV_STRIDE * e + 2].w, run = std::max(1u, w >> 3);
        const size_t end = std::min(ne, e + run);
        bool all_boxed = (w & 4u) != 0u;  // a mesh run: boxed triangles under one transform
        for (size_t k = e; k < end && all_boxed; k++) all_boxed = in[TRAV_STRIDE * k + 1].w == TRAV_BOXED_LEAF_TAG;
        if (all_boxed && end - e >= MIN_RUN) {
            std::vector<size_t> ord(end - e);
            for (size_t k = e; k < end; k++) ord[k - e] = k;
            build.go(ord, 0, ord.size());
        } else {
            for (size_t k = e; k < end; k++)
                for (uint32_t r = 0; r < TRAV_STRIDE; r++) out.push_back(in[TRAV_STRIDE * k + r]);
        }
        for (size_t k = e + 1; k < end; k++) new_index[k] = new_index[e];  // (nothing points into a run)
        e = end;
    }
    new_index[ne] = (uint32_t)(out.size() / TRAV_STRIDE);
    if (P.cluster_stats) {  // development
        size_t leaves = 0, nodes = 0, in_nodes = 0;
        double gsum = 0.0;
        for (size_t e = 0; e < out.size() / TRAV_STRIDE; e++) {
            if (out[TRAV_STRIDE * e + 1].w < 0.0f) leaves++;
            else if (out[TRAV_STRIDE * e + 2].w > 0.0f) {
                nodes++;
                const float4 a = out[TRAV_STRIDE * e + 2];
                gsum += tri_guard / std::sqrt((double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z);
                in_nodes += bits_of(out[TRAV_STRIDE * e].w) - e - 1;
            }
        }
        std::fprintf(stderr, "cluster_leaf_runs: %zu entries -> %zu; %zu groups, %zu leaves, %zu nodes (mean g %.3f, entries under nodes incl. nested %zu)\n",
                     ne, out.size() / TRAV_STRIDE, groups.size(), leaves, nodes, nodes ? gsum / nodes : 0.0, in_nodes);
    }
    for (size_t gpos : groups) {
        out[TRAV_STRIDE * gpos].w = float_of(new_index[std::min<size_t>(bits_of(out[TRAV_STRIDE * gpos].w), ne)]);
    }
    trav->swap(out);
}

// Every leaf entry learns how many consecutive leaf entries OF THE SAME GROUP start with it, and whether those are a MESH
// run -- boxed triangle leaves that all share one inverse transform and one kind / flags
// word, which is what the children of a parsed, transformed, divided mesh are (group.rs:39-44 bakes the group's transform
// into every child) -- see the kernel's trav_run / trav_mesh_run / trav_more, which share e2.w (it holds `more`, 0..3,
// on entry).  A run ends where a group ends: the leaves after a nested group's last child belong to rays that may not
// have entered that group at all.  Returns the longest run.
inline uint32_t mark_leaf_runs(std::vector<float4>* trav, const rtc_scene* scene) {
    const size_t ne = trav->size() / TRAV_STRIDE;
    std::vector<char> ends_subtree(ne + 1, 0);  // [e]: some group's subtree ends right before entry e
    for (size_t e = 0; e < ne; e++)
        if (!((*trav)[TRAV_STRIDE * e + 1].w < 0.0f)) {
            const uint32_t skip = bits_of((*trav)[TRAV_STRIDE * e].w);
            if (skip <= ne) ends_subtree[skip] = 1;
        }
    auto object_of = [&](size_t e) { return bits_of((*trav)[TRAV_STRIDE * e].w); };
    auto same_mesh = [&](size_t a, size_t b) {  // entry b continues the mesh run of entry a
        const uint32_t ia = object_of(a), ib = object_of(b);
        if (ia >= scene->n_objects || ib >= scene->n_objects) return false;
        const rtc_object &oa = scene->objects[ia], &ob = scene->objects[ib];
        return oa.kind == ob.kind && (oa.casts_shadow != 0) == (ob.casts_shadow != 0) && std::memcmp(oa.inv, ob.inv, sizeof(oa.inv)) == 0;
    };
    uint32_t longest = 0, run = 0;
    bool mesh = false;
    for (size_t e = ne; e-- > 0;) {
        if (!((*trav)[TRAV_STRIDE * e + 1].w < 0.0f)) {  // a group
            run = 0;
            continue;
        }
        if (ends_subtree[e + 1]) run = 0;
        const bool boxed_tri = (*trav)[TRAV_STRIDE * e + 1].w == TRAV_BOXED_LEAF_TAG && object_of(e) < scene->n_objects &&
                               scene->objects[object_of(e)].kind == RTC_TRIANGLE;
        mesh = boxed_tri && (run == 0 || (mesh && same_mesh(e, e + 1)));
        run = std::min(run + 1u, 1u << 20);
        longest = std::max(longest, run);
        float& w = (*trav)[TRAV_STRIDE * e + 2].w;
        w = (float)(8u * run + (mesh ? 4u : 0u) + ((uint32_t)w & 3u));
    }
    return longest;
}

// Appends the six `uvrec` records of one UV pattern; UVImage canvases go to `texels` (each distinct host image once).
inline rtc_status pack_uv_pattern(const rtc_uv_pattern& u, std::vector<float4>* uvrec, std::vector<float>* texels,
                                  std::vector<std::pair<const float*, size_t>>* seen) {
    if (u.kind < RTC_UV_CHECKERS || u.kind > RTC_UV_IMAGE) return fail(RTC_ERR_UNSUPPORTED, "UV pattern kind %d is not on the device path", u.kind);
    size_t first_texel = 0;
    uint32_t iw = 0, ih = 0;
    if (u.kind == RTC_UV_IMAGE) {
        if (!u.image_rgb || u.image_width == 0 || u.image_height == 0) return fail(RTC_ERR_INVALID_ARG, "UVImage without a canvas");
        iw = u.image_width;
        ih = u.image_height;
        bool found = false;
        for (auto& e : *seen)
            if (e.first == u.image_rgb) {
                first_texel = e.second;
                found = true;
            }
        if (!found) {
            first_texel = texels->size() / 3;
            texels->insert(texels->end(), u.image_rgb, u.image_rgb + (size_t)iw * ih * 3);
            seen->push_back({u.image_rgb, first_texel});
        }
        if (first_texel + (size_t)iw * ih > 0xffffffffull) return fail(RTC_ERR_UNSUPPORTED, "more than 2^32 texels");
    }
    const float (*c)[3] = u.colors;
    uvrec->push_back(make_float4(float_of((uint32_t)u.kind), u.width, u.height, float_of((uint32_t)first_texel)));
    uvrec->push_back(make_float4(float_of(iw), float_of(ih), 0.0f, 0.0f));
    uvrec->push_back(make_float4(c[0][0], c[0][1], c[0][2], c[1][0]));
    uvrec->push_back(make_float4(c[1][1], c[1][2], c[2][0], c[2][1]));
    uvrec->push_back(make_float4(c[2][2], c[3][0], c[3][1], c[3][2]));
    uvrec->push_back(make_float4(c[4][0], c[4][1], c[4][2], 0.0f));
    return RTC_OK;
}

// TextureMap / CubicMap: the pattern's second record points at its UV patterns, which are appended to `uvrec`.
inline rtc_status pack_texture_map(const rtc_pattern& pt, float4 rec[5], std::vector<float4>* uvrec, std::vector<float>* texels,
                                   std::vector<std::pair<const float*, size_t>>* seen) {
    const uint32_t want = pt.kind == RTC_PATTERN_CUBE_MAP ? 6u : 1u;
    if (pt.n_uv != want || !pt.uv) return fail(RTC_ERR_INVALID_ARG, "pattern kind %d needs %u UV pattern(s), got %u", pt.kind, want, pt.n_uv);
    if (pt.kind == RTC_PATTERN_TEXTURE_MAP && (pt.uv_mapping < RTC_MAP_SPHERICAL || pt.uv_mapping > RTC_MAP_CYLINDRICAL))
        return fail(RTC_ERR_UNSUPPORTED, "UV mapping %d is not on the device path", pt.uv_mapping);
    rec[1] = make_float4(float_of((uint32_t)pt.uv_mapping), float_of((uint32_t)(uvrec->size() / 6)), 0.0f, 0.0f);
    for (uint32_t k = 0; k < want; k++) {
        rtc_status st = pack_uv_pattern(pt.uv[k], uvrec, texels, seen);
        if (st != RTC_OK) return st;
    }
    return RTC_OK;
}
// The five pattern records of one material (see SceneSoA::pat).
inline void pack_pattern(const rtc_pattern& pt, float4 rec[5]) {
    rec[0] = make_float4(pt.a[0], pt.a[1], pt.a[2], float_of((uint32_t)pt.kind));
    // Gradient::new / Sine2D::new keep distance = b - a (gradient.rs:17, sine_2d.rs:17)
    const bool dist = pt.kind == RTC_PATTERN_GRADIENT || pt.kind == RTC_PATTERN_SINE2D;
    rec[1] = dist ? make_float4(pt.b[0] - pt.a[0], pt.b[1] - pt.a[1], pt.b[2] - pt.a[2], 0.0f)
                  : make_float4(pt.b[0], pt.b[1], pt.b[2], 0.0f);
    for (int r = 0; r < 3; r++)
        rec[2 + r] = make_float4(pt.inv[4 * r], pt.inv[4 * r + 1], pt.inv[4 * r + 2], pt.inv[4 * r + 3]);
}

// RTC_AMD_PRUNE=0: every group / node entry gets an infinite slack, with which the walks' distance test never closes one
inline void no_distance_pruning(std::vector<float4>* trav) {
    for (size_t e = 0, ne = trav->size() / TRAV_STRIDE; e < ne; e++)
        if (!((*trav)[TRAV_STRIDE * e + 1].w < 0.0f)) (*trav)[TRAV_STRIDE * e + 1].w = INFINITY;
}
// boxed triangle leaves that follow one another are pre-culled two at a time (for_each_object): mark the first of a pair
inline void mark_pairs(std::vector<float4>* trav) {
    for (size_t e = 0, ne = trav->size() / TRAV_STRIDE; e < ne; e++) {
        if ((*trav)[TRAV_STRIDE * e + 1].w != TRAV_BOXED_LEAF_TAG) continue;
        int more = 0;  // boxed leaves right after this one, up to 3
        while (more < 3 && e + more + 1 < ne && (*trav)[TRAV_STRIDE * (e + more + 1) + 1].w == TRAV_BOXED_LEAF_TAG) more++;
        (*trav)[TRAV_STRIDE * e + 2].w = (float)more;
    }
}
// What a primary ray can see at all, for the scene rectangle (plan_scene): known when every top-level entry is
// bounded -- their padded union is `box` -- or a plane, seen only by rays that point towards it.
struct SceneRegion {
    bool known = false, has_box = false;
    double box[6] = {0, 0, 0, 0, 0, 0};
    std::vector<float> entry_boxes;  // the padded boxes of the bounded top-level entries one by one (HEAVY_BOX_FLOATS each; `box` is their union)
    std::vector<std::array<double, 4>> planes;  // the plane's object-space y of a world point p: r[0] p.x + r[1] p.y + r[2] p.z + r[3]
};

// The scene buffer's columns, in float4 per padded object (padded_count; kernel side: SceneSoA), written by flatten's stages
// and read back by soa_view and plan_scene.  A pattern takes five records per object, a triangle and the light's corners
// three.  The traversal stream follows the columns, the UV pattern records (SceneHdr::uvrec_off) follow that.
enum SoaColumn : size_t {
    COL_GEO = 0, COL_OFF0 = 1, COL_OFF1 = 2, COL_OFF2 = 3, COL_MAT_A = 4, COL_MAT_B = 5, COL_MAT_C = 6,
    COL_PAT = 7, COL_TRI = 12, COL_LCORN = 15, COL_TRN = 18, COL_BSPH = 19, SOA_COLUMNS = 20
};
inline size_t soa_index(SoaColumn col, uint32_t np, size_t i, size_t records = 1) { return (size_t)col * np + records * i; }
inline uint32_t object_bits(const std::vector<float4>& soa, const SceneHdr& hdr, uint32_t i) {  // geo[i].w: shape_bits
    return bits_of(soa[soa_index(COL_GEO, padded_count(hdr.n_objects), i)].w);
}
inline SceneSoA soa_view(const float4* base, const SceneHdr& hdr, const float* d_texels) {
    const uint32_t np = padded_count(hdr.n_objects);
    SceneSoA s;
    s.uvrec = base + hdr.uvrec_off;
    s.texels = d_texels;
    s.geo = base + soa_index(COL_GEO, np, 0);
    s.off0 = base + soa_index(COL_OFF0, np, 0);
    s.off1 = base + soa_index(COL_OFF1, np, 0);
    s.off2 = base + soa_index(COL_OFF2, np, 0);
    s.mat_a = base + soa_index(COL_MAT_A, np, 0);
    s.mat_b = base + soa_index(COL_MAT_B, np, 0);
    s.mat_c = base + soa_index(COL_MAT_C, np, 0);
    s.pat = base + soa_index(COL_PAT, np, 0);
    s.tri = base + soa_index(COL_TRI, np, 0);
    s.lcorn = base + soa_index(COL_LCORN, np, 0);
    s.trn = base + soa_index(COL_TRN, np, 0);
    s.bsph = base + soa_index(COL_BSPH, np, 0);
    s.trav = base + soa_index(SOA_COLUMNS, np, 0);
    return s;
}

struct Extent {  // world_extent() of every object, computed once (a mesh leaf is asked for it by every group around it)
    double lo[3], hi[3];
    bool ok;
};
// What the stages of flatten() share; the stages are its member functions, called by flatten in the order they stand in.
struct Flatten {
    const Policy& P;
    const rtc_scene* scene;
    const rtc_camera* cam;  // null: the batched entry points
    SceneHdr* hdr;
    std::vector<float4>* soa;
    std::vector<float>* texels;
    std::vector<float>* heavy_boxes;  // optional, see flatten
    SceneRegion* region;              // optional
    bool allow_sequence;
    FlatHull* flat_hull;  // optional: filled where the world gets a hierarchy of the library's own (build_flat_bvh)
    float lens_radius;    // of the frame's thin lens, 0 without one: primary rays start on its disc (build_flat_bvh)
    // (flatten fills the eleven above, in the order of its own parameters, and the next three)
    uint32_t n = 0, np = 0;  // objects, and the stride of each column
    float cam_origin[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // camera.rs:70: origin = transform_inverse * point(0,0,0) (only with a camera)
    std::vector<Extent> extent;
    std::vector<float4> tbox;  // 3 records per object: { box.min, usable }, { box.max, 0 }, { unit normal, 0 }, world space; empty: no pre-culling
    std::vector<float4> uvrec;
    std::vector<std::pair<const float*, size_t>> seen_images;

    float4* rec(SoaColumn col, size_t i, size_t records = 1) { return &(*soa)[soa_index(col, np, i, records)]; }

    // 1. object records (geometry, bounding sphere, material, pattern, texture maps) and every object's Extent
    rtc_status pack_objects() {
        extent.resize(n);
        for (uint32_t i = n; i < np; i++) *rec(COL_GEO, i) = make_float4(0.0f, 0.0f, 0.0f, float_of((uint32_t)SHAPE_NONE));
        for (uint32_t i = 0; i < n; i++) {
            const rtc_object& o = scene->objects[i];
            if (o.kind < RTC_SPHERE || o.kind > RTC_TRIANGLE)
                return fail(RTC_ERR_UNSUPPORTED, "object %u: shape kind %d is not on the device path", i, o.kind);
            if (o.kind == RTC_TRIANGLE) pack_triangle(o, rec(COL_TRI, i, 3));
            if (!is_affine(o.inv))
                return fail(RTC_ERR_UNSUPPORTED,
                            "object %u: inverse transform's last row is not exactly [0,0,0,1] (projective transforms "
                            "are not supported)", i);
            float4 g[4];
            pack_geometry(o, g);
            *rec(COL_GEO, i) = g[0], *rec(COL_OFF0, i) = g[1], *rec(COL_OFF1, i) = g[2], *rec(COL_OFF2, i) = g[3];
            *rec(COL_TRN, i) = make_float4(o.inv[3], o.inv[7], o.inv[11], 0.0f);
            {
                double lo[3], hi[3];  // bounding sphere: around the world-space box of the shape's own bounds
                float4 bs = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
                // (a cone's near-parallel branch, cone.rs:99-107, reports roots off the bounded cone: no sphere holds its hits)
                Extent& ex = extent[i];
                ex.ok = world_extent(o, ex.lo, ex.hi);
                for (int a = 0; a < 3; a++) lo[a] = ex.lo[a], hi[a] = ex.hi[a];
                if (o.kind != RTC_CONE && ex.ok) {
                    double r2 = 0.0;
                    for (int a = 0; a < 3; a++) r2 += 0.25 * (hi[a] - lo[a]) * (hi[a] - lo[a]);
                    bs = make_float4((float)(0.5 * (lo[0] + hi[0])), (float)(0.5 * (lo[1] + hi[1])), (float)(0.5 * (lo[2] + hi[2])),
                                     (float)(1.001 * std::sqrt(r2)));
                    if (!std::isfinite(bs.x) || !std::isfinite(bs.y) || !std::isfinite(bs.z) || !std::isfinite(bs.w))
                        bs = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
                }
                *rec(COL_BSPH, i) = bs;
            }
            const rtc_material& m = o.material;
            *rec(COL_MAT_A, i) = make_float4(m.color[0], m.color[1], m.color[2], m.ambient);
            *rec(COL_MAT_B, i) = make_float4(m.diffuse, m.specular, m.shininess, m.reflective);
            *rec(COL_MAT_C, i) = make_float4(m.transparency, m.refractive_index, 0.0f, 0.0f);
            const rtc_pattern& pt = m.pattern;
            if (pt.kind != RTC_PATTERN_NONE) {
                if (pt.kind < RTC_PATTERN_STRIPES || pt.kind > RTC_PATTERN_CUBE_MAP)
                    return fail(RTC_ERR_UNSUPPORTED, "object %u: pattern kind %d is not on the device path", i, pt.kind);
                if (!is_affine(pt.inv))
                    return fail(RTC_ERR_UNSUPPORTED, "object %u: pattern inverse transform is not affine", i);
                hdr->has_patterns = 1;
                float4* pat = rec(COL_PAT, i, 5);
                pack_pattern(pt, pat);
                if (pt.kind >= RTC_PATTERN_TEXTURE_MAP) RTC_TRY(pack_texture_map(pt, pat, &uvrec, texels, &seen_images));
            }
        }
        return RTC_OK;
    }

    // 2. Triangles met by tree walks get a pre-culling box (tri_precull): the ball around everything bounded (and the camera)
    // bounds the distance between a ray's origin and a triangle; rays that start outside it do not pre-cull
    void triangle_boxes() {
        if (!(scene->n_groups && P.tri_precull)) return;
        bool any_triangle = false;
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = 0; i < n; i++) {
            any_triangle = any_triangle || scene->objects[i].kind == RTC_TRIANGLE;
            double olo[3], ohi[3];
            for (int a = 0; a < 3; a++) olo[a] = extent[i].lo[a], ohi[a] = extent[i].hi[a];
            if (extent[i].ok)
                for (int a = 0; a < 3; a++) lo[a] = std::fmin(lo[a], olo[a]), hi[a] = std::fmax(hi[a], ohi[a]);
        }
        if (cam)
            for (int a = 0; a < 3; a++) lo[a] = std::fmin(lo[a], (double)cam_origin[a]), hi[a] = std::fmax(hi[a], (double)cam_origin[a]);
        double r2 = 0.0;
        for (int a = 0; a < 3; a++) r2 += 0.25 * (hi[a] - lo[a]) * (hi[a] - lo[a]);
        if (any_triangle && std::isfinite(r2) && r2 > 0.0) {
            const double radius = 1.05 * std::sqrt(r2);  // a little room: hit points are computed, not exact
            // RTC_AMD_TRI_NAIVE=1 (tests only): no angle guard, no padding -- what tests/test_tri_precull.py must catch
            const bool naive = P.tri_naive;
            hdr->tri_guard = naive ? 0.0f : TRI_GUARD;
            hdr->has_tbox = 1;
            for (int a = 0; a < 3; a++) hdr->cull_c[a] = (float)(0.5 * (lo[a] + hi[a]));
            hdr->cull_r2 = (float)(radius * radius);
            tbox.assign(3 * (size_t)n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            TransformFacts tf;
            // ERROR_BUDGET.md B7: the padding is derived from D, the distance between a ray's origin and a triangle -- and the ray's
            // own transformation into object space is good to 3 u (|M| |origin| + |t|) (E1), which is relative to the
            // COORDINATES: a mesh a thousand of its own sizes from the world's origin moves by that much more.  D stands for both.
            double far_coord = 0.0;
            for (int a = 0; a < 3; a++) far_coord = std::fmax(far_coord, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
            const double d_bound = std::fmax(2.0 * radius, far_coord + radius);
            for (uint32_t i = 0; i < n; i++)
                if (scene->objects[i].kind == RTC_TRIANGLE)
                    triangle_box(scene->objects[i], rec(COL_TRI, i, 3), d_bound, TRI_GUARD, naive ? 0.0 : 1.0,
                                 &tf, &tbox[3 * (size_t)i]);
        }
    }

    // 3a. A flat world of many bounded objects gets a bounding-volume hierarchy of the library's own (see build_flat_bvh)
    void flat_bvh_stream() {
        if (!(cam && n >= 16 && P.bvh)) return;
        std::vector<float4> trav;
        if (build_flat_bvh(scene, cam_origin, &trav, flat_hull, lens_radius, cam->inv)) {
            hdr->max_leaf_run = mark_leaf_runs(&trav, scene);
            hdr->internal_boxes = 1;
            hdr->n_trav = (uint32_t)(trav.size() / TRAV_STRIDE);
            if (!P.prune) no_distance_pruning(&trav);
            soa->insert(soa->end(), trav.begin(), trav.end());
        }
    }

    // 3b. GroupShapes: write the depth-first traversal out as an entry list (see SceneSoA::trav)
    rtc_status group_stream() {
        if (!scene->groups) return fail(RTC_ERR_INVALID_ARG, "scene.groups is NULL");
        const std::vector<char> loose_group = mark_loose_groups();
        std::vector<float4> trav;
        std::vector<std::pair<size_t, uint32_t>> top_level;  // (entry, group) of the groups directly under the world
        bool any = false;                                    // is there a group that is not empty
        RTC_TRY(group_entry_list(loose_group, &trav, &top_level, &any));
        mark_pairs(&trav);
        hdr->max_leaf_run = mark_leaf_runs(&trav, scene);
        if (heavy_boxes) heavy_group_boxes(trav, top_level);
        cluster_long_runs(&trav);
        gates_or_stream(&trav, any);
        return RTC_OK;
    }
    // SHAPE_LOOSE: leaves that some group around them does not (safely) contain -- see the flag.  Such a group must
    // not be pruned by distance either (for_each_object assumes a group's hits lie inside its box): loose_group.
    std::vector<char> mark_loose_groups() {
        std::vector<char> loose_group(scene->n_groups, 0);
        for (uint32_t g = 0; g < scene->n_groups; g++) {
            const rtc_group& grp = scene->groups[g];
            if ((uint64_t)grp.first_object + grp.n_objects > n) continue;  // reported below
            for (uint32_t i = grp.first_object; i < grp.first_object + grp.n_objects; i++) {
                double lo[3], hi[3];
                bool inside = extent[i].ok;
                for (int a = 0; a < 3; a++) lo[a] = extent[i].lo[a], hi[a] = extent[i].hi[a];
                for (int a = 0; a < 3 && inside; a++) {
                    const double tol = 1e-5 * (std::fabs(lo[a]) + std::fabs(hi[a]) + 1.0);
                    inside = lo[a] >= (double)grp.bounds_min[a] - tol && hi[a] <= (double)grp.bounds_max[a] + tol;
                }
                // (a cone's near-parallel branch, cone.rs:99-107, reports roots of the UNBOUNDED double cone: hits outside
                // the cone's own bounds, hence outside any group box built from them)
                if (scene->objects[i].kind == RTC_CONE) loose_group[g] = 1;
                if (!inside) {
                    loose_group[g] = 1;
                    rec(COL_GEO, i)->w = float_of(bits_of(rec(COL_GEO, i)->w) | SHAPE_LOOSE);
                }
            }
        }
        return loose_group;
    }
    // the depth-first entry list: a group's box, slack and pruning margin, then what it holds; leaves carry their pre-culling box
    rtc_status group_entry_list(const std::vector<char>& loose_group, std::vector<float4>* trav_out, std::vector<std::pair<size_t, uint32_t>>* top_level_out,
                                bool* any_out) {
        struct Open {
            uint32_t end;
            size_t entry;
        };
        std::vector<float4>& trav = *trav_out;
        std::vector<std::pair<size_t, uint32_t>>& top_level = *top_level_out;
        bool& any = *any_out;
        std::vector<Open> open;
        uint32_t gi = 0;
        for (uint32_t p = 0; p <= n; p++) {
            while (!open.empty() && open.back().end == p) {  // close: skip index = next entry
                trav[TRAV_STRIDE * open.back().entry].w = float_of((uint32_t)(trav.size() / TRAV_STRIDE));
                open.pop_back();
            }
            for (;;) {
                while (gi < scene->n_groups && scene->groups[gi].n_objects == 0) gi++;  // empty groups never hit
                if (gi >= scene->n_groups || scene->groups[gi].first_object != p) break;
                const rtc_group& g = scene->groups[gi];
                const uint64_t end = (uint64_t)g.first_object + g.n_objects;
                if (end > n || (!open.empty() && end > open.back().end))
                    return fail(RTC_ERR_INVALID_ARG, "group %u: objects [%u, %u) do not nest inside the enclosing group / the world",
                                gi, g.first_object, (unsigned)end);
                if (open.empty()) top_level.push_back({trav.size() / TRAV_STRIDE, gi});
                open.push_back({(uint32_t)end, trav.size() / TRAV_STRIDE});
                float big = 0.0f;  // pruning slack: 4e-3 of the largest |coordinate| (NaN-propagating on purpose; ERROR_BUDGET.md B6)
                for (int a = 0; a < 3; a++) {
                    const float lo = std::fabs(g.bounds_min[a]), hi = std::fabs(g.bounds_max[a]);
                    big = (lo != lo || hi != hi) ? NAN : std::fmax(big, std::fmax(lo, hi));
                }
                // q of the pruning margin (kernel: for_each_object): 1e-6 over the smallest size of a sphere, cylinder or cone below
                // this group -- the unit shape under its transform is at least 1 / |inverse 3x3| (Frobenius) across
                float q = 0.0f;
                for (uint32_t i = g.first_object; i < g.first_object + g.n_objects; i++) {
                    const rtc_object& o = scene->objects[i];
                    if (o.kind != RTC_SPHERE && o.kind != RTC_CYLINDER && o.kind != RTC_CONE) continue;
                    double f2 = 0.0;
                    for (int r = 0; r < 3; r++)
                        for (int cidx = 0; cidx < 3; cidx++) f2 += (double)o.inv[4 * r + cidx] * o.inv[4 * r + cidx];
                    const float qi = (float)(1e-6 * std::sqrt(f2));
                    q = (qi != qi) ? q : std::fmax(q, qi);
                }
                trav.push_back(make_float4(g.bounds_min[0], g.bounds_min[1], g.bounds_min[2], 0.0f));
                trav.push_back(make_float4(g.bounds_max[0], g.bounds_max[1], g.bounds_max[2], loose_group[gi] ? INFINITY : 4e-3f * big));
                trav.push_back(make_float4(q, 0.0f, 0.0f, 0.0f));
                any = true;
                gi++;
            }
            if (p < n) {
                // a leaf; a triangle with a usable pre-culling box carries it along (tri_precull)
                const float4* tb = tbox.empty() ? nullptr : &tbox[3 * (size_t)p];
                const bool boxed = tb && tb[0].w > 0.0f;
                trav.push_back(boxed ? make_float4(tb[0].x, tb[0].y, tb[0].z, float_of(p)) : make_float4(0.0f, 0.0f, 0.0f, float_of(p)));
                trav.push_back(boxed ? make_float4(tb[1].x, tb[1].y, tb[1].z, TRAV_BOXED_LEAF_TAG) : make_float4(0.0f, 0.0f, 0.0f, TRAV_LEAF_TAG));
                trav.push_back(boxed ? tb[2] : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            }
        }
        if (gi != scene->n_groups)
            return fail(RTC_ERR_INVALID_ARG, "group %u: groups must be listed in pre-order with first_object inside [0, n_objects)", gi);
        return RTC_OK;
    }
    // the boxes of the top-level groups that hold long runs of leaves, with their rank (see flatten)
    void heavy_group_boxes(const std::vector<float4>& trav, const std::vector<std::pair<size_t, uint32_t>>& top_level) {
        for (const auto& tl : top_level) {
            const uint32_t skip = bits_of(trav[TRAV_STRIDE * tl.first].w);
            uint32_t longest = 0;
            for (size_t e = tl.first + 1; e < skip && e < trav.size() / TRAV_STRIDE; e++)
                if (trav[TRAV_STRIDE * e + 1].w < 0.0f) longest = std::max(longest, (uint32_t)trav[TRAV_STRIDE * e + 2].w >> 3);
            if (longest >= 16u) {
                const rtc_group& g = scene->groups[tl.second];
                for (int a = 0; a < 3; a++) heavy_boxes->push_back(g.bounds_min[a]);
                for (int a = 0; a < 3; a++) heavy_boxes->push_back(g.bounds_max[a]);
                // how dear a pixel on this group is, as a rank: a surface that both reflects and refracts doubles its rays
                // at every level of the recursion, one that does either keeps them going
                bool refl = false, refr = false;
                for (uint32_t i = g.first_object; i < g.first_object + g.n_objects && i < n; i++) {
                    refl |= scene->objects[i].material.reflective > 0.0f;
                    refr |= scene->objects[i].material.transparency > 0.0f;
                }
                heavy_boxes->push_back(refl && refr ? 3.0f : (refl || refr) ? 2.0f : 1.0f);
            }
        }
    }
    // Long runs of boxed triangles get a hierarchy of the library's own (RTC_AMD_CLUSTERS=0 / 1: never / always) -- in
    // frames large enough to be traced by one or two lanes per pixel.  Where eight lanes split every run (small frames,
    // whose time is that of their slowest wave) the nodes cut the runs into pieces of a lane's share and every piece
    // ends in a round of shuffles: here_be_dragons 1000 x 400 0.79 -> 0.98 ms, 2000 x 800 1.41 -> 1.49; 4000 x 1600 3.25 -> 2.92.
    void cluster_long_runs(std::vector<float4>* trav) {
        const bool clusters_pay = cam && choose_share_log2_runs(((uint64_t)cam->width * cam->height + 63) / 64) <= 1u;
        if (hdr->has_tbox && (hdr->max_leaf_run >= 24u || P.cluster_min_run != 0u) && (P.clusters < 0 ? clusters_pay : P.clusters != 0)) {
            cluster_leaf_runs(trav, (double)hdr->tri_guard, P);
            hdr->has_tbox = 2;  // ... and the walks look for nodes among the group entries (spec_has_nodes)
            mark_pairs(trav);
            (void)mark_leaf_runs(trav, scene);  // (max_leaf_run keeps the length of the reference's runs: what the launch policy goes by)
        }
    }
    // A small tree (<= 8 leaves under <= 8 groups) keeps the unrolled flat kernels: every group becomes a GATE -- its box,
    // tested once per ray with the reference's own aabb test -- and a leaf is intersected only if the ray opens all the
    // groups around it, which is all the recursive walk does (group.rs:115-133).  Same leaves in the same order.
    // Any other tree's entry list goes behind the records as the traversal stream.
    void gates_or_stream(std::vector<float4>* trav, bool any) {
        uint32_t n_gates = 0;
        for (uint32_t g = 0; g < scene->n_groups; g++) n_gates += scene->groups[g].n_objects != 0;
        // (render path only: the batched entry points run the any-count loop for flat worlds, which has no gates)
        if (cam && any && n <= 8 && n_gates <= RTC_MAX_GATES && P.gates) {
            uint32_t k = 0;
            for (uint32_t g = 0; g < scene->n_groups; g++) {
                const rtc_group& grp = scene->groups[g];
                if (grp.n_objects == 0) continue;
                for (int a = 0; a < 3; a++) hdr->gate_box[k][a] = grp.bounds_min[a], hdr->gate_box[k][3 + a] = grp.bounds_max[a];
                for (uint32_t i = grp.first_object; i < grp.first_object + grp.n_objects; i++) hdr->gate_mask[i] |= 1u << k;
                k++;
            }
            hdr->n_gates = n_gates;
        } else if (any) {
            hdr->n_trav = (uint32_t)(trav->size() / TRAV_STRIDE);
            if (!P.prune) no_distance_pruning(trav);
            soa->insert(soa->end(), trav->begin(), trav->end());
        }
    }

    // 4. scene_box (render_body's early-out for primary rays): the union of the top-level entries when all of them are
    // bounded -- groups by their boxes (a ray that misses a group's box is turned away whatever is inside), leaves of the
    // kinds whose hits lie within their bounds (not cones: stray roots; not triangles: ill-conditioned near their plane).
    // Padding: a group's box only needs what the approximate test's rounding needs (the reference's own test of that box
    // is exact about it): 1e-4 of the coordinates.  A leaf is padded by 10 % of its own half extent: ERROR_BUDGET.md B8 --
    // a leaf only counts as bounded when the camera is within ~100 of its own units, where the reference's quadratic reports
    // nothing beyond 1 % of the radius (E2) -- the guards below.  (Up to round 3 the padding also carried 0.6 % of the camera's
    // distance to the scene's far corner, an E2 allowance in world units that the object-space guard makes redundant, and
    // that made the boxes of C5's spheres half as large again as the spheres.)
    struct RegionEntry {
        double lo[3], hi[3];
        bool group;
    };
    void scene_box_and_region() {
        if (!(cam && n > 0)) return;
        std::vector<RegionEntry> entries;  // the bounded ones
        std::vector<std::array<double, 4>> planes;
        bool known = top_level_entries(&entries, &planes);  // every entry is bounded or a plane
        if (known && !entries.empty()) known = pad_entries(entries, known && planes.empty());
        if (region) {
            region->known = known;
            region->planes = planes;
        }
    }
    // the top-level entries one by one: groups by their boxes, planes by their row, leaves where leaf_bounded lets them
    bool top_level_entries(std::vector<RegionEntry>* entries, std::vector<std::array<double, 4>>* planes) {
        bool known = true;
        uint32_t i = 0, g = 0;
        while (i < n && known) {
            while (g < scene->n_groups && (scene->groups[g].n_objects == 0 || scene->groups[g].first_object < i)) g++;  // nested / empty
            if (g < scene->n_groups && scene->groups[g].first_object == i) {
                const rtc_group& grp = scene->groups[g];
                RegionEntry e;
                e.group = true;
                for (int a = 0; a < 3; a++) {
                    known = known && std::isfinite(grp.bounds_min[a]) && std::isfinite(grp.bounds_max[a]);
                    e.lo[a] = grp.bounds_min[a], e.hi[a] = grp.bounds_max[a];
                }
                entries->push_back(e);
                i = grp.first_object + grp.n_objects;
            } else {
                const rtc_object& o = scene->objects[i];
                if (o.kind == RTC_PLANE) {
                    planes->push_back({(double)o.inv[4], (double)o.inv[5], (double)o.inv[6], (double)o.inv[7]});
                    known = known && std::isfinite(o.inv[4]) && std::isfinite(o.inv[5]) && std::isfinite(o.inv[6]) && std::isfinite(o.inv[7]);
                } else {
                    RegionEntry e;
                    e.group = false;
                    known = known && leaf_bounded(o, &e);
                    entries->push_back(e);
                }
                i++;
            }
        }
        return known;
    }
    // ERROR_BUDGET.md B8.  The box asserts "a primary ray that misses it hits nothing", and the reference's f32
    // quadratic reports hits for lines that pass a sphere / cylinder wall at up to sqrt(1 + 16 u oo) of its radius
    // (E2; oo: squared distance of the ray's origin -- here always the camera -- in the OBJECT's space: a disc
    // scaled 1e-3 across, seen from ten world units, is ten thousand of its own units away and "grows" phantom
    // hits seven radii out: wide seeds 177, 217, 249).  So a leaf only counts as bounded when the camera is within
    // ~100 of its own units (32 u oo <= 0.02: the phantom rim is 1 % of the radius, the padding below 10 %), and
    // when the camera's object-space position itself is good to 1e-3 (E1).  A cylinder also reports a wall hit's
    // height wrongly by up to 2e-3 of the height difference to the camera (E2, relative error of t) -- its box
    // grows by four times that -- and from within two radii of its axis by more than any padding covers.
    bool leaf_bounded(const rtc_object& o, RegionEntry* e) const {
        const float* orgf = cam_origin;
        double oc[3], e1 = 0.0;
        for (int r = 0; r < 3; r++) {
            oc[r] = (double)o.inv[4 * r] * orgf[0] + (double)o.inv[4 * r + 1] * orgf[1] + (double)o.inv[4 * r + 2] * orgf[2] + (double)o.inv[4 * r + 3];
            e1 = std::fmax(e1, std::fabs((double)o.inv[4 * r] * orgf[0]) + std::fabs((double)o.inv[4 * r + 1] * orgf[1]) +
                                   std::fabs((double)o.inv[4 * r + 2] * orgf[2]) + std::fabs((double)o.inv[4 * r + 3]));
        }
        const double U = 5.9604644775390625e-8;  // 2^-24
        const double oo = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2], oo_xz = oc[0] * oc[0] + oc[2] * oc[2];
        bool well = 3.0 * U * e1 <= 1e-3;
        double grow_y = 0.0;
        if (o.kind == RTC_SPHERE) well = well && 32.0 * U * oo <= 0.02;
        else if (o.kind == RTC_CYLINDER) {
            well = well && 32.0 * U * oo_xz <= 0.02 && oo_xz >= 4.0;
            grow_y = 8e-3 * (std::fabs(oc[1]) + std::fmax(std::fabs((double)o.min_y), std::fabs((double)o.max_y)));
        }
        return well && (o.kind == RTC_SPHERE || o.kind == RTC_CUBE || o.kind == RTC_CYLINDER) && world_extent(o, e->lo, e->hi, grow_y);
    }
    // the entries padded, one by one (the region's entry boxes) and as their union: SceneHdr::scene_box when nothing else can be
    // seen (`bounded`: no planes), the region's box either way.  False: a box is not finite.
    bool pad_entries(const std::vector<RegionEntry>& entries, bool bounded) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};  // union of the padded entries
        double raw_lo[3] = {INFINITY, INFINITY, INFINITY}, raw_hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        const float* org = cam_origin;
        for (const RegionEntry& e : entries)
            for (int a = 0; a < 3; a++) raw_lo[a] = std::fmin(raw_lo[a], e.lo[a]), raw_hi[a] = std::fmax(raw_hi[a], e.hi[a]);
        double far2 = 0.0;
        for (int a = 0; a < 3; a++) {
            const double d = std::fmax(std::fabs(raw_lo[a] - org[a]), std::fabs(raw_hi[a] - org[a]));
            far2 += d * d;
        }
        const double far = std::sqrt(far2);
        std::vector<float> padded;
        for (const RegionEntry& e : entries) {
            float pb[6];
            for (int a = 0; a < 3; a++) {
                const double pad = (e.group ? 0.0 : 0.05 * (e.hi[a] - e.lo[a])) + 1e-4 * (std::fabs(e.lo[a]) + std::fabs(e.hi[a]) + far);
                lo[a] = std::fmin(lo[a], e.lo[a] - pad), hi[a] = std::fmax(hi[a], e.hi[a] + pad);
                pb[a] = (float)std::nextafter((float)(e.lo[a] - pad), -INFINITY), pb[3 + a] = (float)std::nextafter((float)(e.hi[a] + pad), INFINITY);
            }
            padded.insert(padded.end(), pb, pb + 6);
            padded.push_back(1.0f);
        }
        bool ok = std::isfinite(far);
        float box[6];
        for (int a = 0; a < 3 && ok; a++) {
            box[a] = (float)lo[a];
            box[3 + a] = (float)hi[a];
            ok = std::isfinite(box[a]) && std::isfinite(box[3 + a]);
        }
        if (ok && bounded && P.scene_box) {
            for (int a = 0; a < 6; a++) hdr->scene_box[a] = box[a];
            hdr->has_scene_box = 1u;
        }
        if (region && ok) {
            region->has_box = true;
            for (int a = 0; a < 6; a++) region->box[a] = box[a];
            region->entry_boxes = padded;
        }
        return ok;
    }

    // 5. the light; an area light also leaves every object its light-cone record (light_cone_record)
    rtc_status pack_light() {
        const rtc_light& l = *scene->light;
        hdr->light_kind = l.kind;
        for (int k = 0; k < 3; k++) {
            hdr->li[k] = l.intensity[k];
            hdr->lpos[k] = l.position[k];
            hdr->corner[k] = l.corner[k];
            hdr->uvec[k] = l.u_vec[k];
            hdr->vvec[k] = l.v_vec[k];
        }
        RTC_TRY(check_tuple(l.position, 1.0f, "light.position"));
        hdr->u_steps = hdr->v_steps = 1;
        hdr->cells_f = 1.0f;
        hdr->jitter_mode = RTC_JITTER_CONSTANT;
        if (l.kind == RTC_LIGHT_RECT) {
            RTC_TRY(check_tuple(l.corner, 1.0f, "light.corner"));
            RTC_TRY(check_tuple(l.u_vec, 0.0f, "light.u_vec"));
            RTC_TRY(check_tuple(l.v_vec, 0.0f, "light.v_vec"));
            if (l.u_steps <= 0 || l.v_steps <= 0) return fail(RTC_ERR_INVALID_ARG, "light steps must be positive");
            // (include/rtc.h RTC_LIGHT_CELLS_MAX: above 2^24 cells the reference's own f32 sum of ones saturates; in 64 bits, an int product wraps from 46 341^2)
            const int64_t cells = (int64_t)l.u_steps * (int64_t)l.v_steps;
            if (cells > (int64_t)RTC_LIGHT_CELLS_MAX)
                return fail(RTC_ERR_UNSUPPORTED, "light of %d x %d steps: more than RTC_LIGHT_CELLS_MAX = %d cells (2^24)", l.u_steps, l.v_steps, RTC_LIGHT_CELLS_MAX);
            if (l.jitter_mode != RTC_JITTER_CONSTANT && l.jitter_mode != RTC_JITTER_HASHED && l.jitter_mode != RTC_JITTER_SEQUENCE)
                return fail(RTC_ERR_UNSUPPORTED, "jitter mode %d cannot run on the device (closures are host-only)", l.jitter_mode);
            if (l.jitter_mode == RTC_JITTER_SEQUENCE) {
                // test/utils.rs:19-24: the cycle is state carried across every question a light is asked -- across pixels, in the
                // reference's serial loop.  Only one call on a fresh light is defined without that order: the batched
                // rtc_intensity_at / rtc_point_on_light (cam == nullptr and allow_sequence).
                if (cam || !allow_sequence)
                    return fail(RTC_ERR_UNSUPPORTED, "sequence jitter (hardcoded_jitter) is serial across pixels and rays: only rtc_intensity_at and "
                                                     "rtc_point_on_light accept it");
                if (l.jitter_seq_len < 1 || l.jitter_seq_len > RTC_JITTER_SEQUENCE_MAX)
                    return fail(RTC_ERR_INVALID_ARG, "sequence jitter: %u values (1 .. %d)", l.jitter_seq_len, RTC_JITTER_SEQUENCE_MAX);
            }
            hdr->u_steps = l.u_steps;
            hdr->v_steps = l.v_steps;
            hdr->cells_f = (float)(l.u_steps * l.v_steps);
            hdr->jitter_mode = l.jitter_mode;
            hdr->jitter_const = l.jitter_const;
            hdr->jitter_seed = l.jitter_seed;
            if (l.jitter_mode == RTC_JITTER_SEQUENCE) {
                hdr->jitter_seq_len = l.jitter_seq_len;
                bool unit = true;  // light-cone culling needs every sample inside the parallelogram: all values in [0, 1]
                for (uint32_t k = 0; k < RTC_JITTER_SEQUENCE_MAX; k++) {
                    hdr->jitter_seq[k] = l.jitter_seq[k % l.jitter_seq_len];
                    unit = unit && l.jitter_seq[k % l.jitter_seq_len] >= 0.0f && l.jitter_seq[k % l.jitter_seq_len] <= 1.0f;
                }
                hdr->jitter_const = unit ? 0.5f : 2.0f;  // (what light_cull_mask looks at for a source that is not the hash)
            }
            // light-cone culling inputs: the parallelogram's corners in every object's space, and its y range
            const float su = (float)l.u_steps, sv = (float)l.v_steps;
            float cw[4][3];
            float y_lo = INFINITY, y_hi = -INFINITY, y_abs = 0.0f;
            for (int k = 0; k < 4; k++) {
                const float fu = (k == 1 || k == 2) ? su : 0.0f, fv = (k >= 2) ? sv : 0.0f;
                for (int a = 0; a < 3; a++) cw[k][a] = l.corner[a] + l.u_vec[a] * fu + l.v_vec[a] * fv;
                y_lo = fminf(y_lo, cw[k][1]);
                y_hi = fmaxf(y_hi, cw[k][1]);
                y_abs += fabsf(cw[k][1]);
            }
            {   // classify_cells (ERROR_BUDGET.md B10): half a cell's diagonal -- the longer one -- padded
                double d1 = 0.0, d2 = 0.0, lmax = 0.0;
                for (int a = 0; a < 3; a++) {
                    d1 += ((double)l.u_vec[a] + l.v_vec[a]) * ((double)l.u_vec[a] + l.v_vec[a]);
                    d2 += ((double)l.u_vec[a] - l.v_vec[a]) * ((double)l.u_vec[a] - l.v_vec[a]);
                    for (int k = 0; k < 4; k++) lmax = std::fmax(lmax, std::fabs((double)cw[k][a]));
                }
                const double hd = 0.5 * std::sqrt(std::fmax(d1, d2)) * 1.01 + 8.0 * 5.9604644775390625e-8 * lmax;
                const bool unit_jitter = l.jitter_mode == RTC_JITTER_HASHED || (hdr->jitter_const >= 0.0f && hdr->jitter_const <= 1.0f);
                hdr->cell_hd = (unit_jitter && std::isfinite(hd) && hd > 0.0) ? (float)hd : 0.0f;
            }
            const float ym = 1e-5f * y_abs + 1e-30f;  // far above the sample points' rounding error
            hdr->light_y_lo = y_lo - ym;
            hdr->light_y_hi = y_hi + ym;
            for (uint32_t i = 0; i < n; i++) light_cone_record(i, cw);
        } else if (l.kind != RTC_LIGHT_POINT) {
            return fail(RTC_ERR_UNSUPPORTED, "light kind %d", l.kind);
        }
        hdr->all_cast = 1;
        for (uint32_t i = 0; i < n; i++)
            if (!scene->objects[i].casts_shadow) hdr->all_cast = 0;
        hdr->cull_flags = (P.light_cull ? CULL_ENABLED : 0u) | (P.dark ? CULL_DARK : 0u) | (P.fast_shadow ? CULL_FAST_SHADOW : 0u) | (P.cell_cull ? CULL_CELLS : 0u) | (P.own_blocks ? CULL_OWN_BLOCKS : 0u);
        return RTC_OK;
    }
    // One object's light-cone record (light_cull_mask): the area light's corners `cw` in the object's space, and in trn.w / off2.w
    // the bounds E / errB on their error -- or, for a sphere, off2.w = the cone pre-test's half diagonal
    void light_cone_record(uint32_t i, const float cw[4][3]) {
        const float* m = scene->objects[i].inv;
        float c[4][3];
        for (int k = 0; k < 4; k++)
            for (int r = 0; r < 3; r++)
                c[k][r] = m[4 * r] * cw[k][0] + m[4 * r + 1] * cw[k][1] + m[4 * r + 2] * cw[k][2] + m[4 * r + 3];
        float4* lc = rec(COL_LCORN, i, 3);
        lc[0] = make_float4(c[0][0], c[0][1], c[0][2], c[1][0]);
        lc[1] = make_float4(c[1][1], c[1][2], c[2][0], c[2][1]);
        lc[2] = make_float4(c[2][2], c[3][0], c[3][1], c[3][2]);
        // ERROR_BUDGET.md E1 for light_cull_mask: E bounds, in the object's own units, how far the pyramid the cull reasons
        // about (apex: the computed object-space shade point o; base: these computed corners) can sit from the rays the
        // exact test traces (same apex, direction M (sample - p)): |delta corner| + |delta o| <= 3 u (|M| (|L| + |p|) + 2 |t|),
        // written with 4 u.  |M| |p| is bounded through o itself, which the cull only trusts within 100 radii:
        // componentwise |g_k p_k| <= |o_k| + |t_k| for a scale+translate object, |M| |p| <= |M|_inf |F|_inf (|o|_inf + |t|_inf)
        // otherwise (F: the forward transform).  A plane's rule looks at o.y alone and has no distance limit: the constant
        // holds what does not depend on p, and for a plane that is not scale+translate only the kernel adds errB * |p|_inf.
        const rtc_object& ob = scene->objects[i];
        const double U4 = 4.0 * 5.9604644775390625e-8;
        double Lmax = 0.0, tinf = 0.0, minf = 0.0;
        for (int k = 0; k < 4; k++)
            for (int a = 0; a < 3; a++) Lmax = std::fmax(Lmax, std::fabs((double)cw[k][a]));
        double rows[3];
        for (int r = 0; r < 3; r++) {
            rows[r] = std::fabs((double)m[4 * r]) + std::fabs((double)m[4 * r + 1]) + std::fabs((double)m[4 * r + 2]);
            minf = std::fmax(minf, rows[r]);
            tinf = std::fmax(tinf, std::fabs((double)m[4 * r + 3]));
        }
        const bool diag = m[1] == 0.0f && m[2] == 0.0f && m[4] == 0.0f && m[6] == 0.0f && m[8] == 0.0f && m[9] == 0.0f;
        double E, errB = 0.0;
        if (ob.kind == RTC_PLANE) {
            E = U4 * (2.0 * std::fabs((double)m[7]) + rows[1] * Lmax);
            if (!diag) errB = U4 * rows[1];
        } else {
            double hy = 1.0;
            if (ob.kind == RTC_CYLINDER) hy = std::fmax(std::fabs((double)ob.min_y), std::fabs((double)ob.max_y));
            const double rad = 103.0 * std::sqrt(ob.kind == RTC_CUBE ? 3.0 : 1.0 + (ob.kind == RTC_CYLINDER ? hy * hy : 0.0));  // |o| where the cull still decides
            if (diag) {
                E = U4 * (rad + 2.0 * tinf + minf * Lmax);
            } else {
                double F[9], f[3], finf = INFINITY;
                if (forward_affine(m, F, f)) {
                    finf = 0.0;
                    for (int r = 0; r < 3; r++) finf = std::fmax(finf, std::fabs(F[3 * r]) + std::fabs(F[3 * r + 1]) + std::fabs(F[3 * r + 2]));
                }
                E = U4 * (minf * finf * (rad + tinf) + tinf + minf * Lmax);
            }
        }
        rec(COL_TRN, i)->w = std::isfinite(E) ? (float)E : INFINITY;
        rec(COL_OFF2, i)->w = (float)errB;
        if (ob.kind == RTC_SPHERE) {
            // light_cull_mask's cone pre-test: half the parallelogram's longer diagonal in this sphere's space, 0.1 % up
            double d02 = 0.0, d13 = 0.0;
            for (int r = 0; r < 3; r++) d02 += ((double)c[0][r] - c[2][r]) * ((double)c[0][r] - c[2][r]), d13 += ((double)c[1][r] - c[3][r]) * ((double)c[1][r] - c[3][r]);
            const double hdl = 0.5 * std::sqrt(std::fmax(d02, d13)) * 1.001;
            rec(COL_OFF2, i)->w = std::isfinite(hdl) && hdl > 0.0 ? (float)hdl : 0.0f;
        }
    }

    // 6. the camera
    rtc_status pack_camera() {
        if (!cam) return RTC_OK;
        if (cam->width == 0 || cam->height == 0) return fail(RTC_ERR_INVALID_ARG, "empty canvas");
        if (!is_affine(cam->inv)) return fail(RTC_ERR_UNSUPPORTED, "camera inverse transform is not affine");
        hdr->width = cam->width;
        hdr->height = cam->height;
        hdr->half_w = cam->half_width;
        hdr->half_h = cam->half_height;
        hdr->pixel_size = cam->pixel_size;
        std::memcpy(hdr->cam, cam->inv, sizeof(float) * 12);
        for (int k = 0; k < 3; k++) hdr->cam_origin[k] = cam_origin[k];  // pixel-invariant, computed once
        return RTC_OK;
    }
};

// Validates and flattens rtc_scene + rtc_camera into the kernel's header and
// records (host staging buffer: the columns of SoaColumn, the traversal stream, the UV pattern records).
// `heavy_boxes` (optional): world-space boxes, 7 floats each (min, max, rank), of the top-level GroupShapes that hold long runs of leaves
// (divided meshes) -- where a frame's slow waves are (rtc_ctx_render: block list).  `region` (optional): see SceneRegion.
// An error leaves *hdr half filled: callers discard it.
inline rtc_status flatten(const Policy& P, const rtc_scene* scene, const rtc_camera* cam, SceneHdr* hdr, std::vector<float4>* soa,
                          std::vector<float>* texels, std::vector<float>* heavy_boxes = nullptr, SceneRegion* region = nullptr,
                          bool allow_sequence = false, FlatHull* flat_hull = nullptr, float lens_radius = 0.0f) {
    if (!scene) return fail(RTC_ERR_INVALID_ARG, "scene is NULL");
    if (!scene->light) return fail(RTC_ERR_NO_LIGHT, "World light should be set");  // world.rs:66
    if (scene->n_objects && !scene->objects) return fail(RTC_ERR_INVALID_ARG, "scene.objects is NULL");
    std::memset(hdr, 0, sizeof(*hdr));
    hdr->n_objects = scene->n_objects;
    Flatten f = {P, scene, cam, hdr, soa, texels, heavy_boxes, region, allow_sequence, flat_hull, lens_radius};
    f.n = scene->n_objects;
    f.np = padded_count(f.n);
    soa->assign(soa_index(SOA_COLUMNS, f.np, 0), make_float4(0, 0, 0, 0));
    const float zero[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    if (cam) mat_vec4(cam->inv, zero, f.cam_origin);
    RTC_TRY(f.pack_objects());
    f.triangle_boxes();
    if (scene->n_groups) RTC_TRY(f.group_stream());
    else f.flat_bvh_stream();
    f.scene_box_and_region();
    RTC_TRY(f.pack_light());
    hdr->uvrec_off = (uint32_t)soa->size();
    soa->insert(soa->end(), f.uvrec.begin(), f.uvrec.end());
    return f.pack_camera();
}

// The ahead-of-time kernels: render_kernel<NOBJ, SIMPLE> / hits_kernel<NOBJ, SIMPLE, LIGHT>.  <= 4 / <= 8 objects get fully unrolled
// object loops (SIMPLE: all of them scale+translate-only, no cylinder), anything larger takes the generic loop (0), a
// traversal stream the packet walk (-1).
struct KernelFamily {
    int nobj;  // -1, 4, 8, 0
    bool simple;
    // (no code object's address; ss_k: the supersampling instantiations of the family, rtc_supersample.h, are kernels of their own)
    // seam: the family's ss_seam_render_kernel instantiations, the one-call seam's variant of the supersampling kernels
    // lens: the family's lens_render_kernel instantiations (rtc_lens.h)
    const void* key(uint32_t ss_k = 1u, bool seam = false, bool lens = false) const {
        return (const void*)(uintptr_t)(0x1000 + (lens ? 0x2000 : 0) + (seam ? 0x800 : 0) + 0x100 * ss_k + 2 * (nobj + 1) + (simple ? 1 : 0));
    }
    std::string name(const char* tree_how = "tree") const {
        if (nobj < 0) return std::string("render_kernel<") + tree_how + ">";
        return "render_kernel<" + std::to_string(nobj) + (simple ? ",simple>" : ",general>");
    }
};
inline KernelFamily aot_family(uint32_t n_trav, uint32_t n_objects, bool simple) {
    if (n_trav) return {-1, false};
    if (n_objects <= 4) return {4, simple};
    if (n_objects <= 8) return {8, simple};
    return {0, false};
}

// Which 16 x 16 pixel tiles do the boxes of the mesh-holding groups project to?  ray_for_pixel (camera.rs:60-74) sends
// pixel (px, py) through the camera-space point (half_width - (px + 0.5) s, half_height - (py + 0.5) s, -1); a world
// point maps to camera space through the inverse of Camera.transform_inverse.  Performance only -- which blocks start
// first and with how many lanes per pixel -- so generous padding and "everything" when a box reaches behind the camera.
constexpr size_t HEAVY_BOX_FLOATS = 7;  // min, max, rank (1 .. 3: project_heavy_boxes keeps a tile's highest)
inline void project_heavy_boxes(const Policy& P, const std::vector<float>& boxes, const rtc_camera* cam, std::vector<uint8_t>* tiles, uint32_t* tw, uint32_t* th) {
    tiles->clear();
    *tw = *th = 0;
    if (boxes.empty() || !cam || !P.block_list) return;
    float view[16];
    inverse4(cam->inv, view);
    const uint32_t w = (cam->width + 15u) / 16u, h = (cam->height + 15u) / 16u;
    tiles->assign((size_t)w * h, 0);
    *tw = w;
    *th = h;
    for (size_t b = 0; b + HEAVY_BOX_FLOATS - 1 < boxes.size(); b += HEAVY_BOX_FLOATS) {
        double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
        bool everything = false;
        for (int k = 0; k < 8 && !everything; k++) {
            const float p[4] = {boxes[b + ((k & 1) ? 3 : 0)], boxes[b + ((k & 2) ? 4 : 1)], boxes[b + ((k & 4) ? 5 : 2)], 1.0f};
            float q[4];
            mat_vec4(view, p, q);
            if (!(q[2] < -1e-4f) || !std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) {
                everything = true;
                break;
            }
            const double px = ((double)cam->half_width - (double)q[0] / -(double)q[2]) / cam->pixel_size - 0.5;
            const double py = ((double)cam->half_height - (double)q[1] / -(double)q[2]) / cam->pixel_size - 0.5;
            x0 = std::fmin(x0, px), x1 = std::fmax(x1, px), y0 = std::fmin(y0, py), y1 = std::fmax(y1, py);
        }
        if (everything) x0 = y0 = -1e9, x1 = y1 = 1e9;
        const long tx0 = std::max(0L, (long)std::floor((x0 - 8.0) / 16.0)), tx1 = std::min((long)w - 1, (long)std::floor((x1 + 8.0) / 16.0));
        const long ty0 = std::max(0L, (long)std::floor((y0 - 8.0) / 16.0)), ty1 = std::min((long)h - 1, (long)std::floor((y1 + 8.0) / 16.0));
        for (long ty = ty0; ty <= ty1; ty++)
            for (long tx = tx0; tx <= tx1; tx++) (*tiles)[(size_t)ty * w + tx] = std::max((*tiles)[(size_t)ty * w + tx], (uint8_t)boxes[b + 6]);
    }
}

// A top-level plane (plane.rs:45-56) is hit by a primary ray only if the ray points towards it: with y_o the plane's
// object-space height of the camera and y_d that of the direction, t = -y_o / y_d >= 0 needs y_d of the other sign.  The
// direction through pixel (px, py) is linear in (px, py) (ray_for_pixel, camera.rs:60-74), hence so is y_d: the pixels that can
// see the plane are one side of a straight line -- the horizon -- taken here with 8 pixels to spare, and marked as the 16 x 16
// tiles of their bounding rectangle (the launch is a rectangle anyway).  A camera in the plane, or not finite: everything.
inline void mark_plane_side(const std::array<double, 4>& row, const rtc_camera* cam, std::vector<uint8_t>* tiles, uint32_t tw, uint32_t th) {
    const float* m = cam->inv;
    const double org[3] = {m[3], m[7], m[11]};
    const double y_o = row[0] * org[0] + row[1] * org[1] + row[2] * org[2] + row[3];
    // y_d(px, py) = row . M3 (half_w - (px + 0.5) s, half_h - (py + 0.5) s, -1) = a px + b py + c0
    double col[3];  // row . (columns of the camera matrix's linear part)
    for (int k = 0; k < 3; k++) col[k] = row[0] * m[k] + row[1] * m[4 + k] + row[2] * m[8 + k];
    const double sz = cam->pixel_size, a = -col[0] * sz, b = -col[1] * sz;
    const double c0 = col[0] * (cam->half_width - 0.5 * sz) + col[1] * (cam->half_height - 0.5 * sz) - col[2];
    auto all = [&]() { std::fill(tiles->begin(), tiles->end(), (uint8_t)1); };
    if (!std::isfinite(y_o) || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c0) || y_o == 0.0) return all();
    // visible where sign(y_o) * y_d < 0; keep everything with g(px, py) = sign(y_o) * y_d - margin < 0
    const double sgn = y_o > 0.0 ? 1.0 : -1.0, margin = 8.0 * (std::fabs(a) + std::fabs(b));
    auto g = [&](double px, double py) { return sgn * (a * px + b * py + c0) - margin; };
    const double W = cam->width, Hh = cam->height;
    const double cx[4] = {0.0, W, W, 0.0}, cy[4] = {0.0, 0.0, Hh, Hh};
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int k = 0; k < 4; k++) {
        const int n = (k + 1) & 3;
        const double gk = g(cx[k], cy[k]), gn = g(cx[n], cy[n]);
        if (gk < 0.0) x0 = std::fmin(x0, cx[k]), x1 = std::fmax(x1, cx[k]), y0 = std::fmin(y0, cy[k]), y1 = std::fmax(y1, cy[k]);
        if ((gk < 0.0) != (gn < 0.0)) {  // the line crosses this edge of the image
            const double t = gk / (gk - gn), ex = cx[k] + t * (cx[n] - cx[k]), ey = cy[k] + t * (cy[n] - cy[k]);
            x0 = std::fmin(x0, ex), x1 = std::fmax(x1, ex), y0 = std::fmin(y0, ey), y1 = std::fmax(y1, ey);
        }
    }
    if (!(x0 <= x1) || !(y0 <= y1)) return;  // the plane is behind every pixel's ray
    const long tx0 = std::max(0L, (long)std::floor(x0 / 16.0) - 1), tx1 = std::min((long)tw - 1, (long)std::floor(x1 / 16.0) + 1);
    const long ty0 = std::max(0L, (long)std::floor(y0 / 16.0) - 1), ty1 = std::min((long)th - 1, (long)std::floor(y1 / 16.0) + 1);
    for (long ty = ty0; ty <= ty1; ty++)
        for (long tx = tx0; tx <= tx1; tx++) (*tiles)[(size_t)ty * tw + tx] = 1;
}

// ... and tile by tile, for the scene-tile mask: g is linear in (px, py), so over a tile's square it takes its least value at a
// corner -- a tile none of whose four corners has g < 0 holds no pixel that can see the plane (the same g, the same 8 pixels of
// margin, the same "everything" for a camera in the plane or values that are not finite).  A tile's square is taken from its
// first pixel to its neighbour's, [16 tx, 16 tx + 16]: every pixel centre of the tile lies inside.
inline void mark_plane_tiles(const std::array<double, 4>& row, const rtc_camera* cam, std::vector<uint8_t>* tiles, uint32_t tw, uint32_t th) {
    const float* m = cam->inv;
    const double y_o = row[0] * m[3] + row[1] * m[7] + row[2] * m[11] + row[3];
    double col[3];
    for (int k = 0; k < 3; k++) col[k] = row[0] * m[k] + row[1] * m[4 + k] + row[2] * m[8 + k];
    const double sz = cam->pixel_size, a = -col[0] * sz, b = -col[1] * sz;
    const double c0 = col[0] * (cam->half_width - 0.5 * sz) + col[1] * (cam->half_height - 0.5 * sz) - col[2];
    if (!std::isfinite(y_o) || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c0) || y_o == 0.0) {
        std::fill(tiles->begin(), tiles->end(), (uint8_t)1);
        return;
    }
    const double sgn = y_o > 0.0 ? 1.0 : -1.0, margin = 8.0 * (std::fabs(a) + std::fabs(b));
    auto g = [&](double px, double py) { return sgn * (a * px + b * py + c0) - margin; };
    for (uint32_t ty = 0; ty < th; ty++)
        for (uint32_t tx = 0; tx < tw; tx++) {
            const double x0 = 16.0 * tx, y0 = 16.0 * ty;
            if (g(x0, y0) < 0.0 || g(x0 + 16.0, y0) < 0.0 || g(x0, y0 + 16.0) < 0.0 || g(x0 + 16.0, y0 + 16.0) < 0.0) (*tiles)[(size_t)ty * tw + tx] = 1;
        }
}

// What rtc_ctx_set_scene keeps of a scene beside its records: which tiles of the frame matter, and which kernel renders it.
struct ScenePlan {
    bool simple = false;  // every object scale+translate-only, no cylinder / cone / triangle, no patterns
    std::vector<uint8_t> heavy_tiles;  // the 16 x 16 tiles a mesh projects to, by rank (project_heavy_boxes); empty: no block list
    uint32_t heavy_w = 0u, heavy_h = 0u;
    float scene_box_coverage = 1.0f;            // share of the image the scene's box projects to (1: unknown / all of it)
    uint32_t scene_rect[4] = {0u, 0u, 0u, 0u};  // the tiles outside which no primary ray sees anything: [x0, x1) x [y0, y1); empty: unknown
    float scene_rect_coverage = 1.0f;           // ... and its share of the frame
    std::vector<uint8_t> scene_rect_tiles;      // the tiles scene_rect bounds: the region's box projected, the planes' visible sides
    std::vector<uint8_t> scene_tile_mask;       // the tiles some top-level entry projects to; empty: not known / not worth it
    uint32_t scene_tiles_w = 0u, scene_tiles_h = 0u;
    // ... of a bounded world, under a third of the frame and under two thirds of the rectangle: a frame whose rows leave chunk by
    // chunk (rtc_render_ex) is drawn from the list only then -- a list cannot report rows, and only there it gains more than that costs
    bool scene_tiles_sparse = false;
    bool spec_shares = false, spec_blocks_y = false, spec_rect = false;  // the scene's kernel takes -DRTC_SPEC_SHARE / _BLOCKS_Y / _RECT = 1
    int tree_waves = 0;    // waves per SIMD of the scene's tree kernel (0: the scene has no traversal stream)
    bool wf_pays = false;  // a tree world with long leaf runs whose materials both reflect and transmit
    std::string family_name;  // the ahead-of-time kernel that renders the scene when the scene's own does not
    // The options of the scene's kernel, written down whatever the policy says (deep_kernel may need them later; empty: a world
    // without objects), its name, and `compile_now`: does the policy want the scene-compiled kernel for ordinary depths.
    std::vector<std::string> spec_defs;
    std::string spec_name;
    uint32_t ss_k = 1u;  // the frame's kernel is the supersampling one of this factor (plan_supersampled)
    bool lens = false;   // ... or the lens kernel of this factor (plan_lens)
    bool lens_seam = false;  // ... in the one-call seam's variant (rtc_lens_seam.h)
    bool compile_now = false;
    // ... and the policy's two exceptions to "from 2^18 pixels", which rtc_ctx_trace applies to its number of rays: worlds with divided
    // meshes are compiled whatever the size, a mixed list of many objects (and a world without objects) never
    bool compile_any_size = false, compile_never = false;
};

// how many tiles of a mask are set
inline size_t count_tiles(const std::vector<uint8_t>& tiles) {
    size_t n = 0;
    for (uint8_t b : tiles) n += b ? 1u : 0u;
    return n;
}
// Scene box coverage, scene rectangle and scene tiles of a frame (all three: performance only, and only with a camera).
inline void plan_coverage(const Policy& P, const SceneHdr& hdr, const rtc_camera* camera, const SceneRegion& region, ScenePlan* p) {
    if (hdr.has_scene_box && camera && P.block_list) {
        std::vector<uint8_t> covered;
        uint32_t tw = 0, th = 0;
        std::vector<float> box(hdr.scene_box, hdr.scene_box + 6);
        box.push_back(1.0f);
        project_heavy_boxes(P, box, camera, &covered, &tw, &th);
        size_t n_cov = 0;
        for (uint8_t b : covered) n_cov += b;
        if (!covered.empty()) p->scene_box_coverage = (float)n_cov / (float)covered.size();
    }
    // The scene rectangle (rtc_ctx_render): the 16 x 16 tiles in which a primary ray can see anything at all -- the padded
    // box of the bounded top-level entries, projected, and for every top-level plane the side of its horizon on which rays
    // point towards it.
    if (!(region.known && camera && P.block_list)) return;
    std::vector<uint8_t> covered;
    uint32_t tw = (camera->width + 15u) / 16u, th = (camera->height + 15u) / 16u;
    if (region.has_box) {
        std::vector<float> box(region.box, region.box + 6);
        box.push_back(1.0f);
        project_heavy_boxes(P, box, camera, &covered, &tw, &th);
    }
    if (covered.empty()) covered.assign((size_t)tw * th, 0);
    for (const auto& pl : region.planes) mark_plane_side(pl, camera, &covered, tw, th);
    uint32_t x0 = tw, x1 = 0, y0 = th, y1 = 0;
    for (uint32_t ty = 0; ty < th; ty++)
        for (uint32_t tx = 0; tx < tw; tx++)
            if (covered[(size_t)ty * tw + tx]) x0 = std::min(x0, tx), x1 = std::max(x1, tx + 1u), y0 = std::min(y0, ty), y1 = std::max(y1, ty + 1u);
    if (x0 < x1 && y0 < y1) {
        p->scene_rect[0] = x0, p->scene_rect[1] = x1, p->scene_rect[2] = y0, p->scene_rect[3] = y1;
        p->scene_rect_coverage = (float)((double)(x1 - x0) * (y1 - y0) / ((double)tw * th));
    }
    if (P.jit_print)
        std::fprintf(stderr, "librtc_amd: scene rectangle tiles [%u, %u) x [%u, %u) of %u x %u: %.3f of the frame\n", x0, x1, y0, y1, tw, th,
                     p->scene_rect_coverage);
    // ... and tile by tile: the tiles some entry's padded box projects to (ERROR_BUDGET.md B8 holds for each padded box as it does
    // for their union) and those that can see a top-level plane (mark_plane_tiles).  Frames are drawn from the list of those tiles, and
    // the rest is zero-filled, where that was measured to pay: a bounded world whose entries cover under a third of the frame and
    // under two thirds of their rectangle (C5), a world with planes a fifth of whose tiles or more are in neither (C3's sky).
    if (P.scene_tiles != 0 && (!region.entry_boxes.empty() || !region.planes.empty()) && x0 < x1 && y0 < y1) {
        std::vector<uint8_t> each;
        uint32_t ew = tw, eh = th;
        if (!region.entry_boxes.empty()) project_heavy_boxes(P, region.entry_boxes, camera, &each, &ew, &eh);
        else each.assign((size_t)tw * th, 0);
        if (ew == tw && eh == th && each.size() == (size_t)tw * th) {
            for (uint8_t& b : each) b = b ? 1 : 0;
            for (const auto& pl : region.planes) mark_plane_tiles(pl, camera, &each, tw, th);
            const size_t n_each = count_tiles(each), n_all = (size_t)tw * th, unseen = n_all - n_each;
            const bool sparse = region.planes.empty() && 3u * n_each < n_all && 3u * n_each < 2u * (size_t)(x1 - x0) * (y1 - y0);
            const bool wanted = P.scene_tiles == 2 || (region.planes.empty() ? sparse : 100u * unseen >= (size_t)SCENE_TILES_UNSEEN_PCT * n_all);
            if (n_each > 0 && unseen > 0 && wanted) {
                p->scene_tile_mask = each;
                p->scene_tiles_w = tw, p->scene_tiles_h = th;
                p->scene_tiles_sparse = sparse;
            }
            if (P.jit_print) std::fprintf(stderr, "librtc_amd: scene tiles: %zu of %u x %u%s\n", n_each, tw, th, p->scene_tile_mask.empty() ? " (not used)" : "");
        }
    }
    p->scene_rect_tiles.swap(covered);
}

// Material facts (rtc_kernel_core.h): does any material reflect / transmit at all (a scene without either carries no
// recursion code), does any need powf for a highlight, and how many levels of the recursion stack the kernel keeps in
// registers (FrameStack).  Register levels were built to take the 2.5 GB of frame traffic out of the glass-and-mirror
// scene and do (scratch 448 -> 184 B per lane), but the frame gets only 2.5 % faster at 4 waves per SIMD and every
// other scene slower (tools/ab_env.py): the traffic was not what the waves wait for.  Default 0;
// RTC_AMD_REG_LEVELS=1..8 keeps the experiment reproducible.
struct MaterialFacts {
    bool any_refl = false, any_refr = false, any_specular = false;
    int reg_levels = 0;
    const char* reg_waves = nullptr;  // register levels need the registers: 13 dwords per level on top of the ~70 the kernel works in
};
inline MaterialFacts material_facts(const Policy& P, const rtc_scene* scene, uint32_t n) {
    MaterialFacts f;
    for (uint32_t i = 0; i < n; i++) {
        const rtc_material& m = scene->objects[i].material;
        f.any_refl = f.any_refl || !(m.reflective == 0.0f);
        f.any_refr = f.any_refr || !(m.transparency == 0.0f);
        f.any_specular = f.any_specular || !(m.specular == 0.0f && m.shininess >= 0.0f && m.shininess <= 1e6f);  // phong: needs powf
    }
    f.reg_levels = (!f.any_refl && !f.any_refr) ? 0 : P.reg_levels;
    f.reg_waves = f.reg_levels == 0 ? nullptr : f.reg_levels <= 3 ? "-DRTC_WAVES_PER_SIMD=4" : "-DRTC_WAVES_PER_SIMD=3";
    return f;
}
// The options every scene's kernel takes, whichever of the three kinds it is; each kind puts the groups where it always has
// (jit_get hashes the list in order into the cache key and the kernel id).
struct CommonDefs {
    std::vector<std::string> light;      // light kind, jitter mode, pattern use
    std::vector<std::string> launch;     // lanes per pixel, blocks per workgroup, scene rectangle
    std::vector<std::string> recursion;  // light zeros and the material facts
};
inline CommonDefs common_defs(const SceneHdr& hdr, const ScenePlan& p, const MaterialFacts& f) {
    auto flag = [](const char* name, bool on) { return std::string(name) + (on ? "1" : "0"); };
    // which components of the area light's cell vectors are exact zeros (kernel: LIGHT_ZEROS / point_on_light); only when
    // the factors they would be multiplied with are finite -- hashed jitter is in (0, 1], a constant is the caller's
    uint32_t light_zeros = 0u;
    if (hdr.light_kind == RTC_LIGHT_RECT && (hdr.jitter_mode == RTC_JITTER_HASHED || std::isfinite(hdr.jitter_const)))
        for (int k = 0; k < 3; k++) light_zeros |= (hdr.uvec[k] == 0.0f ? 1u << k : 0u) | (hdr.vvec[k] == 0.0f ? 8u << k : 0u);
    CommonDefs d;
    d.light = {"-DRTC_SPEC_LIGHT_KIND=" + std::to_string(hdr.light_kind), "-DRTC_SPEC_JITTER=" + std::to_string(hdr.jitter_mode),
               flag("-DRTC_SPEC_PATTERNS=", hdr.has_patterns)};
    d.launch = {flag("-DRTC_SPEC_SHARE=", p.spec_shares), flag("-DRTC_SPEC_BLOCKS_Y=", p.spec_blocks_y), flag("-DRTC_SPEC_RECT=", p.spec_rect)};
    d.recursion = {"-DRTC_SPEC_LIGHT_ZEROS=" + std::to_string(light_zeros), flag("-DRTC_SPEC_ANY_REFL=", f.any_refl), flag("-DRTC_SPEC_ANY_REFR=", f.any_refr),
                   "-DRTC_SPEC_REG_LEVELS=" + std::to_string(f.reg_levels), flag("-DRTC_SPEC_ANY_SPECULAR=", f.any_specular)};
    return d;
}
inline void append(std::vector<std::string>* defs, const std::vector<std::string>& more) { defs->insert(defs->end(), more.begin(), more.end()); }
inline std::string hex_word(uint32_t bits) {
    char b[16];
    snprintf(b, sizeof(b), "0x%x", bits);
    return b;
}
// do all objects share one kind / flags word?  (SHAPE_UNIFORM aside: only the unrolled kernels' fast shadow decision
// reads it, and a cloud of spheres must not lose its like-objects kernel because some are squashed)
inline bool like_objects(const std::vector<float4>& soa, const SceneHdr& hdr, uint32_t* first) {
    const uint32_t n = hdr.n_objects;
    *first = object_bits(soa, hdr, 0) & ~(uint32_t)SHAPE_UNIFORM;
    for (uint32_t i = 1; i < n; i++)
        if ((object_bits(soa, hdr, i) & ~(uint32_t)SHAPE_UNIFORM) != *first) return false;
    return n > 0;
}
// Does the policy want the scene's own kernel for `count` pixels (rtc_ctx_set_scene) or rays (rtc_ctx_trace)?  RTC_AMD_SPECIALIZE: 1
// always, 2 from 2^18 -- or whatever the count, `any_size` -- and `never` for the scenes that are left to the ahead-of-time loop.
inline bool wants_scene_kernel(const Policy& P, uint64_t count, bool any_size, bool never) {
    return !never && (P.specialise == 1 || (P.specialise == 2 && (count >= (1ull << 18) || any_size)));
}
inline bool frame_wants_scene_kernel(const Policy& P, const SceneHdr& hdr, const ScenePlan& p) {
    return wants_scene_kernel(P, (uint64_t)hdr.width * hdr.height, p.compile_any_size, p.compile_never);
}

// a traversal stream (GroupShapes, or the library's own hierarchy): packet walk, compiled per scene like the flat kernels
inline void plan_tree_kernel(const Policy& P, const SceneHdr& hdr, const std::vector<float4>& soa, const std::string& how, const MaterialFacts& f,
                             const CommonDefs& d, ScenePlan* p) {
    // (worlds with divided meshes are compiled whatever the frame's size: the ahead-of-time walk has neither the
    // triangle pre-culling specialisation nor the leaf-sharing lanes -- mesh 512 x 384: 7.9 ms)
    p->compile_any_size = hdr.max_leaf_run >= 16u;
    p->compile_now = frame_wants_scene_kernel(P, hdr, *p);
    // the traversal kernel compiled for this scene's light kind / jitter mode / pattern use and, when every object
    // shares one kind / flags word (a triangle mesh, a grid of spheres), for that word as well
    uint32_t first = 0u;
    const bool uniform = like_objects(soa, hdr, &first);
    const std::string b = hex_word(first);
    // Waves per SIMD, i.e. registers per lane (80 at six, 96 at five).  At six the walk's state does not fit and the hot loops spill:
    // hexagons 4096 x 2048 moves 940 MB of HBM-side traffic for its 101 MB canvas at six and 557 MB at five, in the same 0.446 ms;
    // here_be_dragons 1000 x 400 265 -> 151 MB and 0.565 -> 0.533 ms; mesh 1024^2 1.56 -> 1.46 ms, 512 x 384 1.48 -> 1.39; hexagons
    // 1000 x 500, C5, grouped_grid: even.  Only the large frames of divided meshes, whose time is wave slots rather than their
    // longest wave, want the sixth wave: mesh 2048^2 2.03 ms at six / 2.12 at five, here_be_dragons 4000 x 1600 1.71 / 1.83 (and
    // 2000 x 800 0.91 / 0.87 the other way).  profiles/r04_tree_waves.txt.
    p->tree_waves = P.tree_waves ? P.tree_waves : (!p->heavy_tiles.empty() && (uint64_t)hdr.width * hdr.height >= 3000000ull) ? 6 : 5;
    p->spec_defs = {"-DRTC_SPEC_LIST=" + b,
                    uniform ? "-DRTC_SPEC_UNIFORM_BITS=" + b : std::string("-DRTC_SPEC_RUNTIME_BITS=1"),
                    "-DRTC_SPEC_NOBJ=-1", "-DRTC_SPEC_SIMPLE=0",
                    f.reg_waves ? std::string(f.reg_waves) : "-DRTC_WAVES_PER_SIMD=" + std::to_string(p->tree_waves),
                    "-DRTC_SPEC_TBOX=" + std::to_string(hdr.has_tbox)};
    append(&p->spec_defs, d.light);
    append(&p->spec_defs, d.launch);
    append(&p->spec_defs, d.recursion);
    p->spec_name = "render_kernel_spec[" + how + (uniform ? ";all " + b : std::string()) + (hdr.has_patterns ? ";patterns" : "") + "]";
}
// 1 .. 8 objects: the unrolled loops, every object's kind / flags word a compile-time constant
inline void plan_small_kernel(const Policy& P, const SceneHdr& hdr, const std::vector<float4>& soa, const MaterialFacts& f, const CommonDefs& d, ScenePlan* p) {
    const uint32_t n = hdr.n_objects;
    std::vector<std::string>& defs = p->spec_defs;
    p->compile_now = frame_wants_scene_kernel(P, hdr, *p);
    std::string list;
    for (uint32_t i = 0; i < n; i++) list += (i ? "," : "") + hex_word(object_bits(soa, hdr, i));
    defs = {"-DRTC_SPEC_LIST=" + list, "-DRTC_SPEC_NOBJ=" + std::to_string(n), std::string("-DRTC_SPEC_SIMPLE=") + (p->simple ? "1" : "0")};
    append(&defs, d.light);
    defs.push_back(std::string("-DRTC_SPEC_GATES=") + (hdr.n_gates ? "1" : "0"));
    // an area light's geometry as per-lane values in the sample loop (kernel: RTC_LIGHT_VGPRS): the loop's multiplies
    // leave the half-rate class an SGPR operand puts them in, and the compiler no longer re-loads a light vector from
    // the argument block INSIDE the loop when it runs out of scalar registers (C3: 0.988 ms with that load, 0.847
    // without; soft_shadows 2048^2 0.382 -> 0.344; neutral on first_textures and the 1000 x 400 demo frame)
    if (hdr.light_kind == RTC_LIGHT_RECT) defs.push_back("-DRTC_LIGHT_VGPRS");
    append(&defs, d.launch);
    append(&defs, d.recursion);
    if (f.reg_waves) defs.push_back(f.reg_waves);
    // A point light has no sample loop to keep registers free for: cold state stays in VGPRs instead of being parked
    // in LDS around intensity_at (C4 0.86 -> 0.77 ms), and in kernels of a few scale+translate objects the hit
    // object's records are selected from the scalar loads the loops hold anyway instead of being gathered per lane
    // (C4 0.77 -> 0.68 ms; C2 13.9 -> 12.4 us).  Both cost registers that an area light's loop needs (C3 +6 %), and the
    // pattern / rotated-object kernels spill without the parking (reflect_refract 1.21 -> 1.49 ms): left as they were.
    if (hdr.light_kind == RTC_LIGHT_POINT && p->simple && !f.reg_waves) {
        defs.push_back("-DRTC_SPEC_STASH=0");
        // ... and the LDS this frees holds the reflection halves of the recursion frames (five levels, 30 KB per
        // workgroup): C4 0.71 -> 0.63 ms on one box, and its mirror floor no longer writes its recursion to memory
        if (f.any_refl || f.any_refr) defs.push_back("-DRTC_SPEC_LDS_FRAMES=5");
        if (n <= 2) defs.push_back("-DRTC_SPEC_SELECT=1");  // (4 - 6 objects: the selects cost more than the gathers, +13 ... +30 %)
        defs.push_back("-DRTC_WAVES_PER_SIMD=6");
    } else if (hdr.light_kind == RTC_LIGHT_POINT && !f.reg_waves) {
        // ... and the kernels of rotated objects, cylinders, cones and patterns under a point light (round 3): at seven
        // waves per SIMD they spill without the parking (reflect_refract 1.21 -> 1.49 ms, round 2) -- at FIVE (102 VGPRs) they
        // do not, and the LDS holds five levels of reflection halves instead: reflect_refract 4096 x 2048 1.204 -> 0.984 ms
        // (its counters: 64 % of the wave-cycles waiting on memory, 2.4 GB of scratch traffic for a 0.1 GB frame), skybox
        // 0.198 -> 0.188, first_plane / first_patterns -2 %, first_scene +1 % (profiles/r03_ab_point_light_policy.txt)
        defs.push_back("-DRTC_SPEC_STASH=0");
        if (f.any_refl || f.any_refr) defs.push_back("-DRTC_SPEC_LDS_FRAMES=5");
        // ... and FOUR where the world both reflects and transmits and has five objects or more (round 4): reflect_refract's
        // kernel spills 20 registers at five waves (96 VGPRs) and none at four (128) -- 0.874 -> 0.775 ms; skybox (two objects)
        // and the scenes without glass lose up to 12 % at four (profiles/r04_ab_point_light_waves.txt)
        defs.push_back((f.any_refl && f.any_refr && n >= 5u) ? "-DRTC_WAVES_PER_SIMD=4" : "-DRTC_WAVES_PER_SIMD=5");
    } else if (hdr.light_kind == RTC_LIGHT_RECT && !p->simple && !f.reg_waves) {
        // An area light's kernel takes seven waves per SIMD (jit_get's default: C3 0.97 / 0.95 / 1.02 ms at 6 / 7 / 8).  With rotated
        // objects, cylinders, patterns or gates the sample loop's state no longer fits 72 registers and spills: first_textures
        // 4096 x 2048 moves 337 MB HBM-side for its 101 MB canvas at seven and 185 MB at six (84 registers) in the same 0.70 ms; 1024 x
        // 512 and patterns_medley: even, first frames within 2 % either way (profiles/r04_ab_area_light_waves.txt).
        defs.push_back("-DRTC_WAVES_PER_SIMD=6");
    }
    p->spec_name = "render_kernel_spec[" + list + (p->simple ? ";simple" : "") + (hdr.has_patterns ? ";patterns" : "") + (hdr.n_gates ? ";gates" : "") + "]";
}
// many objects: the any-count loop.  When they all share one kind / flags word (C5: 64 scale+translate spheres) that
// word is a compile-time constant -- no per-object kind switch, two 16-byte records per object -- and the policy
// compiles the scene's kernel; a mixed list is left to the ahead-of-time loop (and compiled with run-time words
// only when the recursion is deeper than that kernel's stack)
inline void plan_many_kernel(const Policy& P, const SceneHdr& hdr, const std::vector<float4>& soa, const MaterialFacts& f, const CommonDefs& d, ScenePlan* p) {
    uint32_t first = 0u;
    const bool uniform = like_objects(soa, hdr, &first);
    p->compile_never = !uniform;
    p->compile_now = frame_wants_scene_kernel(P, hdr, *p);
    const std::string b = hex_word(first);
    p->spec_defs = {"-DRTC_SPEC_LIST=" + b, uniform ? "-DRTC_SPEC_UNIFORM_BITS=" + b : std::string("-DRTC_SPEC_RUNTIME_BITS=1"),
                    "-DRTC_SPEC_NOBJ=0", "-DRTC_SPEC_SIMPLE=0"};
    append(&p->spec_defs, d.light);
    append(&p->spec_defs, d.launch);
    if (f.reg_waves) p->spec_defs.push_back(f.reg_waves);
    append(&p->spec_defs, d.recursion);
    p->spec_name = std::string("render_kernel_spec[") + (uniform ? "all " + b : std::string("any")) + (hdr.has_patterns ? ";patterns" : "") + "]";
}

// Which kernel will render the scene that flatten packed into `hdr` and `soa`, and which tiles of the frame matter: everything
// rtc_ctx_set_scene decides between "the records are resident" and the compile.  `camera` may be null (no frame: no coverages).
inline ScenePlan plan_scene(const Policy& P, const SceneHdr& hdr, const std::vector<float4>& soa, const rtc_scene* scene, const rtc_camera* camera,
                            const std::vector<float>& heavy_boxes, const SceneRegion& region) {
    ScenePlan p;
    const uint32_t n = hdr.n_objects;
    p.simple = !hdr.has_patterns;
    for (uint32_t i = 0; i < n; i++)
        if (!simple_shape(object_bits(soa, hdr, i))) p.simple = false;
    project_heavy_boxes(P, heavy_boxes, camera, &p.heavy_tiles, &p.heavy_w, &p.heavy_h);
    // sample-parallel rendering (render_body): compiled in when this frame is small enough to want it
    p.spec_shares = choose_share_log2(hdr, hdr.height, P) != 0u || has_leaf_runs(hdr);  // (kernels of mesh scenes always: their block lists)
    plan_coverage(P, hdr, camera, region, &p);
    // several blocks per workgroup (render_body) where most workgroups see nothing but the sky: the scene's box projects to
    // less than a quarter of the image
    p.spec_blocks_y = p.scene_box_coverage < 0.25f || P.blocks_y != 0;
    // Scene rectangle launches need a few more argument loads and operations in front of every wave, which cost frames of
    // short waves 6 - 10 % (first_plane, first_patterns; C4 0.610 -> 0.648 ms, more than the 3 % its sky rows are worth): only
    // where the rectangle is under half the frame (C5, single_sphere) is the scene's kernel compiled with them.
    p.spec_rect = p.scene_rect[0] < p.scene_rect[1] && p.scene_rect_coverage < P.scene_rect_threshold();
    const MaterialFacts facts = material_facts(P, scene, n);
    // Level-by-level rendering pays where a pixel's ray tree is what makes a frame long: tree worlds with the long leaf runs
    // of divided meshes whose materials both reflect and transmit (every such hit doubles the rays below it)
    p.wf_pays = hdr.n_trav != 0u && hdr.max_leaf_run >= 16u && facts.any_refl && facts.any_refr;
    const CommonDefs defs = common_defs(hdr, p, facts);
    const KernelFamily family = aot_family(hdr.n_trav, n, p.simple);
    p.family_name = family.name();
    p.compile_never = n == 0u;
    if (hdr.n_trav) {
        const std::string how = scene->n_groups ? "tree" : "tree,bvh";
        p.family_name = family.name(how.c_str());
        plan_tree_kernel(P, hdr, soa, how, facts, defs, &p);
    } else if (n >= 1 && n <= 8) {
        plan_small_kernel(P, hdr, soa, facts, defs, &p);
    } else if (n > 8) {
        plan_many_kernel(P, hdr, soa, facts, defs, &p);
    }
    return p;
}

// ---- kernel variants ---------------------------------------------------------------------------------------------------
// One kernel of a scene: the options it is compiled with -- in order: jit_get hashes them into the cache key and the kernel id;
// empty: a world without objects --, the names of the ahead-of-time family and of the scene's own kernel, and which of the four
// kernels it is (rtc_jit.h: entry point, the header beside the core; `k`: the factor of a supersampling or refinement kernel).
// The plan's spec_defs / family_name / spec_name / ss_k are the frame's kernel; the functions below derive every other kernel a
// context keeps from it, and nothing else rewrites an option or a name.
struct KernelVariant {
    std::vector<std::string> defs;
    std::string family_name, spec_name;
    JitKind kind = JitKind::RENDER;
    uint32_t k = 1u;
};
// the launch shapes a variant does not have ("-DRTC_SPEC_RECT=" ...), off in its key
inline void switch_off(std::vector<std::string>* defs, std::initializer_list<const char*> options) {
    for (auto& d : *defs)
        for (const char* o : options)
            if (d == std::string(o) + "1") d.back() = '0';
}
// "kernel<...>" -> "kernel<...;ss=k>", "kernel_spec[...]" likewise (a name that is not there stays empty)
inline std::string with_factor(std::string name, uint32_t k) {
    if (!name.empty()) name.insert(name.size() - 1, ";ss=" + std::to_string(k));
    return name;
}
inline std::string with_prefix(const std::string& name, const char* from, const char* to) {
    return name.rfind(from, 0) == 0 ? to + name.substr(std::strlen(from)) : name;
}
// The frame's kernel of a context of factor k (rtc_supersample.h; 1: the plan's own): ss_render_kernel<...;ss=k>.  The
// supersampling body has neither the loop over blocks nor the rectangle's offsets.
inline KernelVariant render_variant(const ScenePlan& p, uint32_t k = 1u) {
    KernelVariant v = {p.spec_defs, p.family_name, p.spec_name, p.ss_k == 1u ? JitKind::RENDER : p.lens_seam ? JitKind::LENS_SEAM : p.lens ? JitKind::LENS : JitKind::SS, p.ss_k};
    if (k == 1u) return v;
    v.kind = JitKind::SS, v.k = k;
    for (std::string* name : {&v.family_name, &v.spec_name})
        if (!name->empty()) *name = "ss_" + with_factor(*name, k);
    if (!v.defs.empty()) {
        switch_off(&v.defs, {"-DRTC_SPEC_BLOCKS_Y=", "-DRTC_SPEC_RECT="});
        v.defs.push_back("-DRTC_SPEC_SS=" + std::to_string(k));
    }
    return v;
}
// Ray streams (rtc_trace.h): trace_kernel<...>.  No launch shapes, lane sharing among them -- a stream runs one lane per ray, and
// its kernel must not depend on the size of a frame it does not draw.  (Of the plan before plan_supersampled: color_at does not
// read the camera, so a plain and a supersampled context trace with one kernel.)
inline KernelVariant trace_variant(const ScenePlan& p) {
    KernelVariant v = {p.spec_defs, with_prefix(p.family_name, "render_", "trace_"), with_prefix(p.spec_name, "render_", "trace_"), JitKind::TRACE};
    switch_off(&v.defs, {"-DRTC_SPEC_BLOCKS_Y=", "-DRTC_SPEC_RECT=", "-DRTC_SPEC_SHARE="});
    if (!v.defs.empty()) v.defs.push_back("-DRTC_SPEC_TRACE=1");
    return v;
}
// The refinement of an adaptive frame (rtc_adaptive.h), k = 2, 4: adaptive_refine_kernel<...;ss=k>, a ray stream's options with
// its factor in the place of -DRTC_SPEC_TRACE=1.
inline KernelVariant refine_variant(const ScenePlan& p, uint32_t k) {
    KernelVariant v = trace_variant(p);
    v.family_name = with_factor(with_prefix(v.family_name, "trace_", "adaptive_refine_"), k);
    v.spec_name = with_factor(with_prefix(v.spec_name, "trace_", "adaptive_refine_"), k);
    if (!v.defs.empty()) v.defs.back() = "-DRTC_SPEC_ADAPTIVE=" + std::to_string(k);
    v.kind = JitKind::ADAPTIVE, v.k = k;
    return v;
}
// The adaptive kernels of the one-call seam (rtc_adaptive_seam.h; rtc_render_adaptive), k = 2, 4: the refinement of a part's share,
// adaptive_seam_kernel<...;ss=k>; k = 1: its halo pass, adaptive_seam_kernel<...;halo>.  A ray stream's options with
// -DRTC_SPEC_ADAPTIVE_SEAM=k in the place of -DRTC_SPEC_TRACE=1: another kind, so other ids and cache entries than the persistent
// context's refinement kernels, which keep theirs.
inline KernelVariant seam_refine_variant(const ScenePlan& p, uint32_t k) {
    KernelVariant v = trace_variant(p);
    for (std::string* name : {&v.family_name, &v.spec_name}) {
        *name = with_prefix(*name, "trace_", "adaptive_seam_");
        if (!name->empty()) name->insert(name->size() - 1, k == 1u ? std::string(";halo") : ";ss=" + std::to_string(k));
    }
    if (!v.defs.empty()) v.defs.back() = "-DRTC_SPEC_ADAPTIVE_SEAM=" + std::to_string(k);
    v.kind = JitKind::ADAPTIVE_SEAM, v.k = k;
    return v;
}
// A variant with a frame stack of at least `depth` levels, for recursion deeper than RTC_STACK_DEPTH_BASE: 16, 32, ... up to
// RTC_MAX_DEPTH (deep_stack_cap), -DRTC_SPEC_MAX_DEPTH=<cap> last.  The recursion frames of such a kernel all live in per-lane
// scratch -- the LDS placement of the first levels (a tuning of the depth-5 glass-and-mirror frame) is not carried over.
inline int deep_stack_cap(int depth) {
    int cap = 2 * RTC_STACK_DEPTH_BASE;
    while (cap < depth) cap *= 2;
    return std::min(cap, RTC_MAX_DEPTH);
}
inline rtc_status deep_variant(const KernelVariant& v, int depth, KernelVariant* deep) {
    if (v.defs.empty()) return fail(RTC_ERR_INVALID_ARG, "depth %d: no kernel options recorded for this scene", depth);
    *deep = v;
    deep->defs.clear();
    for (const auto& d : v.defs)
        if (d.rfind("-DRTC_SPEC_LDS_FRAMES=", 0) != 0) deep->defs.push_back(d);
    deep->defs.push_back("-DRTC_SPEC_MAX_DEPTH=" + std::to_string(deep_stack_cap(depth)));
    return RTC_OK;
}
// The plan of a supersampled context, k = 2, 4 (`p`: plan_scene of the FINE camera).  Scene tiles, the scene rectangle and several
// blocks per workgroup address the canvas by fine pixels and are not carried over: such scenes are a plain grid, where the
// scene-box early-out still applies; nor is the level-by-level renderer.
inline void plan_supersampled(ScenePlan* p, uint32_t k, bool seam = false) {
    const KernelVariant v = render_variant(*p, k);
    p->spec_defs = v.defs, p->family_name = v.family_name, p->spec_name = v.spec_name, p->ss_k = k;
    // a context of the one-call seam (rtc_render_ss): the variant of the supersampling body that stores bytes and reports its rows
    // (rtc_supersample.h SEAM) -- another option, so another kernel id and cache entry than the persistent context's kernel
    // ... and a name that says so: "ss_seam_render_kernel<...;ss=k>" is the ahead-of-time kernel launched, "ss_render_kernel_spec[...;ss=k;seam]"
    // the scene's own (its entry point keeps its name: the variant is an option of the compile)
    if (seam) {
        if (!p->spec_defs.empty()) p->spec_defs.push_back("-DRTC_SPEC_SS_SEAM=1");
        p->family_name = with_prefix(p->family_name, "ss_render_kernel<", "ss_seam_render_kernel<");
        if (!p->spec_name.empty()) p->spec_name.insert(p->spec_name.size() - 1, ";seam");
    }
    p->scene_tile_mask.clear();
    p->scene_rect[0] = p->scene_rect[1] = p->scene_rect[2] = p->scene_rect[3] = 0u;
    p->spec_blocks_y = p->spec_rect = false;
    p->wf_pays = false;
}
// The plan of a lens context (rtc_lens.h; `p`: plan_supersampled of the same k, never the seam's): the supersampled plan with the
// lens kernel in the supersampling kernel's place -- lens_render_kernel<...;ss=k> / lens_render_kernel_spec[...;ss=k;lens],
// -DRTC_SPEC_LENS=1 last.  What plan_supersampled declines stays declined.  (The scene-box early-out is switched off in the
// launch's header, not here: has_scene_box is run-time data.)
// `seam`: a context of the one-call seam (rtc_render_lens) -- the variant of the lens kernel that stores bytes and reports its rows
// (rtc_lens_seam.h), derived from the same non-seam supersampled plan: -DRTC_SPEC_LENS_SEAM=1 after -DRTC_SPEC_LENS=1, so another
// kernel id and cache entry than the persistent context's, and names that say so -- "lens_seam_render_kernel<...;ss=k>" is the
// ahead-of-time kernel launched, "lens_render_kernel_spec[...;ss=k;lens;seam]" the scene's own (its entry point keeps its name).
inline void plan_lens(ScenePlan* p, bool seam = false) {
    if (!p->spec_defs.empty()) p->spec_defs.push_back("-DRTC_SPEC_LENS=1");
    p->family_name = with_prefix(p->family_name, "ss_render_kernel<", seam ? "lens_seam_render_kernel<" : "lens_render_kernel<");
    p->spec_name = with_prefix(p->spec_name, "ss_render_kernel_spec[", "lens_render_kernel_spec[");
    if (!p->spec_name.empty()) p->spec_name.insert(p->spec_name.size() - 1, seam ? ";lens;seam" : ";lens");
    if (seam && !p->spec_defs.empty()) p->spec_defs.push_back("-DRTC_SPEC_LENS_SEAM=1");
    p->lens = true;
    p->lens_seam = seam;
}

}  // namespace rtc

#endif
