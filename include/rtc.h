/*
 * rtc.h -- C ABI of the MI355X-native render path (librtc_amd.so).
 *
 * This is the drop-in boundary for ONE hot path of
 * garfieldnate/ray_tracer_challenge: the body of
 *
 *     pub fn render(&self, world: World, reflection_recursion_depth: i16) -> Canvas
 *                                                  (lib/src/camera.rs:76-91)
 *
 * and everything it calls per pixel (ray_for_pixel, World::color_at / intersect /
 * shade_hit / is_shadowed / reflected_color / refracted_color, the Sphere /
 * Plane / Cube / Cylinder / Cone intersectors, phong_lighting with the
 * procedural patterns of the pattern module).  The reference has no
 * FFI of its own; INTEGRATION.md shows the `extern "C"` block a maintainer
 * would add to camera.rs to bind these entry points.
 *
 * Plain C: POD structs, pointers and sizes only.  No C++ or torch types cross
 * this boundary.  The library owns all device memory it allocates; the caller
 * owns every buffer it passes in.  All matrices are row-major 4x4 f32.
 *
 * File:line citations are relative to /root/reference/lib/src.
 */
#ifndef RTC_H
#define RTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTC_ABI_VERSION 8 /* (rtc_ctx_trace_hits and rtc_ctx_is_shadowed were added at 8: two entry points more, no struct and
                             no existing signature changed, so callers built against the earlier 8 run unchanged; likewise
                             adaptive supersampling: rtc_ctx_render_adaptive, rtc_ctx_adaptive_stats, rtc_ctx_adaptive_kernel_name
                             / _id and the struct rtc_adaptive_stats are additions, nothing that existed has moved;
                             ray reordering: rtc_ctx_ray_order, rtc_ctx_trace_reordered, rtc_ctx_reorder_stats and the struct
                             rtc_reorder_stats, additions likewise; supersampling through the one-call seam: rtc_render_ss, one
                             entry point more -- rtc_opts and rtc_stats are what they were; the thin-lens camera: rtc_lens_rays,
                             rtc_ctx_set_scene_lens and the struct rtc_lens, additions likewise; the lens through the one-call
                             seam: rtc_render_lens, one entry point more, no struct changed;
                             adaptive supersampling through the one-call seam: rtc_render_adaptive and the struct
                             rtc_seam_adaptive_stats are additions, rtc_adaptive_stats keeps its layout) */
/* reflection_recursion_depth (camera.rs:76: any i16; reference default 5, constants.rs:4; its author renders
 * reflect_refract at 20).  Accepted: 0 .. RTC_MAX_DEPTH.  The kernels keep one frame per suspended shade_hit
 * (world.rs:62-86); up to RTC_STACK_DEPTH_BASE levels every kernel has them, above that the scene's kernel is compiled
 * once more, on first use, with a stack of 16 / 32 / ... levels in per-lane scratch (a second or so; cached like every
 * scene kernel).  Beyond RTC_MAX_DEPTH the call is refused -- the reference would be recursing that deep on its own
 * call stack.  rtc_color_at (a batched test entry point) stops at RTC_STACK_DEPTH_BASE. */
#define RTC_MAX_DEPTH 255
#define RTC_STACK_DEPTH_BASE 8

typedef enum rtc_status {
    RTC_OK = 0,
    RTC_ERR_INVALID_ARG = -1, /* null pointer, zero size, depth out of range ...        */
    RTC_ERR_UNSUPPORTED = -2, /* unknown shape kind, projective transform, closure jitter */
    RTC_ERR_NO_LIGHT = -3,    /* world.rs:66 "World light should be set"                 */
    RTC_ERR_DEVICE = -4,      /* HIP runtime error; text via rtc_last_error()            */
    RTC_ERR_NO_DEVICE = -5    /* no gfx950 device visible: there is NO CPU fallback      */
} rtc_status;

/* shape/{sphere,plane,cube,cylinder,cone,triangle}.rs.  A SmoothTriangle is passed as RTC_TRIANGLE: its
 * local_intersect hands out intersections whose object is the inner flat Triangle (smooth_triangle.rs:37-39), so
 * inside Camera::render it is shaded exactly like one. */
enum { RTC_SPHERE = 0, RTC_PLANE = 1, RTC_CUBE = 2, RTC_CYLINDER = 3, RTC_CONE = 4, RTC_TRIANGLE = 5 };
/* pattern/{stripes,gradient,rings,checkers,sine_2d}.rs; NONE = Material.pattern is None (material.rs:50) */
enum { RTC_PATTERN_NONE = 0, RTC_PATTERN_STRIPES = 1, RTC_PATTERN_GRADIENT = 2, RTC_PATTERN_RINGS = 3,
       RTC_PATTERN_CHECKERS = 4, RTC_PATTERN_SINE2D = 5,
       RTC_PATTERN_TEXTURE_MAP = 6, /* pattern/uv.rs:62-89 TextureMap: one UV pattern through a UV mapping   */
       RTC_PATTERN_CUBE_MAP = 7     /* pattern/uv.rs:200-262 CubicMap: six UV patterns, one per cube face     */ };
/* pattern/uv.rs: UVCheckers :20-55, AlignCheck :125-167, UVImage :347-377 */
enum { RTC_UV_CHECKERS = 1, RTC_UV_ALIGN_CHECK = 2, RTC_UV_IMAGE = 3 };
/* pattern/uv.rs: SphericalMap :91-105, PlanarMap :180-186, CylindricalMap :188-198 */
enum { RTC_MAP_SPHERICAL = 1, RTC_MAP_PLANAR = 2, RTC_MAP_CYLINDRICAL = 3 };
/* light/{point_light,rectangle_light}.rs */
enum { RTC_LIGHT_POINT = 0, RTC_LIGHT_RECT = 1 };
/* RectangleLight jitter source.  The reference takes an arbitrary closure
 * (rectangle_light.rs:27,44-47); a device cannot call one, so two pinned
 * sources are offered: the constant of test/utils.rs:15-17, and a counter-based
 * hash (DESIGN.md "Jitter") standing in for thread_rng(). */
enum { RTC_JITTER_CONSTANT = 0, RTC_JITTER_HASHED = 2,
       /* test/utils.rs:19-24 hardcoded_jitter: a short list of values handed out in a cycle.  The cycle is STATE that
        * the reference carries from call to call (a RefCell inside the closure), serial across everything a light is
        * asked: only the entry points that stand for ONE call on a freshly built light accept it -- rtc_intensity_at
        * (every point is answered as by a new light: draw k of the call is value k mod n, two draws per cell in
        * rectangle_light.rs:76-88's order) and rtc_point_on_light; rtc_render / rtc_ctx_set_scene / rtc_color_at refuse. */
       RTC_JITTER_SEQUENCE = 3 };
#define RTC_JITTER_SEQUENCE_MAX 16
/* The most cells, u_steps x v_steps, a rectangle light may have: 2^24.  rectangle_light.rs:76-88 adds 1.0 per lit sample in
 * f32, and an f32 sum of ones stops growing at 2^24: with more cells the reference answers a fully lit point with
 * 2^24 / cells, not 1.0, and none of the library's ways to answer samples without tracing them reproduces that.
 * rtc_rectangle_light, rtc_scene_validate and every call that takes a scene refuse such a light with RTC_ERR_UNSUPPORTED
 * (the product is formed in 64 bits: 65 536 x 65 536 is refused, not wrapped). */
#define RTC_LIGHT_CELLS_MAX 16777216

/* A boxed Pattern (pattern/pattern.rs:8-26) flattened: the two colours every pattern is built from and
 * BasePattern.t_inverse (pattern.rs:33,52-54).  Gradient and Sine2D keep `distance = b - a`
 * (gradient.rs:17, sine_2d.rs:17); the library forms it from a and b with the same single subtraction.
 * Build with rtc_pattern_init().  (uv.rs texture maps are not on this path.) */
/* One boxed UVPattern (pattern/uv.rs:14-16). */
typedef struct rtc_uv_pattern {
    int32_t kind;           /* RTC_UV_* */
    float width, height;    /* UVCheckers */
    float colors[5][3];     /* UVCheckers: a, b.  AlignCheck: main, ul, ur, bl, br */
    uint32_t image_width;   /* UVImage: its Canvas (canvas.rs:6-10) as image_height rows of image_width RGB f32,  */
    uint32_t image_height;  /* i.e. Canvas.data[y][x]; host memory, copied into HBM by rtc_ctx_set_scene          */
    const float* image_rgb;
} rtc_uv_pattern;

typedef struct rtc_pattern {
    int32_t kind; /* RTC_PATTERN_* */
    float a[3];
    float b[3];
    float inv[16];
    int32_t uv_mapping;       /* TEXTURE_MAP: RTC_MAP_*                                                         */
    uint32_t n_uv;            /* TEXTURE_MAP: 1.  CUBE_MAP: 6, in CubicMap::new's order front, back, left, right, */
    const rtc_uv_pattern* uv; /* up, down (uv.rs:207-231).  Read during rtc_ctx_set_scene / the batched calls.    */
} rtc_pattern;

/* material.rs:18-51 */
typedef struct rtc_material {
    float color[3];
    float ambient;
    float diffuse;
    float specular;
    float shininess;
    float reflective;
    float transparency;
    float refractive_index;
    rtc_pattern pattern; /* kind RTC_PATTERN_NONE: use `color` (phong_lighting.rs:24-27) */
} rtc_material;

/* One entry of World.objects (world.rs:19), flattened.  `inv` is exactly
 * BaseShape.t_inverse (shape/base_shape.rs:17,58); the inverse-transpose is
 * its transpose and is not stored.  Object order is World.objects order: hit
 * tie-breaking depends on it (world.rs:58, intersection.rs:30-35). */
typedef struct rtc_object {
    int32_t kind;         /* RTC_SPHERE ... */
    int32_t casts_shadow; /* BaseShape.casts_shadow, base_shape.rs:14 */
    int32_t closed;       /* Cylinder.closed / Cone.closed, cylinder.rs:18, cone.rs:16 */
    float min_y;          /* Cylinder/Cone.minimum_y (ignored for other kinds) */
    float max_y;          /* Cylinder/Cone.maximum_y */
    float inv[16];
    rtc_material material;
    float p1[3], p2[3], p3[3]; /* Triangle.p1..p3 (triangle.rs:11-13); e1, e2 and the normal are re-derived by
                                  the library exactly as Triangle::new does (:20-22).  Ignored for other kinds. */
} rtc_object;

/* light/point_light.rs:7-10 and light/rectangle_light.rs:12-31 AFTER
 * RectangleLight::new: u_vec/v_vec are the per-cell vectors (already divided by
 * the step counts, :51-52) and `position` is the rectangle centre (:57) or the
 * point light's position.  Build with rtc_point_light()/rtc_rectangle_light(). */
typedef struct rtc_light {
    int32_t kind;
    float intensity[3];
    float position[4];
    float corner[4];
    float u_vec[4];
    float v_vec[4];
    int32_t u_steps;
    int32_t v_steps;
    int32_t jitter_mode;
    float jitter_const;
    uint32_t jitter_seed;
    uint32_t jitter_seq_len;                      /* RTC_JITTER_SEQUENCE: 1 .. RTC_JITTER_SEQUENCE_MAX values ... */
    float jitter_seq[RTC_JITTER_SEQUENCE_MAX];    /* ... set by rtc_light_set_jitter_sequence()                   */
} rtc_light;

/* One GroupShape (shape/group.rs:12-16) of the flattened world.  add_child / set_transformation bake a
 * group's transform into its children (group.rs:39-44,101-114) and Shape::intersect on a group does not
 * transform the ray (:115-117), so a tree of groups flattens to its leaf shapes -- listed in `objects` in
 * depth-first order, which is the order the reference's child loops push intersections in -- plus, per
 * group, the contiguous run of leaves under it and the bounding box that gates them (:119-133).
 * Groups are listed in pre-order (a group before the groups nested inside it); runs nest properly. */
typedef struct rtc_group {
    uint32_t first_object;
    uint32_t n_objects;   /* 0: an empty group (never hit; ignored) */
    float bounds_min[3];  /* GroupShape::bounding_box(), group.rs:138-151 (world space) */
    float bounds_max[3];
} rtc_group;

/* world.rs:18-21 */
typedef struct rtc_scene {
    uint32_t n_objects;
    const rtc_object* objects;
    const rtc_light* light; /* NULL -> RTC_ERR_NO_LIGHT */
    uint32_t n_groups;      /* 0: World.objects is a flat list of shapes */
    const rtc_group* groups;
} rtc_scene;

/* camera.rs:8-21 after Camera::new.  Build with rtc_camera_new(). */
typedef struct rtc_camera {
    uint32_t width;
    uint32_t height;
    float field_of_view;
    float half_width;
    float half_height;
    float pixel_size;
    float inv[16]; /* transform_inverse */
} rtc_camera;

/* Row partition of one image over several devices (one process per GPU).
 * The image is cut into bands of `band_rows` rows; band b belongs to part
 * (b mod n_parts).  A part's rows are stored compactly, band after band. */
typedef struct rtc_partition {
    uint32_t band_rows; /* 0 -> 64 */
    uint32_t n_parts;   /* 0 -> 1  */
    uint32_t part;
} rtc_partition;

/* A thin lens in front of a camera (rtc_ctx_set_scene_lens, rtc_lens_rays): rays leave from a disc of aperture_radius around the
 * camera's origin, in the plane of its x and y axes, and meet where the pinhole's ray is at focal_distance times its unnormalised
 * length (the plane in focus: camera-space z = -focal_distance).  aperture_radius >= 0, focal_distance > 0, both finite. */
typedef struct rtc_lens {
    float aperture_radius;
    float focal_distance;
    uint32_t seed; /* of the lens points' jitter */
} rtc_lens;

typedef struct rtc_stats {
    uint64_t rays;        /* World::intersect evaluations of the last launch (primary, shadow, reflect, refract) */
    uint64_t shaded_hits; /* shade_hit evaluations of the last launch (world.rs:62)                           */
    uint64_t pixels;      /* traced pixels: (w-1)*(h-1) restricted to the rows rendered                        */
    float kernel_ms;      /* mean HIP-event time of the render kernel over `launches`                          */
    uint32_t launches;    /* render launches since the previous rtc_ctx_stats call                             */
    uint32_t rows;        /* rows written to the output buffer                                                 */
    uint64_t culled_shadow_rays; /* of `rays`: area-light shadow rays whose answer ("lit") followed from the
                                    conservative light-cone cull, i.e. that tested no object       */
    uint32_t flags;       /* RTC_STATS_*                                                                       */
    float gather_ms;      /* rtc_render_ex: wall time from the first render launch to the last row's arrival in `out`
                             minus nothing -- i.e. the whole render + transport pipeline of the call (0 elsewhere)  */
} rtc_stats;
/* rtc_stats.flags: the scene's kernel is an ahead-of-time instantiation although the specialisation policy asked for a
 * scene-compiled one (hiprtc failed; same image, several times slower on area-light scenes).  rtc_ctx_jit_status()
 * holds the compiler's message. */
#define RTC_STATS_JIT_FALLBACK 1u

/* Options of rtc_render_ex (SURVEY.md 8(b) `opts`).  Zero-initialise for the defaults. */
typedef struct rtc_opts {
    const int32_t* devices; /* the GPUs to split the image over (64-row bands dealt round-robin, camera.rs:80-85 has no   */
    uint32_t n_devices;     /* order dependence between pixels); NULL / 0: device 0.  A device may be listed twice.      */
    uint32_t band_rows;     /* 0 -> 64 */
    int32_t quantize;       /* 0: `out` receives width*height*3 f32 (the Canvas);  1: width*height*3 u8 -- every channel */
                            /* through scale_color (canvas.rs:39-43), i.e. the numbers Canvas::to_ppm prints             */
    int32_t out_on_device;  /* 0: `out` is host memory (pinned memory from rtc_host_alloc is written without staging);   */
                            /* 1: `out` is device memory on devices[0]: peers' bands travel GPU-to-GPU (xGMI)            */
} rtc_opts;

typedef struct rtc_ctx rtc_ctx;

/* ------------------------------------------------------------------------
 * Host-side scene math.  Restates matrix.rs / transformations.rs /
 * tuple.rs / camera.rs:23-74 operation for operation so that the flattened
 * scene handed to the kernel is bit-identical to what the Rust structs hold.
 * Pure host code; usable without a GPU.
 * ---------------------------------------------------------------------- */
void rtc_translation(float x, float y, float z, float out[16]);                 /* transformations.rs:4-6   */
void rtc_scaling(float x, float y, float z, float out[16]);                     /* :8-10  */
void rtc_rotation_x(float radians, float out[16]);                              /* :12-21 */
void rtc_rotation_y(float radians, float out[16]);                              /* :23-32 */
void rtc_rotation_z(float radians, float out[16]);                              /* :34-43 */
void rtc_shearing(float xy, float xz, float yx, float yz, float zx, float zy, float out[16]); /* :46-53 */
void rtc_view_transform(const float from[4], const float to[4], const float up[4], float out[16]); /* :57-68 */
void rtc_mat_mul(const float a[16], const float b[16], float out[16]);          /* matrix.rs:86-103  */
void rtc_mat_vec(const float a[16], const float v[4], float out[4]);            /* matrix.rs:73-84   */
void rtc_mat_transpose(const float* a, int n, float* out);                      /* matrix.rs:134-143 */
float rtc_mat_determinant(const float* a, int n);                               /* matrix.rs:145-160 */
void rtc_mat_submatrix(const float* a, int n, int row, int col, float* out);    /* matrix.rs:163-182 */
float rtc_mat_minor(const float* a, int n, int row, int col);                   /* matrix.rs:194-196 */
float rtc_mat_cofactor(const float* a, int n, int row, int col);                /* matrix.rs:184-192 */
rtc_status rtc_mat_inverse(const float* a, int n, float* out);                  /* matrix.rs:201-212 */
float rtc_magnitude(const float v[4]);                                          /* tuple.rs:29-33 */
void rtc_norm(const float v[4], float out[4]);                                  /* tuple.rs:34-43 */
float rtc_dot(const float a[4], const float b[4]);                              /* tuple.rs:44-46 */
void rtc_cross(const float a[4], const float b[4], float out[4]);               /* tuple.rs:47-55 */
void rtc_reflect(const float in[4], const float normal[4], float out[4]);       /* ray.rs:42-44   */

/* Material::default(), material.rs:53-57 (no pattern) */
void rtc_material_default(rtc_material* out);
/* Stripes/Gradient/Rings/Checkers/Sine2D::new(a, b) followed by set_transformation(transform):
 * stores transform.inverse() (pattern.rs:52-54).  transform NULL = identity. */
rtc_status rtc_pattern_init(rtc_pattern* out, int32_t kind, const float a[3], const float b[3],
                            const float transform[16]);
/* TextureMap::new(uv_pattern, uv_mapping) (uv.rs:68-76; uv_mapping = RTC_MAP_*, n_uv = 1) or CubicMap::new(front,
 * back, left, right, up, down) (uv.rs:207-231; uv_mapping = 0, n_uv = 6), then set_transformation(transform).
 * `uv` is borrowed, not copied. */
rtc_status rtc_texture_map_init(rtc_pattern* out, int32_t uv_mapping, const rtc_uv_pattern* uv, uint32_t n_uv,
                                const float transform[16]);
/* canvas_from_ppm (canvas.rs:120-197): parses P3 text into a malloc'd width*height*3 f32 image (free with
 * rtc_free).  Errors: RTC_ERR_INVALID_ARG with the ParseError variant's name in rtc_last_error(). */
rtc_status rtc_canvas_from_ppm(const char* text, uint64_t len, uint32_t* width, uint32_t* height, float** out_rgb);
/* Shape::build(transform, material): stores transform.inverse() (base_shape.rs:56-60).
 * Cylinder / Cone bounds default to -inf/+inf, open (cylinder.rs:34-43, cone.rs:33-42). */
rtc_status rtc_object_init(rtc_object* out, int32_t kind, const float transform[16], const rtc_material* m);
/* bounding_box.rs, operation for operation (f32::min / max ignore a NaN operand; points carry w = 1).
 * Host-side helpers for building rtc_group records the way GroupShape::bounding_box / divide do. */
void rtc_bounds_empty(float mn[4], float mx[4]);                                                  /* :13-20  */
void rtc_bounds_add(float mn[4], float mx[4], const float other_mn[4], const float other_mx[4]);  /* :37-50  */
int32_t rtc_bounds_contains(const float mn[4], const float mx[4], const float other_mn[4],
                            const float other_mx[4]);                                             /* :52-60  */
void rtc_bounds_transform(const float mn[4], const float mx[4], const float m[16], float out_mn[4],
                          float out_mx[4]);                                                       /* :62-79  */
void rtc_bounds_split(const float mn[4], const float mx[4], float left_mn[4], float left_mx[4],
                      float right_mn[4], float right_mx[4]);                                      /* :85-113 */
/* Shape::bounding_box (sphere.rs:75-80, plane.rs:61-66, cube.rs:82-87, cylinder.rs:74-79, cone.rs:75-85);
 * with transform != NULL, Shape::parent_space_bounding_box (shape.rs:162-164) for that transformation(). */
rtc_status rtc_shape_bounds(int32_t kind, float min_y, float max_y, const float transform[16], float mn[4],
                            float mx[4]);
/* the same for a Triangle (triangle.rs:74-80) */
void rtc_triangle_bounds(const float p1[3], const float p2[3], const float p3[3], const float transform[16],
                         float mn[4], float mx[4]);
/* Triangle::new's derived fields (triangle.rs:20-22): e1 = p2 - p1, e2 = p3 - p1, normal = e2.cross(e1).norm() */
void rtc_triangle_fields(const float p1[3], const float p2[3], const float p3[3], float e1[3], float e2[3],
                         float normal[3]);
void rtc_point_light(const float position[4], const float intensity[3], rtc_light* out);   /* point_light.rs:12-19 */
rtc_status rtc_rectangle_light(const float intensity[3], const float corner[4], const float u_vec[4],
                               int32_t u_steps, const float v_vec[4], int32_t v_steps, int32_t jitter_mode,
                               float jitter_const, uint32_t jitter_seed, rtc_light* out); /* rectangle_light.rs:33-58 */
/* hardcoded_jitter(values) of test/utils.rs:19-24 for a light built with jitter mode RTC_JITTER_SEQUENCE (see the enum) */
rtc_status rtc_light_set_jitter_sequence(rtc_light* light, const float* values, uint32_t n);
rtc_status rtc_camera_new(uint32_t width, uint32_t height, float field_of_view, const float transform[16],
                          rtc_camera* out);                                               /* camera.rs:23-56 */
void rtc_ray_for_pixel(const rtc_camera* c, uint32_t x, uint32_t y, float origin[4], float direction[4]); /* camera.rs:60-74 */
/* The fine camera of a supersampled frame (rtc_ctx_set_scene_ss): Camera::new(k W, k H, field_of_view, transform) for a camera
 * of W x H pixels built by rtc_camera_new -- the same half_width, half_height and inverse transform, pixel_size =
 * (half_width * 2) / (k W as f32).  k = 1, 2 or 4; any other k, or a fine frame beyond what a launch addresses (2^32 pixels:
 * the pixel index is the jitter key; 2^17 rows), is RTC_ERR_INVALID_ARG with a message.  Host only. */
rtc_status rtc_camera_supersampled(const rtc_camera* camera, uint32_t k, rtc_camera* fine);
/* The rays of a lens frame (rtc_ctx_set_scene_lens), which this function DEFINES: k x k rays per pixel of `output_camera` (W x H),
 * k = 2 or 4, each from its own point of the lens.  Let Cf = rtc_camera_supersampled(output_camera, k).  The ray of fine pixel
 * (x, y) of Cf, all in f32, nothing fused, operands in the order written:
 *  1. o, p: the origin and the world-space pixel point of ray_for_pixel (camera.rs:60-74) for (x, y) of Cf, before it normalises.
 *  2. key = y * k W + x.  ju = J(mix32(mix32(key ^ seed) + 1 * 0x9E3779B9)), jv = J(mix32(mix32(key ^ seed) + 2 * 0x9E3779B9)), where
 *     mix32(h): h ^= h >> 16, h *= 0x7feb352d, h ^= h >> 15, h *= 0x846ca68b, h ^= h >> 16 (32-bit) and J(h) = ((h >> 9) + 1) * 2^-23,
 *     in (0, 1] -- the keyed hash of RTC_JITTER_HASHED lights.
 *  3. i = x mod k, j = y mod k; the lens cell is the sub-pixel cell turned by a quarter: ci = j, cj = k - 1 - i.
 *     u = ((float)ci + ju) / (float)k, v = ((float)cj + jv) / (float)k, r = aperture_radius * sqrtf(u), theta = 6.2831855f * v,
 *     lx = r * cosf(theta), ly = r * cosf(theta - 1.5707964f).  sqrtf is IEEE, cosf the C library's (glibc: correctly rounded in
 *     practice; the kernels carry a bit-exact restatement).
 *  4. right = (inv[0], inv[4], inv[8]), up = (inv[1], inv[5], inv[9]) of the camera; o' = (o + right * lx) + up * ly, per component.
 *  5. P = o + (p - o) * focal_distance; d = (P - o') / |P - o'| (tuple.rs:29-43: the square root of the sum of squares, three divisions).
 * Writes the rays of fine rows y0 .. y0 + n_rows - 1, every column, in image order, to HOST buffers in rtc_ctx_trace's layout:
 * origins[j] = (o', 1), directions[j] = (d, 0), 16 bytes each, j = (y - y0) * k W + x; either may be NULL.  The last fine row
 * and column are written too (a lens frame does not trace them).  Host only, no device.  RTC_ERR_INVALID_ARG with a message: a
 * null camera or lens, k not 2 or 4, aperture_radius negative or not finite, focal_distance <= 0 or not finite, a fine frame
 * rtc_camera_supersampled refuses, y0 + n_rows beyond k H. */
rtc_status rtc_lens_rays(const rtc_camera* output_camera, uint32_t k, const rtc_lens* lens, uint32_t y0, uint32_t n_rows,
                         float* origins, float* directions);

/* Runs the checks and the flattening rtc_ctx_set_scene performs (shape / pattern kinds, affine transforms, group
 * nesting, light and camera sanity), without touching a device: RTC_OK, or the status rtc_ctx_set_scene would
 * return with its message in rtc_last_error().  camera may be NULL. */
rtc_status rtc_scene_validate(const rtc_scene* scene, const rtc_camera* camera);

/* ------------------------------------------------------------------------
 * Device path.  Every function below needs a gfx950 GPU and fails with
 * RTC_ERR_NO_DEVICE otherwise.
 * ---------------------------------------------------------------------- */

/* Camera::render (camera.rs:76-91) in one call: uploads the scene, renders the
 * whole image on device `device`, copies it back.  out_rgb: caller-owned host
 * buffer of width*height*3 f32, row-major [y][x][rgb], fully written -- the
 * last row and last column stay black exactly as in the reference
 * (camera.rs:80-81).  (A supersampled context, rtc_ctx_set_scene_ss, leaves the FINE frame's last row and column black:
 * its output's last row and column are dimmed, not black.)  stats may be NULL. */
rtc_status rtc_render(const rtc_scene* scene, const rtc_camera* camera, int32_t depth, int32_t device,
                      float* out_rgb, rtc_stats* stats);

/* The same with options: several devices (the image's bands are dealt round-robin over opts->devices, each device
 * renders its bands while the previous ones are on their way to `out`), bytes instead of floats, device-resident
 * output.  Contexts, device buffers, pinned staging memory and compiled kernels are kept per device between calls
 * (rtc_render_release drops them), so a second frame costs the kernel plus the transfer.  stats: rays / shaded hits /
 * pixels summed over the devices, kernel_ms = the largest per-device sum of kernel times, gather_ms = wall time of
 * the render + transfer pipeline.  rtc_render(scene, camera, depth, device, out, stats) is rtc_render_ex with
 * opts = {devices = &device, n_devices = 1}.
 * Which kernel: the reference renders one frame per process (camera.rs:76), and compiling a scene's own kernel takes 0.5 - 2 s
 * where the frame it speeds up takes milliseconds.  These calls therefore render a scene with the ahead-of-time kernels the first time a
 * process sees it -- unless its compiled kernel is already in the disk cache (<library dir>/jit_cache) -- and compile it when the same
 * scene is rendered again, for that process and, through the cache, for every later one.  Same frames either way.
 * RTC_AMD_SPECIALIZE=1 compiles at first sight, =0 never; the persistent contexts below (rtc_ctx_set_scene) always compile at once. */
rtc_status rtc_render_ex(const rtc_scene* scene, const rtc_camera* camera, int32_t depth, const rtc_opts* opts,
                         void* out, rtc_stats* stats);
/* rtc_render_ex with k x k rays per pixel of `output_camera` (W x H), reduced inside the render kernel: the frame that
 * rtc_ctx_set_scene_ss defines (below: the fixed-order f32 box filter of the fine camera's frame, jitter keys from the fine pixel
 * index, last row and column dimmed), in one call, with everything rtc_render_ex offers -- `out` is H x W x 3 f32, or bytes with
 * opts->quantize (scale_color of the reduced colour), host memory (pageable or page-locked) or device memory
 * (opts->out_on_device); the rows leave chunk by chunk while later rows render; opts->band_rows counts OUTPUT rows (0 -> 64) and
 * the bands are dealt round-robin over opts->devices (a device may be listed several times, and may own no row).  The fine
 * frame never exists in memory and never crosses the link: a call moves 1 / k^2 of what rtc_render_ex of the fine camera moves.
 * k = 1 is rtc_render_ex; k = 2 or 4; any other k, or a fine frame rtc_camera_supersampled refuses, is RTC_ERR_INVALID_ARG with
 * a message, decided on the host before any device call, in the order rtc_render_ex checks its arguments (null `out` or camera,
 * empty canvas, then k).  The per-device state is rtc_render_ex's own: calls with k = 1, 2, 4 of one scene may alternate, each
 * gives its own frame (another factor is another kernel: the scene is planned again, its records stay resident), and
 * rtc_render_release frees it.  Its contexts launch a variant of the supersampling kernels of their own (bytes, write-through stores,
 * progress words; named "ss_seam_render_kernel<...;ss=k>" / "ss_render_kernel_spec[...;ss=k;seam]", ids "aot_ss<k>_<hash>.seam" /
 * "spec_..."), never the kernels of rtc_ctx_set_scene_ss's contexts.  A launch drawn from a block list (a divided mesh under a point light) cannot report its rows:
 * its chunks leave when its stream is done, as in rtc_render_ex.  stats: rays, shaded_hits and pixels are the fine frame's
 * ((k W - 1)(k H - 1) pixels), summed over the devices; rows = H; launches = one per entry of opts->devices that owns a row,
 * however many chunks its rows leave in; kernel_ms and gather_ms as for rtc_render_ex. */
rtc_status rtc_render_ss(const rtc_scene* scene, const rtc_camera* output_camera, int32_t depth, uint32_t k,
                         const rtc_opts* opts, void* out, rtc_stats* stats);
/* rtc_render_ss through a thin lens: depth of field in one call.  The frame is the one rtc_ctx_set_scene_lens defines (below: the
 * box filter of the fine frame whose pixel is World::color_at of the ray rtc_lens_rays gives it, jitter key y * k W + x, the fine
 * frame's last row and column zero), with everything rtc_render_ss offers: `out` is H x W x 3 f32, or bytes with opts->quantize
 * (scale_color of the reduced colour); pageable, page-locked or device memory (opts->out_on_device); opts->band_rows counts OUTPUT
 * rows (0 -> 64), the bands are dealt round-robin over opts->devices (an entry may repeat and may own no row: a ray depends only on
 * its global fine (x, y), so any split assembles to the same frame); the rows leave chunk by chunk while later rows render.
 * RTC_ERR_INVALID_ARG with a message, decided on the host before any device call, in this order: null `out` or camera, empty
 * canvas (rtc_render_ss's checks), then a null lens (an error, not rtc_render_ss), k not 2 or 4 (k = 1 with a lens is an error),
 * aperture_radius negative or not finite, focal_distance <= 0 or not finite, a fine frame rtc_camera_supersampled refuses.  A
 * valid call on a machine without a device: RTC_ERR_NO_DEVICE.
 * The per-device state is the seam's own: calls of rtc_render_ex, rtc_render_ss and rtc_render_lens of one scene may alternate,
 * each gives its own frame, and rtc_render_release frees it.  A second rtc_render_lens of the same scene, camera and k with
 * another lens is a focus pull: nothing is planned, compiled or uploaded (rtc_ctx_set_scene's rule for the resident scene) -- three words of the
 * launch's arguments change.  Its contexts launch a variant of the lens kernels of their own (bytes, write-through stores, progress
 * words; csrc/rtc_lens_seam.h), never the kernels of rtc_ctx_set_scene_lens's contexts: named "lens_seam_render_kernel<...;ss=k>" /
 * "lens_render_kernel_spec[...;ss=k;lens;seam]", ids "aot_lens<k>_<hash>.seam" -- the hash is the variant's own: it folds in the
 * text of rtc_lens_seam.h after the two headers the persistent lens kernel's hash folds in -- / "spec_..." (one option more,
 * -DRTC_SPEC_LENS_SEAM=1, so another cache entry).  Which kernel renders a scene's first frame: as for rtc_render_ex
 * (RTC_AMD_SPECIALIZE).  A launch drawn from a block list cannot report its rows: its chunks leave when its stream is done.
 * stats: as for rtc_render_ss -- pixels = (k W - 1)(k H - 1), rows = H, launches = one per entry of opts->devices that owns a row. */
rtc_status rtc_render_lens(const rtc_scene* scene, const rtc_camera* output_camera, int32_t depth, uint32_t k, const rtc_lens* lens,
                           const rtc_opts* opts, void* out, rtc_stats* stats);
/* Adaptive supersampling in one call (DESIGN.md 8e "one-call seam"): k x k rays only where neighbouring pixels of the base frame
 * differ.  The frame is exactly rtc_ctx_render_adaptive's O, items (1)-(4) of its comment below -- base frame B, mask M over the
 * WHOLE frame's four neighbours, supersampled frame S, O = S where M and B elsewhere -- for every value of `opts`: any devices
 * list (entries may repeat and may own no row), any band_rows (0 -> 64, counted in output rows), f32 or bytes.  A band's first and
 * last row have a neighbour in a band another entry renders: every entry traces those rows of B itself -- its halo rows, at most
 * two per band, each pixel exactly B's pixel -- so any split assembles to the same frame and the same mask.
 * `out`: H x W x 3 f32, or with opts->quantize H x W x 3 bytes, scale_color of O per channel (the threshold always compares the
 * f32 B).  mask_u8: H x W bytes, 1 = refined, 0 = not; may be NULL.  Both in the memory opts->out_on_device names: host memory,
 * pageable or page-locked, or device memory on devices[0].
 * RTC_ERR_INVALID_ARG with a message, decided on the host before any device call, in this order: null `out` or camera, empty
 * canvas (rtc_render_ss's checks), a threshold that is not finite or is negative, k other than 2 or 4, a fine frame
 * rtc_camera_supersampled refuses.  A valid call on a machine without a device: RTC_ERR_NO_DEVICE.
 * stats: rays, shaded_hits and pixels are the BASE frame's, summed over the entries -- rtc_render_ex's for the same scene whatever
 * the split --, rows = H; launches, kernel_ms (the base pass's kernels) and gather_ms (the whole call) as for rtc_render_ss.
 * `ad` (may be NULL): what the other passes did.  halo_pixels counts every pixel of every halo row, W per row; it is 0 when
 * consecutive bands of an entry are adjacent (one entry).  mask_ms covers the halo pass and the mask kernel.
 * Kernels (csrc/rtc_adaptive_seam.h): the base pass is rtc_render_ex's, without progress words -- a share's rows leave, chunk by
 * chunk, when its stream is done; the halo pass and the refinement are "adaptive_seam_kernel<...;halo>" / "<...;ss=k>", ids
 * "aot_adaptive_seam<1|k>_<hash>" -- the hash folds in rtc_adaptive.h and rtc_adaptive_seam.h -- or the scene's own,
 * "adaptive_seam_kernel_spec[...]" / "spec_..." (-DRTC_SPEC_ADAPTIVE_SEAM=1|k).  Which runs: the seam's rule -- ahead-of-time at
 * a scene's first sighting unless the disk cache has its kernel, compiled from the second on; RTC_AMD_SPECIALIZE=0|1 as for
 * rtc_render_ex; depth above 8 takes the deep-stack variant.  rtc_ctx_render_adaptive's kernels are not touched.
 * Calls of rtc_render_ex, rtc_render_ss, rtc_render_lens and rtc_render_adaptive of one scene may alternate, each gives its own
 * frame; rtc_render_release frees what this call keeps.
 * Not offered: adaptive lens frames, adaptive frames in dist.py, a partitioned rtc_ctx_render_adaptive. */
typedef struct rtc_seam_adaptive_stats {
    uint64_t refined_pixels; /* flagged pixels, summed over the entries: the mask's sum                                    */
    uint64_t refine_rays;    /* rays of the refinement passes, counted as rtc_ctx_trace counts them                        */
    uint64_t halo_pixels;    /* pixels of the halo rows the entries traced beside their shares                             */
    uint64_t halo_rays;      /* ... and the rays that took                                                                 */
    float mask_ms;           /* HIP-event time of an entry's halo pass and mask kernel, the maximum over the entries       */
    float refine_ms;         /* ... and of its refinement kernel                                                           */
} rtc_seam_adaptive_stats;
rtc_status rtc_render_adaptive(const rtc_scene* scene, const rtc_camera* camera, int32_t depth, uint32_t k, float threshold,
                               const rtc_opts* opts, void* out, void* mask_u8, rtc_stats* stats,
                               rtc_seam_adaptive_stats* ad);
/* Frees everything rtc_render / rtc_render_ex / rtc_render_ss / rtc_render_lens / rtc_render_adaptive keep between calls (all devices). */
void rtc_render_release(void);
/* Page-locked host memory (hipHostMalloc): an `out` buffer allocated here is filled by DMA straight from the device. */
void* rtc_host_alloc(size_t bytes);
void rtc_host_free(void* p);

/* Persistent context: scene resident in HBM, output left on the device.
 * Ordering contract: a context serves ONE stream at a time.  rtc_ctx_render is asynchronous; launches on the same
 * stream queue up behind each other, but rendering from one context on two streams concurrently is a race on the
 * context's counters.  rtc_ctx_set_scene waits for every launch the context has issued before it replaces the scene
 * (it synchronises the device), so it may be called right after an asynchronous render. */
rtc_status rtc_ctx_create(int32_t device, rtc_ctx** out);
void rtc_ctx_destroy(rtc_ctx* ctx);
/* Flattens the scene to structure-of-arrays records and uploads it.  Called again with the scene that is resident: nothing
 * happens; with records that are resident and another camera (an animation's usual frame): nothing is uploaded; with a scene
 * of the same frame size: what the frames before measured stays the schedule's starting point. */
rtc_status rtc_ctx_set_scene(rtc_ctx* ctx, const rtc_scene* scene, const rtc_camera* camera);
/* Supersampled rendering: k x k rays per pixel of `output_camera` (W x H), reduced in the render kernel; k = 2 or 4 (k = 1 is
 * rtc_ctx_set_scene; anything else, or a fine frame rtc_camera_supersampled refuses: RTC_ERR_INVALID_ARG, decided before any
 * device call).  Afterwards rtc_ctx_render writes the W x H frame, by definition a fixed-order f32 box filter of the frame F that
 * rtc_ctx_render produces for the fine camera rtc_camera_supersampled(output_camera, k) -- jitter keys from the fine pixel
 * index y * k W + x, the reference's black last row and column at the FINE resolution (camera.rs:80-81), so the output's last
 * row and column are dimmed, not black.  Output pixel (X, Y), per channel, in f32 without fused operations:
 *   k = 2: ((F[2Y][2X] + F[2Y][2X+1]) + (F[2Y+1][2X] + F[2Y+1][2X+1])) * 0.25f
 *   k = 4: per row r = (a0 + a1) + (a2 + a3), then ((r0 + r1) + (r2 + r3)) * 0.0625f
 * Partitions count OUTPUT rows: rtc_partition{band_rows, ...} are bands of band_rows output rows, the buffer is
 * rtc_partition_rows(H, part) x W x 3 f32.  rtc_stats: rays, shaded_hits and pixels are the fine frame's, rows the output
 * rows written.  culled_shadow_rays counts the fine frame's rays too, but which shadow rays the light-cone cull answers depends
 * on which lanes share a wave: it equals a plain render of the fine camera only where both launch one lane per pixel (the
 * ahead-of-time kernels); a scene's own kernel, whose lanes per pixel are capped for k, may cull other rays -- never other
 * colours, and `rays` counts culled rays as traced either way.  rtc_ctx_kernel_name / _id name the supersampling kernel ("ss_render_kernel...";
 * "aot_ss<k>_..." or "spec_..." ids of their own).  The rules of rtc_ctx_set_scene hold: unchanged records are not uploaded,
 * a scene of the same frame size and factor keeps the schedule.  A later rtc_ctx_set_scene leaves supersampled mode.
 * rtc_ctx_render_hits on a supersampled context is RTC_ERR_UNSUPPORTED (a first hit per output pixel is not defined).
 * The one-call seam supersamples through rtc_render_ss (above): the same frame, f32 or bytes, host buffer out, several devices. */
rtc_status rtc_ctx_set_scene_ss(rtc_ctx* ctx, const rtc_scene* scene, const rtc_camera* output_camera, uint32_t k);
/* A thin-lens camera: depth of field.  rtc_ctx_set_scene_ss with the k x k samples of an output pixel leaving from k x k points of
 * `lens` (k = 2 or 4).  Afterwards rtc_ctx_render writes the W x H frame that is, by definition, rtc_ctx_set_scene_ss's box filter
 * (same order, same constants) of the fine frame F whose pixel (x, y) is World::color_at (world.rs:88-101) of the ray
 * rtc_lens_rays gives it, at the render's depth, with jitter key y * k W + x; F's last row and column are zero (camera.rs:80-81
 * at the fine resolution).  aperture_radius = 0 is allowed: every ray leaves the camera's origin towards its focus point -- a
 * supersampled pinhole whose directions are rounded differently; no bit equality with rtc_ctx_set_scene_ss's frame is promised.
 * Everything else is a supersampled context's: partitions count output rows, rtc_stats counts the fine frame, unchanged records
 * are not uploaded -- another lens or camera on the resident scene uploads nothing, so a focus pull costs three words of the next
 * launch's arguments.  The kernel is one of its own (rtc_ctx_kernel_name "lens_render_kernel<...;ss=k>" /
 * "lens_render_kernel_spec[...;ss=k;lens]", ids "aot_lens<k>_<hash>" / "spec_..."); the scene-box early-out of the pinhole kernels,
 * argued for rays from the camera's origin, is off.  A later rtc_ctx_set_scene or rtc_ctx_set_scene_ss leaves lens mode.
 * On a lens context rtc_ctx_render_hits and rtc_ctx_render_adaptive are RTC_ERR_UNSUPPORTED; rtc_ctx_trace, rtc_ctx_trace_hits,
 * rtc_ctx_is_shadowed and rtc_ctx_camera_rays are what they are on any context.
 * RTC_ERR_INVALID_ARG with a message, decided on the host before any device call and before the context is looked at: a null lens
 * or camera, k not 2 or 4, aperture_radius negative or not finite, focal_distance <= 0 or not finite, a fine frame
 * rtc_camera_supersampled refuses.  The one-call seam renders through a lens with rtc_render_lens (above): the same frame, f32 or
 * bytes, host buffer out, several devices.  Not offered: adaptive lens frames, lens frames in dist.py.  (Nor, DESIGN.md
 * 8e: adaptive frames in dist.py, a partitioned rtc_ctx_render_adaptive -- adaptive frames over several devices are rtc_render_adaptive's.) */
rtc_status rtc_ctx_set_scene_lens(rtc_ctx* ctx, const rtc_scene* scene, const rtc_camera* output_camera, uint32_t k,
                                  const rtc_lens* lens);
/* Rows this partition produces (sum of its bands' heights). */
uint32_t rtc_partition_rows(uint32_t height, const rtc_partition* part);
/* Launches the render kernel on `stream` (a hipStream_t; NULL = default
 * stream) and returns without synchronising.  d_out_rgb: DEVICE pointer to
 * rtc_partition_rows()*width*3 f32.  part may be NULL (whole image).
 * "Returns without synchronising" has one exception per scene, partition and depth: the context schedules a frame by what
 * the frame before it measured (which blocks of pixels start first, how many lanes trace a pixel of each),
 * and the second -- for block lists also the third -- call reads those measurements back, which waits for the device.
 * Every frame traces every ray and returns the same values.  RTC_AMD_BLOCK_FEEDBACK=0: every frame like the first. */
rtc_status rtc_ctx_render(rtc_ctx* ctx, int32_t depth, const rtc_partition* part, void* d_out_rgb, void* stream);
/* Waits for every rtc_ctx_render issued on this context so far and reports the
 * last launch's counters plus the mean kernel time since the previous call. */
rtc_status rtc_ctx_stats(rtc_ctx* ctx, rtc_stats* out);
/* Name of the kernel rtc_ctx_render launches for the current scene: an ahead-of-time instantiation
 * ("render_kernel<4,simple>") or a scene-specialised one compiled at rtc_ctx_set_scene
 * ("render_kernel_spec[...]"; env RTC_AMD_SPECIALIZE=0|1 overrides the size-based default). */
const char* rtc_ctx_kernel_name(rtc_ctx* ctx);
/* "" when the current scene's kernel is what the specialisation policy asked for; otherwise why it is not (the hiprtc
 * failure), in which case rtc_stats.flags carries RTC_STATS_JIT_FALLBACK and a warning went to stderr once (silence:
 * RTC_AMD_QUIET=1).  The kernel source is embedded in the library: no file beside librtc_amd.so is read at run time.
 * Compiled kernels are cached in <library dir>/jit_cache, or RTC_AMD_JIT_CACHE=<dir> (0: memory only). */
const char* rtc_ctx_jit_status(rtc_ctx* ctx);
/* Names the CODE the current scene is rendered with -- "spec_<hash of kernel source, compile options and compiler
 * version>.<checksum of the compiled code object>" or "aot_<hash of the kernel source>" -- so that a measurement taken of one kernel (the profiles/ *_pmc.json summaries)
 * is never quoted for another: bench.py prints instruction counts and HBM traffic only from a summary whose id matches. */
const char* rtc_ctx_kernel_id(rtc_ctx* ctx);
/* canvas.rs:39-43 scale_color on the device: n f32 channel values -> n bytes
 * ((c*255).min(255).max(0) as u8).  Both pointers are device pointers. */
rtc_status rtc_ctx_quantize(rtc_ctx* ctx, const void* d_rgb, uint64_t n, void* d_out_u8, void* stream);

/* Canvas::to_ppm (canvas.rs:58-96) on the device: formats an f32 image that is already in HBM
 * (d_rgb: height*width*3 f32) as P3 text into d_text (DEVICE buffer of at least
 * rtc_ppm_max_bytes(width, height) bytes), byte-for-byte what the reference builds, including the
 * 70-column wrapping.  Synchronises `stream`; *out_len = bytes written. */
uint64_t rtc_ppm_max_bytes(uint32_t width, uint32_t height);
rtc_status rtc_ctx_to_ppm(rtc_ctx* ctx, const void* d_rgb, uint32_t width, uint32_t height, void* d_text,
                          uint64_t capacity, uint64_t* out_len, void* stream);

/* Batched World::color_at (world.rs:88-101) for caller-supplied rays; ray i
 * uses pixel index i as its jitter key.  Host buffers: origins/directions
 * n*4 f32, out n*3 f32. */
rtc_status rtc_color_at(const rtc_scene* scene, const float* origins, const float* directions, uint32_t n,
                        int32_t depth, int32_t device, float* out_rgb);
/* ------------------------------------------------------------------------
 * First-hit buffers: what the path knows about a ray's first hit before it becomes a colour.
 * "First hit" is, in this order: xs = World::intersect(ray) (world.rs:52-60); hit = Intersection::hit(xs)
 * (intersection.rs:30-35: the first minimum among distance >= 0, -0.0 counts, ties by list order);
 * comps = precompute_values(ray, hit, xs) (world.rs:212-283) for EVERY hit, opaque or not; and
 * light = world.light.intensity_at(comps.over_point, world), the number shade_hit hands to phong_lighting for that hit
 * (world.rs:75), drawn with the jitter key (pixel index, path 1) -- the key a render gives a pixel's primary hit.
 *
 * One plane per field of PrecomputedValues (world.rs:165-182) plus the light fraction; NULL = not wanted.  A miss stores
 * object = -1 and zeros in every other requested plane; every requested plane is written in full; a plane that is not
 * requested is not touched.  Vector planes are 4 f32 per element with w as the reference's Tuple has it (1 for points, 0 for
 * vectors).  `light` with an RTC_JITTER_SEQUENCE light is refused (the cycle is state, see the enum); without the light
 * plane such a scene is accepted -- no draw is made.
 * ---------------------------------------------------------------------- */
typedef struct rtc_hit_planes {
    int32_t* object;      /* index into rtc_scene.objects; -1: no hit                       */
    float*   distance;    /* Intersection.distance                                           */
    float*   point;       /* 4 f32 each                                                      */
    float*   eye;
    float*   normal;      /* after the inside flip (world.rs:223-226)                        */
    float*   reflectv;    /* from the normal BEFORE the flip (world.rs:220)                  */
    float*   over_point;
    float*   under_point;
    int32_t* inside;      /* 0 / 1                                                           */
    float*   n1n2;        /* 2 f32: n1, n2 (world.rs:234-263)                                */
    float*   light;       /* intensity_at(over_point), 0..1                                  */
} rtc_hit_planes;

/* Batched first hits for caller-supplied rays, like rtc_color_at: host buffers, origins / directions n*4 f32 (origin.w
 * 1, direction.w 0), every plane of `out` n elements; ray i uses pixel index i as its jitter key.  No plane requested, or
 * a null ray pointer with n > 0: RTC_ERR_INVALID_ARG (decided before any device call). */
rtc_status rtc_hit_at(const rtc_scene* scene, const float* origins, const float* directions, uint32_t n,
                      int32_t device, const rtc_hit_planes* out);
/* The first hits of the camera's pixels from a persistent context: the planes are DEVICE pointers, the launch is
 * asynchronous on `stream`, the partition rules and the compact row layout are rtc_ctx_render's -- plane element (yl, x)
 * at index yl*width + x, rtc_partition_rows() rows.  The last row and the last column of a frame (never traced,
 * camera.rs:80-81) are stored as misses.  Rendered by ahead-of-time kernels of the families rtc_ctx_render's ahead-of-time
 * branch chooses from.  Leaves rtc_ctx_stats, the frame schedule's measurements and the scene's compiled render kernel
 * alone: a render after it is scheduled and reported exactly as if this call had not happened.
 * A null context, no plane requested: RTC_ERR_INVALID_ARG (decided before any device call). */
rtc_status rtc_ctx_render_hits(rtc_ctx* ctx, const rtc_partition* part, const rtc_hit_planes* d_out, void* stream);

/* ------------------------------------------------------------------------
 * Ray streams: the caller's rays against the context's resident scene, on the device.
 * ---------------------------------------------------------------------- */
/* World::color_at (world.rs:88-101) for n caller rays against the context's resident scene.  DEVICE pointers:
 * d_origins, d_directions n x 4 f32 (16-byte aligned; x, y, z are read, w is ignored: a ray is a point and a vector
 * by position); d_keys n x u32 or NULL -- ray i draws its light samples as pixel d_keys[i] (NULL: i), the key a render
 * gives pixel y*W+x; d_out_rgb n x 3 f32.  Asynchronous on `stream`.  depth 0 .. RTC_MAX_DEPTH as rtc_ctx_render.
 * The direction is used as given (the reference's color_at does not normalise it either).  Rays with non-finite
 * components are the caller's error: their colour is unspecified.
 * Origins may lie anywhere: no shortcut of the scene's preparation is argued from where the context's camera stands without
 * a guard that each ray carries itself -- a ray that starts beyond the reach of the library's own hierarchy over a flat world
 * (more than 100 of the world's smallest half-axis across, or a coordinate beyond 2 500 of it) is traced against every object
 * in turn, as are the rays of its wave.  The same holds for rtc_ctx_trace_reordered, rtc_ctx_trace_hits and both ends of an
 * rtc_ctx_is_shadowed pair.
 * One lane per ray, ray i in thread i: a wave is 64 consecutive rays, and rays that are neighbours in space trace fastest
 * as neighbours in the buffers.  The kernel is the context's ahead-of-time family or, where rtc_ctx_set_scene's
 * specialisation policy -- with n in the place of the frame's pixel count; RTC_AMD_SPECIALIZE=0|1 as there -- asks for
 * it, the scene's own, compiled by the first trace that wants it (a context that never traces pays nothing) and cached
 * like every scene kernel; depth above 8 takes the deep-stack variant, as for rtc_ctx_render.  A supersampled context
 * traces like any other.
 * RTC_ERR_INVALID_ARG, decided before any device call: a null context, no scene set, a null ray or output pointer with
 * n > 0, origins / directions not 16-byte aligned, keys / output not 4-byte aligned, depth out of range.  n == 0: RTC_OK,
 * nothing is launched.
 * rtc_ctx_stats after a trace reports that launch: rays, shaded_hits and culled_shadow_rays as a render counts them,
 * pixels = n, rows = 0, kernel_ms and launches over the traces since the last such report.  Everything else a trace leaves
 * alone -- block lists, measured wave times, grid feedback, the render kernels' warm-up, rtc_ctx_kernel_name / _id: a
 * render after a trace is scheduled and reported as if the trace had not happened.  (rtc_ctx_render_hits, which leaves
 * rtc_ctx_stats alone, leaves it alone here too: after trace, render_hits, the stats are still the trace's.)
 * One stream at a time, as for the whole context: the trace's counter partials and totals exist once per context, so two traces
 * in flight on different streams compute the right colours and race on what rtc_ctx_stats reports.
 * The argument checks come in this order, the context's last, so that each is reported by name whatever else is wrong:
 * ray and output pointers, alignment, depth, context, scene. */
rtc_status rtc_ctx_trace(rtc_ctx* ctx, int32_t depth, const void* d_origins, const void* d_directions,
                         const void* d_keys, uint32_t n, void* d_out_rgb, void* stream);
/* ray_for_pixel (camera.rs:60-74) of `camera` for image rows [y0, y0 + n_rows), every column, in image order, written
 * to DEVICE buffers in rtc_ctx_trace's layout (origin.w 1, direction.w 0, key y*W+x); any of the three may be NULL.
 * The camera is an argument, not the context's, and no scene need be set.  The rays are the render kernels' own (one device
 * function makes both), the last row and column included, which a render never traces (camera.rs:80-81).
 * RTC_ERR_INVALID_ARG, decided before any device call: a null camera or context, misaligned pointers as for rtc_ctx_trace,
 * y0 + n_rows > height, more than 2^32 - 1 rays.  A camera whose inverse transform is not affine: RTC_ERR_UNSUPPORTED, as
 * rtc_ctx_set_scene answers it.  n_rows == 0: RTC_OK, nothing is launched. */
rtc_status rtc_ctx_camera_rays(rtc_ctx* ctx, const rtc_camera* camera, uint32_t y0, uint32_t n_rows,
                               void* d_origins, void* d_directions, void* d_keys, void* stream);
/* The kernel of the context's last rtc_ctx_trace and the code it names ("trace_kernel<...>" / "trace_kernel_spec[...]";
 * "aot_trace_..." or "spec_..." ids of their own, as rtc_ctx_kernel_name / _id).  "" before the first trace of the current scene. */
const char* rtc_ctx_trace_kernel_name(rtc_ctx* ctx);
const char* rtc_ctx_trace_kernel_id(rtc_ctx* ctx);
/* ------------------------------------------------------------------------
 * Ray reordering: an incoherent stream sorted on the device, traced in sorted order, answered in the caller's.
 * rtc_ctx_trace gives ray i to thread i, and a wave's time is that of its 64 rays together: a stream in random order costs
 * several times a coherent one.  Every colour is exact whatever a ray's neighbours are, so the library may reorder.
 *
 * The coherence key of a ray: a 32-bit unsigned integer, a function of the stream alone (neither scene nor camera), computed
 * with f32 + - * /, compares and float-to-int conversions only, nothing fused, no library function: the same bits on the host.
 *  Stream box: per axis a, lo[a] and hi[a] are the minimum and maximum over the rays' origin components that are finite
 *   (|x| <= FLT_MAX; +inf and -inf where there is none).  Signed zeros are equivalent below.
 *  Origin cell of a component x with its axis' lo, hi: 0 if x is not finite or not hi > lo (a camera's rays all leave one
 *   point); else t = (x - lo) * (16.0f / (hi - lo)) and the cell is 15 if t >= 16.0f, (int)t if t > 0.0f, else 0 (a NaN t: 0).
 *   The three 4-bit cells are interleaved to 12 bits, x lowest: bit k of cell x, y, z is bit 3k, 3k + 1, 3k + 2.
 *  Direction cell, the octahedral map on a 1024 x 1024 grid: |a| is a < 0.0f ? -a : a, sign(a) is a >= 0.0f ? 1.0f : -1.0f;
 *   s = (|dx| + |dy|) + |dz|; if not s > 0.0f or s is not finite, u = v = 0; else px = dx / s, py = dy / s, and where
 *   dz < 0.0f the fold (px, py) <- ((1.0f - |py|) * sign(px), (1.0f - |px|) * sign(py)), both from the unfolded values;
 *   u = cell((px * 0.5f + 0.5f) * 1024.0f), v likewise from py, cell(t) = 1023 if t >= 1024.0f, (int)t if t > 0.0f, else 0.
 *   u and v are interleaved to 20 bits, u lowest: bit k of u, v is bit 2k, 2k + 1.
 *  key = origin << 20 | direction: bits [31:20] the origin, bits [19:0] the direction.
 * The order of a stream: order[j] is the index of the ray that comes j-th by key, ties by index -- a stable sort, the same
 * permutation on every run (a least-significant-digit radix sort on the device, no float arithmetic, no atomics on positions). */
/* The order of n caller rays.  DEVICE pointers: d_origins, d_directions as rtc_ctx_trace takes them; d_order_u32 n x u32.
 * Needs a context (its device, its scratch memory) but no scene.  Asynchronous on `stream`; nothing is read by the host.
 * RTC_ERR_INVALID_ARG, decided before any device call, in this order: a null ray or output pointer with n > 0; origins /
 * directions not 16-byte aligned, the output not 4-byte aligned; a null context.  n == 0 with the pointer checks passed:
 * RTC_OK, nothing is launched (the context is not looked at).  Scratch memory that cannot be had: RTC_ERR_DEVICE, the context
 * stays usable. */
rtc_status rtc_ctx_ray_order(rtc_ctx* ctx, const void* d_origins, const void* d_directions, uint32_t n, void* d_order_u32,
                             void* stream);
/* rtc_ctx_trace with the stream sorted first: its arguments, its checks in its order, and the same bits in d_out_rgb, element i
 * belonging to the caller's ray i.  The rays are ordered (as rtc_ctx_ray_order), gathered into the context's own buffers with
 * their keys -- d_keys[i], or i where d_keys is NULL: a ray draws its light samples as in the caller's order -- traced there by
 * rtc_ctx_trace's launch, and the colours stored back at out[order[j]].
 * Afterwards the context is as after rtc_ctx_trace of the same stream: rtc_ctx_stats reports the trace (rays and shaded_hits
 * equal the plain trace's; culled_shadow_rays is voted by whichever lanes share a wave, so it is not comparable), and
 * rtc_ctx_trace_kernel_name / _id are those the plain trace of the same n would report.  Everything a trace leaves alone
 * stays alone.  The scratch memory -- 52 bytes a ray: 16 for the sort's two (key, index) buffers, 12 of which later hold the
 * colours, 36 for the gathered rays and keys -- is allocated by the first call that needs it, grows on demand (which waits for
 * the device) and is released by rtc_ctx_destroy; if it cannot be had: RTC_ERR_DEVICE, the context stays usable.
 * One stream at a time, as for the whole context.  Off by default for a reason: a stream that is coherent already pays the
 * sort for nothing (DESIGN.md 8f says where the crossover lies). */
rtc_status rtc_ctx_trace_reordered(rtc_ctx* ctx, int32_t depth, const void* d_origins, const void* d_directions,
                                   const void* d_keys, uint32_t n, void* d_out_rgb, void* stream);
typedef struct rtc_reorder_stats {
    uint64_t n;        /* rays of the last rtc_ctx_trace_reordered                                                        */
    float keys_ms;     /* HIP-event time of the stream box and the keys                                                   */
    float sort_ms;     /* ... of the sort's four passes                                                                   */
    float gather_ms;   /* ... of the gather into sorted order                                                             */
    float trace_ms;    /* ... of the trace: the kernel rtc_ctx_stats times, its counter sum and any first-launch warm-up  */
    float scatter_ms;  /* ... of the colours' way back                                                                    */
} rtc_reorder_stats;
/* Waits for the device as rtc_ctx_stats does; all zero before the first rtc_ctx_trace_reordered. */
rtc_status rtc_ctx_reorder_stats(rtc_ctx* ctx, rtc_reorder_stats* out);
/* ------------------------------------------------------------------------
 * Adaptive supersampling: k x k rays only where neighbouring pixels of the rendered frame differ.
 * For the context's resident scene and camera (W x H), k = 2 or 4 and an f32 threshold:
 *  (1) B is exactly what rtc_ctx_render writes for the whole frame at `depth`, its black last row and column included.
 *  (2) Pixel p is flagged when, for any of its up to four neighbours n (x +- 1, y +- 1, inside the frame) and any channel c,
 *      fabsf(B[p][c] - B[n][c]) > threshold: f32 subtraction and fabsf, a strict compare, so a NaN difference (inf - inf) never
 *      flags; the rule is symmetric, both pixels of a contrasting pair are flagged; the last row and column take part like
 *      any pixel (their neighbours are flagged wherever the scene is lit there).
 *  (3) S is rtc_ctx_set_scene_ss's frame for the same camera and k: the fine camera rtc_camera_supersampled(camera, k), jitter
 *      keys from the fine pixel index y_f * k W + x_f, the fine frame's last row and column black, the pairwise f32 tree along
 *      x first, then along y, times 0.25f or 0.0625f, nothing fused (see rtc_ctx_set_scene_ss).
 *  (4) The output O[p] = S[p] where p is flagged, B[p] elsewhere; S is never computed where p is not flagged.  With a
 *      threshold so large that nothing is flagged O is rtc_ctx_render's frame bit for bit.  The picture does not depend on
 *      the order in which flagged pixels are processed.
 * d_out_rgb: DEVICE pointer to H x W x 3 f32.  d_mask_u8: DEVICE pointer to H x W bytes, 1 = refined, 0 = not; may be NULL.
 * The whole frame only: the mask needs neighbours across band edges, so there is no partition; the f32 canvas only (bands over
 * several devices, bytes and host output: rtc_render_adaptive above, whose entries trace the rows across their band edges themselves).
 * Asynchronous on `stream`; nothing comes back to the host between the three passes, the number of flagged pixels included.
 * The base pass IS rtc_ctx_render -- tiles, rectangle, block lists, feedback and its occasional read-back of measurements --
 * so rtc_ctx_stats and rtc_ctx_kernel_name / _id afterwards report it as after rtc_ctx_render, and the schedule moves as a
 * render moves it.  The refinement leaves all of that alone, as a trace does, and the trace's own state as well.  Its kernel
 * is one lane per fine sample, the ahead-of-time family or -- where rtc_ctx_set_scene's specialisation policy asks for it
 * for a frame of W x H pixels; RTC_AMD_SPECIALIZE=0|1 as there -- the scene's own, compiled by the first adaptive call that
 * wants it and cached like every scene kernel; depth above 8 takes the deep-stack variant.
 * Rejected, decided before any device call, in this order, the context's checks last: a threshold that is not finite or is
 * negative, a k other than 2 or 4, a null or misaligned output pointer, a depth out of range, a null context, no scene set
 * (all RTC_ERR_INVALID_ARG); a supersampled context (RTC_ERR_UNSUPPORTED); a fine frame beyond rtc_camera_supersampled's
 * limits, 2^32 pixels or 2^17 rows (RTC_ERR_INVALID_ARG).
 * One stream at a time, as for the whole context. */
typedef struct rtc_adaptive_stats {
    uint64_t refined_pixels;     /* flagged pixels of the last rtc_ctx_render_adaptive                                  */
    uint64_t rays;               /* of the refinement pass, counted as rtc_ctx_trace counts them                        */
    uint64_t shaded_hits;
    uint64_t culled_shadow_rays; /* voted by whichever lanes share a wave: <= rays, otherwise not comparable            */
    float mask_ms;               /* HIP-event time of the mask and list kernel                                          */
    float refine_ms;             /* ... and of the refinement kernel                                                    */
} rtc_adaptive_stats;
rtc_status rtc_ctx_render_adaptive(rtc_ctx* ctx, int32_t depth, uint32_t k, float threshold, void* d_out_rgb,
                                   void* d_mask_u8, void* stream);
/* Waits for the device as rtc_ctx_stats does; all zero before the first rtc_ctx_render_adaptive. */
rtc_status rtc_ctx_adaptive_stats(rtc_ctx* ctx, rtc_adaptive_stats* out);
/* The refinement kernel of the context's last rtc_ctx_render_adaptive and the code it names
 * ("adaptive_refine_kernel<...;ss=k>" / "adaptive_refine_kernel_spec[...;ss=k]"; "aot_adaptive<k>_..." or "spec_..." ids),
 * as rtc_ctx_trace_kernel_name / _id.  "" before the first adaptive call of the current scene. */
const char* rtc_ctx_adaptive_kernel_name(rtc_ctx* ctx);
const char* rtc_ctx_adaptive_kernel_id(rtc_ctx* ctx);

/* The first hits (see "First-hit buffers" above) of n caller rays against the context's resident scene: the rays and keys
 * are rtc_ctx_trace's (DEVICE pointers, x, y, z read, the direction used as given, d_keys NULL: ray i draws as pixel i), the
 * planes are rtc_ctx_render_hits' (`d_out` a host struct of DEVICE pointers, NULL = not wanted), element i belonging to ray
 * i.  A miss stores object = -1 and zeros; every requested plane is written for all n elements and nothing behind them; a
 * plane that is not requested is not touched; w as rtc_ctx_render_hits writes it; `light` is drawn as pixel d_keys[i], path
 * 1 -- the key a render gives that pixel's primary hit.  Asynchronous on `stream`.
 * One lane per ray, ray i in thread i, ahead-of-time kernels of rtc_ctx_render_hits' families; every shortcut that acts
 * inside the scene's intersection and light code applies as in a render.  A supersampled context answers like any other:
 * the camera is not read.
 * Like rtc_ctx_render_hits it leaves rtc_ctx_stats, the trace's counters, block lists, measured wave times, warm-up
 * bookkeeping and rtc_ctx_kernel_name / _id / rtc_ctx_trace_kernel_name / _id alone: a render or a trace after it is
 * scheduled and reported as if this call had not happened.
 * RTC_ERR_INVALID_ARG, decided before any device call, in this order, so that each is reported by name whatever else is
 * wrong: a null ray pointer or a null `d_out` with n > 0; no plane requested; alignment -- origins, directions and the
 * vector planes 16 bytes, n1n2 8, keys and the scalar planes 4; a null context; no scene set.  n == 0 with these pointer
 * checks passed: RTC_OK, nothing is launched (the context is not looked at). */
rtc_status rtc_ctx_trace_hits(rtc_ctx* ctx, const void* d_origins, const void* d_directions, const void* d_keys,
                              uint32_t n, const rtc_hit_planes* d_out, void* stream);
/* World::is_shadowed(light_position, point) (world.rs:104-119) for n pairs against the context's resident scene: is the
 * nearest thing between the two a shadow caster?  Not only for lights: mutual visibility of two points, ambient occlusion.
 * DEVICE pointers: d_light_positions, d_points n x 4 f32 (16-byte aligned; x, y, z are read); d_out_i32 n x int32, 0 / 1 as
 * rtc_is_shadowed writes it.  Asynchronous on `stream`; leaves the context alone as rtc_ctx_trace_hits does.
 * RTC_ERR_INVALID_ARG, decided before any device call, in this order: a null pair or output pointer with n > 0; alignment
 * (16 bytes for the pairs, 4 for the output); a null context; no scene set.  n == 0 as for rtc_ctx_trace_hits. */
rtc_status rtc_ctx_is_shadowed(rtc_ctx* ctx, const void* d_light_positions, const void* d_points, uint32_t n,
                               void* d_out_i32, void* stream);

/* Batched Light::intensity_at (light.rs:10) for n world points (n*4 f32). */
rtc_status rtc_intensity_at(const rtc_scene* scene, const float* points, uint32_t n, int32_t device,
                            float* out);
/* Batched RectangleLight::point_on_light (rectangle_light.rs:60-66) on the device: n (u, v) cell pairs (n*2 int32), each
 * answered as by a freshly built light (a sequence jitter's first two values; a hashed one's cell key with pixel 0, path
 * 1); out n*4 f32 points. */
rtc_status rtc_point_on_light(const rtc_light* light, const int32_t* cells_uv, uint32_t n, int32_t device, float* out);
/* Batched World::is_shadowed (world.rs:104-119): light_positions, points n*4 f32; out n int32 (0/1). */
rtc_status rtc_is_shadowed(const rtc_scene* scene, const float* light_positions, const float* points, uint32_t n,
                           int32_t device, int32_t* out);
/* Batched Shape::local_intersect (shape.rs:50, e.g. cone.rs:52-57) on the device: n object-space rays
 * (n*4 f32 each) against `object`'s kind/bounds; out_t receives up to 4 distances per ray in push
 * order (n*4 f32), out_count the number pushed (n int32). */
rtc_status rtc_local_intersect(const rtc_object* object, const float* origins, const float* directions, uint32_t n,
                               int32_t device, float* out_t, int32_t* out_count);
/* Batched Shape::normal_at (shape.rs:72-154: object space, local_norm_at, back to world, normalise)
 * for n world points (n*4 f32); out n*4 f32 vectors. */
rtc_status rtc_normal_at(const rtc_object* object, const float* world_points, uint32_t n, int32_t device,
                         float* out);
/* Batched Pattern::color_at_object (pattern.rs:15-19) for n world points (n*4 f32) on `object`
 * (NULL: an untransformed shape); out n*3 f32. */
rtc_status rtc_pattern_color_at(const rtc_pattern* pattern, const rtc_object* object, const float* world_points,
                                uint32_t n, int32_t device, float* out_rgb);
/* f32::powf / f32::cos as the reference's Linux build computes them (phong_lighting.rs:56,
 * pattern/sine_2d.rs:40), evaluated on the device; host buffers of n f32. */
rtc_status rtc_powf(const float* x, const float* y, uint32_t n, int32_t device, float* out);
rtc_status rtc_cosf(const float* x, uint32_t n, int32_t device, float* out);
/* f32::atan2 / f32::acos (pattern/uv.rs:108,101) likewise */
rtc_status rtc_atan2f(const float* y, const float* x, uint32_t n, int32_t device, float* out);
rtc_status rtc_acosf(const float* x, uint32_t n, int32_t device, float* out);

/* Canvas::to_ppm (canvas.rs:58-96) on an f32 image already on the host:
 * returns a malloc'd buffer (free with rtc_free) holding the P3 text. */
rtc_status rtc_to_ppm(const float* rgb, uint32_t width, uint32_t height, char** out_text, uint64_t* out_len);
void rtc_free(void* p);

/* Thread-local text of the last error returned on this thread. */
const char* rtc_last_error(void);
int32_t rtc_abi_version(void);
/* Number of usable gfx950 devices (0 if none / no HIP runtime). */
int32_t rtc_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* RTC_H */
