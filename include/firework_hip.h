/*
 * firework_hip.h — C ABI of the MI355X-native path-tracing core.
 *
 * This is the drop-in boundary for ONE path of ritobanrc/firework: the
 * `Renderer::render(&self, scene: Scene) -> Vec<Color>` call
 * (reference src/render.rs:109-161) and the data it consumes
 * (`Scene`, `RenderObject`, shapes, materials, textures, environments,
 * `CameraSettings`).  Everything is plain C: fixed-width scalars, plain
 * pointers and sizes.  No torch / C++ / HIP types appear in a signature.
 *
 * The reference keeps its scene as open sets of trait objects
 * (`Box<dyn SerializableShape>`, `Box<dyn Material>`, `Box<dyn Texture>`,
 * `Box<dyn Environment>`; src/scene.rs:19-24,270-277).  A GPU cannot call a
 * user's trait impl, so the ABI carries CLOSED tagged unions whose tags are
 * exactly the reference's typetag names (src/serde_compat.rs:22,
 * src/material.rs:9, src/texture.rs:7, src/environment.rs:5).
 *
 * Ownership: the caller owns every buffer it passes in or receives results
 * in; the library copies what it needs during the call.  No call throws or
 * aborts across this boundary: errors are negative `fw_status` codes
 * (the reference panics instead: src/bvh.rs:34, src/scene.rs:161).
 *
 * The SAME structs are the input format of the CPU oracle under oracle/
 * (test infrastructure, not part of the product).
 */
#ifndef FIREWORK_HIP_H
#define FIREWORK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FW_ABI_VERSION 8   /* 8: + fw_trace_rays, fw_camera_rays (ray queries; fw_hit, fw_trace_params); 7: + fw_init (loading the library no longer touches the GPU); options EXACT_PRODUCT, PHASE_LOCK, GRAPH; 6: + fw_set_option (the runtime switches leave the environment: read once at load), fw_selftest_wide_bvh; 3: + fw_render_progressive; 4: fw_stats carries this layout's own HBM bytes per kernel class and the one-shot timings;
                              5: + fw_selftest_libm; the 4th float of an accumulation record counts the path segments of the samples that deposited */

/* ---- status codes ------------------------------------------------------ */
typedef enum fw_status {
    FW_OK = 0,
    FW_ERR_BAD_ARG = -1,       /* null pointer, zero size, index out of range      */
    FW_ERR_EMPTY_SCENE = -2,   /* reference: panic "No render objects added to scene!" (src/scene.rs:161)
                                  and unbounded recursion on an empty BVH (src/bvh.rs:29-70)          */
    FW_ERR_NAN_BBOX = -3,      /* reference: panic "Float comparison failed in BVH constructor" (src/bvh.rs:34) */
    FW_ERR_MESH_NORMALS = -4,  /* "TriangleMesh::new() -- normals.len() must equal verts.len()" (src/objects/mesh.rs:46) */
    FW_ERR_MESH_UVS = -5,      /* "TriangleMesh::new() -- uvs.len() must equal verts.len()"     (src/objects/mesh.rs:51) */
    FW_ERR_UNSUPPORTED = -6,   /* valid scene, but a feature the GPU path does not implement yet */
    FW_ERR_HIP = -7,           /* a HIP runtime call failed; see fw_last_error()                  */
    FW_ERR_NO_DEVICE = -8,     /* no gfx950 device visible: the product path never falls back to CPU */
    FW_ERR_BVH_DEPTH = -9,     /* tree deeper than the LDS traversal stack                        */
    FW_ERR_OOM = -10
} fw_status;

/* ---- small value types ------------------------------------------------- */
typedef struct fw_vec3 { float x, y, z; } fw_vec3;

/* ultraviolet::Rotor3 as serialised by src/serde_compat.rs:6-20: {s, bv:{xy,xz,yz}} */
typedef struct fw_rotor3 { float s, xy, xz, yz; } fw_rotor3;

/* ---- textures: src/texture.rs ------------------------------------------ */
typedef enum fw_texture_kind {
    FW_TEX_CONSTANT = 0,    /* ConstantTexture   texture.rs:16-34  */
    FW_TEX_CHECKER = 1,     /* CheckerTexture    texture.rs:36-73  */
    FW_TEX_PERLIN = 2,      /* PerlinNoiseTexture texture.rs:75-168 */
    FW_TEX_TURBULENCE = 3,  /* TurbulenceTexture texture.rs:195-225 */
    FW_TEX_MARBLE = 4,      /* MarbleTexture     texture.rs:227-249 */
    FW_TEX_IMAGE = 5        /* ImageTexture      texture.rs:270-310 */
} fw_texture_kind;

typedef struct fw_texture {
    int32_t kind;
    fw_vec3 color;           /* Constant */
    float scale;             /* Checker / Perlin / Turbulence / Marble */
    uint32_t depth;          /* Turbulence / Marble */
    int32_t odd, even;       /* Checker: indices into fw_scene_desc.textures */
    uint32_t img_w, img_h;   /* Image: RGB8, row 0 = top, tightly packed */
    const uint8_t *img_rgb8;
} fw_texture;

/* ---- materials: src/material.rs ---------------------------------------- */
typedef enum fw_material_kind {
    FW_MAT_LAMBERTIAN = 0,  /* material.rs:25-75   {albedo: texture}   */
    FW_MAT_METAL = 1,       /* material.rs:77-107  {albedo, roughness} */
    FW_MAT_DIELECTRIC = 2,  /* material.rs:109-151 {ref_idx}           */
    FW_MAT_EMISSIVE = 3,    /* material.rs:153-181 {albedo: texture}   */
    FW_MAT_ISOTROPIC = 4,   /* material.rs:183-204 {texture}           */
    FW_MAT_GGX = 5          /* not in the reference: {albedo, roughness}, specified below */
} fw_material_kind;

/* FW_MAT_GGX: an isotropic GGX microfacet conductor, two-sided.  albedo = the normal-incidence reflectance F0, every
   component in [0, 1]; roughness in [0.03, 1]; alpha = roughness^2 (float32).  Anything else: FW_ERR_BAD_ARG naming the material's index.
   Unlike Metal's lobe this one has a density, so its vertices take light samples: the point, spot and directional lights, and under
   FW_FLAG_LIGHT_SAMPLING the sphere and rectangle emitters.
     Frame: wo = -normalized(ray direction); n = the hit normal, negated where wo.n < 0; the tangent frame around n is the branchless basis
       of Duff et al. 2017: s = copysignf(1, n.z), a = -1 / (s + n.z), b = n.x n.y a, t = (1 + s n.x^2 a, s b, -s n.x), u = (b, s + n.y^2 a, -n.y).
     Sampling: (xi1, xi2) = the x and y words of draw(key, purpose 6, segment, 0).  A visible normal h by Heitz 2018: stretch wo by alpha,
       sample the projected disk (r = sqrt(xi1), phi = 2 pi xi2), unstretch; no rejection.  wi = reflect(-wo, h).  The path ends where
       wi.n <= 0; otherwise its attenuation is F(wo.h) G2(wo, wi) / G1(wo), with Schlick's F = F0 + (1 - F0)(1 - wo.h)^5,
       Lambda(w) = (-1 + sqrt(1 + alpha^2 tan^2(theta_w))) / 2, G1 = 1 / (1 + Lambda), G2 = 1 / (1 + Lambda(wo) + Lambda(wi)).
     Evaluation (light samples): f cos(theta_i) = F D(h) G2 / (4 wo.n) with h = normalized(wo + wi), density p_b(wi) = G1(wo) D(h) / (4 wo.n),
       D = alpha^2 / (pi (|h_t|^2 + alpha^2 h_n^2)^2) from h's tangential and normal parts.
     Light samples: a delta light contributes beta f cos L / p (weight 1); an emitter under FW_FLAG_LIGHT_SAMPLING beta f cos Le / p_l x
       p_l^2 / (p_l^2 + p_b^2), and an emitter the scattered ray then hits takes p_b^2 / (p_b^2 + p_l^2).  A vertex whose own sample ends the
       path still takes its light sample.  Under FW_FLAG_ENV_SAMPLING and FW_FLAG_ALL_EMITTERS a GgxMat vertex takes NO light sample, as a
       Metal vertex: what its path meets next keeps weight 1 (unbiased; light samples there are not built).
   Every entry point that takes a fw_scene_desc takes the material. */

typedef struct fw_material {
    int32_t kind;
    int32_t texture;   /* Lambertian / Emissive / Isotropic: index into textures */
    fw_vec3 albedo;    /* Metal; Ggx: F0 */
    float roughness;   /* Metal, Ggx */
    float ref_idx;     /* Dielectric */
} fw_material;

/* ---- shapes: src/objects/ ---------------------------------------------- */
typedef enum fw_shape_kind {
    FW_SHAPE_SPHERE = 0,          /* objects/sphere.rs:10-20  {radius, material}            */
    FW_SHAPE_XYRECT = 1,          /* objects/rect.rs:9-45     AARect<X,Y>                   */
    FW_SHAPE_XZRECT = 2,          /*                          AARect<X,Z>                   */
    FW_SHAPE_YZRECT = 3,          /*                          AARect<Y,Z>                   */
    FW_SHAPE_RECT3D = 4,          /* objects/rect3d.rs:9-86   {pos, size} + 6 derived faces */
    FW_SHAPE_TRIANGLE_MESH = 5,   /* objects/mesh.rs:12-63                                  */
    FW_SHAPE_CONSTANT_MEDIUM = 6, /* objects/volume.rs:10-54  {obj, density, material}      */
    FW_SHAPE_CONE = 7,            /* objects/cone.rs:9-25     {radius, height, material}    */
    FW_SHAPE_CYLINDER = 8,        /* objects/cylinder.rs:10-38 {radius, height, max_phi, material} */
    FW_SHAPE_DISK = 9             /* objects/disk.rs:10-37    {radius, phi_max, inner_radius, material} */
} fw_shape_kind;

typedef struct fw_shape {
    int32_t kind;
    int32_t material;          /* MaterialIdx (src/scene.rs:13) */
    float radius;              /* Sphere, Cone, Cylinder, Disk */
    float height;              /* Cone, Cylinder */
    float phi_max;             /* Cylinder.max_phi / Disk.phi_max, radians */
    float inner_radius;        /* Disk */
    /* AARect<A1,A2>: min=(a_min,b_min) max=(a_max,b_max) on axes (A1,A2), plane at k
       on the third axis (rect.rs:14-20).  XY: a=x b=y; XZ: a=x b=z; YZ: a=y b=z. */
    float a_min, a_max, b_min, b_max, k;
    int32_t flip_normal;       /* AARect.flip_normal (rect.rs:18) */
    fw_vec3 pos, size;         /* Rect3d (rect3d.rs:10-14); faces are derived as in Rect3d::new */
    /* TriangleMesh (mesh.rs:12-18): verts = 3*n_verts floats, indices = n_indices (multiple of 3),
       normals = NULL or 3*n_verts floats, uvs = NULL or 2*n_verts floats */
    const float *verts;
    uint32_t n_verts;
    const uint32_t *indices;
    uint32_t n_indices;
    const float *normals;
    const float *uvs;
    /* ConstantMedium (volume.rs:11-15): inner = index into fw_scene_desc.shapes */
    int32_t inner;
    float density;
} fw_shape;

/* RenderObject (src/scene.rs:270-277): shape + position + rotation + flip_normals */
typedef struct fw_object {
    int32_t shape;             /* index into fw_scene_desc.shapes */
    fw_vec3 position;
    fw_rotor3 rotation;
    int32_t flip_normals;
} fw_object;

/* ---- environments: src/environment.rs (+ examples/hdri_test.rs:22-82) --- */
typedef enum fw_env_kind {
    FW_ENV_COLOR = 0,  /* ColorEnv environment.rs:10-26 (Scene::new default: black, scene.rs:36) */
    FW_ENV_SKY = 1,    /* SkyEnv   environment.rs:28-67                                          */
    FW_ENV_HDR = 2     /* HdrEnvironment: user-side plugin in examples/hdri_test.rs:22-82, promoted
                          to a built-in because a user trait impl cannot cross to the GPU        */
} fw_env_kind;

typedef struct fw_environment {
    int32_t kind;
    fw_vec3 color;             /* ColorEnv */
    fw_vec3 zenith, horizon;   /* SkyEnv   */
    uint32_t hdr_w, hdr_h;     /* HdrEnv: equirect, f32 RGB, row 0 = top */
    const float *hdr_rgb;
} fw_environment;

/* Scene (src/scene.rs:19-24) */
typedef struct fw_scene_desc {
    const fw_object *objects;
    uint32_t n_objects;
    const fw_shape *shapes;
    uint32_t n_shapes;
    const fw_material *materials;
    uint32_t n_materials;
    const fw_texture *textures;
    uint32_t n_textures;
    fw_environment environment;
} fw_scene_desc;

/* CameraSettings (src/camera.rs:18-36); defaults there: (0,0,-10) -> 0, vfov 30, aperture 0, focus 10 */
typedef struct fw_camera_settings {
    fw_vec3 cam_pos, look_at;
    float vfov, aperture, focus_dist;
} fw_camera_settings;

typedef enum fw_rng_mode {
    FW_RNG_CTR = 0,  /* counter-based, keyed (seed,pixel,sample,dimension): the GPU's RNG (spec: DESIGN.md §RNG) */
    FW_RNG_LCG = 1   /* sequential per-pixel LCG seeded with the pixel index (render.rs:172); CPU oracle only    */
} fw_rng_mode;

/* Renderer (src/render.rs:59-77) + what the GPU path needs on top */
typedef struct fw_render_params {
    uint32_t width, height, samples;   /* Default: 1920, 1080, 128 (render.rs:207-209) */
    float gamma;                       /* Default 2.2 (render.rs:214) */
    int32_t use_bvh;                   /* Default false (render.rs:213) */
    int32_t multithreaded;             /* reference: rayon on/off; ignored by the HIP path */
    fw_camera_settings camera;
    uint64_t seed;                     /* CTR mode key; 0 by default */
    int32_t rng_mode;                  /* fw_rng_mode; the HIP path accepts FW_RNG_CTR only */
    /* Pixel subset for framebuffer tiling across GPUs: linear pixel indices
       (idx as in render.rs:127) this call renders, in output order.
       NULL => all width*height pixels in index order. */
    const uint32_t *pixel_ids;
    uint32_t n_pixels;
    uint32_t paths_per_batch;          /* wavefront pool size; 0 = library default */
    uint32_t flags;                    /* FW_FLAG_* */
    int32_t outputs_on_device;         /* !=0: the three output pointers are device pointers */
    void *stream;                      /* hipStream_t to launch on, NULL = default stream    */
} fw_render_params;

#define FW_FLAG_TIME_KERNELS 1u  /* bracket every launch with HIP events and fill fw_stats.ms_<class> */
#define FW_FLAG_COUNT_DEPOSITS 2u /* count the radiance records k_shade really wrote (one extra pass over the sample buffer per
                                     batch, outside the kernel classes' times): makes fw_stats.bytes_shade exact when zero
                                     deposits are elided over a black environment; without it they are counted as written */
#define FW_FLAG_LIGHT_SAMPLING 4u /* next-event estimation with MIS: every Lambertian and Isotropic vertex of segments 0-9
                                     samples one of the scene's sampled lights (EmissiveMat spheres and axis-aligned rectangles, picked
                                     uniformly) through a shadow ray, weighted against the BSDF's own sampling by the power heuristic.  The
                                     same pixels in expectation, with less noise; the paths themselves (fw_stats.rays, rays_per_depth) are
                                     the default frame's, shadow rays are not counted there (their walks count in ms_extend, their resolve in
                                     ms_shade; parked_rays includes their parks).  A scene without a sampled light or without a Lambertian
                                     or Isotropic material renders the default frame.  Honoured by fw_render, fw_render_progressive,
                                     fw_render_scene, fw_render_scene_tiled, fw_render_rays, fw_render_views and fw_render_adaptive (their
                                     frames go through the same path); ignored by fw_render_aovs (first-hit values carry no lighting).
                                     A build without it ignores the bit and renders the default frame. */
#define FW_FLAG_ENV_SAMPLING 8u   /* importance sampling of an HDR environment map: the map joins the sampled lights of
                                     FW_FLAG_LIGHT_SAMPLING (p_env = 1 alone, 1/2 beside the emitters, each emitter (1 - p_env) / n),
                                     sampled in proportion to max(r, g, b) x the solid angle of the texel env lookup returns, through a
                                     shadow ray that counts where it misses, with the same MIS weights.  The same pixels in expectation, with
                                     less noise under a bright sun; paths and shadow-ray accounting as FW_FLAG_LIGHT_SAMPLING.  The table is
                                     built on the device at the first render that asks for it and kept with the scene.  Nothing to sample (a
                                     ColorEnv or SkyEnv, a map of zero total weight, no Lambertian or Isotropic material): the frame without
                                     the bit, bit for bit.  Honoured and ignored by the same entry points as FW_FLAG_LIGHT_SAMPLING. */
#define FW_FLAG_ALL_EMITTERS 16u  /* with FW_FLAG_LIGHT_SAMPLING: the sampled emitters are every emitting primitive of an
                                     EmissiveMat object — a sphere, an axis-aligned rectangle, each face of a Rect3d, a Disk (full or an
                                     annular sector), each triangle of a TriangleMesh (objects that share a mesh each have their own) — and
                                     one is picked in proportion to area x power (power: max(r, g, b) of a ConstantTexture, negative or
                                     non-finite channels counted as 0; any other texture 1), through an alias table whose stored
                                     probabilities every estimate uses.  Flat primitives are sampled uniformly in area, spheres in their
                                     cone; a shadow ray counts only where its closest hit is the sampled primitive itself.  With
                                     FW_FLAG_ENV_SAMPLING the environment keeps p_env = 1/2 and each entry gets (1 - p_env) p_i.  Cones,
                                     cylinders and media are never sampled (their light keeps MIS weight 1).  The table is built at the
                                     first render that asks for it (the triangles' areas on the device, the alias table on the host) and
                                     kept with the scene; fw_scene_update keeps it.  Paths and shadow-ray accounting as
                                     FW_FLAG_LIGHT_SAMPLING.  Without FW_FLAG_LIGHT_SAMPLING the bit does nothing; a scene with no entry of
                                     positive weight (or no Lambertian or Isotropic material) renders the frame without the bit.  More than
                                     2^26 entries: FW_ERR_UNSUPPORTED before any launch.  Honoured and ignored by the same entry points as
                                     FW_FLAG_LIGHT_SAMPLING. */

#define FW_MAX_SEGMENTS 11  /* depths 0..10: render.rs:21 */

typedef struct fw_stats {
    uint64_t samples;                        /* camera samples = pixels * spp (render.rs:177)      */
    uint64_t rays;                           /* root.hit() calls = path segments (render.rs:19)    */
    uint64_t rays_per_depth[FW_MAX_SEGMENTS];
    uint64_t algorithmic_bytes;              /* 160*rays + 24*samples (+12*env misses for HDR), SURVEY §8(d) */
    double ms_scene;                         /* host: flatten + BVH build + LAUNCH of the upload (one-shot call only); the upload kernel itself is asynchronous and the render that follows waits for it, so its time is part of ms_render */
    double ms_render;                        /* device: first launch to last, HIP events on the launch stream */
    double ms_raygen, ms_extend, ms_shade, ms_accumulate; /* per-kernel-class device time (HIP events) */
    uint32_t n_extend_launches, n_shade_launches, n_batches;  /* FIREWORK_FUSED=1: no extend launches, the fused
                                                                 intersect+shade launches are counted and timed as shade */
    uint32_t tlas_nodes, blas_nodes;
    uint32_t reserved;                       /* bits 0-15 / 16-30: depth of the BLAS / TLAS walked; bit 31: this frame's launches were replayed as one hipGraph (option GRAPH) */
    /* HBM bytes THIS layout has to move, per kernel class, exact from the queue counters (DESIGN.md §5 gives the per-ray
       figures; SURVEY's generic 160 B/ray formula stays in algorithmic_bytes): what roofline fractions are computed from. */
    uint64_t bytes_raygen, bytes_extend, bytes_shade, bytes_accumulate;
    uint64_t deposits;                       /* radiance records written by k_shade (FW_FLAG_COUNT_DEPOSITS), else the terminated paths */
    uint64_t parked_rays;                    /* rays handed from the TLAS walk to k_blas (use_bvh with meshes) */
    double ms_wall;                          /* host wall time of the whole call (fw_render_scene: conversion + BVH + upload + render + D2H) */
    double ms_d2h;                           /* device -> host copies of the outputs (0 when outputs_on_device) */
} fw_stats;

typedef struct fw_scene fw_scene;  /* opaque: flattened SoA scene + BVHs resident in HBM */

/* ---- entry points -------------------------------------------------------- */
int fw_abi_version(void);
const char *fw_strerror(int status);
const char *fw_last_error(void);            /* thread-local detail for the last failing call */
int fw_device_count(void);                  /* number of visible HIP devices (0 if none) */

/* Initialisation of one device, explicit and idempotent (ABI v7): the HIP context, this library's code objects and kernel
   handles, its streams and pinned staging, and a path arena of `arena_bytes` (0 = the default: a third of the free HBM, at most
   64 GiB — every default-budget frame of the BASELINE configs fits; FW_INIT_NO_ARENA = none, the first render sizes its own).
   Loading the library makes NO HIP call and holds no memory; a host that never calls fw_init gets the same initialisation,
   without an arena, from its first fw_scene_create / fw_render* on the device (SURVEY §8(b) "Ownership": a lazily created
   per-device context is the only global state).  What it is for: the reference's timed region (main.rs:40-44) starts with
   the process already loaded; a host that wants that region free of one-off costs (0.2-1.1 s for context, code objects
   and, where the driver has pages to clear, the arena) calls fw_init first — `python -m firework_amd` and bench.py do.
   Calling it again with a larger arena_bytes grows the arena; a smaller one changes nothing. */
#define FW_INIT_NO_ARENA UINT64_MAX
int fw_init(int device, uint64_t arena_bytes);

/* `Scene -> SceneInternal` (scene.rs:111-135) + `build_bvh` (bvh.rs:79-85, mesh.rs:21-30):
   flatten, build TLAS/BLAS with the reference's median split, upload to `device`. */
int fw_scene_create(const fw_scene_desc *desc, int device, fw_scene **out);
void fw_scene_destroy(fw_scene *scene);

/* Moves the objects of a resident scene (additive at ABI 8): `desc` describes the scene `scene` was created from, and only the
   `position`, `rotation` and `flip_normals` of its objects may differ.  After FW_OK every later call on `scene` gives bit for bit
   what the same call gives on the scene fw_scene_create(desc) makes, with the same options in force at creation, update and call.
   The object level alone is redone — object records, world boxes, the top-level trees — and only its sections are uploaded; the
   meshes are not flattened again, and textures and environment maps are not uploaded again.  Exception: where the new placements
   reach coordinates larger than a mesh's trees were built for, the whole scene is re-created from desc behind the same handle (every
   mesh flattened again, everything uploaded again).  Memory: the first update moves the object-level sections into an
   allocation of the scene's own; their first copies stay, unread, in the scene's creation allocation until the scene is destroyed
   (about 300 bytes per object: records, boxes, ranks and both top-level trees).
   The caller promises that the arrays desc points to (vertices, indices, normals, uvs, image and HDR pixels) hold what they held at
   creation: they are not compared.  Errors, before any device state is touched (a failed update leaves the scene as it was):
   FW_ERR_BAD_ARG for a NULL argument, another object, shape, material or texture count, another objects[i].shape, any other
   difference in a field of a shape, material, texture or the environment that is not a pointer, or in whether a pointer is NULL;
   a placement fw_scene_create rejects gets the status create returns for desc (a NaN position: FW_ERR_NAN_BBOX).
   Synchronisation is fw_scene_create's: the upload is queued on the library's upload stream and every later call on the device waits
   for it in stream order.  An update must not run at the same time as another call on the same scene. */
int fw_scene_update(fw_scene *scene, const fw_scene_desc *desc);

/* ---- point, spot and directional lights (additive at ABI 8) ---------------------------------------------------------
   Lights without area.  No path can hit one, so they are found by next-event estimation alone: where a resident scene has n > 0 of them
   and some material is Lambertian or Isotropic, every Lambertian and Isotropic vertex of segments 0-9 picks one light and casts a shadow
   ray at it.  No flag is needed.  The paths themselves (fw_stats.rays, rays_per_depth) are those of the frame without lights, and shadow
   rays are accounted as under FW_FLAG_LIGHT_SAMPLING, whose frame layout such a frame takes.  The pick: the lights alone, each 1/n; with
   FW_FLAG_LIGHT_SAMPLING in effect, the group of these lights 1/2 (uniform inside) and the emitters the other half.  Such a sample has
   MIS weight 1 and adds beta x albedo x p_b(w) x L / p:
     point        w = normalized(position - x),  L = intensity / d^2,  visible if the shadow ray meets nothing before the light
     spot         as point, L = intensity s / d^2: c = -w . direction, t = clamp((c - cos_outer) / (cos_inner - cos_outer), 0, 1),
                  s = t^2 (3 - 2t); with cos_inner == cos_outer, s = 1 where c >= cos_outer and 0 otherwise
     directional  w = -direction,  L = intensity (an irradiance),  visible if the shadow ray meets nothing at all
   Honoured by every frame of a resident scene: fw_render, fw_render_progressive, fw_render_views, fw_render_adaptive, fw_render_rays and
   fw_render_model.  fw_render_aovs and fw_render_model_aovs ignore them (first-hit values carry no lighting).  The one-shot calls that
   take a fw_scene_desc, fw_render_scene and fw_render_scene_tiled, have no lights: fw_scene_desc carries none.
   Not supported together: FW_FLAG_ENV_SAMPLING or FW_FLAG_ALL_EMITTERS in a frame whose lights are active gives FW_ERR_UNSUPPORTED. */
typedef enum { FW_LIGHT_POINT = 0, FW_LIGHT_SPOT = 1, FW_LIGHT_DIRECTIONAL = 2 } fw_light_kind;
typedef struct fw_light {
    int32_t kind;
    fw_vec3 position;    /* point, spot */
    fw_vec3 direction;   /* spot: the axis it shines along; directional: the direction the light TRAVELS; any non-zero length, normalised by the library */
    fw_vec3 intensity;   /* point, spot: radiant intensity I (per steradian); directional: irradiance E on a plane facing it; each >= 0, finite */
    float cos_inner, cos_outer;   /* spot: full intensity inside cos_inner, none outside cos_outer; -1 <= cos_outer <= cos_inner <= 1 */
} fw_light;
#define FW_MAX_LIGHTS 65536u
/* Replaces the scene's lights with lights[0..n); n = 0 (lights may be NULL) removes them, and the scene then renders what it rendered before
   it had any, bit for bit.  Everything is validated before device state is touched, and a rejected call leaves the scene as it was.
   FW_ERR_BAD_ARG, with a detail string: a NULL scene, NULL lights with n > 0, n above FW_MAX_LIGHTS, an unknown kind, a non-finite field
   (of any light, used by its kind or not), a negative intensity, a zero direction of a spot or directional light, spot cosines outside
   -1 <= cos_outer <= cos_inner <= 1.  Fields a kind does not use (a directional light's position, a point light's direction and
   cosines) are otherwise ignored.  The lights live in an allocation of the scene's own, uploaded as fw_scene_update uploads; fw_scene_update keeps
   them.  Must not run at the same time as another call on the same scene. */
int fw_scene_set_lights(fw_scene *scene, const fw_light *lights, uint32_t n);
/* The same validation, on the host alone: no device is touched, and none is needed. */
int fw_check_lights(const fw_light *lights, uint32_t n);

/* The hot path: render.rs:123-161 on an uploaded scene.
   Any output pointer may be NULL.  Sizes are N*3 with N = n_pixels (or width*height),
   index order = pixel_ids order, row 0 = image top (util.rs:31-33):
     rgb8       : Color quantisation `(c*255.99) as u8`   (util.rs:14-23)
     gamma_rgb  : post-gamma, clamped floats in [0,1]      (render.rs:185-187) — the parity metric's input
     linear_rgb : pre-gamma per-pixel sample mean          (render.rs:184) */
int fw_render(fw_scene *scene, const fw_render_params *params,
              uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* One-shot render of a whole frame on SEVERAL GPUs from ONE process (what a single Rust binary calls; the Python hosts of
   this repo use one process per GPU and an RCCL gather instead): the frame is cut into 16x16 tiles dealt diagonally over the
   devices, one host thread per device creates the scene there and renders its pixels — with the keys a single GPU would
   use, so the image is bit-identical for any device list — copies its finished tiles peer-to-peer (hipMemcpyPeer: xGMI where
   the devices are linked) to the first listed device, which scatters them to their pixels and sends the frames to the
   caller's host buffers in one transfer.
   `devices` may name a device more than once (its calls are serialised).  render.rs:127-131 shards pixels over rayon workers
   the same way.  stats: counters summed, times = the slowest device. */
int fw_render_scene_tiled(const fw_scene_desc *desc, const fw_render_params *params, const int *devices, int n_devices,
                          uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* Progressive / resumable rendering (progressive preview, checkpointable accumulation buffer).
   Renders the samples [first_sample, first_sample + params->samples) of every pixel, adds them to `accum`
   (n_pixels x 4 floats: r, g, b sums and the number of path segments of the samples that deposited a record — every sample
   unless the environment is black, where zero deposits are elided; all zeros before the first call; host memory, or device memory when
   params->outputs_on_device) and resolves accum / (first_sample + samples) into the output buffers (any may be NULL).
   Every random draw is keyed by (pixel, ABSOLUTE sample index) and a pixel's sums are taken in sample order, so k calls
   of n samples leave bit for bit the accum and the image of one call of k*n samples — whatever is done with `accum`
   between the calls: show a preview, write it to disk, resume in another process.
   Reference: render.rs:172-190 sums `samples` colours per pixel and divides once; there is no progressive mode there. */
int fw_render_progressive(fw_scene *scene, const fw_render_params *params, uint32_t first_sample, float *accum,
                          uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* Adaptive sampling: renders a whole frame until every pixel's noise estimate meets `tolerance`, or its sample count reaches the cap
   params->samples.  Every pixel first gets `min_samples` samples.  After a round in which the active pixels reached n samples, a pixel
   stays active if it has not converged and n < cap, and the next round renders the samples [n, min(2n, cap)) of the active pixels only;
   final counts therefore lie in {min, 2 min, 4 min, ..., cap}.  The rule, evaluated on the device in float32 (IEEE, no contraction):
       nf = (float)n;  S_c, Q_c = the pixel's sum and sum of squares of channel c (r, g, b), in sample order
       m_c = S_c / nf;  v_c = (Q_c - S_c * m_c) / (nf - 1);  L = ((m_r + m_g) + m_b) / 3;  t = tol * (L > 1/256 ? L : 1/256)
       converged <=> all six of S_c, Q_c finite AND v_c <= (t * t) * nf for every c
   (the standard error of every channel's mean is at most tol x the mean brightness; a pixel with a non-finite sum runs to the cap).
   Every draw is keyed by (pixel, absolute sample) and sums are taken in sample order, so for every pixel p with final count n_p, accum[p],
   rgb8, gamma_rgb and linear_rgb equal bit for bit what fw_render (or fw_render_progressive) at n_p samples gives that pixel, under every
   kernel-selecting option.  Outputs (any may be NULL), W*H entries each in row-major pixel order:
     accum        : n x 4 floats, fw_render_progressive's layout (r, g, b sums, then path segments)
     moments      : n x 4 floats, r, g, b sums of squares, and .w = the pixel's final sample count as a float
     rgb8 / gamma_rgb / linear_rgb : as fw_render, each pixel resolved with its own count
     round_pixels : 32 entries, the active pixels of each round followed by zeros (at most 1 + ceil(log2(cap / min)) rounds)
   With params->outputs_on_device every output is a device pointer, as in fw_render.  Errors: FW_ERR_BAD_ARG for a NULL scene or params,
   params->pixel_ids != NULL (whole frames only), min_samples < 2, samples < min_samples, samples > 2^24, a tolerance that is not finite
   or <= 0 — all checked before the scene is looked at; FW_ERR_UNSUPPORTED for FW_RNG_LCG; FW_ERR_NO_DEVICE without a GPU.
   stats: samples = the sum of the final counts; rays, rays_per_depth, n_batches and the byte counts summed over the rounds; ms_render =
   first launch to last; the per-class times under FW_FLAG_TIME_KERNELS (the accumulation with squares counted in ms_accumulate).
   Synchronisation is fw_render's: the launches go to params->stream after the scene's upload, and the call returns after that stream has
   drained (it also waits for one 4-byte survivor count per round).  A round never runs as a frame graph (option GRAPH); if it grows the
   path workspace, the cached frame graph's key is cleared, as fw_trace_rays does. */
int fw_render_adaptive(fw_scene *scene, const fw_render_params *params, float tolerance, uint32_t min_samples,
                       float *accum, float *moments, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb,
                       uint32_t *round_pixels, fw_stats *stats);

/* Several camera views of an uploaded scene in one call: turntables, fly-throughs, stereo pairs, multi-view image sets.  View v of the
   outputs equals bit for bit what fw_render(scene, params', ...) writes, where params' is *params with camera = cameras[v], under every
   kernel-selecting option; params->camera is ignored and every other field keeps its meaning (pixel_ids / n_pixels: the same subset in
   every view; one seed for all views).  The frame's pixel space is (view, pixel), view-major: the batches of the wavefront loop hold
   every view's paths, and a path's random draws are keyed by (seed, its real pixel, its absolute sample) and never by its view.  Views are
   rendered in consecutive groups that fit the batch budget (paths_per_batch, or the library's default), each group with its own sample loop.
   Outputs (any may be NULL) are view-major, n_views x N x 3 with N = n_pixels (or width*height): view v occupies [v*N*3, (v+1)*N*3), in
   fw_render's order inside it.  With params->outputs_on_device they are device pointers, as in fw_render.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, params or cameras,
   n_views == 0, any argument fw_render rejects as FW_ERR_BAD_ARG, a camera with a non-finite field; FW_ERR_UNSUPPORTED for FW_RNG_LCG,
   an image fw_render rejects as too large, n_views x N >= 2^32; then FW_ERR_NO_DEVICE without a GPU.
   stats: samples, rays, rays_per_depth, deposits and parked_rays equal the sums over the per-view fw_render calls; n_batches, the launch
   counts and the byte counts are this call's own (the bytes it moves: the pixel table is read for every path, and the 16-byte camera rays
   are used only when every view is a pinhole at one position, bit for bit); ms_render and the per-class times are summed over the groups,
   ms_wall covers the whole call.  The views never run as a frame graph (option GRAPH; reserved bit 31 stays clear): one call already
   spreads a frame's launches over all its views.  The cached graph of fw_render is left as it is.  Synchronisation is fw_render's. */
int fw_render_views(fw_scene *scene, const fw_render_params *params, const fw_camera_settings *cameras, uint32_t n_views,
                    uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* Radiance along caller-supplied rays (additive at ABI 8): panoramas and light probes, orthographic or fisheye views, irradiance probes,
   a sensor model of the caller's own.  Entry i (one output pixel) of absolute sample s runs render.rs:10-33 `color(ray, ...)` from its
   ray, with every draw keyed (seed, keys[i] or key_base + i, s, segment) exactly as a render keys pixel keys[i]; duplicate keys are
   allowed and give correlated draws, nothing else.  The call renders the absolute samples [first_sample, first_sample + samples).
     per_sample_rays = 1: rays holds samples x n_rays x 6 floats (origin, direction), sample-major: rays[s] is absolute sample
                          first_sample + s;  0: rays holds n_rays x 6 floats, the same ray for every sample (probes).
     accum : n_rays x 4 floats, fw_render_progressive's layout (r, g, b sums, then path segments), the sums of the samples
             [0, first_sample) — all zeros when first_sample is 0 — to which this call's samples are added in sample order; NULL
             only when first_sample == 0 (the sums then start from zero and are not returned).  k calls of n samples leave accum and
             the outputs of one call of k*n samples, bit for bit.
     outputs: accum / (first_sample + samples) resolved as fw_render resolves a pixel, in ray order, n_rays x 3 each; any may be NULL.
   With on_device, rays, keys, accum and the outputs are device pointers on the scene's device (the fast path: the rays are read by the
   ray-generation kernel where they lie); otherwise host memory, and the rays of each batch pass through pinned staging.
   The identity (the contract): for any fw_render_params P (any camera, aperture included, any seed, a pixel subset or the whole frame),
   with rays[s] = fw_camera_rays(P, device, first_sample + s), keys = P.pixel_ids (or NULL with key_base = 0 for a whole frame) and P's
   seed, use_bvh and gamma, accum, rgb8, gamma_rgb and linear_rgb equal fw_render_progressive(P, first_sample, accum)'s bit for bit,
   and for first_sample = 0 fw_render(P)'s (whole frames in row-major order); stats.rays and rays_per_depth equal theirs.  This holds
   under every kernel-selecting option.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, params or rays,
   n_rays == 0, samples outside 1..2^24, first_sample + samples >= 2^32, a gamma that is not finite or <= 0, a NULL accum with
   first_sample > 0, with on_device an accum that is not 16-byte aligned; then FW_ERR_NO_DEVICE without a GPU.  A ray with a non-finite
   component or an all-zero direction makes the call return FW_ERR_BAD_ARG after it has run: accum and the outputs are then unspecified,
   nothing faults and later calls are unaffected.
   stats as fw_render's for n_rays pixels (bytes_raygen counts the 24 bytes per sample read from rays).  The call never runs as a frame
   graph (option GRAPH; reserved bit 31 stays clear); if it grows the path workspace, the cached graph's key is cleared, as fw_trace_rays
   does, and fw_render's cached graph is otherwise left as it is.  Synchronisation is fw_render's with outputs_on_device: the launches go
   to `stream` after the scene's upload, and the call returns after that stream has drained. */
typedef struct fw_render_rays_params {
    uint32_t n_rays;            /* entries (output pixels) */
    uint32_t first_sample;      /* this call renders absolute samples [first_sample, first_sample + samples) */
    uint32_t samples;           /* 1 .. 2^24 */
    int32_t  per_sample_rays;   /* 1: rays = samples x n_rays x 6 floats, sample-major (rays[s] is absolute sample first_sample + s)
                                   0: rays = n_rays x 6 floats, the same ray for every sample (probes) */
    const uint32_t *keys;       /* n_rays RNG pixel keys (the `pixel` word of every draw), or NULL: key_base + i */
    uint32_t key_base;
    uint64_t seed;
    int32_t  use_bvh;
    float    gamma;
    uint32_t paths_per_batch;   /* 0 = library default */
    uint32_t flags;             /* FW_FLAG_TIME_KERNELS, FW_FLAG_COUNT_DEPOSITS */
    int32_t  on_device;         /* rays, keys, accum and the outputs are device pointers on the scene's device */
    void    *stream;
} fw_render_rays_params;

int fw_render_rays(fw_scene *scene, const fw_render_rays_params *p, const float *rays, float *accum,
                   uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* One-shot form with the reference's exact shape: `Renderer::render(&self, scene: Scene)`
   (render.rs:109): scene conversion + BVH build + render inside one call. */
int fw_render_scene(const fw_scene_desc *desc, const fw_render_params *params, int device,
                    uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* The wavefront workspace (path pools, tens of GB for big frames) is cached per device between calls — the library's
   only global state.  This frees it (e.g. before handing the GPU to another library). */
void fw_release_workspace(int device);

/* ---- ray queries (ABI v8) ------------------------------------------------
   The operation the renderer is built on, `Hitable::hit(ray, t_min, t_max, rng) -> Option<RaycastHit>` (render.rs:44-57), for the
   caller's own rays on an uploaded scene: picking, depth / normal / material / object-ID buffers, visibility, integrators of one's
   own.  A trace runs the launches of a render's first segment — the same walks, the same exact-walk flagging, the same options
   (BVH, WIDE, EXACT_ALL, EXACT_FORM, NO_DEFER, NO_HIT4, NO_LDS_TREES, NO_LDS_TRIS, WAVES, PATHS_PER_BATCH) — over the caller's rays.
     - t range: the renderer's fixed (0.001, 2e9) (render.rs:19).  There is no per-ray range.
     - A ray with a non-finite component or an all-zero direction is reported as a miss and never traced.
     - n_rays == 0 returns FW_OK and writes nothing.  A NULL scene or params, and NULL rays / hits with n_rays > 0, return
       FW_ERR_BAD_ARG; with on_device, hits must be 16-byte aligned.  Without a visible GPU the call returns FW_ERR_NO_DEVICE:
       there is no CPU fallback.
     - stats (may be NULL): rays = rays traced (= rays_per_depth[0]), parked_rays, n_batches, ms_render (first launch to last), and
       ms_extend (the walks alone) under FW_FLAG_TIME_KERNELS; every other field 0.
     - Synchronisation is fw_render's with outputs_on_device: the launches go to `stream` (after the scene's upload, which the stream
       waits for), and the call returns after that stream has drained — with on_device the hits are complete on return, and the
       caller's earlier work on `stream` is ordered before the trace reads the rays.
     - A trace leaves renders as they were: it may grow the device's path workspace, which changes the key of a frame graph cached
       by option GRAPH, so a render after it never replays launches recorded against memory the trace moved. */
#define FW_NO_HIT UINT32_MAX

typedef struct fw_hit {          /* RaycastHit (render.rs:35-41) of one ray; 48 bytes */
    float t;                     /* in units of |direction|: directions are never normalised (ray.rs) */
    fw_vec3 point, normal;       /* world space, as RenderObjectInternal::hit returns them (scene.rs:235-266) */
    float u, v;
    uint32_t material;           /* MaterialIdx */
    uint32_t object;             /* index into fw_scene_desc.objects; FW_NO_HIT on a miss, every other field 0 */
    uint32_t prim;               /* triangle of a TriangleMesh, face of a Rect3d, else 0 */
} fw_hit;

typedef struct fw_trace_params {
    int32_t use_bvh;             /* TLAS walk or the linear list (scene.rs:137-175), as in fw_render_params */
    uint32_t flags;              /* FW_FLAG_TIME_KERNELS */
    uint64_t seed;               /* CTR key of ConstantMedium's draws */
    uint32_t key_base;           /* ray i draws as (seed, pixel = key_base + i, sample 0, segment 0): fwo_trace's key at key_base 0 */
    uint32_t rays_per_batch;     /* 0 = library default (a render's pool size) */
    int32_t on_device;           /* rays and hits are device pointers on the scene's device */
    void *stream;                /* hipStream_t, NULL = default */
} fw_trace_params;

/* One root.hit(ray, 0.001, 2e9) (render.rs:19) per ray, on an uploaded scene.  rays: n_rays x 6 floats (origin, direction);
   hits: n_rays records in ray order. */
int fw_trace_rays(fw_scene *scene, const fw_trace_params *params, const float *rays, uint32_t n_rays, fw_hit *hits, fw_stats *stats);

/* The segment-0 rays k_raygen traces for `sample` of every pixel in params->pixel_ids (or all width*height pixels): n x 6 floats
   in pixel_ids order.  Camera::ray (camera.rs:109-116) with the renderer's own keys (params->seed), bit for bit the rays a render
   traces, origin included.  `rays` is host memory, or device memory on `device` when params->outputs_on_device (then on
   params->stream, complete on return). */
int fw_camera_rays(const fw_render_params *params, int device, uint32_t sample, float *rays);

/* ---- guide buffers and denoising (additive at ABI 8) -----------------------------------------------------------------------
   fw_render_aovs: per-pixel guide buffers ("AOVs") of the first hit, averaged over params->samples samples.  Sample s of pixel p is the
   segment-0 ray a render traces for it (fw_camera_rays(params, device, s)), traced by the render's segment-0 walks with the render's keys
   (seed, p, s, segment 0): a ConstantMedium draws what the render draws.  One 48-byte record per pixel, W x H x 12 floats in row-major
   pixel order (row 0 = top), three float4s:
       [0] albedo.xyz, coverage = hits / S        [1] normal.xyz, distance        [2] position.xyz, 0
   Per sample, in IEEE float32 without contraction (the kernels' division / square-root helpers, fw_selftest_arith):
     hit  : albedo = texture_sample(texture, u, v, point) for Lambertian and Isotropic, the albedo of a Metal, (1, 1, 1) for a Dielectric,
            texture_sample clamped to [0, 1] for an Emissive; normal = hit normal / sqrtf((nx*nx + ny*ny) + nz*nz) (0 if that is 0);
            distance = t * sqrtf((dx*dx + dy*dy) + dz*dz); position = the hit point
     miss : albedo = env_sample(d / sqrtf((dx*dx + dy*dy) + dz*dz)) clamped to [0, 1]; normal 0; no distance or position
   Sums in sample order in float32; albedo and normal are divided by S, distance and position by the pixel's hits (0 without hits).
   Errors, in this order: FW_ERR_BAD_ARG for a NULL scene, params or aov, params->pixel_ids != NULL (whole frames only), samples outside
   1..2^24, width or height 0, with outputs_on_device an aov not 16-byte aligned — all before the scene is looked at; FW_ERR_UNSUPPORTED
   for FW_RNG_LCG or W x H >= 2^32; FW_ERR_NO_DEVICE without a GPU.  stats (may be NULL): rays, n_batches, ms_render, ms_wall.
   Synchronisation is fw_render's (params->stream, complete on return).  The call never runs as a frame graph; if it grows the path
   workspace, the cached frame graph's key is cleared, as fw_trace_rays does.  Renders are left as they were. */
int fw_render_aovs(fw_scene *scene, const fw_render_params *params, float *aov, fw_stats *stats);

/* fw_denoise: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with SVGF's variance-guided luminance term, on the device in
   float32.  color = a linear_rgb as fw_render writes it (N x 3), aov = fw_render_aovs' records (N x 12), moments = fw_render_adaptive's
   (N x 4: sums of squares of r, g, b and .w = the pixel's count n) or NULL.  With eps = FW_DENOISE_EPS, per pixel p:
     demodulate : e_p = c_p / (a_p + eps) per channel
     variance   : var_c = max(0, (Q_c - n*c_c*c_c) / (n - 1)) (0 for n < 2);
                  v_p = ((var_r/(a_r+eps)^2 + var_g/(a_g+eps)^2) + var_b/(a_b+eps)^2) / 3 / n; without moments no luminance term
     iteration i = 0..L-1, step h = 2^i: taps q = p + h*(dx, dy), dx, dy in -2..2, inside the image; kappa = (1/16, 1/4, 3/8, 1/4, 1/16);
                  the centre's weight is kappa(0)^2, every other tap's
                    w = kappa(dx) kappa(dy) * max(0, n_p.n_q)^FW_DENOISE_NORMAL_POW
                        * exp(-|n_p.(x_q - x_p)| / (FW_DENOISE_PLANE * d_p + 1e-6))
                        * exp(-|l_p - l_q| / (FW_DENOISE_LUM * sqrt(g_p) + 1e-6))       (with moments only)
                  l = (e_r + e_g + e_b) / 3; g_p = the 3x3 blur of v around p, weights (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), in-image taps
                  with a finite v, renormalised; a tap whose e or v is not finite has weight 0.
                  e'_p = sum w e_q / sum w;  v'_p = sum w^2 v_q / (sum w)^2
     output     : out_p = e_p^(L) * (a_p + eps), then resolve_pixel(out_p, 1, gamma) into linear_rgb / gamma_rgb / rgb8 (any may be NULL).
                  A pixel with coverage 0 or a non-finite input colour, and every pixel at L = 0, passes its input colour through: at L = 0
                  the three outputs equal fw_render's bit for bit.
   One launch per iteration (ping-pong buffers of e and v), no atomics: two calls give the same bits.  Device scratch is allocated per
   call and freed on every path.  With on_device every array is a device pointer on `device` and the launches go to `stream` (complete on
   return); otherwise host arrays.  Errors, all before HIP is called: FW_ERR_BAD_ARG for a NULL p, color or aov, width or height 0,
   iterations > 10, gamma not finite or <= 0, device < 0, with on_device an aov or moments not 16-byte aligned; FW_ERR_UNSUPPORTED for
   W x H >= 2^32; then FW_ERR_NO_DEVICE without a GPU, and FW_ERR_BAD_ARG for a device index past the last one. */
#define FW_DENOISE_EPS 0.01f
#define FW_DENOISE_NORMAL_POW 128       /* 7 squarings */
#define FW_DENOISE_PLANE 0.01f
#define FW_DENOISE_LUM 128.0f
#define FW_DENOISE_ITERATIONS 5         /* the library's default L */
#define FW_DENOISE_MAX_ITERATIONS 10

typedef struct fw_denoise_params {
    uint32_t width, height;
    uint32_t iterations;    /* 0..10; 0 = no filtering; the library's default is FW_DENOISE_ITERATIONS */
    float gamma;            /* for gamma_rgb / rgb8, as fw_render_params.gamma */
    int32_t device;
    int32_t on_device;      /* every array is a device pointer on `device` */
    void *stream;           /* hipStream_t, NULL = default */
} fw_denoise_params;

int fw_denoise(const fw_denoise_params *p, const float *color, const float *aov, const float *moments,
               float *linear_rgb, float *gamma_rgb, uint8_t *rgb8);

/* fw_temporal: temporal accumulation, the other half of SVGF (Schied et al. 2017) — the previous frame's colour and moments are
   reprojected through the guide buffers, tested geometrically and merged with the current frame by sample counts; on the device in
   float32.  N = width x height pixels, row-major, row 0 = top.
     current : color (N x 3, a linear_rgb), moments (N x 4, fw_render_adaptive's layout: sums of squares of r, g, b and .w = the count
               n) or NULL, aov (N x 12, fw_render_aovs' records).  moments == NULL: n = params.samples and Q_c = n * (c_c * c_c),
               which is exact for one sample per pixel and a lower bound on the variance otherwise.
     history : hist_color (N x 3), hist_moments (N x 4): the previous call's out_color and out_moments; hist_aov (N x 12): the previous
               frame's guides.  All three NULL = a first frame: out_color = color and out_moments = moments (or the substitute above)
               bit for bit, out_history = 0.
     prev_position : N x 3 or NULL — for each current pixel the world position its first-hit surface point had in the previous frame.
               NULL = a static scene: aov's position.
     outputs : out_color (N x 3), out_moments (N x 4, the same layout: it feeds fw_denoise and the next fw_temporal unchanged),
               out_history (N floats: the carried-over count n_h, 0 where the history was rejected).  Any may be NULL; none may overlap a
               history array (the kernel gathers).
   Per current pixel p, with X = prev_position[p] or aov[p]'s position, n_p its normal, a_p its albedo, c its colour, (Q_c, n_c) its
   moments, eps = FW_DENOISE_EPS:
     1 pass     : coverage 0, or a non-finite c or X: out = the current values, n_h = 0.
     2 project  : with prev_camera's basis (camera.rs:74-107: w = normalize(cam_pos - look_at), u^ = normalize(cross((0, 1, 0), w)),
                  v^ = cross(w, u^), half_height = tan(vfov / 2), half_width = half_height * W / H):  e = X - cam_pos;
                  depth = -e.w (history rejected unless > 0);  u = 1/2 + (e.u^) / (2 half_width depth);
                  v = 1/2 + (e.v^) / (2 half_height depth);  x = u W - 1/2 the continuous column, row = H - (v H - 1/2) the continuous
                  row: the inverse of the camera ray through (x + 1/2, row + 1/2) (render.rs:178-179, util.rs's row shift included).
                  The history is rejected unless -1 < x < W and -1 < row < H.
     3 taps     : q = (floor x, floor row) + {0, 1}^2 with the bilinear weights b_q.  A tap is dropped if it lies outside the image;
                  b_q < FW_TEMPORAL_MIN_TAP (a camera that did not move keeps one tap of weight 1); its hist_color, hist_moments, or
                  hist_aov albedo, coverage or position is not finite; its count is not > 0; its coverage is 0;
                  n_p.n_q < FW_TEMPORAL_NORMAL_COS (both normalised: AOV normals are means; a zero or non-finite normal, n_p's included,
                  fails); |n_p.(x_q - X)| > FW_TEMPORAL_PLANE |X - prev cam_pos|.  No surviving tap: the history is rejected.
                  Otherwise b_q := b_q / sum of the survivors' b.
     4 resample : demodulated, so that the taps do not blur textures:  mean_h = (a_p + eps) sum b_q hist_color_q / (a_q + eps) per channel;
                  m2_h = (a_p + eps)^2 sum b_q (Q_q / n_q) / (a_q + eps)^2;  n_h = min(sum b_q n_q, max_history).
     5 merge    : n = n_h + n_c;  out_color = (n_h mean_h + n_c c) / n;  out Q = n_h m2_h + Q_c;  out .w = n;  out_history = n_h.
                  A merge that gives a non-finite value is a rejected history.  A rejected history gives the current values and n_h = 0.
   One launch, one thread per pixel, no atomics: two calls give the same bits.  IEEE float32 without contraction, the kernels' division
   and square root.  Specular surfaces lag: what is reprojected is the first hit.  Device scratch (host arrays only) is allocated per
   call and freed on every path.  With on_device every array is a device pointer on `device` and the launch goes to `stream` (complete
   on return).  Errors, all before HIP is called, in this order: FW_ERR_BAD_ARG for a NULL p, color or aov; width or height 0; a history
   that is only partly NULL; an output that overlaps a history array; max_history NaN or <= 0 (INFINITY is allowed); a camera with a
   non-finite field; device < 0; with on_device an aov, moments, history or out_moments array not 16-byte aligned; moments == NULL with
   samples == 0.  Then FW_ERR_UNSUPPORTED for W x H >= 2^32, FW_ERR_NO_DEVICE without a GPU, FW_ERR_BAD_ARG for a device index past the
   last one. */
#define FW_TEMPORAL_NORMAL_COS 0.9f
#define FW_TEMPORAL_PLANE 0.02f
#define FW_TEMPORAL_MIN_TAP 1e-3f

typedef struct fw_temporal_params {
    uint32_t width, height;
    fw_camera_settings camera;       /* the current frame's camera (not read by the statement above; kept with the frame it describes) */
    fw_camera_settings prev_camera;  /* the camera hist_aov was rendered with */
    uint32_t samples;                /* the current frame's count where moments == NULL */
    float max_history;               /* > 0: the largest sample count a pixel carries over; INFINITY = no cap */
    int32_t device;
    int32_t on_device;               /* every array is a device pointer on `device` */
    void *stream;                    /* hipStream_t, NULL = default */
} fw_temporal_params;

int fw_temporal(const fw_temporal_params *p, const float *color, const float *moments, const float *aov,
                const float *hist_color, const float *hist_moments, const float *hist_aov, const float *prev_position,
                float *out_color, float *out_moments, float *out_history);

/* ---- camera models on the device (additive at ABI 8) ---------------------------------------------------------------
   Non-pinhole cameras whose rays are generated on the device (k_model_rays) in the layout fw_render_rays reads: n_samples x W*H x 6
   floats (origin, direction), sample-major, row-major inside a sample with row 0 = the image top.
   Jitter: pixel p (= row * W + x) of absolute sample s gets the sub-pixel offset (xi_x, xi_y) in [0, 1)^2, with the 32-bit mix
       hash32(h) : h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16
       s32 = (uint32)seed ^ ((uint32)(seed >> 32) * 0x9E3779B9);  key = hash32(s32 ^ hash32(s + 0x9E3779B9))
       xi_axis = (hash32(hash32(2 p + axis) ^ key) >> 8) * 2^-24,  axis 0 = x, 1 = y
   (api.pixel_jitter in Python); jitter == 0: (1/2, 1/2).  Everything below is evaluated in float64 on the device and rounded to float32
   once; the basis is camera.rs's, computed in float64 on the host: w = unit(cam_pos - look_at), u = unit(Y x w), v = w x u.
   With px = x + xi_x and py = row + xi_y:
     FW_MODEL_PANORAMA      equirectangular, the inverse of the HDR environment lookup: uu = px / W, vv = 1 - py / H, phi = pi - 2 pi uu,
                            theta = pi vv - pi / 2, d = (cos theta cos phi, sin theta, cos theta sin phi); origin = cam_pos bit for bit.
                            look_at, view_height and fov are not used.
     FW_MODEL_ORTHOGRAPHIC  a view plane view_height high and view_height * W / H wide, centred on cam_pos: with s = px / W and
                            t = 1 - py / H, origin = (cam_pos + ((s - 1/2) view_width) u) + ((t - 1/2) view_height) v;
                            d = look_at - cam_pos bit for bit.  fov is not used.
     FW_MODEL_FISHEYE       equidistant, full frame: a = 2 px - W, b = H - 2 py, rho = sqrt(a a + b b), r = rho / sqrt(W W + H H),
                            theta = r * (fov / 2 in radians), d = sin theta * ((a u + b v) / rho) - cos theta * w, and d = -w where
                            rho = 0; origin = cam_pos.  fov is the full angle across the image diagonal in degrees, in (0, 360].
                            view_height is not used.
   The camera's vfov, aperture and focus_dist are carried (they must be finite) and not used. */
typedef enum fw_model_kind {
    FW_MODEL_PANORAMA = 0,
    FW_MODEL_ORTHOGRAPHIC = 1,
    FW_MODEL_FISHEYE = 2
} fw_model_kind;

typedef struct fw_camera_model {
    int32_t kind;                /* fw_model_kind */
    uint32_t width, height;
    fw_camera_settings camera;   /* cam_pos and look_at */
    double view_height;          /* orthographic: finite and > 0 */
    double fov;                  /* fisheye: degrees, in (0, 360] */
    int32_t jitter;              /* 0: every sample goes through the pixel centres */
    uint64_t seed;               /* of the jitter (a render's own draws take fw_render_rays_params.seed) */
    uint32_t chunk_samples;      /* fw_render_model: samples whose rays are generated at a time; 0 = as many as fit 256 MiB */
} fw_camera_model;

/* fw_model_rays: the rays of the absolute samples [first_sample, first_sample + n_samples) of `model`, n_samples x W*H x 6 floats:
   fw_camera_rays' counterpart.  `rays` is host memory, or with on_device device memory on `device`, written on `stream` and complete on
   return.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL model or rays, an unknown kind, width or height
   0, a non-finite camera field, (orthographic, fisheye) cam_pos == look_at or a view direction parallel to Y, (orthographic) a
   view_height that is not finite and > 0, (fisheye) a fov outside (0, 360], n_samples == 0, first_sample + n_samples > 2^32, with
   on_device rays not 4-byte aligned; FW_ERR_UNSUPPORTED for W x H >= 2^31 (the jitter's counter 2 p + axis is 32-bit); then
   FW_ERR_NO_DEVICE without a GPU, and FW_ERR_BAD_ARG for a device index out of range. */
int fw_model_rays(const fw_camera_model *model, int device, uint32_t first_sample, uint32_t n_samples, float *rays, int on_device,
                  void *stream);

/* fw_render_model: radiance through a camera model.  Bit for bit — accum, the outputs, stats.rays and rays_per_depth — what
   fw_render_rays(scene, rp', rays = fw_model_rays(model, first_sample, samples), ...) gives, with rp' = *rp, per_sample_rays = 1 and
   keys = NULL (entry i is keyed key_base + i), for every chunk size; rp->per_sample_rays and rp->keys are ignored and rp->n_rays must be
   W x H.  The samples are rendered in chunks of model->chunk_samples (0: the most whose rays fit 256 MiB, at least 1): a chunk's rays
   are generated into device scratch that the call allocates and frees on every path, then rendered on top of the running sums as a
   fw_render_rays call of their own.  accum and the outputs are fw_render_rays' (host memory, or device memory with rp->on_device; accum
   may be NULL only when first_sample == 0).
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, model or rp, what
   fw_model_rays rejects in the model, samples outside 1..2^24, first_sample + samples >= 2^32, a gamma that is not finite or <= 0,
   n_rays != W x H, a NULL accum with first_sample > 0, with on_device an accum that is not 16-byte aligned; FW_ERR_UNSUPPORTED for
   W x H >= 2^31; then FW_ERR_NO_DEVICE.
   stats: fw_render_rays' fields summed over the chunks (tlas_nodes, blas_nodes and reserved: the last chunk's); ms_render includes the
   generator's launches, ms_raygen as well under FW_FLAG_TIME_KERNELS; ms_wall covers the whole call.  Synchronisation and the frame
   graph are fw_render_rays'. */
int fw_render_model(fw_scene *scene, const fw_camera_model *model, const fw_render_rays_params *rp, float *accum,
                    uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats);

/* fw_render_model_aovs: fw_render_aovs' guide buffers for a camera model: sample s of pixel p is the model's ray (fw_model_rays at
   sample s), traced and accumulated exactly as fw_render_aovs traces a camera ray — the same record layout, keys (params->seed, p, s,
   segment 0), walks and accumulation order — so the records feed fw_denoise unchanged.  Of params only samples, use_bvh, seed,
   outputs_on_device and stream are read; the frame's size is the model's.
   Errors, in this order: FW_ERR_BAD_ARG for a NULL scene, model, params or aov, what fw_model_rays rejects in the model, samples
   outside 1..2^24, with outputs_on_device an aov not 16-byte aligned; FW_ERR_UNSUPPORTED for W x H >= 2^31; FW_ERR_NO_DEVICE. */
int fw_render_model_aovs(fw_scene *scene, const fw_camera_model *model, const fw_render_params *params, float *aov, fw_stats *stats);

/* ---- irradiance probes baked on the device (additive at ABI 8) -----------------------------------------------------
   A probe set is n_probes positions with D directions each.  Its rays are generated on the device (k_probe_rays) in the layout
   fw_render_rays reads, and the rendered sums are reduced on the device (k_probe_project) to nine real spherical-harmonics
   coefficients (l <= 2) per probe and colour channel: neither rays nor radiance leave the device.
   Rays: entry i = p * D + j is direction j of probe p.  Its origin is positions[p] bit for bit.  Its direction in round r is a
   spherical Fibonacci lattice with a Cranley-Patterson shift (xi_u, xi_v) per (round, probe): fw_model_rays' hash with sample -> round
   and pixel -> probe,
       key = hash32(s32 ^ hash32(r + 0x9E3779B9)),  xi_u = (hash32(hash32(2 p) ^ key) >> 8) * 2^-24,  xi_v likewise from 2 p + 1
   (api.pixel_jitter(seed, r, n_probes)[p] in Python); jitter == 0: (1/2, 1/2).  Evaluated in float64 in this order and rounded to
   float32 once:
       u = (j + xi_u) / D;  c = 1 - 2 u;  rad = sqrt(max(0, 1 - c c));  t = j g + xi_v with g = (sqrt(5) - 1) / 2;  v = t - floor(t);
       phi = 2 pi v;  d = (rad cos phi, c, rad sin phi)                       (polar axis on world y)
   The directions are uniform on the sphere (density 1 / 4 pi).  api.ProbeSet.rays(round) is the numpy float64 statement.
   Basis: real orthonormal SH, index k = l (l + 1) + m, of the unit direction (x, y, z), constants formed in double:
       Y0 = 1/2 sqrt(1/pi)   Y1 = sqrt(3/4pi) y   Y2 = sqrt(3/4pi) z   Y3 = sqrt(3/4pi) x   Y4 = 1/2 sqrt(15/pi) x y
       Y5 = 1/2 sqrt(15/pi) y z   Y6 = 1/4 sqrt(5/pi) (3 z z - 1)   Y7 = 1/2 sqrt(15/pi) x z   Y8 = 1/4 sqrt(15/pi) (x x - y y) */
typedef struct fw_probe_set {
    uint32_t n_probes;
    const float *positions;   /* n_probes x 3, host memory always */
    uint32_t directions;      /* D: rays per probe and round, 1 .. 2^20 */
    int32_t  jitter;          /* 0: every round uses the shift (1/2, 1/2) */
    uint64_t seed;            /* of the shifts */
    uint32_t chunk_probes;    /* fw_bake_probes: probes rendered at a time; 0 = as many as fit 256 MiB of rays + sums, at least 1 */
} fw_probe_set;

/* fw_probe_rays: the rays of round `round` of the probes [first_probe, first_probe + n): n x D x 6 floats (origin, direction).
   `rays` is host memory, or with on_device device memory on `device`, written on `stream` and complete on return (fw_model_rays'
   contract).  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL set, positions or rays, n_probes == 0,
   directions outside 1..2^20, a non-finite position (its index is in fw_last_error()), n == 0, first_probe + n > n_probes, with
   on_device rays not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31; then FW_ERR_NO_DEVICE without a GPU, and
   FW_ERR_BAD_ARG for a device index out of range. */
int fw_probe_rays(const fw_probe_set *set, int device, uint32_t round, uint32_t first_probe, uint32_t n, float *rays, int on_device, void *stream);

/* fw_probe_project: adds one round's projection to the running sums.  rays: n_probes x D x 6 floats (the float32 directions are used as
   stored); accum: n_probes x D x 4 floats, fw_render_progressive's layout (r, g, b sums of `samples` samples, then segments); sums:
   n_probes x 9 x 3 floats.  For probe p, coefficient k and channel c, in float64,
       proj[p][k][c] = (4 pi / D) * sum_j Y_k(d_pj) * (double)accum[p D + j].c / samples
   is rounded to float32 once and added to sums[p][k][c] with one float32 addition.  One wave per probe: lane l accumulates
   j = l, l + 64, ... in ascending order, and the 64 lanes are combined by a fixed tree; no atomics: the result is a pure function of
   the inputs.  Host arrays, or with on_device device arrays on `device` (the kernel then works on the caller's memory), launched on
   `stream` and complete on return.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL rays, accum or sums,
   n_probes == 0, directions outside 1..2^20, samples outside 1..2^24, with on_device an accum that is not 16-byte aligned or rays or
   sums not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index
   out of range. */
int fw_probe_project(int device, uint32_t n_probes, uint32_t directions, uint32_t samples, const float *rays, const float *accum, float *sums, int on_device, void *stream);

/* fw_bake_probes: the rounds [first_round, first_round + rounds) of a probe set against a resident scene.  Of rp, samples (S per
   round), seed, use_bvh, paths_per_batch, flags, on_device (for sums and sh) and stream are read; n_rays, first_sample,
   per_sample_rays, keys, key_base and gamma are ignored.  For each round r and each chunk of probes [p0, p1) (set->chunk_probes at a
   time): k_probe_rays fills device scratch that the call allocates and frees on every path; a zeroed accum is rendered exactly as
   fw_render_rays would with per_sample_rays = 0, first_sample = 0, samples = S, key_base = p0 D, keys = NULL and seed = rp->seed + r;
   k_probe_project adds the chunk into sums.
     sums: n_probes x 9 x 3 floats, the running sums of the rounds [0, first_round) — all zeros when first_round is 0 — to which this
           call's rounds are added in order; NULL only when first_round == 0 (the sums then start from zero and are not returned).
     sh  : the same shape, float(sums / (double)(first_round + rounds)); may be NULL.
   Contracts.  Composition: for every chunk_probes, sums equals bit for bit what fw_probe_rays, fw_render_rays and fw_probe_project
   give when chained by hand on the device over the whole set.  Progressive: k calls of n rounds leave the sums and sh of one call of
   k n rounds, bit for bit.  The frames are fw_render_rays' own, so point, spot and directional lights and the light-sampling flags
   are honoured.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, set or rp, what
   fw_probe_rays rejects in the set, rounds == 0, first_round + rounds >= 2^32, samples outside 1..2^24, a NULL sums with
   first_round > 0, with on_device sums or sh not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31; then FW_ERR_NO_DEVICE.
   stats: fw_render_rays' fields summed over rounds and chunks as fw_render_model sums them; ms_render includes the two kernels'
   launches (under FW_FLAG_TIME_KERNELS ms_raygen and ms_accumulate as well); ms_wall covers the whole call.  Synchronisation and the
   frame graph are fw_render_rays'. */
int fw_bake_probes(fw_scene *scene, const fw_probe_set *set, const fw_render_rays_params *rp, uint32_t first_round, uint32_t rounds, float *sums, float *sh, fw_stats *stats);

/* ---- baked probes read back: irradiance at arbitrary points, and a frame lit from it (additive at ABI 8) --------------
   A probe grid is the two corners and the three counts api.ProbeSet.grid was given; sh is what fw_bake_probes wrote for that set,
   n x 9 x 3 float32 with n = nx ny nz, not repacked.  The lookup at a point p with normal n, everything in float64 from the float32
   inputs, every operation rounded as written (api.probe_lookup is the numpy statement):
     Cell, per axis k.  counts_k = 1: i_k = 0, f_k = 0 (a flat axis does not interpolate).  Otherwise
         s = ((p_k - lo_k) / (hi_k - lo_k)) * (counts_k - 1), clamped to [0, counts_k - 1] (max, then min: a point outside the grid takes
         the boundary's value);  i_k = min(floor(s), counts_k - 2);  f_k = s - i_k.
     Corner weights.  Corner (dx, dy, dz) in {0, 1}^3 — on an axis with counts_k = 1 only d_k = 0 — has w = (wx * wy) * wz with
         wx = 1 - f_x for dx = 0 and f_x for dx = 1, likewise wy and wz.
     FW_PROBE_WRAP (the usual guard against light from probes behind the surface, without visibility data).  With
         P_k = lo_k + (i_k + d_k) * ((hi_k - lo_k) / (counts_k - 1)), or 0.5 * (lo_k + hi_k) on a flat axis, r = P - p,
         rl = sqrt((r_x r_x + r_y r_y) + r_z r_z) and nh = n / sqrt((n_x n_x + n_y n_y) + n_z n_z) per component:
         h = 0.5 * (((nh_x * (r_x / rl) + nh_y * (r_y / rl)) + nh_z * (r_z / rl)) + 1);  w = w * (h * h + 0.2), or w * 1.2 when r is zero.
         The weights are then divided by their sum, added in the order dz, dy, dx with dx fastest.  Without the flag the trilinear
         weights are used as they are.
     Irradiance.  B_k = A_k * Y_k(nh) with the basis above (Y4 = (C x) y, Y5 = (C y) z, Y7 = (C x) z, Y6 = C (3 (z z) - 1),
         Y8 = C (x x - y y)) and the cosine lobe's band factors A = pi, 2 pi / 3 (k = 1..3), pi / 4 (k = 4..8), formed in double.  Per
         corner and channel e = B_0 sh[probe][0][c] + B_1 sh[probe][1][c] + ... with k ascending;  E_c = 0 + w e (corner 0) + w e
         (corner 1) + ... in the order dz, dy, dx with dx fastest;  E_c is rounded to float32 once.
   A point whose position is not finite, or whose normal has a non-finite component or zero length, gets (0, 0, 0).
   fw_probe_irradiance does not clamp: the negative lobes of an l <= 2 reconstruction are the caller's to see.  Every probe the lookup
   reads is one of the grid's, wherever the point lies.  One lane per point, no atomics: the result is a pure function of the inputs. */
#define FW_PROBE_WRAP 1u
typedef struct fw_probe_grid {
    double   lo[3], hi[3];    /* the two corners ProbeSet.grid was given */
    uint32_t counts[3];       /* nx, ny, nz >= 1; probe (ix, iy, iz) is entry (iz ny + iy) nx + ix of sh: x fastest, as ProbeSet.grid */
    uint32_t flags;           /* FW_PROBE_WRAP = 1u */
} fw_probe_grid;

/* fw_probe_irradiance: the lookup at n points.  positions and normals are read at i * stride_floats, three floats each: a stride of 3
   is two packed arrays, a stride of 12 with the pointers aov + 8 and aov + 4 reads fw_render_aovs' records in place.  irradiance: n x 3
   floats.  sh and the point arrays are host memory — staged through one device allocation of the call's own, the points in slabs of at
   most 256 MiB, freed on every path — or with on_device device memory on `device` (the kernel then works on the caller's memory),
   launched on `stream` and complete on return.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL grid, sh,
   positions, normals or irradiance, a count of 0, a non-finite corner, hi_k == lo_k on an axis with counts_k > 1, a hi_k - lo_k that
   overflows, unknown flag bits,
   n == 0, stride_floats < 3, device < 0, with on_device an array not 4-byte aligned; FW_ERR_UNSUPPORTED for nx ny nz >= 2^31; then
   FW_ERR_NO_DEVICE without a GPU, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_probe_irradiance(const fw_probe_grid *grid, const float *sh, int device, uint32_t n, const float *positions, const float *normals,
                        uint32_t stride_floats, float *irradiance, int on_device, void *stream);

/* fw_probe_shade: a frame's guide buffers lit from the grid.  aov = fw_render_aovs' records (W x H x 12 floats: albedo a, coverage v,
   normal, distance, position).  Per pixel E = the lookup at (position, normal), rounded to float32, then max(E, 0); in float32 without
   contraction
       out_c = a_c * (v * (E_c * (float)(1 / pi)) + (1 - v))
   and out goes through resolve_pixel(out, 1, gamma) into linear_rgb / gamma_rgb / rgb8 (any may be NULL, not all three), exactly as
   fw_denoise writes its outputs.  A pixel with v = 0 passes its albedo through: the environment's clamped colour.  Direct and indirect
   diffuse light both come from the probes.  The record does not mark emitters, so an EmissiveMat surface shows its clamped emission
   times E / pi; that and specular transport are out of scope.  Host arrays (staged as fw_probe_irradiance stages its own, the pixels
   in slabs), or with p->on_device device arrays on p->device, launched on p->stream and complete on return.  Errors, in this order and
   before HIP is called: FW_ERR_BAD_ARG for a NULL grid, sh, p or aov, all three outputs NULL, what fw_probe_irradiance rejects in the
   grid, width or height 0, gamma not finite or <= 0, device < 0, with on_device an aov not 16-byte aligned or sh, linear_rgb or
   gamma_rgb not 4-byte aligned; FW_ERR_UNSUPPORTED for nx ny nz >= 2^31 or W x H >= 2^32; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for
   a device index past the last one.  Neither call takes or touches a scene: renders, the path arena and the cached frame graph are
   left as they were. */
typedef struct fw_probe_shade_params {
    uint32_t width, height;
    float gamma;            /* for gamma_rgb / rgb8, as fw_render_params.gamma */
    int32_t device;
    int32_t on_device;      /* every array is a device pointer on `device` */
    void *stream;           /* hipStream_t, NULL = default */
} fw_probe_shade_params;
int fw_probe_shade(const fw_probe_grid *grid, const float *sh, const fw_probe_shade_params *p, const float *aov, float *linear_rgb,
                   float *gamma_rgb, uint8_t *rgb8);

/* ---- probe visibility: depth moments per probe, and lookups weighted by them (additive at ABI 8) ---------------------
   The lookup above blends a probe in a lit room with a probe in the dark room next door.  Each probe therefore also gets an R x R
   octahedral map of the first two moments of the distance to the nearest surface, baked from fw_trace_rays' hit distances along the
   probe's own rays, and the lookup multiplies a corner's weight by a Chebyshev bound of the chance that the corner's probe sees the
   point.  Everything is float64 from the float32 inputs, every operation rounded as written; max and min are fmax and fmin (a NaN
   operand loses).  api.probe_depth_dirs, api.probe_depth_reduce, api.probe_depth_moments and api.probe_lookup_vis are the numpy
   statements.
     Texel centres.  Texel (a, b) is column a, row b, id = b R + a.  ex = ((a + 0.5) * 2) / R - 1, ey likewise from b;
         z = (1 - |ex|) - |ey|;  if z < 0: x = (1 - |ey|) * sgn(ex), y = (1 - |ex|) * sgn(ey) with sgn(0) = +1, otherwise x = ex, y = ey;
         T = (x, y, z) / sqrt((x x + y y) + z z), per component.
     Reduction of one round (fw_probe_depth_reduce, k_probe_depth).  For probe p and ray j the float32 direction d is used as stored
         and h = hits[p D + j]:  dist_j = r_max if h.object == FW_NO_HIT, else min((double)h.t * sqrt((dx dx + dy dy) + dz dz), r_max).
         Per texel c = max(0, (Tx dx + Ty dy) + Tz dz), squared sharpness_log2 times to give w.  Three float64 accumulators start from 0
         and are updated sequentially in ascending j:  A = A + w*dist;  B = B + (w*dist)*dist;  W = W + w.  Each is rounded to float32
         once and added with one float32 addition to sums[p][b][a] = (A, B, W, unused): n_probes x R x R x 4 floats, .w never written.
         One lane owns a texel: no atomics, two runs are bit-equal, and the result does not depend on how the kernel splits the work.
     Moments: n_probes x R x R x 2 floats.  mu = float((double)sums.x / sums.z), mu2 = float((double)sums.y / sums.z); a texel with
         sums.z == 0 gets (r_max, float((double)r_max * r_max)).
     Fetch of (mu, mu2) along a unit direction (x, y, z) from a probe.  s1 = (|x| + |y|) + |z|, ox = x / s1, oy = y / s1; for z < 0 the
         fold of the texel centres: (ox, oy) <- ((1 - |oy|) * sgn(ox), (1 - |ox|) * sgn(oy)).  su = ((ox + 1) * 0.5) * R - 0.5 clamped to
         [0, R - 1] (max, then min), i = min(floor(su), R - 2), fu = su - i; sv, j, fv likewise from oy.  Bilinear over the four texel
         centres, m10 = texel (i + 1, j):  ((m00 (1 - fu) + m10 fu) (1 - fv)) + ((m01 (1 - fu) + m11 fu) fv).  Edges are clamped, not
         wrapped across the octahedral seams: a stated simplification.
     Visibility weight of a corner probe P (the lookup's P) for a point p with unit normal nh; normal_bias >= 0 in world units.
         q = p + normal_bias * nh per component, r' = q - P, dist = sqrt((r'x r'x + r'y r'y) + r'z r'z).  dist == 0: v = 1.  Otherwise
         (mu, mu2) is fetched along r' / dist;  dist <= mu: v = 1;  otherwise var = |mu mu - mu2|, t = dist - mu, c = var / (var + t t),
         v = (c c) c.  g = fac * v with fac the lookup's wrap factor (h h + 0.2, or 1.2 at r = 0), or 1 without FW_PROBE_WRAP;
         g = max(1e-6, g);  if g < 0.2: g = (g * (g * g)) * 25.  The corner's weight is w = ((wx wy) wz) * g, and the weights are always
         divided by their sum, added in the order dz, dy, dx with dx fastest (positive: every g is).
   Everything else is fw_probe_irradiance's statement unchanged: the cell, the flat axes, the basis, the order of E's sums, zeros for a
   non-finite point, one rounding of E.  Seam-correct borders, back-face detection, probe relocation and a view bias are out of scope. */
typedef struct fw_probe_depth {
    uint32_t resolution;      /* R in {4, 8, 16, 32}: each probe has an R x R octahedral map */
    uint32_t sharpness_log2;  /* k in 0..8: a ray's weight in a texel is max(0, T.d)^(2^k), by k squarings — no pow */
    float    max_distance;    /* r_max > 0, finite: distances are clamped to it; a miss counts as r_max */
} fw_probe_depth;

/* fw_probe_depth_reduce: adds one round's reduction to the running sums.  rays: n_probes x D x 6 floats; hits: n_probes x D records, as
   fw_trace_rays wrote them for those rays; sums: n_probes x R x R x 4 floats.  Host arrays — staged through one device allocation of the
   call's own, freed on every path — or with on_device device arrays on `device` (the kernel then works on the caller's memory), launched
   on `stream` and complete on return.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL pd, rays, hits or sums,
   a resolution not in {4, 8, 16, 32}, sharpness_log2 > 8, max_distance not finite or <= 0, n_probes == 0, directions outside 1..2^20,
   with on_device sums or hits not 16-byte aligned or rays not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31 or
   n_probes x R^2 >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index out of range. */
int fw_probe_depth_reduce(int device, const fw_probe_depth *pd, uint32_t n_probes, uint32_t directions, const float *rays, const fw_hit *hits,
                          float *sums, int on_device, void *stream);

/* fw_bake_probe_depth: the rounds [first_round, first_round + rounds) of a probe set's depth maps against a resident scene.  Of tp,
   use_bvh, flags, seed, rays_per_batch, on_device (for sums and moments) and stream are read; key_base is ignored.  For each round r and
   each chunk of probes [p0, p1) (set->chunk_probes at a time; 0 = as many as fit 256 MiB at 72 B per ray, at least 1): k_probe_rays
   fills device scratch that the call allocates and frees on every path; the rays are traced exactly as fw_trace_rays would with
   on_device = 1, key_base = p0 D and seed = tp->seed + r (so a ConstantMedium draws reproducibly); k_probe_depth adds the chunk into sums.
     sums   : n_probes x R x R x 4 floats (with on_device 16-byte aligned), the running sums of the rounds [0, first_round) — zeros when
              first_round is 0 — to which this call's rounds are added in order; NULL only when first_round == 0.
     moments: n_probes x R x R x 2 floats from the sums after this call, divided on the host; may be NULL.
   Contracts.  Composition: for every chunk_probes, sums equals bit for bit what fw_probe_rays, fw_trace_rays (seed + r, key_base 0) and
   fw_probe_depth_reduce give when chained by hand over the whole set.  Progressive: k calls of n rounds leave the sums and moments of one
   call of k n rounds, bit for bit.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, set, pd or tp, what
   fw_probe_rays rejects in the set, what fw_probe_depth_reduce rejects in pd, rounds == 0, first_round + rounds >= 2^32, a NULL sums
   with first_round > 0, with on_device sums not 16-byte aligned or moments not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31
   or n_probes x R^2 >= 2^31; then FW_ERR_NO_DEVICE.
   stats (may be NULL): fw_trace_rays' fields summed over rounds and chunks; ms_render includes the two kernels' launches (under
   FW_FLAG_TIME_KERNELS ms_raygen and ms_accumulate as well); ms_wall covers the whole call.  Synchronisation and what a trace leaves of
   renders are fw_trace_rays'. */
int fw_bake_probe_depth(fw_scene *scene, const fw_probe_set *set, const fw_probe_depth *pd, const fw_trace_params *tp, uint32_t first_round,
                        uint32_t rounds, float *sums, float *moments, fw_stats *stats);

/* fw_probe_irradiance_vis, fw_probe_shade_vis: fw_probe_irradiance and fw_probe_shade with the visibility weight above
   (k_probe_irradiance and k_probe_shade with DEPTH: one lane per point, no atomics).  moments: n x R x R x 2 floats for the grid's n probes,
   host memory or with on_device device memory like sh; a host call stages it after sh.  Every moments index is formed from clamped
   cell and texel indices: no load leaves the arrays wherever the point lies.  Errors, in this order and before HIP is called:
   FW_ERR_BAD_ARG for a NULL pointer (the counterpart's, pd, moments; fw_probe_shade_vis then: all three outputs NULL), a resolution not
   in {4, 8, 16, 32}, sharpness_log2 > 8, max_distance not finite or <= 0, normal_bias negative or not finite, then everything the
   counterpart rejects, in its order, with on_device moments not 4-byte aligned among the alignment checks; FW_ERR_UNSUPPORTED for
   nx ny nz >= 2^31, then for n x R^2 >= 2^31, then (fw_probe_shade_vis) for W x H >= 2^32; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a
   device index past the last one. */
int fw_probe_irradiance_vis(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias, int device,
                            uint32_t n, const float *positions, const float *normals, uint32_t stride_floats, float *irradiance, int on_device,
                            void *stream);
int fw_probe_shade_vis(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias,
                       const fw_probe_shade_params *p, const float *aov, float *linear_rgb, float *gamma_rgb, uint8_t *rgb8);

/* ---- lightmaps baked on the device: irradiance over a mesh's UV texels (additive at ABI 8) ---------------------------
   A fw_lightmap is one mesh placement and a texture size.  It reads nothing from a scene: the scene is only what the rays are traced
   against.  All its pointers are host memory.
   World transform: the tracer's own.  rows = the rotation matrix of `rotation` as fw_object's; a rotation with 1/2 (tr R - 1) >= 0.999
   (float32) is treated as no rotation; point = R p + position, normal = R n, formed in float64 from the float32 rows as
   ((R_k0 x + R_k1 y) + R_k2 z) + position_k; the normal is negated once for flip_normals and once for flip.
   Texels: texel (x, y), row 0 at the top, id = y W + x, has its centre at u = (x + 1/2) / W, v = 1 - (y + 1/2) / H, in float64 — the
   inverse of ImageTexture's lookup (i = floor(u w), j = floor((1 - v) h)), so a baked map put on the mesh as an image texture lands
   where it was baked.
   Coverage (k_lm_cover): with the float32 uvs widened to double, the edge function of the directed edge A -> B at the centre P is
       e(A, B; P) = ((B_u - A_u) (P_v - A_v)) - ((B_v - A_v) (P_u - A_u)),   every operation rounded in float64 as written;
   a texel is inside triangle (a, b, c) when e(a, b; P), e(b, c; P), e(c, a; P) are all >= 0 or all <= 0; a triangle with
   e(a, b; c) == 0 covers nothing; the lowest triangle index that covers a texel owns it (overlaps and shared edges included).
   Records (k_lm_texels): with area = e(a, b; c), b0 = e(b, c; P) / area, b1 = e(c, a; P) / area, b2 = e(a, b; P) / area, the
   object-space position is (b0 p0 + b1 p1) + b2 p2 per component, the normal the same interpolation of the vertex normals or, without
   normals, (p0 - p2) x (p1 - p2) (differences first, then (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x)), divided by its
   length sqrt((x x + y y) + z z); transformed, rounded to float32 once.  Record of texel id: 8 floats, (position.xyz, owner as bits),
   (normal.xyz, 0).  A texel whose normal has zero or non-finite length, or whose position or normal is not finite in float32, has no
   owner; a texel without an owner has the record (0, 0, 0, FW_NO_HIT bits), (0, 0, 0, 0).
   Covered list: the ascending texel ids with an owner; q indexes it.
   Rays (k_lm_rays): entry i = q D + j is direction j of covered texel q.  The shift (xi_u, xi_v) is fw_probe_rays' hash with
   probe -> texel id (api.texel_jitter in Python), so coverage and chunking never change a texel's rays; jitter == 0: (1/2, 1/2).
   In float64, in this order, rounded to float32 once, with n the record's float32 normal m made unit again, n = m / sqrt((m_x m_x +
   m_y m_y) + m_z m_z) (the frame is then orthonormal to float64 and d unit to one float32 rounding):
       u = (j + xi_u) / D;  r = sqrt(u);  c = sqrt(max(0, 1 - u));  t = j g + xi_v with g = (sqrt(5) - 1) / 2;
       phi = 2 pi (t - floor(t));  l = (r cos phi, r sin phi, c);
       s = copysign(1, n_z);  a = -1 / (s + n_z);  b = (n_x n_y) a;                          (Duff et al. 2017)
       T = (1 + (s (n_x n_x)) a, s b, -s n_x);  B = (b, s + (n_y n_y) a, -n_y);  d_k = (l_x T_k + l_y B_k) + l_z n_k
       origin_k = position_k + bias n_k   (bias == 0: the record's position bit for bit)
   The directions are cosine-distributed about n (density cos(theta) / pi). */
typedef struct fw_lightmap {
    const float *verts;        /* 3 * n_verts floats, fw_shape's meaning */
    uint32_t n_verts;
    const uint32_t *indices;   /* n_indices, a multiple of 3 */
    uint32_t n_indices;
    const float *normals;      /* NULL or 3 * n_verts floats */
    const float *uvs;          /* 2 * n_verts floats, required */
    fw_vec3 position;          /* fw_object's meaning */
    fw_rotor3 rotation;
    int32_t flip_normals;
    uint32_t width, height;    /* each 1 .. 16384 */
    uint32_t directions;       /* D: rays per texel and round, 1 .. 2^20 */
    int32_t  jitter;           /* 0: every round uses the shift (1/2, 1/2) */
    uint64_t seed;             /* of the shifts */
    float bias;                /* >= 0: the ray origin is position + bias x normal, world units */
    int32_t flip;              /* bake the other side */
    uint32_t chunk_texels;     /* fw_bake_lightmap: covered texels rendered at a time; 0 = as many as fit 256 MiB at 40 B per entry, at least 1 */
} fw_lightmap;

/* "The lightmap's checks" below — what is wrong in the description itself, FW_ERR_BAD_ARG, in this order: NULL verts, indices or uvs; n_verts == 0;
   n_indices == 0 or not a multiple of 3; width or height outside 1..16384; directions outside 1..2^20; bias negative or not finite; a
   non-finite position or rotation; a vertex index >= n_verts; a non-finite vert, uv or normal — fw_last_error() names the element.
   FW_ERR_UNSUPPORTED, which every call reports after its own argument checks and before HIP is called, when n_cov x D >= 2^31 cannot be
   ruled out from the host: min(W H, the texels of the triangles' clipped UV bounding boxes) x D >= 2^31. */

/* fw_lightmap_texels: records (W H x 8 floats), owner (W H uint32, FW_NO_HIT = none) and *n_covered; each may be NULL.  Host arrays,
   or with on_device device arrays on `device` (n_covered is host memory always), written on `stream` and complete on return.  Errors, in
   this order: FW_ERR_BAD_ARG for a NULL lm, the lightmap's checks, with on_device records not 16-byte or owner not 4-byte aligned;
   FW_ERR_UNSUPPORTED as above; FW_ERR_NO_DEVICE; FW_ERR_BAD_ARG for a device index out of range. */
int fw_lightmap_texels(const fw_lightmap *lm, int device, float *records, uint32_t *owner, uint32_t *n_covered, int on_device, void *stream);

/* fw_lightmap_rays: the rays of round `round` of the entries [first, first + n) of the covered list: n x D x 6 floats (origin,
   direction), host memory or with on_device device memory.  Errors: as fw_lightmap_texels with a NULL rays, n == 0, with on_device rays
   not 4-byte aligned among the argument checks; after the device is found, FW_ERR_BAD_ARG for first + n beyond the covered list. */
int fw_lightmap_rays(const fw_lightmap *lm, int device, uint32_t round, uint32_t first, uint32_t n, float *rays, int on_device, void *stream);

/* fw_lightmap_reduce: adds one round's cosine-weighted mean to running sums.  accum: n x D x 4 floats, fw_render_progressive's layout;
   sums: n_texels x 4 floats (an image of W x H texels), 16-byte aligned; texel_ids: n distinct ids < n_texels, or NULL for the identity
   (then n <= n_texels).  For entry q and channel c, in float64,
       proj = (pi / D) * sum_j ((double)accum[q D + j].c / samples)
   with G = the smallest power of two >= min(D, 64): lane l of a group of G takes j = l, l + G, ... in ascending order, the lanes are
   combined by an xor butterfly over the distances G/2 .. 1; proj is rounded to float32 once and added to sums[texel_ids[q]].c with one
   float32 addition.  .w is never written.  No atomics: two runs are bit-equal.  Errors, in this order and before HIP is called:
   FW_ERR_BAD_ARG for a NULL accum or sums, n == 0, n_texels == 0, directions outside 1..2^20, samples outside 1..2^24, n > n_texels
   without texel_ids, a host texel id >= n_texels, with on_device accum or sums not 16-byte or texel_ids not 4-byte aligned;
   FW_ERR_UNSUPPORTED for n x D >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index out of range. */
int fw_lightmap_reduce(int device, uint32_t n, uint32_t directions, uint32_t samples, const uint32_t *texel_ids, const float *accum, float *sums, uint32_t n_texels, int on_device, void *stream);

/* fw_lightmap_dilate: `passes` (0..64) dilation passes over image (W x H x 4 floats: rgb, a), in place.  In a pass a texel with a > 0
   is copied; a texel with a == 0 looks at its in-image neighbours in the order (dy, dx) = (-1,-1), (-1,0), (-1,1), (0,-1), (0,1),
   (1,-1), (1,0), (1,1): if n >= 1 of them have a > 0 its rgb becomes their float32 sum in that order divided by (float)n and its a 0.5;
   otherwise it is unchanged.  No wrap-around.  Errors: FW_ERR_BAD_ARG for a NULL image, width or height outside 1..16384, passes > 64,
   with on_device an image not 16-byte aligned; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index out of range. */
int fw_lightmap_dilate(int device, uint32_t width, uint32_t height, uint32_t passes, float *image, int on_device, void *stream);

/* fw_bake_lightmap: the rounds [first_round, first_round + rounds) of a lightmap against a resident scene.  Of rp the fields
   fw_bake_probes reads are read.  For each round r and each chunk [q0, q1) of the covered list (lm->chunk_texels at a time): k_lm_rays
   fills device scratch that the call allocates and frees on every path; a zeroed accum is rendered exactly as fw_render_rays would
   with per_sample_rays = 0, first_sample = 0, samples = S, key_base = q0 D, keys = NULL and seed = rp->seed + r; k_lm_reduce adds the
   chunk into sums.
     sums      : W x H x 4 floats (16-byte aligned on the device), the running sums of the rounds [0, first_round); NULL only when
                 first_round == 0.  .w is never written.
     irradiance: W x H x 4 floats, may be NULL: covered texels xyz = float(sums / (double)(first_round + rounds)), w = 1, every other
                 texel 0; then `dilate` (0..64) dilation passes.
   Contracts.  Composition: for every chunk_texels, sums equals bit for bit fw_lightmap_rays, fw_render_rays and fw_lightmap_reduce
   chained by hand over the whole covered list.  Progressive: k calls of n rounds leave the sums and irradiance of one call of k n rounds.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, lm or rp, the lightmap's
   checks, rounds == 0, first_round + rounds >= 2^32, samples outside 1..2^24, dilate > 64, a NULL sums with first_round > 0, with
   on_device sums or irradiance not 16-byte aligned; FW_ERR_UNSUPPORTED as above; then FW_ERR_NO_DEVICE.  stats: as fw_bake_probes. */
int fw_bake_lightmap(fw_scene *scene, const fw_lightmap *lm, const fw_render_rays_params *rp, uint32_t first_round, uint32_t rounds, uint32_t dilate, float *sums, float *irradiance, fw_stats *stats);

/* ---- ambient occlusion and bent normals of surface points (additive at ABI 8) ----------------------------------------
   What a probe grid cannot give: occlusion finer than the probe spacing.  For each of n surface points, D cosine-weighted hemisphere
   rays per round are traced against a resident scene at the renderer's fixed range and their hit distances compared with a radius
   afterwards; the share of occluded rays gives ao in [0, 1] (1 = open), the mean unoccluded direction the bent normal.  Everything is
   float64 from the float32 inputs, every operation rounded as written.  api.ao_rays, api.ao_reduce and api.ao_resolve are the numpy
   statements.
     Points.  Point q of a call is id = ids ? ids[q] : q; its position and its normal are three floats each at positions + id x
         stride_floats and normals + id x stride_floats, stride_floats >= 3.  ids: an optional list of n distinct uint32 (the caller
         promises it).  fw_render_aovs' records are read in place with stride 12, positions = aov + 8, normals = aov + 4;
         fw_lightmap_texels' records with stride 8, positions = rec, normals = rec + 4 and ids = the covered list.  sums and out are
         records of 16 B indexed by id: with ids they are shaped like the records, and entries outside the list are never touched.
         With host arrays and ids every array indexed by id spans max(ids) + 1 entries.  A point is unusable if a component of its
         position or normal is not finite or its normal is (0, 0, 0) — as of every pixel that missed the scene.
     Rays (fw_ao_rays, k_ao_rays): fw_lightmap_rays' statement with "texel id" replaced by id — the same hash of (seed, round, id) for
         the shift (xi_u, xi_v), or (1/2, 1/2) with jitter 0; u = (j + xi_u) / D, r = sqrt u, c = sqrt(max(0, 1 - u)), t = j g + xi_v,
         phi = 2 pi (t - floor t), l = (r cos phi, r sin phi, c) in the basis of Duff et al. 2017 around n = the float32 normal divided
         by its float64 length; origin = position + bias * n (bias 0: the position's bits); one rounding to float32.  Entry q D + j,
         6 floats.  Fed a lightmap's records and covered list with the lightmap's D, seed, jitter, bias and round the rays equal
         fw_lightmap_rays' bit for bit.  An unusable point gets D all-zero rays, which fw_trace_rays reports as misses and never traces.
     Reduction of one round (fw_ao_reduce, k_ao_reduce).  For ray j of point q, d the float32 direction as stored and h its hit: an
         all-zero d contributes nothing; otherwise dist = (double)h.t * sqrt((dx dx + dy dy) + dz dz);  o = 0 if h.object == FW_NO_HIT
         or dist >= radius, else o = 1 (falloff 0) or 1 - dist / radius (falloff 1).  Four float64 accumulators: O += o and
         B_k += (1 - o) * d_k.  With G = the smallest power of two >= min(D, 64), partial sum l takes j = l, l + G, ... in ascending
         order from 0, and the G partial sums are added by an xor butterfly over the distances G/2 ... 1 (x_l <- x_l + x_(l xor m)).
         Each accumulator is multiplied by the float64 1 / D, rounded to float32 once and added with one float32 addition to
         sums[id] = (Bx, By, Bz, O).  Two runs are bit-equal; a point's result depends on no other point.
     Resolve (k_ao_resolve), R = the number of rounds in sums: out[id] = (bx, by, bz, ao) with ao = float(min(1, max(0, 1 - (double)O /
         R))) and b = B / sqrt((Bx Bx + By By) + Bz Bz) in float64, rounded once; (0, 0, 0) when that length is 0 or not finite.  An
         unusable point resolves to (0, 0, 0, 1), a fully occluded one to (0, 0, 0, 0). */
typedef struct fw_ao {
    uint32_t directions;      /* D, 1..2^20 */
    uint32_t falloff;         /* 0 hard, 1 linear */
    float    radius;          /* > 0; +infinity allowed with falloff 0: any hit occludes */
    float    bias;            /* >= 0, finite */
    uint32_t jitter;          /* 0: the shift (1/2, 1/2) */
    uint32_t chunk_points;    /* fw_bake_ao: points per chunk; 0 = as many as fit 256 MiB at 72 B per ray, at least one */
    uint64_t seed;
} fw_ao;

/* fw_ao_rays: the rays of round `round` of the n points: n x D x 6 floats.  Host arrays — staged through device allocations of the
   call's own, freed on every path — or with on_device device arrays on `device`, generated on `stream` and complete on return.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL ao, positions, normals or rays; directions outside
   1..2^20, falloff > 1, radius not > 0 (or NaN), an infinite radius with falloff 1, bias negative or not finite; n == 0;
   stride_floats < 3; with on_device an array not 4-byte aligned; FW_ERR_UNSUPPORTED for n x D >= 2^31; then FW_ERR_NO_DEVICE, and
   FW_ERR_BAD_ARG for a device index past the last one. */
int fw_ao_rays(const fw_ao *ao, int device, uint32_t round, uint32_t n, const float *positions, const float *normals, uint32_t stride_floats,
               const uint32_t *ids, float *rays, int on_device, void *stream);

/* fw_ao_reduce: adds one round's reduction to the running sums.  rays: n x D x 6 floats; hits: n x D records as fw_trace_rays wrote
   them for those rays; sums: records indexed by id.  Host or device arrays as fw_ao_rays.  Errors, in this order and before HIP is
   called: FW_ERR_BAD_ARG for a NULL ao, rays, hits or sums; fw_ao_rays' checks of ao; n == 0; with on_device sums or hits not 16-byte
   aligned, rays or ids not 4-byte aligned; FW_ERR_UNSUPPORTED for n x D >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device
   index past the last one. */
int fw_ao_reduce(int device, const fw_ao *ao, uint32_t n, const uint32_t *ids, const float *rays, const fw_hit *hits, float *sums, int on_device,
                 void *stream);

/* fw_bake_ao: the rounds [first_round, first_round + rounds) of the n points against a resident scene.  Of tp, use_bvh, flags, seed,
   rays_per_batch, on_device (for positions, normals, ids, sums and out) and stream are read; key_base is ignored.  For each round r and
   each chunk of points [q0, q1) (ao->chunk_points at a time): k_ao_rays fills device scratch that the call allocates and frees on every
   path; the rays are traced exactly as fw_trace_rays would with on_device = 1, key_base = q0 D and seed = tp->seed + r (so a
   ConstantMedium draws reproducibly); k_ao_reduce adds the chunk into sums.  k_ao_resolve finishes.  On an error the stream is drained.
     sums: the running sums of the rounds [0, first_round) — zeros when first_round is 0 — to which this call's rounds are added in
           order; NULL only when first_round == 0.
     out : (bent.xyz, ao) after first_round + rounds rounds; may be NULL.
   Contracts.  Composition: for every chunk_points, sums equals bit for bit what fw_ao_rays, fw_trace_rays (seed + r, key_base 0) and
   fw_ao_reduce give when chained by hand over all n points.  Progressive: k calls of n rounds leave the sums and out of one call of k n
   rounds, bit for bit.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, ao, tp, positions or
   normals; fw_ao_rays' checks of ao; n == 0; stride_floats < 3; rounds == 0; first_round + rounds >= 2^32; a NULL sums with
   first_round > 0; with on_device sums or out not 16-byte aligned, positions, normals or ids not 4-byte aligned; FW_ERR_UNSUPPORTED for
   n x D >= 2^31; then FW_ERR_NO_DEVICE.
   stats (may be NULL): fw_trace_rays' fields summed over rounds and chunks (rays = the rays traced: zero rays are not); ms_render
   includes the two kernels' launches (under FW_FLAG_TIME_KERNELS ms_raygen and ms_accumulate as well); ms_wall covers the whole call.
   Synchronisation and what a trace leaves of renders are fw_trace_rays'. */
int fw_bake_ao(fw_scene *scene, const fw_ao *ao, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
               uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats);

/* ---- direct light of point, spot and directional lights at surface points (additive at ABI 8) -------------------------
   What probes and lightmaps lack: a light without area is hit by no ray, so nothing baked from rays holds it.  For each of n surface
   points and each of Ln lights one shadow ray is made, traced by the ordinary walks against a resident scene, resolved by
   fw_scene_set_lights' visibility rule and reduced per point.  Everything is float64 from the float32 inputs, every operation rounded as
   written (no contraction).  api.direct_rays, api.direct_reduce and api.direct_resolve are the numpy statements.
     Lights.  A light's record is what fw_scene_set_lights keeps: (position, kind), (direction, cos_inner), (intensity, cos_outer), twelve
         float32, the direction divided by its float64 length and rounded to float32.  fw_bake_direct reads the resident scene's records;
         the two stand-alone calls build them from a fw_light array with the same host code, after fw_check_lights' checks.
     Points.  fw_bake_ao's addressing: point q of a call is id = ids ? ids[q] : q; position and normal three floats each at id x
         stride_floats, stride_floats >= 3; ids an optional list of n distinct uint32; a point is unusable if a component of its position
         or normal is not finite or its normal is (0, 0, 0).  fw_render_aovs' records are read in place with stride 12 (positions = aov
         + 8, normals = aov + 4), fw_lightmap_texels' with stride 8 and the covered list.  view (may be NULL): the direction from the
         eye, three floats at view + id x view_stride_floats — a ray buffer is read in place at rays + 3 with stride 6.  spec (may be
         NULL, needs view): (F0.rgb, rho), four floats at spec + id x 4.  rho > 0: a glossy point (GgxMat); rho < 0: a point that takes no
         light sample (Metal, Dielectric, Emissive, a miss); any other rho, or no spec: a diffuse point.  sums and out are records of 32 B
         indexed by id; entries outside the list are never touched.  With host arrays and ids every array indexed by id spans max(ids)
         + 1 entries.
     Normal.  nh = the float32 normal divided by its float64 length; with view and face_view = 1 negated where nh . view > 0 (the dot
         product as (x x + y y) + z z on the view as stored): the side the eye sees is the side that is lit.
     Ray of point q and light i, entry q Ln + i, six floats rounded to float32 once: origin o = position + bias * nh (bias 0: the
         position's bits); direction d = the light's position - o for a point or spot light (not normalised: the light sits at t = 1), d
         = -(the record's direction) for a directional one.  With d2 = (dx dx + dy dy) + dz dz, w = d / sqrt(d2), c = nh . w and for a
         spot s = smooth(-(w . axis)): smooth(x) = 1 if x >= cos_outer else 0 where cos_inner <= cos_outer, otherwise t t (3 - 2 t) with
         t = min(max((x - cos_outer) / (cos_inner - cos_outer), 0), 1).  The entry is six zeros — which fw_trace_rays reports as a miss
         and never traces — if the point is unusable; spec is given and rho < 0; the three intensities are 0; d2 is 0 or not finite; not
         c > 0; a spot's s is 0; or a rounded component is not finite or the rounded direction is (0, 0, 0).
     Reduction of one round.  Entry (q, i) is a function of the stored float32 ray, its hit h, the light's record, nh, view and spec.  It
         contributes nothing if its stored direction is (0, 0, 0), the point is unusable or has rho < 0, a glossy point has no view or
         not wo . nh > 0, d2 of the stored direction is not finite, or not c > 0 (d2, w, c, s as above, from the stored direction).
         V = 1 if h.object == FW_NO_HIT; otherwise V = 1 iff the light is a point or spot light and h.t >= 1.0f; V = 0 contributes
         nothing more.  L = (I s) / d2 for a point or spot light (s = 1 for a point light), L = I for a directional one.
           N += 1.
           diffuse point:  E_k += L_k g,  g = c (lobe 0: E is an irradiance) or 2 ((c c) c) (lobe 1: pi x what fw_scene_set_lights'
               light sample adds per unit albedo at a Lambertian vertex, whose density is 2 c^3 / pi).
           glossy point:   S_k += L_k ((F0_k + (1 - F0_k) m5) gg): GgxMat's f cos = F D G2 / (4 wo . n) with wo = -(view / |view|), co =
               nh . wo, alpha = (double)(rho * rho) (the float32 product), a2 = alpha alpha, tan2(x, z) = |x - z nh|^2 / (z z),
               Lambda(x, z) = 0.5 (sqrt(1 + a2 tan2(x, z)) - 1), h = (wo + w) / |wo + w|, hn = nh . h, oh = wo . h,
               sd = |h - hn nh|^2 + a2 (hn hn), D = a2 / (pi (sd sd)), gg = (D / (4 co)) / ((1 + Lambda(wo, co)) + Lambda(w, c)),
               m = 1 - oh, m5 = ((m m)(m m)) m.  A conductor has no diffuse term: E gets nothing.
         Seven float64 accumulators per point (E.rgb, N, S.rgb).  With G = the smallest power of two >= min(Ln, 64), partial sum l takes
         i = l, l + G, ... in ascending order from 0, and the G partial sums are added by an xor butterfly over the distances G/2 ... 1
         (x_l <- x_l + x_(l xor m)): k_ao_reduce's tree with "directions" read as "lights".  Each accumulator is rounded to float32 once
         and added with one float32 addition to sums[id] = (E.rgb, N), (S.rgb, untouched): the eighth float is never written.  Two runs
         are bit-equal; a point's result depends on no other point.
     Resolve, R = the number of rounds in sums: out[id] = float((double)sums[id] / R) for the seven floats, the eighth 0.  Rounds exist
         because a ConstantMedium makes visibility a draw (round r traces with seed + r); without media every round is the same and one
         is exact.  An unusable point resolves to zeros. */
typedef struct fw_direct {
    uint32_t lobe;            /* 0 cosine (irradiance), 1 the renderer's diffuse lobe 2 c^3 */
    uint32_t face_view;       /* 0 / 1; ignored without view */
    float    bias;            /* >= 0, finite */
    uint32_t chunk_points;    /* fw_bake_direct: points per chunk; 0 = as many as fit 256 MiB at 72 B per ray, at least one */
} fw_direct;

/* fw_direct_rays: the n x Ln x 6 floats of the shadow rays.  Host arrays — staged through device allocations of the call's own, freed
   on every path — or with on_device device arrays on `device` (lights is always a host array), generated on `stream` and complete on
   return.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL direct, lights, positions, normals or rays; lobe
   > 1, face_view > 1, bias negative or not finite; n_lights == 0, then fw_check_lights' refusals with its messages; n == 0;
   stride_floats < 3; view with view_stride_floats < 3; spec without view (whether an entry has rho > 0 cannot be checked on device
   arrays); with on_device spec not 16-byte aligned or another array not 4-byte aligned; FW_ERR_UNSUPPORTED for n x Ln >= 2^31; then
   FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_direct_rays(const fw_direct *direct, const fw_light *lights, uint32_t n_lights, int device, uint32_t n, const float *positions,
                   const float *normals, uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats,
                   const float *spec, float *rays, int on_device, void *stream);

/* fw_direct_reduce: adds one round's reduction to the running sums.  rays: n x Ln x 6 floats; hits: n x Ln records as fw_trace_rays
   wrote them for those rays; sums: records of 32 B indexed by id.  Host or device arrays as fw_direct_rays.  Errors, in this order and
   before HIP is called: FW_ERR_BAD_ARG for a NULL direct, lights, positions, normals, rays, hits or sums; then fw_direct_rays' checks
   from lobe to spec without view; with on_device sums, hits or spec not 16-byte aligned or another array not 4-byte aligned;
   FW_ERR_UNSUPPORTED for n x Ln >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_direct_reduce(int device, const fw_direct *direct, const fw_light *lights, uint32_t n_lights, uint32_t n, const float *positions,
                     const float *normals, uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats,
                     const float *spec, const float *rays, const fw_hit *hits, float *sums, int on_device, void *stream);

/* fw_bake_direct: the rounds [first_round, first_round + rounds) of the n points under the resident scene's own lights
   (fw_scene_set_lights), read on the device where they lie.  Of tp, use_bvh, flags, seed, rays_per_batch, on_device (for positions,
   normals, ids, view, spec, sums and out) and stream are read; key_base is ignored.  For each round r and each chunk of points [q0, q1)
   (direct->chunk_points at a time): k_direct_rays fills device scratch that the call allocates and frees on every path; the rays are
   traced exactly as fw_trace_rays would with on_device = 1, key_base = q0 Ln and seed = tp->seed + r; k_direct_reduce adds the chunk
   into sums.  k_direct_resolve finishes.  On an error the stream is drained.  A scene without lights returns FW_OK, traces nothing,
   leaves sums as it was and writes out from it.
     sums: the running sums of the rounds [0, first_round) — zeros when first_round is 0 — to which this call's rounds are added in
           order; NULL only when first_round == 0.
     out : the resolved records after first_round + rounds rounds; may be NULL.
   Contracts.  Composition: for every chunk_points, sums equals bit for bit what fw_direct_rays, fw_trace_rays (on_device, seed + r,
   key_base 0) and fw_direct_reduce give when chained by hand over all n points with the scene's lights.  Progressive: k calls of m rounds
   leave the sums and out of one call of k m rounds, bit for bit.  Renders, and the frame graph's key, are left as fw_trace_rays leaves
   them.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, direct, tp, positions or
   normals; lobe > 1, face_view > 1, a bad bias; n == 0; stride_floats < 3; view with view_stride_floats < 3; spec without view; rounds
   == 0; first_round + rounds >= 2^32; a NULL sums with first_round > 0; with on_device sums, out or spec not 16-byte aligned, another
   array not 4-byte aligned; then FW_ERR_NO_DEVICE; then — Ln is the scene's, and a scene exists only where a device does —
   FW_ERR_UNSUPPORTED for n x Ln >= 2^31.
   stats (may be NULL): fw_bake_ao's — fw_trace_rays' fields summed over rounds and chunks (rays = the rays traced: zero rays are
   not); ms_render includes the two kernels' launches (under FW_FLAG_TIME_KERNELS ms_raygen and ms_accumulate as well); ms_wall covers
   the whole call.  Synchronisation and what a trace leaves of renders are fw_trace_rays'. */
int fw_bake_direct(fw_scene *scene, const fw_direct *direct, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
                   uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats, const float *spec,
                   uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats);

/* ---- SunSky: an analytic sun-and-sky environment (additive at ABI 8) ----------------------------------------------------
   Outdoor light from six numbers: single scattering of the sun through a Rayleigh and Mie atmosphere around a spherical ground, as an
   equirectangular map that loads as FW_ENV_HDR (fw_sky_map), along given directions (fw_sky_radiance), and the sun itself as a
   FW_LIGHT_DIRECTIONAL of the same energy (fw_sky_sun).  Everything is float64 from the float32 fields, every operation rounded as
   written (no contraction), one rounding to float32 at the end.  api.sky_radiance, api.sky_map and api.sky_sun are the numpy statements.
     Constants, metres: Rg = 6360000, Rt = 6420000, H_R = 7994, H_M = 1200, beta_R = (5.8e-6, 13.5e-6, 33.1e-6), beta_M = 21e-6 x
         turbidity with extinction beta_Me = 1.1 beta_M, g = 0.76.  The observer is O = (0, Rg + altitude, 0); the sun's direction is
         s = (cos el cos az, sin el, cos el sin az).  Dot products are (x x + y y) + z z.
     Ground test of (P, w): b = P . w, disc = b b - (P . P - Rg Rg); the ray meets the ground iff b < 0 and disc > 0.
     Optical depth D(P, w, N) = (dR, dM): t_l = -b + sqrt(b b - (P . P - Rt Rt)); for k = 0 .. N - 1 in order: f = (k + 0.5) / N,
         t = t_l (f f), width = t_l ((2 k + 1) / (N N)), Q = P + t w, h = sqrt(Q . Q) - Rg, dR += exp(-h / H_R) width, dM += exp(-h /
         H_M) width.  The spacing is quadratic: the samples crowd towards P, where the air is.
     T(P), per channel: exp(-(beta_R lR + beta_Me lM)) with (lR, lM) = D(P, s, NL), or 0 where (P, s) meets the ground.
     Radiance along the unit direction d: t_max = the atmosphere's exit from O (t_l of (O, d)), or where (O, d) meets the ground the hit
         -b - sqrt(disc).  oR = oM = 0; for i = 0 .. NV - 1 in order: f, t and width as above with t_max and NV, P = O + t d, h as above,
         hr = exp(-h / H_R) width, hm = exp(-h / H_M) width, (lR, lM) = D(P, s, NL), aR = (oR + 0.5 hr) + lR, aM = (oM + 0.5 hm) + lM,
         att_c = exp(-(beta_R,c aR + beta_Me aM)) or 0 where (P, s) meets the ground, S_R,c += att_c hr, S_M,c += att_c hm, then oR += hr,
         oM += hm.  With mu = d . s, m = 1 + mu mu, x = (1 + g g) - (2 g) mu:  p_R = (3 / (16 pi)) m,  p_M = ((3 / (8 pi)) ((1 - g g) m))
         / ((2 + g g) (x sqrt x)) — no pow —  and  L_c = E0_c ((S_R,c beta_R,c) p_R + (S_M,c beta_M) p_M).  A ground hit at G = O + t_max d
         adds (((exp(-(beta_R,c oR + beta_Me oM)) (albedo_c / pi)) E0_c) T_c(G)) max((G / |G|) . s, 0).
         Simplifications: single scattering, no ozone, the ground is lit by the sun alone, no limb darkening.
     Map.  Texel (x, row j) of the W x H map, row 0 at the top, is the radiance along its centre's direction by panorama_rays' formula,
         the exact inverse of the FW_ENV_HDR lookup: u = (x + 0.5) / W, v = 1 - (j + 0.5) / H, phi = pi - (2 pi) u, theta = pi v - pi /
         2, d = (cos theta cos phi, sin theta, cos theta sin phi).
     Disc (FW_SKY_DISC, and only where (O, s) does not meet the ground).  n_t = the number of the S x S directions of texel t at the
         offsets ((a + 0.5) / S, (b + 0.5) / S) in place of (0.5, 0.5) with d . s >= cos(sun_radius), c_t = n_t / (S S).  Omega_j = ((2
         pi) / W) (cos((j pi) / H) - cos(((j + 1) pi) / H)) is the solid angle of a texel of row j.  A = sum over the rows j in ascending
         order, from 0.0, of (N_j / (S S)) Omega_j with N_j = the exact integer sum of n_t over the row.  If A = 0, the texel that the
         FW_ENV_HDR lookup reads for s (float32, as env_sample computes it) takes c = 1 and A = its Omega.  Texel t then holds
         float(L_t + (E0 T(O) c_t) / A): sum_t disc_t Omega_t = E0 T(O) at every resolution, the energy of fw_sky_sun's light.
     Directions (fw_sky_radiance): d = the three floats divided by their float64 length; a zero or non-finite length gives (0, 0, 0).
         With FW_SKY_DISC a direction with d . s >= cos(sun_radius) gains E0 T(O) / ((2 pi) (1 - cos(sun_radius))).
     Two runs are bit-equal; a texel's value depends on no other texel. */
#define FW_SKY_DISC 1u
typedef struct fw_sky {
    float sun_elevation, sun_azimuth; /* radians; elevation in [-pi/2, pi/2]; azimuth is panorama_rays' phi */
    float turbidity;                  /* multiplies the Mie coefficient; [0, 64] */
    fw_vec3 sun_irradiance;           /* E0 above the atmosphere, on a plane facing the sun; each >= 0, finite: the exposure */
    float sun_radius;                 /* angular radius of the disc, radians, (0, 0.1]; the sun's is 0.00465 */
    float altitude;                   /* the observer's height in metres, [1, 50000] */
    fw_vec3 ground_albedo;            /* [0, 1] each */
    uint32_t view_steps, light_steps; /* NV in 1..64 (default 32), NL in 1..32 (default 16) */
    uint32_t sun_samples;             /* S in 1..16: S x S samples per texel for the disc's coverage (default 8) */
    uint32_t flags;                   /* FW_SKY_DISC: draw the sun into the map and the directions */
} fw_sky;

/* fw_check_sky: FW_OK, or FW_ERR_BAD_ARG for, in this order: a NULL sky; sun_elevation not finite or outside [-pi/2, pi/2]; sun_azimuth
   not finite; turbidity outside [0, 64]; a sun_irradiance component negative or not finite; sun_radius outside (0, 0.1]; altitude
   outside [1, 50000]; a ground_albedo component outside [0, 1]; view_steps outside 1..64; light_steps outside 1..32; sun_samples
   outside 1..16; flags with an unknown bit.  A NaN is outside every range.  Touches no device. */
int fw_check_sky(const fw_sky *sky);

/* fw_sky_map: the W x H x 3 floats of the map.  `rgb` is host memory — filled in slabs of rows through device scratch of the call's own,
   freed on every path — or with on_device device memory on `device`, written on `stream` and complete on return; overwritten.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL sky or rgb; fw_check_sky's refusals; width or height < 2;
   with on_device rgb not 4-byte aligned; FW_ERR_UNSUPPORTED for W x H >= 2^31; then FW_ERR_NO_DEVICE without a GPU (rgb untouched),
   and FW_ERR_BAD_ARG for a device index out of range. */
int fw_sky_map(const fw_sky *sky, int device, uint32_t width, uint32_t height, float *rgb, int on_device, void *stream);

/* fw_sky_radiance: rgb[q] = the radiance along the three floats at dirs + q x stride_floats, q < n; a ray buffer is read in place at
   rays + 3 with stride 6.  Host arrays or with on_device device arrays, as fw_sky_map.  Errors, in this order and before HIP is called:
   FW_ERR_BAD_ARG for a NULL sky, dirs or rgb; fw_check_sky's refusals; n == 0; stride_floats < 3; with on_device an array not 4-byte
   aligned; then FW_ERR_NO_DEVICE (rgb untouched), and FW_ERR_BAD_ARG for a device index out of range. */
int fw_sky_radiance(const fw_sky *sky, int device, uint32_t n, const float *dirs, uint32_t stride_floats, float *rgb, int on_device,
                    void *stream);

/* fw_sky_sun: the sun as a light: kind FW_LIGHT_DIRECTIONAL, direction float(-s), intensity float(E0 T(O)) — zeros where the sun is
   below the observer's horizon — every other field 0.  Host only: touches no device.  FW_ERR_BAD_ARG for a NULL sky or out, and
   fw_check_sky's refusals. */
int fw_sky_sun(const fw_sky *sky, fw_light *out);

/* ---- probe relocation and classification: move probes out of geometry (additive at ABI 8) -----------------------------
   A grid is laid over a scene without looking at it: some probes land inside objects or a hair from a wall.  A probe's own rays tell:
   fw_probe_survey reduces one round's hits to "how much of what the probe sees is a back face, and where is the nearest surface",
   fw_probe_relocate_step moves the probe and marks it active or inactive, fw_relocate_probes drives both against a resident scene, and
   the _placed lookups read baked probes where they went.  Everything is float64 from the float32 inputs, every operation rounded as
   written.  api.probe_survey, api.probe_relocate_step and api.probe_lookup_placed are the numpy statements.
     Placement: one 16-byte record (ox, oy, oz, a) per probe.  o is the offset from the probe's nominal position in world units, a is
         1.0 (active) or 0.0 (inactive).  The neutral record is (0, 0, 0, 1).
     Survey: one 48-byte record of three float4s per probe.  [0] = (back.xyz, dist): the stored float32 direction of the nearest
         back-face hit and its distance, (0, 0, 0, +inf) if none.  [1] the same for the nearest front-face hit.  [2] = (n_back, n_front,
         n_miss, 0) as floats, exact since D <= 2^20.
     Survey of one round (fw_probe_survey, k_probe_survey).  For ray j of probe p, d is the stored float32 direction and
         h = hits[p D + j].  An all-zero d is skipped and counts nowhere.  h.object == FW_NO_HIT is a miss.  Otherwise
         dist = (double)h.t * sqrt((dx dx + dy dy) + dz dz), and the hit is a back face iff ((nx dx + ny dy) + nz dz) > 0 with the
         record's float32 normal widened (the products are exact in double), else a front face.  The nearest hit of a class is the
         smallest dist, ties to the lowest j (a NaN distance is counted but is never the nearest); its distance is rounded to float32
         once.  A hit is classified by the normal the walk stored, whatever the shape: a ConstantMedium reports +Y, and counts as what
         that is for the ray.  One wave per probe, the lanes joined by a butterfly of (dist, j) minima and integer sums: no atomics, the
         result is a pure function of the inputs and does not depend on the launch geometry.
     Step (fw_probe_relocate_step, k_probe_relocate_step), per probe:  inside = (double)n_back > (double)back_fraction * (double)D;
         a' = inside ? 0 : 1 (the survey was taken at the current position, so a' classifies that position).  With move == 0 only a is
         written.  Otherwise the candidate c: if inside, c = o + u_back * (dist_back + 0.5 * min_front) with
         u = d / sqrt((dx dx + dy dy) + dz dz) per component; else if n_front > 0 and dist_front < min_front,
         c = o - u_front * (min_front - dist_front); else c = o.  Each component is rounded to float32 once.  If any |c_k| > max_offset_k
         (or c_k is not a number) the move is rejected, not clamped, and o' = o; otherwise o' = c.  A probe that needs a move it is not
         allowed stays where it is and comes out inactive at the classifying step.
     Placed lookup (fw_probe_irradiance_placed, fw_probe_shade_placed): fw_probe_irradiance's statement, or with depth maps
         fw_probe_irradiance_vis', with these changes.  (i) The corner's probe stands at P'_k = P_k + (double)o_k, used in the wrap term
         r = P' - p and the visibility term r' = q - P'; the cell and the trilinear weights stay the nominal grid's.  (ii) A corner whose
         a is 0 is skipped: its sh and moments never enter a sum, so a NaN there does not reach the output.  (iii) The weights of the
         remaining corners are always divided by their sum, added in the order dz, dy, dx.  (iv) No active corner, or a sum of 0, gives
         (0, 0, 0).  With every record (0, 0, 0, 1) the output equals the counterpart's bit for bit whenever the counterpart normalises
         (FW_PROBE_WRAP, or depth maps).  Without wrap and without depth the placed lookup differs from fw_probe_irradiance by the
         division in (iii) alone.  The sh and the depth maps are expected to have been baked at the moved positions: fw_probe_set takes
         arbitrary positions, so that is the caller's to do. */
typedef struct fw_probe_relocate {
    float min_front;          /* > 0, finite: a probe keeps at least this distance to the nearest front face */
    float back_fraction;      /* in [0, 1]: a probe that sees more than this share of back faces is inside geometry (DDGI: 0.25) */
    float max_offset[3];      /* >= 0, finite: the largest |offset| per axis, world units */
} fw_probe_relocate;

/* fw_probe_survey: overwrites survey (n_probes x 12 floats) from one round's rays (n_probes x D x 6 floats) and the hits fw_trace_rays
   wrote for them.  Host arrays — staged through one device allocation of the call's own, freed on every path — or with on_device
   device arrays on `device` (the kernel then works on the caller's memory), launched on `stream` and complete on return.  Errors, in
   this order and before HIP is called: FW_ERR_BAD_ARG for a NULL rays, hits or survey, n_probes == 0, directions outside 1..2^20, with
   on_device hits or survey not 16-byte aligned or rays not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31; then
   FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_probe_survey(int device, uint32_t n_probes, uint32_t directions, const float *rays, const fw_hit *hits, float *survey, int on_device,
                    void *stream);

/* fw_probe_relocate_step: one step over n_probes probes; survey is read, placement (n_probes x 4 floats) is read and written.  Host or
   device arrays as fw_probe_survey.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL rl, survey or placement,
   min_front not finite or <= 0, back_fraction outside [0, 1], a max_offset negative or not finite, n_probes == 0, directions outside
   1..2^20, with on_device survey or placement not 16-byte aligned; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the
   last one. */
int fw_probe_relocate_step(int device, const fw_probe_relocate *rl, uint32_t n_probes, uint32_t directions, const float *survey, float *placement,
                           int move, int on_device, void *stream);

/* fw_relocate_probes: the steps [first_step, first_step + steps) of a probe set against a resident scene, and then one classifying
   step (move = 0) at s = first_step + steps.  set->positions are the nominal positions; placement is n_probes x 4 floats in host
   memory always, read and written (start it at (0, 0, 0, 1)); survey is host memory, n_probes x 12 floats, the last step's, and may be
   NULL.  Of tp, use_bvh, flags, seed, rays_per_batch and stream are read.  For each step s: the moved positions
   float((double)pos_k + (double)o_k) are formed on the host; then for each chunk of probes [p0, p1) (set->chunk_probes at a time; 0 = as
   many as fit 256 MiB at 72 B per ray, at least 1) k_probe_rays fills device scratch of the call's own with round s over the moved
   positions, the rays are traced exactly as fw_trace_rays would with on_device = 1, key_base = p0 D and seed = tp->seed + s,
   k_probe_survey and k_probe_relocate_step run; the placement is copied back, 16 B per probe.  steps may be 0: classify only.
   Contracts.  Composition: for every chunk_probes, placement and survey equal bit for bit what fw_probe_rays (a set at the moved
   positions), fw_trace_rays (seed + s, key_base 0), fw_probe_survey and fw_probe_relocate_step give when chained by hand over the
   whole set.  Progressive: a call of (0, a) followed by one of (a, b) leaves the placement and survey of one call of (0, a + b), bit
   for bit.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, set, rl, tp or placement,
   what fw_probe_rays rejects in the set, what fw_probe_relocate_step rejects in rl, a placement entry that is not finite or whose a is
   neither 0 nor 1 (its index is in fw_last_error()), first_step + steps + 1 >= 2^32; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31; then
   FW_ERR_NO_DEVICE.
   stats (may be NULL): fw_trace_rays' fields summed over steps and chunks as fw_bake_probe_depth sums them; ms_render includes the three
   kernels' launches (under FW_FLAG_TIME_KERNELS ms_raygen and ms_accumulate as well); ms_wall covers the whole call.  Synchronisation
   and what a trace leaves of renders are fw_trace_rays'. */
int fw_relocate_probes(fw_scene *scene, const fw_probe_set *set, const fw_probe_relocate *rl, const fw_trace_params *tp, uint32_t first_step,
                       uint32_t steps, float *placement, float *survey, fw_stats *stats);

/* fw_probe_irradiance_placed, fw_probe_shade_placed: the placed lookup above (k_probe_irradiance and k_probe_shade with PLACED: one lane
   per point, no atomics).  The arguments are fw_probe_irradiance_vis' and fw_probe_shade_vis', and placement: n x 4 floats for the
   grid's n probes, host memory or with on_device device memory like sh; a host call stages it after the moments.  pd and moments may
   both be NULL: no visibility weight (normal_bias is then not read).  Every index is formed from clamped cell and texel indices: no
   load leaves the arrays wherever the point lies.  Errors: the counterpart's, in its order, with placement among the NULL checks and,
   with on_device, among the 4-byte alignment checks; exactly one of pd and moments NULL is FW_ERR_BAD_ARG. */
int fw_probe_irradiance_placed(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias,
                               const float *placement, int device, uint32_t n, const float *positions, const float *normals, uint32_t stride_floats,
                               float *irradiance, int on_device, void *stream);
int fw_probe_shade_placed(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias,
                          const float *placement, const fw_probe_shade_params *p, const float *aov, float *linear_rgb, float *gamma_rgb,
                          uint8_t *rgb8);

/* Probe radiance maps (additive at ABI 8).  Nine SH coefficients cannot hold a highlight, so every probe also gets an
   octahedral map of the radiance its rays saw, with a chain of GGX-prefiltered levels, which a lookup reads along a reflected
   direction.  Everything below is float64 arithmetic from the float32 inputs, every operation rounded as written; max and min are
   fmax and fmin; no atomics.  Texel centres, sgn, the fold and the bilinear fetch are fw_probe_depth's (above), at each level's own
   resolution.  api.probe_radiance_reduce, api.probe_radiance_prefilter, api.probe_radiance_lookup and api.probe_glossy_ref are the
   numpy statements.
     Layout.  Level l has resolution R_l = R >> l.  A probe's pyramid has M = sum_l R_l^2 texels; level l starts at texel sum_(i<l)
         R_i^2, and within a level texel (column a, row b) is b R_l + a.  maps: n_probes x M x 4 floats (r, g, b, flag), flag 1.0 where
         the texel has data, else 0.0.  sums: n_probes x R x R x 4 floats (A_r, A_g, A_b, W), all four written.  On the device both
         are 16-byte aligned.
     Reduction of one round (fw_probe_radiance_reduce, k_probe_radiance_reduce): fw_probe_depth_reduce with radiance in the place of
         distance.  For ray j of probe p, L_c = (double)accum[p D + j].c / samples, and per texel w = max(0, (Tx dx + Ty dy) + Tz dz)
         squared sharpness_log2 times.  A ray with !(w > 0) is skipped for that texel, so a NaN radiance reaches only the texels whose
         lobe it falls in.  Otherwise, sequentially in ascending j, A_c = A_c + w L_c and W = W + w.  Each accumulator is rounded to
         float32 once and added to sums with one float32 addition.  One lane owns a texel: the result is a pure function of the
         inputs and does not depend on the launch geometry.
     Prefilter (fw_probe_radiance_prefilter, k_probe_radiance_prefilter).  Level 0: float((double)A_c / W) with flag 1; a texel with
         W == 0 gets (0, 0, 0, 0).  Level 0 is not filtered: roughness[0] states what the raw lobe is taken to stand for.  Level
         l >= 1, output texel with centre direction T at resolution R_l:  a = (double)rho_l rho_l, a2 = a a; over the source texels s of
         level 0 in ascending id, with their stored float32 values: s is skipped if its flag is 0; c = (Tx Sx + Ty Sy) + Tz Sz, and s
         is skipped if !(c > 0); h = (1 + c) 0.5; den = h (a2 - 1) + 1; w = ((a2 / (den den)) c) omega_s with
         omega_s = (4 / (R R)) / ((len len) len), len the length of the source texel's (x, y, z) before normalisation (the octahedral
         map's Jacobian at the centre); Wt = Wt + w and A_c = A_c + w L_c.  The texel is float(A_c / Wt) with flag 1, or zeros if
         Wt == 0.  This is the split-sum prefilter with n = v = r: the GGX D times n.l, integrated over the map.
     Lookup (fw_probe_radiance_lookup, k_probe_radiance_lookup).  The corner weights are exactly the placed lookup's (above): always
         normalised, inactive corners skipped, wrap and visibility as there; placement NULL means every record is (0, 0, 0, 1), and pd
         and moments may both be NULL.  r = dirs / sqrt((x x + y y) + z z) per component.  rho = min(max(roughness, rho_0), rho_(L-1));
         l is the largest level with rho_l <= rho, capped at L - 2; t = (rho - rho_l) / (rho_(l+1) - rho_l).  Per active corner the rgb of
         levels l and l + 1 is fetched bilinearly along r as fw_probe_depth's moments are, at R_l and R_(l+1), edges clamped, the flags
         not read, and m = m_l (1 - t) + m_(l+1) t.  With L = 1 only level 0 is read and m = m_0.  Out_c = sum (w_d / wsum) m_c in the
         order dz, dy, dx, rounded to float32 once and not clamped.  Zeros for a non-finite position, normal, dir or roughness, a zero
         normal or dir, a point with no active corner, or a zero weight sum.  Every index is formed from clamped cell and texel
         indices, so no load leaves the arrays.  Out of scope: parallax correction — each probe is read along r itself, as if the
         reflected surface were infinitely far away.
     Glossy shade (fw_probe_shade_glossy, k_probe_shade_glossy).  spec: W H x 4 floats (F0.rgb, rho).  view: three floats per pixel at
         view_stride_floats, the ray direction from the eye (a ray buffer is read in place with the pointer rays + 3 and stride 6).  A
         pixel with !(rho > 0) gets fw_probe_shade_placed's output bit for bit (a NULL placement taken as neutral).  Otherwise, with nh
         the unit normal:  u = view / |view|;  c = (nhx ux + nhy uy) + nhz uz;  r_k = float(u_k - (2 c) nh_k);  cos = min(1, max(0, -c));
         m = 1 - cos;  S = ((m m) (m m)) m;  Ls = the lookup above at (position, normal, r, rho), rounded to float32, then max(., 0);
         S = 0 and Ls = 0 for a non-finite or zero view, a non-finite position or a non-finite or zero normal, and Ls = 0 wherever the
         lookup answers with zeros.  In float32 without contraction
         F_c = f0_c + (1 - f0_c) * (float)S and out_c = v * (F_c * Ls_c) + (1 - v) * a_c with v the record's coverage and a its albedo;
         the outputs are resolved as fw_probe_shade's.  A conductor has no diffuse lobe.  Simplification: the split sum's shadowing
         factor (the second, BRDF-integral term) is left out of this call; fw_probe_shade_split (below) is the same shade with that
         term, read from a table that fw_ggx_table bakes. */
#define FW_PROBE_RADIANCE_MAX_LEVELS 4
typedef struct fw_probe_radiance {
    uint32_t resolution;      /* R in {4, 8, 16, 32} */
    uint32_t sharpness_log2;  /* k in 0..8, as fw_probe_depth */
    uint32_t levels;          /* L >= 1; level l has resolution R >> l, and the last level's is >= 4 (R = 4: L = 1; R = 32: up to 4) */
    float    roughness[FW_PROBE_RADIANCE_MAX_LEVELS]; /* rho_l in [0, 1], strictly ascending over l < L; entries >= L are not read */
} fw_probe_radiance;

/* fw_probe_radiance_reduce: adds one round's reduction to the running sums.  rays: n_probes x D x 6 floats; accum: n_probes x D x 4
   floats as fw_render_rays leaves it (fw_probe_project's input); host arrays, or with on_device device arrays on `device`, launched
   on `stream` and complete on return.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL pr, rays, accum or
   sums, a resolution outside {4, 8, 16, 32}, sharpness_log2 > 8, levels == 0 or a last level below resolution 4, a roughness outside
   [0, 1] or not strictly ascending, n_probes == 0, directions outside 1..2^20, samples outside 1..2^24, with on_device sums or accum
   not 16-byte aligned or rays not 4-byte aligned; FW_ERR_UNSUPPORTED for n_probes x D >= 2^31 or n_probes x R^2 >= 2^31; then
   FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index out of range. */
int fw_probe_radiance_reduce(int device, const fw_probe_radiance *pr, uint32_t n_probes, uint32_t directions, uint32_t samples, const float *rays,
                             const float *accum, float *sums, int on_device, void *stream);

/* fw_probe_radiance_prefilter: overwrites maps from sums.  Errors, in this order: FW_ERR_BAD_ARG for a NULL pr, sums or maps, what
   fw_probe_radiance_reduce rejects in pr, n_probes == 0, with on_device arrays not 16-byte aligned; FW_ERR_UNSUPPORTED for
   n_probes x M >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index out of range. */
int fw_probe_radiance_prefilter(int device, const fw_probe_radiance *pr, uint32_t n_probes, const float *sums, float *maps, int on_device,
                                void *stream);

/* fw_bake_probe_radiance: fw_bake_probes' loop — the same rays, the same frames, the same seeds rp->seed + r with key_base = p0 D — with
   k_probe_radiance_reduce on each chunk and, at the end, one prefilter of the final sums into maps (may be NULL).  With sh_sums or sh
   not NULL the same rendered accum also goes through k_probe_project: one render feeds both bakes.
     sums   : n_probes x R x R x 4 floats, the running sums of the rounds [0, first_round); NULL only when first_round == 0.
     sh_sums, sh : fw_bake_probes' sums and sh; sh_sums may be NULL with first_round == 0 (sh is then still written).
   Contracts, bit for bit and for every chunk_probes.  Composition: sums equals fw_probe_rays, fw_render_rays and
   fw_probe_radiance_reduce chained by hand.  sh_sums and sh equal what fw_bake_probes gives for the same arguments.  Progressive: k
   calls of n rounds equal one call of k n rounds.  fw_render is left as it was.
   Errors: fw_bake_probes', in its order, with pr's after the set's; a NULL sums with first_round > 0, and, when sh_sums or sh is given,
   a NULL sh_sums with first_round > 0; with on_device sums or maps not 16-byte aligned, sh_sums or sh not 4-byte aligned;
   FW_ERR_UNSUPPORTED for n_probes x D >= 2^31 or n_probes x M >= 2^31; then FW_ERR_NO_DEVICE.  stats: as fw_bake_probes; the
   prefilter's time is part of ms_render (and of ms_accumulate under FW_FLAG_TIME_KERNELS). */
int fw_bake_probe_radiance(fw_scene *scene, const fw_probe_set *set, const fw_probe_radiance *pr, const fw_render_rays_params *rp,
                           uint32_t first_round, uint32_t rounds, float *sums, float *maps, float *sh_sums, float *sh, fw_stats *stats);

/* fw_probe_radiance_lookup: the lookup above at n points (one lane per point, 16-byte texel loads, no LDS).  positions and normals at
   stride_floats; dirs n x 3 and roughness n, packed; radiance n x 3.  Host arrays, or with on_device device arrays.  Errors: the placed
   lookup's in its order, with pr, maps, dirs and roughness among the NULL checks, pr's own checks before pd's, maps 16-byte aligned
   with on_device, and FW_ERR_UNSUPPORTED for n_probes x M >= 2^31. */
int fw_probe_radiance_lookup(const fw_probe_grid *grid, const fw_probe_radiance *pr, const float *maps, const fw_probe_depth *pd, const float *moments,
                             float normal_bias, const float *placement, int device, uint32_t n, const float *positions, const float *normals,
                             uint32_t stride_floats, const float *dirs, const float *roughness, float *radiance, int on_device, void *stream);

/* fw_probe_shade_glossy: the glossy shade above over fw_probe_shade_placed's arguments (placement may be NULL).  Errors: its
   counterpart's in its order, with pr, maps, spec and view among the NULL checks, view_stride_floats < 3 after gamma, and with on_device
   spec and maps 16-byte aligned like aov. */
int fw_probe_shade_glossy(const fw_probe_grid *grid, const float *sh, const fw_probe_radiance *pr, const float *maps, const fw_probe_depth *pd,
                          const float *moments, float normal_bias, const float *placement, const fw_probe_shade_params *p, const float *aov,
                          const float *spec, const float *view, uint32_t view_stride_floats, float *linear_rgb, float *gamma_rgb, uint8_t *rgb8);

/* ---- the split sum's BRDF term: a GGX albedo table (additive at ABI 8) -------------------------------------------------
   FW_MAT_GGX's directional albedo at the cosine mu of the view and the roughness rho is F0 A + B per channel, with two numbers
   (A, B) that depend on (mu, rho) alone: fw_ggx_terms integrates them, fw_ggx_table lays them out over (mu, rho), fw_ggx_table_lookup
   reads the table, and fw_probe_shade_split is fw_probe_shade_glossy with F0 A + B in the place of the bare Schlick term.  Everything
   is float64 from the float32 inputs, every operation rounded as written (no contraction), max and min are fmax and fmin, one rounding
   to float32 at the end.  api.ggx_terms, api.ggx_table, api.ggx_table_lookup and api.probe_split_ref are the numpy statements.
     Terms at (mu, rho), mu in (0, 1], rho in [0, 1]; zeros for a mu or rho outside its range or not finite.  alpha = the float32 product
         rho rho, widened (as FW_MAT_GGX forms it), a2 = alpha alpha.  wo = (sx, 0, mu) with sx = sqrt(max(1 - mu mu, 0)).  The visible
         normal is FW_MAT_GGX's (Heitz 2018, above) for this wo:  vx = alpha sx;  vl = sqrt(vx vx + mu mu);  Vh = (vhx, 0, vhz) = (vx / vl,
         0, mu / vl);  T1 = (0, 1, 0), which is (-Vh.y, Vh.x, 0) / |.| wherever that exists and as good a tangent as any where it does not
         (Vh = z);  T2 = Vh x T1 = (-vhz, 0, vhx);  s = 0.5 (1 + vhz);  Lo = 0.5 (sqrt(1 + a2 ((sx sx) / (mu mu))) - 1).
         Sample (a, b), a < m1, b < m2:  xi1 = (a + 0.5) / m1, xi2 = (b + 0.5) / m2 — midpoints of the visible-normal square, so that the
         integrand is continuous at the horizon, where Lambda(wi) grows without bound;  r = sqrt(xi1);  phi = (2 pi) xi2;  p1 = r cos phi;
         q1 = 1 - p1 p1;  p2 = (1 - s) sqrt(max(q1, 0)) + s (r sin phi);  nz = sqrt(max(q1 - p2 p2, 0));  nh = (nz vhx - p2 vhz, p1,
         p2 vhx + nz vhz);  g = (alpha nh.x, alpha nh.y, max(nh.z, 0));  h = g / sqrt((g.x g.x + g.y g.y) + g.z g.z);  oh = sx h.x + mu h.z;
         wi = ((2 oh) h.x - sx, (2 oh) h.y, (2 oh) h.z - mu).  Where wi.z > 0:  Li = 0.5 (sqrt(1 + a2 ((wi.x wi.x + wi.y wi.y) / (wi.z
         wi.z))) - 1) and k = (1 + Lo) / ((1 + Lo) + Li) — the renderer's attenuation F G2 / G1 without F;  elsewhere k = 0.
         m = max(1 - oh, 0) (the max guards a rounding of oh past 1);  Fc = ((m m) (m m)) m;  the sample's terms are k (1 - Fc) and k Fc.
         Sum: sample id = a m2 + b.  Lane l of 256 adds the terms of the samples l, l + 256, ... in ascending order from 0.0.  The 256
         partials are added by a fixed tree: within each run of 64 lanes, for d = 32, 16, 8, 4, 2, 1 every lane takes v = v + v[lane
         xor d] (all 64 then hold one value); the four runs' values are added as ((w0 + w1) + w2) + w3.  A and B are those sums
         divided by the product (double)m1 (double)m2.  The albedo of a material is F0 A + B; E1 = A + B is that of a white one.
     fw_ggx_quad = { m1 in 1..1024, m2 in 1..1024 }; the default is 128 x 128.  Against the same rule at 2048 x 2048 the terms differ by
         at most 6.5e-3 at 64 x 64, 8.8e-4 at 128 x 128 and 5.5e-4 at 256 x 256 over mu in {1/64, 0.1, 0.5, 0.99} x rho in {1/64, 0.05,
         0.1, 0.3, 0.6, 1}; xi1 is the dimension that matters.
     Table.  n_mu and n_rho in 2..256.  Texel (i, j) holds the terms at the centres mu_i = float((i + 0.5) / n_mu) and rho_j =
         float((j + 0.5) / n_rho), both divisions in float64.  table[j][i] = (A, B): n_rho x n_mu x 2 floats.  fw_ggx_table equals
         fw_ggx_terms at those centres bit for bit.
     Lookup at (mu, rho):  x = min(max(mu n_mu - 0.5, 0), n_mu - 1);  i0 = min((int)x, n_mu - 2);  tx = x - i0;  likewise y, j0 and ty
         from rho and n_rho;  out = ((t00 (1 - tx) + t10 tx) (1 - ty)) + ((t01 (1 - tx) + t11 tx) ty) per component with t10 the texel
         (i0 + 1, j0) and t01 the texel (i0, j0 + 1), rounded to float32 once.  Zeros for a non-finite mu or rho.  Every index lies in
         the table whatever mu and rho hold.  At a texel centre of a power-of-two size x = i exactly and the texel's bits come back.
         No division, root or transcendental: a device is expected to equal numpy bit for bit.
     Split shade (fw_probe_shade_split, k_probe_split_shade).  fw_probe_shade_glossy's arguments, the table, its sizes and flags.  A
         pixel with !(rho > 0) gets fw_probe_shade_placed's output bit for bit.  A glossy pixel forms u, c, r and Ls exactly as the
         glossy shade above;  mu_f = float(min(1, max(0, -c))), and 0 for a non-finite or zero view, a non-finite position or a
         non-finite or zero normal;  (A, B) = the lookup at (mu_f, rho).  Then in float32 without contraction:  spec_c = f0_c * A + B;
         with FW_SPLIT_ENERGY:  E1 = A + B,  g = (E1 > 0) ? 1 / E1 - 1 : 0,  spec_c = spec_c * (1 + f0_c * g) — the usual single-lobe
         compensation: a white conductor returns all the light it receives; without the flag nothing is multiplied;
         out_c = v * (spec_c * Ls_c) + (1 - v) * a_c.  The outputs are resolved as fw_probe_shade's. */
#define FW_SPLIT_ENERGY 1u
typedef struct fw_ggx_quad {
    uint32_t m1, m2; /* samples of xi1 and of xi2, each in 1..1024 (default 128 x 128) */
} fw_ggx_quad;

/* fw_check_ggx_quad: FW_OK, or FW_ERR_BAD_ARG for, in this order: a NULL quad; m1 outside 1..1024; m2 outside 1..1024.  Touches no
   device. */
int fw_check_ggx_quad(const fw_ggx_quad *quad);

/* fw_ggx_terms: terms[q] = (A, B) at (mu[q], rho[q]), q < n (one workgroup per pair; a pair's terms do not depend on the batch).
   Host arrays — through device scratch of the call's own, freed on every path — or with on_device device arrays on `device`, launched
   on `stream` and complete on return; terms (n x 2 floats) is overwritten.  Errors, in this order and before HIP is called:
   FW_ERR_BAD_ARG for a NULL quad, mu, rho or terms; fw_check_ggx_quad's refusals; n == 0; with on_device terms not 8-byte aligned or
   mu or rho not 4-byte aligned; then FW_ERR_NO_DEVICE without a GPU (terms untouched), and FW_ERR_BAD_ARG for a device index out of
   range. */
int fw_ggx_terms(const fw_ggx_quad *quad, int device, uint32_t n, const float *mu, const float *rho, float *terms, int on_device, void *stream);

/* fw_ggx_table: the n_rho x n_mu x 2 floats of the table, host memory or with on_device device memory, as fw_ggx_terms; overwritten.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL quad or table; fw_check_ggx_quad's refusals; n_mu or n_rho
   outside 2..256; with on_device table not 8-byte aligned; then FW_ERR_NO_DEVICE (table untouched), and FW_ERR_BAD_ARG for a device
   index out of range. */
int fw_ggx_table(const fw_ggx_quad *quad, int device, uint32_t n_mu, uint32_t n_rho, float *table, int on_device, void *stream);

/* fw_ggx_table_lookup: terms[q] = the lookup above of `table` at (mu[q], rho[q]), q < n (one lane per pair, four 8-byte loads).  Host
   arrays or with on_device device arrays, as fw_ggx_terms.  Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL
   table, mu, rho or terms; n_mu or n_rho outside 2..256; n == 0; with on_device table or terms not 8-byte aligned or mu or rho not
   4-byte aligned; then FW_ERR_NO_DEVICE (terms untouched), and FW_ERR_BAD_ARG for a device index out of range. */
int fw_ggx_table_lookup(int device, uint32_t n_mu, uint32_t n_rho, const float *table, uint32_t n, const float *mu, const float *rho, float *terms,
                        int on_device, void *stream);

/* fw_probe_shade_split: the split shade above.  Errors: fw_probe_shade_glossy's in its order, with table among the NULL checks, then
   n_mu or n_rho outside 2..256 and flags with an unknown bit straight after the NULL checks, and with on_device table 8-byte aligned. */
int fw_probe_shade_split(const fw_probe_grid *grid, const float *sh, const fw_probe_radiance *pr, const float *maps, const fw_probe_depth *pd,
                         const float *moments, float normal_bias, const float *placement, const fw_probe_shade_params *p, const float *aov,
                         const float *spec, const float *view, uint32_t view_stride_floats, const float *table, uint32_t n_mu, uint32_t n_rho,
                         uint32_t flags, float *linear_rgb, float *gamma_rgb, uint8_t *rgb8);

/* Diagnostic: the kernels' division / square-root helpers against the compiler's IEEE expansion, bit for bit,
   on n hashed operand pairs.  mode 0 = magnitudes 2^-40..2^40 (must be 0 mismatches), mode 1 = all bit patterns. */
int fw_selftest_arith(int device, uint32_t n, uint32_t seed, int mode, uint64_t *div_mismatches, uint64_t *sqrt_mismatches);

/* Diagnostic: the libm-class functions of the path (firework_amd/csrc/fw_libm.h: glibc's logf, log10f, sinf, asinf, acosf,
   atanf, atan2f, powf restated for the device) evaluated on the device, element-wise, on host arrays: out[i] = fn(x[i] [, y[i]]).
   fn: 0 logf  1 log10f  2 sinf  3 asinf  4 acosf  5 atanf  6 atan2f(x[i], y[i]) = atan2(first, second)  7 powf(x[i], y[i]).
   y may be NULL for the one-argument functions.  tests/test_gpu_libm.py compares the results with the host's libm bit for bit. */
int fw_selftest_libm(int device, int fn, uint32_t n, const float *x, const float *y, float *out);

/* Runtime options.  The library reads the environment variables FIREWORK_<NAME> ONCE, when it is loaded; nothing on the render path
   looks at the environment.  fw_set_option changes one option afterwards (name with or without the FIREWORK_ prefix; value NULL =
   back to the default; name NULL = back to what the environment said at load time) and applies to the scenes created and the renders
   started after it returns.  Results never depend on an option — only which kernels produce them (every pair of settings is
   compared bit for bit in tests/) — except the diagnostics NO_EXACT / EXACT_ALL.  Names:
     BVH=median            walk the reference's own median-split topology instead of the SAH tree (parity / A-B mode)
     WIDE=0|f32|q8         no wide nodes (the pair-node kernels) / force an encoding of the wide nodes
     BUILD=host|device     where a scene's trees are built: the host builders, or their restatement on the device (the same nodes bit for
                           bit); default: the device for a tree of 100 000 items or more.  Other values: FW_ERR_BAD_ARG
     EXACT_ALL=1, NO_EXACT, EXACT_FORM=lane|wave      every ray / no ray through the literal reference walk; its form
     STREAMS=n, WAVES=n, PATHS_PER_BATCH=n            batches in flight, wave queues, pool size
     NO_DEFER NO_HIT4 NO_HOIST NO_LDS_TABLES NO_LDS_TREES NO_LDS_TRIS NO_SHORT_RAYS NO_TILE_ORDER NO_ZERO_SKIP
     DEP_PIXEL_MAJOR DEP_SLOT_MAJOR NO_CHAIN          the layout choices the tests force both ways
     EXACT_PRODUCT=1       scenes with a varying texture keep every scattering's attenuation (16 B per segment) and multiply back to front when
                           a path deposits — render.rs:23-28's own association, the pre-gamma means then equal the CPU oracle's bit for bit
                           (scenes of constant textures always do: their 8-byte chain state).  Default off: the running product, ~1 ulp away
     PHASE_LOCK=0|1        the two batches in flight tied in anti-phase by one event per segment (default: big box-list batches)
     FUSE_SEGMENTS=0|1     1: a box-list batch's segments in one launch (k_segments_boxlist) where the frame is eligible; the frame is the
                           unfused frame bit for bit.  Default off
     GRAPH=0|1             a frame asked for twice in a row is captured into a hipGraph and replayed from then on (default: frames of
                           small batches, whose launches are short); fw_stats.reserved bit 31 reports a replay
     TRACE, DUMP_PATH=file                            host-side timing trace; one path's records (tools/diverge.py)
   Returns FW_ERR_BAD_ARG for a name this build does not know. */
int fw_set_option(const char *name, const char *value);

/* Diagnostic (additive at ABI 8): which walk and shade kernels the last call on `device` launched.  The library picks one
   of about a hundred kernel instantiations from the scene's sizes and the options above; every launch of one records its id, and this
   call writes the recorded names to buf, sorted and separated by commas — names such as k_shade_pl<2,0>, k_extend_linear_defer<true>,
   k_shadow_resolve_env; the walks that keep their tree in LDS carry their waves per workgroup: k_blas_wide<q8,no tris>@12,
   k_extend_tlas_wide<true,true>@16, k_blas_lds<true>@16 (a comma inside <> belongs to a name).  The set is cleared when fw_render,
   fw_render_progressive, fw_render_adaptive, fw_render_aovs, fw_trace_rays or a pass of fw_render_views, fw_render_rays, fw_render_model or
   a bake starts its work on the device, so after a call of several passes it is the last pass's (an adaptive call: all its rounds').  A
   frame replayed as a hipGraph (option GRAPH) runs no launcher: it reports the set recorded while the graph was captured.  device = -1:
   every name this build can launch, without the wave counts (no device is needed).  At most cap - 1 characters and a terminator are
   written (nothing for cap = 0, where buf may be NULL); returns the length of the whole list, as snprintf does, or FW_ERR_BAD_ARG
   (device < -1 or out of range, buf = NULL with cap > 0).  No HIP call is made. */
int fw_debug_kernels(int device, char *buf, uint32_t cap);

/* Diagnostic, CPU only: builds the WIDE nodes the LDS-resident walks step through (four children per node; format 1 = f32 planes,
   2 = planes quantised to 8 bits and rounded outward) over n item boxes (n x 6 floats: min.xyz max.xyz) and checks the finished
   tree: every item the leaf of exactly one slot, every child box as the device decodes it a superset of the exact one (f32: the
   item's own box bit for bit), free slots unhittable.  violations = 0 is the only acceptable answer; stats = nodes, leaves,
   free slots, depth. */
int fw_selftest_wide_bvh(const float *boxes, uint32_t n, int format, uint32_t *violations, uint32_t stats[4]);

/* Diagnostic, CPU only (ABI v7): the host-side tree builders over n item boxes (n x 6 floats) with `threads` host threads — the reference's
   median-split tree (bvh.rs:21-71: what fixes tie ranks and gate boxes) and the binned-SAH tree the device walks.  hashes = FNV-1a of the
   two node arrays, stats = nodes and depth of the median tree, nodes and depth of the SAH tree.  Scene creation builds a mesh's trees in
   parallel (the reference builds inside its timed region, main.rs:40-44, on one thread); any thread count must give the one-thread trees. */
int fw_selftest_bvh_build(const float *boxes, uint32_t n, int threads, uint64_t hashes[2], uint32_t stats[4]);

/* Diagnostic: the same two trees over n item boxes (n x 6 floats), built on GPU `device` by the device builders, or by the host builders
   for device = -1.  ref_nodes / sah_nodes receive the node arrays of the median-split and the SAH tree (8 floats per node: min.xyz, A,
   max.xyz, B; depth-first order; at most (2n - 1) x 8 floats each); stats = nodes and depth of each, as fw_selftest_bvh_build gives them.
   The device's trees equal the host's bit for bit.  Errors: FW_ERR_BAD_ARG (n = 0, a null pointer, device < -1 or out of range),
   FW_ERR_NO_DEVICE (device >= 0 without a GPU), FW_ERR_NAN_BBOX (a centre the median tree compares is NaN), FW_ERR_OOM, FW_ERR_HIP. */
int fw_selftest_bvh_trees(int device, const float *boxes, uint32_t n, float *ref_nodes, float *sah_nodes, uint32_t stats[4]);

/* Diagnostic, CPU only: the sampled lights of a description as FW_FLAG_LIGHT_SAMPLING sees them, in object order, FW_LIGHT_RECORD_FLOATS
   floats each: object index, shape kind (FW_SHAPE_SPHERE / _XYRECT / _XZRECT / _YZRECT), then a rectangle's four world corners (12 floats;
   rotated only where the reference intersects the object rotated, cos_trace < 0.999) or a sphere's centre and radius (4 floats, 8 zeros),
   the area and p_pick (1 / number of lights).  *n = the number of lights; at most cap records are written.  Errors: FW_ERR_BAD_ARG (null
   desc or n, out = NULL with cap > 0). */
#define FW_LIGHT_RECORD_FLOATS 16
int fw_selftest_lights(const fw_scene_desc *desc, float *out, uint32_t cap, uint32_t *n);

/* Diagnostics (GPU): the FW_FLAG_ENV_SAMPLING table of a caller's w x h map (rgb: w h x 3 floats, row-major from the top row, as
   fw_environment.hdr_rgb), built on `device` as a render builds it.  fw_selftest_env_dist: p = the w h per-texel probabilities (float32 of
   the float64 table), *total = the total weight sum(max(r, g, b) x Omega_row).  fw_selftest_env_sample: n samples drawn as a segment-0
   vertex of pixel i with seed32 = seed would draw them, FW_ENV_SAMPLE_FLOATS floats each: the direction (xyz), the reported density (per
   steradian, of the texel the direction looks up), the drawn texel's index and the looked-up texel's index.  Errors: FW_ERR_BAD_ARG (null
   pointers, w h = 0 or above 2^24, n = 0 or above 2^26, for sampling a map of zero total weight), FW_ERR_NO_DEVICE, FW_ERR_HIP. */
#define FW_ENV_SAMPLE_FLOATS 6
int fw_selftest_env_dist(int device, const float *rgb, uint32_t w, uint32_t h, float *p, double *total);
int fw_selftest_env_sample(int device, const float *rgb, uint32_t w, uint32_t h, uint32_t n, uint32_t seed, float *out);

/* Diagnostic, CPU only: the entries of a description as FW_FLAG_ALL_EMITTERS sees them, in object order and within an object
   in primitive order, FW_EMITTER_RECORD_FLOATS floats each: object index, primitive (a Rect3d's face 0-5, a mesh's triangle), shape kind,
   area (object space) and weight (area x power), computed in float64 and rounded to float32.  An object of power 0 (a black emitter) has
   no entries; a primitive of area 0 is listed with weight 0 and never picked.  *n = the number of entries (it may exceed 2^26, which a render refuses); at most cap records are written.  Errors:
   FW_ERR_BAD_ARG (null desc or n, out = NULL with cap > 0). */
#define FW_EMITTER_RECORD_FLOATS 5
int fw_selftest_emitters(const fw_scene_desc *desc, float *out, uint32_t cap, uint32_t *n);
/* Diagnostic (GPU): n picks of the scene's FW_FLAG_ALL_EMITTERS table (built here if no render has built it yet) from the world point x
   (3 floats), pick i drawn as a segment-0 vertex of pixel i with seed32 = seed would draw it, FW_EMITTER_SAMPLE_FLOATS floats each: the
   entry index (the float's bits are the uint32), the entry's pick probability as the table stores it, the sampled point's p_omega from x,
   the sampled world point (xyz) and the point in the object's frame (xyz).  Errors: FW_ERR_BAD_ARG (null pointers, n = 0 or above 2^26),
   FW_ERR_UNSUPPORTED (no entry of positive weight, or more than 2^26 entries), FW_ERR_HIP. */
#define FW_EMITTER_SAMPLE_FLOATS 9
int fw_selftest_emitter_sample(fw_scene *scene, const float *x, uint32_t n, uint32_t seed, float *out);
/* Diagnostic (GPU): n FW_MAT_GGX vertices through the device functions the shade kernels call.  in: FW_GGX_IN_FLOATS per entry: the unit
   normal (xyz), the incoming ray's direction (xyz, any length), roughness, F0 (rgb), xi1, xi2, and a direction omega (xyz, normalised here)
   to evaluate.  out: FW_GGX_OUT_FLOATS per entry: the sampled wi (xyz, world space), the attenuation (rgb; 0 where not alive), alive (1 or
   0), f cos(omega) (rgb) and p_b(omega).  Ranges are not checked (roughness^2 is taken as it comes).  Errors: FW_ERR_BAD_ARG (null pointers,
   n = 0 or above 2^24, device out of range), FW_ERR_NO_DEVICE, FW_ERR_HIP. */
#define FW_GGX_IN_FLOATS 15
#define FW_GGX_OUT_FLOATS 11
int fw_selftest_ggx(int device, uint32_t n, const float *in, float *out);

/* ---- final gather: gather rays lit from baked probes (additive at ABI 8) ------------------------------------------------
   The classic consumer of an irradiance cache.  A probe lookup at the receiver cannot change faster than the probe spacing; one bounce of
   cosine-weighted gather rays from the receiver can: each ray brings back the emission of the emitter it hit, the environment where it
   missed, or hit albedo x E(hit point) / pi with E read from the probes at the hit, where the probes' blur no longer shows.  Three calls:
   fw_hit_surface evaluates the material at a caller's hits (what fw_trace_rays leaves out), fw_gather_reduce sums the rays' radiance per
   receiver, fw_bake_gather chains rays, trace, surface, probe lookup, optionally the delta lights and the reduction.  api.surface_facing,
   api.gather_reduce and api.gather_resolve are the numpy statements.
     Surface record (fw_hit_surface, k_hit_surface): 16 floats (64 B) per ray,
           (albedo.xyz, kind) (facing normal.xyz, distance) (position.xyz, 0) (emitted.xyz, 0):
         the normal at floats 4..6 and the position at floats 8..10 as in fw_render_aovs' records, so every point reader reads them in place
         with stride 16.  All arithmetic is IEEE float32 without contraction; len(v) = sqrt((x x + y y) + z z).
         - A ray with a non-finite component or an all-zero direction — fw_trace_rays never traces it: kind = -2, every other float 0.
         - A miss (object == FW_NO_HIT): kind = -1, emitted = the environment along d / len(d), not clamped; every other float 0.
         - A hit whose material is not below the scene's material count, or whose object is not below its object count: kind = -2, every
           other float 0.  No load leaves the scene's tables, whatever the hit records hold.
         - A hit: kind = the material's kind (FW_MAT_*, 0..5) as a float.  albedo: the texture at (u, v, point) for Lambertian and
           Isotropic, the albedo for Metal, F0 for FW_MAT_GGX, (1, 1, 1) for Dielectric, (0, 0, 0) for Emissive, which never scatters.
           emitted: the texture at (u, v, point) for Emissive, not clamped; 0 otherwise.  distance = t x len(d); position = point;
           normal = n / len(n) with n the hit's normal as stored, (0, 0, 0) if that length is 0, negated when (nx dx + ny dy) + nz dz > 0:
           it faces the side the ray arrived from.
     Reduction of one round (fw_gather_reduce, k_gather_reduce): float64 from the float32 inputs, every operation rounded as written.  For
         ray j of point q with its surface record s, the irradiance E at it (3 floats) and, with `direct`, the record Ed (fw_bake_direct's
         out, 8 floats, floats 0..2 read): kind -2 contributes nothing; kind -1 L = s.emitted and sky += 1; kind 3 (Emissive) L =
         s.emitted; any other kind T_c = (E_c > 0 ? E_c : 0) (+ Ed_c with direct) and L_c = (s.albedo_c x T_c) x (1 / pi), 1 / pi the
         float64 quotient.  Four float64 accumulators (L.rgb, sky) in k_ao_reduce's order: with G = the smallest power of two >= min(D, 64),
         partial sum l takes j = l, l + G, ... in ascending order from 0, and the G partial sums are added by an xor butterfly over the
         distances G/2 ... 1 (x_l <- x_l + x_(l xor m)).  L is multiplied by the float64 pi / D — the rays are cosine-weighted, so the
         receiver's irradiance is pi times the mean radiance — and sky by the float64 1 / D; each is rounded to float32 once and added with
         one float32 addition to sums[id] = (Er, Eg, Eb, sky), indexed by id as fw_ao_reduce indexes its own.  No atomics; two runs are
         bit-equal; a point's result depends on no other point.
     Resolve (k_gather_resolve), R = the number of rounds in sums: out[id] = float((double)sums[id] / R) for the four floats.  An unusable
         point resolves to zeros. */

/* fw_hit_surface: the surface records of n rays and the hits fw_trace_rays wrote for them on this scene.  rays n x 6 floats, hits n
   records, surface n x 16 floats; host arrays — staged through one device allocation of the call's own, freed on every path — or with
   on_device device arrays on the scene's device, evaluated on `stream` (which waits for the scene's upload) and complete on return.
   Errors, in fw_trace_rays' pattern and before the scene is looked at: FW_ERR_BAD_ARG for a NULL scene; n == 0 returns FW_OK and writes
   nothing; FW_ERR_BAD_ARG for NULL rays, hits or surface, rays not 4-byte aligned, with on_device hits or surface not 16-byte aligned;
   then FW_ERR_NO_DEVICE. */
int fw_hit_surface(fw_scene *scene, const float *rays, const fw_hit *hits, uint32_t n, float *surface, int on_device, void *stream);

/* fw_gather_reduce: adds one round's reduction to the running sums.  surface: n x D records; irradiance: n x D x 3 floats, the probe
   lookup at those records; direct: n x D x 8 floats or NULL; sums: records of 16 B indexed by id.  Host or device arrays as fw_ao_reduce.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL surface, irradiance or sums; directions outside 1..2^20;
   n == 0; with on_device sums or surface not 16-byte aligned, irradiance, direct or ids not 4-byte aligned; FW_ERR_UNSUPPORTED for
   n x D >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_gather_reduce(int device, uint32_t directions, uint32_t n, const uint32_t *ids, const float *surface, const float *irradiance,
                     const float *direct, float *sums, int on_device, void *stream);

#define FW_GATHER_DIRECT 1u   /* add the scene's point, spot and directional lights at the gather hits */
#define FW_GATHER_NO_LIGHTS 4u   /* the complement of fw_bake_area: a gather ray that hits one of the scene's sampled area lights (fw_scene_area_lights)
                                    brings back nothing — between steps 3 and 4 k_area_mask (fw_area_mask) rewrites those records of the chunk to
                                    kind -2.  Bit 2 is unassigned and refused. */
#define FW_GATHER_NO_EMITTERS 16u   /* the complement of fw_bake_emitters: k_area_mask runs over the ascending objects that have an entry in
                                       fw_scene_emitters' list in place of the sampled area lights' objects.  Together with
                                       FW_GATHER_NO_LIGHTS: FW_ERR_BAD_ARG ("gather flags").  Bits 2 and 8 stay unassigned and refused. */
typedef struct fw_gather {
    uint32_t directions;     /* D, 1..2^20 */
    uint32_t jitter;         /* fw_ao's */
    float    bias;           /* gather-ray origin offset along the receiver's normal, >= 0, finite */
    float    direct_bias;    /* fw_direct.bias for the shadow rays at the gather hits */
    uint32_t flags;          /* FW_GATHER_DIRECT | FW_GATHER_NO_LIGHTS or FW_GATHER_NO_EMITTERS */
    uint32_t chunk_points;   /* 0: as many as fit 256 MiB at this call's bytes per ray (148, plus Ln x 72 + 64 with direct), at least one */
    uint64_t seed;
} fw_gather;

/* fw_bake_gather: the rounds [first_round, first_round + rounds) of the n points against a resident scene and a baked probe grid.  Points,
   ids, sums, out, first_round / rounds and what is read of tp are fw_bake_ao's.  For each round r and each chunk of points [q0, q1)
   (chunk_points at a time), in device scratch that the call allocates and frees on every path:
     1. k_ao_rays with fw_ao{D, falloff 0, radius +inf, bias, jitter, seed}: fw_ao_rays' rays bit for bit;
     2. the trace, as fw_bake_ao runs it: on_device, seed = tp->seed + r, key_base = q0 D;
     3. k_hit_surface over the chunk's rays and hits;
     4. the probe lookup at the records read in place (stride 16, positions = rec + 8, normals = rec + 4): with placement
        fw_probe_irradiance_placed's (pd and moments both NULL: without visibility), else with pd fw_probe_irradiance_vis', else
        fw_probe_irradiance's — the bits of that public call on those records;
     5. with FW_GATHER_DIRECT on a scene that has lights (Ln of them): fw_bake_direct's kernels, one round, over the same records — lobe 0,
        face_view 0, bias = direct_bias, no ids, view or spec — the shadow rays traced after the gather rays' trace has returned, with
        seed = tp->seed + r and a key base that gives entry e = q D + j (q counted in the whole call) and light i the key e Ln + i: what
        fw_bake_direct gives when called by hand over all n D records with tp->seed + r, whatever the chunking.  Without the flag or
        without lights the step does not run and the reduction reads no direct records;
     6. k_gather_reduce into sums.
   After the last round k_gather_resolve writes out.  On an error the stream is drained.
     sums: the running sums (Er, Eg, Eb, sky) of the rounds [0, first_round), NULL only when first_round == 0;  out: sums / rounds so far:
           the irradiance gathered at the point and the share of its rays that saw the environment; may be NULL.
   Contracts.  Composition: for every chunk_points, sums equals bit for bit what the public calls give when chained by hand over all n
   points: fw_ao_rays, fw_trace_rays, fw_hit_surface, the lookup, (fw_bake_direct,) fw_gather_reduce.  Progressive: k calls of m rounds
   leave the sums and out of one call of k m rounds, bit for bit.  Renders, and the frame graph's key, are left as fw_trace_rays leaves
   them.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, g, tp, positions or normals;
   directions outside 1..2^20, a bias or direct_bias negative or not finite; n == 0; stride_floats < 3; rounds == 0; first_round + rounds
   >= 2^32; a NULL sums with first_round > 0; with on_device sums or out not 16-byte aligned, positions, normals or ids not 4-byte
   aligned; then fw_probe_irradiance_placed's checks of grid, sh, pd, moments, normal_bias and (with on_device) the tables' alignment;
   unknown flag bits; FW_ERR_UNSUPPORTED for n x D >= 2^31 and the tables' sizes; then FW_ERR_NO_DEVICE; then — Ln is the scene's —
   FW_ERR_UNSUPPORTED for n x D x Ln >= 2^31.
   stats (may be NULL): fw_bake_ao's, summed over both traces; the shadow rays' trace lies inside the reduction's span of ms_render (and
   of ms_accumulate under FW_FLAG_TIME_KERNELS).  Synchronisation and what a trace leaves of renders are fw_trace_rays'. */
int fw_bake_gather(fw_scene *scene, const fw_gather *g, const fw_trace_params *tp,
                   const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias, const float *placement,
                   uint32_t n, const float *positions, const float *normals, uint32_t stride_floats, const uint32_t *ids,
                   uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats);

/* ---- reflection gather: GGX-sampled reflection rays lit from baked probes (additive at ABI 8) --------------------------
   The specular counterpart of the final gather.  fw_probe_shade_glossy reads each probe's radiance map along the mirrored direction as
   if the reflected surface were infinitely far away; a reflection ray from the receiver meets what is really there.  From each glossy
   point D rays are drawn from FW_MAT_GGX's visible-normal lobe around its view direction, traced and lit at their hits exactly as the
   final gather's rays are, and summed with the estimator's weight F G2 / G1 — which carries the split sum's BRDF term F0 A + B with it.
   Three calls: fw_reflect_rays makes the rays and their weights, fw_reflect_reduce sums what they brought back, fw_bake_reflect chains
   rays, trace, surface, probe lookup, optionally the delta lights, and the reduction.  api.reflect_rays, api.reflect_reduce and
   api.reflect_resolve are the numpy statements.  A glossy surface that a reflection ray hits is lit as if it were diffuse — its F0 (a
   MetalMat's albedo) times the irradiance from the probes over pi — which is the final gather's own simplification: one bounce, no
   recursion.
     Points: fw_ao_rays' (position and normal three floats each at id x stride_floats, id = ids ? ids[q] : q), plus per id the view —
         three floats at id x view_stride_floats, the direction from the eye towards the point, any length — and spec, four packed floats
         (F0.rgb, rho) as fw_probe_shade_glossy takes them.  A point is usable when position, normal and view are finite, normal and view
         are not (0, 0, 0), and rho is finite and > 0.  An unusable point gets D all-zero rays and all-zero weights.
     Ray j of round r at id (fw_reflect_rays, k_reflect_rays).  Everything is float64 from the float32 inputs, every operation rounded as
         written (no contraction), max is fmax, sqrt, sin and cos are the library's float64 functions, one rounding to float32 at the end.
         1. (xi_u, xi_v) = the two shifts fw_ao_rays draws for (seed, r, id); (1/2, 1/2) with jitter == 0.
         2. xi1 = (j + xi_u) / D;  t = j G + xi_v with G = 0.6180339887498949, fw_ao_rays' constant;  xi2 = t - floor(t).
         3. alpha = the float32 product rho rho, widened (as FW_MAT_GGX forms it);  a2 = alpha alpha.
         4. Frame.  n = normal / sqrt((x x + y y) + z z);  u = view / sqrt((x x + y y) + z z);  wo = (-u.x, -u.y, -u.z);  if (wo.x n.x +
            wo.y n.y) + wo.z n.z < 0 then n = -n: it faces the eye.  The tangent frame around n is Duff et al.'s, as FW_MAT_GGX and
            fw_ao_rays form it:  s = copysign(1, n.z);  a = -1 / (s + n.z);  b = (n.x n.y) a;  T = (1 + (s (n.x n.x)) a, s b, -s n.x);
            B = (b, s + (n.y n.y) a, -n.y).  Local wo:  o = ((wo.x T.x + wo.y T.y) + wo.z T.z, the same with B, the same with n).
         5. The visible normal (Heitz 2018, FW_MAT_GGX's) for this o:  v = (alpha o.x, alpha o.y);  vl = sqrt((v.x v.x + v.y v.y) + o.z
            o.z);  Vh = (v.x / vl, v.y / vl, o.z / vl);  l2 = Vh.x Vh.x + Vh.y Vh.y;  T1 = (-Vh.y il, Vh.x il, 0) with il = 1 / sqrt(l2)
            where l2 > 0, else (1, 0, 0);  T2 = Vh x T1 = (-(Vh.z T1.y), Vh.z T1.x, Vh.x T1.y - Vh.y T1.x);  sh = 0.5 (1 + Vh.z);
            r = sqrt(xi1);  phi = (2 pi) xi2;  p1 = r cos phi;  q1 = 1 - p1 p1;  p2 = (1 - sh) sqrt(max(q1, 0)) + sh (r sin phi);
            pz = sqrt(max(q1 - p2 p2, 0));  nh = ((p1 T1.x + p2 T2.x) + pz Vh.x, (p1 T1.y + p2 T2.y) + pz Vh.y, p2 T2.z + pz Vh.z);
            g = (alpha nh.x, alpha nh.y, max(nh.z, 0));  h = g / sqrt((g.x g.x + g.y g.y) + g.z g.z);  oh = (o.x h.x + o.y h.y) + o.z h.z;
            wi = ((2 oh) h.x - o.x, (2 oh) h.y - o.y, (2 oh) h.z - o.z).
         6. The ray is dead unless wi.z > 0 and o.z > 0 (a NaN is dead): six zeros and the weights (0, 0).  fw_trace_rays never traces
            such a ray and fw_hit_surface gives it kind -2.  Otherwise direction = float(((wi.x T.c + wi.y B.c) + wi.z n.c)) per
            component c and origin = float(position.c + bias n.c), n the normal facing the eye.
         7. Weights (g, s), each rounded to float32 once:  Lo1 = 1 + 0.5 (sqrt(1 + a2 ((o.x o.x + o.y o.y) / (o.z o.z))) - 1);
            Li = 0.5 (sqrt(1 + a2 ((wi.x wi.x + wi.y wi.y) / (wi.z wi.z))) - 1);  g = Lo1 / (Lo1 + Li), which is G2 / G1;  m = max(1 -
            oh, 0);  s = ((m m) (m m)) m, Schlick's weight.  Fresnel is per channel, F_c = f0_c + (1 - f0_c) s, and is applied in the
            resolve: neither the rays nor the sums depend on F0.
         rays: n x D x 6 floats, weights: n x D x 2 floats, entry q D + j.
     Reduction of one round (fw_reflect_reduce, k_reflect_reduce): float64 from the float32 inputs, every operation rounded as written.
         Per ray its radiance L is fw_gather_reduce's: kind -2 nothing; kind -1 L = emitted and sky += 1; kind 3 L = emitted; any other
         kind T_c = (E_c > 0 ? E_c : 0) (+ Ed_c with direct), L_c = (albedo_c T_c) (1 / pi).  Eight accumulators: P_c += (g (1 - s)) L_c;
         Q_c += (g s) L_c;  alive += 1 where the float32 g > 0, whatever the ray's kind;  sky as above.  The order is fw_gather_reduce's:
         G = the smallest power of two >= min(D, 64), partial sum l takes j = l, l + G, ... ascending from 0, the G partial sums are
         added by an xor butterfly over the distances G/2 ... 1.  Each accumulator is multiplied by the float64 1 / D, rounded to
         float32 once and added with one float32 addition to sums[id], a record of 32 B: (P.rgb, alive, Q.rgb, sky).  No atomics; two
         runs are bit-equal; a point's result depends on no other point.
     Resolve (k_reflect_resolve), R = the number of rounds in sums and f0 = spec[id]:  out[id].c = float(((double)f0_c P_c + Q_c) / R)
         for the three channels, out[id].w = float(alive / R): the reflected radiance towards the eye and the share of the rays that
         left the surface.  Under a constant environment of radiance 1 it estimates FW_MAT_GGX's directional albedo F0 A + B
         (fw_ggx_terms).  An unusable point resolves to zeros. */
#define FW_REFLECT_DIRECT 1u   /* add the scene's point, spot and directional lights at the reflection rays' hits */
typedef struct fw_reflect {
    uint32_t directions;     /* D, 1..2^20 */
    uint32_t jitter;         /* fw_ao's */
    float    bias;           /* ray origin offset along the normal facing the eye, >= 0, finite */
    float    direct_bias;    /* fw_direct.bias for the shadow rays at the hits */
    uint32_t flags;          /* FW_REFLECT_DIRECT */
    uint32_t chunk_points;   /* 0: as many as fit 256 MiB at this call's bytes per ray (156, plus Ln x 72 + 64 with direct), at least one */
    uint64_t seed;
} fw_reflect;

/* fw_reflect_rays: the rays and weights of round `round` at n points.  Host or device arrays as fw_ao_rays; rays n x D x 6 floats,
   weights n x D x 2 floats.  Only directions, jitter, bias and seed of the description are read beyond its checks.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL reflect, positions, normals, view, spec, rays or weights;
   directions outside 1..2^20, a bias or direct_bias negative or not finite; n == 0; stride_floats < 3; view_stride_floats < 3; with
   on_device spec not 16-byte aligned, weights not 8-byte aligned, positions, normals, ids, view or rays not 4-byte aligned;
   FW_ERR_UNSUPPORTED for n x D >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_reflect_rays(const fw_reflect *reflect, int device, uint32_t round, uint32_t n, const float *positions, const float *normals,
                    uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats, const float *spec,
                    float *rays, float *weights, int on_device, void *stream);

/* fw_reflect_reduce: adds one round's reduction to the running sums.  surface, irradiance and direct as fw_gather_reduce takes them;
   weights: n x D x 2 floats as fw_reflect_rays wrote them; sums: records of 32 B indexed by id.  Host or device arrays.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL surface, irradiance, weights or sums; directions outside
   1..2^20; n == 0; with on_device sums or surface not 16-byte aligned, weights not 8-byte aligned, irradiance, direct or ids not 4-byte
   aligned; FW_ERR_UNSUPPORTED for n x D >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last one. */
int fw_reflect_reduce(int device, uint32_t directions, uint32_t n, const uint32_t *ids, const float *surface, const float *irradiance,
                      const float *direct, const float *weights, float *sums, int on_device, void *stream);

/* fw_bake_reflect: the rounds [first_round, first_round + rounds) of the n points against a resident scene and a baked probe grid:
   fw_bake_gather's statement with its step 1 replaced by k_reflect_rays (rays and weights of the chunk) and its step 6 by
   k_reflect_reduce; steps 2 to 5 — the trace with seed = tp->seed + r and key_base = q0 D, k_hit_surface, the plain, visibility or
   placed lookup at the records in place, with FW_REFLECT_DIRECT fw_bake_direct's kernels at the hits — are the same code.  After the
   last round k_reflect_resolve writes out.  Points, ids, first_round / rounds and what is read of tp are fw_bake_ao's; view,
   view_stride_floats and spec as fw_reflect_rays takes them.
     sums: the running sums (P.rgb, alive, Q.rgb, sky), 8 floats per id, of the rounds [0, first_round), NULL only when first_round == 0;
     out:  4 floats per id, (S.rgb, alive): the resolve above; may be NULL.
   Contracts.  Composition: for every chunk_points, sums equals bit for bit what the public calls give when chained by hand over all n
   points: fw_reflect_rays, fw_trace_rays, fw_hit_surface, the lookup, (fw_bake_direct,) fw_reflect_reduce.  Progressive: k calls of m
   rounds leave the sums and out of one call of k m rounds, bit for bit.  Renders, and the frame graph's key, are left as fw_trace_rays
   leaves them.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, reflect, tp, positions,
   normals, view or spec; directions outside 1..2^20, a bias or direct_bias negative or not finite; n == 0; stride_floats < 3;
   view_stride_floats < 3; rounds == 0; first_round + rounds >= 2^32; a NULL sums with first_round > 0; with on_device sums, out or
   spec not 16-byte aligned, positions, normals, ids or view not 4-byte aligned; then fw_probe_irradiance_placed's checks of grid, sh,
   pd, moments, normal_bias and (with on_device) the tables' alignment; unknown flag bits; FW_ERR_UNSUPPORTED for n x D >= 2^31 and
   the tables' sizes; then FW_ERR_NO_DEVICE; then — Ln is the scene's — FW_ERR_UNSUPPORTED for n x D x Ln >= 2^31.
   stats (may be NULL): fw_bake_gather's. */
int fw_bake_reflect(fw_scene *scene, const fw_reflect *reflect, const fw_trace_params *tp,
                    const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias, const float *placement,
                    uint32_t n, const float *positions, const float *normals, uint32_t stride_floats, const uint32_t *ids,
                    const float *view, uint32_t view_stride_floats, const float *spec,
                    uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats);

/* ---- sphere and rectangle emitters sampled at surface points (additive at ABI 8) ---------------------------------------
   The direct irradiance of the lights FW_FLAG_LIGHT_SAMPLING samples — every EmissiveMat sphere and axis-aligned rectangle — at arbitrary
   surface points, by light sampling: what a final gather's cosine-weighted rays find only by chance when the lamp is small.  From each
   point S shadow rays per light and round go to points drawn on the light as the point sees it; a ray counts where it reaches that light
   itself (the renderer's own rule), and then carries the emission fw_hit_surface evaluates at its hit, times a geometric weight.  Lights
   are summed, not picked.  Five calls: fw_scene_area_lights returns a resident scene's light records, fw_area_rays makes rays and
   weights, fw_area_reduce sums what reached its light, fw_area_mask takes the sampled lights out of a final gather's records (the
   gather's complement, FW_GATHER_NO_LIGHTS), fw_bake_area chains rays, trace, surface and reduction.  api.area_rays, api.area_reduce,
   api.area_resolve and api.area_mask are the numpy statements.
     Light records: FW_LIGHT_RECORD_FLOATS = 16 floats each as fw_selftest_lights writes them — object, kind, 12 geometry floats (a
         sphere: centre.xyz, radius, 8 unused; a rectangle: the world corners c0 .. c3 in order around it), area, p_pick.  Only kind and
         the geometry are read by the rays; the object is what the reduction and the mask compare a hit's object with.
     Points: fw_ao_rays' (position and normal three floats each at id x stride_floats, id = ids ? ids[q] : q; unusable if a component
         is not finite or the normal is (0, 0, 0)).  The caller promises id x Ln + i < 2^31 for every id.
     Entry e = (q Ln + i) S + s: sample s of light i from point q (fw_area_rays, k_area_rays).  Everything is float64 from the float32
         inputs, every operation rounded as written (no contraction), |v| = sqrt((x x + y y) + z z), a . b = (ax bx + ay by) + az bz,
         max is fmax, sqrt, sin, cos and floor are the library's float64 functions, each output rounded to float32 once.
         1. (xi_u, xi_v) = the two shifts fw_ao_rays draws for (seed, round, item id Ln + i); (1/2, 1/2) with jitter == 0.
            a1 = (s + xi_u) / S;  u1 = a1 - floor(a1);  a2 = s G + xi_v with G = 0.6180339887498949;  u2 = a2 - floor(a2).
         2. n = normal / |normal|;  o = position (bias == 0) or position + bias n, per component.
         3. A rectangle (kind 1..3):  e1 = c1 - c0;  e2 = c3 - c0;  d = ((c0 + u1 e1) + u2 e2) - o per component;  nl = e1 x e2 =
            (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x);  A = |nl|;  d2 = d . d;  w = d / sqrt(d2);
            cr = n . w;  cl = |(nl . w) / A|;  g = ((cr cl) A) / d2.  Live only if cr > 0 and A > 0.
         4. A sphere (kind 0), light_sample's construction:  v = centre - o;  dv = v . v;  r2 = radius radius;  live only
            if dv > r2;  s2 = r2 / dv;  cmax = sqrt(1 - s2);  omc = s2 / (1 + cmax);  om = u1 omc;  ct = 1 - om;  st = sqrt(max(om (2 -
            om), 0));  phi = (2 pi) u2;  lx = st cos phi;  ly = st sin phi;  wv = v / sqrt(dv);  the frame (T, B) around wv is Duff et
            al.'s as fw_ao_rays forms it around n;  dir = (lx T + ly B) + ct wv per component;  b = dir . v;  t = b - sqrt(max(b b - (dv -
            r2), 0));  d = t dir: the near intersection;  cr = n . (d / |d|);  g = (cr (2 pi)) omc.  Live only if cr > 0.
         5. The entry is dead unless the point is usable, the conditions above hold, g is finite, float(g) > 0 and finite, the six
            rounded floats are finite and the rounded direction is not (0, 0, 0) — a NaN anywhere is dead.  A dead entry is six zeros
            and the weight 0: fw_trace_rays never traces it.  A live entry is (float(o), float(d)) and the weight float(g): the light
            sits at t = 1 along the ray.
     Reduction of one round (fw_area_reduce, k_area_reduce) over the M = Ln S entries m = i S + s of point q, with the weight w, the hit
         h that fw_trace_rays wrote for the ray and the record r that fw_hit_surface wrote for that hit: the entry counts exactly where
         w > 0, h.object == objects[i] and r.kind == 3 (FW_MAT_EMISSIVE) — so whatever stops the walk on the way occludes, a
         ConstantMedium included.  Four float64 accumulators: E_c += (double)r.emitted_c x (double)w and V += 1.  The order is
         fw_ao_reduce's over M: G = the smallest power of two >= min(M, 64), partial sum l takes m = l, l + G, ... ascending from 0, the
         G partial sums are added by an xor butterfly over the distances G/2 ... 1.  E is multiplied by the float64 1 / S and V by the
         float64 1 / M; each is rounded to float32 once and added with one float32 addition to sums[id] = (Er, Eg, Eb, vis).  No
         atomics; two runs are bit-equal; a point's result depends on no other point.
     Resolve (k_area_resolve), R = the number of rounds in sums: out[id] = float((double)sums[id] / R) for the four floats: the area
         lights' irradiance at the point and the share of its shadow rays that arrived.
     Mask (fw_area_mask, k_area_mask): record e is rewritten to (kind -2, every other float 0) where its kind is 3 and hits[e].object is
         in the strictly ascending list `objects` (binary search); every other record keeps its bits. */
typedef struct fw_area {
    uint32_t samples;        /* S per light, 1..2^20 */
    uint32_t jitter;         /* fw_ao's */
    float    bias;           /* shadow-ray origin offset along the point's normal, >= 0, finite */
    uint32_t chunk_points;   /* fw_bake_area: points per chunk; 0 = as many as fit 256 MiB at 140 B per entry, at least one */
    uint64_t seed;
} fw_area;

/* fw_scene_area_lights: the records fw_selftest_lights would give for the description the resident scene now represents, objects moved
   by fw_scene_update included, in ascending object order.  *n = their number; the first min(cap, *n) are written to out (host memory).
   CPU only.  FW_ERR_BAD_ARG for a NULL scene or n, or a NULL out with cap > 0. */
int fw_scene_area_lights(fw_scene *scene, float *out, uint32_t cap, uint32_t *n);

/* fw_area_rays: the shadow rays and weights of round `round` from n points towards n_lights records (host memory always).  rays n x Ln
   x S x 6 floats, weights n x Ln x S floats; host or device arrays as fw_ao_rays.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL area, lights, positions, normals, rays or weights; samples
   outside 1..2^20, bias negative or not finite; n_lights outside 1..FW_MAX_LIGHTS or a record whose kind is not 0..3; n == 0;
   stride_floats < 3; with on_device an array not 4-byte aligned; FW_ERR_UNSUPPORTED for n x Ln x S >= 2^31, and for (the largest id +
   1) x Ln >= 2^31 (host ids; n x Ln with device arrays); then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last. */
int fw_area_rays(const fw_area *area, const float *lights, uint32_t n_lights, int device, uint32_t round, uint32_t n, const float *positions,
                 const float *normals, uint32_t stride_floats, const uint32_t *ids, float *rays, float *weights, int on_device, void *stream);

/* fw_area_reduce: adds one round's reduction to the running sums.  objects: the n_objects = Ln lights' object indices in the records'
   order (host memory always); weights n x M floats, hits n x M records, surface n x M x 16 floats; sums records of 16 B indexed by id.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL objects, weights, hits, surface or sums; samples outside
   1..2^20; n_objects outside 1..FW_MAX_LIGHTS; n == 0; with on_device sums, hits or surface not 16-byte aligned, weights or ids not
   4-byte aligned; FW_ERR_UNSUPPORTED for n x M >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last. */
int fw_area_reduce(int device, uint32_t samples, const uint32_t *objects, uint32_t n_objects, uint32_t n, const uint32_t *ids, const float *weights,
                   const fw_hit *hits, const float *surface, float *sums, int on_device, void *stream);

/* fw_area_mask: rewrites in place the records of n hits that lie on one of `objects` (host memory always, strictly ascending).
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL objects, hits or surface; n_objects outside
   1..FW_MAX_LIGHTS or a list that does not ascend strictly; n == 0; with on_device hits or surface not 16-byte aligned;
   FW_ERR_UNSUPPORTED for n >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last. */
int fw_area_mask(int device, const uint32_t *objects, uint32_t n_objects, uint32_t n, const fw_hit *hits, float *surface, int on_device, void *stream);

/* fw_bake_area: the rounds [first_round, first_round + rounds) of the n points against a resident scene and its own sampled lights (Ln
   of them).  Points, ids, sums, out, first_round / rounds and what is read of tp are fw_bake_ao's.  For each round r and each chunk of
   points [q0, q1) (chunk_points at a time), in device scratch that the call allocates and frees on every path:
     1. k_area_rays: fw_area_rays' rays and weights for the scene's records, bit for bit;
     2. the trace, as fw_bake_ao runs it: on_device, seed = tp->seed + r, key_base = q0 Ln S;
     3. k_hit_surface over the chunk's rays and hits;
     4. k_area_reduce into sums.
   After the last round k_area_resolve writes out.  A scene without sampled lights traces nothing: sums stay as they are and out is
   their resolve — zeros.  On an error the stream is drained.
   Contracts.  Composition: for every chunk_points, sums equals bit for bit what fw_area_rays, fw_trace_rays (seed + r, key_base 0),
   fw_hit_surface and fw_area_reduce give when chained by hand over all n points.  Progressive: k calls of m rounds leave the sums and
   out of one call of k m rounds, bit for bit.  Renders, and the frame graph's key, are left as fw_trace_rays leaves them.
   Errors, in this order and before the scene is looked at or HIP is called: FW_ERR_BAD_ARG for a NULL scene, area, tp, positions or
   normals; samples outside 1..2^20, bias negative or not finite; n == 0; stride_floats < 3; rounds == 0; first_round + rounds >= 2^32;
   a NULL sums with first_round > 0; with on_device sums or out not 16-byte aligned, positions, normals or ids not 4-byte aligned; then
   FW_ERR_NO_DEVICE; then — Ln is the scene's — FW_ERR_UNSUPPORTED for n x Ln x S >= 2^31.
   stats (may be NULL): fw_bake_ao's. */
int fw_bake_area(fw_scene *scene, const fw_area *area, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
                 uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats);

/* ---- every emitter sampled at surface points, picked by power (additive at ABI 8) ----------------------------------------
   The direct irradiance of every emitting primitive of a scene — FW_FLAG_ALL_EMITTERS' entries (§9i): EmissiveMat spheres, axis-aligned
   rectangles, Rect3d faces, disks and mesh triangles — at arbitrary surface points.  Each point sends S shadow rays per round whatever the
   number of entries, each towards an entry picked in proportion to area x power through a CDF, with the pick's probability in the weight.
   api.emitters_cdf, api.emitters_rays and api.emitters_reduce are the numpy statements; resolve and mask are fw_bake_area's.
     Records: FW_EMITTERS_RECORD_FLOATS = 16 floats per entry, in fw_selftest_emitters' order: object, kind (FW_SHAPE_*), 12 geometry
         floats, area, weight (fw_selftest_emitters' two).  Geometry, in the world, rotated exactly where the walks rotate the object:
         a sphere: centre.xyz, radius, 8 zeros and a rectangle: its corners c0 .. c3 in order around it — both fw_selftest_lights'
         floats; a Rect3d face: its four corners in the rectangle's order ((lo, lo), (hi, lo), (hi, hi), (lo, hi) in the face's two axes,
         bounds pos and the float32 pos + size); a triangle: v0, v1, v2, three zeros; a disk: centre, the images of the object's x and z
         axes, then radius, inner_radius, phi_max.  Every point other than a sphere's and a rectangle's is float(((R0 x + R1 y) + R2 z) +
         position) per component in float64, R the object's float32 rotation rows (the identity where the walks do not rotate).
         codes: two words per entry, (object, prim): a Rect3d's face, a mesh's triangle, else 0.
     CDF (fw_emitters_cdf): float64 inclusive prefix sums of the float32 weights in entry order, a negative or non-finite weight counted
         as 0, each divided by the last: the last positive entry and every one after it is exactly 1.  An entry's probability is p_i =
         cdf[i] - cdf[i - 1] (cdf[-1] = 0).  A total of 0: "no emitters", the cdf is zeros and nothing may be sampled from it.
     Entry e = q S + s: sample s from point q (fw_emitters_rays, k_emitters_rays); numerics and points are fw_area_rays'.
         1. (xi_u, xi_v) = the two shifts fw_ao_rays draws for (seed, round, item id); (1/2, 1/2) with jitter == 0.
            a1 = (s + xi_u) / S;  xi = a1 - floor(a1);  a2 = s G + xi_v with G = 0.6180339887498949;  u2 = a2 - floor(a2).
         2. The pick i = the first index with cdf[i] > xi;  lo = i ? cdf[i - 1] : 0;  p = cdf[i] - lo;  u1 = min((xi - lo) / p, 1 - 2^-53).
         3. n and o as fw_area_rays' step 2.
         4. A sphere: fw_area_rays' step 4 with (u1, u2), g its g.  A rectangle or Rect3d face: fw_area_rays' step 3, g its g.
         5. A triangle: e1 = v1 - v0;  e2 = v2 - v0;  sq = sqrt(u1);  (b0, b1, b2) = (1 - sq, sq (1 - u2), sq u2);  d = ((b0 v0 + b1 v1)
            + b2 v2) - o;  nl = e1 x e2;  L = |nl|;  A = L / 2.  A disk: r2 = r r;  i2 = r_in r_in;  rr = sqrt(i2 + u1 (r2 - i2));  phi =
            u2 phi_max;  d = ((c + (rr cos phi) ax) + (rr sin phi) az) - o;  nl = ax x az;  L = |nl|;  A = (0.5 phi_max) (r2 - i2).
            Both: d2 = d . d;  w = d / sqrt(d2);  cr = n . w;  cl = |(nl . w) / L|;  g = ((cr cl) A) / d2 (the rectangle's form, where
            A = L).  Live only if cr > 0, A > 0 and L > 0.
         6. The weight is float(g / p).  Dead exactly as fw_area_rays' step 5 with g / p for g: six zeros, the weight 0 and the pick
            0xffffffff; a live entry is (float(o), float(d)), the weight and the pick i.
     Reduction of one round (fw_emitters_reduce, k_emitters_reduce) over the S entries of point q: an entry counts exactly where its
         weight > 0, its pick i < n_entries, the hit's object and prim equal codes[2 i] and codes[2 i + 1], and fw_hit_surface's record
         has kind 3.  Accumulators, order, butterfly and rounding are fw_area_reduce's with M = S; E and V are both multiplied by the
         float64 1 / S. */
#define FW_EMITTERS_RECORD_FLOATS 16
typedef struct fw_emitters {
    uint32_t samples;        /* S per point and round, 1..2^20 */
    uint32_t jitter;         /* fw_ao's */
    float    bias;           /* shadow-ray origin offset along the point's normal, >= 0, finite */
    uint32_t chunk_points;   /* fw_bake_emitters: points per chunk; 0 = as many as fit 256 MiB at 144 B per entry, at least one */
    uint64_t seed;
} fw_emitters;

/* fw_selftest_emitters_records (CPU only): the records and codes of a description's entries.  *n = their number; the first min(cap, *n)
   records (16 floats) and codes (2 words) are written; either array may be NULL with cap == 0.  FW_ERR_BAD_ARG for a NULL desc or n, or a
   NULL records or codes with cap > 0. */
int fw_selftest_emitters_records(const fw_scene_desc *desc, float *records, uint32_t *codes, uint32_t cap, uint32_t *n);

/* fw_scene_emitters: the same for the description a resident scene now represents, objects moved by fw_scene_update included.  The list
   is built by the first call that needs it (this one, fw_bake_emitters, fw_bake_gather with FW_GATHER_NO_EMITTERS) and again after every
   fw_scene_update; a mesh's triangles are read back from the device (objects in a row that share a mesh read it once), so where a mesh emits that first call
   synchronises the whole device once, whatever stream its caller passed.  FW_ERR_BAD_ARG as above; FW_ERR_UNSUPPORTED above 2^24 entries. */
int fw_scene_emitters(fw_scene *scene, float *records, uint32_t *codes, uint32_t cap, uint32_t *n);

/* fw_emitters_cdf (CPU only): cdf[0..n) from weights[0..n).  *total (may be NULL) = the float64 sum; 0: no emitters, cdf is zeros.
   FW_ERR_BAD_ARG for a NULL weights or cdf or n == 0. */
int fw_emitters_cdf(const float *weights, uint32_t n, double *cdf, double *total);

/* fw_emitters_rays: the shadow rays, weights and picks of round `round` from n points towards n_entries records with their cdf (host
   memory always).  rays n x S x 6 floats, weights n x S floats, picks n x S words; host or device arrays as fw_ao_rays.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL emitters, records, cdf, positions, normals, rays, weights or
   picks; samples outside 1..2^20, bias negative or not finite; n_entries outside 1..2^24, a record whose kind is not 0..5 or 9, a cdf
   that decreases, leaves [0, 1] or does not end in 1; n == 0; stride_floats < 3; with on_device an array not 4-byte aligned;
   FW_ERR_UNSUPPORTED for n x S >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last. */
int fw_emitters_rays(const fw_emitters *emitters, const float *records, const double *cdf, uint32_t n_entries, int device, uint32_t round, uint32_t n,
                     const float *positions, const float *normals, uint32_t stride_floats, const uint32_t *ids, float *rays, float *weights,
                     uint32_t *picks, int on_device, void *stream);

/* fw_emitters_reduce: adds one round's reduction to the running sums.  codes: 2 x n_entries words (host memory always); picks and weights
   n x S words, hits n x S records, surface n x S x 16 floats; sums records of 16 B indexed by id.
   Errors, in this order and before HIP is called: FW_ERR_BAD_ARG for a NULL codes, picks, weights, hits, surface or sums; samples outside
   1..2^20; n_entries outside 1..2^24; n == 0; with on_device sums, hits or surface not 16-byte aligned, picks, weights or ids not 4-byte
   aligned; FW_ERR_UNSUPPORTED for n x S >= 2^31; then FW_ERR_NO_DEVICE, and FW_ERR_BAD_ARG for a device index past the last. */
int fw_emitters_reduce(int device, uint32_t samples, const uint32_t *codes, uint32_t n_entries, uint32_t n, const uint32_t *ids, const uint32_t *picks,
                       const float *weights, const fw_hit *hits, const float *surface, float *sums, int on_device, void *stream);

/* fw_bake_emitters: the rounds [first_round, first_round + rounds) of the n points against a resident scene and its own entries.  Points,
   ids, sums, out, first_round / rounds and what is read of tp are fw_bake_ao's.  For each round r and each chunk of points [q0, q1):
     1. k_emitters_rays: fw_emitters_rays' rays, weights and picks for fw_scene_emitters' records and their fw_emitters_cdf, bit for bit;
     2. the trace, as fw_bake_ao runs it: on_device, seed = tp->seed + r, key_base = q0 S;
     3. k_hit_surface over the chunk's rays and hits;
     4. k_emitters_reduce into sums.
   After the last round k_area_resolve writes out.  A scene without entries, or whose weights sum to 0, traces nothing: sums stay as they
   are and out is their resolve — zeros.  Composition and progressive contracts are fw_bake_area's.
   Errors, in this order and before the scene is looked at or HIP is called: fw_bake_area's with `emitters` for `area`; then
   FW_ERR_NO_DEVICE; then FW_ERR_UNSUPPORTED for more than 2^24 entries and for n x S >= 2^31.  stats (may be NULL): fw_bake_ao's. */
int fw_bake_emitters(fw_scene *scene, const fw_emitters *emitters, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
                     uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FIREWORK_HIP_H */
