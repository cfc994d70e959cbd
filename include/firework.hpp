// firework.hpp — header-only C++ mirror of the reference's host API for the render path, over the C ABI of
// firework_hip.h.  The reference is compiled code (Rust); with no Rust toolchain in the image this is the
// compiled-language host side: the same builder names, argument order and defaults as
//
//   Scene / RenderObject                      reference src/scene.rs:19-91,270-334
//   Sphere, XYRect/XZRect/YZRect, Rect3d,     src/objects/*.rs
//     TriangleMesh, Cone, Cylinder, Disk
//   LambertianMat, MetalMat, DielectricMat,   src/material.rs
//     EmissiveMat, IsotropicMat
//   ConstantTexture, CheckerTexture, ...      src/texture.rs
//   ColorEnv, SkyEnv, HdrEnvironment          src/environment.rs, examples/hdri_test.rs:22-82
//   Rotor3, CameraSettings, Renderer          ultraviolet, src/camera.rs:18-71, src/render.rs:59-218
//
// so that `examples/cornell_box.rs` ports line by line (examples/cornell_box.cpp).  `Renderer::render` lowers
// the scene to fw_scene_desc and calls fw_render_scene — no CPU fallback; failures throw std::runtime_error
// carrying the reference's panic messages.
#pragma once
#include "firework_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace firework {

struct Vec3 { float x = 0, y = 0, z = 0; Vec3() = default; Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    static Vec3 broadcast(float v) { return {v, v, v}; } static Vec3 zero() { return {}; } static Vec3 one() { return {1, 1, 1}; } };
inline fw_vec3 lower(Vec3 v) { return fw_vec3{v.x, v.y, v.z}; }

struct Color { uint8_t r, g, b; };   // util.rs:6 `Color(pub u8, pub u8, pub u8)`
static_assert(sizeof(Color) == 3, "Color must be 3 packed bytes (same bytes as the ABI's rgb8 output)");

// ultraviolet::Rotor3 {s, bv:{xy,xz,yz}}; from_rotation_P(t) = {cos(t/2), unit_plane * -sin(t/2)} (pinned by scenes/*.yml)
struct Rotor3 {
    float s = 1, xy = 0, xz = 0, yz = 0;
    static Rotor3 identity() { return {}; }
    static Rotor3 plane(float angle, int which) {
        // sin/cos evaluated in double and rounded once (what firework_amd/api.py does; both reproduce the
        // rotors serialised in the reference's scenes/*.yml)
        float half = angle / 2.0f, ms = -(float)std::sin((double)half);
        Rotor3 r; r.s = (float)std::cos((double)half);
        r.xy = (which == 0 ? 1.0f : 0.0f) * ms; r.xz = (which == 1 ? 1.0f : 0.0f) * ms; r.yz = (which == 2 ? 1.0f : 0.0f) * ms;
        return r;
    }
    static Rotor3 from_rotation_xy(float a) { return plane(a, 0); }
    static Rotor3 from_rotation_xz(float a) { return plane(a, 1); }
    static Rotor3 from_rotation_yz(float a) { return plane(a, 2); }
    Rotor3 operator*(const Rotor3 &b) const {   // geometric product on (1, e12, e13, e23)
        // every sum is an fma chain (ultraviolet builds its products from mul_add): the association that reproduces the
        // rotor serialised in the reference's scenes/conics.yml bit for bit (same chain as firework_amd/api.py)
        const Rotor3 &a = *this; Rotor3 r;
        auto chain = [](float x0, float y0, float x1, float y1, float x2, float y2, float x3, float y3) {
            return std::fma(x0, y0, std::fma(x3, y3, std::fma(x2, y2, x1 * y1)));
        };
        r.s = chain(a.s, b.s, -a.xy, b.xy, -a.xz, b.xz, -a.yz, b.yz);
        r.xy = chain(a.xy, b.s, a.s, b.xy, a.yz, b.xz, -a.xz, b.yz);
        r.xz = chain(a.xz, b.s, a.s, b.xz, -a.yz, b.xy, a.xy, b.yz);
        r.yz = chain(a.yz, b.s, a.s, b.yz, a.xz, b.xy, -a.xy, b.xz);
        return r;
    }
    static Rotor3 from_euler_angles(float roll, float pitch, float yaw) { return from_rotation_xz(yaw) * from_rotation_yz(pitch) * from_rotation_xy(roll); }
};

using MaterialIdx = int32_t;
using RenderObjectIdx = size_t;

// ---- textures ---------------------------------------------------------------------------------------------
struct Texture {
    fw_texture t{}; std::shared_ptr<Texture> odd, even; std::shared_ptr<std::vector<uint8_t>> pixels;
};
using TexturePtr = std::shared_ptr<Texture>;
struct ConstantTexture {
    static TexturePtr new_(Vec3 c) { auto p = std::make_shared<Texture>(); p->t.kind = FW_TEX_CONSTANT; p->t.color = lower(c); return p; }
    static TexturePtr from_rgb(float r, float g, float b) { return new_({r, g, b}); }
};
struct CheckerTexture {
    static TexturePtr new_(TexturePtr odd, TexturePtr even, float scale) { auto p = std::make_shared<Texture>(); p->t.kind = FW_TEX_CHECKER; p->t.scale = scale; p->odd = std::move(odd); p->even = std::move(even); return p; }
    static TexturePtr with_colors(Vec3 odd, Vec3 even, float scale) { return new_(ConstantTexture::new_(odd), ConstantTexture::new_(even), scale); }
};
struct PerlinNoiseTexture { static TexturePtr new_(float scale) { auto p = std::make_shared<Texture>(); p->t.kind = FW_TEX_PERLIN; p->t.scale = scale; return p; } };
struct TurbulenceTexture { static TexturePtr new_(uint32_t depth, float scale) { auto p = std::make_shared<Texture>(); p->t.kind = FW_TEX_TURBULENCE; p->t.depth = depth; p->t.scale = scale; return p; } };
struct MarbleTexture { static TexturePtr new_(uint32_t depth, float scale) { auto p = std::make_shared<Texture>(); p->t.kind = FW_TEX_MARBLE; p->t.depth = depth; p->t.scale = scale; return p; } };
struct ImageTexture {   // RGB8, row 0 = top
    static TexturePtr new_(uint32_t w, uint32_t h, std::vector<uint8_t> rgb8) {
        if (rgb8.size() != (size_t)w * h * 3) throw std::runtime_error("ImageTexture: pixel buffer size mismatch");
        auto p = std::make_shared<Texture>(); p->t.kind = FW_TEX_IMAGE; p->t.img_w = w; p->t.img_h = h;
        p->pixels = std::make_shared<std::vector<uint8_t>>(std::move(rgb8)); p->t.img_rgb8 = p->pixels->data(); return p; }
};

// ---- materials ----------------------------------------------------------------------------------------------
struct Material { fw_material m{}; TexturePtr tex; };
struct LambertianMat { static Material new_(TexturePtr albedo) { Material r; r.m.kind = FW_MAT_LAMBERTIAN; r.tex = std::move(albedo); return r; }
                       static Material with_color(Vec3 c) { return new_(ConstantTexture::new_(c)); } };
struct MetalMat { static Material new_(Vec3 albedo, float roughness) { Material r; r.m.kind = FW_MAT_METAL; r.m.albedo = lower(albedo); r.m.roughness = roughness; return r; } };
// an isotropic GGX conductor (FW_MAT_GGX, firework_hip.h): albedo = F0 in [0, 1], roughness in [0.03, 1]; not in the reference
struct GgxMat { static Material new_(Vec3 albedo, float roughness) { Material r; r.m.kind = FW_MAT_GGX; r.m.albedo = lower(albedo); r.m.roughness = roughness; return r; } };
struct DielectricMat { static Material new_(float ref_idx) { Material r; r.m.kind = FW_MAT_DIELECTRIC; r.m.ref_idx = ref_idx; return r; } };
struct EmissiveMat { static Material new_(TexturePtr albedo) { Material r; r.m.kind = FW_MAT_EMISSIVE; r.tex = std::move(albedo); return r; }
                     static Material with_color(Vec3 c) { return new_(ConstantTexture::new_(c)); } };
struct IsotropicMat { static Material new_(TexturePtr texture) { Material r; r.m.kind = FW_MAT_ISOTROPIC; r.tex = std::move(texture); return r; } };

// ---- shapes -------------------------------------------------------------------------------------------------
struct Shape {
    fw_shape s{}; std::shared_ptr<Shape> inner;
    std::shared_ptr<std::vector<float>> verts, normals, uvs; std::shared_ptr<std::vector<uint32_t>> indices;
};
inline Shape make_shape(int kind, MaterialIdx m) { Shape r; r.s.kind = kind; r.s.material = m; r.s.inner = -1; return r; }
struct Sphere { static Shape new_(float radius, MaterialIdx m) { Shape r = make_shape(FW_SHAPE_SPHERE, m); r.s.radius = radius; return r; } };
inline Shape make_rect(int kind, float a0, float a1, float b0, float b1, float k, MaterialIdx m) {
    Shape r = make_shape(kind, m); r.s.a_min = a0; r.s.a_max = a1; r.s.b_min = b0; r.s.b_max = b1; r.s.k = k; return r; }
struct XYRect { static Shape new_(float x0, float x1, float y0, float y1, float k, MaterialIdx m) { return make_rect(FW_SHAPE_XYRECT, x0, x1, y0, y1, k, m); } };
struct XZRect { static Shape new_(float x0, float x1, float z0, float z1, float k, MaterialIdx m) { return make_rect(FW_SHAPE_XZRECT, x0, x1, z0, z1, k, m); } };
struct YZRect { static Shape new_(float y0, float y1, float z0, float z1, float k, MaterialIdx m) { return make_rect(FW_SHAPE_YZRECT, y0, y1, z0, z1, k, m); } };
struct Rect3d { static Shape with_size(Vec3 size, MaterialIdx m) { Shape r = make_shape(FW_SHAPE_RECT3D, m); r.s.pos = {0, 0, 0}; r.s.size = lower(size); return r; } };
struct Cone { static Shape new_(float radius, float height, MaterialIdx m) { Shape r = make_shape(FW_SHAPE_CONE, m); r.s.radius = radius; r.s.height = height; return r; } };
constexpr float RADS_PER_DEG = 3.14159265358979323846f / 180.0f;   // f32::to_radians
struct Cylinder {
    static Shape new_(float radius, float height, MaterialIdx m) { return partial(radius, height, 360.0f, m); }
    static Shape partial(float radius, float height, float phi_deg, MaterialIdx m) { Shape r = make_shape(FW_SHAPE_CYLINDER, m); r.s.radius = radius; r.s.height = height; r.s.phi_max = phi_deg * RADS_PER_DEG; return r; } };
struct Disk {
    static Shape new_(float radius, MaterialIdx m) { Shape r = make_shape(FW_SHAPE_DISK, m); r.s.radius = radius; r.s.phi_max = 2.0f * 3.14159265358979323846f; return r; }
    static Shape partial(float radius, float phi_deg, float inner_radius, MaterialIdx m) { Shape r = make_shape(FW_SHAPE_DISK, m); r.s.radius = radius; r.s.phi_max = phi_deg * RADS_PER_DEG; r.s.inner_radius = inner_radius; return r; } };
struct TriangleMesh {   // mesh.rs:37-63: same two error strings
    static Shape new_(std::vector<float> verts /*3*n*/, std::vector<uint32_t> indicies, std::vector<float> normals /*empty or 3*n*/,
                      std::vector<float> uvs /*empty or 2*n*/, MaterialIdx m) {
        size_t n = verts.size() / 3;
        if (!normals.empty() && normals.size() != 3 * n) throw std::runtime_error("TriangleMesh::new() -- normals.len() must equal verts.len()");
        if (!uvs.empty() && uvs.size() != 2 * n) throw std::runtime_error("TriangleMesh::new() -- uvs.len() must equal verts.len()");
        Shape r = make_shape(FW_SHAPE_TRIANGLE_MESH, m);
        r.verts = std::make_shared<std::vector<float>>(std::move(verts)); r.indices = std::make_shared<std::vector<uint32_t>>(std::move(indicies));
        if (!normals.empty()) r.normals = std::make_shared<std::vector<float>>(std::move(normals));
        if (!uvs.empty()) r.uvs = std::make_shared<std::vector<float>>(std::move(uvs));
        return r; }
};

// ---- environments ---------------------------------------------------------------------------------------------
struct Environment { fw_environment e{}; std::shared_ptr<std::vector<float>> hdr; };
struct ColorEnv { static Environment new_(Vec3 c) { Environment r; r.e.kind = FW_ENV_COLOR; r.e.color = lower(c); return r; } };
struct SkyEnv { static Environment new_(Vec3 zenith, Vec3 horizon) { Environment r; r.e.kind = FW_ENV_SKY; r.e.zenith = lower(zenith); r.e.horizon = lower(horizon); return r; }
                static Environment default_() { return new_({0.5f, 0.7f, 1.0f}, {1, 1, 1}); } };
struct HdrEnvironment { static Environment new_(uint32_t w, uint32_t h, std::vector<float> rgb) { Environment r; r.e.kind = FW_ENV_HDR; r.e.hdr_w = w; r.e.hdr_h = h;
                        r.hdr = std::make_shared<std::vector<float>>(std::move(rgb)); r.e.hdr_rgb = r.hdr->data(); return r; } };

// ---- RenderObject / Scene -----------------------------------------------------------------------------------------
struct RenderObject {
    Shape obj; Vec3 pos; Rotor3 rotation; bool flip = false;
    static RenderObject new_(Shape s) { RenderObject r; r.obj = std::move(s); return r; }
    RenderObject position(float x, float y, float z) && { pos = {x, y, z}; return std::move(*this); }
    RenderObject position_vec(Vec3 p) && { pos = p; return std::move(*this); }
    RenderObject rotate(Rotor3 r) && { rotation = r; return std::move(*this); }
    RenderObject flip_normals() && { flip = !flip; return std::move(*this); }
};

// Lights without area (not in the reference; fw_scene_set_lights): found by next-event estimation alone, they light the
// Lambertian and Isotropic surfaces of every call on this header's Renderer and DeviceScene (render() of a lit scene goes through a resident
// scene; only its multi-GPU devices() form, fw_render_scene_tiled on a bare description, has none).  intensity: radiant intensity per
// steradian; irradiance: on a plane that faces the light; direction: any length.
struct Light { fw_light l{}; };
struct PointLight { static Light new_(Vec3 position, Vec3 intensity) { Light r; r.l.kind = FW_LIGHT_POINT; r.l.position = lower(position); r.l.intensity = lower(intensity); return r; } };
struct SpotLight {   // full intensity within inner_deg of the axis, none beyond outer_deg, a smoothstep of the cosine between
    static Light new_(Vec3 position, Vec3 direction, Vec3 intensity, float inner_deg, float outer_deg) {
        Light r; r.l.kind = FW_LIGHT_SPOT; r.l.position = lower(position); r.l.direction = lower(direction); r.l.intensity = lower(intensity);
        r.l.cos_inner = (float)std::cos((double)inner_deg * 3.14159265358979323846 / 180.0); r.l.cos_outer = (float)std::cos((double)outer_deg * 3.14159265358979323846 / 180.0);
        return r; } };
struct DirectionalLight { static Light new_(Vec3 direction, Vec3 irradiance) { Light r; r.l.kind = FW_LIGHT_DIRECTIONAL; r.l.direction = lower(direction); r.l.intensity = lower(irradiance); return r; } };

struct Scene {
    std::vector<RenderObject> render_objects; std::vector<Material> materials; Environment environment = ColorEnv::new_({0, 0, 0});   // scene.rs:36
    std::vector<fw_light> lights;
    size_t add_light(const Light &l) { lights.push_back(l.l); return lights.size() - 1; }
    static Scene new_() { return {}; }
    RenderObjectIdx add_object(RenderObject o) { render_objects.push_back(std::move(o)); return render_objects.size() - 1; }
    MaterialIdx add_material(Material m) { materials.push_back(std::move(m)); return (MaterialIdx)materials.size() - 1; }
    RenderObjectIdx add_volume(RenderObject o, float density, TexturePtr texture) {   // scene.rs:47-62
        MaterialIdx mat = add_material(IsotropicMat::new_(std::move(texture)));
        Shape medium = make_shape(FW_SHAPE_CONSTANT_MEDIUM, mat); medium.s.density = density;
        medium.inner = std::make_shared<Shape>(std::move(o.obj)); o.obj = std::move(medium);
        return add_object(std::move(o)); }
    void set_environment(Environment e) { environment = std::move(e); }
};

struct CameraSettings {   // camera.rs:26-36 defaults
    Vec3 cam_pos_{0, 0, -10}, look_at_{0, 0, 0}; float vfov = 30, aperture_ = 0, focus_dist_ = 10;
    static CameraSettings default_() { return {}; }
    CameraSettings cam_pos(Vec3 v) && { cam_pos_ = v; return std::move(*this); }
    CameraSettings look_at(Vec3 v) && { look_at_ = v; return std::move(*this); }
    CameraSettings field_of_view(float f) && { vfov = f; return std::move(*this); }
    CameraSettings aperture(float a) && { aperture_ = a; return std::move(*this); }
    CameraSettings focus_dist(float d) && { focus_dist_ = d; return std::move(*this); }
};

// A non-pinhole camera whose rays are generated on the device (fw_camera_model; not in the reference): an equirectangular panorama from a
// position, parallel rays over a view plane view_height high, or an equidistant full-frame fisheye of fov degrees across the diagonal.
struct CameraModel {
    fw_camera_model m{};
    static CameraModel panorama(Vec3 position, size_t width, size_t height) {
        return make(FW_MODEL_PANORAMA, CameraSettings::default_().cam_pos(position), width, height, 0.0, 0.0); }
    static CameraModel orthographic(const CameraSettings &camera, double view_height, size_t width, size_t height) {
        return make(FW_MODEL_ORTHOGRAPHIC, camera, width, height, view_height, 0.0); }
    static CameraModel fisheye(const CameraSettings &camera, double fov, size_t width, size_t height) {
        return make(FW_MODEL_FISHEYE, camera, width, height, 0.0, fov); }
    CameraModel seed(uint64_t s) && { m.seed = s; return std::move(*this); }
    CameraModel jitter(bool on) && { m.jitter = on ? 1 : 0; return std::move(*this); }
    CameraModel chunk_samples(uint32_t n) && { m.chunk_samples = n; return std::move(*this); }
  private:
    static CameraModel make(int kind, const CameraSettings &c, size_t width, size_t height, double view_height, double fov) {
        CameraModel r; r.m.kind = kind; r.m.width = (uint32_t)width; r.m.height = (uint32_t)height;
        r.m.camera = fw_camera_settings{fw_vec3{c.cam_pos_.x, c.cam_pos_.y, c.cam_pos_.z}, fw_vec3{c.look_at_.x, c.look_at_.y, c.look_at_.z}, c.vfov,
                                        c.aperture_, c.focus_dist_};
        r.m.view_height = view_height; r.m.fov = fov; r.m.jitter = 1;
        return r; }
};

// Irradiance probes (fw_probe_set; not in the reference): positions with `directions` rays each and round, baked by Renderer::bake_probes into
// nine SH coefficients (l <= 2) per probe and colour channel.  grid(): nx x ny x nz probes from corner lo to corner hi, both included (a
// count of 1 sits at the middle), x fastest, then y, then z; the set keeps the grid (has_grid, grid_abi()), which is what
// Renderer::probe_lit needs to read the coefficients back.
struct ProbeSet {
    std::vector<float> positions;       // n x 3
    uint32_t directions = 256, chunk = 0; uint64_t seed_ = 0; bool jitter_ = true;
    bool has_grid = false; double grid_lo[3] = {0, 0, 0}, grid_hi[3] = {0, 0, 0}; uint32_t grid_counts[3] = {0, 0, 0};
    static ProbeSet new_(const std::vector<Vec3> &at, uint32_t directions = 256) {
        ProbeSet r; r.directions = directions;
        for (const Vec3 &v : at) { r.positions.push_back(v.x); r.positions.push_back(v.y); r.positions.push_back(v.z); }
        return r; }
    static ProbeSet grid(Vec3 lo, Vec3 hi, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t directions = 256) {
        ProbeSet r; r.directions = directions;
        auto at = [](float a, float b, uint32_t i, uint32_t n) { return n > 1 ? (float)((double)a + ((double)b - (double)a) * (double)i / (double)(n - 1)) : (float)(0.5 * ((double)a + (double)b)); };
        for (uint32_t z = 0; z < nz; z++) for (uint32_t y = 0; y < ny; y++) for (uint32_t x = 0; x < nx; x++) {
            r.positions.push_back(at(lo.x, hi.x, x, nx)); r.positions.push_back(at(lo.y, hi.y, y, ny)); r.positions.push_back(at(lo.z, hi.z, z, nz)); }
        r.has_grid = true;
        r.grid_lo[0] = lo.x; r.grid_lo[1] = lo.y; r.grid_lo[2] = lo.z; r.grid_hi[0] = hi.x; r.grid_hi[1] = hi.y; r.grid_hi[2] = hi.z;
        r.grid_counts[0] = nx; r.grid_counts[1] = ny; r.grid_counts[2] = nz;
        return r; }
    // the grid as fw_probe_irradiance / fw_probe_shade read it; a set made by new_() has none
    fw_probe_grid grid_abi(bool wrap = true) const {
        if (!has_grid) throw std::runtime_error("the probes have no grid: only a ProbeSet made by ProbeSet::grid can be looked up");
        fw_probe_grid g{};
        for (int k = 0; k < 3; k++) { g.lo[k] = grid_lo[k]; g.hi[k] = grid_hi[k]; g.counts[k] = grid_counts[k]; }
        g.flags = wrap ? FW_PROBE_WRAP : 0u; return g; }
    size_t n_probes() const { return positions.size() / 3; }
    ProbeSet seed(uint64_t s) && { seed_ = s; return std::move(*this); }
    ProbeSet jitter(bool on) && { jitter_ = on; return std::move(*this); }
    ProbeSet chunk_probes(uint32_t n) && { chunk = n; return std::move(*this); }
    fw_probe_set abi() const {
        fw_probe_set s{}; s.n_probes = (uint32_t)n_probes(); s.positions = positions.data(); s.directions = directions; s.jitter = jitter_ ? 1 : 0;
        s.seed = seed_; s.chunk_probes = chunk; return s; }
};

// Lowers a Scene to the flat arrays of fw_scene_desc (owning storage for the duration of a render call).
class Lowered {
  public:
    explicit Lowered(const Scene &sc) {
        for (const Material &m : sc.materials) { fw_material fm = m.m; fm.texture = m.tex ? add_texture(*m.tex) : -1; materials.push_back(fm); }
        for (const RenderObject &ro : sc.render_objects) {
            fw_object o{}; o.shape = add_shape(ro.obj); o.position = lower(ro.pos);
            o.rotation = fw_rotor3{ro.rotation.s, ro.rotation.xy, ro.rotation.xz, ro.rotation.yz}; o.flip_normals = ro.flip ? 1 : 0;
            objects.push_back(o); }
        desc.objects = objects.data(); desc.n_objects = (uint32_t)objects.size();
        desc.shapes = shapes.data(); desc.n_shapes = (uint32_t)shapes.size();
        desc.materials = materials.data(); desc.n_materials = (uint32_t)materials.size();
        desc.textures = textures.data(); desc.n_textures = (uint32_t)textures.size();
        desc.environment = sc.environment.e;
    }
    fw_scene_desc desc{};
  private:
    std::vector<fw_object> objects; std::vector<fw_shape> shapes; std::vector<fw_material> materials; std::vector<fw_texture> textures;
    int32_t add_texture(const Texture &t) {
        fw_texture ft = t.t;
        if (ft.kind == FW_TEX_CHECKER) { ft.odd = add_texture(*t.odd); ft.even = add_texture(*t.even); }
        textures.push_back(ft); return (int32_t)textures.size() - 1; }
    int32_t add_shape(const Shape &s) {
        fw_shape fs = s.s;
        if (fs.kind == FW_SHAPE_TRIANGLE_MESH) { fs.verts = s.verts->data(); fs.n_verts = (uint32_t)(s.verts->size() / 3);
            fs.indices = s.indices->data(); fs.n_indices = (uint32_t)s.indices->size();
            fs.normals = s.normals ? s.normals->data() : nullptr; fs.uvs = s.uvs ? s.uvs->data() : nullptr; }
        if (fs.kind == FW_SHAPE_CONSTANT_MEDIUM) fs.inner = add_shape(*s.inner);
        shapes.push_back(fs); return (int32_t)shapes.size() - 1; }
};

// fw_init (ABI v7): the device's one-off costs — HIP context, code objects, kernel handles, the path arena — where the host wants them, i.e.
// before the region it times (main.rs:40-44 starts with the reference's own binary loaded).  Optional: the first render does it otherwise.
inline void init(int device = 0, uint64_t arena_bytes = 0) {
    const int rc = fw_init(device, arena_bytes);
    if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
}

// fw_scene_create, then the scene's lights (fw_scene_set_lights); on failure nothing is left behind
inline int create_resident(const Scene &scene, const fw_scene_desc *desc, int device, fw_scene **out) {
    int rc = fw_scene_create(desc, device, out);
    if (rc == FW_OK && !scene.lights.empty()) {
        rc = fw_scene_set_lights(*out, scene.lights.data(), (uint32_t)scene.lights.size());
        if (rc != FW_OK) { fw_scene_destroy(*out); *out = nullptr; }
    }
    return rc;
}

struct Renderer {   // render.rs:59-218; Default: 1920x1080, 128 spp, multithreaded, no BVH, gamma 2.2
    size_t width_ = 1920, height_ = 1080, samples_ = 128; bool multithreaded_ = true, use_bvh_ = false; float gamma_ = 2.2f;
    CameraSettings camera_; uint64_t seed_ = 0; int device_ = 0; bool light_sampling_ = false, env_sampling_ = false, all_emitters_ = false;
    static Renderer default_() { return {}; }
    Renderer width(size_t w) && { width_ = w; return std::move(*this); }
    Renderer height(size_t h) && { height_ = h; return std::move(*this); }
    Renderer samples(size_t s) && { samples_ = s; return std::move(*this); }
    Renderer multithreaded(bool m) && { multithreaded_ = m; return std::move(*this); }
    Renderer use_bvh(bool b) && { use_bvh_ = b; return std::move(*this); }
    Renderer gamma(float g) && { gamma_ = g; return std::move(*this); }
    Renderer camera(CameraSettings c) && { camera_ = c; return std::move(*this); }
    Renderer seed(uint64_t s) && { seed_ = s; return std::move(*this); }
    Renderer device(int d) && { device_ = d; return std::move(*this); }
    // next-event estimation with MIS at diffuse vertices (FW_FLAG_LIGHT_SAMPLING): the same image in expectation, less noise
    Renderer light_sampling(bool on = true) && { light_sampling_ = on; return std::move(*this); }
    // importance sampling of an HDR environment map at diffuse vertices (FW_FLAG_ENV_SAMPLING)
    Renderer env_sampling(bool on = true) && { env_sampling_ = on; return std::move(*this); }
    // with light_sampling: every emitting primitive (meshes, disks, boxes too) a sampled light, picked by power (FW_FLAG_ALL_EMITTERS, §9i)
    Renderer all_emitters(bool on = true) && { all_emitters_ = on; return std::move(*this); }

    fw_render_params params() const {
        fw_render_params p{}; p.width = (uint32_t)width_; p.height = (uint32_t)height_; p.samples = (uint32_t)samples_; p.gamma = gamma_;
        p.use_bvh = use_bvh_; p.multithreaded = multithreaded_; p.seed = seed_; p.rng_mode = FW_RNG_CTR;
        p.flags = (light_sampling_ ? FW_FLAG_LIGHT_SAMPLING : 0u) | (env_sampling_ ? FW_FLAG_ENV_SAMPLING : 0u) |
                  (all_emitters_ ? FW_FLAG_ALL_EMITTERS : 0u);
        p.camera = fw_camera_settings{lower(camera_.cam_pos_), lower(camera_.look_at_), camera_.vfov, camera_.aperture_, camera_.focus_dist_};
        return p; }

    // The segment-0 rays a render traces for `sample` of every pixel, index order (fw_camera_rays, ABI v8): width*height x 6 floats
    std::vector<float> camera_rays(uint32_t sample = 0) const {
        fw_render_params p = params();
        std::vector<float> rays(width_ * height_ * 6);
        const int rc = fw_camera_rays(&p, device_, sample, rays.data());
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        return rays; }

    // several GPUs from this one process (fw_render_scene_tiled): the image does not depend on the list
    Renderer devices(std::vector<int> d) && { devices_ = std::move(d); return std::move(*this); }
    std::vector<int> devices_;

    // `pub fn render(&self, scene: Scene) -> Vec<Color>` (render.rs:109): row 0 = image top
    std::vector<Color> render(const Scene &scene, fw_stats *stats = nullptr) const {
        Lowered low(scene);
        fw_render_params p = params();
        std::vector<Color> buffer(width_ * height_, Color{0, 0, 0});
        if (!scene.lights.empty() && devices_.empty()) {     // fw_render_scene takes a bare description, which carries no lights: a resident scene does
            fw_scene *sc = nullptr;
            int lrc = create_resident(scene, &low.desc, device_, &sc);
            if (lrc == FW_OK) { lrc = fw_render(sc, &p, reinterpret_cast<uint8_t *>(buffer.data()), nullptr, nullptr, stats); fw_scene_destroy(sc); }
            if (lrc != FW_OK) throw std::runtime_error(std::string(fw_strerror(lrc)) + " | " + fw_last_error());
            return buffer;
        }
        int rc = devices_.empty()
                     ? fw_render_scene(&low.desc, &p, device_, reinterpret_cast<uint8_t *>(buffer.data()), nullptr, nullptr, stats)
                     : fw_render_scene_tiled(&low.desc, &p, devices_.data(), (int)devices_.size(), reinterpret_cast<uint8_t *>(buffer.data()), nullptr, nullptr, stats);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());   // the reference panics here
        return buffer; }

    // Progressive preview (not in the reference): `passes` passes over the samples, `on_pass(k, image)` after each; `accum`
    // (width*height*4 floats) may be kept by the caller as a checkpoint.  The last image equals render()'s bit for bit.
    template <class F>
    std::vector<Color> render_progressive(const Scene &scene, size_t passes, F on_pass, std::vector<float> *accum_io = nullptr) const {
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        std::vector<float> local; std::vector<float> &accum = accum_io ? *accum_io : local;
        accum.assign(width_ * height_ * 4, 0.f);
        std::vector<Color> buffer(width_ * height_, Color{0, 0, 0});
        passes = std::max<size_t>(1, std::min(passes, samples_));
        for (size_t k = 0; k < passes; k++) {
            const size_t lo = samples_ * k / passes, hi = samples_ * (k + 1) / passes;
            if (hi == lo) continue;
            fw_render_params p = params(); p.samples = (uint32_t)(hi - lo);
            rc = fw_render_progressive(sc, &p, (uint32_t)lo, accum.data(), reinterpret_cast<uint8_t *>(buffer.data()), nullptr, nullptr, nullptr);
            if (rc != FW_OK) { fw_scene_destroy(sc); throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error()); }
            on_pass(k, buffer);
        }
        fw_scene_destroy(sc);
        return buffer; }

    // Adaptive sampling (not in the reference; fw_render_adaptive): every pixel gets min_samples samples, then the pixels whose standard
    // error is above tolerance x their brightness go on in rounds that double their count, up to samples().  Each pixel equals render() at
    // its final count bit for bit; `counts` (if given) receives those counts, width*height in index order.
    std::vector<Color> render_adaptive(const Scene &scene, float tolerance, uint32_t min_samples, std::vector<uint32_t> *counts = nullptr,
                                       fw_stats *stats = nullptr) const {
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        fw_render_params p = params();
        std::vector<Color> buffer(width_ * height_, Color{0, 0, 0});
        std::vector<float> moments(counts ? width_ * height_ * 4 : 0);
        rc = fw_render_adaptive(sc, &p, tolerance, min_samples, nullptr, counts ? moments.data() : nullptr, reinterpret_cast<uint8_t *>(buffer.data()),
                                nullptr, nullptr, nullptr, stats);
        fw_scene_destroy(sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        if (counts) { counts->resize(width_ * height_); for (size_t i = 0; i < counts->size(); i++) (*counts)[i] = (uint32_t)moments[4 * i + 3]; }
        return buffer; }

    // Several camera views in one call (not in the reference; fw_render_views): view v equals render() with camera cameras[v] bit for bit;
    // this renderer's own camera is not used.  One buffer of width*height colours per view.
    std::vector<std::vector<Color>> render_views(const Scene &scene, const std::vector<CameraSettings> &cameras, fw_stats *stats = nullptr) const {
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        fw_render_params p = params();
        std::vector<fw_camera_settings> cams;
        for (const CameraSettings &c : cameras) cams.push_back(fw_camera_settings{lower(c.cam_pos_), lower(c.look_at_), c.vfov, c.aperture_, c.focus_dist_});
        const size_t n = width_ * height_;
        std::vector<Color> all(cams.size() * n, Color{0, 0, 0});
        rc = fw_render_views(sc, &p, cams.data(), (uint32_t)cams.size(), reinterpret_cast<uint8_t *>(all.data()), nullptr, nullptr, stats);
        fw_scene_destroy(sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        std::vector<std::vector<Color>> views;
        for (size_t v = 0; v < cams.size(); v++) views.emplace_back(all.begin() + v * n, all.begin() + (v + 1) * n);
        return views; }

    // A CameraModel rendered on the device (not in the reference; fw_render_model): samples() samples of every pixel of the model's image
    // (its own width x height; this renderer's camera and size are not used), the rays generated on the GPU chunk by chunk of samples.
    std::vector<Color> render_model(const Scene &scene, const CameraModel &model, fw_stats *stats = nullptr) const {
        const uint64_t n_rays = (uint64_t)model.m.width * model.m.height;
        if (n_rays >= (1ull << 31))      // fw_render_model's own limit; n_rays is 32-bit, so the library could not even be told the size
            throw std::runtime_error(std::string(fw_strerror(FW_ERR_UNSUPPORTED)) + " | W x H must be below 2^31");
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        const fw_render_params p = params();
        fw_render_rays_params rp{};
        rp.n_rays = (uint32_t)n_rays; rp.samples = p.samples; rp.per_sample_rays = 1; rp.seed = p.seed; rp.use_bvh = p.use_bvh;
        rp.gamma = p.gamma; rp.flags = p.flags;
        std::vector<Color> buffer((size_t)n_rays, Color{0, 0, 0});
        rc = fw_render_model(sc, &model.m, &rp, nullptr, reinterpret_cast<uint8_t *>(buffer.data()), nullptr, nullptr, stats);
        fw_scene_destroy(sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        return buffer; }

    // Irradiance probes baked on the device (not in the reference; fw_bake_probes): `rounds` rounds of the set's rays, samples() paths per
    // direction and round, with this renderer's seed, use_bvh and flags (its camera, size and gamma are not used).  Returns sh, n x 9 x 3
    // floats: the mean of the rounds' projections; sums (optional, n x 9 x 3) receives the running sums.
    std::vector<float> bake_probes(const Scene &scene, const ProbeSet &probes, uint32_t rounds = 1, std::vector<float> *sums = nullptr,
                                   fw_stats *stats = nullptr) const {
        if (probes.n_probes() >= (1ull << 32))
            throw std::runtime_error(std::string(fw_strerror(FW_ERR_UNSUPPORTED)) + " | n_probes x directions must be below 2^31");
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        const fw_render_params p = params();
        fw_render_rays_params rp{};
        rp.samples = p.samples; rp.seed = p.seed; rp.use_bvh = p.use_bvh; rp.gamma = p.gamma; rp.flags = p.flags;
        const fw_probe_set set = probes.abi();
        std::vector<float> sh(probes.n_probes() * 27), acc(probes.n_probes() * 27, 0.f);
        rc = fw_bake_probes(sc, &set, &rp, 0, rounds, acc.data(), sh.data(), stats);
        fw_scene_destroy(sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        if (sums) *sums = std::move(acc);
        return sh; }

    // A preview lit from baked probes (not in the reference; fw_render_aovs + fw_probe_shade): the first-hit guide buffers of this view at
    // aov_samples samples, shaded from the grid `probes` (made by ProbeSet::grid) and its coefficients sh (n x 9 x 3, as bake_probes
    // returns them): out = albedo (coverage max(E, 0) / pi + (1 - coverage)).  One first-hit pass and no paths; direct and indirect diffuse
    // light both come from the probes.  wrap: FW_PROBE_WRAP, the guard against probes behind the surface.
    std::vector<Color> probe_lit(const Scene &scene, const ProbeSet &probes, const std::vector<float> &sh, uint32_t aov_samples = 8, bool wrap = true,
                                 fw_stats *stats = nullptr) const {
        const fw_probe_grid grid = probes.grid_abi(wrap);
        if (sh.size() != probes.n_probes() * 27) throw std::runtime_error("sh must hold 9 x 3 coefficients per probe");
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        fw_render_params p = params();
        p.samples = aov_samples;
        const size_t n = width_ * height_;
        std::vector<float> aov(n * 12);
        rc = fw_render_aovs(sc, &p, aov.data(), stats);
        fw_scene_destroy(sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        fw_probe_shade_params sp{(uint32_t)width_, (uint32_t)height_, p.gamma, device_, 0, nullptr};
        std::vector<Color> buffer(n, Color{0, 0, 0});
        rc = fw_probe_shade(&grid, sh.data(), &sp, aov.data(), nullptr, nullptr, reinterpret_cast<uint8_t *>(buffer.data()));
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        return buffer; }

    // A denoised frame (not in the reference): samples() samples per pixel filtered by fw_denoise with `iterations` a-trous steps, guided by
    // fw_render_aovs at aov_samples samples.  The frame comes from fw_render_adaptive with min_samples = samples() (one round at the fixed
    // count: fw_render's frame bit for bit, and its moments drive the filter's luminance term), or from fw_render below 2 samples.
    std::vector<Color> render_denoised(const Scene &scene, uint32_t iterations = FW_DENOISE_ITERATIONS, uint32_t aov_samples = 8,
                                       fw_stats *stats = nullptr) const {
        Lowered low(scene);
        fw_scene *sc = nullptr;
        int rc = create_resident(scene, &low.desc, device_, &sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        fw_render_params p = params();
        const size_t n = width_ * height_;
        std::vector<float> linear(n * 3), moments(n * 4), aov(n * 12);
        rc = p.samples >= 2 ? fw_render_adaptive(sc, &p, 1.0f, p.samples, nullptr, moments.data(), nullptr, nullptr, linear.data(), nullptr, stats)
                            : fw_render(sc, &p, nullptr, nullptr, linear.data(), stats);
        if (rc == FW_OK) {
            fw_render_params pa = p;
            pa.samples = aov_samples;
            rc = fw_render_aovs(sc, &pa, aov.data(), nullptr);
        }
        fw_scene_destroy(sc);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        fw_denoise_params dp{(uint32_t)width_, (uint32_t)height_, iterations, p.gamma, device_, 0, nullptr};
        std::vector<Color> buffer(n, Color{0, 0, 0});
        rc = fw_denoise(&dp, linear.data(), aov.data(), p.samples >= 2 ? moments.data() : nullptr, nullptr, nullptr,
                        reinterpret_cast<uint8_t *>(buffer.data()));
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        return buffer; }
};

// Ray queries (ABI v8, not in the reference): a scene uploaded once, and `Hitable::hit(ray, 0.001, 2e9)` (render.rs:19,44-57) for the
// caller's rays — picking, depth / normal / ID buffers, visibility.  See fw_trace_rays for the contract.
class DeviceScene {
  public:
    explicit DeviceScene(const Scene &scene, int device = 0) {
        Lowered low(scene);                      // fw_scene_create copies what it needs
        const int rc = create_resident(scene, &low.desc, device, &sc_);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
    }
    ~DeviceScene() { if (sc_) fw_scene_destroy(sc_); }
    DeviceScene(const DeviceScene &) = delete;
    DeviceScene &operator=(const DeviceScene &) = delete;
    // rays: n x 6 floats (origin, direction) -> one fw_hit per ray (object == FW_NO_HIT: a miss)
    std::vector<fw_hit> trace(const std::vector<float> &rays, bool use_bvh, uint64_t seed = 0, uint32_t key_base = 0, fw_stats *stats = nullptr) const {
        fw_trace_params p{}; p.use_bvh = use_bvh ? 1 : 0; p.seed = seed; p.key_base = key_base;
        std::vector<fw_hit> hits(rays.size() / 6);
        const int rc = fw_trace_rays(sc_, &p, rays.data(), (uint32_t)hits.size(), hits.data(), stats);
        if (rc != FW_OK) throw std::runtime_error(std::string(fw_strerror(rc)) + " | " + fw_last_error());
        return hits; }
  private:
    fw_scene *sc_ = nullptr;
};

// window.rs:59-66 `save_image` (binary PPM: no PNG encoder is linked into this header)
inline void save_image_ppm(const std::vector<Color> &render, const std::string &path, size_t width, size_t height) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("Failed to save image to " + path);
    std::fprintf(f, "P6\n%zu %zu\n255\n", width, height);
    std::fwrite(render.data(), 3, width * height, f);
    std::fclose(f);
}

} // namespace firework
