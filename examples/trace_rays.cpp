// examples/trace_rays.cpp — ray queries on include/firework.hpp: the first hit of every camera ray of a cornell box
// (cornell_box.rs's scene and camera), i.e. the depth / normal / object-ID buffer of sample 0.
// usage: trace_rays out.bin [width height]   writes width*height fw_hit records (48 bytes each, index order) to out.bin
#include "firework.hpp"

#include <cstdio>
#include <cstdlib>

using namespace firework;

static float to_radians(float deg) { return deg * RADS_PER_DEG; }

static Scene cornell_box() {   // cornell_box.rs:10-48
    Scene world = Scene::new_();
    MaterialIdx red = world.add_material(LambertianMat::with_color({0.65f, 0.05f, 0.05f}));
    MaterialIdx white = world.add_material(LambertianMat::with_color({0.73f, 0.73f, 0.73f}));
    MaterialIdx green = world.add_material(LambertianMat::with_color({0.12f, 0.45f, 0.15f}));
    MaterialIdx light = world.add_material(EmissiveMat::with_color({15.f, 15.f, 15.f}));
    world.add_object(RenderObject::new_(XZRect::new_(213.f, 343.f, 227.f, 332.f, 554.f, light)));
    world.add_object(RenderObject::new_(YZRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, green)).flip_normals());
    world.add_object(RenderObject::new_(YZRect::new_(0.f, 555.f, 0.f, 555.f, 0.f, red)));
    world.add_object(RenderObject::new_(XZRect::new_(0.f, 555.f, 0.f, 555.f, 0.f, white)));
    world.add_object(RenderObject::new_(XZRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, white)).flip_normals());
    world.add_object(RenderObject::new_(XYRect::new_(0.f, 555.f, 0.f, 555.f, 555.f, white)).flip_normals());
    world.add_object(RenderObject::new_(Rect3d::with_size({165.f, 165.f, 165.f}, white))
                         .rotate(Rotor3::from_rotation_xz(to_radians(18.f)))
                         .position(130.f, 0.f, 65.f));
    world.add_object(RenderObject::new_(Rect3d::with_size({165.f, 330.f, 165.f}, white))
                         .rotate(Rotor3::from_rotation_xz(to_radians(-15.f)))
                         .position(265.f, 0.f, 295.f));
    return world;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: trace_rays out.bin [width height]\n"); return 2; }
    const size_t width = argc > 3 ? strtoul(argv[2], nullptr, 10) : 64, height = argc > 3 ? strtoul(argv[3], nullptr, 10) : 64;
    CameraSettings camera = CameraSettings::default_().cam_pos({278.f, 278.f, -800.f}).look_at({278.f, 278.f, 0.f}).field_of_view(40.f);
    Renderer renderer = Renderer::default_().width(width).height(height).samples(1).camera(camera);
    try {
        DeviceScene scene(cornell_box());
        const std::vector<fw_hit> hits = scene.trace(renderer.camera_rays(0), false);
        size_t n_hit = 0;
        for (const fw_hit &h : hits) n_hit += h.object != FW_NO_HIT;
        FILE *f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(hits.data(), sizeof(fw_hit), hits.size(), f) != hits.size()) { std::fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
        std::fclose(f);
        std::printf("rays=%zu hits=%zu\n", hits.size(), n_hit);
    }
    catch (const std::exception &e) { std::fprintf(stderr, "trace failed: %s\n", e.what()); return 1; }
    return 0;
}
