// GPU checks of image textures on user scenes built with the host scene API
// (compiled and run by tests/test_gpu_image_texture.py on the GPU box; no
// oracle: the C oracle knows no image texture).
//
//   gpu_image_scene identity
//       A Cornell-like box whose white walls and blocks use a 3x5 image with
//       every texel (186, 186, 186), and the same box with
//       constant_texture(vec3(186 / 255.0)) instead.  Both light lists hold
//       one more sphere (never in the world) whose material carries the
//       image: its geometry steers light sampling in both scenes alike, its
//       material is never shaded, so the constant scene holds an image it
//       never looks up and runs the same SF_IMAGE kernel.  Prints the kernel
//       names, the traversal counts and whether the radiance sums are
//       bit-identical (in every execution form the caller selects through
//       RTW_MODE / RTW_SPLIT).
//   gpu_image_scene identity_gbvh
//       The same pair with a list of twelve more balls on the floor, flattened
//       with BVHs: the list becomes a group BVH, a feature set without a
//       persistent or fused image kernel, so the render must fall back to the
//       split k_intersect / k_shade pair and still look the image up.  Also
//       prints the status of an fp32 render of it, which has no kernel
//       (RTW_ERR_UNSUPPORTED, not a picture without the image).
//   gpu_image_scene emitter
//       A pinhole camera at the origin looking down +z at one diffuse_light
//       xy_rect (normal +z: it emits along the rays) with a 4x2 image, larger
//       than the view, black background; 32x16, 8 spp, depth 2.  Prints the
//       camera, the rect, the image, the GPU's radiance sums and the sums the
//       host classes give for the same samples.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>
#include "rtw/scene.h"
#include "rtw_gpu.h"

namespace {
using pixels = std::shared_ptr<image_texture::byte_array>;

class box_scene : public scene {
public:
    box_scene(double aspect, bool image, bool cluster = false) {
        auto solid = [](double r, double g, double b) { return std::make_shared<constant_texture>(vec3(r, g, b)); };
        pixels grey = std::make_shared<image_texture::byte_array>(3 * 3 * 5, (image_texture::byte)186);
        std::shared_ptr<texture> img = std::make_shared<image_texture>(grey, 3, 5);
        std::shared_ptr<texture> flat = solid(186 / 255.0, 186 / 255.0, 186 / 255.0);
        auto white = std::make_shared<lambertian>(image ? img : flat);
        auto red = std::make_shared<lambertian>(solid(0.65, 0.05, 0.05));
        auto green = std::make_shared<lambertian>(solid(0.12, 0.45, 0.15));
        auto light = std::make_shared<diffuse_light>(solid(15.0, 15.0, 15.0));
        const double L = 555.0;
        auto lamp = std::make_shared<xz_rect>(213.0, 343.0, 227.0, 332.0, 554.0, light);
        Add(lamp);
        lights->objects.push_back(lamp);
        Add(std::make_shared<flip_normals>(std::make_shared<yz_rect>(0.0, L, 0.0, L, L, green)));
        Add(std::make_shared<yz_rect>(0.0, L, 0.0, L, 0.0, red));
        Add(std::make_shared<flip_normals>(std::make_shared<xz_rect>(0.0, L, 0.0, L, L, white)));
        Add(std::make_shared<xz_rect>(0.0, L, 0.0, L, 0.0, white));
        Add(std::make_shared<flip_normals>(std::make_shared<xy_rect>(0.0, L, 0.0, L, L, white)));
        Add(std::make_shared<sphere>(vec3(190, 90, 190), 90, white));
        auto tall = std::make_shared<box>(vec3(0.0, 0.0, 0.0), vec3(165.0, 330.0, 165.0), white);
        Add(std::make_shared<translate>(std::make_shared<rotate_y>(tall, 15.0), vec3(265.0, 0.0, 295.0)));
        if (cluster) {  // more than eight prims in one entry: a group BVH with use_bvh
            std::vector<std::shared_ptr<hittable>> balls;
            for (int k = 0; k < 12; ++k)
                balls.push_back(std::make_shared<sphere>(vec3(60.0 + 40.0 * k, 20.0, 60.0 + 7.0 * (k % 5)), 20.0, white));
            Add(std::make_shared<hittable_list>(balls));
        }
        // in the light list only: an image in the desc that no hit ever reads
        lights->objects.push_back(std::make_shared<sphere>(vec3(400, 400, 150), 40, std::make_shared<lambertian>(img)));
        cam = camera(vec3(278.0, 278.0, -800.0), vec3(278.0, 278.0, 0.0), vec3(0, 1, 0), 40.0, aspect, 0.0, 10.0, 0.0,
                     1.0);
        background_type = BackgroundType::Black;
    }
};

const double kRect[5] = {-1.3, 1.25, -0.7, 0.66, 1.0};  // x0 x1 y0 y1 k

class emitter_scene : public scene {
public:
    pixels px;
    explicit emitter_scene(double aspect) {
        px = std::make_shared<image_texture::byte_array>(3 * 4 * 2);
        for (int k = 0; k < 24; ++k) (*px)[k] = (image_texture::byte)((41 * k + 23) & 255);
        auto glow = std::make_shared<diffuse_light>(std::make_shared<image_texture>(px, 4, 2));
        Add(std::make_shared<xy_rect>(kRect[0], kRect[1], kRect[2], kRect[3], kRect[4], glow));
        cam = camera(vec3(0, 0, 0), vec3(0, 0, 1), vec3(0, 1, 0), 60.0, aspect, 0.0, 1.0, 0.0, 1.0);
        background_type = BackgroundType::Black;
    }
};

struct gpu_result {
    std::vector<double> sums;
    unsigned long long segments = 0;
    std::string kernel;
    int shade_mask = 0;
    int features = 0;
    int fp32_status = 0;  // of a precision = fp32 render (try_fp32)
};

bool gpu_render(const scene& sc, int nx, int ny, int spp, int depth, uint64_t seed, gpu_result& out, int bvh = 0,
                bool try_fp32 = false) {
    rtw_scene_desc* d = nullptr;
    if (rtw_flatten_scene(sc, bvh, &d) != RTW_OK) {
        std::printf("flatten failed: %s\n", rtw_last_error());
        return false;
    }
    void* h = nullptr;
    if (rtw_scene_upload(0, d, &h) != RTW_OK) {
        std::printf("upload failed: %s\n", rtw_last_error());
        return false;
    }
    rtw_scene_info info;
    if (rtw_scene_query(h, &info) != RTW_OK) {
        std::printf("query failed: %s\n", rtw_last_error());
        return false;
    }
    out.kernel = info.kernel;
    out.shade_mask = info.shade_mask;
    out.features = info.features;
    const rtw_camera_desc cam = sc.GetCamera().desc();
    rtw_render_params p;
    std::memset(&p, 0, sizeof p);
    p.nx = nx, p.ny = ny, p.spp = spp, p.max_depth = depth, p.seed = seed, p.row_step = 1;
    out.sums.assign((size_t)nx * ny * 3, 0.0);
    rtw_stats st;
    if (rtw_render_accumulate(h, &cam, &p, out.sums.data(), &st) != RTW_OK) {
        std::printf("render failed: %s\n", rtw_last_error());
        return false;
    }
    out.segments = st.segments;
    if (try_fp32) {
        std::vector<double> scratch(out.sums.size(), 0.0);
        p.precision = RTW_PRECISION_FP32;
        out.fp32_status = rtw_render_accumulate(h, &cam, &p, scratch.data(), &st);
    }
    rtw_scene_free(h);
    rtw_scene_desc_free(d);
    return true;
}

void print_row(const char* tag, const double* v, size_t n) {
    std::printf("%s", tag);
    for (size_t k = 0; k < n; ++k) std::printf(" %.17g", v[k]);
    std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "identity" || mode == "identity_gbvh") {
        const int nx = 32, ny = 32, spp = 8, depth = 20;
        const bool g = mode == "identity_gbvh";
        gpu_result a, b;
        if (!gpu_render(box_scene(1.0, true, g), nx, ny, spp, depth, 5, a, g, g)) return 1;
        if (!gpu_render(box_scene(1.0, false, g), nx, ny, spp, depth, 5, b, g)) return 1;
        std::printf("features %d %d\nfp32_status %d\n", a.features, b.features, a.fp32_status);
        double md = 0, total = 0;
        bool finite = true;
        for (size_t k = 0; k < a.sums.size(); ++k) {
            md = std::fmax(md, std::fabs(a.sums[k] - b.sums[k]));
            total += a.sums[k];
            finite = finite && std::isfinite(a.sums[k]);
        }
        std::printf("kernel_image %s\nkernel_const %s\n", a.kernel.c_str(), b.kernel.c_str());
        std::printf("shade_mask %d %d\n", a.shade_mask, b.shade_mask);
        std::printf("segments %llu %llu\n", a.segments, b.segments);
        std::printf("identical %d\n", std::memcmp(a.sums.data(), b.sums.data(), a.sums.size() * sizeof(double)) == 0);
        std::printf("maxdiff %.17g\ntotal %.17g\nfinite %d\n", md, total, finite ? 1 : 0);
        return 0;
    }
    if (mode == "emitter") {
        const int nx = 32, ny = 16, spp = 8, depth = 2;
        const uint64_t seed = 3;
        emitter_scene sc(double(nx) / double(ny));
        gpu_result g;
        if (!gpu_render(sc, nx, ny, spp, depth, seed, g)) return 1;
        // the host classes on the same samples (tests/cpp/host_render.cpp's
        // loop; a diffuse_light never scatters, so color() is `emitted`)
        std::vector<double> host((size_t)nx * ny * 3, 0.0);
        std::uniform_real_distribution<double> uniform;
        rtw::engine engine;
        camera& cam = sc.GetCamera();
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                vec3 sum(0, 0, 0);
                for (int s = 0; s < spp; ++s) {
                    rtw::path_stream stream(seed, (uint32_t)(j * nx + i), (uint32_t)s);
                    const double u = double(i + uniform(engine)) / double(nx);
                    const double v = double(j + uniform(engine)) / double(ny);
                    const ray r = cam.get_ray(u, v);
                    hit_record rec;
                    if (!sc.GetWorld().hit(r, 0.001f, std::numeric_limits<double>::max(), rec)) continue;
                    scatter_record srec;
                    if (rec.mat_ptr->scatter(r, rec, srec)) return 1;
                    sum += rec.mat_ptr->emitted(r, rec, rec.u, rec.v, rec.p);
                }
                double* o = &host[((size_t)j * nx + i) * 3];
                o[0] = sum.x, o[1] = sum.y, o[2] = sum.z;
            }
        const rtw_camera_desc cd = cam.desc();
        std::printf("size %d %d %d\n", nx, ny, spp);
        std::printf("kernel %s\n", g.kernel.c_str());
        std::printf("segments %llu\n", g.segments);
        print_row("origin", cd.origin, 3);
        print_row("lower_left", cd.lower_left, 3);
        print_row("horizontal", cd.horizontal, 3);
        print_row("vertical", cd.vertical, 3);
        print_row("rect", kRect, 5);
        std::printf("image 4 2");
        for (auto b : *sc.px) std::printf(" %d", (int)b);
        std::printf("\n");
        print_row("gpu", g.sums.data(), g.sums.size());
        print_row("host", host.data(), host.size());
        return 0;
    }
    std::fprintf(stderr, "usage: gpu_image_scene identity|identity_gbvh|emitter\n");
    return 2;
}
