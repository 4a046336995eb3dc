// scenes.cpp — the reference's scenes, rebuilt with the host scene API.
//
// Each constructor produces the same objects, in the same list order, with the
// same fp64 constants (float literals widened exactly as the reference's are)
// as Scene/scene.h.  Tests compare the flattened result field by field with a
// dump of the reference's own scene graph (tests/golden/scene_*.json).
#include <cmath>
#include <random>
#include "rtw/scene.h"

namespace {
using tex_ptr = std::shared_ptr<texture>;
using mat_ptr = std::shared_ptr<material>;

tex_ptr solid(double r, double g, double b) { return std::make_shared<constant_texture>(vec3(r, g, b)); }
mat_ptr diffuse(double r, double g, double b) { return std::make_shared<lambertian>(solid(r, g, b)); }

camera look(const vec3& from, const vec3& at, double vfov, double aspect, double aperture, double focus) {
    return camera(from, at, vec3(0.0, 1.0, 0.0), vfov, aspect, aperture, focus, 0.0, 1.0);
}
}  // namespace

// Scene/scene.h:42-70 — Perlin ground, Perlin ball, a light ball and a light
// quad; no explicit light list (so no light sampling).
light_sample::light_sample(double aspect) {
    tex_ptr marble = std::make_shared<noise_texture>(4.0);
    tex_ptr four = solid(4, 4, 4);
    std::vector<std::shared_ptr<hittable>> objs = {
        std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, std::make_shared<lambertian>(marble)),
        std::make_shared<sphere>(vec3(0, 2, 0), 2.0, std::make_shared<lambertian>(marble)),
        std::make_shared<sphere>(vec3(0, 7, 0), 2.0, std::make_shared<diffuse_light>(four)),
        std::make_shared<xy_rect>(3.0, 5.0, 1.0, 3.0, -2.0, std::make_shared<diffuse_light>(four)),
    };
    world = hittable_list(objs);
    const vec3 from(24, 5, 5), at(0, 3, 0);
    cam = look(from, at, 20.0, aspect, 0.2f, (from - at).length());
}

// Scene/scene.h:72-96 — the Book 1 material test (hollow glass via r < 0).
dielectric_scene::dielectric_scene(double aspect) {
    Add(std::make_shared<sphere>(vec3(0, 0, -1), 0.5f, diffuse(0.1f, 0.2f, 0.5f)));
    Add(std::make_shared<sphere>(vec3(0, -100.5f, -1), 100.0, diffuse(0.8f, 0.8f, 0.0)));
    Add(std::make_shared<sphere>(vec3(1, 0, -1), 0.5f, std::make_shared<metal>(vec3(0.8f, 0.6f, 0.2f), 0.0)));
    Add(std::make_shared<sphere>(vec3(-1, 0, -1), 0.5f, std::make_shared<dielectric>(1.5f)));
    Add(std::make_shared<sphere>(vec3(-1, 0, -1), -0.45f, std::make_shared<dielectric>(1.5f)));
    cam = look(vec3(0, 0, 0), vec3(0, 0, -1), 120.0, aspect, 0.0, 10.0);
}

// Scene/scene.h:98-174 — Book 1's cover: a 22x22 grid of jittered small
// balls (moving lambertian / metal / glass) and three big ones.  The layout
// comes from one default-seeded minstd_rand, drawn in the reference's order;
// the reference computes `vec3 center(a + 0.9f*U, 0.2f, b + 0.9f*U)` and g++
// evaluates those arguments right to left, so the z jitter is drawn first.
random_balls_scene::random_balls_scene(double aspect) {
    std::uniform_real_distribution<double> U;
    std::minstd_rand eng;

    Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, diffuse(0.5f, 0.5f, 0.5f)));

    const vec3 keep_clear(4.0, 0.2f, 0.0);
    for (int a = -11; a < 11; ++a) {
        for (int b = -11; b < 11; ++b) {
            const double pick = U(eng);
            const double jz = U(eng);
            const double jx = U(eng);
            const vec3 c(a + 0.9f * jx, 0.2f, b + 0.9f * jz);
            if (!((c - keep_clear).length() > 0.9f)) continue;

            if (pick < 0.8f) {
                vec3 albedo;
                albedo.r = U(eng) * U(eng);
                albedo.g = U(eng) * U(eng);
                albedo.b = U(eng) * U(eng);
                auto ball = std::make_shared<moving_sphere>(c, 0.2f,
                    std::make_shared<lambertian>(std::make_shared<constant_texture>(albedo)));
                movement_linear path;
                path.center1 = c + vec3(0.0, 0.5f * U(eng), 0.0);
                path.time0 = 0.0;
                path.time1 = 1.0;
                ball->set_movement(path);
                Add(ball);
            } else if (pick < 0.95) {
                vec3 albedo;
                albedo.r = 0.5f * (1 + U(eng));
                albedo.g = 0.5f * (1 + U(eng));
                albedo.b = 0.5f * (1 + U(eng));
                const double fuzz = 0.5f * U(eng);
                Add(std::make_shared<sphere>(c, 0.2f, std::make_shared<metal>(albedo, fuzz)));
            } else {
                const double glass = 1.5f;
                Add(std::make_shared<sphere>(c, 0.2f, std::make_shared<dielectric>(glass)));
            }
        }
    }

    Add(std::make_shared<sphere>(vec3(0, 1, 0), 1.0, std::make_shared<dielectric>(1.5f)));
    Add(std::make_shared<sphere>(vec3(-4, 1, 0), 1.0, diffuse(0.4f, 0.2f, 0.1f)));
    Add(std::make_shared<sphere>(vec3(4, 1, 0), 1.0, std::make_shared<metal>(vec3(0.7f, 0.6f, 0.5f), 0.0)));

    cam = look(vec3(13, 2, 3), vec3(0, 0, 0), 20.0, aspect, 0.0, 10.0);
}

// Scene/scene.h:176-250 — Cornell box, glass-sphere variant (the `#if 1`
// block at :453-459): light quad, five walls, glass ball, tall rotated box.
// lights = { light quad, glass ball } drive the mixture-pdf sampling.
cornell_box_scene::cornell_box_scene(double aspect) {
    auto red = diffuse(0.65f, 0.05f, 0.05f);
    auto white = diffuse(0.73f, 0.73f, 0.73f);
    auto green = diffuse(0.12f, 0.45f, 0.15f);
    auto light = std::make_shared<diffuse_light>(solid(15.0, 15.0, 15.0));

    std::vector<std::shared_ptr<hittable>> objs;
    auto lamp = std::make_shared<xz_rect>(213.0, 343.0, 227.0, 332.0, 554.0, light);
    objs.push_back(lamp);
    lights->objects.push_back(lamp);

    const double L = 555.0;
    objs.push_back(std::make_shared<flip_normals>(std::make_shared<yz_rect>(0.0, L, 0.0, L, L, green)));
    objs.push_back(std::make_shared<yz_rect>(0.0, L, 0.0, L, 0.0, red));
    objs.push_back(std::make_shared<flip_normals>(std::make_shared<xz_rect>(0.0, L, 0.0, L, L, white)));
    objs.push_back(std::make_shared<xz_rect>(0.0, L, 0.0, L, 0.0, white));
    objs.push_back(std::make_shared<flip_normals>(std::make_shared<xy_rect>(0.0, L, 0.0, L, L, white)));

    auto ball = std::make_shared<sphere>(vec3(190, 90, 190), 90, std::make_shared<dielectric>(1.5));
    objs.push_back(ball);
    lights->objects.push_back(ball);

    auto tall = std::make_shared<box>(vec3(0.0, 0.0, 0.0), vec3(165.0, 330.0, 165.0), white);
    objs.push_back(std::make_shared<translate>(std::make_shared<rotate_y>(tall, 15.0), vec3(265.0, 0.0, 295.0)));

    world = hittable_list(objs);
    cam = look(vec3(278.0, 278.0, -800.0), vec3(278.0, 278.0, 0.0), 40.0, aspect, 0.0, 10.0);
    background_type = BackgroundType::Black;
}

// Book 2 "The Next Week" final scene.  Not in the reference;
// composed from the reference's classes, as oracle/ref_harness.cpp does:
// 20x20 ground boxes, a light quad, a moving ball, glass and metal balls, a
// blue smoke ball inside a glass ball, global thin fog, a constant-colour
// ball where the book maps earth.jpg, a Perlin marble ball, and 1000 small
// balls in a rotated, translated cluster.  Random layout from one
// default-seeded minstd_rand, drawn in the order written below.
book2_final_scene::book2_final_scene(double aspect) {
    std::uniform_real_distribution<double> U;
    std::minstd_rand eng;
    auto between = [&](double lo, double hi) { return lo + (hi - lo) * U(eng); };

    auto ground = diffuse(0.48, 0.83, 0.53);
    std::vector<std::shared_ptr<hittable>> boxes1;
    for (int i = 0; i < 20; ++i) {
        for (int j = 0; j < 20; ++j) {
            const double w = 100.0;
            const double x0 = -1000.0 + i * w, z0 = -1000.0 + j * w;
            const double y1 = between(1, 101);
            boxes1.push_back(std::make_shared<box>(vec3(x0, 0.0, z0), vec3(x0 + w, y1, z0 + w), ground));
        }
    }
    Add(std::make_shared<hittable_list>(boxes1));

    auto lamp = std::make_shared<xz_rect>(123.0, 423.0, 147.0, 412.0, 554.0,
                                          std::make_shared<diffuse_light>(solid(7, 7, 7)));
    Add(lamp);
    lights->objects.push_back(lamp);

    const vec3 c0(400, 400, 200);
    auto mover = std::make_shared<moving_sphere>(c0, 50.0, diffuse(0.7, 0.3, 0.1));
    movement_linear path;
    path.center1 = c0 + vec3(30, 0, 0);
    path.time0 = 0.0;
    path.time1 = 1.0;
    mover->set_movement(path);
    Add(mover);

    Add(std::make_shared<sphere>(vec3(260, 150, 45), 50.0, std::make_shared<dielectric>(1.5)));
    Add(std::make_shared<sphere>(vec3(0, 150, 145), 50.0, std::make_shared<metal>(vec3(0.8, 0.8, 0.9), 1.0)));

    auto shell = std::make_shared<sphere>(vec3(360, 150, 145), 70.0, std::make_shared<dielectric>(1.5));
    Add(shell);
    Add(std::make_shared<constant_medium>(shell, 0.2, std::make_shared<isotropic>(solid(0.2, 0.4, 0.9))));
    auto fog = std::make_shared<sphere>(vec3(0, 0, 0), 5000.0, std::make_shared<dielectric>(1.5));
    Add(std::make_shared<constant_medium>(fog, 0.0001, std::make_shared<isotropic>(solid(1, 1, 1))));

    Add(std::make_shared<sphere>(vec3(400, 200, 400), 100.0, diffuse(0.2, 0.3, 0.6)));
    Add(std::make_shared<sphere>(vec3(220, 280, 300), 80.0,
                                 std::make_shared<lambertian>(std::make_shared<noise_texture>(0.1))));

    auto white = diffuse(0.73, 0.73, 0.73);
    std::vector<std::shared_ptr<hittable>> cluster;
    for (int k = 0; k < 1000; ++k) {
        const double z = between(0, 165);
        const double y = between(0, 165);
        const double x = between(0, 165);
        cluster.push_back(std::make_shared<sphere>(vec3(x, y, z), 10.0, white));
    }
    Add(std::make_shared<translate>(std::make_shared<rotate_y>(std::make_shared<hittable_list>(cluster), 15.0),
                                    vec3(-100, 270, 395)));

    cam = look(vec3(478, 278, -600), vec3(278, 278, 0), 40.0, aspect, 0.0, 10.0);
    background_type = BackgroundType::Black;
}

// A test scene for arbitrary nesting (not in the reference; composed the
// same way in oracle/ref_harness.cpp from the reference's classes): the
// Cornell room, then instanced boxes inside a list, a flip over a list
// holding a transformed rect, a medium inside a nested list, a medium inside
// a translated list, lists two deep under rotate_y / translate, and a flip
// over a list holding a bare and a translated rect.  "nested_plain" drops
// the media (world runs instead of the media walk).
nested_scene::nested_scene(double aspect, bool media) {
    auto red = diffuse(0.65f, 0.05f, 0.05f);
    auto white = diffuse(0.73f, 0.73f, 0.73f);
    auto green = diffuse(0.12f, 0.45f, 0.15f);
    auto light = std::make_shared<diffuse_light>(solid(15.0, 15.0, 15.0));
    auto glass = std::make_shared<dielectric>(1.5);
    using list = std::vector<std::shared_ptr<hittable>>;
    auto L_ = [](list v) { return std::make_shared<hittable_list>(v); };

    auto lamp = std::make_shared<xz_rect>(213.0, 343.0, 227.0, 332.0, 554.0, light);
    Add(lamp);
    lights->objects.push_back(lamp);
    const double W = 555.0;
    Add(std::make_shared<flip_normals>(std::make_shared<yz_rect>(0.0, W, 0.0, W, W, green)));
    Add(std::make_shared<yz_rect>(0.0, W, 0.0, W, 0.0, red));
    Add(std::make_shared<flip_normals>(std::make_shared<xz_rect>(0.0, W, 0.0, W, W, white)));
    Add(std::make_shared<xz_rect>(0.0, W, 0.0, W, 0.0, white));
    Add(std::make_shared<flip_normals>(std::make_shared<xy_rect>(0.0, W, 0.0, W, W, white)));
    // instanced boxes in a list
    Add(L_({std::make_shared<translate>(
                std::make_shared<rotate_y>(std::make_shared<box>(vec3(0, 0, 0), vec3(80, 80, 80), white), 30.0),
                vec3(60, 0, 350)),
            std::make_shared<translate>(std::make_shared<box>(vec3(0, 0, 0), vec3(60, 120, 60), red),
                                        vec3(420, 0, 380)),
            std::make_shared<rotate_y>(
                std::make_shared<translate>(std::make_shared<box>(vec3(0, 0, 0), vec3(50, 50, 50), green),
                                            vec3(300, 0, 100)),
                -10.0)}));
    // a flip over a list holding a transformed rect
    Add(std::make_shared<flip_normals>(
        L_({std::make_shared<translate>(std::make_shared<xy_rect>(0.0, 100.0, 0.0, 100.0, 0.0, white),
                                        vec3(230, 300, 500))})));
    // a medium inside a nested list (a glass ball full of fog)
    auto ball = std::make_shared<sphere>(vec3(150, 60, 150), 60.0, glass);
    lights->objects.push_back(ball);
    if (media)
        Add(L_({ball,
                std::make_shared<constant_medium>(std::make_shared<sphere>(vec3(150, 60, 150), 55.0, glass), 0.02,
                                                  std::make_shared<isotropic>(solid(0.9, 0.9, 0.9))),
                std::make_shared<translate>(std::make_shared<box>(vec3(0, 0, 0), vec3(40, 40, 40), white),
                                            vec3(60, 0, 60))}));
    else
        Add(L_({ball, std::make_shared<translate>(std::make_shared<box>(vec3(0, 0, 0), vec3(40, 40, 40), white),
                                                  vec3(60, 0, 60))}));
    // a medium inside a translated list
    if (media)
    Add(std::make_shared<translate>(
        L_({std::make_shared<constant_medium>(
                std::make_shared<rotate_y>(std::make_shared<box>(vec3(0, 0, 0), vec3(100, 100, 100), white), 20.0),
                0.01, std::make_shared<isotropic>(solid(0.2, 0.4, 0.9))),
            std::make_shared<sphere>(vec3(50, 150, 50), 30.0,
                                     std::make_shared<metal>(vec3(0.8, 0.85, 0.88), 0.1))}),
        vec3(350, 0, 150)));
    // lists two deep under transforms
    Add(L_({L_({std::make_shared<translate>(std::make_shared<sphere>(vec3(0, 0, 0), 40.0, white),
                                            vec3(400, 300, 300))}),
            std::make_shared<rotate_y>(
                L_({std::make_shared<translate>(std::make_shared<box>(vec3(0, 0, 0), vec3(50, 50, 50), red),
                                                vec3(100, 350, 250))}),
                20.0)}));
    // a flip over a list of a bare rect and a translated one (the bare rect
    // becomes an entry whose only op is the flip)
    Add(std::make_shared<flip_normals>(
        L_({std::make_shared<xz_rect>(400.0, 500.0, 50.0, 150.0, 500.0, white),
            std::make_shared<translate>(std::make_shared<xz_rect>(0.0, 100.0, 0.0, 100.0, 0.0, green),
                                        vec3(50, 520, 400))})));
    cam = look(vec3(278.0, 278.0, -800.0), vec3(278.0, 278.0, 0.0), 40.0, aspect, 0.0, 10.0);
    background_type = BackgroundType::Black;
}

// The test images of the textured scene: every texel its own colour, no
// symmetry (37 and 53 are odd, so k -> 37 k + c and k -> 53 k + c are
// one-to-one modulo 256 and the red channels alone tell the texels apart).
std::shared_ptr<image_texture::byte_array> textured_scene::test_image(int which, int& nx, int& ny) {
    nx = which == 0 ? 7 : 4;
    ny = which == 0 ? 5 : 3;
    auto px = std::make_shared<image_texture::byte_array>((size_t)3 * nx * ny);
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const int k = i + nx * j;
            image_texture::byte* t = px->data() + 3 * k;
            if (which == 0) {
                t[0] = (image_texture::byte)((37 * k + 11) & 255);
                t[1] = (image_texture::byte)((91 * k + 5 * i + 40) & 255);
                t[2] = (image_texture::byte)((255 - 7 * k - 13 * j * j) & 255);
            } else {
                t[0] = (image_texture::byte)((53 * k + 200) & 255);
                t[1] = (image_texture::byte)((29 * k + 17 * j + 90) & 255);
                t[2] = (image_texture::byte)((19 * k * k + 3 * i + 60) & 255);
            }
        }
    return px;
}

// Image textures on every primitive kind under a gradient sky (no medium, no
// light list): a checker ground whose even child is the first image; that
// image on a sphere, a moving sphere, a hollow (negative-radius) sphere, a
// flipped ceiling rect and an emitting xy_rect whose normal points away from
// the camera (diffuse_light emits where dot(normal, ray) > 0); the second
// image, of another size, on a rotated, translated box (all three rect
// kinds) and one more ball.  Ten world objects, so use_bvh builds a world BVH.
textured_scene::textured_scene(double aspect, std::shared_ptr<image_texture::byte_array> first, int fnx, int fny) {
    int ax = fnx, ay = fny, bx = 0, by = 0;
    auto pa = first ? first : test_image(0, ax, ay);
    auto pb = test_image(1, bx, by);
    tex_ptr img_a = std::make_shared<image_texture>(pa, ax, ay);
    tex_ptr img_b = std::make_shared<image_texture>(pb, bx, by);
    tex_ptr grey = solid(0.3, 0.3, 0.35);
    tex_ptr tiles = std::make_shared<checker_texture>(img_a, grey);  // even = the image
    auto mat_a = std::make_shared<lambertian>(img_a);
    auto mat_b = std::make_shared<lambertian>(img_b);

    Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, std::make_shared<lambertian>(tiles)));
    Add(std::make_shared<sphere>(vec3(0, 1, 0), 1.0, mat_a));
    auto mover = std::make_shared<moving_sphere>(vec3(-2.5, 0.6, -1.0), 0.6, mat_a);
    movement_linear path;
    path.center1 = vec3(-2.5, 1.0, -1.0);
    path.time0 = 0.0;
    path.time1 = 1.0;
    mover->set_movement(path);
    Add(mover);
    Add(std::make_shared<sphere>(vec3(2.5, 0.9, -0.5), -0.9, mat_a));
    auto crate = std::make_shared<box>(vec3(0, 0, 0), vec3(1.0, 1.5, 1.0), mat_b);
    Add(std::make_shared<translate>(std::make_shared<rotate_y>(crate, 25.0), vec3(-1.2, 0.0, 2.5)));
    Add(std::make_shared<flip_normals>(std::make_shared<xz_rect>(-2.0, 2.0, -2.0, 2.0, 3.5, mat_a)));
    Add(std::make_shared<xy_rect>(-1.75, 1.75, 0.25, 2.75, 4.0, std::make_shared<diffuse_light>(img_a)));
    Add(std::make_shared<sphere>(vec3(1.6, 0.4, -2.0), 0.4, mat_b));
    Add(std::make_shared<sphere>(vec3(-0.9, 0.3, -2.6), 0.3, diffuse(0.7, 0.2, 0.2)));
    Add(std::make_shared<sphere>(vec3(3.4, 0.5, 2.2), 0.5, std::make_shared<metal>(vec3(0.8, 0.8, 0.7), 0.1)));

    cam = look(vec3(0.5, 2.0, -9.0), vec3(0.0, 1.2, 0.0), 35.0, aspect, 0.0, 10.0);
}

// A test scene for group BVHs outside the media kernels (not in the
// reference; composed the same way in oracle/ref_harness.cpp): under a
// gradient sky, with no medium and no light list, a ground sphere, a
// translated list of twelve spheres (lambertian, metal and glass in turn), a
// translated, rotated list of five boxes, a mirror ball between the two
// lists so that paths bounce from one group into the other, a glass ball and
// a moving sphere.  Six world objects: with use_bvh the two lists get group
// BVHs and the world stays a list.  `extra` adds six plain spheres in front
// ("grouped_world"): twelve world objects, so a world BVH above the two
// group BVHs.
grouped_scene::grouped_scene(double aspect, bool extra) {
    using list = std::vector<std::shared_ptr<hittable>>;
    Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, diffuse(0.5, 0.5, 0.5)));

    list balls;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 4; ++i) {
            const int k = i + 4 * j;
            mat_ptr m;
            if (k % 3 == 0)
                m = diffuse(0.15 + 0.07 * k, 0.8 - 0.05 * k, 0.3 + 0.04 * k);
            else if (k % 3 == 1)
                m = std::make_shared<metal>(vec3(0.9 - 0.03 * k, 0.7, 0.5 + 0.04 * k), 0.05 * (k % 4));
            else
                m = std::make_shared<dielectric>(1.5);
            balls.push_back(std::make_shared<sphere>(vec3(0.8 * i, 0.3 + 0.1 * (k % 2), 0.8 * j), 0.3, m));
        }
    Add(std::make_shared<translate>(std::make_shared<hittable_list>(balls), vec3(-4.0, 0.0, -0.8)));

    list crates;
    for (int k = 0; k < 5; ++k) {
        const double x0 = 0.9 * k, z0 = 0.3 * (k % 2);
        crates.push_back(std::make_shared<box>(vec3(x0, 0.0, z0), vec3(x0 + 0.6, 0.5 + 0.25 * k, z0 + 0.6),
                                               diffuse(0.75 - 0.1 * k, 0.3 + 0.1 * k, 0.25 + 0.05 * k)));
    }
    Add(std::make_shared<translate>(std::make_shared<rotate_y>(std::make_shared<hittable_list>(crates), 25.0),
                                    vec3(1.6, 0.0, -1.0)));

    Add(std::make_shared<sphere>(vec3(0, 1, 0), 1.0, std::make_shared<metal>(vec3(0.8, 0.8, 0.85), 0.0)));
    Add(std::make_shared<sphere>(vec3(0.2, 0.5, 2.2), 0.5, std::make_shared<dielectric>(1.5)));
    auto mover = std::make_shared<moving_sphere>(vec3(-1.5, 0.4, 2.4), 0.4, diffuse(0.7, 0.3, 0.1));
    movement_linear path;
    path.center1 = vec3(-1.5, 0.8, 2.4);
    path.time0 = 0.0;
    path.time1 = 1.0;
    mover->set_movement(path);
    Add(mover);

    if (extra)
        for (int k = 0; k < 6; ++k) {
            const vec3 c(-3.0 + 1.2 * k, 0.25, 3.6);
            if (k % 2 == 0)
                Add(std::make_shared<sphere>(c, 0.25, diffuse(0.2 + 0.1 * k, 0.4, 0.9 - 0.1 * k)));
            else
                Add(std::make_shared<sphere>(c, 0.25, std::make_shared<metal>(vec3(0.9, 0.6 + 0.05 * k, 0.4), 0.1)));
        }

    cam = look(vec3(3.0, 3.5, 10.0), vec3(0.0, 0.6, 0.0), 35.0, aspect, 0.0, 10.0);
}

// ------------------------------------------------------------------ ties
// Test scenes for the equal-distance rule of hittable_list::hit (a rect
// accepts t == t_max and so the last rect among equals wins; a sphere needs
// t < t_max, so the first sphere is kept; a rect beats a sphere either way).
// Not in the reference; composed the same way in oracle/ref_harness.cpp.
namespace {
mat_ptr mirror() { return std::make_shared<metal>(vec3(0.9, 0.9, 0.9), 0.0); }
std::shared_ptr<hittable> twin_mover(const vec3& c0, const vec3& c1, double r, mat_ptr m) {
    auto ms = std::make_shared<moving_sphere>(c0, r, m);
    movement_linear mv;
    mv.center1 = c1;
    mv.time0 = 0.0;
    mv.time1 = 1.0;
    ms->set_movement(mv);
    return ms;
}
}  // namespace

// "ties": twins -- two primitives of identical geometry, so that their t is
// bit-identical on every ray -- under a gradient sky, without media or
// lights.  Twins differ in material (a Lambertian colour against a mirror)
// and, where the class allows, in normal (radius -r, the same radius^2; or
// flip_normals), so the winner shows in the radiance, the traversal count
// and RenderType::Normal.  Twenty-two world objects (a world BVH under
// use_bvh); in list order, with the flat walk's runs:
//   a  static sphere twins, centre y != 0 } one run of spheres that move
//   c  twin y-only movers                 } along y or not at all
//   d  a sphere, then its twin under translate(., 0); a sphere under
//      translate(., 0), then its plain twin (x - 0 is exact: equal t bits in
//      two different entries, one with ops)
//   b  sphere twins with centre y == 0    } one plain run of spheres, movers
//   c' twin x-movers                      } and rects
//   e  coincident xy_rect twins and a third rect over a part of them
//   f  a yz_rect, then its twin under rotate_y(., 0) (sin 0, cos 1: exact);
//      an xz_rect under rotate_y(., 0), then its flipped twin
//   g  a translated list of five sphere twin pairs (a group BVH of prim
//      items; the order within a pair alternates)
//   h  a translated list of five box twin pairs (a group BVH of box items);
//      neighbouring boxes also share a part of a face
//      (the BVH builder splits by centroid, so twins stay in one leaf of two
//      items; g and h hold one glass triplet each, which it has to part)
ties_scene::ties_scene(double aspect) {
    using list = std::vector<std::shared_ptr<hittable>>;
    const vec3 zero(0.0, 0.0, 0.0);
    Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, diffuse(0.5, 0.5, 0.5)));
    // a
    Add(std::make_shared<sphere>(vec3(-4.0, 0.6, 0.0), 0.6, diffuse(0.8, 0.2, 0.2)));
    Add(std::make_shared<sphere>(vec3(-4.0, 0.6, 0.0), -0.6, mirror()));
    // c
    Add(twin_mover(vec3(-2.5, 0.5, 0.25), vec3(-2.5, 0.9, 0.25), 0.5, diffuse(0.2, 0.7, 0.3)));
    Add(twin_mover(vec3(-2.5, 0.5, 0.25), vec3(-2.5, 0.9, 0.25), -0.5, mirror()));
    // d
    Add(std::make_shared<sphere>(vec3(-1.0, 0.6, 0.0), 0.6, diffuse(0.2, 0.3, 0.8)));
    Add(std::make_shared<translate>(std::make_shared<sphere>(vec3(-1.0, 0.6, 0.0), -0.6, mirror()), zero));
    Add(std::make_shared<translate>(std::make_shared<sphere>(vec3(0.5, 0.6, 0.0), 0.6, diffuse(0.8, 0.7, 0.2)), zero));
    Add(std::make_shared<sphere>(vec3(0.5, 0.6, 0.0), -0.6, mirror()));
    // b
    Add(std::make_shared<sphere>(vec3(2.5, 0.0, 2.5), 0.7, diffuse(0.7, 0.3, 0.7)));
    Add(std::make_shared<sphere>(vec3(2.5, 0.0, 2.5), -0.7, mirror()));
    // c'
    Add(twin_mover(vec3(-3.6, 0.4, 2.5), vec3(-3.3, 0.4, 2.5), 0.4, diffuse(0.3, 0.7, 0.7)));
    Add(twin_mover(vec3(-3.6, 0.4, 2.5), vec3(-3.3, 0.4, 2.5), -0.4, mirror()));
    // e
    Add(std::make_shared<xy_rect>(1.5, 3.0, 0.0, 1.5, -0.5, diffuse(0.8, 0.5, 0.2)));
    Add(std::make_shared<flip_normals>(std::make_shared<xy_rect>(1.5, 3.0, 0.0, 1.5, -0.5, mirror())));
    Add(std::make_shared<xy_rect>(2.25, 3.5, 0.5, 2.0, -0.5, diffuse(0.2, 0.8, 0.5)));
    // f
    Add(std::make_shared<yz_rect>(0.0, 2.0, -1.0, 1.5, 4.0, diffuse(0.5, 0.2, 0.8)));
    Add(std::make_shared<rotate_y>(
        std::make_shared<flip_normals>(std::make_shared<yz_rect>(0.0, 2.0, -1.0, 1.5, 4.0, mirror())), 0.0));
    Add(std::make_shared<rotate_y>(std::make_shared<xz_rect>(-1.0, 1.0, 4.5, 6.5, 0.2, diffuse(0.8, 0.8, 0.3)), 0.0));
    Add(std::make_shared<flip_normals>(std::make_shared<xz_rect>(-1.0, 1.0, 4.5, 6.5, 0.2, mirror())));
    // g
    list balls;
    for (int k = 0; k < 5; ++k) {
        const vec3 c(-2.0 + k, 0.3, 0.0);
        auto plain = std::make_shared<sphere>(c, 0.3, diffuse(0.3 + 0.1 * k, 0.6, 0.9 - 0.15 * k));
        auto twin = std::make_shared<sphere>(c, -0.3, mirror());
        if (k & 1)
            balls.push_back(twin), balls.push_back(plain);
        else
            balls.push_back(plain), balls.push_back(twin);
        // a third coincident sphere: three items of one centre part 1 + 2 into leaves of two
        if (k == 2) balls.push_back(std::make_shared<sphere>(c, 0.3, std::make_shared<dielectric>(1.5)));
    }
    Add(std::make_shared<translate>(std::make_shared<hittable_list>(balls), vec3(0.0, 0.0, 2.0)));
    // h
    list crates;
    for (int k = 0; k < 5; ++k) {
        const vec3 p0(k, 0.0, 0.0), p1(k + 1.0, 0.3 + 0.05 * k, 0.6);
        auto plain = std::make_shared<box>(p0, p1, diffuse(0.9 - 0.15 * k, 0.4, 0.2 + 0.15 * k));
        auto twin = std::make_shared<flip_normals>(std::make_shared<box>(p0, p1, mirror()));
        // a third coincident box, first in the list (the last one wins)
        if (k == 2) crates.push_back(std::make_shared<box>(p0, p1, std::make_shared<dielectric>(1.5)));
        if (k & 1)
            crates.push_back(twin), crates.push_back(plain);
        else
            crates.push_back(plain), crates.push_back(twin);
    }
    Add(std::make_shared<translate>(std::make_shared<hittable_list>(crates), vec3(-2.5, 0.0, 3.2)));

    cam = camera(vec3(0.0, 2.5, 10.0), vec3(0.0, 0.6, 0.0), vec3(0.0, 1.0, 0.0), 38.0, aspect, 0.0, 10.0, 0.0, 1.0);
}

// "ties_axis": stations at x = 10 k, each a sphere((10 k, 0, -5), 1) and an
// xy_rect(10 k - 1, 10 k + 1, -1, 1, -4) that touches it at (10 k, 0, -4).
// A camera at (10 k, 0, 0) whose every ray is (0, 0, -1) (lower_left
// (10 k, 0, -1), horizontal = vertical = 0, no lens; the test's own
// rtw_camera_desc) meets both at exactly t = 4 in small integers.  List
// orders [sphere, rect], [rect, sphere], [rect, sphere, rect'] and, inside
// one translated list, [rect, sphere, rect'] again; the last rect wins.
// Station 4 is [rect, sphere] with a rect ten wide to one side, xy_rect(39,
// 49, -1, 1, -4): its centre lies beside the sphere's, not in front of it, so
// a BVH walk reaches the sphere first and the rect, earlier in the list,
// second (in stations 0 to 3 the rect's box is the nearer one).  The
// winner is flipped and emits (diffuse_light emits where dot(normal, ray) >
// 0): its pixel is its emission, exactly, in either precision, and its Normal
// colour (0.5, 0.5, 0).  The sphere's normal there and the other rect's are
// (0, 0, 1): Normal colour (0.5, 0.5, 1), and Lambertian.  Filler balls bring
// the world to sixteen objects (a world BVH).
ties_axis_scene::ties_axis_scene(double aspect) {
    using list = std::vector<std::shared_ptr<hittable>>;
    auto glow = [](double r, double g, double b) { return std::make_shared<diffuse_light>(solid(r, g, b)); };
    auto ball = [](double x, mat_ptr m) { return std::make_shared<sphere>(vec3(x, 0.0, -5.0), 1.0, m); };
    auto wall = [](double x, mat_ptr m) { return std::make_shared<xy_rect>(x - 1.0, x + 1.0, -1.0, 1.0, -4.0, m); };
    auto won = [&](double x, mat_ptr m) { return std::make_shared<flip_normals>(wall(x, m)); };
    // station 0: [sphere, rect]
    Add(ball(0.0, diffuse(0.8, 0.2, 0.2)));
    Add(won(0.0, glow(0.5, 1.0, 0.25)));
    // station 1: [rect, sphere]
    Add(won(10.0, glow(1.0, 0.25, 0.5)));
    Add(ball(10.0, diffuse(0.8, 0.8, 0.2)));
    // station 2: [rect, sphere, rect']
    Add(wall(20.0, diffuse(0.8, 0.2, 0.8)));
    Add(ball(20.0, diffuse(0.2, 0.8, 0.8)));
    Add(won(20.0, glow(0.25, 0.5, 1.0)));
    // station 3: the same three inside one translated list
    Add(std::make_shared<translate>(
        std::make_shared<hittable_list>(list{wall(0.0, diffuse(0.1, 0.5, 0.9)), ball(0.0, diffuse(0.5, 0.9, 0.1)),
                                             won(0.0, glow(2.0, 0.5, 0.125))}),
        vec3(30.0, 0.0, 0.0)));
    // station 4: [rect, sphere], the rect wide and to one side
    Add(std::make_shared<flip_normals>(std::make_shared<xy_rect>(39.0, 49.0, -1.0, 1.0, -4.0, glow(0.125, 2.0, 1.0))));
    Add(ball(40.0, diffuse(0.6, 0.6, 0.1)));
    for (int k = 0; k < 6; ++k)
        Add(std::make_shared<sphere>(vec3(5.0 + 10.0 * (k % 3), k < 3 ? 3.0 : -3.0, -6.0), 0.5,
                                     diffuse(0.3 + 0.1 * k, 0.5, 0.7 - 0.1 * k)));
    cam = look(vec3(15.0, 0.0, 30.0), vec3(15.0, 0.0, -5.0), 40.0, aspect, 0.0, 10.0);
}

// ---------------------------------------------------------------- probes
// Test scenes for the converged fp32-vs-fp64 comparison: one shading feature
// each, filling the frame, with bounded radiance (a gradient sky, or lights
// reached through the light list) so that per-pixel means converge quickly.
// Not in the reference; built from its classes.  Every kind carries enough
// objects (or one list of more than eight) that use_bvh builds a BVH.
namespace {
// n small Lambertian balls on a ring around `at`, as one translated list
// (more than eight primitives: a group BVH under use_bvh)
std::shared_ptr<hittable> pebbles(int n, double ring, double r, const vec3& at) {
    std::vector<std::shared_ptr<hittable>> v;
    for (int k = 0; k < n; ++k) {
        const double a = 2.0 * 3.14159265358979323846 * (k + 0.25) / n;
        v.push_back(std::make_shared<sphere>(vec3(ring * std::cos(a), 0.0, ring * std::sin(a)), r,
                                             diffuse(0.3 + 0.05 * (k % 5), 0.6 - 0.04 * (k % 7), 0.35 + 0.03 * (k % 3))));
    }
    return std::make_shared<translate>(std::make_shared<hittable_list>(v), at);
}
// single balls, one world object each (with the rest, enough for a world BVH)
void scatter_balls(scene& sc, int n, double ring, double r, double y) {
    for (int k = 0; k < n; ++k) {
        const double a = 2.0 * 3.14159265358979323846 * (k + 0.5) / n;
        sc.Add(std::make_shared<sphere>(vec3(ring * std::cos(a), y, ring * std::sin(a)), r,
                                        diffuse(0.65 - 0.06 * (k % 4), 0.3 + 0.07 * (k % 5), 0.25 + 0.1 * (k % 3))));
    }
}
std::shared_ptr<hittable> mover(vec3 c0, vec3 c1, double r, mat_ptr m, double t0, double t1) {
    auto ms = std::make_shared<moving_sphere>(c0, r, m);
    movement_linear mv;
    mv.center1 = c1;
    mv.time0 = t0;
    mv.time1 = t1;
    ms->set_movement(mv);
    return ms;
}
const char* const kProbeKinds[] = {"rect_light", "sphere_light", "far_sphere_light", "default_light", "glass",
                                   "metal",      "medium",       "motion",           "textures"};
}  // namespace

bool probe_scene::has_kind(const std::string& kind) {
    for (const char* k : kProbeKinds)
        if (kind == k) return true;
    return false;
}

probe_scene::probe_scene(double aspect, const std::string& kind) {
    auto white = diffuse(0.73, 0.73, 0.73);
    auto glass = std::make_shared<dielectric>(1.5);
    const vec3 up(0.0, 1.0, 0.0);

    if (kind == "rect_light" || kind == "default_light") {
        // diffuse_light emits where dot(normal, ray) > 0: a flip_normals'd
        // xz_rect shines upwards.  So the lit surface is a flipped Lambertian
        // rect above the lamp, seen from below, the lamp behind the camera:
        // 4:1 sides (a wrong extent shows; the Cornell lamp is nearly
        // square), a small rotated, translated box and a ring of balls under
        // the lit surface for shadows and the rects' frames.
        auto lamp = std::make_shared<xz_rect>(-2.0, 2.0, -0.5, 0.5, 0.0,
                                              std::make_shared<diffuse_light>(solid(8.0, 8.0, 8.0)));
        Add(std::make_shared<flip_normals>(lamp));
        lights->objects.push_back(lamp);
        Add(std::make_shared<flip_normals>(std::make_shared<xz_rect>(-10.0, 10.0, -10.0, 10.0, 4.0, white)));
        auto crate = std::make_shared<box>(vec3(0, 0, 0), vec3(0.8, 0.8, 0.8), diffuse(0.6, 0.5, 0.3));
        Add(std::make_shared<translate>(std::make_shared<rotate_y>(crate, 25.0), vec3(0.8, 3.2, -0.9)));
        Add(pebbles(10, 2.4, 0.25, vec3(0.0, 3.75, -0.5)));
        cam = camera(vec3(0.0, 0.6, 3.5), vec3(0.0, 4.0, 0.0), up, 50.0, aspect, 0.0, 5.0, 0.0, 1.0);
        background_type = BackgroundType::Black;
        // the second member has no pdf of its own: hittable's default,
        // direction (1,0,0) with pdf 0 (RTW_LIGHT_DEFAULT).  A quarter of the
        // bounces draw it and end the path, and under a black background the
        // lit surface's samples then spread too widely to converge in 2^16
        // per pixel: this kind has the gradient sky below the surface.
        if (kind == "default_light") {
            lights->objects.push_back(std::make_shared<box>(vec3(5, 0, 5), vec3(6, 1, 6), white));
            background_type = BackgroundType::Gradient;
        }
    } else if (kind == "sphere_light" || kind == "far_sphere_light") {
        // a sphere emits towards the side its normal points away from, so an
        // emitter seen from outside has a negative radius (sphere.h:71-77).
        // Near: the cone of directions to it has a half-angle from about 80
        // degrees under it to about 10 at the frame's edge; it is in view
        // (constant emission: no tail).  Far: radius / distance = 1/1000, out
        // of view, emission scaled so that the floor's level is about 1.
        const bool far_light = kind == "far_sphere_light";
        Add(std::make_shared<xz_rect>(-10.0, 10.0, -10.0, 10.0, 0.0, white));
        const double e = far_light ? 1.7e6 : 1.5;
        auto lamp = std::make_shared<sphere>(far_light ? vec3(400.0, 800.0, 450.0) : vec3(0.0, 1.02, 0.0), -1.0,
                                             std::make_shared<diffuse_light>(solid(e, e, e)));
        Add(lamp);
        lights->objects.push_back(lamp);
        auto crate = std::make_shared<box>(vec3(0, 0, 0), vec3(0.8, 0.8, 0.8), diffuse(0.6, 0.5, 0.3));
        Add(std::make_shared<translate>(std::make_shared<rotate_y>(crate, 25.0), vec3(2.0, 0.0, 0.6)));
        Add(pebbles(10, 3.4, 0.25, vec3(0.0, 0.25, 0.0)));
        cam = camera(vec3(0.0, 3.0, 9.0), vec3(0.0, 0.5, 0.0), up, 40.0, aspect, 0.0, 9.0, 0.0, 1.0);
        background_type = BackgroundType::Black;
    } else if (kind == "glass") {
        // a glass ball with a hollow shell (radius -0.9 inside radius 1), a
        // small solid glass ball, a Lambertian ground, gradient sky
        Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, diffuse(0.5, 0.5, 0.5)));
        Add(std::make_shared<sphere>(vec3(-0.5, 1.0, 0.0), 1.0, glass));
        Add(std::make_shared<sphere>(vec3(-0.5, 1.0, 0.0), -0.9, glass));
        Add(std::make_shared<sphere>(vec3(1.4, 0.6, 0.8), 0.6, glass));
        scatter_balls(*this, 7, 2.6, 0.3, 0.3);
        cam = camera(vec3(0.0, 1.8, 5.5), vec3(0.2, 0.8, 0.0), up, 32.0, aspect, 0.0, 5.5, 0.0, 1.0);
    } else if (kind == "metal") {
        // metal spheres with fuzz 0, 0.3 and 1.0 in front of a metal rect,
        // gradient sky
        Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, diffuse(0.5, 0.5, 0.5)));
        Add(std::make_shared<sphere>(vec3(-1.7, 0.8, 0.0), 0.8, std::make_shared<metal>(vec3(0.9, 0.9, 0.9), 0.0)));
        Add(std::make_shared<sphere>(vec3(0.0, 0.8, 0.0), 0.8, std::make_shared<metal>(vec3(0.8, 0.6, 0.2), 0.3)));
        Add(std::make_shared<sphere>(vec3(1.7, 0.8, 0.0), 0.8, std::make_shared<metal>(vec3(0.7, 0.8, 0.9), 1.0)));
        Add(std::make_shared<xy_rect>(-3.0, 3.0, 0.0, 2.4, -1.4, std::make_shared<metal>(vec3(0.85, 0.85, 0.8), 0.05)));
        scatter_balls(*this, 6, 2.8, 0.3, 0.3);
        cam = camera(vec3(0.0, 1.6, 6.0), vec3(0.0, 0.9, 0.0), up, 35.0, aspect, 0.0, 6.0, 0.0, 1.0);
    } else if (kind == "medium") {
        // a medium over a rotated, translated box (density 0.5) and a denser
        // one (2) over a sphere inside a glass shell, coloured isotropic
        // albedo, gradient sky
        Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0, diffuse(0.5, 0.5, 0.5)));
        auto smoke_box = std::make_shared<box>(vec3(0, 0, 0), vec3(2.0, 2.0, 2.0), white);
        Add(std::make_shared<constant_medium>(
            std::make_shared<translate>(std::make_shared<rotate_y>(smoke_box, 20.0), vec3(-2.9, 0.0, -0.6)), 0.5,
            std::make_shared<isotropic>(solid(0.8, 0.3, 0.2))));
        Add(std::make_shared<sphere>(vec3(1.4, 1.1, 0.0), 1.1, glass));
        Add(std::make_shared<constant_medium>(std::make_shared<sphere>(vec3(1.4, 1.1, 0.0), 1.0, glass), 2.0,
                                              std::make_shared<isotropic>(solid(0.2, 0.4, 0.9))));
        Add(pebbles(10, 3.3, 0.25, vec3(0.0, 0.25, 0.6)));
        cam = camera(vec3(0.0, 2.0, 7.0), vec3(0.0, 1.0, 0.0), up, 34.0, aspect, 0.0, 7.0, 0.0, 1.0);
    } else if (kind == "motion") {
        // every motion class the upload derives (tests/cpp/gpu_user_scene.cpp
        // motion_scene): a run of y-only movers and static spheres of odd
        // length, a lamp between the runs, a static sphere at y == 0, an
        // x-mover, a y-mover at x == 0, movers on [0.2, 0.7], a translated
        // mover, and a moving sphere among the lights only
        auto red = diffuse(0.65, 0.05, 0.05);
        auto light = std::make_shared<diffuse_light>(solid(6.0, 6.0, 6.0));
        Add(std::make_shared<sphere>(vec3(0.5, -1000, 0.25), 1000, white));
        for (int k = 0; k < 6; ++k)
            Add(mover(vec3(-2.5 + k, 0.3, 1.5), vec3(-2.5 + k, 0.3 + 0.1 * k, 1.5), 0.3, k & 1 ? red : white, 0.0, 1.0));
        Add(std::make_shared<sphere>(vec3(1.7, 0.4, -0.6), 0.4, glass));
        Add(std::make_shared<sphere>(vec3(-1.2, 0.2, 0.6), 0.2, red));
        auto lamp = std::make_shared<xz_rect>(-1.0, 1.0, -1.0, 1.0, 4.0, light);
        Add(std::make_shared<translate>(std::make_shared<flip_normals>(lamp), vec3(0.0, 0.0, 0.0)));
        lights->objects.push_back(lamp);
        Add(std::make_shared<sphere>(vec3(-1.8, 0.0, -1.2), 0.35, red));
        Add(mover(vec3(-0.8, 0.35, -1.4), vec3(-0.5, 0.35, -1.4), 0.35, white, 0.0, 1.0));
        Add(mover(vec3(0.0, 0.3, -2.0), vec3(0.0, 0.7, -2.0), 0.3, red, 0.0, 1.0));
        Add(mover(vec3(0.9, 0.3, -2.2), vec3(0.9, 0.9, -2.2), 0.3, white, 0.2, 0.7));
        Add(mover(vec3(2.0, 0.5, -1.0), vec3(2.3, 0.5, -1.3), 0.3, glass, 0.2, 0.7));
        Add(std::make_shared<translate>(mover(vec3(0, 0.25, 0), vec3(0, 0.55, 0), 0.25, red, 0.0, 1.0),
                                        vec3(-0.6, 0.0, 2.4)));
        lights->objects.push_back(mover(vec3(2.5, 3.0, 2.0), vec3(2.5, 3.2, 2.0), 0.5, light, 0.0, 1.0));
        cam = camera(vec3(0.0, 2.0, 7.0), vec3(0.0, 0.5, 0.0), up, 40.0, aspect, 0.0, 7.0, 0.0, 1.0);
    } else if (kind == "textures") {
        // a checker ground sphere seen from high enough that coordinates in
        // view reach a few hundred (the checker's sines take thousands of
        // radians), a marble sphere, a thin lens of aperture 0.3; no image
        // texture (the oracle has none)
        tex_ptr dark = solid(0.2, 0.3, 0.1), bright = solid(0.9, 0.9, 0.9);
        tex_ptr marble = std::make_shared<noise_texture>(4.0);
        Add(std::make_shared<sphere>(vec3(0, -1000, 0), 1000.0,
                                     std::make_shared<lambertian>(std::make_shared<checker_texture>(dark, bright))));
        Add(std::make_shared<sphere>(vec3(0.0, 6.0, 0.0), 6.0, std::make_shared<lambertian>(marble)));
        for (int k = 0; k < 8; ++k) {
            const double a = 2.0 * 3.14159265358979323846 * (k + 0.5) / 8;
            mat_ptr m = diffuse(0.7, 0.3 + 0.05 * k, 0.2);
            if (k & 1) m = std::make_shared<lambertian>(marble);
            Add(std::make_shared<sphere>(vec3(11.0 * std::cos(a), 1.5, 11.0 * std::sin(a)), 1.5, m));
        }
        const vec3 from(0.0, 22.0, 60.0), at(0.0, 5.0, 0.0);
        cam = camera(from, at, up, 30.0, aspect, 0.3, (from - at).length(), 0.0, 1.0);
    }
}

std::unique_ptr<scene> make_builtin_scene(const std::string& name, double aspect) {
    if (name.rfind("probe_", 0) == 0 && probe_scene::has_kind(name.substr(6)))
        return std::make_unique<probe_scene>(aspect, name.substr(6));
    if (name == "grouped") return std::make_unique<grouped_scene>(aspect);
    if (name == "grouped_world") return std::make_unique<grouped_scene>(aspect, true);
    if (name == "ties") return std::make_unique<ties_scene>(aspect);
    if (name == "ties_axis") return std::make_unique<ties_axis_scene>(aspect);
    if (name == "nested") return std::make_unique<nested_scene>(aspect);
    if (name == "nested_plain") return std::make_unique<nested_scene>(aspect, false);
    if (name == "cornell_box") return std::make_unique<cornell_box_scene>(aspect);
    if (name == "random_balls") return std::make_unique<random_balls_scene>(aspect);
    if (name == "dielectric") return std::make_unique<dielectric_scene>(aspect);
    if (name == "light_sample") return std::make_unique<light_sample>(aspect);
    if (name == "book2_final") return std::make_unique<book2_final_scene>(aspect);
    if (name == "textured") return std::make_unique<textured_scene>(aspect);
    return nullptr;
}
