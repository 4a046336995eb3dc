// image_scene_check.cpp — the PPM loader and the flattener's handling of
// image textures, through the host C++ API and librtw.so (CPU only).
//
//   image_scene_check load <file.ppm>
//       "ok <nx> <ny> <3*nx*ny bytes as decimals>"  or  "err <status> <message>"
//   image_scene_check shared
//       two image_textures over one byte_array and a third over its own:
//       "bytes <image_bytes>" then one line "tex <nx> <ny> <offset>" per
//       RTW_TEX_IMAGE entry of the flattened scene
//   image_scene_check iso | iso_checker
//       a constant_medium whose isotropic phase material holds an image
//       (directly / as a checker's child): "rc <status> <message>"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "rtw/flatten.h"
#include "rtw/scene.h"
#include "rtw_gpu.h"

namespace {
std::shared_ptr<image_texture::byte_array> ramp(size_t n, int start) {
    auto p = std::make_shared<image_texture::byte_array>(n);
    for (size_t k = 0; k < n; ++k) (*p)[k] = (image_texture::byte)((start + 7 * k) & 255);
    return p;
}

class user_scene : public scene {
public:
    user_scene() {
        cam = camera(vec3(0, 1, -5), vec3(0, 0, 0), vec3(0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0);
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "load" && argc == 3) {
        image_texture::byte_array px;
        int nx = -1, ny = -1;
        const int rc = rtw_load_ppm(argv[2], px, nx, ny);
        if (rc != RTW_OK) {
            std::printf("err %d %s\n", rc, rtw_last_error());
            return 0;
        }
        std::printf("ok %d %d", nx, ny);
        for (auto b : px) std::printf(" %d", (int)b);
        std::printf("\n");
        return 0;
    }
    if (mode == "shared") {
        auto one = ramp(3 * 4 * 2, 10), two = ramp(3 * 3 * 3, 99);
        user_scene sc;
        auto mat = [](std::shared_ptr<texture> t) { return std::make_shared<lambertian>(t); };
        sc.Add(std::make_shared<sphere>(vec3(0, 0, 0), 1.0, mat(std::make_shared<image_texture>(one, 4, 2))));
        sc.Add(std::make_shared<sphere>(vec3(3, 0, 0), 1.0, mat(std::make_shared<image_texture>(two, 3, 3))));
        // the first array again, read as 2 x 4
        sc.Add(std::make_shared<sphere>(vec3(-3, 0, 0), 1.0, mat(std::make_shared<image_texture>(one, 2, 4))));
        rtw_scene_desc* d = nullptr;
        if (rtw_flatten(sc, 0, &d) != RTW_OK) {
            std::printf("err %s\n", rtw_last_error());
            return 1;
        }
        std::printf("bytes %llu\n", (unsigned long long)d->image_bytes);
        for (int k = 0; k < d->n_textures; ++k)
            if (d->textures[k].type == RTW_TEX_IMAGE)
                std::printf("tex %d %d %d\n", d->textures[k].odd, d->textures[k].even, d->textures[k].offset);
        bool same = d->image_bytes == one->size() + two->size() &&
                    std::memcmp(d->image_texels, one->data(), one->size()) == 0 &&
                    std::memcmp(d->image_texels + one->size(), two->data(), two->size()) == 0;
        std::printf("texels %s\n", same ? "match" : "differ");
        rtw_scene_desc_free(d);
        return 0;
    }
    if (mode == "iso" || mode == "iso_checker") {
        std::shared_ptr<texture> img = std::make_shared<image_texture>(ramp(3 * 2 * 2, 5), 2, 2);
        std::shared_ptr<texture> grey = std::make_shared<constant_texture>(vec3(0.5, 0.5, 0.5));
        std::shared_ptr<texture> inner = std::make_shared<checker_texture>(grey, img);
        std::shared_ptr<texture> phase = mode == "iso" ? img : std::make_shared<checker_texture>(inner, grey);
        user_scene sc;
        auto shell = std::make_shared<sphere>(vec3(0, 0, 0), 1.0, std::make_shared<dielectric>(1.5));
        sc.Add(std::make_shared<constant_medium>(shell, 0.2, std::make_shared<isotropic>(phase)));
        rtw_scene_desc* d = nullptr;
        const int rc = rtw_flatten(sc, 0, &d);
        std::printf("rc %d %s\n", rc, rc == RTW_OK ? "" : rtw_last_error());
        if (d) rtw_scene_desc_free(d);
        return 0;
    }
    return 2;
}
