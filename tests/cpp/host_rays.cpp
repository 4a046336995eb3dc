// host_rays.cpp — rtw_query.h's closest-hit query written against this
// repository's host header API only (raytracingweekend_amd/csrc/host/rtw/), as
// host_features.cpp writes the feature sums: for every ray of the file it sets
// rtw::current_stream() to the ray's minstd state, calls the world's
// hittable::hit(ray(o, d, time), 0.001f, t_max, rec) once and reads the state
// back.
//
//   host_rays <scene> <rays.bin> <rng.bin|-> <out.bin>
//     rays.bin: raw rtw_query_ray records (8 doubles: o, d, time, t_max)
//     rng.bin:  one uint32 state per ray ("-": every ray starts at state 1;
//               only a scene with media draws)
//     out.bin:  per ray 8 doubles (hit flag 0 / 1, t, p, normal; zeros after the
//               flag on a miss), then per ray the uint32 state after the call
// The scene is make_builtin_scene(scene, aspect 1): the world does not depend
// on the aspect, only the camera does.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "scene.h"

namespace {
template <class T>
bool slurp(const char* path, std::vector<T>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(T)) {
        std::fclose(f);
        return false;
    }
    out.resize((size_t)bytes / sizeof(T));
    const bool ok = out.empty() || std::fread(out.data(), sizeof(T), out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: host_rays <scene> <rays.bin> <rng.bin|-> <out.bin>\n");
        return 2;
    }
    std::unique_ptr<scene> sc = make_builtin_scene(argv[1], 1.0);
    if (!sc) {
        std::fprintf(stderr, "unknown scene %s\n", argv[1]);
        return 2;
    }
    std::vector<double> rays;
    if (!slurp(argv[2], rays) || rays.size() % 8) {
        std::fprintf(stderr, "%s: not a file of 64-byte ray records\n", argv[2]);
        return 1;
    }
    const size_t n = rays.size() / 8;
    std::vector<uint32_t> rng(n, 1u);
    if (std::string(argv[3]) != "-" && (!slurp(argv[3], rng) || rng.size() != n)) {
        std::fprintf(stderr, "%s: expected one uint32 state per ray\n", argv[3]);
        return 1;
    }
    const hittable& world = sc->GetWorld();
    std::vector<double> out(n * 8, 0.0);
    for (size_t k = 0; k < n; ++k) {
        const double* q = &rays[8 * k];
        const rtw::stream_state saved = rtw::current_stream();
        rtw::current_stream() = rtw::stream_state{rng[k], 0};
        const ray r(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6]);
        hit_record rec;
        const bool hit = world.hit(r, 0.001f, q[7], rec);
        rng[k] = (uint32_t)rtw::current_stream().x;
        rtw::current_stream() = saved;
        if (!hit) continue;
        double* o = &out[8 * k];
        o[0] = 1.0, o[1] = rec.t;
        o[2] = rec.p.x, o[3] = rec.p.y, o[4] = rec.p.z;
        o[5] = rec.normal.x, o[6] = rec.normal.y, o[7] = rec.normal.z;
    }
    FILE* f = std::fopen(argv[4], "wb");
    if (!f) return 1;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fwrite(rng.data(), sizeof(uint32_t), rng.size(), f);
    std::fclose(f);
    return 0;
}
