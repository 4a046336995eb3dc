// rtw_render — the host program of the reference (RayTracingWeekend.cpp:195-289)
// on the MI355X path: build a scene with the hittable API, flatten it, run the
// per-pixel render loop on the GPU through the C ABI, gamma + clamp, write the
// P3 PPM, report Trace/Write milliseconds.
//
//   rtw_render [--scene cornell_box] [--nx 400] [--ny 400] [--spp 64]
//              [--depth 100] [--seed 0] [--bvh] [--device 0] [--gpus 1]
//              [--precision fp64|fp32] [--out out.ppm] [--image FILE.ppm]
//              [--noise] [--noise-target X [--noise-batch 8] [--noise-floor 0.01]]
//              [--adaptive X [--min-spp 16] [--noise-batch B] [--noise-floor 0.01]
//                            [--adaptive-window R]]
//              [--denoise [--denoise-iterations 5]]
//   rtw_render --scene S [--bvh] --rays rays.bin --hits hits.bin [--occluded] [--rng rng.bin]
//   rtw_render --scene S [--bvh] --rays rays.bin --radiance sums.bin --spp N [--depth D] [--seed S] [--rng rng.bin]
//
// --rays rays.bin --radiance sums.bin path-traces the caller's rays
// (rtw_radiance.h): samples [0, --spp) of every ray, ray k keyed k, --depth as
// color()'s depth; sums.bin receives raw doubles, 3 per ray, each ray's sum of
// its samples.  With --rng rng.bin (one uint32 state per ray, --spp 1) ray k's
// sample starts from that state; the file is not rewritten.  Not with --hits,
// --occluded or --out.  Prints one "Radiance:" line.  One GPU.
//
// --rays rays.bin --hits hits.bin traces the caller's rays instead of rendering
// (rtw_query.h): rays.bin holds raw rtw_query_ray records, hits.bin receives
// raw rtw_query_hit records (rtw_trace_closest) or, with --occluded, one byte
// per ray (rtw_trace_occluded).  A scene with media needs --rng rng.bin, one
// uint32 minstd state per ray; the states after the trace are written back to
// that file.  Prints one "Query:" line: kernel, rays, milliseconds.  One GPU.
//
// --noise renders through rtw_render_accumulate_moments (rtw_noise.h) and
// prints the image-wide noise estimate of the --spp samples.  --noise-target X
// renders the sample ranges [0,b) [b,2b) [2b,4b) ... (b = --noise-batch) until
// the estimate's mean relative standard error is at most X or --spp samples
// are done, and finalizes the canvas with the samples it used.  One GPU only.
//
// --adaptive X renders through rtw_render_adaptive (rtw_adaptive.h): --min-spp
// samples of every pixel, then rounds of --noise-batch samples (not given: as
// many as are done so far) of the pixels whose relative standard error is
// still above X, with --spp as the most a pixel takes; the canvas divides
// every pixel's sum by its own sample count.  One GPU only.
// --adaptive-window R (0..16, default 0) keeps a pixel sampling while any pixel
// within R pixels of it is still above X (rtw_render_adaptive_window,
// rtw_adaptive_window.h).
//
// --denoise filters the image before the canvas step (rtw_denoise.h): the
// render keeps second moments, rtw_render_features adds the first-hit features
// of the samples every pixel took, and rtw_denoise (the host function: the
// device filter's bits) gives the mean the canvas is made of.  With plain,
// --noise-target and --adaptive renders; one GPU only.
//
// --image FILE.ppm (with --scene textured): a P6 or P3 PPM, maxval 255, that
// replaces the scene's first image texture (rtw_load_ppm).
//
// --precision fp64 (default) is the parity mode (the reference's double
// arithmetic on every path decision); fp32 the fast mode (single precision,
// statistical parity only; rtw_render_params.precision).
//
// --gpus N renders on devices device .. device+N-1 from this one process
// (rtw_render_multi: one host thread per GPU, RCCL reduce to the first).
//
// Defaults are the reference's compile-time constants (RayTracingWeekend.cpp:32-43,
// scene typedef :201).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rtw/scene.h"
#include "rtw_gpu.h"
#include "rtw_adaptive.h"
#include "rtw_adaptive_window.h"
#include "rtw_denoise.h"
#include "rtw_noise.h"
#include "rtw_query.h"
#include "rtw_radiance.h"

namespace {
bool slurp(const std::string& path, std::vector<char>& out) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = out.empty() || std::fread(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}
bool spill(const std::string& path, const void* data, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}
// the rays of --rays and the states of --rng (empty path: none)
bool load_rays(const std::string& rays_path, const std::string& rng_path, std::vector<rtw_query_ray>& rays,
               std::vector<uint32_t>& rng) {
    std::vector<char> raw, raw_rng;
    if (!slurp(rays_path, raw) || raw.size() % sizeof(rtw_query_ray)) {
        std::fprintf(stderr, "--rays %s: not a file of %zu-byte ray records\n", rays_path.c_str(), sizeof(rtw_query_ray));
        return false;
    }
    const uint64_t n = raw.size() / sizeof(rtw_query_ray);
    rays.resize(n);
    if (n) std::memcpy(rays.data(), raw.data(), raw.size());
    if (!rng_path.empty()) {
        if (!slurp(rng_path, raw_rng) || raw_rng.size() != n * 4) {
            std::fprintf(stderr, "--rng %s: expected one uint32 state per ray\n", rng_path.c_str());
            return false;
        }
        rng.resize(n);
        if (n) std::memcpy(rng.data(), raw_rng.data(), raw_rng.size());
    }
    return true;
}

// --rays --radiance: path-trace the file's rays on `handle`, write the per-ray sums
int run_radiance(void* handle, const std::string& rays_path, const std::string& sums_path, const std::string& rng_path,
                 int spp, int depth, unsigned long long seed) {
    std::vector<rtw_query_ray> rays;
    std::vector<uint32_t> rng;
    if (!load_rays(rays_path, rng_path, rays, rng)) return 1;
    const uint64_t n = rays.size();
    rtw_radiance_params rp;
    std::memset(&rp, 0, sizeof rp);
    rp.max_depth = depth, rp.spp_count = spp, rp.seed = seed, rp.precision = RTW_PRECISION_FP64;
    rtw_stats st;
    std::memset(&st, 0, sizeof st);
    char kernel[128] = "";
    std::vector<double> sums(n * 3, 0.0);
    if (rtw_scene_query_radiance(handle, kernel) != RTW_OK ||
        rtw_trace_radiance(handle, rays.data(), n, rng_path.empty() ? nullptr : rng.data(), &rp, sums.data(), &st) != RTW_OK) {
        std::fprintf(stderr, "radiance: %s\n", rtw_last_error());
        return 1;
    }
    if (!spill(sums_path, sums.data(), sums.size() * sizeof(double))) {
        std::fprintf(stderr, "cannot write %s\n", sums_path.c_str());
        return 1;
    }
    std::printf("Radiance: %s  rays %llu  samples %llu  segments %llu  %.3f ms\n", kernel, (unsigned long long)n,
                (unsigned long long)st.samples, (unsigned long long)st.segments, st.ms_total);
    return 0;
}

// --rays: trace the file's rays on `handle`, write the hits (or flags)
int run_query(void* handle, const std::string& rays_path, const std::string& hits_path, const std::string& rng_path,
              bool occluded) {
    std::vector<rtw_query_ray> rays;
    std::vector<uint32_t> rng;
    if (!load_rays(rays_path, rng_path, rays, rng)) return 1;
    const uint64_t n = rays.size();
    rtw_query_params qp;
    std::memset(&qp, 0, sizeof qp);
    qp.precision = RTW_PRECISION_FP64;
    rtw_stats st;
    std::memset(&st, 0, sizeof st);
    char k_closest[128] = "", k_occluded[128] = "";
    if (rtw_scene_query_trace(handle, k_closest, k_occluded) != RTW_OK) {
        std::fprintf(stderr, "query: %s\n", rtw_last_error());
        return 1;
    }
    std::vector<rtw_query_hit> hits(occluded ? 0 : n);
    std::vector<uint8_t> flags(occluded ? n : 0);
    uint32_t* g = rng.empty() ? nullptr : rng.data();
    const int rc = occluded ? rtw_trace_occluded(handle, rays.data(), n, g, &qp, flags.data(), &st)
                            : rtw_trace_closest(handle, rays.data(), n, g, &qp, hits.data(), &st);
    if (rc != RTW_OK) {
        std::fprintf(stderr, "query: %s\n", rtw_last_error());
        return 1;
    }
    const bool wrote = occluded ? spill(hits_path, flags.data(), flags.size())
                                : spill(hits_path, hits.data(), hits.size() * sizeof(rtw_query_hit));
    if (!wrote || (g && !spill(rng_path, rng.data(), rng.size() * 4))) {
        std::fprintf(stderr, "cannot write %s\n", hits_path.c_str());
        return 1;
    }
    std::printf("Query: %s  rays %llu  %.3f ms\n", occluded ? k_occluded : k_closest, (unsigned long long)n, st.ms_total);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    std::string scene_name = "cornell_box", out = "1.ppm", image;
    int nx = 400, ny = 400, spp = 64, depth = 100, device = 0, bvh = 0, gpus = 1, precision = RTW_PRECISION_FP64;
    unsigned long long seed = 0;
    bool noise = false, to_target = false;
    double noise_target = 0.0, noise_floor = 1e-2;
    int noise_batch = 8, min_spp = 16;
    bool adaptive = false, batch_given = false;
    double adaptive_target = 0.0;
    int adaptive_window = 0;
    bool window_given = false;
    bool denoise = false;
    int denoise_iterations = -1;  // (not given: the library's default)
    std::string rays_path, hits_path, rng_path, radiance_path;
    bool occluded = false, out_given = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "missing value for %s\n", a.c_str());
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--scene") scene_name = next();
        else if (a == "--nx") nx = std::atoi(next());
        else if (a == "--ny") ny = std::atoi(next());
        else if (a == "--spp") spp = std::atoi(next());
        else if (a == "--depth") depth = std::atoi(next());
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--out") out = next(), out_given = true;
        else if (a == "--bvh") bvh = 1;
        else if (a == "--image") image = next();
        else if (a == "--noise") noise = true;
        else if (a == "--noise-target") noise_target = std::atof(next()), noise = to_target = true;
        else if (a == "--noise-batch") noise_batch = std::atoi(next()), batch_given = true;
        else if (a == "--adaptive") adaptive_target = std::atof(next()), adaptive = true;
        else if (a == "--adaptive-window") adaptive_window = std::atoi(next()), window_given = true;
        else if (a == "--min-spp") min_spp = std::atoi(next());
        else if (a == "--noise-floor") noise_floor = std::atof(next());
        else if (a == "--denoise") denoise = true;
        else if (a == "--rays") rays_path = next();
        else if (a == "--hits") hits_path = next();
        else if (a == "--radiance") radiance_path = next();
        else if (a == "--rng") rng_path = next();
        else if (a == "--occluded") occluded = true;
        else if (a == "--denoise-iterations") denoise_iterations = std::atoi(next()), denoise = true;
        else if (a == "--precision") {
            const std::string v = next();
            if (v == "fp64") precision = RTW_PRECISION_FP64;
            else if (v == "fp32") precision = RTW_PRECISION_FP32;
            else {
                std::fprintf(stderr, "--precision %s: expected fp64 or fp32\n", v.c_str());
                return 2;
            }
        }
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }

    if (noise && gpus != 1) {
        std::fprintf(stderr, "--noise / --noise-target render on one GPU (--gpus 1)\n");
        return 2;
    }
    if (noise && (spp < 2 || noise_batch < 2 || (to_target && !(noise_target > 0.0)) || !(noise_floor > 0.0))) {
        std::fprintf(stderr, "--noise needs --spp >= 2, --noise-batch >= 2, --noise-target > 0, --noise-floor > 0\n");
        return 2;
    }

    if (adaptive && (gpus != 1 || noise)) {
        std::fprintf(stderr, "--adaptive renders on one GPU (--gpus 1), without --noise / --noise-target\n");
        return 2;
    }
    if (adaptive && (!(adaptive_target >= 0.0) || min_spp < 2 || spp < min_spp || (batch_given && noise_batch < 1) ||
                     !(noise_floor > 0.0))) {
        std::fprintf(stderr, "--adaptive needs a target >= 0, --min-spp >= 2, --spp >= --min-spp, --noise-batch >= 1, "
                             "--noise-floor > 0\n");
        return 2;
    }

    if (window_given && (!adaptive || adaptive_window < 0 || adaptive_window > RTW_WINDOW_RADIUS_MAX)) {
        std::fprintf(stderr, "--adaptive-window needs --adaptive and a radius in [0, %d]\n", RTW_WINDOW_RADIUS_MAX);
        return 2;
    }

    if (denoise && (gpus != 1 || spp < 2 || (denoise_iterations != -1 && (denoise_iterations < 0 || denoise_iterations > 8)))) {
        std::fprintf(stderr, "--denoise renders on one GPU (--gpus 1) and needs --spp >= 2, --denoise-iterations in [0, 8]\n");
        return 2;
    }

    if (!radiance_path.empty()) {
        if (rays_path.empty() || !hits_path.empty() || occluded || out_given || gpus != 1 || noise || adaptive || denoise ||
            precision != RTW_PRECISION_FP64 || spp < 1 || depth < 0) {
            std::fprintf(stderr, "--rays FILE --radiance FILE --spp N [--depth D] [--rng FILE] go together, on one GPU, in "
                                 "fp64, without --hits, --occluded, --out or a render's options\n");
            return 2;
        }
    } else if (rays_path.empty() != hits_path.empty() || (rays_path.empty() && (occluded || !rng_path.empty())) ||
        (!rays_path.empty() && (gpus != 1 || noise || adaptive || denoise))) {
        std::fprintf(stderr, "--rays FILE --hits FILE [--occluded] [--rng FILE] go together, on one GPU, without a render's "
                             "options\n");
        return 2;
    }

    std::unique_ptr<scene> sc;
    if (!image.empty()) {
        if (scene_name != "textured") {
            std::fprintf(stderr, "--image needs --scene textured\n");
            return 2;
        }
        auto pixels = std::make_shared<image_texture::byte_array>();
        int inx = 0, iny = 0;
        if (rtw_load_ppm(image, *pixels, inx, iny) != RTW_OK) {
            std::fprintf(stderr, "image: %s\n", rtw_last_error());
            return 1;
        }
        sc = std::make_unique<textured_scene>(nx * 1.0 / ny, pixels, inx, iny);
    } else {
        sc = make_builtin_scene(scene_name, nx * 1.0 / ny);  // RayTracingWeekend.cpp:204
    }
    if (!sc) {
        std::fprintf(stderr, "unknown scene %s\n", scene_name.c_str());
        return 2;
    }
    rtw_scene_desc* desc = nullptr;
    if (rtw_flatten_scene(*sc, bvh, &desc) != RTW_OK) {
        std::fprintf(stderr, "flatten: %s\n", rtw_last_error());
        return 1;
    }
    if (gpus < 1 || device < 0 || device + gpus > rtw_device_count()) {
        std::fprintf(stderr, "--device %d --gpus %d: only %d devices visible\n", device, gpus, rtw_device_count());
        return 2;
    }
    std::vector<void*> h(gpus, nullptr);
    for (int g = 0; g < gpus; ++g)
        if (rtw_scene_upload(device + g, desc, &h[g]) != RTW_OK) {
            std::fprintf(stderr, "upload: %s\n", rtw_last_error());
            return 1;
        }
    if (!radiance_path.empty()) {
        const int rc = run_radiance(h[0], rays_path, radiance_path, rng_path, spp, depth, seed);
        rtw_scene_free(h[0]);
        rtw_scene_desc_free(desc);
        return rc;
    }
    if (!rays_path.empty()) {
        const int rc = run_query(h[0], rays_path, hits_path, rng_path, occluded);
        rtw_scene_free(h[0]);
        rtw_scene_desc_free(desc);
        return rc;
    }
    const rtw_camera_desc cam = sc->GetCamera().desc();
    rtw_render_params p;
    std::memset(&p, 0, sizeof p);
    p.nx = nx, p.ny = ny, p.spp = spp, p.max_depth = depth, p.seed = seed, p.row_step = 1;
    p.precision = precision;
    std::vector<double> accum((size_t)nx * ny * 3, 0.0), canvas(accum.size());
    rtw_stats st;
    std::memset(&st, 0, sizeof st);
    int spp_done = spp;
    rtw_noise_summary ns;
    std::memset(&ns, 0, sizeof ns);
    rtw_adaptive_result ar;
    std::memset(&ar, 0, sizeof ar);
    std::vector<uint32_t> counts;
    std::vector<double> accum_sq;
    if (adaptive || noise || denoise) accum_sq.assign(accum.size(), 0.0);
    auto t0 = std::chrono::high_resolution_clock::now();
    if (adaptive) {
        counts.assign((size_t)nx * ny, 0u);
        rtw_adaptive_params ap;
        std::memset(&ap, 0, sizeof ap);
        ap.target_rel = adaptive_target, ap.floor = noise_floor, ap.min_spp = min_spp, ap.max_spp = spp;
        ap.batch = batch_given ? noise_batch : 0;
        const int rc = adaptive_window
                           ? rtw_render_adaptive_window(h[0], &cam, &p, &ap, adaptive_window, accum.data(),
                                                        accum_sq.data(), counts.data(), &ar, &st)
                           : rtw_render_adaptive(h[0], &cam, &p, &ap, accum.data(), accum_sq.data(), counts.data(), &ar,
                                                 &st);
        if (rc != RTW_OK) {
            std::fprintf(stderr, "render: %s\n", rtw_last_error());
            return 1;
        }
    } else if (noise) {
        // one batch of all samples, or (--noise-target) batches that double the
        // total until the estimate reaches the target (render.render_to_noise)
        spp_done = 0;
        while (spp_done < spp) {
            const int want = to_target ? (spp_done == 0 ? noise_batch : spp_done) : spp;
            p.spp_begin = spp_done;
            p.spp_count = want < spp - spp_done ? want : spp - spp_done;
            rtw_stats sb;
            if (rtw_render_accumulate_moments(h[0], &cam, &p, accum.data(), accum_sq.data(), &sb) != RTW_OK) {
                std::fprintf(stderr, "render: %s\n", rtw_last_error());
                return 1;
            }
            st.samples += sb.samples, st.segments += sb.segments;
            spp_done += p.spp_count;
            if (rtw_noise_estimate(accum.data(), accum_sq.data(), nx, ny, spp_done, noise_floor, nullptr, &ns) !=
                RTW_OK) {
                std::fprintf(stderr, "noise: %s\n", rtw_last_error());
                return 1;
            }
            if (to_target && ns.mean_rel <= noise_target) break;
        }
    } else {
        // (--denoise: the same sums, and the second moments beside them)
        const int rc = denoise     ? rtw_render_accumulate_moments(h[0], &cam, &p, accum.data(), accum_sq.data(), &st)
                       : gpus == 1 ? rtw_render_accumulate(h[0], &cam, &p, accum.data(), &st)
                                   : rtw_render_multi(gpus, h.data(), &cam, &p, accum.data(), &st);
        if (rc != RTW_OK) {
            std::fprintf(stderr, "render: %s\n", rtw_last_error());
            return 1;
        }
    }
    rtw_denoise_params dp;
    rtw_denoise_default_params(&dp);
    double denoise_ms = 0.0;
    if (denoise) {
        // the features of the samples every pixel took: all of a plain or
        // --noise-target render, the first --min-spp of an adaptive one
        const auto d0 = std::chrono::high_resolution_clock::now();
        if (denoise_iterations >= 0) dp.iterations = denoise_iterations;
        const int fspp = adaptive ? min_spp : spp_done;
        std::vector<double> features((size_t)nx * ny * RTW_FEATURE_CHANNELS, 0.0), mean(accum.size());
        p.spp_begin = 0, p.spp_count = fspp;
        if (rtw_render_features(h[0], &cam, &p, features.data(), nullptr) != RTW_OK ||
            rtw_denoise(accum.data(), accum_sq.data(), adaptive ? counts.data() : nullptr, spp_done, features.data(), fspp,
                        nx, ny, &dp, mean.data(), nullptr) != RTW_OK ||
            rtw_finalize_canvas_mean(mean.data(), nx, ny, canvas.data()) != RTW_OK) {
            std::fprintf(stderr, "denoise: %s\n", rtw_last_error());
            return 1;
        }
        denoise_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - d0).count();
    } else if (adaptive) rtw_finalize_canvas_counts(accum.data(), counts.data(), nx, ny, canvas.data());
    else rtw_finalize_canvas(accum.data(), nx, ny, spp_done, canvas.data());
    auto t1 = std::chrono::high_resolution_clock::now();
    if (rtw_write_ppm(out.c_str(), canvas.data(), nx, ny) != RTW_OK) {
        std::fprintf(stderr, "write: %s\n", rtw_last_error());
        return 1;
    }
    auto t2 = std::chrono::high_resolution_clock::now();
    using ms = std::chrono::milliseconds;
    std::printf("Trace: %lldms\n", (long long)std::chrono::duration_cast<ms>(t1 - t0).count());
    std::printf("Write: %lldms\n", (long long)std::chrono::duration_cast<ms>(t2 - t1).count());
    std::printf("Msamples/s: %.3f  segments/sample: %.4f\n",
                (double)st.samples / (std::chrono::duration<double>(t1 - t0).count() * 1e6),
                (double)st.segments / (double)st.samples);
    if (noise)
        std::printf("Noise: spp %d of %d  mean_rel %.6e  max_rel %.6e  rms_stderr %.6e\n", spp_done, spp,
                    ns.mean_rel, ns.max_rel, ns.rms_stderr);
    if (adaptive) {
        std::printf("Adaptive: rounds %u  samples %llu of %llu  mean_rel %.6e  max_rel %.6e  at_max %llu", ar.rounds,
                    (unsigned long long)ar.samples, (unsigned long long)nx * ny * spp, ar.final.mean_rel,
                    ar.final.max_rel, (unsigned long long)ar.pixels_at_max);
        if (adaptive_window) std::printf("  window %d", adaptive_window);
        std::printf("\n");
    }
    if (denoise) std::printf("Denoise: iterations %d  %.3f ms\n", dp.iterations, denoise_ms);
    for (void* x : h) rtw_scene_free(x);
    if (gpus > 1) rtw_release_communicators();
    rtw_scene_desc_free(desc);
    return 0;
}
