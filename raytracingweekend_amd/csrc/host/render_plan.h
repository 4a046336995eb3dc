// render_plan.h — how one rtw_render_accumulate call is cut into launches:
// the refusals of its arguments, the resolved sample and row ranges, the pool
// and pass sizes, every buffer's bytes and the arrays carved from them, the
// cameras as the kernels read them and the job's fields.  rtw_plan_call is a
// pure function of its arguments (no HIP, no environment): render_accumulate
// (rtw_kernels.hip) allocates, uploads and launches from its result, and
// tests/cpp/render_plan_check.cpp checks it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include "rtw_div.h"
#include "rtw_gpu.h"
#include "scene_layout.h"

// The fp32 kernels' camera (rtwf::cam32's fields, in its order).
struct call_cam32 {
    float origin[3], lower_left[3], horizontal[3], vertical[3], u[3], v[3];
    float time0, dtime, lens_radius;
};

// Bytes of every buffer a call `ensure`s (0: not needed by this call).
struct call_bytes {
    size_t pool = 0;      // each of the two path pools (paths_bytes)
    size_t fresh = 0;     // staging of new camera rays (fresh_bytes)
    size_t hits = 0;      // hit records: pool doubles (t), then pool int32 (ids) at hits_id_off
    size_t radiance = 0;  // one pass's radiance records
    size_t run = 0;       // per-pixel running sums
    size_t run2 = 0;      // ... of squares (moments renders only)
    size_t camera = 0;    // the device camera and k_recips' two reciprocals after it
    size_t flog = 0;      // the strict build's factor logs
    size_t staging = 0;   // a whole image: the device copy of a host accumulator (each of the two)
    size_t list = 0;      // an active call: the device copy of a host pixel list
    size_t counts = 0;    // ... and of a host counts buffer (a whole image of uint32)
};

// The pixel list of rtw_render_accumulate_active (rtw_adaptive.h), as far as
// the plan reads it: its length and, for the overlap checks only, where the
// list and the counts lie.
struct call_active {
    uint64_t n = 0;
    const void* list = nullptr;
    const void* counts = nullptr;  // may be null
};

struct call_plan {
    // the resolved call
    int spp_count = 0, row_step = 1, n_rows = 0;
    uint64_t npix = 0;      // n_rows * nx; an active call: the list's length
    bool active = false;    // an active call (sample ids index the list: job_t's rows are not read)
    bool noop = false;     // no samples or max_depth <= 0: the accumulator is unchanged, nothing is sized
    uint64_t samples = 0;   // stats.samples of a no-op (spp_count * npix: every sample adds zero)
    bool fast = false;      // precision fp32
    uint32_t pool = 0;      // paths in flight (wavefront form)
    uint64_t pass_spp = 0, pass_samples = 0;  // samples per pixel / samples of a full pass
    call_bytes bytes;
    size_t hits_id_off = 0;
    // cameras
    rtw_camera_desc cam_dev{};  // as copied to the device (a lens-less camera with a non-finite u or v: lens_radius NaN)
    bool pin = false;           // camera_is_pinhole
    call_cam32 cam32{};         // filled for fast renders only
    // job_t's fields that do not change between passes
    uint64_t seed_mix = 0;
    uint32_t cam_pin = 0;
    rtwd::udiv32 div_npix{}, div_nx{};
    uint32_t flog_threads = 0;  // strict build (else 0)
};

// job_t's fields of the pass that starts after `done` samples per pixel, and
// the wavefront form's loop bounds for it.
struct call_pass {
    uint32_t total = 0, spp_pass = 0;
    rtwd::udiv32 div_spp{};
    int32_t s_begin = 0;
    uint32_t fill = 0;      // pool slots the pass starts with: min(pool, total)
    uint64_t iter_cap = 0;  // iterations after which a wavefront pass has failed to drain
};

// The sample range of a render call: [spp_begin, spp_begin + *spp_count) with
// spp_count 0 resolved to the rest of [spp_begin, spp).  RTW_ERR_INVALID with
// "<entry>: bad image / sample parameters" or "<range_prefix>sample range
// exceeds spp" (rtw_render_multi prefixes both with its name).
int rtw_check_sample_range(const rtw_render_params& R, const char* entry, const char* range_prefix, int* spp_count);

// Plans a call.  accum_rgb / accum_sq: the caller's accumulators, for the
// overlap check only (accum_sq null: a plain render).  budget: samples a pass
// may hold (RTW_PASS_SAMPLES).  flog_cus: the device's CUs in the strict
// build, else 0.  RTW_OK, or RTW_ERR_INVALID with the reason; after the
// refusals nothing in it fails.
// act (null: a whole-image call, planned as ever): the call renders the
// act->n listed pixels.  The list takes the rows' place: npix, the passes,
// div_npix and the per-pixel buffers are sized by act->n, `list` and `counts`
// are the device copies a host call needs.  Refused: row_begin != 0 or
// row_step > 1, a null list, more pixels than the image has, and any two of
// the four buffers overlapping.  An empty list is a no-op of 0 samples.
int rtw_plan_call(const rtw_render_params& R, const rtw_camera_desc& camera, const layout_facts& facts,
                  const void* accum_rgb, const void* accum_sq, size_t budget, int flog_cus, call_plan* out,
                  const call_active* act = nullptr);

call_pass rtw_plan_pass(const call_plan& P, const rtw_render_params& R, uint64_t done);

inline uint64_t rtw_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- the pools' layout -------------------------------------------------------
// A pool is one allocation holding its arrays back to back, doubles first.
// The kernels' SoA structs (paths_t, fresh_t) live in the kernel translation
// unit -- their names are part of the kernels' symbols -- so the carving is a
// template over them: any struct with these members.
inline size_t rtw_paths_bytes(uint32_t cap) { return (size_t)cap * (10 * 8 + 3 * 4); }
inline size_t rtw_fresh_bytes(uint32_t cap) { return (size_t)cap * (7 * 8 + 2 * 4); }

template <class P>
P rtw_carve_paths(void* base, uint32_t cap) {
    char* p = static_cast<char*>(base);
    P A;
    double** d[] = {&A.ox, &A.oy, &A.oz, &A.dx, &A.dy, &A.dz, &A.tm, &A.tr, &A.tg, &A.tb};
    for (double** x : d) {
        *x = reinterpret_cast<double*>(p);
        p += (size_t)cap * 8;
    }
    uint32_t** u[] = {&A.rng, &A.depth, &A.qid};
    for (uint32_t** x : u) {
        *x = reinterpret_cast<uint32_t*>(p);
        p += (size_t)cap * 4;
    }
    return A;
}

template <class F>
F rtw_carve_fresh(void* base, uint32_t cap) {
    char* p = static_cast<char*>(base);
    F A;
    double** d[] = {&A.ox, &A.oy, &A.oz, &A.dx, &A.dy, &A.dz, &A.tm};
    for (double** x : d) {
        *x = reinterpret_cast<double*>(p);
        p += (size_t)cap * 8;
    }
    A.rng = reinterpret_cast<uint32_t*>(p);
    A.qid = A.rng + cap;
    return A;
}

// the hit records' two arrays: t of every slot, then the hit ids
inline size_t rtw_hits_bytes(uint32_t cap) { return (size_t)cap * 12; }
inline size_t rtw_hits_id_off(uint32_t cap) { return (size_t)cap * 8; }
