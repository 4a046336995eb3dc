// rtw_kernels.hip — the wavefront path tracer for gfx950 and the C ABI
// around it (include/rtw_gpu.h).
//
// Replaces the triple `_for` of RayTracingWeekend.cpp:211-250.  The recursion
// of color() (RayTracingWeekend.cpp:45-160) is unrolled into an iterative
// wavefront over a pool of in-flight paths kept as SoA arrays in HBM:
//
//   k_fill + k_regen   empty pool, then camera ray-gen for the first samples
//   repeat:
//     k_intersect  one world closest-hit query per live path   (traversal)
//     k_shade      emission / scatter / mixture-pdf sampling per path; a
//                  path that ends writes its 24-byte radiance record to its
//                  sample's slot of the pass's radiance buffer and empties
//                  its pool slot
//     k_regen      (until the sample queue is drained) refills empty slots:
//                  per-block compaction of the empty slots, one atomic on a
//                  sharded sample queue per 1024 slots, camera rays written
//                  densely to a staging buffer, a 4-byte marker per slot
//     k_compact    (tail only, once the sample queue is drained) stream
//                  compaction of live paths, __ballot/prefix-sum per tile
//   k_reduce     per-pixel sum of the samples in increasing sample order
//                (k_reduce_moments: and of their squares, rtw_noise.h)
//
// Paths are independent (the RNG is keyed by (seed, pixel, sample)), so the
// pool order never changes a result, only its speed.
//
// Renders run the persistent kernels by default (k_persist_sort, k_persist,
// k_fast_sort, k_fast below: a whole path per lane, chosen by rtw_select.h).
// The device scene they read is laid out in host/scene_layout.cpp (records: rtw_layout.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>
#include "rtw_device.h"
#include "rtw_fast.h"
#include "rtw_queue.h"
#include "host/adaptive.h"
#include "host/adaptive_window.h"
#include "host/denoise.h"
#include "host/query.h"
#include "host/radiance.h"
#include "host/render_plan.h"
#include "host/rtw_host_util.h"
#include "host/scene_layout.h"

using namespace rtwd;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPWaves = kPBlock / 64;  // k_persist's workgroup (rtw_device.h kPBlock)

// Path pool (SoA, one element per slot).  depth word of a slot:
//   0                    empty
//   1..max_depth         live path: the depth argument of its next color() call
//   kFresh | k           a new camera sample whose ray / time / rng / sample id
//                        sit in staging entry k (written densely by k_regen);
//                        its throughput is 1 and its depth max_depth
constexpr uint32_t kFresh = 0x80000000u;

struct paths_t {
    double *ox, *oy, *oz, *dx, *dy, *dz, *tm, *tr, *tg, *tb;
    uint32_t *rng, *depth, *qid;
};

struct fresh_t {  // staging of new camera rays, indexed like the pool
    double *ox, *oy, *oz, *dx, *dy, *dz, *tm;
    uint32_t *rng, *qid;
};

struct job_t {
    const rtw_camera_desc* cam;  // device copy (read where rays are made, see camera_sample)
    uint64_t seed_mix;   // splitmix64(seed)
    uint32_t total;      // samples in this pass
    uint32_t npix;       // pixels of this call (n_rows * nx)
    int32_t nx, ny, row_begin, row_step, s_begin, max_depth;
    uint32_t spp_pass;   // samples per pixel in this pass
    uint32_t cam_pin;    // camera_is_pinhole(camera): camera_ray's pinhole shortcut applies
    rtwd::udiv32 div_npix, div_nx, div_spp;  // magic numbers of npix, nx, spp_pass (sample_coords)
    double* L;           // per-sample radiance, L[3q + c] (pass-local sample id q)
#if RTW_STRICT_RADIANCE
    // per-thread factor logs of the strict build: bounce k of the path on
    // global thread g at flog[4 (k * flog_threads + g)] = (m.x, m.y, m.z, pdf)
    double* flog;
    uint32_t flog_threads;
#endif
};

// Pass-local sample ids are sample-major: q = sample * npix + pixel, so a
// wave's 64 consecutive ids are 64 neighbouring pixels and k_reduce reads
// each sample plane coalesced.  (Pixel-major ids fill whole lines with a
// wave's records but make k_reduce stage each pixel's run through LDS: the
// step -0.5 %, profiles/r03/ab_pixel_major.log.)  Results do not depend on
// the order: the RNG is keyed by (pixel, sample) and each pixel's records are
// summed in sample order.

// A sample's radiance record.  (Non-temporal stores measured +-0 on T and
// C5, profiles/r05/ab_r5b_*.log.)
template <typename T>
__device__ __forceinline__ void store_record(T* o, T x, T y, T z) {
    o[0] = x, o[1] = y, o[2] = z;
}

// An active call (rtw_adaptive.h) has no row sharding: its pixel list lies
// over row_begin / row_step, 8 bytes at an 8-byte-aligned offset.  job_t is
// the middle of the persistent kernels' argument and its layout theirs, so it
// does not grow; only kernels compiled with F_ACTIVE read the pointer.
static_assert(offsetof(job_t, row_begin) % 8 == 0 && offsetof(job_t, row_step) == offsetof(job_t, row_begin) + 4,
              "the active list's pointer overlays row_begin / row_step");
__device__ __forceinline__ const uint32_t* job_active_list(const job_t& J) {
    const uint32_t* list;
    __builtin_memcpy(&list, &J.row_begin, sizeof list);
    return list;
}

// pass-local sample id -> pixel (i, j) and global sample index s
// ACTIVE: the id's pixel part indexes the call's list of pixel indices (one
// coalesced 4-byte load per new camera sample, in the refill phase; not
// loop-carried).  Ids stay dense in [0, spp_pass * n_active), so the RNG key
// j*nx + i, the jitter and the record at L[3q] need nothing else.
template <bool ACTIVE = false>
__device__ __forceinline__ void sample_coords(const job_t& J, uint32_t q, int& i, int& j, int& s) {
// (the quotients by exact magic-number division, rtw_div.h udiv_fast)
    const uint32_t sl = udiv_fast(q, J.div_npix);
    const uint32_t rem = q - sl * J.npix;
    if constexpr (ACTIVE) {
        const uint32_t pixel = job_active_list(J)[rem];
        const uint32_t k = udiv_fast(pixel, J.div_nx);
        i = (int)(pixel - k * (uint32_t)J.nx);
        j = (int)k;
    } else {
        const uint32_t k = udiv_fast(rem, J.div_nx);
        i = (int)(rem - k * (uint32_t)J.nx);
        j = J.row_begin + (int)k * J.row_step;
    }
    s = J.s_begin + (int)sl;
}

// Render-loop body RayTracingWeekend.cpp:227-231 for sample q: jitter,
// camera::get_ray -> staging entry k.
// JPIN: the pinhole shortcut applies per the job's host-computed flag
// (J.cam_pin), else per the device camera's own lens_radius == 0 and nonzero
// origin -- the host gives a lens-less camera with a non-finite u or v a NaN
// lens_radius in the device copy, so both say the same.  (The two forms
// measure differently through code layout alone: J.cam_pin T +0.6 %, the
// camera test C3 +1.5 %, profiles/r06/ab_r6h_*.log; each kernel takes its
// better one.)
template <bool JPIN = true, bool ACTIVE = false>
__device__ __forceinline__ ray camera_sample(const job_t& J, uint32_t q, uint32_t& rng) {
    int i, j, s;
    sample_coords<ACTIVE>(J, q, i, j, s);
    rng = path_seed(J.seed_mix, (uint32_t)(j * J.nx + i), (uint32_t)s);
    // The camera (23 doubles) is loaded here, with scalar loads, each time
    // rays are made: an opaque pointer stops the compiler from hoisting it
    // into loop-carried SGPRs of the persistent loop, where it spills.
    const rtw_camera_desc* cp = J.cam;
    asm volatile("" : "+s"(cp));
    // u = (i + U) / nx, v = (j + U) / ny with the device's own reciprocals of
    // nx, ny (k_recips, stored after the camera): rtw_div.h's div_hw is the
    // compiler's division sequence bit for bit when the divisor is in
    // [2^-200, 2^200] and the numerator 0 or in [2^-800, 2^100] -- here the
    // divisor is an image size and the numerator 0 or at least 2^-62 (a
    // canonical draw's grain) and below 2^32; +0 / n gives +0 either way.
    // With the magic-number sample decomposition, measured (1 MI355X, A/B,
    // profiles/r05/ab_r5m_udiv_recips.log; bit-identical images,
    // parity_r5m.log): T 4 741 vs 4 705 (+0.8 %), C3 +1.2 %, C5 -0.5 %,
    // T fp32 -0.3 %.
    const double* yr = reinterpret_cast<const double*>(cp + 1);
    const double u = div_hw((double)(i + rnd01(rng)), (double)J.nx, ld(yr));
    const double v = div_hw((double)(j + rnd01(rng)), (double)J.ny, ld(yr + 1));
    rtw_camera_desc c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.origin[k] = ld(&cp->origin[k]);
        c.lower_left[k] = ld(&cp->lower_left[k]);
        c.horizontal[k] = ld(&cp->horizontal[k]);
        c.vertical[k] = ld(&cp->vertical[k]);
        c.u[k] = ld(&cp->u[k]);
        c.v[k] = ld(&cp->v[k]);
    }
    c.time0 = ld(&cp->time0);
    c.time1 = ld(&cp->time1);
    c.lens_radius = ld(&cp->lens_radius);
    const bool pin = JPIN ? J.cam_pin != 0
                          : (c.lens_radius == 0.0 && c.origin[0] != 0.0 && c.origin[1] != 0.0 && c.origin[2] != 0.0);
    return camera_ray(c, u, v, rng, pin);
}
// ... and of the fp32 fast mode (rtw_fast.h): the same sample decomposition
// and engine, single-precision jitter and camera
template <bool ACTIVE = false>
__device__ __forceinline__ rtwf::fray camera_sample_f32(const job_t& J, const rtwf::cam32& cam, uint32_t q,
                                                        uint32_t& rng) {
    int i, j, s;
    sample_coords<ACTIVE>(J, q, i, j, s);
    rng = path_seed(J.seed_mix, (uint32_t)(j * J.nx + i), (uint32_t)s);
    const float u = ((float)i + rtwf::u01(rng)) * rtwf::rcp((float)J.nx);
    const float v = ((float)j + rtwf::u01(rng)) * rtwf::rcp((float)J.ny);
    return rtwf::camera_ray(cam, u, v, rng);
}

// A ray-sourced job (rtw_radiance.h): a fresh path starts from a record of the
// caller's, not from the camera, so the job's camera fields are not read.  As
// with the active list, job_t does not grow: the ray records lie over `cam`
// (a pointer already), the caller's stream states (null: keyed streams) over
// row_begin / row_step, and the first ray's RNG key over nx.  Only
// k_regen_rays and the F_RAYS rows read them (ray_sample).
static_assert(offsetof(job_t, cam) == 0 && sizeof(job_t::cam) == sizeof(const rtw_query_ray*) &&
                  offsetof(job_t, cam) + sizeof(job_t::cam) <= offsetof(job_t, seed_mix),
              "the ray records' pointer overlays cam and nothing else");
static_assert(offsetof(job_t, row_begin) % 8 == 0 && offsetof(job_t, row_step) == offsetof(job_t, row_begin) + 4 &&
                  sizeof(job_t::row_begin) + sizeof(job_t::row_step) == sizeof(const uint32_t*),
              "the caller's stream states' pointer overlays row_begin / row_step, as the active list's does");
static_assert(sizeof(job_t::nx) == sizeof(uint32_t) &&
                  (offsetof(job_t, nx) + sizeof(job_t::nx) <= offsetof(job_t, row_begin) ||
                   offsetof(job_t, nx) >= offsetof(job_t, row_step) + sizeof(job_t::row_step)) &&
                  offsetof(job_t, nx) >= offsetof(job_t, cam) + sizeof(job_t::cam),
              "the first key overlays nx, clear of the two pointers");
// (the fields a ray-sourced job still reads -- seed_mix, total, npix, s_begin, max_depth, div_npix, L -- are
// none of cam, nx, row_begin, row_step)
__device__ __forceinline__ const rtw_query_ray* job_rays(const job_t& J) {
    const rtw_query_ray* rays;
    __builtin_memcpy(&rays, &J.cam, sizeof rays);
    return rays;
}
__device__ __forceinline__ const uint32_t* job_ray_rng(const job_t& J) { return job_active_list(J); }
__device__ __forceinline__ uint32_t job_first_key(const job_t& J) { return (uint32_t)J.nx; }

// The start of sample q of a ray-sourced job: q = sample * n_rays + ray, the
// sample-major order k_reduce sums.  The lane loads its 64-byte record as
// k_query does (16-byte loads with per-lane addresses, a wave's together whole
// lines; vector loads, where the refill happens, so nothing of the record is
// loop-carried beyond the fresh path itself); t_max is not read, and with
// TIME false (F_STATIC rows keep no time per path) neither is the time: the
// record's last 16 bytes are then not loaded.  The stream is the caller's
// state of the ray, or path_seed of (first_key + ray, sample); nothing draws
// from it before color().
template <bool TIME = true>
__device__ __forceinline__ ray ray_sample(const job_t& J, uint32_t q, uint32_t& rng) {
    const uint32_t sl = udiv_fast(q, J.div_npix);
    const uint32_t k = q - sl * J.npix;
    const double2* in = reinterpret_cast<const double2*>(job_rays(J) + k);
    const double2 a = in[0], b = in[1], c = in[2];
    ray r;
    r.o = d3{a.x, a.y, b.x}, r.d = d3{b.y, c.x, c.y}, r.t = 0.0;
    if constexpr (TIME) r.t = in[3].x;
    const uint32_t* states = job_ray_rng(J);
    rng = states ? states[k] : path_seed(J.seed_mix, job_first_key(J) + k, (uint32_t)(J.s_begin + (int)sl));
    return r;
}
// A fresh path of a persistent kernel: the camera's sample, or with F_RAYS the caller's ray.
template <int F, bool JPIN>
__device__ __forceinline__ ray fresh_sample(const job_t& J, uint32_t q, uint32_t& rng) {
    if constexpr ((F & F_RAYS) != 0)
        return ray_sample<(F & F_STATIC) == 0>(J, q, rng);
    else
        return camera_sample<JPIN, (F & F_ACTIVE) != 0>(J, q, rng);
}

// RAYS: of a ray-sourced job (ACTIVE does not apply)
template <bool ACTIVE = false, bool RAYS = false>
__device__ __forceinline__ void raygen(const job_t& J, const fresh_t& F, uint32_t k, uint32_t q) {
    uint32_t rng;
    const ray r = RAYS ? ray_sample<true>(J, q, rng) : camera_sample<true, ACTIVE>(J, q, rng);
    F.ox[k] = r.o.x, F.oy[k] = r.o.y, F.oz[k] = r.o.z;
    F.dx[k] = r.d.x, F.dy[k] = r.d.y, F.dz[k] = r.d.z;
    F.tm[k] = r.t;
    F.rng[k] = rng;
    F.qid[k] = q;
}

// A path as the kernels see it: from the pool, or from staging when fresh.
struct path_in {
    ray r;
    uint32_t depth;
    bool fresh;
    uint32_t src;  // staging index (fresh) or pool slot
};

__device__ __forceinline__ path_in load_ray(const paths_t& P, const fresh_t& F, uint32_t i, uint32_t dw) {
    path_in x;
    x.fresh = (dw & kFresh) != 0;
    x.src = x.fresh ? (dw & ~kFresh) : i;
    // one load per field with a per-lane address: no divergence between
    // fresh and continuing paths
    x.r.o.x = *(x.fresh ? F.ox + x.src : P.ox + i);
    x.r.o.y = *(x.fresh ? F.oy + x.src : P.oy + i);
    x.r.o.z = *(x.fresh ? F.oz + x.src : P.oz + i);
    x.r.d.x = *(x.fresh ? F.dx + x.src : P.dx + i);
    x.r.d.y = *(x.fresh ? F.dy + x.src : P.dy + i);
    x.r.d.z = *(x.fresh ? F.dz + x.src : P.dz + i);
    x.r.t = *(x.fresh ? F.tm + x.src : P.tm + i);
    x.depth = dw;
    return x;
}

// Start a pass: slots [0, n0) empty (depth 0) for k_regen to fill.
__global__ __launch_bounds__(kBlock) void k_fill(paths_t P, ctrs_t* C, uint32_t n0) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n0) P.depth[i] = 0;
    if (i == 0) C->n = n0;
    if (i < kQShards) C->qshard[i].v = 0;
}

// rcp_hw of the image's width and height for camera_sample, once per render
// call, into the two doubles after the camera's device copy
__global__ void k_recips(double* out, int nx, int ny) {
    if (threadIdx.x == 0) out[0] = rcp_hw((double)nx), out[1] = rcp_hw((double)ny);
}

__device__ __forceinline__ unsigned long long lanemask_lt() {
    const unsigned lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// block-wide exclusive prefix of a per-lane flag; returns this lane's rank and
// writes the block total to *total (all lanes).
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* s_wave, uint32_t& total) {
    const unsigned long long m = __ballot(flag);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_wave[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const uint32_t c = s_wave[k];
        before += (k < (int)w) ? c : 0u;
        tot += c;
    }
    total = tot;
    return before + (uint32_t)__popcll(m & lanemask_lt());
}

// Two steps the persistent kernels share.  (The wavefront kernels spell them
// out: through these functions k_intersect, k_segment and k_shade compile to
// other instruction orders, and nothing times those kernels.)
// Copy n16 16-byte units from src into LDS, the block's `block` threads
// striding over them (the caller's barrier follows).
__device__ __forceinline__ void stage_lds(char* lds, const void* src, uint32_t n16, uint32_t block) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(lds);
    for (uint32_t k = threadIdx.x; k < n16; k += block) d[k] = s[k];
}
// The segment counter: every lane's count of world hit queries, folded per
// wave into s_cnt[WAVES], then one 64-bit atomic per block.  ctrs() gives the
// counters where thread 0 adds to them: the kernels load the pointer there
// (loaded before the barrier it cost k_fast<2, true> a spilled VGPR).
template <int WAVES, class Ctrs>
__device__ __forceinline__ void count_segments(uint32_t segs, uint32_t* s_cnt, Ctrs ctrs) {
    for (int off = 32; off > 0; off >>= 1) segs += __shfl_down(segs, off, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = segs;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < WAVES; ++k) t += s_cnt[k];
        if (t) atomicAdd(&ctrs()->segments[blockIdx.x % 8].v, t);
    }
}

// One world closest-hit query per live path.  The next path's ray is loaded
// while the current one is traversed (software pipelining of the HBM reads).
template <int F>
__global__ __launch_bounds__(kBlock) void k_intersect(scene S, paths_t P, fresh_t FR, double* __restrict__ ht,
                                                      int32_t* __restrict__ hid, ctrs_t* C) {
    __shared__ uint32_t s_cnt[kWaves];
    const uint32_t n = C->n;
    const uint32_t stride = gridDim.x * kBlock;
    uint32_t live = 0;
    uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t dw = i < n ? P.depth[i] : 0u;
    path_in cur = load_ray(P, FR, i < n ? i : 0, dw);
    while (i < n) {
        const uint32_t nx = i + stride;
        const uint32_t ndw = nx < n ? P.depth[nx] : 0u;
        const path_in nxt = load_ray(P, FR, nx < n ? nx : i, ndw);
        if (dw != 0) {
            uint32_t rng = 0u;
            if (F & F_MEDIA) rng = cur.fresh ? FR.rng[cur.src] : P.rng[i];
            const hit_state h = world_closest<F>(S, cur.r, rng);
            if (F & F_MEDIA) {
                if (cur.fresh)
                    FR.rng[cur.src] = rng;
                else
                    P.rng[i] = rng;
            }
            ht[i] = h.t;
            hid[i] = h.prim;
            ++live;
        }
        i = nx;
        dw = ndw;
        cur = nxt;
    }
    // one 64-bit atomic per block for the segment counter
    for (int off = 32; off > 0; off >>= 1) live += __shfl_down(live, off, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = live;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < kWaves; ++k) t += s_cnt[k];
        if (t) atomicAdd(&C->segments[blockIdx.x % 8].v, t);
    }
}

// Section profiler (profiling builds only: -DRTW_PROF).  Each lane charges
// the clock since its previous mark to the section it just finished; the
// per-lane sums land in g_prof and rtw_render_accumulate prints them.
enum { PS_LOOP, PS_LOAD, PS_TRAVERSE, PS_HIT, PS_SAMPLE, PS_PDF, PS_STORE, PS_N };
#ifdef RTW_PROF
__device__ unsigned long long g_prof[PS_N];
__device__ unsigned long long g_cls[2][8];  // [0] lanes per class, [1] waves with the class present
struct prof_t {
    uint64_t t;
    uint64_t acc[PS_N];
    uint32_t lanes[8] = {0, 0, 0, 0, 0, 0, 0, 0}, waves[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // segment class of this lane: 0 miss, 1+type material hit, 7 idle
    __device__ __forceinline__ void classify(int cls) {
        for (int k = 0; k < 8; ++k) {
            const unsigned long long m = __ballot(cls == k);
            lanes[k] += (uint32_t)__popcll(m);
            waves[k] += m ? 1u : 0u;
        }
    }
    __device__ prof_t() : t(clock64()) {
        for (int k = 0; k < PS_N; ++k) acc[k] = 0;
    }
    __device__ __forceinline__ void mark(int k) {
        const uint64_t now = clock64();
        acc[k] += now - t;
        t = now;
    }
    __device__ void flush() {
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 8; ++k) {
                atomicAdd(&g_cls[0][k], (unsigned long long)lanes[k]);
                atomicAdd(&g_cls[1][k], (unsigned long long)waves[k]);
            }
        for (int k = 0; k < PS_N; ++k) {
            unsigned long long v = acc[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((threadIdx.x & 63) == 0) atomicAdd(&g_prof[k], v);
        }
    }
};
#elif defined(RTW_REGIONS)  // static attribution: region markers in the ISA
struct prof_t {
    __device__ __forceinline__ void classify(int) {}
    __device__ __forceinline__ void mark(int k) { asm volatile(";RTW_REGION %0" ::"i"(k)); }
    __device__ __forceinline__ void flush() {}
};
#else
struct prof_t {
    __device__ __forceinline__ void classify(int) {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush() {}
};
#endif

// Background of RayTracingWeekend.cpp:141-159.
__device__ __forceinline__ d3 background(const scene& S, const d3& dir) {
    if (S.background != RTW_BG_GRADIENT) return d3{0, 0, 0};
    const d3 u = normalize(dir);
    const double t = 0.5f * (u.y + 1.0);
    return d3{1.0, 1.0, 1.0} * (1.0 - t) + d3{0.5f, 0.7f, 1.0} * t;  // lerp, vec3.h:84-87
}

// A path between two color() calls: the ray of the next call, its engine,
// the depth argument of the next call and its sample id.  (The throughput,
// the product of the attenuation / pdf factors so far, is kept by the caller:
// the persistent kernel parks it in LDS, out of the register budget.)
struct path_st {
    ray r;
    uint32_t rng, depth, q;
};

// Outcome of one segment: the path continues with throughput *= f and the
// next call's ray, or ends with radiance thr * E, or ends with radiance 0.
enum { SEG_CONTINUE = 0, SEG_END = 1, SEG_END_ZERO = 2 };
constexpr uint32_t kDepthBits = 0x3fffffffu;  // a path's depth (bits above: reserved, zero)

// A sink receives the outcome inside the shading branch that produced it:
//   cont(f, next)   the path continues (throughput *= f, ray `next`)
//   end(E)          it ends with radiance thr * E
//   end_zero()      it ends with radiance 0
// seg_out keeps the outcome for the caller (wavefront kernels); the
// persistent kernels' sinks apply it on the spot (LDS throughput update,
// continuation ray into the path's slot, radiance store), so no value of a
// branch is live across the merge of the exec-masked branches, which run
// one after the other.
//   cont_mp(m, pdf, next)  (RTW_STRICT_RADIANCE, the lambertian bounce) the
//                   path continues with the factor m / pdf, m = attenuation
//                   * scattering_pdf, kept apart for the inside-out fold
struct seg_out {
    d3 w;      // f or E
    ray next;  // SEG_CONTINUE only
    RTW_D void cont(const d3& f, const ray& nr) { w = f, next = nr; }
    RTW_D void cont_mp(const d3& m, double pdf, const ray& nr) { cont(m / pdf, nr); }
    RTW_D void end(const d3& E) { w = E; }
    RTW_D void end_zero() {}
};
template <class C, class E, class Z>
struct fn_sink {  // a sink from three callables
    C c;
    E e;
    Z z;
    RTW_D void cont(const d3& f, const ray& nr) { c(f, nr); }
    RTW_D void cont_mp(const d3& m, double pdf, const ray& nr) { c(m / pdf, nr); }
    RTW_D void end(const d3& L) { e(L); }
    RTW_D void end_zero() { z(); }
};
template <class C, class E, class Z>
RTW_D fn_sink<C, E, Z> make_sink(C c, E e, Z z) { return fn_sink<C, E, Z>{c, e, z}; }
// ... and from four: cont_mp of its own (the strict build's k_persist)
template <class C, class M, class E, class Z>
struct fn_sink4 {
    C c;
    M cm;
    E e;
    Z z;
    RTW_D void cont(const d3& f, const ray& nr) { c(f, nr); }
    RTW_D void cont_mp(const d3& m, double pdf, const ray& nr) { cm(m, pdf, nr); }
    RTW_D void end(const d3& L) { e(L); }
    RTW_D void end_zero() { z(); }
};
template <class C, class M, class E, class Z>
RTW_D fn_sink4<C, M, E, Z> make_sink4(C c, M cm, E e, Z z) { return fn_sink4<C, M, E, Z>{c, cm, e, z}; }

// One segment of color() (RayTracingWeekend.cpp:52-159) for path x whose
// world hit is (t, prim); returns the outcome (SEG_*) after handing it to
// the sink.  x.r is only read; on SEG_CONTINUE x.rng and x.depth advance.
// The recursion's inside-out products are folded forward: the radiance of a
// path is thr * (last emitted / background), thr the product of the
// reference's per-bounce factors attenuation * scattering_pdf / pdf (or
// attenuation for specular scatter).
template <int M, bool STATIC = false, bool LIGHTS = false, bool BLACK = false, bool NOLIGHTS = false, class SINK>
__device__ __forceinline__ int shade_core(const scene& S, path_st& x, double t, int32_t prim, SINK& sk,
                                          prof_t& pf) {
    const ray r = x.r;
    uint32_t rng = x.rng;
    const uint32_t depth = x.depth;
    // the scattered branches' common tail: the next color() call has depth
    // depth - 1, and returns 0 when that is 0
    auto scatter = [&](const d3& f, const d3& p, const d3& dir) -> int {
        if (depth <= 1) {
            sk.end_zero();
            return SEG_END_ZERO;
        }
        sk.cont(f, ray{p, dir, r.t});
        x.rng = rng;
        x.depth = depth - 1;
        return SEG_CONTINUE;
    };
    if (prim == -1) {
        sk.end(BLACK ? d3{0, 0, 0} : background(S, r.d));
        return SEG_END;
    }
    d3 p, n, sl{0, 0, 0};  // sl: what (u, v) come from, SF_IMAGE kernels only
    int mat;
    bool rect;
    hit_record<(M & SF_ISO) != 0, STATIC, (M & SF_IMAGE) != 0>(S, r, hit_state{t, prim, false}, p, n, mat, rect, sl);
    if (!BLACK && S.render_type == RTW_RENDER_NORMAL) {  // :135-136
        sk.end(d3{0.5f, 0.5f, 0.5f} * (n + d3{1, 1, 1}));
        return SEG_END;
    }
    const rtw_material& m = S.materials[mat];
    pf.mark(PS_HIT);
    if (m.type == RTW_MAT_DIFFUSE_LIGHT) {  // material.h:232-244: no scatter
        if (!(dot(n, r.d) > 0)) {
            sk.end_zero();
            return SEG_END_ZERO;
        }
        sk.end(texture_value<M>(S, m.texture, p, prim, sl));
        return SEG_END;
    } else if ((M & SF_METAL) && m.type == RTW_MAT_METAL) {  // material.h:128-136
        const d3 reflected = reflect(normalize(r.d), n);
        const d3 dir = reflected + random_in_unit_sphere(rng) * m.fuzz;
        return scatter(ld3(m.albedo), p, dir);
    } else if ((M & SF_DIEL) && m.type == RTW_MAT_DIELECTRIC) {  // material.h:146-222
        d3 outward;
        double ni_over_nt, cosine;
        const double ri = m.ref_idx;
        if (dot(r.d, n) > 0) {
            outward = -n;
            ni_over_nt = ri;
            cosine = dot(r.d, n) / len(r.d);
            cosine = RTW_SQRT(1 - ri * ri * (1 - cosine * cosine));
        } else {
            outward = n;
            ni_over_nt = S.mat_aux[2 * mat];  // 1.0 / ri, host-computed
            cosine = -dot(r.d, n) / len(r.d);
        }
        const d3 reflected = reflect(r.d, n);
        d3 refracted{0, 0, 0};
        const double reflect_prob = refract(r.d, outward, ni_over_nt, refracted) ? schlick_r0(cosine, S.mat_aux[2 * mat + 1]) : 1.0;
        const d3 dir = (rnd01(rng) < reflect_prob) ? reflected : refracted;
        return scatter(d3{1.0, 1.0, 1.0}, p, dir);
    } else if ((M & SF_ISO) && m.type == RTW_MAT_ISOTROPIC) {  // material.h:257-262
        const d3 dir = random_in_unit_sphere(rng);
        return scatter(texture_value<M>(S, m.texture, p, prim, sl), p, dir);
    } else {  // lambertian material.h:81-119 + RayTracingWeekend.cpp:112-132
        // (RTW_RADIANCE_FAST: quantities that only scale radiance -- the
        // attenuation / pdf factor and the pdfs' magnitudes -- are formed with
        // fewer divisions than the reference's expressions; everything a
        // decision reads -- directions, t, the sign of pdf_val -- is the
        // reference's own arithmetic.  See RTW_RADIANCE_FAST below.)
        // onb::build_from_w(normal) (onb.h:32-38), built where it is used
        const surf_frame sf{n, prim, rect, true};
        pf.mark(PS_HIT);
        d3 dir;
        double pdf_val, cosine;
        if (LIGHTS || (!NOLIGHTS && S.n_lights > 0)) {  // mixture_pdf(cosine_pdf, hittable_pdf(lights)) pdf.h:55-79
            dir = mixture_generate(S, sf, p, rng);
            pf.mark(PS_SAMPLE);
            // both cosines before the light pdfs, so the normal and the frame
            // are dead while those run (the values are what the reference
            // computes after them)
            const d3 ud = normalize(dir);
            const double cw = dot(ud, frame_w(S, sf));
            cosine = dot(n, ud);  // material.h:115-119
            const double p0 = (cw <= 0) ? 0 : (RTW_RADIANCE_FAST ? cw * kInvPi : cw / kPi);
            pdf_val = 0.5 * p0 + 0.5 * lights_pdf_value<STATIC>(S, p, dir);
        } else {
            dir = local(frame_onb(S, sf), random_cosine_direction(rng));
            const d3 ud = normalize(dir);
            const double cw = dot(ud, frame_w(S, sf));
            cosine = dot(n, ud);  // material.h:115-119
            pdf_val = (cw <= 0) ? 0 : (RTW_RADIANCE_FAST ? cw * kInvPi : cw / kPi);
        }
        if (pdf_val <= 0.0) {  // :126-127 returns emitted (= 0)
            sk.end_zero();
            return SEG_END_ZERO;
        }
        pf.mark(PS_PDF);
        // attenuation = texture value (material.h:98), read only now: it
        // draws nothing, and a late read keeps it out of the busiest registers
#if RTW_RADIANCE_FAST
        // attenuation * scattering_pdf / pdf_val as one scalar quotient
        const double w = cosine < 0 ? 0 : rad_div(cosine, kPi * pdf_val);
        return scatter(texture_value<M>(S, m.texture, p, prim, sl) * w, p, dir);
#elif RTW_STRICT_RADIANCE
        // the reference's ((attenuation * scattering_pdf) * color) / pdf_val
        // (RayTracingWeekend.cpp:129-132): m and pdf_val go to the path's
        // factor log; the fold applies them around the returned color
        const double spdf = cosine < 0 ? 0 : cosine / kPi;
        if (depth <= 1) {
            sk.end_zero();
            return SEG_END_ZERO;
        }
        sk.cont_mp(texture_value<M>(S, m.texture, p, prim, sl) * spdf, pdf_val, ray{p, dir, r.t});
        x.rng = rng;
        x.depth = depth - 1;
        return SEG_CONTINUE;
#else
        const double spdf = cosine < 0 ? 0 : cosine / kPi;
        return scatter((texture_value<M>(S, m.texture, p, prim, sl) * spdf) / pdf_val, p, dir);
#endif
    }
}

// The wavefront form: path x (read from pool slot i or, fresh, from staging)
// -> shade_core -> continuation written back to slot i (no longer fresh).
template <int M>
__device__ __forceinline__ bool shade_one(const scene& S, const job_t& J, const paths_t& P, const fresh_t& FR,
                                          uint32_t i, const path_in& x, uint32_t rng, double t, int32_t prim, d3& L,
                                          uint32_t& q, prof_t& pf) {
    path_st s;
    s.r = x.r;
    s.rng = rng;
    s.depth = x.fresh ? (uint32_t)J.max_depth : x.depth;
    s.q = x.fresh ? FR.qid[x.src] : P.qid[i];
    q = s.q;
    seg_out so;
    const int out = shade_core<M>(S, s, t, prim, so, pf);
    const d3 w = so.w;
    const ray nr = so.next;
    const d3 thr = x.fresh ? d3{1.0, 1.0, 1.0} : d3{P.tr[i], P.tg[i], P.tb[i]};
    if (out == SEG_END) {
        L = thr * w;
        return true;
    }
    if (out == SEG_END_ZERO) {
        L = thr * 0.0;  // (NaN / inf throughputs give NaN, as the reference's products do)
        return true;
    }
    const d3 nt = thr * w;
    P.ox[i] = nr.o.x, P.oy[i] = nr.o.y, P.oz[i] = nr.o.z;
    P.dx[i] = nr.d.x, P.dy[i] = nr.d.y, P.dz[i] = nr.d.z;
    P.tm[i] = nr.t;
    P.tr[i] = nt.x, P.tg[i] = nt.y, P.tb[i] = nt.z;
    P.rng[i] = s.rng;
    P.depth[i] = s.depth;
    P.qid[i] = s.q;
    return false;
}

// Re-point a scene's shading arrays into an LDS copy of its prefix.
__device__ __forceinline__ scene lds_scene(const scene& S, const char* base, const char* lds) {
    scene L = S;
    auto rb = [&](const void* p) -> const void* { return p ? (const void*)(lds + ((const char*)p - base)) : nullptr; };
    L.prims = (const rtw_prim*)rb(S.prims);
    L.entries = (const dev_entry*)rb(S.entries);
    L.ops = (const dev_op*)rb(S.ops);
    L.materials = (const rtw_material*)rb(S.materials);
    L.textures = (const rtw_texture*)rb(S.textures);
    L.lights = (const rtw_light*)rb(S.lights);
    L.ranvec = (const double*)rb(S.ranvec);
    L.perm = (const int32_t*)rb(S.perm);
    L.media = (const int32_t*)rb(S.media);
    L.prim_onb = (const double*)rb(S.prim_onb);
    L.mat_aux = (const double*)rb(S.mat_aux);
    return L;
}

// Shade every live path; a path that ends stores its radiance in its sample's
// slot of the radiance buffer (one 24-byte record) and empties its pool slot.
// With LDS, a small scene's shading data (prims .. media, `bytes` from `base`)
// is staged in LDS once per block: the dependent chain hit -> primitive ->
// entry -> material -> texture is then LDS latency, not L2 latency.
template <int M, bool LDS>
__global__ __launch_bounds__(kBlock) void k_shade(scene S, job_t J, paths_t P, fresh_t FR,
                                                  const double* __restrict__ ht, const int32_t* __restrict__ hid,
                                                  ctrs_t* C, const char* base, uint32_t bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_scene[];
    if (LDS) {
        const uint4* src = reinterpret_cast<const uint4*>(base);
        uint4* dst = reinterpret_cast<uint4*>(s_scene);
        for (uint32_t k = threadIdx.x; k < bytes / 16; k += kBlock) dst[k] = src[k];
        __syncthreads();
    }
    const scene SS = LDS ? lds_scene(S, base, s_scene) : S;
    const uint32_t n = C->n;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t dw = P.depth[i];
        if (dw == 0) continue;
        d3 L;
        uint32_t q;
        const path_in x = load_ray(P, FR, i, dw);
        const uint32_t rng = x.fresh ? FR.rng[x.src] : P.rng[i];
        prof_t pf;
        if (shade_one<M>(SS, J, P, FR, i, x, rng, ht[i], hid[i], L, q, pf)) {
            double* o = J.L + 3 * (size_t)q;
            store_record(o, L.x, L.y, L.z);
            P.depth[i] = 0;
        }
    }
}

// Fused segment: traversal + shading of each live path in one pass over the
// pool (the ray is read once; no hit records go through HBM).  Same results
// as k_intersect followed by k_shade.
#ifdef RTW_SEG_WAVES  // occupancy experiments: cap registers for N waves per SIMD
#define RTW_SEG_ATTR __attribute__((amdgpu_waves_per_eu(RTW_SEG_WAVES)))
#else
#define RTW_SEG_ATTR
#endif
template <int F, int M, bool LDS>
__global__ __launch_bounds__(kBlock) RTW_SEG_ATTR void k_segment(scene S, job_t J, paths_t P, fresh_t FR, ctrs_t* C,
                                                    const char* base, uint32_t bytes) {
    extern __shared__ __attribute__((aligned(16))) char s_scene[];
    __shared__ uint32_t s_cnt[kWaves];
    if (LDS) {
        const uint4* src = reinterpret_cast<const uint4*>(base);
        uint4* dst = reinterpret_cast<uint4*>(s_scene);
        for (uint32_t k = threadIdx.x; k < bytes / 16; k += kBlock) dst[k] = src[k];
        __syncthreads();
    }
    const scene SS = LDS ? lds_scene(S, base, s_scene) : S;
    const uint32_t n = C->n;
    uint32_t live = 0;
    prof_t pf;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t dw = P.depth[i];
        if (dw == 0) continue;
        pf.mark(PS_LOOP);
        const path_in x = load_ray(P, FR, i, dw);
        uint32_t rng = x.fresh ? FR.rng[x.src] : P.rng[i];
        pf.mark(PS_LOAD);
        const hit_state h = world_closest<F>(S, x.r, rng);
        pf.mark(PS_TRAVERSE);
        ++live;
        d3 L;
        uint32_t q;
        if (shade_one<M>(SS, J, P, FR, i, x, rng, h.t, h.prim, L, q, pf)) {
            double* o = J.L + 3 * (size_t)q;
            store_record(o, L.x, L.y, L.z);
            P.depth[i] = 0;
        }
        pf.mark(PS_STORE);
    }
    pf.flush();
    for (int off = 32; off > 0; off >>= 1) live += __shfl_down(live, off, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = live;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < kWaves; ++k) t += s_cnt[k];
        if (t) atomicAdd(&C->segments[blockIdx.x % 8].v, t);
    }
}

// Persistent form: every lane keeps its path in registers and runs it to the
// end, then takes the next camera sample -- one launch per pass, no path
// state through HBM, no regeneration or compaction launches.
//
// Camera rays are made in batches of 64, one per lane (ray-gen never runs
// for just the few lanes whose paths ended this iteration): a wave reserves
// 64 consecutive sample ids of its queue shard with ONE atomic (neighbouring
// ids are neighbouring pixels; other shards are stolen from once its own is
// dry), every lane generates one ray into the wave's LDS buffer, and idle
// lanes pop rays from that buffer.  A wave exits when the queue is exhausted,
// its buffer is empty and its last path has ended.
// Camera samples a wave generates at once into its batch: 64, lane-full ray
// generation.
constexpr int kPBatch = 64;
// PIN (F_PIN): the origins are the camera's, read from the camera where a
// sample is popped instead of stored per entry -- 24 B x 64 per wave less LDS
// (24 KB per 1 024-thread workgroup), which the BVH node packet takes.
template <int NB, bool PIN = false>
struct ray_batch_t {  // one wave's buffer of generated camera samples (LDS)
    double ox[PIN ? 1 : NB], oy[PIN ? 1 : NB], oz[PIN ? 1 : NB];
    double dx[NB], dy[NB], dz[NB], tm[NB];
    uint32_t rng[NB], q[NB];
};

// the camera's origin (F_PIN batches), scalar loads through an opaque
// pointer as in camera_sample
__device__ __forceinline__ d3 camera_origin(const job_t& J) {
    const rtw_camera_desc* cp = J.cam;
    asm volatile("" : "+s"(cp));
    return d3{ld(&cp->origin[0]), ld(&cp->origin[1]), ld(&cp->origin[2])};
}
// (camera_is_pinhole, when F_PIN applies to a render: host/scene_layout.h)

// Occupancy: left alone the compiler gives k_persist 160-230 VGPRs (2-3
// waves per SIMD).  Capping at 128 (4 waves) costs some spilled registers and
// wins: 2 638 -> 2 980 Msamples/s on Cornell (5 waves spilled too much then).
// The scene-specialised list kernels (F_BLACK: Cornell; F_YSPH with the
// Book-1 material set: random_balls) are lean enough for 5 waves (96 VGPRs):
// Cornell +4.5 %, random_balls flat +6.8 %; the BVH and all-feature kernels
// lose 7-24 % at 5 and keep 4.
#ifdef RTW_SEG_WAVES
#define RTW_PERSIST_WAVES(F, M) RTW_SEG_WAVES
#else
#define RTW_PERSIST_WAVES(F, M)                                                                        \
    ((((F) & F_BLACK) && !((F) & (F_MEDIA | F_WBVH | F_GBVH))) || (((F) & F_YSPH) && (M) != SF_ALL) ? 5 : 4)
#endif
// The persistent kernels' one argument.
struct persist_args {
    scene S;
    job_t J;
    ctrs_t* C;
    const char* base;  // the scene allocation; its shading prefix is staged in LDS
    uint32_t bytes;    // bytes of that prefix
    uint32_t lds_nodes;      // BVH node packet: the top nodes staged in LDS (k_persist, LST)
    uint32_t lds_nodes_off;  // its byte offset in the dynamic LDS (after the prefix)
};

// The persistent kernels' argument, re-read from the kernarg segment (scalar
// loads through the scalar cache) by each phase of a loop iteration that
// uses it.  Read once, every scene / job field a persistent loop touches is
// hoisted into registers held across the whole loop -- some 80 SGPRs, far
// past the 106 a wave has, so they spill into VGPR lanes and push the paths'
// own registers out to scratch.  The opaque copy of the segment pointer stops
// that hoisting: each phase loads what it uses and lets it go.
__device__ __forceinline__ const persist_args& args_now() {
    cptr<persist_args> p = (cptr<persist_args>)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const persist_args*)p;
}

// A wave's reservation on the sample queue (rtw_queue.h): the wave takes one
// id of the pass's `total` for each lane of the ballot `takers` (this lane is
// one of them when `takes`), its block's own shard first, then the others in
// turn (a dry shard is skipped without an atomic).  Lane 0 does the atomics
// and broadcasts each base; the takers get the ids of each grant in lane order.
// k_fast and k_fast_sort call this.  k_persist and k_persist_sort spell the
// same loop out (through the function they measured slower,
// profiles/persist_shared/ab_parent_vs_shared.txt): a change to the queue is
// made here, in those two kernels, and in k_regen's block-level form.
struct reservation {
    uint32_t q;  // this lane's sample id (got)
    bool got;    // this lane holds an id
    bool open;   // the wave got all it wanted: the queue may hold more
};
__device__ __forceinline__ reservation reserve_samples(ctrs_t* C, uint32_t total, unsigned long long takers,
                                                       bool takes) {
    const int own = blockIdx.x % kQShards;
    const bool lead = (threadIdx.x & 63) == 0;
    const uint32_t rank = (uint32_t)__popcll(takers & lanemask_lt());
    uint32_t left = (uint32_t)__popcll(takers), given = 0, q = 0;
    bool got = false;
    for (int a = 0; a < kQShards && left; ++a) {
        const int sh = (own + a) % kQShards;
        const unsigned long long lim = shard_limit(sh, total);
        unsigned long long b = ~0ull;
        if (lead) {
            const bool dry = a > 0 && __hip_atomic_load(&C->qshard[sh].v, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT) >= lim;
            if (!dry) b = atomicAdd(&C->qshard[sh].v, (unsigned long long)left);
        }
        b = __shfl(b, 0, 64);
        if (b == ~0ull || b >= lim) continue;
        const uint32_t ok = (uint32_t)min((unsigned long long)left, lim - b);
        if (takes && rank >= given && rank < given + ok) {
            q = (uint32_t)shard_sample(sh, b + (rank - given));
            got = true;
        }
        given += ok;
        left -= ok;
    }
    return reservation{q, got, left == 0};
}

// LST: BVH traversal stacks in LDS (one column per lane) instead of scratch.
// The loop-carried ray stays in registers: every form that parked it in LDS
// (the whole ray with lane-direct camera samples, or its origin beside
// smaller batches) took that LDS from the node packet or the batches and
// measured slower than the spills it removed (EXPERIMENTS.md).
template <int F, int M, bool LDS, bool LST = false>
__global__ __launch_bounds__(kPBlock) __attribute__((amdgpu_waves_per_eu(RTW_PERSIST_WAVES(F, M))))
void k_persist(persist_args) {
    constexpr int NB = kPBatch;
    constexpr bool PIN = (F & F_PIN) != 0;
    extern __shared__ __attribute__((aligned(16))) char s_scene[];
    __shared__ uint32_t s_cnt[kPWaves];
    __shared__ ray_batch_t<NB, PIN> s_batch[kPWaves];
    __shared__ double s_thr[3][kPBlock];  // each lane's path throughput
    __shared__ uint16_t s_stack[LST ? kLdsStack : 1][kPBlock];
    __shared__ uint32_t s_q[kPBlock];     // each lane's sample id
    if (LDS) {
        const persist_args& A = args_now();
        stage_lds(s_scene, A.base, A.bytes / 16, kPBlock);
    }
    if (LST) {  // the BVH node packet (the top levels of every tree)
        const persist_args& A = args_now();
        constexpr uint32_t kNode16 = (uint32_t)(sizeof(node_store) / 16);
        stage_lds(s_scene + A.lds_nodes_off, A.S.nodes, A.lds_nodes * kNode16, kPBlock);
    }
    if (LDS || LST) __syncthreads();
    const int own = blockIdx.x % kQShards;
    path_st x;
    x.depth = 0;
    bool open = true;      // wave-uniform: the queue may still hold samples
    uint32_t bl = 0, bh = 0;  // wave-uniform: unread batch entries [bl, bh)
    uint32_t segs = 0;
    prof_t pf;
    for (;;) {
        // lane-dependent LDS addresses (batch, throughput, sample id, stack
        // columns) are formed from an opaque copy of the thread index where
        // they are used: left to itself the compiler hoists one VGPR per
        // array out of the loop (C5's kernel: 65 of them)
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const uint32_t ln = tid & 63;
        {
            // (the wave's batch too: formed once per kernel, its per-array
            // addresses were held in 15 VGPRs across the whole loop)
            ray_batch_t<NB, PIN>& B = s_batch[tid >> 6];
            for (int round = 0; round < 2; ++round) {
                const unsigned long long m = __ballot(x.depth == 0);
                if (!m) break;
                if (bl == bh) {
                    if (!open) break;
                    const persist_args& A = args_now();
                    const job_t& J = A.J;
                    ctrs_t* const C = A.C;
                    // reserve up to NB ids, own shard first: reserve_samples' loop spelt out
                    // with rank = lane and every lane eligible (see there: a change to the
                    // queue is made in every copy)
                    uint32_t left = NB, given = 0, q = 0;
                    bool got = false;
                    for (int a = 0; a < kQShards && left; ++a) {
                        const int sh = (own + a) % kQShards;
                        const unsigned long long lim = shard_limit(sh, J.total);
                        unsigned long long b = ~0ull;
                        if (ln == 0) {
                            const bool dry = a > 0 && __hip_atomic_load(&C->qshard[sh].v, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_AGENT) >= lim;
                            if (!dry) b = atomicAdd(&C->qshard[sh].v, (unsigned long long)left);
                        }
                        b = __shfl(b, 0, 64);
                        if (b == ~0ull || b >= lim) continue;
                        const uint32_t ok = (uint32_t)min((unsigned long long)left, lim - b);
                        if (ln >= given && ln < given + ok) {
                            q = (uint32_t)shard_sample(sh, b + (ln - given));
                            got = true;
                        }
                        given += ok;
                        left -= ok;
                    }
                    if (left) open = false;
                    if (got) {  // (lanes >= NB get no id)
                        uint32_t rng;
                        const ray r = fresh_sample<F, false>(J, q, rng);
                        if constexpr (!PIN) B.ox[ln] = r.o.x, B.oy[ln] = r.o.y, B.oz[ln] = r.o.z;
                        B.dx[ln] = r.d.x, B.dy[ln] = r.d.y, B.dz[ln] = r.d.z;
                        B.tm[ln] = r.t;
                        B.rng[ln] = rng;
                        B.q[ln] = q;
                    }
                    bl = 0;
                    bh = given;
                    if (!bh) break;
                    __builtin_amdgcn_wave_barrier();
                }
                const uint32_t rank = (uint32_t)__popcll(m & lanemask_lt());
                const uint32_t avail = bh - bl;
                if (x.depth == 0 && rank < avail) {
                    const uint32_t k = bl + rank;
                    const d3 o = PIN ? camera_origin(args_now().J) : d3{B.ox[k], B.oy[k], B.oz[k]};
                    x.r = ray{o, d3{B.dx[k], B.dy[k], B.dz[k]}, B.tm[k]};
                    x.rng = B.rng[k];
                    s_q[tid] = B.q[k];
                    s_thr[0][tid] = 1.0, s_thr[1][tid] = 1.0, s_thr[2][tid] = 1.0;
                    x.depth = (uint32_t)args_now().J.max_depth;
                }
                bl += min((uint32_t)__popcll(m), avail);
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (!__any(x.depth != 0)) break;
        pf.mark(PS_LOAD);
        if (x.depth != 0) {
            const persist_args& A = args_now();
            scene S = A.S;
            hit_state h;
            if constexpr (LST) {
                S.lnodes = reinterpret_cast<const node_store*>(s_scene + A.lds_nodes_off);
                S.n_lnodes = (int32_t)A.lds_nodes;
                lds_stack stk{&s_stack[0][tid]};
                h = world_closest<F>(S, x.r, x.rng, stk);
            } else {
                h = world_closest<F>(S, x.r, x.rng);
            }
            pf.mark(PS_TRAVERSE);
            ++segs;
            const persist_args& A2 = args_now();
            const scene SS = LDS ? lds_scene(A2.S, A2.base, s_scene) : A2.S;
#ifdef RTW_PROF
            pf.classify(h.prim == -1 ? 0
                        : 1 + SS.materials[h.prim <= -2 ? SS.entries[-h.prim - 2].phase_material
                                                        : SS.prims[h.prim].material].type);
#endif
            // the outcome is applied inside the branch that produced it
            uint32_t me = tid;
            auto radiance = [&](const d3& L) {
                double* o = A2.J.L + 3 * (size_t)s_q[me];
                store_record(o, L.x, L.y, L.z);
            };
            ray nr;
#if RTW_STRICT_RADIANCE
            // the path's factors in its thread's log, folded inside-out at its
            // end: c = E, then c = (m_k * c) / pdf_k for k = last .. 0 -- the
            // returns of the recursive color() (RayTracingWeekend.cpp:107,
            // 129-132; emitted of a scattering material is 0 and 0 + c == c),
            // specular bounces logged with pdf 1 (x / 1 == x)
            const uint32_t kb = (uint32_t)A2.J.max_depth - x.depth;  // this segment's bounce
            const size_t gth = (size_t)blockIdx.x * kPBlock + tid;
            double* const flog = A2.J.flog;
            const size_t nth = A2.J.flog_threads;
            auto log_factor = [&](const d3& m, double pdf, const ray& r) {
                double* e = flog + 4 * ((size_t)kb * nth + gth);
                e[0] = m.x, e[1] = m.y, e[2] = m.z, e[3] = pdf;
                nr = r;
            };
            auto fold = [&](d3 c) {
                for (int k = (int)kb - 1; k >= 0; --k) {
                    const double* e = flog + 4 * ((size_t)k * nth + gth);
                    c = (d3{e[0], e[1], e[2]} * c) / e[3];
                }
                radiance(c);
            };
            auto sk = make_sink4([&](const d3& f, const ray& r) { log_factor(f, 1.0, r); },
                                 [&](const d3& m, double pdf, const ray& r) { log_factor(m, pdf, r); },
                                 [&](const d3& E) { fold(E); }, [&]() { fold(d3{0.0, 0.0, 0.0}); });
#else
            auto sk = make_sink(
                [&](const d3& f, const ray& r) {
                    s_thr[0][me] *= f.x, s_thr[1][me] *= f.y, s_thr[2][me] *= f.z;
                    nr = r;
                },
                [&](const d3& E) { radiance(d3{s_thr[0][me], s_thr[1][me], s_thr[2][me]} * E); },
                [&]() {
                    // thr * 0, not 0: the reference multiplies its factors into
                    // the 0 color() returns, so a non-finite throughput gives NaN
                    const double z = in_place<0>();
                    radiance(d3{s_thr[0][me], s_thr[1][me], s_thr[2][me]} * z);
                });
#endif
            const int out = shade_core<M, (F & F_STATIC) != 0, (F & F_LIGHTS) != 0, (F & F_BLACK) != 0,
                                       (F & F_NOLIGHTS) != 0>(SS, x, h.t, h.prim, sk, pf);
            if (out != SEG_CONTINUE)
                x.depth = 0;
            else
                x.r = nr;
            pf.mark(PS_STORE);
        }
    }
    pf.flush();
    count_segments<kPWaves>(segs, s_cnt, [] { return args_now().C; });
}

// Persistent form with material regrouping.  A wave pays for every shading
// branch one of its lanes takes; on Cornell about half the lanes shade
// lambertian, 30 % dielectric, 20 % emit or miss, and every wave carries all
// of them.  Here, after each traversal, the block's 256 paths are sorted by
// what their hit needs (lambertian, dielectric, metal, isotropic, emitter,
// miss, idle) with a counting sort over wave ballots and moved through LDS
// to the lane of their rank, so most waves run one branch.  Idle lanes end
// up together at the top of the block: they take fresh camera samples
// there, so ray generation also runs nearly lane-full.
// The keys' order is the order of the sorted block: material order, the
// path-ending keys (emitter, miss) last.  The paths that end are the lanes
// that take camera samples next: they sit together at the block's top,
// beside the idle ones, so ray generation runs lane-full in one or two waves.
// (Cheap keys between the expensive ones measured T -7 %, and sorting
// lambertian hits on their mixture choice T -1 %: EXPERIMENTS.md.)
enum { K_LAMB = 0, K_DIEL, K_METAL, K_ISO, K_EMIT, K_MISS, K_IDLE, K_N };

// Ray generation threshold: a wave takes camera samples only when at least
// this many of its lanes are idle.  After shading a few lambertian paths per
// wave end (pdf <= 0, depth), and a wave would run a whole camera_sample
// (~150 VALU) for one to three lanes; with fewer than K idle lanes the slots
// wait one iteration, are sorted to the block's top with the other idle
// records (K_IDLE) and refill there, lane-full.  A block always ends with
// every wave fully idle, so the queue still drains.  Measured (1 MI355X,
// A/B, profiles/r03/ab_refill_min.log): K = 8 T +0.45 %, C2 +0.8 %; K = 24
// T +0.2 %, C2 -0.7 %.
#ifndef RTW_REFILL_MIN
#define RTW_REFILL_MIN 8
#endif
// Paths regrouped together (one workgroup).  (128 or 512 measured T -15 % /
// -13 %, EXPERIMENTS.md.)
constexpr int kSortBlock = 256;
constexpr int kSortWaves = kSortBlock / 64;
// The counting sort's block prefix from a key-major
// count table s_kc[key][wave] (kKeySlots x 4; slots of keys the scene cannot
// produce stay zero): lane k < 8 of every wave reads key k's four per-wave
// counts in one 16-B LDS read and forms their total and the count in the
// waves before its own; an exclusive scan of the totals over lanes 0..7
// (three DPP row shifts) adds the paths of every key before k; each lane
// fetches its own key's base with one ds_bpermute.  The plain form has every
// lane read all 4 x K_N counts and sum them under selects (~67 VALU per
// wave-iteration on T); measured T +3.0 %, T fp32 +4.8 %
// (profiles/r05/ab_r5l_sort_dpp.log).
constexpr int kKeySlots = 8;
__device__ __forceinline__ uint32_t sort_base_dpp(const uint32_t (*s_kc)[4], uint32_t lane, uint32_t wave, int key,
                                                  int k_idle, uint32_t& idle_total) {
    const uint4 c = *reinterpret_cast<const uint4*>(s_kc[lane & (kKeySlots - 1)]);
    const uint32_t tot = c.x + c.y + c.z + c.w;
    const uint32_t before = (wave > 0 ? c.x : 0u) + (wave > 1 ? c.y : 0u) + (wave > 2 ? c.z : 0u);
    uint32_t incl = tot;  // inclusive scan over lanes 0..7 (row_shr:1, 2, 4; lanes without a source add 0)
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, true);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, true);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, true);
    const uint32_t base = incl - tot + before;
    idle_total = (uint32_t)__builtin_amdgcn_readlane((int)tot, k_idle);
    return (uint32_t)__builtin_amdgcn_ds_bpermute(key << 2, (int)base);
}
static_assert(kSortWaves == 4 && K_N <= kKeySlots && rtwf::FK_N <= kKeySlots,
              "sort_base_dpp: 256-thread sort blocks, at most 8 keys");
// Step 3 of the regrouping kernels, the counting sort of the block's paths
// by key: per key, the wave's ballot gives the lane's rank among its wave's
// lanes of that key and, into s_kc, their count; after the barrier
// sort_base_dpp adds the slots before them.  Returns the slot of this lane's
// record in the sorted block.  Keys the kernel cannot produce (`used` false)
// are skipped: their counts stay 0 (s_kc's slots start zeroed, the prefix
// reads them).
template <int NKEYS, class Used>
__device__ __forceinline__ uint32_t sort_slot(uint32_t (*s_kc)[kSortWaves], uint32_t lane, uint32_t wave, int key,
                                              int k_idle, Used used, uint32_t& idle_total) {
    uint32_t rank_in_wave = 0;
#pragma unroll
    for (int k = 0; k < NKEYS; ++k) {
        if (!used(k)) continue;
        const unsigned long long m = __ballot(key == k);
        if (key == k) rank_in_wave = (uint32_t)__popcll(m & lanemask_lt());
        if (lane == 0) s_kc[k][wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    return rank_in_wave + sort_base_dpp(s_kc, lane, wave, key, k_idle, idle_total);
}

// The regrouping kernels' exchange (LDS, SoA): one path record per slot, in
// the kernel's scalar T (double: k_persist_sort, float: k_fast_sort).
// Between iterations a lane's path record sits in its own exchange slot
// (ray, home index, sample id at [tid]); only the engine and the depth
// are loop-carried registers.  A loop-carried ray would hold 12 VGPRs
// through every shading branch (exec-masked branches run one after the
// other, so a value live into any of them is live across all) -- that
// is what pushed k_persist_sort past 96 VGPRs into scratch.
// Path throughputs stay put: each path record (live or idle) owns one
// home slot of thr and carries its index through the exchange, so the
// throughput is read and written only where shading uses it and is never
// held in registers across traversal and sort.  A lane whose path ended
// keeps the record's slot for the camera sample it takes next.
template <typename T>
struct exch_types;
template <>
struct exch_types<double> {
    using vec_t = d3;
    using ray_t = ray;
};
template <>
struct exch_types<float> {
    using vec_t = rtwf::f3;
    using ray_t = rtwf::fray;
};
// The arrays are static members, LDS variables of their own as the kernels'
// other __shared__ arrays are (one set per T and TIME, allocated in every
// kernel that uses them; the time array of a TIME false exchange is never
// referenced and takes no LDS).  TIME false -- F_STATIC scenes -- keeps no
// ray times: they are never read.
template <typename T, bool TIME = true>
struct exchange_t {
    using vec_t = typename exch_types<T>::vec_t;
    using ray_t = typename exch_types<T>::ray_t;
    inline static __shared__ T o[3][kSortBlock], d[3][kSortBlock], tm[kSortBlock], t[kSortBlock];
    inline static __shared__ int32_t prim[kSortBlock];
    inline static __shared__ uint32_t rng[kSortBlock], depth[kSortBlock], q[kSortBlock], home[kSortBlock];
    inline static __shared__ T thr[3][kSortBlock];  // the home slots
    // the record's ray in slot `s`
    __device__ __forceinline__ ray_t ray_at(uint32_t s) const {
        return ray_t{vec_t{o[0][s], o[1][s], o[2][s]}, vec_t{d[0][s], d[1][s], d[2][s]}, TIME ? tm[s] : T(0)};
    }
    // (origin and direction alone: a continuation ray whose time the slot holds already)
    __device__ __forceinline__ void put_ray_od(uint32_t s, const ray_t& r) const {
        o[0][s] = r.o.x, o[1][s] = r.o.y, o[2][s] = r.o.z;
        d[0][s] = r.d.x, d[1][s] = r.d.y, d[2][s] = r.d.z;
    }
    __device__ __forceinline__ void put_ray(uint32_t s, const ray_t& r) const {
        put_ray_od(s, r);
        if constexpr (TIME) tm[s] = r.t;
    }
    // Step 4: this lane's record to slot `dst` (an idle record's ray is
    // garbage and stays behind).  Its home and sample id were read from the
    // lane's own slot before the barrier that precedes these writes.
    __device__ __forceinline__ void move_to(uint32_t dst, const ray_t& r, T hit_t, int32_t hit_prim, uint32_t rng_,
                                            uint32_t depth_, uint32_t home_, uint32_t q_) const {
        if (depth_ != 0) put_ray(dst, r);
        home[dst] = home_;
        t[dst] = hit_t;
        prim[dst] = hit_prim;
        rng[dst] = rng_;
        depth[dst] = depth_;
        q[dst] = q_;
    }
};

template <int F, int M, bool LDS>
__global__ __launch_bounds__(kSortBlock) __attribute__((amdgpu_waves_per_eu(RTW_PERSIST_WAVES(F, M))))
void k_persist_sort(persist_args) {
    extern __shared__ __attribute__((aligned(16))) char s_scene[];
    __shared__ __attribute__((aligned(16))) uint32_t s_kc[kKeySlots][kSortWaves];  // per key, lanes per wave
    if (threadIdx.x < kKeySlots * kSortWaves) (&s_kc[0][0])[threadIdx.x] = 0u;  // (before the barrier below)
    __shared__ uint32_t s_seg[kSortWaves];
    const exchange_t<double, !(F & F_STATIC)> X;  // (F_STATIC: the time is never read)
    X.home[threadIdx.x] = threadIdx.x;
    if (LDS) {
        const persist_args& A = args_now();
        stage_lds(s_scene, A.base, A.bytes / 16, kSortBlock);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int own = blockIdx.x % kQShards;
    path_st x;
    x.depth = 0;
    bool open = true;  // wave-uniform: the queue may still hold samples
    uint32_t segs = 0;
    prof_t pk;  // section profiler (RTW_PROF builds): refill, traverse, sort, exchange, shade
    for (;;) {
        // 1. idle lanes take new camera samples (one reservation per wave)
        {
            const bool idle = x.depth == 0;
            const unsigned long long m = __ballot(idle);
            if (open && __popcll(m) >= RTW_REFILL_MIN) {
                // reserve_samples' loop spelt out, as in k_persist (see there: a change
                // to the queue is made in every copy)
                const persist_args& A = args_now();
                const job_t& J = A.J;
                ctrs_t* const C = A.C;
                const uint32_t want = (uint32_t)__popcll(m);
                const uint32_t rank = (uint32_t)__popcll(m & lanemask_lt());
                uint32_t left = want, given = 0, q = 0;
                bool got = false;
                for (int a = 0; a < kQShards && left; ++a) {
                    const int sh = (own + a) % kQShards;
                    const unsigned long long lim = shard_limit(sh, J.total);
                    unsigned long long b = ~0ull;
                    if (lane == 0) {
                        const bool dry = a > 0 && __hip_atomic_load(&C->qshard[sh].v, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT) >= lim;
                        if (!dry) b = atomicAdd(&C->qshard[sh].v, (unsigned long long)left);
                    }
                    b = __shfl(b, 0, 64);
                    if (b == ~0ull || b >= lim) continue;
                    const uint32_t ok = (uint32_t)min((unsigned long long)left, lim - b);
                    if (idle && rank >= given && rank < given + ok) {
                        q = (uint32_t)shard_sample(sh, b + (rank - given));
                        got = true;
                    }
                    given += ok;
                    left -= ok;
                }
                if (left) open = false;
                if (got) {
                    const ray r = fresh_sample<F, true>(J, q, x.rng);
                    const uint32_t me = threadIdx.x;
                    const uint32_t home = X.home[me];
                    X.put_ray(me, r);
                    X.q[me] = q;
                    x.depth = (uint32_t)J.max_depth;
                    X.thr[0][home] = 1.0, X.thr[1][home] = 1.0, X.thr[2][home] = 1.0;
                }
            }
        }
        pk.mark(PS_LOAD);
        // 2. traversal
        double th = 0.0;
        int32_t hp = -1;
        int key = K_IDLE;
        if (x.depth != 0) {
            const uint32_t me = threadIdx.x;
            x.r = X.ray_at(me);
            const persist_args& A = args_now();
            const scene SS = LDS ? lds_scene(A.S, A.base, s_scene) : A.S;
            const hit_state h = world_closest<F>(A.S, x.r, x.rng);
            ++segs;
            th = h.t;
            hp = h.prim;
            if (hp == -1) {
                key = K_MISS;
            } else {
                const int mat = hp <= -2 ? SS.entries[-hp - 2].phase_material : SS.prims[hp].material;
                const int ty = SS.materials[mat].type;
                key = ty == RTW_MAT_LAMBERTIAN ? K_LAMB
                      : ty == RTW_MAT_DIELECTRIC ? K_DIEL
                      : ty == RTW_MAT_METAL ? K_METAL
                      : ty == RTW_MAT_ISOTROPIC ? K_ISO
                                                : K_EMIT;
            }
        }
        pk.mark(PS_TRAVERSE);
        // 3. counting sort of the block's paths by key (the record's home and
        // sample id are read from the lane's own slot before the barrier that
        // precedes the exchange's writes)
        const uint32_t my_home = X.home[threadIdx.x], my_q = X.q[threadIdx.x];
        // (keys the scene's material set cannot produce are skipped)
        constexpr auto key_used = [](int k) {
            return !((k == K_METAL && !(M & SF_METAL)) || (k == K_ISO && !(M & SF_ISO)));
        };
        uint32_t idle_total;
        const uint32_t dst = sort_slot<K_N>(s_kc, lane, wave, key, K_IDLE, key_used, idle_total);
        if (idle_total == kSortBlock) break;  // block-uniform: nothing left to trace or take
        pk.mark(PS_HIT);
        // 4. move every path to the slot of its rank
        X.move_to(dst, x.r, th, hp, x.rng, x.depth, my_home, my_q);
        __syncthreads();
        // (opaque, so the exchange's per-lane LDS addresses are formed here
        // from one register, not hoisted out of the loop one per array)
        uint32_t me = threadIdx.x;
        asm volatile("" : "+v"(me));
        x.rng = X.rng[me];
        x.depth = X.depth[me];
        pk.mark(PS_SAMPLE);
        // 5. shading, now mostly one branch per wave
        if (x.depth != 0) {
            x.r = X.ray_at(me);
            const persist_args& A = args_now();
            const scene SS = LDS ? lds_scene(A.S, A.base, s_scene) : A.S;
            prof_t pf;
            // the outcome is applied inside the branch that produced it
            auto radiance = [&](const d3& L) {
                double* o = A.J.L + 3 * (size_t)X.q[me];
                store_record(o, L.x, L.y, L.z);
            };
            auto sk = make_sink(
                [&](const d3& f, const ray& nr) {
                    const uint32_t home = X.home[me];
                    X.thr[0][home] *= f.x, X.thr[1][home] *= f.y, X.thr[2][home] *= f.z;
                    // the continuation ray waits in the lane's own slot
                    X.put_ray(me, nr);
                },
                [&](const d3& E) {
                    const uint32_t home = X.home[me];
                    radiance(d3{X.thr[0][home], X.thr[1][home], X.thr[2][home]} * E);
                },
                [&]() {
                    // thr * 0 (k_persist's reason: NaN / inf throughputs give NaN)
                    const uint32_t home = X.home[me];
                    const double z = in_place<0>();
                    radiance(d3{X.thr[0][home], X.thr[1][home], X.thr[2][home]} * z);
                });
            const int out = shade_core<M, (F & F_STATIC) != 0, (F & F_LIGHTS) != 0, (F & F_BLACK) != 0,
                                       (F & F_NOLIGHTS) != 0>(SS, x, X.t[me], X.prim[me], sk, pf);
            if (out != SEG_CONTINUE) x.depth = 0;
        }
        pk.mark(PS_STORE);
    }
    pk.flush();
    count_segments<kSortWaves>(segs, s_seg, [] { return args_now().C; });
}

// ----------------------------------------------------------------------
// fp32 fast mode (RTW_PRECISION_FP32, rtw_fast.h): the persistent form with
// every lane's path in registers -- ray, throughput, engine, depth, sample
// id -- and camera samples taken by idle lanes (one queue reservation per
// wave).  Waves run independently (no block barrier in the loop), so a wave
// leaves as soon as the queue is dry and its last path has ended.
// The fast mode's per-sample radiance record: 12 B of fp32 (k_reduce<float>
// sums it in double in sample order, as it sums fp64 records).
__device__ __forceinline__ void store_record_f32(double* L, uint32_t q, float x, float y, float z) {
    float* o = reinterpret_cast<float*>(L) + 3 * (size_t)q;
    store_record(o, x, y, z);
}

struct fast_args {
    rtwf::fscene S;
    job_t J;
    ctrs_t* C;
    rtwf::cam32 cam;
    uint32_t lds_nodes;  // k_fast<.., LST>: BVH node packet (the top nodes) in dynamic LDS
    // k_fast_sort<.., LDS>: each fscene array's byte offset in the LDS copy of
    // the shading prefix, ~0u for one outside it (host-computed: a range test of
    // every pointer at every use, two 64-bit compares, becomes one 32-bit test)
    uint32_t lds_off[9];
};

// fast_args re-read from the kernarg segment by each phase that uses it
// (args_now's reason: hoisted whole, the scene and job fields fill the
// SGPRs and spill into VGPR lanes)
__device__ __forceinline__ const fast_args& fast_args_now() {
    cptr<fast_args> p = (cptr<fast_args>)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const fast_args*)p;
}

// Waves per SIMD of k_fast.  With the node packet, 8 waves in two
// 1 024-thread workgroups per CU (each with a ~48 KB packet) beat 6 waves in
// two 768-thread ones (~56 KB packets, no spills) although the kernel then
// spills ~17 VGPRs: C3 fp32 4 710 vs 4 386, C5 fp32 806 vs 728 Msamples/s;
// one 1 024-thread workgroup at 6 waves (16 waves per CU) 3 350 / 536; 384
// threads at 6 waves 3 602 / 556; no packet at 6 waves (round 3 before it)
// 3 553 / 645 (1 MI355X, A/B, profiles/r03/ab_fp32_packet.log).
#ifndef RTW_FAST_BVH_WAVES
#define RTW_FAST_BVH_WAVES 8
#endif
// The path -- ray, throughput, engine, depth, sample id -- is in registers.
// (Throughput and sample id in LDS home slots halve the media kernel's spill
// stores but take a third of its node packet: -1 %, EXPERIMENTS.md.)
template <int F, bool LST>
__global__ __launch_bounds__(rtwf::fast_block(F)) __attribute__((amdgpu_waves_per_eu(RTW_FAST_BVH_WAVES)))
void k_fast(fast_args) {
    using namespace rtwf;
    constexpr bool NOISE = (F & FF_NONOISE) == 0;
    constexpr bool IMAGE = (F & FF_IMAGE) != 0;
    constexpr int kFB = fast_block(F);
    constexpr int kFW = kFB / 64;
    extern __shared__ __attribute__((aligned(16))) char s_nodes[];
    __shared__ uint16_t s_stack[LST ? fast_stack(F) : 1][kFB];
    __shared__ uint32_t s_cnt[kFW];
    if (LST) {  // the BVH node packet (the top levels of every tree)
        const fast_args& A = fast_args_now();
        stage_lds(s_nodes, A.S.nodes, A.lds_nodes * (uint32_t)(sizeof(node_store) / 16), kFB);
        __syncthreads();
    }
    fray r{f3{0, 0, 0}, f3{0, 0, 1}, 0};
    f3 thr{1, 1, 1};
    uint32_t rng = 0, depth = 0, q = 0, segs = 0;
    bool open = true;  // wave-uniform: the queue may still hold samples
    for (;;) {
        // idle lanes take new camera samples (RayTracingWeekend.cpp:227-231)
        const bool idle = depth == 0;
        const unsigned long long m = __ballot(idle);
        if (open && m) {
            const fast_args& A = fast_args_now();
            const reservation rs = reserve_samples(A.C, A.J.total, m, idle);
            open = rs.open;
            if (rs.got) {
                r = camera_sample_f32<(F & F_ACTIVE) != 0>(A.J, A.cam, rs.q, rng);
                thr = f3{1, 1, 1};
                q = rs.q;
                depth = (uint32_t)A.J.max_depth;
            }
        }
        if (!__any(depth != 0)) break;
        if (depth == 0) continue;
        fhit h;
        if constexpr (LST) {
            lds_stackf_t<kFB, fast_stack(F)> stk{&s_stack[0][threadIdx.x]};
            const fast_args& A = fast_args_now();
            fscene S = A.S;
            S.lnodes = reinterpret_cast<const node_store*>(s_nodes);
            S.n_lnodes = (int32_t)A.lds_nodes;
            h = world_closest<F>(S, r, rng, stk);
        } else {
            priv_stackf stk;
            h = world_closest<F>(fast_args_now().S, r, rng, stk);
        }
        ++segs;
        // one segment of color() (RayTracingWeekend.cpp:52-159)
        const seg_f sg = shade<NOISE, IMAGE>(fast_args_now().S, r, h, rng, depth);
        bool end = !sg.cont;
        f3 L{0, 0, 0};
        if (sg.cont) {
            thr = thr * sg.w;
            r = sg.next;
            --depth;
        } else {
            L = thr * sg.w;
        }
        if (end) {
            store_record_f32(fast_args_now().J.L, q, L.x, L.y, L.z);
            depth = 0;
        }
    }
    count_segments<kFW>(segs, s_cnt, [] { return fast_args_now().C; });
}

// k_fast_sort re-points its scene with the host's offsets
// (fast_args::lds_off) instead of range-testing every pointer at every use --
// two 64-bit compares, a subtract and selects per pointer, twice per
// iteration, on the scalar unit, which the fp32 kernel's issue shares with
// ~840 VALU per wave-segment (~680 SALU).  Measured (1 MI355X, A/B,
// profiles/r05/ab_r5t_fast_lds_off.log; bit-identical, parity_r5t.log):
// T fp32 8 654 vs 8 075 Msamples/s (+7.2 %), T fp64 +-0.  (The same offsets
// for k_persist_sort's lds_scene, whose rebase has no range test, added
// SALU and VALU there: not used.)
__device__ __forceinline__ rtwf::fscene lds_fscene_off(const rtwf::fscene& S, const uint32_t* off, const char* lds) {
    rtwf::fscene L = S;
    auto rb = [&](const void* p, uint32_t o) -> const void* { return o != ~0u ? (const void*)(lds + o) : p; };
    L.prims = (const rtwf::prim32*)rb(S.prims, off[0]);
    L.entries = (const rtwf::ent32*)rb(S.entries, off[1]);
    L.ops = (const rtwf::op32*)rb(S.ops, off[2]);
    L.materials = (const rtwf::mat32*)rb(S.materials, off[3]);
    L.textures = (const rtwf::tex32*)rb(S.textures, off[4]);
    L.lights = (const rtw_light*)rb(S.lights, off[5]);
    L.ranvec = (const float*)rb(S.ranvec, off[6]);
    L.perm = (const int32_t*)rb(S.perm, off[7]);
    L.frames = (const float*)rb(S.frames, off[8]);
    return L;
}

// fp32 fast mode with material regrouping (list scenes, as k_persist_sort
// for fp64): after each traversal the block's 256 paths are counting-sorted
// by what their hit needs and moved through LDS to the lane of their rank,
// so most waves run one shading branch; idle lanes gather at the top and take
// camera samples there.  Paths wait between iterations in their lane's LDS
// slot; throughputs stay in home slots.  LDS: the fp32 scene (when it fits)
// for shading, traversal reads the scene through the scalar cache.
#ifndef RTW_FAST_WAVES
#define RTW_FAST_WAVES 7  // T fp32: 5 601 (4 waves), 6 465 (5), 7 000 (6), 7 136 (7), 6 462 (8): profiles/r03/ab_fp32_sort_waves.log, ab_fp32_sort_waves7.log
#endif
template <int F, bool LDS>
__global__ __launch_bounds__(kSortBlock) __attribute__((amdgpu_waves_per_eu(RTW_FAST_WAVES)))
void k_fast_sort(fast_args, const char* base, uint32_t bytes) {
    using namespace rtwf;
    constexpr bool NOISE = (F & FF_NONOISE) == 0;
    extern __shared__ __attribute__((aligned(16))) char s_scene[];
    __shared__ __attribute__((aligned(16))) uint32_t s_kc[kKeySlots][kSortWaves];  // per key, lanes per wave
    if (threadIdx.x < kKeySlots * kSortWaves) (&s_kc[0][0])[threadIdx.x] = 0u;  // (before the barrier below)
    __shared__ uint32_t s_seg[kSortWaves];
    const exchange_t<float> X;
    X.home[threadIdx.x] = threadIdx.x;
    if (LDS) stage_lds(s_scene, base, bytes / 16, kSortBlock);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t rng = 0, depth = 0, segs = 0;
    bool open = true;  // wave-uniform: the queue may still hold samples
    for (;;) {
        const uint32_t me = threadIdx.x;
        // 1. idle lanes take new camera samples (one reservation per wave)
        {
            const bool idle = depth == 0;
            const unsigned long long m = __ballot(idle);
            if (open && m) {
                const fast_args& A = fast_args_now();
                const reservation rs = reserve_samples(A.C, A.J.total, m, idle);
                const uint32_t q = rs.q;
                open = rs.open;
                if (rs.got) {
                    const fray r = camera_sample_f32<(F & F_ACTIVE) != 0>(A.J, A.cam, q, rng);
                    X.put_ray(me, r);
                    X.q[me] = q;
                    depth = (uint32_t)A.J.max_depth;
                    const uint32_t home = X.home[me];
                    X.thr[0][home] = 1.0f, X.thr[1][home] = 1.0f, X.thr[2][home] = 1.0f;
                }
            }
        }
        // 2. traversal
        fhit h{0.0f, -1, false};
        int key = FK_IDLE;
        fray r;
        if (depth != 0) {
            r = X.ray_at(me);
            priv_stackf stk;
            h = world_closest<F>(fast_args_now().S, r, rng, stk);
            ++segs;
            const fast_args& A = fast_args_now();
            key = hit_key(LDS ? lds_fscene_off(A.S, A.lds_off, s_scene) : A.S, h);
        }
        // 3. counting sort of the block's paths by key
        const uint32_t my_home = X.home[me], my_q = X.q[me];
        uint32_t idle_total;
        const uint32_t dst = sort_slot<FK_N>(s_kc, lane, wave, key, FK_IDLE, [](int) { return true; }, idle_total);
        if (idle_total == kSortBlock) break;  // block-uniform: nothing left to trace or take
        // 4. move every path to the slot of its rank
        X.move_to(dst, r, h.t, h.prim, rng, depth, my_home, my_q);
        __syncthreads();
        rng = X.rng[me];
        depth = X.depth[me];
        // 5. shading, now mostly one branch per wave
        if (depth != 0) {
            const fray rr = X.ray_at(me);
            const fhit hh{X.t[me], X.prim[me], false};
            const fast_args& A = fast_args_now();
            const seg_f sg = shade<NOISE>(LDS ? lds_fscene_off(A.S, A.lds_off, s_scene) : A.S, rr, hh, rng, depth);
            const uint32_t home = X.home[me];
            const f3 thr{X.thr[0][home], X.thr[1][home], X.thr[2][home]};
            if (sg.cont) {
                X.thr[0][home] = thr.x * sg.w.x, X.thr[1][home] = thr.y * sg.w.y, X.thr[2][home] = thr.z * sg.w.z;
                X.put_ray_od(me, sg.next);  // the continuation ray waits in the lane's own slot
                --depth;
            } else {
                store_record_f32(A.J.L, X.q[me], thr.x * sg.w.x, thr.y * sg.w.y, thr.z * sg.w.z);
                depth = 0;
            }
        }
    }
    count_segments<kSortWaves>(segs, s_seg, [] { return fast_args_now().C; });
}

// Block-wide exclusive prefix sum of one value per thread (blockDim = kBlock).
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += y;
    }
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const uint32_t c = s_wave[k];
        before += (k < (int)w) ? c : 0u;
        tot += c;
    }
    total = tot;
    return before + incl - v;
}

// Refill empty pool slots with new camera samples.  Block b owns the slot
// range [lo, lo + kRegenSlots): its empty slots are ranked with a block prefix
// sum into an LDS list (stream compaction), ONE atomic on queue shard
// b % kQShards reserves that many sample ids, ray-gen runs densely over the
// list and writes the rays DENSELY to staging entries lo, lo+1, ...; each empty
// slot only receives its 4-byte fresh marker.  (Scattered 8-byte stores into
// pool lines that have left L2 cost a memory-side read-modify-write each:
// measured 52 us vs 5 us per launch for 13 scattered arrays vs 3.)
constexpr uint32_t kRegenSlots = 1024;

template <bool ACTIVE, bool RAYS = false>
__device__ __forceinline__ void regen_block(const job_t& J, const paths_t& P, const fresh_t& FR, ctrs_t* C) {
    __shared__ uint32_t s_wave[kWaves];
    __shared__ uint32_t s_list[kRegenSlots];
    const uint32_t n = C->n;
    const uint32_t lo = blockIdx.x * kRegenSlots;
    if (lo >= n) return;
    const uint32_t hi = min(n, lo + kRegenSlots);
    constexpr int kPer = kRegenSlots / kBlock;
    bool need[kPer];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const uint32_t i = lo + threadIdx.x + k * kBlock;
        need[k] = i < hi && P.depth[i] == 0;
        mine += need[k];
    }
    uint32_t total;
    uint32_t off = block_scan(mine, s_wave, total);
    if (total == 0) return;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (need[k]) s_list[off++] = lo + threadIdx.x + k * kBlock;
    // Reserve sample ids: own shard first, then the others while it is dry,
    // so every shard drains whatever the number of blocks.
    __shared__ uint32_t s_got[kQShards];
    __shared__ unsigned long long s_first[kQShards];
    if (threadIdx.x == 0) {
        uint32_t left = total;
        const int own = blockIdx.x % kQShards;
        for (int a = 0; a < kQShards; ++a) {
            const int sh = (own + a) % kQShards;
            s_got[a] = 0;
            if (left == 0) continue;
            const unsigned long long lim = shard_limit(sh, J.total);
            if (a > 0) {  // stealing: skip dry shards without an atomic
                const unsigned long long cur =
                    __hip_atomic_load(&C->qshard[sh].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur >= lim) continue;
            }
            const unsigned long long b = atomicAdd(&C->qshard[sh].v, (unsigned long long)left);
            const uint32_t ok = b >= lim ? 0u : (uint32_t)min((unsigned long long)left, lim - b);
            s_first[a] = b;
            s_got[a] = ok;
            left -= ok;
        }
    }
    __syncthreads();
    const int own = blockIdx.x % kQShards;
    for (uint32_t e = threadIdx.x; e < total; e += kBlock) {
        uint32_t k = e;
        for (int a = 0; a < kQShards; ++a) {
            if (k < s_got[a]) {
                const int sh = (own + a) % kQShards;
                raygen<ACTIVE, RAYS>(J, FR, lo + e, (uint32_t)shard_sample(sh, s_first[a] + k));
                P.depth[s_list[e]] = kFresh | (lo + e);
                break;
            }
            k -= s_got[a];
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_regen(job_t J, paths_t P, fresh_t FR, ctrs_t* C) {
    regen_block<false>(J, P, FR, C);
}
// ... of an active call (rtw_adaptive.h): the only wavefront kernel that makes
// camera rays, so this one instantiation serves every feature and material set
// with the unchanged k_segment / k_intersect / k_shade
__global__ __launch_bounds__(kBlock) void k_regen_active(job_t J, paths_t P, fresh_t FR, ctrs_t* C) {
    regen_block<true>(J, P, FR, C);
}
#if !RTW_STRICT_RADIANCE
// ... of a radiance query (rtw_radiance.h): fresh paths from the caller's ray
// records (ray_sample), for every feature and material set as k_regen_active
__global__ __launch_bounds__(kBlock) void k_regen_rays(job_t J, paths_t P, fresh_t FR, ctrs_t* C) {
    regen_block<false, true>(J, P, FR, C);
}
// Rays whose time the BVH's boxes do not cover, counted before anything is
// traced (a scene with a BVH and moving spheres: rtw_query.h's rule).
__global__ __launch_bounds__(kBlock) void k_check_ray_times(const rtw_query_ray* __restrict__ rays, uint32_t n,
                                                            double sh0, double sh1, uint32_t* bad) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const double t = rays[k].time;
        if (!(t >= sh0 && t <= sh1)) atomicAdd(bad, 1u);
    }
}
#endif

// Tail-phase stream compaction of live slots (depth != 0) from A into B
// (fresh markers move with their slot; staging is not rewritten in the tail).
__global__ __launch_bounds__(kBlock) void k_compact(paths_t A, paths_t B, ctrs_t* C) {
    __shared__ uint32_t s_wave[kWaves];
    __shared__ uint32_t s_base;
    const uint32_t n = C->n;
    for (uint32_t b = blockIdx.x * kBlock; b < n; b += gridDim.x * kBlock) {
        const uint32_t i = b + threadIdx.x;
        const bool live = i < n && A.depth[i] != 0;
        uint32_t total;
        const uint32_t rank = block_rank(live, s_wave, total);
        if (total) {
            if (threadIdx.x == 0) s_base = atomicAdd(&C->n_out, total);
            __syncthreads();
            if (live) {
                const uint32_t o = s_base + rank;
                B.ox[o] = A.ox[i], B.oy[o] = A.oy[i], B.oz[o] = A.oz[i];
                B.dx[o] = A.dx[i], B.dy[o] = A.dy[i], B.dz[o] = A.dz[i];
                B.tm[o] = A.tm[i];
                B.tr[o] = A.tr[i], B.tg[o] = A.tg[i], B.tb[o] = A.tb[i];
                B.rng[o] = A.rng[i], B.depth[o] = A.depth[i], B.qid[o] = A.qid[i];
            }
        }
        __syncthreads();
    }
}

__global__ void k_commit(ctrs_t* C) {
    C->n = C->n_out;
    C->n_out = 0;
}

// running[pix] += sample s of pix for s = 0..S-1 in order (RayTracingWeekend.cpp:235-239)
// Records are doubles (fp64 mode) or floats (the fp32 fast mode's radiance
// is single precision: 12 B records, converted exactly to double here and
// summed in the same order, so its sums are unchanged).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_reduce(const T* __restrict__ L, uint32_t npix, uint32_t spp,
                                                   double* __restrict__ run) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        double r = run[3 * p], g = run[3 * p + 1], bl = run[3 * p + 2];
        for (uint32_t s = 0; s < spp; ++s) {
            const T* x = L + 3 * ((size_t)s * npix + p);
            r = r + (double)x[0];
            g = g + (double)x[1];
            bl = bl + (double)x[2];
        }
        run[3 * p] = r, run[3 * p + 1] = g, run[3 * p + 2] = bl;
    }
}
// k_reduce, and in the same read of each record run2[pix] += x*x (one rounded
// product, one rounded add: the library builds with -ffp-contract=off), the
// raw second moment of rtw_noise.h.  Same access pattern as k_reduce (a wave
// reads 64 consecutive records of one sample plane); the records of kAhead
// samples are loaded before the first of them is added, the additions stay
// in sample order.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_reduce_moments(const T* __restrict__ L, uint32_t npix, uint32_t spp,
                                                           double* __restrict__ run, double* __restrict__ run2) {
    constexpr uint32_t kAhead = 4;
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        double r = run[3 * p], g = run[3 * p + 1], bl = run[3 * p + 2];
        double r2 = run2[3 * p], g2 = run2[3 * p + 1], bl2 = run2[3 * p + 2];
        uint32_t s = 0;
        for (; s + kAhead <= spp; s += kAhead) {
            T x[kAhead][3];
#pragma unroll
            for (uint32_t k = 0; k < kAhead; ++k) {
                const T* src = L + 3 * ((size_t)(s + k) * npix + p);
                x[k][0] = src[0], x[k][1] = src[1], x[k][2] = src[2];
            }
#pragma unroll
            for (uint32_t k = 0; k < kAhead; ++k) {
                const double xr = (double)x[k][0], xg = (double)x[k][1], xb = (double)x[k][2];
                r = r + xr, g = g + xg, bl = bl + xb;
                r2 = r2 + xr * xr, g2 = g2 + xg * xg, bl2 = bl2 + xb * xb;
            }
        }
        for (; s < spp; ++s) {
            const T* src = L + 3 * ((size_t)s * npix + p);
            const double xr = (double)src[0], xg = (double)src[1], xb = (double)src[2];
            r = r + xr, g = g + xg, bl = bl + xb;
            r2 = r2 + xr * xr, g2 = g2 + xg * xg, bl2 = bl2 + xb * xb;
        }
        run[3 * p] = r, run[3 * p + 1] = g, run[3 * p + 2] = bl;
        run2[3 * p] = r2, run2[3 * p + 1] = g2, run2[3 * p + 2] = bl2;
    }
}
// k_reduce's grid for npix pixels
unsigned reduce_grid(uint64_t npix) {
    return (unsigned)std::min<uint64_t>((npix + kBlock - 1) / kBlock, 4096);
}

// accum[(j*nx+i)*3+c] += run[(k*nx+i)*3+c], j = row_begin + k*row_step
__global__ __launch_bounds__(kBlock) void k_emit(const double* __restrict__ run, uint32_t npix, int nx, int row_begin,
                                                 int row_step, double* __restrict__ accum) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        const uint32_t k = p / (uint32_t)nx, i = p - k * (uint32_t)nx;
        const size_t o = ((size_t)(row_begin + (int)k * row_step) * nx + i) * 3;
        accum[o] += run[3 * p];
        accum[o + 1] += run[3 * p + 1];
        accum[o + 2] += run[3 * p + 2];
    }
}

// An active call's scatter-add (rtw_adaptive.h): accum[active[k]] += run[k],
// the same for the sums of squares, counts[active[k]] += spp (each of the
// three where its pointer is set).  The list is strictly ascending
// (k_check_active), so no two threads write one pixel.
__global__ __launch_bounds__(kBlock) void k_emit_active(const double* __restrict__ run, const double* __restrict__ run2,
                                                        uint32_t n, const uint32_t* __restrict__ active, uint32_t spp,
                                                        double* __restrict__ accum, double* __restrict__ accum_sq,
                                                        uint32_t* __restrict__ counts) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const uint32_t p = active[k];
        const size_t o = (size_t)p * 3;
        if (run) {
            accum[o] += run[3 * k];
            accum[o + 1] += run[3 * k + 1];
            accum[o + 2] += run[3 * k + 2];
        }
        if (run2) {
            accum_sq[o] += run2[3 * k];
            accum_sq[o + 1] += run2[3 * k + 1];
            accum_sq[o + 2] += run2[3 * k + 2];
        }
        if (counts) counts[p] += spp;
    }
}

// *bad = 1 unless active[0..n) is strictly ascending and below `limit` (the
// image's pixel count); *bad is zero before the launch.  Every thread that
// finds a fault stores the same 1.
__global__ __launch_bounds__(kBlock) void k_check_active(const uint32_t* __restrict__ active, uint32_t n,
                                                         uint32_t limit, uint32_t* __restrict__ bad) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const uint32_t p = active[k];
        if (p >= limit || (k > 0 && active[k - 1] >= p)) *bad = 1u;
    }
}

// counts[p] = v for the whole image (the adaptive loop's round 0)
__global__ __launch_bounds__(kBlock) void k_set_counts(uint32_t* __restrict__ counts, size_t n, uint32_t v) {
    for (size_t k = blockIdx.x * (size_t)kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock) counts[k] = v;
}

// canvas = min(sqrt(accum / spp), 1) (RayTracingWeekend.cpp:241-244), one
// body for moments.h's divisor sources: D = rtw_div_uniform is the render's
// finalize, rtw_div_counts divides by each pixel's own sample count,
// rtw_div_none takes a mean as it is.  (A template parameter: the uniform
// form has no load or branch for the other two.)
template <class D>
__global__ __launch_bounds__(kBlock) void k_finalize(const double* __restrict__ accum, size_t n, D div,
                                                     double* __restrict__ canvas) {
    for (size_t k = blockIdx.x * (size_t)kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock)
        canvas[k] = rtw_canvas_value(div(accum[k], k));
}

// rtw_noise.h on the device: the standard error of every channel from the
// raw moments (moments.h's add_pixel, the host loop's: the map is
// bit-identical) and one partial of the image-wide summary per block; cnt is
// one n for every pixel or each pixel's own counts[p] (rtw_adaptive.h: a pixel
// with fewer than two samples is left out as a non-finite one is).
// Deterministic: a thread takes pixels p, p + grid*kBlock, ... in order, a
// wave folds its lanes with a fixed shuffle tree, thread 0 merges the waves'
// values from LDS in wave order, the host merges the blocks' partials in
// block order; the grid (noise_grid) depends on the pixel count only.  No
// atomics: the two counters travel in the partials as well.
constexpr unsigned kNoiseMaxGrid = 1024;
unsigned noise_grid(uint64_t npix) {
    return (unsigned)std::min<uint64_t>((npix + kBlock - 1) / kBlock, kNoiseMaxGrid);
}

__global__ __launch_bounds__(kBlock) void k_noise_pixels(const double* __restrict__ accum,
                                                         const double* __restrict__ accum_sq, rtw_count_src cnt,
                                                         uint64_t npix, double floor3,
                                                         double* __restrict__ stderr_rgb,
                                                         rtw_noise_acc* __restrict__ parts) {
    __shared__ rtw_noise_acc s_part[kWaves];
    rtw_noise_acc a = rtw_noise_acc::empty();
    // (64-bit p: the stride may carry p past 2^32 for the largest images)
    for (uint64_t p = blockIdx.x * (uint64_t)kBlock + threadIdx.x; p < npix; p += (uint64_t)gridDim.x * kBlock)
        a.add_pixel(accum, accum_sq, cnt, p, floor3, stderr_rgb);
    // (all 256 threads reach here: the loop above has no barrier)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        a.merge(rtw_noise_acc{__shfl_down(a.sum_rel, off, 64), __shfl_down(a.max_rel, off, 64),
                              __shfl_down(a.sum_se2, off, 64), __shfl_down(a.pixels, off, 64),
                              __shfl_down(a.nonfinite, off, 64)});
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        rtw_noise_acc t = s_part[0];
        for (int w = 1; w < kWaves; ++w) t.merge(s_part[w]);
        parts[blockIdx.x] = t;
    }
}

// rtw_adaptive_select_device: the ascending list of the active pixels
// (adaptive.h rtw_pixel_active, the host's function) without atomics.  Block b
// owns the pixels [b * chunk, (b + 1) * chunk), chunk a multiple of kBlock, and
// walks them in tiles of kBlock: k_select_count leaves each block's number of
// active pixels, k_select_scan their exclusive prefix (and the total after the
// last), k_select_scatter walks the same tiles again and writes each active
// pixel at its block's base plus its rank (block_rank: ballot / popcount).
// The grid depends on the pixel count only (select_grid).
constexpr unsigned kSelectMaxGrid = 1024;
unsigned select_grid(uint64_t npix) {
    return (unsigned)std::min<uint64_t>((npix + kBlock - 1) / kBlock, kSelectMaxGrid);
}
uint64_t select_chunk(uint64_t npix) {
    const uint64_t g = select_grid(npix);
    return ((npix + g - 1) / g + kBlock - 1) / kBlock * kBlock;
}
struct select_args {
    const double *accum, *accum_sq;
    rtw_count_src cnt;
    uint64_t npix, chunk;
    double floor3, target_rel;
    uint32_t max_count;
};
__device__ __forceinline__ bool select_flag(const select_args& A, uint64_t p) {
    if (p >= A.npix) return false;
    const double s1[3] = {A.accum[3 * p], A.accum[3 * p + 1], A.accum[3 * p + 2]};
    const double s2[3] = {A.accum_sq[3 * p], A.accum_sq[3 * p + 1], A.accum_sq[3 * p + 2]};
    return rtw_pixel_active(s1, s2, A.cnt[p], A.floor3, A.target_rel, A.max_count);
}
// (the two bodies are templates over the flag's arguments: select_args here,
// window_args of rtw_adaptive_window.h below)
template <class Args>
__device__ __forceinline__ void select_count_body(const Args& A, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t s_wave[kWaves];
    const uint64_t lo = blockIdx.x * A.chunk;
    uint32_t mine = 0;
    for (uint64_t t = 0; t < A.chunk; t += kBlock) mine += select_flag(A, lo + t + threadIdx.x) ? 1u : 0u;
    uint32_t total;
    block_scan(mine, s_wave, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}
template <class Args>
__device__ __forceinline__ void select_scatter_body(const Args& A, const uint32_t* __restrict__ offsets,
                                                    uint32_t* __restrict__ active) {
    __shared__ uint32_t s_wave[kWaves];
    const uint64_t lo = blockIdx.x * A.chunk;
    uint32_t base = offsets[blockIdx.x];
    for (uint64_t t = 0; t < A.chunk; t += kBlock) {
        const uint64_t p = lo + t + threadIdx.x;
        const bool on = select_flag(A, p);
        uint32_t total;
        const uint32_t rank = block_rank(on, s_wave, total);
        if (on) active[base + rank] = (uint32_t)p;
        base += total;
        __syncthreads();  // (s_wave is rewritten by the next tile)
    }
}
__global__ __launch_bounds__(kBlock) void k_select_count(select_args A, uint32_t* __restrict__ block_counts) {
    select_count_body(A, block_counts);
}
// one block: offsets[b] = block_counts[0] + ... + block_counts[b - 1], offsets[n_blocks] = the total
__global__ __launch_bounds__(kBlock) void k_select_scan(const uint32_t* __restrict__ block_counts, uint32_t n_blocks,
                                                        uint32_t* __restrict__ offsets) {
    __shared__ uint32_t s_wave[kWaves];
    constexpr uint32_t kPer = kSelectMaxGrid / kBlock;
    uint32_t v[kPer], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t b = threadIdx.x * kPer + k;
        v[k] = b < n_blocks ? block_counts[b] : 0u;
        mine += v[k];
    }
    uint32_t total;
    uint32_t off = block_scan(mine, s_wave, total);
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t b = threadIdx.x * kPer + k;
        if (b < n_blocks) offsets[b] = off;
        off += v[k];
    }
    if (threadIdx.x == 0) offsets[n_blocks] = total;
}
__global__ __launch_bounds__(kBlock) void k_select_scatter(select_args A, const uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ active) {
    select_scatter_body(A, offsets, active);
}

// rtw_adaptive_select_window_device (rtw_adaptive_window.h): the window rule
// on bit planes.  A plane holds one bit per pixel, rows padded to
// W = ceil(nx / 64) words so that a word never straddles rows: bit k of word
// j * W + w is pixel (w * 64 + k, j); the bits beyond nx are 0.
//   k_source_bits   a wave owns one word: each lane evaluates "finite" and
//                   SOURCE (adaptive_window.h, the host's functions) of its
//                   pixel -- the only place the fp64 divisions and square
//                   roots of rtw_pixel_rel run, once per pixel -- and a ballot
//                   makes the two words, which lane 0 stores.
//   k_dilate_bits   a thread owns one word of the output plane: the OR over
//                   the rows j - r .. j + r that exist of the source word and
//                   its two neighbours, then the OR of the shifts by -r .. r
//                   with the carries from the neighbours (r <= 16 needs no
//                   word further away), and "finite" ANDed in: bit p of the
//                   result is "p is finite and a source lies in its window".
//   k_window_count / k_window_scatter   k_select_count / k_select_scatter with
//                   that bit and the counts' range as the flag; k_select_scan
//                   between them as it is.
// Every word of the three planes is written before it is read, so scratch
// reused from an earlier call needs no clearing.  No atomics; the grids depend
// on (nx, ny) only.
constexpr unsigned kBitsMaxGrid = 4096;
struct window_planes {
    uint64_t *src, *fin, *out;
    uint32_t nx, ny, W;
    RTW_HD uint64_t words() const { return (uint64_t)ny * W; }
};
__global__ __launch_bounds__(kBlock) void k_source_bits(const double* __restrict__ accum,
                                                        const double* __restrict__ accum_sq,
                                                        const uint32_t* __restrict__ counts, window_planes P,
                                                        double floor3, double target_rel) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t words = P.words();
    // (the loop's condition is the same for a wave's 64 lanes: the ballots see them all)
    for (uint64_t word = blockIdx.x * (uint64_t)kWaves + (threadIdx.x >> 6); word < words;
         word += (uint64_t)gridDim.x * kWaves) {
        const uint32_t j = (uint32_t)(word / P.W), i = (uint32_t)(word % P.W) * 64u + lane;
        bool fin = false, src = false;
        if (i < P.nx) {
            const uint64_t p = (uint64_t)j * P.nx + i;
            const double s1[3] = {accum[3 * p], accum[3 * p + 1], accum[3 * p + 2]};
            const double s2[3] = {accum_sq[3 * p], accum_sq[3 * p + 1], accum_sq[3 * p + 2]};
            fin = rtw_pixel_finite(s1, s2);
            src = rtw_pixel_source(s1, s2, fin, counts[p], floor3, target_rel);
        }
        const unsigned long long mf = __ballot(fin), ms = __ballot(src);
        if (lane == 0) P.fin[word] = mf, P.src[word] = ms;
    }
}
__global__ __launch_bounds__(kBlock) void k_dilate_bits(window_planes P, int radius) {
    const uint64_t words = P.words();
    for (uint64_t word = blockIdx.x * (uint64_t)kBlock + threadIdx.x; word < words;
         word += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(word / P.W), w = (uint32_t)(word % P.W);
        const uint32_t j0 = j > (uint32_t)radius ? j - (uint32_t)radius : 0u;
        const uint32_t j1 = j + (uint32_t)radius < P.ny - 1 ? j + (uint32_t)radius : P.ny - 1;
        uint64_t c = 0, l = 0, r = 0;  // the word's column, the one before and the one after, ORed over the rows
        for (uint32_t jj = j0; jj <= j1; ++jj) {
            const uint64_t* row = P.src + (uint64_t)jj * P.W;
            c |= row[w];
            if (w > 0) l |= row[w - 1];
            if (w + 1 < P.W) r |= row[w + 1];
        }
        uint64_t d = c;
        for (int s = 1; s <= radius; ++s) d |= (c << s) | (l >> (64 - s)) | (c >> s) | (r << (64 - s));
        P.out[word] = d & P.fin[word];
    }
}
struct window_args {
    const uint64_t* bits;  // window_planes::out
    const uint32_t* counts;
    uint64_t npix, chunk;
    uint32_t nx, W, min_count, max_count;
};
__device__ __forceinline__ bool select_flag(const window_args& A, uint64_t p) {
    if (p >= A.npix) return false;
    const uint32_t j = (uint32_t)p / A.nx, i = (uint32_t)p - j * A.nx;  // (npix < 2^32)
    const bool bit = (A.bits[(uint64_t)j * A.W + (i >> 6)] >> (i & 63u)) & 1u;
    return rtw_pixel_eligible(bit, A.counts[p], A.min_count, A.max_count);
}
__global__ __launch_bounds__(kBlock) void k_window_count(window_args A, uint32_t* __restrict__ block_counts) {
    select_count_body(A, block_counts);
}
__global__ __launch_bounds__(kBlock) void k_window_scatter(window_args A, const uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ active) {
    select_scatter_body(A, offsets, active);
}

// ---- rtw_denoise.h ------------------------------------------------------------
// The filter: host/denoise.h's functions, the host's, one thread per pixel.
// k_atrous reads the iteration's input image and the read-only features
// through the caches (a tap: the 64-byte state, the 32-byte geo and the
// coverage, all 16-byte aligned) and writes the other image of the ping-pong;
// the 3x3 variance blur is part of the pass (rtw_dn_pass).
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(const double* __restrict__ accum,
                                                            const double* __restrict__ accum_sq,
                                                            rtw_count_src cnt,
                                                            const double* __restrict__ features, double fs, double eps_a,
                                                            uint64_t npix, rtw_dn_state* __restrict__ st,
                                                            rtw_dn_geo* __restrict__ geo, rtw_dn_alb* __restrict__ alb) {
    const uint64_t p = blockIdx.x * (uint64_t)kBlock + threadIdx.x;
    if (p >= npix) return;
    const double s1[3] = {accum[3 * p], accum[3 * p + 1], accum[3 * p + 2]};
    const double s2[3] = {accum_sq[3 * p], accum_sq[3 * p + 1], accum_sq[3 * p + 2]};
    double f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = features[8 * p + k];
    rtw_dn_state s;
    rtw_dn_geo g;
    rtw_dn_alb a;
    rtw_dn_prepare(s1, s2, cnt[p], f, fs, eps_a, s, g, a);
    st[p] = s, geo[p] = g, alb[p] = a;
}

__global__ __launch_bounds__(kBlock) void k_atrous(const rtw_dn_state* __restrict__ in,
                                                   const rtw_dn_geo* __restrict__ geo,
                                                   const rtw_dn_alb* __restrict__ alb, int nx, int ny, int step,
                                                   double sigma_l, double sigma_z, int npl2,
                                                   rtw_dn_state* __restrict__ out) {
    const uint64_t p = blockIdx.x * (uint64_t)kBlock + threadIdx.x;
    if (p >= (uint64_t)nx * (uint64_t)ny) return;
    const int j = (int)(p / (uint32_t)nx), i = (int)(p - (uint64_t)j * (uint32_t)nx);
    out[p] = rtw_dn_pass(rtw_dn_images{in, geo, alb, nx}, nx, ny, i, j, step, sigma_l, sigma_z, npl2);
}

// ... and with the input staged in LDS, for the dense steps 1 and 2: a
// workgroup owns a tile of kTileX x kTileY pixels (a wave: two rows of 32) and
// stages the tile plus a halo of 2 * STEP pixels -- (32 + 4 STEP) x (8 + 4
// STEP) entries of 104 bytes: 44 928 bytes at step 1, 66 560 at step 2 -- as
// seven planes: the state's four and the geo's two 16-byte halves and the
// coverage.  A wave's 32 lanes of a row then read 32 consecutive 16-byte slots
// of a plane (ds_read_b128 without bank conflicts: each of its 16-lane groups
// covers all 64 banks once), where the array-of-structs image would put every
// fourth lane on the same banks.  Entries outside the image are not filled and
// not read (rtw_dn_pass asks for pixels inside the image only).  The same
// function on the same values: the bits of k_atrous.
constexpr int kTileX = 32, kTileY = 8;
static_assert(kTileX * kTileY == kBlock, "one thread per pixel of the tile");
constexpr int tile_entries(int step) { return (kTileX + 4 * step) * (kTileY + 4 * step); }
constexpr size_t tile_bytes(int step) { return (size_t)tile_entries(step) * (sizeof(rtw_dn_state) + sizeof(rtw_dn_geo) + 8); }
struct dn_tile {
    const double2* pl;  // planes 0..3 the state, 4..5 the geo, each `n` entries
    const double* cv;   // the coverage plane
    int n, pitch, x0, y0;  // entries per plane, entries per row, the image coordinates of entry 0
    RTW_D int at(int x, int y) const { return (y - y0) * pitch + (x - x0); }
    RTW_D rtw_dn_state state(int x, int y) const {
        const int e = at(x, y);
        const double2 a = pl[e], b = pl[n + e], c = pl[2 * n + e], d = pl[3 * n + e];
        return rtw_dn_state{{a.x, a.y, b.x}, b.y, {c.x, c.y, d.x}, d.y};
    }
    RTW_D double lv(int x, int y) const { return pl[3 * n + at(x, y)].y; }
    RTW_D rtw_dn_geo geo(int x, int y) const {
        const int e = at(x, y);
        const double2 a = pl[4 * n + e], b = pl[5 * n + e];
        return rtw_dn_geo{{a.x, a.y, b.x}, b.y};
    }
    RTW_D double cov(int x, int y) const { return cv[at(x, y)]; }
};
template <int STEP>
__global__ __launch_bounds__(kBlock) void k_atrous_tile(const rtw_dn_state* __restrict__ in,
                                                        const rtw_dn_geo* __restrict__ geo,
                                                        const rtw_dn_alb* __restrict__ alb, int nx, int ny,
                                                        double sigma_l, double sigma_z, int npl2,
                                                        rtw_dn_state* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char s_tile[];
    constexpr int H = 2 * STEP, LW = kTileX + 2 * H, LH = kTileY + 2 * H, N = LW * LH;
    double2* pl = reinterpret_cast<double2*>(s_tile);
    double* cv = reinterpret_cast<double*>(pl + 6 * N);
    const int x0 = (int)blockIdx.x * kTileX - H, y0 = (int)blockIdx.y * kTileY - H;
    for (int e = threadIdx.x; e < N; e += kBlock) {
        const int ly = e / LW, lx = e - ly * LW;
        const int x = x0 + lx, y = y0 + ly;
        if (x < 0 || x >= nx || y < 0 || y >= ny) continue;
        const size_t q = (size_t)y * (size_t)nx + (size_t)x;
        const double2* s = reinterpret_cast<const double2*>(in + q);
        const double2* g = reinterpret_cast<const double2*>(geo + q);
        pl[e] = s[0], pl[N + e] = s[1], pl[2 * N + e] = s[2], pl[3 * N + e] = s[3];
        pl[4 * N + e] = g[0], pl[5 * N + e] = g[1];
        cv[e] = alb[q].cov;
    }
    __syncthreads();
    const int i = (int)blockIdx.x * kTileX + (int)(threadIdx.x % kTileX);
    const int j = (int)blockIdx.y * kTileY + (int)(threadIdx.x / kTileX);
    if (i >= nx || j >= ny) return;
    out[(size_t)j * (size_t)nx + (size_t)i] =
        rtw_dn_pass(dn_tile{pl, cv, N, LW, x0, y0}, nx, ny, i, j, STEP, sigma_l, sigma_z, npl2);
}

__global__ __launch_bounds__(kBlock) void k_denoise_finish(const rtw_dn_state* __restrict__ st,
                                                           const rtw_dn_alb* __restrict__ alb, uint64_t npix,
                                                           double* __restrict__ out, double* __restrict__ out_var) {
    const uint64_t p = blockIdx.x * (uint64_t)kBlock + threadIdx.x;
    if (p >= npix) return;
    double o[3], ov[3];
    rtw_dn_finish(st[p], alb[p], o, ov);
    out[3 * p] = o[0], out[3 * p + 1] = o[1], out[3 * p + 2] = o[2];
    if (out_var) out_var[3 * p] = ov[0], out_var[3 * p + 1] = ov[1], out_var[3 * p + 2] = ov[2];
}

// iterations == 0: the mean and the variance of the mean, no filter
__global__ __launch_bounds__(kBlock) void k_denoise_mean(const double* __restrict__ accum,
                                                         const double* __restrict__ accum_sq,
                                                         rtw_count_src cnt, uint64_t npix,
                                                         double* __restrict__ out, double* __restrict__ out_var) {
    const uint64_t p = blockIdx.x * (uint64_t)kBlock + threadIdx.x;
    if (p >= npix) return;
    const double s1[3] = {accum[3 * p], accum[3 * p + 1], accum[3 * p + 2]};
    const double s2[3] = {accum_sq[3 * p], accum_sq[3 * p + 1], accum_sq[3 * p + 2]};
    double m[3], v[3];
    const bool ok = rtw_pixel_moments(s1, s2, cnt[p], m, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[3 * p + c] = m[c];
        if (out_var) out_var[3 * p + c] = ok ? v[c] : __builtin_nan("");
    }
}

// rtw_render_features: the first-hit feature sums of a call's pixels.  A
// thread owns whole pixels (grid stride over the call's pixels, pixel-major):
// it loads the pixel's eight sums, replays the pass's camera samples in
// increasing sample order -- camera_sample is the render's, with the render's
// pass-local sample id q = sample * npix + pixel -- makes one world query per
// sample and writes the sums back once, with 16-byte loads and stores.  Not a
// hot path (one segment per sample): every shading lookup is SF_IMG_ALL's.
#if !RTW_STRICT_RADIANCE
template <int F>
__global__ __launch_bounds__(kBlock) void k_features(scene S, job_t J, double* __restrict__ feat) {
    for (uint32_t rem = blockIdx.x * kBlock + threadIdx.x; rem < J.npix; rem += gridDim.x * kBlock) {
        const uint32_t row = udiv_fast(rem, J.div_nx);
        const uint32_t i = rem - row * (uint32_t)J.nx;
        const uint32_t j = (uint32_t)J.row_begin + row * (uint32_t)J.row_step;
        double2* o = reinterpret_cast<double2*>(feat + ((size_t)j * (size_t)J.nx + i) * RTW_FEATURE_CHANNELS);
        const double2 f0 = o[0], f1 = o[1], f2 = o[2], f3 = o[3];
        d3 alb{f0.x, f0.y, f1.x}, nrm{f1.y, f2.x, f2.y};
        double invt = f3.x, cov = f3.y;
        for (uint32_t sl = 0; sl < J.spp_pass; ++sl) {
            const uint32_t q = sl * J.npix + rem;
            uint32_t rng;
            const ray r = camera_sample<true, false>(J, q, rng);
            const hit_state h = world_closest<F>(S, r, rng);
            if (h.prim == -1) {
                alb = alb + background(S, r.d);
                continue;
            }
            d3 p, n, sfl{0, 0, 0};
            int mat;
            bool rect;
            hit_record<true, false, true>(S, r, h, p, n, mat, rect, sfl);
            const rtw_material& m = S.materials[mat];
            d3 a;
            if (m.type == RTW_MAT_METAL)
                a = ld3(m.albedo);
            else if (m.type == RTW_MAT_DIELECTRIC)
                a = d3{1.0, 1.0, 1.0};
            else  // lambertian, isotropic: the texture at the hit; a diffuse light: its emit texture
                a = texture_value<SF_IMG_ALL>(S, m.texture, p, h.prim, sfl);
            alb = alb + a;
            nrm = nrm + n;
            invt = invt + 1.0 / h.t;
            cov = cov + 1.0;
        }
        o[0] = double2{alb.x, alb.y}, o[1] = double2{alb.z, nrm.x}, o[2] = double2{nrm.y, nrm.z}, o[3] = double2{invt, cov};
    }
}

// ---- rtw_query.h: the caller's rays -------------------------------------------
// A thread owns whole rays (grid stride over the launch's rays; at most
// kQueryLaunchMax of them, so the 32-bit index cannot wrap).  A record is 64
// bytes: four 16-byte loads / stores per lane, as k_features moves a pixel's
// sums -- a wave's four instructions together read 4 KiB of consecutive bytes,
// every line whole, and one world walk per 128 bytes moved leaves nothing for
// an LDS transpose to win.
struct query_args {
    const rtw_query_ray* rays;
    uint32_t* rng;     // null: the scene has no media, no state is read or written
    uint32_t n;
    uint32_t check;    // the scene has a BVH and moving spheres: ray times must lie in [sh0, sh1]
    double sh0, sh1;   // the shutter the BVH's boxes cover
    uint32_t* bad;     // counter of rays outside it (check != 0)
};
struct query_ray_in {
    ray r;
    double t_max;
    bool walk;  // t_max > 0.001f and the ray's time can be traced
};
__device__ __forceinline__ query_ray_in load_query_ray(const query_args& Q, uint32_t k) {
    const double2* in = reinterpret_cast<const double2*>(Q.rays + k);
    const double2 a = in[0], b = in[1], c = in[2], d = in[3];
    query_ray_in x;
    x.r.o = d3{a.x, a.y, b.x}, x.r.d = d3{b.y, c.x, c.y}, x.r.t = d.x;
    x.t_max = d.y;
    x.walk = x.t_max > kTMin;  // (false for NaN)
    if (Q.check && !(x.r.t >= Q.sh0 && x.r.t <= Q.sh1)) {
        atomicAdd(Q.bad, 1u);
        x.walk = false;
    }
    return x;
}

template <int F>
__global__ __launch_bounds__(kBlock) void k_query(scene S, query_args Q, rtw_query_hit* __restrict__ hits) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < Q.n; k += gridDim.x * kBlock) {
        const query_ray_in x = load_query_ray(Q, k);
        hit_state h{x.t_max, -1, false};
        if (x.walk) {
            uint32_t rng = 0;
            if constexpr ((F & F_MEDIA) != 0) rng = Q.rng[k];
            h = world_closest_from<F>(S, x.r, rng, x.t_max);
            if constexpr ((F & F_MEDIA) != 0) Q.rng[k] = rng;
        }
        d3 p{0, 0, 0}, n{0, 0, 0};
        int mat = -1;
        if (h.prim != -1) {
            bool rect;
            d3 sl;
            hit_record<true, false, false>(S, x.r, h, p, n, mat, rect, sl);
        }
        double2* o = reinterpret_cast<double2*>(hits + k);
        const long long ids = (long long)(((unsigned long long)(uint32_t)mat << 32) | (uint32_t)h.prim);
        o[0] = double2{h.t, p.x}, o[1] = double2{p.y, p.z}, o[2] = double2{n.x, n.y};
        o[3] = double2{n.z, __longlong_as_double(ids)};
    }
}

// occluded[k] = k_query's prim != -1.  Media-free forms leave the walk at the
// first accepted hit (world_walk kWalkAny); with media the closest walk runs
// unchanged, draws and states as k_query's.
template <int F>
__global__ __launch_bounds__(kBlock) void k_occluded(scene S, query_args Q, uint8_t* __restrict__ occluded) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < Q.n; k += gridDim.x * kBlock) {
        const query_ray_in x = load_query_ray(Q, k);
        hit_state h{x.t_max, -1, false};
        if (x.walk) {
            uint32_t rng = 0;
            if constexpr ((F & F_MEDIA) != 0) rng = Q.rng[k];
            h = world_closest_from<F, (F & F_MEDIA) == 0>(S, x.r, rng, x.t_max);
            if constexpr ((F & F_MEDIA) != 0) Q.rng[k] = rng;
        }
        occluded[k] = h.prim != -1 ? 1 : 0;
    }
}

// rtw_camera_rays: camera_sample of the pass-local sample ids [q0, q0 + count)
// with the ray and the stream's state after the camera's draws stored.
__global__ __launch_bounds__(kBlock) void k_camera_rays(job_t J, uint32_t q0, uint32_t count,
                                                        rtw_query_ray* __restrict__ rays, uint32_t* __restrict__ rng_out) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < count; k += (uint64_t)gridDim.x * kBlock) {
        uint32_t rng;
        const ray r = camera_sample<true, false>(J, q0 + (uint32_t)k, rng);
        double2* o = reinterpret_cast<double2*>(rays + k);
        o[0] = double2{r.o.x, r.o.y}, o[1] = double2{r.o.z, r.d.x}, o[2] = double2{r.d.y, r.d.z};
        o[3] = double2{r.t, __builtin_inf()};
        if (rng_out) rng_out[k] = rng;
    }
}
#endif

// ======================================================================
// host side
// ======================================================================
#define HIPCHK(x)                                                                             \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess)                                                                  \
            return rtw_fail(RTW_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));      \
    } while (0)

struct dev_buf {
    void* p = nullptr;
    size_t bytes = 0;
    dev_buf() = default;
    dev_buf(const dev_buf&) = delete;
    dev_buf& operator=(const dev_buf&) = delete;
    ~dev_buf() { release(); }  // (rtw_scene_free: on the handle's device, its stream synchronised)
    int ensure(size_t n) {
        if (n <= bytes) return RTW_OK;
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
        if (hipMalloc(&p, n) != hipSuccess) return rtw_fail(RTW_ERR_OOM, "hipMalloc of " + std::to_string(n) + " bytes failed");
        bytes = n;
        return RTW_OK;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct handle_t {
    int device = 0;
    hipStream_t stream = nullptr;
    scene S{};
    layout_facts facts;  // what selection and rtw_scene_query read of it (host/scene_layout.h)
    const char* scene_base = nullptr;
    dev_buf scene_mem;
    dev_buf scene32;  // fp32 mirror of the scene (fast mode, rtw_fast.h)
    rtwf::fscene F32{};
    dev_buf pool[2];  // path SoA, ping-pong for compaction
    dev_buf fresh;    // staging of new camera rays (fresh_t)
    dev_buf hits;
    dev_buf radiance; // per-sample planes of one pass
    dev_buf run;      // per-pixel running sums
    dev_buf flog;     // RTW_STRICT_RADIANCE: per-thread factor logs (job_t::flog)
    dev_buf accum;    // device accum when the caller passes a host pointer
    dev_buf run2;     // rtw_render_accumulate_moments: per-pixel running sums of squares
    dev_buf accum_sq; // ... device accum_sq when the caller passes a host pointer
    dev_buf noise;    // rtw_noise_estimate_device: per-block partials (rtw_noise_acc)
    // rtw_adaptive.h
    dev_buf alist;    // the device copy of a host pixel list; the adaptive loop's list
    dev_buf counts;   // the device copy of a host counts buffer; the adaptive loop's counts
    dev_buf sel;      // rtw_adaptive_select_device: per-block counts, their prefix, the list check's flag
    dev_buf wbits;    // rtw_adaptive_select_window_device: the three bit planes (window_planes)
    // rtw_denoise.h
    dev_buf features;     // the device copy of a host feature buffer
    dev_buf dn_state[2];  // rtw_denoise_device: the iteration state, ping-pong (rtw_dn_state)
    dev_buf dn_geo, dn_alb;  // ... and the per-pixel features the passes only read
    // rtw_query.h
    dev_buf q_rays, q_out, q_rng;  // one staged chunk of a host-buffer query (query_plan)
    dev_buf q_bad;                 // counter of rays whose time the BVH's boxes do not cover
    dev_buf ctrs;
    dev_buf camera;                // device copy of the call's camera
    rtw_camera_desc cam_host{};    // its source (lives until the copy ran)
    ctrs_t* host_ctrs = nullptr;  // pinned
    uint32_t pool_cap = 0;
    int grid = 2048;
    int cus = 256;
    std::vector<hipEvent_t> events;
};

// The scene on the card: rtw_layout_scene's two blobs (host/scene_layout.cpp)
// copied as they are, and the kernels' scene structs pointed into them.
int upload_scene(handle_t* h, const rtw_scene_desc* d) {
    // (RTW_BOX_TABLE=0 at upload: no box-plane table, for tests of the rect path)
    const char* box_env = std::getenv("RTW_BOX_TABLE");
    const bool box_table = !(box_env && *box_env && std::atoi(box_env) == 0);
    scene_layout L;
    if (int rc = rtw_layout_scene(d, box_table, &L)) return rc;
    if (int rc = h->scene_mem.ensure(L.mem64.size())) return rc;
    if (int rc = h->scene32.ensure(L.mem32.size())) return rc;
    HIPCHK(hipMemcpy(h->scene_mem.p, L.mem64.data(), L.mem64.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->scene32.p, L.mem32.data(), L.mem32.size(), hipMemcpyHostToDevice));
    const char* base = static_cast<const char*>(h->scene_mem.p);
    const char* b2 = static_cast<const char*>(h->scene32.p);
    // an absent array is a null pointer
    auto at = [](const char* b, const layout_span& a) { return a.bytes ? (const void*)(b + a.off) : nullptr; };
    const layout_arrays64& A = L.at64;
    const layout_scalars& s = L.s;
    scene& S = h->S;
    S.prims = (const rtw_prim*)at(base, A.prims);
    S.entries = (const dev_entry*)at(base, A.entries);
    S.materials = (const rtw_material*)at(base, A.materials);
    S.textures = (const rtw_texture*)at(base, A.textures);
    S.lights = (const rtw_light*)at(base, A.lights);
    S.ranvec = (const double*)at(base, A.ranvec);
    S.perm = (const int32_t*)at(base, A.perm);
    S.media = (const int32_t*)at(base, A.media);
    S.prim_onb = (const double*)at(base, A.prim_onb);
    S.mat_aux = (const double*)at(base, A.mat_aux);
    S.ops = (const dev_op*)at(base, A.ops);
    S.nodes = (const node_store*)at(base, A.nodes);
    S.items = (const int32_t*)at(base, A.items);
    S.runs = (const world_run*)at(base, A.runs);
    S.ysph = (const float*)at(base, A.ysph);
    S.boxes = (const double*)at(base, A.boxes);
    S.texels = (const uint8_t*)at(base, A.texels);
    S.bvh_bound = s.bvh_bound;
    S.ysb_cx = s.ysb_cx, S.ysb_cy = s.ysb_cy, S.ysb_dy = s.ysb_dy, S.ysb_cz = s.ysb_cz, S.ysb_r2 = s.ysb_r2;
    S.n_runs = s.n_runs;
    S.mv_common = s.mv_common, S.mv_t0 = s.mv_t0, S.mv_den = s.mv_den;
    S.fast_div = s.fast_div;
    S.n_entries = s.n_entries, S.n_lights = s.n_lights, S.light_weight = s.light_weight;
    S.world_bvh_root = s.world_bvh_root, S.n_nodes = s.n_nodes;
    S.render_type = s.render_type, S.background = s.background;
    S.n_media = s.n_media, S.has_media = s.has_media;
    h->scene_base = base;
    const layout_arrays32& B = L.at32;
    rtwf::fscene& F = h->F32;
    F.prims = (const rtwf::prim32*)at(b2, B.prims);
    F.entries = (const rtwf::ent32*)at(b2, B.entries);
    F.ops = (const rtwf::op32*)at(b2, B.ops);
    F.materials = (const rtwf::mat32*)at(b2, B.materials);
    F.textures = (const rtwf::tex32*)at(b2, B.textures);
    F.ranvec = (const float*)at(b2, B.ranvec);
    F.frames = (const float*)(b2 + B.frames.off);  // (never null, prims or not)
    F.lights = (const rtw_light*)at(b2, B.lights);
    F.perm = (const int32_t*)at(b2, B.perm);
    F.nodes = (const node_store*)at(b2, B.nodes);
    F.boxes = (const float*)at(b2, B.boxes);
    F.texels = S.texels, F.items = S.items, F.runs = S.runs, F.media = S.media, F.ysph = S.ysph;
    F.mv_t0 = s.f_mv_t0, F.mv_inv_den = s.f_mv_inv_den, F.light_weight = s.f_light_weight;
    F.n_lights = S.n_lights, F.world_bvh_root = S.world_bvh_root;
    F.render_type = S.render_type, F.background = S.background;
    F.n_media = S.n_media, F.n_runs = S.n_runs, F.n_nodes = S.n_nodes;
    h->facts = L.facts;
    return RTW_OK;
}

// Resident workgroups per CU of kernel `fn` at `block` threads and `shm`
// bytes of dynamic LDS on the current device: one occupancy query per
// (kernel, block, LDS bytes, device), cached.  rtw_render_multi renders from
// one host thread per device at once, so the cache is guarded.  Returns 0
// when the block does not fit at all and -1 when the query itself fails (not
// cached): the packet search reads -1 as "does not fit", only grid sizing
// (grid_blocks) falls back to 2 workgroups per CU.
int blocks_per_cu(const void* fn, int block, size_t shm) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, size_t, int>, int> cache;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    const auto key = std::make_tuple(fn, block, shm, dev);
    {
        std::lock_guard<std::mutex> g(mu);
        const auto it = cache.find(key);
        if (it != cache.end()) return it->second;
    }
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block, shm) != hipSuccess) return -1;
    nb = std::max(nb, 0);
    std::lock_guard<std::mutex> g(mu);
    cache[key] = nb;
    return nb;
}

// Grid of a persistent launch: the number of blocks that can be resident at
// once (workgroups per CU x CUs), so every block starts immediately; a failed
// occupancy query assumes 2 per CU, a block that does not fit still gets 1
// per CU.
int grid_blocks(const void* fn, int block, size_t shm, int cus) {
    const int nb = blocks_per_cu(fn, block, shm);
    return (nb < 0 ? 2 : std::max(1, nb)) * cus;
}

// BVH node packet of a launch with LDS stacks (k_persist<.., true>,
// k_fast<.., true>): the most top nodes (BFS numbering, rtw_scene_upload)
// that fit in LDS beside the kernel's own arrays and the `shm` bytes of
// shading data without costing a workgroup per CU (occupancy query per
// candidate size; a size that does not fit ends the search, so a launch with
// the packet always fits).  RTW_LDS_NODES=<n> caps it (0 = off: A/B).
constexpr size_t kPacketNodeBytes = sizeof(node_store);
uint32_t node_packet(const void* fn, int block, size_t shm, int n_nodes) {
    const char* e = std::getenv("RTW_LDS_NODES");
    uint32_t cap = (e && *e) ? (uint32_t)std::max(0, std::atoi(e)) : 4096u;
    cap = std::min<uint32_t>(cap, (uint32_t)std::max(0, n_nodes));
    if (!cap) return 0;
    const int base = blocks_per_cu(fn, block, shm);
    if (base <= 0) return 0;
    const size_t off = (shm + 15) & ~size_t(15);
    uint32_t best = 0;
    for (uint32_t k = 32; k <= cap + 31; k += 32) {
        const uint32_t kk = std::min(k, cap);
        if (blocks_per_cu(fn, block, off + kk * kPacketNodeBytes) < base) break;
        best = kk;
        if (kk == cap) break;
    }
    return best;
}

// The strict build's factor log holds J.flog_threads threads' paths, indexed
// by global thread id (a path never leaves its thread in k_persist): its grid
// is capped to fit whatever the occupancy query says (a persistent kernel
// drains the sample queue with any grid).
inline int strict_grid(int grid, const job_t& J) {
#if RTW_STRICT_RADIANCE
    return std::max(1, std::min(grid, (int)(J.flog_threads / (uint32_t)kPBlock)));
#else
    return grid;
#endif
}

// The launch tables: one row per entry of rtw_select.h's instantiation lists,
// in their order.  These rows are what instantiates the kernels.
struct persist_row {
    const void *sort, *plain, *lst;  // k_persist_sort<f, m, l>, k_persist<f, m, l, false / true>
};
template <size_t... I>
std::array<persist_row, sizeof...(I)> persist_rows(std::index_sequence<I...>) {
    return {persist_row{
        reinterpret_cast<const void*>(&k_persist_sort<kPersistList[I].f, kPersistList[I].m, kPersistList[I].l>),
        reinterpret_cast<const void*>(&k_persist<kPersistList[I].f, kPersistList[I].m, kPersistList[I].l, false>),
        reinterpret_cast<const void*>(&k_persist<kPersistList[I].f, kPersistList[I].m, kPersistList[I].l, true>)}...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> segment_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_segment<kSegmentList[I].f, kSegmentList[I].m, kSegmentList[I].l>)...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> fast_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_fast<kFastList[I].f, kFastList[I].l>)...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> fast_sort_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_fast_sort<kFastSortList[I].f, kFastSortList[I].l>)...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> shade_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_shade<kShadeList[I].m, kShadeList[I].l>)...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> intersect_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_intersect<kIntersectList[I].f>)...};
}
// ... and the active lists' rows: one kernel each, in the row's form
template <size_t I>
const void* persist_active_fn() {
    constexpr active_inst a = kPersistActiveList[I];
    if constexpr (a.form == kform::persist_sort)
        return reinterpret_cast<const void*>(&k_persist_sort<a.id.f, a.id.m, a.id.l>);
    else
        return reinterpret_cast<const void*>(&k_persist<a.id.f, a.id.m, a.id.l, a.form == kform::persist_lst>);
}
template <size_t... I>
std::array<const void*, sizeof...(I)> persist_active_rows(std::index_sequence<I...>) {
    return {persist_active_fn<I>()...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> fast_active_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_fast<kFastActiveList[I].id.f, kFastActiveList[I].id.l>)...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> fast_sort_active_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_fast_sort<kFastSortActiveList[I].id.f, kFastSortActiveList[I].id.l>)...};
}
// ... and the rows of caller-supplied rays (kPersistRaysList), likewise
template <size_t I>
const void* persist_rays_fn() {
    constexpr active_inst a = kPersistRaysList[I];
    if constexpr (a.form == kform::persist_sort)
        return reinterpret_cast<const void*>(&k_persist_sort<a.id.f, a.id.m, a.id.l>);
    else
        return reinterpret_cast<const void*>(&k_persist<a.id.f, a.id.m, a.id.l, a.form == kform::persist_lst>);
}
template <size_t... I>
std::array<const void*, sizeof...(I)> persist_rays_rows(std::index_sequence<I...>) {
    return {persist_rays_fn<I>()...};
}
const auto kPersistRaysRows = persist_rays_rows(std::make_index_sequence<kPersistRaysList.size()>{});
const auto kPersistActiveRows = persist_active_rows(std::make_index_sequence<kPersistActiveList.size()>{});
const auto kFastActiveRows = fast_active_rows(std::make_index_sequence<kFastActiveList.size()>{});
const auto kFastSortActiveRows = fast_sort_active_rows(std::make_index_sequence<kFastSortActiveList.size()>{});
const auto kShadeRows = shade_rows(std::make_index_sequence<kShadeList.size()>{});
const auto kIntersectRows = intersect_rows(std::make_index_sequence<kIntersectList.size()>{});
const auto kPersistRows = persist_rows(std::make_index_sequence<kPersistList.size()>{});
const auto kSegmentRows = segment_rows(std::make_index_sequence<kSegmentList.size()>{});
const auto kFastRows = fast_rows(std::make_index_sequence<kFastList.size()>{});
const auto kFastSortRows = fast_sort_rows(std::make_index_sequence<kFastSortList.size()>{});

template <class... A>
void launch(const void* fn, int grid, int block, size_t shm, hipStream_t st, A... a) {
    void* args[] = {&a...};
    (void)hipLaunchKernel(fn, dim3(grid), dim3(block), args, shm, st);  // (callers check hipGetLastError)
}

// The environment of the choice.  RTW_MODE and RTW_SPLIT are read at every
// call, RTW_SORT and RTW_FAST_SORT once per process.
select_env read_env() {
    const auto flag = [](const char* name) {  // -1 unset or empty, else 0 / 1
        const char* e = std::getenv(name);
        return (e && *e) ? (std::atoi(e) != 0 ? 1 : 0) : -1;
    };
    static const int sort = flag("RTW_SORT"), fast_sort = flag("RTW_FAST_SORT");
    const char* mode = std::getenv("RTW_MODE");
    return {mode && std::string(mode) == "wavefront", flag("RTW_SPLIT") == 1, sort, fast_sort != 0};
}

// What selection reads of an uploaded scene; pin: the camera is a pinhole.
select_in scene_facts(const handle_t* h, bool pin) {
    select_in s = rtw_layout_select_in(h->facts, pin);
    s.strict = RTW_STRICT_RADIANCE != 0;
    return s;
}

// fp32 renders of a scene with image textures exist for list and world-BVH
// scenes (select_fp32); media or group BVHs with images: fp64 only.
bool fast_image_ok(const handle_t* h) {
    const int f = h->facts.features & (F_MEDIA | F_WBVH | F_GBVH);
    return !(h->facts.shade_mask & SF_IMAGE) || f == 0 || f == F_WBVH;
}

// A render's kernel under the current environment: the choice, its row of the
// launch tables and its LDS layout.  Launches nothing (occupancy queries only).
struct plan_t {
    kernel_choice c;
    const void* fn = nullptr;        // the kernel (the split pair: k_intersect)
    const void* fn_shade = nullptr;  // the split pair's k_shade
    size_t shm = 0;            // LDS bytes of the scene's shading data (0: read through the caches)
    uint32_t packet = 0;       // BVH nodes staged in LDS (persist_lst, fast with LDS stacks)
};
// active: of a pixel list (select_active: a row of the active lists, or a
// wavefront form, which wavefront_pass refills with k_regen_active).
int plan_render(const handle_t* h, bool pin, bool fast, plan_t* out, bool active = false) {
    select_in s = scene_facts(h, pin);
    s.env = read_env();
    s.active = active;
    plan_t p{fast ? select_fp32(s) : select_fp64(s)};
    const kform form = p.c.form;
    if (form == kform::split) {  // (its rows cover every choice: split_resolve)
        const split_rows r = split_resolve(p.c.id);
        p.fn = kIntersectRows[index_of(kIntersectList, r.intersect)];
        p.fn_shade = kShadeRows[index_of(kShadeList, r.shade)];
        p.shm = r.shade.l ? h->facts.shade_bytes : 0;
        *out = p;
        return RTW_OK;
    }
    const inst& id = p.c.id;
    p.shm = !id.l ? 0 : form == kform::fast_sort ? h->facts.f32_bytes : form == kform::fast ? 0 : h->facts.shade_bytes;
    const bool fp64 = form == kform::persist_sort || form == kform::persist || form == kform::persist_lst;
    const bool act = active && form != kform::segment;  // (a row of the active lists)
    const active_inst arow{id, form};
    const int at = act ? (fp64 ? index_of(kPersistActiveList, arow)
                          : form == kform::fast ? index_of(kFastActiveList, arow) : index_of(kFastSortActiveList, arow))
                 : fp64 ? index_of(kPersistList, id) : form == kform::segment ? index_of(kSegmentList, id)
                 : form == kform::fast ? index_of(kFastList, id)
                 : form == kform::fast_sort ? index_of(kFastSortList, id) : 0;
    if (at < 0) return rtw_fail(RTW_ERR_HIP, "no such instantiation: " + p.c.name);
    if (fp64) {
        if (act) {
            p.fn = kPersistActiveRows[at];
        } else {
            const persist_row& r = kPersistRows[at];
            p.fn = form == kform::persist_sort ? r.sort : form == kform::persist ? r.plain : r.lst;
        }
        if (form == kform::persist_lst) p.packet = node_packet(p.fn, kPBlock, p.shm, h->S.n_nodes);
    } else if (form == kform::segment) {
        p.fn = kSegmentRows[at];
    } else if (form == kform::fast) {
        p.fn = act ? kFastActiveRows[at] : kFastRows[at];
        if (id.l) p.packet = node_packet(p.fn, rtwf::fast_block(id.f), 0, h->F32.n_nodes);
    } else if (form == kform::fast_sort) {
        p.fn = act ? kFastSortActiveRows[at] : kFastSortRows[at];
    }
    *out = p;
    return RTW_OK;
}

// A radiance query's kernel (rtw_radiance.h, select_rays): a row of
// kPersistRaysList, or a wavefront form, which wavefront_pass refills with
// k_regen_rays.
int plan_rays(const handle_t* h, plan_t* out) {
    select_in s = scene_facts(h, false);
    s.env = read_env();
    plan_t p{select_rays(s)};
    const kform form = p.c.form;
    const inst& id = p.c.id;
    if (form == kform::split) {
        const split_rows r = split_resolve(id);
        p.fn = kIntersectRows[index_of(kIntersectList, r.intersect)];
        p.fn_shade = kShadeRows[index_of(kShadeList, r.shade)];
        p.shm = r.shade.l ? h->facts.shade_bytes : 0;
    } else {
        p.shm = id.l ? h->facts.shade_bytes : 0;
        const int at = form == kform::segment ? index_of(kSegmentList, id) : index_of(kPersistRaysList, active_inst{id, form});
        if (at < 0) return rtw_fail(RTW_ERR_HIP, "no such instantiation: " + p.c.name);
        p.fn = form == kform::segment ? kSegmentRows[at] : kPersistRaysRows[at];
        if (form == kform::persist_lst) p.packet = node_packet(p.fn, kPBlock, p.shm, h->S.n_nodes);
    }
    *out = p;
    return RTW_OK;
}

// One pass of a persistent plan (FA: the fp32 kernels' arguments).
void launch_persistent(const plan_t& p, const handle_t* h, hipStream_t st, const job_t& J, ctrs_t* C,
                       const fast_args& FA) {
    const persist_args PA{h->S, J, C, h->scene_base, h->facts.shade_bytes};
    switch (p.c.form) {
    case kform::persist_sort:
        launch(p.fn, grid_blocks(p.fn, kSortBlock, p.shm, h->cus), kSortBlock, p.shm, st, PA);
        break;
    case kform::persist:
        launch(p.fn, strict_grid(grid_blocks(p.fn, kPBlock, p.shm, h->cus), J), kPBlock, p.shm, st, PA);
        break;
    case kform::persist_lst: {  // 16-bit LDS stacks, the node packet after the shading data
        persist_args a = PA;
        a.lds_nodes = p.packet;
        a.lds_nodes_off = (uint32_t)((p.shm + 15) & ~size_t(15));
        const size_t shm = p.packet ? a.lds_nodes_off + p.packet * kPacketNodeBytes : p.shm;
        launch(p.fn, strict_grid(grid_blocks(p.fn, kPBlock, p.shm, h->cus), J), kPBlock, shm, st, a);
        break;
    }
    case kform::fast: {
        fast_args a = FA;
        a.lds_nodes = p.packet;
        const size_t shm = (size_t)p.packet * sizeof(node_store);
        const int blk = rtwf::fast_block(p.c.id.f);
        launch(p.fn, grid_blocks(p.fn, blk, shm, h->cus), blk, shm, st, a);
        break;
    }
    case kform::fast_sort: {
        const char* base = static_cast<const char*>(h->scene32.p);
        const uint32_t bytes = h->facts.f32_bytes;
        fast_args a = FA;  // the arrays' offsets in the LDS copy (lds_fscene_off)
        const void* ptrs[9] = {FA.S.prims, FA.S.entries, FA.S.ops, FA.S.materials, FA.S.textures,
                               FA.S.lights, FA.S.ranvec, FA.S.perm, FA.S.frames};
        for (int k = 0; k < 9; ++k) {
            const char* c = static_cast<const char*>(ptrs[k]);
            a.lds_off[k] = (c && base && c >= base && c < base + bytes) ? (uint32_t)(c - base) : ~0u;
        }
        launch(p.fn, grid_blocks(p.fn, kSortBlock, p.shm, h->cus), kSortBlock, p.shm, st, a, base, bytes);
        break;
    }
    case kform::segment:
    case kform::split: break;  // (wavefront_pass)
    }
}

// The split pair's launches, from the plan's rows (rtw_select.h split_resolve).
void launch_shade(const plan_t& p, int grid, hipStream_t st, const scene& S, const job_t& J, const paths_t& A,
                  const fresh_t& F, const double* ht, const int32_t* hid, ctrs_t* C, const char* base, uint32_t bytes) {
    launch(p.fn_shade, grid, kBlock, p.shm, st, S, J, A, F, ht, hid, C, base, bytes);
}
void launch_intersect(const plan_t& p, int grid, hipStream_t st, const scene& S, const paths_t& A, const fresh_t& FR,
                      double* ht, int32_t* hid, ctrs_t* C) {
    launch(p.fn, grid, kBlock, 0, st, S, A, FR, ht, hid, C);
}

hipEvent_t event_at(handle_t* h, size_t k) {
    while (h->events.size() <= k) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->events.push_back(e);
    }
    return h->events[k];
}

size_t pass_budget_samples() {
    if (const char* s = std::getenv("RTW_PASS_SAMPLES")) {
        const long long v = std::atoll(s);
        if (v > 0) return (size_t)v;
    }
    return size_t(1) << 30;  // 24 GiB of per-sample radiance records per pass (T: one pass)
}

// PPM channel bytes (RayTracingWeekend.cpp:266-270): int(255.99f * c) as
// x86 converts (truncation; NaN / out of range -> INT_MIN, cvttsd2si).
__global__ __launch_bounds__(kBlock) void k_quantize(const double* __restrict__ canvas, size_t n,
                                                     int32_t* __restrict__ out) {
    for (size_t k = blockIdx.x * (size_t)kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock) {
        const double x = (double)255.99f * canvas[k];
        out[k] = (x == x && x < 2147483648.0 && x > -2147483649.0) ? (int32_t)x : (int32_t)0x80000000u;
    }
}

// dst += src (rtw_render_multi's final add into a device accumulator)
__global__ __launch_bounds__(kBlock) void k_add(double* __restrict__ dst, const double* __restrict__ src, size_t n) {
    for (size_t k = blockIdx.x * (size_t)kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock)
        dst[k] += src[k];
}

unsigned grid_for(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + kBlock - 1) / kBlock, 8192)); }

}  // namespace

#ifndef RTW_BUILD_ID
#define RTW_BUILD_ID "unknown"
#endif
extern "C" const char* rtw_build_id(void) { return RTW_BUILD_ID; }

extern "C" int rtw_scene_query(void* handle, rtw_scene_info* out) {
    const handle_t* h = static_cast<const handle_t*>(handle);
    if (!h || !out) return rtw_fail(RTW_ERR_INVALID, "rtw_scene_query: null argument");
    std::memset(out, 0, sizeof *out);
    out->device = h->device;
    out->n_world_runs = h->facts.n_runs;
    out->n_ysphere_runs = h->facts.n_ysph_runs;
    out->n_plain_runs = h->facts.n_plain_runs;
    out->features = h->facts.features;
    out->shade_mask = h->facts.shade_mask;
    out->shade_lds_bytes = h->facts.shade_bytes <= kShadeLdsMax ? (int32_t)h->facts.shade_bytes : 0;
    HIPCHK(hipSetDevice(h->device));  // occupancy queries of the plans
    // the kernels of a render with the scene's own camera
    plan_t p64, p32;
    if (int rc = plan_render(h, h->facts.desc_pin, false, &p64)) return rc;
    if (int rc = plan_render(h, h->facts.desc_pin, true, &p32)) return rc;
    out->bvh_lds_nodes = (int32_t)p64.packet;
    std::snprintf(out->kernel, sizeof out->kernel, "%s", p64.c.name.c_str());
    std::snprintf(out->build_id, sizeof out->build_id, "%s", RTW_BUILD_ID);
    std::snprintf(out->kernel_fast, sizeof out->kernel_fast, "%s", p32.c.name.c_str());
    return RTW_OK;
}

extern "C" int rtw_quantize_canvas_device(void* handle, const double* canvas, int nx, int ny, int32_t* out) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !canvas || !out || nx <= 0 || ny <= 0)
        return rtw_fail(RTW_ERR_INVALID, "rtw_quantize_canvas_device: bad argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)nx * (size_t)ny * 3;
    hipLaunchKernelGGL(k_quantize, dim3(grid_for(n)), dim3(kBlock), 0, h->stream, canvas, n, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RTW_OK;
}

// internal (rtw_host_util.h): the device of a handle, and dst += src on it
int rtw_handle_device(void* handle) { return handle ? static_cast<handle_t*>(handle)->device : -1; }

int rtw_handle_add_device(void* handle, double* dst, const double* src, size_t n) {
    handle_t* h = static_cast<handle_t*>(handle);
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_add, dim3(grid_for(n)), dim3(kBlock), 0, h->stream, dst, src, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RTW_OK;
}

// A device accumulator must be memory the scene's GPU can address: device
// memory of that GPU (hipMalloc, torch's caching and expandable-segment
// allocators) or managed memory (hipMallocManaged: any GPU).  Host memory,
// pinned host memory and unknown pointers are refused (a host pointer is
// passed with accum_on_device = 0 instead).
int rtw_check_device_ptr(const void* p, int device, const char* what, bool allow_managed) {
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess ||
        (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged)) {
        (void)hipGetLastError();  // clear the sticky error of a failed query
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": accum_on_device is set but the accumulator is not "
                                                              "device or managed memory");
    }
    if (a.type == hipMemoryTypeManaged && !allow_managed)
        return rtw_fail(RTW_ERR_UNSUPPORTED, std::string(what) + ": a managed-memory accumulator is supported with "
                                                                  "one GPU only (the cross-device write is unverified)");
    if (a.type == hipMemoryTypeDevice && a.device != device)
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": the device accumulator lives on device " +
                                             std::to_string(a.device) + ", the scene on device " +
                                             std::to_string(device));
    return RTW_OK;
}

extern "C" int rtw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int rtw_scene_upload(int device, const rtw_scene_desc* desc, void** out_handle) {
    if (!out_handle) return rtw_fail(RTW_ERR_INVALID, "rtw_scene_upload: null out_handle");
    *out_handle = nullptr;
    int rc = validate_desc(desc);
    if (rc) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return rtw_fail(RTW_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return rtw_fail(RTW_ERR_INVALID, "device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return rtw_fail(RTW_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950");
    handle_t* h = new handle_t;
    h->device = device;
    h->grid = prop.multiProcessorCount * 8;
    h->cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return rtw_fail(RTW_ERR_HIP, "hipStreamCreate failed");
    }
    rc = upload_scene(h, desc);
    if (!rc) rc = h->ctrs.ensure(sizeof(ctrs_t));
    if (!rc && hipHostMalloc((void**)&h->host_ctrs, sizeof(ctrs_t) * 64, hipHostMallocDefault) != hipSuccess)
        rc = rtw_fail(RTW_ERR_OOM, "hipHostMalloc failed");
    if (rc) {
        rtw_scene_free(h);
        return rc;
    }
    *out_handle = h;
    return RTW_OK;
}

extern "C" void rtw_scene_free(void* handle) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->host_ctrs) hipHostFree(h->host_ctrs);
    for (hipEvent_t e : h->events) hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;  // frees its buffers (dev_buf)
}

// The non-null ones of a call's device buffers belong to the handle's device.
static int check_handle_ptrs(const handle_t* h, const char* what, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (p)
            if (int rc = rtw_check_device_ptr(p, h->device, what)) return rc;
    return RTW_OK;
}

// The canvas of an image's sums over a divisor source (k_finalize<D>);
// returns when the kernel has ended.
template <class D>
static int launch_finalize(handle_t* h, const double* sums, int nx, int ny, D div, double* canvas) {
    const size_t n = (size_t)nx * (size_t)ny * 3;
    hipLaunchKernelGGL(k_finalize<D>, dim3(grid_for(n)), dim3(kBlock), 0, h->stream, sums, n, div, canvas);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return RTW_OK;
}

extern "C" int rtw_finalize_canvas_device(void* handle, const double* accum, int nx, int ny, int spp,
                                          double* canvas) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !accum || !canvas || nx <= 0 || ny <= 0 || spp <= 0)
        return rtw_fail(RTW_ERR_INVALID, "rtw_finalize_canvas_device: bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_finalize(h, accum, nx, ny, rtw_div_uniform{(double)spp}, canvas);
}

namespace {

using ev_list = std::vector<std::pair<size_t, size_t>>;  // event slots around timed launches

// A call's events: slots of the handle's event list, handed out in order.
// collect_kernel_times: 1 = events around each traversal launch (the
// roofline kernel), 2 = also around each shade launch.  Every event pair
// costs a few us of queue gap per iteration, so the default is neither.
struct call_events {
    handle_t* h;
    size_t ev = 0;
    ev_list isect_ev, shade_ev;
    ev_list *time_isect = nullptr, *time_shade = nullptr;
    call_events(handle_t* h_, int collect) : h(h_) {
        if (collect != 0) time_isect = &isect_ev;
        if (collect >= 2) time_shade = &shade_ev;
    }
    // launch(), between two events whose slots go to *list (null: untimed)
    template <class L>
    int timed(ev_list* list, L&& launch) {
        if (!list) {
            launch();
            return RTW_OK;
        }
        const size_t e0 = ev++, e1 = ev++;
        if (!event_at(h, e1)) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
        HIPCHK(hipEventRecord(h->events[e0], h->stream));
        launch();
        HIPCHK(hipEventRecord(h->events[e1], h->stream));
        list->push_back({e0, e1});
        return RTW_OK;
    }
};

// The wavefront form's path pool and hit records.
struct wave_pool {
    paths_t A, B;  // ping-pong for compaction
    fresh_t FR;
    double* ht;
    int32_t* hid;
    uint32_t size;
};

// One pass of the wavefront form: fill the pool, then per iteration the plan's
// fused k_segment or the k_intersect / k_shade pair and a refill (k_regen)
// or, once the sample queue is drained, a compaction; ends when a status
// snapshot shows the pool empty.
int wavefront_pass(handle_t* h, const plan_t& plan, const job_t& J, const call_pass& pass, wave_pool& W, call_events& E,
                   rtw_stats& stats) {
    hipStream_t st = h->stream;
    ctrs_t* C = static_cast<ctrs_t*>(h->ctrs.p);
    const int grid = h->grid;
    const int regen_grid = (int)((W.size + kRegenSlots - 1) / kRegenSlots);
    const int check_every = 4;
    const uint32_t n0 = pass.fill;
    int rc;
    // the refill: camera rays of the image's rows, or of the call's pixel list
    const auto regen = [&] {
#if !RTW_STRICT_RADIANCE
        if (plan.c.rays) hipLaunchKernelGGL(k_regen_rays, dim3(regen_grid), dim3(kBlock), 0, st, J, W.A, W.FR, C);
        else
#endif
        if (plan.c.active) hipLaunchKernelGGL(k_regen_active, dim3(regen_grid), dim3(kBlock), 0, st, J, W.A, W.FR, C);
        else hipLaunchKernelGGL(k_regen, dim3(regen_grid), dim3(kBlock), 0, st, J, W.A, W.FR, C);
    };
    hipLaunchKernelGGL(k_fill, dim3((n0 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, W.A, C, n0);
    regen();
    HIPCHK(hipGetLastError());
    bool tail = false;
    std::vector<size_t> checks;  // event slots of status copies, with their copy index
    for (uint64_t it = 0;; ++it) {
        if (it > pass.iter_cap) return rtw_fail(RTW_ERR_HIP, "wavefront did not drain (internal error)");
        if (plan.c.form == kform::segment) {
            rc = E.timed(E.time_isect, [&] {
                launch(plan.fn, grid, kBlock, plan.shm, st, h->S, J, W.A, W.FR, C, h->scene_base, h->facts.shade_bytes);
            });
            if (rc) return rc;
        } else {
            rc = E.timed(E.time_isect, [&] { launch_intersect(plan, grid, st, h->S, W.A, W.FR, W.ht, W.hid, C); });
            if (rc) return rc;
            rc = E.timed(E.time_shade, [&] {
                launch_shade(plan, grid, st, h->S, J, W.A, W.FR, W.ht, W.hid, C, h->scene_base, h->facts.shade_bytes);
            });
            if (rc) return rc;
        }
        if (!tail) regen();
        HIPCHK(hipGetLastError());
        stats.launches_intersect++;
        stats.iterations++;
        if (tail) {
            hipLaunchKernelGGL(k_compact, dim3(grid), dim3(kBlock), 0, st, W.A, W.B, C);
            hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, st, C);
            HIPCHK(hipGetLastError());
            std::swap(W.A, W.B);
        }
        if (it % check_every == check_every - 1) {
            // status snapshot; decide from the previous snapshot so the GPU
            // keeps `check_every` iterations of queued work
            const size_t slot = checks.size() % 64;
            HIPCHK(hipMemcpyAsync(&h->host_ctrs[slot], C, sizeof(ctrs_t), hipMemcpyDeviceToHost, st));
            const size_t e = E.ev++;
            if (!event_at(h, e)) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
            HIPCHK(hipEventRecord(h->events[e], st));
            checks.push_back(e);
            const size_t idx = checks.size() >= 2 ? checks.size() - 2 : 0;
            HIPCHK(hipEventSynchronize(h->events[checks[idx]]));
            const ctrs_t snap = h->host_ctrs[idx % 64];
            if (queue_drained(snap, J.total)) tail = true;
            if (tail && snap.n == 0) break;
        }
    }
    return RTW_OK;
}

// Every buffer of a planned call (render_plan.h call_bytes).
int ensure_buffers(handle_t* h, const call_bytes& b, bool moments) {
    int rc;
    if ((rc = h->pool[0].ensure(b.pool))) return rc;
    if ((rc = h->pool[1].ensure(b.pool))) return rc;
    if ((rc = h->fresh.ensure(b.fresh))) return rc;
    if ((rc = h->hits.ensure(b.hits))) return rc;
    if ((rc = h->radiance.ensure(b.radiance))) return rc;
    if ((rc = h->run.ensure(b.run))) return rc;
    if ((rc = h->run2.ensure(b.run2))) return rc;
    if ((rc = h->camera.ensure(b.camera))) return rc;
    if ((rc = h->flog.ensure(b.flog))) return rc;
    if ((rc = h->accum.ensure(b.staging))) return rc;
    if (moments && (rc = h->accum_sq.ensure(b.staging))) return rc;
    if ((rc = h->alist.ensure(b.list))) return rc;
    if ((rc = h->counts.ensure(b.counts))) return rc;
    return RTW_OK;
}

// The job of a planned call on this handle's buffers, without the pass's
// fields (set_pass).
job_t make_job(const handle_t* h, const call_plan& P, const rtw_render_params& R) {
    job_t J;
    J.cam = static_cast<const rtw_camera_desc*>(h->camera.p);
    J.seed_mix = P.seed_mix;
    J.cam_pin = P.cam_pin;
    J.npix = (uint32_t)P.npix;
    J.nx = R.nx, J.ny = R.ny, J.row_begin = R.row_begin, J.row_step = P.row_step;
    J.div_npix = P.div_npix;
    J.div_nx = P.div_nx;
    J.max_depth = R.max_depth;
    J.L = static_cast<double*>(h->radiance.p);
#if RTW_STRICT_RADIANCE
    J.flog_threads = P.flog_threads;
    J.flog = static_cast<double*>(h->flog.p);
#endif
    return J;
}
// ... of an active call: the device list where the rows were (job_active_list)
void set_job_active_list(job_t& J, const uint32_t* list_dev) {
    std::memcpy(&J.row_begin, &list_dev, sizeof list_dev);
}
// ... of a radiance query: the ray records over cam, the caller's stream
// states (or null) where the rows were, the first key over nx (job_rays,
// job_ray_rng, job_first_key)
void set_job_rays(job_t& J, const rtw_query_ray* rays_dev, const uint32_t* rng_dev, uint32_t first_key) {
    std::memcpy(&J.cam, &rays_dev, sizeof rays_dev);
    std::memcpy(&J.row_begin, &rng_dev, sizeof rng_dev);
    std::memcpy(&J.nx, &first_key, sizeof first_key);
}
void set_pass(job_t& J, const call_pass& p) {
    J.total = p.total;
    J.spp_pass = p.spp_pass;
    J.div_spp = p.div_spp;
    J.s_begin = p.s_begin;
}

// The fp32 kernels' arguments but the job (a fast render; else zeros).
fast_args make_fast_args(const handle_t* h, const call_plan& P) {
    fast_args FA{};
    if (!P.fast) return FA;
    FA.S = h->F32;
    FA.C = static_cast<ctrs_t*>(h->ctrs.p);
    const call_cam32& c = P.cam32;
    for (int k = 0; k < 3; ++k) {
        FA.cam.origin[k] = c.origin[k], FA.cam.lower_left[k] = c.lower_left[k];
        FA.cam.horizontal[k] = c.horizontal[k], FA.cam.vertical[k] = c.vertical[k];
        FA.cam.u[k] = c.u[k], FA.cam.v[k] = c.v[k];
    }
    FA.cam.time0 = c.time0, FA.cam.dtime = c.dtime, FA.cam.lens_radius = c.lens_radius;
    return FA;
}

// The ordered per-pixel reduction of one pass's records into run (k_reduce),
// or with run2 into both sums from one read of each record (k_reduce_moments).
void launch_reduce(hipStream_t st, bool f32, const double* L, uint64_t npix, uint32_t S_pass, double* run, double* run2) {
    const dim3 g(reduce_grid(npix)), b(kBlock);
    const float* Lf = reinterpret_cast<const float*>(L);
    if (run2) {
        if (f32) hipLaunchKernelGGL(k_reduce_moments<float>, g, b, 0, st, Lf, (uint32_t)npix, S_pass, run, run2);
        else hipLaunchKernelGGL(k_reduce_moments<double>, g, b, 0, st, L, (uint32_t)npix, S_pass, run, run2);
    } else {
        if (f32) hipLaunchKernelGGL(k_reduce<float>, g, b, 0, st, Lf, (uint32_t)npix, S_pass, run);
        else hipLaunchKernelGGL(k_reduce<double>, g, b, 0, st, L, (uint32_t)npix, S_pass, run);
    }
}

// acc += sums (the caller's accumulator: through `staging` when it is host memory)
int emit(hipStream_t st, const call_plan& P, const rtw_render_params& R, double* acc, const double* sums,
         const dev_buf& staging) {
    double* acc_dev = acc;
    const size_t img_bytes = P.bytes.staging;
    if (!R.accum_on_device) {
        acc_dev = static_cast<double*>(staging.p);
        HIPCHK(hipMemcpyAsync(acc_dev, acc, img_bytes, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_emit, dim3(std::min<uint64_t>((P.npix + kBlock - 1) / kBlock, 4096)), dim3(kBlock), 0, st, sums,
                       (uint32_t)P.npix, R.nx, R.row_begin, P.row_step, acc_dev);
    HIPCHK(hipGetLastError());
    if (!R.accum_on_device) HIPCHK(hipMemcpyAsync(acc, acc_dev, img_bytes, hipMemcpyDeviceToHost, st));
    return RTW_OK;
}

// An active call's pixel list and counts (rtw_render_accumulate_active).
struct active_call {
    const uint32_t* list = nullptr;  // the caller's, host or device as accum_on_device says
    uint64_t n = 0;
    uint32_t* counts = nullptr;      // may be null
    bool checked = false;            // a device list the library's own select just wrote: no k_check_active
};

// An active call's emit: acc[list[k]] += sums[k], the same for the squares,
// counts[list[k]] += spp, each where its pointer is set (sums null: the counts
// alone).  Host buffers go through whole-image device copies as emit()'s do;
// only the listed pixels change in them.
int emit_active(handle_t* h, const rtw_render_params& R, const active_call& act, const uint32_t* list_dev, uint32_t spp,
                double* acc, const double* sums, double* acc_sq, const double* sums_sq) {
    hipStream_t st = h->stream;
    const size_t img = (size_t)R.nx * R.ny * 24, cnt = img / 6;
    double *acc_dev = sums ? acc : nullptr, *sq_dev = sums_sq ? acc_sq : nullptr;
    uint32_t* counts_dev = act.counts;
    if (!R.accum_on_device) {
        if (sums) {
            if (int rc = h->accum.ensure(img)) return rc;
            acc_dev = static_cast<double*>(h->accum.p);
            HIPCHK(hipMemcpyAsync(acc_dev, acc, img, hipMemcpyHostToDevice, st));
        }
        if (sums_sq) {
            if (int rc = h->accum_sq.ensure(img)) return rc;
            sq_dev = static_cast<double*>(h->accum_sq.p);
            HIPCHK(hipMemcpyAsync(sq_dev, acc_sq, img, hipMemcpyHostToDevice, st));
        }
        if (act.counts) {
            if (int rc = h->counts.ensure(cnt)) return rc;
            counts_dev = static_cast<uint32_t*>(h->counts.p);
            HIPCHK(hipMemcpyAsync(counts_dev, act.counts, cnt, hipMemcpyHostToDevice, st));
        }
    }
    hipLaunchKernelGGL(k_emit_active, dim3(reduce_grid(act.n)), dim3(kBlock), 0, st, sums, sums_sq, (uint32_t)act.n,
                       list_dev, spp, acc_dev, sq_dev, counts_dev);
    HIPCHK(hipGetLastError());
    if (!R.accum_on_device) {
        if (sums) HIPCHK(hipMemcpyAsync(acc, acc_dev, img, hipMemcpyDeviceToHost, st));
        if (sums_sq) HIPCHK(hipMemcpyAsync(acc_sq, sq_dev, img, hipMemcpyDeviceToHost, st));
        if (act.counts) HIPCHK(hipMemcpyAsync(act.counts, counts_dev, cnt, hipMemcpyDeviceToHost, st));
    }
    return RTW_OK;
}

// The list of an active call on the device, checked: a host list is checked
// on the host (adaptive.cpp) and copied to the handle's buffer, a device list
// by k_check_active.  A list that is not strictly ascending or reaches past
// the image is refused here, before any render launch.
int active_list_device(handle_t* h, const rtw_render_params& R, const active_call& act, const uint32_t** out) {
    hipStream_t st = h->stream;
    const uint64_t limit = (uint64_t)R.nx * (uint64_t)R.ny;
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof a);
    const bool known = hipPointerGetAttributes(&a, act.list) == hipSuccess;
    if (!known) (void)hipGetLastError();
    if (!R.accum_on_device) {
        if (known && a.type == hipMemoryTypeDevice)
            return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: a device pixel list with host buffers "
                                             "(accum_on_device covers the list too)");
        if (int rc = rtw_adaptive_check_list("rtw_render_accumulate_active", act.list, act.n, limit)) return rc;
        if (int rc = h->alist.ensure(act.n * 4)) return rc;
        HIPCHK(hipMemcpyAsync(h->alist.p, act.list, act.n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));  // (the caller's list may go after the call)
        *out = static_cast<const uint32_t*>(h->alist.p);
        return RTW_OK;
    }
    if (act.checked) {  // (rtw_render_adaptive: k_select_scatter's list is strictly ascending and in range)
        *out = act.list;
        return RTW_OK;
    }
    if (int rc = rtw_check_device_ptr(act.list, h->device, "rtw_render_accumulate_active")) return rc;
    if (int rc = h->sel.ensure(sizeof(uint32_t) * (2 * kSelectMaxGrid + 2))) return rc;
    uint32_t* bad = static_cast<uint32_t*>(h->sel.p);
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_check_active, dim3(reduce_grid(act.n)), dim3(kBlock), 0, st, act.list, (uint32_t)act.n,
                       (uint32_t)limit, bad);
    HIPCHK(hipGetLastError());
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, bad, sizeof flag, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (flag)
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: the device pixel list is not strictly ascending "
                                         "or reaches past the image");
    *out = act.list;
    return RTW_OK;
}

// The profiling builds' reports of a finished call (RTW_PROF, RTW_PROF_WALK;
// nothing in the product build).
int print_profile(const rtw_stats& stats) {
#ifdef RTW_PROF_WALK
    {
        static unsigned long long w[32][64];
        HIPCHK(hipMemcpyFromSymbol(w, HIP_SYMBOL(g_walk), sizeof w));
        std::fprintf(stderr, "[rtw walk] sampled clock by media-walk position:");
        for (int k = 0; k < 32; ++k) {
            unsigned long long t = 0;
            for (int l = 0; l < 64; ++l) t += w[k][l];
            if (t) std::fprintf(stderr, " %d:%llu", k, t);
        }
        std::fprintf(stderr, "\n");
    }
#endif
#ifdef RTW_PROF
    {
        unsigned long long pr[PS_N];
        HIPCHK(hipMemcpyFromSymbol(pr, HIP_SYMBOL(g_prof), sizeof pr));
        static const char* names[PS_N] = {"loop", "load", "traverse", "hit+material", "sample", "pdf", "store"};
        double tot = 0;
        for (int k = 0; k < PS_N; ++k) tot += (double)pr[k];
        std::fprintf(stderr, "[rtw prof] lane-cycles per segment:");
        for (int k = 0; k < PS_N; ++k)
            std::fprintf(stderr, " %s %.0f (%.1f%%)", names[k], (double)pr[k] / std::max<double>(1, stats.segments),
                         100.0 * pr[k] / std::max(1.0, tot));
        std::fprintf(stderr, "\n");
        std::memset(pr, 0, sizeof pr);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), pr, sizeof pr));
        unsigned long long cl[2][8];
        HIPCHK(hipMemcpyFromSymbol(cl, HIP_SYMBOL(g_cls), sizeof cl));
        static const char* cn[8] = {"miss", "lambertian", "metal", "dielectric", "light", "isotropic", "-", "idle"};
        std::fprintf(stderr, "[rtw prof] segment classes (lane share / share of wave-iterations where present):");
        double lt = 0, wt = 0;
        for (int k = 0; k < 8; ++k) lt += (double)cl[0][k];
        wt = (double)(cl[1][0] + 0);  // every wave-iteration has some class; use max as the iteration count
        for (int k = 0; k < 8; ++k) wt = std::max(wt, (double)cl[1][k]);
        unsigned long long it = 0;
        for (int k = 0; k < 8; ++k) it = std::max(it, cl[1][k]);
        std::fprintf(stderr, " (wave-iterations >= %llu)", it);
        for (int k = 0; k < 8; ++k)
            if (cl[0][k]) std::fprintf(stderr, " %s %.3f/%.3f", cn[k], cl[0][k] / lt, cl[1][k] / wt);
        std::fprintf(stderr, "\n");
        std::memset(cl, 0, sizeof cl);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_cls), cl, sizeof cl));
    }
#endif
    (void)stats;
    return RTW_OK;
}

}  // namespace

// The render of rtw_render_accumulate and, with accum_sq set, of
// rtw_render_accumulate_moments (rtw_noise.h): the same launches, allocations
// and copies, except that k_reduce_moments takes k_reduce's place and a
// second k_emit adds the sums of squares.  With accum_sq null nothing here
// differs from the plain render.
// act (rtw_render_accumulate_active, rtw_adaptive.h; null: a whole-image
// call, which launches exactly what it launched before this path existed):
// the samples of the listed pixels.  The list takes the rows' place in the
// plan and the job, the kernel is a row of the active lists or a wavefront
// form refilled by k_regen_active (rtw_select.h select_active), the passes and
// the ordered reduction run over n_active pixels, and the emit scatters.
static int render_accumulate(handle_t* h, const rtw_camera_desc* camera, const rtw_render_params* prm,
                             double* accum_rgb, double* accum_sq, rtw_stats* out_stats,
                             const active_call* act = nullptr) {
    const rtw_render_params& R = *prm;
    // the call's plan: refusals, sizes, cameras and job fields (render_plan.h)
    call_plan P;
    const call_active plan_act{act ? act->n : 0, act ? act->list : nullptr, act ? act->counts : nullptr};
    if (int rc = rtw_plan_call(R, *camera, h->facts, accum_rgb, accum_sq, pass_budget_samples(),
                               RTW_STRICT_RADIANCE ? h->cus : 0, &P, act ? &plan_act : nullptr))
        return rc;
    if (act && RTW_STRICT_RADIANCE)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build renders whole images only "
                                             "(rtw_render_accumulate_active)");
    HIPCHK(hipSetDevice(h->device));
    if (R.accum_on_device) {
        if (int rc = rtw_check_device_ptr(accum_rgb, h->device, "rtw_render_accumulate")) return rc;
        if (accum_sq)
            if (int rc = rtw_check_device_ptr(accum_sq, h->device, "rtw_render_accumulate_moments")) return rc;
        if (act && act->counts)
            if (int rc = rtw_check_device_ptr(act->counts, h->device, "rtw_render_accumulate_active")) return rc;
    }
    hipStream_t st = h->stream;
    rtw_stats stats;
    std::memset(&stats, 0, sizeof stats);
    const uint32_t* list_dev = nullptr;
    if (act && act->n)
        if (int rc = active_list_device(h, R, *act, &list_dev)) return rc;
    if (P.noop) {
        stats.samples = P.samples;
        // (max_depth <= 0: every sample adds zero radiance, and still counts)
        if (act && act->n && P.spp_count && act->counts) {
            if (int rc = emit_active(h, R, *act, list_dev, (uint32_t)P.spp_count, nullptr, nullptr, nullptr, nullptr))
                return rc;
            HIPCHK(hipStreamSynchronize(st));
        }
        if (out_stats) *out_stats = stats;
        return RTW_OK;
    }

    // execution form: persistent (paths in registers, one launch per pass)
    // unless RTW_MODE=wavefront or no persistent instantiation covers the
    // scene (rtw_select.h; planning launches nothing); the strict build
    // refuses the other forms here, before any allocation or launch
    // fp32 fast mode: its own persistent kernel (rtw_fast.h), same passes,
    // radiance records and ordered per-pixel reduction
    if (P.fast && !fast_image_ok(h))
        return rtw_fail(RTW_ERR_UNSUPPORTED, "precision fp32 with image textures covers list and world-BVH scenes only "
                                             "(this scene has media or group BVHs): render it in fp64");
    if (act && P.fast && !active_fp32_ok(scene_facts(h, P.pin)))
        return rtw_fail(RTW_ERR_UNSUPPORTED, "rtw_render_accumulate_active: precision fp32 of a scene with image "
                                             "textures has no active kernel: render it in fp64");
    plan_t plan;
    if (int rc = plan_render(h, P.pin, P.fast, &plan, act != nullptr)) return rc;
    const bool persistent = plan.c.persistent();
    if (RTW_STRICT_RADIANCE && !persistent)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build renders with the persistent kernel only "
                                             "(RTW_MODE=wavefront or a scene without a persistent instantiation)");

    if (int rc = ensure_buffers(h, P.bytes, accum_sq != nullptr)) return rc;
    wave_pool W{rtw_carve_paths<paths_t>(h->pool[0].p, P.pool), rtw_carve_paths<paths_t>(h->pool[1].p, P.pool),
                rtw_carve_fresh<fresh_t>(h->fresh.p, P.pool), static_cast<double*>(h->hits.p),
                reinterpret_cast<int32_t*>(static_cast<char*>(h->hits.p) + P.hits_id_off), P.pool};
    ctrs_t* C = static_cast<ctrs_t*>(h->ctrs.p);
    double* run = static_cast<double*>(h->run.p);
    double* run2 = accum_sq ? static_cast<double*>(h->run2.p) : nullptr;
    HIPCHK(hipMemsetAsync(run, 0, P.bytes.run, st));
    if (run2) HIPCHK(hipMemsetAsync(run2, 0, P.bytes.run2, st));
    HIPCHK(hipMemsetAsync(C, 0, sizeof(ctrs_t), st));

    // the camera (cam_host lives until the copy ran) and, after it, the
    // device's own reciprocals of nx and ny
    h->cam_host = P.cam_dev;
    HIPCHK(hipMemcpyAsync(h->camera.p, &h->cam_host, sizeof(rtw_camera_desc), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_recips, dim3(1), dim3(64), 0, st,
                       reinterpret_cast<double*>(static_cast<char*>(h->camera.p) + sizeof(rtw_camera_desc)), R.nx, R.ny);
    HIPCHK(hipGetLastError());

    call_events E(h, R.collect_kernel_times);
    hipEvent_t ev_begin = event_at(h, E.ev++), ev_end = event_at(h, E.ev++);
    if (!ev_begin || !ev_end) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
    HIPCHK(hipEventRecord(ev_begin, st));
    job_t J = make_job(h, P, R);
    if (act) set_job_active_list(J, list_dev);
    fast_args FA = make_fast_args(h, P);
    for (uint64_t done = 0; done < (uint64_t)P.spp_count; done += P.pass_spp) {
        const call_pass pass = rtw_plan_pass(P, R, done);
        set_pass(J, pass);
        if (persistent) {
            hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, st, W.A, C, 0u);  // reset the queue
            FA.J = J;
            if (int rc = E.timed(E.time_isect, [&] { launch_persistent(plan, h, st, J, C, FA); })) return rc;
            HIPCHK(hipGetLastError());
            stats.launches_intersect++;
            stats.iterations++;
        } else if (int rc = wavefront_pass(h, plan, J, pass, W, E, stats)) {
            return rc;
        }
        launch_reduce(st, P.fast, J.L, P.npix, pass.spp_pass, run, run2);  // (the wavefront form is fp64 only)
        HIPCHK(hipGetLastError());
        stats.samples += J.total;
    }

    if (act) {
        if (int rc = emit_active(h, R, *act, list_dev, (uint32_t)P.spp_count, accum_rgb, run, accum_sq, run2)) return rc;
    } else {
        if (int rc = emit(st, P, R, accum_rgb, run, h->accum)) return rc;
        if (accum_sq)
            if (int rc = emit(st, P, R, accum_sq, run2, h->accum_sq)) return rc;
    }
    HIPCHK(hipMemcpyAsync(&h->host_ctrs[63], C, sizeof(ctrs_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ev_end, st));
    HIPCHK(hipStreamSynchronize(st));

    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev_begin, ev_end));
    stats.ms_total = ms;
    for (int k = 0; k < 8; ++k) stats.segments += h->host_ctrs[63].segments[k].v;
    for (auto& p : E.isect_ev) {
        HIPCHK(hipEventElapsedTime(&ms, h->events[p.first], h->events[p.second]));
        stats.ms_intersect += ms;
    }
    for (auto& p : E.shade_ev) {
        HIPCHK(hipEventElapsedTime(&ms, h->events[p.first], h->events[p.second]));
        stats.ms_shade += ms;
    }
    if (int rc = print_profile(stats)) return rc;
    // algorithmic traversal bytes: 56 B ray in +
    // 12 B hit out per world query, whatever the execution form (k_persist
    // keeps both in registers; k_segment / k_intersect stream them)
    // (fp32 fast mode: 7 x 4 B ray in, 4 + 4 B hit out = 36 B)
    stats.bytes_intersect = (P.fast ? 36.0 : 68.0) * (double)stats.segments;
    if (out_stats) *out_stats = stats;
    return RTW_OK;
}

extern "C" int rtw_render_accumulate(void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                                     double* accum_rgb, rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !camera || !prm || !accum_rgb) return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate: null argument");
    return render_accumulate(h, camera, prm, accum_rgb, nullptr, out_stats);
}

extern "C" int rtw_render_accumulate_moments(void* handle, const rtw_camera_desc* camera,
                                             const rtw_render_params* prm, double* accum_rgb, double* accum_sq_rgb,
                                             rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !camera || !prm || !accum_rgb || !accum_sq_rgb)
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_moments: null argument");
    return render_accumulate(h, camera, prm, accum_rgb, accum_sq_rgb, out_stats);
}

// k_noise_pixels over an image's moments, then the summary: the blocks'
// partials copied out and merged in block order (returns when the kernel has
// ended).
static int estimate_device(handle_t* h, const double* accum, const double* accum_sq, rtw_count_src cnt, uint64_t npix,
                           double floor, double* stderr_dev, rtw_noise_summary* out) {
    const unsigned grid = noise_grid(npix);
    if (int rc = h->noise.ensure(sizeof(rtw_noise_acc) * kNoiseMaxGrid)) return rc;
    rtw_noise_acc* parts = static_cast<rtw_noise_acc*>(h->noise.p);
    hipLaunchKernelGGL(k_noise_pixels, dim3(grid), dim3(kBlock), 0, h->stream, accum, accum_sq, cnt, npix, 3.0 * floor,
                       stderr_dev, parts);
    HIPCHK(hipGetLastError());
    std::vector<rtw_noise_acc> host(grid);
    HIPCHK(hipMemcpyAsync(host.data(), parts, sizeof(rtw_noise_acc) * grid, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (out) {
        rtw_noise_acc t = host[0];
        for (unsigned b = 1; b < grid; ++b) t.merge(host[b]);
        rtw_noise_finish(t, out);
    }
    return RTW_OK;
}

extern "C" int rtw_noise_estimate_device(void* handle, const double* accum, const double* accum_sq, int nx, int ny,
                                         int n, double floor, double* stderr_dev, rtw_noise_summary* out) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_noise_estimate_device";
    if (!h) return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": null scene handle");
    if (int rc = rtw_noise_check_args(what, accum, accum_sq, nx, ny, n, floor, stderr_dev)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {accum, accum_sq, stderr_dev})) return rc;
    return estimate_device(h, accum, accum_sq, rtw_count_src{nullptr, (uint32_t)n}, (uint64_t)nx * (uint64_t)ny, floor,
                           stderr_dev, out);
}

// ======================================================================
// rtw_adaptive.h
// ======================================================================
extern "C" int rtw_render_accumulate_active(void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                                            const uint32_t* active, uint64_t n_active, double* accum_rgb,
                                            double* accum_sq_rgb, uint32_t* counts, rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !camera || !prm || !accum_rgb || (n_active && !active))
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: null argument");
    const active_call act{active, n_active, counts};
    return render_accumulate(h, camera, prm, accum_rgb, accum_sq_rgb, out_stats, &act);
}

extern "C" int rtw_scene_query_active(void* handle, int precision, char name[128]) {
    const handle_t* h = static_cast<const handle_t*>(handle);
    if (!h || !name) return rtw_fail(RTW_ERR_INVALID, "rtw_scene_query_active: null argument");
    if (precision != RTW_PRECISION_FP64 && precision != RTW_PRECISION_FP32)
        return rtw_fail(RTW_ERR_INVALID, "rtw_scene_query_active: unknown precision");
    const bool fast = precision == RTW_PRECISION_FP32;
    if (RTW_STRICT_RADIANCE)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build renders whole images only");
    if (fast && !active_fp32_ok(scene_facts(h, h->facts.desc_pin)))
        return rtw_fail(RTW_ERR_UNSUPPORTED, "rtw_scene_query_active: precision fp32 of a scene with image textures has "
                                             "no active kernel");
    HIPCHK(hipSetDevice(h->device));  // occupancy queries of the plan
    plan_t p;
    if (int rc = plan_render(h, h->facts.desc_pin, fast, &p, true)) return rc;
    std::snprintf(name, 128, "%s", p.c.name.c_str());
    return RTW_OK;
}

// The select's three launches into active_dev; the length lands in *n_out
// when the stream has run them (the caller synchronises).
static int launch_select(handle_t* h, const double* accum, const double* accum_sq, const uint32_t* counts, uint64_t npix,
                         double floor, double target_rel, uint32_t max_count, uint32_t* active_dev, uint32_t* n_out) {
    if (int rc = h->sel.ensure(sizeof(uint32_t) * (2 * kSelectMaxGrid + 2))) return rc;
    uint32_t* block_counts = static_cast<uint32_t*>(h->sel.p) + 1;  // ([0]: the list check's flag)
    uint32_t* offsets = block_counts + kSelectMaxGrid;
    const unsigned grid = select_grid(npix);
    const select_args A{accum, accum_sq, rtw_count_src{counts, 0}, npix, select_chunk(npix), 3.0 * floor, target_rel,
                        max_count};
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(k_select_count, dim3(grid), dim3(kBlock), 0, st, A, block_counts);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(kBlock), 0, st, block_counts, (uint32_t)grid, offsets);
    hipLaunchKernelGGL(k_select_scatter, dim3(grid), dim3(kBlock), 0, st, A, offsets, active_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n_out, offsets + grid, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return RTW_OK;
}

extern "C" int rtw_adaptive_select_device(void* handle, const double* accum, const double* accum_sq,
                                          const uint32_t* counts, int nx, int ny, double floor, double target_rel,
                                          uint32_t max_count, uint32_t* active_dev, uint64_t* n_active_host) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_adaptive_select_device";
    if (!h) return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": null scene handle");
    if (int rc = rtw_adaptive_check_select(what, accum, accum_sq, counts, nx, ny, floor, target_rel, active_dev,
                                           n_active_host))
        return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {accum, accum_sq, counts, active_dev})) return rc;
    uint32_t n = 0;
    if (int rc = launch_select(h, accum, accum_sq, counts, (uint64_t)nx * (uint64_t)ny, floor, target_rel, max_count,
                               active_dev, &n))
        return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_active_host = n;
    return RTW_OK;
}

// rtw_adaptive_window.h's select: the two bit-plane kernels, then the count,
// scan and scatter over the window bit; *n_out as launch_select leaves it.
static int launch_select_window(handle_t* h, const double* accum, const double* accum_sq, const uint32_t* counts, int nx,
                                int ny, double floor, double target_rel, uint32_t min_count, uint32_t max_count,
                                int radius, uint32_t* active_dev, uint32_t* n_out) {
    const uint64_t npix = (uint64_t)nx * (uint64_t)ny;
    window_planes P{nullptr, nullptr, nullptr, (uint32_t)nx, (uint32_t)ny, ((uint32_t)nx + 63u) / 64u};
    const uint64_t words = P.words();
    if (int rc = h->sel.ensure(sizeof(uint32_t) * (2 * kSelectMaxGrid + 2))) return rc;
    if (int rc = h->wbits.ensure(3 * words * sizeof(uint64_t))) return rc;
    P.src = static_cast<uint64_t*>(h->wbits.p), P.fin = P.src + words, P.out = P.fin + words;
    uint32_t* block_counts = static_cast<uint32_t*>(h->sel.p) + 1;  // ([0]: the list check's flag)
    uint32_t* offsets = block_counts + kSelectMaxGrid;
    const unsigned grid = select_grid(npix);
    const unsigned grid_src = (unsigned)std::min<uint64_t>((words + kWaves - 1) / kWaves, kBitsMaxGrid);
    const unsigned grid_dil = (unsigned)std::min<uint64_t>((words + kBlock - 1) / kBlock, kBitsMaxGrid);
    const window_args A{P.out, counts, npix, select_chunk(npix), P.nx, P.W, min_count, max_count};
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(k_source_bits, dim3(grid_src), dim3(kBlock), 0, st, accum, accum_sq, counts, P, 3.0 * floor,
                       target_rel);
    hipLaunchKernelGGL(k_dilate_bits, dim3(grid_dil), dim3(kBlock), 0, st, P, radius);
    hipLaunchKernelGGL(k_window_count, dim3(grid), dim3(kBlock), 0, st, A, block_counts);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(kBlock), 0, st, block_counts, (uint32_t)grid, offsets);
    hipLaunchKernelGGL(k_window_scatter, dim3(grid), dim3(kBlock), 0, st, A, offsets, active_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n_out, offsets + grid, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return RTW_OK;
}

extern "C" int rtw_adaptive_select_window_device(void* handle, const double* accum, const double* accum_sq,
                                                 const uint32_t* counts, int nx, int ny, double floor,
                                                 double target_rel, uint32_t min_count, uint32_t max_count, int radius,
                                                 uint32_t* active_dev, uint64_t* n_active_host) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_adaptive_select_window_device";
    if (!h) return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": null scene handle");
    if (int rc = rtw_adaptive_window_check_select(what, accum, accum_sq, counts, nx, ny, floor, target_rel, min_count,
                                                  max_count, radius, active_dev, n_active_host))
        return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {accum, accum_sq, counts, active_dev})) return rc;
    uint32_t n = 0;
    if (int rc = launch_select_window(h, accum, accum_sq, counts, nx, ny, floor, target_rel, min_count, max_count,
                                      radius, active_dev, &n))
        return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_active_host = n;
    return RTW_OK;
}

extern "C" int rtw_noise_estimate_counts_device(void* handle, const double* accum, const double* accum_sq,
                                                const uint32_t* counts, int nx, int ny, double floor,
                                                double* stderr_dev, rtw_noise_summary* out) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_noise_estimate_counts_device";
    if (!h) return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": null scene handle");
    if (int rc = rtw_adaptive_check_estimate(what, accum, accum_sq, counts, nx, ny, floor, stderr_dev)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {accum, accum_sq, counts, stderr_dev})) return rc;
    return estimate_device(h, accum, accum_sq, rtw_count_src{counts, 0}, (uint64_t)nx * (uint64_t)ny, floor, stderr_dev,
                           out);
}

extern "C" int rtw_finalize_canvas_counts_device(void* handle, const double* accum, const uint32_t* counts, int nx,
                                                 int ny, double* canvas) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_finalize_canvas_counts_device";
    if (!h || !accum || !counts || !canvas || nx <= 0 || ny <= 0)
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": bad argument");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {accum, counts, canvas})) return rc;
    return launch_finalize(h, accum, nx, ny, rtw_div_counts{counts}, canvas);
}

static void add_stats(rtw_stats& t, const rtw_stats& s) {
    t.samples += s.samples, t.segments += s.segments, t.iterations += s.iterations;
    t.launches_intersect += s.launches_intersect;
    t.ms_total += s.ms_total, t.ms_intersect += s.ms_intersect, t.ms_shade += s.ms_shade;
    t.ms_finalize += s.ms_finalize, t.bytes_intersect += s.bytes_intersect;
}

// The adaptive loop: the schedule is rtw_adaptive_next_round (adaptive.cpp),
// the rounds are this file's own render, select and estimate on device
// buffers -- the caller's, or the handle's when the caller's are host memory
// (copied out once at the end).
// One body for both entry points: radius < 0 is rtw_render_adaptive (a later
// round selects with launch_select), radius >= 0 rtw_render_adaptive_window
// (launch_select_window with min_count = done).
static int adaptive_loop(const char* what, void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                         const rtw_adaptive_params* ap, int radius, double* accum_rgb, double* accum_sq_rgb,
                         uint32_t* counts, rtw_adaptive_result* out_result, rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !camera || !prm || !accum_rgb || !accum_sq_rgb || !counts)
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": null argument");
    if (int rc = rtw_adaptive_check_params(what, ap)) return rc;
    if (RTW_STRICT_RADIANCE)
        return rtw_fail(RTW_ERR_UNSUPPORTED,
                        std::string("the strict-radiance build renders whole images only (") + what + ")");
    if (prm->nx <= 0 || prm->ny <= 0 || (uint64_t)prm->nx * (uint64_t)prm->ny >= (1ull << 31))
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": bad image size");
    const uint64_t npix = (uint64_t)prm->nx * (uint64_t)prm->ny;
    const size_t img = npix * 24, cnt = npix * 4;
    if (rtw_ranges_overlap(accum_rgb, accum_sq_rgb, img) || rtw_spans_overlap(counts, cnt, accum_rgb, img) ||
        rtw_spans_overlap(counts, cnt, accum_sq_rgb, img))
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": two of the buffers overlap");
    HIPCHK(hipSetDevice(h->device));
    const bool on_device = prm->accum_on_device != 0;
    double *a_dev = accum_rgb, *q_dev = accum_sq_rgb;
    uint32_t* c_dev = counts;
    if (on_device) {
        if (int rc = check_handle_ptrs(h, what, {accum_rgb, accum_sq_rgb, counts})) return rc;
    } else {
        if (int rc = h->accum.ensure(img)) return rc;
        if (int rc = h->accum_sq.ensure(img)) return rc;
        if (int rc = h->counts.ensure(cnt)) return rc;
        a_dev = static_cast<double*>(h->accum.p), q_dev = static_cast<double*>(h->accum_sq.p);
        c_dev = static_cast<uint32_t*>(h->counts.p);
    }
    if (int rc = h->alist.ensure(cnt)) return rc;
    uint32_t* list = static_cast<uint32_t*>(h->alist.p);
    hipStream_t st = h->stream;
    HIPCHK(hipMemsetAsync(a_dev, 0, img, st));
    HIPCHK(hipMemsetAsync(q_dev, 0, img, st));

    rtw_render_params R = *prm;  // every round renders on the device buffers
    R.spp = ap->max_spp, R.row_begin = 0, R.row_step = 1, R.accum_on_device = 1;
    rtw_stats total, s;
    std::memset(&total, 0, sizeof total);
    rtw_adaptive_result res;
    std::memset(&res, 0, sizeof res);
    int done = 0;
    for (;;) {
        int begin = 0, count = 0;
        if (int rc = rtw_adaptive_next_round(ap, done, &begin, &count)) return rc;
        if (count == 0) break;
        R.spp_begin = begin, R.spp_count = count;
        if (done == 0) {
            // round 0: every pixel, through the whole-image render
            if (int rc = render_accumulate(h, camera, &R, a_dev, q_dev, &s)) return rc;
            hipLaunchKernelGGL(k_set_counts, dim3(grid_for(npix)), dim3(kBlock), 0, st, c_dev, (size_t)npix,
                               (uint32_t)count);
            HIPCHK(hipGetLastError());
        } else {
            uint32_t n = 0;
            if (int rc = radius < 0 ? launch_select(h, a_dev, q_dev, c_dev, npix, ap->floor, ap->target_rel,
                                                    (uint32_t)ap->max_spp, list, &n)
                                    : launch_select_window(h, a_dev, q_dev, c_dev, prm->nx, prm->ny, ap->floor,
                                                           ap->target_rel, (uint32_t)done, (uint32_t)ap->max_spp,
                                                           radius, list, &n))
                return rc;
            HIPCHK(hipStreamSynchronize(st));
            if (n == 0) break;
            const active_call act{list, n, c_dev, true};
            if (int rc = render_accumulate(h, camera, &R, a_dev, q_dev, &s, &act)) return rc;
        }
        add_stats(total, s);
        done += count;
        ++res.rounds;
    }
    // the summary is the estimate of the buffers the caller gets back: the
    // device estimator's for device buffers, the host's for host buffers
    if (on_device)
        if (int rc = estimate_device(h, a_dev, q_dev, rtw_count_src{c_dev, 0}, npix, ap->floor, nullptr, &res.final))
            return rc;
    std::vector<uint32_t> c_host;
    uint32_t* c_read = counts;
    if (on_device) {
        c_host.resize(npix);
        c_read = c_host.data();
    } else {
        HIPCHK(hipMemcpyAsync(accum_rgb, a_dev, img, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(accum_sq_rgb, q_dev, img, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(c_read, c_dev, cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!on_device)
        if (int rc = rtw_noise_estimate_counts(accum_rgb, accum_sq_rgb, counts, prm->nx, prm->ny, ap->floor, nullptr,
                                               &res.final))
            return rc;
    for (uint64_t p = 0; p < npix; ++p) {
        res.samples += c_read[p];
        res.pixels_at_max += c_read[p] == (uint32_t)ap->max_spp ? 1 : 0;
    }
    if (out_result) *out_result = res;
    if (out_stats) *out_stats = total;
    return RTW_OK;
}

extern "C" int rtw_render_adaptive(void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                                   const rtw_adaptive_params* ap, double* accum_rgb, double* accum_sq_rgb,
                                   uint32_t* counts, rtw_adaptive_result* out_result, rtw_stats* out_stats) {
    return adaptive_loop("rtw_render_adaptive", handle, camera, prm, ap, -1, accum_rgb, accum_sq_rgb, counts,
                         out_result, out_stats);
}

// rtw_adaptive_window.h
extern "C" int rtw_render_adaptive_window(void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                                          const rtw_adaptive_params* ap, int radius, double* accum_rgb,
                                          double* accum_sq_rgb, uint32_t* counts, rtw_adaptive_result* out_result,
                                          rtw_stats* out_stats) {
    const char* const what = "rtw_render_adaptive_window";
    if (int rc = rtw_adaptive_window_check_radius(what, radius)) return rc;
    return adaptive_loop(what, handle, camera, prm, ap, radius, accum_rgb, accum_sq_rgb, counts, out_result, out_stats);
}

// ======================================================================
// rtw_denoise.h
// ======================================================================
#if !RTW_STRICT_RADIANCE
namespace {
// k_features<f> of every entry of kIntersectList: its traversal feature sets
template <size_t... I>
std::array<const void*, sizeof...(I)> feature_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_features<kIntersectList[I].f>)...};
}
const auto kFeatureRows = feature_rows(std::make_index_sequence<kIntersectList.size()>{});
}  // namespace
#endif

// The traversal feature set of the handle's k_features, chosen as the split
// pair's k_intersect is (rtw_select.h split_resolve).
static inst features_inst(const handle_t* h) {
    return split_resolve(inst{h->facts.features & (F_MEDIA | F_WBVH | F_GBVH), SF_IMG_ALL, false}).intersect;
}

extern "C" int rtw_scene_query_features(void* handle, char name[128]) {
    const handle_t* h = static_cast<const handle_t*>(handle);
    if (!h || !name) return rtw_fail(RTW_ERR_INVALID, "rtw_scene_query_features: null argument");
    if (RTW_STRICT_RADIANCE)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build has no feature kernel (rtw_render_features)");
    std::snprintf(name, 128, "%s", kname("k_features", features_inst(h).f, -1).c_str());
    return RTW_OK;
}

extern "C" int rtw_render_features(void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                                   double* features, rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !camera || !prm || !features) return rtw_fail(RTW_ERR_INVALID, "rtw_render_features: null argument");
#if RTW_STRICT_RADIANCE
    return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build has no feature kernel (rtw_render_features)");
#else
    // the render's plan of the same call: its refusals, sample and row ranges,
    // passes (pass-local sample ids are 32-bit), camera and job fields.
    // Precision and depth are not read: planned as one fp64 segment per sample.
    rtw_render_params R = *prm;
    R.precision = RTW_PRECISION_FP64, R.max_depth = 1;
    call_plan P;
    if (int rc = rtw_plan_call(R, *camera, h->facts, features, nullptr, pass_budget_samples(), 0, &P)) return rc;
    HIPCHK(hipSetDevice(h->device));
    rtw_stats stats;
    std::memset(&stats, 0, sizeof stats);
    if (P.noop) {
        if (out_stats) *out_stats = stats;
        return RTW_OK;
    }
    const size_t img = (size_t)R.nx * R.ny * RTW_FEATURE_CHANNELS * sizeof(double);
    hipStream_t st = h->stream;
    double* f_dev = features;
    if (R.accum_on_device) {
        if (int rc = rtw_check_device_ptr(features, h->device, "rtw_render_features")) return rc;
        if (reinterpret_cast<uintptr_t>(features) % 16)
            return rtw_fail(RTW_ERR_INVALID, "rtw_render_features: a device feature buffer must be 16-byte aligned");
    } else {
        if (int rc = h->features.ensure(img)) return rc;
        f_dev = static_cast<double*>(h->features.p);
        HIPCHK(hipMemcpyAsync(f_dev, features, img, hipMemcpyHostToDevice, st));
    }
    if (int rc = h->camera.ensure(P.bytes.camera)) return rc;
    h->cam_host = P.cam_dev;
    HIPCHK(hipMemcpyAsync(h->camera.p, &h->cam_host, sizeof(rtw_camera_desc), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_recips, dim3(1), dim3(64), 0, st,
                       reinterpret_cast<double*>(static_cast<char*>(h->camera.p) + sizeof(rtw_camera_desc)), R.nx, R.ny);
    HIPCHK(hipGetLastError());
    const int at = index_of(kIntersectList, features_inst(h));
    if (at < 0) return rtw_fail(RTW_ERR_HIP, "no such instantiation: k_features");
    hipEvent_t ev_begin = event_at(h, 0), ev_end = event_at(h, 1);
    if (!ev_begin || !ev_end) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
    HIPCHK(hipEventRecord(ev_begin, st));
    job_t J = make_job(h, P, R);
    J.L = nullptr;
    const int grid = (int)std::min<uint64_t>((P.npix + kBlock - 1) / kBlock, (uint64_t)h->grid);
    for (uint64_t done = 0; done < (uint64_t)P.spp_count; done += P.pass_spp) {
        set_pass(J, rtw_plan_pass(P, R, done));
        launch(kFeatureRows[at], grid, kBlock, 0, st, h->S, J, f_dev);
        HIPCHK(hipGetLastError());
        stats.samples += J.total;
        stats.launches_intersect++;
    }
    HIPCHK(hipEventRecord(ev_end, st));
    if (!R.accum_on_device) HIPCHK(hipMemcpyAsync(features, f_dev, img, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev_begin, ev_end));
    stats.ms_total = ms;
    stats.segments = stats.samples;
    stats.bytes_intersect = 68.0 * (double)stats.segments;
    if (out_stats) *out_stats = stats;
    return RTW_OK;
#endif
}

extern "C" int rtw_denoise_device(void* handle, const double* accum, const double* accum_sq, const uint32_t* counts,
                                  int n, const double* features, int feature_spp, int nx, int ny,
                                  const rtw_denoise_params* prm, double* out, double* out_var) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_denoise_device";
    if (!h) return rtw_fail(RTW_ERR_INVALID, "rtw_denoise_device: null scene handle");
    if (int rc = rtw_denoise_check_args(what, accum, accum_sq, counts, n, features, feature_spp, nx, ny, prm, out, out_var))
        return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {accum, accum_sq, counts, features, out, out_var})) return rc;
    const uint64_t npix = (uint64_t)nx * (uint64_t)ny;
    const rtw_count_src cnt{counts, (uint32_t)n};
    const dim3 grid((unsigned)((npix + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = h->stream;
    if (prm->iterations == 0) {
        hipLaunchKernelGGL(k_denoise_mean, grid, block, 0, st, accum, accum_sq, cnt, npix, out, out_var);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return RTW_OK;
    }
    for (dev_buf& b : h->dn_state)
        if (int rc = b.ensure(npix * sizeof(rtw_dn_state))) return rc;
    if (int rc = h->dn_geo.ensure(npix * sizeof(rtw_dn_geo))) return rc;
    if (int rc = h->dn_alb.ensure(npix * sizeof(rtw_dn_alb))) return rc;
    rtw_dn_state* a = static_cast<rtw_dn_state*>(h->dn_state[0].p);
    rtw_dn_state* b = static_cast<rtw_dn_state*>(h->dn_state[1].p);
    rtw_dn_geo* geo = static_cast<rtw_dn_geo*>(h->dn_geo.p);
    rtw_dn_alb* alb = static_cast<rtw_dn_alb*>(h->dn_alb.p);
    // Steps 1 and 2 run the LDS-tile form, the sparser steps the global form: measured at 800x800 on one MI355X,
    // 0.106 against 0.322 ms at step 1 and 0.127 against 0.318 ms at step 2 (profiles/denoise/results.txt); from
    // step 4 on a tile's halo no longer fits.  RTW_DENOISE_TIMES=1 prints each launch's milliseconds (events around
    // every launch: how that file was measured).
    const char* tm = std::getenv("RTW_DENOISE_TIMES");
    const bool times = tm && *tm && std::atoi(tm) != 0;
    size_t ev = 0;
    const auto mark = [&]() -> int {
        if (!times) return RTW_OK;
        hipEvent_t e = event_at(h, ev++);
        if (!e) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
        HIPCHK(hipEventRecord(e, st));
        return RTW_OK;
    };
    if (int rc = mark()) return rc;
    hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, st, accum, accum_sq, cnt, features, (double)feature_spp,
                       prm->eps_a, npix, a, geo, alb);
    if (int rc = mark()) return rc;
    const dim3 tgrid((unsigned)((nx + kTileX - 1) / kTileX), (unsigned)((ny + kTileY - 1) / kTileY));
    for (int k = 0; k < prm->iterations; ++k) {
        if (k == 0)
            hipLaunchKernelGGL(k_atrous_tile<1>, tgrid, block, tile_bytes(1), st, a, geo, alb, nx, ny, prm->sigma_l,
                               prm->sigma_z, prm->normal_power_log2, b);
        else if (k == 1)
            hipLaunchKernelGGL(k_atrous_tile<2>, tgrid, block, tile_bytes(2), st, a, geo, alb, nx, ny, prm->sigma_l,
                               prm->sigma_z, prm->normal_power_log2, b);
        else
            hipLaunchKernelGGL(k_atrous, grid, block, 0, st, a, geo, alb, nx, ny, 1 << k, prm->sigma_l, prm->sigma_z,
                               prm->normal_power_log2, b);
        if (int rc = mark()) return rc;
        std::swap(a, b);
    }
    hipLaunchKernelGGL(k_denoise_finish, grid, block, 0, st, a, alb, npix, out, out_var);
    if (int rc = mark()) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (times) {
        std::fprintf(stderr, "[rtw denoise] %dx%d ms: prepare", nx, ny);
        float total = 0.f;
        for (size_t k = 0; k + 1 < ev; ++k) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, h->events[k], h->events[k + 1]));
            total += ms;
            if (k == 0) std::fprintf(stderr, " %.4f", ms);
            else if (k + 2 == ev) std::fprintf(stderr, " finish %.4f", ms);
            else std::fprintf(stderr, " step%d %.4f", 1 << (k - 1), ms);
        }
        std::fprintf(stderr, " total %.4f\n", total);
    }
    return RTW_OK;
}

extern "C" int rtw_finalize_canvas_mean_device(void* handle, const double* mean, int nx, int ny, double* canvas) {
    handle_t* h = static_cast<handle_t*>(handle);
    const char* const what = "rtw_finalize_canvas_mean_device";
    if (!h || !mean || !canvas || nx <= 0 || ny <= 0) return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": bad argument");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = check_handle_ptrs(h, what, {mean, canvas})) return rc;
    return launch_finalize(h, mean, nx, ny, rtw_div_none{}, canvas);
}

// ======================================================================
// rtw_query.h
// ======================================================================
#if !RTW_STRICT_RADIANCE
namespace {
// k_query<f> and k_occluded<f> of every entry of kIntersectList (its traversal feature sets)
template <size_t... I>
std::array<const void*, sizeof...(I)> query_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_query<kIntersectList[I].f>)...};
}
template <size_t... I>
std::array<const void*, sizeof...(I)> occluded_rows(std::index_sequence<I...>) {
    return {reinterpret_cast<const void*>(&k_occluded<kIntersectList[I].f>)...};
}
const auto kQueryRows = query_rows(std::make_index_sequence<kIntersectList.size()>{});
const auto kOccludedRows = occluded_rows(std::make_index_sequence<kIntersectList.size()>{});

// The trace of a checked, non-empty call.  flags: rtw_trace_occluded.
int query_trace(handle_t* h, const char* what, const rtw_query_ray* rays, uint64_t n, uint32_t* rng,
                const rtw_query_params* prm, void* out, bool flags, rtw_stats* stats) {
    const inst in = features_inst(h);
    const int at = index_of(kIntersectList, in);
    if (at < 0) return rtw_fail(RTW_ERR_HIP, "no such instantiation: k_query");
    const bool media = (in.f & F_MEDIA) != 0;
    if (!media) rng = nullptr;  // never touched
    const size_t stride = flags ? 1 : sizeof(rtw_query_hit);
    HIPCHK(hipSetDevice(h->device));
    if (prm->on_device)
        if (int rc = check_handle_ptrs(h, what, {rays, rng, out})) return rc;
    const query_plan P = rtw_query_plan(n, !prm->on_device, stride, media);
    if (int rc = h->q_rays.ensure(P.bytes_rays)) return rc;
    if (int rc = h->q_out.ensure(P.bytes_out)) return rc;
    if (int rc = h->q_rng.ensure(P.bytes_rng)) return rc;
    hipStream_t st = h->stream;
    uint32_t* bad = nullptr;
    if (h->facts.bvh_motion) {
        if (int rc = h->q_bad.ensure(16)) return rc;
        bad = static_cast<uint32_t*>(h->q_bad.p);
        HIPCHK(hipMemsetAsync(bad, 0, 4, st));
    }
    hipEvent_t ev_begin = event_at(h, 0), ev_end = event_at(h, 1);
    if (!ev_begin || !ev_end) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
    HIPCHK(hipEventRecord(ev_begin, st));
    const void* fn = flags ? kOccludedRows[at] : kQueryRows[at];
    for (uint64_t c = 0; c < P.n_chunks; ++c) {
        const query_span ch = rtw_query_chunk(P, c);
        // the chunk's buffers on the device: the caller's, or the staged copies
        const rtw_query_ray* r_dev = rays + ch.first;
        uint32_t* g_dev = rng ? rng + ch.first : nullptr;
        char* o_dev = static_cast<char*>(out) + ch.first * stride;
        if (P.staged) {
            r_dev = static_cast<const rtw_query_ray*>(h->q_rays.p);
            o_dev = static_cast<char*>(h->q_out.p);
            HIPCHK(hipMemcpyAsync(h->q_rays.p, rays + ch.first, ch.count * sizeof(rtw_query_ray), hipMemcpyHostToDevice, st));
            if (rng) {
                g_dev = static_cast<uint32_t*>(h->q_rng.p);
                HIPCHK(hipMemcpyAsync(g_dev, rng + ch.first, ch.count * 4, hipMemcpyHostToDevice, st));
            }
        }
        for (uint64_t l = 0, nl = rtw_query_launches(P, ch); l < nl; ++l) {
            const query_span ls = rtw_query_launch(P, ch, l);
            const uint64_t rel = ls.first - ch.first;
            query_args Q{};
            Q.rays = r_dev + rel;
            Q.rng = g_dev ? g_dev + rel : nullptr;
            Q.n = (uint32_t)ls.count;
            Q.check = bad ? 1u : 0u;
            Q.sh0 = h->facts.shutter0, Q.sh1 = h->facts.shutter1;
            Q.bad = bad;
            const int grid = (int)std::min<uint64_t>((ls.count + kBlock - 1) / kBlock, (uint64_t)h->grid);
            if (flags)
                launch(fn, grid, kBlock, 0, st, h->S, Q, reinterpret_cast<uint8_t*>(o_dev + rel * stride));
            else
                launch(fn, grid, kBlock, 0, st, h->S, Q, reinterpret_cast<rtw_query_hit*>(o_dev + rel * stride));
            HIPCHK(hipGetLastError());
            stats->launches_intersect++;
        }
        if (P.staged) {
            HIPCHK(hipMemcpyAsync(static_cast<char*>(out) + ch.first * stride, o_dev, ch.count * stride, hipMemcpyDeviceToHost, st));
            if (rng) HIPCHK(hipMemcpyAsync(rng + ch.first, g_dev, ch.count * 4, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipEventRecord(ev_end, st));
    uint32_t n_bad = 0;
    if (bad) HIPCHK(hipMemcpyAsync(&n_bad, bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev_begin, ev_end));
    stats->ms_total = ms;
    stats->samples = stats->segments = n;
    stats->bytes_intersect = 68.0 * (double)n;
    if (n_bad)
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": " + std::to_string(n_bad) +
                                             " rays have a time outside the shutter the scene's BVH was built for "
                                             "(moving spheres)");
    return RTW_OK;
}
}  // namespace
#endif

static int query_entry(const char* what, void* handle, const rtw_query_ray* rays, uint64_t n, uint32_t* rng,
                       const rtw_query_params* prm, void* out, bool flags, rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    // (the strict build refuses before it reads the handle)
    const bool media = !RTW_STRICT_RADIANCE && h && (h->facts.features & F_MEDIA) != 0;
    if (int rc = rtw_query_check_args(what, h, rays, n, rng, prm, out, flags ? 1 : sizeof(rtw_query_hit), media,
                                      RTW_STRICT_RADIANCE != 0))
        return rc;
    rtw_stats stats;
    std::memset(&stats, 0, sizeof stats);
    int rc = RTW_OK;
#if !RTW_STRICT_RADIANCE
    if (n) rc = query_trace(h, what, rays, n, rng, prm, out, flags, &stats);
#endif
    if (!rc && out_stats) *out_stats = stats;
    return rc;
}

extern "C" int rtw_trace_closest(void* handle, const rtw_query_ray* rays, uint64_t n, uint32_t* rng,
                                 const rtw_query_params* prm, rtw_query_hit* hits, rtw_stats* out_stats) {
    return query_entry("rtw_trace_closest", handle, rays, n, rng, prm, hits, false, out_stats);
}

extern "C" int rtw_trace_occluded(void* handle, const rtw_query_ray* rays, uint64_t n, uint32_t* rng,
                                  const rtw_query_params* prm, uint8_t* occluded, rtw_stats* out_stats) {
    return query_entry("rtw_trace_occluded", handle, rays, n, rng, prm, occluded, true, out_stats);
}

extern "C" int rtw_scene_query_trace(void* handle, char closest[128], char occluded[128]) {
    const handle_t* h = static_cast<const handle_t*>(handle);
    if (!h || !closest || !occluded) return rtw_fail(RTW_ERR_INVALID, "rtw_scene_query_trace: null argument");
    if (RTW_STRICT_RADIANCE)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build has no query kernels (rtw_trace_closest)");
    const int f = features_inst(h).f;
    std::snprintf(closest, 128, "%s", kname("k_query", f, -1).c_str());
    std::snprintf(occluded, 128, "%s", kname("k_occluded", f, -1).c_str());
    return RTW_OK;
}

extern "C" int rtw_camera_rays(void* handle, const rtw_camera_desc* camera, const rtw_render_params* prm,
                               rtw_query_ray* rays, uint32_t* rng_out, uint64_t capacity) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (!h || !camera || !prm) return rtw_fail(RTW_ERR_INVALID, "rtw_camera_rays: null argument");
#if RTW_STRICT_RADIANCE
    return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build has no query kernels (rtw_camera_rays)");
#else
    // the render's plan of the same call (as rtw_render_features): its
    // refusals, sample and row ranges, camera and job fields; one pass holds
    // the whole call, so q is the index the header states
    rtw_render_params R = *prm;
    R.precision = RTW_PRECISION_FP64, R.max_depth = 1;
    call_plan P;
    if (int rc = rtw_plan_call(R, *camera, h->facts, rays, nullptr, pass_budget_samples(), 0, &P)) return rc;
    const uint64_t total = (uint64_t)P.spp_count * P.npix;
    if (int rc = rtw_query_check_camera_args(rays, rng_out, capacity, total, R.accum_on_device != 0)) return rc;
    if (total == 0) return RTW_OK;
    HIPCHK(hipSetDevice(h->device));
    if (R.accum_on_device)
        if (int rc = check_handle_ptrs(h, "rtw_camera_rays", {rays, rng_out})) return rc;
    P.pass_spp = (uint64_t)P.spp_count;
    hipStream_t st = h->stream;
    if (int rc = h->camera.ensure(P.bytes.camera)) return rc;
    h->cam_host = P.cam_dev;
    HIPCHK(hipMemcpyAsync(h->camera.p, &h->cam_host, sizeof(rtw_camera_desc), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_recips, dim3(1), dim3(64), 0, st,
                       reinterpret_cast<double*>(static_cast<char*>(h->camera.p) + sizeof(rtw_camera_desc)), R.nx, R.ny);
    HIPCHK(hipGetLastError());
    job_t J = make_job(h, P, R);
    J.L = nullptr;
    set_pass(J, rtw_plan_pass(P, R, 0));
    const query_plan Q = rtw_query_plan(total, !R.accum_on_device, 0, rng_out != nullptr);
    if (int rc = h->q_rays.ensure(Q.bytes_rays)) return rc;
    if (int rc = h->q_rng.ensure(Q.bytes_rng)) return rc;
    for (uint64_t c = 0; c < Q.n_chunks; ++c) {
        const query_span ch = rtw_query_chunk(Q, c);
        rtw_query_ray* r_dev = Q.staged ? static_cast<rtw_query_ray*>(h->q_rays.p) : rays + ch.first;
        uint32_t* g_dev = !rng_out ? nullptr : Q.staged ? static_cast<uint32_t*>(h->q_rng.p) : rng_out + ch.first;
        for (uint64_t l = 0, nl = rtw_query_launches(Q, ch); l < nl; ++l) {
            const query_span ls = rtw_query_launch(Q, ch, l);
            const uint64_t rel = ls.first - ch.first;
            const int grid = (int)std::min<uint64_t>((ls.count + kBlock - 1) / kBlock, (uint64_t)h->grid);
            hipLaunchKernelGGL(k_camera_rays, dim3(grid), dim3(kBlock), 0, st, J, (uint32_t)ls.first, (uint32_t)ls.count,
                               r_dev + rel, g_dev ? g_dev + rel : nullptr);
            HIPCHK(hipGetLastError());
        }
        if (Q.staged) {
            HIPCHK(hipMemcpyAsync(rays + ch.first, r_dev, ch.count * sizeof(rtw_query_ray), hipMemcpyDeviceToHost, st));
            if (rng_out) HIPCHK(hipMemcpyAsync(rng_out + ch.first, g_dev, ch.count * 4, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return RTW_OK;
#endif
}

// ======================================================================
// rtw_radiance.h
// ======================================================================
#if !RTW_STRICT_RADIANCE
namespace {
// The trace of a checked call.  Per chunk (radiance.h): the rays (and states,
// and sums) on the device, the shutter check where the scene needs it, the
// chunk's passes through the plan's kernel exactly as render_accumulate runs a
// render's, k_reduce per pass into the chunk's zeroed sums, and k_add into the
// caller's.
int radiance_trace(handle_t* h, const rtw_query_ray* rays, uint64_t n, const uint32_t* rng,
                   const rtw_radiance_params& prm, double* sum_rgb, rtw_stats* stats) {
    const char* const what = "rtw_trace_radiance";
    const radiance_plan P = rtw_radiance_plan(n, prm, rng != nullptr, pass_budget_samples());
    stats->samples = P.samples;
    if (n == 0) return RTW_OK;
    HIPCHK(hipSetDevice(h->device));
    if (prm.on_device)  // (before the max_depth == 0 no-op: a foreign pointer is refused whatever the depth)
        if (int rc = check_handle_ptrs(h, what, {rays, rng, sum_rgb})) return rc;
    if (P.noop) return RTW_OK;
    plan_t plan;
    if (int rc = plan_rays(h, &plan)) return rc;
    const bool persistent = plan.c.persistent();
    if (int rc = h->q_rays.ensure(P.bytes_rays)) return rc;
    if (int rc = h->q_out.ensure(P.bytes_sums)) return rc;
    if (int rc = h->q_rng.ensure(P.bytes_rng)) return rc;
    hipStream_t st = h->stream;
    uint32_t* bad = nullptr;
    if (h->facts.bvh_motion) {
        if (int rc = h->q_bad.ensure(16)) return rc;
        bad = static_cast<uint32_t*>(h->q_bad.p);
    }
    ctrs_t* C = static_cast<ctrs_t*>(h->ctrs.p);
    HIPCHK(hipMemsetAsync(C, 0, sizeof(ctrs_t), st));
    call_events E(h, 0);
    hipEvent_t ev_begin = event_at(h, E.ev++), ev_end = event_at(h, E.ev++);
    if (!ev_begin || !ev_end) return rtw_fail(RTW_ERR_HIP, "hipEventCreate failed");
    HIPCHK(hipEventRecord(ev_begin, st));
    const fast_args FA{};
    for (uint64_t c = 0; c < P.n_chunks; ++c) {
        radiance_chunk ch;
        if (int rc = rtw_radiance_chunk(P, c, &ch)) return rc;
        const call_plan& CP = ch.call;
        if (int rc = ensure_buffers(h, CP.bytes, false)) return rc;
        // the chunk's buffers on the device: the caller's, or the staged copies
        const rtw_query_ray* r_dev = rays + ch.first;
        const uint32_t* g_dev = rng ? rng + ch.first : nullptr;
        double* s_dev = sum_rgb + 3 * ch.first;
        if (P.staged) {
            r_dev = static_cast<const rtw_query_ray*>(h->q_rays.p);
            s_dev = static_cast<double*>(h->q_out.p);
            HIPCHK(hipMemcpyAsync(h->q_rays.p, rays + ch.first, ch.count * sizeof(rtw_query_ray), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(s_dev, sum_rgb + 3 * ch.first, ch.count * 24, hipMemcpyHostToDevice, st));
            if (rng) {
                g_dev = static_cast<const uint32_t*>(h->q_rng.p);
                HIPCHK(hipMemcpyAsync(h->q_rng.p, rng + ch.first, ch.count * 4, hipMemcpyHostToDevice, st));
            }
        }
        if (bad) {  // before the chunk is traced: a time the boxes do not cover could walk anywhere
            uint32_t n_bad = 0;
            HIPCHK(hipMemsetAsync(bad, 0, 4, st));
            hipLaunchKernelGGL(k_check_ray_times, dim3(reduce_grid(ch.count)), dim3(kBlock), 0, st, r_dev,
                               (uint32_t)ch.count, h->facts.shutter0, h->facts.shutter1, bad);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&n_bad, bad, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (n_bad)
                return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": " + std::to_string(n_bad) +
                                                     " rays have a time outside the shutter the scene's BVH was built "
                                                     "for (moving spheres)");
        }
        wave_pool W{rtw_carve_paths<paths_t>(h->pool[0].p, CP.pool), rtw_carve_paths<paths_t>(h->pool[1].p, CP.pool),
                    rtw_carve_fresh<fresh_t>(h->fresh.p, CP.pool), static_cast<double*>(h->hits.p),
                    reinterpret_cast<int32_t*>(static_cast<char*>(h->hits.p) + CP.hits_id_off), CP.pool};
        double* run = static_cast<double*>(h->run.p);
        HIPCHK(hipMemsetAsync(run, 0, CP.bytes.run, st));
        job_t J = make_job(h, CP, ch.R);
        set_job_rays(J, r_dev, g_dev, ch.first_key);
        for (uint64_t done = 0; done < (uint64_t)CP.spp_count; done += CP.pass_spp) {
            const call_pass pass = rtw_plan_pass(CP, ch.R, done);
            set_pass(J, pass);
            if (persistent) {
                hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, st, W.A, C, 0u);  // reset the queue
                launch_persistent(plan, h, st, J, C, FA);
                HIPCHK(hipGetLastError());
                stats->launches_intersect++;
                stats->iterations++;
            } else if (int rc = wavefront_pass(h, plan, J, pass, W, E, *stats)) {
                return rc;
            }
            launch_reduce(st, false, J.L, CP.npix, pass.spp_pass, run, nullptr);
            HIPCHK(hipGetLastError());
        }
        const size_t n3 = (size_t)ch.count * 3;
        hipLaunchKernelGGL(k_add, dim3(grid_for(n3)), dim3(kBlock), 0, st, s_dev, run, n3);
        HIPCHK(hipGetLastError());
        if (P.staged) {
            HIPCHK(hipMemcpyAsync(sum_rgb + 3 * ch.first, s_dev, ch.count * 24, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));  // (the staging buffers are the next chunk's)
        }
    }
    HIPCHK(hipMemcpyAsync(&h->host_ctrs[63], C, sizeof(ctrs_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ev_end, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev_begin, ev_end));
    stats->ms_total = ms;
    for (int k = 0; k < 8; ++k) stats->segments += h->host_ctrs[63].segments[k].v;
    stats->bytes_intersect = 68.0 * (double)stats->segments;
    return RTW_OK;
}
}  // namespace
#endif

extern "C" int rtw_trace_radiance(void* handle, const rtw_query_ray* rays, uint64_t n, const uint32_t* rng,
                                  const rtw_radiance_params* prm, double* sum_rgb, rtw_stats* out_stats) {
    handle_t* h = static_cast<handle_t*>(handle);
    if (int rc = rtw_radiance_check_args(h, rays, n, rng, prm, sum_rgb, RTW_STRICT_RADIANCE != 0)) return rc;
    rtw_stats stats;
    std::memset(&stats, 0, sizeof stats);
    int rc = RTW_OK;
#if !RTW_STRICT_RADIANCE
    rc = radiance_trace(h, rays, n, rng, *prm, sum_rgb, &stats);
#endif
    if (!rc && out_stats) *out_stats = stats;
    return rc;
}

extern "C" int rtw_scene_query_radiance(void* handle, char name[128]) {
    const handle_t* h = static_cast<const handle_t*>(handle);
    if (!h || !name) return rtw_fail(RTW_ERR_INVALID, "rtw_scene_query_radiance: null argument");
    if (RTW_STRICT_RADIANCE)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "the strict-radiance build has no query kernels (rtw_trace_radiance)");
    HIPCHK(hipSetDevice(h->device));  // occupancy queries of the plan
    plan_t p;
    if (int rc = plan_rays(h, &p)) return rc;
    std::snprintf(name, 128, "%s", p.c.name.c_str());
    return RTW_OK;
}
