// multi.cpp — rtw_render_multi: the render loop of RayTracingWeekend.cpp:
// 211-239 on several GPUs of one node, from ONE host process (the C/C++ host
// of the reference has no MPI / torch.distributed: its loop is a parallel_for).
//
// One host thread per device renders that device's contiguous shard of the
// sample range into a zeroed per-device buffer (rtw_render_accumulate, device
// accumulator); one grouped RCCL reduce (ncclSum, ncclFloat64) over the
// devices' communicators brings the per-pixel sums to the first device, and
// they are added into the caller's accumulator there.  Samples are
// independent (RNG keyed by (seed, pixel, sample)), so this is the only
// exchange: 24 B per pixel per device, 15.4 MB for 800x800 -- about 0.1 ms
// over xGMI, next to renders that take 100 ms or more.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "render_plan.h"
#include "rtw_host_util.h"

namespace {

// Cached per device set: communicators (rank g = devices[g]), one stream and
// one accumulation buffer per device.
struct multi_ctx {
    std::vector<int> devices;
    std::vector<ncclComm_t> comms;
    std::vector<hipStream_t> streams;
    std::vector<double*> parts;
    size_t part_elems = 0;
};

std::mutex g_mu;
std::map<std::vector<int>, multi_ctx*> g_ctx;

int hip_fail(hipError_t e, const char* what) {
    return rtw_fail(RTW_ERR_HIP, std::string("rtw_render_multi: ") + what + ": " + hipGetErrorString(e));
}
int nccl_fail(ncclResult_t r, const char* what) {
    return rtw_fail(RTW_ERR_HIP, std::string("rtw_render_multi: ") + what + ": " + ncclGetErrorString(r));
}

void destroy(multi_ctx* c) {
    for (size_t g = 0; g < c->devices.size(); ++g) {
        hipSetDevice(c->devices[g]);
        if (g < c->streams.size() && c->streams[g]) hipStreamSynchronize(c->streams[g]);
        if (g < c->parts.size() && c->parts[g]) hipFree(c->parts[g]);
        if (g < c->comms.size() && c->comms[g]) ncclCommDestroy(c->comms[g]);
        if (g < c->streams.size() && c->streams[g]) hipStreamDestroy(c->streams[g]);
    }
    delete c;
}

int get_ctx(const std::vector<int>& devs, size_t elems, multi_ctx** out) {
    auto it = g_ctx.find(devs);
    multi_ctx* c = it == g_ctx.end() ? nullptr : it->second;
    if (!c) {
        c = new multi_ctx;
        c->devices = devs;
        c->comms.assign(devs.size(), nullptr);
        c->streams.assign(devs.size(), nullptr);
        c->parts.assign(devs.size(), nullptr);
        const ncclResult_t r = ncclCommInitAll(c->comms.data(), (int)devs.size(), devs.data());
        if (r != ncclSuccess) {
            c->comms.assign(devs.size(), nullptr);
            destroy(c);
            return nccl_fail(r, "ncclCommInitAll");
        }
        for (size_t g = 0; g < devs.size(); ++g) {
            hipError_t e = hipSetDevice(devs[g]);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->streams[g], hipStreamNonBlocking);
            if (e != hipSuccess) {
                destroy(c);
                return hip_fail(e, "stream creation");
            }
        }
        g_ctx[devs] = c;
    }
    if (c->part_elems < elems) {
        for (size_t g = 0; g < devs.size(); ++g) {
            hipSetDevice(devs[g]);
            if (c->parts[g]) hipFree(c->parts[g]);
            c->parts[g] = nullptr;
            const hipError_t e = hipMalloc(&c->parts[g], elems * sizeof(double));
            if (e != hipSuccess) {
                c->part_elems = 0;
                return rtw_fail(RTW_ERR_OOM, "rtw_render_multi: device accumulation buffer: " +
                                                 std::string(hipGetErrorString(e)));
            }
        }
        c->part_elems = elems;
    }
    *out = c;
    return RTW_OK;
}

}  // namespace

extern "C" int rtw_render_multi(int ngpus, void* const* handles, const rtw_camera_desc* camera,
                                const rtw_render_params* params, double* accum_root, rtw_stats* out_stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (ngpus <= 0 || !handles || !camera || !params || !accum_root)
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_multi: bad argument");
    const rtw_render_params& R = *params;
    int count = 0;
    if (int rc = rtw_check_sample_range(R, "rtw_render_multi", "rtw_render_multi: ", &count)) return rc;
    std::vector<int> devs(ngpus);
    for (int g = 0; g < ngpus; ++g) {
        devs[g] = rtw_handle_device(handles[g]);
        if (devs[g] < 0) return rtw_fail(RTW_ERR_INVALID, "rtw_render_multi: null scene handle");
        for (int k = 0; k < g; ++k)
            if (devs[k] == devs[g]) return rtw_fail(RTW_ERR_INVALID, "rtw_render_multi: two handles on one device");
    }
    if (R.precision != RTW_PRECISION_FP64 && R.precision != RTW_PRECISION_FP32)
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_multi: unknown precision");
    if (R.accum_on_device)
        if (int rc = rtw_check_device_ptr(accum_root, devs[0], "rtw_render_multi", ngpus == 1)) return rc;
    const size_t elems = (size_t)R.nx * (size_t)R.ny * 3;

    std::lock_guard<std::mutex> lock(g_mu);  // one multi-render at a time per process
    multi_ctx* c = nullptr;
    if (int rc = get_ctx(devs, elems, &c)) return rc;

    // zero the per-device sums
    for (int g = 0; g < ngpus; ++g) {
        hipError_t e = hipSetDevice(devs[g]);
        if (e == hipSuccess) e = hipMemsetAsync(c->parts[g], 0, elems * sizeof(double), c->streams[g]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->streams[g]);
        if (e != hipSuccess) return hip_fail(e, "zeroing");
    }

    // one host thread per device, each on its contiguous shard of the samples
    std::vector<rtw_stats> st(ngpus);
    std::vector<int> rcs(ngpus, RTW_OK);
    std::vector<std::string> errs(ngpus);
    std::vector<std::thread> workers;
    for (int g = 0; g < ngpus; ++g) {
        const int base = count / ngpus, extra = count % ngpus;
        const int begin = R.spp_begin + g * base + std::min(g, extra);
        const int n = base + (g < extra ? 1 : 0);
        workers.emplace_back([&, g, begin, n]() {
            std::memset(&st[g], 0, sizeof st[g]);
            if (n == 0) return;
            rtw_render_params p = R;
            p.spp_begin = begin;
            p.spp_count = n;
            p.accum_on_device = 1;
            rcs[g] = rtw_render_accumulate(handles[g], camera, &p, c->parts[g], &st[g]);
            if (rcs[g]) errs[g] = rtw_last_error();
        });
    }
    for (auto& w : workers) w.join();
    for (int g = 0; g < ngpus; ++g)
        if (rcs[g]) return rtw_fail(rcs[g], "rtw_render_multi: device " + std::to_string(devs[g]) + ": " + errs[g]);

    // sum the devices' buffers on devs[0] (in place there)
    if (ngpus > 1) {
        ncclResult_t r = ncclGroupStart();
        for (int g = 0; g < ngpus && r == ncclSuccess; ++g)
            r = ncclReduce(c->parts[g], c->parts[g], elems, ncclFloat64, ncclSum, 0, c->comms[g], c->streams[g]);
        const ncclResult_t r2 = ncclGroupEnd();
        if (r != ncclSuccess) return nccl_fail(r, "ncclReduce");
        if (r2 != ncclSuccess) return nccl_fail(r2, "ncclGroupEnd");
        for (int g = 0; g < ngpus; ++g) {
            hipError_t e = hipSetDevice(devs[g]);
            if (e == hipSuccess) e = hipStreamSynchronize(c->streams[g]);
            if (e != hipSuccess) return hip_fail(e, "reduce");
        }
    }

    // accum_root += sums (RayTracingWeekend.cpp:235-239 adds into the pixel's running sum)
    if (R.accum_on_device) {
        if (int rc = rtw_handle_add_device(handles[0], accum_root, c->parts[0], elems)) return rc;
    } else {
        std::vector<double> host(elems);
        hipError_t e = hipSetDevice(devs[0]);
        if (e == hipSuccess) e = hipMemcpy(host.data(), c->parts[0], elems * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "copy to host");
        for (size_t k = 0; k < elems; ++k) accum_root[k] += host[k];
    }

    if (out_stats) {
        rtw_stats s;
        std::memset(&s, 0, sizeof s);
        for (const rtw_stats& x : st) {
            s.samples += x.samples;
            s.segments += x.segments;
            s.iterations += x.iterations;
            s.launches_intersect += x.launches_intersect;
            s.ms_intersect += x.ms_intersect;
            s.ms_shade += x.ms_shade;
            s.bytes_intersect += x.bytes_intersect;
        }
        s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *out_stats = s;
    }
    return RTW_OK;
}

extern "C" void rtw_release_communicators(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto& kv : g_ctx) destroy(kv.second);
    g_ctx.clear();
}
