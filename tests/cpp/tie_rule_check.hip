// tie_rule_check.hip — on the card: the kernels' equal-distance rule
// (rtw_device.h rtwd::better, rtw_fast.h rtwf::better) picks the winner of
// the reference's list walk, whatever the visiting order.
//
// hittable_list::hit walks its objects in list order with t_max = the
// closest hit so far; a rect accepts t <= t_max (hittable.h:149-165), a
// sphere t < t_max (sphere.h:46-81).  So among equal distances the last rect
// wins, without a rect the first sphere.  The host walks every list of 1..4
// items with kind in {rect, sphere} and t in {1, 2} that way (340 lists); the
// kernel folds the same items through both better() functions in every
// permutation of the visiting order (up to 24 per list), with arbitrate's
// acceptance t <= h.t and item index = list position, and writes each fold's
// winner to a buffer the host compares.  Test tool (tests/test_gpu_ties.py).
//
//   tie_rule_check   prints "lists <n> folds <m> mismatches fp64 <a> fp32 <b>"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "rtw_fast.h"

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("HIP error %s\n", hipGetErrorString(e)); return 2; } } while (0)

constexpr int kMaxItems = 4, kMaxOrders = 24;

// item k of a list: bit 2k of `code` = sphere (0: rect), bit 2k+1 = t is 2 (0: 1)
struct tie_list {
    int n, code;
};
__host__ __device__ inline bool item_rect(int code, int k) { return ((code >> (2 * k)) & 1) == 0; }
__host__ __device__ inline double item_t(int code, int k) { return ((code >> (2 * k + 1)) & 1) ? 2.0 : 1.0; }

// the `which`-th permutation of 0..n-1 (factorial number system)
__device__ void nth_order(int n, int which, int* order) {
    int pool[kMaxItems] = {0, 1, 2, 3};
    for (int k = 0; k < n; ++k) {
        int f = 1;
        for (int j = 2; j < n - k; ++j) f *= j;
        const int pick = which / f;
        which %= f;
        order[k] = pool[pick];
        for (int j = pick; j < kMaxItems - 1; ++j) pool[j] = pool[j + 1];
    }
}

// out[2 * (list * 24 + order)] = the fp64 fold's winner, [.. + 1] = the fp32
// fold's; -2 where the list has fewer orders
__global__ void k_fold(const tie_list* lists, int n_lists, int* out) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_lists * kMaxOrders) return;
    const tie_list L = lists[tid / kMaxOrders];
    const int which = tid % kMaxOrders;
    int orders = 1;
    for (int j = 2; j <= L.n; ++j) orders *= j;
    if (which >= orders) {
        out[2 * tid] = out[2 * tid + 1] = -2;
        return;
    }
    int order[kMaxItems];
    nth_order(L.n, which, order);
    rtwd::hit_state h{rtwd::kDblMax, -1, false};
    rtwf::fhit f{rtwf::kFltMaxF, -1, false};
    for (int k = 0; k < L.n; ++k) {
        const int i = order[k];
        const bool rl = item_rect(L.code, i);
        const double t = item_t(L.code, i);
        if (t <= h.t && rtwd::better(t, i, rl, h.t, h.prim, h.rect, h.prim != -1)) h.t = t, h.prim = i, h.rect = rl;
        const float tf = (float)t;
        if (tf <= f.t && rtwf::better(tf, i, rl, f)) f.t = tf, f.prim = i, f.rect = rl;
    }
    out[2 * tid] = h.prim;
    out[2 * tid + 1] = f.prim;
}

// hittable_list::hit over the list, in list order
static int list_winner(const tie_list& L) {
    double closest = 1e300;
    int winner = -1;
    for (int i = 0; i < L.n; ++i) {
        const double t = item_t(L.code, i);
        const bool hit = item_rect(L.code, i) ? t <= closest : t < closest;
        if (hit) closest = t, winner = i;
    }
    return winner;
}

int main() {
    std::vector<tie_list> lists;
    for (int n = 1; n <= kMaxItems; ++n)
        for (int code = 0; code < (1 << (2 * n)); ++code) lists.push_back(tie_list{n, code});
    const int n_lists = (int)lists.size(), total = n_lists * kMaxOrders;
    tie_list* dl;
    int* dout;
    CHK(hipMalloc(&dl, n_lists * sizeof(tie_list)));
    CHK(hipMalloc(&dout, 2 * total * sizeof(int)));
    CHK(hipMemcpy(dl, lists.data(), n_lists * sizeof(tie_list), hipMemcpyHostToDevice));
    CHK(hipMemset(dout, 0xff, 2 * total * sizeof(int)));
    hipLaunchKernelGGL(k_fold, dim3((total + 255) / 256), dim3(256), 0, 0, dl, n_lists, dout);
    CHK(hipGetLastError());
    std::vector<int> out(2 * total);
    CHK(hipMemcpy(out.data(), dout, out.size() * sizeof(int), hipMemcpyDeviceToHost));
    int folds = 0, bad64 = 0, bad32 = 0;
    for (int l = 0; l < n_lists; ++l) {
        const int want = list_winner(lists[l]);
        int orders = 1;
        for (int j = 2; j <= lists[l].n; ++j) orders *= j;
        for (int w = 0; w < kMaxOrders; ++w) {
            const int g64 = out[2 * (l * kMaxOrders + w)], g32 = out[2 * (l * kMaxOrders + w) + 1];
            if (w >= orders) {
                if (g64 != -2 || g32 != -2) ++bad64, ++bad32;
                continue;
            }
            ++folds;
            if ((g64 != want || g32 != want) && bad64 + bad32 < 8)
                std::printf("list n=%d code=%d order %d: want %d, fp64 %d, fp32 %d\n", lists[l].n, lists[l].code, w, want,
                            g64, g32);
            bad64 += g64 != want;
            bad32 += g32 != want;
        }
    }
    std::printf("lists %d folds %d mismatches fp64 %d fp32 %d\n", n_lists, folds, bad64, bad32);
    CHK(hipFree(dl));
    CHK(hipFree(dout));
    return bad64 || bad32 ? 1 : 0;
}
