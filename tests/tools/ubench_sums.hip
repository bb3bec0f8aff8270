// Manual timing of the scan kernels and the gaps kernel of csrc/ansx_sums.h alone: one list of n
// ints, the best of 12 runs per kernel by device events, the last sum and the last gap checked.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o ubench_sums.x tests/tools/ubench_sums.hip && ./ubench_sums.x [n]
#include "../../ans_large_alphabet_amd/csrc/ansx_sums.h"
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t err_ = (x); if (err_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(err_), __LINE__); return 1; } } while (0)
__global__ void k_fill(u32* p, u64 n) { u64 i = (u64)blockIdx.x * 256 + threadIdx.x; if (i < n) p[i] = (u32)(i % 97u); }
int main(int argc, char** argv)
{
    const u64 n = argc > 1 ? strtoull(argv[1], 0, 10) : (1ull << 28);
    const u32 ntiles = (u32)((n + ANSX_SS_TILE - 1) / ANSX_SS_TILE);
    u32 *d, *g, *flag; u64 *offs, *agg;
    CK(hipMalloc(&d, 4 * n + 64)); CK(hipMalloc(&g, 4 * n + 64)); CK(hipMalloc(&flag, 16)); CK(hipMalloc(&offs, 16)); CK(hipMalloc(&agg, 16ull * ntiles));
    const u64 ho[2] = { 0, n };
    CK(hipMemcpy(offs, ho, 16, hipMemcpyHostToDevice));
    hipEvent_t e[5]; for (auto& x : e) CK(hipEventCreate(&x));
    float best[4] = { 1e9f, 1e9f, 1e9f, 1e9f };
    for (int rep = 0; rep < 12; rep++) {
        k_fill<<<(u32)((n + 255) / 256), 256>>>(d, n);
        CK(hipMemset(flag, 0xFF, 16));
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e[0]));
        k_sums_reduce<<<ntiles, ANSX_SS_NT>>>(d, 0, n, offs, 1, agg);
        CK(hipEventRecord(e[1]));
        k_sums_carry<<<1, ANSX_SS_SCAN_NT>>>(agg, agg + ntiles, ntiles);
        CK(hipEventRecord(e[2]));
        k_sums_apply<<<ntiles, ANSX_SS_NT>>>(d, 0, n, offs, 1, agg, agg + ntiles, flag);
        CK(hipEventRecord(e[3]));
        k_gaps<<<ntiles, ANSX_SS_NT>>>(d, g, 0, n, offs, 1, flag);
        CK(hipEventRecord(e[4]));
        CK(hipDeviceSynchronize());
        for (int k = 0; k < 4; k++) { float ms; CK(hipEventElapsedTime(&ms, e[k], e[k + 1])); if (ms < best[k]) best[k] = ms; }
    }
    u32 last, gl; CK(hipMemcpy(&last, d + n - 1, 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(&gl, g + n - 1, 4, hipMemcpyDeviceToHost));
    u64 want = 0; for (u64 i = 0; i < n; i++) want += i % 97u;
    printf("n %llu: reduce %.4f carry %.4f apply %.4f gaps %.4f ms; scan %.4f; last sum %s, last gap %s\n",
        (unsigned long long)n, best[0], best[1], best[2], best[3], best[0] + best[1] + best[2], last == (u32)want ? "ok" : "WRONG",
        gl == (u32)((n - 1) % 97u) ? "ok" : "WRONG");
    return 0;
}
