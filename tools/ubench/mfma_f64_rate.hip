// Microbenchmark: v_mfma_f64_16x16x4_f64 on gfx950.  One wave per SIMD on every CU (and, for the occupancy question, two), each with
// CHAINS independent accumulators that it feeds in turn for `iters` rounds; operands stay in registers, so nothing but the matrix core
// is in the way.  Questions: the issue interval of the instruction (cycles per MFMA per SIMD with enough chains), its dependent latency
// (one chain), and the device's float64 MFMA rate.  Times by HIP events over the whole grid; cycles by s_memtime (100 MHz on this part) are
// not used: the rate is reported in instructions per microsecond per SIMD and in TFLOP/s.
//     hipcc -O3 --offload-arch=gfx950 mfma_f64_rate.hip -o mfma_f64_rate && ./mfma_f64_rate
// (spectra.hip's kernel, DESIGN.md 4.46, issues 2 or 4 independent chains per step.)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int CHAINS>
__global__ __launch_bounds__(256) void k(double* out, int iters) {
    const int lane = threadIdx.x & 63;
    f64x4 acc[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double a = 1e-3 * lane, b = 1.0 - 1e-3 * lane;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
        }
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// a HIP call that fails ends the program: a rate from a time nobody measured is worse than none
#define CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { printf("%s failed: %s\n", #expr, hipGetErrorString(e_)); exit(1); } } while (0)

template <int CHAINS>
void run(double* out, int cus, int waves_per_simd, int iters) {
    const dim3 grid(cus * waves_per_simd), block(256);
    hipEvent_t a, z;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&z));
    hipLaunchKernelGGL(k<CHAINS>, grid, block, 0, 0, out, 16);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(a, 0));
    hipLaunchKernelGGL(k<CHAINS>, grid, block, 0, 0, out, iters);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(z, 0));
    CHECK(hipEventSynchronize(z));
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, a, z));
    CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(z));
    const double per_wave = (double)iters * 8 * CHAINS, simds = 4.0 * cus;
    const double total = per_wave * 4 * grid.x;
    printf("chains %d, waves/SIMD %d: %.3f ms, %.1f MFMA per us per SIMD, %.2f TFLOP/s\n", CHAINS, waves_per_simd, ms,
           total / simds / (ms * 1e3), total * 2048.0 / (ms * 1e-3) / 1e12);
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int cus = prop.multiProcessorCount, iters = 20000;
    printf("%s: %d CUs, %d MHz\n", prop.name, cus, prop.clockRate / 1000);
    double* out = nullptr;
    if (hipMalloc(&out, (size_t)cus * 2 * 256 * sizeof(double)) != hipSuccess) return 1;
    run<1>(out, cus, 1, iters);
    run<2>(out, cus, 1, iters);
    run<4>(out, cus, 1, iters);
    run<8>(out, cus, 1, iters);
    run<4>(out, cus, 2, iters);
    CHECK(hipFree(out));
    return 0;
}
