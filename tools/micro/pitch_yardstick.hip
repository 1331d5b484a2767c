// tools/micro/pitch_yardstick.hip -- development aid of tools/pitch_bench.py: what this part sustains, as measured, for the two
// things WF_HIP_OUT_PITCH is compared with.  Built as a shared library and loaded into the benchmark's own process:
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC pitch_yardstick.hip -o libpitch_yardstick.so
//   yard_fma_ms    the time of `blocks` x 256 threads each issuing iters x 64 x 16 independent float64 FMAs from registers (16
//                  accumulators per lane, no memory traffic), at the pitch kernel's occupancy of four waves per SIMD
//   yard_d2h_ms    the time of one hipMemcpy of `bytes` from device memory to pageable or page-locked host memory
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#define REP 64
__global__ __launch_bounds__(256, 4) void yard_fma_kernel(double *out, int iters, double m, double c)
{
    double a[16];
    for(int i = 0; i < 16; ++i)
        a[i] = (double)threadIdx.x + i;
    for(int it = 0; it < iters; ++it) {
#pragma unroll
        for(int r = 0; r < REP; ++r) {
#pragma unroll
            for(int i = 0; i < 16; ++i)
                asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m), "v"(c));
        }
    }
    double acc = 0.0;
    for(int i = 0; i < 16; ++i)
        acc += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}
extern "C" double yard_fma_per_thread(int iters) { return (double)iters * REP * 16; }
// the best of `reps` timed launches after one warm-up, in ms; negative: a HIP error
extern "C" double yard_fma_ms(int blocks, int iters, int reps)
{
    double *d = nullptr;
    if(hipMalloc(&d, (size_t)blocks * 256 * sizeof(double)) != hipSuccess)
        return -1.0;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    double best = -1.0;
    for(int r = 0; r <= reps; ++r) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(yard_fma_kernel, dim3(blocks), dim3(256), 0, 0, d, iters, 0.5, 0.25);
        hipEventRecord(e1);
        if(hipEventSynchronize(e1) != hipSuccess) {
            best = -1.0;
            break;
        }
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        if(r > 0 && (best < 0.0 || ms < best))
            best = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(d);
    return best;
}
extern "C" double yard_d2h_ms(size_t bytes, int pinned, int reps)
{
    void *d = nullptr, *h = nullptr;
    if(hipMalloc(&d, bytes) != hipSuccess)
        return -1.0;
    hipMemset(d, 1, bytes);
    if(pinned ? hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess : (h = std::malloc(bytes)) == nullptr) {
        hipFree(d);
        return -1.0;
    }
    std::memset(h, 0, bytes);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    double best = -1.0;
    for(int r = 0; r <= reps; ++r) {
        hipDeviceSynchronize();
        hipEventRecord(e0);
        const hipError_t rc = hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        if(rc != hipSuccess) {
            best = -1.0;
            break;
        }
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        if(r > 0 && (best < 0.0 || ms < best))
            best = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if(pinned)
        hipHostFree(h);
    else
        std::free(h);
    hipFree(d);
    return best;
}
