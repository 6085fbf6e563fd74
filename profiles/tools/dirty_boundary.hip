// dirty_boundary.hip -- what the bytes a kernel leaves dirty in L2 cost at its end: the back-to-back period of the pair
//   A (raster_fwd's grid at config 2, 4 608 x 256; writes N MB, 16 B per lane, each wave instruction eight whole 128-B lines)
//   B (one trivial dependent workgroup that reads one word A wrote)
// in one stream, for N in {0, 8, 16, 32, 64} MB and A's stores plain, nt and sc1 (write-through).  Every workgroup of A also
// spins for SPIN us, so the kernel lasts 20-30 us like the real one: "early" stores first and then spins (the forward's stores sit
// in front of the walkers' chains), "late" spins first and stores last (the worst case: everything is still dirty at the end).
// The figure of interest is period(N) - period(0) per policy: what the end of A pays for N MB.
// Build: hipcc --offload-arch=gfx950 -O3 -o profiles/tools/dirty_boundary.bin profiles/tools/dirty_boundary.hip
// Run:   profiles/tools/dirty_boundary.bin [SPIN_US=10] [LAUNCHES=300]    (profiles/tools/dirty_boundary.sh does both)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
typedef float f4 __attribute__((ext_vector_type(4)));
enum { PLAIN = 0, NT = 1, SC1 = 2 };
static const int NWG = 4608, NT_ = 256, WAVES = NWG * (NT_ / 64);
static const size_t CAP = (size_t)64 << 20;                                    // the buffer: the largest N

template <int POLICY> __device__ __forceinline__ void store16(f4* p, f4 v) {
    if constexpr (POLICY == PLAIN) *p = v;
    else if constexpr (POLICY == NT) __builtin_nontemporal_store(v, p);
    else asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void spin(long long ticks) {                        // wall_clock64 counts 100 MHz on this chip
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(1);
}
// Wave g of the launch (waves of one workgroup 4 608 apart, so every N spreads over all workgroups) writes the 1-KB chunks
// g, g + WAVES, ... < nchunks.  nchunks <= CAP / 1024 is checked on the host, so no store leaves the buffer.
template <int POLICY, bool LATE> __global__ void __launch_bounds__(256) k_a(f4* out, int nchunks, int nwaves, long long ticks, float seed) {
    const int lane = threadIdx.x & 63, g = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
    if (LATE) spin(ticks);
    for (int c = g; c < nchunks; c += nwaves) store16<POLICY>(out + (size_t)c * 64 + lane, f4{seed, (float)c, (float)lane, 1.f});
    if (!LATE) spin(ticks);
}
__global__ void k_b(const float* a, float* out) { out[threadIdx.x] = a[threadIdx.x] + 1.f; }

template <class F> static double median_period_us(F&& pair, int n, hipStream_t s) {
    for (int i = 0; i < 30; ++i) pair(i);
    (void)hipStreamSynchronize(s);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    std::vector<double> v;
    for (int rep = 0; rep < 5; ++rep) {                                          // five batches; the median batch is reported
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < n; ++i) pair(i);
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
        v.push_back(ms * 1e3 / n);
    }
    std::sort(v.begin(), v.end());
    return v[2];
}
template <int POLICY, bool LATE> static double run(f4* buf, float* out, int mb, long long ticks, int n, hipStream_t s) {
    const int nchunks = (int)(((size_t)mb << 20) / 1024);
    if ((size_t)nchunks * 1024 > CAP) { fprintf(stderr, "N too large\n"); exit(2); }
    return median_period_us([&](int i) {
        hipLaunchKernelGGL((k_a<POLICY, LATE>), dim3(NWG), dim3(NT_), 0, s, buf, nchunks, WAVES, ticks, (float)i);
        hipLaunchKernelGGL(k_b, dim3(1), dim3(64), 0, s, (const float*)buf, out);
    }, n, s);
}
int main(int argc, char** argv) {
    const double spin_us = argc > 1 ? atof(argv[1]) : 10.0;
    const int n = argc > 2 ? atoi(argv[2]) : 300;
    hipStream_t s; (void)hipStreamCreate(&s);
    f4* buf; float* out;
    if (hipMalloc(&buf, CAP) != hipSuccess || hipMalloc(&out, 64 * sizeof(float)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    (void)hipMemset(buf, 0, CAP);
    const long long ticks = (long long)(spin_us * 100.0);
    const int mbs[] = {0, 8, 16, 32, 64};
    printf("pair period A(4608x256, writes N MB, spins %.0f us per workgroup) -> B(1x64), us; median of 5 batches of %d pairs\n", spin_us, n);
    printf("%-6s %-6s", "place", "policy");
    for (int mb : mbs) printf(" %8dMB", mb);
    printf("   | minus N=0:");
    for (int mb : mbs) if (mb) printf(" %6dMB", mb);
    printf("\n");
    auto row = [&](const char* place, const char* pol, auto fn) {
        double p[5];
        for (int i = 0; i < 5; ++i) p[i] = fn(mbs[i]);
        printf("%-6s %-6s", place, pol);
        for (int i = 0; i < 5; ++i) printf(" %10.2f", p[i]);
        printf("   |           ");
        for (int i = 1; i < 5; ++i) printf(" %8.2f", p[i] - p[0]);
        printf("\n"); fflush(stdout);
    };
    row("early", "plain", [&](int mb) { return run<PLAIN, false>(buf, out, mb, ticks, n, s); });
    row("early", "nt",    [&](int mb) { return run<NT,    false>(buf, out, mb, ticks, n, s); });
    row("early", "sc1",   [&](int mb) { return run<SC1,   false>(buf, out, mb, ticks, n, s); });
    row("late",  "plain", [&](int mb) { return run<PLAIN, true >(buf, out, mb, ticks, n, s); });
    row("late",  "nt",    [&](int mb) { return run<NT,    true >(buf, out, mb, ticks, n, s); });
    row("late",  "sc1",   [&](int mb) { return run<SC1,   true >(buf, out, mb, ticks, n, s); });
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "device error\n"); return 1; }
    return 0;
}
