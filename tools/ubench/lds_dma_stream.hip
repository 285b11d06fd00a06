// Microbenchmark (round 8): what an LDS-direct weight stream delivers per CU.  One workgroup of eight waves on every CU streams one 4.3 MB blob
// (the three weight runs of features.15-17; every workgroup reads the same bytes, so they come from L2) into an LDS double buffer with
// `buffer_load_dwordx4 ... lds`: 1 KiB per wave-instruction, lane-linear image, no staging registers.  A round = every wave issues N pieces into the
// half the round before last has left, then waits with a COUNTED s_waitcnt vmcnt(N) -- the round before has landed, this one stays in flight --
// and meets the others at a bare s_barrier (which does not drain VMEM).  N = 1, 2, 4, 6, 8 pieces in flight per wave.
// Reports bytes per second per CU (events around 20 launches) and issue cycles per piece (s_memtime around each round's block of loads, wave 0 of
// every workgroup: counter ticks, with the ticks of the whole kernel beside them to say what share of a wave's time is issue).
// The last two rounds' bytes are read back from LDS and compared with the blob: a lost wait shows as a mismatch.
// build: hipcc --offload-arch=gfx950 -O3 -o lds_dma_stream tools/ubench/lds_dma_stream.hip ; run: ./lds_dma_stream
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void *lds_ptr_t;
constexpr int kPieces = 4224;                 // 1 KiB pieces: 4.3 MB, a multiple of 8 waves x every N
constexpr int kHalfDw = 8 * 8 * 256;          // one half of the double buffer: 8 waves x 8 pieces (64 KB), whatever N: one workgroup per CU

template <int N>
__global__ __launch_bounds__(512) void stream_k(const unsigned *blob, unsigned *tail, unsigned long long *ticks) {
    __shared__ __attribute__((aligned(16))) unsigned sm[2 * kHalfDw];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned l16 = lane * 16;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(blob), 0, kPieces * 1024, 0x00027000);
    constexpr int rounds = kPieces / (8 * N);
    unsigned long long t_issue = 0;
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
    for (int r = 0; r < rounds; ++r) {
        unsigned *half = sm + (r & 1) * kHalfDw;
        const unsigned src = (unsigned)(r * 8 * N + wave) * 1024u;
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (int i = 0; i < N; ++i)      // piece 8 i + wave of the round -> the same slot of the half
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(half + (8 * i + wave) * 256), 16, l16, src + i * 8192, 0, 0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        t_issue += t1 - t0;
        // round r - 1 has landed (own pieces: the count; everybody's: the barrier); its half is refilled in round r + 1, behind the barrier of round r
        if (r == 0) asm volatile("s_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (blockIdx.x == gridDim.x - 1)     // the last two rounds as they stand in LDS
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < N; ++i)
                *(u32x4 *)&tail[(h * 8 * N + 8 * i + wave) * 256 + lane * 4] = *(const u32x4 *)&sm[h * kHalfDw + (8 * i + wave) * 256 + lane * 4];
    if (threadIdx.x == 0) { ticks[blockIdx.x] = t_issue; ticks[gridDim.x + blockIdx.x] = __builtin_amdgcn_s_memtime() - t_begin; }
}

template <int N>
static bool run(const unsigned *blob, const std::vector<unsigned> &host, unsigned *tail, unsigned long long *ticks, int cus) {
    constexpr int rounds = kPieces / (8 * N);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    stream_k<N><<<cus, 512>>>(blob, tail, ticks);
    if (hipDeviceSynchronize() != hipSuccess) { printf("N = %d: launch failed\n", N); return false; }
    float best = 1e30f, worst = 0.f;
    for (int rep = 0; rep < 5; ++rep) {
        (void)hipEventRecord(e0);
        for (int it = 0; it < 20; ++it) stream_k<N><<<cus, 512>>>(blob, tail, ticks);
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1); ms /= 20;
        best = ms < best ? ms : best; worst = ms > worst ? ms : worst;
    }
    std::vector<unsigned> t(2 * 8 * N * 256);
    std::vector<unsigned long long> tk(2 * cus);
    (void)hipMemcpy(t.data(), tail, t.size() * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(tk.data(), ticks, 2 * cus * 8, hipMemcpyDeviceToHost);
    size_t bad = 0;
    for (int h = 0; h < 2; ++h) {        // half h holds the last round of parity h
        const int r = ((rounds - 1) & 1) == h ? rounds - 1 : rounds - 2;
        for (int i = 0; i < 8 * N * 256; ++i) bad += t[h * 8 * N * 256 + i] != host[(size_t)r * 8 * N * 256 + i];
    }
    double sum = 0, all = 0;
    for (int i = 0; i < cus; ++i) { sum += (double)tk[i]; all += (double)tk[cus + i]; }
    const double tick_piece = sum / cus / ((double)rounds * N);
    const double bytes = (double)kPieces * 1024;
    printf("N = %d: %7.1f us (worst %7.1f)  %6.1f GB/s per CU  issue %6.1f ticks per piece = %4.1f %% of the kernel's %7.0f  %s\n", N, best * 1e3, worst * 1e3,
           bytes / (best * 1e-3) / 1e9, tick_piece, 100.0 * sum / all, all / cus, bad ? "MISMATCH" : "image ok");
    return bad == 0;
}

int main() {
    hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
    const int cus = p.multiProcessorCount;
    std::vector<unsigned> host((size_t)kPieces * 256);
    unsigned s = 12345u;
    for (auto &v : host) { s = s * 1664525u + 1013904223u; v = s; }
    unsigned *blob, *tail; unsigned long long *ticks;
    (void)hipMalloc(&blob, host.size() * 4); (void)hipMalloc(&tail, 2 * 8 * 8 * 1024); (void)hipMalloc(&ticks, 2 * cus * 8);
    (void)hipMemcpy(blob, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    printf("%s, %d CUs, blob %.2f MB shared by all workgroups; the kernel needs 29 GB/s per CU today\n", p.gcnArchName, cus, kPieces * 1024 / 1e6);
    bool ok = true;
    ok &= run<1>(blob, host, tail, ticks, cus);
    ok &= run<2>(blob, host, tail, ticks, cus);
    ok &= run<4>(blob, host, tail, ticks, cus);
    ok &= run<6>(blob, host, tail, ticks, cus);
    ok &= run<8>(blob, host, tail, ticks, cus);
    return ok ? 0 : 1;
}
