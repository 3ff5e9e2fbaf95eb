// tools/record_stream24_bench.hip — does a 640-byte DELTA record (24-bit value fields) stream as many records per second as the 768-byte one?
// The loop is record_stream_bench.hip's, in spmv_rowblock_kernel's configuration: 14 consumer wavefronts of a 1024-thread workgroup per CU,
// 8 records in flight per wavefront, parked in accumulator registers (values a0..a15, gap word a16..a23) until a counted wait, `nt` loads.
//   shape 0: dwordx2 + dword  at 512 + 4 lane              768 bytes: two 32-bit value words, two 16-bit gaps (today's record)
//   shape 1: dwordx2 + ushort at 512 + 2 lane              640 bytes: two 24-bit value fields + gap A in the dwordx2, gap B on its own
//   shape 2: dwordx2 + dword  at 512 + 2 lane (unaligned)  640 bytes: the same record, gap B read as the low half of an unaligned dword
// Every shape walks the SAME number of records (ogbl-ppa's image: 364 539, rounded up to whole rounds per wavefront), once over one
// image (which the Infinity Cache may partly keep between launches) and once round-robin over three images (MALL-cold, like bench.py's leg).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

#define RING_AGPRS "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", \
                   "a18", "a19", "a20", "a21", "a22", "a23"
constexpr int kDepth = 8, kWaves = 14, kWgs = 256;
template <int kShape> constexpr uint32_t record_bytes() { return kShape == 0 ? 768u : 640u; }

template <int kShape, int K>
__device__ __forceinline__ void issue(const uint8_t* base, uint32_t byte_off, uint32_t lane) {
    if (kShape == 0)
        asm volatile("s_nop 4\n\tglobal_load_dwordx2 a[%0:%1], %3, %5 nt\n\tglobal_load_dword a[%2], %4, %5 offset:512 nt" ::"n"(2 * K), "n"(2 * K + 1),
                     "n"(K + 16), "v"(byte_off + lane * 8u), "v"(byte_off + lane * 4u), "s"(base) : "memory", RING_AGPRS);
    if (kShape == 1)
        asm volatile("s_nop 4\n\tglobal_load_dwordx2 a[%0:%1], %3, %5 nt\n\tglobal_load_ushort a[%2], %4, %5 offset:512 nt" ::"n"(2 * K), "n"(2 * K + 1),
                     "n"(K + 16), "v"(byte_off + lane * 8u), "v"(byte_off + lane * 2u), "s"(base) : "memory", RING_AGPRS);
    if (kShape == 2)
        asm volatile("s_nop 4\n\tglobal_load_dwordx2 a[%0:%1], %3, %5 nt\n\tglobal_load_dword a[%2], %4, %5 offset:512 nt" ::"n"(2 * K), "n"(2 * K + 1),
                     "n"(K + 16), "v"(byte_off + lane * 8u), "v"(byte_off + lane * 2u), "s"(base) : "memory", RING_AGPRS);
}
template <int K>
__device__ __forceinline__ uint32_t take() {
    uint32_t a, b, c;
    asm volatile("s_waitcnt vmcnt(%6)\n\tv_accvgpr_read_b32 %0, a[%3]\n\tv_accvgpr_read_b32 %1, a[%4]\n\tv_accvgpr_read_b32 %2, a[%5]"
                 : "=v"(a), "=v"(b), "=v"(c) : "n"(2 * K), "n"(2 * K + 1), "n"(K + 16), "n"(2 * (kDepth - 1)) : "memory");
    return a ^ b ^ c;
}
template <int kShape, int K>
__device__ __forceinline__ void step(const uint8_t* p, uint32_t base, uint32_t last, uint32_t lane, uint32_t& acc) {
    acc ^= take<K>();
    issue<kShape, K>(p, min(base + K + kDepth, last) * record_bytes<kShape>(), lane);
    if constexpr (K + 1 < kDepth) step<kShape, K + 1>(p, base, last, lane, acc);
}
template <int kShape, int K>
__device__ __forceinline__ void prime(const uint8_t* p, uint32_t last, uint32_t lane) {
    issue<kShape, K>(p, min(uint32_t(K), last) * record_bytes<kShape>(), lane);
    if constexpr (K + 1 < kDepth) prime<kShape, K + 1>(p, last, lane);
}

template <int kShape>
__global__ __launch_bounds__(1024) void ring_kernel(const uint8_t* __restrict__ src, uint32_t records_per_wave, uint32_t* sink) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x & 63;
    if (wave >= kWaves) return;
    const uint64_t a = reinterpret_cast<uint64_t>(src + (size_t(blockIdx.x) * kWaves + wave) * records_per_wave * record_bytes<kShape>());
    const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(a >> 32)), lo = __builtin_amdgcn_readfirstlane(uint32_t(a));
    const uint8_t* p = reinterpret_cast<const uint8_t*>((uint64_t(hi) << 32) | lo);
    const uint32_t last = records_per_wave - 1;
    prime<kShape, 0>(p, last, lane);
    uint32_t acc = 0;
    for (uint32_t base = 0; base < records_per_wave; base += kDepth) step<kShape, 0>(p, base, last, lane, acc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory", RING_AGPRS);
    if (acc == 0x12345678u) sink[0] = acc;
}

template <int kShape>
void run(const char* name, const uint8_t* d, uint32_t records_per_wave, int images, uint32_t* sink) {
    const size_t image = size_t(records_per_wave) * kWgs * kWaves * record_bytes<kShape>();
    const size_t stride = (image + 2 + 4095) / 4096 * 4096;   // shape 2 reads two bytes past its last record
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    const int reps = 30;
    for (int i = 0; i < 6; ++i) hipLaunchKernelGGL((ring_kernel<kShape>), dim3(kWgs), dim3(1024), 0, 0, d + (i % images) * stride, records_per_wave, sink);
    hipEventRecord(a);
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL((ring_kernel<kShape>), dim3(kWgs), dim3(1024), 0, 0, d + (i % images) * stride, records_per_wave, sink);
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    const double us = ms / reps * 1e3, records = double(records_per_wave) * kWgs * kWaves;
    printf("%-34s %d image%s of %6.1f MB  %6.1f us  %7.1f GB/s  %6.2f G records/s\n", name, images, images > 1 ? "s" : " ", image / 1e6, us, image / us / 1e3, records / us / 1e3);
}

int main() {
    const size_t cap = 1ull << 30;                             // three 768-byte images of 286 MB and their slack fit
    uint8_t* d; uint32_t* sink;
    if (hipMalloc(&d, cap) != hipSuccess || hipMalloc(&sink, 64) != hipSuccess) return 1;
    hipMemset(d, 1, cap);
    const uint32_t per_wave = (364539 + kWgs * kWaves - 1) / (kWgs * kWaves), records_per_wave = (per_wave + kDepth - 1) / kDepth * kDepth;   // 104
    for (int pass = 0; pass < 3; ++pass)
        for (int images = 1; images <= 3; images += 2) {
            run<0>("768 B dwordx2 + dword", d, records_per_wave, images, sink);
            run<1>("640 B dwordx2 + ushort", d, records_per_wave, images, sink);
            run<2>("640 B dwordx2 + unaligned dword", d, records_per_wave, images, sink);
        }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
