// Micro-benchmark: sustained v_mfma_f32_32x32x16_bf16 rate of the whole chip as a function of the LDS fragment-read
// density (ds_read_b128 per MFMA) -- no global memory traffic inside the loop. Build: hipcc --offload-arch=gfx950 -O3
// tools/probes/mfma_ceiling.hip -o /tmp/mfma_ceiling ; run: /tmp/mfma_ceiling
// The 8-wave rows also exist with v_mfma_f32_16x16x32_bf16 (SHAPE = 16): the same 128x64 output block per wave (32
// accumulators of 4 registers instead of 8 of 16), twice the MFMAs at half the cycles each, and the same fragment reads,
// barriers and LDS-DMA fills per FLOP. main() times the two shapes interleaved in one process (profiles/
// gemm_mfma_shape.txt).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <chrono>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// READS = ds_read_b128 per group of NACC MFMAs; NACC = accumulator tiles per wave = MFMAs per phase (8: the GEMM's 8 waves
// x 128x64; 16: a 4-wave layout, one wave per SIMD owning 128x128 = 256 accumulator registers, 8 fragment reads per 16
// MFMAs = 0.5 per MFMA, the same LDS-DMA bytes per flop: 4 fills per wave and phase)
// SHAPE = 16: a phase is 2 * NACC MFMAs of 16x16x32 on half of the wave's 4 * NACC accumulators; the read and fill slots
// ride after (before) every second MFMA, so a phase has the FLOPs, the reads, the fills and the barrier of SHAPE = 32, and
// one trip of the loop is two phases (iters stays the number of phases and must be even).
template <int READS, int WAVES, int BAR, int DMA, int NACC, int SHAPE = 32>
__global__ __launch_bounds__(64 * WAVES) void mfma_loop(float* out, int iters, unsigned long long* clk, int rnd,
                                                        const char* src) {
  __shared__ __attribute__((aligned(1024))) uint4 lds[4096 + (DMA ? 4096 : 0)];       // 64 KiB (+ 64 KiB DMA landing zone)
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 4096; i += blockDim.x) {
    if (rnd) {                       // random bf16 values in (-2, 2): random sign, exponent 0x3e..0x3f, random mantissa
      uint32_t x = (i + 1) * 2654435761u + blockIdx.x * 40503u, w[4];
      for (int k = 0; k < 4; ++k) {
        x = x * 1664525u + 1013904223u;
        const uint32_t r = x >> 1;
        w[k] = (r & 0x807f807fu) | 0x3e003e00u | ((r >> 8) & 0x01000100u);
      }
      lds[i] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      lds[i] = make_uint4(0x3c003c00u + i, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u);
    }
  }
  __syncthreads();
  constexpr int R = SHAPE == 16 ? 2 : 1;        // MFMAs per slot; phases per trip
  f32x16 acc[SHAPE == 16 ? 1 : NACC];
  f32x4 acc4[SHAPE == 16 ? 4 * NACC : 1];
#pragma unroll
  for (int a = 0; a < (SHAPE == 16 ? 1 : NACC); ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
#pragma unroll
  for (int a = 0; a < (SHAPE == 16 ? 4 * NACC : 1); ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc4[a][r] = 0.f;
  uint4 fa[8], fb[4];
#pragma unroll
  for (int k = 0; k < 8; ++k) fa[k] = lds[(tid * 8 + k) & 4095];
#pragma unroll
  for (int k = 0; k < 4; ++k) fb[k] = lds[(tid * 4 + k + 2048) & 4095];
  // conflict-free fragment addresses: lane l reads 16 B at row (l&31), chunk ((l>>5) ^ ((l>>1)&7)) of 128-B rows
  const int base = ((tid >> 6) * 32 + (lane & 31)) * 8 + (((lane >> 5) ^ ((lane >> 1) & 7)) & 7);
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long t0 = __builtin_readcyclecounter();
  const uint32_t dma_lds = (uint32_t)(uintptr_t)(lds + 4096) + (uint32_t)(tid >> 6) * 8192;
  // every workgroup streams through its own 2 MiB window of an L2 / Infinity-Cache sized buffer (64 MiB)
  const uint32_t dma_lane = (uint32_t)lane * 16 + (uint32_t)(tid >> 6) * 1024;
  const char* dma_base = src + (size_t)(blockIdx.x & 31) * (2u << 20);
  for (int it0 = 0; it0 < iters; it0 += R) {
#pragma unroll
    for (int p = 0; p < R; ++p) {
      const int it = it0 + p;
      if (BAR) {
        if (DMA) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mm = 0; mm < NACC * R; ++mm) {
        const int m = mm / R;                      // the slot: one MFMA of 32x32x16, two of 16x16x32
        // 2 fills of 1 KiB per wave per 8 slots with 8 waves = the GEMM's LDS-DMA rate; 4 per 16 slots with 4 waves
        if (DMA && mm % R == 0 && ((m & 3) == 1) && (NACC == 16 || m == 1 || m == 5)) {
          const uint32_t m0v = __builtin_amdgcn_readfirstlane(dma_lds + (uint32_t)(m >> 2) * 2048u);
          const char* b = dma_base + ((size_t)((it * 4 + (m >> 2)) & 255) * 8192);
          asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(dma_lane), "s"(b)
                       : "memory", "m0");
          __builtin_amdgcn_sched_barrier(0);
        }
        // both MFMAs of a slot take the slot's fa fragment: a fragment read is consumed four slots (128 MFMA cycles)
        // behind its issue in either shape (indexed by mm it would be two MFMAs = 32 cycles, inside the LDS latency)
        if constexpr (SHAPE == 16)
          acc4[p * 2 * NACC + mm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, fb[mm & 3]), __builtin_bit_cast(bf16x8, fa[m & 7]), acc4[p * 2 * NACC + mm], 0, 0, 0);
        else
          acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fb[m & 3]),
                                                           __builtin_bit_cast(bf16x8, fa[m & 7]), acc[m], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (mm % R == R - 1 && m < READS) {
          fa[(m + 4) & 7] = lds[(base + (it & 7) * 256 + m * 8) & 4095];
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < (SHAPE == 16 ? 1 : NACC); ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[a][r];
#pragma unroll
  for (int a = 0; a < (SHAPE == 16 ? 4 * NACC : 1); ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) s += acc4[a][r];
  out[blockIdx.x * blockDim.x + tid] = s;
  // the stamps go to a buffer of their own: shader cycles in clk[0, 256), the 100 MHz reference in clk[256, 512)
  if (tid == 0) { clk[blockIdx.x] = t1 - t0; clk[256 + blockIdx.x] = r1 - r0; }
}

template <int READS, int WAVES, int BAR = 0, int DMA = 0, int NACC = 8>
void run(const char* tag, float* out, unsigned long long* clk, int iters, int rnd, const char* src = nullptr) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int rep = 0; rep < 3; ++rep) {
    hipEventRecord(e0);
    hipLaunchKernelGGL((mfma_loop<READS, WAVES, BAR, DMA, NACC>), dim3(256), dim3(64 * WAVES), 0, 0, out, iters, clk, rnd, src);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    unsigned long long c = 0;
    hipMemcpy(&c, clk, 8, hipMemcpyDeviceToHost);
    const double flops = 256.0 * WAVES * iters * NACC * 32768.0;
    if (rep == 2)
      printf("%s %-30s waves/CU %d  reads/%dmfma %d : %8.3f ms  %7.1f TFLOP/s  shader clock %.3f GHz  mfma-util %.1f %%\n", rnd ? "random" : "const ", tag, WAVES,
             NACC, READS, ms, flops / ms / 1e9, c / (ms * 1e6), 100.0 * iters * NACC * 32.0 * (WAVES / 4) / c);
  }
}

// ---- the two MFMA shapes, interleaved in one process ----
typedef void (*kern_t)(float*, int, unsigned long long*, int, const char*);
struct Arm {
  const char* row; int shape; kern_t k; bool dma;
  std::vector<double> ms, ghz;
};
template <int READS, int BAR, int DMA>
void add_row(std::vector<Arm>& arms, const char* row) {
  arms.push_back({row, 32, mfma_loop<READS, 8, BAR, DMA, 8, 32>, DMA != 0, {}, {}});
  arms.push_back({row, 16, mfma_loop<READS, 8, BAR, DMA, 8, 16>, DMA != 0, {}, {}});
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.size() & 1 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}
// one launch: wall by HIP events, in-kernel clock = d s_memtime / d s_memrealtime x 100 MHz, median over workgroups
static void launch(Arm& a, float* out, unsigned long long* clk, int iters, int rnd, const char* src, bool keep,
                   hipEvent_t e0, hipEvent_t e1) {
  hipEventRecord(e0);
  hipLaunchKernelGGL(a.k, dim3(256), dim3(512), 0, 0, out, iters, clk, rnd, a.dma ? src : (const char*)nullptr);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  if (!keep) return;
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  static unsigned long long h[512];
  hipMemcpy(h, clk, sizeof h, hipMemcpyDeviceToHost);
  std::vector<double> g(256);
  for (int i = 0; i < 256; ++i) g[i] = 0.1 * (double)h[i] / (double)h[256 + i];
  a.ms.push_back(ms);
  a.ghz.push_back(median(g));
}
static void shape_ab(float* out, unsigned long long* clk, int iters, const char* src, int rounds) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  const double flops = 256.0 * 8 * iters * 8 * 32768.0;
  for (int rnd = 0; rnd < 2; ++rnd) {
    std::vector<Arm> arms;
    add_row<0, 0, 0>(arms, "regs only");
    add_row<6, 0, 0>(arms, "0.75 rd/mfma");
    add_row<6, 1, 0>(arms, "0.75 rd + barrier/8");
    add_row<6, 0, 1>(arms, "0.75 rd + DMA");
    add_row<6, 1, 1>(arms, "0.75 rd + barrier + DMA");
    // >= 2 s of back-to-back launches before the first kept round, so the clock has settled under load
    const auto w0 = std::chrono::steady_clock::now();
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 2.0)
      for (Arm& a : arms) launch(a, out, clk, iters, rnd, src, false, e0, e1);
    for (int r = 0; r < rounds; ++r)
      for (Arm& a : arms) launch(a, out, clk, iters, rnd, src, true, e0, e1);
    printf("\n%s operands, %d interleaved rounds, 256 workgroups x 8 waves, 128x64 per wave\n", rnd ? "random" : "const ", rounds);
    printf("%-26s shape     median ms   min ms   max ms   TFLOP/s(med)  clock GHz(med)  mfma-util %%\n", "row");
    for (size_t i = 0; i < arms.size(); ++i) {
      Arm& a = arms[i];
      const double med = median(a.ms), mn = *std::min_element(a.ms.begin(), a.ms.end()),
                   mx = *std::max_element(a.ms.begin(), a.ms.end()), ghz = median(a.ghz);
      printf("%-26s %-9s %9.3f %8.3f %8.3f %12.1f %15.3f %11.1f\n", a.row, a.shape == 16 ? "16x16x32" : "32x32x16", med, mn,
             mx, flops / med / 1e9, ghz, 100.0 * iters * 8 * 32.0 * 2 / (med * 1e6 * ghz));
      if (a.shape == 16) {
        Arm& b = arms[i - 1];
        const double gain = median(b.ms) - med, spread = mx - mn;
        printf("%-26s 16 vs 32: %+.3f ms (%.3fx), spread of the 16x16x32 rounds %.3f ms -> %s\n", "", -gain,
               median(b.ms) / med, spread, gain > 2 * spread ? "faster by more than twice its spread" : "not faster by twice its spread");
      }
    }
  }
}

int main(int argc, char** argv) {
  float* out; unsigned long long* clk;
  hipMalloc(&out, 256 * 512 * 4); hipMalloc(&clk, 512 * 8);
  const int iters = 40000;
  char* src;
  hipMalloc(&src, 64u << 20);
  {   // random bf16 payload for the DMA stream too (data-dependent power)
    uint32_t* h = (uint32_t*)malloc(64u << 20);
    uint32_t x = 12345u;
    for (size_t i = 0; i < (64u << 20) / 4; ++i) { x = x * 1664525u + 1013904223u; h[i] = ((x >> 1) & 0x807f807fu) | 0x3e003e00u; }
    hipMemcpy(src, h, 64u << 20, hipMemcpyHostToDevice);
    free(h);
  }
  if (argc > 1) {                      // mfma_ceiling ROUNDS: the shape comparison alone
    shape_ab(out, clk, iters, src, atoi(argv[1]) > 0 ? atoi(argv[1]) : 15);
    return 0;
  }
  for (int rnd = 0; rnd < 2; ++rnd) {
    run<0, 8>("regs only", out, clk, iters, rnd);
    run<6, 8>("0.75 rd/mfma", out, clk, iters, rnd);
    run<6, 8, 1, 0>("0.75 rd + barrier/8", out, clk, iters, rnd);
    run<6, 8, 0, 1>("0.75 rd + DMA", out, clk, iters, rnd, src);
    run<6, 8, 1, 1>("0.75 rd + barrier + DMA", out, clk, iters, rnd, src);
    run<0, 8, 1, 1>("regs + barrier + DMA", out, clk, iters, rnd, src);
    // the 4-wave layout (one wave per SIMD, 128x128 per wave): half the fragment reads per MFMA, half the barriers
    run<0, 4, 0, 0, 16>("4w regs only", out, clk, iters / 2, rnd);
    run<8, 4, 0, 0, 16>("4w 0.5 rd/mfma", out, clk, iters / 2, rnd);
    run<8, 4, 1, 0, 16>("4w 0.5 rd + barrier/16", out, clk, iters / 2, rnd);
    run<8, 4, 1, 1, 16>("4w 0.5 rd + barrier + DMA", out, clk, iters / 2, rnd, src);
    run<12, 4, 1, 1, 16>("4w 0.75 rd + barrier + DMA", out, clk, iters / 2, rnd, src);
  }
  shape_ab(out, clk, iters, src, 15);
  return 0;
}
