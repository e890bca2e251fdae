// The tiled weight-gradient kernel of lvl_linear_wgrad and its launcher, shared by the translation units that instantiate it:
// wgrad_mfma.hip (the 6x6 and 8x4 wave tiles of the towers and the base decoder; the design notes are in its header) and
// wgrad_160.hip (the 5x5 and 8x5 wave tiles of the 1600-family widths).
#pragma once
#include "internal.h"

// the LDS-DMA fills set M0 inside inline asm and say so in the clobber list; this kernel has no other M0 user
#pragma clang diagnostic ignored "-Winline-asm"

typedef __attribute__((ext_vector_type(8))) __bf16 wg_bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 wg_bf16x2;
typedef __attribute__((ext_vector_type(4))) float wg_f32x4;
typedef __attribute__((ext_vector_type(4))) short wg_s16x4;

namespace {

constexpr int MS = 32;          // rows per step (one MFMA contraction)

__device__ __forceinline__ uint2 tr_read(const uint16_t* p) {
  const wg_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s16x4*)p);
  return __builtin_bit_cast(uint2, v);
}
__device__ __forceinline__ wg_f32x4 mfma16(uint4 a, uint4 b, wg_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wg_bf16x8, a), __builtin_bit_cast(wg_bf16x8, b),
                                                 c, 0, 0, 0);
}

// Row plan of a launch (host-computed, no divisions in the kernel): the M/32 full row blocks are dealt to the S splits
// as `base` blocks each, the first `rem` splits one more; the dynamic schedule cuts a unit into chunks of L blocks
// (L even), nch0 / nch1 of them for a unit of base / base + 1 blocks.
struct RowPlan { int base, rem, L, nch0, nch1, late_mod; };

// XCD-aware decode of a block id into one of the P = ntiles * S split-major (split, tile) pairs: consecutive block ids
// alternate XCDs, so XCD x = bid % 8 is given a contiguous range of the pairs: the workgroups that stream the same rows
// sit behind the same L2. One definition for the kernel and for lvl_linear_wgrad_pair_of_block (the tests' view of it).
template <bool ANY_PAIRS>
__host__ __device__ __forceinline__ int pair_of_block(int P, int bid) {
  if constexpr (!ANY_PAIRS) {
    return (bid & 7) * (P >> 3) + (bid >> 3);      // XCD x owns [x*P/8, (x+1)*P/8); make_plan: P is a multiple of 8
  } else {
    // the 160-family: 4800 x 1600 is 150 tiles at S = 1, so its plans take ANY number of pairs. XCD x owns q (+ 1 for
    // the first r XCDs) consecutive pairs, P = 8 q + r -- as many as there are block ids congruent to x: a bijection
    const int x8 = bid & 7, q = P >> 3, r = P & 7;
    return (x8 < r ? x8 * (q + 1) : r * (q + 1) + (x8 - r) * q) + (bid >> 3);
  }
}

template <int WN, int WK, int TA, int TB>
struct Geo {
  static constexpr int NW = WN * WK, NT = 64 * NW;
  static constexpr int TN = 16 * TA * WN, TK = 16 * TB * WK;     // workgroup tile (rows of dW x columns of dW)
  static constexpr int SA = TN + 16, SB = TK + 16;            // image row strides in elements (+32 B)
  // LDS-DMA plan: one global_load_lds_dwordx4 fills 64 consecutive 16-B chunks (1 KiB) of a stage. An image of
  // MS rows x (stride/8) chunks is exactly IA (IB) such fills; the pad chunks of a row carry don't-care data.
  static constexpr int IA = MS * (SA / 8) / 64, IB = MS * (SB / 8) / 64;      // = TA*WN + 1, TB*WK + 1
  static constexpr int NI = (IA + IB + NW - 1) / NW;                          // fills per wave per step
  static constexpr int STAGE = MS * (SA + SB) + (NI * NW - IA - IB) * 512;    // elements per stage (+ dump area)
  static constexpr int NSTAGE = (4 * STAGE * 2 <= 160 * 1024) ? 4 : 3;   // ring depth: fills run NSTAGE-1 steps ahead
  static_assert(MS * (SA / 8) % 64 == 0 && MS * (SB / 8) % 64 == 0, "images must be whole 1-KiB fills");
};

template <int WN, int WK, int TA, int TB, bool BIAS>
__global__ __launch_bounds__(64 * WN * WK) void wgrad_kernel(const uint16_t* __restrict__ dy,
                                                             const uint16_t* __restrict__ x, float* __restrict__ part,
                                                             float* __restrict__ bpart, int64_t M, int N, int K,
                                                             int tiles_k, int ntiles, int S, RowPlan rp,
                                                             unsigned* __restrict__ sched) {
  using G = Geo<WN, WK, TA, TB>;
  static_assert(TA >= 2, "the mid-step barrier splits the A tiles in two groups (TA/2 and TA - TA/2 tiles)");
  extern __shared__ __attribute__((aligned(16))) uint16_t smem[];     // [NSTAGE][A image | B image | dump]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % WN, wk = wave / WN;
  const int bid = blockIdx.x;
  const int pair = pair_of_block<TA == 5 || TB == 5>(ntiles * S, bid);
  const int split = pair / ntiles, tile = pair % ntiles;
  const int n0 = (tile / tiles_k) * G::TN, k0 = (tile % tiles_k) * G::TK;
  const int64_t steps_total = M / MS;      // full row blocks; the < 32 tail rows are added by wgrad_reduce_kernel
  // (the dbias instantiations keep the static plan: they are not on the training path -- the bias gradients come from
  // the LayerNorm / GEMM epilogues -- and their register budget leaves no room for the claim state)
  const bool dyn = !BIAS && sched != nullptr;

  // ---- staging plan (LDS-DMA, no VGPR round trip) ---------------------------------------------------------------
  // Fill f (0 .. NI*NW-1) of a step is issued by wave f % NW; lane l of the fill lands at stage byte f*1024 + l*16.
  // Fills 0..IA-1 tile the A image, IA..IA+IB-1 the B image, the rest (so that every wave issues exactly NI fills
  // and one s_waitcnt immediate fits all) land in a dump area behind the images. Pad chunks and dump chunks read
  // chunk 0 of their row. Per-lane source pointers advance by one row block per step.
  const uint16_t* src[G::NI];
  int64_t src_step[G::NI];
  int dst_off[G::NI];             // element offset of the fill inside a stage (wave-uniform)
  // point the fill sources at row block `rb` (the first step of a stream)
  auto set_sources = [&](int64_t rb) {
#pragma unroll
    for (int q = 0; q < G::NI; ++q) {
      const int f = wave + q * G::NW;
      dst_off[q] = f * 512;
      const int chunk = f * 64 + lane;
      if (f < G::IA) {
        const int row = chunk / (G::SA / 8), c8 = chunk % (G::SA / 8);
        src[q] = dy + (rb * MS + row) * (int64_t)N + n0 + (c8 < G::TN / 8 ? c8 : 0) * 8;
        src_step[q] = (int64_t)MS * N;
      } else {
        const int cb = f < G::IA + G::IB ? chunk - G::IA * 64 : lane;
        const int row = cb / (G::SB / 8), c8 = cb % (G::SB / 8);
        src[q] = x + (rb * MS + row) * (int64_t)K + k0 + (c8 < G::TK / 8 ? c8 : 0) * 8;
        src_step[q] = (int64_t)MS * K;
      }
    }
  };
  // Fills are issued through inline asm: the compiler's LDS-DMA alias tracking would otherwise put s_waitcnt
  // vmcnt(0) in front of every LDS read and drain the run-ahead fills. Steps at or beyond `last_step` (run-ahead
  // past the end of the matrix) re-read the last full row block.
  int last_step = 0;              // steps_total - 1 - (first row block of the stream)
  int issued = 0;                 // steps issued so far in this stream; src[] points at step min(issued, last_step)
  auto issue_loads = [&](int stage) {
    const uint32_t lds_base = (uint32_t)(uintptr_t)(smem + stage * G::STAGE) ;
#pragma unroll
    for (int q = 0; q < G::NI; ++q) {
      const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)dst_off[q] * 2u);
      asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(m0v), "v"(src[q]) : "memory", "m0");
      if (issued < last_step) src[q] += src_step[q];
    }
    ++issued;
  };

  // ---- chunk claims (dynamic schedule only) ---------------------------------------------------------------------
  // A claim is ONE asm block on wave 0, lane 0 (EXEC narrowed inside it): returning atomic add -> s_waitcnt vmcnt(0) ->
  // ds_write of the reply into the mailbox. The reply never lives in a compiler-visible register across the wait (a
  // parked reply would be at the mercy of live-range splitting). The wait also drains this wave's run-ahead fills,
  // about 1 us once per chunk of >= 24 steps: < 1 % of the kernel. The mailbox is the 32 pad bytes behind row 0 of a
  // stage's dY image: never read by a fragment load, rewritten (with don't-care data) only by that stage's next fill.
  auto mbox_addr = [&](int stage) { return (uint32_t)(uintptr_t)(smem + stage * G::STAGE + G::TN); };
  uint64_t exec_save;
  uint32_t reply;
  auto claim = [&](unsigned* ctr, int stage) {          // mailbox <- old value of *ctr; *ctr += 1
    if (wave == 0)
      asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\t"
                   "s_waitcnt vmcnt(0)\n\tds_write_b32 %5, %0\n\ts_mov_b64 exec, %1"
                   : "=&v"(reply), "=&s"(exec_save) : "v"(0u), "v"(1u), "s"(ctr), "v"(mbox_addr(stage)) : "memory");
  };
  auto peek = [&](unsigned* ctr, int stage) {           // mailbox <- *ctr (agent-scope load)
    if (wave == 0)
      asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\tglobal_load_dword %0, %2, %3 sc1\n\t"
                   "s_waitcnt vmcnt(0)\n\tds_write_b32 %4, %0\n\ts_mov_b64 exec, %1"
                   : "=&v"(reply), "=&s"(exec_save) : "v"(0u), "s"(ctr), "v"(mbox_addr(stage)) : "memory");
  };
  auto count_one = [&](unsigned* ctr) {                 // fire-and-forget atomic add of 1
    if (wave == 0)
      asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %1, %2, %3\n\ts_mov_b64 exec, %0"
                   : "=&s"(exec_save) : "v"(0u), "v"(1u), "s"(ctr) : "memory");
  };
  // mailbox -> every wave; two barriers: write -> read, read -> anything that may overwrite the mailbox
  auto collect = [&](int stage) -> int {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // (asm LDS read: a volatile C++ read becomes a flat load with a vmcnt(0) drain of every wave's run-ahead fills)
    uint32_t raw;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(raw) : "v"(mbox_addr(stage)) : "memory");
    const int v = __builtin_amdgcn_readfirstlane(raw);
    __builtin_amdgcn_s_barrier();
    return v;
  };

  // ---- per-lane fragment offsets -----------------------------------------------------------------------------
  // tr read: lane (g = lane>>4, mm = lane&15) points at row rb + g*4 + mm/4, columns col0 + 4*(mm%4)..+3 and
  // receives rows rb + g*4 .. +3 at column col0 + mm. rb = 0 and 16 -> contraction order (g*4+e | 16+g*4+e).
  const int g = lane >> 4, mm = lane & 15;
  const int rsub = g * 4 + (mm >> 2), csub = (mm & 3) * 4;
  const int offA = rsub * G::SA + wn * (16 * TA) + csub;                  // + i*16 (+ 16*SA for the second half)
  const int offB = MS * G::SA + rsub * G::SB + wk * (16 * TB) + csub;

  wg_f32x4 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j) acc[i][j] = wg_f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[TA];
#pragma unroll
  for (int i = 0; i < TA; ++i) bsum[i] = 0.f;
  const wg_bf16x2 ones = {(__bf16)1.0f, (__bf16)1.0f};

  // NSTAGE-deep ring with the barrier in the MIDDLE of a step. Step s multiplies stage s%NSTAGE in two halves of
  // TA/2 A-tiles each. Between the halves: wait until this wave's fills of step s+1 have landed (vmcnt counts them
  // in order), s_barrier (=> step s+1 is complete for everybody, and everybody is done with step s-1), issue the
  // fills of step s+NSTAGE-1 into the stage step s-1 used, then read the B fragments of step s+1 into a second
  // register set while the second half's MFMAs run. No LDS latency and no fill latency sits between the last MFMA
  // of one step and the first of the next. The barrier is the bare s_barrier: a fence would drain the run-ahead.
  static_assert(G::NSTAGE == 4, "the mid-step schedule is written for a 4-deep ring");
  auto read_b = [&](const uint16_t* img, uint4 (&bf)[TB]) {
#pragma unroll
    for (int j = 0; j < TB; ++j) {
      const uint2 lo = tr_read(img + offB + j * 16), hi = tr_read(img + offB + j * 16 + 16 * G::SB);
      bf[j] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
  };
  auto read_a = [&](const uint16_t* img, int i) {
    const uint2 lo = tr_read(img + offA + i * 16), hi = tr_read(img + offA + i * 16 + 16 * G::SA);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  };
  auto bias_dot = [&](int i, const uint4& af) {
    if (BIAS && (i % WK) == wk) {       // dbias: this wave's share of the n-tiles
      float b = bsum[i];
      b = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(wg_bf16x2, af.x), ones, b, false);
      b = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(wg_bf16x2, af.y), ones, b, false);
      b = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(wg_bf16x2, af.z), ones, b, false);
      b = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(wg_bf16x2, af.w), ones, b, false);
      bsum[i] = b;
    }
  };
  uint4 bf[TB], bf_next[TB], af_next;
  int stage = 0;
  // one step; `cur` holds this step's B fragments, `nxt` receives the next step's (ping-pong: no register copies)
  auto do_step = [&](uint4 (&cur)[TB], uint4 (&nxt)[TB]) {
    const uint16_t* img = smem + stage * G::STAGE;
    const int nstage = stage == G::NSTAGE - 1 ? 0 : stage + 1;
    const uint16_t* img_next = smem + nstage * G::STAGE;
#pragma unroll
    for (int i = 0; i < TA / 2; ++i) {
      const uint4 af = af_next;
      af_next = read_a(img, i + 1);
      bias_dot(i, af);
#pragma unroll
      for (int j = 0; j < TB; ++j) acc[i][j] = mfma16(af, cur[j], acc[i][j]);
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G::NI) : "memory");      // fills of step+1 landed (step+2 may be in flight)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue_loads(stage == 0 ? G::NSTAGE - 1 : stage - 1);               // step+3 -> the stage step-1 used
    read_b(img_next, nxt);
#pragma unroll
    for (int i = TA / 2; i < TA; ++i) {
      const uint4 af = af_next;
      af_next = i + 1 < TA ? read_a(img, i + 1) : read_a(img_next, 0);
      bias_dot(i, af);
#pragma unroll
      for (int j = 0; j < TB; ++j) acc[i][j] = mfma16(af, cur[j], acc[i][j]);
    }
    stage = nstage;
  };

  // Units visited: the own (tile, split) first, then -- dynamic schedule only -- the other splits of the same tile.
  unsigned* const taken = dyn ? sched + ntiles * S + tile : nullptr;      // chunks of this tile consumed so far
  // (test hook, lvl_debug_late_workgroups: a "late" workgroup visits nothing and writes a zero slab)
  const int visits = dyn ? ((rp.late_mod > 0 && bid % rp.late_mod == 1) ? 0 : S) : 1;
  for (int d = 0; d < visits; ++d) {
    int sp = split + d;
    if (sp >= S) sp -= S;
    const int ulen = rp.base + (sp < rp.rem ? 1 : 0);                               // row blocks of the unit
    const int64_t ub = (int64_t)sp * rp.base + (sp < rp.rem ? sp : rp.rem), ue = ub + ulen;
    int L = ulen, nchunks = ulen > 0 ? 1 : 0, cur = 0;
    unsigned* uctr = nullptr;
    if (dyn) {
      L = rp.L;      // even: the fragment ping-pong is back in phase at every boundary the stream may run across
      nchunks = sp < rp.rem ? rp.nch1 : rp.nch0;
      uctr = sched + sp * ntiles + tile;
      if (d > 0) {
        // steal only if the tile still has unconsumed chunks (one load; stale by at most the claims in flight)
        const int total = rp.rem * rp.nch1 + (S - rp.rem) * rp.nch0;
        peek(taken, 0);
        if (collect(0) >= total) break;
      }
      claim(uctr, 0);
      cur = collect(0);
    }
    while (cur < nchunks) {
      // ---- one stream: chunk `cur` and, while the claims keep returning the next index, the chunks behind it ----
      if (dyn) count_one(taken);
      int64_t pos = ub + (int64_t)cur * L;
      set_sources(pos);
      last_step = (int)(steps_total - 1 - pos);
      issued = 0;
      stage = 0;
      issue_loads(0);
      issue_loads(1);
      issue_loads(2);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G::NI) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      read_b(smem, bf);
      af_next = read_a(smem, 0);
      int next = nchunks;            // where the next stream of this unit starts (>= nchunks: none)
      for (;;) {
        const int len = (int)(ue - pos < L ? ue - pos : L);
        const bool more = dyn && cur + 1 < nchunks;
        int step = 0;
        for (; step + 1 < len; step += 2) {
          do_step(bf, bf_next);
          do_step(bf_next, bf);
        }
        if (step < len) do_step(bf, bf_next);          // odd length: only a unit's last chunk
        if (!more) break;
        // every wave has finished the step that used stage `done`: its pad is free until the next step refills it
        const int done = stage == 0 ? G::NSTAGE - 1 : stage - 1;
        claim(uctr, done);
        next = collect(done);
        if (next != cur + 1 || (len & 1)) break;       // a tile-mate took chunks of this unit: stop, restart at `next`
        count_one(taken);
        cur = next;
        next = nchunks;
        pos += L;
      }
      // the run-ahead fills must have landed (and everybody must be done reading) before the stages are reused
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      cur = next;
    }
  }

  // ---- epilogue: partial tile of this split -------------------------------------------------------------------
  float* out = part + ((size_t)split * N + n0 + wn * (16 * TA)) * K + k0 + wk * (16 * TB);
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(i * 16 + g * 4 + r) * K + j * 16 + mm] = acc[i][j][r];
  if (BIAS && k0 == 0) {
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      if ((i % WK) == wk) {
        float b = bsum[i];
        b += __shfl_xor(b, 16, 64);
        b += __shfl_xor(b, 32, 64);
        if (g == 0) bpart[(size_t)split * N + n0 + wn * (16 * TA) + i * 16 + mm] = b;
      }
    }
  }
  if (dyn && wave == 0) {
    // sign-off: this workgroup's counter traffic is complete (every stream ended with vmcnt(0)); the last workgroup
    // out leaves the counter block zeroed for the next launch that is handed the same block
    const int nctr = ntiles * S + ntiles;          // unit counters | per-tile consumed counts | [nctr] = sign-offs
    unsigned gone = 0;
    if (lane == 0) gone = __hip_atomic_fetch_add(sched + nctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gone = __builtin_amdgcn_readfirstlane(gone);
    if (gone == gridDim.x - 1)
      for (int q = lane; q <= nctr; q += 64) __hip_atomic_store(sched + q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct Plan { int cfg, tiles_k, ntiles, S; bool ok; };

// chunks per (tile, split) unit of the dynamic schedule: at least ~48 steps (1536 rows, ~30 us) each, at most 4
RowPlan row_plan(int64_t M, int S) {
  const int64_t steps = M / MS;
  RowPlan rp;
  rp.base = (int)(steps / S);
  rp.rem = (int)(steps % S);
  int c = rp.base / 48;
  c = c < 1 ? 1 : (c > 4 ? 4 : c);
  rp.L = ((rp.base + 1 + c - 1) / c + 1) & ~1;
  if (rp.L < 2) rp.L = 2;
  rp.nch0 = (rp.base + rp.L - 1) / rp.L;
  rp.nch1 = (rp.base + 1 + rp.L - 1) / rp.L;
  rp.late_mod = lvl_debug_late_mod();
  return rp;
}

template <int WN, int WK, int TA, int TB>
int launch(const Plan& p, const void* dy, const void* x, float* part, float* bpart, int64_t M, int N, int K,
           unsigned* sched, hipStream_t st) {
  const RowPlan rp = row_plan(M, p.S);
  using G = Geo<WN, WK, TA, TB>;
  const size_t shmem = (size_t)G::NSTAGE * G::STAGE * sizeof(uint16_t);
  const dim3 grid((unsigned)(p.ntiles * p.S)), block(G::NT);
  if (bpart != nullptr) {
    if (int rc = lvl_allow_lds<wgrad_kernel<WN, WK, TA, TB, true>>()) return rc;
    hipLaunchKernelGGL((wgrad_kernel<WN, WK, TA, TB, true>), grid, block, shmem, st, (const uint16_t*)dy,
                       (const uint16_t*)x, part, bpart, M, N, K, p.tiles_k, p.ntiles, p.S, rp, sched);
  } else {
    if (int rc = lvl_allow_lds<wgrad_kernel<WN, WK, TA, TB, false>>()) return rc;
    hipLaunchKernelGGL((wgrad_kernel<WN, WK, TA, TB, false>), grid, block, shmem, st, (const uint16_t*)dy,
                       (const uint16_t*)x, part, bpart, M, N, K, p.tiles_k, p.ntiles, p.S, rp, sched);
  }
  LVL_CHECK_LAUNCH("linear_wgrad");
  return LVL_OK;
}

}  // namespace
