// The persistent TN GEMM kernel templates (gemm_tn_kernel<EPI, F32O> on v_mfma_f32_32x32x16_bf16, gemm_tn_mfma16<EPI> on
// v_mfma_f32_16x16x32_bf16: one body, gemm_tn_body) and their launcher (launch_tn), described at the top of
// gemm_tn_mfma.hip. A header because two translation units instantiate it: gemm_tn_mfma.hip (epilogues 0-5: every C entry
// point and their dispatch) and gemm_tn_gelu.hip (the exact-GELU epilogues 6-8). Everything here sits in an anonymous
// namespace: each unit gets its own instantiations.
#pragma once
#include <type_traits>

#include "internal.h"
#include "gelu_erf.h"

// the LDS-DMA fills set M0 inside inline asm and say so in the clobber list; this kernel has no other M0 user
#pragma clang diagnostic ignored "-Winline-asm"

typedef __attribute__((ext_vector_type(8))) __bf16 gm_bf16x8;
typedef __attribute__((ext_vector_type(16))) float gm_f32x16;
typedef __attribute__((ext_vector_type(4))) float gm_f32x4;

namespace {

constexpr int BK = 64;                 // contraction elements per K block (one 128-byte line per row)
constexpr int TM = 256, TN = 256;      // workgroup tile
constexpr int SLOT = 128 * 128;        // bytes of one slot: 128 rows x 128 B
constexpr int NSLOT = 8;               // two K blocks x {X0, X1, W0, W1}
constexpr int BIAS_OFF = NSLOT * SLOT; // four 1-KiB images of bias[n0 .. n0+255] behind the ring (tile index & 3)
constexpr int MBOX_OFF = BIAS_OFF + 4 * 1024;   // one word: the tile-queue reply wave 0 publishes to the workgroup
constexpr int SMEM_B = MBOX_OFF + 64;
constexpr int DYN_MIN_NB = 5;          // K blocks a tile needs for the publish (block 2) -> read (block nb-3) hand-off
enum { S_X0 = 0, S_X1 = 1, S_W0 = 2, S_W1 = 3 };

__device__ __forceinline__ gm_f32x16 mfma32(uint4 a, uint4 b, gm_f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gm_bf16x8, a), __builtin_bit_cast(gm_bf16x8, b),
                                                 c, 0, 0, 0);
}
__device__ __forceinline__ gm_f32x4 mfma16(uint4 a, uint4 b, gm_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gm_bf16x8, a), __builtin_bit_cast(gm_bf16x8, b),
                                                 c, 0, 0, 0);
}

// sigmoid1702 / quick_gelu / qgelu1 / bf16_lo / bf16_hi: common.h (shared with quickgelu.hip, which rebuilds the activation)
__device__ __forceinline__ float quick_gelu_grad(float u) {
  const float s = sigmoid1702(u);
  return s * (1.f + 1.702f * u * (1.f - s));
}

// QuickGELU pieces of the bf16 epilogues, scalar f32 on purpose: inside this dependent chain (cvt -> mul -> exp2 -> add -> rcp ->
// mul, two waves per SIMD) the packed forms v_pk_mul / v_pk_add / v_pk_fma_f32 are SLOWER than the scalar ones (3.87 us scalar,
// 5.03 us packed for the same arithmetic: tools/probes/valu_gelu.hip, profiles/r06_gemm_epilogues.txt; their throughput with
// independent operands is fine, profiles/r06_valu_rates.txt) -- the file is compiled with -fno-slp-vectorize so that the
// compiler does not form them either.
// quickgelu(u) = u r, r = sigmoid(1.702 u) = 1 / (1 + 2^(-1.702 log2(e) u)); quickgelu'(u) = r (1 + 1.702 u (1 - r))
// = r + 1.702 (u r)(1 - r).
__device__ __forceinline__ float qgelu_grad1(float y, float r) { return fmaf((1.f - r) * y, 1.702f, r); }

// lanes l < 32 and l + 32 hold adjacent 8-byte pieces (4 bf16) of the same output row for two neighbouring
// column groups `a` (columns c..c+3 | c+4..c+7) and `b` (c+8.. | c+12..): one half-swap per dword leaves the
// lower lane with 16 contiguous bytes of group a and the upper lane with 16 contiguous bytes of group b.
__device__ __forceinline__ uint4 widen_pair(uint2 a, uint2 b) {
  const auto r0 = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
  return make_uint4(r0[0], r1[0], r0[1], r1[1]);
}
// The same for the 16x16x32 accumulator map: the four 16-lane groups g = lane >> 4 hold four adjacent 8-byte pieces
// (columns 4g .. 4g+3) of one output row, for two neighbouring 16-column groups `a` and `b`. permlane16_swap exchanges
// the odd 16-lane groups of its first operand with the even ones of its second: group 0 ends with columns 0-7 of a,
// group 1 with columns 0-7 of b, group 2 with columns 8-15 of a, group 3 with columns 8-15 of b -- 16 contiguous bytes
// at column (g & 1) * 16 + (g >> 1) * 8 of the 32.
__device__ __forceinline__ uint4 widen_quad(uint2 a, uint2 b) {
  const auto r0 = __builtin_amdgcn_permlane16_swap(a.x, b.x, false, false);
  const auto r1 = __builtin_amdgcn_permlane16_swap(a.y, b.y, false, false);
  return make_uint4(r0[0], r1[0], r0[1], r1[1]);
}

// Result stores of the epilogue (bf16 path): plain write-back. nt / sc1 / sc0 sc1 stores measured slower on every shape of a
// block (round 6, profiles/r06_gemm_store_policy.txt). What the flavours do on gfx950 (MI355X_MICROARCH.md, "stores of each
// flavour"): plain / nt keep the written line in the XCD's L2, sc1 / sc0 sc1 drop it -- a 256 x 256 tile leaves 128-256 KB
// per workgroup, 4-8 MB per round per XCD, against a 4 MiB L2 that also has to hold the X and W panels.
__device__ __forceinline__ void gm_store16(void* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }

// GM_AUDIT (debug build only, tests/test_gpu_gemm_tails.py): every wave counts the vector-memory stores its epilogue
// ISSUES, at the issue sites, and records them with the vmcnt allowance the next tile's first K blocks use (see NS below).
// Per lane: byte j of gm_aud_st = stores issued in row group j while the lane was live, gm_aud_cp = column-partial stores.
//
// FILL-ORDER AUDIT (same build, tests/test_gpu_gemm_kblocks.py). The store count shows that an allowance is not larger than
// the stores behind it; it does not show that the fill a barrier waits for is OLDER than the operations its vmcnt(N) leaves
// in flight -- the statement that depends on the number of K blocks per tile. Every wave numbers the vector-memory
// operations it certainly issues (aud_seq: each fill, wave 0's bias DMA and counter atomic, the epilogue's stores as counted
// above; the aux_in loads are left out -- an operation that is not counted only makes the fills in front of it older than
// the audit assumes) and keeps, in wave-uniform integers:
//   aud_done        max over every `s_waitcnt vmcnt(N)` written in the kernel of aud_seq - N: operations numbered <= aud_done
//                   have completed (they return in issue order)
//   aud_fill_*[t]   aud_seq after this wave's second fill of slot type t in the ring half, aud_bias*[i & 3] / aud_pull the same
//                   for wave 0's bias image of tile ordinal i and its counter atomic
// and checks `number <= aud_done` where the kernel relies on it (check codes GM_CHK_*): at every GM_BAR for the slot the
// phase behind it reads, at init_acc for the bias image (the drain behind a tail tile's epilogue is entered into aud_done
// only behind that check: the other waves have the image through the last BARRIER behind a wait of wave 0, not through a
// wait of wave 0 alone), at publish for the counter reply, at the epilogue's re-read of xA / wA for both slots.
// A wave's audit header holds {records, violations, code of the first violation, tightest margin aud_done - number seen}.
#ifdef GM_AUDIT
#define GM_AUD(...) __VA_ARGS__
#define GM_AUD_STORE(j) (gm_aud_st += 1u << (8 * (j)))
#define GM_AUD_COLPART() (++gm_aud_cp)
constexpr int GM_AUDIT_CAP = 255;      // records per wave (one per tile boundary)
// first-violation code: 1 << 30 | check << 24 | min(K block, 4095) << 12 | min(tile ordinal, 4095); K block = nb for the
// checks inside and behind an epilogue, tile ordinal = the tile being multiplied or finished
enum { GM_CHK_OPEN_X0 = 0, GM_CHK_OPEN_W0 = 1, GM_CHK_P0_W1 = 2, GM_CHK_P1_X1 = 3, GM_CHK_P2_X0 = 4, GM_CHK_P3_W0 = 5,
       GM_CHK_BIAS = 6, GM_CHK_PULL = 7, GM_CHK_REREAD_X0 = 8, GM_CHK_REREAD_W0 = 9 };
__device__ __forceinline__ int gm_wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
#else
#define GM_AUD(...)
#define GM_AUD_STORE(j) ((void)0)
#define GM_AUD_COLPART() ((void)0)
#endif

// The kernel body; MS = the MFMA shape of the K loop: 32 = v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16 (bf16
// results only). The shape changes three things and nothing else -- which rows and chunks a fragment read takes, the
// MFMAs of a phase (16 instead of 8 for the same 64 x 32 x 64 quadrant; the read and refill slots ride behind every
// second one), and the accumulator map the epilogue and the bias initialisation follow: tile walk, ring, fills, swizzle,
// barriers, allowances, schedules and audit are the same text. The two __global__ wrappers are behind it.
template <int EPI, bool F32O, int MS>
__device__ __forceinline__ void gemm_tn_body(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W,
                                             const float* __restrict__ bias, void* __restrict__ Yv,
                                             void* __restrict__ aux_out_v, const void* __restrict__ aux_in_v,
                                             float* __restrict__ colpart, int64_t M, int N, int K, int tiles_n,
                                             int ntiles, unsigned* __restrict__ sched, int late_mod) {
  static_assert(MS == 32 || (MS == 16 && !F32O), "MFMA shape: 32x32x16, or 16x16x32 for the bf16 results");
  using out_t = std::conditional_t<F32O, float, uint16_t>;      // element type of y / aux_out / aux_in
  out_t* __restrict__ const Y = static_cast<out_t*>(Yv);
  out_t* __restrict__ const aux_out = static_cast<out_t*>(aux_out_v);
  const out_t* __restrict__ const aux_in = static_cast<const out_t*>(aux_in_v);
  extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];      // [NSLOT][128 rows][128 B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nb = K / BK;
  // PERSISTENT workgroups, one per CU: workgroup b sits on XCD b % 8 and works on that XCD's contiguous range
  // [xstart, xstart + cnt) of the N-fastest tile order (bijective for any tile count): at any time the workgroups of
  // an XCD work on neighbouring tiles, so the N/256 tiles that read the same rows of X share one L2.
  //   static schedule (sched == nullptr): tiles xstart + bid/8, + wpx, + 2 wpx, ...
  //   dynamic schedule: tiles xstart + (value of the XCD's counter when the workgroup asked), see the file header.
  const int nx = gridDim.x >= 8 ? 8 : 1;
  const int bid = blockIdx.x, xcd = bid % nx, wpx = gridDim.x / nx;
  const int tq = ntiles / nx, tr = ntiles % nx;
  const int cnt = tq + (xcd < tr ? 1 : 0);
  const int xstart = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
  const bool dyn = sched != nullptr;            // the host passes a counter block only when nb >= DYN_MIN_NB
  if (dyn) __builtin_assume(nb >= DYN_MIN_NB);
  if (!dyn && bid / nx >= cnt) return;
  int my_tiles = dyn ? 0x7fffffff : (cnt - bid / nx + wpx - 1) / wpx;
  int pair_even = xstart + bid / nx, pair_odd = pair_even;    // tile index (N-fastest order) of tile ordinal i, by i & 1
  auto set_pair = [&](int i, int v) { if (i & 1) pair_odd = v; else pair_even = v; };
  auto get_pair = [&](int i) { return (i & 1) ? pair_odd : pair_even; };
  // wave 0 / lane 0 of a dynamic workgroup: the counter reply in flight. Written by the memory system when the atomic
  // returns, NOT at the asm statement that issues it: it is only ever read by `publish` below, behind a vmcnt wait
  // that covers the atomic (tests/test_boundary_cpu.py checks in the ISA that nothing else touches the register).
  uint32_t pend = 0;
  unsigned* const ctr = sched + xcd;
#ifdef GM_AUDIT
  // fill-order audit (see GM_AUDIT above): wave-uniform, scalar registers only
  int aud_seq = 0, aud_done = 0, aud_pull = 0, aud_at = 0;      // aud_at: min(K block, 4095) << 12 | min(tile ordinal, 4095)
  int aud_viol = 0, aud_first = 0, aud_margin = 0x7fffffff;
  int aud_fill_lo[4] = {0, 0, 0, 0}, aud_fill_hi[4] = {0, 0, 0, 0};      // by slot type; ring half 0 / 1
  int aud_bias0 = 0, aud_bias1 = 0, aud_bias2 = 0, aud_bias3 = 0;       // by tile ordinal & 3 (wave 0)
  auto aud_here = [&](int ti, int kb) { aud_at = min(kb, 4095) << 12 | min(ti, 4095); };
  auto aud_wait = [&](int n) { aud_done = max(aud_done, aud_seq - n); };
  auto aud_check = [&](int number, int chk) {
    const int margin = aud_done - number;
    aud_margin = min(aud_margin, margin);
    aud_first = margin < 0 && aud_viol == 0 ? 1 << 30 | chk << 24 | aud_at : aud_first + 0;      // (selects: no new basic blocks)
    aud_viol += margin < 0 ? 1 : 0;
  };
  // (`+ 0`: a conditional of two lvalues is an lvalue -- a select of ADDRESSES, which would put the integers into scratch)
  auto aud_slot = [&](int chk, int type, int half) { aud_check(half ? aud_fill_hi[type] + 0 : aud_fill_lo[type] + 0, chk); };
  auto aud_bias_set = [&](int i) {
    aud_bias0 = (i & 3) == 0 ? aud_seq + 0 : aud_bias0 + 0;
    aud_bias1 = (i & 3) == 1 ? aud_seq + 0 : aud_bias1 + 0;
    aud_bias2 = (i & 3) == 2 ? aud_seq + 0 : aud_bias2 + 0;
    aud_bias3 = (i & 3) == 3 ? aud_seq + 0 : aud_bias3 + 0;
  };
  auto aud_bias_get = [&](int i) {
    const int odd = (i & 1) ? aud_bias1 + 0 : aud_bias0 + 0, odd2 = (i & 1) ? aud_bias3 + 0 : aud_bias2 + 0;
    return (i & 2) ? odd2 + 0 : odd + 0;
  };
#endif
  // (lane 0 only: EXEC is narrowed inside the asm -- a divergent C++ branch here would make the compiler treat the
  // loop-carried tile cursor as divergent and move the DMA base addresses into vector registers)
  uint64_t exec_save;
  auto pull = [&]() {
    if (wave == 0) {
      asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
                   : "=v"(pend), "=&s"(exec_save) : "v"(0u), "v"(1u), "s"(ctr) : "memory");
      GM_AUD(aud_pull = ++aud_seq;)
    }
  };
  auto publish = [&]() {
    if (wave == 0) {
      GM_AUD(aud_check(aud_pull, GM_CHK_PULL);)
      asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_write_b32 %1, %2\n\ts_mov_b64 exec, %0"
                   : "=&s"(exec_save) : "v"((uint32_t)(uintptr_t)smem + MBOX_OFF), "v"(pend) : "memory");
    }
  };
  // (an LDS read in asm: through a volatile C++ pointer the compiler emits a FLAT load and waits vmcnt(0) for it -- a
  // full drain of the run-ahead fills once per tile, 2-4 % of a launch on the dynamic schedule until round 6)
  auto mailbox = [&]() -> int {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"((uint32_t)(uintptr_t)smem + MBOX_OFF) : "memory");
    return __builtin_amdgcn_readfirstlane(v);
  };
  const bool late = dyn && late_mod > 0 && bid % late_mod == 1;      // test hook (lvl_debug_late_workgroups)
  // first tile: the one synchronous hand-out of a launch. Requested here, consumed behind the address set-up below
  // (nothing else is in flight yet, so the round trip overlaps ~1 us of scalar / vector arithmetic).
  if (dyn && !late) pull();

  // Tile order: all N/256 column tiles of a row block are neighbours (N-fastest). (Panels of 3-6 column tiles, to keep
  // a weight panel L2-resident, measured no faster: the weight re-reads are served by the Infinity Cache.)
  auto decode_tile = [&](int pair, int& tm, int& tn) {
    tm = pair / tiles_n;
    tn = pair - tm * tiles_n;
  };

  // ---- LDS-DMA plan -----------------------------------------------------------------------------------------------
  // A slot is 16 fills of 1 KiB (8 rows x 128 B); wave w issues fills w and w+8 of every slot. Lane l of fill f
  // lands at slot byte f*1024 + l*16 = slot row 8f + (l>>3), physical chunk l&7, and therefore fetches the LOGICAL
  // chunk (l&7) ^ ((row>>1)&7) of its row. Slot rows: X slot q = tile rows q*128 + r; W slot q = tile columns
  // (r>>5)*64 + q*32 + (r&31) (the two 32-column groups of every wave's 64 output columns go to different halves).
  // Per-lane sources are 32-bit byte offsets relative to the tile; the tile and the K block ride in scalars.
  uint32_t xrel[4], wrel[2], xclamp;
  {
    const int sub = lane >> 3;
    const int chunk = (lane & 7) ^ ((4 * wave + (sub >> 1)) & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int lr = 8 * (wave + 8 * h) + sub;
#pragma unroll
      for (int q = 0; q < 2; ++q) xrel[q * 2 + h] = (uint32_t)(q * 128 + lr) * (uint32_t)(K * 2) + chunk * 16;
      wrel[h] = (uint32_t)((lr >> 5) * 64 + (lr & 31)) * (uint32_t)(K * 2) + chunk * 16;
    }
    xclamp = (uint32_t)((M - 1) * K * 2) + chunk * 16;       // tail tile: re-read the last row (never stored)
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  // fetch cursor: the K block the next refills bring in (two blocks ahead of the one being multiplied)
  int f_i = 0, f_j = 0;
  uint32_t f_xrow;                 // byte offset of the fetch tile's first X row
  const char* f_wbase;             // first W row of the fetch tile
  auto fetch_tile = [&](int i) {
    if (!dyn) set_pair(i, xstart + bid / nx + i * wpx);
    const int pair = __builtin_amdgcn_readfirstlane(get_pair(i));
    int tm, tn;
    decode_tile(pair, tm, tn);
    f_xrow = (uint32_t)tm * (uint32_t)(TM * K * 2);
    f_wbase = reinterpret_cast<const char*>(W) + (int64_t)tn * TN * K * 2;
    if (EPI != 2 && EPI != 7 && bias != nullptr && wave == 0) {
      // the tile's 256 bias values travel the same way (one 1-KiB LDS-DMA by wave 0, >= 8 phases before the
      // epilogue that reads them): the epilogue then issues no vector-memory LOAD, so nothing in it has to wait
      // for the run-ahead fills or for its own stores
      const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds0 + BIAS_OFF + (uint32_t)(i & 3) * 1024);
      const uint32_t off = (uint32_t)lane * 16;
      const char* base = reinterpret_cast<const char*>(bias + tn * TN);
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(off), "s"(base)
                   : "memory", "m0");
      GM_AUD(++aud_seq; aud_bias_set(i);)
    }
  };
  auto fetch_advance = [&]() {
    if (++f_j == nb) {
      if (dyn && f_i + 1 < my_tiles) {
        // the reply wave 0 published at K block 2 of the tile being multiplied (>= 4 barriers ago)
        const int v = mailbox();
        if (v < cnt) {
          set_pair(f_i + 1, xstart + v);
        } else {
          my_tiles = f_i + 1;      // the XCD's queue is drained
        }
      }
      if (f_i + 1 < my_tiles) {
        f_j = 0;
        fetch_tile(++f_i);
      } else {
        f_j = nb - 1;              // past the end: keep re-reading the last block (never consumed)
      }
    }
  };
  // Fills go through inline asm: the compiler's LDS-DMA alias tracking would otherwise put s_waitcnt vmcnt(0) in
  // front of every LDS read and drain the run-ahead.
  auto issue_fill = [&](int type, int par, int h) {
    const char* base = type < S_W0 ? reinterpret_cast<const char*>(X) + (int64_t)f_j * (BK * 2)
                                   : f_wbase + (int64_t)f_j * (BK * 2) + (type == S_W1 ? (int64_t)32 * K * 2 : 0);
    uint32_t off;
    if (type < S_W0) {
      off = xrel[type * 2 + h] + f_xrow;
      off = off < xclamp ? off : xclamp;
    } else {
      off = wrel[h];
    }
    const uint32_t m0v =
        __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(par + type) * SLOT + (uint32_t)wave * 1024 + h * 8192);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(off), "s"(base)
                 : "memory", "m0");
    GM_AUD(++aud_seq; if (h == 1) {
      aud_fill_hi[type] = par ? aud_seq + 0 : aud_fill_hi[type] + 0;
      aud_fill_lo[type] = par ? aud_fill_lo[type] + 0 : aud_seq + 0;
    })
  };
  auto issue_group = [&](int type, int par) {
    issue_fill(type, par, 0);
    issue_fill(type, par, 1);
  };

  // ---- fragment addresses -----------------------------------------------------------------------------------------
  // 32x32x16 operand: lane l carries row (l & 31), contraction elements 8*(l>>5) .. +7 of the K=16 slice kk, i.e.
  // logical chunk 2*kk + (l>>5) of the row's eight 16-byte chunks.
  // 16x16x32 operand: lane l carries row (l & 15), contraction elements 8*(l>>4) .. +7 of the K=32 slice ks, i.e. logical
  // chunk 4*ks + (l>>4). A wave's share of a slot is the same 8 X / 4 W fragments: X fragment ks*4 + rg = rows 16 rg .. +15
  // of its 64, W fragment ks*2 + cg = rows 16 cg .. +15 of its 32.
  // SWIZZLE, both shapes: physical chunk = logical chunk ^ ((row>>1) & 7). A ds_read_b128 is served in four groups of 16
  // lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- and a group is conflict-free when its 16 lanes
  // hit 16 different 16-byte columns of the 256-byte bank row, column = 8 (row & 1) + physical chunk: the 8 rows of one
  // parity need 8 different physical chunks. 32x32x16: a group is 16 consecutive rows of one logical chunk c; per parity
  // (row>>1) & 7 takes all 8 values, so does c ^ it. 16x16x32: a group is rows 0-3 and 12-15 with logical chunk c and rows
  // 4-11 with c ^ 1, or the other way round (lanes 16 apart differ in bit 0 of l>>4; the upper two groups: c ^ 2, c ^ 3); per parity
  // q = (row>>1) & 7 is {0, 1, 6, 7} under c and {2, 3, 4, 5} under c ^ 1, physical chunks c ^ {0, 1, 6, 7} and
  // c ^ {3, 2, 5, 4}: all 8 again. The fill side is therefore the same for both shapes. (Without the swizzle, or with a
  // swizzle on bits the lane groups do not separate, this read is 2-way.)
  const int r5 = MS == 16 ? lane & 15 : lane & 31, hi = MS == 16 ? lane >> 4 : lane >> 5;
  const int r5_ = r5, hi_ = hi;
  uint32_t xa[4], wa[4];
#pragma unroll
  for (int kk = 0; kk < (MS == 16 ? 2 : 4); ++kk) {
    const int offk = (((MS == 16 ? 4 : 2) * kk + hi) ^ ((r5 >> 1) & 7)) * 16;
    xa[kk] = (uint32_t)((wm * 64 + r5) * 128 + offk);
    wa[kk] = (uint32_t)((wn * 32 + r5) * 128 + offk);
  }
  // slot byte offset of the lane's share of X fragment k (0..7) / W fragment k (0..3)
  auto x_off = [&](int k) { return MS == 16 ? xa[k >> 2] + (k & 3) * 2048 : xa[k & 3] + (k >> 2) * 4096; };
  auto w_off = [&](int k) { return MS == 16 ? wa[k >> 1] + (k & 1) * 2048 : wa[k]; };
  auto read_x = [&](int slot, uint4 (&xf)[8]) {
    const uint8_t* b = smem + slot * SLOT;
#pragma unroll
    for (int k = 0; k < 8; ++k) xf[k] = *reinterpret_cast<const uint4*>(b + x_off(k));
  };
  auto read_w = [&](int slot, uint4 (&wf)[4]) {
    const uint8_t* b = smem + slot * SLOT;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) wf[kk] = *reinterpret_cast<const uint4*>(b + w_off(kk));
  };

  gm_f32x16 acc[2][2][2];           // [qm][qn][mt]
  gm_f32x4 acc4[2][2][4][2];        // MS == 16: [qm][qn][rg][cg], 16 rows x 16 columns each (the same 128 registers)
  // The accumulators of tile ti START as the tile's bias (read straight from its LDS image into the accumulator
  // registers: no VALU work), so the epilogue has no bias add; without a bias they start at zero.
  auto init_acc = [&](int ti) {
    if constexpr (MS == 16) {
      // accumulator [rg][cg] of column group qn: the lane holds columns qn*32 + cg*16 + 4*hi .. +3 of row rg*16 + r5
      if (EPI != 2 && bias != nullptr) {
        const uint8_t* bias_img = smem + BIAS_OFF + (ti & 3) * 1024;
        GM_AUD(if (wave == 0) aud_check(aud_bias_get(ti), GM_CHK_BIAS);)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int cg = 0; cg < 2; ++cg) {
            const float4 b = *reinterpret_cast<const float4*>(bias_img + (wn * 64 + i * 32 + cg * 16 + 4 * hi) * 4);
#pragma unroll
            for (int a = 0; a < 8; ++a) {
              acc4[a >> 2][i][a & 3][cg][0] = b.x;
              acc4[a >> 2][i][a & 3][cg][1] = b.y;
              acc4[a >> 2][i][a & 3][cg][2] = b.z;
              acc4[a >> 2][i][a & 3][cg][3] = b.w;
            }
          }
      } else {
#pragma unroll
        for (int a = 0; a < 32; ++a)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc4[a >> 4][(a >> 3) & 1][(a >> 1) & 3][a & 1][r] = 0.f;
      }
    } else
    if (EPI != 2 && EPI != 7 && bias != nullptr) {
      const uint8_t* bias_img = smem + BIAS_OFF + (ti & 3) * 1024;
      GM_AUD(if (wave == 0) aud_check(aud_bias_get(ti), GM_CHK_BIAS);)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float4 b = *reinterpret_cast<const float4*>(bias_img + (wn * 64 + i * 32 + 8 * rq + 4 * hi) * 4);
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            acc[a >> 1][i][a & 1][4 * rq + 0] = b.x;
            acc[a >> 1][i][a & 1][4 * rq + 1] = b.y;
            acc[a >> 1][i][a & 1][4 * rq + 2] = b.z;
            acc[a >> 1][i][a & 1][4 * rq + 3] = b.w;
          }
        }
    } else {
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a >> 2][(a >> 1) & 1][a & 1][r] = 0.f;
    }
  };

  uint4 xA[8], xB[8], wA[4], wB[4];      // operand fragments of the K loop (declared here: the epilogue re-reads xA / wA)
  int par = 0;                            // ring half (slot offset 0 / 4) of the K block being multiplied
#ifdef GM_AUDIT
  uint32_t gm_aud_st = 0, gm_aud_cp = 0;
#endif

  auto epilogue = [&](int tm, int tn, int ti) {
    const int64_t m0 = (int64_t)tm * TM;
    const int n0 = tn * TN;
    // the lane's row / column-half as the epilogue sees them: opaque copies, so that the per-lane 64-bit row offsets
    // (tile-invariant: (wm*64 + r5) * N + ...) are computed here, per tile, instead of being hoisted out of the tile
    // loop into registers the K loop does not have (they were spilled, and reloaded BEHIND the result stores)
    int r5 = r5_, hi = hi_;
    asm volatile("" : "+v"(r5), "+v"(hi));
    constexpr bool COLSUM = EPI == 2 || EPI == 5 || EPI == 7;                 // column sums of y leave as a partial slab
    constexpr bool AUXIN = EPI == 2 || EPI == 3 || EPI == 5 || EPI == 7;      // an aux_in row rides with every result row
    constexpr bool TWO_OUT = EPI == 1 || EPI == 4 || EPI == 6 || EPI == 8;
    // value c = column (c>>4)*32 + ((c>>2)&3)*8 + 4*hi + (c&3) of the wave's 64. MS == 16: a lane holds 16 of the 64
    // columns, but two rows of every 32-row group (h*16 + r5): value h*16 + c = column (c>>3)*32 + ((c>>2)&1)*16 + 4*hi +
    // (c&3) of the rows of half h. Kept apart per half, so that the sums are formed in the ORDER of the 32x32x16 map -- per
    // row of the 32 first over the four row groups, then rows r and r + 16, then the butterfly over 16 lanes -- and the
    // column sums of the two shapes are the same floats, not only the same to rounding.
    constexpr int NCS = 32;
    float csum[COLSUM ? NCS : 1];
    if (COLSUM) {
#pragma unroll
      for (int c = 0; c < NCS; ++c) csum[c] = 0.f;
    }
    // One accumulator quad -- 4 consecutive output columns of one row, v -- through the epilogue's arithmetic: the packed
    // bf16 result comes back, the second output of the two-output epilogues goes to upk; ab = the lane's 8 bytes of the
    // aux_in row, rowv = 0 for a row behind M, ci = the quad's first column-sum value.
    auto finish_quad = [&](float (&v)[4], const uint2 ab, const float rowv, const int ci, uint2& upk) -> uint2 {
      if (EPI == 1) {
        upk = make_uint2(f32x2_to_bf16x2(v[0], v[1]), f32x2_to_bf16x2(v[2], v[3]));
        // the activation sees the ROUNDED pre-activation (what the reference's bf16 Linear output holds and
        // what the backward reads back)
        float r;
        qgelu1(bf16_lo(upk.x), v[0], r);
        qgelu1(bf16_hi(upk.x), v[1], r);
        qgelu1(bf16_lo(upk.y), v[2], r);
        qgelu1(bf16_hi(upk.y), v[3], r);
      }
      if (EPI == 6) {                // epilogue 1 with the exact GELU (gelu_erf.h), on the ROUNDED pre-activation too
        upk = make_uint2(f32x2_to_bf16x2(v[0], v[1]), f32x2_to_bf16x2(v[2], v[3]));
        v[0] = gelu_erf(bf16_lo(upk.x));
        v[1] = gelu_erf(bf16_hi(upk.x));
        v[2] = gelu_erf(bf16_lo(upk.y));
        v[3] = gelu_erf(bf16_hi(upk.y));
      }
      if (EPI == 8) {                // y = gelu(u), aux_out = gelu'(u) = Phi(u) + u phi(u): one erf serves both
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) gelu_erf_pair(v[e], v[e], g[e]);
        upk = make_uint2(f32x2_to_bf16x2(g[0], g[1]), f32x2_to_bf16x2(g[2], g[3]));
      }
      if (EPI == 4) {                // y = quickgelu(u), aux_out = quickgelu'(u): one exp2 + one rcp serve both
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float y, r;
          qgelu1(v[e], y, r);
          g[e] = qgelu_grad1(y, r);
          v[e] = y;
        }
        upk = make_uint2(f32x2_to_bf16x2(g[0], g[1]), f32x2_to_bf16x2(g[2], g[3]));
      }
      if (AUXIN) {
        const float a4[4] = {bf16_lo(ab.x), bf16_hi(ab.x), bf16_lo(ab.y), bf16_hi(ab.y)};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (EPI == 3) v[e] += a4[e];        // + the residual row (bf16), in f32 before the one rounding of the sum
          if (EPI == 5) v[e] *= a4[e];        // the forward left quickgelu'(u) itself
          if (EPI == 2) {
            float y, r;
            qgelu1(a4[e], y, r);
            v[e] *= qgelu_grad1(y, r);
          }
          if (EPI == 7) v[e] *= gelu_erf_grad(a4[e]);
        }
      }
      if (COLSUM) {
#pragma unroll
        for (int e = 0; e < 4; ++e) csum[ci + e] = fmaf(v[e], rowv, csum[ci + e]);
        // erff's branches cut the epilogue into basic blocks, and the compiler then sinks the whole chain of these
        // fmas into the last one -- four row groups of products stay live instead of 32 sums (15 VGPRs spilled): the sum
        // is made opaque here, per accumulator quad, so it is formed here
        if (EPI == 7) {
#pragma unroll
          for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(csum[ci + e]));
        }
      }
      return make_uint2(f32x2_to_bf16x2(v[0], v[1]), f32x2_to_bf16x2(v[2], v[3]));
    };
    if constexpr (F32O) {
      // float32 results (f32-class mode): an accumulator quad IS 4 consecutive output columns of one row -> one
      // 16-byte store per quad (and one 16-byte aux access for the QuickGELU epilogues); same arithmetic as below
      // without the bf16 roundings
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t m = m0 + (j >> 1) * 128 + wm * 64 + (j & 1) * 32 + r5;
        const bool valid = m < M;
        const int64_t rowoff = (valid ? m : M - 1) * (int64_t)N + n0 + wn * 64 + 4 * hi;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const gm_f32x16& a16 = acc[j >> 1][i][j & 1];
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const int64_t o = rowoff + i * 32 + 8 * rq;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = a16[4 * rq + e];
            if (EPI == 1 || EPI == 6) {
              if (valid) {
                *reinterpret_cast<float4*>(aux_out + o) = make_float4(v[0], v[1], v[2], v[3]);
                GM_AUD_STORE(j);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = EPI == 1 ? quick_gelu(v[e]) : gelu_erf(v[e]);
            }
            if (EPI == 3) {
              const float4 r = *reinterpret_cast<const float4*>(aux_in + o);
              v[0] += r.x;
              v[1] += r.y;
              v[2] += r.z;
              v[3] += r.w;
            }
            if (EPI == 2 || EPI == 7) {
              const float4 u = *reinterpret_cast<const float4*>(aux_in + o);
              v[0] *= EPI == 2 ? quick_gelu_grad(u.x) : gelu_erf_grad(u.x);
              v[1] *= EPI == 2 ? quick_gelu_grad(u.y) : gelu_erf_grad(u.y);
              v[2] *= EPI == 2 ? quick_gelu_grad(u.z) : gelu_erf_grad(u.z);
              v[3] *= EPI == 2 ? quick_gelu_grad(u.w) : gelu_erf_grad(u.w);
              if (valid) {
#pragma unroll
                for (int e = 0; e < 4; ++e) csum[i * 16 + rq * 4 + e] += v[e];
              }
            }
            if (valid) {
              *reinterpret_cast<float4*>(Y + o) = make_float4(v[0], v[1], v[2], v[3]);
              GM_AUD_STORE(j);
            }
          }
        }
      }
    } else {
    // bf16 results. The hardware's vmcnt counts result stores; the compiler's wait insertion does not count stores that sit
    // under a branch (the `m < M` guard: its counters are merged conservatively across it): a wait it
    // places for an aux_in load (residual stream / QuickGELU derivative / pre-activation rows) BEHIND a group's stores is
    // too strict by the number of those stores and waits for their acknowledgement -- one store drain per row group, +10 us
    // per tile with the loads one group ahead of the stores (round 6: proj + residual 0.34 ms against 0.23 ms for the plain
    // epilogue on the same shape). So the aux rows of ALL FOUR row groups are requested, and every one of them has landed
    // (`landed`: a register use the compiler has to wait for), before the first store leaves; from there on nothing is
    // pending and packing and stores interleave freely. Registers: UPFRONT groups are requested at once, the rest when
    // group 0 is packed and its accumulators are dead; HOLD groups are packed before the first store; the next tile's
    // first fragments (xA / wA, read during the last K block) are not carried across the epilogue but read again from the
    // ring under the last stores (the column-sum epilogues hold 32 running sums on top of the aux rows).
    constexpr int UPFRONT = COLSUM ? 3 : 4;
    constexpr int HOLD = UPFRONT == 4 ? 1 : 2;
    uint2 ub[AUXIN ? 4 : 1][8];
    auto load_u = [&](int j, uint2 (&dst)[8]) {
      if constexpr (MS == 16) {       // [h*4 + qn*2 + cg]: the lane's 8 bytes of row h*16 + r5 in every 16-column group
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t m = m0 + (j >> 1) * 128 + wm * 64 + (j & 1) * 32 + h * 16 + r5;
          const uint16_t* urow = reinterpret_cast<const uint16_t*>(aux_in) + (m < M ? m : M - 1) * (int64_t)N + n0 + wn * 64 + 4 * hi;
#pragma unroll
          for (int q = 0; q < 4; ++q) dst[h * 4 + q] = *reinterpret_cast<const uint2*>(urow + 16 * q);
        }
      } else {
      const int64_t m = m0 + (j >> 1) * 128 + wm * 64 + (j & 1) * 32 + r5;
      const uint16_t* urow = reinterpret_cast<const uint16_t*>(aux_in) + (m < M ? m : M - 1) * (int64_t)N + n0 + wn * 64 + 4 * hi;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) dst[i * 4 + rq] = *reinterpret_cast<const uint2*>(urow + i * 32 + 8 * rq);
      }
    };
    auto landed = [&](const uint2 (&src)[8]) {
#pragma unroll
      for (int q = 0; q < 8; ++q) asm volatile("" ::"v"(src[q].x), "v"(src[q].y));
    };
    if constexpr (AUXIN) {
#pragma unroll
      for (int j = 0; j < UPFRONT; ++j) load_u(j, ub[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
    uint4 yv[AUXIN ? HOLD : 1][2][2], uv[2][2];      // [row group][qn][jj]: 16 bytes = columns qn*32 + 16*jj + 8*hi .. +7 of row r5
    // MS == 16: [row group][h][qn]: 16 bytes = columns qn*32 + (hi&1)*16 + (hi>>1)*8 .. +7 of row h*16 + r5 (widen_quad)
    auto store_group = [&](int j, const uint4 (&y4)[2][2]) {
      // 16-byte stores: lower lanes take columns 16*jj .. +7, upper lanes 16*jj + 8 .. +15 of a column group
      // (an LDS-staged variant that leaves as full 128-byte lines measured no faster: the tail is not line-bound)
      if constexpr (MS == 16) {
        // the row guard is per 16-row group: the same 4 (8) stores per 32 rows, from two guarded halves
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t m = m0 + (j >> 1) * 128 + wm * 64 + (j & 1) * 32 + h * 16 + r5;
          if (m < M) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const int64_t o = m * (int64_t)N + n0 + wn * 64 + i * 32 + (hi & 1) * 16 + (hi >> 1) * 8;
              gm_store16(Y + o, y4[h][i]);
              GM_AUD_STORE(j);
              if (TWO_OUT) {
                gm_store16(aux_out + o, uv[h][i]);
                GM_AUD_STORE(j);
              }
            }
          }
        }
      } else {
      const int64_t m = m0 + (j >> 1) * 128 + wm * 64 + (j & 1) * 32 + r5;
      if (m < M) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int64_t o = m * (int64_t)N + n0 + wn * 64 + i * 32 + 16 * jj + 8 * hi;
            gm_store16(Y + o, y4[i][jj]);
            GM_AUD_STORE(j);
            if (TWO_OUT) {
              gm_store16(aux_out + o, uv[i][jj]);
              GM_AUD_STORE(j);
            }
          }
      }
      }
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // row group (qm, mt): 32 rows
      const int64_t mg = m0 + (j >> 1) * 128 + wm * 64 + (j & 1) * 32;
      const float rowv = mg + r5 < M ? 1.f : 0.f;      // rows behind M (tail tile) stay out of the column sums
      uint4 (&y4)[2][2] = yv[AUXIN && j < HOLD ? j : 0];
      if constexpr (MS == 16) {
        // two 16-row groups h; per column group qn two accumulators cg of 16 columns, one quad each
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float rowh = mg + h * 16 + r5 < M ? 1.f : 0.f;
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            uint2 ypk[2], upk[2];
#pragma unroll
            for (int cg = 0; cg < 2; ++cg) {
              const gm_f32x4& a4 = acc4[j >> 1][i][(j & 1) * 2 + h][cg];
              float v[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = a4[e];
              uint2 ab = make_uint2(0u, 0u);
              if (AUXIN) ab = ub[j][h * 4 + i * 2 + cg];
              ypk[cg] = finish_quad(v, ab, rowh, h * 16 + i * 8 + cg * 4, upk[cg]);
            }
            y4[h][i] = widen_quad(ypk[0], ypk[1]);
            if (TWO_OUT) uv[h][i] = widen_quad(upk[0], upk[1]);
          }
        }
      } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {        // column group qn
        const gm_f32x16& a16 = acc[j >> 1][i][j & 1];
        uint2 ypk[4], upk[4];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = a16[4 * rq + e];
          uint2 ab = make_uint2(0u, 0u);
          if (AUXIN) ab = ub[j][i * 4 + rq];
          ypk[rq] = finish_quad(v, ab, rowv, i * 16 + rq * 4, upk[rq]);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          y4[i][jj] = widen_pair(ypk[2 * jj], ypk[2 * jj + 1]);
          if (TWO_OUT) uv[i][jj] = widen_pair(upk[2 * jj], upk[2 * jj + 1]);
        }
      }
      }
      if constexpr (AUXIN) {
        if (j == 0 && UPFRONT < 4) {
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int jn = UPFRONT; jn < 4; ++jn) load_u(jn, ub[jn]);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (j == HOLD - 1) {               // every aux row has landed: stores may leave
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int jn = HOLD; jn < 4; ++jn) landed(ub[jn]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int jp = 0; jp < HOLD; ++jp) store_group(jp, yv[jp]);
        }
        if (j == 3) {                      // re-read of xA / wA
          __builtin_amdgcn_sched_barrier(0);
          GM_AUD(aud_slot(GM_CHK_REREAD_X0, S_X0, par); aud_slot(GM_CHK_REREAD_W0, S_W0, par);)
          read_x(par + S_X0, xA);
          read_w(par + S_W0, wA);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (j >= HOLD) store_group(j, y4);
      } else {
        store_group(j, y4);
      }
    }
    }
    if (COLSUM) {
      // column sums over the wave's 128 rows: 32 values per lane, summed over the 32 lanes of each half-wave by a
      // halving butterfly (31 exchanges): lane r5 ends up with the total of value index c = r5. MS == 16: the exchange
      // over mask 16 (rows r and r + 16) is the add of the lane's own two halves, the other 15 exchanges run over the 16
      // lanes of each quarter-wave.
      float (&cs)[COLSUM ? NCS : 1] = csum;
      int cnt2 = NCS / 2;
      if constexpr (MS == 16) {
#pragma unroll
        for (int c = 0; c < 16; ++c) cs[c] = cs[c] + cs[c + 16];
        cnt2 = 8;
      }
#pragma unroll
      for (int mask = MS == 16 ? 8 : 16; mask >= 1; mask >>= 1) {
        const bool up = (lane & mask) != 0;
#pragma unroll
        for (int c = 0; c < NCS / 2; ++c) {
          if (c < cnt2) {
            const float lo = cs[c], hv = cs[c + cnt2];
            const float send = up ? lo : hv, keep = up ? hv : lo;
            cs[c] = keep + __shfl_xor(send, mask, 64);
          }
        }
        cnt2 >>= 1;
      }
      const int c = r5;
      const int col = MS == 16 ? (c >> 3) * 32 + ((c >> 2) & 1) * 16 + 4 * hi + (c & 3)
                               : (c >> 4) * 32 + ((c >> 2) & 3) * 8 + 4 * hi + (c & 3);
      colpart[(size_t)(tm * 2 + wm) * N + n0 + wn * 64 + col] = cs[0];
      GM_AUD_COLPART();
    }
  };

#ifdef GM_TRACE
  // debug build only (tools/probe_gemm_trace.py): wall-clock stamps (100 MHz) of wave 0 and wave 4 of every workgroup
  // (the column-sum epilogues keep their partial slab in front of the stamps: [2 * tiles_m][N] floats)
  unsigned long long* trace = reinterpret_cast<unsigned long long*>(colpart + ((EPI == 2 || EPI == 5 || EPI == 7) ? (size_t)2 * (ntiles / tiles_n) * N : 0)) +
                              ((size_t)bid * 2 + wm) * 128;
  int tpos = 0;
#define GM_STAMP()                                                          \
  do {                                                                      \
    if (wn == 0 && lane == 0 && tpos < 64) {                                \
      trace[64 + tpos] = __builtin_readcyclecounter();                      \
      trace[tpos++] = wall_clock64();                                       \
    }                                                                       \
  } while (0)
#else
#define GM_STAMP() do { } while (0)
#endif
#ifdef GM_AUDIT
  // [gridDim.x][8 waves][1 + GM_AUDIT_CAP][4] ints behind the column partials (as GM_TRACE): a header {records, fill-order
  // violations, code of the first one, tightest margin (0x7fffffff: the wave made no check)} and, for every tile ordinal
  // i >= 1, {tm, tn of tile i-1, stores the wave issued in tile i-1's epilogue, allowance used}
  int* const audit = reinterpret_cast<int*>(colpart + ((EPI == 2 || EPI == 5 || EPI == 7) ? (size_t)2 * (ntiles / tiles_n) * N : 0)) +
                     ((size_t)bid * 8 + wave) * (1 + GM_AUDIT_CAP) * 4;
  int aud_n = 0, aud_rec[4] = {0, 0, 0, 0};
#endif
  if (late) {
    my_tiles = 0;                               // as if the queues were drained
  } else if (dyn) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GM_AUD(aud_wait(0);)
    publish();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int v = mailbox();
    if (v >= cnt) my_tiles = 0;                 // queue already drained (this workgroup got its CU late)
    pair_even = xstart + v;
    __builtin_amdgcn_s_barrier();               // everyone has read the mailbox before it is written again
    if (my_tiles) pull();                       // tile 1: the reply lands during the prologue fills and tile 0's first blocks
  }
  GM_STAMP();
  if (my_tiles > 0) {
  fetch_tile(0);
#pragma unroll
  for (int b0 = 0; b0 < 2; ++b0) {         // blocks 0 and 1, groups in the order the phases will read them
    issue_group(S_X0, b0 * 4);
    issue_group(S_W0, b0 * 4);
    issue_group(S_W1, b0 * 4);
    issue_group(S_X1, b0 * 4);
    fetch_advance();
  }
  // LOCKSTEP schedule. All 8 waves run the same phase; ONE barrier per phase. A phase = 8 MFMAs per wave with, riding
  // between them, the fragment reads of the operand the NEXT phase needs and this phase's refill DMAs; the two waves
  // of a SIMD interleave freely inside a phase, so one wave's LDS / DMA issue hides under the other's MFMAs:
  //   P0 = X0.W0  reads W1(j)            no refill
  //   P1 = X0.W1  reads X1(j)            refills X0(j), W0(j) <- block j+2   (both consumed in P0)
  //   P2 = X1.W1  reads X0(j+1)          refills W1(j)        <- block j+2   (consumed in P1)
  //   P3 = X1.W0  reads W0(j+1)          refills X1(j)        <- block j+2   (consumed in P2)
  // (W0 fragment k is re-read right after its last use in P3.) A slot is refilled only after a barrier that follows
  // the phase in which every wave CONSUMED its fragments (the compiler's lgkmcnt wait in front of the consuming MFMA
  // is the completion of the read), and is read again 5-6 phases after the refill. Before each barrier a wave waits
  // until the fills of the slot the next phase reads have landed: fills return in order, so "all but the N newest
  // vector-memory operations" with N = the operations issued after that slot's fills (10 / 8 / 10 / 10 for P0..P3;
  // the bias image and the epilogue's stores only make the wait stricter). The barrier is the bare s_barrier: a
  // fence would drain the run-ahead fills. (CHK: the GM_AUDIT build's check of the slot(s) the phase behind the barrier
  // reads; dropped from every other build.)
#define GM_BAR(N, CHK)                                                \
  do {                                                                \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");          \
    GM_AUD(aud_wait(N); CHK;)                                         \
    __builtin_amdgcn_s_barrier();                                     \
    asm volatile("" ::: "memory");                                    \
    __builtin_amdgcn_sched_barrier(0);                                \
  } while (0)
  // 8 MFMAs; after MFMA k: rd(k) (one fragment read) and dm(k) (one refill DMA or nothing)
#define GM_PHASE32(xf, wf, c, rd, dm)                                                                     \
  do {                                                                                                    \
    _Pragma("unroll") for (int kk = 0; kk < 4; ++kk) {                                                    \
      _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) {                                                  \
        c[mt] = mfma32(wf[kk], xf[mt * 4 + kk], c[mt]);                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        rd(kk * 2 + mt);                                                                                  \
        dm(kk * 2 + mt);                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                \
      }                                                                                                   \
    }                                                                                                     \
  } while (0)
  // MS == 16: 16 MFMAs of half the cycles each; slot s = 0..7 is two of them and rd(s) / dm(s) ride behind the second, so a
  // phase carries the reads and refills of GM_PHASE32 at the same places in time. Slot s multiplies W fragment s >> 1
  // (K = 32 slice s >> 2, 16 columns cg = (s >> 1) & 1) with the X fragments of row groups 2 (s & 1), 2 (s & 1) + 1 of that
  // slice: W fragment kk has been used for the last time behind slot 2 kk + 1, as rd_w0 needs it.
#define GM_PHASE16(xf, wf, c, rd, dm)                                                                     \
  do {                                                                                                    \
    _Pragma("unroll") for (int s = 0; s < 8; ++s) {                                                       \
      _Pragma("unroll") for (int h = 0; h < 2; ++h) {                                                     \
        const int rg = (s & 1) * 2 + h, cg = (s >> 1) & 1;                                                \
        c[rg][cg] = mfma16(wf[s >> 1], xf[(s >> 2) * 4 + rg], c[rg][cg]);                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
      }                                                                                                   \
      rd(s);                                                                                              \
      dm(s);                                                                                              \
      __builtin_amdgcn_sched_barrier(0);                                                                  \
    }                                                                                                     \
  } while (0)
#define GM_PHASE(xf, wf, qm, qn, rd, dm)                                  \
  do {                                                                    \
    if constexpr (MS == 16) GM_PHASE16(xf, wf, acc4[qm][qn], rd, dm);     \
    else GM_PHASE32(xf, wf, acc[qm][qn], rd, dm);                         \
  } while (0)
  GM_BAR(12, (aud_slot(GM_CHK_OPEN_X0, S_X0, 0), aud_slot(GM_CHK_OPEN_W0, S_W0, 0)));      // X0 and W0 of block 0 have landed
  read_x(S_X0, xA);
  read_w(S_W0, wA);
  __builtin_amdgcn_sched_barrier(0);
  GM_STAMP();
  init_acc(0);
  // One K block = four phases. A0 / A1 are added to the vmcnt allowance of the barriers in front of P0,P1 / P2,P3:
  // vector-memory operations retire in issue order, so in the first block(s) after an epilogue -- while the slot a
  // barrier waits for was still filled BEFORE that epilogue -- the epilogue's result stores sit between the awaited
  // fills and the newer ones and may stay in flight (waiting for them to be acknowledged would cost every tile ~2 us of
  // idle matrix pipe).
  // INVARIANT: the allowance a wave uses after an epilogue is at most the number of vector-memory stores THAT WAVE
  // issued in it (otherwise "all but the newest 10 + NS" lets some of the awaited fills still be in flight when the
  // barrier opens and all eight waves read the slot). A full tile issues NS per wave (epilogues 2 / 5 / 7: 16 + the column
  // partial). In a TAIL tile (m0 + TM > M) the stores of a 32-row group wholly at or behind M are skipped (`m < M`): a
  // wave may issue fewer than NS, or none. So after a tail tile's epilogue every wave drains (vmcnt(0)) and the
  // allowance is 0 -- one store drain per tail tile, only there. The GM_AUDIT build records, per wave and tile boundary,
  // the stores counted at the issue sites and the allowance used (tests/test_gpu_gemm_tails.py checks slack <= issued).
  // (f32-class mode: its 32 / 64 wider stores would overflow the 6-bit vmcnt field together with the fills -- no
  // allowance there: the first blocks of the next tile also wait for the previous tile's stores)
  // K BLOCKS PER TILE. "Filled before that epilogue, with exactly the counted operations behind" holds for the slots the two
  // blocks behind an epilogue read at every nb >= 2 (the GM_AUDIT build's fill-order audit checks every barrier at nb = 1 .. 9
  // and finds the tightest margin 0: tests/test_gpu_gemm_kblocks.py). At nb = 1 a tile is ONE block and the fetch cursor runs two
  // TILES ahead: what P0 / P1 read behind tile i's epilogue was filled during tile i-1's block, in front of tile i-1's epilogue
  // too -- the stores of two epilogues lie behind those fills and the allowance counts one. Those two waits are stricter than
  // they need be by NS there, never looser; P2 / P3 (filled during tile i's block) are exact again.
  constexpr int NS = F32O ? 0 : (EPI == 1 || EPI == 4 || EPI == 6 || EPI == 8 ? 32 : 16);
  auto k_block = [&](auto a0_, auto a1_) {
    constexpr int A0 = decltype(a0_)::value, A1 = decltype(a1_)::value;
    const uint8_t* sb = smem + par * SLOT;
    const uint8_t* sbn = smem + (par ^ 4) * SLOT;
    auto rd_w1 = [&](int k) { if (k < 4) wB[k] = *reinterpret_cast<const uint4*>(sb + S_W1 * SLOT + w_off(k)); };
    auto rd_x1 = [&](int k) { xB[k] = *reinterpret_cast<const uint4*>(sb + S_X1 * SLOT + x_off(k)); };
    auto rd_x0 = [&](int k) { xA[k] = *reinterpret_cast<const uint4*>(sbn + S_X0 * SLOT + x_off(k)); };
    // W0 of the next block: fragment kk is free once both MFMAs of step kk have been issued (k = 2*kk + 1)
    auto rd_w0 = [&](int k) { if (k & 1) wA[k >> 1] = *reinterpret_cast<const uint4*>(sbn + S_W0 * SLOT + w_off(k >> 1)); };
    auto dm_none = [&](int) {};
    auto dm_x0w0 = [&](int k) {
      if (k == 0) issue_fill(S_X0, par, 0);
      if (k == 2) issue_fill(S_X0, par, 1);
      if (k == 4) issue_fill(S_W0, par, 0);
      if (k == 6) issue_fill(S_W0, par, 1);
    };
    auto dm_w1 = [&](int k) {
      if (k == 1) issue_fill(S_W1, par, 0);
      if (k == 5) issue_fill(S_W1, par, 1);
    };
    auto dm_x1 = [&](int k) {
      if (k == 0) issue_fill(S_X1, par, 0);
      if (k == 4) issue_fill(S_X1, par, 1);
    };
    GM_BAR(10 + A0, aud_slot(GM_CHK_P0_W1, S_W1, par));
    GM_PHASE(xA, wA, 0, 0, rd_w1, dm_none);
    GM_BAR(8 + A0, aud_slot(GM_CHK_P1_X1, S_X1, par));
    GM_PHASE(xA, wB, 0, 1, rd_x1, dm_x0w0);
    GM_BAR(10 + A1, aud_slot(GM_CHK_P2_X0, S_X0, par ^ 4));
    GM_PHASE(xB, wB, 1, 1, rd_x0, dm_w1);
    GM_BAR(10 + A1, aud_slot(GM_CHK_P3_W0, S_W0, par ^ 4));
    GM_PHASE(xB, wA, 1, 0, rd_w0, dm_x1);
    fetch_advance();
    par ^= 4;
  };
  using I0 = std::integral_constant<int, 0>;
  using IS = std::integral_constant<int, NS>;
  for (int i = 0; i < my_tiles; ++i) {
    int j = 0;
    if (i > 0) {                     // the slots read here were filled before the previous tile's epilogue
#ifdef GM_AUDIT
      if (lane == 0 && aud_n < GM_AUDIT_CAP) {
#pragma unroll
        for (int q = 0; q < 4; ++q) audit[4 * (1 + aud_n) + q] = aud_rec[q];
      }
      ++aud_n;
#endif
      GM_AUD(aud_here(i, 0);)
      k_block(IS{}, IS{});
      GM_AUD(aud_here(i, 1);)
      if (nb > 1) k_block(IS{}, I0{});
      j = 2;
    }
    for (; j < nb; ++j) {
      GM_AUD(aud_here(i, j);)
      if (dyn && j == 2) {
        // K block 2: the counter reply asked for before the previous tile's epilogue is an epilogue and 16 fills old;
        // "all but the 10 newest" -- the wait the next barrier performs anyway -- has it in its register
        if (wave == 0) {
          asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
          GM_AUD(aud_wait(10);)
        }
        publish();
      }
      k_block(I0{}, I0{});
    }
    // the fills of the next tile's first blocks are in flight and its first X0 / W0 fragments already in registers
    // while this tile's results leave
    GM_STAMP();
    // Ask for the tile after the next one NOW, in front of this tile's result stores: vector-memory replies come back
    // in issue order, so a slow device-scope atomic holds up the completion count of every fill issued behind it --
    // here the fills in front of it are the ones the next barriers wait for (the next tile's blocks 0 and 1 were
    // fetched before this point), and the epilogue (~3 us) plus two K blocks pass before anything behind it is awaited.
    // (Issued at the top of a tile the reply delayed that tile's first fills: +3 % on the K = 768 shapes.)
    GM_AUD(aud_here(i, nb);)
    if (dyn && my_tiles == 0x7fffffff) pull();
    // (static schedule: recomputed, not get_pair(i) -- the two-entry store is indexed by i & 1, and with fewer than three K
    // blocks per tile the fetch cursor has called fetch_tile(i + 2) -> set_pair(i + 2) BEFORE this epilogue: in the prologue
    // at nb = 1, at the end of this tile's last block at nb = 2. Tile i's results then went to tile i + 2's place and tile i
    // was never written. The dynamic schedule runs from DYN_MIN_NB on: its cursor wraps three blocks before the end.)
    const int pair = dyn ? get_pair(i) : xstart + bid / nx + i * wpx;
    int tm, tn;
    decode_tile(pair, tm, tn);
    epilogue(tm, tn, i);
    // a tail tile's epilogue may have issued fewer than NS stores in this wave: no allowance after it (see NS above)
    const bool tail = NS > 0 && __builtin_amdgcn_readfirstlane((int64_t)tm * TM + TM > M ? 1 : 0);
    if (tail) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef GM_AUDIT
    {
      int issued = gm_wave_max((int)gm_aud_cp);
#pragma unroll
      for (int q = 0; q < 4; ++q) issued += gm_wave_max((int)((gm_aud_st >> (8 * q)) & 255u));
      issued = __builtin_amdgcn_readfirstlane(issued);
      aud_seq += issued;
      aud_rec[0] = tm;
      aud_rec[1] = tn;
      aud_rec[2] = issued;
      aud_rec[3] = tail ? 0 : NS;
      gm_aud_st = gm_aud_cp = 0;
    }
#endif
    GM_STAMP();
    init_acc(i + 1);
    // (the drain counts only from here: the OTHER waves have wave 0's bias image through the last barrier, not through it)
    GM_AUD(if (tail) aud_wait(0);)
    __builtin_amdgcn_sched_barrier(0);
  }
  }
#undef GM_BAR
#undef GM_PHASE
#undef GM_PHASE16
#undef GM_PHASE32
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // drain the run-ahead fills before this workgroup's LDS is freed
#ifdef GM_AUDIT
  if (lane == 0) {
    audit[0] = aud_n;
    audit[1] = aud_viol;
    audit[2] = aud_first;
    audit[3] = aud_margin;
  }
#endif
  // the last pull's reply is never consumed: keep its register reserved until the drain above has delivered it
  asm volatile("" ::"v"(pend));
  if (dyn && wave == 0 && lane == 0) {
    // every workgroup of the launch signs off once (its counter atomics are complete: vmcnt(0) above); the last one
    // out leaves the counter block zeroed for the next launch that is handed the same block
    const unsigned gone = __hip_atomic_fetch_add(sched + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gone == gridDim.x - 1) {
#pragma unroll
      for (int q = 0; q < 9; ++q) __hip_atomic_store(sched + q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The two kernels over the one body. The 16x16x32 instantiations carry a name of their own (and exist for the bf16 results of
// epilogues 0-5 only: gemm_tn_mfma.hip's dispatch); the f32-class mode and the exact-GELU unit stay on 32x32x16.
#define GM_KERNEL_ARGS                                                                                              \
  const uint16_t *__restrict__ X, const uint16_t *__restrict__ W, const float *__restrict__ bias, void *__restrict__ Yv, \
      void *__restrict__ aux_out_v, const void *__restrict__ aux_in_v, float *__restrict__ colpart, int64_t M, int N, int K, \
      int tiles_n, int ntiles, unsigned *__restrict__ sched, int late_mod
template <int EPI, bool F32O>
__global__ __launch_bounds__(512) void gemm_tn_kernel(GM_KERNEL_ARGS) {
  gemm_tn_body<EPI, F32O, 32>(X, W, bias, Yv, aux_out_v, aux_in_v, colpart, M, N, K, tiles_n, ntiles, sched, late_mod);
}
template <int EPI>
__global__ __launch_bounds__(512) void gemm_tn_mfma16(GM_KERNEL_ARGS) {
  gemm_tn_body<EPI, false, 16>(X, W, bias, Yv, aux_out_v, aux_in_v, colpart, M, N, K, tiles_n, ntiles, sched, late_mod);
}
#undef GM_KERNEL_ARGS
template <int EPI, bool F32O, int MS>
constexpr auto tn_kernel() {
  if constexpr (MS == 16) return &gemm_tn_mfma16<EPI>;
  else return &gemm_tn_kernel<EPI, F32O>;
}

int num_cus() { return lvl_persistent_cus(); }      // one persistent workgroup per compute unit

template <int EPI, bool F32O = false, int MS = 32>
int launch_tn(const void* x, const void* w, const float* bias, void* y, void* aux_out, const void* aux_in,
              float* colpart, int64_t M, int N, int K, unsigned* sched, hipStream_t st) {
  constexpr int shmem = SMEM_B;
  constexpr auto kernel = tn_kernel<EPI, F32O, MS>();
  const int rc = lvl_allow_lds<kernel>();
  if (rc != LVL_OK) return rc;
  const int tiles_n = N / TN;
  const int64_t tiles_m = (M + TM - 1) / TM;
  const int64_t ntiles = tiles_m * tiles_n;
  if (ntiles > 0x7fffffff) return lvl_fail(LVL_EINVAL, "linear_tn: too many tiles");
  int grid = (int)(ntiles < num_cus() ? ntiles : num_cus());
  if (grid >= 8) grid -= grid % 8;          // whole XCD rounds (the kernel maps workgroup b to XCD b % 8)
  if (K / BK < DYN_MIN_NB) sched = nullptr; // too few K blocks per tile for the counter hand-off: static schedule
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(512), shmem, st, (const uint16_t*)x,
                     (const uint16_t*)w, bias, y, aux_out, aux_in, colpart, M,
                     N, K, tiles_n, (int)ntiles, sched, sched ? lvl_debug_late_mod() : 0);
  LVL_CHECK_LAUNCH("linear_tn");
  return LVL_OK;
}

// ---- The epilogues as data: one row per LVL_EPI_* value --------------------------------------------------------------------
// What lvl_linear_tn requires of a call, what its debug twins (GM_AUDIT / GM_TRACE) launch and which kernels a unit
// instantiates all follow from a row; an epilogue is added here and as one case of its unit's tn_launch.
enum { TN_UNIT_MFMA, TN_UNIT_GELU };      // gemm_tn_mfma.hip | gemm_tn_gelu.hip
struct TnEpilogue {
  bool bias, aux_out, aux_in;             // takes a bias | writes aux_out | reads aux_in (an operand it does not take is passed as null)
  bool colpart;                           // leaves [2 * tiles_m][N] column partials to reduce: needs colsum and ws
  bool f32;                               // exists in the f32-class mode (the others keep act'(u) in bf16: bf16 only)
  int unit;                               // the translation unit that instantiates its kernels
  const char* name;                       // in refusal texts
};
constexpr TnEpilogue kTnEpilogues[] = {
    /* 0 LVL_EPI_BIAS                 */ {true, false, false, false, true, TN_UNIT_MFMA, "plain"},
    /* 1 LVL_EPI_BIAS_QUICKGELU       */ {true, true, false, false, true, TN_UNIT_MFMA, "QuickGELU"},
    /* 2 LVL_EPI_QUICKGELU_BWD        */ {false, false, true, true, true, TN_UNIT_MFMA, "QuickGELU-backward"},
    /* 3 LVL_EPI_BIAS_RESIDUAL        */ {true, false, true, false, true, TN_UNIT_MFMA, "residual"},
    /* 4 LVL_EPI_BIAS_QUICKGELU_DERIV */ {true, true, false, false, false, TN_UNIT_MFMA, "QuickGELU + derivative"},
    /* 5 LVL_EPI_MUL_AUX_COLSUM       */ {false, false, true, true, false, TN_UNIT_MFMA, "multiply-by-aux"},
    /* 6 LVL_EPI_BIAS_GELU            */ {true, true, false, false, true, TN_UNIT_GELU, "GELU"},
    /* 7 LVL_EPI_GELU_BWD             */ {false, false, true, true, true, TN_UNIT_GELU, "GELU-backward"},
    /* 8 LVL_EPI_BIAS_GELU_DERIV      */ {true, true, false, false, false, TN_UNIT_GELU, "GELU + derivative"},
};
static_assert(sizeof(kTnEpilogues) / sizeof(kTnEpilogues[0]) == LVL_EPI_BIAS_GELU_DERIV + 1, "one row per LVL_EPI_* value");
constexpr bool tn_epilogue_known(int e) { return e >= LVL_EPI_BIAS && e <= LVL_EPI_BIAS_GELU_DERIV; }

struct TnCall {      // the arguments of launch_tn
  const void *x, *w;
  const float* bias;
  void *y, *aux_out;
  const void* aux_in;
  float* colpart;
  int64_t M;
  int N, K;
  unsigned* sched;
  hipStream_t st;
};

// (EPI, f32, ms) -> the launch_tn instantiation, for the cases of a unit's tn_launch. MS16: the unit carries the 16x16x32
// kernels. A mode the table does not give the epilogue is not instantiated: -1, as for an epilogue of the other unit.
template <int EPI, bool MS16>
int launch_tn_mode(bool f32, int ms, const TnCall& c) {
  constexpr TnEpilogue e = kTnEpilogues[EPI];
  const float* bias = e.bias ? c.bias : nullptr;
  void* aux_out = e.aux_out ? c.aux_out : nullptr;
  const void* aux_in = e.aux_in ? c.aux_in : nullptr;
  if (f32) {
    if constexpr (e.f32) return launch_tn<EPI, true>(c.x, c.w, bias, c.y, aux_out, aux_in, c.colpart, c.M, c.N, c.K, c.sched, c.st);
    else return -1;
  }
  if constexpr (MS16)
    if (ms == 16) return launch_tn<EPI, false, 16>(c.x, c.w, bias, c.y, aux_out, aux_in, c.colpart, c.M, c.N, c.K, c.sched, c.st);
  return launch_tn<EPI>(c.x, c.w, bias, c.y, aux_out, aux_in, c.colpart, c.M, c.N, c.K, c.sched, c.st);
}

// The argument checks lvl_linear_tn and lvl_linear_tn_ragged share, in one order: null pointers, dtype, (bias_only, the ragged
// entry: bf16 and LVL_EPI_BIAS), empty problem, tiling (N in n_mod's, K in 64s), 4 GiB, alignment.
inline int tn_check_args(const char* who, const TnCall& c, int n_mod, int epilogue, int dtype, bool bias_only) {
  LVL_REQUIRE(c.x && c.w && c.y, "%s: null pointer", who);
  LVL_REQUIRE(dtype == LVL_BF16 || dtype == LVL_F32, "%s: unknown dtype %d", who, dtype);
  if (bias_only) {
    if (dtype != LVL_BF16)
      return lvl_fail(LVL_ENOSYS, "%s: bf16 only (float32 rows at these widths: lvl_linear_skinny_f32c)", who);
    LVL_REQUIRE(tn_epilogue_known(epilogue), "%s: unknown epilogue %d", who, epilogue);
    if (epilogue != LVL_EPI_BIAS)
      return lvl_fail(LVL_ENOSYS, "%s: epilogue %d is not available on ragged widths (LVL_EPI_BIAS only)", who, epilogue);
  }
  LVL_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0, "%s: empty problem", who);
  if (c.N % n_mod != 0 || c.K % BK != 0)
    return lvl_fail(LVL_ENOSYS, "%s: no tiling for N=%d K=%d (N %% %d == 0 and K %% 64 == 0 needed)", who, c.N, c.K, n_mod);
  if ((uint64_t)c.M * c.K * 2 >= (1ull << 32) || (uint64_t)c.N * c.K * 2 >= (1ull << 32))
    return lvl_fail(LVL_ENOSYS, "%s: operand larger than 4 GiB (32-bit DMA offsets)", who);
  LVL_REQUIRE(lvl_aligned16(c.x) && lvl_aligned16(c.w) && lvl_aligned16(c.y) && lvl_aligned16(c.bias) &&
                  lvl_aligned16(c.aux_out) && lvl_aligned16(c.aux_in),
              "%s: pointers must be 16-byte aligned", who);
  return LVL_OK;
}

}  // namespace
