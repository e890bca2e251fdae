// The exact-GELU epilogues of the persistent TN GEMM (gemm_tn_kernel.h; described at the top of gemm_tn_mfma.hip):
//   6  u = acc + bias -> aux_out ; y = gelu(u)              bf16 and f32-class
//   7  y = acc * gelu'(aux_in) ; column sums -> partial slab   bf16 and f32-class
//   8  u = acc + bias ; y = gelu(u) ; aux_out = gelu'(u)       bf16
// instantiated in a translation unit of their own: gemm_tn_mfma.hip keeps exactly the instantiations it had (their device
// code does not move when an epilogue is added here), and lvl_linear_tn dispatches epilogues 6-8 to lvl_launch_tn_gelu.
// Compiled with the flags of gemm_tn_mfma.hip (lavila_amd/build.py).
#include "internal.h"
#include "gelu_erf.h"
#include "gemm_tn_kernel.h"

// This unit's kernels: epilogues 6-8 of the table (kTnEpilogues) in the modes it gives them, on 32x32x16. The one switch over
// epilogue codes of this file. -1: not instantiated here.
static int tn_launch(int epilogue, bool f32, const TnCall& c) {
  switch (epilogue) {
    case LVL_EPI_BIAS_GELU: return launch_tn_mode<6, false>(f32, 32, c);
    case LVL_EPI_GELU_BWD: return launch_tn_mode<7, false>(f32, 32, c);
    case LVL_EPI_BIAS_GELU_DERIV: return launch_tn_mode<8, false>(f32, 32, c);
  }
  return -1;
}

// one launch of gemm_tn_kernel<epilogue, f32> (no argument checks: lvl_linear_tn has made them). colpart: the partial slab of
// epilogue 7 (the caller reduces it). An (epilogue, mode) pair that is not instantiated here: LVL_ENOSYS.
int lvl_launch_tn_gelu(const void* x, const void* w, const float* bias, void* y, void* aux_out, const void* aux_in,
                       float* colpart, int64_t M, int N, int K, uint32_t* sched, int epilogue, int f32, hipStream_t st) {
  const int rc = tn_launch(epilogue, f32 != 0, {x, w, bias, y, aux_out, aux_in, colpart, M, N, K, sched, st});
  if (rc != -1) return rc;
  return lvl_fail(LVL_ENOSYS, "linear_tn: no exact-GELU kernel for epilogue %d in %s mode", epilogue, f32 ? "f32-class" : "bf16");
}

#ifdef GM_TRACE
// gemm_tn_mfma.hip's lvl_linear_tn_trace_epi for epilogues 6 and 8 (a debug build of THIS file with the host stub)
extern "C" int lvl_linear_tn_trace_epi(const void* x, const void* w, const float* bias, void* y, void* aux_out,
                                       const void* aux_in, void* trace, int64_t M, int N, int K, int epilogue, void* stream) {
  if (epilogue == LVL_EPI_GELU_BWD) return -1;
  return tn_launch(epilogue, false, {x, w, bias, y, aux_out, aux_in, (float*)trace, M, N, K, nullptr, (hipStream_t)stream});
}
#endif

#ifdef GM_AUDIT
// gemm_tn_mfma.hip's lvl_linear_tn_audit for epilogues 6-8, same arguments and record layout (a debug build of THIS file with
// the host stub; epilogue 7: the records behind its [2 * tiles_m][N] column partials, which are left unreduced)
extern "C" int lvl_linear_tn_audit_cap() { return GM_AUDIT_CAP; }
extern "C" int lvl_linear_tn_audit(const void* x, const void* w, const float* bias, void* y, void* aux_out,
                                   const void* aux_in, void* audit, uint32_t* sched, int64_t M, int N, int K, int epilogue,
                                   int dtype, void* stream) {
  return tn_launch(epilogue, dtype == LVL_F32, {x, w, bias, y, aux_out, aux_in, (float*)audit, M, N, K, sched, (hipStream_t)stream});
}
#endif
