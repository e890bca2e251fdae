// minimal host-side status plumbing for the GM_TRACE / GM_AUDIT debug builds of gemm_tn_mfma.hip
// (tools/probe_gemm_trace.py, tests/test_gpu_gemm_tails.py)
#include <stdarg.h>
#include <stdio.h>
#include <hip/hip_runtime.h>
thread_local char lvl_err_buf[512] = "";
int lvl_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(lvl_err_buf, sizeof(lvl_err_buf), fmt, ap);
  va_end(ap);
  fprintf(stderr, "lvl_fail: %s\n", lvl_err_buf);
  return code;
}

// the compute-unit limit and the late-workgroup modulus, settable under the names the product library uses
static int g_cus = 0, g_late_mod = 0;
extern "C" int lvl_set_compute_units(int n) {
  if (n < 0 || (n != 0 && (n < 8 || n % 8))) return lvl_fail(1, "set_compute_units: %d is not 0 or a multiple of 8", n);
  g_cus = n;
  return 0;
}
extern "C" int lvl_debug_late_workgroups(int mod) {
  if (mod < 0 || mod == 1) return lvl_fail(1, "debug_late_workgroups: mod must be 0 or >= 2");
  g_late_mod = mod;
  return 0;
}
int lvl_persistent_cus() {
  int dev = 0, v = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      v <= 0)
    v = 256;
  return (g_cus > 0 && g_cus < v) ? g_cus : v;
}
int lvl_debug_late_mod() { return g_late_mod; }

// symbols the GEMM file references outside the debug entry points (the column partials of epilogues 2 / 5 stay unreduced)
int lvl_colsum_mid_rows() { return 64; }
int lvl_launch_column_reduce(const float*, int, int, int, float*, float*, float*, float*, hipStream_t) { return 0; }
// lvl_linear_tn_ragged's edge kernel (gemm_tn_edge.hip) is not part of the debug builds: the ragged entry point refuses there
int lvl_launch_tn_edge(const void*, const void*, const float*, void*, int64_t, int, int, int, hipStream_t) {
  return lvl_fail(-38, "linear_tn_ragged: the edge kernel is not linked into this debug build");
}
// lvl_linear_tn's exact-GELU epilogues live in gemm_tn_gelu.hip; a debug build of gemm_tn_mfma.hip alone refuses them, a debug
// build of gemm_tn_gelu.hip brings its own definition (hence weak)
__attribute__((weak)) int lvl_launch_tn_gelu(const void*, const void*, const float*, void*, void*, const void*, float*, int64_t,
                                             int, int, uint32_t*, int, int, hipStream_t) {
  return lvl_fail(-38, "linear_tn: the exact-GELU kernels are not linked into this debug build");
}
