// sogm_lp.hip — the wave LP of sogm_lp.hpp as an entry point of its own (sogm_linprog_batched), for tests and tools that
// hold it to sdlp::linprog<3|4> (traj_utils/include/traj_utils/sdlp.hpp).
#include <hip/hip_runtime.h>

#include "sogm_device.hpp"
#include "sogm_lp.hpp"

namespace sogm {

// sdlp::linprog<d> for a batch of independent LPs: one wave per problem (sogm_linprog_batched)
template <int D>
__global__ __launch_bounds__(64) void k_linprog(const double *__restrict__ c, const double *__restrict__ A,
                                                const double *__restrict__ b,
                                                const int32_t *__restrict__ row_range,
                                                double *__restrict__ out_x, double *__restrict__ out_min) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const LpScratch sc = LpLds::carve(s_dyn);
  const int       p = blockIdx.x, lane = threadIdx.x;
  const int r0 = row_range[2 * p], rows = row_range[2 * p + 1] - r0;
  if (rows >= LP_MAX_ROWS || rows < 0) {  // capacity: NaN, never a silent answer
    if (lane == 0) {
      out_min[p] = __builtin_nan("");
      for (int j = 0; j < D; ++j) out_x[p * D + j] = __builtin_nan("");
    }
    return;
  }
  for (int i = lane; i < rows; i += 64) {
    for (int j = 0; j < D; ++j) sc.A()[i * D + j] = A[(size_t)(r0 + i) * D + j];
    sc.b()[i] = b[r0 + i];
  }
  wave_lds_sync();
  double cv[D], x[D];
  for (int j = 0; j < D; ++j) cv[j] = c[p * D + j];
  const double v = linprog_wave<D>(cv, rows, sc.A(), sc.b(), x, sc.work, sc.perm);
  if (lane == 0) {
    out_min[p] = v;
    for (int j = 0; j < D; ++j) out_x[p * D + j] = x[j];
  }
}

}  // namespace sogm

extern "C" int sogm_linprog_batched(int d, const double *c, const double *A, const double *b,
                                    const int32_t *row_range, int n, double *out_x, double *out_min,
                                    void *stream) {
  if ((d != 3 && d != 4) || n < 0 || (n > 0 && (!c || !row_range || !out_x || !out_min)))
    return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  const size_t lds = sogm::LpLds::bytes();
  hipStream_t  st  = (hipStream_t)stream;
  if (d == 3)
    hipLaunchKernelGGL(sogm::k_linprog<3>, dim3(n), dim3(64), lds, st, c, A, b, row_range, out_x, out_min);
  else
    hipLaunchKernelGGL(sogm::k_linprog<4>, dim3(n), dim3(64), lds, st, c, A, b, row_range, out_x, out_min);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
