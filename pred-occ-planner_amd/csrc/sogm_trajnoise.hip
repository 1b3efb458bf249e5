// Message noise (include/sogm_abi.h "message noise"; the rules are sogm_trajnoise.hpp's, shared with the host).  One launch:
//   k_traj_noise   a workgroup of 256 lanes owns TRAJNOISE_ROWS = 4 rows of the table, one wave per record.  Lanes 0 .. 6 form
//                  the message's seven terms (trajnoise_term: four mixes for the key, three for the draw, one multiply), the
//                  wave shares them by lane reads and every lane forms the same shift; all 64 lanes then stream the
//                  2064-byte record in 16-byte pieces as copy_record does — 129 pieces, two full trips and one piece —
//                  passing both words of a piece through trajnoise_word.  Lanes 0 .. 3 write the row's out_shift.
// A lane writes only the piece it read, so out == table (in place) is the same work; no waiting on other waves.
#include "sogm_device.hpp"
#include "sogm_trajnoise.hpp"

#include <cstdio>

namespace sogm {
namespace {

constexpr int TRAJNOISE_WG   = 256;
constexpr int TRAJNOISE_ROWS = TRAJNOISE_WG / 64;
static_assert(sizeof(SogmTrajRecord) % 16 == 0, "records are streamed in 16-byte pieces");
static_assert(sizeof(SogmTrajNoise) == 56, "include/sogm_abi.h states the size");

struct TrajNoiseArgs {
  SogmTrajNoise         prm;
  const SogmTrajRecord *table;
  SogmTrajRecord       *out;
  double               *out_shift;
  int                   tick, n_total;
};

__global__ __launch_bounds__(TRAJNOISE_WG) void k_traj_noise(TrajNoiseArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * TRAJNOISE_ROWS + wave;
  if (row >= g.n_total) return;  // (uniform in the wave; the kernel has no barrier)
  const int j = (int)row;

  const int noised   = trajnoise_noised(g.table[j].n_pieces);
  double    shift[4] = {0.0, 0.0, 0.0, 0.0};
  if (noised > 0) {  // (uniform in the wave)
    const double term = lane < TRAJNOISE_TERMS ? trajnoise_term(g.prm, g.tick, j, lane) : 0.0;
    for (int c = 0; c < 3; ++c) {
      const double b = __shfl(term, c), e = __shfl(term, 4 + c);
      shift[c] = b + e;
    }
    shift[3] = __shfl(term, 3);
  }
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(g.table + j);
  ulonglong2       *dst = reinterpret_cast<ulonglong2 *>(g.out + j);
  for (int w = lane; w < TRAJ_WORDS / 2; w += 64) {
    ulonglong2 p = src[w];
    p.x = trajnoise_word(2 * w, p.x, noised, shift);
    p.y = trajnoise_word(2 * w + 1, p.y, noised, shift);
    dst[w] = p;
  }
  if (g.out_shift && lane < 4)
    g.out_shift[(size_t)j * 4 + lane] = lane == 0 ? shift[0] : lane == 1 ? shift[1] : lane == 2 ? shift[2] : shift[3];
}

int trajnoise_refused(const char *entry, const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_traj_noise_default_params(SogmTrajNoise *out) {
  using namespace sogm;
  if (!out) return trajnoise_refused("sogm_traj_noise_default_params", "null pointer");
  *out = SogmTrajNoise{};  // no noise
  return SOGM_OK;
}

extern "C" int sogm_traj_noise(const SogmTrajNoise *prm, int tick, const SogmTrajRecord *table, int n_total, SogmTrajRecord *out,
                               double *out_shift, void *stream) {
  using namespace sogm;
  if (const char *why = trajnoise_refuse(prm, tick, table, n_total, out)) return trajnoise_refused("sogm_traj_noise", why);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    set_error_text("sogm_traj_noise: no HIP device");
    return SOGM_ERR_NO_DEVICE;
  }
  TrajNoiseArgs g{};
  g.prm       = *prm;
  g.table     = table;
  g.out       = out;
  g.out_shift = out_shift;
  g.tick      = tick;
  g.n_total   = n_total;
  hipLaunchKernelGGL(k_traj_noise, dim3((unsigned)((n_total - 1) / TRAJNOISE_ROWS + 1)), dim3(TRAJNOISE_WG), 0,
                     (hipStream_t)stream, g);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
