// View mask (include/sogm_abi.h "view mask"; the rules: sogm_viewmask.hpp): the class of every cell of every agent's grid
// against that agent's depth image, as a bit mask in the layout of k_map_audit's region[] and as per-class counts.
// Two launches, stream-ordered:
//   k_view_counts_zero   one lane per counter: out_counts zeroed (only with out_counts)
//   k_view_mask          workgroups of four waves over (agent, words of the agent's mask); one wave per 64-bit word, one
//                        lane per cell.  cam_rot and cam_offset of the agent are read once per workgroup (through LDS); the
//                        class is view_class (fp64, one 2-byte gather from the depth image: neighbouring cells of an x-row
//                        project to neighbouring pixels, and an agent's image fits L2); one __ballot per word for the mask
//                        and one 8-byte store by lane 0; one ballot per class, whose popcounts every wave sums in uniform
//                        registers over its words, then per workgroup in LDS, then ONE integer atomicAdd per class and
//                        workgroup.
// Integer adds only: the counts do not depend on the order the workgroups finish in.
#include "sogm_device.hpp"
#include "sogm_viewmask.hpp"

#include <cmath>
#include <cstdio>

namespace sogm {
namespace {

constexpr int VIEW_WG        = 256;
constexpr int VIEW_WAVES     = VIEW_WG / 64;
constexpr int VIEW_COUNTS    = 8;     // out_counts per agent: five classes, the mask's bits, two zeros
constexpr int VIEW_MAX_BLOCKS = 1024;  // per agent; a wave strides over the words beyond

struct ViewArgs {
  AuditFrustum f;  // R is filled per agent by the kernel
  ViewCamera   cam;
  int          classes;
  int          L, W, H;
  int          row_words, layer_words;
  long long    words;  // per agent: H * layer_words
  float        res, rx, ry, rz;
};

__global__ __launch_bounds__(64) void k_view_counts_zero(int32_t *__restrict__ counts, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) counts[i] = 0;
}

__global__ __launch_bounds__(VIEW_WG) void k_view_mask(ViewArgs p, const uint16_t *__restrict__ depth,
                                                       const double *__restrict__ cam_rot,
                                                       const double *__restrict__ cam_offset,
                                                       unsigned long long *__restrict__ out_mask, int32_t *__restrict__ out_counts) {
  __shared__ double s_cam[12];
  __shared__ int    s_cnt[VIEW_COUNTS];
  const int a = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 9) s_cam[tid] = cam_rot[(size_t)a * 9 + tid];
  if (tid >= 9 && tid < 12 && cam_offset) s_cam[tid] = cam_offset[(size_t)a * 3 + (tid - 9)];
  if (tid < VIEW_COUNTS) s_cnt[tid] = 0;
  __syncthreads();
  AuditFrustum f = p.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) f.R[k] = s_cam[k];
  const bool   has_off = cam_offset != nullptr;
  const double o0 = has_off ? s_cam[9] : 0.0, o1 = has_off ? s_cam[10] : 0.0, o2 = has_off ? s_cam[11] : 0.0;
  const uint16_t     *img  = depth + (size_t)a * (size_t)p.cam.rows * (size_t)p.cam.cols;
  unsigned long long *mask = out_mask + (size_t)a * (size_t)p.words;

  int n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, nm = 0;  // uniform over the wave: sums of popcounts of ballots
  for (long long i = (long long)blockIdx.x * VIEW_WAVES + wave; i < p.words; i += (long long)gridDim.x * VIEW_WAVES) {
    const int z = (int)(i / p.layer_words), rem = (int)(i - (long long)z * p.layer_words);
    const int y = rem / p.row_words, w = rem - y * p.row_words;
    const int x = (w << 6) + lane;
    int       cls = -1;  // a spare bit of the row's last word: no class, no bit
    if (x < p.L)
      cls = view_class(f, p.cam, img, view_centre(x, p.res, p.rx, has_off, o0), view_centre(y, p.res, p.ry, has_off, o1),
                       view_centre(z, p.res, p.rz, has_off, o2));
    const unsigned long long m = __ballot(cls >= 0 && ((p.classes >> cls) & 1));
    n0 += __popcll(__ballot(cls == VIEW_OUTSIDE));
    n1 += __popcll(__ballot(cls == VIEW_OFFIMAGE));
    n2 += __popcll(__ballot(cls == VIEW_FREE));
    n3 += __popcll(__ballot(cls == VIEW_SURFACE));
    n4 += __popcll(__ballot(cls == VIEW_HIDDEN));
    nm += __popcll(m);
    if (lane == 0) mask[i] = m;
  }
  if (!out_counts) return;  // (uniform)
  if (lane == 0) {
    if (n0) atomicAdd(&s_cnt[0], n0);
    if (n1) atomicAdd(&s_cnt[1], n1);
    if (n2) atomicAdd(&s_cnt[2], n2);
    if (n3) atomicAdd(&s_cnt[3], n3);
    if (n4) atomicAdd(&s_cnt[4], n4);
    if (nm) atomicAdd(&s_cnt[5], nm);
  }
  __syncthreads();
  if (tid < 6 && s_cnt[tid]) atomicAdd(out_counts + (size_t)a * VIEW_COUNTS + tid, s_cnt[tid]);
}

int view_refuse(const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "sogm_view_mask: %s", what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_view_default_params(const SogmDepthCamera *cam, SogmViewParams *out) {
  if (!cam || !out) {
    sogm::set_error_text("sogm_view_default_params: null pointer");
    return SOGM_ERR_INVALID_ARG;
  }
  SogmViewParams p{};
  p.fx = cam->fx, p.fy = cam->fy, p.cx = cam->cx, p.cy = cam->cy;
  p.depth_scale = cam->depth_scale, p.max_depth = cam->max_depth;
  p.near_z = 0.0, p.far_z = cam->max_depth;
  p.tan_h = 0.5 * cam->cols / cam->fx, p.tan_v = 0.5 * cam->rows / cam->fy;
  p.band = 0.0;
  p.rows = cam->rows, p.cols = cam->cols;
  p.classes = SOGM_VIEWBIT_FREE | SOGM_VIEWBIT_SURFACE;
  *out = p;
  return SOGM_OK;
}

extern "C" int sogm_view_mask(sogm_ctx *map, const SogmViewParams *prm, const uint16_t *depth, const double *cam_rot,
                              const double *cam_offset, uint64_t *out_mask, int32_t *out_counts, void *stream) {
  using namespace sogm;
  if (!map || !prm || !depth || !cam_rot || !out_mask) return view_refuse("null pointer");
  if (prm->rows < 1 || prm->cols < 1) return view_refuse("rows and cols must be >= 1");
  if ((long long)prm->rows * prm->cols > 2147483647LL) return view_refuse("an image of more than 2^31 - 1 pixels");
  const double num[11] = {prm->fx, prm->fy, prm->cx, prm->cy, prm->depth_scale, prm->max_depth, prm->near_z, prm->far_z,
                          prm->tan_h, prm->tan_v, prm->band};
  for (double v : num)
    if (!std::isfinite(v)) return view_refuse("intrinsics, depth_scale, max_depth, band and the frustum must be finite");
  if (!(prm->fx > 0) || !(prm->fy > 0) || !(prm->depth_scale > 0) || !(prm->max_depth > 0) || !(prm->tan_h > 0) || !(prm->tan_v > 0))
    return view_refuse("fx, fy, depth_scale, max_depth, tan_h and tan_v must be > 0");
  if (prm->near_z < 0 || !(prm->far_z > prm->near_z)) return view_refuse("near_z >= 0 and far_z > near_z are required");
  if (prm->far_z > prm->max_depth) return view_refuse("far_z above max_depth: a zero pixel says nothing beyond max_depth");
  if (prm->band < 0) return view_refuse("band must be >= 0");
  if (prm->classes == 0 || (prm->classes & ~SOGM_VIEWBIT_ALL)) return view_refuse("classes is zero or has a bit above class 4");
  {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
      set_error_text("sogm_view_mask: no HIP device");
      return SOGM_ERR_NO_DEVICE;
    }
  }
  const GridGeom &g = map->geom;
  ViewArgs        p{};
  p.f.near_z = prm->near_z, p.f.far_z = prm->far_z, p.f.tan_h = prm->tan_h, p.f.tan_v = prm->tan_v;
  p.cam.fx = prm->fx, p.cam.fy = prm->fy, p.cam.cx = prm->cx, p.cam.cy = prm->cy;
  p.cam.depth_scale = prm->depth_scale, p.cam.band = prm->band, p.cam.rows = prm->rows, p.cam.cols = prm->cols;
  p.classes = prm->classes;
  p.L = g.L, p.W = g.W, p.H = g.H;
  p.row_words = audit_row_words(g.L), p.layer_words = g.W * p.row_words;
  p.words = view_mask_words(g.L, g.W, g.H);
  p.res = g.res, p.rx = g.rx, p.ry = g.ry, p.rz = g.rz;

  SOGM_HIP_CHECK(hipSetDevice(map->device));
  hipStream_t st = (hipStream_t)stream;
  const int   n  = map->n_agents;
  if (out_counts)
    hipLaunchKernelGGL(k_view_counts_zero, dim3((n * VIEW_COUNTS + 63) / 64), dim3(64), 0, st, out_counts, n * VIEW_COUNTS);
  long long blocks = (p.words + VIEW_WAVES - 1) / VIEW_WAVES;
  if (blocks > VIEW_MAX_BLOCKS) blocks = VIEW_MAX_BLOCKS;
  hipLaunchKernelGGL(k_view_mask, dim3((unsigned)blocks, (unsigned)n), dim3(VIEW_WG), 0, st, p, depth, cam_rot, cam_offset,
                     reinterpret_cast<unsigned long long *>(out_mask), out_counts);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
