// lt_post.hip -- what the reference does with the rendered images right after the hot path:
//   * do_reverse_projection_new  (auxiliary/laserscan.py:475-501): range image + pixel coordinates -> xyz
//   * MultiSemLaserScan.write    (auxiliary/laserscan.py:1121-1178): drop invalid cells, pack the scan as
//     SemanticKITTI `.bin` ([N,4] f32: x, y, z, remission) and `.label` ([N] u32) -- the per-point
//     struct.pack loop of the reference becomes one stable stream compaction on the GPU
//   * compare / iouEval          (auxiliary/laserscan.py:1181-1301, np_ioueval.py:31-70): masked confusion
//     matrix (atomic histogram) and squared range / remission differences
#include "lt_internal.h"
#include "lt_devmem.h"
#include <math.h>
#include <mutex>
#include <type_traits>

// ---- reverse projection (float64, as numpy computes it from int32 / float64 pixel coordinates) ------------
// One kernel for every target sensor.  P: int32 coordinates, or float64 (`preserve_float`: the winner's own).
//   yaw    the full circle: theta = (px / W * 2 - 1) * pi.  SECTOR (what LT_PROJ_SECTOR projected): the column's yaw is that
//          of its ray, the CENTRE of cell px -- yaw = yc + ((px + 0.5) / W - 0.5) * span -- or, with float64 coordinates, the
//          winner's own: yaw = yc + (xf / W - 0.5) * span
//   pitch  the linear rows: 90 - phi.  BEAMS (a beam table): the elevation e = Brad[row], or the winner's pitch itself with
//          float64 coordinates; pitch = pi / 2 - e.  A row outside the table (no caller makes one) reads its nearest end,
//          never memory beside the table
// The three products are multiplied left to right.
template <typename P, int BEAMS, int SECTOR>
__global__ __launch_bounds__(256) void k_reverse(const float* __restrict__ range, const P* __restrict__ px,
                                                 const P* __restrict__ py, int n, double W, double H, double fov,
                                                 double abs_fov_down, const double* __restrict__ Brad, double yc, double span,
                                                 double* __restrict__ out) {
  constexpr bool is_float = std::is_same<P, double>::value;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double depth = (double)range[i];
  double yaw;
  if (SECTOR) {
    const double x = is_float ? (double)px[i] / W : ((double)px[i] + 0.5) / W;
    yaw = yc + (x - 0.5) * span;
  } else {
    const double x = (double)px[i] / W;
    yaw = (x * 2 - 1.0) * M_PI;                                             // theta
  }
  double pitch;
  if (BEAMS) {
    double e;
    if (is_float) {
      e = (double)py[i];
    } else {
      int r = (int)py[i];
      const int h = (int)H;
      r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
      e = Brad[r];
    }
    pitch = M_PI / 2 - e;
  } else {
    const double y = (double)py[i] / H;
    pitch = M_PI / 2 - (1.0 * fov - y * fov - abs_fov_down);                // 90 - phi
  }
  const double sp = sin(pitch);
  out[3 * (size_t)i] = depth * sp * cos(-yaw);
  out[3 * (size_t)i + 1] = depth * sp * sin(-yaw);
  out[3 * (size_t)i + 2] = depth * cos(pitch);
}

// `rows`: a beam table (Brad; the field of view is not read then).  `sec` = (yaw of the middle, width) in radians, or
// NULL: the full circle.
static int reverse_launch(const float* range_img, const void* proj_x, const void* proj_y, int coords_are_f64,
                          const double* Brad, bool rows, double fov_up, double fov_down, int H, int W, const double* sec,
                          double* back_points, hipStream_t st) {
  const double fu = fov_up / 180.0 * M_PI, fd = fov_down / 180.0 * M_PI;
  const double fov = fabs(fd) + fabs(fu);
  const int n = H * W;
  const bool sector = sec != nullptr;
  const double yc = sec ? sec[0] : 0.0, span = sec ? sec[1] : 0.0;
#define LT_REVERSE(P, B, S)                                                                                                  \
  hipLaunchKernelGGL((k_reverse<P, B, S>), dim3((n + 255) / 256), dim3(256), 0, st, range_img, (const P*)proj_x,             \
                     (const P*)proj_y, n, (double)W, (double)H, fov, fabs(fd), Brad, yc, span, back_points)
#define LT_REVERSE_F64(B, S, AZ) LT_REVERSE(double, B, S)  // (offsets: k_reverse_az, below)
#define LT_REVERSE_I32(B, S, AZ) LT_REVERSE(int, B, S)
  if (coords_are_f64) LT_FOR_MODEL(rows, sector, false, LT_REVERSE_F64);
  else LT_FOR_MODEL(rows, sector, false, LT_REVERSE_I32);
#undef LT_REVERSE
#undef LT_REVERSE_F64
#undef LT_REVERSE_I32
  LT_HIP(hipGetLastError());
  return LT_OK;
}

extern "C" int lt_reverse_projection_dev(const float* range_img, const void* proj_x, const void* proj_y,
                                         int coords_are_f64, double fov_up, double fov_down, int H, int W,
                                         double* back_points, void* stream) {
  if (H <= 0 || W <= 0 || !range_img || !proj_x || !proj_y || !back_points) {
    lt_set_error("lt_reverse_projection_dev: invalid argument");
    return LT_ERR_INVALID_ARG;
  }
  return reverse_launch(range_img, proj_x, proj_y, coords_are_f64, nullptr, false, fov_up, fov_down, H, W, nullptr, back_points,
                        (hipStream_t)stream);
}

extern "C" int lt_reverse_projection_beams_dev(const float* range_img, const void* proj_x, const void* proj_y_or_pitch,
                                               int preserve_float, const double* Brad, int H, int W, double* back_points,
                                               void* stream) {
  if (H <= 0 || W <= 0 || !range_img || !proj_x || !proj_y_or_pitch || !back_points || (!preserve_float && !Brad)) {
    lt_set_error("lt_reverse_projection_beams_dev: invalid argument");
    return LT_ERR_INVALID_ARG;
  }
  return reverse_launch(range_img, proj_x, proj_y_or_pitch, preserve_float, Brad, true, 0.0, 0.0, H, W, nullptr, back_points,
                        (hipStream_t)stream);
}

extern "C" int lt_reverse_projection_sector_dev(const float* range_img, const void* proj_x, const void* proj_y_or_pitch,
                                                int preserve_float, int beam_rows, const double* Brad, double fov_up,
                                                double fov_down, int H, int W, double yaw_center, double span,
                                                double* back_points, void* stream) {
  if (H <= 0 || W <= 0 || !range_img || !proj_x || !proj_y_or_pitch || !back_points ||
      (beam_rows && !preserve_float && !Brad) || !(fabs(yaw_center) <= M_PI) || !(span > 0.0 && span < 2 * M_PI)) {
    lt_set_error("lt_reverse_projection_sector_dev: invalid argument (H=%d W=%d yaw_center=%g span=%g)", H, W, yaw_center, span);
    return LT_ERR_INVALID_ARG;
  }
  const double sec[2] = {yaw_center, span};
  return reverse_launch(range_img, proj_x, proj_y_or_pitch, preserve_float, Brad, beam_rows != 0, fov_up, fov_down, H, W, sec,
                        back_points, (hipStream_t)stream);
}

// The same for a beam table whose beams carry AZIMUTH OFFSETS (what LT_PROJ_BEAM_AZIMUTH projected), a kernel of its own so
// that k_reverse keeps its operands: the column's yaw as above (SECTOR or the full circle) is the NOMINAL one, and the beam of
// the cell's row looks az[row] to its left -- yaw = nominal - az[row].  The row is proj_y clamped like the Brad read, or --
// float64 coordinates, where py holds the pitch -- the cell's own row i / W.  The pitch is the table's rule.
template <typename P, int SECTOR>
__global__ __launch_bounds__(256) void k_reverse_az(const float* __restrict__ range, const P* __restrict__ px,
                                                    const P* __restrict__ py, int H, int W, const double* __restrict__ Brad,
                                                    const double* __restrict__ az, double yc, double span,
                                                    double* __restrict__ out) {
  constexpr bool is_float = std::is_same<P, double>::value;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const double depth = (double)range[i];
  double yaw;
  if (SECTOR) {
    const double x = is_float ? (double)px[i] / (double)W : ((double)px[i] + 0.5) / (double)W;
    yaw = yc + (x - 0.5) * span;
  } else {
    const double x = (double)px[i] / (double)W;
    yaw = (x * 2 - 1.0) * M_PI;
  }
  int r = is_float ? i / W : (int)py[i];
  r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
  yaw = yaw - az[r];
  const double e = is_float ? (double)py[i] : Brad[r];
  const double pitch = M_PI / 2 - e;
  const double sp = sin(pitch);
  out[3 * (size_t)i] = depth * sp * cos(-yaw);
  out[3 * (size_t)i + 1] = depth * sp * sin(-yaw);
  out[3 * (size_t)i + 2] = depth * cos(pitch);
}

extern "C" int lt_reverse_projection_beams_az_dev(const float* range_img, const void* proj_x, const void* proj_y_or_pitch,
                                                  int preserve_float, const double* Brad, const double* az_rad,
                                                  const double* sector, int H, int W, double* back_points, void* stream) {
  bool ok = H > 0 && W > 0 && range_img && proj_x && proj_y_or_pitch && back_points && (preserve_float || Brad) && az_rad;
  if (ok && sector) ok = fabs(sector[0]) <= M_PI && sector[1] > 0.0 && sector[1] < 2 * M_PI;
  if (!ok) {
    lt_set_error("lt_reverse_projection_beams_az_dev: invalid argument (H=%d W=%d; the table, the offsets, a sector with "
                 "|yaw_center| <= pi and 0 < span < 2 pi)", H, W);
    return LT_ERR_INVALID_ARG;
  }
  const double yc = sector ? sector[0] : 0.0, span = sector ? sector[1] : 0.0;
  const dim3 grid((H * W + 255) / 256), block(256);
  hipStream_t st = (hipStream_t)stream;
#define LT_REVERSE_AZ(P, S)                                                                                         \
  hipLaunchKernelGGL((k_reverse_az<P, S>), grid, block, 0, st, range_img, (const P*)proj_x, (const P*)proj_y_or_pitch, \
                     H, W, Brad, az_rad, yc, span, back_points)
  if (preserve_float) { if (sector) LT_REVERSE_AZ(double, 1); else LT_REVERSE_AZ(double, 0); }
  else { if (sector) LT_REVERSE_AZ(int, 1); else LT_REVERSE_AZ(int, 0); }
#undef LT_REVERSE_AZ
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// ---- rendered points into another frame (the target sensor's, when it is mounted at a pose of its own) ----------
// float32 point widened to float64, ((m0 * x + m1 * y) + m2 * z) + m3 per row of T (lt_ingest_scans_dev's row form; every
// product and sum rounded on its own), rounded to float32.  Rows with tri < 0 (misses) are copied as they are: (0, 0, 0)
// stays (0, 0, 0) for write()'s filter.  One thread per point reads its three floats before it writes them (out may be
// points); 12-byte rows: three 4-byte accesses, nothing wider is aligned.
struct lt_mat12 { double m[12]; };

__global__ __launch_bounds__(256) void k_points_to_frame(const float* pts, const int* __restrict__ tri, int n,
                                                         lt_mat12 T, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float fx = pts[3 * (size_t)i], fy = pts[3 * (size_t)i + 1], fz = pts[3 * (size_t)i + 2];
  if (tri && tri[i] < 0) {
    out[3 * (size_t)i] = fx;
    out[3 * (size_t)i + 1] = fy;
    out[3 * (size_t)i + 2] = fz;
    return;
  }
  const double x = (double)fx, y = (double)fy, z = (double)fz;
  out[3 * (size_t)i] = (float)(((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3]);
  out[3 * (size_t)i + 1] = (float)(((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7]);
  out[3 * (size_t)i + 2] = (float)(((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11]);
}

extern "C" int lt_points_to_frame_dev(const float* points, const int* tri, int n, const double* T, float* out,
                                      void* stream) {
  if (n < 0 || !T || (n > 0 && (!points || !out))) {
    lt_set_error("lt_points_to_frame_dev: invalid argument (n=%d)", n);
    return LT_ERR_INVALID_ARG;
  }
  if (n == 0) return LT_OK;
  lt_mat12 M;
  for (int k = 0; k < 12; ++k) M.m[k] = T[k];
  hipLaunchKernelGGL(k_points_to_frame, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, points, tri, n, M, out);
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// ---- scan packer ----------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ bool pack_keep(const T* __restrict__ pts, const int* __restrict__ label,
                                          const int* __restrict__ index, int i) {
  if (index && !(index[i] > 0)) return false;            // 'cp': index > 0 (laserscan.py:1138)
  if (label[i] < 0) return false;                        // laserscan.py:1147
  const T s = (pts[3 * (size_t)i] + pts[3 * (size_t)i + 1]) + pts[3 * (size_t)i + 2];
  return s != (T)0;                                      // remove points with (0, 0, 0) (laserscan.py:1151)
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack_count(const T* __restrict__ pts, const int* __restrict__ label,
                                                    const int* __restrict__ index, int n,
                                                    int* __restrict__ blockcount) {
  __shared__ int wcnt[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool keep = i < n && pack_keep<T>(pts, label, index, i);
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blockcount[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(1024) void k_pack_scan(int* __restrict__ blockcount, int nblocks) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nblocks; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nblocks ? blockcount[i] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    if (i < nblocks) blockcount[i] = carry + woff + inc - v;
    if (threadIdx.x == 1023) carry_s = carry + woff + inc;
    __syncthreads();
    carry = carry_s;
  }
  if (threadIdx.x == 0) blockcount[nblocks] = carry;
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack_write(const T* __restrict__ pts, const float* __restrict__ rem,
                                                    const int* __restrict__ label, const int* __restrict__ index,
                                                    int n, const int* __restrict__ blockoff,
                                                    float4* __restrict__ out_bin, unsigned* __restrict__ out_label) {
  __shared__ int wcnt[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool keep = i < n && pack_keep<T>(pts, label, index, i);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int k = blockoff[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) k += wcnt[w];
  // struct.pack("ffff", x, y, z, remission): double -> float conversion rounds to nearest, as C does
  out_bin[k] = make_float4((float)pts[3 * (size_t)i], (float)pts[3 * (size_t)i + 1], (float)pts[3 * (size_t)i + 2],
                           rem[i]);
  out_label[k] = (unsigned)label[i];
}

namespace {
std::mutex g_post_mu;
int* g_blockcount = nullptr;
size_t g_blockcount_cap = 0;
int g_post_dev = -1;
}  // namespace

extern "C" int lt_pack_scan_dev(const void* points, int is_f64, const float* rem, const int* label,
                                const int* index, int n, float* out_bin, unsigned* out_label, int* n_out,
                                void* stream) {
  if (n < 0 || (n > 0 && (!points || !rem || !label || !out_bin || !out_label))) {
    lt_set_error("lt_pack_scan_dev: invalid argument (n=%d)", n);
    return LT_ERR_INVALID_ARG;
  }
  if (n_out) *n_out = 0;
  if (n == 0) return LT_OK;
  std::lock_guard<std::mutex> lock(g_post_mu);
  int dev = 0;
  LT_HIP(hipGetDevice(&dev));
  const int nb = (n + 255) / 256;
  if (dev != g_post_dev || (size_t)nb + 2 > g_blockcount_cap) {
    const size_t cap = (size_t)nb * 2 + 1024;
    const lt_dev_array counts[] = {{(void**)&g_blockcount, cap * sizeof(int)}};
    LT_CHECK(lt_dev_replace("lt_pack_scan_dev", lt_wait_device(), &g_blockcount_cap, cap, counts));
    g_post_dev = dev;
  }
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) {
    hipLaunchKernelGGL(k_pack_count<double>, dim3(nb), dim3(256), 0, st, (const double*)points, label, index, n,
                       g_blockcount);
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, st, g_blockcount, nb);
    hipLaunchKernelGGL(k_pack_write<double>, dim3(nb), dim3(256), 0, st, (const double*)points, rem, label, index, n,
                       (const int*)g_blockcount, (float4*)out_bin, out_label);
  } else {
    hipLaunchKernelGGL(k_pack_count<float>, dim3(nb), dim3(256), 0, st, (const float*)points, label, index, n,
                       g_blockcount);
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, st, g_blockcount, nb);
    hipLaunchKernelGGL(k_pack_write<float>, dim3(nb), dim3(256), 0, st, (const float*)points, rem, label, index, n,
                       (const int*)g_blockcount, (float4*)out_bin, out_label);
  }
  LT_HIP(hipGetLastError());
  int kept = 0;
  LT_HIP(hipMemcpyAsync(&kept, g_blockcount + nb, sizeof(int), hipMemcpyDeviceToHost, st));
  LT_HIP(hipStreamSynchronize(st));
  if (n_out) *n_out = kept;
  return LT_OK;
}

// ---- compare: masked confusion matrix + squared differences ----------------------------------------------------
// Masks as laserscan.py:1200-1210: cells whose SOURCE colour is black, or whose source label is 0, are
// background in both images.  conf[pred = target][gt = source] += 1 over raw label values < n_labels
// (np_ioueval.py:40-47: rows = predictions, columns = ground truth).
__global__ __launch_bounds__(256) void k_compare(const int* __restrict__ src_label, const float* __restrict__ src_color,
                                                 const int* __restrict__ tgt_label, const float* __restrict__ src_range,
                                                 const float* __restrict__ tgt_range, const float* __restrict__ src_rem,
                                                 const float* __restrict__ tgt_rem, int n, int n_labels,
                                                 unsigned long long* __restrict__ conf, float* __restrict__ range_diff,
                                                 float* __restrict__ rem_diff, int* __restrict__ src_masked,
                                                 int* __restrict__ tgt_masked, double* __restrict__ sq_sum) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  bool counted = false;
  unsigned pair = 0u;
  if (i < n) {
    const float csum = (src_color[3 * (size_t)i] + src_color[3 * (size_t)i + 1]) + src_color[3 * (size_t)i + 2];
    int sl = src_label[i], tl = tgt_label[i];
    if (csum == 0.f) { sl = 0; tl = 0; }
    const bool bg = sl == 0;
    if (bg) tl = 0;
    if (src_masked) src_masked[i] = sl;
    if (tgt_masked) tgt_masked[i] = tl;
    counted = (unsigned)sl < (unsigned)n_labels && (unsigned)tl < (unsigned)n_labels;
    pair = counted ? (unsigned)tl * (unsigned)n_labels + (unsigned)sl : 0u;
    const float sr = bg ? 0.f : src_range[i], tr = bg ? 0.f : tgt_range[i];
    const float d = sr - tr;
    const float d2 = d * d;
    if (range_diff) range_diff[i] = d2;
    sq = (double)d2;
    if (rem_diff) {
      const float a = bg ? 0.f : src_rem[i], b = bg ? 0.f : tgt_rem[i];
      rem_diff[i] = (a - b) * (a - b);
    }
  }
  // the confusion matrix: an image holds a handful of label pairs, so an atomic per cell is tens of thousands of memory-side
  // atomics in a row on the same few words (~12 ns each).  The lanes of a wave that hold the same pair count themselves with
  // ballots; one atomic per distinct pair and wave.
  for (unsigned long long rest = __ballot(counted); rest;) {
    const int leader = __ffsll((long long)rest) - 1;
    const unsigned k = (unsigned)__shfl((int)pair, leader, 64);
    const unsigned long long same = __ballot(counted && pair == k);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&conf[k], (unsigned long long)__popcll(same));
    rest &= ~same;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sq_sum, (red[0] + red[1]) + (red[2] + red[3]));
}

extern "C" int lt_compare_dev(const int* src_label, const float* src_color, const int* tgt_label,
                              const float* src_range, const float* tgt_range, const float* src_rem,
                              const float* tgt_rem, int n, int n_labels, unsigned long long* conf,
                              float* range_diff, float* rem_diff, int* src_masked, int* tgt_masked,
                              double* sq_sum, void* stream) {
  if (n < 0 || n_labels <= 0 || !src_label || !src_color || !tgt_label || !src_range || !tgt_range || !conf ||
      !sq_sum || (rem_diff && (!src_rem || !tgt_rem))) {
    lt_set_error("lt_compare_dev: invalid argument");
    return LT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  LT_HIP(hipMemsetAsync(conf, 0, (size_t)n_labels * n_labels * sizeof(unsigned long long), st));
  LT_HIP(hipMemsetAsync(sq_sum, 0, sizeof(double), st));
  if (n > 0)
    hipLaunchKernelGGL(k_compare, dim3((n + 255) / 256), dim3(256), 0, st, src_label, src_color, tgt_label, src_range,
                       tgt_range, src_rem, tgt_rem, n, n_labels, conf, range_diff, rem_diff, src_masked, tgt_masked,
                       sq_sum);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
