// lt_project.hip -- point cloud -> spherical range image with atomic z-min on gfx950.
//
// Replaces the numpy / pure-Python projections of the reference's scan model:
//   LaserScan.do_range_projection        auxiliary/laserscan.py:202-292  (argsort by depth, scatter)
//   LaserScan.do_range_projection_new    auxiliary/laserscan.py:294-391  (per-point Python z-min loop)
//   SemLaserScan.do_label_projection[_new]  auxiliary/laserscan.py:645-649, :672-676
// and create_rays (auxiliary/laserscan.py:1092-1119) as a device kernel.
//
// Semantics: the closest point of a cell wins; among equal depths the LOWEST point index wins --
// the `_new` loop (`depth[i] < range_image[...]`, laserscan.py:376) and one valid outcome of the
// unstable argsort of the old variant.  Implemented as ONE order-independent atomicMin per kept point
// of a 64-bit key per cell that holds the depth and the index (`The key`, below); every entry point
// -- one cloud or a batch -- runs the same kernels.
//
// Arithmetic follows numpy's dtype rules for the array the reference holds: float32 when the scan
// was read from file (laserscan.py:131-136), float64 after a pose was applied (laserscan.py:98-104).
// float32 transcendental results are the correctly rounded value (computed in double, rounded once).
#include "lt_internal.h"
#include "lt_layouts.h"
#include "lt_projpoint.h"  // project_point, pb_key: shared with lt_evaluate.hip
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>

// ---- create_rays (laserscan.py:1092-1119): float64 trigonometry, cast to float32 last ---------------------
// One body for every target sensor.  The three choices are template arguments: as flags read at run time they cost the plain
// sensor (lt_create_rays_dev, 64 x 2048) 0.18 us per call, more than its run-to-run spread (profiles/projection_model).
//   column  the full circle: np.linspace(0, 360, W), + 180, wrapped.  SECTOR: column w is the cell [w, w + 1) * span / W
//           counted clockwise from the sector's left edge, and its ray leaves through the cell's CENTRE -- not wrapped (sin
//           and cos are periodic)
//   row     np.linspace(fov_up, fov_down, H), or -- BEAMS: `beams_deg` (device, [H]) -- the table's angle (degrees) of row h
//           AZ (with BEAMS): beam h looks beams_deg[H + h] degrees to the LEFT of its column's nominal direction (the
//           per-beam azimuth offsets, behind the table in the same buffer): yaw_deg = nominal(w) - offset, no further wrap
//   pose    POSED: the direction, still in float64, turned by the row-major rotation R of the sensor's pose --
//           ((r0 * x + r1 * y) + r2 * z) per component, every product and sum rounded on its own (-ffp-contract=off).
//           Unposed rays are cast as they are, not turned by the identity: -0.0 + 0.0 is +0.0
struct lt_rot9 { double m[9]; };

template <int BEAMS, int SECTOR, int POSED, int AZ = 0>
__global__ __launch_bounds__(256) void k_create_rays(const double* __restrict__ beams_deg, double fov_up, double fov_down,
                                                     int H, int W, double center_deg, double span_deg, lt_rot9 R,
                                                     float* __restrict__ rays) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * W) return;
  const int h = idx / W, w = idx - h * W;
  double yaw_deg;
  if (SECTOR) {
    yaw_deg = (-center_deg - span_deg / 2) + (w + 0.5) * (span_deg / W);
  } else {
    // np.linspace(a, b, n)[i] = a + i * ((b - a) / (n - 1)), last element forced to b
    yaw_deg = W > 1 ? (w == W - 1 ? 360.0 : 0.0 + w * (360.0 / (W - 1))) : 0.0;
    yaw_deg += 180.0;
    if (yaw_deg > 360.0) yaw_deg -= 360.0;
  }
  if (BEAMS && AZ) yaw_deg = yaw_deg - beams_deg[H + h];
  const double yaw = yaw_deg / 180. * M_PI;
  const double pd = BEAMS ? beams_deg[h]
                        : (H > 1 ? (h == H - 1 ? fov_down : fov_up + h * ((fov_down - fov_up) / (H - 1))) : fov_up);
  const double p = M_PI / 2 - pd / 180. * M_PI;
  const double sp = sin(p);
  const double x = sp * cos(-yaw), y = sp * sin(-yaw), z = cos(p) * 1.0;
  if (POSED) {
    rays[3 * (size_t)idx] = (float)((R.m[0] * x + R.m[1] * y) + R.m[2] * z);
    rays[3 * (size_t)idx + 1] = (float)((R.m[3] * x + R.m[4] * y) + R.m[5] * z);
    rays[3 * (size_t)idx + 2] = (float)((R.m[6] * x + R.m[7] * y) + R.m[8] * z);
  } else {
    rays[3 * (size_t)idx] = (float)x;
    rays[3 * (size_t)idx + 1] = (float)y;
    rays[3 * (size_t)idx + 2] = (float)z;
  }
}

// `beams_deg` (host, [H]) or NULL, `az_deg` (host, [H]; with a table only) or NULL, `sec` = (center, span) in degrees or
// NULL, `rot` (host, [9]) or NULL.  Without a table the launch is asynchronous.  With one (once per sensor model) the table
// -- and the offsets behind it -- go to the device in a buffer of this call, which waits for its kernel.
static int create_rays_launch(const double* beams_deg, const double* az_deg, double fov_up, double fov_down, int H, int W,
                              const double* sec, const double* rot, float* rays, hipStream_t st) {
  lt_rot9 R;
  for (int k = 0; k < 9; ++k) R.m[k] = rot ? rot[k] : 0.0;  // (read by the POSED kernels only)
  const dim3 grid((H * W + 255) / 256), block(256);
  const double center_deg = sec ? sec[0] : 0.0, span_deg = sec ? sec[1] : 0.0;
  double* d_beams = nullptr;
  hipError_t e = hipSuccess;
  if (beams_deg) {
    LT_HIP(hipMalloc((void**)&d_beams, (size_t)H * (az_deg ? 2 : 1) * sizeof(double)));
    e = hipMemcpyAsync(d_beams, beams_deg, (size_t)H * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && az_deg)
      e = hipMemcpyAsync(d_beams + H, az_deg, (size_t)H * sizeof(double), hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess) {
#define LT_RAYS(B, S, P, AZ)                                                                                          \
  hipLaunchKernelGGL((k_create_rays<B, S, P, AZ>), grid, block, 0, st, (const double*)d_beams, fov_up, fov_down, H, W, \
                     center_deg, span_deg, R, rays)
#define LT_RAYS_POSED(B, S, AZ) LT_RAYS(B, S, 1, AZ)
#define LT_RAYS_UNPOSED(B, S, AZ) LT_RAYS(B, S, 0, AZ)
    if (rot) LT_FOR_MODEL(beams_deg != nullptr, sec != nullptr, az_deg != nullptr, LT_RAYS_POSED);
    else LT_FOR_MODEL(beams_deg != nullptr, sec != nullptr, az_deg != nullptr, LT_RAYS_UNPOSED);
#undef LT_RAYS
#undef LT_RAYS_POSED
#undef LT_RAYS_UNPOSED
    e = hipGetLastError();
  }
  if (beams_deg) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_beams);
  }
  LT_HIP(e);
  return LT_OK;
}

extern "C" int lt_create_rays_dev(double fov_up, double fov_down, int H, int W, float* rays, void* stream) {
  if (H <= 0 || W <= 0 || !rays) {
    lt_set_error("lt_create_rays_dev: invalid argument (H=%d W=%d)", H, W);
    return LT_ERR_INVALID_ARG;
  }
  return create_rays_launch(nullptr, nullptr, fov_up, fov_down, H, W, nullptr, nullptr, rays, (hipStream_t)stream);
}

extern "C" int lt_create_rays_pose_dev(double fov_up, double fov_down, int H, int W, const double* rot, float* rays,
                                       void* stream) {
  if (!rot) return lt_create_rays_dev(fov_up, fov_down, H, W, rays, stream);
  if (H <= 0 || W <= 0 || !rays) {
    lt_set_error("lt_create_rays_pose_dev: invalid argument (H=%d W=%d)", H, W);
    return LT_ERR_INVALID_ARG;
  }
  return create_rays_launch(nullptr, nullptr, fov_up, fov_down, H, W, nullptr, rot, rays, (hipStream_t)stream);
}

extern "C" int lt_create_rays_beams_dev(const double* beams_deg, int H, int W, const double* rot, float* rays,
                                        void* stream) {
  if (!beams_deg || H <= 0 || W <= 0 || !rays) {
    lt_set_error("lt_create_rays_beams_dev: invalid argument (H=%d W=%d)", H, W);
    return LT_ERR_INVALID_ARG;
  }
  return create_rays_launch(beams_deg, nullptr, 0.0, 0.0, H, W, nullptr, rot, rays, (hipStream_t)stream);
}

extern "C" int lt_create_rays_sector_dev(const double* beams_deg, double fov_up, double fov_down, int H, int W,
                                         double center_deg, double span_deg, const double* rot, float* rays, void* stream) {
  if (H <= 0 || W <= 0 || !rays || !(fabs(center_deg) <= 360.0) || !(span_deg > 0.0 && span_deg < 360.0)) {
    lt_set_error("lt_create_rays_sector_dev: invalid argument (H=%d W=%d center=%g span=%g)", H, W, center_deg, span_deg);
    return LT_ERR_INVALID_ARG;
  }
  const double sec[2] = {center_deg, span_deg};
  return create_rays_launch(beams_deg, nullptr, fov_up, fov_down, H, W, sec, rot, rays, (hipStream_t)stream);
}

extern "C" int lt_create_rays_beams_az_dev(const double* beams_deg, const double* az_deg, int H, int W, const double* sec,
                                           const double* rot, float* rays, void* stream) {
  bool ok = beams_deg && H > 0 && W > 0 && rays;
  if (ok && sec) ok = fabs(sec[0]) <= 360.0 && sec[1] > 0.0 && sec[1] < 360.0;
  if (ok && az_deg)
    for (int h = 0; h < H; ++h) ok = ok && fabs(az_deg[h]) <= 90.0;  // (NaN: not)
  if (!ok) {
    lt_set_error("lt_create_rays_beams_az_dev: invalid argument (H=%d W=%d; a table, offsets within +-90 degrees, a sector "
                 "with |center| <= 360 and 0 < span < 360)", H, W);
    return LT_ERR_INVALID_ARG;
  }
  return create_rays_launch(beams_deg, az_deg, 0.0, 0.0, H, W, sec, rot, rays, (hipStream_t)stream);
}

// The doubles a projection uploads for its sensor model, into `tab` [LT_MODEL_DOUBLES]; returns their number (0: none), -1
// when the arguments do not fit the flags.  Layout (project_model reads it):
//   neither flag          the caller's n_beams hard-coded angles (n_beams may be 0)
//   LT_PROJ_BEAM_ROWS     the caller's table (Brad[H], halfw[H]) checked and completed by the field of view in radians,
//                         which the H == 1 keep rule reads: 2 * H + 2 doubles
//   LT_PROJ_BEAM_AZIMUTH  behind the completed table, the H azimuth offsets of its rows in radians -- from
//                         lt_projector_set_beam_azimuth / lt_range_projection_set_beam_azimuth (`az`, `n_az` of them; NULL:
//                         none were set)
//   LT_PROJ_SECTOR        behind either (and the offsets), the two numbers of the sector -- the yaw of its middle (|.| <= pi)
//                         and its width (in (0, 2 pi)), radians -- from lt_projector_set_sector /
//                         lt_range_projection_set_sector (`sec`, NULL: none was set)
// Declared in lt_internal.h with the two checks below: the target view of lt_evaluate.hip lays its model out with them too.
int model_table(const char* who, const double* beam_angles, int n_beams, unsigned flags, double fov_up_deg,
                double fov_down_deg, int H, const double* sec, const double* az, int n_az, double* tab) {
  const bool rows = (flags & LT_PROJ_BEAM_ROWS) != 0, sector = (flags & LT_PROJ_SECTOR) != 0;
  const bool azimuth = (flags & LT_PROJ_BEAM_AZIMUTH) != 0;
  const unsigned with_az = LT_PROJ_BEAM_AZIMUTH | LT_PROJ_BEAM_ROWS | LT_PROJ_NEW | LT_PROJ_REMOVE;
  if (azimuth && ((flags & ~LT_PROJ_SECTOR) != with_az || !az || n_az != H)) {
    lt_set_error("%s: LT_PROJ_BEAM_AZIMUTH goes with LT_PROJ_BEAM_ROWS | LT_PROJ_NEW | LT_PROJ_REMOVE only, with or without "
                 "LT_PROJ_SECTOR (flags=%u), and after the offsets of exactly H rows were set (%d were; H=%d)", who, flags,
                 az ? n_az : 0, H);
    return -1;
  }
  flags &= ~LT_PROJ_BEAM_AZIMUTH;  // (checked; the two rules below are what they were)
  if (rows && ((flags & ~LT_PROJ_SECTOR) != (LT_PROJ_BEAM_ROWS | LT_PROJ_NEW | LT_PROJ_REMOVE) || n_beams != H || !beam_angles ||
               2 * H + 2 > 1024)) {
    lt_set_error("%s: LT_PROJ_BEAM_ROWS goes with LT_PROJ_NEW | LT_PROJ_REMOVE only (flags=%u) and a table of n_beams == H "
                 "<= 511 rows (n_beams=%d H=%d)", who, flags & ~LT_PROJ_SECTOR, n_beams, H);
    return -1;
  }
  const int n_given = rows ? 2 * H : n_beams;      // doubles of the caller's
  int n_rows = rows ? 2 * H + 2 : n_beams;         // ... and of the row model that the kernels read
  if (sector && ((flags & ~LT_PROJ_BEAM_ROWS) != (LT_PROJ_SECTOR | LT_PROJ_NEW | LT_PROJ_REMOVE) || !sec || n_beams < 0 ||
                 (n_beams > 0 && !beam_angles) || n_rows + 2 > 1024)) {
    lt_set_error("%s: LT_PROJ_SECTOR goes with LT_PROJ_NEW | LT_PROJ_REMOVE only, with or without LT_PROJ_BEAM_ROWS (flags=%u), "
                 "and after the sector was set (%s; n_beams=%d)", who, flags, sec ? "it was" : "it was not", n_beams);
    return -1;
  }
  if (n_given > 0) memcpy(tab, beam_angles, (size_t)n_given * sizeof(double));
  if (rows) {
    tab[2 * H] = fov_down_deg / 180.0 * M_PI;
    tab[2 * H + 1] = fov_up_deg / 180.0 * M_PI;
  }
  if (azimuth) {  // (H <= 511: 3 H + 2 + 2 <= LT_MODEL_DOUBLES)
    memcpy(tab + n_rows, az, (size_t)H * sizeof(double));
    n_rows += H;
  }
  if (sector) {
    tab[n_rows] = sec[0];
    tab[n_rows + 1] = sec[1];
  }
  return n_rows + (sector ? 2 : 0);
}

bool sector_ok(const char* who, double yaw_center, double span) {
  if (!(fabs(yaw_center) <= M_PI) || !(span > 0.0 && span < 2 * M_PI)) {
    lt_set_error("%s: yaw of the sector's middle %g (|.| <= pi) and width %g (0 < . < 2 pi), radians", who, yaw_center, span);
    return false;
  }
  return true;
}

// the offsets of LT_PROJ_BEAM_AZIMUTH: `az` [n] radians, finite and within +-pi/2, for 1 .. 511 rows; NULL or n == 0 clears
bool beam_azimuth_ok(const char* who, const double* az, int n) {
  bool ok = (!az || n == 0) || (n > 0 && n <= 511);
  if (ok && az)
    for (int h = 0; h < n; ++h) ok = ok && fabs(az[h]) <= M_PI / 2;  // (NaN: not)
  if (!ok) lt_set_error("%s: the azimuth offsets of 1 .. 511 rows, radians, each finite and within +-pi/2 (n=%d)", who, n);
  return ok;
}

// ---- the projection: up to LT_PB_MAX clouds per launch sequence, nothing read back by the host ---------------------------
// lt_range_projection_batch_dev projects the `number_of_scans` clouds of one output scan (laserscan.py:874-881:
// do_range_projection_new + do_label_projection_new per scan) in ONE launch sequence on the caller's stream;
// lt_range_projection_dev is the same sequence for one cloud, plus the compaction of its kept points:
//   k_pb_project   a thread per point of every cloud: the reference's per-point expressions (project_model, lt_projpoint.h)
//                  and ONE 64-bit atomicMin per kept point -- no per-point temporaries are written;
//   [k_pb_assign]  only for the OLD variant on float64 clouds, whose order key (a float64 depth) leaves no room for the index
//   [k_pb_prefix]  only when an output needs the numbering of the KEPT points (idx / mask images, proj_x .. images, n_kept,
//                  the compaction)
//   k_pb_resolve   a thread per cell of every image: decodes the winner, RE-COMPUTES its projection from the point itself
//                  (the same deterministic function), gathers remission / label / colour, writes the images and re-arms the
//                  cell's key for the next call (no memsets between calls)
//   [k_pb_compact] lt_range_projection_dev only: a thread per point writes the kept points' rows, in input order.
// The key.  `_new` keeps its running minimum in a float32 image and replaces when `depth[i] < image` (laserscan.py:366, :376):
// the winner is the first point of the minimum's float32 bucket unless points of that bucket lie BELOW the float32 value
// (rounded up) -- then the last of those.  hi word = float32 bits of the depth (positive floats order like unsigned
// integers); lo word = 0x7fffffff - index for a rounded-up point (they beat the others, the highest index first),
// 0x80000000 | index otherwise (lowest index first): one atomicMin yields exactly that point.  float32 clouds never round.
// The OLD variant on float32 clouds: closest point, lowest index among equal depths -- the same key.
#define LT_PB_MAX 8

struct pb_cloud {
  const void* pts; const float* rem; const unsigned* label;
  int n, block0;                 // points; first workgroup of this cloud in the per-point grids
  unsigned long long* key;       // [cells] z-min key, LT_PB_EMPTY when no point fell into the cell
  unsigned long long* dmin;      // [cells] float64 depth bits (OLD variant on float64 clouds), else unused
  unsigned long long* keep;      // [ceil(n / 64)] kept-point mask per wave of k_pb_project
  int* wprefix;                  // [ceil(n / 64)] kept points before the wave (k_pb_prefix)
  int* meta;                     // [2] number of kept points, original index of the last kept point (-1: none)
  int* idx_img; float* range_img; float* xyz_img; float* rem_img; int* label_img; float* color_img; float* mask_img;
  float* fold_img; int* px_img; int* py_img; void* xf_img; void* yf_img; int* n_kept;
  unsigned long long* bacc;      // [blocks of the cloud][6] per-WORKGROUP order-preserving keys of the kept points' bounds (min x,
                                 // max x, min y, ...), written by k_pb_project, folded by k_pb_prefix / k_pb_bnds; NULL: not wanted
  double* bnds_out;              // [6] get_bnds() of the kept points (laserscan.py:678-681), written by k_pb_prefix
};
struct pb_args { pb_cloud c[LT_PB_MAX]; int n_clouds; };

__device__ __forceinline__ int pb_find_cloud(const pb_args& A, int block) {
  int c = 0;
#pragma unroll
  for (int k = 1; k < LT_PB_MAX; ++k)
    if (k < A.n_clouds && block >= A.c[k].block0) c = k;
  return c;
}

// order-preserving map double -> uint64 (and back): unsigned comparison of the keys == comparison of the values
__device__ __forceinline__ unsigned long long pb_ord(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double pb_unord(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// MODE 0: the single-key variants (NEW on any dtype, OLD on float32).  MODE 1: OLD on float64 -- depth minimum only.
// BEAMS, SECTOR, AZ and `beams`: project_model; MODE 0 only.
template <typename T, int MODE, int BEAMS, int SECTOR, int AZ = 0>
__global__ __launch_bounds__(256) void k_pb_project(pb_args A, T pi_t, T abs_fov_down, T fov, int H, int W,
                                                    const double* __restrict__ beams, int n_beams, int drop_zero,
                                                    int drop_outside) {
  const int ci = pb_find_cloud(A, blockIdx.x);
  const pb_cloud& c = A.c[ci];
  const int i = (blockIdx.x - c.block0) * 256 + threadIdx.x;
  bool keep = false;
  if (i < c.n) {
    const T* pts = (const T*)c.pts;
    const T x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const proj_out<T> o = project_model<T, BEAMS, SECTOR, AZ>(x, y, z, pi_t, abs_fov_down, fov, H, W, beams, n_beams,
                                                              drop_zero, drop_outside);
    keep = o.cell >= 0;
    if (keep) {
      if (MODE == 0) atomicMin(&c.key[o.cell], pb_key<T>(o.depth, i));
      else atomicMin(&c.dmin[o.cell], (unsigned long long)__double_as_longlong((double)o.depth));
    }
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && i < c.n) c.keep[i >> 6] = m;
  if (c.bacc) {  // bounds of the kept points: SemLaserScan.get_bnds after remove_points (laserscan.py:678-681)
    // Per WORKGROUP, no atomics: six shared words for the whole cloud were 2 000 memory-side atomics in a row per word (150 us
    // for a 130 k-point cloud), and even LOOKING at them first (a load per wave on six hot addresses) cost 25 us.
    __shared__ unsigned long long s_b[4][6];
    const T* pts = (const T*)c.pts;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double q = keep ? (double)pts[3 * (size_t)i + a] : 0.0;
      unsigned long long lo = keep ? pb_ord(q) : ~0ull, hi = keep ? pb_ord(q) : 0ull;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      if ((threadIdx.x & 63) == 0) { s_b[threadIdx.x >> 6][2 * a] = lo; s_b[threadIdx.x >> 6][2 * a + 1] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
      unsigned long long v = s_b[0][threadIdx.x];
      for (int w = 1; w < 4; ++w) {
        const unsigned long long o = s_b[w][threadIdx.x];
        v = (threadIdx.x & 1) ? (o > v ? o : v) : (o < v ? o : v);
      }
      c.bacc[6 * (size_t)(blockIdx.x - c.block0) + threadIdx.x] = v;
    }
  }
}

// fold the workgroups' partial bounds of a cloud (all 64 lanes of one wave help); lane k < 6 writes word k
__device__ __forceinline__ void pb_fold_bounds(const pb_cloud& c, int lane) {
  const int nb = (c.n + 255) >> 8;
  unsigned long long v[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = (k & 1) ? 0ull : ~0ull;
  for (int b = lane; b < nb; b += 64)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const unsigned long long o = c.bacc[6 * (size_t)b + k];
      v[k] = (k & 1) ? (o > v[k] ? o : v[k]) : (o < v[k] ? o : v[k]);
    }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long x = __shfl_xor(v[k], o);
      v[k] = (k & 1) ? (x > v[k] ? x : v[k]) : (x < v[k] ? x : v[k]);
    }
    if (lane == k) {  // no kept point: (+inf, -inf) -- numpy's amin of an empty array raises
      const bool is_min = (k & 1) == 0;
      const bool none = is_min ? v[k] == ~0ull : v[k] == 0ull;
      c.bnds_out[k] = none ? (is_min ? (double)INFINITY : -(double)INFINITY) : pb_unord(v[k]);
    }
  }
}

// OLD variant, float64: among the points that equal the cell's depth minimum the lowest index wins
__global__ __launch_bounds__(256) void k_pb_assign(pb_args A, double pi_t, double abs_fov_down, double fov, int H, int W,
                                                   const double* __restrict__ beams, int n_beams, int drop_zero,
                                                   int drop_outside) {
  const int ci = pb_find_cloud(A, blockIdx.x);
  const pb_cloud& c = A.c[ci];
  const int i = (blockIdx.x - c.block0) * 256 + threadIdx.x;
  if (i >= c.n) return;
  if (!((c.keep[i >> 6] >> (i & 63)) & 1ull)) return;
  const double* pts = (const double*)c.pts;
  const proj_out<double> o = project_point<double>(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], pi_t,
                                                   abs_fov_down, fov, H, W, beams, n_beams, drop_zero, drop_outside);
  if ((unsigned long long)__double_as_longlong(o.depth) == c.dmin[o.cell])
    atomicMin(&c.key[o.cell], (unsigned long long)(0x80000000u | (unsigned)i));
}

// one workgroup per cloud: exclusive prefix of the waves' kept counts, the total, the last kept point
__global__ __launch_bounds__(256) void k_pb_prefix(pb_args A) {
  __shared__ int part[256];
  __shared__ int last_s;
  const pb_cloud& c = A.c[blockIdx.x];
  const int nw = (c.n + 63) >> 6;
  const int per = (nw + 255) / 256;
  const int w0 = threadIdx.x * per, w1 = min(nw, w0 + per);
  if (threadIdx.x == 0) last_s = -1;
  int sum = 0, last = -1;
  for (int w = w0; w < w1; ++w) {
    const unsigned long long m = c.keep[w];
    sum += __popcll(m);
    if (m) last = w * 64 + 63 - __clzll((long long)m);
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  if (last >= 0) atomicMax(&last_s, last);
  // Hillis-Steele over 256 partials
  for (int o = 1; o < 256; o <<= 1) {
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - sum;
  for (int w = w0; w < w1; ++w) {
    c.wprefix[w] = run;
    run += __popcll(c.keep[w]);
  }
  if (threadIdx.x == 255) {
    c.meta[0] = part[255];
    c.meta[1] = last_s;
    if (c.n_kept) *c.n_kept = part[255];
  }
  if (c.bacc && threadIdx.x < 64) pb_fold_bounds(c, threadIdx.x);
}

// the bounds alone (no image wants the kept points' prefix): one thread per word, one workgroup per cloud
__global__ __launch_bounds__(64) void k_pb_bnds(pb_args A) {
  const pb_cloud& c = A.c[blockIdx.x];
  if (c.bacc) pb_fold_bounds(c, threadIdx.x);
}

template <typename T, int MODE, int BEAMS, int SECTOR, int AZ = 0>
__global__ __launch_bounds__(256) void k_pb_resolve(pb_args A, int blocks_per_cloud, T pi_t, T abs_fov_down, T fov, int H,
                                                    int W, const double* __restrict__ beams, int n_beams, int drop_zero,
                                                    int drop_outside, const float* __restrict__ lut, int lut_len,
                                                    float range_init, float rem_init, float xyz_init, int have_prefix) {
  const int ci = blockIdx.x / blocks_per_cloud;
  const pb_cloud& c = A.c[ci];
  const int cell = (blockIdx.x - ci * blocks_per_cloud) * 256 + threadIdx.x;
  if (cell >= H * W) return;
  const unsigned long long key = c.key[cell];
  c.key[cell] = LT_PB_EMPTY;
  if (MODE == 1) c.dmin[cell] = LT_PB_EMPTY;
  const bool has = key != LT_PB_EMPTY;
  const T* pts = (const T*)c.pts;
  const bool want_xy = c.px_img || c.py_img || c.xf_img || c.yf_img;
  // an empty cell's pixel coordinates are those of the LAST kept point: numpy's index -1 (laserscan.py:384-388); with a beam
  // table they are 0
  int i = has ? pb_key_index(key) : ((!BEAMS && want_xy && have_prefix) ? c.meta[1] : -1);
  T x = (T)0, y = (T)0, z = (T)0;
  proj_out<T> o;
  o.depth = (T)0; o.xf = (T)0; o.yf = (T)0; o.px = 0; o.py = 0; o.cell = -1;
  if (i >= 0) {
    x = pts[3 * (size_t)i]; y = pts[3 * (size_t)i + 1]; z = pts[3 * (size_t)i + 2];
    if (has ? (want_xy || c.range_img) : true)
      o = project_model<T, BEAMS, SECTOR, AZ>(x, y, z, pi_t, abs_fov_down, fov, H, W, beams, n_beams, drop_zero, drop_outside);
  }
  int k = -1;
  if (has && have_prefix) k = c.wprefix[i >> 6] + __popcll(c.keep[i >> 6] & ((1ull << (i & 63)) - 1ull));
  if (c.idx_img) c.idx_img[cell] = has ? k : -1;
  if (c.range_img) c.range_img[cell] = has ? (float)o.depth : range_init;
  if (c.xyz_img) {
    c.xyz_img[3 * (size_t)cell] = has ? (float)x : xyz_init;
    c.xyz_img[3 * (size_t)cell + 1] = has ? (float)y : xyz_init;
    c.xyz_img[3 * (size_t)cell + 2] = has ? (float)z : xyz_init;
  }
  if (c.rem_img) c.rem_img[cell] = (has && c.rem) ? c.rem[i] : rem_init;
  const unsigned lab = (has && c.label) ? c.label[i] : 0u;
  if (c.label_img) c.label_img[cell] = (int)lab;
  // the colour image `integrate` is handed, already folded (laserscan.py:893-895: the label in channel 0;
  // fusion_lidar.py:260-264: float32, floor(c0 * 256 * 256 + c1 * 256 + c2))
  if (c.fold_img) c.fold_img[cell] = floorf((float)lab * 256.0f * 256.0f);
  if (c.color_img) {
    const bool ok = has && lut && lab < (unsigned)lut_len;
    c.color_img[3 * (size_t)cell] = ok ? lut[3 * (size_t)lab] : 0.f;
    c.color_img[3 * (size_t)cell + 1] = ok ? lut[3 * (size_t)lab + 1] : 0.f;
    c.color_img[3 * (size_t)cell + 2] = ok ? lut[3 * (size_t)lab + 2] : 0.f;
  }
  if (c.mask_img) c.mask_img[cell] = (has && k > 0) ? 1.f : 0.f;  // proj_idx > 0 (sic, laserscan.py:292)
  if (c.px_img) c.px_img[cell] = o.px;
  if (c.py_img) c.py_img[cell] = o.py;
  if (c.xf_img) ((T*)c.xf_img)[cell] = o.xf;
  if (c.yf_img) ((T*)c.yf_img)[cell] = o.yf;
}

// The per-point outputs of lt_range_projection_dev, each [n_kept] rows or NULL.  The kernel's own argument: pb_args is the
// hot path's (every scan of a sequence) and stays as small as it is.
template <typename T>
struct pb_kept { T* pts; float* rem; unsigned* label; T* depth; int* px; int* py; T* xf; T* yf; };

// One cloud's kept points, compacted in input order (laserscan.py:265-281: points, remissions, labels, depth, proj_x / proj_y
// and their float forms after remove_points), a thread per input point, after k_pb_prefix.  Kept point i goes to row
// k = kept points before its wave + kept points before it in its wave (k_pb_resolve's numbering); its depth and pixel are
// computed again from the point itself, like the winner's in k_pb_resolve.  Rows at and beyond n_kept are not written.
template <typename T, int BEAMS, int SECTOR, int AZ>
__global__ __launch_bounds__(256) void k_pb_compact(const T* __restrict__ pts, const float* __restrict__ rem,
                                                    const unsigned* __restrict__ label, int n,
                                                    const unsigned long long* __restrict__ keep, const int* __restrict__ wprefix,
                                                    pb_kept<T> out, T pi_t, T abs_fov_down, T fov, int H, int W,
                                                    const double* __restrict__ beams, int n_beams, int drop_zero,
                                                    int drop_outside) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long m = keep[i >> 6];
  if (!((m >> (i & 63)) & 1ull)) return;
  const int k = wprefix[i >> 6] + __popcll(m & ((1ull << (i & 63)) - 1ull));
  const T x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  if (out.pts) {
    out.pts[3 * (size_t)k] = x;
    out.pts[3 * (size_t)k + 1] = y;
    out.pts[3 * (size_t)k + 2] = z;
  }
  if (out.rem && rem) out.rem[k] = rem[i];
  if (out.label && label) out.label[k] = label[i];
  if (out.depth || out.px || out.py || out.xf || out.yf) {
    const proj_out<T> o = project_model<T, BEAMS, SECTOR, AZ>(x, y, z, pi_t, abs_fov_down, fov, H, W, beams, n_beams,
                                                              drop_zero, drop_outside);
    if (out.depth) out.depth[k] = o.depth;
    if (out.px) out.px[k] = o.cell % W;
    if (out.py) out.py[k] = o.cell / W;
    if (out.xf) out.xf[k] = o.xf;
    if (out.yf) out.yf[k] = o.yf;
  }
}

struct lt_projector {
  int device = 0;
  size_t cap_n = 0, cap_cells = 0;          // per cloud slot
  bool armed = false, dmin_armed = false;
  unsigned long long* key[LT_PB_MAX] = {};
  unsigned long long* dmin[LT_PB_MAX] = {};
  unsigned long long* keep[LT_PB_MAX] = {};
  int* wprefix[LT_PB_MAX] = {};
  int* meta = nullptr;                      // [LT_PB_MAX][2]
  double* beams = nullptr;                  // [LT_MODEL_DOUBLES]
  double beams_host[LT_MODEL_DOUBLES];
  int n_beams_cached = -1;
  double sector[2] = {0.0, 0.0};            // lt_projector_set_sector
  bool sector_set = false;
  double az[511];                           // lt_projector_set_beam_azimuth
  int az_n = 0;
  unsigned long long* bacc = nullptr;       // [LT_PB_MAX][bacc_blocks][6] per-workgroup partial bounds of the clouds (no arming: every
  size_t bacc_blocks = 0;                   // workgroup of k_pb_project writes its six words)
  float* img = nullptr;                     // lt_deform_scan_dev: [n][3][H * W] source images (range, remission, folded label)
  size_t img_cap = 0;                       // floats
  double* mm_bnds = nullptr;                // lt_mergemesh_scan_dev: [6] the kept points' bounds of the scan
  std::mutex mu;
};

namespace {
void pj_free(lt_projector* p) {
  for (int k = 0; k < LT_PB_MAX; ++k) {
    void* ps[] = {p->key[k], p->dmin[k], p->keep[k], p->wprefix[k]};
    for (void* q : ps)
      if (q) (void)hipFree(q);
    p->key[k] = p->dmin[k] = p->keep[k] = nullptr;
    p->wprefix[k] = nullptr;
  }
  p->cap_n = p->cap_cells = 0;
  p->armed = p->dmin_armed = false;
}

int pj_reserve(lt_projector* p, size_t n_max, size_t cells, bool need_dmin, hipStream_t st) {
  if (n_max > p->cap_n || cells > p->cap_cells) {
    // one group under two capacities (cap_n is the group's own, cap_cells follows it); dmin is dropped with the rest and
    // comes back below, when a call asks for it
    const size_t cn = std::max(p->cap_n, lt_headroom(n_max)), cc = std::max(p->cap_cells, cells + 1024);
    lt_dev_array slots[4 * LT_PB_MAX];
    for (int k = 0; k < LT_PB_MAX; ++k) {
      slots[4 * k] = {(void**)&p->key[k], cc * sizeof(unsigned long long)};
      slots[4 * k + 1] = {(void**)&p->keep[k], (cn / 64 + 2) * sizeof(unsigned long long)};
      slots[4 * k + 2] = {(void**)&p->wprefix[k], (cn / 64 + 2) * sizeof(int)};
      slots[4 * k + 3] = {(void**)&p->dmin[k], 0};
    }
    p->cap_cells = 0;
    p->armed = p->dmin_armed = false;
    LT_CHECK(lt_dev_replace("lt_range_projection_batch_dev", lt_wait_stream(st), &p->cap_n, cn, slots));
    p->cap_cells = cc;
  }
  if (need_dmin && !p->dmin[0]) {
    lt_dev_array dmin[LT_PB_MAX];
    for (int k = 0; k < LT_PB_MAX; ++k) dmin[k] = {(void**)&p->dmin[k], p->cap_cells * sizeof(unsigned long long)};
    LT_CHECK(lt_dev_replace("lt_range_projection_batch_dev", lt_wait_none(), dmin));
    p->dmin_armed = false;
  }
  if (!p->armed)
    for (int k = 0; k < LT_PB_MAX; ++k)
      LT_HIP(hipMemsetAsync(p->key[k], 0xFF, p->cap_cells * sizeof(unsigned long long), st));
  if (need_dmin && !p->dmin_armed)
    for (int k = 0; k < LT_PB_MAX; ++k)
      LT_HIP(hipMemsetAsync(p->dmin[k], 0xFF, p->cap_cells * sizeof(unsigned long long), st));
  return LT_OK;
}

// The sensor model of one call, checked: what the kernels are handed of it and the doubles they read from the projector's
// `beams` (model_table).  An entry point makes it ONCE, before it allocates or launches anything.  Laser parameters exactly
// as laserscan.py:207-209 (python floats; rounded once to the array dtype at the launch).  The rows, the sector and the
// offsets go with LT_PROJ_NEW | LT_PROJ_REMOVE only (model_table): both drops, and never MODE 1.
struct pj_model {
  int H, W, n_beams;
  double abs_fov_down, fov;
  int drop_zero, drop_outside;
  bool is_new, rows, sector, azimuth;  // LT_PROJ_NEW, _BEAM_ROWS, _SECTOR, _BEAM_AZIMUTH
  int n_tab;                    // doubles of `tab` in use (0: none)
  double tab[LT_MODEL_DOUBLES];
};

// false: the arguments do not fit the flags (the message is set).  `sec`, `az`, `n_az`: model_table
bool pj_model_of(const char* who, const double* beam_angles, int n_beams, unsigned flags, double fov_up_deg,
                 double fov_down_deg, int H, int W, const double* sec, const double* az, int n_az, pj_model& m) {
  m.n_tab = model_table(who, beam_angles, n_beams, flags, fov_up_deg, fov_down_deg, H, sec, az, n_az, m.tab);
  if (m.n_tab < 0) return false;
  const double fu = fov_up_deg / 180.0 * M_PI, fd = fov_down_deg / 180.0 * M_PI;
  m.H = H; m.W = W; m.n_beams = n_beams;
  m.abs_fov_down = fabs(fd);
  m.fov = fabs(fd) + fabs(fu);
  m.drop_zero = (flags & (LT_PROJ_REMOVE | LT_PROJ_NEW)) ? 1 : 0;
  m.drop_outside = (flags & LT_PROJ_REMOVE) ? 1 : 0;
  m.is_new = (flags & LT_PROJ_NEW) != 0;
  m.rows = (flags & LT_PROJ_BEAM_ROWS) != 0;
  m.sector = (flags & LT_PROJ_SECTOR) != 0;
  m.azimuth = (flags & LT_PROJ_BEAM_AZIMUTH) != 0;
  return true;
}

// The sensor-model arguments of every kernel that calls project_model, in their order; for pj_run and pj_compact alone
// (undefined behind them), it reads their `m` (the pj_model) and `p` (the projector).
#define LT_PB_MODEL_ARGS(T) \
  (T)M_PI, (T)m.abs_fov_down, (T)m.fov, m.H, m.W, (const double*)p->beams, m.n_beams, m.drop_zero, m.drop_outside

template <typename T>
int pj_run(lt_projector* p, pb_args& A, int total_blocks, bool old_f64, bool need_prefix, bool bnds_only, const pj_model& m,
           const float* lut, int lut_len, float range_init, float rem_init, float xyz_init, hipStream_t st) {
  const int cells = m.H * m.W, bpc = (cells + 255) / 256;
  // MODE 1 (old_f64) has neither rows nor a sector; the other instantiations are MODE 0
#define LT_PB_PROJECT(MODE, B, S, AZ)                                                                                      \
  hipLaunchKernelGGL((k_pb_project<T, MODE, B, S, AZ>), dim3(total_blocks), dim3(256), 0, st, A, LT_PB_MODEL_ARGS(T))
#define LT_PB_RESOLVE(MODE, B, S, AZ)                                                                                      \
  hipLaunchKernelGGL((k_pb_resolve<T, MODE, B, S, AZ>), dim3(bpc * A.n_clouds), dim3(256), 0, st, A, bpc,                  \
                     LT_PB_MODEL_ARGS(T), lut, lut_len, range_init, rem_init, xyz_init, need_prefix ? 1 : 0)
#define LT_PB_PROJECT0(B, S, AZ) LT_PB_PROJECT(0, B, S, AZ)
#define LT_PB_RESOLVE0(B, S, AZ) LT_PB_RESOLVE(0, B, S, AZ)
  if (total_blocks > 0) {
    if (old_f64) {
      LT_PB_PROJECT(1, 0, 0, 0);
      hipLaunchKernelGGL(k_pb_assign, dim3(total_blocks), dim3(256), 0, st, A, LT_PB_MODEL_ARGS(double));
    } else {
      LT_FOR_MODEL(m.rows, m.sector, m.azimuth, LT_PB_PROJECT0);
    }
  }
  if (need_prefix) hipLaunchKernelGGL(k_pb_prefix, dim3(A.n_clouds), dim3(256), 0, st, A);
  else if (bnds_only) hipLaunchKernelGGL(k_pb_bnds, dim3(A.n_clouds), dim3(64), 0, st, A);
  if (old_f64) LT_PB_RESOLVE(1, 0, 0, 0);
  else LT_FOR_MODEL(m.rows, m.sector, m.azimuth, LT_PB_RESOLVE0);
#undef LT_PB_PROJECT
#undef LT_PB_RESOLVE
#undef LT_PB_PROJECT0
#undef LT_PB_RESOLVE0
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// the kept points of slot 0's cloud, after a pj_run with the prefix (lt_range_projection_dev)
template <typename T>
int pj_compact(lt_projector* p, const lt_cloud& c, const pb_kept<T>& out, const pj_model& m, hipStream_t st) {
#define LT_PB_COMPACT(B, S, AZ)                                                                                            \
  hipLaunchKernelGGL((k_pb_compact<T, B, S, AZ>), dim3((c.n + 255) / 256), dim3(256), 0, st, (const T*)c.points, c.rem,    \
                     c.label, c.n, (const unsigned long long*)p->keep[0], (const int*)p->wprefix[0], out, LT_PB_MODEL_ARGS(T))
  LT_FOR_MODEL(m.rows, m.sector, m.azimuth, LT_PB_COMPACT);
#undef LT_PB_COMPACT
  LT_HIP(hipGetLastError());
  return LT_OK;
}
#undef LT_PB_MODEL_ARGS
}  // namespace

extern "C" int lt_projector_create(lt_projector** pj, int device) {
  if (!pj) {
    lt_set_error("lt_projector_create: NULL handle pointer");
    return LT_ERR_INVALID_ARG;
  }
  *pj = nullptr;
  int dev = device;
  if (dev < 0) LT_HIP(hipGetDevice(&dev));
  LT_HIP(hipSetDevice(dev));
  lt_projector* p = new (std::nothrow) lt_projector();
  if (!p) {
    lt_set_error("lt_projector_create: out of host memory");
    return LT_ERR_NO_MEMORY;
  }
  p->device = dev;
  if (hipMalloc((void**)&p->meta, LT_PB_MAX * 2 * sizeof(int)) != hipSuccess ||
      hipMalloc((void**)&p->beams, LT_MODEL_DOUBLES * sizeof(double)) != hipSuccess) {
    if (p->meta) (void)hipFree(p->meta);
    if (p->beams) (void)hipFree(p->beams);
    delete p;
    (void)hipGetLastError();
    lt_set_error("lt_projector_create: out of device memory");
    return LT_ERR_NO_MEMORY;
  }
  *pj = p;
  return LT_OK;
}

extern "C" int lt_projector_set_sector(lt_projector* p, double yaw_center, double span) {
  if (!p || (span != 0.0 && !sector_ok("lt_projector_set_sector", yaw_center, span))) {
    if (!p) lt_set_error("lt_projector_set_sector: NULL projector");
    return LT_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lock(p->mu);
  p->sector[0] = yaw_center;
  p->sector[1] = span;
  p->sector_set = span != 0.0;
  return LT_OK;
}

extern "C" int lt_projector_set_beam_azimuth(lt_projector* p, const double* az_rad, int H) {
  if (!p || !beam_azimuth_ok("lt_projector_set_beam_azimuth", az_rad, H)) {
    if (!p) lt_set_error("lt_projector_set_beam_azimuth: NULL projector");
    return LT_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lock(p->mu);
  p->az_n = az_rad ? H : 0;
  if (p->az_n > 0) memcpy(p->az, az_rad, (size_t)H * sizeof(double));
  return LT_OK;
}

extern "C" int lt_projector_destroy(lt_projector* p) {
  if (!p) return LT_OK;
  (void)hipSetDevice(p->device);
  (void)hipDeviceSynchronize();
  pj_free(p);
  if (p->meta) (void)hipFree(p->meta);
  if (p->beams) (void)hipFree(p->beams);
  if (p->bacc) (void)hipFree(p->bacc);
  if (p->mm_bnds) (void)hipFree(p->mm_bnds);
  if (p->img) (void)hipFree(p->img);
  delete p;
  return LT_OK;
}

// The projection of checked clouds (n >= 0, points unless n == 0) on a projector that the caller holds locked, queued on
// `st`.  `model` is the caller's, with the sector and the offsets the caller chose: a projector's own, or the process-wide
// ones of the single-cloud call -- p->sector and p->az are not read here.
static int project_clouds(lt_projector* p, const pj_model& model, int n_clouds, const lt_cloud* clouds, int is_f64,
                          const float* color_lut, int lut_len, const lt_proj_images* out, float range_init, float rem_init,
                          float xyz_init, hipStream_t st) {
  size_t n_max = 0;
  for (int k = 0; k < n_clouds; ++k) n_max = std::max(n_max, (size_t)clouds[k].n);
  const double* tab = model.tab;
  const int n_dev = model.n_tab;
  LT_HIP(hipSetDevice(p->device));
  const bool old_f64 = is_f64 && !model.is_new;
  LT_CHECK(pj_reserve(p, n_max, (size_t)model.H * model.W, old_f64, st));
  {  // the per-workgroup partial bounds of the clouds that want get_bnds()
    bool want = false;
    for (int k = 0; k < n_clouds; ++k) want = want || out[k].bnds;
    const size_t nb = n_max / 256 + 2;
    if (want && nb > p->bacc_blocks) {
      const size_t cap = nb + nb / 4 + 64;
      const lt_dev_array bacc[] = {{(void**)&p->bacc, LT_PB_MAX * cap * 6 * sizeof(unsigned long long)}};
      LT_CHECK(lt_dev_replace("lt_range_projection_batch_dev", lt_wait_stream(st), &p->bacc_blocks, cap, bacc));
    }
  }
  p->armed = false;  // (until the resolve pass of this call has been queued)
  if (old_f64) p->dmin_armed = false;
  if (n_dev > 0 && (n_dev != p->n_beams_cached || memcmp(p->beams_host, tab, n_dev * sizeof(double)) != 0)) {
    // the table is read by kernels of EARLIER calls on this stream: the copy is stream-ordered behind them; a pageable
    // source is staged by the runtime before the call returns, so beams_host may be overwritten by the next call
    memcpy(p->beams_host, tab, n_dev * sizeof(double));
    LT_HIP(hipMemcpyAsync(p->beams, p->beams_host, n_dev * sizeof(double), hipMemcpyHostToDevice, st));
    p->n_beams_cached = n_dev;
  }
  for (int g0 = 0; g0 < n_clouds; g0 += LT_PB_MAX) {
    pb_args A;
    A.n_clouds = std::min(LT_PB_MAX, n_clouds - g0);
    int blocks = 0;
    bool need_prefix = false;
    for (int k = 0; k < A.n_clouds; ++k) {
      const lt_cloud& ci = clouds[g0 + k];
      const lt_proj_images& o = out[g0 + k];
      pb_cloud& c = A.c[k];
      c.pts = ci.points; c.rem = ci.rem; c.label = ci.label; c.n = ci.n; c.block0 = blocks;
      blocks += (ci.n + 255) / 256;
      c.key = p->key[k]; c.dmin = p->dmin[k]; c.keep = p->keep[k]; c.wprefix = p->wprefix[k]; c.meta = p->meta + 2 * k;
      c.idx_img = o.idx; c.range_img = o.range; c.xyz_img = o.xyz; c.rem_img = o.rem; c.label_img = o.label;
      c.color_img = o.color; c.mask_img = o.mask; c.fold_img = o.label_folded; c.px_img = o.proj_x; c.py_img = o.proj_y;
      c.xf_img = o.proj_xf; c.yf_img = o.proj_yf; c.n_kept = o.n_kept;
      c.bacc = o.bnds ? p->bacc + 6 * p->bacc_blocks * k : nullptr; c.bnds_out = o.bnds;
      need_prefix = need_prefix || o.idx || o.mask || o.proj_x || o.proj_y || o.proj_xf || o.proj_yf || o.n_kept;
    }
    for (int k = A.n_clouds; k < LT_PB_MAX; ++k) { A.c[k] = A.c[0]; A.c[k].n = 0; A.c[k].block0 = 0x7fffffff; }
    bool wants_bnds = false;
    for (int k = 0; k < A.n_clouds; ++k) wants_bnds = wants_bnds || A.c[k].bacc;
    const int rc = is_f64 ? pj_run<double>(p, A, blocks, old_f64, need_prefix, wants_bnds, model, color_lut, lut_len,
                                           range_init, rem_init, xyz_init, st)
                          : pj_run<float>(p, A, blocks, false, need_prefix, wants_bnds, model, color_lut, lut_len,
                                          range_init, rem_init, xyz_init, st);
    if (rc != LT_OK) return rc;
  }
  p->armed = true;  // k_pb_resolve re-armed every cell it looked at
  if (old_f64) p->dmin_armed = true;
  return LT_OK;
}

extern "C" int lt_range_projection_batch_dev(lt_projector* p, int n_clouds, const lt_cloud* clouds, int is_f64,
                                             double fov_up, double fov_down, int H, int W, const double* beam_angles,
                                             int n_beams, unsigned flags, const float* color_lut, int lut_len,
                                             const lt_proj_images* out, float range_init, float rem_init, float xyz_init,
                                             void* stream) {
  if (!p || n_clouds < 0 || (n_clouds > 0 && (!clouds || !out)) || H <= 0 || W <= 0 || n_beams < 0 || n_beams > 1024 ||
      (n_beams > 0 && !beam_angles)) {
    lt_set_error("lt_range_projection_batch_dev: invalid argument (n_clouds=%d H=%d W=%d n_beams=%d)", n_clouds, H, W, n_beams);
    return LT_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n_clouds; ++k)
    if (clouds[k].n < 0 || (clouds[k].n > 0 && !clouds[k].points)) {
      lt_set_error("lt_range_projection_batch_dev: cloud %d: n=%d points=%p", k, clouds[k].n, clouds[k].points);
      return LT_ERR_INVALID_ARG;
    }
  std::lock_guard<std::mutex> lock(p->mu);
  pj_model model;
  if (!pj_model_of("lt_range_projection_batch_dev", beam_angles, n_beams, flags, fov_up, fov_down, H, W,
                   p->sector_set ? p->sector : nullptr, p->az_n > 0 ? p->az : nullptr, p->az_n, model))
    return LT_ERR_INVALID_ARG;
  return project_clouds(p, model, n_clouds, clouds, is_f64, color_lut, lut_len, out, range_init, rem_init, xyz_init,
                        (hipStream_t)stream);
}

// ---- one cloud, with its kept points compacted and their number on the host (lt_range_projection_dev) -----------------
namespace {
std::mutex g_pmu;
lt_projector* g_pj = nullptr;     // the workspace of lt_range_projection_dev, on the device of its last call
double g_sector[2] = {0.0, 0.0};  // lt_range_projection_set_sector
bool g_sector_set = false;
double g_az[511];                 // lt_range_projection_set_beam_azimuth
int g_az_n = 0;
}  // namespace

extern "C" int lt_range_projection_set_sector(double yaw_center, double span) {
  if (span != 0.0 && !sector_ok("lt_range_projection_set_sector", yaw_center, span)) return LT_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(g_pmu);
  g_sector[0] = yaw_center;
  g_sector[1] = span;
  g_sector_set = span != 0.0;
  return LT_OK;
}

extern "C" int lt_range_projection_set_beam_azimuth(const double* az_rad, int H) {
  if (!beam_azimuth_ok("lt_range_projection_set_beam_azimuth", az_rad, H)) return LT_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(g_pmu);
  g_az_n = az_rad ? H : 0;
  if (g_az_n > 0) memcpy(g_az, az_rad, (size_t)H * sizeof(double));
  return LT_OK;
}

// The batch's kernels for one cloud on a hidden, process-wide projector (g_pj; g_pmu stands in for its mutex), then
// k_pb_compact.  g_pmu is held for the WHOLE call, the final wait for the stream included: the projector is shared by every
// thread of the process, whatever stream each one passes, and a thread that has to regrow it (pj_reserve, which waits for
// its own stream only) may free the buffers only because no other thread's kernels can still be in flight on them.
extern "C" int lt_range_projection_dev(const void* points, int is_f64, const float* rem, const unsigned* label,
                                       int n, double fov_up, double fov_down, int H, int W,
                                       const double* beam_angles, int n_beams, unsigned flags,
                                       const float* color_lut, int lut_len, void* points_kept, float* rem_kept,
                                       unsigned* label_kept, void* depth_kept, int* proj_x_kept, int* proj_y_kept,
                                       void* proj_xf_kept, void* proj_yf_kept, int* idx_img, float* range_img,
                                       float* xyz_img, float* rem_img, int* label_img, float* color_img,
                                       float* mask_img, float range_init, float rem_init, float xyz_init,
                                       int* n_kept, void* stream) {
  if (n < 0 || H <= 0 || W <= 0 || (n > 0 && !points) || n_beams < 0 || n_beams > 1024 ||
      (n_beams > 0 && !beam_angles)) {
    lt_set_error("lt_range_projection: invalid argument (n=%d H=%d W=%d n_beams=%d)", n, H, W, n_beams);
    return LT_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lock(g_pmu);
  pj_model model;  // (the flags and the table are checked before anything is allocated)
  if (!pj_model_of("lt_range_projection", beam_angles, n_beams, flags, fov_up, fov_down, H, W,
                   g_sector_set ? g_sector : nullptr, g_az_n > 0 ? g_az : nullptr, g_az_n, model))
    return LT_ERR_INVALID_ARG;
  int dev = 0;
  LT_HIP(hipGetDevice(&dev));
  if (g_pj && g_pj->device != dev) {  // (destroy waits for the old device and leaves it current; create makes `dev` current again)
    (void)lt_projector_destroy(g_pj);
    g_pj = nullptr;
  }
  if (!g_pj) LT_CHECK(lt_projector_create(&g_pj, dev));
  lt_projector* p = g_pj;
  hipStream_t st = (hipStream_t)stream;
  lt_cloud cloud;
  cloud.points = points; cloud.rem = rem; cloud.label = label; cloud.n = n;
  lt_proj_images img;
  memset(&img, 0, sizeof(img));
  img.idx = idx_img; img.range = range_img; img.xyz = xyz_img; img.rem = rem_img; img.label = label_img;
  img.color = color_img; img.mask = mask_img;
  img.n_kept = p->meta;  // always: the number of kept points goes where k_pb_prefix leaves it anyway, and asking for it asks
                         // for the prefix, which the compaction and the host's n_kept need whatever images are wanted
  LT_CHECK(project_clouds(p, model, 1, &cloud, is_f64, color_lut, lut_len, &img, range_init, rem_init, xyz_init, st));
  if (n > 0 && (points_kept || rem_kept || label_kept || depth_kept || proj_x_kept || proj_y_kept || proj_xf_kept ||
                proj_yf_kept)) {
    if (is_f64) {
      const pb_kept<double> out = {(double*)points_kept, rem_kept, label_kept, (double*)depth_kept, proj_x_kept, proj_y_kept,
                                   (double*)proj_xf_kept, (double*)proj_yf_kept};
      LT_CHECK(pj_compact<double>(p, cloud, out, model, st));
    } else {
      const pb_kept<float> out = {(float*)points_kept, rem_kept, label_kept, (float*)depth_kept, proj_x_kept, proj_y_kept,
                                  (float*)proj_xf_kept, (float*)proj_yf_kept};
      LT_CHECK(pj_compact<float>(p, cloud, out, model, st));
    }
  }
  int kept = 0;
  LT_HIP(hipMemcpyAsync(&kept, p->meta, sizeof(int), hipMemcpyDeviceToHost, st));
  LT_HIP(hipStreamSynchronize(st));
  if (n_kept) *n_kept = kept;
  return LT_OK;
}

// One output scan of the `mesh` adaption FROM POINT CLOUDS in one call (see include/lidarhip.h): projection of the source
// scans into images the projector owns, then lt_fusion_scan_dev on them.  One native call per output scan keeps a host
// thread's share at a few microseconds -- from Python the interpreter lock is released for all of it.
extern "C" int lt_deform_scan_dev(lt_projector* p, lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene, lt_rayset* rayset,
                                  int n_clouds, const lt_cloud* clouds, int is_f64, double fov_up, double fov_down, int H,
                                  int W, const double* beam_angles, int n_beams, float obs_weight, unsigned tsdf_flags,
                                  const float* origin, float* endpoints, int* endcolors, float* range, float* endrem,
                                  int* tri, unsigned trace_flags, void* stream, int sync) {
  if (!p || n_clouds < 0 || n_clouds > 64 || H <= 0 || W <= 0) {
    lt_set_error("lt_deform_scan_dev: invalid argument (n_clouds=%d H=%d W=%d)", n_clouds, H, W);
    return LT_ERR_INVALID_ARG;
  }
  const size_t cells = (size_t)H * W, need = (size_t)(n_clouds > 0 ? n_clouds : 1) * 3 * cells;
  {
    std::lock_guard<std::mutex> lock(p->mu);
    LT_HIP(hipSetDevice(p->device));
    LT_CHECK(lt_dev_grow("lt_deform_scan_dev", lt_wait_stream((hipStream_t)stream), &p->img, &p->img_cap, need, need));
  }
  lt_proj_images out[64];
  const float* color_ims[64];
  const float* depth_ims[64];
  const float* rem_ims[64];
  memset(out, 0, sizeof(out));
  for (int k = 0; k < n_clouds; ++k) {
    float* base = p->img + (size_t)k * 3 * cells;
    out[k].range = base; out[k].rem = base + cells; out[k].label_folded = base + 2 * cells;
    depth_ims[k] = base; rem_ims[k] = base + cells; color_ims[k] = base + 2 * cells;
  }
  // do_range_projection_new(fov, remove=True) + do_label_projection_new per source scan (laserscan.py:874-881)
  LT_CHECK(lt_range_projection_batch_dev(p, n_clouds, clouds, is_f64, fov_up, fov_down, H, W, beam_angles, n_beams,
                                         LT_PROJ_NEW | LT_PROJ_REMOVE, nullptr, 0, out, 0.0f, -1.0f, 0.0f, stream));
  return lt_fusion_scan_dev(vol, mesh, scene, rayset, n_clouds, color_ims, depth_ims, rem_ims, H, W, obs_weight, tsdf_flags,
                            origin, endpoints, endcolors, range, endrem, tri, trace_flags, stream, sync);
}

// deform('mergemesh') of one output scan in one call (see include/lidarhip.h)
extern "C" int lt_mergemesh_scan_dev(lt_projector* p, lt_mm_state* mm, int seq, lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene,
                                     lt_rayset* rayset, const lt_cloud* cloud, int is_f64, double fov_up, double fov_down,
                                     int H, int W, const double* beam_angles, int n_beams, float obs_weight,
                                     unsigned tsdf_flags, const float* origin, float* endpoints, int* endcolors, float* range,
                                     float* endrem, int* tri, unsigned trace_flags, void* stream, lt_mm_geometry* geo,
                                     int* done) {
  int ticket = -1;
  auto fail = [&](int rc) {  // the scans behind this one must not wait for a turn that will not come
    if (mm && seq >= 0 && ticket < 0) (void)lt_mm_geometry_dev(mm, nullptr, seq, &ticket, stream);
    return rc;
  };
  if (!p || !mm || !mesh || !scene || !rayset || !cloud || !geo || !done || H <= 0 || W <= 0) {
    lt_set_error("lt_mergemesh_scan_dev: invalid argument");
    return fail(LT_ERR_INVALID_ARG);
  }
  *done = 0;
  const size_t cells = (size_t)H * W;
  {
    std::lock_guard<std::mutex> lock(p->mu);
    if (hipSetDevice(p->device) != hipSuccess) return fail(LT_ERR_HIP);
    const int rc_img = lt_dev_grow("lt_mergemesh_scan_dev", lt_wait_stream((hipStream_t)stream), &p->img, &p->img_cap, 3 * cells,
                                   3 * cells);
    if (rc_img != LT_OK) return fail(rc_img);
    if (!p->mm_bnds && hipMalloc((void**)&p->mm_bnds, 6 * sizeof(double)) != hipSuccess) {
      lt_set_error("lt_mergemesh_scan_dev: hipMalloc failed");
      return fail(LT_ERR_NO_MEMORY);
    }
  }
  lt_proj_images out;
  memset(&out, 0, sizeof(out));
  out.range = p->img; out.rem = p->img + cells; out.label_folded = p->img + 2 * cells; out.bnds = p->mm_bnds;
  int rc = lt_range_projection_batch_dev(p, 1, cloud, is_f64, fov_up, fov_down, H, W, beam_angles, n_beams,
                                         LT_PROJ_NEW | LT_PROJ_REMOVE, nullptr, 0, &out, 0.0f, -1.0f, 0.0f, stream);
  if (rc != LT_OK) return fail(rc);
  rc = lt_mm_geometry_dev(mm, p->mm_bnds, seq, &ticket, stream);
  if (rc != LT_OK) return rc;
  if (vol) {  // the chain on the expected geometry; it waits for the stream once (the mesh sizes): the record is in by then
    LT_CHECK(lt_mergemesh_rerun_dev(p, vol, mesh, scene, rayset, H, W, obs_weight, tsdf_flags, origin, endpoints, endcolors, range,
                                    endrem, tri, trace_flags, stream));
  }
  LT_CHECK(lt_mm_geometry_get(mm, ticket, geo));
  *done = (vol && geo->status == 0 && memcmp(vol->bnds_given, geo->bnds_given, sizeof(geo->bnds_given)) == 0) ? 1 : 0;
  return LT_OK;
}

extern "C" int lt_mergemesh_rerun_dev(lt_projector* p, lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene, lt_rayset* rayset, int H, int W,
                                      float obs_weight, unsigned tsdf_flags, const float* origin, float* endpoints, int* endcolors,
                                      float* range, float* endrem, int* tri, unsigned trace_flags, void* stream) {
  if (!p || !vol || H <= 0 || W <= 0 || !p->img || p->img_cap < 3 * (size_t)H * W) {
    lt_set_error("lt_mergemesh_rerun_dev: invalid argument (no projected scan of this shape)");
    return LT_ERR_INVALID_ARG;
  }
  const size_t cells = (size_t)H * W;
  const float* depth_im = p->img;
  const float* rem_im = p->img + cells;
  const float* color_im = p->img + 2 * cells;
  return lt_fusion_scan_dev(vol, mesh, scene, rayset, 1, &color_im, &depth_im, &rem_im, H, W, obs_weight, tsdf_flags, origin,
                            endpoints, endcolors, range, endrem, tri, trace_flags, stream, 0);
}

// Host-pointer convenience: stages everything through device buffers, same semantics.
extern "C" int lt_range_projection(const void* points, int is_f64, const float* rem, const unsigned* label, int n,
                                   double fov_up, double fov_down, int H, int W, const double* beam_angles,
                                   int n_beams, unsigned flags, const float* color_lut, int lut_len,
                                   void* points_kept, float* rem_kept, unsigned* label_kept, void* depth_kept,
                                   int* proj_x_kept, int* proj_y_kept, void* proj_xf_kept, void* proj_yf_kept,
                                   int* idx_img, float* range_img, float* xyz_img, float* rem_img, int* label_img,
                                   float* color_img, float* mask_img, float range_init, float rem_init,
                                   float xyz_init, int* n_kept) {
  if (n < 0 || H <= 0 || W <= 0 || (n > 0 && !points)) {
    lt_set_error("lt_range_projection: invalid argument (n=%d H=%d W=%d)", n, H, W);
    return LT_ERR_INVALID_ARG;
  }
  const size_t es = is_f64 ? 8 : 4, cells = (size_t)H * W, N = (size_t)n;
  // one staging allocation: inputs | per-point outputs | images
  const lt_rp_layout L = lt_rp_layout_of(N, es, (size_t)(lut_len > 0 ? lut_len : 0), cells);
  char* base = nullptr;
  LT_HIP(hipMalloc((void**)&base, L.total));
  char* p[LT_RP_ARRAYS];
  for (int k = 0; k < LT_RP_ARRAYS; ++k) p[k] = base + L.at[k];
  int rc = LT_OK;
  auto H2D = [&](void* d, const void* h, size_t b) {
    if (rc == LT_OK && h && b && hipMemcpy(d, h, b, hipMemcpyHostToDevice) != hipSuccess) {
      lt_set_error("lt_range_projection: H2D copy failed");
      rc = LT_ERR_HIP;
    }
  };
  H2D(p[0], points, N * 3 * es);
  H2D(p[1], rem, N * 4);
  H2D(p[2], label, N * 4);
  H2D(p[3], color_lut, (size_t)(lut_len > 0 ? lut_len : 0) * 12);
  int kept = 0;
  if (rc == LT_OK)
    rc = lt_range_projection_dev(p[0], is_f64, rem ? (float*)p[1] : nullptr, label ? (unsigned*)p[2] : nullptr, n,
                                 fov_up, fov_down, H, W, beam_angles, n_beams, flags,
                                 (color_lut && lut_len > 0) ? (float*)p[3] : nullptr, lut_len,
                                 points_kept ? p[4] : nullptr, rem_kept ? (float*)p[5] : nullptr,
                                 label_kept ? (unsigned*)p[6] : nullptr, depth_kept ? p[7] : nullptr,
                                 proj_x_kept ? (int*)p[8] : nullptr, proj_y_kept ? (int*)p[9] : nullptr,
                                 proj_xf_kept ? p[10] : nullptr, proj_yf_kept ? p[11] : nullptr,
                                 idx_img ? (int*)p[12] : nullptr, range_img ? (float*)p[13] : nullptr,
                                 xyz_img ? (float*)p[14] : nullptr, rem_img ? (float*)p[15] : nullptr,
                                 label_img ? (int*)p[16] : nullptr, color_img ? (float*)p[17] : nullptr,
                                 mask_img ? (float*)p[18] : nullptr, range_init, rem_init, xyz_init, &kept, nullptr);
  auto D2H = [&](void* h, const void* d, size_t b) {
    if (rc == LT_OK && h && b && hipMemcpy(h, d, b, hipMemcpyDeviceToHost) != hipSuccess) {
      lt_set_error("lt_range_projection: D2H copy failed");
      rc = LT_ERR_HIP;
    }
  };
  const size_t K = (size_t)kept;
  D2H(points_kept, p[4], K * 3 * es);
  D2H(rem_kept, p[5], K * 4);
  D2H(label_kept, p[6], K * 4);
  D2H(depth_kept, p[7], K * es);
  D2H(proj_x_kept, p[8], K * 4);
  D2H(proj_y_kept, p[9], K * 4);
  D2H(proj_xf_kept, p[10], K * es);
  D2H(proj_yf_kept, p[11], K * es);
  D2H(idx_img, p[12], cells * 4);
  D2H(range_img, p[13], cells * 4);
  D2H(xyz_img, p[14], cells * 12);
  D2H(rem_img, p[15], cells * 4);
  D2H(label_img, p[16], cells * 4);
  D2H(color_img, p[17], cells * 12);
  D2H(mask_img, p[18], cells * 4);
  (void)hipFree(base);
  if (n_kept) *n_kept = kept;
  return rc;
}
