// lt_projpoint.h -- the per-point arithmetic of the spherical projection and the z-min key of its single-key variants: ONE
// definition for every kernel that projects points (lt_project.hip: the single-cloud and the batched projection;
// lt_evaluate.hip: the source reference scan straight from the raw file bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

template <typename T>
struct proj_out {
  int cell;   // py * W + px, or -1 when the point is dropped
  T depth, xf, yf;
  int px, py;
};

__device__ __forceinline__ float lt_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ __forceinline__ double lt_atan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float lt_asin(float q) { return (float)asin((double)q); }
__device__ __forceinline__ double lt_asin(double q) { return asin(q); }
__device__ __forceinline__ float lt_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double lt_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float lt_floor(float v) { return floorf(v); }
__device__ __forceinline__ double lt_floor(double v) { return floor(v); }

// one point through laserscan.py:214-262 (resp. :304-351); all constants pre-rounded to T by the host
template <typename T>
__device__ __forceinline__ proj_out<T> project_point(T x, T y, T z, T pi_t, T abs_fov_down, T fov, int H, int W,
                                                     const double* __restrict__ beams, int n_beams,
                                                     bool drop_zero, bool drop_outside) {
  proj_out<T> o;
  const T depth = lt_sqrt((x * x + y * y) + z * z);  // np.linalg.norm(points, 2, axis=1)
  T yaw = -lt_atan2(y, x);
  T pitch = lt_asin(z / depth);
  if (n_beams > 0) {  // nearest hard-coded beam angle, first minimum (laserscan.py:233-238)
    double best = fabs((double)pitch - beams[0]);
    int bi = 0;
    for (int k = 1; k < n_beams; ++k) {
      const double dlt = fabs((double)pitch - beams[k]);
      if (dlt < best) { best = dlt; bi = k; }
    }
    pitch = (T)beams[bi];
  }
  T px = (T)0.5 * (yaw / pi_t + (T)1.0);
  T py = (T)1.0 - (pitch + abs_fov_down) / fov;
  bool keep = true;
  if (drop_zero && depth == (T)0) keep = false;
  if (drop_outside && !(py >= (T)0 && py <= (T)1)) keep = false;
  if (!(depth == depth) || !(px == px) || !(py == py)) keep = false;  // NaN never reaches an image
  px *= (T)W;
  py *= (T)H;
  o.xf = px;
  o.yf = py;
  T fx = lt_floor(px), fy = lt_floor(py);
  fx = fx < (T)(W - 1) ? fx : (T)(W - 1);
  fx = fx > (T)0 ? fx : (T)0;
  fy = fy < (T)(H - 1) ? fy : (T)(H - 1);
  fy = fy > (T)0 ? fy : (T)0;
  o.px = (int)fx;
  o.py = (int)fy;
  o.depth = depth;
  o.cell = keep ? o.py * W + o.px : -1;
  return o;
}

// The pitch of a float64 point under LT_PROJ_BEAM_ROWS: asin correctly rounded (but for arguments within ~2^-49 ulp of a
// rounding boundary), so that proj_yf is ONE value whatever math library a host or a device has -- two float64 asin
// implementations differ in the last place in one argument of ten, and a row's pitch image is an output.  One Newton step
// from the library's asin: y = y0 + (x - sin(y0)) / cos(y0), sin(y0) from its Taylor series in double-double arithmetic
// (error-free sums and fma products; the build has -ffp-contract=off and no fast-math, so they stay as written); the
// residual is a few ulp of y0 at most, so the quotient in plain double is exact enough.  |x| > 0.99 (beyond +-81 degrees,
// where the derivative grows without bound) and non-finite arguments keep the library's value.
struct lt_dd { double hi, lo; };
__host__ __device__ __forceinline__ lt_dd lt_dd_sum(double a, double b) {  // a + b exactly
  const double s = a + b, bb = s - a;
  return lt_dd{s, (a - (s - bb)) + (b - bb)};
}
__host__ __device__ __forceinline__ lt_dd lt_dd_add(lt_dd a, lt_dd b) {
  lt_dd s = lt_dd_sum(a.hi, b.hi);
  s.lo += a.lo + b.lo;
  return lt_dd_sum(s.hi, s.lo);
}
__host__ __device__ __forceinline__ lt_dd lt_dd_mul(lt_dd a, lt_dd b) {
  const double p = a.hi * b.hi;
  const double e = fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
  return lt_dd_sum(p, e);
}
__host__ __device__ __forceinline__ double lt_asin_cr(double x, double y0) {  // y0: the library's asin(x)
  if (!(fabs(x) <= 0.99)) return y0;
  // (-1)^k / (2k + 1)!, k = 1 .. 15, as double-double
  const lt_dd c[15] = {{-0.16666666666666666, -9.25185853854297e-18}, {0.008333333333333333, 1.1564823173178714e-19},
                       {-0.0001984126984126984, -1.7209558293420705e-22}, {2.7557319223985893e-06, -1.858393274046472e-22},
                       {-2.505210838544172e-08, 1.448814070935912e-24}, {1.6059043836821613e-10, 1.2585294588752098e-26},
                       {-7.647163731819816e-13, -7.03872877733453e-30}, {2.8114572543455206e-15, 1.6508842730861433e-31},
                       {-8.22063524662433e-18, -2.2141894119604265e-34}, {1.9572941063391263e-20, -1.3643503830087908e-36},
                       {-3.868170170630684e-23, 8.843177655482344e-40}, {6.446950284384474e-26, -1.9330404233703465e-42},
                       {-9.183689863795546e-29, -1.4303150396787322e-45}, {1.1309962886447716e-31, 1.0498015412959506e-47},
                       {-1.216125041553518e-34, -5.586290567888806e-51}};
  const lt_dd y = {y0, 0.0};
  const lt_dd y2 = lt_dd_mul(y, y);
  lt_dd q = c[14];
#pragma unroll
  for (int k = 13; k >= 0; --k) q = lt_dd_add(lt_dd_mul(q, y2), c[k]);
  q = lt_dd_mul(lt_dd_mul(q, y2), y);                 // sin(y0) - y0
  const lt_dd r = lt_dd_add(lt_dd_sum(x, -y0), lt_dd{-q.hi, -q.lo});   // x - sin(y0)
  return y0 + (r.hi + r.lo) / cos(y0);
}
__device__ __forceinline__ float lt_pitch_beams(float q) { return lt_asin(q); }
__device__ __forceinline__ double lt_pitch_beams(double q) { return lt_asin_cr(q, asin(q)); }

// One point into the image of a sensor with a BEAM TABLE (LT_PROJ_BEAM_ROWS): the column as above, the row is the NEAREST
// beam.  `tab` (device, float64): Brad[H] descending, halfw[H], fov_down and fov_up in radians.  The pitch q is computed in
// T (the correctly rounded asin for both dtypes) and widened to float64; row = the first minimum of |q - Brad[k]|: a
// binary search for the first beam at or below q, then one comparison of the bracketing pair (neighbouring beams are at least 1e-6 degrees apart, so no beam
// further out can tie).  Kept iff |q - Brad[row]| <= halfw[row] -- a beam samples its own direction, not the gap beside it;
// H == 1: iff fov_down <= q <= fov_up.  depth == 0 and NaN never reach an image.  yf = q, py = row.
template <typename T>
__device__ __forceinline__ proj_out<T> project_point_beams(T x, T y, T z, T pi_t, int H, int W,
                                                           const double* __restrict__ tab) {
  proj_out<T> o;
  const T depth = lt_sqrt((x * x + y * y) + z * z);
  const T yaw = -lt_atan2(y, x);
  const T pitch = lt_pitch_beams(z / depth);  // (float32: correctly rounded already, through double)
  const double q = (double)pitch;
  int lo = 0, hi = H;  // -> the first k with Brad[k] <= q (H: none)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] > q) lo = mid + 1; else hi = mid;
  }
  int row = lo;
  if (lo >= H) row = H - 1;
  else if (lo > 0 && !(fabs(q - tab[lo]) < fabs(q - tab[lo - 1]))) row = lo - 1;
  T px = (T)0.5 * (yaw / pi_t + (T)1.0);
  bool keep = H > 1 ? fabs(q - tab[row]) <= tab[H + row] : (q >= tab[2 * H] && q <= tab[2 * H + 1]);
  if (depth == (T)0) keep = false;
  if (!(depth == depth) || !(px == px) || !(q == q)) keep = false;
  px *= (T)W;
  o.xf = px;
  o.yf = pitch;
  T fx = lt_floor(px);
  fx = fx < (T)(W - 1) ? fx : (T)(W - 1);
  fx = fx > (T)0 ? fx : (T)0;
  o.px = (int)fx;
  o.py = row;
  o.depth = depth;
  o.cell = keep ? row * W + o.px : -1;
  return o;
}

// The column of a sensor with a horizontal SECTOR (LT_PROJ_SECTOR), on top of a point projected by either function above --
// its row, depth, pitch and keep conditions stay, the full-circle column is replaced.  `sec` (device, float64): the yaw of
// the sector's middle yc = -azimuth_center and its width, both in radians; like pi they are rounded to T once.  d = yaw - yc
// is brought into [-pi, pi) by one wrap (|yc| <= pi; a sector may straddle the seam behind the sensor), u = d / span + 0.5
// is the position across the sector: kept iff 0 <= u < 1 as well, px = u * W, column = floor(px) clamped -- column w is the
// cell [w, w + 1) * span / W, whose centre is the ray of that column (lt_create_rays_sector_dev).
template <typename T>
__device__ __forceinline__ void project_sector_yaw(proj_out<T>& o, T yaw, T pi_t, int W, const double* __restrict__ sec) {
  const T yc = (T)sec[0], span_t = (T)sec[1], twopi_t = (T)2 * pi_t;
  T d = yaw - yc;
  if (d < -pi_t) d += twopi_t;
  if (d >= pi_t) d -= twopi_t;
  const T u = d / span_t + (T)0.5;
  const bool in = u >= (T)0 && u < (T)1;  // (NaN: neither)
  const T px = u * (T)W;
  o.xf = px;
  T fx = lt_floor(px);
  fx = fx < (T)(W - 1) ? fx : (T)(W - 1);
  fx = fx > (T)0 ? fx : (T)0;
  o.px = (int)fx;
  o.cell = (o.cell >= 0 && in) ? o.py * W + o.px : -1;
}
template <typename T>
__device__ __forceinline__ void project_sector_column(proj_out<T>& o, T x, T y, T pi_t, int W, const double* __restrict__ sec) {
  project_sector_yaw<T>(o, -lt_atan2(y, x), pi_t, W, sec);
}

// The column of a beam-table sensor whose beams carry AZIMUTH OFFSETS (LT_PROJ_BEAM_AZIMUTH), on top of a point projected by
// project_point_beams -- its row, depth, pitch and keep conditions stay.  `az` (device, float64 [H]): the offset of every row
// in radians, positive to the left (measured like atan2(y, x)); beam `row` of a column looks az[row] to the left of the
// column's nominal direction, so the point's NOMINAL yaw is y' = -atan2(y, x) + a with a = (T)az[row] (|a| <= pi / 2).  Returns
// y' for a sector (whose own wrap follows, project_sector_yaw); on the full circle one wrap back into [-pi, pi], only when
// strictly outside -- the reference's closed interval stays what it is -- then the column as without offsets:
// px = 0.5 (y' / pi + 1) W, floor, clamp.  xf is the nominal coordinate.
template <typename T, int SECTOR>
__device__ __forceinline__ T project_azimuth_column(proj_out<T>& o, T x, T y, T pi_t, int W, const double* __restrict__ az) {
  T yaw = -lt_atan2(y, x) + (T)az[o.py];
  if (!SECTOR) {
    const T twopi_t = (T)2 * pi_t;
    if (yaw > pi_t) yaw -= twopi_t;
    else if (yaw < -pi_t) yaw += twopi_t;
    T px = (T)0.5 * (yaw / pi_t + (T)1.0);
    px *= (T)W;
    o.xf = px;
    T fx = lt_floor(px);
    fx = fx < (T)(W - 1) ? fx : (T)(W - 1);
    fx = fx > (T)0 ? fx : (T)0;
    o.px = (int)fx;
    o.cell = o.cell >= 0 ? o.py * W + o.px : -1;  // (a NaN yaw was dropped with the plain column already)
  }
  return yaw;
}

// One point through the sensor model of a projection kernel -- the one entry point of k_pb_project, k_pb_resolve and
// k_pb_compact.  BEAMS: the rows of a beam table (project_point_beams; `tab` is then the completed table of 2 H + 2 doubles),
// else the linear rows (project_point; `tab` holds the n_beams hard-coded angles, n_beams may be 0).  AZ (with BEAMS only):
// the per-row azimuth offsets, H doubles in radians behind the completed table (project_azimuth_column).  SECTOR: the columns
// of a horizontal sector on top; its two numbers follow the table (and the offsets) or the angles in `tab` -- only this
// function knows where.
template <typename T, int BEAMS, int SECTOR, int AZ = 0>
__device__ __forceinline__ proj_out<T> project_model(T x, T y, T z, T pi_t, T abs_fov_down, T fov, int H, int W,
                                                     const double* __restrict__ tab, int n_beams, bool drop_zero,
                                                     bool drop_outside) {
  proj_out<T> o = BEAMS ? project_point_beams<T>(x, y, z, pi_t, H, W, tab)
                        : project_point<T>(x, y, z, pi_t, abs_fov_down, fov, H, W, tab, n_beams, drop_zero, drop_outside);
  if (BEAMS && AZ) {
    const T yaw = project_azimuth_column<T, SECTOR>(o, x, y, pi_t, W, tab + 2 * H + 2);
    if (SECTOR) project_sector_yaw<T>(o, yaw, pi_t, W, tab + 3 * H + 2);
    return o;
  }
  if (SECTOR) project_sector_column<T>(o, x, y, pi_t, W, tab + (BEAMS ? 2 * H + 2 : n_beams));
  return o;
}

// The z-min key of one point (see the batched projection in lt_project.hip): hi word = float32 bits of the depth (positive
// floats order like unsigned integers); lo word = 0x7fffffff - index for a point whose depth lies BELOW its float32 value
// (they beat the others, the highest index first), 0x80000000 | index otherwise (lowest index first).  float32 clouds never
// round: closest point, lowest index among equal depths.
#define LT_PB_EMPTY (~0ull)

template <typename T>
__device__ __forceinline__ unsigned long long pb_key(T depth, int i) {
  const float df = (float)depth;
  const bool up = (double)depth < (double)df;  // lies below its float32 value: replaces an incumbent of the same bucket
  const unsigned lo = up ? (0x7fffffffu - (unsigned)i) : (0x80000000u | (unsigned)i);
  return ((unsigned long long)__float_as_uint(df) << 32) | lo;
}
__device__ __forceinline__ int pb_key_index(unsigned long long k) {
  const unsigned lo = (unsigned)k;
  return (lo & 0x80000000u) ? (int)(lo & 0x7fffffffu) : (int)(0x7fffffffu - lo);
}
