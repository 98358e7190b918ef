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
