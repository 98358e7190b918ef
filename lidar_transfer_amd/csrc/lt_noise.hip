// lt_noise.hip -- the target sensor's NOISE MODEL (the reference has none: create_rays leaves it as a
// TODO, laserscan.py:1094-1096).  One kernel behind the render and the return model, in place on the render's images: the
// range of a return is jittered along its ray and reported on a grid, its end point follows, its remission is jittered,
// clamped and reported on L levels; a return whose measured range leaves the sensor's gate is lost.
#include "lt_internal.h"
#include "lt_scanimg.h"

// z of lidarhip.h: twelve 16-bit uniforms, the halves of mix(g + first) .. mix(g + first + 5), summed as integers
static __device__ __forceinline__ double lt_noise_draw(unsigned g, unsigned first) {
  int S = 0;
#pragma unroll
  for (unsigned k = 0; k < 6; ++k) {
    const unsigned w = lt_mix32(g + first + k);
    S += (int)(w & 0xffffu) + (int)(w >> 16);
  }
  return (double)(S - 393210) / 65536.0;
}

struct lt_noise_args {
  double range_sigma, range_sigma_rel, range_resolution, remission_sigma;
  double min_range, max_range;
  double levels_m1;    // remission_levels - 1, or 0: off
  double ox, oy, oz;   // the ray origin, widened
  unsigned scan_hash;  // mix(mix(seed ^ 0x6e6f6973) + scan): the part of g that is one number per launch
  int label;
  int n;
};

// One thread per cell.  12-byte rows (end point, colour): three 4-byte accesses, nothing wider is aligned.  The cell's
// loads -- tri, range, remission, end point -- do not depend on one another and are issued together, whether the cell is a
// return or not; everything is loaded before the first store.  No mesh is read, no LDS, no atomics.  The two draws are
// twelve mix() calls: integer VALU work that a lane without a return skips.
__global__ __launch_bounds__(256) void k_noise_model(const lt_noise_args A, float* __restrict__ endpoints,
                                                     int* __restrict__ endcolors, float* __restrict__ range,
                                                     float* __restrict__ endrem, int* __restrict__ tri,
                                                     float* __restrict__ range_error, unsigned char* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const int t = tri[i];
  const float rf = range[i];
  const float er = endrem ? endrem[i] : 0.f;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (endpoints) { px = endpoints[3 * (size_t)i]; py = endpoints[3 * (size_t)i + 1]; pz = endpoints[3 * (size_t)i + 2]; }
  int st = 0;
  float err = 0.f;
  if (t >= 0 && rf > 0.f) {
    const unsigned g = lt_mix32(A.scan_hash + (unsigned)i);
    const double r = (double)rf;
    const double r1 = r + (A.range_sigma + A.range_sigma_rel * r) * lt_noise_draw(g, 1u);
    const double r2 = A.range_resolution > 0.0 ? rint(r1 / A.range_resolution) * A.range_resolution : r1;
    if (!(r2 > 0.0) || r2 < A.min_range || r2 > A.max_range) {
      st = 2;  // the return is lost: the cell becomes a miss
      lt_scan_write_miss({endpoints, endcolors, range, endrem, tri}, (size_t)i, A.label != 0);
    } else {
      st = 1;
      err = (float)(r2 - r);
      range[i] = (float)r2;
      if (endpoints) {
        const double s = r2 / r;
        endpoints[3 * (size_t)i] = (float)(A.ox + ((double)px - A.ox) * s);
        endpoints[3 * (size_t)i + 1] = (float)(A.oy + ((double)py - A.oy) * s);
        endpoints[3 * (size_t)i + 2] = (float)(A.oz + ((double)pz - A.oz) * s);
      }
      if (endrem) {
        double e = (double)er + A.remission_sigma * lt_noise_draw(g, 7u);
        e = e < 0.0 ? 0.0 : (e > 1.0 ? 1.0 : e);
        if (A.levels_m1 > 0.0) e = rint(e * A.levels_m1) / A.levels_m1;
        endrem[i] = (float)e;
      }
    }
  }
  if (range_error) range_error[i] = err;
  if (state) state[i] = (unsigned char)st;
}

extern "C" int lt_noise_model_dev(const float* origin, int n, const lt_noise_model* model, unsigned scan, float* endpoints,
                                  int* endcolors, float* range, float* endrem, int* tri, float* range_error,
                                  unsigned char* state, unsigned trace_flags, void* stream) {
  if (!origin || !model || n < 0 || (n > 0 && (!range || !tri))) {
    lt_set_error("lt_noise_model_dev: invalid argument (an origin, a model, n >= 0 = %d; range and tri are mandatory)", n);
    return LT_ERR_INVALID_ARG;
  }
  // (written so that a NaN fails)
  const double inf = HUGE_VAL;
  if (!lt_finite3(origin)) {
    lt_set_error("lt_noise_model_dev: invalid origin (three finite numbers; %g %g %g)", (double)origin[0], (double)origin[1],
                 (double)origin[2]);
    return LT_ERR_INVALID_ARG;
  }
  if (!(model->range_sigma >= 0.0 && model->range_sigma < inf && model->range_sigma_rel >= 0.0 && model->range_sigma_rel < inf &&
        model->range_resolution >= 0.0 && model->range_resolution < inf && model->remission_sigma >= 0.0 &&
        model->remission_sigma < inf && model->min_range >= 0.0 && model->max_range >= model->min_range) ||
      model->remission_levels == 1u) {
    lt_set_error("lt_noise_model_dev: invalid model (finite range_sigma, range_sigma_rel, range_resolution, remission_sigma >= 0, "
                 "0 <= min_range <= max_range, remission_levels 0 or >= 2; range_sigma=%g range_sigma_rel=%g range_resolution=%g "
                 "remission_sigma=%g min_range=%g max_range=%g remission_levels=%u)", model->range_sigma, model->range_sigma_rel,
                 model->range_resolution, model->remission_sigma, model->min_range, model->max_range, model->remission_levels);
    return LT_ERR_INVALID_ARG;
  }
  if (n == 0) return LT_OK;
  lt_noise_args A;
  A.range_sigma = model->range_sigma; A.range_sigma_rel = model->range_sigma_rel;
  A.range_resolution = model->range_resolution; A.remission_sigma = model->remission_sigma;
  A.min_range = model->min_range; A.max_range = model->max_range;
  A.levels_m1 = model->remission_levels ? (double)(model->remission_levels - 1u) : 0.0;
  A.ox = (double)origin[0]; A.oy = (double)origin[1]; A.oz = (double)origin[2];
  A.scan_hash = lt_mix32(lt_mix32(model->seed ^ 0x6e6f6973u) + scan);
  A.label = (trace_flags & LT_TRACE_LABEL_IMAGE) != 0;
  A.n = n;
  hipLaunchKernelGGL(k_noise_model, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, endpoints, endcolors, range,
                     endrem, tri, range_error, state);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
