// lt_echo.hip -- the target sensor's ECHO MODEL: a beam with a divergence (the reference has none: its
// beams are lines).  Two kernels around the render.  k_subrays turns the finished ray tensor into S sub-rays per cell, the
// central ray and S - 1 on a ring; the render casts them like any single-origin ray batch into S sub-images; k_echo_resolve
// groups a cell's sub-hits into echoes along the range and reports one of them -- the first, the strongest or the last --
// with the blended range of what the spot covers within one pulse.  Sub-rays and sub-images lie PLANE BY PLANE: sub-ray k
// of cell i is element k * n + i, so a wave's loads of one plane are coalesced and plane 0 is a whole image.
//
// The contract (repeated in lidarhip.h so that a host can restate it exactly).  Float64 from the widened float32 values,
// every product, sum, quotient and square root rounded on its own (-ffp-contract=off, IEEE sqrt and /):
//   h2 = x*x + y*y;  dd = h2 + z*z                               d = rays[i] = (x, y, z)
//   n = sqrt(dd);  hx = x/n, hy = y/n, hz = z/n
//   h2 > 0 ? (h = sqrt(h2); ux = -y/h; uy = x/h) : (ux = 1; uy = 0)
//   vx = -(hz*uy);  vy = hz*ux;  vz = hx*uy - hy*ux
// k_subrays: !(dd > 0) or dd not finite, or (a, b) == (0, 0): the three floats of d, copied; else
//   s = float32( (hx + a*ux) + b*vx,  (hy + a*uy) + b*vy,  hz + b*vz )
// k_echo_resolve: sub-ray k is a hit when sub_tri >= 0 and sub_range > 0; the hits are walked in (t, k) order; the first
// opens an echo, one with (double)t - (double)t_first > separation the next; an echo keeps c, St, Srem (float64, in walk
// order, starting from its first member's value) and rep, its smallest k; it is detected when c >= min_subrays; the mode
// chooses among the detected; range = float32(St / c), endrem = float32(Srem / S), fraction = float32((double)c / S),
// label and tri are rep's, end point j = float32(o[j] + h[j] * (double)range).  No detected echo, or !(dd > 0) of the
// central ray: the miss, as lt_scan_write_miss (lt_scanimg.h) writes it.
// k_echo_resolve_dual (a dual-return sensor) is the same body with a SECOND echo per cell: chosen by second_mode among the
// detected echoes other than the primary -- first: the earliest of the rest, last: the latest, strongest: the largest Srem,
// a tie to the larger c, then to the earlier --, written with the primary's expressions on its own c, St, Srem and rep into
// a second set of outputs; fewer than two detected echoes, or !(dd > 0): the miss, and fraction2 = 0.  The primary set is
// bit for bit k_echo_resolve's.
#include <limits.h>
#include <math.h>

#include "lt_internal.h"
#include "lt_scanimg.h"

struct lt_subray_args {
  double off[2 * LT_ECHO_MAX_SUBRAYS];
  int S, n;
};

// One thread per cell: the frame (h, u, v) is two square roots and five quotients in float64, made once and used for the
// cell's S sub-rays.  The k loop is unrolled over the LT_ECHO_MAX_SUBRAYS slots so that off[] is read from the kernel
// arguments at constant offsets.  12-byte rows: three 4-byte accesses, nothing wider is aligned.
__global__ __launch_bounds__(256) void k_subrays(const lt_subray_args A, const float* __restrict__ rays,
                                                 float* __restrict__ subrays) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const float fx = rays[3 * (size_t)i], fy = rays[3 * (size_t)i + 1], fz = rays[3 * (size_t)i + 2];
  const double x = (double)fx, y = (double)fy, z = (double)fz;
  const double h2 = x * x + y * y;
  const double dd = h2 + z * z;
  const bool plain = !(dd > 0.0) || !(dd < HUGE_VAL);
  double hx = 0.0, hy = 0.0, hz = 0.0, ux = 1.0, uy = 0.0;
  if (!plain) {
    const double nn = sqrt(dd);
    hx = x / nn; hy = y / nn; hz = z / nn;
    if (h2 > 0.0) {
      const double h = sqrt(h2);
      ux = -y / h; uy = x / h;
    }
  }
  const double vx = -(hz * uy), vy = hz * ux, vz = hx * uy - hy * ux;
#pragma unroll
  for (int k = 0; k < LT_ECHO_MAX_SUBRAYS; ++k) {
    if (k < A.S) {
      const double a = A.off[2 * k], b = A.off[2 * k + 1];
      float sx = fx, sy = fy, sz = fz;
      if (!plain && !(a == 0.0 && b == 0.0)) {
        sx = (float)((hx + a * ux) + b * vx);
        sy = (float)((hy + a * uy) + b * vy);
        sz = (float)(hz + b * vz);
      }
      const size_t o = 3 * ((size_t)k * (size_t)A.n + (size_t)i);
      subrays[o] = sx; subrays[o + 1] = sy; subrays[o + 2] = sz;
    }
  }
}

struct lt_echo_args {
  double separation;
  double ox, oy, oz;  // the ray origin, widened
  int S, min_subrays, n;
  unsigned mode;
};

// a sub-hit in a register slot: key = (float bits of t) << 3 | k, all ones for an absent slot (no hit, or k >= S), so an
// ascending sort of the keys is the (t, k) order with the absent slots last; t > 0, so its bits order like its value
struct lt_echo_hit {
  unsigned long long key;
  float rem;
};

static __device__ __forceinline__ void lt_echo_cx(lt_echo_hit& a, lt_echo_hit& b) {
  const bool sw = b.key < a.key;
  const unsigned long long ka = sw ? b.key : a.key, kb = sw ? a.key : b.key;
  const float ra = sw ? b.rem : a.rem, rb = sw ? a.rem : b.rem;
  a.key = ka; a.rem = ra; b.key = kb; b.rem = rb;
}

// the echoes of one cell while its hits are walked: the open echo and the chosen one
struct lt_echo_walk {
  double t_first, st, sr;  // the open echo
  int c, rep;
  double ch_st, ch_sr;     // the chosen echo (ch_c == 0: none yet)
  int ch_c, ch_rep, ch_ord;  // ch_ord: its ordinal among the detected echoes (read by the dual resolve only)
  int n_det;
};

// SKIP: the detected echo of ordinal `skip` is passed over (the second walk of the dual resolve, which chooses among the rest)
template <bool SKIP>
static __device__ __forceinline__ void lt_echo_close(lt_echo_walk& w, int min_subrays, unsigned mode, int skip) {
  if (w.c < min_subrays || w.c == 0) return;
  const int ord = w.n_det;
  ++w.n_det;
  if (SKIP && ord == skip) return;
  bool take = w.ch_c == 0;
  if (mode == LT_ECHO_LAST) take = true;
  else if (mode == LT_ECHO_STRONGEST) take = take || w.sr > w.ch_sr || (w.sr == w.ch_sr && w.c > w.ch_c);
  if (take) { w.ch_st = w.st; w.ch_sr = w.sr; w.ch_c = w.c; w.ch_rep = w.rep; w.ch_ord = ord; }
}

// the fully unrolled walk over the sorted slots: steps 3 - 6 of the contract, `mode` choosing among the detected echoes
// (without the one of ordinal `skip` when SKIP)
template <bool SKIP>
static __device__ __forceinline__ void lt_echo_walk_slots(lt_echo_walk& w, const lt_echo_hit (&s)[LT_ECHO_MAX_SUBRAYS],
                                                          double separation, int min_subrays, unsigned mode, int skip) {
  w.t_first = 0.0; w.st = 0.0; w.sr = 0.0; w.c = 0; w.rep = 0;
  w.ch_st = 0.0; w.ch_sr = 0.0; w.ch_c = 0; w.ch_rep = 0; w.ch_ord = -1; w.n_det = 0;
#pragma unroll
  for (int j = 0; j < LT_ECHO_MAX_SUBRAYS; ++j) {
    if (s[j].key != ~0ull) {
      const int k = (int)(s[j].key & 7ull);
      const double t = (double)__uint_as_float((unsigned)(s[j].key >> 3));
      const double r = (double)s[j].rem;
      if (w.c == 0 || t - w.t_first > separation) {
        lt_echo_close<SKIP>(w, min_subrays, mode, skip);
        w.t_first = t; w.st = t; w.sr = r; w.c = 1; w.rep = k;
      } else {
        w.st = w.st + t; w.sr = w.sr + r; w.c += 1; w.rep = k < w.rep ? k : w.rep;
      }
    }
  }
  lt_echo_close<SKIP>(w, min_subrays, mode, skip);
}

// the second return's outputs and its rule (the dual resolve only)
struct lt_echo_second {
  lt_scan_images images;
  float* fraction;
  unsigned mode;
};

// One thread per cell, 256-thread workgroups, no LDS, no atomics.  The S <= 8 candidates stay in registers: fixed
// LT_ECHO_MAX_SUBRAYS slots, a fully unrolled 19-comparator sorting network on the packed keys with the remission carried
// along, then a fully unrolled walk; nothing is indexed at run time (that would go to scratch).  The 2S (or 3S) loads of
// the sub-images do not depend on one another and are issued together; the label and the triangle of the chosen echo's
// representative are two dependent loads behind the walk; every load comes ahead of the cell's first store.
// DUAL: a second walk over the same sorted slots chooses the second echo among the detected ones other than the primary,
// which it passes over by its ordinal; the primary's sums are four registers by then and the slots are still live, so the
// second walk costs no register the first did not.  Both representatives' gathers are issued together behind the walks.
template <bool DUAL>
static __device__ __forceinline__ void lt_echo_body(const lt_echo_args& A, const lt_echo_second& B, const float* __restrict__ rays,
                                                    const float* __restrict__ sub_range, const int* __restrict__ sub_label,
                                                    const float* __restrict__ sub_rem, const int* __restrict__ sub_tri,
                                                    float* __restrict__ endpoints, int* __restrict__ endcolors,
                                                    float* __restrict__ range, float* __restrict__ endrem,
                                                    int* __restrict__ tri, unsigned char* __restrict__ n_echoes,
                                                    float* __restrict__ fraction) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const double x = (double)rays[3 * (size_t)i], y = (double)rays[3 * (size_t)i + 1], z = (double)rays[3 * (size_t)i + 2];
  lt_echo_hit s[LT_ECHO_MAX_SUBRAYS];
#pragma unroll
  for (int k = 0; k < LT_ECHO_MAX_SUBRAYS; ++k) {
    s[k].key = ~0ull;
    s[k].rem = 0.f;
    if (k < A.S) {
      const size_t e = (size_t)k * (size_t)A.n + (size_t)i;
      const int tk = sub_tri[e];
      const float t = sub_range[e];
      const float r = sub_rem ? sub_rem[e] : 0.f;
      if (tk >= 0 && t > 0.f) {
        s[k].key = ((unsigned long long)__float_as_uint(t) << 3) | (unsigned long long)k;
        s[k].rem = r;
      }
    }
  }
  // Batcher's odd-even merge sort of 8: 19 compare-exchanges
  lt_echo_cx(s[0], s[1]); lt_echo_cx(s[2], s[3]); lt_echo_cx(s[4], s[5]); lt_echo_cx(s[6], s[7]);
  lt_echo_cx(s[0], s[2]); lt_echo_cx(s[1], s[3]); lt_echo_cx(s[4], s[6]); lt_echo_cx(s[5], s[7]);
  lt_echo_cx(s[1], s[2]); lt_echo_cx(s[5], s[6]);
  lt_echo_cx(s[0], s[4]); lt_echo_cx(s[1], s[5]); lt_echo_cx(s[2], s[6]); lt_echo_cx(s[3], s[7]);
  lt_echo_cx(s[2], s[4]); lt_echo_cx(s[3], s[5]);
  lt_echo_cx(s[1], s[2]); lt_echo_cx(s[3], s[4]); lt_echo_cx(s[5], s[6]);

  lt_echo_walk w;
  lt_echo_walk_slots<false>(w, s, A.separation, A.min_subrays, A.mode, 0);

  const double h2 = x * x + y * y;
  const double dd = h2 + z * z;
  const bool hit = w.ch_c > 0 && dd > 0.0;
  double st2 = 0.0, sr2 = 0.0;
  int c2 = 0, rep2 = 0;
  if constexpr (DUAL) {
    if (w.n_det >= 2) {   // (n_det < 2: no second echo, and no second walk)
      lt_echo_walk w2;
      lt_echo_walk_slots<true>(w2, s, A.separation, A.min_subrays, B.mode, w.ch_ord);
      st2 = w2.ch_st; sr2 = w2.ch_sr; c2 = w2.ch_c; rep2 = w2.ch_rep;
    }
  }
  const bool hit2 = DUAL && c2 > 0 && dd > 0.0;
  float px = 0.f, py = 0.f, pz = 0.f, rf = 0.f, er = 0.f, fr = 0.f;
  float qx = 0.f, qy = 0.f, qz = 0.f, rf2 = 0.f, er2 = 0.f, fr2 = 0.f;
  int lab = 0, tr = -1, lab2 = 0, tr2 = -1;
  if (hit) {
    const size_t e = (size_t)w.ch_rep * (size_t)A.n + (size_t)i;
    tr = sub_tri[e];
    if (sub_label) lab = sub_label[e];
  }
  if constexpr (DUAL) {
    if (hit2) {
      const size_t e = (size_t)rep2 * (size_t)A.n + (size_t)i;
      tr2 = sub_tri[e];
      if (sub_label) lab2 = sub_label[e];
    }
  }
  if (hit) {
    const double nn = sqrt(dd);
    rf = (float)(w.ch_st / (double)w.ch_c);
    er = (float)(w.ch_sr / (double)A.S);
    fr = (float)((double)w.ch_c / (double)A.S);
    px = (float)(A.ox + (x / nn) * (double)rf);
    py = (float)(A.oy + (y / nn) * (double)rf);
    pz = (float)(A.oz + (z / nn) * (double)rf);
    if constexpr (DUAL) {
      if (hit2) {
        rf2 = (float)(st2 / (double)c2);
        er2 = (float)(sr2 / (double)A.S);
        fr2 = (float)((double)c2 / (double)A.S);
        qx = (float)(A.ox + (x / nn) * (double)rf2);
        qy = (float)(A.oy + (y / nn) * (double)rf2);
        qz = (float)(A.oz + (z / nn) * (double)rf2);
      }
    }
  }
  // (a set without an echo holds the values lt_scan_write_miss writes, and fraction 0)
  lt_scan_write_echo({endpoints, endcolors, range, endrem, tri}, fraction, (size_t)i, px, py, pz, lab, rf, er, tr, fr);
  if (n_echoes) n_echoes[i] = (unsigned char)w.n_det;
  if constexpr (DUAL) lt_scan_write_echo(B.images, B.fraction, (size_t)i, qx, qy, qz, lab2, rf2, er2, tr2, fr2);
}

__global__ __launch_bounds__(256) void k_echo_resolve(const lt_echo_args A, const float* __restrict__ rays,
                                                      const float* __restrict__ sub_range, const int* __restrict__ sub_label,
                                                      const float* __restrict__ sub_rem, const int* __restrict__ sub_tri,
                                                      float* __restrict__ endpoints, int* __restrict__ endcolors,
                                                      float* __restrict__ range, float* __restrict__ endrem,
                                                      int* __restrict__ tri, unsigned char* __restrict__ n_echoes,
                                                      float* __restrict__ fraction) {
  lt_echo_body<false>(A, lt_echo_second{}, rays, sub_range, sub_label, sub_rem, sub_tri, endpoints, endcolors, range, endrem, tri,
                      n_echoes, fraction);
}

__global__ __launch_bounds__(256) void k_echo_resolve_dual(const lt_echo_args A, const lt_echo_second B,
                                                           const float* __restrict__ rays, const float* __restrict__ sub_range,
                                                           const int* __restrict__ sub_label, const float* __restrict__ sub_rem,
                                                           const int* __restrict__ sub_tri, float* __restrict__ endpoints,
                                                           int* __restrict__ endcolors, float* __restrict__ range,
                                                           float* __restrict__ endrem, int* __restrict__ tri,
                                                           unsigned char* __restrict__ n_echoes, float* __restrict__ fraction) {
  lt_echo_body<true>(A, B, rays, sub_range, sub_label, sub_rem, sub_tri, endpoints, endcolors, range, endrem, tri, n_echoes,
                     fraction);
}

// NULL when the model can be used, else what is wrong with it (written so that a NaN fails)
static const char* lt_echo_model_problem(const lt_echo_model* m) {
  if (m->n_subrays < 2 || m->n_subrays > LT_ECHO_MAX_SUBRAYS) return "n_subrays must be 2 .. 8";
  if (m->min_subrays < 1 || m->min_subrays > m->n_subrays) return "min_subrays must be 1 .. n_subrays";
  if (m->mode != LT_ECHO_FIRST && m->mode != LT_ECHO_STRONGEST && m->mode != LT_ECHO_LAST)
    return "mode must be LT_ECHO_FIRST, LT_ECHO_STRONGEST or LT_ECHO_LAST";
  if (!(m->separation > 0.0 && m->separation < HUGE_VAL)) return "separation must be finite and > 0";
  for (int k = 0; k < 2 * m->n_subrays; ++k)
    if (!(m->off[k] - m->off[k] == 0.0)) return "the offsets must be finite";
  return NULL;
}

extern "C" int lt_create_subrays_dev(const float* rays, int n, const lt_echo_model* model, float* subrays, void* stream) {
  if (!model || n < 0 || (n > 0 && (!rays || !subrays))) {
    lt_set_error("lt_create_subrays_dev: invalid argument (a model, n >= 0 = %d; rays and subrays are mandatory)", n);
    return LT_ERR_INVALID_ARG;
  }
  const char* why = lt_echo_model_problem(model);
  if (why) {
    lt_set_error("lt_create_subrays_dev: invalid model: %s (n_subrays=%d min_subrays=%d mode=%u separation=%g)", why,
                 model->n_subrays, model->min_subrays, model->mode, model->separation);
    return LT_ERR_INVALID_ARG;
  }
  if ((long long)n * model->n_subrays > (long long)INT_MAX) {
    lt_set_error("lt_create_subrays_dev: invalid argument (n_subrays * n = %d * %d does not fit an int)", model->n_subrays, n);
    return LT_ERR_INVALID_ARG;
  }
  if (n == 0) return LT_OK;
  lt_subray_args A;
  for (int k = 0; k < 2 * LT_ECHO_MAX_SUBRAYS; ++k) A.off[k] = k < 2 * model->n_subrays ? model->off[k] : 0.0;
  A.S = model->n_subrays;
  A.n = n;
  hipLaunchKernelGGL(k_subrays, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, rays, subrays);
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// the checks the two resolve entries share, with `who` leading the message; LT_OK, or the error that was set
static int lt_echo_resolve_check(const char* who, const float* rays, const float* origin, int n, const lt_echo_model* model,
                                 const float* sub_range, const int* sub_tri, const float* range, const int* tri) {
  if (!origin || !model || n < 0 || (n > 0 && (!rays || !sub_range || !sub_tri || !range || !tri))) {
    lt_set_error("%s: invalid argument (an origin, a model, n >= 0 = %d; rays, sub_range, sub_tri, range and "
                 "tri are mandatory)", who, n);
    return LT_ERR_INVALID_ARG;
  }
  if (!lt_finite3(origin)) {
    lt_set_error("%s: invalid origin (three finite numbers; %g %g %g)", who, (double)origin[0], (double)origin[1],
                 (double)origin[2]);
    return LT_ERR_INVALID_ARG;
  }
  const char* why = lt_echo_model_problem(model);
  if (why) {
    lt_set_error("%s: invalid model: %s (n_subrays=%d min_subrays=%d mode=%u separation=%g)", who, why,
                 model->n_subrays, model->min_subrays, model->mode, model->separation);
    return LT_ERR_INVALID_ARG;
  }
  if ((long long)n * model->n_subrays > (long long)INT_MAX) {
    lt_set_error("%s: invalid argument (n_subrays * n = %d * %d does not fit an int)", who, model->n_subrays, n);
    return LT_ERR_INVALID_ARG;
  }
  return LT_OK;
}

static lt_echo_args lt_echo_args_of(const float* origin, int n, const lt_echo_model* model) {
  lt_echo_args A;
  A.separation = model->separation;
  A.ox = (double)origin[0]; A.oy = (double)origin[1]; A.oz = (double)origin[2];
  A.S = model->n_subrays; A.min_subrays = model->min_subrays; A.n = n;
  A.mode = model->mode;
  return A;
}

extern "C" int lt_echo_resolve_dev(const float* rays, const float* origin, int n, const lt_echo_model* model,
                                   const float* sub_range, const int* sub_label, const float* sub_rem, const int* sub_tri,
                                   float* endpoints, int* endcolors, float* range, float* endrem, int* tri,
                                   unsigned char* n_echoes, float* fraction, void* stream) {
  const int rc = lt_echo_resolve_check("lt_echo_resolve_dev", rays, origin, n, model, sub_range, sub_tri, range, tri);
  if (rc != LT_OK) return rc;
  if (n == 0) return LT_OK;
  const lt_echo_args A = lt_echo_args_of(origin, n, model);
  hipLaunchKernelGGL(k_echo_resolve, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, rays, sub_range, sub_label,
                     sub_rem, sub_tri, endpoints, endcolors, range, endrem, tri, n_echoes, fraction);
  LT_HIP(hipGetLastError());
  return LT_OK;
}

extern "C" int lt_echo_resolve_dual_dev(const float* rays, const float* origin, int n, const lt_echo_model* model,
                                        unsigned second_mode, const float* sub_range, const int* sub_label,
                                        const float* sub_rem, const int* sub_tri, float* endpoints, int* endcolors,
                                        float* range, float* endrem, int* tri, unsigned char* n_echoes, float* fraction,
                                        float* endpoints2, int* endcolors2, float* range2, float* endrem2, int* tri2,
                                        float* fraction2, void* stream) {
  const int rc = lt_echo_resolve_check("lt_echo_resolve_dual_dev", rays, origin, n, model, sub_range, sub_tri, range, tri);
  if (rc != LT_OK) return rc;
  if (n > 0 && (!range2 || !tri2)) {
    lt_set_error("lt_echo_resolve_dual_dev: invalid argument (range2 and tri2 are mandatory)");
    return LT_ERR_INVALID_ARG;
  }
  if (second_mode != LT_ECHO_FIRST && second_mode != LT_ECHO_STRONGEST && second_mode != LT_ECHO_LAST) {
    lt_set_error("lt_echo_resolve_dual_dev: invalid second_mode %u (LT_ECHO_FIRST, LT_ECHO_STRONGEST or LT_ECHO_LAST)",
                 second_mode);
    return LT_ERR_INVALID_ARG;
  }
  if (n == 0) return LT_OK;
  const lt_echo_args A = lt_echo_args_of(origin, n, model);
  const lt_echo_second B = {{endpoints2, endcolors2, range2, endrem2, tri2}, fraction2, second_mode};
  hipLaunchKernelGGL(k_echo_resolve_dual, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, B, rays, sub_range,
                     sub_label, sub_rem, sub_tri, endpoints, endcolors, range, endrem, tri, n_echoes, fraction);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
