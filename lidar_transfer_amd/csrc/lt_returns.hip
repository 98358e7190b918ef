// lt_returns.hip -- the target sensor's RETURN MODEL (the reference has none: throw_rays_at_mesh
// writes every hit, fusion_lidar.py:426-455).  One kernel behind the render, in place on its images: a return outside the
// range gate, seen too close to edge-on, or dropped at random becomes a miss; the remission of one that stands may fall with
// the cosine of the incidence angle.
#include "lt_internal.h"
#include "lt_scanimg.h"

struct lt_ret_args {
  double min_range, max_range, min_cos;
  unsigned drop_threshold;
  unsigned scan_hash;  // mix(mix(seed) + scan): the part of hash(seed, scan, i) that is one number per launch
  int lambert, label;
  int n, n_faces, n_verts;
};

// One thread per cell.  12-byte rows (ray, end point, colour, face, vertex): three 4-byte accesses, nothing wider is
// aligned.  The cell's independent loads -- tri, range, remission, ray -- are issued together; behind tri hangs the one
// dependent chain tri -> face triple -> three vertices (three round trips, k_sc_resolve's shape), which a lane without a
// hit does not enter.  Everything is loaded before the first store.  No LDS, no atomics but the error flag's.
__global__ __launch_bounds__(256) void k_return_model(const lt_ret_args A, const float* __restrict__ rays,
                                                      const float* __restrict__ verts, const int* __restrict__ faces,
                                                      float* __restrict__ endpoints, int* __restrict__ endcolors,
                                                      float* __restrict__ range, float* __restrict__ endrem,
                                                      int* __restrict__ tri, float* __restrict__ incidence,
                                                      unsigned char* __restrict__ drop, unsigned* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const int t = tri[i];
  const float r = range[i];
  const float er = endrem ? endrem[i] : 0.f;
  const float fdx = rays[3 * (size_t)i], fdy = rays[3 * (size_t)i + 1], fdz = rays[3 * (size_t)i + 2];
  // a face beside the mesh, or one whose vertices are: the deferred error; the cell counts as "no hit" and is not touched
  bool hit = t >= 0 && t < A.n_faces;
  bool bad = t < -1 || t >= A.n_faces;
  int i0 = 0, i1 = 0, i2 = 0;
  if (hit) {
    i0 = faces[3 * (size_t)t]; i1 = faces[3 * (size_t)t + 1]; i2 = faces[3 * (size_t)t + 2];
    if ((unsigned)i0 >= (unsigned)A.n_verts || (unsigned)i1 >= (unsigned)A.n_verts || (unsigned)i2 >= (unsigned)A.n_verts) {
      hit = false;
      bad = true;
    }
  }
  if (bad) atomicOr(flags, LT_FLAG_BAD_INDEX);
  int code = 1;
  double c = 0.0;
  if (hit) {
    const float* pa = verts + 3 * (size_t)i0;
    const float* pb = verts + 3 * (size_t)i1;
    const float* pc = verts + 3 * (size_t)i2;
    const double v0x = (double)pa[0], v0y = (double)pa[1], v0z = (double)pa[2];
    const double v1x = (double)pb[0], v1y = (double)pb[1], v1z = (double)pb[2];
    const double v2x = (double)pc[0], v2y = (double)pc[1], v2z = (double)pc[2];
    const double dx = (double)fdx, dy = (double)fdy, dz = (double)fdz;
    const double e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
    const double e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double dot = (nx * dx + ny * dy) + nz * dz;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const double dd = (dx * dx + dy * dy) + dz * dz;
    if (!(nn == 0.0 || dd == 0.0)) {
      const double q = fabs(dot) / sqrt(nn * dd);
      c = q < 1.0 ? q : 1.0;
    }
    const double rd = (double)r;
    if (rd < A.min_range) code = 2;
    else if (rd > A.max_range) code = 3;
    else if (c < A.min_cos) code = 4;
    else if (lt_mix32(A.scan_hash + (unsigned)i) < A.drop_threshold) code = 5;
    else code = 0;
  }
  if (code >= 2) {  // the return is lost: the cell becomes a miss
    lt_scan_write_miss({endpoints, endcolors, range, endrem, tri}, (size_t)i, A.label != 0);
  } else if (code == 0 && A.lambert && endrem) {
    endrem[i] = (float)((double)er * c);
  }
  if (incidence) incidence[i] = code == 0 ? (float)c : -1.f;
  if (drop) drop[i] = (unsigned char)code;
}

extern "C" int lt_return_model_dev(lt_scene* s, const float* rays, int n_rays, const lt_return_model* model, unsigned scan,
                                   float* endpoints, int* endcolors, float* range, float* endrem, int* tri, float* incidence,
                                   unsigned char* drop, unsigned trace_flags, void* stream) {
  if (!s || !model || n_rays < 0 || (n_rays > 0 && (!rays || !range || !tri))) {
    lt_set_error("lt_return_model_dev: invalid argument (a scene, a model, n_rays >= 0 = %d; rays, range and tri are mandatory)",
                 n_rays);
    return LT_ERR_INVALID_ARG;
  }
  // (written so that a NaN fails)
  if (!(model->min_range >= 0.0 && model->max_range >= model->min_range && model->min_cos >= 0.0 && model->min_cos <= 1.0) ||
      (model->flags & ~LT_RETURN_LAMBERT)) {
    lt_set_error("lt_return_model_dev: invalid model (0 <= min_range <= max_range, 0 <= min_cos <= 1, flags LT_RETURN_LAMBERT "
                 "or 0; min_range=%g max_range=%g min_cos=%g flags=%u)", model->min_range, model->max_range, model->min_cos,
                 model->flags);
    return LT_ERR_INVALID_ARG;
  }
  if (n_rays == 0) return LT_OK;
  if (s->n_faces > 0 && (!s->verts || !s->faces)) {
    lt_set_error("lt_return_model_dev: the scene has no mesh");
    return LT_ERR_INVALID_ARG;
  }
  LT_HIP(hipSetDevice(s->device));
  lt_ret_args A;
  A.min_range = model->min_range; A.max_range = model->max_range; A.min_cos = model->min_cos;
  A.drop_threshold = model->drop_threshold;
  A.scan_hash = lt_mix32(lt_mix32(model->seed) + scan);
  A.lambert = (model->flags & LT_RETURN_LAMBERT) != 0;
  A.label = (trace_flags & LT_TRACE_LABEL_IMAGE) != 0;
  A.n = n_rays; A.n_faces = s->n_faces; A.n_verts = s->n_verts;
  hipLaunchKernelGGL(k_return_model, dim3((n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, rays, s->verts,
                     s->faces, endpoints, endcolors, range, endrem, tri, incidence, drop, s->flags);
  LT_HIP(hipGetLastError());
  s->last_stream = (hipStream_t)stream;
  return LT_OK;
}
