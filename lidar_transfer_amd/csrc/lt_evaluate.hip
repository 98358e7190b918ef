// lt_evaluate.hip -- the evaluation half of the reference's per-scan loop body, without a host round trip:
//   * lt_source_scan_dev     the source reference scan of lidar_deform.py:396-409 from ONE resident raw scan: label & 0xFFFF,
//                            remove_classes(ignore), do_range_projection(fov, remove=True) on the float32 file points,
//                            do_label_projection; two kernels (a thread per raw point: ONE 64-bit atomicMin per kept point;
//                            a thread per cell: decode the winner, gather, re-arm the key)
//   * lt_target_view_dev     the same raw scan seen through the TARGET sensor's model from the target's pose -- what `cp` with
//                            one scan would put into the target image: widened to float64, optionally transformed, through
//                            project_model<double, ...> (every target model), the `_new` variant's z-min key; its own project
//                            kernel, then k_src_resolve as it is
//   * lt_compare_record_dev  compare() (auxiliary/laserscan.py:1181-1301) + iouEval.addBatch (np_ioueval.py:31-47) of one
//                            output scan into a small fixed-size record; two kernels (a thread per cell: masks, squared range
//                            difference, per-wave pair counting with ballots into an n_labels^2 workspace, one partial sum per
//                            workgroup; then 64 workgroups compact the counts of the label values present and add the partial
//                            sums in a fixed order) and one asynchronous copy of the record to the caller's memory
// The projection arithmetic is lt_projpoint.h's (shared with lt_project.hip).  Nothing here waits for another workgroup.
#include "lt_internal.h"
#include "lt_devmem.h"
#include "lt_projpoint.h"
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <mutex>
#include <new>

#define LT_EV_BITMAP_WORDS 2048  // 65536 bits: the `ignore` bitmap of long class lists
#define LT_EV_RECORD_BLOCKS 64

struct lt_evaluator {
  int device = 0, n_labels = 0;
  size_t cap_cells = 0;                 // cells the source-scan keys are allocated (and armed) for
  unsigned long long* key = nullptr;    // [cap_cells] z-min keys, LT_PB_EMPTY between calls (k_src_resolve re-arms)
  bool armed = false;
  unsigned* bitmap = nullptr;           // [LT_EV_BITMAP_WORDS]
  unsigned* bad = nullptr;              // [1] labels outside the LUT, 0 between calls (k_src_resolve re-arms)
  unsigned* conf = nullptr;             // [n_labels^2] pair counts, all 0 between calls (k_cmp_record re-arms what was touched)
  unsigned* seen = nullptr;             // [n_labels + 1] == epoch: the value is present in this call; [n_labels]: a label out of range
  unsigned epoch = 0;
  bool conf_dirty = false;              // a call queued k_cmp_pairs but not k_cmp_record: conf must be cleared first
  size_t cap_blocks = 0;
  double* partial = nullptr;            // [cap_blocks] per-workgroup sums of squared range differences
  lt_compare_record* rec = nullptr;     // device staging of the record
  double* model = nullptr;              // [LT_MODEL_DOUBLES] the target view's sensor model (model_table), allocated by its first call
  double model_host[LT_MODEL_DOUBLES];  // ... as uploaded last: a call whose model has these bytes copies nothing
  int n_model = -1;
  std::mutex mu;
};

namespace {

struct SrcArgs {
  const float4* xyzr;
  const unsigned* label;
  int n, n_ign, use_bitmap, lut_len;
  unsigned short ign[LT_INGEST_LIST_ARGS];
};

__device__ __forceinline__ bool src_dropped(const SrcArgs& a, const unsigned* __restrict__ bitmap, unsigned l) {
  if (a.use_bitmap) return (bitmap[l >> 5] >> (l & 31u)) & 1u;
  bool drop = false;
  for (int k = 0; k < a.n_ign; ++k) drop |= l == (unsigned)a.ign[k];
  return drop;
}

// a thread per raw point: a dropped point does not bid for a cell; the raw index orders the kept points as the kept index does
__global__ __launch_bounds__(256) void k_src_project(const SrcArgs a, const unsigned* __restrict__ bitmap, float pi_t,
                                                     float abs_fov_down, float fov, int H, int W,
                                                     unsigned long long* __restrict__ key, unsigned* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool outside_lut = false;
  if (i < a.n) {
    const unsigned l = a.label[i] & 0xFFFFu;        // laserscan.py:588
    outside_lut = l >= (unsigned)a.lut_len;         // colorize() runs BEFORE remove_classes (lidar_deform.py:406-407)
    if (!src_dropped(a, bitmap, l)) {
      const float4 p = a.xyzr[i];                   // one 16-byte load
      const proj_out<float> o = project_point<float>(p.x, p.y, p.z, pi_t, abs_fov_down, fov, H, W, nullptr, 0, true, true);
      if (o.cell >= 0) atomicMin(&key[o.cell], pb_key<float>(o.depth, i));
    }
  }
  const unsigned long long m = __ballot(outside_lut);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(bad, (unsigned)__popcll(m));
}

// The target view's transform: rows 0..2 of T (x_target = T x_source), `on` == 0: none -- the widened values themselves, not
// a product with the identity (-0.0 keeps its sign).
struct ViewXf { double m[12]; int on; };

__device__ __forceinline__ double view_row(const double* __restrict__ m, double x, double y, double z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];  // step 5 of lt_ingest_scans_dev: every product and sum rounded on its own
}

// a thread per raw point, as k_src_project: the point in float64, in the target's frame, through the target's model (`tab`:
// model_table's doubles, no hard-coded beam angles); the `_new` variant's key (pb_key<double>: the rounded-up bucket)
template <int BEAMS, int SECTOR, int AZ>
__global__ __launch_bounds__(256) void k_view_project(const SrcArgs a, const unsigned* __restrict__ bitmap, const ViewXf T,
                                                      double pi_t, double abs_fov_down, double fov, int H, int W,
                                                      const double* __restrict__ tab, unsigned long long* __restrict__ key,
                                                      unsigned* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool outside_lut = false;
  if (i < a.n) {
    const unsigned l = a.label[i] & 0xFFFFu;
    outside_lut = l >= (unsigned)a.lut_len;
    if (!src_dropped(a, bitmap, l)) {
      const float4 p = a.xyzr[i];                   // one 16-byte load
      double x = (double)p.x, y = (double)p.y, z = (double)p.z;
      if (T.on) {
        const double tx = view_row(T.m, x, y, z), ty = view_row(T.m + 4, x, y, z), tz = view_row(T.m + 8, x, y, z);
        x = tx; y = ty; z = tz;
      }
      const proj_out<double> o = project_model<double, BEAMS, SECTOR, AZ>(x, y, z, pi_t, abs_fov_down, fov, H, W, tab, 0, true, true);
      if (o.cell >= 0) atomicMin(&key[o.cell], pb_key<double>(o.depth, i));
    }
  }
  const unsigned long long m = __ballot(outside_lut);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(bad, (unsigned)__popcll(m));
}

// a thread per cell: the winner's range, remission, label, black mask
__global__ __launch_bounds__(256) void k_src_resolve(const SrcArgs a, int H, int W, const float* __restrict__ lut, unsigned long long* __restrict__ key,
                                                     unsigned* __restrict__ bad, const lt_source_images out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0) {
    if (out.bad_labels) *out.bad_labels = *bad;
    *bad = 0u;
  }
  if (c >= H * W) return;
  const unsigned long long k = key[c];
  key[c] = LT_PB_EMPTY;
  const bool has = k != LT_PB_EMPTY;
  float range = -1.f, rem = -1.f;
  unsigned lab = 0u;
  if (has) {
    const int i = pb_key_index(k);
    const float4 p = a.xyzr[i];
    range = __uint_as_float((unsigned)(k >> 32));  // the key's high word IS the winner's float32 depth
    rem = p.w;
    lab = a.label[i] & 0xFFFFu;
  }
  if (out.range) out.range[c] = range;
  if (out.rem) out.rem[c] = rem;
  if (out.label) out.label[c] = (int)lab;
  if (out.black) {  // np.sum(proj_color, axis=2) == 0 on the float64 image (laserscan.py:1200); an empty cell's colour is 0
    double s = 0.0;
    if (has && lut && lab < (unsigned)a.lut_len)
      s = ((double)lut[3 * (size_t)lab] + (double)lut[3 * (size_t)lab + 1]) + (double)lut[3 * (size_t)lab + 2];
    out.black[c] = s == 0.0 ? 1 : 0;
  }
}

// compare(), a thread per cell.  Masks as k_compare (lt_post.hip): a black source cell and source label 0 are background in
// both images.  conf[target * NL + source] over the label values 0 .. NL - 1; the lanes of a wave that hold the same pair
// count themselves with ballots: one atomic per distinct pair and wave.
__global__ __launch_bounds__(256) void k_cmp_pairs(const int* __restrict__ src_label, const unsigned char* __restrict__ black,
                                                   const int* __restrict__ tgt_label, const float* __restrict__ src_range,
                                                   const float* __restrict__ tgt_range, int n, int NL, unsigned epoch,
                                                   unsigned* __restrict__ conf, unsigned* __restrict__ seen,
                                                   double* __restrict__ partial) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  bool counted = false, outside = false;
  unsigned pair = 0u;
  if (i < n) {
    int sl = src_label[i], tl = tgt_label[i];
    if (black[i]) { sl = 0; tl = 0; }
    const bool bg = sl == 0;
    if (bg) tl = 0;
    counted = (unsigned)sl < (unsigned)NL && (unsigned)tl < (unsigned)NL;
    outside = !counted;
    pair = counted ? (unsigned)tl * (unsigned)NL + (unsigned)sl : 0u;
    const float sr = bg ? 0.f : src_range[i], tr = bg ? 0.f : tgt_range[i];
    const float d = sr - tr;
    sq = (double)(d * d);
  }
  for (unsigned long long rest = __ballot(counted); rest;) {
    const int leader = __ffsll((long long)rest) - 1;
    const unsigned k = (unsigned)__shfl((int)pair, leader, 64);
    const unsigned long long same = __ballot(counted && pair == k);
    if ((int)(threadIdx.x & 63) == leader) {
      atomicAdd(&conf[k], (unsigned)__popcll(same));
      const unsigned t = k / (unsigned)NL, s = k - t * (unsigned)NL;
      if (seen[t] != epoch) seen[t] = epoch;   // (every writer stores the same value)
      if (seen[s] != epoch) seen[s] = epoch;
    }
    rest &= ~same;
  }
  if (__ballot(outside) && (threadIdx.x & 63) == 0) seen[NL] = epoch;
  // bitwise reproducible: a fixed shuffle tree per wave, the four waves in order, one stored partial per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// LT_EV_RECORD_BLOCKS workgroups: every one ranks the values present (NL words), then takes the rows t = block, block + 64 ...
// of the pair counts: a row of a value that is not present holds zeros only and is never read.  Workgroup 0 also adds the
// partial sums in a fixed order and writes the record's head.
__global__ __launch_bounds__(256) void k_cmp_record(int NL, unsigned epoch, unsigned* __restrict__ conf,
                                                    const unsigned* __restrict__ seen, const double* __restrict__ partial,
                                                    int nblocks, int n, const unsigned* __restrict__ src_bad,
                                                    lt_compare_record* __restrict__ rec) {
  __shared__ short rank[LT_COMPARE_MAX_NLABELS];
  __shared__ int part[256];
  __shared__ double dsum[256];
  const int tid = threadIdx.x;
  const int per = NL / 256, l0 = tid * per;
  int cnt = 0;
  for (int k = 0; k < per; ++k) cnt += seen[l0 + k] == epoch;
  part[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // Hillis-Steele over 256 counts
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int P = part[255];
  int run = part[tid] - cnt;
  for (int k = 0; k < per; ++k) {
    const bool p = seen[l0 + k] == epoch;
    rank[l0 + k] = p ? (short)run : (short)-1;
    if (p) {
      if (blockIdx.x == 0 && run < LT_COMPARE_MAX_PRESENT) rec->present[run] = l0 + k;
      ++run;
    }
  }
  __syncthreads();
  const bool fits = P <= LT_COMPARE_MAX_PRESENT;
  for (int t = blockIdx.x; t < NL; t += gridDim.x) {
    const int rt = rank[t];
    if (rt < 0) continue;
    for (int s = tid; s < NL; s += 256) {
      const int rs = rank[s];
      if (rs < 0) continue;
      const unsigned v = conf[(size_t)t * NL + s];
      if (fits) rec->counts[rt * P + rs] = v;
      if (v) conf[(size_t)t * NL + s] = 0u;
    }
  }
  if (blockIdx.x == 0) {
    double a = 0.0;
    for (int b = tid; b < nblocks; b += 256) a += partial[b];
    dsum[tid] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) dsum[tid] += dsum[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      rec->status = seen[NL] == epoch ? LT_COMPARE_LABEL_RANGE : (fits ? 0 : LT_COMPARE_OVERFLOW);
      rec->n_present = P;
      rec->n_cells = n;
      rec->src_bad_labels = src_bad ? *src_bad : 0u;
      rec->sq_sum = dsum[0];
    }
  }
}

void ev_free(lt_evaluator* e) {
  void* ps[] = {e->key, e->bitmap, e->bad, e->conf, e->seen, e->partial, e->rec, e->model};
  for (void* p : ps)
    if (p) (void)hipFree(p);
}

// the z-min cells of a view of `cells` cells, exactly; new cells are not armed
int ev_reserve_key(const char* who, lt_evaluator* e, size_t cells, hipStream_t st) {
  if (cells <= e->cap_cells) return LT_OK;
  LT_CHECK(lt_dev_grow(who, lt_wait_stream(st), &e->key, &e->cap_cells, cells, cells));
  e->armed = false;
  return LT_OK;
}

}  // namespace

extern "C" int lt_evaluator_create(lt_evaluator** ev, int n_labels, int device) {
  if (!ev || n_labels < 256 || n_labels > LT_COMPARE_MAX_NLABELS || n_labels % 256) {
    lt_set_error("lt_evaluator_create: n_labels=%d (a multiple of 256, at most %d)", n_labels, LT_COMPARE_MAX_NLABELS);
    return LT_ERR_INVALID_ARG;
  }
  *ev = nullptr;
  int dev = device;
  if (dev < 0) LT_HIP(hipGetDevice(&dev));
  LT_HIP(hipSetDevice(dev));
  lt_evaluator* e = new (std::nothrow) lt_evaluator();
  if (!e) {
    lt_set_error("lt_evaluator_create: out of host memory");
    return LT_ERR_NO_MEMORY;
  }
  e->device = dev;
  e->n_labels = n_labels;
  const size_t nl = (size_t)n_labels;
  bool ok = hipMalloc((void**)&e->bitmap, LT_EV_BITMAP_WORDS * sizeof(unsigned)) == hipSuccess &&
            hipMalloc((void**)&e->bad, sizeof(unsigned)) == hipSuccess &&
            hipMalloc((void**)&e->conf, nl * nl * sizeof(unsigned)) == hipSuccess &&
            hipMalloc((void**)&e->seen, (nl + 1) * sizeof(unsigned)) == hipSuccess &&
            hipMalloc((void**)&e->rec, sizeof(lt_compare_record)) == hipSuccess;
  ok = ok && hipMemset(e->bad, 0, sizeof(unsigned)) == hipSuccess && hipMemset(e->conf, 0, nl * nl * sizeof(unsigned)) == hipSuccess &&
       hipMemset(e->seen, 0, (nl + 1) * sizeof(unsigned)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    ev_free(e);
    delete e;
    (void)hipGetLastError();
    lt_set_error("lt_evaluator_create: out of device memory");
    return LT_ERR_NO_MEMORY;
  }
  *ev = e;
  return LT_OK;
}

extern "C" int lt_evaluator_destroy(lt_evaluator* e) {
  if (!e) return LT_OK;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  ev_free(e);
  delete e;
  return LT_OK;
}

extern "C" int lt_source_scan_dev(lt_evaluator* e, const lt_raw_scan* scan, const int* ignore, int n_ignore, double fov_up,
                                  double fov_down, int H, int W, const float* color_lut, int lut_len,
                                  const lt_source_images* out, void* stream) {
  if (!e || !scan || !out || scan->n < 0 || (scan->n > 0 && (!scan->xyzr || !scan->label)) || ((uintptr_t)scan->xyzr & 15u) ||
      n_ignore < 0 || (n_ignore > 0 && !ignore) || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL - 4096 || lut_len < 0 ||
      (lut_len > 0 && !color_lut)) {
    lt_set_error("lt_source_scan_dev: invalid argument (n=%d H=%d W=%d n_ignore=%d lut_len=%d; xyzr must be 16-byte aligned)",
                 scan ? scan->n : -1, H, W, n_ignore, lut_len);
    return LT_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n_ignore; ++k)
    if (ignore[k] < 0 || ignore[k] > 65535) {
      lt_set_error("lt_source_scan_dev: class %d is outside 0..65535 (labels are masked to 16 bits)", ignore[k]);
      return LT_ERR_INVALID_ARG;
    }
  std::lock_guard<std::mutex> lock(e->mu);
  LT_HIP(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t cells = (size_t)H * W;
  LT_CHECK(ev_reserve_key("lt_source_scan_dev", e, cells, st));
  if (!e->armed) {  // first use, or the previous call failed half way
    LT_HIP(hipMemsetAsync(e->key, 0xFF, e->cap_cells * sizeof(unsigned long long), st));
    LT_HIP(hipMemsetAsync(e->bad, 0, sizeof(unsigned), st));
  }
  e->armed = false;
  SrcArgs a;
  memset(&a, 0, sizeof(a));
  a.xyzr = (const float4*)scan->xyzr;
  a.label = scan->label;
  a.n = scan->n;
  a.lut_len = lut_len;
  a.use_bitmap = n_ignore > LT_INGEST_LIST_ARGS;
  if (a.use_bitmap) {
    unsigned bits[LT_EV_BITMAP_WORDS];
    memset(bits, 0, sizeof(bits));
    for (int k = 0; k < n_ignore; ++k) bits[ignore[k] >> 5] |= 1u << (ignore[k] & 31);
    // (pageable source: the runtime has staged `bits` when the call returns)
    LT_HIP(hipMemcpyAsync(e->bitmap, bits, sizeof(bits), hipMemcpyHostToDevice, st));
  } else {
    a.n_ign = n_ignore;
    for (int k = 0; k < n_ignore; ++k) a.ign[k] = (unsigned short)ignore[k];
  }
  // laser parameters as laserscan.py:207-209 (python floats), rounded once to float32: the file points are float32
  const double fd = fov_down / 180.0 * M_PI, fu = fov_up / 180.0 * M_PI;
  const float pi_t = (float)M_PI, afd = (float)fabs(fd), fov = (float)(fabs(fd) + fabs(fu));
  if (a.n > 0)
    hipLaunchKernelGGL(k_src_project, dim3((a.n + 255) / 256), dim3(256), 0, st, a, (const unsigned*)e->bitmap, pi_t, afd, fov,
                       H, W, e->key, e->bad);
  hipLaunchKernelGGL(k_src_resolve, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a, H, W, color_lut, e->key,
                     e->bad, *out);
  LT_HIP(hipGetLastError());
  e->armed = true;  // k_src_resolve re-armed every cell it looked at
  return LT_OK;
}

extern "C" int lt_target_view_dev(lt_evaluator* e, const lt_raw_scan* scan, const int* ignore, int n_ignore, const double* T,
                                  const lt_view_model* vm, const float* color_lut, int lut_len, const lt_source_images* out,
                                  void* stream) {
  const unsigned model_bits = LT_PROJ_BEAM_ROWS | LT_PROJ_SECTOR | LT_PROJ_BEAM_AZIMUTH;
  if (!e || !scan || !vm || !out || scan->n < 0 || (scan->n > 0 && (!scan->xyzr || !scan->label)) ||
      ((uintptr_t)scan->xyzr & 15u) || n_ignore < 0 || (n_ignore > 0 && !ignore) || vm->H <= 0 || vm->W <= 0 ||
      (long long)vm->H * vm->W > 0x7fffffffLL - 4096 || (vm->flags & ~model_bits) || lut_len < 0 || (lut_len > 0 && !color_lut)) {
    lt_set_error("lt_target_view_dev: invalid argument (n=%d H=%d W=%d flags=%u n_ignore=%d lut_len=%d; xyzr must be 16-byte "
                 "aligned)", scan ? scan->n : -1, vm ? vm->H : -1, vm ? vm->W : -1, vm ? vm->flags : 0u, n_ignore, lut_len);
    return LT_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n_ignore; ++k)
    if (ignore[k] < 0 || ignore[k] > 65535) {
      lt_set_error("lt_target_view_dev: class %d is outside 0..65535 (labels are masked to 16 bits)", ignore[k]);
      return LT_ERR_INVALID_ARG;
    }
  const int H = vm->H, W = vm->W;
  const bool rows = (vm->flags & LT_PROJ_BEAM_ROWS) != 0, sector = (vm->flags & LT_PROJ_SECTOR) != 0;
  const bool azimuth = (vm->flags & LT_PROJ_BEAM_AZIMUTH) != 0;
  if (sector && !sector_ok("lt_target_view_dev", vm->yaw_center, vm->span)) return LT_ERR_INVALID_ARG;
  if (azimuth && !beam_azimuth_ok("lt_target_view_dev", vm->az_rad, H)) return LT_ERR_INVALID_ARG;
  // the model's doubles, laid out and held against the flags where the projections' are; no hard-coded beam angles
  const double sec[2] = {vm->yaw_center, vm->span};
  double tab[LT_MODEL_DOUBLES];
  const int n_tab = model_table("lt_target_view_dev", rows ? vm->rows : nullptr, rows ? H : 0,
                                vm->flags | LT_PROJ_NEW | LT_PROJ_REMOVE, vm->fov_up, vm->fov_down, H, sector ? sec : nullptr,
                                azimuth ? vm->az_rad : nullptr, H, tab);
  if (n_tab < 0) return LT_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(e->mu);
  LT_HIP(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t cells = (size_t)H * W;
  LT_CHECK(ev_reserve_key("lt_target_view_dev", e, cells, st));
  if (!e->model) LT_HIP(hipMalloc((void**)&e->model, LT_MODEL_DOUBLES * sizeof(double)));
  if (!e->armed) {  // first use, or the previous call failed half way
    LT_HIP(hipMemsetAsync(e->key, 0xFF, e->cap_cells * sizeof(unsigned long long), st));
    LT_HIP(hipMemsetAsync(e->bad, 0, sizeof(unsigned), st));
  }
  e->armed = false;
  if (n_tab > 0 && (n_tab != e->n_model || memcmp(e->model_host, tab, (size_t)n_tab * sizeof(double)) != 0)) {
    // read by the kernels of EARLIER calls on this stream: the copy is stream-ordered behind them; a pageable source is
    // staged by the runtime before the call returns.  A sequence's calls bring the same bytes and copy nothing.
    e->n_model = -1;
    memcpy(e->model_host, tab, (size_t)n_tab * sizeof(double));
    LT_HIP(hipMemcpyAsync(e->model, e->model_host, (size_t)n_tab * sizeof(double), hipMemcpyHostToDevice, st));
    e->n_model = n_tab;
  }
  SrcArgs a;
  memset(&a, 0, sizeof(a));
  a.xyzr = (const float4*)scan->xyzr;
  a.label = scan->label;
  a.n = scan->n;
  a.lut_len = lut_len;
  a.use_bitmap = n_ignore > LT_INGEST_LIST_ARGS;
  if (a.use_bitmap) {
    unsigned bits[LT_EV_BITMAP_WORDS];
    memset(bits, 0, sizeof(bits));
    for (int k = 0; k < n_ignore; ++k) bits[ignore[k] >> 5] |= 1u << (ignore[k] & 31);
    LT_HIP(hipMemcpyAsync(e->bitmap, bits, sizeof(bits), hipMemcpyHostToDevice, st));
  } else {
    a.n_ign = n_ignore;
    for (int k = 0; k < n_ignore; ++k) a.ign[k] = (unsigned short)ignore[k];
  }
  ViewXf xf;
  memset(&xf, 0, sizeof(xf));
  xf.on = T != nullptr;
  if (T) memcpy(xf.m, T, sizeof(xf.m));  // (the last row is not read)
  // laser parameters as lt_range_projection_batch_dev derives them for float64 clouds (laserscan.py:207-209, python floats)
  const double fd = vm->fov_down / 180.0 * M_PI, fu = vm->fov_up / 180.0 * M_PI;
  const double afd = fabs(fd), fov = fabs(fd) + fabs(fu);
  if (a.n > 0) {
#define LT_VIEW_PROJECT(B, S, AZ)                                                                                     \
  hipLaunchKernelGGL((k_view_project<B, S, AZ>), dim3((a.n + 255) / 256), dim3(256), 0, st, a, (const unsigned*)e->bitmap, \
                     xf, (double)M_PI, afd, fov, H, W, (const double*)e->model, e->key, e->bad)
    LT_FOR_MODEL(rows, sector, azimuth, LT_VIEW_PROJECT);
#undef LT_VIEW_PROJECT
  }
  hipLaunchKernelGGL(k_src_resolve, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a, H, W, color_lut, e->key,
                     e->bad, *out);
  LT_HIP(hipGetLastError());
  e->armed = true;  // k_src_resolve re-armed every cell it looked at
  return LT_OK;
}

extern "C" int lt_compare_record_dev(lt_evaluator* e, const int* src_label, const unsigned char* src_black,
                                     const int* tgt_label, const float* src_range, const float* tgt_range, int n,
                                     const unsigned* src_bad_labels, lt_compare_record* record, void* stream) {
  if (!e || !src_label || !src_black || !tgt_label || !src_range || !tgt_range || n <= 0 || !record) {
    lt_set_error("lt_compare_record_dev: invalid argument (n=%d)", n);
    return LT_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lock(e->mu);
  LT_HIP(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (n + 255) / 256;
  LT_CHECK(lt_dev_grow("lt_compare_record_dev", lt_wait_stream(st), &e->partial, &e->cap_blocks, (size_t)nb, (size_t)nb));
  if (++e->epoch == 0u) {  // 2^32 calls: the stamps start over
    LT_HIP(hipMemsetAsync(e->seen, 0, ((size_t)e->n_labels + 1) * sizeof(unsigned), st));
    e->epoch = 1u;
  }
  if (e->conf_dirty)
    LT_HIP(hipMemsetAsync(e->conf, 0, (size_t)e->n_labels * e->n_labels * sizeof(unsigned), st));
  e->conf_dirty = true;
  hipLaunchKernelGGL(k_cmp_pairs, dim3(nb), dim3(256), 0, st, src_label, src_black, tgt_label, src_range, tgt_range, n,
                     e->n_labels, e->epoch, e->conf, e->seen, e->partial);
  hipLaunchKernelGGL(k_cmp_record, dim3(LT_EV_RECORD_BLOCKS), dim3(256), 0, st, e->n_labels, e->epoch, e->conf,
                     (const unsigned*)e->seen, (const double*)e->partial, nb, n, src_bad_labels, e->rec);
  LT_HIP(hipGetLastError());
  e->conf_dirty = false;  // k_cmp_record zeroes every cell k_cmp_pairs touched
  // device memory or pinned host memory (lt_host_alloc): behind the kernels in stream order; the host reads the record
  // after an event it recorded behind this call
  LT_HIP(hipMemcpyAsync(record, e->rec, sizeof(lt_compare_record), hipMemcpyDefault, st));
  return LT_OK;
}
