// lt_ingest.hip -- from the bytes of velodyne/N.bin + labels/N.label to the clouds `deform` projects:
//   * MultiSemLaserScan.open_multiple_scans (auxiliary/laserscan.py:776-817): label & 0xFFFF (:588), apply_pose (:98-109),
//     remove_classes(moving) for every slot but the primary one, remove_classes(ignore) for every slot (:658-670, :802-807)
//   * the first statement of each deform branch (:845 / :878 / :949): apply_transformation(inv(poses[idx]))
// One thread per raw point over all slots of the call.  The boolean-mask copies of numpy become one STABLE stream
// compaction: kept points keep their file order, slots follow each other in slot order (np.concatenate, :939-945).
// Two kernels, no communication between workgroups inside a launch: k_ingest_count leaves one count per workgroup,
// k_ingest_write re-evaluates the predicate, sums the counts of the workgroups before it itself (a few thousand ints at
// 5 x 120 k points) and writes.  A dropped point writes one (0, 0, 0) point into the tail [n_kept, capacity) of its region,
// so that the projection can be launched on the capacity without the host ever learning n_kept (do_range_projection_new
// always removes depth-0 points, laserscan.py:307-309, and they sit behind every kept point).
//
// Arithmetic (the contract the tests pin bit for bit): x, y, z float32 -> float64 (exact), then TWO transforms, each row
// as ((m0*x + m1*y) + m2*z) + m3 with every product and sum rounded to float64 on its own -- no fused multiply-add (the
// library is built with -ffp-contract=off; the pragma below says it once more for this file), and no pre-multiplied
// matrix: the reference rounds the world coordinates to float64 before it applies the inverse pose.
#include "lt_internal.h"
#include <stdint.h>
#include <string.h>

#pragma clang fp contract(off)

#define LT_INGEST_BITMAP_WORDS 2048  // 65536 bits

namespace {

struct IngestSlot {
  const float4* xyzr;
  const unsigned* label;
  double* points;
  float* rem;
  unsigned* out_label;
  int n;         // raw points of the slot
  int blk0;      // first workgroup of the slot
  int reg_blk0;  // first workgroup of the slot's output region (merged: 0; per slot: blk0)
  int g0;        // index of the slot's first raw point inside its region
  int cap;       // capacity of the region (merged: sum of n; per slot: n)
  int pad;
};

struct IngestArgs {
  IngestSlot s[LT_INGEST_MAX_SCANS];
  double A[LT_INGEST_MAX_SCANS][12];  // rows 0..2 of poses[slot]
  double B[12];                       // rows 0..2 of `back`
  unsigned short ign[LT_INGEST_LIST_ARGS], mov[LT_INGEST_LIST_ARGS];
  int n_scans, n_ign, n_mov, use_bitmap, has_back, nblocks;
};

__device__ __forceinline__ int ingest_slot_of_block(const IngestArgs& a, int b) {
  int s = 0;
  while (s + 1 < a.n_scans && b >= a.s[s + 1].blk0) ++s;  // (an empty slot shares its blk0 with the next one: skipped)
  return s;
}

// rule 2: dropped if (slot != 0 and l in moving) or l in ignore
__device__ __forceinline__ bool ingest_dropped(const IngestArgs& a, const unsigned* __restrict__ bitmap, unsigned l, int s) {
  bool drop = false;
  if (a.use_bitmap) {
    drop = (bitmap[l >> 5] >> (l & 31u)) & 1u;
    if (s != 0) drop |= (bitmap[LT_INGEST_BITMAP_WORDS + (l >> 5)] >> (l & 31u)) & 1u;
  } else {
    for (int k = 0; k < a.n_ign; ++k) drop |= l == (unsigned)a.ign[k];
    if (s != 0)
      for (int k = 0; k < a.n_mov; ++k) drop |= l == (unsigned)a.mov[k];
  }
  return drop;
}

__global__ __launch_bounds__(256) void k_ingest_count(const IngestArgs a, const unsigned* __restrict__ bitmap,
                                                      int* __restrict__ blockcount) {
  __shared__ int wcnt[4];
  const int s = ingest_slot_of_block(a, blockIdx.x);
  const int i = ((int)blockIdx.x - a.s[s].blk0) * 256 + (int)threadIdx.x;
  const bool keep = i < a.s[s].n && !ingest_dropped(a, bitmap, a.s[s].label[i] & 0xFFFFu, s);
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blockcount[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

__device__ __forceinline__ double ingest_row(const double* __restrict__ m, double x, double y, double z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

__global__ __launch_bounds__(256) void k_ingest_write(const IngestArgs a, const unsigned* __restrict__ bitmap,
                                                      const int* __restrict__ blockcount, int* __restrict__ n_kept) {
  __shared__ int wcnt[4];
  __shared__ int red[3][4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = ingest_slot_of_block(a, b);
  const IngestSlot& sl = a.s[s];
  const int i = (b - sl.blk0) * 256 + (int)threadIdx.x;
  const bool inside = i < sl.n;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned l = 0u;
  if (inside) {
    l = sl.label[i] & 0xFFFFu;  // laserscan.py:588
    p = sl.xyzr[i];             // one 16-byte load
  }
  const bool keep = inside && !ingest_dropped(a, bitmap, l, s);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(m);
  // kept points of the workgroups before this one: in the call, in the region, in the slot
  int all = 0, reg = 0, slot = 0;
  for (int j = threadIdx.x; j < b; j += 256) {
    const int v = blockcount[j];
    all += v;
    if (j >= sl.reg_blk0) reg += v;
    if (j >= sl.blk0) slot += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    all += __shfl_xor(all, o, 64);
    reg += __shfl_xor(reg, o, 64);
    slot += __shfl_xor(slot, o, 64);
  }
  if (lane == 0) {
    red[0][wave] = all;
    red[1][wave] = reg;
    red[2][wave] = slot;
  }
  __syncthreads();
  const int own = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
  if (threadIdx.x == 0) {
    if (b == sl.blk0 + (sl.n + 255) / 256 - 1) n_kept[s] = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]) + own;
    if (b == a.nblocks - 1) n_kept[a.n_scans] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]) + own;
  }
  if (!inside) return;
  // kept points of the region before this thread
  int k = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]) + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) k += wcnt[w];
  if (keep) {
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    const double* A = a.A[s];
    double qx = ingest_row(A, x, y, z), qy = ingest_row(A + 4, x, y, z), qz = ingest_row(A + 8, x, y, z);  // apply_pose
    if (a.has_back) {  // apply_transformation(inv(poses[idx])) on the rounded world coordinates
      const double rx = ingest_row(a.B, qx, qy, qz), ry = ingest_row(a.B + 4, qx, qy, qz), rz = ingest_row(a.B + 8, qx, qy, qz);
      qx = rx, qy = ry, qz = rz;
    }
    double* o = sl.points + 3 * (size_t)k;
    o[0] = qx, o[1] = qy, o[2] = qz;
    sl.rem[k] = p.w;
    sl.out_label[k] = l;
  } else {
    // the d-th dropped point of the region fills cell cap - 1 - d of its tail: d = (raw points before) - (kept before)
    const int t = sl.cap - 1 - ((sl.g0 + i) - k);
    double* o = sl.points + 3 * (size_t)t;
    o[0] = 0.0, o[1] = 0.0, o[2] = 0.0;
    sl.rem[t] = 0.f;
    sl.out_label[t] = 0u;
  }
}

}  // namespace

extern "C" int lt_ingest_scans_dev(int n_scans, const lt_raw_scan* scans, const double* poses, const double* back,
                                   const int* ignore, int n_ignore, const int* moving, int n_moving, unsigned flags,
                                   const lt_ingest_out* out, int* n_kept, int* work, void* stream) {
  if (n_scans < 1 || n_scans > LT_INGEST_MAX_SCANS || !scans || !poses || !out || !n_kept || !work || n_ignore < 0 ||
      n_moving < 0 || (n_ignore > 0 && !ignore) || (n_moving > 0 && !moving) || (flags & ~LT_INGEST_MERGED)) {
    lt_set_error("lt_ingest_scans_dev: invalid argument (n_scans=%d: 1..%d)", n_scans, LT_INGEST_MAX_SCANS);
    return LT_ERR_INVALID_ARG;
  }
  for (int pass = 0; pass < 2; ++pass) {
    const int* list = pass ? moving : ignore;
    for (int k = 0; k < (pass ? n_moving : n_ignore); ++k)
      if (list[k] < 0 || list[k] > 65535) {
        lt_set_error("lt_ingest_scans_dev: class %d is outside 0..65535 (labels are masked to 16 bits)", list[k]);
        return LT_ERR_INVALID_ARG;
      }
  }
  const bool merged = (flags & LT_INGEST_MERGED) != 0;
  IngestArgs a;
  memset(&a, 0, sizeof(a));
  long long total = 0;
  int nblocks = 0;
  for (int i = 0; i < n_scans; ++i) {
    const lt_ingest_out& o = out[merged ? 0 : i];
    const int n = scans[i].n;
    if (n < 0 || (n > 0 && (!scans[i].xyzr || !scans[i].label || !o.points || !o.rem || !o.label)) ||
        ((uintptr_t)scans[i].xyzr & 15u)) {
      lt_set_error("lt_ingest_scans_dev: slot %d: invalid argument (n=%d; xyzr must be 16-byte aligned)", i, n);
      return LT_ERR_INVALID_ARG;
    }
    IngestSlot& s = a.s[i];
    s.xyzr = (const float4*)scans[i].xyzr;
    s.label = scans[i].label;
    s.points = o.points, s.rem = o.rem, s.out_label = o.label;
    s.n = n;
    s.blk0 = nblocks;
    s.reg_blk0 = merged ? 0 : nblocks;
    s.g0 = merged ? (int)total : 0;
    total += n;
    nblocks += (n + 255) / 256;
    for (int r = 0; r < 12; ++r) a.A[i][r] = poses[16 * (size_t)i + r];
  }
  if (total > 0x7fffffffLL - 4096) {
    lt_set_error("lt_ingest_scans_dev: %lld points in one call", total);
    return LT_ERR_TOO_LARGE;
  }
  for (int i = 0; i < n_scans; ++i) a.s[i].cap = merged ? (int)total : a.s[i].n;
  a.n_scans = n_scans;
  a.nblocks = nblocks;
  a.has_back = back != nullptr;
  if (back)
    for (int r = 0; r < 12; ++r) a.B[r] = back[r];
  if (n_scans == 1) n_moving = 0;  // a single scan is the primary one (laserscan.py:809-817)
  hipStream_t st = (hipStream_t)stream;
  LT_HIP(hipMemsetAsync(n_kept, 0, ((size_t)n_scans + 1) * sizeof(int), st));  // (empty slots, an empty call)
  if (nblocks == 0) return LT_OK;
  unsigned* bitmap = (unsigned*)work;
  int* blockcount = work + 2 * LT_INGEST_BITMAP_WORDS;
  a.use_bitmap = n_ignore > LT_INGEST_LIST_ARGS || n_moving > LT_INGEST_LIST_ARGS;
  if (a.use_bitmap) {
    unsigned bits[2 * LT_INGEST_BITMAP_WORDS];
    memset(bits, 0, sizeof(bits));
    for (int k = 0; k < n_ignore; ++k) bits[ignore[k] >> 5] |= 1u << (ignore[k] & 31);
    for (int k = 0; k < n_moving; ++k) bits[LT_INGEST_BITMAP_WORDS + (moving[k] >> 5)] |= 1u << (moving[k] & 31);
    // (pageable source: the runtime has staged `bits` when the call returns)
    LT_HIP(hipMemcpyAsync(bitmap, bits, sizeof(bits), hipMemcpyHostToDevice, st));
  } else {
    a.n_ign = n_ignore, a.n_mov = n_moving;
    for (int k = 0; k < n_ignore; ++k) a.ign[k] = (unsigned short)ignore[k];
    for (int k = 0; k < n_moving; ++k) a.mov[k] = (unsigned short)moving[k];
  }
  hipLaunchKernelGGL(k_ingest_count, dim3(nblocks), dim3(256), 0, st, a, (const unsigned*)bitmap, blockcount);
  hipLaunchKernelGGL(k_ingest_write, dim3(nblocks), dim3(256), 0, st, a, (const unsigned*)bitmap, (const int*)blockcount,
                     n_kept);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
