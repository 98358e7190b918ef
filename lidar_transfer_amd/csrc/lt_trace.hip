// lt_trace.hip -- closest-hit ray cast on gfx950 (replaces the OpenMP ray loop of the reference,
// auxiliary/raytracer/RayTracer.cpp:62-92, with BVH::getIntersection BVH.cpp:19-110,
// Triangle::getIntersection Triangle.h:27-50, normalize Vector3.h:73-89, Ray Ray.h:11-12).
//
// Three kernels over one set of pieces (ray, tile cell, triangle test, write-back, counter reduction):
//   k_trace        binary nodes, one ray per lane: the A/B twin behind LIDARHIP_TRACE=binary
//   k_trace4       4-wide nodes, four lanes per ray: the LBVH strategy's ray cast
//   k_trace4_tail  one wave per ray that k_trace4 handed over
//
// Float arithmetic of the triangle test, the normalisation and the write-back is the reference's,
// operation by operation; the file is compiled with -ffp-contract=off and IEEE division / sqrt.
// The closest hit is the minimum over (t, face index), independent of traversal order.
#include "lt_internal.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "lt_scanimg.h"
#include "lt_normalize.h"  // the reference's RSQRTSS seed, replayed (Intel / AMD table) or exact

#define LT_DONE ((int)0x80000000)
#define LT_NO_FACE 0x7fffffff  // best face of a ray that has hit nothing; reference of a child slot that does not exist
#define LT_TILE_H 4
#define LT_TILE_W 16

// =====================================================================================================
// What the kernels are told, as three PODs by value (helpers: by const reference), built once per call
// by lt_trace_launch: the two below and the images of the call, an lt_scan_images (a null member: not wanted).
// The spill area, the counters, the step cap and tail_args stay arguments of their own.
// =====================================================================================================
struct trace_scene {    // the mesh and its tree
  const float4* nodes;  // binary nodes (k_trace) or 4-wide nodes (k_trace4, k_trace4_tail)
  const float4* tris;   // sorted triangle records
  const int* faces;
  const int* colors;
  const float* rem;
  int n_faces;
};
struct trace_cast {  // one call: the rays and the image they form
  const float* rays;
  float ox, oy, oz;
  int H, W;
  unsigned flags;
};

// A ray as the kernels use it: origin, normalised direction, inverse direction (Ray.h:12, +-inf allowed).
struct trace_ray {
  float ox, oy, oz, dx, dy, dz, ix, iy, iz;
  // A direction or origin with a NaN can never be accepted by the triangle test (every product chain reaches
  // t as NaN, and BVH.cpp:59 keeps a hit only if t < best): such rays are misses without a traversal.
  bool finite;
};

// ray `ray` of the call, direction normalised like Vector3.h:73-89: D = (x^2 + y^2) + z^2, r0 ~ 1/sqrt(D), one
// Newton-Raphson step.  A lane without a ray (`active` false) reads nothing and gets the direction (0, 0, 1).
__device__ __forceinline__ trace_ray trace_ray_of(const trace_cast& c, size_t ray, bool active) {
  trace_ray r;
  r.ox = c.ox; r.oy = c.oy; r.oz = c.oz;
  r.dx = 0.f; r.dy = 0.f; r.dz = 1.f;
  if (active) {
    const float rx = c.rays[3 * ray], ry = c.rays[3 * ray + 1], rz = c.rays[3 * ray + 2];
    const float D = (rx * rx + ry * ry) + rz * rz;
    const float r0 = lt_rsqrt_seed(D, c.flags);
    const float s = (1.5f * r0) + (((D * -0.5f) * r0) * (r0 * r0));
    r.dx = rx * s; r.dy = ry * s; r.dz = rz * s;
  }
  r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
  r.finite = (r.dx == r.dx) && (r.dy == r.dy) && (r.dz == r.dz) && (r.ox == r.ox) && (r.oy == r.oy) && (r.oz == r.oz);
  return r;
}

// The cell of the range image that slot `slot` of wave `wave` of this workgroup works on.  A wave owns a TILE_H x TILE_W
// (beam x azimuth) tile so that its rays walk almost the same nodes.  XCD-aware tile assignment: workgroup b runs on
// XCD b % 8 (private 4 MiB L2); give XCD x the x-th eighth of the (column-major) tile list, i.e. one contiguous azimuth
// sector.  gridDim.x is a multiple of 8 (trace_grid).
struct tile_cell {
  int h, w;
  bool active;  // the cell exists
  size_t ray;   // h * W + w
};
template <int TILE_H, int TILE_W>
__device__ __forceinline__ tile_cell trace_cell(int wave, int slot, int H, int W) {
  const int nb = gridDim.x;
  const int lb = (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3);
  const int tiles_h = (H + TILE_H - 1) / TILE_H, tiles_w = (W + TILE_W - 1) / TILE_W;
  const int wt = lb * 4 + wave;
  const int tile_x = wt / tiles_h, tile_y = wt - tile_x * tiles_h;
  tile_cell c;
  c.h = tile_y * TILE_H + slot / TILE_W;
  c.w = tile_x * TILE_W + slot % TILE_W;
  c.active = tile_x < tiles_w && c.h < H && c.w < W;
  c.ray = (size_t)c.h * W + c.w;
  return c;
}

// (t, face) <- the smaller of it and (ot, of): the order every kernel keeps its best hit by
__device__ __forceinline__ void take_closer(float& t, int& f, float ot, int of) {
  if (ot < t || (ot == t && of < f)) { t = ot; f = of; }
}

// triangles of a leaf reference (< 0, not LT_DONE): `cnt` (1 .. 4) sorted triangle records from `start`
__device__ __forceinline__ void leaf_range(int ref, int& start, int& cnt) {
  const int lref = ~ref;
  start = lref & 0x0fffffff;
  cnt = (lref >> 28) + 1;
}

// Moller-Trumbore with the reference's operation order (Triangle.h:27-50) on a sorted triangle record; returns t
// (INFINITY = no hit) and the face index
__device__ __forceinline__ float trace_tri(const float4* __restrict__ T, const trace_ray& r, int& face) {
  const float eps = 0.000001f;  // Triangle.h:32
  const float4 t0 = T[0], t1 = T[1], t2 = T[2];
  const float e1x = t0.w, e1y = t1.x, e1z = t1.y, e2x = t1.z, e2y = t1.w, e2z = t2.x;
  const float hx = r.dy * e2z - r.dz * e2y, hy = r.dz * e2x - r.dx * e2z, hz = r.dx * e2y - r.dy * e2x;
  const float aa = (e1x * hx + e1y * hy) + e1z * hz;
  face = LT_NO_FACE;
  if (aa < eps && aa > -eps) return INFINITY;
  const float inv_a = lt_rcp_ieee(aa);  // = 1.0f / aa, bit for bit (lt_internal.h)
  const float sx = r.ox - t0.x, sy = r.oy - t0.y, sz = r.oz - t0.z;
  const float u = ((sx * hx + sy * hy) + sz * hz) * inv_a;
  if (u < 0 || u > 1) return INFINITY;
  const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
  const float v = ((r.dx * qx + r.dy * qy) + r.dz * qz) * inv_a;
  if (v < 0 || u + v > 1) return INFINITY;
  const float tt = ((e2x * qx + e2y * qy) + e2z * qz) * inv_a;
  if (tt < eps || !(tt == tt)) return INFINITY;  // NaN t is never recorded by the reference either (BVH.cpp:59)
  face = __float_as_int(t2.y);
  return tt;
}

// write-back of one ray (RayTracer.cpp:73-90); misses are written only with LT_TRACE_WRITE_MISSES
__device__ __forceinline__ void trace_writeback(size_t ray, float best_t, int best_face, const trace_ray& r,
                                                const trace_scene& sc, unsigned flags, const lt_scan_images& o) {
  const bool label = (flags & LT_TRACE_LABEL_IMAGE) != 0;
  if (best_face != LT_NO_FACE)
    lt_scan_write_hit(o, ray, label, best_t, best_face, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, sc.faces, sc.colors, sc.rem);
  else if (flags & LT_TRACE_WRITE_MISSES)
    lt_scan_write_miss(o, ray, label);
}

// LT_TRACE_COUNT: the four per-lane tallies summed over the wave into counters[0 .. 3] (nodes, triangle tests, hits,
// stack entries spilled), one atomic each per wave.  The wave stamps of the kernels follow at counters[8 + ...].
__device__ __forceinline__ void trace_count_reduce(unsigned long long* counters, int lane, unsigned n_nodes,
                                                   unsigned n_tris, bool hit, unsigned n_ovf) {
  unsigned long long vn = n_nodes, vt = n_tris, vh = hit ? 1u : 0u, vo = n_ovf;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    vn += __shfl_xor(vn, o, 64);
    vt += __shfl_xor(vt, o, 64);
    vh += __shfl_xor(vh, o, 64);
    vo += __shfl_xor(vo, o, 64);
  }
  if (lane == 0) {
    atomicAdd(&counters[0], vn);
    atomicAdd(&counters[1], vt);
    atomicAdd(&counters[2], vh);
    atomicAdd(&counters[3], vo);
  }
}

// =====================================================================================================
// Binary traversal: ONE RAY PER LANE.
//
// A wave owns a 4 x 16 tile of the range image (trace_cell).  Traversal is "while-while": lanes descend internal
// nodes until every lane of the wave holds a leaf, then the leaves are intersected.  The per-ray stack of deferred
// children lives in LDS ([depth][lane] layout: bank = lane, conflict-free); entries beyond
// LT_STACK_LDS spill to HBM (never observed on real scenes, kept for adversarial inputs: tests/test_lbvh_paths_gpu.py
// drives the spill, the hand-over and the tail of both kernels on the scenes of tests/lbvh_cases.py).
// =====================================================================================================

// next reference of a lane of k_trace: the top of its stack (`lds`: entry 0 of the lane, `spill`: its entries from
// LT_STACK_LDS on), or LT_DONE when the stack is empty
__device__ __forceinline__ int bin_pop(const int* lds, const int* spill, int& sp) {
  if (sp == 0) return LT_DONE;
  --sp;
  return sp < LT_STACK_LDS ? lds[64 * sp] : spill[sp - LT_STACK_LDS];
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_trace(trace_scene scene, trace_cast cast, lt_scan_images out,
                                               int* __restrict__ overflow, unsigned long long* __restrict__ counters) {
  __shared__ int stack[4][LT_STACK_LDS][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long t_start = COUNT ? (unsigned long long)clock64() : 0ull;
  const tile_cell c = trace_cell<LT_TILE_H, LT_TILE_W>(wave, lane, cast.H, cast.W);
  const trace_ray r = trace_ray_of(cast, c.ray, c.active);

  float best_t = 999999999.f;  // BVH.cpp:20
  int best_face = LT_NO_FACE;
  int sp = 0;
  int* const lds = &stack[wave][0][lane];
  int* const spill = overflow + c.ray * (LT_STACK_MAX - LT_STACK_LDS);
  int cur = (c.active && scene.n_faces > 0 && r.finite) ? 0 : LT_DONE;
  unsigned n_nodes = 0, n_tris = 0, n_ovf = 0;

  while (true) {
    // ---- descend ------------------------------------------------------------------------------
    while (cur >= 0) {
      const float4* N = scene.nodes + 4 * (size_t)cur;
      const float4 q0 = N[0], q1 = N[1], q2 = N[2], q3 = N[3];
      if (COUNT) ++n_nodes;
      const float a0x = (q0.x - r.ox) * r.ix, b0x = (q0.w - r.ox) * r.ix;
      const float a0y = (q0.y - r.oy) * r.iy, b0y = (q1.x - r.oy) * r.iy;
      const float a0z = (q0.z - r.oz) * r.iz, b0z = (q1.y - r.oz) * r.iz;
      const float a1x = (q1.z - r.ox) * r.ix, b1x = (q2.y - r.ox) * r.ix;
      const float a1y = (q1.w - r.oy) * r.iy, b1y = (q2.z - r.oy) * r.iy;
      const float a1z = (q2.x - r.oz) * r.iz, b1z = (q2.w - r.oz) * r.iz;
      const float tn0 = fmaxf(fmaxf(fminf(a0x, b0x), fminf(a0y, b0y)), fmaxf(fminf(a0z, b0z), 0.0f));
      const float tf0 = fminf(fminf(fmaxf(a0x, b0x), fmaxf(a0y, b0y)), fminf(fmaxf(a0z, b0z), best_t));
      const float tn1 = fmaxf(fmaxf(fminf(a1x, b1x), fminf(a1y, b1y)), fmaxf(fminf(a1z, b1z), 0.0f));
      const float tf1 = fminf(fminf(fmaxf(a1x, b1x), fmaxf(a1y, b1y)), fminf(fmaxf(a1z, b1z), best_t));
      const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
      const int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y);
      if (h0 && h1) {
        const bool swap = tn1 < tn0;
        const int farc = swap ? c0 : c1;
        cur = swap ? c1 : c0;
        if (sp < LT_STACK_LDS) {
          lds[64 * sp] = farc;
        } else {
          spill[sp - LT_STACK_LDS] = farc;
          if (COUNT) ++n_ovf;
        }
        ++sp;
      } else if (h0) {
        cur = c0;
      } else if (h1) {
        cur = c1;
      } else {
        cur = bin_pop(lds, spill, sp);
      }
    }
    if (cur == LT_DONE) break;
    // ---- leaf: every triangle of it, one after the other -------------------------------------------
    int start, cnt;
    leaf_range(cur, start, cnt);
    for (int k = 0; k < cnt; ++k) {
      int f;
      const float t = trace_tri(scene.tris + 3 * (size_t)(start + k), r, f);
      if (COUNT) ++n_tris;
      take_closer(best_t, best_face, t, f);
    }
    cur = bin_pop(lds, spill, sp);
  }

  if (c.active) trace_writeback(c.ray, best_t, best_face, r, scene, cast.flags, out);
  if (COUNT) {
    trace_count_reduce(counters, lane, n_nodes, n_tris, c.active && best_face != LT_NO_FACE, n_ovf);
    const int wg = blockIdx.x * 4 + wave;  // debug: wave start / end clock (tools/wave_times.py)
    if (lane == 0 && wg < LT_DBG_WAVES) {
      counters[8 + 2 * wg] = t_start;
      counters[8 + 2 * wg + 1] = (unsigned long long)clock64();
    }
  }
}

// =====================================================================================================
// Quad traversal over the 4-wide nodes: FOUR LANES PER RAY.
//
// A 64x2048 scan is only 131 072 rays = 2 waves per SIMD with one ray per lane: far too few to hide the
// ~1 us dependent node fetch of a pointer-chasing traversal on 256 CUs.  Spreading a ray over a quad of
// lanes gives 8 waves per SIMD (full occupancy), halves the number of dependent steps (4-wide nodes), and
// turns the leaf loop into one step:
//   * node step: the quad reads one 128-B node as a single cache line, lane j tests child j; hits are
//     ranked by entry distance with DPP quad broadcasts; the nearest becomes the next node, the others
//     are pushed so that the nearer one is popped first;
//   * leaf step: lane j runs Moller-Trumbore on triangle j of the leaf (<= 4), then a quad min over
//     (t, face index).
// The per-ray stack is shared by the quad: LDS [depth][16 rays], spill to HBM beyond LT_STACK4_LDS.
//
// What bounds the kernel is the LONGEST walk, not the sum of the walks: a step is a dependent chain of ~0.9 us
// (node line from L2 / Infinity Cache + ~100 dependent VALU / DPP / LDS instructions), the mean ray needs 30 steps
// and the worst one 148 -- per-wave wall-clock stamps (tools/wave_times.py --quad) showed 99 % of the waves gone
// after 71 us of a 123 us launch, the chip 25 % busy over the span.  Two measures (C2: 125 -> 68 + 19 us):
//   * ONE loop whose trips are node OR leaf steps, so that a wave needs max-over-quads trips (the nested form made
//     a quad at a leaf wait for every other quad's run of node steps: 110 trips for the slowest wave although no
//     quad took more than 48 steps);
//   * hand-over: a ray that is not done after `step_cap` steps (LT_TRACE4_STEP_CAP = 40: 6 % of the rays on C2) parks
//     its state -- its stack plus the reference it was about to visit, best (t, face) -- in a queue, compacted
//     across the wave with one ballot-counted atomic per wave, and k_trace4_tail walks each such ray with a WHOLE
//     WAVE: the 16 quads pop 16 stack entries at a time and share best (t, face) through an LDS atomic, so the
//     remaining ~100 dependent steps of the worst ray become ~10.
// Results do not depend on the traversal order (min over (t, face), children are culled only when their entry
// distance exceeds the best t), so both kernels are bit-identical to k_trace and to the brute-force oracle.
// =====================================================================================================
#define LT_Q_BCAST(k) ((k) | ((k) << 2) | ((k) << 4) | ((k) << 6))
#define LT_Q_XOR1 0xB1  // quad_perm [1,0,3,2]
#define LT_Q_XOR2 0x4E  // quad_perm [2,3,0,1]

// (mov_dpp = update_dpp with an UNDEFINED old value: every source lane of a quad permutation exists, so nothing is kept
// from it -- with old = 0 the compiler set the destination to 0 before each of the ten permutations of a node step,
// 10 % of the vector instructions on the dependent chain of every node step)
template <int CTRL>
__device__ __forceinline__ int qperm_i(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float qperm_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}

// rays of a wave: a LT_TILE4_H x LT_TILE4_W tile of the image (16 rays).  k_trace4 on C2 (tools/tile_ab.sh): 2 x 8 60.3 us,
// 1 x 16 61.9, 4 x 4 57.0, 8 x 2 56.9 -- a beam step is 2.5 azimuth steps there, 4 x 4 is the most compact in angle
#ifndef LT_TILE4_H
#define LT_TILE4_H 4
#define LT_TILE4_W 4
#endif

// slab test of child j of a 4-wide node against the ray; hit iff the child exists and tn <= min(tfar, best_t)
__device__ __forceinline__ int trace_slab(const float4 a, const float4 b, const trace_ray& r, float best_t, float& tn,
                                          int& ref) {
  const float l1x = (a.x - r.ox) * r.ix, l2x = (a.w - r.ox) * r.ix;
  const float l1y = (a.y - r.oy) * r.iy, l2y = (b.x - r.oy) * r.iy;
  const float l1z = (a.z - r.oz) * r.iz, l2z = (b.y - r.oz) * r.iz;
  tn = fmaxf(fmaxf(fminf(l1x, l2x), fminf(l1y, l2y)), fmaxf(fminf(l1z, l2z), 0.0f));
  const float tf = fminf(fminf(fmaxf(l1x, l2x), fmaxf(l1y, l2y)), fminf(fmaxf(l1z, l2z), best_t));
  ref = __float_as_int(b.z);
  // an unused child slot (box +inf, ref LT_NO_FACE) fails the slab test of every finite ray, but fminf /
  // fmaxf drop NaN operands, so a ray or origin with a NaN would "hit" it: exclude it explicitly
  return (tn <= tf && ref != LT_NO_FACE) ? 1 : 0;
}

// rank of this lane's child among the hit children of its quad: by (tn, lane) packed into one unsigned key -- tn >= 0, so
// its bits order like its value; the two mantissa bits given to the lane only perturb the ORDER of near-equal
// children, which the result does not depend on; a child that is not hit has the largest key and is never counted
struct quad_ranked {
  int rank;                 // hit children of the quad that come before this one
  int nh;                   // hit children of the quad
  unsigned long long hits;  // the hit ballot of the wave
};
__device__ __forceinline__ quad_ranked quad_rank(int hit, float tn, int lane) {
  const unsigned key = hit ? ((__float_as_uint(tn) & ~3u) | (unsigned)(lane & 3)) : 0xFFFFFFFFu;
  const unsigned k0 = (unsigned)qperm_i<LT_Q_BCAST(0)>((int)key), k1 = (unsigned)qperm_i<LT_Q_BCAST(1)>((int)key);
  const unsigned k2 = (unsigned)qperm_i<LT_Q_BCAST(2)>((int)key), k3 = (unsigned)qperm_i<LT_Q_BCAST(3)>((int)key);
  quad_ranked k;
  k.rank = (int)(k0 < key) + (int)(k1 < key) + (int)(k2 < key) + (int)(k3 < key);
  k.hits = __ballot(hit != 0);
  k.nh = __popc((unsigned)(k.hits >> (lane & ~3)) & 15u);
  return k;
}

// quad min over (t, face): every lane of the quad leaves with the quad's closest hit
__device__ __forceinline__ void quad_min_hit(float& t, int& f) {
  take_closer(t, f, qperm_f<LT_Q_XOR1>(t), qperm_i<LT_Q_XOR1>(f));
  take_closer(t, f, qperm_f<LT_Q_XOR2>(t), qperm_i<LT_Q_XOR2>(f));
}

// The stack of one quad's ray in k_trace4: entry s in LDS below LT_STACK4_LDS, in the spill area above.
// sp is uniform within the quad.
struct quad_stack {
  int (*lds)[16];  // this quad's column of the wave's LDS stacks [depth][16 rays]: entry s at lds[s][0]
  int* spill;      // entry LT_STACK4_LDS of this quad's ray
  int sp;
};

// push of the hit children of a node step but the nearest (rank 0, which the walk goes on with): rank 1 ends on top of the
// stack.  Called by every lane of the quad; -> 1 if this lane's child went to the spill area
__device__ __forceinline__ int quad_push(quad_stack& st, bool hit, const quad_ranked& k, int ref) {
  int spilled = 0;
  if (hit && k.rank > 0) {
    const int slot = st.sp + (k.nh - 1 - k.rank);
    if (slot < LT_STACK4_LDS) {
      st.lds[slot][0] = ref;
    } else {
      st.spill[slot - LT_STACK4_LDS] = ref;
      spilled = 1;
    }
  }
  st.sp += k.nh - 1;
  return spilled;
}

// next reference to visit: the top of the stack, or LT_DONE when it is empty.  (Written as a select of the LDS and the
// spilled entry, the compiler loads through a FLAT pointer chosen per lane: an LDS read always, the global one in a branch
// almost never taken.)
__device__ __forceinline__ int quad_pop(quad_stack& st) {
  int v = LT_DONE;
  if (st.sp > 0) {
    --st.sp;
    typedef __attribute__((address_space(3))) int lds_int;  // (volatile LDS access: not to be merged with the other load)
    v = *(volatile lds_int*)(lds_int*)&st.lds[min(st.sp, LT_STACK4_LDS - 1)][0];
    if (st.sp >= LT_STACK4_LDS) v = st.spill[st.sp - LT_STACK4_LDS];
  }
  return v;
}

// the walk of one quad's ray; everything in it is uniform within the quad
struct quad_walk {
  int cur;  // reference to visit next: >= 0 a node, < 0 a leaf, LT_DONE nothing
  float best_t;
  int best_face;
  quad_stack st;
};
struct trace_tally {  // LT_TRACE_COUNT, per lane
  unsigned nodes, tris, ovf;
};

// node step: lane j of the quad (= lane & 3) tests child j; the walk goes on with the nearest hit child, the others are pushed
template <bool COUNT>
__device__ __forceinline__ void node_step(const trace_scene& scene, const trace_ray& r, int lane, int j, quad_walk& wk,
                                          trace_tally& n) {
  const float4* N = scene.nodes + 8 * (size_t)wk.cur + 2 * j;
  const float4 a = N[0], b = N[1];
  if (COUNT && j == 0) ++n.nodes;
  float tn;
  int ref;
  const int hit = trace_slab(a, b, r, wk.best_t, tn, ref);
  const quad_ranked k = quad_rank(hit, tn, lane);
  if (k.nh == 0) {
    wk.cur = quad_pop(wk.st);
  } else {
    // nearest child -> next node (OR-reduce the single rank-0 reference over the quad)
    int nxt = (hit && k.rank == 0) ? ref : 0;
    nxt |= qperm_i<LT_Q_XOR1>(nxt);
    nxt |= qperm_i<LT_Q_XOR2>(nxt);
    const int spilled = quad_push(wk.st, hit != 0, k, ref);
    if (COUNT) n.ovf += spilled;
    wk.cur = nxt;
  }
}

// leaf step: one triangle per lane (Triangle.h:27-50 operation order), quad min, then the next reference from the stack
template <bool COUNT>
__device__ __forceinline__ void leaf_step(const trace_scene& scene, const trace_ray& r, int lane, int j, quad_walk& wk,
                                          trace_tally& n) {
  int start, cnt;
  leaf_range(wk.cur, start, cnt);
  float t = INFINITY;
  int f = LT_NO_FACE;
  if (j < cnt) {
    t = trace_tri(scene.tris + 3 * (size_t)(start + j), r, f);
    if (COUNT) ++n.tris;
  }
  quad_min_hit(t, f);
  take_closer(wk.best_t, wk.best_face, t, f);
  wk.cur = quad_pop(wk.st);
}

struct tail_args {  // hand-over area of a launch (lt_internal.h: lt_scene::tail_*)
  int* stack; float4* meta; int* queue;
  int* count;       // rays parked by this launch (starts at 0)
  int* count_next;  // the counter of the scene's NEXT launch: k_trace4_tail zeroes it (no memset between launches)
};

// hand-over of the rays that hit the step cap (`handed_over`: wk.cur is the node / leaf reference still to be visited):
// compaction across the wave (one atomic per wave); the quad saves its stack, LDS part and spilled part, with wk.cur on
// top, its best (t, face) and its ray for k_trace4_tail.  Called by every lane of the wave.
__device__ __forceinline__ void park_ray(const tail_args& tail, const quad_walk& wk, size_t ray, bool handed_over,
                                         int lane, int j) {
  const unsigned long long m = __ballot(handed_over && j == 0);
  if (m) {  // wave-uniform
    int base = 0;
    if (lane == 0) base = atomicAdd(tail.count, __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (handed_over) {
      const int slot = base + __popcll(m & ((1ull << (lane & ~3)) - 1ull));  // rank of this quad among the parked ones
      const int sp = wk.st.sp;
      int* dst = tail.stack + (size_t)slot * LT_TAIL_SAVE;
      for (int i = j; i < sp; i += 4) dst[i] = i < LT_STACK4_LDS ? wk.st.lds[i][0] : wk.st.spill[i - LT_STACK4_LDS];
      if (j == 0) {
        dst[sp] = wk.cur;  // the reference it was about to visit goes on top
        tail.meta[slot] = make_float4(wk.best_t, __int_as_float(wk.best_face), __int_as_float(sp + 1), 0.f);
        tail.queue[slot] = (int)ray;
      }
    }
  }
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_trace4(trace_scene scene, trace_cast cast, lt_scan_images out,
                                                int* __restrict__ overflow, unsigned long long* __restrict__ counters,
                                                int step_cap, tail_args tail) {
  __shared__ int stack[4][LT_STACK4_LDS][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 3, q = lane >> 2;
  const bool dbg_times = COUNT || (cast.flags & LT_TRACE_DEBUG_TIMES);
  const unsigned long long t_start = dbg_times ? (unsigned long long)wall_clock64() : 0ull;  // 100 MHz
  const tile_cell c = trace_cell<LT_TILE4_H, LT_TILE4_W>(wave, q, cast.H, cast.W);
  const trace_ray r = trace_ray_of(cast, c.ray, c.active);

  quad_walk wk;
  wk.cur = (c.active && scene.n_faces > 0 && r.finite) ? 0 : LT_DONE;
  wk.best_t = 999999999.f;  // BVH.cpp:20
  wk.best_face = LT_NO_FACE;
  wk.st.lds = (int (*)[16])&stack[wave][0][q];
  wk.st.spill = overflow + c.ray * (LT_STACK4_MAX - LT_STACK4_LDS);
  wk.st.sp = 0;
  trace_tally n = {0, 0, 0};
  int n_steps = 0;  // node + leaf steps of this quad's ray

  // ONE loop whose trips are steps of either kind ("if-if" traversal): a wave needs max-over-its-quads trips.  The
  // nested form (inner loop over nodes, leaf step outside) makes a quad that has reached a leaf wait for every other
  // quad's run of node steps and the other way round: measured 110 trips for the slowest wave although no quad took
  // more than 48 steps.  (wk, n_steps are uniform within a quad.)
  while (wk.cur != LT_DONE && n_steps < step_cap) {
    ++n_steps;
    if (wk.cur >= 0) node_step<COUNT>(scene, r, lane, j, wk, n);
    else leaf_step<COUNT>(scene, r, lane, j, wk, n);
  }
  const bool handed_over = wk.cur != LT_DONE;  // left by the step cap: the ray goes on in k_trace4_tail
  park_ray(tail, wk, c.ray, handed_over, lane, j);

  // ---- write-back by lane 0 of the quad -----------------------------------------------------------------------
  if ((cast.flags & LT_TRACE_DEBUG_STEPS) && out.tri) {  // debug: steps per ray instead of the face (cap off)
    if (c.active && j == 0) out.tri[c.ray] = n_steps;
  } else if (c.active && j == 0 && !handed_over) {
    trace_writeback(c.ray, wk.best_t, wk.best_face, r, scene, cast.flags, out);
  }
  if (COUNT) trace_count_reduce(counters, lane, n.nodes, n.tris, c.active && wk.best_face != LT_NO_FACE && j == 0, n.ovf);
  if (dbg_times && lane == 0) {  // debug (tools/wave_times.py --quad): start / duration at 100 MHz, steps of quad 0
    const int wg = blockIdx.x * 4 + wave;
    if (wg < LT_DBG_WAVES) {
      counters[8 + 2 * wg] = t_start;
      counters[8 + 2 * wg + 1] = ((unsigned long long)wall_clock64() - t_start) | ((unsigned long long)n_steps << 32);
    }
  }
}

// One WAVE per handed-over ray: the 16 quads pop up to 16 entries of the ray's stack at a time (LT_TAIL_DFS: one at a
// time while the stack is very full), every quad visits its node (lane j tests child j against the shared best t) or
// its leaf (lane j tests triangle j; quad minimum into the shared best (t, face) with one 64-bit LDS atomic), the hit
// children of all quads are pushed with a wave prefix sum.  Workgroup = one wave, so __syncthreads() is a wave barrier.
//
// This kernel keeps positional arguments at its boundary and builds the three structs in its first lines: a wave reads its
// ray, and lane 0 the face, colour and remission of the hit, at wave-uniform addresses, and only through a
// `const __restrict__` kernel argument is that a scalar load (a pointer inside a by-value struct cannot say that no store
// of the kernel reaches it: vector loads + readfirstlane).  profiles/trace_pieces/README.md.
__global__ __launch_bounds__(64) void k_trace4_tail(const float4* __restrict__ nodes4, const float4* __restrict__ tris,
                                                    const float* __restrict__ rays, float ox, float oy, float oz,
                                                    const int* __restrict__ faces, const int* __restrict__ colors,
                                                    const float* __restrict__ rem, float* __restrict__ endpoints,
                                                    int* __restrict__ endcolors, float* __restrict__ range,
                                                    float* __restrict__ endrem, int* __restrict__ tri_out, unsigned flags,
                                                    tail_args tail) {
  const trace_scene scene = {nodes4, tris, faces, colors, rem, 0};  // (n_faces, H, W: not needed, a parked ray exists)
  const trace_cast cast = {rays, ox, oy, oz, 0, 0, flags};
  const lt_scan_images out = {endpoints, endcolors, range, endrem, tri_out};
  __shared__ int stk[LT_TAIL_STACK];
  __shared__ unsigned long long best;  // (t bits) << 32 | face: for t > 0 the integer order is the order of (t, face)
  const int lane = threadIdx.x, j = lane & 3, q = lane >> 2;
  const int n_tail = *tail.count;
  if (blockIdx.x == 0 && lane == 0) *tail.count_next = 0;
  for (int it = blockIdx.x; it < n_tail; it += gridDim.x) {
    const size_t ray = (size_t)tail.queue[it];
    const float4 meta = tail.meta[it];
    int sp = __float_as_int(meta.z);
    const int* src = tail.stack + (size_t)it * LT_TAIL_SAVE;
    for (int i = lane; i < sp; i += 64) stk[i] = src[i];
    if (lane == 0) best = ((unsigned long long)__float_as_uint(meta.x) << 32) | (unsigned)__float_as_int(meta.y);
    const trace_ray r = trace_ray_of(cast, ray, true);
    __syncthreads();
    while (sp > 0) {  // sp is wave-uniform
      const int take = sp > LT_TAIL_DFS ? 1 : min(sp, 16);
      const int ref_in = q < take ? stk[sp - 1 - q] : LT_DONE;  // quad 0 takes the top = the nearest deferred child
      const float best_t = __uint_as_float((unsigned)(best >> 32));
      __syncthreads();  // every quad has read its entry and the best t before anything is pushed / improved
      sp -= take;
      int hit = 0, ref = 0;
      float tn = 0.f;
      if (ref_in >= 0) {  // node: lane j tests child j
        const float4* N = scene.nodes + 8 * (size_t)ref_in + 2 * j;
        hit = trace_slab(N[0], N[1], r, best_t, tn, ref);
      } else if (ref_in != LT_DONE) {  // leaf: lane j tests triangle j
        int start, cnt;
        leaf_range(ref_in, start, cnt);
        float t = INFINITY;
        int f = LT_NO_FACE;
        if (j < cnt) t = trace_tri(scene.tris + 3 * (size_t)(start + j), r, f);
        quad_min_hit(t, f);
        if (j == 0 && f != LT_NO_FACE && t < 999999999.f)
          atomicMin(&best, ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)f);
      }
      // push the hit children of all quads: far ones first inside a quad (the nearer child is popped first); the
      // quads are stacked in reverse order so that quad 0's children -- the subtree of the old top -- end on top
      const quad_ranked k = quad_rank(hit, tn, lane);
      // exclusive prefix of nh over the quads ABOVE this one (quads q+1 .. 15), via the hit ballot
      const int above = q == 15 ? 0 : __popcll(k.hits >> ((q + 1) * 4));
      const int total = __popcll(k.hits);
      if (hit) stk[sp + above + (k.nh - 1 - k.rank)] = ref;
      sp += total;
      __syncthreads();
    }
    if (lane == 0) {
      const unsigned long long b = best;
      trace_writeback(ray, __uint_as_float((unsigned)(b >> 32)), (int)(unsigned)(b & 0xFFFFFFFFull), r, scene, cast.flags,
                      out);
    }
    __syncthreads();
  }
}

// =====================================================================================================
// Host
// =====================================================================================================
bool lt_binary_path() {
  static const bool v = []() {
    const char* e = getenv("LIDARHIP_TRACE");
    return e && strcmp(e, "binary") == 0;
  }();
  return v;
}

// workgroups of 4 waves for an H x W image cut into tile_h x tile_w tiles, one tile per wave; a multiple of 8 (trace_cell)
static int trace_grid(int H, int W, int tile_h, int tile_w) {
  const int tiles = ((H + tile_h - 1) / tile_h) * ((W + tile_w - 1) / tile_w);
  const int nblocks = (tiles + 3) / 4;
  return (nblocks + 7) & ~7;
}

template <bool COUNT>
static void launch_k_trace(const lt_scene* s, const trace_scene& scene, const trace_cast& cast, const lt_scan_images& out,
                           hipStream_t stream) {
  hipLaunchKernelGGL(k_trace<COUNT>, dim3(trace_grid(cast.H, cast.W, LT_TILE_H, LT_TILE_W)), dim3(256), 0, stream, scene,
                     cast, out, s->overflow, s->counters);
}

template <bool COUNT>
static void launch_k_trace4(const lt_scene* s, const trace_scene& scene, const trace_cast& cast, const lt_scan_images& out,
                            int step_cap, const tail_args& tail, hipStream_t stream) {
  hipLaunchKernelGGL(k_trace4<COUNT>, dim3(trace_grid(cast.H, cast.W, LT_TILE4_H, LT_TILE4_W)), dim3(256), 0, stream,
                     scene, cast, out, s->overflow, s->counters, step_cap, tail);
}

int lt_trace_launch(lt_scene* s, const float* rays, const float* origin, int n_rays, int height, float* endpoints,
                    int* endcolors, float* range, float* endrem, int* tri, unsigned flags, hipStream_t stream,
                    lt_stats* stats) {
  if (!s->built) {
    lt_set_error("lt_scene_trace_dev: scene has no BVH (call lt_scene_build first)");
    return LT_ERR_NOT_BUILT;
  }
  if (height <= 0 || n_rays < 0 || !origin || (n_rays > 0 && !rays)) {
    lt_set_error("lt_scene_trace_dev: invalid argument (height=%d n_rays=%d)", height, n_rays);
    return LT_ERR_INVALID_ARG;
  }
  s->last_stream = stream;
  const int W = n_rays / height;  // RayTracer.cpp:56
  const int H = height;
  const bool timed = stats != nullptr;
  const bool count = (flags & LT_TRACE_COUNT) != 0;
  const bool binary = lt_binary_path();
  s->stats.n_rays = W * H;
  if (W > 0) {
    LT_CHECK(lt_scene_reserve_rays(s, W * H));
    if (count) LT_HIP(hipMemsetAsync(s->counters, 0, 4 * sizeof(unsigned long long), stream));
    const trace_scene scene = {binary ? s->nodes : s->nodes4, s->tris, s->faces, s->colors, s->rem, s->n_faces};
    const trace_cast cast = {rays, origin[0], origin[1], origin[2], H, W, flags};
    const lt_scan_images out = {endpoints, endcolors, range, endrem, tri};
    if (timed) LT_HIP(hipEventRecord(s->ev[7], stream));
    if (binary) {
      if (count) launch_k_trace<true>(s, scene, cast, out, stream);
      else launch_k_trace<false>(s, scene, cast, out, stream);
    } else {
      // two hand-over counters used alternately: the tail kernel of a launch re-arms the other one
      const bool with_tail = !count && !(flags & LT_TRACE_DEBUG_STEPS);
      const tail_args tail = {s->tail_stack, s->tail_meta, s->tail_queue, s->tail_count + (s->tail_parity & 1),
                              s->tail_count + ((s->tail_parity & 1) ^ 1)};
      if (with_tail) s->tail_parity ^= 1;
      static const int env_cap = []() {
        const char* e = getenv("LIDARHIP_STEP_CAP");
        return e ? atoi(e) : LT_TRACE4_STEP_CAP;
      }();
      // counting and the per-ray step image measure the undisturbed walk: no hand-over there
      const int step_cap = (!with_tail || env_cap <= 0) ? 0x7fffffff : env_cap;
      if (count) {
        launch_k_trace4<true>(s, scene, cast, out, step_cap, tail, stream);
      } else {
        if (s->probe[0]) LT_HIP(hipEventRecord(s->probe[0], stream));
        launch_k_trace4<false>(s, scene, cast, out, step_cap, tail, stream);
        // (launched even when the cap is off: it re-arms the counter and finds an empty queue)
        hipLaunchKernelGGL(k_trace4_tail, dim3(4096), dim3(64), 0, stream, scene.nodes, scene.tris, cast.rays,
                           cast.ox, cast.oy, cast.oz, scene.faces, scene.colors, scene.rem, out.endpoints, out.endcolors,
                           out.range, out.endrem, out.tri, cast.flags, tail);
        if (s->probe[1]) LT_HIP(hipEventRecord(s->probe[1], stream));
        s->probe[0] = s->probe[1] = nullptr;
      }
    }
    if (timed) LT_HIP(hipEventRecord(s->ev[8], stream));
    LT_HIP(hipGetLastError());
  }
  if (timed || count) {
    LT_HIP(hipStreamSynchronize(stream));
    if (timed && W > 0) LT_HIP(hipEventElapsedTime(&s->stats.ms_trace, s->ev[7], s->ev[8]));
    if (count && W > 0) {
      unsigned long long c[4];
      LT_HIP(hipMemcpy(c, s->counters, sizeof(c), hipMemcpyDeviceToHost));
      s->stats.nodes_visited = c[0];
      s->stats.tris_tested = c[1];
      s->stats.n_hits = (int)c[2];
      s->stats.stack_overflows = c[3];
      s->stats.entries_culled = 0;  // (the LT_TRACE_CULL A/B is gone: include/lidarhip.h)
    }
    if (stats) *stats = s->stats;
  }
  return LT_OK;
}
