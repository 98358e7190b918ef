// lt_mc.hip -- marching cubes on the device: the mesh of a TSDF volume is born in HBM.
//
// Replaces `TSDFVolume.get_mesh` of the reference (auxiliary/fusion_lidar.py:403-424): get_volume's device-to-host
// copies of three volumes (:395-400), scikit-image's CPU marching cubes (:407), the numpy attribute look-ups
// (:409-423) -- and, downstream, the upload of the mesh for the ray cast (fusion_lidar.py:433-451).  The mesh is
// written as the four arrays the ray cast consumes (verts [V,3] f32 world, faces [F,3] i32, colors [V,3] i32,
// rem [V] f32), indexed (one vertex per sign-changing lattice edge, shared by the cells around it) like
// scikit-image emits it.
//
// The 800 M-voxel default volume (2000 x 2000 x 200, 3.2 GB per field) is 99.8 % empty space, so the float field is
// read ONCE, as a stream, and everything else works on one SIGN BIT per voxel:
//
//   k_mc_signs    tsdf -> one bit per voxel, set when the value is NOT above the level (wave ballot; rows of nz bits padded
//                 to 64-bit words): 3.2 GB in, 128 MB out
//   k_mc_words    one thread per 64-voxel word: crossing-edge masks ex / ey / ez of the edges its voxels own
//                 (m ^ neighbour word, shifted for z), active-cell mask (the 8 corner words are not all equal), number
//                 of vertices (popcounts) and triangles (case table, only on the set bits); the cells of Lewiner's
//                 ambiguous cases are queued; per-workgroup totals
//   k_mc_amb      one lane per queued cell: the face / interior tests on its eight values pick the tiling; its triangles
//                 and centre vertex are added to the counts, the tiling is filed for k_mc_emit_batch
//   k_mc_scan1/2  exclusive scan of the workgroup totals in two levels -> V, F
//   k_mc_compact  word -> compact index of the active words (the ~2 % that own a vertex or a triangle); per active
//                 word a record {word, vertex base, triangle base, ex, ey, ez}
//   k_mc_emit_batch  one WAVE per 8 active words, one lane per VERTEX / per TRIANGLE of the batch (positions by
//                 scikit-image's centre-of-mass rule in double, attributes from the nearest voxel); the index of a vertex
//                 owned by a neighbouring word comes from that word's record (neighbour records staged in LDS): base +
//                 popcount of the edge masks below the bit; a cell's centre vertex follows its word's edge vertices
//
// WHICH mesh: scikit-image 0.18's `marching_cubes_lewiner` (what the reference calls, fusion_lidar.py:407) -- Lewiner's 33
// cases with their face / interior tests and centre vertices, decided on the cell's eight VALUES where the signs do not
// (1-2 % of a street scene's cells; the rest is table look-up on the sign bits as before), every face's vertices in
// scikit-image's order (gradient_direction = "descent").  The vertices (positions bit for bit, colours, remissions) and the
// FACE STREAM -- face k: the same three vertices in the same order -- equal the reference's get_mesh output (golden F10
// made by the real scikit-image: tests/test_pin_f10_f11_gpu.py; the CPU oracle oracle/lt_mc_oracle.c reproduces the
// reference's arrays and is identical to this file up to the numbering of the vertices).  Faces come by (cell ascending in
// (a0, a1, a2), tiling order), which IS scikit-image's order; vertices are numbered by (word of 64 voxels; owner voxel x, y, z
// ascending, edge axis; then the word's centre vertices) where scikit-image numbers them by first use --
// deterministic (the only atomics, k_mc_amb's, are commutative adds and slot claims whose outcome does not reach the
// output's order); scikit-image numbers vertices by first use in a serial face stream.
// Tables: lt_mc_lewiner_table.h (Lewiner's LookUpTable.h as scikit-image ships it, tools/gen_mc_lewiner.py).
#include "lt_internal.h"
#include "lt_devmem.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define LT_LW_ATTR __device__
#define LT_LW_NO_RAW
#include "lt_mc_lewiner_table.h"  // Lewiner's tables as the device reads them (tools/gen_mc_lewiner.py, derived())

// ---- Lewiner's case selection, as scikit-image 0.18 runs it ---------------------------------------------------------------
// (MarchingCubes.cpp process_cube / test_face / test_interior; skimage/measure/_marching_cubes_lewiner_cy.pyx the_big_switch /
// test_face / test_internal.)  Everything in double on the float32 field values, level 0; `eps` = np.spacing(1.0) -- the
// value scikit-image's `FLT_EPSILON` holds, despite its name.  Two properties of scikit-image's port are reproduced because
// the reference runs IT (both measured against the real library, tools/mc_lewiner_fuzz.py): its divisions are guarded by
// `+ eps` in the denominator, which decides exact ties, and `test_internal` falls off its end (returns 0) where Lewiner's
// C++ returns `s < 0` -- case 4 with a negative TEST4 entry therefore takes tiling 4.1.2 for the 5 / 10 patterns.
#define LT_MC_EPS 2.220446049250313e-16
__device__ __forceinline__ double lw_pick(const double* v, int i) {  // v[i] without a private-memory array
  double r = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) r = (i == k) ? v[k] : r;
  return r;
}
__device__ __forceinline__ bool lw_test_face(const double* v, int face) {
  const int f = face < 0 ? -face : face;
  // faces 1..6: (A, B, C, D) = corners (0,4,5,1) (1,5,6,2) (2,6,7,3) (3,7,4,0) (0,3,2,1) (4,7,6,5)
  const unsigned abcd = f == 1 ? 0x0451u : f == 2 ? 0x1562u : f == 3 ? 0x2673u : f == 4 ? 0x3740u : f == 5 ? 0x0321u : 0x4765u;
  const double A = lw_pick(v, (abcd >> 12) & 7), B = lw_pick(v, (abcd >> 8) & 7), C = lw_pick(v, (abcd >> 4) & 7),
               D = lw_pick(v, abcd & 7);
  const double acbd = A * C - B * D;
  if (acbd > -LT_MC_EPS && acbd < LT_MC_EPS) return face >= 0;
  return (double)face * A * acbd >= 0;
}
// edge < 0: cases 4 and 10 (the interior's saddle along the 0-4 direction); else the reference edge of cases 6, 7, 12, 13
__device__ __forceinline__ bool lw_test_interior(const double* v, int edge, int s) {
  double t, At = 0, Bt, Ct, Dt;
  if (edge < 0) {
    const double a = (v[4] - v[0]) * (v[6] - v[2]) - (v[7] - v[3]) * (v[5] - v[1]);
    const double b = v[2] * (v[4] - v[0]) + v[0] * (v[6] - v[2]) - v[1] * (v[7] - v[3]) - v[3] * (v[5] - v[1]);
    t = -b / (2 * a + LT_MC_EPS);
    if (t < 0 || t > 1) return s > 0;
    At = v[0] + (v[4] - v[0]) * t;
    Bt = v[3] + (v[7] - v[3]) * t;
    Ct = v[2] + (v[6] - v[2]) * t;
    Dt = v[1] + (v[5] - v[1]) * t;
  } else {
    // the reference edge (p, q) and the three edges parallel to it, round the cell: 8 corner numbers, 3 bits each
    const unsigned E = edge == 0 ? 001327645u : edge == 1 ? 012034756u : edge == 2 ? 023105467u : edge == 3 ? 030216574u
                     : edge == 4 ? 045763201u : edge == 5 ? 056470312u : edge == 6 ? 067541023u : edge == 7 ? 074652130u
                     : edge == 8 ? 004372615u : edge == 9 ? 015043726u : edge == 10 ? 026150437u : 037261504u;
    const double p = lw_pick(v, (E >> 21) & 7), q = lw_pick(v, (E >> 18) & 7);
    const double b0 = lw_pick(v, (E >> 15) & 7), b1 = lw_pick(v, (E >> 12) & 7), c0 = lw_pick(v, (E >> 9) & 7),
                 c1 = lw_pick(v, (E >> 6) & 7), d0 = lw_pick(v, (E >> 3) & 7), d1 = lw_pick(v, E & 7);
    t = p / (p - q + LT_MC_EPS);
    Bt = b0 + (b1 - b0) * t;
    Ct = c0 + (c1 - c0) * t;
    Dt = d0 + (d1 - d0) * t;
  }
  const int test = (At >= 0 ? 1 : 0) | (Bt >= 0 ? 2 : 0) | (Ct >= 0 ? 4 : 0) | (Dt >= 0 ? 8 : 0);
  // 0 1 2 3 4 6 8 9 12 -> s > 0;  7 11 13 14 15 -> s < 0;  5 / 10: the saddle's sign, else scikit-image's fall-through (0)
  if ((0x135Fu >> test) & 1u) return s > 0;
  if (test == 5) return (At * Ct - Bt * Dt < LT_MC_EPS) ? s > 0 : false;
  if (test == 10) return (At * Ct - Bt * Dt >= LT_MC_EPS) ? s > 0 : false;
  return s < 0;
}
// a tiling = its rows's offset in LT_LWF | triangles << 16 | uses the centre vertex << 20
#define LWT(T, row) ((unsigned)(LT_LWF_##T + (row) * LT_LWF_##T##_LEN) | ((unsigned)(LT_LWF_##T##_LEN / 3) << 16) | ((unsigned)LT_LWF_##T##_C << 20))
// v[p]: the cell's values in Lewiner's corner order; cs: the device's case index (an AMBIGUOUS one: LT_LWC_FIXED[cs] == ~0)
__device__ __noinline__ unsigned lw_select(const double* v, int cs) {
  const int c = LT_LWC_CASE[cs], g = LT_LWC_CONFIG[cs];
  int sub = 0;
  switch (c) {
    case 3: return lw_test_face(v, LT_LWD_TEST3[g]) ? LWT(TILING3_2, g) : LWT(TILING3_1, g);
    case 4: return lw_test_interior(v, -1, LT_LWD_TEST4[g]) ? LWT(TILING4_1, g) : LWT(TILING4_2, g);
    case 6:
      if (lw_test_face(v, LT_LWD_TEST6[g][0])) return LWT(TILING6_2, g);
      return lw_test_interior(v, LT_LWD_TEST6[g][2], LT_LWD_TEST6[g][1]) ? LWT(TILING6_1_1, g) : LWT(TILING6_1_2, g);
    case 7:
      if (lw_test_face(v, LT_LWD_TEST7[g][0])) sub += 1;
      if (lw_test_face(v, LT_LWD_TEST7[g][1])) sub += 2;
      if (lw_test_face(v, LT_LWD_TEST7[g][2])) sub += 4;
      switch (sub) {
        case 0: return LWT(TILING7_1, g);
        case 1: return LWT(TILING7_2, g * 3 + 0);
        case 2: return LWT(TILING7_2, g * 3 + 1);
        case 3: return LWT(TILING7_3, g * 3 + 0);
        case 4: return LWT(TILING7_2, g * 3 + 2);
        case 5: return LWT(TILING7_3, g * 3 + 1);
        case 6: return LWT(TILING7_3, g * 3 + 2);
        default: return lw_test_interior(v, LT_LWD_TEST7[g][4], LT_LWD_TEST7[g][3]) ? LWT(TILING7_4_2, g) : LWT(TILING7_4_1, g);
      }
    case 10:
      if (lw_test_face(v, LT_LWD_TEST10[g][0])) return lw_test_face(v, LT_LWD_TEST10[g][1]) ? LWT(TILING10_1_1_, g) : LWT(TILING10_2, g);
      if (lw_test_face(v, LT_LWD_TEST10[g][1])) return LWT(TILING10_2_, g);
      return lw_test_interior(v, -1, LT_LWD_TEST10[g][2]) ? LWT(TILING10_1_1, g) : LWT(TILING10_1_2, g);
    case 12:
      if (lw_test_face(v, LT_LWD_TEST12[g][0])) return lw_test_face(v, LT_LWD_TEST12[g][1]) ? LWT(TILING12_1_1_, g) : LWT(TILING12_2, g);
      if (lw_test_face(v, LT_LWD_TEST12[g][1])) return LWT(TILING12_2_, g);
      return lw_test_interior(v, LT_LWD_TEST12[g][3], LT_LWD_TEST12[g][2]) ? LWT(TILING12_1_1, g) : LWT(TILING12_1_2, g);
    case 13: {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (lw_test_face(v, LT_LWD_TEST13[g][k])) sub += 1 << k;
      const int sc = LT_LWD_SUBCONFIG13[sub];
      if (sc < 0) return 0u;  // "Impossible case 13?": nothing is added
      if (sc == 0) return LWT(TILING13_1, g);
      if (sc <= 6) return LWT(TILING13_2, g * 6 + sc - 1);
      if (sc <= 18) return LWT(TILING13_3, g * 12 + sc - 7);
      if (sc <= 22) return LWT(TILING13_4, g * 4 + sc - 19);
      if (sc <= 26)
        return lw_test_interior(v, LT_LWD_EDGE13_5[g][sc - 23], LT_LWD_TEST13[g][6]) ? LWT(TILING13_5_1, g * 4 + sc - 23)
                                                                                        : LWT(TILING13_5_2, g * 4 + sc - 23);
      if (sc <= 38) return LWT(TILING13_3_, g * 12 + sc - 27);
      if (sc <= 44) return LWT(TILING13_2_, g * 6 + sc - 39);
      return LWT(TILING13_1_, g);
    }
    default: return 0u;
  }
}
// the tiling of an AMBIGUOUS cell at voxel (x, y, z) with case index cs: the tests on the cell's eight values (Lewiner's
// corner p sits at (a0, a1, a2) = LW_CORNER[p] of the generator / the oracle: 0 (0,0,0)  1 (0,0,1)  2 (0,1,1)  3 (0,1,0)
// 4 (1,0,0)  5 (1,0,1)  6 (1,1,1)  7 (1,1,0) -- scikit-image's x is the last axis).  Only k_mc_amb calls this: the double
// precision tests cost 100 vector registers, which the sweep and the emission kernels must not pay for 1-2 % of the cells.
__device__ __forceinline__ unsigned lw_cell_eval(const float* __restrict__ c, size_t sx, size_t sy, size_t sz, int cs) {
  double v[8];  // (sx, sy, sz: floats between neighbours along x, y, z)
  v[0] = (double)c[0];       v[1] = (double)c[sz];          v[2] = (double)c[sy + sz];      v[3] = (double)c[sy];
  v[4] = (double)c[sx];      v[5] = (double)c[sx + sz];     v[6] = (double)c[sx + sy + sz]; v[7] = (double)c[sx + sy];
  return lw_select(v, cs);
}
// ---- the ambiguous cells' side channel -------------------------------------------------------------------------------
// k_mc_words queues every ambiguous cell it meets (voxel index, case index, its block of the scan) and counts it with 0
// triangles; k_mc_amb evaluates the queue -- one lane per cell --, adds the cell's triangles / centre vertex to the counts
// of its word and of its block (atomics: the one place of the extraction that has them; the RESULT does not depend on their
// order), and files the tiling under the voxel index in an open-addressing table that k_mc_emit_batch reads.
// The queue is SHARDED: 64 segments of `cap` entries, a counter each in a 128-byte line of its own; a block of k_mc_words
// appends to segment (block & 63).  One counter for all took ~5 000 returning atomics in a row on one address -- 10 of
// k_mc_words' 43 us (measured by taking the atomic out); the order of the queue does not reach the output.
#define LT_MC_SHARDS 64
#define LT_MC_CTR_STRIDE 32  // ints between two shards' counters
struct mc_amb {
  uint2* queue;      // [LT_MC_SHARDS][cap]: (voxel index, case | block << 8)
  int* counter;      // [LT_MC_SHARDS * LT_MC_CTR_STRIDE]: cells queued per shard (may exceed cap: the host then grows the
                     // buffers and starts over), then [LT_MC_SHARDS] the counts of the LAST extraction (k_mc_clear)
  uint2* table;      // [tcap], tcap a power of two >= 4 x LT_MC_SHARDS x cap: (voxel index + 1, tiling); 0 = empty
  unsigned cap, tmask;
};
__device__ __forceinline__ unsigned amb_slot(unsigned i, unsigned tmask) { return (i * 2654435761u) & tmask; }
__device__ __forceinline__ unsigned amb_lookup(const mc_amb& A, unsigned i) {
  for (unsigned h = amb_slot(i, A.tmask);; h = (h + 1) & A.tmask) {
    const uint2 e = A.table[h];
    if (e.x == i + 1u) return e.y;
    if (e.x == 0u) return 0u;  // (not filed: cannot happen after k_mc_amb; no triangles rather than a wild read)
  }
}
#define LW_NT(sel) (((sel) >> 16) & 15u)
#define LW_C(sel) (((sel) >> 20) & 1u)
#define LW_OFF(sel) ((sel) & 0xFFFFu)

// debug (-DLT_MC_STAMP=1: k_mc_words, =2: k_mc_compact; tools/mc_wave_times.py): wall clock (100 MHz) at the start of a wave,
// after its stamp ballot and at its end, and the number of blocks it walked
#ifdef LT_MC_STAMP
__device__ unsigned long long g_mc_stamp[4 << 16];
extern "C" int lt_debug_mc_stamps(unsigned long long* out, int n_waves) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mc_stamp), (size_t)min(n_waves, 1 << 16) * 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#define LT_MC_STAMP_AT(which, w, i, v) do { if (LT_MC_STAMP == (which) && (threadIdx.x & 63) == 0 && (w) < (1 << 16)) g_mc_stamp[(w) * 4 + (i)] = (v); } while (0)
// =3: k_mc_emit_batch by section -- g_mc_stamp[8 b + i]: the wall clock between marks i - 1 and i of batch b (plain stores:
// atomics on eight shared words serialise the waves behind them and measure themselves)
// (st: the batch's mc_stamp -- its number and its last mark)
#define LT_MC_SECTION(st, i) do { if (LT_MC_STAMP == 3) { const unsigned long long t_ = wall_clock64(); if ((threadIdx.x & 63) == 0 && (st).bi < (1 << 15)) g_mc_stamp[(st).bi * 8 + (i)] = t_ - (st).last; (st).last = t_; } } while (0)
#define LT_MC_SECTION_START(bi) {(bi), (unsigned long long)wall_clock64()}
#else
#define LT_MC_STAMP_AT(which, w, i, v) do { } while (0)
#define LT_MC_SECTION(st, i) do { } while (0)
#define LT_MC_SECTION_START(bi) {(bi), 0ull}
#endif
struct mc_stamp { int bi; unsigned long long last; };

typedef unsigned long long u64;

struct mc_dims {
  int nx, ny, nz;
  int wz;        // 64-bit words per (x, y) row
  int n_words;   // nx * ny * wz
  unsigned ny_m; int ny_s;  // row / ny likewise (mc_x_of)
  int vs;        // floats between two voxels of a field array: 1 (three separate arrays, lt_marching_cubes_dev) or 4 (a
                 // TSDF volume's interleaved (tsdf, weight, colour, remission) records, lt_tsdf.hip LT_VOX)
  unsigned wz_m; int wz_s;  // w / wz by multiplication (mc_row_of): an integer division is ~40 vector instructions, and
                            // k_mc_words runs one per word of the volume (16 M on the default one)
};

// row = w / D.wz for 0 <= w < 2^31 (round-up method: m = floor(2^32 (2^s - d) / d) + 1, s = ceil(log2 d))
__device__ __forceinline__ int mc_udiv(int n_, unsigned m, int s) {
  if (s == 0) return n_;  // d == 1
  const unsigned n = (unsigned)n_, t = __umulhi(n, m);
  return (int)((t + ((n - t) >> 1)) >> (s - 1));
}
__device__ __forceinline__ int mc_row_of(const mc_dims& D, int w) { return mc_udiv(w, D.wz_m, D.wz_s); }
__device__ __forceinline__ int mc_x_of(const mc_dims& D, int row) { return mc_udiv(row, D.ny_m, D.ny_s); }  // x = row / ny
static void mc_magic(unsigned d, unsigned* m, int* s) {  // (host)
  int sh = 0;
  while ((1u << sh) < d) ++sh;
  *s = sh;
  *m = sh == 0 ? 0u : (unsigned)((((unsigned long long)1 << 32) * (((unsigned long long)1 << sh) - d)) / d + 1ull);
}

struct mc_rec {  // one per active word
  int w, vbase, tbase, pad;  // pad: the word's triangle count | its number of centre vertices << 16
  u64 ex, ey, ez;
};

struct lt_mesh {
  int device;
  float* verts; int* faces; int* colors; float* rem;
  int cap_v, cap_f, n_verts, n_faces;
  u64* bits; unsigned* cnt; int* cmap; size_t cap_words;
  int* blk; size_t cap_blocks;          // 3 ints per block of 64 rows (mc_triple), then 3 per segment of 256 blocks, then 4 totals
  int* totals_host;                     // pinned: {active words, vertices, triangles, -}
  mc_rec* rec; size_t cap_rec;
  // cnt / cmap hold 0 / -1 for every word that is not an active word of the LAST extraction (k_mc_clear undoes those
  // before the next one): the 2 x 64 MB of the default volume are never swept again.  n_prev: active words of the last
  // extraction (their records are still in `rec`); state_dirty: an extraction did not finish -- sweep everything once
  int n_prev, state_dirty;
  int* wave_na; size_t cap_wave_na;     // active words per wave of 64 rows (k_mc_words -> k_mc_compact)
  mc_amb amb; size_t amb_cap;           // the ambiguous cells' queue and tiling table (k_mc_amb); counter = amb.counter
  int n_amb_prev;                       // cells of the last extraction: their table slots are emptied by k_mc_clear
  // lt_mesh_renumber_dev: the second set of vertex arrays (swapped with the first), first use / new number per vertex, block sums
  float* verts2; int* colors2; float* rem2; int cap_v2;
  int* rn_first; int* rn_newid; size_t cap_rn; int* rn_bsum; size_t cap_bsum;
  float ms_signs, ms_rest;              // last extraction (when timed)
  hipEvent_t ev[3];
};

// ---- k_mc_signs ----------------------------------------------------------------------------------------------------
// col_epoch / epoch (may be NULL): stamps of the (x, y) columns written since the volume's last reset (lt_tsdf.hip) --
// a clean column still holds the initial tsdf = 1 everywhere, its sign bits are 0 without reading it.  A wave takes 64
// rows (= columns of the volume) at a time: lane r zeroes the words of row r when that row is clean; the dirty rows
// are then walked one by one, z along the lanes, four words (loads) in flight.
__global__ __launch_bounds__(256) void k_mc_signs(const float* __restrict__ tsdf, mc_dims D, u64* __restrict__ bits,
                                                  const unsigned* __restrict__ col_epoch, unsigned epoch) {
  const int lane = threadIdx.x & 63;
  const int n_rows = D.nx * D.ny;
  const int n_chunks = (n_rows + 63) / 64;
  for (int chunk = blockIdx.x * 4 + (threadIdx.x >> 6); chunk < n_chunks; chunk += gridDim.x * 4) {
    const int row = chunk * 64 + lane;
    bool dirty = false;
    if (row < n_rows) {
      dirty = !col_epoch || col_epoch[row] == epoch;
      if (!dirty)
        for (int k = 0; k < D.wz; ++k) bits[(size_t)row * D.wz + k] = 0ull;
    }
    u64 m = __ballot(dirty);
    while (m) {
      const int r = chunk * 64 + (__ffsll((long long)m) - 1);
      m &= m - 1;
      const float* src = tsdf + (size_t)r * D.nz * D.vs;
      for (int k0 = 0; k0 < D.wz; k0 += 4) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int z = (k0 + k) * 64 + lane;
          v[k] = z < D.nz ? src[(size_t)z * D.vs] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const u64 w = __ballot(!(v[k] > 0.0f));  // level 0: the bit says "NOT above the level" (Lewiner's index bit, inverted)
          if (lane == 0 && k0 + k < D.wz) bits[(size_t)r * D.wz + k0 + k] = w;
        }
      }
    }
  }
}

// ---- masks of one word ---------------------------------------------------------------------------------------------
struct mc_masks {
  u64 m[2][2];  // sign bits of the rows (x + dx, y + dy)
  u64 s[2][2];  // the same shifted by one z (bit b = voxel z + 1)
  u64 ex, ey, ez, ac;
};

__device__ __forceinline__ u64 low_bits(int n) { return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull)); }

// masks from the 8 sign words of a word's cell corners, w8[dx | dy << 1 | dw << 2] (0 where the volume ends)
__device__ __forceinline__ mc_masks mc_build(const u64* w8, const mc_dims& D, int x, int y, int wz) {
  mc_masks M;
  const bool hx = x + 1 < D.nx, hy = y + 1 < D.ny;
#pragma unroll
  for (int dx = 0; dx < 2; ++dx)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const u64 m = w8[dx | (dy << 1)], nxt = w8[dx | (dy << 1) | 4];
      M.m[dx][dy] = m;
      M.s[dx][dy] = (m >> 1) | (nxt << 63);
    }
  const u64 vzn = low_bits(D.nz - wz * 64);      // voxels that exist
  const u64 vz = low_bits(D.nz - 1 - wz * 64);   // voxels with a +z neighbour
  M.ex = hx ? ((M.m[0][0] ^ M.m[1][0]) & vzn) : 0ull;
  M.ey = hy ? ((M.m[0][0] ^ M.m[0][1]) & vzn) : 0ull;
  M.ez = (M.m[0][0] ^ M.s[0][0]) & vz;
  M.ac = 0ull;
  if (hx && hy) {
    const u64 any = M.m[0][0] | M.m[0][1] | M.m[1][0] | M.m[1][1] | M.s[0][0] | M.s[0][1] | M.s[1][0] | M.s[1][1];
    const u64 all = M.m[0][0] & M.m[0][1] & M.m[1][0] & M.m[1][1] & M.s[0][0] & M.s[0][1] & M.s[1][0] & M.s[1][1];
    M.ac = (any & ~all) & vz;
  }
  return M;
}

__device__ __forceinline__ mc_masks mc_load(const u64* __restrict__ bits, const mc_dims& D, int x, int y, int wz) {
  const bool hx = x + 1 < D.nx, hy = y + 1 < D.ny, hz = wz + 1 < D.wz;
  const int row = x * D.ny + y;
  u64 w8[8];
#pragma unroll
  for (int dx = 0; dx < 2; ++dx)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const bool have = (dx == 0 || hx) && (dy == 0 || hy);
      const size_t i = (size_t)(row + dx * D.ny + dy) * D.wz + wz;
      w8[dx | (dy << 1)] = have ? bits[i] : 0ull;
      w8[dx | (dy << 1) | 4] = (have && hz) ? bits[i + 1] : 0ull;
    }
  return mc_build(w8, D, x, y, wz);
}

// case index of the cell at bit b: corner i at (dx, dy, dz) = (i & 1, (i >> 1) & 1, (i >> 2) & 1)
__device__ __forceinline__ int mc_case(const mc_masks& M, int b) {
  int cs = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u64 m = (i & 4) ? M.s[i & 1][(i >> 1) & 1] : M.m[i & 1][(i >> 1) & 1];
    cs |= (int)((m >> b) & 1ull) << i;
  }
  return cs;
}

// ---- the packed triple ------------------------------------------------------------------------------------------------
// (active words, vertices, triangles) of a row, a block of 64 rows or a prefix of either, summed / scanned across a wave as
// ONE 64-bit word of 20 bits a field.  The largest value a field takes is a block's triangles: 64 rows x wz words x <= 768
// triangles a word (64 cells of <= 12) < 2^20 for wz <= 21 -- mc_dims_of refuses nz > 21 x 64 = 1344 for this reason.  In
// memory a block's triple is three ints, blk[3 b ..] (lt_mesh::blk).
struct mc_triple { unsigned a, v, t; };
__device__ __forceinline__ u64 pack3(unsigned a, unsigned v, unsigned t) { return (u64)a | ((u64)v << 20) | ((u64)t << 40); }
__device__ __forceinline__ mc_triple unpack3(u64 p) {
  return {(unsigned)(p & 0xFFFFF), (unsigned)((p >> 20) & 0xFFFFF), (unsigned)((p >> 40) & 0xFFFFF)};
}
__device__ __forceinline__ u64 wave_sum3(u64 p) {  // the wave's total, in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
  return p;
}
__device__ __forceinline__ mc_triple blk_load3(const int* __restrict__ blk, int b) {
  return {(unsigned)blk[3 * b], (unsigned)blk[3 * b + 1], (unsigned)blk[3 * b + 2]};
}
__device__ __forceinline__ void blk_store3(int* __restrict__ blk, int b, const mc_triple& s) {
  blk[3 * b] = (int)s.a; blk[3 * b + 1] = (int)s.v; blk[3 * b + 2] = (int)s.t;
}
// (k_mc_amb: a cell's late triangles / centre vertex / newly active word; fields that are 0 cost no atomic)
__device__ __forceinline__ void blk_add3(int* __restrict__ blk, int b, const mc_triple& s) {
  if (s.v) atomicAdd(&blk[3 * b + 1], (int)s.v);
  if (s.t) atomicAdd(&blk[3 * b + 2], (int)s.t);
  if (s.a) atomicAdd(&blk[3 * b], (int)s.a);
}

__device__ __forceinline__ u64 wave_incl_scan(u64 p) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 q = __shfl_up(p, o, 64);
    if (lane >= o) p += q;
  }
  return p;
}

// What the pieces of k_mc_words share, by const&.  The kernel puts it together from its arguments: as ONE kernel argument by
// value (tried for k_mc_words, k_mc_amb and k_mc_compact, no load changed kind) the three kernels together were about 1 us
// slower than with separate arguments (profiles/mc_count_phases/README.md, series A to C), so they keep those.
struct mc_sweep_args {
  mc_dims D;
  const u64* bits;
  unsigned* cnt;   // per word: vertices | triangles << 16
  int* blk;        // per block of 64 rows: its triple (blk_load3)
  int* wave_na;    // per block: its active words (k_mc_words -> k_mc_compact)
  int n_blocks;
  mc_amb A;
};

// ---- k_mc_words -----------------------------------------------------------------------------------------------------
// a word can only own a crossing edge or an active cell if its row (x, y) or one of the rows (x, y + 1), (x + 1, y),
// (x + 1, y + 1) was written since the volume's last reset; the stamps are 4 B per row against 8 sign words per thread
__device__ __forceinline__ bool mc_rows_dirty(const unsigned* __restrict__ col_epoch, unsigned epoch, const mc_dims& D,
                                              int row) {
  if (!col_epoch) return true;
  const int last = D.nx * D.ny - 1;
  return col_epoch[row] == epoch || col_epoch[min(row + 1, last)] == epoch || col_epoch[min(row + D.ny, last)] == epoch ||
         col_epoch[min(row + D.ny + 1, last)] == epoch;
}

// One thread per ROW (x, y) of wz words, one block of the scan per WAVE (64 rows): a thread per word was 250 000 waves of
// four stamp loads and a store -- 30 rounds of resident waves waiting for a load each, 103 us -- and the four words of a
// row share their stamps.
//
// Which blocks a wave works on.  The volume stamps every CHUNK of 64 columns it writes into (lt_tsdf.hip), and a block of 64
// rows r .. r + 63 depends on the chunks of the rows r, r + 1, r + ny, r + ny + 1: four flags.  Five blocks in six of a
// street scene are clean (their counts already hold 0, see lt_mesh).  A wave takes LT_MC_BLOCKS_PER_WAVE blocks: its first
// lanes read the flags of one block each, a ballot finds the live ones, and the wave walks those -- 7 816 waves instead of
// 62 500, of which most loaded their flags and left.  The blocks of a wave are a stride apart (block = lane x number of
// waves + wave, lt_deal_count): written chunks come in clusters, dealt this way every wave gets its share (1.4 live
// blocks on average, 4 at most).  What the kernel's time is made of (per-wave wall-clock stamps, tools/mc_wave_times.py):
// a live block is a chain of four dependent round trips to cold memory -- case table, chunk flags, the rows' stamps, the
// sign words: 0.9 us each in this kernel, 0.35 us on an idle chip -- plus 3-4 us of cell loops for the slowest lane: 7.6 us
// for a wave with one block, 11 us with two; the slots are 0.2 busy.
#ifndef LT_MC_BLOCKS_PER_WAVE
#define LT_MC_BLOCKS_PER_WAVE 8
#endif
// a word with more cells than this is counted by the wave (count_cells_wave) ...
#ifndef LT_MC_HEAVY
#define LT_MC_HEAVY 16  // (swept on the default volume: 2: 50 us, 4: 39, 6: 38, 10 .. 24: 32-33, 40: 35, never: 39)
#endif
// ... unless more lanes than this hold such a word (word_by_wave)
#ifndef LT_MC_HEAVY_LANES
#define LT_MC_HEAVY_LANES 8   // (swept: 4 .. 12: 31.5 us, 20 .. 32: 32.4, 64 = never walked: 37.5)
#endif
#define LT_MC_QW 96  // ambiguous cells a wave buffers in LDS per block of 64 rows (amb_buffer)

// A wave's blocks, for k_mc_words and k_mc_compact alike: the kernels differ in what makes a block live.
struct sweep_deal {
  int n_waves, wave;  // waves of the launch, this one's number
  u64 live;           // bit l: block l * n_waves + wave is still to be walked (the ballot of the kernel's predicate)
};
__device__ __forceinline__ sweep_deal sweep_deal_of() {
  const int n_waves = gridDim.x * 4, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  return {n_waves, wave, 0ull};
}
__device__ __forceinline__ int sweep_block(const sweep_deal& d, int l) { return l * d.n_waves + d.wave; }
// lane `lane` looks at a block of its own
__device__ __forceinline__ bool sweep_mine(const sweep_deal& d, int lane, int n_blocks) {
  return lane < LT_MC_BLOCKS_PER_WAVE && sweep_block(d, lane) < n_blocks;
}
__device__ __forceinline__ int sweep_next(sweep_deal& d) {  // the next live block (wave-uniform), taken off the mask
  const int b = sweep_block(d, __ffsll((long long)d.live) - 1);
  d.live &= d.live - 1;
  return b;
}

__device__ __forceinline__ bool mc_block_live(const unsigned* __restrict__ chunk_epoch, unsigned epoch, const mc_dims& D,
                                              int b, int n_chunks) {
  if (!chunk_epoch) return true;
  const int q = (b * 64 + D.ny) >> 6;
  bool any = false;
  const int ch[4] = {b, b + 1, q, q + 1};
#pragma unroll
  for (int k = 0; k < 4; ++k) any = any || (ch[k] < n_chunks && chunk_epoch[min(ch[k], n_chunks - 1)] == epoch);
  return any;
}

// one block of 64 rows as a lane of its wave sees it: the lane's row and what the row has summed up so far
struct mc_block {
  int id, lane;    // the block (wave-uniform) and the lane: row = 64 id + lane
  int row, rowc;   // rowc: the row, or the volume's last where the block reaches beyond it
  int x, y;        // of rowc
  bool rowlive;    // the row exists and it or a neighbour was written (a clean row writes nothing: its words hold 0 -- no
                   // active word of the last extraction is left, k_mc_clear)
  unsigned na, nv, nt;  // the row's active words, vertices, triangles
};
__device__ __forceinline__ mc_block mc_block_of(const mc_dims& D, int id, int lane, const unsigned* __restrict__ col_epoch,
                                                unsigned epoch) {
  mc_block B;
  const int n_rows = D.nx * D.ny;
  B.id = id;
  B.lane = lane;
  B.row = id * 64 + lane;
  B.na = B.nv = B.nt = 0;
  B.rowlive = B.row < n_rows && mc_rows_dirty(col_epoch, epoch, D, B.row);
  B.rowc = min(B.row, n_rows - 1);
  B.x = mc_x_of(D, B.rowc);
  B.y = B.rowc - B.x * D.ny;
  return B;
}

// ---- a row's sign words ----
// Two loaders.  Up to four words a row (D.wz <= 4, the default volume): the sign words of the four rows (x + dx, y + dy),
// ALL loaded before the first is used -- a word's masks need its row neighbours' words at k and k + 1, so a loop over k
// loaded every word twice, in wz dependent rounds.  That takes 16 words in registers under constant indices (an unrolled
// loop); longer rows load the eight words of word k when its turn comes (mc_load).
struct mc_row_words { u64 w[4][5]; };
__device__ __forceinline__ mc_row_words row_words_load(const mc_sweep_args& a, const mc_block& B) {
  const mc_dims& D = a.D;
  const bool hx = B.x + 1 < D.nx, hy = B.y + 1 < D.ny;
  mc_row_words R;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dx = q & 1, dy = q >> 1;
    const bool have = B.rowlive && (dx == 0 || hx) && (dy == 0 || hy);
    const size_t base = (size_t)(B.rowc + (have ? dx * D.ny + dy : 0)) * D.wz;
#pragma unroll
    for (int k = 0; k < 4; ++k) R.w[q][k] = (have && k < D.wz) ? a.bits[base + k] : 0ull;
    R.w[q][4] = 0ull;
  }
  return R;
}
// the masks of word k of the lane's row: from the words loaded ahead (R; k a constant then) or, without them, from memory
__device__ __forceinline__ mc_masks row_masks(const mc_sweep_args& a, const mc_block& B, const mc_row_words* R, int k) {
  if (R) {
    u64 w8[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) { w8[q] = R->w[q][k]; w8[q | 4] = R->w[q][k + 1]; }
    return mc_build(w8, a.D, B.x, B.y, k);  // (a row that is not live holds zeros: no edge, no cell)
  }
  mc_masks M = mc_load(a.bits, a.D, B.x, B.y, k);
  if (!B.rowlive) { M.ex = M.ey = M.ez = M.ac = 0ull; }
  return M;
}

// ---- the ambiguous cells' queue ----
// the ambiguous cells a wave meets in one block of 64 rows, collected in LDS and appended to the queue with ONE global
// atomic (a returning atomic per cell on the one counter -- 14 500 of them on a street scene -- doubled the kernel's time)
// One per wave; n may exceed LT_MC_QW (amb_push).  An entry is the queue's uint2 as ONE word, x | y << 32, written with one
// store: as a uint2 its halves are stored apart, and the compiler merges the second half's store with that of the queue's own
// entry in amb_push -- one store through a FLAT pointer that is either LDS or global (seen in the assembly).
struct amb_buffer { u64 e[LT_MC_QW]; int n; };
__device__ __forceinline__ void amb_begin(amb_buffer& Q, int lane) {
  if (lane == 0) Q.n = 0;
  __builtin_amdgcn_wave_barrier();
}
// the cell at voxel (xx, yy, z) with case cs, met in block `blkid`: queued for k_mc_amb; counts 0 here
__device__ __forceinline__ unsigned amb_push(amb_buffer& Q, const mc_sweep_args& a, int blkid, int xx, int yy, int z, unsigned cs) {
  const mc_amb& A = a.A;
  const uint2 e = make_uint2((unsigned)((xx * a.D.ny + yy) * a.D.nz + z), cs | ((unsigned)blkid << 8));
  const int slot = atomicAdd(&Q.n, 1);  // (LDS)
  if (slot < LT_MC_QW) Q.e[slot] = (u64)e.x | ((u64)e.y << 32);
  else {  // (more than the buffer holds in one block of rows: straight to the queue)
    const unsigned sh = (unsigned)blkid & (LT_MC_SHARDS - 1);
    const unsigned pos = (unsigned)atomicAdd(A.counter + sh * LT_MC_CTR_STRIDE, 1);
    if (pos < A.cap) A.queue[(size_t)sh * A.cap + pos] = e;
  }
  return 0u;
}
// the block's ambiguous cells -> the queue
__device__ __forceinline__ void amb_flush(amb_buffer& Q, const mc_amb& A, int blkid, int lane) {
  __builtin_amdgcn_wave_barrier();
  const int nq = min(Q.n, LT_MC_QW);  // (wave-uniform)
  if (nq > 0) {
    unsigned base = 0;
    const unsigned sh = (unsigned)blkid & (LT_MC_SHARDS - 1);
    if (lane == 0) base = (unsigned)atomicAdd(A.counter + sh * LT_MC_CTR_STRIDE, nq);
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    for (int j = lane; j < nq; j += 64)
      if (base + (unsigned)j < A.cap) A.queue[(size_t)sh * A.cap + base + j] = make_uint2((unsigned)Q.e[j], (unsigned)(Q.e[j] >> 32));
  }
}

// ---- counting one word ----
// triangles per case: the loops below look it up once per active cell, a chain of dependent loads that is three times
// shorter through LDS.  0x80: an ambiguous case of Lewiner's (3, 4, 6, 7, 10, 12, 13) -- the cell's eight VALUES decide
// (k_mc_amb; 1-2 % of a street scene's cells).  256 threads, one case each; the caller's barrier follows.
__device__ __forceinline__ void case_counts_stage(unsigned char* s_nt) {
  const unsigned fx = LT_LWC_FIXED[threadIdx.x];
  s_nt[threadIdx.x] = fx == 0xFFFFFFFFu ? 0x80 : (unsigned char)LW_NT(fx);
}

// Triangles of a word = sum over its active cells of the case's count.  A lane walking its own cells is a chain of
// ~60 instructions and an LDS look-up per cell, and a row through a wall along z has 60 active cells a word: its wave
// waits for that one lane, and the launch for its slowest waves.  Words with more than LT_MC_HEAVY cells are therefore
// counted by the WAVE, a lane per cell: the owner's eight corner masks are broadcast (v_readlane), every lane looks up
// its cell, three ballots add the counts up (42 -> 32 us on the default volume, with the threshold swept and the lanes'
// own loops on 32-bit half words).
// ... unless MANY lanes hold such a word (a wall across the block's rows): the wave's turn costs ~90 instructions
// per heavy word, the lanes' own loops ~25 per cell of the fullest lane -- 64 heavy words at once are cheaper walked
__device__ __forceinline__ bool word_by_wave(const mc_masks& M) {  // (called by all 64 lanes)
  bool heavy = __popcll(M.ac) > LT_MC_HEAVY;
  if (__popcll(__ballot(heavy)) > LT_MC_HEAVY_LANES) heavy = false;
  return heavy;
}
// the lane's own loop -> triangles of word k of its row (ambiguous cells: queued, 0)
__device__ __forceinline__ unsigned count_cells_lane(const mc_sweep_args& a, const mc_block& B, amb_buffer& Q,
                                                     const unsigned char* s_nt, const mc_masks& M, int k) {
  unsigned t = 0;
  // the word's halves one after the other: with 32-bit masks a cell is 8 x (v_bfe_u32, v_lshl_or_b32) + a 32-bit
  // find-first / clear-lowest, a third of the instructions of the 64-bit shifts of mc_case
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    unsigned ac = (unsigned)(M.ac >> (32 * h));
    if (ac == 0u) continue;
    unsigned m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      m[i] = (unsigned)(((i & 4) ? M.s[i & 1][(i >> 1) & 1] : M.m[i & 1][(i >> 1) & 1]) >> (32 * h));
    for (; ac; ac &= ac - 1) {
      const int b = __ffs((int)ac) - 1;
      unsigned cs = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) cs |= ((m[i] >> b) & 1u) << i;
      const unsigned n = s_nt[cs];
      t += (n & 0x80u) ? amb_push(Q, a, B.id, B.x, B.y, k * 64 + 32 * h + b, cs) : n;
    }
  }
  return t;
}
// the wave's turns: every lane whose word is `heavy` has it counted by all 64, a lane per cell, and receives the sum
// (triangles | centre vertices << 16) in t; the other lanes keep theirs.  (Called by all 64 lanes.)
__device__ __forceinline__ unsigned count_cells_wave(const mc_sweep_args& a, const mc_block& B, amb_buffer& Q,
                                                     const unsigned char* s_nt, const mc_masks& M, int k, bool heavy, unsigned t) {
  const int lane = B.lane;
  for (u64 hm = __ballot(heavy); hm; hm &= hm - 1) {
    const int r = __ffsll((long long)hm) - 1;  // (wave-uniform)
    int cs = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u64 m = (i & 4) ? M.s[i & 1][(i >> 1) & 1] : M.m[i & 1][(i >> 1) & 1];
      const u64 mr = (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)m, r) |
                     ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(m >> 32), r) << 32);
      cs |= (int)((mr >> lane) & 1ull) << i;
    }
    const u64 ac = (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)M.ac, r) |
                   ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(M.ac >> 32), r) << 32);
    unsigned n = ((ac >> lane) & 1ull) ? s_nt[cs] : 0u;  // (<= 12, or the marker)
    if (n & 0x80u)  // (the OWNER's x, y: broadcast like its masks)
      n = amb_push(Q, a, B.id, __builtin_amdgcn_readlane(B.x, r), __builtin_amdgcn_readlane(B.y, r), k * 64 + lane, (unsigned)cs);
    const unsigned tot = __popcll(__ballot(n & 1u)) + 2u * __popcll(__ballot(n & 2u)) + 4u * __popcll(__ballot(n & 4u)) +
                         8u * __popcll(__ballot(n & 8u)) + ((unsigned)__popcll(__ballot(n >> 16)) << 16);
    if (lane == r) t = tot;
  }
  return t;
}
// word k of this lane's row is done: its count (vertices | triangles << 16) stored, the row's three sums kept
__device__ __forceinline__ void sweep_word(const mc_sweep_args& a, mc_block& B, amb_buffer& Q, const unsigned char* s_nt,
                                           const mc_masks& M, int k) {  // (called by all 64 lanes)
  const bool heavy = word_by_wave(M);
  const unsigned own = heavy ? 0u : count_cells_lane(a, B, Q, s_nt, M, k);
  const unsigned tc = count_cells_wave(a, B, Q, s_nt, M, k, heavy, own), t = tc & 0xFFFFu;
  const unsigned v = __popcll(M.ex) + __popcll(M.ey) + __popcll(M.ez) + (tc >> 16);
  if (B.rowlive) a.cnt[(size_t)B.row * a.D.wz + k] = v | (t << 16);
  B.na += (v | t) ? 1u : 0u; B.nv += v; B.nt += t;
}

// ---- the block's totals ----
// the wave sum of the rows' triples (20 bits each: the host checks wz, see pack3) and the four stores
__device__ __forceinline__ void block_totals_store(const mc_sweep_args& a, const mc_block& B) {
  const mc_triple s = unpack3(wave_sum3(pack3(B.na, B.nv, B.nt)));
  if (B.lane == 0) {
    blk_store3(a.blk, B.id, s);
    a.wave_na[B.id] = (int)s.a;
  }
}
__device__ __forceinline__ void block_totals_clean(const mc_sweep_args& a, int b) {  // (cnt already holds 0 for the words of a clean block)
  blk_store3(a.blk, b, {0u, 0u, 0u});
  a.wave_na[b] = 0;
}

__global__ __launch_bounds__(256) void k_mc_words(mc_amb A, const u64* __restrict__ bits, mc_dims D, unsigned* __restrict__ cnt,
                                                  int* __restrict__ blk, const unsigned* __restrict__ col_epoch,
                                                  unsigned epoch, const unsigned* __restrict__ chunk_epoch,
                                                  int* __restrict__ wave_na, int n_blocks) {
  const mc_sweep_args a = {D, bits, cnt, blk, wave_na, n_blocks, A};  // (in mc_sweep_args' order)
  const int n_chunks = (D.nx * D.ny + 63) / 64;
  __shared__ unsigned char s_nt[256];
  __shared__ amb_buffer s_q[4];
  case_counts_stage(s_nt);
  amb_buffer& Q = s_q[threadIdx.x >> 6];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  sweep_deal dl = sweep_deal_of();
  LT_MC_STAMP_AT(1, dl.wave, 0, wall_clock64());
  {
    const int b = sweep_block(dl, lane);
    const bool mine = sweep_mine(dl, lane, a.n_blocks);
    const bool act = mine && mc_block_live(chunk_epoch, epoch, D, b, n_chunks);
    if (mine && !act) block_totals_clean(a, b);
    dl.live = __ballot(act);
  }
  LT_MC_STAMP_AT(1, dl.wave, 1, wall_clock64());
  LT_MC_STAMP_AT(1, dl.wave, 3, (unsigned long long)__popcll(dl.live));
  while (dl.live) {
    const int id = sweep_next(dl);
    amb_begin(Q, lane);
    mc_block B = mc_block_of(D, id, lane, col_epoch, epoch);
    if (D.wz <= 4) {  // (wave-uniform; the two loaders: row_words_load)
      const mc_row_words R = row_words_load(a, B);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= D.wz) break;  // (wave-uniform)
        sweep_word(a, B, Q, s_nt, row_masks(a, B, &R, k), k);
      }
    } else {
      for (int k = 0; k < D.wz; ++k) sweep_word(a, B, Q, s_nt, row_masks(a, B, nullptr, k), k);
    }
    amb_flush(Q, a.A, id, lane);
    block_totals_store(a, B);
  }
  LT_MC_STAMP_AT(1, dl.wave, 2, wall_clock64());
}

// ---- k_mc_amb: the queued ambiguous cells, one lane each ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mc_amb(const float* __restrict__ tsdf, mc_dims D, mc_amb A, unsigned* __restrict__ cnt,
                                                int* __restrict__ blk, int* __restrict__ wave_na) {
  // workgroup g: shard g % 64, its chunks of 256 cells g / 64, g / 64 + gridDim / 64, ...
  const unsigned sh = blockIdx.x & (LT_MC_SHARDS - 1), per = max(gridDim.x / LT_MC_SHARDS, 1u);
  const unsigned n = min((unsigned)A.counter[sh * LT_MC_CTR_STRIDE], A.cap);
  const uint2* __restrict__ queue = A.queue + (size_t)sh * A.cap;
  const size_t sz = (size_t)D.vs, sy = (size_t)D.nz * sz, sx = (size_t)D.ny * sy;
  // a workgroup takes 256 queued cells and deals them to its lanes SORTED by Lewiner's case (counting sort in LDS): the seven
  // ambiguous cases run different tests, and a wave pays for every case its lanes hold
  __shared__ uint2 s_e[256];
  __shared__ int s_n[16], s_o[16];
  const int tid = threadIdx.x;
  for (unsigned base = (blockIdx.x / LT_MC_SHARDS) * 256; base < n; base += per * 256) {  // (workgroup-uniform)
    if (tid < 16) s_n[tid] = 0;
    __syncthreads();
    const bool valid = base + tid < n;
    uint2 e0 = make_uint2(0u, 0u);
    int bucket = 0, rank = 0;
    if (valid) {
      e0 = queue[base + tid];
      bucket = LT_LWC_CASE[e0.y & 255u];  // 3, 4, 6, 7, 10, 12, 13
      rank = atomicAdd(&s_n[bucket], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int o = 0;
      for (int k = 0; k < 16; ++k) { s_o[k] = o; o += s_n[k]; }
    }
    __syncthreads();
    if (valid) s_e[s_o[bucket] + rank] = e0;
    __syncthreads();
    if (!valid) continue;  // (no barrier below)
    const uint2 e = s_e[tid];
    const unsigned i = e.x;
    const int cs = (int)(e.y & 255u), b = (int)(e.y >> 8);
    const unsigned sel = lw_cell_eval(tsdf + (size_t)i * sz, sx, sy, sz, cs);
    for (unsigned h = amb_slot(i, A.tmask);; h = (h + 1) & A.tmask)  // (every cell is queued once: the slot is free or foreign)
      if (atomicCAS(&A.table[h].x, 0u, i + 1u) == 0u) { A.table[h].y = sel; break; }
    const unsigned nt = LW_NT(sel), c = LW_C(sel);
    if (nt) {
      const unsigned row = i / (unsigned)D.nz, z = i - row * (unsigned)D.nz;
      const unsigned old = atomicAdd(&cnt[(size_t)row * D.wz + (z >> 6)], c | (nt << 16));
      blk_add3(blk, b, {0u, c, nt});
      if (old == 0u) { blk_add3(blk, b, {1u, 0u, 0u}); atomicAdd(&wave_na[b], 1); }  // the word becomes an active word
    }
  }
}

// undo the last extraction's entries of cnt / cmap (its records are still there): both arrays are back to 0 / -1
// ... and of the ambiguous cells' tiling table (its queue is still there too): every queued cell empties its own slot
__global__ __launch_bounds__(256) void k_mc_clear(const mc_rec* __restrict__ rec, int n, unsigned* __restrict__ cnt,
                                                  int* __restrict__ cmap, mc_amb A, int n_amb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  // n_amb: the largest shard's count of the last extraction; thread i < 64 n_amb looks at entry i % n_amb of shard i / n_amb
  const int sh = n_amb > 0 ? i / n_amb : LT_MC_SHARDS, j = n_amb > 0 ? i - sh * n_amb : 0;
  if (sh < LT_MC_SHARDS && j < A.counter[LT_MC_SHARDS * LT_MC_CTR_STRIDE + sh]) {
    const unsigned key = A.queue[(size_t)sh * A.cap + j].x + 1u;
    unsigned h = amb_slot(key - 1u, A.tmask);
    for (unsigned tries = 0; tries <= A.tmask; ++tries, h = (h + 1) & A.tmask)  // (not stopped by slots others emptied)
      if (A.table[h].x == key) { A.table[h].x = 0u; break; }
  }
  if (i >= n) return;
  const int w = rec[i].w;
  cnt[w] = 0u;
  cmap[w] = -1;
}

// ---- k_mc_scan1 / k_mc_scan2: exclusive scan of the per-workgroup totals in two levels -------------------------------
// level 1: workgroup g scans its segment of 256 totals in place (coalesced) and leaves the segment's sums in seg[3g..];
// level 2: one workgroup scans the (<= 1024) segment sums in place and writes the grand totals.  k_mc_compact adds
// seg[3 * (block / 256) + k] to the block's in-segment prefix.  (A single workgroup walking all 62 500 totals of the
// default volume took 143 us: one CU's L2 bandwidth.)
__global__ __launch_bounds__(256) void k_mc_scan1(int* __restrict__ blk, int n_blocks, int* __restrict__ seg) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  mc_triple mine = {0u, 0u, 0u};
  if (b < n_blocks) mine = blk_load3(blk, b);
  // (the 20-bit packing of pack3 would overflow here -- 256 x 81 920 triangles: three 64-bit scans)
  u64 p[3] = {mine.a, mine.v, mine.t}, inc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) inc[k] = wave_incl_scan(p[k]);
  __shared__ u64 ws[3][4];
  if ((threadIdx.x & 63) == 63)
    for (int k = 0; k < 3; ++k) ws[k][threadIdx.x >> 6] = inc[k];
  __syncthreads();
  u64 off[3] = {0, 0, 0}, tot[3];
  for (int k = 0; k < 3; ++k) {
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off[k] += ws[k][w];
    tot[k] = (ws[k][0] + ws[k][1]) + (ws[k][2] + ws[k][3]);
  }
  // (saturated: the host refuses a mesh of 2^31 - 1 vertices / faces)
  if (b < n_blocks) {
    unsigned ex[3];
    for (int k = 0; k < 3; ++k) ex[k] = (unsigned)min(off[k] + inc[k] - p[k], (u64)2147483647);
    blk_store3(blk, b, {ex[0], ex[1], ex[2]});
  }
  if (threadIdx.x == 0)  // (the segment's triple, laid out like a block's: k_mc_compact reads it with blk_load3)
    for (int k = 0; k < 3; ++k) seg[3 * blockIdx.x + k] = (int)min(tot[k], (u64)2147483647);
}

__global__ __launch_bounds__(1024) void k_mc_scan2(int* __restrict__ seg, int n_seg, int* __restrict__ totals,
                                                   int* __restrict__ amb_counter, int amb_cap) {
  __shared__ long long part[3][1024];
  const int t = threadIdx.x;
  long long s[3] = {0, 0, 0};
  if (t < n_seg)
    for (int k = 0; k < 3; ++k) s[k] = seg[3 * t + k];
  for (int k = 0; k < 3; ++k) part[k][t] = s[k];
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    long long v[3];
    for (int k = 0; k < 3; ++k) v[k] = t >= o ? part[k][t - o] : 0;
    __syncthreads();
    for (int k = 0; k < 3; ++k) part[k][t] += v[k];
    __syncthreads();
  }
  if (t < n_seg)
    for (int k = 0; k < 3; ++k) seg[3 * t + k] = (int)min(part[k][t] - s[k], 2147483647ll);
  if (t < 64) {  // the ambiguous cells queued per shard (k_mc_amb is done): kept for k_mc_clear, re-armed for the next extraction
    const int c = amb_counter[t * LT_MC_CTR_STRIDE];
    amb_counter[LT_MC_SHARDS * LT_MC_CTR_STRIDE + t] = min(c, amb_cap);
    amb_counter[t * LT_MC_CTR_STRIDE] = 0;
    int mx = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (t == 0) totals[3] = mx;  // the fullest shard (beyond the capacity: the host grows the buffers and starts over)
  }
  if (t == 1023)
    for (int k = 0; k < 3; ++k) totals[k] = (int)min(part[k][1023], 2147483647ll);
}

// ---- k_mc_compact ----------------------------------------------------------------------------------------------------
// the row's counts: up to four words ALL loaded before the first is used and kept for row_records_store (a rolled loop
// waited for every load before it issued the next, twice: eight dependent round trips per block of rows)
struct mc_row_counts {
  unsigned c4[4];  // the words' counts when there are `few` (D.wz <= 4)
  mc_triple sum;   // the row's triple
};
__device__ __forceinline__ mc_row_counts row_counts_load(const unsigned* __restrict__ cnt, const mc_dims& D, int row, bool few) {
  unsigned na = 0, nv = 0, nt = 0, c4[4] = {0u, 0u, 0u, 0u};
  if (few) {
#pragma unroll
    for (int k = 0; k < 4; ++k) c4[k] = k < D.wz ? cnt[(size_t)row * D.wz + k] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) { na += c4[k] ? 1u : 0u; nv += c4[k] & 0xFFFFu; nt += c4[k] >> 16; }
  } else {
    for (int k = 0; k < D.wz; ++k) {
      const unsigned c = cnt[(size_t)row * D.wz + k];
      na += c ? 1u : 0u; nv += c & 0xFFFFu; nt += c >> 16;
    }
  }
  return {{c4[0], c4[1], c4[2], c4[3]}, {na, nv, nt}};
}
// the records of the row's active words and the cmap entries of all its words; at: (compact index, vertex base, triangle
// base) of the row's first active word
__device__ __forceinline__ void row_records_store(const u64* __restrict__ bits, const mc_dims& D, const unsigned* __restrict__ cnt,
                                                  int row, bool few, const mc_row_counts R, const mc_triple& at,
                                                  int* __restrict__ cmap, mc_rec* __restrict__ rec, int cap_rec) {
  int ci = (int)at.a, vb = (int)at.v, tb = (int)at.t;
  const int x = mc_x_of(D, row), y = row - x * D.ny;
  for (int k = 0; k < D.wz; ++k) {
    const int w = row * D.wz + k;
    const unsigned c = few ? (k == 0 ? R.c4[0] : k == 1 ? R.c4[1] : k == 2 ? R.c4[2] : R.c4[3]) : cnt[w];
    int mine_ci = -1;
    if (c) {
      if (ci < cap_rec) {
        const mc_masks M = mc_load(bits, D, x, y, k);
        mc_rec r;
        r.w = w;
        r.vbase = vb;
        r.tbase = tb;
        r.ex = M.ex; r.ey = M.ey; r.ez = M.ez;
        // triangles of the word (k_mc_emit_batch: the extent of a batch) | its centre vertices << 16
        r.pad = (int)((c >> 16) | (((c & 0xFFFFu) - (unsigned)(__popcll(M.ex) + __popcll(M.ey) + __popcll(M.ez))) << 16));
        rec[ci] = r;
        mine_ci = ci;
      }
      ++ci; vb += (int)(c & 0xFFFFu); tb += (int)(c >> 16);
    }
    cmap[w] = mine_ci;
  }
}

__global__ __launch_bounds__(256) void k_mc_compact(const u64* __restrict__ bits, mc_dims D,
                                                    const unsigned* __restrict__ cnt, const int* __restrict__ blk,
                                                    const int* __restrict__ seg, int* __restrict__ cmap,
                                                    mc_rec* __restrict__ rec, int cap_rec,
                                                    const int* __restrict__ wave_na, int n_blocks) {
  // thread = row, scan block = a wave's turn (as in k_mc_words, and dealt the same way: sweep_deal); compact order = word order
  const int n_rows = D.nx * D.ny;
  const int lane = threadIdx.x & 63;
  sweep_deal dl = sweep_deal_of();
  LT_MC_STAMP_AT(2, dl.wave, 0, wall_clock64());
  // no active word in a block's 64 rows (most): nothing to rank, and their cmap entries are -1 already (lt_mesh)
  dl.live = __ballot(sweep_mine(dl, lane, n_blocks) && wave_na[min(sweep_block(dl, lane), n_blocks - 1)] != 0);
  LT_MC_STAMP_AT(2, dl.wave, 1, wall_clock64());
  LT_MC_STAMP_AT(2, dl.wave, 3, (unsigned long long)__popcll(dl.live));
  while (dl.live) {
    const int id = sweep_next(dl), row = id * 64 + lane;
    const bool few = D.wz <= 4;  // (wave-uniform)
    mc_row_counts R = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u}};
    if (row < n_rows) R = row_counts_load(cnt, D, row, few);
    const u64 p = pack3(R.sum.a, R.sum.v, R.sum.t);
    const mc_triple in_blk = unpack3(wave_incl_scan(p) - p);  // the rows before this one in the block
    if (row >= n_rows) continue;
    const mc_triple sg = blk_load3(seg, id >> 8), in_seg = blk_load3(blk, id);
    row_records_store(bits, D, cnt, row, few, R, {sg.a + in_seg.a + in_blk.a, sg.v + in_seg.v + in_blk.v, sg.t + in_seg.t + in_blk.t},
                      cmap, rec, cap_rec);
  }
  LT_MC_STAMP_AT(2, dl.wave, 2, wall_clock64());
}

// ---- emission ----------------------------------------------------------------------------------------------------------
struct mc_nb { u64 ex, ey, ez; int vbase; int have; };

// float32 vertex coordinate along the edge from lattice coordinate c (value v1) to c + 1 (value v2): scikit-image's
// centre-of-mass rule (Cell._add_face_from_edge_index), evaluated in double, stored as float32
// (its `FLT_EPSILON` is, despite the name, `np.spacing(1.0)` = 2^-52 -- a double; C's FLT_EPSILON, 1.19e-7, would move
// every vertex by ~1e-7 voxel and exact-zero samples visibly.  Pinned: golden F10 of the real scikit-image, bit for bit.)
__device__ __forceinline__ float mc_edge_coord(int c, float v1, float v2) {
  const double w1 = 1.0 / (LT_MC_EPS + fabs((double)v1));
  const double w2 = 1.0 / (LT_MC_EPS + fabs((double)v2));
  return (float)((double)c + w2 / (w1 + w2));
}

// ---- k_mc_emit_batch: one wave per K = LT_MC_K consecutive active words, one lane per VERTEX / per TRIANGLE ------------------
// A wave per active word with a lane per voxel (rounds 1-2) spent its time issuing instructions for idle lanes: on the default volume's street scene an active word owns
// 3.6 vertices and 7.3 triangles, so the double-precision vertex rule (three IEEE divisions), unrolled over the three edge
// axes, and the 5 x 3 unrolled index computations run with 2-4 of 64 lanes live -- 252 000 waves x ~3 300 cycles = the
// kernel's 265 us (more words per wave or a lane per word change nothing: 272 / 332 us measured).  Here a wave takes K
// words, lists their vertices and triangles in LDS (in output order: the lists ARE the output ranges, a batch's words
// are consecutive), and then lane j computes vertex j / triangle j: every lane live, every store coalesced.
// LDS decides how many batches a CU holds, in granules of 1 280 B per WORKGROUP (tools/occ_probe.hip fine): the 30 224 B of
// four waves are 24 granules = 5 workgroups = 20 waves per CU (one-wave workgroups of 7 752 B held 18).  Six workgroups
// (<= 26 880 B and <= 80 registers: lists of 128, the tiling table back in global memory) were built and measured: 90 us
// against 80 -- a batch is ~1 400 instructions (924 vector: staging 155, cells 222, vertices 283, triangles 263,
// tools/mc_sections.sh; 362 scalar, 102 LDS) and ONE wave issues an instruction every 5-7 cycles whatever runs beside it
// (profiles/r03/valu_calib.txt: 4.7 cycles alone, 7.2 with eight waves per SIMD): 3-4 us of a batch's 8.4 are its own
// instruction stream, which more waves do not shorten and fewer registers (= more instructions) lengthen.
#define LT_MC_VCAP 256   // list windows; a batch with more vertices / triangles is emitted in several passes
#define LT_MC_TCAP 256
#define LT_MC_EW 4  // waves per workgroup of the emission
#define LT_MC_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#ifndef LT_MC_K
#define LT_MC_K 8  // active words per batch (swept 2 / 4 / 8 / 16: profiles/r04/DESIGN_rounds_1_to_4.md; 16 halves the occupancy)
#endif
static_assert(LT_MC_K >= 1 && LT_MC_K <= 16, "list entries hold the word in 4 bits");
static_assert(64 * LT_MC_EW == 256, "the tiling table is staged by 256 threads");

// what the host hands over (mc_emit_args_of); by value into the kernel, by const& into its phases
struct mc_emit_args {
  const float* tsdf; const float* color_vol; const float* rem_vol;  // (AOS: all three the one array of records)
  const u64* bits; mc_dims D; const int* cmap;
  const mc_rec* rec; int n_active;
  float voxel_size, ox, oy, oz;
  float* verts; int* faces; int* colors; float* rem;
  int cap_v, cap_f;
  mc_amb A;
  int xcd_map;
};

// ONE wave's working set in LDS.  LT_MC_EW waves per workgroup, each with a set of its own and no business with the others:
// what would be a workgroup barrier orders ONE wave's LDS accesses, which the hardware executes in order anyway --
// LT_MC_WSYNC only keeps the compiler from moving them.  (Four waves instead of one per workgroup change nothing by
// themselves -- 82.7 us both; they share the tiling table s_lwc, 256 B of LDS per wave instead of 1 KB: 80 us; 75 on a
// volume of records, AOS.)  Size for K = 8: 7 300 B of members, 7 312 B with the 16-byte alignment that lets the compiler read
// the 40-byte records with ds_read_b128 (8-byte alignment: 7 304 B and pairs of ds_read2_b64) -- 30 272 B per workgroup with
// s_lwc, 24 granules of 1 280 B like the 30 224 B of twelve separate arrays.
struct alignas(16) mc_batch {
  mc_rec rec[LT_MC_K];
  int xyz[LT_MC_K][3];       // x, y, wz of the words
  size_t base[LT_MC_K];      // ... and the voxel index of their first voxel
  mc_nb nb[LT_MC_K][8];      // records of the 8 words a cell's triangles can reference
  u64 cm[LT_MC_K][9];        // corner masks m[dx][dy], s[dx][dy] (mc_masks) and the active-cell mask of the words
  union {
    u64 sg[LT_MC_K][8];      // sign words of the cell corners, [dx | dy << 1 | dw << 2] -- dead once the corner masks are built, where
    unsigned short vl[LT_MC_VCAP];  // vertex j of the window: k | b << 4 | axis << 10 (12 bits; axis 3 = the cell's centre vertex) begins its life
  };
  unsigned short tl[LT_MC_TCAP];    // triangle j of the window: index into cl | t << 10
  unsigned cl[LT_MC_K * 64];        // active cells of the batch in order: k | b << 4 | triangles << 10 | centre << 14 | tiling offset << 15
  unsigned short ct[LT_MC_K * 64];  // ... and the (batch-relative) index of their first triangle (< 16 x 64 x 12)
  u64 ccm[LT_MC_K];                 // the words' cells that own a centre vertex
  int cpre[LT_MC_K + 1];            // active cells before word k
};
struct mc_extent {  // of one batch, wave-uniform (emit_stage)
  int nw;              // words
  int ncell;           // active cells
  int vbase0, tbase0;  // its first vertex / triangle in the output
  int nvt, ntt;        // its vertices / triangles
};
constexpr int LT_MC_NPV = (8 * LT_MC_K + 63) / 64;  // (word, segment of 8 voxels) pairs per lane

// ---- staging: records and word coordinates; sign words, compact indices, neighbour records; corner masks; the prefix of
// active cells per word
__device__ __forceinline__ mc_extent emit_stage(const mc_emit_args& a, mc_batch& s, int lane, int ci0, mc_stamp& st) {
  const mc_dims& D = a.D;
  mc_extent e;
  e.nw = min(LT_MC_K, a.n_active - ci0);
  const int nw = e.nw;
  const size_t sy = (size_t)D.nz, sx = (size_t)D.ny * D.nz;
  if (lane < nw) {
    const mc_rec r = a.rec[ci0 + lane];
    s.rec[lane] = r;
    const int row = mc_row_of(D, r.w), x = mc_x_of(D, row);
    s.xyz[lane][2] = r.w - row * D.wz;
    s.xyz[lane][0] = x;
    s.xyz[lane][1] = row - x * D.ny;
    s.base[lane] = (size_t)x * sx + (size_t)(row - x * D.ny) * sy + (size_t)(r.w - row * D.wz) * 64;
  }
  LT_MC_WSYNC();
  LT_MC_SECTION(st, 0);  // records
  for (int p = lane; p < 8 * nw; p += 64) {  // (k, slot): sign word and record of the word (x + dx, y + dy, wz + dw)
    const int k = p >> 3, slot = p & 7;
    const int x = s.xyz[k][0], y = s.xyz[k][1], wz = s.xyz[k][2];
    const int dx = slot & 1, dy = (slot >> 1) & 1, dw = slot >> 2;
    const bool have = x + dx < D.nx && y + dy < D.ny && wz + dw < D.wz;
    const int w2 = ((x + dx) * D.ny + (y + dy)) * D.wz + wz + dw;
    u64 sg = 0ull;
    int c2 = -1;
    if (have) {
      sg = a.bits[w2];
      c2 = slot == 0 ? ci0 + k : a.cmap[w2];
    }
    mc_nb nb;
    nb.ex = nb.ey = nb.ez = 0; nb.vbase = 0; nb.have = 0;
    if (c2 >= 0) {
      const mc_rec r2 = a.rec[c2];
      nb.ex = r2.ex; nb.ey = r2.ey; nb.ez = r2.ez; nb.vbase = r2.vbase; nb.have = 1;
    }
    s.sg[k][slot] = sg;
    s.nb[k][slot] = nb;
  }
  LT_MC_WSYNC();
  LT_MC_SECTION(st, 1);  // sign words, compact indices, neighbour records
  if (lane < nw) {  // the cell masks of word `lane`, once
    u64 w8[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w8[q] = s.sg[lane][q];
    const mc_masks M = mc_build(w8, D, s.xyz[lane][0], s.xyz[lane][1], s.xyz[lane][2]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s.cm[lane][q] = M.m[q & 1][q >> 1];
      s.cm[lane][4 + q] = M.s[q & 1][q >> 1];
    }
    s.cm[lane][8] = M.ac;
  }
  {  // active cells before each word (lanes 0 .. nw - 1 hold the words' counts)
    int c = lane < nw ? __popcll(s.cm[lane][8]) : 0;  // (own write: same lane)
#pragma unroll
    for (int o = 1; o < LT_MC_K; o <<= 1) {
      const int q = __shfl_up(c, o, 64);
      if (lane >= o) c += q;
    }
    if (lane < nw) s.cpre[lane + 1] = c;
    if (lane == 0) s.cpre[0] = 0;
    if (lane < LT_MC_K) s.ccm[lane] = 0ull;
  }
  LT_MC_WSYNC();
  const mc_rec first = s.rec[0], last = s.rec[nw - 1];
  e.vbase0 = first.vbase;
  e.tbase0 = first.tbase;
  e.nvt = last.vbase + __popcll(last.ex) + __popcll(last.ey) + __popcll(last.ez) + (last.pad >> 16) - e.vbase0;
  e.ntt = last.tbase + (last.pad & 0xFFFF) - e.tbase0;
  e.ncell = s.cpre[nw];
  return e;
}

// ---- the batch's active cells in order (word, z) with their TILING, and the (batch-relative) index of every cell's first
// triangle: a lane takes one (word, SEGMENT of 8 voxels) pair, lists the cells of its 8 voxels (the word's cell base + a
// popcount below the segment) -- case index from the corner masks, tiling from the table or, for Lewiner's ambiguous cases,
// from k_mc_amb's side table (the tests on the cell's eight values ran there) -- and adds up their triangle counts; ONE wave scan over the lanes
// turns the sums into offsets, and the lane hands them to its cells.  The cells whose tiling has a centre vertex are
// collected per word (ccm): their vertices follow the word's edge vertices in the output.
// (s_lwc: LT_LWC_FIXED in LDS, once per workgroup: a cell's tiling without a global round trip)
__device__ __forceinline__ void emit_cells(const mc_emit_args& a, mc_batch& s, const unsigned* s_lwc, int lane, int nw) {
  const mc_dims& D = a.D;
  int run = 0;  // triangles of the pairs before this round of 64
#pragma unroll
  for (int i = 0; i < LT_MC_NPV; ++i) {
    const int p = lane + 64 * i, k = p >> 3, seg = p & 7;
    unsigned ac8 = 0, ntp = 0;  // ntp: the triangle counts of the segment's cells, 4 bits each, in cell order
    int c0 = 0, tsum = 0;
    if (k < nw) {
      const u64 ac = s.cm[k][8];
      ac8 = (unsigned)(ac >> (8 * seg)) & 255u;
      if (ac8) {
        c0 = s.cpre[k] + __popcll(ac & ((1ull << (8 * seg)) - 1ull));
        unsigned m8[8];  // the corner masks' bits of this segment
#pragma unroll
        for (int q = 0; q < 8; ++q) m8[q] = (unsigned)(s.cm[k][q] >> (8 * seg)) & 255u;
        int c = c0, sh = 0;
        unsigned cm8 = 0;
        // the tilings of the segment's (up to eight) cells: ALL table look-ups first, independent of one another -- a loop
        // over the set bits with the look-up inside was a chain of dependent global loads, one per cell of the fullest lane
        // (the section's 3.0 of a batch's 9.4 us, tools/mc_wave_times.py)
        // case index of voxel bb: bit q = bit bb of corner mask q (mc_case: corner q = dx | dy << 1 | dz << 2) -- the
        // transpose of an 8 x 8 bit matrix (rows = the masks' bytes), three swap steps on a 64-bit word instead of 64
        // single-bit moves
        u64 tm = 0ull;
#pragma unroll
        for (int q = 0; q < 8; ++q) tm |= (u64)m8[q] << (8 * q);
        u64 tt = (tm ^ (tm >> 7)) & 0x00AA00AA00AA00AAull;
        tm ^= tt ^ (tt << 7);
        tt = (tm ^ (tm >> 14)) & 0x0000CCCC0000CCCCull;
        tm ^= tt ^ (tt << 14);
        tt = (tm ^ (tm >> 28)) & 0x00000000F0F0F0F0ull;
        tm ^= tt ^ (tt << 28);
        unsigned selv[8];
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
          const unsigned cs = (unsigned)(tm >> (8 * bb)) & 255u;
          selv[bb] = ((ac8 >> bb) & 1u) ? s_lwc[cs] : 0u;
        }
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
          if (!((ac8 >> bb) & 1u)) continue;
          unsigned sel = selv[bb];
          if (sel == 0xFFFFFFFFu)  // an ambiguous case: the tiling k_mc_amb filed under the cell's voxel index
            sel = amb_lookup(a.A, (unsigned)((s.xyz[k][0] * D.ny + s.xyz[k][1]) * D.nz + s.xyz[k][2] * 64 + 8 * seg + bb));
          const unsigned nt = LW_NT(sel);
          s.cl[c] = (unsigned)k | ((unsigned)(8 * seg + bb) << 4) | (nt << 10) | (LW_C(sel) << 14) | (LW_OFF(sel) << 15);
          cm8 |= LW_C(sel) << bb;
          ntp |= nt << sh;
          tsum += (int)nt;
          ++c; sh += 4;
        }
        if (cm8) atomicOr((unsigned long long*)&s.ccm[k], (unsigned long long)cm8 << (8 * seg));
      }
    }
    int inc = tsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int q = __shfl_up(inc, o, 64);
      if (lane >= o) inc += q;
    }
    int t0 = run + inc - tsum;
    int c = c0;
    for (unsigned a8 = ac8; a8; a8 &= a8 - 1u, ++c, ntp >>= 4) {
      s.ct[c] = (unsigned short)t0;
      t0 += (int)(ntp & 15u);
    }
    run += __shfl(inc, 63, 64);
  }
  LT_MC_WSYNC();
}

// ---- vertices, a window of LT_MC_VCAP at a time: listed, then a lane per vertex
// Listing: a lane takes one (word, SEGMENT of 8 voxels) pair -- 8 K pairs, one per lane for K = 8 --, finds where its
// segment's vertices start in the batch's output range (the word's base + three popcounts below the segment: no search,
// no scan) and walks its own voxels.  A street scene's segment holds 0.45 vertices on average and 24 at most: the walk
// is short where the batch is sparse and costs what a lane-per-voxel pass costs where it is dense (walls along z), so one
// path serves both -- the lane-per-ITEM search it replaces (word by the bases, voxel by a 6-step binary search over
// three 64-bit popcounts) was 277 vector instructions per batch.
// AOS: the three field pointers are one array of (tsdf, weight, colour, remission) records (a TSDF volume, D.vs == 4): an
// edge vertex's two field samples and its attributes -- which are those of one of the edge's two ends -- come with TWO
// 16-byte loads, nothing waits for the vertex rule (separate arrays: four loads, the last two behind the rule)
template <bool AOS>
__device__ __forceinline__ void emit_vertices(const mc_emit_args& a, mc_batch& s, int lane, const mc_extent& e, mc_stamp& st) {
  const mc_dims& D = a.D;
  const int nw = e.nw, vbase0 = e.vbase0, nvt = e.nvt;
  const size_t sy = (size_t)D.nz, sx = (size_t)D.ny * D.nz;
  for (int vb = 0; vb < nvt; vb += LT_MC_VCAP) {
#pragma unroll
    for (int i = 0; i < LT_MC_NPV; ++i) {
      const int p = lane + 64 * i, k = p >> 3, seg = p & 7;
      if (k < nw) {
        const mc_rec R = s.rec[k];
        const unsigned ex8 = (unsigned)(R.ex >> (8 * seg)) & 255u, ey8 = (unsigned)(R.ey >> (8 * seg)) & 255u,
                       ez8 = (unsigned)(R.ez >> (8 * seg)) & 255u;
        unsigned any = ex8 | ey8 | ez8;
        if (any) {
          const u64 below = (1ull << (8 * seg)) - 1ull;
          int j = R.vbase - vbase0 - vb + __popcll(R.ex & below) + __popcll(R.ey & below) + __popcll(R.ez & below);
          const unsigned e0 = (unsigned)k | ((unsigned)(8 * seg) << 4);
          for (; any; any &= any - 1u) {
            const int bb = __ffs((int)any) - 1;
            const unsigned en = e0 + ((unsigned)bb << 4);
            if ((ex8 >> bb) & 1u) { if ((unsigned)j < LT_MC_VCAP) s.vl[j] = (unsigned short)en; ++j; }
            if ((ey8 >> bb) & 1u) { if ((unsigned)j < LT_MC_VCAP) s.vl[j] = (unsigned short)(en | (1u << 10)); ++j; }
            if ((ez8 >> bb) & 1u) { if ((unsigned)j < LT_MC_VCAP) s.vl[j] = (unsigned short)(en | (2u << 10)); ++j; }
          }
        }
        // the centre vertices of the segment's cells: after all edge vertices of the word, in cell order
        const u64 ccm = s.ccm[k];
        unsigned cm8 = (unsigned)(ccm >> (8 * seg)) & 255u;
        if (cm8) {
          int j = R.vbase - vbase0 - vb + __popcll(R.ex) + __popcll(R.ey) + __popcll(R.ez) + __popcll(ccm & ((1ull << (8 * seg)) - 1ull));
          for (; cm8; cm8 &= cm8 - 1u, ++j) {
            const int bb = __ffs((int)cm8) - 1;
            if ((unsigned)j < LT_MC_VCAP) s.vl[j] = (unsigned short)((unsigned)k | ((unsigned)(8 * seg + bb) << 4) | (3u << 10));
          }
        }
      }
    }
    LT_MC_WSYNC();
    LT_MC_SECTION(st, 3);  // vertex list
#if defined(LT_MC_STOP) && LT_MC_STOP == 2  // ... + vertex list
    continue;
#endif
    const int nwin = min(LT_MC_VCAP, nvt - vb);
    for (int j = lane; j < nwin; j += 64) {
      const unsigned en = s.vl[j];
      const int k = en & 15, b = (en >> 4) & 63, ax = (en >> 10) & 3;
      const int x = s.xyz[k][0], y = s.xyz[k][1], z = s.xyz[k][2] * 64 + b;
      const size_t i = s.base[k] + (size_t)b;  // (64-bit multiplications are quarter rate: once per word, not per vertex)
      float p0 = (float)x, p1 = (float)y, p2 = (float)z;
      constexpr size_t VS = AOS ? 4 : 1;
      float rgb, rm;
      if (ax == 3) {
        // the cell's centre vertex (Cell.calculate_center_vertex): the centre of mass of the eight corners with weights
        // 1 / (eps + |v|), summed in Lewiner's corner order (0 .. 7) in double, stored as float32
        const float* c = a.tsdf + i * VS;
        double ff = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0;
#pragma unroll 1  // (rare: a rolled loop keeps the kernel's registers where they were without the centre vertex)
        for (int q = 0; q < 8; ++q) {  // Lewiner's corner q sits at (a0, a1, a2) = (q >> 2, q >> 1 & 1, (q ^ q >> 1) & 1)
          const int a0 = q >> 2, a1 = (q >> 1) & 1, a2 = (q ^ (q >> 1)) & 1;
          const double w = 1.0 / (LT_MC_EPS + fabs((double)c[((size_t)a0 * sx + (size_t)a1 * sy + (size_t)a2) * VS]));
          ff += w;
          if (a2) f2 += w;
          if (a1) f1 += w;
          if (a0) f0 += w;
        }
        p0 = (float)((double)x + f0 / ff); p1 = (float)((double)y + f1 / ff); p2 = (float)((double)z + f2 / ff);
        // verts_ind = np.round(verts).astype(int) on the float32 coordinates (fusion_lidar.py:409).
        // The vertex lies inside a cell (below: on an edge) that starts at voxel (x, y, z): every rounded coordinate is
        // the voxel's or the next one's, and the next one exists where the cell / the edge does.  (Anything else -- a NaN
        // field value, on which numpy would raise -- counts as "the next one": never a wild address.)
        const size_t jj = i + ((int)rintf(p0) == x ? (size_t)0 : sx) + ((int)rintf(p1) == y ? (size_t)0 : sy) +
                          ((int)rintf(p2) == z ? (size_t)0 : (size_t)1);
        rgb = a.color_vol[jj * VS];
        rm = a.rem_vol[jj * VS];
      } else {
        const size_t i1 = i + (ax == 0 ? sx : (ax == 1 ? sy : (size_t)1));
        const int ce = ax == 0 ? x : (ax == 1 ? y : z);
        if (AOS) {
          const float4 q0 = reinterpret_cast<const float4*>(a.tsdf)[i], q1 = reinterpret_cast<const float4*>(a.tsdf)[i1];
          const float pe = mc_edge_coord(ce, q0.x, q1.x);
          if (ax == 0) p0 = pe; else if (ax == 1) p1 = pe; else p2 = pe;
          const bool far_end = (int)rintf(pe) != ce;
          rgb = far_end ? q1.z : q0.z;
          rm = far_end ? q1.w : q0.w;
        } else {
          const float pe = mc_edge_coord(ce, a.tsdf[i], a.tsdf[i1]);
          if (ax == 0) p0 = pe; else if (ax == 1) p1 = pe; else p2 = pe;
          const size_t jj = (int)rintf(pe) != ce ? i1 : i;
          rgb = a.color_vol[jj];
          rm = a.rem_vol[jj];
        }
      }
      const int vid = vbase0 + vb + j;
      if (vid < a.cap_v) {
        a.verts[3 * (size_t)vid] = p0 * a.voxel_size + a.ox;  // verts * voxel_size + vol_origin in float32 (:412)
        a.verts[3 * (size_t)vid + 1] = p1 * a.voxel_size + a.oy;
        a.verts[3 * (size_t)vid + 2] = p2 * a.voxel_size + a.oz;
        // colour unfolding (:419-423) in float32, .astype(np.uint8) = truncation to 8 bits
        const float cb = floorf(rgb / (float)(256 * 256));
        const float cg = floorf((rgb - cb * 256.0f * 256.0f) / 256.0f);
        const float cr = rgb - cb * 256.0f * 256.0f - cg * 256.0f;
        a.colors[3 * (size_t)vid] = (int)floorf(cr) & 255;
        a.colors[3 * (size_t)vid + 1] = (int)floorf(cg) & 255;
        a.colors[3 * (size_t)vid + 2] = (int)floorf(cb) & 255;
        a.rem[vid] = rm;
      }
    }
    LT_MC_WSYNC();
  }
}

// ---- triangles (cells exist where x + 1 < nx, y + 1 < ny, z + 1 < nz), a window of LT_MC_TCAP at a time: the cells listed
// by emit_cells put their triangles into the window's list, then a lane per triangle computes its three indices
__device__ __forceinline__ void emit_triangles(const mc_emit_args& a, mc_batch& s, int lane, const mc_extent& e) {
  const int ncell = e.ncell, tbase0 = e.tbase0, ntt = e.ntt;
  for (int tb = 0; tb < ntt; tb += LT_MC_TCAP) {
    for (int c = lane; c < ncell; c += 64) {  // a cell's (up to twelve) triangles into the window's list
      const int nt = (int)((s.cl[c] >> 10) & 15u);
      const int j0 = (int)s.ct[c] - tb;
      for (int t = 0; t < nt; ++t)
        if ((unsigned)(j0 + t) < LT_MC_TCAP) s.tl[j0 + t] = (unsigned short)((unsigned)c | ((unsigned)t << 10));
    }
    LT_MC_WSYNC();
    const int nwin = min(LT_MC_TCAP, ntt - tb);
    for (int j = lane; j < nwin; j += 64) {
      const unsigned tl = s.tl[j];
      const unsigned en = s.cl[tl & 1023u];
      const int k = en & 15, b = (en >> 4) & 63, t = (int)(tl >> 10);
      // the triangle's three codes in one 16-bit word (already in the reference's order: np.fliplr(faces)); three byte loads
      // with a branch on each were three dependent round trips per triangle window
      const unsigned codes = LT_LWF3[(en >> 15) / 3u + (unsigned)t];
      const int tid = tbase0 + tb + j;
      int id[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int code = (int)((codes >> (5 * q)) & 31u);
        if (code == 31) {  // the cell's centre vertex: behind the word's edge vertices, ranked among the word's centre cells
          const mc_rec& Rk = s.rec[k];
          id[q] = Rk.vbase + __popcll(Rk.ex) + __popcll(Rk.ey) + __popcll(Rk.ez) + __popcll(s.ccm[k] & ((1ull << b) - 1ull));
          continue;
        }
        const int c0 = code & 7, ax = code >> 3;
        int b2 = b + ((c0 >> 2) & 1), slot = c0 & 3;
        if (b2 == 64) { b2 = 0; slot |= 4; }
        const mc_nb nbe = s.nb[k][slot];
        const u64 l2 = (1ull << b2) - 1ull;
        int v = nbe.vbase + __popcll(nbe.ex & l2) + __popcll(nbe.ey & l2) + __popcll(nbe.ez & l2);
        if (ax > 0) v += (int)((nbe.ex >> b2) & 1ull);
        if (ax > 1) v += (int)((nbe.ey >> b2) & 1ull);
        id[q] = v;
      }
      if (tid < a.cap_f) {
        a.faces[3 * (size_t)tid] = id[0];
        a.faces[3 * (size_t)tid + 1] = id[1];
        a.faces[3 * (size_t)tid + 2] = id[2];
      }
    }
    LT_MC_WSYNC();
  }
}

// Batch order: active words are numbered x-major, so the batch list walks the volume plane by plane.  Workgroups are dealt
// to the eight XCDs round-robin (workgroup id % 8) and the L2s are private: with `xcd_map` XCD q takes the q-th EIGHTH of
// the batch list (its waves in turn within it), so that the columns (x + 1, y) / (x, y + 1) a batch samples are the OWN
// columns of batches the same L2 serves moments later -- instead of every plane's lines being pulled into all eight L2s.
// xcd_map = C > 0: the list is cut into CHUNKS of C batches (a few planes), chunk c belongs to XCD c % 8, and the waves of
// an XCD take the batches of its chunks in turn -- eight contiguous eighths (one per XCD) moved the fewest bytes but the
// XCDs finished at different times (a batch costs 1.5 - 42 us depending on where in the scene it lies).
// -> the batch of a wave's turn `it` (xcd_map: a turn of XCD xq's waves); -1: the list is exhausted.  With xcd_map the
// batch may lie behind the list's end -- the last round of eight chunks is partial: nothing to do in this turn
__device__ __forceinline__ int mc_batch_of(int it, int xcd_map, int xq, int n_batches) {
  if (!xcd_map) return it < n_batches ? it : -1;
  const int round = it / xcd_map;  // (of eight chunks)
  return round * 8 * xcd_map < n_batches ? (round * 8 + xq) * xcd_map + it % xcd_map : -1;
}

// the kernel: a wave takes batches until none is left (by default the grid has a wave per batch -- see the launch).
// (launch bounds: the five workgroups per CU that LDS admits -- five waves per SIMD -- are the register budget; left to
// itself the allocator took 102 registers with the working set in one struct, four waves, and 83 when told)
template <bool AOS>
__global__ __launch_bounds__(64 * LT_MC_EW, 5) void k_mc_emit_batch(const mc_emit_args a) {
  __shared__ mc_batch S[LT_MC_EW];
  __shared__ unsigned s_lwc[256];  // LT_LWC_FIXED, once per workgroup: a cell's tiling without a global round trip
  s_lwc[threadIdx.x & 255u] = LT_LWC_FIXED[threadIdx.x & 255u];
  __syncthreads();  // (the only workgroup barrier: before any wave's first batch)
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63u);
  mc_batch& s = S[wv];
  const int n_batches = (a.n_active + LT_MC_K - 1) / LT_MC_K;
  const int xcd_map = a.xcd_map;
  const int per_xcd = (int)(gridDim.x >> 3) * LT_MC_EW, xq = blockIdx.x & 7, xslot = (int)(blockIdx.x >> 3) * LT_MC_EW + wv;
  if (xcd_map && xslot >= per_xcd) return;  // (a grid that is not a multiple of eight: the tail waves have no share)
  for (int it = xcd_map ? xslot : (int)blockIdx.x * LT_MC_EW + wv;; it += xcd_map ? per_xcd : (int)gridDim.x * LT_MC_EW) {
    const int bi = mc_batch_of(it, xcd_map, xq, n_batches);
    if (bi < 0) break;
    if (bi >= n_batches) continue;
    mc_stamp st = LT_MC_SECTION_START(bi);
    const mc_extent e = emit_stage(a, s, lane, bi * LT_MC_K, st);
#if defined(LT_MC_STOP) && LT_MC_STOP == 1  // instruction-count experiment (tools/mc_sections.sh): staging only
    continue;
#endif
    emit_cells(a, s, s_lwc, lane, e.nw);
    LT_MC_SECTION(st, 5);  // cell masks, cell list, triangle offsets
#if defined(LT_MC_STOP) && LT_MC_STOP == 4  // ... + cell list and scan
    continue;
#endif
    emit_vertices<AOS>(a, s, lane, e, st);
    LT_MC_SECTION(st, 4);  // vertex pass (field samples, attributes, stores drained)
#if defined(LT_MC_STOP) && LT_MC_STOP == 3  // ... + vertex pass
    continue;
#endif
    emit_triangles(a, s, lane, e);
    LT_MC_SECTION(st, 6);  // triangle list + pass (stores drained)
    LT_MC_WSYNC();  // the batch's arrays are reused
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
extern "C" int lt_mesh_create(lt_mesh** out, int device) {
  if (!out) {
    lt_set_error("lt_mesh_create: NULL out pointer");
    return LT_ERR_INVALID_ARG;
  }
  *out = nullptr;
  if (device < 0) LT_HIP(hipGetDevice(&device));
  LT_HIP(hipSetDevice(device));
  lt_mesh* m = (lt_mesh*)calloc(1, sizeof(lt_mesh));
  if (!m) return LT_ERR_NO_MEMORY;
  m->device = device;
  if (hipHostMalloc((void**)&m->totals_host, 4 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    lt_set_error("lt_mesh_create: hipHostMalloc failed");
    free(m);
    return LT_ERR_NO_MEMORY;
  }
  for (int k = 0; k < 3; ++k) (void)hipEventCreate(&m->ev[k]);
  *out = m;
  return LT_OK;
}

extern "C" int lt_mesh_destroy(lt_mesh* m) {
  if (!m) return LT_OK;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  void* ps[] = {m->verts, m->faces, m->colors, m->rem, m->bits, m->cnt, m->cmap, m->blk, m->rec, m->wave_na, m->amb.queue, m->amb.table, m->amb.counter,
                m->verts2, m->colors2, m->rem2, m->rn_first, m->rn_newid, m->rn_bsum};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  if (m->totals_host) (void)hipHostFree(m->totals_host);
  for (int k = 0; k < 3; ++k)
    if (m->ev[k]) (void)hipEventDestroy(m->ev[k]);
  free(m);
  return LT_OK;
}

extern "C" int lt_mesh_get(lt_mesh* m, int* n_verts, int* n_faces, float** verts, int** faces, int** colors,
                           float** rem) {
  if (!m) {
    lt_set_error("lt_mesh_get: NULL mesh");
    return LT_ERR_INVALID_ARG;
  }
  if (n_verts) *n_verts = m->n_verts;
  if (n_faces) *n_faces = m->n_faces;
  if (verts) *verts = m->verts;
  if (faces) *faces = m->faces;
  if (colors) *colors = m->colors;
  if (rem) *rem = m->rem;
  return LT_OK;
}

// one array of the mesh with the headroom rule (lt_devmem.h; the device has finished with the old one before it goes)
template <class T>
static int mc_reserve(T** p, size_t* cap, size_t need) {
  return lt_dev_grow("lt_marching_cubes_dev", lt_wait_device(), p, cap, need, lt_headroom(need));
}

static mc_emit_args mc_emit_args_of(const float* tsdf, const float* color_vol, const float* rem_vol, const u64* bits,
                                    const mc_dims& D, const lt_mesh* m, int n_active, float voxel_size, const float* origin,
                                    int xcd_map) {
  return {tsdf, color_vol, rem_vol, bits, D, m->cmap, m->rec, n_active, voxel_size, origin[0], origin[1], origin[2],
          m->verts, m->faces, m->colors, m->rem, m->cap_v, m->cap_f, m->amb, xcd_map};  // (in mc_emit_args' order)
}

// ---- mc_extract: one extraction, step by step --------------------------------------------------------------------------
// what the steps share
struct mc_job {
  const float* tsdf; const float* color_vol; const float* rem_vol;
  float voxel_size; const float* origin;
  lt_mesh* m; hipStream_t stream; bool timed;
  // the volume's own stamps and sign bits (lt_tsdf_extract_mesh_dev), or NULL
  const unsigned* col_epoch; unsigned epoch; const u64* ext_bits; const unsigned* chunk_epoch;
  mc_dims D;
  int n_blocks;   // one block of the scan per wave of 64 rows
  int n_seg;      // segments of 256 blocks (k_mc_scan1 / 2)
  int sweep_wgs;  // workgroups of k_mc_words and k_mc_compact (a wave takes LT_MC_BLOCKS_PER_WAVE blocks, see k_mc_words)
};
// sign bits: the volume's own (kept current by integrate / reset, lt_tsdf.hip) or one pass over the float field
static const u64* mc_bits_of(const mc_job& J) { return J.ext_bits ? J.ext_bits : J.m->bits; }
static int* mc_seg_of(const mc_job& J) { return J.m->blk + 3 * (size_t)J.n_blocks; }  // (lt_mesh::blk)

// the volume's sizes checked, mc_dims and the sizes of the launches; *empty: no cell, nothing to extract
static int mc_dims_of(int vs, int nx, int ny, int nz, mc_job* J, bool* empty) {
  if ((double)nx * ny * nz >= 2147483647.0) {
    lt_set_error("lt_marching_cubes_dev: more than 2^31 - 1 voxels");
    return LT_ERR_TOO_LARGE;
  }
  LT_HIP(hipSetDevice(J->m->device));
  *empty = nx < 2 || ny < 2 || nz < 2;  // no cell (scikit-image: "Input array must be at least 2x2x2"): the empty mesh
  if (*empty) return LT_OK;
  mc_dims& D = J->D;
  D.nx = nx; D.ny = ny; D.nz = nz; D.vs = vs;
  D.wz = (nz + 63) / 64;
  mc_magic((unsigned)D.wz, &D.wz_m, &D.wz_s);
  mc_magic((unsigned)D.ny, &D.ny_m, &D.ny_s);
  const size_t n_words = (size_t)nx * ny * D.wz;
  if (n_words >= 2147483647ull) {
    lt_set_error("lt_marching_cubes_dev: volume too large");
    return LT_ERR_TOO_LARGE;
  }
  D.n_words = (int)n_words;
  if (D.wz > 21) {  // (the packed per-block totals hold 20 bits a field, see pack3)
    lt_set_error("lt_marching_cubes_dev: nz = %d exceeds 1344", nz);
    return LT_ERR_TOO_LARGE;
  }
  J->n_blocks = ((nx * ny + 255) / 256) * 4;
  J->n_seg = (J->n_blocks + 255) / 256;
  J->sweep_wgs = lt_deal_count(J->n_blocks, LT_MC_BLOCKS_PER_WAVE, ny, 4) / 4;
  return LT_OK;
}

static int mc_reserve_words(const mc_job& J) {  // bits / cnt / cmap
  lt_mesh* m = J.m;
  const size_t n_words = (size_t)J.D.n_words;
  if (n_words > m->cap_words || !m->bits) {
    const lt_dev_array words[] = {{(void**)&m->bits, (n_words + 1) * sizeof(u64)}, {(void**)&m->cnt, n_words * sizeof(unsigned)},
                                  {(void**)&m->cmap, n_words * sizeof(int)}};
    LT_CHECK(lt_dev_replace("lt_marching_cubes_dev", lt_wait_device(), &m->cap_words, n_words, words));
    m->state_dirty = 1;  // (fresh buffers: swept by mc_restore_state)
  }
  return LT_OK;
}

// the ambiguous cells' queue and tiling table: m->amb_cap cells per shard, the counters allocated once
static int mc_reserve_amb(const mc_job& J) {
  lt_mesh* m = J.m;
  hipStream_t stream = J.stream;
  if (m->amb.queue && m->amb.counter && m->amb.cap == m->amb_cap) return LT_OK;
  const size_t cap = m->amb_cap ? m->amb_cap : (size_t)1 << 10;   // per shard
  size_t tcap = 1;
  while (tcap < 4 * LT_MC_SHARDS * cap) tcap <<= 1;
  const size_t n_ctr = LT_MC_SHARDS * LT_MC_CTR_STRIDE + LT_MC_SHARDS;
  const lt_dev_array amb[] = {{(void**)&m->amb.queue, LT_MC_SHARDS * cap * sizeof(uint2)}, {(void**)&m->amb.table, tcap * sizeof(uint2)}};
  LT_CHECK(lt_dev_replace("lt_marching_cubes_dev (ambiguous cells)", lt_wait_device(), &m->amb.cap, (unsigned)cap, amb));
  if (!m->amb.counter) {  // once
    const lt_dev_array counter[] = {{(void**)&m->amb.counter, n_ctr * sizeof(int)}};
    LT_CHECK(lt_dev_replace("lt_marching_cubes_dev (ambiguous cells)", lt_wait_none(), counter));
  }
  m->amb_cap = cap;
  m->amb.tmask = (unsigned)(tcap - 1);
  LT_HIP(hipMemsetAsync(m->amb.counter, 0, n_ctr * sizeof(int), stream));
  LT_HIP(hipMemsetAsync(m->amb.table, 0, tcap * sizeof(uint2), stream));
  m->n_amb_prev = 0;
  return LT_OK;
}

// cnt = 0, cmap = -1, the tiling table empty: by undoing the last extraction's entries (k_mc_clear) or, with new buffers or
// after an extraction that did not finish, by sweeping everything once.  state_dirty stays set until mc_finish.
static int mc_restore_state(const mc_job& J) {
  lt_mesh* m = J.m;
  hipStream_t stream = J.stream;
  if (m->state_dirty) {
    LT_HIP(hipMemsetAsync(m->cnt, 0, m->cap_words * sizeof(unsigned), stream));
    LT_HIP(hipMemsetAsync(m->cmap, 0xFF, m->cap_words * sizeof(int), stream));
    LT_HIP(hipMemsetAsync(m->amb.counter, 0, (LT_MC_SHARDS * LT_MC_CTR_STRIDE + LT_MC_SHARDS) * sizeof(int), stream));
    LT_HIP(hipMemsetAsync(m->amb.table, 0, ((size_t)m->amb.tmask + 1) * sizeof(uint2), stream));
  } else if (m->n_prev > 0) {
    hipLaunchKernelGGL(k_mc_clear, dim3((max(m->n_prev, LT_MC_SHARDS * m->n_amb_prev) + 255) / 256), dim3(256), 0, stream, m->rec,
                       m->n_prev, m->cnt, m->cmap, m->amb, m->n_amb_prev);
  }
  m->state_dirty = 1;  // until this extraction has finished
  m->n_prev = 0;
  m->n_amb_prev = 0;
  return LT_OK;
}

static int mc_reserve_blocks(const mc_job& J) {  // wave_na and blk (the blocks' triples, the segment sums, four totals)
  lt_mesh* m = J.m;
  LT_CHECK(mc_reserve(&m->wave_na, &m->cap_wave_na, (size_t)J.n_blocks));
  if (J.n_seg > 1024) {
    lt_set_error("lt_marching_cubes_dev: volume too large (%d words)", J.D.n_words);
    return LT_ERR_TOO_LARGE;
  }
  return mc_reserve(&m->blk, &m->cap_blocks, (size_t)3 * J.n_blocks + 3 * (size_t)J.n_seg + 4);
}

// The counting part, up to the one synchronisation: m->totals_host holds {active words, vertices, triangles, the fullest
// shard's ambiguous cells}.  mc_extract runs it a second time when it queued more ambiguous cells than the side buffers held.
static int mc_count(const mc_job& J) {
  lt_mesh* m = J.m;
  hipStream_t stream = J.stream;
  const mc_dims& D = J.D;
  int* seg_dev = mc_seg_of(J);
  int* totals_dev = seg_dev + 3 * (size_t)J.n_seg;
  if (J.timed) LT_HIP(hipEventRecord(m->ev[0], stream));
  if (!J.ext_bits)
    hipLaunchKernelGGL(k_mc_signs, dim3((unsigned)min((size_t)16384, ((size_t)D.nx * D.ny + 255) / 256)), dim3(256), 0, stream,
                       J.tsdf, D, m->bits, J.col_epoch, J.epoch);
  if (J.timed) LT_HIP(hipEventRecord(m->ev[1], stream));
  hipLaunchKernelGGL(k_mc_words, dim3(J.sweep_wgs), dim3(256), 0, stream, m->amb, mc_bits_of(J), D, m->cnt, m->blk,
                     J.ext_bits ? J.col_epoch : nullptr, J.epoch, J.ext_bits ? J.chunk_epoch : nullptr, m->wave_na, J.n_blocks);
  // Lewiner's ambiguous cells (1-2 % of a street scene's): tests on their eight values, counts added, tilings filed
  hipLaunchKernelGGL(k_mc_amb, dim3(2 * LT_MC_SHARDS), dim3(256), 0, stream, J.tsdf, D, m->amb, m->cnt, m->blk, m->wave_na);
  hipLaunchKernelGGL(k_mc_scan1, dim3(J.n_seg), dim3(256), 0, stream, m->blk, J.n_blocks, seg_dev);
  hipLaunchKernelGGL(k_mc_scan2, dim3(1), dim3(1024), 0, stream, seg_dev, J.n_seg, totals_dev, m->amb.counter, (int)m->amb.cap);
  LT_HIP(hipMemcpyAsync(m->totals_host, totals_dev, 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
  LT_HIP(hipStreamSynchronize(stream));  // the one synchronisation: the sizes of the mesh
  return LT_OK;
}

// the sizes of the mesh checked, its arrays and the records of the active words reserved
static int mc_reserve_mesh(const mc_job& J) {
  lt_mesh* m = J.m;
  const int n_active = m->totals_host[0], nv = m->totals_host[1], nf = m->totals_host[2];
  static const bool dbg_mc = getenv("LIDARHIP_DEBUG_MC") != nullptr;
  // (tests/test_mc_gpu.py reads this line: keep its wording)
  if (dbg_mc) fprintf(stderr, "marching cubes: %d active words, %d vertices, %d triangles\n", n_active, nv, nf);
  if (nv == 2147483647 || nf == 2147483647) {
    lt_set_error("lt_marching_cubes_dev: mesh exceeds 2^31 - 1 vertices / faces");
    return LT_ERR_TOO_LARGE;
  }
  if (nf >= LT_MAX_FACES) {
    lt_set_error("lt_marching_cubes_dev: %d faces exceed LT_MAX_FACES", nf);
    return LT_ERR_TOO_LARGE;
  }
  LT_CHECK(mc_reserve(&m->rec, &m->cap_rec, (size_t)n_active));
  if (nv > m->cap_v || !m->verts) {
    const size_t cap = lt_headroom((size_t)nv);
    const lt_dev_array vertex[] = {{(void**)&m->verts, cap * 12}, {(void**)&m->colors, cap * 12}, {(void**)&m->rem, cap * 4}};
    LT_CHECK(lt_dev_replace("lt_marching_cubes_dev (vertices)", lt_wait_device(), &m->cap_v, (int)min(cap, (size_t)2147483647), vertex));
  }
  if (nf > m->cap_f || !m->faces) {
    const size_t cap = lt_headroom((size_t)nf);
    const lt_dev_array face[] = {{(void**)&m->faces, cap * 12}};
    LT_CHECK(lt_dev_replace("lt_marching_cubes_dev (faces)", lt_wait_device(), &m->cap_f, (int)min(cap, (size_t)2147483647), face));
  }
  return LT_OK;
}

// k_mc_compact and the emission
static int mc_emit(const mc_job& J) {
  lt_mesh* m = J.m;
  hipStream_t stream = J.stream;
  const int n_active = m->totals_host[0];
  hipLaunchKernelGGL(k_mc_compact, dim3(J.sweep_wgs), dim3(256), 0, stream, mc_bits_of(J), J.D, m->cnt, m->blk, mc_seg_of(J), m->cmap, m->rec,
                     (int)min(m->cap_rec, (size_t)2147483647), m->wave_na, J.n_blocks);
  if (n_active > 0) {
    // The grid: persistent waves taking batches in turn (bi += gridDim), 36 per CU -- 1.8 x the resident capacity (20 waves
    // per CU, see LT_MC_VCAP; swept again with four-wave workgroups on the six-workgroup variant: 24 / 36 / 48 / 72 / 96 per
    // CU = 118 / 90 / 100 / 92 / 102 us).  On the default volume's street scene (31 500 batches; a batch lives 8.3 us on
    // average and up to 42, tools/mc_wave_times.py): a wave per batch 96 us -- a wave's start and drain 31 500 times --,
    // 4 608 / 9 216 / 18 432 persistent waves 107 / 87 / 86 us (static dealing is at the mercy of the heavy batches: with
    // one round of waves the slowest wave is the kernel), and persistent waves DRAWING their batches from eight counters
    // (returning atomics, the draw for the next batch issued under the current one) 117-128 us: a returning atomic is a
    // memory-side round trip that the batch's first barrier waits for.  LIDARHIP_MC_EMIT_WAVES=n: n waves; =0: a wave per batch.
    static const int env_waves = []() { const char* e = getenv("LIDARHIP_MC_EMIT_WAVES"); return e ? atoi(e) : -1; }();
    const int dflt_waves = lt_cu_count(m->device) * 36;
    const int max_waves = env_waves > 0 ? env_waves : (env_waves == 0 ? (1 << 24) : dflt_waves);
    // LIDARHIP_MC_EMIT_XCD=0: batches dealt to the waves round-robin over the whole list (rounds 3-4)
    static const int env_xcd = []() { const char* e = getenv("LIDARHIP_MC_EMIT_XCD"); return e ? atoi(e) : 64; }();
    const int n_batches = (n_active + LT_MC_K - 1) / LT_MC_K;
    const int n_wgs = (min(n_batches, max_waves) + LT_MC_EW - 1) / LT_MC_EW;
    const int xcd_map = (env_xcd > 0 && n_wgs * LT_MC_EW >= 64) ? env_xcd : 0;
    const mc_emit_args args = mc_emit_args_of(J.tsdf, J.color_vol, J.rem_vol, mc_bits_of(J), J.D, m, n_active, J.voxel_size, J.origin,
                                              xcd_map);
    hipLaunchKernelGGL(J.D.vs == 4 ? k_mc_emit_batch<true> : k_mc_emit_batch<false>, dim3((unsigned)n_wgs), dim3(64 * LT_MC_EW), 0,
                       stream, args);
  }
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// the extraction has finished: what the next one's mc_restore_state undoes, and the times when asked for
static int mc_finish(const mc_job& J, float* ms) {
  lt_mesh* m = J.m;
  hipStream_t stream = J.stream;
  m->n_verts = m->totals_host[1];
  m->n_faces = m->totals_host[2];
  m->n_prev = m->totals_host[0];  // (the records k_mc_clear will undo before the next extraction)
  m->n_amb_prev = m->totals_host[3];  // (the fullest shard's count: k_mc_clear's extent per shard)
  m->state_dirty = 0;
  if (ms) {
    LT_HIP(hipEventRecord(m->ev[2], stream));
    LT_HIP(hipStreamSynchronize(stream));
    LT_HIP(hipEventElapsedTime(&m->ms_signs, m->ev[0], m->ev[1]));
    LT_HIP(hipEventElapsedTime(&m->ms_rest, m->ev[1], m->ev[2]));
    ms[0] = m->ms_signs;
    ms[1] = m->ms_rest;
  }
  return LT_OK;
}

static int mc_extract(const float* tsdf, const float* color_vol, const float* rem_vol, int vs, int nx, int ny, int nz,
                      float voxel_size, const float* origin, lt_mesh* m, void* stream_, float* ms,
                      const unsigned* col_epoch, unsigned epoch, const u64* ext_bits, const unsigned* chunk_epoch) {
  if (!tsdf || !color_vol || !rem_vol || !origin || !m || nx <= 0 || ny <= 0 || nz <= 0) {
    lt_set_error("lt_marching_cubes_dev: invalid argument");
    return LT_ERR_INVALID_ARG;
  }
  mc_job J = {tsdf, color_vol, rem_vol, voxel_size, origin, m, (hipStream_t)stream_, ms != nullptr,
              col_epoch, epoch, ext_bits, chunk_epoch};  // (D and the sizes: mc_dims_of)
  bool empty = false;
  LT_CHECK(mc_dims_of(vs, nx, ny, nz, &J, &empty));
  if (empty) {
    m->n_verts = 0;
    m->n_faces = 0;
    if (ms) ms[0] = ms[1] = 0.f;
    return LT_OK;
  }
  LT_CHECK(mc_reserve_words(J));
  for (;;) {
    LT_CHECK(mc_reserve_amb(J));
    LT_CHECK(mc_restore_state(J));
    LT_CHECK(mc_reserve_blocks(J));
    LT_CHECK(mc_count(J));
    const size_t need = (size_t)(unsigned)m->totals_host[3];
    if (need <= m->amb_cap) break;
    // more ambiguous cells in a shard than its segment holds (white noise: a third of all cells): the counts above are incomplete --
    // larger buffers, and the counting once more from the start (cnt / cmap are swept: state_dirty is still set)
    m->amb_cap = need + need / 4 + 1024;
  }
  LT_CHECK(mc_reserve_mesh(J));
  LT_CHECK(mc_emit(J));
  return mc_finish(J, ms);
}

// ---- lt_mesh_renumber_dev: the vertices numbered as scikit-image numbers them ----------------------------------------
// The extraction above emits scikit-image's FACE STREAM with its own vertex numbers (by word / owner voxel / edge axis).
// scikit-image creates a vertex when a face first references it, so its number is the rank of its first use in ITS face
// stream -- which lists a face's corners in the tiling's order; the reversal (np.fliplr, gradient_direction="descent")
// happens afterwards, so position q = 3 face + k of that stream is corner 2 - k of the face array here (rn_at).
// first[v] = min q (atomicMin), flag(q) = "q is a first use", new number = exclusive prefix sum of the flags at first[v]
// (two-level scan, 1024 positions per block), vertex arrays permuted, faces rewritten.
// For the host-facing get_mesh (the arrays then EQUAL the reference's, golden F10); the in-HBM chain has no use for it.
__device__ __forceinline__ int rn_at(int q) { return q + 2 - 2 * (q % 3); }  // index in the face array of stream position q
__global__ __launch_bounds__(256) void k_rn_first(const int* __restrict__ faces, int n3, int* __restrict__ first) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < n3) atomicMin(&first[faces[rn_at(q)]], q);
}
__device__ __forceinline__ int rn_block_excl_scan(int v, int* total) {  // 256 threads; returns the exclusive prefix of v
  __shared__ int ws[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int q = __shfl_up(inc, o, 64);
    if (lane >= o) inc += q;
  }
  __syncthreads();  // (ws may still be read by a previous call)
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wv; ++w) off += ws[w];
  *total = ws[0] + ws[1] + ws[2] + ws[3];
  return off + inc - v;
}
// stream positions [1024 b, 1024 b + 1024): thread t holds the four consecutive positions 1024 b + 4 t ..
template <bool WRITE>
__global__ __launch_bounds__(256) void k_rn_rank(const int* __restrict__ faces, int n3, const int* __restrict__ first,
                                                 int* __restrict__ bsum, int* __restrict__ newid) {
  const int p0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int v[4], f[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = p0 + j < n3 ? faces[rn_at(p0 + j)] : -1;
    f[j] = (v[j] >= 0 && first[v[j]] == p0 + j) ? 1 : 0;
    s += f[j];
  }
  int total;
  int ex = rn_block_excl_scan(s, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    return;
  }
  ex += bsum[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (f[j]) newid[v[j]] = ex;
    ex += f[j];
  }
}
__global__ __launch_bounds__(1024) void k_rn_scan_blocks(int* __restrict__ bsum, int nb) {  // exclusive, in place; total -> bsum[nb]
  __shared__ int carry, ws[16];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int q = __shfl_up(inc, o, 64);
      if (lane >= o) inc += q;
    }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wv; ++w) off += ws[w];
    if (i < nb) bsum[i] = off + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = off + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}
__global__ __launch_bounds__(256) void k_rn_move(const int* __restrict__ newid, int nv, const float* __restrict__ verts,
                                                 const int* __restrict__ colors, const float* __restrict__ rem,
                                                 float* __restrict__ verts2, int* __restrict__ colors2, float* __restrict__ rem2) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int j = newid[v];
  if (j < 0) return;  // (an unreferenced vertex: reported by the host)
#pragma unroll
  for (int k = 0; k < 3; ++k) { verts2[3 * (size_t)j + k] = verts[3 * (size_t)v + k]; colors2[3 * (size_t)j + k] = colors[3 * (size_t)v + k]; }
  rem2[j] = rem[v];
}
__global__ __launch_bounds__(256) void k_rn_faces(int* __restrict__ faces, int n3, const int* __restrict__ newid) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n3) faces[p] = newid[faces[p]];
}

// see include/lidarhip.h
extern "C" int lt_mesh_renumber_dev(lt_mesh* m, void* stream_) {
  if (!m) {
    lt_set_error("lt_mesh_renumber_dev: NULL mesh");
    return LT_ERR_INVALID_ARG;
  }
  const int nv = m->n_verts, n3 = 3 * m->n_faces;
  if (nv == 0 || n3 == 0) return LT_OK;
  if ((long long)m->n_faces * 3 > 2147483647ll) {
    lt_set_error("lt_mesh_renumber_dev: more than 2^31 face corners");
    return LT_ERR_TOO_LARGE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  LT_HIP(hipSetDevice(m->device));
  const int nb = (n3 + 1023) / 1024;
  const char* who = "lt_mesh_renumber_dev";  // (no wait of its own: hipFree waits for the device)
  if ((size_t)nv > m->cap_rn || !m->rn_first) {
    const size_t cap = lt_headroom((size_t)nv);
    const lt_dev_array per_vertex[] = {{(void**)&m->rn_first, cap * sizeof(int)}, {(void**)&m->rn_newid, cap * sizeof(int)}};
    LT_CHECK(lt_dev_replace(who, lt_wait_none(), &m->cap_rn, cap, per_vertex));
  }
  LT_CHECK(lt_dev_grow(who, lt_wait_none(), &m->rn_bsum, &m->cap_bsum, (size_t)nb + 1, (size_t)nb + nb / 4 + 1024));
  if (m->cap_v2 < m->cap_v || !m->verts2) {
    const size_t cap = (size_t)m->cap_v;
    const lt_dev_array second[] = {{(void**)&m->verts2, cap * 12}, {(void**)&m->colors2, cap * 12}, {(void**)&m->rem2, cap * 4}};
    LT_CHECK(lt_dev_replace(who, lt_wait_none(), &m->cap_v2, m->cap_v, second));
  }
  LT_HIP(hipMemsetAsync(m->rn_first, 0x7F, (size_t)nv * sizeof(int), stream));   // 0x7F7F7F7F: beyond any position
  LT_HIP(hipMemsetAsync(m->rn_newid, 0xFF, (size_t)nv * sizeof(int), stream));   // -1
  hipLaunchKernelGGL(k_rn_first, dim3((n3 + 255) / 256), dim3(256), 0, stream, m->faces, n3, m->rn_first);
  hipLaunchKernelGGL(k_rn_rank<false>, dim3(nb), dim3(256), 0, stream, m->faces, n3, m->rn_first, m->rn_bsum, m->rn_newid);
  hipLaunchKernelGGL(k_rn_scan_blocks, dim3(1), dim3(1024), 0, stream, m->rn_bsum, nb);
  hipLaunchKernelGGL(k_rn_rank<true>, dim3(nb), dim3(256), 0, stream, m->faces, n3, m->rn_first, m->rn_bsum, m->rn_newid);
  hipLaunchKernelGGL(k_rn_move, dim3((nv + 255) / 256), dim3(256), 0, stream, m->rn_newid, nv, m->verts, m->colors, m->rem,
                     m->verts2, m->colors2, m->rem2);
  int referenced = 0;
  LT_HIP(hipMemcpyAsync(&referenced, m->rn_bsum + nb, sizeof(int), hipMemcpyDeviceToHost, stream));
  LT_HIP(hipStreamSynchronize(stream));
  LT_HIP(hipGetLastError());
  if (referenced != nv) {  // (cannot happen for a mesh of lt_marching_cubes_dev: every vertex lies on an edge some tiling uses)
    // nothing of the mesh has been touched yet: the faces are rewritten only once the new numbering is known to be complete
    lt_set_error("lt_mesh_renumber_dev: %d of %d vertices are referenced by no face", nv - referenced, nv);
    return LT_ERR_BAD_INDEX;
  }
  hipLaunchKernelGGL(k_rn_faces, dim3((n3 + 255) / 256), dim3(256), 0, stream, m->faces, n3, m->rn_newid);
  LT_HIP(hipGetLastError());
  float* tv = m->verts; m->verts = m->verts2; m->verts2 = tv;
  int* tc = m->colors; m->colors = m->colors2; m->colors2 = tc;
  float* tr = m->rem; m->rem = m->rem2; m->rem2 = tr;
  const int tcap = m->cap_v; m->cap_v = m->cap_v2; m->cap_v2 = tcap;
  return LT_OK;
}

// Marching cubes over a TSDF volume's current state (level 0): replaces TSDFVolume.get_mesh (fusion_lidar.py:403-424).
extern "C" int lt_tsdf_extract_mesh_dev(lt_tsdf* t, lt_mesh* m, void* stream, float* ms) {
  if (!t || !m) {
    lt_set_error("lt_tsdf_extract_mesh_dev: NULL volume / mesh");
    return LT_ERR_INVALID_ARG;
  }
  if (t->device != m->device) {
    lt_set_error("lt_tsdf_extract_mesh_dev: volume on device %d, mesh on device %d", t->device, m->device);
    return LT_ERR_INVALID_ARG;
  }
  // the volume knows which columns were written since its last reset: the others are not read
  return mc_extract(t->tsdf, t->color, t->rem, 4 /* LT_VOX records */, t->dim[0], t->dim[1], t->dim[2], t->voxel_size, t->origin, m, stream, ms,
                    t->all_dirty ? nullptr : t->col_epoch, t->epoch, t->all_dirty ? nullptr : t->bits,
                    t->all_dirty ? nullptr : t->chunk_epoch);
}

extern "C" int lt_marching_cubes_dev(const float* tsdf, const float* color_vol, const float* rem_vol, int nx, int ny,
                                     int nz, float voxel_size, const float* origin, lt_mesh* m, void* stream_,
                                     float* ms) {
  return mc_extract(tsdf, color_vol, rem_vol, 1, nx, ny, nz, voxel_size, origin, m, stream_, ms, nullptr, 0u, nullptr, nullptr);
}

extern "C" int lt_scene_set_mesh(lt_scene* s, lt_mesh* m) {
  if (!s || !m) {
    lt_set_error("lt_scene_set_mesh: NULL scene / mesh");
    return LT_ERR_INVALID_ARG;
  }
  if (s->device != m->device) {
    lt_set_error("lt_scene_set_mesh: scene on device %d, mesh on device %d", s->device, m->device);
    return LT_ERR_INVALID_ARG;
  }
  return lt_scene_set_mesh_dev(s, m->verts, m->faces, m->colors, m->rem, m->n_verts, m->n_faces);
}

// One output scan of the `mesh` adaption (laserscan.py:874-914) in one call: see include/lidarhip.h.
extern "C" int lt_fusion_scan_dev(lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene, lt_rayset* rayset, int n_obs,
                                  const float* const* color_ims, const float* const* depth_ims,
                                  const float* const* rem_ims, int im_h, int im_w, float obs_weight, unsigned tsdf_flags,
                                  const float* origin, float* endpoints, int* endcolors, float* range, float* endrem,
                                  int* tri, unsigned trace_flags, void* stream, int sync) {
  if (!vol || !mesh || !scene || !rayset || !origin || n_obs < 0 || (n_obs > 0 && (!color_ims || !depth_ims || !rem_ims))) {
    lt_set_error("lt_fusion_scan_dev: invalid argument");
    return LT_ERR_INVALID_ARG;
  }
  LT_CHECK(lt_tsdf_reset(vol, stream));
  // (all observations of the fresh volume in one pass where the class-aware update allows it: lt_tsdf.hip)
  LT_CHECK(lt_tsdf_integrate_multi_dev(vol, n_obs, color_ims, depth_ims, rem_ims, im_h, im_w, obs_weight, tsdf_flags, stream));
  LT_CHECK(lt_tsdf_extract_mesh_dev(vol, mesh, stream, nullptr));
  LT_CHECK(lt_scene_set_mesh(scene, mesh));
  LT_CHECK(lt_scene_render_dev(scene, rayset, origin, endpoints, endcolors, range, endrem, tri, trace_flags, stream, nullptr));
  if (sync) LT_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LT_OK;
}
