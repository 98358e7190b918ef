// The carved buffers of lidar_transfer_amd/csrc/lt_layouts.h held against the offset arithmetic they replaced, which is
// restated here as it stood at each site (al = the former align256; b3, b1, bv, ... the sites' own names).  Plain C++, no
// HIP header: compiled and run by tests/test_devmem_layout_cpu.py.  Prints one line per failure; exit status 1 if any.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "lt_layouts.h"

static int g_bad = 0;
static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct region { size_t at, bytes; };

// offsets as expected; every one a multiple of 256; the regions disjoint, in order and inside `total`
static void check(const char* what, size_t n, const std::vector<region>& got, const std::vector<size_t>& want_at, size_t total,
                  size_t want_total) {
  if (total != want_total) { printf("%s n=%zu: total %zu, expected %zu\n", what, n, total, want_total); ++g_bad; }
  for (size_t k = 0; k < got.size(); ++k) {
    if (got[k].at != want_at[k]) { printf("%s n=%zu: array %zu at %zu, expected %zu\n", what, n, k, got[k].at, want_at[k]); ++g_bad; }
    if (got[k].at % 256) { printf("%s n=%zu: array %zu at %zu is not 256-byte aligned\n", what, n, k, got[k].at); ++g_bad; }
    const size_t end = got[k].at + got[k].bytes;
    const size_t next = k + 1 < got.size() ? got[k + 1].at : total;
    if (end < got[k].at || end > next) { printf("%s n=%zu: array %zu [%zu, %zu) runs into %zu\n", what, n, k, got[k].at, end, next); ++g_bad; }
  }
}

int main() {
  static_assert(sizeof(size_t) == 8, "the layouts are size_t arithmetic on a 64-bit host");
  const size_t big = ((size_t)1 << 32) / 12 + 1;  // 12 * big > 2^32: 32-bit arithmetic would wrap
  const size_t sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, big};
  for (size_t n : sizes) {
    for (size_t nf : {n, (size_t)2 * n + 1}) {  // vertices and faces differ
      const size_t nv = n;
      {  // host-pipe mesh (hp_upload / hp_launch)
        const size_t bv = al(nv * 12), bf = al(nf * 12), br = al(nv * 4), b8 = al(nv * 3);
        const lt_hp_mesh_layout L = lt_hp_mesh_layout_of(nv, nf);
        check("hostpipe mesh", n, {{L.verts, nv * 12}, {L.faces, nf * 12}, {L.colors, nv * 12}, {L.rem, nv * 4}, {L.colors_u8, nv * 3}},
              {0, bv, bv + bf, 2 * bv + bf, 2 * bv + bf + br}, L.total, 2 * bv + bf + br + b8 + 256);
      }
      {  // owned mesh (lt_scene_set_mesh_host)
        const size_t bv = al(nv * 12), bf = al(nf * 12), bc = bv, br = al(nv * 4);
        const lt_owned_mesh_layout L = lt_owned_mesh_layout_of(nv, nf);
        check("owned mesh", n, {{L.verts, nv * 12}, {L.faces, nf * 12}, {L.colors, nv * 12}, {L.rem, nv * 4}},
              {0, bv, bv + bf, bv + bf + bc}, L.total, bv + bf + bc + br + 256);
      }
    }
    const size_t R = n;
    for (int label = 0; label < 2; ++label) {  // host-pipe output (lt_hostpipe_create, hp_launch, hp_collect)
      const size_t b3 = al(R * 12), b1 = al(R * 4), bc = label ? b1 : b3;
      const lt_hp_out_layout L = lt_hp_out_layout_of(R, label != 0);
      check(label ? "hostpipe output (label image)" : "hostpipe output", n,
            {{L.endpoints, R * 12}, {L.endcolors, R * (label ? 4 : 12)}, {L.range, R * 4}, {L.endrem, R * 4}, {L.tri, R * 4}},
            {0, b3, b3 + bc, b3 + bc + b1, b3 + bc + 2 * b1}, L.total, b3 + bc + 3 * b1 + 256);
      if (L.images != b3 + bc + 3 * b1) { printf("hostpipe output n=%zu: one transfer of %zu bytes, expected %zu\n", n, L.images, b3 + bc + 3 * b1); ++g_bad; }
    }
    {  // ctrace io (ctrace_thread)
      const size_t b3 = al(R * 12), b1 = al(R * 4);
      const lt_ctrace_io_layout L = lt_ctrace_io_layout_of(R);
      check("ctrace io", n, {{L.rays, R * 12}, {L.endpoints, R * 12}, {L.endcolors, R * 12}, {L.range, R * 4}, {L.endrem, R * 4}, {L.tri, R * 4}},
            {0, b3, 2 * b3, 3 * b3, 3 * b3 + b1, 3 * b3 + 2 * b1}, L.total, 3 * b3 + 3 * b1 + 256);
    }
    for (size_t es : {(size_t)4, (size_t)8}) {  // the 19 staging arrays of lt_range_projection: N points, `cells`, a colour table
      const size_t N = n, cells = 2 * n + 3, lut = n % 7;
      const size_t bytes[19] = {N * 3 * es, N * 4, N * 4, lut * 12, N * 3 * es, N * 4, N * 4, N * es, N * 4, N * 4, N * es, N * es,
                                cells * 4, cells * 4, cells * 12, cells * 4, cells * 4, cells * 12, cells * 4};
      const lt_rp_layout L = lt_rp_layout_of(N, es, lut, cells);
      std::vector<region> got;
      std::vector<size_t> want;
      size_t off = 0, total = 256;
      for (int k = 0; k < 19; ++k) {
        got.push_back({L.at[k], bytes[k]});
        want.push_back(off);
        off += al(bytes[k]);
        total += al(bytes[k]);
      }
      check(es == 4 ? "range projection staging (f32)" : "range projection staging (f64)", n, got, want, L.total, total);
    }
  }
  static_assert(LT_RP_ARRAYS == 19, "lt_range_projection stages 19 arrays");
  if (g_bad) return 1;
  printf("layouts ok\n");
  return 0;
}
