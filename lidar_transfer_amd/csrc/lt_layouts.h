// lt_layouts.h -- the carved device buffers of the library, one function each: whoever fills or reads such a buffer asks
// its function for the offsets, nobody repeats the sums.  size_t arithmetic on lt_carve only (no HIP types): it is compiled
// and checked on the CPU (tests/test_devmem_layout_cpu.py).  `total` includes the trailing 256-byte pad of each buffer.
#pragma once
#include "lt_devmem.h"

// the host pipe's mesh block of a slot (lt_host.hip): verts | faces | colors i32 | rem | colors u8
struct lt_hp_mesh_layout { size_t verts, faces, colors, rem, colors_u8, total; };
static inline lt_hp_mesh_layout lt_hp_mesh_layout_of(size_t n_verts, size_t n_faces) {
  lt_carve c;
  lt_hp_mesh_layout L;
  L.verts = c.take(n_verts * 12);
  L.faces = c.take(n_faces * 12);
  L.colors = c.take(n_verts * 12);
  L.rem = c.take(n_verts * 4);
  L.colors_u8 = c.take(n_verts * 3);
  L.total = c.off + 256;
  return L;
}

// the five images of a scan, on the device and in pinned staging alike (lt_host.hip): endpoints | endcolors | range | endrem
// | tri.  The colour image is [R,3] int32, or [R] with LT_TRACE_LABEL_IMAGE; `images` is what one transfer of all five moves.
struct lt_hp_out_layout { size_t endpoints, endcolors, range, endrem, tri, images, total; };
static inline lt_hp_out_layout lt_hp_out_layout_of(size_t n_rays, bool label_image) {
  lt_carve c;
  lt_hp_out_layout L;
  L.endpoints = c.take(n_rays * 12);
  L.endcolors = c.take(n_rays * (label_image ? 4 : 12));
  L.range = c.take(n_rays * 4);
  L.endrem = c.take(n_rays * 4);
  L.tri = c.take(n_rays * 4);
  L.images = c.off;
  L.total = c.off + 256;
  return L;
}

// lt_ctrace's per-thread staging (lt_host.hip): rays | endpoints | endcolors | range | endrem | tri
struct lt_ctrace_io_layout { size_t rays, endpoints, endcolors, range, endrem, tri, total; };
static inline lt_ctrace_io_layout lt_ctrace_io_layout_of(size_t n_rays) {
  lt_carve c;
  lt_ctrace_io_layout L;
  L.rays = c.take(n_rays * 12);
  L.endpoints = c.take(n_rays * 12);
  L.endcolors = c.take(n_rays * 12);
  L.range = c.take(n_rays * 4);
  L.endrem = c.take(n_rays * 4);
  L.tri = c.take(n_rays * 4);
  L.total = c.off + 256;
  return L;
}

// the mesh a scene owns after lt_scene_set_mesh_host (lt_api.hip): verts | faces | colors | rem
struct lt_owned_mesh_layout { size_t verts, faces, colors, rem, total; };
static inline lt_owned_mesh_layout lt_owned_mesh_layout_of(size_t n_verts, size_t n_faces) {
  lt_carve c;
  lt_owned_mesh_layout L;
  L.verts = c.take(n_verts * 12);
  L.faces = c.take(n_faces * 12);
  L.colors = c.take(n_verts * 12);
  L.rem = c.take(n_verts * 4);
  L.total = c.off + 256;
  return L;
}

// lt_range_projection's staging (lt_project.hip): inputs | per-point outputs | images, `es` bytes per coordinate
enum {
  LT_RP_POINTS, LT_RP_REM, LT_RP_LABEL, LT_RP_LUT,                                                        // inputs
  LT_RP_POINTS_KEPT, LT_RP_REM_KEPT, LT_RP_LABEL_KEPT, LT_RP_DEPTH, LT_RP_PX, LT_RP_PY, LT_RP_XF, LT_RP_YF,  // per kept point
  LT_RP_IDX_IMG, LT_RP_RANGE_IMG, LT_RP_XYZ_IMG, LT_RP_REM_IMG, LT_RP_LABEL_IMG, LT_RP_COLOR_IMG, LT_RP_MASK_IMG,
  LT_RP_ARRAYS  // 19
};
struct lt_rp_layout { size_t at[LT_RP_ARRAYS], total; };
static inline lt_rp_layout lt_rp_layout_of(size_t n, size_t es, size_t lut_len, size_t cells) {
  const size_t bytes[LT_RP_ARRAYS] = {n * 3 * es, n * 4, n * 4, lut_len * 12,
                                      n * 3 * es, n * 4, n * 4, n * es, n * 4, n * 4, n * es, n * es,
                                      cells * 4, cells * 4, cells * 12, cells * 4, cells * 4, cells * 12, cells * 4};
  lt_carve c;
  lt_rp_layout L;
  for (int k = 0; k < LT_RP_ARRAYS; ++k) L.at[k] = c.take(bytes[k]);
  L.total = c.off + 256;
  return L;
}
