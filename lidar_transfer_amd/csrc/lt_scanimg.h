// lt_scanimg.h -- what a cell of a scan's five images (lt_scan_images, lt_internal.h) holds, written in ONE place: a kernel
// that writes scan images writes its hits and its misses through lt_scan_write_hit and lt_scan_write_miss, and the host
// side walks the five images with lt_scan_copy_of instead of naming them one by one.
#pragma once
#include "lt_internal.h"

// mix(x) of lidarhip.h (uint32, products wrap)
static __host__ __device__ __forceinline__ unsigned lt_mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

#ifdef __HIPCC__
// The miss: what LT_TRACE_WRITE_MISSES makes the render write into a cell that nothing hit, and what a post-render kernel
// turns a lost return into -- end point (0, 0, 0), label 0 or colour (0, 0, 0), remission 0, range 0, tri -1.
static __device__ __forceinline__ void lt_scan_write_miss(const lt_scan_images& im, size_t cell, bool label_image) {
  if (im.endpoints) { im.endpoints[3 * cell] = 0.f; im.endpoints[3 * cell + 1] = 0.f; im.endpoints[3 * cell + 2] = 0.f; }
  if (im.endcolors) {
    if (label_image) im.endcolors[cell] = 0;
    else { im.endcolors[3 * cell] = 0; im.endcolors[3 * cell + 1] = 0; im.endcolors[3 * cell + 2] = 0; }
  }
  if (im.endrem) im.endrem[cell] = 0.f;
  if (im.range) im.range[cell] = 0.f;
  if (im.tri) im.tri[cell] = -1;
}

// The hit of a ray (origin o, normalised direction d) on `face` at distance t, as RayTracer.cpp:73-90 writes it: end point
// o + d * t (BVH.cpp:107), colour of vertex 0 as int -> float -> int (RayTracer.cpp:36, :80-82; the label image is its
// third component: deform's unpack label_image = ray_colors[..., 2], laserscan.py:912), mean remission of the three
// vertices (Triangle.h:69), range t, tri face.
static __device__ __forceinline__ void lt_scan_write_hit(const lt_scan_images& im, size_t cell, bool label_image, float t,
                                                         int face, float ox, float oy, float oz, float dx, float dy,
                                                         float dz, const int* faces, const int* colors,
                                                         const float* rem) {
  const int i0 = faces[3 * (size_t)face], i1 = faces[3 * (size_t)face + 1], i2 = faces[3 * (size_t)face + 2];
  // everything the images need is loaded BEFORE the first store: with the stores in between the compiler waited for
  // each attribute in turn -- key, face, colour, remission were four dependent round trips, three are needed
  int c0 = 0, c1 = 0, c2 = 0;
  float r0 = 0.f, r1 = 0.f, r2 = 0.f;
  if (im.endcolors) {
    c2 = colors[3 * (size_t)i0 + 2];
    if (!label_image) { c0 = colors[3 * (size_t)i0]; c1 = colors[3 * (size_t)i0 + 1]; }
  }
  if (im.endrem) { r0 = rem[i0]; r1 = rem[i1]; r2 = rem[i2]; }
  if (im.endpoints) {
    im.endpoints[3 * cell] = ox + dx * t;
    im.endpoints[3 * cell + 1] = oy + dy * t;
    im.endpoints[3 * cell + 2] = oz + dz * t;
  }
  if (im.endcolors) {
    if (label_image) {
      im.endcolors[cell] = (int)(float)c2;
    } else {
      im.endcolors[3 * cell] = (int)(float)c0;
      im.endcolors[3 * cell + 1] = (int)(float)c1;
      im.endcolors[3 * cell + 2] = (int)(float)c2;
    }
  }
  if (im.endrem) im.endrem[cell] = ((r0 + r1) + r2) / 3.0f;
  if (im.range) im.range[cell] = t;
  if (im.tri) im.tri[cell] = face;
}

// One resolved echo of a beam with a divergence (lt_echo.hip) into a set of images and its fraction image: the values are
// the caller's -- the miss among them, which it spells like lt_scan_write_miss --, the colour image is the label image,
// range and tri are mandatory there.
static __device__ __forceinline__ void lt_scan_write_echo(const lt_scan_images& im, float* fraction, size_t cell, float px,
                                                          float py, float pz, int label, float range, float rem, int tri,
                                                          float frac) {
  if (im.endpoints) { im.endpoints[3 * cell] = px; im.endpoints[3 * cell + 1] = py; im.endpoints[3 * cell + 2] = pz; }
  if (im.endcolors) im.endcolors[cell] = label;
  im.range[cell] = range;
  if (im.endrem) im.endrem[cell] = rem;
  im.tri[cell] = tri;
  if (fraction) fraction[cell] = frac;
}
#endif

// ---- host side ------------------------------------------------------------------------------------------------------
// "three finite numbers" (written so that a NaN fails)
static inline bool lt_finite3(const float* v) {
  return v[0] - v[0] == 0.f && v[1] - v[1] == 0.f && v[2] - v[2] == 0.f;
}

// Image k (0 .. LT_SCAN_IMAGES - 1: endpoints, endcolors, range, endrem, tri) of a scan of n_rays as a copy has it: the
// caller's array on the host, where the image is on the other side (`dev`: device memory, or pinned staging laid out like
// it), and its bytes.  host NULL: the caller does not want it.
#define LT_SCAN_IMAGES 5
struct lt_scan_copy { void* host; void* dev; size_t bytes; };
static inline lt_scan_copy lt_scan_copy_of(const lt_scan_images& host, const lt_scan_images& dev, int k, size_t n_rays,
                                           bool label_image) {
  void* const h[LT_SCAN_IMAGES] = {host.endpoints, host.endcolors, host.range, host.endrem, host.tri};
  void* const d[LT_SCAN_IMAGES] = {dev.endpoints, dev.endcolors, dev.range, dev.endrem, dev.tri};
  const size_t b[LT_SCAN_IMAGES] = {n_rays * 12, n_rays * (label_image ? 4 : 12), n_rays * 4, n_rays * 4, n_rays * 4};
  return {h[k], d[k], b[k]};
}
// the five images inside a carved buffer (L: lt_hp_out_layout or lt_ctrace_io_layout of lt_layouts.h)
template <class LAYOUT>
static inline lt_scan_images lt_scan_images_at(char* base, const LAYOUT& L) {
  return {(float*)(base + L.endpoints), (int*)(base + L.endcolors), (float*)(base + L.range), (float*)(base + L.endrem),
          (int*)(base + L.tri)};
}
// `dev` without the images that `host` does not want
static inline lt_scan_images lt_scan_images_wanted(const lt_scan_images& dev, const lt_scan_images& host) {
  return {host.endpoints ? dev.endpoints : nullptr, host.endcolors ? dev.endcolors : nullptr,
          host.range ? dev.range : nullptr, host.endrem ? dev.endrem : nullptr, host.tri ? dev.tri : nullptr};
}
