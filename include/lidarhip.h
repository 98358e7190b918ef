/*
 * lidarhip.h -- C ABI of liblidarhip.so, the MI355X (gfx950) virtual-LiDAR ray-cast path.
 *
 * Drop-in boundary for PRBonn/lidar_transfer's native raytracer: every entry point below names
 * the reference interface it replaces (paths relative to the reference repository).  Plain C
 * types only -- pointers, sizes, an opaque handle -- so the library can be bound from ctypes,
 * Cython, cgo, JNI ... exactly where the reference binds `ctrace`
 * (auxiliary/raytracer/RayTracerCython.pyx:5-7).
 *
 * Conventions
 *   - every function returns an int status: LT_OK (0) or a negative LT_ERR_* code; the message
 *     of the last failure on the calling thread is available from lt_last_error();
 *   - "host" pointers are ordinary process memory, "dev" pointers are HIP device pointers on the
 *     scene's device (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - array layouts are the reference's: all arrays flat and C-contiguous, rays / endpoints /
 *     endcolors at 3*(W*j + i), range / endrem / tri at W*j + i, W = n_rays / height
 *     (auxiliary/raytracer/RayTracer.cpp:56, :65, :86-89); `colors` holds 3 ints per VERTEX and
 *     only vertex 0 of the hit face is reported (RayTracer.cpp:75, Triangle.h:56-61).
 */
#ifndef LIDARHIP_H
#define LIDARHIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_OK 0
#define LT_ERR_INVALID_ARG (-1)  /* NULL pointer, negative size, height <= 0 ...                      */
#define LT_ERR_NO_MEMORY (-2)    /* hipMalloc failed                                                  */
#define LT_ERR_HIP (-3)          /* any other HIP runtime error (message has the HIP error string)    */
#define LT_ERR_BAD_INDEX (-4)    /* a face references a vertex outside [0, n_verts)                   */
#define LT_ERR_NOT_BUILT (-5)    /* trace requested before lt_scene_build                             */
#define LT_ERR_TOO_LARGE (-6)    /* more than LT_MAX_FACES triangles                                  */

#define LT_MAX_FACES (1 << 28)

/* trace flags */
#define LT_TRACE_WRITE_MISSES 1u /* write 0 / tri = -1 for rays that hit nothing (otherwise outputs   */
                                 /* are left untouched for misses, as in RayTracer.cpp:73)            */
#define LT_TRACE_COUNT 2u        /* accumulate nodes visited / triangles tested into the scene stats  */
#define LT_TRACE_NORM_EXACT 4u   /* seed the direction normalisation (Vector3.h:73-89) with a correctly */
                                 /* rounded 1/sqrt instead of the replayed x86 RSQRTSS seed (default:   */
                                 /* the Intel table); vendor independent, last-ulp different            */
#define LT_TRACE_NORM_AMD 16u    /* replay the RSQRTSS seed of an AMD host (measured on EPYC 9575F, Zen 5) instead */
                                 /* of the Intel one: the reference as it runs on the MI355X box's own CPU      */
#define LT_TRACE_LABEL_IMAGE 8u  /* `endcolors` receives [n_rays] ints: colour channel 2 only = the      */
                                 /* semantic label image `deform` unpacks (label_image = ray_colors[:, :, */
                                 /* 2], laserscan.py:912) instead of [n_rays, 3]; device-pointer calls    */

/* Per-phase timings (hipEvent, milliseconds) and work counters of the last build / trace of a scene. */
typedef struct lt_stats {
  float ms_bounds;     /* scene bounds reduction                                        */
  float ms_morton;     /* centroid Morton codes                                         */
  float ms_sort;       /* LSD radix sort (3 passes of 10-bit digits)                    */
  float ms_gather;     /* sorted triangle records + padded leaf boxes                   */
  float ms_segtree;    /* min/max segment tree over the leaf boxes                      */
  float ms_hierarchy;  /* Karras topology into 4-wide nodes + child boxes               */
  float ms_build;      /* whole build, first to last kernel                             */
  float ms_trace;      /* ray-cast kernel(s): k_trace4, or the scatter sequence         */
  int n_faces;
  int n_nodes;         /* node slots (n_faces - 1)                                      */
  int n_rays;
  int n_hits;          /* valid after a LT_TRACE_COUNT trace                            */
  unsigned long long nodes_visited; /* 4-wide nodes fetched (lbvh) / candidate bins (scatter) */
  unsigned long long tris_tested;   /* Moller-Trumbore evaluations, summed over rays    */
  unsigned long long stack_overflows; /* rays that spilled past the LDS stack           */
  unsigned long long entries_culled;  /* always 0; kept for the layout.  It counted the stack entries dropped at pop by the
                                         LT_TRACE_CULL A/B of the lbvh ray cast, which is gone: a measured negative,
                                         recorded in profiles/r04/DESIGN_rounds_1_to_4.md */
} lt_stats;

typedef struct lt_scene lt_scene; /* opaque: device workspace + BVH of one mesh */

/* ---- one-call drop-in ----------------------------------------------------------------------- */

/*
 * lt_ctrace -- same 14 parameters, order and meaning as the reference's
 *   extern "C" void ctrace(float* rays, float* origin, float* verts, int* faces, int* colors,
 *                          float* rem, int n_rays, int n_verts, int n_faces, int height,
 *                          float* endpoints, int* endcolors, float* range, float* endrem)
 * (auxiliary/raytracer/RayTracer.cpp:116-124), but returns a status instead of void.
 * All pointers are HOST pointers; the call uploads the mesh and rays to the current HIP device,
 * casts the rays and copies the four outputs back.  State (workspace, stream, the binned ray set of the previous
 * call) is kept per calling THREAD: concurrent callers do not serialise each other.  As in the reference, outputs
 * are written only for rays that hit (the caller pre-zeroes them, fusion_lidar.py:440-447).
 */
int lt_ctrace(const float* rays, const float* origin, const float* verts, const int* faces,
              const int* colors, const float* rem, int n_rays, int n_verts, int n_faces, int height,
              float* endpoints, int* endcolors, float* range, float* endrem);

/* As lt_ctrace, plus the hit-triangle image `tri` (face index, -1 = miss; may be NULL) and
 * optional statistics (may be NULL).  The reference has no triangle output (IntersectionInfo.h:9-13
 * keeps the object pointer internal). */
int lt_ctrace_ex(const float* rays, const float* origin, const float* verts, const int* faces,
                 const int* colors, const float* rem, int n_rays, int n_verts, int n_faces, int height,
                 float* endpoints, int* endcolors, float* range, float* endrem, int* tri,
                 lt_stats* stats);

/* ---- host buffers, pipelined: a sequence of scans with their transfers overlapped -------------------------------- */

typedef struct lt_hostpipe lt_hostpipe; /* opaque: `depth` scans in flight, uploader + launcher threads, HIP streams */

/*
 * The work of lt_ctrace for a SEQUENCE of scans that share one ray set (one target sensor model, as in the reference's
 * batch loop lidar_deform.py:393-462, which calls throw_rays_at_mesh -> ctrace once per output scan,
 * fusion_lidar.py:434-451): while scan i renders, scan i + 1 uploads and scan i - 1 downloads.
 *   rays    HOST [n_rays,3] f32, uploaded and binned once;  depth = scans in flight (3 overlap; from 4 on two uploader threads share the link: +7 %)
 *   flags   LT_TRACE_LABEL_IMAGE | LT_TRACE_NORM_EXACT | LT_TRACE_NORM_AMD
 * Unlike lt_ctrace the pipe writes EVERY cell of the output images (misses: 0, tri -1) -- what the reference's
 * pre-zeroed arrays (fusion_lidar.py:440-447) contain after ctrace -- so nothing is uploaded for the outputs.
 */
int lt_hostpipe_create(lt_hostpipe** pipe, const float* rays, int n_rays, int height, int depth, unsigned flags,
                       int device);

/* Queue one scan: mesh in HOST arrays with the layouts of ctrace (RayTracer.cpp:116-124), except that `colors` may be
 * the uint8 [n_verts,3] array get_mesh returns (colors_are_u8 != 0; fusion_lidar.py:423) instead of its int32 copy
 * (:435) -- a quarter of the bytes on the link.  Output HOST arrays as for lt_ctrace_ex (any may be NULL).  Returns
 * immediately; every input and output array must stay valid and untouched until lt_hostpipe_wait(ticket),
 * lt_hostpipe_flush, or until `depth` further scans have been submitted (a submit that needs the slot of an older
 * scan completes that scan first -- its status is what this call returns).  Pageable and pinned memory both run at
 * the wire rate here; pinned (lt_host_alloc) input additionally frees the worker thread during the transfer. */
int lt_hostpipe_submit(lt_hostpipe* pipe, const float* origin, const float* verts, const int* faces,
                       const void* colors, int colors_are_u8, const float* rem, int n_verts, int n_faces,
                       float* endpoints, int* endcolors, float* range, float* endrem, int* tri, int* ticket);

/* Block until the scan with this ticket is complete: its images are in the caller's arrays. */
int lt_hostpipe_wait(lt_hostpipe* pipe, int ticket);
/* Complete everything submitted so far; reports deferred device-side errors (LT_ERR_BAD_INDEX). */
int lt_hostpipe_flush(lt_hostpipe* pipe);
int lt_hostpipe_destroy(lt_hostpipe* pipe);

/* Page-locked host memory (hipHostMalloc) for callers that want their arrays DMA-able without staging. */
int lt_host_alloc(void** p, size_t bytes);
int lt_host_free(void* p);

/* ---- split API: build once, trace many, device-resident buffers ----------------------------- */

/* Create an empty scene on HIP device `device` (-1 = current device).  Replaces the per-call
 * `vector<Object*> objects` + `BVH bvh(&objects)` of RayTracer.cpp:22, :54. */
int lt_scene_create(lt_scene** scene, int device);

/* Attach a mesh given as DEVICE pointers (borrowed: they must stay valid until the last trace of
 * this mesh has completed).  Replaces the triangle de-indexing loop RayTracer.cpp:32-51. */
int lt_scene_set_mesh_dev(lt_scene* scene, const float* verts, const int* faces, const int* colors,
                          const float* rem, int n_verts, int n_faces);

/* Same from HOST pointers: the scene copies the mesh into device buffers it owns. */
int lt_scene_set_mesh_host(lt_scene* scene, const float* verts, const int* faces, const int* colors,
                           const float* rem, int n_verts, int n_faces, void* stream);

/* Build the linear BVH (Morton codes -> radix sort -> Karras topology -> child boxes) on `stream`.
 * Asynchronous unless `stats` is non-NULL (then it synchronises and fills the ms_* fields).
 * Replaces BVH::BVH / BVH::build (auxiliary/raytracer/BVH.cpp:116-126, :143-243). */
int lt_scene_build(lt_scene* scene, void* stream, lt_stats* stats);

/* Cast n_rays rays (DEVICE pointer, [n_rays,3] f32, normalised inside like Vector3.h:73-89) from
 * `origin` (HOST pointer to 3 floats) against the built scene on `stream`; outputs are DEVICE
 * pointers, any of them may be NULL.  Asynchronous unless `stats` is non-NULL.
 * Replaces the OpenMP ray loop RayTracer.cpp:62-92 incl. BVH::getIntersection (BVH.cpp:19-110). */
int lt_scene_trace_dev(lt_scene* scene, const float* rays, const float* origin, int n_rays, int height,
                       float* endpoints, int* endcolors, float* range, float* endrem, int* tri,
                       unsigned flags, void* stream, lt_stats* stats);

/* ---- single-origin fast path: ray set + triangle scatter ------------------------------------------ */

typedef struct lt_rayset lt_rayset; /* opaque: normalised directions of one ray batch, binned by direction */

/* Prepare a ray batch (DEVICE pointer rays[n_rays,3] f32) for lt_scene_render_dev: normalise the
 * directions exactly as the trace kernel does (Vector3.h:73-89; flags & LT_TRACE_NORM_EXACT selects
 * the seed) and bin them by azimuth x elevation.  A sensor model's rays do not change from scan to
 * scan (create_rays, laserscan.py:1092-1119, depends only on the YAML), so one rayset serves a whole
 * sequence -- it is read-only once created (the state of a render lives in the scene), so ONE rayset can be used by
 * any number of scenes and streams at the same time.  The call returns when the ray set is ready (it synchronises
 * `stream` once -- a ray set is built once per sensor model); `rays` is not referenced afterwards. */
int lt_rayset_create_dev(lt_rayset** rayset, const float* rays, int n_rays, int height, unsigned flags,
                         void* stream);
/* The same with a bin grid of the caller's size: nb_az / nb_el > 0 are the numbers of azimuth / elevation bins (more than
 * 8192 / 4096 are clamped to that), 0 keeps lt_rayset_create_dev's rule for that axis (W = n_rays / height columns, refitted
 * to W - 1 when the rays close the circle inclusively; `height` rows) -- (0, 0) IS lt_rayset_create_dev.  A given nb_az is
 * not refitted.  The azimuth grid is always the full periodic circle with the phase of ray 0; how far the rays sit from
 * their bins' centres is measured, so every grid renders the same image and only the speed differs: fastest when the rays
 * sit on bin centres.  For a sensor whose W columns span only `span` degrees (lt_create_rays_sector_dev) that is
 * nb_az = round(W * 360 / span): the occupied bins are then a contiguous arc and the others stay empty. */
int lt_rayset_create_grid_dev(lt_rayset** rayset, const float* rays, int n_rays, int height, int nb_az, int nb_el,
                              unsigned flags, void* stream);
int lt_rayset_destroy(lt_rayset* rayset);

/* Closest hit of every ray of `rayset`, all cast from `origin` (HOST pointer to 3 floats), against the
 * scene's CURRENT mesh -- no BVH needed: the triangles are streamed once, each visits only the ray
 * bins inside its angular bounds and merges hits by atomic min over (t, face).  Same outputs, flags and
 * bit-identical results as lt_scene_build + lt_scene_trace_dev; replaces BVH::build + the ray loop
 * (BVH.cpp:143-243, RayTracer.cpp:62-92) for the reference's only call pattern, one origin per call
 * (RayTracer.cpp:58).  A scene renders one scan at a time (its mesh and its z-min image are per scene); the
 * rayset may be shared. */
int lt_scene_render_dev(lt_scene* scene, lt_rayset* rayset, const float* origin, float* endpoints,
                        int* endcolors, float* range, float* endrem, int* tri, unsigned flags, void* stream,
                        lt_stats* stats);

/* The same for up to 8 scans in ONE call -- n_scans (scene, rayset) pairs, the scenes distinct and each with
 * its own current mesh, the raysets normally all the same one (one sensor model: its bin grid then stays in
 * every L2); origins[3 * i ..] is scan i's origin (HOST), the output arguments are HOST arrays
 * of n_scans DEVICE pointers (an array, or single entries of it, may be NULL).  The three kernels of the
 * scatter strategy are launched once for the whole batch instead of once per scan: with tens of thousands of
 * scans per second, the time a hardware queue spends between small kernels is what limits throughput
 * (DESIGN.md section 9).  Results are those of n_scans separate lt_scene_render_dev calls.  Asynchronous;
 * LT_TRACE_COUNT is not accepted. */
int lt_scene_render_batch_dev(int n_scans, lt_scene* const* scenes, lt_rayset* const* raysets,
                              const float* origins, float* const* endpoints, int* const* endcolors,
                              float* const* range, float* const* endrem, int* const* tri, unsigned flags,
                              void* stream);

/* A sensor RIG: the scene's CURRENT mesh rendered from up to 8 sensors in ONE call.  Sensor i is raysets[i], cast from
 * origins[3 * i ..] (HOST), into its own five DEVICE images (the output arguments as in the batch call: an array, or single
 * entries of it, may be NULL); the same ray set may appear more than once, e.g. with two origins.  The flags are those of
 * the batch call (LT_TRACE_COUNT is not accepted); asynchronous on `stream`.  Results are those of n_sensors successive
 * lt_scene_render_dev calls on that scene, byte for byte, including what a miss leaves untouched.  n_sensors == 0 does
 * nothing, n_sensors == 1 IS lt_scene_render_dev.  LT_ERR_INVALID_ARG: n_sensors < 0 or > 8, a NULL ray set, a ray set on
 * another device than the scene.  The z-min cells and queues of sensors 1 .. 7 are render-state slots of the scene, allocated
 * when a rig first needs them: a scene that never renders a rig holds nothing more than before. */
int lt_scene_render_rig_dev(lt_scene* scene, int n_sensors, lt_rayset* const* raysets, const float* origins,
                            float* const* endpoints, int* const* endcolors, float* const* range, float* const* endrem,
                            int* const* tri, unsigned flags, void* stream);

/* Measurement hook: record the caller's two hipEvent_t (passed as void*) on the launch stream immediately
 * before and after the dominant kernel (k_sc_tris / k_trace4) of the NEXT lt_scene_render_dev /
 * lt_scene_trace_dev call; one shot, no synchronisation.  bench.py uses it for the roofline figure. */
int lt_scene_set_probe(lt_scene* scene, void* ev_start, void* ev_stop);

/* Synchronise the scene's last stream and report deferred device-side errors (LT_ERR_BAD_INDEX). */
int lt_scene_status(lt_scene* scene);

/* Free the workspace.  Replaces the delete loop RayTracer.cpp:110-113 and BVH::~BVH (BVH.cpp:112-114). */
int lt_scene_destroy(lt_scene* scene);

/* ---- scan model: rays and spherical projection ------------------------------------------------ */

/* Unit ray direction per (beam, azimuth) cell into a DEVICE buffer rays[H*W*3] (f32, row-major
 * h*W + w).  Replaces MultiSemLaserScan.create_rays (auxiliary/laserscan.py:1092-1119), quirks
 * included: linspace(0, 360, W) holds both end points, beam_angles are ignored, float64
 * trigonometry is cast to float32 last.  fov_up / fov_down in degrees. */
int lt_create_rays_dev(double fov_up, double fov_down, int H, int W, float* rays, void* stream);

/* The same rays for a sensor mounted at a pose of its own: every direction, still in float64, is turned by `rot`
 * (HOST, [9] row-major rotation of the pose; NULL = identity = the call above) as ((r0*x + r1*y) + r2*z) per
 * component, each product and sum rounded on its own, and cast to float32 last.  Asynchronous on `stream`. */
int lt_create_rays_pose_dev(double fov_up, double fov_down, int H, int W, const double* rot, float* rays, void* stream);

/* The rays of a sensor with a BEAM TABLE: lt_create_rays_dev's expressions with beams_deg[h] (HOST, [H] float64, degrees,
 * row 0 first -- descending, so that row 0 is the highest beam as fov_up is above) in place of the evenly spaced angle of
 * row h: p = pi/2 - beams_deg[h] / 180 * pi, then the same three products; with `rot` (HOST [9], NULL = none)
 * lt_create_rays_pose_dev's rotation in float64 before the one cast to float32.  A table equal to
 * linspace(fov_up, fov_down, H) gives lt_create_rays_dev's / lt_create_rays_pose_dev's rays bit for bit.  The table is
 * copied to the device once per call and the call waits for `stream`: it is made once per sensor model. */
int lt_create_rays_beams_dev(const double* beams_deg, int H, int W, const double* rot, float* rays, void* stream);

/* The rays of a sensor with a horizontal SECTOR: its W columns span `span_deg` degrees (0 < span < 360) around the direction
 * `center_deg` (atan2(y, x) in the sensor's frame: 0 is +x, positive to the left; |center| <= 360).  Column 0 is the left
 * edge, columns run clockwise seen from above as in the full image; column w is the cell [w, w + 1) * span / W and its ray
 * leaves through the cell's CENTRE: yaw_deg = (-center - span / 2) + (w + 0.5) * (span / W), yaw = yaw_deg / 180 * pi (not
 * wrapped), then lt_create_rays_dev's expressions.  The row term is linspace(fov_up, fov_down, H), or beams_deg[h] as in
 * lt_create_rays_beams_dev when `beams_deg` (HOST [H], NULL = evenly spaced) is given; `rot` (HOST [9], NULL = none) is
 * lt_create_rays_pose_dev's rotation.  Asynchronous on `stream` without a table; with one the call waits for `stream`. */
int lt_create_rays_sector_dev(const double* beams_deg, double fov_up, double fov_down, int H, int W, double center_deg,
                              double span_deg, const double* rot, float* rays, void* stream);

/* The rays of a sensor with a BEAM TABLE whose beams carry AZIMUTH OFFSETS: the lasers of one firing do not share an azimuth.
 * az_deg[h] (HOST, [H] float64, degrees, |.| <= 90, in the table's row order; NULL = none) is measured like `center_deg`:
 * atan2(y, x) in the sensor's frame, positive to the left -- beam h of column w looks az_deg[h] to the LEFT of the column's
 * nominal direction: yaw_deg = nominal(w) - az_deg[h] in float64, nominal(w) being lt_create_rays_dev's column (linspace(0,
 * 360, W) + 180, wrapped) or, with `sec` (HOST [2]: center_deg, span_deg as in lt_create_rays_sector_dev; NULL = the full
 * circle), the centre of the sector's cell w; no further wrap.  The rest is lt_create_rays_beams_dev's: beams_deg (HOST [H],
 * mandatory), `rot` (HOST [9], NULL = none), one cast to float32.  A row whose offset is 0 gets the bits it has without
 * offsets.  The call waits for `stream`. */
int lt_create_rays_beams_az_dev(const double* beams_deg, const double* az_deg, int H, int W, const double* sec,
                                const double* rot, float* rays, void* stream);

#define LT_PROJ_REMOVE 1u /* `remove=True`: drop depth == 0 and points whose proj_y is outside [0, 1]   */
#define LT_PROJ_NEW 2u    /* do_range_projection_new: depth == 0 is always dropped (laserscan.py:306-309) */
/* LT_PROJ_BEAM_ROWS -- the image rows are the beams of a TABLE (a target sensor whose beams are not evenly spaced), defined
 * together with LT_PROJ_NEW | LT_PROJ_REMOVE only (any other combination: LT_ERR_INVALID_ARG), for lt_range_projection_dev,
 * lt_range_projection and lt_range_projection_batch_dev.  `beam_angles` then carries Brad[H] (the table in radians,
 * descending: row 0 is the highest beam) followed by halfw[H] (half the smaller gap to the neighbouring beams in radians;
 * the one existing gap for the first and the last row; unused for H == 1), and n_beams == H (at most 511).  Per point: the
 * column as without the flag; the pitch q in the cloud's dtype (asin correctly rounded in either dtype), widened to float64; row = the first
 * minimum of |q - Brad[k]|; the point is kept iff |q - Brad[row]| <= halfw[row] (H == 1: iff fov_down <= q <= fov_up in
 * radians) -- a beam samples its own direction, not the gap beside it.  depth == 0 and NaN as without the flag; the z-min
 * rule is the same.  proj_y is the row, proj_yf the winner's pitch in radians (the cloud's dtype), proj_x / proj_xf as
 * without the flag; an EMPTY cell holds 0 in all four. */
#define LT_PROJ_BEAM_ROWS 4u
/* LT_PROJ_SECTOR -- the image columns are those of a horizontal SECTOR (lt_create_rays_sector_dev), defined together with
 * LT_PROJ_NEW | LT_PROJ_REMOVE only, with or without LT_PROJ_BEAM_ROWS (any other combination: LT_ERR_INVALID_ARG), for the
 * same three calls.  The sector's two numbers -- yc = -center / 180 * pi, the yaw of its middle (|yc| <= pi), and its width
 * in radians (0 < span < 2 pi) -- are set beforehand: lt_projector_set_sector for lt_range_projection_batch_dev,
 * lt_range_projection_set_sector for the two single-cloud calls (below); the flag without a sector set is
 * LT_ERR_INVALID_ARG, so no existing signature, struct or argument changes its meaning (`beam_angles` / `n_beams` are as
 * without the flag; at most 510 rows / 1022 angles).  Per point, in the cloud's dtype T with pi, yc and span rounded to T: yaw = -atan2(y, x); d = yaw - yc, plus
 * 2 pi if d < -pi, minus 2 pi if d >= pi (a sector may straddle the seam behind the sensor); u = d / span + 0.5; the point
 * is kept iff 0 <= u < 1 on top of every condition without the flag; proj_xf = u * W, proj_x = floor(proj_xf) clamped to
 * [0, W - 1] -- the column whose ray is nearest.  Rows, the z-min rule and the empty cells are as without the flag. */
#define LT_PROJ_SECTOR 8u
/* The sector that LT_PROJ_SECTOR reads in lt_range_projection_dev / lt_range_projection (one per process, kept until set
 * again; span == 0 clears it).  LT_ERR_INVALID_ARG unless |yaw_center| <= pi and 0 < span < 2 pi (radians). */
int lt_range_projection_set_sector(double yaw_center, double span);
/* LT_PROJ_BEAM_AZIMUTH -- the beams of the table carry AZIMUTH OFFSETS (lt_create_rays_beams_az_dev), defined together with
 * LT_PROJ_BEAM_ROWS | LT_PROJ_NEW | LT_PROJ_REMOVE only, with or without LT_PROJ_SECTOR (any other combination:
 * LT_ERR_INVALID_ARG), for the same three calls.  The offsets -- az[H] in radians, az = az_deg / 180 * pi, in the table's row
 * order -- are set beforehand: lt_projector_set_beam_azimuth for lt_range_projection_batch_dev,
 * lt_range_projection_set_beam_azimuth for the two single-cloud calls; the flag without offsets set for exactly H rows is
 * LT_ERR_INVALID_ARG, so no existing signature, struct or argument changes its meaning.  Per point, in the cloud's dtype T: the
 * row and every keep condition are LT_PROJ_BEAM_ROWS'; then, with a = (T)az[row], the point's NOMINAL yaw is
 * y' = -atan2(y, x) + a -- the column whose beam `row` looks at the point.  Full circle: y' - 2 pi if y' > pi, y' + 2 pi if
 * y' < -pi (only strictly outside: the closed interval of the plain rule stays), proj_xf = 0.5 * (y' / pi + 1) * W, proj_x =
 * floor clamped to [0, W - 1].  With LT_PROJ_SECTOR: d = y' - yc, then that flag's wrap, u, keep rule and column.  proj_xf
 * is the nominal coordinate.  The z-min rule and the empty cells are LT_PROJ_BEAM_ROWS'. */
#define LT_PROJ_BEAM_AZIMUTH 16u
/* The offsets that LT_PROJ_BEAM_AZIMUTH reads in lt_range_projection_dev / lt_range_projection (one set per process, kept
 * until set again; NULL or H == 0 clears them): az_rad HOST [H], copied.  LT_ERR_INVALID_ARG unless 1 <= H <= 511 and every
 * offset is finite with |az| <= pi / 2. */
int lt_range_projection_set_beam_azimuth(const double* az_rad, int H);

/*
 * lt_range_projection_dev -- point cloud -> H x W spherical image, closest point per cell (atomic
 * z-min, lowest point index among equal depths).  Replaces LaserScan.do_range_projection
 * (auxiliary/laserscan.py:202-292), do_range_projection_new(method="depth") (:294-391) and
 * SemLaserScan.do_label_projection[_new] (:645-649, :672-676).
 *
 *   points      [n,3] f32 (is_f64 = 0) or f64 (is_f64 = 1) -- arithmetic is done in that dtype, as
 *               numpy does for the array the reference holds; rem [n] f32 and label [n] u32 may be NULL
 *   fov_up/down degrees (down negative); beam_angles: HOST array of n_beams radians or NULL
 *   color_lut   DEVICE [lut_len,3] f32 or NULL (SemLaserScan.color_lut)
 *   *_kept      per-point outputs COMPACTED to the points that survive the removals, in input
 *               order (what remove_points leaves in self.points / remissions / label, plus depth
 *               = unproj_range, integer and float pixel coordinates); capacity n; any may be NULL
 *   *_img       [H*W] images: idx = index into the compacted arrays (-1 empty), range, xyz [H*W,3],
 *               remission, label, color [H*W,3], mask = (idx > 0) as the reference computes it;
 *               empty cells receive range_init / rem_init / xyz_init (reference: -1 for the old
 *               variant, 0 / -1 for the new one), label 0, color 0
 *   n_kept      HOST int: number of surviving points (the call synchronises `stream`)
 * All array pointers are DEVICE pointers except beam_angles and n_kept.
 */
int lt_range_projection_dev(const void* points, int is_f64, const float* rem, const unsigned* label, int n,
                            double fov_up, double fov_down, int H, int W, const double* beam_angles,
                            int n_beams, unsigned flags, const float* color_lut, int lut_len,
                            void* points_kept, float* rem_kept, unsigned* label_kept, void* depth_kept,
                            int* proj_x_kept, int* proj_y_kept, void* proj_xf_kept, void* proj_yf_kept,
                            int* idx_img, float* range_img, float* xyz_img, float* rem_img, int* label_img,
                            float* color_img, float* mask_img, float range_init, float rem_init,
                            float xyz_init, int* n_kept, void* stream);

/* Same with HOST pointers throughout (uploads, runs lt_range_projection_dev, downloads). */
int lt_range_projection(const void* points, int is_f64, const float* rem, const unsigned* label, int n,
                        double fov_up, double fov_down, int H, int W, const double* beam_angles, int n_beams,
                        unsigned flags, const float* color_lut, int lut_len, void* points_kept,
                        float* rem_kept, unsigned* label_kept, void* depth_kept, int* proj_x_kept,
                        int* proj_y_kept, void* proj_xf_kept, void* proj_yf_kept, int* idx_img,
                        float* range_img, float* xyz_img, float* rem_img, int* label_img, float* color_img,
                        float* mask_img, float range_init, float rem_init, float xyz_init, int* n_kept);

/*
 * lt_range_projection_batch_dev -- the same projection for SEVERAL clouds in one launch sequence, nothing read back by the
 * host, no memsets between calls: the `number_of_scans` observations of one output scan (MultiSemLaserScan.deform,
 * auxiliary/laserscan.py:874-881: do_range_projection_new + do_label_projection_new per source scan; :841-843 for the merged
 * cloud of the `cp` adaption).  Same per-point arithmetic and the same winner per cell as lt_range_projection_dev; the
 * per-point COMPACTED outputs of that call are not produced -- what the callers downstream consume are images:
 *
 *   lt_projector   owns the z-min workspace (one per caller thread / HIP stream; calls on one projector are serialised)
 *   clouds[k]      DEVICE pointers of cloud k: points [n,3] f32 / f64 (is_f64, one dtype per call), rem [n] f32 or NULL,
 *                  label [n] u32 or NULL
 *   out[k]         [H*W] DEVICE images of cloud k, every member may be NULL:
 *                    idx            index of the winning point among the KEPT points (remove_points numbering), -1 empty
 *                    range, xyz [H*W,3], rem, label, color [H*W,3], mask    as lt_range_projection_dev
 *                    label_folded   float32 floor(label * 256 * 256): the colour image TSDFVolume.integrate folds from
 *                                   proj_label3 (laserscan.py:893-895, fusion_lidar.py:260-264) -- feed it to
 *                                   lt_tsdf_integrate_dev / lt_fusion_scan_dev as color_im
 *                    proj_x, proj_y int32 pixel of the winner; proj_xf, proj_yf its unclamped coordinates in the points'
 *                                   dtype (do_range_projection_new's proj_x / proj_y / proj_x_float / proj_y_float,
 *                                   laserscan.py:384-388; an EMPTY cell holds the values of the last kept point, numpy's
 *                                   index -1)
 *                    n_kept         DEVICE int: number of points that survived the removals
 * Asynchronous on `stream`; more than 8 clouds are processed in groups of 8.
 */
typedef struct lt_projector lt_projector;
typedef struct lt_cloud {
  const void* points;
  const float* rem;
  const unsigned* label;
  int n;
} lt_cloud;
typedef struct lt_proj_images {
  int* idx;
  float* range;
  float* xyz;
  float* rem;
  int* label;
  float* color;
  float* mask;
  float* label_folded;
  int* proj_x;
  int* proj_y;
  void* proj_xf;
  void* proj_yf;
  int* n_kept;
  double* bnds; /* [6] {xmin, xmax, ymin, ymax, zmin, zmax} of the KEPT points: SemLaserScan.get_bnds() after the projection's
                 * remove_points (laserscan.py:678-681, read by deform('mergemesh') :957); (+inf, -inf) when none is kept */
} lt_proj_images;
int lt_projector_create(lt_projector** projector, int device);
int lt_projector_destroy(lt_projector* projector);
/* The sector that LT_PROJ_SECTOR reads in this projector's lt_range_projection_batch_dev calls (kept until set again;
 * span == 0 clears it): yaw_center = -center / 180 * pi, span the width, radians.  LT_ERR_INVALID_ARG unless
 * |yaw_center| <= pi and 0 < span < 2 pi.  Host side only: it takes effect with the next call. */
int lt_projector_set_sector(lt_projector* projector, double yaw_center, double span);
/* The offsets that LT_PROJ_BEAM_AZIMUTH reads in this projector's lt_range_projection_batch_dev calls (kept until set again;
 * NULL or H == 0 clears them): az_rad HOST [H] radians in the table's row order, copied.  LT_ERR_INVALID_ARG unless
 * 1 <= H <= 511 and every offset is finite with |az| <= pi / 2.  Host side only: it takes effect with the next call. */
int lt_projector_set_beam_azimuth(lt_projector* projector, const double* az_rad, int H);
int lt_range_projection_batch_dev(lt_projector* projector, int n_clouds, const lt_cloud* clouds, int is_f64,
                                  double fov_up, double fov_down, int H, int W, const double* beam_angles, int n_beams,
                                  unsigned flags, const float* color_lut, int lut_len, const lt_proj_images* out,
                                  float range_init, float rem_init, float xyz_init, void* stream);

/* ---- before the projection: raw scans -> the clouds `deform` projects ---------------------------- */

/* From the bytes of velodyne/N.bin ([n,4] f32 x, y, z, remission) and labels/N.label ([n] u32) of the source scans of one
 * output scan to the clouds MultiSemLaserScan.deform projects; replaces open_multiple_scans (auxiliary/laserscan.py:776-817)
 * and the first statement of each deform branch (:845 / :878 / :949).  Per raw point of slot i, in file order:
 *   1. l = label & 0xFFFF (:588)
 *   2. dropped if (i != 0 and l in moving) or l in ignore (:802-807; n_scans == 1: only `ignore`, :809-817)
 *   3. kept points keep their file order, slots follow each other in slot order (stable; np.concatenate, :939-945)
 *   4. q = A [x y z 1]^T in float64 with A = poses[i] (apply_pose, :98-109), then r = B [q 1]^T with B = back -- two
 *      transforms, each rounded to float64; back == NULL: q is the result (world coordinates)
 *   5. every row as ((m0*x + m1*y) + m2*z) + m3, products and sums rounded separately (no fused multiply-add);
 *      the remission is xyzr[3] unchanged, the label is l
 * scans   HOST array of n_scans (1 .. LT_INGEST_MAX_SCANS) descriptors of DEVICE buffers, in the slot order of
 *         open_multiple_scans (primary scan first); xyzr 16-byte aligned
 * poses   HOST [n_scans][16] row-major float64: the pose of every slot's scan;  back  HOST [16]: inv(poses[idx]) or NULL
 * ignore / moving   HOST class lists, any length, values 0 .. 65535 (anything else: LT_ERR_INVALID_ARG)
 * flags   LT_INGEST_MERGED: ONE cloud out[0] of capacity sum(n) (the merged cloud of `cp` / `mergemesh`); otherwise one
 *         cloud out[i] of capacity scans[i].n per slot (`mesh`).  Outputs: points [cap,3] f64, rem [cap] f32, label
 *         [cap] u32 -- what lt_cloud takes with is_f64 = 1.  The tail [n_kept, cap) of every cloud is filled with points at
 *         (0, 0, 0), remission 0, label 0: do_range_projection_new always removes depth-0 points (:307-309) and they sit behind
 *         every kept point, so the projection may be launched with n = cap and the host never needs n_kept.
 * n_kept  DEVICE [n_scans + 1]: kept points per slot, then their total
 * work    DEVICE scratch of LT_INGEST_WORK_INTS(sum(n), n_scans) ints, the caller's (calls in flight on several streams
 *         each bring their own)
 * Asynchronous on `stream`; the host reads nothing back. */
#define LT_INGEST_MERGED 1u
#define LT_INGEST_MAX_SCANS 16
#define LT_INGEST_LIST_ARGS 16 /* class lists up to this length travel as kernel arguments, longer ones as a bitmap in `work` */
#define LT_INGEST_WORK_INTS(n_total, n_scans) (4096 + (n_total) / 256 + (n_scans) + 1)
typedef struct lt_raw_scan {
  const float* xyzr;
  const unsigned* label;
  int n;
} lt_raw_scan;
typedef struct lt_ingest_out {
  double* points;
  float* rem;
  unsigned* label;
} lt_ingest_out;
int lt_ingest_scans_dev(int n_scans, const lt_raw_scan* scans, const double* poses, const double* back, const int* ignore,
                        int n_ignore, const int* moving, int n_moving, unsigned flags, const lt_ingest_out* out,
                        int* n_kept, int* work, void* stream);

/* ---- before the render: class-aware TSDF fusion of range images (device-resident volumes) -------- */

typedef struct lt_tsdf lt_tsdf; /* opaque: one (tsdf, weight, colour, rem) float32 record per voxel, [dim_x][dim_y][dim_z] */

#define LT_TSDF_MERGE 1u /* class-aware update, the branch the reference runs (fusion_lidar.py:177, :191-228) */
/* the reference's numpy branch of `integrate` (FUSION_GPU_MODE == 0: what it runs without pycuda, fusion_lidar.py:290-388):
 * float64 voxel projection, plain running average (float64 sum and quotient), per-channel colour average with
 * round-half-even, remissions NOT integrated.  Excludes LT_TSDF_MERGE (the numpy branch has no class-aware update). */
#define LT_TSDF_HOST_MODE 2u

/* vol_bnds = {xmin, xmax, ymin, ymax, zmin, zmax} (metres), fov in degrees.  Replaces TSDFVolume.__init__
 * (auxiliary/fusion_lidar.py:23-63): dims = ceil(extent / voxel_size), truncation = 5 voxels,
 * tsdf = 1, weight = colour = remission = 0. */
int lt_tsdf_create(lt_tsdf** vol, const double* vol_bnds, double voxel_size, double fov_up, double fov_down,
                   int device);
/* Back to the initial state (the reference builds a new TSDFVolume per output scan, laserscan.py:886-887); only the
 * voxel columns written since the last reset are re-initialised. */
int lt_tsdf_reset(lt_tsdf* vol, void* stream);
/* Integrate one spherical observation: color_im = labels folded into one float per pixel as
 * fusion_lidar.py:262-264, depth_im, rem_im -- DEVICE pointers [im_h * im_w] f32.  Replaces the pycuda kernel
 * `integrate` (fusion_lidar.py:66-229) and its launch loop (:267-287); like that kernel it ignores cam_pose. */
int lt_tsdf_integrate_dev(lt_tsdf* vol, const float* color_im, const float* depth_im, const float* rem_im,
                          int im_h, int im_w, float obs_weight, unsigned flags, void* stream);
/* `n_obs` observations in order -- the `number_of_scans` range images the reference's `mesh` adaption fuses into ONE new
 * volume, all re-projected into the primary pose (laserscan.py:874-897).  Same result, bit for bit, as n_obs calls of
 * lt_tsdf_integrate_dev; on a volume that holds no observation yet (after lt_tsdf_reset) the class-aware update of up to 8
 * observations runs as ONE pass: every observation projects a voxel into the same pixel, so a voxel's geometry is
 * evaluated once and the updates are applied in order on its state in registers.  color_ims / depth_ims / rem_ims: HOST
 * arrays of n_obs DEVICE image pointers [im_h * im_w] f32 (colour folded as for lt_tsdf_integrate_dev). */
int lt_tsdf_integrate_multi_dev(lt_tsdf* vol, int n_obs, const float* const* color_ims, const float* const* depth_ims,
                                const float* const* rem_ims, int im_h, int im_w, float obs_weight, unsigned flags,
                                void* stream);

/* Device pointers of the volumes (TSDFVolume.get_volume, fusion_lidar.py:395-400, without the copies): the four fields of
 * voxel 0.  The volume is ONE array of (tsdf, weight, colour, remission) records, [x][y][z]: voxel v's field is
 * lt_tsdf_volume_stride() (= 4) floats x v behind the pointer.  (Four separate arrays until ABI 6; one record per voxel
 * makes an update one 16-byte access and hands marching cubes a vertex's samples and attributes in the lines it reads
 * anyway.) */
int lt_tsdf_volumes(lt_tsdf* vol, int* dims, float* origin, float** tsdf, float** weight, float** color,
                    float** rem);
int lt_tsdf_volume_stride(void);
/* Tell the volume that its fields were modified through the pointers above (the library tracks which (x, y) columns
 * its own integrate calls wrote, so that reset and marching cubes skip the untouched ones). */
int lt_tsdf_touch(lt_tsdf* vol);
int lt_tsdf_destroy(lt_tsdf* vol);

/* ---- between fusion and render: marching cubes on the device, the mesh is born in HBM -------------------------- */

typedef struct lt_mesh lt_mesh; /* opaque: an indexed triangle mesh in device memory + the extraction workspace */

int lt_mesh_create(lt_mesh** mesh, int device);
int lt_mesh_destroy(lt_mesh* mesh);

/* Extract the level-0 surface of the volume's current state into `mesh`.  Replaces TSDFVolume.get_mesh
 * (auxiliary/fusion_lidar.py:403-424): the three device-to-host volume copies of get_volume (:395-400),
 * skimage.measure.marching_cubes_lewiner on the CPU (:407), the vertex attribute look-ups (:409-423: nearest-voxel
 * colour / remission, voxel -> world coordinates, colour unfolding incl. the uint8 wrap of labels 256..259) and
 * the later upload of the mesh for the ray cast (:433-451).  The mesh is scikit-image 0.18's: Lewiner's cases with their
 * face / interior tests and centre vertices, one vertex per sign-changing lattice edge shared by the cells around it,
 * positions by its centre-of-mass rule -- the same vertices (bit for bit) and the same FACE STREAM as the reference's
 * get_mesh returns: face k has the same three vertices in the same order (golden F10 of the real scikit-image,
 * tests/test_pin_f10_f11_gpu.py).  Only the NUMBERING of the vertices is this library's (by word of 64 voxels, owner voxel,
 * edge axis; scikit-image numbers them by first use in its serial face stream).
 * The call synchronises `stream` once (the sizes of the mesh are needed on the host).  ms: NULL, or two floats that
 * receive the duration of the sign pass (the one stream over the float field) and of everything else. */
int lt_tsdf_extract_mesh_dev(lt_tsdf* vol, lt_mesh* mesh, void* stream, float* ms);

/* The same on caller-owned DEVICE fields [nx][ny][nz] f32 (z fastest); origin: HOST pointer to 3 floats. */
int lt_marching_cubes_dev(const float* tsdf, const float* color_vol, const float* rem_vol, int nx, int ny, int nz,
                          float voxel_size, const float* origin, lt_mesh* mesh, void* stream, float* ms);

/* Sizes and DEVICE pointers of the last extraction: verts [V,3] f32 (world), faces [F,3] i32, colors [V,3] i32
 * (r, g, b; the label in channel 2, as get_mesh + throw_rays_at_mesh hand it to ctrace), rem [V] f32.  The
 * pointers stay valid until the next extraction into this mesh or lt_mesh_destroy.  Any argument may be NULL. */
int lt_mesh_get(lt_mesh* mesh, int* n_verts, int* n_faces, float** verts, int** faces, int** colors, float** rem);

/* Number the vertices of the last extraction as scikit-image numbers them -- by first use in the face stream -- and rewrite
 * the face array accordingly: verts / colors / rem / faces then EQUAL the arrays the reference's get_mesh returns (golden
 * F10), not only up to the vertices' numbers.  For host-facing consumers of the arrays (TSDFVolume.get_mesh); the ray cast
 * does not care.  Call it BEFORE lt_scene_set_mesh / lt_mesh_get: the vertex arrays move to other buffers.  Synchronises
 * `stream`. */
int lt_mesh_renumber_dev(lt_mesh* mesh, void* stream);

/* lt_scene_set_mesh_dev with the arrays of `mesh` (borrowed until the next extraction): the render reads the
 * mesh where marching cubes wrote it -- no PCIe traffic between fusion and range image. */
int lt_scene_set_mesh(lt_scene* scene, lt_mesh* mesh);

/* One OUTPUT SCAN of the reference's `mesh` adaption in one call, nothing leaving HBM: a fresh volume (lt_tsdf_reset) <-
 * n_obs observations (lt_tsdf_integrate_dev each; color_ims / depth_ims / rem_ims are HOST arrays of n_obs DEVICE
 * pointers, images [im_h * im_w] f32) -> marching cubes into `mesh` -> lt_scene_set_mesh -> lt_scene_render_dev of
 * `rayset` from `origin` (HOST, 3 floats) into the DEVICE output images (any may be NULL), and -- with sync != 0 -- a wait
 * for `stream`.  Replaces the body of MultiSemLaserScan.deform's mesh branch per output scan (auxiliary/laserscan.py:
 * 874-914: TSDFVolume(...) :886, integrate per scan :896-899, throw_rays_at_mesh :907 = get_mesh + C_Trace).  One call
 * per scan is what lets several scans be in flight from several host threads of a Python caller (the interpreter lock is
 * released for the whole chain): lidar_transfer_amd.pipeline.FusionScanPipeline.  Returns the first error of the chain. */
int lt_fusion_scan_dev(lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene, lt_rayset* rayset, int n_obs,
                       const float* const* color_ims, const float* const* depth_ims, const float* const* rem_ims,
                       int im_h, int im_w, float obs_weight, unsigned tsdf_flags, const float* origin,
                       float* endpoints, int* endcolors, float* range, float* endrem, int* tri, unsigned trace_flags,
                       void* stream, int sync);

/* The same from the POINT CLOUDS of the source scans (MultiSemLaserScan.deform's mesh branch, laserscan.py:874-914, in one
 * call): do_range_projection_new(fov, remove=True) + do_label_projection_new per cloud (lt_range_projection_batch_dev, into
 * images the projector owns) -> lt_fusion_scan_dev.  fov_up / fov_down (degrees) and H x W are the SOURCE sensor's, i.e. the
 * volume's; clouds / is_f64 / beam_angles as for lt_range_projection_batch_dev; the rest as for lt_fusion_scan_dev.  At most
 * 64 clouds. */
int lt_deform_scan_dev(lt_projector* projector, lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene, lt_rayset* rayset,
                       int n_clouds, const lt_cloud* clouds, int is_f64, double fov_up, double fov_down, int H, int W,
                       const double* beam_angles, int n_beams, float obs_weight, unsigned tsdf_flags, const float* origin,
                       float* endpoints, int* endcolors, float* range, float* endrem, int* tri, unsigned trace_flags,
                       void* stream, int sync);

/* ---- deform('mergemesh'): the volume geometry as device-resident state ---------------------------------------------
 *
 * The reference's default adaption clips ONE voxel_bounds array output scan after output scan (auxiliary/laserscan.py:957-962
 * on the array lidar_deform.py:321 hands every MultiSemLaserScan; auxiliary/fusion_lidar.py:33-37 then re-derives its upper
 * bounds): a scan's volume depends on every earlier scan of the SEQUENCE.  lt_mm_state holds that array in HBM;
 * lt_mm_geometry_dev applies the five numpy statements to it in stream order, from the kept points' bounds the projection
 * left on the device (lt_proj_images.bnds), and mirrors the outcome into a pinned host record behind an event -- no
 * stream synchronisation between projection and fusion.  lt_mm_geometry_get waits for that event only (passed already
 * when the caller has read the chain's mesh sizes) and returns the record. */
typedef struct lt_mm_state lt_mm_state;
typedef struct lt_mm_geometry {
  double bnds_given[6]; /* the bounds after the clip (:961-962): what TSDFVolume(vol_bnds, ...) is constructed from */
  double bnds_after[6]; /* ... after fusion_lidar.py:36: what the reference leaves in the caller's array            */
  int dim[3];           /* ceil((max - min) / voxel_size), fusion_lidar.py:34                                         */
  int status;           /* 0 ok; 1 no point survived the projection (state untouched; numpy raises in amin);          */
                        /* 2 the clipped volume is empty (state holds the clip; the reference dies in np.ones)        */
  int ticket;           /* the call's ordinal on its state (set by lt_mm_geometry_get): later calls hold later state  */
  int reserved;
} lt_mm_geometry;
/* vol_bnds = {xmin, xmax, ymin, ymax, zmin, zmax}; bounds_are_int: the caller's array has an integer dtype (the YAML's
 * ints: fusion_lidar.py:36 then truncates). */
int lt_mm_state_create(lt_mm_state** state, const double* vol_bnds, int bounds_are_int, double voxel_size, int device);
int lt_mm_state_destroy(lt_mm_state* state);
/* New bounds for a new sequence (the reference starts one process per sequence, experiments/run_lidar_deform.sh). */
int lt_mm_state_reset(lt_mm_state* state, const double* vol_bnds, void* stream);
/* point_bnds: DEVICE [6] as lt_proj_images.bnds.  *ticket names the record.  The kernels of successive calls on one state
 * run in the order of the calls, whatever their streams (each waits for the previous call's event).  seq >= 0: the call is
 * scan `seq` of its sequence (numbered from 0 since create / reset) and waits on the HOST until scans 0 .. seq - 1 have made
 * theirs -- several chains (threads, streams) of one sequence; seq < 0: the caller keeps the order itself.  point_bnds ==
 * NULL with seq >= 0: the scan gives up its turn (it failed before its projection); *ticket = -1. */
int lt_mm_geometry_dev(lt_mm_state* state, const double* point_bnds, int seq, int* ticket, void* stream);
int lt_mm_geometry_get(lt_mm_state* state, int ticket, lt_mm_geometry* out);

/* deform('mergemesh') of ONE output scan in ONE call (auxiliary/laserscan.py:921-1012; the interpreter lock of a Python
 * caller is released for all of it): `cloud` -- the merged source scans -- through do_range_projection_new(fov, remove=True)
 * into images the projector owns (fov_up / fov_down: the TARGET's, H x W: the SOURCE's, laserscan.py:929-931, :952-954) ->
 * lt_mm_geometry_dev(mm, seq) on the kept points' bounds -> with `vol` != NULL (the volume of the geometry the caller
 * EXPECTS, i.e. the previous scan's): lt_fusion_scan_dev on it, then lt_mm_geometry_get -> *geo; *done = 1 when vol was
 * built from exactly geo->bnds_given (the images are this scan's), else 0: the caller makes the volume of geo->bnds_given
 * and calls lt_mergemesh_rerun_dev, which runs the chain on the images the projector still holds.  With vol == NULL the
 * call waits for the record and returns *done = 0.  geo->status != 0: *done = 0, nothing else to do. */
int lt_mergemesh_scan_dev(lt_projector* projector, lt_mm_state* mm, int seq, lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene,
                          lt_rayset* rayset, const lt_cloud* cloud, int is_f64, double fov_up, double fov_down, int H, int W,
                          const double* beam_angles, int n_beams, float obs_weight, unsigned tsdf_flags, const float* origin,
                          float* endpoints, int* endcolors, float* range, float* endrem, int* tri, unsigned trace_flags,
                          void* stream, lt_mm_geometry* geo, int* done);
int lt_mergemesh_rerun_dev(lt_projector* projector, lt_tsdf* vol, lt_mesh* mesh, lt_scene* scene, lt_rayset* rayset, int H, int W,
                           float obs_weight, unsigned tsdf_flags, const float* origin, float* endpoints, int* endcolors,
                           float* range, float* endrem, int* tri, unsigned trace_flags, void* stream);

/* ---- after the render: back-projection, scan packing, comparison ------------------------------- */

/* xyz of every cell from its range and pixel coordinates; replaces LaserScan.do_reverse_projection_new
 * (auxiliary/laserscan.py:475-501).  range_img [H*W] f32, proj_x / proj_y [H*W] int32 (or float64 when
 * coords_are_f64: the `preserve_float` branch), back_points [H*W,3] f64 -- all DEVICE pointers. */
int lt_reverse_projection_dev(const float* range_img, const void* proj_x, const void* proj_y,
                              int coords_are_f64, double fov_up, double fov_down, int H, int W,
                              double* back_points, void* stream);

/* The same for a sensor with a BEAM TABLE (what LT_PROJ_BEAM_ROWS projected): yaw = (proj_x / W * 2 - 1) * pi as above;
 * the elevation e = Brad[proj_y] (proj_x / proj_y int32; Brad: DEVICE [H] float64, the table in radians) or -- with
 * preserve_float -- the pitch image itself (proj_x and the pitch float64; Brad may be NULL); pitch = pi/2 - e; the point is
 * depth * sin(pitch) * cos(-yaw), depth * sin(pitch) * sin(-yaw), depth * cos(pitch), multiplied left to right in
 * float64.  One thread per cell, asynchronous on `stream`. */
int lt_reverse_projection_beams_dev(const float* range_img, const void* proj_x, const void* proj_y_or_pitch,
                                    int preserve_float, const double* Brad, int H, int W, double* back_points, void* stream);

/* The same for a sensor with a horizontal SECTOR (what LT_PROJ_SECTOR projected): yaw = yaw_center + ((proj_x + 0.5) / W -
 * 0.5) * span from the int32 column -- the centre of its cell, the direction of its ray -- or, with preserve_float, yaw =
 * yaw_center + (proj_xf / W - 0.5) * span from the float64 column (yaw_center = -center / 180 * pi and span in radians, as
 * the flag takes them).  The elevation: beam_rows == 0 -- lt_reverse_projection_dev's linear rule from proj_y (int32, or
 * float64 with preserve_float), Brad unused; beam_rows != 0 -- lt_reverse_projection_beams_dev's, Brad[proj_y] or the pitch
 * image.  The point is depth * sin(pitch) * cos(-yaw), ..., multiplied left to right in float64.  Asynchronous. */
int lt_reverse_projection_sector_dev(const float* range_img, const void* proj_x, const void* proj_y_or_pitch,
                                     int preserve_float, int beam_rows, const double* Brad, double fov_up, double fov_down,
                                     int H, int W, double yaw_center, double span, double* back_points, void* stream);

/* The same for a sensor with a beam table whose beams carry AZIMUTH OFFSETS (what LT_PROJ_BEAM_AZIMUTH projected): the yaw
 * of lt_reverse_projection_beams_dev or -- `sector` (HOST [2]: yaw_center, span in radians; NULL = the full circle) -- of
 * lt_reverse_projection_sector_dev is the NOMINAL one, and yaw = nominal - az_rad[row] (az_rad: DEVICE [H] float64, radians)
 * in float64.  The row is proj_y clamped to [0, H - 1] like the Brad read (int32 coordinates), or the cell's own row i / W
 * with preserve_float, where the second image holds the pitch.  The elevation is lt_reverse_projection_beams_dev's (Brad:
 * DEVICE [H]; may be NULL with preserve_float).  Asynchronous on `stream`. */
int lt_reverse_projection_beams_az_dev(const float* range_img, const void* proj_x, const void* proj_y_or_pitch,
                                       int preserve_float, const double* Brad, const double* az_rad, const double* sector,
                                       int H, int W, double* back_points, void* stream);

/* Points into another frame: out[i] = float32(((m0*x + m1*y) + m2*z) + m3) per row of T, in float64 from the float32
 * point.  points / out [n,3] f32 DEVICE (out may be points), tri [n] i32 DEVICE or NULL: rows with tri < 0 (rays
 * that missed) are copied unchanged.  T: HOST [16] row-major (read before the call returns; the last row is not
 * used).  Asynchronous on `stream`. */
int lt_points_to_frame_dev(const float* points, const int* tri, int n, const double* T, float* out, void* stream);

/* ---- the target sensor's return model (the reference writes every hit) ------------------------
 *
 * Applied to a rendered scan cell by cell, in place.  Per cell i: tri[i], range[i], endrem[i]; the ray d = rays[i]; for a
 * hit the float32 vertices v0, v1, v2 of face tri[i] of the scene's CURRENT mesh.  In float64 from the widened float32
 * values, every product and sum rounded on its own, in this order:
 *   e1 = v1 - v0;  e2 = v2 - v0;  n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x)
 *   dot = (nx*dx + ny*dy) + nz*dz;  nn = (nx*nx + ny*ny) + nz*nz;  dd = (dx*dx + dy*dy) + dz*dz
 *   q = |dot| / sqrt(nn * dd);  c = (nn == 0 || dd == 0) ? 0 : (q < 1 ? q : 1)        the cosine of the incidence angle
 * The cell's code is the FIRST rule that applies (all comparisons strict: a cell exactly at a threshold stays):
 *   1  tri[i] < 0 (no hit)       2  (double)range[i] < min_range      3  (double)range[i] > max_range
 *   4  c < min_cos               5  hash(seed, scan, i) < drop_threshold                0  the return stands
 * with  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32, wrapping) and
 * hash(seed, scan, i) = mix(mix(mix(seed) + scan) + i): a pure function of the three, so a scan's pattern does not depend
 * on the chain, rank or order it is rendered in.  `scan`: the output scan's index in its sequence (its file's number).
 * A cell with code 2 - 5 becomes the miss LT_TRACE_WRITE_MISSES writes: end point (0, 0, 0), label / colour 0, remission 0,
 * range 0, tri -1.  Code 0 keeps everything; with LT_RETURN_LAMBERT endrem[i] = float32((double)endrem[i] * c).  Code 1 is
 * left as it is.  incidence[i] = float32(c) for code 0, else -1; drop[i] = the code.  No counters: totals are a bincount.
 * min_cos = cos(max_incidence) and drop_threshold = floor(drop_rate * 2^32) are the HOST's: the kernel has no transcendental. */
typedef struct lt_return_model {
  double min_range, max_range; /* metres; 0 <= min_range <= max_range (+inf: no far gate)                              */
  double min_cos;              /* in [0, 1]; 0 never drops                                                             */
  unsigned drop_threshold;     /* 0 never drops                                                                        */
  unsigned seed;
  unsigned flags;              /* LT_RETURN_LAMBERT or 0                                                               */
} lt_return_model;
#define LT_RETURN_LAMBERT 1u

/* rays [n_rays,3] f32 DEVICE: the tensor the ray set was built from (posed, if the sensor is mounted).  model: HOST, read
 * before the call returns.  tri [n] i32 and range [n] f32 are mandatory; endpoints [n,3] f32, endcolors ([n] i32 with
 * trace_flags & LT_TRACE_LABEL_IMAGE, else [n,3] i32), endrem [n] f32, incidence [n] f32 and drop [n] u8 may each be NULL --
 * all DEVICE, read-modify-write.  A tri value outside [-1, n_faces), or a face whose vertices are outside [0, n_verts),
 * sets the scene's deferred LT_ERR_BAD_INDEX (lt_scene_status); such a cell gets code 1 and nothing beside the mesh is
 * read.  One thread per cell, asynchronous on `stream`. */
int lt_return_model_dev(lt_scene* scene, const float* rays, int n_rays, const lt_return_model* model, unsigned scan,
                        float* endpoints, int* endcolors, float* range, float* endrem, int* tri, float* incidence,
                        unsigned char* drop, unsigned trace_flags, void* stream);

/* ---- the target sensor's noise model (the reference leaves it as a TODO, laserscan.py:1094-1096) ---
 *
 * Applied to a rendered scan cell by cell, in place, behind the return model.  Cell i is a RETURN when tri[i] >= 0 and
 * range[i] > 0; any other cell is left untouched, byte for byte.  With mix(x) as above (uint32, products and sums wrap):
 *   g   = mix(mix(mix(seed ^ 0x6e6f6973) + scan) + i)          a stream of its own: independent of the dropout hash
 *   w_k = mix(g + k)                                           k = 1..6: the range draw;  k = 7..12: the remission draw
 *   S   = the sum over the draw's six words of (w_k & 0xffff) + (w_k >> 16)            twelve 16-bit uniforms, an integer
 *   z   = (double)(S - 393210) / 65536.0                       mean 0, variance 1 - 2^-32, |z| < 6, exact in float64
 * a pure function of (seed, scan, i), so a scan's pattern does not depend on the chain, rank or order it is rendered in.
 * In float64 from the widened float32 values, every product, sum and quotient rounded on its own, in this order:
 *   r  = (double)range[i]
 *   r1 = r + (range_sigma + range_sigma_rel * r) * z_range
 *   r2 = range_resolution > 0 ? rint(r1 / range_resolution) * range_resolution : r1            rint: ties to even
 * State 2, the return is LOST, if !(r2 > 0) or r2 < min_range or r2 > max_range (strict: a cell exactly at the gate stays):
 * the cell becomes the miss LT_TRACE_WRITE_MISSES writes -- end point (0, 0, 0), label / colour 0, remission 0, range 0,
 * tri -1.  Else state 1, the return is NOISED:
 *   range[i] = float32(r2);   s = r2 / r
 *   endpoints[i][k] = float32(o[k] + ((double)endpoints[i][k] - o[k]) * s)      o = (double)origin, k = x, y, z
 *   e = (double)endrem[i] + remission_sigma * z_rem;   e = e < 0 ? 0 : (e > 1 ? 1 : e)
 *   e = remission_levels ? rint(e * (L - 1)) / (L - 1) : e                      L = remission_levels as a double
 *   endrem[i] = float32(e)
 * State 0 is a cell left untouched.  range_error[i] = float32(r2 - r) for state 1, else 0; state[i] = the state.  Both are
 * written for EVERY cell.  No counters and no atomics: totals are a bincount.  The kernel has no transcendental. */
typedef struct lt_noise_model {
  double range_sigma;      /* metres, finite, >= 0: the constant part of the range jitter's standard deviation        */
  double range_sigma_rel;  /* finite, >= 0: the part proportional to the range (metres per metre)                     */
  double range_resolution; /* metres, finite, >= 0; 0: ranges are not put on a grid                                   */
  double remission_sigma;  /* finite, >= 0 (remission is in [0, 1])                                                   */
  double min_range, max_range; /* the sensor's range gate (its return model's; 0 and +inf: none), 0 <= min <= max     */
  unsigned remission_levels;   /* 0: off, else >= 2: remission is reported on this many levels                        */
  unsigned seed;
} lt_noise_model;

/* origin [3] f32 HOST: where the scan's rays start (the target sensor's position in the scene), finite.  model: HOST; both
 * are read before the call returns.  tri [n] i32 and range [n] f32 are mandatory; endpoints [n,3] f32, endcolors ([n] i32
 * with trace_flags & LT_TRACE_LABEL_IMAGE, else [n,3] i32), endrem [n] f32, range_error [n] f32 and state [n] u8 may each
 * be NULL -- all DEVICE; the five images are read-modify-write, so the call is made ONCE per rendered scan.  No scene: no
 * mesh is read.  One thread per cell, one launch, asynchronous on `stream`, on the calling thread's current device (the
 * buffers' and the stream's).  n == 0 is LT_OK; a bad argument is LT_ERR_INVALID_ARG with a message. */
int lt_noise_model_dev(const float* origin, int n, const lt_noise_model* model, unsigned scan, float* endpoints,
                       int* endcolors, float* range, float* endrem, int* tri, float* range_error, unsigned char* state,
                       unsigned trace_flags, void* stream);

/* ---- the target sensor's echo model: a beam with a divergence (the reference has none) -----------
 *
 * A beam illuminates a cone, not a line.  Each cell is rendered with S = n_subrays SUB-RAYS -- the central ray and S - 1 on
 * a ring around it -- into S sub-images, and one kernel resolves them into the cell: the sub-hits are grouped into echoes
 * along the range, one echo is reported.  Sub-rays and sub-images are laid out PLANE BY PLANE: sub-ray k of cell i is
 * element k * n + i, so plane 0 is a whole image.
 *
 * lt_create_subrays_dev, per cell, in float64 from the widened float32 d = rays[i] = (x, y, z); every product, sum,
 * quotient and square root rounded on its own (no fused multiply-add, IEEE sqrt and /):
 *   h2 = x*x + y*y;  dd = h2 + z*z
 *   if !(dd > 0) or dd is not finite: every sub-ray of the cell is d, copied
 *   n = sqrt(dd);  hx = x/n, hy = y/n, hz = z/n
 *   h2 > 0 ? (h = sqrt(h2); ux = -y/h; uy = x/h) : (ux = 1; uy = 0)       u: horizontal, to the LEFT (larger atan2(y, x))
 *   vx = -(hz*uy);  vy = hz*ux;  vz = hx*uy - hy*ux                        v = h x u: upwards for a level ray
 *   (a, b) = (off[2k], off[2k+1]);  (a, b) == (0, 0): the three floats of d, COPIED
 *   else subrays[k*n + i] = float32( (hx + a*ux) + b*vx,  (hy + a*uy) + b*vy,  hz + b*vz )      not normalised
 *
 * lt_echo_resolve_dev, per cell i:
 *   1. sub-ray k is a HIT when sub_tri[k*n+i] >= 0 and sub_range[k*n+i] > 0;
 *   2. the hits are ordered by (t, k) ascending, t the float32 range;
 *   3. walked in that order, the first hit opens an echo, and a hit with (double)t - (double)t_first > separation (strict;
 *      t_first: the open echo's first member) opens the next;
 *   4. an echo keeps its count c, St and Srem -- float64 sums of the widened float32 values, in walk order, starting from
 *      the first member's value -- and its representative rep, the member with the smallest k;
 *   5. an echo is DETECTED when c >= min_subrays; n_echoes[i] = the number of detected echoes;
 *   6. LT_ECHO_FIRST takes the earliest detected echo in walk order, LT_ECHO_LAST the latest, LT_ECHO_STRONGEST the one
 *      with the largest Srem, a tie going to the larger c and a remaining tie to the earlier;
 *   7. range[i] = float32(St / c);  endrem[i] = float32(Srem / S);  fraction[i] = float32((double)c / S);
 *      endcolors[i] = sub_label[rep*n+i];  tri[i] = sub_tri[rep*n+i];
 *      endpoints[i][j] = float32(o[j] + h[j] * (double)range[i])          h: the unit direction above of rays[i], o = origin
 * A cell without a detected echo, or whose central ray has !(dd > 0), becomes the miss LT_TRACE_WRITE_MISSES writes: end
 * point (0, 0, 0), label 0, remission 0, range 0, tri -1, fraction 0 (n_echoes stays the count).  Every output is written
 * for every cell.  A spot wholly on a surface of one remission keeps that remission bit for bit: (S*x)/S is exact, S <= 8.
 * No transcendental on the device: the offsets are made on the host (config.EchoModel.offsets). */
#define LT_ECHO_MAX_SUBRAYS 8
#define LT_ECHO_FIRST 0u
#define LT_ECHO_STRONGEST 1u
#define LT_ECHO_LAST 2u
typedef struct lt_echo_model {
  double off[2 * LT_ECHO_MAX_SUBRAYS]; /* (a_k, b_k), k < n_subrays, finite; the rest is ignored                       */
  double separation;                   /* metres, finite, > 0                                                         */
  int n_subrays;                       /* 2 .. LT_ECHO_MAX_SUBRAYS                                                    */
  int min_subrays;                     /* 1 .. n_subrays: an echo of fewer sub-hits is not detected                   */
  unsigned mode;                       /* LT_ECHO_FIRST | LT_ECHO_STRONGEST | LT_ECHO_LAST                            */
  unsigned reserved;
} lt_echo_model;

/* rays [n,3] f32 DEVICE -> subrays [n_subrays * n, 3] f32 DEVICE, plane by plane.  model: HOST, read before the call
 * returns.  One launch, asynchronous on `stream`, on the calling thread's current device.  n == 0 is LT_OK; a NULL
 * pointer, n < 0 (or n_subrays * n past INT_MAX) and a model outside the ranges above are LT_ERR_INVALID_ARG. */
int lt_create_subrays_dev(const float* rays, int n, const lt_echo_model* model, float* subrays, void* stream);

/* rays [n,3] f32 (the CENTRAL rays), sub_range [S*n] f32, sub_label [S*n] i32 (label-image layout only), sub_rem [S*n]
 * f32, sub_tri [S*n] i32 in; endpoints [n,3] f32, endcolors [n] i32, range [n] f32, endrem [n] f32, tri [n] i32, n_echoes
 * [n] u8, fraction [n] f32 out -- all DEVICE, none of the outputs overlapping an input.  rays, sub_range, sub_tri, range
 * and tri are mandatory; every other output may be NULL, and so may sub_label (reads as label 0) and sub_rem (remission 0).
 * origin [3] f32 and model: HOST, read before the call returns.  One thread per cell, one launch, asynchronous on `stream`,
 * on the calling thread's current device.  n == 0 is LT_OK; a bad argument is LT_ERR_INVALID_ARG with a message. */
int lt_echo_resolve_dev(const float* rays, const float* origin, int n, const lt_echo_model* model,
                        const float* sub_range, const int* sub_label, const float* sub_rem, const int* sub_tri,
                        float* endpoints, int* endcolors, float* range, float* endrem, int* tri,
                        unsigned char* n_echoes, float* fraction, void* stream);

/* The DUAL-RETURN resolve: lt_echo_resolve_dev's cell, plus a SECOND echo of it.  Steps 1 - 7 above are unchanged and give the
 * detected echoes D_0 .. D_{m-1} in walk order, the primary P chosen by model->mode, and the primary set of outputs, bit
 * for bit what lt_echo_resolve_dev writes.  Then:
 *   8. the SECOND echo is chosen by second_mode among the detected echoes OTHER THAN P: LT_ECHO_FIRST the earliest of the
 *      rest in walk order, LT_ECHO_LAST the latest of the rest, LT_ECHO_STRONGEST the one of the rest with the largest Srem,
 *      a tie going to the larger c and a remaining tie to the earlier; with m < 2 there is no second echo;
 *   9. its outputs are step 7's expressions on its own c, St, Srem and rep:  range2[i] = float32(St / c);  endrem2[i] =
 *      float32(Srem / S);  fraction2[i] = float32((double)c / S);  endcolors2[i] = sub_label[rep*n+i];  tri2[i] =
 *      sub_tri[rep*n+i];  endpoints2[i][j] = float32(o[j] + h[j] * (double)range2[i]) -- on the CENTRAL ray.
 * A cell without a second echo, or whose central ray has !(dd > 0), gets the miss LT_TRACE_WRITE_MISSES writes in the second
 * set (end point (0, 0, 0), label 0, remission 0, range 0, tri -1) and fraction2 = 0.  Every output of both sets is written
 * for every cell.  ONE rule, not a sensor's: with mode = strongest and second_mode = last a cell whose strongest echo is
 * also its last gets the latest of the OTHER echoes, where a Velodyne head would report the second strongest.
 * The arguments are lt_echo_resolve_dev's, with second_mode behind the model and the second set behind the first: endpoints2
 * [n,3] f32, endcolors2 [n] i32, range2 [n] f32, endrem2 [n] f32, tri2 [n] i32, fraction2 [n] f32 -- DEVICE, overlapping
 * neither an input nor another output.  range2 and tri2 are mandatory, the others may be NULL.  Everything else is
 * lt_echo_resolve_dev's rule: one thread per cell, one launch, asynchronous on `stream`; n == 0 is LT_OK; a bad argument,
 * a second_mode that is none of the three included, is LT_ERR_INVALID_ARG with a message. */
int lt_echo_resolve_dual_dev(const float* rays, const float* origin, int n, const lt_echo_model* model, unsigned second_mode,
                             const float* sub_range, const int* sub_label, const float* sub_rem, const int* sub_tri,
                             float* endpoints, int* endcolors, float* range, float* endrem, int* tri,
                             unsigned char* n_echoes, float* fraction, float* endpoints2, int* endcolors2, float* range2,
                             float* endrem2, int* tri2, float* fraction2, void* stream);

/* Pack a rendered scan in SemanticKITTI layout; replaces the filtering and the per-point struct.pack loops
 * of MultiSemLaserScan.write (auxiliary/laserscan.py:1133-1178).  Keeps, in order, the cells with
 * (index == NULL or index[i] > 0) and label[i] >= 0 and x + y + z != 0.  points [n,3] f32 or f64,
 * rem [n] f32, label [n] i32, out_bin [n,4] f32 (x, y, z, remission), out_label [n] u32 -- DEVICE
 * pointers; *n_out (HOST) = number of points written (the call synchronises `stream`). */
int lt_pack_scan_dev(const void* points, int is_f64, const float* rem, const int* label, const int* index, int n,
                     float* out_bin, unsigned* out_label, int* n_out, void* stream);

/* Masked comparison of a source and a target image; replaces the array part of compare()
 * (auxiliary/laserscan.py:1181-1301) and iouEval.addBatch (auxiliary/np_ioueval.py:31-47): cells whose
 * source colour is black or whose source label is 0 are background in both images;
 * conf[target * n_labels + source] counts raw label pairs (u64, n_labels^2); range_diff / rem_diff are the
 * squared differences [n] (may be NULL); src_masked / tgt_masked the masked label images (may be NULL);
 * *sq_sum (DEVICE double) = sum of range_diff (MSE = sq_sum / n).  All DEVICE pointers, asynchronous. */
int lt_compare_dev(const int* src_label, const float* src_color, const int* tgt_label, const float* src_range,
                   const float* tgt_range, const float* src_rem, const float* tgt_rem, int n, int n_labels,
                   unsigned long long* conf, float* range_diff, float* rem_diff, int* src_masked, int* tgt_masked,
                   double* sq_sum, void* stream);

/* ---- evaluation on the device: the source reference scan and compare() into a small record -------------------------
 *
 * What lidar_deform.py does around `deform` per output scan when source and target image sizes agree (:396-409, :416-418):
 * a SemLaserScan of the primary scan alone, and compare(scan, scans).  lt_evaluator owns the workspaces of both calls (z-min
 * keys of the source image, an n_labels x n_labels pair-count matrix that is never copied, per-workgroup partial sums); one
 * per caller thread / HIP stream: calls on one evaluator are serialised and must be queued in stream order.  n_labels: a
 * multiple of 256, at most LT_COMPARE_MAX_NLABELS (512 covers SemanticKITTI's labels up to 259). */
typedef struct lt_evaluator lt_evaluator;
#define LT_COMPARE_MAX_NLABELS 2048
#define LT_COMPARE_MAX_PRESENT 64 /* label values one record can hold */
#define LT_COMPARE_OVERFLOW 1     /* lt_compare_record.status: more than LT_COMPARE_MAX_PRESENT values present        */
#define LT_COMPARE_LABEL_RANGE 2  /* ... a masked label outside 0 .. n_labels - 1 (negative ones included)            */
int lt_evaluator_create(lt_evaluator** ev, int n_labels, int device);
int lt_evaluator_destroy(lt_evaluator* ev);

/* [H*W] DEVICE images of the source reference scan; every member may be NULL. */
typedef struct lt_source_images {
  float* range;         /* proj_range, empty cells -1 (laserscan.py:37-39)                                            */
  float* rem;           /* proj_remissions, empty cells -1                                                            */
  int* label;           /* proj_label, empty cells 0                                                                  */
  unsigned char* black; /* 1 where np.sum(proj_color, axis=2) == 0 (laserscan.py:1200): empty cells and black classes */
  unsigned* bad_labels; /* ONE word: raw points whose label & 0xFFFF is outside the LUT (colorize() raises IndexError,  */
                        /* laserscan.py:642); such a cell, if one wins, is black                                      */
} lt_source_images;

/* lt_source_scan_dev -- from ONE resident raw scan (the bytes of velodyne/N.bin + labels/N.label, as lt_ingest_scans_dev
 * takes them) to the source reference image of lidar_deform.py:403-409.  Per raw point, in file order:
 *   1. l = label & 0xFFFF (laserscan.py:588); l >= lut_len is counted into bad_labels (colorize runs before the removal)
 *   2. dropped if l in ignore (remove_classes, :658-670; no `moving` list: the source scan is a primary scan)
 *   3. x, y, z stay float32 and untransformed; do_range_projection(fov_up, fov_down, remove=True) in float32 (:202-292) --
 *      the arithmetic of lt_range_projection_dev for float32 clouds with LT_PROJ_REMOVE, no beam angles (lidar_deform.py:396
 *      constructs the scan without them): depth 0 and proj_y outside [0, 1] are dropped
 *   4. winner per cell: the nearest point, the lowest index among equal depths.  A dropped point does not bid, and because
 *      the removals keep the file order the raw index orders the kept points exactly as the kept index does
 *   5. the cell receives the winner's float32 depth, xyzr[3], l, and black = (sum(color_lut[l]) == 0); empty: -1, -1, 0, 1
 * ignore: HOST list, any length, values 0 .. 65535 (up to LT_INGEST_LIST_ARGS as kernel arguments, longer ones as a bitmap);
 * color_lut: DEVICE [lut_len,3] f32 (SemLaserScan.color_lut).  Asynchronous on `stream`; the host reads nothing back. */
int lt_source_scan_dev(lt_evaluator* ev, const lt_raw_scan* scan, const int* ignore, int n_ignore, double fov_up,
                       double fov_down, int H, int W, const float* color_lut, int lut_len, const lt_source_images* out,
                       void* stream);

/* The TARGET sensor's model as lt_target_view_dev reads it (HOST).  The arrays are what lt_range_projection_batch_dev takes
 * for the same flags: `rows` is its beam_angles under LT_PROJ_BEAM_ROWS, `az_rad` what lt_projector_set_beam_azimuth takes,
 * yaw_center / span what lt_projector_set_sector takes, with the same ranges (1 <= H <= 511 with a table, |az| <= pi / 2,
 * |yaw_center| <= pi, 0 < span < 2 pi). */
typedef struct lt_view_model {
  double fov_up, fov_down;  /* degrees, the TARGET's                                                     */
  int H, W;                 /* the TARGET's image                                                         */
  unsigned flags;           /* 0 or a valid combination of LT_PROJ_BEAM_ROWS | LT_PROJ_SECTOR |          */
                            /* LT_PROJ_BEAM_AZIMUTH (LT_PROJ_NEW | LT_PROJ_REMOVE are implied)            */
  const double* rows;       /* HOST: Brad[H] then halfw[H] with LT_PROJ_BEAM_ROWS, else NULL              */
  const double* az_rad;     /* HOST [H] with LT_PROJ_BEAM_AZIMUTH, else NULL                              */
  double yaw_center, span;  /* radians, with LT_PROJ_SECTOR                                               */
} lt_view_model;

/* lt_target_view_dev -- the TARGET VIEW of one resident raw scan: the primary source scan seen through the target sensor's
 * model from the target's pose, i.e. what `cp` with number_of_scans: 1 and no `moving` list puts into the target image
 * (lt_ingest_scans_dev of the one scan with poses[0] = T and back = NULL, then lt_range_projection_batch_dev under the
 * model's flags | LT_PROJ_NEW | LT_PROJ_REMOVE without beam angles), made in one pass from the file bytes, in the shape
 * lt_compare_record_dev consumes.  On the same lt_evaluator as lt_source_scan_dev (one key workspace, calls in stream
 * order).  Per raw point i, in file order:
 *   1. l = label & 0xFFFF; l >= lut_len is counted into bad_labels
 *   2. dropped if l in ignore (the list-or-bitmap rule of lt_source_scan_dev)
 *   3. x, y, z are widened from float32 to float64.  With T: every row as ((m0*x + m1*y) + m2*z) + m3, products and sums
 *      rounded on their own (step 5 of lt_ingest_scans_dev); the last row of T is not read.  T == NULL: the widened values
 *      themselves, not a product with the identity (a -0.0 keeps its sign)
 *   4. the float64 projection of the model's flags with both drops (depth 0, NaN; outside the rows' keep rule; outside the
 *      sector).  Linear rows have NO hard-coded beam angles, as the source reference scan has none (lidar_deform.py:396);
 *      pi, |fov_down| and fov in radians as lt_range_projection_batch_dev derives them for float64 clouds.  A dropped point
 *      does not bid
 *   5. winner per cell: do_range_projection_new's (laserscan.py:366, :376) -- the first point of the minimum's float32
 *      bucket unless points of that bucket lie below the float32 value, then the last of those.  The raw index stands for
 *      the kept index because the removals keep the file order
 *   6. the cell receives the winner's float32 depth, xyzr[3], l, and black = (sum(color_lut[l]) == 0); empty: -1, -1, 0, 1
 * T: HOST [16] row-major, x_target = T x_source, or NULL.  The model's doubles live in a device buffer of the evaluator and
 * are uploaded, in stream order, only when they differ from the previous call's: the per-scan calls of a sequence copy
 * nothing and wait for nothing.  LT_ERR_INVALID_ARG before any device work: NULL handles, n > 0 without buffers, xyzr not
 * 16-byte aligned, a class outside 0 .. 65535, H or W <= 0 or H * W beyond the key range, flags that do not combine
 * (LT_PROJ_BEAM_AZIMUTH without LT_PROJ_BEAM_ROWS), a flag without its array, values outside the ranges above.
 * ignore, color_lut, out: as lt_source_scan_dev.  Asynchronous on `stream`; the host reads nothing back. */
int lt_target_view_dev(lt_evaluator* ev, const lt_raw_scan* scan, const int* ignore, int n_ignore,
                       const double* T /* HOST [16] row-major, x_target = T x_source; NULL: none */,
                       const lt_view_model* model, const float* color_lut, int lut_len, const lt_source_images* out,
                       void* stream);

/* What compare() + iouEval.addBatch leave of one output scan, compacted on the device. */
typedef struct lt_compare_record {
  int status;              /* 0, LT_COMPARE_OVERFLOW or LT_COMPARE_LABEL_RANGE: then only sq_sum / n_cells are meaningful */
  int n_present;           /* P: label values present in either masked image                                             */
  int n_cells;
  unsigned src_bad_labels; /* *src_bad_labels of the call (lt_source_images.bad_labels), 0 when NULL                      */
  double sq_sum;           /* sum of the squared masked range differences (MSE = sq_sum / n_cells), bitwise reproducible  */
  int present[LT_COMPARE_MAX_PRESENT];                            /* the P values, ascending; entries from P on: undefined */
  unsigned counts[LT_COMPARE_MAX_PRESENT * LT_COMPARE_MAX_PRESENT]; /* dense P x P: counts[t * P + s] = cells whose masked   */
                                                                  /* target label is present[t] and source label present[s]; */
                                                                  /* entries from P * P on are undefined                     */
} lt_compare_record;

/* lt_compare_record_dev -- the array part of compare() (auxiliary/laserscan.py:1181-1301) + iouEval.addBatch
 * (np_ioueval.py:31-47) of one output scan.  src_*: the images of lt_source_scan_dev; tgt_label / tgt_range: the target
 * scan's label and range image (DeviceDeform's `label` / `range`; for `cp` the merged scan's, laserscan.py:1189-1194).
 *   1. a cell that is black in the source, or whose source label is 0, is background in both images: labels 0, ranges 0
 *   2. counts over the (target, source) pairs of masked labels, for the values present only, values ascending
 *   3. sq_sum: float32 (source - target)^2 per cell, summed in float64 -- per workgroup in a fixed tree, the workgroups'
 *      partial sums in a fixed order: two calls on the same images give the same bits
 * The class renumbering and getIoU / getacc are the host's (lidar_transfer_amd.post.confusion_metrics).  `record`: DEVICE
 * memory or pinned HOST memory (lt_host_alloc); it is written by an asynchronous copy behind the kernels, so the host reads
 * it after an event recorded behind this call, without another synchronisation.  All images DEVICE pointers [n]. */
int lt_compare_record_dev(lt_evaluator* ev, const int* src_label, const unsigned char* src_black, const int* tgt_label,
                          const float* src_range, const float* tgt_range, int n, const unsigned* src_bad_labels,
                          lt_compare_record* record, void* stream);

/* ---- misc ------------------------------------------------------------------------------------ */

/* Message of the last error raised on the calling thread ("" if none). */
const char* lt_last_error(void);

/* Library version string, e.g. "lidarhip 0.1 (gfx950)". */
const char* lt_version(void);

/* Layout version of the structs this header declares (lt_proj_images, lt_stats, lt_mm_geometry ...): a caller compiled
 * against another header must not pass them.  lt_abi_version() returns the library's; the Python binding compares at load. */
#define LT_ABI_VERSION 10
int lt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LIDARHIP_H */
