// Internal definitions shared by the translation units of libtdtrt.so (tdt_rt.hip: context, the trace path and its state
// (tdt::TraceState: only forward-declared here), helpers;
// tdt_multi.hip: the multi-device context; tdt_build.hip: the GPU octree builder; tdt_edit.hip: voxel edits;
// tdt_query.hip: ray queries; tdt_compact.hip: voxel extraction and compaction; tdt_region.hip: region edits;
// tdt_connect.hip: connected components; tdt_morph.hip: voxel morphology; tdt_mesh.hip: triangle-mesh voxelisation;
// tdt_fill.hip: enclosed space; tdt_surface.hip: surface extraction; tdt_distance.hip: exact Euclidean distance;
// tdt_bitvol.hip: the dense bit volume that tdt_fill.hip, tdt_distance.hip, tdt_xform.hip and tdt_geodesic.hip stand on, from
// the tree's list to the result's (its templates over a unit's own kernels: bitvol_device.hpp); tdt_xform.hip: affine
// transforms of selections; tdt_geodesic.hip: geodesic distance; tdt_voxlist.hip: the Morton-sorted voxel list the list-based units
// share: the capped tree list, keys, last-of-run unique, scan-gather-count); tdt_denoise.hip: first-hit guide images and the
// edge-stopping filter over them; tdt_reproject.hip: temporal reprojection of samples through those guides; tdt_variance.hip: the
// variance of the luminance and the filter it guides (what these three share on the device: denoise_device.hpp); tdt_upsample.hip:
// guide-keyed upsampling of a frame traced at reduced resolution; tdt_adaptive.hip: the sampling controller that turns per-pixel
// variance into the masks of tdt_dispatch_accumulate_masked; tdt_select.hip: screen-space selection, where the two halves meet:
// voxel-id images, overlays of a voxel list and the voxels of a rectangle; tdt_screen.hip: through-selection, the tree's voxels
// projected into a view and tested against a rectangle, a polygon or a mask; tdt_smooth.hip: voxel smoothing, a ball-density
// threshold filter and the density field, on the bit volume too; tdt_stroke.hip: stroke brushes, capsule and swept-box polylines
// voxelised like a mesh; tdt_faces.hip: face tools, the exposed faces (surface_device.hpp, the one face list of tdt_surface.hip)
// labelled into coplanar face regions (unionfind_device.hpp, the union-find of tdt_connect.hip) and swept into columns.  The host helpers
// around a call that every editing unit repeated are inline here: first_member, edit_replicas, read_word, rebuild_install, list_to_host, region_extract_source;
// and so is the host frame of an image call: device_image, camera_program, overlap, image_grid, images_of_context, images_fit, run_passes.
// Nothing here is part of the C ABI (include/tdt_rt.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "tdt_rt.h"

constexpr int kNumSlots = 8;

// What a trace dispatch depends on besides the sample range — compared with what the recorded pixel costs were measured on
// (see plan_order() in tdt_rt.hip).  A plain struct, zero-filled before it is written, so that a field added later is part of the comparison
// by construction (it used to be a byte string that silently dropped what did not fit).
struct CostSig {
  int32_t cam_i[4]; float cam_f[12]; int32_t part[2];
  float octree_f[7]; int32_t octree_i[3];
  int32_t cover[2], image[2];
  struct { const void *buffer; unsigned long long version; } slot[kNumSlots];
};

namespace tdt { struct Multi; struct EditScratch; struct TraceState; struct BitBox; }
struct TraceParams;

struct tdt_buffer {
  tdt_ctx *ctx;
  void *dev;
  size_t bytes;
  unsigned long long version;   // bumped by every write: invalidates derived data (LDS table image)
  unsigned char shadow[64];   // first bytes, host side: the octree uniform blocks are read from here
  std::vector<tdt_buffer *> replicas;   // multi-device context: the per-device buffers behind this handle (dev is null)
};

struct tdt_image {
  tdt_ctx *ctx;
  float *dev;
  int w, h;
  bool owned;
  tdt_image *full;              // multi-device context: the assembled frame on the first device (dev aliases its memory)
};

// What more than one translation unit uses.  Everything the trace path keeps between launches is tdt::TraceState (tdt_rt.hip).
struct tdt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  tdt_buffer *ssbo[kNumSlots] = {};
  tdt_buffer *atomic0 = nullptr;
  tdt_image *image0 = nullptr;
  unsigned long long *counters = nullptr;   // instrumented dispatches and tdt_selftest (on a multi-device front too: tdt_multi.hip frees it)
  int num_cus = 0;
  tdt::TraceState *trace = nullptr;        // state of the trace path (tdt_rt.hip); null on a multi-device front, whose members have their own
  tdt::Multi *multi = nullptr;             // non-null: this is a multi-device context (tdt_ctx_create_multi); see tdt_multi.hip
  tdt::EditScratch *edit = nullptr;        // scratch of the parallel voxel-edit path (tdt_edit.hip), allocated on first use
  void *query = nullptr; size_t query_bytes = 0;   // staging of the host-memory ray queries (tdt_query.hip), grow-only
  void *denoise = nullptr; size_t denoise_bytes = 0;   // ping-pong images of tdt_image_denoise (tdt_denoise.hip), grow-only
  unsigned long long *reproject_counts = nullptr;      // tdt_debug_reproject_counts: four device words of the last tdt_image_reproject (tdt_reproject.hip)
  unsigned long long *upsample_counts = nullptr;       // tdt_debug_upsample_counts: the device word block of the last tdt_image_upsample (tdt_upsample.hip)
  unsigned long long *adapt_counts = nullptr;          // tdt_debug_adapt_counts: the device word block of the last tdt_image_adapt (tdt_adaptive.hip)
  unsigned long long *overlay_counts = nullptr;        // tdt_debug_overlay_counts: the device word block of the last tdt_image_overlay (tdt_select.hip)
  void *select = nullptr; size_t select_bytes = 0;     // the list of tdt_image_overlay in device memory (tdt_select.hip), grow-only
  uint64_t screen_counts[4] = {0, 0, 0, 0};            // tdt_debug_screen_counts: of the last through-selection that returned TDT_OK (tdt_screen.hip)
  uint32_t fill_passes = 0;      // tdt_debug_fill_passes: flood passes of the last enclosed-space call that changed the volume (tdt_fill.hip)
  uint32_t xform_bricks[2] = {0, 0};   // tdt_debug_xform_bricks: the last transform's bricks in the domain / kept for the count and emit passes (tdt_xform.hip)
  int faces_premerge = 1;        // tdt_debug_faces_premerge: the face labelling's hook stage pre-merges runs inside a wave (tdt_faces.hip)
  uint32_t geodesic_passes = 0;  // tdt_debug_geodesic_passes: relaxation passes of the last geodesic call that changed the volume (tdt_geodesic.hip)
  std::vector<tdt_buffer *> buffers;
  std::vector<tdt_image *> images;
  std::vector<tdt_compute *> computes;
};

struct tdt_compute {
  tdt_ctx *ctx;
  int kind;
  // `uniform Camera camera` raytracer.comp:133-146; GL initialises uniforms to 0
  int32_t image_width, image_height, samples_per_pixel, max_bounce;
  float horizontal[3], vertical[3], lower_left_corner[3], origin[3];
  int part_rank, part_world;
  std::vector<tdt_compute *> replicas;  // multi-device context: the per-device programs behind this handle
};

namespace tdt {

int fail(tdt_ctx *ctx, int code, const std::string &msg);           // records the message, returns the code
int hip_fail(tdt_ctx *ctx, hipError_t e, const char *what);
#define TDT_HIP(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return tdt::hip_fail((ctx), e_, #call); } while (0)

// blocks of 256 lanes: every kernel of the editing units is launched with these
inline unsigned blocks_of(unsigned long long lanes) { return (unsigned)((lanes + 255) / 256); }
// synchronises the stream when it leaves scope: declared after what the stream's queued work still reads or writes
struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } };
// the tail of the calls that list into host memory by tdt_octree_extract's rules: *n_out = n, and when host_out is given and
// n > 0 the capacity check ("capacity C < n <items>"), the copy of n items of item_bytes and one synchronisation
inline int list_to_host(tdt_ctx *ctx, hipStream_t st, const void *dev, size_t n, size_t item_bytes, const char *items, void *host_out,
                        size_t capacity, size_t *n_out) {
  *n_out = n;
  if (!host_out || n == 0) return TDT_OK;
  if (capacity < n) return fail(ctx, TDT_ERR_INVALID_VALUE, "capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " " + items);
  TDT_HIP(ctx, hipMemcpyAsync(host_out, dev, n * item_bytes, hipMemcpyDeviceToHost, st));
  TDT_HIP(ctx, hipStreamSynchronize(st));
  return TDT_OK;
}

template <class T> void erase_from(std::vector<T *> &v, T *p) {
  for (size_t i = 0; i < v.size(); i++) if (v[i] == p) { v.erase(v.begin() + i); return; }
}

// ComputeShader::dispatch_compute's group arithmetic (compute_shader.rs:30-32) and what it covers
struct Cover { int groups_x, groups_y, cover_w, cover_h; };
Cover cover_of(const tdt_compute *c, int width, int height);
// 32x32 work-groups of the covered image and the ones this rank owns (t % world == rank)
struct Tiles { int tiles_x, tiles_y, total, owned; };
Tiles tiles_of(const tdt_compute *c, const Cover &k);

// a tdt_buffer over device memory some kernel of this library filled: `dev` comes from hipMalloc(bytes + 16) with the
// 16 bytes of slack zeroed, and belongs to the buffer from here on (tdt_rt.hip)
int adopt_device_buffer(tdt_ctx *ctx, void *dev, size_t bytes, tdt_buffer **out);

// OctreeFloats / OctreeInts from the shadows of the buffers bound to slots 6 / 7 (both must be bound) into P
int octree_uniforms(tdt_ctx *ctx, TraceParams &P);

// ---- tdt_multi.hip: every public entry point forwards here when the handle belongs to a multi-device context ----
void multi_destroy(tdt_ctx *ctx);
int multi_finish(tdt_ctx *ctx);
int multi_compute_create(tdt_ctx *ctx, int kind, tdt_compute **out);
void multi_compute_destroy(tdt_compute *c);
int multi_set_i32(tdt_compute *c, const char *name, int32_t v);
int multi_set_vec3f(tdt_compute *c, const char *name, float x, float y, float z);
int multi_buffer_create(tdt_ctx *ctx, const void *data, size_t bytes, tdt_buffer **out);
void multi_buffer_destroy(tdt_buffer *b);
int multi_bind_buffer_base(tdt_ctx *ctx, int target, unsigned slot, tdt_buffer *b);
int multi_buffer_sub_data(tdt_buffer *b, size_t offset, size_t bytes, const void *data);
int multi_image_create(tdt_ctx *ctx, void *device_ptr, int width, int height, tdt_image **out);
void multi_image_destroy(tdt_image *img);
int multi_dispatch_compute(tdt_compute *c, int width, int height, int depth);
int multi_dispatch_accumulate(tdt_compute *c, int width, int height, int depth, int spp_begin, int spp_count, void *carry);
int multi_dispatch_resolve(tdt_compute *c, int width, int height, int depth, int total_spp);
int multi_dispatch_counted(tdt_compute *c, int width, int height, int depth, uint64_t counts[8]);
int multi_forget_costs(tdt_ctx *ctx);
tdt_ctx *multi_first_member(tdt_ctx *front);
const std::vector<tdt_ctx *> &multi_members(tdt_ctx *front);
// the single-device context a call that only reads runs on: a multi-device front's first member, or ctx itself
inline tdt_ctx *first_member(tdt_ctx *ctx) { return ctx->multi ? multi_first_member(ctx) : ctx; }
// an edit on every replica: one(member, &cells) on the context itself or on each member in turn, the first failure ending it (the
// checks fail on the first member, before anything is written, and the others hold the same bytes).  *n_cells (may be null) = the
// first member's count; after a failure only where cells_on_failure is set and that count is non-zero (a misfit's size to grow to).
template <class One> int edit_replicas(tdt_ctx *ctx, bool cells_on_failure, uint32_t *n_cells, One one) {
  uint32_t nc = 0;
  if (!ctx->multi) {
    const int rc = one(ctx, &nc);
    if (n_cells && (rc == TDT_OK || (cells_on_failure && nc))) *n_cells = nc;
    return rc;
  }
  if (!ctx->ssbo[TDT_SLOT_CELLS] || !ctx->ssbo[TDT_SLOT_OCTREE_INTS])
    return fail(ctx, TDT_ERR_INCOMPLETE, std::string("no buffer bound to shader-storage slot ") + (ctx->ssbo[TDT_SLOT_CELLS] ? "7" : "0"));
  tdt_ctx *m0 = multi_first_member(ctx);
  for (tdt_ctx *m : multi_members(ctx)) {
    uint32_t k = 0;
    const int rc = one(m, &k);
    if (m == m0) nc = k;
    if (rc != TDT_OK) { if (n_cells && cells_on_failure && nc) *n_cells = nc; return rc; }
  }
  if (n_cells) *n_cells = nc;
  return TDT_OK;
}
// one device word into *host: the copy queued on st, then ONE host synchronisation (hipGetLastError stays with the caller)
inline int read_word(tdt_ctx *front, hipStream_t st, const uint32_t *dev, uint32_t *host) {
  TDT_HIP(front, hipMemcpyAsync(host, dev, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TDT_HIP(front, hipStreamSynchronize(st));
  return TDT_OK;
}

// ---- tdt_edit.hip ----
int launch_update(tdt_compute *c, int width, int height, int depth);
void edit_scratch_destroy(tdt_ctx *ctx);

// ---- tdt_build.hip: pieces of the builder other units reuse ----
// stable LSD radix sort of n (key, value) pairs by the whole 32-bit key, asynchronous on `st`; k / v end up pointing at the
// sorted arrays (the other pair is scratch); hist / scratch: sort_hist_words(n) / sort_scratch_words(n) words
size_t sort_hist_words(uint32_t n);
size_t sort_scratch_words(uint32_t n);
hipError_t sort_pairs_u32(hipStream_t st, uint32_t *&k, uint32_t *&v, uint32_t *k_alt, uint32_t *v_alt, uint32_t n, uint32_t *hist,
                          uint32_t *scratch);
// tdt_octree_build_cells over n > 0 voxels {x, y, z, material + 1} already in device memory of ctx (synchronises)
int build_cells_from_device(tdt_ctx *ctx, const int32_t *d_vox, uint32_t n, int depth, tdt_buffer **out, uint32_t *n_cells);

// ---- tdt_compact.hip: pieces region edits and voxel morphology reuse ----
struct DeviceScratch {         // device temporaries of one operation (or the arrays of a longer-lived owner), freed together
  std::vector<void *> ptrs;
  ~DeviceScratch() { release(); }
  void release() { for (void *p : ptrs) (void)hipFree(p); ptrs.clear(); }
  void drop(void *p) {           // one of them ahead of the others (null: nothing)
    for (size_t i = 0; i < ptrs.size(); i++) if (ptrs[i] == p) { (void)hipFree(p); ptrs.erase(ptrs.begin() + i); return; }
  }
  template <class T> T *get(size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return (T *)p;
  }
};
// slot 0 / 7 bound and max_depth 1..10 on ctx (a single-device context); errors are reported on `front`
int walk_inputs(tdt_ctx *front, tdt_ctx *ctx, int *depth);
// the bound tree's voxels {x, y, z, value + 1}, Morton-sorted, in device memory of ctx (*out allocated in S, null when
// *n == 0).  A LEAF value >= leaf_limit: TDT_ERR_INVALID_VALUE.  Ordered after queued work; one host synchronisation.
int tree_voxels(tdt_ctx *front, tdt_ctx *ctx, uint32_t leaf_limit, DeviceScratch &S, int4 **out, uint32_t *n, int *depth);
// the fit check and in-place install of compaction: nc cells of `built` (null: one all-EMPTY root) over the bound cells
// buffer, tail zeroed, counter = nc, versions bumped.  Too large: TDT_ERR_INVALID_VALUE, nothing written.  Takes `built`.
int install_cells(tdt_ctx *front, tdt_ctx *ctx, tdt_buffer *built, uint32_t nc);
// the end of an edit: the n_res voxels of res (device memory of ctx; 0: the empty tree, one cell) rebuilt, a member's error text
// forwarded to `front`, release() freeing the caller's scratch, then the install.  *n_cells is written after the install, and with
// cells_on_misfit before it too: the size the caller must grow the buffer to.
template <class Release>
int rebuild_install(tdt_ctx *front, tdt_ctx *ctx, const int4 *res, uint32_t n_res, int depth, bool cells_on_misfit, uint32_t *n_cells, Release release) {
  tdt_buffer *built = nullptr;
  uint32_t nc = 1;
  if (n_res) {
    const int rc = build_cells_from_device(ctx, (const int32_t *)res, n_res, depth, &built, &nc);
    if (rc != TDT_OK) return ctx == front ? rc : fail(front, rc, tdt_last_error(ctx));
  }
  release();
  if (cells_on_misfit) *n_cells = nc;
  if (int rc = install_cells(front, ctx, built, nc)) return rc;
  *n_cells = nc;
  return TDT_OK;
}

// ---- tdt_voxlist.hip: the steps the list-based units take on a Morton-sorted voxel list.  Everything is queued on `st`; errors are
// reported on `front`; no_memory is the caller's out-of-memory text ----
constexpr unsigned long long kVoxelListCap = TDT_REGION_BRUSH_CAP;   // voxels of the tree's list: what the 2^26 caps of the units equal
// tree_voxels with the leaf limit of the editing units (254), held to kVoxelListCap (checked on the expanded list: 16 B per voxel
// of the tree before it can fail)
int tree_voxels_capped(tdt_ctx *front, tdt_ctx *ctx, DeviceScratch &S, int4 **out, uint32_t *n, int *depth);
// the cap alone, for a unit that is handed the tree's list (a VoxelSelect): n > kVoxelListCap is TDT_ERR_INVALID_VALUE
int voxlist_within_cap(tdt_ctx *front, uint32_t n);
// k[i] = the Morton key of voxel i, n > 0
void voxlist_keys(hipStream_t st, const int4 *v, uint32_t n, uint32_t *k);
// behind a stable sort of n > 0 pairs by key: flag[i] = i is the LAST of its run of equal keys and not the all-ones key, over n + 1
// lanes (flag[n] = 0); then, excl being the scanned flags, the flagged pairs into (uk, uv) in order and *count = their number
void voxlist_last_flags(hipStream_t st, const uint32_t *keys, uint32_t n, uint32_t *flag);
void voxlist_unique(hipStream_t st, const uint32_t *keys, const uint32_t *vals, uint32_t n, const uint32_t *excl, uint32_t *uk, uint32_t *uv,
                    uint32_t *count);
// the end of a pass of keep flags: keep (n + 1 words, keep[n] = 0; n > 0) scanned in place (scr: its scratch), the kept voxels of v, and
// their keys where k / ok are given, gathered in order into ov / ok, hipGetLastError, and *total (host) = their number: ONE synchronisation
int scan_gather_count(tdt_ctx *front, hipStream_t st, const int4 *v, const uint32_t *k, uint32_t *keep, uint32_t n, uint32_t *scr, int4 *ov,
                      uint32_t *ok, uint32_t *total);

// ---- tdt_region.hip: the V-only path of region edits (PAINT / CLEAR / intersect) driven by a per-voxel membership ----
struct VoxelSelect {
  // queued on ctx's stream once V exists (nv > 0 voxels {x, y, z, value + 1}, Morton-sorted, in S): voxel i is selected when
  // (*selected)[(*label)[i]] != 0; both arrays live in S.  Errors are reported on `front`.
  virtual int run(tdt_ctx *front, tdt_ctx *ctx, const int4 *v, uint32_t nv, int depth, DeviceScratch &S, const uint32_t **label,
                  const uint32_t **selected) = 0;
 protected:
  ~VoxelSelect() = default;
};
// op TDT_REGION_PAINT (material 0..253) or TDT_REGION_CLEAR of the selected voxels, on every replica, by
// tdt_octree_edit_region's rules (the caller has checked op and material)
int region_edit_selected(tdt_ctx *ctx, int op, int32_t material, VoxelSelect &sel, uint32_t *n_cells);
// the selected voxels of device_ids[0]'s tree into host memory, by tdt_octree_extract_region's rules
int region_extract_selected(tdt_ctx *ctx, VoxelSelect &sel, int32_t *host_out, size_t capacity, size_t *n_out);

// ---- tdt_region.hip: the voxel-list form driven by a list that is produced in device memory and never leaves it ----
struct VoxelSource {
  // once slots 0 / 7 are known good on ctx (depth = its max_depth): *vox = *n voxels {x, y, z, material + 1} inside the grid,
  // m 1..254, in device memory of ctx (allocated in S; may be null when *n == 0).  Runs on ctx's stream and may synchronise it.
  // Errors are reported on `front`.
  virtual int run(tdt_ctx *front, tdt_ctx *ctx, int depth, DeviceScratch &S, const int4 **vox, uint32_t *n) = 0;
 protected:
  ~VoxelSource() = default;
};
// tdt_octree_edit_voxels(op, the source's list) on every replica (the caller has checked op)
int region_edit_source(tdt_ctx *ctx, int op, VoxelSource &src, uint32_t *n_cells);
// the voxels of device_ids[0]'s tree that the source's list (at the tree's max_depth) holds, with the tree's materials, into host
// memory by tdt_octree_extract_region's rules (tdt_stroke.hip)
int region_intersect_source(tdt_ctx *ctx, VoxelSource &src, int32_t *host_out, size_t capacity, size_t *n_out);
// the source's list on device_ids[0] (depth: what its run() is given; no tree need be bound) into host memory, by
// tdt_octree_extract's rules
inline int region_extract_source(tdt_ctx *ctx, VoxelSource &src, int depth, int32_t *host_out, size_t capacity, size_t *n_out) {
  tdt_ctx *m = first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  Drain drain{m->stream};
  DeviceScratch S;
  const int4 *vox = nullptr;
  uint32_t n = 0;
  if (int rc = src.run(ctx, m, depth, S, &vox, &n)) return rc;
  return list_to_host(ctx, m->stream, vox, n, sizeof(int4), "voxels", host_out, capacity, n_out);
}

// ---- tdt_mesh.hip: what the solid forms (tdt_fill.hip) start from ----
// everything about a mesh that does not depend on the grid, checked on the host before anything is queued
int check_mesh(tdt_ctx *ctx, const tdt_mesh *m);
// the voxels of a mesh that passed check_mesh, {x, y, z, material + 1}, Morton-sorted and unique, in device memory of ctx
// (allocated in S; null when *n == 0).  Queued on ctx's stream; synchronises.  Errors are reported on `front`.
int mesh_voxels(tdt_ctx *front, tdt_ctx *ctx, const tdt_mesh *m, int depth, DeviceScratch &S, const int4 **out, uint32_t *n);

// ---- tdt_bitvol.hip: the dense bit volume over a box of the grid (layout: bitvol_device.hpp), as enclosed space, exact distance,
// transforms and geodesic distance use it.  Everything is queued on `st`; errors are reported on `front`; no_memory is the
// caller's out-of-memory text ----
constexpr unsigned long long kBitvolCap = kVoxelListCap;   // voxels of a result and of a field's box, as of the tree's list
// B over lo..hi (inclusive, inside the grid)
void bitvol_layout(const int lo[3], const int hi[3], BitBox &B);
// the bounding box of n > 0 voxels {x, y, z, m} in device memory: box[0..2] = min, box[3..5] = max.  One synchronisation.
// A voxel outside the grid of side 2^depth: TDT_ERR_INVALID_VALUE with the text `outside`.
int bitvol_list_bbox(tdt_ctx *front, hipStream_t st, const int4 *v, uint32_t n, int depth, DeviceScratch &S, const char *no_memory,
                     const char *outside, int box[6]);
// occ (B.n_words words) cleared, then the bits of the voxels inside B set; keys / vals (n each) = every voxel's Morton key and m
int bitvol_rasterise(tdt_ctx *front, hipStream_t st, const int4 *v, uint32_t n, const BitBox &B, uint32_t *occ, uint32_t *keys, uint32_t *vals);
// the end of an emit: n > 0 pairs (Morton key, m) in k / v, sorted by key first if asked, into *out = n voxels {x, y, z, m}
// allocated in S.  Synchronises.
int bitvol_emit_list(tdt_ctx *front, hipStream_t st, uint32_t *k, uint32_t *v, uint32_t n, bool sort, DeviceScratch &S, const char *no_memory,
                     const int4 **out);

// ---- tdt_query.hip ----
void query_scratch_destroy(tdt_ctx *ctx);
// the kernel arguments a query needs: slots 0, 6, 7 of the member context m (unbound: TDT_ERR_INCOMPLETE); errors are reported on `front`
int query_params(tdt_ctx *front, tdt_ctx *m, TraceParams &P);
// the camera uniforms of a program into P (what primary_ray reads)
void query_camera(const tdt_compute *cam, TraceParams &P);

// ---- tdt_reproject.hip: a view as the device projects into it (reproject_device.hpp, view_project) ----
struct ViewRows {
  float ru[3], rv[3], rw[3];                         // rows of det * inverse(a | b | c) of the view, det > 0
  float org[3];                                      // its origin
  float sx, sy;                                      // (float)(image_width - 1), (float)(image_height - 1)
};
// the header's per-call arithmetic (tdt_image_reproject) from a view's fp32 fields; false: the determinant is zero or not finite
bool view_rows(const tdt_view &v, ViewRows &R);

// ---- tdt_denoise.hip, and the host frame of an image call that it, tdt_variance.hip, tdt_reproject.hip, tdt_upsample.hip and
// tdt_adaptive.hip share ----
constexpr int kMaxPasses = 8;
void denoise_scratch_destroy(tdt_ctx *ctx);
void reproject_counts_destroy(tdt_ctx *ctx);           // (tdt_reproject.hip)
void upsample_counts_destroy(tdt_ctx *ctx);            // (tdt_upsample.hip)
void adapt_counts_destroy(tdt_ctx *ctx);               // (tdt_adaptive.hip)
void select_scratch_destroy(tdt_ctx *ctx);             // (tdt_select.hip: the overlay's list and its counts)
// the images passes 0 .. passes - 1 (1..8) of an in-place filter over img (w x h RGBA32F on member m) read and write: pass p goes
// seq[p] -> seq[p + 1], seq[0] = img, the others the context's grow-only scratch; seq holds passes + 1 entries.  Ends in img
// unless passes == 1 (run_passes copies seq[1] back).
int denoise_sequence(tdt_ctx *front, tdt_ctx *m, float *img, int w, int h, int passes, float **seq);
// the image a call works on: a multi-device handle stands for the assembled frame on the first device
inline const tdt_image *device_image(const tdt_image *img) { return img->ctx->multi ? img->full : img; }
// the program whose camera a call reads: a multi-device program's first member's
inline const tdt_compute *camera_program(const tdt_compute *c) { return c->replicas.empty() ? c : c->replicas[0]; }
// do two images share memory?
inline bool overlap(const tdt_image *a, const tdt_image *b) {
  const float *ea = a->dev + (size_t)a->w * (size_t)a->h * 4, *eb = b->dev + (size_t)b->w * (size_t)b->h * 4;
  return a->dev < eb && b->dev < ea;
}
// one block per tw x th tile of a w x h image: the grid and its row length
inline int image_grid(tdt_ctx *ctx, int w, int h, int tw, int th, const char *too_large, dim3 &grid, uint32_t &tiles_x) {
  const unsigned long long nx = ((unsigned long long)w + tw - 1) / tw, ny = ((unsigned long long)h + th - 1) / th;
  if (nx * ny > 0x7FFFFFFFull) return fail(ctx, TDT_ERR_INVALID_VALUE, too_large);
  grid = dim3((unsigned)(nx * ny)); tiles_x = (uint32_t)nx;
  return TDT_OK;
}
// The handles of an image call (null: not given), in two steps, because an entry point checks its other arguments in between.
// First: every one belongs to ctx.
inline int images_of_context(tdt_ctx *ctx, const tdt_image *const *handles, int n, const char *another_context) {
  for (int i = 0; i < n; i++)
    if (handles[i] && handles[i]->ctx != ctx) return fail(ctx, TDT_ERR_INVALID_OPERATION, another_context);
  return TDT_OK;
}
// Then: im[i] = the device image of each; the first n_sized have the size of the first, and no two of the n are one image or
// share memory — but for handles in_place_i < in_place_j at one address (tdt_image_reproject's mean_out == sums; -1: none).
inline int images_fit(tdt_ctx *ctx, const tdt_image *const *handles, int n, int n_sized, const tdt_image **im, const char *differ_in_size,
                      const char *share_memory, int in_place_i = -1, int in_place_j = -1) {
  for (int i = 0; i < n; i++) im[i] = handles[i] ? device_image(handles[i]) : nullptr;
  for (int i = 1; i < n_sized; i++)
    if (im[i] && (im[i]->w != im[0]->w || im[i]->h != im[0]->h)) return fail(ctx, TDT_ERR_INVALID_VALUE, differ_in_size);
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) {
      if (!im[i] || !im[j]) continue;
      if (i == in_place_i && j == in_place_j && im[i]->dev == im[j]->dev) continue;
      if (im[i] == im[j] || overlap(im[i], im[j])) return fail(ctx, TDT_ERR_INVALID_VALUE, share_memory);
    }
  return TDT_OK;
}
// Passes 1..8 of an in-place filter over the image a, on the context's first member: the grid of tw x th tiles, the scratch
// sequence, pass p (step 2^p) as launch(tile_step<1>{}) / launch(tile_step<2>{}) / launch(tile_step<0>{}) — the two LDS-tile
// kernels, then the gather — with (step, grid, stream, src, dst, tiles_x), and the copy back when the sequence ends in the scratch.
template <int S> using tile_step = std::integral_constant<int, S>;
template <class Launch> int run_passes(tdt_ctx *ctx, const tdt_image *a, int passes, int tw, int th, Launch launch) {
  dim3 grid;
  uint32_t tiles_x;
  if (int rc = image_grid(ctx, a->w, a->h, tw, th, "image too large", grid, tiles_x)) return rc;
  tdt_ctx *m = first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  float *seq[kMaxPasses + 1];
  if (int rc = denoise_sequence(ctx, m, a->dev, a->w, a->h, passes, seq)) return rc;
  for (int p = 0; p < passes; p++) {
    const float *src = seq[p];
    float *dst = seq[p + 1];
    if (p == 0) launch(tile_step<1>{}, 1, grid, m->stream, src, dst, tiles_x);
    else if (p == 1) launch(tile_step<2>{}, 2, grid, m->stream, src, dst, tiles_x);
    else launch(tile_step<0>{}, 1 << p, grid, m->stream, src, dst, tiles_x);
  }
  TDT_HIP(ctx, hipGetLastError());
  if (seq[passes] != seq[0])
    TDT_HIP(ctx, hipMemcpyAsync(seq[0], seq[passes], (size_t)a->w * (size_t)a->h * 16, hipMemcpyDeviceToDevice, m->stream));
  return TDT_OK;
}

}  // namespace tdt
