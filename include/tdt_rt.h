/*
 * tdt_rt.h — C ABI of libtdtrt.so, the MI355X (gfx950) drop-in for the per-pixel voxel path
 * trace of Avokadoen/tdt4230_project_raytracing.
 *
 * The reference has no FFI layer: its boundary is the `src/renderer` GL-wrapper API that
 * main.rs / camera.rs / octree.rs call on the thread that owns the GL context.  Every entry
 * point below replaces one of those calls one-for-one (cited as file:line of the reference);
 * a Rust maintainer binds them with the `extern "C"` block shown in INTEGRATION.md.
 *
 * Conventions (the GL contract, kept):
 *   - context-affine, no internal locking: call from one thread per context;
 *   - host pointers are borrowed for the duration of the call only; uploads COPY (glBufferData);
 *   - every call returns an int: 0 = TDT_OK, otherwise a TDT_ERR_* code (never aborts); the
 *     message for the last error of a context is available from tdt_last_error();
 *   - handles are owned by their context and die with it;
 *   - all dispatches are asynchronous on the context's HIP stream; tdt_finish() is glFinish().
 * There is NO CPU fallback: without a usable HIP device tdt_ctx_create fails with
 * TDT_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef TDT_RT_H
#define TDT_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdt_ctx tdt_ctx;         /* the GL context            main.rs:58-61,108-112 */
typedef struct tdt_compute tdt_compute; /* renderer::ComputeShader   compute_shader.rs:10-13 */
typedef struct tdt_buffer tdt_buffer;   /* renderer::vbo::VertexBufferObject   vbo.rs:9-13 */
typedef struct tdt_image tdt_image;     /* renderer::texture::Texture          texture.rs:7-14 */

enum {
  TDT_OK = 0,
  TDT_ERR_NO_DEVICE = 1,          /* no HIP device / HIP runtime failure at context creation  */
  TDT_ERR_HIP = 2,                /* a HIP call failed (check_for_gl_error analogue, mod.rs:62-68) */
  TDT_ERR_INVALID_ENUM = 0x0500,  /* = GL_INVALID_ENUM,      mod.rs:47 */
  TDT_ERR_INVALID_VALUE = 0x0501, /* = GL_INVALID_VALUE,     mod.rs:48 */
  TDT_ERR_INVALID_OPERATION = 0x0502, /* = GL_INVALID_OPERATION, mod.rs:49 */
  TDT_ERR_VARIABLE_NOT_FOUND = 3, /* InitializeErr::VariableNotFound, program.rs:144-165, mod.rs:31 */
  TDT_ERR_INCOMPLETE = 4          /* dispatch with a required binding / uniform missing */
};

/* kinds for tdt_compute_create (the two compute programs the reference links) */
enum {
  TDT_PROGRAM_RAYTRACER = 0,      /* assets/shaders/raytracer.comp */
  TDT_PROGRAM_OCTREE_UPDATE = 1   /* assets/shaders/octree_update.comp (next row SURVEY §8f-2): one voxel edit per
                                     invocation; reads slots 0,5,6,7 + the atomic counter, group size {1,1,1} */
};
/* targets for tdt_bind_buffer_base (values are the GL enums the reference passes) */
enum {
  TDT_SHADER_STORAGE_BUFFER = 0x90D2, /* main.rs:352,383,408,430,448; octree.rs:67,98,144 */
  TDT_ATOMIC_COUNTER_BUFFER = 0x92C0  /* octree.rs:115 (accepted, unused by the trace) */
};
/* SSBO slots read by raytracer.comp (binding = N in the shader) */
enum {
  TDT_SLOT_CELLS = 0,        /* Node{uint value; uint type}[]          raytracer.comp:180-182 */
  TDT_SLOT_MATERIALS = 1,    /* {int type, attribute_index, albedo_index}[]   :189-196 */
  TDT_SLOT_ALBEDOS = 2,      /* {float x,y,z}[]                                :203-210 */
  TDT_SLOT_METAL = 3,        /* {float fuzz}[]                                 :214-219 */
  TDT_SLOT_DIELECTRIC = 4,   /* {float ir}[]                                   :222-227 */
  TDT_SLOT_DELTA = 5,        /* DeltaNode{vec3 pos; float type; float value}[] stride 32   octree_update.comp:41-48 */
  TDT_SLOT_OCTREE_FLOATS = 6,/* {vec4 min_point; float scale, inv_scale, inv_cell_count} :150-158 */
  TDT_SLOT_OCTREE_INTS = 7   /* {int max_depth, max_iter, cell_count}          :159-166 */
};

/* ---- context ------------------------------------------------------------------------- */
/* Replaces GL context creation + make_current (main.rs:58-61,108-112).  `stream` is a
 * hipStream_t to launch on (NULL: the context creates its own non-blocking stream). */
int tdt_ctx_create(int device_id, void *stream, tdt_ctx **out);
/* ONE context over n_devices GPUs, driven by the one thread that owns it — the reference's shape (a single
 * GL context on a single thread, main.rs:58-61,105-112), so a host bound per INTEGRATION.md drives a whole node without
 * knowing it.  Every call on the returned context and on handles created from it means what it means on a single-device
 * context: buffer uploads / sub-data / binds / uniforms / edit dispatches are replicated to every device (the scene is
 * read-only and small: <= 64 MB against 288 GB); tdt_dispatch_compute of the raytracer launches each device's share of the
 * 32x32 work-groups (t % n == i, as tdt_set_partition) on that device's own stream, brings the per-device tile buffers to
 * the first device with ONE RCCL gather (librccl.so.1, loaded on first use; a single-process communicator over the
 * devices) and de-interleaves them there into the bound image, so tdt_image_read / tdt_image_read_rgba8 /
 * tdt_image_device_ptr see the assembled frame on device_ids[0].  Device ids may repeat (several shares on one GPU — how
 * the path is tested on a one-GPU box); RCCL cannot form a communicator then and the gather becomes peer copies ordered
 * by events (TDT_MULTI_TRANSPORT=copy forces that, =rccl forbids it).  Progressive passes work on a node too:
 * tdt_dispatch_accumulate keeps every device's running sums (and, when carry_device_ptr is non-NULL, its hit-record carry, in
 * memory the context allocates per device — the pointer itself is not used) in that device's tile buffer, and
 * tdt_dispatch_resolve resolves per device, then gathers and assembles.  A dispatch that fails on one device drains the
 * devices already launched and leaves the context ready for the next frame.  Not available on a multi-device context
 * (TDT_ERR_INVALID_OPERATION): tdt_set_partition, tdt_dispatch_counted_range. */
int tdt_ctx_create_multi(int n_devices, const int *device_ids, tdt_ctx **out);
/* number of devices behind a context (1 for tdt_ctx_create) */
int tdt_ctx_device_count(const tdt_ctx *ctx);
void tdt_ctx_destroy(tdt_ctx *ctx);
/* glFinish: block until every dispatch of this context has completed. */
int tdt_finish(tdt_ctx *ctx);
/* message of the most recent error on this context ("" if none); ctx may be NULL for
 * errors of tdt_ctx_create itself */
const char *tdt_last_error(const tdt_ctx *ctx);
/* InitializeErr's Display (mod.rs:44-59) for a code */
const char *tdt_strerror(int code);

/* ---- programs / uniforms --------------------------------------------------------------- */
/* Shader::from_resources + Program::from_shaders + ComputeShader::new
 * (shader.rs:26, program.rs:101, compute_shader.rs:15-26; called main.rs:156-160). */
int tdt_compute_create(tdt_ctx *ctx, int kind, tdt_compute **out);
void tdt_compute_destroy(tdt_compute *c);          /* Program::drop, program.rs:169 */
/* the COMPUTE_WORK_GROUP_SIZE query of compute_shader.rs:18: {32,32,1} */
int tdt_compute_group_size(const tdt_compute *c, int out[3]);
/* Program::set_i32 / set_f32 / set_vector3_f32 / set_vector3_i32 (program.rs:35-83): uniform
 * addressed by its GLSL name, e.g. "camera.image_width"; unknown name or wrong type ->
 * TDT_ERR_VARIABLE_NOT_FOUND.  Takes effect for the next dispatch. */
int tdt_set_i32(tdt_compute *c, const char *name, int32_t value);
int tdt_set_f32(tdt_compute *c, const char *name, float value);
int tdt_set_vec3f(tdt_compute *c, const char *name, float x, float y, float z);
int tdt_set_vec3i(tdt_compute *c, const char *name, int32_t x, int32_t y, int32_t z);

/* ---- buffers ---------------------------------------------------------------------------- */
/* VertexBufferObject::new::<T>(Vec<T>, ..) = glGenBuffers + glBufferData (vbo.rs:32-55):
 * copies `bytes` bytes to device memory. */
int tdt_buffer_create(tdt_ctx *ctx, const void *data, size_t bytes, tdt_buffer **out);
void tdt_buffer_destroy(tdt_buffer *b);
/* gl::BindBufferBase(target, slot, id) as called by main.rs:352-448 and octree.rs:67-144 */
int tdt_bind_buffer_base(tdt_ctx *ctx, int target, unsigned slot, tdt_buffer *b);
/* gl::BufferSubData (octree.rs:174): how Octree::update_vbo hands the delta nodes to the edit program */
int tdt_buffer_sub_data(tdt_buffer *b, size_t offset, size_t bytes, const void *data);
/* NEW (the reference never reads a buffer back): finishes the stream and copies bytes to dst */
int tdt_buffer_read(tdt_buffer *b, size_t offset, size_t bytes, void *dst);

/* ---- image ------------------------------------------------------------------------------ */
/* Texture::new_2d(TEXTURE0, 0, RGBA32F, RGBA, w, h) (texture.rs:47-75, camera.rs:158-165):
 * W*H*4 floats in device memory, row 0 = bottom scan line, zero-filled (the reference leaves
 * it undefined). */
int tdt_image_create_rgba32f(tdt_ctx *ctx, int width, int height, tdt_image **out);
/* Same, but over device memory the caller owns (e.g. a torch tensor's data_ptr) — used by
 * the multi-GPU harness so the per-rank tile can be handed to RCCL without a copy. */
int tdt_image_wrap_device(tdt_ctx *ctx, void *device_ptr, int width, int height, tdt_image **out);
void tdt_image_destroy(tdt_image *img);
/* glBindImageTexture(unit, ..) of texture.rs:71: only unit 0 exists in raytracer.comp:4 */
int tdt_bind_image(tdt_ctx *ctx, unsigned unit, tdt_image *img);
int tdt_image_width(const tdt_image *img);
int tdt_image_height(const tdt_image *img);
void *tdt_image_device_ptr(const tdt_image *img);
/* NEW (the reference never reads back; quad.frag samples the texture): finishes the stream and
 * copies W*H*4 floats to dst */
int tdt_image_read(tdt_image *img, float *dst);
/* NEXT ROW SURVEY §8f-4, presentation: the RGBA8 frame the reference's quad pass (assets/shaders/quad.frag:10,
 * main.rs:582-600) leaves in a back buffer of the texture's size — per channel clamp to [0,1] (NaN -> 0), x 255, round half
 * to even (pinned on llvmpipe) — converted on the GPU, then W*H*4 bytes copied to dst after finishing the stream.
 * Texture row 0 is the bottom scan-line; top_down = 1 writes the top scan-line first (image-file order). */
int tdt_image_read_rgba8(tdt_image *img, int top_down, uint8_t *dst);

/* ---- dispatch --------------------------------------------------------------------------- */
/* ComputeShader::dispatch_compute(width, height, depth) (compute_shader.rs:28-38; called with
 * (W+1, H+1, 1) at main.rs:579, and by Octree::update_vbo octree.rs:179,181 for the edit program):
 * work-group counts are max(dim / group_size, 1) by integer floor division; for the raytracer the shader has no bounds check, image stores outside the image are dropped;
 * followed by the image-access barrier (= stream order here).  Asynchronous. */
int tdt_dispatch_compute(tdt_compute *c, int width, int height, int depth);

/* ---- extensions with no reference counterpart (documented in DESIGN.md) ------------------ */
/* Tile partition for one-process-per-GPU rendering: the covered image is cut into the
 * reference's own 32x32 work-groups, numbered row-major t = gy * ceil(cover_w/32) + gx; subsequent
 * dispatches of `c` trace only the groups with t % world == rank.  Default (0,1).
 * The bound image is then either the full W x H image (only owned groups are written) or this
 * rank's TILE BUFFER: an image of width 32 and height 32*n, n >= owned groups, i.e. the owned
 * groups packed as [k][32][32] RGBA in the order k = 0,1,.. <-> t = rank + k*world. */
int tdt_set_partition(tdt_compute *c, int rank, int world);
/* number of groups a dispatch of (width,height,depth) gives this rank; optionally the groups
 * per row and the total */
int tdt_owned_tiles(const tdt_compute *c, int width, int height, int depth, int *tiles_x, int *tiles_total);
/* number of pixels a dispatch of (width,height,depth) writes under the current partition */
int64_t tdt_covered_pixels(const tdt_compute *c, int width, int height, int depth);
/* De-interleave gathered tile buffers — `gathered` = device memory [world][tiles_per_rank][32][32]
 * RGBA as produced by `world` ranks — into the full image `dst` (the step after the RCCL gather). */
int tdt_assemble_tiles(tdt_compute *c, const void *gathered, int world, int tiles_per_rank, tdt_image *dst,
                       int width, int height, int depth);
/* Progressive form of the sample loop: adds samples [spp_begin, spp_begin+spp_count) of every
 * covered pixel, in sample order, to the bound image's rgb running sums (and keeps the
 * shader's loop-carried temporaries in `carry`, 16 floats per pixel of the bound image, in
 * device memory; NULL = start from / discard the initial state). */
int tdt_dispatch_accumulate(tdt_compute *c, int width, int height, int depth, int spp_begin, int spp_count,
                            void *carry_device_ptr);
/* tdt_dispatch_accumulate restricted to the covered pixels whose texel of `mask` is LIVE.  mask is an RGBA32F image of the bound
 * image's size; pixel P is live when mask[P].w >= 0.0f: +0 and -0 are live, negative values and NaN are not.  A live pixel gets
 * exactly the bits tdt_dispatch_accumulate would give it from the same prior state (image texel and carry); a pixel that is not
 * live keeps its image texel and its 64 bytes of carry byte for byte.  With no live pixel the call traces nothing and returns
 * TDT_OK.  The done flags are one more producer for the hand-out order's filter (the miss pre-pass is the other), so the trace
 * kernels are the ones every other dispatch runs.  A partition set with tdt_set_partition works on a full-size image: only owned
 * groups are traced.  The call may change the cost history, i.e. the schedule of later frames, never a pixel of them.  The state
 * image of tdt_image_adapt is such a mask.
 * Errors, nothing traced: a NULL mask, a negative range, an unaligned carry, a mask whose size differs from the bound image's:
 * TDT_ERR_INVALID_VALUE.  A multi-device context; a bound tile buffer (the full image must be bound); a mask of another context;
 * a mask that is the bound image or shares memory with it: TDT_ERR_INVALID_OPERATION. */
int tdt_dispatch_accumulate_masked(tdt_compute *c, int width, int height, int depth, int spp_begin, int spp_count,
                                   void *carry_device_ptr, const tdt_image *mask);
/* image = clamp(sqrt(sum / total_spp), 0, 1), alpha = 1: raytracer.comp:249-251 — EVERY covered pixel of the bound image, whatever its
 * alpha (a pixel no pass wrote resolves from the zeros or whatever the caller put there).  (Inside tdt_dispatch_compute, and only for a
 * frame whose miss pre-pass ran, the library's own resolve leaves the pixels that pass finished — alpha 1 — alone.) */
int tdt_dispatch_resolve(tdt_compute *c, int width, int height, int depth, int total_spp);
/* Instrumented dispatch (measurement only, slower): same image as tdt_dispatch_compute, and
 * returns event totals: [0] pixels written, [1] OctreeHit calls, [2] traversal iterations,
 * [3] Node loads (tree levels visited), [4] Lambertian, [5] metal, [6] dielectric scatters,
 * [7] hits on unknown material types.  Synchronous.  These define the algorithmic bytes. */
int tdt_dispatch_counted(tdt_compute *c, int width, int height, int depth, uint64_t counts[8]);
/* the same for one launch of a progressive frame: tdt_dispatch_accumulate(.., spp_begin, spp_count, carry), instrumented */
int tdt_dispatch_counted_range(tdt_compute *c, int width, int height, int depth, int spp_begin, int spp_count,
                               void *carry_device_ptr, uint64_t counts[8]);
/* Drop the per-pixel cost history of the context: the next tdt_dispatch_compute is scheduled like the first frame of a
 * context (two-phase, probe in image order) whatever was traced before.  Only the schedule changes, never a pixel.
 * (Measurement: bench.py times frames "the scheduler has not seen" with it.) */
int tdt_forget_costs(tdt_ctx *ctx);
/* measurement aid: enable != 0 records HIP events around the launches of every following tdt_dispatch_compute; ms (may be
 * NULL) receives the times of the LAST frame: {probe launch, main launch (+ the sort that orders it), resolve} for a
 * two-phase frame, {0, the one launch, 0} otherwise.  Blocks until that frame has finished. */
int tdt_debug_phase_timing(tdt_ctx *ctx, int enable, float ms[3]);
/* multi-device contexts: times of the last raytracer dispatch — trace_ms[i] for each device (its own events), then on the
 * first device gather_ms (from the end of ITS trace to the end of the gather: includes waiting for the slowest device) and
 * assemble_ms.  Blocks until the frame has finished. */
int tdt_debug_multi_timing(tdt_ctx *ctx, float *trace_ms /* n_devices */, float *gather_ms, float *assemble_ms);
/* which transport the last gather of a multi-device context used: "rccl", "copy", or "" */
const char *tdt_debug_multi_transport(const tdt_ctx *ctx);
/* ranks of the RCCL communicator the context really created (0: none — single-device context, or the copy transport) */
int tdt_debug_multi_rccl_ranks(const tdt_ctx *ctx);
/* test hook: the next raytracer dispatch of a multi-device context fails at device index `member` after the devices before
 * it were launched (-1: cancel) — exercises the drain-and-reset path of a half-launched frame */
int tdt_debug_multi_fail(tdt_ctx *ctx, int member);

/* ---- scene ingest on the GPU ------------------------------------------------------------------------
 * The step the reference never wrote (its call is commented out, main.rs:218-224): turn the voxel list its PLY loader
 * yields (ply_point_loader.rs:102-319: PlyFileContent{voxels, albedos, min_point}) into the indirect-cell octree
 * raytracer.comp reads.  Everything between the upload of the voxel list and the finished buffers runs in HIP kernels:
 * Morton keys (x, y, z bit of a level = one child digit, most significant level first) -> stable LSD radix sort ->
 * last-duplicate-wins unique -> per level, bottom-up, segment heads + prefix sum + 8-child reduce (uniform subtrees merge
 * into one LEAF) -> one prefix sum over the MIXED flags of all levels = breadth-first cell numbers -> node emission.
 * Byte-identical to the host builder (tdt_scene_from_ply / tdt_scene_generate in libtdthost.so). */
/* core: n voxels {x, y, z, material index + 1 (1..254)} in grid coordinates [0, 2^depth)^3 (others are dropped; of
 * duplicates the last wins) -> a new cells buffer of *n_cells cells (64 B each) on the context. */
int tdt_octree_build_cells(tdt_ctx *ctx, const int32_t *voxels_xyzm, size_t n_voxels, int depth, tdt_buffer **cells,
                           uint32_t *n_cells);
/* the whole of tdt_scene_from_ply on the GPU: voxels {x, y, z, colour key}, the loader's min_point and palette
 * (key -> r,g,b; n_palette entries in ascending key order).  Creates the seven buffers raytracer.comp reads and returns
 * them in out_slots[0,1,2,3,4,6,7] (out_slots[5] = NULL) WITHOUT binding them; *max_depth / *cell_count are what
 * OctreeInts holds (cell_count = the smallest power of two >= 1024 that holds the tree). */
int tdt_octree_build_from_points(tdt_ctx *ctx, const int32_t *voxels_xyzk, size_t n_voxels, const int32_t min_point[3],
                                 const uint32_t *palette_keys, const uint8_t *palette_rgb, size_t n_palette, int z_up,
                                 int max_iter, tdt_buffer *out_slots[8], int32_t *max_depth, int32_t *cell_count);

/* ---- voxel edits --------------------------------------------------------------------------------------
 * tdt_dispatch_compute of a TDT_PROGRAM_OCTREE_UPDATE program runs octree_update.comp's invocations.  The reference's
 * invocations race when their paths collide (its own comment, octree_update.comp:70-71); the defined result here is the
 * one its only runnable implementation produces — invocations one after the other, x fastest.  A dispatch of more than one
 * invocation is executed in parallel when that provably gives the same bytes: a planning pass walks every invocation's path
 * read-only, marks the nodes it would write, allocates the cells it needs by a prefix sum over the invocations (so each gets
 * the counter values the serial order would hand it), and checks that no invocation reads or writes a node another one
 * writes and that the cells to be allocated are untouched; then one lane per invocation applies its edit.  Any doubt
 * (collision, a walk that leaves the buffer, a non-empty node in the free pool) and the ordered one-lane walk runs instead
 * — decided on the device, no host round trip.  mode: 0 = as described, 1 = always the ordered walk. */
int tdt_debug_edit_mode(tdt_ctx *ctx, int mode);
/* which path the last edit dispatch of the context took: 0 none yet, 1 ordered walk, 2 parallel.  Synchronises. */
int tdt_debug_last_edit_path(tdt_ctx *ctx);
/* ---- ray queries ------------------------------------------------------------------------------------------------------
 * "What is under this pixel?": one query ray per lane through OctreeHit (raytracer.comp:397-450) exactly as the trace runs
 * it for a fresh invocation (zeroed loop-carried temporaries): root slab test with t_min = 0.0003, t_max = +inf, the
 * restart-from-root loop with its `adv` step, the in-octree test, the literal treeLookup, the padded empty-cell exit, and
 * the i > 0 leaf slab test — a pick answers with the bits the renderer traces for that pixel and sample.  Reads slots 0, 6
 * and 7 only; the image, the cost history, the hand-out order and the frame carry are left as they were.  Directions are
 * used as given: the shader's step `adv` is in units of t, so pass normalised directions.  A multi-device context answers
 * from device_ids[0] (device pointers must live there).  n == 0 is a no-op; NULL pointers with n > 0:
 * TDT_ERR_INVALID_VALUE; slots 0 / 6 / 7 unbound: TDT_ERR_INCOMPLETE. */
enum { TDT_RAY_MISS = 0, TDT_RAY_HIT = 1, TDT_RAY_ITER_LIMIT = 2 /* max_iter ran out inside the octree */ };
typedef struct tdt_ray_hit {
  int32_t  status;        /* TDT_RAY_MISS / TDT_RAY_HIT / TDT_RAY_ITER_LIMIT */
  uint32_t material;      /* leaf Node.value: index into slot 1 (hit only) */
  float    t;             /* t_enter of the CubeHit call whose record is returned (the root call site's when found on
                             iteration 0); 0 when that record is a zeroed temporary */
  int32_t  iterations;    /* OctreeHit loop iterations that reached treeLookup */
  float    point[3];      /* hit.point exactly as OctreeHit hands it back */
  float    normal[3];     /* hit.normal (oriented against the ray) */
  int32_t  front_face;
  int32_t  fresh_record;  /* 0: the call site's slab test missed, point / normal / front_face are the zeroed temporaries
                             a fresh invocation hands back (raytracer.comp:426-433) */
  float    cell_min[3];   /* leaf cube's lower corner, the shader's own expression grid_uv * scale + min_point */
  float    cell_size;     /* scale * inv_pow_depth */
} tdt_ray_hit;
#ifdef __cplusplus
static_assert(sizeof(tdt_ray_hit) == 64, "tdt_ray_hit is 64 bytes");
#else
_Static_assert(sizeof(tdt_ray_hit) == 64, "tdt_ray_hit is 64 bytes");
#endif
/* rays: n x {ox, oy, oz, dx, dy, dz} in host memory; synchronous (finishes the context's stream). */
int tdt_raycast(tdt_ctx *ctx, const float *rays, size_t n, tdt_ray_hit *out);
/* the same over device memory (n x 6 floats in, 4-byte aligned; n tdt_ray_hit out, 16-byte aligned), asynchronous on the
 * context's stream */
int tdt_raycast_device(tdt_ctx *ctx, const void *rays_dev, size_t n, void *hits_dev);
/* the primary ray of pixel (x, y) (xy: n pairs, non-negative), sample `sample` >= 0, from the program's camera uniforms
 * (raytracer.comp:240-245), traced as above; rays_out (n x 6 floats, may be NULL) receives the rays themselves.  Synchronous.
 * A TDT_PROGRAM_OCTREE_UPDATE program: TDT_ERR_INVALID_OPERATION. */
int tdt_pick_pixels(tdt_compute *c, const int32_t *xy, size_t n, int sample, float *rays_out, tdt_ray_hit *out);

/* ---- guide images and the denoiser -----------------------------------------------------------------------------------------
 * A low-spp frame is the library's noisiest output; these two calls trade a little bias for much less variance between
 * tdt_dispatch_accumulate and tdt_dispatch_resolve.  Every surface of a voxel scene is an axis-aligned face, so "same surface"
 * is an exact predicate — same material, same face direction, same plane — and the filter built on it is specified bit for bit.
 *
 * tdt_dispatch_guide: for every texel (x, y) of `guide` — any RGBA32F image of the context, of any size, addressed like the
 * trace's image (row 0 = bottom scan line); the camera uniforms define the rays, not the image — the primary ray of pixel (x, y)
 * and sample `sample` >= 0 is traced exactly as tdt_pick_pixels traces it.  Asynchronous on the context's stream.  Reads slots
 * 0, 6 and 7, and slot 1 unless TDT_GUIDE_ALL_MATERIALS is set; the bound image, the cost history, the hand-out order and the
 * frame carry are left as they were.  The texel's 16 bytes become four 32-bit words of that pixel's tdt_ray_hit `hit`
 * (struct tdt_guide_texel):
 *   kind      0 = pass-through, otherwise 1 + face code, face code = 9 s(nx) + 3 s(ny) + s(nz) over hit.normal with s(v) = 0
 *             for v < 0, 2 for v > 0, 1 otherwise (the normal may have more than one non-zero component)
 *   material  hit.material (0 when the ray did not end on a leaf)
 *   plane     hit.cell_min[a] + (hit.normal[a] > 0 ? hit.cell_size : 0.0f), one float add, a = the first of x, y, z whose normal
 *             component is non-zero; +0.0 when kind = 0
 *   t         hit.t: the depth image; not part of the key
 * kind is 0 when status != TDT_RAY_HIT, or fresh_record == 0, or all three normal components are zero, or —
 * TDT_GUIDE_ALL_MATERIALS clear — the material's entry in slot 1 (12 B per entry) does not lie inside the buffer or its first
 * word, `type`, is not 0 (Lambertian).  Pass-through exists because sky is noise-free already and reflections and refractions are
 * not smooth across a face: such pixels are not filtered.
 *
 * tdt_image_denoise: an a-trous wavelet filter over `img`, in place, asynchronous; B3 kernel k = {1/16, 1/4, 3/8, 1/4, 1/16};
 * pass p = 0 .. passes - 1 uses step s = 2^p and reads the whole output of the pass before it; passes 0..8, 0 = no-op; flags 0.
 * For pixel P = (x, y) of a pass, `in` being its input:
 *   guide[P].kind == 0: all four channels are copied bit for bit.
 *   otherwise: num = (0, 0, 0), den = 0; for j = -2..2 (outer), i = -2..2 (inner), Q = (x + i s, y + j s): the tap is SKIPPED
 *   (not multiplied by zero) when Q lies outside the image or words 0, 1, 2 of guide[Q] differ from those of guide[P]; a kept
 *   tap has w = k[j+2] * k[i+2] (exact in fp32), num.c = num.c + w * in[Q].c (a multiply, then an add: never fused), den = den + w;
 *   after the taps out.c = num.c / den (IEEE divide) for c = r, g, b, and alpha is in[P]'s.  The centre tap always matches, so
 *   den >= 9/64.
 * That order is the contract: a numpy model of these lines gives the same bits (NaN and inf propagate as the arithmetic says).
 * The filter does not care whether img holds running sums, means or a resolved frame; the intended use is accumulate, guide,
 * denoise, resolve — filter linear sums, then take the square root.  The passes ping-pong through a grow-only scratch image the
 * context owns and frees (one image; two for an odd number of three or more passes, so that the last pass lands in img; a single
 * pass is copied back).
 *
 * Errors, nothing written: NULL handles, sample < 0, unknown guide flags, passes outside 0..8, non-zero denoise flags, img and guide
 * of different sizes, the same image or sharing memory: TDT_ERR_INVALID_VALUE; tdt_dispatch_guide on a TDT_PROGRAM_OCTREE_UPDATE
 * program, a program whose partition is not (0, 1) (tile buffers are not images), an image of another context:
 * TDT_ERR_INVALID_OPERATION; slots 0, 6 or 7 unbound, or slot 1 unbound without TDT_GUIDE_ALL_MATERIALS: TDT_ERR_INCOMPLETE.  A
 * multi-device context runs both calls on device_ids[0], where the assembled image lives, as the queries do. */
#define TDT_GUIDE_ALL_MATERIALS 1u   /* key every hit, whatever its material: slot 1 is not read */
typedef struct tdt_guide_texel {
  uint32_t kind;          /* 0 = pass-through, otherwise 1 + face code */
  uint32_t material;      /* hit.material */
  float    plane;         /* the face's plane along its first normal axis */
  float    t;             /* hit.t */
} tdt_guide_texel;
#ifdef __cplusplus
static_assert(sizeof(tdt_guide_texel) == 16, "tdt_guide_texel is one RGBA32F texel");
#else
_Static_assert(sizeof(tdt_guide_texel) == 16, "tdt_guide_texel is one RGBA32F texel");
#endif
int tdt_dispatch_guide(tdt_compute *c, tdt_image *guide, int sample, uint32_t flags);
int tdt_image_denoise(tdt_image *img, const tdt_image *guide, int passes, uint32_t flags);

/* ---- temporal reprojection ------------------------------------------------------------------------------------------------
 * The filter above reduces variance within a frame; this call carries samples from one frame of a moving camera to the next.
 * It can be exact here: a ray from the old eye through a world point W on the plane of an axis-aligned face meets that plane only
 * at W, so if the old frame's pixel under W carries the same guide key (kind, material, plane), it saw W up to the pixel's
 * footprint.  History is validated by that bit-exact comparison and nothing else: no depth or normal tolerance.  The guide keys
 * only Lambertian hits by default, whose radiance does not depend on the view.
 *
 * A HISTORY IMAGE is an RGBA32F image whose rgb are running sums of radiance samples and whose alpha is the number of samples
 * behind them, as a float.  tdt_view is a snapshot of the camera uniforms primary_ray reads; tdt_compute_view fills one from the
 * program's current uniforms (a multi-device program: its first member's).
 *
 * tdt_image_reproject, asynchronous on the context's stream, one lane per pixel, reads no scene buffer:
 *   guide       what tdt_dispatch_guide(c, guide, sample, ..) wrote under c's CURRENT camera (the caller keeps them consistent)
 *   sums        this frame's running sums of `spp` samples as tdt_dispatch_accumulate leaves them; alpha is ignored
 *   prev_view, prev_guide, prev_hist   the view, guide and history of an earlier frame; all three NULL for a first frame.  The two
 *               images have one size, which may differ from the current one; prev_view defines the mapping (its image_width /
 *               image_height scale the jitter) independently of the images' sizes
 *   hist_out    receives this frame's history; mean_out (may be NULL) receives rgb = hist_out.rgb / hist_out.a, alpha = 1.
 *               mean_out may be `sums` itself (a lane reads only its own pixel of sums); it may not be any other argument.
 * Per call, on the host, in double from the fp32 fields of prev_view, every product and every add / subtract rounded on its own:
 *   a = horizontal, b = vertical, c = lower_left_corner - origin; Ru = b x c, Rv = c x a, Rw = a x b, each component as
 *   p = x*y; q = z*w; p - q; det = (c.z Rw.z + c.y Rw.y) + c.x Rw.x.  det not finite or 0: TDT_ERR_INVALID_VALUE.  det < 0: all three
 *   rows are negated.  The nine numbers are then rounded to fp32.
 * Per pixel P = (x, y), in fp32, each operation rounded, never fused:
 *   g = guide[P]; r = the primary ray of (x, y, sample) under c's camera (the bits of tdt_pick_pixels' rays_out).
 *   Without history, or with g.kind == 0: hist_out[P] = (sums.rgb, (float)spp).
 *   Otherwise W.k = r.o.k + g.t * r.d.k; D.k = W.k - prev.origin.k; nu = (Ru.z D.z + Ru.y D.y) + Ru.x D.x, nv and nw likewise with
 *   Rv and Rw; fx = (nu / nw) * (float)(prev.image_width - 1); fy = (nv / nw) * (float)(prev.image_height - 1).
 *   The history is FOUND iff nw > 0, and fx >= 0 && fx < (float)prev_w && fy >= 0 && fy < (float)prev_h (prev_w, prev_h: the size
 *   of the prev images; NaN fails), and with Q = ((int)fx, (int)fy) words 0, 1, 2 of prev_guide[Q] equal those of g, and
 *   hn = prev_hist[Q].a satisfies hn > 0.  prev_hist[Q] is read only after the key matched.
 *   Found: h = prev_hist[Q]; if hn > max_samples: s = max_samples / hn, h.rgb = h.rgb * s, hn = max_samples;
 *   hist_out[P] = (sums.rgb + h.rgb, (float)spp + hn).  Not found: as without history.
 * max_samples caps the history's length: once it is reached, what enters is an exponential moving average.
 * The intended frame k: accumulate [k spp, (k+1) spp) into the bound image, guide with sample = k spp, reproject with mean_out =
 * the bound image, optionally tdt_image_denoise, tdt_dispatch_resolve(.., total_spp = 1) (the divide by 1 is exact); the history
 * and guide images ping-pong between frames.  A range that does not start at sample 0 is ADDED to what the bound image holds, which
 * after a frame is the resolved picture: tdt_image_clear (all bytes of the image to zero, asynchronous on the context's stream; a
 * NULL image: TDT_ERR_INVALID_VALUE) comes before the accumulate of every frame but the first.  An image of a multi-device
 * context: TDT_ERR_INVALID_OPERATION, nothing written (there a bound image's running sums live in the members' tile buffers, out
 * of this handle's reach; the frame above is a single-device one).
 *
 * tdt_debug_reproject_counts (synchronises): of the context's last tdt_image_reproject that returned TDT_OK (a call that fails
 * leaves the counts of the call before it), [0] keyed pixels (kind != 0), [1] found, [2] rejected by key or hn, [3] rejected by nw
 * or off-screen; [1] + [2] + [3] = [0] when history was given, else they are 0.  Before any call, and after one on an image of no
 * pixels, all four are 0.
 *
 * Errors, nothing written: NULL c, guide, sums or hist_out; prev_* neither all NULL nor all non-NULL; sample < 0; spp < 1; flags
 * != 0; max_samples not >= 1 (NaN included); guide, sums, hist_out and mean_out not of one size; prev_guide and prev_hist of
 * different sizes, or wider or taller than 2^24 (past which (float)prev_w is no longer exact); a view with image_width < 2 or
 * image_height < 2, or a degenerate determinant; any two images sharing memory except mean_out == sums: TDT_ERR_INVALID_VALUE.
 * A TDT_PROGRAM_OCTREE_UPDATE program, a partition other than (0, 1), an image of another context: TDT_ERR_INVALID_OPERATION.
 * A multi-device context runs on device_ids[0]. */
typedef struct tdt_view {
  float   origin[3], lower_left_corner[3], horizontal[3], vertical[3];
  int32_t image_width, image_height;
} tdt_view;
#ifdef __cplusplus
static_assert(sizeof(tdt_view) == 56, "tdt_view is 56 bytes");
#else
_Static_assert(sizeof(tdt_view) == 56, "tdt_view is 56 bytes");
#endif
int tdt_compute_view(const tdt_compute *c, tdt_view *out);
int tdt_image_reproject(tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp,
                        const tdt_view *prev_view, const tdt_image *prev_guide, const tdt_image *prev_hist,
                        float max_samples, tdt_image *hist_out, tdt_image *mean_out, uint32_t flags);
int tdt_debug_reproject_counts(tdt_ctx *ctx, uint64_t out[4]);
int tdt_image_clear(tdt_image *img);

/* ---- luminance variance and the variance-guided filter --------------------------------------------------------------------
 * tdt_image_denoise stops at surface edges and nowhere else: inside a face every same-key neighbour counts in full, however
 * different its radiance.  These three calls add what tells a lighting edge from noise: a per-pixel estimate of the variance of
 * the luminance, and a filter whose second edge-stopping weight is scaled by it.  The variance lives in the image's ALPHA channel,
 * which neither tdt_image_denoise nor the resolve uses (tdt_dispatch_resolve overwrites it with 1), so a tap is still one texel.
 * Throughout lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b; all arithmetic is fp32, each operation rounded on its own,
 * never fused; "same key" and "inside the image" are tdt_image_denoise's, and a tap that fails them is SKIPPED, not weighted by
 * zero.  A numpy model of these lines gives the same bits.
 *
 * tdt_image_variance, asynchronous on the context's stream: writes img[P].a for every pixel P = (x, y) and nothing else (the alpha
 * word alone is stored, and rgb alone is loaded); moments may be NULL.
 *   guide[P].kind == 0: a = +0.0f.
 *   Temporal estimate, when moments != NULL and n = moments[P].z satisfies n >= min_frames (NaN fails): mu = m.x / n; e2 = m.y / n;
 *   v = e2 - mu * mu; v = v > 0 ? v : 0 (a NaN gives 0); a = v / n — the variance of the mean of n frames, which is what img holds
 *   in the temporal frame.
 *   Spatial estimate otherwise: K = 0, s1 = 0, s2 = 0; for j = -3..3 (outer), i = -3..3 (inner), Q = (x + i, y + j) inside the image
 *   with the same key: l = lum(img[Q].rgb); K = K + 1.0f; s1 = s1 + l; s2 = s2 + l * l.  Then mu = s1 / K; v = s2 / K - mu * mu;
 *   v = v > 0 ? v : 0; a = v.  The centre always counts, so K >= 1; with K == 1 the variance is 0.
 *
 * tdt_image_denoise_variance: tdt_image_denoise's a-trous frame — the B3 kernel k, step s = 2^p in pass p, passes 0..8 (0 = no-op),
 * the same scratch images, the last pass lands in img — with a luminance weight.  Once, on the host: s2 = sigma * sigma.
 * For pixel P of a pass, `in` being its input:
 *   guide[P].kind == 0: all four channels are copied bit for bit.
 *   otherwise lP = lum(in[P].rgb), and the prefiltered variance, always at distance 1 whatever the step, with g = {1/4, 1/2, 1/4}:
 *   gnum = 0, gden = 0; for j = -1..1 (outer), i = -1..1 (inner), Q = (x + i, y + j) inside the image with the same key:
 *   wg = g[j+1] * g[i+1]; gnum = gnum + wg * in[Q].a; gden = gden + wg.  gv = gnum / gden; lim = s2 * gv + floor.
 *   If !(lim > 0 && lim < INFINITY): all four channels of in[P] are copied bit for bit — a pixel whose variance is unknown or
 *   zero is left alone.
 *   Otherwise num = (0, 0, 0), den = 0, vnum = 0; for j = -2..2 (outer), i = -2..2 (inner), Q = (x + i s, y + j s): skipped when Q
 *   lies outside the image or its key differs; d = lum(in[Q].rgb) - lP; d2 = d * d; skipped unless d2 < lim (a comparison: NaN
 *   fails); w = (k[j+2] * k[i+2]) * (lim - d2); num.c = num.c + w * in[Q].c for c = r, g, b; den = den + w;
 *   vnum = vnum + (w * w) * in[Q].a.  After the taps out.c = num.c / den; out.a = vnum / (den * den).
 * The luminance weight is max(lim - d2, 0), compactly supported; its normalising 1 / lim is common to all taps and cancels.  NaN and
 * infinities propagate as these lines say: a NaN centre keeps no tap, den = 0, and the output is NaN.
 *
 * A MOMENTS IMAGE is an RGBA32F image whose texels are (m1, m2, n, 0): the sums over frames of the frame's luminance and of its
 * square, and the number of frames.  tdt_image_reproject_moments is tdt_image_reproject — hist_out, mean_out, the four counts, the
 * FOUND predicate and Q are exactly that call's — and also writes moments_out.  Once, on the host: mf = max_samples / (float)spp.
 * Per pixel: l = lum(sums.rgb / (float)spp), three IEEE divides, then lum.
 *   Not found, no history, or kind == 0: moments_out[P] = (l, l * l, 1, 0).
 *   Found: hm = prev_moments[Q], read only after the key matched and hn > 0.  If !(hm.z > 0): as not found.  If hm.z > mf:
 *   sc = mf / hm.z; hm.x = hm.x * sc; hm.y = hm.y * sc; hm.z = mf.  moments_out[P] = (l + hm.x, l * l + hm.y, 1.0f + hm.z, 0).
 * prev_moments is NULL exactly when the other prev_* are, and has their size.
 * The intended frames: accumulate, guide, tdt_image_variance (spatial), tdt_image_denoise_variance, resolve; and, temporal,
 * clear, accumulate, guide, tdt_image_reproject_moments with mean_out = the bound image, tdt_image_variance with moments_out,
 * tdt_image_denoise_variance, resolve with total_spp = 1; the moments images ping-pong like the histories.
 *
 * Errors, nothing written: NULL handles (moments of tdt_image_variance and mean_out excepted); images not of one size; any two
 * images sharing memory except mean_out == sums; passes outside 0..8; flags != 0; sigma not > 0 or not finite; floor not >= 0 or not
 * finite; min_frames not >= 1 (NaN included); whatever tdt_image_reproject refuses: TDT_ERR_INVALID_VALUE.  An image of another
 * context; for tdt_image_reproject_moments a TDT_PROGRAM_OCTREE_UPDATE program or a partition other than (0, 1):
 * TDT_ERR_INVALID_OPERATION.  A multi-device context runs all three on device_ids[0]. */
int tdt_image_variance(tdt_image *img, const tdt_image *guide, const tdt_image *moments, float min_frames, uint32_t flags);
int tdt_image_denoise_variance(tdt_image *img, const tdt_image *guide, int passes, float sigma, float floor, uint32_t flags);
int tdt_image_reproject_moments(tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp,
                                const tdt_view *prev_view, const tdt_image *prev_guide, const tdt_image *prev_hist,
                                const tdt_image *prev_moments, float max_samples, tdt_image *hist_out, tdt_image *moments_out,
                                tdt_image *mean_out, uint32_t flags);

/* ---- guide-keyed upsampling ------------------------------------------------------------------------------------------------
 * A first-hit guide costs a tenth of a low-spp trace, so the geometry of a frame is nearly free at full resolution and only its
 * radiance is expensive.  tdt_image_upsample spreads sums traced at reduced resolution — an ordinary tdt_dispatch_accumulate under
 * a camera whose image_width / image_height are smaller, into an image of that size — over a full-resolution image, and the
 * guide key (kind, material, plane) of the two resolutions keeps radiance from crossing a face edge: exact, no depth or normal
 * tolerance.  The result is a sums image that tdt_image_denoise, tdt_image_variance, tdt_image_reproject and tdt_dispatch_resolve
 * take unchanged.
 *
 * tdt_image_upsample, asynchronous on the context's stream, one lane per pixel of dst, reads no scene buffer and no camera:
 *   dst, dst_guide   W x H: the image to write and what tdt_dispatch_guide wrote under the full-resolution camera
 *   src, src_guide   w x h, 1 <= w <= W, 1 <= h <= H, every side <= 32768: the low-resolution sums and the guide of the SAME
 *                    sample under the low-resolution camera (the same frustum; the caller keeps them consistent).  W / w need
 *                    not be an integer, nor equal H / h.
 * "Same key" is tdt_image_denoise's: words 0, 1, 2 of two guide texels are equal.  A kind-0 texel is treated like any other:
 * sky interpolates among sky, a pass-through hit among pass-through hits of its material.
 * The mapping, in exact integers, per axis.  primary_ray samples pixel x at (x + jitter) / (image_width - 1), so pixel x of the full
 * frame lies at x (w - 1) / (W - 1) of the low one.  W == 1: i0 = 0, fx = 0.  Otherwise n = x (w - 1); i0 = n / (W - 1) (the integer
 * floor); r = n % (W - 1); fx = (float)r / (float)(W - 1) (an IEEE divide).  i1 = min(i0 + 1, w - 1).  The nearest texel `in` is i0
 * when 2 r < W - 1, else i1.  Likewise for y with H, h: j0, j1, fy, jn.
 * Per pixel P = (x, y), g = dst_guide[P], all in fp32, each operation rounded on its own, never fused:
 *   Stage 1, validated bilinear.  num = (0, 0, 0, 0), den = 0; wx = {1.0f - fx, fx}, wy = {1.0f - fy, fy}; for the taps
 *   Q = (i0, j0), (i1, j0), (i0, j1), (i1, j1) in that order: wt = wy * wx; the tap is SKIPPED unless wt > 0 (so a zero-weight tap
 *   never contributes, which covers the clamped i1 == i0) and skipped when the key of src_guide[Q] differs from g's; src[Q] is
 *   read only after the key matched.  A kept tap: num.c = num.c + wt * src[Q].c for c = r, g, b, a, then den = den + wt.
 *   If den > 0: dst[P].c = num.c / den (IEEE divide): class 1.
 *   Stage 2, the ring, only if den == 0 (num is still zero).  K = 0; for j = j0 - 1 .. j0 + 2 (outer), i = i0 - 1 .. i0 + 2 (inner),
 *   Q = (i, j) inside src with the same key: num.c = num.c + src[Q].c, then K = K + 1.0f.  If K > 0: dst[P].c = num.c / K: class 2.
 *   Stage 3, a hole: no texel of the 4x4 neighbourhood saw this surface.  dst[P] = src[(in, jn)] bit for bit: class 3.
 * All four channels are interpolated alike, so alpha carries whatever the caller keeps there (a variance, a sample count); running
 * sums of `spp` samples come out as running sums of `spp` samples.  Stage 1 starts from +0, so with equal sizes and equal guides
 * the call returns src bit for bit except that -0 comes back as +0 (and a NaN as the NaN the divide by 1 gives).  That order is
 * the contract: a numpy model of these lines gives the same bits.
 * A hole is what sub-pixel geometry gives: where a low-resolution texel covers several faces, most full-resolution pixels find
 * their face in none of the sixteen texels around them, and the call degrades to nearest-texel magnification there.
 *
 * tdt_debug_upsample_counts (synchronises): of the context's last tdt_image_upsample that returned TDT_OK (a call that fails leaves
 * the counts of the call before it), [0] pixels of dst, [1], [2], [3] the pixels of class 1, 2, 3; [1] + [2] + [3] = [0].  Before
 * any call all four are 0.
 *
 * Errors, nothing written: a NULL handle; flags != 0; dst and dst_guide of different sizes; src and src_guide of different sizes;
 * src wider or taller than dst; a side above 32768 (x (w - 1) then fits 32 bits); any two of the four images the same or sharing
 * memory: TDT_ERR_INVALID_VALUE.  An image of another context: TDT_ERR_INVALID_OPERATION.  A multi-device context runs the call on
 * device_ids[0], as tdt_image_denoise does. */
int tdt_image_upsample(tdt_image *dst, const tdt_image *dst_guide, const tdt_image *src, const tdt_image *src_guide, uint32_t flags);
int tdt_debug_upsample_counts(tdt_ctx *ctx, uint64_t out[4]);

/* ---- adaptive sampling: the sampling controller ------------------------------------------------------------------------------
 * tdt_dispatch_accumulate_masked traces a batch of samples for the live pixels of a mask; these calls decide, after each batch,
 * which pixels stay live.  The decision is the classic batch-means test: the variance of the means of the batches a pixel has
 * received estimates the error of its running mean, and the pixel stops when that error is below a fraction of its brightness.
 *
 * A STATE IMAGE is an RGBA32F image whose texels are (L, m2, n, w): L the luminance of the running sums at the last update, m2 the
 * sum of the squared batch luminances, n the number of batches, |w| the number of samples behind the pixel.  A pixel HAS STOPPED
 * when !(w >= 0.0f): w < 0, or a NaN.  That is exactly "not live" in tdt_dispatch_accumulate_masked, so a state image is a mask,
 * and a cleared image (tdt_image_clear) is "every pixel live, nothing traced".  Throughout lum(c) = (0.2126f * c.r + 0.7152f * c.g)
 * + 0.0722f * c.b; all arithmetic is fp32, each operation rounded on its own, never fused.  A numpy model of these lines gives the
 * same bits, with one exception: where a line computes a NaN, the result is a NaN whose sign and payload are not specified (a
 * texel that is copied keeps its bits, NaN or not).
 *
 * tdt_image_adapt, asynchronous on the context's stream, after a batch of k = spp_count samples was added to `sums` for the live
 * pixels of state_in.  Once, on the host: kf = (float)k, lo = (float)a->min_samples, hi = (float)a->max_samples.  Per pixel P with
 * st = state_in[P]:
 *   P has stopped: state_out[P] = st bit for bit, and P PASSES.
 *   Otherwise the update: Lc = lum(sums[P].rgb); lb = (Lc - st.L) / kf; m2' = st.m2 + lb * lb; n' = st.n + 1.0f; s' = st.w + kf;
 *   mean = Lc / s'; v = m2' / n' - mean * mean; var = v < 0 ? 0 : v (a NaN stays a NaN); err2 = var / n';
 *   mx = mean > a->floor ? mean : a->floor (a NaN mean gives floor); thr = a->tolerance * mx; thr2 = thr * thr.
 *   P is CAPPED when s' >= hi, and then PASSES.  Otherwise P passes when s' >= lo && n' >= 2.0f && err2 <= thr2: comparisons, which
 *   a NaN fails, so a pixel whose sums are not finite runs to the cap.
 *   The stop.  guide == NULL: P stops when it passes.  With a guide (what tdt_dispatch_guide wrote for sample 0 of the frame): a
 *   capped P stops; any other P stops when it passes AND every texel Q of its 3x3 neighbourhood that lies inside the image and has
 *   the same key (tdt_image_denoise's: words 0, 1, 2 of the two guide texels are equal; a kind-0 texel is treated like any other)
 *   passes, Q's test being evaluated from state_in and sums as above, never from state_out.  So a pixel whose few batches happened
 *   to agree does not stop next to pixels of its own face that are still noisy; neighbours that stopped earlier or are capped do
 *   not hold it back.
 *   state_out[P] = (Lc, m2', n', stopped ? -s' : s').
 * state_in and state_out are distinct images that ping-pong, as the history images of tdt_image_reproject do.  Batch-mean variance
 * needs two batches: nothing stops before its second update unless it is capped.
 *
 * tdt_debug_adapt_counts (synchronises): of the context's last tdt_image_adapt that returned TDT_OK, [0] the pixels that had not
 * stopped in state_in, [1] those of them stopped by the tolerance, [2] stopped by the cap, [3] still live;
 * [1] + [2] + [3] = [0].  Before any call all four are 0.
 *
 * tdt_image_adapt_mean, asynchronous: img holds the running sums the state describes.  Per pixel, aw = |state[P].w|.  aw == 0:
 * nothing is written.  Otherwise img[P].c = img[P].c / aw for c = r, g, b (IEEE divides), and img[P].a = the variance of the mean
 * luminance: n >= 2.0f (NaN fails): mean = L / aw; v = m2 / n - mean * mean; v = v > 0 ? v : 0 (a NaN gives 0); a = v / n; else
 * a = +0.0f.  The result is the kind of image tdt_image_reproject's mean_out is: tdt_image_denoise, tdt_image_denoise_variance (the
 * alpha is its variance) and tdt_dispatch_resolve with total_spp = 1 take it unchanged.
 *
 * The intended frame: clear the bound image and a state image; then repeat { tdt_dispatch_accumulate_masked(begin, k, carry,
 * state); tdt_image_adapt(image, guide, state, other state, k, ..); swap the states; begin += k } until count [3] is 0; then
 * tdt_image_adapt_mean, the filter, the resolve.  Masks only shrink, so every pixel holds a prefix [0, n_P) of the sample
 * sequence and begin is the same for all live pixels.  Reading the counts is a host synchronisation per round.
 *
 * Errors, nothing written: a NULL handle (guide excepted) or a NULL a; flags != 0; spp_count outside 1..2^24; tolerance or floor
 * negative or not finite; min_samples outside 0..2^24; max_samples outside 1..2^24; images not of one size; any two of the images
 * the same or sharing memory: TDT_ERR_INVALID_VALUE.  An image of another context; a multi-device context:
 * TDT_ERR_INVALID_OPERATION. */
typedef struct tdt_adapt {
  float   tolerance;           /* relative error of the mean luminance at which a pixel stops */
  float   floor;               /* the brightness below which the error is measured against `floor` itself */
  int32_t min_samples;         /* no pixel stops by the tolerance with fewer samples */
  int32_t max_samples;         /* the cap: a pixel with this many samples stops */
} tdt_adapt;
int tdt_image_adapt(const tdt_image *sums, const tdt_image *guide /* may be NULL */, const tdt_image *state_in, tdt_image *state_out,
                    int spp_count, const tdt_adapt *a, uint32_t flags);
int tdt_debug_adapt_counts(tdt_ctx *ctx, uint64_t out[4]);
int tdt_image_adapt_mean(tdt_image *img, const tdt_image *state, uint32_t flags);

/* ---- screen-space selection: voxel-id images, overlays, marquee ---------------------------------------------------------------
 * The editing calls below produce Morton-sorted voxel lists, the image calls above work on RGBA32F images keyed by each pixel's
 * first hit; these calls join the two.  The one primitive is a VOXEL-ID IMAGE: per pixel, the grid voxel a click on that pixel
 * would act on.  Membership of that voxel in a list gives an overlay (a tdt_octree_extract_* preview drawn into a frame), the
 * distinct ids of a rectangle give a marquee selection (the brush of tdt_octree_edit_voxels).  The id image depends on camera
 * and tree only: a brush that is dragged re-runs only the overlay.  First hit only: occluded voxels of a list are not shown, and
 * with place == 1 only empty cells adjacent to a visible face have a pixel.
 *
 * tdt_dispatch_voxel_ids: for every texel (x, y) of `ids` — any RGBA32F image of the context, of any size; the camera uniforms
 * define the rays, not the image — the primary ray of pixel (x, y) and sample `sample` >= 0 is traced exactly as
 * tdt_dispatch_guide traces it: one lane per texel, 16x16 ray tiles.  Asynchronous on the context's stream.  Reads slots 0, 6 and
 * 7 only; the bound image, the cost history, the hand-out order and the frame carry are left as they were.  The texel receives the
 * voxel tdt_pick_grid_voxel(hit, floats, ints, place) returns for that pixel's tdt_pick_pixels record `hit`, computed in fp64 on the
 * device.  For each axis a: q = ((double)point[a] - (double)min[a]) / (double)scale + side * (double)normal[a] * half, where
 * half = 0.5 / 2^depth, side is +1 for place == 1 (the empty cell in front of the face) and -1 for place == 0 (the voxel behind
 * it); k[a] = floor(q * 2^depth).  The voxel is valid when 0 <= k[a] < 2^depth on all three axes.  Products by +-1 and by powers
 * of two are exact, so the only roundings are the subtraction, the divide and the add, each a correctly rounded fp64 operation.
 * tdt_pick_grid_voxel (tdt_host.h) stays the single statement of this arithmetic that tests compare against.  The texel's 16 bytes
 * (struct tdt_voxel_id_texel):
 *   state     1 when status == TDT_RAY_HIT, fresh_record != 0 and the voxel is valid, otherwise 0: exactly when tdt_pick_grid_voxel
 *             succeeds
 *   key       the voxel's Morton key, spread3(x) << 2 | spread3(y) << 1 | spread3(z) in tdt_octree_extract's order; 0 when
 *             state == 0
 *   material  hit.material, as the guide's word
 *   t         the bits of hit.t, as the guide's word
 * Errors, nothing written: NULL handles, sample < 0, place not 0 or 1: TDT_ERR_INVALID_VALUE; a TDT_PROGRAM_OCTREE_UPDATE program,
 * a partition other than (0, 1), an image of another context: TDT_ERR_INVALID_OPERATION; slots 0, 6 or 7 unbound:
 * TDT_ERR_INCOMPLETE; max_depth outside 1..10 (the key must fit 30 bits) or a scale that is not positive and finite:
 * TDT_ERR_INVALID_VALUE.  A multi-device context runs on device_ids[0].
 *
 * tdt_image_overlay: tints, in place over `img`, the pixels whose voxel is in a list.  `ids` has img's size and shares no memory
 * with it.  voxels_xyzm is a host array of n x {x, y, z, m} as tdt_octree_edit_voxels takes it with TDT_REGION_CLEAR: m is
 * ignored, the order is arbitrary, duplicates are allowed, voxels with a coordinate outside [0, 1024) are dropped.  n == 0: the
 * list is empty and img is unchanged, bit for bit.  The list is uploaded before the call returns (one synchronisation of the
 * stream; the host array may be freed on return); keys, sort, unique and the pass itself are queued.  For pixel P:
 *   member(P): ids[P].state == 1 and ids[P].key is in the list.
 *   edge(P): member(P), edge_width >= 1, and some Q != P inside the image with max(|dx|, |dy|) <= edge_width satisfies one of:
 *   !member(Q); TDT_OVERLAY_VOXEL_EDGES is set, and ids[Q].state != 1 or ids[Q].key != ids[P].key.  Pixels outside the image
 *   are not consulted.
 *   A non-member pixel keeps all four channels bit for bit.  A member pixel takes col = edge(P) ? style->edge : style->fill and
 *   a = col[3]; out.c = (in.c * (1.0f - a)) + (col.c * a) for c = r, g, b: one subtract, two multiplies and one add, each rounded
 *   on its own (NaN and inf propagate as the arithmetic says); alpha is in's.
 * The intended use is on a resolved frame.  A numpy model of these lines gives the same bits, with one exception: where a line
 * computes a NaN (inf * 0 with a = 1, inf - inf, an operation on a NaN), the result is a NaN whose sign and payload are not
 * specified (IEEE 754 leaves them open); a channel that is copied keeps its bits, NaN or not.
 *
 * tdt_debug_overlay_counts (synchronises): of the context's last tdt_image_overlay that returned TDT_OK (a call that fails leaves
 * the counts of the call before it), [0] pixels, [1] state == 1 pixels, [2] member pixels, [3] edge pixels.  Before any call all
 * four are 0.
 *
 * Errors, nothing written: NULL img, ids or style, a NULL list with n > 0, edge_width outside 0..4, unknown flags, n above the
 * voxel-list cap (TDT_REGION_BRUSH_CAP), img and ids of different sizes, the same image or sharing memory: TDT_ERR_INVALID_VALUE;
 * an image of another context: TDT_ERR_INVALID_OPERATION.  A multi-device context runs on device_ids[0].
 *
 * tdt_image_extract_voxels: the distinct voxels of the state == 1 texels inside rect = {x0, y0, x1, y1}, inclusive, clipped to
 * the image; NULL means the whole image; an empty rect after clipping, or x0 > x1 (or y0 > y1), gives 0 voxels.  The output is
 * {x, y, z, material + 1}, Morton-sorted, by tdt_octree_extract's rules: voxels_xyzm == NULL: only the count; capacity < the
 * count: TDT_ERR_INVALID_VALUE, *n_voxels still set, nothing written.  Where several texels carry one key with different
 * materials (possible only for place == 1 ids), the last texel in row-major order wins: the stable sort and last-of-run rule of
 * tdt_octree_build_cells.  A selected texel with material >= 254, or a rect of more than TDT_REGION_BRUSH_CAP texels:
 * TDT_ERR_INVALID_VALUE, nothing written.  NULL ids or n_voxels: TDT_ERR_INVALID_VALUE.  Synchronous.  The result is the brush of
 * tdt_octree_edit_voxels: marquee paint or clear is extract followed by edit. */
#define TDT_OVERLAY_VOXEL_EDGES 1u   /* outline every voxel of the selection, not only the selection's silhouette */
typedef struct tdt_voxel_id_texel {
  uint32_t state;         /* 1 = tdt_pick_grid_voxel succeeds for this pixel, else 0 */
  uint32_t key;           /* the voxel's Morton key; 0 when state == 0 */
  uint32_t material;      /* hit.material */
  uint32_t t;             /* the bits of hit.t */
} tdt_voxel_id_texel;
typedef struct tdt_overlay {
  float    fill[4];       /* r, g, b, a for member pixels */
  float    edge[4];       /* r, g, b, a for edge pixels */
  int32_t  edge_width;    /* 0..4 pixels; 0 = no outline */
  uint32_t flags;         /* TDT_OVERLAY_VOXEL_EDGES */
} tdt_overlay;
#ifdef __cplusplus
static_assert(sizeof(tdt_voxel_id_texel) == 16, "tdt_voxel_id_texel is one RGBA32F texel");
static_assert(sizeof(tdt_overlay) == 40, "tdt_overlay is 40 bytes");
#else
_Static_assert(sizeof(tdt_voxel_id_texel) == 16, "tdt_voxel_id_texel is one RGBA32F texel");
_Static_assert(sizeof(tdt_overlay) == 40, "tdt_overlay is 40 bytes");
#endif
int tdt_dispatch_voxel_ids(tdt_compute *c, tdt_image *ids, int place, int sample);
int tdt_image_overlay(tdt_image *img, const tdt_image *ids, const int32_t *voxels_xyzm, size_t n, const tdt_overlay *style);
int tdt_debug_overlay_counts(tdt_ctx *ctx, uint64_t out[4]);
int tdt_image_extract_voxels(const tdt_image *ids, const int32_t rect[4], int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);

/* ---- through-selection ----------------------------------------------------------------------------------------------------
 * The other marquee of an editor: "select everything inside this lasso", "delete all glass behind this rectangle".  Screen-space
 * selection above is first hit only; this is a test per voxel, not per pixel: every voxel of the tree's list V is projected into a
 * view and selected when it lands inside a screen shape, whether something hides it or not.  No occlusion test (that is
 * tdt_image_extract_voxels), no hierarchical culling (the call walks the whole tree, as every list-based unit does), and only the
 * centre or all eight corners are tested: a "crossing" marquee, a voxel that merely touches the shape, is not built.
 *
 * World points.  For voxel k at depth d = max_depth, min and scale come from slot 6, read as tdt_pick_grid_voxel reads them
 * (floats[0..2], floats[4]).  The centre is u[a] = (2 k[a] + 1) * 2^-(d+1); a corner is (k[a] + c) * 2^-d with c in {0, 1}; both are
 * exact in fp32.  w[a] = (u[a] * scale) + min[a]: two rounded fp32 operations, never fused.
 * Projection.  It is exactly tdt_image_reproject's Q, one function on the device: D = w - view.origin; Ru, Rv, Rw from the view as
 * that call computes them per call; nu = (Ru.z D.z + Ru.y D.y) + Ru.x D.x, nv and nw likewise with Rv and Rw;
 * fx = (nu / nw) * (float)(image_width - 1); fy = (nv / nw) * (float)(image_height - 1).  Every operation is rounded, none fused.
 * A point is in front and on screen when nw > 0 && fx >= 0 && fx < (float)image_width && fy >= 0 && fy < (float)image_height; its
 * pixel is (px, py) = ((int)fx, (int)fy).  Only comparisons consume fx and fy, so a NaN (a point at the eye) simply fails.
 * Shape tests on (px, py):
 *   TDT_SCREEN_RECT     x0 <= px <= x1 && y0 <= py <= y1 with rect = {x0, y0, x1, y1}, inclusive, as tdt_image_extract_voxels'
 *                       rect; x0 > x1 or y0 > y1 selects nothing.
 *   TDT_SCREEN_POLYGON  polygon_xy holds n_vertices (3..256) pairs x, y, each |coordinate| <= 2^20.  The even-odd rule at the
 *                       pixel centre, in integers on doubled coordinates: P = (2px+1, 2py+1), A = 2a, B = 2b for each edge a -> b,
 *                       closing the last vertex to the first.  An edge counts when (Ay > Py) != (By > Py) and P is strictly left
 *                       of its crossing: in int64, s = (Px-Ax)*(By-Ay) - (Bx-Ax)*(Py-Ay), and the edge counts when
 *                       (By > Ay) ? s < 0 : s > 0.  Py is odd and vertex rows are even, so no vertex lies on the scan line.  The
 *                       pixel is inside when the count is odd.  The polygon (x0,y0), (x1+1,y0), (x1+1,y1+1), (x0,y1+1) is the
 *                       RECT x0..x1, y0..y1.
 *   TDT_SCREEN_MASK     mask is an RGBA32F image of the context of exactly image_width x image_height; the pixel is inside when
 *                       mask[py][px].x > 0.0f (NaN and -0 are outside).
 * Selection.  Without TDT_SCREEN_WINDOW the tested point is the centre.  With it all eight corners must pass the front / screen
 * test and the shape test, and the centre is not tested: the voxel lies entirely inside a convex shape.  Then
 * material < 0 || voxel material == material.  Then min_distance*min_distance <= dd && dd <= max_distance*max_distance with
 * dd = (D.z*D.z + D.y*D.y) + D.x*D.x of the centre; both squares are rounded fp32 products.  An unused polygon_xy or mask is ignored.
 * As with a pick, the selection is not always what one sees: a voxel whose centre projects onto the border between two pixels falls
 * on the side the fp32 arithmetic above puts it, and a voxel hidden behind others is selected like a visible one.
 *
 * tdt_octree_extract_screen follows tdt_octree_extract_region's rules: the selected voxels as {x, y, z, material + 1},
 * Morton-sorted; voxels_xyzm == NULL only counts; capacity < the count: TDT_ERR_INVALID_VALUE with *n_voxels set.  Synchronous.  A
 * multi-device context answers from device_ids[0].
 * tdt_octree_edit_screen: op TDT_REGION_PAINT (every selected voxel gets `material`, 0..253) or TDT_REGION_CLEAR (removed); the
 * selection is a subset of V, so SET would equal PAINT and FILL would be empty: both are TDT_ERR_INVALID_VALUE.  The list never
 * leaves the device; the tree is left canonical, as for every region edit, on every replica.  Synchronous.
 * tdt_debug_screen_counts (synchronises): of the context's last of these two calls that returned TDT_OK (a failing call leaves
 * them unchanged), [0] voxels of V, [1] voxels whose tested points are all in front and on screen, [2] of those, the voxels
 * inside the shape, [3] voxels selected, after material and distance.  Before any call all four are 0.
 *
 * Errors, nothing written and nothing queued: NULL ctx, view, sel or n_voxels; a shape outside the enum; unknown flag bits; a
 * filter material outside -1..253 (edit: `material` outside 0..253, an op other than PAINT / CLEAR); a distance that is NaN or
 * negative, or min_distance > max_distance; POLYGON with NULL vertices, a count outside 3..256 or a coordinate beyond +-2^20; MASK
 * with a NULL image or an image of another size; image_width or image_height < 2 or above 2^24 (past which (float)image_width is
 * no longer exact); a degenerate view (tdt_image_reproject's determinant); max_depth outside 1..10; a scale that is not positive
 * and finite; |V| above 2^26 (TDT_REGION_BRUSH_CAP): TDT_ERR_INVALID_VALUE.  A mask of another context, or a MASK edit on a
 * multi-device context (the mask lives on device_ids[0] only; RECT and POLYGON edit every replica): TDT_ERR_INVALID_OPERATION.
 * Slots 0, 6 or 7 unbound: TDT_ERR_INCOMPLETE. */
enum { TDT_SCREEN_RECT = 0, TDT_SCREEN_POLYGON = 1, TDT_SCREEN_MASK = 2 };
#define TDT_SCREEN_WINDOW 1u          /* all eight corners of the voxel must pass, not its centre */
#define TDT_SCREEN_MAX_VERTICES 256
typedef struct tdt_screen_select {
  int32_t  shape;                     /* TDT_SCREEN_* */
  int32_t  rect[4];                   /* x0, y0, x1, y1 inclusive, as tdt_image_extract_voxels' rect (RECT only) */
  uint32_t flags;
  int32_t  material;                  /* -1: any; 0..253: only voxels of this material */
  float    min_distance, max_distance;/* 0 and +inf: no limit */
} tdt_screen_select;
#ifdef __cplusplus
static_assert(sizeof(tdt_screen_select) == 36, "tdt_screen_select is 36 bytes");
#else
_Static_assert(sizeof(tdt_screen_select) == 36, "tdt_screen_select is 36 bytes");
#endif
int tdt_octree_extract_screen(tdt_ctx *ctx, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy,
                              size_t n_vertices, const tdt_image *mask, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);
int tdt_octree_edit_screen(tdt_ctx *ctx, int op, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy,
                           size_t n_vertices, const tdt_image *mask, int32_t material, uint32_t *n_cells);
int tdt_debug_screen_counts(tdt_ctx *ctx, uint64_t out[4]);

/* ---- voxel extraction and compaction ----------------------------------------------------------------------------------
 * The steps octree_update.comp lists as TODOs (octree_update.comp:86-94: removing cells that become empty, removing
 * hierarchies when nodes empty) as explicit operations; edits themselves keep the reference's allocate-only semantics.
 * All three walk the LOGICAL tree of the buffers bound to slots 0 and 7, as treeLookup resolves it (raytracer.comp:372-393):
 * node index = 8 * cell + (x*4 + y*2 + z) from cell 0 for max_depth (slot 7) levels; EMPTY -> nothing; LEAF -> the whole
 * block under the node, material = value; any other type -> descend into cell `value`, except on level max_depth; nodes
 * past the end of the buffer read as EMPTY.  A shared cell is walked once per path that reaches it.  max_depth must be
 * 1..10 (TDT_ERR_INVALID_VALUE otherwise); slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Each call is ordered after the work
 * already queued on the context's stream (an edit dispatched just before needs no tdt_finish).  A multi-device context
 * answers census / extract from device_ids[0] and compacts every replica. */
/* out = {reachable cells (once per path), leaf nodes, finest-level voxels, highest cell index descended into, cells the
 * buffer holds (bytes / 64), first word of the atomic counter (slot 0) or -1 when none is bound}.  Synchronous. */
int tdt_octree_census(tdt_ctx *ctx, int64_t out[6]);
/* the tree's voxels {x, y, z, material + 1} (int32, the input format of tdt_octree_build_cells), sorted by ascending Morton
 * key (spread3(x) << 2 | spread3(y) << 1 | spread3(z)), into host memory.  *n_voxels = their number; voxels_xyzm == NULL:
 * only the count.  capacity (in voxels) < the count, or a LEAF value >= 2^31 - 1: TDT_ERR_INVALID_VALUE (*n_voxels still
 * set, nothing written).  Synchronous. */
int tdt_octree_extract(tdt_ctx *ctx, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);
/* rewrite the bound cells buffer IN PLACE into canonical form: its first *n_cells * 64 bytes become exactly what
 * tdt_octree_build_cells(extract, max_depth) builds (uniform subtrees merged, breadth-first numbering), every byte after
 * them zero (the buffer keeps its size: the freed cells return to the edit program's free pool), and the first word of the
 * atomic counter, when one is bound, becomes *n_cells.  Slots 1-7 are untouched; tables the trace derives from the cells
 * buffer are rebuilt on the next dispatch.  An empty tree becomes one all-EMPTY root cell.  A LEAF value >= 254 (not a
 * material the builder takes), or a canonical tree larger than the buffer (possible only with shared cells):
 * TDT_ERR_INVALID_VALUE, every byte left as it was.  Synchronous. */
int tdt_octree_compact(tdt_ctx *ctx, uint32_t *n_cells);

/* ---- region edits ----------------------------------------------------------------------------------------------------
 * Change any set of voxels of any tree the library renders (merged LEAFs of built or compacted trees included) and leave it
 * canonical.  V = the tree's voxel set (what tdt_octree_extract returns, over [0, 2^max_depth)^3), B = the brush's voxel set
 * clipped to the grid; the bound cells buffer is rewritten IN PLACE into tdt_octree_build_cells(op(V, B), max_depth), by
 * tdt_octree_compact's install rule (tail zeroed, counter = *n_cells, versions bumped), so an empty brush gives the
 * compacted bytes.  For a voxel p:
 *                      p in B, occupied    p in B, empty       p not in B
 *   TDT_REGION_SET     brush material      brush material      unchanged
 *   TDT_REGION_FILL    unchanged           brush material      unchanged
 *   TDT_REGION_PAINT   brush material      stays empty         unchanged
 *   TDT_REGION_CLEAR   removed             stays empty         unchanged
 * Shapes, in exact integer arithmetic: box a = lo, b = hi, both inclusive, empty if lo > hi on an axis; sphere a = centre
 * (anywhere), b[0] = radius >= 0, p inside when (x-cx)^2 + (y-cy)^2 + (z-cz)^2 <= r^2 (int64).  Several shapes: their union.
 * Errors, with nothing written: a bad op or shape, a material outside 0..253, a LEAF value >= 254, SET / FILL shapes whose
 * grid-clipped bounding boxes hold more than 2^26 candidate voxels together (TDT_REGION_BRUSH_CAP), or a result larger than
 * the buffer (*n_cells then receives the cell count it needs): TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound:
 * TDT_ERR_INCOMPLETE.  Each call is ordered after work already queued on the context's stream.  A multi-device context
 * edits every replica (a failure leaves them all unchanged).  Synchronous. */
enum { TDT_SHAPE_BOX = 0, TDT_SHAPE_SPHERE = 1 };
enum { TDT_REGION_SET = 0, TDT_REGION_FILL = 1, TDT_REGION_PAINT = 2, TDT_REGION_CLEAR = 3 };
#define TDT_REGION_BRUSH_CAP (1u << 26)
typedef struct tdt_region {
  int32_t shape;               /* TDT_SHAPE_* */
  int32_t a[3];                /* box: lo; sphere: centre */
  int32_t b[3];                /* box: hi; sphere: b[0] = radius */
  int32_t pad;
} tdt_region;
#ifdef __cplusplus
static_assert(sizeof(tdt_region) == 32, "tdt_region is 32 bytes");
#else
_Static_assert(sizeof(tdt_region) == 32, "tdt_region is 32 bytes");
#endif
/* op over the union of n_regions shapes, brush material 0..253 (the LEAF value; voxel lists carry it + 1) */
int tdt_octree_edit_region(tdt_ctx *ctx, int op, const tdt_region *regions, size_t n_regions, int32_t material, uint32_t *n_cells);
/* op over n voxels {x, y, z, m} (per-voxel material + 1), by the builder's input rules: voxels outside the grid are
 * dropped, of duplicates the last one wins; m must be 1..254 (TDT_ERR_INVALID_VALUE otherwise), except for
 * TDT_REGION_CLEAR, which ignores it.  Stamps a model, or applies a batch of clicks. */
int tdt_octree_edit_voxels(tdt_ctx *ctx, int op, const int32_t *voxels_xyzm, size_t n, uint32_t *n_cells);
/* V and B intersected, as {x, y, z, material + 1}, Morton-sorted (tdt_octree_extract's order and rules: voxels_xyzm == NULL only counts;
 * capacity < the count: TDT_ERR_INVALID_VALUE with *n_voxels set).  Copy / paste, and undo: clear a region, then
 * tdt_octree_edit_voxels(SET, saved) puts it back.  A multi-device context answers from device_ids[0]. */
int tdt_octree_extract_region(tdt_ctx *ctx, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm, size_t capacity,
                              size_t *n_voxels);

/* ---- connected components ------------------------------------------------------------------------------------------------
 * Act on objects rather than shapes.  V = the bound tree's voxel set, exactly what tdt_octree_extract returns, in its Morton
 * order.  Two voxels of V are neighbours when they share a face (connectivity 6) or a face, an edge or a corner
 * (connectivity 26); nothing wraps around the grid (a voxel at x = 2^max_depth - 1 has no +x neighbour).  With
 * TDT_MATCH_ANY any two neighbours are connected, with TDT_MATCH_MATERIAL only neighbours of equal material + 1.  A component
 * is a maximal connected set.  Numbering is canonical: components are numbered 0, 1, ... in the Morton order of their first
 * (lowest-key) voxel, so a result does not depend on scheduling and compares bit for bit.
 *
 * Selection (tdt_select): a component C is selected when min_voxels <= |C| <= max_voxels, and n_seeds == 0 or C holds one of
 * the seed voxels {x, y, z}, and n_regions == 0 or some voxel of C lies inside the union of the regions (tdt_region shapes,
 * the same exact integer test as region edits); invert = 1 flips the selection.  Seeds off the grid or on empty voxels
 * match nothing (a click on air does nothing).  The user stories:
 *   paint bucket      {seed}, TDT_MATCH_MATERIAL, TDT_REGION_PAINT
 *   delete object     {seed}, TDT_MATCH_ANY, TDT_REGION_CLEAR
 *   remove debris     min_voxels = 1, max_voxels = N - 1, TDT_REGION_CLEAR
 *   remove floating   regions = {ground box}, invert = 1, TDT_REGION_CLEAR
 *
 * Errors, with nothing written: connectivity other than 6 or 26, match outside 0..1, invert outside 0..1, min_voxels >
 * max_voxels, an op other than PAINT / CLEAR, a material outside 0..253, NULL seeds or regions with a count above 0, a bad
 * shape, a LEAF value >= 254 in the edit form, or a result larger than the buffer (*n_cells then receives the cell count it
 * needs): TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Each call is ordered after the work already queued
 * on the context's stream.  Synchronous.  A multi-device context answers labels and extraction from device_ids[0] and edits
 * every replica. */
enum { TDT_MATCH_ANY = 0, TDT_MATCH_MATERIAL = 1 };
typedef struct tdt_component {
  uint32_t first;              /* index in tdt_octree_extract's order of its first voxel */
  uint32_t voxels;             /* its size */
  int32_t lo[3];               /* bounding box, inclusive */
  int32_t hi[3];
  int32_t material;            /* material + 1 of its first voxel */
  int32_t pad;
} tdt_component;
typedef struct tdt_select {
  int32_t connectivity, match;
  uint32_t min_voxels, max_voxels;   /* size window, inclusive */
  int32_t invert;              /* 1: act on the components NOT selected */
  int32_t pad;
} tdt_select;
#ifdef __cplusplus
static_assert(sizeof(tdt_component) == 40, "tdt_component is 40 bytes");
static_assert(sizeof(tdt_select) == 24, "tdt_select is 24 bytes");
#else
_Static_assert(sizeof(tdt_component) == 40, "tdt_component is 40 bytes");
_Static_assert(sizeof(tdt_select) == 24, "tdt_select is 24 bytes");
#endif
/* labels[i] = the component of voxel i of tdt_octree_extract; *n_voxels, *n_components = the counts (both pointers required).
 * NULL arrays: counts only; a capacity below its count: TDT_ERR_INVALID_VALUE with the counts set and nothing written.  A
 * LEAF value >= 2^31 - 1: TDT_ERR_INVALID_VALUE (extract's limit).  Every call labels the whole tree, a count query too, so
 * count-then-fill costs two labellings: size the labels by tdt_octree_extract(NULL)'s count (a walk only) and pass a generous
 * table, calling again only when *n_components exceeds it. */
int tdt_octree_components(tdt_ctx *ctx, int connectivity, int match, uint32_t *labels, size_t labels_capacity, size_t *n_voxels,
                          tdt_component *components, size_t capacity, size_t *n_components);
/* op = TDT_REGION_PAINT (every voxel of a selected component gets `material`) or TDT_REGION_CLEAR (removed); the tree is
 * rewritten in place into tdt_octree_build_cells(result) by tdt_octree_compact's install rule, like tdt_octree_edit_region.
 * seeds_xyz: n_seeds triples. */
int tdt_octree_edit_connected(tdt_ctx *ctx, int op, const tdt_select *sel, const int32_t *seeds_xyz, size_t n_seeds,
                              const tdt_region *regions, size_t n_regions, int32_t material, uint32_t *n_cells);
/* the selected components' voxels {x, y, z, material + 1}, Morton-sorted (tdt_octree_extract's order and rules: voxels_xyzm
 * == NULL only counts; capacity < the count: TDT_ERR_INVALID_VALUE with *n_voxels set).  A count query labels the tree too:
 * tdt_octree_extract(NULL)'s count (a walk only) bounds the result.  Copy, and undo: extract, edit, then
 * tdt_octree_edit_voxels(TDT_REGION_SET, saved). */
int tdt_octree_extract_connected(tdt_ctx *ctx, const tdt_select *sel, const int32_t *seeds_xyz, size_t n_seeds,
                                 const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm, size_t capacity,
                                 size_t *n_voxels);

/* ---- voxel morphology ----------------------------------------------------------------------------------------------------
 * Edit by distance to the surface: grow, shrink, open, close, hollow.  V = what tdt_octree_extract returns, over the grid
 * G = [0, 2^max_depth)^3.  Offsets d in {-1,0,1}^3 \ {0}, all 26 (connectivity 26) or the 6 with |dx|+|dy|+|dz| = 1
 * (connectivity 6), ordered by t(d) = 9 (dx+1) + 3 (dy+1) + (dz+1).  Nothing wraps around the grid.
 *   One dilate step  D(S) = S + { q in G \ S : q + d in S for some d }.  Voxels of S keep their material.  A new q gets
 *     `material` when that is >= 0; otherwise the material of q + d for the first d in ascending t(d) with q + d in S (S = the
 *     set BEFORE this step, so the result does not depend on scheduling).
 *   One erode step   E_b(S) = { p in S : for every d, p + d in S, or p + d not in G and b = 1 }.  Materials unchanged.
 *   TDT_MORPH_DILATE = D^r(V).  TDT_MORPH_ERODE = E_border^r(V).  TDT_MORPH_SHELL = V \ E_border^r(V): the voxels within r
 *     steps of the surface, original materials (radius 1: the surface voxels).  TDT_MORPH_OPEN = D^r(E_1^r(V)) and
 *     TDT_MORPH_CLOSE = E_1^r(D^r(V)): both ignore `border` and erode with the outside solid.  On the bounded grid that makes
 *     (E_1, D) an adjunction, so OPEN(V) <= V <= CLOSE(V) holds up to the grid faces and both are idempotent.  OPEN's voxels
 *     carry their original materials (it is a subset of V, so `material` has no effect on it); CLOSE's new voxels carry what
 *     the dilate step that created them gave them.
 *   Mask: with n_regions > 0 (tdt_region shapes, the exact integer test of region edits, union of shapes = M) the result is
 *     (op(V) & M) + (V \ M): neighbourhoods are always evaluated on the whole tree, the mask only limits where voxels may
 *     appear or disappear.  n_regions == 0: no mask.
 * tdt_octree_morph rewrites the bound cells buffer IN PLACE into tdt_octree_build_cells(result, max_depth) by
 * tdt_octree_compact's install rule (tail zeroed, counter = *n_cells, versions bumped; an empty result installs the all-EMPTY
 * root), on every replica of a multi-device context.  tdt_octree_extract_morph returns the same result as a Morton-sorted
 * {x, y, z, material + 1} list by tdt_octree_extract's rules (voxels_xyzm == NULL only counts; capacity < the count:
 * TDT_ERR_INVALID_VALUE with *n_voxels set; a multi-device context answers from device_ids[0]) and leaves the tree, its
 * counter and its versions untouched: the preview, the undo record's other half, and with TDT_MORPH_SHELL, radius 1, the
 * surface-voxel query.
 * Errors, nothing written: a bad op / connectivity / border, radius outside 1..64, material outside -1..253, a bad shape, NULL
 * regions with a count above 0, a LEAF value >= 254, the tree's or any intermediate or final list above 2^26 voxels
 * (TDT_REGION_BRUSH_CAP), a result larger than the buffer (*n_cells then receives the cell count it needs):
 * TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Ordered after work queued on the context's stream;
 * synchronous. */
enum { TDT_MORPH_DILATE = 0, TDT_MORPH_ERODE = 1, TDT_MORPH_OPEN = 2, TDT_MORPH_CLOSE = 3, TDT_MORPH_SHELL = 4 };
typedef struct tdt_morph {
  int32_t op;                  /* TDT_MORPH_* */
  int32_t connectivity;        /* 6 or 26: the structuring element of ONE step */
  int32_t radius;              /* number of steps, 1..64 */
  int32_t material;            /* -1: a new voxel inherits (rule above); 0..253: every new voxel gets this LEAF value */
  int32_t border;              /* DILATE / ERODE / SHELL only: 0 = outside the grid is empty, 1 = outside the grid is solid */
  int32_t pad;
} tdt_morph;
#ifdef __cplusplus
static_assert(sizeof(tdt_morph) == 24, "tdt_morph is 24 bytes");
#else
_Static_assert(sizeof(tdt_morph) == 24, "tdt_morph is 24 bytes");
#endif
int tdt_octree_morph(tdt_ctx *ctx, const tdt_morph *m, const tdt_region *regions, size_t n_regions, uint32_t *n_cells);
int tdt_octree_extract_morph(tdt_ctx *ctx, const tdt_morph *m, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                             size_t capacity, size_t *n_voxels);

/* ---- triangle meshes ------------------------------------------------------------------------------------------------------
 * Turn a surface into voxels.  Vertices are fixed point: TDT_MESH_FRAC fractional bits, so one voxel is 64 units and voxel
 * (x, y, z) is the closed cube [64x, 64x + 64] x [64y, 64y + 64] x [64z, 64z + 64]; every coordinate must satisfy |c| <=
 * TDT_MESH_COORD_MAX (tdt_mesh_quantize / tdt_mesh_fit of include/tdt_host.h produce such vertices from floats).  A triangle
 * covers a voxel of the grid [0, 2^depth)^3 iff the closed triangle and the closed cube share a point, decided exactly in
 * integers; it may be degenerate (a segment or a point), a triangle lying in the plane between two voxel layers covers both,
 * and whatever lies outside the grid contributes nothing.  Triangle t carries materials[t] = material + 1 in 1..254 (materials
 * == NULL: `material` + 1 for all, material 0..253); a voxel covered by several triangles takes the material of the one with
 * the highest index — the builder's last-duplicate-wins rule over (triangle, voxel) pairs in triangle order.  This is a
 * surface voxelisation: interiors are not filled.
 * tdt_voxelize_triangles needs no bound tree (depth 1..10) and returns the covered voxels {x, y, z, material + 1}, Morton-sorted
 * and unique, by tdt_octree_extract's rules (voxels_xyzm == NULL only counts; capacity < the count: TDT_ERR_INVALID_VALUE with
 * *n_voxels set and nothing written; a multi-device context answers from device_ids[0]).
 * tdt_octree_edit_triangles is tdt_octree_edit_voxels(op, that list at the max_depth of slot 7) — same op table, install rule,
 * *n_cells on a misfit, every replica of a multi-device context edited and a failure leaving all of them unchanged — without
 * the list ever leaving the device.
 * Limits: the 8^3-voxel tiles inside the triangles' grid-clipped bounding boxes, summed over the mesh, and the covered
 * (triangle, voxel) pairs must each be <= 2^26 (TDT_REGION_BRUSH_CAP).
 * Errors, nothing written: NULL mesh, NULL arrays with a count above 0, a vertex index >= n_vertices, a coordinate or a
 * material out of range, a bad depth or op, a limit exceeded: TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound (edit form):
 * TDT_ERR_INCOMPLETE.  Ordered after work queued on the context's stream; synchronous. */
#define TDT_MESH_FRAC 6
#define TDT_MESH_COORD_MAX (1 << 18)
typedef struct tdt_mesh {
  const int32_t *vertices;     /* n_vertices x {x, y, z}, fixed point */
  const uint32_t *triangles;   /* n_triangles x 3 vertex indices */
  const int32_t *materials;    /* n_triangles x (material + 1), or NULL */
  uint32_t n_vertices, n_triangles;
  int32_t material;            /* used when materials == NULL: 0..253 */
  int32_t pad;
} tdt_mesh;
#ifdef __cplusplus
static_assert(sizeof(tdt_mesh) == 40, "tdt_mesh is 40 bytes");
#else
_Static_assert(sizeof(tdt_mesh) == 40, "tdt_mesh is 40 bytes");
#endif
int tdt_voxelize_triangles(tdt_ctx *ctx, const tdt_mesh *mesh, int depth, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);
int tdt_octree_edit_triangles(tdt_ctx *ctx, int op, const tdt_mesh *mesh, uint32_t *n_cells);

/* ---- stroke brushes ---------------------------------------------------------------------------------------------------------
 * Pull a brush along a path.  A stroke is a set of segments between points given in voxel coordinates (on or off the grid,
 * |coordinate| <= TDT_STROKE_COORD_MAX), swept by a nib of `radius` 0..TDT_STROKE_RADIUS_MAX.  Coverage is defined on the grid
 * alone and decided in exact integers: voxel p of [0, 2^depth)^3 is covered by segment (a, b) when some point q of the closed
 * segment is within `radius` of p — TDT_SHAPE_SPHERE in the Euclidean metric, |p - q|_2 <= r (a capsule), TDT_SHAPE_BOX in the
 * Chebyshev metric, max_k |p_k - q_k| <= r (a swept cube).  A dab (a == b) with SPHERE is exactly the TDT_SHAPE_SPHERE of
 * tdt_region, with BOX exactly the box [a - r, a + r]; radius 0 covers only the lattice points lying on the segment; the set
 * of (a, b) is the set of (b, a).
 *   SPHERE, with d = b - a, w = p - a, L2 = d . d, t = w . d:  t <= 0: |w|^2 <= r^2;  t >= L2: |p - b|^2 <= r^2;  otherwise
 *     (|w|^2 - r^2) L2 <= t^2.
 *   BOX: the slab test of the segment against the cube [p - r, p + r], the ends of the parameter's intervals compared by
 *     cross-multiplication; an axis with d_k = 0 bounds no parameter but must satisfy |w_k| <= r.
 * segments == NULL (n_segments must be 0): the polyline 0-1, 1-2, ... of the points, one point being a single dab; otherwise
 * n_segments x {i, j} point indices (i == j: a dab; n_segments == 0: nothing).  Segment s carries materials[s] = material + 1 in
 * 1..254 (materials == NULL: `material` + 1 for all, material 0..253); a voxel covered by several segments takes the material of
 * the one with the highest index — the builder's last-duplicate-wins rule over (segment, voxel) pairs in segment order.
 * tdt_voxelize_stroke needs no bound tree (depth 1..10) and returns the covered voxels {x, y, z, material + 1}, Morton-sorted
 * and unique, by tdt_octree_extract's rules (voxels_xyzm == NULL only counts; capacity < the count: TDT_ERR_INVALID_VALUE with
 * *n_voxels set and nothing written; a multi-device context answers from device_ids[0]).
 * tdt_octree_edit_stroke is tdt_octree_edit_voxels(op, that list at the max_depth of slot 7) — same op table, install rule,
 * *n_cells on a misfit, every replica of a multi-device context edited and a failure leaving all of them unchanged — without
 * the list ever leaving the device.  tdt_octree_extract_stroke is V (the bound tree's voxels) intersected with that list, with
 * V's own materials, by tdt_octree_extract_region's rules: the undo record to take before a CLEAR or PAINT stroke, and the copy
 * tool.  An empty stroke (n_points == 0) is legal: the empty list, and the edit installs the compacted tree.
 * Limits: the 8^3-voxel tiles inside the grid-clipped bounding boxes of the segments grown by the radius, summed over the
 * stroke, and the covered (segment, voxel) pairs must each be <= 2^26 (TDT_REGION_BRUSH_CAP); n_points and n_segments <= 2^20.
 * Errors, nothing written: NULL stroke, NULL arrays with a count above 0, n_points == 0 with segments, segments == NULL with
 * n_segments != 0, a point index >= n_points, a coordinate, radius, material, shape, depth, op or pad out of range, a limit
 * exceeded: TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound (edit and extract forms): TDT_ERR_INCOMPLETE.  Ordered after work queued
 * on the context's stream; synchronous. */
#define TDT_STROKE_COORD_MAX 8192
#define TDT_STROKE_RADIUS_MAX 2048
typedef struct tdt_stroke {
  const int32_t *points;       /* n_points x {x, y, z}, voxel coordinates */
  const uint32_t *segments;    /* n_segments x {i, j} point indices, or NULL: the polyline of the points */
  const int32_t *materials;    /* per segment, material + 1, or NULL */
  uint32_t n_points, n_segments;
  int32_t shape;               /* TDT_SHAPE_SPHERE: round nib; TDT_SHAPE_BOX: cube nib of half-width radius */
  int32_t radius;              /* 0..TDT_STROKE_RADIUS_MAX */
  int32_t material;            /* used when materials == NULL: 0..253 */
  int32_t pad;                 /* 0 */
} tdt_stroke;
#ifdef __cplusplus
static_assert(sizeof(tdt_stroke) == 48, "tdt_stroke is 48 bytes");
#else
_Static_assert(sizeof(tdt_stroke) == 48, "tdt_stroke is 48 bytes");
#endif
int tdt_voxelize_stroke(tdt_ctx *ctx, const tdt_stroke *stroke, int depth, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);
int tdt_octree_edit_stroke(tdt_ctx *ctx, int op, const tdt_stroke *stroke, uint32_t *n_cells);
int tdt_octree_extract_stroke(tdt_ctx *ctx, const tdt_stroke *stroke, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);

/* ---- enclosed space ---------------------------------------------------------------------------------------------------------
 * Fill what is sealed off: the cavities of a tree, the inside of a watertight mesh.  Let G = [0, 2^depth)^3 and W, a subset of
 * G, a wall set.  Two EMPTY voxels (G \ W) are neighbours under connectivity 6 when they share a face, under connectivity 26
 * when they share a face, an edge or a corner; nothing wraps around the grid.  An empty voxel is OUTSIDE when it lies on a face
 * of G (a coordinate 0 or 2^depth - 1) or is connected to such a voxel through empty neighbours.  E(W, c) = the empty voxels
 * that are not outside.  The space beyond the grid is open: a cavity that reaches a grid face through empties is not enclosed.
 * The definition is a fixed point of the grid alone, so a result does not depend on scheduling and compares bit for bit.
 * Connectivity 6 for the empties is the permissive choice (a diagonal gap in a wall does not leak), 26 the strict one.  The
 * closed-triangle-against-closed-cube coverage of tdt_voxelize_triangles separates even under 26: where the surface passes
 * through a point, every closed cube holding that point is covered, so no empty voxel inside touches one outside, not even by
 * a corner.
 * Material of a voxel q of E: `material` 0..253 is that LEAF value; `material` -1 inherits the material of the first voxel of W
 * met walking from q in decreasing x (it exists, or q would reach the face x = 0).
 * tdt_octree_extract_enclosed: W = V, what tdt_octree_extract returns over max_depth (slot 7).  Returns E(V, c) & M as
 * {x, y, z, material + 1}, Morton-sorted, by tdt_octree_extract's rules (voxels_xyzm == NULL only counts; capacity < the count:
 * TDT_ERR_INVALID_VALUE with *n_voxels set and nothing written; a multi-device context answers from device_ids[0]).  M = the
 * union of the regions (tdt_region shapes, the exact integer test of region edits); n_regions == 0: no mask.  The flood always
 * runs on the whole tree, the mask only limits what is reported.  The tree, its counter and its versions are untouched: it is
 * the preview and the undo record — tdt_octree_edit_voxels(TDT_REGION_CLEAR, that list) undoes a fill.
 * tdt_octree_fill_enclosed rewrites the bound cells buffer IN PLACE into tdt_octree_build_cells(V + that list, max_depth) by
 * tdt_octree_compact's install rule (tail zeroed, counter = *n_cells, versions bumped; an empty E installs the compacted
 * bytes), on every replica of a multi-device context, a failure leaving all of them unchanged.
 * tdt_voxelize_triangles_solid: S = tdt_voxelize_triangles(mesh, depth); the result is S + E(S, c), E's materials by tdt_fill
 * (inherit carries per-triangle materials inward along -x), by the same list rules.  Needs no bound tree.
 * tdt_octree_edit_triangles_solid is tdt_octree_edit_voxels(op, that list at the max_depth of slot 7), all four ops, without the
 * list ever leaving the device, exactly like tdt_octree_edit_triangles.  Enclosure is decided by the mesh's own surface alone,
 * never by what the tree already holds.
 * Errors, nothing written: a NULL tdt_fill, connectivity other than 6 / 26, material outside -1..253, a bad shape, NULL regions
 * with a count above 0, a LEAF value >= 254, a bad op or depth, the mesh errors of tdt_voxelize_triangles, |V|, |S| or |E| above
 * 2^26 (TDT_REGION_BRUSH_CAP), a result larger than the buffer (*n_cells then receives the cell count it needs):
 * TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound (tree forms, mesh edit form): TDT_ERR_INCOMPLETE.  The DOMAIN has no cap: the flood
 * runs on bit volumes over the bounding box of W, at most 2^30 bits = 128 MiB each at depth 10: occupancy, reach, and 128 MiB of
 * per-word counts, 384 MiB in all besides the lists (|S| is bounded by tdt_voxelize_triangles' own limit of 2^26 covered pairs).  Ordered after work queued
 * on the context's stream; synchronous. */
typedef struct tdt_fill {
  int32_t connectivity;        /* 6 or 26: how EMPTY voxels connect */
  int32_t material;            /* -1: inherit (rule above); 0..253: every filled voxel gets this LEAF value */
} tdt_fill;
#ifdef __cplusplus
static_assert(sizeof(tdt_fill) == 8, "tdt_fill is 8 bytes");
#else
_Static_assert(sizeof(tdt_fill) == 8, "tdt_fill is 8 bytes");
#endif
int tdt_octree_extract_enclosed(tdt_ctx *ctx, const tdt_fill *fill, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                                size_t capacity, size_t *n_voxels);
int tdt_octree_fill_enclosed(tdt_ctx *ctx, const tdt_fill *fill, const tdt_region *regions, size_t n_regions, uint32_t *n_cells);
int tdt_voxelize_triangles_solid(tdt_ctx *ctx, const tdt_mesh *mesh, int depth, const tdt_fill *fill, int32_t *voxels_xyzm, size_t capacity,
                                 size_t *n_voxels);
int tdt_octree_edit_triangles_solid(tdt_ctx *ctx, int op, const tdt_mesh *mesh, const tdt_fill *fill, uint32_t *n_cells);
/* the flood passes of the context's last enclosed-space call that changed the volume (0: the seeds were the fixed point, or the
 * box needed no flood); the host queues passes in batches of 8, so up to 8 more ran idle.  Measurement only. */
int tdt_debug_fill_passes(const tdt_ctx *ctx);

/* ---- surface extraction -----------------------------------------------------------------------------------------------------
 * Turn the tree back into a surface: the inverse of tdt_voxelize_triangles.  V = what tdt_octree_extract returns, over the grid
 * G = [0, 2^max_depth)^3.  Faces are numbered f = 0..5 as -x, +x, -y, +y, -z, +z: axis a = f >> 1, sign s = f & 1, in-plane axes
 * u = (a + 1) % 3 and v = (a + 2) % 3.  Voxel p of V has an EXPOSED face f when p -+ e_a is not in V; a neighbour outside G counts
 * as empty and nothing wraps around the grid.  Cavity walls are exposed faces like any other: call tdt_octree_fill_enclosed first
 * for the outer skin only.
 *   Mask: with n_regions > 0 (tdt_region shapes, the exact integer test of region edits) only the faces of voxels inside the union
 *     of the shapes are reported; neighbourhoods are always evaluated on the whole tree (morphology's convention).
 *   by_material = 1: a face carries its voxel's material + 1; by_material = 0: every face carries 0 (the collision-mesh form,
 *     which merges across materials).
 *   Merging is canonical, so a result does not depend on scheduling and compares bit for bit.  Write w for p[a], the voxel's OWN
 *     coordinate along the axis (not the plane's position).  merge = 0: every exposed face is a 1 x 1 quad.  merge = 1, per face
 *     direction f: within one (w, v) a RUN is a maximal set of exposed faces with consecutive u and equal carried material; runs
 *     with the same (w, u0, u1) and carried material on consecutive v form a maximal STACK, and each stack is one quad.  "Runs,
 *     then stacks of identical runs" is deliberately not an optimal greedy cover: it is unique.
 *   Output: tdt_quad, eight int32.  origin is the minimum corner in lattice coordinates 0..2^max_depth: origin[a] = w + s,
 *     origin[u] = u0, origin[v] = v0; size = {u1 - u0 + 1, v1 - v0 + 1}; pad = 0.  Quads are ordered by face, then w, then u0,
 *     then v0.
 * tdt_octree_extract_surface follows tdt_octree_extract's rules: quads == NULL only counts; capacity < the count:
 * TDT_ERR_INVALID_VALUE with *n_quads set and nothing written; a multi-device context answers from device_ids[0].  The tree, its
 * counter and its versions are untouched.  tdt_quads_to_mesh (include/tdt_host.h) turns the quads into the indexed mesh of tdt_mesh.
 * Errors, nothing written: a NULL tdt_surface, merge or by_material outside 0..1, a bad shape, NULL regions with a count above 0,
 * a LEAF value >= 254, |V| or the exposed faces of any one direction above 2^26 (TDT_REGION_BRUSH_CAP): TDT_ERR_INVALID_VALUE;
 * slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Ordered after work queued on the context's stream; synchronous. */
typedef struct tdt_surface {
  int32_t merge;               /* 0: one quad per exposed face; 1: runs, then stacks of identical runs */
  int32_t by_material;         /* 1: faces carry material + 1 and merge within a material only; 0: they carry 0 */
} tdt_surface;
typedef struct tdt_quad {
  int32_t face;                /* 0..5: -x, +x, -y, +y, -z, +z */
  int32_t material;            /* material + 1, or 0 with by_material = 0 */
  int32_t origin[3];           /* minimum corner, lattice coordinates */
  int32_t size[2];             /* extent along u = (a + 1) % 3 and v = (a + 2) % 3 */
  int32_t pad;
} tdt_quad;
#ifdef __cplusplus
static_assert(sizeof(tdt_surface) == 8, "tdt_surface is 8 bytes");
static_assert(sizeof(tdt_quad) == 32, "tdt_quad is 32 bytes");
#else
_Static_assert(sizeof(tdt_surface) == 8, "tdt_surface is 8 bytes");
_Static_assert(sizeof(tdt_quad) == 32, "tdt_quad is 32 bytes");
#endif
int tdt_octree_extract_surface(tdt_ctx *ctx, const tdt_surface *opt, const tdt_region *regions, size_t n_regions, tdt_quad *quads,
                               size_t capacity, size_t *n_quads);

/* ---- face tools -------------------------------------------------------------------------------------------------------------
 * Act on a FACE of the model: the connected coplanar patch under the cursor is pulled out, pushed in or painted.  V, G, the face
 * numbering f = 0..5, a = f >> 1, s = f & 1, u = (a + 1) % 3, v = (a + 2) % 3, w = p[a] and "voxel p has an EXPOSED face f" are
 * those of the surface extraction above; n_f is the outward unit normal of direction f.  All arithmetic is in integers and every
 * result is canonical, so results compare bit for bit.
 *   Face list: F = the exposed faces in the order of tdt_octree_extract_surface with merge = 0, by_material = 1 — by face, then
 *     w, then u, then v — each carrying its voxel's material + 1.  With n_regions > 0 only the faces of voxels inside the union of
 *     the shapes are in F: the mask CONFINES a region (geodesic's convention); exposure is always evaluated on the whole tree.
 *   Adjacency: two faces of F with the same f and the same w are adjacent under connectivity 4 when they differ by 1 in exactly
 *     one of u, v; under connectivity 8 when they differ by at most 1 in each of u, v and are not equal.  Faces of different
 *     direction are never adjacent — not even the -x face at w and the +x face at w - 1, which lie in one geometric plane — and
 *     nothing wraps around the grid.  With TDT_MATCH_MATERIAL only faces of equal carried material are adjacent, with
 *     TDT_MATCH_ANY any two.
 *   Face region: a maximal connected set; regions are numbered 0, 1, .. in the order of their first face in F.
 *   Seeds: n_seeds quadruples {x, y, z, f}; a seed selects the region that holds face f of voxel (x, y, z).  A seed off the grid,
 *     on an empty voxel, on a face that is not exposed or on a face outside the mask selects nothing; duplicates are allowed;
 *     f outside 0..5 is an error.
 *   Columns: for a selected face (p, f) and the signed `distance` d, |d| <= TDT_FACES_DISTANCE_MAX: d > 0: the voxels p + k n_f,
 *     k = 1..d; d < 0: the voxels p - k n_f, k = 0..|d| - 1 (the owner and what lies behind it); d = 0: nothing.  Columns are
 *     clipped to G.  With block = 1 a column ends early: for d > 0 before its first voxel that is in V (it stops at an obstacle),
 *     for d < 0 before its first voxel that is NOT in V (it carves only the contiguous solid run).  With block = 0 it runs its
 *     full clipped length.
 *   Material: a column voxel carries material + 1 for material 0..253; with material = -1 its face's carried material, so an
 *     extrusion continues the wall's colours.
 *   The column list: the (voxel, material) pairs of all selected faces, taken in the order of F, then k, reduced by the
 *     builder's rule that of duplicates the last one wins; Morton-sorted and unique.  Two columns of one region never overlap;
 *     columns of different seeded regions can (opposite walls of a slot pulled towards each other, one direction at different
 *     w), and the last-wins rule decides.
 *   Stories: pull = TDT_REGION_FILL or SET with d > 0; push = TDT_REGION_CLEAR with d < 0; paint a face = TDT_REGION_PAINT with
 *     d = -1; "until it hits something" = block = 1 with a large |d|.
 * tdt_octree_face_regions returns F as 1 x 1 tdt_quads — byte for byte what tdt_octree_extract_surface with merge = 0,
 * by_material = 1 and the same mask returns — the label of each face and the region table, by tdt_octree_components' rules: a
 * NULL array only counts; a capacity below its count: TDT_ERR_INVALID_VALUE with the counts set and nothing written.  It only
 * reads; a multi-device context answers from device_ids[0].
 * tdt_octree_extract_faces lists, by tdt_octree_extract's rules, TDT_FACES_COLUMNS: the column list (the preview, and what
 * tdt_image_overlay takes); TDT_FACES_TREE: V intersected with the column list, with V's own materials (the undo record before a
 * push, a paint or a SET pull).
 * tdt_octree_edit_faces is tdt_octree_edit_voxels(op, the column list) without the list leaving the device: all four ops, the
 * install rule, *n_cells on a misfit, every replica edited and a failure leaving all replicas unchanged exactly as for
 * tdt_octree_edit_stroke.  With n_seeds == 0 or distance == 0 it installs the compacted tree.
 * Limits: |V|, the faces of any one direction and the (face, voxel) pairs of the columns each <= 2^26 (TDT_REGION_BRUSH_CAP);
 * n_seeds <= 2^20.
 * Errors, nothing written: a NULL struct, NULL seeds or regions with a count above 0, connectivity other than 4 or 8, match,
 * block or what out of range, distance or material out of range, non-zero pad, a seed f outside 0..5, a bad shape or op, a LEAF
 * value >= 254, a limit exceeded, a result larger than the buffer: TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound:
 * TDT_ERR_INCOMPLETE.  Ordered after work queued on the context's stream; synchronous. */
#define TDT_FACES_DISTANCE_MAX 1023
enum { TDT_FACES_COLUMNS = 0, TDT_FACES_TREE = 1 };
typedef struct tdt_faces {
  int32_t connectivity;        /* 4 or 8 */
  int32_t match;               /* TDT_MATCH_ANY / TDT_MATCH_MATERIAL */
  int32_t distance;            /* -1023..1023 */
  int32_t block;               /* 0 / 1 */
  int32_t material;            /* -1 inherit, 0..253 */
  int32_t pad;                 /* 0 */
} tdt_faces;
typedef struct tdt_face_region {
  uint32_t first;              /* index in F of its first face */
  uint32_t faces;              /* its size */
  int32_t face, w;             /* direction and the voxels' own coordinate along the axis */
  int32_t lo[2], hi[2];        /* (u, v) bounding box, inclusive */
  int32_t material;            /* carried material of its first face */
  int32_t pad;
} tdt_face_region;
#ifdef __cplusplus
static_assert(sizeof(tdt_faces) == 24, "tdt_faces is 24 bytes");
static_assert(sizeof(tdt_face_region) == 40, "tdt_face_region is 40 bytes");
#else
_Static_assert(sizeof(tdt_faces) == 24, "tdt_faces is 24 bytes");
_Static_assert(sizeof(tdt_face_region) == 40, "tdt_face_region is 40 bytes");
#endif
int tdt_octree_face_regions(tdt_ctx *ctx, int connectivity, int match, const tdt_region *regions, size_t n_regions, tdt_quad *faces,
                            uint32_t *labels, size_t faces_capacity, size_t *n_faces, tdt_face_region *table, size_t capacity,
                            size_t *n_face_regions);
int tdt_octree_extract_faces(tdt_ctx *ctx, const tdt_faces *faces, const int32_t *seeds_xyzf, size_t n_seeds, const tdt_region *regions,
                             size_t n_regions, int what, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);
int tdt_octree_edit_faces(tdt_ctx *ctx, int op, const tdt_faces *faces, const int32_t *seeds_xyzf, size_t n_seeds,
                          const tdt_region *regions, size_t n_regions, uint32_t *n_cells);
/* the labelling's hook stage with (on = 1, the default) or without (0) the in-wave pre-merge of runs along v; both label alike.
 * Measurement only (tools/faces_time.py). */
int tdt_debug_faces_premerge(tdt_ctx *ctx, int on);

/* ---- exact Euclidean distance ----------------------------------------------------------------------------------------------
 * Round grow, shrink, open, close and hollow, and a distance field.  V = what tdt_octree_extract returns, over the grid
 * G = [0, N)^3, N = 2^max_depth.  For a voxel q of G and a set S, d2(q, S) = min over p in S of |q - p|^2, in integers; nothing
 * wraps around the grid.  The NEAREST voxel of q is, of the voxels of S at that minimum, the one with the lowest x, then the
 * lowest y, then the lowest z.  (The order decomposes over three axis passes taken in any order, each keeping among equal sums
 * the lexicographically lowest (x, y, z); at radius2 = 1 it is tdt_octree_morph's "first offset in ascending t".)
 *   B(r2) = { d in Z^3 : |d|^2 <= r2 }, r2 = `radius2` in 1..4096: r * r is the ball of radius r, 2 the 18-neighbourhood, 5 "2 and
 *     a bit".  R = the smallest integer with R * R >= r2, so R <= 64.
 *   D(S) = S + { q in G \ S : d2(q, S) <= r2 }.  Voxels of S keep their material; a new q gets `material` when that is >= 0,
 *     otherwise the material of its nearest voxel of S.
 *   E_b(S) = { p in S : every lattice point q with |q - p|^2 <= r2 is in S, or lies outside G and b = 1 }.  Materials unchanged.
 *     With b = 0 the outside of the grid is empty: p survives only if min over axes of min(p_a + 1, N - p_a) exceeds sqrt(r2).
 *   The ops are the TDT_MORPH_* numbers: DILATE = D(V).  ERODE = E_border(V).  SHELL = V \ E_border(V).  OPEN = D(E_1(V)) and
 *     CLOSE = E_1(D(V)) ignore `border`, for tdt_octree_morph's reason; OPEN is a subset of V and keeps V's materials, CLOSE's
 *     new voxels carry what D gave them.
 *   Mask: as in voxel morphology the result is (op(V) & M) + (V \ M); distances are always taken on the whole tree.
 * tdt_octree_morph_round / tdt_octree_extract_morph_round behave exactly like tdt_octree_morph / tdt_octree_extract_morph: the
 * in-place rebuild by tdt_octree_compact's install rule on every replica of a multi-device context, a failure leaving all of
 * them unchanged, *n_cells on a misfit; the Morton-sorted list by tdt_octree_extract's rules from device_ids[0], the tree, its
 * counter and its versions untouched.  The number of passes, launches and synchronisations
 * does not depend on radius2; the domain's margin, the scans' halo and their length grow with R (DESIGN.md has the measured cost).
 * tdt_octree_distance_field returns the SIGNED squared distance over the inclusive box lo..hi, which must lie inside G and hold
 * <= 2^26 voxels: field[((z - lo z) * ey + (y - lo y)) * ex + (x - lo x)], e = hi - lo + 1.  An empty voxel q gets +d2(q, V)
 * (>= 1); an occupied p gets -(the squared distance to the nearest empty lattice point, the points outside the grid counting
 * when `border` = 0) (<= -1).  A magnitude above `max_d2` (1..4096) is reported as max_d2 + 1, the sign kept.  nearest_xyz is
 * optional, three int32 per voxel: an empty voxel with a value <= max_d2 gets its nearest voxel of V, an occupied voxel its own
 * coordinates, any other {-1, -1, -1}.  field == NULL only sets *n_voxels; capacity below the count: TDT_ERR_INVALID_VALUE with
 * the count set.  The tree, its counter and its versions are untouched; a multi-device context answers from device_ids[0].  An
 * empty tree is valid: every value is max_d2 + 1, and the round ops install the all-EMPTY root or return an empty list.
 * Limit, checked on the host before any volume is allocated: the DOMAIN — bbox(V) (round ops) or the requested box (field),
 * grown by R on every side and clipped to G — must hold <= TDT_ROUND_DOMAIN_CAP voxels.  Over it the unit allocates, per voxel
 * of the domain's rows rounded out to multiples of 32 in x: 3 bytes of offsets, 3 more for DILATE / CLOSE with an inherited
 * material, and up to three bit volumes and one count per 32 voxels (0.5 byte): 6.5 bytes at most, 1.75 GiB at the cap for an
 * aligned domain.  The field form adds 4 (16 with nearest_xyz) bytes per voxel of the box.  |V| and every produced list are
 * held to 2^26 voxels (TDT_REGION_BRUSH_CAP).
 * Errors, nothing written: a NULL struct or pointer, a bad op, radius2 or max_d2 outside 1..4096, material outside -1..253,
 * border outside 0..1, a bad shape, NULL regions with a count above 0, a bad box, a LEAF value >= 254, a limit exceeded:
 * TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Ordered after work queued on the context's stream;
 * synchronous. */
#define TDT_ROUND_DOMAIN_CAP (1u << 28)
typedef struct tdt_round {
  int32_t op;                  /* TDT_MORPH_* */
  int32_t radius2;             /* the squared radius, 1..4096 */
  int32_t material;            /* -1: a new voxel inherits its nearest voxel's; 0..253: every new voxel gets this LEAF value */
  int32_t border;              /* DILATE / ERODE / SHELL only: 0 = outside the grid is empty, 1 = outside the grid is solid */
} tdt_round;
#ifdef __cplusplus
static_assert(sizeof(tdt_round) == 16, "tdt_round is 16 bytes");
#else
_Static_assert(sizeof(tdt_round) == 16, "tdt_round is 16 bytes");
#endif
int tdt_octree_morph_round(tdt_ctx *ctx, const tdt_round *r, const tdt_region *regions, size_t n_regions, uint32_t *n_cells);
int tdt_octree_extract_morph_round(tdt_ctx *ctx, const tdt_round *r, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                                   size_t capacity, size_t *n_voxels);
int tdt_octree_distance_field(tdt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t max_d2, int32_t border, int32_t *field,
                              int32_t *nearest_xyz, size_t capacity, size_t *n_voxels);

/* ---- voxel smoothing ---------------------------------------------------------------------------------------------------------
 * The smooth brush: the density of the object around every voxel, thresholded; and the raw density as a field.  N = 2^max_depth,
 * G = [0, N)^3, V = what tdt_octree_extract returns, B(r2) = { d in Z^3 : |d|^2 <= r2 } as in the round unit, r2 = `radius2` in
 * 1..225 here, so R (the smallest integer with R * R >= r2) <= 15, every x-chord of the ball is at most 31 voxels wide, and |B|
 * (tdt_ball_size) is odd.  For a set S and a voxel q of G:
 *   DENSITY  d(q, S) = |{ p in q + B : p in S }|.  Points outside G are never in S; nothing wraps around the grid.
 *   SUPPORT  n(q) = |B| with `border` = 0: the outside of the grid counts as empty space.  n(q) = |(q + B) & G| with `border` = 1:
 *     the outside of the grid is left out of the vote, so an object cut by a grid face is not rounded off there.
 *   THRESHOLD TEST  T(q, S): `threshold` = 0 (majority): 2 d > n.  `threshold` in 1..65536, a Q16 fraction of the support:
 *     65536 d >= threshold * n, exact in 32-bit unsigned arithmetic because d <= |B(225)| < 2^15.  Either way T implies d >= 1.
 *   ONE STEP  F(S) by `mode`: TDT_SMOOTH_BOTH: the voxels of G with T.  TDT_SMOOTH_ADD: S plus those with T (fills dents only).
 *     TDT_SMOOTH_REMOVE: those of S with T (shaves bumps only).
 *   MATERIALS  A voxel of S that survives keeps its material.  A new voxel q gets `material` when that is >= 0, otherwise the
 *     material of its NEAREST voxel of S by the round unit's rule: among the p in S at the least |p - q|^2 the one with the
 *     lowest x, then y, then z.  Such a p lies inside q + B because d >= 1.  It is taken on the set BEFORE the step.
 *   MASK  With n_regions > 0, M = the union of the shapes by the exact integer test of region edits, a step is
 *     (F(S) & M) + (S \ M); densities are always taken on the whole current set.
 *   RESULT  S_0 = V, S_(k + 1) = one step applied to S_k; the result is S_iterations, `iterations` in 1..16.  (A step that
 *     changes nothing ends the loop: every later one would change nothing either.)
 * Identities: threshold 1, BOTH, border 0 is tdt_octree_morph_round's DILATE at the same radius2, inherited materials included;
 * threshold 65536, BOTH is its ERODE with the same border; ADD gives a superset of V, REMOVE a subset of V with V's materials;
 * with border 0 and threshold 0 a step never leaves bbox(S) (for q outside the box along an axis, mirroring d in that axis maps
 * the ball points that can be occupied injectively onto points that cannot, so 2 d <= |B| - |{d_axis = 0}| < |B|).
 * tdt_octree_smooth rewrites the bound cells buffer in place into tdt_octree_build_cells(result, max_depth) by
 * tdt_octree_compact's install rule, on every replica of a multi-device context; a failure leaves all of them unchanged.
 * *n_cells is written after the install, and on a misfit before the refusal: the size the buffer must grow to.  The list never
 * leaves the device between iterations or before the install.  tdt_octree_extract_smooth returns the same result as a
 * Morton-sorted list by tdt_octree_extract's rules from device_ids[0] (voxels_xyzm == NULL only counts; capacity below the count:
 * TDT_ERR_INVALID_VALUE with the count set); the tree, its counter and its versions are untouched.
 * tdt_octree_density_field follows tdt_octree_distance_field in every convention — the inclusive box inside G holding <= 2^26
 * voxels, density[((z - lo z) * ey + (y - lo y)) * ex + (x - lo x)], density == NULL only setting *n_voxels without walking the
 * tree, capacity below the count: TDT_ERR_INVALID_VALUE with the count set, a multi-device context answering from device_ids[0],
 * an empty tree being valid (all zeros): density[i] = d(q, V), and support (optional) [i] = |(q + B) & G|, the n(q) of border 1.
 * tdt_ball_size is |B(radius2)| for 1..4096 and -1 otherwise, in host arithmetic.
 * Limit, checked on the host before any volume is allocated: the DOMAIN — bbox(V) grown by iterations * R on every side and
 * clipped to G, or the field's box grown by R — holds <= TDT_SMOOTH_DOMAIN_CAP voxels.  With border 0 and a threshold of 0 or
 * above 32768 the growth is 0, by the last identity.  Over the domain the unit keeps two bit volumes and a count per 32 voxels;
 * |V| and every list stay within 2^26 voxels (TDT_REGION_BRUSH_CAP).
 * Errors, nothing written: a NULL struct or pointer, radius2 outside 1..225, iterations outside 1..16, threshold outside
 * 0..65536, a bad mode, material outside -1..253, border outside 0..1, a bad shape, NULL regions with a count above 0, a bad
 * box, a LEAF value >= 254, a limit exceeded: TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Ordered after
 * work queued on the context's stream; synchronous. */
#define TDT_SMOOTH_DOMAIN_CAP (1u << 28)
enum { TDT_SMOOTH_BOTH = 0, TDT_SMOOTH_ADD = 1, TDT_SMOOTH_REMOVE = 2 };
typedef struct tdt_smooth {
  int32_t radius2;             /* the squared radius of the ball, 1..225 */
  int32_t iterations;          /* steps, 1..16 */
  int32_t threshold;           /* 0: majority; 1..65536: Q16 fraction of the support */
  int32_t mode;                /* TDT_SMOOTH_* */
  int32_t material;            /* -1: a new voxel inherits its nearest voxel's; 0..253: every new voxel gets this LEAF value */
  int32_t border;              /* 0 = outside the grid is empty space, 1 = outside the grid is left out of the vote */
} tdt_smooth;
#ifdef __cplusplus
static_assert(sizeof(tdt_smooth) == 24, "tdt_smooth is 24 bytes");
#else
_Static_assert(sizeof(tdt_smooth) == 24, "tdt_smooth is 24 bytes");
#endif
int32_t tdt_ball_size(int32_t radius2);
int tdt_octree_smooth(tdt_ctx *ctx, const tdt_smooth *s, const tdt_region *regions, size_t n_regions, uint32_t *n_cells);
int tdt_octree_extract_smooth(tdt_ctx *ctx, const tdt_smooth *s, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                              size_t capacity, size_t *n_voxels);
int tdt_octree_density_field(tdt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t radius2, int32_t *density, int32_t *support,
                             size_t capacity, size_t *n_voxels);

/* ---- affine transforms of voxel selections -------------------------------------------------------------------------------
 * Move, turn, mirror, rotate and scale a selection by resampling.  N = 2^max_depth, G = [0, N)^3, V = what tdt_octree_extract
 * returns, S = the voxels of V inside the mask: all of V with n_regions == 0, otherwise those inside the union of the regions
 * (tdt_region shapes, the exact integer test of region edits).  The transform is given DESTINATION -> SOURCE, which makes the
 * result onto by construction: no holes under a rotation or an enlargement.  For a destination voxel p, in int64,
 *     q = 2 p + 1                                   (its doubled centre)
 *     s_i = (a[3 i] q_x + a[3 i + 1] q_y + a[3 i + 2] q_z + t_i) >> 17,   i = x, y, z
 * with >> the arithmetic shift (a floor, never a truncating divide), `a` in Q16 (TDT_XFORM_ONE = 65536 is 1.0) and `t` in units
 * of 2^-17 voxel.  The result is
 *     T = { (p, m) : p in G, dst_lo <= p <= dst_hi, s(p) in G, s(p) in S },
 * m = the material + 1 of s(p) when `material` is -1, or `material` + 1 for 0..253; Morton-sorted by p by tdt_octree_extract's
 * rules.  The identity is a = 65536 I, t = 0; a translation by d is t = -d 2^17; a = 32768 I doubles the selection about the
 * corner of the grid.  include/tdt_host.h has builders (tdt_xform_translate, _quarter_turns, _mirror, _scale, _rotate,
 * _from_affine) that fill the struct.
 * tdt_octree_extract_transform returns T by tdt_octree_extract's rules (voxels_xyzm == NULL only counts; capacity < the count:
 * TDT_ERR_INVALID_VALUE with *n_voxels set; a multi-device context answers from device_ids[0]) and leaves the tree, its counter
 * and its versions untouched.  tdt_octree_transform is tdt_octree_edit_voxels with the list T, taken from the tree BEFORE the
 * edit and never leaving the device: op TDT_REGION_SET / FILL / PAINT / CLEAR, the in-place rebuild by tdt_octree_compact's
 * install rule on every replica of a multi-device context, a failure leaving all of them unchanged, *n_cells on a misfit.  The
 * source voxels are not removed: a move is tdt_octree_extract_transform, tdt_octree_edit_region(CLEAR), tdt_octree_edit_voxels.
 * Limits, checked on the host before anything is queued: |a[k]| <= 2^20 and |t_i| <= 2^40 (the sum then stays below 2^41),
 * det(a) != 0, material -1..253, pad 0.  |V| and T are held to 2^26 voxels (TDT_REGION_BRUSH_CAP); T's size is known after the
 * count pass and checked before the list is allocated.
 * Errors, nothing written: a NULL struct or pointer, a limit exceeded, a bad op, a bad shape, NULL regions with a count above
 * 0, a LEAF value >= 254: TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  An empty tree, mask or dst box is
 * valid: T is empty.  Ordered after work queued on the context's stream; synchronous.
 * tdt_debug_xform_bricks: of the context's last transform call, out = {the aligned 8 x 8 x 8 bricks of the destination domain
 * (dst & G & a bounding box of the preimage of S's bounding box), those whose exact source box met S's bounding box and went
 * through the count and emit passes}; DESIGN.md has the scheme. */
#define TDT_XFORM_ONE 65536
typedef struct tdt_xform {
  int64_t t[3];                /* units of 2^-17 voxel, |t| <= 2^40 */
  int32_t a[9];                /* row-major, destination -> source, Q16, |a| <= 2^20 */
  int32_t material;            /* -1: the source voxel's; 0..253: this LEAF value */
  int32_t dst_lo[3], dst_hi[3];  /* inclusive box the result is clipped to (then to the grid); lo > hi on an axis: empty */
  int32_t pad[2];              /* must be 0 */
} tdt_xform;
#ifdef __cplusplus
static_assert(sizeof(tdt_xform) == 96, "tdt_xform is 96 bytes");
#else
_Static_assert(sizeof(tdt_xform) == 96, "tdt_xform is 96 bytes");
#endif
int tdt_octree_extract_transform(tdt_ctx *ctx, const tdt_xform *xf, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                                 size_t capacity, size_t *n_voxels);
int tdt_octree_transform(tdt_ctx *ctx, const tdt_xform *xf, int op, const tdt_region *regions, size_t n_regions, uint32_t *n_cells);
int tdt_debug_xform_bricks(const tdt_ctx *ctx, uint32_t out[2]);

/* ---- geodesic distance --------------------------------------------------------------------------------------------------------
 * How far is it from here if you must stay inside the object, or walk round the walls: reach fields, reach edits and shortest
 * paths.  N = 2^max_depth (slot 7), G = [0, N)^3, V = what tdt_octree_extract returns; nothing wraps around the grid.
 *   Medium P, the voxels a path may visit: TDT_MEDIUM_EMPTY = G \ V; TDT_MEDIUM_SOLID = V when `match` is -1, with `match` in
 *     0..253 only the voxels of V whose LEAF value is `match`.  With n_regions > 0, P is further intersected with the union M of
 *     the regions (tdt_region shapes, the exact integer test of region edits): here the mask constrains the PATHS, not only the
 *     report.  n_regions == 0: no mask.
 *   Steps: an offset d in {-1, 0, 1}^3 \ {0} has class k(d) = |dx| + |dy| + |dz| - 1 (0 across a face, 1 an edge, 2 a corner) and
 *     order t(d) = 9 (dx + 1) + 3 (dy + 1) + (dz + 1), tdt_octree_morph's.  A step p -> p + d is allowed when both ends are in P
 *     and w[k(d)] > 0, and costs w[k(d)].  w[0] is in 1..255, w[1] and w[2] in 0..255, 0 meaning no such step; no ordering between
 *     the three is assumed.  A diagonal step may pass between two voxels that are not in P: the project's meaning of
 *     26-connectivity, as in connected components and enclosed space.  {1, 0, 0} are 6-steps, {1, 1, 1} 26-steps, {3, 4, 5} the
 *     chamfer metric (about 3 x the Euclidean path length).
 *   Distance: seeds are {x, y, z} triples; one off the grid or not in P is ignored.  g(q), q in P, is the minimum over paths of
 *     allowed steps from any seed to q of the summed cost; a seed has g = 0.  g is a fixed point of the grid alone, so it does
 *     not depend on scheduling and compares bit for bit.  `max_cost` is in 0..2^30; the reach set is R = { q in P : g(q) <= max_cost }.
 *   Canonical shortest path from a goal q0 in R: while g(q_i) > 0, q_(i+1) = q_i + d for the first d in ascending t(d) whose step
 *     is allowed and has g(q_i + d) + w[k(d)] == g(q_i).  It ends on a seed.
 * tdt_octree_geodesic_field covers the inclusive box lo..hi, which must lie inside G and hold <= 2^26 voxels, in the layout and by
 * the count / capacity rules of tdt_octree_distance_field (field == NULL only sets *n_voxels; capacity below the count:
 * TDT_ERR_INVALID_VALUE with the count set): g(q) for q in R, -1 everywhere else (not in P, unreachable, beyond max_cost).
 * tdt_octree_extract_geodesic returns R as {x, y, z, m}, Morton-sorted, by tdt_octree_extract's rules; m is the voxel's own
 * material + 1 when `material` is -1 (SOLID only: with TDT_MEDIUM_EMPTY it is an error), else `material` + 1.  The tree, its
 * counter and its versions are untouched.
 * tdt_octree_edit_geodesic is tdt_octree_edit_voxels(op, that list), taken from the tree BEFORE the edit and never leaving the
 * device: all four ops, tdt_octree_compact's install rule on every replica of a multi-device context, a failure leaving all of
 * them unchanged, *n_cells on a misfit, exactly like tdt_octree_transform.
 * tdt_octree_geodesic_path returns the canonical path, path[0] = goal and the last point the seed reached, *cost = g(goal).  A
 * goal not in R: *n_points = 0, *cost = -1, TDT_OK.  path_xyz == NULL only counts; capacity below the count:
 * TDT_ERR_INVALID_VALUE with the count set.
 * Domain: the unit works on the box D = G cut by the bounding box of the regions' union (when masked), by bbox(V) (SOLID), and by
 * the bounding box of the in-grid seeds grown by floor(max_cost / w_min) on every side, w_min the smallest positive weight (a
 * step moves at most 1 per axis and costs at least w_min, so nothing outside is in R).  D must hold <= TDT_GEODESIC_DOMAIN_CAP
 * voxels, checked on the host before any volume over it is allocated (for TDT_MEDIUM_EMPTY before the tree is walked).  Over D
 * the unit allocates 4.5 bytes per voxel of its rows rounded out to multiples of 32 in x.  An empty D, no valid seed, an empty
 * tree or an empty mask are valid: R is empty.
 * Errors, nothing written: a NULL struct or required pointer, a bad medium / match / weight / max_cost / material / pad / op /
 * shape / box, NULL seeds or regions with a count above 0, a LEAF value >= 254, |V| or |R| above 2^26, the domain cap exceeded:
 * TDT_ERR_INVALID_VALUE; slot 0 or 7 unbound: TDT_ERR_INCOMPLETE.  Ordered after work queued on the context's stream;
 * synchronous.  The query forms answer from device_ids[0]. */
enum { TDT_MEDIUM_EMPTY = 0, TDT_MEDIUM_SOLID = 1 };
#define TDT_GEODESIC_DOMAIN_CAP (1u << 27)
typedef struct tdt_geodesic {
  int32_t medium;              /* TDT_MEDIUM_* */
  int32_t match;               /* SOLID: -1 any voxel, 0..253 this LEAF value only; EMPTY: must be -1 */
  int32_t w[3];                /* cost of a face / edge / corner step */
  int32_t max_cost;            /* 0..2^30 */
  int32_t material;            /* list and edit forms: -1 = the voxel's own (SOLID only), 0..253 = this LEAF value */
  int32_t pad;                 /* must be 0 */
} tdt_geodesic;
#ifdef __cplusplus
static_assert(sizeof(tdt_geodesic) == 32, "tdt_geodesic is 32 bytes");
#else
_Static_assert(sizeof(tdt_geodesic) == 32, "tdt_geodesic is 32 bytes");
#endif
int tdt_octree_geodesic_field(tdt_ctx *ctx, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                              size_t n_regions, const int32_t lo[3], const int32_t hi[3], int32_t *field, size_t capacity, size_t *n_voxels);
int tdt_octree_extract_geodesic(tdt_ctx *ctx, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                                size_t n_regions, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels);
int tdt_octree_edit_geodesic(tdt_ctx *ctx, int op, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                             size_t n_regions, uint32_t *n_cells);
int tdt_octree_geodesic_path(tdt_ctx *ctx, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                             size_t n_regions, const int32_t goal[3], int32_t *path_xyz, size_t capacity, size_t *n_points, int32_t *cost);
/* the relaxation passes of the context's last geodesic call that changed the volume (0: the seeds were the fixed point, or D was
 * empty); the host queues passes in batches of 8, so up to 8 more ran idle.  Measurement only. */
int tdt_debug_geodesic_passes(const tdt_ctx *ctx);

/* which build of the trace kernel the context's last trace launch ran: out = {form: 0 the literal float index, 1 the exact form of a
 * power-of-two cell_count, 2 per-cell thresholds (any other count); compile-time depth (0 = the general kernel); tree inside the LDS
 * table; whole-depth table; bricks; the build that skips multiplications by a scale of 1.0f}.  Every build writes the same pixels; this
 * lets a test tell a scene that fell back to the general kernel from one that runs its specialised build. */
int tdt_debug_last_variant(const tdt_ctx *ctx, int out[6]);
/* the launch geometry of that build: out = {threads per block, blocks that share a CU}.  1024 x 1 (four waves per SIMD) for every
 * build but the whole-depth ones, which run 256 x 5 (five waves per SIMD) unless TDT_FOUR_WAVES=1 was set when the context was
 * created. */
int tdt_debug_last_geometry(const tdt_ctx *ctx, int out[2]);
/* every scene-specialised build of the trace kernel the library holds, six ints per build in the order above; needs no context or
 * device.  *count receives the number of builds; the first min(capacity, *count) are written to rows (capacity 0: count only). */
int tdt_debug_trace_variants(int *rows, int capacity, int *count);
/* pass / lane statistics of the PRODUCT trace kernels (how many traversal and event passes the waves ran, how many lanes were live in
 * each code region: the STAT_* rows of csrc/tdt_rt.hip) since the last reset — collected only by a -DTDT_STATS build of the library
 * (tools/loss_budget.py builds one beside the product library; the product library answers TDT_ERR_INVALID_OPERATION).  The first
 * call switches the collection on; reset != 0 clears the totals after reading them.  out: n_words entries (0: the 34 totals) —
 * 34 totals (the last two: traversal passes of a whole-depth build that took the level walk, and the lanes in a band that sent them
 * there), then the time (100 MHz ticks) the first wave met the end of the pixel queue, then up to 8192 per-wave end times. */
int tdt_debug_stats(tdt_ctx *ctx, uint64_t *out, int n_words, int reset);
/* lane-utilisation diagnostics of the last tdt_dispatch_counted of this context (32 totals; layout in
 * csrc/trace_device.hpp `Counters`); development aid */
int tdt_debug_counters(tdt_ctx *ctx, uint64_t out[32]);
/* development aids, filled by tdt_dispatch_counted (tools/timeline.py, tools/pixel_log.py):
 * wave_ends: n <= 16384 + 256 entries — per-wave end times (100 MHz ticks; index = block * 16 + wave), then from
 * entry 16384 two 128-bin histograms (0.1 ms bins) of pixel durations: pixels finished while the queue still had
 * work / by waves that had seen its end.  pixel_log (only when TDT_PIXEL_LOG is set in the environment): 8 u32
 * per queue slot — traversal steps, path events, wave passes, start tick, end tick, wave, event passes, threshold. */
int tdt_debug_wave_ends(tdt_ctx *ctx, uint64_t *out, int n);
int tdt_debug_pixel_log(tdt_ctx *ctx, uint32_t *out, size_t n_u32);
/* exhaustive (all 2^32 inputs) check of the kernels' short correctly-rounded rcp (0) / sqrt (1) /
 * rsq (2) forms against the IEEE expressions, of v_fract_f32 against x - floor(x) for x >= 0 (4), and of the top-level
 * jump tables' claim (5: the 4-level table of LDS-resident trees, 7: the 5-level table of the others): for every coordinate
 * in [0,1) outside the table's bands and every cell index below its bounds (128 / 1024 / 8192 by level) the x decision of
 * treeLookup's first four / five levels is the coordinate's binary digit; and of the short form of CubeHit's normal (9: every
 * bit pattern of the dominant component x zeros / smaller values / ties / NaN on the other axes x ray directions with zero,
 * denormal, inf and NaN components: where its guard holds it returns the bits of the literal normalise-orient-normalise
 * sequence); and of the two one-parameter divisions taken through reciprocal + residual step (11: pow's (m - 1) / (m + 1) for
 * every mantissa, reflectance's (1 - x) / (1 + x) for every x); and of the claim the bricks of depth-8 trees rest on (13:
 * fl(v + f) - v depends on an integer v < 2^22 only through floor(log2 v), for every f in [0, 1); 15: the bands of their
 * level-5 table, one per cell index instead of one for all).  *mismatches must be 0.  Modes 3, 6, 8, 10, 12, 14 and 16 check the
 * harness: the raw reciprocal seed, the claims without the bands, the short normal without its guard, the divisions without
 * the residual step, the wrong binade, and half the band, must fail.
 * Mode 17 reads the cells buffer and octree uniforms bound to ctx (max_depth 5 or 6, a tree the whole-depth table serves;
 * TDT_ERR_INVALID_OPERATION otherwise): for every one of the 8^max_depth table positions, what a traversal step decodes from
 * the table's entry (cell corner, cell size, value, LEAF or not) must equal, bit for bit, what the 16-bit entry's decode computes
 * from the position and what the level walk over the packed node table ends on.
 * Mode 18, on the same bound tree: the table in its plane form (entries that carry three byte offsets into a per-block table of
 * padded slab planes).  For every position the six planes fetched through the entry's offsets must equal, bit for bit, the planes
 * the arithmetic form computes from the 16-bit entry, the bound octree corner and scale.
 * Mode 19, on the same bound tree: the lanes in a band that the five-wave whole-depth builds serve from the table instead of the
 * level walk.  For every integer n of 2^max_depth x, every float x in [0, 1) whose 2^max_depth x lies within the band (2^-11) of n
 * (n = 0: the first and last 32 floats of every binade) and every finest-level (y, z): where the classification does not leave the
 * lane to the walk, what a step reads through the table entry of the resolved position must equal, bit for bit, what the level walk
 * over the packed node table ends on (slab planes, cell size, LEAF or not, a LEAF's value).  The outcome counts follow the mismatches
 * in tdt_debug_counters: [1] lanes resolved to position n, [2] to n - 2^j, [3] lanes left to the walk. */
int tdt_selftest(tdt_ctx *ctx, int which, uint64_t *mismatches);
/* A cell_count that is not a power of two (the reference's own: 100000, main.rs:459) takes treeLookup's x index
 * (raytracer.comp:376-378) through two per-cell thresholds on the level's coordinate instead of the float formula (csrc/
 * trace_device.hpp, x_thresholds).  This checks that claim exhaustively for one (cell_count, inv_cell_count) pair: every
 * coordinate f in [0,1) x every cell index below n_cells (<= 65535) against the literal formula; *mismatches must be 0.
 * *shape_ok = 0: some cell's index is not a two-step function of f — such a scene runs the literal kernel.  shift != 0 moves
 * every threshold by that many ulps first (the harness: mismatches must appear). */
int tdt_selftest_index(tdt_ctx *ctx, int32_t cell_count, float inv_cell_count, uint32_t n_cells, int shift, uint64_t *mismatches,
                       int *shape_ok);

#ifdef __cplusplus
}
#endif
#endif /* TDT_RT_H */
