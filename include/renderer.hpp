// renderer.hpp — C++ mirror of the reference's `src/renderer` module over the C ABI (tdt_rt.h / tdt_host.h).
//
// The reference's host is Rust (no toolchain in this image), so this header plays the part of
// src/renderer/{mod,program,compute_shader,vbo,texture,vao,octree,camera}.rs for a C++ host: same type and
// method names, same argument meaning, same error behaviour — `Result<T, InitializeErr>` becomes "returns T or
// throws InitializeErr" (the reference `.unwrap()`s nearly every one of them: an uncaught throw is that panic).
// Header-only; link with -ltdtrt -ltdthost.  Every item cites the reference lines it stands for.
#pragma once

#include <array>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "tdt_host.h"
#include "tdt_rt.h"

namespace renderer {

// renderer/mod.rs:20-24
enum class Material : uint32_t { Lambertian = 0, Metal, Dielectric };

// renderer/mod.rs:28-59 (InitializeErr + its Display)
struct InitializeErr {
  enum Kind { GL, VariableNotFound, TypedVariableNotFound, InvalidCStr } kind;
  unsigned code = 0;            // GL(code)
  std::string name, type_str;   // VariableNotFound(name) / TypedVariableNotFound(name, type)
  std::string detail;           // message of the C ABI for this failure

  InitializeErr var_into_typed(const std::string &t) const {   // mod.rs:36-41
    InitializeErr e = *this;
    if (e.kind == VariableNotFound) { e.kind = TypedVariableNotFound; e.type_str = t; }
    return e;
  }
  std::string to_string() const {                              // impl Display, mod.rs:44-59
    switch (kind) {
      case GL:
        if (code == 0x0500) return "gl error: invalid enum";
        if (code == 0x0501) return "gl error: invalid value";
        if (code == 0x0502) return "gl error: invalid operation";
        return "got gl error code: " + std::to_string(code);
      case VariableNotFound: return "failed to locate uniform " + name;
      case TypedVariableNotFound: return "failed to locate uniform " + name + " with type " + type_str;
      default: return detail;
    }
  }
};

using Vector3f = std::array<float, 3>;   // cgmath::Vector3<f32>
using Vector3i = std::array<int32_t, 3>;

// The GL context the render thread makes current (main.rs:105-112): one HIP device + stream.
class Context {
 public:
  explicit Context(int device = 0, void *stream = nullptr) {
    if (int rc = tdt_ctx_create(device, stream, &ctx_)) throw InitializeErr{InitializeErr::GL, (unsigned)rc, "", "", tdt_last_error(nullptr)};
  }
  ~Context() { tdt_ctx_destroy(ctx_); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  tdt_ctx *raw() const { return ctx_; }
  // check_for_gl_error (mod.rs:62-68): GL's sticky error is the return code of every call here
  void check(int rc) const {
    if (rc != TDT_OK) throw InitializeErr{InitializeErr::GL, (unsigned)rc, "", "", tdt_last_error(ctx_)};
  }
  void finish() const { check(tdt_finish(ctx_)); }   // glFinish
 private:
  tdt_ctx *ctx_ = nullptr;
};

// renderer/vbo.rs:9-55.  `target` / `usage` are accepted for signature parity and ignored (a HIP buffer has neither).
class VertexBufferObject {
 public:
  template <class T>
  static VertexBufferObject new_(Context &ctx, const std::vector<T> &data, unsigned /*target*/ = 0, unsigned /*usage*/ = 0) {
    VertexBufferObject v;
    v.ctx_ = &ctx;
    ctx.check(tdt_buffer_create(ctx.raw(), data.data(), data.size() * sizeof(T), &v.buf_));
    return v;
  }
  tdt_buffer *id() const { return buf_; }   // vbo.rs:11 `id`
  void sub_data(size_t offset, size_t bytes, const void *data) const { ctx_->check(tdt_buffer_sub_data(buf_, offset, bytes, data)); }
  template <class T> std::vector<T> read(size_t count) const {
    std::vector<T> out(count);
    ctx_->check(tdt_buffer_read(buf_, 0, count * sizeof(T), out.data()));
    return out;
  }
 private:
  Context *ctx_ = nullptr;
  tdt_buffer *buf_ = nullptr;
};

// gl::BindBufferBase(target, slot, id) as main.rs:352-448 and octree.rs:67-144 call it
inline void bind_buffer_base(Context &ctx, int target, unsigned slot, const VertexBufferObject &vbo) {
  ctx.check(tdt_bind_buffer_base(ctx.raw(), target, slot, vbo.id()));
}

// renderer/vao.rs:32-74: vertex-attribute state has no effect on SSBO access ("vao might not be needed",
// main.rs:232); kept so that host code written against the reference compiles unchanged.
struct VertexAttributePointer { unsigned location, size, offset; };
class VertexArrayObject {
 public:
  template <class T> static VertexArrayObject new_(const std::vector<VertexAttributePointer> &, const tdt_buffer *, unsigned) { return {}; }
  template <class T> void append_vbo(const std::vector<VertexAttributePointer> &, const tdt_buffer *, unsigned) const {}
  void bind() const {}
  static void unbind() {}
};

class ComputeShader;

// renderer/texture.rs:7-92
class Texture {
 public:
  // new_2d(TEXTURE0, 0, RGBA32F, RGBA, w, h) texture.rs:47-75; bind = false (NEW): an image that is not the render target (a guide)
  static Texture new_2d(Context &ctx, int width, int height, bool bind = true) {
    Texture t;
    t.ctx_ = &ctx; t.w_ = width; t.h_ = height;
    ctx.check(tdt_image_create_rgba32f(ctx.raw(), width, height, &t.img_));
    if (bind) t.bind();
    return t;
  }
  tdt_image *id() const { return img_; }
  void bind() const { ctx_->check(tdt_bind_image(ctx_->raw(), 0, img_)); }   // BindImageTexture(unit 0)
  int width() const { return w_; }
  int height() const { return h_; }
  int depth() const { return 1; }
  std::vector<float> read() const {   // NEW: the reference never reads back (quad.frag samples the texture)
    std::vector<float> px((size_t)w_ * h_ * 4);
    ctx_->check(tdt_image_read(img_, px.data()));
    return px;
  }
  // NEW: the frame as the quad pass presents it (quad.frag:10), RGBA8, converted on the GPU
  void read_rgba8(bool top_down, uint8_t *dst) const { ctx_->check(tdt_image_read_rgba8(img_, top_down ? 1 : 0, dst)); }
  // NEW: the edge-stopping a-trous filter, in place (tdt_image_denoise): `passes` 0..8 passes of step 1, 2, 4, .. that average only
  // pixels whose guide texels (ComputeShader::dispatch_guide, an image of this size) carry the same surface key.  Asynchronous.
  void denoise(const Texture &guide, int passes) const { ctx_->check(tdt_image_denoise(img_, guide.img_, passes, 0)); }
  // NEW: a guide image's texels {kind, material, plane, t}
  std::vector<tdt_guide_texel> read_guide() const {
    std::vector<tdt_guide_texel> g((size_t)w_ * h_);
    ctx_->check(tdt_image_read(img_, reinterpret_cast<float *>(g.data())));
    return g;
  }
  // NEW: every byte to zero (tdt_image_clear): before accumulating a sample range that does not start at sample 0; a
  // multi-device context's image is refused
  void clear() const { ctx_->check(tdt_image_clear(img_)); }
  // NEW: temporal reprojection (tdt_image_reproject) with this texture as the frame's running sums of `spp` samples: hist_out
  // receives the sums plus, where the earlier frame (its view, guide and history: all three or none) saw the same surface point, at
  // most max_samples of that frame's history; mean_out (may be this texture, or null) receives rgb / sample count.  `guide` is what
  // shader.dispatch_guide(guide, sample) wrote under the shader's current camera.  Asynchronous.  (Defined below ComputeShader.)
  void reproject(const ComputeShader &shader, int sample, const Texture &guide, int spp, const tdt_view *prev_view, const Texture *prev_guide,
                 const Texture *prev_hist, float max_samples, const Texture &hist_out, const Texture *mean_out = nullptr) const;
  // NEW: the variance of the luminance of rgb into alpha (tdt_image_variance): 0 for kind-0 pixels, from `moments` (what
  // reproject_moments wrote, or null) where a pixel has at least min_frames frames behind it, from its 7x7 same-key neighbourhood
  // elsewhere.  Asynchronous.
  void variance(const Texture &guide, const Texture *moments = nullptr, float min_frames = 4.0f) const {
    ctx_->check(tdt_image_variance(img_, guide.img_, moments ? moments->img_ : nullptr, min_frames, 0));
  }
  // NEW: denoise's passes with a luminance edge-stopping weight scaled by the variance in alpha (tdt_image_denoise_variance):
  // max(lim - d^2, 0), lim = sigma^2 * (3x3 prefiltered variance of the centre) + floor.  Asynchronous.
  void denoise_variance(const Texture &guide, int passes, float sigma, float floor = 0.0f) const {
    ctx_->check(tdt_image_denoise_variance(img_, guide.img_, passes, sigma, floor, 0));
  }
  // NEW: reproject, and moments_out receives the luminance moments (m1, m2, frames, 0) joined with prev_moments' wherever the
  // history was found (tdt_image_reproject_moments); prev_moments comes and goes with the other prev_*.  (Defined below ComputeShader.)
  void reproject_moments(const ComputeShader &shader, int sample, const Texture &guide, int spp, const tdt_view *prev_view,
                         const Texture *prev_guide, const Texture *prev_hist, const Texture *prev_moments, float max_samples,
                         const Texture &hist_out, const Texture &moments_out, const Texture *mean_out = nullptr) const;
  // NEW: guide-keyed upsampling into this texture (tdt_image_upsample): `src`, sums traced at reduced resolution, spread over this
  // image's pixels, each taking only texels whose key in src_guide (of src's size) equals its own in dst_guide (of this size):
  // validated bilinear, else the mean of the same-key texels of the 4x4 ring, else the nearest texel.  Asynchronous.
  void upsample(const Texture &dst_guide, const Texture &src, const Texture &src_guide) const {
    ctx_->check(tdt_image_upsample(img_, dst_guide.img_, src.img_, src_guide.img_, 0));
  }
  // NEW: the sampling controller (tdt_image_adapt) with this texture as the running sums: after a batch of spp_count samples for
  // the live pixels of state_in, state_out receives their updated (L, m2, n, w), w negated where the pixel stops.  guide may be
  // null.  state_out is the mask of the next ComputeShader::dispatch_accumulate_masked.  Asynchronous.
  void adapt(const Texture *guide, const Texture &state_in, const Texture &state_out, int spp_count, const tdt_adapt &a) const {
    ctx_->check(tdt_image_adapt(img_, guide ? guide->img_ : nullptr, state_in.img_, state_out.img_, spp_count, &a, 0));
  }
  // NEW: running sums to means by the sample counts of `state`, alpha = the variance of the mean luminance (tdt_image_adapt_mean)
  void adapt_mean(const Texture &state) const { ctx_->check(tdt_image_adapt_mean(img_, state.img_, 0)); }
  // NEW: a voxel list {x, y, z, m} (4 ints each, m ignored) drawn over this texture, in place (tdt_image_overlay): the pixels whose
  // voxel in `ids` (ComputeShader::dispatch_voxel_ids, an image of this size) is in the list are blended with style.fill, those
  // within style.edge_width pixels of the selection's border with style.edge.  First hit only.  The passes are queued.
  void overlay(const Texture &ids, const std::vector<int32_t> &voxels_xyzm, const tdt_overlay &style) const {
    ctx_->check(tdt_image_overlay(img_, ids.img_, voxels_xyzm.empty() ? nullptr : voxels_xyzm.data(), voxels_xyzm.size() / 4, &style));
  }
  // NEW: the distinct voxels {x, y, z, material + 1} visible in this voxel-id image inside rect = {x0, y0, x1, y1} (inclusive,
  // clipped; null: the whole image), in Morton order (tdt_image_extract_voxels): the brush of Octree::edit_voxels
  std::vector<int32_t> extract_voxels(const int32_t *rect = nullptr) const {
    size_t n = 0;
    ctx_->check(tdt_image_extract_voxels(img_, rect, nullptr, 0, &n));
    std::vector<int32_t> v(n * 4);
    if (n) ctx_->check(tdt_image_extract_voxels(img_, rect, v.data(), n, &n));
    return v;
  }
 private:
  Context *ctx_ = nullptr;
  tdt_image *img_ = nullptr;
  int w_ = 0, h_ = 0;
};

// renderer/program.rs:9-174: the uniform-by-name setters (the program object itself is the kernel)
class Program {
 public:
  Program() = default;
  Program(Context &ctx, tdt_compute *c) : ctx_(&ctx), c_(c) {}
  void bind() const {}               // program.rs:21-25 glUseProgram: nothing to do
  static void unbind() {}
  tdt_compute *id() const { return c_; }
  void set_i32(const std::string &name, int32_t v) const { uniform(tdt_set_i32(c_, name.c_str(), v), name, "i32"); }                                  // :35-45
  void set_f32(const std::string &name, float v) const { uniform(tdt_set_f32(c_, name.c_str(), v), name, "f32"); }                                    // :61-71
  void set_vector3_f32(const std::string &name, const Vector3f &v) const { uniform(tdt_set_vec3f(c_, name.c_str(), v[0], v[1], v[2]), name, "vec3 f32"); }   // :73-83
  void set_vector3_i32(const std::string &name, const Vector3i &v) const { uniform(tdt_set_vec3i(c_, name.c_str(), v[0], v[1], v[2]), name, "vec3 i32"); }   // :48-58
 private:
  void uniform(int rc, const std::string &name, const char *type) const {   // register_uniform + var_into_typed, :144-165
    if (rc == TDT_ERR_VARIABLE_NOT_FOUND) throw InitializeErr{InitializeErr::VariableNotFound, 0, name, "", tdt_last_error(ctx_->raw())}.var_into_typed(type);
    ctx_->check(rc);
  }
  Context *ctx_ = nullptr;
  tdt_compute *c_ = nullptr;
};

// renderer/compute_shader.rs:10-38
class ComputeShader {
 public:
  Program program;
  // Shader::from_resources(res, "shaders/raytracer.comp" | "shaders/octree_update.comp") + Program::from_shaders +
  // ComputeShader::new (main.rs:156-160, 226-230): `kind` names which of the two compute programs
  static ComputeShader new_(Context &ctx, int kind = TDT_PROGRAM_RAYTRACER) {
    ComputeShader cs;
    tdt_compute *c = nullptr;
    ctx.check(tdt_compute_create(ctx.raw(), kind, &c));
    cs.program = Program(ctx, c);
    cs.ctx_ = &ctx;
    ctx.check(tdt_compute_group_size(c, cs.group_size_));     // COMPUTE_WORK_GROUP_SIZE, compute_shader.rs:18
    return cs;
  }
  void dispatch_compute(int width, int height, int depth) const {   // compute_shader.rs:28-38 (floor-div groups inside)
    ctx_->check(tdt_dispatch_compute(program.id(), width, height, depth));
  }
  const int *group_size() const { return group_size_; }
  Context &context() const { return *ctx_; }
  // NEW (the reference has no ray query): what the primary ray of each pixel (x, y) and sample `sample` hits first, traced from
  // this program's camera uniforms with the bits the renderer traces (tdt_pick_pixels); `rays` (may be null) receives the rays
  std::vector<tdt_ray_hit> pick(const std::vector<std::array<int32_t, 2>> &xy, int sample = 0, std::vector<float> *rays = nullptr) const {
    std::vector<tdt_ray_hit> out(xy.size());
    if (rays) rays->assign(xy.size() * 6, 0.0f);
    ctx_->check(tdt_pick_pixels(program.id(), xy.empty() ? nullptr : xy[0].data(), xy.size(), sample, rays ? rays->data() : nullptr, out.data()));
    return out;
  }
  // NEW: the first hit of every pixel on the device (tdt_dispatch_guide): texel (x, y) of `guide` receives the surface key and the
  // depth of the primary ray of pixel (x, y), sample `sample`, of this program's camera; flags: TDT_GUIDE_ALL_MATERIALS.  Asynchronous.
  void dispatch_guide(const Texture &guide, int sample = 0, uint32_t flags = 0) const {
    ctx_->check(tdt_dispatch_guide(program.id(), guide.id(), sample, flags));
  }
  // NEW: the voxel a click on every pixel would act on (tdt_dispatch_voxel_ids): texel (x, y) of `ids` receives tdt_pick_grid_voxel
  // of that pixel's pick as a tdt_voxel_id_texel; place = 0 the voxel behind the face, 1 the empty cell in front.  Asynchronous.
  void dispatch_voxel_ids(const Texture &ids, int place = 0, int sample = 0) const {
    ctx_->check(tdt_dispatch_voxel_ids(program.id(), ids.id(), place, sample));
  }
  // NEW: tdt_dispatch_accumulate for the covered pixels whose texel of `mask` has w >= 0 (tdt_dispatch_accumulate_masked); every
  // other pixel keeps its texel and its carry.  A Texture::adapt state image is such a mask.
  void dispatch_accumulate_masked(int width, int height, int depth, int spp_begin, int spp_count, void *carry, const Texture &mask) const {
    ctx_->check(tdt_dispatch_accumulate_masked(program.id(), width, height, depth, spp_begin, spp_count, carry, mask.id()));
  }
  // NEW: a snapshot of this program's camera uniforms (tdt_compute_view): what a later frame reprojects into
  tdt_view view() const {
    tdt_view v;
    ctx_->check(tdt_compute_view(program.id(), &v));
    return v;
  }
 private:
  Context *ctx_ = nullptr;
  int group_size_[3] = {0, 0, 0};
};

inline void Texture::reproject(const ComputeShader &shader, int sample, const Texture &guide, int spp, const tdt_view *prev_view,
                               const Texture *prev_guide, const Texture *prev_hist, float max_samples, const Texture &hist_out,
                               const Texture *mean_out) const {
  ctx_->check(tdt_image_reproject(shader.program.id(), sample, guide.img_, img_, spp, prev_view, prev_guide ? prev_guide->img_ : nullptr,
                                  prev_hist ? prev_hist->img_ : nullptr, max_samples, hist_out.img_, mean_out ? mean_out->img_ : nullptr, 0));
}

inline void Texture::reproject_moments(const ComputeShader &shader, int sample, const Texture &guide, int spp, const tdt_view *prev_view,
                                       const Texture *prev_guide, const Texture *prev_hist, const Texture *prev_moments, float max_samples,
                                       const Texture &hist_out, const Texture &moments_out, const Texture *mean_out) const {
  ctx_->check(tdt_image_reproject_moments(shader.program.id(), sample, guide.img_, img_, spp, prev_view, prev_guide ? prev_guide->img_ : nullptr,
                                          prev_hist ? prev_hist->img_ : nullptr, prev_moments ? prev_moments->img_ : nullptr, max_samples,
                                          hist_out.img_, moments_out.img_, mean_out ? mean_out->img_ : nullptr, 0));
}

// renderer/octree.rs:10-183
class Octree {
 public:
  VertexArrayObject vao;
  static Octree new_(Vector3f min_point, float scale, int max_depth, int cell_count, int active_cell_count,
                     int max_traversal_iter, VertexArrayObject vao = {}) {                      // octree.rs:26-38
    Octree o;
    o.min_point_ = min_point; o.scale_ = scale; o.max_depth_ = max_depth; o.cell_count_ = cell_count;
    o.active_cell_count_ = active_cell_count; o.max_traversal_iter_ = max_traversal_iter; o.vao = vao;
    o.block_distance_ = scale / (float)(1u << (max_depth < 31 ? max_depth : 31));               // scale / 2^max_depth
    return o;
  }
  void init_global_buffers(Context &ctx) {                                                       // octree.rs:40-151
    floats_ = VertexBufferObject::new_<float>(ctx, {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_,
                                                    1.0f / (float)cell_count_});                // :44-50
    bind_buffer_base(ctx, TDT_SHADER_STORAGE_BUFFER, 6, floats_);
    ints_ = VertexBufferObject::new_<int32_t>(ctx, {max_depth_, max_traversal_iter_, cell_count_});   // :76-81
    bind_buffer_base(ctx, TDT_SHADER_STORAGE_BUFFER, 7, ints_);
    counter_ = VertexBufferObject::new_<int32_t>(ctx, {active_cell_count_});                    // :105-110
    bind_buffer_base(ctx, TDT_ATOMIC_COUNTER_BUFFER, 0, counter_);
    delta_ = VertexBufferObject::new_<float>(ctx, std::vector<float>(1000, 0.0f));              // :124-128
    bind_buffer_base(ctx, TDT_SHADER_STORAGE_BUFFER, 5, delta_);
  }
  float block_distance() const { return block_distance_; }
  float scale() const { return scale_; }
  Vector3f min_point() const { return min_point_; }
  bool point_inside(const Vector3f &p) const {                                                   // :165-168
    return p[0] >= min_point_[0] && p[1] >= min_point_[1] && p[2] >= min_point_[2] && p[0] <= min_point_[0] + scale_ &&
           p[1] <= min_point_[1] + scale_ && p[2] <= min_point_[2] + scale_;
  }
  void update_vbo(const std::vector<float> &delta, size_t len, const ComputeShader &update_compute) const {   // :170-183
    const float LOCAL_GROUP_SIZE_X = 32.0f * 32.0f;
    delta_.sub_data(0, len * sizeof(float), delta.data());       // BufferSubData of the generic SSBO target = the delta buffer (:144,:174)
    const float x_schedule = (float)len * 0.2f;
    const int dispatch_count = (int)((float)len * 0.2f);
    const float q = x_schedule / LOCAL_GROUP_SIZE_X;
    if (q - (float)(long long)q != 0.0f) update_compute.dispatch_compute(0, dispatch_count, 0);
    else update_compute.dispatch_compute(dispatch_count, 1, 1);
  }
  const VertexBufferObject &counter() const { return counter_; }
  // NEW: rays {origin, direction} (6 floats each, normalised directions) through the bound octree (tdt_raycast)
  std::vector<tdt_ray_hit> raycast(const Context &ctx, const std::vector<float> &rays) const {
    std::vector<tdt_ray_hit> out(rays.size() / 6);
    ctx.check(tdt_raycast(ctx.raw(), rays.data(), out.size(), out.data()));
    return out;
  }
  // NEW: the bound tree read back as voxels {x, y, z, material + 1} (4 ints each), in Morton order (tdt_octree_extract)
  std::vector<int32_t> voxels(const Context &ctx) const {
    size_t n = 0;
    ctx.check(tdt_octree_extract(ctx.raw(), nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract(ctx.raw(), v.data(), n, &n));
    return v;
  }
  // NEW: {reachable cells, leaf nodes, voxels, highest cell reached, cells the buffer holds, counter} (tdt_octree_census)
  std::array<int64_t, 6> census(const Context &ctx) const {
    std::array<int64_t, 6> c{};
    ctx.check(tdt_octree_census(ctx.raw(), c.data()));
    return c;
  }
  // NEW: what the reference's TODOs (octree_update.comp:86-94) would reclaim: the bound cells buffer rewritten in place into the
  // canonical tree of its voxels, the counter reset to its size (tdt_octree_compact); returns the number of cells
  uint32_t compact(const Context &ctx) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_compact(ctx.raw(), &n));
    return n;
  }
  // NEW: op (TDT_REGION_*) over the union of `regions`, brush material 0..253; the bound tree rebuilt in place in canonical
  // form, merged LEAFs included (tdt_octree_edit_region); returns the number of cells
  uint32_t edit_region(const Context &ctx, int op, const std::vector<tdt_region> &regions, int32_t material) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_region(ctx.raw(), op, regions.empty() ? nullptr : regions.data(), regions.size(), material, &n));
    return n;
  }
  // NEW: op over a voxel list {x, y, z, material + 1} (last duplicate wins, off-grid voxels dropped; tdt_octree_edit_voxels)
  uint32_t edit_voxels(const Context &ctx, int op, const std::vector<int32_t> &voxels_xyzm) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_voxels(ctx.raw(), op, voxels_xyzm.empty() ? nullptr : voxels_xyzm.data(), voxels_xyzm.size() / 4, &n));
    return n;
  }
  // NEW: a brush click: pick pixel (x, y) of the raytracer's camera (sample 0) and on a hit apply `op` over a TDT_SHAPE_SPHERE
  // of radius `size` or a TDT_SHAPE_BOX of half-width `size` centred on the grid voxel in front of the face (SET / FILL) or
  // behind it (PAINT / CLEAR) (tdt_pick_grid_voxel).  Returns whether an edit ran; *hit receives the pick, *n_cells the size.
  bool brush(const ComputeShader &raytracer, int x, int y, int shape, int size, int op, int32_t material, tdt_ray_hit *hit = nullptr,
             uint32_t *n_cells = nullptr) const {
    const tdt_ray_hit h = raytracer.pick({{{x, y}}}, 0)[0];
    if (hit) *hit = h;
    const float floats[7] = {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_, 1.0f / (float)cell_count_};   // :44-50
    const int32_t ints[3] = {max_depth_, max_traversal_iter_, cell_count_};
    const int place = op == TDT_REGION_SET || op == TDT_REGION_FILL ? 1 : 0;
    int32_t c[3];
    if (tdt_pick_grid_voxel(&h, floats, ints, place, c) != 0) return false;                  // miss / stale record / outside
    tdt_region r{};
    r.shape = shape;
    for (int a = 0; a < 3; a++) r.a[a] = c[a];
    if (shape == TDT_SHAPE_SPHERE) r.b[0] = size;
    else for (int a = 0; a < 3; a++) { r.a[a] = c[a] - size; r.b[a] = c[a] + size; }
    const uint32_t n = edit_region(raytracer.context(), op, {r}, material);
    if (n_cells) *n_cells = n;
    return true;
  }
  // NEW: a brush pulled along a path (tdt_octree_edit_stroke): op (TDT_REGION_*) over the voxels within `radius` of the segments
  // between `points_xyz` (voxel coordinates, on or off the grid) — a TDT_SHAPE_SPHERE nib sweeps capsules, a TDT_SHAPE_BOX nib of
  // half-width `radius` swept cubes.  `segments` empty and polyline = true: the polyline of the points (one point: a dab);
  // otherwise pairs of point indices (i == j: a dab).  material 0..253 for every segment or, with `materials`, material + 1 per
  // segment (the highest covering segment wins).  The list never leaves the device; returns the number of cells.
  uint32_t stroke(const Context &ctx, int op, const std::vector<int32_t> &points_xyz, int shape, int radius, int32_t material,
                  const std::vector<uint32_t> &segments = {}, bool polyline = true, const std::vector<int32_t> &materials = {}) const {
    static const uint32_t none[2] = {0, 0};
    const tdt_stroke s = stroke_of(points_xyz, shape, radius, material, segments, polyline, materials, none);
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_stroke(ctx.raw(), op, &s, &n));
    return n;
  }
  // NEW: the tree's voxels that stroke covers, {x, y, z, material + 1} with the tree's own materials, in Morton order
  // (tdt_octree_extract_stroke): the undo record of a CLEAR or PAINT stroke (edit_voxels(TDT_REGION_SET, it) puts them back)
  std::vector<int32_t> extract_stroke(const Context &ctx, const std::vector<int32_t> &points_xyz, int shape, int radius,
                                      const std::vector<uint32_t> &segments = {}, bool polyline = true) const {
    static const uint32_t none[2] = {0, 0};
    const tdt_stroke s = stroke_of(points_xyz, shape, radius, 0, segments, polyline, {}, none);
    size_t n = 0;
    ctx.check(tdt_octree_extract_stroke(ctx.raw(), &s, nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_stroke(ctx.raw(), &s, v.data(), n, &n));
    return v;
  }
  // NEW: a brush dragged over pixels: one batched pick of all of them (tdt_pick_pixels, sample 0), every hit turned into the grid
  // voxel in front of the face (SET / FILL) or behind it (PAINT / CLEAR) (tdt_pick_grid_voxel), consecutive hits joined by
  // segments, a miss breaking the stroke and a hit between two misses left as a dab; then stroke() of those points
  // (tdt_octree_edit_stroke).  Returns the number of cells; *points_xyz receives the points used.  No hit: the empty stroke.
  uint32_t stroke(const ComputeShader &raytracer, const std::vector<std::array<int32_t, 2>> &pixels, int shape, int radius, int op,
                  int32_t material, std::vector<int32_t> *points_xyz = nullptr) const {
    const std::vector<tdt_ray_hit> hits = raytracer.pick(pixels, 0);
    const float floats[7] = {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_, 1.0f / (float)cell_count_};   // :44-50
    const int32_t ints[3] = {max_depth_, max_traversal_iter_, cell_count_};
    const int place = op == TDT_REGION_SET || op == TDT_REGION_FILL ? 1 : 0;
    std::vector<int32_t> pts;
    std::vector<uint32_t> seg;
    std::vector<char> joined;
    bool prev = false;
    for (const tdt_ray_hit &h : hits) {
      int32_t c[3];
      if (tdt_pick_grid_voxel(&h, floats, ints, place, c) != 0) { prev = false; continue; }   // miss / stale record / outside
      const uint32_t i = (uint32_t)(pts.size() / 3);
      pts.insert(pts.end(), c, c + 3);
      joined.push_back(0);
      if (prev) { seg.push_back(i - 1); seg.push_back(i); joined[i - 1] = joined[i] = 1; }
      prev = true;
    }
    for (uint32_t i = 0; i < joined.size(); i++) if (!joined[i]) { seg.push_back(i); seg.push_back(i); }
    if (points_xyz) *points_xyz = pts;
    return stroke(raytracer.context(), op, pts, shape, radius, material, seg, false);
  }
  // NEW: the tree's exposed faces labelled into coplanar face regions (tdt_octree_face_regions): the table, numbered in the order
  // of each region's first face; faces / labels (may be null) receive the 1 x 1 quads of extract_surface(merge = 0) under the same
  // mask and the region of each.  Labels once where it can, as components() does: the arrays are sized by `capacity`, and only a
  // tree with more faces or regions is labelled again, into arrays of the sizes the first call reported.
  std::vector<tdt_face_region> face_regions(const Context &ctx, int connectivity, int match, const std::vector<tdt_region> &mask = {},
                                            std::vector<tdt_quad> *faces = nullptr, std::vector<uint32_t> *labels = nullptr,
                                            size_t capacity = 4096) const {
    size_t nf = 0, nr = 0;
    std::vector<tdt_face_region> table(capacity ? capacity : 1);
    size_t fcap = (faces || labels) ? (capacity ? capacity : 1) : 0;
    auto run = [&]() {
      if (faces) faces->assign(fcap, tdt_quad{});
      if (labels) labels->assign(fcap, 0u);
      return tdt_octree_face_regions(ctx.raw(), connectivity, match, mask.empty() ? nullptr : mask.data(), mask.size(),
                                     faces ? faces->data() : nullptr, labels ? labels->data() : nullptr, fcap, &nf, table.data(), table.size(), &nr);
    };
    int rc = run();
    if (rc == TDT_ERR_INVALID_VALUE && (nr > table.size() || (fcap && nf > fcap))) {
      table.resize(nr);
      if (fcap) fcap = nf;
      rc = run();
    }
    ctx.check(rc);
    table.resize(nr);
    if (faces) faces->resize(nf);
    if (labels) labels->resize(nf);
    return table;
  }
  // NEW: the face regions under the seeds {x, y, z, f} swept by the signed distance of `opt` (tdt_octree_extract_faces), as a
  // voxel list {x, y, z, material + 1} in Morton order — TDT_FACES_COLUMNS: the columns themselves (the preview; what
  // Texture::overlay takes); TDT_FACES_TREE: the tree's voxels they cover, with the tree's materials (the undo record of a push,
  // a paint or a SET pull: edit_voxels(TDT_REGION_SET, it) puts them back)
  std::vector<int32_t> extract_faces(const Context &ctx, const tdt_faces &opt, const std::vector<int32_t> &seeds_xyzf, int what = TDT_FACES_COLUMNS,
                                     const std::vector<tdt_region> &mask = {}) const {
    const int32_t *s = seeds_xyzf.empty() ? nullptr : seeds_xyzf.data();
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    size_t n = 0;
    ctx.check(tdt_octree_extract_faces(ctx.raw(), &opt, s, seeds_xyzf.size() / 4, r, mask.size(), what, nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_faces(ctx.raw(), &opt, s, seeds_xyzf.size() / 4, r, mask.size(), what, v.data(), n, &n));
    return v;
  }
  // NEW: op over those columns without the list leaving the device (tdt_octree_edit_faces): pull (TDT_REGION_FILL / SET, distance
  // > 0), push (TDT_REGION_CLEAR, distance < 0), paint a face (TDT_REGION_PAINT, distance -1).  Returns the number of cells.
  uint32_t extrude(const Context &ctx, int op, const tdt_faces &opt, const std::vector<int32_t> &seeds_xyzf,
                   const std::vector<tdt_region> &mask = {}) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_faces(ctx.raw(), op, &opt, seeds_xyzf.empty() ? nullptr : seeds_xyzf.data(), seeds_xyzf.size() / 4,
                                    mask.empty() ? nullptr : mask.data(), mask.size(), &n));
    return n;
  }
  // NEW: the face under the cursor: pick pixel (x, y) of the raytracer's camera (sample 0), turn the hit into the seed {x, y, z, f}
  // (tdt_pick_face) and extrude() the face region that holds it.  Returns whether an edit ran (a miss, a stale record or a hit
  // outside the octree: none); seed (may be null) receives the four ints, *n_cells the size.
  bool extrude(const ComputeShader &raytracer, int x, int y, int op, const tdt_faces &opt, const std::vector<tdt_region> &mask = {},
               int32_t *seed = nullptr, uint32_t *n_cells = nullptr) const {
    const tdt_ray_hit h = raytracer.pick({{{x, y}}}, 0)[0];
    const float floats[7] = {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_, 1.0f / (float)cell_count_};   // :44-50
    const int32_t ints[3] = {max_depth_, max_traversal_iter_, cell_count_};
    int32_t s[4];
    if (tdt_pick_face(&h, floats, ints, s) != 0) return false;
    if (seed) for (int a = 0; a < 4; a++) seed[a] = s[a];
    const uint32_t n = extrude(raytracer.context(), op, opt, std::vector<int32_t>(s, s + 4), mask);
    if (n_cells) *n_cells = n;
    return true;
  }
  // NEW: connected components of the bound tree (tdt_octree_components): the table, numbered in the Morton order of each
  // component's first voxel; labels (may be null) receive the component of every voxel of extract's list.  A count query costs
  // a whole labelling, so this labels once: labels sized by a walk (tdt_octree_extract's count), the table by `capacity`; only a
  // tree of more components is labelled again, into a table of the size the first call reported.
  std::vector<tdt_component> components(const Context &ctx, int connectivity, int match, std::vector<uint32_t> *labels = nullptr,
                                        size_t capacity = 4096) const {
    size_t nv = 0, nc = 0;
    if (labels) {
      ctx.check(tdt_octree_extract(ctx.raw(), nullptr, 0, &nv));
      labels->assign(nv, 0u);
    }
    std::vector<tdt_component> table(capacity ? capacity : 1);
    auto run = [&]() {
      return tdt_octree_components(ctx.raw(), connectivity, match, labels ? labels->data() : nullptr, labels ? labels->size() : 0, &nv,
                                   table.data(), table.size(), &nc);
    };
    int rc = run();
    if (rc == TDT_ERR_INVALID_VALUE && (nc > table.size() || (labels && nv > labels->size()))) {
      table.resize(nc);
      if (labels) labels->assign(nv, 0u);
      rc = run();
    }
    ctx.check(rc);
    table.resize(nc);
    return table;
  }
  // NEW: op (TDT_REGION_PAINT / TDT_REGION_CLEAR) over the components `sel` selects among those holding one of the seed voxels
  // (x, y, z triples; none: any) and touching `regions` (none: any); the bound tree rebuilt in place (tdt_octree_edit_connected)
  uint32_t edit_connected(const Context &ctx, int op, const tdt_select &sel, const std::vector<int32_t> &seeds_xyz,
                          const std::vector<tdt_region> &regions, int32_t material) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_connected(ctx.raw(), op, &sel, seeds_xyz.empty() ? nullptr : seeds_xyz.data(), seeds_xyz.size() / 3,
                                        regions.empty() ? nullptr : regions.data(), regions.size(), material, &n));
    return n;
  }
  // NEW: through-selection (tdt_octree_extract_screen): every voxel of the bound tree whose centre (TDT_SCREEN_WINDOW: all eight
  // corners) projects, in `view`, into sel's rectangle, the polygon (x, y pairs; TDT_SCREEN_POLYGON) or the mask image
  // (TDT_SCREEN_MASK), hidden or not, as {x, y, z, material + 1} in Morton order: the brush of edit_voxels
  std::vector<int32_t> extract_screen(const Context &ctx, const tdt_view &view, const tdt_screen_select &sel,
                                      const std::vector<int32_t> &polygon_xy = {}, const Texture *mask = nullptr) const {
    size_t n = 0;
    const int32_t *p = polygon_xy.empty() ? nullptr : polygon_xy.data();
    tdt_image *m = mask ? mask->id() : nullptr;
    ctx.check(tdt_octree_extract_screen(ctx.raw(), &view, &sel, p, polygon_xy.size() / 2, m, nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_screen(ctx.raw(), &view, &sel, p, polygon_xy.size() / 2, m, v.data(), n, &n));
    return v;
  }
  // NEW: op (TDT_REGION_PAINT with `material` / TDT_REGION_CLEAR) over that selection, the list never leaving the device
  // (tdt_octree_edit_screen); the bound tree rebuilt in place; returns the number of cells
  uint32_t edit_screen(const Context &ctx, int op, const tdt_view &view, const tdt_screen_select &sel, const std::vector<int32_t> &polygon_xy,
                       const Texture *mask, int32_t material) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_screen(ctx.raw(), op, &view, &sel, polygon_xy.empty() ? nullptr : polygon_xy.data(), polygon_xy.size() / 2,
                                     mask ? mask->id() : nullptr, material, &n));
    return n;
  }
  // NEW: a flood click, the paint bucket / delete-object tool: pick pixel (x, y) of the raytracer's camera (sample 0) and on a
  // hit apply `op` to the components `sel` selects that hold the grid voxel behind the face (tdt_pick_grid_voxel, place 0).
  // Returns whether an edit ran; *hit receives the pick, *n_cells the size.
  bool flood(const ComputeShader &raytracer, int x, int y, int op, const tdt_select &sel, int32_t material, tdt_ray_hit *hit = nullptr,
             uint32_t *n_cells = nullptr) const {
    const tdt_ray_hit h = raytracer.pick({{{x, y}}}, 0)[0];
    if (hit) *hit = h;
    const float floats[7] = {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_, 1.0f / (float)cell_count_};   // :44-50
    const int32_t ints[3] = {max_depth_, max_traversal_iter_, cell_count_};
    int32_t c[3];
    if (tdt_pick_grid_voxel(&h, floats, ints, 0, c) != 0) return false;                      // miss / stale record / outside
    const uint32_t n = edit_connected(raytracer.context(), op, sel, {c[0], c[1], c[2]}, {}, material);
    if (n_cells) *n_cells = n;
    return true;
  }
  // NEW: voxel morphology (tdt_octree_morph): m.op (TDT_MORPH_*) of m.radius steps with the 6- / 26-neighbourhood, inside the
  // union of `mask` (none: everywhere); the bound tree rebuilt in place; returns the number of cells
  uint32_t morph(const Context &ctx, const tdt_morph &m, const std::vector<tdt_region> &mask = {}) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_morph(ctx.raw(), &m, mask.empty() ? nullptr : mask.data(), mask.size(), &n));
    return n;
  }
  // NEW: what morph would leave, as voxels {x, y, z, material + 1} in Morton order, the tree untouched
  // (tdt_octree_extract_morph); TDT_MORPH_SHELL with radius 1: the surface voxels
  std::vector<int32_t> extract_morph(const Context &ctx, const tdt_morph &m, const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_extract_morph(ctx.raw(), &m, r, mask.size(), nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_morph(ctx.raw(), &m, r, mask.size(), v.data(), n, &n));
    return v;
  }
  // NEW: round morphology (tdt_octree_morph_round): r.op (TDT_MORPH_*) with the Euclidean ball of squared radius r.radius2,
  // inside the union of `mask` (none: everywhere); the bound tree rebuilt in place; returns the number of cells
  uint32_t morph_round(const Context &ctx, const tdt_round &r, const std::vector<tdt_region> &mask = {}) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_morph_round(ctx.raw(), &r, mask.empty() ? nullptr : mask.data(), mask.size(), &n));
    return n;
  }
  // NEW: the signed squared Euclidean distance over the inclusive box lo..hi (tdt_octree_distance_field), x fastest; magnitudes
  // above max_d2 come back as max_d2 + 1; `nearest` (optional) receives three coordinates per voxel
  std::vector<int32_t> distance_field(const Context &ctx, const int32_t lo[3], const int32_t hi[3], int32_t max_d2, int32_t border = 0,
                                      std::vector<int32_t> *nearest = nullptr) const {
    size_t n = 0;
    ctx.check(tdt_octree_distance_field(ctx.raw(), lo, hi, max_d2, border, nullptr, nullptr, 0, &n));
    std::vector<int32_t> f(n);
    if (nearest) nearest->assign(3 * n, -1);
    if (n) ctx.check(tdt_octree_distance_field(ctx.raw(), lo, hi, max_d2, border, f.data(), nearest ? nearest->data() : nullptr, n, &n));
    return f;
  }
  // NEW: the smooth brush (tdt_octree_smooth): s.iterations steps of the ball-density threshold filter with the ball of squared
  // radius s.radius2, inside the union of `mask` (none: everywhere); the bound tree rebuilt in place; returns the number of cells
  uint32_t smooth(const Context &ctx, const tdt_smooth &s, const std::vector<tdt_region> &mask = {}) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_smooth(ctx.raw(), &s, mask.empty() ? nullptr : mask.data(), mask.size(), &n));
    return n;
  }
  // NEW: what smooth would leave, as voxels {x, y, z, material + 1} in Morton order, the tree untouched (tdt_octree_extract_smooth)
  std::vector<int32_t> extract_smooth(const Context &ctx, const tdt_smooth &s, const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_extract_smooth(ctx.raw(), &s, r, mask.size(), nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_smooth(ctx.raw(), &s, r, mask.size(), v.data(), n, &n));
    return v;
  }
  // NEW: how many voxels of the tree the ball of squared radius radius2 around each voxel of the inclusive box lo..hi holds
  // (tdt_octree_density_field), x fastest; `support` (optional) receives the number of ball points inside the grid per voxel
  std::vector<int32_t> density_field(const Context &ctx, const int32_t lo[3], const int32_t hi[3], int32_t radius2,
                                     std::vector<int32_t> *support = nullptr) const {
    size_t n = 0;
    ctx.check(tdt_octree_density_field(ctx.raw(), lo, hi, radius2, nullptr, nullptr, 0, &n));
    std::vector<int32_t> d(n);
    if (support) support->assign(n, 0);
    if (n) ctx.check(tdt_octree_density_field(ctx.raw(), lo, hi, radius2, d.data(), support ? support->data() : nullptr, n, &n));
    return d;
  }
  // NEW: move, turn, mirror, rotate or scale a selection (tdt_octree_transform): x is the destination -> source map (the
  // tdt_xform_* builders of tdt_host.h make one from a forward transform); the voxels of the tree inside the union of `mask`
  // (none: all of it) are resampled through it and applied with op (TDT_REGION_*) as a voxel list that never leaves the device.
  // The source voxels stay where they are.  Returns the number of cells.
  uint32_t transform(const Context &ctx, const tdt_xform &x, int op = TDT_REGION_SET, const std::vector<tdt_region> &mask = {}) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_transform(ctx.raw(), &x, op, mask.empty() ? nullptr : mask.data(), mask.size(), &n));
    return n;
  }
  // NEW: the transformed selection itself, voxels {x, y, z, material + 1} in Morton order, the tree untouched
  // (tdt_octree_extract_transform): the preview, and with a CLEAR of the source in between, the move
  std::vector<int32_t> extract_transform(const Context &ctx, const tdt_xform &x, const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_extract_transform(ctx.raw(), &x, r, mask.size(), nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_transform(ctx.raw(), &x, r, mask.size(), v.data(), n, &n));
    return v;
  }
  // NEW: geodesic distance (tdt_octree_edit_geodesic): apply `op` (TDT_REGION_*) to the reach set of `g` — every voxel of g.medium
  // whose cheapest path of face / edge / corner steps (costs g.w) from one of `seeds_xyz` (x, y, z triples), staying inside the
  // medium and inside the union of `mask` (none: anywhere), costs at most g.max_cost — in material g.material (-1: the voxel's
  // own, the SOLID medium only).  The soft selection and the pouring tool.  Returns the number of cells.
  uint32_t reach(const Context &ctx, int op, const tdt_geodesic &g, const std::vector<int32_t> &seeds_xyz, const std::vector<tdt_region> &mask = {}) const {
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_geodesic(ctx.raw(), op, &g, seeds_xyz.empty() ? nullptr : seeds_xyz.data(), seeds_xyz.size() / 3,
                                       mask.empty() ? nullptr : mask.data(), mask.size(), &n));
    return n;
  }
  // NEW: a reach click: pick pixel (x, y) of the raytracer's camera (sample 0) and on a hit run reach() from the grid voxel behind
  // the face (the SOLID medium) or in front of it (the EMPTY medium) (tdt_pick_grid_voxel).  Returns whether an edit ran; *hit
  // receives the pick, *n_cells the size.
  bool reach(const ComputeShader &raytracer, int x, int y, int op, const tdt_geodesic &g, const std::vector<tdt_region> &mask = {},
             tdt_ray_hit *hit = nullptr, uint32_t *n_cells = nullptr) const {
    const tdt_ray_hit h = raytracer.pick({{{x, y}}}, 0)[0];
    if (hit) *hit = h;
    const float floats[7] = {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_, 1.0f / (float)cell_count_};   // :44-50
    const int32_t ints[3] = {max_depth_, max_traversal_iter_, cell_count_};
    int32_t c[3];
    if (tdt_pick_grid_voxel(&h, floats, ints, g.medium == TDT_MEDIUM_EMPTY ? 1 : 0, c) != 0) return false;   // miss / stale record / outside
    const uint32_t n = reach(raytracer.context(), op, g, {c[0], c[1], c[2]}, mask);
    if (n_cells) *n_cells = n;
    return true;
  }
  // NEW: the reach set itself, voxels {x, y, z, material + 1} in Morton order, the tree untouched (tdt_octree_extract_geodesic)
  std::vector<int32_t> extract_reach(const Context &ctx, const tdt_geodesic &g, const std::vector<int32_t> &seeds_xyz,
                                     const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const int32_t *s = seeds_xyz.empty() ? nullptr : seeds_xyz.data();
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_extract_geodesic(ctx.raw(), &g, s, seeds_xyz.size() / 3, r, mask.size(), nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_geodesic(ctx.raw(), &g, s, seeds_xyz.size() / 3, r, mask.size(), v.data(), n, &n));
    return v;
  }
  // NEW: the geodesic distance over the inclusive box lo..hi (tdt_octree_geodesic_field), x fastest; -1 where a voxel is not in
  // the medium, unreachable or beyond g.max_cost
  std::vector<int32_t> reach_field(const Context &ctx, const tdt_geodesic &g, const std::vector<int32_t> &seeds_xyz, const int32_t lo[3],
                                   const int32_t hi[3], const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const int32_t *s = seeds_xyz.empty() ? nullptr : seeds_xyz.data();
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_geodesic_field(ctx.raw(), &g, s, seeds_xyz.size() / 3, r, mask.size(), lo, hi, nullptr, 0, &n));
    std::vector<int32_t> f(n);
    if (n) ctx.check(tdt_octree_geodesic_field(ctx.raw(), &g, s, seeds_xyz.size() / 3, r, mask.size(), lo, hi, f.data(), n, &n));
    return f;
  }
  // NEW: the canonical shortest path from `goal` back to the seed it reaches, x, y, z triples with the goal first
  // (tdt_octree_geodesic_path); *cost receives its cost.  A goal outside the reach set: no points, cost -1.
  std::vector<int32_t> path(const Context &ctx, const tdt_geodesic &g, const std::vector<int32_t> &seeds_xyz, const int32_t goal[3],
                            const std::vector<tdt_region> &mask = {}, int32_t *cost = nullptr) const {
    size_t n = 0;
    int32_t c = -1;
    const int32_t *s = seeds_xyz.empty() ? nullptr : seeds_xyz.data();
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_geodesic_path(ctx.raw(), &g, s, seeds_xyz.size() / 3, r, mask.size(), goal, nullptr, 0, &n, &c));
    std::vector<int32_t> p(3 * n);
    if (n) ctx.check(tdt_octree_geodesic_path(ctx.raw(), &g, s, seeds_xyz.size() / 3, r, mask.size(), goal, p.data(), n, &n, &c));
    if (cost) *cost = c;
    return p;
  }
  // NEW: stamp a triangle mesh (tdt_octree_edit_triangles): op (TDT_REGION_*) over the voxels the closed triangles touch —
  // vertices {x, y, z} fixed point, 64 units per voxel (tdt_mesh_quantize), triangles 3 vertex indices each, material 0..253 for
  // every triangle or, with `materials`, material + 1 per triangle (the highest covering triangle wins).  A surface
  // voxelisation: interiors stay as they are.  Returns the number of cells; *n_voxels receives the size of the mesh's voxel
  // list at this tree's depth (a second rasterisation, tdt_voxelize_triangles counting only).
  uint32_t stamp_mesh(const Context &ctx, int op, const std::vector<int32_t> &vertices_xyz, const std::vector<uint32_t> &triangles,
                      int32_t material, const std::vector<int32_t> &materials = {}, size_t *n_voxels = nullptr) const {
    tdt_mesh m{};
    m.vertices = vertices_xyz.empty() ? nullptr : vertices_xyz.data();
    m.triangles = triangles.empty() ? nullptr : triangles.data();
    m.materials = materials.empty() ? nullptr : materials.data();
    m.n_vertices = (uint32_t)(vertices_xyz.size() / 3); m.n_triangles = (uint32_t)(triangles.size() / 3);
    m.material = material;
    if (n_voxels) ctx.check(tdt_voxelize_triangles(ctx.raw(), &m, max_depth_, nullptr, 0, n_voxels));
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_triangles(ctx.raw(), op, &m, &n));
    return n;
  }
  // NEW: stamp_mesh's solid form (tdt_octree_edit_triangles_solid): the mesh's surface voxels AND the empty voxels that surface
  // seals off from the grid's faces (fill.connectivity 6 / 26 between empty voxels; fill.material -1: each takes the material of
  // the surface voxel at its -x side, 0..253: that material), decided by the mesh alone, whatever the tree holds.  *n_voxels
  // receives the solid's size, at the price of a second rasterisation and flood (tdt_voxelize_triangles_solid counting only).
  // (A name of its own: as an overload, a `{}` argument would fit the tdt_fill and the materials list alike.)
  uint32_t stamp_mesh_solid(const Context &ctx, int op, const std::vector<int32_t> &vertices_xyz, const std::vector<uint32_t> &triangles,
                            int32_t material, const tdt_fill &fill, const std::vector<int32_t> &materials = {}, size_t *n_voxels = nullptr) const {
    tdt_mesh m{};
    m.vertices = vertices_xyz.empty() ? nullptr : vertices_xyz.data();
    m.triangles = triangles.empty() ? nullptr : triangles.data();
    m.materials = materials.empty() ? nullptr : materials.data();
    m.n_vertices = (uint32_t)(vertices_xyz.size() / 3); m.n_triangles = (uint32_t)(triangles.size() / 3);
    m.material = material;
    if (n_voxels) ctx.check(tdt_voxelize_triangles_solid(ctx.raw(), &m, max_depth_, &fill, nullptr, 0, n_voxels));
    uint32_t n = 0;
    ctx.check(tdt_octree_edit_triangles_solid(ctx.raw(), op, &m, &fill, &n));
    return n;
  }
  // NEW: fill the tree's cavities (tdt_octree_fill_enclosed): every empty voxel that no path of empty neighbours
  // (fill.connectivity 6 / 26) connects to a face of the grid becomes solid (fill.material, or -1: the material of the wall at its
  // -x side), inside the union of `mask` (none: everywhere); the bound tree rebuilt in place; returns the number of cells.
  // *n_voxels receives the number of voxels filled (a second flood, tdt_octree_extract_enclosed counting only).
  uint32_t fill_enclosed(const Context &ctx, const tdt_fill &fill, const std::vector<tdt_region> &mask = {}, size_t *n_voxels = nullptr) const {
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    if (n_voxels) ctx.check(tdt_octree_extract_enclosed(ctx.raw(), &fill, r, mask.size(), nullptr, 0, n_voxels));
    uint32_t n = 0;
    ctx.check(tdt_octree_fill_enclosed(ctx.raw(), &fill, r, mask.size(), &n));
    return n;
  }
  // NEW: what fill_enclosed would add, as voxels {x, y, z, material + 1} in Morton order, the tree untouched
  // (tdt_octree_extract_enclosed): the preview, and the undo record (edit_voxels(TDT_REGION_CLEAR, it) undoes the fill)
  std::vector<int32_t> extract_enclosed(const Context &ctx, const tdt_fill &fill, const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_extract_enclosed(ctx.raw(), &fill, r, mask.size(), nullptr, 0, &n));
    std::vector<int32_t> v(4 * n);
    if (n) ctx.check(tdt_octree_extract_enclosed(ctx.raw(), &fill, r, mask.size(), v.data(), n, &n));
    return v;
  }
  // NEW: the tree's exposed voxel faces as quads (tdt_octree_extract_surface), ordered by face, w, u0, v0, the tree untouched:
  // opt.merge 1 joins them into runs and stacks of identical runs (0: one quad per face), opt.by_material 1 keeps materials apart
  // (0: the collision-mesh form), only the faces of voxels inside the union of `mask` (none: everywhere).  tdt_quads_to_mesh
  // (tdt_host.h) turns them into an indexed triangle mesh, tdt_ply_mesh_write into a PLY file.
  std::vector<tdt_quad> extract_surface(const Context &ctx, const tdt_surface &opt, const std::vector<tdt_region> &mask = {}) const {
    size_t n = 0;
    const tdt_region *r = mask.empty() ? nullptr : mask.data();
    ctx.check(tdt_octree_extract_surface(ctx.raw(), &opt, r, mask.size(), nullptr, 0, &n));
    std::vector<tdt_quad> q(n);
    if (n) ctx.check(tdt_octree_extract_surface(ctx.raw(), &opt, r, mask.size(), q.data(), n, &n));
    return q;
  }
  // The click handler (main.rs:551-568) aimed at what is under the cursor: pick pixel (x, y) of the raytracer's camera (sample 0),
  // and on a hit place (ClickEvent::Left) a voxel of `material` in front of the face, or remove (ClickEvent::Right) the one
  // behind it, through the same update_vbo(delta, 5, ..) call.  Returns whether an edit was dispatched; *hit receives the pick.
  bool click(const ComputeShader &raytracer, int x, int y, bool place, float material, const ComputeShader &update_compute,
             tdt_ray_hit *hit = nullptr) const {
    const tdt_ray_hit h = raytracer.pick({{{x, y}}}, 0)[0];
    if (hit) *hit = h;
    const float floats[7] = {min_point_[0], min_point_[1], min_point_[2], 0.0f, scale_, 1.0f / scale_, 1.0f / (float)cell_count_};   // :44-50
    const int32_t ints[3] = {max_depth_, max_traversal_iter_, cell_count_};
    std::vector<float> delta(8, 0.0f);
    if (tdt_pick_edit_delta(&h, floats, ints, place ? 1 : 0, material, delta.data()) != 0) return false;    // miss / stale record / outside
    update_vbo(delta, 5, update_compute);
    return true;
  }
 private:
  // the tdt_stroke of stroke() / extract_stroke(); an explicit empty segment list still points somewhere (NULL means the polyline)
  static tdt_stroke stroke_of(const std::vector<int32_t> &points_xyz, int shape, int radius, int32_t material, const std::vector<uint32_t> &segments,
                              bool polyline, const std::vector<int32_t> &materials, const uint32_t *none) {
    tdt_stroke s{};
    s.points = points_xyz.empty() ? nullptr : points_xyz.data();
    s.segments = !segments.empty() ? segments.data() : polyline ? nullptr : none;
    s.materials = materials.empty() ? nullptr : materials.data();
    s.n_points = (uint32_t)(points_xyz.size() / 3); s.n_segments = (uint32_t)(segments.size() / 2);
    s.shape = shape; s.radius = radius; s.material = material;
    return s;
  }
  Vector3f min_point_{};
  float scale_ = 1, block_distance_ = 0;
  int max_depth_ = 0, cell_count_ = 0, active_cell_count_ = 0, max_traversal_iter_ = 0;
  VertexBufferObject floats_, ints_, counter_, delta_;
};

// renderer/camera.rs:8-16
using CameraSettings = tdt_camera_settings;
inline CameraSettings camera_settings_from_ron(const std::string &text) {                         // main.rs:171, 493
  CameraSettings s;
  if (tdt_camera_settings_from_ron(text.data(), text.size(), &s)) throw InitializeErr{InitializeErr::GL, 0x0501, "", "", tdt_host_last_error()};
  return s;
}

// utility/mod.rs:6-26
enum class Direction { Front, Back, Rigth, Left, Up, Down };
inline Vector3f into_vector3(Direction d) {
  switch (d) {
    case Direction::Front: return {0.0f, 0.0f, -1.0f};
    case Direction::Back: return {0.0f, 0.0f, 1.0f};
    case Direction::Rigth: return {1.0f, 0.0f, 0.0f};
    case Direction::Left: return {-1.0f, 0.0f, 0.0f};
    case Direction::Up: return {0.0f, 1.0f, 0.0f};
    default: return {0.0f, -1.0f, 0.0f};
  }
}

// renderer/camera.rs:20-102: the controller state lives in libtdthost's tdt_camera (cgmath restated there)
class Camera {
 public:
  tdt_camera state{};
  Texture render_texture;
  const float *horizontal() const { return state.horizontal; }
  const float *vertical() const { return state.vertical; }
  const float *lower_left_corner() const { return state.lower_left_corner; }
  const float *origin() const { return state.origin; }
  int32_t image_width() const { return state.image_width; }
  int32_t image_height() const { return state.image_height; }
  const CameraSettings &settings() const { return state.settings; }
  void translate(const Program &program, const Vector3f &by, double deltatime) {                   // :40-43
    tdt_camera_translate(&state, by.data(), deltatime); propagate_changes(program);
  }
  void turn_pitch(const Program &program, float angle) { tdt_camera_turn_pitch(&state, angle); propagate_changes(program); }   // :46-53
  void turn_yaw(const Program &program, float angle) { tdt_camera_turn_yaw(&state, angle); propagate_changes(program); }       // :56-62
  void set_speed_to_normal() { tdt_camera_set_speed_to_normal(&state); }                             // :84-86
  void set_speed_to_sprint() { tdt_camera_set_speed_to_sprint(&state); }                             // :88-90
  Vector3f look_at_world_point(float distance) const {                                              // :92-94
    Vector3f p{}; tdt_camera_look_at_world_point(&state, distance, p.data()); return p;
  }
  void apply_settings(const Program &program, const CameraSettings &s) {                            // :96-101
    tdt_camera_apply_settings(&state, &s);
    program.set_i32("camera.samples_per_pixel", state.settings.samples_per_pixel);
    program.set_i32("camera.max_bounce", state.settings.max_bounce);
  }
 private:
  void propagate_changes(const Program &program) const {                                            // the uploads of :78-81
    program.set_vector3_f32("camera.horizontal", {state.horizontal[0], state.horizontal[1], state.horizontal[2]});
    program.set_vector3_f32("camera.vertical", {state.vertical[0], state.vertical[1], state.vertical[2]});
    program.set_vector3_f32("camera.lower_left_corner", {state.lower_left_corner[0], state.lower_left_corner[1], state.lower_left_corner[2]});
    program.set_vector3_f32("camera.origin", {state.origin[0], state.origin[1], state.origin[2]});
  }
  friend class CameraBuilder;
};

// renderer/camera.rs:104-237
class CameraBuilder {
 public:
  static CameraBuilder new_(float vertical_fov, int32_t image_width) {                           // :119-133
    CameraBuilder b;
    std::memset(&b.b_, 0, sizeof b.b_);
    b.b_.vertical_fov = vertical_fov; b.b_.image_width = image_width;
    return b;
  }
  CameraBuilder &with_aspect_ratio(float a) { b_.has_aspect_ratio = 1; b_.aspect_ratio = a; return *this; }
  CameraBuilder &with_viewport_height(float h) { b_.has_viewport_height = 1; b_.viewport_height = h; return *this; }
  CameraBuilder &with_origin(const Vector3f &o) { b_.has_origin = 1; b_.origin[0] = o[0]; b_.origin[1] = o[1]; b_.origin[2] = o[2]; return *this; }
  CameraBuilder &with_sample_per_pixel(int32_t n) { b_.has_samples_per_pixel = 1; b_.samples_per_pixel = n; return *this; }
  CameraBuilder &with_max_bounce(int32_t n) { b_.has_max_bounce = 1; b_.max_bounce = n; return *this; }
  CameraBuilder &with_turn_rate(float v) { b_.has_turn_rate = 1; b_.turn_rate = v; return *this; }
  CameraBuilder &with_normal_speed(float v) { b_.has_normal_speed = 1; b_.normal_speed = v; return *this; }
  CameraBuilder &with_sprint_speed(float v) { b_.has_sprint_speed = 1; b_.sprint_speed = v; return *this; }
  Camera build(Context &ctx, const Program &program) const {                                     // :135-196
    Camera c;
    if (tdt_camera_init(&b_, &c.state)) throw InitializeErr{InitializeErr::GL, 0x0501, "", "", tdt_host_last_error()};
    c.render_texture = Texture::new_2d(ctx, c.state.image_width, c.state.image_height);          // :158-165
    // initial_uniforms, camera.rs:241-253
    program.set_i32("camera.image_width", c.state.image_width);
    program.set_i32("camera.image_height", c.state.image_height);
    c.propagate_changes(program);
    program.set_i32("camera.samples_per_pixel", c.state.settings.samples_per_pixel);
    program.set_i32("camera.max_bounce", c.state.settings.max_bounce);
    return c;
  }
 private:
  tdt_camera_builder b_;
};

// Presentation: the frame the reference's quad pass would show (main.rs:582-600, quad.frag:10), as a PNG file
inline void present_png(Texture &texture, const std::string &path, bool with_alpha = false) {
  std::vector<uint8_t> frame(static_cast<size_t>(texture.width()) * texture.height() * 4);
  texture.read_rgba8(true, frame.data());
  if (tdt_png_write(path.c_str(), frame.data(), texture.width(), texture.height(), with_alpha ? 1 : 0))
    throw InitializeErr{InitializeErr::GL, 0x0501, "", "", tdt_host_last_error()};
}

}  // namespace renderer
