/*
 * tdt_host.h — C ABI of libtdthost.so: the host-side inputs of the trace, restated from the
 * reference's Rust host code (which cannot be compiled here: no Rust toolchain).
 *
 *   - camera uniforms  : CameraBuilder::build / initial_uniforms   (src/renderer/camera.rs:135-196, 241-253)
 *   - octree payloads  : Octree::init_global_buffers                (src/renderer/octree.rs:40-100)
 *   - the demo scene   : the literal of src/main.rs:235-463 (as data)
 *   - synthetic scenes : deterministic generators for BASELINE.json's configs (the reference
 *                        has no octree builder and no other scene)
 *
 * Pure host code (no HIP).  A scene is nothing but the seven SSBO payloads, byte-for-byte in
 * the layout raytracer.comp reads, so the same blobs feed the reference shader, the oracle
 * and libtdtrt.so.
 */
#ifndef TDT_HOST_H
#define TDT_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- camera ---------------- */
/* CameraBuilder (camera.rs:104-117); a has_* of 0 means "None" and build() applies the
 * reference's default. */
typedef struct {
  float vertical_fov;            /* CameraBuilder::new(vertical_fov, image_width) camera.rs:120 */
  int32_t image_width;
  int32_t has_aspect_ratio;    float aspect_ratio;      /* default 16/9  camera.rs:136 */
  int32_t has_viewport_height; float viewport_height;   /* default 2.0   camera.rs:140 */
  int32_t has_origin;          float origin[3];         /* default 0     camera.rs:143 */
  int32_t has_samples_per_pixel; int32_t samples_per_pixel; /* default 10 camera.rs:156 */
  int32_t has_max_bounce;      int32_t max_bounce;      /* default 3     camera.rs:157 */
  /* controller settings (only tdt_camera_init reads them; tdt_camera_build ignores them like build() does for the uniforms) */
  int32_t has_turn_rate;       float turn_rate;         /* default 0.025 camera.rs:167 */
  int32_t has_normal_speed;    float normal_speed;      /* default 1.0   camera.rs:168 */
  int32_t has_sprint_speed;    float sprint_speed;      /* default 2 * normal_speed camera.rs:169 */
} tdt_camera_builder;

/* what initial_uniforms() sends (camera.rs:241-253) = `uniform Camera camera` raytracer.comp:133-146 */
typedef struct {
  int32_t image_width, image_height;
  float horizontal[3], vertical[3], lower_left_corner[3], origin[3];
  int32_t samples_per_pixel, max_bounce;
} tdt_camera_uniforms;

int tdt_camera_build(const tdt_camera_builder *b, tdt_camera_uniforms *out);
/* the pose main.rs:165-168 builds: fov 90, origin (0,-0.1,-0.3), viewport_height 2.0,
 * aspect = width/height (f32 division) */
int tdt_camera_reference_pose(int width, int height, int spp, int max_bounce, tdt_camera_uniforms *out);

/* ---- next row SURVEY §8f-3: the camera controller and its settings (camera.rs:8-16, 20-102) ----
 * The reference's vector / quaternion arithmetic is the cgmath crate's (Cargo.lock: cgmath 0.18.0; not vendored, no Rust
 * toolchain here): csrc/host_view.cpp restates its published formulas in f32.  PARITY UNPINNED (no reference fixture
 * covers these values). */
typedef struct {                 /* CameraSettings camera.rs:9-16 = assets/settings/camera.ron */
  int32_t samples_per_pixel, max_bounce;
  float turn_rate, normal_speed, sprint_speed;
} tdt_camera_settings;

typedef struct {                 /* Camera camera.rs:20-37, minus the GL texture */
  float horizontal[3], vertical[3];
  float viewport_width, viewport_height;
  float lower_left_corner[3], origin[3];
  float pitch[4], yaw[4];        /* quaternions in Quaternion::new(w, xi, yj, zk) order */
  int32_t image_width, image_height;
  tdt_camera_settings settings;
  float movement_speed;
} tdt_camera;

int tdt_camera_init(const tdt_camera_builder *b, tdt_camera *cam);                     /* CameraBuilder::build camera.rs:135-196 */
int tdt_camera_translate(tdt_camera *cam, const float by[3], double deltatime);        /* camera.rs:40-43; `by` e.g. Direction::into_vector3 utility/mod.rs:15-26 */
int tdt_camera_turn_pitch(tdt_camera *cam, float angle);                               /* camera.rs:46-53 */
int tdt_camera_turn_yaw(tdt_camera *cam, float angle);                                 /* camera.rs:56-62 */
void tdt_camera_set_speed_to_normal(tdt_camera *cam);                                  /* camera.rs:84-86 */
void tdt_camera_set_speed_to_sprint(tdt_camera *cam);                                  /* camera.rs:88-90 */
int tdt_camera_look_at_world_point(const tdt_camera *cam, float distance, float out[3]);   /* camera.rs:92-94 (main.rs:555) */
int tdt_camera_apply_settings(tdt_camera *cam, const tdt_camera_settings *s);          /* camera.rs:96-101 */
/* the uniforms propagate_changes / apply_settings / initial_uniforms have sent so far (camera.rs:78-81, 99-100, 241-253) */
int tdt_camera_get_uniforms(const tdt_camera *cam, tdt_camera_uniforms *out);
/* `ron::de::from_bytes::<CameraSettings>` (main.rs:171, 493) for the RON subset such a file uses: optional struct name,
 * `field: number` pairs in any order, comments, optional trailing comma; a missing field or a float where an i32 is
 * expected is an error (returns 1, message in tdt_host_last_error) */
int tdt_camera_settings_from_ron(const char *text, size_t n, tdt_camera_settings *out);

/* ---- next row SURVEY §8f-4: presentation ----
 * The reference shows the render texture with a full-window quad (assets/shaders/quad.vert, quad.frag:10; main.rs:113-153,
 * 582-600) and never writes a file.  tdt_present_rgba8 is what that pass leaves in an RGBA8 back buffer of the texture's
 * size (pinned on llvmpipe: tests/golden/present_*.npz): per channel clamp to [0,1] (NaN -> 0), x 255, round half to even.
 * Source rows are bottom-up (row 0 = bottom scan-line); top_down = 1 writes the top scan-line first (file order). */
int tdt_present_rgba8(const float *rgba, int w, int h, int top_down, uint8_t *dst);
/* 8-bit PNG (colour type 2, or 6 with_alpha) of a TOP-DOWN RGBA8 frame; *out is malloc'ed: release with tdt_host_free */
int tdt_png_encode(const uint8_t *rgba8, int w, int h, int with_alpha, uint8_t **out, size_t *len);
int tdt_png_write(const char *path, const uint8_t *rgba8, int w, int h, int with_alpha);
void tdt_host_free(void *p);

/* ---------------------------------------------------------------- scenes ---------------- */
typedef struct tdt_scene tdt_scene;

enum { TDT_SCENE_HASH_GRID = 0, TDT_SCENE_TERRAIN = 1, TDT_SCENE_SHELLS = 2 };

typedef struct {
  int32_t kind;          /* TDT_SCENE_*                                                     */
  int32_t max_depth;     /* log2 of the voxel grid edge (OctreeInts.max_depth)              */
  int32_t cell_count;    /* OctreeInts.cell_count: the divisor the shader uses; power of two */
  int32_t max_iter;      /* OctreeInts.max_iter                                             */
  uint64_t seed;
} tdt_scene_params;

/* main.rs:235-463: 19 cells (+ zero padding to 100144 u32), 13 materials, 7 albedos, 4 fuzz,
 * 1 ior; Octree::new(min (-.5,-.5,-1), scale 1, max_depth 10, cell_count 100000, max_iter 100) */
int tdt_scene_demo(tdt_scene **out);
int tdt_scene_generate(const tdt_scene_params *p, tdt_scene **out);
/* BASELINE.json configs 1..5 (config 4 uses the config-3 scene); see DESIGN.md */
int tdt_scene_config(int config, tdt_scene **out);
/* a scene from caller-provided payloads (copied) */
int tdt_scene_from_blobs(const void *const blobs[8], const size_t bytes[8], tdt_scene **out);
void tdt_scene_destroy(tdt_scene *s);
/* payload of SSBO binding `slot` (0,1,2,3,4,6,7); NULL/0 for other slots */
const void *tdt_scene_blob(const tdt_scene *s, int slot, size_t *bytes);
/* counts: [0]=cells in use, [1]=parent nodes, [2]=leaf nodes, [3]=empty nodes,
 * [4]=materials, [5]=occupied finest-level voxels (0 for the demo scene) */
int tdt_scene_counts(const tdt_scene *s, int64_t out[6]);
const char *tdt_host_last_error(void);

/* ---------------------------------------------------------------- scene ingest --- */
/* ply_point_loader::from_resources (src/utility/ply_point_loader.rs:102-319) restated over a byte
 * buffer: the MagicaVoxel ASCII point export ("float" x y z that are really integers, uchar r g b).
 * strict_crlf = 1 is the reference grammar to the byte ("ply\r\n", "format ascii 1.0\r\n", every
 * line CRLF: :121,:130,:158,:175,:207,:312-314); 0 also accepts LF-only files (as checked out on
 * Linux).  Quirks kept: a header word only has to match a PREFIX of its keyword (:138-152); the
 * albedo key is recomputed and inserted after EVERY property of a vertex (:300-307), so the palette
 * also holds the partial colours (0,0,0), (r,0,0), (r,g,0); the Cantor pairing runs in f64 and
 * saturates to u32 (:228-241); the vertex count of the header is not checked against the data.
 * One deviation: an unknown header keyword is an error here (the reference loops forever, :136-153).
 * PARITY UNPINNED: the Rust loader cannot be built or run in this image; tests pin the restatement
 * against hand-derived values for the reference's own 3x3x3 model. */
typedef struct tdt_ply tdt_ply;
int tdt_ply_parse(const void *data, size_t bytes, int strict_crlf, tdt_ply **out);
void tdt_ply_destroy(tdt_ply *p);
/* header.vertex, number of voxels read, min_point (:221), palette size */
int tdt_ply_info(const tdt_ply *p, int64_t *header_vertex, int64_t *n_voxels, int32_t min_point[3], int64_t *n_albedos);
/* 4 x i32 per voxel: x, y, z, albedo_key (as u32 bits) */
const int32_t *tdt_ply_voxels(const tdt_ply *p);
/* palette sorted by key (the reference's HashMap has no order): returns the number written */
int64_t tdt_ply_albedos(const tdt_ply *p, uint32_t *keys, uint8_t *rgb, int64_t capacity);
/* The step the reference never wrote (the loader's result is unused: main.rs:218-224): voxels ->
 * breadth-first indirect cells + one Lambertian material per distinct voxel colour (rgb / 255).
 * The grid edge is the next power of two >= the model's extent; z_up = 1 maps the file's z to the
 * octree's y (MagicaVoxel is z-up); the model is centred in x, stands on the floor and is pushed to
 * the far (z = 0) side of the octree so that the reference camera (main.rs:165-168) looks at it. */
int tdt_scene_from_ply(const tdt_ply *p, int max_iter, int z_up, tdt_scene **out);

/* ---------------------------------------------------------------- triangle meshes ------------ */
/* Float vertices -> the fixed-point vertices of tdt_voxelize_triangles / tdt_octree_edit_triangles (include/tdt_rt.h: 64 units
 * per voxel, |coordinate| <= 2^18 units).  out[3 i + a] = llrint(((double)xyz[3 i + a] * scale + offset[a]) * 64.0), in double,
 * unfused, ties to even — numpy float64 with np.rint reproduces it exactly.  A result that is not finite or beyond +-2^18:
 * TDT_ERR_INVALID_VALUE (0x0501), message in tdt_host_last_error, nothing written. */
int tdt_mesh_quantize(const float *xyz, size_t n, double scale, const double offset[3], int32_t *out);
/* The uniform scale and the offset (voxels) that centre the bounding box of n > 0 vertices in the voxel box lo..hi inclusive,
 * i.e. the continuous box [lo, hi + 1]: scale = the smallest of (hi + 1 - lo)[a] / extent[a] over the axes of non-zero extent,
 * so the mesh fits and its limiting edge spans the box; a mesh of zero extent gets scale 1.  offset[a] = the box's centre -
 * the bounding box's centre * scale.  Coverage is closed: a vertex exactly on an outer face of the box also touches the voxel
 * layer beyond it.  Errors (0x0501): NULL, n == 0, an empty box, a vertex that is not finite. */
int tdt_mesh_fit(const float *xyz, size_t n, const int32_t lo[3], const int32_t hi[3], double *scale, double offset[3]);
/* A minimal ASCII PLY mesh reader, separate from tdt_ply_parse (which restates the reference's point loader).  Grammar: "ply",
 * "format ascii 1.0", LF or CRLF lines; comment / obj_info lines; "element vertex N" whose first three properties are float or
 * double x, y, z (further scalar vertex properties are read and skipped: colours are IGNORED, materials come from the
 * caller); then "element face M" with exactly one "property list uchar|uint8 int|uint|int32|uint32 vertex_indices|vertex_index";
 * "end_header"; N vertices, M faces.  A polygon of k >= 3 vertices becomes the fan (0, i, i + 1).  Anything else — another
 * format, other elements, a list of fewer than 3 indices, an index >= N, truncated or trailing data — is 0x0501 with a
 * message in tdt_host_last_error. */
typedef struct tdt_ply_mesh tdt_ply_mesh;
int tdt_ply_mesh_parse(const void *data, size_t bytes, tdt_ply_mesh **out);
void tdt_ply_mesh_destroy(tdt_ply_mesh *m);
int tdt_ply_mesh_info(const tdt_ply_mesh *m, int64_t *n_vertices, int64_t *n_faces, int64_t *n_triangles);
/* n_vertices x {x, y, z} / n_triangles x 3 indices, owned by m (NULL when empty) */
const float *tdt_ply_mesh_vertices(const tdt_ply_mesh *m);
const uint32_t *tdt_ply_mesh_triangles(const tdt_ply_mesh *m);
/* Quads -> the fixed-point indexed mesh of tdt_mesh: the way back from tdt_octree_extract_surface (include/tdt_rt.h) to polygons.
 * quads: n_quads x tdt_quad as eight int32 {face, material, origin[3], size[2], pad}.  With a = face >> 1, s = face & 1, u = (a + 1) % 3,
 * v = (a + 2) % 3 the corners are c0 = origin, c1 = c0 + size[0] e_u, c2 = c1 + size[1] e_v, c3 = c0 + size[1] e_v, in voxels; they
 * are emitted as c0, c1, c2, c3 for s = 1 and as c0, c3, c2, c1 for s = 0, so every normal points out of the solid, and the quad's
 * triangles are (0, 1, 2) and (0, 2, 3) of the emitted corners, in quad order.  Vertices are in units (64 per voxel), welded: each
 * distinct corner once, in ascending (x, y, z) order.  materials[t] = the quad's material for both of its triangles (0 with
 * by_material = 0: hand tdt_mesh a NULL materials array then).  Count-then-fill: *n_vertices and *n_triangles are always set; with
 * vertices, triangles and materials all NULL nothing else happens; otherwise vertices and triangles are required (materials may
 * be NULL) and a capacity below its count is 0x0501 with nothing written.  Also 0x0501: a face outside 0..5, a size below 1, a
 * corner outside 0..4096 voxels (TDT_MESH_COORD_MAX), more than 2^30 quads. */
int tdt_quads_to_mesh(const int32_t *quads, size_t n_quads, int32_t *vertices, size_t vertex_capacity, size_t *n_vertices,
                      uint32_t *triangles, int32_t *materials, size_t triangle_capacity, size_t *n_triangles);
/* A fixed-point mesh as ASCII PLY in the grammar tdt_ply_mesh_parse accepts: float x, y, z in VOXELS (units / 64: at most six
 * decimals, exact, and exact again as the float the reader stores), faces as triangles "3 i j k".  *bytes = the length of the text
 * (no terminating NUL is written); buffer == NULL only counts; capacity < *bytes: 0x0501 with *bytes set and nothing written.
 * Also 0x0501: NULL arrays with a count above 0, an index >= n_vertices, a coordinate beyond +-2^18 units. */
int tdt_ply_mesh_write(const int32_t *vertices, size_t n_vertices, const uint32_t *triangles, size_t n_triangles, char *buffer,
                       size_t capacity, size_t *bytes);

/* ---------------------------------------------------------------- affine transforms ---------- */
/* Builders of struct tdt_xform (include/tdt_rt.h: the DESTINATION -> SOURCE map s = (a (2 p + 1) + t) >> 17 of
 * tdt_octree_transform / tdt_octree_extract_transform) from the FORWARD transform a caller thinks in.  Each fills *out with
 * material = -1 (keep the source voxel's) and dst = the whole grid (lo 0, hi INT32_MAX); set those two afterwards.  Returns 0,
 * or 0x0501 with a message in tdt_host_last_error and *out untouched: a NULL pointer, a bad axis, an entry beyond the struct's
 * limits (|a| <= 2^20, |t| <= 2^40), a singular matrix.
 * pivot2 is a fixed point of the transform in DOUBLED coordinates: 2 c + 1 is the centre of voxel c, 2 c its low corner; (N, N, N)
 * is the centre of a grid of side N.  The integer builders are exact: with R the forward matrix and P = pivot2,
 * a = 65536 R^-1 and t = 65536 (P - R^-1 P).
 *   identity        a = 65536 I, t = 0: s = p.
 *   translate       the selection moves by d voxels (|d| <= 2^23): t = -d 2^17.
 *   quarter_turns   k quarter turns (any integer, taken mod 4) about `axis` (0 x, 1 y, 2 z) through pivot2; k = 1 takes axis
 *                   (axis + 1) % 3 towards axis (axis + 2) % 3: about z, x towards y, which with pivot2 = (N, N, N) is
 *                   numpy.rot90(grid, 1, axes=(0, 1)) of a grid indexed [x, y, z].  A quarter turn is a bijection of the grid
 *                   (and of the voxel lattice) exactly when the pivot2 components on the two turned axes have EQUAL PARITY;
 *                   with unequal parity voxel centres land on voxel faces and the floor picks a side: still defined, no
 *                   longer one to one.  Half turns (k = 2) and mirrors are bijections of the lattice for every pivot2.
 *   mirror          the reflection of `axis` about the plane through pivot2[axis] (the other two components are not read).
 *   scale           per axis by num / den (both >= 1) about pivot2: a = 65536 den / num rounded to nearest (halves up; exact
 *                   when num divides 65536 den), t = (65536 - a) P, so the pivot stays fixed whatever the rounding.
 *   from_affine     the forward map x' = F x + f on CONTINUOUS coordinates, where voxel c occupies [c, c + 1):
 *                   fwd[4 i + j] = F_ij (j < 3), fwd[4 i + 3] = f_i.  F is inverted in double (adjugate / determinant) and
 *                   a = rint(65536 F^-1), t = rint(-2^17 F^-1 f).  The maps above given as exact doubles reproduce the integer
 *                   builders; in general the last bit rests on the platform's arithmetic and is not pinned.
 *   rotate          by `degrees` about the line through `pivot` (continuous coordinates; the centre of voxel c is c + 1/2) along
 *                   `axis` (any non-zero length), counter-clockwise seen against the axis: Rodrigues' matrix through
 *                   from_affine; cos and sin come from libm, so the last bit is not pinned. */
typedef struct tdt_xform tdt_xform;
int tdt_xform_identity(tdt_xform *out);
int tdt_xform_translate(const int32_t d[3], tdt_xform *out);
int tdt_xform_quarter_turns(int axis, int k, const int32_t pivot2[3], tdt_xform *out);
int tdt_xform_mirror(int axis, const int32_t pivot2[3], tdt_xform *out);
int tdt_xform_scale(const int32_t num[3], const int32_t den[3], const int32_t pivot2[3], tdt_xform *out);
int tdt_xform_from_affine(const double fwd[12], tdt_xform *out);
int tdt_xform_rotate(const double axis[3], double degrees, const double pivot[3], tdt_xform *out);

/* ---------------------------------------------------------------- pick-to-edit --------------- */
/* The DeltaNode (8 floats: the 32-byte std430 stride of octree_update.comp:41-48) for a click on the voxel face a ray query found
 * (tdt_ray_hit, include/tdt_rt.h) — what the reference's click handler (main.rs:551-568) hands Octree::update_vbo, aimed at the
 * face under the cursor instead of a point at a fixed distance.  place = 1: ClickEvent::Left, type 2.0 (LEAF); place = 0:
 * ClickEvent::Right, type 0.0 (EMPTY); value = the active material.  Position: the centre, in unit octree coordinates, of the
 * finest-level cell (2^-max_depth) just outside (place) or just inside (remove) the hit face,
 *     snap((point - min_point) / scale +- normal * 0.5 * 2^-max_depth).
 * octree_floats / octree_ints: the payloads of slots 6 / 7.  Returns 0, or TDT_ERR_INVALID_VALUE (0x0501) when status is not
 * TDT_RAY_HIT, fresh_record == 0, or the position falls outside [0,1)^3 (octree.rs:165-168) — message in tdt_host_last_error. */
typedef struct tdt_ray_hit tdt_ray_hit;
int tdt_pick_edit_delta(const tdt_ray_hit *hit, const float octree_floats[7], const int32_t octree_ints[3], int place, float value,
                        float delta_out[8]);
/* The same finest-level cell as integer grid coordinates in [0, 2^max_depth)^3 (the k of snap's (k + 1/2) 2^-max_depth): just
 * in front of the hit face (place = 1) or just behind it (place = 0).  How a click becomes a brush centre for
 * tdt_octree_edit_region.  Same errors as tdt_pick_edit_delta. */
int tdt_pick_grid_voxel(const tdt_ray_hit *hit, const float octree_floats[7], const int32_t octree_ints[3], int place, int32_t out[3]);
/* The face under the cursor as a seed of the face tools (tdt_octree_edit_faces, include/tdt_rt.h): out[0..2] =
 * tdt_pick_grid_voxel(place = 0), the voxel behind the hit face; out[3] = the face index 0..5 (-x, +x, -y, +y, -z, +z) of the hit
 * normal, which is oriented against the ray and axis-aligned: the component with |n| == 1 gives the axis a, its sign s, and
 * out[3] = 2 a + s.  Same errors as tdt_pick_grid_voxel, and TDT_ERR_INVALID_VALUE for a normal that is not a signed unit axis
 * vector. */
int tdt_pick_face(const tdt_ray_hit *hit, const float octree_floats[7], const int32_t octree_ints[3], int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
