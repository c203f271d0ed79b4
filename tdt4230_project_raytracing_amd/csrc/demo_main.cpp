// tdt_demo — the reference's main.rs, headless: everything main.rs does between creating the GL context and the
// first `dispatch_compute` (main.rs:156-470, 579), written against include/renderer.hpp (the C++ mirror of
// `src/renderer`), then the frame is read back and written as a PFM instead of being blitted to a window.
//
//   tdt_demo [--size WxH] [--spp N] [--bounce N] [--settings camera.ron] [--move KEYS] [--edit x,y,z,type,value]
//            [--pick X,Y [--click left|right] [--material N]] [--brush sphere:R|box:R] [--box x0,y0,z0,x1,y1,z1]
//            [--op set|fill|paint|clear] [--flood paint|clear] [--match any|material] [--connect 6|26] [--components]
//            [--reach COST [--steps 6|26|345] [--medium solid|empty] [--match-material] [--op ..] [--material K] [--mask ..]]
//            [--morph dilate|erode|open|close|shell:R [--conn 6|26] [--mask x0,y0,z0,x1,y1,z1]] [--cells N]
//            [--morph-round dilate|erode|open|close|shell:R2 [--material K] [--border 0|1] [--mask x0,y0,z0,x1,y1,z1]]
//            [--smooth R2[:ITER] [--threshold Q16] [--smooth-mode both|add|remove] [--material K] [--border 0|1] [--mask ..]]
//            [--transform translate:DX,DY,DZ|turn:AXIS,K|mirror:AXIS|scale:NUM/DEN|rotate:AX,AY,AZ,DEG [--pivot X,Y,Z] [--op ..]
//             [--material K] [--mask x0,y0,z0,x1,y1,z1]]
//            [--mesh FILE.ply [--solid] [--material K] [--op set|fill|paint|clear] [--box x0,y0,z0,x1,y1,z1]]
//            [--fill-enclosed [--conn 6|26] [--material K] [--mask x0,y0,z0,x1,y1,z1]]
//            [--export-mesh FILE.ply [--no-merge] [--any-material] [--mask x0,y0,z0,x1,y1,z1]]
//            [--compact] [--config N] [--device N] [--denoise N [--variance SIGMA]] [--temporal N [--turn DEG]] [--upsample S]
//            [--adaptive TOL [--batch K]] [--preview] [--select-rect X0,Y0,X1,Y1 [--op ..] [--material K]]
//            [--select-through X0,Y0,X1,Y1 | --lasso X,Y;X,Y;... [--window] [--only-material K] [--max-distance D]
//             [--op paint|clear --material K] [--preview]]
//            [--stroke X,Y;X,Y;... --brush sphere:R|box:R [--op set|fill|paint|clear] [--material K]]
//            [--pick X,Y --extrude D [--conn 4|8] [--match-material] [--block 0|1] [--op ..] [--material K] [--mask ..]]
//            [--out frame.pfm] [--png frame.png]
//
// Defaults are the reference's: 1280x720 window (main.rs:26), camera.ron's spp 4 / max_bounce 6 / controller rates.
// --move replays key presses through the camera controller (main.rs:506-546), one 1/60 s frame each:
//   w a s d = translate Front / Left / Back / Rigth, u j = Up / Down, q e = turn_yaw(-/+ 1), r f = turn_pitch(-/+ 1),
//   S / N = sprint / normal speed.  --png writes the frame as the quad pass would present it (main.rs:582-600).
// --denoise N: the frame as accumulate, guide, N filter passes, resolve (ComputeShader::dispatch_guide, Texture::denoise) instead
//   of the one dispatch: running sums averaged within each visible voxel face, before the square root.
// --variance SIGMA (with --denoise N): the N passes are the variance-guided ones (Texture::variance, Texture::denoise_variance): the
//   variance of each pixel's luminance, from its 7x7 same-key neighbourhood or, with --temporal, from the moments of the frames
//   behind it (Texture::reproject_moments) where there are at least 4, scales a second, luminance edge-stopping weight.
// --temporal N [--turn DEG]: N frames instead of one, the camera yawing DEG degrees (default 1) before every frame but the first
//   (turn_yaw takes units of 2 * turn_rate radians; DEG is converted with the camera's turn_rate, that of --settings included),
//   each frame's spp samples joined by the history of the frame before wherever that frame saw the same surface point
//   (ComputeShader::view, Texture::reproject; at most 64 samples of history); the last frame is the one written.  Combines with
//   --denoise, which then filters each frame's means.  Prints the last frame's found / rejected pixel counts.
// --upsample S: the frame's radiance traced at 1 / S of the resolution (S >= 1): accumulate and guide under the camera with
//   image_width = ceil(W / S), image_height = ceil(H / S) into images of that size, the full-resolution guide, Texture::upsample into
//   the render texture, then --denoise N [--variance SIGMA] over it as above, and the resolve.  Prints the bilinear / ring / hole
//   pixel counts.  Not with --temporal.
// --adaptive TOL [--batch K]: the frame's samples in batches of K (default 2) for the pixels that are still noisy
//   (ComputeShader::dispatch_accumulate_masked, Texture::adapt with the guide of sample 0): a pixel stops when the error of its mean
//   luminance is below TOL of it in its whole same-key 3x3 neighbourhood, at the latest with spp samples; then Texture::adapt_mean,
//   --denoise N [--variance SIGMA] over the means (the variance is the batch means' own), and the resolve.  Prints the rounds and
//   the mean samples per pixel.  Not with --temporal or --upsample.
// --pick X,Y [--click left|right] [--material N]: the click handler aimed at pixel (X, Y) of the frame's camera (texture
//   coordinates, row 0 at the bottom; sample 0): prints what the pick hit and, on a hit, places (left, the default) or removes
//   (right) a voxel of material N (default 1) through Octree::update_vbo before the frame is rendered.
// --brush sphere:R|box:R [--op set|fill|paint|clear] [--material N]: with --pick, a region edit instead of the click
//   (Octree::brush): a sphere of radius R, or the cube of half-width R, centred on the grid voxel in front of the picked face
//   (set, the default, / fill) or behind it (paint / clear), brush material N.  Prints the pick and the new cell count.
// --box x0,y0,z0,x1,y1,z1 [--op ..] [--material N]: the same edit over a fixed box of grid voxels (both corners inclusive).
// --flood paint|clear [--match any|material] [--connect 6|26] [--material N]: with --pick, the paint bucket / delete-object
//   tool (Octree::flood): the connected component that holds the grid voxel behind the picked face is painted with material N
//   or removed (neighbours by face, 6, the default, or also by edge and corner, 26; any voxel, the default, or only the same
//   material).  Prints the pick and the new cell count.
// --reach COST [--steps 6|26|345] [--medium solid|empty] [--match-material] [--op set|fill|paint|clear] [--material K]
//   [--mask x0,y0,z0,x1,y1,z1]: with --pick, the soft selection / pouring tool (Octree::reach): every voxel within geodesic cost
//   COST of the picked voxel — walking through the object (solid, the default: from the voxel behind the picked face, through
//   voxels of its material only with --match-material) or through the air (empty: from the voxel in front of it), by face steps
//   (6, the default), face / edge / corner steps of cost 1 (26) or the chamfer weights 3 / 4 / 5 (345), inside the --mask box
//   only — is applied with `op` in material K (solid: default the voxel's own).  Prints the pick and the new cell count.
// --stroke X,Y;X,Y;... --brush sphere:R|box:R [--op set|fill|paint|clear] [--material N]: the brush dragged over the pixels
//   (Octree::stroke): every pixel is picked, each hit gives the grid voxel in front of the face (set, the default, / fill) or
//   behind it (paint / clear), consecutive hits are joined by capsules (sphere) or swept cubes (box) of radius R, a miss breaks
//   the stroke.  Applied after the --pick edits and before --select-rect.  Prints the points used and the new cell count.
// --pick X,Y --extrude D [--conn 4|8] [--match-material] [--block 0|1] [--op set|fill|paint|clear] [--material K] [--mask x0,y0,z0,x1,y1,z1]:
//   the face tools (Octree::extrude): the connected coplanar patch of exposed faces under the pixel (4- or 8-connected inside its
//   plane, of any material or with --match-material of the picked face's only, confined to the --mask box) swept by D voxels along
//   its normal: D > 0 pulls (--op fill or set), D < 0 pushes (--op clear) or, with -1, paints (--op paint); --block 1 stops a pull
//   at an obstacle and a push at the air behind; new voxels get --material or continue the wall's own.  Prints the seed and the
//   new cell count.
// --preview: with --box, --pick --brush or --pick --flood, the edit is not applied: the tree's voxels it would touch are
//   extracted (tdt_octree_extract_region / tdt_octree_extract_connected) and drawn over the finished frame
//   (ComputeShader::dispatch_voxel_ids with place 0, sample 0; Texture::overlay: fill 1, .6, 0, .35, edge 1, .6, 0, 1 of width 1).
//   First hit only: voxels that something hides are not shown.  Prints the list's size and the overlay's pixel counts.
// --select-rect X0,Y0,X1,Y1 [--op set|fill|paint|clear] [--material K]: marquee edit: the distinct voxels visible inside the pixel
//   rectangle (inclusive, row 0 at the bottom; Texture::extract_voxels of the voxel ids of sample 0: for set / fill the empty
//   cells in front of the visible faces, for paint / clear the voxels behind them) get `op` in material K
//   (Octree::edit_voxels), after the picks, before --morph.  Prints the list's size and the new cell count.
// --select-through X0,Y0,X1,Y1 | --lasso X,Y;X,Y;... [--window] [--only-material K] [--max-distance D] [--op paint|clear --material K]
//   [--preview]: the marquee that selects through the model (Octree::extract_screen / edit_screen): every voxel whose centre
//   (--window: all eight of whose corners) projects into the pixel rectangle (inclusive) or the lasso polygon (3..256 vertices,
//   even-odd rule) under the frame's camera, hidden or not, of material K only (--only-material) and no farther than D from the
//   eye (--max-distance).  With --op paint|clear the edit is applied (paint in --material K), after --select-rect and before
//   --morph; without --op, --preview draws the list over the frame.  Prints the list's size and the call's four counts.
// --components [--connect 6|26] [--match any|material]: prints the component count and the largest component's size.
// --morph dilate|erode|open|close|shell:R [--conn 6|26] [--mask x0,y0,z0,x1,y1,z1]: voxel morphology (Octree::morph) of R steps with
//   the 6- (default) or 26-neighbourhood, new voxels inheriting their material, the outside of the grid empty; --mask limits the
//   change to a box of grid voxels (both corners inclusive).  Applied after the other edits, before the frame; prints the new
//   cell count.  --cells N: the cells buffer is uploaded padded with zeros to N cells (room for an edit that grows the tree).
// --morph-round dilate|erode|open|close|shell:R2 [--material K] [--border 0|1] [--mask x0,y0,z0,x1,y1,z1]: round morphology
//   (Octree::morph_round) with the Euclidean ball of SQUARED radius R2 (1..4096); new voxels get --material or inherit their
//   nearest voxel's; --border 1: the outside of the grid is solid.  Applied after --morph; prints the new cell count.
// --smooth R2[:ITER] [--threshold Q16] [--smooth-mode both|add|remove] [--material K] [--border 0|1] [--mask x0,y0,z0,x1,y1,z1]: the
//   smooth brush (Octree::smooth): ITER (default 1) steps of the ball-density threshold filter with the ball of SQUARED radius R2
//   (1..225); a voxel holds after a step when more than half of the ball around it is occupied, or with --threshold at least
//   Q16 / 65536 of it; add / remove only fill dents / shave bumps; new voxels get --material or inherit their nearest voxel's;
//   --border 1 leaves the outside of the grid out of the vote.  Applied after --morph-round; prints the new cell count.
// --transform translate:DX,DY,DZ|turn:AXIS,K|mirror:AXIS|scale:NUM/DEN|rotate:AX,AY,AZ,DEG [--pivot X,Y,Z] [--op set|fill|paint|clear]
//   [--material K] [--mask x0,y0,z0,x1,y1,z1]: move, turn (K quarter turns about AXIS 0 / 1 / 2), mirror, scale or rotate (DEG
//   degrees about the axis AX,AY,AZ) the tree's voxels, those inside the --mask box only, about the voxel corner --pivot (default
//   the centre of the grid) and apply the result with `op` (Octree::transform, the tdt_xform_* builders); the voxels keep their
//   material or get K; the source voxels stay.  Applied after --morph-round; prints the new cell count.
// --mesh FILE.ply [--material K] [--op set|fill|paint|clear] [--box x0,y0,z0,x1,y1,z1]: stamp a triangle mesh (Octree::stamp_mesh):
//   the ASCII PLY's polygons (tdt_ply_mesh_parse; colours ignored) are fitted into the box of grid voxels (tdt_mesh_fit; default
//   the whole grid minus a one-voxel margin; with --mesh, --box is this box, not an edit of its own), quantised and applied with
//   `op` and material K before the frame.  Prints the triangle count, the mesh's voxel count and the new cell count.
//   --solid: the mesh's inside is stamped too (Octree::stamp_mesh_solid): the empty voxels its surface seals off from the
//   grid's faces (by face, --conn 6, the default, or also by edge and corner, --conn 26), in material K; the voxel count printed
//   is the solid's.
// --fill-enclosed [--conn 6|26] [--material K] [--mask x0,y0,z0,x1,y1,z1]: fill the tree's cavities (Octree::fill_enclosed): every
//   empty voxel that no path of empty 6- (default) or 26-neighbours connects to a face of the grid becomes solid, in material K
//   or, without --material, the material of the wall at its -x side; --mask limits the fill to a box of grid voxels.  Applied
//   after --morph, before the frame; prints the number of voxels filled and the new cell count.
// --export-mesh FILE.ply [--no-merge] [--any-material] [--mask x0,y0,z0,x1,y1,z1]: the tree's surface as a triangle mesh
//   (Octree::extract_surface, tdt_quads_to_mesh, tdt_ply_mesh_write): the exposed voxel faces merged into quads (--no-merge: one
//   quad per face; --any-material: quads also merge across materials), of the voxels inside the --mask box only, written as an
//   ASCII PLY in voxel coordinates.  Runs after every edit above, before --compact and the frame; prints the quad, vertex and
//   triangle counts.
// --compact: after the edits, rewrite the tree in place into its canonical form (Octree::compact) before the frame is
//   rendered; prints the census (Octree::census) before and after.
// --config N: the synthetic scene N of libtdthost (tdt_scene_config) instead of main.rs's scene literal, with its own octree
//   parameters (slots 6 / 7) and cell count.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "renderer.hpp"

using namespace renderer;

int main(int argc, char **argv) {
  int W = 1280, H = 720, spp = 4, bounce = 6, device = 0;
  std::string out, png, settings_path, moves, mesh_path, export_path;
  bool export_merge = true, export_by_material = true;
  std::vector<float> edit;
  int pick_x = -1, pick_y = -1, material = 1;
  bool place = true, compact = false, material_given = false, solid = false, fill_enclosed = false;
  int brush_shape = -1, brush_size = 0, op = TDT_REGION_SET;
  int flood_op = -1, connect = 6, match = TDT_MATCH_ANY;
  bool components = false;
  int reach_cost = -1, reach_steps = 6, reach_medium = TDT_MEDIUM_SOLID;
  bool reach_match = false;
  int morph_op = -1, morph_radius = 0, morph_conn = 6;
  std::string morph_name;
  int round_op = -1, round_r2 = 0, round_border = 0;
  std::string round_name;
  int smooth_r2 = 0, smooth_iter = 1, smooth_threshold = 0, smooth_mode = TDT_SMOOTH_BOTH;
  std::string xform_kind;
  double xform_arg[4] = {0, 0, 0, 0};
  std::vector<int32_t> pivot;
  std::vector<int32_t> mask;
  long long pad_cells = 0;
  std::vector<int32_t> box;
  int config = -1, denoise = 0, temporal = 0, upsample = 0, batch = 2;
  float adaptive = -1.0f;
  float turn = 1.0f, variance = 0.0f;                                                    // variance 0: the key-only filter
  bool preview = false;
  std::vector<int32_t> select_rect;
  std::vector<int32_t> through_rect, lasso;                                              // --select-through / --lasso
  std::vector<int32_t> stroke_px;                                                         // --stroke
  int extrude = 0, extrude_block = 0;                                                     // --extrude D, --block 0|1
  bool extrude_given = false, conn_given = false;
  bool through_window = false, op_given = false;
  int only_material = -1;
  float max_distance = INFINITY;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> const char * { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
    auto pixel_list = [](const char *t, std::vector<int32_t> &xy) {                        // X,Y;X,Y;... ; false: something else is left
      int x, y, used;
      while (std::sscanf(t, "%d,%d%n", &x, &y, &used) == 2) { xy.push_back(x); xy.push_back(y); t += used; if (*t == ';') t++; else break; }
      return *t == 0;
    };
    if (a == "--size") { if (std::sscanf(next(), "%dx%d", &W, &H) != 2) { std::fprintf(stderr, "--size WxH\n"); return 2; } }
    else if (a == "--spp") spp = std::atoi(next());
    else if (a == "--bounce") bounce = std::atoi(next());
    else if (a == "--device") device = std::atoi(next());
    else if (a == "--out") out = next();
    else if (a == "--png") png = next();
    else if (a == "--settings") settings_path = next();
    else if (a == "--move") moves = next();
    else if (a == "--edit") { float v[5]; if (std::sscanf(next(), "%f,%f,%f,%f,%f", v, v + 1, v + 2, v + 3, v + 4) != 5) { std::fprintf(stderr, "--edit x,y,z,type,value\n"); return 2; } edit.assign(v, v + 5); }
    else if (a == "--pick") { if (std::sscanf(next(), "%d,%d", &pick_x, &pick_y) != 2 || pick_x < 0 || pick_y < 0) { std::fprintf(stderr, "--pick X,Y\n"); return 2; } }
    else if (a == "--click") { const std::string v = next(); if (v != "left" && v != "right") { std::fprintf(stderr, "--click left|right\n"); return 2; } place = v == "left"; }
    else if (a == "--material") { material = std::atoi(next()); material_given = true; }
    else if (a == "--compact") compact = true;
    else if (a == "--denoise") { denoise = std::atoi(next()); if (denoise < 0 || denoise > 8) { std::fprintf(stderr, "--denoise 0..8\n"); return 2; } }
    else if (a == "--variance") { variance = (float)std::atof(next()); if (!(variance > 0.0f) || !(variance < 1e30f)) { std::fprintf(stderr, "--variance SIGMA, SIGMA > 0\n"); return 2; } }
    else if (a == "--temporal") { temporal = std::atoi(next()); if (temporal < 1) { std::fprintf(stderr, "--temporal N, N >= 1\n"); return 2; } }
    else if (a == "--turn") turn = (float)std::atof(next());
    else if (a == "--adaptive") { adaptive = (float)std::atof(next()); if (!(adaptive >= 0.0f) || !(adaptive < 1e30f)) { std::fprintf(stderr, "--adaptive TOL, TOL >= 0\n"); return 2; } }
    else if (a == "--batch") { batch = std::atoi(next()); if (batch < 1) { std::fprintf(stderr, "--batch K, K >= 1\n"); return 2; } }
    else if (a == "--upsample") { upsample = std::atoi(next()); if (upsample < 1) { std::fprintf(stderr, "--upsample S, S >= 1\n"); return 2; } }
    else if (a == "--brush") {
      char kind[16] = {0};
      if (std::sscanf(next(), "%15[a-z]:%d", kind, &brush_size) != 2 || brush_size < 0 || (std::strcmp(kind, "sphere") && std::strcmp(kind, "box"))) {
        std::fprintf(stderr, "--brush sphere:R|box:R\n"); return 2;
      }
      brush_shape = std::strcmp(kind, "sphere") ? TDT_SHAPE_BOX : TDT_SHAPE_SPHERE;
    }
    else if (a == "--box") { int32_t v[6]; if (std::sscanf(next(), "%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5) != 6) { std::fprintf(stderr, "--box x0,y0,z0,x1,y1,z1\n"); return 2; } box.assign(v, v + 6); }
    else if (a == "--op") {
      const std::string v = next();
      op_given = true;
      if (v == "set") op = TDT_REGION_SET; else if (v == "fill") op = TDT_REGION_FILL; else if (v == "paint") op = TDT_REGION_PAINT;
      else if (v == "clear") op = TDT_REGION_CLEAR; else { std::fprintf(stderr, "--op set|fill|paint|clear\n"); return 2; }
    }
    else if (a == "--flood") {
      const std::string v = next();
      if (v == "paint") flood_op = TDT_REGION_PAINT; else if (v == "clear") flood_op = TDT_REGION_CLEAR;
      else { std::fprintf(stderr, "--flood paint|clear\n"); return 2; }
    }
    else if (a == "--match") {
      const std::string v = next();
      if (v == "any") match = TDT_MATCH_ANY; else if (v == "material") match = TDT_MATCH_MATERIAL;
      else { std::fprintf(stderr, "--match any|material\n"); return 2; }
    }
    else if (a == "--connect") { connect = std::atoi(next()); if (connect != 6 && connect != 26) { std::fprintf(stderr, "--connect 6|26\n"); return 2; } }
    else if (a == "--components") components = true;
    else if (a == "--reach") { reach_cost = std::atoi(next()); if (reach_cost < 0) { std::fprintf(stderr, "--reach COST\n"); return 2; } }
    else if (a == "--steps") { reach_steps = std::atoi(next()); if (reach_steps != 6 && reach_steps != 26 && reach_steps != 345) { std::fprintf(stderr, "--steps 6|26|345\n"); return 2; } }
    else if (a == "--medium") {
      const std::string v = next();
      if (v == "solid") reach_medium = TDT_MEDIUM_SOLID; else if (v == "empty") reach_medium = TDT_MEDIUM_EMPTY;
      else { std::fprintf(stderr, "--medium solid|empty\n"); return 2; }
    }
    else if (a == "--match-material") reach_match = true;
    else if (a == "--morph") {
      char kind[16] = {0};
      static const char *names[5] = {"dilate", "erode", "open", "close", "shell"};
      if (std::sscanf(next(), "%15[a-z]:%d", kind, &morph_radius) == 2)
        for (int k = 0; k < 5; k++) if (!std::strcmp(kind, names[k])) morph_op = k;
      if (morph_op < 0) { std::fprintf(stderr, "--morph dilate|erode|open|close|shell:R\n"); return 2; }
      morph_name = kind;
    }
    else if (a == "--morph-round") {
      static const char *names[5] = {"dilate", "erode", "open", "close", "shell"};   // TDT_MORPH_* order
      char kind[16] = {0};
      if (std::sscanf(next(), "%15[a-z]:%d", kind, &round_r2) == 2)
        for (int k = 0; k < 5; k++) if (!std::strcmp(kind, names[k])) round_op = k;
      if (round_op < 0) { std::fprintf(stderr, "--morph-round dilate|erode|open|close|shell:R2\n"); return 2; }
      round_name = kind;
    }
    else if (a == "--transform") {
      char kind[16] = {0};
      const char *v = next();
      const char *colon = std::strchr(v, ':');
      bool good = colon && std::sscanf(v, "%15[a-z]:", kind) == 1;
      xform_kind = kind;
      double *g = xform_arg;
      if (good && xform_kind == "translate") good = std::sscanf(colon + 1, "%lf,%lf,%lf", g, g + 1, g + 2) == 3;
      else if (good && xform_kind == "turn") good = std::sscanf(colon + 1, "%lf,%lf", g, g + 1) == 2;
      else if (good && xform_kind == "mirror") good = std::sscanf(colon + 1, "%lf", g) == 1;
      else if (good && xform_kind == "scale") good = std::sscanf(colon + 1, "%lf/%lf", g, g + 1) == 2;
      else if (good && xform_kind == "rotate") good = std::sscanf(colon + 1, "%lf,%lf,%lf,%lf", g, g + 1, g + 2, g + 3) == 4;
      else good = false;
      if (!good) { std::fprintf(stderr, "--transform translate:DX,DY,DZ|turn:AXIS,K|mirror:AXIS|scale:NUM/DEN|rotate:AX,AY,AZ,DEG\n"); return 2; }
    }
    else if (a == "--pivot") { int32_t v[3]; if (std::sscanf(next(), "%d,%d,%d", v, v + 1, v + 2) != 3) { std::fprintf(stderr, "--pivot X,Y,Z\n"); return 2; } pivot.assign(v, v + 3); }
    else if (a == "--smooth") {
      if (std::sscanf(next(), "%d:%d", &smooth_r2, &smooth_iter) < 1 || smooth_r2 < 1) { std::fprintf(stderr, "--smooth R2[:ITER]\n"); return 2; }
    }
    else if (a == "--threshold") smooth_threshold = std::atoi(next());
    else if (a == "--smooth-mode") {
      const std::string v = next();
      if (v == "both") smooth_mode = TDT_SMOOTH_BOTH; else if (v == "add") smooth_mode = TDT_SMOOTH_ADD; else if (v == "remove") smooth_mode = TDT_SMOOTH_REMOVE;
      else { std::fprintf(stderr, "--smooth-mode both|add|remove\n"); return 2; }
    }
    else if (a == "--border") { round_border = std::atoi(next()); if (round_border != 0 && round_border != 1) { std::fprintf(stderr, "--border 0|1\n"); return 2; } }
    else if (a == "--conn") { morph_conn = std::atoi(next()); conn_given = true; if (morph_conn != 6 && morph_conn != 26 && morph_conn != 4 && morph_conn != 8) { std::fprintf(stderr, "--conn 6|26 (with --extrude: 4|8)\n"); return 2; } }
    else if (a == "--extrude") { extrude = std::atoi(next()); extrude_given = true; if (extrude < -TDT_FACES_DISTANCE_MAX || extrude > TDT_FACES_DISTANCE_MAX) { std::fprintf(stderr, "--extrude D, -1023..1023\n"); return 2; } }
    else if (a == "--block") { extrude_block = std::atoi(next()); if (extrude_block != 0 && extrude_block != 1) { std::fprintf(stderr, "--block 0|1\n"); return 2; } }
    else if (a == "--mask") { int32_t v[6]; if (std::sscanf(next(), "%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5) != 6) { std::fprintf(stderr, "--mask x0,y0,z0,x1,y1,z1\n"); return 2; } mask.assign(v, v + 6); }
    else if (a == "--cells") { pad_cells = std::atoll(next()); if (pad_cells < 0) { std::fprintf(stderr, "--cells N\n"); return 2; } }
    else if (a == "--mesh") mesh_path = next();
    else if (a == "--solid") solid = true;
    else if (a == "--fill-enclosed") fill_enclosed = true;
    else if (a == "--export-mesh") export_path = next();
    else if (a == "--no-merge") export_merge = false;
    else if (a == "--any-material") export_by_material = false;
    else if (a == "--config") config = std::atoi(next());
    else if (a == "--preview") preview = true;
    else if (a == "--select-rect") { int32_t v[4]; if (std::sscanf(next(), "%d,%d,%d,%d", v, v + 1, v + 2, v + 3) != 4) { std::fprintf(stderr, "--select-rect X0,Y0,X1,Y1\n"); return 2; } select_rect.assign(v, v + 4); }
    else if (a == "--select-through") { int32_t v[4]; if (std::sscanf(next(), "%d,%d,%d,%d", v, v + 1, v + 2, v + 3) != 4) { std::fprintf(stderr, "--select-through X0,Y0,X1,Y1\n"); return 2; } through_rect.assign(v, v + 4); }
    else if (a == "--lasso") {
      if (!pixel_list(next(), lasso) || lasso.size() < 6 || lasso.size() > 2 * TDT_SCREEN_MAX_VERTICES) { std::fprintf(stderr, "--lasso X,Y;X,Y;... (3..256 vertices)\n"); return 2; }
    }
    else if (a == "--stroke") {
      if (!pixel_list(next(), stroke_px) || stroke_px.empty() || stroke_px.size() > 2 * 4096) { std::fprintf(stderr, "--stroke X,Y;X,Y;... (1..4096 pixels)\n"); return 2; }
    }
    else if (a == "--window") through_window = true;
    else if (a == "--only-material") { only_material = std::atoi(next()); if (only_material < 0 || only_material > 253) { std::fprintf(stderr, "--only-material 0..253\n"); return 2; } }
    else if (a == "--max-distance") { max_distance = (float)std::atof(next()); if (!(max_distance >= 0.0f)) { std::fprintf(stderr, "--max-distance D, D >= 0\n"); return 2; } }
    else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
  }
  const bool through = !through_rect.empty() || !lasso.empty();
  if (!through_rect.empty() && !lasso.empty()) { std::fprintf(stderr, "--select-through and --lasso do not combine\n"); return 2; }
  if (!through && (through_window || only_material >= 0 || max_distance != INFINITY)) { std::fprintf(stderr, "--window, --only-material and --max-distance need --select-through or --lasso\n"); return 2; }
  if (through && op_given && op != TDT_REGION_PAINT && op != TDT_REGION_CLEAR) { std::fprintf(stderr, "--select-through / --lasso take --op paint|clear\n"); return 2; }
  if (through && op_given && preview) { std::fprintf(stderr, "--select-through / --lasso: --preview shows the list, --op applies it; not both\n"); return 2; }
  if (!stroke_px.empty() && (brush_shape < 0 || pick_x >= 0 || preview)) { std::fprintf(stderr, "--stroke needs --brush sphere:R|box:R and does not combine with --pick or --preview\n"); return 2; }
  if (extrude_given && (pick_x < 0 || reach_cost >= 0 || flood_op >= 0 || brush_shape >= 0 || preview)) { std::fprintf(stderr, "--extrude needs --pick X,Y and does not combine with --reach, --flood, --brush or --preview\n"); return 2; }
  if (!conn_given && extrude_given) morph_conn = 4;
  if (extrude_given != (morph_conn == 4 || morph_conn == 8)) { std::fprintf(stderr, "--conn 6|26 (with --extrude: 4|8)\n"); return 2; }
  if (extrude_block && !extrude_given) { std::fprintf(stderr, "--block needs --extrude D\n"); return 2; }
  if (variance > 0.0f && denoise == 0) { std::fprintf(stderr, "--variance needs --denoise N\n"); return 2; }
  if (adaptive >= 0.0f && (temporal > 0 || upsample > 0)) { std::fprintf(stderr, "--adaptive does not combine with --temporal or --upsample\n"); return 2; }
  if (upsample > 0 && temporal > 0) { std::fprintf(stderr, "--upsample does not combine with --temporal\n"); return 2; }
  if (solid && mesh_path.empty()) { std::fprintf(stderr, "--solid needs --mesh FILE.ply\n"); return 2; }
  const bool preview_box = !box.empty() && mesh_path.empty(), preview_pick = pick_x >= 0 && reach_cost < 0 && (flood_op >= 0 || brush_shape >= 0);
  if (preview && !through && preview_box == preview_pick) { std::fprintf(stderr, "--preview needs one of --box, --pick with --brush, --pick with --flood\n"); return 2; }
  if (preview && through && (preview_box || preview_pick)) { std::fprintf(stderr, "--preview shows one selection: --select-through / --lasso or --box / --pick\n"); return 2; }
  if (preview && (temporal > 0 || !select_rect.empty())) { std::fprintf(stderr, "--preview does not combine with --temporal or --select-rect\n"); return 2; }
  try {
    Context ctx(device);
    // main.rs:156-160
    ComputeShader raytrace_program = ComputeShader::new_(ctx, TDT_PROGRAM_RAYTRACER);
    // main.rs:164-209 (camera.ron's values arrive as --spp / --bounce)
    Camera camera = CameraBuilder::new_(90.0f, W)
                        .with_aspect_ratio((float)W / (float)H)
                        .with_origin({0.0f, -0.1f, -0.3f})
                        .with_viewport_height(2.0f)
                        .with_sample_per_pixel(spp)
                        .with_max_bounce(bounce)
                        .with_turn_rate(0.05f).with_normal_speed(0.03f).with_sprint_speed(0.15f)
                        .build(ctx, raytrace_program.program);
    if (!settings_path.empty()) {                                                          // main.rs:170-176 / 492-494
      FILE *f = std::fopen(settings_path.c_str(), "rb");
      if (!f) { std::perror(settings_path.c_str()); return 1; }
      std::string text; char buf[4096]; size_t n;
      while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
      std::fclose(f);
      camera.apply_settings(raytrace_program.program, camera_settings_from_ron(text));
      spp = camera.settings().samples_per_pixel; bounce = camera.settings().max_bounce;
      camera.set_speed_to_normal();
    }
    for (char k : moves) {                                                                 // main.rs:506-546
      const double dt = 1.0 / 60.0;
      const Program &prog = raytrace_program.program;
      switch (k) {
        case 'w': camera.translate(prog, into_vector3(Direction::Front), dt); break;
        case 'a': camera.translate(prog, into_vector3(Direction::Left), dt); break;
        case 's': camera.translate(prog, into_vector3(Direction::Back), dt); break;
        case 'd': camera.translate(prog, into_vector3(Direction::Rigth), dt); break;
        case 'u': camera.translate(prog, into_vector3(Direction::Up), dt); break;
        case 'j': camera.translate(prog, into_vector3(Direction::Down), dt); break;
        case 'q': camera.turn_yaw(prog, -1.0f); break;
        case 'e': camera.turn_yaw(prog, 1.0f); break;
        case 'r': camera.turn_pitch(prog, -1.0f); break;
        case 'f': camera.turn_pitch(prog, 1.0f); break;
        case 'S': camera.set_speed_to_sprint(); break;
        case 'N': camera.set_speed_to_normal(); break;
        default: std::fprintf(stderr, "unknown key '%c' in --move\n", k); return 2;
      }
    }
    camera.render_texture.bind();                                                        // main.rs:216
    // main.rs:226-230
    ComputeShader octree_update_program = ComputeShader::new_(ctx, TDT_PROGRAM_OCTREE_UPDATE);
    // main.rs:238-450: the scene literal, one buffer per table, each bound to its shader-storage slot
    tdt_scene *scene = nullptr;
    if (config < 0 ? tdt_scene_demo(&scene) : tdt_scene_config(config, &scene)) { std::fprintf(stderr, "%s\n", tdt_host_last_error()); return 1; }
    // main.rs:455-468's octree parameters, or the synthetic scene's own (its slots 6 / 7 and cell count)
    Vector3f min_point{-0.5f, -0.5f, -1.0f};
    float scale = 1.0f;
    int32_t ints[3] = {10, 100, 100000};
    int64_t counts[6] = {19, 0, 0, 0, 0, 0};
    if (config >= 0) {
      size_t nf = 0, ni = 0;
      const float *f = (const float *)tdt_scene_blob(scene, 6, &nf);
      const int32_t *in = (const int32_t *)tdt_scene_blob(scene, 7, &ni);
      if (nf < 28 || ni < 12 || tdt_scene_counts(scene, counts)) { std::fprintf(stderr, "config %d: no octree parameters\n", config); return 1; }
      min_point = {f[0], f[1], f[2]}; scale = f[4];
      std::memcpy(ints, in, sizeof ints);
    }
    std::vector<VertexBufferObject> keep;
    for (unsigned slot = 0; slot <= 4; slot++) {
      size_t bytes = 0;
      const uint32_t *p = (const uint32_t *)tdt_scene_blob(scene, (int)slot, &bytes);
      std::vector<uint32_t> words(p, p + bytes / 4);
      if (slot == 0 && (size_t)pad_cells * 16 > words.size()) words.resize((size_t)pad_cells * 16, 0u);
      keep.push_back(VertexBufferObject::new_<uint32_t>(ctx, words));
      bind_buffer_base(ctx, TDT_SHADER_STORAGE_BUFFER, slot, keep.back());
    }
    tdt_scene_destroy(scene);
    // main.rs:455-468
    Octree octree = Octree::new_(min_point, scale, ints[0], ints[2], (int)counts[0], ints[1]);
    octree.init_global_buffers(ctx);
    std::vector<int32_t> preview_list;                                                     // --preview: the selection, drawn over the frame
    auto region_voxels = [&](const tdt_region &r) {                                        // the tree's voxels inside r (tdt_octree_extract_region)
      size_t n = 0;
      ctx.check(tdt_octree_extract_region(ctx.raw(), &r, 1, nullptr, 0, &n));
      std::vector<int32_t> v(n * 4);
      if (n) ctx.check(tdt_octree_extract_region(ctx.raw(), &r, 1, v.data(), n, &n));
      return v;
    };
    if (!edit.empty()) {                                                                  // main.rs:555-569, one click
      std::vector<float> delta(500, 0.0f);
      std::copy(edit.begin(), edit.end(), delta.begin());
      octree.update_vbo(delta, 5, octree_update_program);
    }
    if (!mesh_path.empty()) {
      FILE *f = std::fopen(mesh_path.c_str(), "rb");
      if (!f) { std::perror(mesh_path.c_str()); return 1; }
      std::string text; char buf[4096]; size_t got;
      while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
      std::fclose(f);
      tdt_ply_mesh *pm = nullptr;
      if (tdt_ply_mesh_parse(text.data(), text.size(), &pm)) { std::fprintf(stderr, "%s: %s\n", mesh_path.c_str(), tdt_host_last_error()); return 1; }
      int64_t nv = 0, nf = 0, nt = 0;
      tdt_ply_mesh_info(pm, &nv, &nf, &nt);
      const int32_t N = 1 << ints[0];
      int32_t lo[3] = {1, 1, 1}, hi[3] = {N - 2, N - 2, N - 2};
      if (N < 4) { lo[0] = lo[1] = lo[2] = 0; hi[0] = hi[1] = hi[2] = N - 1; }
      if (!box.empty()) for (int a = 0; a < 3; a++) { lo[a] = box[a]; hi[a] = box[3 + a]; }
      double fit_scale = 1.0, fit_offset[3] = {0, 0, 0};
      std::vector<int32_t> q(3 * (size_t)nv);
      if (tdt_mesh_fit(tdt_ply_mesh_vertices(pm), (size_t)nv, lo, hi, &fit_scale, fit_offset) ||
          tdt_mesh_quantize(tdt_ply_mesh_vertices(pm), (size_t)nv, fit_scale, fit_offset, q.data())) {
        std::fprintf(stderr, "%s: %s\n", mesh_path.c_str(), tdt_host_last_error()); tdt_ply_mesh_destroy(pm); return 1;
      }
      const uint32_t *tp = tdt_ply_mesh_triangles(pm);
      const std::vector<uint32_t> tris(tp, tp + 3 * (size_t)nt);
      tdt_ply_mesh_destroy(pm);
      static const char *op_names[4] = {"set", "fill", "paint", "clear"};
      size_t voxels = 0;
      tdt_fill fill{};
      fill.connectivity = morph_conn; fill.material = -1;
      const uint32_t cells = solid ? octree.stamp_mesh_solid(ctx, op, q, tris, material, fill, {}, &voxels) : octree.stamp_mesh(ctx, op, q, tris, material, {}, &voxels);
      std::printf("mesh triangles %lld voxels %zu%s op %s cells %u\n", (long long)nt, voxels, solid ? " solid" : "", op_names[op], cells);
    } else if (!box.empty()) {
      tdt_region r{};
      r.shape = TDT_SHAPE_BOX;
      for (int a = 0; a < 3; a++) { r.a[a] = box[a]; r.b[a] = box[3 + a]; }
      if (preview) { preview_list = region_voxels(r); std::printf("preview box voxels %zu\n", preview_list.size() / 4); }
      else std::printf("box cells %u\n", octree.edit_region(ctx, op, {r}, material));
    }
    if (preview && preview_pick) {                                                       // NEW: the click's selection, not applied
      const tdt_ray_hit h = raytrace_program.pick({{{pick_x, pick_y}}}, 0)[0];
      const float floats[7] = {min_point[0], min_point[1], min_point[2], 0.0f, scale, 1.0f / scale, 1.0f / (float)ints[2]};
      const int side = flood_op < 0 && (op == TDT_REGION_SET || op == TDT_REGION_FILL) ? 1 : 0;   // (as Octree::brush / Octree::flood aim)
      int32_t c[3];
      const bool hit = tdt_pick_grid_voxel(&h, floats, ints, side, c) == 0;
      if (hit && flood_op >= 0) {
        tdt_select sel{};
        sel.connectivity = connect; sel.match = match; sel.min_voxels = 0; sel.max_voxels = 0xFFFFFFFFu;
        size_t n = 0;
        ctx.check(tdt_octree_extract_connected(ctx.raw(), &sel, c, 1, nullptr, 0, nullptr, 0, &n));
        preview_list.resize(n * 4);
        if (n) ctx.check(tdt_octree_extract_connected(ctx.raw(), &sel, c, 1, nullptr, 0, preview_list.data(), n, &n));
      } else if (hit) {
        tdt_region r{};
        r.shape = brush_shape;
        for (int a = 0; a < 3; a++) r.a[a] = c[a];
        if (brush_shape == TDT_SHAPE_SPHERE) r.b[0] = brush_size;
        else for (int a = 0; a < 3; a++) { r.a[a] = c[a] - brush_size; r.b[a] = c[a] + brush_size; }
        preview_list = region_voxels(r);
      }
      std::printf("pick %d,%d status %d material %u fresh %d preview %s voxels %zu\n", pick_x, pick_y, h.status, h.material, h.fresh_record,
                  flood_op >= 0 ? "flood" : "brush", preview_list.size() / 4);
    } else if (pick_x >= 0 && reach_cost >= 0) {                                              // a reach click at the pixel
      tdt_ray_hit h;
      uint32_t cells = 0;
      tdt_geodesic g{};
      g.medium = reach_medium; g.match = -1; g.max_cost = reach_cost;
      g.w[0] = reach_steps == 345 ? 3 : 1; g.w[1] = reach_steps == 345 ? 4 : reach_steps == 26 ? 1 : 0; g.w[2] = reach_steps == 345 ? 5 : reach_steps == 26 ? 1 : 0;
      g.material = (material_given || reach_medium == TDT_MEDIUM_EMPTY) ? material : -1;
      if (reach_match) {                                                                 // only the picked voxel's own material
        const tdt_ray_hit first = raytrace_program.pick({{{pick_x, pick_y}}}, 0)[0];
        if (first.status == TDT_RAY_HIT) g.match = (int32_t)first.material;
      }
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      const bool edited = octree.reach(raytrace_program, pick_x, pick_y, op, g, regions, &h, &cells);
      std::printf("pick %d,%d status %d material %u t %.9g point %.9g,%.9g,%.9g normal %g,%g,%g fresh %d reach %d steps %d medium %s %s cells %u\n",
                  pick_x, pick_y, h.status, h.material, h.t, h.point[0], h.point[1], h.point[2], h.normal[0], h.normal[1], h.normal[2], h.fresh_record,
                  reach_cost, reach_steps, reach_medium == TDT_MEDIUM_SOLID ? "solid" : "empty", edited ? "applied" : "none", cells);
    } else if (pick_x >= 0 && extrude_given) {                                           // the face under the pixel pulled, pushed or painted
      tdt_faces f{};
      f.connectivity = morph_conn; f.match = reach_match ? TDT_MATCH_MATERIAL : TDT_MATCH_ANY; f.distance = extrude; f.block = extrude_block;
      f.material = material_given ? material : -1;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      int32_t seed[4] = {-1, -1, -1, 0};
      uint32_t cells = 0;
      static const char *op_names[4] = {"set", "fill", "paint", "clear"};
      const bool edited = octree.extrude(raytrace_program, pick_x, pick_y, op, f, regions, seed, &cells);
      if (edited) std::printf("extrude seed %d,%d,%d face %d distance %d op %s cells %u\n", seed[0], seed[1], seed[2], seed[3], extrude, op_names[op], cells);
      else std::printf("extrude pick %d,%d none\n", pick_x, pick_y);
    } else if (pick_x >= 0 && flood_op >= 0) {                                           // a flood click at the pixel
      tdt_ray_hit h;
      uint32_t cells = 0;
      tdt_select sel{};
      sel.connectivity = connect; sel.match = match; sel.min_voxels = 0; sel.max_voxels = 0xFFFFFFFFu;
      const bool edited = octree.flood(raytrace_program, pick_x, pick_y, flood_op, sel, material, &h, &cells);
      std::printf("pick %d,%d status %d material %u t %.9g point %.9g,%.9g,%.9g normal %g,%g,%g fresh %d flood %s cells %u\n", pick_x, pick_y,
                  h.status, h.material, h.t, h.point[0], h.point[1], h.point[2], h.normal[0], h.normal[1], h.normal[2], h.fresh_record,
                  edited ? "applied" : "none", cells);
    } else if (pick_x >= 0 && brush_shape >= 0) {                                        // a brush click at the pixel
      tdt_ray_hit h;
      uint32_t cells = 0;
      const bool edited = octree.brush(raytrace_program, pick_x, pick_y, brush_shape, brush_size, op, material, &h, &cells);
      std::printf("pick %d,%d status %d material %u t %.9g point %.9g,%.9g,%.9g normal %g,%g,%g fresh %d brush %s cells %u\n", pick_x, pick_y,
                  h.status, h.material, h.t, h.point[0], h.point[1], h.point[2], h.normal[0], h.normal[1], h.normal[2], h.fresh_record,
                  edited ? "applied" : "none", cells);
    } else if (pick_x >= 0) {                                                            // main.rs:551-568, aimed at the pixel
      tdt_ray_hit h;
      const bool edited = octree.click(raytrace_program, pick_x, pick_y, place, (float)material, octree_update_program, &h);
      std::printf("pick %d,%d status %d material %u t %.9g iterations %d point %.9g,%.9g,%.9g normal %g,%g,%g fresh %d edit %s\n",
                  pick_x, pick_y, h.status, h.material, h.t, h.iterations, h.point[0], h.point[1], h.point[2], h.normal[0], h.normal[1],
                  h.normal[2], h.fresh_record, edited ? (place ? "place" : "remove") : "none");
    }
    if (!stroke_px.empty()) {                                                             // NEW: a brush dragged over the pixels
      std::vector<std::array<int32_t, 2>> px(stroke_px.size() / 2);
      for (size_t k = 0; k < px.size(); k++) px[k] = {stroke_px[2 * k], stroke_px[2 * k + 1]};
      std::vector<int32_t> pts;
      static const char *op_names[4] = {"set", "fill", "paint", "clear"};
      const uint32_t cells = octree.stroke(raytrace_program, px, brush_shape, brush_size, op, material, &pts);
      std::printf("stroke pixels %zu points %zu:", px.size(), pts.size() / 3);
      for (size_t k = 0; k < pts.size(); k += 3) std::printf(" %d,%d,%d", pts[k], pts[k + 1], pts[k + 2]);
      std::printf(" op %s cells %u\n", op_names[op], cells);
    }
    if (!select_rect.empty()) {                                                           // NEW: marquee: `op` over what the rectangle shows
      const Texture ids = Texture::new_2d(ctx, camera.render_texture.width(), camera.render_texture.height(), false);
      raytrace_program.dispatch_voxel_ids(ids, op == TDT_REGION_SET || op == TDT_REGION_FILL ? 1 : 0, 0);
      std::vector<int32_t> list = ids.extract_voxels(select_rect.data());
      if (op != TDT_REGION_CLEAR) for (size_t i = 3; i < list.size(); i += 4) list[i] = material + 1;
      static const char *op_names[4] = {"set", "fill", "paint", "clear"};
      std::printf("select-rect %d,%d,%d,%d op %s voxels %zu cells %u\n", select_rect[0], select_rect[1], select_rect[2], select_rect[3], op_names[op],
                  list.size() / 4, octree.edit_voxels(ctx, op, list));
    }
    if (through) {                                                                        // NEW: the marquee that selects through the model
      tdt_screen_select q{};
      q.shape = lasso.empty() ? TDT_SCREEN_RECT : TDT_SCREEN_POLYGON;
      for (int a = 0; a < 4 && lasso.empty(); a++) q.rect[a] = through_rect[a];
      q.flags = through_window ? TDT_SCREEN_WINDOW : 0u; q.material = only_material; q.min_distance = 0.0f; q.max_distance = max_distance;
      const tdt_view view = raytrace_program.view();
      uint64_t counts[4];
      if (op_given) {
        static const char *op_names[4] = {"set", "fill", "paint", "clear"};
        const uint32_t cells = octree.edit_screen(ctx, op, view, q, lasso, nullptr, material);
        ctx.check(tdt_debug_screen_counts(ctx.raw(), counts));
        std::printf("select-through op %s voxels %llu on-screen %llu in-shape %llu selected %llu cells %u\n", op_names[op], (unsigned long long)counts[0],
                    (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3], cells);
      } else {
        const std::vector<int32_t> list = octree.extract_screen(ctx, view, q, lasso);
        ctx.check(tdt_debug_screen_counts(ctx.raw(), counts));
        std::printf("select-through voxels %llu on-screen %llu in-shape %llu selected %llu list %zu\n", (unsigned long long)counts[0],
                    (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3], list.size() / 4);
        if (preview) preview_list = list;
      }
    }
    if (morph_op >= 0) {
      tdt_morph m{};
      m.op = morph_op; m.connectivity = morph_conn; m.radius = morph_radius; m.material = -1; m.border = 0;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      std::printf("morph %s:%d conn %d cells %u\n", morph_name.c_str(), morph_radius, morph_conn, octree.morph(ctx, m, regions));
    }
    if (round_op >= 0) {
      tdt_round q{};
      q.op = round_op; q.radius2 = round_r2; q.material = material_given ? material : -1; q.border = round_border;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      std::printf("morph-round %s:%d border %d cells %u\n", round_name.c_str(), round_r2, round_border, octree.morph_round(ctx, q, regions));
    }
    if (smooth_r2 > 0) {
      tdt_smooth q{};
      q.radius2 = smooth_r2; q.iterations = smooth_iter; q.threshold = smooth_threshold; q.mode = smooth_mode;
      q.material = material_given ? material : -1; q.border = round_border;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      std::printf("smooth %d:%d threshold %d mode %d border %d cells %u\n", smooth_r2, smooth_iter, smooth_threshold, smooth_mode, round_border,
                  octree.smooth(ctx, q, regions));
    }
    if (!xform_kind.empty()) {
      const int32_t half = 1 << (ints[0] - 1);
      const int32_t corner[3] = {pivot.empty() ? half : pivot[0], pivot.empty() ? half : pivot[1], pivot.empty() ? half : pivot[2]};
      const int32_t pivot2[3] = {2 * corner[0], 2 * corner[1], 2 * corner[2]};             // a voxel corner, doubled
      const double *g = xform_arg;
      tdt_xform x;
      int rc = 0;
      if (xform_kind == "translate") { const int32_t d[3] = {(int32_t)g[0], (int32_t)g[1], (int32_t)g[2]}; rc = tdt_xform_translate(d, &x); }
      else if (xform_kind == "turn") rc = tdt_xform_quarter_turns((int)g[0], (int)g[1], pivot2, &x);
      else if (xform_kind == "mirror") rc = tdt_xform_mirror((int)g[0], pivot2, &x);
      else if (xform_kind == "scale") {
        const int32_t num[3] = {(int32_t)g[0], (int32_t)g[0], (int32_t)g[0]}, den[3] = {(int32_t)g[1], (int32_t)g[1], (int32_t)g[1]};
        rc = tdt_xform_scale(num, den, pivot2, &x);
      } else {
        const double centre[3] = {(double)corner[0], (double)corner[1], (double)corner[2]};
        rc = tdt_xform_rotate(g, g[3], centre, &x);
      }
      if (rc != 0) { std::fprintf(stderr, "--transform: %s\n", tdt_host_last_error()); return 2; }
      x.material = material_given ? material : -1;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      std::printf("transform %s cells %u\n", xform_kind.c_str(), octree.transform(ctx, x, op, regions));
    }
    if (fill_enclosed) {
      tdt_fill fill{};
      fill.connectivity = morph_conn; fill.material = material_given ? material : -1;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      size_t voxels = 0;
      const uint32_t cells = octree.fill_enclosed(ctx, fill, regions, &voxels);
      std::printf("fill-enclosed conn %d voxels %zu cells %u\n", morph_conn, voxels, cells);
    }
    if (!export_path.empty()) {
      tdt_surface opt{};
      opt.merge = export_merge ? 1 : 0; opt.by_material = export_by_material ? 1 : 0;
      std::vector<tdt_region> regions;
      if (!mask.empty()) {
        tdt_region r{};
        r.shape = TDT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) { r.a[a] = mask[a]; r.b[a] = mask[3 + a]; }
        regions.push_back(r);
      }
      const std::vector<tdt_quad> quads = octree.extract_surface(ctx, opt, regions);
      const int32_t *q = quads.empty() ? nullptr : &quads[0].face;
      size_t nv = 0, nt = 0, bytes = 0;
      if (tdt_quads_to_mesh(q, quads.size(), nullptr, 0, &nv, nullptr, nullptr, 0, &nt)) { std::fprintf(stderr, "%s\n", tdt_host_last_error()); return 1; }
      std::vector<int32_t> vertices(3 * nv + 1);
      std::vector<uint32_t> triangles(3 * nt + 1);
      if (!quads.empty() && tdt_quads_to_mesh(q, quads.size(), vertices.data(), nv, &nv, triangles.data(), nullptr, nt, &nt)) {
        std::fprintf(stderr, "%s\n", tdt_host_last_error()); return 1;
      }
      if (tdt_ply_mesh_write(vertices.data(), nv, triangles.data(), nt, nullptr, 0, &bytes)) { std::fprintf(stderr, "%s\n", tdt_host_last_error()); return 1; }
      std::vector<char> text(bytes + 1);
      if (tdt_ply_mesh_write(vertices.data(), nv, triangles.data(), nt, text.data(), bytes, &bytes)) { std::fprintf(stderr, "%s\n", tdt_host_last_error()); return 1; }
      FILE *f = std::fopen(export_path.c_str(), "wb");
      if (!f) { std::perror(export_path.c_str()); return 1; }
      const bool written = std::fwrite(text.data(), 1, bytes, f) == bytes;
      if (std::fclose(f) != 0 || !written) { std::fprintf(stderr, "%s: short write\n", export_path.c_str()); return 1; }
      std::printf("export-mesh %s%s quads %zu vertices %zu triangles %zu\n", export_merge ? "merged" : "unmerged",
                  export_by_material ? "" : " any-material", quads.size(), nv, nt);
    }
    if (components) {
      const std::vector<tdt_component> table = octree.components(ctx, connect, match);
      uint32_t largest = 0;
      for (const tdt_component &c : table) largest = c.voxels > largest ? c.voxels : largest;
      std::printf("components %zu largest %u\n", table.size(), largest);
    }
    if (compact) {
      auto print = [](const char *when, const std::array<int64_t, 6> &c) {
        std::printf("census %s reachable %lld leaves %lld voxels %lld max_cell %lld buffer_cells %lld counter %lld\n", when, (long long)c[0],
                    (long long)c[1], (long long)c[2], (long long)c[3], (long long)c[4], (long long)c[5]);
      };
      print("before", octree.census(ctx));
      std::printf("compact cells %u\n", octree.compact(ctx));
      print("after", octree.census(ctx));
    }
    // main.rs:578-580
    octree.vao.bind();
    const int dw = camera.render_texture.width() + 1, dh = camera.render_texture.height() + 1, dd = camera.render_texture.depth();
    if (temporal > 0) {                                                                  // NEW: a turn of `temporal` frames with history
      const int tw = camera.render_texture.width(), th = camera.render_texture.height();
      const Texture hist[2] = {Texture::new_2d(ctx, tw, th, false), Texture::new_2d(ctx, tw, th, false)};
      const Texture guides[2] = {Texture::new_2d(ctx, tw, th, false), Texture::new_2d(ctx, tw, th, false)};
      std::vector<Texture> moments;                                                      // (two more images, only with --variance)
      if (variance > 0.0f) for (int i = 0; i < 2; i++) moments.push_back(Texture::new_2d(ctx, tw, th, false));
      const tdt_compute *const prog = raytrace_program.program.id();
      tdt_view prev_view = {};
      // turn_yaw(angle) rotates by 2 * angle * turn_rate radians (camera.rs:56-62), so DEG degrees are this many of its units
      const float turn_units = turn * 0.017453292519943295f / (2.0f * camera.settings().turn_rate);
      for (int k = 0; k < temporal; k++) {
        const int cur = k & 1, old = cur ^ 1;
        if (k) { camera.turn_yaw(raytrace_program.program, turn_units); camera.render_texture.clear(); }
        ctx.check(tdt_dispatch_accumulate(raytrace_program.program.id(), dw, dh, dd, k * spp, spp, nullptr));
        raytrace_program.dispatch_guide(guides[cur], k * spp);
        if (variance > 0.0f) {
          camera.render_texture.reproject_moments(raytrace_program, k * spp, guides[cur], spp, k ? &prev_view : nullptr, k ? &guides[old] : nullptr,
                                                  k ? &hist[old] : nullptr, k ? &moments[old] : nullptr, 64.0f, hist[cur], moments[cur],
                                                  &camera.render_texture);
          camera.render_texture.variance(guides[cur], &moments[cur]);
          camera.render_texture.denoise_variance(guides[cur], denoise, variance);
        } else {
          camera.render_texture.reproject(raytrace_program, k * spp, guides[cur], spp, k ? &prev_view : nullptr, k ? &guides[old] : nullptr,
                                          k ? &hist[old] : nullptr, 64.0f, hist[cur], &camera.render_texture);
          if (denoise > 0) camera.render_texture.denoise(guides[cur], denoise);
        }
        ctx.check(tdt_dispatch_resolve(raytrace_program.program.id(), dw, dh, dd, 1));
        ctx.check(tdt_compute_view(prog, &prev_view));
      }
      uint64_t counts[4];
      ctx.check(tdt_debug_reproject_counts(ctx.raw(), counts));
      std::printf("temporal frames %d keyed %llu found %llu rejected-key %llu rejected-screen %llu\n", temporal, (unsigned long long)counts[0],
                  (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3]);
    } else if (upsample > 0) {                                                           // NEW: radiance at 1 / upsample of the resolution
      const int tw = camera.render_texture.width(), th = camera.render_texture.height();
      const int lw = (tw + upsample - 1) / upsample, lh = (th + upsample - 1) / upsample;
      const Texture guide = Texture::new_2d(ctx, tw, th, false), low = Texture::new_2d(ctx, lw, lh, false), low_guide = Texture::new_2d(ctx, lw, lh, false);
      const Program &prog = raytrace_program.program;
      prog.set_i32("camera.image_width", lw); prog.set_i32("camera.image_height", lh);
      low.bind();
      ctx.check(tdt_dispatch_accumulate(prog.id(), (lw + 31) / 32 * 32, (lh + 31) / 32 * 32, dd, 0, spp, nullptr));   // (all of the low image)
      raytrace_program.dispatch_guide(low_guide);
      prog.set_i32("camera.image_width", tw); prog.set_i32("camera.image_height", th);
      camera.render_texture.bind();
      raytrace_program.dispatch_guide(guide);
      camera.render_texture.upsample(guide, low, low_guide);
      if (variance > 0.0f) {
        camera.render_texture.variance(guide);
        camera.render_texture.denoise_variance(guide, denoise, variance);
      } else if (denoise > 0) {
        camera.render_texture.denoise(guide, denoise);
      }
      ctx.check(tdt_dispatch_resolve(prog.id(), dw, dh, dd, spp));
      uint64_t counts[4];
      ctx.check(tdt_debug_upsample_counts(ctx.raw(), counts));
      std::printf("upsample %d from %dx%d pixels %llu bilinear %llu ring %llu holes %llu\n", upsample, lw, lh, (unsigned long long)counts[0],
                  (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3]);
    } else if (adaptive >= 0.0f) {                                                       // NEW: batches of samples for the pixels that are still noisy
      const int tw = camera.render_texture.width(), th = camera.render_texture.height();
      const Texture guide = Texture::new_2d(ctx, tw, th, false), carry = Texture::new_2d(ctx, 4 * tw, th, false);   // (carry: 16 floats per pixel)
      const Texture states[2] = {Texture::new_2d(ctx, tw, th, false), Texture::new_2d(ctx, tw, th, false)};
      const tdt_adapt limits = {adaptive, 0.05f, 4, spp};                                // the cap is the camera's samples per pixel
      camera.render_texture.clear();
      uint64_t counts[4] = {0, 0, 0, 0}, samples = 0;
      int cur = 0, rounds = 0;
      for (int begin = 0;; begin += batch) {
        raytrace_program.dispatch_accumulate_masked(dw, dh, dd, begin, batch, tdt_image_device_ptr(carry.id()), states[cur]);
        if (begin == 0) raytrace_program.dispatch_guide(guide);
        camera.render_texture.adapt(&guide, states[cur], states[cur ^ 1], batch, limits);
        cur ^= 1; rounds++;
        ctx.check(tdt_debug_adapt_counts(ctx.raw(), counts));
        samples += counts[0] * (uint64_t)batch;
        if (counts[3] == 0) break;
      }
      camera.render_texture.adapt_mean(states[cur]);
      if (variance > 0.0f) camera.render_texture.denoise_variance(guide, denoise, variance);    // (alpha: the batch-mean variance adapt_mean left)
      else if (denoise > 0) camera.render_texture.denoise(guide, denoise);
      ctx.check(tdt_dispatch_resolve(raytrace_program.program.id(), dw, dh, dd, 1));
      std::printf("adaptive %g batch %d rounds %d mean spp %.3f of %d\n", (double)adaptive, batch, rounds,
                  (double)samples / ((double)tw * (double)th), spp);
    } else if (denoise > 0) {                                                            // NEW: sums, first hits, filter, then the square root
      const Texture guide = Texture::new_2d(ctx, camera.render_texture.width(), camera.render_texture.height(), false);
      ctx.check(tdt_dispatch_accumulate(raytrace_program.program.id(), dw, dh, dd, 0, spp, nullptr));
      raytrace_program.dispatch_guide(guide);
      if (variance > 0.0f) {
        camera.render_texture.variance(guide);
        camera.render_texture.denoise_variance(guide, denoise, variance);
      } else {
        camera.render_texture.denoise(guide, denoise);
      }
      ctx.check(tdt_dispatch_resolve(raytrace_program.program.id(), dw, dh, dd, spp));
    } else {
      raytrace_program.dispatch_compute(dw, dh, dd);
    }
    if (preview) {                                                                       // NEW: the selection over the resolved frame
      const Texture ids = Texture::new_2d(ctx, camera.render_texture.width(), camera.render_texture.height(), false);
      raytrace_program.dispatch_voxel_ids(ids, 0, 0);
      const tdt_overlay style = {{1.0f, 0.6f, 0.0f, 0.35f}, {1.0f, 0.6f, 0.0f, 1.0f}, 1, 0u};
      camera.render_texture.overlay(ids, preview_list, style);
      uint64_t counts[4];
      ctx.check(tdt_debug_overlay_counts(ctx.raw(), counts));
      std::printf("preview voxels %zu pixels %llu with-voxel %llu member %llu edge %llu\n", preview_list.size() / 4, (unsigned long long)counts[0],
                  (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3]);
    }
    VertexArrayObject::unbind();
    const std::vector<float> px = camera.render_texture.read();
    unsigned long long h = 1469598103934665603ull;                                        // FNV-1a of the frame's bits
    for (float f : px) { uint32_t u; std::memcpy(&u, &f, 4); for (int b = 0; b < 4; b++) { h ^= (u >> (8 * b)) & 0xff; h *= 1099511628211ull; } }
    std::printf("%dx%d spp %d bounce %d fnv1a %016llx counter %d\n", camera.image_width(), camera.image_height(), spp, bounce, h,
                octree.counter().read<int32_t>(1)[0]);
    if (!out.empty()) {
      FILE *f = std::fopen(out.c_str(), "wb");
      if (!f) { std::perror(out.c_str()); return 1; }
      std::fprintf(f, "PF4\n%d %d\n-1.0\n", camera.image_width(), camera.image_height());     // 4-channel little-endian float map, bottom row first
      std::fwrite(px.data(), sizeof(float), px.size(), f);
      std::fclose(f);
    }
    if (!png.empty()) present_png(camera.render_texture, png);                           // instead of main.rs:582-600
  } catch (const InitializeErr &e) {
    std::fprintf(stderr, "InitializeErr: %s (%s)\n", e.to_string().c_str(), e.detail.c_str());
    return 1;
  }
  return 0;
}
