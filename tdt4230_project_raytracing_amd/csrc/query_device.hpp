// The query traversal — one ray through OctreeHit (rc:397-450) as the trace kernel's general build runs it for a fresh invocation
// (zeroed Carry) — as a device function, shared by the kernels that ask "what does this ray hit first?": raycast_kernel
// (tdt_query.hip: the record goes out as a tdt_ray_hit) and guide_kernel (tdt_denoise.hip: four words of it per texel).
// A plain gather: no LDS node table, no jump tables, no bricks — node reads go straight to the cells buffer through a raw buffer
// resource whose range check is the reference's robust access.
#pragma once
#include "trace_device.hpp"

namespace tdt {

struct QueryRecord {                                 // the fields of tdt_ray_hit, before they are packed
  int status;                                        // TDT_RAY_*
  uint32_t material;
  float t;
  int lookups;
  HitTmp rec;
  bool fresh;
  float cmin_x, cmin_y, cmin_z, csize;
};

// the node source of a query: fetch_node's LDS table of zero entries (escape: one uint16 of LDS the block's first lane has set to
// kPackedEscape before a barrier), whose sentinel sends every read to the buffer
TDT_DEV NodeSource query_node_source(const TraceParams &P, const uint16_t *escape) {
  NodeSource ns;
  ns.lds = escape; ns.lds_nodes = 0u; ns.lds_cells = 0u;
  ns.grid = nullptr; ns.grid_ok = false; ns.grid_band = 2.0f; ns.full = nullptr; ns.grid32 = nullptr; ns.bricks = nullptr;
  ns.thr = nullptr; ns.thr_f0max = 0.0f;
  ns.cells = __builtin_amdgcn_make_buffer_rsrc((void *)P.cells, 0, (int)((P.cells_dwords >> 1) << 3), 0x00020000);
  return ns;
}

TDT_DEV QueryRecord query_first_hit(const TraceParams &P, const NodeSource &ns, const Ray &r) {
  // OctreeHit prologue rc:399-408: the root call site (t_min = 0.0003, t_max = +inf)
  const float inf = __builtin_inff();
  float ix, iy, iz;
  q_rcp3(r.dx, r.dy, r.dz, ix, iy, iz);
  const float lx = (P.min_x + -r.ox) * ix, ly = (P.min_y + -r.oy) * iy, lz = (P.min_z + -r.oz) * iz;
  const float ux = ((P.min_x + P.scale) + -r.ox) * ix, uy = ((P.min_y + P.scale) + -r.oy) * iy, uz = ((P.min_z + P.scale) + -r.oz) * iz;
  const float mnx = hw_min(lx, ux), mny = hw_min(ly, uy), mnz = hw_min(lz, uz);
  const float mxx = hw_max(lx, ux), mxy = hw_max(ly, uy), mxz = hw_max(lz, uz);
  const float root_enter = hw_max(hw_max(hw_max(mnx, 0.0003f), mny), mnz);
  const float root_exit = hw_min(hw_min(hw_min(mxx, inf), mxy), mxz);
  const bool root_hit = root_exit >= root_enter;
  HitTmp root = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
  float root_t = 0.f, t_octree_max = inf;
  if (root_hit) {
    cube_hit_record(r, root_enter, P.min_x, P.min_y, P.min_z, P.scale, root);
    root_t = root_enter;
    t_octree_max = root_exit;
  }

  // the loop rc:410-447
  float t_stride = root_t, inv_pow_depth = 0.5f;
  int it = 0;
  QueryRecord q;
  q.status = TDT_RAY_MISS; q.material = 0u; q.t = 0.f; q.lookups = 0;
  q.rec = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
  q.fresh = false;
  q.cmin_x = 0.f; q.cmin_y = 0.f; q.cmin_z = 0.f; q.csize = 0.f;
  Counters cnt = {};
  for (;;) {
    if (!(it < P.max_iter && t_stride < t_octree_max)) {
      q.status = (t_stride < t_octree_max) ? TDT_RAY_ITER_LIMIT : TDT_RAY_MISS;
      break;
    }
    const float adv = f_max(0.0001f * (inv_pow_depth + 0.1f), 0.000001f);
    const float tt = t_stride + adv;
    const float wx = tt * r.dx + r.ox, wy = tt * r.dy + r.oy, wz = tt * r.dz + r.oz;
    const float px = (wx + -P.min_x) * P.inv_scale, py = (wy + -P.min_y) * P.inv_scale, pz = (wz + -P.min_z) * P.inv_scale;
    const float ex = f_fract(px) + -px, ey = f_fract(py) + -py, ez = f_fract(pz) + -pz;
    if ((__builtin_fabsf(ez) + __builtin_fabsf(ey)) != -__builtin_fabsf(ex)) break;    // rc:417: not in the octree -> false
    q.lookups++;
    const float ipd_in = inv_pow_depth;
    float gx, gy, gz; uint32_t value;
    const bool leaf = tree_lookup<false>(P, ns, px, py, pz, inv_pow_depth, gx, gy, gz, value, cnt);
    const float bx = gx * P.scale + P.min_x, by = gy * P.scale + P.min_y, bz = gz * P.scale + P.min_z;
    const float cs0 = P.scale * inv_pow_depth;
    if (leaf) {                                      // rc:421-436
      q.status = TDT_RAY_HIT; q.material = value;
      q.cmin_x = bx; q.cmin_y = by; q.cmin_z = bz; q.csize = cs0;
      if (it > 0) {
        float t_enter, t_exit;
        cube_slabs(r, ix, iy, iz, bx, by, bz, cs0, t_stride, t_octree_max, t_enter, t_exit);
        if (!(t_exit < t_enter)) { cube_hit_record(r, t_enter, bx, by, bz, cs0, q.rec); q.t = t_enter; q.fresh = true; }
      } else {
        q.rec = root; q.t = root_t; q.fresh = root_hit;
      }
      break;
    }
    // rc:438-446: the empty cell, padded
    float t_enter, t_exit;
    cube_slabs(r, ix, iy, iz, bx + -0.00001f, by + -0.00001f, bz + -0.00001f, cs0 + 0.00002f, t_stride, t_octree_max, t_enter, t_exit);
    const float ts_new = !(t_exit < t_enter) ? t_exit : t_octree_max;
    // a step that leaves (t_stride, inv_pow_depth) as it found them repeats itself up to max_iter (the loop body is a function of
    // those two and the ray): the shader ends at the iteration limit with every remaining iteration reaching treeLookup
    if (__float_as_uint(ts_new) == __float_as_uint(t_stride) && __float_as_uint(inv_pow_depth) == __float_as_uint(ipd_in)) {
      q.lookups = P.max_iter;
      q.status = TDT_RAY_ITER_LIMIT;
      break;
    }
    t_stride = ts_new;
    it++;
  }
  return q;
}

}  // namespace tdt
