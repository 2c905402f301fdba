// bake.hip -- per-Gaussian ambient occlusion bake (baking.py bake_set).
//
// Built with -ffp-contract=off like geometry.hip, so the projection (project.h) gives the rasterizer's preprocess bits; the
// blend step is the contribution rule of blend_common.h, which turns contraction back on locally, as the blend files are built.
//
//   grid       pc_to_grid(points, 10): bounding box, cell index per point, the occupied cells compacted in (ix, iy, iz)
//              lexicographic order (torch.unique's order), centres min + idx * size + size / 2
//   plan       cov3D of every Gaussian (view-independent), the needed texels of the cube (the nearest texel of each direction)
//              as per-(face, tile) pixel lists, and the (Gaussian, tile) instance count of every (cell, face, tile)
//   visibility per batch of cells: bucket the instances of the batch's (cell, face, tile) tile space, sort each tile's list by
//              (depth, Gaussian id) with the tile-bucket back-end's sorts, blend only the needed pixels (a wave per tile),
//              gather 1 - weight per direction
//   expand     occ[p][hw] = (dir_hw . n_p > 0) * vis[cell(p)][hw]
//   env reduce clamp(sum_hw clamp(occ, 0, 1) * env[hw], 0, 1) per Gaussian, three copies
#include <vector>

#include "blend_common.h"
#include "project.h"

namespace gsr {

constexpr int BK_RES = 10;                     // grid cells per axis
constexpr int BK_CELLS = BK_RES * BK_RES * BK_RES;
constexpr int BK_N = 32;                       // cube face size
constexpr int BK_TEX = 6 * BK_N * BK_N;        // texels per cube
constexpr int BK_TILES = 6 * 4;                // (face, tile) per cell: 2 x 2 tiles of 16 x 16 per face
constexpr int BK_BLOCK = 256;

// ---- grid ------------------------------------------------------------------------------------------------------------
struct GridWs {
  float *bbox;     // [6] min xyz, max xyz
  uint32_t *flags;  // [1000] occupied
  int *map;        // [1000] compact id or -1
  uint32_t *count;  // [1]
};
inline GridWs grid_ws(void *ws, size_t *end = nullptr) {
  GridWs w;
  uintptr_t p = carve_begin(ws);
  carve(p, w.bbox, 8);
  carve(p, w.flags, BK_CELLS);
  carve(p, w.map, BK_CELLS);
  carve(p, w.count, 4);
  if (end) *end = p;
  return w;
}

__global__ __launch_bounds__(1024) void bake_bbox_kernel(int P, const float *pts, GridWs w) {
  __shared__ float s[6][1024];
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int i = threadIdx.x; i < P; i += 1024)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v = pts[3 * (size_t)i + k];
      lo[k] = fminf(lo[k], v);
      hi[k] = fmaxf(hi[k], v);
    }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s[k][threadIdx.x] = lo[k];
    s[3 + k][threadIdx.x] = hi[k];
  }
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
#pragma unroll
      for (int k = 0; k < 3; k++) {
        s[k][threadIdx.x] = fminf(s[k][threadIdx.x], s[k][threadIdx.x + h]);
        s[3 + k][threadIdx.x] = fmaxf(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + h]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) w.bbox[threadIdx.x] = s[threadIdx.x][0];
  for (int i = threadIdx.x; i < BK_CELLS; i += 1024) w.flags[i] = 0u;
}

// size = (max - min) / 10 as torch evaluates it on the GPU: a division by a host scalar is a multiplication by its float
// reciprocal there (0.1f), not an IEEE division
constexpr float GRID_INV = 1.0f / (float)BK_RES;
// idx = clamp(floor((p - min) / size), 0, 9); a zero-extent axis (0 / 0) gets index 0
__device__ __forceinline__ int grid_axis(float p, float lo, float size) {
  const float q = floorf((p - lo) / size);
  if (!(q == q)) return 0;
  return q < 0.f ? 0 : (q > (float)(BK_RES - 1) ? BK_RES - 1 : (int)q);
}

__global__ __launch_bounds__(BK_BLOCK) void bake_cell_kernel(int P, const float *pts, GridWs w, int *cell) {
  const int i = blockIdx.x * BK_BLOCK + threadIdx.x;
  if (i >= P) return;
  int id[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float lo = w.bbox[k], size = (w.bbox[3 + k] - lo) * GRID_INV;
    id[k] = grid_axis(pts[3 * (size_t)i + k], lo, size);
  }
  const int lin = (id[0] * BK_RES + id[1]) * BK_RES + id[2];
  cell[i] = lin;
  w.flags[lin] = 1u;
}

__global__ __launch_bounds__(1024) void bake_compact_kernel(GridWs w, float *centres, float *size_out, int *cell_idx) {
  __shared__ uint32_t wtot[1024 / WAVE];
  const int t = threadIdx.x;
  const uint32_t occ = t < BK_CELLS ? w.flags[t] : 0u;
  const uint32_t incl_w = wave_incl_scan(occ);
  const int wave = t / WAVE, lane = t % WAVE;
  if (lane == WAVE - 1) wtot[wave] = incl_w;
  __syncthreads();
  uint32_t base = 0;
  for (int k = 0; k < wave; k++) base += wtot[k];
  const uint32_t id = base + incl_w - occ;
  float size[3], lo[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    lo[k] = w.bbox[k];
    size[k] = (w.bbox[3 + k] - lo[k]) * GRID_INV;
  }
  if (t < BK_CELLS) {
    w.map[t] = occ ? (int)id : -1;
    if (occ) {
      const int ix[3] = {t / (BK_RES * BK_RES), (t / BK_RES) % BK_RES, t % BK_RES};
#pragma unroll
      for (int k = 0; k < 3; k++) {
        centres[3 * id + k] = (lo[k] + (float)ix[k] * size[k]) + size[k] / 2.0f;
        if (cell_idx) cell_idx[3 * id + k] = ix[k];
      }
    }
  }
  if (t == 1023) *w.count = base + incl_w;
  if (t < 3 && size_out) size_out[t] = size[t];
}

__global__ __launch_bounds__(BK_BLOCK) void bake_remap_kernel(int P, GridWs w, int *cell) {
  const int i = blockIdx.x * BK_BLOCK + threadIdx.x;
  if (i < P) cell[i] = w.map[cell[i]];
}

// ---- plan ------------------------------------------------------------------------------------------------------------
struct PlanWs {
  float *cov3D;        // [P][6]
  uint32_t *counts;    // [C][24] instances per (cell, face, tile)
  uint16_t *pix;       // [24][256] needed pixels (y * 32 + x within the face) per (face, tile)
  int *npix;           // [24]
};
inline PlanWs plan_ws(void *ws, int P, int C, size_t *end = nullptr) {
  PlanWs w;
  uintptr_t p = carve_begin(ws);
  carve(p, w.cov3D, (size_t)P * 6);
  carve(p, w.counts, (size_t)C * BK_TILES);
  carve(p, w.pix, (size_t)BK_TILES * 256);
  carve(p, w.npix, BK_TILES);
  if (end) *end = p;
  return w;
}

__global__ __launch_bounds__(BK_BLOCK) void bake_cov3d_kernel(int P, const float *scales, const float *rots, float *cov3D) {
  const int i = blockIdx.x * BK_BLOCK + threadIdx.x;
  if (i >= P) return;
  float c6[6];
  cov3d_from_scale_rot(make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]), 1.0f,
                       make_float4(rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]), c6);
#pragma unroll
  for (int k = 0; k < 6; k++) cov3D[6 * (size_t)i + k] = c6[k];
}

// needed texels -> per-(face, tile) pixel lists in pixel order (one workgroup)
__global__ __launch_bounds__(1024) void bake_pixels_kernel(const int *dir_texel, int ndir, PlanWs w) {
  __shared__ uint8_t need[BK_TEX];
  for (int i = threadIdx.x; i < BK_TEX; i += 1024) need[i] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < ndir; i += 1024) {
    const int t = dir_texel[i];
    if (t >= 0 && t < BK_TEX) need[t] = 1;
  }
  __syncthreads();
  if (threadIdx.x < BK_TILES) {
    const int ft = threadIdx.x, f = ft / 4, ty = (ft % 4) / 2, tx = ft % 2;
    int n = 0;
    for (int ly = 0; ly < TILE; ly++)
      for (int lx = 0; lx < TILE; lx++) {
        const int pix = (ty * TILE + ly) * BK_N + tx * TILE + lx;
        if (need[f * BK_N * BK_N + pix]) w.pix[ft * 256 + n++] = (uint16_t)pix;
      }
    w.npix[ft] = n;
  }
}

// The rasterizer's preprocess of Gaussian g for one cube-face camera (32 x 32, tanfov 1): geometry.hip preprocess_forward_kernel
// step for step (project.h), without colour.
struct BakeProj {
  float x, y, ca, cb, cc, depth;
  int x0, y0, x1, y1;
};
__device__ __forceinline__ bool bake_project(const float3 p, const float *c6, const float *view, const float *proj, BakeProj &r) {
  const float3 pv = xform4x3(p, view);
  if (pv.z <= 0.2f) return false;
  const float4 ph = xform4x4(p, proj);
  const float pw = 1.0f / (ph.w + 0.0000001f);
  const float pprojx = ph.x * pw, pprojy = ph.y * pw;
  const float focal = (float)BK_N / (2.0f * 1.0f);
  const float3 cv = cov2d(p, focal, focal, 1.0f, 1.0f, c6, view);
  const float det = cv.x * cv.z - cv.y * cv.y;
  if (det == 0.0f) return false;
  const float det_inv = 1.f / det;
  const float mid = 0.5f * (cv.x + cv.z);
  const float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
  const float l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
  const float radf = ceilf(3.f * sqrtf(fmaxf(l1, l2)));
  r.x = ndc2pix(pprojx, BK_N);
  r.y = ndc2pix(pprojy, BK_N);
  tile_rect(r.x, r.y, f2i_sat(radf), 2, 2, r.x0, r.y0, r.x1, r.y1);
  if ((r.x1 - r.x0) * (r.y1 - r.y0) == 0) return false;
  r.ca = cv.z * det_inv;
  r.cb = -cv.y * det_inv;
  r.cc = cv.x * det_inv;
  r.depth = pv.z;
  return true;
}

struct BakeArgs {
  int P;
  const float *means3D, *opacities, *cov3D;
  const int *cell;
  const float *views, *projs;  // [C][6][16]
  const int *npix;             // [24]
};

// Instances of (Gaussian, tile) for cells c0 + blockIdx.y / 6, face blockIdx.y % 6: tiles of the reference's rectangle that hold a
// needed pixel and that the ellipse {alpha >= 1/255} reaches (the binning's tight cull: never changes a pixel).  COUNT: add them to
// counts[(cell, face, tile)]; else write key (depth bits << 32 | g) at cursor[(batch cell, face, tile)]++.  One atomic per wave and
// tile; the arrival order does not matter, the sort orders by (depth, g).
template <bool COUNT>
__global__ __launch_bounds__(BK_BLOCK) void bake_bin_kernel(const BakeArgs a, int c0, uint32_t *ctr, uint64_t *bucket) {
  const int g = blockIdx.x * BK_BLOCK + threadIdx.x;
  const int cf = blockIdx.y, f = cf % 6, c = c0 + cf / 6;
  const float *view = a.views + (size_t)(c * 6 + f) * 16, *proj = a.projs + (size_t)(c * 6 + f) * 16;
  uint32_t bits = 0u;
  BakeProj r;
  if (g < a.P && a.cell[g] != c) {
    const float3 p = make_float3(a.means3D[3 * (size_t)g], a.means3D[3 * (size_t)g + 1], a.means3D[3 * (size_t)g + 2]);
    if (bake_project(p, a.cov3D + 6 * (size_t)g, view, proj, r)) {
      const float o = a.opacities[g];
      for (int ty = r.y0; ty < r.y1; ty++)
        for (int tx = r.x0; tx < r.x1; tx++) {
          const int t = ty * 2 + tx;
          if (a.npix[f * 4 + t] == 0) continue;
          const float px0 = (float)(tx * TILE), py0 = (float)(ty * TILE);
          if (ellipse_hits_rect(r.x, r.y, r.ca, r.cb, r.cc, o, px0, px0 + (float)(TILE - 1), py0, py0 + (float)(TILE - 1)))
            bits |= 1u << t;
        }
    }
  }
  const uint64_t lt = (1ull << lane_id()) - 1ull;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const uint64_t m = __ballot((bits >> t) & 1u);
    if (m == 0ull) continue;
    const int leader = __builtin_ctzll(m);
    uint32_t base = 0u;
    uint32_t *slot = &ctr[(size_t)(COUNT ? (c * 6 + f) : cf) * 4 + t];
    if ((int)lane_id() == leader) base = atomicAdd(slot, (uint32_t)__builtin_popcountll(m));
    base = __shfl(base, leader);
    if (!COUNT && ((bits >> t) & 1u))
      bucket[base + (uint32_t)__builtin_popcountll(m & lt)] = ((uint64_t)__float_as_uint(r.depth) << 32) | (uint64_t)(uint32_t)g;
  }
}

// exclusive scan of the batch's tile counts -> ranges, cursor (one workgroup)
__global__ __launch_bounds__(1024) void bake_scan_kernel(const uint32_t *counts, int n, uint2 *ranges, uint32_t *cursor,
                                                         uint32_t *big_count) {
  __shared__ uint32_t wtot[1024 / WAVE];
  __shared__ uint32_t carry_s;
  if (threadIdx.x == 0) {
    carry_s = 0u;
    *big_count = 0u;
  }
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    const uint32_t v = i < n ? counts[i] : 0u;
    const uint32_t incl_w = wave_incl_scan(v);
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == WAVE - 1) wtot[wave] = incl_w;
    __syncthreads();
    uint32_t woff = 0;
    for (int w = 0; w < wave; w++) woff += wtot[w];
    const uint32_t carry = carry_s;
    const uint32_t start = carry + woff + incl_w - v;
    if (i < n) {
      cursor[i] = start;
      ranges[i] = make_uint2(start, start + v);
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + woff + incl_w;
    __syncthreads();
  }
}

// the blend forward's step for one pixel and one list entry (rows g0 = x, y, qa, qb; g1 = qc, log2(255 o), o): the contribution
// rule of blend_common.h, with contraction on as the blend files are built
__device__ __forceinline__ void bake_blend_step(float4 g0, float4 g1, float px, float py, float &T, float &Wt, float &dbias) {
#pragma clang fp contract(fast)
  float pw;
  if (!cutoff_pre(g0, g1, px, py, dbias, pw)) return;
  const float alpha = blend_alpha(g1.z, pw);
  const bool hit = !(alpha < ALPHA_MIN);
  const float test_T = T * (1.0f - alpha);
  const bool stop = hit && test_T < T_MIN;
  const bool blend = hit && !stop;
  dbias = stop ? CUT_DONE : dbias;
  const float w = blend ? alpha * T : 0.0f;
  Wt += w;
  T = blend ? test_T : T;
}

// one wave per (batch cell, face, tile): walks the sorted list in batches of 64 (each lane projects one entry into LDS), blends the
// tile's needed pixels (up to 4 per lane) and writes 1 - weight into the batch's cube
__global__ __launch_bounds__(WAVE) void bake_blend_kernel(const BakeArgs a, int c0, const uint2 *ranges, const uint32_t *point_list,
                                                          const uint16_t *pix, float *cube) {
  __shared__ float4 s0[WAVE];
  __shared__ float4 s1[WAVE];
  const int t = blockIdx.x, cb = t / BK_TILES, ft = t % BK_TILES, f = ft / 4;
  const int c = c0 + cb;
  const int np = a.npix[ft];
  if (np == 0) return;
  const int lane = (int)threadIdx.x;
  const float *view = a.views + (size_t)(c * 6 + f) * 16, *proj = a.projs + (size_t)(c * 6 + f) * 16;
  float pxf[4], pyf[4], T[4], Wt[4], dbias[4];
  int pid[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int k = lane + s * WAVE;
    pid[s] = k < np ? (int)pix[ft * 256 + k] : -1;
    pxf[s] = (float)(pid[s] >= 0 ? pid[s] % BK_N : 0);
    pyf[s] = (float)(pid[s] >= 0 ? pid[s] / BK_N : 0);
    T[s] = 1.0f;
    Wt[s] = 0.0f;
    dbias[s] = pid[s] >= 0 ? CUT_LIVE : CUT_DONE;
  }
  const uint2 r = ranges[t];
  constexpr float L2E = 1.4426950408889634f;
  for (uint32_t base = r.x; base < r.y; base += WAVE) {
    bool live = false;
#pragma unroll
    for (int s = 0; s < 4; s++) live = live || !(dbias[s] > 0.f);
    if (__ballot(live) == 0ull) break;
    const uint32_t i = base + (uint32_t)lane;
    if (i < r.y) {
      const uint32_t g = point_list[i];
      const float3 p = make_float3(a.means3D[3 * (size_t)g], a.means3D[3 * (size_t)g + 1], a.means3D[3 * (size_t)g + 2]);
      BakeProj pr;
      const bool ok = bake_project(p, a.cov3D + 6 * (size_t)g, view, proj, pr);  // (always: the entry was binned by the same code)
      const float o = ok ? a.opacities[g] : 0.0f;
      s0[lane] = make_float4(pr.x, pr.y, (-0.5f * L2E) * pr.ca, -L2E * pr.cb);
      s1[lane] = make_float4((-0.5f * L2E) * pr.cc, __builtin_amdgcn_logf(255.0f * o), o, 0.0f);
    }
    wave_lds_sync();
    const int cnt = (int)min((uint32_t)WAVE, r.y - base);
    for (int k = 0; k < cnt; k++) {
      const float4 g0 = s0[k], g1 = s1[k];
#pragma unroll
      for (int s = 0; s < 4; s++) bake_blend_step(g0, g1, pxf[s], pyf[s], T[s], Wt[s], dbias[s]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  float *out = cube + (size_t)cb * BK_TEX + f * BK_N * BK_N;
#pragma unroll
  for (int s = 0; s < 4; s++)
    if (pid[s] >= 0) out[pid[s]] = 1.0f - Wt[s];
}

__global__ __launch_bounds__(BK_BLOCK) void bake_gather_kernel(int B, int c0, int ndir, const int *dir_texel, const float *cube,
                                                               float *vis) {
  const int i = blockIdx.x * BK_BLOCK + threadIdx.x;
  if (i >= B * ndir) return;
  const int cb = i / ndir, d = i % ndir, tx = dir_texel[d];
  vis[(size_t)(c0 + cb) * ndir + d] = (tx >= 0 && tx < BK_TEX) ? cube[(size_t)cb * BK_TEX + tx] : __builtin_nanf("");
}

struct VisWs {
  uint2 *ranges;
  uint32_t *cursor, *big_list, *big_count;
  float *cube;
  uint64_t *bucket, *keys_sorted;
  uint32_t *point_list;
};
inline VisWs vis_ws(void *ws, int B, size_t cap, size_t *end = nullptr) {
  VisWs w;
  uintptr_t p = carve_begin(ws);
  const size_t tiles = (size_t)B * BK_TILES;
  carve(p, w.ranges, tiles);
  carve(p, w.cursor, tiles);
  carve(p, w.big_list, tiles);
  carve(p, w.big_count, 4);
  carve(p, w.cube, (size_t)B * BK_TEX);
  carve(p, w.bucket, cap ? cap : 1);
  carve(p, w.keys_sorted, cap ? cap : 1);
  carve(p, w.point_list, cap ? cap : 1);
  if (end) *end = p;
  return w;
}
inline size_t vis_bytes(int B, size_t cap) {
  size_t end = 0;
  vis_ws(nullptr, B, cap, &end);
  return end + 256;
}

// ---- expand and per-frame reduction ------------------------------------------------------------------------------------
// dot as torch's (dirs * n).sum(-1): products, then summed left to right, no contraction (this file is built without it)
__global__ __launch_bounds__(BK_BLOCK) void bake_expand_kernel(int P, int ndir, const int *cell, const float *normals, const float *dirs,
                                                               const float *vis, float *occ) {
  const size_t i = (size_t)blockIdx.x * BK_BLOCK + threadIdx.x;
  if (i >= (size_t)P * ndir) return;
  const size_t p = i / ndir;
  const int d = (int)(i % ndir);
  const float dot = (dirs[3 * d] * normals[3 * p] + dirs[3 * d + 1] * normals[3 * p + 1]) + dirs[3 * d + 2] * normals[3 * p + 2];
  occ[i] = (dot > 0.f ? 1.0f : 0.0f) * vis[(size_t)cell[p] * ndir + d];
}

// one wave per Gaussian: 512 floats = two 16-byte loads per lane
__global__ __launch_bounds__(BK_BLOCK) void bake_env_reduce_kernel(int P, const float *occ, const float *env, float *out) {
  const int p = blockIdx.x * (BK_BLOCK / WAVE) + (int)threadIdx.x / WAVE, lane = (int)threadIdx.x % WAVE;
  if (p >= P) return;
  const float4 *row = reinterpret_cast<const float4 *>(occ + (size_t)p * 512);
  const float4 *e = reinterpret_cast<const float4 *>(env);
  float acc = 0.f;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float4 v = row[lane + h * WAVE], w = e[lane + h * WAVE];
    acc += fminf(fmaxf(v.x, 0.f), 1.f) * w.x + fminf(fmaxf(v.y, 0.f), 1.f) * w.y + fminf(fmaxf(v.z, 0.f), 1.f) * w.z +
           fminf(fmaxf(v.w, 0.f), 1.f) * w.w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane < 3) out[3 * (size_t)p + lane] = fminf(fmaxf(acc, 0.f), 1.f);
}

static inline unsigned blocks_of(size_t n) { return (unsigned)((n + BK_BLOCK - 1) / BK_BLOCK); }

static bool scene_ok(const gsr_bake_scene *s) {
  if (!s || s->P < 0 || s->C < 0 || s->C > BK_CELLS || s->ndir < 1 || s->ndir > BK_TEX) {
    set_error("gsr_bake: bad scene (P >= 0, 0 <= C <= 1000, 1 <= ndir <= 6144)");
    return false;
  }
  if (s->P > 0 && s->C > 0 &&
      (!s->means3D || !s->scales || !s->rotations || !s->opacities || !s->cell || !s->views || !s->projs || !s->dir_texel)) {
    set_error("gsr_bake: null input");
    return false;
  }
  if ((size_t)s->P * 6u * 4u > 0xFFFFFFFFull) {
    set_error("gsr_bake: too many Gaussians");
    return false;
  }
  return true;
}

}  // namespace gsr

using namespace gsr;

size_t gsr_bake_grid_workspace_bytes(void) {
  size_t end = 0;
  grid_ws(nullptr, &end);
  return end + 256;
}

int gsr_bake_grid(int P, const float *points, int *cell, float *centres, float *size, int *cell_idx, int *n_cells, void *workspace,
                  size_t workspace_bytes, gsr_stream_t stream_) {
  if (P < 0 || !n_cells || (P > 0 && (!points || !cell || !centres || !workspace))) {
    set_error("gsr_bake_grid: bad arguments");
    return GSR_EINVAL;
  }
  *n_cells = 0;
  if (P == 0) return GSR_OK;
  if (workspace_bytes < gsr_bake_grid_workspace_bytes()) {
    set_error("gsr_bake_grid: workspace too small");
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  char *ws = reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(workspace), 256));
  const GridWs w = grid_ws(ws);
  hipLaunchKernelGGL(bake_bbox_kernel, dim3(1), dim3(1024), 0, stream, P, points, w);
  GSR_LAUNCH_CHECK(stream, 0);
  hipLaunchKernelGGL(bake_cell_kernel, dim3(blocks_of(P)), dim3(BK_BLOCK), 0, stream, P, points, w, cell);
  GSR_LAUNCH_CHECK(stream, 0);
  hipLaunchKernelGGL(bake_compact_kernel, dim3(1), dim3(1024), 0, stream, w, centres, size, cell_idx);
  GSR_LAUNCH_CHECK(stream, 0);
  hipLaunchKernelGGL(bake_remap_kernel, dim3(blocks_of(P)), dim3(BK_BLOCK), 0, stream, P, w, cell);
  GSR_LAUNCH_CHECK(stream, 0);
  uint32_t count = 0;  // the one host read of the grid: the cell count sizes everything that follows
  GSR_HIP(hipMemcpyAsync(&count, w.count, sizeof(count), hipMemcpyDeviceToHost, stream));
  GSR_HIP(hipStreamSynchronize(stream));
  *n_cells = (int)count;
  return GSR_OK;
}

size_t gsr_bake_plan_bytes(int P, int C) {
  size_t end = 0;
  plan_ws(nullptr, P < 0 ? 0 : P, C < 0 ? 0 : C, &end);
  return end + 256;
}

int gsr_bake_plan(const gsr_bake_scene *s, void *plan, size_t plan_bytes, unsigned long long *instances, gsr_stream_t stream_) {
  if (!scene_ok(s)) return GSR_EINVAL;
  if (!plan || !instances || plan_bytes < gsr_bake_plan_bytes(s->P, s->C)) {
    set_error("gsr_bake_plan: null output or plan buffer too small");
    return GSR_EINVAL;
  }
  instances[0] = instances[1] = 0ull;
  if (s->P == 0 || s->C == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  char *base = reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(plan), 256));
  const PlanWs w = plan_ws(base, s->P, s->C);
  hipLaunchKernelGGL(bake_cov3d_kernel, dim3(blocks_of(s->P)), dim3(BK_BLOCK), 0, stream, s->P, s->scales, s->rotations, w.cov3D);
  GSR_LAUNCH_CHECK(stream, 0);
  hipLaunchKernelGGL(bake_pixels_kernel, dim3(1), dim3(1024), 0, stream, s->dir_texel, s->ndir, w);
  GSR_LAUNCH_CHECK(stream, 0);
  GSR_HIP(zero_async(w.counts, (size_t)s->C * BK_TILES * sizeof(uint32_t), stream));
  const BakeArgs a = {s->P, s->means3D, s->opacities, w.cov3D, s->cell, s->views, s->projs, w.npix};
  hipLaunchKernelGGL(bake_bin_kernel<true>, dim3(blocks_of(s->P), (unsigned)s->C * 6), dim3(BK_BLOCK), 0, stream, a, 0, w.counts,
                     (uint64_t *)nullptr);
  GSR_LAUNCH_CHECK(stream, 0);
  std::vector<uint32_t> counts((size_t)s->C * BK_TILES);
  GSR_HIP(hipMemcpyAsync(counts.data(), w.counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  GSR_HIP(hipStreamSynchronize(stream));
  for (int c = 0; c < s->C; c++) {
    unsigned long long n = 0;
    for (int k = 0; k < BK_TILES; k++) n += counts[(size_t)c * BK_TILES + k];
    instances[0] += n;
    if (n > instances[1]) instances[1] = n;
  }
  return GSR_OK;
}

size_t gsr_bake_visibility_workspace_bytes(int C, size_t capacity) { return vis_bytes(C < 1 ? 1 : C, capacity); }

int gsr_bake_visibility(const gsr_bake_scene *s, const void *plan, float *vis, void *workspace, size_t workspace_bytes,
                        unsigned long long *stats, gsr_stream_t stream_) {
  if (!scene_ok(s)) return GSR_EINVAL;
  if (s->P == 0 || s->C == 0) return GSR_OK;
  if (!plan || !vis || !workspace) {
    set_error("gsr_bake_visibility: null plan, output or workspace");
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const Options opt = options_for(stream);
  const int bmax = opt.bake_batch_cells > 0 ? (opt.bake_batch_cells < s->C ? opt.bake_batch_cells : s->C) : s->C;
  // capacity: what the workspace holds beside the per-batch tables (20 bytes per instance)
  const size_t fixed = vis_bytes(bmax, 0);
  size_t cap = workspace_bytes > fixed ? (workspace_bytes - fixed) / 20u + 64u : 0u;
  while (cap > 0 && vis_bytes(bmax, cap) > workspace_bytes) cap--;  // (the three arrays' alignment padding)
  char *pbase = reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(plan), 256));
  const PlanWs pw = plan_ws(pbase, s->P, s->C);
  char *wbase = reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(workspace), 256));
  const VisWs w = vis_ws(wbase, bmax, cap);
  // the plan's counts, read once more (the plan call may have been on another stream); batches of consecutive cells
  std::vector<uint32_t> counts((size_t)s->C * BK_TILES);
  GSR_HIP(hipMemcpyAsync(counts.data(), pw.counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  GSR_HIP(hipStreamSynchronize(stream));
  std::vector<size_t> per_cell(s->C, 0);
  for (int c = 0; c < s->C; c++)
    for (int k = 0; k < BK_TILES; k++) per_cell[c] += counts[(size_t)c * BK_TILES + k];
  for (int c = 0; c < s->C; c++)
    if (per_cell[c] > cap || per_cell[c] > 0xFFFFFFFFull) {
      set_error("gsr_bake_visibility: cell %d has %zu instances, the workspace holds %zu", c, per_cell[c], cap);
      return GSR_EINVAL;
    }
  const BakeArgs a = {s->P, s->means3D, s->opacities, pw.cov3D, s->cell, s->views, s->projs, pw.npix};
  unsigned long long batches = 0, peak = 0, total = 0;
  for (int c0 = 0; c0 < s->C;) {
    int B = 0;
    size_t n = 0;
    while (c0 + B < s->C && B < bmax && n + per_cell[c0 + B] <= cap) n += per_cell[c0 + B++];
    const size_t tiles = (size_t)B * BK_TILES;
    hipLaunchKernelGGL(bake_scan_kernel, dim3(1), dim3(1024), 0, stream, pw.counts + (size_t)c0 * BK_TILES, (int)tiles, w.ranges,
                       w.cursor, w.big_count);
    GSR_LAUNCH_CHECK(stream, 0);
    if (n > 0) {
      hipLaunchKernelGGL(bake_bin_kernel<false>, dim3(blocks_of(s->P), (unsigned)B * 6), dim3(BK_BLOCK), 0, stream, a, c0, w.cursor,
                         w.bucket);
      GSR_LAUNCH_CHECK(stream, 0);
      const int rc = bucket_sort_lists(w.ranges, w.bucket, w.point_list, w.keys_sorted, w.big_list, w.big_count, tiles, stream);
      if (rc != GSR_OK) return rc;
    }
    hipLaunchKernelGGL(bake_blend_kernel, dim3((unsigned)tiles), dim3(WAVE), 0, stream, a, c0, w.ranges, w.point_list, pw.pix, w.cube);
    GSR_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(bake_gather_kernel, dim3(blocks_of((size_t)B * s->ndir)), dim3(BK_BLOCK), 0, stream, B, c0, s->ndir, s->dir_texel,
                       w.cube, vis);
    GSR_LAUNCH_CHECK(stream, 0);
    batches++;
    total += n;
    if (n > peak) peak = n;
    c0 += B;
  }
  if (stats) {
    stats[0] = total;
    stats[1] = peak;
    stats[2] = batches;
    stats[3] = cap;
  }
  return GSR_OK;
}

int gsr_bake_expand(int P, int ndir, const int *cell, const float *normals, const float *dirs, const float *vis, float *occ,
                    gsr_stream_t stream_) {
  if (P < 0 || ndir < 1 || (P > 0 && (!cell || !normals || !dirs || !vis || !occ))) {
    set_error("gsr_bake_expand: bad arguments");
    return GSR_EINVAL;
  }
  if (P == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(bake_expand_kernel, dim3(blocks_of((size_t)P * ndir)), dim3(BK_BLOCK), 0, stream, P, ndir, cell, normals, dirs, vis,
                     occ);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_bake_env_reduce(int P, const float *occ, const float *env, float *out, gsr_stream_t stream_) {
  if (P < 0 || (P > 0 && (!occ || !env || !out)) || (reinterpret_cast<uintptr_t>(occ) | reinterpret_cast<uintptr_t>(env)) % 16) {
    set_error("gsr_bake_env_reduce: bad arguments (16-byte aligned occ [P][512] and env [512])");
    return GSR_EINVAL;
  }
  if (P == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(bake_env_reduce_kernel, dim3((unsigned)((P + BK_BLOCK / WAVE - 1) / (BK_BLOCK / WAVE))), dim3(BK_BLOCK), 0, stream, P,
                     occ, env, out);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}
