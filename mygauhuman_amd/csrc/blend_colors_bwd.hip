// blend_colors_bwd.hip -- the colour columns of the blend backward, alone (gsr_rasterize_backward_colors).
//
// Once the geometry is frozen (the reference's PBR phase: scene/gaussian_model.py:296-306) the only per-Gaussian gradient anybody
// consumes is   dL/dcolour_k[c] = sum over pixels of  w_k(pixel) . dL/dimage[c](pixel),   w_k = T_k alpha_k,
// and w_k is exactly what the FORWARD forms, front to back.  So this kernel is a replay of blend_forward_kernel (blend_fwd.hip): the
// same quadrant waves on the same visiting slots, the same 64-entry batches culled and compacted into LDS, and the same contribution
// rule, which both take from blend_common.h -- hence the forward's contributors and the forward's weights.
// There is no division of T, no dL/dalpha recursion, no conic or mean moment, and GeomState::grad_rows is never touched.  Lists are
// walked whole from the slot of their first segment, as the forward walks them (the forward's checkpoints are not read).
//
// Reduction.  A survivor that blends into at least one pixel of the quadrant is STAGED: its 64 weights go to a row of an LDS plane
// (CB_STAGE rows of 64 + 4 padding floats), its Gaussian id next to it.  Every CB_STAGE staged survivors (and once at the end of
// the walk) the wave flushes:
//   * lane (k = lane % 16, j = lane / 16) forms, for every live gradient image, the three sums of row k's weights times the image's
//     channels over the pixels 16 j .. 16 j + 15 -- weights and gradients read as 16-byte LDS words (the weight rows conflict-free
//     through the padding, the gradient words broadcast) -- and two cross-lane adds join the four j groups;
//   * the sums are parked in a [CB_STAGE][21] result plane (columns 0..17 = the extra channels, 18..20 = the main colour) and
//     added to the outputs with lane -> (row = lane / 21, column = lane % 21): a Gaussian's live columns are CONTIGUOUS lanes of
//     one atomic wave-instruction, three Gaussians per instruction (72-byte rows of dL_dextra, 12-byte rows of dL_dcolor).
// A null gradient image has no plane in LDS, no sums and no atomics: its columns keep the zeros the entry point wrote.
#include "blend_common.h"

namespace gsr {

constexpr int CB_STAGE = 16;         // staged survivors per flush (lane = 16 rows x 4 pixel groups)
constexpr int CB_WS = WAVE + 4;      // floats per staged weight row (padding: the 16 rows' 16-byte reads hit different banks)
constexpr int CB_COLS = CE_MAX + 3;  // result columns: the extra channels, then the main colour
constexpr int CB_RS = 24;            // floats per result row
constexpr int CB_WPG = 4;            // the four quadrant waves of a tile share a workgroup (one L1 for the tile's records); no barriers

__global__ __launch_bounds__(WAVE * CB_WPG) void blend_colors_backward_kernel(const BlendColorsBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_g_dyn[];  // [wave][3 n_img][64] gradient of the wave's pixels, live images only
  __shared__ float4 s0_all[CB_WPG * WAVE];  // x, y, qa, qb
  __shared__ float4 s1_all[CB_WPG * WAVE];  // qc, log2(255 opacity) | Gaussian id (bits), opacity
  __shared__ __attribute__((aligned(16))) float s_w_all[CB_WPG * CB_STAGE * CB_WS];
  __shared__ float s_res_all[CB_WPG * CB_STAGE * CB_RS];
  __shared__ uint32_t s_id_all[CB_WPG * CB_STAGE];
  const uint32_t wv = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  float *s_g = s_g_dyn + (size_t)wv * (size_t)(3 * a.n_img) * WAVE;
  float4 *s0 = s0_all + wv * WAVE, *s1 = s1_all + wv * WAVE;
  float *s_w = s_w_all + wv * CB_STAGE * CB_WS, *s_res = s_res_all + wv * CB_STAGE * CB_RS;
  uint32_t *s_id = s_id_all + wv * CB_STAGE;

  // one workgroup per visiting slot: a list is walked whole from the slot of its first segment
  const int omode = tile_order_mode(a.order);
  const uint32_t n_slots = tile_slots_of(a.order, a.grid_x, a.grid_y, omode);
  uint32_t slot = blockIdx.x;
  if (!omode) slot = slot < n_slots ? xcd_remap(slot, n_slots) : n_slots;
  const uint32_t entry = tile_of_slot(a.order, omode, slot, n_slots);
  if (entry == ORDER_NO_TILE || order_entry_seg(entry) != 0u) return;  // (workgroup-uniform)
  const uint32_t tile = order_entry_tile(entry), part = wv;
  const int tx = tile % a.grid_x, ty = tile / a.grid_x;
  const uint2 range = a.ranges[tile];
  const int n = (int)(range.y - range.x);
  if (n <= 0) return;
  list_priority(a.order, n, a.list_prio);

  const int px = tx * TILE + (int)(part & 1u) * 8 + (int)(lane & 7u);
  const int py = ty * TILE + (int)(part >> 1) * 8 + (int)(lane >> 3);
  const float pxf = (float)px, pyf = (float)py;
  const bool inside = px < a.W && py < a.H;
  float dbias = inside ? CUT_LIVE : CUT_DONE;
  float T = 1.0f;
  const float rx0 = (float)(tx * TILE + (int)(part & 1u) * 8), rx1 = rx0 + 7.f;
  const float ry0 = (float)(ty * TILE + (int)(part >> 1) * 8), ry1 = ry0 + 7.f;
  const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));

  // the wave's pixels of every live gradient image (a pixel outside the image contributes nothing: its weight is always zero too)
  {
    const size_t plane = (size_t)a.H * a.W;
    const size_t pix = (size_t)py * a.W + px;
#pragma unroll
    for (int t = 0; t < CB_IMAGES; t++) {  // (constant bounds: the pointers stay kernel arguments, no private copy of the array)
      if (t < a.n_img) {
        const float *g = a.g_img[t];
#pragma unroll
        for (int c = 0; c < 3; c++) s_g[(t * 3 + c) * WAVE + (int)lane] = inside ? g[(size_t)c * plane + pix] : 0.f;
      }
    }
  }

  // ---- flush: the staged rows' sums and their atomics (see the header)
  auto flush = [&](int cnt) {
    wave_lds_sync();  // the staged weights, ids (and, the first time, the gradient planes) are in LDS
    const int k = (int)(lane & 15u), j = (int)(lane >> 4);
    float4 w4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w4[i] = *reinterpret_cast<const float4 *>(&s_w[k * CB_WS + j * 16 + i * 4]);
    for (int t = 0; t < a.n_img; t++) {
      float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
      const float *g = s_g + t * 3 * WAVE + j * 16;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float4 g0 = *reinterpret_cast<const float4 *>(g + i * 4);
        const float4 g1 = *reinterpret_cast<const float4 *>(g + WAVE + i * 4);
        const float4 g2 = *reinterpret_cast<const float4 *>(g + 2 * WAVE + i * 4);
        acc0 += w4[i].x * g0.x + w4[i].y * g0.y + w4[i].z * g0.z + w4[i].w * g0.w;
        acc1 += w4[i].x * g1.x + w4[i].y * g1.y + w4[i].z * g1.z + w4[i].w * g1.w;
        acc2 += w4[i].x * g2.x + w4[i].y * g2.y + w4[i].z * g2.z + w4[i].w * g2.w;
      }
      acc0 += __shfl_xor(acc0, 16, WAVE);
      acc1 += __shfl_xor(acc1, 16, WAVE);
      acc2 += __shfl_xor(acc2, 16, WAVE);
      acc0 += __shfl_xor(acc0, 32, WAVE);
      acc1 += __shfl_xor(acc1, 32, WAVE);
      acc2 += __shfl_xor(acc2, 32, WAVE);
      if (j < 3) s_res[k * CB_RS + (int)((a.col0 >> (5 * t)) & 31u) + j] = j == 0 ? acc0 : (j == 1 ? acc1 : acc2);
    }
    wave_lds_sync();
    const int rr = (int)lane / CB_COLS, col = (int)lane % CB_COLS;  // (lane 63: row 3, never used)
    const bool col_live = rr < 3 && ((a.col_mask >> col) & 1u) != 0u;
    for (int r0 = 0; r0 < cnt; r0 += 3) {
      const int row = r0 + rr;
      if (col_live && row < cnt) {
        const uint32_t id = s_id[row];
        float *dst = col < CE_MAX ? a.dL_dextra + (size_t)id * CE_MAX + col : a.dL_dcolor + (size_t)id * 3 + (col - CE_MAX);
        atomicAdd(dst, s_res[row * CB_RS + col]);
      }
    }
    wave_lds_sync();  // the next staged rows are written behind these reads
  };

  // ---- the forward's walk: two-stage prefetch of the list, cull + compaction per batch of 64 entries
  uint32_t id_a = 0, id_cur = 0;
  float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
  if ((int)lane < n) {
    id_cur = a.point_list[range.x + lane];
    const float4 *src = reinterpret_cast<const float4 *>(a.recs + id_cur);
    p0 = src[0];
    p1 = src[1];
    p2 = src[2];
  }
  if ((int)lane + WAVE < n) id_a = a.point_list[range.x + lane + WAVE];
  int nst = 0;  // staged rows (wave-uniform)
  for (int base = 0; base < n; base += WAVE) {
    if (__ballot(!(dbias > 0.f)) == 0ull) break;  // every pixel of the quadrant is saturated (or outside the image)
    const int idx = base + (int)lane;
    const float4 r0 = p0, r1c = p1, r2 = p2;
    const uint32_t id = id_cur;
    bool keep = false;
    if (idx < n) keep = (r0.x + r2.z >= rx0) && (r0.x - r2.z <= rx1) && (r0.y + r2.w >= ry0) && (r0.y - r2.w <= ry1);
    float4 r1 = make_float4(0, 0, 0, 0);
    float l255 = 0.f;
    if (keep) {
      r1 = r1c;
      l255 = __builtin_amdgcn_logf(255.0f * r1.y);
      keep = ellipse_hits_rect_fast(r0.x, r0.y, r0.z, r0.w, r1.x, l255, rx0, rx1, ry0, ry1);
    }
    const uint64_t kmask = __ballot(keep);
    const int cnt = __builtin_popcountll(kmask);
    if (keep) {
      const int sl = __builtin_popcountll(kmask & lt);
      constexpr float L2E = 1.4426950408889634f;
      s0[sl] = make_float4(r0.x, r0.y, (-0.5f * L2E) * r0.z, -L2E * r0.w);
      s1[sl] = make_float4((-0.5f * L2E) * r1.x, l255, __uint_as_float(id), r1.y);
    }
    id_cur = id_a;
    if (idx + WAVE < n) {
      const float4 *src = reinterpret_cast<const float4 *>(a.recs + id_a);
      p0 = src[0];
      p1 = src[1];
      p2 = src[2];
    }
    if (idx + 2 * WAVE < n) id_a = a.point_list[range.x + idx + 2 * WAVE];
    wave_lds_sync();

    // the rows of survivor k + 1 are requested before the arithmetic of survivor k (two register sets used in turn, as the forward)
    struct Row {
      float4 g0, g1;
    };
    auto fetch = [&](Row &r, int k) {  // (a row beyond the last survivor is stale LDS: read, never used)
      const int kk = min(k, WAVE - 1);
      r.g0 = s0[kk];
      r.g1 = s1[kk];
    };
    auto blend_one = [&](const Row &r) {
      float pw;
      const bool pre = cutoff_pre(r.g0, r.g1, pxf, pyf, dbias, pw);
      if (__ballot(pre) != 0ull) {
        const float alpha = blend_alpha(r.g1.w, pw);
        const bool hit = pre && !(alpha < ALPHA_MIN);
        const float test_T = T * (1.0f - alpha);
        const bool stop = hit && test_T < T_MIN;
        const bool blend = hit && !stop;
        dbias = stop ? CUT_DONE : dbias;
        const float w = blend ? alpha * T : 0.0f;
        T = blend ? test_T : T;
        if (__ballot(blend) != 0ull) {  // (wave-uniform) somebody blended it: stage the row
          s_w[nst * CB_WS + (int)lane] = w;
          if (lane == 0) s_id[nst] = __float_as_uint(r.g1.z);
          if (++nst == CB_STAGE) {
            flush(CB_STAGE);
            nst = 0;
          }
        }
      }
    };
    Row A, B;
    fetch(A, 0);
    int k = 0;
    for (; k + 1 < cnt; k += 2) {
      fetch(B, k + 1);
      blend_one(A);
      fetch(A, k + 2);
      blend_one(B);
    }
    if (k < cnt) blend_one(A);
    __builtin_amdgcn_wave_barrier();  // keep the next batch's LDS writes behind this batch's reads
  }
  if (nst > 0) flush(nst);
}

int launch_blend_colors_backward(const BlendColorsBwdArgs &a, hipStream_t stream) {
  const unsigned tiles = (unsigned)(a.grid_x * a.grid_y);
  if (tiles == 0 || a.n_img == 0) return GSR_OK;
  if (a.n_img < 0 || a.n_img > CB_IMAGES || !a.order) {
    set_error("colour-only blend backward: bad launch arguments");
    return GSR_EINVAL;
  }
  const unsigned slots = tile_slots_max(a.grid_x, a.grid_y);
  const size_t dyn = (size_t)CB_WPG * 3u * (size_t)a.n_img * WAVE * sizeof(float);  // <= 21.5 KB
  hipLaunchKernelGGL(blend_colors_backward_kernel, dim3(slots), dim3(WAVE * CB_WPG), dyn, stream, a);
  return GSR_OK;
}

}  // namespace gsr
