// blend_common.h -- what the blend kernels must decide alike for a frame's images and gradients to agree (blend_fwd.hip,
// blend_bwd.hip, blend_colors_bwd.hip; bake.hip takes the contribution rule): which work a workgroup takes, and when a list
// entry contributes to a pixel.
#pragma once
#include "gsr_common.h"

namespace gsr {

// bijective XCD-aware remap: consecutive work items (which share Gaussians) land on the same XCD / L2
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t n) {
  const uint32_t q = n / 8, r = n % 8, xcd = bid % 8, k = bid / 8;
  const uint32_t start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + k;
}

// hand-over of LDS between the lanes of ONE wave: what the lanes wrote before it is visible to every lane's reads after it
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Four one-wave workgroups per visiting slot, one per quadrant (the backward kernels): workgroup blockIdx.x -> the order entry of
// its slot (ORDER_NO_TILE: nothing to do) and its quadrant `part`, from the frame's tile_order_mode and tile_slots_of.  Only the
// natural order is remapped: an ordered frame keeps slot % 8 = workgroup % 8.  What a caller does with an entry of a non-zero
// segment is its own policy: walk it, or return.
__device__ __forceinline__ uint32_t entry_of_quadrant_workgroup(const uint32_t *order, int omode, uint32_t n_slots, uint32_t &part) {
  const uint32_t item = omode ? ordered_item4(blockIdx.x, n_slots) : (blockIdx.x < n_slots * 4u ? xcd_remap(blockIdx.x, n_slots * 4u) : n_slots * 4u);
  const uint32_t entry = tile_of_slot(order, omode, item / 4u, n_slots);
  part = item % 4u;
  return entry;
}

// ---- the contribution rule (the reference's: skip power > 0, alpha = min(0.99, o exp(power)), skip alpha < 1/255, stop without
// blending when T (1 - alpha) < 1e-4).  The helpers keep contraction on in a file built without it (bake.hip): one rounding everywhere.
constexpr float ALPHA_MAX = 0.99f;
constexpr float ALPHA_MIN = 1.0f / 255.0f;  // a smaller alpha is skipped
constexpr float T_MIN = 0.0001f;            // a pixel stops, without blending, at the entry that would take its T below this
// The cut-off test compares against a per-pixel threshold ("dbias"): CUT_LIVE while the pixel is live, CUT_DONE once it is
// saturated or if it lies outside the image -- "done" folded into the test instead of a loop-carried lane mask.
constexpr float CUT_LIVE = -0.02f;  // log2(255 o) + power log2(e) >= 0 is necessary for alpha >= 1/255; 0.02 safety margin
constexpr float CUT_DONE = 1e30f;

// A survivor's cut-off rows: g0 = x, y, qa, qb;  g1 = qc, log2(255 opacity), ...   (qa = -conic_a log2(e)/2, qb = -conic_b log2(e),
// qc = -conic_c log2(e)/2).  Exponent in base 2 at pixel (px, py): pw = power * log2(e) = dx (qa dx + qb dy) + qc dy dy.
// Cheap necessary condition for "this entry reaches alpha >= 1/255 at the pixel"; hands back the exponent.
__device__ __forceinline__ bool cutoff_pre(const float4 &g0, const float4 &g1, float px, float py, float dbias, float &pw) {
#pragma clang fp contract(fast)
  const float dx = g0.x - px, dy = g0.y - py;
  pw = dx * (g0.z * dx + g0.w * dy) + (g1.x * dy) * dy;
  return !(pw > 0.0f) && ((pw + g1.y) >= dbias);
}
// The backward kernels' form: they replay a list for pixels whose end is known, so the threshold is the constant margin and an
// entry counts only in FRONT of the pixel's last contributor (front position fpos < lastc = n_contrib).  (The position test
// comes first and the exponent is written out again: the compiler orders the conditions and contracts the sum as it meets them.)
__device__ __forceinline__ bool cutoff_pre_replay(const float4 &g0, const float4 &g1, float px, float py, int fpos, int lastc, float &pw) {
#pragma clang fp contract(fast)
  const float dx = g0.x - px, dy = g0.y - py;
  pw = dx * (g0.z * dx + g0.w * dy) + (g1.x * dy) * dy;
  return (fpos < lastc) && !(pw > 0.0f) && ((pw + g1.y) >= CUT_LIVE);
}
// alpha of an entry that passed the cut-off test; G = exp(power), which the backward kernels need by itself
__device__ __forceinline__ float blend_alpha(float opacity, float pw, float &G) {
  G = __builtin_amdgcn_exp2f(pw);
  return fminf(ALPHA_MAX, opacity * G);
}
__device__ __forceinline__ float blend_alpha(float opacity, float pw) {
  float G;
  return blend_alpha(opacity, pw, G);
}

}  // namespace gsr
