// densify.hip -- the decisions and the new rows of a densification step (scene/gaussian_model.py:514-708,740-762).
//
// rows.hip moves the rows of a densify / prune operation in one launch; what surrounded it was still chains of torch ops:
// kl_div over gathered [P,3,3] temporaries (~40 launches), the selections (elementwise chains), the row plans (torch.nonzero:
// a host synchronisation each) and the recomputed rows (split children, displaced KL clones, merged means) written into the
// result after the gather.  The four entry points here replace them:
//   gsr_kl_pairs        KL( N_a || N_b ) of every k-NN pair, in the frame of b: 20 floats in, 1 out per Gaussian
//   gsr_densify_select  the clone / split / merge selections as uint8 flags, the comparisons torch makes on the same float32 inputs
//   gsr_densify_plan    flags -> row plan by a stable device-side compaction (count, scan, scatter: no atomics, no host read)
//   gsr_build_rows      gsr_gather_rows + the arithmetic of the new rows
// All of it is memory-bound streaming: 256-thread blocks, one thread per Gaussian or per row element, rows read as they lie.
#include <math.h>

#include "gsr_common.h"

namespace gsr {

constexpr int DN_BLOCK = 256;
constexpr int DN_NEW = 1 << 30;  // the "new Gaussian" bit of a plan entry (ROW_NEW_FLAG of rows.hip)
inline int dn_blocks(int n) { return (n + DN_BLOCK - 1) / DN_BLOCK; }
inline int dn_grid(int n) { return dn_blocks(n) < 8192 ? dn_blocks(n) : 8192; }  // grid-stride beyond
__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// R of the normalised quaternion (w, x, y, z), row-major, the expressions of covariance.build_rotation
__device__ __forceinline__ void quat_rotation(const float *q_, float R[9]) {
  const float a = q_[0], b = q_[1], c = q_[2], d = q_[3];
  const float n = sqrtf(a * a + b * b + c * c + d * d);
  const float w = a / n, x = b / n, y = c / n, z = d / n;
  R[0] = 1.f - 2.f * (y * y + z * z);
  R[1] = 2.f * (x * y - w * z);
  R[2] = 2.f * (x * z + w * y);
  R[3] = 2.f * (x * y + w * z);
  R[4] = 1.f - 2.f * (x * x + z * z);
  R[5] = 2.f * (y * z - w * x);
  R[6] = 2.f * (x * z - w * y);
  R[7] = 2.f * (y * z + w * x);
  R[8] = 1.f - 2.f * (x * x + y * y);
}

// ---------------------------------------------------------------- KL of the pairs
// 1/2 [ tr(S_b^-1 S_a) + d^T S_b^-1 d + ln(det S_b / det S_a) - 3 ] with M = R_b^T R_a:
//   tr = sum_ij M_ij^2 s_aj^2 / s_bi^2,   maha = sum_i (R_b^T d)_i^2 / s_bi^2,   ln det = 2 sum (l_b - l_a)
// Every summand of the first two terms is >= 0 (no cancellation), and no product of scales is formed.
__global__ __launch_bounds__(DN_BLOCK) void kl_pairs_kernel(int P, const float *__restrict__ xyz, const float *__restrict__ rot,
                                                            const float *__restrict__ lscale, const int *__restrict__ pairs,
                                                            float *__restrict__ kl) {
  for (int i = blockIdx.x * DN_BLOCK + threadIdx.x; i < P; i += gridDim.x * DN_BLOCK) {
    const int a = pairs[2 * i], b = pairs[2 * i + 1];
    if ((unsigned)a >= (unsigned)P || (unsigned)b >= (unsigned)P) {
      kl[i] = quiet_nan();
      continue;
    }
    float Ra[9], Rb[9];
    quat_rotation(rot + 4 * (size_t)a, Ra);
    quat_rotation(rot + 4 * (size_t)b, Rb);
    float va[3], wb[3], d[3], logdet = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float la = lscale[3 * (size_t)a + k], lb = lscale[3 * (size_t)b + k];
      const float sa = expf(la), rb = 1.f / expf(lb);
      va[k] = sa * sa;
      wb[k] = rb * rb;
      logdet += lb - la;
      d[k] = xyz[3 * (size_t)b + k] - xyz[3 * (size_t)a + k];
    }
    float trace = 0.f, maha = 0.f;
#pragma unroll
    for (int r = 0; r < 3; r++) {  // row r of M = column r of R_b against the columns of R_a
      float row = 0.f;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float m = Rb[r] * Ra[c] + Rb[3 + r] * Ra[3 + c] + Rb[6 + r] * Ra[6 + c];
        row += m * m * va[c];
      }
      const float t = Rb[r] * d[0] + Rb[3 + r] * d[1] + Rb[6 + r] * d[2];
      trace += row * wb[r];
      maha += t * t * wb[r];
    }
    kl[i] = 0.5f * (trace + maha + 2.f * logdet - 3.f);
  }
}

// ---------------------------------------------------------------- selections
// mode 0 clone: |g_i| >= thr, max s_i <= size      1 split: padded g_i >= thr, max s_i > size      2 merge: padded g_i >= thr,
// max s_i <= size; with kl: and kl_i > kl_thr (clone, split) or kl_i < kl_thr (merge).  NaN compares false, as in torch (whose
// max() carries a NaN, so a NaN scale fails both size tests).
__global__ __launch_bounds__(DN_BLOCK) void densify_select_kernel(int P, int mode, const float *__restrict__ grads, int n_grads,
                                                                  const float *__restrict__ scaling, const float *__restrict__ kl,
                                                                  float grad_thr, float size_thr, float kl_thr,
                                                                  uint8_t *__restrict__ flags) {
  for (int i = blockIdx.x * DN_BLOCK + threadIdx.x; i < P; i += gridDim.x * DN_BLOCK) {
    const float g = i < n_grads ? grads[i] : 0.f;
    bool sel = (mode == GSR_DENSIFY_CLONE ? fabsf(g) : g) >= grad_thr;
    const float s0 = scaling[3 * (size_t)i], s1 = scaling[3 * (size_t)i + 1], s2 = scaling[3 * (size_t)i + 2];
    const float m = fmaxf(s0, fmaxf(s1, s2));
    const bool ordered = s0 == s0 && s1 == s1 && s2 == s2;
    sel = sel && ordered && (mode == GSR_DENSIFY_SPLIT ? m > size_thr : m <= size_thr);
    if (kl) sel = sel && (mode == GSR_DENSIFY_MERGE ? kl[i] < kl_thr : kl[i] > kl_thr);
    flags[i] = sel ? 1 : 0;
  }
}

// ---------------------------------------------------------------- row plans
// A plan is a "keep" part (source rows in order) followed by `copies` blocks of the flagged rows marked new:
//   prune  keep = flag 0, copies 0          clone  keep = every row, copies 1
//   split  keep = flag 0, copies N          merge  keep = neither flagged nor the partner of a flagged row, copies 1 (of pairs[i][0])
// Three launches over blocks of 256 rows: count (keep, flagged) per block, exclusive scan of the block counts by one workgroup
// (which also leaves the header), scatter with the block-local scan.  Positions never depend on the order of execution.
struct PlanArgs {
  int P, kind, copies;
  const uint8_t *flags;
  const int *pairs;
  uint8_t *gone;  // merge: [P] zeroed, 1 = the row leaves the set
  int *block_keep, *block_sel;  // [blocks]
  int *plan, *header;
};

__device__ __forceinline__ bool plan_keeps(const PlanArgs &a, int i) {
  if (a.kind == GSR_PLAN_CLONE) return true;
  if (a.kind == GSR_PLAN_MERGE) return a.gone[i] == 0;
  return a.flags[i] == 0;
}

// every flagged i removes itself and its partner; all writers store the same value, so the result does not depend on their order
__global__ __launch_bounds__(DN_BLOCK) void plan_gone_kernel(const PlanArgs a) {
  for (int i = blockIdx.x * DN_BLOCK + threadIdx.x; i < a.P; i += gridDim.x * DN_BLOCK) {
    if (a.flags[i] == 0) continue;
    a.gone[i] = 1;
    const int b = a.pairs[2 * i + 1];
    if ((unsigned)b < (unsigned)a.P) a.gone[b] = 1;
  }
}

// block-wide exclusive scan of two counters (wave scans + one LDS row per wave); returns the block totals through tot_*
__device__ __forceinline__ void block_excl_scan2(uint32_t k, uint32_t s, uint32_t &ek, uint32_t &es, uint32_t &tot_k, uint32_t &tot_s) {
  __shared__ uint32_t w_k[DN_BLOCK / WAVE], w_s[DN_BLOCK / WAVE];
  const uint32_t ik = wave_incl_scan(k), is = wave_incl_scan(s);
  const int wave = threadIdx.x / WAVE;
  __syncthreads();  // (the rows may still be read by a previous call)
  if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
    w_k[wave] = ik;
    w_s[wave] = is;
  }
  __syncthreads();
  ek = ik - k;
  es = is - s;
  tot_k = tot_s = 0;
#pragma unroll
  for (int w = 0; w < DN_BLOCK / WAVE; w++) {
    if (w < wave) {
      ek += w_k[w];
      es += w_s[w];
    }
    tot_k += w_k[w];
    tot_s += w_s[w];
  }
}

__global__ __launch_bounds__(DN_BLOCK) void plan_count_kernel(const PlanArgs a) {
  const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < a.P;
  uint32_t ek, es, tk, ts;
  block_excl_scan2(in && plan_keeps(a, i), in && a.flags[i] != 0, ek, es, tk, ts);
  if (threadIdx.x == 0) {
    a.block_keep[blockIdx.x] = (int)tk;
    a.block_sel[blockIdx.x] = (int)ts;
  }
}

__global__ __launch_bounds__(DN_BLOCK) void plan_scan_kernel(const PlanArgs a, int blocks) {
  uint32_t base_k = 0, base_s = 0;
  for (int first = 0; first < blocks; first += DN_BLOCK) {
    const int j = first + threadIdx.x;
    const uint32_t k = j < blocks ? (uint32_t)a.block_keep[j] : 0u, s = j < blocks ? (uint32_t)a.block_sel[j] : 0u;
    uint32_t ek, es, tk, ts;
    block_excl_scan2(k, s, ek, es, tk, ts);
    if (j < blocks) {
      a.block_keep[j] = (int)(base_k + ek);
      a.block_sel[j] = (int)(base_s + es);
    }
    base_k += tk;
    base_s += ts;
  }
  if (threadIdx.x == 0) {
    const int n_new = a.copies * (int)base_s;
    a.header[0] = (int)base_k;
    a.header[1] = n_new;
    a.header[2] = (int)base_k + n_new;
    a.header[3] = 0;
  }
}

__global__ __launch_bounds__(DN_BLOCK) void plan_scatter_kernel(const PlanArgs a) {
  const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < a.P;
  const bool keep = in && plan_keeps(a, i), sel = in && a.flags[i] != 0;
  uint32_t ek, es, tk, ts;
  block_excl_scan2(keep, sel, ek, es, tk, ts);
  if (keep) a.plan[a.block_keep[blockIdx.x] + (int)ek] = i;
  if (sel) {
    const int n_keep = a.header[0], n_sel = a.copies ? a.header[1] / a.copies : 0;
    const int pos = a.block_sel[blockIdx.x] + (int)es;
    const int src = a.kind == GSR_PLAN_MERGE ? a.pairs[2 * i] : i;
    for (int c = 0; c < a.copies; c++) a.plan[n_keep + c * n_sel + pos] = src | DN_NEW;
    if (a.kind == GSR_PLAN_MERGE) a.plan[a.P + pos] = a.pairs[2 * i + 1];  // the partner list of the merged rows
  }
}

// ---------------------------------------------------------------- rows
constexpr int BUILD_MAX_ARRAYS = 32;
struct BuildArgs {
  int n_arrays, n_out, n_src, first, mode;
  const int *index, *partner;
  const float *xyz, *rot, *scaling, *unit;  // source parameters [n_src][3 / 4 / 3 activated], unit [n_out - first][3]
  float divisor;
  const float *src[BUILD_MAX_ARRAYS];
  float *dst[BUILD_MAX_ARRAYS];
  int width[BUILD_MAX_ARRAYS];
  int zero_new[BUILD_MAX_ARRAYS];
  int role[BUILD_MAX_ARRAYS];
};

// gather_rows_kernel of rows.hip with the new rows (output rows >= first) of the arrays that carry a role recomputed:
//   children: xyz = R(q_s) (s_s * unit[c]) + xyz_s, log-scaling = log(s_s / divisor)          (s = source row, c = row - first)
//   merge:    averaged arrays = 0.5 (row_s + row_partner[c]), log-scaling = log(s_s / 0.8)
// A source row outside [0, n_src) is not read: the element becomes NaN.
__global__ __launch_bounds__(DN_BLOCK) void build_rows_kernel(const BuildArgs a) {
  __shared__ int s_idx[DN_BLOCK];
  const int first = blockIdx.x * DN_BLOCK;
  const int nrows = min(DN_BLOCK, a.n_out - first);
  if ((int)threadIdx.x < nrows) s_idx[threadIdx.x] = a.index[first + threadIdx.x];
  __syncthreads();
  const float nan = quiet_nan();
  for (int k = 0; k < a.n_arrays; k++) {
    const int w = a.width[k];
    const float *src = a.src[k];
    float *dst = a.dst[k] + (size_t)first * w;
    const bool zn = a.zero_new[k] != 0;
    const int role = a.mode ? a.role[k] : GSR_ROW_COPY;
    for (int e = threadIdx.x; e < nrows * w; e += DN_BLOCK) {
      const int r = e / w, c = e - r * w;
      const int s = s_idx[r];
      const bool is_new = (s & DN_NEW) != 0 && s >= 0;
      const int row = s & (DN_NEW - 1);
      float v;
      if (s < 0 || (zn && is_new)) {
        v = 0.f;
      } else if (row >= a.n_src) {
        v = nan;
      } else if (role == GSR_ROW_COPY || role == GSR_ROW_ROTATION || first + r < a.first) {
        v = src[(size_t)row * w + c];
      } else if (role == GSR_ROW_LOG_SCALING) {
        v = logf(a.scaling[(size_t)row * 3 + c] / a.divisor);
      } else if (a.mode == GSR_BUILD_MERGE) {  // GSR_ROW_XYZ and GSR_ROW_MEAN
        const int other = a.partner[first + r - a.first];
        v = (unsigned)other < (unsigned)a.n_src ? 0.5f * (src[(size_t)row * w + c] + src[(size_t)other * w + c]) : nan;
      } else if (role == GSR_ROW_XYZ) {  // children
        const float *u = a.unit + (size_t)(first + r - a.first) * 3, *sc = a.scaling + (size_t)row * 3;
        float R[9];
        quat_rotation(a.rot + (size_t)row * 4, R);
        v = R[3 * c] * (sc[0] * u[0]) + R[3 * c + 1] * (sc[1] * u[1]) + R[3 * c + 2] * (sc[2] * u[2]) + a.xyz[(size_t)row * 3 + c];
      } else {
        v = src[(size_t)row * w + c];
      }
      dst[e] = v;
    }
  }
}

}  // namespace gsr

extern "C" int gsr_kl_pairs(int P, const float *xyz, const float *rotation, const float *log_scaling, const int *pairs, float *kl,
                            gsr_stream_t stream_) {
  using namespace gsr;
  if (P < 0 || (P > 0 && (!xyz || !rotation || !log_scaling || !pairs || !kl))) {
    set_error("gsr_kl_pairs: bad arguments");
    return GSR_EINVAL;
  }
  if (P == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(kl_pairs_kernel, dim3(dn_grid(P)), dim3(DN_BLOCK), 0, stream, P, xyz, rotation, log_scaling, pairs, kl);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

extern "C" int gsr_densify_select(int P, int mode, const float *grads, int n_grads, const float *scaling, const float *kl,
                                  float grad_threshold, float size_threshold, float kl_threshold, unsigned char *flags,
                                  gsr_stream_t stream_) {
  using namespace gsr;
  if (P < 0 || mode < GSR_DENSIFY_CLONE || mode > GSR_DENSIFY_MERGE || n_grads < 0 || n_grads > P || (n_grads > 0 && !grads) ||
      (P > 0 && (!scaling || !flags))) {
    set_error("gsr_densify_select: bad arguments (mode 0..2, n_grads <= P)");
    return GSR_EINVAL;
  }
  if (P == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(densify_select_kernel, dim3(dn_grid(P)), dim3(DN_BLOCK), 0, stream, P, mode, grads, n_grads, scaling, kl,
                     grad_threshold, size_threshold, kl_threshold, flags);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

extern "C" size_t gsr_densify_plan_workspace_bytes(int P) {
  using namespace gsr;
  if (P < 0) return 0;
  return align_up((size_t)P, 256) + 2 * align_up(sizeof(int) * (size_t)dn_blocks(P), 256) + 256;
}

extern "C" int gsr_densify_plan(int P, int kind, int N, const unsigned char *flags, const int *pairs, int *plan, int *header,
                                char *workspace, size_t workspace_bytes, gsr_stream_t stream_) {
  using namespace gsr;
  if (P < 0 || kind < GSR_PLAN_PRUNE || kind > GSR_PLAN_MERGE || !header || (P > 0 && (!flags || !plan || !workspace)) ||
      (kind == GSR_PLAN_SPLIT && N < 1) || (kind == GSR_PLAN_MERGE && P > 0 && !pairs)) {
    set_error("gsr_densify_plan: bad arguments (kind 0..3, N >= 1, pairs for a merge)");
    return GSR_EINVAL;
  }
  const int copies = kind == GSR_PLAN_PRUNE ? 0 : (kind == GSR_PLAN_SPLIT ? N : 1);
  if ((long long)(copies + 1) * (long long)P >= (long long)DN_NEW) {
    set_error("gsr_densify_plan: (N + 1) * P must stay below 2^30 (bit 30 of a plan entry marks a new row)");
    return GSR_EINVAL;
  }
  if (workspace_bytes < gsr_densify_plan_workspace_bytes(P) || (reinterpret_cast<uintptr_t>(workspace) & 3)) {
    set_error("gsr_densify_plan: workspace too small (gsr_densify_plan_workspace_bytes) or not 4-byte aligned");
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int blocks = dn_blocks(P);
  PlanArgs a = {};
  a.P = P;
  a.kind = kind;
  a.copies = copies;
  a.flags = flags;
  a.pairs = pairs;
  a.plan = plan;
  a.header = header;
  uintptr_t p = carve_begin(workspace);
  carve(p, a.gone, (size_t)P);
  carve(p, a.block_keep, (size_t)blocks);
  carve(p, a.block_sel, (size_t)blocks);
  if (kind == GSR_PLAN_MERGE && P > 0) {
    GSR_HIP(zero_async(a.gone, align_up((size_t)P, 4), stream));
    hipLaunchKernelGGL(plan_gone_kernel, dim3(dn_grid(P)), dim3(DN_BLOCK), 0, stream, a);
    GSR_LAUNCH_CHECK(stream, 0);
  }
  if (P > 0) {
    hipLaunchKernelGGL(plan_count_kernel, dim3(blocks), dim3(DN_BLOCK), 0, stream, a);
    GSR_LAUNCH_CHECK(stream, 0);
  }
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, stream, a, blocks);
  GSR_LAUNCH_CHECK(stream, 0);
  if (P > 0) {
    hipLaunchKernelGGL(plan_scatter_kernel, dim3(blocks), dim3(DN_BLOCK), 0, stream, a);
    GSR_LAUNCH_CHECK(stream, 0);
  }
  return GSR_OK;
}

extern "C" int gsr_build_rows(int n_arrays, const float *const *src, float *const *dst, const int *row_floats, const int *zero_new,
                              const int *role, int n_out, const int *index, int n_src, int first, int mode, const float *scaling,
                              const float *unit, float divisor, const int *partner, gsr_stream_t stream_) {
  using namespace gsr;
  if (n_arrays < 1 || n_arrays > BUILD_MAX_ARRAYS || n_out < 0 || n_src < 0 || !src || !dst || !row_floats || (n_out > 0 && !index) ||
      mode < GSR_BUILD_MOVE || mode > GSR_BUILD_MERGE || (mode != GSR_BUILD_MOVE && (!role || first < 0 || first > n_out))) {
    set_error("gsr_build_rows: bad arguments (1..%d arrays, mode 0..2, roles and 0 <= first <= n_out for modes 1, 2)", BUILD_MAX_ARRAYS);
    return GSR_EINVAL;
  }
  if (n_out == 0) return GSR_OK;
  BuildArgs a = {};
  a.n_arrays = n_arrays;
  a.n_out = n_out;
  a.n_src = n_src;
  a.first = mode == GSR_BUILD_MOVE ? n_out : first;
  a.mode = mode;
  a.index = index;
  a.partner = partner;
  a.scaling = scaling;
  a.unit = unit;
  a.divisor = mode == GSR_BUILD_MERGE ? 0.8f : divisor;
  for (int k = 0; k < n_arrays; k++) {
    if (!src[k] || !dst[k] || row_floats[k] < 1) {
      set_error("gsr_build_rows: array %d has a null pointer or a row size < 1", k);
      return GSR_EINVAL;
    }
    a.src[k] = src[k];
    a.dst[k] = dst[k];
    a.width[k] = row_floats[k];
    a.zero_new[k] = zero_new ? zero_new[k] : 0;
    a.role[k] = role ? role[k] : GSR_ROW_COPY;
    if (a.role[k] < GSR_ROW_COPY || a.role[k] > GSR_ROW_MEAN) {
      set_error("gsr_build_rows: array %d has an unknown role", k);
      return GSR_EINVAL;
    }
    const int need = a.role[k] == GSR_ROW_XYZ || a.role[k] == GSR_ROW_LOG_SCALING ? 3 : (a.role[k] == GSR_ROW_ROTATION ? 4 : 0);
    if (need && a.width[k] != need) {
      set_error("gsr_build_rows: array %d: the role needs rows of %d floats", k, need);
      return GSR_EINVAL;
    }
    // the parameters themselves (the arrays that are not zeroed for new rows) are what the new rows are computed from
    if (!a.zero_new[k] && a.role[k] == GSR_ROW_XYZ) a.xyz = a.src[k];
    if (!a.zero_new[k] && a.role[k] == GSR_ROW_ROTATION) a.rot = a.src[k];
  }
  if (mode != GSR_BUILD_MOVE && a.first < n_out) {
    const bool ok = mode == GSR_BUILD_MERGE ? (scaling && partner) : (scaling && unit && a.xyz && a.rot && divisor > 0.f);
    if (!ok) {
      set_error("gsr_build_rows: new rows need the activated scaling and (children) unit draws, a positive divisor and the xyz and "
                "rotation arrays, or (merge) the partner list");
      return GSR_EINVAL;
    }
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(build_rows_kernel, dim3(dn_blocks(n_out)), dim3(DN_BLOCK), 0, stream, a);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}
