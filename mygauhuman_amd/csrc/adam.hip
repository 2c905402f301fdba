// adam.hip -- multi-tensor Adam step with the densification statistics folded in (train.py:401-423).
//
// What follows loss.backward() in the reference's loop is one fused torch kernel per parameter group plus the counters'
// _foreach_add_, eight elementwise kernels of statistics and a clamp of the light's cube map: twenty to forty launches around
// a single pass over memory.  Here every tensor of every group is one entry of a by-value table (as RowsArgs in rows.hip) and
// ONE kernel streams them all: the work list is the concatenation of every array's 4,096-float chunks (and of the statistics'
// 1,024-row chunks), a workgroup takes entries blockIdx.x, + gridDim.x, ... so a 128-float bias and the 9M-float f_rest keep the
// machine equally busy.  The learning rate comes from the launch arguments or from a device table, the step counts from device
// memory: the launch can be recorded into a graph and replayed under a changing schedule.
//
// The counter hazard: a workgroup forms its bias corrections from its array's step count, so nobody may advance a count while a
// workgroup that has yet to read it is outstanding.  The counts are advanced by a launch of their own IN FRONT of the update
// (one lane per array); the update reads the advanced value.  Two launches per call, ordered by the stream.
#include "gsr_common.h"

#include <math.h>

namespace gsr {

constexpr int ADAM_BLOCK = 256;
constexpr int ADAM_UNROLL = 4;                             // 16-byte accesses per lane and array
constexpr int ADAM_CHUNK = ADAM_BLOCK * 4 * ADAM_UNROLL;   // floats per work-list entry
constexpr int STATS_ROWS = ADAM_BLOCK * 4;                 // rows per statistics entry
constexpr unsigned ADAM_MAX_GRID = 2048;                   // 256 CUs x 8 workgroups; the rest is grid-strided

struct AdamStats {
  int P, stride;
  const float *grad;
  const uint8_t *filter;
  const int *radii;
  float *accum, *denom, *max_radii;
};
struct AdamArgs {
  float *param[GSR_ADAM_MAX_ARRAYS];
  const float *grad[GSR_ADAM_MAX_ARRAYS];
  float *m[GSR_ADAM_MAX_ARRAYS];
  float *v[GSR_ADAM_MAX_ARRAYS];
  uint32_t count[GSR_ADAM_MAX_ARRAYS];
  uint32_t chunk_start[GSR_ADAM_MAX_ARRAYS + 1];  // exclusive prefix of the arrays' chunk counts
  int step_slot[GSR_ADAM_MAX_ARRAYS];
  uint8_t group[GSR_ADAM_MAX_ARRAYS];
  gsr_adam_group groups[GSR_ADAM_MAX_GROUPS];
  const float *lr_table;
  const float *steps;
  int n_arrays;
  uint32_t stats_chunks;
  AdamStats stats;
};
static_assert(sizeof(AdamArgs) <= 4096 - 64, "AdamArgs must stay under the 4 KB kernel-argument limit");
struct AdamAdvanceArgs {
  float *steps;
  int n;
  int slot[GSR_ADAM_MAX_ARRAYS];
};

// per-array constants, formed the way torch.optim.Adam forms them: the bias corrections and the step size in double
struct AdamCoef {
  double b1, w1, b2, w2;
  float bc2_sqrt, neg_step_size, eps, clamp_min;
  bool clamp;
};

__global__ __launch_bounds__(64) void adam_advance_kernel(const AdamAdvanceArgs a) {
  const int i = threadIdx.x;
  if (i < a.n) a.steps[a.slot[i]] += 1.0f;
}

// beta^t for an integer t by repeated squaring (a dozen double multiplications, wave-uniform)
__device__ __forceinline__ double adam_ipow(double b, uint32_t t) {
  double r = 1.0;
  while (t) {
    if (t & 1u) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamCoef &c) {
  // The moments are formed in double and rounded once, as torch's fused Adam does (its betas are doubles): half an ulp per step
  // instead of the two or three a float32 chain leaves in a sum that is carried for thousands of steps.  Five double operations
  // per element are free in a kernel that waits for memory.
  const double gd = (double)g;
  m = (float)fma(c.w1, gd, c.b1 * (double)m);        // exp_avg = beta1 exp_avg + (1 - beta1) grad
  v = (float)fma(c.w2 * gd, gd, c.b2 * (double)v);   // exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) grad^2
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = fmaf(c.neg_step_size, m / denom, p);           // param.addcdiv_(exp_avg, denom, value = -step_size)
  if (c.clamp) p = (p != p) ? p : fmaxf(p, c.clamp_min);
}

__device__ __forceinline__ void adam_stats_chunk(const AdamStats &s, uint32_t chunk) {
#pragma unroll
  for (int j = 0; j < STATS_ROWS / ADAM_BLOCK; j++) {
    const uint32_t row = chunk * STATS_ROWS + j * ADAM_BLOCK + threadIdx.x;
    if (row < (uint32_t)s.P && s.filter[row]) {
      const float gx = s.grad[(size_t)row * s.stride], gy = s.grad[(size_t)row * s.stride + 1];
      s.accum[row] += sqrtf(fmaf(gx, gx, gy * gy));
      s.denom[row] += 1.0f;
      const float r = (float)s.radii[row], old = s.max_radii[row];
      s.max_radii[row] = r > old ? r : old;
    }
  }
}

__global__ __launch_bounds__(ADAM_BLOCK) void adam_update_kernel(const AdamArgs a) {
  const uint32_t n_chunks = a.chunk_start[a.n_arrays], total = n_chunks + a.stats_chunks;
  int cur = -1;
  AdamCoef c = {};
  bool vec = false;
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
    if (w >= n_chunks) {
      adam_stats_chunk(a.stats, w - n_chunks);
      continue;
    }
    // the array of this entry: the largest k with chunk_start[k] <= w (an array without chunks is never the largest)
    int lo = 0, hi = a.n_arrays;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.chunk_start[mid] <= w) lo = mid; else hi = mid;
    }
    const int k = lo;
    if (k != cur) {
      cur = k;
      const gsr_adam_group &g = a.groups[a.group[k]];
      const uint32_t t = (uint32_t)a.steps[a.step_slot[k]];  // already advanced: this update's step number
      const double bc1 = 1.0 - adam_ipow(g.beta1, t), bc2 = 1.0 - adam_ipow(g.beta2, t);
      const float lr = a.lr_table ? a.lr_table[g.lr_slot] : g.lr;
      c.b1 = g.beta1;
      c.w1 = 1.0 - g.beta1;
      c.b2 = g.beta2;
      c.w2 = 1.0 - g.beta2;
      c.bc2_sqrt = (float)sqrt(bc2);
      c.neg_step_size = (float)(-((double)lr / bc1));
      c.eps = g.eps;
      c.clamp_min = g.clamp_min;
      c.clamp = g.clamp_min > -INFINITY;
      vec = ((reinterpret_cast<uintptr_t>(a.param[k]) | reinterpret_cast<uintptr_t>(a.grad[k]) |
              reinterpret_cast<uintptr_t>(a.m[k]) | reinterpret_cast<uintptr_t>(a.v[k])) & 15u) == 0;
    }
    float *__restrict__ P = a.param[k];
    const float *__restrict__ G = a.grad[k];
    float *__restrict__ M = a.m[k];
    float *__restrict__ V = a.v[k];
    const uint32_t n = a.count[k];
    const uint32_t base = (w - a.chunk_start[k]) * (uint32_t)ADAM_CHUNK;
    if (vec) {
      float4 p4[ADAM_UNROLL], g4[ADAM_UNROLL], m4[ADAM_UNROLL], v4[ADAM_UNROLL];
#pragma unroll
      for (int j = 0; j < ADAM_UNROLL; j++) {
        const uint32_t i = base + (j * ADAM_BLOCK + threadIdx.x) * 4;
        if (i + 4 <= n) {
          p4[j] = *reinterpret_cast<const float4 *>(P + i);
          g4[j] = *reinterpret_cast<const float4 *>(G + i);
          m4[j] = *reinterpret_cast<const float4 *>(M + i);
          v4[j] = *reinterpret_cast<const float4 *>(V + i);
        }
      }
#pragma unroll
      for (int j = 0; j < ADAM_UNROLL; j++) {
        const uint32_t i = base + (j * ADAM_BLOCK + threadIdx.x) * 4;
        if (i + 4 <= n) {
          adam_element(p4[j].x, g4[j].x, m4[j].x, v4[j].x, c);
          adam_element(p4[j].y, g4[j].y, m4[j].y, v4[j].y, c);
          adam_element(p4[j].z, g4[j].z, m4[j].z, v4[j].z, c);
          adam_element(p4[j].w, g4[j].w, m4[j].w, v4[j].w, c);
          *reinterpret_cast<float4 *>(P + i) = p4[j];
          *reinterpret_cast<float4 *>(M + i) = m4[j];
          *reinterpret_cast<float4 *>(V + i) = v4[j];
        } else {
          for (uint32_t e = i; e < n; e++) {  // the array's last 1..3 floats
            float p = P[e], m = M[e], v = V[e];
            adam_element(p, G[e], m, v, c);
            P[e] = p;
            M[e] = m;
            V[e] = v;
          }
        }
      }
    } else {
      // some pointer sits at an odd float offset (a view into a flat gradient bucket, rows of 1 / 3 / 45 floats): 4-byte accesses,
      // a wave still covers 256 contiguous bytes per instruction
#pragma unroll
      for (int j0 = 0; j0 < 4 * ADAM_UNROLL; j0 += 4) {
        float p[4], g[4], m[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t i = base + (j0 + j) * ADAM_BLOCK + threadIdx.x;
          if (i < n) {
            p[j] = P[i];
            g[j] = G[i];
            m[j] = M[i];
            v[j] = V[i];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t i = base + (j0 + j) * ADAM_BLOCK + threadIdx.x;
          if (i < n) {
            adam_element(p[j], g[j], m[j], v[j], c);
            P[i] = p[j];
            M[i] = m[j];
            V[i] = v[j];
          }
        }
      }
    }
  }
}

static int stats_from_abi(const gsr_adam_stats *s, AdamStats &out, uint32_t &chunks, const char *who) {
  out = {};
  chunks = 0;
  if (!s || s->P == 0) return GSR_OK;
  if (s->P < 0 || s->grad_stride < 2 || !s->grad || !s->filter || !s->radii || !s->grad_accum || !s->denom || !s->max_radii) {
    set_error("%s: statistics block with P < 0, a row stride < 2 or a null pointer", who);
    return GSR_EINVAL;
  }
  out.P = s->P;
  out.stride = s->grad_stride;
  out.grad = s->grad;
  out.filter = s->filter;
  out.radii = s->radii;
  out.accum = s->grad_accum;
  out.denom = s->denom;
  out.max_radii = s->max_radii;
  chunks = ((uint32_t)s->P + STATS_ROWS - 1) / STATS_ROWS;
  return GSR_OK;
}

}  // namespace gsr

extern "C" int gsr_adam_chunk_floats(void) { return gsr::ADAM_CHUNK; }

extern "C" int gsr_adam_step(int n_arrays, const gsr_adam_array *arrays, int n_groups, const gsr_adam_group *groups,
                             const float *lr_table, float *steps, const gsr_adam_stats *stats, int debug, gsr_stream_t stream_) {
  using namespace gsr;
  if (n_arrays < 0 || n_arrays > GSR_ADAM_MAX_ARRAYS || n_groups < 0 || n_groups > GSR_ADAM_MAX_GROUPS) {
    set_error("gsr_adam_step: %d arrays of %d groups (at most %d arrays and %d groups per call)", n_arrays, n_groups,
              GSR_ADAM_MAX_ARRAYS, GSR_ADAM_MAX_GROUPS);
    return GSR_EINVAL;
  }
  if (n_arrays > 0 && (!arrays || !groups || !steps || n_groups < 1)) {
    set_error("gsr_adam_step: null array table, group table or step table");
    return GSR_EINVAL;
  }
  AdamArgs a = {};
  AdamAdvanceArgs adv = {};
  for (int g = 0; g < (n_arrays > 0 ? n_groups : 0); g++) {
    const gsr_adam_group &q = groups[g];
    if (!(q.beta1 >= 0.0 && q.beta1 < 1.0) || !(q.beta2 >= 0.0 && q.beta2 < 1.0)) {
      set_error("gsr_adam_step: group %d: beta outside [0, 1)", g);
      return GSR_EINVAL;
    }
    if (!(q.eps > 0.f)) {
      set_error("gsr_adam_step: group %d: eps must be > 0", g);
      return GSR_EINVAL;
    }
    if (lr_table && q.lr_slot < 0) {
      set_error("gsr_adam_step: group %d: negative slot in the learning-rate table", g);
      return GSR_EINVAL;
    }
    a.groups[g] = q;
  }
  uint32_t chunks = 0;
  for (int k = 0; k < n_arrays; k++) {
    const gsr_adam_array &q = arrays[k];
    if (q.count < 0 || q.count > 0x7FFFFFFFll || q.group < 0 || q.group >= n_groups || q.step_slot < 0) {
      set_error("gsr_adam_step: array %d: bad element count, group index or step slot", k);
      return GSR_EINVAL;
    }
    if (q.count > 0 && (!q.param || !q.grad || !q.exp_avg || !q.exp_avg_sq)) {
      set_error("gsr_adam_step: array %d has a null pointer", k);
      return GSR_EINVAL;
    }
    for (int j = 0; j < k; j++) {
      if (arrays[j].step_slot == q.step_slot) {
        set_error("gsr_adam_step: arrays %d and %d share step slot %d", j, k, q.step_slot);
        return GSR_EINVAL;
      }
    }
    a.param[k] = q.param;
    a.grad[k] = q.grad;
    a.m[k] = q.exp_avg;
    a.v[k] = q.exp_avg_sq;
    a.count[k] = (uint32_t)q.count;
    a.chunk_start[k] = chunks;
    a.step_slot[k] = adv.slot[k] = q.step_slot;
    a.group[k] = (uint8_t)q.group;
    chunks += (uint32_t)((q.count + ADAM_CHUNK - 1) / ADAM_CHUNK);
  }
  a.chunk_start[n_arrays] = chunks;
  a.n_arrays = n_arrays;
  a.lr_table = lr_table;
  a.steps = steps;
  int rc = stats_from_abi(stats, a.stats, a.stats_chunks, "gsr_adam_step");
  if (rc != GSR_OK) return rc;
  const uint64_t total = (uint64_t)chunks + a.stats_chunks;
  if (n_arrays == 0 && total == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (n_arrays > 0) {
    adv.steps = steps;
    adv.n = n_arrays;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, stream, adv);
    GSR_LAUNCH_CHECK(stream, 0);
  }
  if (total > 0) {
    const unsigned grid = (unsigned)(total < ADAM_MAX_GRID ? total : ADAM_MAX_GRID);
    hipLaunchKernelGGL(adam_update_kernel, dim3(grid), dim3(ADAM_BLOCK), 0, stream, a);
  }
  GSR_LAUNCH_CHECK(stream, debug);
  return GSR_OK;
}

extern "C" int gsr_stats_update(const gsr_adam_stats *stats, int debug, gsr_stream_t stream_) {
  using namespace gsr;
  if (!stats) {
    set_error("gsr_stats_update: null statistics block");
    return GSR_EINVAL;
  }
  AdamArgs a = {};
  int rc = stats_from_abi(stats, a.stats, a.stats_chunks, "gsr_stats_update");
  if (rc != GSR_OK) return rc;
  if (a.stats_chunks == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const unsigned grid = a.stats_chunks < ADAM_MAX_GRID ? a.stats_chunks : ADAM_MAX_GRID;
  hipLaunchKernelGGL(adam_update_kernel, dim3(grid), dim3(ADAM_BLOCK), 0, stream, a);
  GSR_LAUNCH_CHECK(stream, debug);
  return GSR_OK;
}
