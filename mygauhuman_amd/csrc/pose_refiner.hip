// pose_refiner.hip -- the pose-correction network of render() (nets/mlp_delta_body_pose.py: BodyPoseRefiner as
// scene/gaussian_model.py:95 builds it, total_bones = J, embedding_size = 3(J-1), mlp_width = 128, mlp_depth = 2; run every frame
// when motion_offset_flag is set: gaussian_renderer/__init__.py:100-106), forward and backward, ONE launch each way.
//
//   h1 = relu(W0 x + b0)   h2 = relu(W2 h1 + b2)   r = W4 h2 + b4          x, r: E = 3(J-1) per pose row, B <= 16 rows
//   per row of r viewed as [J-1][3]:  theta = sqrt(1e-5 + |r|^2), n = r / theta,  Rs = cos I + (1 - cos) n n^T + sin [n]x
// (the reference's RodriguesModule, entry by entry: NOT the SMPL batch_rodrigues of pose.hip).  As torch ops this is ~15 launches
// forward and ~30 backward for 35k multiply-adds at B = 1: launch latency, not arithmetic.  Here one workgroup of sixteen waves:
//   * every weight a lane will touch is loaded into its registers at the start (at most 62 floats per lane): the three layers'
//     global round trips overlap, one memory latency per call instead of one per layer (the backward reloads W0 for dx late);
//   * output o of a layer belongs to wave o % 16, its input features k to the lanes (k = lane + 64 c), so the weight loads are
//     row-contiguous and coalesced; a dot product ends in a sum over the 64 lanes whose first log2(BB) exchanges each hand half of
//     the remaining pose rows to the partner lane (BB + 6 - log2 BB exchanges for BB rows instead of 6 BB);
//   * activations live in LDS; the backward's transposed products (dh = W^T dz) reuse the same register tiles, each wave summing
//     over its own outputs, then the sixteen partial rows are added in wave order through LDS;
//   * every sum has a fixed order (no atomics): two calls give the same bits, and every gradient tensor is written whole.
#include <math.h>

#include "gsr_common.h"

namespace gsr {

constexpr int PR_W = 128;                    // hidden width: the only one the kernels are built for
constexpr int PR_WAVES = 16;
constexpr int PR_THREADS = PR_WAVES * WAVE;
constexpr int PR_MAX_B = 16;
constexpr int PR_GROUP = 4;                  // pose rows per pass of the cross-wave sums (bounds their LDS)
constexpr int PR_NO = PR_W / PR_WAVES;       // outputs per wave of a hidden layer
constexpr int PR_KCW = PR_W / WAVE;          // 64-wide chunks of a hidden row

struct PoseRefinerArgs {
  const float *x;
  long long sx_b, sx_e;                      // element strides of x [B][E]
  const float *w[3], *b[3];                  // block_mlps.0 / .2 / .4: weight [out][in] row-major, bias [out]
  int B;
  float *Rs;                                 // forward: [B][J-1][9]
  const float *dRs;                          // backward: dL/dRs [B][J-1][9]
  float *dw[3], *db[3], *dx;                 // backward: whole tensors (dx [B][E] or null)
};

template <int E>
struct PrShape {
  static constexpr int KC0 = (E + WAVE - 1) / WAVE;            // 64-wide chunks of an E-long row
  static constexpr int KP = KC0 * WAVE;                         // padded row of x / r in LDS
  static constexpr int NO4 = (E + PR_WAVES - 1) / PR_WAVES;    // outputs per wave of the last layer
  static constexpr int NJ = E / 3;
};

template <int E>
struct PrWeights {                           // this lane's slice: W[wave + 16 i][lane + 64 c]
  float w0[PR_NO][PrShape<E>::KC0];
  float w2[PR_NO][PR_KCW];
  float w4[PrShape<E>::NO4][PR_KCW];
};

// rows o = wave + 16 i (< O) of a row-major [O][K] weight, columns k = lane + 64 c (< K); zero elsewhere
template <int NO, int KC>
__device__ __forceinline__ void pr_load_rows(const float *W, int O, int K, float (&r)[NO][KC], int lane, int wave) {
#pragma unroll
  for (int i = 0; i < NO; i++) {
    const int o = wave + PR_WAVES * i;
#pragma unroll
    for (int c = 0; c < KC; c++) {
      const int k = lane + WAVE * c;
      r[i][c] = (o < O && k < K) ? W[o * K + k] : 0.f;
    }
  }
}

template <int E>
__device__ __forceinline__ void pr_load_weights(const PoseRefinerArgs &a, PrWeights<E> &r, int lane, int wave) {
  pr_load_rows(a.w[0], PR_W, E, r.w0, lane, wave);
  pr_load_rows(a.w[1], PR_W, PR_W, r.w2, lane, wave);
  pr_load_rows(a.w[2], E, PR_W, r.w4, lane, wave);
}

// x -> s_x [BB][KP] (rows >= B and columns >= E: zero), the three biases -> s_bias [128 | 128 | E]
template <int E, int BB>
__device__ __forceinline__ void pr_load_inputs(const PoseRefinerArgs &a, float *s_x, float *s_bias, int tid) {
  constexpr int KP = PrShape<E>::KP;
  for (int t = tid; t < BB * KP; t += PR_THREADS) {
    const int b = t / KP, k = t % KP;
    s_x[t] = (b < a.B && k < E) ? a.x[(long long)b * a.sx_b + (long long)k * a.sx_e] : 0.f;
  }
  for (int t = tid; t < 2 * PR_W + E; t += PR_THREADS)
    s_bias[t] = t < PR_W ? a.b[0][t] : (t < 2 * PR_W ? a.b[1][t - PR_W] : a.b[2][t - 2 * PR_W]);
}

__host__ __device__ constexpr int pr_log2(int n) { return n <= 1 ? 0 : 1 + pr_log2(n / 2); }

// v[b] = this lane's partial sum for pose row b -> v[0] = the sum over all 64 lanes for row lane >> (6 - log2 BB).  The first
// log2(BB) exchanges (masks 32, 16, ...) each hand half of the remaining rows to the partner lane, the rest are a plain butterfly.
template <int BB, int S = 0>
__device__ __forceinline__ void pr_reduce(float (&v)[BB], int lane) {
  if constexpr ((1 << S) < BB) {
    constexpr int m = 32 >> S, h = (BB >> S) / 2;
    const bool hi = (lane & m) != 0;
#pragma unroll
    for (int j = 0; j < h; j++) {
      const float send = hi ? v[j] : v[j + h];
      const float keep = hi ? v[j + h] : v[j];
      v[j] = keep + __shfl_xor(send, m);
    }
    pr_reduce<BB, S + 1>(v, lane);
  } else {
#pragma unroll
    for (int m = 32 >> S; m >= 1; m >>= 1) v[0] += __shfl_xor(v[0], m);
  }
}

// y[b][o] = act(sum_k W[o][k] a[b][k] + bias[o]) for this wave's outputs o = wave + 16 i < O, all BB rows
template <int BB, int KC, int NO, bool RELU>
__device__ __forceinline__ void pr_dense(const float (&w)[NO][KC], const float *s_a, int lda, const float *s_bias, int O, float *s_y,
                                         int ldy, int lane, int wave) {
  constexpr int LB = pr_log2(BB);
#pragma unroll
  for (int i = 0; i < NO; i++) {
    const int o = wave + PR_WAVES * i;
    if (o < O) {
      float v[BB];
#pragma unroll
      for (int b = 0; b < BB; b++) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < KC; c++) s = fmaf(w[i][c], s_a[b * lda + lane + WAVE * c], s);
        v[b] = s;
      }
      pr_reduce<BB>(v, lane);
      if ((lane & ((WAVE >> LB) - 1)) == 0) {
        const float y = v[0] + s_bias[o];
        s_y[(lane >> (6 - LB)) * ldy + o] = RELU ? (y > 0.f ? y : 0.f) : y;
      }
    }
  }
}

// out[b][k] = sum_o W[o][k] g[b][o] (k < K, b < B), zero where mask[b][k] <= 0 (the ReLU's threshold_backward) when a mask is
// given.  Each wave sums over its own outputs from its register tile; the 16 partial rows are added in wave order.  Barriers inside.
template <int BB, int KC, int NO>
__device__ __forceinline__ void pr_dense_t(const float (&w)[NO][KC], const float *s_g, int ldg, int O, float *s_part, float *out,
                                           int ldo, int K, int B, const float *s_mask, int ldm, int lane, int wave, int tid) {
  constexpr int G = BB < PR_GROUP ? BB : PR_GROUP, KP = KC * WAVE;
#pragma unroll
  for (int b0 = 0; b0 < BB; b0 += G) {
    if (b0 >= B) break;                      // (uniform over the workgroup)
    float p[G][KC];
#pragma unroll
    for (int g = 0; g < G; g++) {
#pragma unroll
      for (int c = 0; c < KC; c++) p[g][c] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < NO; i++) {
      const int o = wave + PR_WAVES * i;
      if (o < O) {
#pragma unroll
        for (int g = 0; g < G; g++) {
          const float gv = s_g[(b0 + g) * ldg + o];
#pragma unroll
          for (int c = 0; c < KC; c++) p[g][c] = fmaf(w[i][c], gv, p[g][c]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
#pragma unroll
      for (int c = 0; c < KC; c++) s_part[(wave * G + g) * KP + lane + WAVE * c] = p[g][c];
    }
    __syncthreads();
    for (int t = tid; t < G * K; t += PR_THREADS) {
      const int g = t / K, k = t % K, b = b0 + g;
      float s = 0.f;
      for (int q = 0; q < PR_WAVES; q++) s += s_part[(q * G + g) * KP + k];
      if (s_mask && !(s_mask[b * ldm + k] > 0.f)) s = 0.f;
      if (b < B) out[b * ldo + k] = s;
    }
    __syncthreads();
  }
}

// dW[o][k] = sum_b g[b][o] a[b][k], db[o] = sum_b g[b][o] (b = 0 .. B-1 in order) for this wave's outputs
template <int KC, int NO>
__device__ __forceinline__ void pr_wgrad(const float *s_g, int ldg, const float *s_a, int lda, int O, int K, float *dW, float *db, int B,
                                         int lane, int wave) {
#pragma unroll
  for (int i = 0; i < NO; i++) {
    const int o = wave + PR_WAVES * i;
    if (o < O) {
#pragma unroll
      for (int c = 0; c < KC; c++) {
        const int k = lane + WAVE * c;
        if (k < K) {
          float s = 0.f;
          for (int b = 0; b < B; b++) s = fmaf(s_g[b * ldg + o], s_a[b * lda + k], s);
          dW[o * K + k] = s;
        }
      }
      if (lane == 0) {
        float s = 0.f;
        for (int b = 0; b < B; b++) s += s_g[b * ldg + o];
        db[o] = s;
      }
    }
  }
}

struct PrRod {
  float th, n[3], c, s;
};

__device__ __forceinline__ void pr_rodrigues(const float *r, PrRod &q, float *R) {
  q.th = sqrtf(1e-5f + (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
#pragma unroll
  for (int k = 0; k < 3; k++) q.n[k] = r[k] / q.th;
  q.c = cosf(q.th);
  q.s = sinf(q.th);
  const float n0 = q.n[0], n1 = q.n[1], n2 = q.n[2], c = q.c, s = q.s, omc = 1.f - q.c;
  R[0] = n0 * n0 + (1.f - n0 * n0) * c;
  R[1] = n0 * n1 * omc - n2 * s;
  R[2] = n0 * n2 * omc + n1 * s;
  R[3] = n0 * n1 * omc + n2 * s;
  R[4] = n1 * n1 + (1.f - n1 * n1) * c;
  R[5] = n1 * n2 * omc - n0 * s;
  R[6] = n0 * n2 * omc - n1 * s;
  R[7] = n1 * n2 * omc + n0 * s;
  R[8] = n2 * n2 + (1.f - n2 * n2) * c;
}

// dL/dr from dL/dR (G, row-major 3x3) for R = c I + (1 - c) n n^T + s [n]x, n = r / theta, theta = sqrt(1e-5 + |r|^2)
__device__ __forceinline__ void pr_rodrigues_bwd(const PrRod &q, const float *G, float *dr) {
  const float *n = q.n;
  const float omc = 1.f - q.c;
  float nGn = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) nGn = fmaf(G[3 * i + j] * n[i], n[j], nGn);
  const float dc = (G[0] + G[4] + G[8]) - nGn;
  const float w[3] = {G[7] - G[5], G[2] - G[6], G[3] - G[1]};
  const float ds = n[0] * w[0] + n[1] * w[1] + n[2] * w[2];
  float dn[3], dnn = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) t = fmaf(G[3 * k + j] + G[3 * j + k], n[j], t);
    dn[k] = omc * t + q.s * w[k];
    dnn = fmaf(dn[k], n[k], dnn);
  }
  const float dth = q.c * ds - q.s * dc - dnn / q.th;   // n = r / theta: dn/dtheta = -n / theta
#pragma unroll
  for (int k = 0; k < 3; k++) dr[k] = dn[k] / q.th + dth * n[k];   // dtheta/dr = r / theta = n
}

template <int E, int BB>
__global__ __launch_bounds__(PR_THREADS) void pose_refiner_forward_kernel(const PoseRefinerArgs a) {
  using S = PrShape<E>;
  __shared__ float s_x[BB * S::KP], s_h1[BB * PR_W], s_h2[BB * PR_W], s_r[BB * S::KP], s_bias[2 * PR_W + E];
  const int tid = threadIdx.x, lane = tid % WAVE, wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  PrWeights<E> w;
  pr_load_weights<E>(a, w, lane, wave);
  pr_load_inputs<E, BB>(a, s_x, s_bias, tid);
  __syncthreads();
  pr_dense<BB, S::KC0, PR_NO, true>(w.w0, s_x, S::KP, s_bias, PR_W, s_h1, PR_W, lane, wave);
  __syncthreads();
  pr_dense<BB, PR_KCW, PR_NO, true>(w.w2, s_h1, PR_W, s_bias + PR_W, PR_W, s_h2, PR_W, lane, wave);
  __syncthreads();
  pr_dense<BB, PR_KCW, S::NO4, false>(w.w4, s_h2, PR_W, s_bias + 2 * PR_W, E, s_r, S::KP, lane, wave);
  __syncthreads();
  for (int t = tid; t < a.B * S::NJ; t += PR_THREADS) {
    const int b = t / S::NJ, j = t % S::NJ;
    PrRod q;
    float R[9];
    pr_rodrigues(&s_r[b * S::KP + 3 * j], q, R);
#pragma unroll
    for (int k = 0; k < 9; k++) a.Rs[(size_t)t * 9 + k] = R[k];
  }
}

template <int E, int BB>
__global__ __launch_bounds__(PR_THREADS) void pose_refiner_backward_kernel(const PoseRefinerArgs a) {
  using S = PrShape<E>;
  constexpr int G = BB < PR_GROUP ? BB : PR_GROUP;
  constexpr int PART = PR_WAVES * G * (S::KP > PR_W ? S::KP : PR_W);
  __shared__ float s_x[BB * S::KP], s_h1[BB * PR_W], s_h2[BB * PR_W], s_r[BB * S::KP], s_dz2[BB * PR_W], s_dz1[BB * PR_W],
      s_bias[2 * PR_W + E], s_part[PART];
  const int tid = threadIdx.x, lane = tid % WAVE, wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int B = a.B;
  PrWeights<E> w;
  pr_load_weights<E>(a, w, lane, wave);
  pr_load_inputs<E, BB>(a, s_x, s_bias, tid);
  __syncthreads();
  // ---- the forward again (nothing was kept): h1, h2 (their signs are the ReLU masks) and r
  pr_dense<BB, S::KC0, PR_NO, true>(w.w0, s_x, S::KP, s_bias, PR_W, s_h1, PR_W, lane, wave);
  __syncthreads();
  pr_dense<BB, PR_KCW, PR_NO, true>(w.w2, s_h1, PR_W, s_bias + PR_W, PR_W, s_h2, PR_W, lane, wave);
  __syncthreads();
  pr_dense<BB, PR_KCW, S::NO4, false>(w.w4, s_h2, PR_W, s_bias + 2 * PR_W, E, s_r, S::KP, lane, wave);
  __syncthreads();
  // ---- Rodrigues backward: r -> dL/dr in place (each thread reads and writes its own three entries)
  for (int t = tid; t < B * S::NJ; t += PR_THREADS) {
    const int b = t / S::NJ, j = t % S::NJ;
    float *rr = &s_r[b * S::KP + 3 * j];
    float g[9], R[9], dr[3];
#pragma unroll
    for (int k = 0; k < 9; k++) g[k] = a.dRs[(size_t)t * 9 + k];
    PrRod q;
    pr_rodrigues(rr, q, R);
    pr_rodrigues_bwd(q, g, dr);
#pragma unroll
    for (int k = 0; k < 3; k++) rr[k] = dr[k];
  }
  __syncthreads();
  // ---- last layer: dW4, db4; dz2 = (W4^T dr) where h2 > 0
  pr_wgrad<PR_KCW, S::NO4>(s_r, S::KP, s_h2, PR_W, E, PR_W, a.dw[2], a.db[2], B, lane, wave);
  pr_dense_t<BB, PR_KCW, S::NO4>(w.w4, s_r, S::KP, E, s_part, s_dz2, PR_W, PR_W, B, s_h2, PR_W, lane, wave, tid);
  // ---- W0 again for dx: keeping the forward's copy live through the two products above spills registers at E = 162; the reload
  // (an L2 hit) is issued here and waits behind the middle layer's work
  float w0[PR_NO][S::KC0];
  if (a.dx) pr_load_rows(a.w[0], PR_W, E, w0, lane, wave);
  // ---- middle layer: dW2, db2; dz1 = (W2^T dz2) where h1 > 0
  pr_wgrad<PR_KCW, PR_NO>(s_dz2, PR_W, s_h1, PR_W, PR_W, PR_W, a.dw[1], a.db[1], B, lane, wave);
  pr_dense_t<BB, PR_KCW, PR_NO>(w.w2, s_dz2, PR_W, PR_W, s_part, s_dz1, PR_W, PR_W, B, s_h1, PR_W, lane, wave, tid);
  // ---- first layer: dW0, db0; dx = W0^T dz1 straight to global memory
  pr_wgrad<S::KC0, PR_NO>(s_dz1, PR_W, s_x, S::KP, PR_W, E, a.dw[0], a.db[0], B, lane, wave);
  if (a.dx) pr_dense_t<BB, S::KC0, PR_NO>(w0, s_dz1, PR_W, PR_W, s_part, a.dx, E, E, B, nullptr, 0, lane, wave, tid);
}

static int pr_check(const char *who, int J, int B, int width, const float *x, const float *const *weights, const float *const *biases) {
  if (J != 24 && J != 55) {
    set_error("%s: J = %d; the fused pose refiner is built for J = 24 (SMPL) and 55 (SMPL-X)", who, J);
    return GSR_EINVAL;
  }
  if (width != PR_W) {
    set_error("%s: width = %d; the fused pose refiner is built for width %d", who, width, PR_W);
    return GSR_EINVAL;
  }
  if (B < 1 || B > PR_MAX_B) {
    set_error("%s: B = %d; 1 <= B <= %d pose rows", who, B, PR_MAX_B);
    return GSR_EINVAL;
  }
  if (!x || !weights || !biases) {
    set_error("%s: null argument", who);
    return GSR_EINVAL;
  }
  for (int l = 0; l < 3; l++) {
    if (!weights[l] || !biases[l]) {
      set_error("%s: layer %d: null weight or bias", who, l);
      return GSR_EINVAL;
    }
  }
  return GSR_OK;
}

template <int E, int BB>
static void pr_launch(bool backward, const PoseRefinerArgs &a, hipStream_t stream) {
  if (backward)
    hipLaunchKernelGGL((pose_refiner_backward_kernel<E, BB>), dim3(1), dim3(PR_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((pose_refiner_forward_kernel<E, BB>), dim3(1), dim3(PR_THREADS), 0, stream, a);
}

template <int E>
static void pr_launch_rows(bool backward, const PoseRefinerArgs &a, hipStream_t stream) {
  if (a.B <= 1)
    pr_launch<E, 1>(backward, a, stream);
  else if (a.B <= 2)
    pr_launch<E, 2>(backward, a, stream);
  else if (a.B <= 4)
    pr_launch<E, 4>(backward, a, stream);
  else if (a.B <= 8)
    pr_launch<E, 8>(backward, a, stream);
  else
    pr_launch<E, 16>(backward, a, stream);
}

static int pr_run(bool backward, int J, const PoseRefinerArgs &a, gsr_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (J == 24)
    pr_launch_rows<69>(backward, a, stream);
  else
    pr_launch_rows<162>(backward, a, stream);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

}  // namespace gsr

extern "C" {

int gsr_pose_refiner_forward(int J, int B, int width, const float *x, long long x_row_stride, long long x_col_stride,
                             const float *const *weights, const float *const *biases, float *Rs, gsr_stream_t stream) {
  static const char *who = "gsr_pose_refiner_forward";
  int rc = gsr::pr_check(who, J, B, width, x, weights, biases);
  if (rc != GSR_OK) return rc;
  if (!Rs) {
    gsr::set_error("%s: null argument", who);
    return GSR_EINVAL;
  }
  gsr::PoseRefinerArgs a = {};
  a.x = x, a.sx_b = x_row_stride, a.sx_e = x_col_stride, a.B = B, a.Rs = Rs;
  for (int l = 0; l < 3; l++) a.w[l] = weights[l], a.b[l] = biases[l];
  return gsr::pr_run(false, J, a, stream);
}

int gsr_pose_refiner_backward(int J, int B, int width, const float *x, long long x_row_stride, long long x_col_stride,
                              const float *const *weights, const float *const *biases, const float *dL_dRs,
                              float *const *dL_dweights, float *const *dL_dbiases, float *dL_dx, gsr_stream_t stream) {
  static const char *who = "gsr_pose_refiner_backward";
  int rc = gsr::pr_check(who, J, B, width, x, weights, biases);
  if (rc != GSR_OK) return rc;
  if (!dL_dRs || !dL_dweights || !dL_dbiases) {
    gsr::set_error("%s: null argument", who);
    return GSR_EINVAL;
  }
  gsr::PoseRefinerArgs a = {};
  a.x = x, a.sx_b = x_row_stride, a.sx_e = x_col_stride, a.B = B, a.dRs = dL_dRs, a.dx = dL_dx;
  for (int l = 0; l < 3; l++) {
    if (!dL_dweights[l] || !dL_dbiases[l]) {
      gsr::set_error("%s: layer %d: null weight or bias gradient", who, l);
      return GSR_EINVAL;
    }
    a.w[l] = weights[l], a.b[l] = biases[l], a.dw[l] = dL_dweights[l], a.db[l] = dL_dbiases[l];
  }
  return gsr::pr_run(true, J, a, stream);
}

}  // extern "C"
