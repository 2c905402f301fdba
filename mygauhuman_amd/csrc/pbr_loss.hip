// pbr_loss.hip -- the PBR-phase training loss of train.py:296-363 (iterations > 30,000) less SSIM, LPIPS and the env-map TV:
// masked L1 of the shaded image, masked TV of [albedo; roughness] under alpha, the histogram entropy of albedo and roughness
// (train.py:47-71), the per-Gaussian material smoothness over knn_3 (utils/loss_utils.py:102-124) and the roughness prior.
//
// Forward: ONE launch whose workgroups take three roles -- pixel workgroups (L1, TV, prior sums), smoothness workgroups (one sum
// per material tensor) and six entropy-column workgroups (the histogram of columns 0..2 of each [C * H][W] view and every
// coefficient its backward needs) -- then one workgroup reduces the partials in a fixed order.  No host read, no float atomics.
// Backward: one pixel kernel writes dL/d rgb, a, b and mask; the smoothness gradient gathers through the inverse knn tables.
// Semantics (denominators, empty masks, the entropy branch): include/gsr.h gsr_pbr_loss and DESIGN.md §12.
#include "gsr_common.h"

namespace gsr {

constexpr int PL_PIX_BLOCKS = 1024, PL_SM_BLOCKS = 256, PL_COLS = 6, PL_MAX_BINS = 32;
constexpr int PL_COL_STRIDE = 8 + PL_MAX_BINS;  // [taken, mu, sigma, cv, E, -, -, -, cz_0 .. cz_{bins-1}]
constexpr int PL_PART = (PL_PIX_BLOCKS + PL_SM_BLOCKS) * 8;
constexpr int PL_COL_OFF = PL_PART, PL_SCALE_OFF = PL_COL_OFF + PL_COLS * PL_COL_STRIDE;
constexpr int PL_WORKSPACE = PL_SCALE_OFF + 8;  // scales: s_l1, s_tvh, s_tvw, s_prior, s_sm0, s_sm1
constexpr float PL_EPS = 1e-6f;

// sum of v over the 256 threads of a workgroup, the same order every time; the result is valid in every thread
template <typename T>
__device__ T block_sum(T v, T *lds /* [4] */) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
  __syncthreads();  // (lds may still be read from the previous call)
  if (threadIdx.x % WAVE == 0) lds[threadIdx.x / WAVE] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__device__ inline float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__device__ void pixel_partials(const gsr_pbr_loss &l, int blk, int nblk, float *__restrict__ part) {
  const int W = l.width, H = l.height, npix = W * H;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // sum |rgb - gt|, n_b, tv_h, tv_w, sum (1 - b0), n_a
  for (int i = blk * 256 + threadIdx.x; i < npix; i += nblk * 256) {
    const int y = i / W, x = i - y * W;
    if (l.rgb && l.bound[i] == 1.f) {
#pragma unroll
      for (int c = 0; c < 3; c++)
        acc[0] += fabsf(l.rgb[c * l.rgb_stride[0] + y * l.rgb_stride[1] + x * l.rgb_stride[2]] - l.gt[(size_t)c * npix + i]);
      acc[1] += 1.f;
    }
    if (l.tv) {
      const float m = l.mask[i];
      const float mh = y + 1 < H ? m * l.mask[i + W] : 0.f, mw = x + 1 < W ? m * l.mask[i + 1] : 0.f;
      for (int ch = 0; ch < l.ca + l.cb; ch++) {
        const float *p = ch < l.ca ? l.a + (size_t)ch * npix : l.b + (size_t)(ch - l.ca) * npix;
        const float v = p[i];
        if (y + 1 < H) {
          const float d = p[i + W] - v;
          acc[2] += d * d * mh;
        }
        if (x + 1 < W) {
          const float d = p[i + 1] - v;
          acc[3] += d * d * mw;
        }
      }
    }
    if (l.prior && l.mask[i] > 0.f) {
      acc[4] += 1.f - l.b[i];
      acc[5] += 1.f;
    }
  }
  __shared__ float s[4];
  for (int t = 0; t < 6; t++) {
    const float v = block_sum(acc[t], s);
    if (threadIdx.x == 0) part[blk * 8 + t] = v;
  }
}

__device__ void smooth_partials(const gsr_pbr_loss &l, int blk, int nblk, float *__restrict__ part) {
  float acc[2] = {0.f, 0.f};
  for (int p = blk * 256 + threadIdx.x; p < l.P; p += nblk * 256) {
    const int i1 = l.k1[p], i2 = l.k2[p];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      if (!l.g[t]) continue;
      const int C = l.gc[t];
      for (int c = 0; c < C; c++) {
        const float u = l.g[t][(size_t)i1 * C + c], w = l.g[t][(size_t)i2 * C + c];
        acc[t] += fabsf(u - w) / (w + PL_EPS);
      }
    }
  }
  __shared__ float s[4];
  for (int t = 0; t < 2; t++) {
    const float v = block_sum(acc[t], s);
    if (threadIdx.x == 0) part[(PL_PIX_BLOCKS + blk) * 8 + t] = v;
  }
}

// one column (tensor t = col / 3, column j = col % 3) of gaussian_histogram / gaussian_entropy:
//   sigma = unbiased variance of the column's N values, h_k = delta / (sigma sqrt(2 pi)) sum_n exp(-z_nk^2 / 2), z = (x - c_k) / sigma;
//   S = sum h_k > 1e-6: p = h / S + 1e-6, E = -sum p log p; otherwise E = 0 and the column's gradient is 0.
// dE/dx_n = sum_k cz_k e_nk z_nk + cv (x_n - mu) with cz_k = -a_k K / sigma, cv = 2 / (N - 1) sum_k a_k dh_k/dsigma, a_k = dE/dh_k.
__device__ void entropy_column(const gsr_pbr_loss &l, int col, float *__restrict__ st) {
  const int t = col / 3, j = col % 3, W = l.width;
  const float *x = t == 0 ? l.a : l.b;
  const int N = (t == 0 ? l.ca : l.cb) * l.height;
  __shared__ double sd[4];
  __shared__ float sf[4];
  __shared__ float hs[2][PL_MAX_BINS];
  if (!l.entropy[t] || !x) {
    if (threadIdx.x < PL_COL_STRIDE) st[threadIdx.x] = 0.f;
    return;
  }
  double sum = 0.0;
  for (int r = threadIdx.x; r < N; r += 256) sum += (double)x[(size_t)r * W + j];
  const double mu = block_sum(sum, sd) / (double)N;
  double ss = 0.0;
  for (int r = threadIdx.x; r < N; r += 256) {
    const double d = (double)x[(size_t)r * W + j] - mu;
    ss += d * d;
  }
  const float sigma = (float)(block_sum(ss, sd) / (double)(N - 1));  // N = 1: 0 / 0 (torch's var is NaN there too)
  const int bins = l.bins;
  const float delta = (l.hi - l.lo) / (float)bins;
  for (int k = 0; k < bins; k++) {
    const float c = l.lo + delta * ((float)k + 0.5f);
    float e_sum = 0.f, ez2 = 0.f;
    for (int r = threadIdx.x; r < N; r += 256) {
      const float z = (x[(size_t)r * W + j] - c) / sigma;
      const float e = __expf(-0.5f * z * z);
      e_sum += e;
      ez2 += e * z * z;
    }
    e_sum = block_sum(e_sum, sf);
    ez2 = block_sum(ez2, sf);
    if (threadIdx.x == 0) hs[0][k] = e_sum, hs[1][k] = ez2;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float K = delta / (sigma * 2.5066282746310002f);
  float h[PL_MAX_BINS], S = 0.f;
  for (int k = 0; k < bins; k++) h[k] = K * hs[0][k], S += h[k];
  st[1] = (float)mu, st[2] = sigma;
  if (!(S > PL_EPS)) {  // (NaN when sigma = 0 or N = 1: the branch is not taken)
    st[0] = 0.f, st[3] = 0.f, st[4] = 0.f;
    for (int k = 0; k < bins; k++) st[8 + k] = 0.f;
    return;
  }
  float E = 0.f, gh = 0.f, g[PL_MAX_BINS];
  for (int k = 0; k < bins; k++) {
    const float p = h[k] / S + PL_EPS, lp = logf(p);
    E -= p * lp;
    g[k] = -(lp + 1.f);  // dE/dp_k
    gh += g[k] * h[k];
  }
  float D = 0.f;
  for (int k = 0; k < bins; k++) {
    const float a = (g[k] - gh / S) / S;  // dE/dh_k
    D += a * (-h[k] / sigma + K * hs[1][k] / sigma);
    st[8 + k] = -a * K / sigma;
  }
  st[0] = 1.f, st[3] = D * 2.f / (float)(N - 1), st[4] = E;
}

__global__ __launch_bounds__(256) void pbr_loss_partial_kernel(const gsr_pbr_loss l, int pix_blocks, int sm_blocks,
                                                               float *__restrict__ ws) {
  const int b = blockIdx.x;
  if (b < pix_blocks)
    pixel_partials(l, b, pix_blocks, ws);
  else if (b < pix_blocks + sm_blocks)
    smooth_partials(l, b - pix_blocks, sm_blocks, ws);
  else {
    const int col = b - pix_blocks - sm_blocks;
    entropy_column(l, col, ws + PL_COL_OFF + col * PL_COL_STRIDE);
  }
}

__global__ __launch_bounds__(256) void pbr_loss_finish_kernel(const gsr_pbr_loss l, int pix_blocks, int sm_blocks,
                                                              float *__restrict__ ws) {
  __shared__ double s[4];
  double tot[8];
  for (int t = 0; t < 6; t++) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < pix_blocks; b += 256) acc += (double)ws[b * 8 + t];
    tot[t] = block_sum(acc, s);
  }
  for (int t = 0; t < 2; t++) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < sm_blocks; b += 256) acc += (double)ws[(PL_PIX_BLOCKS + b) * 8 + t];
    tot[6 + t] = block_sum(acc, s);
  }
  if (threadIdx.x != 0) return;
  const double W = l.width, H = l.height, C = l.ca + l.cb;
  double term[5] = {0, 0, 0, 0, 0};
  float *sc = ws + PL_SCALE_OFF;
  for (int i = 0; i < 8; i++) sc[i] = 0.f;
  if (l.rgb) {
    term[0] = tot[0] / (3.0 * tot[1]);  // (n_b = 0: 0 / 0 = NaN, the mean of an empty tensor)
    sc[0] = tot[1] > 0 ? (float)(1.0 / (3.0 * tot[1])) : 0.f;
  }
  if (l.tv) {
    const double nh = C * (H - 1) * W, nw = C * H * (W - 1);
    term[1] = tot[2] / nh + tot[3] / nw;
    sc[1] = nh > 0 ? (float)(1.0 / nh) : 0.f;
    sc[2] = nw > 0 ? (float)(1.0 / nw) : 0.f;
  }
  for (int col = 0; col < PL_COLS; col++) term[2] += (double)ws[PL_COL_OFF + col * PL_COL_STRIDE + 4];
  for (int t = 0; t < 2; t++)
    if (l.g[t]) {
      const double n = (double)l.P * l.gc[t];
      term[3] += tot[6 + t] / n;
      sc[4 + t] = (float)(1.0 / n);
    }
  if (l.prior) {
    term[4] = tot[4] / tot[5];
    sc[3] = tot[5] > 0 ? (float)(1.0 / tot[5]) : 0.f;
  }
  const double w[5] = {l.w_l1, l.w_tv, l.w_entropy, l.w_smooth, l.w_prior};
  const bool on[5] = {l.rgb != nullptr, l.tv != 0, l.entropy[0] || l.entropy[1], l.g[0] || l.g[1], l.prior != 0};
  double loss = 0.0;
  for (int i = 0; i < 5; i++) {
    l.terms[i] = (float)term[i];
    if (on[i]) loss += w[i] * term[i];
  }
  l.loss[0] = (float)loss;
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pbr_loss_image_bwd_kernel(const gsr_pbr_loss l, const float *__restrict__ ws) {
  const int W = l.width, H = l.height, npix = W * H;
  const float up = l.upstream ? l.upstream[0] : 1.f;
  const float *sc = ws + PL_SCALE_OFF;
  const float g_l1 = up * l.w_l1 * sc[0], g_h = 2.f * up * l.w_tv * sc[1], g_w = 2.f * up * l.w_tv * sc[2];
  const float g_prior = -up * l.w_prior * sc[3], g_ent = up * l.w_entropy;
  const float delta = (l.hi - l.lo) / (float)l.bins;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    if (l.d_rgb) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const size_t o = c * l.rgb_stride[0] + y * l.rgb_stride[1] + x * l.rgb_stride[2];
        l.d_rgb[o] = (l.rgb && l.bound[i] == 1.f) ? g_l1 * sgn(l.rgb[o] - l.gt[(size_t)c * npix + i]) : 0.f;
      }
    }
    float m = 0.f, mu = 0.f, md = 0.f, ml = 0.f, mr = 0.f;
    if (l.tv) {
      m = l.mask[i];
      mu = y > 0 ? l.mask[i - W] : 0.f, md = y + 1 < H ? l.mask[i + W] : 0.f;
      ml = x > 0 ? l.mask[i - 1] : 0.f, mr = x + 1 < W ? l.mask[i + 1] : 0.f;
    }
    float gm = 0.f;
    for (int ch = 0; ch < l.ca + l.cb; ch++) {
      const bool in_a = ch < l.ca;
      const int t = in_a ? 0 : 1, lc = in_a ? ch : ch - l.ca;
      float *dst = in_a ? l.d_a : l.d_b;
      if (!dst && !(l.tv && l.d_mask)) continue;
      const float *p = (in_a ? l.a : l.b) + (size_t)lc * npix;
      const float v = p[i];
      float g = 0.f;
      if (l.tv) {
        if (y > 0) {
          const float d = v - p[i - W];
          g += g_h * d * mu * m;
          gm += 0.5f * g_h * d * d * mu;
        }
        if (y + 1 < H) {
          const float d = p[i + W] - v;
          g -= g_h * d * m * md;
          gm += 0.5f * g_h * d * d * md;
        }
        if (x > 0) {
          const float d = v - p[i - 1];
          g += g_w * d * ml * m;
          gm += 0.5f * g_w * d * d * ml;
        }
        if (x + 1 < W) {
          const float d = p[i + 1] - v;
          g -= g_w * d * m * mr;
          gm += 0.5f * g_w * d * d * mr;
        }
      }
      if (x < 3 && l.entropy[t]) {
        const float *st = ws + PL_COL_OFF + (t * 3 + x) * PL_COL_STRIDE;
        if (st[0] != 0.f) {
          const float sigma = st[2];
          float ge = st[3] * (v - st[1]);
          for (int k = 0; k < l.bins; k++) {
            const float z = (v - (l.lo + delta * ((float)k + 0.5f))) / sigma;
            ge += st[8 + k] * __expf(-0.5f * z * z) * z;
          }
          g += g_ent * ge;
        }
      }
      if (!in_a && lc == 0 && l.prior && l.mask[i] > 0.f) g += g_prior;
      if (dst) dst[(size_t)lc * npix + i] = g;
    }
    if (l.d_mask) l.d_mask[i] = gm;
  }
}

// dL/dg[t][i][c] = sum over entries p with k1[p] = i of sign(d)/q  +  over p with k2[p] = i of -sign(d)/q - |d|/q^2,
// d = g[k1[p]][c] - g[k2[p]][c], q = g[k2[p]][c] + 1e-6: a gather, each row written once
__global__ __launch_bounds__(256) void pbr_loss_smooth_bwd_kernel(const gsr_pbr_loss l, const float *__restrict__ ws) {
  const float up = l.upstream ? l.upstream[0] : 1.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < l.P; i += gridDim.x * 256) {
    const int b1 = l.inv_off[0][i], e1 = l.inv_off[0][i + 1], b2 = l.inv_off[1][i], e2 = l.inv_off[1][i + 1];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      if (!l.d_g[t]) continue;
      const float s = up * l.w_smooth * ws[PL_SCALE_OFF + 4 + t];
      const float *g = l.g[t];
      const int C = l.gc[t];
      for (int c = 0; c < C; c++) {
        const float own = g[(size_t)i * C + c];
        float acc = 0.f;
        for (int e = b1; e < e1; e++) {  // i is k1 of entry p: the numerator's first operand
          const float w = g[(size_t)l.k2[l.inv_idx[0][e]] * C + c];
          acc += sgn(own - w) / (w + PL_EPS);
        }
        for (int e = b2; e < e2; e++) {  // i is k2 of entry p: the numerator's second operand and the denominator
          const float u = g[(size_t)l.k1[l.inv_idx[1][e]] * C + c], q = own + PL_EPS, d = u - own;
          acc += -sgn(d) / q - fabsf(d) / (q * q);
        }
        l.d_g[t][(size_t)i * C + c] = s * acc;
      }
    }
  }
}

static bool smooth_on(const gsr_pbr_loss *l) { return l->g[0] || l->g[1]; }

static const char *validate(const gsr_pbr_loss *l) {
  if (l->width <= 0 || l->height <= 0) return "width and height must be positive";
  if ((long long)l->width * l->height >= (1ll << 31) / 4) return "image too large";
  if (l->rgb && (!l->gt || !l->bound)) return "the L1 term needs rgb, gt and bound";
  if (l->a && l->ca <= 0) return "ca must be positive when a is given";
  if (l->b && l->cb <= 0) return "cb must be positive when b is given";
  if (!l->a && l->ca) return "ca must be 0 without a";
  if (!l->b && l->cb) return "cb must be 0 without b";
  if (l->tv && (!l->mask || !l->a)) return "the TV term needs a and mask";
  if (l->prior && (!l->mask || !l->b)) return "the prior term needs b and mask";
  if ((l->entropy[0] && !l->a) || (l->entropy[1] && !l->b)) return "an entropy term needs its image";
  if ((l->entropy[0] || l->entropy[1]) && (l->width < 3 || l->bins < 1 || l->bins > PL_MAX_BINS))
    return "the entropy term needs width >= 3 and 1..32 bins";
  if (smooth_on(l)) {
    if (l->P <= 0 || !l->k1 || !l->k2) return "the smoothness term needs P > 0, k1 and k2";
    for (int t = 0; t < 2; t++)
      if (l->g[t] && l->gc[t] <= 0) return "gc must be positive for a given g";
  }
  if (!l->loss || !l->terms) return "loss and terms are required";
  return nullptr;
}

static int pix_blocks(const gsr_pbr_loss *l) {
  if (!l->rgb && !l->tv && !l->prior) return 0;
  const int n = (l->width * l->height + 255) / 256;
  return n < PL_PIX_BLOCKS ? n : PL_PIX_BLOCKS;
}
static int sm_blocks(const gsr_pbr_loss *l) {
  if (!smooth_on(l)) return 0;
  const int n = (l->P + 255) / 256;
  return n < PL_SM_BLOCKS ? n : PL_SM_BLOCKS;
}

}  // namespace gsr

extern "C" size_t gsr_pbr_loss_workspace_floats(void) { return (size_t)gsr::PL_WORKSPACE; }

extern "C" int gsr_pbr_loss_forward(const gsr_pbr_loss *l, float *workspace, gsr_stream_t stream_) {
  const char *bad = l ? gsr::validate(l) : "loss is null";
  if (!bad && !workspace) bad = "workspace is null";
  if (bad) {
    gsr::set_error("gsr_pbr_loss_forward: %s", bad);
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int pb = gsr::pix_blocks(l), sb = gsr::sm_blocks(l);
  hipLaunchKernelGGL(gsr::pbr_loss_partial_kernel, dim3(pb + sb + gsr::PL_COLS), dim3(256), 0, stream, *l, pb, sb, workspace);
  hipLaunchKernelGGL(gsr::pbr_loss_finish_kernel, dim3(1), dim3(256), 0, stream, *l, pb, sb, workspace);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

extern "C" int gsr_pbr_loss_backward(const gsr_pbr_loss *l, const float *workspace, gsr_stream_t stream_) {
  const char *bad = l ? gsr::validate(l) : "loss is null";
  if (!bad && !workspace) bad = "workspace is null";
  if (!bad && l->d_rgb && !l->rgb) bad = "d_rgb needs rgb";
  if (!bad && ((l->d_a && !l->a) || (l->d_b && !l->b))) bad = "d_a / d_b need their images";
  if (!bad && l->d_mask && !l->mask) bad = "d_mask needs mask";
  if (!bad && ((l->d_g[0] && !l->g[0]) || (l->d_g[1] && !l->g[1]))) bad = "d_g needs g";
  if (!bad && (l->d_g[0] || l->d_g[1]) && (!l->inv_off[0] || !l->inv_off[1] || !l->inv_idx[0] || !l->inv_idx[1]))
    bad = "the smoothness gradient needs both inverse tables";
  if (bad) {
    gsr::set_error("gsr_pbr_loss_backward: %s", bad);
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (l->d_rgb || l->d_a || l->d_b || l->d_mask) {
    const int n = (l->width * l->height + 255) / 256;
    hipLaunchKernelGGL(gsr::pbr_loss_image_bwd_kernel, dim3(n < 2048 ? n : 2048), dim3(256), 0, stream, *l, workspace);
  }
  if (l->d_g[0] || l->d_g[1]) {
    const int n = (l->P + 255) / 256;
    hipLaunchKernelGGL(gsr::pbr_loss_smooth_bwd_kernel, dim3(n < 2048 ? n : 2048), dim3(256), 0, stream, *l, workspace);
  }
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}
