// eval.hip -- the evaluation "view finish" of render.py:186-350 (and of training_report, train.py:480-540) without a host read.
//
// What the reference does to a view's images after render() / pbr_shading return is ~60 torch launches and ~22 blocking reads:
//   eleven  img.permute(1,2,0)[bound_mask[0]==0] = 0 if background.sum().item() == 0 else 1     (index_put + .item())
//   thirteen torch.clamp(img, 0, 1), thirteen save_image quantisations (mul 255, add 0.5, clamp, uint8, permute),
//   psnr() and ssim() of the finished pair as five grouped conv2d calls and ~15 elementwise kernels.
// Here, three launches:
//   eval_finish_kernel   one pass over the pixels for up to 16 image slots: flip_z, fill under the bound mask (the fill value from the
//                        DEVICE background), clamp, the float result in place or to a second buffer, the 8-bit image, and the
//                        per-channel squared differences of the metric pair reduced to one partial per workgroup;
//   eval_ssim_kernel     ssim.hip's forward tile kernel on the finished pair, with no map written: one partial per tile;
//   eval_metrics_kernel  one workgroup: the partials in a fixed order (double) -> table[counter] = (psnr, ssim), counter + 1.
// No atomics, no memset, nothing carried between calls: two calls on the same inputs write the same bits.
// Built with -ffp-contract=off: x * 255 + 0.5 and n * 2 - 1 are two roundings in torch and must be two here.
#include <climits>

#include "gsr_common.h"
#include "ssim_window.h"

namespace gsr {

constexpr int EV_THREADS = 256, EV_PX = 4;  // a thread owns EV_PX consecutive pixels of one row
constexpr int EV_WAVES = EV_THREADS / WAVE;

__device__ inline float ev_clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }  // NaN fails both tests: stays
__device__ inline unsigned ev_quant(float x) {
  const float q = fminf(fmaxf(x * 255.f + 0.5f, 0.f), 255.f);
  return (unsigned)(int)q;
}

// One slot of one thread's pixels.  `s` is indexed with a constant by the caller (a runtime index into the by-value struct would put
// it into scratch memory).  fin[c][j]: the finished values, returned for the metric pair.
__device__ __forceinline__ void finish_slot(const gsr_eval_slot &s, int W, int y, int x4, int n, const bool inside[EV_PX], float fill,
                                            float fin[3][EV_PX]) {
  const int ch = s.channels;
  const long long s0 = s.stride[0], s1 = s.stride[1], s2 = s.stride[2];
  float *out = s.dst ? s.dst : s.src;
  // 16-byte accesses where the four pixels are four consecutive aligned floats (wave-uniform)
  const bool vec = n == EV_PX && s2 == 1 && W % 4 == 0 && s1 % 4 == 0 && s0 % 4 == 0 && reinterpret_cast<uintptr_t>(s.src) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const long long row = (long long)y * s1 + (long long)x4 * s2;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c < ch) {
      const float *p = s.src + c * s0 + row;
      if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        fin[c][0] = q.x, fin[c][1] = q.y, fin[c][2] = q.z, fin[c][3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < EV_PX; j++) fin[c][j] = j < n ? p[j * s2] : 0.f;
      }
    }
  }
  if (s.flags & GSR_EVAL_FLIP_Z) {  // render.py:191-193, the same operations in the same order on every channel
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int j = 0; j < EV_PX; j++) {
        float t = fin[c][j] * 2.f - 1.f;
        if (c == 2) t = -t;
        fin[c][j] = (t + 1.f) / 2.f;
      }
  }
  const bool fill_on = (s.flags & GSR_EVAL_FILL) != 0;
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int j = 0; j < EV_PX; j++) {
      float t = fin[c][j];
      if (fill_on && !inside[j]) t = fill;
      fin[c][j] = ev_clamp01(t);
    }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c < ch) {
      float *p = out + c * s0 + row;
      if (vec) {
        *reinterpret_cast<float4 *>(p) = make_float4(fin[c][0], fin[c][1], fin[c][2], fin[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < EV_PX; j++)
          if (j < n) p[j * s2] = fin[c][j];
      }
    }
  }
  if (s.u8) {
    unsigned char *o = s.u8 + ((size_t)y * W + x4) * ch;
    // whole dwords where every group of the image starts on one (W % 4 == 0 makes every row offset a multiple of 4 bytes)
    const bool dwords = n == EV_PX && W % 4 == 0 && reinterpret_cast<uintptr_t>(s.u8) % 4 == 0;
    if (ch == 3) {
      unsigned b[12];
#pragma unroll
      for (int j = 0; j < EV_PX; j++)
#pragma unroll
        for (int c = 0; c < 3; c++) b[j * 3 + c] = ev_quant(fin[c][j]);
      if (dwords) {
        unsigned *o32 = reinterpret_cast<unsigned *>(o);
#pragma unroll
        for (int d = 0; d < 3; d++) o32[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < 12; i++)
          if (i < n * 3) o[i] = (unsigned char)b[i];
      }
    } else {
      unsigned b[4];
#pragma unroll
      for (int j = 0; j < EV_PX; j++) b[j] = ev_quant(fin[0][j]);
      if (dwords) {
        *reinterpret_cast<unsigned *>(o) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < EV_PX; j++)
          if (j < n) o[j] = (unsigned char)b[j];
      }
    }
  }
}

__global__ __launch_bounds__(EV_THREADS) void eval_finish_kernel(const gsr_eval_view v, double *__restrict__ sse_partials) {
  __shared__ double red[EV_WAVES][3];
  const int H = v.height, W = v.width;
  const int groups_x = (W + EV_PX - 1) / EV_PX;
  const long long gid = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
  const bool active = gid < (long long)H * groups_x;
  const int y = active ? (int)(gid / groups_x) : 0, x4 = active ? (int)(gid - (long long)y * groups_x) * EV_PX : 0;
  const int n = active ? min(EV_PX, W - x4) : 0;
  double sse[3] = {0.0, 0.0, 0.0};
  if (active) {
    bool inside[EV_PX] = {true, true, true, true};
    float fill = 0.f;
    if (v.mask) {
      const size_t m0 = (size_t)y * W + x4;
#pragma unroll
      for (int j = 0; j < EV_PX; j++)
        if (j < n)
          inside[j] = v.mask_dtype == GSR_MASK_F32 ? static_cast<const float *>(v.mask)[m0 + j] != 0.f
                                                   : static_cast<const unsigned char *>(v.mask)[m0 + j] != 0;
      fill = (v.background[0] + v.background[1]) + v.background[2] == 0.f ? 0.f : 1.f;  // background.sum().item() == 0
    }
    float mi[3][EV_PX] = {}, mg[3][EV_PX] = {};
#pragma unroll
    for (int k = 0; k < GSR_EVAL_MAX_SLOTS; k++) {
      if (k < v.slots) {
        float fin[3][EV_PX] = {};
        finish_slot(v.slot[k], W, y, x4, n, inside, fill, fin);
        if (k == v.metric_image) {
#pragma unroll
          for (int c = 0; c < 3; c++)
#pragma unroll
            for (int j = 0; j < EV_PX; j++) mi[c][j] = fin[c][j];
        }
        if (k == v.metric_gt) {
#pragma unroll
          for (int c = 0; c < 3; c++)
#pragma unroll
            for (int j = 0; j < EV_PX; j++) mg[c][j] = fin[c][j];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int j = 0; j < EV_PX; j++)
        if (j < n) {
          const double d = (double)(mi[c][j] - mg[c][j]);  // the float32 difference, as (img1 - img2) is formed there
          sse[c] += d * d;
        }
  }
  if (v.metric_image < 0) return;  // (uniform)
  // wave fold, one LDS hop, one store per workgroup and channel; the same order every time
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sse[c] += __shfl_xor(sse[c], d, WAVE);
  if (threadIdx.x % WAVE == 0)
#pragma unroll
    for (int c = 0; c < 3; c++) red[threadIdx.x / WAVE][c] = sse[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int w = 0; w < EV_WAVES; w++) t += red[w][threadIdx.x];
    sse_partials[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

// ssim_forward_kernel (ssim.hip) on two strided images, forward only: nothing but the tile's sum leaves the workgroup
struct EvImage {
  const float *p;
  long long s0, s1, s2;
};

__global__ __launch_bounds__(SS_T *SS_T) void eval_ssim_kernel(int H, int W, EvImage img1, EvImage img2, SsimWindow win,
                                                               float *__restrict__ partials) {
  __shared__ float s1[SS_IN][SS_IN + 1], s2[SS_IN][SS_IN + 1];
  __shared__ float h[5][SS_IN][SS_T + 1];  // horizontally filtered rows: x, y, xx, yy, xy
  __shared__ float red[SS_T * SS_T];
  const float *p1 = img1.p + blockIdx.z * img1.s0, *p2 = img2.p + blockIdx.z * img2.s0;
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const int t = threadIdx.y * SS_T + threadIdx.x;
  for (int e = t; e < SS_IN * SS_IN; e += SS_T * SS_T) {
    const int ly = e / SS_IN, lx = e % SS_IN;
    const int gx = x0 + lx - SS_R, gy = y0 + ly - SS_R;
    const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
    s1[ly][lx] = in ? p1[gy * img1.s1 + gx * img1.s2] : 0.f;
    s2[ly][lx] = in ? p2[gy * img2.s1 + gx * img2.s2] : 0.f;
  }
  __syncthreads();
  for (int e = t; e < SS_IN * SS_T; e += SS_T * SS_T) {
    const int ly = e / SS_T, lx = e % SS_T;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float u = s1[ly][lx + k], w = s2[ly][lx + k], wk = win.w[k];
      a += wk * u;
      b += wk * w;
      aa += wk * (u * u);
      bb += wk * (w * w);
      ab += wk * (u * w);
    }
    h[0][ly][lx] = a;
    h[1][ly][lx] = b;
    h[2][ly][lx] = aa;
    h[3][ly][lx] = bb;
    h[4][ly][lx] = ab;
  }
  __syncthreads();
  const int px = x0 + threadIdx.x, py = y0 + threadIdx.y;
  float f = 0.f;
  if (px < W && py < H) {
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float wk = win.w[k];
      mu1 += wk * h[0][threadIdx.y + k][threadIdx.x];
      mu2 += wk * h[1][threadIdx.y + k][threadIdx.x];
      e11 += wk * h[2][threadIdx.y + k][threadIdx.x];
      e22 += wk * h[3][threadIdx.y + k][threadIdx.x];
      e12 += wk * h[4][threadIdx.y + k][threadIdx.x];
    }
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float sg1 = e11 - mu1_sq, sg2 = e22 - mu2_sq, sg12 = e12 - mu12;
    f = ((2.f * mu12 + C1) * (2.f * sg12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sg1 + sg2 + C2));
  }
  // the tile's sum, the same order every time (pixels outside the frame add 0): folded by the first wave alone
  red[t] = f;
  __syncthreads();
  if (t >= WAVE) return;
  f = (red[t] + red[t + WAVE]) + (red[t + 2 * WAVE] + red[t + 3 * WAVE]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) f += __shfl_xor(f, d, WAVE);
  if (t == 0) partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = f;
}

// fold over the workgroup; valid in thread 0
__device__ inline double ev_fold(double a, double *lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, WAVE);
  __syncthreads();  // (lds is reused from one fold to the next)
  if (threadIdx.x % WAVE == 0) lds[threadIdx.x / WAVE] = a;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < EV_WAVES; w++) t += lds[w];
  return t;
}

__global__ __launch_bounds__(EV_THREADS) void eval_metrics_kernel(int H, int W, int nblk, const double *__restrict__ sse_partials,
                                                                  int ntile, const float *__restrict__ ssim_partials,
                                                                  int *__restrict__ counter, double *__restrict__ table, int capacity,
                                                                  int *__restrict__ overflow) {
  __shared__ double lds[EV_WAVES];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += EV_THREADS)
#pragma unroll
    for (int c = 0; c < 3; c++) acc[c] += sse_partials[(size_t)i * 3 + c];
  for (int i = threadIdx.x; i < ntile; i += EV_THREADS) acc[3] += (double)ssim_partials[i];
#pragma unroll
  for (int c = 0; c < 4; c++) acc[c] = ev_fold(acc[c], lds);
  if (threadIdx.x != 0) return;
  const double pixels = (double)H * (double)W;
  double psnr = 0.0;
#pragma unroll
  for (int c = 0; c < 3; c++) psnr += 20.0 * log10(1.0 / sqrt(acc[c] / pixels));  // mse == 0: 1 / 0 = inf, log10(inf) = inf
  const int row = counter[0];
  if (row >= 0 && row < capacity) {
    table[2 * (size_t)row] = psnr / 3.0;
    table[2 * (size_t)row + 1] = acc[3] / (3.0 * pixels);
  } else {
    overflow[0] = 1;
  }
  if (row < INT_MAX) counter[0] = row + 1;
}

static int finish_blocks(int H, int W) {
  const long long groups = (long long)H * ((W + EV_PX - 1) / EV_PX);
  return (int)((groups + EV_THREADS - 1) / EV_THREADS);
}
static int ssim_tiles(int H, int W) { return 3 * ((H + SS_T - 1) / SS_T) * ((W + SS_T - 1) / SS_T); }

static const char *validate(const gsr_eval_view *v, const float *workspace) {
  if (v->slots < 1 || v->slots > GSR_EVAL_MAX_SLOTS) return "1..16 slots";
  if (v->height <= 0 || v->width <= 0) return "height and width must be positive";
  if ((long long)v->height * v->width >= (1ll << 31)) return "image too large";
  bool any_fill = false;
  for (int k = 0; k < v->slots; k++) {
    const gsr_eval_slot &s = v->slot[k];
    if (!s.src) return "a slot's src is null";
    if (s.channels != 1 && s.channels != 3) return "channels must be 1 or 3";
    if (s.flags & ~(GSR_EVAL_FILL | GSR_EVAL_FLIP_Z)) return "unknown slot flags";
    if ((s.flags & GSR_EVAL_FLIP_Z) && s.channels != 3) return "GSR_EVAL_FLIP_Z needs 3 channels";
    for (int d = 0; d < 3; d++)
      if (s.stride[d] < 0) return "strides must not be negative";
    any_fill |= (s.flags & GSR_EVAL_FILL) != 0;
  }
  if (any_fill && (!v->mask || !v->background)) return "mask and background are required by GSR_EVAL_FILL";
  if (v->mask && v->mask_dtype != GSR_MASK_F32 && v->mask_dtype != GSR_MASK_U8) return "mask_dtype must be GSR_MASK_F32 or GSR_MASK_U8";
  if (v->mask && !v->background) return "background is null";
  if (v->metric_image == -1 && v->metric_gt == -1) return nullptr;
  if (v->metric_image < 0 || v->metric_image >= v->slots || v->metric_gt < 0 || v->metric_gt >= v->slots ||
      v->metric_image == v->metric_gt)
    return "metric pair must name two different slots (or be -1, -1)";
  if (v->slot[v->metric_image].channels != 3 || v->slot[v->metric_gt].channels != 3) return "metric pair must be two 3-channel slots";
  if (!v->counter || !v->table || !v->overflow) return "counter, table and overflow are required by the metric pair";
  if (v->capacity <= 0) return "capacity must be positive";
  if (!workspace) return "workspace is null";
  if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return "workspace must be 8-byte aligned";
  return nullptr;
}

}  // namespace gsr

extern "C" {

size_t gsr_eval_workspace_floats(int height, int width) {
  if (height <= 0 || width <= 0 || (long long)height * width >= (1ll << 31)) return 0;
  return 2 * 3 * (size_t)gsr::finish_blocks(height, width) + (size_t)gsr::ssim_tiles(height, width);
}

int gsr_eval_view_finish(const gsr_eval_view *view, float *workspace, gsr_stream_t stream_) {
  using namespace gsr;
  const char *bad = view ? validate(view, workspace) : "view is null";
  if (bad) {
    set_error("gsr_eval_view_finish: %s", bad);
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int H = view->height, W = view->width, nblk = finish_blocks(H, W);
  double *sse = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(nblk), dim3(EV_THREADS), 0, stream, *view, sse);
  if (view->metric_image >= 0) {
    float *tiles = workspace + 2 * 3 * (size_t)nblk;
    const gsr_eval_slot &a = view->slot[view->metric_image], &b = view->slot[view->metric_gt];
    const EvImage i1 = {a.dst ? a.dst : a.src, a.stride[0], a.stride[1], a.stride[2]};
    const EvImage i2 = {b.dst ? b.dst : b.src, b.stride[0], b.stride[1], b.stride[2]};
    const dim3 grid((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, 3);
    hipLaunchKernelGGL(eval_ssim_kernel, grid, dim3(SS_T, SS_T), 0, stream, H, W, i1, i2, make_window(), tiles);
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(1), dim3(EV_THREADS), 0, stream, H, W, nblk, sse, ssim_tiles(H, W), tiles,
                       view->counter, view->table, view->capacity, view->overflow);
  }
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

}  // extern "C"
