// ssim_crop.hip -- the SSIM term of train.py:269-281 and :318-321 without its host read:
//     x, y, w, h = cv2.boundingRect(bound_mask[0].cpu().numpy().astype(np.uint8));  ssim(image[:, y:y+h, x:x+w][None], gt[...])
//
// bounding_rect: the rectangle of a mask's nonzero pixels into DEVICE memory.  One pass of 16-byte loads over the mask (each thread
//   keeps min / max column and row of the nonzero pixels it saw), one box per workgroup into the workspace, then one workgroup folds
//   the boxes.  Integer min / max only: exact whatever the order, no atomics, no state carried between calls.
// ssim_crop: ssim() pads with zeros, so SSIM of the crop is the full-frame SSIM map of the two images zeroed outside the rectangle,
//   averaged over the rectangle.  The kernels are ssim.hip's (same window, same separable 26 x 26 LDS staging, same A / B / C maps)
//   launched over the whole frame, with the frame bounds test replaced by a test against the rectangle read from device memory:
//   a workgroup whose tile misses the rectangle leaves before it stages anything.  The mean is fused: one partial sum per workgroup,
//   added in a fixed order (in double) by one workgroup per group.  The backward divides the upstream scalar by planes * w * h on
//   the device and writes zeros outside the rectangle itself.  Up to four (img1, img2) groups share a launch (image and normal).
#include <climits>

#include "gsr_common.h"
#include "ssim_window.h"

namespace gsr {

// ---- bounding rectangle -----------------------------------------------------------------------------------------------------------
constexpr int BR_BLOCKS = 1024, BR_THREADS = 256;

struct Box {
  int x0, y0, x1, y1;  // smallest / largest column and row seen; x1 < 0: nothing seen
};

__device__ inline void box_add(Box &b, int x, int y) {
  b.x0 = min(b.x0, x), b.y0 = min(b.y0, y), b.x1 = max(b.x1, x), b.y1 = max(b.y1, y);
}

// fold over the 256 threads of a workgroup; valid in thread 0
__device__ inline Box box_fold(Box b, int (*lds)[4]) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    b.x0 = min(b.x0, __shfl_xor(b.x0, d, WAVE)), b.y0 = min(b.y0, __shfl_xor(b.y0, d, WAVE));
    b.x1 = max(b.x1, __shfl_xor(b.x1, d, WAVE)), b.y1 = max(b.y1, __shfl_xor(b.y1, d, WAVE));
  }
  if (threadIdx.x % WAVE == 0) {
    int *o = lds[threadIdx.x / WAVE];
    o[0] = b.x0, o[1] = b.y0, o[2] = b.x1, o[3] = b.y1;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < BR_THREADS / WAVE; w++) {
      b.x0 = min(b.x0, lds[w][0]), b.y0 = min(b.y0, lds[w][1]);
      b.x1 = max(b.x1, lds[w][2]), b.y1 = max(b.y1, lds[w][3]);
    }
  return b;
}

// V = elements per 16-byte load (1: the mask pointer is not 16-byte aligned, element loads)
template <typename T, int V>
__global__ __launch_bounds__(BR_THREADS) void bounding_rect_partial_kernel(int H, int W, const T *__restrict__ mask,
                                                                           int *__restrict__ ws) {
  __shared__ int lds[BR_THREADS / WAVE][4];
  const int n = H * W, nvec = n / V;
  Box b = {INT_MAX, INT_MAX, -1, -1};
  for (int v = blockIdx.x * BR_THREADS + threadIdx.x; v < nvec; v += gridDim.x * BR_THREADS) {
    union {
      uint4 q;
      T e[V > 1 ? V : 16 / sizeof(T)];
    } u;
    if constexpr (V > 1)
      u.q = reinterpret_cast<const uint4 *>(mask)[v];
    else
      u.e[0] = mask[v];
    const int i = v * V;
    int y = i / W, x = i - y * W;
#pragma unroll
    for (int k = 0; k < V; k++) {
      if (u.e[k] != (T)0) box_add(b, x, y);
      if (++x == W) x = 0, y++;
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < n - nvec * V) {  // the last n % V elements
    const int i = nvec * V + threadIdx.x;
    if (mask[i] != (T)0) box_add(b, i % W, i / W);
  }
  b = box_fold(b, lds);
  if (threadIdx.x == 0) {
    int *o = ws + blockIdx.x * 4;
    o[0] = b.x0, o[1] = b.y0, o[2] = b.x1, o[3] = b.y1;
  }
}

__global__ __launch_bounds__(BR_THREADS) void bounding_rect_finish_kernel(int nblk, const int *__restrict__ ws,
                                                                          int *__restrict__ rect) {
  __shared__ int lds[BR_THREADS / WAVE][4];
  Box b = {INT_MAX, INT_MAX, -1, -1};
  for (int k = threadIdx.x; k < nblk; k += BR_THREADS) {
    const int *p = ws + k * 4;
    b.x0 = min(b.x0, p[0]), b.y0 = min(b.y0, p[1]), b.x1 = max(b.x1, p[2]), b.y1 = max(b.y1, p[3]);
  }
  b = box_fold(b, lds);
  if (threadIdx.x == 0) {
    const bool any = b.x1 >= 0;
    rect[0] = any ? b.x0 : 0;
    rect[1] = any ? b.y0 : 0;
    rect[2] = any ? b.x1 - b.x0 + 1 : 0;
    rect[3] = any ? b.y1 - b.y0 + 1 : 0;
  }
}

static int bounding_rect_blocks(int n, int per_thread) {
  const long long v = ((long long)n / per_thread + BR_THREADS - 1) / BR_THREADS;
  return v < 1 ? 1 : (v > BR_BLOCKS ? BR_BLOCKS : (int)v);
}

// ---- SSIM on the rectangle --------------------------------------------------------------------------------------------------------
constexpr int SC_G = GSR_SSIM_CROP_MAX_GROUPS;

struct CropRect {
  int x0, y0, x1, y1;  // [x0, x1) x [y0, y1), inside the frame; x1 <= x0 or y1 <= y0: empty
};

// the same address in every lane: scalar loads, once per workgroup
__device__ inline CropRect load_rect(const int *__restrict__ rect, int H, int W) {
  const long long x = rect[0], y = rect[1], w = rect[2], h = rect[3];
  CropRect r;
  r.x0 = (int)max(x, 0ll), r.y0 = (int)max(y, 0ll);
  r.x1 = (int)min(x + max(w, 0ll), (long long)W), r.y1 = (int)min(y + max(h, 0ll), (long long)H);
  return r;
}

__device__ inline bool rect_empty(const CropRect &r) { return r.x1 <= r.x0 || r.y1 <= r.y0; }
__device__ inline bool in_rect(const CropRect &r, int x, int y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }
__device__ inline bool tile_misses(const CropRect &r, int x0, int y0) {
  return rect_empty(r) || x0 >= r.x1 || x0 + SS_T <= r.x0 || y0 >= r.y1 || y0 + SS_T <= r.y0;
}

// the group a plane of the launch belongs to, picked with constant indices (a runtime index into the by-value struct would put
// it into scratch memory)
struct CropGroup {
  int plane, planes;  // plane within the group; planes < 0: no group (cannot happen for a valid launch)
  const float *img1, *img2;
  int s0, s1, s2;  // img1's element strides (the host checked that every offset fits in 31 bits)
  float *dA, *dB, *dC, *d_img1;
  const float *upstream;
};

__device__ inline CropGroup pick_group(const gsr_ssim_crop &c, int z) {
  CropGroup g = {};
  g.planes = -1;
  int first = 0;
#pragma unroll
  for (int k = 0; k < SC_G; k++) {
    if (k < c.groups) {
      if (z >= first && z < first + c.planes[k]) {
        g.plane = z - first, g.planes = c.planes[k];
        g.img1 = c.img1[k], g.img2 = c.img2[k];
        g.s0 = (int)c.img1_stride[k][0], g.s1 = (int)c.img1_stride[k][1], g.s2 = (int)c.img1_stride[k][2];
        g.dA = c.dA[k], g.dB = c.dB[k], g.dC = c.dC[k], g.d_img1 = c.d_img1[k];
        g.upstream = c.upstream[k];
      }
      first += c.planes[k];
    }
  }
  return g;
}

__global__ __launch_bounds__(SS_T *SS_T) void ssim_crop_forward_kernel(const gsr_ssim_crop c, SsimWindow win,
                                                                       float *__restrict__ partials) {
  __shared__ float s1[SS_IN][SS_IN + 1], s2[SS_IN][SS_IN + 1];
  __shared__ float h[5][SS_IN][SS_T + 1];  // horizontally filtered rows: x, y, xx, yy, xy
  __shared__ float red[SS_T * SS_T];
  const int H = c.height, W = c.width;
  const CropRect r = load_rect(c.rect, H, W);
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  if (tile_misses(r, x0, y0)) return;  // (its partial is never read: the final pass walks the tiles of the rectangle only)
  const CropGroup g = pick_group(c, blockIdx.z);
  if (g.planes < 0) return;
  const size_t plane = (size_t)H * W;
  const float *p1 = g.img1 + (size_t)g.plane * g.s0, *p2 = g.img2 + g.plane * plane;
  const int t = threadIdx.y * SS_T + threadIdx.x;
  for (int e = t; e < SS_IN * SS_IN; e += SS_T * SS_T) {
    const int ly = e / SS_IN, lx = e % SS_IN;
    const int gx = x0 + lx - SS_R, gy = y0 + ly - SS_R;
    const bool in = in_rect(r, gx, gy);
    s1[ly][lx] = in ? p1[gy * g.s1 + gx * g.s2] : 0.f;
    s2[ly][lx] = in ? p2[gy * W + gx] : 0.f;
  }
  __syncthreads();
  for (int e = t; e < SS_IN * SS_T; e += SS_T * SS_T) {
    const int ly = e / SS_T, lx = e % SS_T;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float u = s1[ly][lx + k], v = s2[ly][lx + k], wk = win.w[k];
      a += wk * u;
      b += wk * v;
      aa += wk * (u * u);
      bb += wk * (v * v);
      ab += wk * (u * v);
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
  if (in_rect(r, px, py)) {
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
    const float a = 2.f * mu12 + C1, b = 2.f * sg12 + C2, cc = mu1_sq + mu2_sq + C1, d = sg1 + sg2 + C2;
    f = (a * b) / (cc * d);
    if (g.dA) {
      const size_t o = g.plane * plane + (size_t)py * W + px;
      const float df_dmu1 = (2.f * mu2 * b) / (cc * d) - f * (2.f * mu1) / cc;
      const float df_ds1 = -f / d;
      const float df_ds12 = (2.f * a) / (cc * d);
      g.dA[o] = df_dmu1 - 2.f * mu1 * df_ds1 - mu2 * df_ds12;
      g.dB[o] = df_ds1;
      g.dC[o] = df_ds12;
    }
  }
  // the tile's sum, the same order every time (pixels outside the rectangle add 0): folded by the first wave alone
  red[t] = f;
  __syncthreads();
  if (t >= WAVE) return;
  f = (red[t] + red[t + WAVE]) + (red[t + 2 * WAVE] + red[t + 3 * WAVE]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) f += __shfl_xor(f, d, WAVE);
  if (t == 0) partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = f;
}

// one workgroup per group: the partials of the tiles that touch the rectangle, in a fixed order, in double
constexpr int SC_FIN = 1024;  // threads of the final pass

__global__ __launch_bounds__(SC_FIN) void ssim_crop_finish_kernel(const gsr_ssim_crop c, int tiles_x, int tiles_y,
                                                               const float *__restrict__ partials) {
  __shared__ double s[SC_FIN / WAVE];
  const CropRect r = load_rect(c.rect, c.height, c.width);
  int first = 0, planes = 0;
  float *value = nullptr;
#pragma unroll
  for (int k = 0; k < SC_G; k++) {
    if (k < (int)blockIdx.x) first += c.planes[k];
    if (k == (int)blockIdx.x) planes = c.planes[k], value = c.value[k];
  }
  if (rect_empty(r)) {
    if (threadIdx.x == 0) value[0] = 0.f;
    return;
  }
  const int tx0 = r.x0 / SS_T, ty0 = r.y0 / SS_T, ntx = (r.x1 - 1) / SS_T - tx0 + 1, nty = (r.y1 - 1) / SS_T - ty0 + 1;
  const int per_plane = ntx * nty, n = planes * per_plane;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += SC_FIN) {
    const int p = i / per_plane, q = i - p * per_plane, ty = q / ntx, tx = q - ty * ntx;
    acc += (double)partials[((size_t)(first + p) * tiles_y + ty0 + ty) * tiles_x + tx0 + tx];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, WAVE);
  if (threadIdx.x % WAVE == 0) s[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < SC_FIN / WAVE; w++) tot += s[w];
    value[0] = (float)(tot / ((double)planes * (double)(r.x1 - r.x0) * (double)(r.y1 - r.y0)));
  }
}

__global__ __launch_bounds__(SS_T *SS_T) void ssim_crop_backward_kernel(const gsr_ssim_crop c, SsimWindow win) {
  __shared__ float s[3][SS_IN][SS_IN + 1];
  __shared__ float h[3][SS_IN][SS_T + 1];
  const int H = c.height, W = c.width;
  const CropGroup g = pick_group(c, blockIdx.z);
  if (g.planes < 0 || !g.d_img1) return;
  const CropRect r = load_rect(c.rect, H, W);
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const int px = x0 + threadIdx.x, py = y0 + threadIdx.y;
  const size_t base = g.plane * (size_t)H * W;
  if (tile_misses(r, x0, y0)) {
    if (px < W && py < H) g.d_img1[base + (size_t)py * W + px] = 0.f;
    return;
  }
  const float up = (g.upstream ? g.upstream[0] : 1.f) / ((float)g.planes * (float)(r.x1 - r.x0) * (float)(r.y1 - r.y0));
  const int t = threadIdx.y * SS_T + threadIdx.x;
  for (int e = t; e < SS_IN * SS_IN; e += SS_T * SS_T) {
    const int ly = e / SS_IN, lx = e % SS_IN;
    const int gx = x0 + lx - SS_R, gy = y0 + ly - SS_R;
    const bool in = in_rect(r, gx, gy);  // (the maps hold nothing outside the rectangle: not read there)
    const size_t o = base + (size_t)gy * W + gx;
    s[0][ly][lx] = in ? up * g.dA[o] : 0.f;
    s[1][ly][lx] = in ? up * g.dB[o] : 0.f;
    s[2][ly][lx] = in ? up * g.dC[o] : 0.f;
  }
  __syncthreads();
  for (int e = t; e < SS_IN * SS_T; e += SS_T * SS_T) {
    const int ly = e / SS_T, lx = e % SS_T;
    float a = 0.f, b = 0.f, cc = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float wk = win.w[k];
      a += wk * s[0][ly][lx + k];
      b += wk * s[1][ly][lx + k];
      cc += wk * s[2][ly][lx + k];
    }
    h[0][ly][lx] = a;
    h[1][ly][lx] = b;
    h[2][ly][lx] = cc;
  }
  __syncthreads();
  if (px >= W || py >= H) return;
  const size_t o = base + (size_t)py * W + px;
  if (!in_rect(r, px, py)) {
    g.d_img1[o] = 0.f;
    return;
  }
  float a = 0.f, b = 0.f, cc = 0.f;
#pragma unroll
  for (int k = 0; k < 11; k++) {
    const float wk = win.w[k];
    a += wk * h[0][threadIdx.y + k][threadIdx.x];
    b += wk * h[1][threadIdx.y + k][threadIdx.x];
    cc += wk * h[2][threadIdx.y + k][threadIdx.x];
  }
  g.d_img1[o] = a + 2.f * g.img1[(size_t)g.plane * g.s0 + (py * g.s1 + px * g.s2)] * b + g.img2[o] * cc;
}

static const char *validate(const gsr_ssim_crop *c, bool backward, int *total_planes) {
  if (c->groups < 1 || c->groups > SC_G) return "1..4 groups";
  if (c->height <= 0 || c->width <= 0) return "height and width must be positive";
  if ((long long)c->height * c->width >= (1ll << 31)) return "image too large";
  if (!c->rect) return "rect is null";
  long long total = 0;
  for (int k = 0; k < c->groups; k++) {
    if (c->planes[k] <= 0) return "planes must be positive";
    total += c->planes[k];
    if (!c->img1[k] || !c->img2[k]) return "img1 and img2 are required";
    long long span = 0;
    const long long ext[3] = {c->planes[k], c->height, c->width};
    for (int d = 0; d < 3; d++) {
      if (c->img1_stride[k][d] < 0) return "img1 strides must not be negative";
      span += c->img1_stride[k][d] * (ext[d] - 1);
    }
    if (span >= (1ll << 31)) return "img1 spans more than 2^31 elements";
    if ((long long)c->planes[k] * c->height * c->width >= (1ll << 31)) return "group too large";
    const bool any = c->dA[k] || c->dB[k] || c->dC[k], all = c->dA[k] && c->dB[k] && c->dC[k];
    if (any && !all) return "dA, dB and dC come together";
    if (!backward && !c->value[k]) return "value is required";
    if (backward && c->d_img1[k] && !all) return "d_img1 needs dA, dB and dC";
  }
  if (total > 65535) return "at most 65535 planes";
  *total_planes = (int)total;
  return nullptr;
}

}  // namespace gsr

extern "C" {

size_t gsr_bounding_rect_workspace_ints(void) { return (size_t)gsr::BR_BLOCKS * 4; }

int gsr_bounding_rect(int height, int width, const void *mask, int mask_dtype, int *rect, int *workspace, gsr_stream_t stream_) {
  using namespace gsr;
  const char *bad = nullptr;
  if (height <= 0 || width <= 0)
    bad = "height and width must be positive";
  else if ((long long)height * width >= (1ll << 31))
    bad = "mask too large";
  else if (!mask || !rect || !workspace)
    bad = "mask, rect and workspace are required";
  else if (mask_dtype != GSR_MASK_F32 && mask_dtype != GSR_MASK_U8)
    bad = "mask_dtype must be GSR_MASK_F32 or GSR_MASK_U8";
  if (bad) {
    set_error("gsr_bounding_rect: %s", bad);
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int n = height * width;
  const bool wide = reinterpret_cast<uintptr_t>(mask) % 16 == 0;
  int nblk;
  if (mask_dtype == GSR_MASK_F32) {
    const float *m = static_cast<const float *>(mask);
    nblk = bounding_rect_blocks(n, wide ? 4 : 1);
    if (wide)
      hipLaunchKernelGGL((bounding_rect_partial_kernel<float, 4>), dim3(nblk), dim3(BR_THREADS), 0, stream, height, width, m, workspace);
    else
      hipLaunchKernelGGL((bounding_rect_partial_kernel<float, 1>), dim3(nblk), dim3(BR_THREADS), 0, stream, height, width, m, workspace);
  } else {
    const unsigned char *m = static_cast<const unsigned char *>(mask);
    nblk = bounding_rect_blocks(n, wide ? 16 : 1);
    if (wide)
      hipLaunchKernelGGL((bounding_rect_partial_kernel<unsigned char, 16>), dim3(nblk), dim3(BR_THREADS), 0, stream, height, width, m,
                         workspace);
    else
      hipLaunchKernelGGL((bounding_rect_partial_kernel<unsigned char, 1>), dim3(nblk), dim3(BR_THREADS), 0, stream, height, width, m,
                         workspace);
  }
  hipLaunchKernelGGL(bounding_rect_finish_kernel, dim3(1), dim3(BR_THREADS), 0, stream, nblk, workspace, rect);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

size_t gsr_ssim_crop_workspace_floats(int total_planes, int height, int width) {
  if (total_planes <= 0 || height <= 0 || width <= 0) return 0;
  return (size_t)total_planes * ((height + gsr::SS_T - 1) / gsr::SS_T) * ((width + gsr::SS_T - 1) / gsr::SS_T);
}

int gsr_ssim_crop_forward(const gsr_ssim_crop *c, float *workspace, gsr_stream_t stream_) {
  using namespace gsr;
  int total = 0;
  const char *bad = c ? validate(c, false, &total) : "crop is null";
  if (!bad && !workspace) bad = "workspace is null";
  if (bad) {
    set_error("gsr_ssim_crop_forward: %s", bad);
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int tx = (c->width + SS_T - 1) / SS_T, ty = (c->height + SS_T - 1) / SS_T;
  hipLaunchKernelGGL(ssim_crop_forward_kernel, dim3(tx, ty, total), dim3(SS_T, SS_T), 0, stream, *c, make_window(), workspace);
  hipLaunchKernelGGL(ssim_crop_finish_kernel, dim3(c->groups), dim3(SC_FIN), 0, stream, *c, tx, ty, workspace);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_ssim_crop_backward(const gsr_ssim_crop *c, gsr_stream_t stream_) {
  using namespace gsr;
  int total = 0;
  const char *bad = c ? validate(c, true, &total) : "crop is null";
  if (bad) {
    set_error("gsr_ssim_crop_backward: %s", bad);
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int tx = (c->width + SS_T - 1) / SS_T, ty = (c->height + SS_T - 1) / SS_T;
  hipLaunchKernelGGL(ssim_crop_backward_kernel, dim3(tx, ty, total), dim3(SS_T, SS_T), 0, stream, *c, make_window());
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

}  // extern "C"
