// pbr.hip -- the image-based-lighting stage of the reference's pbr package: texture / cube-map sampling (the three
// nvdiffrast.torch.texture call shapes of pbr/light.py and pbr/shade.py), the light's prefilter (CubemapLight.build_mips: 2x2
// mip, diffuse and GGX specular cube convolutions) and pbr_shading fused into one kernel forward and one backward.
//
// Sampling rules (DESIGN.md "PBR stage"; tests/pbr_reference.py restates them in float64):
//   * face: the largest |component| (z wins ties with nothing, y wins against x only when strictly larger, else x); face-local
//     (a, b) / m from pbr/light.py cube_to_dir, u = (a/m + 1)/2 clamped to [0, 1], texel centres at (i + 0.5)/N;
//   * bilinear taps outside the face: a tap off one edge is the texel of the neighbouring face that contains the tap's
//     texel-centre direction (exact integer arithmetic); a tap off two edges (a cube corner) has no texel: its weight goes in
//     equal thirds to the footprint's other three taps;
//   * a zero or non-finite direction / uv samples 0 and takes no gradient;
//   * 2-D: the clamp boundary (tap indices clamped); mip: level = clamp(bias, 0, L-1), trilinear between floor(level) and the
//     next level (the last level with itself).
// Backward reductions onto the textures: the concatenated gradient space of every level is cut into as few windows as fit in LDS
// (at most PBR_WIN_MAX floats each); a workgroup sums its pixels' tap gradients for one window in LDS and adds the non-zero entries
// to global memory once.
#include "gsr_common.h"

#include <math.h>

namespace gsr {

constexpr int PBR_WIN_MAX = 38912;  // LDS floats per workgroup at most (152 KiB of the CU's 160)
constexpr int PBR_BLOCK = 1024;
constexpr int PBR_FWD_BLOCK = 256;
constexpr int PBR_MAXSEG = 2 * GSR_PBR_MAX_LEVELS + 1;

// ---- cube geometry --------------------------------------------------------------------------------------------------
// direction (scaled by m) of face-local (a, b) on face f: pbr/light.py cube_to_dir with the major component m
template <typename T>
__device__ __forceinline__ void cube_dir(int f, T a, T b, T m, T &x, T &y, T &z) {
  switch (f) {
    case 0: x = m; y = -b; z = -a; break;
    case 1: x = -m; y = -b; z = a; break;
    case 2: x = a; y = m; z = b; break;
    case 3: x = a; y = -m; z = -b; break;
    case 4: x = a; y = -b; z = m; break;
    default: x = -a; y = -b; z = -m; break;
  }
}
template <typename T>
__device__ __forceinline__ int face_of(T x, T y, T z) {
  const T ax = x < 0 ? -x : x, ay = y < 0 ? -y : y, az = z < 0 ? -z : z;
  if (az > (ax > ay ? ax : ay)) return z < 0 ? 5 : 4;
  if (ay > ax) return y < 0 ? 3 : 2;
  return x < 0 ? 1 : 0;
}
// inverse of cube_dir: face-local (a, b) and the major magnitude m of direction (x, y, z) on face f
template <typename T>
__device__ __forceinline__ void face_coords(int f, T x, T y, T z, T &a, T &b, T &m) {
  switch (f) {
    case 0: m = x; a = -z; b = -y; break;
    case 1: m = -x; a = z; b = -y; break;
    case 2: m = y; a = x; b = z; break;
    case 3: m = -y; a = x; b = -z; break;
    case 4: m = z; a = x; b = -y; break;
    default: m = -z; a = -x; b = -y; break;
  }
}

// four bilinear taps: element offsets (texel index; -1 = none) and weights
struct Taps {
  int t[4];
  float w[4];
};

// texel index of tap (x, y) on face f of an N x N cube, -2 for a corner tap, wrapping a tap off one edge onto its neighbour face
__device__ __forceinline__ int cube_tap(int f, int x, int y, int N) {
  const bool ox = x < 0 || x >= N, oy = y < 0 || y >= N;
  if (!ox && !oy) return (f * N + y) * N + x;
  if (ox && oy) return -2;
  int dx, dy, dz, a, b, m;
  cube_dir<int>(f, 2 * x + 1 - N, 2 * y + 1 - N, N, dx, dy, dz);  // the tap's texel centre, scaled by N
  const int g = face_of<int>(dx, dy, dz);
  face_coords<int>(g, dx, dy, dz, a, b, m);                       // m = N + 1 here
  const int nx = min(max((a + m) * N / (2 * m), 0), N - 1), ny = min(max((b + m) * N / (2 * m), 0), N - 1);
  return (g * N + ny) * N + nx;
}

__device__ __forceinline__ bool cube_footprint(float dx, float dy, float dz, int N, Taps &tp) {
  const int f = face_of<float>(dx, dy, dz);
  float a, b, m;
  face_coords<float>(f, dx, dy, dz, a, b, m);
  if (!(m > 0.f) || !isfinite(a) || !isfinite(b) || !isfinite(m)) return false;
  const float u = fminf(fmaxf((a / m + 1.f) * 0.5f, 0.f), 1.f), v = fminf(fmaxf((b / m + 1.f) * 0.5f, 0.f), 1.f);
  const float sx = u * (float)N - 0.5f, sy = v * (float)N - 0.5f;
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx = sx - fx0, fy = sy - fy0;
  tp.w[0] = (1.f - fx) * (1.f - fy);
  tp.w[1] = fx * (1.f - fy);
  tp.w[2] = (1.f - fx) * fy;
  tp.w[3] = fx * fy;
  tp.t[0] = cube_tap(f, x0, y0, N);
  tp.t[1] = cube_tap(f, x0 + 1, y0, N);
  tp.t[2] = cube_tap(f, x0, y0 + 1, N);
  tp.t[3] = cube_tap(f, x0 + 1, y0 + 1, N);
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (tp.t[k] == -2) {  // at most one corner tap: its weight in thirds to the others
      const float share = tp.w[k] * (1.f / 3.f);
      tp.w[k] = 0.f;
      tp.t[k] = -1;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j != k) tp.w[j] += share;
    }
  return true;
}

// 2-D clamp footprint; dsx/dsy: d(weight)/d(u*W), d(weight)/d(v*H) per tap, for the uv gradient
__device__ __forceinline__ bool flat_footprint(float u, float v, int W, int H, Taps &tp, float *dwu, float *dwv) {
  if (!isfinite(u) || !isfinite(v)) return false;
  const float sx = fminf(fmaxf(u * (float)W - 0.5f, -1.f), (float)W), sy = fminf(fmaxf(v * (float)H - 0.5f, -1.f), (float)H);
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx = sx - fx0, fy = sy - fy0;
  const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
  const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
  tp.t[0] = ya * W + xa;
  tp.t[1] = ya * W + xb;
  tp.t[2] = yb * W + xa;
  tp.t[3] = yb * W + xb;
  tp.w[0] = (1.f - fx) * (1.f - fy);
  tp.w[1] = fx * (1.f - fy);
  tp.w[2] = (1.f - fx) * fy;
  tp.w[3] = fx * fy;
  if (dwu) {
    dwu[0] = -(1.f - fy) * W; dwu[1] = (1.f - fy) * W; dwu[2] = -fy * W; dwu[3] = fy * W;
    dwv[0] = -(1.f - fx) * H; dwv[1] = -fx * H; dwv[2] = (1.f - fx) * H; dwv[3] = fx * H;
  }
  return true;
}

__device__ __forceinline__ bool footprint(const gsr_pbr_texture &tx, int l, const float *c, Taps &tp, float *dwu = nullptr,
                                          float *dwv = nullptr) {
  if (tx.cube) return cube_footprint(c[0], c[1], c[2], tx.width[l], tp);
  return flat_footprint(c[0], c[1], tx.width[l], tx.height[l], tp, dwu, dwv);
}

// mip level selection: levels l0, l1, the weight t of l1; pass: whether the bias lies inside [0, L-1] (its gradient flows)
__device__ __forceinline__ void mip_select(int L, const float *bias, int p, int &l0, int &l1, float &t, bool &pass) {
  if (!bias || L == 1) {
    l0 = l1 = 0;
    t = 0.f;
    pass = false;
    return;
  }
  const float b = bias[p];
  const float lv = fminf(fmaxf(b, 0.f), (float)(L - 1));
  pass = b >= 0.f && b <= (float)(L - 1);
  l0 = min((int)floorf(lv), L - 1);
  l1 = min(l0 + 1, L - 1);
  t = lv - (float)l0;
}

// ---- backward reduction: gradient space of up to PBR_MAXSEG arrays, one LDS window per workgroup ----------------------------
struct GradSpace {
  int total, win;  // win: floats of this launch's LDS window
  int off[PBR_MAXSEG + 1];
  float *ptr[PBR_MAXSEG];
  const float *chain;  // non-null: segment 0 is the raw diffuse cube, its gradient is multiplied by d clamp(x^(1/2.2)) / dx
};

__device__ __forceinline__ void win_add(float *lds, int lo, int win, int idx, float v) {
  const unsigned r = (unsigned)(idx - lo);
  if (r < (unsigned)win && v != 0.f) atomicAdd(&lds[r], v);
}

__device__ __forceinline__ float diffuse_pow(float x) { return fminf(fmaxf(__powf(x, 1.f / 2.2f), 0.f), 1.f); }
__device__ __forceinline__ float diffuse_pow_grad(float x) {
  const float y = powf(x, 1.f / 2.2f);
  return (y >= 0.f && y <= 1.f) ? (1.f / 2.2f) * powf(x, 1.f / 2.2f - 1.f) : 0.f;
}

__device__ void win_zero(float *lds, int win) {
  for (int i = threadIdx.x; i < win; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
}
__device__ void win_flush(float *lds, int lo, const GradSpace &gs) {
  __syncthreads();
  for (int i = threadIdx.x; i < gs.win; i += blockDim.x) {
    const int g = lo + i;
    if (g >= gs.total) break;
    float v = lds[i];
    if (v == 0.f) continue;
    int s = 0;
    while (g >= gs.off[s + 1]) s++;
    const int e = g - gs.off[s];
    if (s == 0 && gs.chain) v *= diffuse_pow_grad(gs.chain[e]);
    if (gs.ptr[s]) atomicAdd(gs.ptr[s] + e, v);
  }
}

// ---- generic texture ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PBR_FWD_BLOCK) void texture_forward_kernel(gsr_pbr_texture tx, int n, const float *coords,
                                                                        const float *bias, float *out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int C = tx.channels, D = tx.cube ? 3 : 2;
  float c[3];
  for (int k = 0; k < D; k++) c[k] = coords[(size_t)p * D + k];
  int l0, l1;
  float t;
  bool pass;
  mip_select(tx.levels, bias, p, l0, l1, t, pass);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int side = 0; side < 2; side++) {
    const int l = side ? l1 : l0;
    if (side && l1 == l0) break;
    const float lw = side ? t : 1.f - t;
    Taps tp;
    if (!footprint(tx, l, c, tp)) break;
    for (int k = 0; k < 4; k++)
      if (tp.t[k] >= 0)
        for (int ch = 0; ch < C; ch++) acc[ch] += lw * tp.w[k] * tx.data[l][(size_t)tp.t[k] * C + ch];
  }
  for (int ch = 0; ch < C; ch++) out[(size_t)p * C + ch] = acc[ch];
}

__global__ __launch_bounds__(PBR_BLOCK) void texture_backward_kernel(gsr_pbr_texture tx, int n, const float *coords,
                                                                     const float *bias, const float *dout, float *dcoords,
                                                                     float *dbias, GradSpace gs, int per_wg) {
  extern __shared__ float lds[];
  const int lo = blockIdx.y * gs.win;
  win_zero(lds, gs.win);
  const int C = tx.channels, D = tx.cube ? 3 : 2;
  const int p_begin = blockIdx.x * per_wg, p_end = min(n, p_begin + per_wg);
  for (int p = p_begin + threadIdx.x; p < p_end; p += blockDim.x) {
    float c[3], g[4];
    for (int k = 0; k < D; k++) c[k] = coords[(size_t)p * D + k];
    for (int ch = 0; ch < C; ch++) g[ch] = dout[(size_t)p * C + ch];
    int l0, l1;
    float t;
    bool pass;
    mip_select(tx.levels, bias, p, l0, l1, t, pass);
    float du = 0.f, dv = 0.f, dl = 0.f;
    for (int side = 0; side < 2; side++) {
      if (side && l1 == l0) break;
      const int l = side ? l1 : l0;
      const float lw = side ? t : 1.f - t;
      Taps tp;
      float dwu[4], dwv[4];
      if (!footprint(tx, l, c, tp, dwu, dwv)) break;
      for (int k = 0; k < 4; k++) {
        if (tp.t[k] < 0) continue;
        float gv = 0.f;
        for (int ch = 0; ch < C; ch++) {
          const float tv = tx.data[l][(size_t)tp.t[k] * C + ch];
          gv += g[ch] * tv;
          win_add(lds, lo, gs.win, gs.off[l] + tp.t[k] * C + ch, lw * tp.w[k] * g[ch]);
        }
        if (!tx.cube) {
          du += lw * dwu[k] * gv;
          dv += lw * dwv[k] * gv;
        }
        dl += (side ? 1.f : -1.f) * tp.w[k] * gv;
      }
    }
    if (blockIdx.y == 0) {
      if (dcoords && !tx.cube) {
        dcoords[(size_t)p * 2] = du;
        dcoords[(size_t)p * 2 + 1] = dv;
      }
      if (dbias) dbias[p] = (pass && l1 != l0) ? dl : 0.f;
    }
  }
  win_flush(lds, lo, gs);
}

// ---- build_mips -----------------------------------------------------------------------------------------------------------
__global__ void cube_mip_forward_kernel(int n, int C, const float *fine, float *coarse) {
  const int h = n / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * h * h * C) return;
  const int ch = i % C, x = (i / C) % h, y = (i / C / h) % h, f = i / C / h / h;
  const float *s = fine + ((size_t)(f * n + 2 * y) * n + 2 * x) * C + ch;
  coarse[i] = 0.25f * (s[0] + s[C] + s[(size_t)n * C] + s[(size_t)n * C + C]);
}

// d_fine at every fine texel-centre direction = cube lookup of 0.25 d_coarse (pbr/light.py:39-54)
__global__ void cube_mip_backward_kernel(int n, int C, const float *dcoarse, float *dfine) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * n * n) return;
  const int x = i % n, y = (i / n) % n, f = i / n / n;
  float dx, dy, dz;
  cube_dir<float>(f, (float)(2 * x + 1 - n) / (float)n, (float)(2 * y + 1 - n) / (float)n, 1.f, dx, dy, dz);
  const float r = 1.f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
  Taps tp;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (cube_footprint(dx * r, dy * r, dz * r, n / 2, tp))
    for (int k = 0; k < 4; k++)
      if (tp.t[k] >= 0)
        for (int ch = 0; ch < C; ch++) acc[ch] += tp.w[k] * dcoarse[(size_t)tp.t[k] * C + ch];
  for (int ch = 0; ch < C; ch++) dfine[(size_t)i * C + ch] = 0.25f * acc[ch];
}

// normalised texel-centre direction and the reference's per-texel solid-angle weight (atan differences, integer half-size)
__device__ __forceinline__ void texel_dir(int i, int N, float &x, float &y, float &z) {
  const int px = i % N, py = (i / N) % N, f = i / N / N;
  cube_dir<float>(f, 2.f * (((float)px + 0.5f) / (float)N) - 1.f, 2.f * (((float)py + 0.5f) / (float)N) - 1.f, 1.f, x, y, z);
  const float r = 1.f / sqrtf(x * x + y * y + z * z);
  x *= r;
  y *= r;
  z *= r;
}
__device__ __forceinline__ float texel_area(int i, int N) {
  if (N <= 1) return 1.f;
  const int H = N / 2, x = abs(i % N - H), y = abs((i / N) % N - H);
  const float dx = atanf((float)(x + 1) / (float)H) - atanf((float)x / (float)H);
  const float dy = atanf((float)(y + 1) / (float)H) - atanf((float)y / (float)H);
  return dx * dy;
}
__device__ __forceinline__ float diffuse_w(const float *n, const float *l, float area) {
  const float c = fminf(fmaxf(n[0] * l[0] + n[1] * l[1] + n[2] * l[2], 0.f), 0.999f);
  return c * area / 3.141592f;
}
// GGX weight of input texel direction l (solid angle `area`) for the output direction v
__device__ __forceinline__ float specular_w(const float *v, const float *l, float area, float alpha2, float cutoff) {
  const float d = v[0] * l[0] + v[1] * l[1] + v[2] * l[2];
  if (!(d >= cutoff)) return 0.f;
  float hx = l[0] + v[0], hy = l[1] + v[1], hz = l[2] + v[2];
  const float hl = sqrtf(hx * hx + hy * hy + hz * hz);
  if (hl > 0.f) {
    hx /= hl;
    hy /= hl;
    hz /= hl;
  }
  const float noh = fminf(fmaxf(v[0] * hx + v[1] * hy + v[2] * hz, 0.f), 1.f);
  const float dd = (noh * alpha2 - noh) * noh + 1.f;
  const float D = alpha2 / (dd * dd * 3.14159265358979323846f);
  return fmaxf(d, 0.f) * D * area / 4.f;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Prefilter sums, brute force over every texel pair: one wave per row (forward: an output texel, summing over the inputs;
// backward: an input texel, gathering over the outputs -- no atomics), the lanes stride over the other index, then a wave sum.
constexpr int PF_BLOCK = 256;

template <bool BWD>
__global__ __launch_bounds__(PF_BLOCK) void diffuse_kernel(int N, const float *src, float *dst) {
  const int T = 6 * N * N, row = blockIdx.x * (PF_BLOCK / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  if (row >= T) return;  // uniform per wave
  float a[3], c[3];
  texel_dir(row, N, a[0], a[1], a[2]);
  const float arow = texel_area(row, N);
  float r = 0.f, g = 0.f, b = 0.f;
  for (int k = lane; k < T; k += WAVE) {
    texel_dir(k, N, c[0], c[1], c[2]);
    // forward: out[row] += w(N = row, L = k) src[k]; backward: d_cube[row] += w(N = k, L = row) d_out[k] (w is symmetric in the
    // directions, the solid angle is the input texel's)
    const float w = diffuse_w(a, c, BWD ? arow : texel_area(k, N));
    r += w * src[3 * k];
    g += w * src[3 * k + 1];
    b += w * src[3 * k + 2];
  }
  r = wave_sum(r);
  g = wave_sum(g);
  b = wave_sum(b);
  if (lane == 0) {
    dst[3 * row] = r;
    dst[3 * row + 1] = g;
    dst[3 * row + 2] = b;
  }
}

// forward: out[row] = sum_k w(V = row, L = k) cube[k] / wsum[row]; backward: d_cube[row] = sum_k w(V = k, L = row) d_out[k] / wsum[k]
template <bool BWD>
__global__ __launch_bounds__(PF_BLOCK) void specular_kernel(int N, float alpha2, float cutoff, const float *src, float *dst,
                                                            float *wsum) {
  const int T = 6 * N * N, row = blockIdx.x * (PF_BLOCK / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  if (row >= T) return;
  float a[3], c[3];
  texel_dir(row, N, a[0], a[1], a[2]);
  const float arow = texel_area(row, N);
  float r = 0.f, g = 0.f, b = 0.f, ws = 0.f;
  for (int k = lane; k < T; k += WAVE) {
    texel_dir(k, N, c[0], c[1], c[2]);
    float w = BWD ? specular_w(c, a, arow, alpha2, cutoff) : specular_w(a, c, texel_area(k, N), alpha2, cutoff);
    if (w == 0.f) continue;
    if (BWD) w /= wsum[k];
    r += w * src[3 * k];
    g += w * src[3 * k + 1];
    b += w * src[3 * k + 2];
    ws += w;
  }
  r = wave_sum(r);
  g = wave_sum(g);
  b = wave_sum(b);
  ws = wave_sum(ws);
  if (lane == 0) {
    const float inv = BWD ? 1.f : 1.f / ws;
    dst[3 * row] = r * inv;
    dst[3 * row + 1] = g * inv;
    dst[3 * row + 2] = b * inv;
    if (!BWD) wsum[row] = ws;
  }
}

// ---- fused shading ----------------------------------------------------------------------------------------------------------
constexpr float MIN_R = 0.08f, MAX_R = 0.5f;

// one pixel forward; keeps what the backward needs
struct PixelState {
  float n[3], alb[3], occ, met, rough;
  float dl_raw[3];  // diffuse cube lookup before the occlusion
  float dl[3];      // diffuse_light
  float spec[3], spec0[3], spec1[3];
  float fg, dfg_dv;
  float lvl_t;
  int l0, l1;
  bool lvl_pass;
  float dlvl_dr;
  float F0[3];
  float pre[3];   // diffuse_rgb + specular_rgb
  float mapped[3];  // after clamp / tone
  float out[3];
  bool valid_d, valid_s;
  Taps td, ts0, ts1;
};

__device__ __forceinline__ float lookup3(const float *data, const Taps &tp, int ch, bool pw) {
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (tp.t[k] >= 0) {
      const float v = data[(size_t)tp.t[k] * 3 + ch];
      a += tp.w[k] * (pw ? diffuse_pow(v) : v);
    }
  return a;
}

__device__ __forceinline__ float aces(float x) {
  return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
}
__device__ __forceinline__ float aces_grad(float x) {
  const float nu = x * (2.51f * x + 0.03f), de = x * (2.43f * x + 0.59f) + 0.14f;
  return ((5.02f * x + 0.03f) * de - nu * (4.86f * x + 0.59f)) / (de * de);
}
constexpr float SRGB_EPS = 1.1920928955078125e-07f;
__device__ __forceinline__ float to_srgb(float x) {
  return x <= 0.0031308f ? 323.f / 25.f * x : (211.f * powf(fmaxf(x, SRGB_EPS), 5.f / 12.f) - 11.f) / 200.f;
}
__device__ __forceinline__ float to_srgb_grad(float x) {
  if (x <= 0.0031308f) return 323.f / 25.f;
  if (x < SRGB_EPS) return 0.f;
  return 211.f / 200.f * (5.f / 12.f) * powf(x, 5.f / 12.f - 1.f);
}

__device__ void shade_pixel(const gsr_pbr_shade &s, int p, PixelState &st) {
  float v[3];
  for (int k = 0; k < 3; k++) {
    st.n[k] = s.normals[(size_t)p * 3 + k];
    v[k] = s.view_dirs[(size_t)p * 3 + k];
    st.alb[k] = s.albedo[(size_t)p * 3 + k];
  }
  st.rough = s.roughness[p];
  st.occ = s.occlusion ? s.occlusion[p] : 1.f;
  st.met = s.metallic ? s.metallic[p] : 0.f;
  const float nv = st.n[0] * v[0] + st.n[1] * v[1] + st.n[2] * v[2];
  const float rc = 2.f * fmaxf(nv, 0.f);
  const float rd[3] = {rc * st.n[0] - v[0], rc * st.n[1] - v[1], rc * st.n[2] - v[2]};
  // diffuse
  st.valid_d = cube_footprint(st.n[0], st.n[1], st.n[2], s.diffuse.width[0], st.td);
  for (int c = 0; c < 3; c++) {
    st.dl_raw[c] = st.valid_d ? lookup3(s.diffuse.data[0], st.td, c, true) : 0.f;
    st.dl[c] = s.occlusion ? st.dl_raw[c] * st.occ : st.dl_raw[c];
  }
  // split-sum LUT at (NoV, roughness), channel 0
  const float nov = fminf(fmaxf(nv, 1e-4f), 1.f);
  {
    Taps tl;
    float dwu[4], dwv[4];
    st.fg = 0.f;
    st.dfg_dv = 0.f;
    if (flat_footprint(nov, st.rough, s.lut.width[0], s.lut.height[0], tl, dwu, dwv)) {
      const int C = s.lut.channels;
      for (int k = 0; k < 4; k++) {
        const float tv = s.lut.data[0][(size_t)tl.t[k] * C];
        st.fg += tl.w[k] * tv;
        st.dfg_dv += dwv[k] * tv;
      }
    }
  }
  // mip level: CubemapLight.get_mip
  const int L = s.specular.levels;
  float lvl;
  if (st.rough < MAX_R) {
    lvl = (fminf(fmaxf(st.rough, MIN_R), MAX_R) - MIN_R) / (MAX_R - MIN_R) * (float)(L - 2);
    st.dlvl_dr = (st.rough >= MIN_R && st.rough <= MAX_R) ? (float)(L - 2) / (MAX_R - MIN_R) : 0.f;
  } else {
    lvl = (fminf(fmaxf(st.rough, MAX_R), 1.f) - MAX_R) / (1.f - MAX_R) + (float)(L - 2);
    st.dlvl_dr = (st.rough >= MAX_R && st.rough <= 1.f) ? 1.f / (1.f - MAX_R) : 0.f;
  }
  mip_select(L, &lvl, 0, st.l0, st.l1, st.lvl_t, st.lvl_pass);
  st.valid_s = cube_footprint(rd[0], rd[1], rd[2], s.specular.width[st.l0], st.ts0);
  if (st.valid_s) cube_footprint(rd[0], rd[1], rd[2], s.specular.width[st.l1], st.ts1);
  for (int c = 0; c < 3; c++) {
    st.spec0[c] = st.valid_s ? lookup3(s.specular.data[st.l0], st.ts0, c, false) : 0.f;
    st.spec1[c] = st.valid_s ? lookup3(s.specular.data[st.l1], st.ts1, c, false) : 0.f;
    st.spec[c] = (1.f - st.lvl_t) * st.spec0[c] + st.lvl_t * st.spec1[c];
  }
  const bool inside = s.mask[p] > 0.f;
  for (int c = 0; c < 3; c++) {
    st.F0[c] = s.metallic ? (1.f - st.met) * 0.04f + st.alb[c] * st.met : 0.04f;
    const float drgb = st.dl[c] * st.alb[c], srgb = st.spec[c] * (st.F0[c] * st.fg);
    st.pre[c] = drgb + srgb;
    float m = s.tone ? fminf(fmaxf(aces(st.pre[c]), 0.f), 1.f) : fminf(fmaxf(st.pre[c], 0.f), 1.f);
    st.mapped[c] = m;
    if (s.gamma) m = to_srgb(m);
    st.out[c] = inside ? m : (s.background ? s.background[(size_t)p * 3 + c] : 0.f);
  }
}

__global__ __launch_bounds__(PBR_FWD_BLOCK) void shade_forward_kernel(gsr_pbr_shade s) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= s.n) return;
  PixelState st;
  shade_pixel(s, p, st);
  for (int c = 0; c < 3; c++) {
    const size_t o = (size_t)p * 3 + c;
    s.render_rgb[o] = st.out[c];
    s.diffuse_rgb[o] = st.dl[c] * st.alb[c];
    s.specular_rgb[o] = st.spec[c] * (st.F0[c] * st.fg);
    s.diffuse_light[o] = st.dl[c];
  }
}

// gradient space: [diffuse cube (3 ch)] [specular level 0] ... [specular level L-1]
__global__ __launch_bounds__(PBR_BLOCK) void shade_backward_kernel(gsr_pbr_shade s, GradSpace gs, int per_wg) {
  extern __shared__ float lds[];
  const int lo = blockIdx.y * gs.win;
  win_zero(lds, gs.win);
  const int p_begin = blockIdx.x * per_wg, p_end = min(s.n, p_begin + per_wg);
  for (int p = p_begin + threadIdx.x; p < p_end; p += blockDim.x) {
    PixelState st;
    shade_pixel(s, p, st);
    const bool inside = s.mask[p] > 0.f;
    float gd[3], gsp[3], gdl[3];
    for (int c = 0; c < 3; c++) {
      const size_t o = (size_t)p * 3 + c;
      float g = (inside && s.d_render_rgb) ? s.d_render_rgb[o] : 0.f;
      if (s.gamma) g *= to_srgb_grad(st.mapped[c]);
      if (s.tone) {
        const float y = aces(st.pre[c]);
        g = (y >= 0.f && y <= 1.f) ? g * aces_grad(st.pre[c]) : 0.f;
      } else {
        g = (st.pre[c] >= 0.f && st.pre[c] <= 1.f) ? g : 0.f;
      }
      gd[c] = g + (s.d_diffuse_rgb ? s.d_diffuse_rgb[o] : 0.f);
      gsp[c] = g + (s.d_specular_rgb ? s.d_specular_rgb[o] : 0.f);
      gdl[c] = gd[c] * st.alb[c] + (s.d_diffuse_light ? s.d_diffuse_light[o] : 0.f);
    }
    float d_occ = 0.f, d_fg = 0.f, d_met = 0.f, d_lvl = 0.f, d_alb[3];
    float gspec[3], graw[3];
    for (int c = 0; c < 3; c++) {
      d_alb[c] = gd[c] * st.dl[c];
      d_occ += gdl[c] * st.dl_raw[c];
      graw[c] = s.occlusion ? gdl[c] * st.occ : gdl[c];
      gspec[c] = gsp[c] * st.F0[c] * st.fg;
      const float g_refl = gsp[c] * st.spec[c];
      d_fg += g_refl * st.F0[c];
      const float g_f0 = g_refl * st.fg;
      if (s.metallic) {
        d_met += g_f0 * (st.alb[c] - 0.04f);
        d_alb[c] += g_f0 * st.met;
      }
      d_lvl += gspec[c] * (st.spec1[c] - st.spec0[c]);
    }
    if (blockIdx.y == 0) {
      for (int c = 0; c < 3; c++)
        if (s.d_albedo) s.d_albedo[(size_t)p * 3 + c] = d_alb[c];
      if (s.d_occlusion) s.d_occlusion[p] = d_occ;
      if (s.d_metallic) s.d_metallic[p] = d_met;
      if (s.d_roughness) s.d_roughness[p] = d_fg * st.dfg_dv + (st.lvl_pass ? d_lvl * st.dlvl_dr : 0.f);
    }
    // texture gradients into the window
    if (st.valid_d)
      for (int k = 0; k < 4; k++)
        if (st.td.t[k] >= 0)
          for (int c = 0; c < 3; c++) win_add(lds, lo, gs.win, gs.off[0] + st.td.t[k] * 3 + c, st.td.w[k] * graw[c]);
    if (st.valid_s) {
      for (int side = 0; side < 2; side++) {
        if (side && st.l1 == st.l0) break;
        const Taps &tp = side ? st.ts1 : st.ts0;
        const int l = side ? st.l1 : st.l0;
        const float lw = side ? st.lvl_t : 1.f - st.lvl_t;
        for (int k = 0; k < 4; k++)
          if (tp.t[k] >= 0)
            for (int c = 0; c < 3; c++) win_add(lds, lo, gs.win, gs.off[1 + l] + tp.t[k] * 3 + c, lw * tp.w[k] * gspec[c]);
      }
    }
  }
  win_flush(lds, lo, gs);
}

static bool texture_ok(const gsr_pbr_texture &t, bool need_data = true) {
  if (t.channels < 1 || t.channels > 4 || t.levels < 1 || t.levels > GSR_PBR_MAX_LEVELS) return false;
  for (int l = 0; l < t.levels; l++) {
    if (t.width[l] < 1 || t.height[l] < 1 || (need_data && !t.data[l])) return false;
    if (t.cube && t.width[l] != t.height[l]) return false;
    if ((size_t)t.width[l] * t.height[l] * (t.cube ? 6 : 1) * t.channels > (size_t)1 << 30) return false;
  }
  return true;
}
static size_t texture_floats(const gsr_pbr_texture &t, int l) {
  return (size_t)t.width[l] * t.height[l] * (t.cube ? 6 : 1) * t.channels;
}
// windows of the gradient space (gs.total floats) and the pixel split: about one round of workgroups over the 256 CUs in all
static void bwd_grid(int n, GradSpace &gs, int &nwg, int &groups, int &per_wg) {
  groups = (gs.total + PBR_WIN_MAX - 1) / PBR_WIN_MAX;
  gs.win = ((gs.total + groups - 1) / groups + 63) / 64 * 64;
  nwg = max(1, min(max(1, 256 / groups), (n + 4095) / 4096));
  per_wg = (n + nwg - 1) / nwg;
}

}  // namespace gsr

extern "C" {

int gsr_pbr_texture_forward(const gsr_pbr_texture *tex, int n, const float *coords, const float *mip_bias, float *out,
                            gsr_stream_t stream_) {
  using namespace gsr;
  if (!tex || n < 0 || !texture_ok(*tex) || (n > 0 && (!coords || !out))) {
    set_error("gsr_pbr_texture_forward: bad arguments");
    return GSR_EINVAL;
  }
  if (n == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(texture_forward_kernel, dim3((n + PBR_FWD_BLOCK - 1) / PBR_FWD_BLOCK), dim3(PBR_FWD_BLOCK), 0, stream, *tex,
                     n, coords, mip_bias, out);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_texture_backward(const gsr_pbr_texture *tex, int n, const float *coords, const float *mip_bias, const float *d_out,
                             float *d_coords, float *d_bias, gsr_stream_t stream_) {
  using namespace gsr;
  if (!tex || n < 0 || !texture_ok(*tex) || (n > 0 && (!coords || !d_out))) {
    set_error("gsr_pbr_texture_backward: bad arguments");
    return GSR_EINVAL;
  }
  if (n == 0) return GSR_OK;
  GradSpace gs{};
  size_t total = 0;
  for (int l = 0; l < tex->levels; l++) {
    gs.off[l] = (int)total;
    gs.ptr[l] = tex->grad[l];
    total += texture_floats(*tex, l);
  }
  if (total > (size_t)1 << 30) {
    set_error("gsr_pbr_texture_backward: texture too large");
    return GSR_EINVAL;
  }
  gs.off[tex->levels] = gs.total = (int)total;
  int nwg, groups, per_wg;
  bwd_grid(n, gs, nwg, groups, per_wg);
  const size_t lds = (size_t)gs.win * sizeof(float);
  GSR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(texture_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(texture_backward_kernel, dim3(nwg, groups), dim3(PBR_BLOCK), lds, stream, *tex, n, coords, mip_bias, d_out,
                     d_coords, d_bias, gs, per_wg);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_cube_mip_forward(int n, int channels, const float *fine, float *coarse, gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 2 || n % 2 || n > 4096 || channels < 1 || channels > 4 || !fine || !coarse) {
    set_error("gsr_pbr_cube_mip_forward: bad arguments (n even >= 2, 1..4 channels)");
    return GSR_EINVAL;
  }
  const int total = 6 * (n / 2) * (n / 2) * channels;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(cube_mip_forward_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, n, channels, fine, coarse);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_cube_mip_backward(int n, int channels, const float *d_coarse, float *d_fine, gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 2 || n % 2 || n > 4096 || channels < 1 || channels > 4 || !d_coarse || !d_fine) {
    set_error("gsr_pbr_cube_mip_backward: bad arguments (n even >= 2, 1..4 channels)");
    return GSR_EINVAL;
  }
  const int total = 6 * n * n;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(cube_mip_backward_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, n, channels, d_coarse, d_fine);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_diffuse_forward(int n, const float *cube, float *out, gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 1 || n > 256 || !cube || !out) {
    set_error("gsr_pbr_diffuse_forward: bad arguments (1 <= n <= 256)");
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(diffuse_kernel<false>, dim3((6 * n * n + 3) / 4), dim3(PF_BLOCK), 0, stream, n, cube, out);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_diffuse_backward(int n, const float *d_out, float *d_cube, gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 1 || n > 256 || !d_out || !d_cube) {
    set_error("gsr_pbr_diffuse_backward: bad arguments (1 <= n <= 256)");
    return GSR_EINVAL;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(diffuse_kernel<true>, dim3((6 * n * n + 3) / 4), dim3(PF_BLOCK), 0, stream, n, d_out, d_cube);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_specular_forward(int n, float roughness, float costheta_cutoff, const float *cube, float *out, float *wsum,
                             gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 1 || n > 256 || !cube || !out || !wsum || !(roughness >= 0.f)) {
    set_error("gsr_pbr_specular_forward: bad arguments (1 <= n <= 256)");
    return GSR_EINVAL;
  }
  const float alpha = roughness * roughness;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(specular_kernel<false>, dim3((6 * n * n + 3) / 4), dim3(PF_BLOCK), 0, stream, n, alpha * alpha,
                     costheta_cutoff, cube, out, wsum);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_specular_backward(int n, float roughness, float costheta_cutoff, const float *wsum, const float *d_out,
                              float *d_cube, gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 1 || n > 256 || !wsum || !d_out || !d_cube || !(roughness >= 0.f)) {
    set_error("gsr_pbr_specular_backward: bad arguments (1 <= n <= 256)");
    return GSR_EINVAL;
  }
  const float alpha = roughness * roughness;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(specular_kernel<true>, dim3((6 * n * n + 3) / 4), dim3(PF_BLOCK), 0, stream, n, alpha * alpha,
                     costheta_cutoff, d_out, d_cube, const_cast<float *>(wsum));
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

static int shade_check(const gsr_pbr_shade *s, const char *what, bool bwd) {
  using namespace gsr;
  bool ok = s && s->n >= 0 && texture_ok(s->diffuse) && texture_ok(s->specular) && texture_ok(s->lut) && s->diffuse.cube &&
            s->specular.cube && !s->lut.cube && s->diffuse.channels == 3 && s->specular.channels == 3 && s->lut.channels >= 1 &&
            s->diffuse.levels == 1 && s->lut.levels == 1;
  if (ok && s->n > 0) {
    ok = s->normals && s->view_dirs && s->albedo && s->roughness && s->mask;
    if (!bwd) ok = ok && s->render_rgb && s->diffuse_rgb && s->specular_rgb && s->diffuse_light;
  }
  if (!ok) {
    set_error("%s: bad arguments (3-channel one-level diffuse cube, 3-channel specular cube levels, 2-D LUT, [n] pixel arrays)",
              what);
    return GSR_EINVAL;
  }
  return GSR_OK;
}

int gsr_pbr_shade_forward(const gsr_pbr_shade *s, gsr_stream_t stream_) {
  using namespace gsr;
  if (shade_check(s, "gsr_pbr_shade_forward", false) != GSR_OK) return GSR_EINVAL;
  if (s->n == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(shade_forward_kernel, dim3((s->n + PBR_FWD_BLOCK - 1) / PBR_FWD_BLOCK), dim3(PBR_FWD_BLOCK), 0, stream, *s);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_shade_backward(const gsr_pbr_shade *s, gsr_stream_t stream_) {
  using namespace gsr;
  if (shade_check(s, "gsr_pbr_shade_backward", true) != GSR_OK) return GSR_EINVAL;
  if (s->n == 0) return GSR_OK;
  GradSpace gs{};
  gs.off[0] = 0;
  gs.ptr[0] = s->diffuse.grad[0];
  gs.chain = s->diffuse.data[0];
  size_t total = texture_floats(s->diffuse, 0);
  for (int l = 0; l < s->specular.levels; l++) {
    gs.off[1 + l] = (int)total;
    gs.ptr[1 + l] = s->specular.grad[l];
    total += texture_floats(s->specular, l);
  }
  if (total > (size_t)1 << 30) {
    set_error("gsr_pbr_shade_backward: light too large");
    return GSR_EINVAL;
  }
  gs.off[1 + s->specular.levels] = gs.total = (int)total;
  int nwg, groups, per_wg;
  bwd_grid(s->n, gs, nwg, groups, per_wg);
  const size_t lds = (size_t)gs.win * sizeof(float);
  GSR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(shade_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(shade_backward_kernel, dim3(nwg, groups), dim3(PBR_BLOCK), lds, stream, *s, gs, per_wg);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

}  // extern "C"

// ==== The environment light's own share of a PBR step ==========================================================
// The grey environment map (train.py:195-198), the environment-map TV regulariser (train.py:352-363) and the view directions
// (render.py:215-222).  A separate section of this file, not a translation unit of its own, because the lookups must be the ones
// of texture_forward_kernel: cube_footprint and the LDS-window reduction above are used as they are.  No kernel above is changed.
namespace gsr {

constexpr int ENV_BLOCK = 256;
// torchvision.transforms.functional.rgb_to_grayscale: l = 0.2989 r + 0.587 g + 0.114 b
constexpr float GREY_R = 0.2989f, GREY_G = 0.587f, GREY_B = 0.114f;

// the linear cube lookup of texture_forward_kernel (one level, three channels) at direction d[0..2]
__device__ __forceinline__ void env_sample(const float *__restrict__ base, int N, const float *__restrict__ d, float *e) {
  e[0] = e[1] = e[2] = 0.f;
  Taps tp;
  if (!cube_footprint(d[0], d[1], d[2], N, tp)) return;
  for (int k = 0; k < 4; k++)
    if (tp.t[k] >= 0)
      for (int ch = 0; ch < 3; ch++) e[ch] += tp.w[k] * base[(size_t)tp.t[k] * 3 + ch];
}

__global__ __launch_bounds__(ENV_BLOCK) void env_grey_kernel(int N, const float *__restrict__ base, int n,
                                                             const float *__restrict__ dirs, float *__restrict__ out) {
  const int p = blockIdx.x * ENV_BLOCK + threadIdx.x;
  if (p >= n) return;
  float e[3];
  env_sample(base, N, dirs + (size_t)p * 3, e);
  const float r = fminf(fmaxf(e[0], 0.f), 1.f), g = fminf(fmaxf(e[1], 0.f), 1.f), b = fminf(fmaxf(e[2], 0.f), 1.f);
  out[p] = GREY_R * r + GREY_G * g + GREY_B * b;
}

// sum over a workgroup of ENV_BLOCK threads, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float env_block_sum(float v, float *red) {
  v = wave_sum(v);
  __syncthreads();
  if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < ENV_BLOCK / WAVE; i++) s += red[i];
  return s;
}

// TV forward, first launch: e[p] = lookup at dirs[p] (kept for the backward) and, per workgroup, the sums of the squared
// differences to the sample below and to the sample to the right.  A thread looks its two neighbours up itself (the same
// instructions on the same inputs: the same bits as the neighbour's own e), so no workgroup waits for another.
__global__ __launch_bounds__(ENV_BLOCK) void env_tv_partial_kernel(int N, const float *__restrict__ base, int h, int w,
                                                                   const float *__restrict__ dirs, float *__restrict__ e,
                                                                   float *__restrict__ partials) {
  __shared__ float red[ENV_BLOCK / WAVE];
  const int n = h * w, p = blockIdx.x * ENV_BLOCK + threadIdx.x;
  float sv = 0.f, sh = 0.f;
  if (p < n) {
    float e0[3], e1[3];
    env_sample(base, N, dirs + (size_t)p * 3, e0);
    for (int c = 0; c < 3; c++) e[(size_t)p * 3 + c] = e0[c];
    const int x = p % w, y = p / w;
    if (y + 1 < h) {
      env_sample(base, N, dirs + (size_t)(p + w) * 3, e1);
      for (int c = 0; c < 3; c++) sv += (e1[c] - e0[c]) * (e1[c] - e0[c]);
    }
    if (x + 1 < w) {
      env_sample(base, N, dirs + (size_t)(p + 1) * 3, e1);
      for (int c = 0; c < 3; c++) sh += (e1[c] - e0[c]) * (e1[c] - e0[c]);
    }
  }
  sv = env_block_sum(sv, red);
  sh = env_block_sum(sh, red);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = sv;
    partials[2 * blockIdx.x + 1] = sh;
  }
}

// TV forward, second launch: one workgroup adds the partials in a fixed order, in double, and forms the two means
__global__ __launch_bounds__(ENV_BLOCK) void env_tv_finish_kernel(int h, int w, int nblk, const float *__restrict__ partials,
                                                                  float *__restrict__ loss) {
  __shared__ double red[2][ENV_BLOCK];
  double sv = 0.0, sh = 0.0;
  for (int i = threadIdx.x; i < nblk; i += ENV_BLOCK) {
    sv += (double)partials[2 * i];
    sh += (double)partials[2 * i + 1];
  }
  red[0][threadIdx.x] = sv;
  red[1][threadIdx.x] = sh;
  __syncthreads();
  for (int s = ENV_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0)
    loss[0] = (float)(red[0][0] / (3.0 * (double)(h - 1) * (double)w) + red[1][0] / (3.0 * (double)h * (double)(w - 1)));
}

// TV backward: d e of a sample from its four neighbours in e, through the sample's taps into the LDS window, one flush per
// workgroup (the reduction of texture_backward_kernel)
__global__ __launch_bounds__(PBR_BLOCK) void env_tv_backward_kernel(int N, int h, int w, const float *__restrict__ dirs,
                                                                    const float *__restrict__ e,
                                                                    const float *__restrict__ upstream, GradSpace gs, int per_wg) {
  extern __shared__ float lds[];
  const int lo = blockIdx.y * gs.win;
  win_zero(lds, gs.win);
  const int n = h * w;
  const float up = upstream[0];
  const float cv = up * (2.f / (3.f * (float)(h - 1) * (float)w)), chz = up * (2.f / (3.f * (float)h * (float)(w - 1)));
  const int p_begin = blockIdx.x * per_wg, p_end = min(n, p_begin + per_wg);
  for (int p = p_begin + threadIdx.x; p < p_end; p += blockDim.x) {
    const int x = p % w, y = p / w;
    float de[3];
    for (int c = 0; c < 3; c++) {
      const size_t o = (size_t)p * 3 + c;
      const float e0 = e[o];
      float v = 0.f, z = 0.f;
      if (y > 0) v += e0 - e[o - (size_t)w * 3];
      if (y + 1 < h) v -= e[o + (size_t)w * 3] - e0;
      if (x > 0) z += e0 - e[o - 3];
      if (x + 1 < w) z -= e[o + 3] - e0;
      de[c] = cv * v + chz * z;
    }
    Taps tp;
    if (!cube_footprint(dirs[(size_t)p * 3], dirs[(size_t)p * 3 + 1], dirs[(size_t)p * 3 + 2], N, tp)) continue;
    for (int k = 0; k < 4; k++)
      if (tp.t[k] >= 0)
        for (int c = 0; c < 3; c++) win_add(lds, lo, gs.win, tp.t[k] * 3 + c, tp.w[k] * de[c]);
  }
  win_flush(lds, lo, gs);
}

// cofactor (r, c) of the row-major 4 x 4 matrix a
__device__ __forceinline__ float cofactor4(const float *a, int r, int c) {
  int ri[3], ci[3];
  for (int i = 0, k = 0, l = 0; i < 4; i++) {
    if (i != r) ri[k++] = i;
    if (i != c) ci[l++] = i;
  }
  const float m00 = a[ri[0] * 4 + ci[0]], m01 = a[ri[0] * 4 + ci[1]], m02 = a[ri[0] * 4 + ci[2]];
  const float m10 = a[ri[1] * 4 + ci[0]], m11 = a[ri[1] * 4 + ci[1]], m12 = a[ri[1] * 4 + ci[2]];
  const float m20 = a[ri[2] * 4 + ci[0]], m21 = a[ri[2] * 4 + ci[1]], m22 = a[ri[2] * 4 + ci[2]];
  const float d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
  return ((r + c) & 1) ? -d : d;
}

constexpr int VD_PER_THREAD = 4;

// out[p] = -(R ray[p] / max(|ray[p]|, 1e-12)), R = the upper-left 3 x 3 block of inverse(wvt^T): the full 4 x 4 cofactor inverse,
// formed once per workgroup (ten cofactors on ten threads; a singular matrix gives non-finite directions)
__global__ __launch_bounds__(ENV_BLOCK) void view_dirs_kernel(int n, const float *__restrict__ rays,
                                                              const float *__restrict__ wvt, float *__restrict__ out) {
  __shared__ float a[16], cof[10], R[9];
  const int t = threadIdx.x;
  if (t < 16) a[t] = wvt[(t % 4) * 4 + t / 4];  // a = wvt^T
  __syncthreads();
  if (t < 10) cof[t] = t < 9 ? cofactor4(a, t / 3, t % 3) : cofactor4(a, 0, 3);
  __syncthreads();
  if (t < 9) {
    const float det = a[0] * cof[0] + a[1] * cof[1] + a[2] * cof[2] + a[3] * cof[9];
    R[t] = cof[(t % 3) * 3 + t / 3] / det;  // inverse[i][j] = cofactor[j][i] / det
  }
  __syncthreads();
  float r[9];
  for (int i = 0; i < 9; i++) r[i] = R[i];
  const size_t first = (size_t)blockIdx.x * (ENV_BLOCK * VD_PER_THREAD) + t;
  for (int k = 0; k < VD_PER_THREAD; k++) {
    const size_t p = first + (size_t)k * ENV_BLOCK;
    if (p >= (size_t)n) break;
    const float x = rays[p * 3], y = rays[p * 3 + 1], z = rays[p * 3 + 2];
    const float len = fmaxf(sqrtf(x * x + y * y + z * z), 1e-12f);
    const float nx = x / len, ny = y / len, nz = z / len;
    for (int i = 0; i < 3; i++) out[p * 3 + i] = -(nx * r[i * 3] + ny * r[i * 3 + 1] + nz * r[i * 3 + 2]);
  }
}

static bool env_base_ok(int N, size_t n) { return N >= 1 && N <= 4096 && n <= (size_t)1 << 30; }
static int env_tv_blocks(int h, int w) { return (h * w + ENV_BLOCK - 1) / ENV_BLOCK; }

}  // namespace gsr

extern "C" {

int gsr_pbr_env_grey(int base_n, const float *base, int n, const float *dirs, float *out, gsr_stream_t stream_) {
  using namespace gsr;
  if (!env_base_ok(base_n, n < 0 ? 0 : (size_t)n) || n < 0 || !base || (n > 0 && (!dirs || !out))) {
    set_error("gsr_pbr_env_grey: bad arguments (base [6][n][n][3], 1 <= n <= 4096; dirs [n][3]; out [n])");
    return GSR_EINVAL;
  }
  if (n == 0) return GSR_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(env_grey_kernel, dim3((n + ENV_BLOCK - 1) / ENV_BLOCK), dim3(ENV_BLOCK), 0, stream, base_n, base, n, dirs,
                     out);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

size_t gsr_pbr_env_tv_workspace_floats(int h, int w) {
  if (h < 1 || w < 1 || (size_t)h * (size_t)w > (size_t)1 << 28) return 0;
  return (size_t)h * w * 3 + 2 * (size_t)gsr::env_tv_blocks(h, w);
}

int gsr_pbr_env_tv_forward(int base_n, const float *base, int h, int w, const float *dirs, float *workspace, float *loss,
                           gsr_stream_t stream_) {
  using namespace gsr;
  if (h < 2 || w < 2 || (size_t)h * (size_t)w > (size_t)1 << 28 || !env_base_ok(base_n, 0) || !base || !dirs || !workspace ||
      !loss) {
    set_error("gsr_pbr_env_tv_forward: bad arguments (base [6][n][n][3], 1 <= n <= 4096; dirs [h][w][3], h, w >= 2)");
    return GSR_EINVAL;
  }
  const int nblk = env_tv_blocks(h, w);
  float *partials = workspace + (size_t)h * w * 3;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(env_tv_partial_kernel, dim3(nblk), dim3(ENV_BLOCK), 0, stream, base_n, base, h, w, dirs, workspace, partials);
  GSR_LAUNCH_CHECK(stream, 0);
  hipLaunchKernelGGL(env_tv_finish_kernel, dim3(1), dim3(ENV_BLOCK), 0, stream, h, w, nblk, partials, loss);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_env_tv_backward(int base_n, int h, int w, const float *dirs, const float *workspace, const float *upstream,
                            float *d_base, int reduce, gsr_stream_t stream_) {
  using namespace gsr;
  if (h < 2 || w < 2 || (size_t)h * (size_t)w > (size_t)1 << 28 || !env_base_ok(base_n, 0) || !dirs || !workspace || !upstream ||
      !d_base || reduce < 0 || reduce > 2) {
    set_error("gsr_pbr_env_tv_backward: bad arguments (dirs [h][w][3], h, w >= 2; reduce 0..2)");
    return GSR_EINVAL;
  }
  const int n = h * w;
  GradSpace gs{};
  gs.off[0] = 0;
  gs.ptr[0] = d_base;
  gs.off[1] = gs.total = 6 * base_n * base_n * 3;
  int nwg, groups, per_wg;
  bwd_grid(n, gs, nwg, groups, per_wg);  // GSR_PBR_ENV_TV_WINDOW: the split of texture_backward_kernel
  if (groups > 1 && reduce == GSR_PBR_ENV_TV_WHOLE) {
    set_error("gsr_pbr_env_tv_backward: the gradient of a base of %d does not fit in LDS (reduce = whole)", base_n);
    return GSR_EINVAL;
  }
  if (groups == 1 && reduce != GSR_PBR_ENV_TV_WINDOW) {  // the whole gradient in LDS: one pass of PBR_BLOCK samples per workgroup
    nwg = max(1, min(256, (n + PBR_BLOCK - 1) / PBR_BLOCK));
    per_wg = (n + nwg - 1) / nwg;
  }
  const size_t lds = (size_t)gs.win * sizeof(float);
  GSR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(env_tv_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(env_tv_backward_kernel, dim3(nwg, groups), dim3(PBR_BLOCK), lds, stream, base_n, h, w, dirs, workspace,
                     upstream, gs, per_wg);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

int gsr_pbr_view_dirs(int n, const float *rays, const float *world_view_transform, float *out, gsr_stream_t stream_) {
  using namespace gsr;
  if (n < 0 || (size_t)n > (size_t)1 << 30 || !world_view_transform || (n > 0 && (!rays || !out))) {
    set_error("gsr_pbr_view_dirs: bad arguments (rays [n][3], world_view_transform [4][4], out [n][3])");
    return GSR_EINVAL;
  }
  if (n == 0) return GSR_OK;
  const int per = ENV_BLOCK * VD_PER_THREAD;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(view_dirs_kernel, dim3((n + per - 1) / per), dim3(ENV_BLOCK), 0, stream, n, rays, world_view_transform, out);
  GSR_LAUNCH_CHECK(stream, 0);
  return GSR_OK;
}

}  // extern "C"
