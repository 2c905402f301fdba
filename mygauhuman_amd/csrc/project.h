// project.h -- the per-Gaussian projection device functions of the forward preprocess (geometry.hip), shared with the bake
// (bake.hip).  Every includer is built with -ffp-contract=off: one IEEE rounding per source-level operation, GLM's
// evaluation order written out term by term, so both produce the same bits.
#pragma once
#include "gsr_common.h"

namespace gsr {

__device__ __forceinline__ float3 xform4x3(const float3 p, const float *m) {
  return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                     m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 xform4x4(const float3 p, const float *m) {
  return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                     m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14], m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

// CR/auxiliary.h:41-44: double arithmetic, one rounding to float
__device__ __forceinline__ float ndc2pix(float v, int S) { return (float)(((v + 1.0) * S - 1.0) * 0.5); }

// Sigma = (S R)^T (S R) with the quaternion used as given (CR/forward.cu:118-152)
__device__ __forceinline__ void cov3d_from_scale_rot(const float3 sc, float mod, const float4 q, float *cov6) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  float R[3][3];
  R[0][0] = 1.f - 2.f * (y * y + z * z);
  R[0][1] = 2.f * (x * y - r * z);
  R[0][2] = 2.f * (x * z + r * y);
  R[1][0] = 2.f * (x * y + r * z);
  R[1][1] = 1.f - 2.f * (x * x + z * z);
  R[1][2] = 2.f * (y * z - r * x);
  R[2][0] = 2.f * (x * z - r * y);
  R[2][1] = 2.f * (y * z + r * x);
  R[2][2] = 1.f - 2.f * (x * x + y * y);
  const float s[3] = {mod * sc.x, mod * sc.y, mod * sc.z};
  float M[3][3];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int rr = 0; rr < 3; rr++) M[c][rr] = s[rr] * R[c][rr];
#define GSR_SIG(c, rr) (M[rr][0] * M[c][0] + M[rr][1] * M[c][1] + M[rr][2] * M[c][2])
  cov6[0] = GSR_SIG(0, 0);
  cov6[1] = GSR_SIG(0, 1);
  cov6[2] = GSR_SIG(0, 2);
  cov6[3] = GSR_SIG(1, 1);
  cov6[4] = GSR_SIG(1, 2);
  cov6[5] = GSR_SIG(2, 2);
#undef GSR_SIG
}

// EWA 2D covariance (CR/forward.cu:74-113); returns (a, b, c) with the 0.3 dilation
__device__ __forceinline__ float3 cov2d(const float3 mean, float fx, float fy, float tanx, float tany, const float *c6,
                                        const float *vm) {
  float3 t = xform4x3(mean, vm);
  const float limx = 1.3f * tanx, limy = 1.3f * tany;
  const float txtz = t.x / t.z, tytz = t.y / t.z;
  t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
  t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
  const float J00 = fx / t.z, J02 = -(fx * t.x) / (t.z * t.z);
  const float J11 = fy / t.z, J12 = -(fy * t.y) / (t.z * t.z);
  const float W0[3] = {vm[0], vm[4], vm[8]}, W1[3] = {vm[1], vm[5], vm[9]}, W2[3] = {vm[2], vm[6], vm[10]};
  float T0[3], T1[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    T0[r] = W0[r] * J00 + W2[r] * J02;
    T1[r] = W1[r] * J11 + W2[r] * J12;
  }
  const float V[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
  float A[3][2];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    A[c][0] = T0[0] * V[c][0] + T0[1] * V[c][1] + T0[2] * V[c][2];
    A[c][1] = T1[0] * V[c][0] + T1[1] * V[c][1] + T1[2] * V[c][2];
  }
  const float c00 = A[0][0] * T0[0] + A[1][0] * T0[1] + A[2][0] * T0[2];
  const float c01 = A[0][1] * T0[0] + A[1][1] * T0[1] + A[2][1] * T0[2];
  const float c11 = A[0][1] * T1[0] + A[1][1] * T1[1] + A[2][1] * T1[2];
  return make_float3(c00 + 0.3f, c01, c11 + 0.3f);
}

}  // namespace gsr
