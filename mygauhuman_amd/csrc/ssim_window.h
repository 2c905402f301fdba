// ssim_window.h -- what the SSIM kernels share (ssim.hip, ssim_crop.hip): the tile geometry and the 11-tap window.
#pragma once
#include "gsr_common.h"

namespace gsr {

constexpr int SS_T = 16, SS_R = 5, SS_IN = SS_T + 2 * SS_R;  // tile, window radius, staged extent (26)

struct SsimWindow {
  float w[11];
};
// gaussian(11, 1.5) normalised (utils/loss_utils.py:25-27), evaluated in double on the host like the reference's Python floats
static SsimWindow make_window() {
  SsimWindow s;
  double g[11], sum = 0.0;
  for (int i = 0; i < 11; i++) {
    g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    sum += g[i];
  }
  // the reference builds a float32 tensor of the unnormalised values, then divides by their float32 sum
  float gf[11], sf = 0.f;
  for (int i = 0; i < 11; i++) gf[i] = (float)g[i];
  for (int i = 0; i < 11; i++) sf += gf[i];
  for (int i = 0; i < 11; i++) s.w[i] = gf[i] / sf;
  (void)sum;
  return s;
}

}  // namespace gsr
