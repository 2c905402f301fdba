// ssim_window.h -- what the SSIM kernels share (ssim.hip, ssim_crop.hip): the tile geometry and the 11-tap window.
#pragma once
#include "gsr_common.h"

namespace gsr {

constexpr int SS_T = 16, SS_R = 5, SS_IN = SS_T + 2 * SS_R;  // tile, window radius, staged extent (26)

struct SsimWindow {
  float w[11];
};
// gaussian(11, 1.5) normalised (utils/loss_utils.py:25-27), evaluated in double on the host like the reference's Python floats;
// the eleven weights are meant to be the reference's bit for bit.  tests/test_image_loss_reference_host.py holds the numpy restatement
// (image_loss_reference.window()) to torch's bits; this function is covered through the kernels only, which reproduce the float32
// restatement built on those weights bit for bit (tests/test_gpu_image_loss_f64.py)
static SsimWindow make_window() {
  SsimWindow s;
  // the reference builds a float32 tensor of the unnormalised values on the CPU, then divides by its float32 sum.  torch's sum of
  // these eleven values is their exact sum rounded once (3.7592327594757080); adding them one after the other in float32 lands
  // one ulp below it (3.7592325210571289) and scales every weight by 1 + 6e-8, so the sum is taken in double and rounded once.
  float gf[11];
  double sum = 0.0;
  for (int i = 0; i < 11; i++) {
    gf[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    sum += (double)gf[i];
  }
  const float sf = (float)sum;
  for (int i = 0; i < 11; i++) s.w[i] = gf[i] / sf;
  return s;
}

}  // namespace gsr
