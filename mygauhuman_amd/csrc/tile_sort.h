// tile_sort.h -- the per-tile list sort shared by the binning (binning_bucket.hip) and the plain blend forward (blend_fwd.hip),
// which sorts the short lists of its own tile in its prologue (Options::blend_sort).
#pragma once
#include "gsr_common.h"

namespace gsr {

constexpr int SORT_WAVE_MAX = 512;  // longest list sorted as runs of 64 + rank merge (one wave, or the forward's workgroup); longer ones: bucket_sort_kernel

// ---- sort by runs + rank merge (lists of 65 .. 512 keys) ---------------------------------------------------------------
// A full bitonic network over NREG x 64 keys costs log^2 stages over every register and needs a power-of-two size: a tile with
// 260 keys pays for 512.  Here every register is sorted ACROSS THE LANES as its own run of 64 (21 stages, all runs in lockstep),
// the runs go to LDS, and each key finds its final position as  lane + sum over the other runs of (keys smaller than it)  by a
// binary search per run (keys are unique: they contain the Gaussian id).  Work grows with the number of runs actually needed
// (5 runs for 260 keys), not with the next power of two; at C3 (lists of ~240, up to 355) this is ~2x fewer instructions.
constexpr int MERGE_MAX_RUNS = 8;

template <int J>
__device__ __forceinline__ uint64_t lane_xor_u64(uint64_t v) {
  uint32_t lo, hi;
  if constexpr (J < 32) {  // ds_swizzle bit-mode: lane ^ J inside each group of 32
    lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)v, (J << 10) | 0x1F);
    hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(v >> 32), (J << 10) | 0x1F);
  } else {
    lo = (uint32_t)__shfl_xor((int)(uint32_t)v, J, WAVE);
    hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), J, WAVE);
  }
  return ((uint64_t)hi << 32) | lo;
}
// one compare-exchange stage (block size K, distance J) of an ASCENDING bitonic sort of 64 keys held one per lane
template <int NRUN, int K, int J>
__device__ __forceinline__ void run_stage(uint64_t (&key)[NRUN], uint32_t lane) {
  const bool take_min = ((lane & (uint32_t)J) == 0) == ((lane & (uint32_t)K) == 0 || K == WAVE);
#pragma unroll
  for (int r = 0; r < NRUN; r++) {
    const uint64_t mine = key[r], other = lane_xor_u64<J>(mine);
    key[r] = take_min ? (mine < other ? mine : other) : (mine > other ? mine : other);
  }
}
template <int NRUN, int K, int J>
__device__ __forceinline__ void run_merge(uint64_t (&key)[NRUN], uint32_t lane) {
  run_stage<NRUN, K, J>(key, lane);
  if constexpr (J > 1) run_merge<NRUN, K, J / 2>(key, lane);
}
template <int NRUN, int K>
__device__ __forceinline__ void run_levels(uint64_t (&key)[NRUN], uint32_t lane) {
  run_merge<NRUN, K, K / 2>(key, lane);
  if constexpr (K < WAVE) run_levels<NRUN, K * 2>(key, lane);
}

// position of key k among the keys of one sorted run of 64 (keys are unique; the padding ~0 is never smaller): branch-free, so the
// searches of a key in several runs (and of a lane's other keys) are independent chains of LDS reads the scheduler can overlap
__device__ __forceinline__ uint32_t rank_in_run(const uint64_t *run, uint64_t k) {
  uint32_t c = 0u;
#pragma unroll
  for (int step = WAVE / 2; step >= 1; step >>= 1) c += run[c + step - 1] < k ? (uint32_t)step : 0u;
  return run[WAVE - 1] < k ? (uint32_t)WAVE : c;  // whole run smaller?
}

}  // namespace gsr
