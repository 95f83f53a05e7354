// consensus.hip — the two decisions several data-parallel ranks must take identically, each from numbers that were summed
// over the ranks beforehand (one small all-reduce, Shared_grad_buffers.all_reduce_small): every rank runs the same kernel on
// the same reduced bits and therefore writes the same stop flag, learning rate and reward scale.
//
//   cadre_kl_consensus        the target_kl gate and the KL-adaptive learning rate of one optimiser step (the rule of
//                             kl_rule.h, which the loss kernel applies to its own rank's KL when no consensus is asked for)
//   cadre_return_scale_merge  the reward scale from the per-rank return statistics (Chan's merge in rank order)
//
// Both are one workgroup with one deciding lane per output; everything is written with plain stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"
#include "kl_rule.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

__global__ __launch_bounds__(64) void kl_consensus_kernel(const float* kl, float target_kl, int32_t* stop, double desired,
                                                          double* hp, float* row, int32_t F) {
  if (threadIdx.x != 0) return;
  cadre_kl_rule(kl[0], kl[1], target_kl, stop, row, F, desired, hp);
}

// lane = head.  The merge of return_stats_kernel (rollout_finish.hip) with ranks in place of storages, from an empty
// accumulator; a rank that has seen no return yet (count 0) is skipped, so its mean and M2 slots are never read into the sum.
__global__ __launch_bounds__(64) void return_scale_merge_kernel(const double* stats, int world, double epsilon, double* state,
                                                                double* merged) {
#pragma clang fp contract(off)
  const int h = threadIdx.x;
  if (h >= 2) return;
  double cnt = 0.0, mu = 0.0, m2 = 0.0;
  for (int r = 0; r < world; ++r) {
    const double* s = stats + 6 * (int64_t)r + 3 * h;
    const double nb = s[0], mk = s[1], qk = s[2];
    if (!(nb > 0.0)) continue;
    const double tot = cnt + nb, delta = mk - mu;
    mu = mu + delta * nb / tot;
    m2 = m2 + qk + delta * delta * cnt * nb / tot;
    cnt = tot;
  }
  if (merged) {
    merged[3 * h] = cnt;
    merged[3 * h + 1] = mu;
    merged[3 * h + 2] = m2;
  }
  if (cnt > 0.0) state[CADRE_RS_SCALE + h] = (double)(float)(1.0 / sqrt(m2 / cnt + epsilon));
}

}  // namespace

extern "C" int cadre_kl_consensus(const float* kl, float target_kl, int32_t* stop, double desired_kl, double* hp,
                                  float* stats_row, int32_t F, void* stream) {
  FAIL_IF(!kl, "cadre_kl_consensus: null operand (kl: the two reduced approx_kl values)");
  FAIL_IF(!(target_kl >= 0.f) || (target_kl > 0.f && !stop),
          "cadre_kl_consensus: bad argument (target_kl >= 0, a stop flag with target_kl > 0)");
  FAIL_IF(desired_kl > 0.0 && (!hp || ((uintptr_t)hp & 7)),
          "cadre_kl_consensus: desired_kl > 0 needs the hyper-parameter block (device double[CADRE_HP_FIELDS], 8-byte aligned)");
  FAIL_IF(stats_row && F < CADRE_PPO_STATS_FIELDS, "cadre_kl_consensus: bad stats row (F >= CADRE_PPO_STATS_FIELDS)");
  hipLaunchKernelGGL(kl_consensus_kernel, dim3(1), dim3(64), 0, ST(stream), kl, target_kl, stop, desired_kl, hp, stats_row, F);
  return (int)hipGetLastError();
}

extern "C" int cadre_return_scale_merge(const double* stats, int32_t world, double epsilon, double* state, double* merged,
                                        void* stream) {
  FAIL_IF(!stats || !state, "cadre_return_scale_merge: null operand");
  FAIL_IF(world < 1 || !(epsilon >= 0.0) || !(epsilon < INFINITY),
          "cadre_return_scale_merge: bad argument (world >= 1, finite epsilon >= 0)");
  hipLaunchKernelGGL(return_scale_merge_kernel, dim3(1), dim3(64), 0, ST(stream), stats, (int)world, epsilon, state, merged);
  return (int)hipGetLastError();
}
