// kl_rule.h — what one optimiser step decides from its approximate KL, stated once: the target_kl gate and the KL-adaptive
// learning rate.  Called by the loss kernel's last arriving workgroup (cadre_kernels.hip, ppo_loss_body: the KL of this rank's
// minibatch) and by cadre_kl_consensus (consensus.hip: the KL summed over the ranks), by ONE lane.
//
//   stopped = *stop (sticky: only the caller clears it);  target_kl > 0 and fmaxf(kl0, kl1) > 1.5f * target_kl sets it
//   row (may be NULL): applied = !stopped goes into field 6 of both heads of the stats row [2][F]
//   hp (may be NULL) and desired > 0 and not stopped, with k = max(kl0, kl1) as double, all in double:
//     k > 2 desired:        hp[LR] = max(hp[LR_MIN], hp[LR] / hp[LR_FACTOR])
//     0 < k < desired / 2:  hp[LR] = min(hp[LR_MAX], hp[LR] * hp[LR_FACTOR])
//
// NaN: fmaxf / fmax return the other operand when one is NaN, so a head whose KL is NaN is ignored; when both are NaN every
// comparison is false: the flag is not set and lr does not move.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"

__device__ __forceinline__ void cadre_kl_rule(float kl0, float kl1, float target_kl, int32_t* stop, float* row, int32_t F,
                                              double desired, double* hp) {
  int32_t stopped = stop ? __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
  if (stop && target_kl > 0.f && fmaxf(kl0, kl1) > 1.5f * target_kl) stopped = 1;
  if (stop) __hip_atomic_store(stop, stopped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (row) {
    row[6] = stopped ? 0.f : 1.f;                   // applied: the optimiser step of this minibatch runs
    row[F + 6] = row[6];
  }
  if (hp) {
    // KL-adaptive lr (the rsl_rl / RL-Games rule), all in double; the optimiser step of THIS minibatch reads the result
    if (desired > 0.0 && !stopped) {
      const double k = fmax((double)kl0, (double)kl1);
      double lr = hp[CADRE_HP_LR];
      if (k > 2.0 * desired) lr = fmax(hp[CADRE_HP_LR_MIN], lr / hp[CADRE_HP_LR_FACTOR]);
      else if (k > 0.0 && k < desired / 2.0) lr = fmin(hp[CADRE_HP_LR_MAX], lr * hp[CADRE_HP_LR_FACTOR]);
      hp[CADRE_HP_LR] = lr;
    }
  }
}
