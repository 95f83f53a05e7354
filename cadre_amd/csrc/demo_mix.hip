// demo_mix.hip — the demonstration term inside the PPO step (DAPG-style mixing): one loss launch for a minibatch that holds
// PPO rows and demonstration rows.
//
//   cadre_ppo_demo_loss   where cadre_ppo_loss_ord / cadre_bc_loss stand in the update: same addressing, grid, scratch protocol,
//                         poison and rank table.  row_kind [2][B] says per head which rows are PPO rows (0: the statements of
//                         ppo_loss_body, cadre_kernels.hip) and which are demonstration rows (1: the statements of
//                         bc_loss_kernel, imitation.hip, without the entropy term).  The row statements are restated here; the
//                         per-row bit-equality tests (tests/test_demo_mix_gpu.py) hold the copy to the two originals.
//   cadre_mix_row_kinds   row_kind[h][pos[h][u]] = (u >= B_ppo): the kinds of a minibatch whose unsorted rows B_ppo .. B - 1 are
//                         the demonstration rows, in the (possibly command-sorted) layout of the update
//
// Everything this file writes is written with plain vector stores or agent-scope atomics.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"
#include "kl_rule.h"
#include "ordinal.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)
#define MAX_NOUT 64

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

#define PPO_NSTAT 6
#define BC_NSTAT CADRE_BC_STATS_FIELDS
#define DM_NPART (2 + BC_NSTAT)       // demo partials per workgroup: value sum, cross-entropy sum, then the six statistics
struct mix_stats_t {
  float* row;           // [2 heads][F] PPO stats row of this step (STATS)
  int32_t F;
  float* part;          // [2 * nblk][PPO_NSTAT] per-workgroup partials
  float target_kl;      // > 0: KL gate armed
  int32_t* stop;        // sticky gate flag (may be NULL when the gate is off)
  float* demo_row;      // [2 heads][demo_F] demo stats row (NULL: no demo statistics)
  int32_t demo_F;
  float* demo_part;     // [2 * nblk][DM_NPART] per-workgroup demo partials (always: the two demo losses go through it)
};

// One wave per row (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups.  Up to the normalised logits lg, the
// probabilities pk, the entropy H and the log-prob lp the two kinds run the same statements; then a PPO row continues with
// ppo_loss_body's and a demonstration row with bc_loss_kernel's.  The PPO sums (and STATS) run over the PPO rows only, the
// demo sums over the demonstration rows only; the last arriver combines both sets in workgroup order.
template <bool STATS, bool HP>
__global__ __launch_bounds__(256) void ppo_demo_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                            int64_t ldv, int64_t v_ns, const int64_t* actions,
                                                            const int32_t* commands, const float* old_values,
                                                            const float* returns, const float* old_logp, const float* adv,
                                                            const int32_t* row_kind, int B, int C, int n_steer, int n_throttle,
                                                            double* hp, float clip, float value_coeff, float clip_coeff,
                                                            float ent_coeff, float inv_b, float eps, float demo_coeff,
                                                            float demo_value_coeff, float inv_bd, float* losses,
                                                            float* demo_losses, float* dlogits, float* dvalues, float* scratch,
                                                            const int32_t* poison, mix_stats_t so, const int32_t* ord) {
  if constexpr (HP) {
    clip = (float)hp[CADRE_HP_CLIP];
    value_coeff = (float)hp[CADRE_HP_VALUE_COEFF];
    clip_coeff = (float)hp[CADRE_HP_CLIP_COEFF];
    ent_coeff = (float)hp[CADRE_HP_ENT_COEFF];
    demo_coeff = (float)hp[CADRE_HP_DEMO_COEFF];
    demo_value_coeff = (float)hp[CADRE_HP_DEMO_VALUE_COEFF];
  }
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool dstats = so.demo_row != nullptr;
  __shared__ float red[3 + PPO_NSTAT + DM_NPART][4];
  float s_act = 0.f, s_val = 0.f, s_ent = 0.f;     // PPO rows; lane 0 of each wave
  float s_kl = 0.f, s_okl = 0.f, s_cf = 0.f, s_vcf = 0.f, s_r = 0.f, m_lr = 0.f;   // (STATS only)
  float d_val = 0.f, d_ce = 0.f;                   // demonstration rows
  float d_st[BC_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane, binv = lane;
  if (ordinal) {
    rk = lane < K ? ord[hd * 64 + lane] : lane;
    binv = ord_inverse(rk, lane);
  }
  const float t_off = eps / (float)K, t_on = (1.f - eps) + t_off;     // the smoothed target: off / on the demonstrated bin
  for (int i = 0; i < 4; ++i) {
    const int b = blockIdx.x * 16 + wave * 4 + i;
    if (b >= B) break;
    const int row = hd * B + b;                    // per-head sample arrays are [2][B]
    const int c = commands[row];
    const int64_t a64 = actions[row];
    const bool demo = row_kind[row] != 0;
    // a PPO row counts when its command is in range; a demonstration row also needs a bin of the head (-1: no label)
    const bool own_ok = c >= 0 && c < C && (!demo || (a64 >= 0 && a64 < K));
    for (int cc = 0; cc < C; ++cc) {
      if (own_ok && cc == c) continue;
      if (lane < ldl) dlogits[(int64_t)(hd * C + cc) * l_ns + (int64_t)b * ldl + lane] = 0.f;
      if (lane == 0) dvalues[(int64_t)(hd * C + cc) * v_ns + (int64_t)b * ldv] = 0.f;
    }
    if (!own_ok) continue;
    const int a = (int)a64;
    const int net = hd * C + c;
    const bool on = lane < K;
    float x = on ? logits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] : -INFINITY;
    float sg = 0.f, tg = 0.f;                      // (ordinal head) sigmoid(x), sigmoid(-x) of this lane's threshold unit
    if (ordinal) x = ord_logits(x, on, rk, lane, sg, tg);
    const float mx = wave_max(x);
    const float se = wave_sum(on ? expf(x - mx) : 0.f);
    const float lse = mx + logf(se);
    const float lg = x - lse;
    const float mx2 = wave_max(on ? lg : -INFINITY);
    const float e2 = on ? expf(lg - mx2) : 0.f;
    const float se2 = wave_sum(e2);
    const float pk = e2 / se2;
    const float H = -wave_sum(on ? pk * lg : 0.f);
    const float lp = __shfl(lg, a, 64);
    const float v = values[(int64_t)net * v_ns + (int64_t)b * ldv];
    const float R = returns[row];
    if (!demo) {
      // ---- a PPO row: ppo_loss_body
      const float A = adv[row], ov = old_values[row];
      const float ratio = expf(lp - old_logp[row]);
      const float s1 = ratio * A;
      const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
      const float s2 = rc * A;
      const float dv = v - ov;
      const float dvc = fminf(fmaxf(dv, -clip), clip);
      const float vpc = ov + dvc;
      const float vl = (v - R) * (v - R), vlc = (vpc - R) * (vpc - R);
      s_act += -fminf(s1, s2);
      s_val += fmaxf(vl, vlc);
      s_ent += H;
      if constexpr (STATS) {
        const float lr = lp - old_logp[row];          // log r (the exponent of `ratio` above)
        s_kl += (ratio - 1.f) - lr;                   // k3 estimator, >= 0
        s_okl += -lr;
        s_cf += fabsf(ratio - 1.f) > clip ? 1.f : 0.f;
        s_vcf += fabsf(dv) > clip ? 1.f : 0.f;
        s_r += ratio;
        m_lr = fmaxf(m_lr, fabsf(lr));
      }
      // ---- backward of total = vc*0.5*mean(max) + cc*mean(-min) - ec*mean(H)
      const bool in_ratio = ratio >= 1.f - clip && ratio <= 1.f + clip;
      float dmin_dr;                                 // d min(s1,s2) / d ratio (torch ties split 0.5/0.5)
      if (s1 < s2) dmin_dr = A;
      else if (s1 > s2) dmin_dr = in_ratio ? A : 0.f;
      else dmin_dr = 0.5f * A + (in_ratio ? 0.5f * A : 0.f);
      const float dlp = clip_coeff * inv_b * (-dmin_dr) * ratio;
      const bool in_v = dv >= -clip && dv <= clip;
      float dmax_dv;
      const float g1 = 2.f * (v - R), g2 = in_v ? 2.f * (vpc - R) : 0.f;
      if (vl > vlc) dmax_dv = g1;
      else if (vl < vlc) dmax_dv = g2;
      else dmax_dv = 0.5f * g1 + 0.5f * g2;
      if (lane == 0) dvalues[(int64_t)net * v_ns + (int64_t)b * ldv] = value_coeff * inv_b * 0.5f * dmax_dv;
      const float dH = -ent_coeff * inv_b;
      float gk = on ? dlp * ((lane == a ? 1.f : 0.f) - pk) + dH * (-pk * (lg + H)) : 0.f;
      if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
      if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
    } else {
      // ---- a demonstration row: bc_loss_kernel with bc_coeff = demo_coeff, value_coeff = demo_value_coeff, no entropy term
      const float tk = on ? (lane == a ? t_on : t_off) : 0.f;
      const float ce = -wave_sum(tk != 0.f ? tk * lg : 0.f);
      const float w = adv[row];                      // the row weight travels in the advantage slot
      const float dv = v - R;
      d_val += w * (dv * dv);
      d_ce += w * ce;
      if (dstats) {
        // top-1: the lowest index among the largest probabilities
        const float pm = wave_max(on ? pk : -1.f);
        const unsigned long long hit = __ballot(on && pk == pm);
        const int top = hit ? __ffsll((long long)hit) - 1 : -1;
        d_st[0] += top == a ? 1.f : 0.f;
        d_st[1] += -lp;
        d_st[2] += H;
        d_st[3] += fabsf(dv);
        d_st[4] += w;
        d_st[5] += 1.f;
      }
      const float wb = w * inv_bd;
      if (lane == 0) dvalues[(int64_t)net * v_ns + (int64_t)b * ldv] = demo_value_coeff * wb * dv;
      // d total / d logit_k = w inv_bd demo_coeff (p_k - t_k)   (sum_k t_k = 1)
      float gk = on ? wb * (demo_coeff * (pk - tk)) : 0.f;
      if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
      if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
    }
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_act; red[2][wave] = s_ent;
    red[3][wave] = s_kl; red[4][wave] = s_okl; red[5][wave] = s_cf;
    red[6][wave] = s_vcf; red[7][wave] = s_r; red[8][wave] = m_lr;
    red[9][wave] = d_val; red[10][wave] = d_ce;
#pragma unroll
    for (int k = 0; k < BC_NSTAT; ++k) red[11 + k][wave] = d_st[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nblk = gridDim.x, me = hd * nblk + blockIdx.x, total = 2 * nblk;
    float* part = scratch + 4;                      // [total][3]; scratch[0] is the arrival counter (zero on entry, reset below)
    const float tv = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const float ta = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const float te = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    __hip_atomic_store(part + 3 * me + 0, tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + 3 * me + 1, ta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + 3 * me + 2, te, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (STATS) {
      for (int k = 0; k < PPO_NSTAT; ++k) {
        const float* r = red[3 + k];
        const float t = k == 5 ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
        __hip_atomic_store(so.part + PPO_NSTAT * me + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    for (int k = 0; k < (dstats ? DM_NPART : 2); ++k) {
      const float* r = red[9 + k];
      __hip_atomic_store(so.demo_part + DM_NPART * me + k, (r[0] + r[1]) + (r[2] + r[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(scratch), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (unsigned)(total - 1)) {          // last arriver: every partial has been published
      float sv = 0.f, sa = 0.f, sn = 0.f;
      for (int w = 0; w < total; ++w) {             // workgroup order: equal inputs give equal bits
        sv += __hip_atomic_load(part + 3 * w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sa += __hip_atomic_load(part + 3 * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sn += __hip_atomic_load(part + 3 * w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      float dsv = 0.f, dsc = 0.f;
      for (int w = 0; w < total; ++w) {
        dsv += __hip_atomic_load(so.demo_part + DM_NPART * w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dsc += __hip_atomic_load(so.demo_part + DM_NPART * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const float bad = (poison && __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? __builtin_nanf("") : 0.f;
      losses[0] = value_coeff * 0.5f * sv * inv_b + bad;
      losses[1] = clip_coeff * sa * inv_b + bad;
      losses[2] = ent_coeff * sn * inv_b + bad;
      demo_losses[0] = demo_coeff * dsc * inv_bd + bad;
      demo_losses[1] = demo_value_coeff * 0.5f * dsv * inv_bd + bad;
      if (dstats) {
        for (int h = 0; h < 2; ++h) {
          float t[BC_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < BC_NSTAT; ++k)
              t[k] += __hip_atomic_load(so.demo_part + DM_NPART * w + 2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          float* o = so.demo_row + h * so.demo_F;
          for (int k = 0; k < BC_NSTAT; ++k) o[k] = t[k] * inv_bd;
        }
      }
      if constexpr (STATS) {
        // per head, partials in workgroup order; means over inv_b (the PPO losses' denominator), PPO rows only
        float kl[2];
        for (int h = 0; h < 2; ++h) {
          float t[PPO_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < PPO_NSTAT; ++k) {
              const float x = __hip_atomic_load(so.part + PPO_NSTAT * w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              t[k] = k == 5 ? fmaxf(t[k], x) : t[k] + x;
            }
          float* o = so.row + h * so.F;
          for (int k = 0; k < 5; ++k) o[k] = t[k] * inv_b;
          o[5] = t[5];
          kl[h] = t[0] * inv_b;
        }
        // the gate, `applied` and (HP) the KL-adaptive lr: the rule of kl_rule.h on the KL of the PPO rows
        if constexpr (HP) cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, hp[CADRE_HP_DESIRED_KL], hp);
        else cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, 0.0, nullptr);
      }
      __hip_atomic_store(reinterpret_cast<unsigned*>(scratch), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// row_kind[h][pos[h][u]] = (u >= B_ppo); pos NULL: the identity.  A position outside 0 .. B - 1 writes nothing.
__global__ __launch_bounds__(256) void mix_row_kinds_kernel(const int32_t* pos, int B, int B_ppo, int32_t* row_kind) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x, hd = blockIdx.y;
  if (u >= B) return;
  const int d = pos ? pos[hd * B + u] : u;
  if (d >= 0 && d < B) row_kind[hd * B + d] = u >= B_ppo ? 1 : 0;
}

}  // namespace

extern "C" int cadre_ppo_demo_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                                   int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values,
                                   const float* returns, const float* old_logp, const float* adv, const int32_t* row_kind,
                                   int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip,
                                   float value_coeff, float clip_coeff, float ent_coeff, float inv_b, float label_smoothing,
                                   float demo_coeff, float demo_value_coeff, float inv_bd, float* losses, float* demo_losses,
                                   float* dlogits, float* dvalues, float* scratch, float* demo_scratch, const int32_t* poison,
                                   float* stats_row, int32_t F, float* stats_scratch, float target_kl, int32_t* stop,
                                   float* demo_stats_row, int32_t demo_F, const int32_t* ord, void* stream) {
  FAIL_IF(!logits || !values || !actions || !commands || !old_values || !returns || !old_logp || !adv || !losses ||
              !demo_losses || !dlogits || !dvalues || !scratch || !demo_scratch || B < 1 || C < 1 || n_out_steer < 1 ||
              n_out_steer > MAX_NOUT || n_out_throttle < 1 || n_out_throttle > MAX_NOUT || ldl < n_out_steer ||
              ldl < n_out_throttle || ldl > 64,
          "cadre_ppo_demo_loss: bad argument");
  FAIL_IF(!row_kind, "cadre_ppo_demo_loss: null row_kind (device int32 [2][B]; 0 a PPO row, 1 a demonstration row)");
  FAIL_IF(!(label_smoothing >= 0.f && label_smoothing < 1.f), "cadre_ppo_demo_loss: label_smoothing must be in [0, 1)");
  FAIL_IF(stats_row && (F < CADRE_PPO_STATS_FIELDS || !stats_scratch || !(target_kl >= 0.f) || (target_kl > 0.f && !stop)),
          "cadre_ppo_demo_loss: bad stats argument (F >= CADRE_PPO_STATS_FIELDS, target_kl >= 0, a stop flag with target_kl > 0)");
  FAIL_IF(demo_stats_row && demo_F < CADRE_BC_STATS_FIELDS, "cadre_ppo_demo_loss: bad demo stats argument (demo_F >= CADRE_BC_STATS_FIELDS)");
  FAIL_IF(hp && ((uintptr_t)hp & 7), "cadre_ppo_demo_loss: bad hyper-parameter block (device double[CADRE_HP_FIELDS], 8-byte aligned)");
  // inv_bd scales the demo losses, gradients and statistics: with the scalars in the block it is always needed
  const bool needs_bd = hp || demo_coeff != 0.f || demo_value_coeff != 0.f || demo_stats_row;
  FAIL_IF(needs_bd && !(isfinite(inv_bd) && inv_bd > 0.f), "cadre_ppo_demo_loss: inv_bd must be finite and > 0 (1 / demonstration rows per step)");
  const mix_stats_t so{stats_row, F, stats_scratch, target_kl, stop, demo_stats_row, demo_F, demo_scratch};
  const dim3 grid((B + 15) / 16, 2), block(256);
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
#define CADRE_MIX_LAUNCH(S_, H_)                                                                                               \
  hipLaunchKernelGGL((ppo_demo_loss_kernel<S_, H_>), grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, \
                     commands, old_values, returns, old_logp, adv, row_kind, B, C, n_out_steer, n_out_throttle, hp, clip,      \
                     value_coeff, clip_coeff, ent_coeff, inv_b, label_smoothing, demo_coeff, demo_value_coeff, inv_bd, losses, \
                     demo_losses, dlogits, dvalues, scratch, poison, so, ord)
  if (stats_row && hp) CADRE_MIX_LAUNCH(true, true);
  else if (stats_row) CADRE_MIX_LAUNCH(true, false);
  else if (hp) CADRE_MIX_LAUNCH(false, true);
  else CADRE_MIX_LAUNCH(false, false);
#undef CADRE_MIX_LAUNCH
  return (int)hipGetLastError();
}

extern "C" int cadre_mix_row_kinds(const int32_t* pos, int32_t B, int32_t B_ppo, int32_t* row_kind, void* stream) {
  FAIL_IF(!row_kind || B < 1, "cadre_mix_row_kinds: bad argument");
  FAIL_IF(B_ppo < 0 || B_ppo > B, "cadre_mix_row_kinds: B_ppo must be in 0 .. B");
  hipLaunchKernelGGL(mix_row_kinds_kernel, dim3((B + 255) / 256, 2), dim3(256), 0, ST(stream), pos, B, B_ppo, row_kind);
  return (int)hipGetLastError();
}
