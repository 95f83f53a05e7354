// selfimit.hip — self-imitation learning (Oh et al. 2018) inside the PPO step: prioritised rows of the agent's own past
// rollouts ride behind the workers' rows, and one loss launch treats each row by its kind.
//
//   cadre_ppo_sil_loss   where cadre_ppo_loss_ord / cadre_ppo_demo_loss stand in the update: same addressing, grid, scratch
//                        protocol, poison and rank table.  row_kind [2][B] (cadre_mix_row_kinds, demo_mix.hip) says per head
//                        which rows are PPO rows (0: the statements of ppo_loss_body, cadre_kernels.hip, restated as in
//                        demo_mix.hip) and which are SIL rows (1: w = max(R - v, 0), policy term -lp w, value term 0.5 w^2).
//   cadre_sil_prepare    per append: realised returns, closed / eligible flags and the first priorities of a slot's storages
//   cadre_sil_draw       the prioritised draw: integer prefix sums of the priority table, then one search per draw
//   cadre_sil_scatter    after a step: the priorities of the drawn rows from the w that step computed
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
#define SIL_NSTAT CADRE_SIL_STATS_FIELDS
#define SL_NPART (2 + SIL_NSTAT)      // SIL partials per workgroup: policy sum, value sum, then the six statistics
struct sil_stats_t {
  float* row;           // [2 heads][F] PPO stats row of this step (STATS)
  int32_t F;
  float* part;          // [2 * nblk][PPO_NSTAT] per-workgroup partials
  float target_kl;      // > 0: KL gate armed
  int32_t* stop;        // sticky gate flag (may be NULL when the gate is off)
  float* sil_row;       // [2 heads][sil_F] SIL stats row (NULL: no SIL statistics)
  int32_t sil_F;
  float* sil_part;      // [2 * nblk][SL_NPART] per-workgroup SIL partials (always: the two SIL losses go through it)
};

// One wave per row (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups, as ppo_demo_loss_kernel.  Up to the normalised
// logits lg, the probabilities pk, the entropy H and the log-prob lp the two kinds run the same statements; then a PPO row
// continues with ppo_loss_body's and a SIL row with the self-imitation terms.  The PPO sums (and STATS) run over the PPO rows
// only, the SIL sums over the SIL rows only; the last arriver combines both sets in workgroup order.
template <bool STATS, bool HP>
__global__ __launch_bounds__(256) void ppo_sil_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                           int64_t ldv, int64_t v_ns, const int64_t* actions,
                                                           const int32_t* commands, const float* old_values,
                                                           const float* returns, const float* old_logp, const float* adv,
                                                           const int32_t* row_kind, int B, int C, int n_steer, int n_throttle,
                                                           double* hp, float clip, float value_coeff, float clip_coeff,
                                                           float ent_coeff, float inv_b, float sil_coeff, float sil_value_coeff,
                                                           float inv_bs, float* losses, float* sil_losses, float* sil_w,
                                                           float* dlogits, float* dvalues, float* scratch,
                                                           const int32_t* poison, sil_stats_t so, const int32_t* ord) {
  if constexpr (HP) {
    clip = (float)hp[CADRE_HP_CLIP];
    value_coeff = (float)hp[CADRE_HP_VALUE_COEFF];
    clip_coeff = (float)hp[CADRE_HP_CLIP_COEFF];
    ent_coeff = (float)hp[CADRE_HP_ENT_COEFF];
    sil_coeff = (float)hp[CADRE_HP_SIL_COEFF];
    sil_value_coeff = (float)hp[CADRE_HP_SIL_VALUE_COEFF];
  }
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool sstats = so.sil_row != nullptr;
  __shared__ float red[3 + PPO_NSTAT + SL_NPART][4];
  float s_act = 0.f, s_val = 0.f, s_ent = 0.f;     // PPO rows; lane 0 of each wave
  float s_kl = 0.f, s_okl = 0.f, s_cf = 0.f, s_vcf = 0.f, s_r = 0.f, m_lr = 0.f;   // (STATS only)
  float q_pol = 0.f, q_val = 0.f;                  // SIL rows
  float q_st[SIL_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane, binv = lane;
  if (ordinal) {
    rk = lane < K ? ord[hd * 64 + lane] : lane;
    binv = ord_inverse(rk, lane);
  }
  for (int i = 0; i < 4; ++i) {
    const int b = blockIdx.x * 16 + wave * 4 + i;
    if (b >= B) break;
    const int row = hd * B + b;                    // per-head sample arrays are [2][B]
    const int c = commands[row];
    const int64_t a64 = actions[row];
    const bool sil = row_kind[row] != 0;
    // a PPO row counts when its command is in range; a SIL row also needs a bin of the head
    const bool own_ok = c >= 0 && c < C && (!sil || (a64 >= 0 && a64 < K));
    for (int cc = 0; cc < C; ++cc) {
      if (own_ok && cc == c) continue;
      if (lane < ldl) dlogits[(int64_t)(hd * C + cc) * l_ns + (int64_t)b * ldl + lane] = 0.f;
      if (lane == 0) dvalues[(int64_t)(hd * C + cc) * v_ns + (int64_t)b * ldv] = 0.f;
    }
    if (!own_ok) {
      if (lane == 0) sil_w[row] = 0.f;
      continue;
    }
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
    if (!sil) {
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
      if (lane == 0) sil_w[row] = 0.f;
    } else {
      // ---- a SIL row: total += sil_coeff mean(-lp w) + sil_value_coeff mean(0.5 w^2), w = max(R - v, 0) a constant in the
      // policy term; no entropy term, no ratio
      const float dR = R - v;
      const float w = fmaxf(dR, 0.f);
      q_pol += -lp * w;
      q_val += w * w;
      if (sstats) {
        q_st[0] += w;
        q_st[1] += w > 0.f ? 1.f : 0.f;
        q_st[2] += -lp;
        q_st[3] += fabsf(dR);
        q_st[4] = fmaxf(q_st[4], w);
        q_st[5] += 1.f;
      }
      if (lane == 0) {
        sil_w[row] = w;
        dvalues[(int64_t)net * v_ns + (int64_t)b * ldv] = -(sil_value_coeff * inv_bs * w);
      }
      // d total / d logit_k = sil_coeff inv_bs w (p_k - [k = a])
      const float gw = sil_coeff * inv_bs * w;
      float gk = on ? gw * (pk - (lane == a ? 1.f : 0.f)) : 0.f;
      if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
      if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
    }
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_act; red[2][wave] = s_ent;
    red[3][wave] = s_kl; red[4][wave] = s_okl; red[5][wave] = s_cf;
    red[6][wave] = s_vcf; red[7][wave] = s_r; red[8][wave] = m_lr;
    red[9][wave] = q_pol; red[10][wave] = q_val;
#pragma unroll
    for (int k = 0; k < SIL_NSTAT; ++k) red[11 + k][wave] = q_st[k];
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
    for (int k = 0; k < (sstats ? SL_NPART : 2); ++k) {
      const float* r = red[9 + k];
      const float t = k == 2 + 4 ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
      __hip_atomic_store(so.sil_part + SL_NPART * me + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
      float qp = 0.f, qv = 0.f;
      for (int w = 0; w < total; ++w) {
        qp += __hip_atomic_load(so.sil_part + SL_NPART * w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        qv += __hip_atomic_load(so.sil_part + SL_NPART * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const float bad = (poison && __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? __builtin_nanf("") : 0.f;
      losses[0] = value_coeff * 0.5f * sv * inv_b + bad;
      losses[1] = clip_coeff * sa * inv_b + bad;
      losses[2] = ent_coeff * sn * inv_b + bad;
      sil_losses[0] = sil_coeff * qp * inv_bs + bad;
      sil_losses[1] = sil_value_coeff * 0.5f * qv * inv_bs + bad;
      if (sstats) {
        for (int h = 0; h < 2; ++h) {
          float t[SIL_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < SIL_NSTAT; ++k) {
              const float x = __hip_atomic_load(so.sil_part + SL_NPART * w + 2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              t[k] = k == 4 ? fmaxf(t[k], x) : t[k] + x;
            }
          float* o = so.sil_row + h * so.sil_F;
          for (int k = 0; k < 4; ++k) o[k] = t[k] * inv_bs;
          o[4] = t[4];
          o[5] = t[5];
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

// ---------------------------------------------------------------------------- priorities
// q = clamp(floor((w + eps)^alpha 2^16), 1, 2^31 - 1); the power in double (one thread per row, off the hot path).  alpha == 1
// (proportional priorities) takes no power: pow(x, 1) of the device library is not exact, and w = 1 must give 2^16.
__device__ __forceinline__ uint32_t sil_quantise(float w, double eps, double alpha) {
  const double b = (double)w + eps;
  const double x = floor((alpha == 1.0 ? b : pow(b, alpha)) * 65536.0);
  if (!(x >= 1.0)) return 1u;
  if (x > 2147483647.0) return 2147483647u;
  return (uint32_t)x;
}

struct sil_prep_row_t {
  const float* rewards; const float* masks; const float* time_limits; const float* value_preds;
  float* returns; int32_t* flags; uint32_t* q;
};
constexpr int MAX_T = 3000;      // 4 (T + 1) floats of LDS

// One workgroup per storage.  The scan is gae_multi_kernel's (rollout_finish.hip) with tau = 1 and V = 0, statement for
// statement, FMA contraction off: delta = r, gae = delta + (gamma m) gae, gae = gae * keep, ret = gae + 0.  tail == 1 differs
// only where a chain starts: at row T with value_preds[T] and at a time-limit row with value_preds[t] in the place of 0, which
// a closing row (m == 0) multiplies away.
__global__ __launch_bounds__(64) void sil_prepare_kernel(const sil_prep_row_t* rows, int T, float gamma, const double* state,
                                                         float clip_r, int tail, double alpha, double eps) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  float* r = sm, *m = sm + (T + 1), *keep = m + (T + 1), *ret = keep + (T + 1);
  const int k = blockIdx.x, lane = threadIdx.x;
  const sil_prep_row_t g = rows[k];
  const float scale = state ? (float)state[CADRE_RS_SCALE + (k & 1)] : 1.f;
  for (int i = lane; i <= T; i += 64) {
    float x = g.rewards[i];
    if (state) {
      x = (x * scale);
      x = fminf(fmaxf(x, -clip_r), clip_r);
    }
    r[i] = x;
    m[i] = g.masks[i];
    keep[i] = g.time_limits ? (1.f - g.time_limits[i]) : 1.f;
  }
  __syncthreads();
  if (lane == 0) {
    float gae = tail ? g.value_preds[T] : 0.f;
    bool closed = false;
    for (int t = T - 1; t >= 0; --t) {
      const float t1 = (gamma * 0.f);             // V[t + 1] = 0
      const float t2 = (t1 * m[t]);
      const float t3 = (r[t] + t2);
      const float delta = (t3 - 0.f);
      const float u1 = (gamma * m[t]);
      const float u2 = (u1 * gae);
      gae = (delta + u2);
      gae = (gae * keep[t]);
      if (keep[t] != 1.f) {                       // a time-limit flag, read as the scan reads it
        closed = false;
        closed = false;
        if (tail) gae = g.value_preds[t];
      } else if (m[t] == 0.f) {
        closed = true;
      }
      ret[t] = (gae + 0.f);
      r[t] = closed ? 1.f : 0.f;                  // (r[t] has been consumed)
    }
  }
  __syncthreads();
  for (int i = lane; i < T; i += 64) {
    const bool closed = r[i] != 0.f;
    const bool elig = closed || tail != 0;
    const float R = ret[i];
    g.returns[i] = R;
    g.flags[i] = (closed ? 1 : 0) | (elig ? 2 : 0);
    const float w = fmaxf(R - g.value_preds[i], 0.f);
    g.q[i] = elig ? sil_quantise(w, eps, alpha) : 0u;
  }
  if (lane == 0) {
    g.flags[T] = 0;
    g.q[T] = 0u;
  }
}

// ---------------------------------------------------------------------------- the draw
constexpr int SIL_CH = 1024;     // rows per block sum

__global__ __launch_bounds__(256) void sil_block_sums_kernel(const uint32_t* q, int64_t Rcap, int64_t nfill, int nblk,
                                                             unsigned long long* bsum) {
  __shared__ unsigned long long s[256];
  const int blk = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x;
  const int64_t r0 = (int64_t)blk * SIL_CH + tid * 4;
  unsigned long long t = 0;
  for (int j = 0; j < 4; ++j) {
    const int64_t r = r0 + j;
    if (r < nfill) t += q[hd * Rcap + r];
  }
  s[tid] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  if (tid == 0) bsum[(int64_t)hd * nblk + blk] = s[0];
}

// bpre[h][i] = sum of bsum[h][0 .. i - 1], i = 0 .. nblk (the last entry is the head's total)
__global__ __launch_bounds__(256) void sil_scan_blocks_kernel(const unsigned long long* bsum, int nblk, unsigned long long* bpre) {
  __shared__ unsigned long long s[256];
  __shared__ unsigned long long carry;
  const int hd = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + tid;
    const unsigned long long x = i < nblk ? bsum[(int64_t)hd * nblk + i] : 0ull;
    s[tid] = x;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const unsigned long long y = tid >= o ? s[tid - o] : 0ull;
      __syncthreads();
      s[tid] += y;
      __syncthreads();
    }
    const unsigned long long c = carry;
    if (i < nblk) bpre[(int64_t)hd * (nblk + 1) + i] = c + s[tid] - x;
    __syncthreads();
    if (tid == 255) carry = c + s[255];
    __syncthreads();
  }
  if (tid == 0) bpre[(int64_t)hd * (nblk + 1) + nblk] = carry;
}

// One wave per draw: the block whose span of the prefix sums holds the target, then the row inside the block.
__global__ __launch_bounds__(64) void sil_pick_kernel(const uint32_t* q, int64_t Rcap, int64_t nfill, int nblk,
                                                      const unsigned long long* bpre, const int64_t* u, int n, int64_t* idx) {
  __shared__ unsigned long long s[64];
  const int j = blockIdx.x, hd = blockIdx.y, lane = threadIdx.x;
  const unsigned long long* pre = bpre + (int64_t)hd * (nblk + 1);
  const unsigned long long total = pre[nblk];
  if (total == 0) {                                // (the host launches nothing for a head without an eligible row)
    if (lane == 0) idx[(int64_t)hd * n + j] = 0;
    return;
  }
  const unsigned long long t = (unsigned long long)u[(int64_t)hd * n + j] % total;
  int lo = 0, hi = nblk - 1;                        // the largest blk with pre[blk] <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int64_t r0 = (int64_t)lo * SIL_CH + lane * 16;
  unsigned long long mine = 0;
  for (int i = 0; i < 16; ++i)
    if (r0 + i < nfill) mine += q[hd * Rcap + r0 + i];
  s[lane] = mine;
  __syncthreads();
  if (lane == 0) {
    unsigned long long cum = pre[lo];
    int64_t found = (int64_t)lo * SIL_CH < nfill ? (int64_t)lo * SIL_CH : nfill - 1;
    int l = 0;
    while (l < 63 && cum + s[l] <= t) cum += s[l++];
    const int64_t base = (int64_t)lo * SIL_CH + l * 16;
    for (int i = 0; i < 16; ++i) {
      const int64_t r = base + i;
      if (r >= nfill) break;
      cum += q[hd * Rcap + r];
      if (cum > t) {
        found = r;
        break;
      }
    }
    idx[(int64_t)hd * n + j] = found;
  }
}

// q[h][idx[h][j]] = quantise(sil_w[h][pos[h][B_ppo + j]]); pos NULL: the identity.  An index outside 0 .. Rcap - 1 or a
// position outside 0 .. B - 1 writes nothing.
__global__ __launch_bounds__(256) void sil_scatter_kernel(uint32_t* q, int64_t Rcap, const int64_t* idx, int n, const float* sil_w,
                                                          const int32_t* pos, int B, int B_ppo, double alpha, double eps) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, hd = blockIdx.y;
  if (j >= n) return;
  const int64_t r = idx[(int64_t)hd * n + j];
  const int un = B_ppo + j;
  const int d = pos ? pos[hd * B + un] : un;
  if (r < 0 || r >= Rcap || d < 0 || d >= B) return;
  q[hd * Rcap + r] = sil_quantise(fmaxf(sil_w[hd * B + d], 0.f), eps, alpha);
}

}  // namespace

extern "C" int cadre_ppo_sil_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                                  int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values,
                                  const float* returns, const float* old_logp, const float* adv, const int32_t* row_kind,
                                  int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip,
                                  float value_coeff, float clip_coeff, float ent_coeff, float inv_b, float sil_coeff,
                                  float sil_value_coeff, float inv_bs, float* losses, float* sil_losses, float* sil_w,
                                  float* dlogits, float* dvalues, float* scratch, float* sil_scratch, const int32_t* poison,
                                  float* stats_row, int32_t F, float* stats_scratch, float target_kl, int32_t* stop,
                                  float* sil_stats_row, int32_t sil_F, const int32_t* ord, void* stream) {
  FAIL_IF(!logits || !values || !actions || !commands || !old_values || !returns || !old_logp || !adv || !losses ||
              !sil_losses || !sil_w || !dlogits || !dvalues || !scratch || !sil_scratch || B < 1 || C < 1 || n_out_steer < 1 ||
              n_out_steer > MAX_NOUT || n_out_throttle < 1 || n_out_throttle > MAX_NOUT || ldl < n_out_steer ||
              ldl < n_out_throttle || ldl > 64,
          "cadre_ppo_sil_loss: bad argument");
  FAIL_IF(!row_kind, "cadre_ppo_sil_loss: null row_kind (device int32 [2][B]; 0 a PPO row, 1 a SIL row)");
  FAIL_IF(stats_row && (F < CADRE_PPO_STATS_FIELDS || !stats_scratch || !(target_kl >= 0.f) || (target_kl > 0.f && !stop)),
          "cadre_ppo_sil_loss: bad stats argument (F >= CADRE_PPO_STATS_FIELDS, target_kl >= 0, a stop flag with target_kl > 0)");
  FAIL_IF(sil_stats_row && sil_F < CADRE_SIL_STATS_FIELDS, "cadre_ppo_sil_loss: bad SIL stats argument (sil_F >= CADRE_SIL_STATS_FIELDS)");
  FAIL_IF(hp && ((uintptr_t)hp & 7), "cadre_ppo_sil_loss: bad hyper-parameter block (device double[CADRE_HP_FIELDS], 8-byte aligned)");
  FAIL_IF(!hp && !(isfinite(sil_coeff) && isfinite(sil_value_coeff)), "cadre_ppo_sil_loss: sil_coeff and sil_value_coeff must be finite");
  // inv_bs scales the SIL losses, gradients and statistics: with the scalars in the block it is always needed
  const bool needs_bs = hp || sil_coeff != 0.f || sil_value_coeff != 0.f || sil_stats_row;
  FAIL_IF(needs_bs && !(isfinite(inv_bs) && inv_bs > 0.f), "cadre_ppo_sil_loss: inv_bs must be finite and > 0 (1 / SIL rows per step)");
  const sil_stats_t so{stats_row, F, stats_scratch, target_kl, stop, sil_stats_row, sil_F, sil_scratch};
  const dim3 grid((B + 15) / 16, 2), block(256);
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
#define CADRE_SIL_LAUNCH(S_, H_)                                                                                               \
  hipLaunchKernelGGL((ppo_sil_loss_kernel<S_, H_>), grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, \
                     commands, old_values, returns, old_logp, adv, row_kind, B, C, n_out_steer, n_out_throttle, hp, clip,     \
                     value_coeff, clip_coeff, ent_coeff, inv_b, sil_coeff, sil_value_coeff, inv_bs, losses, sil_losses, sil_w, \
                     dlogits, dvalues, scratch, poison, so, ord)
  if (stats_row && hp) CADRE_SIL_LAUNCH(true, true);
  else if (stats_row) CADRE_SIL_LAUNCH(true, false);
  else if (hp) CADRE_SIL_LAUNCH(false, true);
  else CADRE_SIL_LAUNCH(false, false);
#undef CADRE_SIL_LAUNCH
  return (int)hipGetLastError();
}

#define SIL_PRIO_CHECK(name)                                                                                         \
  FAIL_IF(!(alpha > 0.0) || !isfinite(alpha), name ": alpha must be finite and > 0");                               \
  FAIL_IF(!(prio_eps >= 0.0) || !isfinite(prio_eps), name ": prio_eps must be finite and >= 0")

extern "C" int cadre_sil_prepare(const void* row_table, int32_t n, int32_t T, float gamma, const double* state, float clip_r,
                                 int32_t tail, double alpha, double prio_eps, void* stream) {
  FAIL_IF(!row_table, "cadre_sil_prepare: null operand");
  FAIL_IF(n < 1 || n > 65535 || T < 2 || T > MAX_T || (state && !(clip_r > 0.f)) || !(gamma >= 0.f && gamma <= 1.f),
          "cadre_sil_prepare: bad argument (1 <= n <= 65535 storages, 2 <= T <= 3000, 0 <= gamma <= 1, clip_r > 0 with "
          "reward scaling)");
  FAIL_IF(tail != 0 && tail != 1, "cadre_sil_prepare: tail must be 0 (drop) or 1 (bootstrap)");
  SIL_PRIO_CHECK("cadre_sil_prepare");
  const size_t shm = sizeof(float) * 4 * (T + 1);
  hipLaunchKernelGGL(sil_prepare_kernel, dim3(n), dim3(64), shm, ST(stream), (const sil_prep_row_t*)row_table, T, gamma, state,
                     clip_r, tail, alpha, prio_eps);
  return (int)hipGetLastError();
}

extern "C" int cadre_sil_draw(const uint32_t* q, int64_t Rcap, int64_t filled, const int64_t* u, int32_t n, int64_t* idx,
                              uint64_t* scratch, void* stream) {
  FAIL_IF(!q || !u || !idx || !scratch, "cadre_sil_draw: null operand");
  FAIL_IF(Rcap < 1 || Rcap > ((int64_t)1 << 30) || filled < 1 || filled > Rcap || n < 1 || n > 65535,
          "cadre_sil_draw: bad argument (1 <= Rcap <= 2^30, 1 <= filled <= Rcap, 1 <= n <= 65535)");
  const int nblk = (int)((Rcap + SIL_CH - 1) / SIL_CH);
  unsigned long long* bsum = (unsigned long long*)scratch;
  unsigned long long* bpre = bsum + 2 * (int64_t)nblk;
  hipLaunchKernelGGL(sil_block_sums_kernel, dim3(nblk, 2), dim3(256), 0, ST(stream), q, Rcap, filled, nblk, bsum);
  hipLaunchKernelGGL(sil_scan_blocks_kernel, dim3(2), dim3(256), 0, ST(stream), bsum, nblk, bpre);
  hipLaunchKernelGGL(sil_pick_kernel, dim3(n, 2), dim3(64), 0, ST(stream), q, Rcap, filled, nblk, bpre, u, n, idx);
  return (int)hipGetLastError();
}

extern "C" int cadre_sil_scatter(uint32_t* q, int64_t Rcap, const int64_t* idx, int32_t n, const float* sil_w, const int32_t* pos,
                                 int32_t B, int32_t B_ppo, double alpha, double prio_eps, void* stream) {
  FAIL_IF(!q || !idx || !sil_w, "cadre_sil_scatter: null operand");
  FAIL_IF(Rcap < 1 || n < 1 || B < 1 || B_ppo < 0 || (int64_t)B_ppo + n > B,
          "cadre_sil_scatter: bad argument (Rcap >= 1, n >= 1, B >= 1, the n SIL rows are unsorted rows B_ppo .. B_ppo + n - 1 <= B - 1)");
  SIL_PRIO_CHECK("cadre_sil_scatter");
  hipLaunchKernelGGL(sil_scatter_kernel, dim3((n + 255) / 256, 2), dim3(256), 0, ST(stream), q, Rcap, idx, n, sil_w, pos, B, B_ppo,
                     alpha, prio_eps);
  return (int)hipGetLastError();
}
