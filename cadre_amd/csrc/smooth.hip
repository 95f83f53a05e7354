// smooth.hip — the temporal action-smoothness term of CAPS (Mysore et al. 2021) inside the PPO step: successor rows (row t + 1 of a
// worker's own storages) ride behind the workers' rows, and one loss launch couples each row with its partner.
//
//   cadre_smooth_mates     after the gather / sort: which rows of the minibatch are successor rows (row_kind) and where each row's
//                          partner lies in the workspace (mate, -1: none)
//   cadre_ppo_smooth_loss  where cadre_ppo_loss_ord / cadre_ppo_sil_loss stand in the update: same addressing, grid, scratch
//                          protocol, poison and rank table.  A row of kind 0 runs the statements of ppo_loss_body (cadre_kernels.hip,
//                          restated as in selfimit.hip); a paired row also reads its partner's logits row, forms the mean control
//                          mu = sum_k p_k c_k of both rows and adds the gradient of d^2, d = mu_own - mu_mate.
//   cadre_action_jitter    what the rollouts did: |c[a_{t+1}] - c[a_t]| over the same pairs, per storage
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

// mu = sum_k p_k c_k in the tree order of wave_sum, every product and sum rounded on its own (no FMA): the two partners of a pair
// form the mu of a row with these statements, so both hold the same bits and their d are exact negatives.
__device__ __forceinline__ float smooth_mu(float pk, float ck, bool on) {
  float v = on ? __fmul_rn(pk, ck) : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

// The pair (row t, row t + 1) of one storage counts: t + 1 is a row of the rollout, row t did not end its episode (masks[t] is the
// factor cadre_gae_multi multiplies V[t + 1] by), was not cut by a step limit, and both rows drive under one command in range.
__device__ __forceinline__ bool smooth_pair_valid(const float* masks, const float* time_limits, const int32_t* command, int64_t t,
                                                  int T, int C) {
  if (t < 0 || t > (int64_t)T - 2) return false;
  if (masks[t] == 0.f) return false;
  if (time_limits && time_limits[t] != 0.f) return false;
  const int c = command[t];
  return c >= 0 && c < C && command[t + 1] == c;
}

#define PPO_NSTAT 6
#define SM_NSTAT CADRE_SMOOTH_STATS_FIELDS
struct smooth_stats_t {
  float* row;           // [2 heads][F] PPO stats row of this step (STATS)
  int32_t F;
  float* part;          // [2 * nblk][PPO_NSTAT] per-workgroup partials
  float target_kl;      // > 0: KL gate armed
  int32_t* stop;        // sticky gate flag (may be NULL when the gate is off)
};
struct smooth_t {
  const int32_t* row_kind;   // [2][B] 0 a PPO row, 1 a successor row
  const int32_t* mate;       // [2][B] the partner's position, -1: none
  const float* ctrl;         // [2][64] control value of each bin
  float scale_steer, scale_throttle;   // head_scale
  float inv_bp;              // 1 / pair slots per step and head
  float* losses;             // smooth_losses[1]
  float* d;                  // smooth_d [2][B]
  float* part;               // [2 * nblk][SM_NSTAT] per-workgroup partials: pairs, sum |d|, max |d|, sum d^2
  float* row;                // [2 heads][F] smoothness stats row (NULL: none)
  int32_t F;
};

// One wave per row (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups, as ppo_sil_loss_kernel.  The front (raw logits to the
// normalised logits lg and the probabilities pk) and mu run in ONE loop body that a paired row passes twice, first on its partner's
// logits row, then on its own: both partners execute the same instructions on a given row.
template <bool STATS, bool HP>
__global__ __launch_bounds__(256) void ppo_smooth_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                              int64_t ldv, int64_t v_ns, const int64_t* actions,
                                                              const int32_t* commands, const float* old_values,
                                                              const float* returns, const float* old_logp, const float* adv, int B,
                                                              int C, int n_steer, int n_throttle, double* hp, float clip,
                                                              float value_coeff, float clip_coeff, float ent_coeff, float inv_b,
                                                              float smooth_coeff, float* losses, float* dlogits, float* dvalues,
                                                              float* scratch, const int32_t* poison, smooth_stats_t so, smooth_t sm,
                                                              const int32_t* ord) {
  if constexpr (HP) {
    clip = (float)hp[CADRE_HP_CLIP];
    value_coeff = (float)hp[CADRE_HP_VALUE_COEFF];
    clip_coeff = (float)hp[CADRE_HP_CLIP_COEFF];
    ent_coeff = (float)hp[CADRE_HP_ENT_COEFF];
    smooth_coeff = (float)hp[CADRE_HP_SMOOTH_COEFF];
  }
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float red[3 + PPO_NSTAT + SM_NSTAT][4];
  float s_act = 0.f, s_val = 0.f, s_ent = 0.f;     // PPO rows; lane 0 of each wave
  float s_kl = 0.f, s_okl = 0.f, s_cf = 0.f, s_vcf = 0.f, s_r = 0.f, m_lr = 0.f;   // (STATS only)
  float q_n = 0.f, q_ad = 0.f, q_mx = 0.f, q_d2 = 0.f;                              // pairs, counted by their kind-0 partner
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane, binv = lane;
  if (ordinal) {
    rk = lane < K ? ord[hd * 64 + lane] : lane;
    binv = ord_inverse(rk, lane);
  }
  const bool on = lane < K;
  const float ck = on ? sm.ctrl[hd * 64 + lane] : 0.f;
  const float cf = smooth_coeff * (hd == 0 ? sm.scale_steer : sm.scale_throttle) * sm.inv_bp;
  for (int i = 0; i < 4; ++i) {
    const int b = blockIdx.x * 16 + wave * 4 + i;
    if (b >= B) break;
    const int row = hd * B + b;                    // per-head sample arrays are [2][B]
    const int c = commands[row];
    const bool succ = sm.row_kind[row] != 0;
    const int m = sm.mate[row];
    int cm = -1;
    if (m >= 0 && m < B) cm = commands[hd * B + m];
    const bool paired = cm >= 0 && cm < C;
    // a PPO row counts when its command is in range; a successor row also needs its partner
    const bool own_ok = c >= 0 && c < C && (!succ || paired);
    for (int cc = 0; cc < C; ++cc) {
      if (own_ok && cc == c) continue;
      if (lane < ldl) dlogits[(int64_t)(hd * C + cc) * l_ns + (int64_t)b * ldl + lane] = 0.f;
      if (lane == 0) dvalues[(int64_t)(hd * C + cc) * v_ns + (int64_t)b * ldv] = 0.f;
    }
    if (!own_ok) {
      if (lane == 0) sm.d[row] = 0.f;
      continue;
    }
    const int net = hd * C + c;
    const float* own_row = logits + (int64_t)net * l_ns + (int64_t)b * ldl;
    const float* mate_row = paired ? logits + (int64_t)(hd * C + cm) * l_ns + (int64_t)m * ldl : own_row;
    float lg = 0.f, pk = 0.f, sg = 0.f, tg = 0.f;  // of the pass that ran last: the row's own
    float mu = 0.f, mu_mate = 0.f;
#pragma nounroll
    for (int pass = paired ? 0 : 1; pass < 2; ++pass) {
      mu_mate = mu;
      const float* src = pass == 0 ? mate_row : own_row;
      float x = on ? src[lane] : -INFINITY;
      if (ordinal) x = ord_logits(x, on, rk, lane, sg, tg);   // (sg, tg: sigmoid(x), sigmoid(-x) of this lane's threshold unit)
      const float mx = wave_max(x);
      const float se = wave_sum(on ? expf(x - mx) : 0.f);
      const float lse = mx + logf(se);
      lg = x - lse;
      const float mx2 = wave_max(on ? lg : -INFINITY);
      const float e2 = on ? expf(lg - mx2) : 0.f;
      const float se2 = wave_sum(e2);
      pk = e2 / se2;
      mu = smooth_mu(pk, ck, on);
    }
    // d total / d logit_k (own row) = cf 2 d p_k (c_k - mu_own), d = mu_own - mu_mate
    const float d = paired ? __fsub_rn(mu, mu_mate) : 0.f;
    const float gd = cf * (2.f * d);
    const float gs = on ? gd * (pk * (ck - mu)) : 0.f;
    if (lane == 0) sm.d[row] = d;
    if (!succ) {
      // ---- a PPO row: ppo_loss_body
      const int a = (int)actions[row];
      const float H = -wave_sum(on ? pk * lg : 0.f);
      const float lp = __shfl(lg, a, 64);
      const float v = values[(int64_t)net * v_ns + (int64_t)b * ldv];
      const float R = returns[row];
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
      if (paired) {
        // ---- and the pair, counted here only: total += cf d^2
        gk = gk + gs;
        q_n += 1.f;
        q_ad += fabsf(d);
        q_mx = fmaxf(q_mx, fabsf(d));
        q_d2 += d * d;
      }
      if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
      if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
    } else {
      // ---- a successor row: the smoothness gradient only; no PPO term, no entropy term, no value gradient
      float gk = gs;
      if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
      if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
      if (lane == 0) dvalues[(int64_t)net * v_ns + (int64_t)b * ldv] = 0.f;
    }
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_act; red[2][wave] = s_ent;
    red[3][wave] = s_kl; red[4][wave] = s_okl; red[5][wave] = s_cf;
    red[6][wave] = s_vcf; red[7][wave] = s_r; red[8][wave] = m_lr;
    red[9][wave] = q_n; red[10][wave] = q_ad; red[11][wave] = q_mx; red[12][wave] = q_d2;
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
    for (int k = 0; k < SM_NSTAT; ++k) {
      const float* r = red[9 + k];
      const float t = k == 2 ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
      __hip_atomic_store(sm.part + SM_NSTAT * me + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
      const float bad = (poison && __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? __builtin_nanf("") : 0.f;
      losses[0] = value_coeff * 0.5f * sv * inv_b + bad;
      losses[1] = clip_coeff * sa * inv_b + bad;
      losses[2] = ent_coeff * sn * inv_b + bad;
      // per head, partials in workgroup order: pairs, sum |d|, max |d|, sum d^2
      float qt[2][SM_NSTAT];
      for (int h = 0; h < 2; ++h) {
        float t[SM_NSTAT] = {0.f, 0.f, 0.f, 0.f};
        for (int w = h * nblk; w < (h + 1) * nblk; ++w)
          for (int k = 0; k < SM_NSTAT; ++k) {
            const float x = __hip_atomic_load(sm.part + SM_NSTAT * w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t[k] = k == 2 ? fmaxf(t[k], x) : t[k] + x;
          }
        for (int k = 0; k < SM_NSTAT; ++k) qt[h][k] = t[k];
      }
      const float l0 = (smooth_coeff * sm.scale_steer * sm.inv_bp) * qt[0][3];
      const float l1 = (smooth_coeff * sm.scale_throttle * sm.inv_bp) * qt[1][3];
      sm.losses[0] = (l0 + l1) + bad;
      if (sm.row != nullptr) {
        for (int h = 0; h < 2; ++h) {
          float* o = sm.row + h * sm.F;
          o[0] = qt[h][0];
          o[1] = sm.inv_bp * qt[h][1];
          o[2] = qt[h][2];
          o[3] = sm.inv_bp * qt[h][3];
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
        // the gate, `applied` and (HP) the KL-adaptive lr: the rule of kl_rule.h on the KL of the PPO rows, without the pairs
        if constexpr (HP) cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, hp[CADRE_HP_DESIRED_KL], hp);
        else cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, 0.0, nullptr);
      }
      __hip_atomic_store(reinterpret_cast<unsigned*>(scratch), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------- pair placement
struct smooth_src_t {
  const float* masks; const float* time_limits; const int32_t* command;
};

// One thread per (head, unsorted row).  Unsorted row u = entry e, row r of the entry (u = e Bw + r); entries 0 .. nW - 1 are the
// workers', entry nW + k is successor entry k, which belongs to worker (rot + k) mod nW.  Every thread writes the two words of its own
// row at its own workspace position: both arrays are overwritten completely, and no two threads write one word.
__global__ __launch_bounds__(256) void smooth_mates_kernel(const smooth_src_t* src, const int64_t* idx, int nW, int E, int Bw, int T,
                                                           int C, int rot, const int32_t* pos, int B, int32_t* row_kind,
                                                           int32_t* mate) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x, hd = blockIdx.y;
  if (u >= B) return;
  const int e = u / Bw, r = u - e * Bw;
  int w, k;
  if (e < nW) {
    w = e;
    k = (w - rot) % nW;
    if (k < 0) k += nW;
  } else {
    k = e - nW;
    w = (rot + k) % nW;
  }
  bool valid = false;
  int partner = -1;
  if (k < E) {                                     // (a worker without a successor entry this step has k >= E)
    const int64_t t = idx[(int64_t)(2 * w + hd) * Bw + r], t1 = idx[(int64_t)(2 * (nW + k) + hd) * Bw + r];
    const smooth_src_t s = src[2 * w + hd];
    valid = smooth_pair_valid(s.masks, s.time_limits, s.command, t, T, C) && t1 == t + 1;
    partner = e < nW ? (nW + k) * Bw + r : w * Bw + r;
  }
  const int me = pos ? pos[hd * B + u] : u;
  if (me < 0 || me >= B) return;
  int pm = -1;
  if (valid) {
    pm = pos ? pos[hd * B + partner] : partner;
    if (pm < 0 || pm >= B) pm = -1;
  }
  row_kind[hd * B + me] = e < nW ? 0 : 1;
  mate[hd * B + me] = pm;
}

// ---------------------------------------------------------------------------- realised jitter
struct jitter_src_t {
  const int64_t* action; const float* masks; const float* time_limits; const int32_t* command;
};

// One wave per storage (storage k belongs to head k & 1).  Lane l takes t = l, l + 64, ... in ascending order; the lanes' doubles
// are combined by the xor tree (32, 16, .. 1): a fixed order.
__global__ __launch_bounds__(64) void action_jitter_kernel(const jitter_src_t* src, int T, int C, int K0, int K1, const float* ctrl,
                                                           double* out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const jitter_src_t g = src[k];
  const int hd = k & 1, K = hd == 0 ? K0 : K1;
  const float* c = ctrl + hd * 64;
  double n = 0.0, s = 0.0, mx = 0.0;
  for (int t = lane; t <= T - 2; t += 64) {
    if (!smooth_pair_valid(g.masks, g.time_limits, g.command, t, T, C)) continue;
    const int64_t a0 = g.action[t], a1 = g.action[t + 1];
    if (a0 < 0 || a0 >= K || a1 < 0 || a1 >= K) continue;
    const double df = (double)fabsf(__fsub_rn(c[a1], c[a0]));
    n += 1.0;
    s += df;
    mx = fmax(mx, df);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    s += __shfl_xor(s, o, 64);
    mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    out[3 * k + 0] = n;
    out[3 * k + 1] = s;
    out[3 * k + 2] = mx;
  }
}

}  // namespace

extern "C" int cadre_smooth_mates(const void* src_table, const int64_t* idx, int32_t nW, int32_t E, int32_t Bw, int32_t T, int32_t C,
                                  int64_t rotation, const int32_t* pos, int32_t Bt, int32_t* row_kind, int32_t* mate, void* stream) {
  FAIL_IF(!src_table || !idx || !row_kind || !mate, "cadre_smooth_mates: null operand");
  FAIL_IF(nW < 1 || nW > 16384 || E < 1 || E > nW || Bw < 1 || T < 2 || C < 1 || rotation < 0,
          "cadre_smooth_mates: bad argument (1 <= nW <= 16384 worker entries, 1 <= E <= nW successor entries, Bw >= 1, T >= 2, C >= 1, "
          "rotation >= 0)");
  FAIL_IF((int64_t)(nW + E) * Bw != (int64_t)Bt, "cadre_smooth_mates: Bt must be (nW + E) * Bw");
  const int rot = (int)(rotation % nW);
  hipLaunchKernelGGL(smooth_mates_kernel, dim3((Bt + 255) / 256, 2), dim3(256), 0, ST(stream), (const smooth_src_t*)src_table, idx,
                     nW, E, Bw, T, C, rot, pos, Bt, row_kind, mate);
  return (int)hipGetLastError();
}

extern "C" int cadre_ppo_smooth_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                                     const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                                     const float* old_logp, const float* adv, const int32_t* row_kind, const int32_t* mate,
                                     const float* ctrl, int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, double* hp,
                                     float clip, float value_coeff, float clip_coeff, float ent_coeff, float inv_b, float smooth_coeff,
                                     float scale_steer, float scale_throttle, float inv_bp, float* losses, float* smooth_losses,
                                     float* smooth_d, float* dlogits, float* dvalues, float* scratch, float* smooth_scratch,
                                     const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch, float target_kl,
                                     int32_t* stop, float* smooth_stats_row, int32_t smooth_F, const int32_t* ord, void* stream) {
  FAIL_IF(!logits || !values || !actions || !commands || !old_values || !returns || !old_logp || !adv || !losses || !smooth_losses ||
              !smooth_d || !dlogits || !dvalues || !scratch || !smooth_scratch || B < 1 || C < 1 || n_out_steer < 1 ||
              n_out_steer > MAX_NOUT || n_out_throttle < 1 || n_out_throttle > MAX_NOUT || ldl < n_out_steer ||
              ldl < n_out_throttle || ldl > 64,
          "cadre_ppo_smooth_loss: bad argument");
  FAIL_IF(!row_kind || !mate, "cadre_ppo_smooth_loss: null row_kind or mate (device int32 [2][B]; cadre_smooth_mates writes both)");
  FAIL_IF(!ctrl, "cadre_ppo_smooth_loss: null ctrl (device float32 [2][64]: the control value of each bin)");
  FAIL_IF(stats_row && (F < CADRE_PPO_STATS_FIELDS || !stats_scratch || !(target_kl >= 0.f) || (target_kl > 0.f && !stop)),
          "cadre_ppo_smooth_loss: bad stats argument (F >= CADRE_PPO_STATS_FIELDS, target_kl >= 0, a stop flag with target_kl > 0)");
  FAIL_IF(smooth_stats_row && smooth_F < CADRE_SMOOTH_STATS_FIELDS,
          "cadre_ppo_smooth_loss: bad smoothness stats argument (smooth_F >= CADRE_SMOOTH_STATS_FIELDS)");
  FAIL_IF(hp && ((uintptr_t)hp & 7), "cadre_ppo_smooth_loss: bad hyper-parameter block (device double[CADRE_HP_FIELDS], 8-byte aligned)");
  FAIL_IF(!hp && !isfinite(smooth_coeff), "cadre_ppo_smooth_loss: smooth_coeff must be finite");
  FAIL_IF(!(isfinite(scale_steer) && scale_steer >= 0.f && isfinite(scale_throttle) && scale_throttle >= 0.f),
          "cadre_ppo_smooth_loss: scale_steer and scale_throttle must be finite and >= 0");
  FAIL_IF(!(isfinite(inv_bp) && inv_bp > 0.f), "cadre_ppo_smooth_loss: inv_bp must be finite and > 0 (1 / pair slots per step and head)");
  const smooth_stats_t so{stats_row, F, stats_scratch, target_kl, stop};
  const smooth_t sm{row_kind, mate, ctrl, scale_steer, scale_throttle, inv_bp, smooth_losses, smooth_d, smooth_scratch,
                    smooth_stats_row, smooth_F};
  const dim3 grid((B + 15) / 16, 2), block(256);
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
#define CADRE_SMOOTH_LAUNCH(S_, H_)                                                                                                \
  hipLaunchKernelGGL((ppo_smooth_loss_kernel<S_, H_>), grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, \
                     commands, old_values, returns, old_logp, adv, B, C, n_out_steer, n_out_throttle, hp, clip, value_coeff,      \
                     clip_coeff, ent_coeff, inv_b, smooth_coeff, losses, dlogits, dvalues, scratch, poison, so, sm, ord)
  if (stats_row && hp) CADRE_SMOOTH_LAUNCH(true, true);
  else if (stats_row) CADRE_SMOOTH_LAUNCH(true, false);
  else if (hp) CADRE_SMOOTH_LAUNCH(false, true);
  else CADRE_SMOOTH_LAUNCH(false, false);
#undef CADRE_SMOOTH_LAUNCH
  return (int)hipGetLastError();
}

extern "C" int cadre_action_jitter(const void* src_table, int32_t n, int32_t T, int32_t C, int32_t n_out_steer, int32_t n_out_throttle,
                                   const float* ctrl, double* out, void* stream) {
  FAIL_IF(!src_table || !ctrl || !out, "cadre_action_jitter: null operand");
  FAIL_IF(n < 1 || n > 65535 || T < 2 || C < 1 || n_out_steer < 1 || n_out_steer > MAX_NOUT || n_out_throttle < 1 ||
              n_out_throttle > MAX_NOUT,
          "cadre_action_jitter: bad argument (1 <= n <= 65535 storages, T >= 2, C >= 1, 1 <= bins <= 64)");
  FAIL_IF((uintptr_t)out & 7, "cadre_action_jitter: out must be 8-byte aligned (device float64 [n][3])");
  hipLaunchKernelGGL(action_jitter_kernel, dim3(n), dim3(64), 0, ST(stream), (const jitter_src_t*)src_table, T, C, n_out_steer,
                     n_out_throttle, ctrl, out);
  return (int)hipGetLastError();
}
