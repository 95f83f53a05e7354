// actmask.hip — action masks: per-row allowed-bin sets in sampling and in the PPO loss (actmask.h).
//
//   cadre_sample_am            cadre_sample_ord with one word per row
//   cadre_sample_rows_am       cadre_sample_rows_ord with one word per (environment, head)
//   cadre_categorical_eval_am  cadre_categorical_eval_ord under the mask (forward only)
//   cadre_allowed_note         allowed[k][slot[k]] = word[k] for the 2N storages of one env step
//   cadre_allowed_rows         out[h][pos[h][row]] = allowed_src[idx]: the words of a minibatch in the layout of the update
//   cadre_ppo_am_loss          where cadre_ppo_loss_ord stands in the update: same addressing, grid, scratch protocol, poison,
//                              rank table and kl_rule.h gate.  A row runs the statements of ppo_loss_body (cadre_kernels.hip)
//                              with on_m in the place of on behind the ordinal transform.
//
// Everything this file writes is written with plain vector stores or agent-scope atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"
#include "actmask.h"
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

// the logit of bin `lane` in bin space: x itself, or ord_logits for an ordinal head (ord[0] >= 0)
__device__ __forceinline__ float am_row_logit(float x, int K, int lane, const int32_t* ord) {
  if (ord[0] >= 0) {
    float s, t;
    return ord_logits(x, lane < K, lane < K ? ord[lane] : lane, lane, s, t);
  }
  return x;
}

// ---------------------------------------------------------------------------- sampling: argmax(p / q) over allowed bins
// sample_kernel<true> (cadre_kernels.hip) with on_m; q is read for all K bins as the host drew it.
__global__ __launch_bounds__(64) void sample_am_kernel(const float* logits, int64_t ldl, const float* q, int64_t ldq, int K,
                                                       int64_t* action, float* logp, const int32_t* ord,
                                                       const int64_t* allowed) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const uint64_t m = am_effective(am_word(allowed, r), K);
  const bool on_m = lane < K && am_on(m, lane);
  float x = am_row_logit(lane < K ? logits[(int64_t)r * ldl + lane] : -INFINITY, K, lane, ord);
  x = on_m ? x : -INFINITY;
  const float mx = wave_max(x);
  const float se = wave_sum(on_m ? expf(x - mx) : 0.f);
  const float lg = x - (mx + logf(se));                          // normalised logits
  const float mx2 = wave_max(on_m ? lg : -INFINITY);
  const float e2 = on_m ? expf(lg - mx2) : 0.f;
  const float p = e2 / wave_sum(e2);
  const float pn = p / wave_sum(p);
  float best = on_m ? pn / q[(int64_t)r * ldq + lane] : -INFINITY;
  int bi = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                             // argmax, lowest index wins ties
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const float lsel = __shfl(lg, bi, 64);
  if (lane == 0) { action[r] = bi; logp[r] = lsel; }
}

// sample_rows_kernel<true> (act_batch.hip) with the words allowed[e][h]
__global__ __launch_bounds__(64) void sample_rows_am_kernel(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos,
                                                            const int32_t* cmd, int N, int C, const float* q, int K0, int K1,
                                                            int64_t* action, float* logp, float* value, const int32_t* ord,
                                                            const int64_t* allowed) {
  const int e = blockIdx.x >> 1, h = blockIdx.x & 1, lane = threadIdx.x;
  const int K = h ? K1 : K0;
  const int c = cmd[e], p = pos[e];
  if (c < 0 || c >= C || p < 0 || p >= N) return;                 // (the host checked)
  const int z = 2 * (h * C + c);
  const float* lr = O3 + (int64_t)z * z_str + (int64_t)p * ldo;
  const uint64_t m = am_effective(am_word(allowed, e * 2 + h), K);
  const bool on_m = lane < K && am_on(m, lane);
  float x = am_row_logit(lane < K ? lr[lane] : -INFINITY, K, lane, ord + h * 64);
  x = on_m ? x : -INFINITY;
  const float mx = wave_max(x);
  const float se = wave_sum(on_m ? expf(x - mx) : 0.f);
  const float lg = x - (mx + logf(se));
  const float mx2 = wave_max(on_m ? lg : -INFINITY);
  const float e2 = on_m ? expf(lg - mx2) : 0.f;
  const float pr = e2 / wave_sum(e2);
  const float pn = pr / wave_sum(pr);
  float best = on_m ? pn / q[((int64_t)e * 2 + h) * 64 + lane] : -INFINITY;
  int bi = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const float lsel = __shfl(lg, bi, 64);
  if (lane == 0) {
    action[e * 2 + h] = bi;
    logp[e * 2 + h] = lsel;
    value[e * 2 + h] = O3[(int64_t)(z + 1) * z_str + (int64_t)p * ldo];
  }
}

// categorical_eval_kernel<true> (cadre_kernels.hip) under the mask; the given action is allowed by definition, as in the loss
__global__ __launch_bounds__(64) void categorical_eval_am_kernel(const float* logits, int64_t ldl, const int64_t* actions, int K,
                                                                 float* logp, float* entropy, const int32_t* ord,
                                                                 const int64_t* allowed) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int a = (int)actions[r];
  uint64_t m = am_effective(am_word(allowed, r), K);
  if (a >= 0 && a < K) m |= 1ull << a;
  const bool on_m = lane < K && am_on(m, lane);
  float x = am_row_logit(lane < K ? logits[(int64_t)r * ldl + lane] : -INFINITY, K, lane, ord);
  x = on_m ? x : -INFINITY;
  const float mx = wave_max(x);
  const float se = wave_sum(on_m ? expf(x - mx) : 0.f);
  const float lg = x - (mx + logf(se));
  const float mx2 = wave_max(on_m ? lg : -INFINITY);
  const float e2 = on_m ? expf(lg - mx2) : 0.f;
  const float p = e2 / wave_sum(e2);
  const float h = wave_sum(on_m ? -p * lg : 0.f);
  const float la = __shfl(lg, a & 63, 64);
  if (lane == 0) { logp[r] = la; entropy[r] = h; }
}

// ---------------------------------------------------------------------------- recording
__global__ __launch_bounds__(64) void allowed_note_kernel(const int64_t* table, const int32_t* slots, const int64_t* words,
                                                          int n, int T) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  int64_t* al = reinterpret_cast<int64_t*>(table[k]);
  const int s = slots[k];
  if (al && s >= 0 && s <= T) al[s] = words[k];
}

// ---------------------------------------------------------------------------- words of a minibatch
// Source zi = 2 * worker + head, as in gather_sorted_multi_kernel: unsorted row ob = worker * Bw + b of head hd goes to
// workspace position pos[hd * Bt + ob].  A source without the tensor (pointer 0) gives the word 0: unmasked.
__global__ __launch_bounds__(256) void allowed_rows_kernel(const int64_t* src, int n_src, const int64_t* idx, int Bw, int T,
                                                           const int32_t* pos, int Bt, int64_t* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x, zi = blockIdx.y;
  if (b >= Bw) return;
  const int wi = zi >> 1, hd = zi & 1;
  const int ob = wi * Bw + b;
  if (ob >= Bt) return;
  const int d = pos ? pos[hd * Bt + ob] : ob;
  if (d < 0 || d >= Bt) return;
  const int64_t* al = reinterpret_cast<const int64_t*>(src[zi]);
  int64_t w = 0;
  if (al) {
    const int64_t t = idx[(int64_t)zi * Bw + b];
    if (t < 0 || t >= T) return;
    w = al[t];
  }
  out[(int64_t)hd * Bt + d] = w;
}

// ---------------------------------------------------------------------------- the loss
#define PPO_NSTAT 6
#define AM_NPART 5                    // per workgroup: rows with a proper mask, allowed bins, pressure, action bits OR-ed in, rows counted
struct am_stats_t {
  float* row;           // [2 heads][F] PPO stats row of this step (STATS)
  int32_t F;
  float* part;          // [2 * nblk][PPO_NSTAT] per-workgroup partials
  float target_kl;      // > 0: KL gate armed
  int32_t* stop;        // sticky gate flag (may be NULL when the gate is off)
  float* am_row;        // [2 heads][am_F] mask stats row (NULL: none)
  int32_t am_F;
  float* am_part;       // [2 * nblk][AM_NPART] per-workgroup partials (with am_row)
};

// One wave per row (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups: ppo_loss_body with the row's word.
template <bool STATS, bool HP>
__global__ __launch_bounds__(256) void ppo_am_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                          int64_t ldv, int64_t v_ns, const int64_t* actions,
                                                          const int32_t* commands, const float* old_values,
                                                          const float* returns, const float* old_logp, const float* adv, int B,
                                                          int C, int n_steer, int n_throttle, double* hp, float clip,
                                                          float value_coeff, float clip_coeff, float ent_coeff, float inv_b,
                                                          float* losses, float* dlogits, float* dvalues, float* scratch,
                                                          const int32_t* poison, am_stats_t so, const int32_t* ord,
                                                          const int64_t* allowed) {
  if constexpr (HP) {
    clip = (float)hp[CADRE_HP_CLIP];
    value_coeff = (float)hp[CADRE_HP_VALUE_COEFF];
    clip_coeff = (float)hp[CADRE_HP_CLIP_COEFF];
    ent_coeff = (float)hp[CADRE_HP_ENT_COEFF];
  }
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool astats = so.am_row != nullptr;
  __shared__ float red[3 + PPO_NSTAT + AM_NPART][4];
  float s_act = 0.f, s_val = 0.f, s_ent = 0.f;     // lane 0 of each wave
  float s_kl = 0.f, s_okl = 0.f, s_cf = 0.f, s_vcf = 0.f, s_r = 0.f, m_lr = 0.f;   // (STATS only)
  float a_pr = 0.f, a_n = 0.f, a_ps = 0.f, a_or = 0.f, a_ct = 0.f;   // (am_row only) proper rows, allowed bins, pressure, bits OR-ed in, rows
  const bool ordinal = ord[hd * 64] >= 0;
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
    const bool own_ok = c >= 0 && c < C;
    for (int cc = 0; cc < C; ++cc) {
      if (own_ok && cc == c) continue;
      if (lane < ldl) dlogits[(int64_t)(hd * C + cc) * l_ns + (int64_t)b * ldl + lane] = 0.f;
      if (lane == 0) dvalues[(int64_t)(hd * C + cc) * v_ns + (int64_t)b * ldv] = 0.f;
    }
    if (!own_ok) continue;
    const int a = (int)actions[row];
    const int net = hd * C + c;
    const bool on = lane < K;
    // the row's word: empty means all, and the taken action is allowed by definition
    uint64_t m = am_effective(am_word(allowed, row), K);
    const bool forced = a >= 0 && a < K && !am_on(m, a);
    if (forced) m |= 1ull << a;
    const bool on_m = on && am_on(m, lane);
    float x = on ? logits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] : -INFINITY;
    float sg = 0.f, tg = 0.f;                      // (ordinal head) sigmoid(x), sigmoid(-x) of this lane's threshold unit
    if (ordinal) x = ord_logits(x, on, rk, lane, sg, tg);
    const float xu = x;                            // the unmasked logit in bin space (the pressure)
    x = on_m ? x : -INFINITY;
    const float mx = wave_max(x);
    const float se = wave_sum(on_m ? expf(x - mx) : 0.f);
    const float lse = mx + logf(se);
    const float lg = x - lse;
    const float mx2 = wave_max(on_m ? lg : -INFINITY);
    const float e2 = on_m ? expf(lg - mx2) : 0.f;
    const float se2 = wave_sum(e2);
    const float pk = e2 / se2;
    const float H = -wave_sum(on_m ? pk * lg : 0.f);
    const float lp = __shfl(lg, a, 64);
    const float v = values[(int64_t)net * v_ns + (int64_t)b * ldv];
    const float A = adv[row], ov = old_values[row], R = returns[row];
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
    if (astats) {                                  // (wave-uniform)
      const bool proper = am_proper(m, K);
      a_pr += proper ? 1.f : 0.f;
      a_n += (float)am_count(m);
      a_ps += am_pressure(xu, on, lse, proper);
      a_or += forced ? 1.f : 0.f;
      a_ct += 1.f;
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
    float gk = on_m ? dlp * ((lane == a ? 1.f : 0.f) - pk) + dH * (-pk * (lg + H)) : 0.f;
    if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
    if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_act; red[2][wave] = s_ent;
    red[3][wave] = s_kl; red[4][wave] = s_okl; red[5][wave] = s_cf;
    red[6][wave] = s_vcf; red[7][wave] = s_r; red[8][wave] = m_lr;
    red[9][wave] = a_pr; red[10][wave] = a_n; red[11][wave] = a_ps; red[12][wave] = a_or; red[13][wave] = a_ct;
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
    if (astats) {
      for (int k = 0; k < AM_NPART; ++k) {
        const float* r = red[9 + k];
        __hip_atomic_store(so.am_part + AM_NPART * me + k, (r[0] + r[1]) + (r[2] + r[3]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
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
      if (astats) {
        // per head, partials in workgroup order: shares and means over the head's counted rows (a command in range; the
        // counts are integers, exact in fp32), OR-ed rows as a count
        for (int h = 0; h < 2; ++h) {
          float t[AM_NPART] = {0.f, 0.f, 0.f, 0.f, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < AM_NPART; ++k)
              t[k] += __hip_atomic_load(so.am_part + AM_NPART * w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          float* o = so.am_row + h * so.am_F;
          const bool any = t[4] > 0.f;
          o[0] = any ? t[0] / t[4] : 0.f;
          o[1] = any ? t[1] / t[4] : 0.f;
          o[2] = any ? t[2] / t[4] : 0.f;
          o[3] = t[3];
        }
      }
      if constexpr (STATS) {
        // per head, partials in workgroup order; means over inv_b (the losses' denominator)
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
        // the gate, `applied` and (HP) the KL-adaptive lr: the rule of kl_rule.h on the masked ratio's KL
        if constexpr (HP) cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, hp[CADRE_HP_DESIRED_KL], hp);
        else cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, 0.0, nullptr);
      }
      __hip_atomic_store(reinterpret_cast<unsigned*>(scratch), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

extern "C" int cadre_sample_am(const float* logits, int64_t ldl, const float* q, int64_t ldq, int32_t R, int32_t n_out,
                               int64_t* action, float* logp, const int32_t* ord, const int64_t* allowed, void* stream) {
  FAIL_IF(!logits || !q || !action || !logp || R < 1 || n_out < 1 || n_out > 64 || ldl < n_out || ldq < n_out,
          "cadre_sample_am: bad argument");
  FAIL_IF(!ord, "cadre_sample_am: null rank table (device int32 [64]; ord[0] = -1 marks the categorical head)");
  FAIL_IF(!allowed, "cadre_sample_am: null allowed (device int64 [R]; bit k set: bin k may be chosen, no bit among K: unmasked)");
  hipLaunchKernelGGL(sample_am_kernel, dim3(R), dim3(64), 0, ST(stream), logits, ldl, q, ldq, n_out, action, logp, ord, allowed);
  return (int)hipGetLastError();
}

extern "C" int cadre_sample_rows_am(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd,
                                    int32_t N, int32_t C, const float* q, int32_t K_steer, int32_t K_throttle, int64_t* action,
                                    float* logp, float* value, const int32_t* ord, const int64_t* allowed, void* stream) {
  FAIL_IF(!O3 || !pos || !cmd || !q || !action || !logp || !value, "cadre_sample_rows_am: null operand");
  FAIL_IF(!ord, "cadre_sample_rows_am: null rank table (device int32 [2][64]; ord[h][0] = -1 marks a categorical head)");
  FAIL_IF(!allowed, "cadre_sample_rows_am: null allowed (device int64 [N][2])");
  FAIL_IF(N < 1 || C < 1 || C > 16 || K_steer < 1 || K_steer > 64 || K_throttle < 1 || K_throttle > 64 || ldo < K_steer ||
              ldo < K_throttle || z_str < (int64_t)N * ldo,
          "cadre_sample_rows_am: bad argument (N >= 1, 1 <= C <= 16, 1 <= K <= 64, ldo >= K, z_str >= N * ldo)");
  hipLaunchKernelGGL(sample_rows_am_kernel, dim3(2 * N), dim3(64), 0, ST(stream), O3, ldo, z_str, pos, cmd, N, C, q, K_steer,
                     K_throttle, action, logp, value, ord, allowed);
  return (int)hipGetLastError();
}

extern "C" int cadre_categorical_eval_am(const float* logits, int64_t ldl, const int64_t* actions, int32_t R, int32_t n_out,
                                         float* logp, float* entropy, const int32_t* ord, const int64_t* allowed,
                                         void* stream) {
  FAIL_IF(!logits || !actions || !logp || !entropy || R < 1 || n_out < 1 || n_out > 64 || ldl < n_out,
          "cadre_categorical_eval_am: bad argument");
  FAIL_IF(!ord, "cadre_categorical_eval_am: null rank table (device int32 [64]; ord[0] = -1 marks the categorical head)");
  FAIL_IF(!allowed, "cadre_categorical_eval_am: null allowed (device int64 [R])");
  hipLaunchKernelGGL(categorical_eval_am_kernel, dim3(R), dim3(64), 0, ST(stream), logits, ldl, actions, n_out, logp, entropy,
                     ord, allowed);
  return (int)hipGetLastError();
}

extern "C" int cadre_allowed_note(const void* table, const int32_t* slots, const int64_t* words, int32_t n, int32_t T,
                                  void* stream) {
  FAIL_IF(!table || !slots || !words || n < 1 || T < 1, "cadre_allowed_note: bad argument");
  hipLaunchKernelGGL(allowed_note_kernel, dim3((n + 63) / 64), dim3(64), 0, ST(stream), (const int64_t*)table, slots, words, n, T);
  return (int)hipGetLastError();
}

extern "C" int cadre_allowed_rows(const void* src_table, int32_t n_src, const int64_t* idx, int32_t Bw, int32_t T,
                                  const int32_t* pos, int32_t B, int64_t* out, void* stream) {
  FAIL_IF(!src_table || !idx || !out || n_src < 2 || (n_src & 1) || Bw < 1 || T < 1 || (n_src / 2) * (int64_t)Bw > B,
          "cadre_allowed_rows: bad argument ((n_src / 2) * Bw <= B)");
  hipLaunchKernelGGL(allowed_rows_kernel, dim3((Bw + 255) / 256, n_src), dim3(256), 0, ST(stream), (const int64_t*)src_table,
                     n_src, idx, Bw, T, pos, B, out);
  return (int)hipGetLastError();
}

extern "C" int cadre_ppo_am_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                                 const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                                 const float* old_logp, const float* adv, int32_t B, int32_t C, int32_t n_out_steer,
                                 int32_t n_out_throttle, double* hp, float clip, float value_coeff, float clip_coeff,
                                 float ent_coeff, float inv_b, float* losses, float* dlogits, float* dvalues, float* scratch,
                                 const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch, float target_kl,
                                 int32_t* stop, const int32_t* ord, const int64_t* allowed, float* am_stats, int32_t am_F,
                                 float* am_scratch, void* stream) {
  FAIL_IF(!logits || !values || !actions || !commands || !old_values || !returns || !old_logp || !adv || !losses ||
              !dlogits || !dvalues || !scratch || B < 1 || C < 1 || n_out_steer < 1 || n_out_steer > MAX_NOUT || n_out_throttle < 1 ||
              n_out_throttle > MAX_NOUT || ldl < n_out_steer || ldl < n_out_throttle || ldl > 64,
          "cadre_ppo_am_loss: bad argument");
  FAIL_IF(!ord, "cadre_ppo_am_loss: null rank table (device int32 [2][64]; ord[h][0] = -1 marks a categorical head)");
  FAIL_IF(!allowed, "cadre_ppo_am_loss: null allowed (device int64 [2][B]; bit k set: bin k may be chosen, no bit among K: unmasked)");
  FAIL_IF(stats_row && (F < CADRE_PPO_STATS_FIELDS || !stats_scratch || !(target_kl >= 0.f) || (target_kl > 0.f && !stop)),
          "cadre_ppo_am_loss: bad stats argument (F >= CADRE_PPO_STATS_FIELDS, target_kl >= 0, a stop flag with target_kl > 0)");
  FAIL_IF(am_stats && (am_F < CADRE_AM_STATS_FIELDS || !am_scratch),
          "cadre_ppo_am_loss: bad mask stats argument (am_F >= CADRE_AM_STATS_FIELDS, am_scratch of 10 * ceil(B / 16) floats)");
  FAIL_IF(hp && ((uintptr_t)hp & 7), "cadre_ppo_am_loss: bad hyper-parameter block (device double[CADRE_HP_FIELDS], 8-byte aligned)");
  const am_stats_t so{stats_row, F, stats_scratch, target_kl, stop, am_stats, am_F, am_scratch};
  const dim3 grid((B + 15) / 16, 2), block(256);
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
#define CADRE_AM_LAUNCH(S_, H_)                                                                                               \
  hipLaunchKernelGGL((ppo_am_loss_kernel<S_, H_>), grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, \
                     commands, old_values, returns, old_logp, adv, B, C, n_out_steer, n_out_throttle, hp, clip, value_coeff,  \
                     clip_coeff, ent_coeff, inv_b, losses, dlogits, dvalues, scratch, poison, so, ord, allowed)
  if (stats_row && hp) CADRE_AM_LAUNCH(true, true);
  else if (stats_row) CADRE_AM_LAUNCH(true, false);
  else if (hp) CADRE_AM_LAUNCH(false, true);
  else CADRE_AM_LAUNCH(false, false);
#undef CADRE_AM_LAUNCH
  return (int)hipGetLastError();
}
