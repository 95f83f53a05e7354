// suggest.hip — exploration suggestions (Zhang et al. 2021, "End-to-End Urban Driving by Imitating a Reinforcement Learning
// Coach", the exploration loss of its section 3.2): on the last rows before a named terminal event the PPO loss gains
// KL(pi(.|s) || p_z) towards a prior p_z chosen for that event.
//
//   cadre_suggest_note   events[k][slot[k]] = code[k] for the 2N storages of one env step
//   cadre_suggest_mark   per storage, the backward scan that turns the recorded event codes into a kind per row
//   cadre_suggest_rows   kind[h][pos[h][row]] = suggest_src[idx]: the kinds of a minibatch in the layout of the update
//   cadre_ppo_sug_loss   where cadre_ppo_loss_ord stands in the update: same addressing, grid, scratch protocol, poison and
//                        rank table.  A row of kind 0 runs exactly the statements of ppo_loss_body (cadre_kernels.hip); a row
//                        of kind z >= 1 adds sug_coeff inv_b KL(pi || softmax(prior[h][z])) and its logit gradient on top.
//                        The prior row is normalised by the statements that normalise the policy row: raw logits bit-equal to
//                        the prior row give lg == lq bit for bit, so the KL and its gradient are exact zeros.
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
#define SUG_MAX_Z 8

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

// ---------------------------------------------------------------------------- recording
__global__ __launch_bounds__(64) void suggest_note_kernel(const int64_t* table, const int32_t* slots, const int32_t* codes,
                                                          int n, int T) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  int32_t* ev = reinterpret_cast<int32_t*>(table[k]);
  const int s = slots[k];
  if (ev && s >= 0 && s <= T) ev[s] = codes[k];
}

// ---------------------------------------------------------------------------- marking
struct mark_src_t {
  const int32_t* events;       // [T + 1]
  const float* masks;          // [T + 1]
  const float* time_limits;    // [T + 1] or NULL
  int32_t* suggest;            // [T]
};

// One workgroup per storage.  Row t is a RESET row when it carries an event of this head with a horizon > 0, or else ends an
// episode (mask 0 or a time-limit flag).  The backward scan of the header leaves row t with the state set by the nearest reset
// row t' >= t, `left` lowered by t' - t: suggest[t] = e(t') when t' is an event row and horizon - (t' - t) > 0, else 0.  The
// nearest reset row is a suffix minimum over row indices: chunks of 256 rows from the end, a shuffle-free LDS ladder inside a
// chunk, the minimum of the chunks behind carried in a register.  All integers: the order of combination cannot matter.
#define MARK_NT 256
__global__ __launch_bounds__(MARK_NT) void suggest_mark_kernel(const mark_src_t* src, int T, int Z, const int32_t* horizon) {
  const mark_src_t g = src[blockIdx.x];
  const int hd = blockIdx.x & 1;
  __shared__ int32_t hz[SUG_MAX_Z + 1];
  __shared__ int32_t near_[MARK_NT];
  if ((int)threadIdx.x <= Z) hz[threadIdx.x] = threadIdx.x == 0 ? 0 : horizon[hd * (Z + 1) + threadIdx.x];
  __syncthreads();
  int carry = INT_MAX;                               // nearest reset row behind the current chunk
  const int nchunk = (T + MARK_NT - 1) / MARK_NT;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int t = ch * MARK_NT + (int)threadIdx.x;
    int r = INT_MAX;
    if (t < T) {
      const int e = g.events[t];
      const bool ev = e >= 1 && e <= Z && hz[e] > 0;
      const bool end = g.masks[t] == 0.f || (g.time_limits && g.time_limits[t] != 0.f);
      if (ev || end) r = t;
    }
    near_[threadIdx.x] = r;
    __syncthreads();
    for (int o = 1; o < MARK_NT; o <<= 1) {          // inclusive suffix minimum
      const int other = (int)threadIdx.x + o < MARK_NT ? near_[threadIdx.x + o] : INT_MAX;
      __syncthreads();
      r = min(r, other);
      near_[threadIdx.x] = r;
      __syncthreads();
    }
    const int first = near_[0];
    r = min(r, carry);
    if (t < T) {
      int out = 0;
      if (r < T) {                                   // (r != INT_MAX; a reset row is a row of this rollout)
        const int e = g.events[r];
        if (e >= 1 && e <= Z && hz[e] > 0 && hz[e] - (r - t) > 0) out = e;
      }
      g.suggest[t] = out;
    }
    carry = min(carry, first);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------- kinds of a minibatch
// Source zi = 2 * worker + head, as in gather_sorted_multi_kernel: unsorted row ob = worker * Bw + b of head hd goes to
// workspace position pos[hd * Bt + ob].
__global__ __launch_bounds__(256) void suggest_rows_kernel(const int64_t* src, int n_src, const int64_t* idx, int Bw, int T,
                                                           const int32_t* pos, int Bt, int32_t* kind) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x, zi = blockIdx.y;
  if (b >= Bw) return;
  const int wi = zi >> 1, hd = zi & 1;
  const int ob = wi * Bw + b;
  if (ob >= Bt) return;
  const int d = pos ? pos[hd * Bt + ob] : ob;
  if (d < 0 || d >= Bt) return;
  const int32_t* sg = reinterpret_cast<const int32_t*>(src[zi]);
  int32_t k = 0;
  if (sg) {
    const int64_t t = idx[(int64_t)zi * Bw + b];
    if (t < 0 || t >= T) return;
    k = sg[t];
  }
  kind[hd * Bt + d] = k;
}

// ---------------------------------------------------------------------------- the loss
#define PPO_NSTAT 6
#define SG_NPART 4                    // per workgroup: kl sum, marked rows, max kl, sum of p[mode of the prior]
struct sug_stats_t {
  float* row;           // [2 heads][F] PPO stats row of this step (STATS)
  int32_t F;
  float* part;          // [2 * nblk][PPO_NSTAT] per-workgroup partials
  float target_kl;      // > 0: KL gate armed
  int32_t* stop;        // sticky gate flag (may be NULL when the gate is off)
  float* sug_row;       // [2 heads][sug_F] suggestion stats row (NULL: none)
  int32_t sug_F;
  float* sug_part;      // [2 * nblk][SG_NPART] per-workgroup partials (always: the suggestion loss goes through it)
};

// One wave per row (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups: ppo_loss_body with, for a marked row, one more
// 64-lane pass over the prior row between the PPO gradient and its store.
template <bool STATS, bool HP>
__global__ __launch_bounds__(256) void ppo_sug_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                           int64_t ldv, int64_t v_ns, const int64_t* actions,
                                                           const int32_t* commands, const float* old_values,
                                                           const float* returns, const float* old_logp, const float* adv,
                                                           const int32_t* kind, const float* prior, int Z, int B, int C,
                                                           int n_steer, int n_throttle, double* hp, float clip,
                                                           float value_coeff, float clip_coeff, float ent_coeff, float inv_b,
                                                           float sug_coeff, float* losses, float* sug_losses, float* dlogits,
                                                           float* dvalues, float* scratch, const int32_t* poison, sug_stats_t so,
                                                           const int32_t* ord) {
  if constexpr (HP) {
    clip = (float)hp[CADRE_HP_CLIP];
    value_coeff = (float)hp[CADRE_HP_VALUE_COEFF];
    clip_coeff = (float)hp[CADRE_HP_CLIP_COEFF];
    ent_coeff = (float)hp[CADRE_HP_ENT_COEFF];
    sug_coeff = (float)hp[CADRE_HP_SUGGEST_COEFF];
  }
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool sstats = so.sug_row != nullptr;
  __shared__ float red[3 + PPO_NSTAT + SG_NPART][4];
  float s_act = 0.f, s_val = 0.f, s_ent = 0.f;     // lane 0 of each wave
  float s_kl = 0.f, s_okl = 0.f, s_cf = 0.f, s_vcf = 0.f, s_r = 0.f, m_lr = 0.f;   // (STATS only)
  float g_kl = 0.f, g_n = 0.f, g_mx = -INFINITY, g_pm = 0.f;   // marked rows: kl sum, rows, max kl, p[mode of the prior]
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
    // ---- the suggestion term of a marked row: + sug_coeff inv_b KL(pi || softmax(prior row))
    int z = kind[row];
    if (z < 1 || z > Z) z = 0;
    if (z != 0) {                                  // (wave-uniform)
      float y = on ? prior[(int64_t)(hd * (Z + 1) + z) * 64 + lane] : -INFINITY;
      const float qmx = wave_max(y);
      const float qse = wave_sum(on ? expf(y - qmx) : 0.f);
      const float qlse = qmx + logf(qse);
      const float lq = y - qlse;
      const float df = on ? lg - lq : 0.f;
      const float kl = wave_sum(on ? pk * df : 0.f);
      const float gs = on ? (sug_coeff * inv_b) * (pk * (df - kl)) : 0.f;
      gk = gk + gs;
      g_kl += kl;
      g_n += 1.f;
      g_mx = fmaxf(g_mx, kl);
      if (sstats) {
        // the prior's mode: the lowest index among its largest entries
        const unsigned long long hit = __ballot(on && y == qmx);
        const int top = hit ? __ffsll((long long)hit) - 1 : 0;
        g_pm += __shfl(pk, top, 64);
      }
    }
    if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
    if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_act; red[2][wave] = s_ent;
    red[3][wave] = s_kl; red[4][wave] = s_okl; red[5][wave] = s_cf;
    red[6][wave] = s_vcf; red[7][wave] = s_r; red[8][wave] = m_lr;
    red[9][wave] = g_kl; red[10][wave] = g_n; red[11][wave] = g_mx; red[12][wave] = g_pm;
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
    for (int k = 0; k < SG_NPART; ++k) {
      const float* r = red[9 + k];
      const float t = k == 2 ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
      __hip_atomic_store(so.sug_part + SG_NPART * me + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
      float sk = 0.f;
      for (int w = 0; w < total; ++w) sk += __hip_atomic_load(so.sug_part + SG_NPART * w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float bad = (poison && __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? __builtin_nanf("") : 0.f;
      losses[0] = value_coeff * 0.5f * sv * inv_b + bad;
      losses[1] = clip_coeff * sa * inv_b + bad;
      losses[2] = ent_coeff * sn * inv_b + bad;
      sug_losses[0] = sug_coeff * sk * inv_b + bad;
      if (sstats) {
        for (int h = 0; h < 2; ++h) {
          float t[SG_NPART] = {0.f, 0.f, -INFINITY, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < SG_NPART; ++k) {
              const float p = __hip_atomic_load(so.sug_part + SG_NPART * w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              t[k] = k == 2 ? fmaxf(t[k], p) : t[k] + p;
            }
          float* o = so.sug_row + h * so.sug_F;
          o[0] = t[1];
          o[1] = t[0] * inv_b;
          o[2] = t[1] > 0.f ? t[2] : 0.f;
          o[3] = t[1] > 0.f ? t[3] / t[1] : 0.f;
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
        // the gate, `applied` and (HP) the KL-adaptive lr: the rule of kl_rule.h on the PPO ratio's KL, as without suggestions
        if constexpr (HP) cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, hp[CADRE_HP_DESIRED_KL], hp);
        else cadre_kl_rule(kl[0], kl[1], so.target_kl, so.stop, so.row, so.F, 0.0, nullptr);
      }
      __hip_atomic_store(reinterpret_cast<unsigned*>(scratch), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

extern "C" int cadre_suggest_note(const void* table, const int32_t* slots, const int32_t* codes, int32_t n, int32_t T,
                                  void* stream) {
  FAIL_IF(!table || !slots || !codes || n < 1 || T < 1, "cadre_suggest_note: bad argument");
  hipLaunchKernelGGL(suggest_note_kernel, dim3((n + 63) / 64), dim3(64), 0, ST(stream), (const int64_t*)table, slots, codes, n, T);
  return (int)hipGetLastError();
}

extern "C" int cadre_suggest_mark(const void* table, int32_t n, int32_t T, int32_t Z, const int32_t* horizon, void* stream) {
  FAIL_IF(!table || !horizon || n < 1 || T < 1, "cadre_suggest_mark: bad argument");
  FAIL_IF(Z < 1 || Z > SUG_MAX_Z, "cadre_suggest_mark: Z (event kinds) must be in 1 .. 8");
  hipLaunchKernelGGL(suggest_mark_kernel, dim3(n), dim3(MARK_NT), 0, ST(stream), (const mark_src_t*)table, T, Z, horizon);
  return (int)hipGetLastError();
}

extern "C" int cadre_suggest_rows(const void* src_table, int32_t n_src, const int64_t* idx, int32_t Bw, int32_t T,
                                  const int32_t* pos, int32_t Bt, int32_t* kind, void* stream) {
  FAIL_IF(!src_table || !idx || !kind || n_src < 2 || (n_src & 1) || Bw < 1 || T < 1 || (n_src / 2) * (int64_t)Bw > Bt,
          "cadre_suggest_rows: bad argument ((n_src / 2) * Bw <= Bt)");
  hipLaunchKernelGGL(suggest_rows_kernel, dim3((Bw + 255) / 256, n_src), dim3(256), 0, ST(stream), (const int64_t*)src_table, n_src,
                     idx, Bw, T, pos, Bt, kind);
  return (int)hipGetLastError();
}

extern "C" int cadre_ppo_sug_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                                  const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                                  const float* old_logp, const float* adv, const int32_t* kind, const float* prior, int32_t Z,
                                  int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip,
                                  float value_coeff, float clip_coeff, float ent_coeff, float inv_b, float sug_coeff,
                                  float* losses, float* sug_losses, float* dlogits, float* dvalues, float* scratch,
                                  float* sug_scratch, const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch,
                                  float target_kl, int32_t* stop, float* sug_stats_row, int32_t sug_F, const int32_t* ord,
                                  void* stream) {
  FAIL_IF(!logits || !values || !actions || !commands || !old_values || !returns || !old_logp || !adv || !losses ||
              !dlogits || !dvalues || !scratch || B < 1 || C < 1 || n_out_steer < 1 || n_out_steer > MAX_NOUT || n_out_throttle < 1 ||
              n_out_throttle > MAX_NOUT || ldl < n_out_steer || ldl < n_out_throttle || ldl > 64,
          "cadre_ppo_sug_loss: bad argument");
  FAIL_IF(!ord, "cadre_ppo_sug_loss: null rank table (device int32 [2][64]; ord[h][0] = -1 marks a categorical head)");
  FAIL_IF(!kind, "cadre_ppo_sug_loss: null kind (device int32 [2][B]; 0 a plain PPO row, z >= 1 a row marked for prior z)");
  FAIL_IF(!prior, "cadre_ppo_sug_loss: null prior (device float [2][Z + 1][64] of raw log-priors)");
  FAIL_IF(!sug_losses || !sug_scratch, "cadre_ppo_sug_loss: null sug_losses or sug_scratch");
  FAIL_IF(Z < 1 || Z > SUG_MAX_Z, "cadre_ppo_sug_loss: Z (event kinds) must be in 1 .. 8");
  FAIL_IF(!isfinite(sug_coeff), "cadre_ppo_sug_loss: sug_coeff must be finite");
  FAIL_IF(stats_row && (F < CADRE_PPO_STATS_FIELDS || !stats_scratch || !(target_kl >= 0.f) || (target_kl > 0.f && !stop)),
          "cadre_ppo_sug_loss: bad stats argument (F >= CADRE_PPO_STATS_FIELDS, target_kl >= 0, a stop flag with target_kl > 0)");
  FAIL_IF(sug_stats_row && sug_F < CADRE_SUG_STATS_FIELDS, "cadre_ppo_sug_loss: bad suggestion stats argument (sug_F >= CADRE_SUG_STATS_FIELDS)");
  FAIL_IF(hp && ((uintptr_t)hp & 7), "cadre_ppo_sug_loss: bad hyper-parameter block (device double[CADRE_HP_FIELDS], 8-byte aligned)");
  const sug_stats_t so{stats_row, F, stats_scratch, target_kl, stop, sug_stats_row, sug_F, sug_scratch};
  const dim3 grid((B + 15) / 16, 2), block(256);
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
#define CADRE_SUG_LAUNCH(S_, H_)                                                                                               \
  hipLaunchKernelGGL((ppo_sug_loss_kernel<S_, H_>), grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, \
                     commands, old_values, returns, old_logp, adv, kind, prior, Z, B, C, n_out_steer, n_out_throttle, hp, clip, \
                     value_coeff, clip_coeff, ent_coeff, inv_b, sug_coeff, losses, sug_losses, dlogits, dvalues, scratch,      \
                     poison, so, ord)
  if (stats_row && hp) CADRE_SUG_LAUNCH(true, true);
  else if (stats_row) CADRE_SUG_LAUNCH(true, false);
  else if (hp) CADRE_SUG_LAUNCH(false, true);
  else CADRE_SUG_LAUNCH(false, false);
#undef CADRE_SUG_LAUNCH
  return (int)hipGetLastError();
}
