// reuse.hip — sample reuse in the PPO step (GePPO, Queeney et al. 2021): the rows of the last few rollouts ride in the policy
// update as further worker entries, with V-trace targets (Espeholt et al. 2018) and truncated importance weights.
//
//   cadre_reuse_record   logp_now[h][row_id], value_now[h][row_id] = the current nets' log-probability of the row's stored action
//                        and critic output, for the rows of a minibatch: the addressing and grid of cadre_aux_record
//   cadre_vtrace_multi   for every stale storage in one launch: ratio = pi_now / mu per row, the V-trace value targets, the
//                        policy advantages (normalised per storage, then times the truncated weight): the twin of cadre_gae_multi
//
// The record forms the log-probability with the statements of ppo_loss_body (cadre_kernels.hip), so a row recorded from logits
// X and fed to the loss on the same X with old_logp := logp_now has lp - old_logp == 0 and ratio == expf(0) == 1 exactly.  The
// scan is gae_multi_kernel's (rollout_finish.hip), statement for statement, with the importance factors multiplied in: with
// logp_now == behaviour_logp and both bars >= 1 every factor is exactly 1 and the outputs are cadre_gae_multi's bits.
//
// Everything this file writes is written with plain vector stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"
#include "ordinal.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)
#define MAX_NOUT 64

namespace {

constexpr int MAX_T = 3000;      // 5 (T + 1) floats of LDS stay below 64 KiB, as in cadre_gae_multi

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
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct reuse_rows_t {
  const int32_t* pos;      // [2][B] workspace position of unsorted row u (NULL: identity)
  const int64_t* row_id;   // [2][B] table row of unsorted row u
  float* logp_now;         // [2][R]
  float* value_now;        // [2][R]
  int32_t R;
};

// aux_record_kernel's layout: one wave per unsorted row u (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups.  A position
// outside 0 .. B - 1, a command outside 0 .. C - 1 or a row_id outside 0 .. R - 1 writes nothing; an action outside 0 .. K - 1
// (the bootstrap row of a storage has none) writes the value only.
__global__ __launch_bounds__(256) void reuse_record_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                           int64_t ldv, int64_t v_ns, const int32_t* commands,
                                                           const int64_t* actions, reuse_rows_t rr, int B, int C, int n_steer,
                                                           int n_throttle, const int32_t* ord) {
  const int hd = blockIdx.y;
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane;
  if (ordinal) rk = lane < K ? ord[hd * 64 + lane] : lane;
  for (int i = 0; i < 4; ++i) {
    const int u = blockIdx.x * 16 + wave * 4 + i;
    if (u >= B) break;
    const int b = rr.pos ? rr.pos[hd * B + u] : u;
    if (b < 0 || b >= B) continue;
    const int row = hd * B + b;                    // per-head sample arrays are [2][B] in workspace order
    const int c = commands[row];
    const int64_t rid = rr.row_id[hd * B + u];
    if (!(c >= 0 && c < C && rid >= 0 && rid < rr.R)) continue;
    const int64_t a = actions[row];
    const int net = hd * C + c;
    const bool on = lane < K;
    float x = on ? logits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] : -INFINITY;
    float sg = 0.f, tg = 0.f;
    if (ordinal) x = ord_logits(x, on, rk, lane, sg, tg);
    // ---- ppo_loss_body
    const float mx = wave_max(x);
    const float se = wave_sum(on ? expf(x - mx) : 0.f);
    const float lse = mx + logf(se);
    const float lg = x - lse;
    const bool has_action = a >= 0 && a < K;
    const float lp = __shfl(lg, has_action ? (int)a : 0, 64);
    if (lane == 0) {
      const int64_t o = (int64_t)hd * rr.R + rid;
      if (has_action) rr.logp_now[o] = lp;
      rr.value_now[o] = values[(int64_t)net * v_ns + (int64_t)b * ldv];
    }
  }
}

struct vtrace_row_t {
  const float* rewards; const float* masks;
  const float* time_limits;      // may be NULL: no row was cut
  float* value_now;              // [T+1]; element T is overwritten with the bootstrap the scan used
  const float* boot_keep;        // [1]: 0 when the rollout ended in `done`, else 1
  const float* behaviour_logp; const float* logp_now;
  float* returns; float* adv; float* ratio;
  float* diag;                   // [CADRE_VTRACE_DIAG_FIELDS]
};

// gae_multi_kernel with the importance factors: the same staging, the same four statements for delta, the same normalisation.
// m[] is read for row t before ret[t] is written, so the two share one LDS array; r[t] likewise becomes the policy chain's
// return of row t once the reward of row t has been read.
__global__ __launch_bounds__(64) void vtrace_multi_kernel(const vtrace_row_t* rows, int T, float gamma, float gamma_tau,
                                                          int normalise, const double* state, float clip_r, float rho_bar,
                                                          float c_bar) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  float* r = sm, *V = sm + (T + 1), *m = V + (T + 1), *keep = m + (T + 1), *w = keep + (T + 1);
  float* ret = m, *pret = r;
  const int k = blockIdx.x, lane = threadIdx.x;
  const vtrace_row_t g = rows[k];
  const float scale = state ? (float)state[CADRE_RS_SCALE + (k & 1)] : 1.f;
  double s_w = 0.0, s_over = 0.0, s_rho = 0.0, s_rho2 = 0.0;
  float m_lr = 0.f;
  for (int i = lane; i <= T; i += 64) {
    float x = g.rewards[i];
    if (state) {
      x = (x * scale);
      x = fminf(fmaxf(x, -clip_r), clip_r);
    }
    r[i] = x;
    V[i] = g.value_now[i];
    m[i] = g.masks[i];
    keep[i] = g.time_limits ? (1.f - g.time_limits[i]) : 1.f;
    if (i < T) {
      const float lr = (g.logp_now[i] - g.behaviour_logp[i]);
      const float ratio = expf(lr);
      const float rho = fminf(rho_bar, ratio);
      w[i] = ratio;
      g.ratio[i] = ratio;
      s_w += (double)ratio;
      s_over += ratio > rho_bar ? 1.0 : 0.0;
      s_rho += (double)rho;
      s_rho2 += (double)rho * (double)rho;
      m_lr = fmaxf(m_lr, fabsf(lr));
    }
  }
  s_w = wave_sum_d(s_w); s_over = wave_sum_d(s_over); s_rho = wave_sum_d(s_rho); s_rho2 = wave_sum_d(s_rho2);
  m_lr = wave_max(m_lr);
  if (lane == 0) {
    g.diag[0] = (float)(s_w / T);
    g.diag[1] = (float)(s_over / T);
    g.diag[2] = m_lr;
    g.diag[3] = (float)((s_rho * s_rho) / ((double)T * s_rho2));
  }
  __syncthreads();
  if (lane == 0) {
    V[T] = g.boot_keep[0] != 0.f ? V[T] : 0.f;          // a select: 0 * V would keep the sign of V
    float acc = 0.f, gae = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const float rho_t = fminf(rho_bar, w[t]);
      const float cw_t = fminf(c_bar, w[t]);
      const float t1 = (gamma * V[t + 1]);
      const float t2 = (t1 * m[t]);
      const float t3 = (r[t] + t2);
      const float delta = (t3 - V[t]);
      const float u1 = (gamma_tau * m[t]);
      const float a2 = (u1 * acc);                      // the policy advantage: GAE whose tail is the V-trace-corrected chain
      gae = (delta + a2);
      gae = (gae * keep[t]);
      const float rd = (rho_t * delta);
      const float uc = (u1 * cw_t);
      const float u2 = (uc * acc);
      acc = (rd + u2);
      acc = (acc * keep[t]);                            // a row cut by a time limit: returns[t] = V[t], both chains restart
      ret[t] = (acc + V[t]);                            // the V-trace value target v_s
      pret[t] = (gae + V[t]);                           // gae_multi's ret[t] of the policy chain
    }
    g.value_now[T] = V[T];
  }
  __syncthreads();
  double sum = 0.0;
  for (int i = lane; i < T; i += 64) {
    g.returns[i] = ret[i];
    const float a = (pret[i] - V[i]);                   // train.py:82
    r[i] = a;
    sum += (double)a;
  }
  sum = wave_sum_d(sum);
  if (!normalise) {
    for (int i = lane; i < T; i += 64) g.adv[i] = (r[i] * fminf(rho_bar, w[i]));
    return;
  }
  const double mean = sum / T;
  double sq = 0.0;
  for (int i = lane; i < T; i += 64) {
    const double d = (double)r[i] - mean;
    sq += d * d;
  }
  sq = wave_sum_d(sq);
  const float meanf = (float)mean;
  const float stdf = (float)sqrt(sq / (T - 1));         // torch.std default: unbiased
  const float den = (stdf + 1e-8f);
  for (int i = lane; i < T; i += 64) {                  // train.py:87, then the truncated weight
    const float an = ((r[i] - meanf) / den);
    g.adv[i] = (an * fminf(rho_bar, w[i]));
  }
}

}  // namespace

extern "C" int cadre_reuse_record(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                                  const int32_t* commands, const int64_t* actions, const int32_t* pos, const int64_t* row_id,
                                  int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, const int32_t* ord,
                                  float* logp_now, float* value_now, int32_t R, void* stream) {
  FAIL_IF(!logits || !values || !commands || !actions || !row_id || !logp_now || !value_now || B < 1 || C < 1 ||
              n_out_steer < 1 || n_out_steer > MAX_NOUT || n_out_throttle < 1 || n_out_throttle > MAX_NOUT ||
              ldl < n_out_steer || ldl < n_out_throttle || ldl > 64 || ldv < 1,
          "cadre_reuse_record: bad argument");
  FAIL_IF(R < 1, "cadre_reuse_record: the tables need R >= 1 rows");
  const reuse_rows_t rr{pos, row_id, logp_now, value_now, R};
  hipLaunchKernelGGL(reuse_record_kernel, dim3((B + 15) / 16, 2), dim3(256), 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns,
                     commands, actions, rr, B, C, n_out_steer, n_out_throttle, ord);
  return (int)hipGetLastError();
}

extern "C" int cadre_vtrace_multi(const void* row_table, int32_t n, int32_t T, float gamma, float gamma_tau, int32_t normalise,
                                  const double* state, float clip_r, float rho_bar, float c_bar, void* stream) {
  FAIL_IF(!row_table, "cadre_vtrace_multi: null operand");
  FAIL_IF(n < 1 || n > 65535 || T < 2 || T > MAX_T || (state && !(clip_r > 0.f)),
          "cadre_vtrace_multi: bad argument (1 <= n <= 65535 storages, 2 <= T <= 3000, clip_r > 0 with reward scaling)");
  FAIL_IF(!(rho_bar > 0.f) || !(rho_bar < INFINITY) || !(c_bar > 0.f) || !(c_bar < INFINITY),
          "cadre_vtrace_multi: bad truncation level (rho_bar and c_bar finite and > 0)");
  const size_t shm = sizeof(float) * 5 * (T + 1);
  hipLaunchKernelGGL(vtrace_multi_kernel, dim3(n), dim3(64), shm, ST(stream), (const vtrace_row_t*)row_table, T, gamma, gamma_tau,
                     normalise, state, clip_r, rho_bar, c_bar);
  return (int)hipGetLastError();
}
