// phasic.hip — the auxiliary phase of Phasic Policy Gradient (Cobbe et al. 2020, the shared-trunk variant of its section 3.5):
// extra critic epochs over the rows of past rollouts while a KL term holds the policy at the distributions it had when the
// phase began.
//
//   cadre_aux_record   table[h][row_id] = the normalised log-probabilities of the current policy for the rows of a minibatch
//   cadre_aux_loss     forward + backward of  aux_value_coeff 0.5 mean (v - R)^2 + beta_clone mean KL(pi_old || pi)
//                      where ppo_loss_* (cadre_kernels.hip) and cadre_bc_loss (imitation.hip) stand in the update: same
//                      addressing, grid, scratch protocol, poison and rank table, so everything behind the loss launch (MLP /
//                      LSTM backward, clip + Adam) is indifferent to which of them ran
//
// Both kernels form the normalised logits lg with the statements of bc_loss_kernel (aux_row_lg below), and the loss forms
// p_old from the stored row with the statements that form pk from lg (aux_row_p): a row recorded from logits X and trained
// on the same X has p_old == pk bit for bit, so its KL and its logit gradient are exact zeros, not rounding noise.
//
// Everything this file writes is written with plain vector stores or agent-scope atomics.
#include <hip/hip_runtime.h>
#include <limits.h>
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

// x: this lane's raw logit (-inf on lanes >= K), already through ord_logits on an ordinal head -> x - logsumexp(x)
__device__ __forceinline__ float aux_row_lg(float x, bool on) {
  const float mx = wave_max(x);
  const float se = wave_sum(on ? expf(x - mx) : 0.f);
  const float lse = mx + logf(se);
  return x - lse;
}
// normalised log-probabilities -> probabilities (the second max / expf / wave_sum / divide of the loss kernels)
__device__ __forceinline__ float aux_row_p(float lg, bool on) {
  const float mx2 = wave_max(on ? lg : -INFINITY);
  const float e2 = on ? expf(lg - mx2) : 0.f;
  const float se2 = wave_sum(e2);
  return e2 / se2;
}

struct aux_rows_t {
  const int32_t* pos;      // [2][B] workspace position of unsorted row u (NULL: identity)
  const int64_t* row_id;   // [2][B] table row of unsorted row u
  float* table;            // [2][R][64]
  int32_t R;
};

// One wave per unsorted row u (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups.  The row's logits are at workspace
// position b = pos[u]; a position outside 0 .. B - 1, a command outside 0 .. C - 1 or a row_id outside 0 .. R - 1 writes nothing.
__global__ __launch_bounds__(256) void aux_record_kernel(const float* logits, int64_t ldl, int64_t l_ns, const int32_t* commands,
                                                         aux_rows_t ar, int B, int C, int n_steer, int n_throttle,
                                                         const int32_t* ord) {
  const int hd = blockIdx.y;
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane;
  if (ordinal) rk = lane < K ? ord[hd * 64 + lane] : lane;
  for (int i = 0; i < 4; ++i) {
    const int u = blockIdx.x * 16 + wave * 4 + i;
    if (u >= B) break;
    const int b = ar.pos ? ar.pos[hd * B + u] : u;
    if (b < 0 || b >= B) continue;
    const int c = commands[hd * B + b];
    const int64_t rid = ar.row_id[hd * B + u];
    if (!(c >= 0 && c < C && rid >= 0 && rid < ar.R)) continue;
    const int net = hd * C + c;
    const bool on = lane < K;
    float x = on ? logits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] : -INFINITY;
    float sg = 0.f, tg = 0.f;
    if (ordinal) x = ord_logits(x, on, rk, lane, sg, tg);
    const float lg = aux_row_lg(x, on);
    ar.table[((int64_t)hd * ar.R + rid) * 64 + lane] = on ? lg : -INFINITY;
  }
}

#define AUX_NSTAT CADRE_AUX_STATS_FIELDS
struct aux_stats_t {
  float* row;           // [2 heads][F] stats row of this step (NULL: no statistics)
  int32_t F;
  float* part;          // [2 * nblk][AUX_NSTAT] per-workgroup partials
};

// The layout of bc_loss_kernel over the UNSORTED rows u of the minibatch; row u lives at workspace position b = pos[u] (as a
// permutation of 0 .. B - 1 the positions cover every workspace row, so every row of dlogits / dvalues is written).  A row
// counts for head hd when its command and its row_id are in range; every other row gets exact zeros in all C nets of the head
// and adds nothing to any sum.  A position outside 0 .. B - 1 is skipped altogether.
__global__ __launch_bounds__(256) void aux_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                       int64_t ldv, int64_t v_ns, const int32_t* commands, const float* returns,
                                                       aux_rows_t ar, int B, int C, int n_steer, int n_throttle, float beta,
                                                       float value_coeff, float inv_b, float* losses, float* dlogits,
                                                       float* dvalues, float* scratch, const int32_t* poison, aux_stats_t so,
                                                       const int32_t* ord) {
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool stats = so.row != nullptr;
  __shared__ float red[2 + AUX_NSTAT][4];
  float s_val = 0.f, s_kl = 0.f;                   // lane 0 of each wave
  float s_st[AUX_NSTAT] = {0.f, -INFINITY, 0.f, 0.f, 0.f, 0.f};
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane, binv = lane;
  if (ordinal) {
    rk = lane < K ? ord[hd * 64 + lane] : lane;
    binv = ord_inverse(rk, lane);
  }
  for (int i = 0; i < 4; ++i) {
    const int u = blockIdx.x * 16 + wave * 4 + i;
    if (u >= B) break;
    const int b = ar.pos ? ar.pos[hd * B + u] : u;
    if (b < 0 || b >= B) continue;
    const int row = hd * B + b;                    // per-head sample arrays are [2][B] in workspace order
    const int c = commands[row];
    const int64_t rid = ar.row_id[hd * B + u];
    const bool own_ok = c >= 0 && c < C && rid >= 0 && rid < ar.R;
    for (int cc = 0; cc < C; ++cc) {
      if (own_ok && cc == c) continue;
      if (lane < ldl) dlogits[(int64_t)(hd * C + cc) * l_ns + (int64_t)b * ldl + lane] = 0.f;
      if (lane == 0) dvalues[(int64_t)(hd * C + cc) * v_ns + (int64_t)b * ldv] = 0.f;
    }
    if (!own_ok) continue;
    const int net = hd * C + c;
    const bool on = lane < K;
    float x = on ? logits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] : -INFINITY;
    float sg = 0.f, tg = 0.f;                      // (ordinal head) sigmoid(x), sigmoid(-x) of this lane's threshold unit
    if (ordinal) x = ord_logits(x, on, rk, lane, sg, tg);
    const float lg = aux_row_lg(x, on);
    const float pk = aux_row_p(lg, on);
    const float lo = ar.table[((int64_t)hd * ar.R + rid) * 64 + lane];
    const float po = aux_row_p(lo, on);
    // KL(pi_old || pi) = sum_k p_old,k (lo_k - lg_k); not clamped at zero (a bin of probability 0 adds nothing)
    const float kl = wave_sum((on && po != 0.f) ? po * (lo - lg) : 0.f);
    const float v = values[(int64_t)net * v_ns + (int64_t)b * ldv];
    const float R = returns[row];
    const float dv = v - R;
    s_val += dv * dv;
    s_kl += kl;
    if (stats) {
      const float H = -wave_sum(on ? pk * lg : 0.f);
      s_st[0] += kl;
      s_st[1] = fmaxf(s_st[1], kl);
      s_st[2] += fabsf(dv);
      s_st[3] += H;
      s_st[4] += dv * dv;
      s_st[5] += 1.f;
    }
    if (lane == 0) dvalues[(int64_t)net * v_ns + (int64_t)b * ldv] = value_coeff * inv_b * dv;
    // d KL / d logit_k = p_k - p_old,k   (sum_k p_old,k = 1)
    float gk = on ? beta * inv_b * (pk - po) : 0.f;
    if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
    if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_kl;
#pragma unroll
    for (int k = 0; k < AUX_NSTAT; ++k) red[2 + k][wave] = s_st[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nblk = gridDim.x, me = hd * nblk + blockIdx.x, total = 2 * nblk;
    float* part = scratch + 4;                      // [total][3] (two used); scratch[0] is the arrival counter (zero on entry, reset below)
    for (int k = 0; k < 2; ++k)
      __hip_atomic_store(part + 3 * me + k, (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    if (stats) {
      for (int k = 0; k < AUX_NSTAT; ++k) {
        const float* r = red[2 + k];
        const float t = k == 1 ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
        __hip_atomic_store(so.part + AUX_NSTAT * me + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(scratch), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (unsigned)(total - 1)) {          // last arriver: every partial has been published
      float sv = 0.f, sk = 0.f;
      for (int w = 0; w < total; ++w) {             // workgroup order: equal inputs give equal bits
        sv += __hip_atomic_load(part + 3 * w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sk += __hip_atomic_load(part + 3 * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const float bad = (poison && __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? __builtin_nanf("") : 0.f;
      losses[0] = value_coeff * 0.5f * sv * inv_b + bad;
      losses[1] = beta * sk * inv_b + bad;
      losses[2] = 0.f + bad;
      if (stats) {
        for (int h = 0; h < 2; ++h) {
          float t[AUX_NSTAT] = {0.f, -INFINITY, 0.f, 0.f, 0.f, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < AUX_NSTAT; ++k) {
              const float p = __hip_atomic_load(so.part + AUX_NSTAT * w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              t[k] = k == 1 ? fmaxf(t[k], p) : t[k] + p;
            }
          float* o = so.row + h * so.F;
          for (int k = 0; k < AUX_NSTAT; ++k) o[k] = k == 1 ? (t[5] > 0.f ? t[1] : 0.f) : t[k] * inv_b;   // (no row counted: max 0)
        }
      }
      __hip_atomic_store(reinterpret_cast<unsigned*>(scratch), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

extern "C" int cadre_aux_record(const float* logits, int64_t ldl, int64_t l_ns, const int32_t* commands, const int32_t* pos,
                                const int64_t* row_id, int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle,
                                const int32_t* ord, float* table, int32_t R, void* stream) {
  FAIL_IF(!logits || !commands || !row_id || !table || B < 1 || C < 1 || n_out_steer < 1 || n_out_steer > MAX_NOUT ||
              n_out_throttle < 1 || n_out_throttle > MAX_NOUT || ldl < n_out_steer || ldl < n_out_throttle || ldl > 64,
          "cadre_aux_record: bad argument");
  FAIL_IF(R < 1, "cadre_aux_record: the table needs R >= 1 rows");
  const aux_rows_t ar{pos, row_id, table, R};
  hipLaunchKernelGGL(aux_record_kernel, dim3((B + 15) / 16, 2), dim3(256), 0, ST(stream), logits, ldl, l_ns, commands, ar, B, C,
                     n_out_steer, n_out_throttle, ord);
  return (int)hipGetLastError();
}

extern "C" int cadre_aux_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                              const int32_t* commands, const float* returns, const int32_t* pos, const int64_t* row_id,
                              const float* table, int32_t R, int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle,
                              float beta_clone, float aux_value_coeff, float inv_b, float* losses, float* dlogits,
                              float* dvalues, float* scratch, const int32_t* poison, float* stats_row, int32_t F,
                              float* stats_scratch, const int32_t* ord, void* stream) {
  FAIL_IF(!logits || !values || !commands || !returns || !row_id || !table || !losses || !dlogits || !dvalues || !scratch ||
              B < 1 || C < 1 || n_out_steer < 1 || n_out_steer > MAX_NOUT || n_out_throttle < 1 || n_out_throttle > MAX_NOUT ||
              ldl < n_out_steer || ldl < n_out_throttle || ldl > 64,
          "cadre_aux_loss: bad argument");
  FAIL_IF(R < 1, "cadre_aux_loss: the table needs R >= 1 rows");
  FAIL_IF(stats_row && (F < CADRE_AUX_STATS_FIELDS || !stats_scratch),
          "cadre_aux_loss: bad stats argument (F >= CADRE_AUX_STATS_FIELDS and a stats scratch)");
  const aux_rows_t ar{pos, row_id, const_cast<float*>(table), R};
  const aux_stats_t so{stats_row, F, stats_scratch};
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
  hipLaunchKernelGGL(aux_loss_kernel, dim3((B + 15) / 16, 2), dim3(256), 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns,
                     commands, returns, ar, B, C, n_out_steer, n_out_throttle, beta_clone, aux_value_coeff, inv_b, losses,
                     dlogits, dvalues, scratch, poison, so, ord);
  return (int)hipGetLastError();
}
