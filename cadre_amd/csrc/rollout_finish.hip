// rollout_finish.hip — the stage between a rollout and its PPO update, for every storage of a learner section at once:
// the return statistics behind reward scaling (cadre_return_stats), GAE + advantage normalisation of all storages in one
// launch with the optional reward scaling and time-limit cut (cadre_gae_multi), and the twin of cadre_insert_rows that
// also writes the time-limit flag of a row (cadre_insert_rows_tl).
//
// Storages come as a device table of finish_row_t records; storage k belongs to head k & 1 (steer, throttle).  The scan of
// cadre_gae_multi is gae_kernel's (cadre_kernels.hip), statement for statement, with FMA contraction off.  Everything this
// file writes is written with plain stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

constexpr int MAX_T = 3000;      // 5 (T + 1) floats (GAE) and 20 T bytes (statistics) of LDS stay below 64 KiB

struct finish_row_t {
  const float* rewards; float* value_preds; const float* masks; const float* next_value; float* returns; float* adv;
  const float* time_limits;      // may be NULL: no row was cut
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------- return statistics
// One 64-lane workgroup per storage: stage r and m' = mask (1 - time_limit) in LDS, lane 0 runs the forward recurrence
// G_t = r_t + gamma m'_{t-1} G_{t-1} in fp64 from the carry of the state block, all lanes then form the storage's mean
// and M2 (two passes, shuffle tree: a fixed order).  The workgroup that finishes last (a ticket in scratch[0]) merges
// the storages of each head into the head's (count, mean, M2) with Chan's formula IN STORAGE ORDER and forms the scale,
// so the result does not depend on which workgroup that was.
__global__ __launch_bounds__(64) void return_stats_kernel(const finish_row_t* rows, int n, int T, double gamma,
                                                          double epsilon, double* state, double* scratch) {
#pragma clang fp contract(off)
  extern __shared__ double smd[];
  double* G = smd, *mp = smd + T;
  float* r = (float*)(mp + T);
  __shared__ unsigned int ticket;
  const int k = blockIdx.x, lane = threadIdx.x;
  const finish_row_t g = rows[k];
  for (int i = lane; i < T; i += 64) {
    r[i] = g.rewards[i];
    const double tl = g.time_limits ? (double)g.time_limits[i] : 0.0;
    mp[i] = (double)g.masks[i] * (1.0 - tl);
  }
  __syncthreads();
  double* carry = state + CADRE_RS_CARRY + 2 * k;
  if (lane == 0) {
    double acc = carry[0], pm = carry[1];
    for (int t = 0; t < T; ++t) {
      const double d = (gamma * pm);
      acc = ((double)r[t] + (d * acc));
      G[t] = acc;
      pm = mp[t];
    }
    carry[0] = acc;
    carry[1] = pm;
  }
  __syncthreads();
  double sum = 0.0;
  for (int i = lane; i < T; i += 64) sum += G[i];
  const double mean = wave_sum_d(sum) / T;
  double sq = 0.0;
  for (int i = lane; i < T; i += 64) {
    const double d = G[i] - mean;
    sq += d * d;
  }
  sq = wave_sum_d(sq);
  unsigned int* tick = (unsigned int*)scratch;
  if (lane == 0) {
    scratch[1 + 2 * k] = mean;
    scratch[2 + 2 * k] = sq;
    __threadfence();                                    // the partials are visible before the ticket is taken
    ticket = atomicAdd(tick, 1u);
  }
  __syncthreads();
  if (ticket != (unsigned int)(n - 1)) return;
  __threadfence();
  if (lane < 2) {                                       // lane = head
    const volatile double* part = scratch;
    double cnt = state[3 * lane], mu = state[3 * lane + 1], m2 = state[3 * lane + 2];
    for (int s = lane; s < n; s += 2) {
      const double mk = part[1 + 2 * s], qk = part[2 + 2 * s], nb = (double)T;
      const double tot = cnt + nb, delta = mk - mu;
      mu = mu + delta * nb / tot;
      m2 = m2 + qk + delta * delta * cnt * nb / tot;
      cnt = tot;
    }
    state[3 * lane] = cnt;
    state[3 * lane + 1] = mu;
    state[3 * lane + 2] = m2;
    state[CADRE_RS_SCALE + lane] = (double)(float)(1.0 / sqrt(m2 / cnt + epsilon));
  }
  if (lane == 0) *tick = 0u;                            // ready for the next launch on the stream
}

// ---------------------------------------------------------------------------- GAE of every storage
// gae_kernel (cadre_kernels.hip) with the storage taken from the table: the same statements in the same order, plus
// the staged reward scaled and clamped (scaling on) and `gae = gae * keep[t]` after the recurrence (keep = 1 - time_limit;
// 1.0f without flags, an exact identity).
__global__ __launch_bounds__(64) void gae_multi_kernel(const finish_row_t* rows, int T, float gamma, float gamma_tau,
                                                       int normalise, const double* state, float clip_r) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  float* r = sm, *V = sm + (T + 1), *m = V + (T + 1), *ret = m + (T + 1), *keep = ret + (T + 1);
  const int k = blockIdx.x, lane = threadIdx.x;
  const finish_row_t g = rows[k];
  const float scale = state ? (float)state[CADRE_RS_SCALE + (k & 1)] : 1.f;
  for (int i = lane; i <= T; i += 64) {
    float x = g.rewards[i];
    if (state) {
      x = (x * scale);
      x = fminf(fmaxf(x, -clip_r), clip_r);
    }
    r[i] = x;
    V[i] = g.value_preds[i];
    m[i] = g.masks[i];
    keep[i] = g.time_limits ? (1.f - g.time_limits[i]) : 1.f;
  }
  __syncthreads();
  if (lane == 0) {
    V[T] = g.next_value[0];                             // storage.py:70
    float gae = 0.f;
    for (int t = T - 1; t >= 0; --t) {                  // storage.py:72-76
      const float t1 = (gamma * V[t + 1]);
      const float t2 = (t1 * m[t]);
      const float t3 = (r[t] + t2);
      const float delta = (t3 - V[t]);
      const float u1 = (gamma_tau * m[t]);
      const float u2 = (u1 * gae);
      gae = (delta + u2);
      gae = (gae * keep[t]);                            // a row cut by a time limit: returns[t] = V[t], the chain restarts
      ret[t] = (gae + V[t]);
    }
    g.value_preds[T] = V[T];
  }
  __syncthreads();
  double sum = 0.0;
  for (int i = lane; i < T; i += 64) {
    g.returns[i] = ret[i];
    const float a = (ret[i] - V[i]);                    // train.py:82
    r[i] = a;                                           // reuse r[] for advantages
    sum += (double)a;
  }
  sum = wave_sum_d(sum);
  if (!normalise) {
    for (int i = lane; i < T; i += 64) g.adv[i] = r[i];
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
  for (int i = lane; i < T; i += 64)                    // train.py:87
    g.adv[i] = ((r[i] - meanf) / den);
}

// ---------------------------------------------------------------------------- storage insert with the time-limit flag
struct insert_tl_dst_t {
  float* obs; float* hn; float* cn; int64_t* action; float* logp; float* value_preds; float* rewards; float* masks;
  int32_t* command; float* time_limits;
};

// insert_rows_kernel (act_batch.hip) whose record carries the time_limits pointer and whose rm row carries a third float.
__global__ __launch_bounds__(128) void insert_rows_tl_kernel(const insert_tl_dst_t* dst, const int32_t* slot, int S,
                                                             int64_t ldo, int64_t ldh, int D, int Hd, int T,
                                                             const float* feat, int64_t ldf, const int64_t* action,
                                                             const float* logp, const float* value, const float* rm,
                                                             const int32_t* cmd) {
  const int k = blockIdx.x, y = blockIdx.y, e = k >> 1;
  const insert_tl_dst_t g = dst[k];
  const int64_t s = slot[k];
  if (s < 0 || s > T) return;                                     // (cursor in [0, T]: the host checked)
  if (y < S) {
    const float* src = feat + ((int64_t)e * S + y) * ldf;
    float* o = g.obs + (s * S + y) * ldo;
    for (int d = threadIdx.x; d < D; d += blockDim.x) o[d] = src[d];
    return;
  }
  if (s < T) {
    for (int d = threadIdx.x; d < Hd; d += blockDim.x) {
      g.hn[(s + 1) * ldh + d] = 0.f;
      g.cn[(s + 1) * ldh + d] = 0.f;
    }
  }
  if (threadIdx.x == 0) {
    g.action[s] = action[k];
    g.logp[s] = logp[k];
    g.value_preds[s] = value[k];
    g.rewards[s] = rm[3 * k];
    g.masks[s] = rm[3 * k + 1];
    g.time_limits[s] = rm[3 * k + 2];
    g.command[s] = cmd[e];
  }
}

}  // namespace

extern "C" int cadre_return_stats(const void* row_table, int32_t n, int32_t T, double gamma, double epsilon, int32_t update,
                                  double* state, double* scratch, void* stream) {
  FAIL_IF(!row_table || !state || !scratch, "cadre_return_stats: null operand");
  FAIL_IF(n < 2 || (n & 1) || n > 65534 || T < 2 || T > MAX_T || !(gamma >= 0.0 && gamma <= 1.0) || !(epsilon >= 0.0) ||
              !(epsilon < INFINITY),
          "cadre_return_stats: bad argument (an even number 2 .. 65534 of storages, 2 <= T <= 3000, 0 <= gamma <= 1, "
          "finite epsilon >= 0)");
  if (!update) return 0;                                          // evaluation / replay: the stored scale stands
  const size_t shm = (size_t)T * (2 * sizeof(double) + sizeof(float));
  hipLaunchKernelGGL(return_stats_kernel, dim3(n), dim3(64), shm, ST(stream), (const finish_row_t*)row_table, n, T, gamma,
                     epsilon, state, scratch);
  return (int)hipGetLastError();
}

extern "C" int cadre_gae_multi(const void* row_table, int32_t n, int32_t T, float gamma, float gamma_tau, int32_t normalise,
                               const double* state, float clip_r, void* stream) {
  FAIL_IF(!row_table, "cadre_gae_multi: null operand");
  FAIL_IF(n < 1 || n > 65535 || T < 2 || T > MAX_T || (state && !(clip_r > 0.f)),
          "cadre_gae_multi: bad argument (1 <= n <= 65535 storages, 2 <= T <= 3000, clip_r > 0 with reward scaling)");
  const size_t shm = sizeof(float) * 5 * (T + 1);
  hipLaunchKernelGGL(gae_multi_kernel, dim3(n), dim3(64), shm, ST(stream), (const finish_row_t*)row_table, T, gamma, gamma_tau,
                     normalise, state, clip_r);
  return (int)hipGetLastError();
}

extern "C" int cadre_insert_rows_tl(const void* dst_table, const int32_t* slot, int32_t n_dst, int32_t S, int64_t ldo,
                                    int64_t ldh, int32_t D, int32_t Hd, int32_t T, const float* feat, int64_t ldf,
                                    const int64_t* action, const float* logp, const float* value, const float* rm,
                                    const int32_t* cmd, void* stream) {
  FAIL_IF(!dst_table || !slot || !feat || !action || !logp || !value || !rm || !cmd, "cadre_insert_rows_tl: null operand");
  FAIL_IF(n_dst < 2 || (n_dst & 1) || S < 1 || T < 1 || D < 1 || Hd < 1 || ldo < D || ldh < Hd || ldf < D,
          "cadre_insert_rows_tl: bad argument (an even number >= 2 of storages, S >= 1, T >= 1, ldo >= D, ldh >= Hd, ldf >= D)");
  hipLaunchKernelGGL(insert_rows_tl_kernel, dim3(n_dst, S + 1), dim3(128), 0, ST(stream), (const insert_tl_dst_t*)dst_table,
                     slot, S, ldo, ldh, D, Hd, T, feat, ldf, action, logp, value, rm, cmd);
  return (int)hipGetLastError();
}
