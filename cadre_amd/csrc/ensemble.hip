// ensemble.hip — one env step of N evaluation environments served by an ensemble of M snapshots (eval.py:53-63 of the
// reference: every agent acts on the observation, agent.avg_action averages their controls).  The nets of a GROUP of Mg
// agents live in one stacked parameter arena with Mg * C commands: agent j's net (head h, command c) is arena net
// h * Mg * C + j * C + c, and all of them read the same sorted rows of one LSTM input block (row_seg tiled per agent), so
// a group is one LSTM + MLP launch chain.  This file holds what follows the chain:
//
//   cadre_sample_rows_ens     sampling (or the greedy pick) for every (environment, group agent, head): one wave each
//   cadre_ensemble_controls   the control average of agent.py:83-95 per environment, in float64, on the device
//
// Everything this file writes is written with plain stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"
#include "ordinal.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------------------- sampling
// The statements of sample_rows_kernel (act_batch.hip) per (environment e, group agent j, head h): the same logits and
// the same q give the same bits.  q == nullptr: the divisor is exactly 1.0f, i.e. the first largest probability wins.
template <bool ORD>
__global__ __launch_bounds__(64) void sample_rows_ens_kernel(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos,
                                                             const int32_t* cmd, int N, int C, int Mg, int m0, int M,
                                                             const float* q, int K0, int K1, int64_t* action, float* logp,
                                                             float* value, const int32_t* ord) {
  const int h = blockIdx.x & 1, ej = blockIdx.x >> 1, lane = threadIdx.x;
  const int e = ej / Mg, j = ej - e * Mg;
  const int K = h ? K1 : K0;
  const int c = cmd[e], p = pos[e];
  if (c < 0 || c >= C || p < 0 || p >= N) return;                 // (the host checked)
  const int z = 2 * (h * Mg * C + j * C + c);
  const int64_t o = ((int64_t)e * M + m0 + j) * 2 + h;            // slot of (environment, agent, head) in q and the outputs
  const float* lr = O3 + (int64_t)z * z_str + (int64_t)p * ldo;
  float x = lane < K ? lr[lane] : -INFINITY;
  if constexpr (ORD) {
    const int32_t* oh = ord + h * 64;
    if (oh[0] >= 0) {
      float s, t;
      x = ord_logits(x, lane < K, lane < K ? oh[lane] : lane, lane, s, t);
    }
  }
  const float mx = wave_max64(x);
  const float se = wave_sum64(lane < K ? expf(x - mx) : 0.f);
  const float lg = x - (mx + logf(se));
  const float mx2 = wave_max64(lane < K ? lg : -INFINITY);
  const float e2 = lane < K ? expf(lg - mx2) : 0.f;
  const float pr = e2 / wave_sum64(e2);
  const float pn = pr / wave_sum64(pr);
  const float qv = q ? q[o * 64 + lane] : 1.0f;
  float best = lane < K ? pn / qv : -INFINITY;
  int bi = lane;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const float lsel = __shfl(lg, bi, 64);
  if (lane == 0) {
    action[o] = bi;
    logp[o] = lsel;
    value[o] = O3[(int64_t)(z + 1) * z_str + (int64_t)p * ldo];
  }
}

// ---------------------------------------------------------------------------- control average
// Thread = environment.  numpy's np.array([...]).mean(0) of agent.py:83-95: each column summed in agent order in float64,
// then divided by the count; no contraction, so every operation rounds where numpy's does.
__global__ __launch_bounds__(64) void ensemble_controls_kernel(const int64_t* action, int N, int M, const double* steer_tab,
                                                               int Ks, const double* throttle_tab, int Kt, double* controls) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= N) return;
  double s = 0.0, t = 0.0, b = 0.0;
  bool bad = false;
  for (int m = 0; m < M; ++m) {
    const int64_t a0 = action[((int64_t)e * M + m) * 2], a1 = action[((int64_t)e * M + m) * 2 + 1];
    if (a0 < 0 || a0 >= Ks || a1 < 0 || a1 >= Kt) {              // never index outside a table
      bad = true;
      continue;
    }
    s = s + steer_tab[a0];
    t = t + throttle_tab[2 * a1];
    b = b + throttle_tab[2 * a1 + 1];
  }
  s = s / (double)M;
  t = t / (double)M;
  b = b / (double)M;
  if (M > 1 && b < 0.5) b = 0.0;
  if (bad) s = t = b = (double)NAN;
  controls[(int64_t)e * 3] = s;
  controls[(int64_t)e * 3 + 1] = t;
  controls[(int64_t)e * 3 + 2] = b;
}

}  // namespace

extern "C" int cadre_sample_rows_ens(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd,
                                     int32_t N, int32_t C, int32_t Mg, int32_t m0, int32_t M, const float* q, int32_t K_steer,
                                     int32_t K_throttle, int64_t* action, float* logp, float* value, const int32_t* ord,
                                     void* stream) {
  FAIL_IF(!O3 || !pos || !cmd || !action || !logp || !value, "cadre_sample_rows_ens: null operand");
  FAIL_IF(N < 1 || C < 1 || Mg < 1 || (int64_t)Mg * C > 16 || m0 < 0 || M < 1 || (int64_t)m0 + Mg > M || K_steer < 1 ||
              K_steer > 64 || K_throttle < 1 || K_throttle > 64 || ldo < K_steer || ldo < K_throttle ||
              z_str < (int64_t)N * ldo || (int64_t)N * Mg > (1 << 29),
          "cadre_sample_rows_ens: bad argument (N >= 1, C >= 1, Mg >= 1, Mg * C <= 16, 0 <= m0, m0 + Mg <= M, 1 <= K <= 64, "
          "ldo >= K, z_str >= N * ldo)");
  const dim3 grid((unsigned)(2 * N * Mg));
  if (ord)
    hipLaunchKernelGGL(sample_rows_ens_kernel<true>, grid, dim3(64), 0, ST(stream), O3, ldo, z_str, pos, cmd, N, C, Mg, m0, M, q,
                       K_steer, K_throttle, action, logp, value, ord);
  else
    hipLaunchKernelGGL(sample_rows_ens_kernel<false>, grid, dim3(64), 0, ST(stream), O3, ldo, z_str, pos, cmd, N, C, Mg, m0, M,
                       q, K_steer, K_throttle, action, logp, value, nullptr);
  return (int)hipGetLastError();
}

extern "C" int cadre_ensemble_controls(const int64_t* action, int32_t N, int32_t M, const double* steer_tab, int32_t K_steer,
                                       const double* throttle_tab, int32_t K_throttle, double* controls, void* stream) {
  FAIL_IF(!action || !steer_tab || !throttle_tab || !controls, "cadre_ensemble_controls: null operand");
  FAIL_IF(N < 1 || M < 1 || K_steer < 1 || K_throttle < 1,
          "cadre_ensemble_controls: bad argument (N >= 1, M >= 1, K_steer >= 1, K_throttle >= 1)");
  hipLaunchKernelGGL(ensemble_controls_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, ST(stream), action, N, M, steer_tab,
                     K_steer, throttle_tab, K_throttle, controls);
  return (int)hipGetLastError();
}
