// act_batch.hip — one env step of N environments in one launch chain (CadreAgent.act_batch, ppo_agent/agent.py:114-141 of
// the reference called once per environment): the LSTM input rows of every environment's sliding window, the sampling of
// every (environment, head) pair and the rollout-storage insert of all 2N storages, one launch each.
//
// Rows of the LSTM / MLP pass are sorted by command (row_seg of ppo_update.hip): environment e sits at sorted row pos[e];
// the host builds pos / seg from the N host-side commands.  Everything this file writes is written with plain stores.
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

constexpr int LAT = 512;     // encoder latent width
constexpr int NMEAS = 18;    // measurements: 3 values repeated 6 times (agent.py:97-112)

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

// ---------------------------------------------------------------------------- window rows
// One workgroup per environment; thread = column.  A column of the ring is read and rewritten by one thread only, in
// ascending window order (row s + 1 is read before row s + 1 is written), so the in-place shift needs no second buffer.
__global__ __launch_bounds__(256) void act_windows_kernel(float* ring, int64_t ring_env_str, const float* fresh,
                                                          int64_t ld_fresh, const int32_t* mode, const int32_t* first,
                                                          const double* meas, const int32_t* pos, int N, int S, int F, float* X,
                                                          int64_t ldx, int DP, float* feat, int64_t ldf) {
  const int e = blockIdx.x;
  const int shifted = mode[e];
  const int f0 = first[e];
  const int p = pos[e];
  if (p < 0 || p >= N || f0 < 0 || f0 + (shifted ? 1 : S) > F) return;     // (the host checked; never index outside)
  float* rg = ring + (int64_t)e * ring_env_str;
  const double* me = meas + (int64_t)e * S * 3;
  for (int d = threadIdx.x; d < DP; d += blockDim.x) {
    for (int s = 0; s < S; ++s) {
      float v;
      if (d < LAT) {
        if (shifted)
          v = s + 1 < S ? rg[(int64_t)(s + 1) * LAT + d] : fresh[(int64_t)f0 * ld_fresh + d];
        else
          v = fresh[(int64_t)(f0 + s) * ld_fresh + d];
        rg[(int64_t)s * LAT + d] = v;
      } else if (d < LAT + NMEAS) {
        v = (float)me[s * 3 + (d - LAT) % 3];          // cadre_append_measurements
      } else {
        v = 0.f;
      }
      X[((int64_t)s * N + p) * ldx + d] = v;
      if (feat) feat[((int64_t)e * S + s) * ldf + d] = v;
    }
  }
}

// ---------------------------------------------------------------------------- sampling
// sample_kernel (cadre_kernels.hip) per (environment, head): argmax(p / q), lowest index wins ties; wave = pair.
// ORD (cadre_sample_rows_ord): `ord` int32 [2][64] holds each head's bin -> rank table (ordinal.h); a head whose first entry
// is -1 is the plain categorical head and runs exactly the statements of the ORD = false kernel.
template <bool ORD>
__global__ __launch_bounds__(64) void sample_rows_kernel(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos,
                                                         const int32_t* cmd, int N, int C, const float* q, int K0, int K1,
                                                         int64_t* action, float* logp, float* value, const int32_t* ord) {
  const int e = blockIdx.x >> 1, h = blockIdx.x & 1, lane = threadIdx.x;
  const int K = h ? K1 : K0;
  const int c = cmd[e], p = pos[e];
  if (c < 0 || c >= C || p < 0 || p >= N) return;                 // (the host checked)
  const int z = 2 * (h * C + c);
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
  float best = lane < K ? pn / q[((int64_t)e * 2 + h) * 64 + lane] : -INFINITY;
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

// ---------------------------------------------------------------------------- storage insert
struct insert_dst_t {
  float* obs; float* hn; float* cn; int64_t* action; float* logp; float* value_preds; float* rewards; float* masks;
  int32_t* command;
};

// Storage k = 2 e + head (steer, throttle).  blockIdx.y < S: window row y of obs[slot]; y == S: the zero hidden state of
// slot + 1 (while slot < T) and the scalars.
__global__ __launch_bounds__(128) void insert_rows_kernel(const insert_dst_t* dst, const int32_t* slot, int S, int64_t ldo,
                                                          int64_t ldh, int D, int Hd, int T, const float* feat, int64_t ldf,
                                                          const int64_t* action, const float* logp, const float* value,
                                                          const float* rm, const int32_t* cmd) {
  const int k = blockIdx.x, y = blockIdx.y, e = k >> 1;
  const insert_dst_t g = dst[k];
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
    g.rewards[s] = rm[2 * k];
    g.masks[s] = rm[2 * k + 1];
    g.command[s] = cmd[e];
  }
}

}  // namespace

extern "C" int cadre_act_windows(float* ring, int64_t ring_env_str, int32_t n_ring, const float* fresh, int64_t ld_fresh,
                                 int32_t F, const int32_t* mode, const int32_t* first, const double* meas, const int32_t* pos,
                                 int32_t N, int32_t S, float* X, int64_t ldx, int32_t DP, float* feat, int64_t ldf,
                                 void* stream) {
  FAIL_IF(!ring || !fresh || !mode || !first || !meas || !pos || !X, "cadre_act_windows: null operand");
  FAIL_IF(N < 1 || N > n_ring || S < 1 || F < 1 || DP < LAT + NMEAS || ldx < DP || ld_fresh < LAT ||
              ring_env_str < (int64_t)S * LAT || (feat && ldf < DP),
          "cadre_act_windows: bad argument (1 <= N <= ring slots, S >= 1, F >= 1, DP >= 530, ldx >= DP, ring slot >= S x 512)");
  hipLaunchKernelGGL(act_windows_kernel, dim3(N), dim3(256), 0, ST(stream), ring, ring_env_str, fresh, ld_fresh, mode, first,
                     meas, pos, N, S, F, X, ldx, DP, feat, ldf);
  return (int)hipGetLastError();
}

extern "C" int cadre_sample_rows(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd, int32_t N,
                                 int32_t C, const float* q, int32_t K_steer, int32_t K_throttle, int64_t* action, float* logp,
                                 float* value, void* stream) {
  FAIL_IF(!O3 || !pos || !cmd || !q || !action || !logp || !value, "cadre_sample_rows: null operand");
  FAIL_IF(N < 1 || C < 1 || C > 16 || K_steer < 1 || K_steer > 64 || K_throttle < 1 || K_throttle > 64 || ldo < K_steer ||
              ldo < K_throttle || z_str < (int64_t)N * ldo,
          "cadre_sample_rows: bad argument (N >= 1, 1 <= C <= 16, 1 <= K <= 64, ldo >= K, z_str >= N * ldo)");
  hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(2 * N), dim3(64), 0, ST(stream), O3, ldo, z_str, pos, cmd, N, C, q, K_steer,
                     K_throttle, action, logp, value, nullptr);
  return (int)hipGetLastError();
}

extern "C" int cadre_sample_rows_ord(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd,
                                     int32_t N, int32_t C, const float* q, int32_t K_steer, int32_t K_throttle, int64_t* action,
                                     float* logp, float* value, const int32_t* ord, void* stream) {
  FAIL_IF(!O3 || !pos || !cmd || !q || !action || !logp || !value, "cadre_sample_rows_ord: null operand");
  FAIL_IF(!ord, "cadre_sample_rows_ord: null rank table (device int32 [2][64]; ord[h][0] = -1 marks a categorical head)");
  FAIL_IF(N < 1 || C < 1 || C > 16 || K_steer < 1 || K_steer > 64 || K_throttle < 1 || K_throttle > 64 || ldo < K_steer ||
              ldo < K_throttle || z_str < (int64_t)N * ldo,
          "cadre_sample_rows_ord: bad argument (N >= 1, 1 <= C <= 16, 1 <= K <= 64, ldo >= K, z_str >= N * ldo)");
  hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(2 * N), dim3(64), 0, ST(stream), O3, ldo, z_str, pos, cmd, N, C, q, K_steer,
                     K_throttle, action, logp, value, ord);
  return (int)hipGetLastError();
}

extern "C" int cadre_insert_rows(const void* dst_table, const int32_t* slot, int32_t n_dst, int32_t S, int64_t ldo, int64_t ldh,
                                 int32_t D, int32_t Hd, int32_t T, const float* feat, int64_t ldf, const int64_t* action,
                                 const float* logp, const float* value, const float* rm, const int32_t* cmd, void* stream) {
  FAIL_IF(!dst_table || !slot || !feat || !action || !logp || !value || !rm || !cmd, "cadre_insert_rows: null operand");
  FAIL_IF(n_dst < 2 || (n_dst & 1) || S < 1 || T < 1 || D < 1 || Hd < 1 || ldo < D || ldh < Hd || ldf < D,
          "cadre_insert_rows: bad argument (an even number >= 2 of storages, S >= 1, T >= 1, ldo >= D, ldh >= Hd, ldf >= D)");
  hipLaunchKernelGGL(insert_rows_kernel, dim3(n_dst, S + 1), dim3(128), 0, ST(stream), (const insert_dst_t*)dst_table, slot, S,
                     ldo, ldh, D, Hd, T, feat, ldf, action, logp, value, rm, cmd);
  return (int)hipGetLastError();
}
