// ordinal.h — the ordinal policy head (Tang & Agrawal, "Discretizing Continuous Action Space for On-Policy Optimization";
// the commented-out block of the reference's ppo_agent/distributions.py:45-79) as wave-level device functions, shared by
// the loss kernel (cadre_kernels.hip) and the sampling kernels (cadre_kernels.hip, act_batch.hip).  One wave per row.
//
// Lane j of the raw tower output x is threshold unit j in RANK space (rank[k] = position of bin k in ascending order of
// its control value).  With eps = 1e-8:
//   s_j = sigmoid(x_j)   t_j = sigmoid(-x_j)   u_j = log(s_j + eps)   w_j = log(t_j + eps)
//   z_r = sum_{j <= r} u_j + sum_{j > r} w_j            logit of bin k = z_{rank[k]}
// and, with G_r = d total / d z_r,
//   d total / d x_j = s_j t_j / (s_j + eps) * sum_{r >= j} G_r  -  s_j t_j / (t_j + eps) * sum_{r < j} G_r.
// The running sums are shuffle ladders with one fixed combination order: the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define CADRE_ORD_EPS 1e-8f

// inclusive prefix sum over lanes 0 .. lane
__device__ __forceinline__ float ord_scan_up(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// inclusive suffix sum over lanes lane .. 63
__device__ __forceinline__ float ord_scan_down(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_down(v, o, 64);
    if (lane + o < 64) v += t;
  }
  return v;
}

// Lane = bin.  rk: rank of this lane's bin (lanes >= K: the lane itself, so that rk is a permutation of 0 .. 63).
// Returns the lane r with bin[r], i.e. the inverse permutation (a push: lane k writes its index to lane rk).
__device__ __forceinline__ int ord_inverse(int rk, int lane) {
  return __builtin_amdgcn_ds_permute(rk << 2, lane);
}

// x: raw output of threshold unit `lane` (anything on lanes >= K), on = lane < K.  Returns the unnormalised logit of bin
// `lane` (-inf on lanes >= K); s, t: the two sigmoids of this lane's threshold unit, for ord_backward.
__device__ __forceinline__ float ord_logits(float x, bool on, int rk, int lane, float& s, float& t) {
  x = on ? x : 0.f;
  s = 1.f / (1.f + expf(-x));
  t = 1.f / (1.f + expf(x));                       // sigmoid(-x): 1 - s has no relative accuracy left for x >~ 8
  const float u = on ? logf(s + CADRE_ORD_EPS) : 0.f;
  const float w = on ? logf(t + CADRE_ORD_EPS) : 0.f;
  const float wn = __shfl_down(w, 1, 64);          // exclusive suffix of w = inclusive suffix of w shifted by one lane
  const float z = ord_scan_up(u, lane) + ord_scan_down(lane < 63 ? wn : 0.f, lane);
  const float lg = __shfl(z, rk, 64);
  return on ? lg : -INFINITY;
}

// g: d total / d (logit of bin `lane`), 0 on lanes >= K; binv = ord_inverse(rk).  Returns d total / d x_lane.
__device__ __forceinline__ float ord_backward(float g, bool on, float s, float t, int binv, int lane) {
  const float G = __shfl(g, binv, 64);
  const float pre = __shfl_up(ord_scan_up(G, lane), 1, 64);     // sum_{r < lane} G_r (lane 0: masked below)
  const float suf = ord_scan_down(G, lane);                      // sum_{r >= lane} G_r
  const float st = s * t;
  const float a = st / (s + CADRE_ORD_EPS), b = st / (t + CADRE_ORD_EPS);
  return on ? a * suf - b * (lane > 0 ? pre : 0.f) : 0.f;
}
