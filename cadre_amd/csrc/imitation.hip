// imitation.hip — behaviour cloning from recorded episodes: the imitation loss of the update's hot path and the kernel
// that lays a demonstration set's observation rows out.
//
//   cadre_bc_loss     forward + backward of  value_coeff 0.5 mean(w (v - R)^2) + bc_coeff mean(w CE(t, p)) - ent_coeff mean(w H)
//                     where ppo_loss_* (cadre_kernels.hip) stands in the update: same addressing, grid, scratch protocol,
//                     poison and rank table, so everything behind the loss launch (MLP / LSTM backward, clip + Adam) is
//                     indifferent to which of the two ran
//   cadre_demo_rows   obs[t][s] = latent[window[t][s]] | measurements x 6 | zeros, for a whole demonstration set at once
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

#define BC_NSTAT CADRE_BC_STATS_FIELDS
struct bc_stats_t {
  float* row;           // [2 heads][F] stats row of this step (NULL: no statistics)
  int32_t F;
  float* part;          // [2 * nblk][BC_NSTAT] per-workgroup partials
};

// One wave per row (lane = bin), 16 rows per workgroup, B/16 x 2 workgroups: the layout of ppo_loss_body, and up to the
// normalised logits lg, the probabilities pk and the entropy H the same statements.  A row counts for head hd when its
// command is in range AND its action is a bin of the head; every other row gets exact zeros in all C nets of the head
// and adds nothing to any sum.  GRAD = false is the evaluation form: no gradient is stored.
template <bool GRAD>
__global__ __launch_bounds__(256) void bc_loss_kernel(const float* logits, int64_t ldl, int64_t l_ns, const float* values,
                                                      int64_t ldv, int64_t v_ns, const int64_t* actions,
                                                      const int32_t* commands, const float* returns, const float* weights,
                                                      int B, int C, int n_steer, int n_throttle, float eps, float bc_coeff,
                                                      float value_coeff, float ent_coeff, float inv_b, float* losses,
                                                      float* dlogits, float* dvalues, float* scratch, const int32_t* poison,
                                                      bc_stats_t so, const int32_t* ord) {
  const int hd = blockIdx.y;                       // 0 steer, 1 throttle
  const int K = hd == 0 ? n_steer : n_throttle;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool stats = so.row != nullptr;
  __shared__ float red[3 + BC_NSTAT][4];
  float s_val = 0.f, s_ce = 0.f, s_ent = 0.f;      // lane 0 of each wave
  float s_st[BC_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool ordinal = ord != nullptr && ord[hd * 64] >= 0;
  int rk = lane, binv = lane;
  if (ordinal) {
    rk = lane < K ? ord[hd * 64 + lane] : lane;
    binv = ord_inverse(rk, lane);
  }
  const float t_off = eps / (float)K, t_on = (1.f - eps) + t_off;     // the smoothed target: off / on the demonstrated bin
  for (int i = 0; i < 4; ++i) {
    const int b = blockIdx.x * 16 + wave * 4 + i;
    if (b >= B) break;
    const int row = hd * B + b;                    // per-head sample arrays are [2][B]
    const int c = commands[row];
    const int64_t a64 = actions[row];
    const bool own_ok = c >= 0 && c < C && a64 >= 0 && a64 < K;       // (-1: no label for this head)
    if constexpr (GRAD) {
      for (int cc = 0; cc < C; ++cc) {
        if (own_ok && cc == c) continue;
        if (lane < ldl) dlogits[(int64_t)(hd * C + cc) * l_ns + (int64_t)b * ldl + lane] = 0.f;
        if (lane == 0) dvalues[(int64_t)(hd * C + cc) * v_ns + (int64_t)b * ldv] = 0.f;
      }
    }
    if (!own_ok) continue;
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
    const float lp = __shfl(lg, a, 64);            // a < K: a valid bin's lane
    const float tk = on ? (lane == a ? t_on : t_off) : 0.f;
    const float ce = -wave_sum(tk != 0.f ? tk * lg : 0.f);
    const float v = values[(int64_t)net * v_ns + (int64_t)b * ldv];
    const float R = returns[row];
    const float w = weights ? weights[row] : 1.f;
    const float dv = v - R;
    s_val += w * (dv * dv);
    s_ce += w * ce;
    s_ent += w * H;
    if (stats) {
      // top-1: the lowest index among the largest probabilities
      const float pm = wave_max(on ? pk : -1.f);
      const unsigned long long hit = __ballot(on && pk == pm);
      const int top = hit ? __ffsll((long long)hit) - 1 : -1;
      s_st[0] += top == a ? 1.f : 0.f;
      s_st[1] += -lp;
      s_st[2] += H;
      s_st[3] += fabsf(dv);
      s_st[4] += w;
      s_st[5] += 1.f;
    }
    if constexpr (GRAD) {
      const float wb = w * inv_b;
      if (lane == 0) dvalues[(int64_t)net * v_ns + (int64_t)b * ldv] = value_coeff * wb * dv;
      // d total / d logit_k = w inv_b (bc (p_k - t_k) + ec p_k (lg_k + H))   (sum_k t_k = 1; dH / d logit_k = -p_k (lg_k + H))
      float gk = on ? wb * (bc_coeff * (pk - tk) + ent_coeff * (pk * (lg + H))) : 0.f;
      if (ordinal) gk = ord_backward(gk, on, sg, tg, binv, lane);
      if (lane < ldl) dlogits[(int64_t)net * l_ns + (int64_t)b * ldl + lane] = gk;
    }
  }
  if (lane == 0) {
    red[0][wave] = s_val; red[1][wave] = s_ce; red[2][wave] = s_ent;
#pragma unroll
    for (int k = 0; k < BC_NSTAT; ++k) red[3 + k][wave] = s_st[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nblk = gridDim.x, me = hd * nblk + blockIdx.x, total = 2 * nblk;
    float* part = scratch + 4;                      // [total][3]; scratch[0] is the arrival counter (zero on entry, reset below)
    for (int k = 0; k < 3; ++k)
      __hip_atomic_store(part + 3 * me + k, (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    if (stats) {
      for (int k = 0; k < BC_NSTAT; ++k) {
        const float* r = red[3 + k];
        __hip_atomic_store(so.part + BC_NSTAT * me + k, (r[0] + r[1]) + (r[2] + r[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(scratch), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (unsigned)(total - 1)) {          // last arriver: every partial has been published
      float sv = 0.f, sc = 0.f, sn = 0.f;
      for (int w = 0; w < total; ++w) {             // workgroup order: equal inputs give equal bits
        sv += __hip_atomic_load(part + 3 * w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sc += __hip_atomic_load(part + 3 * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sn += __hip_atomic_load(part + 3 * w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const float bad = (poison && __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? __builtin_nanf("") : 0.f;
      losses[0] = value_coeff * 0.5f * sv * inv_b + bad;
      losses[1] = bc_coeff * sc * inv_b + bad;
      losses[2] = ent_coeff * sn * inv_b + bad;
      if (stats) {
        for (int h = 0; h < 2; ++h) {
          float t[BC_NSTAT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int w = h * nblk; w < (h + 1) * nblk; ++w)
            for (int k = 0; k < BC_NSTAT; ++k)
              t[k] += __hip_atomic_load(so.part + BC_NSTAT * w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          float* o = so.row + h * so.F;
          for (int k = 0; k < BC_NSTAT; ++k) o[k] = t[k] * inv_b;
        }
      }
      __hip_atomic_store(reinterpret_cast<unsigned*>(scratch), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// One workgroup of 128 lanes per observation row, 16 bytes per lane: lane i copies floats 4 i .. 4 i + 3 of the frame's
// latent, lanes 0 .. (ldo - 512) / 4 - 1 then write the tail — the three measurements six times (columns 512 .. 529, the
// statement of append_meas_kernel) and zeros up to the pitch.  A window index outside the table reads nothing and gives
// NaN in columns 0 .. 529 (the pad stays zero).
__global__ __launch_bounds__(128) void demo_rows_kernel(const float* latent, int64_t ld_lat, int n_frames,
                                                        const int32_t* window, const double* meas, float* obs, int64_t ldo) {
  const int64_t r = blockIdx.x;                    // t * S + s
  const int f = window[r];
  const bool ok = f >= 0 && f < n_frames;
  const int i = threadIdx.x;
  const float nan = __builtin_nanf("");
  float4* dst = reinterpret_cast<float4*>(obs + r * ldo);
  float4 v = make_float4(nan, nan, nan, nan);
  if (ok) v = reinterpret_cast<const float4*>(latent + (int64_t)f * ld_lat)[i];
  dst[i] = v;
  const int n_tail = (int)((ldo - 512) >> 2);      // <= 128 (the entry point checked)
  if (i < n_tail) {
    float m[3] = {nan, nan, nan};
    if (ok) {
      m[0] = (float)meas[(int64_t)f * 3 + 0]; m[1] = (float)meas[(int64_t)f * 3 + 1]; m[2] = (float)meas[(int64_t)f * 3 + 2];
    }
    float e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * i + q;                     // column 512 + j
      e[q] = j < 18 ? m[j % 3] : 0.f;
    }
    dst[128 + i] = make_float4(e[0], e[1], e[2], e[3]);
  }
}

}  // namespace

extern "C" int cadre_bc_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                             const int64_t* actions, const int32_t* commands, const float* returns, const float* weights,
                             int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, float label_smoothing,
                             float bc_coeff, float value_coeff, float ent_coeff, float inv_b, float* losses, float* dlogits,
                             float* dvalues, float* scratch, const int32_t* poison, float* stats_row, int32_t F,
                             float* stats_scratch, const int32_t* ord, void* stream) {
  FAIL_IF(!logits || !values || !actions || !commands || !returns || !losses || !scratch || B < 1 || C < 1 ||
              n_out_steer < 1 || n_out_steer > MAX_NOUT || n_out_throttle < 1 || n_out_throttle > MAX_NOUT ||
              ldl < n_out_steer || ldl < n_out_throttle || ldl > 64,
          "cadre_bc_loss: bad argument");
  FAIL_IF(!(label_smoothing >= 0.f && label_smoothing < 1.f), "cadre_bc_loss: label_smoothing must be in [0, 1)");
  FAIL_IF((dlogits == nullptr) != (dvalues == nullptr),
          "cadre_bc_loss: dlogits and dvalues go together (both NULL is the evaluation form)");
  FAIL_IF(stats_row && (F < CADRE_BC_STATS_FIELDS || !stats_scratch),
          "cadre_bc_loss: bad stats argument (F >= CADRE_BC_STATS_FIELDS and a stats scratch)");
  const bc_stats_t so{stats_row, F, stats_scratch};
  const dim3 grid((B + 15) / 16, 2), block(256);
  // scratch[0] (arrival counter) must be zero on entry, as for cadre_ppo_loss: the last arriver resets it
  if (dlogits)
    hipLaunchKernelGGL(bc_loss_kernel<true>, grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, commands,
                       returns, weights, B, C, n_out_steer, n_out_throttle, label_smoothing, bc_coeff, value_coeff, ent_coeff,
                       inv_b, losses, dlogits, dvalues, scratch, poison, so, ord);
  else
    hipLaunchKernelGGL(bc_loss_kernel<false>, grid, block, 0, ST(stream), logits, ldl, l_ns, values, ldv, v_ns, actions, commands,
                       returns, weights, B, C, n_out_steer, n_out_throttle, label_smoothing, bc_coeff, value_coeff, ent_coeff,
                       inv_b, losses, dlogits, dvalues, scratch, poison, so, ord);
  return (int)hipGetLastError();
}

extern "C" int cadre_demo_rows(const float* latent, int64_t ld_lat, int32_t n_frames, const int32_t* window,
                               const double* meas, int32_t T, int32_t S, float* obs, int64_t ldo, void* stream) {
  FAIL_IF(!latent || !window || !meas || !obs || n_frames < 1 || T < 1 || S < 1 || (int64_t)T * S > INT_MAX,
          "cadre_demo_rows: bad argument");
  FAIL_IF(ld_lat < 512 || (ld_lat & 3) || ldo < 532 || (ldo & 3) || ldo > 1024 || ((uintptr_t)latent & 15) || ((uintptr_t)obs & 15),
          "cadre_demo_rows: rows move 16 bytes per lane (latent pitch >= 512, 532 <= obs pitch <= 1024, both multiples of 4 "
          "floats, 16-byte aligned bases)");
  hipLaunchKernelGGL(demo_rows_kernel, dim3(T * S), dim3(128), 0, ST(stream), latent, ld_lat, n_frames, window, meas, obs, ldo);
  return (int)hipGetLastError();
}
