// frame_table.hip — storages that keep every distinct frame row once and their windows as frame ids.
//
//   cadre_gather_*_ft     the four minibatch gathers of cadre_kernels.hip with one more pointer per source: win == NULL is a
//                         materialised source (obs [T+1][S][ldo], row (t, s) at obs + (t*S + s)*ldo, as today), win != NULL a
//                         frame table (obs = frames [F][ldo], row (t, s) at frames + win[t*S + s]*ldo).  Placement, sort rank,
//                         pos / seg, h0 / c0 / scalars and the zero pad are the statements of the kernels they twin.
//   cadre_frames_scan     which window rows of a materialised storage are new frames (the slide and the reset fill are not)
//   cadre_frames_copy     the new rows into a frame table, every window row's global id into a window-index array
//
// Rows move 16 bytes per lane wherever pitches and bases allow it, else element by element.  Everything this file writes is
// written with plain vector stores.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

// One source of the multi gathers: the nine pointers of gather_src_t (cadre_kernels.hip), the window ids and the frame count.
struct gather_src_ft_t {
  const float* obs; const float* hn; const float* cn; const int64_t* action; const float* value_preds;
  const float* returns; const float* logp; const int32_t* command; const float* adv;
  const int32_t* win;          // NULL: obs is materialised
  int64_t n_frames;            // rows of the frame table (read only when win != NULL)
};

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// dst[0 .. ld) = src[0 .. D) | zeros by the whole workgroup.  src == NULL: NaN in columns < D (an id outside the table).
// vec: src, dst 16-byte aligned and ld a multiple of 4 (the caller checked; uniform over the workgroup).
__device__ __forceinline__ void ft_row(const float* src, float* dst, int ld, int D, bool vec) {
  const float nan = __builtin_nanf("");
  if (vec) {
    const int n4 = ld >> 2, full = D >> 2;          // float4 groups; groups that lie wholly below D
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int k = threadIdx.x; k < n4; k += blockDim.x) {
      float4 v;
      if (k < full) {
        v = src ? reinterpret_cast<const float4*>(src)[k] : make_float4(nan, nan, nan, nan);
      } else {
        float e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = 4 * k + q;
          e[q] = c < D ? (src ? src[c] : nan) : 0.f;
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
      }
      d4[k] = v;
    }
    return;
  }
  for (int c = threadIdx.x; c < ld; c += blockDim.x) dst[c] = c < D ? (src ? src[c] : nan) : 0.f;
}

// The source row of window row (t, s): NULL for a frame id outside [0, n_frames).
__device__ __forceinline__ const float* ft_src(const float* obs, const int32_t* win, int64_t n_frames, int64_t t, int S, int s,
                                               int64_t ldo) {
  if (!win) return obs + (t * S + s) * ldo;
  const int64_t f = win[t * S + s];
  return (f >= 0 && f < n_frames) ? obs + f * ldo : nullptr;
}

__device__ __forceinline__ bool ft_vec(const float* obs, int64_t ldo, const float* X, int64_t ldx) {
  return !(ldo & 3) && !(ldx & 3) && al16(obs) && al16(X);
}

// ---------------------------------------------------------------------------- gather_obs_kernel + win
__global__ __launch_bounds__(128) void gather_obs_ft_kernel(const float* obs, const int32_t* win, int64_t n_frames, int64_t ldo,
                                                            int S, const int64_t* idx, int B, float* x, int64_t ldx, int D) {
  const int b = blockIdx.x, s = blockIdx.y;
  const float* src = ft_src(obs, win, n_frames, idx[b], S, s, ldo);
  ft_row(src, x + ((int64_t)s * B + b) * ldx, (int)ldx, D, ft_vec(obs, ldo, x, ldx));
}

// ---------------------------------------------------------------------------- gather_minibatch_kernel + win
__global__ __launch_bounds__(128) void gather_minibatch_ft_kernel(
    const float* obs, const int32_t* win, int64_t n_frames, int64_t ldo, int S, const float* hn, const float* cn, int64_t ldh,
    const int64_t* action, const float* value_preds, const float* returns, const float* logp, const int32_t* command,
    const float* adv, const int64_t* idx, int B, int D, int Hd, int Bt, int b0, float* X, int64_t ldx, float* h0, float* c0,
    int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o, float* returns_o, float* old_logp_o, float* adv_o) {
  const int b = blockIdx.x, s = blockIdx.y;
  const int64_t t = idx[b];
  const int ob = b0 + b;
  if (s < S) {
    ft_row(ft_src(obs, win, n_frames, t, S, s, ldo), X + ((int64_t)s * Bt + ob) * ldx, (int)ldx, D, ft_vec(obs, ldo, X, ldx));
    return;
  }
  const float* hs = hn + t * ldh;
  const float* cs = cn + t * ldh;
  for (int d = threadIdx.x; d < ldho; d += blockDim.x) {
    h0[(int64_t)ob * ldho + d] = d < Hd ? hs[d] : 0.f;
    c0[(int64_t)ob * ldho + d] = d < Hd ? cs[d] : 0.f;
  }
  if (threadIdx.x == 0) {
    actions_o[ob] = action[t];
    commands_o[ob] = command[t];
    old_values_o[ob] = value_preds[t];
    returns_o[ob] = returns[t];
    old_logp_o[ob] = logp[t];
    adv_o[ob] = adv[t];
  }
}

// ---------------------------------------------------------------------------- gather_minibatch_multi_kernel + win
__global__ __launch_bounds__(128) void gather_minibatch_multi_ft_kernel(
    const gather_src_ft_t* src, int64_t ldo, int S, int64_t ldh, const int64_t* idx, int Bw, int D, int Hd, int Bt, float* X,
    int64_t x_hs, int64_t ldx, float* h0, float* c0, int64_t h_hs, int64_t ldho, int64_t* actions_o, int32_t* commands_o,
    float* old_values_o, float* returns_o, float* old_logp_o, float* adv_o) {
  const int b = blockIdx.x, s = blockIdx.y, zi = blockIdx.z;
  const int wi = zi >> 1, hd = zi & 1;
  const gather_src_ft_t g = src[zi];
  const int64_t t = idx[(int64_t)zi * Bw + b];
  const int ob = wi * Bw + b;
  if (s < S) {
    float* Xh = X + hd * x_hs;
    ft_row(ft_src(g.obs, g.win, g.n_frames, t, S, s, ldo), Xh + ((int64_t)s * Bt + ob) * ldx, (int)ldx, D,
           ft_vec(g.obs, ldo, Xh, ldx));
    return;
  }
  const float* hs = g.hn + t * ldh;
  const float* cs = g.cn + t * ldh;
  for (int d = threadIdx.x; d < ldho; d += blockDim.x) {
    h0[hd * h_hs + (int64_t)ob * ldho + d] = d < Hd ? hs[d] : 0.f;
    c0[hd * h_hs + (int64_t)ob * ldho + d] = d < Hd ? cs[d] : 0.f;
  }
  if (threadIdx.x == 0) {
    const int64_t o = (int64_t)hd * Bt + ob;
    actions_o[o] = g.action[t];
    commands_o[o] = g.command[t];
    old_values_o[o] = g.value_preds[t];
    returns_o[o] = g.returns[t];
    old_logp_o[o] = g.logp[t];
    adv_o[o] = g.adv[t];
  }
}

// ---------------------------------------------------------------------------- gather_sorted_multi_kernel + win
// (the rank of a row: rows with a smaller command + earlier rows with the same command, re-derived by every workgroup)
__global__ __launch_bounds__(128) void gather_sorted_multi_ft_kernel(
    const gather_src_ft_t* src, int64_t ldo, int S, int64_t ldh, const int64_t* idx, int Bw, int D, int Hd, int Bt, int C, float* X,
    int64_t x_hs, int64_t ldx, float* h0, float* c0, int64_t h_hs, int64_t ldho, int64_t* actions_o, int32_t* commands_o,
    float* old_values_o, float* returns_o, float* old_logp_o, float* adv_o, int32_t* pos, int32_t* seg) {
  extern __shared__ int32_t gs_cmd[];                      // [Bt] commands of this head, then 2 counters
  const int b = blockIdx.x, s = blockIdx.y, zi = blockIdx.z;
  const int wi = zi >> 1, hd = zi & 1;
  for (int r = threadIdx.x; r < Bt; r += blockDim.x) {
    const int w2 = r / Bw, b2 = r - w2 * Bw;
    const int z2 = 2 * w2 + hd;
    gs_cmd[r] = src[z2].command[idx[(int64_t)z2 * Bw + b2]];
  }
  int32_t* cnt = gs_cmd + Bt;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int ob = wi * Bw + b;
  const int cme = gs_cmd[ob];
  int below = 0, before = 0;
  for (int r = threadIdx.x; r < Bt; r += blockDim.x) {
    const int c = gs_cmd[r];
    below += c < cme;
    before += (c == cme) & (r < ob);
  }
  atomicAdd(&cnt[0], below);                               // (integer sums: any order gives the same value)
  atomicAdd(&cnt[1], before);
  __syncthreads();
  const int d = cnt[0] + cnt[1];
  const gather_src_ft_t g = src[zi];
  const int64_t t = idx[(int64_t)zi * Bw + b];
  if (s < S) {
    float* Xh = X + hd * x_hs;
    ft_row(ft_src(g.obs, g.win, g.n_frames, t, S, s, ldo), Xh + ((int64_t)s * Bt + d) * ldx, (int)ldx, D,
           ft_vec(g.obs, ldo, Xh, ldx));
    return;
  }
  const float* hs = g.hn + t * ldh;
  const float* cs = g.cn + t * ldh;
  for (int k = threadIdx.x; k < ldho; k += blockDim.x) {
    h0[hd * h_hs + (int64_t)d * ldho + k] = k < Hd ? hs[k] : 0.f;
    c0[hd * h_hs + (int64_t)d * ldho + k] = k < Hd ? cs[k] : 0.f;
  }
  if (threadIdx.x == 0) {
    const int64_t o = (int64_t)hd * Bt + d;
    actions_o[o] = g.action[t];
    commands_o[o] = cme;
    old_values_o[o] = g.value_preds[t];
    returns_o[o] = g.returns[t];
    old_logp_o[o] = g.logp[t];
    adv_o[o] = g.adv[t];
    pos[hd * Bt + ob] = d;
  }
  if (b == 0 && wi == 0 && (int)threadIdx.x < C) {         // the head's run table
    int off = 0, n = 0;
    for (int r = 0; r < Bt; ++r) { off += gs_cmd[r] < (int)threadIdx.x; n += gs_cmd[r] == (int)threadIdx.x; }
    seg[2 * (hd * C + threadIdx.x)] = off;
    seg[2 * (hd * C + threadIdx.x) + 1] = n;
  }
}

// ---------------------------------------------------------------------------- packing a materialised storage into frames
// Rows are compared as 32-bit patterns over columns 0 .. D-1: the pad does not count, -0.0 differs from +0.0, equal NaN
// bits are equal.  One wave per window row (t, s) of storage z.
__device__ __forceinline__ bool rows_equal(const float* a, const float* b, int D, int lane) {
  const uint32_t* ua = reinterpret_cast<const uint32_t*>(a);
  const uint32_t* ub = reinterpret_cast<const uint32_t*>(b);
  bool differ = false;
  if (!(((uintptr_t)a | (uintptr_t)b) & 15)) {
    const int full = D >> 2;
    for (int k = lane; k < full; k += 64) {
      const uint4 x = reinterpret_cast<const uint4*>(ua)[k], y = reinterpret_cast<const uint4*>(ub)[k];
      differ |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
    }
    for (int c = 4 * full + lane; c < D; c += 64) differ |= ua[c] != ub[c];
  } else {
    for (int c = lane; c < D; c += 64) differ |= ua[c] != ub[c];
  }
  return !__any(differ);
}

// flags[z][t][s]: 0 a new frame, 1 the slide (the id of row (t-1, s+1)), 2 the reset fill (the id of row (t, s-1))
__global__ __launch_bounds__(64) void frames_flags_kernel(const float* const* src, int P, int S, int64_t ldo, int D,
                                                          int32_t* flags) {
  const int r = blockIdx.x, z = blockIdx.y, lane = threadIdx.x;
  const int t = r / S, s = r - t * S;
  const float* obs = src[z];
  const float* me = obs + (int64_t)r * ldo;
  int f = 0;
  if (t > 0 && s < S - 1 && rows_equal(me, obs + ((int64_t)(t - 1) * S + s + 1) * ldo, D, lane)) f = 1;
  else if (s > 0 && rows_equal(me, me - ldo, D, lane)) f = 2;
  if (lane == 0) flags[((int64_t)z * P + t) * S + s] = f;
}

// The ids: serial in t, one wave per storage (lane s holds row (t, s); S <= 16).
__global__ __launch_bounds__(64) void frames_ids_kernel(const int32_t* flags, int P, int S, int32_t* win_local, int32_t* count) {
  const int z = blockIdx.x, lane = threadIdx.x;
  const int32_t* fl = flags + (int64_t)z * P * S;
  int32_t* wl = win_local + (int64_t)z * P * S;
  int n_new = 0, prev = 0;                                 // prev: the id of row (t-1, lane)
  for (int t = 0; t < P; ++t) {
    const int f = lane < S ? fl[(int64_t)t * S + lane] : 0;
    const bool is_new = lane < S && f == 0;
    const unsigned long long m = __ballot(is_new);
    const int from_prev = __shfl(prev, (lane + 1) & 63, 64);
    int id = is_new ? n_new + __popcll(m & ((1ull << lane) - 1ull)) : from_prev;
    int done = f != 2;
    for (int k = 1; k < S; ++k) {                          // a fill takes the id to its left, which may be a fill itself
      const int left = __shfl(id, (lane + 63) & 63, 64), ldone = __shfl(done, (lane + 63) & 63, 64);
      if (!done && ldone) { id = left; done = 1; }
    }
    if (lane < S) wl[(int64_t)t * S + lane] = id;
    n_new += __popcll(m);
    prev = id;
  }
  if (lane == 0) count[z] = n_new;
}

__global__ __launch_bounds__(128) void frames_copy_kernel(const float* const* src, int P, int S, int64_t ldo, int D,
                                                          const int32_t* flags, const int32_t* win_local, const int32_t* base,
                                                          float* frames, int64_t ld, int64_t F_cap, int32_t* win_dst,
                                                          const int32_t* row0) {
  const int r = blockIdx.x, z = blockIdx.y;
  const int64_t o = (int64_t)z * P * S + r;
  const int64_t gid = (int64_t)base[z] + win_local[o];
  if (threadIdx.x == 0) win_dst[(int64_t)row0[z] * S + r] = (int32_t)gid;
  if (flags[o] != 0 || gid < 0 || gid >= F_cap) return;    // (a row past the capacity is not written: the host sized it)
  const float* sp = src[z] + (int64_t)r * ldo;
  float* dp = frames + gid * ld;
  ft_row(sp, dp, (int)ld, D, !(ldo & 3) && !(ld & 3) && al16(src[z]) && al16(frames));
}

}  // namespace

extern "C" int cadre_gather_obs_ft(const float* obs, const int32_t* win, int64_t n_frames, int64_t ldo, int32_t S,
                                   const int64_t* idx, int32_t B, float* x, int64_t ldx, int32_t D, void* stream) {
  FAIL_IF(!obs || !idx || !x || S < 1 || B < 1 || D < 1 || ldx < D || ldo < D || ldx > INT_MAX || (win && n_frames < 1),
          "cadre_gather_obs_ft: bad argument");
  hipLaunchKernelGGL(gather_obs_ft_kernel, dim3(B, S), dim3(128), 0, ST(stream), obs, win, n_frames, ldo, S, idx, B, x, ldx, D);
  return (int)hipGetLastError();
}

extern "C" int cadre_gather_minibatch_ft(const float* obs, const int32_t* win, int64_t n_frames, int64_t ldo, int32_t S,
                                         const float* hn, const float* cn, int64_t ldh, const int64_t* action,
                                         const float* value_preds, const float* returns, const float* logp,
                                         const int32_t* command, const float* adv, const int64_t* idx, int32_t B, int32_t D,
                                         int32_t Hd, int32_t Bt, int32_t b0, float* X, int64_t ldx, float* h0, float* c0,
                                         int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                                         float* returns_o, float* old_logp_o, float* adv_o, void* stream) {
  FAIL_IF(!obs || !hn || !cn || !action || !value_preds || !returns || !logp || !command || !adv || !idx || !X ||
              !h0 || !c0 || !actions_o || !commands_o || !old_values_o || !returns_o || !old_logp_o || !adv_o ||
              S < 1 || B < 1 || D < 1 || Hd < 1 || b0 < 0 || b0 + B > Bt || ldx < D || ldo < D || ldx > INT_MAX || ldho < Hd ||
              (win && n_frames < 1),
          "cadre_gather_minibatch_ft: bad argument");
  hipLaunchKernelGGL(gather_minibatch_ft_kernel, dim3(B, S + 1), dim3(128), 0, ST(stream), obs, win, n_frames, ldo, S, hn, cn,
                     ldh, action, value_preds, returns, logp, command, adv, idx, B, D, Hd, Bt, b0, X, ldx, h0, c0, ldho,
                     actions_o, commands_o, old_values_o, returns_o, old_logp_o, adv_o);
  return (int)hipGetLastError();
}

extern "C" int cadre_gather_minibatch_multi_ft(const void* src_table, int32_t n_src, int64_t ldo, int32_t S, int64_t ldh,
                                               const int64_t* idx, int32_t Bw, int32_t D, int32_t Hd, int32_t Bt, float* X,
                                               int64_t x_head_stride, int64_t ldx, float* h0, float* c0,
                                               int64_t h_head_stride, int64_t ldho, int64_t* actions_o, int32_t* commands_o,
                                               float* old_values_o, float* returns_o, float* old_logp_o, float* adv_o,
                                               void* stream) {
  FAIL_IF(!src_table || !idx || !X || !h0 || !c0 || !actions_o || !commands_o || !old_values_o || !returns_o || !old_logp_o ||
              !adv_o || n_src < 2 || (n_src & 1) || S < 1 || Bw < 1 || D < 1 || Hd < 1 || (n_src / 2) * Bw > Bt || ldx < D ||
              ldo < D || ldx > INT_MAX || ldho < Hd,
          "cadre_gather_minibatch_multi_ft: bad argument");
  // (a head stride off 16 bytes only switches head 1 to the element-wise copy: the kernel looks at the head's own base)
  hipLaunchKernelGGL(gather_minibatch_multi_ft_kernel, dim3(Bw, S + 1, n_src), dim3(128), 0, ST(stream),
                     (const gather_src_ft_t*)src_table, ldo, S, ldh, idx, Bw, D, Hd, Bt, X, x_head_stride, ldx, h0, c0,
                     h_head_stride, ldho, actions_o, commands_o, old_values_o, returns_o, old_logp_o, adv_o);
  return (int)hipGetLastError();
}

extern "C" int cadre_gather_sorted_multi_ft(const void* src_table, int32_t n_src, int64_t ldo, int32_t S, int64_t ldh,
                                            const int64_t* idx, int32_t Bw, int32_t D, int32_t Hd, int32_t Bt, int32_t C, float* X,
                                            int64_t x_head_stride, int64_t ldx, float* h0, float* c0, int64_t h_head_stride,
                                            int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                                            float* returns_o, float* old_logp_o, float* adv_o, int32_t* pos, int32_t* seg,
                                            void* stream) {
  FAIL_IF(!src_table || !idx || !X || !h0 || !c0 || !actions_o || !commands_o || !old_values_o || !returns_o || !old_logp_o ||
              !adv_o || !pos || !seg || n_src < 2 || (n_src & 1) || S < 1 || Bw < 1 || D < 1 || Hd < 1 || (n_src / 2) * Bw != Bt ||
              Bt > 8192 || C < 1 || C > 16 || ldx < D || ldo < D || ldx > INT_MAX || ldho < Hd,
          "cadre_gather_sorted_multi_ft: bad argument (every row of the minibatch comes from the table: (n_src / 2) * Bw == Bt)");
  hipLaunchKernelGGL(gather_sorted_multi_ft_kernel, dim3(Bw, S + 1, n_src), dim3(128), (Bt + 2) * sizeof(int32_t), ST(stream),
                     (const gather_src_ft_t*)src_table, ldo, S, ldh, idx, Bw, D, Hd, Bt, C, X, x_head_stride, ldx, h0, c0,
                     h_head_stride, ldho, actions_o, commands_o, old_values_o, returns_o, old_logp_o, adv_o, pos, seg);
  return (int)hipGetLastError();
}

extern "C" int cadre_frames_scan(const void* src_table, int32_t n, int32_t P, int32_t S, int64_t ldo, int32_t D, int32_t* flags,
                                 int32_t* win_local, int32_t* count, void* stream) {
  FAIL_IF(!src_table || !flags || !win_local || !count || n < 1 || n > 65535 || P < 1 || S < 1 || S > 16 || D < 1 || ldo < D ||
              (int64_t)P * S > INT_MAX,
          "cadre_frames_scan: bad argument (1 <= S <= 16, n <= 65535, P * S below 2^31, ldo >= D)");
  hipLaunchKernelGGL(frames_flags_kernel, dim3(P * S, n), dim3(64), 0, ST(stream), (const float* const*)src_table, P, S, ldo, D,
                     flags);
  hipLaunchKernelGGL(frames_ids_kernel, dim3(n), dim3(64), 0, ST(stream), flags, P, S, win_local, count);
  return (int)hipGetLastError();
}

extern "C" int cadre_frames_copy(const void* src_table, int32_t n, int32_t P, int32_t S, int64_t ldo, int32_t D,
                                 const int32_t* flags, const int32_t* win_local, const int32_t* base, float* frames, int64_t ld,
                                 int64_t F_cap, int32_t* win_dst, const int32_t* row0, void* stream) {
  FAIL_IF(!src_table || !flags || !win_local || !base || !frames || !win_dst || !row0 || n < 1 || n > 65535 || P < 1 || S < 1 ||
              S > 16 || D < 1 || ldo < D || ld < D || ld > INT_MAX || F_cap < 1 || (int64_t)P * S > INT_MAX,
          "cadre_frames_copy: bad argument (1 <= S <= 16, n <= 65535, P * S below 2^31, ldo >= D, ld >= D, F_cap >= 1)");
  hipLaunchKernelGGL(frames_copy_kernel, dim3(P * S, n), dim3(128), 0, ST(stream), (const float* const*)src_table, P, S, ldo, D,
                     flags, win_local, base, frames, ld, F_cap, win_dst, row0);
  return (int)hipGetLastError();
}
