// curiosity.hip — random network distillation on the latent rows of the rollout storages (cadre_amd/curiosity.py): the running
// feature statistics (cadre_rnd_obs_stats), normalisation + both towers + the error in one launch (cadre_rnd_forward), the
// bonus scale and the mixed reward of every storage (cadre_rnd_reward) and the predictor's backward pass (cadre_rnd_backward).
//
// The dense products run on v_mfma_f32_32x32x2_f32 (exact fp32) through the tile product of tower.h.  Every sum has a fixed
// order and nothing is accumulated with atomics; everything is written with plain vector stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"
#include "tower.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

constexpr int MAX_DIM = 256;     // hidden / embed
constexpr int MAX_D = 1024;

struct rnd_row_t { const float* rewards; float* mixed; };

// ---------------------------------------------------------------------------- feature statistics
// Workgroup = 64 features x 16 row groups.  Group g sums rows g, g + 16, ...; the 16 partials are added in group order.  Two
// passes (mean, then squared deviations), then Chan's merge into the running statistics.  The count is advanced by the
// one-thread launch behind this one: every workgroup here reads the old count.
__global__ __launch_bounds__(1024) void obs_stats_kernel(const float* const* obs, int N, int T, int S, int64_t ldo, int D,
                                                         double* state) {
#pragma clang fp contract(off)
  __shared__ double part[16][64];
  const int fx = threadIdx.x, g = threadIdx.y, d = blockIdx.x * 64 + fx, R = N * T;
  const bool on = d < D;
  double s = 0.0;
  if (on)
    for (int r = g; r < R; r += 16) {
      const int w = r / T, t = r - w * T;
      s += (double)obs[w][((int64_t)t * S + (S - 1)) * ldo + d];
    }
  part[g][fx] = s;
  __syncthreads();
  double tot = 0.0;
  for (int i = 0; i < 16; ++i) tot += part[i][fx];
  const double mean = tot / (double)R;
  __syncthreads();
  double q = 0.0;
  if (on)
    for (int r = g; r < R; r += 16) {
      const int w = r / T, t = r - w * T;
      const double dv = (double)obs[w][((int64_t)t * S + (S - 1)) * ldo + d] - mean;
      q += dv * dv;
    }
  part[g][fx] = q;
  __syncthreads();
  if (g != 0 || !on) return;
  double qt = 0.0;
  for (int i = 0; i < 16; ++i) qt += part[i][fx];
  double* mu = state + CADRE_RND_HEAD, *m2 = mu + D;
  const double cnt = state[CADRE_RND_N], nb = (double)R, all = cnt + nb, delta = mean - mu[d];
  mu[d] = mu[d] + delta * nb / all;
  m2[d] = m2[d] + qt + delta * delta * cnt * nb / all;
}

__global__ void obs_count_kernel(double* state, int R) {
  if (threadIdx.x == 0 && blockIdx.x == 0) state[CADRE_RND_N] = state[CADRE_RND_N] + (double)R;
}

// ---------------------------------------------------------------------------- normalise, both towers, error
// One workgroup (4 waves) per 32 rows.  LDS (all dynamic): the rows' pointers, the feature chunk [32][PX] with its float mean /
// deviation [2][KC], h1 and h2 [32][H + 2], the two outputs [32][E + 2].  The towers run one after the other through the same
// statements (tw = 0 the target, 1 the predictor): equal weights give equal bits.
__global__ __launch_bounds__(256) void rnd_forward_kernel(const float* const* obs, int T, int S, int64_t ldo, int D, int H, int E,
                                                          int row0, int rows, const double* state, double eps_obs, float clip,
                                                          const float* target, const float* predictor, float* err, float* xh,
                                                          float* h1, float* h2, float* diff) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  const float** rowp = (const float**)sm;                // 32 row pointers in front of the float arrays
  const int PH = H + 2, PE = E + 2;
  float* xs = sm + 64, *mus = xs + 32 * PX, *sds = mus + KC, *h1s = sds + KC, *h2s = h1s + 32 * PH, *os0 = h2s + 32 * PH,
       *os1 = os0 + 32 * PE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.x * 32, valid = min(32, rows - i0);
  if (tid < 32) {
    const int r = row0 + i0 + min(tid, valid - 1), w = r / T, t = r - w * T;
    rowp[tid] = obs[w] + ((int64_t)t * S + (S - 1)) * ldo;
  }
  const double n = state[CADRE_RND_N];
  const double* mu = state + CADRE_RND_HEAD, *m2 = mu + D;
  for (int tw = 0; tw < 2; ++tw) {
    const float* P = tw ? predictor : target;
    const float* W1 = P, *b1 = W1 + (int64_t)D * H, *W2 = b1 + H, *b2 = W2 + (int64_t)H * H, *W3 = b2 + H, *b3 = W3 + (int64_t)H * E;
    float* sx = tw ? xh : nullptr, *s1 = tw ? h1 : nullptr, *s2 = tw ? h2 : nullptr;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    for (int k0 = 0; k0 < D; k0 += KC) {
      __syncthreads();                                   // the chunk before this one (and rowp) is no longer read / is written
      for (int k = tid; k < KC; k += 256) {
        const int d = k0 + k;
        float m = 0.f, sd = 1.f;
        if (d < D) {
          m = (float)mu[d];
          sd = (float)sqrt((n > 0.0 ? m2[d] / n : 1.0) + eps_obs);
        }
        mus[k] = m;
        sds[k] = sd;
      }
      __syncthreads();
      for (int idx = tid; idx < 32 * KC; idx += 256) {
        const int row = idx / KC, k = idx - row * KC, d = k0 + k;
        float v = 0.f;
        if (row < valid && d < D) {                      // the row tail and the k tail are zeros in LDS; nothing else is read
          v = ((rowp[row][d] - mus[k]) / sds[k]);
          v = fminf(fmaxf(v, -clip), clip);
          if (sx) sx[(int64_t)(i0 + row) * D + d] = v;
        }
        xs[row * PX + k] = v;
      }
      __syncthreads();
      const int klen = min(KC, D - k0);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ct = wave + 4 * t;
        if (ct < H / 32)
          for (int kk = 0; kk < klen; kk += 32)
            mfma32(acc[t], xs + (lane & 31) * PX + kk, W1 + (int64_t)(k0 + kk) * H + ct * 32 + (lane & 31), H, klen - kk, lane);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ct = wave + 4 * t;
      if (ct < H / 32) tile_out<true>(acc[t], b1, ct, h1s, PH, s1 ? s1 + (int64_t)i0 * H : nullptr, H, valid, lane);
    }
    __syncthreads();
    dense_lds<true>(h1s, PH, H, W2, b2, H, h2s, PH, s2 ? s2 + (int64_t)i0 * H : nullptr, valid, wave, lane);
    __syncthreads();
    dense_lds<false>(h2s, PH, H, W3, b3, E, tw ? os1 : os0, PE, nullptr, valid, wave, lane);
  }
  __syncthreads();
  if (tid < valid) {
    float s = 0.f;
    for (int k = 0; k < E; ++k) {
      const float dv = (os1[tid * PE + k] - os0[tid * PE + k]);
      s = (s + (dv * dv));
    }
    err[i0 + tid] = (s / (float)E);
  }
  if (diff)
    for (int idx = tid; idx < valid * E; idx += 256) {
      const int row = idx / E, k = idx - row * E;
      diff[(int64_t)(i0 + row) * E + k] = (os1[row * PE + k] - os0[row * PE + k]);
    }
}

// ---------------------------------------------------------------------------- bonus scale and mixed reward
__device__ __forceinline__ double block_sum_256(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// One workgroup.  Thread `tid` scans workers tid, tid + 256, ... twice (sum, then squared deviations from the mean: the scan
// costs less than keeping N T doubles); the partials meet in a fixed tree.
__global__ __launch_bounds__(256) void rnd_reward_kernel(const float* err, int N, int T, const rnd_row_t* rows, double* state,
                                                         int D, double gamma, double eps, int update) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  __shared__ double sig;
  const int tid = threadIdx.x;
  double* carry = state + CADRE_RND_HEAD + 2 * D;
  if (update) {
    double s = 0.0;
    for (int w = tid; w < N; w += 256) {
      double rho = carry[w];
      for (int t = 0; t < T; ++t) {
        rho = ((gamma * rho) + (double)err[(int64_t)w * T + t]);
        s += rho;
      }
    }
    const double nb = (double)N * (double)T, mean = block_sum_256(s, red, tid) / nb;
    double q = 0.0;
    for (int w = tid; w < N; w += 256) {
      double rho = carry[w];
      for (int t = 0; t < T; ++t) {
        rho = ((gamma * rho) + (double)err[(int64_t)w * T + t]);
        q += (rho - mean) * (rho - mean);
      }
      carry[w] = rho;
    }
    const double qt = block_sum_256(q, red, tid);
    if (tid == 0) {
      const double cnt = state[CADRE_RND_RHO_N], all = cnt + nb, delta = mean - state[CADRE_RND_RHO_MEAN];
      const double m2 = state[CADRE_RND_RHO_M2] + qt + delta * delta * cnt * nb / all;
      state[CADRE_RND_RHO_N] = all;
      state[CADRE_RND_RHO_MEAN] = state[CADRE_RND_RHO_MEAN] + delta * nb / all;
      state[CADRE_RND_RHO_M2] = m2;
      sig = sqrt(m2 / all + eps);
      state[CADRE_RND_SIGMA] = sig;
    }
  } else if (tid == 0) {
    sig = state[CADRE_RND_SIGMA];
  }
  __syncthreads();
  const float sigma = (float)sig, beta = (float)state[CADRE_RND_BETA], ext = (float)state[CADRE_RND_EXT];
  const int64_t total = (int64_t)2 * N * T;
  for (int64_t i = tid; i < total; i += 256) {
    const int k = (int)(i / T), t = (int)(i - (int64_t)k * T);
    const float ri = (err[(int64_t)(k >> 1) * T + t] / sigma);
    rows[k].mixed[t] = ((ext * rows[k].rewards[t]) + (beta * ri));
  }
}

// ---------------------------------------------------------------------------- predictor backward
__device__ __forceinline__ uint32_t mask_bits(uint64_t key, uint64_t ctr) {
  uint64_t z = key * 0x9E3779B97F4A7C15ull + ctr;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 40);
}

// One workgroup: the row mask, its count and the masked loss; the generator's counter then advances by `rows`.
__global__ __launch_bounds__(256) void rnd_mask_kernel(const float* err, int rows, double* state, int thresh, float* mask, float* cnt_out,
                                                       float* loss) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const uint64_t key = (uint64_t)state[CADRE_RND_KEY], ctr = (uint64_t)state[CADRE_RND_CTR];
  double c = 0.0, ls = 0.0;
  for (int i = tid; i < rows; i += 256) {
    const bool m = (int)mask_bits(key, ctr + (uint64_t)i) < thresh;
    mask[i] = m ? 1.f : 0.f;
    if (m) {
      c += 1.0;
      ls += (double)err[i];
    }
  }
  const double cnt = block_sum_256(c, red, tid);         // (whole numbers: exact in any order)
  const double tot = block_sum_256(ls, red, tid);
  if (tid == 0) {
    const double den = cnt > 1.0 ? cnt : 1.0;
    cnt_out[0] = (float)den;
    loss[0] = (float)(tot / den);
    loss[1] = (float)cnt;
    state[CADRE_RND_CTR] = (double)(ctr + (uint64_t)rows);
  }
}

// dX [rows][n_out] = (dY [rows][Kd] . W^T) where act > 0, W [n_out][Kd] (a layer's input-major matrix).  FROM_DIFF: dY is formed
// from the saved g - f (dO = 2 m diff / (E max(cnt, 1)), one rounding) and also stored to dO_out.  One workgroup per 32 rows.
template <bool FROM_DIFF>
__global__ __launch_bounds__(256) void rnd_dx_kernel(const float* src, int Kd, const float* W, const float* act, float* dX, int n_out,
                                                     int rows, const float* mask, const float* cnt, float* dO_out) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  const int PY = Kd + 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.x * 32, valid = min(32, rows - i0);
  const float den = FROM_DIFF ? ((float)Kd * cnt[0]) : 1.f;
  for (int idx = tid; idx < 32 * Kd; idx += 256) {
    const int row = idx / Kd, k = idx - row * Kd;
    float v = 0.f;
    if (row < valid) {
      v = src[(int64_t)(i0 + row) * Kd + k];
      if (FROM_DIFF) {
        v = mask[i0 + row] != 0.f ? ((2.f * v) / den) : 0.f;
        dO_out[(int64_t)(i0 + row) * Kd + k] = v;
      }
    }
    sm[row * PY + k] = v;
  }
  __syncthreads();
  for (int ct = wave; ct < n_out / 32; ct += 4) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int col = ct * 32 + (lane & 31);
    const float* Ar = sm + (lane & 31) * PY;
    const float* Bg = W + (int64_t)col * Kd;             // B[k][n] = W[n][k]: stride 1 in k
    for (int k0 = 0; k0 < Kd; k0 += 32) mfma32(acc, Ar + k0, Bg + k0, 1, 32, lane);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = acc_row(v, lane);
      if (row < valid) {
        const int64_t o = (int64_t)(i0 + row) * n_out + col;
        dX[o] = act[o] > 0.f ? acc[v] : 0.f;
      }
    }
  }
}

// dW [Kin][n_out] = X^T [Kin][rows] . dY [rows][n_out] and db = the column sums of dY.  One wave per 32 x 32 tile of dW walks
// all rows in order (A[i][r] = X[r][i], B[r][j] = dY[r][j], both straight from global memory: the lanes read consecutive
// floats); the tiles of blockIdx.y == n_it sum the bias columns, one lane per column, in row order.
__global__ __launch_bounds__(64) void rnd_dw_kernel(const float* X, const float* dY, int rows, int Kin, int n_out, float* dW, float* db) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, jt = blockIdx.x, it = blockIdx.y, h = lane >> 5;
  const int j = jt * 32 + (lane & 31);
  if (it == (Kin + 31) / 32) {
    if (lane < 32) {
      float s = 0.f;
      for (int r = 0; r < rows; ++r) s = (s + dY[(int64_t)r * n_out + j]);
      db[j] = s;
    }
    return;
  }
  const int i = it * 32 + (lane & 31);
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < rows; r0 += 32) {
    float a[16], b[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = r0 + 2 * q + h;
      const bool ok = r < rows;
      a[q] = (ok && i < Kin) ? X[(int64_t)r * Kin + i] : 0.f;
      b[q] = ok ? dY[(int64_t)r * n_out + j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int row = it * 32 + acc_row(v, lane);
    if (row < Kin) dW[(int64_t)row * n_out + j] = acc[v];
  }
}

bool dims_ok(int D, int H, int E) {
  return D >= 1 && D <= MAX_D && H >= 32 && H <= MAX_DIM && H % 32 == 0 && E >= 32 && E <= MAX_DIM && E % 32 == 0;
}

}  // namespace

extern "C" int cadre_rnd_obs_stats(const void* obs_table, int32_t N, int32_t T, int32_t S, int64_t ldo, int32_t D, int32_t update,
                                   double* state, void* stream) {
  FAIL_IF(!obs_table || !state, "cadre_rnd_obs_stats: null operand");
  FAIL_IF(N < 1 || T < 1 || S < 1 || D < 1 || D > MAX_D || ldo < D || (int64_t)N * T > (1 << 24),
          "cadre_rnd_obs_stats: bad argument (N, T, S >= 1, 1 <= D <= 1024, ldo >= D, N T <= 2^24)");
  if (!update) return 0;                                          // evaluation: the stored statistics stand
  hipLaunchKernelGGL(obs_stats_kernel, dim3((D + 63) / 64), dim3(64, 16), 0, ST(stream), (const float* const*)obs_table, N, T, S, ldo,
                     D, state);
  hipLaunchKernelGGL(obs_count_kernel, dim3(1), dim3(64), 0, ST(stream), state, N * T);
  return (int)hipGetLastError();
}

extern "C" int cadre_rnd_forward(const void* obs_table, int32_t N, int32_t T, int32_t S, int64_t ldo, int32_t D, int32_t H, int32_t E,
                                 int32_t row0, int32_t rows, const double* state, double eps_obs, float clip, const float* target,
                                 const float* predictor, float* err, float* xh, float* h1, float* h2, float* diff, void* stream) {
  FAIL_IF(!obs_table || !state || !target || !predictor || !err, "cadre_rnd_forward: null operand");
  FAIL_IF(N < 1 || T < 1 || S < 1 || ldo < D || (int64_t)N * T > (1 << 24) || !dims_ok(D, H, E),
          "cadre_rnd_forward: bad argument (N, T, S >= 1, 1 <= D <= 1024, ldo >= D, N T <= 2^24, hidden and embed multiples of 32 "
          "up to 256)");
  FAIL_IF(row0 < 0 || rows < 1 || (int64_t)row0 + rows > (int64_t)N * T, "cadre_rnd_forward: rows outside 0 .. N T - 1");
  FAIL_IF(!(eps_obs >= 0.0) || !(eps_obs < INFINITY) || !(clip > 0.f), "cadre_rnd_forward: eps_obs must be finite >= 0, clip > 0");
  const size_t shm = sizeof(float) * (64 + 32 * PX + 2 * KC + 2 * 32 * (H + 2) + 2 * 32 * (E + 2));
  // above 64 KiB of dynamic LDS a kernel needs the opt-in, per device: set when needed, at every such call (a host-side setting)
  if (shm > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)rnd_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    FAIL_IF(e != hipSuccess, "cadre_rnd_forward: the device refused the dynamic LDS size of this hidden / embed");
  }
  hipLaunchKernelGGL(rnd_forward_kernel, dim3((rows + 31) / 32), dim3(256), shm, ST(stream), (const float* const*)obs_table, T, S, ldo,
                     D, H, E, row0, rows, state, eps_obs, clip, target, predictor, err, xh, h1, h2, diff);
  return (int)hipGetLastError();
}

extern "C" int cadre_rnd_reward(const float* err, int32_t N, int32_t T, const void* row_table, double* state, int32_t D, double gamma,
                                double eps, int32_t update, void* stream) {
  FAIL_IF(!err || !row_table || !state, "cadre_rnd_reward: null operand");
  FAIL_IF(N < 1 || T < 1 || D < 1 || D > MAX_D || (int64_t)N * T > (1 << 24) || !(gamma >= 0.0 && gamma <= 1.0) || !(eps > 0.0) ||
              !(eps < INFINITY),
          "cadre_rnd_reward: bad argument (N, T >= 1, N T <= 2^24, 1 <= D <= 1024, 0 <= gamma <= 1, finite eps > 0)");
  hipLaunchKernelGGL(rnd_reward_kernel, dim3(1), dim3(256), 0, ST(stream), err, N, T, (const rnd_row_t*)row_table, state, D, gamma, eps,
                     update);
  return (int)hipGetLastError();
}

extern "C" int cadre_rnd_backward(const float* xh, const float* h1, const float* h2, const float* diff, const float* err, int32_t rows,
                                  int32_t D, int32_t H, int32_t E, const float* predictor, double* state, int32_t thresh, float* grads,
                                  float* loss, float* scratch, void* stream) {
  FAIL_IF(!xh || !h1 || !h2 || !diff || !err || !predictor || !state || !grads || !loss || !scratch, "cadre_rnd_backward: null operand");
  FAIL_IF(rows < 1 || rows > (1 << 24) || !dims_ok(D, H, E) || thresh < 0 || thresh > (1 << 24),
          "cadre_rnd_backward: bad argument (1 <= rows <= 2^24, 1 <= D <= 1024, hidden and embed multiples of 32 up to 256, "
          "0 <= thresh <= 2^24)");
  float* mask = scratch, *cnt = mask + rows, *dO = cnt + 2, *dH2 = dO + (int64_t)rows * E, *dH1 = dH2 + (int64_t)rows * H;
  const float* W2 = predictor + (int64_t)D * H + H, *W3 = W2 + (int64_t)H * H + H;
  float* gW1 = grads, *gb1 = gW1 + (int64_t)D * H, *gW2 = gb1 + H, *gb2 = gW2 + (int64_t)H * H, *gW3 = gb2 + H, *gb3 = gW3 + (int64_t)H * E;
  const dim3 tiles((rows + 31) / 32);
  hipStream_t st = ST(stream);
  hipLaunchKernelGGL(rnd_mask_kernel, dim3(1), dim3(256), 0, st, err, rows, state, thresh, mask, cnt, loss);
  hipLaunchKernelGGL(rnd_dx_kernel<true>, tiles, dim3(256), sizeof(float) * 32 * (E + 2), st, diff, E, W3, h2, dH2, H, rows, mask, cnt, dO);
  hipLaunchKernelGGL(rnd_dw_kernel, dim3(E / 32, H / 32 + 1), dim3(64), 0, st, h2, dO, rows, H, E, gW3, gb3);
  hipLaunchKernelGGL(rnd_dx_kernel<false>, tiles, dim3(256), sizeof(float) * 32 * (H + 2), st, dH2, H, W2, h1, dH1, H, rows, nullptr,
                     nullptr, nullptr);
  hipLaunchKernelGGL(rnd_dw_kernel, dim3(H / 32, H / 32 + 1), dim3(64), 0, st, h1, dH2, rows, H, H, gW2, gb2);
  hipLaunchKernelGGL(rnd_dw_kernel, dim3(H / 32, (D + 31) / 32 + 1), dim3(64), 0, st, xh, dH1, rows, D, H, gW1, gb1);
  return (int)hipGetLastError();
}
