// constraint.hip — cost constraints, PPO-Lagrangian with one cost critic per head (cadre_amd/constraint.py):
//   cadre_cost_note      costs[k][slot[k]] = cost[k] for the 2N storages of one env step
//   cadre_cost_forward   the cost critic D -> H -> H -> 1 (ReLU) on the newest frame row of the storages' window rows
//   cadre_cost_backward  the gradient of 0.5 mean (v - cost_returns)^2 in the tower's flat layout
//   cadre_cost_lambda    the cost rate J of each head and the projected multiplier step
//   cadre_lag_mix        advantages <- (A_r - lambda (A_c - mean A_c)) / (1 + lambda) per storage
//
// The dense products run on v_mfma_f32_32x32x2_f32 (exact fp32) through the tile product of tower.h.  Every sum has a fixed order
// and nothing is accumulated with atomics; everything is written with plain vector stores.
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

constexpr int MAX_DIM = 256;     // hidden
constexpr int MAX_D = 1024;
constexpr int MAX_T = 3000;      // what cadre_gae_multi accepts

struct mix_row_t { const float* cost_adv; float* advantages; };

// the newest frame row of row r = w * Tr + t of the table's storages
__device__ __forceinline__ const float* obs_row(const float* const* obs, int r, int Tr, int S, int64_t ldo) {
  const int w = r / Tr, t = r - w * Tr;
  return obs[w] + ((int64_t)t * S + (S - 1)) * ldo;
}

// sum_r a[r * lda] b[r * ldb] (b == NULL: sum_r a[r * lda]) over r < rows in row order, one rounded product and one rounded add per
// row; eight rows are loaded before their adds are issued, which leaves the order as it is
__device__ __forceinline__ float ordered_sum(const float* a, int64_t lda, const float* b, int64_t ldb, int rows) {
#pragma clang fp contract(off)
  float s = 0.f;
  int r = 0;
  for (; r + 8 <= rows; r += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = b ? (a[(int64_t)(r + u) * lda] * b[(int64_t)(r + u) * ldb]) : a[(int64_t)(r + u) * lda];
#pragma unroll
    for (int u = 0; u < 8; ++u) s = (s + v[u]);
  }
  for (; r < rows; ++r) s = (s + (b ? (a[(int64_t)r * lda] * b[(int64_t)r * ldb]) : a[(int64_t)r * lda]));
  return s;
}

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

// ---------------------------------------------------------------------------- costs of one env step
__global__ __launch_bounds__(64) void cost_note_kernel(const int64_t* table, const int32_t* slots, const float* costs, int n, int T) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  float* c = reinterpret_cast<float*>(table[k]);
  const int s = slots[k];
  if (c && s >= 0 && s <= T) c[s] = costs[k];
}

// ---------------------------------------------------------------------------- the cost critic
// One workgroup (4 waves) per 32 rows.  LDS (all dynamic): the rows' pointers, the feature chunk [32][PX], h1 and h2 [32][H + 2].
// The row tail and the k tail are zeros in LDS; nothing behind column D - 1 of a storage row or row D - 1 of W1 is read.
__global__ __launch_bounds__(256) void cost_forward_kernel(const float* const* obs, int Tr, int S, int64_t ldo, int D, int H, int row0,
                                                           int rows, const float* P, float* values, float* h1, float* h2) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  const float** rowp = (const float**)sm;                // 32 row pointers in front of the float arrays
  const int PH = H + 2;
  float* xs = sm + 64, *h1s = xs + 32 * PX, *h2s = h1s + 32 * PH;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.x * 32, valid = min(32, rows - i0);
  if (tid < 32) rowp[tid] = obs_row(obs, row0 + i0 + min(tid, valid - 1), Tr, S, ldo);
  const float* W1 = P, *b1 = W1 + (int64_t)D * H, *W2 = b1 + H, *b2 = W2 + (int64_t)H * H, *W3 = b2 + H, *b3 = W3 + H;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
  for (int k0 = 0; k0 < D; k0 += KC) {
    __syncthreads();                                     // the chunk before this one (and rowp) is no longer read / is written
    for (int idx = tid; idx < 32 * KC; idx += 256) {
      const int row = idx / KC, k = idx - row * KC, d = k0 + k;
      xs[row * PX + k] = (row < valid && d < D) ? rowp[row][d] : 0.f;
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
    if (ct < H / 32) tile_out<true>(acc[t], b1, ct, h1s, PH, h1 ? h1 + (int64_t)i0 * H : nullptr, H, valid, lane);
  }
  __syncthreads();
  dense_lds<true>(h1s, PH, H, W2, b2, H, h2s, PH, h2 ? h2 + (int64_t)i0 * H : nullptr, valid, wave, lane);
  __syncthreads();
  if (tid < valid) {                                     // the last layer: a dot product over h2 in k order, then the bias
    float s = 0.f;
    for (int k = 0; k < H; ++k) s = (s + (h2s[tid * PH + k] * W3[k]));
    values[i0 + tid] = (s + b3[0]);
  }
}

// ---------------------------------------------------------------------------- the cost critic's backward
// One workgroup: d = v - R, dv = d / rows, loss[0] = 0.5 mean d^2, loss[1] = rows, db3 = sum dv (float64 partials of thread tid over
// rows tid, tid + 256, ..., met in a fixed tree).
__global__ __launch_bounds__(256) void cost_dv_kernel(const float* values, const float* returns, int64_t ldr, int Tr, int row0, int rows,
                                                      float* dv, float* gb3, float* loss) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float fr = (float)rows;
  double q = 0.0, s = 0.0;
  for (int i = tid; i < rows; i += 256) {
    const int r = row0 + i, w = r / Tr, t = r - w * Tr;
    const float d = (values[i] - returns[(int64_t)w * ldr + t]);
    const float g = (d / fr);
    dv[i] = g;
    q += (double)d * (double)d;
    s += (double)g;
  }
  const double qt = block_sum_256(q, red, tid), st = block_sum_256(s, red, tid);
  if (tid == 0) {
    loss[0] = (float)(0.5 * qt / (double)rows);
    loss[1] = fr;
    gb3[0] = (float)st;
  }
}

// Workgroups 0 .. tiles - 1: dH2 = (dv W3^T) where h2 > 0 for 32 rows each; the workgroup behind them: dW3[j] = sum_i h2[i][j] dv[i]
// in row order, one thread per column.
__global__ __launch_bounds__(256) void cost_top_kernel(const float* h2, const float* dv, const float* W3, int rows, int H, float* dH2,
                                                       float* gW3) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  if (blockIdx.x == gridDim.x - 1) {
    for (int j = tid; j < H; j += 256) gW3[j] = ordered_sum(h2 + j, H, dv, 1, rows);
    return;
  }
  const int i0 = blockIdx.x * 32, valid = min(32, rows - i0);
  for (int idx = tid; idx < valid * H; idx += 256) {
    const int row = idx / H, k = idx - row * H;
    const int64_t o = (int64_t)(i0 + row) * H + k;
    dH2[o] = h2[o] > 0.f ? (dv[i0 + row] * W3[k]) : 0.f;
  }
}

// dX [rows][n_out] = (dY [rows][Kd] . W^T) where act > 0, W [n_out][Kd] (a layer's input-major matrix).  One workgroup per 32 rows.
__global__ __launch_bounds__(256) void cost_dx_kernel(const float* dY, int Kd, const float* W, const float* act, float* dX, int n_out,
                                                      int rows) {
#pragma clang fp contract(off)
  extern __shared__ float sm[];
  const int PY = Kd + 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.x * 32, valid = min(32, rows - i0);
  for (int idx = tid; idx < 32 * Kd; idx += 256) {
    const int row = idx / Kd, k = idx - row * Kd;
    sm[row * PY + k] = row < valid ? dY[(int64_t)(i0 + row) * Kd + k] : 0.f;
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

// dW [Kin][n_out] = X^T [Kin][rows] . dY [rows][n_out] and db = the column sums of dY.  One wave per 32 x 32 tile of dW walks all
// rows in order; the tiles of blockIdx.y == n_it sum the bias columns, one lane per column, in row order.  X: a dense [rows][Kin]
// array, or (obs != NULL) the storage rows themselves: row r of the step is row row0 + r of the table's storages.
__global__ __launch_bounds__(64) void cost_dw_kernel(const float* X, const float* const* obs, int Tr, int S, int64_t ldo, int row0,
                                                     const float* dY, int rows, int Kin, int n_out, float* dW, float* db) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, jt = blockIdx.x, it = blockIdx.y, h = lane >> 5;
  const int j = jt * 32 + (lane & 31);
  if (it == (Kin + 31) / 32) {
    if (lane < 32) db[j] = ordered_sum(dY + j, n_out, nullptr, 0, rows);
    return;
  }
  const int i = it * 32 + (lane & 31);
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < rows; r0 += 32) {
    float a[16], b[16];
    int w = 0, t = 0;                                    // (storage, row) of this lane's next row: one division per 32 rows
    if (obs) {
      w = (row0 + r0 + h) / Tr;
      t = row0 + r0 + h - w * Tr;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = r0 + 2 * q + h;
      const bool ok = r < rows;
      a[q] = 0.f;
      if (ok && i < Kin) a[q] = obs ? (obs[w] + ((int64_t)t * S + (S - 1)) * ldo)[i] : X[(int64_t)r * Kin + i];
      b[q] = ok ? dY[(int64_t)r * n_out + j] : 0.f;
      if (obs) {
        t += 2;
        while (t >= Tr) {
          t -= Tr;
          ++w;
        }
      }
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

// ---------------------------------------------------------------------------- the multiplier
// One workgroup per head.  Thread tid sums rows tid, tid + 256, ... of the head's N T rows in (storage, time) order in float64; the
// partials meet in a fixed tree.  Then, when updating, the projected step of lambda.
__global__ __launch_bounds__(256) void cost_lambda_kernel(const float* const* costs, int N, int T, double* state, int update) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x, h = blockIdx.x, total = N * T;
  double s = 0.0, p = 0.0;
  for (int i = tid; i < total; i += 256) {
    const int w = i / T, t = i - w * T;
    const float c = costs[2 * w + h][t];
    s += (double)c;
    if (c > 0.f) p += 1.0;
  }
  const double st = block_sum_256(s, red, tid), pt = block_sum_256(p, red, tid);
  if (tid != 0) return;
  double* b = state + h * CADRE_LAG_STRIDE;
  const double J = (st / (double)total);
  b[CADRE_LAG_J] = J;
  b[CADRE_LAG_SHARE] = (pt / (double)total);
  if (update) {
    const double e = (J - b[CADRE_LAG_BUDGET]);
    const double g = (b[CADRE_LAG_LR] * e);
    double lam = (b[CADRE_LAG_LAMBDA] + g);
    lam = fmin(fmax(lam, 0.0), b[CADRE_LAG_MAX]);
    b[CADRE_LAG_LAMBDA] = lam;
    b[CADRE_LAG_UPDATES] = (b[CADRE_LAG_UPDATES] + 1.0);
  }
}

// ---------------------------------------------------------------------------- the mix
// One workgroup per storage.  The cost advantages go through LDS once; thread 0 sums them in row order in float64.  With
// (float)lambda == 0 nothing is stored into `advantages`.  diag (may be NULL) double [n][2]: mean |lambda (A_c - m)| / (1 + lambda)
// and mean |A_r| / (1 + lambda) of the storage.
__global__ __launch_bounds__(256) void lag_mix_kernel(const mix_row_t* rows, int T, const double* state, double* diag) {
#pragma clang fp contract(off)
  extern __shared__ float ca[];
  __shared__ double red[256];
  __shared__ float ms;
  const int tid = threadIdx.x, k = blockIdx.x;
  const float lam = (float)state[(k & 1) * CADRE_LAG_STRIDE + CADRE_LAG_LAMBDA];
  if (lam == 0.f && !diag) return;
  const float* cost_adv = rows[k].cost_adv;
  float* adv = rows[k].advantages;
  for (int t = tid; t < T; t += 256) ca[t] = cost_adv[t];
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s = (s + (double)ca[t]);
    ms = ((float)s / (float)T);
  }
  __syncthreads();
  const float m = ms, den = (1.f + lam);
  double sp = 0.0, sr = 0.0;
  for (int t = tid; t < T; t += 256) {
    const float ar = adv[t];
    const float c = (ca[t] - m);
    const float p = (lam * c);
    const float q = (ar - p);
    if (lam != 0.f) adv[t] = (q / den);
    sp += (double)fabsf(p) / (double)den;
    sr += (double)fabsf(ar) / (double)den;
  }
  if (!diag) return;
  const double spt = block_sum_256(sp, red, tid), srt = block_sum_256(sr, red, tid);
  if (tid == 0) {
    diag[2 * k] = spt / (double)T;
    diag[2 * k + 1] = srt / (double)T;
  }
}

bool dims_ok(int D, int H) { return D >= 1 && D <= MAX_D && H >= 32 && H <= MAX_DIM && H % 32 == 0; }

}  // namespace

extern "C" int cadre_cost_note(const void* table, const int32_t* slots, const float* costs, int32_t n, int32_t T, void* stream) {
  FAIL_IF(!table || !slots || !costs || n < 1 || T < 1, "cadre_cost_note: bad argument");
  hipLaunchKernelGGL(cost_note_kernel, dim3((n + 63) / 64), dim3(64), 0, ST(stream), (const int64_t*)table, slots, costs, n, T);
  return (int)hipGetLastError();
}

extern "C" int cadre_cost_forward(const void* obs_table, int32_t n, int32_t Tr, int32_t S, int64_t ldo, int32_t D, int32_t H,
                                  int32_t row0, int32_t rows, const float* tower, float* values, float* h1, float* h2, void* stream) {
  FAIL_IF(!obs_table || !tower || !values, "cadre_cost_forward: null operand");
  FAIL_IF(n < 1 || Tr < 1 || S < 1 || ldo < D || (int64_t)n * Tr > (1 << 24) || !dims_ok(D, H),
          "cadre_cost_forward: bad argument (n, Tr, S >= 1, 1 <= D <= 1024, ldo >= D, n Tr <= 2^24, hidden a multiple of 32 up to 256)");
  FAIL_IF(row0 < 0 || rows < 1 || (int64_t)row0 + rows > (int64_t)n * Tr, "cadre_cost_forward: rows outside 0 .. n Tr - 1");
  const size_t shm = sizeof(float) * (64 + 32 * PX + 2 * 32 * (H + 2));
  // above 64 KiB of dynamic LDS a kernel needs the opt-in, per device: set when needed, at every such call (a host-side setting)
  if (shm > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)cost_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    FAIL_IF(e != hipSuccess, "cadre_cost_forward: the device refused the dynamic LDS size of this hidden width");
  }
  hipLaunchKernelGGL(cost_forward_kernel, dim3((rows + 31) / 32), dim3(256), shm, ST(stream), (const float* const*)obs_table, Tr, S, ldo,
                     D, H, row0, rows, tower, values, h1, h2);
  return (int)hipGetLastError();
}

extern "C" int cadre_cost_backward(const void* obs_table, int32_t n, int32_t Tr, int32_t S, int64_t ldo, int32_t D, int32_t H,
                                   int32_t row0, int32_t rows, const float* tower, const float* values, const float* h1, const float* h2,
                                   const float* returns, int64_t ldr, float* grads, float* loss, float* scratch, void* stream) {
  FAIL_IF(!obs_table || !tower || !values || !h1 || !h2 || !returns || !grads || !loss || !scratch, "cadre_cost_backward: null operand");
  FAIL_IF(n < 1 || Tr < 1 || S < 1 || ldo < D || ldr < Tr || (int64_t)n * Tr > (1 << 24) || !dims_ok(D, H),
          "cadre_cost_backward: bad argument (n, Tr, S >= 1, 1 <= D <= 1024, ldo >= D, ldr >= Tr, n Tr <= 2^24, hidden a multiple of 32 "
          "up to 256)");
  FAIL_IF(row0 < 0 || rows < 1 || (int64_t)row0 + rows > (int64_t)n * Tr, "cadre_cost_backward: rows outside 0 .. n Tr - 1");
  float* dv = scratch, *dH2 = dv + rows, *dH1 = dH2 + (int64_t)rows * H;
  const float* W2 = tower + (int64_t)D * H + H, *W3 = W2 + (int64_t)H * H + H;
  float* gW1 = grads, *gb1 = gW1 + (int64_t)D * H, *gW2 = gb1 + H, *gb2 = gW2 + (int64_t)H * H, *gW3 = gb2 + H, *gb3 = gW3 + H;
  const int tiles = (rows + 31) / 32;
  const float* const* obs = (const float* const*)obs_table;
  hipStream_t st = ST(stream);
  hipLaunchKernelGGL(cost_dv_kernel, dim3(1), dim3(256), 0, st, values, returns, ldr, Tr, row0, rows, dv, gb3, loss);
  hipLaunchKernelGGL(cost_top_kernel, dim3(tiles + 1), dim3(256), 0, st, h2, dv, W3, rows, H, dH2, gW3);
  hipLaunchKernelGGL(cost_dw_kernel, dim3(H / 32, H / 32 + 1), dim3(64), 0, st, h1, nullptr, Tr, S, ldo, row0, dH2, rows, H, H, gW2, gb2);
  hipLaunchKernelGGL(cost_dx_kernel, dim3(tiles), dim3(256), sizeof(float) * 32 * (H + 2), st, dH2, H, W2, h1, dH1, H, rows);
  hipLaunchKernelGGL(cost_dw_kernel, dim3(H / 32, (D + 31) / 32 + 1), dim3(64), 0, st, nullptr, obs, Tr, S, ldo, row0, dH1, rows, D, H,
                     gW1, gb1);
  return (int)hipGetLastError();
}

extern "C" int cadre_cost_lambda(const void* cost_table, int32_t N, int32_t T, double* state, int32_t update, void* stream) {
  FAIL_IF(!cost_table || !state, "cadre_cost_lambda: null operand");
  FAIL_IF(N < 1 || N > 32767 || T < 2 || T > MAX_T, "cadre_cost_lambda: bad argument (1 <= N <= 32767 environments, 2 <= T <= 3000)");
  hipLaunchKernelGGL(cost_lambda_kernel, dim3(2), dim3(256), 0, ST(stream), (const float* const*)cost_table, N, T, state, update);
  return (int)hipGetLastError();
}

extern "C" int cadre_lag_mix(const void* row_table, int32_t n, int32_t T, const double* state, double* diag, void* stream) {
  FAIL_IF(!row_table || !state, "cadre_lag_mix: null operand");
  FAIL_IF(n < 2 || n > 65534 || (n & 1) || T < 2 || T > MAX_T,
          "cadre_lag_mix: bad argument (an even number of storages 2 .. 65534, 2 <= T <= 3000)");
  hipLaunchKernelGGL(lag_mix_kernel, dim3(n), dim3(256), sizeof(float) * T, ST(stream), (const mix_row_t*)row_table, T, state, diag);
  return (int)hipGetLastError();
}
