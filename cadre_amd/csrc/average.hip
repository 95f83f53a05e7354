// average.hip — weight averaging on the parameter arena: cadre_ema_update (the exponential moving average of the parameters
// behind an optimiser step, with the per-model squared distance between the two), cadre_arena_swap (exchange two flat
// buffers in one pass) and cadre_arena_mean (the weighted mean of K flat buffers, accumulated in double).
//
// All three are plain HBM streams: 16-byte loads and stores on the aligned body of a range, scalar words before and behind
// it (as state_capture_kernel does), nothing kept between launches but what the header names.  Traffic of the average:
// 12 bytes per element (read p, read e, write e); the distance is formed from the values already in registers.
//
// The distance is summed in a fixed order — per lane over its grid-stride elements, per wave by butterfly, per workgroup
// over its four waves, per model over the CADRE_EMA_GRID workgroup partials in `work` by the finishing launch — so two runs
// over equal bytes give equal bits.  Everything here is written with plain vector stores; there is no atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

constexpr int BLOCK = 256;                 // 4 waves
constexpr int GX = CADRE_EMA_GRID;         // workgroups that stride over one model's segment (x); y = the model
constexpr int STREAM_GRID = 2048;          // workgroups of the swap and the mean (grid-stride over the 16-byte vectors)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// words before the first 16-byte boundary of `ptr`, at most n
__device__ __forceinline__ int64_t head_words(const void* ptr, int64_t n) {
  const int64_t h = (int64_t)(((16 - ((uintptr_t)ptr & 15)) & 15) >> 2);
  return h < n ? h : n;
}

// four consecutive floats at s: one 16-byte load where s is aligned (VEC), four words otherwise
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* s) {
  if (VEC) return *reinterpret_cast<const float4*>(s);
  return make_float4(s[0], s[1], s[2], s[3]);
}

// ---------------------------------------------------------------------------------------------------- the moving average
// One element of the rule: t = p - e rounded to fp32, e' = fma(om, t, e) — the lerp form, so p == e keeps e (t == 0 keeps
// the bits of e outright: fma(om, +0, -0) would turn a negative zero over).  d2 gains ((double)p - (double)e')^2.
__device__ __forceinline__ float ema_elem(float p, float e, float om, double& d2) {
  const float t = __fsub_rn(p, e);
  const float en = (t == 0.f) ? e : __fmaf_rn(om, t, e);
  const double d = __dsub_rn((double)p, (double)en);
  d2 = __dadd_rn(d2, __dmul_rn(d, d));
  return en;
}

__device__ __forceinline__ float4 ema_vec(const float4 p, const float4 e, float om, double& d2) {
  float4 o;
  o.x = ema_elem(p.x, e.x, om, d2);
  o.y = ema_elem(p.y, e.y, om, d2);
  o.z = ema_elem(p.z, e.z, om, d2);
  o.w = ema_elem(p.w, e.w, om, d2);
  return o;
}

// The 16-byte body of a segment: vectors [v0, nvec) step `stride`, vector v = elements 4 v .. 4 v + 3 of e4 (16-byte
// aligned) and p4 (aligned iff PVEC).  Two vectors of each side in flight per lane.
template <bool PVEC>
__device__ __forceinline__ double ema_body(const float* p4, float* e4, int64_t v0, int64_t nvec, int64_t stride, float om) {
  double d2 = 0.0;
  int64_t v = v0;
  for (; v + stride < nvec; v += 2 * stride) {
    const float4 pa = load4<PVEC>(p4 + 4 * v), pb = load4<PVEC>(p4 + 4 * (v + stride));
    const float4 ea = *reinterpret_cast<const float4*>(e4 + 4 * v), eb = *reinterpret_cast<const float4*>(e4 + 4 * (v + stride));
    *reinterpret_cast<float4*>(e4 + 4 * v) = ema_vec(pa, ea, om, d2);
    *reinterpret_cast<float4*>(e4 + 4 * (v + stride)) = ema_vec(pb, eb, om, d2);
  }
  if (v < nvec) {
    const float4 pa = load4<PVEC>(p4 + 4 * v);
    const float4 ea = *reinterpret_cast<const float4*>(e4 + 4 * v);
    *reinterpret_cast<float4*>(e4 + 4 * v) = ema_vec(pa, ea, om, d2);
  }
  return d2;
}

// The gate and the decay of the call, before any workgroup of the pass runs: work[0] = 1 (go) / 0 (skipped), work[1] = d.
// The count itself moves in ema_finish_kernel, behind the pass.
__global__ void ema_prep_kernel(double* state, double* work, const int32_t* stop) {
  if (threadIdx.x != 0) return;
  if (stop && *stop != 0) {
    state[CADRE_EMA_SKIPPED] += 1.0;
    work[0] = 0.0;
    return;
  }
  const double n = state[CADRE_EMA_COUNT];
  double d = state[CADRE_EMA_DECAY];
  if (state[CADRE_EMA_WARMUP] != 0.0) {
    const double w = __ddiv_rn(1.0 + n, 10.0 + n);
    d = w < d ? w : d;
  }
  work[0] = 1.0;
  work[1] = d;
}

// Model m = blockIdx.y, elements [seg_off[m], seg_off[m + 1]).  Elements before the first 16-byte boundary of e and the
// last < 4 go as single words (workgroup 0 of the model), the rest as 16-byte vectors, grid-stride over the x workgroups.
// Every workgroup leaves its partial of the model's squared distance in work[CADRE_EMA_WORK_HEAD + m * GX + x].
__global__ __launch_bounds__(BLOCK) void ema_kernel(const float* __restrict__ params, float* __restrict__ ema,
                                                    const int64_t* __restrict__ seg_off, double* __restrict__ work) {
  if (work[0] == 0.0) return;                          // (the gate: uniform over the grid)
  __shared__ double part[BLOCK / 64];
  const int m = blockIdx.y, bx = blockIdx.x, tid = threadIdx.x;
  const float om = (float)(1.0 - work[1]);
  const int64_t lo = seg_off[m], hi = seg_off[m + 1];
  const int64_t n = hi > lo ? hi - lo : 0;
  const float* p = params + lo;
  float* e = ema + lo;
  const int64_t head = head_words(e, n);
  const int64_t nvec = (n - head) >> 2;
  const int64_t v0 = (int64_t)bx * BLOCK + tid, stride = (int64_t)GX * BLOCK;
  double d2;
  if ((((uintptr_t)(p + head)) & 15) == 0) d2 = ema_body<true>(p + head, e + head, v0, nvec, stride, om);
  else d2 = ema_body<false>(p + head, e + head, v0, nvec, stride, om);
  if (bx == 0) {
    if (tid < head) e[tid] = ema_elem(p[tid], e[tid], om, d2);
    const int64_t i = head + 4 * nvec + tid;           // at most three words
    if (i < n) e[i] = ema_elem(p[i], e[i], om, d2);
  }
  d2 = wave_sum(d2);
  if ((tid & 63) == 0) part[tid >> 6] = d2;
  __syncthreads();
  if (tid == 0) work[CADRE_EMA_WORK_HEAD + (int64_t)m * GX + bx] = (part[0] + part[1]) + (part[2] + part[3]);
}

// One wave per model sums the model's GX partials in a fixed order; the first also moves EMA_D and EMA_COUNT.
__global__ __launch_bounds__(64) void ema_finish_kernel(double* state, const double* work, int n_models) {
  if (work[0] == 0.0) return;
  const int m = blockIdx.x, lane = threadIdx.x;
  if (m < n_models) {
    const double* w = work + CADRE_EMA_WORK_HEAD + (int64_t)m * GX;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < GX / 64; ++k) s += w[lane + 64 * k];
    s = wave_sum(s);
    if (lane == 0) state[CADRE_EMA_HEAD + m] = s;
  }
  if (m == 0 && lane == 0) {
    state[CADRE_EMA_D] = work[1];
    state[CADRE_EMA_COUNT] = state[CADRE_EMA_COUNT] + 1.0;
  }
}

// ---------------------------------------------------------------------------------------------------- swap
template <bool BVEC>
__device__ __forceinline__ void swap_body(float* a4, float* b4, int64_t v0, int64_t nvec, int64_t stride) {
  for (int64_t v = v0; v < nvec; v += stride) {
    const float4 x = *reinterpret_cast<const float4*>(a4 + 4 * v);
    const float4 y = load4<BVEC>(b4 + 4 * v);
    *reinterpret_cast<float4*>(a4 + 4 * v) = y;
    if (BVEC) {
      *reinterpret_cast<float4*>(b4 + 4 * v) = x;
    } else {
      float* b = b4 + 4 * v;
      b[0] = x.x; b[1] = x.y; b[2] = x.z; b[3] = x.w;
    }
  }
}

// The body is cut at the 16-byte boundaries of a; b goes by 16 bytes where it is aligned like a, else by words.  Every
// element is read and written by one thread only, and the two ranges do not overlap (the entry point refuses that).
__global__ __launch_bounds__(BLOCK) void arena_swap_kernel(float* a, float* b, int64_t n) {
  const int bx = blockIdx.x, tid = threadIdx.x;
  const int64_t head = head_words(a, n);
  const int64_t nvec = (n - head) >> 2;
  const int64_t v0 = (int64_t)bx * BLOCK + tid, stride = (int64_t)gridDim.x * BLOCK;
  if ((((uintptr_t)(b + head)) & 15) == 0) swap_body<true>(a + head, b + head, v0, nvec, stride);
  else swap_body<false>(a + head, b + head, v0, nvec, stride);
  if (bx == 0) {
    if (tid < head) { const float x = a[tid]; a[tid] = b[tid]; b[tid] = x; }
    const int64_t i = head + 4 * nvec + tid;
    if (i < n) { const float x = a[i]; a[i] = b[i]; b[i] = x; }
  }
}

// ---------------------------------------------------------------------------------------------------- weighted mean
// acc starts at -0.0, so the first fma gives exactly the rounded product w_0 x_0 (sign of a zero included) and K = 1 with
// weight 1 copies the bits.
__device__ __forceinline__ float mean_elem(const int64_t* table, const double* w, int K, int64_t i) {
  double acc = -0.0;
  for (int k = 0; k < K; ++k) acc = fma(w[k], (double)reinterpret_cast<const float*>(table[k])[i], acc);
  return (float)acc;
}

// A thread reads all K values of its elements before it writes them, and no other thread reads them: `out` may be one
// of the sources.  The body is cut at the 16-byte boundaries of out; a source aligned like it goes by 16-byte loads.
__global__ __launch_bounds__(BLOCK) void arena_mean_kernel(const int64_t* __restrict__ table, const double* __restrict__ w, int K,
                                                           float* out, int64_t n) {
  const int bx = blockIdx.x, tid = threadIdx.x;
  const int64_t head = head_words(out, n);
  const int64_t nvec = (n - head) >> 2;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t v = (int64_t)bx * BLOCK + tid; v < nvec; v += stride) {
    const int64_t i = head + 4 * v;
    double a0 = -0.0, a1 = -0.0, a2 = -0.0, a3 = -0.0;
    for (int k = 0; k < K; ++k) {
      const float* s = reinterpret_cast<const float*>(table[k]) + i;
      const float4 x = (((uintptr_t)s) & 15) == 0 ? load4<true>(s) : load4<false>(s);
      const double wk = w[k];
      a0 = fma(wk, (double)x.x, a0);
      a1 = fma(wk, (double)x.y, a1);
      a2 = fma(wk, (double)x.z, a2);
      a3 = fma(wk, (double)x.w, a3);
    }
    *reinterpret_cast<float4*>(out + i) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
  }
  if (bx == 0) {
    if (tid < head) out[tid] = mean_elem(table, w, K, tid);
    const int64_t i = head + 4 * nvec + tid;
    if (i < n) out[i] = mean_elem(table, w, K, i);
  }
}

int stream_grid(int64_t n) {
  const int64_t g = (n / 4 + BLOCK - 1) / BLOCK;
  return (int)(g < 1 ? 1 : (g > STREAM_GRID ? STREAM_GRID : g));
}

}  // namespace

extern "C" int cadre_ema_update(const float* params, float* ema, const int64_t* seg_off, int32_t n_models, double* state,
                                double* work, const int32_t* stop, void* stream) {
  FAIL_IF(n_models < 0 || n_models > CADRE_EMA_MAX_MODELS, "cadre_ema_update: bad argument (0 <= n_models <= 4096)");
  FAIL_IF(!params || !ema || !seg_off || !state || !work, "cadre_ema_update: null operand");
  FAIL_IF(((uintptr_t)params & 3) || ((uintptr_t)ema & 3) || ((uintptr_t)seg_off & 7) || ((uintptr_t)state & 7) ||
          ((uintptr_t)work & 7) || ((uintptr_t)stop & 3),
          "cadre_ema_update: misaligned operand (params, ema and stop 4 bytes; seg_off, state and work 8 bytes)");
  hipLaunchKernelGGL(ema_prep_kernel, dim3(1), dim3(64), 0, ST(stream), state, work, stop);
  if (n_models > 0)
    hipLaunchKernelGGL(ema_kernel, dim3(GX, n_models), dim3(BLOCK), 0, ST(stream), params, ema, seg_off, work);
  hipLaunchKernelGGL(ema_finish_kernel, dim3(n_models > 0 ? n_models : 1), dim3(64), 0, ST(stream), state,
                     (const double*)work, (int)n_models);
  return (int)hipGetLastError();
}

extern "C" int cadre_arena_swap(float* a, float* b, int64_t n, void* stream) {
  FAIL_IF(n < 0, "cadre_arena_swap: bad argument (n >= 0)");
  if (n == 0) return 0;
  FAIL_IF(!a || !b, "cadre_arena_swap: null operand");
  FAIL_IF(((uintptr_t)a & 3) || ((uintptr_t)b & 3), "cadre_arena_swap: misaligned operand (4 bytes)");
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  FAIL_IF(ua < ub + bytes && ub < ua + bytes, "cadre_arena_swap: the two ranges overlap");
  hipLaunchKernelGGL(arena_swap_kernel, dim3(stream_grid(n)), dim3(BLOCK), 0, ST(stream), a, b, n);
  return (int)hipGetLastError();
}

extern "C" int cadre_arena_mean(const int64_t* src_table, const double* weights, int32_t K, float* out, int64_t n,
                                void* stream) {
  FAIL_IF(K < 1 || K > CADRE_MEAN_MAX_SOURCES || n < 0, "cadre_arena_mean: bad argument (1 <= K <= 64, n >= 0)");
  if (n == 0) return 0;
  FAIL_IF(!src_table || !weights || !out, "cadre_arena_mean: null operand");
  FAIL_IF(((uintptr_t)src_table & 7) || ((uintptr_t)weights & 7) || ((uintptr_t)out & 3),
          "cadre_arena_mean: misaligned operand (table and weights 8 bytes, out 4 bytes)");
  hipLaunchKernelGGL(arena_mean_kernel, dim3(stream_grid(n)), dim3(BLOCK), 0, ST(stream), src_table, weights, (int)K, out, n);
  return (int)hipGetLastError();
}
