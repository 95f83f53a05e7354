// tower.h — the dense fp32 tile product of the small side networks (curiosity.hip, constraint.hip) on v_mfma_f32_32x32x2_f32.
// A wave owns 32 x 32 output tiles; per 32 k it first loads its 16 A and 16 B operands into registers and then issues the 16
// MFMAs back to back.  Device helpers only: every translation unit that includes this gets its own copies.
#ifndef CADRE_TOWER_H
#define CADRE_TOWER_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KC = 128;          // k-chunk of the first layer: 32 rows x KC features in LDS at a time
constexpr int PX = KC + 2;       // LDS pitches are 2 (mod 64): lane l reads [row l & 31][k + (l >> 5)], 64 distinct banks

// accumulator register v of lane l holds row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 tile
__device__ __forceinline__ int acc_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

// 32 k of one tile product.  Ar: this lane's row of A (LDS, or global with stride 1 in k); B(k) = Bg[k * ldb] for k < kvalid,
// else 0 (the k tail of the first layer: A is zero-filled there, the weights behind row D - 1 are not read).
__device__ __forceinline__ void mfma32(f32x16& acc, const float* Ar, const float* Bg, int64_t ldb, int kvalid, int lane) {
  const int h = lane >> 5;
  float a[16], b[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = Ar[2 * i + h];
#pragma unroll
  for (int i = 0; i < 16; ++i) b[i] = (2 * i + h < kvalid) ? Bg[(int64_t)(2 * i + h) * ldb] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
}

// bias, optional ReLU, the tile into LDS (every row: the tail rows hold the bias path of zero inputs and are never stored to
// global memory) and, when wanted, the valid rows to `save` [rows][n_out]
template <bool RELU>
__device__ __forceinline__ void tile_out(const f32x16& acc, const float* bias, int ct, float* Os, int ldo, float* save, int n_out,
                                         int valid, int lane) {
#pragma clang fp contract(off)
  const int col = ct * 32 + (lane & 31);
  const float bc = bias[col];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int row = acc_row(v, lane);
    float y = (acc[v] + bc);
    if (RELU) y = fmaxf(y, 0.f);
    Os[row * ldo + col] = y;
    if (save && row < valid) save[(int64_t)row * n_out + col] = y;
  }
}

// out [32][n_out] = act(A [32][K] . W [K][n_out] + b): A in LDS, W input-major in global memory; tile ct belongs to wave ct & 3
template <bool RELU>
__device__ __forceinline__ void dense_lds(const float* As, int lda, int K, const float* W, const float* bias, int n_out, float* Os,
                                          int ldo, float* save, int valid, int wave, int lane) {
  for (int ct = wave; ct < n_out / 32; ct += 4) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* Ar = As + (lane & 31) * lda;
    const float* Bg = W + ct * 32 + (lane & 31);
    for (int k0 = 0; k0 < K; k0 += 32) mfma32(acc, Ar + k0, Bg + (int64_t)k0 * n_out, n_out, 32, lane);
    tile_out<RELU>(acc, bias, ct, Os, ldo, save, n_out, valid, lane);
  }
}

}  // namespace
#endif
