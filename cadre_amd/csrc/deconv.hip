// deconv.hip — the decoder's transposed convolutions for gfx950 (MI355X): ConvTranspose2d(k 3, stride 2, padding 1,
// output_padding (oph, opw)) of the reference's reverse modules (danet_blocks/visual_branch.py:141-163), fp32, dense NHWC.
//
// A stride-2 transposed 3x3 convolution is four ordinary small convolutions, one per output parity class (py, px):
//     out[2m+py][2n+px] = sum over dy <= py, dx <= px of  x[m+dy][n+dx] . w[:, :, ky(py, dy), kx(px, dx)]
// with ky(0, 0) = 1, ky(1, 0) = 2, ky(1, 1) = 0 (output row 2m+1 takes x[m] through kernel row 2 and x[m+1] through kernel
// row 0), the same for columns, and neighbours outside the map contributing nothing: 1, 2, 2 and 4 taps.  No zero-stuffed
// input, no scatter: every output element belongs to one class and one input position, and is written once by one wave.
//
// cadre_deconv3x3_s2 (levels 1-4): each class is an implicit GEMM — rows = the F*H*W input positions, columns = Cout,
// K = taps * Cin — on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains).  Workgroup = 4 waves, tile 128 rows x 32*WN columns
// (wave w owns rows 32w .. 32w+31 and all columns), BK = 32, double-buffered LDS image with the 36-float row pitch of
// gemm_f32.hip (conflict-free ds_read_b128 fragments, the same k permutation on A and B).  A rows are the NHWC pixels
// themselves (position m is row m: byte offset m * Cin * 4), a tap is one wave-uniform delta, a missing neighbour an
// out-of-window offset of the raw buffer load (zero fill, no branch).  The host packs the weights per class as
// [Cout][tap][Cin], so B is a k-contiguous operand whose k-tile kt starts at float 32 * kt.  grid = (tiles, 4 classes, Z
// modules): the segmentation and the route decoder run in one launch, at level 1 from the same input (z stride 0).
//
// cadre_deconv3x3_s2_out (level 5, 32 -> Cout <= 8): a bandwidth kernel on the vector ALU.  One thread per INPUT position
// computes its 2x2 output quad (9 taps, every lane the same work), weights broadcast from LDS, and writes what the caller
// asked for: logits, the u8 argmax map (lowest index wins a tie), the sigmoid (Cout = 1).
//
// cadre_bc_head: the behaviour-cloning head, one fused kernel (see bc_head_kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern thread_local char g_cadre_err[256];
int cadre_fail(const char* msg);

#define DC_BK 32
#define DC_PITCH 36
#define DC_BM 128

struct deconv_args {
  const float* x;
  const float* w;
  const float* scale;
  const float* shift;
  float* out;
  int64_t x_zstride;
  int F, H, W, Cin, Cout, oph, opw, act;
  float slope;
};

template <int WN>
__global__ __launch_bounds__(256, 2) void deconv3x3_s2_kernel(deconv_args p) {
  constexpr int BM = DC_BM, BN = 32 * WN;
  constexpr int RA = BM / 32;          // 16-B chunks per thread per A tile (256 threads = 32 rows x 8 chunks per pass)
  constexpr int RB = BN / 32;
  constexpr unsigned OOB = 0x80000000u;
  __shared__ __attribute__((aligned(16))) float lds[2 * (BM + BN) * DC_PITCH];
  __shared__ int orow[BM];             // element offset of the row's output pixel in this module's output, -1: none
  float* As = lds;
  float* Bs = lds + 2 * BM * DC_PITCH;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int cls = blockIdx.y, py = cls >> 1, px = cls & 1, z = blockIdx.z;
  const int tilesN = (p.Cout + BN - 1) / BN;
  const int m0 = (blockIdx.x / tilesN) * BM, n0 = (blockIdx.x % tilesN) * BN;
  const int M = p.F * p.H * p.W;
  const int Ho = 2 * p.H - 1 + p.oph, Wo = 2 * p.W - 1 + p.opw;
  const int ntap = (1 + py) * (1 + px), nci = p.Cin / DC_BK, nk = ntap * nci;
  const int coff = cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5));       // taps of the classes in front
  const int64_t wcc = (int64_t)p.Cin * p.Cout;
  const float* X = p.x + (int64_t)z * p.x_zstride;
  const float* Wc = p.w + ((int64_t)z * 9 + coff) * wcc;
  float* Out = p.out + (int64_t)z * p.F * Ho * Wo * p.Cout;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (int)((int64_t)M * p.Cin * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Wc, 0, (int)((int64_t)ntap * wcc * 4), 0x00020000);

  if (tid < BM) {
    const int m = m0 + tid;
    int o = -1;
    if (m < M) {
      const int f = m / (p.H * p.W), rem = m - f * (p.H * p.W);
      const int iy = rem / p.W, ix = rem - iy * p.W;
      const int oy = 2 * iy + py, ox = 2 * ix + px;
      if (oy < Ho && ox < Wo) o = ((f * Ho + oy) * Wo + ox) * p.Cout;
    }
    orow[tid] = o;
  }

  const int cc = tid & 7, rr = tid >> 3;
  unsigned aoff[RA], amask[RA], boff[RB];
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    const int m = m0 + rr + 32 * i;
    aoff[i] = OOB;
    amask[i] = 0;
    if (m < M) {
      const int rem = m % (p.H * p.W);
      const int iy = rem / p.W, ix = rem - iy * p.W;
      aoff[i] = (unsigned)((m * p.Cin + cc * 4) * 4);
      for (int dy = 0; dy <= py; ++dy)
        for (int dx = 0; dx <= px; ++dx)
          if (iy + dy < p.H && ix + dx < p.W) amask[i] |= 1u << (dy * (1 + px) + dx);
    }
  }
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int n = n0 + rr + 32 * i;
    boff[i] = n < p.Cout ? (unsigned)((n * ntap * p.Cin + cc * 4) * 4) : OOB;
  }

  f32x4 areg[RA], breg[RB];
  auto ldg = [](const __amdgpu_buffer_rsrc_t& rs, unsigned off) -> f32x4 {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
  };
  auto load_tiles = [&](int kt) {          // kt < nk (wave-uniform)
    const int tap = kt / nci, ci0 = (kt - tap * nci) * DC_BK;
    const int dy = tap / (1 + px), dx = tap - dy * (1 + px);
    const unsigned delta = (unsigned)(((dy * p.W + dx) * p.Cin + ci0) * 4);
    const unsigned bit = 1u << tap;
#pragma unroll
    for (int i = 0; i < RA; ++i) areg[i] = ldg(rsA, (amask[i] & bit) ? aoff[i] + delta : OOB);
    const unsigned kb_ = (unsigned)kt * (DC_BK * 4);
#pragma unroll
    for (int i = 0; i < RB; ++i) breg[i] = ldg(rsB, boff[i] == OOB ? OOB : boff[i] + kb_);
  };
  auto store_tiles = [&](int buf) {
    float* as = As + buf * BM * DC_PITCH;
    float* bs = Bs + buf * BN * DC_PITCH;
#pragma unroll
    for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(as + (rr + 32 * i) * DC_PITCH + cc * 4) = areg[i];
#pragma unroll
    for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(bs + (rr + 32 * i) * DC_PITCH + cc * 4) = breg[i];
  };

  f32x16 acc[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // k-loop: barrier; request tile kt+1 into registers; MFMAs of tile kt from LDS buffer kt&1; write tile kt+1 into the
  // other buffer (its last readers, the MFMAs of tile kt-1, are behind this iteration's barrier)
  load_tiles(0);
  store_tiles(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
    const bool more = kt + 1 < nk;
    if (more) load_tiles(kt + 1);
    const float* as = As + (kt & 1) * BM * DC_PITCH + (wave * 32 + l31) * DC_PITCH;
    const float* bs = Bs + (kt & 1) * BN * DC_PITCH + l31 * DC_PITCH;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const int kq = kb * 8 + lh * 4;       // lane half lh owns k = 8 kb + 4 lh + s of the step (A and B alike)
      const f32x4 af = *reinterpret_cast<const f32x4*>(as + kq);
      f32x4 bf[WN];
#pragma unroll
      for (int j = 0; j < WN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(bs + j * 32 * DC_PITCH + kq);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[j][s], acc[j], 0, 0, 0);
    }
    if (more) store_tiles((kt + 1) & 1);
  }

  // epilogue: accumulator register r of lane (l31, lh) is row (r & 3) + 8 (r >> 2) + 4 lh, column l31 of the 32 x 32 tile:
  // one store instruction writes two rows of 32 consecutive channels (128 B each)
  const float* scale = p.scale + (int64_t)z * p.Cout;
  const float* shift = p.shift + (int64_t)z * p.Cout;
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int col = n0 + j * 32 + l31;
    if (col >= p.Cout) continue;
    const float sc = scale[col], sh = shift[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = orow[wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
      if (o < 0) continue;
      float v = acc[j][r] * sc + sh;
      if (p.act == 1) v = fmaxf(v, 0.f);
      else if (p.act == 2) v = v > 0.f ? v : v * p.slope;
      Out[o + col] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- level 5: 32 -> Cout <= 8
#define DO_CIN 32

template <int CO>
__global__ __launch_bounds__(256) void deconv3x3_s2_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* logits, uint8_t* cls,
                                                               float* sig, int F, int H, int W, int Cout, int oph, int opw) {
  __shared__ __attribute__((aligned(16))) float ws[9 * DO_CIN * CO];      // [ky][kx][ci][CO], zero past Cout
  for (int i = threadIdx.x; i < 9 * DO_CIN * CO; i += 256) ws[i] = w[i];
  __syncthreads();
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= F * H * W) return;
  const int f = pos / (H * W), rem = pos - f * (H * W);
  const int iy = rem / W, ix = rem - iy * W;
  const bool right = ix + 1 < W, down = iy + 1 < H;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4* x00 = reinterpret_cast<const f32x4*>(x + (int64_t)pos * DO_CIN);
  const f32x4* x01 = x00 + DO_CIN / 4;
  const f32x4* x10 = x00 + W * (DO_CIN / 4);
  const f32x4* x11 = x10 + DO_CIN / 4;
  float a00[CO], a01[CO], a10[CO], a11[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) a00[c] = a01[c] = a10[c] = a11[c] = 0.f;
  auto wt = [&](int ky, int kx, int ci) { return ws + ((ky * 3 + kx) * DO_CIN + ci) * CO; };
#pragma unroll 1
  for (int c4 = 0; c4 < DO_CIN / 4; ++c4) {
    const f32x4 v00 = x00[c4];
    const f32x4 v01 = right ? x01[c4] : zero;
    const f32x4 v10 = down ? x10[c4] : zero;
    const f32x4 v11 = (right && down) ? x11[c4] : zero;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ci = c4 * 4 + e;
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        a00[c] = fmaf(v00[e], wt(1, 1, ci)[c], a00[c]);
        a01[c] = fmaf(v00[e], wt(1, 2, ci)[c], a01[c]);
        a01[c] = fmaf(v01[e], wt(1, 0, ci)[c], a01[c]);
        a10[c] = fmaf(v00[e], wt(2, 1, ci)[c], a10[c]);
        a10[c] = fmaf(v10[e], wt(0, 1, ci)[c], a10[c]);
        a11[c] = fmaf(v00[e], wt(2, 2, ci)[c], a11[c]);
        a11[c] = fmaf(v01[e], wt(2, 0, ci)[c], a11[c]);
        a11[c] = fmaf(v10[e], wt(0, 2, ci)[c], a11[c]);
        a11[c] = fmaf(v11[e], wt(0, 0, ci)[c], a11[c]);
      }
    }
  }
  const int Ho = 2 * H - 1 + oph, Wo = 2 * W - 1 + opw;
  auto emit = [&](const float* a, int oy, int ox) {
    if (oy >= Ho || ox >= Wo) return;
    const int64_t o = ((int64_t)f * Ho + oy) * Wo + ox;
    float v[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) v[c] = c < Cout ? a[c] + bias[c] : 0.f;
    if (logits) {
#pragma unroll
      for (int c = 0; c < CO; ++c)
        if (c < Cout) logits[o * Cout + c] = v[c];
    }
    if (cls) {
      int best = 0;
      float bv = v[0];
#pragma unroll
      for (int c = 1; c < CO; ++c)
        if (c < Cout && v[c] > bv) { bv = v[c]; best = c; }
      cls[o] = (uint8_t)best;
    }
    if (sig) {        // e = exp(-|v|) in (0, 1]: 1 / (1 + e) for v >= 0, e / (1 + e) below
      const float e = expf(-fabsf(v[0]));
      sig[o] = (v[0] >= 0.f ? 1.f : e) / (1.f + e);
    }
  };
  emit(a00, 2 * iy, 2 * ix);
  emit(a01, 2 * iy, 2 * ix + 1);
  emit(a10, 2 * iy + 1, 2 * ix);
  emit(a11, 2 * iy + 1, 2 * ix + 1);
}

// first maximum of each row (the reference's torch.max over the light-state logits, danet.py:355)
__global__ void argmax_rows_kernel(const float* x, int64_t ld, int rows, int n, int32_t* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* row = x + (int64_t)r * ld;
  int best = 0;
  float bv = row[0];
  for (int c = 1; c < n; ++c)
    if (row[c] > bv) { bv = row[c]; best = c; }
  out[r] = best;
}

// The behaviour-cloning head (danet.py:176-181, bc_branch.py:56-61) for one latent row per workgroup: att_bc = latent[256:512]
// (+ in_bc_speed_fc(speed): Linear 1 -> 64, leaky, Linear 64 -> 256), then Linear 256 -> 128, leaky, Linear 128 -> 2.  50 k
// multiply-adds per row: too small for the tiled GEMM (M = F rows of a 128-row tile, K = 1 .. 256), so one fused kernel.  Every
// layer's output is an fp32 value as in the reference; the sums inside a layer run in double (free at this size), so each
// layer owes one rounding instead of a K-long chain's.
__global__ __launch_bounds__(256) void bc_head_kernel(const float* __restrict__ lat, int64_t ld, const float* __restrict__ speed,
                                                      const float* __restrict__ sw1, const float* __restrict__ sb1,
                                                      const float* __restrict__ sw2, const float* __restrict__ sb2,
                                                      const float* __restrict__ bw1, const float* __restrict__ bb1,
                                                      const float* __restrict__ bw2, const float* __restrict__ bb2, float* out, float slope) {
  __shared__ float s1[64], att[256], h[128];
  const int f = blockIdx.x, t = threadIdx.x;
  auto leaky = [slope](float v) { return v > 0.f ? v : v * slope; };
  if (speed && t < 64) s1[t] = leaky((float)((double)speed[f] * sw1[t] + sb1[t]));
  __syncthreads();
  float a = lat[(int64_t)f * ld + 256 + t];
  if (speed) {
    double acc = sb2[t];
    for (int j = 0; j < 64; ++j) acc += (double)sw2[t * 64 + j] * s1[j];
    a += (float)acc;
  }
  att[t] = a;
  __syncthreads();
  if (t < 128) {
    double acc = bb1[t];
    for (int i = 0; i < 256; ++i) acc += (double)bw1[t * 256 + i] * att[i];
    h[t] = leaky((float)acc);
  }
  __syncthreads();
  if (t < 2) {
    double acc = bb2[t];
    for (int i = 0; i < 128; ++i) acc += (double)bw2[t * 128 + i] * h[i];
    out[(int64_t)f * 2 + t] = (float)acc;
  }
}

// ---------------------------------------------------------------------------------------------- C ABI
static bool deconv_shape_ok(int64_t Z, int64_t F, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int oph, int opw) {
  if (Z < 1 || F < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || oph < 0 || oph > 1 || opw < 0 || opw > 1) return false;
  const int64_t lim = 1ll << 31;
  // (factor by factor: the product of four 31-bit values does not fit 64 bits)
  if (Z >= lim || F >= lim || H >= lim || W >= lim || Cin >= lim || Cout >= lim) return false;
  const int64_t Ho = 2 * H - 1 + oph, Wo = 2 * W - 1 + opw;
  auto below = [&](int64_t a, int64_t b, int64_t c, int64_t d, int64_t e) {       // a b c d e * 4 bytes < 2 GiB
    int64_t v = 4;
    for (int64_t t : {a, b, c, d, e}) {
      if (v * t >= lim) return false;       // v < 2^31 and t < 2^31: no overflow
      v *= t;
    }
    return true;
  };
  return below(Z, F, H, W, Cin) && below(Z, F, Ho, Wo, Cout) && below(Z, 9, Cin, Cout, 1);
}

extern "C" int cadre_deconv3x3_s2_supported(int32_t Z, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                            int32_t oph, int32_t opw) {
  return (Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0 && deconv_shape_ok(Z, F, H, W, Cin, Cout, oph, opw)) ? 1 : 0;
}

extern "C" int cadre_deconv3x3_s2(const float* x, int64_t x_zstride, const float* w, const float* scale, const float* shift,
                                  float* out, int32_t Z, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                  int32_t oph, int32_t opw, int32_t act, float slope, void* stream) {
  if (!x || !w || !scale || !shift || !out) return cadre_fail("cadre_deconv3x3_s2: null pointer");
  if (!cadre_deconv3x3_s2_supported(Z, F, H, W, Cin, Cout, oph, opw))
    return cadre_fail("cadre_deconv3x3_s2: needs Cin % 32 == 0, Cout % 32 == 0, output padding 0 / 1 and every tensor below 2 GiB");
  if (act < 0 || act > 2) return cadre_fail("cadre_deconv3x3_s2: act must be 0 (none), 1 (ReLU) or 2 (leaky ReLU)");
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || (x_zstride & 3)) return cadre_fail("cadre_deconv3x3_s2: x and w must be 16-byte aligned, x_zstride % 4 == 0");
  if (x_zstride != 0 && x_zstride < (int64_t)F * H * W * Cin) return cadre_fail("cadre_deconv3x3_s2: x_zstride must be 0 or at least F*H*W*Cin");
  deconv_args p;
  p.x = x; p.w = w; p.scale = scale; p.shift = shift; p.out = out; p.x_zstride = x_zstride;
  p.F = F; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.oph = oph; p.opw = opw; p.act = act; p.slope = slope;
  const int M = F * H * W, tilesM = (M + DC_BM - 1) / DC_BM;
  hipStream_t st = (hipStream_t)stream;
  if (Cout % 64 == 0) hipLaunchKernelGGL((deconv3x3_s2_kernel<2>), dim3(tilesM * (Cout / 64), 4, Z), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((deconv3x3_s2_kernel<1>), dim3(tilesM * (Cout / 32), 4, Z), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

extern "C" int cadre_deconv3x3_s2_out(const float* x, const float* w, const float* bias, float* logits, uint8_t* cls, float* sig,
                                      int32_t F, int32_t H, int32_t W, int32_t Cout, int32_t oph, int32_t opw, void* stream) {
  if (!x || !w || !bias) return cadre_fail("cadre_deconv3x3_s2_out: null pointer");
  if (!logits && !cls && !sig) return cadre_fail("cadre_deconv3x3_s2_out: no output wanted");
  if (Cout < 1 || Cout > 8) return cadre_fail("cadre_deconv3x3_s2_out: 1 <= Cout <= 8");
  if (sig && Cout != 1) return cadre_fail("cadre_deconv3x3_s2_out: the sigmoid output needs Cout == 1");
  if (!deconv_shape_ok(1, F, H, W, DO_CIN, Cout, oph, opw)) return cadre_fail("cadre_deconv3x3_s2_out: bad shape, or a tensor of 2 GiB or more");
  if ((uintptr_t)x & 15) return cadre_fail("cadre_deconv3x3_s2_out: x must be 16-byte aligned");
  const int blocks = (F * H * W + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
#define DO_LAUNCH(CO_) hipLaunchKernelGGL((deconv3x3_s2_out_kernel<CO_>), dim3(blocks), dim3(256), 0, st, x, w, bias, logits, cls, sig, F, H, W, Cout, oph, opw)
  if (Cout == 1) DO_LAUNCH(1);
  else if (Cout == 2) DO_LAUNCH(2);
  else if (Cout <= 4) DO_LAUNCH(4);
  else DO_LAUNCH(8);
#undef DO_LAUNCH
  return (int)hipGetLastError();
}

extern "C" int cadre_argmax_rows(const float* x, int64_t ld, int32_t rows, int32_t n, int32_t* out, void* stream) {
  if (!x || !out) return cadre_fail("cadre_argmax_rows: null pointer");
  if (rows < 1 || n < 1 || ld < n) return cadre_fail("cadre_argmax_rows: needs rows >= 1, 1 <= n <= ld");
  hipLaunchKernelGGL(argmax_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, ld, rows, n, out);
  return (int)hipGetLastError();
}

extern "C" int cadre_bc_head(const float* lat, int64_t ld, const float* speed, const float* sw1, const float* sb1, const float* sw2,
                             const float* sb2, const float* bw1, const float* bb1, const float* bw2, const float* bb2, float* out,
                             int32_t F, float slope, void* stream) {
  if (!lat || !sw1 || !sb1 || !sw2 || !sb2 || !bw1 || !bb1 || !bw2 || !bb2 || !out) return cadre_fail("cadre_bc_head: null pointer");
  if (F < 1 || ld < 512) return cadre_fail("cadre_bc_head: needs F >= 1 rows of at least 512 floats");
  hipLaunchKernelGGL(bc_head_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, lat, ld, speed, sw1, sb1, sw2, sb2, bw1, bb1, bw2, bb2, out, slope);
  return (int)hipGetLastError();
}
