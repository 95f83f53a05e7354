/*
 * cadre_hip.h — C ABI of libcadre_hip.so, the MI355X (gfx950) kernels behind the Cadre PPO
 * learner hot path.  Plain pointers + sizes + a hipStream_t (passed as void*),
 * int status return (0 = ok, <0 = bad argument, >0 = hipError_t), never throws, never owns
 * caller memory, no torch types.  All pointers are DEVICE pointers unless noted.
 *
 * The reference (BIT-MCS/Cadre) is pure Python; the "FFI" a maintainer binds is ctypes
 * (see INTEGRATION.md).  Each entry point cites the reference code it replaces
 * (paths relative to /root/reference).
 */
#ifndef CADRE_HIP_H
#define CADRE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CADRE_ABI_VERSION 15
int cadre_abi_version(void);
/* human-readable last argument error of the calling thread ("" if none) */
const char* cadre_last_error(void);

/* ---------------------------------------------------------------- generic tiled GEMM / conv
 * C[z][M,N] = act( (sum_k A(m,k) B(n,k)) * scale[n] + shift[n] + resid[m,n] )
 * on v_mfma_f32_32x32x2_f32 (exact f32 fma chain).  Replaces every nn.Linear / nn.Conv2d /
 * nn.LSTMCell matmul on the path: carla_perception/Networks/danet_blocks/resnet.py:111-181,
 * danet.py:21-41,96,108, intertask_att.py:39-80, ppo_agent/models.py:130-177,
 * ppo_agent/distributions.py:34-40 (forward) and their autograd backward (dX, dW).
 */
typedef struct {
  const float* A;      /* a_mode 0: [M][lda] (k contiguous); 1: [K][lda] (m contiguous);
                          2: NHWC activation, implicit-GEMM conv gather (Cin%32==0);
                          3: NHWC4 activation (Cin==4 stem), k-tile = one kernel row:
                             K = KH*32, B rows laid out [KH][32] with zeros past KW*4       */
  const float* B;      /* b_mode 0: [N][ldb] (k contiguous); 1: [K][ldb] (n contiguous)  */
  float* C;            /* [M][ldc] row-major (== NHWC for convs)                         */
  const float* scale;  /* per-n multiplier or NULL (=1)   (folded eval BatchNorm)        */
  const float* shift;  /* per-n addend or NULL (=0)       (bias / folded BN)             */
  const float* resid;  /* [M][ldr] added before the activation, or NULL; may alias C     */
  int64_t lda, ldb, ldc, ldr;
  int32_t M, N, K;
  int32_t a_mode, b_mode;
  int32_t act;         /* 0 none, 1 ReLU, 2 LeakyReLU(slope); |16: add resid AFTER the act   */
  float slope;
  /* batch (grid.z): operand offset = ((z / div) % mod) * stride elements                */
  int32_t batch;
  int32_t a_div, a_mod, b_div, b_mod, c_div, c_mod, s_div, s_mod, r_div, r_mod;
  int64_t a_str, b_str, c_str, s_str, r_str;
  /* conv geometry (a_mode 2/3): input [Nimg][H][W][Cin], output [Nimg][Ho][Wo][N]       */
  int32_t H, W, Cin, Ho, Wo, KH, KW, stride, pad;
  /* split-K: >1 writes raw partial sums, slice s to `C + s*M*ldc` (batch 1) or to
     `C + s*slots*c_str + z-offset` (batched; slots = distinct C z-slots); finish with
     cadre_splitk_reduce.  With split_k>1 scale/shift/resid/act are ignored here.        */
  int32_t split_k;
  int32_t tile;        /* 0 auto, 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 256x128,
                          5 = 128x256, 6 = 256x64 (4-6: one workgroup per CU);
                          7 = 256x256 on 8 waves (cadre_gemm_bf16 only);
                          8 = 128x128 on 8 waves, 9 = 32x128 on 4 waves (row-sorted
                          minibatches: skips in 32-row steps), 10 = 128x64 on 8 waves
                          (8, 9: cadre_gemm_f32 only; 10 also cadre_gemm_bf16, which adds
                          11 = 256x64 on 8 waves).  Tiles 11 (fp32) / 12 exist only in the A/B
                          build (include/cadre_hip_ab.h)                                    */
  int32_t flags;       /* bit 1: C is bf16; bit 2: resid is bf16 (cadre_gemm_bf16; bit 1 also
                          honoured by cadre_gemm_f32's vector epilogue); others must be 0   */
  /* Row segments (cadre_gemm_f32 only; PPO update with the minibatch rows sorted by command,
     agent.py:170-182 evaluates every command net on every row and masks 3 of 4): batch entry z
     owns rows [row_seg[2*(z/seg_div)], +row_seg[2*(z/seg_div)+1]) of every period of
     `seg_period` rows.  seg_modes 1 and 2 skip in tiles and need seg_period % 32 == 0 (mode 1: the
     M tile must divide the period — 32- or 64-row tiles, chosen by the library where the requested
     tile does not); seg_mode 3 takes ANY seg_period >= 1 (the act path's period is the number of
     environments) and needs only M % seg_period == 0.
     seg_mode 1: M-tiles that own no row of their period return without writing; seg_mode 2: k-tiles (k = row index, K % seg_period == 0) outside the segment are
     not multiplied.  Rows of other nets inside a computed tile are still multiplied — callers
     keep their gradients exactly zero (cadre_relu_bwd / cadre_lstm_pointwise_bwd masks).
     seg_mode 3 (NT products, no split-K / residual): the M index runs over the entry's OWN rows
     only, period after period (compact row mc = row (mc / cnt) * seg_period + beg + mc % cnt
     of A and C): no row of another net is read, multiplied or written, whatever the run's
     alignment (the LSTM input projection of the update: [S*B] rows, period B).              */
  int32_t seg_mode;    /* 0 off                                                               */
  const int32_t* row_seg;
  int32_t seg_period, seg_div;
} cadre_gemm_t;
int cadre_gemm_f32(const cadre_gemm_t* p, void* stream);
/* the tile id cadre_gemm_f32 would use for this descriptor (p->tile, or the auto choice) */
int cadre_gemm_pick_tile(const cadre_gemm_t* p);
/* Same contract with bf16 A/B operands (element counts/strides in bf16 elements), fp32
 * accumulation on v_mfma_f32_32x32x16_bf16 and an fp32 epilogue; a_mode 0, 2 (Cin%64==0) or
 * 4 (Cin==4 stem on a zero-padded NHWC4 image: H, W = padded sizes, pad = 0, K = ceil(KH/2)*64,
 * B rows [ceil(KH/2)][64] = two kernel rows of 8 pixels x 4 channels, zeros elsewhere), b_mode 0; C bf16 or f32 (flags bit 1), resid bf16 or f32 (flags bit 2).  BASELINE config C3
 * ("bf16 encoder / fp32 losses"). */
int cadre_gemm_bf16(const cadre_gemm_t* p, void* stream);
/* tile id cadre_gemm_bf16 would launch for this descriptor (host logic, no launch) */
int cadre_gemm_bf16_pick_tile(const cadre_gemm_t* p);
/* 3x3 / stride 1 / pad 1 convolution on dense NHWC (resnet.py:26-55 conv1/conv2, danet.py:21-41 conv5a/5c/51/52):
 * x [F][H][W][Cin], w [N][NC][9][128 B] (NC = Cin*elem/128 channel chunks; chunk-major, tap = kh*3+kw, then the
 * chunk's channels), y = act(conv*scale[n] + shift[n] (+ resid)) (+ resid after act when act & 16), out [F*H*W][N].
 * flags bit 0: bf16 operands (else fp32); bit 1: out bf16; bit 2: resid bf16.  Each input pixel goes through LDS once
 * per channel chunk (conv3x3_ring.hip).  cadre_conv3x3_ring_supported: host logic, no launch; it takes the same flags
 * word plus 8 = a residual is present and bounds every tensor (< 2 GiB: 32-bit buffer offsets) at its own element size,
 * so a 1 from it means cadre_conv3x3_ring with those flags does not fail on geometry. */
int cadre_conv3x3_ring(const void* x, const void* w, const float* scale, const float* shift, const void* resid,
                       void* out, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N, int32_t act,
                       int32_t flags, void* stream);
int cadre_conv3x3_ring_supported(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N, int32_t flags);
/* tile configuration as ntile (64 / 128) + 1000 * WVM (waves along the positions: 4 = 256-position tile on 8 waves, one
 * workgroup per CU) + 100000 when an 8-wave ping-pong kernel runs + 1000000 * G when it is the G-k-tiles-per-slot form
 * (bf16): names the instantiation conv3x3_ring_kernel<bf16, ntile, res, out_bf16, WVM> /
 * conv3x3_ring_pp_kernel<bf16, ntile, res, out_bf16, false> / conv3x3_ring_pp2_kernel<ntile, res, out_bf16, G> */
int cadre_conv3x3_ring_ntile(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N, int32_t bf16);
/* 3x3 / STRIDE 2 / pad 1 convolution on dense bf16 NHWC (resnet.py:26-55 conv1 of layer2.0 / layer3.0 / layer4.0, stride 2:
 * resnet.py:152-158), bf16 model: x [F][H][W][Cin] with even H, W; w [N][Cin/64][9][64] with the nine taps of a 64-channel
 * chunk in PLANE order (kh,kw) = (0,0) (0,2) (2,0) (2,2) (1,0) (1,2) (0,1) (2,1) (1,1); y = act(conv + shift[n]) as bf16
 * [F*(H/2)*(W/2)][N]; scale must be NULL (the caller folds the BN scale into the weight rows: the kernel starts its sums at
 * the shift and has no epilogue multiply); act 0 / 1 (ReLU).  The input is staged as four parity planes in LDS, each pixel once per (M tile,
 * channel chunk, N tile) instead of once per tap (conv3x3_s2.hip).  cadre_conv3x3_s2_supported: host logic, no launch. */
int cadre_conv3x3_s2(const void* x, const void* w, const float* scale, const float* shift, void* out, int32_t F, int32_t H,
                     int32_t W, int32_t Cin, int32_t N, int32_t act, void* stream);
int cadre_conv3x3_s2_supported(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N);
/* Second conv of a down-sampling BasicBlock with the block's shortcut folded in (resnet.py:40-55 with downsample = resnet.py:152-158),
 * bf16 model: out = act( conv3x3_s1_p1(x; W2) + conv1x1_s2(x2; Wd) + shift[n] ) as bf16 [F*H*W][N], one fp32 accumulation —
 * x [F][H][W][C1], x2 [F][2H][2W][Cd] (the shortcut reads pixel (2h, 2w)), both folded-BN scales already in the weight rows,
 * shift = shift2 + shift_d.  w [N][9*C1/64 + Cd/64][64]: per 64-channel chunk c of C1 the nine taps kh*3+kw of W2, then (c < Cd/64)
 * chunk c of Wd (cadre_amd/encoder.py _s1x_w).  Needs Cd <= C1.  conv3x3_s1x.hip; _supported: host logic, no launch. */
int cadre_conv3x3_s1x(const void* x, const void* x2, const void* w, const float* shift, void* out, int32_t F, int32_t H, int32_t W,
                      int32_t C1, int32_t Cd, int32_t N, int32_t act, void* stream);
int cadre_conv3x3_s1x_supported(int32_t F, int32_t H, int32_t W, int32_t C1, int32_t Cd, int32_t N);
/* weight stages of the launch at this map width / channel count (2, or 3 under CADRE_S1X_STAGES=3 where they fit): the second
 * template argument of conv3x3_s1x_kernel<nps, stages> */
int cadre_conv3x3_s1x_stages(int32_t W, int32_t N);
/* Dense bf16 NT product with split-K into raw fp32 partial sums (the inter-task attention's first layers, intertask_att.py:39-80, bf16
 * model): slab[s][M][ldc] = A[M][k in slice s] . B[N][k in slice s]^T, slice s = 64-element k-tiles [s * per, (s + 1) * per), per =
 * ceil(K / 64 / split_k) — the slices, the k order and therefore every partial sum of cadre_gemm_bf16 with split_k (reduce with
 * cadre_splitk_reduce).  A [M][lda] bf16; B in FRAGMENT order [N/128][K/16][4 blocks of 32 columns][64 lanes][8]: lane (l31, lh) of
 * block cb of 16-element k-step q holds B[128 g + 32 cb + l31][16 q + 8 lh .. + 7] (cadre_amd/encoder.py _w128_dense_b) — it goes from
 * memory straight to the matrix cores' operand registers, only A is staged in LDS (gemm_bf16_w128.hip).  N % 256 == 0, K % 64 == 0.
 * _supported: host logic, no launch. */
int cadre_gemm_bf16_w128(const void* A, const void* B, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldc,
                         int32_t split_k, void* stream);
int cadre_gemm_bf16_w128_supported(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldc, int32_t split_k);
/* Sustained matrix-pipe rate of this device (peaks.hip; SURVEY.md 8d asks for the measured peak next to the datasheet
 * one): workgroups x 4 waves, each iters x 8 register-operand MFMAs on independent accumulators (fp32:
 * v_mfma_f32_32x32x2_f32 = 4096 FLOP, bf16: v_mfma_f32_32x32x16_bf16 = 32768 FLOP).  The caller times the launch. */
int cadre_mfma_peak(int32_t bf16, int32_t workgroups, int32_t iters, float* sink, void* stream);
/* bf16 MFMA shape comparison on pseudo-random register operands (peaks.hip): shape 32 = v_mfma_f32_32x32x16_bf16,
 * shape 16 = v_mfma_f32_16x16x32_bf16; 262144 FLOP per wave and iteration either way; workgroups x 4 waves.
 * shape 2 = v_mfma_f32_32x32x2_f32, shape 4 = v_mfma_f32_16x16x4_f32 on random fp32 operands: 8 x 4096 / 32 x 2048 FLOP per wave and iteration. */
int cadre_mfma_shape(int32_t shape, int32_t workgroups, int32_t iters, float* sink, void* stream);
/* HBM stream peaks of this device (peaks.hip): mode 0 reads `bytes` from src with 16-B loads, 8 in flight per lane
 * (nothing stored), mode 1 copies src -> dst.  The caller times the launch (read: bytes / t, copy: 2 * bytes / t). */
int cadre_hbm_stream(int32_t mode, const void* src, void* dst, int64_t bytes, float* sink, void* stream);
/* C[M][ldc] = act(sum_s slab[s][M][lds] * scale + shift + resid) */
int cadre_splitk_reduce(const float* slabs, int32_t split_k, int64_t slab_stride, int64_t lds,
                        float* C, int64_t ldc, int32_t M, int32_t N, const float* scale,
                        const float* shift, int32_t act, float slope, const int32_t* row_seg, int32_t period,
                        void* stream);
/* (row_seg != NULL: the M rows are [batch][period] sorted by command, row_seg [batch][2]; only the rows of the 32-row
 * tiles of each batch entry's run — the ones a seg_mode 1 GEMM wrote — are reduced, the others left as they are.) */

/* ---------------------------------------------------------------- encoder pieces
 * pre_process: ppo_agent/agent.py:43-75.  rgb u8 [F][H][W][3], route u8 [F][W][H] (stored
 * transposed like the reference) -> out f32 NHWC [F][H][W][4].  rgb/255 via the 256-entry
 * LUT `lut255` (host computes float32(i/255.) in double, bit-exact with agent.py:46).
 * Route quirk agent.py:51-54: per-frame max, value stored back into uint8 -> {0,1}.
 * `route_norm` (u8 [F][W][H], may be NULL) receives the mutated route the reference leaves
 * in the caller's dict.  `frame_max` is u32 [F] scratch. */
int cadre_preprocess(const uint8_t* rgb, const uint8_t* route, const float* lut255,
                     float* out, uint8_t* route_norm, uint32_t* frame_max,
                     int32_t F, int32_t H, int32_t W, void* stream);
/* Same conversion into the interior (pad_t, pad_l) of a zero-padded bf16 NHWC4 image
 * [F][Hp][Wp][4] whose border the caller keeps zero: input of the bf16 stem (cadre_gemm_bf16
 * a_mode 4), which then needs no halo masks. */
int cadre_preprocess_bf16pad(const uint8_t* rgb, const uint8_t* route, const float* lut255, void* out,
                             uint8_t* route_norm, uint32_t* frame_max, int32_t F, int32_t H, int32_t W,
                             int32_t Hp, int32_t Wp, int32_t pad_t, int32_t pad_l, void* stream);
/* The same pre_process as ONE packed dword per pixel for the fused front (cadre_stem_pool):
 * out u32 [F][H][W] = R | G<<8 | B<<16 | route<<24, the normalised route {0,1} stored as byte 0 / 255 so
 * that every byte takes the same /255 conversion (255/255 == 1.0f exactly).  route_norm / frame_max as above.
 * frame_idx (i64 [F], may be NULL): output frame f is source frame frame_idx[f] — the sliding 8-frame windows of
 * train.py:50-75 repeat each camera frame 8 times, the gather rides on the packing pass. */
int cadre_pack_obs(const uint8_t* rgb, const uint8_t* route, uint32_t* out, uint8_t* route_norm,
                   uint32_t* frame_max, int32_t F, int32_t H, int32_t W, const int64_t* frame_idx, int32_t n_src,
                   void* stream);
/* (with frame_idx the route maxima are taken once per SOURCE frame: n_src = number of frames in rgb / route, frame_max
 * u32 scratch of n_src entries; without it n_src is ignored and frame_max holds F entries.) */
/* Fused encoder front: packed observation -> /255 -> conv1 7x7/s2/p3 (4 -> 64) + folded BN + ReLU ->
 * MaxPool2d(3,2,1)  (agent.py:46, resnet.py:111-115,168-172) in one kernel; the stem map never reaches HBM.
 * wt: tap-major weights [64][taps][4]; fp32: tap = ky*7 + kx, 50 taps (one zero tap), BN scale in `scale`;
 *     bf16: tap = ky*8 + kx, 56 taps (kx = 7: zeros), ALREADY multiplied by the BN scale and `scale` = NULL
 *     (the kernel starts its sums at the shift).
 * out: pooled map, element (f, p, c, ch) at out_off + f*out_frame + p*out_row + c*out_px + ch (f32, or bf16 when
 * bf16 == 1, which also selects bf16 MFMA).  bf16 == 2: the fp32 front (fp32 `scale`, fp32 out) computed on the bf16 matrix cores
 * with exact products — wt = [3 pieces][64][216] bf16 with piece1 + piece2 + piece3 == the fp32 weight exactly, k = tap*4 + channel,
 * tap = ky*7 + kx, zeros past tap 48; pixel bytes are exact in bf16, sums are fp32.  Geometries: cadre_stem_pool_supported(H, W)
 * (host logic). */
int cadre_stem_pool(const uint32_t* img, const void* wt, const float* scale, const float* shift,
                    void* out, int32_t F, int32_t H, int32_t W, int32_t bf16,
                    int64_t out_frame, int64_t out_row, int32_t out_px, int64_t out_off, void* stream);
int cadre_stem_pool_supported(int32_t H, int32_t W);

/* FUSED Winograd F(2x2, 3x3) for 64 -> 64 stride-1 / pad-1 3x3 convs in fp32 (csrc/winograd_c64.hip; the fp32 model's layer1,
 * resnet.py:26-55): input transform, 16 plane products and inverse transform in one kernel, nothing of the transform
 * domain leaves the CU.  U: the transformed weights (G g G^T)[xi][cout][cin] laid out [8 chunks of 8 cin][16 planes][64 positions][8],
 * position 16 b + n = output channel 4 n + b, cin of chunk 2d + e at index 2q + s = input channel 16 d + 4 q + 2 e + s
 * (cadre_amd/encoder.py _winograd_u_c64).  out = act(conv * scale + shift (+ resid)), act 0 none / 1 ReLU; x, resid, out
 * [F][H][W][64] below 2 GiB. */
int cadre_winograd_c64(const float* x, const float* U, const float* scale, const float* shift, const float* resid, float* out,
                       int32_t F, int32_t H, int32_t W, int32_t act, void* stream);

/* Winograd F(m x m, 3x3) transforms, m = 2, 3 or 4, fp32, NHWC (csrc/winograd.hip).  A stride-1 / pad-1 3x3 convolution
 * (resnet.py:26-55) = cadre_winograd_in -> ONE cadre_gemm_f32 with batch (m+2)^2 (M[xi] = V[xi] . U[xi]^T,
 * U[xi][cout][cin] = (G g G^T)[xi] prepared by the host; Cook-Toom points 0, 1, -1, inf (m = 2) / 0, 3/4, -3/4, 2, inf (m = 3) /
 * 0, +-3/4, +-3/2, inf (m = 4):
 * cadre_amd/encoder.py _WINO_G) -> cadre_winograd_out.
 * T = F * ceil(H/m) * ceil(W/m) tiles.  V: [(m+2)^2][T][C], Mx: [(m+2)^2][T][N], x / resid / out: [F][H][W][C or N].
 * out = act(M . scale + shift (+ resid)) with cadre_gemm_t's act codes (0 none, 1 ReLU, bit 4: residual after act). */
int cadre_winograd_in(const float* x, float* V, int32_t F, int32_t H, int32_t W, int32_t C, int32_t m, void* stream);
int cadre_winograd_out(const float* Mx, const float* scale, const float* shift, const float* resid, float* out,
                       int32_t F, int32_t H, int32_t W, int32_t N, int32_t act, int32_t m, void* stream);
/* Winograd F(m x m, 3x3), m = 2, 3 or 4, fp32, with the plane products and the inverse transform in ONE kernel (csrc/winograd_fused.hip;
 * the stride-1 / pad-1 3x3 convs of resnet.py:26-55 and danet.py:21-41 with >= 128 channels): the (m+2)^2 product planes M never
 * reach HBM.  cadre_winograd_in_frag writes V = B^T d B in MFMA-fragment order [(m+2)^2][C/16][Tpad/16][4 kk][16 tiles][4]
 * (channel 16 c + 4 kk + e of tile 16 tb + t at float ((((xi * C/16 + c) * Tpad/16 + tb) * 4 + kk) * 16 + t) * 4 + e; Tpad = T rounded up
 * to 64; cadre_winograd_frag_elems floats); cadre_winograd_gemm_out multiplies every plane by U — (G g G^T)[xi][cout][cin] packed
 * [N/32][C/16][(m+2)^2][2 nb][4 kk][16 couts][4] (cadre_amd/encoder.py _winograd_u_frag) — and stores
 * out = act(A^T M A * scale + shift (+ resid)), act as in cadre_winograd_out.  The kernels take m 2..4, C % 32 == 0, N % 32 == 0, every
 * tensor below 2 GiB; cadre_winograd_fused_capable says so; cadre_winograd_fused_supported is the encoder's dispatch question — capability AND policy (default: m == 4, where
 * the fused form measured faster; CADRE_WINOGRAD_FUSED=2: every geometry the kernels take, 0: never). */
int cadre_winograd_fused_supported(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N, int32_t m);
int cadre_winograd_fused_capable(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N, int32_t m);
/* tile blocks per workgroup of the cadre_winograd_gemm_out launch for T tiles x N channels: 4 (items of 64 tiles) or 1 (few tiles: items
 * of 16 tiles on 128-thread workgroups) — the same bits either way; wino_gemm_out_kernel<m, NTB> */
int cadre_winograd_fused_ntb(int32_t T, int32_t N);
int64_t cadre_winograd_frag_elems(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t m);
int cadre_winograd_in_frag(const float* x, float* V, int32_t F, int32_t H, int32_t W, int32_t C, int32_t m, void* stream);
int cadre_winograd_gemm_out(const float* V, const float* U, const float* scale, const float* shift, const float* resid, float* out,
                            int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t N, int32_t act, int32_t m, void* stream);
/* The fused front converts bytes arithmetically (fma(x, r_hi, x * r_lo), r_hi + r_lo = 1/255 split in two floats) instead of through the
 * table: counts, into *mismatches (device int32), the i in 0..255 for which that differs from lut255[i]; must be 0. */
int cadre_div255_selfcheck(const float* lut255, int32_t* mismatches, void* stream);
/* nn.MaxPool2d(3,2,1) resnet.py:114 on NHWC [F][H][W][C] (C%4==0) -> [F][Ho][Wo][C] */
int cadre_maxpool3x3s2(const float* x, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                       void* stream);
/* bf16 NHWC variant of cadre_maxpool3x3s2 (C%8==0) */
int cadre_maxpool3x3s2_bf16(const void* x, void* y, int32_t F, int32_t H, int32_t W, int32_t C,
                            void* stream);
/* PAM_Module.forward da_att.py:32-51 after the three 1x1 convs: qkv [F][Np][160] =
 * (query 16 | key 16 | value 128) comes from ONE cadre_gemm_f32 over the concatenated
 * query/key/value conv weights; this kernel does energy = q.k^T, row softmax,
 * out = att.v, y = gamma*out + x on NHWC x [F][Np][128].  Np <= 128: one workgroup per frame (the attention matrix of a frame
 * lives in one CU's LDS); 128 < Np <= 1024: a workgroup per block of 32 query rows, keys / values from global memory. */
int cadre_pam(const float* x, const float* qkv, float gamma, float* y, int32_t F, int32_t Np,
              void* stream);
/* CAM_Module.forward da_att.py:63-83 on NHWC x [F][Np][128] */
int cadre_cam(const float* x, float gamma, float* y, int32_t F, int32_t Np, void* stream);
/* same kernels writing y as bf16 (fp32 math; feeds the bf16 conv51/conv52) */
int cadre_pam_bf16out(const float* x, const float* qkv, float gamma, void* y, int32_t F, int32_t Np,
                      void* stream);
int cadre_cam_bf16out(const float* x, float gamma, void* y, int32_t F, int32_t Np, void* stream);
/* InterTaskAtt 'transformer' tail intertask_att.py:137-176: qkv [F][6][256] ordered
 * (vis_q, vis_k, vis_v, bc_q, bc_k, bc_v) -> out [F][ldo] = cat(att_visual, att_bc) */
int cadre_intertask_att(const float* qkv, float* out, int64_t ldo, int32_t F, float temperature,
                        void* stream);
/* agent.py:105-111: feat[f][512..529] = float(measurements[f][j%3]) (f64 -> f32), ld = ldo */
int cadre_append_measurements(const double* meas, float* feat, int64_t ldo, int32_t F, void* stream);

/* ---------------------------------------------------------------- storage math
 * RolloutStorage.compute_returns GAE branch (ppo_agent/storage.py:69-76), strict fp32
 * left-to-right, no FMA contraction; one lane per sequence.  Arrays are [nseq][T+1]
 * (value_preds[.][T] is overwritten with next_value like storage.py:70).  Then
 * train.py:82-88: adv = ret[:-1]-V[:-1], optional (adv-mean)/(std_unbiased+1e-8). */
int cadre_gae(const float* rewards, float* value_preds, const float* masks, const float* next_value,
              float* returns, float* adv, int32_t nseq, int32_t T, float gamma, float gamma_tau,
              int32_t normalise, void* stream);
/* feed_forward_generator gather (storage.py:99-120): obs [T+1][S][ldo] rows idx[B] ->
 * time-major x [S][B][ldx]; hn/cn/scalars gathered likewise. */
int cadre_gather_obs(const float* obs, int64_t ldo, int32_t S, const int64_t* idx, int32_t B,
                     float* x, int64_t ldx, int32_t D, void* stream);

/* storage.py:99-120 + the unpacking at agent.py:167-168 in one launch: every field of one head's
 * minibatch (rows idx[0..B) of the storage) is written into rows b0..b0+B of the Bt-row packed
 * update workspace: X [S][Bt][ldx] time-major, h0/c0 [Bt][ldho], scalars [Bt]. */
int cadre_gather_minibatch(const float* obs, int64_t ldo, int32_t S, const float* hn, const float* cn,
                           int64_t ldh, const int64_t* action, const float* value_preds,
                           const float* returns, const float* logp, const int32_t* command,
                           const float* adv, const int64_t* idx, int32_t B, int32_t D, int32_t Hd,
                           int32_t Bt, int32_t b0, float* X, int64_t ldx, float* h0, float* c0,
                           int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                           float* returns_o, float* old_logp_o, float* adv_o, void* stream);

/* The same gather for every worker and both heads in one launch (train.py:93-102 iterates workers; each worker's two
 * feed_forward_generators storage.py:93-120).  src_table: n_src = 2 * workers records of nine device pointers
 * {obs, hn, cn, action, value_preds, returns, action_log_probs, command, adv} for (worker, head) = (i / 2, i % 2);
 * idx [n_src][Bw] row ids; worker w fills rows w*Bw .. of the Bt-row batch; outputs are [2][...] arrays of the two
 * heads (X / h0 / c0 with the given head strides, the scalars [2][Bt]). */
int cadre_gather_minibatch_multi(const void* src_table, int32_t n_src, int64_t ldo, int32_t S, int64_t ldh,
                                 const int64_t* idx, int32_t Bw, int32_t D, int32_t Hd, int32_t Bt, float* X,
                                 int64_t x_head_stride, int64_t ldx, float* h0, float* c0, int64_t h_head_stride,
                                 int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                                 float* returns_o, float* old_logp_o, float* adv_o, void* stream);
/* The same gather with the stable counting sort by command and the placement of cadre_sort_rows_by_command +
 * cadre_permute_minibatch in the SAME launch: row (worker, b) of head hd lands at its sorted position in the [2][...] workspace
 * arrays, pos[hd * Bt + row] gets that position and seg[2 * (hd * C + c)] = (first row, rows) of command c (agent.py:166-237's
 * per-command nets each read one run of rows).  Needs (n_src / 2) * Bw == Bt. */
int cadre_gather_sorted_multi(const void* src_table, int32_t n_src, int64_t ldo, int32_t S, int64_t ldh,
                              const int64_t* idx, int32_t Bw, int32_t D, int32_t Hd, int32_t Bt, int32_t C, float* X,
                              int64_t x_head_stride, int64_t ldx, float* h0, float* c0, int64_t h_head_stride,
                              int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                              float* returns_o, float* old_logp_o, float* adv_o, int32_t* pos, int32_t* seg, void* stream);

/* Recurrent weights W [4*D][ldw = 544] of `Z` nets (net z at + z * w_str) -> MFMA FRAGMENT ORDER for the fused LSTM
 * steps, both directions (ppo_update.hip): `fwd` for cadre_lstm_step_fwd, `bwd` (the transpose: the backward reduces
 * over the gate axis) for cadre_lstm_step_bwd; ceil(D / 16) * 4 * 34 * 256 floats per net each, net stride p_str.
 * Once per optimiser step — a fragment read from the row-major matrix is 16 rows x 64 bytes per wave instruction, from
 * these copies one contiguous KiB. */
int cadre_pack_lstm_weights(const float* W, int64_t w_str, int32_t ldw, int32_t D, int32_t Z, float* fwd, float* bwd,
                            int64_t p_str, void* stream);
/* One LSTM time step of `Z` nets, product AND cell math in one launch (ppo_update.hip; models.py:139-152 nn.LSTMCell):
 * gates = G (x-projection + b_ih, [B][ldg] per net) + h_{t-1} W^T + bias; G <- (i, f, g, o) activated; c_t, h_t,
 * tanh(c_t) written.  Wp: the packed weights (`fwd` of cadre_pack_lstm_weights); K = ldh = 544 (hidden D zero padded);
 * net z at + z * *_str.  row_seg [Z][2] (may be NULL): (first row, count) of net z's run of rows — exactly those rows
 * are read and written (16-row tiles from the run's first row).
 * `rev` (0/1): order in which the unit slices are walked — alternate it from step to step so that each XCD's L2
 * re-uses the most recently read weights first (speed only). */
int cadre_lstm_step_fwd(const float* Wp, int64_t wp_str, const float* bias, int64_t b_str, float* G, int32_t ldg,
                        int64_t g_str, const float* Hprev, const float* Cprev, float* Hout, float* Cout, float* TCout,
                        int32_t ldh, int64_t h_str, int32_t B, int32_t D, int32_t Z, const int32_t* row_seg,
                        int32_t rev, void* stream);
/* The MLP towers of update_policy (models.py:171-177 critic, distributions.py:34-40 actor; Linear(530 -> 128) ReLU
 * Linear(128 -> 128) ReLU Linear(128 -> n_out), n_out rows padded to 64, input rows [B][ldh = 544]) for Z2 = 2 * nets
 * towers in three launches (ppo_update.hip).  Tower z2 = 2*net + {actor, critic} at P + z2 * t_str; offs[6] = float
 * offsets of (W1, b1, W2, b2, W3, b3) inside a tower, weights [out][in] row-major; A1 / A2 / dA1 / dA2 [Z2][B][128],
 * O3 / dO3 [Z2][B][64]; net z's input rows at Hin + z * h_str.  row_seg [Z2/2][2] (may be NULL = every row): (first
 * row, count) of the run of rows net z owns in the row-sorted minibatch — no other row is read or written.
 * cadre_mlp_fwd: A1, A2 (post-ReLU) and O3.  cadre_mlp_bwd: dA2 = (dO3 W3) [A2 > 0], dA1 = (dA2 W2) [A1 > 0] and
 * dH[net] = sum over the net's two towers of dA1 W1 ([B][ldh] at dH + net * d_str).  cadre_mlp_dw: the gradients of the
 * six parameter blocks of every tower at G + z2 * t_str + offs[...] (written, not accumulated). */
int cadre_mlp_fwd(const float* P, int64_t t_str, const int32_t* offs, const float* Hin, int32_t ldh, int64_t h_str,
                  float* A1, float* A2, float* O3, int32_t B, int32_t Z2, const int32_t* row_seg, void* stream);
int cadre_mlp_bwd(const float* P, int64_t t_str, const int32_t* offs, const float* dO3, const float* A1, const float* A2,
                  float* dA1, float* dA2, float* dH, int32_t ldh, int64_t d_str, int32_t B, int32_t Z2,
                  const int32_t* row_seg, void* stream);
int cadre_mlp_dw(const float* dO3, const float* dA2, const float* dA1, const float* A2, const float* A1, const float* Hin,
                 int32_t ldh, int64_t h_str, float* G, int64_t t_str, const int32_t* offs, int32_t B, int32_t Z2,
                 const int32_t* row_seg, void* stream);
/* One backward time step: dh_{t-1} = dG_t W (+ dh_in) on the packed transposed weights (`bwd` of
 * cadre_pack_lstm_weights) and dG_t in fragment order (dGp_in: what the previous call left in its dGp_out), then the
 * cell backward of step t-1 in the same launch: dG_{t-1} from the activated gates G_act, tanh(c_{t-1}), c_{t-2}, written
 * row-major (dG_out, [B][ldg]) AND in fragment order (dGp_out: ceil(B / 16) tiles of 16 x 2176 floats per net, net stride
 * gp_str; zero-initialised by the caller, pad never written); dC in/out.  dGp_in == NULL: no product (first step:
 * dh = dh_in, the gradient of the MLP towers).  commands [2][B] (may be NULL): net z = head*C + c keeps only rows whose
 * command is c, the others get dG = 0 and dc = 0 (unsorted minibatch); row_seg [Z][2] (may be NULL): (first row, count) of
 * net z's run in the row-sorted minibatch — exactly those rows are read and written, and the 16-row tiles of dGp count
 * from the run's first row. */
int cadre_lstm_step_bwd(const float* Wp, int64_t wp_str, const float* dGp_in, float* dGp_out, int64_t gp_str,
                        float* dG_out, const float* G_act, int32_t ldg, int64_t g_str, const float* dh_in, float* dC,
                        int64_t d_str, const float* TC, const float* Cprev, int32_t ldh, int64_t h_str, int32_t B, int32_t D,
                        int32_t Z, const int32_t* commands, int32_t C, const int32_t* row_seg, int32_t rev, void* stream);
/* The LSTM weight gradients of `Z` nets in one launch (ppo_update.hip): dWhh = sum_t dG_t^T h_{t-1}, dWih = sum_t
 * dG_t^T x_t ([H4][ldw] each, columns 0..N-1 written), dbih = dbhh = column sums of dG.  dG [S][B][ldg] (gate axis zero
 * padded to a multiple of 64), Hs [S+1][B][ldh] (slot t = h_{t-1}), X [S][B][ldh] (net z reads input slot z / x_div).
 * row_seg: only rows [beg & ~3, beg + cnt) of every time step are multiplied — the rows of other nets hold exact zeros. */
int cadre_lstm_dw(const float* dG, int32_t ldg, int64_t g_str, const float* Hs, const float* X, int32_t ldh,
                  int64_t h_str, int64_t x_str, int32_t x_div, float* dWhh, float* dWih, float* dbih, float* dbhh,
                  int32_t ldw, int64_t w_str, int32_t B, int32_t S, int32_t H4, int32_t N, int32_t Z,
                  const int32_t* row_seg, void* stream);
/* column sums: out[z][n] (+)= sum_m X[z][m][n]  (bias gradients) */
int cadre_colsum(const float* X, int64_t ldx, int64_t x_str, float* out, int64_t o_str,
                 int32_t M, int32_t N, int32_t batch, int32_t accumulate, void* stream);
/* y = relu'(act) * dy elementwise, in place on dy.  Optional ownership mask (commands != NULL): the
 * buffers are [2*Z][B][hid] (tower z = 2*net + t, net = head*C + c); rows whose command differs from
 * the net's c are set to exactly 0. */
int cadre_relu_bwd(const float* act, float* dy, int64_t n, const int32_t* commands, int32_t B,
                   int32_t hid, int32_t C, void* stream);
/* Stable sort of each head's B minibatch rows by command: pos[hd][b] = sorted position of row b,
 * seg[hd*C + c] = (begin, count) of command c.  commands/pos are [2][B] i32, seg is [2*C][2] i32. */
int cadre_sort_rows_by_command(const int32_t* commands, int32_t B, int32_t C, int32_t* pos, int32_t* seg,
                               void* stream);
/* Apply pos to the packed minibatch (cadre_gather_minibatch outputs) of `heads` heads in one launch: dst row pos[b] = src
 * row b for X [S][B][ldx], h0/c0 [B][ldh] and the six per-row scalars; head h reads and writes X + h * x_hstr,
 * h0 / c0 + h * h_hstr, pos and the scalars + h * B. */
int cadre_permute_minibatch(const int32_t* pos, int32_t B, int32_t S, const float* X, float* Xo, int64_t ldx,
                            const float* h0, const float* c0, float* h0o, float* c0o, int64_t ldh,
                            const int64_t* actions, const int32_t* commands, const float* old_values,
                            const float* returns, const float* old_logp, const float* adv, int64_t* actions_o,
                            int32_t* commands_o, float* old_values_o, float* returns_o, float* old_logp_o,
                            float* adv_o, int32_t heads, int64_t x_hstr, int64_t h_hstr, void* stream);

/* ---------------------------------------------------------------- policy head + PPO loss
 * Replaces Model.evaluate_actions (models.py:199-208), Categorical_1d (distributions.py:
 * 66-105) and the loss of CadreAgent.update_policy (agent.py:166-229) forward AND backward.
 * Per head hd in {0:steer,1:throttle}, command net c in 0..C-1 (net = hd*C+c; C = command_num, the reference ships 4):
 *   logits: net n row b at logits + n*l_ns + b*ldl (first n_out[hd] columns valid),
 *   values: net n row b at values + n*v_ns + b*ldv.  Sample arrays are [2 heads][B].
 * Outputs: losses[3] = (value_loss*value_coeff, action_loss*clip_coeff, ent*ent_coeff),
 *   dlogits / dvalues (same addressing) = d total_loss / d(raw logits | critic output);
 *   whole dlogits rows (ldl columns) are written, only column 0 of a dvalues row.
 * `inv_b` = 1/(rows per worker minibatch) (sum of per-worker means).
 * `scratch`: 4 + 6 * ceil(B / 16) floats of device memory (arrival counter + per-workgroup partial sums: the losses are
 * summed in a fixed order whatever the order the workgroups finish in; scratch[0] must be ZERO before the first launch on a
 * scratch buffer — every launch leaves it zero again, so consecutive launches need no clearing).  `poison` (may be NULL): device int32; when
 * nonzero (the status word of the A/B build's cadre_lstm_seq_fwd) the three losses come out NaN. */
int cadre_ppo_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                   int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                   const float* old_logp, const float* adv, int32_t B, int32_t C, int32_t n_out_steer,
                   int32_t n_out_throttle, float clip, float value_coeff, float clip_coeff,
                   float ent_coeff, float inv_b, float* losses, float* dlogits, float* dvalues,
                   float* scratch, const int32_t* poison, void* stream);
/* cadre_ppo_loss with PPO update diagnostics and the KL gate (opt-in; the same loss kernel body compiled with its stats
 * reductions, losses / dlogits / dvalues bit-identical to cadre_ppo_loss).  Per head hd, with log r = lp - old_logp and
 * every mean taken with inv_b (the losses' denominator), the launch writes stats_row[hd * F + k]:
 *   k = 0 approx_kl = mean((r - 1) - log r)   1 old_approx_kl = mean(-log r)   2 clip_fraction = mean(|r - 1| > clip)
 *   3 value_clip_fraction = mean(|v - v_old| > clip)   4 ratio_mean   5 max |log r|   6 applied (1.0 / 0.0)
 * (k = 7 is not written here — cadre_grad_norms_hp puts the step's learning rate there; F >= CADRE_PPO_STATS_FIELDS).  The sums are combined by the loss kernel's last arriving workgroup
 * in workgroup order: two launches on the same inputs give the same bits.  stats_scratch: 12 * ceil(B / 16) floats.
 * target_kl > 0 arms the gate: when max(approx_kl steer, throttle) > 1.5 * target_kl, *stop is set to 1; *stop is
 * sticky (only the caller clears it) and `applied` = (*stop == 0) after the check.  target_kl == 0: no check; stop may
 * then be NULL (applied = 1) or a flag that is only read. */
#define CADRE_PPO_STATS_FIELDS 8
int cadre_ppo_loss_stats(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                         int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values,
                         const float* returns, const float* old_logp, const float* adv, int32_t B, int32_t C,
                         int32_t n_out_steer, int32_t n_out_throttle, float clip, float value_coeff, float clip_coeff,
                         float ent_coeff, float inv_b, float* losses, float* dlogits, float* dvalues, float* scratch,
                         const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch, float target_kl,
                         int32_t* stop, void* stream);
/* Per-model pre-clip gradient norms sqrt(norms2[m]) (what clip_grad_norm_ returns) of the optimiser step that just ran on
 * norms2, into a stats row [2][F]: model m = kind * 2C + head * C + c (the arena's segment order: 2C LSTM blocks, then 2C
 * MLP-tower pairs) goes to stats_row[head * F + CADRE_PPO_STATS_FIELDS + kind * C + c].  F >= CADRE_PPO_STATS_FIELDS + 2 C. */
int cadre_grad_norms(const double* norms2, int32_t C, float* stats_row, int32_t F, void* stream);

/* ---------------------------------------------------------------- device-resident hyper-parameters
 * The hyper-parameter block: a device array of CADRE_HP_FIELDS doubles (8-byte aligned) that the `_hp` entry points read
 * at RUN time, so a captured hipGraph follows whatever the block holds when it is replayed.  The fields past
 * CADRE_HP_SIL_VALUE_COEFF are reserved no longer: the one that was left, 15, is CADRE_HP_SMOOTH_COEFF, so every field of the
 * block is in use.  betas and eps stay by-value arguments.  The block is written by ordinary
 * stream-ordered copies from the host, and by the KL-adaptive controller below. */
#define CADRE_HP_FIELDS 16
#define CADRE_HP_LR 0
#define CADRE_HP_CLIP 1
#define CADRE_HP_VALUE_COEFF 2
#define CADRE_HP_CLIP_COEFF 3
#define CADRE_HP_ENT_COEFF 4
#define CADRE_HP_MAX_GRAD_NORM 5
#define CADRE_HP_DESIRED_KL 6       /* > 0: the KL-adaptive learning rate is on */
#define CADRE_HP_LR_MIN 7
#define CADRE_HP_LR_MAX 8
#define CADRE_HP_LR_FACTOR 9
/* Two of the reserved fields, read by cadre_ppo_demo_loss only and zero for everyone else: the weight of the demonstration
 * cross-entropy and of the demonstration rows' value regression.  (Enumerators: the macros above are the ten fields every
 * `_hp` entry point shares, the list the Python binding's HP table mirrors one to one.) */
enum { CADRE_HP_DEMO_COEFF = 10, CADRE_HP_DEMO_VALUE_COEFF = 11 };
/* A third reserved field, read by cadre_ppo_sug_loss only and zero for everyone else: the weight of the exploration-suggestion
 * KL term. */
enum { CADRE_HP_SUGGEST_COEFF = 12 };
/* Two more, read by cadre_ppo_sil_loss only and zero for everyone else: the weight of the self-imitation policy term and of
 * its value term. */
enum { CADRE_HP_SIL_COEFF = 13, CADRE_HP_SIL_VALUE_COEFF = 14 };
/* The last field, read by cadre_ppo_smooth_loss only and zero for everyone else: the weight of the temporal smoothness term. */
enum { CADRE_HP_SMOOTH_COEFF = 15 };
/* cadre_ppo_loss / cadre_ppo_loss_stats with clip, value_coeff, clip_coeff, ent_coeff = (float)hp[CADRE_HP_*] (the same
 * kernel bodies, the scalars read once per thread before the row loop; the stats variant uses the same clip for its clip
 * fractions).  Equal values give results bit-identical to the by-value entry points.
 * cadre_ppo_loss_stats_hp also runs the KL-ADAPTIVE LEARNING RATE when hp[CADRE_HP_DESIRED_KL] > 0: in the last arriving
 * workgroup, after the target_kl gate check, unless the stop flag is set after that check, with
 * kl = max(approx_kl steer, approx_kl throttle) of this launch (the float32 values of the stats row, as double):
 *   kl > 2 desired:         hp[LR] = max(hp[LR_MIN], hp[LR] / hp[LR_FACTOR])
 *   0 < kl < desired / 2:   hp[LR] = min(hp[LR_MAX], hp[LR] * hp[LR_FACTOR])
 * in double; the optimiser step that follows on the stream reads the new value. */
int cadre_ppo_loss_hp(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                      int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values,
                      const float* returns, const float* old_logp, const float* adv, int32_t B, int32_t C,
                      int32_t n_out_steer, int32_t n_out_throttle, double* hp, float inv_b, float* losses,
                      float* dlogits, float* dvalues, float* scratch, const int32_t* poison, void* stream);
int cadre_ppo_loss_stats_hp(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                            int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values,
                            const float* returns, const float* old_logp, const float* adv, int32_t B, int32_t C,
                            int32_t n_out_steer, int32_t n_out_throttle, double* hp, float inv_b, float* losses,
                            float* dlogits, float* dvalues, float* scratch, const int32_t* poison, float* stats_row,
                            int32_t F, float* stats_scratch, float target_kl, int32_t* stop, void* stream);
/* cadre_grad_norms that also writes the learning rate the step used, (float)hp[CADRE_HP_LR], into
 * stats_row[CADRE_PPO_STATS_LR] (field 7 of head 0, which cadre_ppo_loss_stats leaves alone).  To be enqueued after the
 * optimiser step and before the next loss launch. */
#define CADRE_PPO_STATS_LR 7
int cadre_grad_norms_hp(const double* norms2, int32_t C, float* stats_row, int32_t F, const double* hp, void* stream);
/* Explained variance of the value head per storage: src_table = device array of n_src records {const float* returns,
 * const float* value_preds, int64_t T}; out[i] = 1 - Var(R - V) / Var(R) over rows 0 .. T-1 (population variances,
 * fp64, fixed summation order), NaN where Var(R) == 0. */
int cadre_explained_variance(const void* src_table, int32_t n_src, double* out, void* stream);
/* Model.act sampling (models.py:184-189, distributions.py:96-99) == argmax(p/q), q supplied
 * by the host from the torch CPU generator.  logits [R][ldl] raw; outputs action i64 [R],
 * log_prob f32 [R] of the sampled action. */
int cadre_sample(const float* logits, int64_t ldl, const float* q, int64_t ldq, int32_t R,
                 int32_t n_out, int64_t* action, float* logp, void* stream);

/* ---------------------------------------------------------------- act for N environments (csrc/act_batch.hip)
 * CadreAgent.act_batch: agent.py:97-141 of N environments in one launch chain.  Rows of the LSTM / MLP pass are sorted
 * by command: environment e is row pos[e] (0 <= pos[e] < N).
 * cadre_act_windows: the LSTM input rows of every environment's window.  ring [n_ring][S][512] (slot stride
 * ring_env_str floats) holds environment e's last window of latents at slot e; fresh [F][ld_fresh] the latents encoded
 * this step.  mode[e] 1: the window shifted by one frame (rows 1..S-1 of the ring, then fresh row first[e]); 0: S fresh
 * rows first[e] .. first[e] + S - 1.  meas f64 [N][S][3].  Writes X[s][pos[e]][0..DP) = latent | the measurements as
 * f32, repeated 6 times at columns 512..529 (cadre_append_measurements) | zeros, the same rows in environment order into
 * feat [N][S][ldf] (may be NULL), and the new window into the ring. */
int cadre_act_windows(float* ring, int64_t ring_env_str, int32_t n_ring, const float* fresh, int64_t ld_fresh, int32_t F,
                      const int32_t* mode, const int32_t* first, const double* meas, const int32_t* pos, int32_t N,
                      int32_t S, float* X, int64_t ldx, int32_t DP, float* feat, int64_t ldf, void* stream);
/* cadre_sample for every (environment, head) pair in one launch (one wave each, the same arithmetic): environment e
 * with command cmd[e] (0 <= cmd[e] < C) reads the actor tower z = 2 * (head * C + cmd[e]) and the critic z + 1 of
 * O3 [2 Z][z_str] at row pos[e] (row pitch ldo), and q [N][2][64].  action i64 / logp / value f32 [N][2] are written
 * in ENVIRONMENT order (the sort is undone). */
int cadre_sample_rows(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd, int32_t N,
                      int32_t C, const float* q, int32_t K_steer, int32_t K_throttle, int64_t* action, float* logp,
                      float* value, void* stream);
/* RolloutStorage.insert (storage.py:45-58) for n_dst = 2 N storages in one launch.  dst_table: device array of n_dst
 * records of nine pointers (obs [T+1][S][ldo], hn, cn [T+1][ldh], action i64, action_log_probs, value_preds,
 * rewards, masks f32, command i32 [T+1]); storage k = 2 e + head is written at cursor slot[k] (0 <= slot[k] <= T,
 * the cursors stay on the host): obs <- feat[e] ([S][ldf], D columns), action / log-prob / value <- entry k of the
 * [N][2] outputs of cadre_sample_rows, reward / mask <- rm [n_dst][2], command <- cmd[e], and the zero hidden state
 * into hn / cn[slot + 1] (Hd columns) while slot < T. */
int cadre_insert_rows(const void* dst_table, const int32_t* slot, int32_t n_dst, int32_t S, int64_t ldo, int64_t ldh,
                      int32_t D, int32_t Hd, int32_t T, const float* feat, int64_t ldf, const int64_t* action,
                      const float* logp, const float* value, const float* rm, const int32_t* cmd, void* stream);

/* Model.evaluate_actions forward (models.py:199-208): per row log-prob of `actions` and entropy
 * of Categorical(logits=raw logits) */
int cadre_categorical_eval(const float* logits, int64_t ldl, const int64_t* actions, int32_t R,
                           int32_t n_out, float* logp, float* entropy, void* stream);
/* Categorical_1d.forward (distributions.py:66-83): what Categorical(logits=raw) exposes — normalised
 * `logits` = raw - logsumexp(raw) and `probs` = softmax(logits), [R][n_out] each (dense rows), plus the
 * per-row argmax of probs (first maximum, `mode`).  Any of the three outputs may be NULL. */
int cadre_categorical_dist(const float* raw, int64_t ldl, int32_t R, int32_t n_out, float* logits_out,
                           float* probs_out, int64_t* mode_out, void* stream);

/* ---------------------------------------------------------------- ordinal policy heads (opt-in, csrc/ordinal.h)
 * The ordinal parameterisation of Tang & Agrawal, "Discretizing Continuous Action Space for On-Policy Optimization" (the
 * commented-out "ordinal policy" block of distributions.py:45-79) for heads whose bins are an ordered quantity.  Per head
 * with K bins, rank[k] in 0 .. K-1 is the position of bin k in ascending order of its control value (a permutation),
 * bin[r] its inverse, and column j of the actor tower's raw output x is threshold unit j in RANK space.  With eps = 1e-8:
 *   s_j = sigmoid(x_j)   t_j = sigmoid(-x_j)   u_j = log(s_j + eps)   w_j = log(t_j + eps)
 *   z_r = sum_{j <= r} u_j + sum_{j > r} w_j            (mask1 of the reference: a[i][j] = 1 iff i >= j)
 *   logit of bin k = z_{rank[k]}
 * From there everything is the categorical head on these logits, in bin space: normalised logits, probs, entropy,
 * log-prob, argmax(p / q) sampling with q[k] belonging to bin k (lowest bin index wins ties), mode, diagnostics.
 * Backward, with g_k = d total / d logit_k (what dlogits holds for a categorical head) and G_r = g_{bin[r]}:
 *   d total / d x_j = s_j t_j / (s_j + eps) * sum_{r >= j} G_r  -  s_j t_j / (t_j + eps) * sum_{r < j} G_r
 * which is what dlogits holds for an ordinal head: the gradient with respect to the raw tower outputs.  The running sums
 * are wave scans with one fixed combination order: two launches on the same inputs give the same bits.
 * Rank table `ord`: device int32 [2][64], head-major, ord[h][k] = rank[k] for k < K_h; ord[h][0] = -1 marks head h as the
 * plain categorical head.  A single-head table is int32 [64] with the same convention.  The caller guarantees a
 * permutation of 0 .. K-1 (the kernels do not check).  With the -1 marker every output is bit-identical to the entry
 * point that is extended.
 *
 * cadre_ppo_loss_ord: cadre_ppo_loss / _stats / _hp / _stats_hp in one entry point.  hp == NULL: clip, value_coeff,
 * clip_coeff and ent_coeff are the by-value arguments, else they are read from the block and the by-value ones are
 * ignored.  stats_row == NULL: no diagnostics (F, stats_scratch, target_kl, stop are then ignored).  Same grid, scratch
 * sizes and last-arriver reduction as the entry points it extends. */
int cadre_ppo_loss_ord(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv,
                       int64_t v_ns, const int64_t* actions, const int32_t* commands, const float* old_values,
                       const float* returns, const float* old_logp, const float* adv, int32_t B, int32_t C,
                       int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip, float value_coeff,
                       float clip_coeff, float ent_coeff, float inv_b, float* losses, float* dlogits, float* dvalues,
                       float* scratch, const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch,
                       float target_kl, int32_t* stop, const int32_t* ord, void* stream);
/* cadre_sample / cadre_categorical_eval / cadre_categorical_dist with one head's rank table ord int32 [64] (ldl >= n_out
 * is checked here); cadre_categorical_dist_ord returns normalised logits, probs and mode in bin space. */
int cadre_sample_ord(const float* logits, int64_t ldl, const float* q, int64_t ldq, int32_t R, int32_t n_out,
                     int64_t* action, float* logp, const int32_t* ord, void* stream);
int cadre_categorical_eval_ord(const float* logits, int64_t ldl, const int64_t* actions, int32_t R, int32_t n_out,
                               float* logp, float* entropy, const int32_t* ord, void* stream);
int cadre_categorical_dist_ord(const float* raw, int64_t ldl, int32_t R, int32_t n_out, float* logits_out,
                               float* probs_out, int64_t* mode_out, const int32_t* ord, void* stream);
/* cadre_sample_rows with both heads' tables ord int32 [2][64]. */
int cadre_sample_rows_ord(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd, int32_t N,
                          int32_t C, const float* q, int32_t K_steer, int32_t K_throttle, int64_t* action, float* logp,
                          float* value, const int32_t* ord, void* stream);

/* ---------------------------------------------------------------- behaviour cloning (csrc/imitation.hip)
 * cadre_bc_loss: the imitation loss where cadre_ppo_loss_ord stands in the update — the same addressing of logits, values,
 * dlogits and dvalues, the same grid, the same `scratch` (arrival counter zero on entry and left zero, partials combined by
 * the last arriving workgroup in workgroup order: two launches on the same inputs give the same bits), the same `poison`
 * and the same rank table `ord` (NULL, or ord[h][0] = -1: the plain categorical head).  Sample arrays [2 heads][B]:
 * actions (the demonstrated bin), commands, returns (the critic's regression target), weights (NULL: 1).
 * For head h, row b, command c in range, the own net's normalised logits lg_k and probabilities p_k (the statements of the
 * PPO kernel), K = n_out of the head, e = label_smoothing and t_k = (1 - e) [k = a] + e / K:
 *   ce_b = -sum_k t_k lg_k     H_b = -sum_k p_k lg_k     vl_b = (v - R)^2
 *   losses[0] = value_coeff 0.5 sum w_b vl_b inv_b   losses[1] = bc_coeff sum w_b ce_b inv_b   losses[2] = ent_coeff sum w_b H_b inv_b
 * (total = losses[0] + losses[1] - losses[2]), and
 *   dlogits = w_b inv_b (bc_coeff (p_k - t_k) + ent_coeff p_k (lg_k + H_b))   in bin space (an ordinal head: through ord_backward)
 *   dvalues = value_coeff w_b inv_b (v - R)
 * for the own net; columns >= K and the other C - 1 nets of the head get exact zeros (whole rows of ldl columns).
 * A row whose command is out of range or whose action is outside 0 .. K - 1 (-1 is the "no label for this head" marker)
 * adds nothing for that head and gets exact zeros in all C nets.
 * dlogits == NULL && dvalues == NULL: the evaluation form, losses and statistics only (exactly one NULL is refused).
 * stats_row (may be NULL) float [2][F], F >= CADRE_BC_STATS_FIELDS, per head, means over inv_b in the same fixed order:
 *   0 top-1 accuracy (the lowest index among the largest p_k equals a)   1 mean -lg_a (unweighted, unsmoothed)
 *   2 mean H   3 mean |v - R|   4 sum w inv_b   5 rows counted inv_b
 * stats_scratch: 2 * ceil(B / 16) * CADRE_BC_STATS_FIELDS floats.  Refused before any launch: bad B, C or n_out,
 * ldl < n_out or > 64, NULL required pointers, label_smoothing outside [0, 1), exactly one of dlogits / dvalues NULL. */
#define CADRE_BC_STATS_FIELDS 6
int cadre_bc_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                  const int64_t* actions, const int32_t* commands, const float* returns, const float* weights,
                  int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, float label_smoothing,
                  float bc_coeff, float value_coeff, float ent_coeff, float inv_b, float* losses, float* dlogits,
                  float* dvalues, float* scratch, const int32_t* poison, float* stats_row, int32_t F,
                  float* stats_scratch, const int32_t* ord, void* stream);
/* cadre_demo_rows: the observation rows of a demonstration set in one launch.  latent f32 [n_frames][ld_lat >= 512] (each
 * distinct frame encoded once), window int32 [T][S], meas f64 [n_frames][3] -> obs f32 [T][S][ldo]:
 *   obs[t][s][0:512] = latent[window[t][s]] | [512:530] = the frame's three measurements as f32, six times
 *   (cadre_append_measurements) | zeros up to the pitch.
 * A window index outside 0 .. n_frames - 1 reads nothing and gives NaN in columns 0 .. 529.  16 bytes per lane: both
 * pitches are multiples of 4 floats, both bases 16-byte aligned, 532 <= ldo <= 1024.  Rows past T are not touched. */
int cadre_demo_rows(const float* latent, int64_t ld_lat, int32_t n_frames, const int32_t* window, const double* meas,
                    int32_t T, int32_t S, float* obs, int64_t ldo, void* stream);

/* ---------------------------------------------------------------- demonstration term inside the PPO step (csrc/demo_mix.hip)
 * cadre_ppo_demo_loss: ONE loss launch for a minibatch that holds PPO rows and demonstration rows (DAPG-style mixing), where
 * cadre_ppo_loss_ord / cadre_bc_loss stand in the update — the same addressing of logits, values, dlogits and dvalues, the
 * same grid, the same `scratch` (4 + 6 * ceil(B / 16) floats; arrival counter zero on entry and left zero, partials combined
 * by the last arriving workgroup in workgroup order: two launches on the same inputs give the same bits), the same `poison`
 * and the same rank table `ord` (NULL, or ord[h][0] = -1: the plain categorical head).  Sample arrays [2 heads][B].
 * row_kind int32 [2][B], per head: 0 a PPO row, anything else a demonstration row.
 *   A PPO row runs exactly the statements of cadre_ppo_loss_ord with clip, value_coeff, clip_coeff, ent_coeff and inv_b
 *   (1 / rows per worker minibatch); a row with a bad command behaves as there.
 *   A demonstration row runs the statements of cadre_bc_loss with bc_coeff = demo_coeff, value_coeff = demo_value_coeff, no
 *   entropy term and inv_bd (1 / demonstration rows per step) for inv_b: its weight w is read from the `adv` slot, its target
 *   from `returns`, its label from `actions`; old_values and old_logp are not read.  With a command out of range or an action
 *   outside 0 .. K - 1 (-1: no label for this head) it gets exact zeros in all C nets of the head and adds nothing to any sum.
 * hp == NULL: every scalar is the by-value argument.  Otherwise clip, value_coeff, clip_coeff, ent_coeff are read from the
 * block as in cadre_ppo_loss_ord and demo_coeff = (float)hp[CADRE_HP_DEMO_COEFF], demo_value_coeff =
 * (float)hp[CADRE_HP_DEMO_VALUE_COEFF]; label_smoothing, inv_b and inv_bd stay by value.
 *   losses[3]      the three PPO terms over the PPO rows only, as cadre_ppo_loss writes them
 *   demo_losses[2] (demo_coeff sum w ce inv_bd,  demo_value_coeff 0.5 sum w (v - R)^2 inv_bd) over the demonstration rows
 *   total = losses[0] + losses[1] - losses[2] + demo_losses[0] + demo_losses[1]; dlogits / dvalues are its derivative
 * stats_row (may be NULL; then F, stats_scratch, target_kl, stop are ignored): the CADRE_PPO_STATS_FIELDS diagnostics of
 * cadre_ppo_loss_stats per head over the PPO rows ONLY (means with inv_b), followed by the rule of cadre_ppo_loss_stats(_hp):
 * the target_kl gate, `applied` and with hp the KL-adaptive lr see the policy's KL on its own rollouts, undiluted by
 * demonstration rows.  stats_scratch: 12 * ceil(B / 16) floats.
 * demo_stats_row (may be NULL) float [2][demo_F], demo_F >= CADRE_BC_STATS_FIELDS: the six statistics of cadre_bc_loss per head
 * over the demonstration rows, means with inv_bd.
 * demo_scratch (always required: the demo sums go through it): 2 * ceil(B / 16) * (2 + CADRE_BC_STATS_FIELDS) floats; it
 * needs no initialisation.
 * Refused before any launch: the argument checks of cadre_ppo_loss_ord and cadre_bc_loss, NULL row_kind, NULL demo_losses or
 * demo_scratch, label_smoothing outside [0, 1), inv_bd not finite or <= 0 while anything needs it (hp != NULL, a non-zero
 * demo coefficient, or a demo stats row). */
int cadre_ppo_demo_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                        const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                        const float* old_logp, const float* adv, const int32_t* row_kind, int32_t B, int32_t C,
                        int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip, float value_coeff,
                        float clip_coeff, float ent_coeff, float inv_b, float label_smoothing, float demo_coeff,
                        float demo_value_coeff, float inv_bd, float* losses, float* demo_losses, float* dlogits,
                        float* dvalues, float* scratch, float* demo_scratch, const int32_t* poison, float* stats_row, int32_t F,
                        float* stats_scratch, float target_kl, int32_t* stop, float* demo_stats_row, int32_t demo_F,
                        const int32_t* ord, void* stream);
/* cadre_mix_row_kinds: row_kind[h][pos[h][u]] = (u >= B_ppo) for both heads — the kinds of a minibatch whose unsorted rows
 * B_ppo .. B - 1 are the demonstration rows.  pos int32 [2][B]: the sorted position of each unsorted row
 * (cadre_gather_sorted_multi / cadre_sort_rows_by_command); NULL: the identity (unsorted layout).  A position outside
 * 0 .. B - 1 writes nothing.  Refused before any launch: NULL row_kind, B < 1, B_ppo outside 0 .. B. */
int cadre_mix_row_kinds(const int32_t* pos, int32_t B, int32_t B_ppo, int32_t* row_kind, void* stream);

/* ---------------------------------------------------------------- PPG auxiliary phase (csrc/phasic.hip)
 * Extra critic epochs over the rows of past rollouts, with the policy held by a KL term against its own distributions as
 * recorded when the phase began (Cobbe et al. 2020, "Phasic Policy Gradient", the shared-trunk variant of section 3.5).
 * Both entry points address a minibatch through three arrays: commands int32 [2][B] in WORKSPACE order (the possibly
 * command-sorted layout of the update), pos int32 [2][B] = the workspace position of UNSORTED row u (cadre_gather_sorted_multi /
 * cadre_sort_rows_by_command; NULL: the identity) and row_id int64 [2][B] = the table row of unsorted row u, head-major.
 * table float [2][R][64]: per head and buffer row the normalised log-probabilities of the recorded policy, -inf in columns >= K.
 * One wave per row, 16 rows per workgroup, grid (ceil(B / 16), 2): the layout of cadre_bc_loss.
 *
 * cadre_aux_record: for head h and unsorted row u with b = pos[h][u], c = commands[h][b] in 0 .. C - 1 and
 * r = row_id[h][u] in 0 .. R - 1:   table[h][r][k] = lg_k = x_k - logsumexp(x)   (k < K; -inf for K <= k < 64)
 * with x the own net's logits at workspace row b (an ordinal head: through ord_logits) and lg formed by exactly the statements
 * of the loss kernels.  A row with b, c or r out of range writes nothing.  Two rows of one launch with the same r race (both
 * values are then stored by plain stores; launches in one stream are ordered).  Refused before any launch: NULL logits,
 * commands, row_id or table, B < 1, C < 1, n_out outside 1 .. 64, ldl < n_out or > 64, R < 1. */
int cadre_aux_record(const float* logits, int64_t ldl, int64_t l_ns, const int32_t* commands, const int32_t* pos,
                     const int64_t* row_id, int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle,
                     const int32_t* ord, float* table, int32_t R, void* stream);
/* cadre_aux_loss: the auxiliary loss where cadre_ppo_loss_ord / cadre_bc_loss stand in the update — the same addressing of
 * logits, values, dlogits and dvalues, the same `scratch` (4 + 6 * ceil(B / 16) floats; arrival counter zero on entry and left
 * zero, partials combined by the last arriving workgroup in workgroup order: two launches on the same inputs give the same
 * bits), the same `poison` and rank table `ord`.  returns float [2][B] in workspace order (the critic's regression target).
 * For head h, a row that counts (b, c, r in range as above), lo = table[h][r], lg / p of the current policy as above and
 * p_old formed from lo by the statements that form p from lg (max, expf, sum, divide: equal bits in give equal bits out):
 *   kl_b = sum_k p_old,k (lo_k - lg_k)   (not clamped at zero; a bin with p_old,k == 0 adds nothing)     vl_b = (v - R)^2
 *   losses[0] = aux_value_coeff 0.5 sum vl_b inv_b   losses[1] = beta_clone sum kl_b inv_b   losses[2] = 0
 *   (total = losses[0] + losses[1]; a non-zero *poison adds NaN to all three)
 *   dlogits = beta_clone inv_b (p_k - p_old,k)   in bin space (an ordinal head: through ord_backward)
 *   dvalues = aux_value_coeff inv_b (v - R)
 * for the own net; columns >= K and the other C - 1 nets of the head get exact zeros (whole rows of ldl columns).  A row whose
 * command or row_id is out of range adds nothing and gets exact zeros in all C nets; a row whose position b is out of range is
 * skipped.  A row recorded by cadre_aux_record from the logits it is trained on has kl_b == 0 and dlogits == 0 exactly.
 * stats_row (may be NULL) float [2][F], F >= CADRE_AUX_STATS_FIELDS, per head, partials combined in workgroup order:
 *   0 mean kl_b   1 max kl_b (fmaxf in the same order; 0 when no row counted)   2 mean |v - R|
 *   3 mean entropy of the current policy   4 mean (v - R)^2   5 rows counted   — the means and field 5 times inv_b, as in
 *   cadre_bc_loss.  stats_scratch: 2 * ceil(B / 16) * CADRE_AUX_STATS_FIELDS floats.
 * Refused before any launch: NULL logits, values, commands, returns, row_id, table, losses, dlogits, dvalues or scratch,
 * B < 1, C < 1, n_out outside 1 .. 64, ldl < n_out or > 64, R < 1, a stats row with F too small or no stats scratch. */
#define CADRE_AUX_STATS_FIELDS 6
int cadre_aux_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                   const int32_t* commands, const float* returns, const int32_t* pos, const int64_t* row_id,
                   const float* table, int32_t R, int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle,
                   float beta_clone, float aux_value_coeff, float inv_b, float* losses, float* dlogits, float* dvalues,
                   float* scratch, const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch,
                   const int32_t* ord, void* stream);

/* ---------------------------------------------------------------- exploration suggestions (csrc/suggest.hip)
 * Terminal-event priors in the PPO loss (Zhang et al. 2021, "End-to-End Urban Driving by Imitating a Reinforcement Learning
 * Coach", the exploration loss): an episode that ends with a named event z marks the last rows before it, and a marked row
 * adds KL(pi(.|s) || p_z) towards a prior p_z chosen for the event to its PPO terms.  A storage records a small integer code
 * per row (events int32 [T + 1], 0: none), the mark launch turns the codes into a kind per row (suggest int32 [T]), the rows
 * launch carries the kinds of a minibatch into the layout of the update, and the loss launch reads them there.
 *
 * cadre_suggest_note: events_k[slots[k]] = codes[k] for k < n, table = n device pointers (int64) to the `events` arrays; the
 * 2N codes of one env step in one launch.  A NULL pointer or a slot outside 0 .. T writes nothing.  Refused before any launch:
 * NULL table, slots or codes, n < 1, T < 1. */
int cadre_suggest_note(const void* table, const int32_t* slots, const int32_t* codes, int32_t n, int32_t T, void* stream);
/* cadre_suggest_mark: one launch for the n storages of a section, storage k belonging to head k & 1.  table = n records of
 * four device pointers (int64) {events int32 [T + 1], masks float [T + 1], time_limits float [T + 1] or 0, suggest int32 [T]};
 * Z event kinds, 1 <= Z <= 8; horizon int32 [2][Z + 1] = rows marked per (head, kind), entry 0 unused.  Per storage the result
 * is that of this backward scan, all in integers:
 *   cur = 0; left = 0
 *   for t = T - 1 .. 0:
 *     e = events[t]
 *     if 1 <= e <= Z and horizon[head][e] > 0:  cur = e; left = horizon[head][e]          (the nearest following event wins)
 *     elif masks[t] == 0 or (time_limits and time_limits[t] != 0):  cur = 0; left = 0     (row t ends an episode without an event)
 *     suggest[t] = cur if left > 0 else 0
 *     if left > 0: left -= 1
 * A window never crosses an episode boundary; an event code outside 1 .. Z is ignored.  Refused before any launch: NULL table
 * or horizon, n < 1, T < 1, Z outside 1 .. 8. */
int cadre_suggest_mark(const void* table, int32_t n, int32_t T, int32_t Z, const int32_t* horizon, void* stream);
/* cadre_suggest_rows: the kinds of a minibatch.  src_table = n_src device pointers (int64) to `suggest` arrays, source
 * zi = 2 * worker + head, and idx int64 [n_src][Bw] as handed to cadre_gather_sorted_multi.  A source pointer of 0 is a storage
 * without marks: its rows get kind 0.  kind int32 [2][Bt] in workspace order: row (worker, b) of head h goes to
 * kind[h][pos[h * Bt + worker * Bw + b]]; pos NULL: the identity (the placement of cadre_mix_row_kinds).  An index outside
 * 0 .. T - 1 or a position outside 0 .. Bt - 1 writes nothing.  Refused before any launch: NULL src_table, idx or kind, n_src
 * odd or < 2, Bw < 1, T < 1, (n_src / 2) * Bw > Bt. */
int cadre_suggest_rows(const void* src_table, int32_t n_src, const int64_t* idx, int32_t Bw, int32_t T, const int32_t* pos,
                       int32_t Bt, int32_t* kind, void* stream);
/* cadre_ppo_sug_loss: ONE loss launch where cadre_ppo_loss_ord stands in the update — the same addressing of logits, values,
 * dlogits and dvalues, the same grid, the same `scratch` (4 + 6 * ceil(B / 16) floats; arrival counter zero on entry and left
 * zero, partials combined by the last arriving workgroup in workgroup order: two launches on the same inputs give the same
 * bits), the same `poison`, rank table `ord` (required, as there), hp-or-by-value scalars and stats / target_kl / stop.
 * kind int32 [2][B] in workspace order; a kind outside 0 .. Z counts as 0.  prior float [2][Z + 1][64]: RAW log-priors in
 * columns < K per (head, kind), row 0 unused.
 *   A row of kind 0 runs exactly the statements of cadre_ppo_loss_ord.
 *   A row of kind z >= 1 runs them too and, with lg the policy's normalised log-probabilities, p its probabilities and
 *   lq = y - (max y + logf(sum expf(y - max y))) the prior row y normalised by the statements that normalise the policy row,
 *     kl = sum_k p_k (lg_k - lq_k)          dlogits += sug_coeff inv_b p_j ((lg_j - lq_j) - kl)   in bin space
 *   (an ordinal head: the sum of both gradients goes through ord_backward).  On a categorical head a row whose raw logits are
 *   bit-equal to its prior row has kl == 0 and a suggestion gradient of exact zeros.
 * The mean runs over the minibatch rows with inv_b, marked or not: the coefficient's meaning does not move with the count.
 *   losses[3]      the PPO terms, as cadre_ppo_loss_ord writes them
 *   sug_losses[1]  sug_coeff inv_b sum kl          total = losses[0] + losses[1] - losses[2] + sug_losses[0]
 * sug_coeff is the by-value argument, or (float)hp[CADRE_HP_SUGGEST_COEFF] when hp is not NULL.
 * stats_row: as in cadre_ppo_loss_ord — the PPO diagnostics, the KL gate and the adaptive lr see what they see without
 * suggestions (approx_kl is about the PPO ratio).  sug_stats_row (may be NULL) float [2][sug_F], sug_F >= CADRE_SUG_STATS_FIELDS,
 * per head: 0 marked rows   1 mean kl over the minibatch (sum kl inv_b)   2 max kl (0 when no row is marked)
 *   3 mean probability the policy gives the prior's mode (lowest index among the largest entries) over the marked rows.
 * sug_scratch (always required): 2 * ceil(B / 16) * 4 floats; it needs no initialisation.
 * Refused before any launch: the argument checks of cadre_ppo_loss_ord, NULL kind, prior, sug_losses or sug_scratch, Z outside
 * 1 .. 8, a sug_coeff that is not finite, sug_F too small. */
#define CADRE_SUG_STATS_FIELDS 4
int cadre_ppo_sug_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                       const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                       const float* old_logp, const float* adv, const int32_t* kind, const float* prior, int32_t Z, int32_t B,
                       int32_t C, int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip, float value_coeff,
                       float clip_coeff, float ent_coeff, float inv_b, float sug_coeff, float* losses, float* sug_losses,
                       float* dlogits, float* dvalues, float* scratch, float* sug_scratch, const int32_t* poison,
                       float* stats_row, int32_t F, float* stats_scratch, float target_kl, int32_t* stop, float* sug_stats_row,
                       int32_t sug_F, const int32_t* ord, void* stream);

/* ---------------------------------------------------------------- self-imitation learning (csrc/selfimit.hip)
 * Oh et al. 2018, "Self-Imitation Learning": rows of the agent's own past rollouts whose realised return R beat the critic
 * are replayed with weight w = max(R - v, 0).  A buffer of past storages keeps, per head and row, the return R, a flag word and
 * a priority q (uint32, 0: never drawn); SIL rows are drawn by priority on the device, ride behind the workers' rows of a
 * minibatch (kind 1 of cadre_mix_row_kinds), and the priorities of the drawn rows follow the w the step computed.
 *   quantise(w) = clamp(floor((w + prio_eps)^alpha * 2^16), 1, 2^31 - 1), the power in double (alpha == 1 takes none: exact).
 *
 * cadre_ppo_sil_loss: ONE loss launch where cadre_ppo_loss_ord / cadre_ppo_demo_loss stand in the update — the same addressing,
 * grid, `scratch` protocol (arrival counter zero on entry and left zero, partials combined by the last arriving workgroup in
 * workgroup order: equal inputs give equal bits), `poison`, rank table `ord`, hp-or-by-value scalars and stats / target_kl /
 * stop.  row_kind int32 [2][B] in workspace order.
 *   A row of kind 0 runs exactly the statements of cadre_ppo_loss_ord; the PPO sums, losses[3], the PPO diagnostics and the KL
 *   gate / adaptive lr see these rows only (means over inv_b).
 *   A row of kind != 0 is a SIL row (it needs a command in range and an action in 0 .. K - 1, else it writes zeros): with lp
 *   the log-prob of its action, p the probabilities, v its own net's value and R = returns[row],
 *     w = fmaxf(R - v, 0)     dlogits_k = (sil_coeff inv_bs w) (p_k - [k = a])  (through ord_backward on an ordinal head)
 *     dvalues = -(sil_value_coeff inv_bs w)      no entropy term; old_values, old_logp and adv are not read.
 *   A row with R <= v has w, every logit gradient and the value gradient exactly zero.
 *   sil_losses[2]  sil_coeff inv_bs sum(-lp w),  sil_value_coeff 0.5 inv_bs sum(w^2)
 *                  total = losses[0] + losses[1] - losses[2] + sil_losses[0] + sil_losses[1]
 *   sil_w [2][B]   the row's w in the update's layout, 0 for a PPO row or a row that does not count
 * sil_coeff / sil_value_coeff are the by-value arguments, or (float)hp[CADRE_HP_SIL_COEFF / CADRE_HP_SIL_VALUE_COEFF] when hp is
 * not NULL.  inv_bs = 1 / SIL rows per step.
 * sil_stats_row (may be NULL) float [2][sil_F], sil_F >= CADRE_SIL_STATS_FIELDS, per head over the SIL rows:
 *   0 mean w   1 share of rows with w > 0   2 mean -lp   3 mean |R - v|   (sums times inv_bs)   4 max w   5 rows counted
 * sil_scratch (always required): 2 * ceil(B / 16) * (2 + CADRE_SIL_STATS_FIELDS) floats; it needs no initialisation.
 * Refused before any launch: the argument checks of cadre_ppo_demo_loss, NULL row_kind, sil_losses, sil_w or sil_scratch,
 * by-value coefficients that are not finite, an inv_bs that is not finite and > 0 when hp, a non-zero coefficient or
 * sil_stats_row needs it, sil_F too small, a misaligned hp. */
#define CADRE_SIL_STATS_FIELDS 6
int cadre_ppo_sil_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                       const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                       const float* old_logp, const float* adv, const int32_t* row_kind, int32_t B, int32_t C,
                       int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip, float value_coeff, float clip_coeff,
                       float ent_coeff, float inv_b, float sil_coeff, float sil_value_coeff, float inv_bs, float* losses,
                       float* sil_losses, float* sil_w, float* dlogits, float* dvalues, float* scratch, float* sil_scratch,
                       const int32_t* poison, float* stats_row, int32_t F, float* stats_scratch, float target_kl, int32_t* stop,
                       float* sil_stats_row, int32_t sil_F, const int32_t* ord, void* stream);
/* cadre_sil_prepare: one launch for the n storages of a buffer slot, storage k belonging to head k & 1.  row_table = n records
 * of seven device pointers (int64) {rewards f32 [T + 1], masks f32 [T + 1], time_limits f32 [T + 1] or 0, value_preds f32
 * [T + 1], returns f32 [T + 1] (out), flags int32 [T + 1] (out), q uint32 [T + 1] (out)}.  2 <= T <= 3000.
 * Rewards are staged as cadre_gae_multi stages them (state NULL: raw; else clamp(r * (float)state[CADRE_RS_SCALE + head],
 * -clip_r, clip_r)), and the scan is cadre_gae_multi's with tau = 1 and V = 0, statement for statement in strict fp32:
 *   R_t = (r_t + (gamma m_t) R_{t+1}) (1 - time_limit_t),  R_T = 0.
 * A row is CLOSED when the nearest row t' >= t with m == 0 or a time-limit flag has m == 0 and no flag (its episode ended
 * inside the rollout by a true termination).  tail = 0 ("drop"): only closed rows are eligible.  tail = 1 ("bootstrap"): every
 * row is eligible, and the chains start from the stored values, R_T = value_preds[T] and R_t = value_preds[t] at a flagged
 * row; a closing row multiplies that start away, so R on closed rows carries the same bits under both settings.
 * Written for t < T: returns[t] = R_t, flags[t] = closed | eligible << 1, q[t] = quantise(fmaxf(R_t - value_preds[t], 0)) on
 * eligible rows and 0 elsewhere; flags[T] = 0 and q[T] = 0.  returns[T] is not written.
 * Refused before any launch: NULL table, n outside 1 .. 65535, T outside 2 .. 3000, gamma outside [0, 1], clip_r <= 0 with a
 * state, tail not 0 / 1, alpha not finite or <= 0, prio_eps not finite or < 0. */
int cadre_sil_prepare(const void* row_table, int32_t n, int32_t T, float gamma, const double* state, float clip_r, int32_t tail,
                      double alpha, double prio_eps, void* stream);
/* cadre_sil_draw: the prioritised draw, with replacement.  q uint32 [2][Rcap]; rows >= filled count as 0.  For head h, draw j:
 *   idx[h][j] = the smallest row r with cum[h][r] > (uint64)u[h][j] mod total[h],
 * cum the inclusive prefix sum of q[h] in uint64, total[h] = cum[h][filled - 1]: integers throughout, so the result does not
 * depend on the order of summation, and a row with q == 0 is never returned.  u int64 [2][n] non-negative random words, idx
 * int64 [2][n].  Three launches: sums of blocks of 1024 rows, their scan, one wave per draw.  scratch: 4 * ceil(Rcap / 1024) + 2
 * uint64, no initialisation.  The caller guarantees total[h] >= 1 (a head without an eligible row gets idx 0).
 * Refused before any launch: NULL q, u, idx or scratch, Rcap outside 1 .. 2^30, filled outside 1 .. Rcap, n outside 1 .. 65535. */
int cadre_sil_draw(const uint32_t* q, int64_t Rcap, int64_t filled, const int64_t* u, int32_t n, int64_t* idx, uint64_t* scratch,
                   void* stream);
/* cadre_sil_scatter: after the step, q[h][idx[h][j]] = quantise(fmaxf(sil_w[h][pos[h * B + B_ppo + j]], 0)) for j < n — SIL row
 * j is unsorted row B_ppo + j of the minibatch, pos as cadre_mix_row_kinds takes it (NULL: the identity).  A row drawn twice
 * gets the same value twice.  An index outside 0 .. Rcap - 1 or a position outside 0 .. B - 1 writes nothing.
 * Refused before any launch: NULL q, idx or sil_w, Rcap < 1, n < 1, B < 1, B_ppo < 0, B_ppo + n > B, alpha not finite or <= 0,
 * prio_eps not finite or < 0. */
int cadre_sil_scatter(uint32_t* q, int64_t Rcap, const int64_t* idx, int32_t n, const float* sil_w, const int32_t* pos, int32_t B,
                      int32_t B_ppo, double alpha, double prio_eps, void* stream);

/* ---------------------------------------------------------------- temporal action smoothness (csrc/smooth.hip)
 * Mysore et al. 2021, "Regularizing Action Policies for Smooth Control" (CAPS), the temporal term: the squared distance between
 * the policy's mean control at consecutive states, differentiated into both rows.  Successor rows (row t + 1 of a worker's own
 * storages) ride behind the workers' rows of a minibatch; this is the first loss here that couples two rows.
 *   c      float32 [2][64]: the control value of each bin per head (host-built; none is built into the kernels)
 *   mu     = sum_k p_k c_k of a row (p: the policy's probabilities, an ordinal head through ordinal.h first), one wave sum with
 *            every product and sum rounded on its own, lanes >= K contributing 0
 *   d      = mu(row t) - mu(row t + 1)
 *   total += smooth_coeff scale_head inv_bp sum over pair slots of d^2,   inv_bp = 1 / pair slots per step and head — invalid
 *            slots included, so the coefficient's meaning does not move with the number of valid pairs (cadre_ppo_sug_loss's rule)
 *
 * The pair (row t, row t + 1) of a storage is VALID iff t <= T - 2, masks[t] != 0 (the factor cadre_gae_multi multiplies V[t + 1]
 * by in row t's delta), time_limits[t] == 0 (NULL: no cuts), command[t] == command[t + 1] in 0 .. C - 1.  One device function
 * states this for cadre_smooth_mates and cadre_action_jitter.
 *
 * cadre_smooth_mates: one launch after the gather / sort (where cadre_suggest_rows runs), outside the captured graph.  The
 * minibatch has nW worker entries and E successor entries (1 <= E <= nW) of Bw rows; successor entry k belongs to worker
 * (rotation + k) mod nW.  src_table = 2 nW records of three device pointers (int64) {masks f32 [T + 1], time_limits f32 [T + 1]
 * or 0, command int32 [T + 1]}, record 2 w + head; idx = the step's staged index block int64 [2 (nW + E)][Bw], row 2 entry + head.
 * Slot (worker w, row r) is valid iff the pair at t = idx[2 w + head][r] is valid and idx[2 (nW + k) + head][r] == t + 1.
 *   row_kind int32 [2][Bt]  in workspace order (through pos [2][Bt]; NULL: the identity): 0 a PPO row, 1 a successor row
 *   mate     int32 [2][Bt]  in workspace order: the partner's workspace position; -1 on both rows of an invalid slot and on the
 *                           rows of a worker without a successor entry this step
 * Both arrays are overwritten completely.  Refused before any launch: a NULL table, idx, row_kind or mate, nW outside 1 .. 16384,
 * E outside 1 .. nW, Bw < 1, T < 2, C < 1, rotation < 0, Bt != (nW + E) Bw. */
int cadre_smooth_mates(const void* src_table, const int64_t* idx, int32_t nW, int32_t E, int32_t Bw, int32_t T, int32_t C,
                       int64_t rotation, const int32_t* pos, int32_t Bt, int32_t* row_kind, int32_t* mate, void* stream);
/* cadre_ppo_smooth_loss: ONE loss launch where cadre_ppo_loss_ord / cadre_ppo_sil_loss stand in the update — the same addressing,
 * grid (one wave per row, 16 rows per workgroup), `scratch` protocol (arrival counter zero on entry and left zero, partials
 * combined by the last arriving workgroup in workgroup order: equal inputs give equal bits), `poison`, rank table `ord`,
 * hp-or-by-value scalars and stats / target_kl / stop.  row_kind, mate int32 [2][B] as cadre_smooth_mates writes them.
 *   kind 0, mate < 0   exactly the statements of cadre_ppo_loss_ord, bit for bit
 *   kind 0, mate >= 0  those statements; then the wave reads the mate's logits row (the mate's own command net and position),
 *                      forms mu_mate with the device function that forms mu_own, and adds, with d_own = mu_own - mu_mate,
 *                        dlogits_k += (smooth_coeff scale_head inv_bp) (2 d_own) p_k (c_k - mu_own)
 *                      (the sum of both gradients goes through ord_backward once on an ordinal head) and d^2 to the smoothness
 *                      sum: only the kind-0 partner counts the pair
 *   kind 1, mate >= 0  the smoothness gradient only (CAPS does not stop the gradient), dvalues = 0; old_values, old_logp, adv,
 *                      returns, actions and values of the row are not read
 *   kind 1, mate < 0, or a command out of range: zeros everywhere the row owns.  A mate outside 0 .. B - 1 or with a command out
 *   of range counts as no mate.  Other nets' dlogits / dvalues rows are zeroed as cadre_ppo_sil_loss does.
 * The PPO sums, losses[3], the PPO diagnostics, the KL gate and the adaptive lr see the kind-0 rows only, without the smoothness term.
 *   smooth_losses[1]  sum over heads of (smooth_coeff scale_head inv_bp) sum d^2
 *                     total = losses[0] + losses[1] - losses[2] + smooth_losses[0]
 *   smooth_d [2][B]   each row's d_own, 0 for an unpaired row; the two partners' entries are exact negatives of each other
 * smooth_coeff is the by-value argument, or (float)hp[CADRE_HP_SMOOTH_COEFF] when hp is not NULL; scale_steer / scale_throttle
 * are by value always.
 * smooth_stats_row (may be NULL) float [2][smooth_F], smooth_F >= CADRE_SMOOTH_STATS_FIELDS, per head:
 *   0 valid pairs   1 inv_bp sum |d|   2 max |d|   3 inv_bp sum d^2
 * smooth_scratch (always required): 2 * ceil(B / 16) * CADRE_SMOOTH_STATS_FIELDS floats; it needs no initialisation.
 * Refused before any launch: the argument checks of cadre_ppo_sil_loss, NULL row_kind, mate, ctrl, smooth_losses, smooth_d or
 * smooth_scratch, a by-value smooth_coeff that is not finite, a scale that is not finite and >= 0, an inv_bp that is not finite
 * and > 0, smooth_F too small, a misaligned hp. */
#define CADRE_SMOOTH_STATS_FIELDS 4
int cadre_ppo_smooth_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                          const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                          const float* old_logp, const float* adv, const int32_t* row_kind, const int32_t* mate, const float* ctrl,
                          int32_t B, int32_t C, int32_t n_out_steer, int32_t n_out_throttle, double* hp, float clip,
                          float value_coeff, float clip_coeff, float ent_coeff, float inv_b, float smooth_coeff, float scale_steer,
                          float scale_throttle, float inv_bp, float* losses, float* smooth_losses, float* smooth_d, float* dlogits,
                          float* dvalues, float* scratch, float* smooth_scratch, const int32_t* poison, float* stats_row, int32_t F,
                          float* stats_scratch, float target_kl, int32_t* stop, float* smooth_stats_row, int32_t smooth_F,
                          const int32_t* ord, void* stream);
/* cadre_action_jitter: what the rollouts did.  One launch for n storages (storage k belongs to head k & 1), one wave each:
 * src_table = n records of four device pointers (int64) {action int64 [T + 1], masks f32 [T + 1], time_limits f32 [T + 1] or 0,
 * command int32 [T + 1]}.  out float64 [n][3]: the valid pairs t = 0 .. T - 2 (the rule above; an action outside 0 .. K - 1 makes
 * the pair invalid), sum |c[a_{t+1}] - c[a_t]| and its max.  The terms are fp32 differences widened to double; lane l adds the
 * terms of t = l, l + 64, ... in ascending order and the lanes are combined by the xor tree (32, 16, .. 1): a fixed order.
 * Refused before any launch: a NULL table, ctrl or out, n outside 1 .. 65535, T < 2, C < 1, bins outside 1 .. 64, a misaligned out. */
int cadre_action_jitter(const void* src_table, int32_t n, int32_t T, int32_t C, int32_t n_out_steer, int32_t n_out_throttle,
                        const float* ctrl, double* out, void* stream);

/* ---------------------------------------------------------------- ensemble evaluation (csrc/ensemble.hip)
 * eval.py:53-63 for N environments and M snapshots.  A group of Mg agents (Mg * C <= 16) shares one stacked arena with
 * Mg * C commands: agent j's net (head h, command c) is arena net h * Mg * C + j * C + c, and O3 [2 * 2 Mg C][z_str] is
 * that arena's tower output on the N sorted rows (row pitch ldo).
 * cadre_sample_rows_ens: cadre_sample_rows / _ord for every (environment e, group agent j < Mg, head h), one wave each,
 * the same statements: the actor row is tower z = 2 * (h * Mg * C + j * C + cmd[e]) at row pos[e], the critic z + 1.
 * q [N][M][2][64] (agent m0 + j of the M of the whole ensemble); q == NULL is the greedy pick: the divisor is exactly
 * 1.0f, the lowest index among the largest probabilities wins.  ord: NULL, or both heads' rank tables int32 [2][64] as
 * in cadre_sample_rows_ord.  action i64 / logp / value f32 [N][M][2] are written at agent m0 + j only; an environment
 * whose cmd or pos is out of range is skipped. */
int cadre_sample_rows_ens(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd, int32_t N,
                          int32_t C, int32_t Mg, int32_t m0, int32_t M, const float* q, int32_t K_steer, int32_t K_throttle,
                          int64_t* action, float* logp, float* value, const int32_t* ord, void* stream);
/* CadreAgent.avg_action (agent.py:83-95) per environment: action i64 [N][M][2] (steer bin, throttle bin), steer_tab f64
 * [K_steer], throttle_tab f64 [K_throttle][2] (throttle, brake) -> controls f64 [N][3] = (steer, throttle, brake).  Each
 * column is summed in float64 in agent order 0 .. M-1 and divided by (double)M (numpy's mean(0), bit for bit); with
 * M > 1 a brake < 0.5 becomes 0.  A bin outside its table gives NaN for that environment's three controls; no table is
 * read out of bounds. */
int cadre_ensemble_controls(const int64_t* action, int32_t N, int32_t M, const double* steer_tab, int32_t K_steer,
                            const double* throttle_tab, int32_t K_throttle, double* controls, void* stream);

/* Initial LSTM state of every net z < Z: Hs[z*z_str ..] <- h0[(z / x_div)*n_per ..], same for Cs <- c0 (n_per floats
 * each, agent.py:166-175 hidden_state_batch shared by a head's command nets) and dC (Z*n_per floats, may be NULL) <- 0 */
int cadre_lstm_init(const float* h0, const float* c0, float* Hs, float* Cs, float* dC, int64_t n_per,
                    int64_t z_str, int32_t x_div, int32_t Z, void* stream);

/* ---------------------------------------------------------------- optimiser
 * chief.py:13-21 + main.py:55: per-model clip_grad_norm_(max_norm) then Adam (torch defaults)
 * over a flat parameter arena made of `n_models` segments [seg_off[i], seg_off[i+1]).
 * norms2 is f64 [n_models] scratch (zeroed inside). */
int cadre_clip_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                    const int64_t* seg_off, int32_t n_models, double* norms2, double max_norm,
                    double lr, double beta1, double beta2, double eps, int32_t step, void* stream);

/* Same math, hipGraph-capturable: the 1-based step counter is *step_dev (device int32,
 * incremented by the call); norms2 must hold n_models + 2 doubles. */
int cadre_clip_adam_graph(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                          const int64_t* seg_off, int32_t n_models, double* norms2, double max_norm,
                          double lr, double beta1, double beta2, double eps, int32_t* step_dev,
                          void* stream);


/* cadre_clip_adam_graph that ALSO maintains the fragment-order copies of the recurrent weights (cadre_pack_lstm_weights'
 * `fwd` / `bwd`, net stride p_str): models 0 .. n_lstm-1 are LSTM blocks of lstm_str floats whose W_hh [H4 = 4 D][ldw = 544]
 * starts o_whh floats into the block.  The thread that steps a 4 x 4 block of W_hh stores it into both copies, so the
 * update needs no packing launch after an optimiser step (chief.py:13-21 + models.py:139-152's weights for the next step).
 * Same parameters, bit for bit, as cadre_clip_adam_graph followed by cadre_pack_lstm_weights. */
int cadre_clip_adam_pack_graph(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                               const int64_t* seg_off, int32_t n_models, double* norms2, double max_norm, double lr,
                               double beta1, double beta2, double eps, int32_t* step_dev, int32_t n_lstm,
                               int64_t lstm_str, int64_t o_whh, int32_t H4, int32_t ldw, int32_t D, float* fwd,
                               float* bwd, int64_t p_str, void* stream);

/* Gated twins of cadre_clip_adam_graph / cadre_clip_adam_pack_graph (the target_kl early stop): `stop` is the device flag of
 * cadre_ppo_loss_stats.  While *stop != 0 the step writes no parameter, exp_avg, exp_avg_sq or weight copy and leaves
 * *step_dev as it is; the per-model square norms are still computed into norms2.  With *stop == 0 the result is bit-identical
 * to the ungated entry point. */
int cadre_clip_adam_graph_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                const int64_t* seg_off, int32_t n_models, double* norms2, double max_norm,
                                double lr, double beta1, double beta2, double eps, int32_t* step_dev,
                                const int32_t* stop, void* stream);
int cadre_clip_adam_pack_graph_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                     const int64_t* seg_off, int32_t n_models, double* norms2, double max_norm, double lr,
                                     double beta1, double beta2, double eps, int32_t* step_dev, int32_t n_lstm,
                                     int64_t lstm_str, int64_t o_whh, int32_t H4, int32_t ldw, int32_t D, float* fwd,
                                     float* bwd, int64_t p_str, const int32_t* stop, void* stream);

/* Data-parallel ranks with a reduce-scattered gradient arena (reference semantics chief.py:13-21: SUM
 * over workers, per-model clip, Adam): this rank owns arena elements [rlo, rhi) (multiples of 4).
 * cadre_clip_adam_norms: increments *step_dev, stores the step's bias-correction scalars in norms2[n_models..+2) and
 * leaves the PARTIAL per-model square norms of grads[rlo..rhi) in norms2[0..n_models) — the caller all-reduces those
 * n_models doubles (SUM) over the ranks.  cadre_clip_adam_apply: clip + Adam on the shard; exp_avg / exp_avg_sq hold
 * the shard's state only (rhi - rlo floats each, element i of the arena at [i - rlo]); params / grads are the full
 * arenas.  The caller then all-gathers the parameter shards.  With [0, total) the pair equals cadre_clip_adam_graph. */
int cadre_clip_adam_norms(const float* grads, const int64_t* seg_off, int32_t n_models, double* norms2, double lr,
                          double beta1, double beta2, int32_t* step_dev, int64_t rlo, int64_t rhi, void* stream);
int cadre_clip_adam_apply(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                          const int64_t* seg_off, int32_t n_models, const double* norms2, double max_norm,
                          double beta1, double beta2, double eps, int64_t rlo, int64_t rhi, void* stream);


/* Hyper-parameter block forms of the optimiser entry points above: lr = hp[CADRE_HP_LR] (read by the preparation kernel,
 * the only place lr enters the step) and max_norm = (float)hp[CADRE_HP_MAX_GRAD_NORM] at run time; everything else as in
 * the by-value sibling, and bit-identical to it for equal values. */
int cadre_clip_adam_graph_hp(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                             const int64_t* seg_off, int32_t n_models, double* norms2, const double* hp,
                             double beta1, double beta2, double eps, int32_t* step_dev, void* stream);
int cadre_clip_adam_graph_hp_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                   const int64_t* seg_off, int32_t n_models, double* norms2, const double* hp,
                                   double beta1, double beta2, double eps, int32_t* step_dev, const int32_t* stop,
                                   void* stream);
int cadre_clip_adam_pack_graph_hp(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                  const int64_t* seg_off, int32_t n_models, double* norms2, const double* hp,
                                  double beta1, double beta2, double eps, int32_t* step_dev, int32_t n_lstm,
                                  int64_t lstm_str, int64_t o_whh, int32_t H4, int32_t ldw, int32_t D, float* fwd,
                                  float* bwd, int64_t p_str, void* stream);
int cadre_clip_adam_pack_graph_hp_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                        const int64_t* seg_off, int32_t n_models, double* norms2, const double* hp,
                                        double beta1, double beta2, double eps, int32_t* step_dev, int32_t n_lstm,
                                        int64_t lstm_str, int64_t o_whh, int32_t H4, int32_t ldw, int32_t D,
                                        float* fwd, float* bwd, int64_t p_str, const int32_t* stop, void* stream);
int cadre_clip_adam_norms_hp(const float* grads, const int64_t* seg_off, int32_t n_models, double* norms2,
                             const double* hp, double beta1, double beta2, int32_t* step_dev, int64_t rlo, int64_t rhi,
                             void* stream);
int cadre_clip_adam_apply_hp(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                             const int64_t* seg_off, int32_t n_models, const double* norms2, const double* hp,
                             double beta1, double beta2, double eps, int64_t rlo, int64_t rhi, void* stream);

/* ---------------------------------------------------------------- rollout finishing (csrc/rollout_finish.hip)
 * The stage between a rollout and its update for all n storages of a learner section.  row_table: device array of n
 * records of seven pointers {rewards, value_preds, masks [T+1], next_value [1], returns [T+1], advantages [T],
 * time_limits [T+1] or NULL}, all f32; storage k belongs to head k & 1 (steer, throttle).  2 <= T <= 3000.
 *
 * Return-statistics state: one block of 8 + 2 n doubles,
 *   [3 h + 0 .. 2]             count, mean, M2 of the discounted returns head h has seen          (CADRE_RS_STATS)
 *   [CADRE_RS_SCALE + h]       the reward scale of head h: a float32 value held in a double slot, initially 1
 *   [CADRE_RS_CARRY + 2 k + 0] G of the last row of storage k's previous rollout, initially 0
 *   [CADRE_RS_CARRY + 2 k + 1] m' of that row, initially 0
 * and a scratch of 1 + 2 n doubles, zero before the first launch (a ticket and the per-storage partials).
 *
 * cadre_return_stats: for every storage, over rows 0 .. T-1 in slot order, G_t = r_t + gamma m'_{t-1} G_{t-1} in fp64,
 * m' = mask (1 - time_limit), carries read from and written back to the block; the T values of a storage give a
 * two-pass (mean, M2), the storages of a head are merged into the head's statistics with Chan's formula in storage
 * order (a fixed order: equal inputs give equal bits), and then scale_h = float32(1 / sqrt(M2_h / count_h + epsilon)) is
 * stored.  n even.  With update == 0 nothing is launched: statistics, carries and scale stay as they are. */
#define CADRE_RS_STATS 0
#define CADRE_RS_SCALE 6
#define CADRE_RS_CARRY 8
int cadre_return_stats(const void* row_table, int32_t n, int32_t T, double gamma, double epsilon, int32_t update,
                       double* state, double* scratch, void* stream);
/* cadre_gae for every storage of the table in one launch (one workgroup per storage; next_value is read from the
 * record, value_preds[T] is overwritten with it): the same arithmetic in the same order, so with time_limits NULL and
 * state NULL the returns, advantages and value_preds[T] are bit-identical to n cadre_gae launches.
 * time_limits: after `gae = delta + gamma_tau m gae` of row t, gae = gae * (1 - time_limit[t]) — a cut row has
 * returns[t] == value_preds[t] and advantage 0 before normalisation (it still counts in the mean / std), the chain
 * restarts behind it and row t - 1 bootstraps from value_preds[t].
 * state (may be NULL: no reward scaling): the block of cadre_return_stats; a staged reward becomes
 * clamp(r * (float)state[CADRE_RS_SCALE + head], -clip_r, clip_r), one fp32 multiply, then the clamp.  The rewards
 * array itself is not written. */
int cadre_gae_multi(const void* row_table, int32_t n, int32_t T, float gamma, float gamma_tau, int32_t normalise,
                    const double* state, float clip_r, void* stream);
/* cadre_insert_rows whose records carry a tenth pointer, time_limits f32 [T+1], and whose rm is [n_dst][3]:
 * reward, mask, time-limit flag (0 or 1) of the row. */
int cadre_insert_rows_tl(const void* dst_table, const int32_t* slot, int32_t n_dst, int32_t S, int64_t ldo, int64_t ldh,
                         int32_t D, int32_t Hd, int32_t T, const float* feat, int64_t ldf, const int64_t* action,
                         const float* logp, const float* value, const float* rm, const int32_t* cmd, void* stream);

/* ---------------------------------------------------------------- sample reuse (csrc/reuse.hip)
 * The rows of the last few rollouts ride in the PPO step as further worker entries (GePPO, Queeney et al. 2021, with the
 * V-trace targets of Espeholt et al. 2018).  The GePPO surrogate with rho = pi / mu and clip centre pi_k / mu equals
 * (pi_k / mu) min(r A, clip(r, 1 - eps, 1 + eps) A) with r = pi / pi_k, so the cadre_ppo_loss* kernels compute it once a stale
 * row's old_logp is its log-probability under the policy at the start of the update (cadre_reuse_record) and its advantage
 * carries the truncated weight min(rho_bar, pi_k / mu) (cadre_vtrace_multi).
 *
 * cadre_reuse_record: the addressing and grid of cadre_aux_record, plus values (row pitch ldv, net stride v_ns) and actions
 * int64 [2][B] in workspace order as cadre_ppo_loss reads them.  For head h and unsorted row u with b = pos[h][u],
 * c = commands[h][b] in 0 .. C - 1 and r = row_id[h][u] in 0 .. R - 1:
 *   value_now[h][r] = values[net h C + c][b]                              (the same bits)
 *   logp_now[h][r]  = lg_a = x_a - logsumexp(x),  a = actions[h][b]       (only when a is in 0 .. K - 1)
 * with x the own net's logits at workspace row b (an ordinal head: through ord_logits) and lg_a formed by exactly the
 * statements that form lp in the loss kernels: the same logits fed to cadre_ppo_loss* with old_logp := logp_now give
 * lp - old_logp == 0 and ratio == 1 exactly.  logp_now, value_now: float [2][R].  An action out of range (the bootstrap row of
 * a storage has none) writes the value only; a row with b, c or r out of range writes nothing.  Two rows of one launch with the
 * same r race as in cadre_aux_record.  Refused before any launch: NULL logits, values, commands, actions, row_id, logp_now or
 * value_now, B < 1, C < 1, n_out outside 1 .. 64, ldl < n_out or > 64, ldv < 1, R < 1.
 *
 * cadre_vtrace_multi: cadre_gae_multi for stale storages.  row_table: device array of n records of eleven pointers
 * {rewards [T+1], masks [T+1], time_limits [T+1] or NULL, value_now [T+1], boot_keep [1], behaviour_logp [T], logp_now [T],
 * returns [T], advantages [T], ratio [T], diag [CADRE_VTRACE_DIAG_FIELDS]}, all f32; storage k belongs to head k & 1.
 * 2 <= T <= 3000 (five arrays of T + 1 floats in LDS, as cadre_gae_multi).  Rewards are read as cadre_gae_multi reads them
 * (state, clip_r).  V = value_now with V[T] = boot_keep != 0 ? value_now[T] : 0 (a select; value_now[T] is overwritten with it).
 * Per row  ratio_t = expf(logp_now[t] - behaviour_logp[t])  (stored),  rho_t = fminf(rho_bar, ratio_t),
 * cw_t = fminf(c_bar, ratio_t).  For t = T - 1 .. 0, acc = 0 at the start, one rounded fp32 operation per statement, no FMA:
 *   t1 = gamma V[t+1]   t2 = t1 m[t]   t3 = r[t] + t2   delta = t3 - V[t]   u1 = gamma_tau m[t]
 *   a2 = u1 acc   A = delta + a2   A = A keep[t]                  (policy advantage: GAE with the V-trace-corrected tail)
 *   rd = rho_t delta   uc = u1 cw_t   u2 = uc acc   acc = rd + u2   acc = acc keep[t]
 *   returns[t] = acc + V[t]                                        (the V-trace value target v_s)
 *   p = A + V[t]   a_t = p - V[t]                                  (the round trip cadre_gae_multi's advantage makes)
 * The a_t are normalised per storage as cadre_gae_multi normalises (double sums, unbiased std, + 1e-8f; cut rows count), and
 * the last statement is advantages[t] = a_norm_t rho_t (a_t rho_t with normalise == 0).  With logp_now == behaviour_logp,
 * rho_bar >= 1 and c_bar >= 1 every factor is exactly 1 and returns, advantages and value_now[T] are cadre_gae_multi's bits.
 * diag, sums in double, stored as float: 0 mean ratio   1 share of rows with ratio > rho_bar   2 max |logp_now - behaviour_logp|
 * 3 effective-sample share (sum rho)^2 / (T sum rho^2).
 * Refused before any launch: what cadre_gae_multi refuses; rho_bar or c_bar not finite or not > 0. */
#define CADRE_VTRACE_DIAG_FIELDS 4
int cadre_reuse_record(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                       const int32_t* commands, const int64_t* actions, const int32_t* pos, const int64_t* row_id, int32_t B,
                       int32_t C, int32_t n_out_steer, int32_t n_out_throttle, const int32_t* ord, float* logp_now,
                       float* value_now, int32_t R, void* stream);
int cadre_vtrace_multi(const void* row_table, int32_t n, int32_t T, float gamma, float gamma_tau, int32_t normalise,
                       const double* state, float clip_r, float rho_bar, float c_bar, void* stream);

/* ---------------------------------------------------------------- rank consensus (csrc/consensus.hip)
 * Decisions that several data-parallel ranks must take identically.  The caller sums the inputs over the ranks first (one
 * small all-reduce); every rank then runs the same kernel on the same reduced bits.  Sums, not means: R ranks with N workers
 * each decide what one rank with R N workers decides.
 *
 * cadre_kl_consensus: one workgroup, one deciding lane, the rule the last arriver of cadre_ppo_loss_stats[_hp] applies
 * (csrc/kl_rule.h, the same function, the same types).  kl: device float[2], the reduced approx_kl of steer and throttle.
 * *stop is sticky; target_kl > 0 and fmaxf(kl[0], kl[1]) > 1.5f * target_kl sets it; applied = (*stop == 0) after the check
 * goes to stats_row[6] and stats_row[F + 6] (stats_row may be NULL; no other field is written).  Then, unless stopped and when
 * desired_kl > 0, the double-precision lr rule of cadre_ppo_loss_stats_hp runs on hp[CADRE_HP_LR] with hp[CADRE_HP_LR_MIN],
 * hp[CADRE_HP_LR_MAX] and hp[CADRE_HP_LR_FACTOR]; desired_kl is the by-value argument, hp[CADRE_HP_DESIRED_KL] is not read
 * (the caller keeps it 0 so that the loss kernel does not adapt on its own).  No other hp field is written.
 * NaN: fmaxf ignores a NaN operand, so a head with a NaN KL does not count; with both NaN every comparison is false, the flag
 * is not set and lr does not move — as in the loss kernel.
 * Refused before any launch: NULL kl, target_kl negative or NaN, target_kl > 0 without stop, desired_kl > 0 without hp,
 * stats_row with F < CADRE_PPO_STATS_FIELDS. */
int cadre_kl_consensus(const float* kl, float target_kl, int32_t* stop, double desired_kl, double* hp, float* stats_row,
                       int32_t F, void* stream);
/* cadre_return_scale_merge: stats = device double [world][6], per rank the (count, mean, M2) of head 0 then head 1 (the
 * first six doubles of that rank's return-statistics state).  Per head the ranks are merged with Chan's formula in rank
 * order 0 .. world - 1 from an empty accumulator, ranks with count 0 skipped, and
 * state[CADRE_RS_SCALE + h] = float32(1 / sqrt(M2 / count + epsilon)) is stored — the expression and rounding of
 * cadre_return_stats.  While the merged count is 0 the scale slot is left as it is (initially 1).  Nothing else of `state`
 * is written: the rank's own statistics and carries stay.  merged (may be NULL): receives the six merged doubles.
 * Refused before any launch: NULL stats or state, world < 1, epsilon negative, NaN or infinite. */
int cadre_return_scale_merge(const double* stats, int32_t world, double epsilon, double* state, double* merged, void* stream);

/* ---------------------------------------------------------------- training checkpoints (csrc/checkpoint.hip)
 * cadre_state_capture: ONE launch copies n_ranges device ranges into one staging buffer and forms one 64-bit digest per
 * range from the same read (each source word is read once, each staging word written once; the digest costs no further
 * memory traffic).  range_table: device array of n_ranges records {const void* src; int64_t dst_off; int64_t bytes}
 * (24 bytes each); range k goes to (char*)staging + dst_off and its digest to digests[k].  bytes is a multiple of 4 (every
 * piece of state is fp32, fp64, int32 or int64); src and staging + dst_off need 4-byte alignment only: 16-byte accesses
 * are used where the alignment allows, with a word-wise head and tail.  staging == NULL: digests only (verification of
 * an uploaded checkpoint).  The digest slots are zeroed on `stream` before the launch.
 *
 * Digest of the 32-bit words w_0 .. w_{n-1} of a range, all arithmetic mod 2^64, i a 64-bit index:
 *     D = sum_i (uint64(w_i) + 1) * ((2 i + 1) * 0x9E3779B97F4A7C15)
 * Wrap-around addition is associative and commutative: the partial sums of lanes, waves and workgroups give the same
 * bits in any order, so equal bytes give equal digests in every launch.  The multiplier is odd (every single-bit flip
 * changes D) and the + 1 makes the length count.  This is an INTEGRITY check against corruption and mix-ups, NOT a
 * cryptographic hash: it is trivially forgeable.
 *
 * Status: the arguments the host can see are checked (0 <= n_ranges <= CADRE_CAPTURE_MAX_RANGES, non-NULL table and
 * digests of 8-byte alignment, staging of 4-byte alignment) and refused with a negative status.  The table lives in
 * device memory; a record the launch finds malformed (bytes negative or no multiple of 4, src or dst_off off a 4-byte
 * boundary) is not copied and its digest slot is set to CADRE_CAPTURE_BAD_RANGE.  cadre_amd.hip.capture_table refuses
 * such records on the host before a table is built. */
#define CADRE_CAPTURE_MAX_RANGES 65535
#define CADRE_CAPTURE_BAD_RANGE 0xFFFFFFFFFFFFFFFFull
int cadre_state_capture(const void* range_table, int32_t n_ranges, void* staging, uint64_t* digests, void* stream);

/* ---------------------------------------------------------------- frame-table storages (csrc/frame_table.hip)
 * A storage may keep every distinct frame row once, frames f32 [F][ldo], and its windows as frame ids, win int32 [T+1][S],
 * in place of the materialised rows obs [T+1][S][ldo].  The four gathers above have a twin each that takes the ids:
 *     win == NULL   a materialised source: window row (t, s) is read at obs + (t * S + s) * ldo, exactly as the twin reads it
 *     win != NULL   obs is the frame table and window row (t, s) is read at obs + win[t * S + s] * ldo
 * Everything else is the statement of the twin: placement and sort rank, pos / seg, h0 / c0 / scalars, the zero pad up to
 * ldx — the outputs are bit-identical for equal content.  A frame id outside [0, n_frames) reads nothing and gives NaN in
 * columns 0 .. D-1 of its row (the pad stays zero), as cadre_demo_rows treats it.  Rows move 16 bytes per lane when ldo and
 * ldx are multiples of 4 floats and the source base and the destination (of the head) are 16-byte aligned; else element by
 * element.
 * The multi forms: src_table holds n_src records of ELEVEN 8-byte words — the nine pointers of the records above, then
 * `const int32_t* win` and `int64_t n_frames` (the count rides in the record: one table, one cache key; not read where win
 * is NULL).  Materialised and frame-table sources may stand in one table. */
int cadre_gather_obs_ft(const float* obs, const int32_t* win, int64_t n_frames, int64_t ldo, int32_t S, const int64_t* idx,
                        int32_t B, float* x, int64_t ldx, int32_t D, void* stream);
int cadre_gather_minibatch_ft(const float* obs, const int32_t* win, int64_t n_frames, int64_t ldo, int32_t S, const float* hn,
                              const float* cn, int64_t ldh, const int64_t* action, const float* value_preds,
                              const float* returns, const float* logp, const int32_t* command, const float* adv,
                              const int64_t* idx, int32_t B, int32_t D, int32_t Hd, int32_t Bt, int32_t b0, float* X,
                              int64_t ldx, float* h0, float* c0, int64_t ldho, int64_t* actions_o, int32_t* commands_o,
                              float* old_values_o, float* returns_o, float* old_logp_o, float* adv_o, void* stream);
int cadre_gather_minibatch_multi_ft(const void* src_table, int32_t n_src, int64_t ldo, int32_t S, int64_t ldh,
                                    const int64_t* idx, int32_t Bw, int32_t D, int32_t Hd, int32_t Bt, float* X,
                                    int64_t x_head_stride, int64_t ldx, float* h0, float* c0, int64_t h_head_stride,
                                    int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                                    float* returns_o, float* old_logp_o, float* adv_o, void* stream);
int cadre_gather_sorted_multi_ft(const void* src_table, int32_t n_src, int64_t ldo, int32_t S, int64_t ldh,
                                 const int64_t* idx, int32_t Bw, int32_t D, int32_t Hd, int32_t Bt, int32_t C, float* X,
                                 int64_t x_head_stride, int64_t ldx, float* h0, float* c0, int64_t h_head_stride,
                                 int64_t ldho, int64_t* actions_o, int32_t* commands_o, float* old_values_o,
                                 float* returns_o, float* old_logp_o, float* adv_o, int32_t* pos, int32_t* seg, void* stream);
/* Packing materialised storages into frames (buffers filled from live rollouts, whose rows carry no frame identity).
 * cadre_frames_scan: src_table = n device pointers to obs [P][S][ldo] (P rows per storage, 1 <= S <= 16).  Per storage z and
 * window row (t, s), rows compared as 32-bit patterns over columns 0 .. D-1 only (the pad is ignored, -0.0 differs from
 * +0.0, identical NaN bits are equal):
 *     1. t > 0, s < S-1 and row (t, s) equals row (t-1, s+1): flags = 1, it takes that row's id (the window slid)
 *     2. else s > 0 and it equals row (t, s-1): flags = 2, it takes that row's id (a reset filled the window with one frame)
 *     3. else flags = 0, a new frame: id = the number of new rows of the storage before it in (t, s) order
 * flags, win_local int32 [n][P][S]; count int32 [n] = the new rows of each storage.  Two launches: the compares (one wave per
 * window row), then the ids (one wave per storage, serial in t).
 * cadre_frames_copy: every new row goes to frames[base[z] + id] (ld floats: columns 0 .. D-1 as they are, zeros up to ld; a
 * row at or past F_cap is not written) and every window row's global id to win_dst[(row0[z] + t) * S + s] = base[z] + id.
 * base, row0: device int32 [n], filled by the host after it read `count`. */
int cadre_frames_scan(const void* src_table, int32_t n, int32_t P, int32_t S, int64_t ldo, int32_t D, int32_t* flags,
                      int32_t* win_local, int32_t* count, void* stream);
int cadre_frames_copy(const void* src_table, int32_t n, int32_t P, int32_t S, int64_t ldo, int32_t D, const int32_t* flags,
                      const int32_t* win_local, const int32_t* base, float* frames, int64_t ld, int64_t F_cap,
                      int32_t* win_dst, const int32_t* row0, void* stream);

/* ---- decoder (csrc/deconv.hip): the reverse modules of the reference's visual branch (visual_branch.py:141-163), fp32.
 * cadre_deconv3x3_s2: out = act(ConvTranspose2d(Cin, Cout, 3, stride 2, padding 1, output_padding (oph, opw))(x) * scale + shift)
 * for Z independent modules in one launch.  Dense NHWC: x [Z][F][H][W][Cin] with module stride x_zstride floats (0: every
 * module reads the same input), out [Z][F][2H-1+oph][2W-1+opw][Cout], scale / shift [Z][Cout] (bias and eval-mode BatchNorm
 * folded by the host), act 0 none / 1 ReLU / 2 leaky ReLU(slope).  w [Z][9 * Cin * Cout]: per module the four output-parity
 * classes c = 2 py + px one after the other, class c as [Cout][tap][Cin] with tap = dy (1 + px) + dx over dy <= py,
 * dx <= px, holding the reference weight [Cin][Cout][ky][kx] at ky = 1 (py = 0), 2 (py = 1, dy = 0), 0 (py = 1, dy = 1),
 * kx alike (cadre_amd/decoder.py pack_deconv).  out[2m+py][2n+px] reads x[m+dy][n+dx]; every output is written once.
 * _supported: Cin % 32 == 0, Cout % 32 == 0, oph / opw in {0, 1}, every tensor below 2 GiB (host logic, no launch).
 * cadre_deconv3x3_s2_out: the last level, Cin = 32 -> Cout <= 8, bias only.  x [F][H][W][32]; w [3][3][32][CO] with CO = Cout
 * rounded up to a power of two and zeros past Cout (w[ky][kx][ci][co] = reference weight [ci][co][ky][kx]).  Outputs, each
 * NULL when not wanted: logits fp32 [F][Ho][Wo][Cout], cls u8 [F][Ho][Wo] = the first maximum over channels, sig fp32
 * [F][Ho][Wo] = sigmoid of channel 0 (Cout == 1 only).
 * cadre_argmax_rows: out[r] = index of the first maximum of x[r][0 .. n-1] (row pitch ld floats).
 * cadre_bc_head: out [F][2] = (steer, throttle) = bc_model(att_bc), att_bc = lat[f][256 .. 511] (+ in_bc_speed_fc(speed[f]) when speed
 * is not NULL); lat rows of ld >= 512 floats.  Reference weights as stored: sw1 [64][1], sb1 [64], sw2 [256][64], sb2 [256]
 * (in_bc_speed_fc.1 / .3), bw1 [128][256], bb1 [128], bw2 [2][128], bb2 [2] (bc_branch.bc_model.1 / .3); leaky ReLU(slope)
 * between.  One workgroup per row; each layer's output is fp32, its sum runs in double. */
int cadre_deconv3x3_s2_supported(int32_t Z, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t oph, int32_t opw);
int cadre_deconv3x3_s2(const float* x, int64_t x_zstride, const float* w, const float* scale, const float* shift, float* out,
                       int32_t Z, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t oph, int32_t opw,
                       int32_t act, float slope, void* stream);
int cadre_deconv3x3_s2_out(const float* x, const float* w, const float* bias, float* logits, uint8_t* cls, float* sig,
                           int32_t F, int32_t H, int32_t W, int32_t Cout, int32_t oph, int32_t opw, void* stream);
int cadre_argmax_rows(const float* x, int64_t ld, int32_t rows, int32_t n, int32_t* out, void* stream);
int cadre_bc_head(const float* lat, int64_t ld, const float* speed, const float* sw1, const float* sb1, const float* sw2,
                  const float* sb2, const float* bw1, const float* bb1, const float* bw2, const float* bb2, float* out, int32_t F,
                  float slope, void* stream);

/* ---- curiosity (csrc/curiosity.hip): random network distillation on the newest frame row of every window row, fp32 towers
 * on v_mfma_f32_32x32x2_f32.  Rows: r = w * T + t for worker w < N and storage row t < T; x = obs_w[t][S - 1][0 .. D-1], obs_table
 * = N device pointers to the workers' window rows [T + 1][S][ldo] (the steer storage's: both heads hold the same rows).
 * State block (float64): [CADRE_RND_N] rows merged into the feature statistics, [CADRE_RND_BETA] the bonus coefficient,
 * [CADRE_RND_EXT] the factor of the raw reward, [CADRE_RND_RHO_N / _MEAN / _M2] the running statistics of the carried error
 * sums, [CADRE_RND_SIGMA] sqrt(var + eps) of the last merge (1 before any), [CADRE_RND_KEY / _CTR] key and counter of the mask
 * generator (whole numbers below 2^32 / 2^53), then from CADRE_RND_HEAD: mu [D], M2 [D], carry [N].
 * A tower is one flat fp32 buffer: W1 [D][H], b1 [H], W2 [H][H], b2 [H], W3 [H][E], b3 [E] — every matrix input-major (row k
 * holds the weights that input k feeds), so the gradient buffer of cadre_rnd_backward has the same layout.  H and E are
 * multiples of 32, at most 256; 1 <= D <= 1024.
 * cadre_rnd_obs_stats: with `update`, merges the N T rows into {n, mu, M2} (Chan): per feature the batch mean and the batch sum
 * of squared deviations in two passes, rows summed in 16 interleaved groups, groups in order.  update == 0: no launch.  Columns
 * D .. ldo-1 and frames s < S - 1 are not read.
 * cadre_rnd_forward: rows row0 .. row0 + rows - 1.  xh = clamp((x - (float)mu) / (float)sqrt(M2 / n + eps_obs), -clip, clip)
 * (variance 1 while n == 0), then for the target and the predictor, one code path: h1 = relu(xh W1 + b1), h2 = relu(h1 W2 + b2),
 * o = h2 W3 + b3; err[i] = (sum_k (g_k - f_k)^2 in k order) / E for i = r - row0.  A row's result does not depend on the other
 * rows of the launch.  xh [rows][D], h1, h2 [rows][H], diff [rows][E] (g - f): the predictor's, each NULL when not wanted.
 * cadre_rnd_reward: one workgroup.  With `update`, per worker rho <- gamma rho + err[w][t] forward in time from the carry, the
 * N T values merged into the rho statistics, sigma = sqrt(M2 / n + eps), carries stored.  Then for storage k < 2 N (worker
 * k / 2) and t < T: mixed_k[t] = ext * rewards_k[t] + beta * (err[w][t] / (float)sigma).  row_table = 2 N records {rewards,
 * mixed} of device pointers; row T of `mixed` is not written.
 * cadre_rnd_backward: rows = the rows of one predictor step with their saved xh, h1, h2, diff and err.  m_i = 1 where the top 24
 * bits of splitmix64(key * 0x9E3779B97F4A7C15 + ctr + i) are below `thresh` (update_proportion * 2^24), cnt = sum m; the
 * counter then advances by `rows`.  loss[0] = sum m err / max(cnt, 1), loss[1] = cnt.  dO = 2 m diff / (E max(cnt, 1)); dW3 = h2^T
 * dO, dH2 = (dO W3^T) [h2 > 0], dW2 = h1^T dH2, dH1 = (dH2 W2^T) [h1 > 0], dW1 = xh^T dH1, db = column sums; every sum over rows runs
 * in row order inside one wave.  scratch: rows (E + 2 H + 1) + 2 floats.  Six launches, no atomics. */
#define CADRE_RND_N 0
#define CADRE_RND_BETA 1
#define CADRE_RND_EXT 2
#define CADRE_RND_RHO_N 3
#define CADRE_RND_RHO_MEAN 4
#define CADRE_RND_RHO_M2 5
#define CADRE_RND_SIGMA 6
#define CADRE_RND_KEY 7
#define CADRE_RND_CTR 8
#define CADRE_RND_HEAD 16
int cadre_rnd_obs_stats(const void* obs_table, int32_t N, int32_t T, int32_t S, int64_t ldo, int32_t D, int32_t update,
                        double* state, void* stream);
int cadre_rnd_forward(const void* obs_table, int32_t N, int32_t T, int32_t S, int64_t ldo, int32_t D, int32_t H, int32_t E,
                      int32_t row0, int32_t rows, const double* state, double eps_obs, float clip, const float* target,
                      const float* predictor, float* err, float* xh, float* h1, float* h2, float* diff, void* stream);
int cadre_rnd_reward(const float* err, int32_t N, int32_t T, const void* row_table, double* state, int32_t D, double gamma,
                     double eps, int32_t update, void* stream);
int cadre_rnd_backward(const float* xh, const float* h1, const float* h2, const float* diff, const float* err, int32_t rows,
                       int32_t D, int32_t H, int32_t E, const float* predictor, double* state, int32_t thresh, float* grads,
                       float* loss, float* scratch, void* stream);

/* ---------------------------------------------------------------- action masks (opt-in, csrc/actmask.h, csrc/actmask.hip)
 * Invalid-action masking (Huang & Ontañón 2020) for the two categorical / ordinal heads.  A row of a head carries one 64-bit
 * word `allowed` (int64 tensors, read as uint64): bit k set means bin k may be chosen.  The mask acts in BIN space, after the
 * ordinal transform where the head is ordinal: with on = lane < K and x the logit of bin `lane`,
 *   on_m = on && bit(lane)      x = on_m ? x : -inf
 * and the two softmax passes, the entropy, the probabilities and d total / d logit use on_m where the unmasked kernels use on
 * (ord_backward receives the masked gradient and the unmasked on).  A word with no bit set among the head's K bins means
 * "unmasked": all K bins allowed.  With every bit of the K bins set (or none) every output is bit-identical to the entry
 * point that is extended.  `ord` is required as in the `_ord` entry points (a marker table selects the categorical head).
 *
 * cadre_sample_am / cadre_sample_rows_am: cadre_sample_ord / cadre_sample_rows_ord with allowed int64 [R] / [N][2]
 * (environment order): argmax(p / q) over the allowed bins, lowest index on ties; q is read for all K bins; logp is the
 * masked log-probability of the chosen bin.
 * cadre_categorical_eval_am: cadre_categorical_eval_ord under allowed int64 [R]; the given action's bit is OR-ed in first.
 * cadre_allowed_note: allowed[k][slots[k]] = words[k] for n storages in one launch; table: device array of n pointers to the
 * storages' int64 [T + 1] tensors (0: skipped), 0 <= slots[k] <= T.
 * cadre_allowed_rows: the words of a minibatch in the layout of the update, out int64 [2][B]: source zi = 2 * worker + head of
 * src_table (n_src pointers to int64 [T + 1], 0: a storage without words, its rows get 0 = unmasked), row b of the worker is
 * idx[zi * Bw + b] (0 <= idx < T) and goes to out[head * B + pos[head * B + worker * Bw + b]] (pos NULL: identity).
 * cadre_ppo_am_loss: the argument list and behaviour of cadre_ppo_loss_ord (grid, scratch protocol, poison, stats row,
 * kl_rule.h gate) plus allowed int64 [2][B] in the layout of the sample arrays.  In the loss the taken action is allowed by
 * definition: after the "empty means all" rule, m |= 1 << a, so foreign data cannot produce -inf log-probabilities.
 * am_stats (may be NULL) float [2][am_F], am_F >= CADRE_AM_STATS_FIELDS, per head with every mean taken over the head's counted
 * rows (a command in range; zeros for a head without one):
 *   0 share of rows with a proper mask (a bin of K forbidden)   1 mean number of allowed bins
 *   2 mean pressure 1 - exp(lse_masked - lse_unmasked), the mass the unmasked head would put on forbidden bins
 *   3 rows whose action bit had to be OR-ed in (a count)
 * am_scratch (needed with am_stats): 10 * ceil(B / 16) floats of per-workgroup partials, combined by the last arriving
 * workgroup in workgroup order (no float atomics: two launches on the same inputs give the same bits). */
#define CADRE_AM_STATS_FIELDS 4
int cadre_sample_am(const float* logits, int64_t ldl, const float* q, int64_t ldq, int32_t R, int32_t n_out, int64_t* action,
                    float* logp, const int32_t* ord, const int64_t* allowed, void* stream);
int cadre_sample_rows_am(const float* O3, int64_t ldo, int64_t z_str, const int32_t* pos, const int32_t* cmd, int32_t N,
                         int32_t C, const float* q, int32_t K_steer, int32_t K_throttle, int64_t* action, float* logp,
                         float* value, const int32_t* ord, const int64_t* allowed, void* stream);
int cadre_categorical_eval_am(const float* logits, int64_t ldl, const int64_t* actions, int32_t R, int32_t n_out, float* logp,
                              float* entropy, const int32_t* ord, const int64_t* allowed, void* stream);
int cadre_allowed_note(const void* table, const int32_t* slots, const int64_t* words, int32_t n, int32_t T, void* stream);
int cadre_allowed_rows(const void* src_table, int32_t n_src, const int64_t* idx, int32_t Bw, int32_t T, const int32_t* pos,
                       int32_t B, int64_t* out, void* stream);
int cadre_ppo_am_loss(const float* logits, int64_t ldl, int64_t l_ns, const float* values, int64_t ldv, int64_t v_ns,
                      const int64_t* actions, const int32_t* commands, const float* old_values, const float* returns,
                      const float* old_logp, const float* adv, int32_t B, int32_t C, int32_t n_out_steer,
                      int32_t n_out_throttle, double* hp, float clip, float value_coeff, float clip_coeff, float ent_coeff,
                      float inv_b, float* losses, float* dlogits, float* dvalues, float* scratch, const int32_t* poison,
                      float* stats_row, int32_t F, float* stats_scratch, float target_kl, int32_t* stop, const int32_t* ord,
                      const int64_t* allowed, float* am_stats, int32_t am_F, float* am_scratch, void* stream);

/* ---------------------------------------------------------------- cost constraints (opt-in, csrc/constraint.hip)
 * PPO-Lagrangian (Ray et al. 2019) per head: a cost c >= 0 is recorded beside every reward, a cost critic per head values it,
 * and the advantages of the update become (A_r - lambda (A_c - mean A_c)) / (1 + lambda) with a multiplier lambda per head
 * that follows the cost RATE J = mean c of the section against a budget.  No loss kernel changes.
 * A cost tower is one flat fp32 buffer: W1 [D][H], b1 [H], W2 [H][H], b2 [H], W3 [H], b3 [1] — every matrix input-major, the
 * layout of the gradient buffer too.  H a multiple of 32, at most 256; 1 <= D <= 1024.  Rows: r = w * Tr + t for storage w < n
 * of obs_table (n device pointers to window rows [..][S][ldo], the storages of ONE head) and row t < Tr; x = obs_w[t][S - 1][0 ..
 * D-1] as stored.  Columns D .. ldo-1 and frames s < S - 1 are not read.
 * State block (float64), CADRE_LAG_STRIDE doubles per head h at state + h * CADRE_LAG_STRIDE: [CADRE_LAG_LAMBDA] the multiplier,
 * [CADRE_LAG_BUDGET] the budget of the cost rate, [CADRE_LAG_LR] lr_lambda, [CADRE_LAG_MAX] lambda_max, [CADRE_LAG_J] the last
 * cost rate, [CADRE_LAG_SHARE] the share of the last section's rows with c > 0, [CADRE_LAG_UPDATES] the multiplier steps taken.
 * cadre_cost_note: costs[k][slots[k]] = cost[k] for n storages in one launch; table: n device pointers to the storages' f32
 * [T + 1] tensors (0: skipped), 0 <= slots[k] <= T.
 * cadre_cost_forward: rows row0 .. row0 + rows - 1: h1 = relu(x W1 + b1), h2 = relu(h1 W2 + b2), values[i] = (sum_k h2_k W3_k in k
 * order) + b3 for i = r - row0, strict fp32.  h1, h2 [rows][H]: each NULL when not wanted.  A row's result does not depend on the
 * other rows of the launch.
 * cadre_cost_backward: the rows of one critic step with the values, h1, h2 the forward saved.  R_i = returns[w * ldr + t] of row
 * r = row0 + i.  d = v - R, dv = d / rows; loss[0] = 0.5 mean d^2 (float64 sum in a fixed order), loss[1] = rows; db3 = sum dv,
 * dW3 = h2^T dv, dH2 = (dv W3^T) [h2 > 0], dW2 = h1^T dH2, dH1 = (dH2 W2^T) [h1 > 0], dW1 = x^T dH1 with x read from the storage rows
 * themselves, db = column sums; every sum over rows runs in a fixed order.  scratch: rows (2 H + 1) floats.  Five launches, no
 * atomics.
 * cadre_cost_lambda: one workgroup per head.  cost_table: 2 N device pointers to costs f32 [T + 1], storage k of head k & 1.
 * J_h = (sum of the head's N T costs, rows 0 .. T-1 of its storages, float64, thread i of 256 summing rows i, i + 256, ... of
 * the (storage, time) order, the partials met in a fixed tree) / (N T); [CADRE_LAG_J] and [CADRE_LAG_SHARE] are written; with
 * `update`, lambda <- min(max(lambda + lr (J - budget), 0), lambda_max) in float64, one rounding per operation, and the
 * step count advances.
 * cadre_lag_mix: one workgroup per storage k of n (head k & 1), row_table: n records {cost_adv f32 [T], advantages f32 [T]}.
 * lf = (float)lambda_h.  m = (float)(float64 sum of cost_adv[0 .. T-1] in row order) / (float)T, then per row in strict fp32, one
 * rounding per statement: c = cost_adv[t] - m; p = lf c; q = advantages[t] - p; advantages[t] = q / (1 + lf).  With lf == 0
 * NOTHING is stored into that storage's advantages.  diag (may be NULL) double [n][2]: mean |p| / (1 + lf) and mean
 * |advantages[t] before the mix| / (1 + lf) of the storage.  Must run behind the cadre_cost_lambda launch whose lambda it reads.
 * Refused before any launch: null operands, dimensions outside the above, T outside 2 .. 3000 (cadre_gae_multi's range) for
 * cadre_cost_lambda and cadre_lag_mix, rows outside the table. */
#define CADRE_LAG_LAMBDA 0
#define CADRE_LAG_BUDGET 1
#define CADRE_LAG_LR 2
#define CADRE_LAG_MAX 3
#define CADRE_LAG_J 4
#define CADRE_LAG_SHARE 5
#define CADRE_LAG_UPDATES 6
#define CADRE_LAG_STRIDE 8
int cadre_cost_note(const void* table, const int32_t* slots, const float* costs, int32_t n, int32_t T, void* stream);
int cadre_cost_forward(const void* obs_table, int32_t n, int32_t Tr, int32_t S, int64_t ldo, int32_t D, int32_t H, int32_t row0,
                       int32_t rows, const float* tower, float* values, float* h1, float* h2, void* stream);
int cadre_cost_backward(const void* obs_table, int32_t n, int32_t Tr, int32_t S, int64_t ldo, int32_t D, int32_t H, int32_t row0,
                        int32_t rows, const float* tower, const float* values, const float* h1, const float* h2,
                        const float* returns, int64_t ldr, float* grads, float* loss, float* scratch, void* stream);
int cadre_cost_lambda(const void* cost_table, int32_t N, int32_t T, double* state, int32_t update, void* stream);
int cadre_lag_mix(const void* row_table, int32_t n, int32_t T, const double* state, double* diag, void* stream);

/* ---------------------------------------------------------------- weight averaging (csrc/average.hip)
 * Polyak / exponential moving average of a flat parameter buffer behind an optimiser step, the exchange of two flat buffers and
 * the weighted mean of K of them.  Plain HBM streams: 16-byte loads and stores on the aligned body of a range, single words
 * before and behind it; every store is a plain vector store and there is no atomic.
 *
 * State block of the average, float64 [CADRE_EMA_HEAD + n_models]: [CADRE_EMA_DECAY] the configured decay, [CADRE_EMA_WARMUP]
 * 0 or 1, [CADRE_EMA_COUNT] updates applied so far, [CADRE_EMA_D] the decay the last applied update used,
 * [CADRE_EMA_SKIPPED] updates skipped by the gate, the rest up to CADRE_EMA_HEAD reserved; then dist2[n_models], the
 * per-model squared distance after the last applied update.
 *
 * cadre_ema_update: params / ema float32 (any 4-byte alignment, not overlapping), seg_off int64 [n_models + 1], any
 * non-decreasing table of element offsets into both (model m = elements [seg_off[m], seg_off[m + 1])), 0 <= n_models <=
 * CADRE_EMA_MAX_MODELS; state as above (8-byte aligned); work float64 [CADRE_EMA_WORK_HEAD + n_models * CADRE_EMA_GRID]
 * scratch (8-byte aligned, need not be cleared); stop NULL or the device flag of cadre_ppo_loss_stats that
 * cadre_clip_adam_graph_gated reads.  With stop != NULL and *stop != 0 nothing is written except state[CADRE_EMA_SKIPPED] += 1
 * (and scratch).  Otherwise, with n = state[CADRE_EMA_COUNT] and d = state[CADRE_EMA_DECAY] — with warm-up d = min(d,
 * (1 + n) / (10 + n)) in double, the num_updates rule, so that the initial copy fades fast — and om = (float)(1.0 - d), every
 * element i of [seg_off[0], seg_off[n_models]):  t = p[i] - e[i] rounded to fp32;  e[i] = fmaf(om, t, e[i])  (the lerp form:
 * p == e leaves e bit for bit, t == 0 keeps the bits of e outright);  dist2[m] = sum over model m of ((double)p[i] -
 * (double)e_new[i])^2, each term rounded as written, summed in a fixed order (per lane, wave, workgroup into `work`, then the
 * CADRE_EMA_GRID partials of a model by the finishing launch): two runs over equal bytes give equal bits.  Then state[CADRE_EMA_D]
 * = d and state[CADRE_EMA_COUNT] = n + 1.  Three launches (preparation: gate and decay into `work`, read by every workgroup of
 * the pass before the count moves; the pass; the finish), no host sync: hipGraph-capturable.  Nothing outside [seg_off[0],
 * seg_off[n_models]) of ema is touched; params is only read.
 *
 * cadre_arena_swap: exchanges a[0 .. n) and b[0 .. n) (float32, any 4-byte alignment of either side, n >= 0) in one pass, one
 * launch.  Overlapping ranges are refused.
 *
 * cadre_arena_mean: src_table device int64 [K] (the addresses of K float32 buffers of n elements, 4-byte aligned), weights
 * device float64 [K], 1 <= K <= CADRE_MEAN_MAX_SOURCES; out[i] = (float)sum_k weights[k] (double)src_k[i], accumulated in
 * double in the order k = 0 .. K - 1 with one fma per term (the first onto -0.0: the rounded product itself, so K = 1 with
 * weight 1 copies the bits).  One launch.  out (any 4-byte alignment) may BE one of the sources — a thread reads all K values of
 * its elements before it writes them — but may not overlap one at another offset.
 * Refused before any launch, with a message: null operands, n_models / K / n outside the above, misaligned operands. */
#define CADRE_EMA_DECAY 0
#define CADRE_EMA_WARMUP 1
#define CADRE_EMA_COUNT 2
#define CADRE_EMA_D 3
#define CADRE_EMA_SKIPPED 4
#define CADRE_EMA_HEAD 8
#define CADRE_EMA_GRID 256
#define CADRE_EMA_WORK_HEAD 2
#define CADRE_EMA_MAX_MODELS 4096
#define CADRE_MEAN_MAX_SOURCES 64
int cadre_ema_update(const float* params, float* ema, const int64_t* seg_off, int32_t n_models, double* state, double* work,
                     const int32_t* stop, void* stream);
int cadre_arena_swap(float* a, float* b, int64_t n, void* stream);
int cadre_arena_mean(const int64_t* src_table, const double* weights, int32_t K, float* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
