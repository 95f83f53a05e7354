// checkpoint.hip — the device side of a training checkpoint: cadre_state_capture copies every range of a device table
// into one staging buffer and forms a 64-bit digest of each range from the words it has just read, in ONE launch.
//
// The digest of a range of 32-bit words w_0 .. w_{n-1} is  D = sum_i (uint64(w_i) + 1) ((2 i + 1) K)  mod 2^64,
// K = 0x9E3779B97F4A7C15.  Addition mod 2^64 is associative and commutative, so the per-lane, per-wave and per-workgroup
// partial sums below give the same bits whatever order the workgroups arrive in: two launches over equal bytes give equal
// digests by construction.  An integrity check (every single-bit flip, every swap of two unequal words and every change
// of length moves it), NOT a cryptographic hash.
//
// A plain HBM-bound stream: each source word is read once, each staging word written once, the digest costs no further
// memory traffic.  Everything this file writes is written with plain vector stores and one 64-bit vector atomic add per
// workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cadre_hip.h"

int cadre_fail(const char* msg);
#define ST(s) ((hipStream_t)(s))
#define FAIL_IF(cond, msg) \
  if (cond) return cadre_fail(msg)

namespace {

constexpr int BLOCK = 256;                 // 4 waves
constexpr int GRID_X = 512;                // workgroups that stride over one range (x); y = the range
constexpr uint64_t K = 0x9E3779B97F4A7C15ull;

struct range_t {
  const void* src; int64_t dst_off; int64_t bytes;
};

// (uint64(w) + 1) m  =  w m + m   (one 32 x 64 multiply-add)
__device__ __forceinline__ uint64_t term(uint32_t w, uint64_t m) { return (uint64_t)w * m + m; }

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// Device memory through global (not flat) instructions: the table hands the pointers over as plain integers.
#define GLOBAL_AS __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef GLOBAL_AS const u32x4* gld4_t;
typedef GLOBAL_AS u32x4* gst4_t;
typedef GLOBAL_AS u32x2* gst2_t;
typedef GLOBAL_AS uint32_t* gst1_t;

// The 16-byte body of a range: vectors [v0, nvec) step `stride`, vector v = words head + 4 v .. + 3 (s4 = src + head is
// 16-byte aligned).  STORE: 0 digests only, 16 / 8 / 4 = the widest store the staging side's alignment allows.
template <int STORE>
__device__ __forceinline__ uint64_t body(const uint32_t* src, uint32_t* dst, int64_t head, int64_t v0, int64_t nvec,
                                         int64_t stride) {
  const gld4_t s4 = (gld4_t)(src + head);
  uint64_t acc = 0;
  for (int64_t v = v0; v < nvec; v += stride) {
    const u32x4 x = s4[v];
    const int64_t i = head + 4 * v;
    uint64_t m = (2 * (uint64_t)i + 1) * K;
    acc += term(x.x, m); m += 2 * K;
    acc += term(x.y, m); m += 2 * K;
    acc += term(x.z, m); m += 2 * K;
    acc += term(x.w, m);
    if (STORE == 16) {
      *(gst4_t)(dst + i) = x;
    } else if (STORE == 8) {
      const gst2_t d = (gst2_t)(dst + i);
      d[0] = u32x2{x.x, x.y};
      d[1] = u32x2{x.z, x.w};
    } else if (STORE == 4) {
      const gst1_t d = (gst1_t)(dst + i);
      d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
    }
  }
  return acc;
}

// Range r = blockIdx.y.  Words [0, head) bring the source to a 16-byte boundary (workgroup 0), words [head, head + 4 nvec)
// go as 16-byte loads, grid-stride over the x workgroups, and the last n - head - 4 nvec < 4 words are workgroup 0's
// again.  The staging side is written with 16-byte stores when it is aligned like the source, else with 8- or 4-byte ones.
__global__ __launch_bounds__(BLOCK) void state_capture_kernel(const range_t* table, char* staging, uint64_t* digests) {
  __shared__ uint64_t part[BLOCK / 64];
  const int r = blockIdx.y, bx = blockIdx.x, tid = threadIdx.x;
  const range_t g = table[r];
  const bool bad = g.bytes < 0 || (g.bytes & 3) || ((uintptr_t)g.src & 3) || (g.bytes > 0 && !g.src) ||
                   (staging && (g.dst_off < 0 || (g.dst_off & 3)));
  if (bad) {                                           // a record the host wrapper would have refused: nothing is copied
    if (bx == 0 && tid == 0) digests[r] = ~0ull;
    return;
  }
  const int64_t n = g.bytes >> 2;
  const uint32_t* src = (const uint32_t*)g.src;
  int64_t head = (int64_t)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int64_t nvec = (n - head) >> 2;
  if (bx > 0 && (int64_t)bx * BLOCK >= nvec) return;   // (uniform per workgroup; covers n == 0 for every x > 0)
  uint32_t* dst = staging ? (uint32_t*)(staging + g.dst_off) : nullptr;
  const int dalign = dst ? (int)((uintptr_t)(dst + head) & 15) : -1;
  const int64_t v0 = (int64_t)bx * BLOCK + tid, stride = (int64_t)gridDim.x * BLOCK;
  uint64_t acc;
  if (dalign < 0) acc = body<0>(src, dst, head, v0, nvec, stride);
  else if (dalign == 0) acc = body<16>(src, dst, head, v0, nvec, stride);
  else if (dalign == 8) acc = body<8>(src, dst, head, v0, nvec, stride);
  else acc = body<4>(src, dst, head, v0, nvec, stride);
  if (bx == 0) {
    const int64_t tail0 = head + 4 * nvec;
    if (tid < head) {
      const uint32_t w = src[tid];
      acc += term(w, (2 * (uint64_t)tid + 1) * K);
      if (dst) dst[tid] = w;
    }
    const int64_t i = tail0 + tid;
    if (i < n) {                                       // at most three words
      const uint32_t w = src[i];
      acc += term(w, (2 * (uint64_t)i + 1) * K);
      if (dst) dst[i] = w;
    }
  }
  acc = wave_sum_u64(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    uint64_t tot = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) tot += part[k];
    atomicAdd((unsigned long long*)(digests + r), (unsigned long long)tot);
  }
}

}  // namespace

extern "C" int cadre_state_capture(const void* range_table, int32_t n_ranges, void* staging, uint64_t* digests,
                                   void* stream) {
  FAIL_IF(n_ranges < 0 || n_ranges > CADRE_CAPTURE_MAX_RANGES, "cadre_state_capture: bad argument (0 <= n_ranges <= 65535)");
  if (n_ranges == 0) return 0;
  FAIL_IF(!range_table || !digests, "cadre_state_capture: null operand");
  FAIL_IF(((uintptr_t)range_table & 7) || ((uintptr_t)digests & 7) || ((uintptr_t)staging & 3),
          "cadre_state_capture: misaligned operand (table and digests 8 bytes, staging 4 bytes)");
  // the slots are accumulated into: zero them on the same stream first
  hipError_t e = hipMemsetAsync(digests, 0, sizeof(uint64_t) * (size_t)n_ranges, ST(stream));
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(state_capture_kernel, dim3(GRID_X, n_ranges), dim3(BLOCK), 0, ST(stream),
                     (const range_t*)range_table, (char*)staging, digests);
  return (int)hipGetLastError();
}
