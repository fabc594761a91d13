// Helpers shared by the HBM-bound kernels (elementwise.hip, batchnorm.hip, maskhead.hip, window_shift.hip) and the
// roi_heads files (project.hip, boxes.hip, rpn.hip, roi_targets.hip, rpn_targets.hip): 16-byte pack/unpack, deterministic column and block
// sums, the block prefix scan, the box encoder, smooth-L1; on the host, the f32 / bf16 activation checks, the class-count check and
// dtype dispatch.
#pragma once
#include <type_traits>

#include "common.h"

namespace sfvos {

template <int DT> __device__ __forceinline__ void unpack(const u32x4& v, float* f);
template <> __device__ __forceinline__ void unpack<SFVOS_F32>(const u32x4& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    // copy the lane to a scalar first: hipcc (ROCm 7.2) mis-compiles __builtin_bit_cast applied
    // directly to an ext-vector element lvalue (every e reads element 0)
    const unsigned u = v[e];
    f[e] = __builtin_bit_cast(float, u);
  }
}
template <> __device__ __forceinline__ void unpack<SFVOS_BF16>(const u32x4& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned u = v[e];
    const unsigned lo = u << 16, hi = u & 0xffff0000u;
    f[2 * e] = __builtin_bit_cast(float, lo);
    f[2 * e + 1] = __builtin_bit_cast(float, hi);
  }
}
template <int DT> __device__ __forceinline__ u32x4 pack(const float* f);
template <> __device__ __forceinline__ u32x4 pack<SFVOS_F32>(const float* f) {
  u32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __builtin_bit_cast(unsigned, f[e]);
  return v;
}
template <> __device__ __forceinline__ u32x4 pack<SFVOS_BF16>(const float* f) {
  u32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned lo = __builtin_bit_cast(unsigned short, (__bf16)f[2 * e]);
    const unsigned hi = __builtin_bit_cast(unsigned short, (__bf16)f[2 * e + 1]);
    v[e] = lo | (hi << 16);
  }
  return v;
}

// v_cvt_pk_fp8_f32 alone does not saturate: a value that rounds beyond 448 (and +-inf) becomes the NaN code 0x7f.  The
// median of (v, 448, -448) clamps first; it does not keep a NaN (v_med3_f32 with a NaN operand takes min3, which
// drops it: -448), so a NaN is passed through and stays a NaN code.  The counts are taken before the clamp.
__device__ __forceinline__ float sat_e4m3(float v) {
  const float c = __builtin_amdgcn_fmed3f(v, 448.f, -448.f);
  return v != v ? v : c;
}
template <> __device__ __forceinline__ u32x4 pack<SFVOS_FP8>(const float* f) {  // 16 floats -> 16 e4m3 (saturating)
  u32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(sat_e4m3(f[4 * e]), sat_e4m3(f[4 * e + 1]), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(sat_e4m3(f[4 * e + 2]), sat_e4m3(f[4 * e + 3]), w, true);
    v[e] = (unsigned)w;
  }
  return v;
}

// Deterministic column sums of part[rows][ncol]: block = 32 channels x RL row lanes, each lane sums
// its strided rows (4 loads in flight), then lane 0 adds the RL lane sums in a fixed order.
constexpr int RL = 32;
__device__ __forceinline__ double column_sum(const float* part, int rows, int ncol, int col, int sub, double* scratch,
                                             int c_local) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int rI = sub;
  for (; rI + 3 * RL < rows; rI += 4 * RL) {
    s0 += (double)part[(long long)rI * ncol + col];
    s1 += (double)part[(long long)(rI + RL) * ncol + col];
    s2 += (double)part[(long long)(rI + 2 * RL) * ncol + col];
    s3 += (double)part[(long long)(rI + 3 * RL) * ncol + col];
  }
  for (; rI < rows; rI += RL) s0 += (double)part[(long long)rI * ncol + col];
  scratch[sub * 32 + c_local] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  double tot = 0.0;
  if (sub == 0)
#pragma unroll
    for (int k = 0; k < RL; ++k) tot += scratch[k * 32 + c_local];
  __syncthreads();
  return tot;
}

// Sum of one double per thread of a 1024-thread block in a fixed tree order (512, 256, ..., 1); red: 1024 doubles of
// LDS of the caller's (one array per sum).  Every thread gets the total.
__device__ __forceinline__ double block_sum_1024(double* red, double v) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// exclusive prefix sum over the 1024 threads of a block (thread order); wsum: 16 ints of LDS
__device__ __forceinline__ int block_excl_scan_1024(int v, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  __syncthreads();
  return base + inc - v;
}

// BoxCoder.encode_single of one box: t[0..4) = targets of the reference box g against the proposal p (boxes.hip's
// sfvos_box_encode and roi_targets.hip's sampler).  The products and sums are written one by one as torch issues them;
// the compiler may still fuse `p[0] + 0.5 pw` and its three siblings into multiply-adds (the _rn intrinsics are plain
// operators to it), which changes nothing: scaling by 0.5 is exact, so the fused and the separate form round the same sum.
__device__ __forceinline__ void box_encode_one(const float* g, const float* p, float wx, float wy, float ww, float wh,
                                               float* t) {
  const float pw = p[2] - p[0], ph = p[3] - p[1];
  const float pcx = p[0] + __fmul_rn(0.5f, pw), pcy = p[1] + __fmul_rn(0.5f, ph);
  const float gw = g[2] - g[0], gh = g[3] - g[1];
  const float gcx = g[0] + __fmul_rn(0.5f, gw), gcy = g[1] + __fmul_rn(0.5f, gh);
  t[0] = __fmul_rn(wx, gcx - pcx) / pw;
  t[1] = __fmul_rn(wy, gcy - pcy) / ph;
  t[2] = __fmul_rn(ww, logf(gw / pw));
  t[3] = __fmul_rn(wh, logf(gh / ph));
}

// torch's smooth_l1_loss of one difference (boxes.hip's box loss, rpn_targets.hip's): beta = 0 is plain L1
__device__ __forceinline__ float smooth_l1(float d, float beta) {
  const float a = fabsf(d);
  return a < beta ? 0.5f * d * d / beta : a - 0.5f * beta;
}

static inline unsigned grid_for(long long work_items, int per_block, unsigned cap = 2048u * 4u) {
  long long g = ceil_div64(work_items, per_block);
  if (g < 1) g = 1;
  if (g > (long long)cap) g = cap;
  return (unsigned)g;
}

// Bytes per element of an f32 / bf16 operand; 16 / elt_bytes elements fill a 16-byte chunk.  The entry points refuse
// every other dtype, except packed_weight_bytes, which sizes it as f32.
static inline int elt_bytes(int dtype) { return dtype == SFVOS_BF16 ? 2 : 4; }

// f32 / bf16 activations: C a multiple of 32 up to 256, two pitches of whole 16-byte chunks
static inline int check_act(const char* what, int dtype, int C, int ld_a, int ld_b) {
  const int ce = 16 / elt_bytes(dtype);
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "%s: bad dtype %d", what, dtype);
  SFVOS_REQUIRE(C > 0 && C % 32 == 0 && C <= 256, "%s: C %d must be a multiple of 32, <= 256", what, C);
  SFVOS_REQUIRE(ld_a >= C && ld_b >= C && ld_a % ce == 0 && ld_b % ce == 0,
                "%s: pitches %d, %d must be >= C and multiples of %d", what, ld_a, ld_b, ce);
  return SFVOS_OK;
}

// Classes of the roi_heads entry points that cap them (project.hip, boxes.hip)
constexpr int HEAD_MAXK = 8;
static inline int check_classes(const char* what, int num_classes) {
  SFVOS_REQUIRE(num_classes >= 1 && num_classes <= HEAD_MAXK, "%s: num_classes %d out of [1, %d]", what, num_classes,
                HEAD_MAXK);
  return SFVOS_OK;
}

// Launch of a kernel template over f32 / bf16: launch(dt) gets dt = std::integral_constant<int, SFVOS_F32 or
// SFVOS_BF16>, which instantiates the kernel (`kern<dt>`).  Any other dtype is refused as "<what>: bad dtype"; a launch
// error is reported under `kernel`, by default `what`.
template <class F>
static int launch_dt(int dtype, const char* what, F&& launch, const char* kernel = nullptr) {
  if (dtype == SFVOS_F32)
    launch(std::integral_constant<int, SFVOS_F32>());
  else if (dtype == SFVOS_BF16)
    launch(std::integral_constant<int, SFVOS_BF16>());
  else {
    set_error("%s: bad dtype %d", what, dtype);
    return SFVOS_E_ARG;
  }
  return check_launch(kernel ? kernel : what);
}

}  // namespace sfvos
