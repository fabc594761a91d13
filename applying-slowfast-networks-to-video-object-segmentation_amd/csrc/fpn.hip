// fpn.hip -- the feature pyramid network in front of the RPN and the SlowFast layers (torchvision's
// FeaturePyramidNetwork + LastLevelMaxPool, frozen in the reference: inference only).
//
// sfvos_fpn_lateral: inner_blocks[i](x[i]) + nearest-upsampled coarser inner map, one pass.  A GEMM
//   y[position][n] = sum_c x[c][position] W[n][c] with the POSITIONS as the MFMA rows: lane (r = lane & 31, h = lane >> 5)
//   holds position r of its wave's 32 and the channels of chunk 2 s + h of MFMA step s, so the A fragment is CE dword
//   loads per step straight from the planar fp32 tensor (each load: 32 consecutive positions of one channel, 128 B per
//   lane half), converted in registers.  W[n][c] in the compute dtype is the B operand as it lies: lane r reads the 16
//   bytes of row n0 + r at the same channels.  C/D: column (lane & 31) = n, rows = positions, so a store instruction
//   writes 32 consecutive channels of one position per lane half.
//   Workgroup = 4 waves.  KS = 1: the waves take 4 consecutive position tiles and share each staged weight slab
//   [32 NT rows][32 channels] through LDS; the next slab and the next x loads are in flight while a slab is multiplied.
//   NT <= 4 (128 channels: four waves per SIMD in bf16, three in fp32; 256 channels in one workgroup leave one): a
//   256-channel level is two slices of the same positions that run on the same XCD, so x comes from memory once and
//   from that XCD's L2 the second time.  KS = 4 (few positions, many channels: C5): the waves take the same position
//   tile and a quarter of every 128-channel slab each; their accumulators are added in wave order through LDS (fixed
//   order: deterministic, no atomics).
// sfvos_fpn_pool: LastLevelMaxPool = max_pool2d(kernel 1, stride 2) = the subsample dst[b][i][j] = src[b][2i][2j].
#include "elt_util.h"

namespace sfvos {

constexpr int FPN_KC = 32;  // channels of one staged weight slab per wave

struct FpnLateralArgs {
  const float* x;
  long long stride_b, stride_c, stride_h;
  const void* w;
  const float* bias;
  const void* top;
  void* y;
  int c_in, c_out, h, w_, P, top_h, top_w, ld_top, ld_y;
  int n_btiles;  // position tiles of the launch (KS = 1: of 128 positions, KS = 4: of 32)
};

template <int DT, int NT, int KS>
__global__ __launch_bounds__(256, 3) void fpn_lateral_kernel(const FpnLateralArgs a) {
  typedef typename Elt<DT>::type T;
  constexpr int CE = Elt<DT>::CE, ES = 16 / CE;
  constexpr int STEPS = FPN_KC / (2 * CE);  // MFMA steps per slab: bf16 2 (32x32x16), f32 4 (4 x 32x32x2 each)
  constexpr int KW = KS * FPN_KC;           // channels staged per iteration
  constexpr int ROWB = KW * ES + 16;        // bytes of a staged row; the 16 spread the rows over the banks
  constexpr int ROWS = NT * 32;
  constexpr int STAGE = ROWS * ROWB, RED = (KS - 1) * NT * 1024 * 4;
  __shared__ __attribute__((aligned(16))) char smem[STAGE > RED ? STAGE : RED];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hf = lane >> 5;
  const int slices = a.c_out / ROWS;
  // workgroups go to the 8 XCDs round-robin: the slices of one position tile are 8 apart in the grid, so they share an L2
  // and only the first of them reads its part of x from memory
  const int grp = blockIdx.x / (8 * slices), rem8 = blockIdx.x - grp * 8 * slices;
  const int slice = rem8 >> 3, btile = grp * 8 + (rem8 & 7);
  if (btile >= a.n_btiles) return;
  const int n_base = slice * ROWS;
  const long long p0 = 32ll * (KS == 1 ? btile * 4 + wave : btile);  // first position of this wave's tile
  const int hw = a.h * a.w_;

  // this lane's position (clamped: lanes past the end load a valid address and store nothing)
  const unsigned pl = (unsigned)(p0 + r < a.P ? p0 + r : a.P - 1);
  const unsigned pb = pl / (unsigned)hw, prem = pl - pb * (unsigned)hw;
  const unsigned pi = prem / (unsigned)a.w_, pj = prem - pi * (unsigned)a.w_;
  const int kw0 = KS == 1 ? 0 : wave * FPN_KC;  // this wave's channels inside a staged slab
  const float* xp = a.x + pb * a.stride_b + pi * a.stride_h + pj + (long long)(kw0 + hf * CE) * a.stride_c;

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  float cur[STEPS * CE], nxt[STEPS * CE] = {};
  auto load_a = [&](float* f, int k0) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int e = 0; e < CE; ++e) f[s * CE + e] = xp[(long long)(k0 + 2 * s * CE + e) * a.stride_c];
  };

  // weight slab [ROWS][KW] of this slice: global -> registers one iteration ahead, registers -> LDS behind the barrier
  constexpr int CPR = KW / CE;                     // 16-byte chunks per staged row
  constexpr int WPT = (ROWS * CPR + 255) / 256;    // chunks per thread
  u32x4 wreg[WPT];
  auto load_w = [&](int k0) {
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int c = tid + i * 256, row = c / CPR, cc = c - row * CPR;
      if (c < ROWS * CPR)
        wreg[i] = *(const u32x4*)((const char*)a.w + ((long long)(n_base + row) * a.c_in + k0) * ES + cc * 16);
    }
  };

  const int iters = a.c_in / KW;
  load_a(cur, 0);
  load_w(0);
  for (int it = 0; it < iters; ++it) {
    const int k0 = it * KW;
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int c = tid + i * 256, row = c / CPR, cc = c - row * CPR;
      if (c < ROWS * CPR) *(u32x4*)(smem + row * ROWB + cc * 16) = wreg[i];
    }
    __syncthreads();
    if (it + 1 < iters) {   // in flight while this slab is multiplied
      load_a(nxt, k0 + KW);
      load_w(k0 + KW);
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const u32x4 af = pack<DT>(cur + s * CE);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const u32x4 bf = lds_read16(smem + (t * 32 + r) * ROWB + (kw0 + (2 * s + hf) * CE) * ES);
        Mma<DT>::run(acc[t], af, bf);
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < STEPS * CE; ++i) cur[i] = nxt[i];
  }

  if constexpr (KS > 1) {  // waves 1 .. KS-1 hand their sums to wave 0, which adds them in wave order
    float* red = (float*)smem;
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[((wave - 1) * NT + t) * 1024 + i * 64 + lane] = acc[t][i];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int v = 0; v < KS - 1; ++v)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] += red[(v * NT + t) * 1024 + i * 64 + lane];
  }

  // epilogue: register i of lane half hf is position row (i & 3) + 8 (i >> 2) + 4 hf of the tile, column r of the n-tile.
  // Four rows at a time: their 4 NT loads of the top map are unconditional (rows past the end read the last position's)
  // and independent, so they are in flight together; only the stores are predicated.
  const T* top = (const T*)a.top;
  T* y = (T*)a.y;
  float bias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bias[t] = a.bias[n_base + t * 32 + r];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const long long pg = p0 + 8 * g + 4 * hf;   // rows pg .. pg + 3 = registers 4 g .. 4 g + 3
    if (top) {
      T tv[NT][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned p = (unsigned)(pg + q < a.P ? pg + q : a.P - 1);
        const unsigned b = p / (unsigned)hw, rem = p - b * (unsigned)hw;
        const unsigned ii = rem / (unsigned)a.w_, jj = rem - ii * (unsigned)a.w_;
        const T* tp = top + (((long long)b * a.top_h + (ii >> 1)) * a.top_w + (jj >> 1)) * a.ld_top + n_base + r;
#pragma unroll
        for (int t = 0; t < NT; ++t) tv[t][q] = tp[t * 32];
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][4 * g + q] = (acc[t][4 * g + q] + bias[t]) + Elt<DT>::to_f32(tv[t][q]);
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][4 * g + q] += bias[t];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (pg + q < a.P) {
        T* yp = y + (pg + q) * a.ld_y + n_base + r;
#pragma unroll
        for (int t = 0; t < NT; ++t) yp[t * 32] = Elt<DT>::from_f32(acc[t][4 * g + q]);
      }
    }
  }
}

template <int DT, int NT, int KS>
static void launch_lateral(const FpnLateralArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((fpn_lateral_kernel<DT, NT, KS>), dim3(grid), dim3(256), 0, s, a);
}

// dst[b][i][j][chunk] = src[b][2i][2j][chunk], 16-byte chunks; pitches in chunks
__global__ __launch_bounds__(256) void fpn_pool_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                       long long total, int h, int w, int oh, int ow, int chunks,
                                                       int lds, int ldd) {
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % chunks);
    const long long pos = idx / chunks;
    const int j = (int)(pos % ow);
    const long long bi = pos / ow;
    const int i = (int)(bi % oh);
    const long long b = bi / oh;
    dst[pos * ldd + c] = src[((b * h + 2 * i) * w + 2 * j) * lds + c];
  }
}

}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_fpn_lateral(const float* x, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                                 int batch, int c_in, int h, int w, const void* weight, const float* bias, int c_out,
                                 const void* top, int top_h, int top_w, int ld_top, void* y, int ld_y, int dtype,
                                 sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && weight && bias && y, "fpn_lateral: null pointer");
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "fpn_lateral: bad dtype %d (f32 or bf16)", dtype);
  SFVOS_REQUIRE(stride_w == 1, "fpn_lateral: stride_w must be 1, got %lld", (long long)stride_w);
  SFVOS_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_h >= 0, "fpn_lateral: negative stride");
  SFVOS_REQUIRE(c_in > 0 && c_in % 32 == 0, "fpn_lateral: c_in %d must be a positive multiple of 32", c_in);
  SFVOS_REQUIRE(c_out > 0 && c_out % 32 == 0 && c_out <= 256, "fpn_lateral: c_out %d must be a multiple of 32, <= 256",
                c_out);
  SFVOS_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && (long long)batch * h * w < (1ll << 31) - 128,
                "fpn_lateral: bad extent (batch %d, %dx%d)", batch, h, w);
  SFVOS_REQUIRE(ld_y >= c_out, "fpn_lateral: pitch ld_y %d smaller than c_out %d", ld_y, c_out);
  SFVOS_REQUIRE((uintptr_t)weight % 16 == 0, "fpn_lateral: the weight image must be 16-byte aligned");
  if (top) {
    SFVOS_REQUIRE(top_h >= 1 && top_w >= 1 && (h == 2 * top_h || h == 2 * top_h - 1) &&
                      (w == 2 * top_w || w == 2 * top_w - 1),
                  "fpn_lateral: a %dx%d level cannot follow a %dx%d top (each side must be 2 n or 2 n - 1)", h, w, top_h,
                  top_w);
    SFVOS_REQUIRE(ld_top >= c_out, "fpn_lateral: pitch ld_top %d smaller than c_out %d", ld_top, c_out);
  }
  FpnLateralArgs a;
  a.x = x; a.stride_b = stride_b; a.stride_c = stride_c; a.stride_h = stride_h;
  a.w = weight; a.bias = bias; a.top = top; a.y = y;
  a.c_in = c_in; a.c_out = c_out; a.h = h; a.w_ = w; a.P = batch * h * w;
  a.top_h = top_h; a.top_w = top_w; a.ld_top = ld_top; a.ld_y = ld_y;

  // Fill the chip: the widest channel slice (fewest re-reads of x through L2) that still gives every CU a workgroup; with too few
  // positions even for 32-channel slices, the waves of a workgroup split the channels of x instead (KS = 4).
  const long long tiles = ceil_div64(a.P, 32), btiles = ceil_div64(tiles, 4), want = device_cu_count();
  const int nt_all = c_out / 32;
  int nt = 1, ks = 1;
  for (int c = 4; c >= 1; c >>= 1)
    if (nt_all % c == 0 && btiles * (nt_all / c) >= want) { nt = c; break; }
  if (btiles * (nt_all / nt) < want && c_in % (4 * FPN_KC) == 0) { nt = 1; ks = 4; }
  a.n_btiles = (int)(ks == 4 ? tiles : btiles);
  const unsigned grid = (unsigned)(ceil_div64(a.n_btiles, 8) * 8 * (nt_all / nt));
  hipStream_t s = (hipStream_t)stream;
  return launch_dt(dtype, "fpn_lateral", [&](auto dt) {
    constexpr int D = decltype(dt)::value;
    if (ks == 4) launch_lateral<D, 1, 4>(a, grid, s);
    else if (nt == 4) launch_lateral<D, 4, 1>(a, grid, s);
    else if (nt == 2) launch_lateral<D, 2, 1>(a, grid, s);
    else launch_lateral<D, 1, 1>(a, grid, s);
  });
}

extern "C" int sfvos_fpn_pool(const void* src, int ld_src, void* dst, int ld_dst, int batch, int h, int w, int C,
                              int dtype, sfvos_stream_t stream) {
  SFVOS_REQUIRE(src && dst, "fpn_pool: null pointer");
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "fpn_pool: bad dtype %d (f32 or bf16)", dtype);
  const int ce = 16 / elt_bytes(dtype);
  SFVOS_REQUIRE(C > 0 && C % ce == 0, "fpn_pool: C %d must be a whole number of 16-byte chunks (%d elements)", C, ce);
  SFVOS_REQUIRE(ld_src >= C && ld_dst >= C && ld_src % ce == 0 && ld_dst % ce == 0,
                "fpn_pool: pitches %d, %d must be >= C %d and multiples of %d", ld_src, ld_dst, C, ce);
  SFVOS_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && (long long)batch * h * w < (1ll << 31),
                "fpn_pool: bad extent (batch %d, %dx%d)", batch, h, w);
  SFVOS_REQUIRE((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, "fpn_pool: buffers must be 16-byte aligned");
  const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1, chunks = C / ce;
  const long long total = (long long)batch * oh * ow * chunks;
  hipLaunchKernelGGL(fpn_pool_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src,
                     (u32x4*)dst, total, h, w, oh, ow, chunks, ld_src / ce, ld_dst / ce);
  return check_launch("fpn_pool");
}
