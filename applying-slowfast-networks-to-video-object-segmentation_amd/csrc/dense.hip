// dense.hip -- dense layers for the box head of roi_heads (torchvision models/detection/faster_rcnn.py: TwoMLPHead =
// fc6 12544 -> 1024 + ReLU, fc7 1024 -> 1024 + ReLU) on 512 (training) or 1000 (evaluation) RoIs per frame.
//
//   forward        y[M][N]  = act(x[M][K] . Wp^T + b)      Wp[N][K] = packed image of nn.Linear's weight [N][K]
//   data gradient  dx[M][K] = dz[M][N] . W                 the same kernel on the image Wd[K][N] (sfvos_pack_dense_dgrad)
//   weight grad.   dW[N][K] = dz^T . x                     reduction over the M rows only
//
// The fc6 images carry the permutation between torchvision's flatten of NCHW RoI features (column c*HW + p) and the
// channels-last rows the library produces (column p*C + c), so the kernels read and write [N,7,7,256] rows as they are.
//
// GEMM kernel: 128 x 128 output tile per workgroup (4 waves as 2 x 2, 64 x 64 each), both operands k-contiguous and
// staged through LDS in full 128-byte row pieces by global_load_lds (16 bytes per lane), two buffers, one barrier per
// stage.  LDS image of a stage: [row][8 chunks of 16 B], chunk c of row r at position c ^ (r & 7) -- the swizzle is
// applied to the SOURCE address of the copy, whose destination is lane-linear.  bf16: v_mfma_f32_16x16x32_bf16,
// f32: v_mfma_f32_32x32x2_f32 (exact products), fp32 accumulation either way.  K is split over blockIdx.z into fp32
// slabs when the tiles alone do not fill the chip; a second launch sums the slabs in a fixed order and applies bias,
// ReLU and the rounding of the store once (no atomics: results are bit-identical from run to run).
#include "elt_util.h"

namespace sfvos {

constexpr int DN_TILE = 128;            // rows and columns of a workgroup's output tile
constexpr int DN_STAGE = DN_TILE * 128; // bytes of one operand's stage image
constexpr int DN_LDS = 4 * DN_STAGE;    // 2 buffers x (x image + w image)
constexpr int DN_MAX_SPLITS = 16;

template <int DT> struct DenseMma;
template <> struct DenseMma<SFVOS_BF16> {
  static constexpr int TILE = 16;
  typedef f32x4 acc_t;
  static __device__ __forceinline__ void run(acc_t& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0,
                                                   0, 0);
  }
  // C/D layout: column = lane & 15, row = 4 (lane >> 4) + e
  static __device__ __forceinline__ int row(int e, int lane) { return 4 * (lane >> 4) + e; }
};
template <> struct DenseMma<SFVOS_F32> {
  static constexpr int TILE = 32;
  typedef f32x16 acc_t;
  static __device__ __forceinline__ void run(acc_t& acc, const u32x4& a, const u32x4& b) { Mma<SFVOS_F32>::run(acc, a, b); }
  // C/D layout: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  static __device__ __forceinline__ int row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
};

// x [M][K], wp [N][K] (both DT, K contiguous).  splits == 1 (slab == NULL): y = act(acc + bias) in DT;
// otherwise slab[blockIdx.z][M][N] = this split's fp32 sums.
template <int DT>
__global__ __launch_bounds__(256) void dense_kernel(const char* __restrict__ x, const char* __restrict__ wp,
                                                    const float* __restrict__ bias, char* y, float* slab, int M, int N,
                                                    int K, int relu, int stages_per_split) {
  typedef typename Elt<DT>::type T;
  typedef DenseMma<DT> MM;
  typedef typename MM::acc_t acc_t;
  constexpr int CE = Elt<DT>::CE;
  constexpr int TILE = MM::TILE, NT = 64 / TILE;   // MFMA tile side; tiles per wave side
  constexpr int CPS = 64 / TILE, STEPS = 8 / CPS;  // 16-byte chunks one MFMA step consumes along k; steps per stage
  constexpr int AE = TILE * TILE / 64;             // accumulator elements per lane and tile
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][x image 16 KB | w image 16 KB]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * DN_TILE, n0 = blockIdx.x * DN_TILE;
  const int kchunks = K / CE;
  const int total_stages = (kchunks + 7) / 8;
  const int s_begin = blockIdx.z * stages_per_split;
  const int s_end = min(total_stages, s_begin + stages_per_split);

  // copies: wave wv moves the 8-row pieces 4 wv .. 4 wv + 3 of both images; lane i = (row i / 8, position i % 8) reads
  // source chunk (i % 8) ^ (i / 8).  Rows past M / N are clamped (computed and dropped), chunks past K too (their MFMA
  // steps are skipped).
  const int cr = lane >> 3, csrc = (lane & 7) ^ cr;
  const char* xrow[4];
  const char* wrow[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = (wv * 4 + q) * 8 + cr;
    xrow[q] = x + (long long)min(m0 + r, M - 1) * kchunks * 16;
    wrow[q] = wp + (long long)min(n0 + r, N - 1) * kchunks * 16;
  }
  auto issue = [&](int s, int buf) {
    const int kc = min(s * 8 + csrc, kchunks - 1);
    char* base = smem + buf * 2 * DN_STAGE + wv * 4 * 1024;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      glds16(xrow[q] + (long long)kc * 16, base + q * 1024);
      glds16(wrow[q] + (long long)kc * 16, base + DN_STAGE + q * 1024);
    }
  };

  acc_t acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < AE; ++e) acc[i][j][e] = 0.f;

  const int lr = lane % TILE, lc = lane / TILE;   // fragment row and k chunk of this lane
  if (s_begin < s_end) issue(s_begin, 0);
  for (int s = s_begin; s < s_end; ++s) {
    const int buf = (s - s_begin) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // stage s is in LDS; every wave is done with the other buffer
    if (s + 1 < s_end) issue(s + 1, buf ^ 1);
    const char* xa = smem + buf * 2 * DN_STAGE;
    const char* wb = xa + DN_STAGE;
#pragma unroll
    for (int ks = 0; ks < STEPS; ++ks) {
      if (s * 8 + ks * CPS >= kchunks) break;   // the half stage behind K (bf16, K = 32 mod 64); wave-uniform
      const int c = ks * CPS + lc;
      u32x4 a[NT], b[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int ra = wm * 64 + i * TILE + lr, rb = wn * 64 + i * TILE + lr;
        a[i] = lds_read16(xa + (ra * 8 + (c ^ (ra & 7))) * 16);
        b[i] = lds_read16(wb + (rb * 8 + (c ^ (rb & 7))) * 16);
      }
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) MM::run(acc[i][j], a[i], b[j]);
    }
  }

#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + wn * 64 + j * TILE + lr;
      if (n >= N) continue;
      const float bv = (!slab && bias) ? bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < AE; ++e) {
        const int m = m0 + wm * 64 + i * TILE + MM::row(e, lane);
        if (m >= M) continue;
        if (slab) {
          slab[((long long)blockIdx.z * M + m) * N + n] = acc[i][j][e];
        } else {
          float v = acc[i][j][e] + bv;
          if (relu) v = fmaxf(v, 0.f);
          ((T*)y)[(long long)m * N + n] = Elt<DT>::from_f32(v);
        }
      }
    }
}

// y[m][n] = act(((slab[0] + slab[1]) + ...) + bias[n]): fixed order, one rounding of the store
template <int DT>
__global__ __launch_bounds__(256) void dense_combine_kernel(const float* __restrict__ slab, int splits,
                                                            const float* __restrict__ bias, char* y, long long MN, int N,
                                                            int relu) {
  typedef typename Elt<DT>::type T;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < MN; i += (long long)gridDim.x * 1024) {
    f32x4 s = *(const f32x4*)(slab + i);
    for (int k = 1; k < splits; ++k) s += *(const f32x4*)(slab + k * MN + i);
    const int n = (int)(i % N);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = s[e] + (bias ? bias[n + e] : 0.f);
      if (relu) v = fmaxf(v, 0.f);
      ((T*)y)[i + e] = Elt<DT>::from_f32(v);
    }
  }
}

// nn.Linear weight w[N][K] fp32 -> forward image wp[n][k'] / data-gradient image wd[k'][n], k' = p*C + c for the
// state-dict column c*HW + p (C = K / HW; HW = 1: k' = k)
template <int DT>
__global__ __launch_bounds__(256) void pack_dense_kernel(const float* __restrict__ w, char* packed, int N, int K, int hw,
                                                         int dgrad) {
  typedef typename Elt<DT>::type T;
  const long long total = (long long)N * K;
  const int C = K / hw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(dgrad ? i % N : i / K), kp = (int)(dgrad ? i / N : i % K);
    const int p = kp / C, c = kp - p * C;
    ((T*)packed)[i] = Elt<DT>::from_f32(w[(long long)n * K + (long long)c * hw + p]);
  }
}

// ---- weight gradient: dW[n][perm(k')] (=|+=) sum_m dz[m][n] x[m][k'] -------------------------------------------------
// Both operands have the reduction index m as their slow index; the exact-f32 MFMA (32x32x2: one k per lane half)
// takes one element per lane, 32 lanes = 32 consecutive columns, so no transpose is needed; bf16 operands are widened on
// load (their products are exact in fp32).  Wave = 32 n x 128 k' (four accumulator tiles share the dz operand) over all M
// rows: one chain per output, no split; the N K / 4096 waves are the parallelism.
constexpr int DWG_UNROLL = 8, DWG_KT = 4;
template <int DT>
__global__ __launch_bounds__(256) void dense_wgrad_kernel(const char* __restrict__ x, const char* __restrict__ dz,
                                                          float* gw, int M, int N, int K, int hw, int accumulate) {
  typedef typename Elt<DT>::type T;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int tiles_k = (K + 32 * DWG_KT - 1) / (32 * DWG_KT);
  const int tile = blockIdx.x * 4 + wv;
  if (tile >= (N / 32) * tiles_k) return;
  const int nt = tile / tiles_k, kt = tile - nt * tiles_k;
  f32x16 acc[DWG_KT];
#pragma unroll
  for (int j = 0; j < DWG_KT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  const T* ga = (const T*)dz + nt * 32 + r;
  const T* xb[DWG_KT];
#pragma unroll
  for (int j = 0; j < DWG_KT; ++j) xb[j] = (const T*)x + min(kt * 32 * DWG_KT + j * 32 + r, K - 1);  // clamped, not stored
  for (int m0 = 0; m0 < M; m0 += 2 * DWG_UNROLL) {
    float av[DWG_UNROLL], bv[DWG_UNROLL][DWG_KT];
#pragma unroll
    for (int u = 0; u < DWG_UNROLL; ++u) {
      const int m = m0 + 2 * u + hh;
      const bool ok = m < M;
      const int mc = ok ? m : M - 1;
      const float a = Elt<DT>::to_f32(ga[(long long)mc * N]);
      av[u] = ok ? a : 0.f;
#pragma unroll
      for (int j = 0; j < DWG_KT; ++j) bv[u][j] = Elt<DT>::to_f32(xb[j][(long long)mc * K]);
    }
#pragma unroll
    for (int u = 0; u < DWG_UNROLL; ++u)
#pragma unroll
      for (int j = 0; j < DWG_KT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][j], acc[j], 0, 0, 0);
  }
  const int C = K / hw;
#pragma unroll
  for (int j = 0; j < DWG_KT; ++j) {
    const int kp = kt * 32 * DWG_KT + j * 32 + r;
    if (kp >= K) continue;
    const int p = kp / C, c = kp - p * C;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = nt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      float* o = gw + (long long)n * K + (long long)c * hw + p;
      *o = accumulate ? *o + acc[j][e] : acc[j][e];
    }
  }
}

static int dense_check(const char* what, int dtype, int m, int n, int k) {
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "%s: bad dtype %d", what, dtype);
  SFVOS_REQUIRE(m >= 1 && m <= (1 << 20), "%s: rows %d out of [1, 2^20]", what, m);
  SFVOS_REQUIRE(n > 0 && k > 0 && n % 32 == 0 && k % 32 == 0 && n <= (1 << 20) && k <= (1 << 20),
                "%s: features must be positive multiples of 32 (in %d, out %d)", what, k, n);
  return SFVOS_OK;
}

// K split of a [m][n] output over k inputs: as many splits as bring the workgroups to about one per compute unit,
// each of at least four stages
static int dense_split(int dtype, int m, int n, int k, int* stages_per_split) {
  const int ce = 16 / elt_bytes(dtype);
  const int stages = ceil_div(k / ce, 8);
  const int tiles = ceil_div(m, DN_TILE) * ceil_div(n, DN_TILE);
  int want = device_cu_count() / tiles;
  want = want < 1 ? 1 : want > DN_MAX_SPLITS ? DN_MAX_SPLITS : want;
  if (want > stages / 4) want = stages / 4 < 1 ? 1 : stages / 4;
  const int per = ceil_div(stages, want);
  *stages_per_split = per;
  return ceil_div(stages, per);
}
}  // namespace sfvos

using namespace sfvos;

static int pack_dense(const char* what, const float* w, void* packed, int dtype, int n, int k, int hw, int dgrad,
                      sfvos_stream_t stream) {
  SFVOS_REQUIRE(w && packed, "%s: null pointer", what);
  if (int rc = dense_check(what, dtype, 1, n, k)) return rc;
  SFVOS_REQUIRE(hw >= 1 && k % hw == 0, "%s: positions %d do not divide the %d input features", what, hw, k);
  return launch_dt(dtype, what, [&](auto dt) {
    hipLaunchKernelGGL(pack_dense_kernel<dt>, dim3(grid_for((long long)n * k, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (char*)packed, n, k, hw, dgrad);
  });
}

extern "C" int sfvos_pack_dense_fwd(const float* w, void* packed, int dtype, int n_out, int k_in, int positions,
                                    sfvos_stream_t stream) {
  return pack_dense("pack_dense_fwd", w, packed, dtype, n_out, k_in, positions, 0, stream);
}

extern "C" int sfvos_pack_dense_dgrad(const float* w, void* packed, int dtype, int n_out, int k_in, int positions,
                                      sfvos_stream_t stream) {
  return pack_dense("pack_dense_dgrad", w, packed, dtype, n_out, k_in, positions, 1, stream);
}

extern "C" int sfvos_dense_splits(int dtype, int m, int n, int k) {
  int per;
  if (dense_check("dense_splits", dtype, m, n, k)) return 0;
  return dense_split(dtype, m, n, k, &per);
}

extern "C" size_t sfvos_dense_workspace_bytes(int dtype, int m, int n, int k) {
  const int splits = sfvos_dense_splits(dtype, m, n, k);
  return splits > 1 ? (size_t)splits * m * n * sizeof(float) : 0;
}

extern "C" int sfvos_dense(const void* x, const void* w_packed, const float* bias, void* y, int dtype, int m, int n,
                           int k, int relu, void* workspace, sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && w_packed && y, "dense: null pointer");
  if (int rc = dense_check("dense", dtype, m, n, k)) return rc;
  int per;
  const int splits = dense_split(dtype, m, n, k, &per);
  SFVOS_REQUIRE(splits == 1 || workspace, "dense: %d K splits need the workspace of sfvos_dense_workspace_bytes", splits);
  float* slab = splits > 1 ? (float*)workspace : nullptr;
  dim3 grid((unsigned)ceil_div(n, DN_TILE), (unsigned)ceil_div(m, DN_TILE), (unsigned)splits);
  int attr_rc = SFVOS_OK;
  int rc = launch_dt(dtype, "dense", [&](auto dt) {
    static LdsAttrOnce once;
    attr_rc = once.ensure((const void*)dense_kernel<dt>, DN_LDS, "dense");
    if (attr_rc) return;
    hipLaunchKernelGGL(dense_kernel<dt>, grid, dim3(256), DN_LDS, (hipStream_t)stream, (const char*)x,
                       (const char*)w_packed, bias, (char*)y, slab, m, n, k, relu, per);
  });
  if (attr_rc || rc || splits == 1) return attr_rc ? attr_rc : rc;
  const long long mn = (long long)m * n;
  return launch_dt(dtype, "dense", [&](auto dt) {
    hipLaunchKernelGGL(dense_combine_kernel<dt>, dim3(grid_for(mn, 1024)), dim3(256), 0, (hipStream_t)stream, slab,
                       splits, bias, (char*)y, mn, n, relu);
  }, "dense_combine");
}

extern "C" int sfvos_dense_wgrad(const void* x, const void* dz, int dtype, int m, int n, int k, int positions,
                                 float* grad_w, int accumulate, sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && dz && grad_w, "dense_wgrad: null pointer");
  if (int rc = dense_check("dense_wgrad", dtype, m, n, k)) return rc;
  SFVOS_REQUIRE(positions >= 1 && k % positions == 0, "dense_wgrad: positions %d do not divide the %d input features",
                positions, k);
  const int tiles = (n / 32) * ceil_div(k, 32 * DWG_KT);
  return launch_dt(dtype, "dense_wgrad", [&](auto dt) {
    hipLaunchKernelGGL(dense_wgrad_kernel<dt>, dim3((unsigned)ceil_div(tiles, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const char*)x, (const char*)dz, grad_w, m, n, k, positions, accumulate);
  });
}
