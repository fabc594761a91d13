// body.hip -- the ResNet-50 body in front of the feature pyramid network (torchvision's resnet50 through
// IntermediateLayerGetter, every BatchNorm a FrozenBatchNorm2d; frozen in the reference: inference only).
//
// sfvos_conv2d: every conv of the 16 bottlenecks, an implicit GEMM on channels-last activations with the frozen norm's
//   affine, the residual and the ReLU in its epilogue.  K runs over (tap, channel); a slab of the K loop is 128 bytes of one
//   tap (64 bf16 / 32 f32 channels: c_in is a multiple of 64, so a slab never straddles two taps).  The weight image
//   [c_out][taps][c_in] in the compute dtype is the A operand as it lies, the gathered positions are B, so of the C/D tile
//   a lane holds one POSITION (column lane & 31) and four consecutive CHANNELS per register quad (rows): scale, shift,
//   residual and the store are 4-element vectors.
//   Workgroup = 4 waves; both operands of a slab go global -> registers one slab ahead, registers -> LDS behind the
//   barrier (rows of 128 + 16 bytes: the 16 spread consecutive rows over the banks).  A position outside the image is a
//   chunk of zeros (never loaded).  Three tiles (channels x positions): 128 x 128 (waves 2 x 2, 64 x 64 each), 64 x 128
//   (waves side by side over the positions, 64 x 32 each) and 64 x 64 (waves 2 x 2, 32 x 32 each); conv2d_plan takes the
//   largest that still fills the chip, and where even the smallest does not (layer4: 1008 positions), the slabs of K are
//   split over gridDim.y: every split writes its fp32 tile to a workspace slab, and conv2d_combine_kernel adds the slabs
//   in split order and applies the epilogue (fixed order: deterministic, no atomics).
// sfvos_body_stem: conv1 (7x7, stride 2, pad 3, 3 -> 64) + affine + ReLU straight from the planar fp32 image.  K is laid
//   out as (channel, dh) rows of 8 with dw in 0..6 (the eighth weight is zero, its x is never loaded): 21 rows + 1 row of
//   zeros = 176.  The weights (64 x 176) sit in LDS for the whole workgroup; a lane gathers its position's chunk from the
//   image (7 consecutive floats of one row) and rounds it to the compute dtype in registers.
// sfvos_maxpool3x3s2: max_pool2d(3, 2, 1) channels-last, one 16-byte chunk per thread, padding -inf.
#include "elt_util.h"

namespace sfvos {

constexpr int CV_ROWB = 128 + 16;   // bytes of a staged row: one K slab of one channel / position, padded

struct Conv2dArgs {
  const void* x;
  const void* w;
  const float* scale;
  const float* shift;
  const void* res;
  void* y;
  float* slab;              // K splits: [splits][P][c_out] fp32; NULL without a split
  int h, w_, oh, ow, P;     // input sides, output sides, output positions of the batch
  int c_in, c_out, taps, stride, ld_x, ld_y, ld_res, relu;
  int n_tiles;              // channel tiles of the launch (blockIdx.x = position tile * n_tiles + channel tile)
  int slabs, per;           // K slabs in all, slabs per split (blockIdx.y)
};

// acc quad -> scale, shift, residual, ReLU, one rounding, one 4-element store
template <int DT>
__device__ __forceinline__ void conv2d_finish(const Conv2dArgs& a, long long p, int n, const float* v) {
  typedef typename Elt<DT>::type T;
  const f32x4 sc = *(const f32x4*)(a.scale + n), sh = *(const f32x4*)(a.shift + n);
  float o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = v[q] * sc[q] + sh[q];
  if (a.res) {
    const T* rp = (const T*)a.res + p * a.ld_res + n;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] += Elt<DT>::to_f32(rp[q]);
  }
  if (a.relu) {
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = fmaxf(o[q], 0.f);
  }
  T* yp = (T*)a.y + p * a.ld_y + n;
  if constexpr (DT == SFVOS_F32) {
    f32x4 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = o[q];
    *(f32x4*)yp = r;
  } else {
    bf16x4 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = (__bf16)o[q];
    *(bf16x4*)yp = r;
  }
}

// WN x WM: 32 x 32 MFMA tiles of a wave (channels x positions); GN: waves along the channels (4 / GN along the positions)
template <int DT, int WN, int WM, int GN>
__global__ __launch_bounds__(256, 2) void conv2d_kernel(const Conv2dArgs a) {
  constexpr int CE = Elt<DT>::CE, ES = 16 / CE;
  constexpr int GM = 4 / GN, BN = GN * WN * 32, BM = GM * WM * 32;
  constexpr int KCH = 8 * CE;                 // channels of a slab
  constexpr int NA = BN / 32, NB = BM / 32;   // 16-byte chunks a thread stages per slab, weights / positions
  __shared__ __attribute__((aligned(16))) char smem[(BN + BM) * CV_ROWB];
  char* const sw = smem;
  char* const sx = smem + BN * CV_ROWB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hf = lane >> 5;
  const int ntile = blockIdx.x % a.n_tiles, mtile = blockIdx.x / a.n_tiles;
  const int n0 = ntile * BN;
  const long long m0 = (long long)mtile * BM;
  const int wn = wave % GN, wm = wave / GN;
  const int pad = a.taps == 9 ? 1 : 0;

  // staging: thread -> chunk (tid & 7) of rows (tid >> 3) + 32 i
  const int srow = tid >> 3, scc = tid & 7;
  const char* wsrc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i)
    wsrc[i] = (const char*)a.w + (long long)(n0 + srow + 32 * i) * a.taps * a.c_in * ES + scc * 16;
  long long xoff[NB];   // byte offset of tap (0, 0), channel chunk scc of each row's position; may lie outside x
  int ih0[NB], iw0[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const long long p = m0 + srow + 32 * i;
    const unsigned pl = (unsigned)(p < a.P ? p : 0);
    const unsigned ohw = (unsigned)(a.oh * a.ow);
    const unsigned b = pl / ohw, rem = pl - b * ohw;
    const unsigned oi = rem / (unsigned)a.ow, oj = rem - oi * (unsigned)a.ow;
    ih0[i] = p < a.P ? (int)oi * a.stride - pad : -(1 << 20);   // rows past the end: every tap out of range
    iw0[i] = (int)oj * a.stride - pad;
    xoff[i] = (((long long)b * a.h + (p < a.P ? ih0[i] : 0)) * a.w_ + iw0[i]) * a.ld_x * ES + scc * 16;
  }

  u32x4 wreg[NA], xreg[NB];
  auto load = [&](int kb) {
    const int k0 = kb * KCH, tap = k0 / a.c_in, c0 = k0 - tap * a.c_in;
    const int dh = tap / 3, dw = tap - 3 * dh;      // taps == 1: tap = 0
#pragma unroll
    for (int i = 0; i < NA; ++i) wreg[i] = *(const u32x4*)(wsrc[i] + (long long)k0 * ES);
    const long long xo = ((long long)(dh * a.w_ + dw) * a.ld_x + c0) * ES;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool in = (unsigned)(ih0[i] + dh) < (unsigned)a.h && (unsigned)(iw0[i] + dw) < (unsigned)a.w_;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (in) v = *(const u32x4*)((const char*)a.x + (xoff[i] + xo));
      xreg[i] = v;
    }
  };

  f32x16 acc[WN][WM];
#pragma unroll
  for (int t = 0; t < WN; ++t)
#pragma unroll
    for (int u = 0; u < WM; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

  const int kb_begin = blockIdx.y * a.per;
  const int kb_end = kb_begin + a.per < a.slabs ? kb_begin + a.per : a.slabs;
  load(kb_begin);
  for (int kb = kb_begin; kb < kb_end; ++kb) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *(u32x4*)(sw + (srow + 32 * i) * CV_ROWB + scc * 16) = wreg[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *(u32x4*)(sx + (srow + 32 * i) * CV_ROWB + scc * 16) = xreg[i];
    __syncthreads();
    if (kb + 1 < kb_end) load(kb + 1);   // in flight while this slab is multiplied
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 af[WN], bf[WM];
#pragma unroll
      for (int t = 0; t < WN; ++t) af[t] = lds_read16(sw + ((wn * WN + t) * 32 + r) * CV_ROWB + (2 * s + hf) * 16);
#pragma unroll
      for (int u = 0; u < WM; ++u) bf[u] = lds_read16(sx + ((wm * WM + u) * 32 + r) * CV_ROWB + (2 * s + hf) * 16);
#pragma unroll
      for (int t = 0; t < WN; ++t)
#pragma unroll
        for (int u = 0; u < WM; ++u) Mma<DT>::run(acc[t][u], af[t], bf[u]);
    }
    __syncthreads();
  }

  // register 4 g + q of lane half hf: channel row 8 g + 4 hf + q of the 32-channel tile, position column r
#pragma unroll
  for (int u = 0; u < WM; ++u) {
    const long long p = m0 + (wm * WM + u) * 32 + r;
    if (p >= a.P) continue;
#pragma unroll
    for (int t = 0; t < WN; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + (wn * WN + t) * 32 + 8 * g + 4 * hf;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[t][u][4 * g + q];
        if (a.slab) {
          f32x4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = v[q];
          *(f32x4*)(a.slab + ((long long)blockIdx.y * a.P + p) * a.c_out + n) = o;
        } else {
          conv2d_finish<DT>(a, p, n, v);
        }
      }
  }
}

// y = epilogue(sum over the splits, in split order, of slab[split][p][n]); one channel quad per thread
template <int DT>
__global__ __launch_bounds__(256) void conv2d_combine_kernel(const Conv2dArgs a, int splits) {
  const int quads = a.c_out >> 2;
  const long long total = (long long)a.P * quads;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long p = idx / quads;
    const int n = (int)(idx - p * quads) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < splits; ++z) {
      const f32x4 s = *(const f32x4*)(a.slab + ((long long)z * a.P + p) * a.c_out + n);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += s[q];
    }
    conv2d_finish<DT>(a, p, n, v);
  }
}

// ---- stem ------------------------------------------------------------------------------------------------------------
constexpr int STEM_KP = 176;    // (3 channels x 7 rows + 1 row of zeros) x 8
constexpr int STEM_C = 64;

struct StemArgs {
  const float* x;
  long long stride_b, stride_c, stride_h;
  const void* w;
  const float* scale;
  const float* shift;
  void* y;
  int h, w_, oh, ow, P, ld_y;
};

template <int DT>
__global__ __launch_bounds__(256, 2) void body_stem_kernel(const StemArgs a) {
  typedef typename Elt<DT>::type T;
  constexpr int CE = Elt<DT>::CE, ES = 16 / CE;
  constexpr int ROWB = STEM_KP * ES + 16;
  constexpr int CPR = STEM_KP / CE;           // 16-byte chunks of a weight row
  constexpr int STEPS = CPR / 2;
  __shared__ __attribute__((aligned(16))) char smem[STEM_C * ROWB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hf = lane >> 5;
  for (int c = tid; c < STEM_C * CPR; c += 256) {
    const int row = c / CPR, cc = c - row * CPR;
    *(u32x4*)(smem + row * ROWB + cc * 16) = *(const u32x4*)((const char*)a.w + ((long long)row * CPR + cc) * 16);
  }
  __syncthreads();

  const long long p = ((long long)blockIdx.x * 4 + wave) * 32 + r;
  const unsigned pl = (unsigned)(p < a.P ? p : a.P - 1);    // lanes past the end compute the last position, store nothing
  const unsigned ohw = (unsigned)(a.oh * a.ow);
  const unsigned b = pl / ohw, rem = pl - b * ohw;
  const unsigned oi = rem / (unsigned)a.ow, oj = rem - oi * (unsigned)a.ow;
  const int ih0 = 2 * (int)oi - 3, iw0 = 2 * (int)oj - 3;
  const float* xb = a.x + b * a.stride_b;

  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

#pragma unroll 2
  for (int s = 0; s < STEPS; ++s) {
    const int q = 2 * s + hf;                          // this lane's chunk of K
    const int rc = CE == 8 ? q : q >> 1;               // (channel, dh) row of the chunk; 21 = the row of zeros
    const int dw0 = CE == 8 ? 0 : (q & 1) * 4;
    const int c = rc / 7, dh = rc - 7 * c;
    const int ih = ih0 + dh;
    const bool row_in = rc < 21 && (unsigned)ih < (unsigned)a.h;
    const float* xr = xb + c * a.stride_c + (long long)(row_in ? ih : 0) * a.stride_h;
    float f[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      const int iw = iw0 + dw0 + e;
      const bool in = row_in && dw0 + e < 7 && (unsigned)iw < (unsigned)a.w_;
      f[e] = in ? xr[iw] : 0.f;
    }
    const u32x4 bf = pack<DT>(f);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const u32x4 af = lds_read16(smem + (t * 32 + r) * ROWB + q * 16);
      Mma<DT>::run(acc[t], af, bf);
    }
  }

  if (p >= a.P) return;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = t * 32 + 8 * g + 4 * hf;
      const f32x4 sc = *(const f32x4*)(a.scale + n), sh = *(const f32x4*)(a.shift + n);
      T* yp = (T*)a.y + p * a.ld_y + n;
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = fmaxf(acc[t][4 * g + k] * sc[k] + sh[k], 0.f);
      if constexpr (DT == SFVOS_F32) {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = o[k];
        *(f32x4*)yp = v;
      } else {
        bf16x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (__bf16)o[k];
        *(bf16x4*)yp = v;
      }
    }
}

// ---- max pool 3 x 3, stride 2, pad 1 -----------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                           long long total, int h, int w, int oh, int ow, int chunks,
                                                           int lds, int ldd) {
  constexpr int CE = Elt<DT>::CE;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % chunks);
    const long long pos = idx / chunks;
    const int j = (int)(pos % ow);
    const long long bi = pos / ow;
    const int i = (int)(bi % oh);
    const long long b = bi / oh;
    float m[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) m[e] = -__builtin_huge_valf();
#pragma unroll
    for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
      for (int dw = -1; dw <= 1; ++dw) {
        const int ii = 2 * i + dh, jj = 2 * j + dw;
        if ((unsigned)ii < (unsigned)h && (unsigned)jj < (unsigned)w) {
          float f[CE];
          unpack<DT>(src[((b * h + ii) * w + jj) * lds + c], f);
#pragma unroll
          for (int e = 0; e < CE; ++e) m[e] = fmaxf(m[e], f[e]);
        }
      }
    dst[pos * ldd + c] = pack<DT>(m);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// tile ids of conv2d_plan: channels x positions of a workgroup; + CV_SPLIT with a K split (64 x 64 tiles only)
enum { CV_128x128 = 0, CV_64x128 = 1, CV_64x64 = 2, CV_SPLIT = 3 };
constexpr int CV_MAX_SPLITS = 8;

static int conv2d_check(const char* what, int dtype, int batch, int h, int w, int c_in, int c_out, int taps, int stride) {
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "%s: bad dtype %d (f32 or bf16)", what, dtype);
  SFVOS_REQUIRE(taps == 1 || taps == 9, "%s: taps must be 1 or 9, got %d", what, taps);
  SFVOS_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2, got %d", what, stride);
  SFVOS_REQUIRE(c_in > 0 && c_in % 64 == 0 && c_in <= 2048 && c_out > 0 && c_out % 64 == 0 && c_out <= 2048,
                "%s: channels must be multiples of 64 up to 2048 (c_in %d, c_out %d)", what, c_in, c_out);
  SFVOS_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && (long long)batch * h * w < (1ll << 31) - 128,
                "%s: bad extent (batch %d, %dx%d)", what, batch, h, w);
  return SFVOS_OK;
}

// the plan of a shape conv2d_check accepted: tile id (+ CV_SPLIT), splits and slabs per split
static int conv2d_pick(int dtype, int batch, int h, int w, int c_in, int c_out, int taps, int stride, int cus,
                       int* splits, int* per) {
  if (cus <= 0) cus = device_cu_count();
  const long long P = (long long)batch * ((h - 1) / stride + 1) * ((w - 1) / stride + 1);
  const int slabs = taps * c_in / (8 * (16 / elt_bytes(dtype)));
  *splits = 1;
  *per = slabs;
  // the largest tile that still gives 7 of 8 CUs a workgroup
  const long long fill = 7ll * cus;
  if (c_out % 128 == 0 && 8 * ceil_div64(P, 128) * (c_out / 128) >= fill) return CV_128x128;
  if (8 * ceil_div64(P, 128) * (c_out / 64) >= fill) return CV_64x128;
  const long long tiles = ceil_div64(P, 64) * (c_out / 64);
  if (8 * tiles >= fill) return CV_64x64;
  // too few positions: split K so that the workgroups fill the chip, at least two slabs per split
  long long want = ceil_div64(cus, tiles);
  if (want > CV_MAX_SPLITS) want = CV_MAX_SPLITS;
  if (want > slabs / 2) want = slabs / 2;
  if (want <= 1) return CV_64x64;
  *per = ceil_div(slabs, (int)want);
  *splits = ceil_div(slabs, *per);    // no empty split
  return *splits > 1 ? CV_64x64 + CV_SPLIT : CV_64x64;
}

}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_conv2d_plan(int dtype, int batch, int h, int w, int c_in, int c_out, int taps, int stride, int cus,
                                 int* splits) {
  if (splits) *splits = 0;
  if (int rc = conv2d_check("conv2d_plan", dtype, batch, h, w, c_in, c_out, taps, stride)) return rc;
  SFVOS_REQUIRE(cus >= 0, "conv2d_plan: cus %d must be >= 0 (0 = the current device's)", cus);
  int sp, per;
  const int id = conv2d_pick(dtype, batch, h, w, c_in, c_out, taps, stride, cus, &sp, &per);
  if (splits) *splits = sp;
  return id;
}

extern "C" size_t sfvos_conv2d_workspace_bytes(int dtype, int batch, int h, int w, int c_in, int c_out, int taps,
                                               int stride) {
  if (conv2d_check("conv2d_workspace_bytes", dtype, batch, h, w, c_in, c_out, taps, stride)) return 0;
  int sp, per;
  conv2d_pick(dtype, batch, h, w, c_in, c_out, taps, stride, 0, &sp, &per);
  const long long P = (long long)batch * ((h - 1) / stride + 1) * ((w - 1) / stride + 1);
  return sp > 1 ? (size_t)sp * P * c_out * sizeof(float) : 0;
}

template <int DT, int WN, int WM, int GN>
static void launch_conv2d(const Conv2dArgs& a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((conv2d_kernel<DT, WN, WM, GN>), grid, dim3(256), 0, s, a);
}

extern "C" int sfvos_conv2d(const void* x, int ld_x, const void* weight, const float* scale, const float* shift,
                            const void* residual, int ld_res, void* y, int ld_y, int batch, int h, int w, int c_in,
                            int c_out, int taps, int stride, int relu, int dtype, void* workspace,
                            sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && weight && scale && shift && y, "conv2d: null pointer");
  if (int rc = conv2d_check("conv2d", dtype, batch, h, w, c_in, c_out, taps, stride)) return rc;
  const int ce = 16 / elt_bytes(dtype);
  SFVOS_REQUIRE(ld_x >= c_in && ld_x % ce == 0, "conv2d: pitch ld_x %d must be >= c_in %d and a multiple of %d", ld_x, c_in,
                ce);
  SFVOS_REQUIRE(ld_y >= c_out && ld_y % ce == 0, "conv2d: pitch ld_y %d must be >= c_out %d and a multiple of %d", ld_y,
                c_out, ce);
  SFVOS_REQUIRE(!residual || (ld_res >= c_out && ld_res % ce == 0),
                "conv2d: pitch ld_res %d must be >= c_out %d and a multiple of %d", ld_res, c_out, ce);
  SFVOS_REQUIRE(relu == 0 || relu == 1, "conv2d: relu must be 0 or 1, got %d", relu);
  SFVOS_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)weight % 16 == 0 && (uintptr_t)y % 16 == 0 &&
                    (uintptr_t)residual % 16 == 0 && (uintptr_t)scale % 16 == 0 && (uintptr_t)shift % 16 == 0,
                "conv2d: x, weight, scale, shift, residual and y must be 16-byte aligned");
  int splits, per;
  const int id = conv2d_pick(dtype, batch, h, w, c_in, c_out, taps, stride, 0, &splits, &per);
  SFVOS_REQUIRE(splits == 1 || (workspace && (uintptr_t)workspace % 16 == 0),
                "conv2d: %d K splits need the 16-byte aligned workspace of sfvos_conv2d_workspace_bytes", splits);
  Conv2dArgs a;
  a.x = x; a.w = weight; a.scale = scale; a.shift = shift; a.res = residual; a.y = y;
  a.slab = splits > 1 ? (float*)workspace : nullptr;
  a.h = h; a.w_ = w; a.oh = (h - 1) / stride + 1; a.ow = (w - 1) / stride + 1; a.P = batch * a.oh * a.ow;
  a.c_in = c_in; a.c_out = c_out; a.taps = taps; a.stride = stride;
  a.ld_x = ld_x; a.ld_y = ld_y; a.ld_res = ld_res; a.relu = relu;
  a.slabs = taps * c_in / (8 * ce); a.per = per;
  const int tile = id % CV_SPLIT;
  const int bn = tile == CV_128x128 ? 128 : 64, bm = tile == CV_64x64 ? 64 : 128;
  a.n_tiles = c_out / bn;
  const long long wgs = ceil_div64(a.P, bm) * a.n_tiles;
  SFVOS_REQUIRE(wgs < (1ll << 31), "conv2d: grid of %lld workgroups out of range", wgs);
  const dim3 grid((unsigned)wgs, (unsigned)splits);
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_dt(dtype, "conv2d", [&](auto dt) {
    constexpr int D = decltype(dt)::value;
    if (tile == CV_128x128) launch_conv2d<D, 2, 2, 2>(a, grid, s);
    else if (tile == CV_64x128) launch_conv2d<D, 2, 1, 1>(a, grid, s);
    else launch_conv2d<D, 1, 1, 2>(a, grid, s);
  });
  if (rc || splits == 1) return rc;
  return launch_dt(dtype, "conv2d", [&](auto dt) {
    constexpr int D = decltype(dt)::value;
    hipLaunchKernelGGL((conv2d_combine_kernel<D>), dim3(grid_for((long long)a.P * (c_out / 4), 256)), dim3(256), 0, s, a,
                       splits);
  }, "conv2d (combine)");
}

extern "C" int sfvos_body_stem(const float* x, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                               int batch, int h, int w, const void* weight, const float* scale, const float* shift, void* y,
                               int ld_y, int dtype, sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && weight && scale && shift && y, "body_stem: null pointer");
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "body_stem: bad dtype %d (f32 or bf16)", dtype);
  SFVOS_REQUIRE(stride_w == 1, "body_stem: stride_w must be 1, got %lld", (long long)stride_w);
  SFVOS_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_h >= 0, "body_stem: negative stride");
  SFVOS_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && (long long)batch * h * w < (1ll << 31) - 128,
                "body_stem: bad extent (batch %d, %dx%d)", batch, h, w);
  const int ce = 16 / elt_bytes(dtype);
  SFVOS_REQUIRE(ld_y >= STEM_C && ld_y % ce == 0, "body_stem: pitch ld_y %d must be >= %d and a multiple of %d", ld_y,
                STEM_C, ce);
  SFVOS_REQUIRE((uintptr_t)weight % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)scale % 16 == 0 &&
                    (uintptr_t)shift % 16 == 0 && (uintptr_t)x % 4 == 0,
                "body_stem: weight, scale, shift and y must be 16-byte aligned (x: 4)");
  StemArgs a;
  a.x = x; a.stride_b = stride_b; a.stride_c = stride_c; a.stride_h = stride_h;
  a.w = weight; a.scale = scale; a.shift = shift; a.y = y;
  a.h = h; a.w_ = w; a.oh = (h - 1) / 2 + 1; a.ow = (w - 1) / 2 + 1; a.P = batch * a.oh * a.ow; a.ld_y = ld_y;
  const unsigned grid = (unsigned)ceil_div64(a.P, 128);
  return launch_dt(dtype, "body_stem", [&](auto dt) {
    hipLaunchKernelGGL((body_stem_kernel<decltype(dt)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  });
}

extern "C" int sfvos_maxpool3x3s2(const void* src, int ld_src, void* dst, int ld_dst, int batch, int h, int w, int C,
                                  int dtype, sfvos_stream_t stream) {
  SFVOS_REQUIRE(src && dst, "maxpool3x3s2: null pointer");
  SFVOS_REQUIRE(dtype == SFVOS_F32 || dtype == SFVOS_BF16, "maxpool3x3s2: bad dtype %d (f32 or bf16)", dtype);
  const int ce = 16 / elt_bytes(dtype);
  SFVOS_REQUIRE(C > 0 && C % ce == 0, "maxpool3x3s2: C %d must be a whole number of 16-byte chunks (%d elements)", C, ce);
  SFVOS_REQUIRE(ld_src >= C && ld_dst >= C && ld_src % ce == 0 && ld_dst % ce == 0,
                "maxpool3x3s2: pitches %d, %d must be >= C %d and multiples of %d", ld_src, ld_dst, C, ce);
  SFVOS_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && (long long)batch * h * w < (1ll << 31),
                "maxpool3x3s2: bad extent (batch %d, %dx%d)", batch, h, w);
  SFVOS_REQUIRE((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, "maxpool3x3s2: buffers must be 16-byte aligned");
  const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1, chunks = C / ce;
  const long long total = (long long)batch * oh * ow * chunks;
  return launch_dt(dtype, "maxpool3x3s2", [&](auto dt) {
    hipLaunchKernelGGL((maxpool3x3s2_kernel<decltype(dt)::value>), dim3(grid_for(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const u32x4*)src, (u32x4*)dst, total, h, w, oh, ow, chunks, ld_src / ce,
                       ld_dst / ce);
  });
}
