// project.hip -- the last step of both branches of roi_heads and its backward: an fp32 projection of channels-last rows
// onto a handful of outputs (mask branch: mask_fcn_logits, conv1x1 C -> K, torchvision's MaskRCNNPredictor; box branch:
// cls_score + bbox_pred, C -> K + 4K, FastRCNNPredictor).  One kernel pair serves both.
//
// A projection is (J0, J1, P): rows m = n*P + p of x [M][C]; output j < J0 belongs to block 0 (weights w0[j][c]),
// output j >= J0 to block 1 (weights w1[j - J0][c]); element (m, j) of an output or gradient block b with Jb columns
// lives at (n*Jb + j_b)*P + p.  Mask head: (K, 0, positions) -> [n][k][p];  box head: (K, 4K, 1) -> [m][k] | [m][4k].
// Everything is summed in a fixed order (no atomics): bit-identical from run to run.
#include "elt_util.h"

namespace sfvos {

// ---- forward: one wave per row, 64 lanes x C/64 channels, shuffle reduction, then the bias ---------------------------
// out0 == NULL (mask inference): only the channel of labels[n] is computed.  prob [n][1][p] (optional) = sigmoid of
// that channel (maskrcnn_inference).  BLOCKS = 1 (J1 == 0) or 2: the mask head's instance carries no code for block 1
// (with that code, rolled or not, its 100 352 one-row waves at 128 RoIs measured 1 - 2.5 us of 44 slower).
// 27 (BLOCKS 1) / 33 (2) VGPRs for both dtypes, no LDS, no scratch.
template <int DT, int BLOCKS>
__global__ __launch_bounds__(256) void project_kernel(const char* __restrict__ x, const float* __restrict__ w0,
                                                      const float* __restrict__ b0, const float* __restrict__ w1,
                                                      const float* __restrict__ b1,
                                                      const long long* __restrict__ labels, long long M, int P, int C,
                                                      int J0, int J1, float* out0, float* out1, float* prob) {
  typedef typename Elt<DT>::type T;
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int n = (int)(m / P), p = (int)(m - (long long)n * P);
  const T* xr = (const T*)x + m * C;
  const long long o0 = (long long)n * J0 * P + p, o1 = (long long)n * J1 * P + p;   // element (m, 0) of the two blocks
  // a label outside [0, J0) selects no channel: prob becomes NaN (torch raises an index error there; an
  // out-of-range label must never turn into an out-of-bounds access or an uninitialised result)
  const long long lab64 = labels ? labels[n] : 0;
  const int lab = (lab64 >= 0 && lab64 < J0) ? (int)lab64 : -1;
  if (prob && lab < 0 && lane == 0) prob[m] = __builtin_nanf("");
  // block by block; kept a loop: unrolled into one copy per block, the compiler loads block 1's arguments behind
  // block 0, and the box head's launch (512 RoIs, bf16) measured 1.2 us of 44 slower
#pragma nounroll
  for (int b = 0; b < BLOCKS; ++b) {
    const float* __restrict__ w = b ? w1 : w0;
    const float* __restrict__ bias = b ? b1 : b0;
    float* out = b ? out1 : out0;
    const long long o = b ? o1 : o0;
    const int Jb = b ? J1 : J0;
    for (int j = 0; j < Jb; ++j) {
      const bool chosen = b == 0 && j == lab;   // the labels select from block 0
      if (!out && !chosen) continue;
      float s = 0.f;
      for (int c = lane; c < C; c += 64) s += Elt<DT>::to_f32(xr[c]) * w[(long long)j * C + c];
#pragma unroll
      for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k);
      s += bias ? bias[j] : 0.f;
      if (lane == 0) {
        if (out) out[o + (long long)j * P] = s;
        if (prob && chosen) prob[m] = 1.f / (1.f + expf(-s));
      }
    }
  }
}

// ---- backward, and the ReLU in front of the projection ------------------------------------------------------------------
// g[m][j] = (g0 | g1)[m][j], w[j][c] = (w0 | w1)[j][c], J = J0 + J1:
//   dz[m][c] = (relu == 0 || x[m][c] > 0) ? sum_j g[m][j] w[j][c] : 0
//   part[row block] = [ sum_m g[m][j] x[m][c]  (J x C) | sum_m g[m][j]  (J) | sum_m dz[m][c]  (C) ]  over PB_ROWS rows
// thread = one column c, grid (row blocks, ceil(C / 256)); the rows' g sit in LDS, zero beyond the block's rows and J.
// Instances, picked by J (hipcc -Rpass-analysis=kernel-resource-usage, f32 / bf16; no scratch, no spills):
//   JMAX  2:  42 /  37 VGPRs,    512 bytes of LDS, 8 waves per SIMD   (the mask head's two classes)
//   JMAX 10:  62 /  62 VGPRs,  2 560 bytes,        8 waves per SIMD   (mask head up to 8 classes; box head with 1 or 2)
//   JMAX 40: 125 / 126 VGPRs, 10 240 bytes,        4 waves per SIMD   (box head with 3 to 8 classes)
// Outputs beyond J are zeros in LDS and in wr: they add exact zeros.
constexpr int PB_ROWS = 64;
template <int DT, int JMAX>
__global__ __launch_bounds__(256) void project_bwd_kernel(const char* __restrict__ x, const float* __restrict__ g0,
                                                          const float* __restrict__ g1, const float* __restrict__ w0,
                                                          const float* __restrict__ w1, long long M, int P, int C, int J0,
                                                          int J1, int relu, char* dz, float* part) {
  typedef typename Elt<DT>::type T;
  __shared__ float g[PB_ROWS][JMAX];
  const int J = J0 + J1, L = J * C + J + C;
  const long long m0 = (long long)blockIdx.x * PB_ROWS;
  const int rows = (int)min((long long)PB_ROWS, M - m0);
  {
    const int r = threadIdx.x & 63;   // wave = one column j of the block's rows
    const long long n = (m0 + r) / P, p = m0 + r - n * P;
    for (int j = threadIdx.x >> 6; j < JMAX; j += 4) {
      float v = 0.f;
      if (r < rows && j < J) v = j < J0 ? g0[(n * J0 + j) * P + p] : g1[(n * J1 + j - J0) * P + p];
      g[r][j] = v;
    }
  }
  __syncthreads();
  float* out = part + (long long)blockIdx.x * L;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (blockIdx.y == 0 && (int)threadIdx.x < J) {
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += g[r][threadIdx.x];
    out[J * C + threadIdx.x] = s;
  }
  if (c >= C) return;
  float aw[JMAX], wr[JMAX];
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    aw[j] = 0.f;
    wr[j] = j < J ? (j < J0 ? w0[(long long)j * C + c] : w1[(long long)(j - J0) * C + c]) : 0.f;
  }
  float cs = 0.f;
  for (int r = 0; r < rows; ++r) {
    const long long o = (m0 + r) * C + c;
    const float xv = Elt<DT>::to_f32(((const T*)x)[o]);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      aw[j] += g[r][j] * xv;
      d += g[r][j] * wr[j];
    }
    if (relu && !(xv > 0.f)) d = 0.f;
    cs += d;
    ((T*)dz)[o] = Elt<DT>::from_f32(d);
  }
#pragma unroll
  for (int j = 0; j < JMAX; ++j)
    if (j < J) out[(long long)j * C + c] = aw[j];
  out[J * C + J + c] = cs;
}

static int launch_project(const char* what, const void* x, int dtype, const float* w0, const float* b0, const float* w1,
                          const float* b1, const int64_t* labels, long long M, int P, int C, int J0, int J1, float* out0,
                          float* out1, float* prob, sfvos_stream_t stream) {
  return launch_dt(dtype, what, [&](auto dt) {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div64(M, 4)), dim3(256), 0, (hipStream_t)stream, (const char*)x, w0,
                         b0, w1, b1, (const long long*)labels, M, P, C, J0, J1, out0, out1, prob);
    };
    if (J1 > 0)
      go(project_kernel<dt, 2>);
    else
      go(project_kernel<dt, 1>);
  });
}

static int launch_project_bwd(const char* what, const void* x, int dtype, const float* g0, const float* g1,
                              const float* w0, const float* w1, long long M, int P, int C, int J0, int J1, int relu,
                              void* dz, float* part, sfvos_stream_t stream) {
  const dim3 grid((unsigned)ceil_div64(M, PB_ROWS), (unsigned)ceil_div(C, 256));
  return launch_dt(dtype, what, [&](auto dt) {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, (const char*)x, g0, g1, w0, w1, M, P, C, J0, J1,
                         relu, (char*)dz, part);
    };
    if (J0 + J1 <= 2)
      go(project_bwd_kernel<dt, 2>);
    else if (J0 + J1 <= 10)
      go(project_bwd_kernel<dt, 10>);
    else
      go(project_bwd_kernel<dt, 5 * HEAD_MAXK>);
  });
}
}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_mask_logits(const void* x, int dtype, const float* w, const float* bias, const int64_t* labels,
                                 int n, int positions, int c, int num_classes, float* logits, float* prob,
                                 sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && w && n > 0 && positions > 0 && c > 0 && num_classes > 0 && (logits || prob),
                "mask_logits: bad argument");
  SFVOS_REQUIRE(!prob || labels || num_classes == 1, "mask_logits: prob needs the labels of the boxes");
  return launch_project("mask_logits", x, dtype, w, bias, nullptr, nullptr, labels, (long long)n * positions, positions,
                        c, num_classes, 0, logits, nullptr, prob, stream);
}

extern "C" int sfvos_box_predictor(const void* x, int dtype, const float* w_cls, const float* b_cls, const float* w_box,
                                   const float* b_box, int m, int c, int num_classes, float* logits, float* deltas,
                                   sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && w_cls && w_box && logits && deltas && m > 0 && c > 0, "box_predictor: bad argument");
  if (int rc = check_classes("box_predictor", num_classes)) return rc;
  return launch_project("box_predictor", x, dtype, w_cls, b_cls, w_box, b_box, nullptr, m, 1, c, num_classes,
                        4 * num_classes, logits, deltas, nullptr, stream);
}

extern "C" int sfvos_mask_logits_bwd_rows(int n, int positions) {
  return n > 0 && positions > 0 ? (int)ceil_div64((long long)n * positions, PB_ROWS) : 0;
}

extern "C" int sfvos_mask_logits_bwd(const void* y, int dtype, const float* dlogits, const float* w, int n, int positions,
                                     int c, int num_classes, int relu, void* dz, float* part, sfvos_stream_t stream) {
  SFVOS_REQUIRE(y && dlogits && w && dz && part && n > 0 && positions > 0, "mask_logits_bwd: bad argument");
  SFVOS_REQUIRE(c > 0 && c % 64 == 0 && c <= 512 && num_classes > 0 && num_classes <= HEAD_MAXK,
                "mask_logits_bwd: C must be a multiple of 64 (<= %d), num_classes <= %d", 512, HEAD_MAXK);
  return launch_project_bwd("mask_logits_bwd", y, dtype, dlogits, nullptr, w, nullptr, (long long)n * positions,
                            positions, c, num_classes, 0, relu, dz, part, stream);
}

extern "C" int sfvos_box_predictor_bwd_rows(int m) { return m > 0 ? ceil_div(m, PB_ROWS) : 0; }

extern "C" int sfvos_box_predictor_bwd(const void* x, int dtype, const float* dlogits, const float* ddeltas,
                                       const float* w_cls, const float* w_box, int m, int c, int num_classes, int relu,
                                       void* dz, float* part, sfvos_stream_t stream) {
  SFVOS_REQUIRE(x && dlogits && ddeltas && w_cls && w_box && dz && part && m > 0 && c > 0,
                "box_predictor_bwd: bad argument");
  if (int rc = check_classes("box_predictor_bwd", num_classes)) return rc;
  return launch_project_bwd("box_predictor_bwd", x, dtype, dlogits, ddeltas, w_cls, w_box, m, 1, c, num_classes,
                            4 * num_classes, relu, dz, part, stream);
}
