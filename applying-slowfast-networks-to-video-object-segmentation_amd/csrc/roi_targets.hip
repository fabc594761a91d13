// roi_targets.hip -- what turns proposals + ground truth into the arguments of roi_heads' losses in training
// (model.py:346 with targets, trained at :369), restated from torchvision's published sources (models/detection/
// roi_heads.py: select_training_samples, add_gt_proposals, assign_targets_to_proposals, project_masks_on_boxes; _utils.py:
// Matcher, BalancedPositiveNegativeSampler, BoxCoder; ops/boxes.py: box_iou; ops/roi_align.py with sampling_ratio <= 0) --
// parity unpinned by the reference, torchvision is neither vendored nor installed.  One image per call.
//
//   candidates = proposals followed by the ground truth; IoU matcher, labels         sfvos_roi_match
//   balanced sampler over explicit keys, gathers, BoxCoder(10, 10, 5, 5).encode      sfvos_roi_sample
//   RoIAlign (adaptive grid) of the matched ground-truth mask onto each positive     sfvos_mask_targets
//
// The only random input is the caller's key per candidate: the n smallest (key, index) pairs of a class are its sample.
// No atomics; ranks come from counting, slots from a prefix scan: every result is bit-identical from run to run.
#include "elt_util.h"

// Every fp32 operation below is rounded on its own (the IoU, the sample coordinates of the adaptive grid decide something
// and are restated operation by operation in tests/roi_targets_ref.py): no contraction into fused multiply-adds.  Plain
// operators under this pragma, not the _rn intrinsics: those are inline functions of a header in front of the pragma,
// whose multiply and add keep the default (contractable) flags and do fuse.
#pragma clang fp contract(off)

namespace sfvos {

constexpr int RT_MAX_N = 8192;       // candidates of one image: the ranking is N^2 compare steps (6.7e7 at the cap)
constexpr int RT_MAX_G = 1024;       // ground-truth boxes of one image
constexpr int RT_MAX_BATCH = 4096;   // batch_size_per_image
constexpr int RT_MAX_M = 64;         // side of a mask target

// candidate i of the list [proposals (n_p), ground truth (G)]
__device__ __forceinline__ const float* cand_box(const float* props, const float* gt, int n_p, int i) {
  return i < n_p ? props + 4 * (long long)i : gt + 4 * (long long)(i - n_p);
}

// ---- match: thread = candidate, the ground truth walks through LDS in tiles -----------------------------------------------
// IoU as rpn_iou_kernel / det_iou_kernel compute it: inter / (area_a + area_b - inter), fp32, every operation rounded on
// its own.  The largest IoU wins, the lower index on a tie; a NaN IoU never wins.
__global__ __launch_bounds__(256) void roi_match_kernel(const float* __restrict__ props, const float* __restrict__ gt,
                                                        const long long* __restrict__ gt_labels, int n_p, int G,
                                                        float high, float low, int* matched, long long* labels,
                                                        float* max_iou) {
  __shared__ float gb[256][4];
  const int N = n_p + G, i = blockIdx.x * 256 + threadIdx.x;
  const bool mine = i < N;
  float ax1 = 0.f, ay1 = 0.f, ax2 = 0.f, ay2 = 0.f;
  if (mine) {
    const float* a = cand_box(props, gt, n_p, i);
    ax1 = a[0]; ay1 = a[1]; ax2 = a[2]; ay2 = a[3];
  }
  const float area_a = (ax2 - ax1) * (ay2 - ay1);
  float best = -__builtin_inff();
  int arg = 0;
  for (int g0 = 0; g0 < G; g0 += 256) {
    const int g = g0 + threadIdx.x;
    if (g < G)
      for (int d = 0; d < 4; ++d) gb[threadIdx.x][d] = gt[4 * (long long)g + d];
    __syncthreads();
    if (mine) {
      const int m = min(256, G - g0);
      for (int t = 0; t < m; ++t) {
        const float w = fmaxf(fminf(ax2, gb[t][2]) - fmaxf(ax1, gb[t][0]), 0.f);
        const float h = fmaxf(fminf(ay2, gb[t][3]) - fmaxf(ay1, gb[t][1]), 0.f);
        const float inter = w * h;
        const float area_b = (gb[t][2] - gb[t][0]) * (gb[t][3] - gb[t][1]);
        const float iou = inter / ((area_a + area_b) - inter);
        if (iou > best) { best = iou; arg = g0 + t; }
      }
    }
    __syncthreads();
  }
  if (!mine) return;
  if (G == 0) {   // no ground truth: background, as assign_targets_to_proposals fills it
    matched[i] = 0; labels[i] = 0;
    if (max_iou) max_iou[i] = 0.f;
    return;
  }
  const bool hit = best >= high;
  matched[i] = hit ? arg : 0;                                  // Matcher's -1 / -2 clamped at 0
  labels[i] = hit ? gt_labels[arg] : (best < low ? 0 : -1);    // background / between the thresholds: ignored
  if (max_iou) max_iou[i] = best;
}

// ---- sample -----------------------------------------------------------------------------------------------------------
// order-preserving 32-bit image of a key, ascending: -0 -> +0, the usual sign fold, NaN above every number
__device__ __forceinline__ unsigned sample_key(float v) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// 1: positive (label >= 1), 0: negative (label 0), -1: ignored
__device__ __forceinline__ int sample_class(long long label) { return label >= 1 ? 1 : (label == 0 ? 0 : -1); }

// rank by counting, as det_rank_kernel: rank[i] = candidates of i's class whose (key, index) pair is smaller
__global__ __launch_bounds__(256) void roi_rank_kernel(const long long* __restrict__ labels, const float* __restrict__ keys,
                                                       int N, int* rank) {
  __shared__ unsigned long long sc[256];
  __shared__ int scl[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool mine = i < N;
  const int cls = mine ? sample_class(labels[i]) : -1;
  const unsigned long long comp = mine ? (((unsigned long long)sample_key(keys[i]) << 32) | (unsigned)i) : 0ull;
  int r = 0;
  for (int j0 = 0; j0 < N; j0 += 256) {
    const int j = j0 + threadIdx.x;
    scl[threadIdx.x] = j < N ? sample_class(labels[j]) : -2;
    sc[threadIdx.x] = j < N ? (((unsigned long long)sample_key(keys[j]) << 32) | (unsigned)j) : 0ull;
    __syncthreads();
    if (cls >= 0)
      for (int t = 0; t < 256; ++t) r += (scl[t] == cls && sc[t] < comp) ? 1 : 0;
    __syncthreads();
  }
  if (mine) rank[i] = cls >= 0 ? r : -1;
}

struct SampleArgs {
  const long long* labels;
  const int* matched;
  const int* rank;
  const float* props;
  const float* gt;
  int n_p, G, batch, quota;
  float wx, wy, ww, wh;
  int* counts;
  int* index;
  float* out_boxes;
  long long* out_labels;
  int* out_matched;
  float* targets;
  int* pos_slot;
};

// one workgroup: the two class counts, then the chosen candidates compacted in ascending index (a prefix scan per 1024
// candidates, positives in the high half of the scanned word), their gathers and regression targets
__global__ __launch_bounds__(1024) void roi_compact_kernel(SampleArgs a) {
  __shared__ int wsum[16];
  __shared__ int tot;
  const int N = a.n_p + a.G, tid = threadIdx.x;
  int c = 0;
  for (int i = tid; i < N; i += 1024) {
    const int cls = sample_class(a.labels[i]);
    c += cls == 1 ? (1 << 16) : (cls == 0 ? 1 : 0);
  }
  int ex = block_excl_scan_1024(c, wsum);
  if (tid == 1023) tot = ex + c;
  __syncthreads();
  const int n_pos = min(tot >> 16, a.quota), n_neg = min(tot & 0xffff, a.batch - n_pos);
  __syncthreads();
  int base = 0, pbase = 0;
  for (int c0 = 0; c0 < N; c0 += 1024) {
    const int i = c0 + tid;
    int cls = -1;
    bool sel = false;
    if (i < N) {
      cls = sample_class(a.labels[i]);
      const int r = a.rank[i];
      sel = (cls == 1 && r < n_pos) || (cls == 0 && r < n_neg);
    }
    const int v = sel ? (cls == 1 ? (1 << 16) | 1 : 1) : 0;
    ex = block_excl_scan_1024(v, wsum);
    if (tid == 1023) tot = ex + v;
    __syncthreads();
    const int slot = base + (ex & 0xffff);
    if (sel && slot < a.batch) {
      const float* b = cand_box(a.props, a.gt, a.n_p, i);
      const int m = a.matched[i];
      float zero[4] = {0.f, 0.f, 0.f, 0.f};   // no (or no such) ground truth: torchvision encodes a box of zeros
      const float* g = (m >= 0 && m < a.G) ? a.gt + 4 * (long long)m : zero;
      a.index[slot] = i;
      for (int d = 0; d < 4; ++d) a.out_boxes[4 * (long long)slot + d] = b[d];
      a.out_labels[slot] = a.labels[i];
      a.out_matched[slot] = m;
      box_encode_one(g, b, a.wx, a.wy, a.ww, a.wh, a.targets + 4 * (long long)slot);
      if (cls == 1) a.pos_slot[pbase + (ex >> 16)] = slot;
    }
    base += tot & 0xffff;
    pbase += tot >> 16;
    __syncthreads();
  }
  for (int s = base + tid; s < a.batch; s += 1024) a.index[s] = -1;
  if (tid == 0) { a.counts[0] = base; a.counts[1] = pbase; }
}

// ---- mask targets: thread = one element of targets[P][M][M] ---------------------------------------------------------------
// torchvision's roi_align with sampling_ratio <= 0 (the grid of a bin is ceil(roi extent / M) per axis), aligned = False,
// spatial_scale 1, on the one-channel image masks[matched[r]].  The geometry is fp32 with every operation rounded on its own,
// in the order of torchvision's kernel:  y = (y1 + ph bin) + ((iy + .5) bin) / grid.
// The grid comes from device data and has no bound, so a table of a whole axis (roialign.hip's RoiSample rows) has no
// fixed size: each thread computes the row parameters once per iy and the column parameters per sample.  Samples more
// than a pixel outside the mask add nothing and the samples of an axis are monotonic, so the loops run over the range
// that can touch the mask (found in double, two samples of slack; every sample is still tested): a garbage box of any
// size costs O(H W) steps per thread at the worst (O(H) rows times O(W) columns for the bin that covers the mask), never more.
// The column parameters are recomputed for every row sample (grid_h times redundant): a table of the bin's columns in
// LDS for bounded grids, with this loop as the fall-back, is the open step.
struct AxisRange { int lo, hi; };
__device__ __forceinline__ AxisRange axis_range(float base, float bin, int grid, int L) {
  const double step = (double)bin / (double)grid;
  const double lo = ceil((-1.0 - (double)base) / step - 0.5) - 2.0, hi = floor(((double)L - (double)base) / step - 0.5) + 2.0;
  AxisRange r;
  r.lo = lo > 0.0 ? (lo < (double)grid ? (int)lo : grid) : 0;          // NaN compares false: 0
  r.hi = hi < (double)(grid - 1) ? (hi >= 0.0 ? (int)hi : -1) : grid - 1;
  if (!(hi == hi)) r.hi = min(grid - 1, 1);
  return r;
}

// bilinear_interpolate's rules along one axis: false = outside (adds nothing)
__device__ __forceinline__ bool axis_sample(float y, int L, int* lo, int* hi, float* wlo, float* whi) {
  if (y < -1.f || y > (float)L) return false;
  if (y <= 0.f) y = 0.f;
  int l = (int)y, h;
  if (l >= L - 1) { h = l = L - 1; y = (float)l; } else { h = l + 1; }
  if (l < 0) l = h = 0;   // a NaN coordinate: stays inside the mask (the result is NaN)
  const float f = y - (float)l;
  *lo = l; *hi = h; *wlo = 1.f - f; *whi = f;
  return true;
}

template <class T>
__global__ __launch_bounds__(256) void mask_targets_kernel(const T* __restrict__ masks, int G, int H, int W,
                                                           const float* __restrict__ boxes,
                                                           const int* __restrict__ matched, int P, int M, float* out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)P * M * M) return;
  const int pw = (int)(idx % M), ph = (int)((idx / M) % M), r = (int)(idx / ((long long)M * M));
  const int m = matched[r];
  if (m < 0 || m >= G) {   // no such mask: nothing is read through it
    out[idx] = 0.f;
    return;
  }
  const T* img = masks + (long long)m * H * W;
  const float* b = boxes + 4 * (long long)r;
  const float x1 = b[0], y1 = b[1];
  const float roi_w = fmaxf(b[2] - x1, 1.f), roi_h = fmaxf(b[3] - y1, 1.f);
  const float bin_h = roi_h / (float)M, bin_w = roi_w / (float)M;
  // an infinite or huge bin: the cast stays defined (2147483520 = the largest float below 2^31)
  const int gh = (int)fminf(ceilf(bin_h), 2147483520.f), gw = (int)fminf(ceilf(bin_w), 2147483520.f);
  const float by = y1 + (float)ph * bin_h, bx = x1 + (float)pw * bin_w;
  const AxisRange ry = axis_range(by, bin_h, gh, H), rx = axis_range(bx, bin_w, gw, W);
  float sum = 0.f;
  for (int iy = ry.lo; iy <= ry.hi; ++iy) {
    const float y = by + (((float)iy + .5f) * bin_h) / (float)gh;
    int ylo, yhi;
    float hy, ly;
    if (!axis_sample(y, H, &ylo, &yhi, &hy, &ly)) continue;
    const T* row_lo = img + (long long)ylo * W;
    const T* row_hi = img + (long long)yhi * W;
    for (int ix = rx.lo; ix <= rx.hi; ++ix) {
      const float x = bx + (((float)ix + .5f) * bin_w) / (float)gw;
      int xlo, xhi;
      float hx, lx;
      if (!axis_sample(x, W, &xlo, &xhi, &hx, &lx)) continue;
      sum += hy * hx * (float)row_lo[xlo] + hy * lx * (float)row_lo[xhi] + ly * hx * (float)row_hi[xlo] +
             ly * lx * (float)row_hi[xhi];
    }
  }
  out[idx] = sum / fmaxf((float)gh * (float)gw, 1.f);
}

static size_t sample_ws_bytes(int N) { return (((size_t)(N > 0 ? N : 1) * 4) + 15) & ~(size_t)15; }

// the candidate-list checks of roi_match and roi_sample
static int check_candidates(const char* what, int n_p, int G, const void* props, const void* gt) {
  SFVOS_REQUIRE(n_p >= 0 && G >= 0, "%s: negative count (%d proposals, %d ground-truth boxes)", what, n_p, G);
  SFVOS_REQUIRE(G <= RT_MAX_G, "%s: %d ground-truth boxes, at most %d", what, G, RT_MAX_G);
  SFVOS_REQUIRE(n_p <= RT_MAX_N && n_p + G <= RT_MAX_N, "%s: %d + %d candidates, at most %d", what, n_p, G, RT_MAX_N);
  SFVOS_REQUIRE((n_p == 0 || props) && (G == 0 || gt), "%s: null box pointer", what);
  return SFVOS_OK;
}

}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_roi_match(const float* proposals, int n_p, const float* gt_boxes, const int64_t* gt_labels, int G,
                               float high, float low, int* matched, int64_t* labels, float* max_iou,
                               sfvos_stream_t stream) {
  if (int rc = check_candidates("roi_match", n_p, G, proposals, gt_boxes)) return rc;
  SFVOS_REQUIRE((G == 0 || gt_labels) && matched && labels, "roi_match: null pointer");
  const int N = n_p + G;
  if (N == 0) return SFVOS_OK;
  hipLaunchKernelGGL(roi_match_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, proposals,
                     gt_boxes, (const long long*)gt_labels, n_p, G, high, low, matched, (long long*)labels, max_iou);
  return check_launch("roi_match");
}

extern "C" size_t sfvos_roi_sample_workspace_bytes(int n) { return n >= 0 && n <= RT_MAX_N ? sample_ws_bytes(n) : 0; }

extern "C" int sfvos_roi_sample(const int64_t* labels, const int* matched, const float* keys, const float* proposals,
                                int n_p, const float* gt_boxes, int G, int batch_size_per_image,
                                double positive_fraction, float wx, float wy, float ww, float wh, void* workspace,
                                int* counts, int* index, float* out_boxes, int64_t* out_labels, int* out_matched,
                                float* regression_targets, int* pos_slot, sfvos_stream_t stream) {
  if (int rc = check_candidates("roi_sample", n_p, G, proposals, gt_boxes)) return rc;
  SFVOS_REQUIRE(batch_size_per_image >= 1 && batch_size_per_image <= RT_MAX_BATCH,
                "roi_sample: batch_size_per_image %d out of [1, %d]", batch_size_per_image, RT_MAX_BATCH);
  SFVOS_REQUIRE(positive_fraction >= 0.0 && positive_fraction <= 1.0, "roi_sample: positive_fraction %g out of [0, 1]",
                positive_fraction);
  SFVOS_REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "roi_sample: weights must be positive");
  const int N = n_p + G;
  SFVOS_REQUIRE((N == 0 || (labels && matched && keys)) && workspace && counts && index && out_boxes && out_labels &&
                    out_matched && regression_targets && pos_slot,
                "roi_sample: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (N > 0)
    hipLaunchKernelGGL(roi_rank_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, (const long long*)labels,
                       keys, N, (int*)workspace);
  SampleArgs a;
  a.labels = (const long long*)labels; a.matched = matched; a.rank = (const int*)workspace;
  a.props = proposals; a.gt = gt_boxes; a.n_p = n_p; a.G = G; a.batch = batch_size_per_image;
  a.quota = (int)((double)batch_size_per_image * positive_fraction);   // torchvision: int(batch * fraction), doubles
  a.wx = wx; a.wy = wy; a.ww = ww; a.wh = wh;
  a.counts = counts; a.index = index; a.out_boxes = out_boxes; a.out_labels = (long long*)out_labels;
  a.out_matched = out_matched; a.targets = regression_targets; a.pos_slot = pos_slot;
  hipLaunchKernelGGL(roi_compact_kernel, dim3(1), dim3(1024), 0, st, a);
  return check_launch("roi_sample");
}

extern "C" int sfvos_mask_targets(const void* masks, int masks_are_u8, int G, int H, int W, const float* boxes,
                                  const int* matched, int P, int M, float* targets, sfvos_stream_t stream) {
  SFVOS_REQUIRE(M >= 1 && M <= RT_MAX_M, "mask_targets: M %d out of [1, %d]", M, RT_MAX_M);
  SFVOS_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "mask_targets: bad mask extent %dx%d", H, W);
  SFVOS_REQUIRE(G >= 0 && P >= 0 && P <= (1 << 20), "mask_targets: bad count (%d masks, %d boxes)", G, P);
  if (P == 0) return SFVOS_OK;
  SFVOS_REQUIRE((G == 0 || masks) && boxes && matched && targets, "mask_targets: null pointer");
  const dim3 grid((unsigned)ceil_div64((long long)P * M * M, 256));
  if (masks_are_u8)
    hipLaunchKernelGGL(mask_targets_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)masks, G, H, W, boxes, matched, P, M, targets);
  else
    hipLaunchKernelGGL(mask_targets_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)masks, G, H, W,
                       boxes, matched, P, M, targets);
  return check_launch("mask_targets");
}
