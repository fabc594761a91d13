// rpn_targets.hip -- the training call of the region proposal network (model.py:236-240 with targets, :329-335; its two
// losses enter total_loss at :361-368), restated from torchvision's published sources (models/detection/rpn.py:
// assign_targets_to_anchors, compute_loss; _utils.py: Matcher with allow_low_quality_matches, set_low_quality_matches_,
// BalancedPositiveNegativeSampler, BoxCoder(1, 1, 1, 1).encode; ops/boxes.py: box_iou) -- parity unpinned by the
// reference, torchvision is neither vendored nor installed.  The RPN is frozen and the call runs under no_grad: no backward.
//
//   anchors against the ground truth: IoU matcher, low-quality rule, labels        sfvos_rpn_match    (one image per call)
//   balanced sampler over explicit keys, regression targets of the positives      sfvos_rpn_sample   (one image per call)
//   BCE-with-logits and smooth-L1 over the sampled anchors of all images          sfvos_rpn_loss
//
// Anchor n of an image is n = A (sum_{l' < l} H_l' W_l' + h W_l + w) + a, torchvision's per-image concatenation (level, h,
// w, a); its box is base_anchors[l][a] + (w stride_w, h stride_h, w stride_w, h stride_h) as rpn_decode_kernel forms it.
// No anchor array is ever in memory.  Objectness and deltas stay in the pyramid's level-major storage.
//
// Integer atomics only (a maximum of bit patterns, histogram bins, a slot counter), on words a launch of the call zeroes.  A maximum and a histogram do not
// depend on the order; what the slot counter ordered is re-ranked by counting: every result is bit-identical from run to
// run.  One launch per pass; no grid-wide barrier, no persistent workgroup, no spin-wait.
#include "elt_util.h"

// The IoU decides something and is restated operation by operation in tests/rpn_loss_ref.py: every fp32 operation is
// rounded on its own (see roi_targets.hip on why this is the pragma and not the _rn intrinsics).
#pragma clang fp contract(off)

namespace sfvos {

constexpr int RT_A = 8;                 // anchors per position
constexpr int RT_G = 1024;              // ground-truth boxes of one image
constexpr int RT_BATCH = 4096;          // batch_size_per_image
constexpr int RT_N = 1 << 24;           // anchors of one image (exclusive): the index fills 24 bits of the sort word
constexpr int RT_TILE = 64;             // ground-truth boxes of one LDS tile of the match
constexpr int RT_BINS = 4096;           // bins of the widest digit
constexpr int RT_PASSES = 5;            // digits of the 56-bit (key, index) word: 12 + 11 + 11 + 11 + 11 bits

struct AnchorGrid {
  int n_levels, A, N;
  int W[SFVOS_MAX_LEVELS], HW[SFVOS_MAX_LEVELS];
  int stride_h[SFVOS_MAX_LEVELS], stride_w[SFVOS_MAX_LEVELS];
  int before[SFVOS_MAX_LEVELS];   // positions of one image in front of level l
};

// anchor n -> (level, position in the level, anchor of the position)
__device__ __forceinline__ void anchor_locate(const AnchorGrid& g, int n, int* l, int* p, int* a) {
  int lv = 0;
  while (lv + 1 < g.n_levels && n >= g.A * g.before[lv + 1]) ++lv;
  const int r = n - g.A * g.before[lv];
  *l = lv; *p = r / g.A; *a = r - (r / g.A) * g.A;
}

__device__ __forceinline__ void anchor_box(const AnchorGrid& g, const float* __restrict__ base, int n, float* box) {
  int l, p, a;
  anchor_locate(g, n, &l, &p, &a);
  const int h = p / g.W[l], w = p - h * g.W[l];
  const float* ba = base + ((long long)l * g.A + a) * 4;
  const float sx = (float)(w * g.stride_w[l]), sy = (float)(h * g.stride_h[l]);
  box[0] = ba[0] + sx; box[1] = ba[1] + sy; box[2] = ba[2] + sx; box[3] = ba[3] + sy;
}

// order-preserving 32-bit image of a float, ascending: -0 -> +0, the usual sign fold; a NaN maps to `nan`
__device__ __forceinline__ unsigned float_key(float v, unsigned nan) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return nan;
  if (u == 0x80000000u) u = 0u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// the words the atomics of a call add to or take a maximum over, zeroed by a launch of its own in front of them (a plain
// kernel: the chain stays a sequence of kernel launches on the caller's stream, in a captured graph too)
__global__ __launch_bounds__(256) void rpn_zero_kernel(unsigned* __restrict__ words, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) words[i] = 0u;
}

// ---- match: thread = anchor, the ground truth walks through LDS in tiles ---------------------------------------------------
// IoU as roi_match_kernel / det_iou_kernel compute it: inter / ((area_a + area_b) - inter).
__device__ __forceinline__ float iou_one(float ax1, float ay1, float ax2, float ay2, float area_a, const float* b) {
  const float w = fmaxf(fminf(ax2, b[2]) - fmaxf(ax1, b[0]), 0.f);
  const float h = fmaxf(fminf(ay2, b[3]) - fmaxf(ay1, b[1]), 0.f);
  const float inter = w * h;
  const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / ((area_a + area_b) - inter);
}

// pass 0: the largest IoU of every anchor (the lower ground-truth index on a tie, a NaN never wins), matched / labels /
//         max_iou by the two thresholds; with `highest`: highest[g] = max over the anchors of float_key(IoU(g, n)), first
//         per workgroup in LDS, then across workgroups (0 = no number seen).
// pass 1: set_low_quality_matches_ -- the same IoUs from the same device function, so the test is an exact comparison:
//         an anchor whose IoU with some g equals highest[g] gets label 1 and its own argmax as match.
__global__ __launch_bounds__(256) void rpn_match_kernel(AnchorGrid g, const float* __restrict__ base,
                                                        const float* __restrict__ gt, int G, float high, float low,
                                                        int pass, unsigned* highest, int* matched, int* labels,
                                                        float* max_iou) {
  __shared__ float gb[RT_TILE][4];
  __shared__ unsigned hi[RT_TILE];
  const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
  const bool mine = i < g.N;
  if (G == 0) {   // no ground truth: every anchor is background, as assign_targets_to_anchors fills it
    if (mine) {
      matched[i] = 0; labels[i] = 0;
      if (max_iou) max_iou[i] = 0.f;
    }
    return;
  }
  float ab[4] = {0.f, 0.f, 0.f, 0.f};
  if (mine) anchor_box(g, base, i, ab);
  const float area_a = (ab[2] - ab[0]) * (ab[3] - ab[1]);
  float best = -__builtin_inff();
  int arg = 0;
  bool low_quality = false;
  for (int g0 = 0; g0 < G; g0 += RT_TILE) {
    const int gi = g0 + tid;
    const bool loader = tid < RT_TILE && gi < G;   // the first wave owns slot tid of the tile
    if (loader) {
      for (int d = 0; d < 4; ++d) gb[tid][d] = gt[4 * (long long)gi + d];
      hi[tid] = pass == 1 ? highest[gi] : 0u;
    }
    __syncthreads();
    if (mine) {
      const int m = min(RT_TILE, G - g0);
      for (int t = 0; t < m; ++t) {
        const float iou = iou_one(ab[0], ab[1], ab[2], ab[3], area_a, gb[t]);
        if (iou > best) { best = iou; arg = g0 + t; }
        const unsigned k = float_key(iou, 0u);
        if (pass == 1) {
          low_quality |= k != 0u && k == hi[t];
        } else if (highest && k > ((volatile unsigned*)hi)[t]) {
          atomicMax(&hi[t], k);
        }
      }
    }
    __syncthreads();
    // slot tid is read here and rewritten above by the same thread; nobody else touches the tile before the next barrier
    if (pass == 0 && highest && loader && hi[tid] != 0u) atomicMax(&highest[gi], hi[tid]);
  }
  if (!mine) return;
  if (pass == 1) {
    if (low_quality) { matched[i] = arg; labels[i] = 1; }
    return;
  }
  const bool hit = best >= high;
  matched[i] = hit ? arg : 0;                     // Matcher's -1 / -2 clamped at 0
  labels[i] = hit ? 1 : (best < low ? 0 : -1);    // background / between the thresholds: ignored
  if (max_iou) max_iou[i] = best;
}

// ---- sample: radix select of the n smallest (key, index) words of each class over several workgroups ----------------------
// word = float_key(key) << 24 | index (56 bits, all distinct: no ties to order); class 1 = label >= 1, class 0 = label 0.
// Launch p = 0 .. 4 adds the histogram of digit p of the words that share the prefix found so far (per workgroup in LDS,
// merged into the workspace with integer atomics); every workgroup of launch p >= 1 first derives that prefix from the
// finished histogram of launch p - 1, workgroup 0 stores it for the next launch.  The totals of histogram 0 are the class
// counts, from which n_pos and n_neg follow.  Launch 5 derives the n-th smallest word of each class and appends every
// word up to it to a list (slot counter); launch 6, one workgroup, ranks the list by counting and writes the outputs.
struct SelWs {
  int* hist;                    // [RT_PASSES][2][RT_BINS]
  unsigned long long* prefix;   // [RT_PASSES + 1][2]: the bits fixed in front of pass p
  int* krem;                    // [RT_PASSES + 1][2]: words still to take inside that prefix (0: the class takes none)
  int* n;                       // [2]: n_neg, n_pos
  int* slot;                    // [1]
  int* list;                    // [batch_size_per_image]: (class 1 ? 0 : 1) << 24 | index
};
constexpr size_t RT_HIGHEST_BYTES = (size_t)RT_G * 4;
constexpr size_t RT_HIST_BYTES = (size_t)RT_PASSES * 2 * RT_BINS * 4;
constexpr size_t RT_STATE_BYTES = 256;   // prefix 96, krem 48, n 8, slot 4
static inline size_t sel_ws_layout(int batch, void* base, unsigned** highest, SelWs* w) {
  char* p = (char*)base;
  if (highest) *highest = (unsigned*)p;
  size_t o = RT_HIGHEST_BYTES;
  if (w) {
    w->hist = (int*)(p + o);
    w->prefix = (unsigned long long*)(p + o + RT_HIST_BYTES);
    w->krem = (int*)(p + o + RT_HIST_BYTES + 96);
    w->n = (int*)(p + o + RT_HIST_BYTES + 144);
    w->slot = (int*)(p + o + RT_HIST_BYTES + 152);
    w->list = (int*)(p + o + RT_HIST_BYTES + RT_STATE_BYTES);
  }
  o += RT_HIST_BYTES + RT_STATE_BYTES;
  o += (((size_t)batch * 4) + 15) & ~(size_t)15;
  return o;
}

__device__ __forceinline__ int digit_shift(int p) { return 44 - 11 * p; }
__device__ __forceinline__ int digit_bins(int p) { return p == 0 ? 4096 : 2048; }
__device__ __forceinline__ int sample_class(int label) { return label >= 1 ? 1 : (label == 0 ? 0 : -1); }
__device__ __forceinline__ unsigned long long sample_word(float key, int i) {
  return ((unsigned long long)float_key(key, 0xffffffffu) << 24) | (unsigned)i;   // a NaN key: behind every number
}

// State in front of pass p >= 1 (p = RT_PASSES: the complete word) from histogram p - 1, by every thread of a 1024-thread
// workgroup: s_pref[c], s_k[c].  Thread t owns the bins per t .. per t + per - 1; the thread whose bins hold the k-th word
// finds its bin.  k of pass 1 comes from the class totals (s_n), later from the stored state.
__device__ __forceinline__ void sel_advance(const SelWs& ws, int p, int batch, int quota, int* wsum,
                                            unsigned long long* s_pref, int* s_k, int* s_n, bool store) {
  const int tid = threadIdx.x, q0 = p - 1, nb = digit_bins(q0), per = nb >> 10, shift = digit_shift(q0);
  for (int c = 1; c >= 0; --c) {
    const int* h = ws.hist + ((long long)q0 * 2 + c) * RT_BINS;
    int cnt = 0;
    for (int q = 0; q < per; ++q) cnt += h[per * tid + q];
    int E = block_excl_scan_1024(cnt, wsum);
    if (tid == 1023) s_n[2 + c] = E + cnt;   // the class total
    __syncthreads();
    int k;
    if (p == 1) k = c == 1 ? min(s_n[3], quota) : min(s_n[2], batch - s_n[1]);
    else k = ws.krem[q0 * 2 + c];
    const unsigned long long prev = p == 1 ? 0ull : ws.prefix[q0 * 2 + c];
    if (k >= 1 && E < k && k <= E + cnt) {   // exactly one thread
      for (int q = 0; q < per; ++q) {
        const int bin = per * tid + q, hc = h[bin];
        if (k <= E + hc) {
          s_pref[c] = prev | ((unsigned long long)bin << shift);
          s_k[c] = k - E;
          break;
        }
        E += hc;
      }
    }
    if (tid == 0) {
      if (k < 1) { s_pref[c] = 0ull; s_k[c] = 0; }
      if (p == 1) s_n[c] = k;
    }
    __syncthreads();
  }
  if (store && tid == 0) {
    for (int c = 0; c < 2; ++c) {
      ws.prefix[p * 2 + c] = s_pref[c];
      ws.krem[p * 2 + c] = s_k[c];
      if (p == 1) ws.n[c] = s_n[c];
    }
  }
}

__global__ __launch_bounds__(1024) void rpn_sample_hist_kernel(const int* __restrict__ labels,
                                                               const float* __restrict__ keys, int N, int p, int batch,
                                                               int quota, SelWs ws) {
  __shared__ int lh[2][RT_BINS];
  __shared__ int wsum[16];
  __shared__ unsigned long long s_pref[2];
  __shared__ int s_k[2], s_n[4];
  const int tid = threadIdx.x, nb = digit_bins(p), shift = digit_shift(p);
  for (int b = tid; b < 2 * RT_BINS; b += 1024) (&lh[0][0])[b] = 0;
  if (p >= 1) sel_advance(ws, p, batch, quota, wsum, s_pref, s_k, s_n, blockIdx.x == 0);
  __syncthreads();
  const unsigned long long above = p == 0 ? 0ull : ~((1ull << digit_shift(p - 1)) - 1ull);
  for (long long i = (long long)blockIdx.x * 1024 + tid; i < N; i += (long long)gridDim.x * 1024) {
    const int c = sample_class(labels[i]);
    if (c < 0 || (p >= 1 && s_k[c] == 0)) continue;
    const unsigned long long w = sample_word(keys[i], (int)i);
    if (p >= 1 && (w & above) != s_pref[c]) continue;
    atomicAdd(&lh[c][(int)(w >> shift) & (nb - 1)], 1);
  }
  __syncthreads();
  int* h = ws.hist + (long long)p * 2 * RT_BINS;
  for (int b = tid; b < 2 * RT_BINS; b += 1024) {
    const int v = (&lh[0][0])[b];
    if (v) atomicAdd(&h[b], v);
  }
}

__global__ __launch_bounds__(1024) void rpn_sample_gather_kernel(const int* __restrict__ labels,
                                                                 const float* __restrict__ keys, int N, int batch,
                                                                 int quota, SelWs ws) {
  __shared__ int wsum[16];
  __shared__ unsigned long long s_pref[2];
  __shared__ int s_k[2], s_n[4];
  sel_advance(ws, RT_PASSES, batch, quota, wsum, s_pref, s_k, s_n, false);
  for (long long i = (long long)blockIdx.x * 1024 + threadIdx.x; i < N; i += (long long)gridDim.x * 1024) {
    const int c = sample_class(labels[i]);
    if (c < 0 || s_k[c] == 0) continue;
    if (sample_word(keys[i], (int)i) > s_pref[c]) continue;   // s_pref: the n-th smallest word of the class
    const int s = atomicAdd(ws.slot, 1);
    if (s < batch) ws.list[s] = ((c == 1 ? 0 : 1) << 24) | (int)i;
  }
}

// one workgroup: the list (at most batch_size_per_image entries, in the order the slot counter gave) ranked by counting --
// positives in ascending anchor index, then the negatives in ascending anchor index, torchvision's cat([pos, neg]) -- and
// the regression targets of the positives: BoxCoder(1, 1, 1, 1).encode of gt_boxes[matched] against the anchor.
__global__ __launch_bounds__(1024) void rpn_sample_emit_kernel(AnchorGrid g, const float* __restrict__ base,
                                                               const int* __restrict__ matched,
                                                               const float* __restrict__ gt, int G, int batch, SelWs ws,
                                                               int* counts, int* index, float* targets) {
  __shared__ int e[RT_BATCH];
  const int tid = threadIdx.x;
  const int n_pos = min(max(ws.n[1], 0), batch);
  const int n_all = min(max(min(min(max(ws.n[0], 0), batch) + n_pos, *ws.slot), 0), batch);   // never outside [0, batch]
  for (int s = tid; s < n_all; s += 1024) e[s] = ws.list[s];
  __syncthreads();
  for (int s = tid; s < n_all; s += 1024) {
    const int mine = e[s];
    int r = 0;
    for (int j = 0; j < n_all; ++j) r += e[j] < mine;
    const int i = mine & 0xffffff;
    index[r] = i;
    if (r < n_pos) {
      float ab[4];
      anchor_box(g, base, i, ab);
      const int m = matched[i];
      float zero[4] = {0.f, 0.f, 0.f, 0.f};   // no such ground truth: torchvision encodes a box of zeros
      box_encode_one((m >= 0 && m < G) ? gt + 4 * (long long)m : zero, ab, 1.f, 1.f, 1.f, 1.f,
                     targets + 4 * (long long)r);
    }
  }
  for (int s = n_all + tid; s < batch; s += 1024) index[s] = -1;
  if (tid == 0) { counts[0] = n_all; counts[1] = min(n_pos, n_all); }
}

// ---- loss: one workgroup, f64 sums in a fixed order ------------------------------------------------------------------------
// row (b, r), r < S_b: x = the objectness logit of anchor index[b][r] of image b, z = r < P_b;
//   bce = max(x, 0) - x z + log1p(exp(-|x|));   for r < P_b: box = sum_d smooth_l1(delta_d - target_d; beta)
// out[0] = sum bce / S_tot, out[1] = sum box / S_tot, S_tot = sum_b S_b (0 / 0 when nothing was sampled, as torch).
__global__ __launch_bounds__(1024) void rpn_loss_kernel(const float* __restrict__ obj, const float* __restrict__ deltas,
                                                        AnchorGrid g, int batch, const int* __restrict__ index,
                                                        const int* __restrict__ counts,
                                                        const float* __restrict__ targets, int bspi, float beta,
                                                        float* per_sample, float* out) {
  __shared__ double red[2][1024];
  double sc = 0.0, sb = 0.0;
  const int rows = batch * bspi;
  for (int row = threadIdx.x; row < rows; row += 1024) {
    const int b = row / bspi, r = row - b * bspi;
    const int S = min(max(counts[2 * b], 0), bspi), P = min(max(counts[2 * b + 1], 0), S);
    if (r >= S) continue;
    const int n = index[row];
    float bce = __builtin_nanf(""), box = r < P ? __builtin_nanf("") : 0.f;
    if (n >= 0 && n < g.N) {   // anything else: NaN, nothing is read through it
      int l, p, a;
      anchor_locate(g, n, &l, &p, &a);
      const long long at = (((long long)batch * g.before[l] + (long long)b * g.HW[l] + p) * g.A + a);
      const float x = obj[at], z = r < P ? 1.f : 0.f;
      bce = fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
      if (r < P) {
        box = 0.f;
        for (int d = 0; d < 4; ++d) box += smooth_l1(deltas[4 * at + d] - targets[4 * (long long)row + d], beta);
      }
    }
    if (per_sample) { per_sample[2 * (long long)row] = bce; per_sample[2 * (long long)row + 1] = box; }
    sc += (double)bce;
    sb += (double)box;
  }
  sc = block_sum_1024(red[0], sc);
  sb = block_sum_1024(red[1], sb);
  if (threadIdx.x == 0) {
    long long s_tot = 0;
    for (int b = 0; b < batch; ++b) s_tot += min(max(counts[2 * b], 0), bspi);
    out[0] = (float)(sc / (double)s_tot);
    out[1] = (float)(sb / (double)s_tot);
  }
}

// the anchor grid of a call and the checks the three entry points share
static int make_grid(const char* what, const sfvos_pyramid* pyr, int A, int tensor_h, int tensor_w, AnchorGrid* g) {
  SFVOS_REQUIRE(pyr != nullptr, "%s: null pyramid", what);
  SFVOS_REQUIRE(pyr->n_levels >= 1 && pyr->n_levels <= SFVOS_MAX_LEVELS, "%s: n_levels %d out of [1, %d]", what,
                pyr->n_levels, SFVOS_MAX_LEVELS);
  SFVOS_REQUIRE(A >= 1 && A <= RT_A, "%s: num_anchors %d out of [1, %d]", what, A, RT_A);
  SFVOS_REQUIRE(tensor_h >= 1 && tensor_w >= 1, "%s: bad tensor size %dx%d", what, tensor_h, tensor_w);
  g->n_levels = pyr->n_levels; g->A = A;
  long long px = 0;
  for (int l = 0; l < SFVOS_MAX_LEVELS; ++l) {
    const bool live = l < pyr->n_levels;
    const int H = live ? pyr->h[l] : 1, W = live ? pyr->w[l] : 1;
    SFVOS_REQUIRE(H >= 1 && W >= 1 && (long long)H * W * A < RT_N, "%s: level %d has bad extent %dx%d", what, l, H, W);
    g->W[l] = W; g->HW[l] = H * W;
    g->stride_h[l] = tensor_h / H; g->stride_w[l] = tensor_w / W;
    g->before[l] = (int)px;
    if (live) px += (long long)H * W;
    SFVOS_REQUIRE(px * A < RT_N, "%s: %lld anchors per image, fewer than 2^24 are implemented", what, px * A);
  }
  g->N = (int)(px * A);
  return SFVOS_OK;
}

static int check_counts(const char* what, int G, int batch_size_per_image) {
  SFVOS_REQUIRE(G >= 0 && G <= RT_G, "%s: %d ground-truth boxes out of [0, %d]", what, G, RT_G);
  SFVOS_REQUIRE(batch_size_per_image >= 1 && batch_size_per_image <= RT_BATCH,
                "%s: batch_size_per_image %d out of [1, %d]", what, batch_size_per_image, RT_BATCH);
  return SFVOS_OK;
}

}  // namespace sfvos

using namespace sfvos;

extern "C" size_t sfvos_rpn_targets_workspace_bytes(const sfvos_pyramid* pyr, int num_anchors, int G,
                                                    int batch_size_per_image) {
  AnchorGrid g;
  if (make_grid("rpn_targets_workspace_bytes", pyr, num_anchors, 1, 1, &g) ||
      check_counts("rpn_targets_workspace_bytes", G, batch_size_per_image))
    return 0;
  return sel_ws_layout(batch_size_per_image, nullptr, nullptr, nullptr);
}

extern "C" int sfvos_rpn_match(const sfvos_pyramid* pyr, int num_anchors, const float* base_anchors, int tensor_h,
                               int tensor_w, const float* gt_boxes, int G, float high, float low, int allow_low_quality,
                               void* workspace, int* matched, int* labels, float* max_iou, sfvos_stream_t stream) {
  AnchorGrid g;
  if (int rc = make_grid("rpn_match", pyr, num_anchors, tensor_h, tensor_w, &g)) return rc;
  if (int rc = check_counts("rpn_match", G, 1)) return rc;
  SFVOS_REQUIRE(high >= 0.f && high <= 1.f && low >= 0.f && low <= 1.f, "rpn_match: thresholds %g, %g out of [0, 1]",
                (double)high, (double)low);
  SFVOS_REQUIRE(base_anchors && (G == 0 || gt_boxes) && workspace && matched && labels, "rpn_match: null pointer");
  hipStream_t st = (hipStream_t)stream;
  unsigned* highest = nullptr;
  sel_ws_layout(1, workspace, &highest, nullptr);
  const bool lowq = allow_low_quality != 0 && G > 0;
  if (lowq) hipLaunchKernelGGL(rpn_zero_kernel, dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, st, highest, G);
  const dim3 grid((unsigned)ceil_div(g.N, 256));
  hipLaunchKernelGGL(rpn_match_kernel, grid, dim3(256), 0, st, g, base_anchors, gt_boxes, G, high, low, 0,
                     lowq ? highest : nullptr, matched, labels, max_iou);
  if (lowq)
    hipLaunchKernelGGL(rpn_match_kernel, grid, dim3(256), 0, st, g, base_anchors, gt_boxes, G, high, low, 1, highest,
                       matched, labels, max_iou);
  return check_launch("rpn_match");
}

extern "C" int sfvos_rpn_sample(const int* labels, const int* matched, const float* keys, int N,
                                const sfvos_pyramid* pyr, int num_anchors, const float* base_anchors, int tensor_h,
                                int tensor_w, const float* gt_boxes, int G, int batch_size_per_image,
                                double positive_fraction, void* workspace, int* counts, int* index,
                                float* regression_targets, sfvos_stream_t stream) {
  AnchorGrid g;
  if (int rc = make_grid("rpn_sample", pyr, num_anchors, tensor_h, tensor_w, &g)) return rc;
  if (int rc = check_counts("rpn_sample", G, batch_size_per_image)) return rc;
  SFVOS_REQUIRE(N == g.N, "rpn_sample: %d labels, the pyramid has %d anchors per image", N, g.N);
  SFVOS_REQUIRE(positive_fraction >= 0.0 && positive_fraction <= 1.0, "rpn_sample: positive_fraction %g out of [0, 1]",
                positive_fraction);
  SFVOS_REQUIRE(labels && matched && keys && base_anchors && (G == 0 || gt_boxes) && workspace && counts && index &&
                    regression_targets,
                "rpn_sample: null pointer");
  hipStream_t st = (hipStream_t)stream;
  SelWs ws;
  sel_ws_layout(batch_size_per_image, workspace, nullptr, &ws);
  const int zero_words = (int)((RT_HIST_BYTES + RT_STATE_BYTES) / 4);   // histograms, state, counts, slot counter
  hipLaunchKernelGGL(rpn_zero_kernel, dim3((unsigned)ceil_div(zero_words, 256)), dim3(256), 0, st, (unsigned*)ws.hist,
                     zero_words);
  const int quota = (int)((double)batch_size_per_image * positive_fraction);   // torchvision: int(batch * fraction)
  const int wgs = ceil_div(N, 4096);
  const dim3 grid((unsigned)(wgs < 256 ? wgs : 256));
  for (int p = 0; p < RT_PASSES; ++p)
    hipLaunchKernelGGL(rpn_sample_hist_kernel, grid, dim3(1024), 0, st, labels, keys, N, p, batch_size_per_image, quota,
                       ws);
  hipLaunchKernelGGL(rpn_sample_gather_kernel, grid, dim3(1024), 0, st, labels, keys, N, batch_size_per_image, quota, ws);
  hipLaunchKernelGGL(rpn_sample_emit_kernel, dim3(1), dim3(1024), 0, st, g, base_anchors, matched, gt_boxes, G,
                     batch_size_per_image, ws, counts, index, regression_targets);
  return check_launch("rpn_sample");
}

extern "C" int sfvos_rpn_loss(const float* objectness, const float* deltas, const sfvos_pyramid* pyr, int batch,
                              int num_anchors, const int* index, const int* counts, const float* regression_targets,
                              int batch_size_per_image, float beta, float* per_sample, float* out,
                              sfvos_stream_t stream) {
  AnchorGrid g;
  if (int rc = make_grid("rpn_loss", pyr, num_anchors, 1, 1, &g)) return rc;
  if (int rc = check_counts("rpn_loss", 0, batch_size_per_image)) return rc;
  SFVOS_REQUIRE(batch >= 1 && batch <= 4096, "rpn_loss: batch %d out of [1, 4096]", batch);
  SFVOS_REQUIRE(beta >= 0.f, "rpn_loss: beta %g must not be negative", (double)beta);
  SFVOS_REQUIRE(objectness && deltas && index && counts && regression_targets && out, "rpn_loss: null pointer");
  hipLaunchKernelGGL(rpn_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, objectness, deltas, g, batch, index,
                     counts, regression_targets, batch_size_per_image, beta, per_sample, out);
  return check_launch("rpn_loss");
}
