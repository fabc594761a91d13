// rpn.hip -- the proposal filter of the region proposal network (model.py:236-240), restated from torchvision's published
// sources (models/detection/rpn.py: RegionProposalNetwork.filter_proposals; anchor_utils.py: AnchorGenerator; _utils.py:
// BoxCoder(1, 1, 1, 1); ops/boxes.py: clip_boxes_to_image, remove_small_boxes, batched_nms) -- parity unpinned by the
// reference, torchvision is neither vendored nor installed.  The head in front of it is sfvos_conv3d (3x3 + ReLU over the
// whole pyramid) and sfvos_box_predictor (the two 1x1 heads), which leave objectness [positions][A] and deltas
// [positions][4A] in the pyramid's level-major order: segment (level l, image b) is contiguous.
//
//   per-segment top k by objectness logit, ranked                       sfvos_rpn_select
//   anchors from (index, base table, strides), decode, clip, filter     sfvos_rpn_decode
//   per-segment greedy NMS (blocked scan), merge, the first post_nms    sfvos_rpn_nms
//
// The order everywhere: logit descending, ties by (level, anchor index) ascending; values compare as floats (-0 == +0,
// +-inf ordinary) and NaN ranks below every number.  Integer atomics only (LDS histogram and slot counters); what they
// order is re-ranked by counting, so every result is bit-identical from run to run.  One launch per stage covers all
// (level, image) segments.
#include "elt_util.h"

namespace sfvos {

constexpr int RPN_MAX_K = 4096;   // pre_nms_top_n per level: the ranking keeps k (key, index) pairs in 32 KB of LDS
constexpr int RPN_MAX_A = 8;      // anchors per position (sfvos_box_predictor's class limit)

// segments s = l * batch + b of one call
struct RpnSegs {
  int n_levels, batch, A, k;
  int H[SFVOS_MAX_LEVELS], W[SFVOS_MAX_LEVELS];
  int stride_h[SFVOS_MAX_LEVELS], stride_w[SFVOS_MAX_LEVELS];
  long long pos0[SFVOS_MAX_LEVELS];   // first position of the level: batch * sum_{l' < l} H W
};

// order-preserving 32-bit key of a logit: NaN -> 0 (below everything), -0 -> +0, then the usual sign fold
__device__ __forceinline__ unsigned rpn_key(float v) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// ---- select: one workgroup per segment -----------------------------------------------------------------------------------
// Radix select of the K-th largest key (K = min(k, n)) in three passes of 11 + 11 + 10 bits, each a histogram of the keys
// that share the prefix found so far; then one pass that copies the keys above the K-th and the lowest-index ties of it
// into LDS, and a ranking of those K by counting (K^2 compares of (key, ~index) pairs).
__global__ __launch_bounds__(1024) void rpn_select_kernel(const float* __restrict__ obj, RpnSegs g, int* counts,
                                                          int* index) {
  __shared__ unsigned long long comp[RPN_MAX_K];
  __shared__ int hist[2048];
  __shared__ int wsum[16];
  __shared__ int weq[16];
  __shared__ int sh[4];   // bin, ties still to admit, keys equal to the K-th, slot counter of the keys above
  __shared__ int sh_eq;
  const int s = blockIdx.x, l = s / g.batch, b = s - l * g.batch;
  const int HW = g.H[l] * g.W[l], n = g.A * HW, K = min(g.k, n);
  const float* x = obj + (g.pos0[l] + (long long)b * HW) * g.A;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  unsigned prefix = 0, pmask = 0;
  int k_rem = K, eq_total = 0;
#pragma nounroll
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const int nb = pass == 2 ? 1024 : 2048, per = nb >> 10;
    hist[tid] = 0;
    hist[tid + 1024] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
      const unsigned key = rpn_key(x[i]);
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & (nb - 1)], 1);
    }
    __syncthreads();
    // thread t owns the bins nb-1 - per t ... (from the top); E = keys in the bins above its own
    int c = 0;
    for (int q = 0; q < per; ++q) c += hist[nb - 1 - (per * tid + q)];
    int E = block_excl_scan_1024(c, wsum);
    if (E < k_rem && k_rem <= E + c) {   // exactly one thread
      for (int q = 0; q < per; ++q) {
        const int bin = nb - 1 - (per * tid + q), hc = hist[bin];
        if (k_rem <= E + hc) {
          sh[0] = bin; sh[1] = k_rem - E; sh[2] = hc;
          break;
        }
        E += hc;
      }
    }
    __syncthreads();
    prefix |= (unsigned)sh[0] << shift;
    pmask |= (unsigned)(nb - 1) << shift;
    k_rem = sh[1];
    eq_total = sh[2];
    __syncthreads();
  }
  // prefix = the K-th largest key; k_rem of the eq_total keys equal to it are admitted, the lowest indices first
  const int gt_total = K - k_rem;
  const bool ordered = eq_total != k_rem;
  const int chunk = ((n + 15) / 16 + 63) & ~63;   // each wave walks a contiguous range, 64 indices at a time
  const int start = wave * chunk, end = min(n, start + chunk);
  if (tid == 0) { sh[3] = 0; sh_eq = 0; }
  if (ordered) {
    int cnt = 0;
    for (int i0 = start; i0 < end; i0 += 64) {
      const int i = i0 + lane;
      const bool eq = i < end && rpn_key(x[i]) == prefix;
      cnt += __popcll(__ballot(eq));
    }
    if (lane == 0) weq[wave] = cnt;
  }
  __syncthreads();
  int ord = 0;   // ties in front of this wave's 64 indices
  if (ordered)
    for (int w = 0; w < wave; ++w) ord += weq[w];
  for (int i0 = start; i0 < end; i0 += 64) {
    const int i = i0 + lane;
    const unsigned key = i < end ? rpn_key(x[i]) : 0u;
    const bool gt = i < end && key > prefix, eq = i < end && key == prefix;
    const unsigned long long beq = __ballot(eq);
    int slot = -1;
    if (gt) slot = atomicAdd(&sh[3], 1);
    if (eq) {
      if (ordered) {
        const int o = ord + __popcll(beq & ((1ull << lane) - 1ull));
        if (o < k_rem) slot = gt_total + o;
      } else {
        slot = gt_total + atomicAdd(&sh_eq, 1);
      }
    }
    ord += __popcll(beq);
    if (slot >= 0 && slot < K) comp[slot] = ((unsigned long long)key << 32) | (unsigned)(0xffffffffu - (unsigned)i);
  }
  __syncthreads();
  // rank by counting: larger key first, then the lower index (pairs are distinct)
  unsigned long long mine[RPN_MAX_K / 1024];
  int r[RPN_MAX_K / 1024];
#pragma unroll
  for (int q = 0; q < RPN_MAX_K / 1024; ++q) {
    const int i = tid + 1024 * q;
    mine[q] = i < K ? comp[i] : ~0ull;
    r[q] = 0;
  }
  if (tid < K)
    for (int j = 0; j < K; ++j) {
      const unsigned long long c = comp[j];
#pragma unroll
      for (int q = 0; q < RPN_MAX_K / 1024; ++q) r[q] += c > mine[q];
    }
  int* out = index + (long long)s * g.k;
#pragma unroll
  for (int q = 0; q < RPN_MAX_K / 1024; ++q) {
    const int i = tid + 1024 * q;
    if (i < K) out[r[q]] = (int)(0xffffffffu - (unsigned)(mine[q] & 0xffffffffull));
    else if (i < g.k) out[i] = -1;
  }
  if (tid == 0) counts[s] = K;
}

// ---- decode: thread = (segment, rank) ------------------------------------------------------------------------------------
// anchor = base[l][a] + (w stride_w, h stride_h, w stride_w, h stride_h); BoxCoder(1, 1, 1, 1).decode_single with separate
// multiplies and adds as torch issues them; clip to the image's own size; score = sigmoid(logit); valid = both sides >=
// min_size and score > score_thresh (a NaN fails).  Ranks behind the segment's count: zeros, invalid.
__global__ __launch_bounds__(256) void rpn_decode_kernel(const float* __restrict__ obj, const float* __restrict__ deltas,
                                                         const int* __restrict__ counts, const int* __restrict__ index,
                                                         RpnSegs g, const float* __restrict__ base_anchors,
                                                         const float* __restrict__ image_sizes, float clip, float min_size,
                                                         float score_thresh, float* boxes, float* logits, float* scores,
                                                         int* valid) {
  const int s = blockIdx.y, rk = blockIdx.x * 256 + threadIdx.x;
  if (rk >= g.k) return;
  const long long o = (long long)s * g.k + rk;
  const int l = s / g.batch, b = s - l * g.batch;
  const int W = g.W[l], HW = g.H[l] * W;
  const int idx = rk < counts[s] ? index[o] : -1;
  if (idx < 0 || idx >= g.A * HW) {
    boxes[4 * o] = 0.f; boxes[4 * o + 1] = 0.f; boxes[4 * o + 2] = 0.f; boxes[4 * o + 3] = 0.f;
    logits[o] = 0.f; scores[o] = 0.f; valid[o] = 0;
    return;
  }
  const int p = idx / g.A, a = idx - p * g.A, h = p / W, w = p - h * W;
  const long long pos = g.pos0[l] + (long long)b * HW + p;
  const float* ba = base_anchors + ((long long)l * g.A + a) * 4;
  const float sx = (float)(w * g.stride_w[l]), sy = (float)(h * g.stride_h[l]);
  const float ax1 = ba[0] + sx, ay1 = ba[1] + sy, ax2 = ba[2] + sx, ay2 = ba[3] + sy;
  const float aw = ax2 - ax1, ah = ay2 - ay1;
  const float cx = ax1 + __fmul_rn(0.5f, aw), cy = ay1 + __fmul_rn(0.5f, ah);
  const float* d = deltas + (pos * g.A + a) * 4;
  const float dx = d[0], dy = d[1], dw = fminf(d[2], clip), dh = fminf(d[3], clip);
  const float pcx = __fmul_rn(dx, aw) + cx, pcy = __fmul_rn(dy, ah) + cy;
  const float hw_ = __fmul_rn(0.5f, __fmul_rn(expf(dw), aw)), hh_ = __fmul_rn(0.5f, __fmul_rn(expf(dh), ah));
  const float img_h = image_sizes[2 * b], img_w = image_sizes[2 * b + 1];
  const float x1 = fminf(fmaxf(pcx - hw_, 0.f), img_w), x2 = fminf(fmaxf(pcx + hw_, 0.f), img_w);
  const float y1 = fminf(fmaxf(pcy - hh_, 0.f), img_h), y2 = fminf(fmaxf(pcy + hh_, 0.f), img_h);
  const float z = obj[pos * g.A + a];
  const float sc = 1.f / (1.f + expf(-z));
  boxes[4 * o] = x1; boxes[4 * o + 1] = y1; boxes[4 * o + 2] = x2; boxes[4 * o + 3] = y2;
  logits[o] = z;
  scores[o] = sc;
  valid[o] = (x2 - x1) >= min_size && (y2 - y1) >= min_size && sc > score_thresh;
}

// ---- NMS -----------------------------------------------------------------------------------------------------------------
// workspace: [mask S x kpad x nw x 8 B] [kept S x k] [klogit S x k] [nkept S], kpad = 64 nw, nw = ceil(k / 64)
struct RpnWs {
  unsigned long long* mask;
  int* kept;
  float* klogit;
  int* nkept;
  int nw;
};
static inline size_t rpn_ws_layout(int segs, int k, void* base, RpnWs* w) {
  const int nw = (k + 63) / 64;
  char* p = (char*)base;
  size_t o = 0;
  if (w) { w->mask = (unsigned long long*)p; w->nw = nw; }
  o += (size_t)segs * nw * 64 * nw * 8;
  if (w) w->kept = (int*)(p + o);
  o += (((size_t)segs * k * 4) + 15) & ~(size_t)15;
  if (w) w->klogit = (float*)(p + o);
  o += (((size_t)segs * k * 4) + 15) & ~(size_t)15;
  if (w) w->nkept = (int*)(p + o);
  o += (((size_t)segs * 4) + 15) & ~(size_t)15;
  return o;
}

// mask[s][i][bj] bit jj: candidate j = 64 bj + jj > i of segment s has IoU(i, j) > thresh (det_iou_kernel's arithmetic:
// inter / (area_i + area_j - inter), fp32, every operation rounded on its own)
__global__ __launch_bounds__(64) void rpn_iou_kernel(const float* __restrict__ boxes, const int* __restrict__ counts,
                                                     int k, float nms_thresh, RpnWs ws) {
  __shared__ float cb[64][4];
  const int s = blockIdx.z, bi = blockIdx.y, bj = blockIdx.x, t = threadIdx.x;
  const int nv = min(counts[s], k);
  if (bj < bi || bi * 64 >= nv || bj * 64 >= nv) return;   // block-uniform; the scan reads words bj >= bi below ceil(nv / 64)
  const float* sb = boxes + 4 * (long long)s * k;
  const int jc = bj * 64 + t;
  if (jc < nv)
    for (int d = 0; d < 4; ++d) cb[t][d] = sb[4 * (long long)jc + d];
  __syncthreads();
  const int i = bi * 64 + t;
  unsigned long long bits = 0;
  if (i < nv) {
    const float* a = sb + 4 * (long long)i;
    const float ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3];
    const float area_a = __fmul_rn(ax2 - ax1, ay2 - ay1);
    for (int jj = 0; jj < 64; ++jj) {
      const int j = bj * 64 + jj;
      if (j <= i || j >= nv) continue;
      const float w = fmaxf(fminf(ax2, cb[jj][2]) - fmaxf(ax1, cb[jj][0]), 0.f);
      const float h = fmaxf(fminf(ay2, cb[jj][3]) - fmaxf(ay1, cb[jj][1]), 0.f);
      const float inter = __fmul_rn(w, h);
      const float area_b = __fmul_rn(cb[jj][2] - cb[jj][0], cb[jj][3] - cb[jj][1]);
      const float iou = inter / (__fadd_rn(area_a, area_b) - inter);
      if (iou > nms_thresh) bits |= 1ull << jj;
    }
  }
  ws.mask[((long long)s * ws.nw * 64 + i) * ws.nw + bj] = bits;   // rows nv .. 64 ceil(nv / 64): zeros
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// Blocked greedy scan, one workgroup of four waves per segment.  Lane w of every wave holds word w of the removed bitmap
// (invalid candidates start removed).  Per block of 64 candidates: the block's kept ones follow from its diagonal mask
// words alone (a register chain, no memory in it); then the rows of the kept ones are OR-ed into the words behind the
// block, sixteen independent loads per wave.  The dependent chain through memory is ceil(n / 64) steps.
__global__ __launch_bounds__(256) void rpn_scan_kernel(const float* __restrict__ logits, const int* __restrict__ valid,
                                                       const int* __restrict__ counts, int k, int post, RpnWs ws) {
  __shared__ unsigned long long part[4][64];
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = min(counts[s], k), nb = (nv + 63) / 64, nw = ws.nw;
  const unsigned long long* mp = ws.mask + (long long)s * nw * 64 * nw;
  const long long so = (long long)s * k;
  unsigned long long removed = ~0ull;
  for (int b = 0; b < nb; ++b) {
    const int i = b * 64 + lane;
    const unsigned long long bal = __ballot(i < nv && valid[so + i] != 0);
    if (lane == b) removed = ~bal;
  }
  int nk = 0;
  for (int b = 0; b < nb && nk < post; ++b) {
    unsigned long long rem = shfl64(removed, b);
    const int i = b * 64 + lane;
    const unsigned long long diag = i < nv ? mp[(long long)i * nw + b] : 0ull;
    unsigned long long keptm = 0;
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const unsigned long long dt = shfl64(diag, t);
      if (!((rem >> t) & 1ull)) {   // wave-uniform
        keptm |= 1ull << t;
        rem |= dt;
      }
    }
    while (__popcll(keptm) > post - nk) keptm &= ~(1ull << (63 - __clzll((long long)keptm)));
    if (wave == 0 && ((keptm >> lane) & 1ull)) {
      const int pos = nk + __popcll(keptm & ((1ull << lane) - 1ull));
      ws.kept[so + pos] = i;
      ws.klogit[so + pos] = logits[so + i];
    }
    nk += __popcll(keptm);
    if (nk >= post || b + 1 >= nb) break;   // block-uniform
    unsigned long long acc = 0;
    const bool live = lane > b && lane < nb;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int t = wave * 16 + q;
      const unsigned long long v = live ? mp[(long long)(b * 64 + t) * nw + lane] : 0ull;   // rows < 64 nb <= kpad
      acc |= ((keptm >> t) & 1ull) ? v : 0ull;
    }
    part[wave][lane] = acc;
    __syncthreads();
    removed |= part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws.nkept[s] = nk;
}

// Merge of the levels' kept lists of one image (each in logit order) by counting: the rank of a kept candidate is its
// place in its own list plus, per other level, the entries that come first (larger logit; equal logit in a lower level).
// The first `post` are stored, zeros / -1 behind the count.
__global__ __launch_bounds__(256) void rpn_merge_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                        int n_levels, int batch, int k, int post, RpnWs ws,
                                                        float* out_boxes, float* out_scores, int* out_index,
                                                        int* out_count) {
  const int b = blockIdx.x;
  int total = 0;
  for (int l = 0; l < n_levels; ++l) total += ws.nkept[l * batch + b];
  const int cnt = min(total, post);
  float* ob = out_boxes + 4ll * b * post;
  float* os = out_scores + (long long)b * post;
  int* oi = out_index + (long long)b * post;
  for (int e = threadIdx.x; e < total; e += 256) {
    int l = 0, p = e;
    while (p >= ws.nkept[l * batch + b]) { p -= ws.nkept[l * batch + b]; ++l; }
    const long long so = (long long)(l * batch + b) * k;
    const float z = ws.klogit[so + p];
    int rank = p;
    for (int l2 = 0; l2 < n_levels; ++l2) {
      if (l2 == l) continue;
      const int s2 = l2 * batch + b, n2 = ws.nkept[s2];
      const float* kz = ws.klogit + (long long)s2 * k;
      int lo = 0, hi = n2;   // first entry that does not come before (z, l)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float v = kz[mid];
        if (v > z || (v == z && l2 < l)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < post) {
      const int i = ws.kept[so + p];
      for (int d = 0; d < 4; ++d) ob[4 * rank + d] = boxes[4 * (so + i) + d];
      os[rank] = scores[so + i];
      oi[rank] = l * k + i;
    }
  }
  for (int r = cnt + threadIdx.x; r < post; r += 256) {
    for (int d = 0; d < 4; ++d) ob[4 * r + d] = 0.f;
    os[r] = 0.f;
    oi[r] = -1;
  }
  if (threadIdx.x == 0) out_count[b] = cnt;
}

// the checks every rpn entry point shares
static int check_rpn(const char* what, int n_levels, int batch, int num_anchors, int k) {
  SFVOS_REQUIRE(n_levels >= 1 && n_levels <= SFVOS_MAX_LEVELS, "%s: n_levels %d out of [1, %d]", what, n_levels,
                SFVOS_MAX_LEVELS);
  SFVOS_REQUIRE(batch >= 1 && batch <= 4096, "%s: batch %d out of [1, 4096]", what, batch);
  SFVOS_REQUIRE(num_anchors >= 1 && num_anchors <= RPN_MAX_A, "%s: num_anchors %d out of [1, %d]", what, num_anchors,
                RPN_MAX_A);
  SFVOS_REQUIRE(k >= 1 && k <= RPN_MAX_K, "%s: pre_nms_top_n %d out of [1, %d]", what, k, RPN_MAX_K);
  return SFVOS_OK;
}

static int make_segs(const char* what, const sfvos_pyramid* pyr, int batch, int A, int k, int tensor_h, int tensor_w,
                     RpnSegs* g) {
  SFVOS_REQUIRE(pyr != nullptr, "%s: null pyramid", what);
  if (int rc = check_rpn(what, pyr->n_levels, batch, A, k)) return rc;
  g->n_levels = pyr->n_levels; g->batch = batch; g->A = A; g->k = k;
  long long px = 0;
  for (int l = 0; l < SFVOS_MAX_LEVELS; ++l) {
    const bool live = l < pyr->n_levels;
    const int H = live ? pyr->h[l] : 1, W = live ? pyr->w[l] : 1;
    SFVOS_REQUIRE(H >= 1 && W >= 1 && (long long)H * W * A < (1ll << 30), "%s: level %d has bad extent %dx%d", what, l, H,
                  W);
    g->H[l] = H; g->W[l] = W;
    g->stride_h[l] = tensor_h / H; g->stride_w[l] = tensor_w / W;
    g->pos0[l] = (long long)batch * px;
    if (live) px += (long long)H * W;
  }
  return SFVOS_OK;
}

}  // namespace sfvos

using namespace sfvos;

extern "C" size_t sfvos_rpn_workspace_bytes(int n_levels, int batch, int pre_nms_top_n) {
  if (n_levels < 1 || n_levels > SFVOS_MAX_LEVELS || batch < 1 || batch > 4096 || pre_nms_top_n < 1 ||
      pre_nms_top_n > RPN_MAX_K)
    return 0;
  return rpn_ws_layout(n_levels * batch, pre_nms_top_n, nullptr, nullptr);
}

extern "C" int sfvos_rpn_select(const float* objectness, const sfvos_pyramid* pyr, int batch, int num_anchors,
                                int pre_nms_top_n, int* counts, int* index, sfvos_stream_t stream) {
  SFVOS_REQUIRE(objectness && counts && index, "rpn_select: null pointer");
  RpnSegs g;
  if (int rc = make_segs("rpn_select", pyr, batch, num_anchors, pre_nms_top_n, 1, 1, &g)) return rc;
  hipLaunchKernelGGL(rpn_select_kernel, dim3((unsigned)(g.n_levels * batch)), dim3(1024), 0, (hipStream_t)stream,
                     objectness, g, counts, index);
  return check_launch("rpn_select");
}

extern "C" int sfvos_rpn_decode(const float* objectness, const float* deltas, const int* counts, const int* index,
                                const sfvos_pyramid* pyr, int batch, int num_anchors, int pre_nms_top_n,
                                const float* base_anchors, int tensor_h, int tensor_w, const float* image_sizes,
                                float clip, float min_size, float score_thresh, float* boxes, float* logits,
                                float* scores, int* valid, sfvos_stream_t stream) {
  SFVOS_REQUIRE(objectness && deltas && counts && index && base_anchors && image_sizes && boxes && logits && scores &&
                    valid,
                "rpn_decode: null pointer");
  SFVOS_REQUIRE(tensor_h >= 1 && tensor_w >= 1, "rpn_decode: bad tensor size %dx%d", tensor_h, tensor_w);
  RpnSegs g;
  if (int rc = make_segs("rpn_decode", pyr, batch, num_anchors, pre_nms_top_n, tensor_h, tensor_w, &g)) return rc;
  hipLaunchKernelGGL(rpn_decode_kernel, dim3((unsigned)ceil_div(pre_nms_top_n, 256), (unsigned)(g.n_levels * batch)),
                     dim3(256), 0, (hipStream_t)stream, objectness, deltas, counts, index, g, base_anchors, image_sizes,
                     clip, min_size, score_thresh, boxes, logits, scores, valid);
  return check_launch("rpn_decode");
}

extern "C" int sfvos_rpn_nms(const float* boxes, const float* logits, const float* scores, const int* valid,
                             const int* counts, int n_levels, int batch, int pre_nms_top_n, float nms_thresh,
                             int post_nms_top_n, void* workspace, float* out_boxes, float* out_scores, int* out_index,
                             int* out_count, sfvos_stream_t stream) {
  SFVOS_REQUIRE(boxes && logits && scores && valid && counts && workspace && out_boxes && out_scores && out_index &&
                    out_count,
                "rpn_nms: null pointer");
  if (int rc = check_rpn("rpn_nms", n_levels, batch, 1, pre_nms_top_n)) return rc;
  SFVOS_REQUIRE(post_nms_top_n >= 1 && post_nms_top_n <= (1 << 20), "rpn_nms: post_nms_top_n %d out of [1, 2^20]",
                post_nms_top_n);
  const int segs = n_levels * batch, k = pre_nms_top_n;
  RpnWs ws;
  rpn_ws_layout(segs, k, workspace, &ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rpn_iou_kernel, dim3((unsigned)ws.nw, (unsigned)ws.nw, (unsigned)segs), dim3(64), 0, st, boxes,
                     counts, k, nms_thresh, ws);
  hipLaunchKernelGGL(rpn_scan_kernel, dim3((unsigned)segs), dim3(256), 0, st, logits, valid, counts, k, post_nms_top_n,
                     ws);
  hipLaunchKernelGGL(rpn_merge_kernel, dim3((unsigned)batch), dim3(256), 0, st, boxes, scores, n_levels, batch, k,
                     post_nms_top_n, ws, out_boxes, out_scores, out_index, out_count);
  return check_launch("rpn_nms");
}
