// boxes.hip -- the box branch of roi_heads behind its two dense layers (dense.hip), restated from torchvision's
// published sources (models/detection/faster_rcnn.py: FastRCNNPredictor; roi_heads.py: fastrcnn_loss,
// postprocess_detections; _utils.py: BoxCoder; ops/boxes.py: clip_boxes_to_image, remove_small_boxes, batched_nms;
// transform.py: resize_boxes) -- parity unpinned by the reference, torchvision is neither vendored nor installed:
//
//   cls_score (C -> K) + bbox_pred (C -> 4K)                       sfvos_box_predictor / _bwd (project.hip)
//   cross_entropy + smooth_l1(beta 1/9, sum) / N                   sfvos_fastrcnn_loss / _grad
//   BoxCoder.decode + softmax + clip, class 0 dropped              sfvos_box_decode;  BoxCoder.encode_single: sfvos_box_encode
//   score threshold, small boxes, class-wise NMS, top k, resize    sfvos_detections
//
// Everything is reduced in a fixed order (no atomics on data): bit-identical from run to run.
#include "elt_util.h"

namespace sfvos {

// candidates of one sfvos_detections call: 1000 RoIs x 7 foreground classes fit; ranking is n^2 compare steps
// (6.7e7 at the cap) and the IoU masks take n^2 / 8 bytes (8 MB)
constexpr int DET_MAX_N = 8192;

// ---- fastrcnn_loss ----------------------------------------------------------------------------------------------------
//   losses[0] = mean_i ( logsumexp(z_i) - z_i[label_i] )
//   losses[1] = sum_{i: label_i > 0} sum_{d < 4} smooth_l1(deltas[i][4 label_i + d] - targets[i][d]; beta) / N
// A label outside [0, K) makes both NaN and nothing is read through it.
// (smooth_l1: elt_util.h)

__global__ __launch_bounds__(1024) void fastrcnn_loss_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ deltas,
                                                             const long long* __restrict__ labels,
                                                             const float* __restrict__ targets, int N, int K,
                                                             float beta, float* losses) {
  __shared__ double red[2][1024];
  double sc = 0.0, sb = 0.0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const long long lab = labels[i];
    if (lab < 0 || lab >= K) {
      sc += (double)__builtin_nanf("");
      sb += (double)__builtin_nanf("");
      continue;
    }
    const float* z = logits + (long long)i * K;
    float mx = z[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
    float se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(z[k] - mx);
    sc += (double)(mx + logf(se) - z[lab]);
    if (lab > 0) {
      float b = 0.f;
      for (int d = 0; d < 4; ++d)
        b += smooth_l1(deltas[(long long)i * 4 * K + 4 * lab + d] - targets[(long long)i * 4 + d], beta);
      sb += (double)b;
    }
  }
  sc = block_sum_1024(red[0], sc);
  sb = block_sum_1024(red[1], sb);
  if (threadIdx.x == 0) {
    losses[0] = (float)(sc / (double)N);
    losses[1] = (float)(sb / (double)N);
  }
}

//   dlogits[i][k] = up[0] (softmax(z_i)[k] - [k == label_i]) / N
//   ddeltas[i][j] = up[1] clamp((deltas - targets) / beta, -1, 1) / N  for j in the 4 columns of label_i > 0, else 0
__global__ __launch_bounds__(256) void fastrcnn_loss_grad_kernel(const float* __restrict__ logits,
                                                                 const float* __restrict__ deltas,
                                                                 const long long* __restrict__ labels,
                                                                 const float* __restrict__ targets,
                                                                 const float* __restrict__ upstream, int N, int K,
                                                                 float beta, float* dlogits, float* ddeltas) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float uc = (upstream ? upstream[0] : 1.f) / (float)N, ub = (upstream ? upstream[1] : 1.f) / (float)N;
  const long long lab = labels[i];
  const bool ok = lab >= 0 && lab < K;   // an out-of-range label: zero gradient
  const float* z = logits + (long long)i * K;
  float mx = z[0];
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
  float se = 0.f;
  for (int k = 0; k < K; ++k) se += expf(z[k] - mx);
  for (int k = 0; k < K; ++k)
    dlogits[(long long)i * K + k] = ok ? uc * (expf(z[k] - mx) / se - (k == lab ? 1.f : 0.f)) : 0.f;
  for (int j = 0; j < 4 * K; ++j) {
    float gd = 0.f;
    if (ok && lab > 0 && (j >> 2) == lab) {
      const float d = deltas[(long long)i * 4 * K + j] - targets[(long long)i * 4 + (j & 3)];
      gd = ub * (fabsf(d) < beta ? d / beta : (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f));
    }
    ddeltas[(long long)i * 4 * K + j] = gd;
  }
}

// ---- BoxCoder ---------------------------------------------------------------------------------------------------------
// decode of the classes [first, K) of each RoI (+ softmax score and label of the class when scores != NULL, clipping to
// the image when img_w > 0): candidate i (K - first) + (k - first).  Separate multiplies and adds as torch issues them.
__global__ __launch_bounds__(256) void box_decode_kernel(const float* __restrict__ logits, const float* __restrict__ deltas,
                                                         const float* __restrict__ props, int M, int K, int first,
                                                         float wx, float wy, float ww, float wh, float clip, float img_h,
                                                         float img_w, float* boxes, float* scores, long long* labels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const float* p = props + 4 * (long long)i;
  const float pw = p[2] - p[0], ph = p[3] - p[1];
  const float cx = p[0] + __fmul_rn(0.5f, pw), cy = p[1] + __fmul_rn(0.5f, ph);
  float mx = 0.f, se = 1.f;
  if (scores) {
    const float* z = logits + (long long)i * K;
    mx = z[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
    se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(z[k] - mx);
  }
  for (int k = first; k < K; ++k) {
    const float* d = deltas + ((long long)i * K + k) * 4;
    const float dx = d[0] / wx, dy = d[1] / wy, dw = fminf(d[2] / ww, clip), dh = fminf(d[3] / wh, clip);
    const float pcx = __fmul_rn(dx, pw) + cx, pcy = __fmul_rn(dy, ph) + cy;
    const float hw_ = __fmul_rn(0.5f, __fmul_rn(expf(dw), pw)), hh_ = __fmul_rn(0.5f, __fmul_rn(expf(dh), ph));
    float x1 = pcx - hw_, y1 = pcy - hh_, x2 = pcx + hw_, y2 = pcy + hh_;
    if (img_w > 0.f) {
      x1 = fminf(fmaxf(x1, 0.f), img_w); x2 = fminf(fmaxf(x2, 0.f), img_w);
      y1 = fminf(fmaxf(y1, 0.f), img_h); y2 = fminf(fmaxf(y2, 0.f), img_h);
    }
    const long long o = (long long)i * (K - first) + (k - first);
    boxes[4 * o] = x1; boxes[4 * o + 1] = y1; boxes[4 * o + 2] = x2; boxes[4 * o + 3] = y2;
    if (scores) scores[o] = expf(logits[(long long)i * K + k] - mx) / se;
    if (labels) labels[o] = k;
  }
}

// encode_single: targets of the reference boxes against the proposals
__global__ __launch_bounds__(256) void box_encode_kernel(const float* __restrict__ ref, const float* __restrict__ props,
                                                         int M, float wx, float wy, float ww, float wh, float* targets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  box_encode_one(ref + 4 * (long long)i, props + 4 * (long long)i, wx, wy, ww, wh, targets + 4 * (long long)i);
}

// transform.resize_boxes
__global__ __launch_bounds__(256) void box_scale_kernel(const float* __restrict__ boxes, int n, float ratio_h,
                                                        float ratio_w, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // one coordinate
  if (i < 4 * n) out[i] = boxes[i] * ((i & 1) ? ratio_h : ratio_w);
}

// ---- postprocess_detections behind the decode: filter, rank, class-wise NMS, top k -----------------------------------
// workspace: [nvalid (16 B)] [valid n] [order n] [slabel n] [sbox n x 4] [mask n x nw x 8 B], nw = ceil(n / 64)
struct DetWs {
  int* nvalid;
  int* valid;
  int* order;
  int* slabel;
  float* sbox;
  unsigned long long* mask;
  int nw;
};
static inline size_t det_ws_layout(int n, void* base, DetWs* w) {
  const size_t n4 = ((size_t)n * 4 + 15) & ~(size_t)15;
  char* p = (char*)base;
  size_t o = 16;
  if (w) w->nvalid = (int*)p;
  if (w) w->valid = (int*)(p + o);
  o += n4;
  if (w) w->order = (int*)(p + o);
  o += n4;
  if (w) w->slabel = (int*)(p + o);
  o += n4;
  if (w) w->sbox = (float*)(p + o);
  o += (size_t)n * 16;
  if (w) w->mask = (unsigned long long*)(p + o);
  const int nw = (n + 63) / 64;
  if (w) w->nw = nw;
  o += (size_t)n * nw * 8;
  return o;
}

// a candidate stays when score > thresh and both sides >= min_size (NaN scores fail the comparison)
__global__ __launch_bounds__(1024) void det_filter_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                          int n, float score_thresh, float min_size, DetWs ws) {
  __shared__ int red[1024];
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float* b = boxes + 4 * (long long)i;
    const int v = scores[i] > score_thresh && (b[2] - b[0]) >= min_size && (b[3] - b[1]) >= min_size;
    ws.valid[i] = v;
    cnt += v;
  }
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws.nvalid[0] = red[0];
}

// rank by counting: position of candidate i among the valid ones in descending score, ties by the lower index
__global__ __launch_bounds__(256) void det_rank_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                       const long long* __restrict__ labels, int n, DetWs ws) {
  __shared__ float ss[256];
  __shared__ int sv[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool mine = i < n && ws.valid[i];
  const float s = mine ? scores[i] : 0.f;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    sv[threadIdx.x] = j < n ? ws.valid[j] : 0;
    ss[threadIdx.x] = j < n ? scores[j] : 0.f;
    __syncthreads();
    if (mine)
      for (int t = 0; t < 256; ++t)
        if (sv[t] && (ss[t] > s || (ss[t] == s && j0 + t < i))) ++rank;
    __syncthreads();
  }
  if (mine) {
    ws.order[rank] = i;
    ws.slabel[rank] = (int)labels[i];
    for (int d = 0; d < 4; ++d) ws.sbox[4 * (long long)rank + d] = boxes[4 * (long long)i + d];
  }
}

// mask[i][bj] bit jj: ranked candidate j = 64 bj + jj > i has i's label and IoU(i, j) > thresh (torchvision's nms:
// inter / (area_i + area_j - inter), fp32, every operation rounded on its own)
__global__ __launch_bounds__(64) void det_iou_kernel(float nms_thresh, DetWs ws) {
  __shared__ float cb[64][4];
  __shared__ int cl[64];
  const int nv = ws.nvalid[0];
  const int bi = blockIdx.y, bj = blockIdx.x, t = threadIdx.x;
  if (bi * 64 >= nv) return;   // block-uniform
  const int jc = bj * 64 + t;
  if (jc < nv) {
    for (int d = 0; d < 4; ++d) cb[t][d] = ws.sbox[4 * (long long)jc + d];
    cl[t] = ws.slabel[jc];
  }
  __syncthreads();
  const int i = bi * 64 + t;
  if (i >= nv) return;
  unsigned long long bits = 0;
  if (bj >= bi) {
    const float* a = ws.sbox + 4 * (long long)i;
    const float ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3];
    const float area_a = __fmul_rn(ax2 - ax1, ay2 - ay1);
    const int la = ws.slabel[i];
    for (int jj = 0; jj < 64; ++jj) {
      const int j = bj * 64 + jj;
      if (j <= i || j >= nv || cl[jj] != la) continue;
      const float w = fmaxf(fminf(ax2, cb[jj][2]) - fmaxf(ax1, cb[jj][0]), 0.f);
      const float h = fmaxf(fminf(ay2, cb[jj][3]) - fmaxf(ay1, cb[jj][1]), 0.f);
      const float inter = __fmul_rn(w, h);
      const float area_b = __fmul_rn(cb[jj][2] - cb[jj][0], cb[jj][3] - cb[jj][1]);
      const float iou = inter / (__fadd_rn(area_a, area_b) - inter);
      if (iou > nms_thresh) bits |= 1ull << jj;
    }
  }
  ws.mask[(long long)i * ws.nw + bj] = bits;
}

// one wave walks the ranked candidates: the first max_det that no kept one suppresses; stores the detections (boxes
// scaled by the resize ratios), the count, and zeros / -1 behind it
__global__ __launch_bounds__(64) void det_scan_kernel(const float* __restrict__ scores, int classes_per_roi, int max_det,
                                                      float ratio_h, float ratio_w, DetWs ws, int* count,
                                                      float* out_boxes, float* out_scores, long long* out_labels,
                                                      int* out_index, int* out_roi) {
  __shared__ unsigned long long removed[DET_MAX_N / 64];
  const int lane = threadIdx.x, nv = ws.nvalid[0], nw = ws.nw;
  for (int w = lane; w < nw; w += 64) removed[w] = 0;
  __syncthreads();
  int kept = 0;
  for (int i = 0; i < nv && kept < max_det; ++i) {
    if ((removed[i >> 6] >> (i & 63)) & 1) continue;   // wave-uniform
    if (lane == 0) {
      const int src = ws.order[i];
      const float* b = ws.sbox + 4 * (long long)i;
      out_boxes[4 * kept] = b[0] * ratio_w; out_boxes[4 * kept + 1] = b[1] * ratio_h;
      out_boxes[4 * kept + 2] = b[2] * ratio_w; out_boxes[4 * kept + 3] = b[3] * ratio_h;
      out_scores[kept] = scores[src];
      out_labels[kept] = ws.slabel[i];
      out_index[kept] = src;
      out_roi[kept] = src / classes_per_roi;
    }
    ++kept;
    __syncthreads();   // every lane has read removed[i >> 6]
    for (int w = (i >> 6) + lane; w < nw; w += 64) removed[w] |= ws.mask[(long long)i * nw + w];
    __syncthreads();
  }
  if (lane == 0) count[0] = kept;
  for (int k = kept + lane; k < max_det; k += 64) {
    for (int d = 0; d < 4; ++d) out_boxes[4 * k + d] = 0.f;
    out_scores[k] = 0.f;
    out_labels[k] = 0;
    out_index[k] = -1;
    out_roi[k] = -1;
  }
}

}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_fastrcnn_loss(const float* logits, const float* deltas, const int64_t* labels, const float* targets,
                                   int n, int num_classes, float beta, float* losses, sfvos_stream_t stream) {
  SFVOS_REQUIRE(logits && deltas && labels && targets && losses && n > 0 && beta > 0.f, "fastrcnn_loss: bad argument");
  if (int rc = check_classes("fastrcnn_loss", num_classes)) return rc;
  hipLaunchKernelGGL(fastrcnn_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, deltas,
                     (const long long*)labels, targets, n, num_classes, beta, losses);
  return check_launch("fastrcnn_loss");
}

extern "C" int sfvos_fastrcnn_loss_grad(const float* logits, const float* deltas, const int64_t* labels,
                                        const float* targets, const float* upstream, int n, int num_classes, float beta,
                                        float* dlogits, float* ddeltas, sfvos_stream_t stream) {
  SFVOS_REQUIRE(logits && deltas && labels && targets && dlogits && ddeltas && n > 0 && beta > 0.f,
                "fastrcnn_loss_grad: bad argument");
  if (int rc = check_classes("fastrcnn_loss_grad", num_classes)) return rc;
  hipLaunchKernelGGL(fastrcnn_loss_grad_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     logits, deltas, (const long long*)labels, targets, upstream, n, num_classes, beta, dlogits, ddeltas);
  return check_launch("fastrcnn_loss_grad");
}

extern "C" int sfvos_box_decode(const float* logits, const float* deltas, const float* proposals, int m, int num_classes,
                                int first_class, float wx, float wy, float ww, float wh, float clip, float img_h,
                                float img_w, float* boxes, float* scores, int64_t* labels, sfvos_stream_t stream) {
  SFVOS_REQUIRE(deltas && proposals && boxes && m > 0 && (!scores || logits), "box_decode: bad argument");
  if (int rc = check_classes("box_decode", num_classes)) return rc;
  SFVOS_REQUIRE(first_class >= 0 && first_class < num_classes, "box_decode: first_class %d out of [0, %d)", first_class,
                num_classes);
  SFVOS_REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "box_decode: weights must be positive");
  hipLaunchKernelGGL(box_decode_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (hipStream_t)stream, logits,
                     deltas, proposals, m, num_classes, first_class, wx, wy, ww, wh, clip, img_h, img_w, boxes, scores,
                     (long long*)labels);
  return check_launch("box_decode");
}

extern "C" int sfvos_box_encode(const float* reference, const float* proposals, int m, float wx, float wy, float ww,
                                float wh, float* targets, sfvos_stream_t stream) {
  SFVOS_REQUIRE(reference && proposals && targets && m > 0, "box_encode: bad argument");
  hipLaunchKernelGGL(box_encode_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (hipStream_t)stream, reference,
                     proposals, m, wx, wy, ww, wh, targets);
  return check_launch("box_encode");
}

extern "C" int sfvos_box_scale(const float* boxes, int n, float ratio_h, float ratio_w, float* out,
                               sfvos_stream_t stream) {
  SFVOS_REQUIRE(boxes && out && n > 0 && n < (1 << 28), "box_scale: bad argument");
  hipLaunchKernelGGL(box_scale_kernel, dim3((unsigned)ceil_div(4 * n, 256)), dim3(256), 0, (hipStream_t)stream, boxes, n,
                     ratio_h, ratio_w, out);
  return check_launch("box_scale");
}


extern "C" size_t sfvos_detections_workspace_bytes(int n) {
  return n > 0 && n <= DET_MAX_N ? det_ws_layout(n, nullptr, nullptr) : 0;
}

extern "C" int sfvos_detections(const float* boxes, const float* scores, const int64_t* labels, int n,
                                int classes_per_roi, float score_thresh, float min_size, float nms_thresh, int max_det,
                                float ratio_h, float ratio_w, void* workspace, int* count, float* out_boxes,
                                float* out_scores, int64_t* out_labels, int* out_index, int* out_roi,
                                sfvos_stream_t stream) {
  SFVOS_REQUIRE(boxes && scores && labels && workspace && count && out_boxes && out_scores && out_labels && out_index &&
                    out_roi,
                "detections: null pointer");
  SFVOS_REQUIRE(n > 0 && n <= DET_MAX_N, "detections: %d candidates out of [1, %d]", n, DET_MAX_N);
  SFVOS_REQUIRE(classes_per_roi >= 1 && max_det >= 1, "detections: bad classes_per_roi %d / max_det %d", classes_per_roi,
                max_det);
  DetWs ws;
  det_ws_layout(n, workspace, &ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(det_filter_kernel, dim3(1), dim3(1024), 0, st, boxes, scores, n, score_thresh, min_size, ws);
  hipLaunchKernelGGL(det_rank_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, boxes, scores,
                     (const long long*)labels, n, ws);
  hipLaunchKernelGGL(det_iou_kernel, dim3((unsigned)ws.nw, (unsigned)ws.nw), dim3(64), 0, st, nms_thresh, ws);
  hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(64), 0, st, scores, classes_per_roi, max_det, ratio_h, ratio_w, ws,
                     count, out_boxes, out_scores, (long long*)out_labels, out_index, out_roi);
  return check_launch("detections");
}
