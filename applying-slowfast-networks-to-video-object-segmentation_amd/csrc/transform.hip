// transform.hip -- torchvision's GeneralizedRCNNTransform in front of the ResNet body (model.py:283, :298): what the
// reference's `maskrcnn_model.transform(images, targets)` does to the pixels.
//
// sfvos_transform_image: normalise, bilinear resize (align_corners = False, the scale recomputed from the sizes) and zero
//   pad in ONE pass, written straight into the batched planar fp32 tensor sfvos_body_stem reads.  One thread owns 4
//   consecutive pixels of one output row for all 3 channels: the indices and weights of a pixel are computed once, each
//   channel ends in one 16-byte store, and the threads of a wave cover 1 KiB of a row per channel.  The grid covers the
//   whole Hp x Wp tensor, so the pad is written (+0.0f) by the same launch; a thread whose pixels lie in the pad loads
//   nothing.  No LDS: the source (at most 4 B per output pixel and channel, less when upscaling) is read through L1 / L2,
//   each tap by the threads that need it.  Algorithmically the kernel moves 12 B of stores per padded pixel; measured, it
//   reaches 0.2-0.3 of the achievable copy rate on a batch: a thread's 48 loads and 48 correctly
//   rounded divisions (one per tap and channel, the contract's order of operations) cost more than its three stores.
//   A byte source (a decoded HWC frame, read in place through its strides) is converted as ToTensor does, float(u) / 255.0f,
//   and then takes exactly the fp32 path.
//   The index and weight arithmetic is the header's contract (fp32, every operation rounded on its own): this file is
//   compiled without floating-point contraction, so no multiply-add fuses two of its roundings.
// sfvos_transform_masks: the nearest resize of the target masks, bytes to bytes; one thread makes 4 consecutive bytes
//   of a plane and stores them as one word where the address allows it.
#include "elt_util.h"

#pragma clang fp contract(off)

namespace sfvos {

struct TransformArgs {
  const void* src;
  long long sb, sc, sh, sw;    // source element strides
  float* dst;
  long long db, dc, dh;        // destination element strides (1 along w)
  int batch, h, w, oh, ow, Hp, Wp, Wq;   // Wq = groups of 4 pixels per padded row
  float scale_h, scale_w;      // (float)in / (float)out
  float mean[3], std[3];
};

// area_pixel_compute_source_index of upsample_bilinear2d (align_corners = False, cubic = False), in fp32
__device__ __forceinline__ float source_index(float scale, int d) {
  const float s = scale * ((float)d + 0.5f) - 0.5f;
  return s < 0.f ? 0.f : s;
}

template <bool U8> __device__ __forceinline__ float load_px(const void* p, long long off);
template <> __device__ __forceinline__ float load_px<false>(const void* p, long long off) { return ((const float*)p)[off]; }
template <> __device__ __forceinline__ float load_px<true>(const void* p, long long off) {
  return __fdiv_rn((float)((const unsigned char*)p)[off], 255.0f);   // ToTensor
}

template <bool U8>
__global__ __launch_bounds__(256) void transform_image_kernel(const TransformArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;    // (row, group of 4 pixels) of the padded frame; Hp * Wq < 2^31
  if (i >= a.Hp * a.Wq) return;
  const int y = i / a.Wq, x0 = (i - y * a.Wq) * 4;
  const bool inside = y < a.oh && x0 < a.ow;
  int y0 = 0, y1 = 0;
  float ly0 = 0.f, ly1 = 0.f;
  int xa[4], xb[4];
  float lx0[4], lx1[4];
  if (inside) {
    const float sy = source_index(a.scale_h, y);
    y0 = min((int)sy, a.h - 1);   // (int)sy < h for every size the entry point takes; the clamp only guards the load
    y1 = min(y0 + 1, a.h - 1);
    ly1 = sy - (float)(int)sy;
    ly0 = 1.f - ly1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sx = source_index(a.scale_w, x0 + j);   // pixels behind ow are computed and dropped (indices stay in range)
      xa[j] = min((int)sx, a.w - 1);
      xb[j] = min(xa[j] + 1, a.w - 1);
      lx1[j] = sx - (float)(int)sx;
      lx0[j] = 1.f - lx1[j];
    }
  }
  for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
    float* row = a.dst + (long long)b * a.db + (long long)y * a.dh + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (inside) {
        const long long base = (long long)b * a.sb + (long long)c * a.sc;
        const long long r0 = base + (long long)y0 * a.sh, r1 = base + (long long)y1 * a.sh;
        const float m = a.mean[c], s = a.std[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (x0 + j < a.ow) {
            const long long ca = (long long)xa[j] * a.sw, cb = (long long)xb[j] * a.sw;
            const float v00 = __fdiv_rn(load_px<U8>(a.src, r0 + ca) - m, s);
            const float v10 = __fdiv_rn(load_px<U8>(a.src, r1 + ca) - m, s);
            const float v01 = __fdiv_rn(load_px<U8>(a.src, r0 + cb) - m, s);
            const float v11 = __fdiv_rn(load_px<U8>(a.src, r1 + cb) - m, s);
            const float left = ly0 * v00 + ly1 * v10, right = ly0 * v01 + ly1 * v11;   // vertically first
            o[j] = lx0[j] * left + lx1[j] * right;
          }
        }
      }
      float* p = row + (long long)c * a.dc;
      if (x0 + 4 <= a.Wp) {
        *(f32x4*)p = f32x4{o[0], o[1], o[2], o[3]};
      } else {
        for (int j = 0; x0 + j < a.Wp; ++j) p[j] = o[j];
      }
    }
  }
}

// dst[g][y][x] = src[g][min((int)floorf(y * scale_h), h - 1)][min((int)floorf(x * scale_w), w - 1)]
__global__ __launch_bounds__(256) void transform_masks_kernel(const unsigned char* src, unsigned char* dst, int G, int h, int w,
                                                              int oh, int ow, float scale_h, float scale_w) {
  const int plane = oh * ow;                       // < 2^31 - 4 (checked by the entry point)
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= plane) return;
  const int n = min(4, plane - i0);
  int off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = min(i0 + j, plane - 1);
    const int y = i / ow, x = i - y * ow;
    const int sy = min((int)floorf((float)y * scale_h), h - 1), sx = min((int)floorf((float)x * scale_w), w - 1);
    off[j] = sy * w + sx;                          // h * w < 2^31 (checked)
  }
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const unsigned char* s = src + (long long)g * h * w;
    unsigned char* d = dst + (long long)g * plane + i0;
    unsigned v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = s[off[j]];
    if (n == 4 && ((uintptr_t)d & 3) == 0) {
      *(unsigned*)d = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
      for (int j = 0; j < n; ++j) d[j] = (unsigned char)v[j];
    }
  }
}

}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_transform_image(const void* src, int src_dtype, int64_t stride_b, int64_t stride_c, int64_t stride_h,
                                     int64_t stride_w, int batch, int h, int w, float mean0, float mean1, float mean2,
                                     float std0, float std1, float std2, float* dst, int64_t dst_stride_b,
                                     int64_t dst_stride_c, int64_t dst_stride_h, int oh, int ow, int Hp, int Wp,
                                     sfvos_stream_t stream) {
  SFVOS_REQUIRE(src && dst, "transform_image: null pointer");
  SFVOS_REQUIRE(src_dtype == SFVOS_F32 || src_dtype == SFVOS_U8, "transform_image: bad source dtype %d (f32 or u8)",
                src_dtype);
  SFVOS_REQUIRE(src_dtype == SFVOS_U8 || stride_w == 1, "transform_image: stride_w of an f32 source must be 1, got %lld",
                (long long)stride_w);
  SFVOS_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "transform_image: negative stride");
  SFVOS_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && oh >= 1 && ow >= 1 && Hp >= 1 && Wp >= 1,
                "transform_image: bad extent (batch %d, source %dx%d, image %dx%d, tensor %dx%d)", batch, h, w, oh, ow, Hp,
                Wp);
  SFVOS_REQUIRE(oh <= Hp && ow <= Wp, "transform_image: the image %dx%d does not fit the tensor %dx%d", oh, ow, Hp, Wp);
  const long long Wq = ceil_div64(Wp, 4);
  SFVOS_REQUIRE((long long)Hp * Wq < (1ll << 31) - 256 && (long long)h * w < (1ll << 31) && h < (1 << 23) &&
                    w < (1 << 23) && Hp < (1 << 23) && Wp < (1 << 23),
                "transform_image: frame too large (source %dx%d, tensor %dx%d)", h, w, Hp, Wp);
  SFVOS_REQUIRE(std0 > 0.f && std1 > 0.f && std2 > 0.f, "transform_image: std must be positive, got (%g, %g, %g)", std0,
                std1, std2);
  SFVOS_REQUIRE(mean0 == mean0 && mean1 == mean1 && mean2 == mean2, "transform_image: mean is NaN");
  SFVOS_REQUIRE((uintptr_t)dst % 16 == 0 && (src_dtype == SFVOS_U8 || (uintptr_t)src % 4 == 0),
                "transform_image: dst must be 16-byte aligned (an f32 source: 4)");
  SFVOS_REQUIRE(dst_stride_h >= Wp && dst_stride_h % 4 == 0 && dst_stride_c >= 0 && dst_stride_c % 4 == 0 &&
                    dst_stride_b >= 0 && dst_stride_b % 4 == 0,
                "transform_image: dst strides (%lld, %lld, %lld) must be non-negative multiples of 4 elements (16-byte "
                "rows), the row stride >= Wp %d",
                (long long)dst_stride_b, (long long)dst_stride_c, (long long)dst_stride_h, Wp);
  TransformArgs a;
  a.src = src; a.sb = stride_b; a.sc = stride_c; a.sh = stride_h; a.sw = stride_w;
  a.dst = dst; a.db = dst_stride_b; a.dc = dst_stride_c; a.dh = dst_stride_h;
  a.batch = batch; a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.Hp = Hp; a.Wp = Wp; a.Wq = (int)Wq;
  a.scale_h = (float)h / (float)oh; a.scale_w = (float)w / (float)ow;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.std[0] = std0; a.std[1] = std1; a.std[2] = std2;
  const dim3 grid((unsigned)ceil_div64((long long)Hp * Wq, 256), (unsigned)(batch < 65535 ? batch : 65535));
  if (src_dtype == SFVOS_U8)
    hipLaunchKernelGGL(transform_image_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(transform_image_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("transform_image");
}

extern "C" int sfvos_transform_masks(const unsigned char* src, int G, int h, int w, unsigned char* dst, int oh, int ow,
                                     sfvos_stream_t stream) {
  SFVOS_REQUIRE(G >= 0, "transform_masks: negative mask count %d", G);
  SFVOS_REQUIRE(h >= 1 && w >= 1 && oh >= 1 && ow >= 1, "transform_masks: bad extent (%dx%d -> %dx%d)", h, w, oh, ow);
  SFVOS_REQUIRE((long long)h * w < (1ll << 31) && (long long)oh * ow < (1ll << 31) - 1024 && oh < (1 << 24) && ow < (1 << 24),
                "transform_masks: plane too large (%dx%d -> %dx%d)", h, w, oh, ow);
  if (G == 0) return SFVOS_OK;
  SFVOS_REQUIRE(src && dst, "transform_masks: null pointer");
  const dim3 grid((unsigned)ceil_div64((long long)oh * ow, 1024), (unsigned)(G < 65535 ? G : 65535));
  hipLaunchKernelGGL(transform_masks_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, dst, G, h, w, oh, ow,
                     (float)h / (float)oh, (float)w / (float)ow);
  return check_launch("transform_masks");
}
