// Shared device/host helpers for libsfvos (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/sfvos.h"

namespace sfvos {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define SFVOS_LDS __attribute__((address_space(3)))
#define SFVOS_GLOBAL __attribute__((address_space(1)))

// ---- element traits: everything on chip is organised in 16-byte chunks ---------------------
template <int DT> struct Elt;
template <> struct Elt<SFVOS_F32> {
  typedef float type;
  static constexpr int CE = 4;  // elements per 16-B chunk
  static __device__ __forceinline__ float to_f32(float v) { return v; }
  static __device__ __forceinline__ float from_f32(float v) { return v; }
};
template <> struct Elt<SFVOS_BF16> {
  typedef __bf16 type;
  static constexpr int CE = 8;
  static __device__ __forceinline__ float to_f32(__bf16 v) { return (float)v; }
  static __device__ __forceinline__ __bf16 from_f32(float v) { return (__bf16)v; }
};

template <> struct Elt<SFVOS_FP8> {   // OCP e4m3 bytes; conversions go through v_cvt_pk_fp8_f32 / v_cvt_f32_fp8
  typedef unsigned char type;
  static constexpr int CE = 16;
};
// element type a conv writes for a given operand type: fp8 operands -> bf16 results
template <int DT> struct YOf { static constexpr int DTY = DT == SFVOS_FP8 ? SFVOS_BF16 : DT; };
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

// One MFMA "step" consumes one 16-B chunk per lane of A and of B: lane half h (lane>>5)
// holds chunk 2*step+h.  bf16: one 32x32x16; f32: four 32x32x2 (element e of both chunks
// pairs k = {chunk(2s)*4+e, chunk(2s+1)*4+e}); the k-sum is the same set either way.
template <int DT> struct Mma;
template <> struct Mma<SFVOS_BF16> {
  static __device__ __forceinline__ void run(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0,
                                                   0, 0);
  }
};
template <> struct Mma<SFVOS_F32> {
  static __device__ __forceinline__ void run(f32x16& acc, const u32x4& a, const u32x4& b) {
    f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], acc, 0, 0, 0);
  }
};

// async global -> LDS copy of 16 B per lane; LDS destination = wave-uniform base + lane*16.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const SFVOS_GLOBAL void*)gsrc, (SFVOS_LDS void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ u32x4 lds_read16(const void* p) { return *(const u32x4*)p; }
// two ds_read_b128 -> one 32-byte e4m3 MFMA operand (a register octet)
__device__ __forceinline__ i32x8 read8(const char* lo, const char* hi) {
  const i32x4 l = __builtin_bit_cast(i32x4, lds_read16(lo)), h = __builtin_bit_cast(i32x4, lds_read16(hi));
  return __builtin_shufflevector(l, h, 0, 1, 2, 3, 4, 5, 6, 7);
}

// LDS-DMA through a buffer descriptor, as one asm statement: buffer_load_dwordx4 ... offen lds.
// Why not __builtin_amdgcn_raw_ptr_buffer_load_lds: hipcc tracks that builtin as an LDS write and, when it cannot
// prove that the destination does not alias a following LDS read (dynamic ring slots), puts `s_waitcnt vmcnt(0)`
// right behind the copy -- a full memory round trip inside the MFMA loop.  The copies here are ordered by hand
// (one `s_waitcnt vmcnt(0)` + barrier per stage before anything reads what they wrote), so the statement is opaque
// to the compiler on purpose.  M0 (the LDS destination base) is saved and restored inside the statement.
//   base/records: descriptor of the source (wave-uniform); voff: this lane's byte offset, >= records reads zeros;
//   lds_offset: wave-uniform byte offset inside the workgroup's LDS allocation (kernels here have dynamic LDS only, so
//   `ptr - smem` is the LDS address), lane i lands at +16 i.
__device__ __forceinline__ void lds_dma16(const void* base, int records, unsigned voff, unsigned lds_offset) {
  const unsigned long long b = (unsigned long long)base;
  i32x4 rs;
  rs[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
  rs[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(b >> 32) & 0xffffu));   // stride 0
  rs[2] = __builtin_amdgcn_readfirstlane(records);
  rs[3] = 0x00020000;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_offset);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %2, %3, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(dst), "v"(voff), "s"(rs)
      : "memory");
}

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the instruction takes an immediate): one case per count in [LO, HI],
// any other count drains the counter.  Counts outside the range branch to the default, so the compiler drops their cases
// and each caller gets exactly the switch of its range.
template <int HI, int LO = 0>
__device__ __forceinline__ void wait_vmcnt(int n) {
  static_assert(LO >= 0 && HI <= 47, "wait_vmcnt: counts in [0, 47]");
#define SFVOS_VMW(k) \
  case k: if constexpr (k < LO || k > HI) goto drain; asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    SFVOS_VMW(0) SFVOS_VMW(1) SFVOS_VMW(2) SFVOS_VMW(3) SFVOS_VMW(4) SFVOS_VMW(5) SFVOS_VMW(6) SFVOS_VMW(7)
    SFVOS_VMW(8) SFVOS_VMW(9) SFVOS_VMW(10) SFVOS_VMW(11) SFVOS_VMW(12) SFVOS_VMW(13) SFVOS_VMW(14) SFVOS_VMW(15)
    SFVOS_VMW(16) SFVOS_VMW(17) SFVOS_VMW(18) SFVOS_VMW(19) SFVOS_VMW(20) SFVOS_VMW(21) SFVOS_VMW(22) SFVOS_VMW(23)
    SFVOS_VMW(24) SFVOS_VMW(25) SFVOS_VMW(26) SFVOS_VMW(27) SFVOS_VMW(28) SFVOS_VMW(29) SFVOS_VMW(30) SFVOS_VMW(31)
    SFVOS_VMW(32) SFVOS_VMW(33) SFVOS_VMW(34) SFVOS_VMW(35) SFVOS_VMW(36) SFVOS_VMW(37) SFVOS_VMW(38) SFVOS_VMW(39)
    SFVOS_VMW(40) SFVOS_VMW(41) SFVOS_VMW(42) SFVOS_VMW(43) SFVOS_VMW(44) SFVOS_VMW(45) SFVOS_VMW(46) SFVOS_VMW(47)
    default: drain: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;   // more than the counter holds: drain
  }
#undef SFVOS_VMW
}

// ---- host side -------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);
int current_device();   // hipGetDevice, -1 on error
int device_cu_count();  // compute units of the current device (256 when the query fails)

// hipFuncAttributeMaxDynamicSharedMemorySize must be raised once per (kernel, device): one instance per kernel
// template instantiation (function-local static), one atomic flag per device ordinal.
struct LdsAttrOnce {
  static constexpr int MAX_DEV = 64;
  int done[MAX_DEV] = {};
  int ensure(const void* kern, int lds_bytes, const char* what) {
    const int dev = current_device();
    if (dev >= 0 && dev < MAX_DEV && __atomic_load_n(&done[dev], __ATOMIC_ACQUIRE)) return SFVOS_OK;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) {
      set_error("%s: hipFuncSetAttribute(%d B LDS) failed: %s", what, lds_bytes, hipGetErrorString(e));
      return SFVOS_E_LAUNCH;
    }
    if (dev >= 0 && dev < MAX_DEV) __atomic_store_n(&done[dev], 1, __ATOMIC_RELEASE);
    return SFVOS_OK;
  }
};

// lateral.hip: dedicated kernel for the lateral (k x 1 x 1) data gradient; -1 = shape not covered
int lateral_dgrad_try(const sfvos_conv_desc* d, const void* x, const void* w_packed, void* y, hipStream_t stream);
// ... and for its forward (32 -> 64 channels): shape test, statistics rows (= workgroups) of a level, launch
bool lateral_fwd_applies(const sfvos_conv_desc* d);
int lateral_fwd_rows(const sfvos_conv_desc* d, int level);
int lateral_fwd_launch(const sfvos_conv_desc* d, const void* x, const void* w_packed, const float* bias, void* y,
                       float* stat_part, hipStream_t stream);

// lateral_wgrad.hip: weight gradient of the lateral convs; -1 / 0 = shape not covered
size_t lateral_wgrad_workspace_bytes(const sfvos_conv_desc* d);
int lateral_wgrad_try(const sfvos_conv_desc* d, const void* x, const void* dy, float* grad_w, int accumulate,
                      void* workspace, hipStream_t stream);
// wgrad.hip: grad_w[n][c][dt][tap] (=|+=) sum over the psplit slabs [n][dt][tap][c], fixed order
// wgrad_t1.hip: weight gradient of a kt x 3 x 3 conv 32 -> 32 with one output frame (fast_conv3); -1 / 0 = shape not covered
size_t wgrad_t1_workspace_bytes(const sfvos_conv_desc* d);
int wgrad_t1_try(const sfvos_conv_desc* d, const void* x, const void* dy, float* grad_w, int accumulate, void* workspace,
                 hipStream_t stream);
int launch_wgrad_reduce(const float* slab, int psplit, int c_out, int c_in, int kt, int taps, float* grad_w,
                        int accumulate, hipStream_t stream);

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

#define SFVOS_REQUIRE(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      sfvos::set_error(__VA_ARGS__); \
      return SFVOS_E_ARG;          \
    }                              \
  } while (0)

// ---- conv family (conv3d, wgrad, lateral, lateral_wgrad, wgrad_t1): descriptor, level table, launch -----------------

// The checks every conv entry point shares; `what` ("conv", "wgrad") prefixes the message.  The kernels' shape predicates
// run after it and rely on it: levels in [1, SFVOS_MAX_LEVELS], every extent >= 1, every x frame under 2 GiB.
static inline int check_conv_desc(const sfvos_conv_desc* d, const char* what) {
  SFVOS_REQUIRE(d != nullptr, "%s: null desc", what);
  SFVOS_REQUIRE(d->struct_size == (int)sizeof(sfvos_conv_desc),
                "%s: sfvos_conv_desc.struct_size is %d, this library's struct has %d bytes (stale binding?)", what,
                d->struct_size, (int)sizeof(sfvos_conv_desc));
  SFVOS_REQUIRE(d->dtype == SFVOS_F32 || d->dtype == SFVOS_BF16 || d->dtype == SFVOS_FP8, "%s: bad dtype %d", what,
                d->dtype);
  SFVOS_REQUIRE(d->taps == 9 || d->taps == 1, "%s: taps must be 9 or 1, got %d", what, d->taps);
  SFVOS_REQUIRE(d->c_in > 0 && d->c_in % 32 == 0 && d->c_out > 0 && d->c_out % 32 == 0,
                "%s: channels must be positive multiples of 32 (c_in %d, c_out %d)", what, d->c_in, d->c_out);
  SFVOS_REQUIRE(d->batch >= 1 && d->t_in >= 1 && d->kt >= 1 && d->t_alloc >= 1,
                "%s: bad extent (batch %d, t_in %d, kt %d, t_alloc %d)", what, d->batch, d->t_in, d->kt, d->t_alloc);
  // level-major x: the window [t_offset, t_offset + t_in) may stick out of the buffer's t_alloc frames on either side;
  // those frames are zeros (never read)
  SFVOS_REQUIRE(d->t_offset > -(1 << 20) && d->t_offset < (1 << 20) && d->t_in < (1 << 20),
                "%s: x window [t_offset %d, +t_in %d) out of range", what, d->t_offset, d->t_in);
  SFVOS_REQUIRE(d->pyr.n_levels >= 1 && d->pyr.n_levels <= SFVOS_MAX_LEVELS, "%s: n_levels %d out of [1,%d]", what,
                d->pyr.n_levels, SFVOS_MAX_LEVELS);
  const int es = d->dtype == SFVOS_BF16 ? 2 : d->dtype == SFVOS_FP8 ? 1 : 4;
  const long long pitch = d->x_group_stride ? 64 : (long long)d->ld_x * es;  // bytes between x positions of a frame
  for (int l = 0; l < d->pyr.n_levels; ++l) {
    const int H = d->pyr.h[l], W = d->pyr.w[l];
    SFVOS_REQUIRE(H >= 1 && W >= 1, "%s: level %d has bad extent %dx%d", what, l, H, W);
    SFVOS_REQUIRE((long long)H * W * pitch < (1ll << 31),
                  "%s: level %d frame of %dx%d x pitch %d exceeds the 2 GiB per-frame offset range", what, l, H, W,
                  d->ld_x);
  }
  return SFVOS_OK;
}

// positions of the largest frame of the pyramid (of a descriptor check_conv_desc accepted)
static inline long long max_frame_positions(const sfvos_conv_desc* d) {
  long long m = 0;
  for (int l = 0; l < d->pyr.n_levels; ++l)
    if ((long long)d->pyr.h[l] * d->pyr.w[l] > m) m = (long long)d->pyr.h[l] * d->pyr.w[l];
  return m;
}

// Per-level table of a pyramid launch.  Tiles enumerate (level, clip, tile row, tile column); levels past n are 1 x 1
// and start at the total.  xpos / ypos: first position of the level in the x / y pyramid buffers.
struct LevelTable {
  int n;
  int H[SFVOS_MAX_LEVELS], W[SFVOS_MAX_LEVELS], tiles_h[SFVOS_MAX_LEVELS], tiles_w[SFVOS_MAX_LEVELS];
  int tile_begin[SFVOS_MAX_LEVELS + 1];  // first tile of each level
  long long xpos[SFVOS_MAX_LEVELS], ypos[SFVOS_MAX_LEVELS];
};

// Tile rule: th x tw pixel tiles, or with th = 0 runs of tw consecutive positions of the flattened frame (tiles_h = 1).
// x_frames / y_frames: frames per clip of a level in the x / y buffers (1 for a frame-major ring).
// Returns the tiles over all levels and clips; tile_begin holds it only when it is below 2^31 (callers check).
static inline long long level_table(const sfvos_conv_desc* d, long long x_frames, long long y_frames, int th, int tw,
                                    LevelTable* t) {
  t->n = d->pyr.n_levels;
  long long tiles = 0, px = 0;
  for (int l = 0; l < SFVOS_MAX_LEVELS; ++l) {
    const bool live = l < t->n;
    const int H = live ? d->pyr.h[l] : 1, W = live ? d->pyr.w[l] : 1;
    t->H[l] = H; t->W[l] = W;
    t->tiles_h[l] = th ? ceil_div(H, th) : 1;
    t->tiles_w[l] = th ? ceil_div(W, tw) : ceil_div(H * W, tw);
    t->tile_begin[l] = (int)tiles;
    t->xpos[l] = d->batch * x_frames * px;
    t->ypos[l] = d->batch * y_frames * px;
    if (live) {
      tiles += (long long)d->batch * t->tiles_h[l] * t->tiles_w[l];
      px += (long long)H * W;
    }
  }
  t->tile_begin[SFVOS_MAX_LEVELS] = (int)tiles;
  return tiles;
}

// The 1-D launches keep their level fields inline (their argument layouts cannot embed a LevelTable): copy them.
static inline void copy_levels_1d(const LevelTable& t, int* n, int* HW, int* begin, long long* xpos, long long* ypos) {
  *n = t.n;
  for (int l = 0; l < SFVOS_MAX_LEVELS; ++l) {
    HW[l] = t.H[l] * t.W[l]; begin[l] = t.tile_begin[l]; xpos[l] = t.xpos[l]; ypos[l] = t.ypos[l];
  }
  begin[SFVOS_MAX_LEVELS] = t.tile_begin[SFVOS_MAX_LEVELS];
}

// The dedicated lateral / t1 kernels; diagnostic builds switch them off with SFVOS_NO_LATERAL_KERNEL.
static inline bool lateral_kernels_on() {
#ifdef SFVOS_DIAG
  if (getenv("SFVOS_NO_LATERAL_KERNEL")) return false;
#endif
  return true;
}

// Launch of a kernel with dynamic LDS: raises its LDS limit to lds_attr once per device (one LdsAttrOnce per kernel
// instance), launches it with lds bytes and checks the launch.
template <auto KERN, class A>
static int launch_lds(dim3 grid, dim3 block, int lds, int lds_attr, hipStream_t stream, const char* what, const A& a) {
  static LdsAttrOnce once;
  if (int rc = once.ensure((const void*)KERN, lds_attr, what)) return rc;
  hipLaunchKernelGGL(KERN, grid, block, lds, stream, a);
  return check_launch(what);
}

}  // namespace sfvos
