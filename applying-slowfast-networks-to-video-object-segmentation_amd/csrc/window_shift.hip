// window_shift.hip -- the pre-BatchNorm buffer of a training window built from the previous window's (SlowFastWindows,
// reference code/helpers/model.py:316-374: consecutive centre frames under the same weights).  A first-layer conv's
// output frames depend only on the weights and the input frames, so the window one centre frame later holds the
// previous window's output frames s .. T-1 followed by s new ones:
//     out[l][b][t] = prev[l][b][t + s]          t <  T - s
//     out[l][b][t] = fresh[l][b][t - (T - s)]   t >= T - s
// The copy writes the partial (sum, sum of squares) rows of the values it stores in the same pass, in the layout
// sfvos_conv3d's statistics rows have (level-major [rows][2][C]), so the BatchNorm finalize that follows is unchanged.
// HBM-bound: 16-byte lane accesses, several loads in flight per lane; fixed-order sums (no atomics).
#include "elt_util.h"

namespace sfvos {

constexpr int WS_THREADS = 256;
constexpr int WS_RUN = 512;         // positions of one work unit; a run never crosses a frame
constexpr int WS_MAX_ROWS = 512;    // workgroups (= statistics rows) per level

struct ShiftTab {
  int n, T, s;
  int hw[SFVOS_MAX_LEVELS];          // positions per frame
  int rpf[SFVOS_MAX_LEVELS];         // runs per frame
  long long runs[SFVOS_MAX_LEVELS];  // runs of the level (B * T frames)
  long long pos[SFVOS_MAX_LEVELS];   // first position of the level in prev / out (B * T frames per level)
  long long fpos[SFVOS_MAX_LEVELS];  // ... in fresh (B * s frames per level)
  long long m_out, m_fresh;          // positions of prev / out and of fresh
  int blk_begin[SFVOS_MAX_LEVELS + 1];
};

static int make_shift_tab(const sfvos_pyramid* pyr, int B, int T, int s, int C, ShiftTab* t, const char* what) {
  SFVOS_REQUIRE(pyr != nullptr && pyr->n_levels >= 1 && pyr->n_levels <= SFVOS_MAX_LEVELS, "%s: bad pyramid", what);
  SFVOS_REQUIRE(B >= 1 && T >= 2 && s >= 1 && s < T, "%s: need B >= 1 and 1 <= s < T (B=%d T=%d s=%d)", what, B, T, s);
  SFVOS_REQUIRE(C > 0 && C % 32 == 0 && C <= 256, "%s: C must be a multiple of 32, <= 256 (got %d)", what, C);
  t->n = pyr->n_levels;
  t->T = T;
  t->s = s;
  long long pos = 0, fpos = 0;
  int blk = 0;
  for (int l = 0; l < SFVOS_MAX_LEVELS; ++l) {
    t->blk_begin[l] = blk;
    t->hw[l] = 0; t->rpf[l] = 0; t->runs[l] = 0; t->pos[l] = pos; t->fpos[l] = fpos;
    if (l >= t->n) continue;
    SFVOS_REQUIRE(pyr->h[l] >= 1 && pyr->w[l] >= 1, "%s: level %d is empty", what, l);
    const long long hw = (long long)pyr->h[l] * pyr->w[l];
    SFVOS_REQUIRE(hw <= (1ll << 30), "%s: level %d too large", what, l);
    t->hw[l] = (int)hw;
    t->rpf[l] = (int)ceil_div64(hw, WS_RUN);
    t->runs[l] = (long long)B * T * t->rpf[l];
    blk += (int)(t->runs[l] < WS_MAX_ROWS ? t->runs[l] : WS_MAX_ROWS);
    pos += (long long)B * T * hw;
    fpos += (long long)B * s * hw;
  }
  t->blk_begin[SFVOS_MAX_LEVELS] = blk;
  t->m_out = pos;
  t->m_fresh = fpos;
  return SFVOS_OK;
}

// grid = rows (level-major); a workgroup belongs to ONE level and owns a strided set of its runs.  Thread = (16-byte
// chunk of channels, row lane); each lane sums the positions it copies in ascending order, then the lanes are added in
// a fixed order through LDS -> one deterministic [2][C] row per workgroup.
template <int DT, bool STATS>
__global__ __launch_bounds__(WS_THREADS) void shift_frames_kernel(const char* __restrict__ prev,
                                                                  const char* __restrict__ fresh, char* __restrict__ out,
                                                                  ShiftTab tab, int C, int ld, float* __restrict__ part) {
  constexpr int CE = Elt<DT>::CE, ES = 16 / CE;
  int lvl = 0;
#pragma unroll
  for (int l = 1; l < SFVOS_MAX_LEVELS; ++l)
    if (l < tab.n && (int)blockIdx.x >= tab.blk_begin[l]) lvl = l;
  const int bi = blockIdx.x - tab.blk_begin[lvl], nblk = tab.blk_begin[lvl + 1] - tab.blk_begin[lvl];
  const int cpr = C / CE;               // chunks per position (<= 64)
  const int rl = WS_THREADS / cpr;      // row lanes
  const int ch = threadIdx.x % cpr, rowl = threadIdx.x / cpr;
  const int c = ch * CE;
  const int hw = tab.hw[lvl], rpf = tab.rpf[lvl], T = tab.T, s = tab.s;
  const long long row_bytes = (long long)ld * ES;
  float a0[CE], a1[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) a0[e] = a1[e] = 0.f;
  if (rowl < rl) {
    for (long long r = bi; r < tab.runs[lvl]; r += nblk) {
      const long long f = r / rpf;                   // frame b*T + t of the level
      const int j = (int)(r - f * rpf);
      const int b = (int)(f / T), t = (int)(f - (long long)b * T);
      const char* src = t < T - s ? prev + (tab.pos[lvl] + (f + s) * hw) * row_bytes
                                  : fresh + (tab.fpos[lvl] + ((long long)b * s + t - (T - s)) * hw) * row_bytes;
      char* dst = out + (tab.pos[lvl] + f * hw) * row_bytes;
      const int p_end = (j + 1) * WS_RUN < hw ? (j + 1) * WS_RUN : hw;
      constexpr int UN = 4;   // positions per lane and trip: every load is issued before the first store
      for (int p0 = j * WS_RUN + rowl; p0 < p_end; p0 += UN * rl) {
        u32x4 v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int p = p0 + u * rl;
          if (p < p_end) v[u] = *(const u32x4*)(src + p * row_bytes + c * ES);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int p = p0 + u * rl;
          if (p >= p_end) break;
          *(u32x4*)(dst + p * row_bytes + c * ES) = v[u];
          if (STATS) {
            float x[CE];
            unpack<DT>(v[u], x);
#pragma unroll
            for (int e = 0; e < CE; ++e) {
              a0[e] += x[e];
              a1[e] += x[e] * x[e];
            }
          }
        }
      }
    }
  }
  if (!STATS) return;
  __shared__ float red[2][WS_THREADS][8];
#pragma unroll
  for (int e = 0; e < CE; ++e) {
    red[0][threadIdx.x][e] = a0[e];
    red[1][threadIdx.x][e] = a1[e];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += WS_THREADS) {
    const int which = i / C, cc = i - which * C;
    const int chunk = cc / CE, e = cc - chunk * CE;
    float sum = 0.f;
    for (int k = 0; k < rl; ++k) sum += red[which][k * cpr + chunk][e];
    part[((long long)blockIdx.x * 2 + which) * C + cc] = sum;
  }
}

static bool overlaps(const void* a, long long a_bytes, const void* b, long long b_bytes) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace sfvos

using namespace sfvos;

extern "C" int sfvos_shift_frames_stat_rows(const sfvos_pyramid* pyr, int B, int T, int C, int* rows_per_level) {
  ShiftTab tab;
  // the row count does not depend on the shift: any valid s gives the same table
  if (make_shift_tab(pyr, B, T, 1, C, &tab, "shift_frames_stat_rows") != SFVOS_OK) return SFVOS_E_ARG;
  if (rows_per_level)
    for (int l = 0; l < tab.n; ++l) rows_per_level[l] = tab.blk_begin[l + 1] - tab.blk_begin[l];
  return tab.blk_begin[SFVOS_MAX_LEVELS];
}

extern "C" int sfvos_shift_frames(const void* prev, const void* fresh, void* out, int dtype, const sfvos_pyramid* pyr,
                                  int B, int T, int s, int C, int ld, float* stat_part, sfvos_stream_t stream) {
  ShiftTab tab;
  int rc = make_shift_tab(pyr, B, T, s, C, &tab, "shift_frames");
  if (rc) return rc;
  if ((rc = check_act("shift_frames", dtype, C, ld, ld))) return rc;
  SFVOS_REQUIRE(prev && fresh && out, "shift_frames: null buffer");
  SFVOS_REQUIRE(((uintptr_t)prev | (uintptr_t)fresh | (uintptr_t)out | (uintptr_t)stat_part) % 16 == 0,
                "shift_frames: buffers must be 16-byte aligned");
  const int es = elt_bytes(dtype);
  const long long b_out = tab.m_out * ld * es, b_fresh = tab.m_fresh * ld * es;
  SFVOS_REQUIRE(!overlaps(out, b_out, prev, b_out) && !overlaps(out, b_out, fresh, b_fresh),
                "shift_frames: out must not overlap prev or fresh (never in place)");
  auto launch = [&](auto dt, auto stats) {
    hipLaunchKernelGGL((shift_frames_kernel<dt, stats>), dim3((unsigned)tab.blk_begin[SFVOS_MAX_LEVELS]),
                       dim3(WS_THREADS), 0, (hipStream_t)stream, (const char*)prev, (const char*)fresh, (char*)out, tab,
                       C, ld, stat_part);
  };
  return launch_dt(dtype, "shift_frames", [&](auto dt) {
    if (stat_part)
      launch(dt, std::true_type());
    else
      launch(dt, std::false_type());
  });
}
