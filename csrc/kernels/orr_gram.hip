// ORR Gram, wide form: 129 ≤ dz = d + 2 ≤ 1024 columns, PolynomialFeatures(2) fused.
//
// G += Σ zzᵀ over the rows with a finite target, z = [x, (x_a·x_b per pair), 1, y]. The two
// kernels of dense_learners.hip end at 128 columns (gram_map_kernel: every wave holds every
// upper-triangle tile) or read each operand with a scalar global load and compute both
// triangles (gram_mfma_kernel). Here the columns are padded to 128-column panels and only the
// upper-triangle 128 × 128 macro-tiles (mi ≤ mj) are computed: M = MB(MB + 1)/2, MB = ⌈dz/128⌉.
//
// Work split. Grid = M macro-tiles × `splits` row ranges (M·splits ≈ the 256 CUs; a split is a
// whole number of 64-row chunks). A workgroup has four waves; wave w owns the 64 × 64 quadrant
// (w >> 1, w & 1) of the macro-tile: 2 × 2 tiles of v_mfma_f32_32x32x2_f32 (exact fp32
// products, as the normal equations need), 64 accumulator registers, 2 + 2 operands and four
// independent MFMAs per row pair. No accumulator is shared, so nothing is reduced across waves.
// On a diagonal macro-tile the lower-left quadrant is the transpose of the upper-right one: its
// wave stages and waits at the barriers but issues no MFMA and writes nothing.
//
// Staging. 64-row chunks, double-buffered in LDS; the next chunk's global loads sit in registers
// while this chunk computes (the idiom of gram_map_kernel). A thread owns one staged column and
// every RS-th row of the chunk, so what its column holds is decided once:
//   plain form: the block stages the 128 columns of panel mi and, off the diagonal, of panel mj
//               (row stride 257 floats: 2 × 64 × 257 × 4 B ≈ 129 KiB of LDS); a lane's four
//               operands are four LDS reads per row pair.
//   map form:   the staged row is the raw [x (d0), 1, y, 0] (d0 ≤ 61, ≤ 12 KiB); a lane keeps
//               the (fa, fb) entries of its column in its two row blocks and two column blocks
//               and forms z_c = s[fa]·s[fb] in the fetch: the expansion never reaches HBM.
// The `1` and `y` columns are synthesised at staging. A row with a NaN target, or past the
// split's range, is staged as zeros BY SELECTION: such a row's features may hold anything, NaN
// included (the contract of kmeans_seq.hip), and the fetch needs no per-row `valid` multiply.
// Each wave loads the chunk's 64 targets itself (lane = row) and ballots them into a mask, so
// validity costs no LDS traffic and no extra barrier.
//
// Flush. Every block stores its 128 × 128 partial (64 KiB) with plain stores to slot
// [split][macro-tile] of a workspace; orr_gram_reduce_kernel sums the splits in index order for
// every element with row ≤ col < dz, adds the sum to G[row][col] and G[col][row] (the solve
// kernels read the lower triangle) and entry (d, d) = Σ 1·1, the fitted-row count, to the fp64
// `cnt`. No atomics: G's increment is bit-symmetric and the same bits on every run.
#include "common.h"

namespace omldm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGwMinDz = 129, kGwMaxDz = 1024;
constexpr int kGwRC = 64;           // rows per staged chunk
constexpr int kGwTile = 128;        // macro-tile edge
constexpr int kGwSlot = 128 * 128;  // floats of one block's partial
constexpr int kGwBlocks = 256;      // M · splits aims at one block per CU
constexpr int kGwMapD0 = 61;        // map form: the staged raw row d0 + 3 ≤ 64 columns

struct GwPlan {
  int MB, M, splits, cps;  // panels, macro-tiles, row splits, 64-row chunks per split
};

inline GwPlan gw_plan(int B, int dz) {
  GwPlan p;
  p.MB = (dz + kGwTile - 1) / kGwTile;
  p.M = p.MB * (p.MB + 1) / 2;
  const long long nch = ((long long)B + kGwRC - 1) / kGwRC;
  long long s = kGwBlocks / p.M;
  if (s < 1) s = 1;
  if (s > nch) s = nch;
  p.cps = (int)((nch + s - 1) / s);
  p.splits = (int)((nch + p.cps - 1) / p.cps);  // every split holds at least one chunk
  return p;
}

// t-th upper-triangle macro-tile in row-major order → (mi, mj), mi ≤ mj < MB
__device__ __forceinline__ void gw_tile(int t, int MB, int& mi, int& mj) {
  mi = 0;
  while (t >= MB - mi) {
    t -= MB - mi;
    ++mi;
  }
  mj = mi + t;
}

// grid (M, splits), 256 threads; dynamic LDS 2 · 64 · LDW floats (LDW: 257, or (d0 + 3) | 1).
// MAP: x is the raw [B][d0] batch and `pairs` its degree-2 table; else x is [B][d0], npairs = 0.
template <bool MAP>
__global__ __launch_bounds__(256) void orr_gram_wide_kernel(
    const float* __restrict__ x, const float* __restrict__ y, int B, int d0,
    const int* __restrict__ pairs, int npairs, int MB, int cps, float* __restrict__ work) {
  constexpr int PW = MAP ? 64 : 128;  // staged columns a panel spreads over the threads
  constexpr int RS = 256 / PW;        // rows between a thread's staging slots
  constexpr int SL = kGwRC / RS;      // slots per thread and panel
  constexpr int NP = MAP ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, col = lane & 31;
  const int d = d0 + npairs;  // z = [mapped features (d), 1, y]
  int mi, mj;
  gw_tile(blockIdx.x, MB, mi, mj);
  const bool diag = mi == mj;
  const int np = (MAP || diag) ? 1 : 2;
  const int W = MAP ? d0 + 3 : 128 * np;  // staged columns of a row
  const int LDW = MAP ? (W | 1) : 257;    // odd stride: the half-waves' rows on different banks
  const long long r_begin = (long long)blockIdx.y * cps * kGwRC;
  const long long r_end = min((long long)B, r_begin + (long long)cps * kGwRC);  // > r_begin

  // ---- what this thread stages: column sc of each panel, rows wrow + RS·k of the chunk.
  // Raw column g of [x (d0), 1, y, 0…]: only the x columns (g < d0) change from chunk to chunk
  // and go through registers. The `1` and `y` entries of row r are written by thread r of wave
  // 0, and the zero columns (tile padding; the map form's ZERO entry) once, below.
  const int sc = tid & (PW - 1);
  const int wrow = __builtin_amdgcn_readfirstlane(tid / PW);  // wave-uniform
  uint32_t cx[NP];  // byte offset of the column in a row of x
  bool isx[NP];
  int o_one[NP], o_y[NP];  // staged columns of `1` and `y` in panel p (block-uniform), or −1
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int g0 = MAP ? 0 : (p == 0 ? mi : mj) * kGwTile, g = g0 + sc;
    isx[p] = g < d0;
    cx[p] = g < d0 ? 4u * g : 0u;
    const int w = MAP ? W : kGwTile;
    o_one[p] = d0 >= g0 && d0 < g0 + w ? p * kGwTile + d0 - g0 : -1;
    o_y[p] = d0 + 1 >= g0 && d0 + 1 < g0 + w ? p * kGwTile + d0 + 1 - g0 : -1;
    if (p < np && g >= d0 + 2 && sc < w)
      for (int r = wrow; r < 2 * kGwRC; r += RS) lds[(size_t)r * LDW + p * kGwTile + sc] = 0.f;
  }
  float xr[NP][SL];
  float yr = 0.f;
  auto load = [&](long long rc) {
    yr = y[min(rc + lane, r_end - 1)];  // first: store() needs it before the x values
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < np) {
        // a wave-uniform row base plus the lane's 32-bit column offset (the compiler still builds
        // an address pair per slot: profiles/round13/orr_gram.md)
#pragma unroll
        for (int k = 0; k < SL; ++k) {
          const long long r = min(rc + wrow + RS * k, r_end - 1);  // clamped: always in range
          xr[p][k] = *(const float*)((const char*)(x + (size_t)r * d0) + cx[p]);
        }
      }
  };
  // rc: the chunk that load() fetched. Every wave holds the chunk's targets (lane = row) and
  // ballots them here (so that load() waits on nothing): bit r = row r is trained on.
  auto store = [&](int buf, long long rc) {
    float* b = lds + (size_t)buf * kGwRC * LDW;
    const bool ok = rc + lane < r_end && !__builtin_isnan(yr);
    const unsigned long long mask = __ballot(ok) >> wrow;  // bit RS·k: this thread's k-th row
    if (wave == 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (p < np && o_one[p] >= 0) b[(size_t)lane * LDW + o_one[p]] = ok ? 1.f : 0.f;
        if (p < np && o_y[p] >= 0) b[(size_t)lane * LDW + o_y[p]] = ok ? yr : 0.f;
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < np && isx[p]) {
#pragma unroll
        for (int k = 0; k < SL; ++k)  // selected, never multiplied: the row may hold NaN
          b[(size_t)(wrow + RS * k) * LDW + p * kGwTile + sc] =
              (mask >> (RS * k)) & 1ull ? xr[p][k] : 0.f;
      }
  };

  // ---- this lane's operands: column `col` of row blocks i and column blocks j of the quadrant
  int fa[4], fb[4];  // [0, 1]: row blocks, [2, 3]: column blocks; plain form uses fa only
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lc = ((q < 2 ? wr : wc) * 2 + (q & 1)) * 32 + col;  // column inside the panel
    if (MAP) {
      const int c = (q < 2 ? mi : mj) * kGwTile + lc;
      const int ONE = d0, YC = d0 + 1, ZERO = d0 + 2;
      if (c < d0) {
        fa[q] = c;
        fb[q] = ONE;
      } else if (c < d) {
        fa[q] = min(max(pairs[2 * (c - d0)], 0), d0 - 1);
        fb[q] = min(max(pairs[2 * (c - d0) + 1], 0), d0 - 1);
      } else if (c == d) {
        fa[q] = fb[q] = ONE;
      } else if (c == d + 1) {
        fa[q] = YC;
        fb[q] = ONE;
      } else {
        fa[q] = fb[q] = ZERO;
      }
    } else {
      fa[q] = (q >= 2 && np == 2 ? kGwTile : 0) + lc;
      fb[q] = 0;
    }
  }
  const bool live = !(diag && wr > wc);  // the diagonal tile's lower-left quadrant is not needed

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load(r_begin);
  store(0, r_begin);
  __syncthreads();
  int buf = 0;
  for (long long rc = r_begin; rc < r_end; rc += kGwRC) {
    const bool more = rc + kGwRC < r_end;
    if (more) load(rc + kGwRC);  // in flight while this chunk computes
    if (live) {
      const float* xb = lds + (size_t)buf * kGwRC * LDW + (size_t)half * LDW;
      // the LDS reads of row pair kp + 1 are issued before the MFMAs of pair kp
      float ra[4], rb[4];
      auto issue = [&](int kp) {
        const float* xrow = xb + (size_t)(2 * kp) * LDW;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ra[q] = xrow[fa[q]];
          if (MAP) rb[q] = xrow[fb[q]];
        }
      };
      issue(0);
#pragma unroll 8
      for (int kp = 0; kp < kGwRC / 2; ++kp) {
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) z[q] = MAP ? ra[q] * rb[q] : ra[q];
        if (kp + 1 < kGwRC / 2) issue(kp + 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(z[i], z[2 + j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) store(buf ^ 1, rc + kGwRC);  // buffer buf ^ 1 was last read before the previous barrier
    __syncthreads();
    buf ^= 1;
  }
  if (!live) return;
  // C/D map (32x32): col = lane & 31, row = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5)
  float* slot = work + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kGwSlot;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = (wr * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        slot[lr * kGwTile + (wc * 2 + j) * 32 + col] = acc[i][j][r];
      }
}

// grid (M, 64), 256 threads: thread = one element of a macro-tile; the splits' partials are
// added in index order. Elements below the diagonal or past dz are never read (the diagonal
// tiles' lower-left quadrants are never written).
__global__ __launch_bounds__(256) void orr_gram_reduce_kernel(const float* __restrict__ work,
                                                              int MB, int splits, int dz,
                                                              float* __restrict__ G, int ld,
                                                              double* __restrict__ cnt) {
  int mi, mj;
  gw_tile(blockIdx.x, MB, mi, mj);
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int row = mi * kGwTile + (e >> 7), cl = mj * kGwTile + (e & 127);
  if (row > cl || cl >= dz) return;
  const float* p = work + (size_t)blockIdx.x * kGwSlot + e;
  const size_t step = (size_t)gridDim.x * kGwSlot;
  float s = 0.f;
#pragma unroll 8
  for (int k = 0; k < splits; ++k) s += p[k * step];
  G[(size_t)row * ld + cl] += s;
  if (row != cl) G[(size_t)cl * ld + row] += s;
  if (cnt && row == dz - 2 && cl == dz - 2) {
    // Σ 1·1 per split is that split's trained rows (exact in fp32: < 2^24); the total in fp64
    double c = 0.0;
    for (int k = 0; k < splits; ++k) c += (double)p[k * step];
    *cnt += c;
  }
}

}  // namespace omldm

using namespace omldm;

// Bytes of workspace omldm_gram_update_wide needs for B rows and dz columns; −1 outside
// 129 ≤ dz ≤ 1024 or for B < 1.
OMLDM_API long long omldm_gram_wide_ws_bytes(int B, int dz) {
  if (B < 1 || dz < kGwMinDz || dz > kGwMaxDz) return -1;
  const GwPlan p = gw_plan(B, dz);
  return (long long)p.M * p.splits * kGwSlot * 4;
}

// G[ld×ld] += zᵀz over rows with finite y, z = [x, 1, y] (pairs == nullptr, d0 = d) or
// z = [x, x_a·x_b for (a, b) in pairs, 1, y] (pairs: int32 [npairs][2], x the raw [B][d0]),
// dz = d0 + npairs + 2; cnt (may be null) += the number of those rows. `work`: 4-byte aligned,
// work_bytes ≥ omldm_gram_wide_ws_bytes(B, dz); what it holds on entry does not matter. Two
// launches in stream order. Returns a HIP error code, −1 for ld < dz, −2 outside 129 ≤ dz ≤
// 1024 (or a map of more than 61 raw features), −3 for a missing or short workspace or other bad
// arguments; nothing is launched on a negative return.
OMLDM_API int omldm_gram_update_wide(const float* x, const float* y, int B, int d0,
                                     const int* pairs, int npairs, float* G, int ld, double* cnt,
                                     float* work, long long work_bytes, void* stream) {
  if (B <= 0) return 0;
  if (d0 < 1 || npairs < 0 || (!pairs && npairs)) return -3;
  const long long dzl = (long long)d0 + npairs + 2;
  if (ld < dzl) return -1;
  if (dzl < kGwMinDz || dzl > kGwMaxDz || (pairs && d0 > kGwMapD0)) return -2;
  const int dz = (int)dzl;
  const GwPlan p = gw_plan(B, dz);
  if (!x || !y || !G || !work || ((uintptr_t)work & 3) ||
      work_bytes < (long long)p.M * p.splits * kGwSlot * 4)
    return -3;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.M, p.splits);
  if (pairs) {
    const size_t lds = (size_t)2 * kGwRC * ((d0 + 3) | 1) * 4;
    hipLaunchKernelGGL(orr_gram_wide_kernel<true>, grid, dim3(256), lds, st, x, y, B, d0, pairs,
                       npairs, p.MB, p.cps, work);
  } else {
    const size_t lds = (size_t)2 * kGwRC * 257 * 4;
    auto fn = orr_gram_wide_kernel<false>;
    const int e = check_dyn_lds((const void*)fn, lds);
    if (e) return e;
    hipLaunchKernelGGL(fn, grid, dim3(256), lds, st, x, y, B, d0, pairs, 0, p.MB, p.cps, work);
  }
  hipLaunchKernelGGL(orr_gram_reduce_kernel, dim3(p.M, kGwSlot / 256), dim3(256), 0, st, work,
                     p.MB, p.splits, dz, G, ld, cnt);
  return (int)hipGetLastError();
}
