// Exact sequential round and batched predict of the linear family on numerical-only
// batches of 257-2048 columns (D = dn + bias): one Synchronous round of S virtual spokes
// with the semantics of omldm_cpu_linear_round (csrc/host/linear_cpu.cpp) at dc = 0. Up to
// 256 columns the dense round (linear_dense.hip) runs; behind PolynomialFeatures(2) the
// fused round (linear_poly.hip) trains on the unexpanded rows. Here the row itself is wide:
// it cannot be rebuilt from a few raw words, so whole rows go through LDS in chunks.
//
//  * One workgroup per (spoke, pipeline), W waves. Wave v owns the columns
//    [256v, 256v + 256), lane ℓ of it the columns 256v + ℓ + 64k, k < 4, and holds the
//    round-start weights w0 and its private delta d for them in registers for the whole
//    round: the model touches neither LDS nor HBM between the round's start and its end.
//  * W is instantiated at 2, 3, 4, 6 and 8; ⌈D / 256⌉ = 5 or 7 runs on the next one, whose
//    last wave owns no column and carries zeros. Every W would be 98 kernels for 70, and
//    rounding up to 2 / 4 / 8 (42 kernels) would give the widths of 513-768 and 1025-1536
//    columns up to twice the LDS traffic, prefetch and barrier width they need.
//  * A chunk is CR rows of 256·W + 1 words (odd stride) in LDS, the bias column as 1 and
//    the columns past D as 0: CR = 32 at W ≤ 4 (64-129 KB), 16 at W = 6 and 8 (96-128 KB),
//    so that one workgroup is resident per CU. What bounds CR is not LDS alone: the next
//    chunk waits in 4·CR registers of every thread (128 of the 512 a wave has at W ≤ 4, 64
//    of the 256 at W = 6 and 8), which is why W = 2 does not take 64 rows.
//  * All W·64 threads load the next chunk into registers one chunk ahead, row by row, each
//    row coalesced (thread t: columns t + 64W·k), with clamped addresses and no guard but
//    the launch-uniform one that skips the column blocks past dn. The chunk is laid out when
//    the current chunk ends; the columns at and past dn are written once, before the loop.
//  * Once per chunk, off the row chain: thread (q, i) sums slice q of row i's ‖x‖², the
//    columns [q·SL, q·SL + SL) in column order, SL = ⌈D / NS⌉, NS = 64W / CR, and lane i of
//    every wave adds the NS slices in slice order: the order is a function of D and W only.
//    Then the label, τ's denominator and cap, the shrink and Pegasos' T terms as in the dense
//    round (linear_step.h: row_terms), lane i of every wave for row i.
//  * Per row: 4 LDS reads fetched a row ahead and 4 fmas per lane, the fixed-order DPP wave
//    sum, one word per wave into the LDS slot of the row's parity, ONE workgroup barrier,
//    the W partials read back and added in wave order, the wave-uniform step math redundantly
//    in every wave (same operands, same order, contraction off: same bits), 4 update fmas.
//    The parity slot is what makes one barrier enough: a wave that writes row r + 2's partial
//    has passed row r + 1's barrier, which every wave reaches only after reading row r's.
//  * Margins are parked per row; wave 0 computes the chunk's loss / mistakes / squared error
//    from them once per chunk.
//  * Round end: every (pipeline, spoke) stores one workspace row (D deltas scaled by
//    σ·inv_p, the statistics) and round_fold_kernel (linear_step.h) adds the rows in spoke
//    order into the accumulator: no float atomics, no workgroup waits for another, a round
//    is bit-reproducible.
//
// The predict (omldm_linear_predict's form for dc = 0 past 256 features) is one wave per
// row, the lanes striding the columns so that a row is read coalesced, the model's D words
// staged in LDS once per block.
#include "common.h"
#include "linear_step.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

constexpr int kWideMin = 257;  // columns dn + bias: below, the dense round
constexpr int kWideMax = 2048;
constexpr int kWideWsw = kWideMax + 8;  // workspace row: D deltas, at 2048 the statistics
constexpr int kWideStat = kWideMax;

template <int W>
struct WideShape {
  static constexpr int kT = 64 * W;              // threads
  static constexpr int kRows = W <= 4 ? 32 : 16;  // rows per chunk
  static constexpr int kStride = 256 * W + 1;     // odd: the ‖x‖² pass reads a row per lane
  static constexpr int kSlices = kT / kRows;      // ‖x‖² slices of a row
  // the waves' partials by row parity [2][8], the margins [kRows], the slices [kT], the rows
  static constexpr int kWords = 16 + kRows + kT + kRows * kStride;
};

// Rows [t0, t0 + CR) of the spoke into registers as raw bits, thread tid the columns
// tid + T·k of every row, with the label of row t0 + lane. A row at or past t1 reads row
// t1 − 1 and a column at or past dn column dn − 1, so every address is inside the batch; a
// column block that starts at or past dn (k ≥ kl, the same for every thread) is not loaded.
// No select or conversion on the loaded values: the loads stay in flight until the chunk is
// laid out in LDS.
template <int W, bool NBF>
__device__ __forceinline__ void wide_load(const void* __restrict__ num, const void* __restrict__ y,
                                          int y_i8, long long t0, long long t1, int dn, int kl,
                                          int tid, unsigned (&x)[WideShape<W>::kRows][4],
                                          unsigned& yraw) {
  constexpr int T = WideShape<W>::kT, CR = WideShape<W>::kRows;
#pragma unroll
  for (int r = 0; r < CR; ++r) {
    const long long t = t0 + r < t1 ? t0 + r : t1 - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = tid + T * k;
      const size_t i = (size_t)t * dn + (j < dn ? j : dn - 1);
      if (k < kl)
        x[r][k] = NBF ? (unsigned)static_cast<const unsigned short*>(num)[i]
                      : static_cast<const unsigned*>(num)[i];
    }
  }
  const int lane = tid & 63;
  const long long t = t0 + lane < t1 ? t0 + lane : t1 - 1;
  if (y_i8)
    yraw = (unsigned)(int)static_cast<const signed char*>(y)[t];
  else
    yraw = static_cast<const unsigned*>(y)[t];
}

template <int W, int RULE, bool SHR, bool NBF>
__global__ __launch_bounds__(W * 64) void wide_round_kernel(
    DensePipes P, const void* __restrict__ num, int dn, const void* __restrict__ y, int y_i8,
    int B, int R, int S, int dim, float* __restrict__ ws, int variant, int bias, int w_bf16,
    float inv_p) {
  constexpr int T = WideShape<W>::kT, CR = WideShape<W>::kRows, ST = WideShape<W>::kStride;
  constexpr int NS = WideShape<W>::kSlices;
  extern __shared__ __attribute__((aligned(16))) float wide_sm[];
  float* part = wide_sm;   // [2][8]
  float* ms = part + 16;   // the chunk's margins, row i at i
  float* pns = ms + CR;    // [NS][CR]: the ‖x‖² slices
  float* xs = pns + T;     // [CR][ST]
  const int s = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const long long a = (long long)s * R;
  if (a >= B) return;  // an idle spoke is no worker of the round
  const long long b = a + R < (long long)B ? a + R : (long long)B;
  const int nrows = (int)(b - a);
  const int D = dn + (bias ? 1 : 0);
  const int kl = (dn + T - 1) / T;      // column blocks of T with a loaded column
  const int SL = (D + NS - 1) / NS;     // ‖x‖² slice of a thread: NS·SL ≥ D
  const float C = P.C[m], eps = P.eps[m], lr = P.lr[m], lam = P.lam[m], tbase = P.tbase[m];
  const float shr = RULE == kLogistic ? 1.f - lr * lam : 1.f - lam;

  // the columns no chunk brings: the bias column 1, the rest 0; the partials
#pragma unroll 1
  for (int r = 0; r < CR; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = tid + T * k;
      if (j >= dn) xs[r * ST + j] = (j == dn && j < D) ? 1.f : 0.f;
    }
  if (tid < 16) part[tid] = 0.f;

  // this lane's 4 columns: their round-start weights and deltas
  float w0[4], d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = 256 * wv + lane + 64 * k;
    const int slot = j < dn ? j : dim - 1;
    float v = 0.f;
    if (j < D)
      v = w_bf16 ? to_f(static_cast<const __hip_bfloat16*>(P.w[m])[slot])
                 : static_cast<const float*>(P.w[m])[slot];
    w0[k] = v;
    d[k] = 0.f;
  }

  float sigma = 1.f, loss_l = 0.f, nex_l = 0.f, mist_l = 0.f, sqe_l = 0.f;  // wave 0's lanes
  unsigned xn[CR][4], yn;
  wide_load<W, NBF>(num, y, y_i8, a, b, dn, kl, tid, xn, yn);

  const float* xcol = xs + 256 * wv + lane;  // this lane's columns of row 0
  const int nchunks = (nrows + CR - 1) / CR;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int nr = nrows - ch * CR < CR ? nrows - ch * CR : CR;
#pragma unroll
    for (int r = 0; r < CR; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = tid + T * k;
        if (k < kl && j < dn)
          xs[r * ST + j] = __builtin_bit_cast(float, NBF ? xn[r][k] << 16 : xn[r][k]);
      }
    const long long t0 = a + (long long)ch * CR;
    const float yl = y_i8 ? (float)(int)yn : __builtin_bit_cast(float, yn);
    const float yv = (lane < CR && t0 + lane < b) ? yl : __builtin_nanf("");
    __syncthreads();
    // the next chunk's rows, in flight while this one runs (past the last chunk: row b − 1)
    wide_load<W, NBF>(num, y, y_i8, t0 + CR, b, dn, kl, tid, xn, yn);

    // lane i of every wave holds row i's terms: what the row's step needs besides the model
    const bool skip = yv != yv;  // unlabeled, past the spoke's last row, or no row's lane
    const float ys = skip ? 0.f : yv;
    float pn = 0.f;
    if (RULE == kHinge || RULE == kEps) {
      const int i = tid % CR, q = tid / CR;
      const float* xrow = xs + i * ST;
      const int j1 = q * SL + SL < D ? q * SL + SL : D;
      float ps = 0.f;
#pragma unroll 4
      for (int j = q * SL; j < j1; ++j) ps += xrow[j] * xrow[j];
      pns[q * CR + i] = ps;
      __syncthreads();
      const int li = lane < CR ? lane : 0;
      pn = pns[li];
#pragma unroll
      for (int v = 1; v < NS; ++v) pn += pns[v * CR + li];
    }
    float capv, denv, shv, cyv;
    row_terms<RULE>(skip, ys, pn, tbase + (float)(ch * CR + lane), variant, C, lam, shr, capv,
                    denv, shv, cyv);

    float x[4], xq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = xcol[64 * k];  // row 0
    for (int r = 0; r < nr; ++r) {
      float pm = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) pm = __builtin_fmaf(x[k], w0[k] + d[k], pm);
      const float pw = wave_sum_last(pm);
      if (lane == 0) part[(r & 1) * 8 + wv] = pw;
      // the next row belongs to the batch, not the model: fetched while the waves meet
      // (past the chunk's last row: row CR − 1 again, unused)
      const float* xnext = xcol + (r + 1 < CR ? r + 1 : CR - 1) * ST;
#pragma unroll
      for (int k = 0; k < 4; ++k) xq[k] = xnext[64 * k];
      __syncthreads();
      const float4 pa = *reinterpret_cast<const float4*>(part + (r & 1) * 8);
      float tot = pa.x + pa.y;
      if (W > 2) tot += pa.z;
      if (W > 3) tot += pa.w;
      if (W > 4) {
        const float4 pb = *reinterpret_cast<const float4*>(part + (r & 1) * 8 + 4);
        tot += pb.x;
        tot += pb.y;
        if (W > 6) tot += pb.z;
        if (W > 7) tot += pb.w;
      }
      const float mg = sigma * tot;
      if (tid == 0) ms[r] = mg;
      const float yt = readlane_f(ys, r);
      const float c = step_coef<RULE>(yt, mg, readlane_f(capv, r), readlane_f(denv, r),
                                      readlane_f(cyv, r), eps, lr);
      float cv = c;
      if (SHR) {
        sigma *= readlane_f(shv, r);
        cv = c != 0.f ? c / sigma : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        d[k] = __builtin_fmaf(cv, x[k], d[k]);
        x[k] = xq[k];
      }
    }

    // the chunk's statistics from the parked margins, lane i of wave 0 for row i
    __syncthreads();
    if (wv == 0 && !skip) {
      nex_l += 1.f;
      row_stats<RULE>(yv, ms[lane], eps, loss_l, mist_l, sqe_l);
    }
    __syncthreads();  // before the next chunk is laid out over this one
  }

  const float scale = sigma * inv_p;
  float* wrow = ws + ((size_t)m * S + s) * kWideWsw;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = 256 * wv + lane + 64 * k;
    if (j < D) wrow[j] = d[k] * scale;
  }
  if (wv == 0) {
    const float loss_sum = wave_sum(loss_l), nex = wave_sum(nex_l), mist = wave_sum(mist_l),
                sqe = wave_sum(sqe_l);
    if (lane == 0) {
      wrow[kWideStat + 0] = loss_sum;
      wrow[kWideStat + 1] = nex;
      wrow[kWideStat + 2] = mist;
      wrow[kWideStat + 3] = sqe;
      wrow[kWideStat + 4] = sigma;
      wrow[kWideStat + 5] = 0.f;
      wrow[kWideStat + 6] = scale;
    }
  }
}

struct WideArgs {
  const void* num;
  const void* y;
  float* ws;
  int dn, y_i8, B, R, S, dim, variant, bias, w_bf16, num_bf16;
  float inv_p;
};

template <int W, int RULE, bool SHR, bool NBF>
int launch_wide_t(dim3 grid, hipStream_t st, const DensePipes& P, const WideArgs& A) {
  constexpr size_t lds = WideShape<W>::kWords * sizeof(float);
  static_assert(lds <= 160 * 1024, "one workgroup's chunk fits a CU's LDS");
  if (int e = check_dyn_lds((const void*)wide_round_kernel<W, RULE, SHR, NBF>, lds)) return e;
  hipLaunchKernelGGL((wide_round_kernel<W, RULE, SHR, NBF>), grid, dim3(W * 64), lds, st, P, A.num,
                     A.dn, A.y, A.y_i8, A.B, A.R, A.S, A.dim, A.ws, A.variant, A.bias, A.w_bf16,
                     A.inv_p);
  return (int)hipGetLastError();
}

template <int W, int RULE, bool SHR>
int launch_wide(dim3 grid, hipStream_t st, const DensePipes& P, const WideArgs& A) {
  return A.num_bf16 ? launch_wide_t<W, RULE, SHR, true>(grid, st, P, A)
                    : launch_wide_t<W, RULE, SHR, false>(grid, st, P, A);
}

template <int W>
int dispatch_wide(int rule, int shr, dim3 grid, hipStream_t st, const DensePipes& P,
                  const WideArgs& A) {
  if (rule == kPegasos) return launch_wide<W, kPegasos, true>(grid, st, P, A);
  if (rule == kHinge)
    return shr ? launch_wide<W, kHinge, true>(grid, st, P, A)
               : launch_wide<W, kHinge, false>(grid, st, P, A);
  if (rule == kEps)
    return shr ? launch_wide<W, kEps, true>(grid, st, P, A)
               : launch_wide<W, kEps, false>(grid, st, P, A);
  return shr ? launch_wide<W, kLogistic, true>(grid, st, P, A)
             : launch_wide<W, kLogistic, false>(grid, st, P, A);
}

// ------------------------------------------------------------------ predict
constexpr int kPredWaves = 4;  // rows in flight per block
constexpr int kPredU = 8;      // columns of a row a lane has in flight

// One wave per row, M stacked models (w + m·wstride) → out[t·M + m]: the model's dn
// columns (and its bias, slot dim − 1) are staged as fp32 in LDS once per block; a row is read
// coalesced, lane ℓ the columns ℓ + 64k, kPredU of them in flight.
template <typename NumT, typename WT>
__global__ __launch_bounds__(kPredWaves * 64) void wide_predict_kernel(
    const WT* __restrict__ w, long long wstride, int M, const NumT* __restrict__ num, int dn,
    int B, int dim, int bias, const float* __restrict__ wscale, float* __restrict__ out) {
  __shared__ float wl[kWideMax];
  const int tid = threadIdx.x, lane = tid & 63, m = blockIdx.y;
  const WT* wm = w + (size_t)m * wstride;
  for (int j = tid; j < dn; j += kPredWaves * 64) wl[j] = to_f(wm[j]);
  const float wb = bias ? to_f(wm[dim - 1]) : 0.f;
  const float sc = wscale ? wscale[m] : 1.f;
  __syncthreads();
  const int nwaves = gridDim.x * kPredWaves;
  for (int t = blockIdx.x * kPredWaves + (tid >> 6); t < B; t += nwaves) {
    const NumT* row = num + (size_t)t * dn;
    float acc = lane == 0 ? wb : 0.f;
    for (int j0 = lane; j0 < dn; j0 += 64 * kPredU) {
      float x[kPredU];
#pragma unroll
      for (int u = 0; u < kPredU; ++u) {
        const int j = j0 + 64 * u;
        x[u] = to_f(row[j < dn ? j : dn - 1]);
      }
#pragma unroll
      for (int u = 0; u < kPredU; ++u) {
        const int j = j0 + 64 * u;
        acc = __builtin_fmaf(j < dn ? x[u] : 0.f, wl[j < dn ? j : 0], acc);
      }
    }
    acc = wave_sum_last(acc);
    if (lane == 0) out[(size_t)t * M + m] = acc * sc;
  }
}

template <typename NumT, typename WT>
int launch_wide_predict(const void* w, long long wstride, int M, const void* num, int dn, int B,
                        int dim, int bias, const float* wscale, float* out, hipStream_t st) {
  int blocks = (B + kPredWaves - 1) / kPredWaves;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL((wide_predict_kernel<NumT, WT>), dim3(blocks, M), dim3(kPredWaves * 64), 0,
                     st, (const WT*)w, wstride, M, (const NumT*)num, dn, B, dim, bias, wscale,
                     out);
  return (int)hipGetLastError();
}

}  // namespace

// omldm_linear_predict's form for dc = 0 and 256 < dn + bias ≤ 2048 (linear_spoke.hip calls
// it; its arguments are that entry point's).
int linear_wide_predict(const void* w, int w_bf16, long long wstride, int M, const void* num,
                        int num_bf16, int dn, int B, int dim, int bias, const float* wscale,
                        float* out, hipStream_t st) {
  const int D = dn + (bias ? 1 : 0);
  if (D < kWideMin || D > kWideMax || dn > dim - (bias ? 1 : 0) || M > 65535) return -2;
  if (num_bf16) {
    if (w_bf16)
      return launch_wide_predict<__hip_bfloat16, __hip_bfloat16>(w, wstride, M, num, dn, B, dim,
                                                                 bias, wscale, out, st);
    return launch_wide_predict<__hip_bfloat16, float>(w, wstride, M, num, dn, B, dim, bias,
                                                      wscale, out, st);
  }
  if (w_bf16)
    return launch_wide_predict<float, __hip_bfloat16>(w, wstride, M, num, dn, B, dim, bias, wscale,
                                                      out, st);
  return launch_wide_predict<float, float>(w, wstride, M, num, dn, B, dim, bias, wscale, out, st);
}

}  // namespace omldm

using namespace omldm;

OMLDM_API int omldm_linear_wide_max() { return kWideMax; }

// Floats of workspace a launch of M pipelines × S spokes needs.
OMLDM_API long long omldm_linear_wide_ws_words(int M, int S) {
  return (long long)(M > 0 ? M : 0) * (S > 0 ? S : 0) * kWideWsw;
}

// One Synchronous round of M pipelines (1 ≤ M ≤ 16) on one batch without categorical
// columns and 256 < dn + bias ≤ 2048: num is [B, dn] (contiguous), the model's columns are
// at slots [0, dn) and the bias at dim − 1. The arguments are omldm_linear_dense_round's.
// Returns a HIP error code, or < 0 for a shape it does not take (nothing is launched).
OMLDM_API int omldm_linear_wide_round(int M, const void* const* w, float* const* dacc,
                                      double* const* cum, float* const* stats, const float* C,
                                      const float* eps, const float* lr, const float* lam,
                                      const float* tbase, int w_bf16, const void* num,
                                      int num_bf16, int dn, const void* y, int y_i8, int B, int R,
                                      int S, int dim, float* ws, int rule, int variant, int bias,
                                      int shr, float inv_p, void* stream) {
  const int D = dn + (bias ? 1 : 0);
  if (M < 1 || M > kDenseMaxM || !w || !dacc || !C || !eps || !lr || !lam || !tbase) return -1;
  if (dn < 1 || D < kWideMin || D > kWideMax || D > dim) return -2;
  if (B < 0 || R < 1 || S < 1 || !ws || !y || !num) return -3;
  if (rule < kHinge || rule > kPegasos || variant < 0 || variant > 2 || shr < 0 || shr > 2) return -4;
  if ((rule == kPegasos) != (shr == 2)) return -4;
  if (y_i8 && rule == kEps) return -5;
  DensePipes P;
  DenseOut O;
  for (int m = 0; m < kDenseMaxM; ++m) {
    const int i = m < M ? m : 0;
    if (!w[i] || !dacc[i]) return -1;
    if (rule == kPegasos && !(lam[i] > 0.f && tbase[i] >= 2.f)) return -6;
    P.w[m] = w[i];
    P.C[m] = C[i];
    P.eps[m] = eps[i];
    P.lr[m] = lr[i];
    P.lam[m] = lam[i];
    P.tbase[m] = tbase[i];
    O.dacc[m] = dacc[i];
    O.cum[m] = cum ? cum[i] : nullptr;
    O.stats[m] = stats ? stats[i] : nullptr;
  }
  if (B == 0) return 0;
  const long long sact = ((long long)B + R - 1) / R;
  const int S_act = sact < S ? (int)sact : S;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(S_act, M);
  const WideArgs A{num, y, ws, dn, y_i8, B, R, S, dim, variant, bias, w_bf16, num_bf16, inv_p};
  int e;
  if (D <= 512)
    e = dispatch_wide<2>(rule, shr, grid, st, P, A);
  else if (D <= 768)
    e = dispatch_wide<3>(rule, shr, grid, st, P, A);
  else if (D <= 1024)
    e = dispatch_wide<4>(rule, shr, grid, st, P, A);
  else if (D <= 1536)
    e = dispatch_wide<6>(rule, shr, grid, st, P, A);
  else
    e = dispatch_wide<8>(rule, shr, grid, st, P, A);
  if (e) return e;
  hipLaunchKernelGGL(round_fold_kernel<kWideWsw>, dim3(M), dim3(256), 0, st, O, ws, S, S_act, dn, D,
                     dim, inv_p);
  return (int)hipGetLastError();
}
