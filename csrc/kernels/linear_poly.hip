// Exact sequential round of the linear family behind PolynomialFeatures(2), for numerical-
// only batches whose expansion is 257-1024 columns: one Synchronous round of S virtual
// spokes with the semantics of omldm_cpu_linear_round (csrc/host/linear_cpu.cpp) at dc = 0
// on the batch [x, x_a·x_b for (a, b) in pairs] (+ the bias column), which is never
// materialised. Up to 256 columns the dense round (linear_dense.hip) runs on the expanded
// batch.
//
//  * One workgroup per (spoke, pipeline), W = ⌈D / 256⌉ waves (2, 3 or 4). Wave v owns the
//    columns [256v, 256v + 256), lane ℓ of it the columns 256v + ℓ + 64k, k < 4, and holds
//    the round-start weights w0 and its private delta d for them in registers for the whole
//    round: the model touches neither LDS nor HBM between the round's start and its end.
//  * Only the raw rows go through LDS: 64 rows of d0 + 2 words (odd stride), the two extra
//    words ONE = 1 and ZERO = 0. A column is a pair of word offsets (a, b) into the row,
//    fixed before the row loop: linear column j = (j, ONE), a product = (a, b), the bias =
//    (ONE, ONE), padding past D = (ZERO, ZERO). Its value is row[a]·row[b] without a branch:
//    x·1 is exact and a product is the one fp32 rounding omldm_poly makes, so the kernel
//    sees the oracle's batch bit for bit.
//  * A chunk (64 raw rows: one contiguous span of the batch) is loaded coalesced by all
//    W·64 threads into registers one chunk ahead, with clamped addresses and no guards,
//    and laid out when the current chunk ends.
//  * Once per chunk, off the row chain: thread (v, i) sums slice v of row i's ‖x‖² — the
//    columns [v·SL, v·SL + SL), SL = 4·⌈D / 4W⌉, in column order — and lane i of every wave
//    adds the W slices in slice order; then the label, τ's denominator and cap, the shrink
//    and Pegasos' T terms as in the dense round (linear_step.h: row_terms). The order is a
//    function of D alone. Every wave holds every row's terms (lane i: row i).
//  * Per row: 4 fmas per lane on products formed a row ahead, the fixed-order DPP wave sum,
//    one word per wave into the LDS slot of the row's parity, ONE workgroup barrier, the W
//    partials read back and added in wave order, the wave-uniform step math redundantly in
//    every wave (same operands, same order, contraction off: same bits), 4 update fmas.
//    The parity slot is what makes one barrier enough: a wave that writes row r + 2's
//    partial has passed row r + 1's barrier, which every wave reaches only after reading
//    row r's.
//  * Margins are parked per row; wave 0 computes the chunk's loss / mistakes / squared
//    error from them once per chunk.
//  * Round end: every (pipeline, spoke) stores one workspace row (D scaled deltas, the
//    statistics) and round_fold_kernel (linear_step.h) adds the rows in spoke order into the
//    accumulator: no float atomics, no workgroup waits for another, a round is
//    bit-reproducible.
#include "common.h"
#include "linear_step.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

constexpr int kPolyMin = 257;     // columns d0 + npairs + bias: below, the dense round
constexpr int kPolyMax = 1024;
constexpr int kPolyRawMax = 45;   // raw columns: 64 rows × 47 words of LDS, and ...
constexpr int kPolyRows = 64;     // rows per chunk
constexpr int kPolyStride = kPolyRawMax + 2;
constexpr int kPolyWsw = kPolyMax + 8;  // workspace row: D deltas, at 1024 the statistics
constexpr int kPolyStat = kPolyMax;

// ... a chunk's 64·d0 words in NL registers of each of the W·64 threads: d0 ≤ 30 / 39 / 45
// at W = 2 / 3 / 4 (the full degree-2 table of a width with that W has d0 ≤ 30 / 37 / 43)
template <int W>
struct PolyShape {
  static constexpr int kNL = W == 2 ? 15 : W == 3 ? 13 : 12;
  static constexpr int kRawMax = kNL * W < kPolyRawMax ? kNL * W : kPolyRawMax;
};

// Column j as two word offsets into the LDS row.
__device__ __forceinline__ void poly_column(int j, int d0, int npairs, int D,
                                            const int* __restrict__ pairs, int& ca, int& cb) {
  const int one = d0, zero = d0 + 1;
  if (j < d0) {
    ca = j;
    cb = one;
  } else if (j < d0 + npairs) {
    const int a = pairs[2 * (j - d0)], b = pairs[2 * (j - d0) + 1];
    ca = a < 0 ? 0 : (a < d0 ? a : d0 - 1);  // (a pair outside the row reads inside it)
    cb = b < 0 ? 0 : (b < d0 ? b : d0 - 1);
  } else {
    ca = cb = j < D ? one : zero;
  }
}

// Thread tid's words tid + n·T of the 64·d0-word span that starts at row t0, as raw bits,
// with the label of row t0 + lane. A word at or past row t1 reads the batch's word
// t1·d0 − 1 and a label at or past t1 the label t1 − 1, so every address is inside the
// batch (NL·T ≥ 64·d0: the words past the span are loaded too and dropped). No guard, and no
// select or conversion on the loaded values: the loads stay in flight until the chunk is
// laid out in LDS.
template <int T, int NL, bool NBF>
__device__ __forceinline__ void poly_load(const void* __restrict__ num, const void* __restrict__ y,
                                          int y_i8, long long t0, long long t1, int d0, int tid,
                                          unsigned (&x)[NL], unsigned& yraw) {
  const long long g0 = t0 * d0 + tid, gmax = t1 * d0 - 1;
#pragma unroll
  for (int n = 0; n < NL; ++n) {
    const long long g = g0 + n * T < gmax ? g0 + n * T : gmax;
    x[n] = NBF ? (unsigned)static_cast<const unsigned short*>(num)[g]
               : static_cast<const unsigned*>(num)[g];
  }
  const int lane = tid & 63;
  const long long t = t0 + lane < t1 ? t0 + lane : t1 - 1;
  if (y_i8)
    yraw = (unsigned)(int)static_cast<const signed char*>(y)[t];
  else
    yraw = static_cast<const unsigned*>(y)[t];
}

template <int W, int RULE, bool SHR, bool NBF>
__global__ __launch_bounds__(W * 64) void poly_round_kernel(
    DensePipes P, const void* __restrict__ num, int d0, const int* __restrict__ pairs, int npairs,
    const void* __restrict__ y, int y_i8, int B, int R, int S, int dim, float* __restrict__ ws,
    int variant, int bias, int w_bf16, float inv_p) {
  constexpr int T = W * 64;
  constexpr int NL = PolyShape<W>::kNL;
  constexpr int CR = kPolyRows;
  __shared__ float xs[CR * kPolyStride + 1];  // (+ a dump word for the span's tail)
  __shared__ __attribute__((aligned(16))) unsigned desc[W * 256];  // column j: a | b << 16
  __shared__ float pns[W][CR];  // the ‖x‖² slices
  __shared__ float ms[CR];      // the chunk's margins, row i at i
  __shared__ __attribute__((aligned(16))) float part[2][4];  // the waves' partials, by row parity
  const int s = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const long long a = (long long)s * R;
  if (a >= B) return;  // an idle spoke is no worker of the round
  const long long b = a + R < (long long)B ? a + R : (long long)B;
  const int nrows = (int)(b - a);
  const int D = d0 + npairs + (bias ? 1 : 0);
  const int ST = (d0 + 2) | 1;
  const int SL = 4 * ((D + 4 * W - 1) / (4 * W));  // ‖x‖² slice of a thread: W·SL ≥ D
  const float C = P.C[m], eps = P.eps[m], lr = P.lr[m], lam = P.lam[m], tbase = P.tbase[m];
  const float shr = RULE == kLogistic ? 1.f - lr * lam : 1.f - lam;

  // the column table (the ‖x‖² pass reads it), the rows' ONE and ZERO words, the partials
  for (int j = tid; j < W * 256; j += T) {
    int ca, cb;
    poly_column(j, d0, npairs, D, pairs, ca, cb);
    desc[j] = (unsigned)ca | (unsigned)cb << 16;
  }
  if (tid < CR) {
    xs[tid * ST + d0] = 1.f;
    xs[tid * ST + d0 + 1] = 0.f;
  }
  if (tid < 8) part[tid >> 2][tid & 3] = 0.f;

  // this lane's 4 columns: their offsets, round-start weights and deltas
  int oa[4], ob[4];
  float w0[4], d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = 256 * wv + lane + 64 * k;
    poly_column(j, d0, npairs, D, pairs, oa[k], ob[k]);
    const int slot = j < d0 + npairs ? j : dim - 1;
    float v = 0.f;
    if (j < D)
      v = w_bf16 ? to_f(static_cast<const __hip_bfloat16*>(P.w[m])[slot])
                 : static_cast<const float*>(P.w[m])[slot];
    w0[k] = v;
    d[k] = 0.f;
  }
  // where this thread's loaded words go in LDS (the same for every chunk)
  int dst[NL];
#pragma unroll
  for (int n = 0; n < NL; ++n) {
    const int e = tid + n * T, r = e / d0;
    dst[n] = r < CR ? r * ST + (e - r * d0) : CR * kPolyStride;
  }

  float sigma = 1.f, loss_l = 0.f, nex_l = 0.f, mist_l = 0.f, sqe_l = 0.f;  // wave 0's lanes
  unsigned xn[NL], yn;
  poly_load<T, NL, NBF>(num, y, y_i8, a, b, d0, tid, xn, yn);

  const int nchunks = (nrows + CR - 1) / CR;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int nr = nrows - ch * CR < CR ? nrows - ch * CR : CR;
#pragma unroll
    for (int n = 0; n < NL; ++n)
      xs[dst[n]] = __builtin_bit_cast(float, NBF ? xn[n] << 16 : xn[n]);
    const long long t0 = a + (long long)ch * CR;
    const float yl = y_i8 ? (float)(int)yn : __builtin_bit_cast(float, yn);
    const float yv = t0 + lane < b ? yl : __builtin_nanf("");
    __syncthreads();
    // the next chunk's rows, in flight while this one runs (past the last chunk: word b·d0 − 1)
    poly_load<T, NL, NBF>(num, y, y_i8, t0 + CR, b, d0, tid, xn, yn);

    // lane i of every wave holds row i's terms: what the row's step needs besides the model
    const bool skip = yv != yv;  // unlabeled, or past the spoke's last row
    const float ys = skip ? 0.f : yv;
    const float* xrow = xs + lane * ST;
    float pn = 0.f;
    if (RULE == kHinge || RULE == kEps) {
      float ps = 0.f;
      for (int j = wv * SL; j < wv * SL + SL; j += 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(desc + j);
        const float p0 = xrow[q.x & 0xFFFF] * xrow[q.x >> 16];
        const float p1 = xrow[q.y & 0xFFFF] * xrow[q.y >> 16];
        const float p2 = xrow[q.z & 0xFFFF] * xrow[q.z >> 16];
        const float p3 = xrow[q.w & 0xFFFF] * xrow[q.w >> 16];
        ps += p0 * p0;
        ps += p1 * p1;
        ps += p2 * p2;
        ps += p3 * p3;
      }
      pns[wv][lane] = ps;
      __syncthreads();
      pn = pns[0][lane];
#pragma unroll
      for (int v = 1; v < W; ++v) pn += pns[v][lane];
    }
    float capv, denv, shv, cyv;
    row_terms<RULE>(skip, ys, pn, tbase + (float)(ch * CR + lane), variant, C, lam, shr, capv,
                    denv, shv, cyv);

    float x[4], xq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = xs[oa[k]] * xs[ob[k]];  // row 0's products
    for (int r = 0; r < nr; ++r) {
      float pm = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) pm = __builtin_fmaf(x[k], w0[k] + d[k], pm);
      const float pw = wave_sum_last(pm);
      if (lane == 0) part[r & 1][wv] = pw;
      // the next row's products belong to the row, not the model: formed while the waves
      // meet (past the chunk's last row: row 63 again, unused)
      const float* xnext = xs + (r + 1 < CR ? r + 1 : CR - 1) * ST;
#pragma unroll
      for (int k = 0; k < 4; ++k) xq[k] = xnext[oa[k]] * xnext[ob[k]];
      __syncthreads();
      const float4 pp = *reinterpret_cast<const float4*>(part[r & 1]);
      float tot = pp.x + pp.y;
      if (W > 2) tot += pp.z;
      if (W > 3) tot += pp.w;
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
  float* wrow = ws + ((size_t)m * S + s) * kPolyWsw;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = 256 * wv + lane + 64 * k;
    if (j < D) wrow[j] = d[k] * scale;
  }
  if (wv == 0) {
    const float loss_sum = wave_sum(loss_l), nex = wave_sum(nex_l), mist = wave_sum(mist_l),
                sqe = wave_sum(sqe_l);
    if (lane == 0) {
      wrow[kPolyStat + 0] = loss_sum;
      wrow[kPolyStat + 1] = nex;
      wrow[kPolyStat + 2] = mist;
      wrow[kPolyStat + 3] = sqe;
      wrow[kPolyStat + 4] = sigma;
      wrow[kPolyStat + 5] = 0.f;
      wrow[kPolyStat + 6] = scale;
    }
  }
}

struct PolyArgs {
  const void* num;
  const int* pairs;
  const void* y;
  float* ws;
  int d0, npairs, y_i8, B, R, S, dim, variant, bias, w_bf16, num_bf16;
  float inv_p;
};

template <int W, int RULE, bool SHR>
int launch_poly(dim3 grid, hipStream_t st, const DensePipes& P, const PolyArgs& A) {
  if (A.num_bf16)
    hipLaunchKernelGGL((poly_round_kernel<W, RULE, SHR, true>), grid, dim3(W * 64), 0, st, P,
                       A.num, A.d0, A.pairs, A.npairs, A.y, A.y_i8, A.B, A.R, A.S, A.dim, A.ws,
                       A.variant, A.bias, A.w_bf16, A.inv_p);
  else
    hipLaunchKernelGGL((poly_round_kernel<W, RULE, SHR, false>), grid, dim3(W * 64), 0, st, P,
                       A.num, A.d0, A.pairs, A.npairs, A.y, A.y_i8, A.B, A.R, A.S, A.dim, A.ws,
                       A.variant, A.bias, A.w_bf16, A.inv_p);
  return (int)hipGetLastError();
}

template <int W>
int dispatch_poly(int rule, int shr, dim3 grid, hipStream_t st, const DensePipes& P,
                  const PolyArgs& A) {
  if (rule == kPegasos) return launch_poly<W, kPegasos, true>(grid, st, P, A);
  if (rule == kHinge)
    return shr ? launch_poly<W, kHinge, true>(grid, st, P, A)
               : launch_poly<W, kHinge, false>(grid, st, P, A);
  if (rule == kEps)
    return shr ? launch_poly<W, kEps, true>(grid, st, P, A)
               : launch_poly<W, kEps, false>(grid, st, P, A);
  return shr ? launch_poly<W, kLogistic, true>(grid, st, P, A)
             : launch_poly<W, kLogistic, false>(grid, st, P, A);
}

}  // namespace
}  // namespace omldm

using namespace omldm;

OMLDM_API int omldm_linear_poly_max() { return kPolyMax; }

// Floats of workspace a launch of M pipelines × S spokes needs.
OMLDM_API long long omldm_linear_poly_ws_words(int M, int S) {
  return (long long)(M > 0 ? M : 0) * (S > 0 ? S : 0) * kPolyWsw;
}

// One Synchronous round of M pipelines (1 ≤ M ≤ 16) on one batch without categorical
// columns behind the degree-2 map: num is [B, d0] (contiguous), pairs int32 [npairs][2] on
// the device, the model's columns are the d0 raw ones at slots [0, d0), the products at
// [d0, d0 + npairs) and the bias at dim − 1, with 256 < d0 + npairs + bias ≤ 1024 and
// 1 ≤ d0 ≤ 30 / 39 / 45 at up to 512 / 768 / 1024 columns. The other arguments are
// omldm_linear_dense_round's. Returns a HIP error code, or < 0 for a shape it does not take
// (nothing is launched).
OMLDM_API int omldm_linear_poly_round(int M, const void* const* w, float* const* dacc,
                                      double* const* cum, float* const* stats, const float* C,
                                      const float* eps, const float* lr, const float* lam,
                                      const float* tbase, int w_bf16, const void* num,
                                      int num_bf16, int d0, const int* pairs, int npairs,
                                      const void* y, int y_i8, int B, int R, int S, int dim,
                                      float* ws, int rule, int variant, int bias, int shr,
                                      float inv_p, void* stream) {
  if (M < 1 || M > kDenseMaxM || !w || !dacc || !C || !eps || !lr || !lam || !tbase) return -1;
  if (d0 < 1 || d0 > kPolyRawMax || npairs < 0 || npairs > kPolyMax) return -2;
  const int D = d0 + npairs + (bias ? 1 : 0);
  if (D < kPolyMin || D > kPolyMax || d0 + npairs > dim - 1) return -2;
  if (d0 > (D <= 512 ? PolyShape<2>::kRawMax : D <= 768 ? PolyShape<3>::kRawMax
                                                        : PolyShape<4>::kRawMax))
    return -2;
  if (B < 0 || R < 1 || S < 1 || !ws || !y || !num || (npairs > 0 && !pairs)) return -3;
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
  const PolyArgs A{num, pairs, y, ws, d0, npairs, y_i8, B, R, S, dim, variant, bias, w_bf16,
                   num_bf16, inv_p};
  int e;
  if (D <= 512)
    e = dispatch_poly<2>(rule, shr, grid, st, P, A);
  else if (D <= 768)
    e = dispatch_poly<3>(rule, shr, grid, st, P, A);
  else
    e = dispatch_poly<4>(rule, shr, grid, st, P, A);
  if (e) return e;
  hipLaunchKernelGGL(round_fold_kernel<kPolyWsw>, dim3(M), dim3(256), 0, st, O, ws, S, S_act,
                     d0 + npairs, D, dim, inv_p);
  return (int)hipGetLastError();
}
