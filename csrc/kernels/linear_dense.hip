// Exact dense sequential round for numerical-only linear pipelines (no categorical
// columns): one Synchronous round of S virtual spokes with the semantics of
// omldm_cpu_linear_round (csrc/host/linear_cpu.cpp) at dc = 0.
//
// The model a spoke touches is its D = dn + bias ≤ 256 dense columns, so a spoke is ONE
// wavefront that keeps the round-start weights w0 and its private delta d in registers
// (lane ℓ owns columns ℓ, ℓ+64, ℓ+128, ℓ+192) — no hash table, no occurrence lists, no
// prep pass. Grid (S, M): M pipelines that share the batch run in one launch.
//
//  * Rows come in chunks (64 rows; 32 at four columns per lane). A chunk is loaded
//    coalesced into registers one chunk ahead (clamped addresses, no guards, so the loads
//    stay in flight while the current chunk runs) and is then laid out in LDS, the bias
//    column as 1 and the columns past D as 0.
//  * Everything that does not depend on the model is computed once per chunk with lane i
//    owning row i: the label, ‖x‖² (summed in the oracle's order), τ's denominator and
//    cap, the shrink, Pegasos' T, 1/(λT)·y and (T − 1)/T. The row loop fetches them with
//    one readlane each. An unlabeled row (NaN) has label 0, cap 0 and shrink 1 there, so
//    its step is 0 without a branch.
//  * Per row the dependency chain is: the per-lane fmas of x·(w0 + d), one wave reduction
//    (DPP, fixed order), the wave-uniform step math in the oracle's operation order
//    (contraction off, so the only numerical difference from the oracle is the summation
//    order of the dot product) and the per-lane update fmas. The row's margin is parked in
//    lane i; loss, mistakes and squared error are computed from the parked margins once
//    per chunk, again lane-owned, and summed over the wave at the end of the round.
//  * The spoke carries the model scale σ like the oracle: m = σ·Σx(w0 + d), σ ×= shrink,
//    d += (c/σ)·x.
//  * Round end: every (pipeline, spoke) stores one workspace row (its D deltas scaled by
//    σ·inv_p, σ·inv_p, the statistics) and a second tiny kernel folds the rows in spoke
//    order into the accumulator — no workgroup waits for another and no float atomics, so
//    a round is bit-reproducible.
#include "common.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

constexpr int kDenseMax = 256;   // columns (dn + bias) per spoke
constexpr int kDenseMaxM = 16;   // pipelines per launch
constexpr int kU = 8;            // rows per unrolled step of the row loop
constexpr int kStatOff = kDenseMax;      // workspace row: [0, D) deltas, then the statistics
constexpr int kWsw = kDenseMax + 8;      // loss, n, mistakes, sq_err, σ, overflow, σ·inv_p, -

enum { kHinge = 0, kEps = 1, kLogistic = 2, kPegasos = 3 };

struct DensePipes {
  const void* w[kDenseMaxM];
  float C[kDenseMaxM], eps[kDenseMaxM], lr[kDenseMaxM], lam[kDenseMaxM], tbase[kDenseMaxM];
};

struct DenseOut {
  float* dacc[kDenseMaxM];
  double* cum[kDenseMaxM];
  float* stats[kDenseMaxM];
};

// v of another lane for the rows of ROWS, v itself for the others.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_rows(float v) {
  const int b = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, CTRL, ROWS, 0xF, false));
}

// Full-wave sum, wave-uniform, in one fixed order: the 16-lane row sums, then row_bcast:15
// into rows 1 and 3 and row_bcast:31 into rows 2 and 3 leave the total in lane 63 (the
// rows a step does not write double instead; nothing reads them afterwards).
__device__ __forceinline__ float wave_sum_last(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x124>(v);
  v += dpp_mov<0x128>(v);
  v += dpp_rows<0x142, 0xA>(v);
  v += dpp_rows<0x143, 0xC>(v);
  return readlane_f(v, 63);
}

template <int CPL>
struct DenseShape {
  static constexpr int kRows = CPL == 4 ? 32 : 64;  // rows per chunk
  static constexpr int kStride = 64 * CPL + 1;      // odd: row-per-lane reads hit 32 banks
};

// Rows [t0, t0 + kRows) of the spoke into registers as raw bits, with the label of row
// t0 + lane. A row at or past t1 reads row t1 - 1 and a column at or past dn reads column
// dn - 1 (ld: the row stride), so every address is inside the batch. No branch, select or
// conversion here: the loads stay in flight until the chunk is laid out in LDS.
template <int CPL, bool NBF>
__device__ __forceinline__ void load_chunk(const void* __restrict__ num, const void* __restrict__ y,
                                           int y_i8, long long t0, long long t1, int dn, int ld,
                                           int lane, unsigned (&x)[DenseShape<CPL>::kRows][CPL],
                                           unsigned& yraw) {
  constexpr int CR = DenseShape<CPL>::kRows;
#pragma unroll
  for (int r = 0; r < CR; ++r) {
    const long long t = t0 + r < t1 ? t0 + r : t1 - 1;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int j = lane + 64 * k;
      const size_t i = (size_t)t * ld + (j < dn ? j : dn - 1);
      x[r][k] = NBF ? (unsigned)static_cast<const unsigned short*>(num)[i]
                    : static_cast<const unsigned*>(num)[i];
    }
  }
  const long long t = t0 + lane < t1 ? t0 + lane : t1 - 1;
  if (y_i8)
    yraw = (unsigned)(int)static_cast<const signed char*>(y)[t];
  else
    yraw = static_cast<const unsigned*>(y)[t];
}

template <int CPL, int RULE, bool SHR, bool NBF>
__global__ __launch_bounds__(64) void dense_round_kernel(
    DensePipes P, const void* __restrict__ num_, int dn_, const void* __restrict__ y,
    int y_i8, int B, int R, int S, int dim, float* __restrict__ ws, int variant, int bias,
    int w_bf16, float inv_p) {
  constexpr int CR = DenseShape<CPL>::kRows;
  constexpr int ST = DenseShape<CPL>::kStride;
  __shared__ float xs[CR * ST];
  __shared__ float ms[CR];  // the chunk's margins, row i at i
  const int s = blockIdx.x, m = blockIdx.y, lane = threadIdx.x;
  const long long a = (long long)s * R;
  if (a >= B) return;  // an idle spoke is no worker of the round
  const long long b = a + R < (long long)B ? a + R : (long long)B;
  const int nrows = (int)(b - a);
  const int D = dn_ + (bias ? 1 : 0);
  // bias only (dn = 0): the loads read word 0 of the workspace (row stride 0), which no
  // column uses
  const void* num = dn_ > 0 ? num_ : ws;
  const int dn = dn_ > 0 ? dn_ : 1;
  const float C = P.C[m], eps = P.eps[m], lr = P.lr[m], lam = P.lam[m], tbase = P.tbase[m];
  const float shr = RULE == kLogistic ? 1.f - lr * lam : 1.f - lam;
  const float inf = __builtin_inff();

  float w0[CPL], d[CPL], fill[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int j = lane + 64 * k;
    const int slot = j < dn_ ? j : dim - 1;
    float v = 0.f;
    if (j < D)
      v = w_bf16 ? to_f(static_cast<const __hip_bfloat16*>(P.w[m])[slot])
                 : static_cast<const float*>(P.w[m])[slot];
    w0[k] = v;
    d[k] = 0.f;
    fill[k] = (j == dn_ && j < D) ? 1.f : 0.f;  // the bias column; 0 past D
  }

  float sigma = 1.f, loss_l = 0.f, nex_l = 0.f, mist_l = 0.f, sqe_l = 0.f;  // per-lane sums
  unsigned xn[CR][CPL], yn;
  load_chunk<CPL, NBF>(num, y, y_i8, a, b, dn, dn_, lane, xn, yn);

  const int nchunks = (nrows + CR - 1) / CR;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int nr = nrows - ch * CR < CR ? nrows - ch * CR : CR;
    // the chunk into LDS: column j < dn its value, the bias column 1, the rest 0
#pragma unroll
    for (int r = 0; r < CR; ++r)
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int j = lane + 64 * k;
        const float v = __builtin_bit_cast(float, NBF ? xn[r][k] << 16 : xn[r][k]);
        xs[r * ST + j] = j < dn_ ? v : fill[k];
      }
    const long long t0 = a + (long long)ch * CR;
    const float yl = y_i8 ? (float)(int)yn : __builtin_bit_cast(float, yn);
    const float yv = (lane < CR && t0 + lane < b) ? yl : __builtin_nanf("");
    __syncthreads();
    // the next chunk's rows, in flight while this one runs (past the last chunk: row b - 1)
    load_chunk<CPL, NBF>(num, y, y_i8, t0 + CR, b, dn, dn_, lane, xn, yn);

    // lane i owns row i of the chunk: what the row's step needs besides the model
    const bool skip = yv != yv;  // unlabeled, or past the spoke's last row
    const float ys = skip ? 0.f : yv;
    float capv = 0.f, denv = 1.f, shv = skip ? 1.f : shr, cyv = 0.f;
    if (RULE == kHinge || RULE == kEps) {
      const float* xrow = xs + (lane < CR ? lane : 0) * ST;
      float pn = 0.f;
#pragma unroll 8
      for (int j = 0; j < D; ++j) pn += xrow[j] * xrow[j];
      if (!skip && pn > 0.f) {
        capv = variant == 1 ? C : inf;
        denv = variant == 2 ? pn + 0.5f / C : pn;
      }
    }
    if (RULE == kPegasos) {
      const float T = tbase + (float)(ch * CR + lane);
      cyv = (1.f / (lam * T)) * ys;
      shv = skip ? 1.f : (T - 1.f) / T;
    }

    for (int r0 = 0; r0 < nr; r0 += kU) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int r = r0 + u;  // a row at or past nr is a skipped row: its step is 0
        float x[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) x[k] = xs[r * ST + lane + 64 * k];
        const float yt = readlane_f(ys, r);
        float pm = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) pm = __builtin_fmaf(x[k], w0[k] + d[k], pm);
        const float mg = sigma * wave_sum_last(pm);
        ms[r] = mg;  // every lane stores the same word
        float c;
        if (RULE == kPegasos) {
          c = yt * mg < 1.f ? readlane_f(cyv, r) : 0.f;
        } else if (RULE == kHinge) {
          const float loss = fmaxf(0.f, 1.f - yt * mg);
          c = fminf(readlane_f(capv, r), loss / readlane_f(denv, r)) * yt;
        } else if (RULE == kEps) {
          const float err = yt - mg;
          const float loss = fmaxf(0.f, fabsf(err) - eps);
          c = fminf(readlane_f(capv, r), loss / readlane_f(denv, r)) * (err >= 0.f ? 1.f : -1.f);
        } else {
          c = lr * yt / (1.f + expf(yt * mg));
        }
        float cv = c;
        if (SHR) {
          sigma *= readlane_f(shv, r);
          cv = c != 0.f ? c / sigma : 0.f;
        }
#pragma unroll
        for (int k = 0; k < CPL; ++k) d[k] = __builtin_fmaf(cv, x[k], d[k]);
      }
    }

    // the chunk's statistics from the parked margins, lane i for row i
    __syncthreads();
    if (!skip) {
      const float mv = ms[lane];
      nex_l += 1.f;
      if (RULE == kEps) {
        const float err = yv - mv;
        loss_l += fmaxf(0.f, fabsf(err) - eps);
        sqe_l += err * err;
      } else if (RULE == kLogistic) {
        const float z = yv * mv;
        loss_l += z > 0.f ? log1pf(expf(-z)) : (-z + log1pf(expf(z)));
        mist_l += z <= 0.f ? 1.f : 0.f;
      } else {
        const float ym = yv * mv;
        loss_l += fmaxf(0.f, 1.f - ym);
        mist_l += ym <= 0.f ? 1.f : 0.f;
      }
    }
    __syncthreads();
  }

  const float loss_sum = wave_sum(loss_l), nex = wave_sum(nex_l), mist = wave_sum(mist_l),
              sqe = wave_sum(sqe_l);
  const float scale = sigma * inv_p;
  float* wrow = ws + ((size_t)m * S + s) * kWsw;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int j = lane + 64 * k;
    if (j < D) wrow[j] = d[k] * scale;
  }
  if (lane == 0) {
    wrow[kStatOff + 0] = loss_sum;
    wrow[kStatOff + 1] = nex;
    wrow[kStatOff + 2] = mist;
    wrow[kStatOff + 3] = sqe;
    wrow[kStatOff + 4] = sigma;
    wrow[kStatOff + 5] = 0.f;
    wrow[kStatOff + 6] = scale;
  }
}

// The round's fold, one block per pipeline: the S_act workspace rows in spoke order into
// the accumulator's D touched slots, the round counters, the running totals and the
// optional per-spoke statistics. The counters are SET (Σσ·inv_p and Σinv_p summed from 0
// in spoke order): linear_apply leaves them as they are, like every GPU round kernel's.
__global__ __launch_bounds__(256) void dense_fold_kernel(DenseOut O, const float* __restrict__ ws,
                                                         int S, int S_act, int dn, int D, int dim,
                                                         float inv_p) {
  const int m = blockIdx.x, j = threadIdx.x;
  const float* wm = ws + (size_t)m * S * kWsw;
  float* dacc = O.dacc[m];
  if (j < D) {
    const int slot = j < dn ? j : dim - 1;
    float v = dacc[slot];
    for (int s = 0; s < S_act; ++s) v += wm[(size_t)s * kWsw + j];
    dacc[slot] = v;
  }
  if (j < 8) {
    float t = 0.f;
    for (int s = 0; s < S_act; ++s) t += j == 7 ? inv_p : wm[(size_t)s * kWsw + kStatOff + j];
    if (j == 6) dacc[dim] = t;
    else if (j == 7) dacc[dim + 1] = t;
    else if (j != 4 && O.cum[m]) O.cum[m][j] += (double)t;  // σ is no running total
  }
  float* st = O.stats[m];
  if (st)
    for (int i = j; i < S * 6; i += 256) {
      const int s = i / 6, c = i - 6 * s;
      st[i] = s < S_act ? wm[(size_t)s * kWsw + kStatOff + c] : (c == 4 ? 1.f : 0.f);
    }
}

template <int CPL, int RULE, bool SHR>
int launch_dense(dim3 grid, hipStream_t st, const DensePipes& P, const void* num, int num_bf16,
                 int dn, const void* y, int y_i8, int B, int R, int S, int dim, float* ws,
                 int variant, int bias, int w_bf16, float inv_p) {
  if (num_bf16)
    hipLaunchKernelGGL((dense_round_kernel<CPL, RULE, SHR, true>), grid, dim3(64), 0, st, P, num,
                       dn, y, y_i8, B, R, S, dim, ws, variant, bias, w_bf16, inv_p);
  else
    hipLaunchKernelGGL((dense_round_kernel<CPL, RULE, SHR, false>), grid, dim3(64), 0, st, P, num,
                       dn, y, y_i8, B, R, S, dim, ws, variant, bias, w_bf16, inv_p);
  return (int)hipGetLastError();
}

template <int CPL>
int dispatch_dense(int rule, int shr, dim3 grid, hipStream_t st, const DensePipes& P,
                   const void* num, int num_bf16, int dn, const void* y, int y_i8, int B, int R,
                   int S, int dim, float* ws, int variant, int bias, int w_bf16, float inv_p) {
#define OMLDM_DENSE(RULE, SHR)                                                                \
  return launch_dense<CPL, RULE, SHR>(grid, st, P, num, num_bf16, dn, y, y_i8, B, R, S, dim, \
                                      ws, variant, bias, w_bf16, inv_p)
  if (rule == kPegasos) OMLDM_DENSE(kPegasos, true);
  if (rule == kHinge) {
    if (shr) OMLDM_DENSE(kHinge, true);
    OMLDM_DENSE(kHinge, false);
  }
  if (rule == kEps) {
    if (shr) OMLDM_DENSE(kEps, true);
    OMLDM_DENSE(kEps, false);
  }
  if (shr) OMLDM_DENSE(kLogistic, true);
  OMLDM_DENSE(kLogistic, false);
#undef OMLDM_DENSE
}

}  // namespace
}  // namespace omldm

using namespace omldm;

OMLDM_API int omldm_linear_dense_max() { return kDenseMax; }

// Floats of workspace a launch of M pipelines × S spokes needs.
OMLDM_API long long omldm_linear_dense_ws_words(int M, int S) {
  return (long long)(M > 0 ? M : 0) * (S > 0 ? S : 0) * kWsw;
}

// One Synchronous round of M pipelines (1 ≤ M ≤ 16) on one batch without categorical
// columns. w / dacc / cum / stats: M pointers each (cum and stats, or their entries, may be
// NULL); C / eps / lr / lam / tbase: M floats each. shr: 0 no shrink, 1 σ ×= 1 − λ per row
// (logistic: 1 − lr·λ), 2 Pegasos. Every dacc is [dim + 2] with dacc[:dim] = 0 on entry.
// Returns a HIP error code, or < 0 for a shape it does not take (nothing is launched).
OMLDM_API int omldm_linear_dense_round(int M, const void* const* w, float* const* dacc,
                                       double* const* cum, float* const* stats, const float* C,
                                       const float* eps, const float* lr, const float* lam,
                                       const float* tbase, int w_bf16, const void* num,
                                       int num_bf16, int dn, const void* y, int y_i8, int B, int R,
                                       int S, int dim, float* ws, int rule, int variant, int bias,
                                       int shr, float inv_p, void* stream) {
  const int D = dn + (bias ? 1 : 0);
  if (M < 1 || M > kDenseMaxM || !w || !dacc || !C || !eps || !lr || !lam || !tbase) return -1;
  if (dn < 0 || D < 1 || D > kDenseMax || D > dim) return -2;
  if (B < 0 || R < 1 || S < 1 || !ws || !y || (dn > 0 && !num)) return -3;
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
  int e;
  if (D <= 64)
    e = dispatch_dense<1>(rule, shr, grid, st, P, num, num_bf16, dn, y, y_i8, B, R, S, dim, ws,
                          variant, bias, w_bf16, inv_p);
  else if (D <= 128)
    e = dispatch_dense<2>(rule, shr, grid, st, P, num, num_bf16, dn, y, y_i8, B, R, S, dim, ws,
                          variant, bias, w_bf16, inv_p);
  else
    e = dispatch_dense<4>(rule, shr, grid, st, P, num, num_bf16, dn, y, y_i8, B, R, S, dim, ws,
                          variant, bias, w_bf16, inv_p);
  if (e) return e;
  hipLaunchKernelGGL(dense_fold_kernel, dim3(M), dim3(256), 0, st, O, ws, S, S_act, dn, D, dim,
                     inv_p);
  return (int)hipGetLastError();
}
