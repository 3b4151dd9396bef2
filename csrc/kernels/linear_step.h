// What the register-resident sequential rounds of the linear family share
// (linear_dense.hip: ≤ 256 columns in one wave; linear_poly.hip: PolynomialFeatures(2) of
// the raw row, 257-1024 columns split over the waves of a workgroup): the per-launch
// pipeline tables, the fixed-order wave sum, a row's step in the oracle's operation order
// (csrc/host/linear_cpu.cpp: omldm_cpu_linear_round) and the round's fold.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

constexpr int kDenseMaxM = 16;  // pipelines per launch

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

// What a row's step needs besides the model, for the lane that owns the row: τ's cap and
// denominator from the row's ‖x‖² pn (hinge, ε-insensitive), the row's shrink, Pegasos'
// 1/(λT)·y and (T − 1)/T at the row's step index T. A skipped row (unlabeled, or past the
// spoke's last row; ys = 0) has cap 0 and shrink 1, so its step is 0 without a branch.
template <int RULE>
__device__ __forceinline__ void row_terms(bool skip, float ys, float pn, float T, int variant,
                                          float C, float lam, float shr, float& capv, float& denv,
                                          float& shv, float& cyv) {
  capv = 0.f;
  denv = 1.f;
  shv = skip ? 1.f : shr;
  cyv = 0.f;
  if (RULE == kHinge || RULE == kEps) {
    if (!skip && pn > 0.f) {
      capv = variant == 1 ? C : __builtin_inff();
      denv = variant == 2 ? pn + 0.5f / C : pn;
    }
  }
  if (RULE == kPegasos) {
    cyv = (1.f / (lam * T)) * ys;
    shv = skip ? 1.f : (T - 1.f) / T;
  }
}

// The row's step c (the update is d += (c/σ)·x) from its label yt and margin mg.
template <int RULE>
__device__ __forceinline__ float step_coef(float yt, float mg, float cap, float den, float cy,
                                           float eps, float lr) {
  if (RULE == kPegasos) return yt * mg < 1.f ? cy : 0.f;
  if (RULE == kHinge) {
    const float loss = fmaxf(0.f, 1.f - yt * mg);
    return fminf(cap, loss / den) * yt;
  }
  if (RULE == kEps) {
    const float err = yt - mg;
    const float loss = fmaxf(0.f, fabsf(err) - eps);
    return fminf(cap, loss / den) * (err >= 0.f ? 1.f : -1.f);
  }
  return lr * yt / (1.f + expf(yt * mg));
}

// A labeled row's loss, mistake and squared error from its label and parked margin.
template <int RULE>
__device__ __forceinline__ void row_stats(float yv, float mv, float eps, float& loss, float& mist,
                                          float& sqe) {
  if (RULE == kEps) {
    const float err = yv - mv;
    loss += fmaxf(0.f, fabsf(err) - eps);
    sqe += err * err;
  } else if (RULE == kLogistic) {
    const float z = yv * mv;
    loss += z > 0.f ? log1pf(expf(-z)) : (-z + log1pf(expf(z)));
    mist += z <= 0.f ? 1.f : 0.f;
  } else {
    const float ym = yv * mv;
    loss += fmaxf(0.f, 1.f - ym);
    mist += ym <= 0.f ? 1.f : 0.f;
  }
}

// The round's fold, one block per pipeline: the S_act workspace rows (WSW words: D deltas,
// then at WSW − 8 loss, n, mistakes, sq_err, σ, overflow, σ·inv_p, -) in spoke order into
// the accumulator's D touched slots (column j < ncol at slot j, the bias column at
// dim − 1), the round counters, the running totals and the optional per-spoke statistics.
// The counters are SET (Σσ·inv_p and Σinv_p summed from 0 in spoke order): linear_apply
// leaves them as they are, like every GPU round kernel's.
template <int WSW>
__global__ __launch_bounds__(256) void round_fold_kernel(DenseOut O, const float* __restrict__ ws,
                                                         int S, int S_act, int ncol, int D, int dim,
                                                         float inv_p) {
  constexpr int kStat = WSW - 8;
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* wm = ws + (size_t)m * S * WSW;
  float* dacc = O.dacc[m];
  for (int j = tid; j < D; j += 256) {
    const int slot = j < ncol ? j : dim - 1;
    float v = dacc[slot];
    for (int s = 0; s < S_act; ++s) v += wm[(size_t)s * WSW + j];
    dacc[slot] = v;
  }
  if (tid < 8) {
    float t = 0.f;
    for (int s = 0; s < S_act; ++s) t += tid == 7 ? inv_p : wm[(size_t)s * WSW + kStat + tid];
    if (tid == 6) dacc[dim] = t;
    else if (tid == 7) dacc[dim + 1] = t;
    else if (tid != 4 && O.cum[m]) O.cum[m][tid] += (double)t;  // σ is no running total
  }
  float* st = O.stats[m];
  if (st)
    for (int i = tid; i < S * 6; i += 256) {
      const int s = i / 6, c = i - 6 * s;
      st[i] = s < S_act ? wm[(size_t)s * WSW + kStat + c] : (c == 4 ? 1.f : 0.f);
    }
}

}  // namespace
}  // namespace omldm
