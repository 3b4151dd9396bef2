// The serving plan: the table that drives serve_plan_kernel (serving.hip) and its CPU
// mirror (csrc/host/serve_plan_cpu.cpp). Plain C++, no HIP: both sides include this file,
// so the layout and the validation are one text.
//
// A plan is n_models entries of kPlanWords int32 words. Entry m:
//   [kPlKind]     kPlanLinear / kPlanMulticlass / kPlanKmeans / kPlanMlp / kPlanTree
//   [kPlOut]      index into Mailbox::result
//   [kPlStages]   number of preprocessor stages (≤ kPlanMaxStages)
//   [kPlFlags]    kPlanFlagBias: a bias lane (value 1, slot width − 1);
//                 kPlanFlagSign: the result is ±1 (score ≥ 0), not the score;
//                 kPlanFlagDense: categorical lanes are not scored (ORR)
//   [kPlOff]      arena offset (floats) of the parameters
//   [kPlWidth]    row width: the hashed dim, d + 1 for a dense row, d for centroids
//   [kPlK]        rows: 1, the classes K, or the centroids k
//   [kPlStage0 + 4·s ..]  stage s: type, a, b, input width
//                 kPlanAffine: a / b = arena offsets of shift[n] / div[n]
//                 kPlanPoly2:  a = first pair (index into the entry's pair area)
//                 kPlanPoly2Lazy: the same map, not laid out in lanes — only as the last
//                              stage of a kPlanTree entry, whose walk needs one feature per
//                              node: feature f < n is lane f, feature n + p is the product of
//                              pair p in the order of PolynomialFeatures(2), (0,0), (0,1), …,
//                              (0,n−1), (1,1), …, worked out from p (no pair table). The lanes
//                              stay n wide, the tree's features n + n(n+1)/2 (poly2_pair).
//   [kPlAux ..]   the parameters of a kPlanMlp / kPlanTree entry (words 24–63, else unused)
//                 kPlanMlp:  L, activation (0 relu, 1 tanh, 2 sigmoid, 3 identity), task
//                            (0 score out[0], 1 ±1 by out[0] ≥ 0, 2 argmax, lowest index on a
//                            tie), then the L + 1 widths w_0 … w_L (each 1..64, w_0 = the dense
//                            width after the stages). Arena region, layer by layer: Wt_l
//                            [w_l × w_{l+1}] input-major (lane j reads Wt_l[i·w_{l+1} + j]),
//                            then b_l [w_{l+1}]; kPlWidth = the region's floats, kPlK = 1.
//                 kPlanTree: N nodes (1..1024), C classes (2..32), depth (the walk takes at
//                            most depth + 1 steps). Arena region: feat[N], thr[N], left[N],
//                            right[N], cc[N·C] — the head of a Hoeffding tree's state;
//                            kPlWidth = N·(4 + C), kPlK = 1.
//   [kPlPairs ..] pair area: 64 words, pair p = a | b << 8 (new lane = v[a]·v[b])
// The parameters live in an fp32 arena, one per bank, both of one layout.
#pragma once
#include <stdint.h>

namespace omldm {

constexpr int kPlanWords = 128;
constexpr int kPlanMaxModels = 60;
constexpr int kPlanMaxStages = 4;
constexpr int kPlanLanes = 64;

constexpr int kPlanLinear = 0, kPlanMulticlass = 1, kPlanKmeans = 2;
constexpr int kPlanMlp = 4, kPlanTree = 5;  // (3 is no kind)
constexpr int kPlanMlpMaxLayers = 4, kPlanMlpMaxWidth = 64;
constexpr int kPlanTreeMaxNodes = 1024, kPlanTreeMaxClasses = 32;
constexpr int kPlanAffine = 0, kPlanPoly2 = 1, kPlanPoly2Lazy = 2;
constexpr int kPlanFlagBias = 1, kPlanFlagSign = 2, kPlanFlagDense = 4;

constexpr int kPlKind = 0, kPlOut = 1, kPlStages = 2, kPlFlags = 3, kPlOff = 4, kPlWidth = 5,
              kPlK = 6, kPlStage0 = 8, kPlAux = 24, kPlPairs = 64;

// error codes of plan_check (omldm_serve_plan_start / omldm_cpu_serve_plan return them)
constexpr int kPlanErrShape = -10;    // n_models, dn, dc, dim, a kind or a flag out of range
constexpr int kPlanErrLanes = -11;    // more than 64 lanes (dense after stages + dc + bias)
constexpr int kPlanErrStages = -12;   // more than 4 stages, or a stage's width does not chain
constexpr int kPlanErrArena = -13;    // an offset or extent outside the arena
constexpr int kPlanErrOutput = -14;   // an output index ≥ 60 or used twice
constexpr int kPlanErrPairs = -15;    // a pair outside the pair area or ≥ the input width

// Pair p of the degree-2 products over n inputs, in combinations-with-replacement order:
// a = the row, b = a + the position in it. 0 ≤ p < n(n+1)/2 (at most n steps).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void poly2_pair(int p, int n, int* a, int* b) {
  int row = 0;
  while (row < n - 1 && p >= n - row) {
    p -= n - row;
    ++row;
  }
  *a = row;
  *b = row + p;
}

// The plan holds a kPlanMlp or kPlanTree entry (the launcher then starts the instantiation of
// the wave that knows them).
inline bool plan_has_nonlinear(const int* plan, int n_models) {
  for (int m = 0; m < n_models; ++m) {
    const int kind = plan[(long long)m * kPlanWords + kPlKind];
    if (kind == kPlanMlp || kind == kPlanTree) return true;
  }
  return false;
}

// 0 when every entry is safe to run against an arena of `arena_floats` floats.
inline int plan_check(const int* plan, int n_models, long long arena_floats, int dn, int dc,
                      int dim) {
  if (!plan || n_models < 1 || n_models > kPlanMaxModels || dn < 0 || dc < 0 || dim < 1 ||
      arena_floats < 0)
    return kPlanErrShape;
  if (dn + dc > kPlanLanes - 3) return kPlanErrLanes;  // the request line's payload
  unsigned long long used = 0;
  for (int m = 0; m < n_models; ++m) {
    const int* e = plan + (long long)m * kPlanWords;
    const int kind = e[kPlKind], flags = e[kPlFlags], ns = e[kPlStages];
    const long long off = e[kPlOff], width = e[kPlWidth], K = e[kPlK];
    const bool nonlinear = kind == kPlanMlp || kind == kPlanTree;
    if (((kind < kPlanLinear || kind > kPlanKmeans) && !nonlinear) || (flags & ~7))
      return kPlanErrShape;
    if (e[kPlOut] < 0 || e[kPlOut] >= kPlanMaxModels || ((used >> e[kPlOut]) & 1ull))
      return kPlanErrOutput;
    used |= 1ull << e[kPlOut];
    if (ns < 0 || ns > kPlanMaxStages) return kPlanErrStages;
    int D = dn;
    for (int s = 0; s < ns; ++s) {
      const int* st = e + kPlStage0 + 4 * s;
      if (st[3] != D) return kPlanErrStages;
      if (st[0] == kPlanPoly2Lazy) {
        // (the lanes stay D wide; the tree's features become D + D(D+1)/2)
        if (kind != kPlanTree || s != ns - 1 || D < 1 || D > kPlanLanes) return kPlanErrStages;
      } else if (st[0] == kPlanAffine) {
        for (int q = 1; q <= 2; ++q)
          if (st[q] < 0 || (long long)st[q] + D > arena_floats) return kPlanErrArena;
      } else if (st[0] == kPlanPoly2) {
        const int np = D * (D + 1) / 2;
        if (D + np > kPlanLanes) return kPlanErrLanes;
        if (st[1] < 0 || st[1] + np > kPlanWords - kPlPairs) return kPlanErrPairs;
        for (int p = 0; p < np; ++p) {
          const int w = e[kPlPairs + st[1] + p];
          if (w < 0 || (w & 0xff) >= D || (w >> 8) >= D) return kPlanErrPairs;
        }
        D += np;
      } else {
        return kPlanErrStages;
      }
    }
    const int bias = (flags & kPlanFlagBias) ? 1 : 0;
    if (off < 0 || width < 1 || K < 1) return kPlanErrArena;
    if (kind == kPlanMlp) {
      const int* a = e + kPlAux;
      const int L = a[0];
      if (L < 1 || L > kPlanMlpMaxLayers || a[1] < 0 || a[1] > 3 || a[2] < 0 || a[2] > 2 ||
          flags || K != 1)
        return kPlanErrShape;
      long long floats = 0;
      for (int l = 0; l <= L; ++l) {
        if (a[3 + l] < 1 || a[3 + l] > kPlanMlpMaxWidth) return kPlanErrShape;
        if (l) floats += (long long)a[2 + l] * a[3 + l] + a[3 + l];
      }
      if (a[3] != D || width != floats) return kPlanErrShape;
    } else if (kind == kPlanTree) {
      const int* a = e + kPlAux;
      if (a[0] < 1 || a[0] > kPlanTreeMaxNodes || a[1] < 2 || a[1] > kPlanTreeMaxClasses ||
          a[2] < 0 || flags || K != 1 || D < 1 || D > kPlanLanes ||
          width != (long long)a[0] * (4 + a[1]))
        return kPlanErrShape;
    } else if (kind == kPlanKmeans) {
      if (D < 1 || D > kPlanLanes) return kPlanErrLanes;
      if (width != D || flags) return kPlanErrShape;
    } else {
      const int dense = (flags & kPlanFlagDense) ? 1 : 0;
      if (D + (dense ? 0 : dc) + bias > kPlanLanes) return kPlanErrLanes;
      if (kind == kPlanLinear && K != 1) return kPlanErrShape;
      if (kind == kPlanMulticlass && (flags & (kPlanFlagSign | kPlanFlagDense)))
        return kPlanErrShape;
      if (dense ? width != D + bias : width != dim) return kPlanErrShape;
    }
    if (off + K * width > arena_floats) return kPlanErrArena;
  }
  return 0;
}

}  // namespace omldm
