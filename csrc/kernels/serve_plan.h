// The serving plan: the table that drives serve_plan_kernel (serving.hip) and its CPU
// mirror (csrc/host/serve_plan_cpu.cpp). Plain C++, no HIP: both sides include this file,
// so the layout and the validation are one text.
//
// A plan is n_models entries of kPlanWords int32 words. Entry m:
//   [kPlKind]     kPlanLinear / kPlanMulticlass / kPlanKmeans
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
constexpr int kPlanAffine = 0, kPlanPoly2 = 1;
constexpr int kPlanFlagBias = 1, kPlanFlagSign = 2, kPlanFlagDense = 4;

constexpr int kPlKind = 0, kPlOut = 1, kPlStages = 2, kPlFlags = 3, kPlOff = 4, kPlWidth = 5,
              kPlK = 6, kPlStage0 = 8, kPlPairs = 64;

// error codes of plan_check (omldm_serve_plan_start / omldm_cpu_serve_plan return them)
constexpr int kPlanErrShape = -10;    // n_models, dn, dc, dim, a kind or a flag out of range
constexpr int kPlanErrLanes = -11;    // more than 64 lanes (dense after stages + dc + bias)
constexpr int kPlanErrStages = -12;   // more than 4 stages, or a stage's width does not chain
constexpr int kPlanErrArena = -13;    // an offset or extent outside the arena
constexpr int kPlanErrOutput = -14;   // an output index ≥ 60 or used twice
constexpr int kPlanErrPairs = -15;    // a pair outside the pair area or ≥ the input width

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
    if (kind < kPlanLinear || kind > kPlanKmeans || (flags & ~7)) return kPlanErrShape;
    if (e[kPlOut] < 0 || e[kPlOut] >= kPlanMaxModels || ((used >> e[kPlOut]) & 1ull))
      return kPlanErrOutput;
    used |= 1ull << e[kPlOut];
    if (ns < 0 || ns > kPlanMaxStages) return kPlanErrStages;
    int D = dn;
    for (int s = 0; s < ns; ++s) {
      const int* st = e + kPlStage0 + 4 * s;
      if (st[3] != D) return kPlanErrStages;
      if (st[0] == kPlanAffine) {
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
    if (kind == kPlanKmeans) {
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
