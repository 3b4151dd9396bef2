// CPU mirror of serve_plan_kernel (csrc/kernels/serving.hip): one point against a serving
// plan and its parameter arena, in plain C++. It is the oracle of the plan layout
// (csrc/kernels/serve_plan.h) on a machine without a GPU — the tests build a plan and an
// arena and compare this with Pipeline.predict — and is not on any runtime path.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../kernels/serve_plan.h"
#include "hashing.h"

#define OMLDM_HOST_API extern "C" __attribute__((visibility("default")))

using namespace omldm;

// num [dn] floats and cat [dc] int32 are the request line's payload: the compact uint16
// value (cspan > 0), the wide signed slot (cspan == 0) or the raw token (cspan < 0).
// out [60]: result[] as the wave would publish it (untouched where no model writes).
// Returns 0, or the plan_check code without touching out.
OMLDM_HOST_API int omldm_cpu_serve_plan(const int* plan, int n_models, const float* arena,
                                        long long arena_floats, int dn, int dc, int cspan,
                                        int dim, const float* num, const int* cat, float* out) {
  const int bad = plan_check(plan, n_models, arena_floats, dn, dc, dim);
  if (bad) return bad;
  // the decoded point
  int cidx[kPlanLanes];
  float cval[kPlanLanes];
  for (int j = 0; j < dc; ++j) {
    cidx[j] = -1;
    cval[j] = 0.f;
    const uint32_t u32 = (uint32_t)cat[j];
    if (cspan < 0) {
      if (u32 != omldm_hash::kAbsentToken) {
        const int32_t code = omldm_hash::hash_token(u32, j, dn, dc, dim);
        cidx[j] = code & 0x7fffffff;
        cval[j] = code < 0 ? -1.f : 1.f;
      }
    } else if (cspan > 0) {
      const unsigned u = u32 & 0xFFFFu;
      if (u != 0xFFFFu) {
        cidx[j] = dn + j * cspan + (int)(u & 0x7fffu);
        cval[j] = (u & 0x8000u) ? -1.f : 1.f;
      }
    } else if (cat[j] != -1) {
      cidx[j] = cat[j] & 0x7fffffff;
      cval[j] = cat[j] < 0 ? -1.f : 1.f;
    }
    if ((unsigned)cidx[j] >= (unsigned)dim) {
      cidx[j] = -1;
      cval[j] = 0.f;
    }
  }
  for (int m = 0; m < n_models; ++m) {
    const int* e = plan + (long long)m * kPlanWords;
    const int kind = e[kPlKind], flags = e[kPlFlags], width = e[kPlWidth], K = e[kPlK];
    const float* P = arena + e[kPlOff];
    float v[kPlanLanes];
    int D = dn;
    for (int j = 0; j < dn; ++j) v[j] = num[j];
    for (int s = 0; s < e[kPlStages]; ++s) {
      const int* st = e + kPlStage0 + 4 * s;
      if (st[0] == kPlanAffine) {
        for (int j = 0; j < D; ++j) v[j] = (v[j] - arena[st[1] + j]) / arena[st[2] + j];
      } else {
        const int np = D * (D + 1) / 2;
        for (int p = 0; p < np; ++p) {
          const int w = e[kPlPairs + st[1] + p];
          v[D + p] = v[w & 0xff] * v[w >> 8];
        }
        D += np;
      }
    }
    float r;
    if (kind == kPlanKmeans) {
      float bd = std::numeric_limits<float>::infinity();
      int best = 0;
      for (int c = 0; c < K; ++c) {
        float dd = 0.f;
        for (int f = 0; f < D; ++f) {
          const float t = v[f] - P[(size_t)c * width + f];
          dd = std::fmaf(t, t, dd);
        }
        if (dd < bd) {
          bd = dd;
          best = c;
        }
      }
      r = (float)best;
    } else {
      const int nc = (flags & kPlanFlagDense) ? 0 : dc;
      float best = -std::numeric_limits<float>::infinity();
      int bk = 0;
      float score = 0.f;
      for (int k = 0; k < K; ++k) {
        const float* w = P + (size_t)k * width;
        float acc = 0.f;
        for (int j = 0; j < D; ++j)
          if (j < width) acc += v[j] * w[j];
        for (int j = 0; j < nc; ++j)
          if (cidx[j] >= 0 && cidx[j] < width) acc += cval[j] * w[cidx[j]];
        if (flags & kPlanFlagBias) acc += w[width - 1];
        if (k == 0) score = acc;
        if (acc > best) {
          best = acc;
          bk = k;
        }
      }
      if (kind == kPlanLinear)
        r = (flags & kPlanFlagSign) ? (score >= 0.f ? 1.f : -1.f) : score;
      else
        r = (float)bk;
    }
    out[e[kPlOut]] = r;
  }
  return 0;
}
