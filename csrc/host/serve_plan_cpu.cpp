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

// kPlanMlp: unit j of a layer is b[j], then one fma per input in index order into a single
// accumulator — the wave's arithmetic (plan_mlp, serving.hip), so relu / identity networks
// agree bit for bit. P: Wt_0 [w_0 × w_1] input-major, b_0, Wt_1, …
static float mlp_forward(const int* e, const float* P, const float* v) {
  const int* a = e + kPlAux;
  const int L = a[0], act = a[1], task = a[2];
  float h[kPlanLanes], g[kPlanLanes];
  int win = a[3];
  for (int j = 0; j < win; ++j) h[j] = v[j];
  for (int l = 0; l < L; ++l) {
    const int wout = a[4 + l];
    const float* b = P + (size_t)win * wout;
    for (int j = 0; j < wout; ++j) {
      float acc = b[j];
      for (int i = 0; i < win; ++i) acc = std::fmaf(P[(size_t)i * wout + j], h[i], acc);
      if (l + 1 < L) {
        if (act == 0) acc = std::fmax(acc, 0.f);
        else if (act == 1) acc = std::tanh(acc);
        else if (act == 2) acc = 1.f / (1.f + std::exp(-acc));
      }
      g[j] = acc;
    }
    for (int j = 0; j < wout; ++j) h[j] = g[j];
    P += (size_t)win * wout + wout;
    win = wout;
  }
  if (task == 0) return h[0];
  if (task == 1) return h[0] >= 0.f ? 1.f : -1.f;
  int best = 0;
  for (int j = 1; j < win; ++j)
    if (h[j] > h[best]) best = j;
  return (float)best;
}

// kPlanTree: the successor of every node for this point, then the chain from node 0 for at
// most depth + 1 steps (depth clamped to the node limit), then the majority class of the
// reached node — the stop rules and the bound of plan_tree (serving.hip). Every index is
// range-checked as a float before it is converted (a NaN or a huge value stops the walk).
static float tree_predict(const int* e, const float* P, const float* v, int D, bool lazy) {
  const int* a = e + kPlAux;
  const int N = a[0], C = a[1];
  const int steps = (a[2] < kPlanTreeMaxNodes ? a[2] : kPlanTreeMaxNodes) + 1;
  const float *feat = P, *thr = P + N, *left = P + 2 * (size_t)N, *right = P + 3 * (size_t)N;
  const float* cc = P + 4 * (size_t)N;
  // behind a lazy poly2 stage: D lanes, then the D(D+1)/2 pair products (poly2_pair)
  const int DF = lazy ? D + D * (D + 1) / 2 : D;
  int node = 0;
  for (int it = 0; it < steps; ++it) {
    const float ff = feat[node];
    if (!(ff >= 0.f && ff < (float)DF)) break;
    const int f = (int)ff;
    float x;
    if (f < D) {
      x = v[f];
    } else {
      int a2, b2;
      poly2_pair(f - D, D, &a2, &b2);
      x = v[a2] * v[b2];
    }
    const float ch = x <= thr[node] ? left[node] : right[node];
    if (!(ch >= 0.f && ch < (float)N)) break;
    node = (int)ch;
  }
  const float* cn = cc + (size_t)node * C;
  int best = 0;
  for (int c = 1; c < C; ++c)
    if (cn[c] > cn[best]) best = c;
  return (float)best;
}

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
    bool lazy = false;
    for (int s = 0; s < e[kPlStages]; ++s) {
      const int* st = e + kPlStage0 + 4 * s;
      if (st[0] == kPlanPoly2Lazy) {
        lazy = true;
      } else if (st[0] == kPlanAffine) {
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
    if (kind == kPlanMlp) {
      r = mlp_forward(e, P, v);
    } else if (kind == kPlanTree) {
      r = tree_predict(e, P, v, D, lazy);
    } else if (kind == kPlanKmeans) {
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
