// Stand-alone self-test of the serving plan's CPU mirror (csrc/host/serve_plan_cpu.cpp) on
// hostile tree arenas, meant to be built with -fsanitize=address,undefined
// (tests/test_serving_plan_nonlinear_cpu.py). Every arena is a heap block of exactly the
// plan's extent, so a read outside a region is a sanitizer report. Each call must return 0
// with a class in [0, C): children out of range, self-loops under the largest depth word,
// features ≥ D (also behind a lazy poly2 stage), NaN thresholds / features / children. An MLP
// entry of the largest shape runs once for the same extent check.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../kernels/serve_plan.h"

extern "C" int omldm_cpu_serve_plan(const int* plan, int n_models, const float* arena,
                                    long long arena_floats, int dn, int dc, int cspan, int dim,
                                    const float* num, const int* cat, float* out);

using namespace omldm;

static int failures = 0;

static void expect(bool ok, const char* what, int a = 0, float b = 0.f) {
  if (!ok) {
    std::printf("FAIL %s (%d, %g)\n", what, a, b);
    ++failures;
  }
}

constexpr int kDn = 4, kDim = 16;

struct Tree {
  int N, C, depth;
  std::vector<float> a;  // feat, thr, left, right, cc
  Tree(int n, int c, int d) : N(n), C(c), depth(d), a((size_t)n * (4 + c), 0.f) {
    for (int i = 0; i < n; ++i) a[i] = -1.f;  // all leaves
    for (int i = 0; i < n * c; ++i) a[4 * (size_t)n + i] = (float)((i * 7) % 5);
  }
  float& feat(int i) { return a[i]; }
  float& thr(int i) { return a[N + i]; }
  float& left(int i) { return a[2 * N + i]; }
  float& right(int i) { return a[3 * N + i]; }
};

static void run(Tree& t, const char* what, bool lazy = false) {
  std::vector<int> plan(kPlanWords, 0);
  plan[kPlKind] = kPlanTree;
  if (lazy) {  // a lazy poly2 stage: 4 lanes, 4 + 10 features
    plan[kPlStages] = 1;
    plan[kPlStage0] = kPlanPoly2Lazy;
    plan[kPlStage0 + 3] = kDn;
  }
  plan[kPlWidth] = t.N * (4 + t.C);
  plan[kPlK] = 1;
  plan[kPlAux] = t.N;
  plan[kPlAux + 1] = t.C;
  plan[kPlAux + 2] = t.depth;
  const float pts[3][kDn] = {{0.f, 0.f, 0.f, 0.f},
                             {-3.f, 2.f, 1e30f, -1e30f},
                             {std::numeric_limits<float>::quiet_NaN(), 1.f, -1.f, 5.f}};
  for (const auto& p : pts) {
    float out[kPlanMaxModels];
    for (float& o : out) o = -7.f;
    const int rc = omldm_cpu_serve_plan(plan.data(), 1, t.a.data(), (long long)t.a.size(), kDn, 0,
                                        0, kDim, p, nullptr, out);
    expect(rc == 0, what, rc);
    expect(out[0] >= 0.f && out[0] < (float)t.C && out[0] == std::floor(out[0]), what, rc,
           out[0]);
    expect(out[1] == -7.f, "only the entry's output is written");
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const int big = std::numeric_limits<int>::max();
  {  // children out of range
    const float bad[] = {8.f, 100.f, -1.f, -5.f, 1e30f, -1e30f, inf, -inf, 2147483648.f};
    for (float l : bad)
      for (float r : bad) {
        Tree t(8, 3, 12);
        t.feat(0) = 1.f;
        t.left(0) = l;
        t.right(0) = r;
        run(t, "children out of range");
      }
  }
  for (int depth : {0, 1, 12, 1024, 1025, big}) {  // self-loops, and a two-node cycle
    Tree t(8, 3, depth);
    for (int i = 0; i < 8; ++i) {
      t.feat(i) = (float)(i % kDn);
      t.left(i) = t.right(i) = (float)i;
    }
    run(t, "self-loops");
    t.left(0) = t.right(0) = 1.f;
    t.left(1) = t.right(1) = 0.f;
    run(t, "a cycle");
  }
  for (float f : {4.f, 63.f, 64.f, 1e9f, 2147483648.f, inf, nan, -0.5f, -inf}) {  // f ≥ D …
    Tree t(8, 3, 12);
    t.feat(0) = f;
    t.left(0) = 1.f;
    t.right(0) = 2.f;
    run(t, "feature outside [0, D)");
  }
  for (float f : {0.f, 3.f, 4.f, 7.f, 8.f, 13.f, 14.f, 15.f, 1e9f, inf, nan}) {  // lazy poly2
    Tree t(8, 3, 12);
    t.feat(0) = f;
    t.thr(0) = 0.5f;
    t.left(0) = 1.f;
    t.right(0) = 2.f;
    run(t, "lazy poly2 features", true);
  }
  {  // NaN thresholds and children
    Tree t(7, 2, big);
    for (int i = 0; i < 3; ++i) {
      t.feat(i) = (float)i;
      t.thr(i) = nan;
      t.left(i) = (float)(2 * i + 1);
      t.right(i) = (float)(2 * i + 2);
    }
    run(t, "NaN thresholds");
    t.left(2) = nan;
    t.right(2) = nan;
    t.right(0) = 2.f;
    run(t, "NaN children");
  }
  {  // the largest tree: 1024 nodes, 32 classes, one long right-leaning chain
    Tree t(kPlanTreeMaxNodes, kPlanTreeMaxClasses, big);
    for (int i = 0; i + 1 < t.N; ++i) {
      t.feat(i) = (float)(i % kDn);
      t.thr(i) = -inf;
      t.left(i) = 0.f;
      t.right(i) = (float)(i + 1);
    }
    run(t, "the largest tree");
  }
  {  // an MLP of the largest shape against an arena of exactly its extent
    const int w[5] = {kDn, 64, 64, 64, 64};
    size_t floats = 0;
    for (int l = 0; l < 4; ++l) floats += (size_t)w[l] * w[l + 1] + w[l + 1];
    std::vector<float> arena(floats);
    for (size_t i = 0; i < floats; ++i) arena[i] = (float)((int)(i % 13) - 6) * 0.03f;
    for (int act = 0; act < 4; ++act)
      for (int task = 0; task < 3; ++task) {
        std::vector<int> plan(kPlanWords, 0);
        plan[kPlKind] = kPlanMlp;
        plan[kPlWidth] = (int)floats;
        plan[kPlK] = 1;
        plan[kPlAux] = 4;
        plan[kPlAux + 1] = act;
        plan[kPlAux + 2] = task;
        for (int l = 0; l < 5; ++l) plan[kPlAux + 3 + l] = w[l];
        const float p[kDn] = {0.5f, -1.f, 2.f, 0.f};
        float out[kPlanMaxModels] = {0};
        int rc = omldm_cpu_serve_plan(plan.data(), 1, arena.data(), (long long)floats, kDn, 0, 0,
                                      kDim, p, nullptr, out);
        expect(rc == 0 && std::isfinite(out[0]), "mlp", rc, out[0]);
        if (task == 2) expect(out[0] >= 0.f && out[0] < 64.f, "mlp class", rc, out[0]);
        rc = omldm_cpu_serve_plan(plan.data(), 1, arena.data(), (long long)floats - 1, kDn, 0, 0,
                                  kDim, p, nullptr, out);
        expect(rc == kPlanErrArena, "mlp region one float past the arena", rc);
      }
  }
  if (failures) {
    std::printf("serve plan selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("serve plan selftest OK\n");
  return 0;
}
