// Low-latency forecasting: a persistent predict wavefront fed through a host mailbox.
//
// Reference path: forecasting record → FlinkSpoke → learner predict → Prediction side
// output → predictions topic (omldm/operators/spoke/FlinkSpoke.scala:105,
// omldm/network/FlinkNetwork.scala:250); its latency is a Flink task hop + JVM call.
// Here one resident wavefront polls a 256-byte request line in fine-grained (coherent),
// pinned host memory. Every poll is ONE wave-wide PCIe read of the whole line (lane l
// loads dword l): sequence number, checksum and the point itself — so a new request is
// picked up together with its payload in a single round trip instead of "read sequence,
// then read payload". The host writes the payload, then a position-mixed checksum keyed
// by the sequence, then the sequence (release); a torn read (new sequence, stale payload)
// fails the checksum and is simply re-polled. The wave scores the point against M models
// (same feature decoding as the training kernel) and publishes scores + the completion
// sequence with system-scope stores. No kernel launch or stream sync per request.
// cspan < 0: the request carries raw 32-bit category tokens (the binary wire), hashed by
// the wave itself (hash_dev.h) — the same hash as the training round.
//
// Model versions: the wave reads one of two weight banks, chosen per request by the
// request line's last dword (lane 63, covered by the checksum). The engine publishes each
// round's models into the bank no request is reading and switches requests to it once the
// publishing copy has completed (engine/forecast_server.py), so a prediction never sees a
// model that is half-way through an update.
//
// Safety: the wave exits on the stop word or after `lifetime_us` of wall time
// (s_memrealtime, 100 MHz), whichever comes first; every spin is bounded by it.
//
// Two kernels share the mailbox, the request line and the host side of a request:
// * serve_kernel: M hashed-linear rows of one weight matrix (omldm_serve_start);
// * serve_plan_kernel: a plan (serve_plan.h), one entry per pipeline — StandardScaler /
//   MinMaxScaler (a per-lane (x − shift) / div) and PolynomialFeatures(2) (a product of two
//   lanes) in front of a hashed-linear or dense ridge row, the K rows of a MultiClassPA
//   (argmax on the device), the k centroids of a K-means (argmin on the device), a small MLP
//   (≤ 4 layers of ≤ 64 units) or a Hoeffding tree (≤ 1024 nodes, ≤ 32 classes), all
//   evaluated by the one wave from the request line it already holds
//   (omldm_serve_plan_start; CPU mirror: csrc/host/serve_plan_cpu.cpp).
#include "common.h"
#include "hash_dev.h"
#include "serve_plan.h"

#include <chrono>
#include <cstdlib>
#include <cstring>

namespace omldm {

constexpr int kReqWords = 64;  // request line: [seq, csum, payload (dn + dc dwords), …, bank]
constexpr int kBankWord = kReqWords - 1;

struct alignas(256) Mailbox {
  unsigned int req[kReqWords];  // host → device (one 256-B line)
  unsigned int seq_done;        // device → host: last completed sequence number
  unsigned int stop;            // host → device: exit request
  unsigned int alive;           // device → host: 1 while the wave is polling
  unsigned int exit_reason;     // device → host: 1 stop word, 2 lifetime expired
  float result[60];             // scores of up to 60 models
  unsigned long long t_start, t_exit, t_end;  // diagnostics (100 MHz clock)
};

template <typename T>
__device__ __forceinline__ T sys_load(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <typename T>
__device__ __forceinline__ void sys_store(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ unsigned long long rt_now() {
  return __builtin_amdgcn_s_memrealtime();  // 100 MHz constant clock
}

__host__ __device__ __forceinline__ uint32_t line_mix(uint32_t d, uint32_t pos) {
  uint32_t h = d + pos * 0x9E3779B9u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

template <typename WT, bool GROUPED>
__global__ __launch_bounds__(64) void serve_kernel(const WT* __restrict__ w0,
                                                   const WT* __restrict__ w1, long long wstride,
                                                   int M, int dn, int dc, int dim, int bias,
                                                   int cspan, Mailbox* mb,
                                                   unsigned long long lifetime_ticks) {
  const int lane = threadIdx.x;
  const int nf = dn + dc;
  const unsigned long long t_end = rt_now() + lifetime_ticks;
  unsigned int last = sys_load(&mb->req[0]);
  if (lane == 0) {
    sys_store(&mb->t_start, t_end - lifetime_ticks);
    sys_store(&mb->t_end, t_end);
    sys_store(&mb->alive, 1u);
  }
  int polls = 0;
  while (true) {
    const unsigned int d = sys_load(&mb->req[lane]);  // the whole line in one read
    const unsigned int seq = __builtin_amdgcn_readfirstlane(d);
    if (seq == last) {
      if (++polls >= 64) {  // re-check the clock / stop word every 64 polls
        polls = 0;
        bool quit = false;
        if (lane == 0) {
          const bool st = sys_load(&mb->stop) != 0u;
          const bool late = rt_now() > t_end;
          quit = st || late;
          if (quit) {
            sys_store(&mb->exit_reason, st ? 1u : 2u);
            sys_store(&mb->t_exit, rt_now());
          }
        }
        if (__builtin_amdgcn_readfirstlane(quit ? 1 : 0)) break;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    // checksum over the payload lanes (position-mixed), keyed by the sequence
    const bool pl = (lane >= 2 && lane < 2 + nf) || lane == kBankWord;
    const uint32_t x = wave_xor(pl ? line_mix(d, (uint32_t)lane) : 0u) ^ line_mix(seq, 0u);
    const uint32_t csum = (uint32_t)__shfl((int)d, 1, 64);
    if (__builtin_amdgcn_readfirstlane(x == csum ? 1 : 0) == 0) continue;  // torn: re-poll
    const WT* __restrict__ w = __builtin_amdgcn_readlane((int)d, kBankWord) ? w1 : w0;
    // lane j ← payload dword j (feature j)
    const unsigned int fj = (unsigned int)__shfl((int)d, (lane + 2) & 63, 64);
    int idx = -1;
    float v = 0.f;
    const int j = lane;
    if (j == nf && bias) {
      idx = dim - 1;
      v = 1.f;
    } else if (j < dn) {
      idx = j;
      v = __uint_as_float(fj);
    } else if (j < nf) {
      const int c = (int)fj;
      if (cspan < 0) {  // raw binary wire: the 32-bit category token, hashed here
        const int code = hash_token_dev(fj, j - dn, dn, (uint32_t)((dim - dn - 1) / dc));
        if (code != -1) {
          idx = code & 0x7fffffff;
          v = code < 0 ? -1.f : 1.f;
        }
      } else if (cspan > 0) {
        const unsigned u = (unsigned)c & 0xFFFFu;
        if (u != 0xFFFFu) {
          idx = dn + (j - dn) * cspan + (int)(u & 0x7fffu);
          v = (u & 0x8000u) ? -1.f : 1.f;
        }
      } else if (c != -1) {
        idx = c & 0x7fffffff;
        v = c < 0 ? -1.f : 1.f;
      }
    }
    if ((unsigned)idx >= (unsigned)dim) {
      idx = -1;
      v = 0.f;
    }
    if constexpr (GROUPED) {
      // Models in groups of 16: the group's 16 gathers are issued back to back (one HBM
      // round trip per group, not per model), then reduced; lane m keeps model m's
      // score and the wave publishes all M scores with ONE wave-wide store.
      float mine = 0.f;
      for (int m0 = 0; m0 < M; m0 += 16) {
        float g[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
          g[k] = (idx >= 0 && m0 + k < M) ? to_f(w[(size_t)(m0 + k) * wstride + idx]) : 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (m0 + k < M) {  // wave-uniform: no reductions for absent models
            const float sk = wave_sum(v * g[k]);
            if (lane == m0 + k) mine = sk;
          }
        }
      }
      if (lane < M) sys_store(&mb->result[lane], mine);
    } else {  // one model: gather, reduce, lane 0 publishes
      for (int m = 0; m < M; ++m) {
        float acc = idx >= 0 ? v * to_f(w[(size_t)m * wstride + idx]) : 0.f;
        acc = wave_sum(acc);
        if (lane == 0) sys_store(&mb->result[m], acc);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (lane == 0) sys_store(&mb->seq_done, seq);
    last = seq;
    polls = 0;
  }
  if (lane == 0) sys_store(&mb->alive, 0u);
}

// ---- the plan-driven wave ---------------------------------------------------------------
// The same mailbox protocol, but each model is a plan entry (serve_plan.h): preprocessor
// stages on the dense lanes, then a hashed or dense dot product, K hashed dot products and an
// argmax, or k centroid distances and an argmin. The parameters come from one of two fp32
// arenas (the request's bank word); the plan itself is copied into LDS when the wave starts.
// Every plan entry was validated by omldm_serve_plan_start; the kernel still checks each
// gather index against its region's width, as serve_kernel checks idx against dim.
__device__ __forceinline__ int plan_word(const int* e, int i) {
  return __builtin_amdgcn_readfirstlane(e[i]);
}

// ---- kPlanMlp / kPlanTree (the NL instantiation of serve_plan_kernel only) ------------------
__device__ __forceinline__ float plan_act(float v, int act) {
  switch (act) {
    case 0: return fmaxf(v, 0.f);
    case 1: return tanhf(v);
    case 2: return 1.f / (1.f + expf(-v));
    default: return v;
  }
}

// A multi-layer perceptron of at most 4 layers of at most 64 units. Lane j owns unit j of the
// current layer: acc = b[j], then one fma per input i in index order (a single accumulator —
// the arithmetic of the CPU mirror), h_i broadcast from lane i with a wave-uniform readlane.
// Wt is input-major, so for a fixed i the lanes read consecutive floats; a layer's loads (its
// bias and its ≤ 64 rows) are all issued before its fma chain: one round trip per layer.
// The next layer's rows are not prefetched during the chain: its extents depend on nothing
// but the plan, yet holding two layers' rows would double the live registers for a chain of
// ≤ 64 fmas (≈ 0.1 µs) — the loads of a ≤ 17 KB layer are L2 hits after the first request.
__device__ __forceinline__ float plan_mlp(const float* __restrict__ A, const int* e, int off,
                                          int width, float v, int D, int lane) {
  const int* a = e + kPlAux;
  const int L = min(plan_word(a, 0), kPlanMlpMaxLayers);
  const int act = plan_word(a, 1), task = plan_word(a, 2);
  int win = min(plan_word(a, 3), kPlanLanes);
  float h = lane < min(D, win) ? v : 0.f;
  long long o = off;
  const long long end = (long long)off + width;
  float acc = 0.f;
  int wout = 1;
  for (int l = 0; l < L; ++l) {
    wout = min(max(plan_word(a, 4 + l), 1), kPlanLanes);
    if (o < 0 || o + (long long)win * wout + wout > end) return 0.f;  // outside the region
    const float* __restrict__ W = A + o;
    const bool on = lane < wout;
    acc = on ? W[win * wout + lane] : 0.f;
    float wv[kPlanLanes];
#pragma unroll
    for (int i = 0; i < kPlanLanes; ++i) wv[i] = (on && i < win) ? W[i * wout + lane] : 0.f;
#pragma unroll
    for (int i = 0; i < kPlanLanes; ++i) {
      if (i < win) acc = fmaf(wv[i], readlane_f(h, i), acc);  // wave-uniform
    }
    if (l + 1 < L) acc = plan_act(acc, act);
    h = on ? acc : 0.f;
    o += (long long)win * wout + wout;
    win = wout;
  }
  const float s0 = readlane_f(h, 0);
  if (task == 0) return s0;
  if (task == 1) return s0 >= 0.f ? 1.f : -1.f;
  float bv = lane < wout ? h : -INFINITY;  // argmax over the outputs, the lowest index on a tie
  int bi = lane < wout ? lane : 0x7fffffff;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const float ov = __shfl_xor(bv, s, 64);
    const int oi = __shfl_xor(bi, s, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  bi = __builtin_amdgcn_readfirstlane(bi);
  return (unsigned)bi < (unsigned)wout ? (float)bi : 0.f;
}

// A Hoeffding tree (the head of HT.state: feat, thr, left, right, cc). A node-by-node walk of
// the arena is two dependent global loads per level; instead every lane loads its nodes
// lane, lane + 64, … of the four arrays in one round trip, decides each node's successor for
// this point (x[f] ≤ thr ? left : right; "stop" on a leaf, on a feature outside [0, D) — or
// [0, D + D(D+1)/2) behind a lazy poly2 stage — or a child outside [0, N)) and writes it to LDS; the chain from node 0 is then followed through
// LDS for at most depth + 1 steps (ht_route's bound; depth is clamped to the node limit — a
// path in a tree of ≤ 1024 nodes is shorter). The reached node's class counts are read by C
// lanes; argmax, the lowest class on a tie (ht_predict_kernel).
__device__ __forceinline__ float plan_tree(const float* __restrict__ A, const int* e, int off,
                                           int width, float v, int D, bool lazy, int lane,
                                           short* s_next) {
  const int* a = e + kPlAux;
  const int N = min(max(plan_word(a, 0), 1), kPlanTreeMaxNodes);
  const int C = min(max(plan_word(a, 1), 1), kPlanTreeMaxClasses);
  const int steps = min(max(plan_word(a, 2), 0), kPlanTreeMaxNodes) + 1;
  if (off < 0 || (long long)N * (4 + C) > width) return 0.f;  // outside the region
  const float* __restrict__ T = A + off;
  constexpr int kPer = kPlanTreeMaxNodes / kPlanLanes;
  float nf[kPer], nt[kPer], nl[kPer], nr[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int n = u * kPlanLanes + lane;
    const bool on = n < N;
    nf[u] = on ? T[n] : -1.f;
    nt[u] = on ? T[N + n] : 0.f;
    nl[u] = on ? T[2 * N + n] : -1.f;
    nr[u] = on ? T[3 * N + n] : -1.f;
  }
  const float xv = lane < D ? v : 0.f;
  // behind a lazy poly2 stage (wave-uniform) the features are the D lanes, then the
  // D(D+1)/2 pair products: feature D + p = lane a · lane b of pair p (poly2_pair)
  const int DF = lazy ? D + D * (D + 1) / 2 : D;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    if (u * kPlanLanes < N) {  // wave-uniform
      const int n = u * kPlanLanes + lane;
      const bool inner = nf[u] >= 0.f && nf[u] < (float)DF;
      const int f = inner ? (int)nf[u] : 0;
      int fa = f, fb = -1;
      if (f >= D) poly2_pair(f - D, D, &fa, &fb);
      float x = __shfl(xv, fa & 63, 64);
      if (lazy) {  // wave-uniform: the shuffle runs in every lane
        const float xb = __shfl(xv, fb & 63, 64);
        if (fb >= 0) x *= xb;
      }
      const float ch = x <= nt[u] ? nl[u] : nr[u];
      const bool go = inner && ch >= 0.f && ch < (float)N;
      if (n < N) s_next[n] = go ? (short)(int)ch : (short)-1;
    }
  }
  __syncthreads();
  int node = 0;
  for (int it = 0; it < steps; ++it) {
    const int nx = s_next[node];  // the same address in every lane: one LDS broadcast
    if (nx < 0) break;
    node = nx;
  }
  node = __builtin_amdgcn_readfirstlane(node);
  __syncthreads();  // the next tree entry rewrites s_next
  float bv = lane < C ? T[(size_t)4 * N + (size_t)node * C + lane] : -INFINITY;
  int bi = lane < C ? lane : 0x7fffffff;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const float ov = __shfl_xor(bv, s, 64);
    const int oi = __shfl_xor(bi, s, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  bi = __builtin_amdgcn_readfirstlane(bi);
  return (unsigned)bi < (unsigned)C ? (float)bi : 0.f;
}

// NL: the instantiation that also knows kPlanMlp and kPlanTree entries (and holds the tree's
// successor table in LDS); a plan without them runs the other one.
template <bool NL>
__global__ __launch_bounds__(64) void serve_plan_kernel(const int* __restrict__ plan, int M,
                                                        const float* __restrict__ a0,
                                                        const float* __restrict__ a1, int dn, int dc,
                                                        int dim, int cspan, Mailbox* mb,
                                                        unsigned long long lifetime_ticks) {
  __shared__ int s_plan[kPlanMaxModels * kPlanWords];
  const int lane = threadIdx.x;
  const int nf = dn + dc;
  for (int i = lane; i < M * kPlanWords; i += 64) s_plan[i] = plan[i];
  __syncthreads();
  const unsigned long long t_end = rt_now() + lifetime_ticks;
  unsigned int last = sys_load(&mb->req[0]);
  if (lane == 0) {
    sys_store(&mb->t_start, t_end - lifetime_ticks);
    sys_store(&mb->t_end, t_end);
    sys_store(&mb->alive, 1u);
  }
  int polls = 0;
  while (true) {
    const unsigned int d = sys_load(&mb->req[lane]);  // the whole line in one read
    const unsigned int seq = __builtin_amdgcn_readfirstlane(d);
    if (seq == last) {
      if (++polls >= 64) {  // re-check the clock / stop word every 64 polls
        polls = 0;
        bool quit = false;
        if (lane == 0) {
          const bool st = sys_load(&mb->stop) != 0u;
          const bool late = rt_now() > t_end;
          quit = st || late;
          if (quit) {
            sys_store(&mb->exit_reason, st ? 1u : 2u);
            sys_store(&mb->t_exit, rt_now());
          }
        }
        if (__builtin_amdgcn_readfirstlane(quit ? 1 : 0)) break;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    const bool pl = (lane >= 2 && lane < 2 + nf) || lane == kBankWord;
    const uint32_t x = wave_xor(pl ? line_mix(d, (uint32_t)lane) : 0u) ^ line_mix(seq, 0u);
    const uint32_t csum = (uint32_t)__shfl((int)d, 1, 64);
    if (__builtin_amdgcn_readfirstlane(x == csum ? 1 : 0) == 0) continue;  // torn: re-poll
    const float* __restrict__ A = __builtin_amdgcn_readlane((int)d, kBankWord) ? a1 : a0;
    // the decoded point: lane j < dn holds numerical value j, lanes [dn, nf) their field's
    // hashed slot and sign (decoded once, as serve_kernel does; the same for every model)
    const unsigned int fj = (unsigned int)__shfl((int)d, (lane + 2) & 63, 64);
    const float x0 = lane < dn ? __uint_as_float(fj) : 0.f;
    int cidx = -1;
    float cval = 0.f;
    if (lane >= dn && lane < nf) {
      const int c = (int)fj;
      if (cspan < 0) {  // raw binary wire: the 32-bit category token, hashed here
        const int code = hash_token_dev(fj, lane - dn, dn, (uint32_t)((dim - dn - 1) / dc));
        if (code != -1) {
          cidx = code & 0x7fffffff;
          cval = code < 0 ? -1.f : 1.f;
        }
      } else if (cspan > 0) {
        const unsigned u = (unsigned)c & 0xFFFFu;
        if (u != 0xFFFFu) {
          cidx = dn + (lane - dn) * cspan + (int)(u & 0x7fffu);
          cval = (u & 0x8000u) ? -1.f : 1.f;
        }
      } else if (c != -1) {
        cidx = c & 0x7fffffff;
        cval = c < 0 ? -1.f : 1.f;
      }
    }
    float mine = 0.f;  // lane o keeps the result of the model whose output index is o
    bool has = false;
    for (int m = 0; m < M; ++m) {
      const int* e = s_plan + m * kPlanWords;
      const int kind = plan_word(e, kPlKind), flags = plan_word(e, kPlFlags);
      const int ns = min(plan_word(e, kPlStages), kPlanMaxStages);
      const int off = plan_word(e, kPlOff), width = plan_word(e, kPlWidth);
      const int K = plan_word(e, kPlK);
      // stages, on the dense lanes only
      float v = x0;
      int D = dn;
      [[maybe_unused]] bool lazy = false;
      for (int s = 0; s < ns; ++s) {
        const int* st = e + kPlStage0 + 4 * s;
        const int type = plan_word(st, 0), pa = plan_word(st, 1), pb = plan_word(st, 2);
        if (NL && type == kPlanPoly2Lazy) {
          lazy = true;  // (a tree's last stage: the products are taken per node, plan_tree)
        } else if (type == kPlanAffine) {
          if (lane < D) v = (v - A[pa + lane]) / A[pb + lane];
        } else {  // kPlanPoly2: lanes [D, D + D(D+1)/2) take the pair products
          const int np = D * (D + 1) / 2;
          const int j = lane - D;
          const bool fresh = j >= 0 && j < np;
          const int pw = fresh ? e[kPlPairs + ((pa + j) & 63)] : 0;
          const float va = __shfl(v, pw & 63, 64), vb = __shfl(v, (pw >> 8) & 63, 64);
          if (fresh) v = va * vb;
          D = min(D + np, kPlanLanes);
        }
      }
      float r;
      bool nonlinear = false;
      if constexpr (NL) {
        __shared__ short s_next[kPlanTreeMaxNodes];
        if (kind == kPlanMlp) {
          r = plan_mlp(A, e, off, width, v, D, lane);
          nonlinear = true;
        } else if (kind == kPlanTree) {
          r = plan_tree(A, e, off, width, v, D, lazy, lane, s_next);
          nonlinear = true;
        }
      }
      if (nonlinear) {
      } else if (kind == kPlanKmeans) {
        // lane j owns centroid c0 + j; x_f is broadcast, the distance accumulates in column
        // order with one fma per column (the arithmetic of kmeans_assign_kernel)
        const int dd_w = min(D, width);
        float bd = INFINITY;
        int bi = 0x7fffffff;
        for (int c0 = 0; c0 < K; c0 += 64) {
          const int c = c0 + lane;
          const bool on = c < K;
          const float* __restrict__ cr = A + off + (size_t)(on ? c : 0) * width;
          float dd = 0.f;
          for (int f0 = 0; f0 < dd_w; f0 += 8) {  // 8 loads in flight, then the fma chain
            float cf[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) cf[u] = f0 + u < dd_w ? cr[f0 + u] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              if (f0 + u < dd_w) {
                const float t = readlane_f(v, f0 + u) - cf[u];
                dd = fmaf(t, t, dd);
              }
            }
          }
          if (on && dd < bd) {
            bd = dd;
            bi = c;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // wave argmin, the lowest index wins a tie
          const float od = __shfl_xor(bd, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (od < bd || (od == bd && oi < bi)) {
            bd = od;
            bi = oi;
          }
        }
        r = bi == 0x7fffffff ? 0.f : (float)bi;
      } else {
        // lanes [0, D) dense, [D, D + dc) the categorical slots (they keep their slots
        // however wide the dense block became), then the bias lane
        const int nc = (flags & kPlanFlagDense) ? 0 : dc;
        const int src = (lane - D + dn) & 63;
        const int ci = __shfl(cidx, src, 64);
        const float cf = __shfl(cval, src, 64);
        int idx = -1;
        float val = 0.f;
        if (lane < D) {
          idx = lane;
          val = v;
        } else if (lane < D + nc) {
          idx = ci;
          val = cf;
        } else if (lane == D + nc && (flags & kPlanFlagBias)) {
          idx = width - 1;
          val = 1.f;
        }
        if ((unsigned)idx >= (unsigned)width) {
          idx = -1;
          val = 0.f;
        }
        if (kind == kPlanLinear) {
          r = wave_sum(idx >= 0 ? val * A[off + idx] : 0.f);
          if (flags & kPlanFlagSign) r = r >= 0.f ? 1.f : -1.f;
        } else {  // kPlanMulticlass: K rows, gathers in groups of 16, argmax (lowest index)
          float best = -INFINITY;
          int bk = 0;
          for (int k0 = 0; k0 < K; k0 += 16) {
            float g[16];
#pragma unroll
            for (int k = 0; k < 16; ++k)
              g[k] = (idx >= 0 && k0 + k < K) ? A[off + (size_t)(k0 + k) * width + idx] : 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              if (k0 + k < K) {  // wave-uniform
                const float sk = wave_sum(val * g[k]);
                if (sk > best) {
                  best = sk;
                  bk = k0 + k;
                }
              }
            }
          }
          r = (float)bk;
        }
      }
      if (lane == plan_word(e, kPlOut)) {
        mine = r;
        has = true;
      }
    }
    if (has) sys_store(&mb->result[lane], mine);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (lane == 0) sys_store(&mb->seq_done, seq);
    last = seq;
    polls = 0;
  }
  if (lane == 0) sys_store(&mb->alive, 0u);
}

}  // namespace omldm

using namespace omldm;

OMLDM_API void* omldm_mailbox_alloc() {
  void* p = nullptr;
  if (hipHostMalloc(&p, sizeof(Mailbox), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    return nullptr;
  memset(p, 0, sizeof(Mailbox));
  return p;
}

OMLDM_API void omldm_mailbox_free(void* p) {
  if (p) hipHostFree(p);
}

// w1: the second weight bank (nullptr: the requests' bank 1 reads w as well).
OMLDM_API int omldm_serve_start(const void* w, const void* w1, int w_bf16, long long wstride,
                                int M, int dn, int dc, int dim, int bias, int cspan,
                                void* mailbox, long long lifetime_us, void* stream) {
  if (M < 1 || M > 60 || dn + dc > kReqWords - 3 || dn + dc + (bias ? 1 : 0) > 64) return -2;
  if (w1 == nullptr) w1 = w;
  Mailbox* hmb = (Mailbox*)mailbox;
  void* dmb = nullptr;
  if (hipHostGetDevicePointer(&dmb, mailbox, 0) != hipSuccess || !dmb) return -3;
  __atomic_store_n(&hmb->stop, 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(&hmb->exit_reason, 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(&hmb->alive, 0u, __ATOMIC_SEQ_CST);
  const unsigned long long ticks = (unsigned long long)lifetime_us * 100ull;  // 100 MHz
  // grouped gathers for several models; OMLDM_SERVE_GROUPED=0/1 forces a variant (A/B)
  bool grouped = M > 1;
  if (const char* e = getenv("OMLDM_SERVE_GROUPED")) grouped = e[0] == '1';
  hipStream_t st = (hipStream_t)stream;
#define OMLDM_SERVE(WT, G)                                                                   \
  hipLaunchKernelGGL((serve_kernel<WT, G>), dim3(1), dim3(64), 0, st, (const WT*)w,          \
                     (const WT*)w1, wstride, M,                                               \
                     dn, dc, dim, bias, cspan, (Mailbox*)dmb, ticks)
  if (w_bf16) {
    if (grouped) OMLDM_SERVE(__hip_bfloat16, true);
    else OMLDM_SERVE(__hip_bfloat16, false);
  } else {
    if (grouped) OMLDM_SERVE(float, true);
    else OMLDM_SERVE(float, false);
  }
#undef OMLDM_SERVE
  return (int)hipGetLastError();
}

// The plan-driven wave (serve_plan_kernel). plan: n_models entries (serve_plan.h) in pinned,
// mapped host memory — checked here, read once by the wave into LDS; arena0 / arena1: the two
// parameter banks of arena_floats floats each (arena1 nullptr: both banks read arena0).
// Returns a negative code (serve_plan.h) without launching when the plan is not safe to run.
OMLDM_API int omldm_serve_plan_start(const int* plan, int n_models, const float* arena0,
                                     const float* arena1, long long arena_floats, int dn, int dc,
                                     int cspan, int dim, void* mailbox, long long lifetime_us,
                                     void* stream) {
  const int bad = plan_check(plan, n_models, arena_floats, dn, dc, dim);
  if (bad) return bad;
  if (!arena0 || !mailbox) return kPlanErrShape;
  if (arena1 == nullptr) arena1 = arena0;
  Mailbox* hmb = (Mailbox*)mailbox;
  void *dmb = nullptr, *dplan = nullptr;
  if (hipHostGetDevicePointer(&dmb, mailbox, 0) != hipSuccess || !dmb) return -3;
  if (hipHostGetDevicePointer(&dplan, (void*)plan, 0) != hipSuccess || !dplan) return -3;
  __atomic_store_n(&hmb->stop, 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(&hmb->exit_reason, 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(&hmb->alive, 0u, __ATOMIC_SEQ_CST);
  const unsigned long long ticks = (unsigned long long)lifetime_us * 100ull;  // 100 MHz
  // a plan of linear / multi-class / k-means entries runs the instantiation without the MLP
  // and tree code (and without the tree's LDS table)
  if (plan_has_nonlinear(plan, n_models))
    hipLaunchKernelGGL(serve_plan_kernel<true>, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       (const int*)dplan, n_models, arena0, arena1, dn, dc, dim, cspan,
                       (Mailbox*)dmb, ticks);
  else
    hipLaunchKernelGGL(serve_plan_kernel<false>, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       (const int*)dplan, n_models, arena0, arena1, dn, dc, dim, cspan,
                       (Mailbox*)dmb, ticks);
  return (int)hipGetLastError();
}

// Host side of one request: payload → checksum → sequence (release), then a bounded spin
// on the completion sequence; copies the M scores out. Returns 0, or -1 on timeout.
OMLDM_API int omldm_serve_request(void* mailbox, const float* num, int dn, const int* cat, int dc,
                                  int M, float* out, long long timeout_us, int bank) {
  Mailbox* mb = (Mailbox*)mailbox;
  const unsigned int seq = __atomic_load_n(&mb->req[0], __ATOMIC_RELAXED) + 1u;
  uint32_t x = line_mix(seq, 0u);
  for (int j = 0; j < dn; ++j) {
    uint32_t u;
    std::memcpy(&u, &num[j], 4);
    __atomic_store_n(&mb->req[2 + j], u, __ATOMIC_RELAXED);
    x ^= line_mix(u, (uint32_t)(2 + j));
  }
  for (int j = 0; j < dc; ++j) {
    const uint32_t u = (uint32_t)cat[j];
    __atomic_store_n(&mb->req[2 + dn + j], u, __ATOMIC_RELAXED);
    x ^= line_mix(u, (uint32_t)(2 + dn + j));
  }
  const uint32_t bk = bank ? 1u : 0u;
  __atomic_store_n(&mb->req[kBankWord], bk, __ATOMIC_RELAXED);
  x ^= line_mix(bk, (uint32_t)kBankWord);
  __atomic_store_n(&mb->req[1], x, __ATOMIC_RELAXED);
  __atomic_store_n(&mb->req[0], seq, __ATOMIC_RELEASE);
  const auto t0 = std::chrono::steady_clock::now();
  while (__atomic_load_n(&mb->seq_done, __ATOMIC_ACQUIRE) != seq) {
    if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() -
                                                              t0).count() > timeout_us)
      return -1;
  }
  for (int m = 0; m < M; ++m) out[m] = mb->result[m];
  return 0;
}

OMLDM_API void omldm_serve_stop(void* mailbox) {
  __atomic_store_n(&((Mailbox*)mailbox)->stop, 1u, __ATOMIC_SEQ_CST);
}

OMLDM_API void omldm_serve_times(void* mailbox, unsigned long long* out3) {
  const Mailbox* m = (const Mailbox*)mailbox;
  out3[0] = m->t_start;
  out3[1] = m->t_exit;
  out3[2] = m->t_end;
}

OMLDM_API int omldm_serve_exit_reason(void* mailbox) {
  return (int)__atomic_load_n(&((Mailbox*)mailbox)->exit_reason, __ATOMIC_ACQUIRE);
}

OMLDM_API int omldm_serve_alive(void* mailbox) {
  return (int)__atomic_load_n(&((Mailbox*)mailbox)->alive, __ATOMIC_ACQUIRE);
}

// The published-bank word of the native forecast lane (csrc/host/fcst_lane.cpp): a pinned
// coherent host word the GPU writes after a publish copy, in stream order
// (hipStreamWriteValue32), so the lane switches banks only once the copy has completed.
OMLDM_API void* omldm_bank_word_alloc() {
  void* p = nullptr;
  if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    return nullptr;
  memset(p, 0, 64);
  return p;
}

OMLDM_API void omldm_bank_word_free(void* p) {
  if (p) hipHostFree(p);
}

OMLDM_API int omldm_bank_word_set(void* word, unsigned int v, void* stream) {
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, word, 0) != hipSuccess || !d) return -3;
  return (int)hipStreamWriteValue32((hipStream_t)stream, d, v, 0);
}
