// NN learner: MLP training and inference on the matrix cores.
//
// Reference: the NN learner runs DL4J MultiLayerNetwork.fit on ND4J/OpenBLAS — GEMM,
// the row-wise bias broadcast that crashed (BaseLayer.preOutputWithPreNorm → doRowWise →
// execBroadcast, hs_err_pid77107.log:97-110), activations and an SGD step, each a
// separate native call per layer per mini-batch.
//
// Map of the file. One protocol round is one launch of a round kernel (+ the column sums),
// inference one launch of a forward kernel; omldm_mlp_plan picks both for a layer stack:
// * fused-32 (v1): mlp_round_kernel, 4 waves, and mlp_forward_kernel. The model sits in
//   LDS with widths zero-padded to 32; the loss is a serial pass per row, so any output
//   width goes. Takes the stacks whose 32-padded layout fits one CU's LDS and that
//   fused-16 does not take; its forward kernel serves every stack with that layout,
//   whichever kernel trains it.
// * fused-16 (v2, the default where it applies): mlp_round2_kernel, 16 waves. Widths
//   padded to 16, the loss fused into the last layer's epilogue, one barrier per
//   backward layer. Takes output widths ≤ 16 whose 16-padded layout (one more gradient
//   buffer and the bias gradients) fits.
// * streamed: mlp_round_stream_kernel, 16 waves, and mlp_forward_stream_kernel, 8 waves.
//   Only the mini-batch is in LDS, the weights stream from HBM. Takes what no fused layout
//   holds, up to kMlpLdsMax of activations, and everything under form 4.
// What the forms share:
// * the mini-batch: one workgroup = one virtual spoke running plain SGD over its row range
//   in steps of kMB = 32 rows (rows with a NaN label are left out, a step without labels
//   is skipped), every GEMM-shaped step on 16×16 MFMA tiles (gemm16p; the streamed forward
//   and dH read their weight operand from HBM instead):
//     forward   H_{l+1} = act(H_l · W_lᵀ + b_l)
//     backward  dH_l    = (dZ_{l+1} · W_l) ⊙ act'(H_l)   (derivative from the stored output)
//               W_l    -= η · dZ_{l+1}ᵀ · H_l             (from the accumulators: one owner
//                                                          lane per weight)
//   padded columns stay exactly zero through every step;
// * the flat layout of the parameter vector: per layer W_l [n_{l+1} × n_l] row-major, then
//   b_l (woff / boff) — what the protocol ships and the hub averages;
// * the delta hand-off: at round end a spoke writes Δ = W_spoke − W_0 into its row of the
//   S × nparams workspace, mlp_colsum_kernel folds the rows into dacc, and an apply pass
//   averages over the active spokes (omldm_multiclass_apply).
// LDS row strides are ≡ 4 floats mod 64 banks, so the 16-lane groups of a b128 operand read
// hit disjoint banks.
#include "common.h"

namespace omldm {

constexpr int kMB = 32;
constexpr int kT = 16;  // output tile of every GEMM: 16×16
constexpr int kMaxLayers = 4;

enum MlpAct : int { kRelu = 0, kTanh = 1, kSigmoid = 2, kIdentity = 3 };

struct MlpDesc {
  int L, task, K, act;  // act: hidden-layer activation (MlpAct)
  int bf16;             // 1: GEMM operands rounded to bf16 (v_mfma_f32_16x16x16_bf16)
  int n[kMaxLayers + 1], np[kMaxLayers + 1];
  int woff[kMaxLayers], boff[kMaxLayers];
  int lw[kMaxLayers], lb[kMaxLayers], ldw[kMaxLayers];
  int lh[kMaxLayers + 1], ldh[kMaxLayers + 1];
  int lg0, lg1, ldg, ly, total;
  // round kernel v2 (mlp_round2_kernel): bias-gradient accumulators per layer, three
  // rotating gradient buffers, a 4-float statistics scratch
  int lbg[kMaxLayers], lgb[3], lsc;
};

__device__ __forceinline__ short bf16_bits(float v) {
  return __builtin_bit_cast(short, __float2bfloat16(v));
}

// The tile product of every form: C[16×16] = A[16×K]·B[K×16] with A(i,k) = a[i·ars + k·acs],
// B(k,j) = b[k·brs + j·bcs] in LDS, on v_mfma_f32_16x16x4_f32 / v_mfma_f32_16x16x16_bf16
// (operands rounded to bf16, RNE, as they leave LDS; fp32 accumulation). A 32-row
// mini-batch against 64-wide layers is 8–16 such tiles per GEMM, so every wave of the
// spoke works in every phase. Lane l (i = l&15, g = l>>4) supplies, per 16-wide k step, the
// 4 consecutive k = k0 + 4g + u of its A row and B column — one b128 read where k is
// contiguous in LDS (AK: acs == 1, BK: brs == 1), one float per k otherwise; fp32 MFMA u
// takes value u (a permutation of the k sum), bf16 takes all four at once.
// acc[j] = C(4g + j, i).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));

// K a multiple of 16: operands read at the top of each 16-wide k step (issued while the
// previous step's MFMAs are in the pipe), the accumulator chained through the MFMAs in
// place — no register copies of it between steps (a copy waits for the matrix pipe to
// drain). BF = 0 / 1: the fp32 / bf16 instantiation (no branch in the loop); BF < 0: one
// loop that picks per k step by `bf16` (a uniform branch).
template <bool AK, bool BK, int BF>
__device__ __forceinline__ f32x4 gemm16t(const float* a, int ars, int acs, const float* b,
                                         int brs, int bcs, int K, int bf16 = 0) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* ap = a + r * ars + 4 * g * (AK ? 1 : acs);
  const float* bp = b + 4 * g * (BK ? 1 : brs) + r * bcs;
  for (int k = 0; k < K; k += 16) {
    float av[4], bv[4];
    if constexpr (AK) {
      const float4 t = *reinterpret_cast<const float4*>(ap + k);
      av[0] = t.x; av[1] = t.y; av[2] = t.z; av[3] = t.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) av[u] = ap[(k + u) * acs];
    }
    if constexpr (BK) {
      const float4 t = *reinterpret_cast<const float4*>(bp + k);
      bv[0] = t.x; bv[1] = t.y; bv[2] = t.z; bv[3] = t.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) bv[u] = bp[(k + u) * brs];
    }
    if (BF < 0 ? bf16 != 0 : BF > 0) {
      const bf16x4 af = {bf16_bits(av[0]), bf16_bits(av[1]), bf16_bits(av[2]), bf16_bits(av[3])};
      const bf16x4 bfv = {bf16_bits(bv[0]), bf16_bits(bv[1]), bf16_bits(bv[2]), bf16_bits(bv[3])};
      acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(af, bfv, acc, 0, 0, 0);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
  }
  return acc;
}
// INLOOP: the branch on `bf16` inside the k loop (one copy of the loop: the 4-wave round
// kernel, whose fp32 rounds measured 1.1–1.5 % slower with two: profiles/round8/nn_refactor.md)
template <bool AK, bool BK, bool INLOOP = false>
__device__ __forceinline__ f32x4 gemm16p(const float* a, int ars, int acs, const float* b,
                                         int brs, int bcs, int K, int bf16) {
  if constexpr (INLOOP) return gemm16t<AK, BK, -1>(a, ars, acs, b, brs, bcs, K, bf16);
  return bf16 ? gemm16t<AK, BK, 1>(a, ars, acs, b, brs, bcs, K)
              : gemm16t<AK, BK, 0>(a, ars, acs, b, brs, bcs, K);
}

// Activation and its derivative expressed through the activation's OUTPUT h (what the
// forward pass keeps in LDS): relu' = [h > 0], tanh' = 1 − h², σ' = h(1 − h).
__device__ __forceinline__ float act_fwd(float v, int act) {
  switch (act) {
    case kTanh: return tanhf(v);
    case kSigmoid: return 1.f / (1.f + __expf(-v));
    case kIdentity: return v;
    default: return fmaxf(v, 0.f);
  }
}

__device__ __forceinline__ float act_grad(float h, int act) {
  switch (act) {
    case kTanh: return 1.f - h * h;
    case kSigmoid: return h * (1.f - h);
    case kIdentity: return 1.f;
    default: return h > 0.f ? 1.f : 0.f;
  }
}

__device__ void load_model(const float* __restrict__ w, float* sm, const MlpDesc& g) {
  for (int l = 0; l < g.L; ++l) {
    const int rows = g.np[l + 1], ld = g.ldw[l], nin = g.n[l], nout = g.n[l + 1];
    float* W = sm + g.lw[l];
    for (int i = threadIdx.x; i < rows * ld; i += blockDim.x) {
      const int o = i / ld, c = i - o * ld;
      W[i] = (o < nout && c < nin) ? w[g.woff[l] + o * nin + c] : 0.f;
    }
    for (int o = threadIdx.x; o < rows; o += blockDim.x)
      sm[g.lb[l] + o] = o < nout ? w[g.boff[l] + o] : 0.f;
  }
}

// Forward of one 32-row tile already staged in H_0; H_L holds the logits.
template <bool INLOOP>
__device__ void forward(float* sm, const MlpDesc& g) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ci = lane & 15, cg = lane >> 4;  // accumulator column / row group
  for (int l = 0; l < g.L; ++l) {
    const float* H = sm + g.lh[l];
    float* Ho = sm + g.lh[l + 1];
    const float* W = sm + g.lw[l];
    const float* bs = sm + g.lb[l];
    const int ntc = g.np[l + 1] / kT, nt = (kMB / kT) * ntc, ldo = g.ldh[l + 1];
    const bool hidden = l + 1 < g.L;
    for (int t = wave; t < nt; t += 4) {
      const int rt = t / ntc, ct = t - rt * ntc;
      const f32x4 acc = gemm16p<true, true, INLOOP>(H + rt * kT * g.ldh[l], g.ldh[l], 1,
                                            W + ct * kT * g.ldw[l], 1, g.ldw[l], g.np[l], g.bf16);
      const int col = ct * kT + ci;
      const float bias = bs[col];
      const bool pad = col >= g.n[l + 1];  // padding columns stay exactly zero
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = acc[q] + bias;
        if (hidden) v = pad ? 0.f : act_fwd(v, g.act);
        Ho[(rt * kT + 4 * cg + q) * ldo + col] = v;
      }
    }
    __syncthreads();
  }
}

__device__ void stage_rows(const float* __restrict__ x, long long r0, long long r1, float* sm,
                           const MlpDesc& g) {
  const int np0 = g.np[0], n0 = g.n[0], ld = g.ldh[0];
  float* H = sm + g.lh[0];
  for (int i = threadIdx.x; i < kMB * np0; i += blockDim.x) {
    const int r = i / np0, c = i - r * np0;
    const long long row = r0 + r;
    H[r * ld + c] = (row < r1 && c < n0) ? x[row * n0 + c] : 0.f;
  }
}

// Mini-batch staging of the fused round kernels (NT threads): H_0 and the labels of the
// step at m0, with the NEXT mini-batch's loads in flight while the current one trains
// (np0 ≤ 64: kSlots slots of the 32 × np0 tile per thread, fixed (row, col) per slot, held
// in registers); wider inputs stage synchronously. Rows past r1 read as zero, their labels
// as NaN. The caller's barrier follows.
template <int NT>
struct RowStager {
  static constexpr int kSlots = (kMB * 64 + NT - 1) / NT;
  bool pf;
  int n0;
  int soff[kSlots], srow[kSlots], scol[kSlots];
  float xr[kSlots], yr;

  __device__ __forceinline__ void init(const MlpDesc& g) {
    const int tid = threadIdx.x, np0 = g.np[0], ld0 = g.ldh[0];
    n0 = g.n[0];
    pf = np0 <= 64;
    yr = 0.f;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const int i = tid + NT * j;
      const bool in = pf && i < kMB * np0;
      srow[j] = in ? i / np0 : -1;
      scol[j] = in ? i - srow[j] * np0 : 0;
      soff[j] = in ? srow[j] * ld0 + scol[j] : 0;
    }
  }
  // unconditional loads from clamped rows
  __device__ __forceinline__ void fetch(const float* __restrict__ x, const float* __restrict__ yv,
                                        long long m, long long r1) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const long long row = min(m + (srow[j] < 0 ? 0 : srow[j]), r1 - 1);
      xr[j] = x[row * n0 + (scol[j] < n0 ? scol[j] : 0)];
    }
    yr = yv[min(m + (tid < kMB ? tid : 0), r1 - 1)];
  }
  __device__ __forceinline__ void stage(const float* __restrict__ x, const float* __restrict__ yv,
                                        long long m0, long long r1, float* sm, const MlpDesc& g) {
    const int tid = threadIdx.x;
    if (pf) {
      float* H = sm + g.lh[0];
#pragma unroll
      for (int j = 0; j < kSlots; ++j)
        if (srow[j] >= 0) H[soff[j]] = (m0 + srow[j] < r1 && scol[j] < n0) ? xr[j] : 0.f;
      if (tid < kMB) sm[g.ly + tid] = m0 + tid < r1 ? yr : __builtin_nanf("");
      if (m0 + kMB < r1) fetch(x, yv, m0 + kMB, r1);
    } else {
      stage_rows(x, m0, r1, sm, g);
      if (tid < kMB) {
        const long long row = m0 + tid;
        sm[g.ly + tid] = row < r1 ? yv[row] : __builtin_nanf("");
      }
    }
  }
};

// Round end of the fused kernels: Δ = W_spoke − W_0. With a workspace: the spoke's own row,
// plain coalesced stores (mlp_colsum_kernel sums the rows); without: atomics into the
// accumulator (every spoke hits the same nparams addresses — the slow fallback).
template <int NT>
__device__ __forceinline__ void store_delta(const float* __restrict__ w, const float* sm,
                                            const MlpDesc& g, float* __restrict__ dacc,
                                            float* __restrict__ ws, int nparams) {
  const int tid = threadIdx.x;
  float* wrow = ws ? ws + (size_t)blockIdx.x * nparams : nullptr;
  for (int l = 0; l < g.L; ++l) {
    const int nin = g.n[l], nout = g.n[l + 1], ld = g.ldw[l];
    const float* W = sm + g.lw[l];
    for (int i = tid; i < nout * nin; i += NT) {
      const int o = i / nin, c = i - o * nin;
      const float d = W[o * ld + c] - w[g.woff[l] + i];
      if (wrow) wrow[g.woff[l] + i] = d;
      else if (d != 0.f) atomicAdd(&dacc[g.woff[l] + i], d);
    }
    for (int o = tid; o < nout; o += NT) {
      const float d = sm[g.lb[l] + o] - w[g.boff[l] + o];
      if (wrow) wrow[g.boff[l] + o] = d;
      else if (d != 0.f) atomicAdd(&dacc[g.boff[l] + o], d);
    }
  }
}

// Diagnostics only (csrc/tests/mlp_stamp_probe.hip builds with OMLDM_MLP_STAMPS): per
// spoke, clock64 sums of the mini-batch phases (staging+barrier, forward, loss, backward).
// The sums stay in registers until the round's end (a global read-modify-write per stamp
// would put a memory round trip into every phase it measures).
#ifdef OMLDM_MLP_STAMPS
__device__ unsigned long long* g_mlp_stamps;
#define MLP_STAMP(k)                                                                  \
  do {                                                                                \
    const unsigned long long now_ = clock64();                                        \
    if ((k) > 0) mlp_acc_[(k) & 7] += now_ - mlp_t_;                                    \
    mlp_t_ = now_;                                                                    \
  } while (0)
#define MLP_STAMP_FLUSH()                                                             \
  do {                                                                                \
    if (tid == 0)                                                                     \
      for (int k_ = 1; k_ < 8; ++k_) g_mlp_stamps[(size_t)blockIdx.x * 8 + k_] += mlp_acc_[k_]; \
  } while (0)
#else
#define MLP_STAMP_FLUSH() \
  do {                    \
  } while (0)
#define MLP_STAMP(k) \
  do {               \
  } while (0)
#endif

__global__ __launch_bounds__(256) void mlp_round_kernel(const float* __restrict__ w,
                                                        const float* __restrict__ x,
                                                        const float* __restrict__ yv, long long B,
                                                        int R, float lr, float* __restrict__ dacc,
                                                        float* __restrict__ stats,
                                                        float* __restrict__ nact, MlpDesc g,
                                                        float* __restrict__ ws, int nparams) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ci = lane & 15, cg = lane >> 4;  // accumulator column / row group
  const long long r0 = (long long)blockIdx.x * R;
  const long long r1 = min(B, r0 + R);
  if (r0 >= B) return;
  load_model(w, sm, g);
  float loss = 0.f, corr = 0.f, nv = 0.f;
  const int L = g.L, npL = g.np[L];
  RowStager<256> rows;
  rows.init(g);
  if (rows.pf) rows.fetch(x, yv, r0, r1);
#ifdef OMLDM_MLP_STAMPS
  unsigned long long mlp_t_ = clock64();
  unsigned long long mlp_acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  for (long long m0 = r0; m0 < r1; m0 += kMB) {
    MLP_STAMP(0);
    rows.stage(x, yv, m0, r1, sm, g);
    __syncthreads();
    MLP_STAMP(1);
    forward<true>(sm, g);
    MLP_STAMP(2);
    // ---- loss gradient dZ_L (one thread per row)
    bool valid = false;
    if (tid < kMB) {
      const float y = sm[g.ly + tid];
      valid = !__builtin_isnan(y);
      const float* o = sm + g.lh[L] + tid * g.ldh[L];
      float* G = sm + g.lg0 + tid * g.ldg;
      for (int k = 0; k < npL; ++k) G[k] = 0.f;
      if (valid) {
        if (g.task == 0) {  // regression, squared error (sum)
          const float e = o[0] - y;
          G[0] = 2.f * e;
          loss += e * e;
        } else if (g.task == 1) {  // binary logistic on ±1 / {0,1} labels
          const float t = y > 0.f ? 1.f : 0.f, z = o[0];
          G[0] = 1.f / (1.f + __expf(-z)) - t;
          loss += fmaxf(z, 0.f) - z * t + log1pf(__expf(-fabsf(z)));
          corr += ((z >= 0.f) == (t > 0.f)) ? 1.f : 0.f;
        } else {  // multiclass softmax cross-entropy
          int yi = (int)y;
          yi = yi < 0 ? 0 : (yi >= g.K ? g.K - 1 : yi);
          float m = o[0];
          int am = 0;
          for (int k = 1; k < g.K; ++k)
            if (o[k] > m) {
              m = o[k];
              am = k;
            }
          float se = 0.f;
          for (int k = 0; k < g.K; ++k) se += __expf(o[k] - m);
          const float inv = 1.f / se;
          for (int k = 0; k < g.K; ++k) G[k] = __expf(o[k] - m) * inv - (k == yi ? 1.f : 0.f);
          loss += -(o[yi] - m - __logf(se));
          corr += am == yi ? 1.f : 0.f;
        }
        nv += 1.f;
      }
    }
    const int cnt = __syncthreads_count(valid ? 1 : 0);
    MLP_STAMP(3);
    if (cnt == 0) continue;
    const float eta = lr / (float)cnt;
    int gcur = g.lg0, gnext = g.lg1;
    for (int l = L - 1; l >= 0; --l) {
      const float* Gc = sm + gcur;
      float* W = sm + g.lw[l];
      const float* H = sm + g.lh[l];
      const int ldw = g.ldw[l], ldh = g.ldh[l], nin = g.np[l], nout = g.np[l + 1];
      if (l > 0) {  // dH_l = (dZ · W_l) ⊙ act'(H_l)
        float* Gn = sm + gnext;
        const int ntc = nin / kT;
        for (int t = wave; t < (kMB / kT) * ntc; t += 4) {
          const int rt = t / ntc, ct = t - rt * ntc;
          const f32x4 acc = gemm16p<true, false, true>(Gc + rt * kT * g.ldg, g.ldg, 1, W + ct * kT, ldw,
                                                 1, nout, g.bf16);
          const int col = ct * kT + ci;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int row = rt * kT + 4 * cg + q;
            Gn[row * g.ldg + col] = acc[q] * act_grad(H[row * ldh + col], g.act);
          }
        }
      }
      __syncthreads();  // W_l fully read before it is updated
      MLP_STAMP(5);
      const int ntc = nin / kT, nto = nout / kT;
      for (int t = wave; t < nto * ntc; t += 4) {
        const int to = t / ntc, tc = t - to * ntc;
        const f32x4 acc =
            gemm16p<false, false, true>(Gc + to * kT, 1, g.ldg, H + tc * kT, ldh, 1, kMB, g.bf16);
        const int c = tc * kT + ci;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int o = to * kT + 4 * cg + q;
          W[o * ldw + c] -= eta * acc[q];
        }
      }
      MLP_STAMP(6);
      for (int o = tid; o < nout; o += blockDim.x) {
        float s = 0.f;
        for (int i = 0; i < kMB; ++i) s += Gc[i * g.ldg + o];
        sm[g.lb[l] + o] -= eta * s;
      }
      __syncthreads();
      MLP_STAMP(7);
      const int tmp = gcur;
      gcur = gnext;
      gnext = tmp;
    }
    MLP_STAMP(4);
  }
  MLP_STAMP_FLUSH();
  store_delta<256>(w, sm, g, dacc, ws, nparams);
  if (wave == 0) {
    loss = wave_sum(loss);
    corr = wave_sum(corr);
    nv = wave_sum(nv);
    if (lane == 0 && nv > 0.f) {
      atomicAdd(&stats[0], loss);
      atomicAdd(&stats[1], nv);
      atomicAdd(&stats[2], corr);
      atomicAdd(&stats[3], 1.f);
      if (nact) atomicAdd(nact, 1.f);  // the apply kernel's divisor (its own buffer)
    }
  }
}

// ------------------------------------------------------------------ round kernel v2
// The same mini-batch SGD, restructured for step latency (one 32-row step of a
// [13, 64, 64, 1] spoke is a chain of ~10 small GEMMs on one CU; the v1 kernel spent
// ~15 µs per step there, mostly in barriers, zero-padded work and serial loops):
// * widths padded to 16, not 32 (13 → 16 inputs, 1 → 16 outputs: half the MFMAs of the
//   first and last layers; row strides stay ≡ 4 floats mod 64 banks);
// * the loss is the last layer's epilogue: a row's ≤ 16 logits sit in one 16-lane DPP
//   row of the accumulator, so softmax max / sum / argmax are row_ror reductions and the
//   output gradient goes straight to LDS (no loss phase, no barrier);
// * bias gradients are column sums taken in the epilogue that produces each gradient
//   (LDS float atomics), not a 32-row serial loop per layer;
// * backward phase l computes dH_l (reads W_l) together with the update of W_{l+1} (whose
//   dH was the previous phase) from three rotating gradient buffers, and the last phase
//   updates W_1 and W_0 together: one barrier per layer instead of two;
// * the valid-row count of a step comes from a ballot over the staged labels in every
//   wave (no block-wide count);
// * operand loads of the next 16-wide k step are issued before the current MFMAs.
// Same arithmetic as v1 (fp32 MFMA, same mini-batch order); sums may associate
// differently.

// 16-lane DPP row reductions (every lane of the row gets the result)
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x124>(v));
  return fmaxf(v, dpp_mov<0x128>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x124>(v);
  return v + dpp_mov<0x128>(v);
}
__device__ __forceinline__ float row16_min(float v) {
  v = fminf(v, dpp_mov<0xB1>(v));
  v = fminf(v, dpp_mov<0x4E>(v));
  v = fminf(v, dpp_mov<0x124>(v));
  return fminf(v, dpp_mov<0x128>(v));
}

constexpr int kRound2Waves = 16;

__global__ __launch_bounds__(kRound2Waves * 64) void mlp_round2_kernel(
    const float* __restrict__ w, const float* __restrict__ x, const float* __restrict__ yv,
    long long B, int R, float lr, float* __restrict__ dacc, float* __restrict__ stats,
    float* __restrict__ nact, MlpDesc g, float* __restrict__ ws, int nparams) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NW = kRound2Waves, NT = NW * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ci = lane & 15, cg = lane >> 4;  // accumulator column / row group
  const long long r0 = (long long)blockIdx.x * R;
  const long long r1 = min(B, r0 + R);
  if (r0 >= B) return;
  load_model(w, sm, g);
  const int L = g.L;
  for (int l = 0; l < L; ++l)
    for (int o = tid; o < g.np[l + 1]; o += NT) sm[g.lbg[l] + o] = 0.f;
  if (tid < 4) sm[g.lsc + tid] = 0.f;
  float loss = 0.f, corr = 0.f, nv = 0.f;
  auto gb = [&](int j) { return sm + g.lgb[j % 3]; };
  RowStager<NT> rows;
  rows.init(g);
  if (rows.pf) rows.fetch(x, yv, r0, r1);
  __syncthreads();
#ifdef OMLDM_MLP_STAMPS
  unsigned long long mlp_t_ = clock64();
  unsigned long long mlp_acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  for (long long m0 = r0; m0 < r1; m0 += kMB) {
    MLP_STAMP(0);
    rows.stage(x, yv, m0, r1, sm, g);
    __syncthreads();
    // valid rows of the step: every wave counts them itself
    const float yl = sm[g.ly + (lane & 31)];
    const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < 32 && yl == yl));
    if (cnt == 0) {
      __syncthreads();
      continue;
    }
    const float eta = lr / (float)cnt;
    MLP_STAMP(1);
    // ---- hidden layers: H_{l+1} = act(H_l · W_lᵀ + b_l)
    for (int l = 0; l + 1 < L; ++l) {
      const float* H = sm + g.lh[l];
      float* Ho = sm + g.lh[l + 1];
      const float* W = sm + g.lw[l];
      const float* bs = sm + g.lb[l];
      const int ntc = g.np[l + 1] / 16, nt = 2 * ntc, ldo = g.ldh[l + 1];
      for (int t = wave; t < nt; t += NW) {
        const int rt = t / ntc, ct = t - rt * ntc;
        const f32x4 acc = gemm16p<true, true>(H + rt * 16 * g.ldh[l], g.ldh[l], 1,
                                              W + ct * 16 * g.ldw[l], 1, g.ldw[l], g.np[l], g.bf16);
        const int col = ct * 16 + ci;
        const float bias = bs[col];
        const bool pad = col >= g.n[l + 1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float v = acc[q] + bias;
          Ho[(rt * 16 + 4 * cg + q) * ldo + col] = pad ? 0.f : act_fwd(v, g.act);
        }
      }
      __syncthreads();
    }
    MLP_STAMP(2);
    // ---- output layer + loss (np_L = 16: one column tile, a row's logits in one DPP row)
    {
      const int l = L - 1;
      float* GL = gb(L);
      for (int rt = wave; rt < 2; rt += NW) {
        const f32x4 acc = gemm16p<true, true>(sm + g.lh[l] + rt * 16 * g.ldh[l], g.ldh[l], 1,
                                              sm + g.lw[l], 1, g.ldw[l], g.np[l], g.bf16);
        const float bias = sm[g.lb[l] + ci];
        float csum = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = rt * 16 + 4 * cg + q;
          const float o = acc[q] + bias;
          const float y = sm[g.ly + row];
          const bool valid = y == y;
          float gr = 0.f;
          if (g.task == 2) {
            const bool live = ci < g.K;
            int yi = valid ? (int)y : 0;
            yi = yi < 0 ? 0 : (yi >= g.K ? g.K - 1 : yi);
            const float m = row16_max(live ? o : -INFINITY);
            const float e = live ? __expf(o - m) : 0.f;
            const float se = row16_sum(e);
            const float am = row16_min(live && o == m ? (float)ci : 64.f);
            gr = valid && live ? e / se - (ci == yi ? 1.f : 0.f) : 0.f;
            if (valid && ci == yi) {
              loss += -(o - m - __logf(se));
              corr += (int)am == yi ? 1.f : 0.f;
            }
          } else if (ci == 0 && valid) {
            if (g.task == 0) {
              const float e = o - y;
              gr = 2.f * e;
              loss += e * e;
            } else {
              const float tt = y > 0.f ? 1.f : 0.f;
              gr = 1.f / (1.f + __expf(-o)) - tt;
              loss += fmaxf(o, 0.f) - o * tt + __logf(1.f + __expf(-fabsf(o)));  // statistic
              corr += ((o >= 0.f) == (tt > 0.f)) ? 1.f : 0.f;
            }
          }
          if (ci == 0 && valid) nv += 1.f;
          GL[row * g.ldg + ci] = gr;
          csum += gr;
        }
        atomicAdd(&sm[g.lbg[l] + ci], csum);
      }
      __syncthreads();
    }
    MLP_STAMP(3);
    // ---- backward: phase l = dH_l (l ≥ 1) + update of W_{l+1} (l + 1 ≤ L − 1), and the
    // last phase (l = 0) updates W_1 and W_0
    for (int l = L - 1; l >= 0; --l) {
      const int na = l >= 1 ? 2 * (g.np[l] / 16) : 0;
      const int ub = l + 1 <= L - 1 ? l + 1 : -1;  // W_{l+1}
      const int nb = ub >= 0 ? (g.np[ub + 1] / 16) * (g.np[ub] / 16) : 0;
      const int nc = l == 0 ? (g.np[1] / 16) * (g.np[0] / 16) : 0;
      for (int t = wave; t < na + nb + nc; t += NW) {
        if (t < na) {  // dH_l = (G_{l+1} · W_l) ⊙ act'(H_l)
          const float* Gc = gb(l + 1);
          float* Gn = gb(l);
          const float* W = sm + g.lw[l];
          const float* H = sm + g.lh[l];
          const int ntc = g.np[l] / 16, rt = t / ntc, ct = t - rt * ntc;
          const f32x4 acc = gemm16p<true, false>(Gc + rt * 16 * g.ldg, g.ldg, 1, W + ct * 16,
                                                 g.ldw[l], 1, g.np[l + 1], g.bf16);
          const int col = ct * 16 + ci;
          float csum = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int row = rt * 16 + 4 * cg + q;
            const float v = acc[q] * act_grad(H[row * g.ldh[l] + col], g.act);
            Gn[row * g.ldg + col] = v;
            csum += v;
          }
          atomicAdd(&sm[g.lbg[l - 1] + col], csum);
        } else {  // W_u −= η · G_{u+1}ᵀ · H_u
          const int u = t < na + nb ? ub : 0;
          const int tt = t < na + nb ? t - na : t - na - nb;
          const float* Gc = gb(u + 1);
          float* W = sm + g.lw[u];
          const float* H = sm + g.lh[u];
          const int ntc = g.np[u] / 16, to = tt / ntc, tc = tt - to * ntc;
          const f32x4 acc = gemm16p<false, false>(Gc + to * 16, 1, g.ldg, H + tc * 16, g.ldh[u], 1,
                                                  kMB, g.bf16);
          const int c = tc * 16 + ci;
#pragma unroll
          for (int q = 0; q < 4; ++q) W[(to * 16 + 4 * cg + q) * g.ldw[u] + c] -= eta * acc[q];
        }
      }
      auto bias_step = [&](int u) {
        for (int o = tid; o < g.np[u + 1]; o += NT) {
          sm[g.lb[u] + o] -= eta * sm[g.lbg[u] + o];
          sm[g.lbg[u] + o] = 0.f;
        }
      };
      if (ub >= 0) bias_step(ub);
      if (l == 0) bias_step(0);
      __syncthreads();
      MLP_STAMP(4 + (l < 3 ? l : 3));  // 4: phase 0 (W_1, W_0), 5: phase 1, 6: phase 2
    }
  }
  MLP_STAMP_FLUSH();
  store_delta<NT>(w, sm, g, dacc, ws, nparams);
  loss = wave_sum(loss);
  corr = wave_sum(corr);
  nv = wave_sum(nv);
  if (lane == 0 && nv > 0.f) {
    atomicAdd(&sm[g.lsc + 0], loss);
    atomicAdd(&sm[g.lsc + 1], nv);
    atomicAdd(&sm[g.lsc + 2], corr);
  }
  __syncthreads();
  if (tid == 0 && sm[g.lsc + 1] > 0.f) {
    atomicAdd(&stats[0], sm[g.lsc + 0]);
    atomicAdd(&stats[1], sm[g.lsc + 1]);
    atomicAdd(&stats[2], sm[g.lsc + 2]);
    atomicAdd(&stats[3], 1.f);
    if (nact) atomicAdd(nact, 1.f);
  }
}

// Inference: every block stages the model once and walks 32-row tiles (grid-stride).
__global__ __launch_bounds__(256) void mlp_forward_kernel(const float* __restrict__ w,
                                                          const float* __restrict__ x,
                                                          long long B, float* __restrict__ out,
                                                          MlpDesc g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  load_model(w, sm, g);
  const int L = g.L;
  for (long long m0 = (long long)blockIdx.x * kMB; m0 < B; m0 += (long long)gridDim.x * kMB) {
    __syncthreads();  // previous tile's H_L consumed
    stage_rows(x, m0, B, sm, g);
    __syncthreads();
    forward<false>(sm, g);
    const float* o = sm + g.lh[L];
    for (int i = threadIdx.x; i < kMB * g.K; i += blockDim.x) {
      const int r = i / g.K, k = i - r * g.K;
      if (m0 + r < B) out[(m0 + r) * g.K + k] = o[r * g.ldh[L] + k];
    }
  }
}

static int make_desc(int L, const int* widths, int task, int act, MlpDesc* g, int pad = 32) {
  if (L < 1 || L > kMaxLayers || (act & 0xff) > kIdentity || (act & ~0x1ff)) return -1;
  *g = MlpDesc{};
  g->L = L;
  g->task = task;
  g->act = act & 0xff;        // low byte: hidden activation
  g->bf16 = (act >> 8) & 1;   // bit 8: bf16 GEMM operands
  g->K = widths[L];
  int off = 0;
  for (int l = 0; l <= L; ++l) {
    if (widths[l] < 1) return -1;
    g->n[l] = widths[l];
    g->np[l] = (widths[l] + pad - 1) / pad * pad;
  }
  for (int l = 0; l < L; ++l) {  // flat parameter layout: W_l [n_{l+1} × n_l], b_l
    g->woff[l] = off;
    off += g->n[l + 1] * g->n[l];
    g->boff[l] = off;
    off += g->n[l + 1];
  }
  // row strides ≡ 4 floats mod 64 banks (np is a multiple of 32): a 16-lane group reading
  // 16 bytes each from 16 rows covers all 64 banks once, and a lane reading one float per
  // row (the strided operands) sees rows 4 banks apart; region starts 16-byte aligned
  int p = 0, maxnp = 0;
  auto al4 = [](int v) { return (v + 3) & ~3; };
  for (int l = 0; l < L; ++l) {
    g->ldw[l] = g->np[l] + 4;
    g->lw[l] = p;
    p = al4(p + g->np[l + 1] * g->ldw[l]);
    g->lb[l] = p;
    p = al4(p + g->np[l + 1]);
  }
  for (int l = 0; l <= L; ++l) {
    g->ldh[l] = g->np[l] + 4;
    g->lh[l] = p;
    p = al4(p + kMB * g->ldh[l]);
    if (g->np[l] > maxnp) maxnp = g->np[l];
  }
  g->ldg = maxnp + 4;
  g->lg0 = p;
  p += kMB * g->ldg;
  g->lg1 = p;
  p += kMB * g->ldg;
  g->ly = p;
  p += kMB;
  if (pad == 16) {  // v2 layout: three gradient buffers (lg0, lg1 + one more), bias grads
    g->lgb[0] = g->lg0;
    g->lgb[1] = g->lg1;
    g->lgb[2] = p;
    p += kMB * g->ldg;
    for (int l = 0; l < L; ++l) {
      g->lbg[l] = p;
      p = al4(p + g->np[l + 1]);
    }
    g->lsc = p;
    p += 4;
  }
  g->total = p;
  return 0;
}

// dacc[c] += Σ_{s in this block's 64-spoke slab} ws[s][c]: one atomic per (column, slab)
// instead of one per (column, spoke).
constexpr int kMlpSlab = 64;
__global__ __launch_bounds__(256) void mlp_colsum_kernel(const float* __restrict__ ws, int S,
                                                         int n, float* __restrict__ dacc) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int s0 = blockIdx.y * kMlpSlab, s1 = min(S, s0 + kMlpSlab);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int s = s0;
  for (; s + 3 < s1; s += 4) {
    a0 += ws[(size_t)s * n + c];
    a1 += ws[(size_t)(s + 1) * n + c];
    a2 += ws[(size_t)(s + 2) * n + c];
    a3 += ws[(size_t)(s + 3) * n + c];
  }
  for (; s < s1; ++s) a0 += ws[(size_t)s * n + c];
  const float t = (a0 + a1) + (a2 + a3);
  if (t != 0.f) atomicAdd(&dacc[c], t);
}

// ------------------------------------------------------------------ streamed-weight form
// Layer stacks whose weights do not fit one CU's LDS (128-wide hidden layers and up). The
// same 32-row mini-batch SGD, one workgroup (16 waves) per spoke, but the spoke's working
// model is its row of the S × nparams scratch `ws` in HBM (L2-resident in practice): copied
// from w at round start, trained in place, turned into W_spoke − w at round end, where
// mlp_colsum_kernel folds the rows into dacc as for the fused forms. LDS holds only the
// mini-batch: H_0..H_L, the layer-output gradients G_1..G_L, the biases and y.
// * forward and dH: each wave owns 16×16 output tiles; the activation / gradient operand
//   comes from LDS, the weight operand straight from the slab (forward: a weight row is
//   k-contiguous, 16 bytes per lane and k step; dH: the tile's 16 columns are contiguous
//   across lanes). The slab is the flat, unpadded parameter layout, so loads are masked to
//   the real rows and columns (padding reads as zero) and carry 4-byte alignment only;
// * update W_l −= η·G_{l+1}ᵀ·H_l: both operands from LDS, the read-modify-write of the slab
//   straight from the MFMA accumulators (one owner lane per weight);
// * biases and their gradients (column sums of G) stay in LDS.
// Why workgroup scope suffices: a slab row is written and read by ONE workgroup, hence on
// ONE CU, through that CU's vector L1 (write-through: a store updates the line there and
// goes on to L2). Every slab hand-off between waves is store → __syncthreads() → load; the
// barrier's workgroup-scope release/acquire waits for the stores (vmcnt(0)) before any
// wave passes it, and no other CU's L1 ever holds or needs these lines inside the launch.
// Nothing crosses workgroups before the kernel boundary (w is read-only here; the colsum
// pass is a later launch), so there are no flags, spins or agent-scope fences.
struct MlpStreamDesc {
  int L, task, K, act, bf16;
  int n[kMaxLayers + 1], np[kMaxLayers + 1];  // widths, and padded to 16
  int woff[kMaxLayers], boff[kMaxLayers];     // flat parameter layout (= slab layout)
  int lh[kMaxLayers + 1], ldh[kMaxLayers + 1];  // LDS: H_l, row stride (also G_l's)
  int lg[kMaxLayers + 1];                       // LDS: G_l, l = 1..L
  int lb[kMaxLayers];                           // LDS: b_l, np[l+1] floats
  int ly, fwd_total, total;                     // floats: forward kernel / round kernel
};

struct __attribute__((packed, aligned(4))) SlabVec4 {
  float v[4];
};

// row[k..k+3] of an n-float slab row; zero past n or when the row itself is padding
__device__ __forceinline__ void slab_ld4(const float* row, int k, int n, bool ok, float (&o)[4]) {
  if (ok && k + 3 < n) {
    const SlabVec4 t = *reinterpret_cast<const SlabVec4*>(row + k);
    o[0] = t.v[0]; o[1] = t.v[1]; o[2] = t.v[2]; o[3] = t.v[3];
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = (ok && k + u < n) ? row[k + u] : 0.f;
  }
}

template <bool BF16>
__device__ __forceinline__ f32x4 mfma16_step(const float (&av)[4], const float (&bv)[4], f32x4 acc) {
  if constexpr (BF16) {
    const bf16x4 af = {bf16_bits(av[0]), bf16_bits(av[1]), bf16_bits(av[2]), bf16_bits(av[3])};
    const bf16x4 bfv = {bf16_bits(bv[0]), bf16_bits(bv[1]), bf16_bits(bv[2]), bf16_bits(bv[3])};
    acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(af, bfv, acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
  }
  return acc;
}

// Both 16-row tiles of the mini-batch against one 16-column weight tile, so a weight
// fragment is loaded once: c0 / c1 = A[0..15 / 16..31]·Wtᵀ with A(i, k) = a[i·lda + k] in
// LDS and Wt = 16 slab rows of n_in floats, of which the first `rows` exist. K = padded
// n_in. Operand map and accumulator layout of gemm16t. The k steps whose 16 columns all
// exist load unconditionally (a padding row re-reads row 0 and is zeroed by a select) and
// are unrolled, so several steps' loads are in flight; the last, partial step is masked.
template <bool BF16>
__device__ __forceinline__ void stream_gemm_fwd(const float* a, int lda, const float* wt, int n_in,
                                                int rows, int K, f32x4& c0, f32x4& c1) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  c0 = f32x4{0.f, 0.f, 0.f, 0.f};
  c1 = c0;
  const float* ap0 = a + r * lda + 4 * g;
  const float* ap1 = ap0 + 16 * lda;
  const bool ok = r < rows;
  const float* brow = wt + (size_t)(ok ? r : 0) * n_in;
  const int Kf = n_in & ~15;
  auto step = [&](int k, const float (&bv)[4]) {
    float a0[4], a1[4];
    const float4 t0 = *reinterpret_cast<const float4*>(ap0 + k);
    const float4 t1 = *reinterpret_cast<const float4*>(ap1 + k);
    a0[0] = t0.x; a0[1] = t0.y; a0[2] = t0.z; a0[3] = t0.w;
    a1[0] = t1.x; a1[1] = t1.y; a1[2] = t1.z; a1[3] = t1.w;
    c0 = mfma16_step<BF16>(a0, bv, c0);
    c1 = mfma16_step<BF16>(a1, bv, c1);
  };
  int k = 0;
  for (; k + 64 <= Kf; k += 64) {  // four k steps' loads issued ahead of their MFMAs
    SlabVec4 t[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = *reinterpret_cast<const SlabVec4*>(brow + k + 16 * s + 4 * g);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float bv[4] = {ok ? t[s].v[0] : 0.f, ok ? t[s].v[1] : 0.f, ok ? t[s].v[2] : 0.f,
                           ok ? t[s].v[3] : 0.f};
      step(k + 16 * s, bv);
    }
  }
  for (; k < Kf; k += 16) {
    const SlabVec4 t = *reinterpret_cast<const SlabVec4*>(brow + k + 4 * g);
    const float bv[4] = {ok ? t.v[0] : 0.f, ok ? t.v[1] : 0.f, ok ? t.v[2] : 0.f, ok ? t.v[3] : 0.f};
    step(k, bv);
  }
  if (Kf < K) {
    float bv[4];
    slab_ld4(brow, Kf + 4 * g, n_in, ok, bv);
    step(Kf, bv);
  }
}

// c0 / c1 = A[0..15 / 16..31]·W[:, cb..cb+15]: A(i, k) = a[i·lda + k] in LDS (k over the
// layer's outputs), W the layer's n_out × n_in slab block. K = padded n_out. The tile's 16
// columns are contiguous across lanes; a padding column re-reads column 0 and is zeroed.
template <bool BF16>
__device__ __forceinline__ void stream_gemm_bwd(const float* a, int lda, const float* W, int n_in,
                                                int n_out, int cb, int K, f32x4& c0, f32x4& c1) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  c0 = f32x4{0.f, 0.f, 0.f, 0.f};
  c1 = c0;
  const float* ap0 = a + r * lda + 4 * g;
  const float* ap1 = ap0 + 16 * lda;
  const int j = cb + r;
  const bool ok = j < n_in;
  const float* bp = W + (size_t)(4 * g) * n_in + (ok ? j : 0);
  const int Kf = n_out & ~15;
  auto step = [&](int k, const float (&bv)[4]) {
    float a0[4], a1[4];
    const float4 t0 = *reinterpret_cast<const float4*>(ap0 + k);
    const float4 t1 = *reinterpret_cast<const float4*>(ap1 + k);
    a0[0] = t0.x; a0[1] = t0.y; a0[2] = t0.z; a0[3] = t0.w;
    a1[0] = t1.x; a1[1] = t1.y; a1[2] = t1.z; a1[3] = t1.w;
    c0 = mfma16_step<BF16>(a0, bv, c0);
    c1 = mfma16_step<BF16>(a1, bv, c1);
  };
  int k = 0;
  for (; k + 32 <= Kf; k += 32) {  // two k steps' loads issued ahead of their MFMAs
    float t[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int u = 0; u < 4; ++u) t[s][u] = bp[(size_t)(k + 16 * s + u) * n_in];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float bv[4] = {ok ? t[s][0] : 0.f, ok ? t[s][1] : 0.f, ok ? t[s][2] : 0.f,
                           ok ? t[s][3] : 0.f};
      step(k + 16 * s, bv);
    }
  }
  for (; k < Kf; k += 16) {
    float bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = bp[(size_t)(k + u) * n_in];
      bv[u] = ok ? t : 0.f;
    }
    step(k, bv);
  }
  if (Kf < K) {
    float bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = Kf + 4 * g + u;
      bv[u] = (ok && kk < n_out) ? W[(size_t)kk * n_in + j] : 0.f;
    }
    step(Kf, bv);
  }
}

// One layer of a staged 32-row tile: Ho = act(H·Wᵀ + b) (no activation on the output
// layer); padding columns of Ho stay exactly zero. `bias` holds n_out floats. A wave takes
// a 16-column tile of the layer's outputs for all 32 rows.
template <bool BF16>
__device__ __forceinline__ void stream_layer_fwd(const float* H, int ldh, float* Ho, int ldo,
                                                 const float* W, const float* bias, int n_in,
                                                 int np_in, int n_out, int np_out, bool hidden,
                                                 int act) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int ci = lane & 15, cg = lane >> 4;
  for (int ct = wave; ct < np_out / 16; ct += nw) {
    f32x4 c0, c1;
    stream_gemm_fwd<BF16>(H, ldh, W + (size_t)ct * 16 * n_in, n_in, n_out - ct * 16, np_in, c0, c1);
    const int col = ct * 16 + ci;
    const bool pad = col >= n_out;
    const float b = pad ? 0.f : bias[col];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v0 = c0[q] + b, v1 = c1[q] + b;
      if (hidden) {
        v0 = act_fwd(v0, act);
        v1 = act_fwd(v1, act);
      }
      Ho[(4 * cg + q) * ldo + col] = pad ? 0.f : v0;
      Ho[(16 + 4 * cg + q) * ldo + col] = pad ? 0.f : v1;
    }
  }
}

__device__ __forceinline__ void stream_stage(const float* __restrict__ x, long long r0, long long r1,
                                             float* H, int n0, int np0, int ld) {
  for (int i = threadIdx.x; i < kMB * np0; i += blockDim.x) {
    const int r = i / np0, c = i - r * np0;
    const long long row = r0 + r;
    H[r * ld + c] = (row < r1 && c < n0) ? x[row * n0 + c] : 0.f;
  }
}

constexpr int kStreamWaves = 16;

// The barrier behind slab stores: every storing wave first waits until its stores have
// left for L2 through this CU's L1 (vmcnt(0)), so the loads of any wave past the barrier
// find them; __syncthreads() orders the LDS side.
__device__ __forceinline__ void slab_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ __launch_bounds__(kStreamWaves * 64) void mlp_round_stream_kernel(
    const float* __restrict__ w, const float* __restrict__ x, const float* __restrict__ yv,
    long long B, int R, float lr, float* __restrict__ stats, float* __restrict__ nact,
    MlpStreamDesc g, float* ws, int nparams) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NT = kStreamWaves * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ci = lane & 15, cg = lane >> 4;
  float* slab = ws + (size_t)blockIdx.x * nparams;
  const long long r0 = (long long)blockIdx.x * R;
  const long long r1 = min(B, r0 + R);
  if (r0 >= B) {  // a spoke without rows: a zero delta for the column sums
    for (int i = tid; i < nparams; i += NT) slab[i] = 0.f;
    return;
  }
  const int L = g.L, npL = g.np[L];
  for (int i = tid; i < nparams; i += NT) slab[i] = w[i];
  for (int l = 0; l < L; ++l)
    for (int o = tid; o < g.np[l + 1]; o += NT)
      sm[g.lb[l] + o] = o < g.n[l + 1] ? w[g.boff[l] + o] : 0.f;
  slab_barrier();
  float loss = 0.f, corr = 0.f, nv = 0.f;
  for (long long m0 = r0; m0 < r1; m0 += kMB) {
    stream_stage(x, m0, r1, sm + g.lh[0], g.n[0], g.np[0], g.ldh[0]);
    if (tid < kMB) {
      const long long row = m0 + tid;
      sm[g.ly + tid] = row < r1 ? yv[row] : __builtin_nanf("");
    }
    __syncthreads();
    const float yl = sm[g.ly + (lane & 31)];
    const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < 32 && yl == yl));
    if (cnt == 0) {
      __syncthreads();  // every wave has read y before the next step restages it
      continue;
    }
    const float eta = lr / (float)cnt;
    // ---- forward
    for (int l = 0; l < L; ++l) {
      const float* W = slab + g.woff[l];
      if (g.bf16)
        stream_layer_fwd<true>(sm + g.lh[l], g.ldh[l], sm + g.lh[l + 1], g.ldh[l + 1], W,
                               sm + g.lb[l], g.n[l], g.np[l], g.n[l + 1], g.np[l + 1], l + 1 < L,
                               g.act);
      else
        stream_layer_fwd<false>(sm + g.lh[l], g.ldh[l], sm + g.lh[l + 1], g.ldh[l + 1], W,
                                sm + g.lb[l], g.n[l], g.np[l], g.n[l + 1], g.np[l + 1], l + 1 < L,
                                g.act);
      __syncthreads();
    }
    // ---- loss gradient G_L: one thread per row, a serial pass over the row's logits in
    // LDS (any output width; the rules of mlp_round_kernel)
    if (tid < kMB) {
      const float y = sm[g.ly + tid];
      const float* o = sm + g.lh[L] + tid * g.ldh[L];
      float* G = sm + g.lg[L] + tid * g.ldh[L];
      for (int k = 0; k < npL; ++k) G[k] = 0.f;
      if (y == y) {
        if (g.task == 0) {
          const float e = o[0] - y;
          G[0] = 2.f * e;
          loss += e * e;
        } else if (g.task == 1) {
          const float t = y > 0.f ? 1.f : 0.f, z = o[0];
          G[0] = 1.f / (1.f + __expf(-z)) - t;
          loss += fmaxf(z, 0.f) - z * t + log1pf(__expf(-fabsf(z)));
          corr += ((z >= 0.f) == (t > 0.f)) ? 1.f : 0.f;
        } else {
          int yi = (int)y;
          yi = yi < 0 ? 0 : (yi >= g.K ? g.K - 1 : yi);
          float m = o[0];
          int am = 0;
          for (int k = 1; k < g.K; ++k)
            if (o[k] > m) {
              m = o[k];
              am = k;
            }
          float se = 0.f;
          for (int k = 0; k < g.K; ++k) se += __expf(o[k] - m);
          const float inv = 1.f / se;
          for (int k = 0; k < g.K; ++k) G[k] = __expf(o[k] - m) * inv - (k == yi ? 1.f : 0.f);
          loss += -(o[yi] - m - __logf(se));
          corr += am == yi ? 1.f : 0.f;
        }
        nv += 1.f;
      }
    }
    __syncthreads();
    // ---- backward, per layer: dH_l from the slab's W_l, barrier, then W_l and b_l updated
    for (int l = L - 1; l >= 0; --l) {
      const float* Gc = sm + g.lg[l + 1];
      const int ldg = g.ldh[l + 1];
      const float* H = sm + g.lh[l];
      const int ldh = g.ldh[l], n_in = g.n[l], n_out = g.n[l + 1];
      float* W = slab + g.woff[l];
      if (l > 0) {  // G_l = (G_{l+1} · W_l) ⊙ act'(H_l)
        float* Gn = sm + g.lg[l];
        for (int ct = wave; ct < g.np[l] / 16; ct += kStreamWaves) {
          f32x4 c0, c1;
          if (g.bf16)
            stream_gemm_bwd<true>(Gc, ldg, W, n_in, n_out, ct * 16, g.np[l + 1], c0, c1);
          else
            stream_gemm_bwd<false>(Gc, ldg, W, n_in, n_out, ct * 16, g.np[l + 1], c0, c1);
          const int col = ct * 16 + ci;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int row = 4 * cg + q;
            Gn[row * ldh + col] = c0[q] * act_grad(H[row * ldh + col], g.act);
            Gn[(row + 16) * ldh + col] = c1[q] * act_grad(H[(row + 16) * ldh + col], g.act);
          }
        }
        __syncthreads();  // W_l fully read before it is updated
      }
      // the tile's old weights are requested first and arrive while the product is formed
      const int ntc = g.np[l] / 16, nto = g.np[l + 1] / 16;
      for (int t = wave; t < nto * ntc; t += kStreamWaves) {
        const int to = t / ntc, tc = t - to * ntc;
        const int c = tc * 16 + ci, o0 = to * 16 + 4 * cg;
        float* Wp = W + (size_t)o0 * n_in + c;
        float old[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) old[q] = (c < n_in && o0 + q < n_out) ? Wp[(size_t)q * n_in] : 0.f;
        const f32x4 acc = gemm16p<false, false>(Gc + to * 16, 1, ldg, H + tc * 16, ldh, 1, kMB, g.bf16);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c < n_in && o0 + q < n_out) Wp[(size_t)q * n_in] = old[q] - eta * acc[q];
      }
      for (int o = tid; o < n_out; o += NT) {
        float s = 0.f;
        for (int i = 0; i < kMB; ++i) s += Gc[i * ldg + o];
        sm[g.lb[l] + o] -= eta * s;
      }
      slab_barrier();
    }
  }
  // ---- round end: the slab row becomes Δ = W_spoke − W_0 (every step ended in a barrier)
  for (int l = 0; l < L; ++l) {
    const int nw = g.n[l + 1] * g.n[l];
    for (int i = tid; i < nw; i += NT) slab[g.woff[l] + i] -= w[g.woff[l] + i];
    for (int o = tid; o < g.n[l + 1]; o += NT)
      slab[g.boff[l] + o] = sm[g.lb[l] + o] - w[g.boff[l] + o];
  }
  if (wave == 0) {
    loss = wave_sum(loss);
    corr = wave_sum(corr);
    nv = wave_sum(nv);
    if (lane == 0 && nv > 0.f) {
      atomicAdd(&stats[0], loss);
      atomicAdd(&stats[1], nv);
      atomicAdd(&stats[2], corr);
      atomicAdd(&stats[3], 1.f);
      if (nact) atomicAdd(nact, 1.f);
    }
  }
}

// Inference at the same widths: 32-row tiles grid-stride, activations in LDS, weights and
// biases read from w itself (read-only, shared by every workgroup).
constexpr int kStreamFwdWaves = 8;
__global__ __launch_bounds__(kStreamFwdWaves * 64) void mlp_forward_stream_kernel(
    const float* __restrict__ w, const float* __restrict__ x, long long B,
    float* __restrict__ out, MlpStreamDesc g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L;
  for (long long m0 = (long long)blockIdx.x * kMB; m0 < B; m0 += (long long)gridDim.x * kMB) {
    __syncthreads();  // previous tile's H_L consumed
    stream_stage(x, m0, B, sm + g.lh[0], g.n[0], g.np[0], g.ldh[0]);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      if (g.bf16)
        stream_layer_fwd<true>(sm + g.lh[l], g.ldh[l], sm + g.lh[l + 1], g.ldh[l + 1],
                               w + g.woff[l], w + g.boff[l], g.n[l], g.np[l], g.n[l + 1],
                               g.np[l + 1], l + 1 < L, g.act);
      else
        stream_layer_fwd<false>(sm + g.lh[l], g.ldh[l], sm + g.lh[l + 1], g.ldh[l + 1],
                                w + g.woff[l], w + g.boff[l], g.n[l], g.np[l], g.n[l + 1],
                                g.np[l + 1], l + 1 < L, g.act);
      __syncthreads();
    }
    const float* o = sm + g.lh[L];
    for (int i = threadIdx.x; i < kMB * g.K; i += blockDim.x) {
      const int r = i / g.K, k = i - r * g.K;
      if (m0 + r < B) out[(m0 + r) * g.K + k] = o[r * g.ldh[L] + k];
    }
  }
}

// LDS layout of the streamed form. Gradient buffers: one per layer output (G_1..G_L), or
// two max-width buffers that layers of equal parity share (only G_{l+1} and G_l are live
// together) — whichever is smaller, so the form admits the union of both sets
// ([13, 512, 1] needs the first, deep equal-width stacks gain from the second).
static int make_stream_desc(int L, const int* widths, int task, int act, MlpStreamDesc* g) {
  if (L < 1 || L > kMaxLayers || (act & 0xff) > kIdentity || (act & ~0x1ff)) return -1;
  *g = MlpStreamDesc{};
  g->L = L;
  g->task = task;
  g->act = act & 0xff;
  g->bf16 = (act >> 8) & 1;
  g->K = widths[L];
  long long off = 0;
  for (int l = 0; l <= L; ++l) {
    if (widths[l] < 1 || widths[l] > (1 << 15)) return -1;
    g->n[l] = widths[l];
    g->np[l] = (widths[l] + 15) / 16 * 16;
  }
  for (int l = 0; l < L; ++l) {
    g->woff[l] = (int)off;
    off += (long long)g->n[l + 1] * g->n[l];
    g->boff[l] = (int)off;
    off += g->n[l + 1];
    if (off > (1ll << 30)) return -1;
  }
  long long p = 0, per = 0;
  int maxld = 0;
  for (int l = 0; l <= L; ++l) {
    g->ldh[l] = g->np[l] + 4;
    g->lh[l] = (int)p;
    p += kMB * g->ldh[l];
    if (l >= 1) {
      per += kMB * g->ldh[l];
      if (g->ldh[l] > maxld) maxld = g->ldh[l];
    }
  }
  g->fwd_total = (int)p;
  for (int l = 0; l < L; ++l) {
    g->lb[l] = (int)p;
    p += g->np[l + 1];
  }
  const long long rot = 2ll * kMB * maxld;
  if (per <= rot) {
    for (int l = 1; l <= L; ++l) {
      g->lg[l] = (int)p;
      p += kMB * g->ldh[l];
    }
  } else {
    for (int l = 1; l <= L; ++l) g->lg[l] = (int)(p + (l & 1) * kMB * maxld);
    p += rot;
  }
  g->ly = (int)p;
  p += kMB;
  if (p > (1ll << 28)) return -1;
  g->total = (int)p;
  return 0;
}

}  // namespace omldm

using namespace omldm;

// Round kernel form: 0 fused-32 (v1) wherever a fused kernel runs, 3 (the default) fused-16
// (v2) where it applies, 4 the streamed-weight form at every shape it takes, also where a
// fused form fits (tests and benchmarks; it applies to omldm_mlp_forward too). Whatever the
// form, a stack no fused kernel holds goes to the streamed form. `set` ∈ {0, 3, 4} sets it,
// any other value only reads it; the default comes from OMLDM_MLP_FORM (3, also for any
// other value there). (1 and 2 were 4- and 8-wave fused-16 kernels: docs/KERNELS.md.)
static bool mlp_form_known(int form) { return form == 0 || form == 3 || form == 4; }

OMLDM_API int omldm_mlp_form(int set) {
  static int form = [] {
    const char* e = getenv("OMLDM_MLP_FORM");
    const int f = e ? atoi(e) : 3;
    return mlp_form_known(f) ? f : 3;
  }();
  if (mlp_form_known(set)) form = set;
  return form;
}

// LDS bytes the fused kernels need for this layer stack (host-side feasibility check).
OMLDM_API long long omldm_mlp_lds_bytes(int L, const int* widths) {
  MlpDesc g;
  if (make_desc(L, widths, 0, 0, &g)) return -1;
  return (long long)g.total * 4;
}

// LDS bytes of the streamed-weight form (mini-batch activations and gradients only).
OMLDM_API long long omldm_mlp_stream_lds_bytes(int L, const int* widths) {
  MlpStreamDesc g;
  if (make_stream_desc(L, widths, 0, 0, &g)) return -1;
  return (long long)g.total * 4;
}

// LDS bytes of the fused-16 layout; -1 where fused-16 does not apply (output width > 16).
OMLDM_API long long omldm_mlp_fused16_lds_bytes(int L, const int* widths) {
  MlpDesc g;
  if (make_desc(L, widths, 0, 0, &g, 16) || widths[L] > 16) return -1;
  return (long long)g.total * 4;
}

constexpr size_t kMlpLdsMax = 160 * 1024;  // LDS of one CU: every form's limit

enum { kMlpFused32 = 0, kMlpFused16 = 1, kMlpStream = 2 };  // kernel ids of a plan

// The routing of omldm_mlp_round and omldm_mlp_forward (host code only; both launchers
// consume it and decide nothing themselves): which kernels take the layer stack under `form`
// (< 0: the form in use). out = {round kernel, its waves, its LDS bytes, forward kernel, its
// LDS bytes}. 0: out is filled; −1: not a layer stack (layer count, a width < 1 or past the
// streamed form's index range); −2: no form holds it.
// * round: fused-16 for output widths ≤ 16 whose 16-padded layout fits (not under form 0),
//   else fused-32 if the 32-padded layout fits — which also takes the output-≤-16 stacks
//   that fit padded to 32 but not with fused-16's third gradient buffer and bias gradients
//   — else streamed; form 4 streams everything;
// * forward: the fused kernel whenever the 32-padded layout fits, whatever trains the stack;
//   else (and under form 4) streamed, refused past the ROUND's activation limit so that one
//   limit holds for training and scoring.
OMLDM_API int omldm_mlp_plan(int L, const int* widths, int form, int* out) {
  for (int i = 0; i < 5; ++i) out[i] = 0;
  if (!mlp_form_known(form)) form = omldm_mlp_form(-1);
  MlpDesc g32, g16;
  MlpStreamDesc gs;
  if (make_desc(L, widths, 0, 0, &g32)) return -1;
  const size_t lds32 = (size_t)g32.total * 4;
  const bool fits32 = lds32 <= kMlpLdsMax;
  const bool fits16 = form == 3 && widths[L] <= 16 && make_desc(L, widths, 0, 0, &g16, 16) == 0 &&
                      (size_t)g16.total * 4 <= kMlpLdsMax;
  const int round = form == 4 ? kMlpStream : fits16 ? kMlpFused16 : fits32 ? kMlpFused32 : kMlpStream;
  const int fwd = form == 4 || !fits32 ? kMlpStream : kMlpFused32;
  if (round == kMlpStream || fwd == kMlpStream) {
    if (make_stream_desc(L, widths, 0, 0, &gs)) return -1;
    if ((size_t)gs.total * 4 > kMlpLdsMax) return -2;
  }
  out[0] = round;
  out[1] = round == kMlpFused32 ? 4 : round == kMlpFused16 ? kRound2Waves : kStreamWaves;
  out[2] = round == kMlpFused32 ? (int)lds32 : round == kMlpFused16 ? g16.total * 4 : gs.total * 4;
  out[3] = fwd;
  out[4] = fwd == kMlpFused32 ? (int)lds32 : gs.fwd_total * 4;
  return 0;
}

static bool mlp_act_known(int act) { return (act & 0xff) <= kIdentity && !(act & ~0x1ff); }

static int launch_round_stream(const float* w, const float* x, const float* y, long long B, int R,
                               int S, int L, const int* widths, int task, int act, float lr,
                               size_t lds, float* dacc, float* stats, float* nact, float* ws,
                               hipStream_t stream) {
  MlpStreamDesc g;
  if (make_stream_desc(L, widths, task, act, &g)) return -1;
  if (!ws) return -4;  // the working models live in the scratch rows
  const int e = check_dyn_lds((const void*)mlp_round_stream_kernel, lds);
  if (e) return e;
  const int nparams = g.boff[L - 1] + g.n[L];
  hipLaunchKernelGGL(mlp_round_stream_kernel, dim3(S), dim3(kStreamWaves * 64), lds, stream, w, x,
                     y, B, R, lr, stats, nact, g, ws, nparams);
  hipLaunchKernelGGL(mlp_colsum_kernel, dim3((nparams + 255) / 256, (S + kMlpSlab - 1) / kMlpSlab),
                     dim3(256), 0, stream, ws, S, nparams, dacc);
  return (int)hipGetLastError();
}

// One protocol round: S spokes × R rows (spoke s owns rows [sR, sR+R)); task 0 regression,
// 1 binary logistic, 2 softmax. dacc[nparams] += Σ_s Δ_s; stats[0..3] += loss, n, correct,
// active spokes (spokes with ≥ 1 labelled row); nact (optional, zeroed beforehand) += active
// spokes too. Follow with omldm_multiclass_apply(w, dacc, nparams, ..., nact, ...): the
// apply kernel clears stats, so its divisor must live in a separate buffer.
// ws: optional S × nparams scratch (spoke deltas by plain stores + slab column sums); the
// streamed-weight form (stacks past the fused kernels' LDS) requires it: -4 without.
OMLDM_API int omldm_mlp_round(const float* w, const float* x, const float* y, long long B, int R,
                              int S, int L, const int* widths, int task, int act, float lr,
                              float* dacc, float* stats, float* nact, float* ws, void* stream) {
  if (B <= 0 || S <= 0) return 0;
  if (R <= 0 || (long long)R * S < B) return -3;
  int plan[5];
  if (!mlp_act_known(act)) return -1;
  if (const int rc = omldm_mlp_plan(L, widths, -1, plan)) return rc;
  const size_t lds = (size_t)plan[2];
  const dim3 block(plan[1] * 64);
  MlpDesc g;
  int e;
  switch (plan[0]) {
    case kMlpStream:
      return launch_round_stream(w, x, y, B, R, S, L, widths, task, act, lr, lds, dacc, stats, nact,
                                 ws, (hipStream_t)stream);
    case kMlpFused16:
      if (make_desc(L, widths, task, act, &g, 16)) return -1;
      if ((e = check_dyn_lds((const void*)mlp_round2_kernel, lds))) return e;
      hipLaunchKernelGGL(mlp_round2_kernel, dim3(S), block, lds, (hipStream_t)stream, w, x, y, B, R,
                         lr, dacc, stats, nact, g, ws, g.boff[L - 1] + g.n[L]);
      break;
    default:  // kMlpFused32
      if (make_desc(L, widths, task, act, &g)) return -1;
      if ((e = check_dyn_lds((const void*)mlp_round_kernel, lds))) return e;
      hipLaunchKernelGGL(mlp_round_kernel, dim3(S), block, lds, (hipStream_t)stream, w, x, y, B, R,
                         lr, dacc, stats, nact, g, ws, g.boff[L - 1] + g.n[L]);
  }
  const int nparams = g.boff[L - 1] + g.n[L];
  if (ws)
    hipLaunchKernelGGL(mlp_colsum_kernel, dim3((nparams + 255) / 256, (S + kMlpSlab - 1) / kMlpSlab),
                       dim3(256), 0, (hipStream_t)stream, ws, S, nparams, dacc);
  return (int)hipGetLastError();
}

OMLDM_API int omldm_mlp_forward(const float* w, const float* x, long long B, int L,
                                const int* widths, int act, float* out, void* stream) {
  if (B <= 0) return 0;
  int plan[5];
  if (!mlp_act_known(act)) return -1;
  if (const int rc = omldm_mlp_plan(L, widths, -1, plan)) return rc;
  const size_t lds = (size_t)plan[4];
  const long long tiles = (B + kMB - 1) / kMB;
  const int blocks = (int)(tiles < 1024 ? tiles : 1024);
  int e;
  switch (plan[3]) {
    case kMlpStream: {
      MlpStreamDesc sg;
      if (make_stream_desc(L, widths, 0, act, &sg)) return -1;
      if ((e = check_dyn_lds((const void*)mlp_forward_stream_kernel, lds))) return e;
      hipLaunchKernelGGL(mlp_forward_stream_kernel, dim3(blocks), dim3(kStreamFwdWaves * 64), lds,
                         (hipStream_t)stream, w, x, B, out, sg);
      break;
    }
    default: {  // kMlpFused32
      MlpDesc g;
      if (make_desc(L, widths, 0, act, &g)) return -1;
      if ((e = check_dyn_lds((const void*)mlp_forward_kernel, lds))) return e;
      hipLaunchKernelGGL(mlp_forward_kernel, dim3(blocks), dim3(256), lds, (hipStream_t)stream, w,
                         x, B, out, g);
    }
  }
  return (int)hipGetLastError();
}
