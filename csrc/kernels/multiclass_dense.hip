// Exact dense sequential MultiClassPA round for numerical-only streams (no categorical
// columns): one Synchronous round of S virtual spokes with the semantics of
// omldm_cpu_multiclass_round (csrc/host/linear_cpu.cpp) at dc = 0.
//
// The model a spoke touches is K × D dense floats (D = dn + bias), so a spoke is one
// workgroup that keeps the round-start prototypes w0[K][D] and its private delta d[K][D]
// in LDS, apart: the oracle sums x·(W + d), a merged copy would round differently, and d
// has to come out exactly. No hash table, no spill, no prep pass.
//
//  * Two waves. Wave 1 is the loader: it stages the next chunk of rows in LDS (bias column
//    1, padding 0) and computes, with lane i owning row i, everything that does not depend
//    on the model: the label, ‖x‖² in the oracle's column order, τ's denominator 2‖x‖²
//    (PA-II: + 0.5/C) and τ's cap. An unlabelled row gets cap 0, so its τ is 0 without a
//    branch. Wave 0 runs the rows of the current chunk; one barrier per chunk.
//  * K ≤ 64: Kpad = 4 … 64 classes, G = 64 / Kpad lanes per class, lane (k, g) owning the
//    columns g, g + G, … of class k. Slot i of lane ℓ is word i·65 + ℓ of w0 and of d, so
//    a slot of all lanes is one conflict-free row of LDS, and so are the slots of one lane.
//    K > 64: ⌈K/64⌉ classes per lane, the model as [k][D | 1].
//  * Per row the chain is: the lane's fmas of x·(w0 + d), one butterfly over the G lanes of
//    a class (DPP inside a 16-lane row, one fixed order), one wave arg-max over the classes
//    other than y (the lowest class among equals), the wave-uniform step math in the
//    oracle's operation order (contraction off) and the update d[y] += τx, d[r] −= τx —
//    skipped when τ = 0, as in the oracle. Below 8 slots per lane the lanes that own the two
//    classes update their slots; from 8 on, and at K > 64, all lanes share the two classes'
//    D columns (one wave: its LDS accesses run in order, wave_lds_sync holds the compiler
//    to it). The only numerical difference from the oracle is the summation order (and the
//    fma) of a score.
//  * The row's margin is parked in lane i; loss and mistakes are computed from the parked
//    margins once per chunk and summed over the wave at the end of the round.
//  * Round end: every spoke stores one workspace row (its K·D deltas, its statistics) and a
//    second small kernel folds the rows in spoke order into dacc[k][0..dn), dacc[k][dim−1]
//    and stats — no float atomics, no workgroup waits for another: a round is
//    bit-reproducible. Padded classes and columns never reach the workspace.
#include "spoke_table.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

constexpr int kMcdMaxD = 256;      // columns (dn + bias)
constexpr int kMcdMaxK = 256;      // classes
constexpr int kMcdMaxKD = 16384;   // K·D: 128 KiB for w0 + d
constexpr int kMcdLds = 160 * 1024;
constexpr int kMcdStat = 8;        // workspace row: K·D deltas, then loss, rows, mistakes, 1
constexpr int kMcdSS = 65;         // words between a lane's slots (K ≤ 64): odd, so one lane's
                                   // slots fall in different banks as well as one slot's lanes
constexpr int kMcdCoop = 8;        // slots per lane from which all lanes share a class's update

struct McdGeom {
  int G;    // lanes per class (K ≤ 64), 0: several classes per lane
  int CW;   // slots per lane (G > 0) or classes per lane (G = 0)
  int NM;   // floats of w0, and of d
  int XS;   // floats of a staged row
  int CR;   // rows per chunk
  int Dp;   // row stride of the [k][Dp] model (G = 0)
};

inline bool mcd_fits(int dn, int bias, int K) {
  const int D = dn + (bias ? 1 : 0);
  return dn >= 0 && D >= 1 && D <= kMcdMaxD && K >= 2 && K <= kMcdMaxK &&
         (long long)K * D <= kMcdMaxKD;
}

inline size_t mcd_lds_bytes(const McdGeom& g) {
  return ((size_t)2 * g.NM + (size_t)2 * g.CR * g.XS + 6 * 64) * sizeof(float);
}

inline McdGeom mcd_geom(int D, int K) {
  McdGeom g{};
  if (K <= 64) {
    const int kp = K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64;
    g.G = 64 / kp;
    g.CW = (D + g.G - 1) / g.G;
    g.NM = kMcdSS * g.CW;
    g.XS = g.G * g.CW;
  } else {
    g.CW = (K + 63) / 64;
    g.Dp = D | 1;  // odd: the lanes' rows fall in different banks
    g.NM = K * g.Dp;
    g.XS = D;
  }
  for (g.CR = 64; g.CR > 8; g.CR >>= 1)
    if (mcd_lds_bytes(g) <= (size_t)kMcdLds) break;
  return g;
}

template <bool NBF>
__device__ __forceinline__ float mcd_num(const void* __restrict__ num, size_t i) {
  if (NBF)
    return __uint_as_float((unsigned)static_cast<const unsigned short*>(num)[i] << 16);
  return static_cast<const float*>(num)[i];
}

// Sum over the G adjacent lanes of a class, the same bits in each of them.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  if (G >= 2) v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  if (G >= 4) v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  if (G >= 8) v += dpp_mov<0x141>(v);   // row_half_mirror: the other quad of the 8
  if (G >= 16) v += dpp_mov<0x140>(v);  // row_mirror: the other half of the row
  return v;
}

// Orders one wave's LDS accesses: what its lanes stored before is what any of its lanes loads
// after (the hardware runs a wave's LDS instructions in order; this keeps the compiler from
// moving or reusing loads across it).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// d[st·i] ±= τ·x[xst·i] for i < n (d += τx on the label's class, d −= τx on the rival's), the
// product rounded before the sum like the oracle's. The loads of four steps go ahead of
// their stores, so a step does not wait for an LDS round trip of its own.
__device__ __forceinline__ void mcd_update(float* d, int st, const float* x, int xst, int n,
                                           float tau, bool up) {
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    float xv[4], dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xv[u] = x[xst * (i + u)];
      dv[u] = d[st * (i + u)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = tau * xv[u];
      d[st * (i + u)] = dv[u] + (up ? t : -t);
    }
  }
  for (; i < n; ++i) {
    const float t = tau * x[xst * i];
    d[st * i] += up ? t : -t;
  }
}

// U steps of a lane's score, p += x[G·(i+u)]·(w[65·(i+u)] + d[65·(i+u)]) in the order of u:
// every load goes ahead of the first fma, one LDS round trip for the U steps.
template <int U, int G>
__device__ __forceinline__ float mcd_dot(const float* x, const float* w, const float* d, int i,
                                         float p) {
  float xv[U], wv[U], dv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    xv[u] = x[G * (i + u)];
    wv[u] = w[kMcdSS * (i + u)];
    dv[u] = d[kMcdSS * (i + u)];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) p = __builtin_fmaf(xv[u], wv[u] + dv[u], p);
  return p;
}

template <int G, bool NBF>
__global__ __launch_bounds__(128) void mcd_round_kernel(
    const float* __restrict__ W, const void* __restrict__ num, int dn,
    const void* __restrict__ y, int y_i8, int B, int R, int dim, int K, int variant, float C,
    int bias, float* __restrict__ ws, McdGeom geo) {
  extern __shared__ __attribute__((aligned(16))) float mcd_smem[];
  const int NM = geo.NM, XS = geo.XS, CR = geo.CR, CW = geo.CW, Dp = geo.Dp;
  float* w0 = mcd_smem;
  float* dl = w0 + NM;
  float* xs = dl + NM;                   // [2][CR][XS]
  float* denL = xs + (size_t)2 * CR * XS;  // [2][64]
  float* capL = denL + 128;              // [2][64]
  int* ycL = reinterpret_cast<int*>(capL + 128);  // [2][64]: class, −1 out of range, −2 skipped
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long a = (long long)s * R;
  if (a >= B) return;  // an idle spoke is no worker of the round (the grid has none)
  const long long b = a + R < (long long)B ? a + R : (long long)B;
  const int nrows = (int)(b - a);
  const int D = dn + (bias ? 1 : 0);
  const float inf = __builtin_inff();

  // the round-start prototypes and a zero delta; the constant columns of both staging buffers
  for (int idx = tid; idx < NM; idx += 128) {
    int k, j;
    if constexpr (G > 0) {
      const int ln = idx % kMcdSS;  // word 64 of a slot row is padding (k = Kpad ≥ K)
      k = ln / G;
      j = ln % G + G * (idx / kMcdSS);
    } else {
      k = idx / Dp;
      j = idx - k * Dp;
    }
    float v = 0.f;
    if (k < K && j < D) v = W[(size_t)k * dim + (j < dn ? j : dim - 1)];
    w0[idx] = v;
    dl[idx] = 0.f;
  }
  for (int idx = tid; idx < 2 * CR * XS; idx += 128)
    xs[idx] = (bias && idx % XS == dn) ? 1.f : 0.f;
  __syncthreads();

  const int nchunks = (nrows + CR - 1) / CR;

  // wave 1: chunk ch into its staging buffer, and what its rows' steps need besides the model
  auto produce = [&](int ch) {
    const int buf = ch & 1;
    const long long t0 = a + (long long)ch * CR;
    const int nr = b - t0 < CR ? (int)(b - t0) : CR;
    const bool in = lane < nr;
    const long long t = in ? t0 + lane : b - 1;
    const float yv = load_label(y, (int)t, y_i8);
    const bool skip = !in || yv != yv;
    const size_t base = (size_t)t * dn;
    float pn = 0.f;
#pragma unroll 8
    for (int j = 0; j < dn; ++j) {
      const float xv = mcd_num<NBF>(num, base + j);
      pn += xv * xv;
    }
    if (bias) pn += 1.f;
    float cap = 0.f, den = 1.f;
    if (!skip && pn > 0.f) {
      den = 2.f * pn;
      if (variant == 2) den = den + 0.5f / C;
      cap = variant == 1 ? C : inf;
    }
    int yc = -2;
    if (!skip) yc = (yv > -1.f && yv < (float)K) ? (int)yv : -1;
    denL[buf * 64 + lane] = den;
    capL[buf * 64 + lane] = cap;
    ycL[buf * 64 + lane] = yc;
    // the chunk's nr·dn values are contiguous: element e = row·dn + col, 64 per step
    if (dn > 0) {
      float* xb = xs + (size_t)buf * CR * XS;
      const size_t e0 = (size_t)t0 * dn;
      const int ne = nr * dn, q64 = 64 / dn, r64 = 64 % dn;
      int row = lane / dn, col = lane % dn;
      for (int e = lane; e < ne; e += 256) {
        float v[4];
        int at[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int eu = e + 64 * u;
          v[u] = mcd_num<NBF>(num, e0 + (eu < ne ? eu : ne - 1));
          at[u] = eu < ne ? row * XS + col : -1;
          row += q64;
          col += r64;
          if (col >= dn) {
            col -= dn;
            ++row;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (at[u] >= 0) xb[at[u]] = v[u];
      }
    }
  };

  float loss_l = 0.f, nex_l = 0.f, mist_l = 0.f;  // per-lane sums (wave 0)

  // wave 0: the rows of chunk ch, in order
  auto consume = [&](int ch) {
    const int buf = ch & 1;
    const int nr = nrows - ch * CR < CR ? nrows - ch * CR : CR;
    const float* xb = xs + (size_t)buf * CR * XS;
    float mpark = 0.f;  // lane i: the margin of row i
    // lane i holds what row i's step needs; the row loop fetches it with one readlane each
    const int ycv = ycL[buf * 64 + lane];
    const float denv = denL[buf * 64 + lane], capv = capL[buf * 64 + lane];
    if constexpr (G > 0) {
      const int k = lane / G, g = lane % G;
      for (int r = 0; r < nr; ++r) {
        const float* xr = xb + r * XS + g;
        const int yc = __builtin_amdgcn_readlane(ycv, r);
        const float den = readlane_f(denv, r), cap = readlane_f(capv, r);
        float p = 0.f;
        int i = 0;
        for (; i + 8 <= CW; i += 8) p = mcd_dot<8, G>(xr, w0 + lane, dl + lane, i, p);
        if (i + 4 <= CW) {
          p = mcd_dot<4, G>(xr, w0 + lane, dl + lane, i, p);
          i += 4;
        }
        if (i + 2 <= CW) {
          p = mcd_dot<2, G>(xr, w0 + lane, dl + lane, i, p);
          i += 2;
        }
        if (i < CW) p = mcd_dot<1, G>(xr, w0 + lane, dl + lane, i, p);
        p = group_sum<G>(p);
        const float cand = (k < K && k != yc) ? p : -inf;
        const float m = wave_max(cand);
        const unsigned long long at = __builtin_amdgcn_ballot_w64(cand == m);
        const int rr = (at ? __builtin_ctzll(at) : 0) / G;
        const float sy = yc >= 0 ? readlane_f(p, yc * G) : 0.f;
        const float margin = sy - m;
        const float loss = fmaxf(0.f, 1.f - margin);
        float tau = fminf(cap, loss / den);
        if (!(m > -inf)) tau = 0.f;  // no rival
        mpark = lane == r ? margin : mpark;
        if (tau != 0.f) {  // wave-uniform
          if (CW >= kMcdCoop) {
            // all lanes on the two classes' D columns: column j is slot j / G of lane k·G + j % G
            for (int j = lane; j < D; j += 64) {
              const float u = tau * xb[r * XS + j];
              const int at = (j / G) * kMcdSS + j % G;
              if (yc >= 0) dl[at + yc * G] += u;
              dl[at + rr * G] -= u;
            }
            wave_lds_sync();  // the next row's lanes read what other lanes wrote
          } else if (k == yc || k == rr) {
            mcd_update(dl + lane, kMcdSS, xr, G, CW, tau, k == yc);
          }
        }
      }
    } else {
      int kc[4], kb[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kc[c] = lane + 64 * c;
        kb[c] = (kc[c] < K ? kc[c] : K - 1) * Dp;  // a class past K reads class K − 1
      }
      for (int r = 0; r < nr; ++r) {
        const float* xr = xb + r * XS;
        const int yc = __builtin_amdgcn_readlane(ycv, r);
        const float den = readlane_f(denv, r), cap = readlane_f(capv, r);
        float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < D; ++j) {
          const float xv = xr[j];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < CW) sc[c] = __builtin_fmaf(xv, w0[kb[c] + j] + dl[kb[c] + j], sc[c]);
        }
        float bv = -inf;
        int bk = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < CW && kc[c] < K && kc[c] != yc && sc[c] > bv) {
            bv = sc[c];
            bk = kc[c];
          }
        const float m = wave_max(bv);
        const bool any = m > -inf;
        // the lowest class among the lanes that hold the maximum
        const float low = -wave_max(bv == m ? -(float)bk : -inf);
        const int rr = any ? (int)low : -1;
        float syv = sc[0];
#pragma unroll
        for (int c = 1; c < 4; ++c)
          if ((yc >> 6) == c) syv = sc[c];
        const float sy = yc >= 0 ? readlane_f(syv, yc & 63) : 0.f;
        const float margin = sy - m;
        const float loss = fmaxf(0.f, 1.f - margin);
        float tau = fminf(cap, loss / den);
        if (!any) tau = 0.f;
        mpark = lane == r ? margin : mpark;
        if (tau != 0.f) {  // wave-uniform
          for (int j = lane; j < D; j += 64) {  // all lanes on the two classes' rows
            const float u = tau * xr[j];
            if (yc >= 0) dl[yc * Dp + j] += u;
            dl[rr * Dp + j] -= u;
          }
          wave_lds_sync();  // the next row's lanes read what other lanes wrote
        }
      }
    }
    // the chunk's statistics from the parked margins, lane i for row i
    if (lane < nr && ycv != -2) {
      nex_l += 1.f;
      loss_l += fmaxf(0.f, 1.f - mpark);
      mist_l += mpark <= 0.f ? 1.f : 0.f;
    }
  };

  if (wave == 1) produce(0);
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    if (wave == 1) {
      if (ch + 1 < nchunks) produce(ch + 1);
    } else {
      consume(ch);
    }
    __syncthreads();
  }
  if (wave != 0) return;

  const float loss_sum = wave_sum(loss_l), nex = wave_sum(nex_l), mist = wave_sum(mist_l);
  float* wrow = ws + (size_t)s * ((size_t)K * D + kMcdStat);
  if constexpr (G > 0) {
    const int k = lane / G, g = lane % G;
    for (int i = 0; i < CW; ++i) {
      const int j = g + G * i;
      if (k < K && j < D) wrow[(size_t)k * D + j] = dl[i * kMcdSS + lane];
    }
  } else {
    for (int c = 0; c < CW; ++c) {
      const int k = lane + 64 * c;
      if (k < K)
        for (int j = 0; j < D; ++j) wrow[(size_t)k * D + j] = dl[k * Dp + j];
    }
  }
  if (lane == 0) {
    wrow[(size_t)K * D + 0] = loss_sum;
    wrow[(size_t)K * D + 1] = nex;
    wrow[(size_t)K * D + 2] = mist;
    wrow[(size_t)K * D + 3] = 1.f;  // a spoke with rows, labelled or not
  }
}

// The round's fold: the S_act workspace rows in spoke order into the K·D touched entries of
// the accumulator (columns [0, dn) and dim − 1 of each class) and into stats[0..3].
__global__ __launch_bounds__(256) void mcd_fold_kernel(const float* __restrict__ ws, int S_act,
                                                       int dn, int D, int K, int dim,
                                                       float* __restrict__ dacc,
                                                       float* __restrict__ stats) {
  const int KD = K * D;
  const size_t wsw = (size_t)KD + kMcdStat;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < KD) {
    const int k = e / D, j = e - k * D;
    const size_t at = (size_t)k * dim + (j < dn ? j : dim - 1);
    float v = dacc[at];
    for (int s = 0; s < S_act; ++s) v += ws[s * wsw + e];
    dacc[at] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    float t = stats[threadIdx.x];
    for (int s = 0; s < S_act; ++s) t += ws[s * wsw + KD + threadIdx.x];
    stats[threadIdx.x] = t;
  }
}

template <int G>
int launch_mcd(int S_act, hipStream_t st, const McdGeom& geo, const float* W, const void* num,
               int num_bf16, int dn, const void* y, int y_i8, int B, int R, int dim, int K,
               int variant, float C, int bias, float* ws) {
  const size_t lds = mcd_lds_bytes(geo);
  if (num_bf16) {
    if (int e = check_dyn_lds((const void*)mcd_round_kernel<G, true>, lds)) return e;
    hipLaunchKernelGGL((mcd_round_kernel<G, true>), dim3(S_act), dim3(128), lds, st, W, num, dn, y,
                       y_i8, B, R, dim, K, variant, C, bias, ws, geo);
  } else {
    if (int e = check_dyn_lds((const void*)mcd_round_kernel<G, false>, lds)) return e;
    hipLaunchKernelGGL((mcd_round_kernel<G, false>), dim3(S_act), dim3(128), lds, st, W, num, dn,
                       y, y_i8, B, R, dim, K, variant, C, bias, ws, geo);
  }
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace omldm

using namespace omldm;

// 1 when the dense round takes dn numerical columns (+ the bias) and K classes.
OMLDM_API int omldm_multiclass_dense_fits(int dn, int bias, int K) {
  return mcd_fits(dn, bias, K) ? 1 : 0;
}

// Floats of workspace a round of S spokes needs.
OMLDM_API long long omldm_multiclass_dense_ws_words(int K, int D, int S) {
  if (K < 1 || D < 1 || S < 1) return 0;
  return (long long)S * ((long long)K * D + kMcdStat);
}

// One Synchronous round of S exact sequential MultiClassPA spokes of R rows on a batch
// without categorical columns. W: fp32 [nclass][dim]; dacc [nclass][dim] += Σ_s Δ_s in its
// columns [0, dn) and dim − 1 only; stats[0..3] += loss, rows, mistakes, spokes with rows.
// Returns a HIP error code, or < 0 for a shape it does not take (nothing is launched).
OMLDM_API int omldm_multiclass_dense_round(const float* W, const void* num, int num_bf16, int dn,
                                           const void* y, int y_i8, int B, int R, int S, int dim,
                                           int nclass, int variant, float C, int bias,
                                           float* dacc, float* stats, float* ws, void* stream) {
  const int D = dn + (bias ? 1 : 0);
  if (!mcd_fits(dn, bias, nclass)) return -2;
  if (dim < 1 || dn > dim - (bias ? 1 : 0) || D > dim) return -2;
  if (B < 0 || R < 1 || S < 1 || !W || !dacc || !stats || !ws || !y || (dn > 0 && !num)) return -3;
  if (variant < 0 || variant > 2 || !(C > 0.f)) return -4;
  if (B == 0) return 0;
  const McdGeom geo = mcd_geom(D, nclass);
  if (geo.CR < 8 || mcd_lds_bytes(geo) > (size_t)kMcdLds) return -5;
  const long long sact = ((long long)B + R - 1) / R;
  const int S_act = sact < S ? (int)sact : S;
  hipStream_t st = (hipStream_t)stream;
  int e;
#define OMLDM_MCD(GG)                                                                          \
  e = launch_mcd<GG>(S_act, st, geo, W, num, num_bf16, dn, y, y_i8, B, R, dim, nclass, variant, \
                     C, bias, ws)
  switch (geo.G) {
    case 16: OMLDM_MCD(16); break;
    case 8: OMLDM_MCD(8); break;
    case 4: OMLDM_MCD(4); break;
    case 2: OMLDM_MCD(2); break;
    case 1: OMLDM_MCD(1); break;
    default: OMLDM_MCD(0); break;
  }
#undef OMLDM_MCD
  if (e) return e;
  const int KD = nclass * D;
  hipLaunchKernelGGL(mcd_fold_kernel, dim3((KD + 255) / 256), dim3(256), 0, st, ws, S_act, dn, D,
                     nclass, dim, dacc, stats);
  return (int)hipGetLastError();
}
