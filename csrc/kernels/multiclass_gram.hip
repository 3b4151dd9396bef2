// Chunk-Gram dense sequential MultiClassPA round for numerical-only streams past the LDS
// round's box (multiclass_dense.hip: D ≤ 256, K·D ≤ 16384): 1 ≤ D = dn + bias ≤ 2048 columns,
// 2 ≤ K ≤ 256 classes, any R. One Synchronous round of S virtual spokes with the semantics
// of omldm_cpu_multiclass_round (csrc/host/linear_cpu.cpp) at dc = 0, the contract of
// omldm_multiclass_dense_round.
//
// A spoke is one workgroup of 8 waves. The round-start prototypes w0 stay in HBM, read-only;
// the spoke's private delta d[K][D] is its workspace row (HBM/L2), zeroed by the kernel,
// written and re-read by this workgroup only. The rows go in chunks of 64, three phases per
// chunk, __syncthreads() (workgroup-scope release/acquire) between them:
//
//  1. Score and Gram, all waves, v_mfma_f32_32x32x2_f32. D is walked in slabs of 32 columns:
//     the chunk's x slab [64][33] (bias column 1, padding 0) and the model slab w0 + d
//     [Kp][33] (the sum formed per element on the way in, so every product is the oracle's)
//     are staged in LDS, and the 2·Kp/32 score tiles Sc = x·(w0 + d)ᵀ and the 4 Gram tiles
//     Gc = x·xᵀ are accumulated from the same x fragments. Tile t of wave w's work items
//     w, w + 8, … (≤ 3 accumulators); at K ≤ 32 there are 6 tiles, so a slab's 16 k-steps
//     are split four ways as well (24 items) and the partial tiles are summed in LDS in the
//     order of the split. Results: Sc[64][Kp + 1], Gc[64][65] (odd strides: a row read and a
//     column read-modify-write are both conflict-free). Wave 7 (lane i = row i) also sums
//     ‖x‖² from the staged slabs in the oracle's column order and leaves per row the class
//     code (−1 out of range, −2 skipped), τ's denominator and τ's cap (0: no step).
//  2. The chain, wave 0 alone. Row i: each lane reads its ⌈K/64⌉ scores of Sc[i][·], one
//     wave arg-max over the classes other than y (lowest class among equals), the step math
//     in the oracle's operation order (contraction off), the margin parked in lane i; if
//     τ ≠ 0, lanes r > i move the later rows' two scores, Sc[r][y] += τ·Gc[i][r] and
//     Sc[r][rival] −= τ·Gc[i][r], and (i, y, rival, τ) is appended to the chunk's step list.
//     Only the wave's own LDS order (wave_lds_sync) synchronises; nothing depends on D.
//  3. Delta update, all waves. Work item (class k, 256-column block), item i to wave i mod 8;
//     an item whose class no step names costs one ballot. Otherwise lane ℓ owns columns
//     ℓ, ℓ + 64, … of the block: it loads d[k][j], walks the steps that name k in row order
//     adding ±(τ_t·x_t[j]) — the product rounded before the sum, the next step's x loads in
//     flight ahead of the adds — and stores. With equal τ this is the oracle's d bit for bit.
//
// The only numerical freedom against the oracle is the summation order of a score and its
// split into the chunk-start score plus Gram corrections (the v3 multiclass scan's freedom).
// Round end: the workspace row already holds d; wave 0 adds the statistics tail, and a second
// small kernel folds the rows in spoke order into dacc[k][0..dn), dacc[k][dim − 1] and
// stats[0..3] — no float atomics, no waiting between workgroups: a round is bit-reproducible.
#include "spoke_table.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

typedef float mcg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMcgMaxD = 2048;   // columns (dn + bias)
constexpr int kMcgMaxK = 256;    // classes
constexpr int kMcgLds = 160 * 1024;
constexpr int kMcgStat = 8;      // workspace row: K·D deltas, then loss, rows, mistakes, 1
constexpr int kMcgRows = 64;     // rows per chunk
constexpr int kMcgSlab = 32;     // columns per staged slab
constexpr int kMcgXS = kMcgSlab + 1;  // staged row stride (odd)
constexpr int kMcgGS = kMcgRows + 1;  // Gram row stride (odd)
constexpr int kMcgWaves = 8;
constexpr int kMcgThreads = 64 * kMcgWaves;
constexpr int kMcgAcc = 3;       // accumulators per wave: ⌈(2·8 + 4) / 8⌉
constexpr int kMcgCols = 4;      // columns per lane of a phase-3 item

inline bool mcg_fits(int dn, int bias, int K) {
  const int D = dn + (bias ? 1 : 0);
  return dn >= 0 && D >= 1 && D <= kMcgMaxD && K >= 2 && K <= kMcgMaxK;
}

inline int mcg_kpad(int K) { return (K + 31) & ~31; }

inline size_t mcg_lds_bytes(int K) {
  const int Kp = mcg_kpad(K);
  return ((size_t)kMcgRows * (Kp + 1) + kMcgRows * kMcgGS + kMcgRows * kMcgXS +
          (size_t)Kp * kMcgXS + 8 * 64) * sizeof(float);
}

template <bool NBF>
__device__ __forceinline__ float mcg_num(const void* __restrict__ num, size_t i) {
  if (NBF)
    return __uint_as_float((unsigned)static_cast<const unsigned short*>(num)[i] << 16);
  return static_cast<const float*>(num)[i];
}

// Orders one wave's LDS accesses (multiclass_dense.hip: wave_lds_sync).
__device__ __forceinline__ void mcg_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool NBF>
__global__ __launch_bounds__(kMcgThreads) void mcg_round_kernel(
    const float* __restrict__ W, const void* __restrict__ num, int dn,
    const void* __restrict__ y, int y_i8, int B, int R, int dim, int K, int variant, float C,
    int bias, float* ws) {
  extern __shared__ __attribute__((aligned(16))) float mcg_smem[];
  const int Kp = (K + 31) & ~31, SS = Kp + 1, NTs = Kp >> 5;
  float* Sc = mcg_smem;                         // [64][Kp + 1]
  float* Gc = Sc + kMcgRows * SS;               // [64][65]
  float* xs = Gc + kMcgRows * kMcgGS;           // [64][33]
  float* wsl = xs + kMcgRows * kMcgXS;          // [Kp][33]
  float* denL = wsl + Kp * kMcgXS;              // [64]
  float* capL = denL + 64;                      // [64]
  int* ycL = reinterpret_cast<int*>(capL + 64);  // [64]: class, −1 out of range, −2 skipped
  int* stI = ycL + 64;                          // the chunk's steps: row,
  int* stY = stI + 64;                          //   label's class (−1: none moves),
  int* stR = stY + 64;                          //   rival,
  float* stT = reinterpret_cast<float*>(stR + 64);  // τ
  int* nstL = reinterpret_cast<int*>(stT + 64);     // [1] steps in the list
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long a = (long long)s * R;
  if (a >= B) return;  // an idle spoke is no worker of the round (the grid has none)
  const long long b = a + R < (long long)B ? a + R : (long long)B;
  const int nrows = (int)(b - a);
  const int D = dn + (bias ? 1 : 0);
  const float inf = __builtin_inff();
  float* wrow = ws + (size_t)s * ((size_t)K * D + kMcgStat);

  for (int e = tid; e < K * D + kMcgStat; e += kMcgThreads) wrow[e] = 0.f;

  // phase 1's work items of this wave: item = tile·KS + k-split, tile < 2·NTs a score tile
  // (row tile tile & 1, class tile tile >> 1), the last four the Gram's
  const int ksh = NTs == 1 ? 2 : 0, KS = 1 << ksh;
  const int NI = (2 * NTs + 4) << ksh;
  const int l31 = lane & 31, h = lane >> 5;
  const int nk = (kMcgSlab / 2) >> ksh;  // k-steps of a slab per item
  const float* opA[kMcgAcc];
  const float* opB[kMcgAcc];
  float* out[kMcgAcc];   // element (reg 0, this lane) of the item's tile in Sc or Gc
  int ost[kMcgAcc];      // its row stride
#pragma unroll
  for (int i = 0; i < kMcgAcc; ++i) {
    const int it = wave + kMcgWaves * i;
    const int tile = it >> ksh, k0 = (it & (KS - 1)) * nk;
    const int rt = tile & 1, g = tile - 2 * NTs;
    opA[i] = xs + (rt * 32 + l31) * kMcgXS + 2 * k0 + h;
    opB[i] = (g < 0 ? wsl + ((tile >> 1) * 32 + l31) * kMcgXS
                    : xs + ((g >> 1) * 32 + l31) * kMcgXS) + 2 * k0 + h;
    ost[i] = g < 0 ? SS : kMcgGS;
    out[i] = (g < 0 ? Sc + (tile >> 1) * 32 : Gc + (g >> 1) * 32) +
             (rt * 32 + 4 * h) * ost[i] + l31;
  }

  float loss_l = 0.f, nex_l = 0.f, mist_l = 0.f;  // per-lane sums (wave 0)
  const int nchunks = (nrows + kMcgRows - 1) / kMcgRows;
  const int ncb = (D + 64 * kMcgCols - 1) / (64 * kMcgCols);

  for (int ch = 0; ch < nchunks; ++ch) {
    const long long t0 = a + (long long)ch * kMcgRows;
    const int nr = b - t0 < kMcgRows ? (int)(b - t0) : kMcgRows;

    // ---- phase 1: Sc = x·(w0 + d)ᵀ, Gc = x·xᵀ, the rows' norms
    mcg_f32x16 acc[kMcgAcc];
#pragma unroll
    for (int i = 0; i < kMcgAcc; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float pn = 0.f;  // wave 7, lane i: ‖x_i‖²
    for (int j0 = 0; j0 < D; j0 += kMcgSlab) {
      __syncthreads();  // the slab buffers are free (and, at j0 = 0, phase 3's d is visible)
      {
        const int c = tid & 31, j = j0 + c;
        for (int r = tid >> 5; r < kMcgRows; r += kMcgThreads / 32) {
          float v = 0.f;
          if (r < nr) {
            if (j < dn) v = mcg_num<NBF>(num, (size_t)(t0 + r) * dn + j);
            else if (j < D) v = 1.f;
          }
          xs[r * kMcgXS + c] = v;
        }
        const int wcol = j < dn ? j : dim - 1;
        for (int k = tid >> 5; k < Kp; k += kMcgThreads / 32) {
          float v = 0.f;
          if (k < K && j < D) v = W[(size_t)k * dim + wcol] + wrow[(size_t)k * D + j];
          wsl[k * kMcgXS + c] = v;
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kMcgAcc; ++i) {
        if (wave + kMcgWaves * i < NI) {
#pragma unroll 4
          for (int u = 0; u < nk; ++u)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(opA[i][2 * u], opB[i][2 * u], acc[i],
                                                          0, 0, 0);
        }
      }
      if (wave == kMcgWaves - 1) {
#pragma unroll 8
        for (int c = 0; c < kMcgSlab; ++c) {
          const float xv = xs[lane * kMcgXS + c];
          pn += xv * xv;
        }
      }
    }
    if (wave == kMcgWaves - 1) {
      const bool in = lane < nr;
      const float yv = load_label(y, (int)(in ? t0 + lane : b - 1), y_i8);
      const bool skip = !in || yv != yv;
      float cap = 0.f, den = 1.f;
      if (!skip && pn > 0.f) {
        den = 2.f * pn;
        if (variant == 2) den = den + 0.5f / C;
        cap = variant == 1 ? C : inf;
      }
      int yc = -2;
      if (!skip) yc = (yv > -1.f && yv < (float)K) ? (int)yv : -1;
      denL[lane] = den;
      capL[lane] = cap;
      ycL[lane] = yc;
    }
    // the tiles to LDS: C/D map (32×32) col = lane & 31, row = (reg & 3) + 8·(reg >> 2) +
    // 4·(lane >> 5); the k-splits of a tile one after the other, the first one stores
    for (int q = 0; q < KS; ++q) {
#pragma unroll
      for (int i = 0; i < kMcgAcc; ++i) {
        const int it = wave + kMcgWaves * i;
        if (it < NI && (it & (KS - 1)) == q) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* p = out[i] + ((r & 3) + 8 * (r >> 2)) * ost[i];
            *p = q == 0 ? acc[i][r] : *p + acc[i][r];
          }
        }
      }
      __syncthreads();
    }

    // ---- phase 2: the chunk's rows in order, wave 0
    if (wave == 0) {
      const int ycv = ycL[lane];
      const float denv = denL[lane], capv = capL[lane];
      float mpark = 0.f;  // lane i: the margin of row i
      int n = 0;
      for (int i = 0; i < nr; ++i) {
        const int yc = __builtin_amdgcn_readlane(ycv, i);
        if (yc == -2) continue;  // unlabelled: no step, no statistics
        const float den = readlane_f(denv, i), cap = readlane_f(capv, i);
        const float* row = Sc + i * SS;
        float bv = -inf;
        int bk = 0;
#pragma unroll
        for (int c = 0; c < kMcgMaxK / 64; ++c) {
          const int kc = lane + 64 * c;
          if (kc < K && kc != yc) {
            const float sv = row[kc];
            if (sv > bv) {
              bv = sv;
              bk = kc;
            }
          }
        }
        const float m = wave_max(bv);
        const bool any = m > -inf;
        // the lowest class among the lanes that hold the maximum
        const float low = -wave_max(bv == m ? -(float)bk : -inf);
        const int rr = any ? (int)low : 0;
        const float sy = yc >= 0 ? row[yc] : 0.f;
        const float margin = sy - m;
        const float loss = fmaxf(0.f, 1.f - margin);
        float tau = fminf(cap, loss / den);
        if (!any) tau = 0.f;
        tau = readlane_f(tau, 0);  // (the same bits in every lane)
        mpark = lane == i ? margin : mpark;
        if (tau != 0.f) {
          if (lane > i) {  // the later rows' scores of the two classes that move
            const float t = tau * Gc[i * kMcgGS + lane];
            if (yc >= 0) Sc[lane * SS + yc] += t;
            Sc[lane * SS + rr] -= t;
          }
          if (lane == 0) {
            stI[n] = i;
            stY[n] = yc;
            stR[n] = rr;
            stT[n] = tau;
          }
          ++n;
          mcg_wave_lds_sync();  // the next row's lanes read what other lanes wrote
        }
      }
      if (lane == 0) nstL[0] = n;
      if (lane < nr && ycv != -2) {
        nex_l += 1.f;
        loss_l += fmaxf(0.f, 1.f - mpark);
        mist_l += mpark <= 0.f ? 1.f : 0.f;
      }
    }
    __syncthreads();

    // ---- phase 3: d[k] ±= τ_t·x_t over the chunk's steps, all waves
    const int n = nstL[0];
    if (n > 0) {
      int si = 0, sy = -3, sr = -3;
      float st = 0.f;
      if (lane < n) {
        si = stI[lane];
        sy = stY[lane];
        sr = stR[lane];
        st = stT[lane];
      }
      for (int item = wave; item < K * ncb; item += kMcgWaves) {
        const int k = item / ncb, cb = item - k * ncb;
        unsigned long long m = __builtin_amdgcn_ballot_w64(sy == k || sr == k);
        if (!m) continue;
        const int jb = cb * 64 * kMcgCols + lane;
        float* dk = wrow + (size_t)k * D;
        float dv[kMcgCols], xv[kMcgCols], xn[kMcgCols];
#pragma unroll
        for (int u = 0; u < kMcgCols; ++u) {
          dv[u] = jb + 64 * u < D ? dk[jb + 64 * u] : 0.f;
          xn[u] = 0.f;
        }
        auto load_x = [&](int t, float* x) {
          const size_t base = (size_t)(t0 + __builtin_amdgcn_readlane(si, t)) * dn;
#pragma unroll
          for (int u = 0; u < kMcgCols; ++u) {
            const int j = jb + 64 * u;
            x[u] = j < dn ? mcg_num<NBF>(num, base + j) : (j < D ? 1.f : 0.f);
          }
        };
        load_x(__builtin_ctzll(m), xv);
        while (m) {
          const int t = __builtin_ctzll(m);
          m &= m - 1;
          if (m) load_x(__builtin_ctzll(m), xn);  // the next step's loads go ahead
          const float tau = readlane_f(st, t);
          const bool up = __builtin_amdgcn_readlane(sy, t) == k;
#pragma unroll
          for (int u = 0; u < kMcgCols; ++u) {
            const float p = tau * xv[u];
            dv[u] = up ? dv[u] + p : dv[u] - p;
            xv[u] = xn[u];
          }
        }
#pragma unroll
        for (int u = 0; u < kMcgCols; ++u)
          if (jb + 64 * u < D) dk[jb + 64 * u] = dv[u];
      }
    }
    // (the next chunk's first barrier, or the kernel's end, publishes d)
  }
  if (wave != 0) return;

  const float loss_sum = wave_sum(loss_l), nex = wave_sum(nex_l), mist = wave_sum(mist_l);
  if (lane == 0) {
    wrow[(size_t)K * D + 0] = loss_sum;
    wrow[(size_t)K * D + 1] = nex;
    wrow[(size_t)K * D + 2] = mist;
    wrow[(size_t)K * D + 3] = 1.f;  // a spoke with rows, labelled or not
  }
}

// The round's fold (multiclass_dense.hip: mcd_fold_kernel): the S_act workspace rows in spoke
// order into the K·D touched entries of the accumulator (columns [0, dn) and dim − 1 of each
// class) and into stats[0..3].
__global__ __launch_bounds__(256) void mcg_fold_kernel(const float* __restrict__ ws, int S_act,
                                                       int dn, int D, int K, int dim,
                                                       float* __restrict__ dacc,
                                                       float* __restrict__ stats) {
  const int KD = K * D;
  const size_t wsw = (size_t)KD + kMcgStat;
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

template <bool NBF>
int launch_mcg(int S_act, hipStream_t st, const float* W, const void* num, int dn, const void* y,
               int y_i8, int B, int R, int dim, int K, int variant, float C, int bias,
               float* ws) {
  const size_t lds = mcg_lds_bytes(K);
  if (int e = check_dyn_lds((const void*)mcg_round_kernel<NBF>, lds)) return e;
  hipLaunchKernelGGL((mcg_round_kernel<NBF>), dim3(S_act), dim3(kMcgThreads), lds, st, W, num, dn,
                     y, y_i8, B, R, dim, K, variant, C, bias, ws);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace omldm

using namespace omldm;

// 1 when the chunk-Gram round takes dn numerical columns (+ the bias) and K classes.
OMLDM_API int omldm_multiclass_gram_fits(int dn, int bias, int K) {
  return mcg_fits(dn, bias, K) ? 1 : 0;
}

// Floats of workspace a round of S spokes needs.
OMLDM_API long long omldm_multiclass_gram_ws_words(int K, int D, int S) {
  if (K < 1 || D < 1 || S < 1) return 0;
  return (long long)S * ((long long)K * D + kMcgStat);
}

// One Synchronous round of S exact sequential MultiClassPA spokes of R rows on a batch
// without categorical columns. W: fp32 [nclass][dim]; dacc [nclass][dim] += Σ_s Δ_s in its
// columns [0, dn) and dim − 1 only; stats[0..3] += loss, rows, mistakes, spokes with rows.
// Returns a HIP error code, or < 0 for a shape it does not take (nothing is launched).
OMLDM_API int omldm_multiclass_gram_round(const float* W, const void* num, int num_bf16, int dn,
                                          const void* y, int y_i8, int B, int R, int S, int dim,
                                          int nclass, int variant, float C, int bias,
                                          float* dacc, float* stats, float* ws, void* stream) {
  const int D = dn + (bias ? 1 : 0);
  if (!mcg_fits(dn, bias, nclass)) return -2;
  if (dim < 1 || dn > dim - (bias ? 1 : 0) || D > dim) return -2;
  if (B < 0 || R < 1 || S < 1 || !W || !dacc || !stats || !ws || !y || (dn > 0 && !num)) return -3;
  if (variant < 0 || variant > 2 || !(C > 0.f)) return -4;
  if (B == 0) return 0;
  if (mcg_lds_bytes(nclass) > (size_t)kMcgLds) return -5;
  const long long sact = ((long long)B + R - 1) / R;
  const int S_act = sact < S ? (int)sact : S;
  hipStream_t st = (hipStream_t)stream;
  const int e = num_bf16 ? launch_mcg<true>(S_act, st, W, num, dn, y, y_i8, B, R, dim, nclass,
                                            variant, C, bias, ws)
                         : launch_mcg<false>(S_act, st, W, num, dn, y, y_i8, B, R, dim, nclass,
                                             variant, C, bias, ws);
  if (e) return e;
  const int KD = nclass * D;
  hipLaunchKernelGGL(mcg_fold_kernel, dim3((KD + 255) / 256), dim3(256), 0, st, ws, S_act, dn, D,
                     nclass, dim, dacc, stats);
  return (int)hipGetLastError();
}
