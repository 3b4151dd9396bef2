// ORR solve: w = fp32((G[:n, :n] + shift·I)⁻¹ G[:n, n]), n = d + 1 ≤ 128, in one launch of one
// workgroup (8 waves), fp64 throughout, everything LDS-resident from load to result.
//
// G is the fp64 master Gram of z = [x, 1, y] (omldm_amd/models/dense.py ORR): A is its leading
// n × n block, b its column n. shift = λ when λ > 0, else the relative jitter
// 1e-12·trace(A)/n + 1e-30 — the semantics of ORR.weights().
//
// Layout. A padded square in LDS, row stride S = NP + 1 doubles (NP = n rounded up to 16; the odd
// stride keeps the 16 rows of a tile on distinct banks):
//   rows 0 .. NP−1    the lower triangle of A (upper tiles are never read); columns n .. NP−1 are
//                     padded with an identity diagonal, so partial panels factor to 1 and solve to 0
//   rows NP .. NP+15  one more tile row: row NP carries b, the rest is zero
// plus NP reciprocal pivots and two scalars: ((NP + 16)·(NP + 1) + NP + 2)·8 bytes, 149,648 B at
// n = 128 (of the CU's 160 KiB), 4,496 B at n ≤ 16.
//
// Algorithm: blocked right-looking Cholesky on 16-column panels.
//   1. wave 0 factors the 16 × 16 diagonal block in registers (lane = row; pivots and multipliers
//      cross lanes by v_readlane). The fp64 sqrt and division of the factorisation sit here only
//      (one more division forms the mean of the λ = 0 jitter).
//   2. all waves solve the rows below against L11ᵀ, one row per lane, rows dealt round-robin
//      over the waves (multiplications by the stored reciprocal pivots, no division).
//   3. A22 −= L21·L21ᵀ on v_mfma_f64_16x16x4_f64, operands straight from LDS, lower-triangle tiles
//      only, tiles dealt round-robin over the waves.
// The b row rides along as one more row of L21, so when the last panel is done row NP holds
// y = L⁻¹b and no forward pass exists. Back substitution Lᵀw = y runs panel by panel from the
// bottom: wave 0 does the 16 sequential steps of a block in registers, then all threads fold
// that block's weights into the y entries above it.
//
// A pivot that is not > 0 (possible only for a loaded model) never traps or spins: sqrt and the
// division produce NaN/Inf, the loops do not depend on data, and the kernel writes NaN weights.
//
// Past 128 unknowns the matrix outgrows the LDS of one CU: omldm_orr_solve_blocked (second half of
// this file) keeps the factor in an HBM workspace and runs the same panel steps on 64 × 64 blocks,
// one launch per block column, for n ≤ 512.
#include "common.h"

namespace omldm {
namespace {

constexpr int kOrrMaxN = 128;
constexpr int kOrrWaves = 8;
constexpr int kOrrThreads = kOrrWaves * kWave;

typedef double d4_t __attribute__((ext_vector_type(4)));

// Lane `lane` (a constant) of v as a wave-uniform value.
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

inline size_t orr_lds_bytes(int n) {
  const size_t NP = (size_t)((n + 15) / 16) * 16;
  return ((NP + 16) * (NP + 1) + NP + 2) * sizeof(double);
}

// The steps of one 16-column panel, shared by the LDS-resident and the blocked kernel.
//
// Diagonal block, one wave: lane i (mod 16) owns the row `row` points at. Entries on and right of
// the diagonal are carried along unmasked: they never feed an entry left of it, and nothing reads
// them back (every later step divides by the pivot through invd).
__device__ __forceinline__ void orr_factor_diag16(double* row, double* invd, int lane, bool& bad) {
  double a[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) a[k] = row[k];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double djj = readlane_d(a[j], j);
    bad |= !(djj > 0.0);
    const double inv = 1.0 / sqrt(djj);
    if (lane == 0) invd[j] = inv;
    a[j] *= inv;
#pragma unroll
    for (int k = j + 1; k < 16; ++k) {
      a[k] -= a[j] * readlane_d(a[j], k);
      // the update happens here: sunk to where a[k] is next read, all 120 multipliers would
      // have to stay live in SGPRs
      asm volatile("" : "+v"(a[k]));
    }
  }
  if (lane < 16) {
#pragma unroll
    for (int k = 0; k < 16; ++k) row[k] = a[k];
  }
}

// One row below the block: x·L11ᵀ = a in place, L11 and the row at LDS row stride S.
template <int S>
__device__ __forceinline__ void orr_solve_row16(double* row, const double* L11,
                                                const double* invd) {
  double x[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) x[k] = row[k];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    x[j] *= invd[j];
#pragma unroll
    for (int k = j + 1; k < 16; ++k) x[k] -= x[j] * L11[k * S + j];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) row[k] = x[k];
}

// acc −= La·Lbᵀ over 4·KS columns on the fp64 MFMA, La and Lb already offset to the lane's
// (row l % 16, column l / 16): A operand −La[16·ti + i][4s + k], B operand Lb[16·tj + i][4s + k];
// accumulator register v of lane l is C[4v + l / 16][l % 16].
template <int KS>
__device__ __forceinline__ d4_t orr_tile_mfma(const double* La, const double* Lb, d4_t acc) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-La[4 * s], Lb[4 * s], acc, 0, 0, 0);
  return acc;
}

// One 16 × 16 tile of the trailing update of a panel, C (offset to row l / 16, column l % 16)
// read from and written back to LDS.
template <int S>
__device__ __forceinline__ void orr_tile_update(const double* La, const double* Lb, double* C) {
  d4_t acc;
#pragma unroll
  for (int v = 0; v < 4; ++v) acc[v] = C[4 * v * S];
  acc = orr_tile_mfma<4>(La, Lb, acc);
#pragma unroll
  for (int v = 0; v < 4; ++v) C[4 * v * S] = acc[v];
}

// The 16 sequential steps of a block of the back substitution, one wave: lane k (mod 16) owns
// y[k] (yk), its reciprocal pivot ik and column k of the diagonal block (Lc). Lanes k ≥ i are
// done at step i: what the update leaves in them is not read again.
__device__ __forceinline__ void orr_backsub16(const double (&Lc)[16], double yk, double ik,
                                              double* y, int lane) {
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    const double wi = readlane_d(yk * ik, i);
    if (lane == 0) y[i] = wi;
    yk -= Lc[i] * wi;
  }
}

// TC: the number of 16-column panels, a template constant so that every LDS row offset is an
// immediate of the ds instruction and not a scalar product kept live across the panel loop.
template <int TC>
__global__ __launch_bounds__(kOrrThreads) void orr_solve_kernel(const double* __restrict__ G,
                                                                int ld, int n, double lam,
                                                                float* __restrict__ w) {
  extern __shared__ double orr_sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NP = TC << 4, S = NP + 1, MP = NP + 16;
  double* A = orr_sm;
  double* invd = A + MP * S;  // 1 / L[j][j]
  double* scal = invd + NP;   // [0]: a pivot was not > 0
  double* y = A + NP * S;     // the b row: L⁻¹b after the factorisation, then w

  // ---- load: G's lower triangle and column n once from HBM, λ on the diagonal on the way in
  {
    const double add = lam > 0.0 ? lam : 0.0;
    const int c = tid & 127;
    if (c < NP) {
      for (int r = tid >> 7; r < MP; r += kOrrThreads / 128) {
        double v = 0.0;
        if (r < n) {
          if (c <= r) v = G[(size_t)r * ld + c];
          if (c == r) v += add;
        } else if (r < NP) {
          v = c == r ? 1.0 : 0.0;
        } else if (r == NP && c < n) {
          v = G[(size_t)c * ld + n];
        }
        A[r * S + c] = v;
      }
    }
  }
  if (!(lam > 0.0)) {  // λ = 0: the relative jitter, from the trace of what was just loaded
    __syncthreads();
    if (wave == 0) {
      double t = 0.0;
      for (int i = lane; i < n; i += kWave) t += A[i * S + i];
      for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o);
      const double shift = 1e-12 * (t / (double)n) + 1e-30;
      for (int i = lane; i < n; i += kWave) A[i * S + i] += shift;
    }
  }
  __syncthreads();

  bool bad = false;  // meaningful in wave 0, where it is wave-uniform
  for (int p = 0; p < TC; ++p) {
    const int c0 = p << 4;
    // ---- 1. diagonal block, wave 0
    if (wave == 0)
      orr_factor_diag16(A + (c0 + (lane & 15)) * S + c0, invd + c0, lane, bad);
    __syncthreads();

    // ---- 2. rows below the block, then the b row: x·L11ᵀ = a, one row per lane
    {
      const int R = NP - c0 - 15;  // NP − c0 − 16 rows of A, and the b row
      const int q = lane * kOrrWaves + wave;
      if (q < R)
        orr_solve_row16<S>(A + (q == R - 1 ? NP : c0 + 16 + q) * S + c0, A + c0 * S + c0,
                           invd + c0);
    }
    __syncthreads();
    if (p == TC - 1) break;  // nothing trails the last panel

    // ---- 3. trailing update on the fp64 MFMA
    {
      const int li = lane & 15, lk = lane >> 4;
      int t = 0;
      for (int ti = p + 1; ti <= TC; ++ti) {
        const int tjmax = ti < TC ? ti : TC - 1;  // tile row TC (the b row) has no diagonal tile
        for (int tj = p + 1; tj <= tjmax; ++tj, ++t) {
          if ((t & (kOrrWaves - 1)) != wave) continue;
          orr_tile_update<S>(A + (ti * 16 + li) * S + c0 + lk, A + (tj * 16 + li) * S + c0 + lk,
                             A + (ti * 16 + lk) * S + tj * 16 + li);
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) scal[0] = bad ? 1.0 : 0.0;

  // ---- back substitution Lᵀw = y, bottom panel first
  for (int p = TC - 1; p >= 0; --p) {
    const int c0 = p << 4;
    if (wave == 0) {  // lane k (mod 16) owns y[c0 + k] and column k of the diagonal block
      const int k = lane & 15;
      double Lc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) Lc[i] = A[(c0 + i) * S + c0 + k];
      orr_backsub16(Lc, y[c0 + k], invd[c0 + k], y + c0, lane);
    }
    __syncthreads();
    if (tid < c0) {
      double acc = y[tid];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc -= A[(c0 + i) * S + tid] * y[c0 + i];
      y[tid] = acc;
    }
    __syncthreads();
  }
  if (tid < n) w[tid] = scal[0] != 0.0 ? __builtin_nanf("") : (float)y[tid];
}

template <int TC>
int launch_orr(const double* G, int ld, int n, double lam, float* w, hipStream_t st) {
  const size_t lds = orr_lds_bytes(n);
  const int e = check_dyn_lds((const void*)orr_solve_kernel<TC>, lds);
  if (e) return e;
  hipLaunchKernelGGL(orr_solve_kernel<TC>, dim3(1), dim3(kOrrThreads), lds, st, G, ld, n, lam, w);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ blocked solve, n ≤ 512
// The factor lives in an HBM workspace (2.1 MB at n = 512: it stays in L2), cut into 64 × 64
// blocks; NPAD = n rounded up to 64, nb = NPAD / 64, padding as above (identity diagonal, zero b).
// Workspace, in doubles:
//   [0, NPAD²)             L, row-major at row stride NPAD (blocks right of the diagonal unused)
//   [NPAD², +NPAD)         the b row: y = L⁻¹b once the last block column is done
//   then NPAD              reciprocal pivots
//   then nb                per block column: a pivot was not > 0
//
// Left-looking over block columns, one launch per block column p and one workgroup per block
// row i ≥ p, the b row being one more block row (i = nb, one real row in one 16-row tile):
//   1. stream L[p, 0:64p] and L[i, 0:64p] from the workspace through LDS in 64-column chunks (the
//      next chunk's loads are in flight in registers while the MFMAs run on the current one);
//   2. D = A[p,p] − L[p,:]·L[p,:]ᵀ and E = A[i,p] − L[i,:]·L[p,:]ᵀ on v_mfma_f64_16x16x4_f64, each
//      wave keeping its ≤ 4 tiles of [D; E] in registers across the chunks;
//   3. the four 16-column panel steps of the LDS-resident kernel on the stacked [D; E] in LDS. D
//      is factored by every workgroup of the launch redundantly, so no workgroup ever waits on
//      another: the order of dependent steps is stream order alone. E's rows ride along as rows
//      below the block (as the b row does above), which leaves E·L_pp⁻ᵀ without a pass of its own (a
//      row-per-lane solve against all 64 columns would be a chain of 2016 fmas per lane);
//   4. write L[i,p]; workgroup i = p writes L_pp, the reciprocal pivots and the pivot flag.
// A last one-workgroup launch does the back substitution from the workspace, casts and writes w.
// Loop trip counts depend on n, p and i only.
constexpr int kOrrBlockedMaxN = 512;
constexpr int kBlk = 64;        // block edge
constexpr int kBS = kBlk + 1;   // LDS row stride of a block (odd: 16 rows of a tile, 16 banks)

inline int orr_npad(int n) { return (n + kBlk - 1) / kBlk * kBlk; }

inline size_t orr_blocked_ws_bytes(int n) {
  const size_t NPAD = (size_t)orr_npad(n);
  return ((NPAD + 1) * NPAD + NPAD + NPAD / kBlk) * sizeof(double);
}

// [D; E] (128 rows), the chunks of L[p,:] and L[i,:], 64 reciprocal pivots, 8 wave sums
constexpr size_t kOrrColLds = (size_t)(4 * kBlk * kBS + kBlk + kOrrWaves) * sizeof(double);

__global__ __launch_bounds__(kOrrThreads) void orr_block_column_kernel(
    const double* __restrict__ G, int ld, int n, double lam, int p, double* __restrict__ work) {
  extern __shared__ double orr_sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NPAD = (n + kBlk - 1) / kBlk * kBlk, nb = NPAD / kBlk;
  const int i = p + (int)blockIdx.x;       // block row; nb: the b row
  const bool diag = i == p, brow = i == nb;
  const int ET = diag ? 0 : brow ? 1 : 4;  // tile rows of E
  double* M = orr_sm;                      // rows 0 .. 63: D, rows 64 .. 127: E
  double* Lp = M + 2 * kBlk * kBS;         // a chunk of L[p, :]
  double* Li = Lp + kBlk * kBS;            // the same columns of L[i, :]
  double* invd = Li + kBlk * kBS;          // 1 / L_pp[j][j]
  double* red = invd + kBlk;
  double* Lw = work;
  double* yw = Lw + (size_t)NPAD * NPAD;
  const int c = tid & 63, r0 = tid >> 6;   // the thread's column and first row of a 64-wide load
  const int P0 = p * kBlk, I0 = i * kBlk;

  // ---- shift: λ, or for λ = 0 the relative jitter from the trace (every workgroup sums it)
  double shift = lam;
  if (!(lam > 0.0)) {
    double t = tid < n ? G[(size_t)tid * ld + tid] : 0.0;  // n ≤ 512 threads
    for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) red[wave] = t;
    __syncthreads();
    t = 0.0;
    for (int k = 0; k < kOrrWaves; ++k) t += red[k];
    shift = 1e-12 * (t / (double)n) + 1e-30;
  }

  // ---- A[p,p] and A[i,p] from G: the lower triangle and column n only, the shift on the way in
  for (int j = 0; j < (diag ? 8 : 16); ++j) {
    const int rr = r0 + 8 * j, gc = P0 + c;
    double v = 0.0;
    if (rr < kBlk) {
      const int gr = P0 + rr;
      if (gr < n) {
        if (c <= rr) v = G[(size_t)gr * ld + gc];
        if (c == rr) v += shift;
      } else {
        v = c == rr ? 1.0 : 0.0;
      }
    } else if (brow) {
      if (rr == kBlk && gc < n) v = G[(size_t)gc * ld + n];
    } else {
      const int gr = I0 + rr - kBlk;
      if (gr < n) v = G[(size_t)gr * ld + gc];  // gc < 64·i ≤ gr
    }
    M[rr * kBS + c] = v;
  }

  // ---- 1, 2. the left-looking update. Tile t of [D; E]: 0 .. 9 the lower tiles of D, 10 + 4e + tj
  // tile (e, tj) of E; wave w owns tiles w, w + 8, w + 16, w + 24
  const int li = lane & 15, lk = lane >> 4;
  if (p > 0) {
    int ti[4], tj[4];
    bool on[4];
    d4_t acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int t = wave + 8 * s;
      if (t < 10) {
        ti[s] = t < 1 ? 0 : t < 3 ? 1 : t < 6 ? 2 : 3;
        tj[s] = t - ti[s] * (ti[s] + 1) / 2;
        on[s] = true;
      } else {
        ti[s] = 4 + ((t - 10) >> 2);
        tj[s] = (t - 10) & 3;
        on[s] = ti[s] - 4 < ET;
      }
      acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
    }
    double pp[8], pi[8];  // the chunk in flight: rows r0 + 8j of L[p, :] and L[i, :], column c
    auto fetch = [&](int kc) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int rr = r0 + 8 * j;
        pp[j] = Lw[(size_t)(P0 + rr) * NPAD + kc * kBlk + c];
        pi[j] = 0.0;
        if (brow) {
          if (rr == 0) pi[j] = yw[kc * kBlk + c];
        } else if (!diag) {
          pi[j] = Lw[(size_t)(I0 + rr) * NPAD + kc * kBlk + c];
        }
      }
    };
    fetch(0);
    for (int kc = 0; kc < p; ++kc) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        Lp[(r0 + 8 * j) * kBS + c] = pp[j];
        Li[(r0 + 8 * j) * kBS + c] = pi[j];
      }
      __syncthreads();
      if (kc + 1 < p) fetch(kc + 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (!on[s]) continue;
        // E's tile rows 4 .. 7 follow D's in LDS: Li starts 64 rows after Lp
        acc[s] = orr_tile_mfma<16>(Lp + (ti[s] * 16 + li) * kBS + lk,
                                   Lp + (tj[s] * 16 + li) * kBS + lk, acc[s]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!on[s]) continue;
      double* C = M + (ti[s] * 16 + lk) * kBS + tj[s] * 16 + li;
#pragma unroll
      for (int v = 0; v < 4; ++v) C[4 * v * kBS] += acc[s][v];
    }
  }
  __syncthreads();

  // ---- 3. the panel steps on [D; E]
  const int erows = diag ? 0 : brow ? 1 : kBlk;
  bool bad = false;  // meaningful in wave 0, where it is wave-uniform
  for (int q = 0; q < 4; ++q) {
    const int c0 = q << 4;
    if (wave == 0) orr_factor_diag16(M + (c0 + (lane & 15)) * kBS + c0, invd + c0, lane, bad);
    __syncthreads();
    {
      const int below = kBlk - 16 - c0;  // rows of D under the diagonal block
      const int x = lane * kOrrWaves + wave;
      if (x < below + erows)
        orr_solve_row16<kBS>(M + (x < below ? c0 + 16 + x : kBlk + x - below) * kBS + c0,
                             M + c0 * kBS + c0, invd + c0);
    }
    __syncthreads();
    if (q == 3) break;  // nothing trails the last panel
    int t = 0;
    for (int a = q + 1; a < 4 + ET; ++a) {
      const int bmax = a < 4 ? a : 3;
      for (int b = q + 1; b <= bmax; ++b, ++t) {
        if ((t & (kOrrWaves - 1)) != wave) continue;
        orr_tile_update<kBS>(M + (a * 16 + li) * kBS + c0 + lk, M + (b * 16 + li) * kBS + c0 + lk,
                             M + (a * 16 + lk) * kBS + b * 16 + li);
      }
    }
    __syncthreads();
  }

  // ---- 4. L[i,p] to the workspace; the diagonal workgroup writes L_pp, pivots and flag
  if (diag) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      Lw[(size_t)(P0 + r0 + 8 * j) * NPAD + P0 + c] = M[(r0 + 8 * j) * kBS + c];
    if (tid < kBlk) yw[NPAD + P0 + tid] = invd[tid];
    if (tid == 0) yw[2 * NPAD + p] = bad ? 1.0 : 0.0;
  } else if (brow) {
    if (tid < kBlk) yw[P0 + tid] = M[kBlk * kBS + tid];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      Lw[(size_t)(I0 + r0 + 8 * j) * NPAD + P0 + c] = M[(kBlk + r0 + 8 * j) * kBS + c];
  }
}

// Back substitution Lᵀw = y from the workspace, one workgroup, bottom panel first as above. The
// rows of L that a panel folds into the entries above it, and its diagonal block, do not depend
// on the solution: they are loaded one panel ahead, so the 16 sequential steps and the fold of a
// panel run while the next panel's loads are in flight.
__global__ __launch_bounds__(kOrrThreads) void orr_backsub_kernel(
    const double* __restrict__ work, int n, float* __restrict__ w) {
  extern __shared__ double orr_sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NPAD = (n + kBlk - 1) / kBlk * kBlk, nb = NPAD / kBlk;
  const double* Lw = work;
  const double* yw = Lw + (size_t)NPAD * NPAD;
  double* y = orr_sm;
  double* invd = y + NPAD;
  if (tid < NPAD) {  // NPAD ≤ 512 threads
    y[tid] = yw[tid];
    invd[tid] = yw[NPAD + tid];
  }
  bool bad = false;
  for (int j = 0; j < nb; ++j) bad |= yw[2 * NPAD + j] != 0.0;

  double cur[16], dcur[16], nxt[16], dnxt[16];
  // Every thread issues all 32 loads, those it has no use for included (threads ≥ c0 read blocks
  // right of the diagonal, which hold nothing; waves 1 .. 7 the diagonal block): with no branch
  // around a load the compiler can count the loads in flight, and wave 0's wait for the current
  // panel leaves the next panel's outstanding.
  const int col = tid < NPAD ? tid : NPAD - 1;
  auto fetch = [&](int c0, double (&f)[16], double (&dg)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      f[k] = Lw[(size_t)(c0 + k) * NPAD + col];
      dg[k] = Lw[(size_t)(c0 + k) * NPAD + c0 + (lane & 15)];
    }
  };
  fetch(NPAD - 16, cur, dcur);
  __syncthreads();
  for (int c0 = NPAD - 16; c0 >= 0; c0 -= 16) {
    fetch(c0 > 0 ? c0 - 16 : 0, nxt, dnxt);  // (the last one is not used)
    if (wave == 0)  // lane k (mod 16) owns y[c0 + k] and column k of the diagonal block
      orr_backsub16(dcur, y[c0 + (lane & 15)], invd[c0 + (lane & 15)], y + c0, lane);
    __syncthreads();
    if (tid < c0) {
      double acc = y[tid];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc -= cur[k] * y[c0 + k];
      y[tid] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      cur[k] = nxt[k];
      dcur[k] = dnxt[k];
    }
  }
  if (tid < n) w[tid] = bad ? __builtin_nanf("") : (float)y[tid];
}

int launch_orr_blocked(const double* G, int ld, int n, double lam, float* w, double* work,
                       hipStream_t st) {
  const int nb = orr_npad(n) / kBlk;
  for (int p = 0; p < nb; ++p) {
    const int e = check_dyn_lds((const void*)orr_block_column_kernel, kOrrColLds);
    if (e) return e;
    hipLaunchKernelGGL(orr_block_column_kernel, dim3(nb - p + 1), dim3(kOrrThreads), kOrrColLds,
                       st, G, ld, n, lam, p, work);
    const int le = (int)hipGetLastError();
    if (le) return le;
  }
  const size_t lds = (size_t)2 * orr_npad(n) * sizeof(double);
  const int e = check_dyn_lds((const void*)orr_backsub_kernel, lds);
  if (e) return e;
  hipLaunchKernelGGL(orr_backsub_kernel, dim3(1), dim3(kOrrThreads), lds, st,
                     (const double*)work, n, w);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace omldm

// w[0 .. d] = fp32 of the ridge solution held by the fp64 Gram G (row stride ld ≥ d + 2) of
// [x, 1, y]: (G[:n, :n] + λI)⁻¹ G[:n, n] with n = d + 1, or the relative jitter in λ's place when
// λ = 0. G is read at indices < d + 2 only. Returns a HIP error code, −1 for ld < d + 2, −2 for
// n > 128 (the caller keeps its library path), −3 for other bad arguments; nothing is launched
// on a negative return.
OMLDM_API int omldm_orr_solve(const double* G, int ld, int d, double lam, float* w, void* stream) {
  using namespace omldm;
  if (d < 0 || ld < d + 2) return -1;
  const int n = d + 1;
  if (n > kOrrMaxN) return -2;
  if (!G || !w || !(lam >= 0.0)) return -3;
  switch ((n + 15) / 16) {
    case 1: return launch_orr<1>(G, ld, n, lam, w, (hipStream_t)stream);
    case 2: return launch_orr<2>(G, ld, n, lam, w, (hipStream_t)stream);
    case 3: return launch_orr<3>(G, ld, n, lam, w, (hipStream_t)stream);
    case 4: return launch_orr<4>(G, ld, n, lam, w, (hipStream_t)stream);
    case 5: return launch_orr<5>(G, ld, n, lam, w, (hipStream_t)stream);
    case 6: return launch_orr<6>(G, ld, n, lam, w, (hipStream_t)stream);
    case 7: return launch_orr<7>(G, ld, n, lam, w, (hipStream_t)stream);
    default: return launch_orr<8>(G, ld, n, lam, w, (hipStream_t)stream);
  }
}

// Bytes of workspace omldm_orr_solve_blocked needs for d + 1 unknowns (the layout is described at
// the blocked kernels above); −1 where it refuses d.
OMLDM_API long long omldm_orr_solve_blocked_ws_bytes(int d) {
  if (d < 0 || d + 1 > omldm::kOrrBlockedMaxN) return -1;
  return (long long)omldm::orr_blocked_ws_bytes(d + 1);
}

// omldm_orr_solve for 1 ≤ n = d + 1 ≤ 512: the same result from the blocked factorisation in the
// workspace `work` (8-byte aligned, work_bytes ≥ omldm_orr_solve_blocked_ws_bytes(d); what it
// holds on entry does not matter), ⌈n / 64⌉ + 1 launches in stream order. Returns a HIP error
// code, −1 for ld < d + 2, −2 for n > 512, −3 for other bad arguments or a workspace that is too
// small; nothing is launched on a negative return.
OMLDM_API int omldm_orr_solve_blocked(const double* G, int ld, int d, double lam, float* w,
                                      void* work, long long work_bytes, void* stream) {
  using namespace omldm;
  if (d < 0 || ld < d + 2) return -1;
  const int n = d + 1;
  if (n > kOrrBlockedMaxN) return -2;
  if (!G || !w || !(lam >= 0.0) || !work || ((uintptr_t)work & 7) ||
      work_bytes < (long long)orr_blocked_ws_bytes(n))
    return -3;
  return launch_orr_blocked(G, ld, n, lam, w, (double*)work, (hipStream_t)stream);
}
