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
    // ---- 1. diagonal block, wave 0: lane i (mod 16) owns row i. Entries on and right of the
    // diagonal are carried along unmasked: they never feed an entry left of it, and nothing
    // reads them back from LDS (every later step divides by the pivot through invd)
    if (wave == 0) {
      double* row = A + (c0 + (lane & 15)) * S + c0;
      double a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = row[k];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double djj = readlane_d(a[j], j);
        bad |= !(djj > 0.0);
        const double inv = 1.0 / sqrt(djj);
        if (lane == 0) invd[c0 + j] = inv;
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
    __syncthreads();

    // ---- 2. rows below the block, then the b row: x·L11ᵀ = a, one row per lane
    {
      const int R = NP - c0 - 15;  // NP − c0 − 16 rows of A, and the b row
      const int q = lane * kOrrWaves + wave;
      if (q < R) {
        double* row = A + (q == R - 1 ? NP : c0 + 16 + q) * S + c0;
        const double* L11 = A + c0 * S + c0;
        double x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = row[k];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          x[j] *= invd[c0 + j];
#pragma unroll
          for (int k = j + 1; k < 16; ++k) x[k] -= x[j] * L11[k * S + j];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = x[k];
      }
    }
    __syncthreads();
    if (p == TC - 1) break;  // nothing trails the last panel

    // ---- 3. trailing update on the fp64 MFMA. A operand: lane (i = l % 16, k = l / 16) holds
    // −L[16·ti + i][c0 + 4s + k]; B operand: L[16·tj + i][c0 + 4s + k]; accumulator register v of
    // lane l is C[4v + l / 16][l % 16].
    {
      const int li = lane & 15, lk = lane >> 4;
      int t = 0;
      for (int ti = p + 1; ti <= TC; ++ti) {
        const int tjmax = ti < TC ? ti : TC - 1;  // tile row TC (the b row) has no diagonal tile
        for (int tj = p + 1; tj <= tjmax; ++tj, ++t) {
          if ((t & (kOrrWaves - 1)) != wave) continue;
          const double* La = A + (ti * 16 + li) * S + c0 + lk;
          const double* Lb = A + (tj * 16 + li) * S + c0 + lk;
          double* C = A + (ti * 16 + lk) * S + tj * 16 + li;
          d4_t acc;
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[v] = C[4 * v * S];
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-La[4 * s], Lb[4 * s], acc, 0, 0, 0);
#pragma unroll
          for (int v = 0; v < 4; ++v) C[4 * v * S] = acc[v];
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
      double yk = y[c0 + k];
      const double ik = invd[c0 + k];
#pragma unroll
      for (int i = 15; i >= 0; --i) {
        const double wi = readlane_d(yk * ik, i);
        if (lane == 0) y[c0 + i] = wi;
        yk -= Lc[i] * wi;  // lanes k ≥ i are done: what this leaves in them is not read again
      }
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
