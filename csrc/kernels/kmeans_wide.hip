// K-means assignment past one CU's LDS: 1 ≤ k ≤ 4096 centroids, 1 ≤ d ≤ 8192 features.
//
// The two kernels of dense_learners.hip keep every centroid and the k × d cluster sums in one
// workgroup's LDS and end near k·d ≈ 19 000. Here nothing lives in LDS for a whole launch but
// the tile being worked on; the results contract is that of omldm_kmeans_assign. Three passes,
// each in stream order, no float atomics to HBM anywhere:
//
// 1. Distances and arg-min (kmeans_wide_dist_kernel). A workgroup of four waves owns a 128-row
//    tile of x and walks the centroids in 128-centroid tiles and d in 32-column slabs. Both
//    slabs are staged in LDS (row stride 33 floats: the 32 lanes of an operand column on
//    distinct banks), double-buffered, the next slab's global loads in registers while the
//    MFMAs run on this one (the scheme of orr_gram.hip). Wave w computes the 64 × 64 quadrant
//    (centroids (w & 1)·64.., rows (w >> 1)·64..) as 2 × 2 accumulators of
//    v_mfma_f32_32x32x2_f32 (exact fp32 products): A = centroids, B = rows, so a lane ends a
//    centroid tile holding c·x of 2 × 16 centroids for each of its two rows. The score is
//    ‖c‖² − 2c·x (‖c‖² from a pre-pass, +inf for the padded centroids of the last tile; padded
//    columns are zero in both operands), folded in ascending centroid order into a running
//    (best, index) per row. After the last tile the half-waves combine by __shfl_xor and the two
//    waves of a row through LDS, smaller value first, then smaller index: exact ties go to the
//    lowest index. ‖x‖² is summed from the staged x slabs during the first centroid tile only.
//    The block writes assign[r] and, to its own workspace slot, Σ max(0, ‖x‖² + best) over its
//    training rows.
// 2. Cluster sums (kmeans_wide_sums_kernel). Grid = column slabs × row splits. A workgroup holds
//    [k][cs] fp32 sums (cs: the largest multiple of 8 with k·cs·4 ≤ 128 KiB, capped at d) and,
//    on slab 0, the k counts; it reads its rows' assign and y, its column slab of x coalesced,
//    adds with LDS atomics and stores its partial to its split's row of a partials image.
// 3. Fixed-order fold (kmeans_wide_fold_kernel, kmeans_wide_inertia_kernel): a thread per
//    column adds the splits' partials in index order into sums / counts; one wave adds the
//    inertia slots (lane l: slots l, l + 64, … in order, then the fixed wave tree) into inertia.
#include "common.h"

namespace omldm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKwMaxK = 4096, kKwMaxD = 8192;
constexpr int kKwTile = 128;             // rows of x and centroids per tile
constexpr int kKwSlab = 32;              // columns per staged slab
constexpr int kKwLd = kKwSlab + 1;       // odd LDS row stride
constexpr int kKwTF = kKwTile * kKwLd;   // floats of one staged slab
constexpr int kKwSumLds = 128 * 1024;    // bytes of [k][cs] in pass 2
constexpr int kKwSumBlocks = 512;        // pass 2 aims at two workgroups per CU
constexpr int kKwMinSplit = 256;         // rows of a split, at least

struct KwPlan {
  int kp;          // k rounded up to whole centroid tiles
  int nblk;        // 128-row tiles of x = workgroups of pass 1 = inertia slots
  int cs, nsl;     // pass 2: columns per slab, slabs
  int splits;      // pass 2: row splits (split i: rows [i·B/splits, (i + 1)·B/splits))
  long long pw;    // floats of one split's partial: k·d sums, k counts
  long long o_cn, o_in, o_as, o_part, words;  // workspace offsets and size, in 4-byte words
};

inline KwPlan kw_plan(int B, int d, int k) {
  KwPlan p;
  p.kp = (k + kKwTile - 1) / kKwTile * kKwTile;
  p.nblk = (int)(((long long)B + kKwTile - 1) / kKwTile);
  p.cs = (kKwSumLds / 4 / k) & ~7;  // ≥ 8 at k ≤ 4096
  if (p.cs > d) p.cs = d;
  p.nsl = (d + p.cs - 1) / p.cs;
  int s = kKwSumBlocks / p.nsl, smax = B / kKwMinSplit;
  if (s > smax) s = smax;
  p.splits = s < 1 ? 1 : s;
  p.pw = (long long)k * d + k;
  p.o_cn = 0;
  p.o_in = p.o_cn + p.kp;
  p.o_as = p.o_in + p.nblk;
  p.o_part = p.o_as + B;
  p.words = p.o_part + p.splits * p.pw;
  return p;
}

// cn[r] = ‖c_r‖² for r < k, +inf for k ≤ r < kp. One wave per centroid, four per block.
__global__ __launch_bounds__(256) void kmeans_wide_cnorm_kernel(const float* __restrict__ cent,
                                                                int k, int d, int kp,
                                                                float* __restrict__ cn) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (r >= kp) return;
  float a = 0.f;
  if (r < k)
    for (int c = lane; c < d; c += 64) {
      const float v = cent[(size_t)r * d + c];
      a = fmaf(v, v, a);
    }
  a = wave_sum(a);
  if (lane == 0) cn[r] = r < k ? a : INFINITY;
}

// grid ⌈B/128⌉, 256 threads, dynamic LDS 2 buffers × (x slab, centroid slab) = 4 · kKwTF floats
// (66 KiB). Two waves per SIMD: ≤ 256 registers, so that two workgroups share a CU's LDS.
__global__ __launch_bounds__(256, 2) void kmeans_wide_dist_kernel(
    const float* __restrict__ x, const float* __restrict__ yv, int B, int d, int k,
    const float* __restrict__ cent, const float* __restrict__ cn, int* __restrict__ assign,
    float* __restrict__ islot) {
  extern __shared__ __attribute__((aligned(16))) float stage[];  // [buf][x | centroids][128][33]
  __shared__ float rb[kKwTile];      // the centroid-half-1 waves' best per row
  __shared__ int ri[kKwTile];
  __shared__ float xxs[2 * kKwTile];  // ‖x‖² of the row's columns 0..15 and 16..31 of every slab
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, col = lane & 31;
  const long long row0 = (long long)blockIdx.x * kKwTile;
  const int nsl = (d + kKwSlab - 1) / kKwSlab, nct = (k + kKwTile - 1) / kKwTile;

  // ---- staging: this thread owns column lc of the slab and rows lr + 8·s of both tiles
  const int lc = tid & 31, lr = tid >> 5;
  float xr[16], cr[16];
  auto load = [&](int ct, int sl) {
    const int gc = sl * kKwSlab + lc;
    const int gcc = gc < d ? gc : 0;  // clamped: always in range, masked in store()
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const long long r = min(row0 + lr + 8 * s, (long long)B - 1);
      xr[s] = x[(size_t)r * d + gcc];
      const int c = min(ct * kKwTile + lr + 8 * s, k - 1);
      cr[s] = cent[(size_t)c * d + gcc];
    }
  };
  auto store = [&](int buf, int ct, int sl) {
    float* xb = stage + (size_t)buf * 2 * kKwTF;
    float* cb = xb + kKwTF;
    const bool cok = sl * kKwSlab + lc < d;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int r = lr + 8 * s;
      xb[r * kKwLd + lc] = cok ? xr[s] : 0.f;  // rows past B: copies of row B − 1, never written out
      cb[r * kKwLd + lc] = cok && ct * kKwTile + r < k ? cr[s] : 0.f;
    }
  };

  f32x16 acc[2][2];  // [centroid block i][row block j]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  float best[2] = {INFINITY, INFINITY};
  int bi[2] = {0, 0};
  float xx = 0.f;  // thread = (row tid & 127, column half tid >> 7) of the x slab

  load(0, 0);
  store(0, 0, 0);
  __syncthreads();
  int buf = 0;
  for (int ct = 0; ct < nct; ++ct) {
    for (int sl = 0; sl < nsl; ++sl) {
      const int nsl_ = sl + 1 < nsl ? sl + 1 : 0, nct_ = sl + 1 < nsl ? ct : ct + 1;
      const bool more = nct_ < nct;
      if (more) load(nct_, nsl_);  // in flight while this slab computes
      const float* xb = stage + (size_t)buf * 2 * kKwTF;
      const float* cb = xb + kKwTF;
      const float* xo = xb + (size_t)(wr * 64 + col) * kKwLd + half;
      const float* co = cb + (size_t)(wc * 64 + col) * kKwLd + half;
#pragma unroll
      for (int kp = 0; kp < kKwSlab / 2; ++kp) {
        const float a0 = co[2 * kp], a1 = co[32 * kKwLd + 2 * kp];
        const float b0 = xo[2 * kp], b1 = xo[32 * kKwLd + 2 * kp];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if (ct == 0) {  // 64 consecutive rows at stride 33: every lane on its own bank
        const float* xs = xb + (size_t)(tid & 127) * kKwLd + (tid >> 7) * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) xx = fmaf(xs[c], xs[c], xx);
      }
      if (more) store(buf ^ 1, nct_, nsl_);  // buf ^ 1 was last read before the previous barrier
      __syncthreads();
      buf ^= 1;
    }
    // C/D map (32x32): column (row of x) = lane & 31, row (centroid) = (q & 3) + 8·(q >> 2) +
    // 4·half: ascending in q, so a strict < keeps the lowest index among equal scores
    const int cbase = ct * kKwTile + wc * 64 + 4 * half;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ci = cbase + i * 32 + (q & 3) + 8 * (q >> 2);
        const float n2 = cn[ci];  // ci < kp; one address per half-wave
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float sc = fmaf(-2.f, acc[i][j][q], n2);
          if (sc < best[j]) {
            best[j] = sc;
            bi[j] = ci;
          }
          acc[i][j][q] = 0.f;
        }
      }
  }
  // the other half-wave holds the row's other 2 × 16 centroids of every tile
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float ob = __shfl_xor(best[j], 32);
    const int oi = __shfl_xor(bi[j], 32);
    if (ob < best[j] || (ob == best[j] && oi < bi[j])) {
      best[j] = ob;
      bi[j] = oi;
    }
  }
  xxs[tid] = xx;
  if (wc == 1 && half == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      rb[wr * 64 + j * 32 + col] = best[j];
      ri[wr * 64 + j * 32 + col] = bi[j];
    }
  }
  __syncthreads();
  float my_in = 0.f;
  if (wc == 0 && half == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int l = wr * 64 + j * 32 + col;
      const float ob = rb[l];
      const int oi = ri[l];
      if (ob < best[j] || (ob == best[j] && oi < bi[j])) {
        best[j] = ob;
        bi[j] = oi;
      }
      const long long row = row0 + l;
      if (row < B) {
        assign[row] = bi[j];
        const bool train = yv == nullptr || !__builtin_isnan(yv[row]);
        if (train) my_in += fmaxf(0.f, (xxs[l] + xxs[kKwTile + l]) + best[j]);  // ‖x − c‖² ≥ 0
      }
    }
  }
  const float w = wave_sum(my_in);
  if (lane == 0) part[wave] = w;
  __syncthreads();
  if (tid == 0) islot[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// grid (nsl, splits), 256 threads, dynamic LDS (k·cs + k) floats. tpr threads share a row (the
// smallest power of two ≥ the slab's columns, ≤ 256) and 256 / tpr rows are in flight, four
// deep: the loads of four rows are issued before their LDS atomics.
__global__ __launch_bounds__(256) void kmeans_wide_sums_kernel(
    const float* __restrict__ x, const float* __restrict__ yv, int B, int d, int k,
    const int* __restrict__ assign, int cs, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float acc[];  // [k][cs] sums, [k] counts
  float* s = acc;
  float* n = acc + (size_t)k * cs;
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * cs, cw = min(cs, d - c0);
  const long long r0 = (long long)blockIdx.y * B / gridDim.y;
  const long long r1 = (long long)(blockIdx.y + 1) * B / gridDim.y;
  for (int i = tid; i < k * cs + k; i += 256) acc[i] = 0.f;
  __syncthreads();
  int tpr = 1;
  while (tpr < cw && tpr < 256) tpr <<= 1;
  const int rp = 256 / tpr, sub = tid / tpr, c = tid & (tpr - 1);
  const bool cnt = blockIdx.x == 0 && c == 0;
  for (long long rbase = r0 + sub; rbase < r1; rbase += 4 * rp) {
    int a[4];
    bool ok[4];
    const float* xp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long r = rbase + (long long)u * rp;
      ok[u] = r < r1;
      const long long rr = ok[u] ? r : r1 - 1;  // clamped: always in range
      a[u] = min(max(assign[rr], 0), k - 1);
      if (yv) ok[u] = ok[u] && !__builtin_isnan(yv[rr]);
      xp[u] = x + (size_t)rr * d + c0;
    }
    for (int cc = c; cc < cw; cc += tpr) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = xp[u][cc];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) atomicAdd(&s[a[u] * cs + cc], v[u]);
    }
    if (cnt) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) atomicAdd(&n[a[u]], 1.f);
    }
  }
  __syncthreads();
  float* row = part + (size_t)blockIdx.y * ((size_t)k * d + k);
  for (int i = tid; i < k * cw; i += 256) {
    const int j = i / cw, f = i - j * cw;
    row[(size_t)j * d + c0 + f] = s[j * cs + f];
  }
  if (blockIdx.x == 0)
    for (int i = tid; i < k; i += 256) row[(size_t)k * d + i] = n[i];
}

// thread = one column of the partials image [splits][kd + k]: the splits in index order.
__global__ __launch_bounds__(256) void kmeans_wide_fold_kernel(const float* __restrict__ part,
                                                               int splits, long long kd,
                                                               long long pw,
                                                               float* __restrict__ sums,
                                                               float* __restrict__ counts) {
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= pw) return;
  float a = 0.f;
  for (int sp = 0; sp < splits; ++sp) a += part[(size_t)sp * pw + col];
  if (col < kd) sums[col] += a;
  else counts[col - kd] += a;
}

// one wave: lane l adds slots l, l + 64, … in order; the wave tree has a fixed order too.
__global__ __launch_bounds__(64) void kmeans_wide_inertia_kernel(const float* __restrict__ islot,
                                                                 int nslot,
                                                                 float* __restrict__ inertia) {
  float a = 0.f;
  for (int i = threadIdx.x; i < nslot; i += 64) a += islot[i];
  a = wave_sum(a);
  if (threadIdx.x == 0) *inertia += a;
}

}  // namespace omldm

using namespace omldm;

// 1 when omldm_kmeans_assign_wide takes d features and k centroids.
OMLDM_API int omldm_kmeans_wide_fits(int d, int k) {
  return d >= 1 && d <= kKwMaxD && k >= 1 && k <= kKwMaxK;
}

// Bytes of workspace omldm_kmeans_assign_wide needs (whichever outputs are asked for); −1
// outside the box or for B < 1.
OMLDM_API long long omldm_kmeans_wide_ws_bytes(int B, int d, int k) {
  if (B < 1 || !omldm_kmeans_wide_fits(d, k)) return -1;
  return kw_plan(B, d, k).words * 4;
}

// omldm_kmeans_assign for 1 ≤ k ≤ 4096, 1 ≤ d ≤ 8192: assign[r] (may be null) = a nearest
// centroid of row r, exact ties to the lowest index; sums[k][d] and counts[k] (both or neither)
// += the rows with a non-NaN y (all rows when y is null) and their number per cluster; inertia
// (may be null, with or without sums) += Σ ‖x − c‖² of those rows. `work`: 4-byte aligned,
// work_bytes ≥ omldm_kmeans_wide_ws_bytes(B, d, k); what it holds on entry does not matter. Up
// to five launches in stream order. Returns a HIP error code, −2 outside the box, −3 for bad
// arguments or a missing or short workspace; nothing is launched on a negative return.
OMLDM_API int omldm_kmeans_assign_wide(const float* x, const float* y, int B, int d, int k,
                                       const float* cent, float* sums, float* counts, int* assign,
                                       float* inertia, float* work, long long work_bytes,
                                       void* stream) {
  if (B <= 0) return 0;
  if (!omldm_kmeans_wide_fits(d, k)) return -2;
  const KwPlan p = kw_plan(B, d, k);
  if (!x || !cent || (sums != nullptr) != (counts != nullptr) || !work || ((uintptr_t)work & 3) ||
      work_bytes < p.words * 4)
    return -3;
  hipStream_t st = (hipStream_t)stream;
  float* cn = work + p.o_cn;
  float* islot = work + p.o_in;
  int* as = assign ? assign : reinterpret_cast<int*>(work + p.o_as);
  float* part = work + p.o_part;
  const size_t lds1 = (size_t)4 * kKwTF * 4;
  int e = check_dyn_lds((const void*)kmeans_wide_dist_kernel, lds1);
  if (e) return e;
  const size_t lds2 = ((size_t)k * p.cs + k) * 4;
  if (sums && (e = check_dyn_lds((const void*)kmeans_wide_sums_kernel, lds2))) return e;
  hipLaunchKernelGGL(kmeans_wide_cnorm_kernel, dim3(p.kp / 4), dim3(256), 0, st, cent, k, d, p.kp,
                     cn);
  hipLaunchKernelGGL(kmeans_wide_dist_kernel, dim3(p.nblk), dim3(256), lds1, st, x, y, B, d, k,
                     cent, cn, as, islot);
  if (sums) {
    hipLaunchKernelGGL(kmeans_wide_sums_kernel, dim3(p.nsl, p.splits), dim3(256), lds2, st, x, y,
                       B, d, k, as, p.cs, part);
    hipLaunchKernelGGL(kmeans_wide_fold_kernel, dim3((unsigned)((p.pw + 255) / 256)), dim3(256), 0,
                       st, part, p.splits, (long long)k * d, p.pw, sums, counts);
  }
  if (inertia)
    hipLaunchKernelGGL(kmeans_wide_inertia_kernel, dim3(1), dim3(64), 0, st, islot, p.nblk,
                       inertia);
  return (int)hipGetLastError();
}
