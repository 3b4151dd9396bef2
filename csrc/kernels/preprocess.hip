// Streaming preprocessors on the dense feature block of a micro-batch:
// StandardScaler (running moments, Chan merge), MinMaxScaler (running extrema),
// PolynomialFeatures (monomial expansion). Reference: the three preprocessor names the
// request validator accepts (omldm/utils/parsers/requestStream/PipelineMap.scala:67).
//
// x is row-major [B, d] (d ≤ a few hundred, B up to ~10^6). Column moments are taken in a
// single pass on 256-thread blocks that each own a slab of rows and accumulate per-column
// partials in LDS, then one block per column merges the slab partials into the running f64
// state — no host round trip, no same-address global atomics.
//
// The shift of the pass comes from the batch itself: every block subtracts its own first
// row (z = x − x[r0], exact in f64) and sums z and z² in f64 (ds_add_f64), so a column whose
// mean is large against its spread does not cancel, on the first batch (running mean 0) as
// on any other. The merge re-bases every block's sums to the batch's first row x[0] — it
// reads the very fp32 values the blocks subtracted — and forms M2 = S2 − S1²/B. The shift is
// a data point, so S2 ≤ (B + 1)·M2: the subtraction loses at most log2(B + 1) of f64's 53
// bits (a constant column gives z = 0 and M2 = 0 exactly).
//
// Contract: finite features in training rows (as for k-means). A NaN or ±inf feature
// poisons its column's mean and M2 (as on the CPU path); a NaN is skipped by the extrema
// here (integer keys, fminf / fmaxf) where the CPU path propagates it.
#include "common.h"

namespace omldm {

constexpr int kPPThreads = 256;
constexpr int kPPPartialBytes = 24;  // per (block, column): f64 Σz, f64 Σz², f32 min, f32 max

// A block's partials: [d] f64 Σz, [d] f64 Σz², [d] f32 min, [d] f32 max.
struct PPPartial {
  double* s1;
  double* s2;
  float* mn;
  float* mx;
};

__device__ inline PPPartial pp_partial(void* partial, int blk, int d) {
  PPPartial p;
  p.s1 = reinterpret_cast<double*>(static_cast<unsigned char*>(partial) +
                                   (size_t)blk * d * kPPPartialBytes);
  p.s2 = p.s1 + d;
  p.mn = reinterpret_cast<float*>(p.s2 + d);
  p.mx = p.mn + d;
  return p;
}

// Order-preserving int key of a float (−inf < … < −0.0 < +0.0 < … < +inf) and its inverse:
// extrema are taken on the keys, so ±0.0 and denormals come out bit-exact.
__device__ inline int pp_key(float v) {
  const int iv = __float_as_int(v);
  return iv >= 0 ? iv : (iv ^ 0x7fffffff);
}
__device__ inline float pp_unkey(int k) { return __int_as_float(k >= 0 ? k : (k ^ 0x7fffffff)); }

// The block's rows [r0, r1): Σ(x − x[r0]), Σ(x − x[r0])² (mode bit0), min, max per column.
__global__ __launch_bounds__(kPPThreads) void colmoments_kernel(
    const float* __restrict__ x, int B, int d, int rows_per_block, int mode,
    void* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* s1 = reinterpret_cast<double*>(smem);
  double* s2 = s1 + d;
  int* mn = reinterpret_cast<int*>(s2 + d);  // pp_key of the extrema
  int* mx = mn + d;
  for (int c = threadIdx.x; c < d; c += kPPThreads) {
    s1[c] = 0.0;
    s2[c] = 0.0;
    mn[c] = 0x7fffffff;
    mx[c] = (int)0x80000000;
  }
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min((long long)B, r0 + rows_per_block);
  const long long n = (r1 - r0) * d;
  const float* base = x + r0 * d;
  const bool moments = mode & 1;
  for (long long e = threadIdx.x; e < n; e += kPPThreads) {
    const int c = (int)(e % d);
    const float v = base[e];
    if (moments) {
      const double z = (double)v - (double)base[c];  // shift = the block's first row
      atomicAdd(&s1[c], z);
      atomicAdd(&s2[c], z * z);
    }
    const int key = pp_key(v);
    atomicMin(&mn[c], key);
    atomicMax(&mx[c], key);
  }
  __syncthreads();
  const PPPartial o = pp_partial(partial, blockIdx.x, d);
  for (int c = threadIdx.x; c < d; c += kPPThreads) {
    o.s1[c] = s1[c];
    o.s2[c] = s2[c];
    o.mn[c] = pp_unkey(mn[c]);
    o.mx[c] = pp_unkey(mx[c]);
  }
}

// One block per column: re-base the slab partials to the batch's first row and reduce them,
// then merge into the running state. mode bit0: update mean/M2 (Chan), bit1: update min/max.
__global__ __launch_bounds__(kPPThreads) void colmoments_merge_kernel(
    const float* __restrict__ x, void* __restrict__ partial, int nblk, int d, int B,
    int rows_per_block, double count, double* __restrict__ mean, double* __restrict__ m2,
    float* __restrict__ lo, float* __restrict__ hi, int mode) {
  __shared__ double r1[kPPThreads], r2[kPPThreads];
  __shared__ int rmn[kPPThreads], rmx[kPPThreads];
  const int c = blockIdx.x;
  const double sh0 = (double)x[c];
  double a1 = 0.0, a2 = 0.0;
  int amn = 0x7fffffff, amx = (int)0x80000000;
  for (int b = threadIdx.x; b < nblk; b += kPPThreads) {
    const PPPartial o = pp_partial(partial, b, d);
    if (mode & 1) {
      // Σ(x − sh0) and Σ(x − sh0)² from the block's sums about its own first row
      const long long row = (long long)b * rows_per_block;
      const double nb = (double)(min((long long)B, row + rows_per_block) - row);
      const double dl = (double)x[row * d + c] - sh0;
      const double b1 = o.s1[c], b2 = o.s2[c];
      a1 += b1 + nb * dl;
      a2 += b2 + dl * (2.0 * b1 + nb * dl);
    }
    amn = min(amn, pp_key(o.mn[c]));
    amx = max(amx, pp_key(o.mx[c]));
  }
  r1[threadIdx.x] = a1;
  r2[threadIdx.x] = a2;
  rmn[threadIdx.x] = amn;
  rmx[threadIdx.x] = amx;
  __syncthreads();
  for (int s = kPPThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      r1[threadIdx.x] += r1[threadIdx.x + s];
      r2[threadIdx.x] += r2[threadIdx.x + s];
      rmn[threadIdx.x] = min(rmn[threadIdx.x], rmn[threadIdx.x + s]);
      rmx[threadIdx.x] = max(rmx[threadIdx.x], rmx[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && B > 0) {
    if (mode & 1) {
      const double nb = (double)B;
      const double mb = sh0 + r1[0] / nb;
      double m2b = r2[0] - r1[0] * r1[0] / nb;
      if (m2b < 0.0) m2b = 0.0;
      const double tot = count + nb;
      const double delta = mb - mean[c];
      mean[c] += delta * nb / tot;
      m2[c] += m2b + delta * delta * count * nb / tot;
    }
    if (mode & 2) {
      lo[c] = pp_unkey(min(pp_key(lo[c]), rmn[0]));
      hi[c] = pp_unkey(max(pp_key(hi[c]), rmx[0]));
    }
  }
}

// y = (x − μ)/σ (σ = sqrt(M2/N), 1 where 0) or (x − lo)/(hi − lo) (range 0 → 0).
__global__ __launch_bounds__(kPPThreads) void scale_kernel(
    const float* __restrict__ x, float* __restrict__ y, long long n, int d, int mode,
    const double* __restrict__ mean, const double* __restrict__ m2, double count,
    const float* __restrict__ lo, const float* __restrict__ hi) {
  for (long long e = (long long)blockIdx.x * kPPThreads + threadIdx.x; e < n;
       e += (long long)gridDim.x * kPPThreads) {
    const int c = (int)(e % d);
    const float v = x[e];
    float r;
    if (mode == 0) {
      const double var = count > 0.0 ? m2[c] / count : 0.0;
      const float sd = var > 0.0 ? (float)sqrt(var) : 1.f;
      r = (v - (float)mean[c]) / sd;
    } else {
      const float rg = hi[c] - lo[c];
      r = rg > 0.f ? (v - lo[c]) / rg : 0.f;
    }
    y[e] = r;
  }
}

// out[b] = [x[b, 0:d], Π_k x[b, idx[r][k]] for r in combos] ; idx −1 = no factor.
__global__ __launch_bounds__(kPPThreads) void poly_kernel(const float* __restrict__ x, int B, int d,
                                                          const int* __restrict__ idx, int ncomb,
                                                          int deg, float* __restrict__ out) {
  const int dout = d + ncomb;
  const long long n = (long long)B * dout;
  for (long long e = (long long)blockIdx.x * kPPThreads + threadIdx.x; e < n;
       e += (long long)gridDim.x * kPPThreads) {
    const long long b = e / dout;
    const int j = (int)(e - b * dout);
    const float* xr = x + b * d;
    float v;
    if (j < d) {
      v = xr[j];
    } else {
      const int* ir = idx + (size_t)(j - d) * deg;
      v = 1.f;
      for (int k = 0; k < deg; ++k)
        if (ir[k] >= 0) v *= xr[ir[k]];
    }
    out[e] = v;
  }
}

}  // namespace omldm

using namespace omldm;

static int grid_for(long long n) {
  long long g = (n + kPPThreads - 1) / kPPThreads;
  if (g > 4096) g = 4096;
  return g < 1 ? 1 : (int)g;
}

// Updates the running state with x [B, d]; mode bit0 moments, bit1 extrema.
// partial must hold ceil(B / rows_per_block) * d * 24 bytes, 8-byte aligned.
OMLDM_API int omldm_colstats_update(const float* x, int B, int d, double count, double* mean,
                                    double* m2, float* lo, float* hi, int mode, float* partial,
                                    int rows_per_block, void* stream) {
  if (B <= 0) return 0;
  if (((mode & 1) && (!mean || !m2)) || ((mode & 2) && (!lo || !hi)) || !partial) return -4;
  if (d <= 0 || rows_per_block <= 0 || ((uintptr_t)partial & 7)) return -4;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (B + rows_per_block - 1) / rows_per_block;
  const size_t lds = (size_t)d * kPPPartialBytes;
  if (lds > 160 * 1024) return -1;
  int e = check_dyn_lds((const void*)colmoments_kernel, lds);
  if (e) return e;
  hipLaunchKernelGGL(colmoments_kernel, dim3(nblk), dim3(kPPThreads), lds, st, x, B, d,
                     rows_per_block, mode, (void*)partial);
  hipLaunchKernelGGL(colmoments_merge_kernel, dim3(d), dim3(kPPThreads), 0, st, x,
                     (void*)partial, nblk, d, B, rows_per_block, count, mean, m2, lo, hi, mode);
  return (int)hipGetLastError();
}

OMLDM_API int omldm_scale(const float* x, float* y, int B, int d, int mode, const double* mean,
                          const double* m2, double count, const float* lo, const float* hi,
                          void* stream) {
  const long long n = (long long)B * d;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(kPPThreads), 0, (hipStream_t)stream,
                     x, y, n, d, mode, mean, m2, count, lo, hi);
  return (int)hipGetLastError();
}

OMLDM_API int omldm_poly(const float* x, int B, int d, const int* idx, int ncomb, int deg,
                         float* out, void* stream) {
  const long long n = (long long)B * (d + ncomb);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(poly_kernel, dim3(grid_for(n)), dim3(kPPThreads), 0, (hipStream_t)stream, x,
                     B, d, idx, ncomb, deg, out);
  return (int)hipGetLastError();
}
