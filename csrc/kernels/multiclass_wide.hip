// Wide MultiClassPA round on hashed batches: one Synchronous round of S virtual spokes with
// the semantics of omldm_cpu_multiclass_round (csrc/host/linear_cpu.cpp) for 2 ≤ K ≤ 256
// classes and 1 ≤ F = dn + dc + bias ≤ 256 features per row — the shapes past the v3 scan
// (K ≤ 16) and the spoke tables (K ≤ 16, F ≤ 64).
//
//  * One workgroup of two waves per spoke; no workgroup waits for another. The spoke's
//    private delta lives in HBM: an open-addressing table keyed by hashed key with kp =
//    class_pad(K) floats per entry (the Spill layout of spoke_table.h: keys | vals[kp] |
//    list | count). Every key of a row goes through it, numerical columns and the intercept
//    included; the launcher refuses a table that cannot hold the spoke's worst case.
//  * Wave 1, the loader, prepares chunk c + 1 while wave 0 runs chunk c (one barrier per
//    chunk): it decodes the rows, compacts a row's present features (the oracle's column
//    order), resolves every key to its table entry by find-or-insert (only this wave
//    inserts; every probe loop is bounded by the table size), flags the later occurrences of
//    an entry within a row, computes ‖x‖² in the oracle's order, τ's denominator and cap, and
//    accumulates the round-start scores base[i][k] = Σ_f x_if · Wt[key_if][k] into LDS.
//  * Wave 0, lane = class (⌈K/64⌉ classes per lane), per row: score[k] = base[i][k] +
//    Σ_f x_f · d[entry_f][k] with one coalesced read of an entry's deltas across the class
//    lanes and 16 to 32 reads in flight, one wave arg-max over the classes other than y (the lowest
//    class among equals), the wave-uniform step math in the oracle's operation order
//    (contraction off, IEEE division), and, when τ ≠ 0, d[entry_f][y] += τ·x_f and
//    d[entry_f][r] −= τ·x_f with lane = feature. A later occurrence of an entry in the row
//    (wide wire at a small dim) acts after the first, one at a time in column order, so a key
//    that occurs twice acts twice as in the oracle. The deltas are read and written with
//    agent-scope accesses and a row's updates are drained (vmcnt(0)) before the next row
//    reads them.
//  * Round end: one small fold launch per spoke, in spoke order on the stream, adds the
//    spoke's listed entries into dacc[k][key] (k < K; a spoke's keys are distinct: plain
//    read-add-write, no float atomics) and restores them (key empty, values 0); a last
//    launch sums the per-spoke statistics rows in spoke order and clears the counters. The
//    same inputs give the same bits, and the table is clean for the next round.
#include "spoke_table.h"

#pragma clang fp contract(off)

namespace omldm {
namespace {

constexpr int kMcwMaxK = 256;
constexpr int kMcwMaxF = 256;
constexpr int kMcwStat = 8;            // workspace row: loss, rows, mistakes, 1, -, overflow, -, -
constexpr int kMcwLds = 128 * 1024;
constexpr int kMcwDup = 1 << 30;       // flag on a staged entry: a later occurrence in its row
constexpr int kMcwDupLog2 = 9;         // per-row occurrence table: 512 ≥ 2·F slots
constexpr int kMcwMaxLog2 = 24;        // entries per spoke (log2) the launcher takes
// delta reads in flight per lane and class slot: 16 up to 64 classes (32 measured
// no faster there: a row of 40 features pads to 64 reads), 32 / ⌈K/64⌉ above
inline constexpr int mcw_step(int CW) { return CW == 1 ? 16 : 32 / CW; }

struct McwGeom {
  int CR;     // rows per chunk
  int FS;     // words of a staged row: F rounded up to the read step, + 1 (odd)
  int nodup;  // no entry can occur twice in a row (field-aware slots apart from the intercept)
};

inline int mcw_cw(int K) { return K <= 64 ? 1 : K <= 128 ? 2 : 4; }

inline size_t mcw_lds_bytes(int CR, int FS, int K) {
  const size_t KL = 64 * (size_t)mcw_cw(K);
  return ((size_t)2 * CR * (2 * FS + KL) + (size_t)CR * FS + 2 * (1 << kMcwDupLog2) + 8 * 64) *
         sizeof(float);
}

// Worst-case distinct keys of a spoke of R rows, and the smallest table (log2 entries) at
// load ≤ 1/2 — ops/dense.py multiclass_wide_table_log2 asks this function.
inline int mcw_table_log2(int dn, int dc, int bias, int R, int cspan, int dim) {
  long long range = cspan > 0 ? (long long)dc * cspan : (long long)dim - dn - 1;
  if (range < 0) range = 0;
  long long cat = (long long)R * dc;
  if (cat > range) cat = range;
  const long long distinct = (long long)dn + (bias ? 1 : 0) + cat;
  int lg = 0;
  while (((long long)1 << lg) < 2 * distinct) ++lg;
  return lg;
}

inline bool mcw_shape_fits(int dn, int dc, int bias, int K) {
  const long long F = (long long)dn + dc + (bias ? 1 : 0);
  return dn >= 0 && dc >= 0 && F >= 1 && F <= kMcwMaxF && K >= 2 && K <= kMcwMaxK;
}

inline bool mcw_fits(int dn, int dc, int bias, int K, int R, int cspan, int dim, int log2gcap) {
  if (!mcw_shape_fits(dn, dc, bias, K) || R < 1 || dim < 1 || cspan < 0) return false;
  const int need = mcw_table_log2(dn, dc, bias, R, cspan, dim);
  return need >= 1 && log2gcap >= need && log2gcap <= kMcwMaxLog2;
}

// Orders one wave's LDS accesses (see multiclass_dense.hip).
__device__ __forceinline__ void mcw_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Entry of `key` in the spoke's table (find or insert, spill_find_or_insert's probe order and
// list; inlined, its arguments in registers): −1 only when all 2^lg entries are taken.
__device__ __forceinline__ int mcw_find_or_insert(int* keys, int* list, int* count, int lg,
                                                  int key) {
  const int gcap = 1 << lg;
  uint32_t i = hmix((uint32_t)key) >> (32 - lg);
  for (int q = 0; q < gcap; ++q) {
    const int k = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return (int)i;
    if (k == kEmptyKey) {
      const int prev = atomicCAS(&keys[i], kEmptyKey, key);
      if (prev == kEmptyKey) {
        const int at = atomicAdd(count, 1);
        if (at < gcap) list[at] = (int)i;
        return (int)i;
      }
      if (prev == key) return (int)i;
    }
    i = (i + 1) & (uint32_t)(gcap - 1);
  }
  return -1;
}

__device__ __forceinline__ void mcw_store(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int CW, typename NumT>
__global__ __launch_bounds__(128) void mcw_round_kernel(
    const float* __restrict__ Wt, int kp, const NumT* __restrict__ num, int dn,
    const void* __restrict__ cat, int dc, int cspan, const void* __restrict__ yv, int y_i8, int B,
    int R, int dim, int K, int variant, float C, int bias, float* __restrict__ ws, Spill sp,
    McwGeom geo) {
  extern __shared__ __attribute__((aligned(16))) float mcw_smem[];
  constexpr int KL = 64 * CW;
  constexpr int U = mcw_step(CW);
  constexpr int UB = 64 / CW;
  constexpr int NT = 1 << kMcwDupLog2;
  const int CR = geo.CR, FS = geo.FS;
  int* entL = reinterpret_cast<int*>(mcw_smem);   // [2][CR][FS]
  float* xsL = mcw_smem + (size_t)2 * CR * FS;    // [2][CR][FS]
  float* baseL = xsL + (size_t)2 * CR * FS;       // [2][CR][KL]
  int* keyL = reinterpret_cast<int*>(baseL + (size_t)2 * CR * KL);  // [CR][FS], loader only
  int* tk = keyL + (size_t)CR * FS;               // [NT] entries of the row (loader only)
  int* tf = tk + NT;                              // [NT] their first column
  int* nfL = tf + NT;                             // [2][64] present features of a row
  int* ycL = nfL + 128;                           // [2][64] class, −1 out of range, −2 skipped
  float* denL = reinterpret_cast<float*>(ycL + 128);  // [2][64]
  float* capL = denL + 128;                       // [2][64]
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long a = (long long)s * R;
  if (a >= B) return;  // an idle spoke is no worker of the round (the grid has none)
  const long long b = a + R < (long long)B ? a + R : (long long)B;
  const int nrows = (int)(b - a);
  const int F = dn + dc + (bias ? 1 : 0);
  const float inf = __builtin_inff();
  const size_t gcap = (size_t)1 << sp.log2gcap;
  float* vals = sp.vals + (size_t)s * gcap * kp;
  int* tkeys = sp.keys + (size_t)s * gcap;
  int* tlist = sp.list + (size_t)s * gcap;
  const int nchunks = (nrows + CR - 1) / CR;
  int kc[CW], kl[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    kc[c] = lane + 64 * c;
    kl[c] = kc[c] < kp ? kc[c] : kp - 1;  // a lane past the entry reads its last (padded) class
  }
  float ovf = 0.f;

  // wave 1: chunk ch into its staging buffer
  auto produce = [&](int ch) {
    const int buf = ch & 1;
    const long long t0 = a + (long long)ch * CR;
    const int nr = b - t0 < CR ? (int)(b - t0) : CR;
    int* eb = entL + (size_t)buf * CR * FS;
    float* xb = xsL + (size_t)buf * CR * FS;
    float* bb = baseL + (size_t)buf * CR * KL;
    // the rows' present features in column order, each key resolved to its table entry
    // (the first 64 columns of the next row are read while this row's keys are resolved)
    FeatRaw ahead = load_feature_raw(num, dn, cat, dc, (int)t0, lane, cspan);
    for (int r = 0; r < nr; ++r) {
      const int t = (int)(t0 + r);
      const FeatRaw first = ahead;
      ahead = load_feature_raw(num, dn, cat, dc, r + 1 < nr ? t + 1 : t, lane, cspan);
      int off = 0;
      for (int j0 = 0; j0 < F; j0 += 64) {
        const int j = j0 + lane;
        const FeatRaw raw = j0 == 0 ? first : load_feature_raw(num, dn, cat, dc, t, j, cspan);
        int idx;
        float v;
        decode_feature(raw, dn, dc, j, dim, bias, cspan, true, idx, v);
        int gi = 0;
        if (idx >= 0) {
          gi = mcw_find_or_insert(tkeys, tlist, sp.count + s, sp.log2gcap, idx);
          if (gi < 0) {  // never: the launcher sized the table for the worst case
            ovf += 1.f;
            gi = 0;
            v = 0.f;
          }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(idx >= 0);
        const int pos = off + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (idx >= 0) {
          keyL[r * FS + pos] = idx;
          eb[r * FS + pos] = gi;
          xb[r * FS + pos] = v;
        }
        off += __builtin_popcountll(m);
      }
      // pad to the read step: entry 0 and key 0 with x = 0 add nothing
      if (lane < U && off + lane < FS) {
        keyL[r * FS + off + lane] = 0;
        eb[r * FS + off + lane] = 0;
        xb[r * FS + off + lane] = 0.f;
      }
      if (lane == 0) nfL[buf * 64 + r] = off;
    }
    mcw_lds_sync();
    // later occurrences of an entry within a row: the first column of every entry of the
    // row through a small LDS table, every other column flagged
    if (!geo.nodup) {
      for (int r = 0; r < nr; ++r) {
        const int nf = nfL[buf * 64 + r];
        for (int i = lane; i < NT; i += 64) {
          tk[i] = kEmptyKey;
          tf[i] = 0x7fffffff;
        }
        mcw_lds_sync();
        int sl[kMcwMaxF / 64];
#pragma unroll
        for (int q = 0; q < kMcwMaxF / 64; ++q) {
          const int j = q * 64 + lane;
          sl[q] = -1;
          if (j < nf) {
            sl[q] = lds_find_or_insert(tk, eb[r * FS + j], kMcwDupLog2);
            if (sl[q] >= 0) atomicMin(&tf[sl[q]], j);
          }
        }
        mcw_lds_sync();
#pragma unroll
        for (int q = 0; q < kMcwMaxF / 64; ++q) {
          const int j = q * 64 + lane;
          if (j < nf && (sl[q] < 0 || tf[sl[q]] != j)) eb[r * FS + j] |= kMcwDup;
        }
        mcw_lds_sync();
      }
    }
    // lane i, row i: the label, ‖x‖² in the oracle's column order, τ's denominator and cap
    {
      const bool in = lane < nr;
      const long long t = in ? t0 + lane : b - 1;
      const float yl = load_label(yv, (int)t, y_i8);
      const bool skip = !in || yl != yl;
      float pn = 0.f;
      if (in) {
        const int nf = nfL[buf * 64 + lane];
        for (int j = 0; j < nf; ++j) {
          const float x = xb[lane * FS + j];
          pn += x * x;
        }
      }
      float cap = 0.f, den = 1.f;
      if (!skip && pn > 0.f) {
        den = 2.f * pn;
        if (variant == 2) den = den + 0.5f / C;
        cap = variant == 1 ? C : inf;
      }
      int yc = -2;
      if (!skip) yc = (yl > -1.f && yl < (float)K) ? (int)yl : -1;
      denL[buf * 64 + lane] = den;
      capL[buf * 64 + lane] = cap;
      ycL[buf * 64 + lane] = yc;
    }
    mcw_lds_sync();
    // the round-start scores of the labelled rows, lane = class
    for (int r = 0; r < nr; ++r) {
      if (ycL[buf * 64 + r] == -2) continue;
      const int nf = nfL[buf * 64 + r];
      float acc[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) acc[c] = 0.f;
      // up to 64 prototype reads per lane in flight: a row of ≤ 64 / CW features is one round
      // trip (these mostly miss the L2); a column past nf re-reads the last key with x = 0
      for (int j = 0; j < nf; j += UB) {
        float wv[UB][CW];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int jj = j + u < nf ? j + u : nf - 1;
          const float* p = Wt + (size_t)keyL[r * FS + jj] * kp;
#pragma unroll
          for (int c = 0; c < CW; ++c) wv[u][c] = p[kl[c]];
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int jj = j + u < nf ? j + u : nf - 1;
          const float x = j + u < nf ? xb[r * FS + jj] : 0.f;
#pragma unroll
          for (int c = 0; c < CW; ++c) acc[c] = __builtin_fmaf(x, wv[u][c], acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < CW; ++c) bb[r * KL + kc[c]] = acc[c];
    }
  };

  float loss_l = 0.f, nex_l = 0.f, mist_l = 0.f;  // per-lane sums (wave 0)

  // wave 0: the rows of chunk ch, in order
  auto consume = [&](int ch) {
    const int buf = ch & 1;
    const int nr = nrows - ch * CR < CR ? nrows - ch * CR : CR;
    const int* eb = entL + (size_t)buf * CR * FS;
    const float* xb = xsL + (size_t)buf * CR * FS;
    const float* bb = baseL + (size_t)buf * CR * KL;
    float mpark = 0.f;  // lane i: the margin of row i
    const int ycv = ycL[buf * 64 + lane], nfv = nfL[buf * 64 + lane];
    const float denv = denL[buf * 64 + lane], capv = capL[buf * 64 + lane];
    for (int r = 0; r < nr; ++r) {
      const int yc = __builtin_amdgcn_readlane(ycv, r);
      if (yc == -2) continue;  // unlabelled row (wave-uniform)
      const int nf = __builtin_amdgcn_readlane(nfv, r);
      const float den = readlane_f(denv, r), cap = readlane_f(capv, r);
      const int* er = eb + r * FS;
      const float* xr = xb + r * FS;
      float sc[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) sc[c] = bb[r * KL + kc[c]];
      for (int j = 0; j < nf; j += U) {
        float xv[U], dv[U][CW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          xv[u] = xr[j + u];
          const float* p = vals + (size_t)(er[j + u] & ~kMcwDup) * kp;
#pragma unroll
          for (int c = 0; c < CW; ++c) dv[u][c] = spill_load(p + kl[c]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int c = 0; c < CW; ++c) sc[c] = __builtin_fmaf(xv[u], dv[u][c], sc[c]);
      }
      float bv = -inf;
      int bk = 0;
#pragma unroll
      for (int c = 0; c < CW; ++c)
        if (kc[c] < K && kc[c] != yc && sc[c] > bv) {
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
      for (int c = 1; c < CW; ++c)
        if ((yc >> 6) == c) syv = sc[c];
      const float sy = yc >= 0 ? readlane_f(syv, yc & 63) : 0.f;
      const float margin = sy - m;
      const float loss = fmaxf(0.f, 1.f - margin);
      float tau = fminf(cap, loss / den);
      if (!any) tau = 0.f;
      mpark = lane == r ? margin : mpark;
      if (tau != 0.f) {  // wave-uniform
        for (int j0 = 0; j0 < nf; j0 += 64) {
          const int j = j0 + lane;
          const int ew = j < nf ? er[j] : 0;
          const float u = j < nf ? tau * xr[j] : 0.f;
          float* p = vals + (size_t)(ew & ~kMcwDup) * kp;
          float* py = p + (yc >= 0 ? yc : rr);
          const bool dup = (ew & kMcwDup) != 0;
          if (j < nf && !dup) {  // distinct entries: a plain read-add-write per lane
            const float vy = spill_load(py), vr = spill_load(p + rr);
            if (yc >= 0) mcw_store(py, vy + u);
            mcw_store(p + rr, vr - u);
          }
          unsigned long long dm = __builtin_amdgcn_ballot_w64(dup);
          while (dm) {  // later occurrences, one at a time in column order
            const int bl = __builtin_ctzll(dm);
            dm &= dm - 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == bl) {
              const float vy = spill_load(py), vr = spill_load(p + rr);
              if (yc >= 0) mcw_store(py, vy + u);
              mcw_store(p + rr, vr - u);
            }
          }
        }
        // the next row's reads of d observe these writes
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
  float* wrow = ws + (size_t)s * kMcwStat;
  if (wave == 1) {
    const float o = wave_sum(ovf);
    if (lane == 0) wrow[5] = o;
    return;
  }
  const float loss_sum = wave_sum(loss_l), nex = wave_sum(nex_l), mist = wave_sum(mist_l);
  if (lane == 0) {
    wrow[0] = loss_sum;
    wrow[1] = nex;
    wrow[2] = mist;
    wrow[3] = 1.f;  // a spoke with rows, labelled or not
  }
}

// Spoke s's listed entries into dacc[k][key], k < K, and back to empty. 256 / kp whole
// entries per block step, thread = (entry, class): an entry's threads share a block, so the
// key is cleared after all of them have read it.
__global__ __launch_bounds__(256) void mcw_fold_kernel(Spill sp, int s, int kp, int K, int dim,
                                                       float* __restrict__ dacc) {
  const size_t gcap = (size_t)1 << sp.log2gcap;
  int* keys = sp.keys + (size_t)s * gcap;
  int* list = sp.list + (size_t)s * gcap;
  float* vals = sp.vals + (size_t)s * gcap * kp;
  const int n = sp.count[s];
  const int epb = 256 / kp;
  const int e = (int)threadIdx.x / kp, k = (int)threadIdx.x - e * kp;
  for (long long j0 = (long long)blockIdx.x * epb; j0 < n; j0 += (long long)gridDim.x * epb) {
    const long long j = j0 + e;
    const bool ok = e < epb && j < n;
    int gi = 0, key = -1;
    if (ok) {
      gi = list[j];
      key = ((size_t)gi < gcap) ? keys[gi] : -1;
    }
    if (ok && (size_t)gi < gcap) {
      float* v = vals + (size_t)gi * kp + k;
      const float x = *v;
      if (k < K && x != 0.f && (unsigned)key < (unsigned)dim) dacc[(size_t)k * dim + key] += x;
      *v = 0.f;
    }
    __syncthreads();
    if (ok && k == 0) {
      if ((size_t)gi < gcap) keys[gi] = kEmptyKey;
      list[j] = 0;
    }
  }
}

// The spokes' statistics rows in spoke order into stats[0..3] and stats[5]; the tables'
// counters back to 0 (after every fold has read them).
__global__ __launch_bounds__(64) void mcw_finish_kernel(const float* __restrict__ ws, int S_act,
                                                        Spill sp, float* __restrict__ stats) {
  const int c = threadIdx.x;
  if (c < 4 || c == 5) {
    float t = stats[c];
    for (int s = 0; s < S_act; ++s) t += ws[(size_t)s * kMcwStat + c];
    stats[c] = t;
  }
  for (int s = c; s < S_act; s += 64) sp.count[s] = 0;
}

template <int CW, typename NumT>
int launch_mcw(int S_act, hipStream_t st, size_t lds, const float* Wt, int kp, const void* num,
               int dn, const void* cat, int dc, int cspan, const void* y, int y_i8, int B, int R,
               int dim, int K, int variant, float C, int bias, float* ws, const Spill& sp,
               const McwGeom& geo) {
  auto fn = mcw_round_kernel<CW, NumT>;
  if (int e = check_dyn_lds((const void*)fn, lds)) return e;
  hipLaunchKernelGGL(fn, dim3(S_act), dim3(128), lds, st, Wt, kp, (const NumT*)num, dn, cat, dc,
                     cspan, y, y_i8, B, R, dim, K, variant, C, bias, ws, sp, geo);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace omldm

using namespace omldm;

// 1 when the wide round takes this shape with a table of 2^log2gcap entries per spoke.
OMLDM_API int omldm_multiclass_wide_fits(int dn, int dc, int bias, int nclass, int R, int cspan,
                                         int dim, int log2gcap) {
  return mcw_fits(dn, dc, bias, nclass, R, cspan, dim, log2gcap) ? 1 : 0;
}

// log2 of the table entries per spoke the wide round needs for this shape (mcw_table_log2).
OMLDM_API int omldm_multiclass_wide_table_log2(int dn, int dc, int bias, int R, int cspan,
                                               int dim) {
  return mcw_table_log2(dn, dc, bias, R, cspan, dim);
}

// One Synchronous round of S exact sequential MultiClassPA spokes of R rows on a hashed
// batch. Wt: the fp32 key-major shadow [dim][kp], kp = class_pad(nclass); dacc
// [nclass][dim] += Σ_s Δ_s; stats[0..3] += loss, rows, mistakes, spokes with rows; stats[5]
// += keys the table could not take (0: the launcher refuses such a table). ws: S·8 floats;
// table: spill_words(S, log2gcap, kp) words, keys −1 and the rest 0 (every round leaves it
// so). Returns a HIP error code, or < 0 for what it does not take (nothing is launched).
OMLDM_API int omldm_multiclass_wide_round(const void* Wt, int wt_bf16, const void* num,
                                          int num_bf16, int dn, const void* cat, int dc, int cspan,
                                          const void* y, int y_i8, int B, int R, int S, int dim,
                                          int nclass, int variant, float C, int bias, float* dacc,
                                          float* stats, float* ws, void* table, int log2gcap,
                                          void* stream) {
  if (wt_bf16) return -7;  // fp32 shadow only
  if (nclass < 2 || nclass > kMcwMaxK) return -3;
  if (!mcw_shape_fits(dn, dc, bias, nclass)) return -2;
  if (B < 0 || R < 1 || S < 1 || dim < 1 || cspan < 0 || !Wt || !dacc || !stats || !ws || !table ||
      !y || (dn > 0 && !num) || (dc > 0 && !cat))
    return -4;
  if (variant < 0 || variant > 2 || !(C > 0.f)) return -4;
  if (!mcw_fits(dn, dc, bias, nclass, R, cspan, dim, log2gcap)) return -6;
  if (B == 0) return 0;
  const int F = dn + dc + (bias ? 1 : 0);
  const int kp = nclass <= 2 ? 2 : nclass <= 4 ? 4 : nclass <= 8 ? 8 : nclass <= 16 ? 16
                                                                  : (nclass + 3) / 4 * 4;
  const int CW = mcw_cw(nclass);
  const int U = mcw_step(CW);
  McwGeom geo{};
  geo.FS = ((F + U - 1) / U * U) | 1;
  geo.nodup = cspan > 0 && (long long)dn + (long long)dc * cspan <= (long long)dim - (bias ? 1 : 0);
  for (geo.CR = 32; geo.CR > 8; geo.CR >>= 1)
    if (mcw_lds_bytes(geo.CR, geo.FS, nclass) <= (size_t)kMcwLds) break;
  const size_t lds = mcw_lds_bytes(geo.CR, geo.FS, nclass);
  if (lds > (size_t)kMcwLds) return -5;
  const Spill sp = make_spill(table, S, log2gcap, kp);
  const long long sact = ((long long)B + R - 1) / R;
  const int S_act = sact < S ? (int)sact : S;
  hipStream_t st = (hipStream_t)stream;
  const float* wt = static_cast<const float*>(Wt);
  int e;
#define OMLDM_MCW(CWW)                                                                         \
  e = num_bf16 ? launch_mcw<CWW, __hip_bfloat16>(S_act, st, lds, wt, kp, num, dn, cat, dc, cspan, \
                                                 y, y_i8, B, R, dim, nclass, variant, C, bias, ws, \
                                                 sp, geo)                                      \
               : launch_mcw<CWW, float>(S_act, st, lds, wt, kp, num, dn, cat, dc, cspan, y, y_i8, \
                                        B, R, dim, nclass, variant, C, bias, ws, sp, geo)
  if (CW == 1) OMLDM_MCW(1);
  else if (CW == 2) OMLDM_MCW(2);
  else OMLDM_MCW(4);
#undef OMLDM_MCW
  if (e) return e;
  // a spoke lists at most its worst-case distinct keys (≤ half the table)
  const long long maxn = (long long)1 << (log2gcap - 1);
  const int epb = 256 / kp;
  long long blocks = (maxn + epb - 1) / epb;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  for (int s = 0; s < S_act; ++s)
    hipLaunchKernelGGL(mcw_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, st, sp, s, kp, nclass,
                       dim, dacc);
  hipLaunchKernelGGL(mcw_finish_kernel, dim3(1), dim3(64), 0, st, ws, S_act, sp, stats);
  return (int)hipGetLastError();
}
