// Quantile backtest (composite_factor.py:47-134, the inner quantile_backtest_log :63-98):
// per-date quantile buckets of a factor and the mean return of every bucket, lagged one
// row per symbol.  DESIGN.md §15.
//
//   k_cs_qlabel     one (factor, date) row per workgroup: ordinal ranks (pandas
//                   rank(method="first"): ties by the lower asset column) from an LDS
//                   bitonic sort of (key, asset) pairs, the pd.qcut label of every rank from
//                   the date's row of the host-built cut table, one uint8 group per cell.
//   k_cs_qlabel_part  the same output for rows past 1,024 assets: sample buckets, and a
//                   sort of only the buckets that a rank threshold cuts.
//   k_qbucket_mean  one date x a chunk of factors per workgroup: the returns row staged in
//                   LDS, the label bytes of every cell's previous row, exact fixed-point
//                   sums (exactsum.hpp) and counts per group -> mean / count.
//
// The cut points are pandas' own: cum[m][k] = number of ordinal ranks 1..m whose qcut label
// is <= k comes from the host (engine.qcut_cum), because pandas' floating-point bin edges
// do not follow a closed form (an edge can land an ulp below an integer).
#include <vector>

#include "exactsum.hpp"
#include "rank_launch.hpp"
#include "rowkit.hpp"

namespace fmx {

constexpr int QL_MAX_A = 8192;      // (key, asset) pairs of one row in LDS: 10 B per slot
constexpr int QL_MAX_GROUPS = 32;
constexpr int QL_NT = 256;          // k_cs_qlabel: rows of A <= 1024
constexpr int QB_NT = 256;
constexpr int QB_NW = QB_NT / FMX_WAVE;
constexpr int QB_SLOTS = EX_SLOTS + 1;   // limbs, invalid-term flag, count
// Returns are scaled by 2^48 (exact) before the fixed-point conversion: the accumulator's
// LSB is then 2^-112 of a return, so every double of magnitude >= 2^-60 adds without
// truncation (exactsum.hpp alone truncates at 2^-64, which a return of 1e-4 already
// reaches); a term below 2^-60 loses what lies under 2^-112.  |r| >= 2^79 or non-finite
// sets the flag limb: the bucket's mean is NaN.
constexpr double QB_SCALE = 281474976710656.0;            // 2^48
constexpr double QB_UNSCALE = 1.0 / QB_SCALE;

// labels [F][D][A] (dense, no padding): 0 = no group (absent, NaN, or a date of m <= 1
// valid cells), else n - label (1 = top).  A date whose m has no row in the cut table
// (m_index[m] < 0) writes 255 on its valid cells.
__global__ void __launch_bounds__(QL_NT)
k_cs_qlabel(const double* __restrict__ X, const uint8_t* __restrict__ present, const int32_t* __restrict__ cum,
            const int32_t* __restrict__ m_index, uint8_t* __restrict__ labels, int64_t D, int64_t A, int64_t ld, int P,
            int n) {
  extern __shared__ uint64_t keys[];
  uint16_t* idx = (uint16_t*)(keys + P);
  int* iscr = (int*)(idx + P + 8);
  int* cm = iscr + 16;
  const int64_t d = blockIdx.x, f = blockIdx.y;
  const double* x = X + (f * D + d) * ld;
  uint8_t* lab = labels + (f * D + d) * A;
  const uint8_t* prow = present ? present + d * ld : nullptr;
  int nv_l = 0;
  for (int i = threadIdx.x; i < P; i += QL_NT) {
    uint64_t k = KEY_SENTINEL;
    uint16_t id = 0xffff;
    if (i < A && (prow ? prow[i] != 0 : true)) {
      const double t = x[i];
      if (t == t) { k = okey(t); id = (uint16_t)i; nv_l += 1; }
    }
    keys[i] = k;
    idx[i] = id;
  }
  int m;
  block_exscan<QL_NT>(nv_l, iscr, &m);
  const int row = m >= 2 ? m_index[m] : -1;             // block-uniform
  if (m >= 2 && row < 0) {                               // no table row for this m
    for (int i = threadIdx.x; i < A; i += QL_NT) lab[i] = idx[i] != 0xffff ? 255 : 0;   // own slots
    return;
  }
  const bool sorted = m >= 2;
  if (sorted) {
    if ((int)threadIdx.x < n) cm[threadIdx.x] = cum[(int64_t)row * n + threadIdx.x];
    bitonic_sort<QL_NT>(keys, idx, P);                     // ends with a barrier: cm is visible
  }
  // the sorted keys are not read again (rank of sorted position p is p + 1): the label
  // bytes are assembled over them and leave in one coalesced pass
  constexpr int EPT = 1024 / QL_NT;                     // serves P <= 1024
  int assets[EPT];
  uint8_t groups[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int p = threadIdx.x + k * QL_NT;
    assets[k] = -1;
    groups[k] = 0;
    if (!sorted || p >= m) continue;                    // m <= A <= P
    assets[k] = idx[p];
    const int r = p + 1;
    int lo = 0, hi = n;                                 // first k with cum[k] >= r
    while (lo < hi) { const int md = (lo + hi) >> 1; if (cm[md] < r) lo = md + 1; else hi = md; }
    groups[k] = (uint8_t)(n - lo);                      // lo == n (a short table row): none
  }
  __syncthreads();
  uint8_t* lb = (uint8_t*)keys;
  for (int i = threadIdx.x; i < A; i += QL_NT) lb[i] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EPT; ++k)
    if (assets[k] >= 0) lb[assets[k]] = groups[k];
  __syncthreads();
  if ((A & 3) == 0) {                                   // rows start 4-byte aligned
    const uint32_t* src = (const uint32_t*)lb;
    uint32_t* dst = (uint32_t*)lab;
    for (int i = threadIdx.x; i < (int)(A >> 2); i += QL_NT) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < A; i += QL_NT) lab[i] = lb[i];
  }
}

// Rows of more than 1,024 assets: the label of a cell only depends on which side of the
// n - 1 rank thresholds cum[0 .. n-2] its ordinal rank falls, so a full sort is not needed.
//   1. QP_S positional samples are sorted as (key, asset) pairs; the pairs are all distinct,
//      so equal keys spread over the buckets by asset and ties cannot crowd one bucket.
//   2. every valid cell finds its bucket (#samples below it, binary search) and counts it;
//      a scan turns the counts into the rank range (st[b], st[b+1]] of every bucket.
//   3. a bucket with no threshold strictly inside its range labels its cells at once; the
//      cells of the (at most n - 1) other buckets are compacted and sorted with the bitonic
//      sort, sized by their number, and take rank = st[b] + position in the bucket.
// Any input is handled: if the sample is bad (most cells in one bucket) the sort just grows,
// up to the whole row.  1,024 threads, 8 cells per thread.
constexpr int QP_NT = 1024;
constexpr int QP_EPT = QL_MAX_A / QP_NT;
constexpr int QP_S = 256;
constexpr int QP_NB = QP_S + 1;

__device__ __forceinline__ int ql_label(const int* cm, int n, int r) {
  int lo = 0, hi = n;                                   // first k with cum[k] >= r
  while (lo < hi) { const int md = (lo + hi) >> 1; if (cm[md] < r) lo = md + 1; else hi = md; }
  return n - lo;                                        // lo == n (a short table row): none
}

__global__ void __launch_bounds__(QP_NT)
k_cs_qlabel_part(const double* __restrict__ X, const uint8_t* __restrict__ present, const int32_t* __restrict__ cum,
                 const int32_t* __restrict__ m_index, uint8_t* __restrict__ labels, int64_t D, int64_t A, int64_t ld,
                 int P, int n) {
  extern __shared__ uint64_t keys[];
  uint64_t* skey = keys + P;
  uint16_t* idx = (uint16_t*)(skey + QP_S);
  uint16_t* sidx = idx + P + 8;
  int* iscr = (int*)(sidx + QP_S);
  int* cm = iscr + 16;                                  // [32]
  int* cnt = cm + QL_MAX_GROUPS;                        // [QP_NB + 1] bucket sizes
  int* st = cnt + QP_NB + 1;                            // [QP_NB + 1] ranks before the bucket
  int* coff = st + QP_NB + 1;                           // [QP_NB + 1] offset in the sort buffer, -1 = not sorted
  int* fill = coff + QP_NB + 1;                         // [QP_NB + 1]
  int* flag = fill + QP_NB + 1;                         // [QP_NB + 1]
  int* clb = flag + QP_NB + 1;                          // [32] the sorted buckets, ascending
  int* clo = clb + QL_MAX_GROUPS;                       // [32] their offsets
  uint8_t* lb = (uint8_t*)(clo + QL_MAX_GROUPS);        // [A]
  const int t = threadIdx.x;
  const int64_t d = blockIdx.x, f = blockIdx.y;
  const double* x = X + (f * D + d) * ld;
  uint8_t* lab = labels + (f * D + d) * A;
  const uint8_t* prow = present ? present + d * ld : nullptr;
  uint64_t key[QP_EPT];
  int nv_l = 0;
#pragma unroll
  for (int k = 0; k < QP_EPT; ++k) {
    const int a = t + k * QP_NT;
    key[k] = KEY_SENTINEL;
    if (a < A && (prow ? prow[a] != 0 : true)) {
      const double v = x[a];
      if (v == v) { key[k] = okey(v); nv_l += 1; }
    }
  }
  for (int i = t; i <= QP_NB; i += QP_NT) { cnt[i] = 0; fill[i] = 0; flag[i] = 0; }
  int m;
  block_exscan<QP_NT>(nv_l, iscr, &m);
  const int row = m >= 2 ? m_index[m] : -1;             // block-uniform
  if (m < 2 || row < 0) {                               // nothing to label / no table row for this m
#pragma unroll
    for (int k = 0; k < QP_EPT; ++k) {
      const int a = t + k * QP_NT;
      if (a < A) lab[a] = (m >= 2 && key[k] != KEY_SENTINEL) ? 255 : 0;
    }
    return;
  }
  if (t < n) cm[t] = cum[(int64_t)row * n + t];
  if (t < QP_S) {                                       // positional sample (A > QP_S: distinct cells)
    const int a = (int)(((int64_t)t * A) / QP_S);
    uint64_t k = KEY_SENTINEL;
    if (prow ? prow[a] != 0 : true) {
      const double v = x[a];
      if (v == v) k = okey(v);
    }
    skey[t] = k;
    sidx[t] = (uint16_t)a;
  }
  __syncthreads();
  bitonic_sort<QP_NT>(skey, sidx, QP_S);
  int bk[QP_EPT];
#pragma unroll
  for (int k = 0; k < QP_EPT; ++k) {
    bk[k] = -1;
    if (key[k] == KEY_SENTINEL) continue;
    const uint32_t a = t + k * QP_NT;
    int lo = 0, hi = QP_S;                              // #samples below (key, a)
    while (lo < hi) {
      const int md = (lo + hi) >> 1;
      const uint64_t sk = skey[md];
      if (sk < key[k] || (sk == key[k] && (uint32_t)sidx[md] < a)) lo = md + 1; else hi = md;
    }
    bk[k] = lo;
    atomicAdd(&cnt[lo], 1);
  }
  __syncthreads();
  {
    int tot;
    const int e = block_exscan<QP_NT>(t < QP_NB ? cnt[t] : 0, iscr, &tot);
    if (t < QP_NB) st[t] = e;
    if (t == 0) st[QP_NB] = tot;                        // == m
  }
  __syncthreads();
  if (t < n - 1) {                                      // the bucket threshold t falls strictly inside
    const int c = cm[t];
    int lo = 0, hi = QP_NB + 1;                         // first i with st[i] >= c
    while (lo < hi) { const int md = (lo + hi) >> 1; if (st[md] < c) lo = md + 1; else hi = md; }
    if (lo >= 1 && lo <= QP_NB && st[lo] != c) flag[lo - 1] = 1;
  }
  __syncthreads();
  int C, ncrit;
  {
    const bool fl = t < QP_NB && flag[t] != 0;
    const int e = block_exscan<QP_NT>(fl ? cnt[t] : 0, iscr, &C);
    const int j = block_exscan<QP_NT>(fl ? 1 : 0, iscr, &ncrit);
    if (t < QP_NB) coff[t] = fl ? e : -1;
    if (fl) { clb[j] = t; clo[j] = e; }
  }
  __syncthreads();
  int Pc = 2;
  while (Pc < C) Pc <<= 1;                              // C <= m <= A <= P
#pragma unroll
  for (int k = 0; k < QP_EPT; ++k) {
    const int a = t + k * QP_NT;
    if (a >= A) continue;
    const int b = bk[k];
    if (b < 0) { lb[a] = 0; continue; }
    const int o = coff[b];
    if (o < 0) { lb[a] = (uint8_t)ql_label(cm, n, st[b] + 1); continue; }
    const int pos = o + atomicAdd(&fill[b], 1);
    keys[pos] = key[k];
    idx[pos] = (uint16_t)a;
  }
  for (int i = C + t; i < Pc; i += QP_NT) { keys[i] = KEY_SENTINEL; idx[i] = 0xffff; }
  __syncthreads();
  if (C > 0) {
    bitonic_sort<QP_NT>(keys, idx, Pc);
    for (int q = t; q < C; q += QP_NT) {
      int j = 0;
      while (j + 1 < ncrit && clo[j + 1] <= q) ++j;
      lb[idx[q]] = (uint8_t)ql_label(cm, n, st[clb[j]] + (q - clo[j]) + 1);
    }
  }
  __syncthreads();
  if ((A & 3) == 0) {                                   // rows start 4-byte aligned
    const uint32_t* src = (const uint32_t*)lb;
    uint32_t* dst = (uint32_t*)lab;
    for (int i = t; i < (int)(A >> 2); i += QP_NT) dst[i] = src[i];
  } else {
    for (int i = t; i < A; i += QP_NT) lab[i] = lb[i];
  }
}

static size_t qp_lds_bytes(int P, int64_t A) {
  return (size_t)P * 10 + 16 + QP_S * 10 + 16 * 4 + QL_MAX_GROUPS * 4 * 3 + (QP_NB + 1) * 4 * 5 + (size_t)A + 64;
}

// acc: [QB_NW][rep][n][QB_SLOTS] 64-bit integers.  Integer additions commute, so the LDS
// atomics give the same limbs in any order and under any launch geometry.
__global__ void __launch_bounds__(QB_NT)
k_qbucket_mean(const uint8_t* __restrict__ labels, const double* __restrict__ R, const uint8_t* __restrict__ rpresent,
               const int32_t* __restrict__ prev_row, double* __restrict__ mean, int32_t* __restrict__ count, int64_t F,
               int64_t D, int64_t A, int n, int fchunk, int rep) {
  extern __shared__ unsigned long long qacc[];
  const int nacc = QB_NW * rep * n * QB_SLOTS;
  double* rs = (double*)(qacc + nacc);
  int32_t* pv = (int32_t*)(rs + A);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t d = blockIdx.x;
  const int64_t f0 = (int64_t)blockIdx.y * fchunk, f1 = f0 + fchunk < F ? f0 + fchunk : F;
  for (int i = t; i < nacc; i += QB_NT) qacc[i] = 0ull;
  for (int64_t a = t; a < A; a += QB_NT) {
    double r = R[d * A + a];
    if (rpresent && !rpresent[d * A + a]) r = qnan();
    int32_t p = prev_row ? prev_row[d * A + a] : (int32_t)d - 1;
    if (p < -1 || p >= D) p = -1;                       // checked on the host before the launch
    if (p < 0) r = qnan();
    rs[a] = r;
    if (prev_row) pv[a] = p;
  }
  __syncthreads();
  unsigned long long* mine = qacc + (size_t)(w * rep + lane % rep) * n * QB_SLOTS;
  for (int64_t f = f0; f < f1; ++f) {
    const uint8_t* lf = labels + f * D * A;
    for (int64_t a = t; a < A; a += QB_NT) {
      const double r = rs[a];
      if (!(r == r)) continue;
      const int64_t p = prev_row ? (int64_t)pv[a] : d - 1;
      const int g = lf[p * A + a];
      if (g == 0 || g > n) continue;
      int64_t lim[EX_SLOTS];
#pragma unroll
      for (int k = 0; k < EX_SLOTS; ++k) lim[k] = 0;
      ex_add(lim, r * QB_SCALE);
      unsigned long long* dst = mine + (g - 1) * QB_SLOTS;
#pragma unroll
      for (int k = 0; k < EX_SLOTS; ++k)
        if (lim[k] != 0) atomicAdd(dst + k, (unsigned long long)lim[k]);
      atomicAdd(dst + EX_SLOTS, 1ull);
    }
    __syncthreads();
    if (t < n) {
      int64_t tot[QB_SLOTS];
#pragma unroll
      for (int k = 0; k < QB_SLOTS; ++k) tot[k] = 0;
      for (int c = 0; c < QB_NW * rep; ++c)
#pragma unroll
        for (int k = 0; k < QB_SLOTS; ++k) tot[k] += (int64_t)qacc[((size_t)c * n + t) * QB_SLOTS + k];
      const int64_t cnt = tot[EX_SLOTS];
      const int64_t o = (f * D + d) * n + t;
      mean[o] = cnt > 0 ? (ex_value(tot) * QB_UNSCALE) / (double)cnt : qnan();
      count[o] = (int32_t)cnt;
    }
    __syncthreads();
    for (int i = t; i < nacc; i += QB_NT) qacc[i] = 0ull;
    __syncthreads();
  }
}

static int qb_rep(int n) { return n <= 10 ? 8 : 2; }

}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_cs_qlabel(const double* X, const uint8_t* present, const int32_t* cum,
                                    const int32_t* m_index, uint8_t* labels, int64_t F, int64_t D, int64_t A,
                                    int64_t ld, int32_t n_groups, void* stream) {
  FMX_ARG(n_groups >= 2 && n_groups <= QL_MAX_GROUPS, "qlabel: 2 <= n_groups <= 32");
  FMX_ARG(F >= 0 && D >= 0 && A >= 0 && ld >= A && D <= 0x7fffffff && F <= 65535, "qlabel: bad dims");
  FMX_ARG(A <= QL_MAX_A, "qlabel: rows of A <= 8192 assets");
  if (F == 0 || D == 0 || A == 0) return FMX_OK;
  FMX_ARG(X && cum && m_index && labels, "null pointer");
  int P = next_pow2((int)A);
  if (P < 2) P = 2;
  // rows past 1,024 assets: sample buckets, only the buckets a threshold cuts are sorted
  const bool part = P > 1024;
  const size_t lds = part ? qp_lds_bytes(P, A) : (size_t)P * 10 + 16 + 16 * 4 + QL_MAX_GROUPS * 4 + 64;
  const void* k = part ? (const void*)k_cs_qlabel_part : (const void*)k_cs_qlabel;
  const int nt = part ? QP_NT : QL_NT;
  FMX_HIP(set_dyn_lds(k, lds));
  int n = n_groups;
  void* args[] = {(void*)&X, (void*)&present, (void*)&cum, (void*)&m_index, (void*)&labels, (void*)&D, (void*)&A,
                  (void*)&ld, (void*)&P, (void*)&n};
  FMX_HIP(hipLaunchKernel(k, dim3((unsigned)D, (unsigned)F), dim3(nt), args, lds, as_stream(stream)));
  return FMX_OK;
}

extern "C" fmx_status fmx_qbucket_mean(const uint8_t* labels, const double* R, const uint8_t* rpresent,
                                       const int32_t* prev_row, double* mean, int32_t* count, int64_t F, int64_t D,
                                       int64_t A, int32_t n_groups, void* stream) {
  FMX_ARG(n_groups >= 2 && n_groups <= QL_MAX_GROUPS, "qbucket_mean: 2 <= n_groups <= 32");
  FMX_ARG(F >= 0 && D >= 0 && A >= 0 && D <= 0x7fffffff, "qbucket_mean: bad dims");
  FMX_ARG(A <= QL_MAX_A, "qbucket_mean: rows of A <= 8192 assets");
  if (F == 0 || D == 0) return FMX_OK;
  FMX_ARG(mean && count, "null pointer");
  FMX_ARG(A == 0 || (labels && R), "null pointer");
  hipStream_t s = as_stream(stream);
  // the previous-row table is read back and checked: an entry outside [-1, D) is an
  // argument error, not a fault
  if (prev_row && A > 0) {
    std::vector<int32_t> hp((size_t)(D * A));
    FMX_HIP(hipMemcpyAsync(hp.data(), prev_row, sizeof(int32_t) * hp.size(), hipMemcpyDeviceToHost, s));
    FMX_HIP(hipStreamSynchronize(s));
    for (int32_t v : hp) FMX_ARG(v >= -1 && v < D, "qbucket_mean: prev_row entry outside [-1, D)");
  }
  int n = n_groups;
  const int rep = qb_rep(n);
  // factors per workgroup: enough workgroups to fill the device, the returns row staged
  // once per workgroup (the result does not depend on the split)
  int64_t fc = (F * D) / 4096;
  fc = fc < 1 ? 1 : (fc > 16 ? 16 : fc);
  int fchunk = (int)fc;
  const int64_t gy = ceil_div(F, fc);
  FMX_ARG(gy <= 65535, "qbucket_mean: too many factors for one call");
  const size_t lds = (size_t)QB_NW * rep * n * QB_SLOTS * 8 + (size_t)A * 8 + (prev_row ? (size_t)A * 4 : 0);
  FMX_HIP(set_dyn_lds((const void*)k_qbucket_mean, lds));
  void* args[] = {(void*)&labels, (void*)&R, (void*)&rpresent, (void*)&prev_row, (void*)&mean, (void*)&count,
                  (void*)&F, (void*)&D, (void*)&A, (void*)&n, (void*)&fchunk, (void*)&rep};
  FMX_HIP(hipLaunchKernel((const void*)k_qbucket_mean, dim3((unsigned)D, (unsigned)gy), dim3(QB_NT), args, lds, s));
  return FMX_OK;
}
