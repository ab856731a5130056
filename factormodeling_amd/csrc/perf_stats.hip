// Performance statistics of a returns table (portfolio_analyzer.py of the reference, batched):
// fmx_perf_stats / fmx_perf_periods.
//
// One series is one column of a dates x K table of SIMPLE returns, stored [K][ld] with the T rows
// of a series contiguous (NaN = no observation).  k_perf_stats runs one 256-thread workgroup per
// series; every number is pandas' operation sequence on that series alone, so a series gives the
// same bits alone or in a batch of any K (fixed order, no atomics).
//
// * Series.mean() / .std() (nanops.nanmean / nanvar): numpy's pairwise sum of the NaN -> 0 masked
//   values over the full T, divided by the count; the variance is the pairwise sum of
//   (avg - v) * (avg - v), masked, over count - 1.  pf_pw_sum walks the schedule of length T
//   (rowkit.hpp's tables).  The same for E = R - rf_daily.
//   (pf_pw_sum below: block_pw_sum with the 1 .. 7-element last buffer of n = 8193 .. 8199 summed
//   sequentially, as numpy does.)
// * Sortino's downside series E[E < 0]: compacted in date order into LDS (each thread owns a
//   contiguous run of rows; one exclusive scan of the per-thread counts gives its slot), then
//   the same two sums on the schedule of ITS length m (pw.get(m)).
// * cumprod / cummax / drawdown: sequential by nature (a scan with another association does not
//   round like numpy's left-to-right accumulate), so after the sums the LDS buffer is refilled with
//   the series and lane 0 walks it: cp *= 1 + r, cum = cp - 1, peak = max(peak, cum + 1),
//   dd = (cum + 1) / peak - 1, NaN rows skipped (NaN out).  cum is left in LDS and stored by the
//   whole block; dd is stored by the walking lane.  (A branch-free walk in batches of eight rows,
//   meant to overlap a batch's divides, measured 12 % slower and was not kept: DESIGN section 29.)
//
// LDS: T doubles (dynamic) + 520 doubles of pairwise nodes; T <= FMX_PERF_TMAX = 16384 (128 KiB).
// A 2,520-row series takes 24 KiB, six workgroups per CU.
//
// k_perf_periods: one workgroup per series, one thread per bucket; seg is non-decreasing, so a
// bucket's rows are the range between two binary searches, and its product runs left to right
// over the non-NaN rows.  A seg that breaks its contract cannot move an access out of [0, T).
#include <cmath>

#include "rowkit.hpp"

namespace fmx {

constexpr int PF_NT = 256;
constexpr int PF_NODES = 2 * (FMX_PERF_TMAX / 64) + 8;     // numpy leaves past n = 128 hold >= 64 elements

// block_pw_sum (rowkit.hpp) for ANY n <= FMX_PERF_TMAX.  Past 8192 elements numpy adds the sums of
// 8192-element buffers in order, so for n = 8193 .. 8199 (and 16385 ..) the last buffer is a leaf of
// 1 .. 7 elements, which numpy sums sequentially from 0; rowkit's version forms every leaf of a
// multi-leaf schedule from 8 lanes and would read elem(i) for i >= n there.  Here such a leaf is
// summed by its first lane alone, and elem(i) is never called with i >= n.  nodes: >= 2L + 1 doubles.
template <class Elem>
__device__ double pf_pw_sum(Elem elem, const int32_t* __restrict__ sched, double* nodes) {
  PwView s{sched};
  const int L = s.L();
  const int tid = threadIdx.x;
  if (L == 0) {
    if (tid == 0) {
      double r = 0.0;
      const int n = s.n();
      for (int i = 0; i < n; ++i) r += elem(i);
      nodes[0] = r;
    }
    __syncthreads();
    const double r = nodes[0];
    __syncthreads();
    return r;
  }
  for (int t0 = 0; t0 < L * 8; t0 += PF_NT) {
    const int t = t0 + tid;
    const bool act = t < L * 8;
    const int leaf = t >> 3, j = t & 7;
    double r = 0.0;
    int st = 0, len = 0, stop = 0;
    if (act) {
      st = s.lstart(leaf);
      len = s.llen(leaf);
      stop = len < 8 ? 0 : len - (len & 7);                // a short leaf is all tail
      if (len >= 8) {
        r = elem(st + j);
        for (int i = 8; i < stop; i += 8) r += elem(st + i + j);
      }
    }
    // ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)) as an xor butterfly (IEEE + commutes)
    r = r + __shfl_xor(r, 1);
    r = r + __shfl_xor(r, 2);
    r = r + __shfl_xor(r, 4);
    if (act && j == 0) {
      if (len < 8) r = 0.0;                                // numpy: res = 0.; res += a[i] ...
      for (int i = stop; i < len; ++i) r += elem(st + i);
      nodes[leaf] = r;
    }
  }
  __syncthreads();
  const int R = s.R();
  const int32_t* tr = s.trip();
  for (int rr = 0; rr < R; ++rr) {
    for (int q = s.roff(rr) + tid; q < s.roff(rr + 1); q += PF_NT)
      nodes[tr[3 * q]] = nodes[tr[3 * q + 1]] + nodes[tr[3 * q + 2]];
    __syncthreads();
  }
  const double r = nodes[s.root()];
  __syncthreads();
  return r;
}

// mean and std (ddof 1) of the cnt unmasked cells of a length-n series, pandas' nanmean / nanvar
template <class Val, class Ok>
__device__ void pf_moments(Val val, Ok ok, int cnt, const int32_t* sched, double* nodes, double* mean, double* sd) {
  const double s = pf_pw_sum([&](int i) { return ok(i) ? val(i) : 0.0; }, sched, nodes);
  const double c = (double)cnt;
  const double avg = s / c;                                // cnt == 0: NaN, and neither result reads it
  const double q = pf_pw_sum(
      [&](int i) {
        const double d = avg - val(i);
        return ok(i) ? d * d : 0.0;
      },
      sched, nodes);
  *mean = cnt > 0 ? avg : qnan();
  *sd = cnt > 1 ? sqrt(q / (c - 1.0)) : qnan();
}

__global__ void __launch_bounds__(PF_NT)
k_perf_stats(const double* __restrict__ R, double* __restrict__ stats, double* __restrict__ cum,
             double* __restrict__ dd, int64_t K, int T, int64_t ld, double rf, PwTable pw) {
  extern __shared__ double buf[];                          // [T]: the downside series, then the curve
  __shared__ double nodes[PF_NODES];
  __shared__ double dscr[PF_NT / 64];
  __shared__ int iscr[PF_NT / 64];
  const int tid = threadIdx.x;
  const int64_t k = blockIdx.x;
  const double* r = R + k * ld;
  const double inf = __builtin_inf();

  // ---- counts, extremes and the date-ordered compaction of E < 0
  const int chunk = (T + PF_NT - 1) / PF_NT;
  const int a = tid * chunk < T ? tid * chunk : T;
  const int b = a + chunk < T ? a + chunk : T;
  int c = 0, m = 0;
  double mx = -inf, mn = inf;
  for (int i = a; i < b; ++i) {
    const double v = r[i];
    const bool ok = v == v;
    c += ok;
    m += (v - rf < 0.0);                                   // false on NaN
    mx = (ok && v > mx) ? v : mx;
    mn = (ok && v < mn) ? v : mn;
  }
  int cnt, nneg;
  block_exscan<PF_NT>(c, iscr, &cnt);
  int pos = block_exscan<PF_NT>(m, iscr, &nneg);
  for (int i = a; i < b; ++i) {
    const double e = r[i] - rf;
    if (e < 0.0) buf[pos++] = e;                           // pos < nneg <= T
  }
  mx = block_max<PF_NT>(mx, dscr);
  mn = block_min<PF_NT>(mn, dscr);
  __syncthreads();

  // ---- the six pairwise sums
  const int32_t* sT = pw.get(T);
  auto ok = [&](int i) { const double v = r[i]; return v == v; };
  auto yes = [](int) { return true; };
  double mean_r, sd_r, mean_e, sd_e, mean_n, sd_n;
  pf_moments([&](int i) { return r[i]; }, ok, cnt, sT, nodes, &mean_r, &sd_r);
  pf_moments([&](int i) { return r[i] - rf; }, ok, cnt, sT, nodes, &mean_e, &sd_e);
  pf_moments([&](int i) { return buf[i]; }, yes, nneg, pw.get(nneg), nodes, &mean_n, &sd_n);

  // ---- the curves: the series into LDS, lane 0 walks it
  for (int i = tid; i < T; i += PF_NT) buf[i] = r[i];
  __syncthreads();
  if (tid == 0) {
    double cp = 1.0, peak = -inf, mdd = inf, last = qnan();
    int mrow = -1, prow = -1, mprow = -1, run = 0, best = 0;
    double* ddk = dd ? dd + k * ld : nullptr;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const double v = buf[t];
      double d = qnan();
      last = qnan();
      if (v == v) {
        cp = cp * (1.0 + v);
        const double cu = cp - 1.0, c1 = cu + 1.0;         // the class re-adds 1 to cumulative_return
        buf[t] = cu;
        if (c1 > peak) { peak = c1; prow = t; }
        d = c1 / peak - 1.0;
        if (d < mdd) { mdd = d; mrow = t; mprow = prow; }
        if (d < 0.0) { run += 1; best = run > best ? run : best; }
        else run = 0;
        last = c1;
      }
      if (ddk) ddk[t] = d;
    }
    double* s = stats + k;
    s[FMX_PERF_MEAN * K] = mean_r;
    s[FMX_PERF_STD * K] = sd_r;
    s[FMX_PERF_MAX * K] = cnt > 0 ? mx : qnan();
    s[FMX_PERF_MIN * K] = cnt > 0 ? mn : qnan();
    s[FMX_PERF_COUNT * K] = (double)cnt;
    s[FMX_PERF_EX_MEAN * K] = mean_e;
    s[FMX_PERF_EX_STD * K] = sd_e;
    s[FMX_PERF_DOWN_COUNT * K] = (double)nneg;
    s[FMX_PERF_DOWN_MEAN * K] = mean_n;
    s[FMX_PERF_DOWN_STD * K] = sd_n;
    s[FMX_PERF_FINAL * K] = last;
    s[FMX_PERF_MAXDD * K] = mrow >= 0 ? mdd : qnan();
    s[FMX_PERF_MAXDD_ROW * K] = (double)mrow;
    s[FMX_PERF_MAXDD_PEAK_ROW * K] = (double)mprow;
    s[FMX_PERF_DD_RUN * K] = (double)best;
  }
  __syncthreads();
  if (cum) {
    double* ck = cum + k * ld;
    for (int i = tid; i < T; i += PF_NT) ck[i] = buf[i];   // NaN rows still hold their NaN
  }
}

// first row t in [0, T) with seg[t] >= s (T if none)
__device__ __forceinline__ int pf_lower(const int32_t* __restrict__ seg, int T, int s) {
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(PF_NT)
k_perf_periods(const double* __restrict__ R, const int32_t* __restrict__ seg, double* __restrict__ out, int64_t K,
               int T, int64_t ld, int nseg) {
  const int64_t k = blockIdx.x;
  const double* r = R + k * ld;
  for (int s = threadIdx.x; s < nseg; s += PF_NT) {
    const int lo = pf_lower(seg, T, s);
    const int hi = s + 1 < nseg ? pf_lower(seg, T, s + 1) : T;   // lo, hi in [0, T] whatever seg holds
    double p = 1.0;
    for (int t = lo; t < hi; ++t) {
      const double v = r[t];
      p = (v == v) ? p * (1.0 + v) : p;
    }
    out[(int64_t)s * K + k] = p - 1.0;
  }
}

}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_perf_stats(const double* R, int64_t K, int64_t T, int64_t ld, double rf_daily,
                                     double* stats, double* cum, double* dd, void* stream) {
  FMX_ARG(R && stats, "perf_stats: null returns or stats");
  FMX_ARG(K >= 1 && T >= 1, "perf_stats: K and T must be >= 1");
  FMX_ARG(ld >= T, "perf_stats: ld < T");
  FMX_ARG(T <= FMX_PERF_TMAX, "perf_stats: more than 16384 rows per series (FMX_PERF_TMAX)");
  FMX_ARG(K < (int64_t)1 << 31, "perf_stats: too many series for one launch");
  FMX_ARG(cum != R && dd != R && (!cum || cum != dd), "perf_stats: cum / dd may not alias R or each other");
  fmx_status e = FMX_OK;
  PwTable pw = pw_table((int)T, &e);
  if (e) return e;
  const size_t lds = (size_t)T * sizeof(double);
  const void* kf = (const void*)k_perf_stats;
  if (lds > 64 * 1024) FMX_HIP(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int t32 = (int)T;
  void* args[] = {(void*)&R, (void*)&stats, (void*)&cum, (void*)&dd, (void*)&K, (void*)&t32, (void*)&ld,
                  (void*)&rf_daily, (void*)&pw};
  FMX_HIP(hipLaunchKernel(kf, dim3((unsigned)K), dim3(PF_NT), args, lds, as_stream(stream)));
  return FMX_OK;
}

extern "C" fmx_status fmx_perf_periods(const double* R, int64_t K, int64_t T, int64_t ld, const int32_t* seg,
                                       int32_t nseg, double* out, void* stream) {
  FMX_ARG(R && seg && out, "perf_periods: null returns, seg or out");
  FMX_ARG(K >= 1 && T >= 1, "perf_periods: K and T must be >= 1");
  FMX_ARG(ld >= T, "perf_periods: ld < T");
  FMX_ARG(nseg >= 1, "perf_periods: nseg must be >= 1");
  FMX_ARG(T < (int64_t)1 << 31 && K < (int64_t)1 << 31, "perf_periods: table too large for one launch");
  FMX_ARG(out != R, "perf_periods: out may not alias R");
  hipLaunchKernelGGL(k_perf_periods, dim3((unsigned)K), dim3(PF_NT), 0, as_stream(stream), R, seg, out, K, (int)T, ld,
                     (int)nseg);
  FMX_LAUNCH_CHECK("k_perf_periods");
  return FMX_OK;
}
