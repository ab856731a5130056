// Rolling order statistics (per-symbol): ts_min / ts_max / ts_argmin / ts_argmax /
// ts_median / ts_quantile.  Builder-defined (the reference has none of them), pinned to
// pandas: x.rolling(w).min() / .max() / .median() / .quantile(q, interpolation), and for the
// arg operators rolling(w).apply(rows back to the extreme, ties to the most recent row).
//
// Row semantics are ts_rank's: a row gets a value only when its symbol has `window` present
// rows ending at it and none of them is NaN; on a ragged panel the window is the symbol's
// last `window` PRESENT rows.  Lanes of a wave are 64 consecutive assets of one factor, so
// every row access is one coalesced 512-B load.  Three kernels, no window refused:
//   k_tso_ext  the four extremes: k_ts_win's date tiles (a thread owns T dates of a column
//              and streams the W + T - 1 rows that feed them once); one compare / select per
//              (row, output), registers only, any W;
//   k_tso_sel  median / quantile with W <= TSO_LDS_MAXW: a per-thread ring of the window's W
//              RANKS (ties broken by age, so the ranks are a permutation of 0..W-1) in LDS;
//              one O(W) sweep per output updates the ranks for the leaving and the entering
//              row and picks up the elements of rank i and i + 1;
//   k_tso_bis  median / quantile for longer windows: stateless, one thread per output, the
//              k-th smallest by bisection on the order-preserving 64-bit key (65 counting
//              passes over the window).
#include <cstdlib>

#include "fmx_common.hpp"

namespace fmx {

constexpr int TSO_T = 16;                       // dates per thread of k_tso_ext
constexpr int TSO_LDS_BYTES = 160 * 1024;
constexpr int TSO_LDS_MAXW = TSO_LDS_BYTES / (64 * 2);   // 1280: W 16-bit ranks x 64 lanes
constexpr int64_t TSO_SEL_MIN_WAVES = 4096;     // k_tso_sel: 256 CUs x 16 one-wave workgroups

// how the output is formed from v0 = sorted[i0] and v1 = sorted[i0 + 1]
constexpr int TSO_SEL_LO = 0;    // v0
constexpr int TSO_SEL_HI = 1;    // v1
constexpr int TSO_SEL_LIN = 2;   // v0 + (v1 - v0) * frac
constexpr int TSO_SEL_MID = 3;   // (v0 + v1) / 2

__device__ __forceinline__ int tso_wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double tso_pos_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

__device__ __forceinline__ double tso_combine(double v0, double v1, int mode, double frac) {
  if (mode == TSO_SEL_LO) return v0;
  if (mode == TSO_SEL_HI) return v1;
  if (mode == TSO_SEL_LIN) return v0 + (v1 - v0) * frac;
  return (v0 + v1) / 2.0;
}

// The date of the (W-1)th present row before d0 in this lane's column (or the column's first
// present row, or d0 when there is none), and how many present rows lie in [s, d0): the walk
// back of k_ts_win, wave-uniform control flow, 8 presence bytes in flight.
__device__ __forceinline__ void tso_walk_back(const uint8_t* pres, int64_t ld, int d0, int W, bool ok, int& pre,
                                              int& s) {
  if (pres == nullptr) {
    pre = min(W - 1, d0);
    s = d0 - pre;
    return;
  }
  pre = 0;
  s = d0;
  for (int db = d0 - 1;; db -= 8) {
    const bool need = ok && pre < W - 1 && db >= 0;
    if (__ballot(need) == 0) break;
    uint8_t pb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) pb[k] = (db - k >= 0) ? pres[(int64_t)(db - k) * ld] : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (need && pre < W - 1 && pb[k]) { ++pre; s = db - k; }
  }
}

// ------------------------------------------------------------------------------------
// Extremes.  The tile scheme of k_ts_win: thread = T consecutive dates of one column; it
// streams the present rows from the (W-1)th before its tile to the tile's end, oldest
// first.  Row p has weight kk = p - q_t + W in output t's window (1 = oldest, W = the
// output's own row); `<=` / `>=` on an oldest-first stream leaves the MOST RECENT of equal
// extremes, and W - kk is its distance in rows.  +-inf are ordinary values; -0.0 == 0.0.
template <int OP, int T>
__global__ void __launch_bounds__(256)
k_tso_ext(const double* __restrict__ X, double* __restrict__ Y, int64_t F, int64_t D, int64_t A, int64_t ld, int W,
          const uint8_t* __restrict__ present, int64_t achunks, int64_t ntiles) {
  static_assert(T <= 30, "tile bit mask");
  constexpr bool ISMIN = OP == FMX_TSO_MIN || OP == FMX_TSO_ARGMIN;
  constexpr bool ISARG = OP == FMX_TSO_ARGMIN || OP == FMX_TSO_ARGMAX;
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t ac = wid % achunks, rest = wid / achunks;
  const int64_t tile = rest % ntiles, f = rest / ntiles;
  if (f >= F) return;                                   // wave-uniform
  const int64_t a = ac * 64 + lane;
  const bool ok = a < A;
  const double* x = X + f * D * ld + (ok ? a : A - 1);
  const uint8_t* pres = present ? present + (ok ? a : A - 1) : nullptr;
  const int Di = (int)D;
  const int d0 = (int)tile * T;
  const int d1 = min(Di, d0 + T);
  unsigned pm = 0;                                      // the tile's present rows
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int d = d0 + t;
    if (d < d1 && (pres == nullptr || pres[(int64_t)d * ld] != 0)) pm |= 1u << t;
  }
  int pre, s;
  tso_walk_back(pres, ld, d0, W, ok, pre, s);
  int qW[T];                                            // q_t - W, q_t = present index from s
  {
    int q = pre;
#pragma unroll
    for (int t = 0; t < T; ++t) { qW[t] = q - W; q += (pm >> t) & 1u; }
  }
  double best[T];
  int bk[T];
  unsigned nanm = 0;
#pragma unroll
  for (int t = 0; t < T; ++t) { best[t] = ISMIN ? tso_pos_inf() : -tso_pos_inf(); bk[t] = 0; }
  const int smin = tso_wave_min(ok ? s : d0);
  int pd = 0;                                           // present index of the next row
  for (int db = smin; db < d1; db += 8) {
    double u[8];
    bool pu[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int d = db + k;
      u[k] = d < d1 ? x[(int64_t)d * ld] : 0.0;
      pu[k] = d < d1 && d >= s && (pres == nullptr || pres[(int64_t)d * ld] != 0);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!pu[k]) continue;
      const double uk = u[k];
      const bool isn = uk != uk;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const unsigned kk = (unsigned)pd - (unsigned)qW[t];  // true value in [-14, 2 W + 15]
        const bool inw = kk - 1u < (unsigned)W;              // 1 <= kk <= W
        const bool take = inw && (ISMIN ? uk <= best[t] : uk >= best[t]);
        best[t] = take ? uk : best[t];
        if (ISARG) bk[t] = take ? (int)kk : bk[t];
        nanm |= (inw && isn) ? (1u << t) : 0u;
      }
      pd += 1;
    }
  }
  if (!ok) return;
  double* y = Y + f * D * ld + a;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int d = d0 + t;
    if (d >= d1) break;
    double o = qnan();
    if (((pm >> t) & 1u) && qW[t] >= -1 && !((nanm >> t) & 1u))   // W present rows, none NaN
      o = ISARG ? (double)(W - bk[t]) : best[t];
    y[(int64_t)d * ld] = o;
  }
}

// ------------------------------------------------------------------------------------
// Median / quantile, W <= TSO_LDS_MAXW.  One wave per (factor, segment of L dates, 64
// assets); a thread walks its column's dates from the (W-1)th present row before the
// segment (the warm-up, no outputs) to the segment's end.  State: ring[j][lane], the rank
// (0 = smallest) of the window element whose present index is j mod W -- 16 bits, lane
// fastest, so a wave's access to any slots is 32 distinct banks.  Elements are ordered by
// (value, age): of equal values the older is smaller, NaN sorts above everything.
// A slide, for entering value xn:
//   the leaving element (same slot as the entering one) has rank ro;
//   every remaining element, re-read oldest first through L2:  rank -= (rank > ro);
//     rank += (element above xn); the elements not above xn are counted;
//   xn's rank is that count.  Whoever ends with rank i0 / i0 + 1 is v0 / v1.
// The remaining elements are the column's present rows between the ring's oldest date and
// the current one, so on a ragged panel the sweep walks dates and skips absent rows; the
// wave sweeps from the smallest such date of its lanes.  Slot indices wrap inside [0, W) by
// construction, whatever the presence mask holds.
__device__ __forceinline__ bool tso_above(double a, double b) { return a > b || (a != a && b == b); }

__global__ void __launch_bounds__(64)
k_tso_sel(const double* __restrict__ X, double* __restrict__ Y, int64_t F, int64_t D, int64_t A, int64_t ld, int W,
          const uint8_t* __restrict__ present, int64_t achunks, int64_t nseg, int L, int i0, int mode, double frac) {
  extern __shared__ uint16_t tso_ring[];                // [W][64]
  const int lane = threadIdx.x & 63;
  const int64_t wid = blockIdx.x;
  const int64_t ac = wid % achunks, rest = wid / achunks;
  const int64_t seg = rest % nseg, f = rest / nseg;
  if (f >= F) return;
  const int64_t a = ac * 64 + lane;
  const bool ok = a < A;
  const double* x = X + f * D * ld + (ok ? a : A - 1);
  double* y = Y + f * D * ld + (ok ? a : A - 1);
  const uint8_t* pres = present ? present + (ok ? a : A - 1) : nullptr;
  const int Di = (int)D;
  const int d0 = (int)seg * L;
  const int d1 = min(Di, d0 + L);
  int pre, s;
  tso_walk_back(pres, ld, d0, W, ok, pre, s);
  const int i1 = mode == TSO_SEL_LO ? i0 : i0 + 1;
  uint16_t* ring = tso_ring + lane;
  int cnt = 0;        // present rows consumed since s
  int cslot = 0;      // cnt mod W: the entering element's slot
  int tail = s;       // date of the ring's oldest element (cnt > 0)
  const int smin = tso_wave_min(ok ? s : d0);
  for (int d = smin; d < d1; ++d) {
    const double xn = x[(int64_t)d * ld];
    const bool act = d >= s && (pres == nullptr || pres[(int64_t)d * ld] != 0);
    const bool rem = cnt >= W;                          // the oldest element leaves
    const int lo = (act && cnt > 0) ? (rem ? tail + 1 : tail) : d;
    const int lomin = tso_wave_min(lo);
    const int ro = rem ? (int)ring[cslot * 64] : 0x7fffffff;
    int sl = cslot - (rem ? W - 1 : cnt);               // slot of the oldest remaining element
    if (sl < 0) sl += W;
    int newtail = -1, below = 0;
    bool isn = xn != xn;
    double v0 = 0.0, v1 = 0.0;
    for (int db = lomin; db < d; db += 8) {
      double u[8];
      bool pu[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int dd = db + k;
        u[k] = dd < d ? x[(int64_t)dd * ld] : 0.0;
        pu[k] = dd < d && dd >= lo && (pres == nullptr || pres[(int64_t)dd * ld] != 0);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (!pu[k]) continue;
        const double uk = u[k];
        if (newtail < 0) newtail = db + k;
        int r = (int)ring[sl * 64];
        r -= (r > ro) ? 1 : 0;
        const bool ab = tso_above(uk, xn);
        r += ab ? 1 : 0;
        below += ab ? 0 : 1;
        ring[sl * 64] = (uint16_t)r;
        v0 = r == i0 ? uk : v0;
        v1 = r == i1 ? uk : v1;
        isn = isn || uk != uk;
        if (++sl == W) sl = 0;
      }
    }
    double out = qnan();
    if (act) {
      ring[cslot * 64] = (uint16_t)below;
      v0 = below == i0 ? xn : v0;
      v1 = below == i1 ? xn : v1;
      tail = newtail < 0 ? d : newtail;
      cnt += 1;
      if (++cslot == W) cslot = 0;
      if (cnt >= W && !isn) out = tso_combine(v0, v1, mode, frac);
    }
    if (d >= d0 && ok) y[(int64_t)d * ld] = out;
  }
}

// ------------------------------------------------------------------------------------
// Median / quantile for windows whose rank ring does not fit LDS.  One thread per output
// (wave = 64 assets of one (factor, date)), no state: the window's present rows are walked
// 65 times -- 64 counting passes fix the bits of the i0-th smallest key from the top (okey:
// order-preserving, -0.0 folded into +0.0), one more finds the next distinct key above it
// and how many elements sit at or below, which gives sorted[i0 + 1].  O(65 W) per output.
__global__ void __launch_bounds__(256)
k_tso_bis(const double* __restrict__ X, double* __restrict__ Y, int64_t F, int64_t D, int64_t A, int64_t ld, int W,
          const uint8_t* __restrict__ present, int64_t achunks, int i0, int mode, double frac) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t ac = wid % achunks, rest = wid / achunks;
  const int64_t dl = rest % D, f = rest / D;
  if (f >= F) return;                                   // wave-uniform
  const int d = (int)dl;
  const int64_t a = ac * 64 + lane;
  const bool ok = a < A;
  const double* x = X + f * D * ld + (ok ? a : A - 1);
  const uint8_t* pres = present ? present + (ok ? a : A - 1) : nullptr;
  const bool me = pres == nullptr || pres[(int64_t)d * ld] != 0;
  // s: the date of the W-th present row counting back from d (d itself is the first)
  int pre, s;
  tso_walk_back(pres, ld, d, W, ok && me, pre, s);
  const bool full = ok && me && pre == W - 1;
  if (__ballot(full) == 0) {                            // wave-uniform
    if (ok) Y[f * D * ld + (int64_t)d * ld + a] = qnan();
    return;
  }
  const int lo = full ? s : d;
  const int lomin = tso_wave_min(lo);
  const int need = i0 + 1;
  uint64_t K = 0;
  bool isn = false;
  for (int bit = 63; bit >= 0; --bit) {
    const uint64_t Tk = K | ((1ull << bit) - 1ull);
    int c = 0;
    for (int db = lomin; db <= d; db += 8) {
      double u[8];
      bool pu[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int dd = db + k;
        u[k] = dd <= d ? x[(int64_t)dd * ld] : 0.0;
        pu[k] = dd <= d && dd >= lo && (pres == nullptr || pres[(int64_t)dd * ld] != 0);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (!pu[k]) continue;
        isn = isn || u[k] != u[k];
        c += okey(u[k]) <= Tk ? 1 : 0;
      }
    }
    if (c < need) K |= 1ull << bit;
  }
  const double v0 = okey_inv(K);
  double v1 = v0;
  if (mode != TSO_SEL_LO) {
    int c = 0;
    uint64_t m = KEY_SENTINEL;
    for (int db = lomin; db <= d; db += 8) {
      double u[8];
      bool pu[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int dd = db + k;
        u[k] = dd <= d ? x[(int64_t)dd * ld] : 0.0;
        pu[k] = dd <= d && dd >= lo && (pres == nullptr || pres[(int64_t)dd * ld] != 0);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (!pu[k]) continue;
        const uint64_t key = okey(u[k]);
        c += key <= K ? 1 : 0;
        m = (key > K && key < m) ? key : m;
      }
    }
    if (c < need + 1) v1 = okey_inv(m);
  }
  if (ok) Y[f * D * ld + (int64_t)d * ld + a] = (full && !isn) ? tso_combine(v0, v1, mode, frac) : qnan();
}

template <int T>
static const void* tso_ext_kernel(int op) {
  switch (op) {
    case FMX_TSO_MIN: return (const void*)k_tso_ext<FMX_TSO_MIN, T>;
    case FMX_TSO_MAX: return (const void*)k_tso_ext<FMX_TSO_MAX, T>;
    case FMX_TSO_ARGMIN: return (const void*)k_tso_ext<FMX_TSO_ARGMIN, T>;
    default: return (const void*)k_tso_ext<FMX_TSO_ARGMAX, T>;
  }
}

}  // namespace fmx

using namespace fmx;

// Dispatch (no window cap):
//   min / max / argmin / argmax             -> k_tso_ext (date tiles, registers only)
//   median / quantile, W <= TSO_LDS_MAXW    -> k_tso_sel (rank ring in LDS, date segments)
//   median / quantile, longer windows       -> k_tso_bis (stateless key bisection)
// A window longer than the panel has no full window anywhere: it runs as D + 1.
extern "C" fmx_status fmx_ts_order(int32_t op, const double* X, double* Y, int64_t F, int64_t D, int64_t A,
                                   int64_t ld, int32_t window, double q, int32_t interp, const uint8_t* present,
                                   void* stream) {
  FMX_ARG(X && Y, "null panel");
  FMX_ARG(F >= 0 && D >= 0 && A >= 0 && ld >= A, "bad dims");
  FMX_ARG(op >= FMX_TSO_MIN && op <= FMX_TSO_QUANTILE, "unknown ts order op");
  FMX_ARG(window >= 1, "window must be >= 1");
  if (op == FMX_TSO_QUANTILE) {
    FMX_ARG(q >= 0.0 && q <= 1.0, "quantile must be in [0, 1]");      // false for NaN
    FMX_ARG(interp >= FMX_TSO_LINEAR && interp <= FMX_TSO_NEAREST, "unknown interpolation");
  }
  FMX_ARG(D < (int64_t)1 << 30, "too many dates for the windowed kernel");
  if (F == 0 || D == 0 || A == 0) return FMX_OK;
  hipStream_t st = as_stream(stream);
  int W = (int)std::min<int64_t>(window, D + 1);
  int64_t achunks = ceil_div(A, 64);
  if (op <= FMX_TSO_ARGMAX) {
    int64_t ntiles = ceil_div(D, TSO_T);
    const int64_t waves = F * ntiles * achunks;
    FMX_ARG(ceil_div(waves, 4) < (int64_t)1 << 31, "panel too large for one windowed launch");
    void* args[] = {(void*)&X, (void*)&Y, (void*)&F, (void*)&D, (void*)&A, (void*)&ld, (void*)&W,
                    (void*)&present, (void*)&achunks, (void*)&ntiles};
    FMX_HIP(hipLaunchKernel(tso_ext_kernel<TSO_T>(op), dim3((unsigned)ceil_div(waves, 4)), dim3(256), args, 0, st));
    return FMX_OK;
  }
  // sorted[i0] (and sorted[i0 + 1]) of the window, and how they combine: pandas' roll_median_c
  // and roll_quantile (window/aggregations.pyx), every window full (nobs = window)
  int i0, mode = TSO_SEL_LO;
  double frac = 0.0;
  if (op == FMX_TSO_MEDIAN) {
    if (window % 2) { i0 = window / 2; }
    else { i0 = window / 2 - 1; mode = TSO_SEL_MID; }
  } else {
    const double fi = q * (double)(window - 1);
    i0 = (int)fi;
    frac = fi - (double)i0;
    if (fi != (double)i0) {
      if (interp == FMX_TSO_LINEAR) mode = TSO_SEL_LIN;
      else if (interp == FMX_TSO_HIGHER) mode = TSO_SEL_HI;
      else if (interp == FMX_TSO_MIDPOINT) mode = TSO_SEL_MID;
      else if (interp == FMX_TSO_NEAREST)                              // round half to even
        mode = (frac == 0.5) ? (i0 % 2 == 0 ? TSO_SEL_LO : TSO_SEL_HI) : (frac < 0.5 ? TSO_SEL_LO : TSO_SEL_HI);
    }
  }
  if (window > D) { i0 = 0; mode = TSO_SEL_LO; }          // no output; keep the indices inside W
  if (W <= TSO_LDS_MAXW) {
    // segment length: 4 W keeps the O(W^2 / 2) warm-up at an eighth of the segment's own
    // O(L W) work; panels that would leave the device short of waves take shorter segments,
    // down to W (warm-up a half) -- the outputs do not depend on L
    const int Lmin = std::max(W, 16);
    int L = std::max(4 * W, 32);
    while (L > Lmin && F * ceil_div(D, L) * achunks < TSO_SEL_MIN_WAVES) L = std::max(L / 2, Lmin);
    int64_t nseg = ceil_div(D, L);
    const int64_t waves = F * nseg * achunks;
    FMX_ARG(waves < (int64_t)1 << 31, "panel too large for one windowed launch");
    const size_t lds = (size_t)W * 64 * sizeof(uint16_t);
    if (lds > 64 * 1024)
      FMX_HIP(hipFuncSetAttribute((const void*)k_tso_sel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* args[] = {(void*)&X, (void*)&Y, (void*)&F, (void*)&D, (void*)&A, (void*)&ld, (void*)&W, (void*)&present,
                    (void*)&achunks, (void*)&nseg, (void*)&L, (void*)&i0, (void*)&mode, (void*)&frac};
    FMX_HIP(hipLaunchKernel((const void*)k_tso_sel, dim3((unsigned)waves), dim3(64), args, lds, st));
    return FMX_OK;
  }
  const int64_t waves = F * D * achunks;
  FMX_ARG(ceil_div(waves, 4) < (int64_t)1 << 31, "panel too large for one windowed launch");
  void* args[] = {(void*)&X, (void*)&Y, (void*)&F, (void*)&D, (void*)&A, (void*)&ld, (void*)&W, (void*)&present,
                  (void*)&achunks, (void*)&i0, (void*)&mode, (void*)&frac};
  FMX_HIP(hipLaunchKernel((const void*)k_tso_bis, dim3((unsigned)ceil_div(waves, 4)), dim3(256), args, 0, st));
  return FMX_OK;
}
