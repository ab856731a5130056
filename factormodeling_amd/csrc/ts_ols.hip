// Rolling multi-factor OLS (fmx_ts_ols): for every (y column f, asset a, date d) the least
// squares of the column's last W valid rows ending at d on K regressors, per-symbol
// ([K][D][ld]) or shared by all symbols ([K][D], e.g. factor returns).  Builder-defined (the
// reference's rolling regression has one regressor and raw moments); DESIGN §22 holds the
// specification.  The fit is cs_ols's with unit weights: means, columns centred
// in a second pass, the Gram scaled to unit diagonal, an in-order Cholesky that drops a
// column under the same three rules, every sum over the window oldest row first.
//
// One thread per output.  The 64 lanes of a wave are 64 consecutive assets of one date (a
// window row is one coalesced 512-B access per regressor), the waves of a workgroup are
// consecutive dates of the same assets (their windows overlap: the re-reads hit in cache).
//   0. k_ts_ols_valid writes one validity byte per (f, d, a), so the walks test a byte
//      and not K + 1 doubles;
//   1. walk back from d over the column's validity bytes to the window's oldest row t0;
//   2. rows [min t0 of the wave, d] forward, wave-uniform (so the lanes stay on one row and
//      the shared table is read through the scalar unit), each lane using its own rows:
//      pass 1 the means, pass 2 the centred Gram / g / SST in registers;
//   3. scaling, Cholesky with the right-hand side as an extra row, both substitutions:
//      fully unrolled, static indices, branch-free (a dropped column is zeroed, not skipped);
//   4. fitted / resid at row d; pass 3 over the window for SSR when r2 or sigma is wanted.
#include <algorithm>

#include "fmx_common.hpp"

namespace fmx {

constexpr int TSO_MAXK = 8;
constexpr int TSO_WAVES = 4;                   // dates per workgroup
constexpr double TSO_PIVOT_MIN = 1e-10;        // DESIGN §19's constants
constexpr double TSO_CONST_REL = 1e-13;

__device__ __forceinline__ bool tso_finite(double v) { return fabs(v) < __builtin_inf(); }

struct TsOlsArgs {
  const double* Y;        // [Fy][D][ld]
  const double* X;        // [K][D][ld], or [K][D] when shared
  const uint8_t* present; // [D][ld] or null
  uint8_t* valid;         // [Fy][D][ld] work
  double* beta;           // [Fy][K][D][ld] or null
  double* alpha;          // [Fy][D][ld] or null, like every output below
  double* fitted;
  double* resid;
  double* r2;
  double* sigma;
  int64_t D, A, ld, d0;
  int W, intercept;
};

template <int K, bool SHARED>
__global__ void __launch_bounds__(256) k_ts_ols_valid(TsOlsArgs p) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t d = p.d0 + blockIdx.y;
  const int64_t f = blockIdx.z;
  if (a >= p.A) return;
  const int64_t row = d * p.ld + a, fstride = p.D * p.ld;
  bool ok = (p.present ? p.present[row] != 0 : true) && tso_finite(p.Y[f * fstride + row]);
#pragma unroll
  for (int k = 0; k < K; ++k) ok &= tso_finite(SHARED ? p.X[k * p.D + d] : p.X[k * fstride + row]);
  p.valid[f * fstride + row] = ok;
}

template <int K, bool SHARED>
__global__ void __launch_bounds__(64 * TSO_WAVES) k_ts_ols(TsOlsArgs p) {
  constexpr int Kp = K + 1;                    // row K of M is the right-hand side (y)
  const int64_t ld = p.ld, fstride = p.D * ld;
  const int64_t f = blockIdx.z;
  // a wave is one row of the 64 x TSO_WAVES block: its date is uniform (readfirstlane tells the compiler)
  const int64_t d = p.d0 + (int64_t)blockIdx.y * TSO_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int64_t a_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (d >= p.D) return;                        // a whole wave
  const bool lane_on = a_raw < p.A;
  const int64_t a = lane_on ? a_raw : p.A - 1; // idle lanes read a real column, store nothing
  const int W = p.W;
  const uint8_t* vcol = p.valid + f * fstride + a;          // row t at vcol[t * ld]
  const double* ycol = p.Y + f * fstride + a;
  const double* xcol = SHARED ? p.X : p.X + a;              // regressor k, row t: see xat()
  auto xat = [&](int k, int64_t t) -> double {
    return SHARED ? xcol[(int64_t)k * p.D + t] : xcol[(int64_t)k * fstride + t * ld];
  };

  // ---- 1. the window's oldest row: the W-th valid row counting back from d (eight bytes a step)
  int64_t t0 = d;
  bool ok = lane_on && vcol[d * ld] != 0;
  {
    int cnt = 1;
    int64_t base = d;                          // rows below base are not scanned yet
    while (ok && cnt < W && base > 0) {
      uint8_t b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t tt = base - 1 - u;
        b[u] = tt >= 0 ? vcol[tt * ld] : (uint8_t)0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (cnt < W && b[u]) { ++cnt; t0 = base - 1 - u; }
      base -= 8;
    }
    ok = ok && cnt >= W;
  }
  const int64_t off = f * fstride + d * ld + a;
  if (!ok) t0 = d + 1;                         // an empty window: the lane idles through the passes
  // the wave walks rows [tlo, d]: tlo = the smallest t0 of its lanes
  int tmin = (int)t0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) tmin = min(tmin, __shfl_xor(tmin, m, 64));
  const int64_t tlo = __builtin_amdgcn_readfirstlane(tmin);

  // ---- 2a. means (and the uncentred second moments for the constant-column test)
  double mean[Kp], sw2[K];
#pragma unroll
  for (int k = 0; k < Kp; ++k) mean[k] = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) sw2[k] = 0.0;
  if (p.intercept) {
    for (int64_t t = tlo; t <= d; ++t) {
      const bool use = t >= t0 && vcol[t * ld] != 0;
      double v[Kp];
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = xat(k, t);
      v[K] = ycol[t * ld];
      if (use) {
#pragma unroll
        for (int k = 0; k < Kp; ++k) mean[k] += v[k];
#pragma unroll
        for (int k = 0; k < K; ++k) sw2[k] += v[k] * v[k];
      }
    }
    const double n = (double)W;
#pragma unroll
    for (int k = 0; k < Kp; ++k) mean[k] = mean[k] / n;
  }

  // ---- 2b. Gram of the centred columns, lower triangle; row K = g, M[K][K] = SST
  double M[Kp][Kp];
#pragma unroll
  for (int r = 0; r < Kp; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) M[r][c] = 0.0;
  for (int64_t t = tlo; t <= d; ++t) {
    const bool use = t >= t0 && vcol[t * ld] != 0;
    double z[Kp];
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = xat(k, t) - mean[k];
    z[K] = ycol[t * ld] - mean[K];
    if (use) {
#pragma unroll
      for (int r = 0; r < Kp; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) M[r][c] += z[r] * z[c];
    }
  }
  const double sst = M[K][K];

  // ---- 3. scaling to unit diagonal, in-order Cholesky with dropping, back substitution
  double sc[K];
  bool kept[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = sqrt(M[k][k]);
    bool drop = !(s > 0.0);                                              // zero (or NaN) scale
    if (p.intercept && s <= TSO_CONST_REL * sqrt(sw2[k])) drop = true;   // a constant column
    sc[k] = s;
    kept[k] = !drop;
  }
#pragma unroll
  for (int r = 0; r < Kp; ++r)
#pragma unroll
    for (int c = 0; c <= r && c < K; ++c) {
      const double q = M[r][c] / ((r < K ? sc[r] : 1.0) * sc[c]);
      // a dropped column leaves the system: its row and column are zero, not 0 / 0
      M[r][c] = (kept[c] && (r == K || kept[r])) ? q : 0.0;
    }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double piv = M[k][k];
    const bool keep = kept[k] && piv >= TSO_PIVOT_MIN;
    kept[k] = keep;
    const double lkk = keep ? sqrt(piv) : 1.0;
    M[k][k] = lkk;
#pragma unroll
    for (int c = 0; c < k; ++c) M[k][c] = keep ? M[k][c] : 0.0;
#pragma unroll
    for (int r = k + 1; r < Kp; ++r) M[r][k] = keep ? M[r][k] / lkk : 0.0;
#pragma unroll
    for (int r = k + 1; r < Kp; ++r) {
      const double lrk = M[r][k];
#pragma unroll
      for (int c = k + 1; c <= r && c < K; ++c) M[r][c] -= lrk * M[c][k];
    }
  }
  double bet[K];                               // 0 at dropped columns
  int nkept = 0;
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    const double bk = M[K][k] / M[k][k];       // L^T b = z, z in row K
#pragma unroll
    for (int r = 0; r < k; ++r) M[K][r] -= M[k][r] * bk;
    bet[k] = kept[k] ? bk / sc[k] : 0.0;
    nkept += kept[k];
  }
  double alpha = qnan();
  if (p.intercept) {
    alpha = mean[K];
#pragma unroll
    for (int k = 0; k < K; ++k) alpha -= bet[k] * mean[k];
  }

  // ---- 4. the row's own fitted value and residual; SSR over the window
  double fit = mean[K];
#pragma unroll
  for (int k = 0; k < K; ++k) fit += bet[k] * (xat(k, d) - mean[k]);
  const double res = ycol[d * ld] - fit;
  double r2 = qnan(), sigma = qnan();
  if (p.r2 || p.sigma) {
    double ssr = 0.0;
    for (int64_t t = tlo; t <= d; ++t) {
      const bool use = t >= t0 && vcol[t * ld] != 0;
      double ft = mean[K];
#pragma unroll
      for (int k = 0; k < K; ++k) ft += bet[k] * (xat(k, t) - mean[k]);
      const double rt = ycol[t * ld] - ft;
      if (use) ssr += rt * rt;
    }
    if (sst != 0.0) r2 = 1.0 - ssr / sst;
    const int dof = W - (nkept + p.intercept);
    if (dof > 0) sigma = sqrt(ssr / (double)dof);
  }

  if (!lane_on) return;
  const double nan = qnan();
  if (p.beta) {
#pragma unroll
    for (int k = 0; k < K; ++k)
      p.beta[((f * K + k) * p.D + d) * ld + a] = (ok && kept[k]) ? bet[k] : nan;
  }
  if (p.alpha) p.alpha[off] = ok ? alpha : nan;
  if (p.fitted) p.fitted[off] = ok ? fit : nan;
  if (p.resid) p.resid[off] = ok ? res : nan;
  if (p.r2) p.r2[off] = ok ? r2 : nan;
  if (p.sigma) p.sigma[off] = ok ? sigma : nan;
}

template <int K, bool SHARED>
static fmx_status ts_ols_launch(TsOlsArgs p, int64_t Fy, hipStream_t s) {
  for (int64_t d0 = 0; d0 < p.D; d0 += 32768) {
    p.d0 = d0;
    const int64_t nd = std::min<int64_t>(32768, p.D - d0);
    hipLaunchKernelGGL((k_ts_ols_valid<K, SHARED>), dim3((unsigned)ceil_div(p.A, 256), (unsigned)nd, (unsigned)Fy),
                       dim3(256), 0, s, p);
    FMX_LAUNCH_CHECK("k_ts_ols_valid");
  }
  // every validity byte is written before any window is walked (same stream)
  for (int64_t d0 = 0; d0 < p.D; d0 += 32768 * TSO_WAVES) {
    p.d0 = d0;
    const int64_t nd = std::min<int64_t>(32768 * TSO_WAVES, p.D - d0);
    hipLaunchKernelGGL((k_ts_ols<K, SHARED>),
                       dim3((unsigned)ceil_div(p.A, 64), (unsigned)ceil_div(nd, TSO_WAVES), (unsigned)Fy),
                       dim3(64, TSO_WAVES), 0, s, p);
    FMX_LAUNCH_CHECK("k_ts_ols");
  }
  return FMX_OK;
}

template <int K>
static fmx_status ts_ols_k(const TsOlsArgs& p, int64_t Fy, bool shared, hipStream_t s) {
  return shared ? ts_ols_launch<K, true>(p, Fy, s) : ts_ols_launch<K, false>(p, Fy, s);
}

}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_ts_ols(const double* Y, const double* X, const uint8_t* present, int64_t Fy, int64_t K,
                                 int64_t D, int64_t A, int64_t ld, int32_t window, int32_t intercept, int32_t shared,
                                 double* beta, double* alpha, double* fitted, double* resid, double* r2,
                                 double* sigma, uint8_t* work, void* stream) {
  FMX_ARG(Y && X, "ts_ols: null panel");
  FMX_ARG(Fy >= 0 && D >= 0 && D < ((int64_t)1 << 31) && A >= 0 && ld >= A, "ts_ols: bad dims");   // rows are int
  FMX_ARG(K >= 1 && K <= TSO_MAXK, "ts_ols: the number of regressors K must be in 1..8");
  FMX_ARG(intercept == 0 || intercept == 1, "ts_ols: intercept must be 0 or 1");
  FMX_ARG(shared == 0 || shared == 1, "ts_ols: shared must be 0 or 1");
  FMX_ARG((int64_t)window >= K + intercept, "ts_ols: the window is shorter than the number of coefficients");
  FMX_ARG(Fy <= 65535, "ts_ols: more than 65535 y columns in one call");
  if (Fy == 0 || D == 0 || A == 0) return FMX_OK;
  FMX_ARG(work, "ts_ols: null work buffer (Fy * D * ld bytes)");
  TsOlsArgs p;
  p.Y = Y; p.X = X; p.present = present; p.valid = work;
  p.beta = beta; p.alpha = alpha; p.fitted = fitted; p.resid = resid; p.r2 = r2; p.sigma = sigma;
  p.D = D; p.A = A; p.ld = ld; p.d0 = 0;
  p.W = window; p.intercept = intercept;
  hipStream_t s = as_stream(stream);
  switch ((int)K) {
    case 1: return ts_ols_k<1>(p, Fy, shared, s);
    case 2: return ts_ols_k<2>(p, Fy, shared, s);
    case 3: return ts_ols_k<3>(p, Fy, shared, s);
    case 4: return ts_ols_k<4>(p, Fy, shared, s);
    case 5: return ts_ols_k<5>(p, Fy, shared, s);
    case 6: return ts_ols_k<6>(p, Fy, shared, s);
    case 7: return ts_ols_k<7>(p, Fy, shared, s);
    default: return ts_ols_k<8>(p, Fy, shared, s);
  }
}
