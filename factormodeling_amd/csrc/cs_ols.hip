// Per-date multi-factor OLS (fmx_cs_ols): one workgroup per (y column, date) regresses the
// date's valid rows of Y[f] on K columns of X (optionally weighted, optionally with an
// intercept) and writes beta / alpha / r2 / n / resid / fitted.  Builder-defined (the
// reference has no multi-regressor cross-sectional regression); DESIGN §19 holds the
// specification, which is written so that the result is defined under collinearity:
// centred columns, a Gram scaled to unit diagonal, and an in-order Cholesky that drops a
// column whose pivot falls under 1e-10 (as R's lm drops aliased columns).
//
// Phases of a workgroup:
//   1. validity flags of the row (coalesced), then the valid positions compacted in asset
//      order into LDS (uint16);
//   2. weighted means (and, for the constant-column test, the uncentred second moments): the
//      compacted rows staged in LDS chunk by chunk, thread (column, residue class of the rows)
//      sums its rows in row order, the classes of a column are added in class order;
//   3. the rows staged again, centred; every thread owns one 4x4 tile of the (K + 1) x (K + 1)
//      lower triangle (the y column is the last row) and one residue class of the rows, and
//      keeps its 16 partial sums in registers over all chunks; the classes of a tile are then
//      added in class order.  Both orders depend on (K, n) only, never on the batch or the
//      launch.  (Means by block_pw_sum straight from global memory -- 2K + 3 gathered passes
//      with dependent loads and eight barriers each -- made the kernel 1.2x to 2.7x slower:
//      DESIGN §19.)
//   4. scaling, Cholesky with the right-hand side as an extra row, and the back
//      substitution by wave 0 in LDS;
//   5. a last pass over X writes fitted / resid and sums the weighted squared residuals.
#include "rowkit.hpp"

namespace fmx {

constexpr int OLS_NT = 256;
constexpr int OLS_MAXK = 32;
constexpr int OLS_MAXA = 16384;
constexpr int OLS_MS = OLS_MAXK + 2;           // row stride of the LDS matrix (K + 1 rows used)
constexpr int OLS_STAGE = 5120;                // doubles of the staging area (40 KB)
constexpr double OLS_PIVOT_MIN = 1e-10;
constexpr double OLS_CONST_REL = 1e-13;

__device__ __forceinline__ bool ols_finite(double v) { return fabs(v) < __builtin_inf(); }
// LDS traffic of one wave is in order; this makes a step's stores visible to the next step.
// (the wave barrier is a convergent scheduling fence: no code moves across it or into a branch)
__device__ __forceinline__ void ols_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

struct OlsArgs {
  const double* Y;        // [Fy][D][ld]
  const double* X;        // [K][D][ld]
  const double* W;        // [D][ld] or null
  const uint8_t* present; // [D][ld] or null
  double* beta;           // [Fy][D][K] or null
  double* alpha;          // [Fy][D] or null
  double* r2;             // [Fy][D] or null
  int32_t* nout;          // [Fy][D] or null
  double* resid;          // [Fy][D][ld] or null
  double* fitted;         // [Fy][D][ld] or null
  int64_t D, A, ld, d0;
  int Fy, K, intercept;
};

__global__ void __launch_bounds__(OLS_NT) k_cs_ols(OlsArgs p) {
  extern __shared__ double lds[];
  const int K = p.K, Kp = K + 1, Kq = (Kp + 3) & ~3, RS = Kq + 1;   // RS: staged row stride (w first)
  const int64_t A = p.A;
  double* stage = lds;                         // [OLS_STAGE]: flags / staged rows / tile partials
  double* M = stage + OLS_STAGE;               // [OLS_MS][OLS_MS]
  double* mean = M + OLS_MS * OLS_MS;          // [36] x means, [K] = y mean
  double* sc = mean + 36;                      // [36] s_k = sqrt(G_kk)
  double* sw2 = sc + 36;                       // [36] sum w x_k^2 (uncentred)
  double* bet = sw2 + 36;                      // [36] coefficients (0 at dropped columns)
  double* red = bet + 36;                      // [16]
  int* iscr = (int*)(red + 16);                // [16]
  int* kept = iscr + 16;                       // [36]
  uint16_t* pos = (uint16_t*)(kept + 36);      // [A]
  uint8_t* flags = (uint8_t*)stage;            // [A] (A <= 16384 < 8 * OLS_STAGE)

  const int tid = threadIdx.x;
  const int f = blockIdx.x;
  const int64_t d = p.d0 + blockIdx.y;
  const int64_t row = d * p.ld, fstride = p.D * p.ld;
  const double* y = p.Y + (int64_t)f * fstride + row;
  const double* x0 = p.X + row;                // column k at x0 + k * fstride
  const double* w = p.W ? p.W + row : nullptr;
  const uint8_t* prow = p.present ? p.present + row : nullptr;
  double* ores = p.resid ? p.resid + (int64_t)f * fstride + row : nullptr;
  double* ofit = p.fitted ? p.fitted + (int64_t)f * fstride + row : nullptr;
  const int64_t fd = (int64_t)f * p.D + d;

  // ---- 1. validity and compaction
  for (int64_t a = tid; a < A; a += OLS_NT) {
    bool ok = (prow ? prow[a] != 0 : true) && ols_finite(y[a]);
    if (ok && w) { const double wv = w[a]; ok = ols_finite(wv) && wv > 0.0; }
    for (int k = 0; k < K; ++k) ok &= ols_finite(x0[k * fstride + a]);   // branch-free: the loads overlap
    flags[a] = ok;
    if (ores) ores[a] = qnan();
    if (ofit) ofit[a] = qnan();
  }
  __syncthreads();
  const int64_t C = (A + OLS_NT - 1) / OLS_NT;
  const int64_t a0 = min<int64_t>(A, tid * C), a1 = min<int64_t>(A, a0 + C);
  int cnt = 0;
  for (int64_t a = a0; a < a1; ++a) cnt += flags[a];
  int n;
  int base = block_exscan<OLS_NT>(cnt, iscr, &n);
  for (int64_t a = a0; a < a1; ++a)
    if (flags[a]) pos[base++] = (uint16_t)a;
  __syncthreads();
  if (tid == 0 && p.nout) p.nout[fd] = n;
  if (n < K + p.intercept) {
    if (tid < K && p.beta) p.beta[fd * K + tid] = qnan();
    if (tid == 0) {
      if (p.alpha) p.alpha[fd] = qnan();
      if (p.r2) p.r2[fd] = qnan();
    }
    return;
  }

  // ---- 2. weighted means and uncentred second moments of the K + 1 columns (x_0.., y)
  // The raw rows are staged chunk by chunk; thread (column c, class sl) sums the rows of its
  // residue class in row order, and the classes are then added in class order.
  const int CH = OLS_STAGE / RS;
  auto stage_chunk = [&](int c0, int cn) {     // rows [c0, c0 + cn) minus mean[] -> stage[i][0..RS)
    // eight elements per thread and step: the eight global loads are issued before the first
    // LDS store waits for one (one load per step left the kernel waiting on memory latency)
    const int tot = cn * RS;
    for (int e0 = tid; e0 < tot; e0 += 8 * OLS_NT) {
      double v[8], m[8];
      int off[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = min(e0 + u * OLS_NT, tot - 1);   // clamped: in bounds, stored only if e is real
        const int kk = e / cn, i = e - kk * cn;        // column kk of the staged row: 0 = w, 1.. = z
        const int a = pos[c0 + i];
        off[u] = i * RS + kk;
        if (kk == 0) { v[u] = w ? w[a] : 1.0; m[u] = 0.0; }
        else if (kk <= K) { v[u] = x0[(kk - 1) * fstride + a]; m[u] = mean[kk - 1]; }
        else if (kk == Kp) { v[u] = y[a]; m[u] = mean[K]; }
        else { v[u] = 0.0; m[u] = 0.0; }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (e0 + u * OLS_NT < tot) stage[off[u]] = v[u] - m[u];
    }
  };
  if (tid <= K) {
    mean[tid] = 0.0;
    sw2[tid] = 0.0;
  }
  __syncthreads();
  if (p.intercept) {
    const int nsl = OLS_NT / Kp, c = tid % Kp, sl = tid / Kp;
    const bool mact = sl < nsl;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int c0 = 0; c0 < n; c0 += CH) {
      const int cn = min(CH, n - c0);
      stage_chunk(c0, cn);
      __syncthreads();
      if (mact) {
        for (int i = (sl + nsl - (c0 % nsl)) % nsl; i < cn; i += nsl) {
          const double wi = stage[i * RS], v = stage[i * RS + 1 + c], wv = wi * v;
          s0 += wi;
          s1 += wv;
          s2 += wv * v;
        }
      }
      __syncthreads();
    }
    if (mact) {
      double* q = stage + (sl * Kp + c) * 3;
      q[0] = s0; q[1] = s1; q[2] = s2;
    }
    __syncthreads();
    if (tid < Kp) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
      for (int j = 0; j < nsl; ++j) {
        const double* q = stage + (j * Kp + tid) * 3;
        t0 += q[0]; t1 += q[1]; t2 += q[2];
      }
      mean[tid] = t1 / t0;
      sw2[tid] = t2;
    }
    __syncthreads();
  }

  // ---- 3. Gram of the centred columns: G[j][k] = sum_i w_i z_ij z_ik, z = [xc_0..xc_{K-1}, yc]
  const int nt4 = Kq >> 2, ntile = nt4 * (nt4 + 1) / 2, nslice = OLS_NT / ntile;
  const int tl = tid % ntile, slice = tid / ntile;
  const bool gact = slice < nslice;
  int ta = 0;
  while ((ta + 1) * (ta + 2) / 2 <= tl) ++ta;
  const int tb = tl - ta * (ta + 1) / 2;       // ta >= tb: the lower triangle
  double acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int cn = min(CH, n - c0);
    stage_chunk(c0, cn);
    __syncthreads();
    if (gact) {
      // rows of residue class `slice` (mod nslice) of the compacted row, whatever the chunking
      const int i0 = (slice + nslice - (c0 % nslice)) % nslice;
      for (int i = i0; i < cn; i += nslice) {
        const double* r = stage + i * RS;
        const double wi = r[0];
        double za[4], zb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { za[q] = wi * r[1 + 4 * ta + q]; zb[q] = r[1 + 4 * tb + q]; }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[q * 4 + s] += za[q] * zb[s];
      }
    }
    __syncthreads();
  }
  if (gact) {
#pragma unroll
    for (int e = 0; e < 16; ++e) stage[(slice * ntile + tl) * 16 + e] = acc[e];
  }
  __syncthreads();
  for (int q = tid; q < ntile * 16; q += OLS_NT) {
    const int t = q >> 4, e = q & 15;
    double s = 0.0;
    for (int sl = 0; sl < nslice; ++sl) s += stage[(sl * ntile + t) * 16 + e];
    int qa = 0;
    while ((qa + 1) * (qa + 2) / 2 <= t) ++qa;
    const int qb = t - qa * (qa + 1) / 2;
    const int r = 4 * qa + (e >> 2), c = 4 * qb + (e & 3);
    if (r <= K && c <= r) M[r * OLS_MS + c] = s;
  }
  __syncthreads();

  // ---- 4. scaling, in-order Cholesky with dropping, back substitution
  if (tid < K) {
    const double s = sqrt(M[tid * OLS_MS + tid]);
    bool drop = !(s > 0.0);                                           // zero (or NaN) scale
    if (p.intercept && s <= OLS_CONST_REL * sqrt(sw2[tid])) drop = true;  // a constant column
    sc[tid] = s;
    kept[tid] = !drop;
  }
  if (tid == K) sc[K] = 1.0;
  __syncthreads();
  const double sst = M[K * OLS_MS + K];
  for (int q = tid; q < Kp * K; q += OLS_NT) {
    const int r = q / K, c = q - r * K;
    if (c <= r) M[r * OLS_MS + c] = M[r * OLS_MS + c] / (sc[r] * sc[c]);
  }
  __syncthreads();
  if (tid < 64) {
    const int r = tid;                         // lane r owns row r of the factor; row K is the rhs
    for (int k = 0; k < K; ++k) {
      const double piv = M[k * OLS_MS + k];
      const bool keep = kept[k] && piv >= OLS_PIVOT_MIN;
      ols_wave_sync();
      if (!keep) {
        if (r == 0) kept[k] = 0;
        continue;
      }
      const double lkk = sqrt(piv);
      if (r >= k && r <= K) M[r * OLS_MS + k] = r == k ? lkk : M[r * OLS_MS + k] / lkk;
      ols_wave_sync();
      if (r > k && r <= K) {
        const double lrk = M[r * OLS_MS + k];
        const int cend = min(r, K - 1);
        for (int c = k + 1; c <= cend; ++c) M[r * OLS_MS + c] -= lrk * M[c * OLS_MS + k];
      }
      ols_wave_sync();
    }
    // L^T b = z with z in row K; kept columns only
    for (int k = K - 1; k >= 0; --k) {
      if (!kept[k]) {
        if (r == 0) bet[k] = 0.0;
        continue;
      }
      const double bk = M[K * OLS_MS + k] / M[k * OLS_MS + k];
      ols_wave_sync();
      if (r < k) M[K * OLS_MS + r] -= M[k * OLS_MS + r] * bk;
      if (r == 0) bet[k] = bk / sc[k];
      ols_wave_sync();
    }
  }
  __syncthreads();
  double alpha = qnan();
  if (p.intercept) {
    alpha = mean[K];
    for (int k = 0; k < K; ++k)
      if (kept[k]) alpha -= bet[k] * mean[k];
  }
  if (tid < K && p.beta) p.beta[fd * K + tid] = kept[tid] ? bet[tid] : qnan();
  if (tid == 0 && p.alpha) p.alpha[fd] = alpha;
  if (!ores && !ofit && !p.r2) return;

  // ---- 5. fitted values, residuals, weighted squared residuals
  const double ybar = mean[K];
  double ssr = 0.0;
  for (int i = tid; i < n; i += OLS_NT) {
    const int a = pos[i];
    double fit = ybar;
    for (int k = 0; k < K; ++k) fit += bet[k] * (x0[k * fstride + a] - mean[k]);   // bet = 0 where dropped
    const double res = y[a] - fit;
    if (ofit) ofit[a] = fit;
    if (ores) ores[a] = res;
    ssr += (w ? w[a] : 1.0) * res * res;
  }
  if (p.r2) {
    ssr = block_sum<OLS_NT>(ssr, red);
    if (tid == 0) p.r2[fd] = sst == 0.0 ? qnan() : 1.0 - ssr / sst;
  }
}

static size_t ols_lds_bytes(int64_t A) {
  return (size_t)(OLS_STAGE + OLS_MS * OLS_MS + 4 * 36 + 16) * 8 + (16 + 36) * 4 + (size_t)A * 2 + 16;
}

}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_cs_ols(const double* Y, const double* X, const double* W, const uint8_t* present,
                                 int64_t Fy, int64_t K, int64_t D, int64_t A, int64_t ld, int32_t intercept,
                                 double* beta, double* alpha, double* r2, int32_t* n, double* resid, double* fitted,
                                 void* stream) {
  FMX_ARG(Y && X, "cs_ols: null panel");
  FMX_ARG(Fy >= 0 && D >= 0 && A >= 0 && ld >= A, "cs_ols: bad dims");
  FMX_ARG(K >= 1 && K <= OLS_MAXK, "cs_ols: the number of regressors K must be in 1..32");
  FMX_ARG(A <= OLS_MAXA, "cs_ols: rows longer than 16384 assets are not supported");
  FMX_ARG(Fy <= 65535, "cs_ols: more than 65535 y columns in one call");
  FMX_ARG(intercept == 0 || intercept == 1, "cs_ols: intercept must be 0 or 1");
  if (Fy == 0 || D == 0 || A == 0) return FMX_OK;
  OlsArgs p;
  p.Y = Y; p.X = X; p.W = W; p.present = present;
  p.beta = beta; p.alpha = alpha; p.r2 = r2; p.nout = n; p.resid = resid; p.fitted = fitted;
  p.D = D; p.A = A; p.ld = ld;
  p.Fy = (int)Fy; p.K = (int)K; p.intercept = intercept;
  const size_t lds = ols_lds_bytes(A);
  if (lds > 64 * 1024)
    FMX_HIP(hipFuncSetAttribute((const void*)k_cs_ols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // y columns fastest: the Fy workgroups of a date read the same K rows of X out of L2
  for (int64_t d0 = 0; d0 < D; d0 += 32768) {
    p.d0 = d0;
    const int64_t nd = std::min<int64_t>(32768, D - d0);
    hipLaunchKernelGGL(k_cs_ols, dim3((unsigned)Fy, (unsigned)nd), dim3(OLS_NT), lds, as_stream(stream), p);
    FMX_LAUNCH_CHECK("k_cs_ols");
  }
  return FMX_OK;
}
