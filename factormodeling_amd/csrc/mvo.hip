// Mean-variance factor selection (factor_selection_methods.py:60-175) for J rolling windows
// at once: the window's mean / Ledoit-Wolf covariance (stage A) and the box- and
// budget-constrained QP (stage B, ADMM) each run as one workgroup per window.
//
//   max_w  mu'w - gamma w'Sigma w - tau |w - p|_1    s.t.  sum w = 1, 0 <= w <= u
//
// Stage A (k_mvo_cov): mu, the ddof=1 sample covariance S, the constant-correlation target
// T, the shrinkage intensity lambda and Sigma = lambda T + (1 - lambda) S, in the operation
// order of the host ledoit_wolf_shrinkage.  The reference's per-observation
// sum_k |rc_k rc_k' - S|_F^2 is taken in its closed form sum_k |rc_k|^4 - (n - 2) |S|_F^2.
//
// Stage B (k_mvo_admm): ADMM on x (quadratic + budget) / z (box + L1) with the scaled dual y.
//   K = 2 gamma Sigma + rho I is inverted once (symmetric sweep = Gauss-Jordan without
//   pivoting, every pivot a Schur-complement diagonal of the SPD K); K^-1 and K^-1 1 stay
//   resident -- in LDS for F <= MVO_LDS_F, else in the window's workspace slot (L2 / MALL).
//   x = K^-1 b - nu K^-1 1,  b = mu + rho (z - y),  nu = ((K^-1 1)'b - 1) / (1'K^-1 1)
//   z = clip(p + soft(x + y - p, tau / rho), 0, u),  y += x - z
//   stop when |x - z|_inf <= eps, |sum z - 1| <= eps / 10 and rho |z - z_prev|_inf <= eps.
//   rho = sqrt(l_min l_max) of 2 gamma Sigma: l_max by power iteration, l_min by the Rayleigh
//   quotient after power iteration on (c I - Sigma), floored at 1e-2 l_max (singular Sigma).
// All arithmetic is plain fp64 (fma); no fast-math, no cooperative launch, <= 16 waves.
#include "fmx_common.hpp"

namespace fmx {

constexpr int MVO_MAX_F = 256;   // same cap as the fused Gram (FUSED_GRAM_MAX_F)
constexpr int MVO_LDS_F = 128;   // K^-1 in LDS up to here (128 KiB), streamed from the workspace above
constexpr int MVO_POWER_ITERS = 32;
constexpr double MVO_RATIO_FLOOR = 1e-2;   // rho >= 0.1 l_max(2 gamma Sigma)
constexpr int MVO_RED = 48;      // one reduction buffer: 16 waves x 3 values

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// Workgroup reduction of (sum a, max b, max c) in two halves around a barrier the caller
// owns: red_put, __syncthreads(), red_get.  Two buffers alternate (buf), so the next put
// needs no barrier of its own after this get.
__device__ __forceinline__ void red_put(double* red, int buf, double a, double b, double c) {
  a = wave_sum(a);
  b = wave_max(b);
  c = wave_max(c);
  if ((threadIdx.x & 63) == 0) {
    double* r = red + buf * MVO_RED + (threadIdx.x >> 6) * 3;
    r[0] = a;
    r[1] = b;
    r[2] = c;
  }
}
__device__ __forceinline__ void red_get(const double* red, int buf, double& a, double& b, double& c) {
  const int nw = (blockDim.x + 63) >> 6;
  const double* r = red + buf * MVO_RED;
  a = r[0];
  b = r[1];
  c = r[2];
  for (int w = 1; w < nw; ++w) {
    a += r[3 * w];
    b = fmax(b, r[3 * w + 1]);
    c = fmax(c, r[3 * w + 2]);
  }
}
__device__ __forceinline__ double block_sum(double* red, int& buf, double v) {
  double b = 0.0, c = 0.0;
  red_put(red, buf, v, 0.0, 0.0);
  __syncthreads();
  red_get(red, buf, v, b, c);
  buf ^= 1;
  return v;
}

__device__ __forceinline__ bool finite_(double v) {
  return (((uint32_t)__double2hiint(v) >> 20) & 0x7ffu) != 0x7ffu;
}

// ---------------------------------------------------------------------------------- stage A
// One workgroup per window.  mu [J][F], cov [J][F][F], lam [J]; status [J] (may be NULL):
// 0 ok, 2 rejected (bad bounds, n < 2, or a non-finite return in the window) -- a rejected
// window's mu / cov / lam are NaN.
__global__ __launch_bounds__(1024) void k_mvo_cov(const double* __restrict__ fret, int64_t D, int F,
                                                  const int32_t* __restrict__ d0, const int32_t* __restrict__ d1,
                                                  int use_shrinkage, double* __restrict__ mu, double* __restrict__ cov,
                                                  double* __restrict__ lam, int32_t* __restrict__ status) {
  __shared__ double mean[MVO_MAX_F];
  __shared__ double sd[MVO_MAX_F];
  __shared__ double red[2 * MVO_RED];
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t a = d0[j], b = d1[j];
  double* muj = mu + j * F;
  double* S = cov + j * (int64_t)F * F;
  const int FF = F * F;
  int buf = 0;

  const bool range_ok = a >= 0 && b <= D && b - a >= 2;
  const int n = range_ok ? (int)(b - a) : 0;
  const double* R = fret + (range_ok ? a : 0) * F;   // the window's rows: n * F contiguous doubles
  int bad = range_ok ? 0 : 1;
  if (tid < F) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) {
      const double v = R[(int64_t)k * F + tid];
      bad |= !finite_(v);
      s += v;
    }
    mean[tid] = s / (double)(n > 0 ? n : 1);
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    for (int i = tid; i < FF; i += T) S[i] = qnan();
    if (tid < F) muj[tid] = qnan();
    if (tid == 0) {
      lam[j] = qnan();
      if (status) status[j] = 2;
    }
    return;
  }
  if (tid < F) muj[tid] = mean[tid];

  // S = rc'rc / (n - 1); each thread owns the entries idx = tid, tid + T, ...
  const double rdof = 1.0 / (double)(n - 1);
  double ss = 0.0;   // |S|_F^2
  for (int idx = tid; idx < FF; idx += T) {
    const int i = idx / F, c = idx - i * F;
    const double mi = mean[i], mc = mean[c];
    double acc = 0.0;
    for (int k = 0; k < n; ++k) acc = __builtin_fma(R[(int64_t)k * F + i] - mi, R[(int64_t)k * F + c] - mc, acc);
    const double s = acc * rdof;
    S[idx] = s;
    ss = __builtin_fma(s, s, ss);
    if (i == c) sd[i] = sqrt(s);
  }
  __syncthreads();
  if (!use_shrinkage) {
    if (tid == 0) {
      lam[j] = 0.0;
      if (status) status[j] = 0;
    }
    return;
  }
  ss = block_sum(red, buf, ss);

  // sum_k |rc_k|^4: a wave per observation
  double q4 = 0.0;
  {
    const int lane = tid & 63, nw = T >> 6;
    for (int k = tid >> 6; k < n; k += nw) {
      double q = 0.0;
      for (int f = lane; f < F; f += 64) {
        const double r = R[(int64_t)k * F + f] - mean[f];
        q = __builtin_fma(r, r, q);
      }
      q = wave_sum(q);
      if (lane == 0) q4 = __builtin_fma(q, q, q4);
    }
  }
  q4 = block_sum(red, buf, q4);

  // mean correlation over the pairs i < c with both sigmas > 0
  double cs = 0.0, cn = 0.0;
  for (int idx = tid; idx < FF; idx += T) {
    const int i = idx / F, c = idx - i * F;
    if (i < c && sd[i] > 0.0 && sd[c] > 0.0) {
      cs += S[idx] / (sd[i] * sd[c]);
      cn += 1.0;
    }
  }
  cs = block_sum(red, buf, cs);
  cn = block_sum(red, buf, cn);
  const double mcorr = cn > 0.0 ? cs / cn : 0.0;

  // d = |S - T|_F^2, T_ic = (mcorr sd_i) sd_c, T_ii = S_ii
  double dd = 0.0;
  for (int idx = tid; idx < FF; idx += T) {
    const int i = idx / F, c = idx - i * F;
    if (i != c) {
      const double e = S[idx] - (mcorr * sd[i]) * sd[c];
      dd = __builtin_fma(e, e, dd);
    }
  }
  dd = block_sum(red, buf, dd);
  const double x = ((q4 - (double)(n - 2) * ss) / (double)n) / dd;
  double l = (x < 1.0) ? x : 1.0;   // Python's min(1, x): 1 for inf / nan
  l = (l > 0.0) ? l : 0.0;          // max(0, .)
  for (int idx = tid; idx < FF; idx += T) {
    const int i = idx / F, c = idx - i * F;
    const double s = S[idx];
    const double t = (i == c) ? s : (mcorr * sd[i]) * sd[c];
    S[idx] = l * t + (1.0 - l) * s;
  }
  if (tid == 0) {
    lam[j] = l;
    if (status) status[j] = 0;
  }
}

// ---------------------------------------------------------------------------------- stage B
// t = M v for a symmetric M [F][F] (row-major, read down its columns so that consecutive
// lanes read consecutive words) and v in LDS: the workgroup is P slices of C = roundup(F, 64)
// lanes, slice g sums its share of the rows, thread i < F adds the P partials.  The caller
// has written v and passed a barrier; one barrier inside.
__device__ __forceinline__ double sym_matvec(const double* M, const double* v, double* part, int F, int C, int P) {
  const int tid = threadIdx.x;
  const int g = tid / C, i = tid - g * C;
  if (g < P) {
    double acc = 0.0;
    if (i < F) {
      const int per = (F + P - 1) / P;
      const int r0 = g * per, r1 = min(F, r0 + per);
#pragma unroll 4
      for (int r = r0; r < r1; ++r) acc = __builtin_fma(M[r * F + i], v[r], acc);
    }
    part[g * C + i] = acc;
  }
  __syncthreads();
  double t = 0.0;
  if (tid < F)
    for (int q = 0; q < P; ++q) t += part[q * C + tid];
  return t;
}

template <bool LDSK>
__global__ __launch_bounds__(1024) void k_mvo_admm(const double* __restrict__ mu, double* __restrict__ cov,
                                                   const double* __restrict__ lam,
                                                   const int32_t* __restrict__ status, int F, double gamma,
                                                   double u, double tau, const double* __restrict__ prev,
                                                   int max_iter, double eps, double* __restrict__ w_out,
                                                   double* __restrict__ info) {
  extern __shared__ double sm[];
  double* vec = sm;                      // [MVO_MAX_F]
  double* part = vec + MVO_MAX_F;        // [1024]
  double* red = part + 1024;             // [2 * MVO_RED]
  double* Kl = red + 2 * MVO_RED;        // [F * F] when LDSK
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, T = blockDim.x;
  const int C = (F + 63) & ~63, P = T / C;
  const int FF = F * F;
  double* A = cov + j * (int64_t)FF;     // Sigma, then (F > MVO_LDS_F) K and K^-1 in place
  double* Kinv = LDSK ? Kl : A;
  double* wj = w_out + j * F;
  double* inf = info + j * 6;
  const bool own = tid < F;
  int buf = 0;

  // rejected by stage A, or no w in the box sums to one (F u < 1: cvxpy reports the problem
  // infeasible and the reference falls back to zeros)
  if (status[j] != 0 || !(u * (double)F >= 1.0 - 1e-12)) {
    if (own) wj[tid] = 0.0;
    if (tid == 0) {
      inf[0] = 2.0;
      inf[1] = inf[2] = inf[3] = inf[5] = 0.0;
      inf[4] = lam[j];
    }
    return;
  }

  // Sigma <- (Sigma + Sigma') / 2, in place (each thread owns whole pairs)
  for (int idx = tid; idx < FF; idx += T) {
    const int i = idx / F, c = idx - i * F;
    if (i < c) {
      const double s = 0.5 * (A[idx] + A[c * F + i]);
      A[idx] = s;
      A[c * F + i] = s;
    }
  }
  __syncthreads();

  // l_max of Sigma: power iteration from a positive start
  double v = own ? 1.0 + 0.01 * (double)((tid * 37) % 11) : 0.0;
  double lmax = 0.0;
  for (int it = 0; it < MVO_POWER_ITERS; ++it) {
    if (own) vec[tid] = v;
    __syncthreads();
    const double t = sym_matvec(A, vec, part, F, C, P);
    const double vv = block_sum(red, buf, v * v);
    const double tt = block_sum(red, buf, t * t);
    lmax = vv > 0.0 ? sqrt(tt / vv) : 0.0;
    v = tt > 0.0 ? t / sqrt(tt) : 0.0;
  }
  // l_min of Sigma: power iteration on (c I - Sigma) from a sign-mixed start, then the
  // Rayleigh quotient of Sigma there (an upper estimate of l_min, within a small factor)
  const double shift = 1.05 * lmax;
  v = own ? (((tid * 2654435761u) >> 16) & 1u ? 1.0 : -1.0) * (1.0 + 0.1 * (double)(tid % 7)) : 0.0;
  double lmin = 0.0;
  for (int it = 0; it <= MVO_POWER_ITERS; ++it) {
    if (own) vec[tid] = v;
    __syncthreads();
    const double t = sym_matvec(A, vec, part, F, C, P);
    const double vv = block_sum(red, buf, v * v);
    const double vt = block_sum(red, buf, v * t);
    lmin = vv > 0.0 ? vt / vv : 0.0;
    const double w = __builtin_fma(shift, v, -t);
    const double ww = block_sum(red, buf, w * w);
    v = ww > 0.0 ? w / sqrt(ww) : 0.0;
  }
  // rho = sqrt(l_min l_max) of 2 gamma Sigma, the ratio l_min / l_max floored at MVO_RATIO_FLOOR:
  // along (near-)null directions of Sigma the problem is linear and a small rho oscillates
  const double g2 = 2.0 * gamma;
  const double ratio = (lmax > 0.0 && lmin > MVO_RATIO_FLOOR * lmax) ? lmin / lmax : MVO_RATIO_FLOOR;
  double rho = g2 * lmax * sqrt(ratio);
  if (!(rho > 0.0) || !finite_(rho)) rho = 1.0;

  // K = 2 gamma Sigma + rho I
  for (int idx = tid; idx < FF; idx += T) {
    const int i = idx / F, c = idx - i * F;
    Kinv[idx] = g2 * A[idx] + (i == c ? rho : 0.0);
  }
  __syncthreads();
  // symmetric sweep on every pivot: K <- -K^-1
  const int sg = tid / C, sc = tid - sg * C;
  int notpd = 0;
  for (int k = 0; k < F; ++k) {
    if (own) vec[tid] = Kinv[k * F + tid];
    __syncthreads();
    const double piv = vec[k];
    if (!(piv > 0.0) || !finite_(piv)) {   // uniform: every thread reads the same word
      notpd = 1;
      break;
    }
    const double ip = 1.0 / piv;
    if (sg < P && sc < F) {
      const double cj = vec[sc];
      for (int i = sg; i < F; i += P) {
        const double ci = vec[i];
        double nv;
        if (i == k)
          nv = (sc == k) ? -ip : cj * ip;
        else if (sc == k)
          nv = ci * ip;
        else
          nv = __builtin_fma(-ci * ip, cj, Kinv[i * F + sc]);
        Kinv[i * F + sc] = nv;
      }
    }
    __syncthreads();
  }
  if (notpd) {
    if (own) wj[tid] = 0.0;
    if (tid == 0) {
      inf[0] = 2.0;
      inf[1] = inf[2] = inf[3] = 0.0;
      inf[4] = lam[j];
      inf[5] = rho;
    }
    return;
  }
  for (int idx = tid; idx < FF; idx += T) Kinv[idx] = -Kinv[idx];
  if (own) vec[tid] = 1.0;
  __syncthreads();
  const double k1 = sym_matvec(Kinv, vec, part, F, C, P);   // K^-1 1
  const double k11 = block_sum(red, buf, k1);

  const double mui = own ? mu[j * F + tid] : 0.0;
  const bool l1 = tau > 0.0 && prev != nullptr;
  const double pi = (own && l1) ? prev[tid] : 0.0;
  const double kappa = l1 ? tau / rho : 0.0;
  double z = own ? 1.0 / (double)F : 0.0, y = 0.0;
  double rp = 0.0, rd = 0.0;
  int it = 0, st = 1;
  while (it < max_iter) {
    ++it;
    const double bi = own ? mui + rho * (z - y) : 0.0;
    if (own) vec[tid] = bi;
    red_put(red, buf, k1 * bi, 0.0, 0.0);
    __syncthreads();
    const double t = sym_matvec(Kinv, vec, part, F, C, P);
    double s, e0, e1;
    red_get(red, buf, s, e0, e1);
    buf ^= 1;
    const double nu = (s - 1.0) / k11;
    double zs = 0.0, ep = 0.0, ed = 0.0;
    if (own) {
      const double x = __builtin_fma(-nu, k1, t);
      const double xv = x + y;
      double dlt = xv - pi;
      dlt = dlt > kappa ? dlt - kappa : (dlt < -kappa ? dlt + kappa : 0.0);
      double zn = pi + dlt;
      zn = zn < 0.0 ? 0.0 : (zn > u ? u : zn);
      ep = fabs(x - zn);
      ed = rho * fabs(zn - z);
      y = xv - zn;
      z = zn;
      zs = zn;
    }
    red_put(red, buf, zs, ep, ed);
    __syncthreads();
    red_get(red, buf, zs, rp, rd);
    buf ^= 1;
    // the budget error moves the objective at first order (by the budget multiplier), the
    // split error |x - z| only through Sigma: the budget is held to eps / 10
    const double eb = fabs(zs - 1.0);
    const bool done = rp <= eps && eb <= 0.1 * eps && rd <= eps;
    rp = fmax(rp, eb);
    if (done) {
      st = 0;
      break;
    }
  }
  if (own) wj[tid] = z;
  if (tid == 0) {
    inf[0] = (double)st;
    inf[1] = (double)it;
    inf[2] = rp;
    inf[3] = rd;
    inf[4] = lam[j];
    inf[5] = rho;
  }
}

static int mvo_cov_threads(int64_t F) { return F * F <= 4096 ? 256 : 1024; }
static int mvo_admm_threads(int64_t F) { return F <= 64 ? 256 : (F <= 128 ? 512 : 1024); }

static fmx_status mvo_check(const double* fret, int64_t D, int64_t F, const int32_t* d0, const int32_t* d1, int64_t J) {
  FMX_ARG(fret && d0 && d1, "null pointer");
  FMX_ARG(D >= 0 && J >= 0, "bad dims");
  FMX_ARG(F >= 2 && F <= MVO_MAX_F, "mvo: 2 <= F <= 256");
  FMX_ARG(J <= 0x7fffffff, "mvo: too many windows");
  return FMX_OK;
}

}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_mvo_covariance(const double* fret, int64_t D, int64_t F, const int32_t* d0_dev,
                                         const int32_t* d1_dev, int64_t J, int32_t use_shrinkage, double* mu_out,
                                         double* cov_out, double* lam_out, void* stream) {
  fmx_status st = mvo_check(fret, D, F, d0_dev, d1_dev, J);
  if (st != FMX_OK) return st;
  FMX_ARG(mu_out && cov_out && lam_out, "null pointer");
  if (J == 0) return FMX_OK;
  k_mvo_cov<<<(unsigned)J, mvo_cov_threads(F), 0, as_stream(stream)>>>(fret, D, (int)F, d0_dev, d1_dev, use_shrinkage,
                                                                      mu_out, cov_out, lam_out, nullptr);
  FMX_LAUNCH_CHECK("k_mvo_cov");
  return FMX_OK;
}

// workspace: mu [J][F] | Sigma / K^-1 [J][F][F] | lambda [J] | status int32 [J] (8-byte padded)
extern "C" int64_t fmx_mvo_windows_work_bytes(int64_t D, int64_t F, int64_t J) {
  (void)D;
  if (F < 0 || J < 0) return 0;
  return 8 * (J * F + J * F * F + J + (J + 1) / 2);
}

extern "C" fmx_status fmx_mvo_windows(const double* fret, int64_t D, int64_t F, const int32_t* d0_dev,
                                      const int32_t* d1_dev, int64_t J, double risk_aversion, double max_weight,
                                      double turnover_penalty, const double* prev, int32_t use_shrinkage,
                                      int32_t max_iter, double eps, double* w_out, double* info, void* work,
                                      int64_t work_bytes, void* stream) {
  fmx_status st = mvo_check(fret, D, F, d0_dev, d1_dev, J);
  if (st != FMX_OK) return st;
  FMX_ARG(w_out && info, "null pointer");
  FMX_ARG(risk_aversion >= 0.0 && risk_aversion == risk_aversion, "mvo: risk_aversion must be >= 0");
  FMX_ARG(max_weight == max_weight && turnover_penalty == turnover_penalty, "mvo: NaN parameter");
  FMX_ARG(max_iter >= 1 && eps > 0.0, "mvo: max_iter >= 1 and eps > 0");
  if (J == 0) return FMX_OK;
  FMX_ARG(work && work_bytes >= fmx_mvo_windows_work_bytes(D, F, J), "mvo: workspace too small");
  double* mu = (double*)work;
  double* cov = mu + J * F;
  double* lam = cov + J * F * F;
  int32_t* status = (int32_t*)(lam + J);
  const double u = max_weight < 1.0 ? max_weight : 1.0;
  hipStream_t s = as_stream(stream);
  k_mvo_cov<<<(unsigned)J, mvo_cov_threads(F), 0, s>>>(fret, D, (int)F, d0_dev, d1_dev, use_shrinkage, mu, cov, lam,
                                                       status);
  FMX_LAUNCH_CHECK("k_mvo_cov");
  const bool ldsk = F <= MVO_LDS_F;
  const size_t lds = sizeof(double) * (MVO_MAX_F + 1024 + 2 * MVO_RED + (ldsk ? (size_t)(F * F) : 0));
  const void* fn = ldsk ? (const void*)k_mvo_admm<true> : (const void*)k_mvo_admm<false>;
  if (lds > 64 * 1024) FMX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const double* mu_c = mu;
  const double* lam_c = lam;
  const int32_t* status_c = status;
  int Fi = (int)F, mi = max_iter;
  void* args[] = {(void*)&mu_c, (void*)&cov, (void*)&lam_c, (void*)&status_c, (void*)&Fi,    (void*)&risk_aversion,
                  (void*)&u,    (void*)&turnover_penalty,   (void*)&prev,     (void*)&mi,    (void*)&eps,
                  (void*)&w_out, (void*)&info};
  FMX_HIP(hipLaunchKernel(fn, dim3((unsigned)J), dim3(mvo_admm_threads(F)), args, lds, s));
  return FMX_OK;
}
