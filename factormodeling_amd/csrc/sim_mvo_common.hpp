// The shared parts of the MVO book solvers.  Every device function is called by all threads of
// the workgroup, owns the barriers it names and keeps one operation order, so a kernel built
// from these pieces gives the same bits as the text it replaced (-ffp-contract=off).
//
// Users: S = k_sim_mvo (sim_mvo.hip), U = k_smt_setup and C = k_smt_chain (sim_mvo_turnover.hip),
// R = k_risk_mvo (sim_mvo_risk.hip).
//
//   smv_carve                        the LDS layout                                     S U C R
//   smv_put / get / sum3 / sum       workgroup reductions                               S U C R
//   smv_signs                        the day's legs                                     S U C R
//   smv_window_setup                 column means, delta, sc2, centred Gram, l_max,
//     (smv_col_means, _diag_sum,     rho, M^-1 = (c/2 I + sc2 C C')^-1                  S U
//      _gram, _lmax, _rho, _sweep)   (C: the means; R: l_max, rho and the sweep)
//   smv_kapply, SmvApply             the Woodbury apply of K^-1 = (2 Sigma + rho I)^-1   S C
//   smv_leg_system<Apply>, SmvLegs   p+-, the 2 x 2 system of the leg multipliers       S C R
//     (smv_uniform)                  (its four values travel in scalar registers)
//   smv_admm<Apply>                  the ADMM loop on the signed box                    S R
//   smv_stop                         the stop rule and the reported residuals           S C R
//   smv_write_row, smv_write_info    a date's row, counts and info                      S C R
//   smv_rowdot<CLEAN>                one wave's dot with a panel row (CLEAN: R)         S U C R
//
// C keeps its own loop (an over-relaxed z-step around the previous book, a fifth reduced value)
// around smv_stop.  risk_model.hip takes smv_wsum and smv_finite from here.
// Host side, for the three fmx_*_books entry points: smv_threads and SMV_KERNEL (the block size
// and the EPT instantiation), smv_launch, smv_check_windows.
#pragma once
#include <string>
#include <vector>

#include "fmx_common.hpp"

namespace fmx {

constexpr int SMV_MAX_A = 16384;
constexpr int SMV_MAX_T = 64;
constexpr int SMV_POWER_ITERS = 32;
constexpr double SMV_RATIO_FLOOR = 1e-3;   // rho >= 0.032 l_max(2 Sigma); DESIGN 14
constexpr int SMV_RED = 64;                // one reduction buffer: 16 waves x 4 values
constexpr int SMV_SMALL = 2 * SMV_MAX_T + 2 * SMV_RED + SMV_MAX_T / 2;   // gv, hv, red, rows (in doubles)
constexpr size_t SMV_LDS_MAX = 160 * 1024;

namespace {

__device__ __forceinline__ double smv_wsum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double smv_wmax(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// Workgroup reduction of (sum a, sum b, f(c), f(d)), f = sum or max, in two halves around a
// barrier the caller owns.  Two buffers alternate, so the next put needs no barrier of its own.
template <bool MAXCD>
__device__ __forceinline__ void smv_put(double* red, int buf, double a, double b, double c, double d) {
  a = smv_wsum(a);
  b = smv_wsum(b);
  c = MAXCD ? smv_wmax(c) : smv_wsum(c);
  d = MAXCD ? smv_wmax(d) : smv_wsum(d);
  if ((threadIdx.x & 63) == 0) {
    double* r = red + buf * SMV_RED + (threadIdx.x >> 6) * 4;
    r[0] = a;
    r[1] = b;
    r[2] = c;
    r[3] = d;
  }
}
template <bool MAXCD>
__device__ __forceinline__ void smv_get(const double* red, int buf, double& a, double& b, double& c, double& d) {
  const int nw = blockDim.x >> 6;
  const double* r = red + buf * SMV_RED;
  a = r[0];
  b = r[1];
  c = r[2];
  d = r[3];
  for (int w = 1; w < nw; ++w) {
    a += r[4 * w];
    b += r[4 * w + 1];
    c = MAXCD ? fmax(c, r[4 * w + 2]) : c + r[4 * w + 2];
    d = MAXCD ? fmax(d, r[4 * w + 3]) : d + r[4 * w + 3];
  }
}
__device__ __forceinline__ void smv_sum3(double* red, int& buf, double& a, double& b, double& c) {
  double d = 0.0;
  smv_put<false>(red, buf, a, b, c, 0.0);
  __syncthreads();
  smv_get<false>(red, buf, a, b, c, d);
  buf ^= 1;
}
__device__ __forceinline__ double smv_sum(double* red, int& buf, double a) {
  double b = 0.0, c = 0.0;
  smv_sum3(red, buf, a, b, c);
  return a;
}

__device__ __forceinline__ bool smv_finite(double v) {
  return (((uint32_t)__double2hiint(v) >> 20) & 0x7ffu) != 0x7ffu;
}

// dot of the LDS vector vec [A] with the panel row r [A], by one wave (every lane gets it).
// CLEAN: a non-finite cell of r reads as 0.  The two variants keep the load order each had as a
// function of its own (CLEAN: the four cells ahead of the LDS reads): either order for both moves
// the other kernels' register allocation (k_smt_chain's scratch at 1 and 2 elements per thread).
template <bool CLEAN>
__device__ __forceinline__ double smv_clean(double v) {
  return !CLEAN || smv_finite(v) ? v : 0.0;
}
template <bool CLEAN = false>
__device__ __forceinline__ double smv_rowdot(const double* vec, const double* __restrict__ r, int A) {
  const int lane = threadIdx.x & 63;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int a = lane;
  for (; a + 192 < A; a += 256) {
    if constexpr (CLEAN) {
      const double r0 = r[a], r1 = r[a + 64], r2 = r[a + 128], r3 = r[a + 192];
      a0 = __builtin_fma(vec[a], smv_clean<true>(r0), a0);
      a1 = __builtin_fma(vec[a + 64], smv_clean<true>(r1), a1);
      a2 = __builtin_fma(vec[a + 128], smv_clean<true>(r2), a2);
      a3 = __builtin_fma(vec[a + 192], smv_clean<true>(r3), a3);
    } else {
      a0 = __builtin_fma(vec[a], r[a], a0);
      a1 = __builtin_fma(vec[a + 64], r[a + 64], a1);
      a2 = __builtin_fma(vec[a + 128], r[a + 128], a2);
      a3 = __builtin_fma(vec[a + 192], r[a + 192], a3);
    }
  }
  for (; a < A; a += 64) a0 = __builtin_fma(vec[a], smv_clean<CLEAN>(r[a]), a0);
  return smv_wsum((a0 + a1) + (a2 + a3));
}

// The dynamic LDS of every kernel here: the A-vector, two T-vectors, two reduction buffers, the
// window's rows, then the kernel's own tail (M^-1, the K x K matrices, the chain's buffers).
struct SmvLds {
  double* vec;    // [A]
  double* gv;     // [SMV_MAX_T]
  double* hv;     // [SMV_MAX_T]
  double* red;    // [2 * SMV_RED]
  int* rows;      // [SMV_MAX_T]
  double* tail;   // sm + A + SMV_SMALL
};
__device__ __forceinline__ SmvLds smv_carve(double* sm, int A) {
  double* gv = sm + A;
  double* red = gv + 2 * SMV_MAX_T;
  return {sm, gv, gv + SMV_MAX_T, red, (int*)(red + 2 * SMV_RED), sm + A + SMV_SMALL};
}

// The workgroup's view of one date: the panel, the window's rows and the LDS pieces.
struct SmvDay {
  const double* R0;   // [Dr][A]
  int A, T;
  int* rows;          // [T] window rows of R0 (LDS)
  double* vec;        // [A]
  double* gv;         // [SMV_MAX_T]
  double* hv;         // [SMV_MAX_T]
  double* red;        // [2 * SMV_RED]
  double* M;          // [T * T], LDS or workspace
  int buf;            // the reduction buffer in turn
};

// sg: +1 / -1 on the legs, 0 elsewhere; pr: the symbol has a row on this date
template <int EPT>
__device__ __forceinline__ void smv_signs(const double* __restrict__ xj, const uint8_t* __restrict__ pj, int A,
                                          int (&sg)[EPT], bool (&pr)[EPT], double& cp, double& cn, double& cr) {
  const int tid = threadIdx.x, NT = blockDim.x;
  cp = 0.0;
  cn = 0.0;
  cr = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = tid + e * NT;
    sg[e] = 0;
    pr[e] = false;
    if (a < A) {
      pr[e] = !pj || pj[a];
      const double xv = xj[a];
      if (pr[e]) sg[e] = xv > 0.0 ? 1 : (xv < 0.0 ? -1 : 0);
      cr += pr[e] ? 1.0 : 0.0;
      cp += sg[e] > 0 ? 1.0 : 0.0;
      cn += sg[e] < 0 ? 1.0 : 0.0;
    }
  }
}

// m: the window's column means
template <int EPT>
__device__ __forceinline__ void smv_col_means(const SmvDay& d, double (&m)[EPT]) {
  const int tid = threadIdx.x, NT = blockDim.x;
  double acc[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
  for (int k = 0; k < d.T; ++k) {
    const double* r = d.R0 + (int64_t)d.rows[k] * d.A;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < d.A) acc[e] += r[a];
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) m[e] = acc[e] / (double)d.T;
}

// this thread's share of sum over present columns of sum_k (r_k[a] - m[a])^2
template <int EPT>
__device__ __forceinline__ double smv_diag_sum(const SmvDay& d, const double (&m)[EPT], const bool (&pr)[EPT]) {
  const int tid = threadIdx.x, NT = blockDim.x;
  double acc[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
  for (int k = 0; k < d.T; ++k) {
    const double* r = d.R0 + (int64_t)d.rows[k] * d.A;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < d.A && pr[e]) {
        const double c = r[a] - m[e];
        acc[e] = __builtin_fma(c, c, acc[e]);
      }
    }
  }
  double dsum = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) dsum += acc[e];
  return dsum;
}

// centred Gram over the active columns into d.M: G_kl = sum_a c_k[a] (X_l[a] - m[a])
template <int EPT>
__device__ __forceinline__ void smv_gram(SmvDay& d, const double (&m)[EPT], const int (&sg)[EPT]) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
  const int T = d.T, A = d.A;
  for (int k = 0; k < T; ++k) {
    const double* r = d.R0 + (int64_t)d.rows[k] * A;
    double mu = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) {
        const double c = sg[e] != 0 ? r[a] - m[e] : 0.0;
        d.vec[a] = c;
        mu = __builtin_fma(c, m[e], mu);
      }
    }
    mu = smv_sum(d.red, d.buf, mu);   // barrier inside: vec is complete
    for (int l = wv; l <= k; l += nw) {
      const double v = smv_rowdot(d.vec, d.R0 + (int64_t)d.rows[l] * A, A) - mu;
      if (lane == 0) {
        d.M[k * T + l] = v;
        d.M[l * T + k] = v;
      }
    }
    __syncthreads();
  }
}

// l_max of the Gram in d.M: power iteration from a positive start
__device__ __forceinline__ double smv_lmax(SmvDay& d) {
  const int tid = threadIdx.x, T = d.T;
  const bool own = tid < T;
  double lmax = 0.0;
  double v = own ? 1.0 + 0.01 * (double)((tid * 37) % 11) : 0.0;
  for (int it = 0; it < SMV_POWER_ITERS; ++it) {
    if (own) d.hv[tid] = v;
    __syncthreads();
    double t = 0.0;
    if (own)
      for (int r = 0; r < T; ++r) t = __builtin_fma(d.M[r * T + tid], d.hv[r], t);
    double vv = v * v, tt = t * t, z0 = 0.0;
    smv_sum3(d.red, d.buf, vv, tt, z0);
    lmax = vv > 0.0 ? sqrt(tt / vv) : 0.0;
    v = tt > 0.0 ? t / sqrt(tt) : 0.0;
  }
  return lmax;
}

// d.M (the Gram G) <- M = c/2 I + sc2 G, inverted in place by a symmetric sweep on every pivot
// (M <- -M^-1).  Returns nonzero when rho or a pivot is not a positive finite number; d.M is
// then unusable.  The caller negates d.M after a zero return.
__device__ __forceinline__ int smv_sweep(SmvDay& d, double c, double sc2, double rho) {
  const int tid = threadIdx.x, NT = blockDim.x, T = d.T;
  const bool own = tid < T;
  double* M = d.M;
  const int TT = T * T;
  for (int idx = tid; idx < TT; idx += NT) {
    const int i = idx / T;
    M[idx] = sc2 * M[idx] + (idx - i * T == i ? 0.5 * c : 0.0);
  }
  __syncthreads();
  int bad = !(rho > 0.0) || !smv_finite(rho);
  for (int k = 0; k < T && !bad; ++k) {
    if (own) d.hv[tid] = M[k * T + tid];
    __syncthreads();
    const double piv = d.hv[k];
    if (!(piv > 0.0) || !smv_finite(piv)) {   // uniform: every thread reads the same word
      bad = 1;
      break;
    }
    const double ip = 1.0 / piv;
    for (int idx = tid; idx < TT; idx += NT) {
      const int i = idx / T, cc = idx - i * T;
      const double ci = d.hv[i], cj = d.hv[cc];
      double nv;
      if (i == k)
        nv = (cc == k) ? -ip : cj * ip;
      else if (cc == k)
        nv = ci * ip;
      else
        nv = __builtin_fma(-ci * ip, cj, M[idx]);
      M[idx] = nv;
    }
    __syncthreads();
  }
  return bad;
}

// out = K^-1 v on the active columns (v is zero elsewhere); t1 = pp'v, t2 = pn'v.  d.M holds M^-1.
template <int EPT>
__device__ __forceinline__ void smv_kapply(SmvDay& d, const double (&v)[EPT], double (&out)[EPT], double& t1, double& t2,
                                           const double (&pp)[EPT], const double (&pn)[EPT], const double (&m)[EPT],
                                           const int (&sg)[EPT], double sc2, double rc) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
  const int T = d.T, A = d.A;
  const bool own = tid < T;
  double mv = 0.0;
  t1 = 0.0;
  t2 = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = tid + e * NT;
    if (a < A) {
      d.vec[a] = v[e];
      mv = __builtin_fma(m[e], v[e], mv);
      t1 = __builtin_fma(pp[e], v[e], t1);
      t2 = __builtin_fma(pn[e], v[e], t2);
    }
  }
  smv_sum3(d.red, d.buf, mv, t1, t2);   // barrier inside: vec is complete
  for (int k = wv; k < T; k += nw) {
    const double dd = smv_rowdot(d.vec, d.R0 + (int64_t)d.rows[k] * A, A);
    if (lane == 0) d.gv[k] = dd - mv;
  }
  __syncthreads();
  double h = 0.0;
  if (own) {
    for (int r = 0; r < T; ++r) h = __builtin_fma(d.M[r * T + tid], d.gv[r], h);
    d.hv[tid] = h;
  }
  const double hs = smv_sum(d.red, d.buf, h);   // barrier inside: hv is complete
  double acc[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
  for (int k = 0; k < T; ++k) {
    const double* r = d.R0 + (int64_t)d.rows[k] * A;
    const double hk = d.hv[k];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A && sg[e] != 0) acc[e] = __builtin_fma(r[a], hk, acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const double ct = __builtin_fma(-m[e], hs, acc[e]);
    out[e] = sg[e] != 0 ? __builtin_fma(-sc2, ct, v[e]) * rc : 0.0;
  }
}

// v when every lane of the wave holds the same v, as a scalar-register value
__device__ __forceinline__ double smv_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// smv_kapply as the callable smv_leg_system and smv_admm take
template <int EPT>
struct SmvApply {
  SmvDay& d;
  const double (&m)[EPT];
  const int (&sg)[EPT];
  double sc2, rc;
  __device__ __forceinline__ void operator()(const double (&v)[EPT], double (&out)[EPT], double& t1, double& t2,
                                             const double (&pp)[EPT], const double (&pn)[EPT]) const {
    smv_kapply<EPT>(d, v, out, t1, t2, pp, pn, m, sg, sc2, rc);
  }
};

// The 2 x 2 system of the leg multipliers: [e+'p+  e+'p-; e-'p+  e-'p-] nu = (p+'b - 1, p-'b + 1)
struct SmvLegs {
  double a11, a12, a22, rdet;
  __device__ __forceinline__ void nu(double t1, double t2, double& nup, double& nun) const {
    const double r1 = t1 - 1.0, r2 = t2 + 1.0;
    nup = (r1 * a22 - r2 * a12) * rdet;
    nun = (a11 * r2 - a12 * r1) * rdet;
  }
};

// p+ = K^-1 e+, p- = K^-1 e- (apply: out = K^-1 v, t1 = pp'v, t2 = pn'v) and their 2 x 2 system
template <int EPT, class Apply>
__device__ __forceinline__ SmvLegs smv_leg_system(const Apply& apply, double* red, int& buf, const int (&sg)[EPT],
                                                  double (&pp)[EPT], double (&pn)[EPT]) {
#pragma unroll
  for (int e = 0; e < EPT; ++e) pp[e] = pn[e] = 0.0;
  double t1, t2;
  {
    double ev[EPT], o1[EPT], o2[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) ev[e] = sg[e] > 0 ? 1.0 : 0.0;
    apply(ev, o1, t1, t2, pp, pn);
#pragma unroll
    for (int e = 0; e < EPT; ++e) ev[e] = sg[e] < 0 ? 1.0 : 0.0;
    apply(ev, o2, t1, t2, pp, pn);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      pp[e] = o1[e];
      pn[e] = o2[e];
    }
  }
  double a11 = 0.0, a12 = 0.0, a22 = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    a11 += sg[e] > 0 ? pp[e] : 0.0;
    a12 += sg[e] > 0 ? pn[e] : 0.0;
    a22 += sg[e] < 0 ? pn[e] : 0.0;
  }
  smv_sum3(red, buf, a11, a12, a22);
  // every lane holds the same four values: scalar registers carry them through the loop
  return {smv_uniform(a11), smv_uniform(a12), smv_uniform(a22), smv_uniform(1.0 / (a11 * a22 - a12 * a12))};
}

// rho = sqrt(l_lo l_hi), the ends of 2 Sigma's spectrum, with the ratio floored
__device__ __forceinline__ double smv_rho(double l_lo, double l_hi) {
  const double ratio = l_lo > SMV_RATIO_FLOOR * l_hi ? l_lo / l_hi : SMV_RATIO_FLOOR;
  return l_hi * sqrt(ratio);
}

// The window of one date, from its rows to M^-1 in d.M: column means m, delta and sc2 (the
// shrunk sample covariance is delta I + sc2 C'C), the centred Gram, rho, the sweep.  Returns
// nonzero for a window the solver has no answer to (a non-finite return: x0, :451-459); d.M is
// then unusable.  No barrier after the last write of d.M: a caller that reads it owns that one.
template <int EPT>
__device__ __forceinline__ int smv_window_setup(SmvDay& d, const int32_t* __restrict__ wrows, const int (&sg)[EPT],
                                                const bool (&pr)[EPT], double npres, double shrink, double (&m)[EPT],
                                                double& delta, double& sc2, double& rho) {
  const int tid = threadIdx.x, T = d.T;
  if (tid < T) d.rows[tid] = wrows[tid];
  __syncthreads();
  smv_col_means<EPT>(d, m);
  double dsum = smv_diag_sum<EPT>(d, m, pr);
  dsum = smv_sum(d.red, d.buf, dsum);
  const double avg_var = dsum / ((double)(T - 1) * npres) + 1e-6;
  const double q = shrink > 0.0 ? 1.0 - shrink : 1.0;
  delta = q * 1e-6 + (shrink > 0.0 ? shrink * avg_var : 0.0);
  sc2 = q / (double)(T - 1);
  smv_gram<EPT>(d, m, sg);
  rho = smv_rho(2.0 * delta, 2.0 * delta + 2.0 * sc2 * smv_lmax(d));
  if (smv_sweep(d, 2.0 * delta + rho, sc2, rho)) return 1;
  for (int idx = tid; idx < T * T; idx += blockDim.x) d.M[idx] = -d.M[idx];
  return 0;
}

// The stop rule, after the reduction.  In: rp = |x - z|_inf, rd = rho |z - z_prev|_inf, the leg
// sums sp / sn and the gradient scale gs.  A leg-sum error moves the objective at first order (by
// the leg's multiplier), the split error |x - z| only through Sigma: the legs are held to
// eps / 10.  Out: rp and rd as info reports them.
__device__ __forceinline__ bool smv_stop(double sp, double sn, double gs, double eps, double& rp, double& rd) {
  const double eb = fmax(fabs(sp - 1.0), fabs(sn + 1.0));
  const bool done = rp <= eps && eb <= 0.1 * eps && rd <= eps * gs;
  rp = fmax(rp, eb);
  rd = gs > 0.0 ? rd / gs : rd;
  return done;
}

// ADMM on x (quadratic + the two leg budgets, through apply and the leg system) / z (the signed
// box [0, u] / [-u, 0]) from the equal-leg x0, at most max_iter rounds.  z is the last iterate;
// st 0 converged, 1 max_iter reached; rp / rd as smv_stop leaves them.
template <int EPT, class Apply>
__device__ __forceinline__ void smv_admm(const Apply& apply, double* red, int& buf, const int (&sg)[EPT],
                                         const double (&pp)[EPT], const double (&pn)[EPT], const SmvLegs& lg,
                                         double npos, double nneg, double rho, double u, int max_iter, double eps,
                                         double (&z)[EPT], int& st, int& it, double& rp, double& rd) {
  double y[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    z[e] = sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0);
    y[e] = 0.0;
  }
  rp = 0.0;
  rd = 0.0;
  it = 0;
  st = 1;
  while (it < max_iter) {
    ++it;
    double b[EPT], kb[EPT], t1, t2, nup, nun;
#pragma unroll
    for (int e = 0; e < EPT; ++e) b[e] = sg[e] != 0 ? rho * (z[e] - y[e]) : 0.0;
    apply(b, kb, t1, t2, pp, pn);
    lg.nu(t1, t2, nup, nun);
    double sp = 0.0, sn = 0.0, ep = 0.0, ed = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if (sg[e] != 0) {
        const double x = __builtin_fma(-nun, pn[e], __builtin_fma(-nup, pp[e], kb[e]));
        const double xv = x + y[e];
        const double lo = sg[e] > 0 ? 0.0 : -u, hi = sg[e] > 0 ? u : 0.0;
        const double zn = xv < lo ? lo : (xv > hi ? hi : xv);
        ep = fmax(ep, fabs(x - zn));
        ed = fmax(ed, rho * fabs(zn - z[e]));
        y[e] = xv - zn;
        z[e] = zn;
        sp += sg[e] > 0 ? zn : 0.0;
        sn += sg[e] < 0 ? zn : 0.0;
      }
    }
    smv_put<true>(red, buf, sp, sn, ep, ed);
    __syncthreads();
    smv_get<true>(red, buf, sp, sn, rp, rd);
    buf ^= 1;
    if (smv_stop(sp, sn, fmax(fabs(nup), fabs(nun)), eps, rp, rd)) {
      st = 0;
      break;
    }
  }
}

// A date's row: wl / ws on the legs, 0 elsewhere (z: the solver's iterate), NaN on absent cells
template <int EPT>
__device__ __forceinline__ void smv_write_row(double* wj, int A, const int (&sg)[EPT], const bool (&pr)[EPT],
                                              double wl, double ws) {
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = threadIdx.x + e * blockDim.x;
    if (a < A) wj[a] = pr[e] ? (sg[e] > 0 ? wl : (sg[e] < 0 ? ws : 0.0)) : qnan();
  }
}
template <int EPT>
__device__ __forceinline__ void smv_write_row(double* wj, int A, const bool (&pr)[EPT], const double (&z)[EPT]) {
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = threadIdx.x + e * blockDim.x;
    if (a < A) wj[a] = pr[e] ? z[e] : qnan();
  }
}

// A date's counts [2] and info [6] (status, iterations, primal and dual residual, delta, rho)
__device__ __forceinline__ void smv_write_info(double* cnt, double* inf, double nl, double ns, int st,
                                               int it, double rp, double rd, double delta, double rho) {
  if (threadIdx.x == 0) {
    cnt[0] = nl;
    cnt[1] = ns;
    inf[0] = (double)st;
    inf[1] = (double)it;
    inf[2] = rp;
    inf[3] = rd;
    inf[4] = delta;
    inf[5] = rho;
  }
}

}  // namespace

static inline size_t smv_lds_bytes(int64_t A, int64_t Lmax, bool m_in_lds) {
  return sizeof(double) * (size_t)(A + SMV_SMALL + (m_in_lds ? Lmax * Lmax : 0));
}

// ---- host side: one block size and one EPT instantiation per asset count, the launch, the
// window tables' check

static inline int smv_threads(int64_t A) { return A <= 256 ? 256 : (A <= 512 ? 512 : 1024); }

// the instantiation of the kernel template k whose EPT elements per thread cover A columns
#define SMV_KERNEL(k, A) fmx::smv_pick(A, (const void*)k<1>, (const void*)k<2>, (const void*)k<4>, (const void*)k<8>, \
                                       (const void*)k<16>)
static inline const void* smv_pick(int64_t A, const void* k1, const void* k2, const void* k4, const void* k8,
                                   const void* k16) {
  const int64_t ept = ceil_div(A, smv_threads(A));
  return ept <= 1 ? k1 : ept <= 2 ? k2 : ept <= 4 ? k4 : ept <= 8 ? k8 : k16;
}

// dynamic LDS above 64 KiB has to be allowed per kernel before the launch
static inline fmx_status smv_launch(const void* fn, int64_t grid, int nt, void** args, size_t lds, hipStream_t s) {
  if (lds > 64 * 1024) FMX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FMX_HIP(hipLaunchKernel(fn, dim3((unsigned)grid), dim3(nt), args, lds, s));
  return FMX_OK;
}

// The row lists are read back and checked: an index outside the panel is an argument error.
// win_T [rows], win_rows [rows][Lmax]; prefix names the caller in the message.
static inline fmx_status smv_check_windows(const int32_t* win_T, const int32_t* win_rows, int64_t rows, int64_t Lmax,
                                           int64_t Dr, hipStream_t s, const char* prefix) {
  std::vector<int32_t> ht((size_t)rows), hr((size_t)(rows * Lmax));
  FMX_HIP(hipMemcpyAsync(ht.data(), win_T, sizeof(int32_t) * ht.size(), hipMemcpyDeviceToHost, s));
  FMX_HIP(hipMemcpyAsync(hr.data(), win_rows, sizeof(int32_t) * hr.size(), hipMemcpyDeviceToHost, s));
  FMX_HIP(hipStreamSynchronize(s));
  for (int64_t j = 0; j < rows; ++j) {
    FMX_ARG(ht[j] >= 0 && ht[j] <= Lmax, std::string(prefix) + ": win_T outside [0, Lmax]");
    for (int32_t k = 0; k < ht[j]; ++k)
      FMX_ARG(hr[j * Lmax + k] >= 0 && hr[j * Lmax + k] < Dr,
              std::string(prefix) + ": window row index outside the returns panel");
  }
  return FMX_OK;
}

}  // namespace fmx
