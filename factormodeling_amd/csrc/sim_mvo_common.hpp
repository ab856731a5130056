// What the simulator's two MVO trade lists share (sim_mvo.hip: 'mvo', one workgroup per date;
// sim_mvo_turnover.hip: 'mvo_turnover', set-up per date and one workgroup per chain): the
// workgroup reductions, the day's legs, the window statistics, the centred Gram, its largest
// eigenvalue, the inverse of M = c/2 I + sc2 C C' and the Woodbury apply of
// K^-1 = (2 Sigma + rho I)^-1.  Every function is called by all threads of the workgroup, owns
// the barriers it names and keeps the operation order k_sim_mvo had before the split, so
// k_sim_mvo's results are the same bits.
#pragma once
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

// dot of the LDS vector vec [A] with the panel row r [A], by one wave (every lane gets it)
__device__ __forceinline__ double smv_rowdot(const double* vec, const double* __restrict__ r, int A) {
  const int lane = threadIdx.x & 63;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int a = lane;
  for (; a + 192 < A; a += 256) {
    a0 = __builtin_fma(vec[a], r[a], a0);
    a1 = __builtin_fma(vec[a + 64], r[a + 64], a1);
    a2 = __builtin_fma(vec[a + 128], r[a + 128], a2);
    a3 = __builtin_fma(vec[a + 192], r[a + 192], a3);
  }
  for (; a < A; a += 64) a0 = __builtin_fma(vec[a], r[a], a0);
  return smv_wsum((a0 + a1) + (a2 + a3));
}

// The workgroup's view of one date: the panel, the window's rows and the LDS pieces.
struct SmvDay {
  const double* R0;   // [Dr][A]
  int A, T;
  const int* rows;    // [T] window rows of R0 (LDS)
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

// p+ = K^-1 e+, p- = K^-1 e- and the 2 x 2 system of the leg multipliers
template <int EPT>
__device__ __forceinline__ void smv_leg_system(SmvDay& d, double (&pp)[EPT], double (&pn)[EPT], const double (&m)[EPT],
                                               const int (&sg)[EPT], double sc2, double rc, double& a11, double& a12,
                                               double& a22) {
#pragma unroll
  for (int e = 0; e < EPT; ++e) pp[e] = pn[e] = 0.0;
  double t1, t2;
  {
    double ev[EPT], o1[EPT], o2[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) ev[e] = sg[e] > 0 ? 1.0 : 0.0;
    smv_kapply<EPT>(d, ev, o1, t1, t2, pp, pn, m, sg, sc2, rc);
#pragma unroll
    for (int e = 0; e < EPT; ++e) ev[e] = sg[e] < 0 ? 1.0 : 0.0;
    smv_kapply<EPT>(d, ev, o2, t1, t2, pp, pn, m, sg, sc2, rc);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      pp[e] = o1[e];
      pn[e] = o2[e];
    }
  }
  a11 = 0.0;
  a12 = 0.0;
  a22 = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    a11 += sg[e] > 0 ? pp[e] : 0.0;
    a12 += sg[e] > 0 ? pn[e] : 0.0;
    a22 += sg[e] < 0 ? pn[e] : 0.0;
  }
  smv_sum3(d.red, d.buf, a11, a12, a22);
}

// rho = sqrt(l_min l_max) of 2 Sigma with the ratio floored
__device__ __forceinline__ double smv_rho(double delta, double sc2, double lmax) {
  const double l_lo = 2.0 * delta, l_hi = 2.0 * delta + 2.0 * sc2 * lmax;
  const double ratio = l_lo > SMV_RATIO_FLOOR * l_hi ? l_lo / l_hi : SMV_RATIO_FLOOR;
  return l_hi * sqrt(ratio);
}

}  // namespace

static inline size_t smv_lds_bytes(int64_t A, int64_t Lmax, bool m_in_lds) {
  return sizeof(double) * (size_t)(A + SMV_SMALL + (m_in_lds ? Lmax * Lmax : 0));
}

}  // namespace fmx
