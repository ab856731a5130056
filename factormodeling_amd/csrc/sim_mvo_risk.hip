// Daily trade list, method 'mvo', against the factor risk model: the problem,
// constraints, box, statuses, counts and info of k_sim_mvo (sim_mvo.hip), one workgroup per date,
// with
//
//   Sigma = diag(s2) + B'F B   on the day's active cells
//
// B [K][Dm][A] the exposures (a non-finite exposure counts as 0), Fc [Dm][K][K] the factor
// covariance (lower triangle), S2 [Dm][A] the specific variances, all at the model date
// model_row[j] of book j (-1: no model, status 4).  ADMM exactly as k_sim_mvo with
//   K = 2 Sigma + rho I = E + 2 B'L L'B,   E = 2 diag(s2) + rho I (per asset),   F = L L'
//   K^-1 v = E^-1 v - E^-1 B' P B E^-1 v,  P = L M^-1 L',  M = 1/2 I + L'G L,  G = B E^-1 B'
// (Woodbury; G, M and P are K x K, K <= 32).  L is a semidefinite Cholesky factor built in LDS:
// a pivot at or below 1e-10 of its diagonal entry is dropped (its column of L is zero), the
// rule fmx_cs_ols applies to collinear columns; a pivot below -1e-10 of it is a fallback.  G is
// built one staged row at a time over the active columns, like smv_gram.
//   rho: with more active cells than factors, n - K eigenvalues of 2 Sigma lie in
//   [2 min s2, 2 max s2] and at most K above; the x-step inverts those K directions exactly and
//   rho = 2 max s2, the top of the bulk (sqrt(l_min l_max) over the whole spectrum is orders of
//   magnitude above the bulk and the numpy model does not converge with it).  With
//   n <= K every direction is a factor direction and rho is k_sim_mvo's: sqrt(l_min l_max),
//   l_min = 2 min s2, l_max = 2 max s2 + 2 l_max(L'B B'L) by power iteration on the K x K
//   matrix (an unweighted Gram pass), the ratio floored at SMV_RATIO_FLOOR.
// Per-asset state (z, y, p+, p-, 1/E, sign) lives in registers, EPT elements per thread.  LDS:
// one A-vector, three K x K matrices, the K-vectors and the reduction buffers (157,952 bytes at
// A = 16,384).  Plain fp64 (fma); no fast-math, no cooperative launch, <= 16 waves.
//
// status: 0 converged, 1 max_iter reached, 2 x0 fallback (an infeasible leg, a non-finite or
// negative s2 on an active cell, a non-finite Fc entry, a negative pivot, a non-finite sweep
// pivot), 3 flat day, 4 no model (the caller splices the equal-weight book; the row holds zeros).
#include <vector>

#include "sim_mvo_common.hpp"

namespace fmx {

constexpr int RMV_MAX_K = 32;
constexpr double RMV_PIVOT_REL = 1e-10;
constexpr int RMV_KK = RMV_MAX_K * RMV_MAX_K;

namespace {

// smv_rowdot with the exposure row's non-finite cells read as 0
__device__ __forceinline__ double rmv_rowdot(const double* vec, const double* __restrict__ r, int A) {
  const int lane = threadIdx.x & 63;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int a = lane;
  for (; a + 192 < A; a += 256) {
    const double r0 = r[a], r1 = r[a + 64], r2 = r[a + 128], r3 = r[a + 192];
    a0 = __builtin_fma(vec[a], smv_finite(r0) ? r0 : 0.0, a0);
    a1 = __builtin_fma(vec[a + 64], smv_finite(r1) ? r1 : 0.0, a1);
    a2 = __builtin_fma(vec[a + 128], smv_finite(r2) ? r2 : 0.0, a2);
    a3 = __builtin_fma(vec[a + 192], smv_finite(r3) ? r3 : 0.0, a3);
  }
  for (; a < A; a += 64) {
    const double r0 = r[a];
    a0 = __builtin_fma(vec[a], smv_finite(r0) ? r0 : 0.0, a0);
  }
  return smv_wsum((a0 + a1) + (a2 + a3));
}

// The workgroup's view of one date of the model.
struct RmvDay {
  const double* Bd;   // B + model_row * A: row k at Bd + k * stride
  int64_t stride;     // Dm * A
  int A, K;
  double* vec;        // [A]
  double* gv;         // [SMV_MAX_T]
  double* hv;         // [SMV_MAX_T]
  double* G;          // [K * K]: the Gram, then M^-1, then P
  double* Xb;         // [K * K] scratch
  double* L;          // [K * K]
};

// out = op(a) op(b) (K x K), then a barrier
template <bool TA, bool TB>
__device__ __forceinline__ void rmv_mm(double* out, const double* a, const double* b, int K) {
  for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
    const int i = idx / K, j = idx - i * K;
    double s = 0.0;
    for (int r = 0; r < K; ++r) s = __builtin_fma(TA ? a[r * K + i] : a[i * K + r], TB ? b[j * K + r] : b[r * K + j], s);
    out[idx] = s;
  }
  __syncthreads();
}

// d.G <- sum over the columns a of wgt[a] B_k[a] B_l[a] (wgt zero outside the active cells), then
// d.G <- L' G L.  Barriers inside.
template <int EPT>
__device__ __forceinline__ void rmv_gram(RmvDay& d, const double (&wgt)[EPT]) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
  const int K = d.K, A = d.A;
  for (int k = 0; k < K; ++k) {
    const double* r = d.Bd + k * d.stride;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) {
        const double bv = r[a];
        d.vec[a] = wgt[e] != 0.0 && smv_finite(bv) ? wgt[e] * bv : 0.0;
      }
    }
    __syncthreads();
    for (int l = wv; l <= k; l += nw) {
      const double v = rmv_rowdot(d.vec, d.Bd + l * d.stride, A);
      if (lane == 0) {
        d.G[k * K + l] = v;
        d.G[l * K + k] = v;
      }
    }
    __syncthreads();
  }
  rmv_mm<false, false>(d.Xb, d.G, d.L, K);
  rmv_mm<true, false>(d.G, d.L, d.Xb, K);
}

// out = K^-1 v on the active columns (v is zero elsewhere); t1 = pp'v, t2 = pn'v.  d.G holds P.
template <int EPT>
__device__ __forceinline__ void rmv_kapply(RmvDay& d, SmvDay& s, const double (&v)[EPT], double (&out)[EPT], double& t1,
                                           double& t2, const double (&pp)[EPT], const double (&pn)[EPT],
                                           const double (&ie)[EPT]) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
  const int K = d.K, A = d.A;
  double z0 = 0.0;
  t1 = 0.0;
  t2 = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = tid + e * NT;
    if (a < A) {
      d.vec[a] = v[e] * ie[e];
      t1 = __builtin_fma(pp[e], v[e], t1);
      t2 = __builtin_fma(pn[e], v[e], t2);
    }
  }
  smv_sum3(s.red, s.buf, t1, t2, z0);   // barrier inside: vec is complete
  for (int k = wv; k < K; k += nw) {
    const double dd = rmv_rowdot(d.vec, d.Bd + k * d.stride, A);
    if (lane == 0) d.gv[k] = dd;
  }
  __syncthreads();
  if (tid < K) {
    double h = 0.0;
    for (int r = 0; r < K; ++r) h = __builtin_fma(d.G[r * K + tid], d.gv[r], h);
    d.hv[tid] = h;
  }
  __syncthreads();
  double acc[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
  for (int k = 0; k < K; ++k) {
    const double* r = d.Bd + k * d.stride;
    const double hk = d.hv[k];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A && ie[e] != 0.0) {
        const double bv = r[a];
        acc[e] = __builtin_fma(smv_finite(bv) ? bv : 0.0, hk, acc[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) out[e] = ie[e] != 0.0 ? (v[e] - acc[e]) * ie[e] : 0.0;
}

}  // namespace

template <int EPT>
__global__ __launch_bounds__(1024) void k_risk_mvo(const double* __restrict__ B, const double* __restrict__ Fc,
                                                   const double* __restrict__ S2, int K, int64_t Dm, int A,
                                                   const int32_t* __restrict__ model_row, const double* __restrict__ X,
                                                   const uint8_t* __restrict__ present, double u, int max_iter,
                                                   double eps, double* __restrict__ W, double* __restrict__ counts,
                                                   double* __restrict__ info) {
  extern __shared__ double sm[];
  double* vec = sm;                          // [A]
  double* gv = vec + A;                      // [SMV_MAX_T]
  double* hv = gv + SMV_MAX_T;               // [SMV_MAX_T]
  double* red = hv + SMV_MAX_T;              // [2 * SMV_RED]
  double* G = sm + A + SMV_SMALL;            // [RMV_KK] x 3
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int mr = model_row[j];
  const double* xj = X + j * A;
  const uint8_t* pj = present ? present + j * A : nullptr;
  double* wj = W + j * A;
  double* inf = info + j * 6;
  SmvDay s = {nullptr, A, K, nullptr, vec, gv, hv, red, G, 0};
  int& buf = s.buf;

  // ---- the day's legs
  int sg[EPT];
  bool pr[EPT];
  double cp, cn, cr;
  smv_signs<EPT>(xj, pj, A, sg, pr, cp, cn, cr);
  smv_sum3(red, buf, cp, cn, cr);
  const double npos = cp, nneg = cn, npres = cr;

  const bool flat = npos == 0.0 || nneg == 0.0 || npres < 2.0;
  const bool feasible = u * npos >= 1.0 - 1e-12 && u * nneg >= 1.0 - 1e-12;
  int st = flat ? 3 : (mr < 0 ? 4 : (feasible ? 0 : 2));
  double delta = 0.0, rho = 0.0, smax = -1.0, nsmin = -1.7e308;
  double ie[EPT];                           // 1 / E on the active cells, 0 elsewhere
  RmvDay d = {B + (int64_t)(mr < 0 ? 0 : mr) * A, Dm * (int64_t)A, A, K, vec, gv, hv, G, G + RMV_KK, G + 2 * RMV_KK};

  if (st == 0) {
    // ---- s2 on the active cells: finite, >= 0; its range
    double nb = 0.0, z0 = 0.0;
    const double* s2j = S2 + (int64_t)mr * A;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      ie[e] = 0.0;
      if (a < A && sg[e] != 0) {
        const double v = s2j[a];
        ie[e] = v;                           // s2 until rho is known
        if (!smv_finite(v) || v < 0.0) nb += 1.0;
        else {
          smax = fmax(smax, v);
          nsmin = fmax(nsmin, -v);
        }
      }
    }
    // ---- Fc's lower triangle into Xb (both triangles), finite
    const double* Fj = Fc + (int64_t)mr * K * K;
    for (int idx = tid; idx < K * K; idx += NT) {
      const int i = idx / K, c = idx - i * K;
      const double v = c <= i ? Fj[idx] : Fj[c * K + i];
      if (!smv_finite(v)) nb += 1.0;
      d.Xb[idx] = v;
      d.L[idx] = 0.0;
      if (c == i) gv[i] = v;                 // the diagonal before elimination
    }
    smv_put<true>(red, buf, nb, z0, smax, nsmin);
    __syncthreads();
    smv_get<true>(red, buf, nb, z0, smax, nsmin);
    buf ^= 1;
    delta = -nsmin;
    if (nb != 0.0) st = 2;
    // ---- F = L L', pivots in order; Xb holds the Schur complement
    for (int k = 0; k < K && st == 0; ++k) {
      const double piv = d.Xb[k * K + k], tol = RMV_PIVOT_REL * fabs(gv[k]);   // uniform reads
      if (gv[k] < 0.0 || piv < -tol) {
        st = 2;
        break;
      }
      if (!(piv > tol)) continue;            // dropped: column k of L stays zero
      const double lkk = sqrt(piv);
      if (tid >= k && tid < K) d.L[tid * K + k] = tid == k ? lkk : d.Xb[tid * K + k] / lkk;
      __syncthreads();
      for (int idx = tid; idx < K * K; idx += NT) {
        const int i = idx / K, c = idx - i * K;
        if (i > k && c > k) d.Xb[idx] = __builtin_fma(-d.L[i * K + k], d.L[c * K + k], d.Xb[idx]);
      }
      __syncthreads();
    }
  }
  if (st == 0) {
    // ---- rho
    if (npos + nneg > (double)K) {
      rho = 2.0 * smax;
    } else {
      double one[EPT];
#pragma unroll
      for (int e = 0; e < EPT; ++e) one[e] = sg[e] != 0 ? 1.0 : 0.0;
      rmv_gram<EPT>(d, one);
      const double lmax = smv_lmax(s);
      const double l_lo = 2.0 * delta, l_hi = 2.0 * smax + 2.0 * lmax;
      const double ratio = l_lo > SMV_RATIO_FLOOR * l_hi ? l_lo / l_hi : SMV_RATIO_FLOOR;
      rho = l_hi * sqrt(ratio);
      __syncthreads();
    }
    if (!(rho > 0.0) || !smv_finite(rho)) st = 2;
  }
  if (st == 0) {
    // ---- 1 / E, G = B E^-1 B', M = 1/2 I + L'G L inverted in place, P = L M^-1 L'
#pragma unroll
    for (int e = 0; e < EPT; ++e) ie[e] = sg[e] != 0 ? 1.0 / __builtin_fma(2.0, ie[e], rho) : 0.0;
    rmv_gram<EPT>(d, ie);
    if (smv_sweep(s, 1.0, 1.0, rho)) st = 2;
  }
  if (st != 0) {
    const bool x0 = st == 2;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) wj[a] = pr[e] ? (x0 ? (sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0)) : 0.0) : qnan();
    }
    if (tid == 0) {
      counts[2 * j] = x0 ? npos : 0.0;
      counts[2 * j + 1] = x0 ? nneg : 0.0;
      inf[0] = (double)st;
      inf[1] = inf[2] = inf[3] = 0.0;
      inf[4] = delta;
      inf[5] = rho;
    }
    return;
  }
  for (int idx = tid; idx < K * K; idx += NT) G[idx] = -G[idx];
  __syncthreads();
  rmv_mm<false, true>(d.Xb, d.G, d.L, K);
  rmv_mm<false, false>(d.G, d.L, d.Xb, K);

  // ---- p+ = K^-1 e+, p- = K^-1 e-, and the 2 x 2 system of the leg multipliers
  double pp[EPT], pn[EPT];
  double t1, t2, a11 = 0.0, a12 = 0.0, a22 = 0.0;
  {
    double ev[EPT], o1[EPT], o2[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      pp[e] = pn[e] = 0.0;
      ev[e] = sg[e] > 0 ? 1.0 : 0.0;
    }
    rmv_kapply<EPT>(d, s, ev, o1, t1, t2, pp, pn, ie);
#pragma unroll
    for (int e = 0; e < EPT; ++e) ev[e] = sg[e] < 0 ? 1.0 : 0.0;
    rmv_kapply<EPT>(d, s, ev, o2, t1, t2, pp, pn, ie);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      pp[e] = o1[e];
      pn[e] = o2[e];
      a11 += sg[e] > 0 ? pp[e] : 0.0;
      a12 += sg[e] > 0 ? pn[e] : 0.0;
      a22 += sg[e] < 0 ? pn[e] : 0.0;
    }
    smv_sum3(red, buf, a11, a12, a22);
  }
  const double rdet = 1.0 / (a11 * a22 - a12 * a12);

  // ---- ADMM from x0
  double z[EPT], y[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    z[e] = sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0);
    y[e] = 0.0;
  }
  double rp = 0.0, rd = 0.0;
  int it = 0;
  st = 1;
  while (it < max_iter) {
    ++it;
    double b[EPT], kb[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) b[e] = sg[e] != 0 ? rho * (z[e] - y[e]) : 0.0;
    rmv_kapply<EPT>(d, s, b, kb, t1, t2, pp, pn, ie);
    const double r1 = t1 - 1.0, r2 = t2 + 1.0;
    const double nup = (r1 * a22 - r2 * a12) * rdet, nun = (a11 * r2 - a12 * r1) * rdet;
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
    const double eb = fmax(fabs(sp - 1.0), fabs(sn + 1.0));
    const double gs = fmax(fabs(nup), fabs(nun));
    const bool done = rp <= eps && eb <= 0.1 * eps && rd <= eps * gs;
    rp = fmax(rp, eb);
    rd = gs > 0.0 ? rd / gs : rd;
    if (done) {
      st = 0;
      break;
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = tid + e * NT;
    if (a < A) wj[a] = pr[e] ? z[e] : qnan();
  }
  if (tid == 0) {
    counts[2 * j] = npos;
    counts[2 * j + 1] = nneg;
    inf[0] = (double)st;
    inf[1] = (double)it;
    inf[2] = rp;
    inf[3] = rd;
    inf[4] = delta;
    inf[5] = rho;
  }
}

constexpr size_t rmv_lds_bytes(int64_t A) { return sizeof(double) * (size_t)(A + SMV_SMALL + 3 * RMV_KK); }

}  // namespace fmx

using namespace fmx;

// the K x K matrices always fit in LDS beside the A-vector: no workspace
extern "C" int64_t fmx_risk_mvo_books_work_bytes(int64_t A, int64_t K, int64_t J) {
  (void)A;
  (void)K;
  (void)J;
  return 0;
}

extern "C" fmx_status fmx_risk_mvo_books(const double* B, const double* Fc, const double* S2, int64_t K, int64_t Dm,
                                         int64_t A, const int32_t* model_row, const double* X, const uint8_t* present,
                                         int64_t J, double max_weight, int32_t max_iter, double eps, double* W,
                                         double* counts, double* info, void* stream) {
  FMX_ARG(K >= 1 && K <= RMV_MAX_K, "risk_mvo: 1 <= K <= 32 factors");
  FMX_ARG(Dm >= 0 && Dm <= 0x7fffffff && J >= 0 && J <= 0x7fffffff, "risk_mvo: bad dims");
  FMX_ARG(A >= 1 && A <= SMV_MAX_A, "risk_mvo: 1 <= A <= 16384");
  FMX_ARG(model_row && X && W && counts && info, "null pointer");
  FMX_ARG(Dm == 0 || (B && Fc && S2), "null pointer");
  FMX_ARG(max_weight == max_weight, "risk_mvo: NaN max_weight");
  FMX_ARG(max_iter >= 1 && eps > 0.0, "risk_mvo: max_iter >= 1 and eps > 0");
  static_assert(rmv_lds_bytes(SMV_MAX_A) <= SMV_LDS_MAX, "the A-vector and the K x K matrices must fit in LDS");
  if (J == 0) return FMX_OK;
  hipStream_t s = as_stream(stream);
  // the model rows are read back and checked: an index outside the model is an argument error
  {
    std::vector<int32_t> hm((size_t)J);
    FMX_HIP(hipMemcpyAsync(hm.data(), model_row, sizeof(int32_t) * hm.size(), hipMemcpyDeviceToHost, s));
    FMX_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < J; ++j) FMX_ARG(hm[j] >= -1 && hm[j] < Dm, "risk_mvo: model_row outside [-1, Dm)");
  }
  const size_t lds = rmv_lds_bytes(A);
  const int nt = A <= 256 ? 256 : (A <= 512 ? 512 : 1024);
  const int ept = (int)ceil_div(A, nt);
  const void* fn = ept <= 1 ? (const void*)k_risk_mvo<1> : ept <= 2 ? (const void*)k_risk_mvo<2>
                 : ept <= 4 ? (const void*)k_risk_mvo<4> : ept <= 8 ? (const void*)k_risk_mvo<8>
                            : (const void*)k_risk_mvo<16>;
  if (lds > 64 * 1024) FMX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int Ki = (int)K, Ai = (int)A, mi = max_iter;
  void* args[] = {(void*)&B, (void*)&Fc, (void*)&S2, (void*)&Ki, (void*)&Dm, (void*)&Ai, (void*)&model_row, (void*)&X,
                  (void*)&present, (void*)&max_weight, (void*)&mi, (void*)&eps, (void*)&W, (void*)&counts, (void*)&info};
  FMX_HIP(hipLaunchKernel(fn, dim3((unsigned)J), dim3(nt), args, lds, s));
  return FMX_OK;
}
