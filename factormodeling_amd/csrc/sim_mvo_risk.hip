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
      const double v = smv_rowdot<true>(d.vec, d.Bd + l * d.stride, A);
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
    const double dd = smv_rowdot<true>(d.vec, d.Bd + k * d.stride, A);
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

// rmv_kapply as the callable smv_leg_system and smv_admm take
template <int EPT>
struct RmvApply {
  RmvDay& d;
  SmvDay& s;
  const double (&ie)[EPT];
  __device__ __forceinline__ void operator()(const double (&v)[EPT], double (&out)[EPT], double& t1, double& t2,
                                             const double (&pp)[EPT], const double (&pn)[EPT]) const {
    rmv_kapply<EPT>(d, s, v, out, t1, t2, pp, pn, ie);
  }
};

}  // namespace

template <int EPT>
__global__ __launch_bounds__(1024) void k_risk_mvo(const double* __restrict__ B, const double* __restrict__ Fc,
                                                   const double* __restrict__ S2, int K, int64_t Dm, int A,
                                                   const int32_t* __restrict__ model_row, const double* __restrict__ X,
                                                   const uint8_t* __restrict__ present, double u, int max_iter,
                                                   double eps, double* __restrict__ W, double* __restrict__ counts,
                                                   double* __restrict__ info) {
  extern __shared__ double sm[];
  const SmvLds l = smv_carve(sm, A);
  double* gv = l.gv;
  double* red = l.red;
  double* G = l.tail;                        // [RMV_KK] x 3
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int mr = model_row[j];
  double* wj = W + j * A;
  SmvDay s = {nullptr, A, K, nullptr, l.vec, gv, l.hv, red, G, 0};
  int& buf = s.buf;

  // ---- the day's legs
  int sg[EPT];
  bool pr[EPT];
  double npos, nneg, npres;
  smv_signs<EPT>(X + j * A, present ? present + j * A : nullptr, A, sg, pr, npos, nneg, npres);
  smv_sum3(red, buf, npos, nneg, npres);

  const bool flat = npos == 0.0 || nneg == 0.0 || npres < 2.0;
  const bool feasible = u * npos >= 1.0 - 1e-12 && u * nneg >= 1.0 - 1e-12;
  int st = flat ? 3 : (mr < 0 ? 4 : (feasible ? 0 : 2));
  double delta = 0.0, rho = 0.0, smax = -1.0, nsmin = -1.7e308;
  double ie[EPT];                           // 1 / E on the active cells, 0 elsewhere
  RmvDay d = {B + (int64_t)(mr < 0 ? 0 : mr) * A, Dm * (int64_t)A, A, K, l.vec, gv, l.hv, G, G + RMV_KK, G + 2 * RMV_KK};

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
      rho = smv_rho(2.0 * delta, 2.0 * smax + 2.0 * smv_lmax(s));
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
  if (st != 0) {   // no solve today: a zero row, or x0 on status 2
    const bool x0 = st == 2;
    smv_write_row<EPT>(wj, A, sg, pr, x0 ? 1.0 / npos : 0.0, x0 ? -1.0 / nneg : 0.0);
    smv_write_info(counts + 2 * j, info + 6 * j, x0 ? npos : 0.0, x0 ? nneg : 0.0, st, 0, 0.0, 0.0, delta, rho);
    return;
  }
  for (int idx = tid; idx < K * K; idx += NT) G[idx] = -G[idx];
  __syncthreads();
  rmv_mm<false, true>(d.Xb, d.G, d.L, K);
  rmv_mm<false, false>(d.G, d.L, d.Xb, K);

  // ---- p+-, the leg multipliers' system, ADMM from x0
  double pp[EPT], pn[EPT], z[EPT], rp, rd;
  int it;
  const RmvApply<EPT> apply = {d, s, ie};
  const SmvLegs lg = smv_leg_system<EPT>(apply, red, buf, sg, pp, pn);
  smv_admm<EPT>(apply, red, buf, sg, pp, pn, lg, npos, nneg, rho, u, max_iter, eps, z, st, it, rp, rd);
  smv_write_row<EPT>(wj, A, pr, z);
  smv_write_info(counts + 2 * j, info + 6 * j, npos, nneg, st, it, rp, rd, delta, rho);
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
  int Ki = (int)K, Ai = (int)A, mi = max_iter;
  void* args[] = {(void*)&B, (void*)&Fc, (void*)&S2, (void*)&Ki, (void*)&Dm, (void*)&Ai, (void*)&model_row, (void*)&X,
                  (void*)&present, (void*)&max_weight, (void*)&mi, (void*)&eps, (void*)&W, (void*)&counts, (void*)&info};
  return smv_launch(SMV_KERNEL(k_risk_mvo, A), J, smv_threads(A), args, rmv_lds_bytes(A), s);
}
