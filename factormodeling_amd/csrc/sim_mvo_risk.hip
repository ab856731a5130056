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

// ---- Factor-neutral books: k_risk_mvo's problem with B_k . w = 0 for the factors k
// of a mask N.  With G = B E^-1 B' and Q = I - P G,  K^-1 B' = E^-1 B' Q:  K^-1 applied to a
// neutral row is E^-1 B' times a K-vector, and every product of the rows C = [e+; e-; B_N] with
// K^-1 is K x K algebra on the gv = B E^-1 v the x-step forms anyway:
//   S = C K^-1 C':  the leg block a11 a12 a22,  S_N+- = Q_N' g+-  (g+- = B E^-1 e+-, the gv of the
//   two leg applies),  S_NN = (G Q)_NN
//   hv' = (P + Q_N S^-1_NN Q_N') gv + Q_N S^-1_N+- (t1 - 1, t2 + 1)
//   nu+- = S^-1_+-N Q_N' gv + S^-1_+-+- (t1 - 1, t2 + 1)
//   x = E^-1 (b - B' hv') - nu+ p+ - nu- p-
// S is eliminated legs first, then the neutral rows in factor order by symmetric sweeps: a row
// whose pivot is at or below RMV_PIVOT_REL of its own diagonal entry is dropped (a duplicated
// factor), as is a row with no exposure on the active cells; a non-finite entry of S or a pivot
// below -RMV_PIVOT_REL of it is the x0 fallback (status 2).  The set-up runs through the three
// K x K slots (P | G -> G Q -> S_NN -> T -> T Q' | L -> Q); the loop keeps one matrix, two
// K-vectors and three more uniform values.  When smv_stop passes, the neutrality of z is
// confirmed (|B_k . z| <= eps max|B_k| for k in N) before the loop ends.  expo [J][K] = B . w of
// the returned row (NaN on status 3 / 4).
constexpr int RMN_VECS = 12;   // K-vectors behind the three matrices

namespace {

// out = op(a) op(b), or out += with ADD (K x K); out may be a or b: every sum is complete before
// the first store.  K * K <= 4 blockDim.  Barriers inside.
template <bool TA, bool TB, bool ADD>
__device__ __forceinline__ void rmn_mm(double* out, const double* a, const double* b, int K) {
  double acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = threadIdx.x + q * blockDim.x;
    acc[q] = 0.0;
    if (idx < K * K) {
      const int i = idx / K, j = idx - i * K;
      double s = 0.0;
      for (int r = 0; r < K; ++r) s = __builtin_fma(TA ? a[r * K + i] : a[i * K + r], TB ? b[j * K + r] : b[r * K + j], s);
      acc[q] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = threadIdx.x + q * blockDim.x;
    if (idx < K * K) out[idx] = ADD ? out[idx] + acc[q] : acc[q];
  }
  __syncthreads();
}

// out <- sum over the columns a of wgt[a] B_k[a] B_l[a] (rmv_gram without L), bmax[k] <- max |B_k|
// over the columns with a weight.  Barriers inside.
template <int EPT>
__device__ __forceinline__ void rmn_gram(RmvDay& d, SmvDay& s, double* out, double* bmax, const double (&wgt)[EPT]) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
  const int K = d.K, A = d.A;
  for (int k = 0; k < K; ++k) {
    const double* r = d.Bd + k * d.stride;
    double bm = 0.0, z0 = 0.0, z1 = 0.0, z2 = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) {
        const double bv = r[a];
        const bool on = wgt[e] != 0.0 && smv_finite(bv);
        d.vec[a] = on ? wgt[e] * bv : 0.0;
        if (on) bm = fmax(bm, fabs(bv));
      }
    }
    smv_put<true>(s.red, s.buf, z0, z1, bm, z2);
    __syncthreads();                         // vec is complete
    smv_get<true>(s.red, s.buf, z0, z1, bm, z2);
    s.buf ^= 1;
    if (tid == 0) bmax[k] = bm;
    for (int l = wv; l <= k; l += nw) {
      const double v = smv_rowdot<true>(d.vec, d.Bd + l * d.stride, A);
      if (lane == 0) {
        out[k * K + l] = v;
        out[l * K + k] = v;
      }
    }
    __syncthreads();
  }
}

// ej[k] <- B_k . z over the date's columns (z is zero off the legs), by the waves in turn
template <int EPT>
__device__ __forceinline__ void rmn_expo(const RmvDay& d, const double (&z)[EPT], double* ej) {
  const int tid = threadIdx.x, NT = blockDim.x;
  __syncthreads();                           // the last readers of vec
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int a = tid + e * NT;
    if (a < d.A) d.vec[a] = z[e];
  }
  __syncthreads();
  for (int k = tid >> 6; k < d.K; k += NT >> 6) {
    const double v = smv_rowdot<true>(d.vec, d.Bd + k * d.stride, d.A);
    if ((tid & 63) == 0) ej[k] = v;
  }
}

}  // namespace

template <int EPT>
__global__ __launch_bounds__(1024) void k_risk_mvo_neutral(const double* __restrict__ B, const double* __restrict__ Fc,
                                                           const double* __restrict__ S2, int K, int64_t Dm, int A,
                                                           const int32_t* __restrict__ model_row,
                                                           const double* __restrict__ X, const uint8_t* __restrict__ present,
                                                           uint32_t nmask, double u, int max_iter, double eps,
                                                           double* __restrict__ W, double* __restrict__ counts,
                                                           double* __restrict__ info, double* __restrict__ expo) {
  extern __shared__ double sm[];
  const SmvLds l = smv_carve(sm, A);
  double* gv = l.gv;
  double* hv = l.hv;
  double* red = l.red;
  double* G = l.tail;                        // [RMV_KK] x 3, then RMN_VECS K-vectors
  double* kv = G + 3 * RMV_KK;
  double *gp = kv, *gn = kv + RMV_MAX_K, *sp = kv + 2 * RMV_MAX_K, *sn = kv + 3 * RMV_MAX_K, *tp = kv + 4 * RMV_MAX_K,
         *tn = kv + 5 * RMV_MAX_K, *vp = kv + 6 * RMV_MAX_K, *vn = kv + 7 * RMV_MAX_K, *cp = kv + 8 * RMV_MAX_K,
         *cn = kv + 9 * RMV_MAX_K, *d0 = kv + 10 * RMV_MAX_K, *bmax = kv + 11 * RMV_MAX_K;
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
  const int mr = model_row[j];
  double* wj = W + j * A;
  double* ej = expo ? expo + j * K : nullptr;
  SmvDay s = {nullptr, A, K, nullptr, l.vec, gv, hv, red, G, 0};
  int& buf = s.buf;

  // ---- the day's legs, s2, F = L L', rho, P: k_risk_mvo's set-up
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
  RmvDay d = {B + (int64_t)(mr < 0 ? 0 : mr) * A, Dm * (int64_t)A, A, K, l.vec, gv, hv, G, G + RMV_KK, G + 2 * RMV_KK};

  if (st == 0) {
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
#pragma unroll
    for (int e = 0; e < EPT; ++e) ie[e] = sg[e] != 0 ? 1.0 / __builtin_fma(2.0, ie[e], rho) : 0.0;
    rmv_gram<EPT>(d, ie);
    if (smv_sweep(s, 1.0, 1.0, rho)) st = 2;
  }

  double pp[EPT], pn[EPT], z[EPT];
  double ai11 = 0.0, ai12 = 0.0, ai22 = 0.0;   // the inverse of the leg block [a11 a12; a12 a22]
  double s11 = 0.0, s12 = 0.0, s22 = 0.0;      // the leg block of S^-1
  uint32_t inN = 0;                         // the mask's rows with an exposure on the active cells
  if (st == 0) {
    for (int idx = tid; idx < K * K; idx += NT) G[idx] = -G[idx];
    __syncthreads();
    rmv_mm<false, true>(d.Xb, d.G, d.L, K);
    rmv_mm<false, false>(d.G, d.L, d.Xb, K);

    // ---- p+- = K^-1 e+-, g+- and the leg block
#pragma unroll
    for (int e = 0; e < EPT; ++e) pp[e] = pn[e] = 0.0;
    {
      double ev[EPT], o1[EPT], o2[EPT], t1, t2;
#pragma unroll
      for (int e = 0; e < EPT; ++e) ev[e] = sg[e] > 0 ? 1.0 : 0.0;
      rmv_kapply<EPT>(d, s, ev, o1, t1, t2, pp, pn, ie);
      if (tid < K) gp[tid] = gv[tid];
#pragma unroll
      for (int e = 0; e < EPT; ++e) ev[e] = sg[e] < 0 ? 1.0 : 0.0;
      rmv_kapply<EPT>(d, s, ev, o2, t1, t2, pp, pn, ie);
      if (tid < K) gn[tid] = gv[tid];
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
    const double rdet = 1.0 / (a11 * a22 - a12 * a12);
    ai11 = smv_uniform(a22 * rdet);
    ai12 = smv_uniform(-a12 * rdet);
    ai22 = smv_uniform(a11 * rdet);

    // ---- Xb = G, L = Q = I - P G, Xb = G Q; S_N+-, the diagonal of S_NN
    rmn_gram<EPT>(d, s, d.Xb, bmax, ie);
    rmn_mm<false, false, false>(d.L, d.G, d.Xb, K);
    for (int idx = tid; idx < K * K; idx += NT) d.L[idx] = (idx / K == idx % K ? 1.0 : 0.0) - d.L[idx];
    __syncthreads();
    rmn_mm<false, false, false>(d.Xb, d.Xb, d.L, K);
    if (tid < K) {
      double hp = 0.0, hn = 0.0;
      for (int r = 0; r < K; ++r) {
        hp = __builtin_fma(d.L[r * K + tid], gp[r], hp);
        hn = __builtin_fma(d.L[r * K + tid], gn[r], hn);
      }
      sp[tid] = hp;
      sn[tid] = hn;
      d0[tid] = d.Xb[tid * K + tid];
    }
    __syncthreads();
    for (int k = 0; k < K; ++k)
      if (((nmask >> k) & 1u) && bmax[k] > 0.0) inN |= 1u << k;   // uniform reads
    inN = __builtin_amdgcn_readfirstlane(inN);

    // ---- S finite; the legs eliminated from S_NN
    double nb = smv_finite(ai11) && smv_finite(ai12) && smv_finite(ai22) ? 0.0 : 1.0;
    for (int idx = tid; idx < K * K; idx += NT) {
      const int i = idx / K, c = idx - i * K;
      if (((inN >> i) & 1u) && ((inN >> c) & 1u)) {
        const double v = d.Xb[idx];
        if (!smv_finite(v) || !smv_finite(sp[i]) || !smv_finite(sn[i])) nb += 1.0;
        d.Xb[idx] = v - (sp[i] * (ai11 * sp[c] + ai12 * sn[c]) + sn[i] * (ai12 * sp[c] + ai22 * sn[c]));
      }
    }
    if (smv_sum(red, buf, nb) != 0.0) st = 2;   // barrier inside: Xb is complete
  }
  uint32_t kept = 0;
  if (st == 0) {
    // ---- the neutral rows in factor order: Xb <- -(S_NN - S_N+- A^-1 S_+-N)^-1 on the kept rows
    for (int k = 0; k < K; ++k) {
      if (!((inN >> k) & 1u)) continue;
      if (tid < K) hv[tid] = d.Xb[k * K + tid];
      __syncthreads();
      const double piv = hv[k], tol = RMV_PIVOT_REL * fabs(d0[k]);   // uniform reads
      if (piv < -tol || !smv_finite(piv)) {
        st = 2;
        break;
      }
      if (!(piv > tol)) {                    // dropped
        __syncthreads();
        continue;
      }
      kept |= 1u << k;
      const double ip = 1.0 / piv;
      for (int idx = tid; idx < K * K; idx += NT) {
        const int i = idx / K, cc = idx - i * K;
        const double ci = hv[i], cj = hv[cc];
        double nv;
        if (i == k)
          nv = (cc == k) ? -ip : cj * ip;
        else if (cc == k)
          nv = ci * ip;
        else
          nv = __builtin_fma(-ci * ip, cj, d.Xb[idx]);
        d.Xb[idx] = nv;
      }
      __syncthreads();
    }
    kept = __builtin_amdgcn_readfirstlane(kept);
  }
  if (st != 0) {   // no solve today: a zero row, or x0 on status 2
    const bool x0 = st == 2;
    smv_write_row<EPT>(wj, A, sg, pr, x0 ? 1.0 / npos : 0.0, x0 ? -1.0 / nneg : 0.0);
    smv_write_info(counts + 2 * j, info + 6 * j, x0 ? npos : 0.0, x0 ? nneg : 0.0, st, 0, 0.0, 0.0, delta, rho);
    if (ej) {
      if (x0) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) z[e] = sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0);
        rmn_expo<EPT>(d, z, ej);
      } else if (tid < K) {
        ej[tid] = qnan();
      }
    }
    return;
  }

  // ---- T = S^-1_NN (zero off the kept rows), S^-1's other blocks, the loop's vectors and matrix
  for (int idx = tid; idx < K * K; idx += NT) {
    const int i = idx / K, c = idx - i * K;
    d.Xb[idx] = ((kept >> i) & 1u) && ((kept >> c) & 1u) ? -d.Xb[idx] : 0.0;
  }
  __syncthreads();
  if (tid < K) {
    double hp = 0.0, hn = 0.0;
    for (int r = 0; r < K; ++r) {
      hp = __builtin_fma(d.Xb[tid * K + r], sp[r], hp);
      hn = __builtin_fma(d.Xb[tid * K + r], sn[r], hn);
    }
    tp[tid] = hp;
    tn[tid] = hn;
  }
  __syncthreads();
  {
    // uniform: every thread reads the same words
    double w11 = 0.0, w12 = 0.0, w22 = 0.0;
    for (int r = 0; r < K; ++r) {
      w11 = __builtin_fma(sp[r], tp[r], w11);
      w12 = __builtin_fma(sp[r], tn[r], w12);
      w22 = __builtin_fma(sn[r], tn[r], w22);
    }
    const double m11 = ai11 * w11 + ai12 * w12, m12 = ai11 * w12 + ai12 * w22;
    const double m21 = ai12 * w11 + ai22 * w12, m22 = ai12 * w12 + ai22 * w22;
    s11 = smv_uniform(ai11 + (m11 * ai11 + m12 * ai12));
    s12 = smv_uniform(ai12 + (m11 * ai12 + m12 * ai22));
    s22 = smv_uniform(ai22 + (m21 * ai12 + m22 * ai22));
    if (tid < K) {
      vp[tid] = -(tp[tid] * ai11 + tn[tid] * ai12);
      vn[tid] = -(tp[tid] * ai12 + tn[tid] * ai22);
    }
  }
  __syncthreads();
  if (tid < K) {
    double hp = 0.0, hn = 0.0;
    for (int r = 0; r < K; ++r) {
      hp = __builtin_fma(d.L[tid * K + r], vp[r], hp);
      hn = __builtin_fma(d.L[tid * K + r], vn[r], hn);
    }
    cp[tid] = hp;
    cn[tid] = hn;
  }
  rmn_mm<false, true, false>(d.Xb, d.Xb, d.L, K);   // T Q'
  rmn_mm<false, false, true>(d.G, d.L, d.Xb, K);    // P + Q T Q'

  // ---- ADMM from x0: smv_admm's loop around the neutral x-step
  double y[EPT], rp = 0.0, rd = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    z[e] = sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0);
    y[e] = 0.0;
  }
  int it = 0;
  st = 1;
  while (it < max_iter) {
    ++it;
    double b[EPT], t1 = 0.0, t2 = 0.0, z0 = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      b[e] = sg[e] != 0 ? rho * (z[e] - y[e]) : 0.0;
      if (a < A) {
        d.vec[a] = b[e] * ie[e];
        t1 = __builtin_fma(pp[e], b[e], t1);
        t2 = __builtin_fma(pn[e], b[e], t2);
      }
    }
    smv_sum3(red, buf, t1, t2, z0);          // barrier inside: vec is complete
    for (int k = wv; k < K; k += nw) {
      const double dd = smv_rowdot<true>(d.vec, d.Bd + k * d.stride, A);
      if (lane == 0) gv[k] = dd;
    }
    __syncthreads();
    const double r1 = t1 - 1.0, r2 = t2 + 1.0;
    if (tid < K) {
      double h = 0.0;
      for (int r = 0; r < K; ++r) h = __builtin_fma(d.G[r * K + tid], gv[r], h);
      hv[tid] = __builtin_fma(cn[tid], r2, __builtin_fma(cp[tid], r1, h));
    } else if (tid == 64 || tid == 65) {     // nu+ and nu- by two threads of the second wave
      const double* c = tid == 64 ? cp : cn;
      double h = 0.0;
      for (int r = 0; r < K; ++r) h = __builtin_fma(c[r], gv[r], h);
      hv[K + tid - 64] = tid == 64 ? __builtin_fma(s12, r2, __builtin_fma(s11, r1, h))
                                   : __builtin_fma(s22, r2, __builtin_fma(s12, r1, h));
    }
    __syncthreads();
    const double nup = smv_uniform(hv[K]), nun = smv_uniform(hv[K + 1]);
    double acc[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* r = d.Bd + k * d.stride;
      const double hk = hv[k];
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int a = tid + e * NT;
        if (a < A && ie[e] != 0.0) {
          const double bv = r[a];
          acc[e] = __builtin_fma(smv_finite(bv) ? bv : 0.0, hk, acc[e]);
        }
      }
    }
    double sp1 = 0.0, sn1 = 0.0, ep = 0.0, ed = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if (sg[e] != 0) {
        const double kb = (b[e] - acc[e]) * ie[e];
        const double x = __builtin_fma(-nun, pn[e], __builtin_fma(-nup, pp[e], kb));
        const double xv = x + y[e];
        const double lo = sg[e] > 0 ? 0.0 : -u, hi = sg[e] > 0 ? u : 0.0;
        const double zn = xv < lo ? lo : (xv > hi ? hi : xv);
        ep = fmax(ep, fabs(x - zn));
        ed = fmax(ed, rho * fabs(zn - z[e]));
        y[e] = xv - zn;
        z[e] = zn;
        sp1 += sg[e] > 0 ? zn : 0.0;
        sn1 += sg[e] < 0 ? zn : 0.0;
      }
    }
    smv_put<true>(red, buf, sp1, sn1, ep, ed);
    __syncthreads();
    smv_get<true>(red, buf, sp1, sn1, rp, rd);
    buf ^= 1;
    if (smv_stop(sp1, sn1, fmax(fabs(nup), fabs(nun)), eps, rp, rd)) {
      // ---- z's own neutrality, once per pass of the stop rule
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int a = tid + e * NT;
        if (a < A) d.vec[a] = z[e];
      }
      __syncthreads();
      double worst = 0.0, z1 = 0.0, z2 = 0.0;
      for (int k = wv; k < K; k += nw) {
        if (!((inN >> k) & 1u)) continue;
        worst = fmax(worst, fabs(smv_rowdot<true>(d.vec, d.Bd + k * d.stride, A)) / bmax[k]);
      }
      z0 = 0.0;
      smv_put<true>(red, buf, z0, z1, worst, z2);
      __syncthreads();
      smv_get<true>(red, buf, z0, z1, worst, z2);
      buf ^= 1;
      if (worst <= eps) {
        st = 0;
        break;
      }
    }
  }
  smv_write_row<EPT>(wj, A, pr, z);
  smv_write_info(counts + 2 * j, info + 6 * j, npos, nneg, st, it, rp, rd, delta, rho);
  if (ej) rmn_expo<EPT>(d, z, ej);
}

// B . w of finished rows (the empty mask's expo): W's NaN cells read as 0, NaN on status 3 / 4
__global__ __launch_bounds__(256) void k_risk_mvo_expo(const double* __restrict__ B, int K, int64_t Dm, int A,
                                                       const int32_t* __restrict__ model_row, const double* __restrict__ W,
                                                       const double* __restrict__ info, double* __restrict__ expo) {
  extern __shared__ double sm[];
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, mr = model_row[j];
  double* ej = expo + j * K;
  if (mr < 0 || info[6 * j] >= 3.0) {
    if (tid < K) ej[tid] = qnan();
    return;
  }
  for (int a = tid; a < A; a += blockDim.x) {
    const double w = W[j * A + a];
    sm[a] = smv_finite(w) ? w : 0.0;
  }
  __syncthreads();
  const double* Bd = B + (int64_t)mr * A;
  for (int k = tid >> 6; k < K; k += blockDim.x >> 6) {
    const double v = smv_rowdot<true>(sm, Bd + k * Dm * (int64_t)A, A);
    if ((tid & 63) == 0) ej[k] = v;
  }
}

constexpr size_t rmn_lds_bytes(int64_t A) { return rmv_lds_bytes(A) + sizeof(double) * RMN_VECS * RMV_MAX_K; }

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

// the set-up runs through the three K x K slots and the K-vectors in LDS: no workspace
extern "C" int64_t fmx_risk_mvo_neutral_books_work_bytes(int64_t A, int64_t K, int64_t J) {
  (void)A;
  (void)K;
  (void)J;
  return 0;
}

extern "C" fmx_status fmx_risk_mvo_neutral_books(const double* B, const double* Fc, const double* S2, int64_t K,
                                                 int64_t Dm, int64_t A, const int32_t* model_row, const double* X,
                                                 const uint8_t* present, int64_t J, uint32_t neutral_mask,
                                                 double max_weight, int32_t max_iter, double eps, double* W,
                                                 double* counts, double* info, double* expo, void* work,
                                                 int64_t work_bytes, void* stream) {
  (void)work;
  FMX_ARG(work_bytes >= 0, "risk_mvo_neutral: negative work_bytes");
  FMX_ARG(K >= 1 && K <= RMV_MAX_K, "risk_mvo: 1 <= K <= 32 factors");
  FMX_ARG(K == RMV_MAX_K || (neutral_mask >> K) == 0, "risk_mvo_neutral: a neutral factor at or above K");
  static_assert(rmn_lds_bytes(SMV_MAX_A) <= SMV_LDS_MAX, "the A-vector, the K x K matrices and the K-vectors must fit in LDS");
  hipStream_t s = as_stream(stream);
  int Ki = (int)K, Ai = (int)A, mi = max_iter;
  if (neutral_mask == 0) {   // today's problem: today's kernel
    const fmx_status rc = fmx_risk_mvo_books(B, Fc, S2, K, Dm, A, model_row, X, present, J, max_weight, max_iter, eps, W,
                                             counts, info, stream);
    if (rc != FMX_OK || !expo || J == 0) return rc;
    void* eargs[] = {(void*)&B, (void*)&Ki, (void*)&Dm, (void*)&Ai, (void*)&model_row, (void*)&W, (void*)&info, (void*)&expo};
    return smv_launch((const void*)k_risk_mvo_expo, J, 256, eargs, sizeof(double) * (size_t)A, s);
  }
  FMX_ARG(Dm >= 0 && Dm <= 0x7fffffff && J >= 0 && J <= 0x7fffffff, "risk_mvo: bad dims");
  FMX_ARG(A >= 1 && A <= SMV_MAX_A, "risk_mvo: 1 <= A <= 16384");
  FMX_ARG(model_row && X && W && counts && info, "null pointer");
  FMX_ARG(Dm == 0 || (B && Fc && S2), "null pointer");
  FMX_ARG(max_weight == max_weight, "risk_mvo: NaN max_weight");
  FMX_ARG(max_iter >= 1 && eps > 0.0, "risk_mvo: max_iter >= 1 and eps > 0");
  if (J == 0) return FMX_OK;
  {
    std::vector<int32_t> hm((size_t)J);
    FMX_HIP(hipMemcpyAsync(hm.data(), model_row, sizeof(int32_t) * hm.size(), hipMemcpyDeviceToHost, s));
    FMX_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < J; ++j) FMX_ARG(hm[j] >= -1 && hm[j] < Dm, "risk_mvo: model_row outside [-1, Dm)");
  }
  void* args[] = {(void*)&B, (void*)&Fc, (void*)&S2, (void*)&Ki, (void*)&Dm, (void*)&Ai, (void*)&model_row, (void*)&X,
                  (void*)&present, (void*)&neutral_mask, (void*)&max_weight, (void*)&mi, (void*)&eps, (void*)&W,
                  (void*)&counts, (void*)&info, (void*)&expo};
  return smv_launch(SMV_KERNEL(k_risk_mvo_neutral, A), J, smv_threads(A), args, rmn_lds_bytes(A), s);
}
