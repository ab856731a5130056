// Daily trade list, method 'mvo' (portfolio_simulation.py:96-154, :183-204, :315-461): the
// minimum-variance long/short book of every date in one launch, one workgroup per date.
//
//   min_w  w'Sigma w   s.t.  sum_pos w = 1, sum_neg w = -1, 0 <= w_i <= u on pos (x_i > 0),
//                            -u <= w_i <= 0 on neg (x_i < 0), w_i = 0 elsewhere
//
// Sigma (:349-374) is the ddof=1 sample covariance of the day's window of returns (T rows of
// the zero-filled panel R0, the rows listed per date) plus 1e-6 I, shrunk towards avg_var I
// with avg_var the mean diagonal over the day's PRESENT symbols.  On the active columns
//   Sigma = delta I + sc2 C'C,   C = X - 1 m' (T x n, m the column means),
//   sc2 = (1 - s) / (T - 1),     delta = (1 - s) 1e-6 + s avg_var        (s <= 0: s = 0)
// so T <= 64 rows carry the whole matrix.  ADMM on x (quadratic + the two leg budgets) /
// z (signed box) with the scaled dual y and K = 2 Sigma + rho I = c I + 2 sc2 C'C, c = 2 delta + rho:
//   K^-1 v = (v - sc2 C' M^-1 C v) / c,   M = c/2 I + sc2 C C'   (Woodbury, M is T x T)
//   x = K^-1 b - nu+ p+ - nu- p-,  b = rho (z - y),  p+- = K^-1 e+-,  (nu+, nu-) from the 2 x 2
//       system  [e+'p+  e+'p-; e-'p+  e-'p-] nu = (p+'b - 1, p-'b + 1)
//   z = clip(x + y, box),  y += x - z
//   stop when |x - z|_inf <= eps, both leg-sum errors <= eps / 10 and rho |z - z_prev|_inf <= eps g,
//   g = max(|nu+|, |nu-|).  This is k_mvo_admm's rule with the dual residual taken relative to the
//   gradient: 2 Sigma w equals -nu+- on the interior of a leg, and is of order 1e-7 (5,000 assets)
//   to 1e-5, so an absolute 1e-9 would pass long before the KKT conditions hold to 1e-6 of it.
//   rho = sqrt(l_min l_max) of 2 Sigma: l_min = 2 delta (exact whenever T - 1 < n), l_max =
//   2 delta + 2 sc2 l_max(C C') by power iteration on the T x T Gram; l_min / l_max floored at
//   SMV_RATIO_FLOOR.
// The centring is applied algebraically ((X - 1 m')v = Xv - 1 (m'v)), so every panel read is a
// coalesced row read over the full asset width; inactive entries are held at zero.  Per-asset
// state (z, y, p+, p-, m, sign) lives in registers, EPT elements per thread (EPT = 16 at
// A = 16,384 spills part of it to scratch).  LDS: one A-vector, M^-1 (in the workspace instead
// when the two do not fit in 160 KiB together), the T-vectors and the reduction buffers.
// The centred Gram is M^-1's source: C C' = sum over active columns, one staged row at a time.
// All arithmetic is plain fp64 (fma); no fast-math, no cooperative launch, <= 16 waves.
//
// The phases (legs, window statistics, Gram, power iteration, sweep, Woodbury apply) are the
// functions of sim_mvo_common.hpp, shared with sim_mvo_turnover.hip.
//
// Caps: A <= 16,384 (SMV_MAX_A), T <= 64 rows per window (SMV_MAX_T).
#include <vector>

#include "sim_mvo_common.hpp"

namespace fmx {

// status (info[0]): 0 converged, 1 max_iter reached (last iterate kept), 2 x0 fallback (T = 1,
// an infeasible leg or a non-finite window), 3 flat day, 4 no returns history (T = 0: the
// caller splices the equal-weight book; the row holds zeros).
template <int EPT>
__global__ __launch_bounds__(1024) void k_sim_mvo(const double* __restrict__ R0, int A, const int32_t* __restrict__ win_rows,
                                                  int Lmax, const int32_t* __restrict__ win_T,
                                                  const double* __restrict__ X, const uint8_t* __restrict__ present,
                                                  double shrink, double u, int max_iter, double eps,
                                                  double* __restrict__ W, double* __restrict__ counts,
                                                  double* __restrict__ info, double* __restrict__ work) {
  extern __shared__ double sm[];
  double* vec = sm;                          // [A]
  double* gv = vec + A;                      // [SMV_MAX_T]
  double* hv = gv + SMV_MAX_T;               // [SMV_MAX_T]
  double* red = hv + SMV_MAX_T;              // [2 * SMV_RED]
  int* rows = (int*)(red + 2 * SMV_RED);     // [SMV_MAX_T]
  const int64_t j = blockIdx.x;
  double* M = work ? work + j * (SMV_MAX_T * SMV_MAX_T) : sm + A + SMV_SMALL;   // [T * T]
  const int tid = threadIdx.x, NT = blockDim.x;
  const int T = win_T[j];
  const double* xj = X + j * A;
  const uint8_t* pj = present ? present + j * A : nullptr;
  double* wj = W + j * A;
  double* inf = info + j * 6;
  SmvDay d = {R0, A, T, rows, vec, gv, hv, red, M, 0};
  int& buf = d.buf;

  // ---- the day's legs
  int sg[EPT];      // +1 / -1 on the legs, 0 elsewhere
  bool pr[EPT];     // the symbol has a row on this date
  double cp, cn, cr;
  smv_signs<EPT>(xj, pj, A, sg, pr, cp, cn, cr);
  smv_sum3(red, buf, cp, cn, cr);
  const double npos = cp, nneg = cn, npres = cr;

  const bool flat = npos == 0.0 || nneg == 0.0 || npres < 2.0;
  const bool feasible = u * npos >= 1.0 - 1e-12 && u * nneg >= 1.0 - 1e-12;
  if (flat || T <= 1 || !feasible) {
    const bool x0 = !flat && T != 0;
    const double wl = x0 ? 1.0 / npos : 0.0, ws = x0 ? -1.0 / nneg : 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) wj[a] = pr[e] ? (sg[e] > 0 ? wl : (sg[e] < 0 ? ws : 0.0)) : qnan();
    }
    if (tid == 0) {
      counts[2 * j] = x0 ? npos : 0.0;
      counts[2 * j + 1] = x0 ? nneg : 0.0;
      inf[0] = flat ? 3.0 : (T == 0 ? 4.0 : 2.0);
      inf[1] = inf[2] = inf[3] = inf[4] = inf[5] = 0.0;
    }
    return;
  }

  // ---- column means and the diagonal of the sample covariance
  if (tid < T) rows[tid] = win_rows[j * Lmax + tid];
  __syncthreads();
  double m[EPT];
  smv_col_means<EPT>(d, m);
  double dsum = smv_diag_sum<EPT>(d, m, pr);
  dsum = smv_sum(red, buf, dsum);
  const double avg_var = dsum / ((double)(T - 1) * npres) + 1e-6;
  const double q = shrink > 0.0 ? 1.0 - shrink : 1.0;
  const double delta = q * 1e-6 + (shrink > 0.0 ? shrink * avg_var : 0.0);
  const double sc2 = q / (double)(T - 1);

  // ---- centred Gram over the active columns, its l_max, rho
  smv_gram<EPT>(d, m, sg);
  const double rho = smv_rho(delta, sc2, smv_lmax(d));
  const double c = 2.0 * delta + rho;

  // ---- M = c/2 I + sc2 G, inverted in place
  const int TT = T * T;
  if (smv_sweep(d, c, sc2, rho)) {   // a non-finite return in the window: the solver has no answer, x0 (:451-459)
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) wj[a] = pr[e] ? (sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0)) : qnan();
    }
    if (tid == 0) {
      counts[2 * j] = npos;
      counts[2 * j + 1] = nneg;
      inf[0] = 2.0;
      inf[1] = inf[2] = inf[3] = 0.0;
      inf[4] = delta;
      inf[5] = rho;
    }
    return;
  }
  for (int idx = tid; idx < TT; idx += NT) M[idx] = -M[idx];
  __syncthreads();

  // ---- p+ = K^-1 e+, p- = K^-1 e-, and the 2 x 2 system of the leg multipliers
  double pp[EPT], pn[EPT];
  const double rc = 1.0 / c;
  double t1, t2, a11, a12, a22;
  smv_leg_system<EPT>(d, pp, pn, m, sg, sc2, rc, a11, a12, a22);
  const double rdet = 1.0 / (a11 * a22 - a12 * a12);

  // ---- ADMM from x0
  double z[EPT], y[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    z[e] = sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0);
    y[e] = 0.0;
  }
  double rp = 0.0, rd = 0.0;
  int it = 0, st = 1;
  while (it < max_iter) {
    ++it;
    double b[EPT], kb[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) b[e] = sg[e] != 0 ? rho * (z[e] - y[e]) : 0.0;
    smv_kapply<EPT>(d, b, kb, t1, t2, pp, pn, m, sg, sc2, rc);
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
    // a leg-sum error moves the objective at first order (by the leg's multiplier), the split
    // error |x - z| only through Sigma: the legs are held to eps / 10
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

}  // namespace fmx

using namespace fmx;

// workspace: M^-1 [J][64][64] when the A-vector and M^-1 do not fit in LDS together, else none
extern "C" int64_t fmx_sim_mvo_books_work_bytes(int64_t A, int64_t Lmax, int64_t J) {
  if (A < 0 || Lmax < 0 || J < 0 || Lmax > SMV_MAX_T) return 0;
  if (smv_lds_bytes(A, Lmax, true) <= SMV_LDS_MAX) return 0;
  return (int64_t)sizeof(double) * J * SMV_MAX_T * SMV_MAX_T;
}

extern "C" fmx_status fmx_sim_mvo_books(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows,
                                        const int32_t* win_T, int64_t Lmax, const double* X, const uint8_t* present,
                                        int64_t J, double shrinkage, double max_weight, int32_t max_iter, double eps,
                                        double* W, double* counts, double* info, void* work, int64_t work_bytes,
                                        void* stream) {
  FMX_ARG(Dr >= 0 && J >= 0 && J <= 0x7fffffff, "sim_mvo: bad dims");
  FMX_ARG(A >= 1 && A <= SMV_MAX_A, "sim_mvo: 1 <= A <= 16384");
  FMX_ARG(Lmax >= 1 && Lmax <= SMV_MAX_T, "sim_mvo: 1 <= Lmax <= 64 window rows");
  FMX_ARG(win_rows && win_T && X && W && counts && info, "null pointer");
  FMX_ARG(Dr == 0 || R0, "null pointer");
  FMX_ARG(shrinkage == shrinkage && shrinkage <= 1.0, "sim_mvo: shrinkage_intensity must be <= 1");
  FMX_ARG(max_weight == max_weight, "sim_mvo: NaN max_weight");
  FMX_ARG(max_iter >= 1 && eps > 0.0, "sim_mvo: max_iter >= 1 and eps > 0");
  if (J == 0) return FMX_OK;
  hipStream_t s = as_stream(stream);
  // the row lists are read back and checked: an index outside the panel is an argument error
  {
    std::vector<int32_t> ht((size_t)J), hr((size_t)(J * Lmax));
    FMX_HIP(hipMemcpyAsync(ht.data(), win_T, sizeof(int32_t) * ht.size(), hipMemcpyDeviceToHost, s));
    FMX_HIP(hipMemcpyAsync(hr.data(), win_rows, sizeof(int32_t) * hr.size(), hipMemcpyDeviceToHost, s));
    FMX_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < J; ++j) {
      FMX_ARG(ht[j] >= 0 && ht[j] <= Lmax, "sim_mvo: win_T outside [0, Lmax]");
      for (int32_t k = 0; k < ht[j]; ++k)
        FMX_ARG(hr[j * Lmax + k] >= 0 && hr[j * Lmax + k] < Dr, "sim_mvo: window row index outside the returns panel");
    }
  }
  const bool m_in_lds = smv_lds_bytes(A, Lmax, true) <= SMV_LDS_MAX;
  double* mwork = nullptr;
  if (!m_in_lds) {
    FMX_ARG(work && work_bytes >= fmx_sim_mvo_books_work_bytes(A, Lmax, J), "sim_mvo: workspace too small");
    mwork = (double*)work;
  }
  const size_t lds = smv_lds_bytes(A, Lmax, m_in_lds);
  const int nt = A <= 256 ? 256 : (A <= 512 ? 512 : 1024);
  const int ept = (int)ceil_div(A, nt);
  const void* fn = ept <= 1 ? (const void*)k_sim_mvo<1> : ept <= 2 ? (const void*)k_sim_mvo<2>
                 : ept <= 4 ? (const void*)k_sim_mvo<4> : ept <= 8 ? (const void*)k_sim_mvo<8>
                            : (const void*)k_sim_mvo<16>;
  if (lds > 64 * 1024) FMX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int Ai = (int)A, Li = (int)Lmax, mi = max_iter;
  void* args[] = {(void*)&R0, (void*)&Ai, (void*)&win_rows, (void*)&Li, (void*)&win_T, (void*)&X, (void*)&present,
                  (void*)&shrinkage, (void*)&max_weight, (void*)&mi, (void*)&eps, (void*)&W, (void*)&counts,
                  (void*)&info, (void*)&mwork};
  FMX_HIP(hipLaunchKernel(fn, dim3((unsigned)J), dim3(nt), args, lds, s));
  return FMX_OK;
}
