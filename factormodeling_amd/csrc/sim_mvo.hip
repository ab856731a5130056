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
// Every phase is a function of sim_mvo_common.hpp; this file is their sequence and the entry point.
//
// Caps: A <= 16,384 (SMV_MAX_A), T <= 64 rows per window (SMV_MAX_T).
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
  const SmvLds l = smv_carve(sm, A);
  const int64_t j = blockIdx.x;
  const int T = win_T[j];
  double* wj = W + j * A;
  double* M = work ? work + j * (SMV_MAX_T * SMV_MAX_T) : l.tail;   // [T * T]
  SmvDay d = {R0, A, T, l.rows, l.vec, l.gv, l.hv, l.red, M, 0};

  // ---- the day's legs
  int sg[EPT];      // +1 / -1 on the legs, 0 elsewhere
  bool pr[EPT];     // the symbol has a row on this date
  double npos, nneg, npres;
  smv_signs<EPT>(X + j * A, present ? present + j * A : nullptr, A, sg, pr, npos, nneg, npres);
  smv_sum3(d.red, d.buf, npos, nneg, npres);
  const bool flat = npos == 0.0 || nneg == 0.0 || npres < 2.0;
  const bool feasible = u * npos >= 1.0 - 1e-12 && u * nneg >= 1.0 - 1e-12;
  double m[EPT], delta = 0.0, sc2 = 0.0, rho = 0.0;
  int st = flat ? 3 : (T == 0 ? 4 : 2);
  // no solve today: a zero row, or x0 on status 2.  The test names T itself: the set-up's loops
  // and divisions are compiled knowing T >= 2
  if (flat || T <= 1 || !feasible) {
    const bool x0 = st == 2;
    smv_write_row<EPT>(wj, A, sg, pr, x0 ? 1.0 / npos : 0.0, x0 ? -1.0 / nneg : 0.0);
    smv_write_info(counts + 2 * j, info + 6 * j, x0 ? npos : 0.0, x0 ? nneg : 0.0, st, 0, 0.0, 0.0, 0.0, 0.0);
    return;
  }
  if (smv_window_setup<EPT>(d, win_rows + j * Lmax, sg, pr, npres, shrink, m, delta, sc2, rho)) {
    smv_write_row<EPT>(wj, A, sg, pr, 1.0 / npos, -1.0 / nneg);
    smv_write_info(counts + 2 * j, info + 6 * j, npos, nneg, 2, 0, 0.0, 0.0, delta, rho);
    return;
  }
  __syncthreads();   // M^-1 is complete

  // ---- p+-, the leg multipliers' system, ADMM from x0
  double pp[EPT], pn[EPT], z[EPT], rp, rd;
  int it;
  const SmvApply<EPT> apply = {d, m, sg, sc2, 1.0 / (2.0 * delta + rho)};
  const SmvLegs lg = smv_leg_system<EPT>(apply, d.red, d.buf, sg, pp, pn);
  smv_admm<EPT>(apply, d.red, d.buf, sg, pp, pn, lg, npos, nneg, rho, u, max_iter, eps, z, st, it, rp, rd);
  smv_write_row<EPT>(wj, A, pr, z);
  smv_write_info(counts + 2 * j, info + 6 * j, npos, nneg, st, it, rp, rd, delta, rho);
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
  if (fmx_status r = smv_check_windows(win_T, win_rows, J, Lmax, Dr, s, "sim_mvo")) return r;
  const bool m_in_lds = smv_lds_bytes(A, Lmax, true) <= SMV_LDS_MAX;
  double* mwork = nullptr;
  if (!m_in_lds) {
    FMX_ARG(work && work_bytes >= fmx_sim_mvo_books_work_bytes(A, Lmax, J), "sim_mvo: workspace too small");
    mwork = (double*)work;
  }
  int Ai = (int)A, Li = (int)Lmax, mi = max_iter;
  void* args[] = {(void*)&R0, (void*)&Ai, (void*)&win_rows, (void*)&Li, (void*)&win_T, (void*)&X, (void*)&present,
                  (void*)&shrinkage, (void*)&max_weight, (void*)&mi, (void*)&eps, (void*)&W, (void*)&counts,
                  (void*)&info, (void*)&mwork};
  return smv_launch(SMV_KERNEL(k_sim_mvo, A), J, smv_threads(A), args, smv_lds_bytes(A, Lmax, m_in_lds), s);
}
