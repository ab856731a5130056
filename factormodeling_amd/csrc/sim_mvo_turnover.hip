// Daily trade list, method 'mvo_turnover' (portfolio_simulation.py:96-154, :206-248, :463-585):
// the minimum-variance book with an L1 turnover penalty against the previous day's book and a
// linear reward on the signal,
//
//   min_w  w'Sigma w + tau sum_i |w_i - p_i| - r sum_i x_i w_i
//   s.t.   sum_pos w = 1, sum_neg w = -1, 0 <= w <= u on pos, -u <= w <= 0 on neg, w = 0 elsewhere
//
// with Sigma, the legs, the exits and the status codes of sim_mvo.hip (the shared pieces are in
// sim_mvo_common.hpp).  p is the last book of the chain, whatever kind of day produced it,
// aligned to today's rows (0 where the symbol had no row yesterday; all zeros on the first date).
//
// Two kernels on one stream, no host synchronisation between them or between dates:
//
//   k_smt_setup  one workgroup per (chain, date): everything that does not depend on p -- the
//                legs and the exit status, the window statistics (delta, sc2), the centred Gram
//                over the active columns, l_max, rho and M^-1 = (c/2 I + sc2 C C')^-1 -- into the
//                date's workspace slot (a 16-double header and the T x T matrix).
//   k_smt_chain  one workgroup per chain, walking the dates in order.  Per date: the column
//                means and p+-, the 2 x 2 budget system (two Woodbury applies: cheaper to redo
//                than 3 A doubles per date of workspace), then ADMM
//                  x = K^-1 (r x_sig + rho (z - y)) - nu+ p+ - nu- p-
//                  xh = 1.6 x - 0.6 z                                  (over-relaxation)
//                  z = clip(p + soft(xh + y - p, tau / rho), box),   y += xh - z
//                started at z0 = the equal-leg x0 and the dual where it will end,
//                  y0 = sign(d_leg) tau / rho on every cell of the leg,
//                  d_leg = (+1 or -1) - sum_leg clip(p, box)
//                (from y0 = 0 the scaled dual would have to climb to tau / rho ~ 1e3 in steps of
//                |x - z|).  The kernel iterates on y - y0: the constant only shifts
//                the leg multipliers and the dead zone of the soft threshold.
//                Stop as k_sim_mvo does, the dual residual taken relative to |q|_inf,
//                q = 2 Sigma x - r x_sig = rho (z - y - x) - nu_leg (free per cell; the
//                multipliers carry tau here and no longer measure the gradient).
//                Then the reference's post-solve step (:553-573): |w| < 1e-6 -> 0 per leg and,
//                when both leg sums stay positive, each leg divided by its sum.  The sums are
//                exact (two integer-valued partial sums per leg, one rounding), so the row does
//                not depend on the reduction order.  The book stays in registers as the next p:
//                the same thread owns a column on every date.
//
// fmx_sim_mvo_turnover_chains (multi_manager's managers): every chain may have its own
// window tables (row b * wchain + j; wchain = 0 is the shared table of fmx_sim_mvo_turnover_books)
// and, with skip_absent, its own date list: a (chain, date) without a present cell gets status 5
// from the set-up, and the chain writes a NaN row and NaN counts and leaves its book untouched, so
// the next date's p is the book of the chain's last date with rows (:100, :206-225).
//
// Wopt (optional) is z before the post-solve step: exactly p_i on cells that did not move and
// exactly 0 / +-u at the box ends.  u is used as min(u, 1): with a leg that sums to 1 the two
// boxes hold the same books.
// Caps as sim_mvo.hip: A <= 16,384, 1 <= Lmax <= 64.  Plain fp64, no cooperative launch.
#include <cmath>

#include "sim_mvo_common.hpp"

namespace fmx {

constexpr int SMT_HDR = 16;    // slot header: status (-1: solve), n_pos, n_neg, delta, sc2, rho
constexpr int SMT_RED5 = 80;   // one 5-value reduction buffer: 16 waves x 5
constexpr double SMT_PRUNE = 1e-6;
constexpr double SMT_RELAX = 1.6;   // ADMM over-relaxation: x -> 1.6 x - 0.6 z_prev in the z- and y-steps

namespace {

// Workgroup reduction of (sum a, sum b, max c, max d, max e): smv_put / smv_get with a fifth value.
__device__ __forceinline__ void smt_put5(double* red, int buf, double a, double b, double c, double d, double e) {
  a = smv_wsum(a);
  b = smv_wsum(b);
  c = smv_wmax(c);
  d = smv_wmax(d);
  e = smv_wmax(e);
  if ((threadIdx.x & 63) == 0) {
    double* r = red + buf * SMT_RED5 + (threadIdx.x >> 6) * 5;
    r[0] = a;
    r[1] = b;
    r[2] = c;
    r[3] = d;
    r[4] = e;
  }
}
__device__ __forceinline__ void smt_get5(const double* red, int buf, double& a, double& b, double& c, double& d,
                                         double& e) {
  const int nw = blockDim.x >> 6;
  const double* r = red + buf * SMT_RED5;
  a = r[0];
  b = r[1];
  c = r[2];
  d = r[3];
  e = r[4];
  for (int w = 1; w < nw; ++w) {
    a += r[5 * w];
    b += r[5 * w + 1];
    c = fmax(c, r[5 * w + 2]);
    d = fmax(d, r[5 * w + 3]);
    e = fmax(e, r[5 * w + 4]);
  }
}

}  // namespace

template <int EPT>
__global__ __launch_bounds__(1024) void k_smt_setup(const double* __restrict__ R0, int A,
                                                    const int32_t* __restrict__ win_rows, int Lmax,
                                                    const int32_t* __restrict__ win_T, const double* __restrict__ X,
                                                    const uint8_t* __restrict__ present, int J, double shrink, double u,
                                                    double* __restrict__ work, int64_t stride, int64_t wchain,
                                                    int skip_absent) {
  extern __shared__ double sm[];
  const SmvLds l = smv_carve(sm, A);
  const int64_t bj = blockIdx.x;
  const int64_t wj = (bj / J) * wchain + bj % J;   // the date's row of the window tables (wchain 0: shared)
  const int T = win_T[wj];
  double* slot = work + bj * stride;
  SmvDay d = {R0, A, T, l.rows, l.vec, l.gv, l.hv, l.red, slot + SMT_HDR, 0};

  int sg[EPT];
  bool pr[EPT];
  double npos, nneg, npres;
  smv_signs<EPT>(X + bj * A, present ? present + bj * A : nullptr, A, sg, pr, npos, nneg, npres);
  smv_sum3(d.red, d.buf, npos, nneg, npres);
  const bool flat = npos == 0.0 || nneg == 0.0 || npres < 2.0;
  const bool feasible = u * npos >= 1.0 - 1e-12 && u * nneg >= 1.0 - 1e-12;
  double status = -1.0, delta = 0.0, sc2 = 0.0, rho = 0.0;
  if (skip_absent && npres == 0.0) {
    status = 5.0;   // no row at all: not a date of this chain
  } else if (flat || T <= 1 || !feasible) {
    status = flat ? 3.0 : (T == 0 ? 4.0 : 2.0);
  } else {
    double m[EPT];
    if (smv_window_setup<EPT>(d, win_rows + wj * Lmax, sg, pr, npres, shrink, m, delta, sc2, rho)) status = 2.0;
  }
  if (threadIdx.x == 0) {
    slot[0] = status;
    slot[1] = npos;
    slot[2] = nneg;
    slot[3] = delta;
    slot[4] = sc2;
    slot[5] = rho;
  }
}

template <int EPT>
__global__ __launch_bounds__(1024) void k_smt_chain(const double* __restrict__ R0, int A,
                                                    const int32_t* __restrict__ win_rows, int Lmax,
                                                    const int32_t* __restrict__ win_T, const double* __restrict__ X,
                                                    const uint8_t* __restrict__ present, int J, double u, double tau,
                                                    double rw, int max_iter, double eps, double* W, double* Wopt,
                                                    double* __restrict__ counts, double* __restrict__ info,
                                                    const double* work, int64_t stride, int m_in_lds,
                                                    int64_t wchain) {
  extern __shared__ double sm[];
  const SmvLds l = smv_carve(sm, A);
  double* red = l.red;
  double* red5 = l.tail;                     // [2 * SMT_RED5]
  double* Mlds = red5 + 2 * SMT_RED5;        // [Lmax * Lmax] when m_in_lds
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, NT = blockDim.x;
  if (u > 1.0) u = 1.0;
  int buf = 0, buf5 = 0;

  double book[EPT];   // the last book on this thread's columns, 0 where the symbol had no row
#pragma unroll
  for (int e = 0; e < EPT; ++e) book[e] = 0.0;

  for (int64_t j = 0; j < J; ++j) {
    const int64_t bj = b * J + j;
    const double* slot = work + bj * stride;
    const double* xj = X + bj * A;
    double* wj = W + bj * A;
    double* oj = Wopt ? Wopt + bj * A : nullptr;
    double* inf = info + bj * 6;
    __syncthreads();   // the previous date is done with rows, M and the vectors
    const int st0 = (int)slot[0];
    const double npos = slot[1], nneg = slot[2], delta = slot[3], sc2 = slot[4], rho = slot[5];
    const int64_t wr = b * wchain + j;
    const int T = win_T[wr];

    if (st0 == 5) {   // skip_absent: every cell is absent; the book in registers is not touched
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int a = tid + e * NT;
        if (a < A) {
          wj[a] = qnan();
          if (oj) oj[a] = qnan();
        }
      }
      smv_write_info(counts + 2 * bj, inf, qnan(), qnan(), 5, 0, 0.0, 0.0, 0.0, 0.0);
      continue;
    }

    int sg[EPT];
    bool pr[EPT];
    {
      double c0, c1, c2;
      smv_signs<EPT>(xj, present ? present + bj * A : nullptr, A, sg, pr, c0, c1, c2);
    }

    if (st0 >= 0) {   // no solve today: flat (3), the caller's equal-weight row (4) or x0 (2)
      const bool x0 = st0 == 2;
      const double wl = x0 ? 1.0 / npos : 0.0, ws = x0 ? -1.0 / nneg : 0.0;
      if (st0 != 4) smv_write_row<EPT>(wj, A, sg, pr, wl, ws);
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int a = tid + e * NT;
        if (a < A) {
          double v = sg[e] > 0 ? wl : (sg[e] < 0 ? ws : 0.0);
          if (st0 == 4) {
            v = wj[a];
            if (!smv_finite(v)) v = 0.0;
          }
          if (oj) oj[a] = pr[e] ? v : qnan();
          book[e] = pr[e] ? v : 0.0;
        }
      }
      smv_write_info(counts + 2 * bj, inf, x0 ? npos : 0.0, x0 ? nneg : 0.0, st0, 0, 0.0, 0.0, delta, rho);
      continue;
    }

    // ---- the window, M^-1 from the set-up, p+-, the 2 x 2 system
    if (tid < T) l.rows[tid] = win_rows[wr * Lmax + tid];
    const double* Ms = slot + SMT_HDR;
    if (m_in_lds)
      for (int idx = tid; idx < T * T; idx += NT) Mlds[idx] = Ms[idx];
    __syncthreads();
    SmvDay d = {R0, A, T, l.rows, l.vec, l.gv, l.hv, red, m_in_lds ? Mlds : const_cast<double*>(Ms), buf};
    double m[EPT], pp[EPT], pn[EPT];
    smv_col_means<EPT>(d, m);
    const SmvApply<EPT> apply = {d, m, sg, sc2, 1.0 / (2.0 * delta + rho)};
    const SmvLegs lg = smv_leg_system<EPT>(apply, red, d.buf, sg, pp, pn);

    // ---- the start: z = x0 and the dual of a leg that has to move one way, y0 = s tau / rho
    // (s = +-1 per leg, 0 for a leg already on target).  y0 is never added to anything: in the
    // x-step a constant on a leg only shifts the leg's multiplier (nu' = nu + rho y0), so
    // y holds y - y0 and the soft threshold's dead zone becomes [-kt (1 + s), kt (1 - s)].
    // Carrying y0 ~ 1e3 inside y would bury q ~ 1e-8 in the rounding of rho y ~ tau.
    const double kt = tau / rho;
    double z[EPT], y[EPT];
    double tlo_p, thi_p, tlo_n, thi_n;
    {
      double sp = 0.0, sn = 0.0, z0 = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const double pc = sg[e] > 0 ? fmin(fmax(book[e], 0.0), u) : fmin(fmax(book[e], -u), 0.0);
        sp += sg[e] > 0 ? pc : 0.0;
        sn += sg[e] < 0 ? pc : 0.0;
      }
      smv_sum3(red, d.buf, sp, sn, z0);
      const double dp = 1.0 - sp, dn = -1.0 - sn;
      const double s_p = dp > 0.0 ? 1.0 : (dp < 0.0 ? -1.0 : 0.0), s_n = dn > 0.0 ? 1.0 : (dn < 0.0 ? -1.0 : 0.0);
      tlo_p = -kt * (1.0 + s_p);
      thi_p = kt * (1.0 - s_p);
      tlo_n = -kt * (1.0 + s_n);
      thi_n = kt * (1.0 - s_n);
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        z[e] = sg[e] > 0 ? 1.0 / npos : (sg[e] < 0 ? -1.0 / nneg : 0.0);
        y[e] = 0.0;
      }
    }

    double rp = 0.0, rd = 0.0;
    int it = 0, st = 1;
    while (it < max_iter) {
      ++it;
      double bv[EPT], kb[EPT], t1, t2, nup, nun;
      if (rw != 0.0) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          const int a = tid + e * NT;
          bv[e] = sg[e] != 0 ? __builtin_fma(rw, xj[a], rho * (z[e] - y[e])) : 0.0;
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) bv[e] = sg[e] != 0 ? rho * (z[e] - y[e]) : 0.0;
      }
      apply(bv, kb, t1, t2, pp, pn);
      lg.nu(t1, t2, nup, nun);
      double sp = 0.0, sn = 0.0, ep = 0.0, ed = 0.0, eq = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        if (sg[e] != 0) {
          const double x = __builtin_fma(-nun, pn[e], __builtin_fma(-nup, pp[e], kb[e]));
          eq = fmax(eq, fabs(rho * (z[e] - y[e] - x) - (sg[e] > 0 ? nup : nun)));
          const double xv = __builtin_fma(SMT_RELAX, x, (1.0 - SMT_RELAX) * z[e]) + y[e];   // over-relaxed x
          const double dv = xv - book[e];
          const double tlo = sg[e] > 0 ? tlo_p : tlo_n, thi = sg[e] > 0 ? thi_p : thi_n;
          const double zc = book[e] + (dv > thi ? dv - thi : (dv < tlo ? dv - tlo : 0.0));   // p exactly when it does not move
          const double lo = sg[e] > 0 ? 0.0 : -u, hi = sg[e] > 0 ? u : 0.0;
          const double zn = zc < lo ? lo : (zc > hi ? hi : zc);
          ep = fmax(ep, fabs(x - zn));
          ed = fmax(ed, rho * fabs(zn - z[e]));
          y[e] = xv - zn;
          z[e] = zn;
          sp += sg[e] > 0 ? zn : 0.0;
          sn += sg[e] < 0 ? zn : 0.0;
        }
      }
      double gs;
      smt_put5(red5, buf5, sp, sn, ep, ed, eq);
      __syncthreads();
      smt_get5(red5, buf5, sp, sn, rp, rd, gs);
      buf5 ^= 1;
      if (smv_stop(sp, sn, gs, eps, rp, rd)) {
        st = 0;
        break;
      }
    }

    // ---- post-solve (:553-573): prune per leg, renormalise when both legs keep weight.
    // |w| in {0} U [1e-6, 1]: |w| 2^36 = hi + lo 2^-36 with hi and lo integers below 2^37, so the
    // partial sums are integers below 2^53 in any order and the leg sum is rounded once.
    double hp = 0.0, lp = 0.0, hn = 0.0, ln = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const double wa = fabs(z[e]) < SMT_PRUNE ? 0.0 : fabs(z[e]);
      const double s = wa * 0x1p36, h = floor(s), l = (s - h) * 0x1p36;
      hp += sg[e] > 0 ? h : 0.0;
      lp += sg[e] > 0 ? l : 0.0;
      hn += sg[e] < 0 ? h : 0.0;
      ln += sg[e] < 0 ? l : 0.0;
    }
    smv_put<false>(red, d.buf, hp, lp, hn, ln);
    __syncthreads();
    smv_get<false>(red, d.buf, hp, lp, hn, ln);
    d.buf ^= 1;
    const double dl = (hp + lp * 0x1p-36) * 0x1p-36, ds = (hn + ln * 0x1p-36) * 0x1p-36;
    const bool renorm = dl > 0.0 && ds > 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int a = tid + e * NT;
      if (a < A) {
        if (oj) oj[a] = pr[e] ? z[e] : qnan();
        double v = z[e];
        if (renorm && sg[e] != 0) v = fabs(v) < SMT_PRUNE ? 0.0 : v / (sg[e] > 0 ? dl : ds);
        wj[a] = pr[e] ? v : qnan();
        book[e] = pr[e] ? v : 0.0;
      }
    }
    smv_write_info(counts + 2 * bj, inf, npos, nneg, st, it, rp, rd, delta, rho);
    buf = d.buf;
  }
}

static size_t smt_lds_bytes(int64_t A, int64_t Lmax, bool m_in_lds) {
  return smv_lds_bytes(A, Lmax, m_in_lds) + sizeof(double) * 2 * SMT_RED5;
}

}  // namespace fmx

using namespace fmx;

// workspace: one slot of SMT_HDR + Lmax^2 doubles per (chain, date)
extern "C" int64_t fmx_sim_mvo_turnover_books_work_bytes(int64_t A, int64_t Lmax, int64_t J, int64_t B) {
  if (A < 0 || Lmax < 0 || J < 0 || B < 0 || Lmax > SMV_MAX_T) return 0;
  return (int64_t)sizeof(double) * B * J * (SMT_HDR + Lmax * Lmax);
}

extern "C" int64_t fmx_sim_mvo_turnover_chains_work_bytes(int64_t A, int64_t Lmax, int64_t J, int64_t B) {
  return fmx_sim_mvo_turnover_books_work_bytes(A, Lmax, J, B);
}

// Both entry points: win_stride is the number of table rows between two chains' window tables
// (0: one table shared by the chains, J: one per chain).
static fmx_status smt_run(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows, const int32_t* win_T,
                          int64_t Lmax, int64_t win_stride, const double* X, const uint8_t* present, int64_t J,
                          int64_t B, double shrinkage, double max_weight, double turnover_penalty, double return_weight,
                          int32_t max_iter, double eps, int32_t skip_absent, double* W, double* Wopt, double* counts,
                          double* info, void* work, int64_t work_bytes, void* stream) {
  FMX_ARG(Dr >= 0 && J >= 0 && B >= 0 && B <= 0x7fffffff && J * B <= 0x7fffffff, "sim_mvo_turnover: bad dims");
  FMX_ARG(A >= 1 && A <= SMV_MAX_A, "sim_mvo_turnover: 1 <= A <= 16384");
  FMX_ARG(Lmax >= 1 && Lmax <= SMV_MAX_T, "sim_mvo_turnover: 1 <= Lmax <= 64 window rows");
  FMX_ARG(win_rows && win_T && X && W && counts && info, "null pointer");
  FMX_ARG(Dr == 0 || R0, "null pointer");
  FMX_ARG(shrinkage == shrinkage && shrinkage <= 1.0, "sim_mvo_turnover: shrinkage_intensity must be <= 1");
  FMX_ARG(max_weight == max_weight, "sim_mvo_turnover: NaN max_weight");
  FMX_ARG(turnover_penalty >= 0.0 && std::isfinite(turnover_penalty), "sim_mvo_turnover: turnover_penalty must be finite and >= 0");
  FMX_ARG(std::isfinite(return_weight), "sim_mvo_turnover: return_weight must be finite");
  FMX_ARG(max_iter >= 1 && eps > 0.0, "sim_mvo_turnover: max_iter >= 1 and eps > 0");
  FMX_ARG(win_stride == 0 || win_stride == J, "sim_mvo_turnover: the window tables' chain stride must be 0 or J");
  if (J == 0 || B == 0) return FMX_OK;
  hipStream_t s = as_stream(stream);
  const int64_t NR = win_stride == 0 ? J : B * J;   // rows of the window tables
  if (fmx_status r = smv_check_windows(win_T, win_rows, NR, Lmax, Dr, s, "sim_mvo_turnover")) return r;
  FMX_ARG(work && work_bytes >= fmx_sim_mvo_turnover_books_work_bytes(A, Lmax, J, B),
          "sim_mvo_turnover: workspace too small");
  double* wk = (double*)work;
  const int64_t stride = SMT_HDR + Lmax * Lmax;
  const int m_in_lds = smt_lds_bytes(A, Lmax, true) <= SMV_LDS_MAX ? 1 : 0;
  const size_t lds_setup = smv_lds_bytes(A, Lmax, false), lds_chain = smt_lds_bytes(A, Lmax, m_in_lds != 0);
  int Ai = (int)A, Li = (int)Lmax, Ji = (int)J, mi = max_iter, ml = m_in_lds;
  int64_t st = stride, wc = win_stride;
  int sk = skip_absent ? 1 : 0;
  void* a1[] = {(void*)&R0, (void*)&Ai, (void*)&win_rows, (void*)&Li, (void*)&win_T, (void*)&X, (void*)&present,
                (void*)&Ji, (void*)&shrinkage, (void*)&max_weight, (void*)&wk, (void*)&st, (void*)&wc, (void*)&sk};
  // the chain kernel's LDS attribute is raised after the set-up launch: if that fails, the set-up
  // has only written its workspace slots
  if (fmx_status r = smv_launch(SMV_KERNEL(k_smt_setup, A), B * J, smv_threads(A), a1, lds_setup, s)) return r;
  void* a2[] = {(void*)&R0, (void*)&Ai, (void*)&win_rows, (void*)&Li, (void*)&win_T, (void*)&X, (void*)&present,
                (void*)&Ji, (void*)&max_weight, (void*)&turnover_penalty, (void*)&return_weight, (void*)&mi,
                (void*)&eps, (void*)&W, (void*)&Wopt, (void*)&counts, (void*)&info, (void*)&wk, (void*)&st, (void*)&ml,
                (void*)&wc};
  return smv_launch(SMV_KERNEL(k_smt_chain, A), B, smv_threads(A), a2, lds_chain, s);
}

extern "C" fmx_status fmx_sim_mvo_turnover_books(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows,
                                                 const int32_t* win_T, int64_t Lmax, const double* X,
                                                 const uint8_t* present, int64_t J, int64_t B, double shrinkage,
                                                 double max_weight, double turnover_penalty, double return_weight,
                                                 int32_t max_iter, double eps, double* W, double* Wopt, double* counts,
                                                 double* info, void* work, int64_t work_bytes, void* stream) {
  return smt_run(R0, Dr, A, win_rows, win_T, Lmax, 0, X, present, J, B, shrinkage, max_weight, turnover_penalty,
                 return_weight, max_iter, eps, 0, W, Wopt, counts, info, work, work_bytes, stream);
}

extern "C" fmx_status fmx_sim_mvo_turnover_chains(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows,
                                                  const int32_t* win_T, int64_t Lmax, int64_t win_stride,
                                                  const double* X, const uint8_t* present, int64_t J, int64_t B,
                                                  double shrinkage, double max_weight, double turnover_penalty,
                                                  double return_weight, int32_t max_iter, double eps,
                                                  int32_t skip_absent, double* W, double* Wopt, double* counts,
                                                  double* info, void* work, int64_t work_bytes, void* stream) {
  return smt_run(R0, Dr, A, win_rows, win_T, Lmax, win_stride, X, present, J, B, shrinkage, max_weight,
                 turnover_penalty, return_weight, max_iter, eps, skip_absent, W, Wopt, counts, info, work, work_bytes,
                 stream);
}
