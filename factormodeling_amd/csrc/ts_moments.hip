// Rolling higher moments (per symbol, over its own present rows): ts_skew / ts_kurt / ts_cov.
// Builder-defined (the reference has none of them), pinned to pandas 2.3:
// x.groupby(level="symbol").rolling(w).skew() / .kurt() / .cov(y), the fixed-window machines of
// window/aggregations.pyx (roll_skew, roll_kurt, roll_mean) restated operation for operation,
// so the results are pandas' bits as values.
//
// One lane per (column, symbol); the 64 lanes of a wave are 64 consecutive assets, so a date row
// is one coalesced 512-B load and one coalesced store.  A launch is F * ceil(A / 64) one-wave
// workgroups, each D rows long: dates are NOT split across threads, because the Kahan
// compensations of the power sums are never reset (pandas takes its fresh-start branch at row 0
// only), so a symbol's state carries its whole history and two segments do not recombine to the
// bits of the sequential walk.  Registers only: no LDS, no scratch buffer.
//
// skew / kurt walk the column twice.  Walk 1: the plain-order sum, count and minimum of the
// symbol's finite rows -> the centre: mean = sum / n, subtracted from every row after C round()
// (halves AWAY from zero) unless min - mean <= -1e5 (skew) / -1e4 (kurt).  The centre is a
// function of the symbol's WHOLE series, later rows included: where |mean| >= 0.5 the last bits
// of a value on date t can depend on rows after t, and a date-subset of a panel need not
// reproduce them.  That is pandas' behaviour and is kept.  Walk 2: the P = 3 | 4 power sums
// with Kahan compensation on the add and on the remove side, the entering row and the row w
// present rows back.  Overflow of x^3 / x^4 is not pinned: once a power sum is inf the state is
// NaN for good, in pandas too.
//
// cov runs three of pandas' mean machines (x y, x, y: Kahan add / remove, the sign-count clamp
// and the consecutive-same-value rule, as ts_ops.hip states them for ts_corr) and the pair count
// in one walk: (mean(xy) - mean(x) mean(y)) * (cnt / (cnt - 1)).  The product of two finite
// values that overflows is not pinned (ts_corr's stance).
//
// The leaving row: on a dense panel it is date d - w, an address that depends on no state, so it
// is prefetched like the entering row; on a ragged panel a trailing pointer walks the symbol's
// own present rows (as k_ts_ptr) and the next leaving value is loaded as soon as the pointer
// moves, a step ahead of its use.  The entering rows (values and presence bytes) of the next
// TSM_B dates are loaded into registers while the dependent chain runs over the current TSM_B.
//
// Row rule (the library's): an absent cell (present == 0) is no row of its symbol -- it changes
// no state and its output is NaN; +-inf count as NaN (Rolling._prep_values).  Every multiply,
// add, divide and sqrt is the IEEE fp64 operation in pandas' order (-ffp-contract=off: val * val
// * val - comp must not contract; no reciprocal shortcuts).
#include <cmath>

#include "fmx_common.hpp"

namespace fmx {

constexpr int TSM_B = 8;          // rows per register batch, one batch in flight ahead of the chain

struct TsmArgs {
  const double* X;                // [F][D][ld]
  const double* Y;                // cov: [D][ld] (y_fstride 0) or [F][D][ld]
  double* O;                      // [F][D][ld]
  const uint8_t* present;         // [D][ld] or nullptr
  int64_t F, D, A, ld, y_fstride, achunks;
  int32_t W;
};

// pandas' _prep_values: +-inf count as NaN
__device__ __forceinline__ double tsm_clean(double v) {
  return (v - v == 0.0) ? v : qnan();
}

// One Kahan step of a power sum: s += y with the compensation c carried (pandas' add_* / remove_*)
__device__ __forceinline__ void tsm_kahan(double& s, double& c, double term) {
  const double y = term - c;
  const double t = s + y;
  c = t - s - y;
  s = t;
}

// ------------------------------------------------------------------------------------------------
// skew (P = 3) / kurt (P = 4)
template <int P, bool RAGGED>
__global__ void __launch_bounds__(64) k_ts_moment(TsmArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = blockIdx.x;
  const int64_t ac = wid % p.achunks, fcol = wid / p.achunks;
  if (fcol >= p.F) return;                                  // wave-uniform
  const int64_t a = ac * 64 + lane;
  const bool ok = a < p.A;
  const int64_t acl = ok ? a : p.A - 1;                     // idle lanes re-read the last column
  const int64_t ld = p.ld, D = p.D;
  const int W = p.W;
  const double* x = p.X + fcol * D * ld + acl;
  const uint8_t* pres = RAGGED ? p.present + acl : nullptr;
  double* o = p.O + fcol * D * ld + a;

  // TSM_B rows from date db on, clamped into [0, D): every load is in bounds and unconditional
  auto load = [&](int64_t db, double (&uu)[TSM_B], uint8_t (&pp)[TSM_B]) {
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) {
      int64_t d = db + k < D ? db + k : D - 1;
      d = d < 0 ? 0 : d;
      uu[k] = x[d * ld];
      pp[k] = RAGGED ? pres[d * ld] : (uint8_t)1;
    }
  };

  double u[TSM_B], un[TSM_B];
  uint8_t pb[TSM_B], pn[TSM_B];

  // ---- walk 1: the centre of the symbol's whole series
  double sum = 0.0, mn = __builtin_inf();
  int n = 0;
  auto step1 = [&](double raw, bool pr) {
    const double v = tsm_clean(raw);
    const bool in = pr && v == v;
    sum = in ? sum + v : sum;
    n += in ? 1 : 0;
    mn = (in && v < mn) ? v : mn;
  };
  load(0, u, pb);
  int64_t db = 0;
  for (; db + TSM_B <= D; db += TSM_B) {
    load(db + TSM_B, un, pn);
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) step1(u[k], pb[k] != 0);
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) { u[k] = un[k]; pb[k] = pn[k]; }
  }
#pragma unroll
  for (int k = 0; k < TSM_B - 1; ++k)
    if (db + k < D) step1(u[k], pb[k] != 0);
  double mean = sum / (double)n;                            // n == 0: NaN, and the comparison is false
  const bool centred = mn - mean > (P == 3 ? -1e5 : -1e4);
  mean = centred ? round(mean) : 0.0;                       // C round: halves away from zero
  auto val_of = [&](double raw) {
    const double v = tsm_clean(raw);
    return centred ? v - mean : v;
  };

  // ---- walk 2: the power sums
  double S[P], CA[P], CR[P];
#pragma unroll
  for (int k = 0; k < P; ++k) S[k] = CA[k] = CR[k] = 0.0;
  double prev = qnan();
  int nobs = 0, same = 0;
  const int minp = W > P ? W : P;
  int64_t i = 0;                                            // present rows seen
  int64_t tail = -1;                                        // ragged: date of present row i - W
  double oldv = 0.0;                                        // ragged: x at `tail`

  auto step2 = [&](int64_t d, double raw, double leaving, bool pr) {
    if (RAGGED && !pr) {
      if (ok) o[d * ld] = qnan();
      return;
    }
    double old = leaving;
    if (RAGGED) {
      if (tail < 0) { tail = d; oldv = raw; }
      if (i >= W) {
        old = oldv;
        // present row i - W + 1 is at or before d (row d is present): the walk stops there
        do { ++tail; } while (pres[tail * ld] == 0);
        oldv = x[tail * ld];
      }
    }
    if (i >= W) {
      const double val = val_of(old);
      if (val == val) {
        nobs -= 1;
        double pw = val;
#pragma unroll
        for (int k = 0; k < P; ++k) {
          if (k) pw = pw * val;                             // val * val * val, left to right
          tsm_kahan(S[k], CR[k], -pw);
        }
      }
    }
    {
      const double val = val_of(raw);
      if (val == val) {
        nobs += 1;
        double pw = val;
#pragma unroll
        for (int k = 0; k < P; ++k) {
          if (k) pw = pw * val;
          tsm_kahan(S[k], CA[k], pw);
        }
        same = (val == prev) ? same + 1 : 1;
        prev = val;
      }
    }
    i += 1;
    double r = qnan();
    if (nobs >= minp) {
      const double dn = (double)nobs;
      if (P == 3) {
        const double A_ = S[0] / dn;
        const double B = S[1] / dn - A_ * A_;
        const double C = S[2] / dn - A_ * A_ * A_ - 3 * A_ * B;
        if (same >= nobs) {
          r = 0.0;
        } else if (!(B <= 1e-14)) {
          const double R = sqrt(B);
          r = (sqrt(dn * (dn - 1.)) * C) / ((dn - 2) * R * R * R);
        }
      } else {
        const double A_ = S[0] / dn;
        double R = A_ * A_;
        const double B = S[1] / dn - R;
        R = R * A_;
        const double C = S[2] / dn - R - 3 * A_ * B;
        R = R * A_;
        const double Dm = S[P - 1] / dn - R - 6 * B * A_ * A_ - 4 * C * A_;
        if (same >= nobs) {
          r = -3.0;
        } else if (!(B <= 1e-14)) {
          const double K = (dn * dn - 1.) * Dm / (B * B) - 3 * ((dn - 1.) * (dn - 1.));
          r = K / ((dn - 2.) * (dn - 3.));
        }
      }
    }
    if (ok) o[d * ld] = r;
  };

  // dense: the leaving rows d - W of a batch, prefetched with it (clamped; read only where i >= W)
  double lv[TSM_B], ln[TSM_B];
  uint8_t pdummy[TSM_B];
  load(0, u, pb);
  if (!RAGGED) load(-(int64_t)W, lv, pdummy);
  db = 0;
  for (; db + TSM_B <= D; db += TSM_B) {
    load(db + TSM_B, un, pn);
    if (!RAGGED) load(db + TSM_B - W, ln, pdummy);
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) step2(db + k, u[k], RAGGED ? 0.0 : lv[k], pb[k] != 0);
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) {
      u[k] = un[k]; pb[k] = pn[k];
      if (!RAGGED) lv[k] = ln[k];
    }
  }
#pragma unroll
  for (int k = 0; k < TSM_B - 1; ++k)                       // the last D % TSM_B rows
    if (db + k < D) step2(db + k, u[k], RAGGED ? 0.0 : lv[k], pb[k] != 0);
}

// ------------------------------------------------------------------------------------------------
// cov: pandas' roll_mean machine (Kahan add / remove, sign counts, consecutive-same-value rule);
// the three machines of a pair share the count, since a row counts for all of them or for none
struct TsmMean {
  double s, ca, cr, prev;
  int neg, same;
  __device__ void init() { s = ca = cr = 0.0; prev = qnan(); neg = same = 0; }
  __device__ void add(double v) {
    tsm_kahan(s, ca, v);
    if (__builtin_signbit(v)) neg += 1;
    same = (v == prev) ? same + 1 : 1;
    prev = v;
  }
  __device__ void remove(double v) {
    tsm_kahan(s, cr, -v);
    if (__builtin_signbit(v)) neg -= 1;
  }
  // n > 0
  __device__ double result(int n) const {
    double r = s / (double)n;
    if (same >= n) r = prev;
    else if (neg == 0 && r < 0) r = 0.0;
    else if (neg == n && r > 0) r = 0.0;
    return r;
  }
};

__device__ __forceinline__ bool tsm_fin(double v) { return __builtin_fabs(v) < __builtin_inf(); }

template <bool RAGGED>
__global__ void __launch_bounds__(64) k_ts_cov(TsmArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = blockIdx.x;
  const int64_t ac = wid % p.achunks, fcol = wid / p.achunks;
  if (fcol >= p.F) return;                                  // wave-uniform
  const int64_t a = ac * 64 + lane;
  const bool ok = a < p.A;
  const int64_t acl = ok ? a : p.A - 1;
  const int64_t ld = p.ld, D = p.D;
  const int W = p.W;
  const double* x = p.X + fcol * D * ld + acl;
  const double* y = p.Y + fcol * p.y_fstride + acl;
  const uint8_t* pres = RAGGED ? p.present + acl : nullptr;
  double* o = p.O + fcol * D * ld + a;

  auto load = [&](int64_t db, double (&uu)[TSM_B], double (&vv)[TSM_B], uint8_t (&pp)[TSM_B]) {
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) {
      int64_t d = db + k < D ? db + k : D - 1;
      d = d < 0 ? 0 : d;
      uu[k] = x[d * ld];
      vv[k] = y[d * ld];
      pp[k] = RAGGED ? pres[d * ld] : (uint8_t)1;
    }
  };

  TsmMean mxy, mx, my;
  mxy.init(); mx.init(); my.init();
  int cnt = 0;
  int64_t i = 0, tail = -1;
  double oldx = 0.0, oldy = 0.0;

  auto step = [&](int64_t d, double xr, double yr, double lx, double ly, bool pr) {
    if (RAGGED && !pr) {
      if (ok) o[d * ld] = qnan();
      return;
    }
    if (RAGGED) {
      if (tail < 0) { tail = d; oldx = xr; oldy = yr; }
      if (i >= W) {
        lx = oldx; ly = oldy;
        do { ++tail; } while (pres[tail * ld] == 0);
        oldx = x[tail * ld]; oldy = y[tail * ld];
      }
    }
    if (i >= W && tsm_fin(lx) && tsm_fin(ly)) {
      const double ox = lx + 0.0 * ly, oy = ly + 0.0 * lx;   // pandas' prep_binary forms
      mxy.remove(ox * oy); mx.remove(ox); my.remove(oy);
      cnt -= 1;
    }
    if (tsm_fin(xr) && tsm_fin(yr)) {
      const double xv = xr + 0.0 * yr, yv = yr + 0.0 * xr;
      mxy.add(xv * yv); mx.add(xv); my.add(yv);
      cnt += 1;
    }
    i += 1;
    double r = qnan();
    if (cnt >= W && cnt > 0) {
      const double c = (double)cnt;
      r = (mxy.result(cnt) - mx.result(cnt) * my.result(cnt)) * (c / (c - 1.0));
    }
    if (ok) o[d * ld] = r;
  };

  double u[TSM_B], v[TSM_B], un[TSM_B], vn[TSM_B];
  double lu[TSM_B], lw[TSM_B], lun[TSM_B], lwn[TSM_B];
  uint8_t pb[TSM_B], pn[TSM_B], pdummy[TSM_B];
  load(0, u, v, pb);
  if (!RAGGED) load(-(int64_t)W, lu, lw, pdummy);
  int64_t db = 0;
  for (; db + TSM_B <= D; db += TSM_B) {
    load(db + TSM_B, un, vn, pn);
    if (!RAGGED) load(db + TSM_B - W, lun, lwn, pdummy);
#pragma unroll
    for (int k = 0; k < TSM_B; ++k)
      step(db + k, u[k], v[k], RAGGED ? 0.0 : lu[k], RAGGED ? 0.0 : lw[k], pb[k] != 0);
#pragma unroll
    for (int k = 0; k < TSM_B; ++k) {
      u[k] = un[k]; v[k] = vn[k]; pb[k] = pn[k];
      if (!RAGGED) { lu[k] = lun[k]; lw[k] = lwn[k]; }
    }
  }
#pragma unroll
  for (int k = 0; k < TSM_B - 1; ++k)
    if (db + k < D) step(db + k, u[k], v[k], RAGGED ? 0.0 : lu[k], RAGGED ? 0.0 : lw[k], pb[k] != 0);
}

template <class K>
static fmx_status tsm_launch(K kernel, const TsmArgs& p, hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)(p.F * p.achunks)), dim3(64), 0, st, p);
  FMX_LAUNCH_CHECK("k_ts_moment");
  return FMX_OK;
}

}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_ts_moment(int32_t op, const double* X, const double* Ycol, double* Y, int64_t F, int64_t D,
                                    int64_t A, int64_t ld, int64_t y_fstride, int32_t window, const uint8_t* present,
                                    void* stream) {
  FMX_ARG(X && Y, "null panel");
  FMX_ARG(F >= 0 && D >= 0 && A >= 0 && ld >= A, "bad dims");
  FMX_ARG(D < (int64_t)1 << 31, "ts_moment: too many dates");
  FMX_ARG(window >= 1, "ts_moment: window must be >= 1");
  FMX_ARG(op == FMX_TSM_SKEW || op == FMX_TSM_KURT || op == FMX_TSM_COV, "ts_moment: unknown op");
  FMX_ARG(op != FMX_TSM_COV || Ycol, "ts_moment: cov needs Ycol");
  FMX_ARG(y_fstride >= 0, "ts_moment: bad y_fstride");
  if (F == 0 || D == 0 || A == 0) return FMX_OK;
  TsmArgs p{};
  p.X = X; p.Y = Ycol; p.O = Y; p.present = present;
  p.F = F; p.D = D; p.A = A; p.ld = ld; p.y_fstride = y_fstride;
  p.achunks = ceil_div(A, 64);
  p.W = window;
  FMX_ARG(F * p.achunks < (int64_t)1 << 31, "panel too large for one launch");
  hipStream_t st = as_stream(stream);
  const bool ragged = present != nullptr;
  switch (op) {
    case FMX_TSM_SKEW:
      return ragged ? tsm_launch(k_ts_moment<3, true>, p, st) : tsm_launch(k_ts_moment<3, false>, p, st);
    case FMX_TSM_KURT:
      return ragged ? tsm_launch(k_ts_moment<4, true>, p, st) : tsm_launch(k_ts_moment<4, false>, p, st);
    default:
      return ragged ? tsm_launch(k_ts_cov<true>, p, st) : tsm_launch(k_ts_cov<false>, p, st);
  }
}
