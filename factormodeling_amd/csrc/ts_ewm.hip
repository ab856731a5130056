// Exponentially weighted operators (per symbol, over its whole history): ts_ewm_mean / var /
// std / zscore / cov / corr.  Builder-defined (the reference has none of them), pinned to
// pandas 2.3: x.groupby(level="symbol").ewm(com, adjust, ignore_na, min_periods).mean() /
// .var() / .std() / .cov(y) / .corr(y), the recursions of window/aggregations.pyx (ewm,
// ewmcov) restated operation for operation, so the results are pandas' bits as values.
//
// Not a windowed kernel: a recurrence along dates, independent across (column, asset).  One
// thread per (column, asset); the 64 lanes of a wave are 64 consecutive assets, so a date row
// is one coalesced 512-B load and one coalesced store per output.  The row addresses do not
// depend on the state, so the next EWM_B rows (values and presence bytes) are loaded into
// registers while the dependent chain runs over the current EWM_B.  Registers only: no LDS, no
// scratch.  The chain is predicated (selects, no lane-divergent branches around the divides);
// every divide and sqrt is the IEEE operation in pandas' order (-ffp-contract=off, no
// reciprocal shortcuts: a quotient of two state variables has no table to lean on).
//
// Dates are NOT split across threads: the state after a segment is a rounded value, and two
// segments' states do not recombine to the bits of the sequential recursion.  A panel therefore
// launches F * ceil(A / 64) one-wave workgroups, each D rows long.
//
// Row rule (the library's): an absent cell (present == 0) is not a row of its symbol -- it
// changes no state and its output is NaN; a present NaN row (and +-inf, which pandas replaces
// by NaN first) decays the weights unless ignore_na.  pandas' first-row rule (state = the
// first row, no decay) is the general step from the state (NaN, old_wt = 1, nobs = 0), so the
// kernel has no first-row case and a late listing needs none either.
#include <cmath>

#include "fmx_common.hpp"

namespace fmx {

// rows per register batch, one batch in flight ahead of the chain.  16 measured within 7 % either
// way and needs 126 / 255 / 256 VGPRs against 72 / 164 / 158.
constexpr int EWM_B = 8;

constexpr int EWM_K_MEAN = 0;     // state (weighted, old_wt, nobs):                      mean
constexpr int EWM_K_VAR = 1;      // ewmcov(x, x): (mean, cov, sum_wt, sum_wt2, old_wt, nobs): mean var std zscore
constexpr int EWM_K_PAIR = 2;     // ewmcov(x, y) + the biased (x,x) (y,y):                cov corr

struct EwmArgs {
  const double* X;                // [F][D][ld]
  const double* Y;                // [D][ld] (pair) or nullptr
  double* O[4];                   // mean var std zscore | cov corr - -; nullptr = not wanted
  const uint8_t* present;         // [D][ld] or nullptr
  int64_t F, D, A, ld, achunks;
  double f;                       // old_wt_factor = 1 - alpha
  double nw;                      // new_wt = adjust ? 1 : alpha
  int32_t adjust, ignore_na, minp;
};

// pandas' _prep_values: +-inf count as NaN
__device__ __forceinline__ double ewm_clean(double v) {
  return (v - v == 0.0) ? v : qnan();
}

// bias=False factor of ewmcov: (sum_wt^2 / (sum_wt^2 - sum_wt2)) * cov, NaN unless the denominator is positive
__device__ __forceinline__ double ewm_debias(double sw, double sw2, double cov) {
  const double num = sw * sw;
  const double den = num - sw2;
  const double r = (num / den) * cov;
  return den > 0.0 ? r : qnan();
}

// pandas.core.window.common.zsqrt: sqrt with negative arguments giving 0 (NaN stays NaN)
__device__ __forceinline__ double ewm_zsqrt(double v) {
  const double r = sqrt(v);
  return v < 0.0 ? 0.0 : r;
}

template <int KIND>
__global__ void __launch_bounds__(64) k_ts_ewm(EwmArgs p) {
  constexpr bool PAIR = KIND == EWM_K_PAIR;
  const int lane = threadIdx.x & 63;
  const int64_t wid = blockIdx.x;
  const int64_t ac = wid % p.achunks, fcol = wid / p.achunks;
  if (fcol >= p.F) return;                                  // wave-uniform
  const int64_t a = ac * 64 + lane;
  const bool ok = a < p.A;
  const int64_t acl = ok ? a : p.A - 1;                     // idle lanes re-read the last column
  const int64_t ld = p.ld, D = p.D;
  const double* x = p.X + fcol * D * ld + acl;
  const double* y = PAIR ? p.Y + acl : nullptr;
  const uint8_t* pres = p.present ? p.present + acl : nullptr;
  const int64_t obase = fcol * D * ld + a;
  const double f = p.f, nw = p.nw, ff = f * f, nw2 = nw * nw;
  const bool adjust = p.adjust != 0, decay_na = p.ignore_na == 0;
  const int minp = p.minp;
  double* const o0 = p.O[0];
  double* const o1 = p.O[1];
  double* const o2 = p.O[2];
  double* const o3 = p.O[3];

  // state
  double mx = qnan(), my = qnan();
  double cxy = 0.0, cxx = 0.0, cyy = 0.0, sw = 1.0, sw2 = 1.0, ow = 1.0;
  int nobs = 0;

  // one row of the recursion; d is its date, (raw, rawy) its values, pr its presence
  auto step = [&](int64_t d, double raw, double rawy, bool pr) {
    const double cx = ewm_clean(raw);
    const double cy = PAIR ? ewm_clean(rawy) : cx;
    const bool obs = pr && cx == cx && cy == cy;
    nobs += obs ? 1 : 0;
    const bool live = mx == mx;                           // a first observation has been seen
    const bool dec = pr && live && (obs || decay_na);     // the row decays the weights
    const bool upd = dec && obs;
    const bool first = pr && !live && obs;
    ow = dec ? ow * f : ow;
    if (KIND != EWM_K_MEAN) {
      sw = dec ? sw * f : sw;
      sw2 = dec ? sw2 * ff : sw2;
    }
    const double wsum = ow + nw;
    const double omx = mx, omy = my;
    const double mxn = ((ow * omx) + (nw * cx)) / wsum;
    mx = (upd && omx != cx) ? mxn : mx;                   // pandas' guard: a constant series keeps its bits
    if (PAIR) {
      const double myn = ((ow * omy) + (nw * cy)) / wsum;
      my = (upd && omy != cy) ? myn : my;
    }
    if (KIND == EWM_K_VAR) {
      const double dm = omx - mx, dc = cx - mx;
      const double cn = ((ow * (cxx + (dm * dm))) + (nw * (dc * dc))) / wsum;
      cxx = upd ? cn : cxx;
    }
    if (PAIR) {
      const double dmx = omx - mx, dmy = omy - my, dcx = cx - mx, dcy = cy - my;
      const double cn = ((ow * (cxy + (dmx * dmy))) + (nw * (dcx * dcy))) / wsum;
      cxy = upd ? cn : cxy;
      if (o1 != nullptr) {                                // the corr's two variances; kernel-uniform
        const double cnx = ((ow * (cxx + (dmx * dmx))) + (nw * (dcx * dcx))) / wsum;
        const double cny = ((ow * (cyy + (dmy * dmy))) + (nw * (dcy * dcy))) / wsum;
        cxx = upd ? cnx : cxx;
        cyy = upd ? cny : cyy;
      }
    }
    if (KIND == EWM_K_MEAN) {
      ow = upd ? (adjust ? wsum : 1.0) : ow;
    } else {
      sw = upd ? sw + nw : sw;
      sw2 = upd ? sw2 + nw2 : sw2;
      ow = upd ? wsum : ow;
      if (!adjust) {                                      // kernel-uniform
        sw = upd ? sw / ow : sw;
        sw2 = upd ? sw2 / (ow * ow) : sw2;
        ow = upd ? 1.0 : ow;
      }
    }
    mx = first ? cx : mx;
    if (PAIR) my = first ? cy : my;

    if (!ok) return;                                        // the tail wave's idle lanes
    const bool full = pr && nobs >= minp;
    const int64_t oi = obase + d * ld;
    if (KIND == EWM_K_MEAN) {
      o0[oi] = full ? mx : qnan();
    } else if (KIND == EWM_K_VAR) {
      const double mean = full ? mx : qnan();
      const double var = full ? ewm_debias(sw, sw2, cxx) : qnan();
      if (o0 != nullptr) o0[oi] = mean;
      if (o1 != nullptr) o1[oi] = var;
      if (o2 != nullptr || o3 != nullptr) {
        const double sd = ewm_zsqrt(var);
        if (o2 != nullptr) o2[oi] = sd;
        if (o3 != nullptr) o3[oi] = (raw - mean) / sd;
      }
    } else {
      if (o0 != nullptr) o0[oi] = full ? ewm_debias(sw, sw2, cxy) : qnan();
      if (o1 != nullptr) o1[oi] = full ? cxy / ewm_zsqrt(cxx * cyy) : qnan();
    }
  };
  // EWM_B rows from date db on, clamped at the last date: every load is in bounds and
  // unconditional, and a presence byte is compared only where its row is consumed
  auto load = [&](int64_t db, double (&uu)[EWM_B], double (&vv)[EWM_B], uint8_t (&pp)[EWM_B]) {
#pragma unroll
    for (int k = 0; k < EWM_B; ++k) {
      const int64_t d = db + k < D ? db + k : D - 1;
      uu[k] = x[d * ld];
      vv[k] = PAIR ? y[d * ld] : 0.0;
      pp[k] = pres != nullptr ? pres[d * ld] : (uint8_t)1;
    }
  };

  double u[EWM_B], v[EWM_B], un[EWM_B], vn[EWM_B];
  uint8_t pb[EWM_B], pn[EWM_B];
  load(0, u, v, pb);
  int64_t db = 0;
  for (; db + EWM_B <= D; db += EWM_B) {
    load(db + EWM_B, un, vn, pn);                           // the next batch: no address depends on the state
#pragma unroll
    for (int k = 0; k < EWM_B; ++k) step(db + k, u[k], v[k], pb[k] != 0);
#pragma unroll
    for (int k = 0; k < EWM_B; ++k) { u[k] = un[k]; v[k] = vn[k]; pb[k] = pn[k]; }
  }
#pragma unroll
  for (int k = 0; k < EWM_B - 1; ++k)                       // the last D % EWM_B rows
    if (db + k < D) step(db + k, u[k], v[k], pb[k] != 0);
}

template <int KIND>
static fmx_status ewm_launch(const EwmArgs& p, hipStream_t st) {
  hipLaunchKernelGGL(k_ts_ewm<KIND>, dim3((unsigned)(p.F * p.achunks)), dim3(64), 0, st, p);
  FMX_LAUNCH_CHECK("k_ts_ewm");
  return FMX_OK;
}

}  // namespace fmx

using namespace fmx;

// One pass over X for mean / var / std / zscore (mean alone runs the three-variable state), one
// more over (X, Ycol) for cov / corr.
extern "C" fmx_status fmx_ts_ewm(const double* X, const double* Ycol, double* Omean, double* Ovar, double* Ostd,
                                 double* Ozscore, double* Ocov, double* Ocorr, int64_t F, int64_t D, int64_t A,
                                 int64_t ld, double com, int32_t adjust, int32_t ignore_na, int32_t min_periods,
                                 const uint8_t* present, void* stream) {
  FMX_ARG(X, "null panel");
  FMX_ARG(F >= 0 && D >= 0 && A >= 0 && ld >= A, "bad dims");
  FMX_ARG(com >= 0.0, "ts_ewm: com must be >= 0");                        // false for NaN
  FMX_ARG(min_periods >= 0, "ts_ewm: min_periods must be >= 0");
  const bool single = Omean || Ovar || Ostd || Ozscore, pair = Ocov || Ocorr;
  FMX_ARG(single || pair, "ts_ewm: no output requested");
  FMX_ARG(!pair || Ycol, "ts_ewm: cov / corr need Ycol");
  if (F == 0 || D == 0 || A == 0) return FMX_OK;
  EwmArgs p{};
  p.X = X;
  p.present = present;
  p.F = F; p.D = D; p.A = A; p.ld = ld;
  p.achunks = ceil_div(A, 64);
  FMX_ARG(F * p.achunks < (int64_t)1 << 31, "panel too large for one launch");
  const double alpha = 1.0 / (1.0 + com);                                 // pandas' rounding path
  p.f = 1.0 - alpha;
  p.nw = adjust ? 1.0 : alpha;
  p.adjust = adjust ? 1 : 0;
  p.ignore_na = ignore_na ? 1 : 0;
  p.minp = min_periods > 1 ? min_periods : 1;                             // 0 behaves as 1
  hipStream_t st = as_stream(stream);
  if (single) {
    p.Y = nullptr;
    p.O[0] = Omean; p.O[1] = Ovar; p.O[2] = Ostd; p.O[3] = Ozscore;
    fmx_status e = (Ovar || Ostd || Ozscore) ? ewm_launch<EWM_K_VAR>(p, st) : ewm_launch<EWM_K_MEAN>(p, st);
    if (e != FMX_OK) return e;
  }
  if (pair) {
    p.Y = Ycol;
    p.O[0] = Ocov; p.O[1] = Ocorr; p.O[2] = nullptr; p.O[3] = nullptr;
    return ewm_launch<EWM_K_PAIR>(p, st);
  }
  return FMX_OK;
}
