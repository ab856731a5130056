/*
 * fmx.h -- C ABI of libfmx, the MI355X (gfx950) engine for the FactorModeling
 * factor-panel hot path.
 *
 * Boundary: the reference (Yuming-Yang/FactorModeling) is pure Python; its "FFI" for this
 * path is the set of Python functions in operations.py, factor_selector.py,
 * factor_selection_methods.py and composite_factor.py.  The drop-in modules in
 * factormodeling_amd/ keep those signatures and bind the entry points below through
 * ctypes.  Each entry point names the reference function(s) it
 * replaces.
 *
 * Conventions
 *   - Panels are device pointers to float64 X[F][D][ld] (factor, date, asset; asset
 *     fastest; ld >= A is the row stride in elements).  Returns R are [D][ld].
 *   - present: optional device uint8[D][ld]; 0 marks a (date, symbol) pair with no row
 *     in the reference's long (date, symbol) MultiIndex.  NULL = dense panel.
 *     Time-series ops walk each symbol's present rows (row-based, as the reference's
 *     groupby('symbol') + rolling/shift); cross-sectional ops reduce over the present
 *     rows of a date.  Outputs at absent cells are NaN.
 *   - stream: a hipStream_t passed as void* (NULL = default stream).  All calls are
 *     stream-ordered and asynchronous; no call allocates on the hot path (the only
 *     hipMalloc is the one-time cache of a row length's pairwise-sum schedule).
 *   - Scratch: calls that need device scratch take (work, work_bytes) from the caller,
 *     sized by the matching fmx_*_work_bytes / fmx_*_work_len query; one buffer may be
 *     reused by every call on the same stream.
 *   - Errors: every call returns an fmx_status; fmx_last_error() gives a thread-local
 *     message.  No exceptions cross the ABI.
 */
#ifndef FMX_H_
#define FMX_H_

#include <stdint.h>

/* Doubled average rank of a cell among its row's non-NaN cells (2*#less + #equal + 1; 0
 * for NaN): <= 2A <= 32768 for the A <= 16384 rows the ranked kernels take, so 16 bits. */
typedef uint16_t fmx_rank2_t;

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t fmx_status;
#define FMX_OK 0
#define FMX_ERR_ARG 1
#define FMX_ERR_HIP 2
#define FMX_ERR_UNSUPPORTED 3
#define FMX_ERR_NOMEM 4

#define FMX_ABI_VERSION 1

/* time-series ops (fmx_ts_op) */
#define FMX_TS_SUM 0      /* operations.py:6   ts_sum      rolling(w).sum()            */
#define FMX_TS_MEAN 1     /* operations.py:10  ts_mean     rolling(w).mean()           */
#define FMX_TS_STD 2      /* operations.py:14  ts_std      rolling(w).std()            */
#define FMX_TS_VAR 3      /*                   rolling(w).var() (helper)               */
#define FMX_TS_ZSCORE 4   /* operations.py:18  ts_zscore                               */
#define FMX_TS_RANK 5     /* operations.py:23  ts_rank     pct rank of last in window  */
#define FMX_TS_DECAY 6    /* operations.py:40  ts_decay    linear-weight MA            */
#define FMX_TS_DIFF 7     /* operations.py:34  ts_diff     diff(w), w may be <= 0      */
#define FMX_TS_DELAY 8    /* operations.py:37  ts_delay    shift(w), w may be <= 0     */
#define FMX_TS_BACKFILL 9 /* operations.py:50  ts_backfill ffill()                     */

/* rolling order statistics (fmx_ts_order; builder-defined, pandas semantics) */
#define FMX_TSO_MIN 0      /* ts_min      rolling(w).min()                               */
#define FMX_TSO_MAX 1      /* ts_max      rolling(w).max()                               */
#define FMX_TSO_ARGMIN 2   /* ts_argmin   rows back to the window's minimum, latest tie  */
#define FMX_TSO_ARGMAX 3   /* ts_argmax   rows back to the window's maximum, latest tie  */
#define FMX_TSO_MEDIAN 4   /* ts_median   rolling(w).median()                            */
#define FMX_TSO_QUANTILE 5 /* ts_quantile rolling(w).quantile(q, interpolation)          */

/* ts_quantile interpolation (pandas Rolling.quantile(interpolation=...)) */
#define FMX_TSO_LINEAR 0
#define FMX_TSO_LOWER 1
#define FMX_TSO_HIGHER 2
#define FMX_TSO_MIDPOINT 3
#define FMX_TSO_NEAREST 4

/* rolling higher moments (fmx_ts_moment; builder-defined, pandas semantics) */
#define FMX_TSM_SKEW 0     /* ts_skew     rolling(w).skew()                              */
#define FMX_TSM_KURT 1     /* ts_kurt     rolling(w).kurt()   (excess kurtosis)          */
#define FMX_TSM_COV 2      /* ts_cov      rolling(w).cov(y)   (ddof 1)                   */

/* cross-sectional moment ops (fmx_cs_moment) */
#define FMX_CS_ZSCORE 0            /* operations.py:77  cs_zscore         */
#define FMX_CS_MEAN 1              /* operations.py:85  cs_mean           */
#define FMX_CS_MARKET_NEUTRALIZE 2 /* operations.py:171 market_neutralize */
#define FMX_CS_STATS 3             /* row (mean, std ddof=0) only (fmx_cs_moment_stats) */

/* rank methods (pandas Series.rank(method=...)) */
#define FMX_RANK_AVERAGE 0
#define FMX_RANK_MIN 1
#define FMX_RANK_MAX 2
#define FMX_RANK_FIRST 3
#define FMX_RANK_DENSE 4
#define FMX_RANK_AVERAGE_PROPAGATE 5 /* scipy.stats.rankdata: any NaN -> row NaN; no 0.5 rule */

/* group ops (fmx_group_op) */
#define FMX_GROUP_MEAN 0       /* operations.py:112 group_mean            */
#define FMX_GROUP_NEUTRALIZE 1 /* operations.py:124 group_neutralize      */
#define FMX_GROUP_NORMALIZE 2  /* operations.py:137 group_normalize       */
#define FMX_GROUP_RANK 3       /* operations.py:152 group_rank_normalized */

/* elementwise ops (fmx_elementwise) */
#define FMX_EW_SIGN 0  /* operations.py:88  sign            */
#define FMX_EW_POWER 1 /* operations.py:91  power(x, a)     */
#define FMX_EW_LOG 2   /* operations.py:94  log             */
#define FMX_EW_ABS 3   /* operations.py:97  abs_            */
#define FMX_EW_CLIP 4  /* operations.py:100 clip(x, a, b)   */
#define FMX_EW_WHERE 5 /* operations.py:80  cs_bool(cond, a, b), cond as 0/1 */

/* cs_regression rettype (operations.py:248) */
#define FMX_CSREG_RESID 0
#define FMX_CSREG_BETA 1
#define FMX_CSREG_ALPHA 2
#define FMX_CSREG_FITTED 3
#define FMX_CSREG_R2 4

/* ---- library ------------------------------------------------------------------ */
const char* fmx_last_error(void);
int32_t fmx_abi_version(void);
/* "product", or "diagnostic: ..." for a development build whose kernels carry wrong-result
 * timing arms (-DFMX_DIAG); the Python loader refuses the latter unless FMX_ALLOW_DIAG=1. */
const char* fmx_build_variant(void);
/* Writes "gfx950 ... CUs ... HBM bytes" of the current device into buf. */
fmx_status fmx_device_info(char* buf, int64_t buflen);

/* ---- time series (operations.py:6-51) -------------------------------------------- */
/* Replaces ts_sum/ts_mean/ts_std/ts_zscore/ts_rank/ts_decay/ts_diff/ts_delay/ts_backfill
 * (operations.py:6-51).  Y may not alias X.  Rolling sums/means/variances reproduce
 * pandas' Kahan/Welford kernels bit-for-bit.  Any window (no LDS ring: DESIGN §12), dense
 * or ragged; window < 0 for diff / delay is a lead. */
fmx_status fmx_ts_op(int32_t op, const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld,
                     int32_t window, const uint8_t* present, void* stream);

/* Fused rolling set: ts_mean(window), ts_std(window), ts_zscore(window), ts_rank(rank_window)
 * and ts_decay(window) (operations.py:10-48) from ONE read of X.  Any output may be NULL
 * (not computed); none may alias X.  Each output is bit-identical to fmx_ts_op of that op.
 * Dense panels with (window, rank_window) = (20, 10) run one fused kernel; other windows
 * and ragged panels run one fmx_ts_op pass per requested output. */
fmx_status fmx_ts_set(const double* X, double* Ymean, double* Ystd, double* Yzscore, double* Yrank, double* Ydecay,
                      int64_t F, int64_t D, int64_t A, int64_t ld, int32_t window, int32_t rank_window,
                      const uint8_t* present, void* stream);

/* Builder-defined rolling order statistics (no reference counterpart): per-symbol
 * x.rolling(window).min() / .max() / .median() / .quantile(q, interpolation) and, for
 * FMX_TSO_ARGMIN / ARGMAX, the number of rows back from the current row to the window's
 * extreme (0.0 = the current row; ties go to the most recent row).  ts_rank's row rule: a
 * value only where the symbol has `window` present rows ending at the row and none is NaN,
 * NaN elsewhere.  Results are bit-identical to pandas as values (the sign of a zero result
 * is unspecified).  Any window >= 1 (no cap), dense or ragged; q in [0, 1] and interp
 * (FMX_TSO_LINEAR ...) are read for FMX_TSO_QUANTILE only.  Y may not alias X.  No scratch. */
fmx_status fmx_ts_order(int32_t op, const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld,
                        int32_t window, double q, int32_t interp, const uint8_t* present, void* stream);

/* Builder-defined exponentially weighted operators (no reference counterpart): per symbol,
 * over its own rows in date order, x.ewm(com, adjust, ignore_na, min_periods).mean() / .var()
 * / .std() / .cov(y) / .corr(y) of pandas 2.3 (bias=False for var / std / cov), bit-identical
 * as values, and zscore = (x - mean) / std in IEEE double.  Outputs are [F][D][ld]; a NULL
 * output is not computed (FMX_EWM_* name them in argument order).  mean / var / std / zscore
 * come from ONE pass over X sharing one state (mean alone runs a smaller one); cov / corr take
 * one more pass and need Ycol, one [D][ld] series shared by all F columns.  com >= 0 is the
 * centre of mass (alpha = 1 / (1 + com) in double; span, halflife and alpha are converted by
 * the caller as pandas does); min_periods 0 behaves as 1.  +-inf count as NaN.  An absent
 * cell (present == 0) is no row of its symbol: it decays nothing and its output is NaN; a
 * present NaN row decays the weights unless ignore_na.  No output may alias X or Ycol.  No
 * scratch.  A null panel, ld < A, com < 0 or NaN, min_periods < 0, cov / corr without Ycol
 * and a call with no output are refused before any device work. */
#define FMX_EWM_MEAN 0
#define FMX_EWM_VAR 1
#define FMX_EWM_STD 2
#define FMX_EWM_ZSCORE 3
#define FMX_EWM_COV 4
#define FMX_EWM_CORR 5
fmx_status fmx_ts_ewm(const double* X, const double* Ycol, double* Omean, double* Ovar, double* Ostd,
                      double* Ozscore, double* Ocov, double* Ocorr, int64_t F, int64_t D, int64_t A, int64_t ld,
                      double com, int32_t adjust, int32_t ignore_na, int32_t min_periods, const uint8_t* present,
                      void* stream);

/* Builder-defined rolling higher moments (no reference counterpart): per symbol, over its own
 * present rows in date order, x.rolling(window).skew() / .kurt() / .cov(y) of pandas 2.3
 * (min_periods = window, cov with ddof 1), bit-identical as values, NaN pattern included.
 * +-inf count as NaN.  An absent cell (present == 0) is no row of its symbol and its output
 * is NaN.  Any window >= 1: FMX_TSM_SKEW is all NaN for window < 3, FMX_TSM_KURT for
 * window < 4, FMX_TSM_COV for window < 2.  Ycol is read for FMX_TSM_COV only: one [D][ld]
 * series shared by all F columns (y_fstride 0) or [F][D][ld] (y_fstride = D * ld).
 * skew / kurt centre a symbol's series as pandas does, by C round() of the mean of ALL its
 * rows (unless its minimum lies 1e5 / 1e4 below the mean): where |mean| >= 0.5 the last bits
 * of a value can depend on later rows, so a date-subset of a panel need not reproduce them.
 * Overflow of x^3 / x^4, and of a product x y of two finite values, is not pinned.  One
 * streaming pass per (column, symbol) (skew / kurt: two reads of X), dense or ragged; no
 * scratch.  Y may not alias X or Ycol.  A null panel, ld < A, window < 1, FMX_TSM_COV
 * without Ycol and an unknown op are refused before any device work. */
fmx_status fmx_ts_moment(int32_t op, const double* X, const double* Ycol, double* Y, int64_t F, int64_t D,
                         int64_t A, int64_t ld, int64_t y_fstride, int32_t window, const uint8_t* present,
                         void* stream);

/* Builder-defined ts_corr (no reference counterpart): per-symbol rolling Pearson of X[f]
 * against Ycol (y_fstride = 0: one [D][ld] series shared by all factors, e.g. returns),
 * pandas Rolling.corr semantics, min_periods = window. */
fmx_status fmx_ts_corr(const double* X, const double* Ycol, double* Out, int64_t F, int64_t D, int64_t A,
                       int64_t ld, int64_t y_fstride, int32_t window, const uint8_t* present, void* stream);

/* ts_regression_fast rolling moments (operations.py:185-246) for one [D][ld] pair.
 * Xv is the globally shifted x; valid marks rows kept by the reference's dropna().
 * rettype 0 resid, 1 alpha, 2 beta, 3 fitted, 6 R^2.  NaN where not computed. */
fmx_status fmx_ts_regression(const double* Yv, const double* Xv, const uint8_t* valid, double* Out, int64_t D,
                             int64_t A, int64_t ld, int32_t window, int32_t rettype, void* stream);

/* ---- cross section (operations.py:54-101, 171-182, 248-304) ---------------------- */
fmx_status fmx_cs_moment(int32_t op, const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld,
                         const uint8_t* present, void* stream);
/* fmx_cs_moment that also writes stats[F][D][2] = (nanmean, nanstd ddof=0) per row, the
 * numpy-pairwise moments cs_zscore uses (operations.py:77-78).  op FMX_CS_STATS writes
 * only the stats (Y may be NULL); they feed fmx_gram_fused. */
fmx_status fmx_cs_moment_stats(int32_t op, const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld,
                               const uint8_t* present, double* stats, void* stream);

/* C5's feature (builder-defined; BASELINE configs[4] "60-day rolling ts_corr/ts_std feeding
 * IC-weighted composite"): Y = sign(C) * (X / ts_std(X, window)) per column, ts_std ==
 * 0 -> NaN, C = fmx_ts_corr(X, R, window) of the same rows (np.sign semantics).  The std is
 * pandas' rolling Welford (operations.py:14-15), bit-identical to fmx_ts_op(FMX_TS_STD).
 * Dense panels. */
fmx_status fmx_ts_corr_vol_feature(const double* X, const double* C, double* Y, int64_t F, int64_t D, int64_t A,
                                   int64_t ld, int32_t window, void* stream);
/* The same feature straight from the returns in ONE pass (C5's chain: ts_corr of x with
 * Ycol feeding sign(corr) * x / ts_std(x, window), pipeline.ipynb's corr-vol signal): the
 * corr panel is neither written nor re-read.  Y is bit-identical to fmx_ts_corr (dense) +
 * fmx_ts_corr_vol_feature; C, when not NULL, also receives the corr.  Dense panels,
 * 1 <= window <= 4096, Ycol as in fmx_ts_corr (y_fstride 0: one [D][ld] return panel). */
fmx_status fmx_ts_corr_feature(const double* X, const double* Ycol, double* C, double* Y, int64_t F, int64_t D,
                               int64_t A, int64_t ld, int64_t y_fstride, int32_t window, void* stream);
/* cs_zscore (Yz) and market_neutralize (Yn) of the same rows from ONE set of moments
 * (operations.py:77-78, :171-182); optional stats[F][D][2] = (mean, std ddof=0).  Outputs
 * bit-identical to fmx_cs_moment of each op; distinct from X and each other. */
fmx_status fmx_cs_zscore_neutralize(const double* X, double* Yz, double* Yn, int64_t F, int64_t D, int64_t A,
                                    int64_t ld, const uint8_t* present, double* stats, void* stream);
/* cs_rank (operations.py:54-62): (rank - 1) / (rows - 1), rows counting NaN. */
fmx_status fmx_cs_rank(const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld, int32_t method,
                       const uint8_t* present, void* stream);

/* cs_rank(method='average') and cs_winsor(limits=(qlo, qhi)) of the same rows in ONE pass
 * (operations.py:54-68): the winsor quantiles' order statistics are read off the rank
 * histogram.  Outputs bit-identical to fmx_cs_rank / fmx_cs_winsor; distinct from X.
 * rank2 (optional, device fmx_rank2_t [F][D][ld], needs present == NULL and A <= 16384): the
 * doubled average rank of every non-NaN cell (2*#less + #equal + 1; 0 for NaN), the input
 * of fmx_ic_daily_ranked. */
fmx_status fmx_cs_rank_winsor(const double* X, double* Yrank, double* Ywinsor, int64_t F, int64_t D, int64_t A,
                              int64_t ld, double qlo, double qhi, const uint8_t* present, fmx_rank2_t* rank2,
                              void* stream);
/* cs_rank (average) + cs_winsor (qlo, qhi) + cs_zscore + market_neutralize of the same dense
 * rows in ONE pass (operations.py:54-68, :77-78, :171-182): each row is read once for the
 * four operators; every output is bit-identical to its own entry point (fmx_cs_rank_winsor,
 * fmx_cs_zscore_neutralize); rank2 as in fmx_cs_rank_winsor (or NULL).  Five distinct
 * panels.  Rows past the fused kernel (A > 16384) take the two two-output passes. */
fmx_status fmx_cs_rank_winsor_zn(const double* X, double* Yrank, double* Ywinsor, double* Yzscore, double* Yneutralize,
                                 int64_t F, int64_t D, int64_t A, int64_t ld, double qlo, double qhi,
                                 fmx_rank2_t* rank2, void* stream);
/* cs_rank, every method, for any row length (A <= 65535): rows sorted in HBM (rocPRIM
 * segmented radix sort of (value key, asset) pairs, stable), then one wave per row walks
 * its tie runs and scatters the ranks.  fmx_cs_rank takes 'first' / 'dense' up to A = 8192
 * (LDS bitonic) and the other methods up to 16384 (fine buckets); this entry has no such
 * limit.  work: fmx_cs_rank_sorted_work_bytes(F, D, A). */
fmx_status fmx_cs_rank_sorted(const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld, int32_t method,
                              const uint8_t* present, void* work, int64_t work_bytes, void* stream);
int64_t fmx_cs_rank_sorted_work_bytes(int64_t F, int64_t D, int64_t A);
/* cs_winsor (op 0) / cs_filter_center (op 1) (operations.py:64-75) for any row length
 * (A <= 65535): the numpy 'linear' order statistics read off the sorted rows.  work:
 * fmx_cs_rank_sorted_work_bytes(F, D, A). */
fmx_status fmx_cs_quantile_sorted(int32_t op, const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld,
                                  double qlo, double qhi, const uint8_t* present, void* work, int64_t work_bytes,
                                  void* stream);
/* group_rank_normalized (operations.py:152-168) for any group size and row length (A <=
 * 65535): rows sorted by (group, value) in two stable passes.  G, ngroups as fmx_group_op;
 * methods average / min / max / first / dense.  work: fmx_group_rank_sorted_work_bytes. */
fmx_status fmx_group_rank_sorted(const double* X, const int32_t* G, double* Y, int64_t F, int64_t D, int64_t A,
                                 int64_t ld, int32_t ngroups, int32_t method, const uint8_t* present, void* work,
                                 int64_t work_bytes, void* stream);
int64_t fmx_group_rank_sorted_work_bytes(int64_t F, int64_t D, int64_t A);
/* Only the doubled average ranks of fmx_cs_rank_winsor (rank2 [F][D][ld] fmx_rank2_t, A <=
 * 16384): the rank pass of a daily IC over raw factors (fmx_ic_daily_ranked) when no
 * operator output of the same rows is wanted (factor_selector.py:36-48's rankdata). */
fmx_status fmx_cs_rank2(const double* X, fmx_rank2_t* rank2, int64_t F, int64_t D, int64_t A, int64_t ld,
                        void* stream);
/* fmx_cs_rank_winsor_zn / fmx_cs_rank2 on the rows of dates [d0, d1) of every factor of an
 * [F][D][ld] panel (outputs at the same rows; other rows untouched).  The date-sharded step
 * runs the four operators on its owned dates while the halo exchange is in flight and the
 * doubled ranks of the halo rows after it (the daily IC reads exposures at t - lag).
 * Replaces the same reference functions as the two whole-panel entries
 * (operations.py:54-68, :77-78, :171-182; factor_selector.py:36-48).  A <= 16384. */
fmx_status fmx_cs_rank_winsor_zn_dates(const double* X, double* Yrank, double* Ywinsor, double* Yzscore,
                                       double* Yneutralize, int64_t F, int64_t D, int64_t A, int64_t ld, int64_t d0,
                                       int64_t d1, double qlo, double qhi, fmx_rank2_t* rank2, void* stream);
fmx_status fmx_cs_rank2_dates(const double* X, fmx_rank2_t* rank2, int64_t F, int64_t D, int64_t A, int64_t ld,
                              int64_t d0, int64_t d1, void* stream);
/* cs_winsor (operations.py:64-68); qlo/qhi are the fractions numpy sees
 * (pandas passes q*100 and numpy divides by 100). */
fmx_status fmx_cs_winsor(const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld, double qlo,
                         double qhi, const uint8_t* present, void* stream);
/* cs_filter_center (operations.py:70-75). */
fmx_status fmx_cs_filter_center(const double* X, double* Y, int64_t F, int64_t D, int64_t A, int64_t ld,
                                double qlo, double qhi, const uint8_t* present, void* stream);
/* group ops (operations.py:112-168).  G: device int32[D][ld] dense group ids, shared by
 * all F factors; an absent cell or a code outside [0, ngroups) (-1 = the NaN group)
 * belongs to no group: counted in none, output NaN.  Every output cell is written.
 * Rows up to 4096 assets: whole-row LDS sort; up to 16384: per-group compaction (the rank
 * sorts each group in LDS: groups of <= 8192 members, larger groups come out NaN --
 * factormodeling_amd.engine.group_op counts first and takes fmx_group_rank_sorted for
 * those).  Rank methods
 * average / min / max / first / dense. */
fmx_status fmx_group_op(int32_t op, const double* X, const int32_t* G, double* Y, int64_t F, int64_t D, int64_t A,
                        int64_t ld, int32_t ngroups, int32_t method, const uint8_t* present, void* stream);
/* group_mean / group_neutralize / group_normalize (operations.py:112-149) on rows of ANY
 * length up to 65,535 assets (fmx_group_op holds a row in registers: A <= 16384): rows
 * stay in HBM, each group's members are compacted in asset order into device scratch and
 * summed with numpy's pairwise schedule (bit-identical to fmx_group_op where both run).
 * Codes outside [0, ngroups) = no group.  work: fmx_group_op_long_work_bytes(F, D, A). */
int64_t fmx_group_op_long_work_bytes(int64_t F, int64_t D, int64_t A);
fmx_status fmx_group_op_long(int32_t op, const double* X, const int32_t* G, double* Y, int64_t F, int64_t D, int64_t A,
                             int64_t ld, int32_t ngroups, const uint8_t* present, void* work, int64_t work_bytes,
                             void* stream);
/* cs_regression (operations.py:248-304) for one [D][ld] pair. */
fmx_status fmx_cs_regression(const double* Yv, const double* Xv, double* Out, int64_t D, int64_t A, int64_t ld,
                             int32_t rettype, const uint8_t* present, void* stream);
/* elementwise over n contiguous doubles (operations.py:80-101). */
fmx_status fmx_elementwise(int32_t op, const double* X, double* Y, int64_t n, double a, double b, void* stream);
/* bucket (operations.py:104-110): pd.cut(right=True, include_lowest=True) label codes. */
fmx_status fmx_bucket(const double* X, int32_t* codes, int64_t n, const double* edges, int32_t n_edges,
                      void* stream);

/* ---- IC, metrics, selection (factor_selector.py:26-139, factor_selection_methods.py:6-26) */
/* Daily stats for each lag in lags[0..n_lags) (HOST int32 array, lags >= 0): pairs
 * (X[f][t-L], R[t]).  out: [n_lags][4][F][D] = (n_pairs, IC, rank_IC, beta); NaN where
 * undefined.  Each exposure row is ranked once for up to two lags. */
fmx_status fmx_ic_daily(const double* X, const double* R, int64_t F, int64_t D, int64_t A, int64_t ld,
                        const int32_t* lags, int32_t n_lags, double* out, void* stream);
/* Daily IC records for rows of ANY length up to 65,535 assets (the fine kernels' 16-bit
 * doubled ranks end at 16,384; factor_selector.py:36-48 has no limit): each (f, s) row
 * is sorted in HBM (rocPRIM segmented radix sort, chunks of rows), then one wave per row
 * ranks each lag's pair-valid subset off the sorted keys and reduces the same
 * (n, IC, rank IC, beta) records as fmx_ic_daily (out layout identical).  work:
 * fmx_ic_daily_sorted_work_bytes(F, D, A) bytes of device scratch. */
int64_t fmx_ic_daily_sorted_work_bytes(int64_t F, int64_t D, int64_t A);
fmx_status fmx_ic_daily_sorted(const double* X, const double* R, int64_t F, int64_t D, int64_t A, int64_t ld,
                               const int32_t* lags, int32_t n_lags, double* out, void* work, int64_t work_bytes,
                               void* stream);
/* fmx_ic_daily for a panel whose rows fmx_cs_rank_winsor already ranked (rank2): the
 * rank among each lag's pairs is rank2 corrected by the exposures whose return is NaN, so
 * no row is ranked again; one wavefront per row (single-pass shifted moments: records
 * agree with fmx_ic_daily to ~1e-15 relative, pair counts exactly).  work: device int32
 * scratch of fmx_ic_ranked_work_len(F, D) elements.  A <= 16384. */
int64_t fmx_ic_ranked_work_len(int64_t F, int64_t D);
fmx_status fmx_ic_daily_ranked(const double* X, const fmx_rank2_t* rank2, const double* R, int64_t F, int64_t D,
                               int64_t A, int64_t ld, const int32_t* lags, int32_t n_lags, int32_t* work,
                               int64_t work_len, double* out, void* stream);
/* cs_rank(method='average') + cs_winsor (operations.py:54-68) AND the daily IC of the same
 * rows (factor_selector.py:36-48: pearsonr, pearsonr(rankdata), beta of the pairs
 * (X[f][t-L], R[t])) in ONE pass: each row's ranks feed its IC records inside the
 * workgroup, so no rank panel is written or re-read.  Yrank / Ywinsor: both set (outputs
 * bit-identical to fmx_cs_rank_winsor) or both NULL (the IC's rank pass alone).  lags: HOST
 * int32[n_lags], n_lags 1 or 2; out as fmx_ic_daily (records agree with it to ~1e-15
 * relative, pair counts exactly).  rank2: device fmx_rank2_t [F][D][ld] scratch, written
 * only for rows with > 256 NaN returns (finished by the workgroup kernel of
 * fmx_ic_daily_ranked).  work: device int32 of fmx_rank_ic_work_len(F, D, A).  Dense rows
 * (no presence mask), A <= 16384. */
int64_t fmx_rank_ic_work_len(int64_t F, int64_t D, int64_t A);
fmx_status fmx_cs_rank_winsor_ic(const double* X, double* Yrank, double* Ywinsor, const double* R, int64_t F,
                                 int64_t D, int64_t A, int64_t ld, double qlo, double qhi, const int32_t* lags,
                                 int32_t n_lags, fmx_rank2_t* rank2, int32_t* work, int64_t work_len, double* out,
                                 void* stream);
/* Window summaries of one lag's daily stats [4][F][D] over J date windows [d0, d1).
 * out: [J][F][8] = IC, IC_IR, rank_IC, rank_IC_IR, tstat, n_beta, pct_pos, n_days. */
fmx_status fmx_ic_window(const double* daily, int64_t F, int64_t D, const int32_t* d0_dev, const int32_t* d1_dev,
                         int64_t J, double* out, void* stream);
/* icir_top_selector (factor_selection_methods.py:6-26) for J days of window metrics.
 * order_out [J][F] (rank_IC_IR-descending factor order), w_out [J][F] weights. */
fmx_status fmx_select_icir_top(const double* metrics, int64_t J, int64_t F, int32_t use_rank_icir,
                               double threshold, int32_t top_x, int32_t* order_out, double* w_out, void* stream);
/* mvo_selector (factor_selection_methods.py:60-175) for J windows of factor returns.
 * fret: [D][F] row-major device float64; window j is the rows [d0[j], d1[j]) (device int32).
 * fmx_mvo_covariance: mu_out [J][F] the window mean, cov_out [J][F][F] the Ledoit-Wolf
 * constant-correlation shrunk covariance (use_shrinkage) or the ddof=1 sample covariance,
 * lam_out [J] the shrinkage intensity (0 without shrinkage).  A window with n < 2 rows, bounds
 * outside [0, D] or a NaN / inf return is rejected: NaN mu / cov / lambda.
 * fmx_mvo_windows: the exact optimum of
 *   max_w mu'w - risk_aversion w'Sigma w - turnover_penalty |w - prev|_1,
 *   sum w = 1, 0 <= w <= min(max_weight, 1)
 * by ADMM (one workgroup per window).  prev: device [F] or NULL (no turnover term).  w_out
 * [J][F] (inside the box exactly; not re-normalised), info [J][6] = status (0 converged, 1
 * max_iter reached, 2 no solution: window rejected or F min(max_weight, 1) < 1, w = 0),
 * iterations, primal residual max(|x - z|_inf, |sum w - 1|), dual residual, lambda, rho.
 * 2 <= F <= 256. */
fmx_status fmx_mvo_covariance(const double* fret, int64_t D, int64_t F, const int32_t* d0_dev, const int32_t* d1_dev,
                              int64_t J, int32_t use_shrinkage, double* mu_out, double* cov_out, double* lam_out,
                              void* stream);
fmx_status fmx_mvo_windows(const double* fret, int64_t D, int64_t F, const int32_t* d0_dev, const int32_t* d1_dev,
                           int64_t J, double risk_aversion, double max_weight, double turnover_penalty,
                           const double* prev, int32_t use_shrinkage, int32_t max_iter, double eps, double* w_out,
                           double* info, void* work, int64_t work_bytes, void* stream);
int64_t fmx_mvo_windows_work_bytes(int64_t D, int64_t F, int64_t J);

/* ---- factor correlation GEMM (builder-defined) ------------------------ */
/* Z: per-date z-scored exposures (float64 [F][D][ld], NaN -> 0); M: validity as bf16
 * 0/1 (uint16 bit patterns [F][D][ld]).  stats: fmx_cs_moment_stats' [F][D][2] (mean, sd)
 * -- the oracle's numpy moments bit for bit -- or NULL for in-kernel block sums. */
fmx_status fmx_zscore_exposures(const double* X, const double* stats, double* Z, uint16_t* M, int64_t F, int64_t D,
                                int64_t A, int64_t ld, void* stream);
/* fmx_zscore_exposures for the dates [d0, d1) only: Z / M are [F][d1 - d0][ld] (chunked
 * Gram of a panel whose full Z / M would not fit next to X, e.g. C4 at 121 GB). */
fmx_status fmx_zscore_exposures_range(const double* X, const double* stats, double* Z, uint16_t* M, int64_t F,
                                      int64_t D, int64_t A, int64_t ld, int64_t d0, int64_t d1, void* stream);
/* G[F][F] (+)= sum_{d in [d0,d1), a} Z[i][d][a] Z[j][d][a] on fp64 MFMA
 * (v_mfma_f64_16x16x4_f64) and N[F][F] (+)= the same sum over M on bf16 MFMA (exact
 * pair counts).  accumulate = 0 overwrites.  M/N may be NULL. */
/* The wide-panel correlation Gram straight from the raw panel (builder-defined A19, C4's
 * 2000 x 2000): G = Z^T Z (fp64 MFMA, 128 x 128 tiles) with Z z-scored while each tile
 * chunk is staged from stats[F][D][2] (fmx_cs_moment_stats: numpy-pairwise mean / std
 * ddof=0; NaN -> 0, sigma 0 or NaN -> row 0), and N = M^T M as AND + popcount of validity
 * bits (exact).  No Z / M panels are materialised.  Dates [d0, d1); accumulate adds into
 * G / N.  work: fmx_gram_direct_work_bytes. */
int64_t fmx_gram_direct_work_bytes(int64_t F, int64_t D, int64_t A, int64_t d0, int64_t d1);
fmx_status fmx_gram_direct(const double* X, const double* stats, double* G, double* N, int64_t F, int64_t D,
                           int64_t A, int64_t ld, int64_t d0, int64_t d1, int32_t accumulate, void* work,
                           int64_t work_bytes, void* stream);
fmx_status fmx_gram(const double* Z, const uint16_t* M, double* G, double* N, int64_t F, int64_t D, int64_t A,
                    int64_t ld, int64_t d0, int64_t d1, int32_t accumulate, void* work, int64_t work_bytes,
                    void* stream);
/* Device workspace fmx_gram needs for these dims (with_mask: M and N given). */
int64_t fmx_gram_work_bytes(int64_t F, int64_t D, int64_t A, int64_t d0, int64_t d1, int32_t with_mask);
/* Fused form for F <= 256: G and N straight from the raw panel X with the row stats of
 * fmx_cs_moment_stats (z = (x - mean) / sd where x is non-NaN and sd > 0, else 0; M the
 * same validity), one pass over X, both MFMA products in the same workgroup.  stats ==
 * NULL: X already holds the z-scores (the fmx_cs_zscore output of the same rows: z is
 * used where finite, else 0 / invalid -- the same Z and M).  Returns
 * FMX_ERR_UNSUPPORTED for F > 256 (use fmx_zscore_exposures + fmx_gram). */
fmx_status fmx_gram_fused(const double* X, const double* stats, double* G, double* N, int64_t F, int64_t D,
                          int64_t A, int64_t ld, int64_t d0, int64_t d1, int32_t accumulate, void* work,
                          int64_t work_bytes, void* stream);
/* Device workspace fmx_gram_fused needs (per-slice partial tiles, validity bits, counts). */
int64_t fmx_gram_fused_work_bytes(int64_t F, int64_t D, int64_t A, int64_t d0, int64_t d1);
/* Exact, GPU-count-independent form of fmx_gram_fused (F <= 256) for the date-sharded
 * step (SURVEY 5 "bit-identical at 1/2/4/8 GPUs"; replaces the float sum of Gram partials
 * behind the builder-defined corr-prune, A19).  The dates [d0, d1) are cut into fixed
 * units (fmx_gram_exact_units_per_date(A) asset ranges per date), each unit's Z^T Z is
 * computed on fp64 MFMA and folded into a signed fixed-point accumulator (LSB 2^-64, 6 x
 * 32-bit payload limbs in int64 + an invalid-term flag): limbs [FMX_GRAM_EXACT_SLOTS][F][F]
 * (upper triangle), counts [F][F] int64 pair counts (upper triangle).  Both are plain
 * integer sums, so ranks add them with an int64 all-reduce (any order) and
 * fmx_gram_exact_finalize gives the same G and N bits at every GPU count.  accumulate = 0
 * zeroes limbs and counts first.  stats == NULL: X holds the z-scores (as fmx_gram_fused). */
#define FMX_GRAM_EXACT_SLOTS 7
fmx_status fmx_gram_exact(const double* X, const double* stats, int64_t* limbs, int64_t* counts, int64_t F,
                          int64_t D, int64_t A, int64_t ld, int64_t d0, int64_t d1, int32_t accumulate, void* work,
                          int64_t work_bytes, void* stream);
int64_t fmx_gram_exact_work_bytes(int64_t F, int64_t D, int64_t A, int64_t d0, int64_t d1);
/* fmx_gram_exact (z input only: X holds the z-scores) restricted to H <= 64 rows of the
 * panel, named by the device list rows int64 [H] (never read by the host: no sync before
 * the launch).  limbs [FMX_GRAM_EXACT_SLOTS][H][H] and counts [H][H] (upper triangles) are
 * indexed by position in the list; an index outside [0, F) is an all-invalid row.  Same
 * units, chunks and MFMA chain per unit as fmx_gram_exact, so every limb and count equals
 * that entry's for the same factor pair bit for bit, at any d0, d1 and any date split.
 * The panel rows are read in place (no gathered copy). */
fmx_status fmx_gram_exact_rows(const double* Z, const int64_t* rows, int64_t H, int64_t* limbs, int64_t* counts,
                               int64_t F, int64_t D, int64_t A, int64_t ld, int64_t d0, int64_t d1,
                               int32_t accumulate, void* work, int64_t work_bytes, void* stream);
int64_t fmx_gram_exact_rows_work_bytes(int64_t H, int64_t D, int64_t A, int64_t d0, int64_t d1);
/* The step's prune from a head block: C = N > 0 ? G / N : 0 of the (all-reduced) limbs
 * [FMX_GRAM_EXACT_SLOTS][H][H] / counts [H][H] of fmx_gram_exact_rows(order[0..H)), then
 * fmx_greedy_prune's walk over positions 0 .. min(H, n_order) - 1 (order entries outside
 * [0, F) are skipped), in one workgroup.  kept (int32 [min(top_x, H)], factor indices),
 * n_kept and done (int32 [1] each) are device buffers; done = n_kept == top_x or
 * H >= n_order: the walk of the whole order would return the same list.  H <= 64. */
fmx_status fmx_prune_head(const int64_t* limbs, const int64_t* counts, const int64_t* order, int64_t H,
                          int64_t n_order, int64_t F, double rho, int64_t top_x, int32_t* kept, int32_t* n_kept,
                          int32_t* done, void* stream);
/* Exact, GPU-count-independent form of fmx_gram_direct (any F; C4's 2000 x 2000 at
 * 2/4/8 GPUs, builder-defined A19).  The tile kernel's date slices are ABSOLUTE blocks of
 * FMX_GRAM_DATE_BLOCK dates (local row 0 of X is absolute date d_origin); each block's fp64
 * partial tiles fold into the same fixed-point limbs as fmx_gram_exact.  A date shard whose
 * bounds are multiples of FMX_GRAM_DATE_BLOCK holds whole blocks, so an int64 all-reduce of
 * limbs / counts + fmx_gram_exact_finalize gives the same G, N bits at every GPU count.
 * accumulate = 0 zeroes limbs and counts first.  work: fmx_gram_direct_exact_work_bytes.
 * Rows of 8..8192 assets: a z pass computes the row moments itself, writes
 * zero-filled z-scores for chunks of 32 date blocks into the workspace and an LDS-DMA tile
 * kernel multiplies them, so stats is ignored and may be NULL.  Other rows z-score while
 * staging from stats = fmx_cs_moment_stats (mean, std) [F][D][2]; NULL there computes them
 * into the workspace first. */
#define FMX_GRAM_DATE_BLOCK 16
fmx_status fmx_gram_direct_exact(const double* X, const double* stats, int64_t* limbs, int64_t* counts, int64_t F,
                                 int64_t D, int64_t A, int64_t ld, int64_t d0, int64_t d1, int64_t d_origin,
                                 int32_t accumulate, void* work, int64_t work_bytes, void* stream);
int64_t fmx_gram_direct_exact_work_bytes(int64_t F, int64_t D, int64_t A, int64_t d0, int64_t d1, int64_t d_origin);
/* G, N [F][F] (symmetric) from exact limbs / counts (N and counts may be NULL); a flagged
 * (non-finite or >= 2^127) term makes the entry NaN. */
fmx_status fmx_gram_exact_finalize(const int64_t* limbs, const int64_t* counts, double* G, double* N, int64_t F,
                                   void* stream);
int32_t fmx_gram_exact_units_per_date(int64_t A);
/* Host-side run of the same accumulator over n doubles (test hook; no GPU needed). */
void fmx_debug_exact_fold(const double* x, int64_t n, int64_t* limbs_out, double* value_out);
/* The step's greedy prune (builder-defined A19, the host walk of engine.greedy_prune): walk
 * order[0..n_order); factor f is kept iff max over the kept k of |C[f][k]| is NaN or < rho;
 * at most top_x kept.  C is the symmetric correlation matrix [F][ldc] on the device; kept
 * (int32 [top_x or F]) and n_kept (int32 [1]) are device buffers.  F <= 20480. */
fmx_status fmx_greedy_prune(const double* C, int64_t F, int64_t ldc, const int64_t* order, int64_t n_order,
                            double rho, int64_t top_x, int32_t* kept, int32_t* n_kept, void* stream);

/* The builder-defined corr_prune selector for J rolling windows in one call:
 * per-date Gram partials of the raw panel X (z-scored with stats [F][D][2] from
 * fmx_cs_moment_stats) for every date any window touches, then per window j the pooled
 * G / N over raw dates [s0_host[j], s0_host[j] + window) (the lag-1 factors of the window's
 * dates) and the greedy walk of order [J][F] (metrics [J][F][8] column rank_IC_IR or IC_IR
 * > threshold; keep iff |C| < rho against every kept factor; up to top_x).  w_out [J][F] =
 * 1 / #kept on the kept factors.  F <= 256. */
fmx_status fmx_corr_prune_windows(const double* X, const double* stats, int64_t F, int64_t D, int64_t A, int64_t ld,
                                  int64_t J, int32_t window, const int32_t* s0_host, const int32_t* order,
                                  const double* metrics, int32_t use_rank_icir, double threshold, double rho,
                                  int32_t top_x, double* w_out, void* work, int64_t work_bytes, void* stream);
/* Device workspace fmx_corr_prune_windows needs (per-date partials of the touched dates). */
int64_t fmx_corr_prune_windows_work_bytes(int64_t F, int64_t D, int64_t J, int32_t window, const int32_t* s0_host);

/* ---- composite factors (composite_factor.py:137-342) ------------------------------- */
/* composite_factor_calculation preprocessing (:157-178): Adj[k] = suffix-scaled X[cols[k]]
 * with per-(column, date) numpy linear nanpercentiles.  suffix codes 0 none, 1 _eq,
 * 2 _flx, 3 _long, 4 _short; qlo/qhi: device double[5] percentile fractions per code. */
fmx_status fmx_comp_adj(const double* X, const int32_t* cols_dev, const int32_t* suffix_dev, const double* qlo_dev,
                        const double* qhi_dev, double* Adj, int64_t K, int64_t D, int64_t A, void* stream);
/* prefix-group proxies (:181-190): skipna mean over the columns gcols[goff[g]..goff[g+1]). */
fmx_status fmx_comp_proxy(const double* Adj, const int32_t* gcols_dev, const int32_t* goff_dev, double* Prox,
                          int64_t G, int64_t D, int64_t A, void* stream);
/* combine normalised proxies (mode 0 skipna mean / 1 skipna sum) and demean (:204-216). */
fmx_status fmx_comp_combine(const double* Nrm, int64_t G, int64_t D, int64_t A, int32_t mode,
                            const uint8_t* present, double* Out, void* stream);
/* weighted_composite_factor (:220-342): pooled suffix percentiles per selection row j
 * (columns scol[soff[4j+s-1] .. soff[4j+s]) for suffix s=1..4); lohi[J][4][3] = lo, hi, n. */
fmx_status fmx_wcomp_pct(const double* X, const int32_t* pdate, const int32_t* soff, const int32_t* scol, int64_t J,
                         int64_t D, int64_t A, const double* qlo_dev, const double* qhi_dev, double* lohi,
                         void* stream);
/* per-row prefix-group proxies Prox[G][J][A] from the row plan (ncol, col, suf, grp). */
fmx_status fmx_wcomp_proxy(const double* X, const int32_t* pdate, const int32_t* ncol, const int32_t* col,
                           const int32_t* suf, const int32_t* grp, int32_t KMAX, int64_t J, int64_t D, int64_t A,
                           const double* lohi, int64_t G, double* Prox, void* stream);
/* weighted sum of normalised proxies (Python sum, NaN propagates), demean, NaN -> 0,
 * written to Out[pdate[j]][:]. */
fmx_status fmx_wcomp_combine(const double* Nrm, const int32_t* pdate, const int32_t* ngrp, const double* gw,
                             int32_t KMAX, int64_t J, int64_t D, int64_t A, const uint8_t* present, double* Out,
                             void* stream);

/* ---- daily trade list (portfolio_simulation.py:96-170, method 'equal') ------------ */
/* Replaces Simulation._daily_trade_list with _calculate_equal_weights (:156-170) and
 * _normalize_legs (:250-262) over one [D][A] signal panel X (present [D][A] or NULL):
 * Wraw = same-day weights (NaN on absent cells), Wout = per-symbol shift(1) of Wraw
 * over present rows (:151-152), counts [D][2] = (long_count, short_count), NaN on dates
 * with no present row.  A <= 16384. */
fmx_status fmx_trade_equal(const double* X, const uint8_t* present, double* Wraw, double* Wout,
                           double* counts, int64_t D, int64_t A, double pct, void* stream);
/* Method 'linear' (portfolio_simulation.py:172-181): the signal on its positive / negative
 * cells, _normalize_legs (:250-262) and _cap_and_redistribute(max_weight, 10, 1e-6)
 * (:264-313), every pandas sum a numpy pairwise sum over its subset in symbol order
 * (bit-identical); counts = (len(pos), len(neg)).  Same layout as fmx_trade_equal. */
fmx_status fmx_trade_linear(const double* X, const uint8_t* present, double* Wraw, double* Wout,
                            double* counts, int64_t D, int64_t A, double max_weight, void* stream);
/* F trade books in one launch (multi_manager.py:41-49: one manager per factor): X, Wraw,
 * Wout [F][D][A], counts [F][D][2]; method 0 = equal (pct), 1 = linear (max_weight);
 * present [D][A] shared (or NULL); nan_absent = 1 treats NaN cells as no row
 * (factors_df[fac].dropna()). */
fmx_status fmx_trade_books(int32_t method, const double* X, const uint8_t* present, int32_t nan_absent,
                           double* Wraw, double* Wout, double* counts, int64_t F, int64_t D, int64_t A,
                           double pct, double max_weight, void* stream);
/* Per-symbol shift(1) over the present rows of F same-day books W [F][D][A] (present
 * cells are never NaN in a book, absent ones always are): out[f][d][a] = the book's value
 * on the symbol's previous present row (portfolio_simulation.py:151-152). */
fmx_status fmx_shift_rows(const double* W, double* out, int64_t F, int64_t D, int64_t A, void* stream);
/* Replaces multi_manager.compute_multimanager_weights' combination loop (:51-72): Wf
 * [F][D][A] shifted manager books and counts [F][D][2] (NaN on dates a manager has no
 * rows) from fmx_trade_equal; fw [Dw][Fw] factor weights, colmap [Fw] column -> manager
 * (-1: no such factor), wdate [Dw] -> date index.  out [Dw][A], out_counts [Dw][2]. */
fmx_status fmx_mm_combine(const double* Wf, const double* counts, const double* fw, const int32_t* colmap,
                          const int32_t* wdate, double* out, double* out_counts, int64_t Fw, int64_t Dw,
                          int64_t D, int64_t A, void* stream);
/* Method 'mvo' (portfolio_simulation.py:96-154, :183-204, :315-461): the same-day minimum-
 * variance books of J dates in one launch, one workgroup per date (csrc/sim_mvo.hip).
 *   R0 [Dr][A]: the returns panel, missing cells and NaN as 0 (unstack().fillna(0), :337);
 *   win_rows [J][Lmax], win_T [J] (device int32): date j's window is the rows
 *     win_rows[j][0 .. win_T[j]) of R0 -- the last lookback_period distinct returns dates
 *     before it on which one of its symbols has a row (:319-334); 1 <= Lmax <= 64;
 *   X [J][A] the signal, present [J][A] (or NULL: every cell is a row).
 * Per date: Sigma = (1 - s) (cov(ddof=1) + 1e-6 I) + s avg_var I with avg_var the mean
 * diagonal over the PRESENT symbols (:349-374; s = shrinkage <= 0: no shrinkage), then
 *   min w'Sigma w,  sum_{x>0} w = 1, sum_{x<0} w = -1, 0 <= w <= u on x > 0,
 *   -u <= w <= 0 on x < 0, w = 0 elsewhere                      (u = max_weight, :376-421)
 * by ADMM with a Woodbury x-step (Sigma = delta I + low rank).  W [J][A]: the weights, 0 on
 * present cells outside the legs, NaN on absent cells (the layout fmx_shift_rows takes);
 * counts [J][2] = (long_count, short_count); info [J][6] = status, iterations, primal
 * residual max(|x - z|_inf, leg-sum errors), dual residual rho |z - z_prev|_inf relative to the
 * larger leg multiplier (the gradient's size), delta, rho.  status: 0 converged (|x - z|_inf
 * <= eps, leg sums within eps / 10, relative dual residual <= eps), 1 max_iter reached
 * (last iterate, inside the box exactly), 2 the x0 fallback +1/n_pos, -1/n_neg (:388-390,
 * :451-459: T = 1, u n_pos < 1 or u n_neg < 1, non-finite window), 3 flat day (a leg empty or
 * fewer than 2 rows, :109-126: zeros, counts 0), 4 no returns history (win_T = 0, :188-190:
 * the caller supplies the equal-weight book; zeros, counts 0).  A row index outside [0, Dr)
 * or win_T outside [0, Lmax] is FMX_ERR_ARG (the lists are read back before the launch).
 * A <= 16384.  work: fmx_sim_mvo_books_work_bytes(A, Lmax, J) bytes (0 unless the A-vector
 * and the Lmax x Lmax matrix exceed the LDS together). */
int64_t fmx_sim_mvo_books_work_bytes(int64_t A, int64_t Lmax, int64_t J);
fmx_status fmx_sim_mvo_books(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows, const int32_t* win_T,
                             int64_t Lmax, const double* X, const uint8_t* present, int64_t J, double shrinkage,
                             double max_weight, int32_t max_iter, double eps, double* W, double* counts,
                             double* info, void* work, int64_t work_bytes, void* stream);
/* Method 'mvo_turnover' (portfolio_simulation.py:96-154, :206-248, :463-585): B independent
 * chains of J dates over one returns panel (csrc/sim_mvo_turnover.hip).  Per date, with Sigma,
 * the legs, the exits and the status codes of fmx_sim_mvo_books,
 *   min w'Sigma w + tau sum_i |w_i - p_i| - r sum_i x_i w_i   under the same constraints,
 * tau = turnover_penalty >= 0, r = return_weight (finite; either is FMX_ERR_ARG otherwise).
 * p is the chain's last book, whatever kind of day produced it, aligned to today's rows: 0
 * where the symbol had no row on the previous date, all zeros on the first date.  A set-up
 * kernel prepares what does not depend on p for all B * J dates at once; a second kernel,
 * one workgroup per chain, solves the dates in order (ADMM with a soft-threshold z-step and
 * the dual started at +-tau / rho), then applies the reference's post-solve step (:553-573)
 * on solved days: |w| < 1e-6 -> 0 per leg and, when both leg sums stay > 0, each leg divided
 * by its (exactly rounded) sum.  No host synchronisation between dates.
 *   R0, win_rows, win_T, Lmax: as fmx_sim_mvo_books, shared by the chains;
 *   X [B][J][A], present [B][J][A] or NULL;
 *   W [B][J][A] in/out: the row of a status-4 date (win_T = 0 and both legs present) arrives
 *     holding the caller's equal-weight book and is read as the next date's p; every other row
 *     is written (0 on present cells outside the legs, NaN on absent cells);
 *   Wopt [B][J][A] or NULL: the solver's z before the post-solve step -- exactly p_i on cells
 *     that did not move, exactly 0 or +-min(u, 1) at the box ends; the book itself on days
 *     without a solve;
 *   counts [B][J][2] (0, 0 on status 3 and 4), info [B][J][6] as fmx_sim_mvo_books, the dual
 *     residual relative to |2 Sigma x - r x_sig|_inf.
 * work: fmx_sim_mvo_turnover_books_work_bytes(A, Lmax, J, B) bytes, always needed. */
int64_t fmx_sim_mvo_turnover_books_work_bytes(int64_t A, int64_t Lmax, int64_t J, int64_t B);
fmx_status fmx_sim_mvo_turnover_books(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows,
                                      const int32_t* win_T, int64_t Lmax, const double* X, const uint8_t* present,
                                      int64_t J, int64_t B, double shrinkage, double max_weight,
                                      double turnover_penalty, double return_weight, int32_t max_iter, double eps,
                                      double* W, double* Wopt, double* counts, double* info, void* work,
                                      int64_t work_bytes, void* stream);
/* fmx_sim_mvo_turnover_books with per-chain window tables and per-chain date lists: the B
 * chains are the managers of multi_manager.compute_multimanager_weights, each over its own
 * dropna() rows of one (date, symbol) grid.
 *   win_rows [.][Lmax], win_T [.]: win_stride is the number of table rows between two chains'
 *     tables -- 0: one [J] table shared by the chains, J: [B][J] tables, chain b's date j at
 *     row b * J + j.  Every row read is range-checked before the launch, as above.
 *   skip_absent != 0: a (chain, date) without a present cell is not a date of that chain: its
 *     W / Wopt row is NaN, its counts are NaN, info[0] = 5, and the chain's book is left as it
 *     was, so the next date's p is the book of the last date on which the chain had rows
 *     (the reference iterates the manager's own dates, portfolio_simulation.py:100, :206-225).
 *     A date with one present row stays a flat day (status 3): its zero book is the next p.
 *   skip_absent == 0 and win_stride == 0 are fmx_sim_mvo_turnover_books, bit for bit.
 * work: fmx_sim_mvo_turnover_chains_work_bytes(A, Lmax, J, B) bytes. */
int64_t fmx_sim_mvo_turnover_chains_work_bytes(int64_t A, int64_t Lmax, int64_t J, int64_t B);
fmx_status fmx_sim_mvo_turnover_chains(const double* R0, int64_t Dr, int64_t A, const int32_t* win_rows,
                                       const int32_t* win_T, int64_t Lmax, int64_t win_stride, const double* X,
                                       const uint8_t* present, int64_t J, int64_t B, double shrinkage,
                                       double max_weight, double turnover_penalty, double return_weight,
                                       int32_t max_iter, double eps, int32_t skip_absent, double* W, double* Wopt,
                                       double* counts, double* info, void* work, int64_t work_bytes, void* stream);
/* The returns windows of N (manager, date) rows (portfolio_simulation.py:319-334;
 * csrc/sim_mvo_windows.hip): row n's window is the last Lmax returns dates r < nbefore[n] on
 * which at least one symbol present in fpresent[n] has a returns row.
 *   fpresent [N][A], rpresent [Dr][A] (uint8, nonzero = present; rpresent may be NULL when
 *   Dr = 0), nbefore [N] (device int32): the number of returns dates before the row's date,
 *   0 <= nbefore <= Dr (read back and checked: FMX_ERR_ARG otherwise);
 *   win_rows [N][Lmax] ascending, the unused tail 0; win_T [N] the window lengths.
 * 1 <= A <= 16384, 1 <= Lmax <= 64.  work: fmx_sim_mvo_window_rows_work_bytes(N, A, Dr) bytes
 * (both masks packed to 64-bit words). */
int64_t fmx_sim_mvo_window_rows_work_bytes(int64_t N, int64_t A, int64_t Dr);
fmx_status fmx_sim_mvo_window_rows(const uint8_t* fpresent, const uint8_t* rpresent, const int32_t* nbefore,
                                   int64_t N, int64_t A, int64_t Dr, int64_t Lmax, int32_t* win_rows, int32_t* win_T,
                                   void* work, int64_t work_bytes, void* stream);

/* ---- factor risk model (builder-defined) ------------------------------- */
/* Sigma_d = B_d' F_d B_d + diag(s2_d) over the symbols present on date d: B [K][D][A] the
 * exposures (a non-finite exposure and an absent symbol count as 0), Fc [D][K][K] the factor
 * covariance (the lower triangle is read), S2 [D][A] the specific variances, 1 <= K <= 32.
 * Predicted risk and attribution of M books W [M][D][A] (a NaN cell is not held: 0)
 * (csrc/risk_model.hip):
 *   var [M][D][3] = (total, factor = b'F b with b = B w, specific = sum w^2 s2);
 *   expo [M][D][K] = b;  contrib [M][D][K] = b_k (F b)_k (their sum over k is the factor variance);
 *   marginal [M][D][A] or NULL = (Sigma w)_a = sum_k B_ka (F b)_k + s2_a w_a, NaN on absent cells.
 * present [D][A] or NULL (every cell is a row); valid [D] (uint8) or NULL: a date with
 * valid[d] == 0 is NaN in every output.  Every sum runs in a fixed order that depends on
 * neither M nor D: a book has the same bits alone or in a batch, a date alone or in a panel.
 * The exposures of a date are read once per 16 books (once more for marginal). */
fmx_status fmx_risk_books(const double* B, const double* Fc, const double* S2, const double* W, const uint8_t* present,
                          const uint8_t* valid, int64_t K, int64_t D, int64_t A, int64_t M, double* var, double* expo,
                          double* contrib, double* marginal, void* stream);
/* fmx_sim_mvo_books' QP -- the same constraints, box, counts, info [J][6] and status codes --
 * against the factor model (csrc/sim_mvo_risk.hip): book j is optimised under
 * Sigma = diag(S2[r]) + B[.][r]' Fc[r] B[.][r] on its active cells, r = model_row[j].
 *   B [K][Dm][A], Fc [Dm][K][K], S2 [Dm][A]: the model's Dm dates, 1 <= K <= 32, A <= 16384;
 *   model_row [J] (device int32): -1 = no model for book j -> status 4 (zeros, counts 0; the
 *     caller supplies the equal-weight book).  Read back and checked before the launch: an
 *     entry outside [-1, Dm) is FMX_ERR_ARG;
 *   X [J][A] the signal, present [J][A] or NULL.
 * ADMM with a Woodbury x-step over a per-asset diagonal and a K x K core.  status 2 (x0)
 * also covers a non-finite or negative S2 on an active cell, a non-finite Fc entry and an Fc
 * that is not positive semidefinite.  info[4] = min S2 over the active cells, info[5] = rho.
 * The K x K matrices live in LDS: fmx_risk_mvo_books_work_bytes is 0 and no workspace is taken. */
int64_t fmx_risk_mvo_books_work_bytes(int64_t A, int64_t K, int64_t J);
fmx_status fmx_risk_mvo_books(const double* B, const double* Fc, const double* S2, int64_t K, int64_t Dm, int64_t A,
                              const int32_t* model_row, const double* X, const uint8_t* present, int64_t J,
                              double max_weight, int32_t max_iter, double eps, double* W, double* counts, double* info,
                              void* stream);
/* fmx_risk_mvo_books with the book also neutral to factors of the model: on the
 * active cells B_k . w = 0 for every factor k whose bit is set in neutral_mask (a bit at or
 * above K is FMX_ERR_ARG; B read as above).  The rows enter the x-step exactly through K x K
 * algebra.  A neutral row with no exposure on the active cells, or dependent on the legs and
 * the rows before it, is dropped; a non-finite or indefinite system of the rows is status 2.
 * Status 0 also needs |B_k . w| <= eps max|B_k| for every k of the mask.  Neutrality can make
 * the constraints infeasible; no test is made: such a date ends with status 1 at max_iter.
 *   expo [J][K] or NULL: B . w of the returned row over all K factors (NaN on status 3 / 4).
 * neutral_mask == 0 is fmx_risk_mvo_books itself (the same kernel, the same bytes).  The
 * set-up runs in LDS: the work_bytes function returns 0 and work is not read. */
int64_t fmx_risk_mvo_neutral_books_work_bytes(int64_t A, int64_t K, int64_t J);
fmx_status fmx_risk_mvo_neutral_books(const double* B, const double* Fc, const double* S2, int64_t K, int64_t Dm,
                                      int64_t A, const int32_t* model_row, const double* X, const uint8_t* present,
                                      int64_t J, uint32_t neutral_mask, double max_weight, int32_t max_iter, double eps,
                                      double* W, double* counts, double* info, double* expo, void* work,
                                      int64_t work_bytes, void* stream);

/* ---- portfolio P&L (portfolio_simulation.py:748-819) ---------- */
/* Replaces Simulation._daily_portfolio_returns' per-date sums on the aligned [D][A] grid
 * (union of the weights' and returns' dates/symbols; NaN cells count as 0 as after
 * unstack().fillna(0)): W shifted weights, R returns, CAP cap flags (or NULL: no cost),
 * wprev [D] = row of the previous weights date (-1: none).  out [D][6] = (sum longs*r,
 * sum shorts*r, long turnover, short turnover, long cost, short cost); contrib [A][2]
 * (optional) = per-symbol long / short P&L net of cost (contributor=True, :790-793). */
fmx_status fmx_pnl_daily(const double* W, const double* R, const double* CAP, const int32_t* wprev, double* out,
                         double* contrib, int64_t D, int64_t A, void* stream);
/* The six sums of fmx_pnl_daily (portfolio_simulation.py:748-797) for F books in one launch.
 * Wraw [F][D][A] holds the SAME-DAY books (the raw output of fmx_trade_books: finite where
 * the feature has a row, NaN elsewhere); the per-symbol shift(1) is folded into the read,
 * so no shifted copy is made.  R, CAP (or NULL: no cost) [D][A] and wprev [D] are as in
 * fmx_pnl_daily and shared by all books.
 *   prev_row [D][A] (device int32), shared by all books: p >= 0 = the cell has a feature row
 *     and its shifted weight is Wraw[f][p][a]; -1 = the shifted weight is 0 (no row, or the
 *     symbol's first row); NULL = the dense grid (p = d - 1, -1 at d = 0).  The table and
 *     wprev are read back before the launch: a prev_row entry outside [-1, d) or a wprev
 *     entry outside [-1, D) is FMX_ERR_ARG.
 * out [F][D][6]: out[f] holds the same bits as fmx_pnl_daily on book f of
 * fmx_shift_rows(Wraw) (the same per-lane order, shuffle tree and wave order per date). */
fmx_status fmx_pnl_books(const double* Wraw, const double* R, const double* CAP, const int32_t* prev_row,
                         const int32_t* wprev, double* out, int64_t F, int64_t D, int64_t A, void* stream);
/* Replaces _calculate_metrics' daily IC (:799-805): per date, Series.corr (np.corrcoef) of
 * the pair-valid (X, R) cells.  out [D][2] = (n, corr); corr NaN for n < 2 or constant. */
fmx_status fmx_daily_corr(const double* X, const double* R, double* out, int64_t D, int64_t A, void* stream);

/* ---- quantile backtest (composite_factor.py:47-134; csrc/qbacktest.hip) ------------ */
/* The per-date bucket of every cell (composite_factor.py:71-77: pd.qcut of the date's
 * rank(method="first") into n_groups bins, group = n_groups - label, 1 = top).  Per
 * (factor, date) row, m = number of present non-NaN cells; the ordinal rank r in 1..m
 * breaks ties by the lower asset column; the label is the first k with cum[row][k] >= r.
 *   cum [M][n_groups] (device int32): row j holds, for one m, the number of ranks 1..m
 *     whose qcut label is <= k -- filled on the host from pandas' own bin edges;
 *   m_index [A + 1] (device int32): the row of cum for every m, or -1.
 * labels [F][D][A] uint8 (dense): 0 = none (absent, NaN, or m <= 1), else the group; a row
 * whose m has no table row gets 255 on its valid cells (fmx_qbucket_mean then counts none
 * of them: 255 is outside 1..n_groups).  2 <= n_groups <= 32, A <= 8192. */
fmx_status fmx_cs_qlabel(const double* X, const uint8_t* present, const int32_t* cum, const int32_t* m_index,
                         uint8_t* labels, int64_t F, int64_t D, int64_t A, int64_t ld, int32_t n_groups,
                         void* stream);
/* The mean return of every (date, group) (composite_factor.py:79-98: the groups shifted one
 * row per symbol, joined with the returns, group-by mean).  Cell (d, a) of factor f belongs
 * to group labels[f][prev_row[d][a]][a]; it is kept when that group is in 1..n_groups and
 * R[d][a] is not NaN (rpresent [D][A], or NULL, marks the returns cells that exist).
 *   prev_row [D][A] (device int32): the symbol's previous row of the feature index, -1 =
 *     none or not a feature row; NULL = the dense grid (row d - 1).  The table is read back
 *     before the launch: an entry outside [-1, D) is FMX_ERR_ARG.
 * mean [F][D][n_groups] (NaN for an empty group), count [F][D][n_groups] int32.  The sums
 * are fixed-point integers (exactsum.hpp on returns scaled by 2^48: exact for every term of
 * magnitude >= 2^-60, smaller terms truncated at 2^-112; the conversion back to double may
 * round more than once), so the outputs do not depend on the launch geometry, the split of
 * the factors over workgroups or dense-vs-gather addressing.  Returns of magnitude >= 2^79, or non-finite,
 * make their group's mean NaN.  2 <= n_groups <= 32, A <= 8192. */
fmx_status fmx_qbucket_mean(const uint8_t* labels, const double* R, const uint8_t* rpresent, const int32_t* prev_row,
                            double* mean, int32_t* count, int64_t F, int64_t D, int64_t A, int32_t n_groups,
                            void* stream);

/* ---- per-date multi-factor OLS (builder-defined) ---------------------- */
/* For every (y column f, date d): weighted least squares of Y[f][d][:] on the K columns
 * X[:][d][:] over the VALID rows -- present, Y finite, all K X finite and, with W, W finite
 * and > 0.  n = #valid rows, p = K + intercept; n < p makes every output of (f, d) NaN but n.
 * With an intercept the columns are centred on their weighted means; G = Xc' W Xc is scaled
 * to unit diagonal by s_k = sqrt(G_kk) and factored by a Cholesky in column order.  Column k
 * is DROPPED (beta NaN, no contribution to fitted) when s_k == 0, when (intercept only)
 * s_k <= 1e-13 sqrt(sum w x_k^2), or when its pivot after eliminating the kept columns
 * before it is < 1e-10.  alpha = ybar - sum_kept beta_k xbar_k (NaN without an intercept);
 * r2 = 1 - SSR / SST, both weighted, SST centred iff intercept, NaN if SST == 0.
 *   Y [Fy][D][ld], X [K][D][ld], W [D][ld] or NULL, present [D][ld] or NULL;
 *   beta [Fy][D][K], alpha / r2 [Fy][D], n [Fy][D] int32, resid / fitted [Fy][D][ld] (NaN
 *   on rows that are not valid).  Any output pointer may be NULL.
 * Sums run in a fixed order that depends on (K, n) only: a column's bits do not depend on
 * the other columns of the batch, nor on the run.  1 <= K <= 32 and A <= 16384; anything
 * else is FMX_ERR_ARG before any launch. */
fmx_status fmx_cs_ols(const double* Y, const double* X, const double* W, const uint8_t* present, int64_t Fy,
                      int64_t K, int64_t D, int64_t A, int64_t ld, int32_t intercept, double* beta, double* alpha,
                      double* r2, int32_t* n, double* resid, double* fitted, void* stream);

/* ---- rolling multi-factor OLS (builder-defined) ----------------------- */
/* For every (y column f, asset a, date d): least squares of the column's last `window`
 * VALID rows ending at d on K regressors.  Row t of column (f, a) is valid when it is present,
 * Y[f][t][a] is finite and all K regressors of the row are finite; invalid rows drop out of the
 * column's sequence (dropna, then roll over the surviving rows, per symbol).  An output exists
 * where row d is valid and the column has `window` valid rows up to and including d; every
 * output is NaN elsewhere (a window longer than the panel gives all NaN).  The fit is
 * fmx_cs_ols's with unit weights: means, columns centred in a second pass, G = Xc'Xc scaled to
 * unit diagonal, Cholesky in column order; column k is DROPPED (beta NaN, no contribution) when
 * s_k == 0, when (intercept only) s_k <= 1e-13 sqrt(sum x_k^2), or when its pivot is < 1e-10.
 *   Y [Fy][D][ld]; X [K][D][ld], or with shared != 0 a table [K][D] (the same regressors for
 *   every symbol, e.g. factor returns); present [D][ld] or NULL.
 *   beta [Fy][K][D][ld]; alpha (NaN without an intercept), fitted and resid (row d under the
 *   coefficients of the window ending at d), r2 = 1 - SSR / SST over the window (SST centred
 *   iff intercept, NaN if SST == 0) and sigma = sqrt(SSR / (window - p_kept)) (p_kept = kept
 *   columns + intercept; NaN unless window > p_kept): all [Fy][D][ld].  Any may be NULL.
 *   work: Fy * D * ld bytes of device memory (one validity byte per cell).
 * Every sum runs over the window oldest row first: a column's bits do not depend on the other
 * columns of the batch, on the launch or on the run, and a shared table gives the bits of the
 * same table broadcast to a panel.  1 <= K <= 8, window >= K + intercept, ld >= A, D < 2^31,
 * non-null panels; anything else is FMX_ERR_ARG before any launch. */
fmx_status fmx_ts_ols(const double* Y, const double* X, const uint8_t* present, int64_t Fy, int64_t K, int64_t D,
                      int64_t A, int64_t ld, int32_t window, int32_t intercept, int32_t shared, double* beta,
                      double* alpha, double* fitted, double* resid, double* r2, double* sigma, uint8_t* work,
                      void* stream);

/* ---- performance statistics (portfolio_analyzer.py:9-81) ---------------- */
/* Replaces the numbers of PortfolioAnalyzer (average_return ... min_daily_return, the
 * cumulative and drawdown curves, monthly_return / yearly_return) for K series at once.
 * Layout: R is [K][ld], ONE SERIES CONTIGUOUS (series k occupies R[k * ld .. k * ld + T)), the
 * transpose of a dates x K table: a workgroup owns a series and reads it with unit stride.
 * R holds SIMPLE returns (exp(log_return) - 1, taken on the host); NaN = no observation;
 * +-inf is not pinned.  cum and dd are [K][ld] like R, either may be NULL (not written).
 * Everything is pandas' own operation sequence on the series alone (pandas 2.3 without
 * bottleneck), bit-identical as values, and does not depend on K or on the other series:
 *   cum[t]  = cumprod of 1 + R over the non-NaN rows up to t, minus 1; NaN on a NaN row
 *   dd[t]   = (cum[t] + 1) / peak[t] - 1, peak = cummax of cum + 1 over the non-NaN rows
 * stats is [FMX_PERF_NSTAT][K] (stat s of series k at stats[s * K + k]):
 *   MEAN, STD      Series.mean() / .std() (ddof 1) of R: numpy pairwise sums over the T
 *                  NaN -> 0 masked values / count, then of (avg - v) * (avg - v) / (count - 1)
 *   MAX, MIN       over the non-NaN rows;  COUNT  the number of non-NaN rows
 *   EX_MEAN, EX_STD          the same mean / std of E = R - rf_daily
 *   DOWN_COUNT, _MEAN, _STD  count, mean, std of the compacted E[E < 0] (date order), summed
 *                  on numpy's pairwise schedule of ITS OWN length (Sortino's downside std)
 *   FINAL          cum[T - 1] + 1 (NaN when the last row is NaN, as .iloc[-1] gives)
 *   MAXDD          nanmin(dd)
 *   MAXDD_ROW      builder-defined: the row of that minimum, first occurrence (-1: no row)
 *   MAXDD_PEAK_ROW builder-defined: the earliest row at which the peak in force at MAXDD_ROW
 *                  was attained (-1: no row)
 *   DD_RUN         builder-defined: the longest run of non-NaN rows with dd < 0; NaN rows
 *                  neither count nor break a run
 * A count of 0 gives a NaN mean, max, min and MAXDD; a count of 0 or 1 a NaN std; a zero std
 * is returned as 0 (the caller's ratio is then IEEE's +-inf or NaN).  Counts and rows are exact
 * integers stored as doubles.  The ratios (Sharpe, Sortino), sqrt(trading days) and the
 * annualising power final ** (1 / years) are the caller's host arithmetic.
 * T <= FMX_PERF_TMAX (the downside series and the curve are staged in T doubles of LDS).  No
 * scratch, no allocation (but the one-time pairwise schedule cache).  Null R or stats, K < 1,
 * T < 1, ld < T, T > FMX_PERF_TMAX and cum / dd aliasing R or each other are refused before
 * any device work. */
#define FMX_PERF_TMAX 16384
#define FMX_PERF_MEAN 0
#define FMX_PERF_STD 1
#define FMX_PERF_MAX 2
#define FMX_PERF_MIN 3
#define FMX_PERF_COUNT 4
#define FMX_PERF_EX_MEAN 5
#define FMX_PERF_EX_STD 6
#define FMX_PERF_DOWN_COUNT 7
#define FMX_PERF_DOWN_MEAN 8
#define FMX_PERF_DOWN_STD 9
#define FMX_PERF_FINAL 10
#define FMX_PERF_MAXDD 11
#define FMX_PERF_MAXDD_ROW 12
#define FMX_PERF_MAXDD_PEAK_ROW 13
#define FMX_PERF_DD_RUN 14
#define FMX_PERF_NSTAT 15
fmx_status fmx_perf_stats(const double* R, int64_t K, int64_t T, int64_t ld, double rf_daily, double* stats,
                          double* cum, double* dd, void* stream);

/* Period returns (portfolio_analyzer.py:62-68, resample(...).apply(lambda x: (1 + x).prod() - 1))
 * of the same [K][ld] table.  seg is a DEVICE int32[T]: the bucket of each row, non-decreasing,
 * in [0, nseg) (calendar months or years counted from the first date's, built by the caller).
 * out is [nseg][K]: out[s * K + k] = the left-to-right product of 1 + R over the bucket's
 * non-NaN rows, minus 1; a bucket with no row, or only NaN rows, gives exactly 0.0.
 * seg is TRUSTED: the entry point cannot read device memory without a synchronisation, so the
 * caller checks it (the Python layer does, on the host copy it uploads).  A seg that breaks the
 * contract gives unspecified values but no access outside the T rows.  No cap on T, no
 * scratch.  Null pointers, K < 1, T < 1, ld < T and nseg < 1 are refused before any device
 * work. */
fmx_status fmx_perf_periods(const double* R, int64_t K, int64_t T, int64_t ld, const int32_t* seg, int32_t nseg,
                            double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H_ */
