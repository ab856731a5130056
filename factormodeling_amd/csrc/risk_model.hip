// Predicted risk and attribution of M books under the factor risk model:
//
//   Sigma_d = B_d' F_d B_d + diag(s2_d)   over the symbols present on date d
//
// B [K][D][A] the exposures (a non-finite exposure and an absent symbol count as 0), Fc [D][K][K]
// the factor covariance (the lower triangle is read), S2 [D][A] the specific variances, W [M][D][A]
// the books (a NaN cell is not held and reads as 0).  Per (book m, date d):
//   expo_k = b_k = sum_a B_ka w_a,   (F b)_k,   contrib_k = b_k (F b)_k,
//   var = (factor + specific, factor = sum_k contrib_k, specific = sum_a w_a^2 s2_a),
//   marginal_a = sum_k B_ka (F b)_k + s2_a w_a   (optional; NaN on absent cells).
// A date with valid[d] == 0 is NaN in every output.
//
// One workgroup of 16 waves per (date, tile of up to 16 books).  The date's row is walked in
// chunks of 256 assets: the workgroup stages the tile's weights of the chunk in LDS (each read
// from memory once), then wave v multiplies the chunk of its two factor rows B[2v][d][:] and
// B[2v + 1][d][:] -- read once, coalesced -- against every book of the tile from LDS, the
// partial sums in registers.  So the exposures of a date are read once for the whole tile, and
// a weight once per tile instead of once per factor row (a first version without the staging
// re-read W K / 2 times through L2 and ran M = 32 at 6 % of the copy rate).  Every
// sum has one fixed order (a lane's assets ascending, the xor-shuffle tree, then k or j
// ascending), which does not depend on M, D or the tile: a book gives the same bits alone or
// in a batch, a date the same bits alone or inside a panel.  Plain fp64 with fma; no atomics.
#include "sim_mvo_common.hpp"   // smv_finite, smv_wsum

namespace fmx {
namespace {

constexpr int RB_NT = 1024;      // 16 waves: one per pair of factor rows at K = 32
constexpr int RB_MAX_K = 32;
constexpr int RB_TILE = 16;      // books per workgroup
constexpr int RB_CA = 256;       // assets per staged chunk

template <int MT>
__global__ __launch_bounds__(RB_NT) void k_risk_books(const double* __restrict__ B, const double* __restrict__ Fc,
                                                      const double* __restrict__ S2, const double* __restrict__ W,
                                                      const uint8_t* __restrict__ present,
                                                      const uint8_t* __restrict__ valid, int K, int64_t D, int A, int M,
                                                      double* __restrict__ var, double* __restrict__ expo,
                                                      double* __restrict__ contrib, double* __restrict__ marginal) {
  __shared__ double bl[RB_TILE][RB_MAX_K];    // b
  __shared__ double fb[RB_TILE][RB_MAX_K];    // F b
  __shared__ double sv[RB_TILE];              // specific variance
  __shared__ double ws[MT][RB_CA];            // the tile's weights of one chunk, cleaned
  const int64_t d = blockIdx.x;
  const int m0 = blockIdx.y * MT;
  const int mt = min(MT, M - m0);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t DA = D * (int64_t)A;
  const uint8_t* pd = present ? present + d * A : nullptr;
  const double* wd = W + d * A;               // book m at wd + m * DA
  const double* s2d = S2 + d * A;

  if (valid && !valid[d]) {
    for (int i = tid; i < mt * K; i += RB_NT) {
      const int64_t o = ((int64_t)(m0 + i / K) * D + d) * K + i % K;
      expo[o] = qnan();
      contrib[o] = qnan();
    }
    for (int i = tid; i < mt * 3; i += RB_NT) var[((int64_t)(m0 + i / 3) * D + d) * 3 + i % 3] = qnan();
    if (marginal)
      for (int m = 0; m < mt; ++m)
        for (int a = tid; a < A; a += RB_NT) marginal[(int64_t)(m0 + m) * DA + d * A + a] = qnan();
    return;
  }

  // ---- b = B w and the specific variance, chunk by chunk: wave v owns the factor rows 2v and
  // 2v + 1 (K <= 32 = 2 x 16 waves) and, for v < mt, the specific variance of book v
  const int k0 = 2 * wv;
  const bool rows = k0 < K, two = k0 + 1 < K;
  const double* r0 = B + (int64_t)(rows ? k0 : 0) * DA + d * A;
  const double* r1 = two ? r0 + DA : r0;
  double a0[MT], a1[MT], as = 0.0;
#pragma unroll
  for (int m = 0; m < MT; ++m) a0[m] = a1[m] = 0.0;
  for (int c0 = 0; c0 < A; c0 += RB_CA) {
    __syncthreads();                           // the previous chunk has been read
    for (int i = tid; i < mt * RB_CA; i += RB_NT) {
      const int m = i / RB_CA, c = i - m * RB_CA, a = c0 + c;
      double w = 0.0;
      if (a < A && (!pd || pd[a])) {
        w = wd[(int64_t)(m0 + m) * DA + a];
        w = w == w ? w : 0.0;
      }
      ws[m][c] = w;
    }
    __syncthreads();
    const int cn = min(RB_CA, A - c0);
    if (rows) {
      for (int c = lane; c < cn; c += 64) {
        double b0 = r0[c0 + c], b1 = r1[c0 + c];
        b0 = smv_finite(b0) ? b0 : 0.0;
        b1 = two && smv_finite(b1) ? b1 : 0.0;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (m < mt) {
            const double w = ws[m][c];         // 0 on absent cells
            a0[m] = __builtin_fma(b0, w, a0[m]);
            a1[m] = __builtin_fma(b1, w, a1[m]);
          }
        }
      }
    }
    if (wv < mt) {
      for (int c = lane; c < cn; c += 64) {
        const double w = ws[wv][c];
        if (w != 0.0) as = __builtin_fma(w * w, s2d[c0 + c], as);
      }
    }
  }
  if (rows) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m < mt) {
        const double s0 = smv_wsum(a0[m]), s1 = smv_wsum(a1[m]);
        if (lane == 0) {
          bl[m][k0] = s0;
          if (two) bl[m][k0 + 1] = s1;
        }
      }
    }
  }
  if (wv < mt) {
    as = smv_wsum(as);
    if (lane == 0) sv[wv] = as;
  }
  __syncthreads();

  // ---- F b (lower triangle of Fc), j ascending
  const double* Fd = Fc + d * (int64_t)K * K;
  for (int i = tid; i < mt * K; i += RB_NT) {
    const int m = i / K, k = i - m * K;
    double s = 0.0;
    for (int j = 0; j < K; ++j) s = __builtin_fma(j <= k ? Fd[k * K + j] : Fd[j * K + k], bl[m][j], s);
    fb[m][k] = s;
    const int64_t o = ((int64_t)(m0 + m) * D + d) * K + k;
    expo[o] = bl[m][k];
    contrib[o] = bl[m][k] * s;
  }
  __syncthreads();
  if (tid < mt) {
    double f = 0.0;
    for (int k = 0; k < K; ++k) f += bl[tid][k] * fb[tid][k];
    double* v = var + ((int64_t)(m0 + tid) * D + d) * 3;
    v[0] = f + sv[tid];
    v[1] = f;
    v[2] = sv[tid];
  }
  if (!marginal) return;

  // ---- marginal = B'(F b) + s2 w: a second pass over the exposures, k ascending
  for (int a = tid; a < A; a += RB_NT) {
    const bool pr = !pd || pd[a];
    double acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.0;
    if (pr) {
      for (int k = 0; k < K; ++k) {
        double b = B[(int64_t)k * DA + d * A + a];
        b = smv_finite(b) ? b : 0.0;
#pragma unroll
        for (int m = 0; m < MT; ++m)
          if (m < mt) acc[m] = __builtin_fma(b, fb[m][k], acc[m]);
      }
    }
    const double s2 = s2d[a];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m < mt) {
        const double w = wd[(int64_t)(m0 + m) * DA + a];
        const double own = (w == w && w != 0.0) ? s2 * w : 0.0;
        marginal[(int64_t)(m0 + m) * DA + d * A + a] = pr ? acc[m] + own : qnan();
      }
    }
  }
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" fmx_status fmx_risk_books(const double* B, const double* Fc, const double* S2, const double* W,
                                     const uint8_t* present, const uint8_t* valid, int64_t K, int64_t D, int64_t A,
                                     int64_t M, double* var, double* expo, double* contrib, double* marginal,
                                     void* stream) {
  FMX_ARG(K >= 1 && K <= RB_MAX_K, "risk_books: 1 <= K <= 32 factors");
  FMX_ARG(D >= 0 && D <= 0x7fffffff && M >= 0 && M <= 65535 * (int64_t)RB_TILE, "risk_books: bad dims");
  FMX_ARG(A >= 1 && A <= 0x7fffffff, "risk_books: bad A");
  if (D == 0 || M == 0) return FMX_OK;
  FMX_ARG(B && Fc && S2 && W && var && expo && contrib, "null pointer");
  hipStream_t s = as_stream(stream);
  const int Ki = (int)K, Ai = (int)A, Mi = (int)M;
  if (M == 1) {
    hipLaunchKernelGGL(k_risk_books<1>, dim3((unsigned)D, (unsigned)M), dim3(RB_NT), 0, s, B, Fc, S2, W, present, valid,
                       Ki, D, Ai, Mi, var, expo, contrib, marginal);
  } else if (M <= 4) {
    hipLaunchKernelGGL(k_risk_books<4>, dim3((unsigned)D, 1), dim3(RB_NT), 0, s, B, Fc, S2, W, present, valid, Ki, D, Ai,
                       Mi, var, expo, contrib, marginal);
  } else {
    hipLaunchKernelGGL(k_risk_books<RB_TILE>, dim3((unsigned)D, (unsigned)ceil_div(M, RB_TILE)), dim3(RB_NT), 0, s, B, Fc,
                       S2, W, present, valid, Ki, D, Ai, Mi, var, expo, contrib, marginal);
  }
  FMX_LAUNCH_CHECK("k_risk_books");
  return FMX_OK;
}
