// The returns windows of N (manager, date) rows at once (portfolio_simulation.py:319-334, the
// rule simulation.mvo_window_rows states): row n's window is the last L returns dates
// r < nbefore[n] on which at least one of the row's present symbols has a returns row.
//
// Two kernels on one stream:
//
//   k_smw_pack   both presence masks ([N][A] and [Dr][A] uint8) to 64-bit words, one wave per
//                word: lane l reads byte 64 w + l (coalesced) and the wave's ballot is the word.
//                A <= 16,384 gives NW = ceil(A / 64) <= 256 words per row.
//   k_smw_walk   one wave per row.  Lane l keeps the row's words l, l + 64, l + 128, l + 192 in
//                registers (4 x 64 bits), walks r downwards from nbefore - 1, ANDs them against
//                the returns date's words (one coalesced read of NW * 8 bytes) and takes a
//                wave-wide any.  Four dates are loaded per step so their latencies overlap; they
//                are still judged in descending order.  The k-th hit is parked in lane k (L <= 64),
//                so the ascending list is written once at the end, the unused tail as zeros.
//                The loop counts r down to 0 and leaves at L hits: at most nbefore <= Dr steps.
//
// No LDS, no scratch; the walk kernel compiles to 26 VGPRs (the 4 feature words and the returns
// words of the 4 dates in flight), the pack kernel to 18.  This replaces the
// [N][A] x [A][Dr] presence product and the [N][Dr] cumsum of the single-manager search: a few
// hundred bytes read per candidate date.
#include <vector>

#include "fmx_common.hpp"

namespace fmx {

constexpr int SMW_MAX_A = 16384;
constexpr int SMW_MAX_L = 64;
constexpr int SMW_KW = SMW_MAX_A / 64 / 64;   // words per lane: 4

// bits [rows][NW]: bit (a & 63) of word a >> 6 is set when P[row][a] != 0; grid-stride over words
__global__ __launch_bounds__(256) void k_smw_pack(const uint8_t* __restrict__ P, int64_t rows, int A, int NW,
                                                  uint64_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int64_t nwords = rows * NW;
  const int64_t step = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nwords; w += step) {
    const int64_t row = w / NW;
    const int a = (int)(w - row * NW) * 64 + lane;
    const bool on = a < A && P[row * A + a] != 0;
    const uint64_t word = __ballot(on);
    if (lane == 0) bits[w] = word;
  }
}

__global__ __launch_bounds__(256) void k_smw_walk(const uint64_t* __restrict__ fbits, const uint64_t* __restrict__ rbits,
                                                  const int32_t* __restrict__ nbefore, int64_t N, int NW, int L,
                                                  int32_t* __restrict__ win_rows, int32_t* __restrict__ win_T) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n >= N) return;   // the whole wave leaves together
  uint64_t fw[SMW_KW];
#pragma unroll
  for (int k = 0; k < SMW_KW; ++k) {
    const int w = lane + 64 * k;
    fw[k] = w < NW ? fbits[n * NW + w] : 0;
  }
  int cnt = 0, mine = 0;
  int r = nbefore[n] - 1;
  while (r >= 0 && cnt < L) {
    bool hit[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rq = r - q;
      uint64_t any = 0;
      if (rq >= 0) {
        const uint64_t* rb = rbits + (int64_t)rq * NW;
#pragma unroll
        for (int k = 0; k < SMW_KW; ++k) {
          const int w = lane + 64 * k;
          if (w < NW) any |= fw[k] & rb[w];
        }
      }
      hit[q] = any != 0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool h = __ballot(hit[q]) != 0;   // wave-uniform
      if (h && cnt < L) {
        if (lane == cnt) mine = r - q;
        ++cnt;
      }
    }
    r -= 4;
  }
  // lane k holds the k-th hit counted from the latest date: ascending order reverses it
  const int src = cnt - 1 - lane;
  const int v = __shfl(mine, src >= 0 ? src : 0);
  if (lane < L) win_rows[n * L + lane] = lane < cnt ? v : 0;
  if (lane == 0) win_T[n] = cnt;
}

}  // namespace fmx

using namespace fmx;

// workspace: both masks as 64-bit words, (N + Dr) * ceil(A / 64) of them
extern "C" int64_t fmx_sim_mvo_window_rows_work_bytes(int64_t N, int64_t A, int64_t Dr) {
  if (N < 0 || A < 0 || Dr < 0) return 0;
  return (int64_t)sizeof(uint64_t) * (N + Dr) * ceil_div(A, 64);
}

extern "C" fmx_status fmx_sim_mvo_window_rows(const uint8_t* fpresent, const uint8_t* rpresent, const int32_t* nbefore,
                                              int64_t N, int64_t A, int64_t Dr, int64_t Lmax, int32_t* win_rows,
                                              int32_t* win_T, void* work, int64_t work_bytes, void* stream) {
  FMX_ARG(N >= 0 && N <= 0x7fffffff && Dr >= 0 && Dr <= 0x7fffffff, "sim_mvo_window_rows: bad dims");
  FMX_ARG(A >= 1 && A <= SMW_MAX_A, "sim_mvo_window_rows: 1 <= A <= 16384");
  FMX_ARG(Lmax >= 1 && Lmax <= SMW_MAX_L, "sim_mvo_window_rows: 1 <= Lmax <= 64 window rows");
  if (N == 0) return FMX_OK;
  FMX_ARG(fpresent && nbefore && win_rows && win_T, "null pointer");
  FMX_ARG(Dr == 0 || rpresent, "null pointer");
  hipStream_t s = as_stream(stream);
  // nbefore bounds the walk: it is read back and checked before anything is launched
  {
    std::vector<int32_t> hb((size_t)N);
    FMX_HIP(hipMemcpyAsync(hb.data(), nbefore, sizeof(int32_t) * hb.size(), hipMemcpyDeviceToHost, s));
    FMX_HIP(hipStreamSynchronize(s));
    for (int64_t n = 0; n < N; ++n)
      FMX_ARG(hb[n] >= 0 && hb[n] <= Dr, "sim_mvo_window_rows: nbefore outside [0, Dr]");
  }
  FMX_ARG(work && work_bytes >= fmx_sim_mvo_window_rows_work_bytes(N, A, Dr),
          "sim_mvo_window_rows: workspace too small");
  const int NW = (int)ceil_div(A, 64);
  uint64_t* fbits = (uint64_t*)work;
  uint64_t* rbits = fbits + N * NW;
  const int Ai = (int)A, Li = (int)Lmax;
  const int64_t cap = 1 << 20;   // blocks of 4 waves; the pack kernel strides over the rest
  {
    const unsigned g = (unsigned)std::min<int64_t>(ceil_div(N * NW, 4), cap);
    hipLaunchKernelGGL(k_smw_pack, dim3(g), dim3(256), 0, s, fpresent, N, Ai, NW, fbits);
    FMX_LAUNCH_CHECK("k_smw_pack");
  }
  if (Dr > 0) {
    const unsigned g = (unsigned)std::min<int64_t>(ceil_div(Dr * NW, 4), cap);
    hipLaunchKernelGGL(k_smw_pack, dim3(g), dim3(256), 0, s, rpresent, Dr, Ai, NW, rbits);
    FMX_LAUNCH_CHECK("k_smw_pack");
  }
  hipLaunchKernelGGL(k_smw_walk, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, s, (const uint64_t*)fbits,
                     (const uint64_t*)rbits, nbefore, N, NW, Li, win_rows, win_T);
  FMX_LAUNCH_CHECK("k_smw_walk");
  return FMX_OK;
}
