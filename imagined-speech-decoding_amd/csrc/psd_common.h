// What csrc/psd.hip (Welch PSD) and csrc/csd.hip (cross-spectral density) share: the plan, the operand maps of the two
// 16x16x4 MFMAs, the staging of a [64][KC] tile through registers into LDS, one staged chunk into the accumulators,
// and the fp64 segment-mean pre-pass.  See psd.hip for the tiling these serve.
#pragma once
#include <algorithm>
#include "common.h"

struct isd_psd_plan {
  int n_fft, n_per_seg, n_overlap, step, k_lo, k_hi, K, Kp, remove_dc;
  int np32, np64;            // n_per_seg rounded up to whole chunks of the float / double kernel
  float *d_tab32, *d_scale32;   // [2][Kp][np32]: cos rows then sin rows; scale [K]
  double *d_tab64, *d_scale64;
};

namespace isd {

template <typename S> struct PsdOps;                            // chunk length and LDS row stride (elements)
template <> struct PsdOps<float> : Mfma16<float> {
  static constexpr int KC = 64, LD = KC + 4;
};
template <> struct PsdOps<double> : Mfma16<double> {
  static constexpr int KC = 32, LD = KC + 4;
};

constexpr int kPsdThreads = 256;
constexpr int kPsdRows = 64;                                    // data rows of a workgroup
constexpr int kPsdBins = 64;                                    // bins of a workgroup: 16 per wave
constexpr int kPsdMaxFft = 2048;
constexpr int kPsdSplitBelow = 256;                             // fewer (row, bin) tiles than CUs: split the segments
constexpr int kPsdSplitTarget = 512;                            // ... into about two workgroups per CU

// A [64][KC] tile on its way to LDS: a thread owns column tid % KC of rows tid / KC + (256 / KC) j, so a wave's loads
// are consecutive elements.  Zero where the row is >= nrow or the column >= ncol: nothing else is read.
template <typename S, int PF>
__device__ __forceinline__ void psd_fetch_tile(S (&pre)[PF], const S* __restrict__ p0, int64_t ld, int nrow, int ncol,
                                               int tid) {
  constexpr int KC = PsdOps<S>::KC, RPP = kPsdThreads / KC;
  const int r0 = tid / KC, t = tid % KC;
  const S* p = p0 + (int64_t)r0 * ld + t;
#pragma unroll
  for (int j = 0; j < PF; ++j) pre[j] = (r0 + j * RPP < nrow && t < ncol) ? p[(int64_t)j * RPP * ld] : (S)0;
}

template <typename S, int PF>
__device__ __forceinline__ void psd_store_tile(S* dst, const S (&pre)[PF], int tid) {
  constexpr int KC = PsdOps<S>::KC, RPP = kPsdThreads / KC, LD = PsdOps<S>::LD;
  const int r0 = tid / KC, t = tid % KC;
#pragma unroll
  for (int j = 0; j < PF; ++j) dst[(r0 + j * RPP) * LD + t] = pre[j];
}

// the data tile: the segment mean comes off in fp64; padding stays zero
template <typename S, int PF>
__device__ __forceinline__ void psd_store_data(S* dst, const S (&pre)[PF], const double* mus, int nrow, int ncol,
                                               int tid) {
  constexpr int KC = PsdOps<S>::KC, RPP = kPsdThreads / KC, LD = PsdOps<S>::LD;
  const int r0 = tid / KC, t = tid % KC;
#pragma unroll
  for (int j = 0; j < PF; ++j)
    dst[(r0 + j * RPP) * LD + t] = (r0 + j * RPP < nrow && t < ncol) ? (S)((double)pre[j] - mus[r0 + j * RPP]) : (S)0;
}

// One staged chunk into the accumulators of NB 16-bin tiles as straight-line code: all LDS reads of a k block first,
// then 2 NB independent MFMAs between two uses of one accumulator.  (float; 256 registers with no spill.)
template <typename S, int NB>
__device__ __forceinline__ void psd_mma_chunk(typename PsdOps<S>::Acc (&re)[kPsdBins / 16],
                                              typename PsdOps<S>::Acc (&im)[kPsdBins / 16], const S* pa, const S* pbc,
                                              const S* pbs) {
  using O = PsdOps<S>;
  using Vec = typename O::Vec;
  constexpr int KC = O::KC, LD = O::LD, VEC = O::VEC;
#pragma unroll
  for (int k = 0; k < KC; k += 4 * VEC) {
    const Vec va = *reinterpret_cast<const Vec*>(pa + k);
    Vec vc[NB], vs[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      vc[b] = *reinterpret_cast<const Vec*>(pbc + b * 16 * LD + k);
      vs[b] = *reinterpret_cast<const Vec*>(pbs + b * 16 * LD + k);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        re[b] = O::mma(va[v], vc[b][v], re[b]);
        im[b] = O::mma(va[v], vs[b][v], im[b]);
      }
    }
  }
}

// means [rows][S] (fp64): one wave per (row, segment), lanes stride the segment, then a fixed butterfly
template <typename S>
__global__ __launch_bounds__(kPsdThreads) void psd_mean_kernel(const S* __restrict__ x, double* __restrict__ means,
                                                              int64_t units, int64_t S_, int64_t T, int nps,
                                                              int step) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < units; u += (int64_t)gridDim.x * 4) {
    const int64_t row = u / S_, s = u % S_;
    const S* p = x + row * T + s * step;
    double a = 0.0;
    for (int t = lane; t < nps; t += 64) a += (double)p[t];     // never past the segment
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
    if (lane == 0) means[u] = a / (double)nps;
  }
}

}  // namespace isd

// ------------------------------------------------------------------ host side
namespace isd {

static inline int64_t psd_segments(const isd_psd_plan* p, int64_t T) {
  return T < p->n_per_seg ? 0 : (T - p->n_per_seg) / p->step + 1;
}

}  // namespace isd
