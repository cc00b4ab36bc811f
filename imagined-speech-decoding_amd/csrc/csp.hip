// Common Spatial Patterns: the data-sized steps of the classical baseline's transformer,
//   Pipeline(CSP(8, log=True) -> StandardScaler -> SVC)      (notebooks/svm_baseline.ipynb:238-248, :307, :316)
// behind the band-pass of fir.hip.  The eigen-decomposition works on [K][C][C] and stays on the host (isd_amd/csp.py).
//
//   trial_cov   cov_i = X_i X_i^T / T, the second moment without mean removal.  One workgroup of four waves per
//               trial.  A chunk of KC time steps of all (zero-padded to a multiple of 16) channels is staged in LDS
//               with coalesced loads along T; every wave owns up to MAXQ of the UPPER 16x16 tiles and feeds them
//               v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 with both operands read from the same LDS image
//               (A = rows of tile row ti, B = rows of tile row tj).  Only elements on or above the diagonal are kept;
//               each is stored twice, at [a][b] and [b][a], so the matrix is symmetric bit for bit.
//   group_mean  out_k = mean over a class's trials of cov_i (optionally each divided by its trace), one thread per
//               output element walking the class's trials in the order of idx in fp64: no atomics.
//   csp_power   out[i][j] = mean_t (sum_c w[j][c] x[i][c][t])^2, optionally its log.  One workgroup per trial, a
//               lane owns VEC consecutive samples (16-byte loads where the rows are aligned), the filters sit in LDS
//               transposed and zero-padded to MB rows so that one broadcast read serves MB FMAs.  The projection is
//               never written; the sum over T is a shuffle tree plus a serial sum over the waves (fixed order).
#include "common.h"

namespace isd {

template <typename S> struct CovOps;
template <> struct CovOps<float> : Mfma16<float> {
  static constexpr int KC = 64;                                 // time steps staged per pass
};
template <> struct CovOps<double> : Mfma16<double> {
  static constexpr int KC = 32;
};

constexpr int kCovPad = 4;                                      // LDS row skew (elements)
constexpr int kCovWaves = 4;

template <typename S, int MAXQ>
__global__ __launch_bounds__(64 * kCovWaves) void trial_cov_kernel(const S* __restrict__ x, S* __restrict__ cov, int C,
                                                                   int T) {
  using O = CovOps<S>;
  constexpr int KC = O::KC, LD = KC + kCovPad;
  extern __shared__ __attribute__((aligned(16))) unsigned char cov_smem[];
  S* xs = reinterpret_cast<S*>(cov_smem);                        // [nt * 16][LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (C + 15) >> 4, Cp = nt * 16, U = nt * (nt + 1) / 2;
  const S* xi = x + (int64_t)blockIdx.x * C * T;

  int ti[MAXQ], tj[MAXQ];
  typename O::Acc acc[MAXQ];
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) {
    int u = q * kCovWaves + wave, a = 0;                         // u-th upper tile, row-major over (ti <= tj)
    while (a < nt && u >= nt - a) { u -= nt - a; ++a; }
    ti[q] = a;
    tj[q] = a + u;                                               // >= nt (or ti == nt) when the wave has no q-th tile
    acc[q] = (typename O::Acc)(0);
  }

  for (int t0 = 0; t0 < T; t0 += KC) {
    __syncthreads();                                             // the previous chunk has been consumed
    for (int e = tid; e < Cp * KC; e += 64 * kCovWaves) {
      const int c = e / KC, k = e % KC, t = t0 + k;
      xs[c * LD + k] = (c < C && t < T) ? xi[(int64_t)c * T + t] : (S)0;    // never past a row, never past C rows
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
      if (q * kCovWaves + wave < U) {                            // wave-uniform
        const S* pa = xs + (ti[q] * 16 + (lane & 15)) * LD + (lane >> 4);
        const S* pb = xs + (tj[q] * 16 + (lane & 15)) * LD + (lane >> 4);
#pragma unroll 4
        for (int k = 0; k < KC; k += 4) acc[q] = O::mma(pa[k], pb[k], acc[q]);
      }
    }
  }

  S* ci = cov + (int64_t)blockIdx.x * C * C;
  const S den = (S)T;
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) {
    if (q * kCovWaves + wave < U) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = ti[q] * 16 + O::lane_row(lane, r), b = tj[q] * 16 + (lane & 15);
        if (a <= b && b < C) {                                   // a <= b < C; the lower triangle is the mirror
          const S v = acc[q][r] / den;
          ci[a * C + b] = v;
          ci[b * C + a] = v;
        }
      }
    }
  }
}

template <typename S>
__global__ __launch_bounds__(256) void cov_group_mean_kernel(const S* __restrict__ cov, const int64_t* __restrict__ idx,
                                                             const int64_t* __restrict__ offs, int norm_trace,
                                                             double* __restrict__ out, int64_t n, int C) {
  const int k = blockIdx.y, CC = C * C;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= CC) return;
  const int64_t p0 = offs[k], p1 = offs[k + 1];
  double s = 0.0;
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t i = idx[p];
    if (i < 0 || i >= n) { s = __longlong_as_double(0x7ff8000000000000LL); continue; }   // no read outside cov
    const S* ci = cov + i * CC;
    double v = (double)ci[e];
    if (norm_trace) {
      double tr = 0.0;
      for (int c = 0; c < C; ++c) tr += (double)ci[c * C + c];   // wave-uniform addresses, index order
      v /= tr;
    }
    s += v;
  }
  out[(int64_t)k * CC + e] = p1 > p0 ? s / (double)(p1 - p0) : 0.0;
}

template <typename S, int VEC> struct PowVec;
template <> struct PowVec<float, 1> { using V = float; };
template <> struct PowVec<float, 4> { using V = float4; };
template <> struct PowVec<double, 1> { using V = double; };
template <> struct PowVec<double, 2> { using V = double2; };

template <typename S, int VEC>
__device__ __forceinline__ void pow_load(const S* p, S (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = *p;
  } else {
    const typename PowVec<S, VEC>::V w = *reinterpret_cast<const typename PowVec<S, VEC>::V*>(p);
    v[0] = w.x;
    v[1] = w.y;
    if constexpr (VEC == 4) { v[2] = w.z; v[3] = w.w; }
  }
}

template <typename S>
__device__ __forceinline__ S wave_sum_fixed(S v) {               // xor tree: the same association on every run
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// blockDim.x = 64 * n_waves (1..4); T % VEC == 0 and every row 16-byte aligned when VEC > 1
template <typename S, int VEC, int MB>
__global__ __launch_bounds__(256) void csp_power_kernel(const S* __restrict__ x, const S* __restrict__ w,
                                                        S* __restrict__ out, int C, int T, int m, int take_log) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pow_smem[];
  S* ws = reinterpret_cast<S*>(pow_smem);                        // [C][MB], ws[c][j] = w[j][c], 0 for j >= m
  S* part = ws + C * MB;                                         // [n_waves][MB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  for (int e = tid; e < C * MB; e += blockDim.x) {
    const int c = e / MB, j = e % MB;
    ws[e] = j < m ? w[j * C + c] : (S)0;
  }
  __syncthreads();
  const S* xi = x + (int64_t)blockIdx.x * C * T;
  S sq[MB];
#pragma unroll
  for (int j = 0; j < MB; ++j) sq[j] = (S)0;
  for (int t = tid * VEC; t < T; t += blockDim.x * VEC) {        // t + VEC <= T: T is a multiple of VEC
    S y[MB][VEC];
#pragma unroll
    for (int j = 0; j < MB; ++j)
#pragma unroll
      for (int v = 0; v < VEC; ++v) y[j][v] = (S)0;
    const S* xp = xi + t;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      S xv[VEC];
      pow_load<S, VEC>(xp + (int64_t)c * T, xv);
#pragma unroll
      for (int j = 0; j < MB; ++j) {
        const S wj = ws[c * MB + j];                             // the same address in every lane: a broadcast read
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[j][v] = fma(wj, xv[v], y[j][v]);
      }
    }
#pragma unroll
    for (int j = 0; j < MB; ++j)
#pragma unroll
      for (int v = 0; v < VEC; ++v) sq[j] = fma(y[j][v], y[j][v], sq[j]);
  }
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    const S s = wave_sum_fixed(sq[j]);
    if (lane == 0) part[wave * MB + j] = s;
  }
  __syncthreads();
  if (tid < m) {
    S s = (S)0;
    for (int q = 0; q < n_waves; ++q) s += part[q * MB + tid];
    s /= (S)T;
    out[(int64_t)blockIdx.x * m + tid] = take_log ? log(s) : s;
  }
}

}  // namespace isd

using namespace isd;

template <typename S>
static int trial_cov_launch(const S* x, S* cov, int64_t n, int C, int T, void* stream, const char* who) {
  ISD_CHECK_ARG(x && cov, "%s: null argument", who);
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL, "%s: n=%lld", who, (long long)n);
  ISD_CHECK_ARG(C >= 1 && C <= 128 && T >= 1, "%s: C=%d T=%d (need 1 <= C <= 128, T >= 1)", who, C, T);
  ISD_CHECK_ARG((const void*)x != (const void*)cov, "%s: x and cov are the same buffer", who);
  if (n == 0) return ISD_OK;
  const int nt = (C + 15) / 16;
  const size_t lds = (size_t)nt * 16 * (CovOps<S>::KC + kCovPad) * sizeof(S);      // <= 36.9 KB
  const dim3 grid((unsigned)n), block(64 * kCovWaves);
  hipStream_t st = (hipStream_t)stream;
  if (nt <= 2) hipLaunchKernelGGL((trial_cov_kernel<S, 1>), grid, block, lds, st, x, cov, C, T);         // <= 3 tiles
  else if (nt <= 4) hipLaunchKernelGGL((trial_cov_kernel<S, 3>), grid, block, lds, st, x, cov, C, T);    // <= 10
  else hipLaunchKernelGGL((trial_cov_kernel<S, 9>), grid, block, lds, st, x, cov, C, T);                 // <= 36
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

extern "C" int isd_trial_cov_f32(const float* x, float* cov, int64_t n, int C, int T, void* stream) {
  return trial_cov_launch<float>(x, cov, n, C, T, stream, "isd_trial_cov_f32");
}

extern "C" int isd_trial_cov_f64(const double* x, double* cov, int64_t n, int C, int T, void* stream) {
  return trial_cov_launch<double>(x, cov, n, C, T, stream, "isd_trial_cov_f64");
}

extern "C" int isd_cov_group_mean(const void* cov, int cov_f64, const int64_t* idx, const int64_t* offs, int norm_trace,
                                  double* out, int64_t n, int C, int K, void* stream) {
  ISD_CHECK_ARG(cov && idx && offs && out, "isd_cov_group_mean: null argument");
  ISD_CHECK_ARG(n >= 0 && C >= 1 && C <= 128 && K >= 1 && K <= 65535, "isd_cov_group_mean: n=%lld C=%d K=%d",
                (long long)n, C, K);
  const dim3 grid((unsigned)cdiv(C * C, 256), (unsigned)K);
  if (cov_f64)
    hipLaunchKernelGGL((cov_group_mean_kernel<double>), grid, dim3(256), 0, (hipStream_t)stream, (const double*)cov,
                       idx, offs, norm_trace, out, n, C);
  else
    hipLaunchKernelGGL((cov_group_mean_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)cov, idx,
                       offs, norm_trace, out, n, C);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

template <typename S, int VEC>
static int csp_power_launch_mb(const S* x, const S* w, S* out, int64_t n, int C, int T, int m, int take_log,
                               hipStream_t st) {
  const int mb = m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : m <= 8 ? 8 : 16;
  const int64_t per = cdiv(T, VEC);
  const int waves = per >= 256 ? 4 : (int)cdiv(per, 64);        // 1..4
  const size_t lds = (size_t)(C + 4) * mb * sizeof(S);          // <= 16.5 KB
  const dim3 grid((unsigned)n), block(64 * waves);
  switch (mb) {
#define ISD_POW_CASE(MB)                                                                                          \
  case MB:                                                                                                        \
    hipLaunchKernelGGL((csp_power_kernel<S, VEC, MB>), grid, block, lds, st, x, w, out, C, T, m, take_log);       \
    break;
    ISD_POW_CASE(1)
    ISD_POW_CASE(2)
    ISD_POW_CASE(4)
    ISD_POW_CASE(8)
    ISD_POW_CASE(16)
#undef ISD_POW_CASE
  }
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

template <typename S>
static int csp_power_launch(const S* x, const S* w, S* out, int64_t n, int C, int T, int m, int take_log, void* stream,
                            const char* who) {
  ISD_CHECK_ARG(x && w && out, "%s: null argument", who);
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL, "%s: n=%lld", who, (long long)n);
  ISD_CHECK_ARG(C >= 1 && C <= 128 && T >= 1 && m >= 1 && m <= 16,
                "%s: C=%d T=%d m=%d (need 1 <= C <= 128, T >= 1, 1 <= m <= 16)", who, C, T, m);
  if (n == 0) return ISD_OK;
  constexpr int VEC = 16 / sizeof(S);
  const bool wide = T % VEC == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;   // then every row starts on 16 bytes
  hipStream_t st = (hipStream_t)stream;
  return wide ? csp_power_launch_mb<S, VEC>(x, w, out, n, C, T, m, take_log, st)
              : csp_power_launch_mb<S, 1>(x, w, out, n, C, T, m, take_log, st);
}

extern "C" int isd_csp_power_f32(const float* x, const float* w, float* out, int64_t n, int C, int T, int m,
                                 int take_log, void* stream) {
  return csp_power_launch<float>(x, w, out, n, C, T, m, take_log, stream, "isd_csp_power_f32");
}

extern "C" int isd_csp_power_f64(const double* x, const double* w, double* out, int64_t n, int C, int T, int m,
                                 int take_log, void* stream) {
  return csp_power_launch<double>(x, w, out, n, C, T, m, take_log, stream, "isd_csp_power_f64");
}
