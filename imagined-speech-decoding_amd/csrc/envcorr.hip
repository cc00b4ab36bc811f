// Pairwise (orthogonalised) envelope correlation: the data-sized step of isd_amd.connectivity.envelope_correlation.
// Per trial, z [C][T] complex (the analytic signal), m = |z|, e = m (or log m^2), ec = e - mean e, se = |ec|_2:
//
//   o[l|j][t] = |Im(z_l conj(z_j))| / m_j = q / m_j,   q = |a_l b_j - b_l a_j|   (a = Re z, b = Im z; log: log o^2)
//   corr[l|j] = sum_t (o - mean o)(t) ec_j(t) / (se_j |o - mean o|_2),   out[l][j] = out[j][l] = (A[l|j] + A[j|l]) / 2
//
// with A = |corr| under `absolute`; `plain` is corr[l][j] = sum ec_l ec_j / (se_l se_j) instead.
//
//   envcorr_rows_kernel  one wave per (trial, channel) row, everything in fp64: the mean of e, then ec, its norm, and
//                        the sum of the rounded ec; it leaves W[row][t] = (1 / m, ec) rounded to S (1 / m = 0 where
//                        m = 0) beside z's (a, b), and stats[row] = (se, sum_t W.ec) in fp64.
//   envcorr_pair_kernel  one wave (one workgroup of 64) per (trial, pair of 16-channel tiles J <= I), enumerated as in
//                        csd_product_kernel.  T runs through LDS in chunks of kEnvChunk samples, the next chunk's
//                        loads in flight in registers: per (channel, sample) one record (a, b, 1 / m, ec), rows padded
//                        by one record so that 16 channels at one sample fall on 16 different 16-byte slots.  Lane
//                        (g, c) owns the four pairs (l = 16 I + 4 g + k, j = 16 J + c): q is symmetric in (l, j), so
//                        one q serves o[l|j] = q / m_j and o[j|l] = q / m_l.  The cross product is Kahan's
//                        compensated form (w = b_l a_j, err = fma(-b_l, a_j, w), q = fma(a_l, b_j, -w) + err): two
//                        channels nearly in phase cancel, and log amplifies the relative error of a small q.
//                        Every o is centred on its first sample before it is summed -- d = q / m - o(0) in one
//                        fma, or d = log (o / o(0))^2 -- which changes nothing in exact arithmetic, keeps sum d^2
//                        - (sum d)^2 / T free of cancellation and log o of microvolt data at the size of its spread,
//                        and leaves the o = 0 of real-valued z or a dead channel an exact zero (at T = 1 every ec is
//                        0 and so is the result).  sum d, sum d^2 and sum d ec accumulate in fp64 (24 accumulators
//                        a lane), in sample order, with no atomics: the result is bitwise repeatable.  The epilogue
//                        forms both correlations, symmetrises once and stores the same value twice; on a diagonal
//                        tile the lanes with l > j store, l = j stores the diagonal.
//
// No load goes outside z, W or stats (a chunk's tail and the channels past C are not loaded; their records are zeros
// and nothing of them is stored); no store outside W, stats or out.
#include <algorithm>
#include <cmath>
#include "common.h"

namespace isd {

constexpr int kEnvMaxChannels = 128;
constexpr int kEnvChunk = 16;                                   // samples per staged chunk
constexpr int kEnvRowWaves = 4;                                 // rows per workgroup of the prepass
enum { kEnvLog = 1, kEnvAbsolute = 2, kEnvPlain = 4 };

__device__ __forceinline__ double wave_sum(double v) {           // the same order in every lane and on every call
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

template <typename S, bool LOG>
__global__ __launch_bounds__(64 * kEnvRowWaves) void envcorr_rows_kernel(const S* __restrict__ z, S* __restrict__ W,
                                                                         double* __restrict__ stats, int64_t rows,
                                                                         int64_t T) {
  using V2 = S __attribute__((ext_vector_type(2)));
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kEnvRowWaves + (threadIdx.x >> 6);
  if (row >= rows) return;                                       // wave-uniform
  const V2* zr = reinterpret_cast<const V2*>(z) + row * T;
  V2* wr = reinterpret_cast<V2*>(W) + row * T;
  double sum = 0.0;
  for (int64_t t = lane; t < T; t += 64) {
    const V2 v = zr[t];
    const double a = (double)v[0], b = (double)v[1];
    const double m = sqrt(a * a + b * b);
    sum += LOG ? 2.0 * log(m) : m;
  }
  const double mean = wave_sum(sum) / (double)T;
  double ss = 0.0, sr = 0.0;
  for (int64_t t = lane; t < T; t += 64) {
    const V2 v = zr[t];
    const double a = (double)v[0], b = (double)v[1];
    const double m = sqrt(a * a + b * b);
    const double ec = (LOG ? 2.0 * log(m) : m) - mean;
    const S ecs = (S)ec;
    ss += ec * ec;
    sr += (double)ecs;
    const V2 w = {m > 0.0 ? (S)(1.0 / m) : (S)0, ecs};
    wr[t] = w;
  }
  ss = wave_sum(ss);
  sr = wave_sum(sr);
  if (lane == 0) {
    stats[2 * row] = sqrt(ss);
    stats[2 * row + 1] = sr;
  }
}

__device__ __forceinline__ float env_log(float x) { return logf(x); }
__device__ __forceinline__ double env_log(double x) { return log(x); }
__device__ __forceinline__ float env_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double env_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// q = |a_l b_j - b_l a_j|, compensated: w is a rounded product and err its exact rounding error
template <typename S>
__device__ __forceinline__ S env_cross(S al, S bl, S aj, S bj) {
  const S w = bl * aj;
  const S err = env_fma(-bl, aj, w);
  return fabs(env_fma(al, bj, -w) + err);
}

// MODE 0: o = q / m; 1: o = log (q / m)^2; 2: plain (no orthogonalisation)
template <typename S, int MODE>
__global__ __launch_bounds__(64) void envcorr_pair_kernel(const S* __restrict__ z, const S* __restrict__ W,
                                                          const double* __restrict__ stats, S* __restrict__ out,
                                                          int C, int64_t T, int absolute) {
  using V2 = S __attribute__((ext_vector_type(2)));
  using V4 = S __attribute__((ext_vector_type(4)));
  constexpr int KC = kEnvChunk, LD = KC + 1;                      // records per staged row, one of them padding
  constexpr int NF = 32 * KC / 64;                                // (channel, sample) records a lane stages per chunk
  __shared__ __attribute__((aligned(16))) V4 rec[32 * LD];
  const int lane = threadIdx.x, g = lane >> 4, c16 = lane & 15;
  const int nct = (C + 15) >> 4, ntp = nct * (nct + 1) / 2;
  int tp = (int)(blockIdx.x % ntp);
  const int64_t trial = blockIdx.x / ntp;
  int I = 0;
  while (tp > I) {                                               // tile pair tp -> (I, J), J <= I; at most 8 steps
    tp -= I + 1;
    ++I;
  }
  const int J = tp;
  const V2* zt = reinterpret_cast<const V2*>(z) + trial * C * T;
  const V2* wt = reinterpret_cast<const V2*>(W) + trial * C * T;

  // staging: record r of this lane is sample (lane & 15) of staged row 4 r + (lane >> 4); rows 0..15 are tile I
  const int ft = lane & (KC - 1);
  V2 pz[NF], pw[NF];
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int r = 0; r < NF; ++r) {
      const int srow = 4 * r + (lane >> 4);
      const int ch = 16 * (srow < 16 ? I : J) + (srow & 15);
      const bool in = ch < C && t0 + ft < T;
      const int64_t at = (int64_t)ch * T + t0 + ft;
      pz[r] = in ? zt[at] : V2{(S)0, (S)0};
      pw[r] = in ? wt[at] : V2{(S)0, (S)0};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int r = 0; r < NF; ++r) {
      const V4 v = {pz[r][0], pz[r][1], pw[r][0], pw[r][1]};
      rec[(4 * r + (lane >> 4)) * LD + ft] = v;
    }
  };

  double acc[4][2][3];
  S piv[4][2];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      acc[k][d][0] = acc[k][d][1] = acc[k][d][2] = 0.0;
      piv[k][d] = (S)0;
    }

  const V4* rl = rec + (4 * g) * LD;                             // this lane's four l rows (a broadcast per 16 lanes)
  const V4* rj = rec + (16 + c16) * LD;                          // its j row
  fetch(0);
  for (int64_t t0 = 0; t0 < T; t0 += KC) {
    wave_lds_sync();                                             // the last chunk's reads are done
    stage();
    wave_lds_sync();
    if (t0 + KC < T) fetch(t0 + KC);
    const int nt = (int)min((int64_t)KC, T - t0);
    if (MODE != 2 && t0 == 0) {                                  // the pivots: o at the first sample
      const V4 vj = rj[0];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const V4 vl = rl[k * LD];
        const S q = env_cross<S>(vl[0], vl[1], vj[0], vj[1]);
        const S o0 = q * vj[2], o1 = q * vl[2];
        piv[k][0] = MODE == 1 ? (S)1 / o0 : o0;
        piv[k][1] = MODE == 1 ? (S)1 / o1 : o1;
      }
    }
    for (int t = 0; t < nt; ++t) {
      const V4 vj = rj[t];
      const double ecj = (double)vj[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const V4 vl = rl[k * LD + t];
        if (MODE == 2) {
          acc[k][0][0] = fma((double)vl[3], ecj, acc[k][0][0]);
        } else {
          const S q = env_cross<S>(vl[0], vl[1], vj[0], vj[1]);
          S d0, d1;
          if (MODE == 1) {
            d0 = (S)2 * env_log(q * vj[2] * piv[k][0]);
            d1 = (S)2 * env_log(q * vl[2] * piv[k][1]);
          } else {
            d0 = env_fma(q, vj[2], -piv[k][0]);
            d1 = env_fma(q, vl[2], -piv[k][1]);
          }
          const double D0 = (double)d0, D1 = (double)d1;
          acc[k][0][0] += D0;
          acc[k][0][1] = fma(D0, D0, acc[k][0][1]);
          acc[k][0][2] = fma(D0, ecj, acc[k][0][2]);
          acc[k][1][0] += D1;
          acc[k][1][1] = fma(D1, D1, acc[k][1][1]);
          acc[k][1][2] = fma(D1, (double)vl[3], acc[k][1][2]);
        }
      }
    }
  }

  const int j = 16 * J + c16;
  if (j >= C) return;
  const double* st = stats + trial * C * 2;
  const double sej_raw = st[2 * j], sumj = st[2 * j + 1];
  const double sej = sej_raw == 0.0 ? 1.0 : sej_raw;
  const double invT = 1.0 / (double)T;
  S* ob = out + trial * C * C;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int l = 16 * I + 4 * g + k;
    if (l >= C || (I == J && l < j)) continue;                   // a diagonal tile: the pair belongs to the lane l > j
    if (l == j) {                                                // plain: 1, or 0 for a row of zero norm; NaN stays
      ob[(int64_t)l * C + l] = MODE == 2 ? (S)(sej_raw == 0.0 ? 0.0 : sej_raw / sej_raw) : (S)0;
      continue;
    }
    const double sel_raw = st[2 * l], suml = st[2 * l + 1];
    const double sel = sel_raw == 0.0 ? 1.0 : sel_raw;
    double v;
    if (MODE == 2) {
      v = acc[k][0][0] / (sel * sej);
    } else {
      double cr[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {                              // d = 0: o[l|j] against ec_j; 1: o[j|l] against ec_l
        const double s0 = acc[k][d][0];
        double var = acc[k][d][1] - s0 * s0 * invT;
        var = var < 0.0 ? 0.0 : var;                             // (a NaN stays a NaN)
        double so = sqrt(var);
        so = so == 0.0 ? 1.0 : so;
        const double num = acc[k][d][2] - s0 * invT * (d == 0 ? sumj : suml);
        cr[d] = num / ((d == 0 ? sej : sel) * so);
        if (absolute) cr[d] = fabs(cr[d]);
      }
      v = (cr[0] + cr[1]) * 0.5;
    }
    ob[(int64_t)l * C + j] = (S)v;
    ob[(int64_t)j * C + l] = (S)v;
  }
}

}  // namespace isd

using namespace isd;

namespace {

// The workspace in bytes: two fp64 statistics per row, then the prepass's W (two values per sample).
struct EnvWs { int64_t stats, W, slack, end; };
EnvWs env_layout(int64_t n, int64_t C, int64_t T, int64_t el) {
  EnvWs l;
  WorkCarver c;
  l.stats = c.take(n * C * 2 * 8, 256);
  l.W = c.take(n * C * T * 2 * el, 256);
  l.slack = c.take(256);                                          // never a zero-byte buffer
  l.end = c.end;
  return l;
}

template <typename S>
int envcorr_launch(const S* z, S* out, int64_t n, int64_t C, int64_t T, int flags, void* work, void* stream,
                   const char* who) {
  ISD_CHECK_ARG(n >= 0, "%s: n=%lld", who, (long long)n);
  ISD_CHECK_SUPPORTED(C >= 1 && C <= kEnvMaxChannels, "%s: C=%lld (need 1 <= C <= %d)", who, (long long)C,
                      kEnvMaxChannels);
  ISD_CHECK_ARG((flags & ~(kEnvLog | kEnvAbsolute | kEnvPlain)) == 0, "%s: flags=%d", who, flags);
  if (n == 0) return ISD_OK;
  ISD_CHECK_ARG(T >= 1, "%s: T=%lld (need T >= 1)", who, (long long)T);
  ISD_CHECK_ARG(z && out && work, "%s: null argument", who);
  const int nct = ((int)C + 15) / 16, ntp = nct * (nct + 1) / 2;
  ISD_CHECK_SUPPORTED(n * ntp <= 0x7fffffffLL && n * C <= 0x7fffffffLL * kEnvRowWaves,
                      "%s: n=%lld trials of %lld channels are more workgroups than one launch holds", who,
                      (long long)n, (long long)C);
  hipStream_t st = (hipStream_t)stream;
  const EnvWs l = env_layout(n, C, T, sizeof(S));
  double* stats = reinterpret_cast<double*>(static_cast<char*>(work) + l.stats);
  S* W = reinterpret_cast<S*>(static_cast<char*>(work) + l.W);
  const int64_t rows = n * C;
  const dim3 rgrid((unsigned)cdiv(rows, kEnvRowWaves)), rblock(64 * kEnvRowWaves);
  if (flags & kEnvLog)
    hipLaunchKernelGGL((envcorr_rows_kernel<S, true>), rgrid, rblock, 0, st, z, W, stats, rows, T);
  else
    hipLaunchKernelGGL((envcorr_rows_kernel<S, false>), rgrid, rblock, 0, st, z, W, stats, rows, T);
  ISD_LAUNCH_CHECK();
  const dim3 pgrid((unsigned)(n * ntp)), pblock(64);
  const int absolute = (flags & kEnvAbsolute) != 0;
  if (flags & kEnvPlain)
    hipLaunchKernelGGL((envcorr_pair_kernel<S, 2>), pgrid, pblock, 0, st, z, (const S*)W, (const double*)stats, out,
                       (int)C, T, absolute);
  else if (flags & kEnvLog)
    hipLaunchKernelGGL((envcorr_pair_kernel<S, 1>), pgrid, pblock, 0, st, z, (const S*)W, (const double*)stats, out,
                       (int)C, T, absolute);
  else
    hipLaunchKernelGGL((envcorr_pair_kernel<S, 0>), pgrid, pblock, 0, st, z, (const S*)W, (const double*)stats, out,
                       (int)C, T, absolute);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

}  // namespace

extern "C" int64_t isd_envcorr_work_bytes(int64_t n, int64_t C, int64_t T, int is_f64) {
  if (n < 0 || C < 1 || C > kEnvMaxChannels || T < 0) {
    set_error("isd_envcorr_work_bytes: n=%lld, C=%lld or T=%lld", (long long)n, (long long)C, (long long)T);
    return ISD_ERR_INVALID;
  }
  return env_layout(n, C, T, is_f64 ? 8 : 4).end;
}

extern "C" int isd_envcorr_f32(const float* z, float* out, int64_t n, int64_t C, int64_t T, int flags, void* work,
                               void* stream) {
  return envcorr_launch<float>(z, out, n, C, T, flags, work, stream, "isd_envcorr_f32");
}

extern "C" int isd_envcorr_f64(const double* z, double* out, int64_t n, int64_t C, int64_t T, int flags, void* work,
                               void* stream) {
  return envcorr_launch<double>(z, out, n, C, T, flags, work, stream, "isd_envcorr_f64");
}
