// Independent component analysis (parallel FastICA, logcosh contrast): the data-sized steps of isd_amd.ICA, the
// artifact-removal stage between the band-pass of fir.hip and CSP / the deep models
//   ICA(n_components, method='fastica').fit(epochs); ica.apply(epochs, exclude=[...])   (scripts/artifact_analysis.py:61)
// The whitening and the symmetric decorrelation work on [m][C] matrices and stay on the host (isd_amd/ica.py).
//
//   ica_step       one pass over x per FastICA iteration:  G = tanh(U x - b),  P = sum G x^T,  s = sum G,
//                  q = sum (1 - G^2).  A workgroup of four waves walks (trial, chunk of KC time steps) units, dealt
//                  round-robin.  Per unit it stages all (zero-padded to a multiple of 16) channels of the chunk in LDS
//                  as trial_cov_kernel does, forms the [mp][KC] projection on the matrix cores (A = rows of U in LDS,
//                  B = the chunk), applies tanh in the accumulator registers, adds s and q there, puts G in LDS and
//                  accumulates P += G chunk^T on the matrix cores with both operands read from LDS.  Neither the
//                  projection nor G reaches memory.  Each workgroup leaves its partial P, s, q in a workspace;
//   ica_reduce     adds the workgroups' partials in fp64 in workgroup order, one thread per element: no atomics, the
//                  same bits on every run.
//   spatial_apply  out_i = M x_i + bias on the same tiles: blockIdx.y owns 64 rows of M (staged in LDS once), the
//                  workgroup walks the same units and stores the accumulators straight to out.
// Padding is always zeros in LDS: no load goes past a row of x, past its C rows, or past the rows of U / M.
//
// Operand order.  A 16x16x4 MFMA takes A[row][k] and B[k][col] from lane (row or col) + 16 k.  A sum over k does not
// care which k a lane group takes, as long as A and B agree, so inside a block of 4 VEC steps (VEC = 4 floats or 2
// doubles = 16 bytes) lane group g takes k = VEC g + s in MFMA s: an operand whose k runs along an LDS row is then ONE
// 16-byte read per VEC MFMAs instead of one read per MFMA.  The row strides below keep those reads off each other's
// banks (16-byte reads go in groups of 16 lanes over 64 banks; 4- and 8-byte reads in groups of 32).
// The next unit's chunk is fetched into registers while the current one is computed.
#include <algorithm>
#include "common.h"

namespace isd {

template <typename S> struct IcaOps;
template <> struct IcaOps<float> : Mfma16<float> {
  static constexpr int KC = 64;                                 // time steps staged per unit
  static constexpr int LDX = KC + 4, LDG = KC + 8, PADM = 8;    // row strides (elements): chunk, G, U / M (Cp + PADM)
};
template <> struct IcaOps<double> : Mfma16<double> {
  static constexpr int KC = 32;
  static constexpr int LDX = KC + 4, LDG = KC + 4, PADM = 4;
};

constexpr int kIcaWaves = 4;
constexpr int kIcaThreads = 64 * kIcaWaves;
constexpr int kIcaRows = 64;                                    // rows of U / M one workgroup holds
constexpr int kIcaCUs = 256;                                    // compute units of an MI355X
constexpr int kIcaMaxOcc = 3;                                   // workgroups per CU the grids are sized for
constexpr int kIcaLdsPerCU = 160 * 1024;

// ms[r][c] = M[row0 + r][c] for the rp rows from row0, zero where row0 + r >= rows or c >= C
template <typename S>
__device__ __forceinline__ void ica_stage_matrix(S* ms, const S* __restrict__ M, int rows, int row0, int rp, int C,
                                                 int Cp, int ldm, int tid) {
  for (int e = tid; e < rp * Cp; e += kIcaThreads) {
    const int r = e / Cp, c = e % Cp;
    ms[r * ldm + c] = (row0 + r < rows && c < C) ? M[(int64_t)(row0 + r) * C + c] : (S)0;
  }
}

// The chunk of unit (trial i, time steps t0 .. t0 + KC) on its way to LDS: a thread owns step tid % KC of channels
// tid / KC + (256 / KC) j, so its loads sit one fixed stride apart; zero where the channel is >= C or the step >= T.
// PF = (largest Cp) * KC / 256 registers per thread.
template <typename S, int PF>
__device__ __forceinline__ void ica_fetch_chunk(S (&pre)[PF], const S* __restrict__ xi, int C, int T, int t0, int tid) {
  constexpr int KC = IcaOps<S>::KC, RPP = kIcaThreads / KC;     // channels per pass of the 256 threads
  const int c0 = tid / KC, t = t0 + tid % KC;
  const S* p = xi + (int64_t)c0 * T + t;
  const int64_t stride = (int64_t)RPP * T;
#pragma unroll
  for (int j = 0; j < PF; ++j)
    pre[j] = (c0 + j * RPP < C && t < T) ? p[j * stride] : (S)0;                   // never past a row or past C rows
}

template <typename S, int PF>
__device__ __forceinline__ void ica_store_chunk(S* xs, const S (&pre)[PF], int Cp, int tid) {
  constexpr int KC = IcaOps<S>::KC, LD = IcaOps<S>::LDX;
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int e = tid + j * kIcaThreads;
    if (j * kIcaThreads < Cp * KC) xs[(e / KC) * LD + e % KC] = pre[j];          // Cp * KC is a multiple of 256
  }
}

// the 16 x 16 tile (rows mi*16.. of ms) x (time steps tj*16.. of the chunk), summed over the Cp staged channels
template <typename S>
__device__ __forceinline__ typename IcaOps<S>::Acc ica_project(const S* ms, const S* xs, int mi, int tj, int Cp,
                                                               int ldm, int lane) {
  using O = IcaOps<S>;
  constexpr int LD = O::LDX, VEC = O::VEC;
  const S* pa = ms + (mi * 16 + (lane & 15)) * ldm + VEC * (lane >> 4);      // A[row][k]: VEC channels of one row
  const S* pb = xs + VEC * (lane >> 4) * LD + tj * 16 + (lane & 15);         // B[k][col]: the same channels, one step
  typename O::Acc y = (typename O::Acc)(0);
  for (int c0 = 0; c0 < Cp; c0 += 16) {                         // Cp is a multiple of 16
#pragma unroll
    for (int c = c0; c < c0 + 16; c += 4 * VEC) {
      const typename O::Vec va = *reinterpret_cast<const typename O::Vec*>(pa + c);
#pragma unroll
      for (int s = 0; s < VEC; ++s) y = O::mma(va[s], pb[(c + s) * LD], y);
    }
  }
  return y;
}

template <typename S>
__device__ __forceinline__ S ica_row_sum16(S v) {                // over the 16 lanes that share lane >> 4, fixed order
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// work [gridDim.x][m * C + 2 * m]: per workgroup P (row-major [m][C]), then s [m], then q [m].  CPMAX: 64 or 128,
// the largest padded channel count this instance stages; MAXB: P tiles per wave.
template <typename S, int MAXB, int CPMAX>
__global__ __launch_bounds__(kIcaThreads) void ica_step_kernel(const S* __restrict__ x, const S* __restrict__ U,
                                                              const S* __restrict__ b, S* __restrict__ work,
                                                              int64_t units, int nchunk, int C, int T, int m) {
  using O = IcaOps<S>;
  using Acc = typename O::Acc;
  using Vec = typename O::Vec;
  constexpr int KC = O::KC, LD = O::LDX, LDG = O::LDG, VEC = O::VEC, TT = KC / 16;
  constexpr int MAXA = kIcaRows / 16 * TT / kIcaWaves, PF = CPMAX * KC / kIcaThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char ica_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (C + 15) >> 4, Cp = nt * 16, mt = (m + 15) >> 4, mp = mt * 16, ldu = Cp + O::PADM;
  const int nA = mt * TT, nB = mt * nt;                          // tiles of the projection, tiles of P
  S* xs = reinterpret_cast<S*>(ica_smem);                        // [Cp][LD]  the chunk
  S* gs = xs + Cp * LD;                                          // [mp][LDG] G of the chunk
  S* us = gs + mp * LDG;                                         // [mp][ldu] U, zero padded
  ica_stage_matrix<S>(us, U, m, 0, mp, C, Cp, ldu, tid);         // visible after the first barrier pair below

  S bq[MAXA][4];
  Acc sacc[MAXA], qacc[MAXA], pacc[MAXB];
#pragma unroll
  for (int a = 0; a < MAXA; ++a) {
    const int u = a * kIcaWaves + wave, mi = u / TT;             // tile u of the projection: rows mi, time tile u % TT
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = mi * 16 + O::lane_row(lane, r);
      bq[a][r] = (u < nA && row < m) ? b[row] : (S)0;
    }
    sacc[a] = (Acc)(0);
    qacc[a] = (Acc)(0);
  }
#pragma unroll
  for (int q = 0; q < MAXB; ++q) pacc[q] = (Acc)(0);

  S pre[PF];
  int64_t unit = blockIdx.x;                                     // gridDim.x <= units: every workgroup has a unit
  ica_fetch_chunk<S, PF>(pre, x + unit / nchunk * C * T, C, T, (int)(unit % nchunk) * KC, tid);
  for (; unit < units; unit += gridDim.x) {
    const int t0 = (int)(unit % nchunk) * KC;
    __syncthreads();                                             // the previous chunk and its G have been consumed
    ica_store_chunk<S, PF>(xs, pre, Cp, tid);
    const int64_t next = unit + gridDim.x;
    if (next < units)                                            // workgroup-uniform; in flight during the MFMAs
      ica_fetch_chunk<S, PF>(pre, x + next / nchunk * C * T, C, T, (int)(next % nchunk) * KC, tid);
    __syncthreads();
#pragma unroll
    for (int a = 0; a < MAXA; ++a) {
      const int u = a * kIcaWaves + wave;
      if (u < nA) {                                              // wave-uniform
        const int mi = u / TT, tj = u % TT;
        const Acc y = ica_project<S>(us, xs, mi, tj, Cp, ldu, lane);
        const bool live = t0 + tj * 16 + (lane & 15) < T;        // a padded time step adds nothing
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mi * 16 + O::lane_row(lane, r);
          const S t = tanh(y[r] - bq[a][r]);                     // saturates to +-1: 1 - t*t is then 0, never NaN
          const S g = (live && row < m) ? t : (S)0;
          sacc[a][r] += g;
          qacc[a][r] += live ? (S)1 - g * g : (S)0;
          gs[row * LDG + tj * 16 + (lane & 15)] = g;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXB; ++q) {
      const int u = q * kIcaWaves + wave;
      if (u < nB) {                                              // wave-uniform
        const int mi = u / nt, cj = u % nt;
        const S* pa = gs + (mi * 16 + (lane & 15)) * LDG + VEC * (lane >> 4);    // A[row][k]: VEC steps of G's row
        const S* pb = xs + (cj * 16 + (lane & 15)) * LD + VEC * (lane >> 4);     // B[k][col]: of the channel's row
#pragma unroll
        for (int k = 0; k < KC; k += 4 * VEC) {
          const Vec va = *reinterpret_cast<const Vec*>(pa + k), vb = *reinterpret_cast<const Vec*>(pb + k);
#pragma unroll
          for (int s = 0; s < VEC; ++s) pacc[q] = O::mma(va[s], vb[s], pacc[q]);
        }
      }
    }
  }

  S* wp = work + (int64_t)blockIdx.x * ((int64_t)m * C + 2 * m);
#pragma unroll
  for (int q = 0; q < MAXB; ++q) {
    const int u = q * kIcaWaves + wave;
    if (u < nB) {
      const int mi = u / nt, cj = u % nt;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mi * 16 + O::lane_row(lane, r), col = cj * 16 + (lane & 15);
        if (row < m && col < C) wp[row * C + col] = pacc[q][r];
      }
    }
  }
  __syncthreads();                                               // gs is free: [nA][16] row sums of s, then of q
  S* red = gs;
#pragma unroll
  for (int a = 0; a < MAXA; ++a) {
    const int u = a * kIcaWaves + wave;
    if (u < nA) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const S sv = ica_row_sum16(sacc[a][r]), qv = ica_row_sum16(qacc[a][r]);
        if ((lane & 15) == 0) {
          red[u * 16 + O::lane_row(lane, r)] = sv;
          red[(nA + u) * 16 + O::lane_row(lane, r)] = qv;
        }
      }
    }
  }
  __syncthreads();
  if (tid < m) {
    const int mi = tid >> 4;
    S sv = (S)0, qv = (S)0;
    for (int tj = 0; tj < TT; ++tj) {                            // time tiles in order
      sv += red[(mi * TT + tj) * 16 + (tid & 15)];
      qv += red[(nA + mi * TT + tj) * 16 + (tid & 15)];
    }
    wp[m * C + tid] = sv;
    wp[m * C + m + tid] = qv;
  }
}

template <typename S>
__global__ __launch_bounds__(256) void ica_reduce_kernel(const S* __restrict__ work, int G, int m, int C,
                                                         double* __restrict__ P, double* __restrict__ s,
                                                         double* __restrict__ q) {
  const int mC = m * C, E = mC + 2 * m;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double a = 0.0;
#pragma unroll 8
  for (int g = 0; g < G; ++g) a += (double)work[(int64_t)g * E + e];        // workgroup order
  if (e < mC) P[e] = a;
  else if (e < mC + m) s[e - mC] = a;
  else q[e - mC - m] = a;
}

template <typename S, int CPMAX>
__global__ __launch_bounds__(kIcaThreads) void spatial_apply_kernel(const S* __restrict__ x, const S* __restrict__ M,
                                                                   const S* __restrict__ bias, S* __restrict__ out,
                                                                   int64_t units, int nchunk, int C, int T, int R) {
  using O = IcaOps<S>;
  using Acc = typename O::Acc;
  constexpr int KC = O::KC, LD = O::LDX, TT = KC / 16;
  constexpr int MAXA = kIcaRows / 16 * TT / kIcaWaves, PF = CPMAX * KC / kIcaThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char ica_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (C + 15) >> 4, Cp = nt * 16, ldm = Cp + O::PADM;
  const int row0 = blockIdx.y * kIcaRows, rt = (min(kIcaRows, R - row0) + 15) >> 4, nA = rt * TT;
  S* xs = reinterpret_cast<S*>(ica_smem);                        // [Cp][LD]
  S* ms = xs + Cp * LD;                                          // [rt * 16][ldm] rows row0.. of M, zero padded
  ica_stage_matrix<S>(ms, M, R, row0, rt * 16, C, Cp, ldm, tid);

  S bq[MAXA][4];
#pragma unroll
  for (int a = 0; a < MAXA; ++a) {
    const int u = a * kIcaWaves + wave;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + (u / TT) * 16 + O::lane_row(lane, r);
      bq[a][r] = (bias != nullptr && u < nA && row < R) ? bias[row] : (S)0;
    }
  }

  S pre[PF];
  int64_t unit = blockIdx.x;                                     // gridDim.x <= units
  ica_fetch_chunk<S, PF>(pre, x + unit / nchunk * C * T, C, T, (int)(unit % nchunk) * KC, tid);
  for (; unit < units; unit += gridDim.x) {
    const int64_t i = unit / nchunk;
    const int t0 = (int)(unit % nchunk) * KC;
    __syncthreads();                                             // the previous chunk has been consumed
    ica_store_chunk<S, PF>(xs, pre, Cp, tid);
    const int64_t next = unit + gridDim.x;
    if (next < units)                                            // workgroup-uniform; in flight during the MFMAs
      ica_fetch_chunk<S, PF>(pre, x + next / nchunk * C * T, C, T, (int)(next % nchunk) * KC, tid);
    __syncthreads();
    S* oi = out + i * R * T;
#pragma unroll
    for (int a = 0; a < MAXA; ++a) {
      const int u = a * kIcaWaves + wave;
      if (u < nA) {                                              // wave-uniform
        const int mi = u / TT, tj = u % TT, t = t0 + tj * 16 + (lane & 15);
        const Acc y = ica_project<S>(ms, xs, mi, tj, Cp, ldm, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + mi * 16 + O::lane_row(lane, r);
          if (row < R && t < T) oi[(int64_t)row * T + t] = y[r] + bq[a][r];  // never past a row, never past R rows
        }
      }
    }
  }
}

}  // namespace isd

using namespace isd;

namespace {

// LDS of one workgroup: the chunk, `rows` rows of U / M and, for the step, the G tile
template <typename S>
size_t ica_lds_bytes(int C, int rows, bool with_g) {
  using O = IcaOps<S>;
  const int Cp = (C + 15) / 16 * 16, rp = (rows + 15) / 16 * 16;
  return ((size_t)Cp * O::LDX + (size_t)rp * (Cp + O::PADM) + (with_g ? (size_t)rp * O::LDG : 0)) * sizeof(S);
}

// Workgroups of a launch: as many as are resident at once (up to kIcaMaxOcc per CU, fewer where LDS allows fewer),
// never more than there are units.  A function of the shape alone, so the order of every sum is too.
int ica_grid(int64_t units, size_t lds) {
  const int occ = std::max(1, std::min<int>(kIcaMaxOcc, (int)(kIcaLdsPerCU / (lds + 1024))));
  return (int)std::min<int64_t>(units, (int64_t)kIcaCUs * occ);
}

bool ica_step_shape_ok(int64_t n, int C, int T, int m) {
  return n >= 0 && n <= 2147483647LL && C >= 1 && C <= 128 && T >= 1 && m >= 1 && m <= kIcaRows;
}

template <typename S>
int ica_step_grid(int64_t n, int C, int T, int m) {
  return ica_grid(n * cdiv(T, IcaOps<S>::KC), ica_lds_bytes<S>(C, m, true));
}

template <typename S, int MAXB>
int ica_step_launch_cp(int grid, size_t lds, hipStream_t st, const S* x, const S* U, const S* b, S* work,
                       int64_t units, int nchunk, int C, int T, int m) {
  const dim3 g((unsigned)grid), blk(kIcaThreads);
  return C <= 64 ? launch_lds(ica_step_kernel<S, MAXB, 64>, g, blk, lds, st, x, U, b, work, units, nchunk, C, T, m)
                 : launch_lds(ica_step_kernel<S, MAXB, 128>, g, blk, lds, st, x, U, b, work, units, nchunk, C, T, m);
}

template <typename S>
int ica_step_launch(const S* x, const S* U, const S* b, double* P, double* s, double* q, void* work,
                    int64_t work_bytes, int64_t n, int C, int T, int m, void* stream, const char* who) {
  ISD_CHECK_ARG((x || n == 0) && U && b && P && s && q && work, "%s: null argument", who);   // no trials: x may be null
  ISD_CHECK_ARG(ica_step_shape_ok(n, C, T, m), "%s: n=%lld C=%d T=%d m=%d (need 1 <= C <= 128, T >= 1, 1 <= m <= 64)",
                who, (long long)n, C, T, m);
  const int64_t need = isd_ica_step_work_bytes(n, C, T, m, sizeof(S) == 8);
  ISD_CHECK_ARG(work_bytes >= need, "%s: workspace of %lld bytes, need %lld", who, (long long)work_bytes,
                (long long)need);
  hipStream_t st = (hipStream_t)stream;
  int grid = 0;
  if (n > 0) {
    const int nchunk = (int)cdiv(T, IcaOps<S>::KC), nB = ((m + 15) / 16) * ((C + 15) / 16);
    const int64_t units = n * nchunk;
    const size_t lds = ica_lds_bytes<S>(C, m, true);             // <= 124 KB
    grid = ica_step_grid<S>(n, C, T, m);
    S* w = static_cast<S*>(work);
    int rc;
    if (nB <= 4) rc = ica_step_launch_cp<S, 1>(grid, lds, st, x, U, b, w, units, nchunk, C, T, m);
    else if (nB <= 8) rc = ica_step_launch_cp<S, 2>(grid, lds, st, x, U, b, w, units, nchunk, C, T, m);
    else if (nB <= 16) rc = ica_step_launch_cp<S, 4>(grid, lds, st, x, U, b, w, units, nchunk, C, T, m);
    else rc = ica_step_launch_cp<S, 8>(grid, lds, st, x, U, b, w, units, nchunk, C, T, m);
    if (rc != ISD_OK) return rc;
  }
  const int E = m * C + 2 * m;                                   // with no workgroups the sums are zeros
  hipLaunchKernelGGL((ica_reduce_kernel<S>), dim3((unsigned)cdiv(E, 256)), dim3(256), 0, st,
                     static_cast<const S*>(work), grid, m, C, P, s, q);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

template <typename S>
int spatial_apply_launch(const S* x, const S* M, const S* bias, S* out, int64_t n, int C, int T, int R, void* stream,
                         const char* who) {
  ISD_CHECK_ARG(((x && out) || n == 0) && M, "%s: null argument", who);
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL, "%s: n=%lld", who, (long long)n);
  ISD_CHECK_ARG(C >= 1 && C <= 128 && T >= 1 && R >= 1 && R <= 128,
                "%s: C=%d T=%d R=%d (need 1 <= C <= 128, T >= 1, 1 <= R <= 128)", who, C, T, R);
  if (n == 0) return ISD_OK;
  ISD_CHECK_ARG((const void*)x != (const void*)out, "%s: x and out are the same buffer (not an in-place operation)",
                who);
  const int nchunk = (int)cdiv(T, IcaOps<S>::KC);
  const int64_t units = n * nchunk;
  const size_t lds = ica_lds_bytes<S>(C, std::min(R, kIcaRows), false);          // <= 105 KB
  const dim3 grid((unsigned)ica_grid(units, lds), (unsigned)cdiv(R, kIcaRows)), blk(kIcaThreads);
  hipStream_t st = (hipStream_t)stream;
  return C <= 64 ? launch_lds(spatial_apply_kernel<S, 64>, grid, blk, lds, st, x, M, bias, out, units, nchunk, C, T, R)
                 : launch_lds(spatial_apply_kernel<S, 128>, grid, blk, lds, st, x, M, bias, out, units, nchunk, C, T, R);
}

}  // namespace

extern "C" int64_t isd_ica_step_work_bytes(int64_t n, int C, int T, int m, int is_f64) {
  if (!ica_step_shape_ok(n, C, T, m)) {
    set_error("isd_ica_step_work_bytes: n=%lld C=%d T=%d m=%d (need 1 <= C <= 128, T >= 1, 1 <= m <= 64)",
              (long long)n, C, T, m);
    return ISD_ERR_INVALID;
  }
  const size_t el = is_f64 ? sizeof(double) : sizeof(float);
  if (n == 0) return (int64_t)el;                                // never a zero-byte buffer
  const int grid = is_f64 ? ica_step_grid<double>(n, C, T, m) : ica_step_grid<float>(n, C, T, m);
  return (int64_t)grid * ((int64_t)m * C + 2 * m) * (int64_t)el;
}

extern "C" int isd_ica_step_f32(const float* x, const float* U, const float* b, double* P, double* s, double* q,
                                void* work, int64_t work_bytes, int64_t n, int C, int T, int m, void* stream) {
  return ica_step_launch<float>(x, U, b, P, s, q, work, work_bytes, n, C, T, m, stream, "isd_ica_step_f32");
}

extern "C" int isd_ica_step_f64(const double* x, const double* U, const double* b, double* P, double* s, double* q,
                                void* work, int64_t work_bytes, int64_t n, int C, int T, int m, void* stream) {
  return ica_step_launch<double>(x, U, b, P, s, q, work, work_bytes, n, C, T, m, stream, "isd_ica_step_f64");
}

extern "C" int isd_spatial_apply_f32(const float* x, const float* M, const float* bias, float* out, int64_t n, int C,
                                     int T, int R, void* stream) {
  return spatial_apply_launch<float>(x, M, bias, out, n, C, T, R, stream, "isd_spatial_apply_f32");
}

extern "C" int isd_spatial_apply_f64(const double* x, const double* M, const double* bias, double* out, int64_t n,
                                     int C, int T, int R, void* stream) {
  return spatial_apply_launch<double>(x, M, bias, out, n, C, T, R, stream, "isd_spatial_apply_f64");
}
