// Cross-spectral density by Welch's method: the data-sized steps of isd_amd.connectivity.csd_array_welch and
// spectral_connectivity.  S[k][i][j] = mean over segments (and, over_trials, trials) of X_i[k] conj(X_j[k]) with
// X[k] = sum_t (x[t] - mu) w[t] exp(-2 pi i k t / n_fft) (numpy's rfft sign), scaled to a density by the plan's
// scale[k] = c_k / (sfreq sum w^2).  The plan, its tables and the segment rules are those of psd.hip, unchanged.
//
//   psd_mean_kernel      (psd_common.h) the segment means in fp64.
//   csd_spectra_kernel   the tiling and staging of psd_welch_kernel: 64 rows x up to 64 live bins per workgroup, chunks
//                        of KC samples through LDS with the next chunk in flight.  When a segment completes it stores
//                        a = Re X = sum x w cos and b = -Im X = sum x w sin (divided by sqrt(a^2 + b^2) under
//                        unit_modulus; an exact zero stays zero) into
//                            Z[bin][trial][q][channel],  q = 2 segment + {0: a, 1: b},
//                        channel fastest.  Rows are trial * C + channel, so a tile may straddle trials.  The wave's A
//                        rows are ordered so that a lane's four results are four consecutive rows in both precisions
//                        (the f64 C/D map would give rows g, g + 4, g + 8, g + 12): with C a multiple of 4 they are
//                        four channels of one trial and leave as one vector store, otherwise as four scalar stores.
//                        blockIdx.z owns a range of segments; nothing is summed here, so the split needs no reduce.
//   csd_product_kernel   one wave per (matrix, bin, pair of 16-channel tiles J <= I[, range of pairs]); a matrix is a
//                        trial (per trial, N = S) or everything (over_trials, N = n S: Z[bin] is one contiguous run of
//                        n S (a, b) row pairs).  Lane (g, c) loads a and b of channel 16 I + c and of channel 16 J + c
//                        at pair 4 m + g: that is the A and the B operand of the 16x16x4 MFMA at once, so
//                            Re S_ij += a_i a_j ; += b_i b_j        Im S_ij += a_i b_j ; += b_i (-a_j)
//                        and the mirrored tile with the operands swapped and the products in the same order,
//                            Re S_ji += a_j a_i ; += b_j b_i        Im S_ji += b_j (-a_i) ; += a_j b_i
//                        which is the exact conjugate, bit for bit, because every product is the same product and
//                        every partial sum the negated partial sum.  Missing pairs and channels are zeros in
//                        registers (the inner dimension is padded to whole MFMAs of four pairs).  Both tiles are
//                        stored row-major with (re, im) interleaved: 16 lanes write 16 consecutive complex values.
//                        On a diagonal tile the element above the diagonal comes from the mirrored accumulator and the
//                        diagonal's imaginary part is written as 0.
//   csd_reduce_kernel    over_trials with too few (bin, tile pair) waves to fill the card splits the pairs over
//                        ranges; each leaves unscaled sums in `work`; this kernel adds them in range order, adds the
//                        running sum of the earlier trial chunks, and scales at the last chunk.  No atomics: the split
//                        and the chunks are functions of the shape (and of the chunk budget) alone.
//
// The bound is the output: C^2 K complex values per trial against an inner dimension of S.  No load goes outside x
// (as psd.hip) or outside the Z of the chunk; no store outside Z, the partial sums, or out.
#include <algorithm>
#include <cmath>
#include "psd_common.h"

namespace isd {

constexpr int kCsdMaxChannels = 128;
constexpr int kCsdSplitBelow = 2048;                            // fewer product workgroups than two per SIMD (a wave
constexpr int kCsdSplitTarget = 4096;                           // waits on its loads every four pairs): split the pairs
constexpr int kCsdMinPairs = 8;                                 // of a range
constexpr int64_t kCsdChunkBytes = 256LL << 20;                 // Z + means of one trial chunk
// Per thread: isd_csd_work_bytes and the isd_csd_welch_* call it sizes `work` for read the same value whatever
// another thread sets in between.
static thread_local int64_t g_csd_chunk_bytes = kCsdChunkBytes;

// Z [K][nt][2 S][C] of this chunk's nt trials
template <typename S>
__global__ __launch_bounds__(kPsdThreads, 2) void csd_spectra_kernel(const S* __restrict__ x, const S* __restrict__ tab,
                                                                 const double* __restrict__ means, S* __restrict__ Z,
                                                                 int64_t rows, int C, int64_t nt, int64_t T,
                                                                 int64_t S_, int seg_per_z, int nps, int step, int np,
                                                                 int K, int Kp, int unit_modulus) {
  using O = PsdOps<S>;
  using Acc = typename O::Acc;
  using Vec = typename O::Vec;
  constexpr int KC = O::KC, LD = O::LD, VEC = O::VEC, PF = kPsdRows * KC / kPsdThreads;
  constexpr int NT = kPsdBins / 16;
  constexpr S kTiny = sizeof(S) == 4 ? (S)1e-15 : (S)1e-140;    // a modulus whose square is still far from underflow
  __shared__ __attribute__((aligned(16))) S xs[kPsdRows * LD];
  __shared__ __attribute__((aligned(16))) S cs[kPsdBins * LD];
  __shared__ __attribute__((aligned(16))) S ss[kPsdBins * LD];
  __shared__ double mus[kPsdRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kPsdRows;
  const int nrow = (int)min((int64_t)kPsdRows, rows - row0);
  const int bin0 = blockIdx.y * kPsdBins;
  const int nb = min(NT, (K - bin0 + 15) >> 4);
  const int64_t s_begin = (int64_t)blockIdx.z * seg_per_z;
  const int nseg = (int)min((int64_t)seg_per_z, S_ - s_begin);
  const int nchunk = np / KC;
  const bool live = wave * 16 < nrow;
  const S* xr = x + row0 * T;
  const S* tc = tab + (int64_t)bin0 * np;
  const S* ts = tc + (int64_t)Kp * np;
  // MFMA row i of the wave holds data row arow(i): a lane's results r = 0..3 are then data rows 4 g + r
  const int i16 = lane & 15;
  const int arow = sizeof(S) == 8 ? 4 * (i16 & 3) + (i16 >> 2) : i16;
  const int64_t orow = row0 + wave * 16 + 4 * (lane >> 4);      // the first of the lane's four rows
  const bool vec_ok = (C & 3) == 0;                             // four channels of one trial, 16-byte aligned in Z

  Acc re[NT], im[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) re[b] = im[b] = (Acc)(0);

  S px[PF], pc[PF], ps[PF];
  int c = 0;
  int64_t s = s_begin;
  const double* mp = (means != nullptr && tid < nrow) ? means + (row0 + tid) * S_ : nullptr;
  double mu = mp ? mp[s] : 0.0;
  psd_fetch_tile<S, PF>(px, xr + s * step, T, nrow, nps, tid);
  psd_fetch_tile<S, PF>(pc, tc, np, nb * 16, KC, tid);
  psd_fetch_tile<S, PF>(ps, ts, np, nb * 16, KC, tid);
  const int nunit = nseg * nchunk;
  for (int u = 0; u < nunit; ++u) {
    __syncthreads();
    if (c == 0) {
      if (tid < kPsdRows) mus[tid] = mu;
      __syncthreads();
    }
    psd_store_data<S, PF>(xs, px, mus, nrow, nps - c * KC, tid);
    psd_store_tile<S, PF>(cs, pc, tid);
    psd_store_tile<S, PF>(ss, ps, tid);
    const bool last = c == nchunk - 1;
    const int c1 = last ? 0 : c + 1;
    const int64_t s1 = last ? s + 1 : s;
    if (u + 1 < nunit) {
      if (last) mu = mp ? mp[s1] : 0.0;
      psd_fetch_tile<S, PF>(px, xr + s1 * step + c1 * KC, T, nrow, nps - c1 * KC, tid);
      psd_fetch_tile<S, PF>(pc, tc + c1 * KC, np, nb * 16, KC, tid);
      psd_fetch_tile<S, PF>(ps, ts + c1 * KC, np, nb * 16, KC, tid);
    }
    __syncthreads();
    if (live) {
      const S* pa = xs + (wave * 16 + arow) * LD + VEC * (lane >> 4);
      const S* pbc = cs + i16 * LD + VEC * (lane >> 4);
      const S* pbs = ss + i16 * LD + VEC * (lane >> 4);
      if constexpr (sizeof(S) == 4) {
        switch (nb) {
          case 1: psd_mma_chunk<S, 1>(re, im, pa, pbc, pbs); break;
          case 2: psd_mma_chunk<S, 2>(re, im, pa, pbc, pbs); break;
          case 3: psd_mma_chunk<S, 3>(re, im, pa, pbc, pbs); break;
          default: psd_mma_chunk<S, 4>(re, im, pa, pbc, pbs); break;
        }
      } else {
#pragma unroll
        for (int k = 0; k < KC; k += 4 * VEC) {
          const Vec va = *reinterpret_cast<const Vec*>(pa + k);
#pragma unroll
          for (int b = 0; b < NT; ++b) {
            if (b < nb) {
              const Vec vc = *reinterpret_cast<const Vec*>(pbc + b * 16 * LD + k);
              const Vec vs = *reinterpret_cast<const Vec*>(pbs + b * 16 * LD + k);
#pragma unroll
              for (int v = 0; v < VEC; ++v) {
                re[b] = O::mma(va[v], vc[v], re[b]);
                im[b] = O::mma(va[v], vs[v], im[b]);
              }
            }
          }
        }
      }
      if (last) {                                                // the segment is complete: its spectra leave
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          const int bin = bin0 + b * 16 + i16;
          Acc a = re[b], bb = im[b];
          re[b] = im[b] = (Acc)(0);
          if (unit_modulus) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              S m = sqrt(a[r] * a[r] + bb[r] * bb[r]);
              if (m < kTiny) {                                   // the squares lose bits or underflow: scale first
                const S big = max(fabs(a[r]), fabs(bb[r]));
                if (big > (S)0) {
                  a[r] /= big;
                  bb[r] /= big;
                  m = sqrt(a[r] * a[r] + bb[r] * bb[r]);         // in [1, sqrt 2]
                }
              }
              if (m > (S)0) {                                    // only an exact zero stays zero
                a[r] /= m;
                bb[r] /= m;
              }
            }
          }
          if (bin < K && orow < rows) {
            if (vec_ok) {                                        // rows is a multiple of 4 too: all four rows exist
              const int64_t trial = orow / C;
              const int ch = (int)(orow - trial * C);
              S* zp = Z + ((((int64_t)bin * nt + trial) * (2 * S_) + 2 * s) * C + ch);
              *reinterpret_cast<Acc*>(zp) = a;
              *reinterpret_cast<Acc*>(zp + C) = bb;
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int64_t row = orow + r;
                if (row < rows) {
                  const int64_t trial = row / C;
                  const int ch = (int)(row - trial * C);
                  S* zp = Z + ((((int64_t)bin * nt + trial) * (2 * S_) + 2 * s) * C + ch);
                  zp[0] = a[r];
                  zp[C] = bb[r];
                }
              }
            }
          }
        }
      }
    }
    c = c1;
    s = s1;
  }
}

// Z [K][M][P][2][C]: M matrices of P (a, b) row pairs each.  One wave per (range z, matrix, bin, tile pair); dst is
// out [M][K][C][C][2] scaled by sc(k) / N, or with `partial` [Zr][M = 1][K][C][C][2] unscaled.
template <typename S>
__global__ __launch_bounds__(kPsdThreads) void csd_product_kernel(const S* __restrict__ Z, const S* __restrict__ scale,
                                                                  S* __restrict__ dst, int64_t M, int64_t P,
                                                                  int64_t pairs_per_z, int C, int K, int64_t waves,
                                                                  double N, int use_scale, int partial) {
  using O = PsdOps<S>;
  using Acc = typename O::Acc;
  using V2 = S __attribute__((ext_vector_type(2)));              // f32x2 / f64x2: (re, im), one store
  const int lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
  const int64_t w = (int64_t)blockIdx.x * (kPsdThreads / 64) + (threadIdx.x >> 6);
  if (w >= waves) return;                                        // wave-uniform
  const int nct = (C + 15) >> 4, ntp = nct * (nct + 1) / 2;
  int tp = (int)(w % ntp);
  int64_t rest = w / ntp;
  const int bin = (int)(rest % K);
  rest /= K;
  const int64_t m = rest % M, z = rest / M;
  int I = 0;
  while (tp > I) {                                               // tile pair tp -> (I, J), J <= I; at most 8 steps
    tp -= I + 1;
    ++I;
  }
  const int J = tp;
  const int ci = 16 * I + c16, cj = 16 * J + c16;
  const bool in_i = ci < C, in_j = cj < C;
  const int64_t p_begin = z * pairs_per_z, p_end = min(P, p_begin + pairs_per_z);
  const S* zb = Z + ((int64_t)bin * M + m) * P * 2 * C;

  Acc re = (Acc)(0), imn = (Acc)(0), rem = (Acc)(0), imm = (Acc)(0);
  for (int64_t p0 = p_begin; p0 < p_end; p0 += 4) {
    const int64_t p = p0 + g;
    const bool in_p = p < p_end;
    const S* zp = zb + p * 2 * C;
    const S ai = (in_p && in_i) ? zp[ci] : (S)0;
    const S bi = (in_p && in_i) ? zp[C + ci] : (S)0;
    const S aj = (in_p && in_j) ? zp[cj] : (S)0;
    const S bj = (in_p && in_j) ? zp[C + cj] : (S)0;
    re = O::mma(ai, aj, re);
    re = O::mma(bi, bj, re);
    imn = O::mma(ai, bj, imn);
    imn = O::mma(bi, -aj, imn);
    rem = O::mma(aj, ai, rem);
    rem = O::mma(bj, bi, rem);
    imm = O::mma(bj, -ai, imm);
    imm = O::mma(aj, bi, imm);
  }

  S sc = (S)1;
  if (!partial) sc = (use_scale ? scale[bin] : (S)1) / (S)N;
  S* ob = dst + (((partial ? z : m) * K + bin) * (int64_t)C * C) * 2;
  const int y = c16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int xr = O::lane_row(lane, r);
    if (I != J) {
      if (16 * I + xr < C && in_j) {
        V2 v = {re[r] * sc, imn[r] * sc};
        *reinterpret_cast<V2*>(ob + ((int64_t)(16 * I + xr) * C + cj) * 2) = v;
      }
      if (16 * J + xr < C && in_i) {
        V2 v = {rem[r] * sc, imm[r] * sc};
        *reinterpret_cast<V2*>(ob + ((int64_t)(16 * J + xr) * C + ci) * 2) = v;
      }
    } else if (16 * I + xr < C && in_j) {
      V2 v;
      if (xr > y) {
        v = V2{re[r] * sc, imn[r] * sc};
      } else if (xr < y) {
        v = V2{rem[r] * sc, imm[r] * sc};
      } else {
        v = V2{re[r] * sc, (S)0};
      }
      *reinterpret_cast<V2*>(ob + ((int64_t)(16 * I + xr) * C + cj) * 2) = v;
    }
  }
}

// dst[e] = (acc ? acc[e] : 0) + sum_z part[z][e], times sc(k) / N when `final`; e over [K][C][C][2]
template <typename S>
__global__ __launch_bounds__(256) void csd_reduce_kernel(const S* __restrict__ part, const S* acc,
                                                         const S* __restrict__ scale, S* dst, int64_t E,
                                                         int64_t per_bin, int Zr, double N, int use_scale, int final) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  S a = acc ? acc[e] : (S)0;
  for (int z = 0; z < Zr; ++z) a += part[(int64_t)z * E + e];    // range order = trial, segment order
  if (final) a *= (use_scale ? scale[e / per_bin] : (S)1) / (S)N;
  dst[e] = a;
}

}  // namespace isd

using namespace isd;

namespace {

struct CsdLayout {
  int64_t S_, nc;                // segments per trial; trials per chunk
  int64_t means, z, part, acc, slack, end;   // byte offsets into the workspace; part and acc are empty without over_trials
  int zr_max;                    // over_trials: ranges of a full chunk, the most any chunk has ...
  int64_t per;                   // ... because every chunk is cut into ranges of this many pairs
};

struct CsdSplit {
  int Zr;
  int64_t per;
};

// over_trials: the ranges of P pairs; a function of the shape alone
CsdSplit csd_split(int K, int C, int64_t P) {
  const int nct = (C + 15) / 16, ntp = nct * (nct + 1) / 2;
  const int64_t base = cdiv((int64_t)K * ntp, kPsdThreads / 64);
  int64_t Zr = base >= kCsdSplitBelow ? 1 : std::min<int64_t>(cdiv(P, kCsdMinPairs), cdiv(kCsdSplitTarget, base));
  Zr = std::max<int64_t>(Zr, 1);
  const int64_t per = cdiv(cdiv(P, Zr), 4) * 4;                  // whole MFMAs of four pairs
  return {(int)cdiv(P, per), per};
}

CsdLayout csd_layout(const isd_psd_plan* p, int64_t n, int64_t C, int64_t T, int over_trials, int is_f64) {
  CsdLayout L = {};
  WorkCarver c;
  const int64_t el = is_f64 ? 8 : 4;
  L.S_ = psd_segments(p, T);
  if (n == 0 || L.S_ == 0) {
    L.slack = c.take(256);                                       // never a zero-byte buffer
    L.end = c.end;
    return L;
  }
  const int64_t per_trial = C * L.S_ * 8 + (int64_t)p->K * 2 * L.S_ * C * el;
  L.nc = std::max<int64_t>(1, std::min<int64_t>(n, g_csd_chunk_bytes / std::max<int64_t>(per_trial, 1)));
  L.nc = std::min<int64_t>(L.nc, (1LL << 30) / std::max<int64_t>(1, std::max<int64_t>(C, 2 * L.S_)));
  L.means = c.take(L.nc * C * L.S_ * 8, 256);
  L.z = c.take((int64_t)p->K * L.nc * 2 * L.S_ * C * el, 256);
  const int64_t E = (int64_t)p->K * C * C * 2;
  // The split is taken once, from a full chunk, and a shorter last chunk is cut into ranges of the same length: it
  // then has no more ranges than `part` holds (a split of its own can have more: the count is not monotone in P).
  const CsdSplit full = csd_split(p->K, (int)C, L.nc * L.S_);
  L.zr_max = over_trials ? full.Zr : 0;
  L.per = full.per;
  L.part = c.take(over_trials ? L.zr_max * E * el : 0, 256);
  L.acc = c.take(over_trials ? E * el : 0, 256);
  L.slack = c.take(256, 256);
  L.end = c.end;
  return L;
}

template <typename S>
int csd_launch(const isd_psd_plan* p, const S* x, S* out, int64_t n, int64_t C, int64_t T, int over_trials,
               int unit_modulus, void* work, void* stream, const char* who) {
  ISD_CHECK_ARG(p, "%s: null plan", who);
  ISD_CHECK_ARG(n >= 0, "%s: n=%lld", who, (long long)n);
  ISD_CHECK_SUPPORTED(C >= 1 && C <= kCsdMaxChannels, "%s: C=%lld (need 1 <= C <= %d)", who, (long long)C,
                      kCsdMaxChannels);
  if (n == 0) return ISD_OK;
  ISD_CHECK_SUPPORTED(T >= p->n_per_seg, "%s: T=%lld is shorter than n_per_seg=%d", who, (long long)T, p->n_per_seg);
  const bool f64 = sizeof(S) == 8;
  const CsdLayout L = csd_layout(p, n, C, T, over_trials, f64);
  ISD_CHECK_SUPPORTED(L.S_ <= (1LL << 28), "%s: %lld segments (at most 2^28)", who, (long long)L.S_);
  ISD_CHECK_ARG(x && out && work, "%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  const S* tab = f64 ? (const S*)p->d_tab64 : (const S*)p->d_tab32;
  const S* scale = f64 ? (const S*)p->d_scale64 : (const S*)p->d_scale32;
  const int np = f64 ? p->np64 : p->np32;
  char* wb = static_cast<char*>(work);
  double* means = reinterpret_cast<double*>(wb + L.means);
  S* Z = reinterpret_cast<S*>(wb + L.z);
  S* part = reinterpret_cast<S*>(wb + L.part);
  S* acc = reinterpret_cast<S*>(wb + L.acc);
  const int K = p->K, Ci = (int)C;
  const int nct = (Ci + 15) / 16, ntp = nct * (nct + 1) / 2;
  const int64_t E = (int64_t)K * C * C * 2;
  const int bin_tiles = (int)cdiv(K, kPsdBins);
  const int64_t nchunks = cdiv(n, L.nc);
  const int use_scale = !unit_modulus;

  for (int64_t ic = 0; ic < nchunks; ++ic) {
    const int64_t t0 = ic * L.nc, nt = std::min<int64_t>(L.nc, n - t0), rows = nt * C;
    const S* xc = x + t0 * C * T;
    if (p->remove_dc) {
      const int64_t units = rows * L.S_;
      const unsigned gm = (unsigned)std::min<int64_t>(cdiv(units, 4), 256 * 16);
      hipLaunchKernelGGL((psd_mean_kernel<S>), dim3(gm), dim3(kPsdThreads), 0, st, xc, means, units, L.S_, T,
                         p->n_per_seg, p->step);
      ISD_LAUNCH_CHECK();
    }
    // spectra: segments over blockIdx.z when the (row, bin) tiles are few; every segment is stored on its own
    const int64_t row_tiles = cdiv(rows, kPsdRows);
    const int64_t base = row_tiles * bin_tiles;
    int64_t Zs = base >= kPsdSplitBelow ? 1 : std::min<int64_t>(L.S_, cdiv(kPsdSplitTarget, base));
    const int64_t seg_per_z = cdiv(L.S_, Zs);
    Zs = cdiv(L.S_, seg_per_z);
    ISD_CHECK_SUPPORTED(Zs <= 65535, "%s: %lld segment ranges", who, (long long)Zs);
    hipLaunchKernelGGL((csd_spectra_kernel<S>), dim3((unsigned)row_tiles, (unsigned)bin_tiles, (unsigned)Zs),
                       dim3(kPsdThreads), 0, st, xc, tab, p->remove_dc ? (const double*)means : nullptr, Z, rows, Ci,
                       nt, T, L.S_, (int)seg_per_z, p->n_per_seg, p->step, np, K, p->Kp, unit_modulus);
    ISD_LAUNCH_CHECK();

    if (!over_trials) {
      const int64_t waves = nt * K * ntp;
      hipLaunchKernelGGL((csd_product_kernel<S>), dim3((unsigned)cdiv(waves, kPsdThreads / 64)), dim3(kPsdThreads), 0,
                         st, (const S*)Z, scale, out + t0 * E, nt, L.S_, L.S_, Ci, K, waves, (double)L.S_, use_scale,
                         0);
      ISD_LAUNCH_CHECK();
    } else {
      const int64_t P = nt * L.S_;
      const CsdSplit sp = {(int)cdiv(P, L.per), L.per};
      ISD_CHECK_ARG(sp.Zr >= 1 && sp.Zr <= L.zr_max, "%s: %d ranges for room for %d", who, sp.Zr, L.zr_max);
      const bool direct = nchunks == 1 && sp.Zr == 1;
      const int64_t waves = (int64_t)sp.Zr * K * ntp;
      hipLaunchKernelGGL((csd_product_kernel<S>), dim3((unsigned)cdiv(waves, kPsdThreads / 64)), dim3(kPsdThreads), 0,
                         st, (const S*)Z, scale, direct ? out : part, (int64_t)1, P, sp.per, Ci, K, waves,
                         (double)(n * L.S_), use_scale, direct ? 0 : 1);
      ISD_LAUNCH_CHECK();
      if (!direct) {
        const bool last = ic == nchunks - 1;
        hipLaunchKernelGGL((csd_reduce_kernel<S>), dim3((unsigned)cdiv(E, 256)), dim3(256), 0, st, (const S*)part,
                           ic > 0 ? (const S*)acc : (const S*)nullptr, scale, last ? out : acc, E, C * C * 2, sp.Zr,
                           (double)(n * L.S_), use_scale, last ? 1 : 0);
        ISD_LAUNCH_CHECK();
      }
    }
  }
  return ISD_OK;
}

}  // namespace

extern "C" int64_t isd_csd_chunk_bytes(int64_t bytes) {
  const int64_t before = g_csd_chunk_bytes;
  if (bytes >= 0) g_csd_chunk_bytes = bytes == 0 ? kCsdChunkBytes : bytes;
  return before;
}

extern "C" int64_t isd_csd_work_bytes(const isd_psd_plan* p, int64_t n, int64_t C, int64_t T, int over_trials,
                                      int is_f64) {
  if (!p || n < 0 || C < 1 || C > kCsdMaxChannels) {
    set_error("isd_csd_work_bytes: null plan, n=%lld or C=%lld", (long long)n, (long long)C);
    return ISD_ERR_INVALID;
  }
  return csd_layout(p, n, C, T, over_trials, is_f64).end;
}

extern "C" int isd_csd_welch_f32(const isd_psd_plan* plan, const float* x, float* out, int64_t n, int64_t C, int64_t T,
                                 int over_trials, int unit_modulus, void* work, void* stream) {
  return csd_launch<float>(plan, x, out, n, C, T, over_trials, unit_modulus, work, stream, "isd_csd_welch_f32");
}

extern "C" int isd_csd_welch_f64(const isd_psd_plan* plan, const double* x, double* out, int64_t n, int64_t C,
                                 int64_t T, int over_trials, int unit_modulus, void* work, void* stream) {
  return csd_launch<double>(plan, x, out, n, C, T, over_trials, unit_modulus, work, stream, "isd_csd_welch_f64");
}
