// Time-resolved spectral connectivity: the data-sized step of isd_amd.connectivity.spectral_connectivity_time.
// z [n][C][F][T] complex is the wavelet map of n trials (csrc/tfr.hip, mode 0).  Per (trial, frequency, pair of
// channels l, j), with w = a + i b, s = w_l conj(w_j), u = s / |s| (0 where |s| = 0) and the sums over the samples
// t0 <= t < t1, N = t1 - t0 of them:
//
//   Hermitian   sum Re s, sum Im s, P_c = sum |w_c|^2       coh = |sum s| / sqrt(P_l P_j),  imcoh = sum Im s / sqrt(..)
//   unit        sum Re u, sum Im u,  E = sum u / N           plv = |E|,  ciplv = |Im E| / sqrt((1 - |Re E|)(1 + |Re E|))
//   lag         sum Im s, sum |Im s|, sum (Im s)^2 and the counts n+ of Im s > 0 and n- of Im s < 0
//               pli = |n+ - n-| / N,  dpli = (n+ + (N - n+ - n-) / 2) / N   (sum sign = n+ - n-, H(0) = 1/2)
//               wpli = |sum Im s| / sum |Im s|,  wpli2_debiased = ((sum Im s)^2 - sum (Im s)^2) / ((sum |Im s|)^2 - ..)
//
//   contime_pair_kernel<S, HERM, UNIT, LAG, AVG>
//     one wave (one workgroup of 64) per (trial, frequency, pair of 16-channel tiles J <= I), the tile pairs enumerated
//     as in envcorr_pair_kernel and csd_product_kernel; with AVG one wave per (frequency, tile pair) that walks the n
//     trials in index order.  The three groups are template switches: a call pays for the sums of the groups whose
//     measures it asks for and no other (a 'coh' call has no sqrt / divide of u, no lag accumulators).
//     The channel row (trial, c, f) of z is T complex values long and rows of one trial are F T apart.  The samples
//     [t0, t1) run through LDS in chunks of kConChunk, the next chunk's loads in flight in registers: per (channel,
//     sample) one record (a, b) or, with UNIT, (a, b, ua, ub), (ua, ub) = (a, b) / sqrt(a^2 + b^2) formed ONCE per
//     record at staging (u_l conj(u_j) = s / |s|; an exact zero of |w|, also one that a^2 + b^2 underflows to, gives
//     the zero record and contributes 0).  A staged row is kConChunk records and 16 bytes of padding, so that the 16
//     channels read at one sample start on 16 different 16-byte slots of the 256-byte bank row (8-byte records: on 16
//     different 8-byte pairs of banks); the four l records of a lane are a broadcast within its 16 lanes.
//     Lane (g, c) owns the four pairs (l = 16 I + 4 g + k, j = 16 J + c).  Im s = b_l a_j - a_l b_j is Kahan's
//     compensated cross product in S (w = a_l b_j, err = fma(-a_l, b_j, w), im = fma(b_l, a_j, -w) + err): its sign
//     is what pli and dpli are made of, and plain fp32 cancellation gets the sign of a nearly in-phase pair wrong.
//     Every sum is fp64 (the two counts are integers, exact as well), in sample order, with no atomics: bitwise
//     repeatable.  sum |w_c|^2 of the 32 staged rows is kept once per row (by lane r and, the same bits, lane r + 32)
//     and handed round through LDS after the last chunk.  The epilogue forms the measures of `mask` in fp64, rounds
//     once and stores the value at [l][j] and its mirror at [j][l]: the same bits, or for the antisymmetric ones -v
//     (imcoh) and 1 - v (dpli) in S arithmetic.
//     On a diagonal tile the lanes with l > j store, and l = j stores the diagonal, which is set, not computed:
//     coh = plv = 1, imcoh = pli = 0, dpli = 1/2, ciplv = wpli = wpli2_debiased = NaN (0 / 0).
//     With AVG the per-trial fp64 measures are added in trial order, divided by n and stored once.
//
// No load goes outside z: channels past C and samples outside [t0, t1) are zero records in registers and are never
// loaded.  No store goes outside out, and nothing is stored for a pair with l or j past C.
#include <cmath>
#include "common.h"

namespace isd {

constexpr int kConMaxChannels = 128;
constexpr int kConChunk = 16;                                   // samples per staged chunk
// measure m is bit m of the mask; measures are stored in bit order
enum { kCoh = 0, kImcoh, kPlv, kCiplv, kPli, kDpli, kWpli, kWpli2, kConMeasures };
constexpr int kConHermMask = 1 << kCoh | 1 << kImcoh, kConUnitMask = 1 << kPlv | 1 << kCiplv;
constexpr int kConLagMask = 1 << kPli | 1 << kDpli | 1 << kWpli | 1 << kWpli2;

__device__ __forceinline__ float con_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double con_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float con_sqrt(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double con_sqrt(double a) { return __builtin_sqrt(a); }
// Im (w_l conj(w_j)) = b_l a_j - a_l b_j, compensated: w is a rounded product and err its exact rounding error
template <typename S>
__device__ __forceinline__ S con_cross(S al, S bl, S aj, S bj) {
  const S w = al * bj;
  const S err = con_fma(-al, bj, w);
  return con_fma(bl, aj, -w) + err;
}

template <typename S, bool HERM, bool UNIT, bool LAG, bool AVG>
__global__ __launch_bounds__(64) void contime_pair_kernel(const S* __restrict__ z, S* __restrict__ out, int64_t n,
                                                          int C, int F, int64_t T, int64_t t0, int64_t t1, int mask) {
  using V2 = S __attribute__((ext_vector_type(2)));
  constexpr int KC = kConChunk;
  constexpr int REC = UNIT ? 4 : 2;                               // values per record
  constexpr int RS = KC * REC + 16 / (int)sizeof(S);              // values per staged row: 16 bytes of padding
  constexpr int NF = 32 * KC / 64;                                // (channel, sample) records a lane stages per chunk
  constexpr bool IM = HERM || LAG;                                // sum Im s is kept
  __shared__ __attribute__((aligned(16))) S rec[32 * RS];
  const int lane = threadIdx.x, g = lane >> 4, c16 = lane & 15;
  const int nct = (C + 15) >> 4, ntp = nct * (nct + 1) / 2;
  int64_t bid = blockIdx.x;
  int tp = (int)(bid % ntp);
  bid /= ntp;
  const int f = (int)(bid % F);
  const int64_t first = AVG ? 0 : bid / F, trials = AVG ? n : 1;
  int I = 0;
  while (tp > I) {                                               // tile pair tp -> (I, J), J <= I; at most 8 steps
    tp -= I + 1;
    ++I;
  }
  const int J = tp;
  const int j = 16 * J + c16;
  const double N = (double)(t1 - t0);

  // where measure m of pair k goes: slot = its rank among the measures asked for
  auto put = [&](int k, int m, double v, int64_t trial) {
    const int l = 16 * I + 4 * g + k;
    if (j >= C || l >= C || (I == J && l < j)) return;           // a diagonal tile: the pair belongs to the lane l > j
    const int slot = __builtin_popcount(mask & ((1 << m) - 1));
    S* ob = out + (((int64_t)slot * (AVG ? 1 : n) + trial) * F + f) * C * C;
    if (l == j) {                                                // set, not computed
      const S nan = (S)__builtin_nan("");
      ob[(int64_t)l * C + l] = (m == kCoh || m == kPlv) ? (S)1
                               : (m == kImcoh || m == kPli) ? (S)0
                               : m == kDpli ? (S)0.5 : nan;
      return;
    }
    const S vs = (S)v;
    ob[(int64_t)l * C + j] = vs;
    ob[(int64_t)j * C + l] = m == kImcoh ? -vs : (m == kDpli ? (S)1 - vs : vs);
  };

  double av[AVG ? 4 : 1][kConMeasures];
  if (AVG) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int m = 0; m < kConMeasures; ++m) av[k][m] = 0.0;
  }

  // staging: record r of this lane is sample (lane & 15) of staged row 4 r + (lane >> 4); rows 0..15 are tile I
  const int ft = lane & (KC - 1);
  const S* rl = rec + (4 * g) * RS;                              // this lane's four l rows (a broadcast per 16 lanes)
  const S* rj = rec + (16 + c16) * RS;                           // its j row
  const S* rp = rec + (lane & 31) * RS;                          // the row whose power this lane sums

  for (int64_t trial = first; trial < first + trials; ++trial) {
    const V2* zt = reinterpret_cast<const V2*>(z) + (trial * C * F + f) * T;
    V2 pz[NF];
    auto fetch = [&](int64_t tb) {
#pragma unroll
      for (int r = 0; r < NF; ++r) {
        const int srow = 4 * r + (lane >> 4);
        const int ch = 16 * (srow < 16 ? I : J) + (srow & 15);
        const bool in = ch < C && tb + ft < t1;                  // tb >= t0 >= 0
        pz[r] = in ? zt[(int64_t)ch * F * T + tb + ft] : V2{(S)0, (S)0};
      }
    };
    auto stage = [&]() {
#pragma unroll
      for (int r = 0; r < NF; ++r) {
        S* at = rec + (4 * r + (lane >> 4)) * RS + ft * REC;
        *reinterpret_cast<V2*>(at) = pz[r];
        if (UNIT) {
          const S m2 = con_fma(pz[r][0], pz[r][0], pz[r][1] * pz[r][1]);
          const S inv = m2 > (S)0 ? (S)1 / con_sqrt(m2) : (S)0;
          *reinterpret_cast<V2*>(at + 2) = V2{pz[r][0] * inv, pz[r][1] * inv};
        }
      }
    };

    double sre[4], sim[4], ure[4], uim[4], aim[4], im2[4], pown = 0.0;
    int npos[4], nneg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sre[k] = sim[k] = ure[k] = uim[k] = aim[k] = im2[k] = 0.0;
      npos[k] = nneg[k] = 0;
    }

    fetch(t0);
    for (int64_t tb = t0; tb < t1; tb += KC) {
      wave_lds_sync();                                           // the last chunk's reads are done
      stage();
      wave_lds_sync();
      if (tb + KC < t1) fetch(tb + KC);
      const int nt = (int)min((int64_t)KC, t1 - tb);
      for (int t = 0; t < nt; ++t) {
        const V2 vj = *reinterpret_cast<const V2*>(rj + t * REC);
        V2 uj = {(S)0, (S)0};
        if (UNIT) uj = *reinterpret_cast<const V2*>(rj + t * REC + 2);
        if (HERM) {                                              // sum |w|^2 of staged row lane & 31, once per row
          const V2 vp = *reinterpret_cast<const V2*>(rp + t * REC);
          pown += (double)con_fma(vp[0], vp[0], vp[1] * vp[1]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const V2 vl = *reinterpret_cast<const V2*>(rl + k * RS + t * REC);
          if (HERM) {
            sre[k] += (double)con_fma(vl[0], vj[0], vl[1] * vj[1]);
          }
          if (UNIT) {
            const V2 ul = *reinterpret_cast<const V2*>(rl + k * RS + t * REC + 2);
            ure[k] += (double)con_fma(ul[0], uj[0], ul[1] * uj[1]);
            uim[k] += (double)con_fma(ul[1], uj[0], -(ul[0] * uj[1]));
          }
          if (IM) {
            const S im = con_cross<S>(vl[0], vl[1], vj[0], vj[1]);
            const double D = (double)im;
            sim[k] += D;
            if (LAG) {
              aim[k] += fabs(D);
              im2[k] = fma(D, D, im2[k]);
              npos[k] += im > (S)0 ? 1 : 0;
              nneg[k] += im < (S)0 ? 1 : 0;
            }
          }
        }
      }
    }

    double pl[4] = {0.0, 0.0, 0.0, 0.0}, pj = 0.0;
    if (HERM) {                                                  // hand the 32 row powers round through LDS
      double* pw = reinterpret_cast<double*>(rec);
      wave_lds_sync();                                           // the last chunk's reads are done
      if (lane < 32) pw[lane] = pown;
      wave_lds_sync();
      pj = pw[16 + c16];
#pragma unroll
      for (int k = 0; k < 4; ++k) pl[k] = pw[4 * g + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // no contraction here: with one sample (sum Im s)^2 and sum (Im s)^2 are the same rounded square, and their
      // difference must be the exact 0 of the formula (0 / 0), not the rounding error an fma would leave
#pragma clang fp contract(off)
      double v[kConMeasures] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (HERM) {
        const double den = sqrt(pl[k] * pj);
        v[kCoh] = sqrt(sre[k] * sre[k] + sim[k] * sim[k]) / den;
        v[kImcoh] = sim[k] / den;
      }
      if (UNIT) {
        const double er = ure[k] / N, ei = uim[k] / N;
        v[kPlv] = sqrt(er * er + ei * ei);
        v[kCiplv] = fabs(ei) / sqrt((1.0 - fabs(er)) * (1.0 + fabs(er)));
      }
      if (LAG) {
        const double np = (double)npos[k], nn = (double)nneg[k];
        v[kPli] = fabs(np - nn) / N;
        v[kDpli] = (np + 0.5 * (N - np - nn)) / N;
        v[kWpli] = fabs(sim[k]) / aim[k];
        v[kWpli2] = (sim[k] * sim[k] - im2[k]) / (aim[k] * aim[k] - im2[k]);
      }
#pragma unroll
      for (int m = 0; m < kConMeasures; ++m) {
        const bool have = (m <= kImcoh && HERM) || (m >= kPlv && m <= kCiplv && UNIT) || (m >= kPli && LAG);
        if (!have || !((mask >> m) & 1)) continue;
        if (AVG)
          av[k][m] += v[m];
        else
          put(k, m, v[m], trial);
      }
    }
  }

  if (AVG) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int m = 0; m < kConMeasures; ++m)
        if ((mask >> m) & 1) put(k, m, av[k][m] / (double)n, 0);
  }
}

}  // namespace isd

using namespace isd;

namespace {

template <typename S, bool AVG>
void contime_dispatch(int groups, dim3 grid, hipStream_t st, const S* z, S* out, int64_t n, int C, int F, int64_t T,
                      int64_t t0, int64_t t1, int mask) {
  const dim3 block(64);
#define ISD_CONTIME_CASE(G, H, U, L)                                                                              \
  case G:                                                                                                         \
    hipLaunchKernelGGL((contime_pair_kernel<S, H, U, L, AVG>), grid, block, 0, st, z, out, n, C, F, T, t0, t1, mask); \
    break;
  switch (groups) {                                              // bit 0 Hermitian, bit 1 unit-modulus, bit 2 lag
    ISD_CONTIME_CASE(1, true, false, false)
    ISD_CONTIME_CASE(2, false, true, false)
    ISD_CONTIME_CASE(3, true, true, false)
    ISD_CONTIME_CASE(4, false, false, true)
    ISD_CONTIME_CASE(5, true, false, true)
    ISD_CONTIME_CASE(6, false, true, true)
    ISD_CONTIME_CASE(7, true, true, true)
  }
#undef ISD_CONTIME_CASE
}

template <typename S>
int contime_launch(const S* z, S* out, int64_t n, int64_t C, int64_t F, int64_t T, int64_t t0, int64_t t1, int mask,
                   int average, void* stream, const char* who) {
  ISD_CHECK_ARG(n >= 0, "%s: n=%lld", who, (long long)n);
  ISD_CHECK_SUPPORTED(C >= 1 && C <= kConMaxChannels, "%s: C=%lld (need 1 <= C <= %d)", who, (long long)C,
                      kConMaxChannels);
  ISD_CHECK_ARG(mask > 0 && mask < (1 << kConMeasures), "%s: methods_mask=%d (need 1 .. %d)", who, mask,
                (1 << kConMeasures) - 1);
  ISD_CHECK_ARG(n > 0 || !average, "%s: the average of n=0 trials", who);
  if (n == 0) return ISD_OK;
  ISD_CHECK_ARG(F >= 1 && T >= 1, "%s: F=%lld, T_out=%lld (need >= 1)", who, (long long)F, (long long)T);
  ISD_CHECK_ARG(0 <= t0 && t0 < t1 && t1 <= T, "%s: t0=%lld, t1=%lld (need 0 <= t0 < t1 <= T_out=%lld)", who,
                (long long)t0, (long long)t1, (long long)T);
  ISD_CHECK_ARG(z && out, "%s: null argument", who);
  const int nct = ((int)C + 15) / 16, ntp = nct * (nct + 1) / 2;
  const int64_t waves = (average ? 1 : n) * F * ntp;
  ISD_CHECK_SUPPORTED(F <= 0x7fffffffLL && waves <= 0x7fffffffLL,
                      "%s: n=%lld trials of %lld frequencies and %lld channels are more workgroups than one launch "
                      "holds", who, (long long)n, (long long)F, (long long)C);
  const int groups = ((mask & kConHermMask) ? 1 : 0) | ((mask & kConUnitMask) ? 2 : 0) | ((mask & kConLagMask) ? 4 : 0);
  const dim3 grid((unsigned)waves);
  hipStream_t st = (hipStream_t)stream;
  if (average)
    contime_dispatch<S, true>(groups, grid, st, z, out, n, (int)C, (int)F, T, t0, t1, mask);
  else
    contime_dispatch<S, false>(groups, grid, st, z, out, n, (int)C, (int)F, T, t0, t1, mask);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

}  // namespace

extern "C" int isd_contime_f32(const float* z, float* out, int64_t n, int64_t C, int64_t F, int64_t T_out, int64_t t0,
                               int64_t t1, int methods_mask, int average, void* stream) {
  return contime_launch<float>(z, out, n, C, F, T_out, t0, t1, methods_mask, average, stream, "isd_contime_f32");
}

extern "C" int isd_contime_f64(const double* z, double* out, int64_t n, int64_t C, int64_t F, int64_t T_out,
                               int64_t t0, int64_t t1, int methods_mask, int average, void* stream) {
  return contime_launch<double>(z, out, n, C, F, T_out, t0, t1, methods_mask, average, stream, "isd_contime_f64");
}
