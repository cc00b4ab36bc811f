// Complex FIR bank over the rows of a [n][C][T] array: the data-sized step of isd_amd.tfr_array_morlet / tfr.cwt.
//   out[row][f][t] = sum_k w_f[k] x[row][t decim + h_f - k],   h_f = (len(w_f) - 1) / 2,   x zero outside [0, T)
// i.e. np.convolve(x[row], w_f, 'same')[::decim].  Nothing here knows about Morlet wavelets: the taps, their lengths
// and every argument check of the transform are host work (isd_amd/tfr.py).
//
// Formulation.  A product on the fp32 / fp64 matrix cores (mfma 16x16x4) with the Hankel operand of ts_conv_tiles
// (tsception.hip): time on the M side, taps on K, A[i][k] = xs[(t0 + i) decim + k] read straight from an LDS tile of
// the row.  The N side is eight frequencies x (re, im): the plan sorts the frequencies by length, cuts them into
// groups of eight and stores per group a table B[k][2 f + c] of the taps, reversed, centred on the group's longest
// wavelet (half length H) and zero elsewhere, K padded to a multiple of 16 (one 16- / 32-byte B load per lane feeds
// four k steps of eight M tiles).  A step of decim on the M side costs
// nothing: only kept samples are computed.  The arithmetic spent on the zeros of the shorter wavelets of a group is
// the price of this layout (DESIGN.md 3.15 has the fractions); equal lengths (n_cycles = freqs / 2) pay none.
//
//   tfr_cwt_kernel<X, S, MODE>   blockIdx.x = (row or channel, time tile), blockIdx.y = a range of groups.  The workgroup
//       stages the tile's samples with a halo of the plan's longest half length on both sides in LDS, zero outside the
//       row: x is read once per (row, time tile) and reused by every frequency.  Its four waves share out the items
//       (chunk of 128 outputs, group); an item is eight accumulators (M tiles) fed by one B load per four k steps, the
//       next load on its way from L2 meanwhile.  re and im of a frequency land in neighbouring lanes; one exchange
//       leaves each lane with two whole complex samples, so every epilogue is in-lane: the pair as one 8- / 16-byte
//       store, or re^2 + im^2.
//       MODE 0 complex, 1 power, 5 phase (atan2 in fp64, in-lane): one trial per workgroup, every group
//       (blockIdx.y has one value).
//       (X, S) = (float, double): float samples, the product in fp64 -- the phase and the inter-trial coherence of
//       the f32 entry, which depend on the relative error of a weak sample.
//       MODE 2 avg_power, 3 itc, 4 both: the workgroup owns (channel, time tile, its groups) and walks the trials in
//       index order; a wave has at most ONE item, so its sums stay in registers, in fp64 for both input types, and
//       are stored once.  No atomics, nothing of size n C F T is written, the same bits on every run.  x is read once
//       per group range here (from L2: the workgroups of one tile run together).
//
//   tfr_mean_kernel   one wave per row: its mean in fp64, into `work`.  The samples are staged minus that mean, and the
//       epilogue adds mean x (the sum of the taps that met a sample of the row) back in fp64, from prefix sums of
//       the taps the plan holds (away from the row's ends: the whole sum).  The result is unchanged in exact
//       arithmetic; in fp32 a trial that sits at -200 no longer costs 200 x the rounding error of one at 0, which is
//       what the phase, and with it the inter-trial coherence, of a weak sample is sensitive to.
//
// Tiling is a function of the shape alone and does not touch the values: every output is the same k-ordered chain.
// LDS: ((TT - 1) decim + 2 Hmax + 16) samples, TT decim <= 2048, Hmax <= 2047: at most 49 KB in fp64.
// No load goes outside a row or the tables (each has 16 zero rows behind it for the prefetch); x needs element
// alignment only, the complex output the alignment of its (re, im) pair.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>
#include "common.h"

struct isd_tfr_plan {
  int F, G, decim, Hmax;
  int64_t useful_taps, padded_taps;   // sum of n_taps; sum over groups of 8 x the padded K
  int *d_gH, *d_gK, *d_fmap;          // per group: half length, padded K; [8 G] frequency of a slot or -1
  int64_t* d_goff;                    // per group: offset of its table [K / 16 + 1][64 lanes][4]
  int* d_ntaps;                       // [F]
  int64_t* d_poff;                    // [F] offset of a frequency's prefix sums in d_pre
  double* d_pre;                      // per frequency [n_taps + 1][2]: P[k] = sum of taps 0 .. k - 1 (re, im)
  float* d_tab32;
  double* d_tab64;
};

namespace isd {

constexpr int kTfrThreads = 256;
constexpr int kTfrMT = 8;                       // M tiles (of 16 outputs) of an item
constexpr int kTfrChunk = 16 * kTfrMT;          // outputs of an item
constexpr int kTfrMaxTile = 512;                // outputs of a time tile: one chunk per wave
constexpr int kTfrSpan = 2048;                  // TT * decim stays below this (but TT >= 16)
constexpr int kTfrMaxTaps = 4095, kTfrMaxFreqs = 256, kTfrMaxDecim = 128;
constexpr int kTfrKB = 16;                      // k steps of one B fragment load: K is padded to whole blocks
constexpr int kTfrTabTail = kTfrKB;             // zero rows behind a table: the prefetch after the last block

struct TfrGeo {
  int64_t T, T_out, ntile, CF;        // CF = C (modes 2-4: rows of a trial) or 0
  int F, decim, Hmax, TT, nchunk, G, gpw, ntrial;
  // Modes 2, 3: element idx goes to out[idx * ostride + ooff].  (1, 0) from tfr_geometry; only the float entry's
  // mode 4 sets them otherwise (on its own copy), to let modes 2 and 3 write the halves of its pairs.
  int ostride, ooff;
};

// means [rows] (fp64): one wave per row, lanes stride the row, then a fixed butterfly
template <typename S>
__global__ __launch_bounds__(kTfrThreads) void tfr_mean_kernel(const S* __restrict__ x, double* __restrict__ means,
                                                               int64_t rows, int64_t T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const S* p = x + r * T;
    double a = 0.0;
    for (int64_t t = lane; t < T; t += 64) a += (double)p[t];     // never past the row
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
    if (lane == 0) means[r] = a / (double)T;
  }
}

// X: the type of x and out; S: the type the product runs in (X, or double over float samples for the coherence)
template <typename X, typename S, int MODE>
__global__ __launch_bounds__(kTfrThreads) void tfr_cwt_kernel(const X* __restrict__ x, const S* __restrict__ tab,
                                                              const int* __restrict__ gH, const int* __restrict__ gK,
                                                              const int64_t* __restrict__ goff,
                                                              const int* __restrict__ fmap,
                                                              const int* __restrict__ ntaps,
                                                              const int64_t* __restrict__ poff,
                                                              const f64x2* __restrict__ pre,
                                                              const double* __restrict__ means, X* __restrict__ out,
                                                              TfrGeo g) {
  using O = Mfma16<S>;
  using Acc = typename O::Acc;
  using Pair = X __attribute__((ext_vector_type(2)));             // two results side by side, one store
  extern __shared__ __attribute__((aligned(16))) unsigned char tfr_lds[];
  S* xs = reinterpret_cast<S*>(tfr_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, q = lane >> 4, c = col & 1;
  const int64_t row = (int64_t)blockIdx.x / g.ntile;              // a (trial, channel) row, or a channel
  const int64_t o0 = ((int64_t)blockIdx.x % g.ntile) * g.TT;      // first output of the tile
  const int n_out = (int)min((int64_t)g.TT, g.T_out - o0);
  const int64_t s0 = o0 * g.decim - g.Hmax;                       // the sample at xs[0]
  const int nfill = (((n_out + 15) & ~15) - 1) * g.decim + 2 * g.Hmax + kTfrKB;
  const int g0 = blockIdx.y * g.gpw, ng = min(g.gpw, g.G - g0);
  const int nitems = g.nchunk * ng;

  constexpr bool kAvg = MODE >= 2 && MODE <= 4;
  double sp[kTfrMT][2], sr[kTfrMT][2], si[kTfrMT][2];             // kAvg: this wave's one item, summed over trials
  if constexpr (kAvg) {
#pragma unroll
    for (int m = 0; m < kTfrMT; ++m)
#pragma unroll
      for (int e = 0; e < 2; ++e) sp[m][e] = sr[m][e] = si[m][e] = 0.0;
  }

  for (int trial = 0; trial < g.ntrial; ++trial) {
    const int64_t xr = (int64_t)trial * g.CF + row;
    const X* xrow = x + xr * g.T;
    const double mu = means[xr];                                  // the row's mean comes off in fp64 ...
    __syncthreads();                                              // the previous trial's tile has been consumed
    for (int e = tid; e < nfill; e += kTfrThreads) {
      const int64_t s = s0 + e;
      xs[e] = (s >= 0 && s < g.T) ? (S)((double)xrow[s] - mu) : (S)0;
    }
    __syncthreads();
    for (int item = wave; item < nitems; item += 4) {             // kAvg: nitems <= 4, one pass
      const int chunk = item % g.nchunk, grp = g0 + item / g.nchunk;
      const int H = gH[grp], K = gK[grp];
      const int nm = min(kTfrMT, (n_out - chunk * kTfrChunk + 15) >> 4);      // live M tiles; wave-uniform
      if (nm <= 0) continue;                                      // the row's last tile: chunks past its end
      const S* bp = tab + goff[grp] + lane * 4;                   // B[k0 + 4 j + q][col], j = 0 .. 3 side by side
      const S* ap = xs + (chunk * kTfrChunk + col) * g.decim + (g.Hmax - H) + q;   // A[i = col][k0 + q]
      const int mstep = 16 * g.decim;
      Acc acc[kTfrMT];
#pragma unroll
      for (int m = 0; m < kTfrMT; ++m) acc[m] = (Acc)(0);
      Acc bn = *reinterpret_cast<const Acc*>(bp);
      for (int k0 = 0; k0 < K; k0 += kTfrKB) {
        const Acc b = bn;                                         // 32 MFMAs under the next fragment's way from L2
        bn = *reinterpret_cast<const Acc*>(bp + (k0 + kTfrKB) * 16);   // past the last block: the table's zero tail
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int m = 0; m < kTfrMT; ++m)
            if (m < nm) acc[m] = O::mma(ap[k0 + 4 * j + m * mstep], b[j], acc[m]);
      }
      const int f = fmap[grp * 8 + (col >> 1)];
      // ... and goes back on as mu x (the sum of the taps that met a sample of the row): exact in fp64 from the
      // prefix sums P of the taps.  Away from the row's ends that is the whole sum.
      const int h = f >= 0 ? (ntaps[f] - 1) >> 1 : 0;
      const f64x2* P = pre + (f >= 0 ? poff[f] : 0);
      const f64x2 whole = f >= 0 ? P[2 * h + 1] : f64x2{0.0, 0.0};
#pragma unroll
      for (int m = 0; m < kTfrMT; ++m) {
        if (m < nm) {
          // lane c = 0 holds re, c = 1 im of rows r = 0..3: after the exchange c = 0 owns rows 0, 1 and c = 1 rows 2, 3
          const S g0v = __shfl_xor(c ? acc[m][0] : acc[m][2], 1, 64);
          const S g1v = __shfl_xor(c ? acc[m][1] : acc[m][3], 1, 64);
          const S zr[2] = {c ? g0v : acc[m][0], c ? g1v : acc[m][1]};
          const S zi[2] = {c ? acc[m][2] : g0v, c ? acc[m][3] : g1v};
          S re[2], im[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int lo = chunk * kTfrChunk + 16 * m + O::row(q, 2 * c + e);
            const bool ok = f >= 0 && lo < n_out;
            f64x2 sw = whole;
            if (ok) {
              const int64_t td = (o0 + lo) * g.decim;              // < T
              const int64_t after = g.T - 1 - td;
              if (td < h || after < h) {                           // the wavelet hangs over an end of the row
                const f64x2 hi = P[h + (int)min((int64_t)h, td) + 1], lw = P[h - (int)min((int64_t)h, after)];
                sw = hi - lw;
              }
            }
            re[e] = (S)fma(mu, sw[0], (double)zr[e]);
            im[e] = (S)fma(mu, sw[1], (double)zi[e]);
            const S p = fma(re[e], re[e], im[e] * im[e]);
            if constexpr (MODE == 0) {
              if (ok) {
                Pair v;
                v[0] = (X)re[e];
                v[1] = (X)im[e];
                *reinterpret_cast<Pair*>(out + 2 * ((row * g.F + f) * g.T_out + o0 + lo)) = v;
              }
            } else if constexpr (MODE == 1) {
              if (ok) out[(row * g.F + f) * g.T_out + o0 + lo] = (X)p;
            } else if constexpr (MODE == 5) {
              if (ok) out[(row * g.F + f) * g.T_out + o0 + lo] = (X)atan2((double)im[e], (double)re[e]);
            } else if (ok) {
              if constexpr (MODE != 3) sp[m][e] += (double)p;
              if constexpr (MODE != 2) {
                const double rd = (double)re[e], id = (double)im[e];
                const double m2 = fma(rd, rd, id * id);
                if (m2 > 0.0) {                                   // |z| = 0 contributes nothing
                  const double inv = 1.0 / sqrt(m2);
                  sr[m][e] += rd * inv;
                  si[m][e] += id * inv;
                }
              }
            }
          }
        }
      }
    }
  }

  if constexpr (kAvg) {
    const int item = wave;
    if (item < nitems) {
      const int chunk = item % g.nchunk, grp = g0 + item / g.nchunk;
      const int f = fmap[grp * 8 + (col >> 1)];
      const double inv_n = 1.0 / (double)g.ntrial;
#pragma unroll
      for (int m = 0; m < kTfrMT; ++m)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int lo = chunk * kTfrChunk + 16 * m + O::row(q, 2 * c + e);
          if (f >= 0 && lo < n_out) {
            const int64_t idx = (row * g.F + f) * g.T_out + o0 + lo;
            const X pw = (X)(sp[m][e] * inv_n);
            const X itc = (X)(sqrt(fma(sr[m][e], sr[m][e], si[m][e] * si[m][e])) * inv_n);
            if constexpr (MODE == 2) out[idx * g.ostride + g.ooff] = pw;
            if constexpr (MODE == 3) out[idx * g.ostride + g.ooff] = itc;
            if constexpr (MODE == 4) {
              Pair v;
              v[0] = pw;
              v[1] = itc;
              *reinterpret_cast<Pair*>(out + 2 * idx) = v;
            }
          }
        }
    }
  }
}

}  // namespace isd

using namespace isd;

namespace {

int64_t tfr_out_len(const isd_tfr_plan* p, int64_t T) { return T <= 0 ? 0 : (T + p->decim - 1) / p->decim; }

// the tiling: a function of (plan, shape, mode) alone
TfrGeo tfr_geometry(const isd_tfr_plan* p, int64_t n, int64_t C, int64_t T, int mode) {
  TfrGeo g;
  g.T = T;
  g.T_out = tfr_out_len(p, T);
  g.F = p->F;
  g.decim = p->decim;
  g.Hmax = p->Hmax;
  g.G = p->G;
  const bool avg = mode >= 2 && mode <= 4;
  g.CF = avg ? C : 0;
  g.ntrial = avg ? (int)n : 1;
  int TT = std::max(16, std::min(kTfrMaxTile, kTfrSpan / p->decim / 16 * 16));
  TT = (int)std::min<int64_t>(TT, cdiv(std::max<int64_t>(g.T_out, 1), 16) * 16);
  if (avg)                                                         // few workgroups: shorter tiles, down to one chunk
    while (TT > kTfrChunk && C * cdiv(g.T_out, TT) * cdiv(g.G, std::max(1, 4 / (int)cdiv(TT, kTfrChunk))) < 512)
      TT = (int)cdiv(TT / 2, 16) * 16;
  g.TT = TT;
  g.nchunk = (int)cdiv(TT, kTfrChunk);
  g.ntile = cdiv(std::max<int64_t>(g.T_out, 1), TT);
  g.gpw = avg ? std::max(1, 4 / g.nchunk) : g.G;
  g.ostride = 1;
  g.ooff = 0;
  return g;
}

template <typename X, typename S, int MODE>
int tfr_launch_mode(const isd_tfr_plan* p, const X* x, X* out, const double* means, const TfrGeo& g, int64_t rows,
                    hipStream_t st) {
  const S* tab = sizeof(S) == 8 ? (const S*)p->d_tab64 : (const S*)p->d_tab32;
  const size_t lds = ((size_t)(g.TT - 1) * g.decim + 2 * (size_t)g.Hmax + kTfrKB) * sizeof(S);
  const dim3 grid((unsigned)(rows * g.ntile), (unsigned)cdiv(g.G, g.gpw));
  return launch_lds(tfr_cwt_kernel<X, S, MODE>, grid, dim3(kTfrThreads), lds, st, x, tab, (const int*)p->d_gH,
                    (const int*)p->d_gK, (const int64_t*)p->d_goff, (const int*)p->d_fmap, (const int*)p->d_ntaps,
                    (const int64_t*)p->d_poff, (const f64x2*)p->d_pre, means, out, g);
}

template <typename S>
int tfr_launch(const isd_tfr_plan* p, const S* x, void* out, int64_t n, int64_t C, int64_t T, int mode, void* work,
               void* stream, const char* who) {
  ISD_CHECK_ARG(p, "%s: null plan", who);
  ISD_CHECK_ARG(n >= 0 && C >= 0 && T >= 0, "%s: n=%lld, C=%lld, T=%lld", who, (long long)n, (long long)C,
                (long long)T);
  ISD_CHECK_ARG(mode >= 0 && mode <= 5, "%s: mode=%d (0 complex, 1 power, 2 avg_power, 3 itc, 4 both, 5 phase)", who,
                mode);
  const bool avg = mode >= 2 && mode <= 4;
  ISD_CHECK_ARG(!(avg && n == 0), "%s: an average over n=0 trials", who);
  if (n == 0 || C == 0 || T == 0) return ISD_OK;
  ISD_CHECK_ARG(x && out && work, "%s: null argument", who);
  ISD_CHECK_SUPPORTED(n <= 2147483647LL && C <= 2147483647LL, "%s: n=%lld, C=%lld (at most 2^31 - 1 each)", who,
                      (long long)n, (long long)C);
  ISD_CHECK_SUPPORTED(T <= (1LL << 40), "%s: T=%lld (at most 2^40)", who, (long long)T);
  TfrGeo g = tfr_geometry(p, n, C, T, mode);
  const int64_t rows = avg ? C : n * C;
  ISD_CHECK_SUPPORTED(rows <= 2147483647LL / g.ntile, "%s: %lld rows x %lld time tiles (at most 2^31 - 1 workgroups)",
                      who, (long long)rows, (long long)g.ntile);
  hipStream_t st = (hipStream_t)stream;
  S* o = static_cast<S*>(out);
  double* means = static_cast<double*>(work);                     // [n C]
  hipLaunchKernelGGL((tfr_mean_kernel<S>), dim3((unsigned)std::min<int64_t>(cdiv(n * C, 4), 256 * 16)),
                     dim3(kTfrThreads), 0, st, x, means, n * C, T);
  ISD_LAUNCH_CHECK();
  // The phase, and the coherence as a mean of z / |z|, depend on the RELATIVE error of a sample: an error of 1e-7 of
  // the row's largest |z| turns the phase of a sample at 1e-3 of it by 1e-4.  Over float samples their product
  // therefore runs in fp64 (the samples widened on their way to LDS), and mode 4 is the launches of modes 2 and 3
  // writing the two halves of the pairs: the same bits as each.
  switch (mode) {
    case 0: return tfr_launch_mode<S, S, 0>(p, x, o, means, g, rows, st);
    case 1: return tfr_launch_mode<S, S, 1>(p, x, o, means, g, rows, st);
    case 2: return tfr_launch_mode<S, S, 2>(p, x, o, means, g, rows, st);
    case 3: return tfr_launch_mode<S, double, 3>(p, x, o, means, g, rows, st);
    case 5: return tfr_launch_mode<S, double, 5>(p, x, o, means, g, rows, st);
    default:
      if constexpr (sizeof(S) == 8) return tfr_launch_mode<S, S, 4>(p, x, o, means, g, rows, st);
      g.ostride = 2;
      if (int rc = tfr_launch_mode<S, S, 2>(p, x, o, means, g, rows, st)) return rc;
      g.ooff = 1;
      return tfr_launch_mode<S, double, 3>(p, x, o, means, g, rows, st);
  }
}

}  // namespace

extern "C" int isd_tfr_plan_create(isd_tfr_plan** out, int n_freqs, const int* n_taps, const double* taps, int decim) {
  ISD_CHECK_ARG(out && n_taps && taps, "isd_tfr_plan_create: null argument");
  ISD_CHECK_SUPPORTED(n_freqs >= 1 && n_freqs <= kTfrMaxFreqs,
                      "isd_tfr_plan_create: n_freqs=%d (need 1 <= n_freqs <= %d)", n_freqs, kTfrMaxFreqs);
  ISD_CHECK_SUPPORTED(decim >= 1 && decim <= kTfrMaxDecim, "isd_tfr_plan_create: decim=%d (need 1 <= decim <= %d)",
                      decim, kTfrMaxDecim);
  int64_t total = 0;
  for (int f = 0; f < n_freqs; ++f) {
    ISD_CHECK_SUPPORTED(n_taps[f] >= 1 && n_taps[f] <= kTfrMaxTaps && (n_taps[f] & 1),
                        "isd_tfr_plan_create: n_taps[%d]=%d (need an odd count, 1 <= n_taps <= %d)", f, n_taps[f],
                        kTfrMaxTaps);
    total += n_taps[f];
  }
  for (int64_t e = 0; e < 2 * total; ++e)
    ISD_CHECK_SUPPORTED(std::isfinite(taps[e]), "isd_tfr_plan_create: taps[%lld] is not finite", (long long)e);
  if (int rc = require_device("isd_tfr_plan_create")) return rc;
  std::vector<int64_t> start(n_freqs);                            // offset of a frequency's taps, in complex elements
  for (int64_t f = 0, s = 0; f < n_freqs; s += n_taps[f], ++f) start[f] = s;
  std::vector<int> order(n_freqs);                                // longest first; equal lengths keep their order
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_taps[a] > n_taps[b]; });

  isd_tfr_plan* p = new isd_tfr_plan();
  p->F = n_freqs;
  p->decim = decim;
  p->G = (int)cdiv(n_freqs, 8);
  p->Hmax = (n_taps[order[0]] - 1) / 2;
  p->useful_taps = total;
  std::vector<int> gH(p->G), gK(p->G), fmap((size_t)8 * p->G, -1);
  std::vector<int64_t> goff(p->G);
  int64_t size = 0;
  for (int gi = 0; gi < p->G; ++gi) {
    gH[gi] = (n_taps[order[gi * 8]] - 1) / 2;
    gK[gi] = (int)cdiv(2 * gH[gi] + 1, kTfrKB) * kTfrKB;
    goff[gi] = size;
    size += (int64_t)(gK[gi] + kTfrTabTail) * 16;
    p->padded_taps += (int64_t)8 * gK[gi];
  }
  std::vector<double> t64((size_t)size, 0.0);
  for (int gi = 0; gi < p->G; ++gi)
    for (int s = 0; s < 8 && gi * 8 + s < n_freqs; ++s) {
      const int f = order[gi * 8 + s], h = (n_taps[f] - 1) / 2, H = gH[gi];
      fmap[(size_t)gi * 8 + s] = f;
      const double* w = taps + 2 * start[f];
      for (int kk = H - h; kk <= H + h; ++kk) {                   // B[kk] = w[h + H - kk]: sample t decim + (kk - H)
        const int k = h + H - kk;
        // block kk / 16 holds, per lane (q = kk % 4, column), the four rows kk % 16 / 4 = 0 .. 3 side by side
        const size_t at = (size_t)goff[gi] + (((size_t)(kk / 16) * 64 + (kk % 4) * 16 + 2 * s) * 4 + (kk % 16) / 4);
        t64[at] = w[2 * k];
        t64[at + 4] = w[2 * k + 1];
      }
    }
  std::vector<float> t32(t64.begin(), t64.end());
  std::vector<int> nt(n_taps, n_taps + n_freqs);
  std::vector<int64_t> poff(n_freqs);
  std::vector<double> pre((size_t)2 * (total + n_freqs));
  for (int64_t f = 0, o = 0; f < n_freqs; o += n_taps[f] + 1, ++f) {
    poff[f] = o;
    double sr = 0.0, si = 0.0;
    for (int k = 0; k <= n_taps[f]; ++k) {
      pre[2 * (o + k)] = sr;
      pre[2 * (o + k) + 1] = si;
      if (k < n_taps[f]) {
        sr += taps[2 * (start[f] + k)];
        si += taps[2 * (start[f] + k) + 1];
      }
    }
  }
  hipError_t e = upload(&p->d_tab64, t64);
  if (e == hipSuccess) e = upload(&p->d_ntaps, nt);
  if (e == hipSuccess) e = upload(&p->d_poff, poff);
  if (e == hipSuccess) e = upload(&p->d_pre, pre);
  if (e == hipSuccess) e = upload(&p->d_tab32, t32);
  if (e == hipSuccess) e = upload(&p->d_gH, gH);
  if (e == hipSuccess) e = upload(&p->d_gK, gK);
  if (e == hipSuccess) e = upload(&p->d_fmap, fmap);
  if (e == hipSuccess) e = upload(&p->d_goff, goff);
  if (e != hipSuccess) {
    set_error("isd_tfr_plan_create: %s", hipGetErrorString(e));
    isd_tfr_plan_destroy(p);
    return ISD_ERR_HIP;
  }
  *out = p;
  return ISD_OK;
}

extern "C" int isd_tfr_plan_destroy(isd_tfr_plan* p) {
  if (!p) return ISD_OK;
  if (p->d_tab64) (void)hipFree(p->d_tab64);
  if (p->d_tab32) (void)hipFree(p->d_tab32);
  if (p->d_gH) (void)hipFree(p->d_gH);
  if (p->d_gK) (void)hipFree(p->d_gK);
  if (p->d_fmap) (void)hipFree(p->d_fmap);
  if (p->d_goff) (void)hipFree(p->d_goff);
  if (p->d_ntaps) (void)hipFree(p->d_ntaps);
  if (p->d_poff) (void)hipFree(p->d_poff);
  if (p->d_pre) (void)hipFree(p->d_pre);
  delete p;
  return ISD_OK;
}

extern "C" int64_t isd_tfr_plan_out_len(const isd_tfr_plan* p, int64_t T) {
  return p ? tfr_out_len(p, T) : (int64_t)ISD_ERR_INVALID;
}

extern "C" int64_t isd_tfr_plan_padded_taps(const isd_tfr_plan* p) {
  return p ? p->padded_taps : (int64_t)ISD_ERR_INVALID;
}

extern "C" int64_t isd_tfr_work_bytes(const isd_tfr_plan* p, int64_t n, int64_t C, int64_t T, int mode, int is_f64) {
  if (!p || n < 0 || C < 0 || T < 0 || mode < 0 || mode > 5) {
    set_error("isd_tfr_work_bytes: null plan, n=%lld, C=%lld, T=%lld or mode=%d", (long long)n, (long long)C,
              (long long)T, mode);
    return ISD_ERR_INVALID;
  }
  (void)is_f64;
  return std::max<int64_t>(256, (n * C * 8 + 255) / 256 * 256);   // the rows' means (fp64); never zero bytes
}

extern "C" int isd_tfr_cwt_f32(const isd_tfr_plan* plan, const float* x, void* out, int64_t n, int64_t C, int64_t T,
                               int mode, void* work, void* stream) {
  return tfr_launch<float>(plan, x, out, n, C, T, mode, work, stream, "isd_tfr_cwt_f32");
}

extern "C" int isd_tfr_cwt_f64(const isd_tfr_plan* plan, const double* x, void* out, int64_t n, int64_t C, int64_t T,
                               int mode, void* work, void* stream) {
  return tfr_launch<double>(plan, x, out, n, C, T, mode, work, stream, "isd_tfr_cwt_f64");
}
