// Welch power spectral density: the data-sized step of isd_amd.psd_array_welch, the counterpart of
//   raw.compute_psd(method='welch') -> mne.time_frequency.psd_array_welch          (scripts/artifact_analysis.py:45)
// Segment bookkeeping, the window and the argument checks are host work (isd_amd/psd.py: welch_design).
//
// The segments that occur are short (n_fft 256 at 250 Hz, up to 2048 at 1024 Hz), the result is tiny and the kept
// band is often a fraction of the spectrum, so the transform is a dense product on the matrix cores and only the kept
// bins are computed:   re[row][k] = sum_t (x[row][s step + t] - mu) Wc[k][t],   Wc[k][t] = w[t] cos(2 pi k t / n_fft),
// im likewise with Ws, power = re^2 + im^2.  The plan owns Wc and Ws, built on the host in fp64 from one period of
// cos / sin with the angle reduced in integers ((k t) mod n_fft), zero-padded to whole tiles in k and t.
//
//   psd_mean_kernel    one wave per (row, segment): the segment mean in fp64 whatever the input type (a float mean of
//                      samples near 200 would leave a DC residue of 1e-5 x sum(w) in bins 0 and 1), written to `work`.
//   psd_welch_kernel   blockIdx.x owns 64 data rows, blockIdx.y 64 bins, blockIdx.z a range of segments.  The M side
//                      of a tile is data rows at one segment index, the N side bins; wave v owns rows 16 v .. 16 v + 15
//                      of the 64 and the workgroup's 16-bin tiles that hold a kept bin (up to four), with one
//                      accumulator for cos and one for sin per tile: the two land in the same lane and register, so
//                      re^2 + im^2 needs no shuffle.  The workgroup walks its segments in order; per segment it stages
//                      chunks of KC samples (rows minus their mean, zero past n_per_seg and past the last row) and
//                      the same chunk of its cos and sin table rows through LDS, the next chunk on its way to
//                      registers while the current one is multiplied.  After the last chunk the power is added to a
//                      register accumulator (or, per_segment, stored): the mean over segments is a sum in segment
//                      order inside one thread.  A workgroup's time goes with its live bin tiles: K = 129 costs nine
//                      16-bin tiles, not twelve.
//   psd_reduce_kernel  with few row tiles the segment range is split over blockIdx.z; each z leaves its sums in `work`
//                      and this kernel adds them in z order and scales.  The split is a function of the shape alone:
//                      no atomics, the same bits on every run.
//
// LDS per workgroup: three tiles [64][KC + 4]: float KC = 64: 3 x 64 x 68 x 4 = 51 KB; double KC = 32: 3 x 64 x 36 x 8
// = 54 KB.  Two workgroups per CU (of 160 KB), two waves per SIMD; the table slice of a workgroup (64 bins x 2 x
// n_per_seg: 128 KB float / 256 KB double at n_fft 256) does not fit beside them and is re-read per segment from L2,
// one chunk of it per chunk of samples.  Operand order inside a block of 4 VEC steps as in ica.hip: lane group g
// takes k = VEC g + s in MFMA s, so both operands are one 16-byte LDS read per VEC MFMAs.
// No load goes past a row's last used sample, past the last row, or past the (padded) table; x needs element
// alignment only (every lane loads one element, a wave 64 consecutive ones).
#include <algorithm>
#include <cmath>
#include <vector>
#include "psd_common.h"

namespace isd {

// out: per_segment ? [rows][K][S] : (partial ? [gridDim.z][rows][K] unscaled sums : [rows][K] the mean)
template <typename S>
__global__ __launch_bounds__(kPsdThreads, 2) void psd_welch_kernel(const S* __restrict__ x, const S* __restrict__ tab,
                                                               const S* __restrict__ scale,
                                                               const double* __restrict__ means, S* __restrict__ out,
                                                               int64_t rows, int64_t T, int64_t S_, int seg_per_z,
                                                               int nps, int step, int np, int K, int Kp,
                                                               int per_segment, int partial) {
  using O = PsdOps<S>;
  using Acc = typename O::Acc;
  using Vec = typename O::Vec;
  constexpr int KC = O::KC, LD = O::LD, VEC = O::VEC, PF = kPsdRows * KC / kPsdThreads;
  constexpr int NT = kPsdBins / 16;
  __shared__ __attribute__((aligned(16))) S xs[kPsdRows * LD];  // [64 rows][KC] the samples
  __shared__ __attribute__((aligned(16))) S cs[kPsdBins * LD];  // [64 bins][KC] w cos
  __shared__ __attribute__((aligned(16))) S ss[kPsdBins * LD];  // [64 bins][KC] w sin
  __shared__ double mus[kPsdRows];                               // the rows' means of the current segment
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kPsdRows;
  const int nrow = (int)min((int64_t)kPsdRows, rows - row0);
  const int bin0 = blockIdx.y * kPsdBins;
  const int nb = min(NT, (K - bin0 + 15) >> 4);                 // 16-bin tiles of this workgroup that hold a kept bin
  const int64_t s_begin = (int64_t)blockIdx.z * seg_per_z;
  const int nseg = (int)min((int64_t)seg_per_z, S_ - s_begin);  // >= 1 by the choice of gridDim.z
  const int nchunk = np / KC;
  const bool live = wave * 16 < nrow;                           // wave-uniform: the wave's 16 rows hold data
  const S* xr = x + row0 * T;
  const S* tc = tab + (int64_t)bin0 * np;                       // rows bin0 .. bin0 + 63 exist: Kp is a multiple of 64
  const S* ts = tc + (int64_t)Kp * np;

  Acc re[NT], im[NT], pw[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) re[b] = im[b] = pw[b] = (Acc)(0);

  S px[PF], pc[PF], ps[PF];
  int c = 0;
  int64_t s = s_begin;
  const double* mp = (means != nullptr && tid < nrow) ? means + (row0 + tid) * S_ : nullptr;   // thread tid: row tid
  double mu = mp ? mp[s] : 0.0;
  psd_fetch_tile<S, PF>(px, xr + s * step, T, nrow, nps, tid);
  psd_fetch_tile<S, PF>(pc, tc, np, nb * 16, KC, tid);           // table rows of dead tiles are not fetched
  psd_fetch_tile<S, PF>(ps, ts, np, nb * 16, KC, tid);
  const int nunit = nseg * nchunk;
  for (int u = 0; u < nunit; ++u) {
    __syncthreads();                                             // the previous chunk has been consumed
    if (c == 0) {                                                // workgroup-uniform: a new segment
      if (tid < kPsdRows) mus[tid] = mu;
      __syncthreads();
    }
    psd_store_data<S, PF>(xs, px, mus, nrow, nps - c * KC, tid);
    psd_store_tile<S, PF>(cs, pc, tid);
    psd_store_tile<S, PF>(ss, ps, tid);
    const bool last = c == nchunk - 1;
    const int c1 = last ? 0 : c + 1;
    const int64_t s1 = last ? s + 1 : s;
    if (u + 1 < nunit) {                                         // workgroup-uniform; in flight during the MFMAs
      if (last) mu = mp ? mp[s1] : 0.0;
      psd_fetch_tile<S, PF>(px, xr + s1 * step + c1 * KC, T, nrow, nps - c1 * KC, tid);
      psd_fetch_tile<S, PF>(pc, tc + c1 * KC, np, nb * 16, KC, tid);
      psd_fetch_tile<S, PF>(ps, ts + c1 * KC, np, nb * 16, KC, tid);
    }
    __syncthreads();
    if (live) {
      const S* pa = xs + (wave * 16 + (lane & 15)) * LD + VEC * (lane >> 4);    // A[row][k]: VEC samples of a row
      const S* pbc = cs + (lane & 15) * LD + VEC * (lane >> 4);                 // B[k][bin]: of the bin's table row
      const S* pbs = ss + (lane & 15) * LD + VEC * (lane >> 4);
      if constexpr (sizeof(S) == 4) {
        switch (nb) {                                            // workgroup-uniform
          case 1: psd_mma_chunk<S, 1>(re, im, pa, pbc, pbs); break;
          case 2: psd_mma_chunk<S, 2>(re, im, pa, pbc, pbs); break;
          case 3: psd_mma_chunk<S, 3>(re, im, pa, pbc, pbs); break;
          default: psd_mma_chunk<S, 4>(re, im, pa, pbc, pbs); break;
        }
      } else {
#pragma unroll                                                   // double: the tile count at run time, a tile at a time
        for (int k = 0; k < KC; k += 4 * VEC) {                  // (the straight-line form spills there, and the longer
          const Vec va = *reinterpret_cast<const Vec*>(pa + k);  // fp64 MFMAs cover the LDS reads of the next tile)
#pragma unroll
          for (int b = 0; b < NT; ++b) {
            if (b < nb) {                                        // workgroup-uniform
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
      if (last) {                                                // the segment is complete
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          const int bin = bin0 + b * 16 + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const S p = re[b][r] * re[b][r] + im[b][r] * im[b][r];
            if (per_segment) {
              const int64_t row = row0 + wave * 16 + O::lane_row(lane, r);
              if (row < rows && bin < K) out[(row * K + bin) * S_ + s] = p * scale[bin];
            } else {
              pw[b][r] += p;                                     // segment order, one thread: no reduction
            }
          }
          re[b] = im[b] = (Acc)(0);
        }
      }
    }
    c = c1;
    s = s1;
  }

  if (live && !per_segment) {
    S* o = partial ? out + (int64_t)blockIdx.z * rows * K : out;
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const int bin = bin0 + b * 16 + (lane & 15);
      const S sc = (partial || bin >= K) ? (S)1 : scale[bin] / (S)S_;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + wave * 16 + O::lane_row(lane, r);
        if (row < rows && bin < K) o[row * K + bin] = pw[b][r] * sc;
      }
    }
  }
}

template <typename S>
__global__ __launch_bounds__(256) void psd_reduce_kernel(const S* __restrict__ part, const S* __restrict__ scale,
                                                         S* __restrict__ out, int64_t E, int K, int Z, int64_t S_) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  S a = (S)0;
  for (int z = 0; z < Z; ++z) a += part[(int64_t)z * E + e];    // z order = segment order
  out[e] = a * (scale[e % K] / (S)S_);
}

}  // namespace isd

using namespace isd;

namespace {

struct PsdSplit {
  int64_t row_tiles;
  int bin_tiles, Z, seg_per_z;
};

// a function of the shape alone
PsdSplit psd_split(const isd_psd_plan* p, int64_t rows, int64_t S_) {
  PsdSplit sp;
  sp.row_tiles = cdiv(rows, kPsdRows);
  sp.bin_tiles = (int)cdiv(p->K, kPsdBins);
  const int64_t base = sp.row_tiles * sp.bin_tiles;
  int64_t Z = base >= kPsdSplitBelow ? 1 : std::min<int64_t>(S_, cdiv(kPsdSplitTarget, base));
  const int64_t per = cdiv(S_, Z);
  sp.seg_per_z = (int)per;
  sp.Z = (int)cdiv(S_, per);                                     // no empty z
  return sp;
}

// The workspace in bytes: the fp64 segment means, then (when the segments are split over z) each z's partial spectra.
struct PsdWs {
  int64_t means, part, slack, end;
  PsdSplit sp;
};
PsdWs psd_layout(const isd_psd_plan* p, int64_t rows, int64_t S_, int64_t el) {
  PsdWs l = {};
  WorkCarver c;
  if (rows == 0 || S_ == 0) {
    l.slack = c.take(256);                                       // never a zero-byte buffer
  } else {
    l.sp = psd_split(p, rows, S_);
    l.means = c.take(rows * S_ * 8, 256);
    l.part = c.take(l.sp.Z > 1 ? (int64_t)l.sp.Z * rows * p->K * el : 0, 256);
    l.slack = c.take(l.sp.Z > 1 ? 0 : 256, 256);                 // whole lines; a line of slack where there is no `part`
  }
  l.end = c.end;
  return l;
}

template <typename S>
int psd_launch(const isd_psd_plan* p, const S* x, S* out, int64_t rows, int64_t T, int per_segment, void* work,
               void* stream, const char* who) {
  ISD_CHECK_ARG(p, "%s: null plan", who);
  ISD_CHECK_ARG(rows >= 0, "%s: rows=%lld", who, (long long)rows);
  if (rows == 0) return ISD_OK;
  ISD_CHECK_SUPPORTED(T >= p->n_per_seg, "%s: T=%lld is shorter than n_per_seg=%d", who, (long long)T, p->n_per_seg);
  const int64_t S_ = psd_segments(p, T);
  ISD_CHECK_SUPPORTED(S_ <= 2147483647LL, "%s: %lld segments (at most 2^31 - 1)", who, (long long)S_);
  ISD_CHECK_ARG(x && out && work, "%s: null argument", who);
  const PsdWs l = psd_layout(p, rows, S_, sizeof(S));
  const PsdSplit& sp = l.sp;
  ISD_CHECK_SUPPORTED(sp.row_tiles <= 2147483647LL, "%s: rows=%lld", who, (long long)rows);
  hipStream_t st = (hipStream_t)stream;
  const bool f64 = sizeof(S) == 8;
  const S* tab = f64 ? (const S*)p->d_tab64 : (const S*)p->d_tab32;
  const S* scale = f64 ? (const S*)p->d_scale64 : (const S*)p->d_scale32;
  const int np = f64 ? p->np64 : p->np32;
  double* means = nullptr;
  if (p->remove_dc) {
    means = reinterpret_cast<double*>(static_cast<char*>(work) + l.means);
    const int64_t units = rows * S_;
    const unsigned g = (unsigned)std::min<int64_t>(cdiv(units, 4), 256 * 16);
    hipLaunchKernelGGL((psd_mean_kernel<S>), dim3(g), dim3(kPsdThreads), 0, st, x, means, units, S_, T, p->n_per_seg,
                       p->step);
    ISD_LAUNCH_CHECK();
  }
  const int partial = !per_segment && sp.Z > 1;
  S* part = reinterpret_cast<S*>(static_cast<char*>(work) + l.part);
  const dim3 grid((unsigned)sp.row_tiles, (unsigned)sp.bin_tiles, (unsigned)sp.Z);
  hipLaunchKernelGGL((psd_welch_kernel<S>), grid, dim3(kPsdThreads), 0, st, x, tab, scale, (const double*)means,
                     partial ? part : out, rows, T, S_, sp.seg_per_z, p->n_per_seg, p->step, np, p->K, p->Kp,
                     per_segment, partial);
  ISD_LAUNCH_CHECK();
  if (partial) {
    const int64_t E = rows * p->K;
    hipLaunchKernelGGL((psd_reduce_kernel<S>), dim3((unsigned)cdiv(E, 256)), dim3(256), 0, st, (const S*)part, scale,
                       out, E, p->K, sp.Z, S_);
    ISD_LAUNCH_CHECK();
  }
  return ISD_OK;
}

}  // namespace

extern "C" int isd_psd_plan_create(isd_psd_plan** out, int n_fft, int n_per_seg, int n_overlap, int k_lo, int k_hi,
                                   const double* window, double sfreq, int remove_dc) {
  ISD_CHECK_ARG(out && window, "isd_psd_plan_create: null argument");
  ISD_CHECK_SUPPORTED(n_fft >= 2 && n_fft <= kPsdMaxFft, "isd_psd_plan_create: n_fft=%d (need 2 <= n_fft <= %d)", n_fft,
                      kPsdMaxFft);
  ISD_CHECK_SUPPORTED(n_per_seg >= 1 && n_per_seg <= n_fft,
                      "isd_psd_plan_create: n_per_seg=%d (need 1 <= n_per_seg <= n_fft=%d)", n_per_seg, n_fft);
  ISD_CHECK_SUPPORTED(n_overlap >= 0 && n_overlap < n_per_seg,
                      "isd_psd_plan_create: n_overlap=%d (need 0 <= n_overlap < n_per_seg=%d)", n_overlap, n_per_seg);
  ISD_CHECK_SUPPORTED(k_lo >= 0 && k_lo <= k_hi && k_hi <= n_fft / 2,
                      "isd_psd_plan_create: bins %d..%d (need 0 <= k_lo <= k_hi <= n_fft/2 = %d)", k_lo, k_hi,
                      n_fft / 2);
  double sw2 = 0.0;
  for (int t = 0; t < n_per_seg; ++t) {
    ISD_CHECK_SUPPORTED(std::isfinite(window[t]), "isd_psd_plan_create: window[%d] is not finite", t);
    sw2 += window[t] * window[t];
  }
  ISD_CHECK_SUPPORTED(std::isfinite(sfreq) && sfreq > 0 && sw2 > 0,
                      "isd_psd_plan_create: sfreq=%g, sum of squared taps %g (both must be positive)", sfreq, sw2);
  if (int rc = require_device("isd_psd_plan_create")) return rc;
  isd_psd_plan* p = new isd_psd_plan();
  p->n_fft = n_fft;
  p->n_per_seg = n_per_seg;
  p->n_overlap = n_overlap;
  p->step = n_per_seg - n_overlap;
  p->k_lo = k_lo;
  p->k_hi = k_hi;
  p->K = k_hi - k_lo + 1;
  p->Kp = (int)cdiv(p->K, kPsdBins) * kPsdBins;
  p->remove_dc = remove_dc != 0;
  p->np32 = (int)cdiv(n_per_seg, PsdOps<float>::KC) * PsdOps<float>::KC;
  p->np64 = (int)cdiv(n_per_seg, PsdOps<double>::KC) * PsdOps<double>::KC;

  const double two_pi = 6.283185307179586476925286766559;
  std::vector<double> c1(n_fft), s1(n_fft);                      // one period; the angle is reduced in integers
  for (int m = 0; m < n_fft; ++m) {
    c1[m] = std::cos(two_pi * m / n_fft);
    s1[m] = std::sin(two_pi * m / n_fft);
  }
  std::vector<double> t64((size_t)2 * p->Kp * p->np64, 0.0), sc64(p->K);
  std::vector<float> t32((size_t)2 * p->Kp * p->np32, 0.f), sc32(p->K);
  for (int i = 0; i < p->K; ++i) {
    const int k = k_lo + i;
    const double ck = (k == 0 || 2 * k == n_fft) ? 1.0 : 2.0;
    sc64[i] = ck / (sfreq * sw2);
    sc32[i] = (float)sc64[i];
    for (int t = 0; t < n_per_seg; ++t) {
      const int m = (int)(((int64_t)k * t) % n_fft);
      const double wc = window[t] * c1[m], ws = window[t] * s1[m];
      t64[(size_t)i * p->np64 + t] = wc;
      t64[((size_t)p->Kp + i) * p->np64 + t] = ws;
      t32[(size_t)i * p->np32 + t] = (float)wc;
      t32[((size_t)p->Kp + i) * p->np32 + t] = (float)ws;
    }
  }
  hipError_t e = upload(&p->d_tab64, t64);
  if (e == hipSuccess) e = upload(&p->d_tab32, t32);
  if (e == hipSuccess) e = upload(&p->d_scale64, sc64);
  if (e == hipSuccess) e = upload(&p->d_scale32, sc32);
  if (e != hipSuccess) {
    set_error("isd_psd_plan_create: %s", hipGetErrorString(e));
    isd_psd_plan_destroy(p);
    return ISD_ERR_HIP;
  }
  *out = p;
  return ISD_OK;
}

extern "C" int isd_psd_plan_destroy(isd_psd_plan* p) {
  if (!p) return ISD_OK;
  if (p->d_tab64) (void)hipFree(p->d_tab64);
  if (p->d_tab32) (void)hipFree(p->d_tab32);
  if (p->d_scale64) (void)hipFree(p->d_scale64);
  if (p->d_scale32) (void)hipFree(p->d_scale32);
  delete p;
  return ISD_OK;
}

extern "C" int isd_psd_plan_bins(const isd_psd_plan* p) { return p ? p->K : ISD_ERR_INVALID; }

extern "C" int64_t isd_psd_plan_segments(const isd_psd_plan* p, int64_t T) {
  return p ? psd_segments(p, T) : (int64_t)ISD_ERR_INVALID;
}

extern "C" int64_t isd_psd_work_bytes(const isd_psd_plan* p, int64_t rows, int64_t T, int is_f64) {
  if (!p || rows < 0) {
    set_error("isd_psd_work_bytes: null plan or rows=%lld", (long long)rows);
    return ISD_ERR_INVALID;
  }
  return psd_layout(p, rows, psd_segments(p, T), is_f64 ? 8 : 4).end;
}

extern "C" int isd_psd_welch_f32(const isd_psd_plan* plan, const float* x, float* out, int64_t rows, int64_t T,
                                 int per_segment, void* work, void* stream) {
  return psd_launch<float>(plan, x, out, rows, T, per_segment, work, stream, "isd_psd_welch_f32");
}

extern "C" int isd_psd_welch_f64(const isd_psd_plan* plan, const double* x, double* out, int64_t rows, int64_t T,
                                 int per_segment, void* work, void* stream) {
  return psd_launch<double>(plan, x, out, rows, T, per_segment, work, stream, "isd_psd_welch_f64");
}
