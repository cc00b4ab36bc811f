// Phase-amplitude coupling with circular-shift surrogates: the data-sized step of isd_amd.phase_amplitude_coupling.
// Per row (trial, channel): pha [P][T] phases in [-pi, pi], amp [A][T] amplitudes >= 0, shifts [1 + S] with
// shifts[0] = 0.  The phase bin is b[t] = min(B - 1, max(0, floor((double(pha[t]) + pi) c))), c = B / (2 pi) formed by
// the caller, evaluated in fp64 in both precisions: one add, one multiply, floor.  Per (p, q, shift s), with
// a^s[t] = a_q[(t + s) mod T] and n_j samples in bin j:
//
//   mvl = |sum_t a^s[t] e^{i pha_p[t]}| / T
//   m_j = (sum_{t: b[t] = j} a^s[t]) / n_j (0 for an empty bin),   P_j = m_j / sum_k m_k
//   mi  = 1 + sum_{j: P_j > 0} P_j log P_j / log B,   hr = (max_j m_j - min_j m_j) / max_j m_j
//
//   pac_rank_by_key    one wave ranks n items by (key, index), key < 64: per group of 64 items one ballot and a
//                      popcount prefix per key present, lane j keeping the count of key j.  No atomics; the ranking is
//                      stable and repeatable.
//   pac_sort_kernel    one wave per (row, p): the samples ranked by phase bin.  It leaves in the workspace, in
//                      bin-sorted order, (cos pha, sin pha) (sincos in fp64, rounded to S) and t, and the B + 1
//                      segment offsets.  A row of records is padded to a multiple of kPacBlock.
//   pac_order_kernel   one wave: the shifts ranked by shift mod 32, for the lane assignment below.
//   pac_main_kernel    one workgroup per (row, q), its waves over p.  The amplitude row is staged once in LDS at
//                      doubled length, so (t + s) mod T is a plain add.  Each LANE OWNS ONE SHIFT; the 1 + S shifts
//                      run in groups of 64.  All lanes walk the same sorted records, which are therefore loaded
//                      through the scalar unit kPacBlock at a time, the next block in flight; a lane gathers
//                      a[t + s_lane] from LDS and accumulates re += a cos, im += a sin and the running bin sum, which
//                      is closed at each segment boundary (wave-uniform): one address, one LDS read, two fma and an
//                      add per (pair, shift, sample).  The gather is the only LDS traffic of the loop, and lanes l, l'
//                      of one 32-lane half collide on a bank at EVERY sample iff s_l = s_l' mod 32 (4-byte banks mod
//                      32 for float, 8-byte slots mod 32 for double).  So shifts go to lanes by rank r in
//                      pac_order_kernel's order: half-wave r mod H, lane r / H of it (H half-waves in all), which
//                      spreads each residue class evenly over the half-waves; with 200 random shifts most halves see
//                      no residue twice, where the given order would see one about 3.5 times.
//                      mi and hr are invariant to the amplitude's scale, so a closed bin mean is divided by the row's
//                      mean amplitude first and sum_j u_j and sum_j u_j log u_j accumulate in fp64 at the size of 1:
//                      mi = 1 + (sum u log u / sum u - log sum u) / log B is then free of the cancellation that the
//                      log of microvolt amplitudes would bring.  The epilogue forms the three measures per lane,
//                      rounds them to S (what `surr` receives), and reduces over the shifts in a fixed order: the mean
//                      and the population std in fp64 about one surrogate's value as pivot, and the count of
//                      surrogates >= the estimate.
//
// Every sum runs in a fixed order and there are no atomics: the result is bitwise repeatable.  No load goes outside
// pha, amp, shifts or the workspace (a shift is clamped to [0, T - 1], shift 0 is taken as 0 whatever shifts[0]
// holds, lanes without a shift walk shift 0 and store nothing, and the records past T of a padded row are loaded
// but never used); no store outside the workspace, out or surr.  With S = 0 the surrogate mean and std are NaN (0 / 0)
// and n_ge is 0; an all-zero amplitude row gives NaN for mi and hr (0 / 0), as the definition does.
#include <cmath>
#include "common.h"

namespace isd {

constexpr int kPacMaxT = 4096;
constexpr int kPacMaxBins = 64;
constexpr int kPacMaxSurr = 4095;
constexpr int kPacBlock = 8;                                     // records per scalar load
constexpr int kPacSortWaves = 4;                                 // (row, p) per workgroup of the prepass
constexpr int kPacMainWaves = 4;                                 // at most; fewer when P is smaller
constexpr double kPacPi = 3.14159265358979323846;

__device__ __forceinline__ double pac_wave_sum(double v) {       // the same order in every lane and on every call
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// Items 0..n-1 ranked by (key(i), i), 0 <= key < 64: emit(i, rank) once per item, by the lane i & 63.  Returns in
// lane j the rank of the first item of key j (the number of items if there is none after it).
template <typename KeyFn, typename EmitFn>
__device__ __forceinline__ int pac_rank_by_key(int n, int lane, KeyFn key, EmitFn emit) {
  const unsigned long long below = (1ull << lane) - 1ull;
  int cnt = 0;                                                   // lane j: the items of key j
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int b = i < n ? key(i) : -1;
    unsigned long long rem = __ballot(i < n);
    while (rem) {                                                // once per key present among these 64 items
      const int j = __builtin_amdgcn_readlane(b, __builtin_ctzll(rem));
      const unsigned long long m = __ballot(b == j);
      if (lane == j) cnt += __builtin_popcountll(m);
      rem &= ~m;
    }
  }
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  const int first = incl - cnt;
  int run = first;                                               // lane j: the rank of the next item of key j
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int b = i < n ? key(i) : -1;
    int rank = 0;
    unsigned long long rem = __ballot(i < n);
    while (rem) {
      const int j = __builtin_amdgcn_readlane(b, __builtin_ctzll(rem));
      const unsigned long long m = __ballot(b == j);
      const int base = __builtin_amdgcn_readlane(run, j);
      if (b == j) rank = base + __builtin_popcountll(m & below);
      if (lane == j) run += __builtin_popcountll(m);
      rem &= ~m;
    }
    if (i < n) emit(i, rank);                                    // rank < n
  }
  return first;
}

__device__ __forceinline__ int pac_bin(double phi, int B, double c) {
  const double v = floor((phi + kPacPi) * c);                    // one add, one multiply, floor: NumPy's bits
  return v >= 0.0 ? (v <= (double)(B - 1) ? (int)v : B - 1) : 0; // a NaN goes to bin 0
}

template <typename S>
__global__ __launch_bounds__(64 * kPacSortWaves) void pac_sort_kernel(const S* __restrict__ pha, S* __restrict__ cs,
                                                                      int* __restrict__ ti, int* __restrict__ off,
                                                                      int64_t n_rp, int T, int Tp, int B, double c) {
  using V2 = S __attribute__((ext_vector_type(2)));
  const int lane = threadIdx.x & 63;
  const int64_t rp = (int64_t)blockIdx.x * kPacSortWaves + (threadIdx.x >> 6);
  if (rp >= n_rp) return;                                        // wave-uniform
  const S* ph = pha + rp * T;
  V2* csr = reinterpret_cast<V2*>(cs) + rp * Tp;
  int* tir = ti + rp * Tp;
  const int first = pac_rank_by_key(
      T, lane, [&](int t) { return pac_bin((double)ph[t], B, c); },
      [&](int t, int pos) {
        double sn, cn;
        sincos((double)ph[t], &sn, &cn);
        const V2 v = {(S)cn, (S)sn};
        csr[pos] = v;
        tir[pos] = t;
      });
  int* offr = off + rp * (kPacMaxBins + 1);
  if (lane < B) offr[lane] = first;
  if (lane == 0) offr[B] = T;
}

__device__ __forceinline__ int pac_shift(const int* __restrict__ shifts, int idx, int T) {
  return idx >= 1 ? min(max(shifts[idx], 0), T - 1) : 0;
}

// order[r] = the index of the shift of rank r by (shift mod 32, index); order[0] = 0, the estimate
__global__ __launch_bounds__(64) void pac_order_kernel(const int* __restrict__ shifts, int* __restrict__ order, int n,
                                                       int T) {
  pac_rank_by_key(
      n, (int)threadIdx.x, [&](int i) { return pac_shift(shifts, i, T) & 31; },
      [&](int i, int rank) { order[rank] = i; });
}

__device__ __forceinline__ float pac_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double pac_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float pac_log(float x) { return logf(x); }
__device__ __forceinline__ double pac_log(double x) { return log(x); }
__device__ __forceinline__ float pac_read_lane(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ __forceinline__ double pac_read_lane(double v, int src) { return read_lane(v, src); }

template <typename S>
struct PacBlock {                                                // kPacBlock records, wave-uniform
  int t[kPacBlock];
  S c[kPacBlock], s[kPacBlock];
};

template <typename S>
__global__ __launch_bounds__(64 * kPacMainWaves) void pac_main_kernel(
    const S* __restrict__ amp, const S* __restrict__ cs, const int* __restrict__ ti, const int* __restrict__ off,
    const int* __restrict__ order, const int* __restrict__ shifts, S* __restrict__ out, S* __restrict__ surr, int A,
    int P, int T, int Tp, int B, int n_surr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pac_lds[];
  const int lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // uniform, and known to be: scalar record loads
  S* a2 = reinterpret_cast<S*>(pac_lds);                         // [2 T]

  const int64_t rq = blockIdx.x;                                 // (row, q)
  const int64_t row = rq / A;
  const S* ar = amp + rq * T;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const S v = ar[t];
    a2[t] = v;
    a2[t + T] = v;
  }
  __syncthreads();
  double asum = 0.0;                                             // every wave: the same sum in the same order
  for (int t = lane; t < T; t += 64) asum += (double)a2[t];
  asum = pac_wave_sum(asum);
  const S rinv = asum > 0.0 ? (S)((double)T / asum) : (S)0;
  const double inv_log_b = 1.0 / log((double)B), inv_t = 1.0 / (double)T;
  const int n = 1 + n_surr, H = (n + 31) >> 5;                   // H half-waves hold the n shifts
  const int n_groups = (H + 1) >> 1;

  for (int p = wave; p < P; p += n_waves) {                      // wave-uniform
    const int64_t rp = row * P + p;
    const S* gcs = cs + rp * Tp * 2;
    const int* gti = ti + rp * Tp;
    const int* offr = off + rp * (kPacMaxBins + 1);
    const int seg_end = lane < B ? offr[lane + 1] : T;           // lane j: where bin j ends
    const int64_t obase = (rq * P + p) * 3;

    S v0[3] = {(S)0, (S)0, (S)0}, piv[3] = {(S)0, (S)0, (S)0};
    double sd[3] = {0.0, 0.0, 0.0}, sdd[3] = {0.0, 0.0, 0.0};
    int nge[3] = {0, 0, 0};

    for (int g = 0; g < n_groups; ++g) {
      const int h = 2 * g + (lane >> 5), r = (lane & 31) * H + h;         // this lane's rank in `order`
      const bool live = h < H && r < n;
      const int idx = live ? order[r] : 0;                       // order[0] = 0: lane 0 of group 0 is the estimate
      const bool is_surr = live && idx >= 1;
      const S* ap = a2 + pac_shift(shifts, is_surr ? idx : 0, T);         // ap[t], t < T: inside a2's 2 T

      S re = (S)0, im = (S)0, bs = (S)0, mx = (S)0, mn = (S)INFINITY;
      double M = 0.0, L = 0.0;
      int j = 0, start = 0, endj = __builtin_amdgcn_readlane(seg_end, 0);
      auto close_bin = [&]() {                                   // wave-uniform but for u
        const int nj = endj - start;
        const S u = nj > 0 ? bs / (S)nj * rinv : (S)0;
        M += (double)u;
        if (u > (S)0) L = fma((double)u, (double)pac_log(u), L);
        mx = u > mx ? u : mx;
        mn = u < mn ? u : mn;
        bs = (S)0;
        start = endj;
        ++j;
        endj = j < B ? __builtin_amdgcn_readlane(seg_end, j) : -1;
      };
      auto load = [&](int k) {                                   // k a multiple of kPacBlock below Tp
        PacBlock<S> b;
#pragma unroll
        for (int i = 0; i < kPacBlock; ++i) {
          b.t[i] = gti[k + i];
          b.c[i] = gcs[2 * (k + i)];
          b.s[i] = gcs[2 * (k + i) + 1];
        }
        return b;
      };
      auto sample = [&](const PacBlock<S>& b, int i) {
        const S a = ap[b.t[i]];
        re = pac_fma(a, b.c[i], re);
        im = pac_fma(a, b.s[i], im);
        bs += a;
      };

      PacBlock<S> cur = load(0);
      for (int k = 0; k < T; k += kPacBlock) {
        const PacBlock<S> nxt = load(k + kPacBlock < T ? k + kPacBlock : k);
        if (k + kPacBlock <= min(T, endj)) {                     // inside one bin: j < B and endj > k here
#pragma unroll
          for (int i = 0; i < kPacBlock; ++i) sample(cur, i);
        } else {
#pragma unroll
          for (int i = 0; i < kPacBlock; ++i) {
            while (j < B && endj == k + i) close_bin();          // every bin that ends here, empty ones too
            if (k + i < T) sample(cur, i);
          }
        }
        cur = nxt;
      }
      while (j < B) close_bin();                                 // what ends at T

      S v[3];
      v[0] = (S)(sqrt((double)re * (double)re + (double)im * (double)im) * inv_t);
      v[1] = (S)(1.0 + (L / M - log(M)) * inv_log_b);
      v[2] = (mx - mn) / mx;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        if (g == 0) {                                            // lane 1 holds rank H < n, a surrogate, when S >= 1
          v0[m] = pac_read_lane(v[m], 0);
          piv[m] = pac_read_lane(v[m], n_surr >= 1 ? 1 : 0);
        }
        if (is_surr) {
          if (surr) surr[(obase + m) * n_surr + idx - 1] = v[m];
          const double d = (double)v[m] - (double)piv[m];
          sd[m] += d;
          sdd[m] = fma(d, d, sdd[m]);
        }
        nge[m] += __builtin_popcountll(__ballot(is_surr && v[m] >= v0[m]));
      }
    }

#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double ns = (double)n_surr;
      const double md = pac_wave_sum(sd[m]) / ns;                // S = 0: 0 / 0, NaN
      double var = pac_wave_sum(sdd[m]) / ns - md * md;
      var = var < 0.0 ? 0.0 : var;                               // (a NaN stays a NaN)
      if (lane == 0) {
        S* o = out + (obase + m) * 4;
        o[0] = v0[m];
        o[1] = (S)((double)piv[m] + md);
        o[2] = (S)sqrt(var);
        o[3] = (S)nge[m];
      }
    }
  }
}

}  // namespace isd

using namespace isd;

namespace {

int64_t pac_padded(int64_t T) { return cdiv(T, kPacBlock) * kPacBlock; }

// The workspace in bytes: per (row, p) the ranked (cos, sin) records, their sample indices and the bin offsets; then the
// surrogates' order, whose whole lines also keep the buffer from being empty.
struct PacWs { int64_t cs, ti, off, order, end; };
PacWs pac_layout(int64_t n_rp, int64_t T, int64_t el) {
  static_assert((kPacMaxSurr + 1) * 4 % 256 == 0, "`order` ends on a line: the size is in whole lines");
  PacWs l;
  WorkCarver c;
  l.cs = c.take(n_rp * pac_padded(T) * 2 * el, 256);
  l.ti = c.take(n_rp * pac_padded(T) * 4, 256);
  l.off = c.take(n_rp * (kPacMaxBins + 1) * 4, 256);
  l.order = c.take((kPacMaxSurr + 1) * 4, 256);
  l.end = c.end;
  return l;
}

template <typename S>
int pac_launch(const S* pha, const S* amp, const int32_t* shifts, S* out, S* surr, int64_t rows, int64_t P, int64_t A,
               int64_t T, int64_t n_surr, int n_bins, double c, void* work, void* stream, const char* who) {
  ISD_CHECK_ARG(rows >= 0 && P >= 1 && A >= 1, "%s: rows=%lld P=%lld A=%lld", who, (long long)rows, (long long)P,
                (long long)A);
  ISD_CHECK_ARG(T >= 1 && n_surr >= 0 && n_bins >= 1, "%s: T=%lld S=%lld n_bins=%d", who, (long long)T,
                (long long)n_surr, n_bins);
  ISD_CHECK_SUPPORTED(T <= kPacMaxT, "%s: T=%lld (need 1 <= T <= %d)", who, (long long)T, kPacMaxT);
  ISD_CHECK_SUPPORTED(n_bins >= 2 && n_bins <= kPacMaxBins, "%s: n_bins=%d (need 2 <= n_bins <= %d)", who, n_bins,
                      kPacMaxBins);
  ISD_CHECK_SUPPORTED(n_surr <= kPacMaxSurr, "%s: S=%lld surrogates (need 0 <= S <= %d)", who, (long long)n_surr,
                      kPacMaxSurr);
  ISD_CHECK_SUPPORTED((double)rows * (double)A * (double)P < 2147483648.0,
                      "%s: rows * A * P = %lld * %lld * %lld (need < 2^31)", who, (long long)rows, (long long)A,
                      (long long)P);
  ISD_CHECK_ARG(c > 0.0, "%s: c=%g", who, c);
  if (rows == 0) return ISD_OK;
  ISD_CHECK_ARG(pha && amp && shifts && out && work, "%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_rp = rows * P;
  const PacWs l = pac_layout(n_rp, T, sizeof(S));
  char* w = static_cast<char*>(work);
  S* cs = reinterpret_cast<S*>(w + l.cs);
  int* ti = reinterpret_cast<int*>(w + l.ti);
  int* off = reinterpret_cast<int*>(w + l.off);
  int* order = reinterpret_cast<int*>(w + l.order);
  const int Tp = (int)pac_padded(T);
  hipLaunchKernelGGL((pac_sort_kernel<S>), dim3((unsigned)cdiv(n_rp, kPacSortWaves)), dim3(64 * kPacSortWaves), 0, st,
                     pha, cs, ti, off, n_rp, (int)T, Tp, n_bins, c);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(pac_order_kernel, dim3(1), dim3(64), 0, st, (const int*)shifts, order, (int)n_surr + 1, (int)T);
  ISD_LAUNCH_CHECK();
  const int n_waves = (int)(P < kPacMainWaves ? P : kPacMainWaves);
  return launch_lds(pac_main_kernel<S>, dim3((unsigned)(rows * A)), dim3(64 * n_waves), (size_t)2 * T * sizeof(S), st,
                    amp, (const S*)cs, (const int*)ti, (const int*)off, (const int*)order, (const int*)shifts, out,
                    surr, (int)A, (int)P, (int)T, Tp, n_bins, (int)n_surr);
}

}  // namespace

extern "C" int64_t isd_pac_work_bytes(int64_t rows, int64_t P, int64_t A, int64_t T, int is_f64) {
  if (rows < 0 || P < 1 || A < 1 || T < 1 || T > kPacMaxT || (double)rows * (double)P * (double)A >= 2147483648.0) {
    set_error("isd_pac_work_bytes: rows=%lld, P=%lld, A=%lld or T=%lld", (long long)rows, (long long)P, (long long)A,
              (long long)T);
    return T > kPacMaxT ? ISD_ERR_UNSUPPORTED : ISD_ERR_INVALID;
  }
  return pac_layout(rows * P, T, is_f64 ? 8 : 4).end;
}

extern "C" int isd_pac_f32(const float* pha, const float* amp, const int32_t* shifts, float* out, float* surr,
                           int64_t rows, int64_t P, int64_t A, int64_t T, int64_t n_surr, int n_bins, double c,
                           void* work, void* stream) {
  return pac_launch<float>(pha, amp, shifts, out, surr, rows, P, A, T, n_surr, n_bins, c, work, stream, "isd_pac_f32");
}

extern "C" int isd_pac_f64(const double* pha, const double* amp, const int32_t* shifts, double* out, double* surr,
                           int64_t rows, int64_t P, int64_t A, int64_t T, int64_t n_surr, int n_bins, double c,
                           void* work, void* stream) {
  return pac_launch<double>(pha, amp, shifts, out, surr, rows, P, A, T, n_surr, n_bins, c, work, stream, "isd_pac_f64");
}
