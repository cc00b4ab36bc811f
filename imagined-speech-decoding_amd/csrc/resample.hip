// Polyphase rational resampling: scipy.signal.resample_poly (isd_amd.resample_poly, isd_amd.resample).
//
//   y[n] = bg + sum_m xe[m] h[half + n down - m up]     over the m with 0 <= half + n down - m up < L,  0 <= n < n_out
//
// n_out = ceil(T up / down); h are the L taps (already times up), half their centre; xe is the row (minus its
// background bg, when one is given) extended beyond 0 .. T-1 by `mode`.  Taps, up and down come from the host
// (isd_amd/resampling.py resample_design); the library knows nothing about windows.
//
// A row's outputs are cut into blocks of 16.  With q = 16 b down = Q up + phi (0 <= phi < up), block b is the banded
// product
//   Y[rows x 16] = Xwin[rows x K] . B_phi[K x 16],    Xwin[r][k] = xe_r[Q + c(phi) + k],
//   B_phi[k][j] = h[half + phi + j down - (c(phi) + k) up]   (0 where that index leaves 0 .. L-1),
//   c(phi) = ceil((half + phi - (L - 1)) / up): the first sample any output of the block touches.
// B depends on phi alone and phi takes up / gcd(up, 16 down) values, so the plan holds that many [K][16] tables (K:
// the longest window over the phases, rounded up to 4) in fp32 and fp64, and the kernel never sees a tap index.
//
// Kernel: one wave per (slab of 64 rows, output block).  The window goes through LDS in chunks of KC samples (64 fp32,
// 32 fp64: 16 bytes per lane and row, four rows per pass).  A chunk that lies inside 0 .. T-1 is read with 16-byte
// loads when x, T and the chunk's first sample are aligned to them (a run-time test) and by element otherwise, eight
// passes in flight; a chunk over an end of the row goes sample by sample through the extension.  The background is
// taken off per element in fp64.  A sample outside 0 .. T-1 is never read, so no neighbouring row is touched even
// under a zero tap.  The chunk's B fragments (64 consecutive table elements per four samples) are requested before the
// staging and each feeds four v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, one per 16-row group with its own
// accumulator: output row r is a product of window row r alone, so rows do not mix, and the order of the sum is fixed
// by the plan -- no atomics, the same bits on every call and in every batch.  y is written by element (16 consecutive
// outputs of a row per quarter wave); x and y need element alignment only.
//
// A VALU kernel in the style of fir.hip was not written.  The first version of this kernel (element loads, one pass
// in flight) ran [2048, 128, 4096] fp32 at 1/4 in 10.7 ms, this one in 2.05 ms: 0.52 of the copy rate of its bytes and
// 24 % of the fp32 matrix rate.  What is left is the latency of one wave's stage-then-multiply
// sequence at two waves per SIMD; a second staging buffer is the next step.
#include "common.h"

#include <vector>

struct isd_resample_plan {
  int up, down, n_taps, half_len;
  int n_phase, phase_step;   // phi = phase_step * (index of the table), phase_step = gcd(up, 16 down)
  int K;                     // rows of every B table, a multiple of 4
  int* d_c0;                 // [n_phase] c(phi)
  float* d_bf;               // [n_phase][K][16]
  double* d_bd;
};

namespace isd {

constexpr int kRsRows = 64;                                // rows per wave: four MFMA row groups
constexpr int kRsBatch = 8;                               // staging passes (of 4 rows) in flight together
constexpr int64_t kRsTableBudget = (int64_t)16 << 20;      // bytes of device tables (fp32 + fp64) a plan may hold
enum { kRsConstant = 0, kRsEdge = 1, kRsReflect = 2, kRsSymmetric = 3, kRsLine = 4 };

template <typename S> struct RsOps;
template <> struct RsOps<float> : Mfma16<float> {
  static constexpr int KC = 64, LD = KC + 4;               // LD = 4 mod 64 dwords: the 64 A reads hit 64 banks
};
template <> struct RsOps<double> : Mfma16<double> {
  static constexpr int KC = 32, LD = KC + 2;               // 2 LD = 4 mod 64 dwords
};

// sample m of the row (minus bg) extended by `mode`; only indices inside 0 .. T-1 are read
template <typename S>
__device__ __forceinline__ S rs_ext(const S* __restrict__ row, int64_t m, int T, int mode, S cval, double bg,
                                    bool has_bg) {
  int64_t idx = m;
  if (m < 0 || m >= T) {
    if (mode == kRsConstant) return cval;
    if (mode == kRsLine) {                                 // T >= 2 (checked by the host)
      const double a = (double)row[0], b = (double)row[T - 1];
      return (S)(a + (b - a) / (double)(T - 1) * (double)m);
    }
    if (mode == kRsEdge) {
      idx = m < 0 ? 0 : T - 1;
    } else {                                               // whole-sample (period 2T - 2) or half-sample (2T) mirror
      const int64_t p = mode == kRsReflect ? 2 * (int64_t)T - 2 : 2 * (int64_t)T;
      int64_t r = m % p;
      if (r < 0) r += p;
      idx = r < T ? r : (mode == kRsReflect ? p - r : p - 1 - r);
    }
  }
  const S v = row[idx];
  return has_bg ? (S)((double)v - bg) : v;
}

template <typename S>
__global__ __launch_bounds__(64) void resample_kernel(const S* __restrict__ x, S* __restrict__ y,
                                                      const S* __restrict__ tables, const int* __restrict__ c0,
                                                      const double* __restrict__ background, int64_t rows, int T,
                                                      int n_out, int n_blocks, int up, int down, int phase_step, int K,
                                                      int mode, S cval) {
  using O = RsOps<S>;
  using Acc = typename O::Acc;
  using Vec = typename O::Vec;
  constexpr int KC = O::KC, LD = O::LD, VEC = O::VEC, STEPS = KC / 4;
  __shared__ __attribute__((aligned(16))) S xs[kRsRows * LD];
  const int lane = threadIdx.x;
  // workgroups are dealt to the eight XCDs in turn: renumber so that an XCD's workgroups are consecutive blocks of
  // the same rows, whose windows overlap, and share them in its L2
  const unsigned per_xcd = gridDim.x >> 3;
  const unsigned wg = blockIdx.x < 8 * per_xcd ? (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3) : blockIdx.x;
  const int64_t slab = wg / (unsigned)n_blocks;
  const int b = (int)(wg - slab * n_blocks);
  const int64_t row0 = slab * kRsRows;
  const int n_rows = rows - row0 < kRsRows ? (int)(rows - row0) : kRsRows;

  const int64_t q = (int64_t)16 * b * down;
  const int64_t Q = q / up;
  const int pi = (int)(q - Q * up) / phase_step;
  const int64_t m0 = Q + c0[pi];
  const S* __restrict__ B = tables + (int64_t)pi * K * 16;
  const bool has_bg = background != nullptr;
  const int sr = lane >> 4, sc = (lane & 15) * VEC;        // staging: 4 rows per pass, 16 bytes per lane

  Acc acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = (Acc){0, 0, 0, 0};

  for (int kc = 0; kc < K; kc += KC) {
    const int len = K - kc < KC ? K - kc : KC;             // a multiple of 4
    // the chunk's B fragments: requested in front of the staging, used behind it (past the chunk's end: a repeat)
    S bf[STEPS];
#pragma unroll
    for (int i = 0; i < STEPS; ++i) bf[i] = B[(int64_t)(kc + (4 * i < len ? 4 * i : len - 4)) * 16 + lane];
    if (kc) __syncthreads();                               // the previous chunk has been read
    const int64_t mc = m0 + kc;
    if (sc < len) {
      if (mc >= 0 && mc + len <= T) {
        // wave-uniform: no sample of the chunk needs the extension.  The passes are requested kRsBatch at a time before the first
        // of them is used.  A slab's missing rows repeat its last row: their products are never stored.
        const bool vec = ((reinterpret_cast<uintptr_t>(x) & 15) | ((uintptr_t)T & (VEC - 1)) | ((uintptr_t)mc & (VEC - 1))) == 0;
#pragma unroll
        for (int h = 0; h < kRsRows / 4; h += kRsBatch) {
        Vec t[kRsBatch];
        if (vec) {                                         // every row's 16 bytes are aligned
#pragma unroll
          for (int j = 0; j < kRsBatch; ++j) {
            const int r = sr + 4 * (h + j) < n_rows ? sr + 4 * (h + j) : n_rows - 1;
            t[j] = *reinterpret_cast<const Vec*>(x + (row0 + r) * T + mc + sc);
          }
        } else {
#pragma unroll
          for (int j = 0; j < kRsBatch; ++j) {
            const int r = sr + 4 * (h + j) < n_rows ? sr + 4 * (h + j) : n_rows - 1;
            const S* p = x + (row0 + r) * T + mc + sc;
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[j][e] = p[e];
          }
        }
        if (has_bg) {
#pragma unroll
          for (int j = 0; j < kRsBatch; ++j) {
            const int r = sr + 4 * (h + j) < n_rows ? sr + 4 * (h + j) : n_rows - 1;
            const double bg = background[row0 + r];
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[j][e] = (S)((double)t[j][e] - bg);
          }
        }
#pragma unroll
        for (int j = 0; j < kRsBatch; ++j) *reinterpret_cast<Vec*>(xs + (sr + 4 * (h + j)) * LD + sc) = t[j];
        }
      } else {                                             // a chunk over an end of the row: sample by sample
        for (int r = sr; r < kRsRows; r += 4) {
          Vec t;
#pragma unroll
          for (int e = 0; e < VEC; ++e) t[e] = (S)0;
          if (r < n_rows) {
            const double bg = has_bg ? background[row0 + r] : 0.0;
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[e] = rs_ext(x + (row0 + r) * T, mc + sc + e, T, mode, cval, bg, has_bg);
          }
          *reinterpret_cast<Vec*>(xs + r * LD + sc) = t;   // LD and sc are multiples of 16 bytes
        }
      }
    }
    __syncthreads();
    const S* pa = xs + (lane & 15) * LD + (lane >> 4);
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
      if (4 * i < len) {                                   // wave-uniform
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = O::mma(pa[g * 16 * LD + 4 * i], bf[i], acc[g]);
      }
    }
  }

  const int n = 16 * b + (lane & 15);
  if (n >= n_out) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = 16 * g + O::lane_row(lane, reg);
      if (r < n_rows) {
        const S v = acc[g][reg];
        y[(row0 + r) * n_out + n] = has_bg ? (S)((double)v + background[row0 + r]) : v;
      }
    }
  }
}

static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }
static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

}  // namespace isd

using namespace isd;

extern "C" int isd_resample_plan_create(isd_resample_plan** out, int up, int down, int n_taps, const double* taps,
                                        int half_len) {
  ISD_CHECK_ARG(out && taps, "isd_resample_plan_create: null argument");
  ISD_CHECK_ARG(up >= 1 && down >= 1 && n_taps >= 1, "isd_resample_plan_create: up=%d down=%d n_taps=%d (need >= 1)", up, down, n_taps);
  ISD_CHECK_ARG(gcd64(up, down) == 1, "isd_resample_plan_create: up=%d down=%d are not reduced", up, down);
  ISD_CHECK_ARG(half_len >= 0 && half_len < n_taps, "isd_resample_plan_create: half_len=%d outside the %d taps", half_len, n_taps);
  ISD_CHECK_SUPPORTED(up <= ISD_RESAMPLE_MAX_RATE && down <= ISD_RESAMPLE_MAX_RATE, "isd_resample_plan_create: up=%d down=%d (at most %d is provided)", up, down, ISD_RESAMPLE_MAX_RATE);
  ISD_CHECK_SUPPORTED(n_taps <= ISD_RESAMPLE_MAX_TAPS, "isd_resample_plan_create: %d taps (at most %d are provided)", n_taps, ISD_RESAMPLE_MAX_TAPS);
  const int L = n_taps;
  const int step = (int)gcd64(up, (int64_t)16 * down), n_phase = up / step;
  std::vector<int> c0(n_phase);
  int64_t K = 0;
  for (int i = 0; i < n_phase; ++i) {
    const int64_t phi = (int64_t)i * step;
    c0[i] = (int)ceil_div(half_len + phi - (L - 1), up);
    const int64_t last = floor_div(half_len + phi + (int64_t)15 * down, up);      // last sample of output 15
    if (last - c0[i] + 1 > K) K = last - c0[i] + 1;
  }
  K = (K + 3) / 4 * 4;
  const int64_t n_el = (int64_t)n_phase * K * 16;
  ISD_CHECK_SUPPORTED(n_el * (int64_t)(sizeof(float) + sizeof(double)) <= kRsTableBudget, "isd_resample_plan_create: the phase tables need %lld bytes (budget %lld)", (long long)(n_el * 12), (long long)kRsTableBudget);
  if (int rc = require_device("isd_resample_plan_create")) return rc;
  std::vector<double> bd((size_t)n_el, 0.0);
  std::vector<float> bf((size_t)n_el, 0.f);
  for (int i = 0; i < n_phase; ++i)
    for (int64_t k = 0; k < K; ++k)
      for (int j = 0; j < 16; ++j) {
        const int64_t t = half_len + (int64_t)i * step + (int64_t)j * down - (c0[i] + k) * up;
        if (t >= 0 && t < L) {
          const size_t at = ((size_t)i * K + k) * 16 + j;
          bd[at] = taps[t];
          bf[at] = (float)taps[t];
        }
      }
  isd_resample_plan* p = new isd_resample_plan();
  p->up = up; p->down = down; p->n_taps = n_taps; p->half_len = half_len;
  p->n_phase = n_phase; p->phase_step = step; p->K = (int)K;
  hipError_t e = upload(&p->d_c0, c0);
  if (e == hipSuccess) e = upload(&p->d_bf, bf);
  if (e == hipSuccess) e = upload(&p->d_bd, bd);
  if (e != hipSuccess) {
    set_error("isd_resample_plan_create: %s", hipGetErrorString(e));
    isd_resample_plan_destroy(p);
    return ISD_ERR_HIP;
  }
  *out = p;
  return ISD_OK;
}

extern "C" int isd_resample_plan_destroy(isd_resample_plan* p) {
  if (!p) return ISD_OK;
  if (p->d_c0) (void)hipFree(p->d_c0);
  if (p->d_bf) (void)hipFree(p->d_bf);
  if (p->d_bd) (void)hipFree(p->d_bd);
  delete p;
  return ISD_OK;
}

extern "C" int64_t isd_resample_out_len(const isd_resample_plan* p, int64_t T) {
  if (!p || T < 0) return ISD_ERR_INVALID;
  return (T * p->up + p->down - 1) / p->down;
}

template <typename S>
static int resample_launch(const isd_resample_plan* p, const S* x, S* y, int64_t rows, int T, int mode, double cval,
                           const double* background, void* stream, const S* tables) {
  ISD_CHECK_ARG(p && x && y, "isd_resample_poly: null argument");
  ISD_CHECK_ARG(rows >= 0 && T >= 1, "isd_resample_poly: rows=%lld T=%d", (long long)rows, T);
  ISD_CHECK_ARG(mode >= kRsConstant && mode <= kRsLine, "isd_resample_poly: mode=%d", mode);
  ISD_CHECK_ARG(T >= 2 || (mode != kRsReflect && mode != kRsLine), "isd_resample_poly: mode %d needs T >= 2", mode);
  ISD_CHECK_ARG((const void*)x != (const void*)y, "isd_resample_poly: in-place resampling is not supported");
  const int64_t n_out = isd_resample_out_len(p, T);
  ISD_CHECK_SUPPORTED(n_out <= INT32_MAX, "isd_resample_poly: %lld output samples per row (need < 2^31)", (long long)n_out);
  if (rows == 0) return ISD_OK;
  const int64_t n_blocks = cdiv(n_out, 16), slabs = cdiv(rows, kRsRows);
  // one workgroup per (slab, block) on grid.x; a launch takes as many whole slabs as fit under 2^31 - 1 workgroups
  const int64_t per = INT32_MAX / n_blocks;
  for (int64_t s0 = 0; s0 < slabs; s0 += per) {
    const int64_t ns = slabs - s0 < per ? slabs - s0 : per;
    const int64_t r0 = s0 * kRsRows;
    hipLaunchKernelGGL((resample_kernel<S>), dim3((unsigned)(ns * n_blocks)), dim3(64), 0, (hipStream_t)stream,
                       x + r0 * T, y + r0 * n_out, tables, p->d_c0, background ? background + r0 : nullptr, rows - r0,
                       T, (int)n_out, (int)n_blocks, p->up, p->down, p->phase_step, p->K, mode, (S)cval);
    ISD_LAUNCH_CHECK();
  }
  return ISD_OK;
}

extern "C" int isd_resample_poly_f32(const isd_resample_plan* p, const float* x, float* y, int64_t rows, int T,
                                     int mode, double cval, const double* background, void* stream) {
  return resample_launch<float>(p, x, y, rows, T, mode, cval, background, stream, p ? p->d_bf : nullptr);
}

extern "C" int isd_resample_poly_f64(const isd_resample_plan* p, const double* x, double* y, int64_t rows, int T,
                                     int mode, double cval, const double* background, void* stream) {
  return resample_launch<double>(p, x, y, rows, T, mode, cval, background, stream, p ? p->d_bd : nullptr);
}
