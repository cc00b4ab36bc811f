// Riemannian geometry of covariance matrices: the data-sized steps of isd_amd.riemann (Covariances -> TangentSpace ->
// a linear classifier, and MDM), the covariance-manifold baseline beside CSP + SVM of notebooks/svm_baseline.ipynb.
// Everything after the covariance is a matrix function of n small symmetric positive-definite matrices.  The [K][C][C]
// work (square roots of the class means, exp, step control) stays on the host (isd_amd/riemann.py).  All fp64.
//
//   spd_congruence  out_i = W_k cov_i W_k^T, k = widx[i].  One workgroup of four waves per matrix, two products on
//                   v_mfma_f64_16x16x4_f64:  Y = cov_i W_k^T  (all tiles, kept in LDS, zero beyond C),  then
//                   out = W_k Y  on the UPPER 16x16 tiles only, each value stored at [a][b] and [b][a].  A wave owns
//                   whole tile rows, so one operand from memory per k step feeds up to eight MFMAs.  The operands
//                   that come from memory (cov_i, W_k) are read per lane straight into the MFMA operand registers
//                   (clamped addresses, zeroed by selects: no read past a row or past C rows);
//                   W_k is shared by every matrix of its class and stays in L1 / L2.
//   spd_eigfun      A = V L V^T, f(A) = V f(L) V^T by one-sided (Hestenes) Jacobi on the columns of G = A: plane
//                   rotations from the right make the columns mutually orthogonal, and then G = V L, so that
//                   l_j = |g_j| and v_j = g_j / |g_j|; V itself is never stored.  One workgroup per matrix, G
//                   column-major in LDS (the only C x C array there).  A sweep is m - 1 rounds (m = C rounded up to
//                   even) of m / 2 disjoint column pairs in round-robin (circle method) order; a pair belongs to a
//                   group of L lanes, each lane holding rows l, l + L, ... of both columns in registers.  Per round:
//                   three dot products (serial per lane, xor tree over the group: every lane ends with the same
//                   bits), the rotation  zeta = (beta - alpha) / (2 gamma),  t = sign(zeta) / (|zeta| + sqrt(1 +
//                   zeta^2)),  c = 1 / sqrt(1 + t^2),  s = c t,  the update of both columns, ONE barrier.  A pair is
//                   left alone when |gamma| <= tol sqrt(alpha beta), tol = C * 2^-52: the rounding error of gamma
//                   itself is of that order, so a tighter test would chase noise.  The iteration stops after the
//                   first sweep without a rotation and in any case after kSpdMaxSweeps sweeps: every loop is bounded
//                   by a count.  A NaN fails the `>` test, so a NaN matrix stops rotating at once.
//                   Epilogue: f(A)[a][b] = sum_j f(l_j) / l_j^2 g_j[a] g_j[b] for a <= b from LDS to memory.
//                   G = V L keeps |l| only; the sign is checked through the trace: sum_j |l_j| exceeds trace(A) iff an
//                   eigenvalue is negative.
//                   Pair order and every sum order are fixed and depend on C alone: a matrix's result is the same
//                   bits wherever it stands in whatever batch.
#include <float.h>
#include "common.h"

namespace isd {

constexpr int kSpdMaxC = 128;
constexpr int kSpdMaxSweeps = 30;
constexpr int kCongWaves = 4;
constexpr int kCongPad = 4;                                     // LDS row skew of Y (doubles)

__device__ __forceinline__ double spd_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---------------------------------------------------------------------------------------------------- congruence
// Keeps a loaded value from being sunk behind the test that selects it.  Put AFTER a group of loads: the value has
// to be there at this point, so the loads before it are issued together and waited for in order.
__device__ __forceinline__ double spd_pin(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// NT = nt: 16 x 16 tiles per side
template <typename S, int NT>
__global__ __launch_bounds__(64 * kCongWaves) void spd_congruence_kernel(const S* __restrict__ cov,
                                                                         const double* __restrict__ W,
                                                                         const int* __restrict__ widx,
                                                                         double* __restrict__ out, int C, int K) {
  using O = Mfma16<double>;                                      // both products run in fp64 whatever S is
  extern __shared__ __attribute__((aligned(16))) unsigned char cong_smem[];
  double* ys = reinterpret_cast<double*>(cong_smem);             // [Cp][ldy]: Y = cov W^T, zero beyond C
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int nt = NT, Cp = nt * 16, ldy = Cp + kCongPad;      // C in (16 (NT - 1), 16 NT]
  const int64_t CC = (int64_t)C * C;
  const S* ci = cov + (int64_t)blockIdx.x * CC;
  double* oi = out + (int64_t)blockIdx.x * CC;
  const int k = widx ? widx[blockIdx.x] : 0;
  if (k < 0 || k >= K) {                                         // workgroup-uniform; W is never read outside [0, K)
    for (int e = tid; e < C * C; e += 64 * kCongWaves) oi[e] = spd_nan();
    return;
  }
  const double* wk = W + (int64_t)k * CC;
  const int lr = lane & 15, lk = lane >> 4;                      // operand row / column, operand k

  // Y tile row ti = cov[ti rows][:] . W^T: one operand of cov per k step serves the nt tiles of the row
  for (int ti = wave; ti < nt; ti += kCongWaves) {
    const int ra = ti * 16 + lr;
    const S* pa = ci + (int64_t)min(ra, C - 1) * C;              // clamped: never past C rows
    f64x4 acc[NT];
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) acc[tj] = (f64x4)(0);
    // Sixteen channels (four k steps) per turn: all their loads are issued first, unconditionally at clamped
    // addresses, and zeroed by selects afterwards.  Behind a test each load would be waited for by itself; spd_pin
    // keeps the compiler from putting them back there.
    for (int c0 = 0; c0 < Cp; c0 += 16) {
      double av[4], bv[4][NT];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int cc = min(c0 + 4 * s + lk, C - 1);              // clamped: never past a row
        av[s] = (double)pa[cc];
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) bv[s][tj] = wk[(int64_t)min(tj * 16 + lr, C - 1) * C + cc];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        av[s] = spd_pin(av[s]);
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) bv[s][tj] = spd_pin(bv[s][tj]);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bool inc = c0 + 4 * s + lk < C;
        const double a = (ra < C && inc) ? av[s] : 0.0;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
          const double b = (tj * 16 + lr < C && inc) ? bv[s][tj] : 0.0;
          acc[tj] = O::mma(a, b, acc[tj]);
        }
      }
    }
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) ys[(ti * 16 + O::row(lk, r)) * ldy + tj * 16 + lr] = acc[tj][r];
  }
  __syncthreads();

  // out tile row ti = W[ti rows][:] . Y on the tiles tj >= ti.  A wave takes rows pp and nt - 1 - pp, which together
  // hold nt + 1 tiles whatever pp is.
  for (int pp = wave; 2 * pp < nt; pp += kCongWaves) {
    for (int h = 0; h < 2; ++h) {
      const int ti = h ? nt - 1 - pp : pp;
      if (h && ti == pp) break;                                  // the middle row of an odd nt, once
      const int ra = ti * 16 + lr;
      const double* pa = wk + (int64_t)min(ra, C - 1) * C;
      f64x4 acc[NT];
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) acc[tj] = (f64x4)(0);
      for (int c0 = 0; c0 < Cp; c0 += 16) {
        double av[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[s] = pa[min(c0 + 4 * s + lk, C - 1)];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[s] = spd_pin(av[s]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int c = c0 + 4 * s + lk;
          const double a = (ra < C && c < C) ? av[s] : 0.0;
          const double* pb = ys + c * ldy + lr;
#pragma unroll
          for (int tj = 0; tj < NT; ++tj)
            if (tj >= ti) acc[tj] = O::mma(a, pb[tj * 16], acc[tj]);
        }
      }
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) {
        if (tj >= ti) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = ti * 16 + O::row(lk, r), b = tj * 16 + lr;
            if (a <= b && b < C) {                               // a <= b < C; the lower triangle is the mirror
              oi[a * C + b] = acc[tj][r];
              oi[b * C + a] = acc[tj][r];
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------- eigfun
__device__ __forceinline__ double spd_apply(double lam, int fn) {
  switch (fn) {
    case ISD_SPD_LOG: return log(lam);
    case ISD_SPD_SQRT: return sqrt(lam);
    case ISD_SPD_INVSQRT: return 1.0 / sqrt(lam);
    case ISD_SPD_INV: return 1.0 / lam;
    default: return lam;
  }
}

template <int L>
__device__ __forceinline__ double group_sum(double v) {          // xor tree over L consecutive lanes: all get the sum
#pragma unroll
  for (int d = L / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// blockDim.x = PAIRS * L: lane group `grp` owns the grp-th pair of every round; C <= 2 * PAIRS and C <= L * NR.
template <int L, int NR, int PAIRS>
__global__ __launch_bounds__(PAIRS* L) void spd_eigfun_kernel(const double* __restrict__ a, double* __restrict__ out,
                                                             double* __restrict__ eigvals, int* __restrict__ info,
                                                             int C, int fn, int out_kind) {
  constexpr int NT = PAIRS * L;
  extern __shared__ __attribute__((aligned(16))) unsigned char eig_smem[];
  const int ld = C | 1;                                          // odd column stride: columns start on distinct banks
  double* g = reinterpret_cast<double*>(eig_smem);               // [C][ld], g[j * ld + r] = G[r][j]
  double* wj = g + C * ld;                                       // [C] f(l_j) / l_j^2
  double* lamv = wj + C;                                         // [C] l_j
  double* diag = lamv + C;                                       // [C] A[c][c], kept for the trace test
  int* rotated = reinterpret_cast<int*>(diag + C);               // [kSpdMaxSweeps] a rotation happened in sweep s
  int* status = rotated + kSpdMaxSweeps;                         // [1]
  const int tid = threadIdx.x, grp = tid / L, l = tid % L;
  const int64_t CC = (int64_t)C * C;
  const double* ai = a + (int64_t)blockIdx.x * CC;

  for (int e = tid; e < C * C; e += NT) {
    const double v = ai[e];
    g[(e % C) * ld + e / C] = v;
    if (e % C == e / C) diag[e / C] = v;                         // g itself is rotated from the first round on
  }
  if (tid < kSpdMaxSweeps) rotated[tid] = 0;
  __syncthreads();

  const int m = C + (C & 1), m1 = m - 1;                         // columns with the phantom of an odd C; rounds
  const double tol = (double)C * DBL_EPSILON;
  int sweeps = 0;
  bool converged = false;
  for (int s = 0; s < kSpdMaxSweeps && !converged; ++s) {        // workgroup-uniform: `rotated` is read after a barrier
    for (int r = 0; r < m1; ++r) {
      int p = grp == 0 ? m1 : (r + grp) % m1;
      int q = grp == 0 ? r : (r - grp + m1) % m1;
      if (p > q) { const int t = p; p = q; q = t; }
      if (2 * grp < m && q < C) {                                // uniform over the lane group; p < q < C
        double* gp = g + p * ld;
        double* gq = g + q * ld;
        double x[NR], y[NR];
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int row = l + i * L;
          x[i] = row < C ? gp[row] : 0.0;
          y[i] = row < C ? gq[row] : 0.0;
          alpha = fma(x[i], x[i], alpha);
          beta = fma(y[i], y[i], beta);
          gamma = fma(x[i], y[i], gamma);
        }
        alpha = group_sum<L>(alpha);
        beta = group_sum<L>(beta);
        gamma = group_sum<L>(gamma);
        if (fabs(gamma) > tol * sqrt(alpha * beta)) {            // false for NaN: a NaN matrix is left alone
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));   // 0 if zeta^2 overflows
          const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
          for (int i = 0; i < NR; ++i) {
            const int row = l + i * L;
            if (row < C) {
              gp[row] = c * x[i] - sn * y[i];
              gq[row] = sn * x[i] + c * y[i];
            }
          }
          if (l == 0) rotated[s] = 1;                            // every writer stores the same value
        }
      }
      __syncthreads();                                           // the one barrier of the round
    }
    sweeps = s + 1;
    converged = rotated[s] == 0;
  }

  // l_j = |g_j| in row order, one thread per column; its weight f(l_j) / l_j^2 (0 for a zero column: v_j is then
  // undefined and f(0) = 0 for the functions that accept it)
  if (tid < C) {
    const double* gj = g + tid * ld;
    double s2 = 0.0;
    for (int r = 0; r < C; ++r) s2 = fma(gj[r], gj[r], s2);
    const double lam = sqrt(s2);
    lamv[tid] = lam;
    wj[tid] = lam > 0.0 ? spd_apply(lam, fn) / s2 : 0.0;
    if (eigvals) eigvals[(int64_t)blockIdx.x * C + tid] = lam;
  }
  __syncthreads();                                               // wj, lamv complete; nobody writes g any more
  if (tid == 0) {
    const bool need_pos = fn == ISD_SPD_LOG || fn == ISD_SPD_INVSQRT || fn == ISD_SPD_INV;
    double sum = 0.0, trace = 0.0;
    bool bad = false;
    for (int j = 0; j < C; ++j) {
      const double lj = lamv[j];
      sum += lj;
      trace += diag[j];
      bad = bad || !(lj <= DBL_MAX) || !(wj[j] == wj[j]) || fabs(wj[j]) > DBL_MAX || (need_pos && !(lj > 0.0));
    }
    // trace(A) = sum of the signed eigenvalues; both sides carry rounding of the order C eps sum|l|
    bad = bad || !(trace >= sum * (1.0 - 64.0 * (double)C * DBL_EPSILON));
    const int st = bad ? -2 : (converged ? sweeps : -1);
    *status = st;
    if (info) info[blockIdx.x] = st;
  }
  __syncthreads();
  if (out_kind == ISD_SPD_NOOUT) return;
  const bool bad = *status == -2;
  const int64_t tri = (int64_t)C * (C + 1) / 2;
  double* oi = out + (int64_t)blockIdx.x * (out_kind == ISD_SPD_FULL ? CC : tri);
  for (int e = tid; e < C * C; e += NT) {
    const int ra = e % C, rb = e / C;                            // consecutive lanes: consecutive rows of one g_j
    if (ra > rb) continue;
    double acc = 0.0;
    for (int j = 0; j < C; ++j) acc = fma(wj[j] * g[j * ld + ra], g[j * ld + rb], acc);
    if (bad) acc = spd_nan();
    if (out_kind == ISD_SPD_FULL) {
      oi[ra * C + rb] = acc;
      oi[rb * C + ra] = acc;
    } else {                                                     // np.triu_indices(C) order, off-diagonal times sqrt 2
      oi[(int64_t)ra * C - ra * (ra - 1) / 2 + (rb - ra)] = ra == rb ? acc : acc * 1.4142135623730951;
    }
  }
}

}  // namespace isd

using namespace isd;

template <typename S>
static int congruence_launch(const S* cov, const double* W, const int* widx, double* out, int64_t n, int C, int K,
                             hipStream_t st) {
  const int nt = (C + 15) / 16, Cp = nt * 16;
  const size_t lds = (size_t)Cp * (Cp + kCongPad) * sizeof(double);                  // <= 132 KiB
  const dim3 grid((unsigned)n), block(64 * kCongWaves);
  switch (nt) {
#define ISD_CONG_CASE(NT) \
  case NT: return launch_lds(spd_congruence_kernel<S, NT>, grid, block, lds, st, cov, W, widx, out, C, K);
    ISD_CONG_CASE(1) ISD_CONG_CASE(2) ISD_CONG_CASE(3) ISD_CONG_CASE(4)
    ISD_CONG_CASE(5) ISD_CONG_CASE(6) ISD_CONG_CASE(7) ISD_CONG_CASE(8)
#undef ISD_CONG_CASE
  }
  return ISD_ERR_UNSUPPORTED;                                    // not reached: 1 <= C <= 128
}

extern "C" int isd_spd_congruence(const void* cov, int cov_f64, const double* W, const int32_t* widx, double* out,
                                  int64_t n, int C, int K, void* stream) {
  ISD_CHECK_ARG(cov && W && out, "isd_spd_congruence: null argument");
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL && C >= 1 && K >= 1, "isd_spd_congruence: n=%lld C=%d K=%d", (long long)n,
                C, K);
  ISD_CHECK_ARG((const void*)out != cov && (const void*)out != (const void*)W,
                "isd_spd_congruence: out is the same buffer as an input");
  if (C > kSpdMaxC) {
    set_error("isd_spd_congruence: C=%d (at most %d channels are provided)", C, kSpdMaxC);
    return ISD_ERR_UNSUPPORTED;
  }
  if (n == 0) return ISD_OK;
  hipStream_t st = (hipStream_t)stream;
  return cov_f64 ? congruence_launch<double>((const double*)cov, W, widx, out, n, C, K, st)
                 : congruence_launch<float>((const float*)cov, W, widx, out, n, C, K, st);
}

template <int L, int NR, int PAIRS>
static int eigfun_launch(const double* a, double* out, double* eigvals, int* info, int64_t n, int C, int fn,
                         int out_kind, hipStream_t st) {
  const size_t lds = ((size_t)C * (C | 1) + 3 * C) * sizeof(double) + (kSpdMaxSweeps + 2) * sizeof(int);   // <= 130 KiB
  return launch_lds(spd_eigfun_kernel<L, NR, PAIRS>, dim3((unsigned)n), dim3(PAIRS * L), lds, st, a, out, eigvals,
                    info, C, fn, out_kind);
}

extern "C" int isd_spd_eigfun(const double* a, double* out, double* eigvals, int32_t* info, int64_t n, int C, int fn,
                              int out_kind, void* stream) {
  ISD_CHECK_ARG(a, "isd_spd_eigfun: null argument");
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL && C >= 1, "isd_spd_eigfun: n=%lld C=%d", (long long)n, C);
  ISD_CHECK_ARG(fn >= ISD_SPD_LOG && fn <= ISD_SPD_NONE, "isd_spd_eigfun: fn=%d", fn);
  ISD_CHECK_ARG(out_kind >= ISD_SPD_FULL && out_kind <= ISD_SPD_NOOUT, "isd_spd_eigfun: out_kind=%d", out_kind);
  ISD_CHECK_ARG(out_kind == ISD_SPD_NOOUT || (out && out != a), "isd_spd_eigfun: out is null or the input buffer");
  if (C > kSpdMaxC) {
    set_error("isd_spd_eigfun: C=%d (at most %d channels are provided)", C, kSpdMaxC);
    return ISD_ERR_UNSUPPORTED;
  }
  if (n == 0) return ISD_OK;
  hipStream_t st = (hipStream_t)stream;
  if (C <= 16) return eigfun_launch<16, 1, 8>(a, out, eigvals, info, n, C, fn, out_kind, st);
  if (C <= 32) return eigfun_launch<16, 2, 16>(a, out, eigvals, info, n, C, fn, out_kind, st);
  if (C <= 64) return eigfun_launch<8, 8, 32>(a, out, eigvals, info, n, C, fn, out_kind, st);
  // eight waves: measured 16 % faster at [2048, 128, 128] than four waves with 4 lanes x 32 rows per pair, which leave
  // one wave per SIMD alone with the latency of its own sqrt / divide chain
  return eigfun_launch<8, 16, 64>(a, out, eigvals, info, n, C, fn, out_kind, st);
}
