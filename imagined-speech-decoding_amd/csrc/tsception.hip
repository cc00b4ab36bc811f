// TSception (the deep comparison model of the reference's scripts/train_tsception.py), fp32, one device.
//
//   x [B][C][T] -> three banks of temporal filters (k1 > k2 > k3 taps) + bias + LeakyReLU + AvgPool(8), concatenated
//   along time -> BN_t -> Sception1 (all C rows) | Sception2 (two blocks of C/2 rows) + LeakyReLU + AvgPool(2) -> BN_s
//   -> 3-row fusion conv + LeakyReLU + AvgPool(4) -> BN_fusion -> time mean -> Linear + ReLU + Dropout + Linear.
//
// The temporal stage is 97 % of the arithmetic and runs on the fp32 matrix cores (v_mfma_f32_16x16x4_f32): per
// channel row it is the product of the row's Hankel matrix (time x taps, a lane's operand is x[t + k] out of an
// LDS-resident segment) with the filter bank (taps x 16 filters).  Time sits on the M side, so the pool of 8 is three
// in-lane adds and one cross-lane add, and only the pooled map reaches memory.  The backward recomputes the
// pre-activation the same way, forms dz in LDS and contracts it with the same Hankel operand over time
// (filters x time) x (time x taps); neither direction writes an un-pooled tensor.
//
// Sums: BatchNorm statistics, BatchNorm backward sums go through ExactAcc (exact.h); weight-gradient partials are
// written per workgroup / wave and added in a fixed order (ts_reduce).  No floating-point atomics: a step is
// bitwise repeatable.
#include "common.h"
#include "exact.h"

namespace isd {
namespace {


constexpr int kMaxF = 16;        // num_T, num_S (one MFMA N tile)
constexpr int kMaxH = 64;        // hidden
constexpr int kMaxNC = 16;       // classes
constexpr int kMaxTaps = 512;
constexpr int kMaxC = 128;
constexpr int kTP = 256;         // pooled samples per time tile of the temporal kernels (2048 input samples + halo)
constexpr int kXSeg = kTP * 8 + kMaxTaps + 64;
constexpr int kDzStride = 68;    // floats per filter row of a wave's dz tile (64 samples, 16-byte aligned rows)
constexpr float kSlope = 0.01f;
constexpr int kRedGroup = 64;    // rows added by one thread of a reduction stage
constexpr int kMaxBatch = 350;   // trials per pass: the notebook's full batch, the largest the kernels have run at

struct TsScale {
  int k, kpad, Lt, Loff, ntile;
  int woff, boff;                // offsets of this bank's weight / bias in the parameter block
};

struct TsGeo {
  int C, T, F, S, H, NC, Ch;
  int L, L2, L3;
  TsScale sc[3];
  int oS1w, oS1b, oS2w, oS2b, oFw, oFb, oBt, oBs, oBf, oFc0w, oFc0b, oFc3w, oFc3b, n_params;
};

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : kSlope * v; }
__device__ __forceinline__ float lrelu_grad(float v) { return v > 0.f ? 1.f : kSlope; }

// sum over the 64 lanes of a wave in a fixed order (every lane gets it)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// keep / drop of unit j of trial b: splitmix64 of (seed, trial, unit); 1 / (1 - p) when kept
__device__ __forceinline__ float drop_scale(uint64_t seed, int64_t b, int j, float p) {
  if (p <= 0.f) return 1.f;
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(b * kMaxH + j + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(z >> 40) * (1.f / 16777216.f);
  return u >= p ? 1.f / (1.f - p) : 0.f;
}

// ------------------------------------------------------------------ temporal stage
// z[t][f] = sum_k x[t + k] W[f][k] for the 64 samples at xs (4 M tiles of 16): A[i = time][k] = xs[16 m + i + k],
// B[k][j = filter] = Wl[k][j].  acc[m][r]: time 16 m + 4 (lane >> 4) + r, filter lane & 15.
__device__ __forceinline__ void ts_conv_tiles(const float* xs, const float* Wl, int kpad, int lane, f32x4 acc[4]) {
  const int i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xa = xs + q + i;
  const float* wb = Wl + q * 16 + i;
  for (int k0 = 0; k0 < kpad; k0 += 4) {
    const float b = wb[k0 * 16];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k0 + 16 * m], b, acc[m], 0, 0, 0);
  }
}

// filter bank of one scale into LDS as Wl[k][16], zero past the taps and past the filters
__device__ __forceinline__ void ts_load_bank(float* Wl, const float* params, const TsScale& s, int F, int tid) {
  for (int e = tid; e < s.kpad * 16; e += 256) {
    const int k = e >> 4, f = e & 15;
    Wl[e] = (k < s.k && f < F) ? params[s.woff + f * s.k + k] : 0.f;
  }
}

// x[row][t0 ...] into LDS, zero past the row's end
__device__ __forceinline__ void ts_load_seg(float* xs, const float* xrow, int t0, int T, int n, int tid) {
  for (int e = tid; e < n; e += 256) xs[e] = (t0 + e < T) ? xrow[t0 + e] : 0.f;
}

// grid (workgroups, 3 scales), 256 threads; a workgroup walks the items (row, time tile) of its scale
__global__ __launch_bounds__(256) void ts_temporal_fwd(const float* __restrict__ x, const float* __restrict__ params,
                                                       float* __restrict__ P, TsGeo g, int64_t rows) {
  extern __shared__ float lds[];
  const TsScale s = g.sc[blockIdx.y];
  float* Wl = lds;
  float* xs = lds + s.kpad * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  ts_load_bank(Wl, params, s, g.F, tid);
  const float bias = i < g.F ? params[s.boff + i] : 0.f;
  const int64_t items = rows * s.ntile;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t row = item / s.ntile;
    const int p0 = (int)(item % s.ntile) * kTP;
    const int np = min(kTP, s.Lt - p0), nwt = (np + 7) >> 3;
    __syncthreads();
    ts_load_seg(xs, x + row * g.T, p0 * 8, g.T, nwt * 64 + s.kpad + 16, tid);
    __syncthreads();
    const int64_t b = row / g.C;
    const int c = (int)(row % g.C);
    float* prow = P + ((b * g.F + i) * g.C + c) * (int64_t)g.L + s.Loff;
    for (int wt = wave; wt < nwt; wt += 4) {
      f32x4 acc[4];
      ts_conv_tiles(xs + wt * 64, Wl, s.kpad, lane, acc);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float v = lrelu(acc[m][0] + bias) + lrelu(acc[m][1] + bias) + lrelu(acc[m][2] + bias) + lrelu(acc[m][3] + bias);
        v += __shfl_xor(v, 16);
        const int pl = p0 + wt * 8 + m * 2 + (q >> 1);
        if ((q & 1) == 0 && i < g.F && pl < s.Lt) prow[pl] = v * 0.125f;
      }
    }
  }
}

// Weight / bias gradient partials of one scale: part[(workgroup * 4 + wave)][F * k + F].  dp = coef-transformed
// gradient of the pooled map (BN_t backward folded in: dP = cA dPh + cB + cC P).
template <int NT>
__global__ __launch_bounds__(256) void ts_temporal_bwd(const float* __restrict__ x, const float* __restrict__ params,
                                                       const float* __restrict__ P, const float* __restrict__ dPh,
                                                       const float* __restrict__ coef, float* __restrict__ part,
                                                       TsGeo g, int scale, int64_t rows) {
  extern __shared__ float lds[];
  const TsScale s = g.sc[scale];
  float* Wl = lds;
  float* xs = lds + s.kpad * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  float* dzw = xs + kXSeg + wave * (16 * kDzStride);
  ts_load_bank(Wl, params, s, g.F, tid);
  const float bias = i < g.F ? params[s.boff + i] : 0.f;
  const float cA = coef[i], cB = coef[16 + i], cC = coef[32 + i];
  f32x4 dacc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) dacc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbsum = 0.f;
  const int64_t items = rows * s.ntile;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t row = item / s.ntile;
    const int p0 = (int)(item % s.ntile) * kTP;
    const int np = min(kTP, s.Lt - p0), nwt = (np + 7) >> 3;
    __syncthreads();
    ts_load_seg(xs, x + row * g.T, p0 * 8, g.T, nwt * 64 + 16 * NT + 16, tid);
    __syncthreads();
    const int64_t b = row / g.C;
    const int c = (int)(row % g.C);
    const int64_t prow = ((b * g.F + i) * g.C + c) * (int64_t)g.L + s.Loff;
    for (int wt = wave; wt < nwt; wt += 4) {
      f32x4 acc[4];
      ts_conv_tiles(xs + wt * 64, Wl, s.kpad, lane, acc);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int pl = p0 + wt * 8 + m * 2 + (q >> 1);
        float dp = 0.f;
        if (i < g.F && pl < s.Lt) dp = (cA * dPh[prow + pl] + cB + cC * P[prow + pl]) * 0.125f;
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = dp * lrelu_grad(acc[m][r] + bias);
        dbsum += (d[0] + d[1]) + (d[2] + d[3]);
        *(f32x4*)&dzw[i * kDzStride + m * 16 + q * 4] = d;
      }
      wave_lds_sync();
      // dW[f][k] += sum_t dz[f][t] x[t + k]:  A[i = filter][kk = time] = dz,  B[kk = time][j = tap] = x[t + 16 nt + j]
      const float* xb = xs + wt * 64 + q + i;
      for (int kk = 0; kk < 64; kk += 4) {
        const float a = dzw[i * kDzStride + kk + q];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          dacc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[kk + 16 * nt], dacc[nt], 0, 0, 0);
      }
      wave_lds_sync();
    }
  }
  float* out = part + ((int64_t)blockIdx.x * 4 + wave) * (int64_t)(g.F * s.k + g.F);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 4 * q + r, tap = 16 * nt + i;
      if (f < g.F && tap < s.k) out[f * s.k + tap] = dacc[nt][r];
    }
  dbsum += __shfl_xor(dbsum, 16);
  dbsum += __shfl_xor(dbsum, 32);
  if (q == 0 && i < g.F) out[g.F * s.k + i] = dbsum;
}

// ------------------------------------------------------------------ BatchNorm statistics
// in [B][nch][inner]: per-channel sum and sum of squares into acc[ch], acc[16 + ch].  grid (chunks, nch, B).
__global__ __launch_bounds__(256) void ts_chan_stats(const float* __restrict__ in, ExactAcc* acc, int nch, int inner) {
  __shared__ double red[2][4];
  const float* p = in + ((int64_t)blockIdx.z * nch + blockIdx.y) * (int64_t)inner;
  const int lo = blockIdx.x * 4096, hi = min(inner, lo + 4096);
  double s1 = 0., s2 = 0.;
  for (int e = lo + threadIdx.x; e < hi; e += 256) {
    const double v = p[e];
    s1 += v;
    s2 += v * v;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s1;
    red[1][threadIdx.x >> 6] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double t = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
    const float h = (float)t, l = (float)(t - (double)h);
    ExactAcc* a = acc + threadIdx.x * 16 + blockIdx.y;
    exact_add(a, h);
    exact_add(a, l);
  }
}

// coef[0..15] mean, [16..] 1/std, [32..] scale = gamma / std, [48..] shift = beta - mean scale, [64] training flag
__global__ void ts_bn_finalize(const ExactAcc* acc, const float* gamma, const float* beta, float* rmean, float* rvar,
                               float* coef, int nch, double N, int training, float momentum, float eps) {
  const int ch = threadIdx.x;
  if (ch == 0) coef[64] = training ? 1.f : 0.f;
  if (ch >= 16) return;
  float mean = 0.f, istd = 0.f, scale = 0.f, shift = 0.f;
  if (ch < nch) {
    double mu, var;
    if (training) {
      mu = exact_get(acc + ch) / N;
      var = exact_get(acc + 16 + ch) / N - mu * mu;
      if (var < 0.) var = 0.;
      rmean[ch] = (float)((1. - momentum) * rmean[ch] + momentum * mu);
      rvar[ch] = (float)((1. - momentum) * rvar[ch] + momentum * var * (N > 1. ? N / (N - 1.) : 1.));
    } else {
      mu = rmean[ch];
      var = rvar[ch];
    }
    const double is = 1. / sqrt(var + (double)eps);
    mean = (float)mu;
    istd = (float)is;
    scale = (float)(gamma[ch] * is);
    shift = (float)(beta[ch] - mu * gamma[ch] * is);
  }
  coef[ch] = mean;
  coef[16 + ch] = istd;
  coef[32 + ch] = scale;
  coef[48 + ch] = shift;
}

// Backward of one BatchNorm from acc[ch] = sum dy, acc[16 + ch] = sum dy xhat:  dgamma, dbeta, and the coefficients of
// dx = cA dy + cB + cC x  (batch statistics; running statistics: dx = scale dy).
__global__ void ts_bn_bwd_finalize(const ExactAcc* acc, const float* coef, float* bcoef, float* dgamma, float* dbeta,
                                   int nch, double N) {
  const int ch = threadIdx.x;
  if (ch >= 16) return;
  float cA = 0.f, cB = 0.f, cC = 0.f;
  if (ch < nch) {
    const double sdy = exact_get(acc + ch), sdyx = exact_get(acc + 16 + ch);
    dgamma[ch] = (float)sdyx;
    dbeta[ch] = (float)sdy;
    const double mu = coef[ch], is = coef[16 + ch], gs = coef[32 + ch];
    cA = (float)gs;
    if (coef[64] != 0.f) {
      const double m1 = sdy / N, m2 = sdyx / N;
      cB = (float)(-gs * m1 + gs * m2 * is * mu);
      cC = (float)(-gs * m2 * is);
    }
  }
  bcoef[ch] = cA;
  bcoef[16 + ch] = cB;
  bcoef[32 + ch] = cC;
}

// ------------------------------------------------------------------ spatial stage
// Y[b][s][r][t]: r = 0 Sception1 over all C rows, r = 1, 2 Sception2 over rows [0, Ch) and [Ch, 2 Ch); the input is
// BN_t(P) = P scale[f] + shift[f].  One thread per (b, t); the weights are wave-uniform.
__global__ __launch_bounds__(64) void ts_spatial_fwd(const float* __restrict__ P, const float* __restrict__ params,
                                                     const float* __restrict__ coef, float* __restrict__ Y, TsGeo g) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (t >= g.L) return;
  const float* W1 = params + g.oS1w;
  const float* W2 = params + g.oS2w;
  float acc[3][kMaxF];
#pragma unroll
  for (int s = 0; s < kMaxF; ++s) {
    acc[0][s] = s < g.S ? params[g.oS1b + s] : 0.f;
    acc[1][s] = acc[2][s] = s < g.S ? params[g.oS2b + s] : 0.f;
  }
  for (int f = 0; f < g.F; ++f) {
    const float sc = coef[32 + f], sh = coef[48 + f];
    const float* pf = P + ((b * g.F + f) * g.C) * (int64_t)g.L + t;
    for (int c = 0; c < g.C; ++c) {
      const float v = fmaf(pf[(int64_t)c * g.L], sc, sh);
      const int r = c < g.Ch ? 1 : (c < 2 * g.Ch ? 2 : 0);
      const int c2 = c - (r == 2 ? g.Ch : 0);
#pragma unroll
      for (int s = 0; s < kMaxF; ++s)
        if (s < g.S) acc[0][s] = fmaf(W1[(s * g.F + f) * g.C + c], v, acc[0][s]);
      if (r == 1) {
#pragma unroll
        for (int s = 0; s < kMaxF; ++s)
          if (s < g.S) acc[1][s] = fmaf(W2[(s * g.F + f) * g.Ch + c2], v, acc[1][s]);
      } else if (r == 2) {
#pragma unroll
        for (int s = 0; s < kMaxF; ++s)
          if (s < g.S) acc[2][s] = fmaf(W2[(s * g.F + f) * g.Ch + c2], v, acc[2][s]);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kMaxF; ++s)
    if (s < g.S) {
#pragma unroll
      for (int r = 0; r < 3; ++r) Y[((b * g.S + s) * 3 + r) * (int64_t)g.L + t] = acc[r][s];
    }
}

// out[row][j] = mean_u LeakyReLU(in[row][j pool + u]); trailing samples dropped
__global__ void ts_lrelu_pool(const float* __restrict__ in, float* __restrict__ out, int64_t n_out, int Lin, int Lout,
                              int pool) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out) return;
  const int64_t row = e / Lout;
  const int j = (int)(e % Lout);
  const float* p = in + row * Lin + j * pool;
  float v = 0.f;
  for (int u = 0; u < pool; ++u) v += lrelu(p[u]);
  out[e] = v / (float)pool;
}

// U[b][s'][t] = bf[s'] + sum_{s, r} Wf[s'][s][r] BN_s(Q)[b][s][r][t]; one thread per (b, t)
__global__ __launch_bounds__(64) void ts_fusion_fwd(const float* __restrict__ Q, const float* __restrict__ params,
                                                    const float* __restrict__ coef, float* __restrict__ U, TsGeo g) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (t >= g.L2) return;
  const float* Wf = params + g.oFw;
  float acc[kMaxF];
#pragma unroll
  for (int o = 0; o < kMaxF; ++o) acc[o] = o < g.S ? params[g.oFb + o] : 0.f;
  for (int s = 0; s < g.S; ++s) {
    const float sc = coef[32 + s], sh = coef[48 + s];
    for (int r = 0; r < 3; ++r) {
      const float v = fmaf(Q[((b * g.S + s) * 3 + r) * (int64_t)g.L2 + t], sc, sh);
#pragma unroll
      for (int o = 0; o < kMaxF; ++o)
        if (o < g.S) acc[o] = fmaf(Wf[(o * g.S + s) * 3 + r], v, acc[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < kMaxF; ++o)
    if (o < g.S) U[(b * g.S + o) * (int64_t)g.L2 + t] = acc[o];
}

// ------------------------------------------------------------------ head: time mean -> Linear -> ReLU -> Dropout -> Linear
// one thread per trial.  Keeps mV[b][s] (time mean of V) and h[b][j] (after ReLU, before dropout).
__global__ __launch_bounds__(64) void ts_head_fwd(const float* __restrict__ V, const float* __restrict__ params,
                                                  const float* __restrict__ coef, float* __restrict__ mV,
                                                  float* __restrict__ h, float* __restrict__ logits, TsGeo g, int64_t B,
                                                  float p, uint64_t seed) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float m[kMaxF];
#pragma unroll
  for (int s = 0; s < kMaxF; ++s) {
    m[s] = 0.f;
    if (s < g.S) {
      const float* v = V + (b * g.S + s) * (int64_t)g.L3;
      float a = 0.f;
      for (int t = 0; t < g.L3; ++t) a += v[t];
      a /= (float)g.L3;
      mV[b * g.S + s] = a;
      m[s] = fmaf(a, coef[32 + s], coef[48 + s]);
    }
  }
  float lg[kMaxNC];
#pragma unroll
  for (int k = 0; k < kMaxNC; ++k) lg[k] = k < g.NC ? params[g.oFc3b + k] : 0.f;
  for (int j = 0; j < g.H; ++j) {
    float a = params[g.oFc0b + j];
#pragma unroll
    for (int s = 0; s < kMaxF; ++s)
      if (s < g.S) a = fmaf(params[g.oFc0w + j * g.S + s], m[s], a);
    a = fmaxf(a, 0.f);
    h[b * g.H + j] = a;
    const float hd = a * drop_scale(seed, b, j, p);
#pragma unroll
    for (int k = 0; k < kMaxNC; ++k)
      if (k < g.NC) lg[k] = fmaf(params[g.oFc3w + k * g.H + j], hd, lg[k]);
  }
#pragma unroll
  for (int k = 0; k < kMaxNC; ++k)
    if (k < g.NC) logits[b * g.NC + k] = lg[k];
}

// dlogits -> hd (dropped hidden units, for fc.3's gradient), dhp (gradient before the ReLU, for fc.0's), dm (gradient
// of the BN_fusion output's time mean) and BN_fusion's backward sums.
__global__ __launch_bounds__(64) void ts_head_bwd(const float* __restrict__ dlogits, const float* __restrict__ params,
                                                  const float* __restrict__ coef, const float* __restrict__ mV,
                                                  const float* __restrict__ h, float* __restrict__ hd,
                                                  float* __restrict__ dhp, float* __restrict__ dm, ExactAcc* acc,
                                                  TsGeo g, int64_t B, float p, uint64_t seed) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = b < B;
  float dl[kMaxNC], dms[kMaxF];
#pragma unroll
  for (int k = 0; k < kMaxNC; ++k) dl[k] = (live && k < g.NC) ? dlogits[b * g.NC + k] : 0.f;
#pragma unroll
  for (int s = 0; s < kMaxF; ++s) dms[s] = 0.f;
  if (live) {
    for (int j = 0; j < g.H; ++j) {
      const float hv = h[b * g.H + j], ds = drop_scale(seed, b, j, p);
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxNC; ++k)
        if (k < g.NC) a = fmaf(params[g.oFc3w + k * g.H + j], dl[k], a);
      a = hv > 0.f ? a * ds : 0.f;
      hd[b * g.H + j] = hv * ds;
      dhp[b * g.H + j] = a;
#pragma unroll
      for (int s = 0; s < kMaxF; ++s)
        if (s < g.S) dms[s] = fmaf(params[g.oFc0w + j * g.S + s], a, dms[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < kMaxF; ++s) {
    if (s < g.S) {                                                 // (wave-uniform)
      float xh = 0.f;
      if (live) {
        dm[b * g.S + s] = dms[s];
        xh = (mV[b * g.S + s] - coef[s]) * coef[16 + s];
      }
      const float s1 = wave_sum(dms[s]), s2 = wave_sum(dms[s] * xh);
      if (threadIdx.x == 0) {
        exact_add(acc + s, s1);
        exact_add(acc + 16 + s, s2);
      }
    }
  }
}

// dm -> dV (BN_fusion backward) -> dU (pool 4, LeakyReLU) -> dQh = gradient of BN_s's output, with BN_s's backward
// sums.  One thread per (b, t2).
__global__ __launch_bounds__(64) void ts_fusion_bwd(const float* __restrict__ dm, const float* __restrict__ V,
                                                    const float* __restrict__ U, const float* __restrict__ Q,
                                                    const float* __restrict__ params, const float* __restrict__ bcoef_f,
                                                    const float* __restrict__ coef_s, float* __restrict__ dU,
                                                    float* __restrict__ dQh, ExactAcc* acc, TsGeo g) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int64_t b = blockIdx.y;
  const bool live = t < g.L2;
  const float* Wf = params + g.oFw;
  float du[kMaxF];
#pragma unroll
  for (int o = 0; o < kMaxF; ++o) {
    du[o] = 0.f;
    if (o < g.S && live) {
      const int t3 = t >> 2;
      float d = 0.f;
      if (t3 < g.L3) {
        const float dv = bcoef_f[o] * (dm[b * g.S + o] / (float)g.L3) + bcoef_f[16 + o] +
                         bcoef_f[32 + o] * V[(b * g.S + o) * (int64_t)g.L3 + t3];
        d = dv * 0.25f * lrelu_grad(U[(b * g.S + o) * (int64_t)g.L2 + t]);
      }
      du[o] = d;
      dU[(b * g.S + o) * (int64_t)g.L2 + t] = d;
    }
  }
  for (int s = 0; s < g.S; ++s) {
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < 3; ++r) {
      float d = 0.f;
#pragma unroll
      for (int o = 0; o < kMaxF; ++o)
        if (o < g.S) d = fmaf(Wf[(o * g.S + s) * 3 + r], du[o], d);
      if (live) {
        const int64_t idx = ((b * g.S + s) * 3 + r) * (int64_t)g.L2 + t;
        dQh[idx] = d;
        s1 += d;
        s2 += d * ((Q[idx] - coef_s[s]) * coef_s[16 + s]);
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x == 0) {
      exact_add(acc + s, s1);
      exact_add(acc + 16 + s, s2);
    }
  }
}

// dQh -> dQ (BN_s backward) -> dY (pool 2, LeakyReLU) -> dPh = gradient of BN_t's output, with BN_t's backward sums.
// One thread per (b, t).
__global__ __launch_bounds__(64) void ts_spatial_bwd(const float* __restrict__ dQh, const float* __restrict__ Q,
                                                     const float* __restrict__ Y, const float* __restrict__ P,
                                                     const float* __restrict__ params, const float* __restrict__ bcoef_s,
                                                     const float* __restrict__ coef_t, float* __restrict__ dY,
                                                     float* __restrict__ dPh, ExactAcc* acc, TsGeo g) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int64_t b = blockIdx.y;
  const bool live = t < g.L;
  const int tc = live ? t : g.L - 1;
  const float* W1 = params + g.oS1w;
  const float* W2 = params + g.oS2w;
  float dy[3][kMaxF];
#pragma unroll
  for (int s = 0; s < kMaxF; ++s) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float d = 0.f;
      if (s < g.S && live) {
        const int t2 = t >> 1;
        if (t2 < g.L2) {
          const int64_t qi = ((b * g.S + s) * 3 + r) * (int64_t)g.L2 + t2;
          const float dq = bcoef_s[s] * dQh[qi] + bcoef_s[16 + s] + bcoef_s[32 + s] * Q[qi];
          d = dq * 0.5f * lrelu_grad(Y[((b * g.S + s) * 3 + r) * (int64_t)g.L + t]);
        }
        dY[((b * g.S + s) * 3 + r) * (int64_t)g.L + t] = d;
      }
      dy[r][s] = d;
    }
  }
  for (int f = 0; f < g.F; ++f) {
    const float mu = coef_t[f], is = coef_t[16 + f];
    const int64_t base = ((b * g.F + f) * g.C) * (int64_t)g.L + tc;
    float s1 = 0.f, s2 = 0.f;
    for (int c = 0; c < g.C; ++c) {
      const int r = c < g.Ch ? 1 : (c < 2 * g.Ch ? 2 : 0);
      const int c2 = c - (r == 2 ? g.Ch : 0);
      float d = 0.f;
#pragma unroll
      for (int s = 0; s < kMaxF; ++s)
        if (s < g.S) d = fmaf(W1[(s * g.F + f) * g.C + c], dy[0][s], d);
      if (r == 1) {
#pragma unroll
        for (int s = 0; s < kMaxF; ++s)
          if (s < g.S) d = fmaf(W2[(s * g.F + f) * g.Ch + c2], dy[1][s], d);
      } else if (r == 2) {
#pragma unroll
        for (int s = 0; s < kMaxF; ++s)
          if (s < g.S) d = fmaf(W2[(s * g.F + f) * g.Ch + c2], dy[2][s], d);
      }
      if (live) {
        const int64_t idx = base + (int64_t)c * g.L;
        dPh[idx] = d;
        s1 += d;
        s2 += d * ((P[idx] - mu) * is);
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x == 0) {
      exact_add(acc + f, s1);
      exact_add(acc + 16 + f, s2);
    }
  }
}

// Spatial weight-gradient partials.  grid (channel tiles of 64, F, trial chunks), one wave: lane = channel.
// part[chunk]: G1[s][f][c] (Sception1) | G2[s][f][c] (Sception2, still indexed by the input row c) | sums of dY [3][16].
__global__ __launch_bounds__(64) void ts_spatial_dw(const float* __restrict__ P, const float* __restrict__ dY,
                                                    const float* __restrict__ coef_t, float* __restrict__ part, TsGeo g,
                                                    int64_t B, int chunk) {
  __shared__ float Pt[64][65];
  __shared__ __attribute__((aligned(16))) float dYt[64][48];
  const int lane = threadIdx.x, f = blockIdx.y, c0 = blockIdx.x * 64, c = c0 + lane;
  const int r2 = c < g.Ch ? 1 : 2;
  const float sc = coef_t[32 + f], sh = coef_t[48 + f];
  const int64_t nW = (int64_t)g.S * g.F * g.C;
  float a0[kMaxF], a1[kMaxF];
#pragma unroll
  for (int s = 0; s < kMaxF; ++s) a0[s] = a1[s] = 0.f;
  float bs = 0.f;
  const int64_t b_lo = (int64_t)blockIdx.z * chunk, b_hi = min(B, b_lo + chunk);
  for (int64_t b = b_lo; b < b_hi; ++b)
    for (int t0 = 0; t0 < g.L; t0 += 64) {
      const int t = t0 + lane;
      for (int cc = 0; cc < 64; ++cc) {
        float v = 0.f;
        if (t < g.L && c0 + cc < g.C) v = fmaf(P[((b * g.F + f) * g.C + c0 + cc) * (int64_t)g.L + t], sc, sh);
        Pt[cc][lane] = v;
      }
      for (int e = 0; e < 48; ++e) {
        const int r = e >> 4, s = e & 15;
        dYt[lane][e] = (t < g.L && s < g.S) ? dY[((b * g.S + s) * 3 + r) * (int64_t)g.L + t] : 0.f;
      }
      wave_lds_sync();
      for (int tt = 0; tt < 64; ++tt) {
        const float p = Pt[lane][tt];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const f32x4 d0 = *(const f32x4*)&dYt[tt][s4 * 4];
          const f32x4 d1 = *(const f32x4*)&dYt[tt][r2 * 16 + s4 * 4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            a0[s4 * 4 + u] = fmaf(d0[u], p, a0[s4 * 4 + u]);
            a1[s4 * 4 + u] = fmaf(d1[u], p, a1[s4 * 4 + u]);
          }
        }
        if (lane < 48) bs += dYt[tt][lane];
      }
      wave_lds_sync();
    }
  float* out = part + (int64_t)blockIdx.z * (2 * nW + 48);
  if (c < g.C) {
#pragma unroll
    for (int s = 0; s < kMaxF; ++s)
      if (s < g.S) {
        out[((int64_t)s * g.F + f) * g.C + c] = a0[s];
        out[nW + ((int64_t)s * g.F + f) * g.C + c] = c < 2 * g.Ch ? a1[s] : 0.f;
      }
  }
  if (blockIdx.x == 0 && f == 0 && lane < 48) out[2 * nW + lane] = bs;
}

// gsp (ts_spatial_dw's layout, summed over the chunks) -> dS1.w | dS1.b | dS2.w | dS2.b in the parameter block
__global__ void ts_spatial_merge(const float* __restrict__ gsp, float* __restrict__ dparams, TsGeo g) {
  const int64_t nW = (int64_t)g.S * g.F * g.C, nW2 = (int64_t)g.S * g.F * g.Ch;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nW) dparams[g.oS1w + e] = gsp[e];
  if (e < nW2) {
    const int64_t sf = e / g.Ch;
    const int c2 = (int)(e % g.Ch);
    dparams[g.oS2w + e] = gsp[nW + sf * g.C + c2] + gsp[nW + sf * g.C + g.Ch + c2];
  }
  if (e < g.S) {
    dparams[g.oS1b + e] = gsp[2 * nW + e];
    dparams[g.oS2b + e] = gsp[2 * nW + 16 + e] + gsp[2 * nW + 32 + e];
  }
}

// Small weight gradients:  G[i][j] = sum_b sum_{t < Tn} A[b sAb + i sAi + t] Bv[b][j][t],  Bv = Bm[b sBb + j sBj + t]
// (scale[j / jdiv] and shift[j / jdiv] applied when given), and the bias gradient G[i][J] = sum A.  One thread per
// element, grid (elements / 256, trial chunks); part[chunk]: weight [I][J] | bias [I].
__global__ void ts_outer(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ coef,
                         int jdiv, int I, int J, int Tn, int64_t sAb, int64_t sAi, int64_t sBb, int64_t sBj, int64_t B,
                         int chunk, float* __restrict__ part) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= I * (J + 1)) return;
  const int i = e / (J + 1), j = e % (J + 1);
  float sc = 1.f, sh = 0.f;
  if (coef && j < J) {
    sc = coef[32 + j / jdiv];
    sh = coef[48 + j / jdiv];
  }
  const int64_t b_lo = (int64_t)blockIdx.y * chunk, b_hi = min(B, b_lo + chunk);
  float acc = 0.f;
  for (int64_t b = b_lo; b < b_hi; ++b) {
    const float* a = A + b * sAb + i * sAi;
    if (j < J) {
      const float* bm = Bm + b * sBb + j * sBj;
      for (int t = 0; t < Tn; ++t) acc = fmaf(a[t], fmaf(bm[t], sc, sh), acc);
    } else {
      for (int t = 0; t < Tn; ++t) acc += a[t];
    }
  }
  part[(int64_t)blockIdx.y * (I * J + I) + (j < J ? i * J + j : I * J + i)] = acc;
}

// One stage of the fixed-order sum over partial rows: dst[grp][j] = sum of kRedGroup consecutive rows of src.
struct TsRedEntry {
  const float* src;
  float* dst;
  int rows, n;
};
struct TsRedTable {
  TsRedEntry e[8];
};
__global__ void ts_reduce(TsRedTable tab) {
  const TsRedEntry e = tab.e[blockIdx.z];
  const int grp = blockIdx.y;
  const int r_lo = grp * kRedGroup, r_hi = min(e.rows, r_lo + kRedGroup);
  if (r_lo >= e.rows) return;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < e.n; j += gridDim.x * 256) {
    double s = 0.;
    for (int r = r_lo; r < r_hi; ++r) s += (double)e.src[(int64_t)r * e.n + j];
    e.dst[(int64_t)grp * e.n + j] = (float)s;
  }
}

// ------------------------------------------------------------------ workspace
struct TsWs {
  int64_t acc, coef, P, Y, Q, U, V, mV, h, hd, dhp, dm, dU, dQh, dY, dPh, partT[3], partS, gsp, partF, part0, part3,
      red, total;                                                  // float offsets
  int nblkT[3], chunkS, nchunkS, chunkO, nchunkO;
};
constexpr int kAccFwd = 3 * 32, kAccAll = 6 * 32;                   // ExactAcc: per BatchNorm 16 + 16, forward then backward
constexpr int kCoefStride = 80;                                    // floats per coefficient block (65 used)

TsWs ts_layout(const TsGeo& g, int64_t B) {
  TsWs w;
  WorkCarver c;
  auto take = [&](int64_t n) { return c.take(n, 64); };           // every region on a 256-byte line
  w.acc = take((int64_t)kAccAll * (sizeof(ExactAcc) / 4));
  w.coef = take(6 * kCoefStride);                                  // BN_t, BN_s, BN_f forward; then backward
  w.P = take(B * g.F * g.C * g.L);
  w.Y = take(B * g.S * 3 * g.L);
  w.Q = take(B * g.S * 3 * g.L2);
  w.U = take(B * g.S * g.L2);
  w.V = take(B * g.S * g.L3);
  w.mV = take(B * g.S);
  w.h = take(B * g.H);
  w.hd = take(B * g.H);
  w.dhp = take(B * g.H);
  w.dm = take(B * g.S);
  w.dU = take(B * g.S * g.L2);
  w.dQh = take(B * g.S * 3 * g.L2);
  w.dY = take(B * g.S * 3 * g.L);
  w.dPh = take(B * g.F * g.C * g.L);
  int64_t red = 0;
  for (int s = 0; s < 3; ++s) {
    const int64_t items = B * g.C * g.sc[s].ntile;
    w.nblkT[s] = (int)(items < 512 ? items : 512);
    const int64_t n = g.F * g.sc[s].k + g.F;
    w.partT[s] = take((int64_t)w.nblkT[s] * 4 * n);
    red += cdiv(w.nblkT[s] * 4, kRedGroup) * n;
  }
  w.chunkS = (int)cdiv(B, 64);
  w.nchunkS = (int)cdiv(B, w.chunkS);
  const int64_t nS = 2 * (int64_t)g.S * g.F * g.C + 48;
  w.partS = take(w.nchunkS * nS);
  w.gsp = take(nS);
  w.chunkO = w.chunkS;
  w.nchunkO = w.nchunkS;
  const int64_t nF = g.S * g.S * 3 + g.S, n0 = g.H * g.S + g.H, n3 = g.NC * g.H + g.NC;
  w.partF = take(w.nchunkO * nF);
  w.part0 = take(w.nchunkO * n0);
  w.part3 = take(w.nchunkO * n3);
  red += nS + nF + n0 + n3;                                        // at most kRedGroup chunks: one row each
  w.red = take(red);
  take(0);                                                         // the size counts whole lines
  w.total = c.end;
  return w;
}

int ts_check_pointers(const char* fn, const isd_tsception_plan* plan, const void* a, const void* b, const void* c,
                      const void* d, int64_t B) {
  if (zone_batch_open()) {
    set_error("%s: TSception is one network on the whole montage; its calls cannot be recorded into a zone batch", fn);
    return ISD_ERR_UNSUPPORTED;
  }
  ISD_CHECK_ARG(plan && a && b && c && d, "%s: null argument", fn);
  ISD_CHECK_ARG(B >= 1 && B <= kMaxBatch, "%s: B=%lld not in [1, %d] (split a larger batch)", fn, (long long)B,
                kMaxBatch);
  return ISD_OK;
}

}  // namespace
}  // namespace isd

using namespace isd;

struct isd_tsception_plan {
  TsGeo g;
  int n_bufs;
};

extern "C" int isd_tsception_plan_create(isd_tsception_plan** out, int in_channels, int T, int k1, int k2, int k3,
                                         int num_T, int num_S, int hidden, int n_classes) {
  const char* fn = "isd_tsception_plan_create";
  ISD_CHECK_ARG(out, "%s: null argument", fn);
  *out = nullptr;
  ISD_CHECK_ARG(in_channels >= 2 && in_channels <= kMaxC && in_channels != 3,
                "%s: in_channels=%d not in [2, %d] or 3 (Sception2 must yield exactly two rows)", fn, in_channels, kMaxC);
  const int k[3] = {k1, k2, k3};
  for (int s = 0; s < 3; ++s)
    ISD_CHECK_ARG(k[s] >= 1 && k[s] <= kMaxTaps, "%s: %d taps in bank %d, not in [1, %d]", fn, k[s], s + 1, kMaxTaps);
  ISD_CHECK_ARG(num_T >= 1 && num_T <= kMaxF, "%s: num_T=%d not in [1, %d]", fn, num_T, kMaxF);
  ISD_CHECK_ARG(num_S >= 1 && num_S <= kMaxF, "%s: num_S=%d not in [1, %d]", fn, num_S, kMaxF);
  ISD_CHECK_ARG(hidden >= 1 && hidden <= kMaxH, "%s: hidden=%d not in [1, %d]", fn, hidden, kMaxH);
  ISD_CHECK_ARG(n_classes >= 1 && n_classes <= kMaxNC, "%s: n_classes=%d not in [1, %d]", fn, n_classes, kMaxNC);
  ISD_CHECK_ARG(T >= 1 && T <= (1 << 24), "%s: T=%d not in [1, 2^24]", fn, T);
  TsGeo g{};
  g.C = in_channels; g.T = T; g.F = num_T; g.S = num_S; g.H = hidden; g.NC = n_classes; g.Ch = in_channels / 2;
  int o = 0, L = 0;
  for (int s = 0; s < 3; ++s) {
    TsScale& sc = g.sc[s];
    sc.k = k[s];
    sc.kpad = (k[s] + 3) / 4 * 4;
    sc.Lt = T - k[s] + 1 >= 8 ? (T - k[s] + 1) / 8 : 0;
    ISD_CHECK_ARG(sc.Lt >= 1, "%s: T=%d leaves fewer than 8 valid samples for the %d-tap bank", fn, T, k[s]);
    sc.Loff = L;
    L += sc.Lt;
    sc.ntile = (sc.Lt + kTP - 1) / kTP;
    sc.woff = o; o += num_T * k[s];
    sc.boff = o; o += num_T;
  }
  g.L = L; g.L2 = L / 2; g.L3 = g.L2 / 4;
  ISD_CHECK_ARG(g.L3 >= 1, "%s: T=%d pools to %d samples, too short for AvgPool(2) and the fusion layer's AvgPool(4)",
                fn, T, L);
  g.oS1w = o; o += num_S * num_T * g.C;
  g.oS1b = o; o += num_S;
  g.oS2w = o; o += num_S * num_T * g.Ch;
  g.oS2b = o; o += num_S;
  g.oFw = o; o += num_S * num_S * 3;
  g.oFb = o; o += num_S;
  g.oBt = o; o += 2 * num_T;
  g.oBs = o; o += 2 * num_S;
  g.oBf = o; o += 2 * num_S;
  g.oFc0w = o; o += hidden * num_S;
  g.oFc0b = o; o += hidden;
  g.oFc3w = o; o += n_classes * hidden;
  g.oFc3b = o; o += n_classes;
  g.n_params = o;
  isd_tsception_plan* p = new isd_tsception_plan();
  p->g = g;
  p->n_bufs = 2 * num_T + 4 * num_S;
  *out = p;
  return ISD_OK;
}

extern "C" int isd_tsception_plan_destroy(isd_tsception_plan* p) {
  delete p;
  return ISD_OK;
}
extern "C" int64_t isd_tsception_param_count(const isd_tsception_plan* p) { return p ? p->g.n_params : ISD_ERR_INVALID; }
extern "C" int64_t isd_tsception_buffer_count(const isd_tsception_plan* p) { return p ? p->n_bufs : ISD_ERR_INVALID; }
extern "C" int64_t isd_tsception_workspace_bytes(const isd_tsception_plan* p, int64_t B) {
  if (!p || B < 1 || B > kMaxBatch) {
    set_error("isd_tsception_workspace_bytes: B=%lld not in [1, %d] (split a larger batch)", (long long)B, kMaxBatch);
    return ISD_ERR_INVALID;
  }
  return ts_layout(p->g, B).total * 4;
}

namespace {

int ts_stats(const float* in, ExactAcc* acc, int nch, int64_t inner, int64_t B, hipStream_t st) {
  hipLaunchKernelGGL(ts_chan_stats, dim3((unsigned)cdiv(inner, 4096), nch, (unsigned)B), dim3(256), 0, st, in, acc, nch,
                     (int)inner);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

int ts_launch_temporal_fwd(const TsGeo& g, const TsWs& w, const float* x, const float* params, float* ws, int64_t B,
                           hipStream_t st) {
  int kmax = 0;
  int64_t imax = 0;
  for (int s = 0; s < 3; ++s) {
    kmax = g.sc[s].kpad > kmax ? g.sc[s].kpad : kmax;
    const int64_t it = B * g.C * g.sc[s].ntile;
    imax = it > imax ? it : imax;
  }
  return launch_lds(ts_temporal_fwd, dim3((unsigned)(imax < 2048 ? imax : 2048), 3), dim3(256),
                    (size_t)(kmax * 16 + kXSeg) * 4, st, x, params, ws + w.P, g, B * g.C);
}

template <int NT>
int ts_launch_temporal_bwd(const TsGeo& g, const TsWs& w, int s, const float* x, const float* params, float* ws,
                           int64_t B, hipStream_t st) {
  const size_t lds = (size_t)(g.sc[s].kpad * 16 + kXSeg + 4 * 16 * kDzStride) * 4;
  return launch_lds(ts_temporal_bwd<NT>, dim3(w.nblkT[s]), dim3(256), lds, st, x, params, (const float*)(ws + w.P),
                    (const float*)(ws + w.dPh), (const float*)(ws + w.coef + 3 * kCoefStride), ws + w.partT[s], g, s,
                    B * g.C);
}

// the three banks' weight-gradient kernels, each with the smallest tap-tile count that holds its taps
int ts_launch_temporal_bwd_all(const TsGeo& g, const TsWs& w, const float* x, const float* params, float* ws, int64_t B,
                               hipStream_t st) {
  for (int s = 0; s < 3; ++s) {
    const int nt = (g.sc[s].k + 15) / 16;
    int rc;
    if (nt <= 2) rc = ts_launch_temporal_bwd<2>(g, w, s, x, params, ws, B, st);
    else if (nt <= 4) rc = ts_launch_temporal_bwd<4>(g, w, s, x, params, ws, B, st);
    else if (nt <= 8) rc = ts_launch_temporal_bwd<8>(g, w, s, x, params, ws, B, st);
    else if (nt <= 16) rc = ts_launch_temporal_bwd<16>(g, w, s, x, params, ws, B, st);
    else rc = ts_launch_temporal_bwd<32>(g, w, s, x, params, ws, B, st);
    if (rc != ISD_OK) return rc;
  }
  return ISD_OK;
}

}  // namespace

extern "C" int isd_tsception_temporal_probe(const isd_tsception_plan* plan, const float* x, const float* params,
                                            void* workspace, int64_t B, int backward, void* stream) {
  int rc = ts_check_pointers("isd_tsception_temporal_probe", plan, x, params, workspace, workspace, B);
  if (rc != ISD_OK) return rc;
  const TsGeo& g = plan->g;
  const TsWs w = ts_layout(g, B);
  return backward ? ts_launch_temporal_bwd_all(g, w, x, params, (float*)workspace, B, (hipStream_t)stream)
                  : ts_launch_temporal_fwd(g, w, x, params, (float*)workspace, B, (hipStream_t)stream);
}

extern "C" int isd_tsception_forward(const isd_tsception_plan* plan, const float* x, const float* params,
                                     float* buffers, float* logits, void* workspace, int64_t B, int training,
                                     float momentum, float eps, float dropout_p, uint64_t seed, void* stream) {
  int rc = ts_check_pointers("isd_tsception_forward", plan, x, params, buffers, logits, B);
  if (rc != ISD_OK) return rc;
  ISD_CHECK_ARG(workspace, "isd_tsception_forward: null workspace");
  ISD_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "isd_tsception_forward: dropout_p=%g not in [0, 1)", dropout_p);
  const TsGeo& g = plan->g;
  const TsWs w = ts_layout(g, B);
  ISD_CHECK_ARG(B * g.F * g.C * (int64_t)g.L < (1ll << 40), "isd_tsception_forward: batch too large");
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  ExactAcc* acc = (ExactAcc*)(ws + w.acc);
  float* coef = ws + w.coef;
  float* rb = buffers;                                             // BN_t mean, var | BN_s mean, var | BN_f mean, var
  if (training) ISD_HIP_TRY(hipMemsetAsync(acc, 0, kAccFwd * sizeof(ExactAcc), st));
  if ((rc = ts_launch_temporal_fwd(g, w, x, params, ws, B, st)) != ISD_OK) return rc;
  if (training && (rc = ts_stats(ws + w.P, acc, g.F, (int64_t)g.C * g.L, B, st)) != ISD_OK) return rc;
  hipLaunchKernelGGL(ts_bn_finalize, dim3(1), dim3(64), 0, st, acc, params + g.oBt, params + g.oBt + g.F, rb, rb + g.F,
                     coef, g.F, (double)B * g.C * g.L, training, momentum, eps);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_spatial_fwd, dim3((unsigned)cdiv(g.L, 64), (unsigned)B), dim3(64), 0, st,
                     (const float*)(ws + w.P), params, (const float*)coef, ws + w.Y, g);
  ISD_LAUNCH_CHECK();
  const int64_t nQ = B * g.S * 3 * g.L2;
  hipLaunchKernelGGL(ts_lrelu_pool, dim3((unsigned)cdiv(nQ, 256)), dim3(256), 0, st, (const float*)(ws + w.Y), ws + w.Q,
                     nQ, g.L, g.L2, 2);
  ISD_LAUNCH_CHECK();
  if (training && (rc = ts_stats(ws + w.Q, acc + 32, g.S, 3 * (int64_t)g.L2, B, st)) != ISD_OK) return rc;
  rb += 2 * g.F;
  hipLaunchKernelGGL(ts_bn_finalize, dim3(1), dim3(64), 0, st, acc + 32, params + g.oBs, params + g.oBs + g.S, rb,
                     rb + g.S, coef + kCoefStride, g.S, (double)B * 3 * g.L2, training, momentum, eps);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_fusion_fwd, dim3((unsigned)cdiv(g.L2, 64), (unsigned)B), dim3(64), 0, st,
                     (const float*)(ws + w.Q), params, (const float*)(coef + kCoefStride), ws + w.U, g);
  ISD_LAUNCH_CHECK();
  const int64_t nV = B * g.S * g.L3;
  hipLaunchKernelGGL(ts_lrelu_pool, dim3((unsigned)cdiv(nV, 256)), dim3(256), 0, st, (const float*)(ws + w.U), ws + w.V,
                     nV, g.L2, g.L3, 4);
  ISD_LAUNCH_CHECK();
  if (training && (rc = ts_stats(ws + w.V, acc + 64, g.S, g.L3, B, st)) != ISD_OK) return rc;
  rb += 2 * g.S;
  hipLaunchKernelGGL(ts_bn_finalize, dim3(1), dim3(64), 0, st, acc + 64, params + g.oBf, params + g.oBf + g.S, rb,
                     rb + g.S, coef + 2 * kCoefStride, g.S, (double)B * g.L3, training, momentum, eps);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_head_fwd, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, (const float*)(ws + w.V), params,
                     (const float*)(coef + 2 * kCoefStride), ws + w.mV, ws + w.h, logits, g, B,
                     training ? dropout_p : 0.f, seed);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

extern "C" int isd_tsception_backward(const isd_tsception_plan* plan, const float* x, const float* params,
                                      const float* dlogits, float* dparams, void* workspace, int64_t B, float dropout_p,
                                      uint64_t seed, void* stream) {
  int rc = ts_check_pointers("isd_tsception_backward", plan, x, params, dlogits, dparams, B);
  if (rc != ISD_OK) return rc;
  ISD_CHECK_ARG(workspace, "isd_tsception_backward: null workspace");
  ISD_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "isd_tsception_backward: dropout_p=%g not in [0, 1)", dropout_p);
  const TsGeo& g = plan->g;
  const TsWs w = ts_layout(g, B);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  ExactAcc* acc = (ExactAcc*)(ws + w.acc) + kAccFwd;               // BN_t, BN_s, BN_f backward sums
  const float* coef = ws + w.coef;
  float* bcoef = ws + w.coef + 3 * kCoefStride;
  ISD_HIP_TRY(hipMemsetAsync(acc, 0, (kAccAll - kAccFwd) * sizeof(ExactAcc), st));
  const dim3 gO0((unsigned)cdiv(g.H * (g.S + 1), 256), w.nchunkO), gO3((unsigned)cdiv(g.NC * (g.H + 1), 256), w.nchunkO),
      gOF((unsigned)cdiv(g.S * (3 * g.S + 1), 256), w.nchunkO);

  hipLaunchKernelGGL(ts_head_bwd, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, dlogits, params,
                     coef + 2 * kCoefStride, (const float*)(ws + w.mV), (const float*)(ws + w.h), ws + w.hd, ws + w.dhp,
                     ws + w.dm, acc + 64, g, B, dropout_p, seed);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_outer, gO3, dim3(256), 0, st, dlogits, (const float*)(ws + w.hd), (const float*)nullptr, 1, g.NC,
                     g.H, 1, (int64_t)g.NC, (int64_t)1, (int64_t)g.H, (int64_t)1, B, w.chunkO, ws + w.part3);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_outer, gO0, dim3(256), 0, st, (const float*)(ws + w.dhp), (const float*)(ws + w.mV),
                     coef + 2 * kCoefStride, 1, g.H, g.S, 1, (int64_t)g.H, (int64_t)1, (int64_t)g.S, (int64_t)1, B,
                     w.chunkO, ws + w.part0);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_bn_bwd_finalize, dim3(1), dim3(64), 0, st, (const ExactAcc*)(acc + 64), coef + 2 * kCoefStride,
                     bcoef + 2 * kCoefStride, dparams + g.oBf, dparams + g.oBf + g.S, g.S, (double)B * g.L3);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_fusion_bwd, dim3((unsigned)cdiv(g.L2, 64), (unsigned)B), dim3(64), 0, st,
                     (const float*)(ws + w.dm), (const float*)(ws + w.V), (const float*)(ws + w.U),
                     (const float*)(ws + w.Q), params, (const float*)(bcoef + 2 * kCoefStride), coef + kCoefStride,
                     ws + w.dU, ws + w.dQh, acc + 32, g);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_outer, gOF, dim3(256), 0, st, (const float*)(ws + w.dU), (const float*)(ws + w.Q),
                     coef + kCoefStride, 3, g.S, 3 * g.S, g.L2, (int64_t)g.S * g.L2, (int64_t)g.L2,
                     (int64_t)3 * g.S * g.L2, (int64_t)g.L2, B, w.chunkO, ws + w.partF);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_bn_bwd_finalize, dim3(1), dim3(64), 0, st, (const ExactAcc*)(acc + 32), coef + kCoefStride,
                     bcoef + kCoefStride, dparams + g.oBs, dparams + g.oBs + g.S, g.S, (double)B * 3 * g.L2);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_spatial_bwd, dim3((unsigned)cdiv(g.L, 64), (unsigned)B), dim3(64), 0, st,
                     (const float*)(ws + w.dQh), (const float*)(ws + w.Q), (const float*)(ws + w.Y),
                     (const float*)(ws + w.P), params, (const float*)(bcoef + kCoefStride), coef, ws + w.dY, ws + w.dPh,
                     acc, g);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_spatial_dw, dim3((unsigned)cdiv(g.C, 64), g.F, w.nchunkS), dim3(64), 0, st,
                     (const float*)(ws + w.P), (const float*)(ws + w.dY), coef, ws + w.partS, g, B, w.chunkS);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_bn_bwd_finalize, dim3(1), dim3(64), 0, st, (const ExactAcc*)acc, coef, bcoef, dparams + g.oBt,
                     dparams + g.oBt + g.F, g.F, (double)B * g.C * g.L);
  ISD_LAUNCH_CHECK();
  if ((rc = ts_launch_temporal_bwd_all(g, w, x, params, ws, B, st)) != ISD_OK) return rc;
  // fixed-order sums of the partial rows: groups of kRedGroup rows, then the group sums
  TsRedTable t1{}, t2{};
  const int64_t nS = 2 * (int64_t)g.S * g.F * g.C + 48;
  const int nF = g.S * g.S * 3 + g.S, n0 = g.H * g.S + g.H, n3 = g.NC * g.H + g.NC;
  float* red = ws + w.red;
  int nmax = 0, gmax = 1;
  for (int s = 0; s < 3; ++s) {
    const int n = g.F * g.sc[s].k + g.F, rows = w.nblkT[s] * 4, grp = (int)cdiv(rows, kRedGroup);
    t1.e[s] = {ws + w.partT[s], red, rows, n};
    t2.e[s] = {red, dparams + g.sc[s].woff, grp, n};
    red += (int64_t)grp * n;
    nmax = n > nmax ? n : nmax;
    gmax = grp > gmax ? grp : gmax;
  }
  const TsRedEntry small[4] = {{ws + w.partS, ws + w.gsp, w.nchunkS, (int)nS},
                               {ws + w.partF, dparams + g.oFw, w.nchunkO, nF},
                               {ws + w.part0, dparams + g.oFc0w, w.nchunkO, n0},
                               {ws + w.part3, dparams + g.oFc3w, w.nchunkO, n3}};
  for (int i = 0; i < 4; ++i) {
    t1.e[3 + i] = small[i];                                         // at most kRedGroup rows: one stage
    nmax = small[i].n > nmax ? small[i].n : nmax;
  }
  const unsigned gx = (unsigned)(cdiv(nmax, 256) < 64 ? cdiv(nmax, 256) : 64);
  hipLaunchKernelGGL(ts_reduce, dim3(gx, gmax, 7), dim3(256), 0, st, t1);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_reduce, dim3(gx, 1, 3), dim3(256), 0, st, t2);
  ISD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_spatial_merge, dim3((unsigned)cdiv((int64_t)g.S * g.F * g.C, 256)), dim3(256), 0, st,
                     (const float*)(ws + w.gsp), dparams, g);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}
