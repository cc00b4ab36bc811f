// Expected-gradients attributions (isd_amd.explain.GradientExplainer): the sampling arithmetic around the model's
// forward / backward passes.  Two streaming, HBM-bound kernels:
//   isd_attr_mix         out[q]    = bg[r] + alpha * (x[i] - bg[r])                 one interpolated input per pair
//   isd_attr_accumulate  acc[i]   += (x[i] - bg[r]) * grad[q], sequentially in s     one thread owns an element
// A [C, T] map is a row of E = C*T floats.  E % 4 == 0 is not guaranteed (T = 795 with an odd C), so a row may start
// at any dword: each row is cut into fewer than four leading elements up to the first 16-byte boundary of the row that
// is WRITTEN, a body of 16-byte accesses (aligned stores; the loads of the other rows need dword alignment only on
// gfx950, tools/ubench/unaligned_x4.hip), and fewer than four trailing elements.  The ragged ends are served apart by
// the row's first workgroup; the body has no per-access bounds test.
#include "common.h"

namespace isd {
namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at a dword-aligned address
typedef float f4a __attribute__((ext_vector_type(4)));

template <int W>
struct Pack {
  float v[W];
};
template <int W>
__device__ __forceinline__ Pack<W> ld(const float* p);
template <>
__device__ __forceinline__ Pack<1> ld<1>(const float* p) {
  return {{p[0]}};
}
template <>
__device__ __forceinline__ Pack<4> ld<4>(const float* p) {
  const f4u t = *reinterpret_cast<const f4u*>(p);
  return {{t.x, t.y, t.z, t.w}};
}
// read once, far larger than the caches (the gradient rows): no allocation on the way in
template <int W>
__device__ __forceinline__ Pack<W> ld_stream(const float* p);
template <>
__device__ __forceinline__ Pack<1> ld_stream<1>(const float* p) {
  return {{__builtin_nontemporal_load(p)}};
}
template <>
__device__ __forceinline__ Pack<4> ld_stream<4>(const float* p) {
  const f4u t = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p));
  return {{t.x, t.y, t.z, t.w}};
}
// W == 4: p is 16-byte aligned by construction (the row's leading elements were split off)
template <int W>
__device__ __forceinline__ void st(float* p, const Pack<W>& a);
template <>
__device__ __forceinline__ void st<1>(float* p, const Pack<1>& a) {
  p[0] = a.v[0];
}
template <>
__device__ __forceinline__ void st<4>(float* p, const Pack<4>& a) {
  *reinterpret_cast<f4a*>(p) = (f4a){a.v[0], a.v[1], a.v[2], a.v[3]};
}

// elements in front of the first 16-byte boundary of a row that starts at `row`
__device__ __forceinline__ int row_head(const float* row, int E) {
  const int h = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) >> 2) & 3;
  return h < E ? h : E;
}
// the ragged element thread t of the row's first workgroup serves, or -1: t in [0, head) the leading ones,
// t in [4, 4 + tail) the trailing ones
__device__ __forceinline__ int ragged_element(int t, int head, int nvec, int E) {
  if (t < head) return t;
  const int e = head + 4 * nvec + (t - 4);
  return (t >= 4 && t < 8 && e < E) ? e : -1;
}

// ------------------------------------------------------------------------------------------------ mix
constexpr int kMixThreads = 256, kMixUnroll = 4;        // 1024 vectors = 4096 floats per workgroup

template <int W>
__device__ __forceinline__ Pack<W> mix(const Pack<W>& xv, const Pack<W>& bv, float a) {
  Pack<W> o;
#pragma unroll
  for (int k = 0; k < W; ++k) o.v[k] = fmaf(a, xv.v[k] - bv.v[k], bv.v[k]);
  return o;
}

__global__ __launch_bounds__(kMixThreads) void attr_mix_kernel(const float* __restrict__ x, const float* __restrict__ bg,
                                                               const int* __restrict__ ridx,
                                                               const float* __restrict__ alpha, float* __restrict__ out,
                                                               int64_t pair0, int S, int E, int cpr) {
  const int64_t q = blockIdx.x / cpr;
  const int chunk = blockIdx.x % cpr;
  const int64_t p = pair0 + q;
  const float a = alpha[p];
  const float* xr = x + (p / S) * E;
  const float* br = bg + (int64_t)ridx[p] * E;
  float* orow = out + q * E;
  const int head = row_head(orow, E);
  const int nvec = (E - head) >> 2;
  const int t = threadIdx.x;
  if (chunk == 0) {
    const int e = ragged_element(t, head, nvec, E);
    if (e >= 0) st<1>(orow + e, mix<1>(ld<1>(xr + e), ld<1>(br + e), a));
  }
  const int v0 = chunk * (kMixThreads * kMixUnroll);
  xr += head, br += head, orow += head;
  if (v0 + kMixThreads * kMixUnroll <= nvec) {            // whole chunk: every load first, no bounds test
    Pack<4> xv[kMixUnroll], bv[kMixUnroll];
#pragma unroll
    for (int u = 0; u < kMixUnroll; ++u) {
      const int v = v0 + u * kMixThreads + t;
      xv[u] = ld<4>(xr + 4 * v);
      bv[u] = ld<4>(br + 4 * v);
    }
#pragma unroll
    for (int u = 0; u < kMixUnroll; ++u) st<4>(orow + 4 * (v0 + u * kMixThreads + t), mix<4>(xv[u], bv[u], a));
    return;
  }
  for (int v = v0 + t; v < nvec; v += kMixThreads) st<4>(orow + 4 * v, mix<4>(ld<4>(xr + 4 * v), ld<4>(br + 4 * v), a));
}

// ------------------------------------------------------------------------------------------------ accumulate
// One thread owns W consecutive elements of trial i for every pair of the tile that belongs to i and runs the fma
// chain in s order: the bits do not depend on how the pairs were cut into tiles (acc carries the chain between calls,
// and fp32 in memory is the register's value).  The loads of kAccDepth pairs are issued before the first fma: with one
// chain per element there are only E/4 lanes per trial, so the bytes in flight come from the depth, not the width.
constexpr int kAccThreads = 64, kAccDepth = 8;

template <int W>
__device__ __forceinline__ void acc_chain(const float* __restrict__ xp, const float* __restrict__ bgp,
                                          const float* __restrict__ gp, const int* __restrict__ rp, int ns, int64_t E,
                                          float* __restrict__ ap, bool last, float scale) {
  const Pack<W> xv = ld<W>(xp);
  Pack<W> a = ld<W>(ap);
  int s = 0;
  for (; s + kAccDepth <= ns; s += kAccDepth) {
    Pack<W> b[kAccDepth], g[kAccDepth];
#pragma unroll
    for (int u = 0; u < kAccDepth; ++u) {
      b[u] = ld<W>(bgp + (int64_t)rp[s + u] * E);
      g[u] = ld_stream<W>(gp + (int64_t)(s + u) * E);
    }
#pragma unroll
    for (int u = 0; u < kAccDepth; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) a.v[k] = fmaf(xv.v[k] - b[u].v[k], g[u].v[k], a.v[k]);
  }
  for (; s < ns; ++s) {
    const Pack<W> b = ld<W>(bgp + (int64_t)rp[s] * E), g = ld_stream<W>(gp + (int64_t)s * E);
#pragma unroll
    for (int k = 0; k < W; ++k) a.v[k] = fmaf(xv.v[k] - b.v[k], g.v[k], a.v[k]);
  }
  if (last)                                               // the trial's last pair is in this tile: the mean
#pragma unroll
    for (int k = 0; k < W; ++k) a.v[k] *= scale;
  st<W>(ap, a);
}

__global__ __launch_bounds__(kAccThreads) void attr_acc_kernel(const float* __restrict__ x, const float* __restrict__ bg,
                                                               const int* __restrict__ ridx,
                                                               const float* __restrict__ grad, float* __restrict__ acc,
                                                               int64_t pair0, int64_t n_pairs, int S, int E, int cpr,
                                                               float scale) {
  const int64_t i = pair0 / S + blockIdx.x / cpr;
  const int chunk = blockIdx.x % cpr;
  const int64_t lo = i * S, hi = lo + S, end = pair0 + n_pairs;
  const int64_t pb = lo > pair0 ? lo : pair0, pe = hi < end ? hi : end;    // the trial's pairs inside the tile
  const bool last = pe == hi;
  const int ns = (int)(pe - pb);
  const float* xr = x + i * E;
  float* arow = acc + i * E;
  const float* g0 = grad + (pb - pair0) * E;
  const int* rp = ridx + pb;
  const int head = row_head(arow, E);
  const int nvec = (E - head) >> 2;
  const int t = threadIdx.x;
  if (chunk == 0) {
    const int e = ragged_element(t, head, nvec, E);
    if (e >= 0) acc_chain<1>(xr + e, bg + e, g0 + e, rp, ns, E, arow + e, last, scale);
  }
  const int v = chunk * kAccThreads + t;
  if (v < nvec) {
    const int off = head + 4 * v;
    acc_chain<4>(xr + off, bg + off, g0 + off, rp, ns, E, arow + off, last, scale);
  }
}

int check_common(const char* fn, const void* x, const void* bg, const void* ridx, const void* a, const void* b,
                 int64_t n_pairs, int64_t pair0, int S, int64_t E, int M) {
  ISD_CHECK_ARG(x && bg && ridx && a && b, "%s: null pointer", fn);
  ISD_CHECK_ARG(S >= 1, "%s: bad S=%d (draws per trial, at least 1)", fn, S);
  ISD_CHECK_ARG(E >= 1 && E <= (int64_t)0x7ffffff0, "%s: bad E=%lld (elements per trial)", fn, (long long)E);
  ISD_CHECK_ARG(M >= 1, "%s: bad M=%d (background trials, at least 1)", fn, M);
  ISD_CHECK_ARG(n_pairs >= 0 && pair0 >= 0, "%s: bad tile n_pairs=%lld pair0=%lld", fn, (long long)n_pairs,
                (long long)pair0);
  return ISD_OK;
}

}  // namespace
}  // namespace isd

using namespace isd;

extern "C" int isd_attr_mix(const float* x, const float* bg, const int32_t* ridx, const float* alpha, float* out,
                            int64_t n_pairs, int64_t pair0, int S, int64_t E, int M, void* stream) {
  if (int rc = check_common("isd_attr_mix", x, bg, ridx, alpha, out, n_pairs, pair0, S, E, M)) return rc;
  if (n_pairs == 0) return ISD_OK;
  const int64_t cpr = cdiv(E / 4 > 0 ? E / 4 : 1, kMixThreads * kMixUnroll);
  ISD_CHECK_ARG(n_pairs * cpr <= 0x7fffffff, "isd_attr_mix: tile of %lld pairs is too large for one launch",
                (long long)n_pairs);
  hipLaunchKernelGGL(attr_mix_kernel, dim3((unsigned)(n_pairs * cpr)), dim3(kMixThreads), 0, (hipStream_t)stream, x, bg,
                     ridx, alpha, out, pair0, S, (int)E, (int)cpr);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

extern "C" int isd_attr_accumulate(const float* x, const float* bg, const int32_t* ridx, const float* grad, float* acc,
                                   int64_t n_pairs, int64_t pair0, int S, int64_t E, int M, float scale,
                                   void* stream) {
  if (int rc = check_common("isd_attr_accumulate", x, bg, ridx, grad, acc, n_pairs, pair0, S, E, M)) return rc;
  if (n_pairs == 0) return ISD_OK;
  const int64_t cpr = cdiv(E / 4 > 0 ? E / 4 : 1, kAccThreads);
  const int64_t trials = (pair0 + n_pairs - 1) / S - pair0 / S + 1;
  ISD_CHECK_ARG(trials * cpr <= 0x7fffffff, "isd_attr_accumulate: tile of %lld pairs is too large for one launch",
                (long long)n_pairs);
  hipLaunchKernelGGL(attr_acc_kernel, dim3((unsigned)(trials * cpr)), dim3(kAccThreads), 0, (hipStream_t)stream, x, bg,
                     ridx, grad, acc, pair0, n_pairs, S, (int)E, (int)cpr, scale);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}
