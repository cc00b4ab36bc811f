// Shared host/device helpers for libisd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <vector>
#include "../../include/isd_hip.h"

namespace isd {

void set_error(const char* fmt, ...);
bool zone_batch_open();             // a zone batch is recording on this thread (zonebatch.hip)

#define ISD_CHECK_ARG(cond, ...)                 \
  do {                                           \
    if (!(cond)) {                               \
      isd::set_error(__VA_ARGS__);               \
      return ISD_ERR_INVALID;                    \
    }                                            \
  } while (0)

// a well-formed request that the kernels do not cover
#define ISD_CHECK_SUPPORTED(cond, ...)           \
  do {                                           \
    if (!(cond)) {                               \
      isd::set_error(__VA_ARGS__);               \
      return ISD_ERR_UNSUPPORTED;                \
    }                                            \
  } while (0)

#define ISD_HIP_TRY(expr)                                                         \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      isd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                     __FILE__, __LINE__);                                         \
      return ISD_ERR_HIP;                                                         \
    }                                                                             \
  } while (0)

// checks the launch that was just enqueued (no host sync)
#define ISD_LAUNCH_CHECK() ISD_HIP_TRY(hipGetLastError())

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

#if defined(__HIPCC__)
#define ISD_HOST_DEVICE __host__ __device__
#else
#define ISD_HOST_DEVICE
#endif

// Carver hands out the regions of one allocation front to back: a region starts where the one before it ended, rounded
// up to `align` (a power of two), so two regions cannot overlap, and slack is a `take` of its own.  It counts whatever
// unit its caller counts.  Every allocation with more than one region has ONE `*_layout` function that carves it: the
// size that is asked for is that function's `end`, and every pointer into the allocation comes from the same struct.
//   LdsCarver   dynamic LDS of a kernel (conv.hip): floats; the kernel and its host launch share the constexpr layout
//   WorkCarver  a global workspace, host side: floats with align = 64 in the heads and conv.hip, bytes with
//               align = 256 in the signal transforms.  The size query (`*_work_bytes`, `*_workspace_bytes`) returns
//               `end`; the launch, which receives a bare pointer, addresses nothing else.
template <typename I>
struct Carver {
  I end = 0;
  ISD_HOST_DEVICE constexpr I take(I n, I align = 1) {
    const I at = (end + align - 1) & ~(align - 1);
    end = at + n;
    return at;
  }
};
using LdsCarver = Carver<int>;
using WorkCarver = Carver<int64_t>;

constexpr bool work_carver_ok() {   // disjoint, aligned, `end` as expected; empty regions take no room; 64-bit offsets
  WorkCarver c, big{(int64_t)5 << 32};
  const int64_t a = c.take(1, 256), b = c.take(257, 256), none = c.take(0, 256), slack = c.take(256);
  return a == 0 && b == 256 && none == 768 && slack == 768 && c.end == 1024 && c.take(5) == 1024 && c.end == 1029 &&
         big.take(3, 64) == ((int64_t)5 << 32) && big.take(1, 64) == ((int64_t)5 << 32) + 64;
}
static_assert(work_carver_ok(), "WorkCarver: a region starts at the aligned end of the one before it");

// ------------------------------------------------------------------ device side
#if defined(__HIPCC__)

typedef float f32x4 __attribute__((ext_vector_type(4)));   // an MFMA accumulator fragment
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// v_mfma_{f32,f64}_16x16x4: Acc is the C/D fragment, Vec 16 bytes of one LDS row (VEC elements), row(q, r) the row of
// C/D register r in lane group q = lane >> 4 (the column is lane & 15); lane_row(lane, r) is the same for a kernel that
// has the lane in hand, not q.  A transform's own tile constants go in a struct derived from this one.
template <typename S> struct Mfma16;
template <> struct Mfma16<float> {
  using Acc = f32x4;
  using Vec = f32x4;
  static constexpr int VEC = 4;
  static __device__ __forceinline__ Acc mma(float a, float b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int q, int r) { return 4 * q + r; }
  static __device__ __forceinline__ int lane_row(int lane, int r) { return row(lane >> 4, r); }
};
template <> struct Mfma16<double> {
  using Acc = f64x4;
  using Vec = f64x2;
  static constexpr int VEC = 2;
  static __device__ __forceinline__ Acc mma(double a, double b, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // the f64 C/D map: a lane group's four registers are rows q, q + 4, q + 8, q + 12, not four consecutive rows
  static __device__ __forceinline__ int row(int q, int r) { return q + 4 * r; }
  static __device__ __forceinline__ int lane_row(int lane, int r) { return row(lane >> 4, r); }
};

// DPP row shift right by N inside each 16-lane row; lanes with no source get 0 (bound_ctrl: no `old` operand to
// initialise, and the shift can fold into a consuming VOP2).
template <int N>
__device__ __forceinline__ float row_shr(float v) {
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + N, 0xf, 0xf, true);
  return __int_as_float(r);
}
template <int N>
__device__ __forceinline__ double row_shr(double v) {
  long long b = __double_as_longlong(v);
  int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), 0x110 + N, 0xf, 0xf, true);
  int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x110 + N, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// DPP row shift left by N (lane i reads lane i+N of its 16-lane row; 0 past the end).
template <int N>
__device__ __forceinline__ float row_shl(float v) {
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + N, 0xf, 0xf, true);
  return __int_as_float(r);
}
// DPP rotate right by N inside the 16-lane row (lane i reads lane (i - N) mod 16): dpp_ctrl row_ror:N
template <int N>
__device__ __forceinline__ float row_ror(float v) {
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xf, 0xf, true);
  return __int_as_float(r);
}
// DPP shift right by one lane across the WHOLE wave (gfx9 wave_shr:1; lane 0 gets 0): joins neighbouring chunks of a
// row that spans two or four 16-lane DPP rows
__device__ __forceinline__ float wave_shr1(float v) {
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true);
  return __int_as_float(r);
}
// value of lane `src` (wave-uniform index) broadcast to every lane
__device__ __forceinline__ double read_lane(double v, int src) {
  long long b = __double_as_longlong(v);
  int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), src);
  int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// GELU (erf form, nn.GELU's default) and its derivative through  erfc(|z|) = t (a1 + t (a2 + ...)) exp(-z^2),
// t = 1 / (1 + p |z|)  (Abramowitz & Stegun 7.1.26, absolute error 1.5e-7 -- the fp32 rounding level of the
// activation).  libm's erff is ~100 instructions per element and, where an activation tile ends in GELU and GELU',
// was the larger part of the kernel's vector work.  cdf = 0.5 (1 + erf(x / sqrt 2)),  ez = exp(-x^2 / 2).
__device__ __forceinline__ void gelu_parts(float x, float& cdf, float& ez) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.f));
  ez = __expf(-z * z);
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f),
                              0.254829592f);
  const float c = 0.5f * poly * ez;                      // 0.5 erfc(|z|)
  cdf = x < 0.f ? c : 1.f - c;
}
__device__ __forceinline__ float gelu_fast(float x) {
  float cdf, ez;
  gelu_parts(x, cdf, ez);
  return x * cdf;
}
__device__ __forceinline__ float gelu_grad_fast(float x) {
  float cdf, ez;
  gelu_parts(x, cdf, ez);
  return fmaf(x * 0.39894228040143267794f, ez, cdf);
}

// LDS hand-over between the lanes of ONE wave (workgroups of 64 threads): LDS operations of a wave execute in
// order, so it is enough to wait for the outstanding LDS operations and to keep the compiler from moving accesses
// across this point.  Unlike __syncthreads() this does not drain vmcnt: global stores and loads stay in flight.
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// The same hand-over between the waves of a workgroup: every wave's LDS operations are complete before any wave goes
// on.  Like wave_lds_sync() and unlike __syncthreads() it leaves global loads and stores in flight.
__device__ __forceinline__ void wg_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ------------------------------------------------------------------ host side, HIP sources
// Launches `kernel` with `lds_bytes` of dynamic LDS and checks the launch.  A kernel may use up to 48 KiB without
// asking; above that its limit is raised first.
template <typename... Params, typename... Args>
static inline int launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
                             Args... args) {
  if (lds_bytes > 48 * 1024)
    ISD_HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
  ISD_LAUNCH_CHECK();
  return ISD_OK;
}

// ISD_OK when there is a HIP device; what a plan creator asks before it allocates
static inline int require_device(const char* who) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) return ISD_OK;
  set_error("%s: no HIP device", who);
  return ISD_ERR_NO_DEVICE;
}

// A host table of n elements into a new device buffer at *dst: never a zero-byte allocation, no copy of nothing.
// A plan creator chains these on the hipError_t and leaves the freeing to its *_plan_destroy.
template <typename T>
static inline hipError_t upload(T** dst, const T* src, size_t n) {
  hipError_t e = hipMalloc((void**)dst, (n > 0 ? n : 1) * sizeof(T));
  if (e == hipSuccess && n > 0) e = hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice);
  return e;
}
template <typename T>
static inline hipError_t upload(T** dst, const std::vector<T>& v) {
  return upload(dst, v.data(), v.size());
}

#endif  // __HIPCC__
}  // namespace isd
