// Zone-batched launches for the one-encoder-per-zone heads (EEGNet_Encoder, CVBlock, HeadConv_Paper_Version;
// fast.py:203-210: eight small encoders on eight channel subsets).  Each encoder pass is a chain of ~20 short
// kernels; eight chains of them are launch-bound however they are queued (HIP-graph kernel nodes cost ~6 us each).
//
// The host code of a head stays as it is -- one plan, one call per zone.  Between isd_zone_batch_begin() and
// isd_zone_batch_launch() every kernel launch of this thread is RECORDED instead of issued (kernel, grid, block,
// arguments); isd_zone_batch_next() closes a zone.  The launch then zips the zones' chains: launch i of every zone
// is the same kernel, so it goes out ONCE with blockIdx.z = zone and the zones' argument tuples side by side in the
// kernel argument block.  A zone-batchable kernel is a struct K that is written once: `kBounds` is its launch bound and
// the static __device__ function `run(ZoneGrid, params...)` its code.  zone_kernel<K, params...> is the plain launch of
// one zone, zone_multi_kernel<K, params...> the zipped one; run() gets its own zone's grid size -- and blockIdx.z /
// gridDim.z -- in the ZoneGrid: grid-stride loops must not see the other zones', and blockIdx.z is the zone in the
// multi-zone launch.  zone_launch<K>(grid, block, lds, stream, args...) issues or records; both kernels are named at
// that launch site, so a kernel that can be launched can be zone-batched.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <tuple>
#include <utility>
#include <vector>

#include "common.h"

namespace isd {

constexpr int kMaxBatchZones = 8;

template <typename... P>
struct ZoneArgs {
  int n;
  unsigned gx[kMaxBatchZones], gy[kMaxBatchZones];
  std::tuple<P...> a[kMaxBatchZones];
};

// this zone's own gridDim.x / .y, blockIdx.z and gridDim.z
struct ZoneGrid {
  unsigned gx, gy, bz, gz;
};

#if defined(__HIPCC__)
// One zone: the plain launch.  Top-level __restrict__ is not part of run()'s type, so its pointer parameters would
// reach the entry point without it, and the compiler would then order one zone's loads and stores as if its buffers
// could overlap.  ZoneParam puts it back.  The rule that makes this right: EVERY pointer parameter of a run() is
// __restrict__ (a kernel whose buffers may overlap takes them as one pointer and offsets).
template <typename T>
struct ZoneParam {
  using type = T;
};
template <typename T>
struct ZoneParam<T*> {
  using type = T* __restrict__;
};
template <typename K, typename... P>
__global__ __launch_bounds__(K::kBounds) void zone_kernel(typename ZoneParam<P>::type... a) {
  K::run(ZoneGrid{gridDim.x, gridDim.y, blockIdx.z, gridDim.z}, a...);
}
template <typename K, typename... P>
__global__ __launch_bounds__(K::kBounds) void zone_multi_kernel(ZoneArgs<P...> m) {
  const int z = blockIdx.z;
  if (blockIdx.x >= m.gx[z] || blockIdx.y >= m.gy[z]) return;      // outside this zone's own grid
  std::apply([&](const P&... a) { K::run(ZoneGrid{m.gx[z], m.gy[z], 0u, 1u}, a...); }, m.a[z]);
}

struct ZoneFill {
  int n;
  void* p[kMaxBatchZones];
  unsigned long long n4[kMaxBatchZones];                            // 4-byte words to clear
};
__global__ __launch_bounds__(256) inline void zone_fill_kernel(ZoneFill m) {
  const int z = blockIdx.y;
  unsigned* d = reinterpret_cast<unsigned*>(m.p[z]);
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < m.n4[z]; i += (unsigned long long)gridDim.x * 256)
    d[i] = 0u;
}
#endif

// one recorded operation of one zone
struct ZoneOp {
  // kind 0: kernel; 1: clear
  int kind = 0;
  const void* kernel = nullptr;                                     // zone_kernel<K, P...>'s stub: the chain's identity
  // zips `n` recorded argument tuples (type-erased) into one launch
  hipError_t (*zip)(int n, const ZoneOp* const* ops, hipStream_t st) = nullptr;
  dim3 grid, block;
  unsigned lds = 0;
  std::shared_ptr<void> args;                                       // std::tuple<P...>
  void* ptr = nullptr;                                              // clear
  size_t bytes = 0;
};

struct ZoneRecorder {
  bool active = false;
  std::vector<std::vector<ZoneOp>> zones;
};
ZoneRecorder& zone_recorder();                                      // thread-local (zonebatch.hip)

#if defined(__HIPCC__)
template <typename K, typename... P>
hipError_t zone_zip(int n, const ZoneOp* const* ops, hipStream_t st) {
  ZoneArgs<P...> m;
  m.n = n;
  unsigned gx = 1, gy = 1, lds = 0;
  for (int z = 0; z < n; ++z) {
    m.gx[z] = ops[z]->grid.x;
    m.gy[z] = ops[z]->grid.y;
    m.a[z] = *static_cast<const std::tuple<P...>*>(ops[z]->args.get());
    gx = m.gx[z] > gx ? m.gx[z] : gx;
    gy = m.gy[z] > gy ? m.gy[z] : gy;
    lds = ops[z]->lds > lds ? ops[z]->lds : lds;
  }
  for (int z = n; z < kMaxBatchZones; ++z) {
    m.gx[z] = m.gy[z] = 0;
    m.a[z] = m.a[0];
  }
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)zone_multi_kernel<K, P...>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((zone_multi_kernel<K, P...>), dim3(gx, gy, (unsigned)n), ops[0]->block, lds, st, m);
  return hipGetLastError();
}

// Launch K now, or record it when a zone batch is open on this thread.  Returns false when the launch cannot be
// recorded.  The parameter types P... are those of K::run after its ZoneGrid.
template <typename K, typename Run = decltype(&K::run)>
struct ZoneLaunch;
template <typename K, typename... P>
struct ZoneLaunch<K, void (*)(ZoneGrid, P...)> {
  template <typename... A>
  static bool launch(dim3 grid, dim3 block, unsigned lds, hipStream_t st, A&&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "argument count");
    ZoneRecorder& r = zone_recorder();
    if (!r.active) {
      hipLaunchKernelGGL((zone_kernel<K, P...>), grid, block, lds, st, static_cast<P>(args)...);
      return true;
    }
    if (grid.z != 1) {
      set_error("zone batch: a kernel of this call is not zone-batchable");
      r.active = false;                                             // poison: isd_zone_batch_launch reports it
      r.zones.clear();
      return false;
    }
    ZoneOp op;
    op.kind = 0;
    op.kernel = reinterpret_cast<const void*>(&zone_kernel<K, P...>);
    op.zip = &zone_zip<K, P...>;
    op.grid = grid;
    op.block = block;
    op.lds = lds;
    op.args = std::make_shared<std::tuple<P...>>(static_cast<P>(args)...);
    r.zones.back().push_back(std::move(op));
    return true;
  }
};
template <typename K, typename... A>
bool zone_launch(dim3 grid, dim3 block, unsigned lds, hipStream_t st, A&&... args) {
  return ZoneLaunch<K>::launch(grid, block, lds, st, std::forward<A>(args)...);
}
// every launch of a zone-batchable kernel goes through zone_launch; a refused record ends the calling function
#define ISD_ZLAUNCH(K, ...)                                      \
  do {                                                           \
    if (!zone_launch<K>(__VA_ARGS__)) return ISD_ERR_INVALID;    \
  } while (0)

// hipMemsetAsync(ptr, 0, bytes) -- or its record (ptr and bytes must be multiples of 4)
inline hipError_t zone_clear(void* ptr, size_t bytes, hipStream_t st) {
  ZoneRecorder& r = zone_recorder();
  if (!r.active) return hipMemsetAsync(ptr, 0, bytes, st);
  ZoneOp op;
  op.kind = 1;
  op.ptr = ptr;
  op.bytes = bytes;
  r.zones.back().push_back(std::move(op));
  return hipSuccess;
}

#endif  // __HIPCC__

}  // namespace isd
