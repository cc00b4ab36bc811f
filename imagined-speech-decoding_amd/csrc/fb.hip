// Filterbank: per-band Butterworth SOS cascade as a chunked linear-recurrence scan.
//
// Replaces scipy `sosfilt(butter(..., 'sos'), x, axis=-1)` (spec S steps 1-2; the
// reference's only band-pass is notebooks/svm_baseline.ipynb:238).
//
// Mapping (CDNA4, wave64): a 16-lane DPP row owns one 512-sample segment of one
// (trial, channel) row; each lane owns a contiguous 32-sample chunk in registers.
// Per band and per biquad section:
//   1. in-chunk DF2T recursion from zero state            (3 VALU ops / sample)
//   2. inclusive scan of the chunk-end states over the 16 lanes with the constant
//      2x2 transition matrix M = A^32 (Kogge-Stone over DPP row_shr, fp64)
//   3. zero-input correction  y[n] += h1[n]*s1_in + h2[n]*s2_in   (2 FMA / sample)
// Global traffic is coalesced float4; the chunk<->coalesced transposition goes
// through a padded LDS tile (stride 36 floats: conflict-free ds_read_b128).
// Rows longer than 512 samples chain 2 or 4 rows-of-16-lanes (and loop) with the
// group transition matrix P = M^16 and per-lane powers Q_i = M^i.
#include "common.h"
#include "stft_plan.h"
#include <math.h>
#include <stdlib.h>
#include <vector>
#include <string.h>
#include <type_traits>
#include <atomic>
#include <algorithm>

namespace isd {

constexpr int kL = 32;          // samples per lane
constexpr int kSeg = 16 * kL;   // samples per 16-lane group
constexpr int kPad = kL + 4;    // LDS chunk stride (floats)
constexpr int kMaxSec = 8;
constexpr int64_t kMaxRows = 0x7fffffffLL / (8 * 8);   // rows = trials x channels: 32-bit row / workgroup ids on the device

struct FbSec {                  // constants of one (band, section); wave-uniform -> SMEM loads
  double Mp[4][4];              // M^(1,2,4,8), row-major 2x2, M = A^32
  double P[4];                  // M^16
  double N16d[4];               // A^16: joins the two 16-sample halves a lane runs side by side
  double a1d, a2d;
  double hdq[2][kL / 2];        // zero-input response seen at the output (row 0 of A^n), n < 16, structure-of-arrays
  float a1f, a2f;
  float N16f[4];
  float hq[2][kL / 2];
};

struct FbBand {
  double gd;
  float gf;
  float pad;
};

// The constants of one (band, section) as fused_serial_kernel reads them: three 64-byte lines, every scalar load inside
// one line, 6.8 KiB for the nine bands of the headline set (FbSec, 624 bytes of which that kernel needs 192 scattered
// over seven lines, made the tables of a workgroup's step -- 22 KiB -- larger than the 16 KiB scalar cache).
struct alignas(64) SerSec {
  double M[4];                  // A^32
  float a1, a2, N16[4], one, pad;   // recursion coefficients, A^16, 1.0f (see section_serial_f32)
  float hq[2][kL / 2];          // zero-input response at the output, n < 16
};
static_assert(sizeof(SerSec) == 192, "SerSec is three cache lines");

}  // namespace isd

// The bands of a plan are split by arithmetic: set 0 runs the in-chunk recursion in fp32, set 1 in fp64
// (ISD_FB_AUTO decides per band; ISD_FB_F32 / ISD_FB_F64 put every band in one set).  `d_map` gives the
// position of a set's band in the caller's band order.
struct FbSet {
  int nb;
  isd::FbSec* d_sec;   // [nb][n_sections]
  isd::FbBand* d_band; // [nb]
  double* d_Q;         // [nb][n_sections][16][4]  per-lane M^i
  int* d_map;          // [nb] output band index
  isd::SerSec* d_ser;  // [nb][n_sections] compact copy for fused_serial_kernel (fp32 set only)
};
struct isd_fb_plan {
  int n_bands, n_sections, precision;   // precision: ISD_FB_F32, ISD_FB_F64 or ISD_FB_MIXED
  FbSet set[2];
  int* host_map[2];    // host copies of the output maps (band-bin tables are gathered through them)
};

namespace isd {

typedef float f2 __attribute__((ext_vector_type(2)));

// The lane's 32 input samples, always fp32: 16 register PAIRS {sample j, sample j + 16}.
typedef f2 XArr[kL / 2];

// Arithmetic types of the in-chunk recursion.  The two 16-sample halves of the chunk are independent recurrences
// (zero state each) joined afterwards through A^16 (section<>, below):
//  * float: the halves share one register pair, so the whole cascade runs on v_pk_add / v_pk_fma_f32
//    (tools/ubench/valu_rate.hip: v_fma_f32 70 TF, v_pk_fma_f32 119 TF, v_fma_f64 62 TF);
//  * double (bands with a pole too close to z = 1 for fp32): the halves are two interleaved dependency chains of
//    v_fma_f64.  The chunk stays fp64 until the state fix-up has been added: the zero-state response of a chunk is
//    ~30x larger than the signal for these bands (it cancels against the fix-up), so rounding it to fp32 first costs
//    1.6e-6 of the peak where the fp64 sum is good to 6e-8.
template <typename VT> struct VOps;
template <> struct VOps<float> {
  using S = float;
  typedef f2 Arr[kL / 2];
  static __device__ __forceinline__ float at(const Arr& a, int n) { return (n & 16) ? a[n & 15].y : a[n & 15].x; }
  static __device__ __forceinline__ float g(const FbBand& b) { return b.gf; }
  static __device__ __forceinline__ void from_x(Arr& v, const XArr& xs, float gain) {
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) v[j] = xs[j] * gain;
  }
  static __device__ __forceinline__ void to_f32(const Arr& v, XArr& o) {
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) o[j] = v[j];
  }
};
template <> struct VOps<double> {
  using S = double;
  typedef double Arr[kL];                          // natural order: n < 16 first half, n >= 16 second half
  static __device__ __forceinline__ double at(const Arr& a, int n) { return a[n]; }
  static __device__ __forceinline__ double g(const FbBand& b) { return b.gd; }
  static __device__ __forceinline__ void from_x(Arr& v, const XArr& xs, double gain) {
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) {
      v[j] = (double)xs[j].x * gain;
      v[j + 16] = (double)xs[j].y * gain;
    }
  }
  static __device__ __forceinline__ void to_f32(const Arr& v, XArr& o) {
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) o[j] = (f2){(float)v[j], (float)v[j + 16]};
  }
};

// The same pointer, opaque to the compiler from here on: loads through the result cannot be hoisted above this point
// or merged with earlier loads of the structure.  The scalar tables of a section (116 dwords in the fp64 instance) do
// not fit the SGPR file at once; left alone, the scheduler clusters their s_loads at the top of the section and the
// register allocator spills the surplus into VGPR lanes (v_writelane / v_readlane: 42 % of the VALU instructions of
// the first fp64 long-row kernel).
// (The opaque part is a zero OFFSET, not the pointer: the result is still based on the __restrict__ kernel argument,
// so the loads stay scalar -- a laundered pointer may alias the kernel's stores and its loads turn into vector loads.)
template <typename P>
__device__ __forceinline__ const P* later(const P* p) {
  int zero = 0;
  asm volatile("" : "+s"(zero));
  return reinterpret_cast<const P*>(reinterpret_cast<const char*>(p) + zero);
}

// value of lane 15 of each 16-lane DPP row in every lane of the row (gfx90a+ row_newbcast)
__device__ __forceinline__ double row_bcast15(double v) {
  long long b = __double_as_longlong(v);
  int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), 0x15F, 0xf, 0xf, true);
  int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x15F, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <int D>
__device__ __forceinline__ void scan_step(double& e1, double& e2, const double* M) {
  double p1 = row_shr<D>(e1), p2 = row_shr<D>(e2);
  e1 = fma(M[0], p1, fma(M[1], p2, e1));
  e2 = fma(M[2], p1, fma(M[3], p2, e2));
}

// One biquad section over the lane's chunk, including the cross-chunk state fix-up.
// c1/c2: incoming state of the wave's first group (GPR == 4 loop carry), updated.
// Qsec (GPR > 1): the 16 per-lane matrices M^i of this section, [16][4] doubles.  The long-row kernels stage them in
// LDS once per band: as a per-lane global load inside the section they were waited for ~100 instructions after issue,
// at L2 latency under a saturated write stream (PMC: the fp32 long-row kernel sat in s_waitcnt for half of its wave
// cycles).
// CARRY (with GPR == 1): every 16-lane group walks its own row in 512-sample passes; (c1, c2) is the state entering the
// group's pass and comes back, on lane 15 of the group, as the state leaving it (P c + the group's own end state).
template <typename VT, int GPR, bool CARRY = false>
__device__ __forceinline__ void section(typename VOps<VT>::Arr& v, const FbSec& sc, const double* Qsec,
                                        int lane, double& c1, double& c2) {
  // in-chunk recursion from zero state, both halves side by side; sA = final state of the first half,
  // (e1, e2) = state after the whole chunk = A^16 sA + sB
  double e1, e2;
  [[maybe_unused]] float sA1f = 0.f, sA2f = 0.f;
  [[maybe_unused]] double sA1d = 0.0, sA2d = 0.0;
  if constexpr (std::is_same<VT, float>::value) {
    const float na1 = -sc.a1f, na2 = -sc.a2f;
    const f2 NA1 = {na1, na1}, NA2 = {na2, na2};
    f2 S1 = {0.f, 0.f}, S2 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) {
      const f2 x = v[j];
      const f2 y = x + S1;
      S1 = __builtin_elementwise_fma(NA1, y, S2);
      S2 = __builtin_elementwise_fma(NA2, y, -x);
      v[j] = y;
    }
    sA1f = S1.x; sA2f = S2.x;
    e1 = (double)fmaf(sc.N16f[0], S1.x, fmaf(sc.N16f[1], S2.x, S1.y));
    e2 = (double)fmaf(sc.N16f[2], S1.x, fmaf(sc.N16f[3], S2.x, S2.y));
  } else {
    const double na1 = -sc.a1d, na2 = -sc.a2d;
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0;
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) {
      const double xa = v[j], xb = v[j + 16];
      const double ya = xa + s1a, yb = xb + s1b;
      s1a = fma(na1, ya, s2a);
      s1b = fma(na1, yb, s2b);
      s2a = fma(na2, ya, -xa);
      s2b = fma(na2, yb, -xb);
      v[j] = ya;
      v[j + 16] = yb;
    }
    sA1d = s1a; sA2d = s2a;
    e1 = fma(sc.N16d[0], s1a, fma(sc.N16d[1], s2a, s1b));
    e2 = fma(sc.N16d[2], s1a, fma(sc.N16d[3], s2a, s2b));
  }
  // inclusive scan of the chunk-end states over the 16 lanes of a DPP row (always fp64)
  const FbSec& sm = *later(&sc);
  scan_step<1>(e1, e2, sm.Mp[0]);
  scan_step<2>(e1, e2, sm.Mp[1]);
  scan_step<4>(e1, e2, sm.Mp[2]);
  scan_step<8>(e1, e2, sm.Mp[3]);
  double i1 = row_shr<1>(e1);                          // exclusive; lane 0 of each 16-lane row -> 0
  double i2 = row_shr<1>(e2);
  if (GPR == 1 && CARRY) {
    const double2* Q2 = reinterpret_cast<const double2*>(Qsec + (lane & 15) * 4);      // M^i of this lane
    const double2 Qa = Q2[0], Qb = Q2[1];
    i1 = fma(Qa.x, c1, fma(Qa.y, c2, i1));
    i2 = fma(Qb.x, c1, fma(Qb.y, c2, i2));
    const double n1 = fma(sm.P[0], c1, fma(sm.P[1], c2, e1));    // meaningful on lane 15: M^16 c + the group's end state
    const double n2 = fma(sm.P[2], c1, fma(sm.P[3], c2, e2));
    c1 = n1;
    c2 = n2;
  }
  if (GPR > 1) {
    // group totals (wave-uniform) and the serial chain over the 4 groups of the wave
    double E1[4], E2[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      E1[g] = read_lane(e1, 16 * g + 15);
      E2[g] = read_lane(e2, 16 * g + 15);
    }
    double C1[4], C2[4];
    C1[0] = (GPR == 4) ? c1 : 0.0;
    C2[0] = (GPR == 4) ? c2 : 0.0;
    const FbSec& sp = sm;
#pragma unroll
    for (int g = 1; g < 4; ++g) {
      if (g % GPR == 0) {
        C1[g] = 0.0;
        C2[g] = 0.0;
      } else {
        C1[g] = fma(sp.P[0], C1[g - 1], fma(sp.P[1], C2[g - 1], E1[g - 1]));
        C2[g] = fma(sp.P[2], C1[g - 1], fma(sp.P[3], C2[g - 1], E2[g - 1]));
      }
    }
    if (GPR == 4) {
      c1 = fma(sp.P[0], C1[3], fma(sp.P[1], C2[3], E1[3]));
      c2 = fma(sp.P[2], C1[3], fma(sp.P[3], C2[3], E2[3]));
    }
    const int q = lane >> 4;
    const double m1 = q == 0 ? C1[0] : q == 1 ? C1[1] : q == 2 ? C1[2] : C1[3];
    const double m2 = q == 0 ? C2[0] : q == 1 ? C2[1] : q == 2 ? C2[2] : C2[3];
    const double2* Q2 = reinterpret_cast<const double2*>(Qsec + (lane & 15) * 4);      // M^i of this lane
    const double2 Qa = Q2[0], Qb = Q2[1];
    const double Q[4] = {Qa.x, Qa.y, Qb.x, Qb.y};
    i1 = fma(Q[0], m1, fma(Q[1], m2, i1));
    i2 = fma(Q[2], m1, fma(Q[3], m2, i2));
  }
  // zero-input correction; the table scalars are fetched here, after the scan released its matrix SGPRs
  const FbSec& sh = *later(&sc);
  if constexpr (std::is_same<VT, float>::value) {
    const float t1 = (float)i1, t2 = (float)i2;
    // incoming state of the second half: A^16 t + sA; both halves then take the same 16-entry table
    const float u1 = fmaf(sh.N16f[0], t1, fmaf(sh.N16f[1], t2, sA1f));
    const float u2 = fmaf(sh.N16f[2], t1, fmaf(sh.N16f[3], t2, sA2f));
    const f2 T1 = {t1, u1}, T2 = {t2, u2};
#pragma unroll
    for (int j = 0; j < kL / 2; ++j)
      v[j] = __builtin_elementwise_fma((f2){sh.hq[0][j], sh.hq[0][j]}, T1,
                                       __builtin_elementwise_fma((f2){sh.hq[1][j], sh.hq[1][j]}, T2, v[j]));
  } else {
    const double u1 = fma(sh.N16d[0], i1, fma(sh.N16d[1], i2, sA1d));
    const double u2 = fma(sh.N16d[2], i1, fma(sh.N16d[3], i2, sA2d));
#pragma unroll
    for (int q = 0; q < kL / 2; q += 8) {
      const FbSec& sq = *later(&sc);                         // 16 table doubles (32 SGPRs) per batch
#pragma unroll
      for (int j = q; j < q + 8; ++j) {
        const double h1 = sq.hdq[0][j], h2 = sq.hdq[1][j];
        v[j] = fma(h1, i1, fma(h2, i2, v[j]));
        v[j + 16] = fma(h1, u1, fma(h2, u2, v[j + 16]));
      }
    }
  }
}

// The band's per-lane matrices (Qtab: [band * ns + section][16 lanes][4 doubles]) into LDS, 32 bytes per lane.
__device__ __forceinline__ void stage_q(double* Qlds, const double* __restrict__ Qtab, int b, int ns, int lane) {
  for (int e = lane; e < ns * 16; e += 64) {
    const double2* q = reinterpret_cast<const double2*>(Qtab + (int64_t)b * ns * 64 + e * 4);
    const double2 a = q[0], c = q[1];
    reinterpret_cast<double2*>(Qlds + e * 4)[0] = a;
    reinterpret_cast<double2*>(Qlds + e * 4)[1] = c;
  }
}

// Cooperative (whole wave) coalesced load of the 4 groups' 512-sample segments into the
// padded chunk-major LDS tile.  gbase[g] < 0 marks an absent group.
// FULL: every group present, whole 512-sample segments, 16-byte aligned rows -- eight loads back to back, no tests
template <bool FULL = false>
__device__ __forceinline__ void tile_load(float* tile, const float* __restrict__ x, int lane,
                                          const int64_t (&gbase)[4], const int (&gt0)[4], int T, bool vec) {
  if (FULL) {
    float4 val[8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k)
        val[g * 2 + k] = *reinterpret_cast<const float4*>(x + gbase[g] + gt0[g] + (k * 64 + lane) * 4);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = (k * 64 + lane) * 4;
        *reinterpret_cast<float4*>(tile + (g * 16 + (e >> 5)) * kPad + (e & 31)) = val[g * 2 + k];
      }
    return;
  }
  if (vec) {
    // T % 4 == 0, aligned rows: a float4 lies wholly inside its row or wholly outside.  Outside ones read x[0..3]
    // (always there) and are zeroed by a select, so the eight loads still issue back to back (a test around each
    // load would give each its own basic block and its own wait).
    float4 val[8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int t = gt0[g] + (k * 64 + lane) * 4;
        const bool ok = gbase[g] >= 0 && t < T;
        val[g * 2 + k] = *reinterpret_cast<const float4*>(x + (ok ? gbase[g] + t : (int64_t)0));
      }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = (k * 64 + lane) * 4;
        const bool ok = gbase[g] >= 0 && gt0[g] + e < T;
        float4 v = val[g * 2 + k];
        v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
        *reinterpret_cast<float4*>(tile + (g * 16 + (e >> 5)) * kPad + (e & 31)) = v;
      }
    return;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = (k * 64 + lane) * 4;              // element inside the 512-sample segment
      const int t = gt0[g] + e;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gbase[g] >= 0) {
        const float* p = x + gbase[g] + t;
        if (vec && t + 3 < T) {
          val = *reinterpret_cast<const float4*>(p);
        } else {
          if (t + 0 < T) val.x = p[0];
          if (t + 1 < T) val.y = p[1];
          if (t + 2 < T) val.z = p[2];
          if (t + 3 < T) val.w = p[3];
        }
      }
      *reinterpret_cast<float4*>(tile + (g * 16 + (e >> 5)) * kPad + (e & 31)) = val;
    }
  }
}

// FULL: every group present, whole 512-sample segments, 16-byte aligned rows -- no test stands between the eight
// tile reads and the eight stores
// The filtered signals are written once and are far larger than the caches (4.8 GB per pass at cfg 2): non-temporal
// stores (no allocation in L2 / MALL on the way out) took the materialising filterbank from 4.70-4.73 to 4.79-4.83 TB/s
// on one box.
__device__ __forceinline__ void store_stream4(float* p, const float4& w) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store((f4v){w.x, w.y, w.z, w.w}, reinterpret_cast<f4v*>(p));
}

template <bool FULL = false>
__device__ __forceinline__ void tile_store(const float* tile, float* __restrict__ y, int lane,
                                           const int64_t (&gbase)[4], const int (&gt0)[4], int T, bool vec) {
  if (FULL) {
    float4 val[8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = (k * 64 + lane) * 4;
        val[g * 2 + k] = *reinterpret_cast<const float4*>(tile + (g * 16 + (e >> 5)) * kPad + (e & 31));
      }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) store_stream4(y + gbase[g] + gt0[g] + (k * 64 + lane) * 4, val[g * 2 + k]);
    return;
  }
  if (vec) {                                          // all tile reads first, then the (predicated) stores
    float4 val[8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = (k * 64 + lane) * 4;
        val[g * 2 + k] = *reinterpret_cast<const float4*>(tile + (g * 16 + (e >> 5)) * kPad + (e & 31));
      }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int t = gt0[g] + (k * 64 + lane) * 4;
        if (gbase[g] >= 0 && t < T) store_stream4(y + gbase[g] + t, val[g * 2 + k]);
      }
    return;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = (k * 64 + lane) * 4;
      const int t = gt0[g] + e;
      if (gbase[g] < 0 || t >= T) continue;
      const float4 val = *reinterpret_cast<const float4*>(tile + (g * 16 + (e >> 5)) * kPad + (e & 31));
      float* p = y + gbase[g] + t;
      if (vec && t + 3 < T) {
        *reinterpret_cast<float4*>(p) = val;
      } else {
        p[0] = val.x;
        if (t + 1 < T) p[1] = val.y;
        if (t + 2 < T) p[2] = val.z;
        if (t + 3 < T) p[3] = val.w;
      }
    }
  }
}

// Load the lane's chunk through the LDS tile (coalesced global reads, chunk-major registers).
template <bool FULL = false>
__device__ __forceinline__ void load_chunks(XArr& xs, float* tile, const float* __restrict__ x, int lane,
                                            const int64_t (&xbase)[4], const int (&gt0)[4], int T, bool vec) {
  wave_lds_sync();
  tile_load<FULL>(tile, x, lane, xbase, gt0, T, vec);
  wave_lds_sync();
  const float* src = tile + lane * kPad;              // (q*16 + i) == lane
#pragma unroll
  for (int n = 0; n < kL / 2; n += 4) {
    const float4 a = *reinterpret_cast<const float4*>(src + n);
    const float4 b = *reinterpret_cast<const float4*>(src + n + 16);
    xs[n] = (f2){a.x, b.x};
    xs[n + 1] = (f2){a.y, b.y};
    xs[n + 2] = (f2){a.z, b.z};
    xs[n + 3] = (f2){a.w, b.w};
  }
}

// The lane's chunk written back as 32 consecutive floats of its LDS tile row.  fp32: register pair j holds samples
// j and j + 16, which is exactly one ds_write2_b32 (two dword slots 16 apart) -- assembling float4s first costs 32
// register moves and their temporaries, which the 96-register fp32 long-row kernel does not have.
template <typename VT>
__device__ __forceinline__ void chunk_to_tile(float* dst, const typename VOps<VT>::Arr& v) {
  if constexpr (std::is_same<VT, float>::value) {
    // (inline asm: written as scalar stores, the SLP vectoriser re-assembles the float4s.  A DS write reads its
    // operands at issue and wave_lds_sync() waits for lgkmcnt(0) before any lane reads the tile.)
    const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)dst;
#pragma unroll
    for (int j = 0; j < kL / 2; ++j)
      asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(a), "v"(v[j].x), "v"(v[j].y), "i"(j), "i"(j + 16)
                   : "memory");
  } else {
#pragma unroll
    for (int n = 0; n < kL; n += 4)
      *reinterpret_cast<float4*>(dst + n) = make_float4((float)v[n], (float)v[n + 1], (float)v[n + 2], (float)v[n + 3]);
  }
}

// Rows of at most 1024 samples.  One wave per workgroup; GPR = 16-lane groups per row (1: T<=512, 2: T<=1024);
// the wave serves 4/GPR rows.  The input chunk stays in registers (fp32) for all bands.
template <typename VT, int GPR, bool FULL = false>
__global__ __launch_bounds__(64) void fb_kernel(const FbSec* __restrict__ secs, const FbBand* __restrict__ bands,
                                                const double* __restrict__ Qtab, const float* __restrict__ x,
                                                float* __restrict__ y, int R, int C, int T, int nb, int ns,
                                                int vec, const int* __restrict__ bmap, int nb_out) {
  using O = VOps<VT>;
  static_assert(GPR == 1 || GPR == 2, "long rows take fb_long_kernel");
  __shared__ __attribute__((aligned(16))) float tile[4 * 16 * kPad];
  const int lane = threadIdx.x;
  constexpr int RPS = 4 / GPR;                                             // rows per wave
  const int row0 = blockIdx.x * RPS;
  int64_t xbase[4], yrow[4];
  int gt0[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    gt0[g] = (g % GPR) * kSeg;
    const int row = row0 + g / GPR;
    const bool ok = row < R && gt0[g] < T;
    xbase[g] = ok ? row * (int64_t)T : -1;
    const int bt = row / C, ch = row - bt * C;
    yrow[g] = ok ? ((int64_t)bt * nb_out * C + ch) * (int64_t)T : -1;     // band 0 of the row's trial
  }
  const int64_t bstride = (int64_t)C * T;
  XArr xs;
  load_chunks<FULL>(xs, tile, x, lane, xbase, gt0, T, vec != 0);
  for (int b = 0; b < nb; ++b) {
    typename O::Arr v;
    O::from_x(v, xs, O::g(bands[b]));
    for (int s = 0; s < ns; ++s) {
      double c1 = 0.0, c2 = 0.0;
      section<VT, GPR>(v, secs[b * ns + s], Qtab + (int64_t)(b * ns + s) * 64, lane, c1, c2);
    }
    wave_lds_sync();                              // earlier readers of the tile are done
    chunk_to_tile<VT>(tile + lane * kPad, v);
    wave_lds_sync();
    int64_t ybase[4];
    const int64_t boff = (int64_t)bmap[b] * bstride;
#pragma unroll
    for (int g = 0; g < 4; ++g) ybase[g] = yrow[g] < 0 ? -1 : yrow[g] + boff;
    tile_store<FULL>(tile, y, lane, ybase, gt0, T, vec != 0);
  }
}

// The lane's 32 samples of pass `it` straight from global memory (128 contiguous bytes per lane, 8 KiB per wave), in
// two steps so that the loads can be requested long before they are needed:
//   chunk_issue  -- eight float4 loads, unconditionally and back to back (addresses clamped into the row);
//   chunk_finish -- zeroes what lies past the end of the row (ragged last pass only) and forms the sample pairs.
// With the bounds tests around the individual loads the compiler merged the variants per load and put an
// s_waitcnt vmcnt(0) behind every one of them: eight serial L2 round trips per pass (PMC: the fp32 long-row kernel
// sat in s_waitcnt for half of its wave cycles).  VEC: rows are 16-byte aligned and T % 4 == 0.
template <bool VEC>
__device__ __forceinline__ void chunk_issue(float4 (&f)[kL / 4], const float* __restrict__ src, int it, int lane,
                                            int T) {
  const int e0 = (it * 64 + lane) * kL;
  if (VEC) {
    const int emax = T - 4;                                     // last valid float4 of the row
#pragma unroll
    for (int n = 0; n < kL / 4; ++n) {
      const int e = e0 + 4 * n;
      f[n] = *reinterpret_cast<const float4*>(src + (e < emax ? e : emax));
    }
  } else {
    const int last = T - 1;
#pragma unroll
    for (int n = 0; n < kL / 4; ++n) {
      const int e = e0 + 4 * n;
      f[n] = make_float4(src[e < last ? e : last], src[e + 1 < last ? e + 1 : last], src[e + 2 < last ? e + 2 : last],
                         src[e + 3 < last ? e + 3 : last]);
    }
  }
}
__device__ __forceinline__ float f4_get(const float4& q, int c) { return c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w; }
__device__ __forceinline__ void chunk_finish(XArr& xs, const float4 (&f)[kL / 4], int it, int lane, int T) {
  if ((it + 1) * 64 * kL > T) {                                 // wave-uniform: the ragged last pass
    const int e0 = (it * 64 + lane) * kL;
#pragma unroll
    for (int j = 0; j < kL / 2; ++j)
      xs[j] = (f2){e0 + j < T ? f4_get(f[j >> 2], j & 3) : 0.f, e0 + j + 16 < T ? f4_get(f[(j >> 2) + 4], j & 3) : 0.f};
  } else {
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) xs[j] = (f2){f4_get(f[j >> 2], j & 3), f4_get(f[(j >> 2) + 4], j & 3)};
  }
}

constexpr int kLongShare = 8;                    // one-wave workgroups sharing a long row (fused_long_kernel: 4 -> 4.58 ms, 8 -> 4.47 ms per 128 stress trials)

// Rows longer than 1024 samples (the stress configuration: 4096).  One row per wave, 2048 samples per pass, the
// section states carried from pass to pass in LDS.  The band loop is outermost and the x pass is re-read from global
// memory for every band (it stays in the XCD's L2): nothing of x lives in registers across bands, which is what
// lets the fp64 instance run at 4 waves per SIMD (the first version kept x and the chunk as doubles: 201 VGPRs, 2
// waves per SIMD, 18.6 % of the HBM peak).  kLongShare one-wave workgroups share a row, each taking every
// kLongShare-th band; their ids are congruent mod 8 (workgroups go to the 8 XCDs round-robin by id, each XCD has its
// own L2) inside 64 consecutive ids, so the re-reads of a row hit one L2.  The filtered pass leaves through half of
// the chunk-major LDS tile at a time (coalesced float4 stores, 4.6 KiB of LDS per wave).
template <typename VT, bool VEC, bool EARLYX>
__device__ __forceinline__ void fb_long_body(
    const FbSec* __restrict__ secs, const FbBand* __restrict__ bands, const double* __restrict__ Qtab,
    const float* __restrict__ x, float* __restrict__ y, int C, int T, int nb, int ns,
    const int* __restrict__ bmap, int nb_out, int n_rows) {
  using O = VOps<VT>;
  // EARLYX: the x pass of the NEXT (band, pass) is requested in front of this pass's stores (vmcnt retires in issue
  // order, so a load issued behind the eight stores waits for their acknowledgement).  Measured on the fp32 instance:
  // 1.96 ms per 128 stress trials at the 4 waves per SIMD its 32 extra live registers leave, against 1.70 ms without
  // it at 5 waves -- not dispatched.
  constexpr bool kEarlyX = EARLYX;
  __shared__ __attribute__((aligned(16))) float tile[2 * 16 * kPad];        // 32 chunks: half a pass
  __shared__ __attribute__((aligned(16))) double Qlds[kMaxSec * 64];        // the band's per-lane M^i
  __shared__ double carry[kMaxSec * 2];
  const int lane = threadIdx.x;
  const int n_iter = (T + 4 * kSeg - 1) / (4 * kSeg);
  // id = 8 kLongShare q + 8 w + c  <->  row = 8 q + c, band subset w
  const int id = blockIdx.x;
  const int row = (id / (8 * kLongShare)) * 8 + (id & 7);
  const int share = (id >> 3) % kLongShare;
  if (row >= n_rows) return;
  const int bt = row / C, ch = row - bt * C;
  const float* src = x + row * (int64_t)T;
  float* dst0 = y + ((int64_t)bt * nb_out * C + ch) * (int64_t)T;
  const int64_t bstride = (int64_t)C * T;
  float4 xf[kL / 4];
  if (kEarlyX) chunk_issue<VEC>(xf, src, 0, lane, T);
  for (int b = share; b < nb; b += kLongShare) {
    if (lane < ns * 2) carry[lane] = 0.0;
    stage_q(Qlds, Qtab, b, ns, lane);
    wave_lds_sync();
    float* dst = dst0 + (int64_t)bmap[b] * bstride;
    const auto gain = O::g(bands[b]);
    for (int it = 0; it < n_iter; ++it) {
      if (!kEarlyX) chunk_issue<VEC>(xf, src, it, lane, T);
      typename O::Arr v;
      {
        XArr xs;
        chunk_finish(xs, xf, it, lane, T);
        O::from_x(v, xs, gain);
      }
      for (int sct = 0; sct < ns; ++sct) {
        double c1 = carry[sct * 2], c2 = carry[sct * 2 + 1];
        section<VT, 4>(v, secs[b * ns + sct], Qlds + sct * 64, lane, c1, c2);
        wave_lds_sync();                                // every lane has read the incoming carry
        if (lane == 0) {
          carry[sct * 2] = c1;
          carry[sct * 2 + 1] = c2;
        }
      }
      if (kEarlyX) chunk_issue<VEC>(xf, src, it + 1 < n_iter ? it + 1 : 0, lane, T);
      // transposition to coalesced stores, half a pass (1024 samples = 32 chunks) at a time
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        wave_lds_sync();                                // the previous half's readers are done
        if ((lane >> 5) == h) chunk_to_tile<VT>(tile + (lane & 31) * kPad, v);
        wave_lds_sync();
        const int t_half = (it * 2 + h) * 2 * kSeg;     // first sample of this half pass
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = (k * 64 + lane) * 4;            // element inside the half pass
          const int t = t_half + e;
          if (t >= T) continue;
          const float4 val = *reinterpret_cast<const float4*>(tile + (e >> 5) * kPad + (e & 31));
          float* p = dst + t;
          if (VEC) {                                    // T % 4 == 0: t < T implies t + 3 < T
            *reinterpret_cast<float4*>(p) = val;
          } else {
            p[0] = val.x;
            if (t + 1 < T) p[1] = val.y;
            if (t + 2 < T) p[2] = val.z;
            if (t + 3 < T) p[3] = val.w;
          }
        }
      }
    }
    wave_lds_sync();
  }
}

#define ISD_FB_LONG_ARGS                                                                                          \
  const FbSec *__restrict__ secs, const FbBand *__restrict__ bands, const double *__restrict__ Qtab,            \
      const float *__restrict__ x, float *__restrict__ y, int C, int T, int nb, int ns,                         \
      const int *__restrict__ bmap, int nb_out, int n_rows
// the register cap is per instance: 96 VGPRs (5 waves per SIMD) for fp32, 128 (4 waves) for fp64
template <bool VEC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void fb_long_kernel_f32(ISD_FB_LONG_ARGS) {
  fb_long_body<float, VEC, false>(secs, bands, Qtab, x, y, C, T, nb, ns, bmap, nb_out, n_rows);
}
template <bool VEC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void fb_long_kernel_f64(ISD_FB_LONG_ARGS) {
  fb_long_body<double, VEC, false>(secs, bands, Qtab, x, y, C, T, nb, ns, bmap, nb_out, n_rows);
}
#undef ISD_FB_LONG_ARGS

// Long rows of whole 512-sample passes, FOUR ROWS PER WAVE: every 16-lane group walks its own row and carries its
// section states from pass to pass (two doubles per band, section and group in LDS), so the serial cross-group chain
// of fb_long_body -- a hundred vector instructions per section in a kernel the PMC shows 87 % VALU-busy -- is gone.
// kLongShare workgroups share a quad of rows, each taking every kLongShare-th band, and the PASS loop is outermost:
// a pass of x is read once per workgroup and filtered through all of the workgroup's bands (with the band loop
// outermost the quad was re-read per band: the PMC showed 2.75 GB through the fabric for a 268 MB input next to the
// 6.4 GB of filtered output -- the kernel sat at the memory system's limit on traffic it did not need).  The per-lane
// M^i come straight from global memory (L1-resident, 64 bytes per lane and section).  The filtered pass leaves two
// rows at a time through the half tile as coalesced float4 stores.
constexpr int kRows4Bands = (kMaxBands + kLongShare - 1) / kLongShare;      // bands of one workgroup
template <typename VT, bool PASS_OUTER, bool FULLQ>
__device__ __forceinline__ void fb_rows4_body(
    const FbSec* __restrict__ secs, const FbBand* __restrict__ bands, const double* __restrict__ Qtab,
    const float* __restrict__ x, float* __restrict__ y, int C, int T, int nb, int ns,
    const int* __restrict__ bmap, int nb_out, int n_rows, int share_n) {
  using O = VOps<VT>;
  __shared__ __attribute__((aligned(16))) float tile[2 * 16 * kPad];        // 32 chunks: two rows of one pass
  __shared__ double carry[kRows4Bands * kMaxSec * 8];                       // [band of this workgroup][section][group][2]
  const int lane = threadIdx.x;
  const int n_iter = T / kSeg;
  // share_n workgroups share a quad (host: rows4_share(nb) -- the count in [4, 8] that leaves the fewest idle band
  // slots: 35 bands -> 7 x 5, 5 bands -> 5 x 1; with a fixed 8 the last round of a 35-band set ran 3 of 8 sharers)
  const int id = blockIdx.x;
  const int quad = (id / (8 * share_n)) * 8 + (id & 7);
  const int share = (id >> 3) % share_n;
  if (quad * 4 >= n_rows) return;
  const int64_t bstride = (int64_t)C * T;
  const int q = lane >> 4, li = lane & 15;
  const int row = quad * 4 + q < n_rows ? quad * 4 + q : n_rows - 1;
  const float* src = x + row * (int64_t)T;
  for (int e = lane; e < kRows4Bands * kMaxSec * 8; e += 64) carry[e] = 0.0;
  wave_lds_sync();
  int64_t ybase[4];                                     // band 0 of each row of the quad (wave-uniform)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = quad * 4 + r < n_rows ? quad * 4 + r : n_rows - 1;
    ybase[r] = ((int64_t)(rr / C) * nb_out * C + (rr % C)) * (int64_t)T;
  }
  auto load_x = [&](XArr& xs, int it) {
    float4 xf[kL / 4];
    chunk_issue<true>(xf, src, 0, it * 16 + li, T);
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) xs[j] = (f2){f4_get(xf[j >> 2], j & 3), f4_get(xf[(j >> 2) + 4], j & 3)};
  };
  auto filter_store = [&](const XArr& xs, int it, int b, int bi) {
    typename O::Arr v;
    O::from_x(v, xs, O::g(bands[b]));
    double* cb = carry + (bi * kMaxSec * 4 + q) * 2;
    for (int sct = 0; sct < ns; ++sct) {
      double c1 = cb[sct * 8], c2 = cb[sct * 8 + 1];
      section<VT, 1, true>(v, secs[b * ns + sct], Qtab + (int64_t)(b * ns + sct) * 64, lane, c1, c2);
      wave_lds_sync();                                  // every lane has read the incoming carry
      if (li == 15) {
        cb[sct * 8] = c1;
        cb[sct * 8 + 1] = c2;
      }
    }
    // transposition to coalesced stores: rows 2 h and 2 h + 1 of the quad (32 chunks) at a time
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      wave_lds_sync();                                  // the previous half's readers are done
      if ((lane >> 5) == h) chunk_to_tile<VT>(tile + (lane & 31) * kPad, v);
      wave_lds_sync();
      // the four tile reads first, then the four stores (a test between a read and its store leaves each pair in
      // its own basic block behind its own wait); rows past the end are a whole quad's tail: wave-uniform
      float4 val[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = (k * 64 + lane) * 4;              // element inside the half tile: chunk e >> 5, sample e & 31
        val[k] = *reinterpret_cast<const float4*>(tile + (e >> 5) * kPad + (e & 31));
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rr = quad * 4 + 2 * h + (k >> 1);
        if (!FULLQ && rr >= n_rows) continue;
        const int64_t rbase = FULLQ ? ybase[2 * h + (k >> 1)] : ((int64_t)(rr / C) * nb_out * C + (rr % C)) * (int64_t)T;
        float* dst = y + rbase + (int64_t)bmap[b] * bstride;
        store_stream4(dst + it * kSeg + (((k * 64 + lane) * 4) & (kSeg - 1)), val[k]);
      }
    }
  };
  if (PASS_OUTER) {
    for (int it = 0; it < n_iter; ++it) {
      XArr xs;
      load_x(xs, it);
      int bi = 0;
      for (int b = share; b < nb; b += share_n, ++bi) filter_store(xs, it, b, bi);
    }
  } else {
    // fp64: the 16 registers of a pass of x held across the bands cost the instance a wave per SIMD (184 VGPRs, 1.62 ->
    // 1.87 ms per 128 stress trials); it re-reads the pass per band instead
    int bi = 0;
    for (int b = share; b < nb; b += share_n, ++bi) {
      for (int it = 0; it < n_iter; ++it) {
        XArr xs;
        load_x(xs, it);
        filter_store(xs, it, b, bi);
      }
    }
  }
}
template <bool FULLQ>
__global__ __launch_bounds__(64) void fb_rows4_kernel_f32(
    const FbSec* __restrict__ secs, const FbBand* __restrict__ bands, const double* __restrict__ Qtab,
    const float* __restrict__ x, float* __restrict__ y, int C, int T, int nb, int ns,
    const int* __restrict__ bmap, int nb_out, int n_rows, int share_n) {
  fb_rows4_body<float, true, FULLQ>(secs, bands, Qtab, x, y, C, T, nb, ns, bmap, nb_out, n_rows, share_n);
}
template <bool FULLQ>
__global__ __launch_bounds__(64) void fb_rows4_kernel_f64(
    const FbSec* __restrict__ secs, const FbBand* __restrict__ bands, const double* __restrict__ Qtab,
    const float* __restrict__ x, float* __restrict__ y, int C, int T, int nb, int ns,
    const int* __restrict__ bmap, int nb_out, int n_rows, int share_n) {
  fb_rows4_body<double, false, FULLQ>(secs, bands, Qtab, x, y, C, T, nb, ns, bmap, nb_out, n_rows, share_n);
}

struct FusedBands {
  int klo[kMaxBands];
  int khi[kMaxBands];
  float inv[kMaxBands];          // 1 / (number of bins), 0 for an empty band
};

// log(P + eps) on the hardware log2 (v_log_f32, 1 ulp): |error| <= 2e-6 in the log domain for P + eps >= 1e-10,
// against the 1e-4 feature gate; the libm logf costs ~20 instructions per value and every band needs two.
__device__ __forceinline__ float fast_log(float v) { return __builtin_amdgcn_logf(v) * 0.69314718055994531f; }


// Windowed DFT of the band's own bins over the lane's chunk (register pairs) and the reduction to
// band magnitude / power.  Frame j of the row is chunk j-1 (first window half, table entries 0..31)
// followed by chunk j (second half, 32..63): every lane forms both partial sums, `row_shr:1` joins
// neighbours.  o0 = frame (lane & 15), o16 = frame 16 (meaningful on lane 15).
// MAG: mean magnitude (a square root per bin and frame) instead of mean power -- a template parameter because the
// compiler turns the run-time test into selects and evaluates both square roots (a third of the loop) either way.
// GPR: 16-lane groups per row (1: rows of <= 512 samples, frame 16 on lane 15; 2: <= 1024 samples, the neighbour join
// crosses the DPP row boundary and frame 32 sits on lane 31 of the row's 32 lanes).
template <bool MAG, int GPR = 1>
__device__ __forceinline__ void band_reduce_pairs(const f2 (&vf)[kL / 2], const float2* __restrict__ dft, int klo,
                                                  int khi, bool mine_lo_hi_valid, int my_klo, int my_khi, float scale2,
                                                  float& o0, float& o16, bool row_start = false) {
  float acc = 0.f, acc16 = 0.f;
  for (int k = klo; k <= khi; ++k) {
    const f2* __restrict__ tb = reinterpret_cast<const f2*>(dft + k * 64);   // [4][16] sample-pair entries (stft.hip)
    // four real dot products over the lane's 32 samples: first / second window half x real / imaginary part; each
    // accumulates the j-part and the (j + 16)-part in the two lanes of a packed register
    f2 a1r = {0.f, 0.f}, a1i = {0.f, 0.f}, a2r = {0.f, 0.f}, a2i = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < kL / 2; q += 8) {
      const f2* __restrict__ tq = later(tb);          // 64 table scalars per batch in the SGPR file
#pragma unroll
      for (int j = q; j < q + 8; ++j) {
        const f2 pr = vf[j];                          // samples j, j + 16
        a1r = __builtin_elementwise_fma(pr, tq[j], a1r);
        a1i = __builtin_elementwise_fma(pr, tq[16 + j], a1i);
        a2r = __builtin_elementwise_fma(pr, tq[32 + j], a2r);
        a2i = __builtin_elementwise_fma(pr, tq[48 + j], a2i);
      }
    }
    const f2 p1 = {a1r.x + a1r.y, a1i.x + a1i.y}, p2 = {a2r.x + a2r.y, a2i.x + a2i.y};
    float nr, ni;                                         // first-half sums of the previous chunk of the row
    if (GPR == 1) {
      nr = row_shr<1>(p1.x); ni = row_shr<1>(p1.y);
    } else {
      nr = wave_shr1(p1.x); ni = wave_shr1(p1.y);
      nr = row_start ? 0.f : nr; ni = row_start ? 0.f : ni;
    }
    const float zr = p2.x + nr, zi = p2.y + ni;
    float pw = (zr * zr + zi * zi) * scale2;
    float pw16 = (p1.x * p1.x + p1.y * p1.y) * scale2;
    if (MAG) { pw = sqrtf(pw); pw16 = sqrtf(pw16); }
    const bool in = !mine_lo_hi_valid || (k >= my_klo && k <= my_khi);
    acc += in ? pw : 0.f;
    acc16 += in ? pw16 : 0.f;
  }
  o0 = acc;
  o16 = acc16;
}

// the STFT sees y[0..T) then zeros, not the filter's ringing
__device__ __forceinline__ void zero_past_end(XArr& vf, int i, int T) {
#pragma unroll
  for (int j = 0; j < kL / 2; ++j) {
    if (i * kL + j >= T) vf[j].x = 0.f;
    if (i * kL + j + 16 >= T) vf[j].y = 0.f;
  }
}

// Band aggregation of materialised filtered signals y[B][nb][C][T] (nperseg 64 / hop 32, T <= 512):
// same chunk layout as the filterbank (coalesced float4 loads through the LDS tile), direct DFT of
// each row's own band bins.  HBM-bound: reads nb*C*T*4 bytes per trial, writes nb*C*J*4.
template <bool MAG, bool FULL = false>
__global__ __launch_bounds__(64) void bandpower_direct_kernel(const float2* __restrict__ dft,
                                                              const float* __restrict__ y, float* __restrict__ feat,
                                                              int R, int C, int T, int nb, int J, float scale2,
                                                              FusedBands fbnd, int mode, float eps, int vec) {
  __shared__ __attribute__((aligned(16))) float tile[4 * 16 * kPad];
  const int lane = threadIdx.x;
  const int i = lane & 15;
  const int row0 = blockIdx.x * 4;
  int64_t xbase[4];
  int gt0[4];
  int wlo = 1 << 30, whi = -1;                                  // wave-uniform union of the 4 rows' bin ranges
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    gt0[g] = 0;
    const int r = row0 + g;
    xbase[g] = (r < R) ? r * (int64_t)T : -1;
    if (r < R) {
      const int band = (r / C) % nb;
      if (fbnd.khi[band] >= fbnd.klo[band]) {
        wlo = fbnd.klo[band] < wlo ? fbnd.klo[band] : wlo;
        whi = fbnd.khi[band] > whi ? fbnd.khi[band] : whi;
      }
    }
  }
  XArr vf;
  load_chunks<FULL>(vf, tile, y, lane, xbase, gt0, T, vec != 0);
  if (T < kSeg) zero_past_end(vf, i, T);
  const int row = row0 + (lane >> 4);
  const int band = (row / C) % nb;
  const int klo = fbnd.klo[band], khi = fbnd.khi[band];
  float o0, o16;
  band_reduce_pairs<MAG>(vf, dft, wlo, whi, true, klo, khi, scale2, o0, o16);
  const float inv = fbnd.inv[band];
  o0 *= inv;
  o16 *= inv;
  if (mode == ISD_BP_LOGPOWER) { o0 = fast_log(o0 + eps); o16 = fast_log(o16 + eps); }
  if (row < R) {
    float* o = feat + row * (int64_t)J;                         // feat has the same [B][nb][C] row order as y
    if (i < J) o[i] = o0;
    if (i == 15 && J == 17) o[16] = o16;
  }
}

// Fused spec-S extractor for T <= 1024 (GPR = 1: T <= 512; GPR = 2: the reference-native 800-sample trial,
// src/fast/data/preprocess.py:62), nperseg 64 / hop 32: after the cascade each lane
// holds chunk i of its row; STFT frame j is chunk j-1 (window first half) followed by
// chunk j (second half), so every lane forms two partial windowed DFT sums per bin and
// one DPP row_shr joins neighbours.  Only the band's own bins are evaluated.
// Everything that does not depend on the band (the row's trial / channel split -- an integer division -- and its
// output address) is computed once in front of the band loop: inside it the compiler does not hoist them out of the
// `row < R` branch, and they were a tenth of the loop's instructions.
template <typename VT, bool MAG, int GPR, bool FULL>
__global__ __launch_bounds__(64) void fused_kernel(const FbSec* __restrict__ secs, const FbBand* __restrict__ bands,
                                                   const double* __restrict__ Qtab,
                                                   const float2* __restrict__ dft, const float* __restrict__ x,
                                                   float* __restrict__ feat, int R, int C, int T, int nb, int ns,
                                                   int J, float scale2, FusedBands fbnd, int mode, float eps,
                                                   int vec, const int* __restrict__ bmap, int nb_out, int out16) {
  using O = VOps<VT>;
  static_assert(GPR == 1 || GPR == 2, "rows of at most 1024 samples");
  __shared__ __attribute__((aligned(16))) float tile[4 * 16 * kPad];
  const int lane = threadIdx.x;
  constexpr int LPR = 16 * GPR;                             // lanes (= 32-sample chunks) per row
  const int i = lane & (LPR - 1);
  const int row0 = blockIdx.x * (4 / GPR);
  int64_t xbase[4];
  int gt0[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    gt0[g] = (g % GPR) * kSeg;
    const int r = row0 + g / GPR;
    xbase[g] = (r < R && gt0[g] < T) ? r * (int64_t)T : -1;
  }
  const int row = row0 + lane / LPR;
  const bool row_ok = row < R;
  const int bt = row / C, ch = row - bt * C;
  const int64_t oidx = ((int64_t)bt * nb_out * C + ch) * (int64_t)J + i;        // band 0, frame i of this lane's row
  float* const orow = feat + oidx;
  // out16 (BASELINE config 3): the feature map leaves as bf16 (RNE) -- the rounding the bf16 first layer (and the
  // reference's autocast, which casts the convolution's input) applies anyway, half the bytes for the classifier to read
  unsigned short* const orow16 = reinterpret_cast<unsigned short*>(feat) + oidx;
  const int64_t bstride = (int64_t)C * J;
  const bool st0 = row_ok && i < J, st16 = row_ok && i == LPR - 1 && J == LPR + 1;
  XArr xs;
  load_chunks<FULL>(xs, tile, x, lane, xbase, gt0, T, vec != 0);
#ifdef ISD_MFMA_PROBE
  typedef float f32x4p __attribute__((ext_vector_type(4)));
  f32x4p probe[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#endif
  for (int b = 0; b < nb; ++b) {
    typename O::Arr v;
    O::from_x(v, xs, O::g(bands[b]));
    for (int s = 0; s < ns; ++s) {
      double c1 = 0.0, c2 = 0.0;
      section<VT, GPR>(v, secs[b * ns + s], GPR > 1 ? Qtab + (int64_t)(b * ns + s) * 64 : nullptr, lane, c1, c2);
    }
    XArr vf;                                          // fp32 copy for the DFT (the chunk itself when VT is fp32)
    O::to_f32(v, vf);
    if (!FULL && T < LPR * kL) zero_past_end(vf, i, T);   // FULL: T == LPR * kL
#ifdef ISD_MFMA_PROBE
    // Measurement build (ISD_HIPCC_FLAGS=-DISD_MFMA_PROBE=32, tools/mfma_probe.sh): the matrix-pipe load a
    // band DFT on the matrix cores would add -- ISD_MFMA_PROBE v_mfma_f32_16x16x4_f32 per band and wave on live
    // registers, four independent accumulators -- issued BESIDE the unchanged vector code: what co-issue costs the
    // VALU-bound kernel, before anything is saved.
#pragma unroll
    for (int pi = 0; pi < ISD_MFMA_PROBE; ++pi)
      probe[pi & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[pi & 15].x, vf[(pi + 5) & 15].y, probe[pi & 3], 0, 0, 0);
#endif
    float o0, o16;
    band_reduce_pairs<MAG, GPR>(vf, dft, fbnd.klo[b], fbnd.khi[b], false, 0, 0, scale2, o0, o16, i == 0);
    const float inv = fbnd.inv[b];
    o0 *= inv;
    o16 *= inv;
    if (mode == ISD_BP_LOGPOWER) { o0 = fast_log(o0 + eps); o16 = fast_log(o16 + eps); }
    if (out16) {
      unsigned short* o = orow16 + (int64_t)bmap[b] * bstride;
      unsigned pk;                                      // both values in one gfx950 conversion (RNE)
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(o0), "v"(o16));
      if (st0) o[0] = (unsigned short)pk;
      if (st16) o[1] = (unsigned short)(pk >> 16);
    } else {
      float* o = orow + (int64_t)bmap[b] * bstride;
      if (st0) o[0] = o0;
      if (st16) o[1] = o16;
    }
  }
#ifdef ISD_MFMA_PROBE
  {                                                   // keeps the probe's accumulators alive; never true
    const float ps = probe[0][0] + probe[1][1] + probe[2][2] + probe[3][3];
    if (ps == 1.2345678e30f && row_ok) feat[0] = ps;
  }
#endif
}

// Fused spec-S extractor for long rows with heavily overlapped frames (stress configuration: 4096 samples,
// nperseg 1024, hop 64): the filterbank cascade of fb_long_kernel (one row per wave, 2048 samples per pass, the
// section states carried across passes) followed, in registers, by the per-block DFT sums of the block-sum band
// power (stft.hip): every lane holds half of a 64-sample block, forms the half-block sums of the band's bins and
// their two neighbours, lane pairs are joined by one DPP shift and the 64 block sums of the row wait in LDS for
// blocksum_finish.  The filtered rows (86 MB per trial at the stress shape) are never written.
// The x row is re-read from global memory for every band and pass, and kLongShare one-wave workgroups share a row
// (each takes every kLongShare-th band).  Their ids are congruent mod 8 -- workgroups go to the 8 XCDs round-robin
// by id, and each XCD has its own L2 -- and lie within 64 consecutive ids, so the sharers run on one XCD at about
// the same time and the rows in flight there (~80 x 16 KiB) fit its 4 MiB L2.  With one workgroup per row walking
// all bands the rows in flight were ~10x the L2: the PMC counters showed 6.1 GB through the fabric for a 268 MB input.
template <typename VT, int KB, bool VEC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(std::is_same<VT, float>::value && KB <= 5 ? 5 : 4)))
void fused_long_kernel(const FbSec* __restrict__ secs, const FbBand* __restrict__ bands,
                                                        const double* __restrict__ Qtab, const float2* __restrict__ blk,
                                                        const float* __restrict__ x, float* __restrict__ feat, int C,
                                                        int T, int nb, int ns, int J, int log2_nblk, int n_bins_max,
                                                        float scale2, FusedBands fbnd, int mode, float eps,
                                                        const int* __restrict__ bmap, int nb_out, int n_rows,
                                                        int out16) {
  using O = VOps<VT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int n_iter = (T + 4 * kSeg - 1) / (4 * kSeg);
  float2* Sblk = reinterpret_cast<float2*>(smem_raw);                      // [KB][64]
  float2* tw = Sblk + KB * 64;                                             // [64]  e^{-2 pi i u / nblk}
  double* carry = reinterpret_cast<double*>(tw + 64);                      // [kMaxSec][2]
  double* Qlds = carry + kMaxSec * 2;                                      // [kMaxSec][16][4] the band's per-lane M^i
  // id = 8 kLongShare q + 8 w + c  <->  row = 8 q + c, band subset w
  const int id = blockIdx.x;
  const int row = (id / (8 * kLongShare)) * 8 + (id & 7);
  const int share = (id >> 3) % kLongShare;
  if (row >= n_rows) return;
  const int bt = row / C;
  const int ch = row - bt * C;
  const int nblk = 1 << log2_nblk;
  const float* src = x + row * (int64_t)T;
  if (lane < nblk) {
    float sn, cs;
    sincospif(2.f * (float)lane / (float)nblk, &sn, &cs);
    tw[lane] = make_float2(cs, -sn);
  }
  wave_lds_sync();
  const int lane0 = lane;
  for (int b = share; b < nb; b += kLongShare) {
    // lane-derived addresses are recomputed per band instead of staying live across the whole kernel: hoisted, they
    // were what the fp64 instance spilled to scratch at its 128-register cap (13 dwords per lane, written once per
    // wave: 436 MB of scratch writes per 128 trials for 68 MB of features)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int klo = fbnd.klo[b], khi = fbnd.khi[b];
    const int k0 = klo - 1, nbin = khi - klo + 1;
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) Sblk[kk * 64 + lane] = make_float2(0.f, 0.f);
    if (lane < ns * 2) carry[lane] = 0.0;
    stage_q(Qlds, Qtab, b, ns, lane);
    wave_lds_sync();
    const auto gain = O::g(bands[b]);
    for (int it = 0; it < n_iter; ++it) {
      // the lane's 32 samples straight from global memory (the row is re-read once per band and stays in L2 / MALL):
      // a row staged in LDS would cost 18 KiB per wave and hold the CU at 7 waves
      typename O::Arr v;
      {
        float4 xf[kL / 4];
        chunk_issue<VEC>(xf, src, it, lane, T);
        XArr xs;
        chunk_finish(xs, xf, it, lane, T);
        O::from_x(v, xs, gain);
      }
      for (int sct = 0; sct < ns; ++sct) {
        double c1 = carry[sct * 2], c2 = carry[sct * 2 + 1];
        section<VT, 4>(v, secs[b * ns + sct], Qlds + sct * 64, lane, c1, c2);
        wave_lds_sync();                                // every lane has read the incoming carry
        if (lane == 0) {
          carry[sct * 2] = c1;
          carry[sct * 2 + 1] = c2;
        }
      }
      wave_lds_sync();
      // the STFT sees y[0..T) then zeros, not the filter's ringing
      const int base = (it * 64 + lane) * kL;
      float vf[kL];
#pragma unroll
      for (int n = 0; n < kL; ++n) vf[n] = (float)O::at(v, n);
      if ((it + 1) * 64 * kL > T) {                     // only the last pass of a ragged row (wave-uniform)
#pragma unroll
        for (int n = 0; n < kL; ++n) vf[n] = base + n < T ? vf[n] : 0.f;
      }
      // half-block DFT sums with block-local phase (this lane's 32 samples start at offset 32*(lane&1) in the block)
      float2 P[KB];
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) {
        __builtin_amdgcn_sched_barrier(0);              // one bin's 64 table scalars at a time in the SGPR file
        const int k = k0 + kk < n_bins_max ? k0 + kk : n_bins_max;
        const float2* tb = blk + (int64_t)k * 64;
        f2 acc = {0.f, 0.f}, acc_b = {0.f, 0.f};
#pragma unroll
        for (int n = 0; n < kL; n += 2) {             // two chains: a dependent v_pk_fma costs a wait state each
            acc = __builtin_elementwise_fma((f2){vf[n], vf[n]}, (f2){tb[n].x, tb[n].y}, acc);
            acc_b = __builtin_elementwise_fma((f2){vf[n + 1], vf[n + 1]}, (f2){tb[n + 1].x, tb[n + 1].y}, acc_b);
          }
          acc += acc_b;
        const float2 ph = tb[kL];                       // e^{-2 pi i k 32 / n}: the odd lane's offset in the block
        P[kk] = (lane & 1) ? make_float2(acc.x * ph.x - acc.y * ph.y, acc.x * ph.y + acc.y * ph.x)
                           : make_float2(acc.x, acc.y);
      }
      const int m = it * 32 + (lane >> 1);
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) {
        const float sx = P[kk].x + row_shl<1>(P[kk].x), sy = P[kk].y + row_shl<1>(P[kk].y);
        if (!(lane & 1)) Sblk[kk * 64 + m] = make_float2(sx, sy);
      }
    }
    wave_lds_sync();
    float2 S[KB];
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) S[kk] = Sblk[kk * 64 + lane];
    // out16: feat is the bf16 map [B][nb_out][C][J] (byte offset formed as in fused_serial_kernel)
    const int64_t oi = (((int64_t)bt * nb_out + bmap[b]) * C + ch) * (int64_t)J;
    blocksum_finish<KB>(S, tw, lane, k0, nbin, nblk, J, scale2, mode, eps,
                        reinterpret_cast<char*>(feat) + (oi << (out16 ? 1 : 2)), out16);
    wave_lds_sync();
  }
}

// Dynamic LDS of fused_long_kernel: block sums [KB][64] and twiddles, then the carried states and the per-lane M^i
static size_t fused_long_lds(int KB) {
  return sizeof(float2) * ((size_t)KB * 64 + 64) + sizeof(double) * (2 * kMaxSec + 64 * kMaxSec);
}

// Real sample x complex twiddle into a (re, im) accumulator, the sample taken from the LOW / HIGH half of a register
// pair and the twiddle from an SGPR pair.  Written as (f2){s, s} * t the compiler materialises the duplicated pairs
// (a v_mov per sample and 64 more live registers); the packed FMA's operand selects do the broadcast for nothing.
__device__ __forceinline__ void cmac_lo(f2& acc, const f2& pr, const f2& t) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(pr), "s"(t));
}
__device__ __forceinline__ void cmac_hi(f2& acc, const f2& pr, const f2& t) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(pr), "s"(t));
}
// x * g on the plain (unpacked) multiplier, opaque to the SLP vectoriser: written into one half of a register pair it
// needs no copy, where packing two loaded dwords for a v_pk_mul costs a v_mov each
__device__ __forceinline__ float mul_unpacked(float x, float g) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(g));
  return r;
}
// {hi(p) + lo(q), hi(p) - lo(q)}: the sum and the difference of the two samples that lie symmetrically about the middle
// of a lane's chunk (pairs hold {sample j, sample j + 16}: sample 16 + m is hi(pair m), sample 16 - m is lo(pair 16 - m))
__device__ __forceinline__ f2 sym_pair(const f2& p, const f2& q) {
  f2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(p), "v"(q));
  return r;
}
// acc += ad * t elementwise: {sum, difference} x {cos, -sin} of the pair's angle, the table entry in an SGPR pair
__device__ __forceinline__ void pmac(f2& acc, const f2& ad, const f2& t) {
  asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(ad), "s"(t));
}
// ad * t + 0: the first term of a sum (the same fma as pmac on a zeroed accumulator, without the v_mov_b64 of the zeros)
__device__ __forceinline__ f2 pmac0(const f2& ad, const f2& t) {
  f2 acc;
  asm("v_pk_fma_f32 %0, %1, %2, 0" : "=v"(acc) : "v"(ad), "s"(t));
  return acc;
}
// u.x += hi(p), in place (written as a vector add, the compiler issued a v_pk_add and a v_mov for the untouched half)
__device__ __forceinline__ void add_lo(f2& u, const f2& p) {
  float x = u.x;
  asm("v_add_f32 %0, %0, %1" : "+v"(x) : "v"(p.y));
  u.x = x;
}
// acc += lo(pr) * conj(t)
__device__ __forceinline__ void cmac_lo_conj(f2& acc, const f2& pr, const f2& t) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "+v"(acc) : "v"(pr), "s"(t));
}

// The same extraction with FOUR ROWS PER WAVE (rows of a multiple of 512 samples, at most 16 blocks per frame): every
// 16-lane group walks its own row in 512-sample passes and carries its section states from pass to pass.  In
// fused_long_kernel the wave's four groups hold consecutive quarters of one 2048-sample pass and their end states are
// chained serially per section -- 16 v_readlane, 16 uniform fp64 FMAs and 12 selects on top of the 136-instruction
// section body of a kernel that is VALU-issue bound (PMC: 1 447 vector instructions per band and pass, 100 % of the
// launch at 4 cycles each).  Groups that own their rows need none of it: the carry is two doubles per (section,
// group) in LDS.  The frames are finished as the row streams by: a frame is the sum of nblk consecutive block sums,
// so after every SECOND pass the sixteen frames whose last block has arrived are formed from a 32-block ring per
// (row, bin), one frame per lane of the row's group -- keeping all 64 blocks of four rows until the end of the band
// cost 10 KiB of LDS and two waves per SIMD.
//
// Round 3 (the kernel is VALU-issue bound: 1 228 vector instructions per band and pass, 95 useful flops each):
//  * the lane's 128 bytes of a pass come as eight float4 loads off ONE address with immediate offsets, and the gain
//    multiply writes the register pairs directly (mul_unpacked): 42 v_mov + 32 address instructions + 16 v_pk_mul
//    became 32 v_mul + 4;
//  * the half-block DFT sums take the sample from a pair half by operand select (cmac_lo / cmac_hi) instead of from a
//    duplicated pair: -49 v_mov per pass and 32 fewer live registers; the table comes through SMEM in opaque-offset
//    batches (later()) like fused_kernel's;
//  * the odd lane's half-block rotation e^{-2 pi i k 32 / n} and the block's absolute phase e^{-2 pi i k m / nblk} are
//    ONE per-lane factor per bin, looked up once per band (it changes sign from pass to pass for odd bins at 16 blocks
//    per frame: one v_xor per component): a complex multiply instead of two plus an index computation per bin and pass;
//  * frames are finished every second pass, sixteen at a time (one per lane, no half-window join).
//  * NS > 0 (the section count as a template parameter; fp32 instance): the section states a group carries from pass
//    to pass stay in registers -- lane 15 of the group holds the new state after the scan and one DPP row broadcast
//    per dword hands it to the group's lanes -- instead of going through LDS (a write, a wait and a read per section
//    and pass).  NS == 0: any section count, states in LDS (the fp64 instance is at its register cap).
template <typename VT, int KB, int NS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(std::is_same<VT, float>::value ? 4 : 3)))
void fused_rows4_kernel(const FbSec* __restrict__ secs, const FbBand* __restrict__ bands,
                        const double* __restrict__ Qtab, const float2* __restrict__ blk,
                        const float* __restrict__ x, float* __restrict__ feat, int C,
                        int T, int nb, int ns, int J, int log2_nblk, int n_bins_max,
                        float scale2, FusedBands fbnd, int mode, float eps,
                        const int* __restrict__ bmap, int nb_out, int n_rows, int share_n, int out16) {
  using O = VOps<VT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane0 = threadIdx.x;
  const int n_iter = T / kSeg;                                             // 512-sample passes
  float2* ring = reinterpret_cast<float2*>(smem_raw);                      // [4 rows][KB][32]: block m at m & 31
  float2* tw = ring + 4 * KB * 32;                                         // [64]  e^{-2 pi i u / (4 nblk)}, u < 4 nblk
  double* carry = reinterpret_cast<double*>(tw + 64);                      // [ns][4 groups][2]
  double* Qlds = carry + ns * 8;                                           // [ns][16][4] the band's per-lane M^i
  // id = 8 share_n q + 8 w + c  <->  row quad = 8 q + c, band subset w (the sharers of a quad run on one XCD);
  // share_n = rows4_share(nb): 35 bands -> 7 sharers x 5 bands, 5 bands -> 5 x 1 (no idle band slots)
  const int id = blockIdx.x;
  const int quad = (id / (8 * share_n)) * 8 + (id & 7);
  const int share = (id >> 3) % share_n;
  if (quad * 4 >= n_rows) return;
  const int nblk = 1 << log2_nblk, nblk4 = 4 * nblk;                       // nblk <= 16: the table fits its 64 entries
  if (lane0 < nblk4) {
    float sn, cs;
    sincospif(2.f * (float)lane0 / (float)nblk4, &sn, &cs);
    tw[lane0] = make_float2(cs, -sn);
  }
  wave_lds_sync();
  for (int b = share; b < nb; b += share_n) {
    int lane = lane0;                                    // lane-derived addresses are re-formed per band (see above)
    asm volatile("" : "+v"(lane));
    const int q = lane >> 4, li = lane & 15;
    const bool row_ok = quad * 4 + q < n_rows;
    const int row = row_ok ? quad * 4 + q : n_rows - 1;                    // a missing row recomputes the last one
    const float4* src4 = reinterpret_cast<const float4*>(x + row * (int64_t)T + li * kL);
    const int bt = row / C, ch = row - bt * C;
    // out16: feat is the bf16 map [B][nb_out][C][J] (byte offset formed as in fused_serial_kernel)
    char* out = reinterpret_cast<char*>(feat) + ((((int64_t)bt * nb_out + bmap[b]) * C + ch) * (int64_t)J << (out16 ? 1 : 2));
    const int klo = fbnd.klo[b], khi = fbnd.khi[b];
    const int k0 = klo - 1, nbin = khi - klo + 1;
    if (NS == 0 && lane < ns * 8) carry[lane] = 0.0;
    [[maybe_unused]] double creg[NS ? NS : 1][2];
#pragma unroll
    for (int e = 0; e < (NS ? NS : 1); ++e) creg[e][0] = creg[e][1] = 0.0;
#pragma unroll
    for (int e = 0; e < 2 * KB; ++e) ring[e * 64 + lane] = make_float2(0.f, 0.f);      // 4 x KB x 32 slots
    stage_q(Qlds, Qtab, b, ns, lane);
    // this lane's factor per bin: block phase e^{-2 pi i k m / nblk} of its block m = 8 it + (li >> 1) at it = 0, times
    // the half-block offset e^{-2 pi i k 32 / n} on odd lanes, times the rotation e^{-2 pi i k 16 / n} about the middle
    // of the lane's chunk (the symmetric DFT sums below): k (2 li + 1) steps of 1 / (4 nblk) turns; pass it multiplies by
    // e^{-2 pi i k 8 it / nblk} = +-1.  The fp32 instance keeps the KB factors in registers; the fp64 instance, which
    // is at its register cap, looks them up per pass.
    constexpr bool kFacRegs = std::is_same<VT, float>::value;
    f2 fac[kFacRegs ? KB : 1];
    unsigned flip[kFacRegs ? KB : 1];                    // wave-uniform: sign bit when the factor alternates
    if constexpr (kFacRegs) {
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) {
        const int kq = k0 + kk;
        const float2 w = tw[(kq * (2 * li + 1)) & (nblk4 - 1)];
        fac[kk] = (f2){w.x, w.y};
        flip[kk] = ((32 * kq) & (nblk4 - 1)) ? 0x80000000u : 0u;          // 16 k / (2 nblk) turns per pass: 0 or 1/2
      }
    }
    wave_lds_sync();
    const auto gain = O::g(bands[b]);
    for (int it = 0; it <= n_iter; ++it) {
      if (it == n_iter && !(lane & 1)) {                 // the eight blocks past the end of the row: zeros
        const int sl = (it * 8 + (li >> 1)) & 31;
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) ring[(q * KB + kk) * 32 + sl] = make_float2(0.f, 0.f);
      }
      if (it < n_iter) {
        typename O::Arr v;
        {
          float4 xf[kL / 4];
          const float4* p4 = src4 + it * (kSeg / 4);     // one address, eight immediate offsets
#pragma unroll
          for (int e = 0; e < kL / 4; ++e) xf[e] = p4[e];
          if constexpr (std::is_same<VT, float>::value) {
#pragma unroll
            for (int j = 0; j < kL / 2; ++j)
              v[j] = (f2){mul_unpacked(f4_get(xf[j >> 2], j & 3), gain), mul_unpacked(f4_get(xf[(j >> 2) + 4], j & 3), gain)};
          } else {
#pragma unroll
            for (int j = 0; j < kL / 2; ++j) {
              v[j] = (double)f4_get(xf[j >> 2], j & 3) * gain;
              v[j + 16] = (double)f4_get(xf[(j >> 2) + 4], j & 3) * gain;
            }
          }
        }
        if constexpr (NS > 0) {
#pragma unroll
          for (int sct = 0; sct < NS; ++sct) {
            double c1 = creg[sct][0], c2 = creg[sct][1];
            section<VT, 1, true>(v, secs[b * NS + sct], Qlds + sct * 64, lane, c1, c2);
            creg[sct][0] = row_bcast15(c1);             // the state leaving the pass sits on lane 15 of the group
            creg[sct][1] = row_bcast15(c2);
          }
        } else {
          for (int sct = 0; sct < ns; ++sct) {
            double c1 = carry[(sct * 4 + q) * 2], c2 = carry[(sct * 4 + q) * 2 + 1];
            section<VT, 1, true>(v, secs[b * ns + sct], Qlds + sct * 64, lane, c1, c2);
            wave_lds_sync();                            // every lane has read the incoming carry
            if (li == 15) {
              carry[(sct * 4 + q) * 2] = c1;
              carry[(sct * 4 + q) * 2 + 1] = c2;
            }
          }
        }
        XArr vf;                                        // fp32 pairs {sample j, sample j + 16} (the chunk itself in fp32)
        O::to_f32(v, vf);
        // half-block DFT sums with block-local phase (this lane's 32 samples start at offset 32 (lane & 1) in the block).
        // The 32 samples are taken in pairs symmetric about sample 16:
        //   sum_n y[n] e^{-i th n} = e^{-i 16 th} [ y[16] + y[0] e^{+i 16 th} + sum_{m=1..15} (a_m cos(m th) - i d_m sin(m th)) ],
        //   a_m = y[16 + m] + y[16 - m],  d_m = y[16 + m] - y[16 - m]:
        // one packed add per pair, shared by the bins, then ONE packed FMA per pair and bin ({a, d} x {cos, -sin}: the
        // table's own entry m) instead of two -- 17 instead of 32 per bin.  The rotation e^{-i 16 th} rides in the
        // lane's per-bin factor (tw4 index k (2 li + 1), below).
        const int sl = (it * 8 + (li >> 1)) & 31;
        f2 ad[15];
#pragma unroll
        for (int m = 1; m < 16; ++m) ad[m - 1] = sym_pair(vf[m], vf[16 - m]);
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
          const int k = k0 + kk < n_bins_max ? k0 + kk : n_bins_max;
          const f2* __restrict__ tb = reinterpret_cast<const f2*>(blk + (int64_t)k * 64);
          f2 acc_a = {0.f, 0.f}, acc_b = {0.f, 0.f};     // two chains
          {
            const f2* __restrict__ tq = later(tb);       // entries 1..8: 16 table scalars per batch in the SGPR file
#pragma unroll
            for (int m = 1; m <= 8; m += 2) {
              pmac(acc_a, ad[m - 1], tq[m]);
              pmac(acc_b, ad[m], tq[m + 1]);
            }
          }
          {
            const f2* __restrict__ tq = later(tb);       // entries 9..16
#pragma unroll
            for (int m = 9; m <= 13; m += 2) {
              pmac(acc_a, ad[m - 1], tq[m]);
              pmac(acc_b, ad[m], tq[m + 1]);
            }
            pmac(acc_a, ad[14], tq[15]);
            cmac_lo_conj(acc_b, vf[0], tq[16]);          // y[0] e^{+i 16 th}
          }
          f2 sum = acc_a + acc_b;
          sum.x += vf[0].y;                              // y[16]
          f2 fk;
          if constexpr (kFacRegs) {
            fk = fac[kk];
            fac[kk] = (f2){__uint_as_float(__float_as_uint(fk.x) ^ flip[kk]), __uint_as_float(__float_as_uint(fk.y) ^ flip[kk])};
          } else {
            const float2 w = tw[((k0 + kk) * (2 * (li + 16 * it) + 1)) & (nblk4 - 1)];
            fk = (f2){w.x, w.y};
          }
          float px = sum.x * fk.x - sum.y * fk.y, py = sum.x * fk.y + sum.y * fk.x;
          px += row_shl<1>(px);
          py += row_shl<1>(py);
          if (!(lane & 1)) ring[(q * KB + kk) * 32 + sl] = make_float2(px, py);
        }
      }
      if (!(it & 1) && it != n_iter) continue;           // frames are finished after every second pass (and the last)
      wave_lds_sync();
      // frames j = 8 it - 15 .. 8 it, one per lane of the group: their last block (j + half - 1 <= 8 it + 7) has arrived
      // or lies past the row, their first (j - half >= 8 it - 23) is still in the 32-block ring.  (After the last
      // pass of a row with an even number of passes the first eight of them are formed a second time.)
      {
        const int half = nblk >> 1;
        const int j = 8 * it - 15 + li;
        const int m0 = j - half;                         // this frame's nblk blocks: m0 .. m0 + nblk - 1
        // blocks before the row and past its end read as zero because their ring slots ARE zero (cleared at the start
        // of the band and, for the slots past the end, before the last round): no test per read
        const float2* rq = ring + q * KB * 32;
        f2 R[KB];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) R[kk] = (f2){0.f, 0.f};
        if (nblk == 16) {
#pragma unroll
          for (int d = 0; d < 16; ++d) {
            const int sl = (m0 + d) & 31;
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
              const float2 sv = rq[kk * 32 + sl];
              R[kk] += (f2){sv.x, sv.y};
            }
          }
        } else {
          for (int d = 0; d < nblk; ++d) {
            const int sl = (m0 + d) & 31;
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
              const float2 sv = rq[kk * 32 + sl];
              R[kk] += (f2){sv.x, sv.y};
            }
          }
        }
        const float2 wn = tw[(4 * j) & (nblk4 - 1)];                   // e^{-2 pi i j/nblk};  w^j = conj(wn)
        float acc = 0.f;
#pragma unroll
        for (int bq = 0; bq < KB - 2; ++bq) {
          if (bq < nbin) {
            const f2 lo = R[bq], mid = R[bq + 1], hi = R[bq + 2];
            const float sx = hi.x * wn.x + hi.y * wn.y + lo.x * wn.x - lo.y * wn.y;
            const float sy = hi.y * wn.x - hi.x * wn.y + lo.y * wn.x + lo.x * wn.y;
            const float vx = 0.5f * mid.x + 0.25f * sx, vy = 0.5f * mid.y + 0.25f * sy;
            const float pw = (vx * vx + vy * vy) * scale2;
            acc += mode == ISD_BP_MAGNITUDE ? sqrtf(pw) : pw;
          }
        }
        float r = nbin > 0 ? acc / (float)nbin : 0.f;
        if (mode == ISD_BP_LOGPOWER) r = logf(r + eps);
        if (row_ok && j >= 0 && j < J) store_feat(out, j, r, out16);
      }
      wave_lds_sync();                                   // the ring slots this round read may be overwritten next pass
    }
  }
}

// Dynamic LDS of fused_rows4_kernel: the block ring of four rows and the twiddles, then the carried states and the
// per-lane M^i of every section.  At most 8 (4 5 32 + 64) + 8 72 8 = 10240 bytes (KB <= 5, n_sections <= 8): far below
// the 48 KiB a kernel may use without raising its limit, so no launch sets the attribute.
static size_t fused_rows4_lds(int KB, int n_sections) {
  return sizeof(float2) * ((size_t)4 * KB * 32 + 64) + sizeof(double) * (8 + 64) * (size_t)n_sections;
}
static_assert(sizeof(float2) * (4 * 5 * 32 + 64) + sizeof(double) * (8 + 64) * kMaxSec == 10240, "rows4 LDS bound");

// ---------------------------------------------------------------------------------------------------------------
// Round 4: the fused spec-S extractor with ONE ROW PER LANE (rows of whole 32-sample chunks, nperseg 64 / hop 32).
//
// fused_kernel gives a 16-lane DPP row one (trial, channel) row and a lane one 32-sample chunk, so every biquad section
// pays for a lane scan of the chunk-end states: 16 v_fma_f64 + 24 DPP moves + the joins = 48 of the section body's 130
// vector instructions (ISA count, profiles/r04_fused_isa_counts.txt), in a kernel that is vector-issue bound.  Here a
// lane OWNS a row and walks it chunk by chunk: the state entering chunk c is simply the state that left chunk c - 1,
// carried in two fp64 registers per section -- S' = M S + e, four v_fma_f64 -- and there is no scan, no DPP and no
// cross-lane traffic at all.  The arithmetic of every sample is the arithmetic of fused_kernel / fb_kernel, operation
// for operation (fp32 zero-state recursion over the chunk's two 16-sample halves side by side in one register pair,
// the A^16 join in fp32, chunk-end states accumulated in fp64, fp32 state fix-up from the same tables), so the
// materialising path and this one still round alike; only the fp64 summation order of the carried state differs.
//
// Workgroup = 64 consecutive rows x NW waves; wave w runs bands w, w + NW, ... (at most BPW of them) and keeps their
// section states (8 doubles per band) and the previous chunk's half-frame DFT sums in registers.  The row chunks
// (64 rows x 128 bytes per step) are fetched once per workgroup, coalesced (eight lanes per row), through a
// double-buffered LDS tile with a 16-byte XOR swizzle (slot = quad ^ ((row >> 1) & 7): the loader's writes are
// contiguous kilobytes, the readers' ds_read_b128 -- lane = row -- hit every bank once per 16 lanes).
//
// Band power: the UNWINDOWED half-frame sums U_c[k] = sum_{n<32} y[32 c + n] e^{-2 pi i k n / 64} over sample pairs
// symmetric about the middle of the chunk ({y[16+m] + y[16-m], y[16+m] - y[16-m]} x {cos, -sin}: 17 packed FMAs per
// bin), frame j = U_{j-1} + (-1)^k U_j, and the periodic Hann window applied in the frequency
// domain, 0.5 X[k] - 0.25 (X[k-1] + X[k+1]).  The rotation e^{-i 16 th_k} = (-i)^k of the symmetric form is never
// applied: it cancels out of |.|^2 once the neighbours' relative rotations (+-i) are folded into the combination.
// Scalar tables by hand.  The section's constants (44 dwords: M = A^32 in fp64, A^16 and the 2 x 16 fix-up table in fp32)
// are fetched by explicit s_loads IN FRONT of the recursion and waited for behind it: the 64 packed instructions of the
// recursion cover the scalar-cache latency.  Left to the compiler the loads sink to their first use (its scheduler works
// bottom-up and prices a scalar load at a few cycles), which parked the wave twice per section -- PMC of the first
// version: 57 % of the wave cycles in s_waitcnt at three waves per SIMD.  The asm statements are volatile (they keep
// their order) and each carries a vector register of the arithmetic it must stay in front of / behind.
// 16 bytes per lane, global -> LDS (lds_base + 16 lane; lds_base wave-uniform), issued behind the compiler's back like
// conv.hip's dma16_async: through the builtin every later LDS access of the kernel would first wait for it.
__device__ __forceinline__ void ser_dma16(const void* src_lane, unsigned lds_base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :: "s"(__builtin_amdgcn_readfirstlane(lds_base)), "v"(src_lane) : "memory", "m0");
}

// One section over the lane's chunk.  All of the section's constants (48 dwords) come in ONE batch of scalar loads at
// the top -- the lane-scan kernels fetch them in three, each where it is needed, because the scan holds the SGPR file
// in between -- so a section parks its wave on the scalar cache once instead of three or four times (PMC of the first
// version of this kernel, three waves per SIMD: 57 % of the wave cycles in s_waitcnt, 34 waits per band and chunk).
// (Issuing the loads a stage AHEAD by hand does not work with this compiler: an inline-asm output of an SGPR vector
// type reads back as its first element in every lane of the vector -- hipcc 7.2, "=s" / "+s" on ext_vector_type(2..16)
// -- and left to itself the scheduler sinks scalar loads to their first use.)
// d = fma(a, b, c) into a register of the compiler's choice (the accumulating v_fmac ties d to c's register)
__device__ __forceinline__ float fma_to(float a, float b, float c) {
  float d;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "s"(a), "v"(b), "v"(c));
  return d;
}
// d = fma(a, b, c) over d, whose old value is dead (d = c2 of the carried state)
__device__ __forceinline__ void fma_over(double& d, double a, double b, double c) {
  asm("v_fma_f64 %0, %1, %2, %3" : "+v"(d) : "s"(a), "v"(b), "v"(c));
}
// d = fma(a, d, c) in place (d = c1 of the carried state)
__device__ __forceinline__ void fma_over_mid(double& d, double a, double c) {
  asm("v_fma_f64 %0, %1, %0, %2" : "+v"(d) : "s"(a), "v"(c));
}

__device__ __forceinline__ void section_serial_f32(f2 (&v)[kL / 2], const SerSec& sc0, double& c1, double& c2) {
  const SerSec& sc = *later(&sc0);
  const float na1 = -sc.a1, na2 = -sc.a2;
  const float n16[4] = {sc.N16[0], sc.N16[1], sc.N16[2], sc.N16[3]};
  const double m0 = sc.M[0], m1 = sc.M[1], m2 = sc.M[2], m3 = sc.M[3];
  float h0[kL / 2], h1[kL / 2];
#pragma unroll
  for (int j = 0; j < kL / 2; ++j) { h0[j] = sc.hq[0][j]; h1[j] = sc.hq[1][j]; }
  // y = x + S1 is issued as the packed FMA one * x + S1 -- the same value, bit for bit -- with `one` = 1.0f from the
  // section's table: hipcc's gfx940 "destination select" forwarding rule takes the default op_sel_hi bit of a packed
  // fp32 operation's FIRST source for a 16-bit partial write and puts an s_nop behind every v_pk_add_f32 whose result
  // the next instruction reads (a packed fp32 result is two whole dwords); a scalar splat as first source clears the bit.
  // That was 14 s_nop per section in a chain that has nothing else to put there: a tenth of the kernel's issue slots.
  const float one = sc.one;
  const f2 NA1 = {na1, na1}, NA2 = {na2, na2}, ONE = {one, one};
  f2 S1 = {0.f, 0.f}, S2 = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kL / 2; ++j) {
    const f2 x = v[j];
    const f2 y = j == 0 ? x : __builtin_elementwise_fma(ONE, x, S1);
    S1 = j == 0 ? NA1 * y : __builtin_elementwise_fma(NA1, y, S2);
    S2 = __builtin_elementwise_fma(NA2, y, -x);
    v[j] = y;
  }
  const float sA1 = S1.x, sA2 = S2.x;
  const double e1 = (double)fmaf(n16[0], S1.x, fmaf(n16[1], S2.x, S1.y));
  const double e2 = (double)fmaf(n16[2], S1.x, fmaf(n16[3], S2.x, S2.y));
  const float t1 = (float)c1, t2 = (float)c2;                      // state entering the chunk
  // State leaving the chunk, M c + e, written over the carried registers: n2 first (c1 is still needed for it), then n1.
  // Computed into fresh registers the new states were copied back at the end of every band (8 v_mov_b64).
  const double i1 = fma(m1, c2, e1), i2 = fma(m3, c2, e2);
  fma_over(c2, m2, c1, i2);
  fma_over_mid(c1, m0, i1);
  // u written by non-accumulating FMAs, so that it lands in the high half of its fix-up pair (v_fmac accumulated it in
  // the register of S.x and a v_mov per value carried it over)
  const float u1 = fma_to(n16[0], t1, fmaf(n16[1], t2, sA1));
  const float u2 = fma_to(n16[2], t1, fmaf(n16[3], t2, sA2));
  const f2 T1 = {t1, u1}, T2 = {t2, u2};
#pragma unroll
  for (int j = 0; j < kL / 2; ++j)
    v[j] = __builtin_elementwise_fma((f2){h0[j], h0[j]}, T1, __builtin_elementwise_fma((f2){h1[j], h1[j]}, T2, v[j]));
}

constexpr int kSerRows = 64;                 // rows per workgroup = lanes per wave
constexpr int kSerBins = 4;                  // a band's bins plus its two neighbours (bands of one or two bins)
constexpr int kSerMaxGroups = 4;             // row groups (of 64 rows) per workgroup

constexpr int kSerMaxWaves = 12;
// The flat layout, instance BPW = 0.  Every wave owns ONE (row group, band) slot, numbered flat across workgroups: slot
// s = W blockIdx.x + wave (W waves per workgroup, 16 or 8), row group s / nb, band s % nb, so that a workgroup is W waves
// whatever the band count -- two workgroups per CU at W = 8 (the default), one at W = 16: four waves on every SIMD, which
// no grouped shape reaches at nine bands (its 9-, 10- and 12-wave workgroups fit once per CU).  Its slots touch row groups
// floor(W blockIdx.x / nb) .. floor((W blockIdx.x + W - 1) / nb), at most ceil((W - 1) / nb) + 1 of them; it holds one
// double-buffered tile for each, and a row group that straddles two workgroups is fetched by both.  The tiles' 1 KiB
// pieces are dealt round-robin over all W waves, whichever row group a wave computes.  Waves whose slot lies past the
// last row group fetch and keep the barriers, nothing else.  The chunk body is the grouped instances', one band per wave.
constexpr int kSerFlatMaxWaves = 16;
template <int BPW, bool MAG>
__global__ __launch_bounds__(64 * (BPW ? kSerMaxWaves : kSerFlatMaxWaves))
__attribute__((amdgpu_waves_per_eu(BPW == 1 ? 5 : BPW == 3 ? 3 : 4)))
void fused_serial_kernel(const SerSec* __restrict__ secs, const FbBand* __restrict__ bands,
                         const float2* __restrict__ sym, const float* __restrict__ x, float* __restrict__ feat,
                         int R, int C, int T, int nb, int J, float scale2, FusedBands fbnd, int mode, float eps,
                         const int* __restrict__ bmap, int nb_out, int out16, int NW) {
  constexpr int NS = 4;                                              // order-4 Butterworth band-pass: four sections
  // A workgroup = G row groups of 64 rows x NW waves per row group; the host makes G NW a multiple of four where it can
  // (the waves of a workgroup go to the CU's SIMDs by their index modulo 4: 9-wave workgroups at five waves per SIMD fit
  // once per CU, 8-wave ones twice, 6-wave ones ran a third slower than 3- or 12-wave ones).  Row groups are independent;
  // they only share the workgroup barrier.
  extern __shared__ __attribute__((aligned(16))) float ring_raw[];   // [G][2][64 * 32]: two tiles per row group
  const int lane = threadIdx.x & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr bool FLAT = BPW == 0;
  constexpr int NBW = FLAT ? 1 : BPW;                                // bands a wave carries
  int grp, wave, row0, flat_pieces = 0;
  if constexpr (FLAT) {
    const int W = (int)(blockDim.x >> 6), slot0 = W * (int)blockIdx.x, n_groups = (R + kSerRows - 1) / kSerRows;
    const int g0 = slot0 / nb, g1 = min((slot0 + W - 1) / nb, n_groups - 1);   // the workgroup's row groups (with rows)
    const int g = (slot0 + wave_all) / nb;
    wave = slot0 + wave_all - g * nb;                                // this wave's band, or nb: a slot past the end
    if (g >= n_groups) wave = nb;
    grp = min(g, g1) - g0;                                           // its tile
    row0 = g * kSerRows;
    flat_pieces = 8 * (g1 - g0 + 1);
  } else {
    grp = wave_all / NW, wave = wave_all - grp * NW;                 // row group of this wave, its index in the group
    row0 = (blockIdx.x * (int)(blockDim.x >> 6) / NW + grp) * kSerRows;   // first row of the group
  }
  float* const ring = ring_raw + grp * (2 * kSerRows * kL);
  const int row = row0 + lane;
  const bool row_ok = row < R;
  const int rowc = row_ok ? row : R - 1;                             // a missing row recomputes the last one
  const int bt = rowc / C, ch = rowc - bt * C;
  // band 0, frame 0 of this lane's row as a 32-bit BYTE offset (the host sends maps of 2 GiB and more to the other
  // kernel); opaque, so that it stays in its register instead of being re-derived (a dozen 64-bit multiply steps) in
  // front of every store.  The band / frame part of the address is wave-uniform and rides in the store's scalar base.
  unsigned obyte = (unsigned)(((int64_t)bt * nb_out * C + ch) * (int64_t)J) << (out16 ? 1 : 2);
  asm volatile("" : "+v"(obyte));
  const int64_t bstride = (int64_t)C * J;
  const int n_chunks = T / kL;

  // loader (LDS-DMA, 16 bytes per lane straight into the tile: no registers, nothing to spill): instruction i covers
  // rows 8 i .. 8 i + 7 of the workgroup, eight lanes per row; the instruction's kilobyte of LDS is contiguous, so the
  // swizzle is applied on the GLOBAL side -- the lane that fills slot p of row r fetches quad p ^ ((r >> 1) & 7)
  const unsigned ring_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)ring;
  auto fetch_tile = [&](int c) {                                     // chunk c of the group's 64 rows -> ring[c & 1]
    if (c >= n_chunks) return;
    if constexpr (FLAT) {                                            // piece p: rows 8 (p & 7) .. + 7 of tile p >> 3
      const int W = (int)(blockDim.x >> 6), first = W * (int)blockIdx.x / nb * kSerRows;
      for (int p = wave_all; p < flat_pieces; p += W) {
        const int r = 8 * (p & 7) + (lane >> 3);
        int gr = first + (p >> 3) * kSerRows + r;
        gr = gr < R ? gr : R - 1;
        const float* src = x + (int64_t)gr * T + c * kL + 4 * ((lane & 7) ^ ((r >> 1) & 7));
        const unsigned all_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)ring_raw;
        ser_dma16(src, all_base + (unsigned)(((2 * (p >> 3) + (c & 1)) * kSerRows * kL) * 4 + (p & 7) * 1024));
      }
      return;
    }
    for (int i = wave; i < 8; i += NW) {
      const int r = 8 * i + (lane >> 3);
      int gr = row0 + r;
      gr = gr < R ? gr : R - 1;
      const float* src = x + (int64_t)gr * T + c * kL + 4 * ((lane & 7) ^ ((r >> 1) & 7));
      ser_dma16(src, ring_base + (unsigned)(((c & 1) * kSerRows * kL) * 4 + i * 1024));
    }
  };
  const int rbase = lane * kL, rswz = (lane >> 1) & 7;

  double S[NBW][NS][2];
  f2 prevU[NBW][kSerBins];
  float ob[NBW][4];                                                  // the band's last frames, waiting for their store
#pragma unroll
  for (int i = 0; i < NBW; ++i) {
    ob[i][0] = ob[i][1] = ob[i][2] = ob[i][3] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) S[i][s][0] = S[i][s][1] = 0.0;
#pragma unroll
    for (int kk = 0; kk < kSerBins; ++kk) prevU[i][kk] = (f2){0.f, 0.f};
  }

  // One workgroup barrier per chunk step (0.03 of the kernel's 0.77 ms at the headline shape: the waves of a workgroup sit
  // on different SIMDs with other company each, and every barrier waits for the slowest; one barrier per TWO chunks, with
  // tiles of two chunks, measured the same -- the skew is persistent, not per-step noise).
  int pend = 0;                                  // stores issued behind the last fetch (wave-uniform)
  fetch_tile(0);
  for (int c = 0; c <= n_chunks; ++c) {
    const bool last = c == n_chunks;             // the closing frame: chunk n_chunks - 1 + zeros
    const float* tile = ring + (c & 1) * (kSerRows * kL);
    // This wave's share of tile c has landed (it was issued a whole step ago) ... everyone's has, and every wave is done
    // reading tile c - 1, whose buffer the next fetch overwrites.  The wait must not cover the feature stores the wave
    // issued BEHIND that fetch (an acknowledged store is a microsecond away): vmcnt counts in order, so "all but the
    // youngest `pend`" retires the fetch and leaves the stores in flight.
    if (pend == 1) __builtin_amdgcn_s_waitcnt(0x0F71);
    else if (pend == 2) __builtin_amdgcn_s_waitcnt(0x0F72);
    else if (pend == 3) __builtin_amdgcn_s_waitcnt(0x0F73);
    else __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    fetch_tile(c + 1);
    pend = 0;
#pragma unroll
    for (int i = 0; i < NBW; ++i) {
      const int b = FLAT ? wave : wave + i * NW;
      if (b < nb) {
        const int klo = fbnd.klo[b], khi = fbnd.khi[b];
        const int k0 = klo - 1, nbin = khi - klo + 1;
        f2 Xs[kSerBins];
        if (!last) {
          f2 v[kL / 2];
          {
            const float gain = bands[b].gf;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {                          // quads qd and qd + 4: samples 4 qd .. and 16 + 4 qd ..
              const float4 a = *reinterpret_cast<const float4*>(&tile[rbase + ((qd ^ rswz) << 2)]);
              const float4 h = *reinterpret_cast<const float4*>(&tile[rbase + (((qd + 4) ^ rswz) << 2)]);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                v[4 * qd + e] = (f2){mul_unpacked(f4_get(a, e), gain), mul_unpacked(f4_get(h, e), gain)};
            }
          }
#pragma unroll
          for (int s = 0; s < NS; ++s) section_serial_f32(v, secs[b * NS + s], S[i][s][0], S[i][s][1]);
          f2 ad[15];
#pragma unroll
          for (int m = 1; m < 16; ++m) ad[m - 1] = sym_pair(v[m], v[16 - m]);
#pragma unroll
          for (int kk = 0; kk < kSerBins; ++kk) {
            const int k = k0 + kk;
            // the bin's 16 table entries in ONE batch of scalar loads (32 dwords)
            const f2* __restrict__ tq = later(reinterpret_cast<const f2*>(sym + (int64_t)k * 16));
            f2 tc[17];
#pragma unroll
            for (int m = 1; m <= 16; ++m) tc[m] = tq[m - 1];
            f2 acc_a = pmac0(ad[0], tc[1]), acc_b = pmac0(ad[1], tc[2]);
#pragma unroll
            for (int m = 3; m <= 13; m += 2) {
              pmac(acc_a, ad[m - 1], tc[m]);
              pmac(acc_b, ad[m], tc[m + 1]);
            }
            pmac(acc_a, ad[14], tc[15]);
            cmac_lo_conj(acc_b, v[0], tc[16]);                        // y[0] e^{+i 16 th}
            f2 U = acc_a + acc_b;
            add_lo(U, v[0]);                                          // y[16]
            // frame j = U_{j-1} + (-1)^k U_j; the sign as a wave-uniform bit pattern (a float select was a v_cndmask)
            const float sg = __builtin_bit_cast(float, 0x3f800000u | ((unsigned)k << 31));
            Xs[kk] = __builtin_elementwise_fma(U, (f2){sg, sg}, prevU[i][kk]);
            prevU[i][kk] = U;
          }
        } else {
#pragma unroll
          for (int kk = 0; kk < kSerBins; ++kk) Xs[kk] = prevU[i][kk];
        }
        // Hann in the frequency domain, in the un-rotated coordinates: Z'[k] = 0.5 X'[k] - 0.25 i (X'[k-1] - X'[k+1])
        float acc = 0.f;
#pragma unroll
        for (int bq = 0; bq < kSerBins - 2; ++bq) {
          const f2 w = Xs[bq] - Xs[bq + 2], mid = Xs[bq + 1];
          const float vx = fmaf(0.25f, w.y, 0.5f * mid.x), vy = fmaf(-0.25f, w.x, 0.5f * mid.y);
          float pw = (vx * vx + vy * vy) * scale2;
          if (MAG) pw = sqrtf(pw);
          acc += bq < nbin ? pw : 0.f;
        }
        float r = acc * fbnd.inv[b];
        if (mode == ISD_BP_LOGPOWER) r = fast_log(r + eps);
        // Four frames per store.  A lane's frames of one band are 4 (2) bytes apart, the lanes' rows 4 J bytes: a store
        // per frame is 64 separate dword requests to the L2 (17 per row and band: the first version spent a seventh of
        // its time there); the lane keeps four frames and writes them as one 16-byte (8-byte) piece -- dword (half-word)
        // aligned only, which gfx950's global stores take (tools/ubench/unaligned_x4.hip) -- and the rest one by one.
        const int cq = c & 3;
        if (cq == 0) ob[i][0] = r; else if (cq == 1) ob[i][1] = r; else if (cq == 2) ob[i][2] = r; else ob[i][3] = r;
        if ((cq == 3 || last) && row0 < R) pend += (cq == 3) ? 1 : cq + 1;   // (a group past the end stores nothing)
        if (row_ok && (cq == 3 || last)) {
          const int64_t ou = (int64_t)bmap[b] * bstride + (c - cq);  // wave-uniform: first frame of the group
          if (out16) {
            char* fu = reinterpret_cast<char*>(reinterpret_cast<unsigned short*>(feat) + ou) + obyte;
            if (cq == 3) {
              unsigned p0, p1;                                        // gfx950 conversion (RNE)
              asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p0) : "v"(ob[i][0]), "v"(ob[i][1]));
              asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p1) : "v"(ob[i][2]), "v"(ob[i][3]));
              typedef unsigned u2h __attribute__((ext_vector_type(2), aligned(2)));
              *reinterpret_cast<u2h*>(fu) = (u2h){p0, p1};
            } else {
#pragma unroll
              for (int k = 0; k < 3; ++k)
                if (k <= cq) {
                  unsigned pk;
                  asm("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(pk) : "v"(ob[i][k]));
                  reinterpret_cast<unsigned short*>(fu)[k] = (unsigned short)pk;
                }
            }
          } else {
            char* fu = reinterpret_cast<char*>(feat + ou) + obyte;
            if (cq == 3) {
              typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
              *reinterpret_cast<f4u*>(fu) = (f4u){ob[i][0], ob[i][1], ob[i][2], ob[i][3]};
            } else {
#pragma unroll
              for (int k = 0; k < 3; ++k)
                if (k <= cq) reinterpret_cast<float*>(fu)[k] = ob[i][k];
            }
          }
        }
      }
    }
  }
}

// Dynamic LDS of fused_serial_kernel: two 64 x 32 tiles per row group
static size_t fused_serial_lds(int groups) { return sizeof(float) * (size_t)groups * 2 * kSerRows * kL; }

static void mat2_mul(const double* a, const double* b, double* o) {
  double r[4] = {a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2],
                 a[2] * b[1] + a[3] * b[3]};
  memcpy(o, r, sizeof(r));
}

}  // namespace isd

using namespace isd;

extern "C" int isd_fb_plan_destroy(isd_fb_plan* p);

// The extractor's environment switches: A/B measurements, and the tests that hold two routes against each other
// (DESIGN.md 3.2a has the table).  They are read here and nowhere else.
// Once per process -- ISD_FUSED_ROWS4_OFF: long rows go to the one-row-per-wave kernels; ISD_ROWS4_LDS_CARRY: the fp32
// rows4 kernel keeps its carried section states in LDS
static bool env_rows4_off() { static const bool v = getenv("ISD_FUSED_ROWS4_OFF") != nullptr; return v; }
static bool env_rows4_lds_carry() { static const bool v = getenv("ISD_ROWS4_LDS_CARRY") != nullptr; return v; }
// Per call, so that a test can switch them -- ISD_FUSED_SERIAL=0: short rows stay on fused_kernel; ISD_SERIAL_BPW (1..3)
// and ISD_SERIAL_GROUPS: the serial kernel's bands per wave and row groups per workgroup, 0 when unset
static bool env_fused_serial() { const char* e = getenv("ISD_FUSED_SERIAL"); return !(e && e[0] == '0'); }
static int env_serial_bpw() { const char* e = getenv("ISD_SERIAL_BPW"); return e ? atoi(e) : 0; }
static int env_serial_groups() { const char* e = getenv("ISD_SERIAL_GROUPS"); return e ? atoi(e) : 0; }
// ISD_SERIAL_FLAT: waves per workgroup of the serial family's flat layout, 8 or 16; 0 keeps the grouped layout; unset
// (or anything else) is the default.  8 -- two workgroups per CU, a smaller barrier, two tiles at nine bands -- is the
// one that cleared the bar at the headline shape (profiles/r24_serial_flat_ab.txt); 16 did not.
constexpr int kSerFlatDefault = 8;
static int env_serial_flat() {
  const char* e = getenv("ISD_SERIAL_FLAT");
  const int v = e ? atoi(e) : kSerFlatDefault;
  return v == 0 || v == 8 || v == 16 ? v : kSerFlatDefault;
}
// Per plan -- ISD_FB_AUTO_LIMIT replaces the AUTO threshold on the round-off amplification estimate: a positive number,
// or the call fails (atof("") = 0 would silently send every band to the fp64 kernels)
static int env_fb_auto_limit(double* limit) {
  const char* e = getenv("ISD_FB_AUTO_LIMIT");
  char* end = nullptr;
  const double v = e ? strtod(e, &end) : *limit;
  ISD_CHECK_ARG(!e || (end != e && *end == '\0' && v > 0.0 && v < 1e300),
                "isd_fb_plan_create: ISD_FB_AUTO_LIMIT='%s' is not a positive number", e);
  *limit = v;
  return ISD_OK;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// float4 accesses: rows of a multiple of four samples behind 16-byte aligned bases
static bool vec_ok(int T, const void* a, const void* b = nullptr) { return (T & 3) == 0 && aligned16(a) && aligned16(b); }

// Workgroups that share a quad of rows in the rows4 kernels: the count in [4, 8] (8 preferred) that wastes the fewest
// band slots -- ceil(nb / s) s / nb -- and keeps a workgroup's bands within its carry slots.
static int rows4_share(int nb) {
  int best = kLongShare;
  double best_w = 1e30;
  for (int s = kLongShare; s >= 4; --s) {
    const int per = (nb + s - 1) / s;
    if (per > kRows4Bands) continue;
    const double w = (double)per * s / (double)(nb > 0 ? nb : 1);
    if (w < best_w - 1e-9) { best_w = w; best = s; }
  }
  return best;
}

// The constants of one biquad section (wave-uniform tables of the kernels) and its 16 per-lane matrices M^i
static void build_section(double a1, double a2, FbSec& sc, double* Qout) {
  const double A[4] = {-a1, 1.0, -a2, 0.0};
  double An[4] = {1, 0, 0, 1};
  for (int k = 0; k < kL; ++k) {              // h[n] = row 0 of A^n ; afterwards An = A^32
    if (k < kL / 2) {
      sc.hdq[0][k] = An[0];
      sc.hdq[1][k] = An[1];
      sc.hq[0][k] = (float)An[0];
      sc.hq[1][k] = (float)An[1];
    }
    if (k == kL / 2)
      for (int e = 0; e < 4; ++e) {
        sc.N16d[e] = An[e];
        sc.N16f[e] = (float)An[e];
      }
    mat2_mul(A, An, An);
  }
  double Mk[4];
  memcpy(Mk, An, sizeof(Mk));
  double Qi[4] = {1, 0, 0, 1};
  for (int i = 0; i < 16; ++i) {              // Q_i = M^i
    memcpy(Qout + i * 4, Qi, sizeof(Qi));
    mat2_mul(Mk, Qi, Qi);
  }
  memcpy(sc.P, Qi, sizeof(Qi));               // M^16
  for (int k = 0; k < 4; ++k) {               // M^(1,2,4,8)
    memcpy(sc.Mp[k], Mk, sizeof(Mk));
    mat2_mul(Mk, Mk, Mk);
  }
  sc.a1d = a1; sc.a2d = a2; sc.a1f = (float)a1; sc.a2f = (float)a2;
}

extern "C" int isd_fb_plan_create(isd_fb_plan** out, int n_bands, int n_sections, const double* a12,
                                  const double* gain, int precision) {
  ISD_CHECK_ARG(out && a12 && gain, "isd_fb_plan_create: null argument");
  ISD_CHECK_ARG(n_bands >= 1 && n_bands <= 4096, "isd_fb_plan_create: n_bands=%d out of range", n_bands);
  ISD_CHECK_ARG(n_sections >= 1 && n_sections <= kMaxSec, "isd_fb_plan_create: n_sections=%d not in [1,%d]",
                n_sections, kMaxSec);
  ISD_CHECK_ARG(precision == ISD_FB_F32 || precision == ISD_FB_F64 || precision == ISD_FB_AUTO,
                "isd_fb_plan_create: bad precision %d", precision);
  const int n = n_bands * n_sections;
  std::vector<FbSec> secs(n);
  std::vector<FbBand> bands(n_bands);
  std::vector<double> Q((size_t)n * 64);
  std::vector<double> worst(n_bands, 0.0);
  for (int b = 0; b < n_bands; ++b) {
    bands[b].gd = gain[b];
    bands[b].gf = (float)gain[b];
    bands[b].pad = 0.f;
    for (int s = 0; s < n_sections; ++s) {
      const int bs = b * n_sections + s;
      const double a1 = a12[bs * 2], a2 = a12[bs * 2 + 1];
      // stability (poles strictly inside the unit circle)
      ISD_CHECK_ARG(a2 < 1.0 && a2 > -1.0 && fabs(a1) < 1.0 + a2,
                    "isd_fb_plan_create: band %d section %d is not stable (a1=%g a2=%g)", b, s, a1, a2);
      build_section(a1, a2, secs[bs], &Q[(size_t)bs * 64]);
      // fp32 round-off amplification of a resonator ~ 1 / ((1-r) sin(theta))
      if (a2 > 0.0) {
        const double r = sqrt(a2);
        double c = -a1 / (2.0 * r);
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
        const double st = sqrt(1.0 - c * c);
        const double g = 1.0 / ((1.0 - r) * (st > 1e-9 ? st : 1e-9));
        if (g > worst[b]) worst[b] = g;
      }
    }
  }
  // per-band arithmetic: AUTO sends a band to the fp64 set when one of its poles is too close to z = 1.  The threshold
  // on the round-off amplification estimate was 2000 until round 3; measured at the stress set (tools/
  // auto_limit_probe.py, |feature - scipy fp64| / max(1, |feature|), gate 1e-4): the bands between 2000 and 6000
  // (2-Hz bands from 14 to 36 Hz at 1024 Hz) stay within 5e-6 in fp32, the five above 6000 (4 - 14 Hz) reach 1.3e-5
  // -- inside that relative gate, but with them in fp32 the 1024-point golden features (g3 "c5") are off by up to
  // 1.09e-4 in ABSOLUTE log power (a log power near -12: 9e-6 relative), over the 1e-4 the golden-vector tests hold
  // (tests/test_features_gpu.py), so they stay on the fp64 kernels -- and the 0.5 - 4 Hz band of the 5-band set
  // (20 900) misses both.  A host replay of the fp32 chunk arithmetic as the criterion was tried and dropped: it
  // ranks the five like the estimate does (rms error 2.9e-5 / 1.3e-5 / 1.9e-5 / 1.4e-5 / 7e-6 of the signal) and
  // separates the 5-band set's 0.5 - 4 Hz band (1.4e-4) no better.  ISD_FB_AUTO_LIMIT overrides.
  double auto_limit = 6000.0;
  if (const int rc = env_fb_auto_limit(&auto_limit)) return rc;
  isd_fb_plan* p = new isd_fb_plan();
  p->n_bands = n_bands; p->n_sections = n_sections;
  for (int k = 0; k < 2; ++k) {
    p->set[k] = FbSet{0, nullptr, nullptr, nullptr, nullptr, nullptr};
    p->host_map[k] = nullptr;
  }
  std::vector<int> idx[2];
  for (int b = 0; b < n_bands; ++b) {
    const int k = precision == ISD_FB_AUTO ? (worst[b] > auto_limit ? 1 : 0) : (precision == ISD_FB_F64 ? 1 : 0);
    idx[k].push_back(b);
  }
  p->precision = idx[1].empty() ? ISD_FB_F32 : (idx[0].empty() ? ISD_FB_F64 : ISD_FB_MIXED);
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    const int nb = (int)idx[k].size();
    if (!nb) continue;
    std::vector<FbSec> ss((size_t)nb * n_sections);
    std::vector<FbBand> bb(nb);
    std::vector<double> qq((size_t)nb * n_sections * 64);
    for (int i = 0; i < nb; ++i) {
      const int b = idx[k][i];
      bb[i] = bands[b];
      for (int sct = 0; sct < n_sections; ++sct) {
        ss[(size_t)i * n_sections + sct] = secs[(size_t)b * n_sections + sct];
        memcpy(&qq[((size_t)i * n_sections + sct) * 64], &Q[((size_t)b * n_sections + sct) * 64], sizeof(double) * 64);
      }
    }
    FbSet& fs = p->set[k];
    fs.nb = nb;
    p->host_map[k] = new int[nb];
    memcpy(p->host_map[k], idx[k].data(), sizeof(int) * nb);
    e = hipMalloc(&fs.d_sec, sizeof(FbSec) * ss.size());
    if (e == hipSuccess) e = hipMalloc(&fs.d_band, sizeof(FbBand) * nb);
    if (e == hipSuccess) e = hipMalloc(&fs.d_Q, sizeof(double) * qq.size());
    if (e == hipSuccess) e = hipMalloc(&fs.d_map, sizeof(int) * nb);
    if (e == hipSuccess) e = hipMemcpy(fs.d_sec, ss.data(), sizeof(FbSec) * ss.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fs.d_band, bb.data(), sizeof(FbBand) * nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fs.d_Q, qq.data(), sizeof(double) * qq.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fs.d_map, idx[k].data(), sizeof(int) * nb, hipMemcpyHostToDevice);
    if (e == hipSuccess && k == 0) {
      std::vector<SerSec> sv(ss.size());
      for (size_t i = 0; i < ss.size(); ++i) {
        SerSec& d = sv[i];
        const FbSec& c = ss[i];
        memcpy(d.M, c.Mp[0], sizeof(d.M));
        d.a1 = c.a1f; d.a2 = c.a2f; d.one = 1.f; d.pad = 0.f;
        memcpy(d.N16, c.N16f, sizeof(d.N16));
        memcpy(d.hq, c.hq, sizeof(d.hq));
      }
      e = hipMalloc(&fs.d_ser, sizeof(SerSec) * sv.size());
      if (e == hipSuccess) e = hipMemcpy(fs.d_ser, sv.data(), sizeof(SerSec) * sv.size(), hipMemcpyHostToDevice);
    }
  }
  if (e != hipSuccess) {
    set_error("isd_fb_plan_create: %s", hipGetErrorString(e));
    isd_fb_plan_destroy(p);
    return e == hipErrorNoDevice ? ISD_ERR_NO_DEVICE : ISD_ERR_HIP;
  }
  *out = p;
  return ISD_OK;
}

extern "C" int isd_fb_plan_destroy(isd_fb_plan* p) {
  if (!p) return ISD_OK;
  for (int k = 0; k < 2; ++k) {
    FbSet& fs = p->set[k];
    if (fs.d_sec) (void)hipFree(fs.d_sec);
    if (fs.d_band) (void)hipFree(fs.d_band);
    if (fs.d_Q) (void)hipFree(fs.d_Q);
    if (fs.d_map) (void)hipFree(fs.d_map);
    if (fs.d_ser) (void)hipFree(fs.d_ser);
    delete[] p->host_map[k];
  }
  delete p;
  return ISD_OK;
}

extern "C" int isd_fb_plan_precision(const isd_fb_plan* p) { return p ? p->precision : ISD_ERR_INVALID; }

// One launch of the filterbank or of the fused extractor: the kernel family, the template selectors of the instance and
// what the launch derives from the shape.  choose_fb_route / choose_fused_route fill it and hold every shape, alignment,
// band-count and environment test (DESIGN.md 3.2a has the table); the launch functions only read it.
enum Family {
  kFbShort, kFbLong, kFbRows4,               // isd_fb_forward: fb_kernel, fb_long_kernel_*, fb_rows4_kernel_*
  kDirect16, kSerial, kLong, kRows4          // the fused call: fused_kernel, fused_serial_, fused_long_, fused_rows4_kernel
};
struct Route {
  Family family;
  dim3 grid, block;
  size_t lds;                  // dynamic LDS bytes
  // Template selectors.  f64: VT double (the plan's fp64 set) or float | gpr: GPR, 16-lane groups per row | full: FULL,
  // whole waves of whole segments | mag: MAG | vec: VEC and the kernels' `vec` argument, float4 row accesses | kb: KB,
  // bin slots (blocksum_plan) | carry_n: NS of fused_rows4_kernel, 4 = carried states in registers, 0 = in LDS | bpw:
  // BPW, bands per wave of the serial kernel | fullq: FULLQ, every quad of rows is whole | flat: the serial family's flat
  // layout with that many waves per workgroup (fused_serial_kernel<0, MAG>), 0 = the grouped layout
  bool f64, full, mag, fullq;
  int gpr, vec, kb, carry_n, bpw, flat;
  int share_n, nw, groups, log2_nblk;   // scalar launch arguments derived from the shape
};

static Route choose_fb_route(const isd_fb_plan* p, int k, const float* x, const float* y, int64_t R, int T) {
  const FbSet& fs = p->set[k];
  Route r = {};
  r.f64 = k == 1;
  r.block = dim3(64);
  r.vec = vec_ok(T, x, y);
  if (T <= 2 * kSeg) {
    r.family = kFbShort;
    r.gpr = T <= kSeg ? 1 : 2;
    r.full = r.vec && T == r.gpr * kSeg && R % (4 / r.gpr) == 0;
    r.grid = dim3((unsigned)cdiv(R, 4 / r.gpr));
  } else if (r.vec && T % kSeg == 0 && fs.nb <= kMaxBands && !env_rows4_off()) {
    r.family = kFbRows4;                     // four rows per wave, group-local carries (carry slots for kMaxBands bands)
    r.share_n = rows4_share(fs.nb);
    r.fullq = R % 4 == 0;
    r.grid = dim3((unsigned)(cdiv(cdiv(R, 4), 8) * 8 * r.share_n));
  } else {
    r.family = kFbLong;
    r.grid = dim3((unsigned)(cdiv(R, 8) * 8 * kLongShare));
  }
  return r;
}

static int fb_launch(const isd_fb_plan* p, int k, const Route& r, const float* x, float* y, int64_t R, int C, int T,
                     hipStream_t st) {
  const FbSet& fs = p->set[k];
  switch (r.family) {
    case kFbShort: {
      static constexpr decltype(&fb_kernel<float, 1, false>) kern[2][2][2] = {   // [f64][gpr - 1][full]
          {{fb_kernel<float, 1, false>, fb_kernel<float, 1, true>}, {fb_kernel<float, 2, false>, fb_kernel<float, 2, true>}},
          {{fb_kernel<double, 1, false>, fb_kernel<double, 1, true>},
           {fb_kernel<double, 2, false>, fb_kernel<double, 2, true>}}};
      return launch_lds(kern[r.f64][r.gpr - 1][r.full], r.grid, r.block, 0, st, fs.d_sec, fs.d_band, fs.d_Q, x, y, (int)R,
                        C, T, fs.nb, p->n_sections, r.vec, fs.d_map, p->n_bands);
    }
    case kFbRows4: {
      static constexpr decltype(&fb_rows4_kernel_f32<false>) kern[2][2] = {      // [f64][fullq]
          {fb_rows4_kernel_f32<false>, fb_rows4_kernel_f32<true>}, {fb_rows4_kernel_f64<false>, fb_rows4_kernel_f64<true>}};
      return launch_lds(kern[r.f64][r.fullq], r.grid, r.block, 0, st, fs.d_sec, fs.d_band, fs.d_Q, x, y, C, T, fs.nb,
                        p->n_sections, fs.d_map, p->n_bands, (int)R, r.share_n);
    }
    default: {
      static constexpr decltype(&fb_long_kernel_f32<false>) kern[2][2] = {       // [f64][vec]
          {fb_long_kernel_f32<false>, fb_long_kernel_f32<true>}, {fb_long_kernel_f64<false>, fb_long_kernel_f64<true>}};
      return launch_lds(kern[r.f64][r.vec], r.grid, r.block, 0, st, fs.d_sec, fs.d_band, fs.d_Q, x, y, C, T, fs.nb,
                        p->n_sections, fs.d_map, p->n_bands, (int)R);
    }
  }
}

extern "C" int isd_fb_forward(const isd_fb_plan* p, const float* x, float* y, int64_t B, int64_t C, int64_t T,
                              void* stream) {
  ISD_CHECK_ARG(p, "isd_fb_forward: null plan");
  ISD_CHECK_ARG(B >= 0 && C >= 1 && T >= 1 && T <= (1 << 24) && C <= (1 << 20), "isd_fb_forward: bad shape B=%lld C=%lld T=%lld",
                (long long)B, (long long)C, (long long)T);
  if (B == 0) return ISD_OK;
  ISD_CHECK_ARG(x && y, "isd_fb_forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = B * C;
  ISD_CHECK_ARG(R <= kMaxRows, "isd_fb_forward: too many rows (%lld)", (long long)R);
  for (int k = 0; k < 2; ++k) {
    if (!p->set[k].nb) continue;
    const int rc = fb_launch(p, k, choose_fb_route(p, k, x, y, R, (int)T), x, y, R, (int)C, (int)T, st);
    if (rc) return rc;
  }
  return ISD_OK;
}

// host side of FusedBands: bin ranges plus 1 / (number of bins)
static void set_band(FusedBands& f, int i, int klo, int khi) {
  f.klo[i] = klo;
  f.khi[i] = khi;
  f.inv[i] = khi >= klo ? 1.f / (float)(khi - klo + 1) : 0.f;
}

// The bands of precision set k, in the set's order, out of the plan's
static FusedBands set_bands(const isd_fb_plan* fb, int k, const FusedBands& all) {
  FusedBands f = {};
  for (int i = 0; i < fb->set[k].nb; ++i) set_band(f, i, all.klo[fb->host_map[k][i]], all.khi[fb->host_map[k][i]]);
  return f;
}

// What isd_features_fused_last_path() reports: the family of the fp32 set's launch (1 fused_kernel, 2
// fused_serial_kernel, 3 long rows); assigned once per call, in features_fused_impl
static thread_local int g_fused_path = 0;
extern "C" int isd_features_fused_last_path(void) { return g_fused_path; }
// What isd_features_fused_last_serial_waves() reports: the waves per workgroup of the flat layout if the fp32 set's
// launch took the flat layout, else 0; assigned beside g_fused_path
static thread_local int g_serial_waves = 0;
extern "C" int isd_features_fused_last_serial_waves(void) { return g_serial_waves; }

static constexpr decltype(&fused_serial_kernel<1, false>) kSerialKernels[4][2] = {   // [bpw, 0 = flat][mag]
    {fused_serial_kernel<0, false>, fused_serial_kernel<0, true>},
    {fused_serial_kernel<1, false>, fused_serial_kernel<1, true>},
    {fused_serial_kernel<2, false>, fused_serial_kernel<2, true>},
    {fused_serial_kernel<3, false>, fused_serial_kernel<3, true>}};
// Tiles above 48 KiB (four row groups: 64 KiB) need the kernels' dynamic-LDS limit raised: once per process and device,
// to the largest tile the launcher builds, instead of twice in front of every launch.
static void serial_lds_limit() {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const unsigned long long bit = 1ull << dev;
  if (done.load(std::memory_order_relaxed) & bit) return;
  for (const auto& per_bpw : kSerialKernels)
    for (const auto f : per_bpw)
      (void)hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)fused_serial_lds(kSerMaxGroups));
  done.fetch_or(bit, std::memory_order_relaxed);
}

// The two row shapes the fused call serves
static bool fused_short_rows(const isd_stft_plan* st) {
  return st->n == 64 && st->hop == 32 && st->T <= 2 * kSeg && st->d_dft;
}
static bool fused_long_rows(const isd_stft_plan* st) { return st->d_blk && st->hop == 64 && st->T <= 64 * 64; }

// The route of precision set k of a fused call over R rows; `all` holds the plan's bands in the caller's order
static int choose_fused_route(const isd_fb_plan* fb, int k, const isd_stft_plan* st, const float* x, int64_t R, int C,
                              const FusedBands& all, int mode, Route& r) {
  const FbSet& fs = fb->set[k];
  r = Route{};
  r.f64 = k == 1;
  r.mag = mode == ISD_BP_MAGNITUDE;
  r.block = dim3(64);
  r.vec = vec_ok(st->T, x);
  if (!fused_short_rows(st)) {
    // long rows, heavily overlapped frames: filterbank + block sums in one kernel per band set
    r.family = kLong;
    const int bad = blocksum_plan(st, all.klo, all.khi, fb->n_bands, &r.kb, &r.log2_nblk);
    if (bad >= 0) {
      set_error("isd_features_fused: band %d needs 1..6 interior bins for the block-sum path (bins %d..%d)", bad,
                all.klo[bad], all.khi[bad]);
      return ISD_ERR_UNSUPPORTED;
    }
    // rows of whole 512-sample passes covering all 64 blocks: four rows per wave, no cross-group chain.  Its instances
    // stop at KB = 5; wider bands stay on the one-row-per-wave kernel.
    if (r.vec && st->T % kSeg == 0 && r.log2_nblk <= 4 && r.log2_nblk >= 1 && !env_rows4_off() && r.kb <= 5) {
      r.family = kRows4;
      // fp32 with the usual four sections (order-4 Butterworth band-pass): the carried states in registers
      r.carry_n = !r.f64 && fb->n_sections == 4 && !env_rows4_lds_carry() ? 4 : 0;
      r.share_n = rows4_share(fs.nb);
      r.grid = dim3((unsigned)(cdiv(cdiv(R, 4), 8) * 8 * r.share_n));
      r.lds = fused_rows4_lds(r.kb, fb->n_sections);
    } else {
      r.grid = dim3((unsigned)(cdiv(R, 8) * 8 * kLongShare));
      r.lds = fused_long_lds(r.kb);
    }
    return ISD_OK;
  }
  // One row per lane (fused_serial_kernel): the fp32 set of at most 12 bands, each of one or two interior bins, four
  // sections, 16-byte aligned rows of whole 32-sample chunks, and 32-bit byte offsets into the feature map
  bool serial = !r.f64 && env_fused_serial() && st->d_sym && fs.d_ser && st->n == 64 && st->hop == 32 &&
                st->T % kL == 0 && st->T >= kL && st->J == st->T / kL + 1 && fb->n_sections == 4 && aligned16(x) &&
                fs.nb >= 1 && fs.nb <= 12 && cdiv(R, C) * (int64_t)fb->n_bands * C * st->J * 4 < (1LL << 31);
  for (int i = 0; serial && i < fs.nb; ++i) {
    const int klo = all.klo[fb->host_map[k][i]], khi = all.khi[fb->host_map[k][i]], nbin = khi - klo + 1;
    serial = nbin >= 1 && nbin <= kSerBins - 2 && klo >= 1 && khi <= st->n / 2 - 1;
  }
  if (serial) {
    r.family = kSerial;
    // bands per wave: 1 (five waves per SIMD), 2 (four) or 3 (three); ISD_SERIAL_BPW overrides the choice
    const int want = env_serial_bpw(), g = env_serial_groups();
    int bpw = want >= 1 && want <= 3 ? want : 3;
    while (bpw < 3 && (fs.nb + bpw - 1) / bpw > kSerMaxWaves) ++bpw;
    r.nw = (fs.nb + bpw - 1) / bpw;                                       // waves per row group
    r.bpw = (fs.nb + r.nw - 1) / r.nw;
    r.groups = r.nw % 4 == 0 ? 1 : r.nw % 2 == 0 ? 2 : 4;                 // waves per workgroup: a multiple of four
    while (r.groups > 1 && r.groups * r.nw > kSerMaxWaves) r.groups >>= 1;
    if (g >= 1 && g <= kSerMaxGroups && g * r.nw <= kSerMaxWaves) r.groups = g;
    r.grid = dim3((unsigned)cdiv(R, (int64_t)kSerRows * r.groups));
    r.block = dim3(64 * r.nw * r.groups);
    r.lds = fused_serial_lds(r.groups);
    // The flat layout (one band per wave, W waves per workgroup whatever the band count) unless a grouped geometry was
    // asked for: a workgroup's slots touch at most ceil((W - 1) / nb) + 1 row groups, one double-buffered tile each
    const int W = env_serial_flat();
    const int64_t n_groups = cdiv(R, kSerRows);
    const int64_t tiles = cdiv(W - 1, fs.nb) + 1;
    if (W && !want && !g && tiles <= kSerMaxGroups) {
      r.flat = W;
      r.bpw = 1;
      r.groups = (int)std::min(tiles, n_groups);
      r.grid = dim3((unsigned)cdiv(n_groups * fs.nb, W));
      r.block = dim3(64 * W);
      r.lds = fused_serial_lds(r.groups);
    }
  } else {
    r.family = kDirect16;
    r.gpr = st->T > kSeg ? 2 : 1;                                         // rows of 513..1024 samples: two 16-lane groups
    r.full = r.vec && st->T == r.gpr * kSeg && R % (4 / r.gpr) == 0;
    r.grid = dim3((unsigned)cdiv(R, 4 / r.gpr));
  }
  return ISD_OK;
}

static int fused_launch(const isd_fb_plan* fb, int k, const isd_stft_plan* st, const Route& r, const float* x,
                        float* feat, int64_t R, int C, const FusedBands& fbnd, int mode, float eps, hipStream_t s,
                        int out16) {
  const FbSet& fs = fb->set[k];
  const float scale2 = st->scale * st->scale;
  const int kbi = r.kb == 8 ? 3 : r.kb - 4;                               // KB 4, 5, 6, 8
  switch (r.family) {
    case kSerial: {
      if (r.lds > 48 * 1024) serial_lds_limit();      // not launch_lds: it would raise the limit before every launch
      hipLaunchKernelGGL(kSerialKernels[r.flat ? 0 : r.bpw][r.mag], r.grid, r.block, r.lds, s, fs.d_ser, fs.d_band, st->d_sym,
                         x, feat, (int)R, C, st->T, fs.nb, st->J, scale2, fbnd, mode, eps, fs.d_map, fb->n_bands, out16, r.nw);
      ISD_LAUNCH_CHECK();
      return ISD_OK;
    }
    case kRows4: {                           // KB 4 or 5; fp64 has no register-carry instance
      using K = decltype(&fused_rows4_kernel<float, 4, 0>);
      static constexpr K f32[2][2] = {{fused_rows4_kernel<float, 4, 0>, fused_rows4_kernel<float, 4, 4>},
                                      {fused_rows4_kernel<float, 5, 0>, fused_rows4_kernel<float, 5, 4>}};
      static constexpr K f64[2] = {fused_rows4_kernel<double, 4, 0>, fused_rows4_kernel<double, 5, 0>};
      return launch_lds(r.f64 ? f64[r.kb - 4] : f32[r.kb - 4][r.carry_n == 4], r.grid, r.block, r.lds, s, fs.d_sec,
                        fs.d_band, fs.d_Q, st->d_blk, x, feat, C, st->T, fs.nb, fb->n_sections, st->J, r.log2_nblk,
                        st->n / 2, scale2, fbnd, mode, eps, fs.d_map, fb->n_bands, (int)R, r.share_n, out16);
    }
    case kLong: {
      static constexpr decltype(&fused_long_kernel<float, 4, false>) kern[2][4][2] = {   // [f64][KB: 4, 5, 6, 8][vec]
          {{fused_long_kernel<float, 4, false>, fused_long_kernel<float, 4, true>},
           {fused_long_kernel<float, 5, false>, fused_long_kernel<float, 5, true>},
           {fused_long_kernel<float, 6, false>, fused_long_kernel<float, 6, true>},
           {fused_long_kernel<float, 8, false>, fused_long_kernel<float, 8, true>}},
          {{fused_long_kernel<double, 4, false>, fused_long_kernel<double, 4, true>},
           {fused_long_kernel<double, 5, false>, fused_long_kernel<double, 5, true>},
           {fused_long_kernel<double, 6, false>, fused_long_kernel<double, 6, true>},
           {fused_long_kernel<double, 8, false>, fused_long_kernel<double, 8, true>}}};
      return launch_lds(kern[r.f64][kbi][r.vec], r.grid, r.block, r.lds, s, fs.d_sec, fs.d_band, fs.d_Q, st->d_blk, x,
                        feat, C, st->T, fs.nb, fb->n_sections, st->J, r.log2_nblk, st->n / 2, scale2, fbnd, mode, eps,
                        fs.d_map, fb->n_bands, (int)R, out16);
    }
    default: {
      static constexpr decltype(&fused_kernel<float, false, 1, false>) kern[2][2][2][2] = {   // [f64][mag][gpr - 1][full]
          {{{fused_kernel<float, false, 1, false>, fused_kernel<float, false, 1, true>},
            {fused_kernel<float, false, 2, false>, fused_kernel<float, false, 2, true>}},
           {{fused_kernel<float, true, 1, false>, fused_kernel<float, true, 1, true>},
            {fused_kernel<float, true, 2, false>, fused_kernel<float, true, 2, true>}}},
          {{{fused_kernel<double, false, 1, false>, fused_kernel<double, false, 1, true>},
            {fused_kernel<double, false, 2, false>, fused_kernel<double, false, 2, true>}},
           {{fused_kernel<double, true, 1, false>, fused_kernel<double, true, 1, true>},
            {fused_kernel<double, true, 2, false>, fused_kernel<double, true, 2, true>}}}};
      return launch_lds(kern[r.f64][r.mag][r.gpr - 1][r.full], r.grid, r.block, 0, s, fs.d_sec, fs.d_band, fs.d_Q,
                        st->d_dft, x, feat, (int)R, C, st->T, fs.nb, fb->n_sections, st->J, scale2, fbnd, mode, eps, r.vec,
                        fs.d_map, fb->n_bands, out16);
    }
  }
}

static int features_fused_impl(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x, float* feat,
                               int64_t B, int64_t C, const int* klo, const int* khi, int mode, float eps,
                               void* stream, int out16) {
  ISD_CHECK_ARG(fb && st, "isd_features_fused: null plan");
  ISD_CHECK_ARG(B == 0 || (x && feat), "isd_features_fused: null argument");
  ISD_CHECK_ARG(B >= 0 && C >= 1 && C <= (1 << 20), "isd_features_fused: bad shape B=%lld C=%lld", (long long)B,
                (long long)C);
  ISD_CHECK_ARG(mode >= ISD_BP_MAGNITUDE && mode <= ISD_BP_LOGPOWER, "isd_features_fused: bad mode %d", mode);
  if (!fused_short_rows(st) && !fused_long_rows(st)) {
    set_error("isd_features_fused: needs nperseg=64/noverlap=32/T<=1024, or hop 64 with nperseg = 2^a*64 and T<=4096 "
              "(got nperseg=%d hop=%d T=%d)", st->n, st->hop, st->T);
    return ISD_ERR_UNSUPPORTED;
  }
  FusedBands all = {};
  int rc = fill_band_args(st, fb->n_bands, klo, khi, all.klo, all.khi, "isd_features_fused");
  if (rc) return rc;
  if (B == 0) return ISD_OK;
  const int64_t R = B * C;
  ISD_CHECK_ARG(R <= kMaxRows, "isd_features_fused: too many rows (%lld)", (long long)R);
  Route route[2] = {};
  for (int k = 0; k < 2 && rc == ISD_OK; ++k)
    if (fb->set[k].nb) rc = choose_fused_route(fb, k, st, x, R, (int)C, all, mode, route[k]);
  g_fused_path = !fused_short_rows(st) ? 3 : route[0].family == kSerial ? 2 : 1;
  g_serial_waves = g_fused_path == 2 ? route[0].flat : 0;
  for (int k = 0; k < 2 && rc == ISD_OK; ++k)
    if (fb->set[k].nb)
      rc = fused_launch(fb, k, st, route[k], x, feat, R, (int)C, set_bands(fb, k, all), mode, eps, (hipStream_t)stream,
                        out16);
  return rc;
}

extern "C" int isd_features_fused(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x, float* feat,
                                  int64_t B, int64_t C, const int* klo, const int* khi, int mode, float eps,
                                  void* stream) {
  return features_fused_impl(fb, st, x, feat, B, C, klo, khi, mode, eps, stream, 0);
}

// The same extraction with the feature map written as bf16 [B][n_bands][C][J] (round to nearest even)
extern "C" int isd_features_fused_bf16(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x, uint16_t* feat,
                                       int64_t B, int64_t C, const int* klo, const int* khi, int mode, float eps,
                                       void* stream) {
  return features_fused_impl(fb, st, x, reinterpret_cast<float*>(feat), B, C, klo, khi, mode, eps, stream, 1);
}

// whole waves of whole segments: the FULL instances' branch-free loads
bool isd::bandpower_direct_full(const isd_stft_plan* st, const float* y, int64_t R) {
  return vec_ok(st->T, y) && st->T == kSeg && R % 4 == 0;
}

int isd::bandpower_direct(const isd_stft_plan* st, const float* y, float* feat, int64_t R, int C, int nb,
                          const int* klo, const int* khi, int mode, float eps, hipStream_t stream) {
  FusedBands fbnd = {};
  for (int b = 0; b < nb; ++b) set_band(fbnd, b, klo[b], khi[b]);
  const int64_t items = cdiv(R, 4);
  ISD_CHECK_ARG(R <= kMaxRows, "isd_stft_bandpower: too many rows (%lld)", (long long)R);
  const int vec = vec_ok(st->T, y);
  const bool full = bandpower_direct_full(st, y, R);
  static constexpr decltype(&bandpower_direct_kernel<false, false>) kern[2][2] = {   // [magnitude][full]
      {bandpower_direct_kernel<false, false>, bandpower_direct_kernel<false, true>},
      {bandpower_direct_kernel<true, false>, bandpower_direct_kernel<true, true>}};
  return launch_lds(kern[mode == ISD_BP_MAGNITUDE][full], dim3((unsigned)items), dim3(64), 0, stream, st->d_dft, y, feat,
                    (int)R, C, st->T, nb, st->J, st->scale * st->scale, fbnd, mode, eps, vec);
}

// ------------------------------------------------------------------------------------------------------------------
// Input gradient of the extractor (isd_features_backward).  Per (trial, channel) row and band b, with
// s = 1 / sum(w) and frame starts s_j = j hop - N/2 (y_b is zero outside [0, T)):
//   forward   y_b = H_b x ;  Z_jk = s sum_n w[n] y_b[s_j + n] e^{-2 pi i k n / N}  (k = klo..khi, nk bins) ;
//             P_j = (1/nk) sum_k |Z_jk|^2 ;  feature log(P_j + eps) | P_j | (1/nk) sum_k |Z_jk|
//   backward  dy_b[t] = sum_j sum_k w[t - s_j] Re(C_jk e^{+2 pi i k (t - s_j) / N}),  C_jk = c_jk Z_jk,
//             c_jk = 2 s g_j / (nk (P_j + eps)) | 2 s g_j / nk | s g_j / (nk |Z_jk|) (0 where |Z_jk| = 0) ;
//             dx = sum_b H_b^T dy_b,  H_b^T = R H_b R: the same causal cascade over the time-reversed gradient.
// The cascade is the forward's own section arithmetic: fp32 bands run section_serial_f32 (zero-state fp32 chunk
// recursion, fp64 carried states), fp64 bands a serial fp64 recursion.
// One row per lane, every lane of a wave in the same band / frame / sample loop: the tables (window, twiddles, section
// constants) are wave-uniform and only the row data differ.  The row data live in the caller's workspace laid out
// [sample][row] (row fastest), so that every access of a wave is coalesced:
//   xT [T][RS] the trials | yT [T][RS] y_b, then dy_b | dT [T][RS] the running band sum of dx | co [J][nkmax][RS] float2
//   Z_jk, then C_jk
// for RS rows at a time (larger batches run in chunks).  Each lane owns its row and adds the bands into it in a fixed
// order (the fp32 set, then the fp64 set, each in plan order): no atomics, the same bits on every call and for a trial
// at any batch size.
namespace isd {

constexpr int kGradKB = 8;                              // bins per register block of the frame DFT / synthesis
constexpr int64_t kGradWorkspaceCap = 2LL << 30;        // bytes of workspace; more rows run in chunks

struct GradBands {                                      // the bands of one precision set, in set order
  int out[kMaxBands];                                   // position in the caller's band order (feature map)
  int klo[kMaxBands];
  int khi[kMaxBands];
};

// e^{-2 pi i m / N} from the plan's half table tw[u] = e^{-2 pi i u / N}, u < N/2
__device__ __forceinline__ float2 grad_twiddle(const float2* __restrict__ tw, int m, int N) {
  const int u = m & (N - 1);
  const float2 e = tw[u & (N / 2 - 1)];
  return (u & (N / 2)) ? make_float2(-e.x, -e.y) : e;
}

// Serial fp64 DF2T section over a chunk (the fp64 bands, both directions); (s1, s2) the carried state
__device__ __forceinline__ void section_grad_f64(double (&v)[kL], const FbSec& sc, double& s1, double& s2) {
  const double na1 = -sc.a1d, na2 = -sc.a2d;
#pragma unroll
  for (int j = 0; j < kL; ++j) {
    const double xj = v[j], y = xj + s1;
    s1 = fma(na1, y, s2);
    s2 = fma(na2, y, -xj);
    v[j] = y;
  }
}

// gain + the band's cascade over one 32-sample chunk of the lane's row, in place; st: the lane's carried section
// states in LDS, [section][2][64 lanes]
template <typename VT>
__device__ __forceinline__ void grad_cascade(float (&io)[kL], const FbSec* __restrict__ sec,
                                             const SerSec* __restrict__ ser, const FbBand& band, int ns, double* st,
                                             int lane) {
  if constexpr (std::is_same<VT, float>::value) {
    f2 v[kL / 2];                                       // sample pairs {j, j + 16}, as fused_serial_kernel holds them
    const float g = band.gf;
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) v[j] = (f2){io[j] * g, io[j + 16] * g};
    for (int s = 0; s < ns; ++s) {
      double c1 = st[(2 * s) * 64 + lane], c2 = st[(2 * s + 1) * 64 + lane];
      section_serial_f32(v, ser[s], c1, c2);
      st[(2 * s) * 64 + lane] = c1;
      st[(2 * s + 1) * 64 + lane] = c2;
    }
#pragma unroll
    for (int j = 0; j < kL / 2; ++j) {
      io[j] = v[j].x;
      io[j + 16] = v[j].y;
    }
  } else {
    double v[kL];
    const double g = band.gd;
#pragma unroll
    for (int j = 0; j < kL; ++j) v[j] = (double)io[j] * g;
    for (int s = 0; s < ns; ++s) {
      double c1 = st[(2 * s) * 64 + lane], c2 = st[(2 * s + 1) * 64 + lane];
      section_grad_f64(v, sec[s], c1, c2);
      st[(2 * s) * 64 + lane] = c1;
      st[(2 * s + 1) * 64 + lane] = c2;
    }
#pragma unroll
    for (int j = 0; j < kL; ++j) io[j] = (float)v[j];
  }
}

// One precision set of bands over n_rows rows starting at row0.  first: copy the trials in and clear the dx sum;
// last: write dx out.
template <typename VT>
__global__ __launch_bounds__(64) void features_grad_kernel(
    const FbSec* __restrict__ secs, const SerSec* __restrict__ sers, const FbBand* __restrict__ bands, GradBands gb,
    int nb, int ns, const float* __restrict__ win, const float2* __restrict__ tw, const float* __restrict__ x,
    const float* __restrict__ dfeat, float* __restrict__ dx, float* __restrict__ ws, int64_t row0, int n_rows,
    int64_t RS, int C, int T, int N, int hop, int J, int nb_out, int nkmax, float scale, int mode, float eps,
    int first, int last) {
  __shared__ double st[kMaxSec * 2 * 64];
  const int lane = threadIdx.x;
  const int r = blockIdx.x * 64 + lane;
  if (r >= n_rows) return;                              // lanes never exchange data
  const int64_t row = row0 + r, bt = row / C, ch = row - bt * C;
  float* const xT = ws + r;
  float* const yT = ws + (int64_t)T * RS + r;
  float* const dT = ws + 2 * (int64_t)T * RS + r;
  float2* const co = reinterpret_cast<float2*>(ws + 3 * (int64_t)T * RS) + r;
  const int half = N / 2;
  if (first) {
    const float* xr = x + row * (int64_t)T;
    for (int t = 0; t < T; ++t) {
      xT[t * RS] = xr[t];
      dT[t * RS] = 0.f;
    }
  }
  for (int i = 0; i < nb; ++i) {
    const int klo = gb.klo[i], khi = gb.khi[i];
    if (khi < klo) continue;                            // an empty band contributes nothing
    const int nk = khi - klo + 1;
    const FbSec* bsec = secs + i * ns;
    const SerSec* bser = std::is_same<VT, float>::value ? sers + i * ns : nullptr;
    const FbBand band = bands[i];
    // 1. causal pass: y_b
    for (int e = 0; e < 2 * ns; ++e) st[e * 64 + lane] = 0.0;
    for (int t0 = 0; t0 < T; t0 += kL) {
      float io[kL];
#pragma unroll
      for (int j = 0; j < kL; ++j) io[j] = t0 + j < T ? xT[(t0 + j) * RS] : 0.f;
      grad_cascade<VT>(io, bsec, bser, band, ns, st, lane);
#pragma unroll
      for (int j = 0; j < kL; ++j)
        if (t0 + j < T) yT[(t0 + j) * RS] = io[j];
    }
    // 2. Z_jk of every frame, kGradKB bins at a time
    for (int k0 = klo; k0 <= khi; k0 += kGradKB) {
      const int nkb = min(kGradKB, khi - k0 + 1);
      for (int j = 0; j < J; ++j) {
        const int s0 = j * hop - half, n0 = max(0, -s0), n1 = min(N, T - s0);
        float2 acc[kGradKB];
#pragma unroll
        for (int q = 0; q < kGradKB; ++q) acc[q] = make_float2(0.f, 0.f);
        for (int n = n0; n < n1; ++n) {
          const float yw = yT[(s0 + n) * RS] * win[n];
#pragma unroll
          for (int q = 0; q < kGradKB; ++q)
            if (q < nkb) {
              const float2 e = grad_twiddle(tw, (k0 + q) * n, N);
              acc[q].x = fmaf(yw, e.x, acc[q].x);
              acc[q].y = fmaf(yw, e.y, acc[q].y);
            }
        }
#pragma unroll
        for (int q = 0; q < kGradKB; ++q)
          if (q < nkb) co[((int64_t)j * nkmax + (k0 - klo + q)) * RS] = make_float2(acc[q].x * scale, acc[q].y * scale);
      }
    }
    // 3. C_jk = c_jk Z_jk in place
    const float* gr = dfeat + ((bt * nb_out + gb.out[i]) * C + ch) * (int64_t)J;
    const float inv = 1.f / (float)nk;
    for (int j = 0; j < J; ++j) {
      float2* cj = co + (int64_t)j * nkmax * RS;
      const float g = gr[j];
      float P = 0.f;
      if (mode != ISD_BP_MAGNITUDE) {
        for (int k = 0; k < nk; ++k) {
          const float2 z = cj[k * RS];
          P = fmaf(z.x, z.x, fmaf(z.y, z.y, P));
        }
        P *= inv;
      }
      const float cp = mode == ISD_BP_LOGPOWER ? 2.f * scale * g * inv / (P + eps) : 2.f * scale * g * inv;
      for (int k = 0; k < nk; ++k) {
        const float2 z = cj[k * RS];
        float c = cp;
        if (mode == ISD_BP_MAGNITUDE) {
          const float a = sqrtf(fmaf(z.x, z.x, z.y * z.y));
          c = a > 0.f ? scale * g * inv / a : 0.f;
        }
        cj[k * RS] = make_float2(c * z.x, c * z.y);
      }
    }
    // 4. dy_b over y_b: frame by frame, Re(C e^{+i th}) = C.x cos th - C.y sin th with the table's (cos, -sin)
    for (int t = 0; t < T; ++t) yT[t * RS] = 0.f;
    for (int k0 = klo; k0 <= khi; k0 += kGradKB) {
      const int nkb = min(kGradKB, khi - k0 + 1);
      for (int j = 0; j < J; ++j) {
        float2 cc[kGradKB];
#pragma unroll
        for (int q = 0; q < kGradKB; ++q)
          cc[q] = q < nkb ? co[((int64_t)j * nkmax + (k0 - klo + q)) * RS] : make_float2(0.f, 0.f);
        const int s0 = j * hop - half, n0 = max(0, -s0), n1 = min(N, T - s0);
        for (int n = n0; n < n1; ++n) {
          float d = 0.f;
#pragma unroll
          for (int q = 0; q < kGradKB; ++q)
            if (q < nkb) {
              const float2 e = grad_twiddle(tw, (k0 + q) * n, N);
              d = fmaf(cc[q].x, e.x, fmaf(cc[q].y, e.y, d));
            }
          float* p = yT + (s0 + n) * RS;
          *p = fmaf(win[n], d, *p);
        }
      }
    }
    // 5. anti-causal pass R H_b R dy_b, added into dx (reversed sample q <-> t = T - 1 - q)
    for (int e = 0; e < 2 * ns; ++e) st[e * 64 + lane] = 0.0;
    for (int q0 = 0; q0 < T; q0 += kL) {
      float io[kL];
#pragma unroll
      for (int j = 0; j < kL; ++j) io[j] = q0 + j < T ? yT[(T - 1 - q0 - j) * RS] : 0.f;
      grad_cascade<VT>(io, bsec, bser, band, ns, st, lane);
#pragma unroll
      for (int j = 0; j < kL; ++j)
        if (q0 + j < T) {
          float* p = dT + (T - 1 - q0 - j) * RS;
          *p += io[j];
        }
    }
  }
  if (last) {
    float* dr = dx + row * (int64_t)T;
    for (int t = 0; t < T; ++t) dr[t] = dT[t * RS];
  }
}

// Workspace bytes per row, and the rows of one chunk (a multiple of 64, at most kGradWorkspaceCap bytes)
static int64_t grad_row_bytes(const isd_stft_plan* st, int nkmax) {
  return ((int64_t)3 * st->T + (int64_t)2 * st->J * nkmax) * (int64_t)sizeof(float);
}
static int64_t grad_chunk_rows(int64_t rows, int64_t row_bytes) {
  int64_t rc = (kGradWorkspaceCap / row_bytes) / 64 * 64;
  if (rc < 64) rc = 64;
  const int64_t all = cdiv(rows, 64) * 64;
  return rc < all ? rc : all;
}
// The band-bin tables checked, and the widest band (at least 1)
static int grad_bins(const isd_fb_plan* fb, const isd_stft_plan* st, const int* klo, const int* khi, int* lo, int* hi,
                     int& nkmax, const char* who) {
  const int rc = fill_band_args(st, fb->n_bands, klo, khi, lo, hi, who);
  if (rc) return rc;
  nkmax = 1;
  for (int b = 0; b < fb->n_bands; ++b)
    if (hi[b] - lo[b] + 1 > nkmax) nkmax = hi[b] - lo[b] + 1;
  return ISD_OK;
}

}  // namespace isd

extern "C" int64_t isd_features_backward_workspace_bytes(const isd_fb_plan* fb, const isd_stft_plan* st, int64_t B,
                                                         int64_t C, const int* klo, const int* khi) {
  ISD_CHECK_ARG(fb && st, "isd_features_backward_workspace_bytes: null plan");
  ISD_CHECK_ARG(B >= 0 && C >= 1 && C <= (1 << 20), "isd_features_backward_workspace_bytes: bad shape B=%lld C=%lld",
                (long long)B, (long long)C);
  int lo[kMaxBands], hi[kMaxBands], nkmax = 1;
  const int rc = grad_bins(fb, st, klo, khi, lo, hi, nkmax, "isd_features_backward_workspace_bytes");
  if (rc) return rc;
  if (B == 0) return 0;
  const int64_t rb = grad_row_bytes(st, nkmax);
  return grad_chunk_rows(B * C, rb) * rb;
}

extern "C" int isd_features_backward(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x, const float* dfeat,
                                     float* dx, void* workspace, int64_t B, int64_t C, const int* klo, const int* khi,
                                     int mode, float eps, void* stream) {
  ISD_CHECK_ARG(mode >= ISD_BP_MAGNITUDE && mode <= ISD_BP_LOGPOWER, "isd_features_backward: bad mode %d", mode);
  ISD_CHECK_ARG(B >= 0 && C >= 1 && C <= (1 << 20), "isd_features_backward: bad shape B=%lld C=%lld", (long long)B,
                (long long)C);
  ISD_CHECK_ARG(fb && st, "isd_features_backward: null plan");
  ISD_CHECK_ARG(B == 0 || (x && dfeat && dx && workspace), "isd_features_backward: null argument");
  int lo[kMaxBands], hi[kMaxBands], nkmax = 1;
  const int rc = grad_bins(fb, st, klo, khi, lo, hi, nkmax, "isd_features_backward");
  if (rc) return rc;
  if (B == 0) return ISD_OK;
  ISD_CHECK_ARG(B * C <= kMaxRows, "isd_features_backward: too many rows (%lld)", (long long)(B * C));
  GradBands gb[2] = {};
  int nsets = 0;
  for (int k = 0; k < 2; ++k) {
    for (int i = 0; i < fb->set[k].nb; ++i) {
      const int b = fb->host_map[k][i];
      gb[k].out[i] = b;
      gb[k].klo[i] = lo[b];
      gb[k].khi[i] = hi[b];
    }
    if (fb->set[k].nb) ++nsets;
  }
  const int64_t rows = B * C, RS = grad_chunk_rows(rows, grad_row_bytes(st, nkmax));
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  for (int64_t r0 = 0; r0 < rows; r0 += RS) {
    const int n = (int)(rows - r0 < RS ? rows - r0 : RS);
    int done = 0;
    for (int k = 0; k < 2; ++k) {
      const FbSet& fs = fb->set[k];
      if (!fs.nb) continue;
      const int first = done == 0, last = done == nsets - 1;
      const dim3 grid((unsigned)cdiv(n, 64));
static constexpr decltype(&features_grad_kernel<float>) kern[2] = {features_grad_kernel<float>,
                                                                        features_grad_kernel<double>};
      const int rc_k = launch_lds(kern[k], grid, dim3(64), 0, s, fs.d_sec, fs.d_ser, fs.d_band, gb[k], fs.nb,
                                  fb->n_sections, st->d_win, st->d_tw, x, dfeat, dx, ws, r0, n, RS, (int)C, st->T, st->n,
                                  st->hop, st->J, fb->n_bands, nkmax, st->scale, mode, eps, first, last);
      if (rc_k) return rc_k;
      ++done;
    }
  }
  return ISD_OK;
}

// ------------------------------------------------------------------------------------------------ filter-bank CSP
// The two data-sized steps of isd_amd.FBCSP (Ang et al. 2008: one CSP per band of a filterbank), without the
// [n][n_bands][C][T] filtered map in memory.  Both run a band's gain and cascade with grad_cascade: one row per lane,
// a 32-sample chunk at a time, the section states carried in LDS and cleared at the start of every workgroup, so a
// trial's result does not depend on the batch or on earlier launches.
//
//   fb_cov_kernel   cov[i][b] = Y Y^T / T, Y = band b of trial i.  A workgroup has one trial and BW bands; a band has
//                   NW waves (1 for C <= 64, 2 above), lane = channel.  Per chunk the workgroup stages the trial's x
//                   rows in LDS once (coalesced along T, fetched into registers one chunk ahead), every wave filters
//                   its rows and writes them, samples past T zeroed, into its band's [64 NW][32 + 4] LDS tile, and the
//                   band's waves feed the UPPER 16x16 tiles to v_mfma_f32_16x16x4_f32 as trial_cov_kernel does
//                   (csp.hip): 10 tiles in one wave at C = 64, 36 over two waves at C = 128.  Elements on or above the
//                   diagonal are stored twice, at [a][c] and [c][a].
//   fb_pow_kernel   out[i][b][j] = mean_t y^2, y = band b of the projected row z = sum_c w[b][j][c] x_i[c][.]: the
//                   projection commutes with the filter and leaves m rows to filter instead of C.  A workgroup has G
//                   trials and up to four bands, one wave per band, lane = (trial, component).  Per chunk the workgroup
//                   stages its trials' x rows in LDS (fetched one chunk ahead), every wave forms z = W_b x of each trial
//                   on the matrix cores (two 16x16 tiles, W_b's fragments in registers for the whole kernel) into its
//                   own LDS tile, every lane reads its row, filters it and adds y^2 sample by sample, chunk by chunk:
//                   a fixed order.
namespace isd {

constexpr int kFcLD = kL + 4;                         // LDS row stride of a chunk tile (floats): 16-byte rows, skewed banks
constexpr int kFcStateDoubles = 2 * 64;               // carried state of one section of one wave
constexpr size_t kFcMaxLds = 160 * 1024;

template <typename VT, int NW, int BW>
__global__ __launch_bounds__(64 * NW * BW) void fb_cov_kernel(
    const FbSec* __restrict__ secs, const SerSec* __restrict__ sers, const FbBand* __restrict__ bands,
    const int* __restrict__ map, int nb, int ns, int nb_out, const float* __restrict__ x, float* __restrict__ cov,
    int C, int T) {
  constexpr int NT = 64 * NW * BW, ROWS = 64 * NW, LD = kFcLD, MAXQ = NW == 1 ? 10 : 18;
  constexpr int NPRE = (ROWS * kL + NT - 1) / NT;      // staged elements per thread and chunk
  extern __shared__ __attribute__((aligned(16))) unsigned char fc_smem[];
  double* st_all = reinterpret_cast<double*>(fc_smem);                   // [BW * NW][ns][2][64]
  float* xs = reinterpret_cast<float*>(st_all + BW * NW * ns * kFcStateDoubles);   // [ROWS][LD]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wb = wave / NW, wc = wave % NW;
  const int groups = (nb + BW - 1) / BW;
  const int trial = blockIdx.x / groups, bi = (blockIdx.x % groups) * BW + wb;
  const bool active = bi < nb;                                           // wave-uniform
  float* ys = xs + ROWS * LD + wb * ROWS * LD;                           // the band's filtered chunk, [ROWS][LD]
  double* st = st_all + wave * ns * kFcStateDoubles;
  const int nt = (C + 15) >> 4, Cp = nt * 16, U = nt * (nt + 1) / 2;
  const float* xi = x + (int64_t)trial * C * T;
  const int ch = wc * 64 + lane;                                         // the lane's channel

  for (int e = 0; e < 2 * ns; ++e) st[e * 64 + lane] = 0.0;
  int ti[MAXQ], tj[MAXQ];
  f32x4 acc[MAXQ];
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) {
    int u = q * NW + wc, a = 0;                                          // u-th upper tile, row-major over (ti <= tj)
    while (a < nt && u >= nt - a) { u -= nt - a; ++a; }
    ti[q] = a;
    tj[q] = a + u;
    acc[q] = (f32x4)(0.f);
  }
  const FbSec* bsec = secs + (active ? bi : 0) * ns;
  const SerSec* bser = std::is_same<VT, float>::value ? sers + (active ? bi : 0) * ns : nullptr;
  const FbBand band = bands[active ? bi : 0];

  float pre[NPRE];
#pragma unroll
  for (int i = 0; i < NPRE; ++i) {
    const int e = i * NT + tid, c = e >> 5, k = e & 31;
    // never past a row, never past C rows; branch-free (loads behind a branch are waited for one by one) and not
    // looked at before the store below (a select here would wait for the load)
    pre[i] = xi[(c < C && k < T) ? (int64_t)c * T + k : 0];
  }
  for (int t0 = 0; t0 < T; t0 += kL) {
    __syncthreads();                                                     // the previous chunk has been consumed
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int e = i * NT + tid, c = e >> 5, k = e & 31;
      if (e < Cp * kL) xs[c * LD + k] = (c < C && t0 + k < T) ? pre[i] : 0.f;   // rows C .. Cp - 1 are zeros
    }
    __syncthreads();
    if (t0 + kL < T) {
#pragma unroll
      for (int i = 0; i < NPRE; ++i) {
        const int e = i * NT + tid, c = e >> 5, t = t0 + kL + (e & 31);
        pre[i] = xi[(c < C && t < T) ? (int64_t)c * T + t : 0];
      }
    }
    if (active) {
      float io[kL];
      float4 xv[kL / 4];                                                 // rows >= Cp of xs are never written:
#pragma unroll
      for (int q = 0; q < kL / 4; ++q) xv[q] = *reinterpret_cast<const float4*>(xs + ch * LD + 4 * q);
#pragma unroll
      for (int q = 0; q < kL / 4; ++q) {                                 // their lanes filter zeros
        io[4 * q] = ch < Cp ? xv[q].x : 0.f; io[4 * q + 1] = ch < Cp ? xv[q].y : 0.f;
        io[4 * q + 2] = ch < Cp ? xv[q].z : 0.f; io[4 * q + 3] = ch < Cp ? xv[q].w : 0.f;
      }
      grad_cascade<VT>(io, bsec, bser, band, ns, st, lane);
#pragma unroll
      for (int j = 0; j < kL; ++j) io[j] = t0 + j < T ? io[j] : 0.f;     // the filter rings on past T: not part of Y
#pragma unroll
      for (int q = 0; q < kL / 4; ++q)
        *reinterpret_cast<float4*>(ys + ch * LD + 4 * q) = make_float4(io[4 * q], io[4 * q + 1], io[4 * q + 2], io[4 * q + 3]);
    }
    if constexpr (NW == 1) wave_lds_sync(); else __syncthreads();        // the band's tile is complete
    if (NW == 1 && nt == 4) {
      if (active) {                                                      // all ten tiles: four row blocks feed them
        float a[4][kL / 4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
          for (int k = 0; k < kL / 4; ++k) a[rb][k] = ys[(rb * 16 + (lane & 15)) * LD + (lane >> 4) + 4 * k];
        __builtin_amdgcn_sched_barrier(0);                               // every fragment is requested before the first MFMA
#pragma unroll
        for (int k = 0; k < kL / 4; ++k) {
          int u = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j, ++u)
              if (u < MAXQ) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][k], a[j][k], acc[u], 0, 0, 0);
        }
      }
    } else if (active) {
#pragma unroll
      for (int q = 0; q < MAXQ; ++q) {
        if (q * NW + wc < U) {                                           // wave-uniform
          const float* pa = ys + (ti[q] * 16 + (lane & 15)) * LD + (lane >> 4);
          const float* pb = ys + (tj[q] * 16 + (lane & 15)) * LD + (lane >> 4);
#pragma unroll
          for (int k = 0; k < kL; k += 4) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k], pb[k], acc[q], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  float* ci = cov + ((int64_t)trial * nb_out + map[bi]) * C * C;
  const float den = (float)T;
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) {
    if (q * NW + wc < U) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = ti[q] * 16 + 4 * (lane >> 4) + r, b = tj[q] * 16 + (lane & 15);
        if (a <= b && b < C) {                                           // a <= b < C; the lower triangle is the mirror
          const float v = acc[q][r] / den;
          ci[a * C + b] = v;
          ci[b * C + a] = v;
        }
      }
    }
  }
}

constexpr int kFpWaves = 4, kFpNT = 64 * kFpWaves;    // fb_pow_kernel: four waves stage, up to four own a band
constexpr int kFpRows = 512;                          // staged rows (trials x channels padded to 16) per workgroup
constexpr int kFpPre = kFpRows * kL / kFpNT;          // staged elements per thread and chunk

// G trials per workgroup (G m <= 64, G CP <= kFpRows with CP = C rounded up to 16), BW <= 4 bands
template <typename VT>
__global__ __launch_bounds__(kFpNT) void fb_pow_kernel(
    const FbSec* __restrict__ secs, const SerSec* __restrict__ sers, const FbBand* __restrict__ bands,
    const int* __restrict__ map, int nb, int ns, int nb_out, const float* __restrict__ x, const float* __restrict__ w,
    float* __restrict__ out, int64_t n, int C, int T, int m, int G, int BW, int take_log) {
  constexpr int LD = kFcLD;
  extern __shared__ __attribute__((aligned(16))) unsigned char fp_smem[];
  double* st_all = reinterpret_cast<double*>(fp_smem);                   // [kFpWaves][ns][2][64]
  float* zt_all = reinterpret_cast<float*>(st_all + kFpWaves * ns * kFcStateDoubles);   // [kFpWaves][64][LD]
  float* xs = zt_all + kFpWaves * 64 * LD;                               // [G][CP][LD], rows C .. CP - 1 zeros
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int CP = (C + 15) & ~15, GR = G * CP, nkg = CP >> 4;
  const int groups = (nb + BW - 1) / BW;
  const int64_t trial0 = (int64_t)(blockIdx.x / groups) * G;
  const int bi = (blockIdx.x % groups) * BW + wave;
  const bool active = wave < BW && bi < nb;                              // wave-uniform
  double* st = st_all + wave * ns * kFcStateDoubles;
  float* zt = zt_all + wave * 64 * LD;                                   // the wave's projected rows, row = lane
  const int g_l = lane / m, j_l = lane - g_l * m;
  const bool lane_ok = g_l < G && trial0 + g_l < n;                      // the last lanes and the last group have no trial
  const int64_t left = n - trial0;
  const int Gn = left < G ? (int)left : G;                               // trials of this workgroup that exist
  const float* xg = x + trial0 * C * T;
  const int aj = lane & 15, ac = lane >> 4;                              // MFMA operand position

  for (int e = 0; e < 2 * ns; ++e) st[e * 64 + lane] = 0.0;
  const int band_out = map[active ? bi : 0];
  const FbSec* bsec = secs + (active ? bi : 0) * ns;
  const SerSec* bser = std::is_same<VT, float>::value ? sers + (active ? bi : 0) * ns : nullptr;
  const FbBand band = bands[active ? bi : 0];
  float wa[32];                                                          // A fragments: wa[ks] = w[band][aj][4 ks + ac]
  {
    const float* wb = w + (int64_t)band_out * m * C;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
      const int c = 4 * ks + ac;
      wa[ks] = (active && aj < m && c < C) ? wb[aj * C + c] : 0.f;
    }
  }

  // staging: thread (rsub, k) owns sample k of the rows i * 8 + rsub; CP is a multiple of 8, so the trial of row
  // block i is wave-uniform
  const int rsub = tid >> 5, kk = tid & 31;
  float pre[kFpPre];
  auto fetch = [&](int t0) {
    int g = 0, cb = 0;
#pragma unroll
    for (int i = 0; i < kFpPre; ++i) {
      const int c = cb + rsub, t = t0 + kk;
      // never past x; branch-free (loads behind a branch are waited for one by one) and not looked at before the
      // store (a select here would wait for the load)
      pre[i] = xg[(i * 8 < GR && g < Gn && c < C && t < T) ? ((int64_t)g * C + c) * T + t : 0];
      const bool wrap = cb + 8 >= CP;
      cb = wrap ? 0 : cb + 8;
      g += wrap ? 1 : 0;
    }
  };
  fetch(0);
  float sq = 0.f;
  for (int t0 = 0; t0 < T; t0 += kL) {
    __syncthreads();                                                     // the previous chunk has been consumed
    {
      int g = 0, cb = 0;
#pragma unroll
      for (int i = 0; i < kFpPre; ++i) {
        if (i * 8 < GR) xs[(i * 8 + rsub) * LD + kk] = (g < Gn && cb + rsub < C && t0 + kk < T) ? pre[i] : 0.f;
        const bool wrap = cb + 8 >= CP;
        cb = wrap ? 0 : cb + 8;
        g += wrap ? 1 : 0;
      }
    }
    __syncthreads();
    if (t0 + kL < T) fetch(t0 + kL);
    if (active) {
      for (int g = 0; g < G; ++g) {                                      // z = W x of trial g: [16][32] in two tiles
        const float* xb = xs + (g * CP + ac) * LD + aj;
        f32x4 z0 = (f32x4)(0.f), z1 = (f32x4)(0.f);
        float b0[32], b1[32];                                            // the trial's B fragments, all requested
#pragma unroll
        for (int kg = 0; kg < 8; ++kg) {                                 // before the first MFMA
          if (kg < nkg) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int ks = kg * 4 + u;
              b0[ks] = xb[4 * ks * LD];
              b1[ks] = xb[4 * ks * LD + 16];
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kg = 0; kg < 8; ++kg) {
          if (kg < nkg) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int ks = kg * 4 + u;
              z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ks], b0[ks], z0, 0, 0, 0);
              z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ks], b1[ks], z1, 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 4 * ac + r;
          if (j < m) {
            zt[(g * m + j) * LD + aj] = z0[r];
            zt[(g * m + j) * LD + 16 + aj] = z1[r];
          }
        }
      }
      wave_lds_sync();
      float io[kL];
      float4 zv[kL / 4];                                                 // rows >= G m of zt are never written:
#pragma unroll
      for (int q = 0; q < kL / 4; ++q) zv[q] = *reinterpret_cast<const float4*>(zt + lane * LD + 4 * q);
#pragma unroll
      for (int q = 0; q < kL / 4; ++q) {                                 // their lanes filter zeros
        io[4 * q] = g_l < G ? zv[q].x : 0.f; io[4 * q + 1] = g_l < G ? zv[q].y : 0.f;
        io[4 * q + 2] = g_l < G ? zv[q].z : 0.f; io[4 * q + 3] = g_l < G ? zv[q].w : 0.f;
      }
      grad_cascade<VT>(io, bsec, bser, band, ns, st, lane);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kL; ++i) s = t0 + i < T ? fmaf(io[i], io[i], s) : s;     // the ringing past T is not summed
      sq += s;
      wave_lds_sync();                                                   // the rows are read before the next chunk's
    }
  }
  if (active && lane_ok) {
    const float v = sq / (float)T;
    out[((trial0 + g_l) * nb_out + band_out) * m + j_l] = take_log ? logf(v) : v;
  }
}

// bands of one workgroup: the split of nb bands into groups of 3 or 4 that leaves fewer idle waves
static int fc_band_waves(int nb) {
  if (nb <= 2) return 1;
  const int w3 = (int)cdiv(nb, 3) * 3 - nb, w4 = (int)cdiv(nb, 4) * 4 - nb;
  return w3 < w4 ? 3 : 4;
}

template <typename VT>
static int fb_cov_launch(const FbSet& fs, int ns, int nb_out, const float* x, float* cov, int64_t n, int C, int T,
                         hipStream_t st) {
  const int NW = C > 64 ? 2 : 1, BW = NW == 2 ? 1 : fc_band_waves(fs.nb);
  const int64_t blocks = n * cdiv(fs.nb, BW);
  ISD_CHECK_ARG(blocks <= 0x7fffffffLL, "isd_fb_trial_cov: n=%lld trials of %d bands are too many for one launch",
                (long long)n, fs.nb);
  const size_t lds = sizeof(double) * BW * NW * ns * kFcStateDoubles + sizeof(float) * (1 + BW) * 64 * NW * kFcLD;
  const dim3 grid((unsigned)blocks), block(64 * NW * BW);
#define ISD_FC_COV(NW_, BW_)                                                                                        \
  return launch_lds(fb_cov_kernel<VT, NW_, BW_>, grid, block, lds, st, fs.d_sec, fs.d_ser, fs.d_band, fs.d_map,     \
                    fs.nb, ns, nb_out, x, cov, C, T)
  if (NW == 2) ISD_FC_COV(2, 1);
  if (BW == 1) ISD_FC_COV(1, 1);
  if (BW == 3) ISD_FC_COV(1, 3);
  ISD_FC_COV(1, 4);
#undef ISD_FC_COV
}

template <typename VT>
static int fb_pow_launch(const FbSet& fs, int ns, int nb_out, const float* x, const float* w, float* out, int64_t n,
                         int C, int T, int m, int take_log, hipStream_t st) {
  const int BW = fs.nb <= kFpWaves ? fs.nb : fc_band_waves(fs.nb);
  const int CP = (C + 15) / 16 * 16;
  int G = 64 / m;                                       // lanes of a wave
  if (G > kFpRows / CP) G = kFpRows / CP;               // 72 KiB of staged rows at the most
  const int64_t blocks = cdiv(n, G) * cdiv(fs.nb, BW);
  ISD_CHECK_ARG(blocks <= 0x7fffffffLL, "isd_fb_csp_power: n=%lld trials of %d bands are too many for one launch",
                (long long)n, fs.nb);
  const size_t lds = sizeof(double) * kFpWaves * ns * kFcStateDoubles +
                     sizeof(float) * ((size_t)kFpWaves * 64 + (size_t)G * CP) * kFcLD;
  ISD_CHECK_ARG(lds <= kFcMaxLds, "isd_fb_csp_power: %zu bytes of LDS", lds);
  return launch_lds(fb_pow_kernel<VT>, dim3((unsigned)blocks), dim3(kFpNT), lds, st, fs.d_sec, fs.d_ser, fs.d_band,
                    fs.d_map, fs.nb, ns, nb_out, x, w, out, n, C, T, m, G, BW, take_log);
}

}  // namespace isd

// The shape is checked before the pointers, so a bad shape is refused whatever else is passed.
extern "C" int isd_fb_trial_cov(const isd_fb_plan* plan, const float* x, float* cov, int64_t n, int C, int T,
                                void* stream) {
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL, "isd_fb_trial_cov: n=%lld", (long long)n);
  ISD_CHECK_ARG(C >= 1 && C <= 128 && T >= 1 && T <= 0x7fffffff - kL,
                "isd_fb_trial_cov: C=%d T=%d (need 1 <= C <= 128, T >= 1)", C, T);
  ISD_CHECK_ARG(plan, "isd_fb_trial_cov: null plan");
  ISD_CHECK_ARG(x && cov, "isd_fb_trial_cov: null argument");
  if (n == 0) return ISD_OK;
  for (int k = 0; k < 2; ++k) {
    const FbSet& fs = plan->set[k];
    if (!fs.nb) continue;
    const int rc = k == 0 ? fb_cov_launch<float>(fs, plan->n_sections, plan->n_bands, x, cov, n, C, T, (hipStream_t)stream)
                          : fb_cov_launch<double>(fs, plan->n_sections, plan->n_bands, x, cov, n, C, T, (hipStream_t)stream);
    if (rc) return rc;
  }
  return ISD_OK;
}

extern "C" int isd_fb_csp_power(const isd_fb_plan* plan, const float* x, const float* w, float* out, int64_t n, int C,
                                int T, int m, int take_log, void* stream) {
  ISD_CHECK_ARG(n >= 0 && n <= 2147483647LL, "isd_fb_csp_power: n=%lld", (long long)n);
  ISD_CHECK_ARG(C >= 1 && C <= 128 && T >= 1 && T <= 0x7fffffff - kL && m >= 1 && m <= 16,
                "isd_fb_csp_power: C=%d T=%d m=%d (need 1 <= C <= 128, T >= 1, 1 <= m <= 16)", C, T, m);
  ISD_CHECK_ARG(plan, "isd_fb_csp_power: null plan");
  ISD_CHECK_ARG(x && w && out, "isd_fb_csp_power: null argument");
  if (n == 0) return ISD_OK;
  for (int k = 0; k < 2; ++k) {
    const FbSet& fs = plan->set[k];
    if (!fs.nb) continue;
    const int rc = k == 0 ? fb_pow_launch<float>(fs, plan->n_sections, plan->n_bands, x, w, out, n, C, T, m, take_log,
                                                 (hipStream_t)stream)
                          : fb_pow_launch<double>(fs, plan->n_sections, plan->n_bands, x, w, out, n, C, T, m, take_log,
                                                  (hipStream_t)stream);
    if (rc) return rc;
  }
  return ISD_OK;
}
