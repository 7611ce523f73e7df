// flexam_amd/csrc/raster_colors.hip -- the colour tables of the conditioning videos, on the device
// (flexam_amd/conditioning_raster.py; the reference: pipelines.py:1523-1545 tracking, :1775-1792 depth, :1675-1692 cosine codes).
//
// Everything in a colour table is arithmetic per point EXCEPT its percentiles (np.percentile over the first frame, over the whole
// clip, and per frame over the visible points).  They are exact order statistics, found here by radix selection:
//   select_hist_kernel   one pass over the values per 8-bit digit of an order-preserving 32-bit code of the float.  A workgroup keeps
//                        one LDS histogram per wanted rank (ranks whose prefixes still agree share one), fed by wave-aggregated LDS
//                        atomics -- a scene's depths share their exponent, so the first digits have a handful of live bins -- and
//                        flushes its non-empty bins with integer atomics.  The z component of [.., 3] points is read as the wave's
//                        768 contiguous bytes, each lane keeping the dword that is its value; the inverse-depth transform is applied
//                        in registers.
//   select_pick_kernel   one workgroup per segment between passes: the bin each rank falls into extends its prefix.
// Integer sums only: the same bits on every run; no flags or waits across workgroups.  numpy's interpolation between the two
// neighbouring order statistics (select_lerp_kernel) and the per-point colour kernels follow, contraction off, divisions correctly
// rounded, so that the bytes are the host expressions' bytes.
#include "common.h"
#include "flexam_hip.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_KMAX = FLEXAM_SELECT_MAX_RANKS;
constexpr int SEL_BINS = 256;
constexpr int SEL_UNROLL = 4;                                  // 64-value wave tiles a wave has in flight
constexpr int SEL_TILE = SEL_THREADS * SEL_UNROLL;             // values a workgroup takes per step
constexpr int SEL_GRID = 2048;                                 // workgroups of a pass, over all segments
// workspace of one segment, in 32-bit words: histograms [KMAX][BINS], then per rank its prefix, its leader (the first rank with the
// same prefix, whose histogram it shares) and the rank that remains inside the prefix
constexpr int SEL_PREFIX = SEL_KMAX * SEL_BINS, SEL_LEAD = SEL_PREFIX + SEL_KMAX, SEL_REM = SEL_LEAD + SEL_KMAX;
constexpr int SEL_WS_WORDS = SEL_REM + 2 * SEL_KMAX;
static_assert(SEL_WS_WORDS * 4 == FLEXAM_SELECT_WS_SEGMENT_BYTES, "FLEXAM_SELECT_WS_SEGMENT_BYTES follows the layout");
constexpr int COL_THREADS = 256;

// ascending float -> ascending code; every NaN above everything (numpy sorts NaN last); -0 just below +0
__device__ __forceinline__ unsigned float_code(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float code_float(unsigned c) {
  return __uint_as_float((c & 0x80000000u) ? (c ^ 0x80000000u) : ~c);           // 0xFFFFFFFF -> 0x7FFFFFFF, a NaN
}

// hist[digit] += 1 for the lanes with `pred`.  Two rounds in which the first live lane's digit is counted for the whole wave by
// ballot (equal digits would otherwise serialise on one LDS address), then plain LDS atomics for what is left.
__device__ __forceinline__ void hist_add(unsigned* hist, bool pred, unsigned digit, int lane) {
  unsigned long long live = __ballot(pred);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (!live) return;
    const int first = __ffsll((long long)live) - 1;
    const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, __builtin_amdgcn_readfirstlane(first));
    const unsigned long long same = __ballot(pred && digit == d);
    if (lane == first) atomicAdd(&hist[d], (unsigned)__popcll(same));
    pred = pred && digit != d;
    live &= ~same;
  }
  if (pred) atomicAdd(&hist[digit], 1u);
}

template <bool kStride3>
__global__ __launch_bounds__(SEL_THREADS) void select_hist_kernel(const float* __restrict__ src, int stride, int comp, int transform,
                                                                  const unsigned char* __restrict__ mask, int64_t seg_len, int K, int shift,
                                                                  unsigned* __restrict__ ws, unsigned long long* __restrict__ info) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[SEL_KMAX * SEL_BINS];
  __shared__ unsigned s_prefix[SEL_KMAX], s_live[SEL_KMAX], s_flags;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.y;
  unsigned* seg_ws = ws + (int64_t)s * SEL_WS_WORDS;
  const bool first = shift == 24;                    // no prefix yet: one histogram serves every rank (and counts the valid values)
  const int nk = first ? 1 : K;
  for (int i = tid; i < nk * SEL_BINS; i += SEL_THREADS) hist[i] = 0;
  if (tid < SEL_KMAX) {
    s_prefix[tid] = (first || tid >= nk) ? 0u : seg_ws[SEL_PREFIX + tid];
    s_live[tid] = tid < nk && (first || seg_ws[SEL_LEAD + tid] == (unsigned)tid);
  }
  if (tid == 0) s_flags = 0;
  __syncthreads();
  const int64_t seg0 = (int64_t)s * seg_len;
  const int own = kStride3 ? (comp + 3 - lane % 3) % 3 : 0;              // which of the lane's three dwords is a value: (lane + 64 j) % 3 == comp
  unsigned flags = 0;
  for (int64_t base = (int64_t)blockIdx.x * SEL_TILE; base < seg_len; base += (int64_t)gridDim.x * SEL_TILE) {
    float v[SEL_UNROLL];
    bool valid[SEL_UNROLL];
#pragma unroll
    for (int u = 0; u < SEL_UNROLL; ++u) {
      const int64_t i0 = base + (int64_t)(u * (SEL_THREADS / 64) + wave) * 64;      // the wave's 64 values: i0 .. i0 + 63 of the segment
      int64_t i;
      v[u] = 0.f;
      if (kStride3) {
        const float* p = src + (seg0 + i0) * 3;
        const int64_t left = (seg_len - i0) * 3;                                    // floats of this segment from p on (<= 0: none)
        const float f0 = lane < left ? p[lane] : 0.f, f1 = lane + 64 < left ? p[lane + 64] : 0.f, f2 = lane + 128 < left ? p[lane + 128] : 0.f;
        v[u] = own == 0 ? f0 : own == 1 ? f1 : f2;
        i = i0 + (lane + 64 * own) / 3;
      } else {
        i = i0 + lane;
        if (i < seg_len) v[u] = src[(seg0 + i) * stride + comp];
      }
      valid[u] = i < seg_len && (!mask || mask[seg0 + i] != 0);
    }
#pragma unroll
    for (int u = 0; u < SEL_UNROLL; ++u) {
      float x = v[u];
      if (first && valid[u] && !(x == 0.f)) flags |= 2u;
      if (transform == 1) x = __fdiv_rn(1.0f, x + 1e-10f);
      if (first && valid[u] && x != x) flags |= 1u;
      const unsigned code = float_code(x);
      const unsigned digit = (code >> shift) & 0xFFu;
      for (int k = 0; k < nk; ++k) {
        if (!s_live[k]) continue;
        const bool in = valid[u] && (first || ((code ^ s_prefix[k]) >> (shift + 8)) == 0);
        hist_add(hist + k * SEL_BINS, in, digit, lane);
      }
    }
  }
  if (first && flags) atomicOr(&s_flags, flags);
  __syncthreads();
  for (int i = tid; i < nk * SEL_BINS; i += SEL_THREADS) {
    const unsigned c = hist[i];
    if (c) atomicAdd(&seg_ws[i], c);
  }
  if (first && tid == 0 && s_flags) {
    if (s_flags & 1u) atomicOr(&info[(int64_t)s * 4 + 1], 1ull);
    if (s_flags & 2u) atomicOr(&info[(int64_t)s * 4 + 2], 1ull);
  }
}

// inclusive scan of one unsigned per thread over the workgroup's 256 threads
__device__ __forceinline__ unsigned block_inclusive_scan(unsigned own, unsigned* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  __syncthreads();                                   // `part` may still be read from the previous use
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += part[w];
  return incl;
}

// one workgroup per segment, thread = bin: every rank's prefix grows by the digit whose bin holds it
__global__ __launch_bounds__(SEL_THREADS) void select_pick_kernel(unsigned* __restrict__ ws, const int64_t* __restrict__ ranks, int K, int shift,
                                                                  float* __restrict__ values, unsigned long long* __restrict__ info) {
  __shared__ unsigned part[SEL_THREADS / 64], s_bin[SEL_KMAX], s_below[SEL_KMAX], s_rem[SEL_KMAX], s_prefix[SEL_KMAX], s_n;
  const int tid = threadIdx.x, s = blockIdx.x;
  unsigned* seg_ws = ws + (int64_t)s * SEL_WS_WORDS;
  const bool first = shift == 24;
  unsigned n;
  if (first) {
    const unsigned total = block_inclusive_scan(seg_ws[tid], part);
    if (tid == SEL_THREADS - 1) {
      info[(int64_t)s * 4] = total;
      s_n = total;
    }
    __syncthreads();
    n = s_n;
  } else {
    n = (unsigned)info[(int64_t)s * 4];
  }
  if (tid < SEL_KMAX) s_bin[tid] = s_below[tid] = s_rem[tid] = 0;
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    unsigned lead = 0, rem;
    if (first) {
      const int64_t r = ranks[(int64_t)s * K + k];
      rem = n == 0 ? 0u : r < 0 ? 0u : r >= (int64_t)n ? n - 1 : (unsigned)r;      // ranks past the end: the last element
    } else {
      lead = seg_ws[SEL_LEAD + k];
      rem = seg_ws[SEL_REM + k];
    }
    const unsigned c = seg_ws[lead * SEL_BINS + tid];
    const unsigned incl = block_inclusive_scan(c, part);
    if (incl - c <= rem && rem < incl) {             // one thread at most (none when n == 0)
      s_bin[k] = tid;
      s_below[k] = incl - c;
    }
    if (tid == 0) s_rem[k] = rem;
  }
  __syncthreads();
  if (tid < K) s_prefix[tid] = (first ? 0u : seg_ws[SEL_PREFIX + tid]) | (s_bin[tid] << shift);
  __syncthreads();
  for (int i = tid; i < K * SEL_BINS; i += SEL_THREADS) seg_ws[i] = 0;              // every histogram was read above: clear for the next pass
  if (tid < K) {
    int lead = tid;
    for (int j = tid - 1; j >= 0; --j)
      if (s_prefix[j] == s_prefix[tid]) lead = j;
    seg_ws[SEL_PREFIX + tid] = s_prefix[tid];
    seg_ws[SEL_LEAD + tid] = (unsigned)lead;
    seg_ws[SEL_REM + tid] = s_rem[tid] - s_below[tid];
    if (shift == 0) values[(int64_t)s * K + tid] = n ? code_float(s_prefix[tid]) : __uint_as_float(0x7FC00000u);
  }
}

__global__ __launch_bounds__(COL_THREADS) void select_lerp_kernel(const float* __restrict__ values, const double* __restrict__ gamma,
                                                                  const unsigned long long* __restrict__ info, int total, int Q, int f32_form,
                                                                  void* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * COL_THREADS + threadIdx.x;
  if (i >= total) return;
  const int s = i / Q;
  const float lo = values[2 * i], hi = values[2 * i + 1];
  const float d = hi - lo;
  const bool none = info[(int64_t)s * 4] == 0 || info[(int64_t)s * 4 + 1] != 0;
  if (f32_form) {
    const float g = (float)gamma[i];
    const float a = d * g, b = d * (1.0f - g);
    const float r = g >= 0.5f ? hi - b : lo + a;
    reinterpret_cast<float*>(out)[i] = none ? __uint_as_float(0x7FC00000u) : r;
  } else {
    const double g = gamma[i];
    const double a = (double)d * g, b = (double)d * (1.0 - g);
    const double r = g >= 0.5 ? (double)hi - b : (double)lo + a;
    reinterpret_cast<double*>(out)[i] = none ? __longlong_as_double(0x7FF8000000000000ll) : r;
  }
}

// (np.clip(x, 0, 1) * 255).astype(np.uint8) in float32; NaN -> 0
__device__ __forceinline__ unsigned char unit_byte(float x) {
#pragma clang fp contract(off)
  if (x != x) return 0;
  const float c = x < 0.f ? 0.f : x > 1.f ? 1.f : x;
  return (unsigned char)(int)(c * 255.0f);
}

// the workgroup's 256 rows of 3 bytes leave as 192 dwords (a tail workgroup: as bytes); `first` = its first row
__device__ __forceinline__ void store_rows(unsigned char* __restrict__ out, int64_t first, int64_t rows, unsigned char r, unsigned char g,
                                           unsigned char b) {
  __shared__ unsigned stage[COL_THREADS * 3 / 4];
  unsigned char* st = reinterpret_cast<unsigned char*>(stage);
  const int tid = threadIdx.x;
  st[3 * tid] = r;
  st[3 * tid + 1] = g;
  st[3 * tid + 2] = b;
  __syncthreads();
  const int64_t left = rows - first;                 // > 0
  if (left >= COL_THREADS) {
    if (tid < COL_THREADS * 3 / 4) reinterpret_cast<unsigned*>(out + first * 3)[tid] = stage[tid];       // first * 3 = 768 * block: 4-byte aligned
  } else if (tid < left) {
    out[(first + tid) * 3] = r;
    out[(first + tid) * 3 + 1] = g;
    out[(first + tid) * 3 + 2] = b;
  }
}

__global__ __launch_bounds__(COL_THREADS) void colors_tracking_kernel(const float* __restrict__ pts, int64_t N, float W, float H,
                                                                      const float* __restrict__ pct, const unsigned char* __restrict__ blue,
                                                                      unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t first = (int64_t)blockIdx.x * COL_THREADS, n = first + threadIdx.x;
  unsigned char r = 0, g = 0, b = 0;
  if (n < N) {
    const float u = pts[n * 3], v = pts[n * 3 + 1], z = pts[n * 3 + 2];
    r = unit_byte(__fdiv_rn(u, W));
    g = unit_byte(__fdiv_rn(v, H));
    if (blue) {
      b = blue[n];
    } else {
      const float p2 = pct[0], p98 = pct[1];
      const float inv = __fdiv_rn(1.0f, z + 1e-10f);
      b = unit_byte(__fdiv_rn(inv - p2, (p98 - p2) + 1e-10f));
    }
  }
  store_rows(out, first, N, r, g, b);
}

__global__ __launch_bounds__(COL_THREADS) void colors_depth_kernel(const float* __restrict__ pts, const unsigned char* __restrict__ vis, int64_t N,
                                                                   int64_t total, const double* __restrict__ pct,
                                                                   const unsigned char* __restrict__ lut, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t first = (int64_t)blockIdx.x * COL_THREADS, i = first + threadIdx.x;
  unsigned char r = 0, g = 0, b = 0;
  if (i < total && (!vis || vis[i] != 0)) {
    const int64_t t = i / N;
    const double p2 = pct[2 * t], p98 = pct[2 * t + 1];
    int k = 0;                                       // p98 <= p2 (or a NaN percentile): the normalised depth is 0
    bool bad = false;
    if (p98 > p2) {
      const double d = (double)pts[i * 3 + 2];
      const double c = d != d ? d : (d < p2 ? p2 : d > p98 ? p98 : d);
      const double xa = (c - p2) / (p98 - p2) * 256.0;
      bad = xa != xa;
      k = xa < 0.0 ? 256 : xa == 256.0 ? 255 : xa > 256.0 ? 257 : (int)xa;          // under, the closed upper end, over
    }
    if (!bad) {
      r = lut[3 * k];
      g = lut[3 * k + 1];
      b = lut[3 * k + 2];
    }
  }
  store_rows(out, first, total, r, g, b);
}

__global__ __launch_bounds__(COL_THREADS) void colors_cosine_kernel(const float* __restrict__ code, int64_t N, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t first = (int64_t)blockIdx.x * COL_THREADS, n = first + threadIdx.x;
  unsigned char c[3] = {0, 0, 0};
  if (n < N) {
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = unit_byte((code[n * 3 + j] + 1.0f) / 2.0f);     // / 2 is exact
  }
  store_rows(out, first, N, c[0], c[1], c[2]);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int64_t col_blocks(int64_t rows) { return (rows + COL_THREADS - 1) / COL_THREADS; }

}  // namespace

extern "C" int flexam_select_f32(const float* src, int stride, int comp, int transform, const unsigned char* mask, int S, int64_t seg_len,
                                 const int64_t* ranks, int K, float* values, int64_t* info, void* ws, int64_t ws_bytes, void* stream) {
  FX_REQUIRE(src && info && ws, FLEXAM_E_ARG, "select_f32: null pointer (src, info, ws)");
  FX_REQUIRE(K >= 0 && K <= SEL_KMAX, FLEXAM_E_SHAPE, "select_f32: K=%d ranks per segment (0 .. %d)", K, SEL_KMAX);
  FX_REQUIRE(K == 0 || (ranks && values), FLEXAM_E_ARG, "select_f32: K=%d ranks need ranks and values", K);
  FX_REQUIRE(aligned(src, 4) && aligned(values, 4) && aligned(ranks, 8) && aligned(info, 8) && aligned(ws, 4), FLEXAM_E_ARG,
             "select_f32: src, values and ws need 4-byte, ranks and info 8-byte alignment");
  FX_REQUIRE(S > 0 && S <= 65535 && seg_len > 0 && seg_len <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "select_f32: S=%d (1 .. 65535) seg_len=%lld (1 .. 2^31 - 1)", S,
             (long long)seg_len);
  FX_REQUIRE(stride >= 1 && stride <= 64 && comp >= 0 && comp < stride, FLEXAM_E_SHAPE, "select_f32: stride=%d (1 .. 64) comp=%d (0 .. stride - 1)", stride,
             comp);
  FX_REQUIRE(transform == 0 || transform == 1, FLEXAM_E_ARG, "select_f32: transform=%d (0: none, 1: 1 / (x + 1e-10))", transform);
  FX_REQUIRE(ws_bytes >= (int64_t)S * FLEXAM_SELECT_WS_SEGMENT_BYTES, FLEXAM_E_ARG, "select_f32: workspace of %lld bytes, %lld needed (%d per segment)",
             (long long)ws_bytes, (long long)S * FLEXAM_SELECT_WS_SEGMENT_BYTES, FLEXAM_SELECT_WS_SEGMENT_BYTES);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, (size_t)S * FLEXAM_SELECT_WS_SEGMENT_BYTES, st) != hipSuccess ||
      hipMemsetAsync(info, 0, (size_t)S * 4 * sizeof(int64_t), st) != hipSuccess)
    return flexam_fail(FLEXAM_E_LAUNCH, "select_f32: clearing the workspace failed");
  const int64_t tiles = (seg_len + SEL_TILE - 1) / SEL_TILE;
  const int64_t per_seg = SEL_GRID / S > 0 ? SEL_GRID / S : 1;
  const dim3 grid((unsigned)(tiles < per_seg ? tiles : per_seg), (unsigned)S);
  unsigned* w = reinterpret_cast<unsigned*>(ws);
  unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (stride == 3)
      hipLaunchKernelGGL(select_hist_kernel<true>, grid, dim3(SEL_THREADS), 0, st, src, stride, comp, transform, mask, seg_len, K, shift, w, inf);
    else
      hipLaunchKernelGGL(select_hist_kernel<false>, grid, dim3(SEL_THREADS), 0, st, src, stride, comp, transform, mask, seg_len, K, shift, w, inf);
    hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)S), dim3(SEL_THREADS), 0, st, w, ranks, K, shift, values, inf);
    if (K == 0) break;                               // counting only: the first pass holds the counts and the flags
  }
  return flexam_check_launch("flexam_select_f32");
}

extern "C" int flexam_select_lerp(const float* values, const double* gamma, const int64_t* info, int S, int Q, int f32_form, void* out, void* stream) {
  FX_REQUIRE(values && gamma && info && out, FLEXAM_E_ARG, "select_lerp: null pointer");
  FX_REQUIRE(aligned(values, 4) && aligned(gamma, 8) && aligned(info, 8) && aligned(out, f32_form ? 4 : 8), FLEXAM_E_ARG, "select_lerp: misaligned pointer");
  FX_REQUIRE(S > 0 && S <= 65535 && Q > 0 && 2 * Q <= SEL_KMAX, FLEXAM_E_SHAPE, "select_lerp: S=%d (1 .. 65535) Q=%d (1 .. %d)", S, Q, SEL_KMAX / 2);
  const int total = S * Q;
  hipLaunchKernelGGL(select_lerp_kernel, dim3((unsigned)col_blocks(total)), dim3(COL_THREADS), 0, (hipStream_t)stream, values, gamma,
                     reinterpret_cast<const unsigned long long*>(info), total, Q, f32_form, out);
  return flexam_check_launch("flexam_select_lerp");
}

extern "C" int flexam_raster_colors_tracking(const float* points, int64_t N, int H, int W, const float* pct, const unsigned char* blue,
                                             unsigned char* colors, void* stream) {
  FX_REQUIRE(points && colors && (pct || blue), FLEXAM_E_ARG, "raster_colors_tracking: null pointer (points, colors, and pct or blue)");
  FX_REQUIRE(aligned(points, 4) && aligned(pct, 4) && aligned(colors, 4), FLEXAM_E_ARG, "raster_colors_tracking: points, pct and colors need 4-byte alignment");
  FX_REQUIRE(N > 0 && N <= 0x7FFFFFFF && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), FLEXAM_E_SHAPE,
             "raster_colors_tracking: N=%lld H=%d W=%d (frame sides must be exact in float32)", (long long)N, H, W);
  hipLaunchKernelGGL(colors_tracking_kernel, dim3((unsigned)col_blocks(N)), dim3(COL_THREADS), 0, (hipStream_t)stream, points, N, (float)W, (float)H, pct,
                     blue, colors);
  return flexam_check_launch("flexam_raster_colors_tracking");
}

extern "C" int flexam_raster_colors_depth(const float* points, const unsigned char* visible, int T, int64_t N, const double* pct,
                                          const unsigned char* lut, unsigned char* colors, void* stream) {
  FX_REQUIRE(points && pct && lut && colors, FLEXAM_E_ARG, "raster_colors_depth: null pointer");
  FX_REQUIRE(aligned(points, 4) && aligned(pct, 8) && aligned(colors, 4), FLEXAM_E_ARG, "raster_colors_depth: points and colors need 4-byte, pct 8-byte alignment");
  FX_REQUIRE(T > 0 && N > 0 && N <= 0x7FFFFFFF && col_blocks((int64_t)T * N) <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "raster_colors_depth: T=%d N=%lld", T,
             (long long)N);
  const int64_t total = (int64_t)T * N;
  hipLaunchKernelGGL(colors_depth_kernel, dim3((unsigned)col_blocks(total)), dim3(COL_THREADS), 0, (hipStream_t)stream, points, visible, N, total, pct, lut,
                     colors);
  return flexam_check_launch("flexam_raster_colors_depth");
}

extern "C" int flexam_raster_colors_cosine(const float* code, int64_t N, unsigned char* colors, void* stream) {
  FX_REQUIRE(code && colors, FLEXAM_E_ARG, "raster_colors_cosine: null pointer");
  FX_REQUIRE(aligned(code, 4) && aligned(colors, 4), FLEXAM_E_ARG, "raster_colors_cosine: code and colors need 4-byte alignment");
  FX_REQUIRE(N > 0 && N <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "raster_colors_cosine: N=%lld", (long long)N);
  hipLaunchKernelGGL(colors_cosine_kernel, dim3((unsigned)col_blocks(N)), dim3(COL_THREADS), 0, (hipStream_t)stream, code, N, colors);
  return flexam_check_launch("flexam_raster_colors_cosine");
}
