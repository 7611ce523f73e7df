// flexam_amd/csrc/motion.hip -- edit tracks: camera and object motion on the 3-D tracks (flexam_amd/motion.py).
//
// The reference's CameraMotionGenerator / ObjectMotionGenerator / convert_moge_to_delta_format (pipelines.py:195-850, 852-1038,
// 1255-1291; demo.py:216-358) move every tracked point of every frame through one 3x4 affine map (object motion, selected points
// only), one 3x4 camera pose, one 3x3 intrinsic matrix and a division, as boolean-index gathers, bmm's and a host round trip.  The
// O(T) matrices stay on the host (motion.py); everything per point is here:
//   flexam_motion_select_map / _pixels   which points an object mask selects, and the sums of their coordinates and their count in
//                                        double in a fixed order (per-workgroup partials, combined by index): the centre is reproducible
//   flexam_motion_compact                a [N] byte mask -> the ascending list of its set positions and their number (two-level scan)
//   flexam_motion_transform_f32          per (frame, point): [object affine if flagged] -> [pose, intrinsics, division, depth] -> scale,
//                                        gathered through an index list, from [T, N, 3] or from ONE [N, 3] map shared by all frames
//   flexam_motion_unproject_f64 / _project_f64   the VGGT route's pixel <-> world maps in double
// Arithmetic is spelled out (fmaf chains in the order k = 0..3, contraction off), so a fused call and the same stages run one after
// the other give the same bits.  A workgroup of the float32 transform owns 256 consecutive output points and walks a strip of frames:
// the 12-byte points go through LDS so that global loads and stores are consecutive dwords, and the per-frame matrices are
// wave-uniform reads.
#include "common.h"
#include "flexam_hip.h"

namespace {

constexpr int MO_THREADS = 256;
constexpr int MO_CHUNK = FLEXAM_MOTION_CHUNK;     // points per workgroup of the select and compact passes
constexpr int MO_PER_THREAD = MO_CHUNK / MO_THREADS;
constexpr int MO_STRIP = 8;                       // frames a workgroup walks when all frames share one source map

__device__ __forceinline__ double wave_sum_f64(double v) {       // butterfly: every lane ends with the same bits, whatever the lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// torch's `x.round().long()` followed by clamp_(0, n - 1): halves to even; NaN and everything below 0 -> 0
__device__ __forceinline__ int pixel_index(float v, int n) {
  const float r = rintf(v);
  if (!(r >= 0.f)) return 0;
  return r >= (float)(n - 1) ? n - 1 : (int)r;
}

template <bool kPixels>
__global__ __launch_bounds__(MO_THREADS) void motion_select_kernel(const float* __restrict__ pts, int64_t N,
                                                                   const unsigned char* __restrict__ mask, int Hm, int Wm,
                                                                   unsigned char* __restrict__ flags, double* __restrict__ partial) {
  __shared__ double red[MO_THREADS / 64][4];
  const int64_t base = (int64_t)blockIdx.x * MO_CHUNK;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < MO_PER_THREAD; ++j) {
    const int64_t n = base + j * MO_THREADS + threadIdx.x;
    if (n >= N) continue;
    const float x = pts[n * 3], y = pts[n * 3 + 1], z = pts[n * 3 + 2];
    bool sel;
    if (kPixels) sel = mask[(int64_t)pixel_index(y, Hm) * Wm + pixel_index(x, Wm)] != 0;
    else sel = mask[n] != 0 && !(x != x || y != y || z != z);
    flags[n] = sel ? 1 : 0;
    if (sel) {
      s[0] += (double)x;
      s[1] += (double)y;
      s[2] += (double)z;
      s[3] += 1.0;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = wave_sum_f64(s[k]);
    if (lane == 0) red[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = red[0][threadIdx.x];
    for (int w = 1; w < MO_THREADS / 64; ++w) t += red[w][threadIdx.x];
    partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// sums[k] = partial[0][k] + partial[1][k] + ... : thread t takes blocks t, t + 256, ... in order, then the same fixed tree
__global__ __launch_bounds__(MO_THREADS) void motion_select_combine_kernel(const double* __restrict__ partial, int64_t nblk,
                                                                           double* __restrict__ sums) {
  __shared__ double red[MO_THREADS / 64][4];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nblk; b += MO_THREADS)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += partial[b * 4 + k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = wave_sum_f64(s[k]);
    if (lane == 0) red[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = red[0][threadIdx.x];
    for (int w = 1; w < MO_THREADS / 64; ++w) t += red[w][threadIdx.x];
    sums[threadIdx.x] = t;
  }
}

// exclusive scan of one int per thread over the workgroup; returns the thread's offset, `total` = the workgroup's sum
__device__ __forceinline__ int block_exclusive_scan(int own, int* part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  __syncthreads();                                 // `part` may still be read from the previous use
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int off = incl - own;
  total = 0;
#pragma unroll
  for (int w = 0; w < MO_THREADS / 64; ++w) {
    if (w < wave) off += part[w];
    total += part[w];
  }
  return off;
}

// thread t of workgroup b owns positions b * CHUNK + t * 4 .. + 3: ascending positions <-> ascending (workgroup, thread, j)
__device__ __forceinline__ int compact_own(const unsigned char* __restrict__ mask, int64_t N, int64_t first, bool (&set)[MO_PER_THREAD]) {
  int own = 0;
#pragma unroll
  for (int j = 0; j < MO_PER_THREAD; ++j) {
    set[j] = first + j < N && mask[first + j] != 0;
    own += set[j] ? 1 : 0;
  }
  return own;
}

__global__ __launch_bounds__(MO_THREADS) void motion_compact_count_kernel(const unsigned char* __restrict__ mask, int64_t N,
                                                                          int* __restrict__ block_count) {
  __shared__ int part[MO_THREADS / 64];
  bool set[MO_PER_THREAD];
  int total;
  block_exclusive_scan(compact_own(mask, N, (int64_t)blockIdx.x * MO_CHUNK + threadIdx.x * MO_PER_THREAD, set), part, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// in place: block_count -> exclusive offsets; *count = the total.  One workgroup walks the list 256 entries at a time.
__global__ __launch_bounds__(MO_THREADS) void motion_compact_scan_kernel(int* __restrict__ block_count, int64_t nblk, int* __restrict__ count) {
  __shared__ int part[MO_THREADS / 64];
  int carry = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += MO_THREADS) {
    const int64_t b = b0 + threadIdx.x;
    const int own = b < nblk ? block_count[b] : 0;
    int total;
    const int off = block_exclusive_scan(own, part, total);
    if (b < nblk) block_count[b] = carry + off;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(MO_THREADS) void motion_compact_write_kernel(const unsigned char* __restrict__ mask, int64_t N,
                                                                          const int* __restrict__ block_offset, int* __restrict__ index) {
  __shared__ int part[MO_THREADS / 64];
  bool set[MO_PER_THREAD];
  const int64_t first = (int64_t)blockIdx.x * MO_CHUNK + threadIdx.x * MO_PER_THREAD;
  int total;
  int at = block_offset[blockIdx.x] + block_exclusive_scan(compact_own(mask, N, first, set), part, total);   // < count <= N: inside `index`
#pragma unroll
  for (int j = 0; j < MO_PER_THREAD; ++j)
    if (set[j]) index[at++] = (int)(first + j);
}

// r = A[0] x + A[1] y + A[2] z + A[3], summed in that order
__device__ __forceinline__ float affine_row(const float* __restrict__ A, float x, float y, float z) {
  return __builtin_fmaf(A[2], z, __builtin_fmaf(A[1], y, A[0] * x)) + A[3];
}
__device__ __forceinline__ float linear_row(const float* __restrict__ A, float x, float y, float z) {
  return __builtin_fmaf(A[2], z, __builtin_fmaf(A[1], y, A[0] * x));
}

__global__ __launch_bounds__(MO_THREADS) void motion_transform_f32_kernel(const float* __restrict__ src, int64_t src_frame_stride, int T,
                                                                          const unsigned char* __restrict__ flags,
                                                                          const float* __restrict__ motion, const float* __restrict__ pose,
                                                                          const float* __restrict__ intr, float scale_u, float scale_v,
                                                                          const int* __restrict__ index, int64_t M, float* __restrict__ out,
                                                                          int strip) {
#pragma clang fp contract(off)
  __shared__ float stage[MO_THREADS * 3];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * MO_THREADS;
  const bool live = p0 + tid < M;
  const int64_t n = live ? (index ? (int64_t)index[p0 + tid] : p0 + tid) : 0;
  const bool moved = live && motion && (!flags || flags[n] != 0);
  const int words = (int)(M - p0 < MO_THREADS ? M - p0 : MO_THREADS) * 3;
  const int t0 = blockIdx.y * strip, t1 = t0 + strip < T ? t0 + strip : T;
  float x0 = 0.f, y0 = 0.f, z0 = 0.f;
  if (src_frame_stride == 0 && live) {
    x0 = src[n * 3];
    y0 = src[n * 3 + 1];
    z0 = src[n * 3 + 2];
  }
  for (int t = t0; t < t1; ++t) {
    float x = x0, y = y0, z = z0;
    if (src_frame_stride != 0) {
      const float* s = src + (int64_t)t * src_frame_stride;
      if (index) {                                  // ascending positions: neighbouring lanes read neighbouring points, with gaps
        if (live) {
          x = s[n * 3];
          y = s[n * 3 + 1];
          z = s[n * 3 + 2];
        }
      } else {                                      // consecutive dwords in, own point out of LDS (stride 3: no bank conflict)
        for (int k = tid; k < words; k += MO_THREADS) stage[k] = s[p0 * 3 + k];
        __syncthreads();
        x = stage[tid * 3];
        y = stage[tid * 3 + 1];
        z = stage[tid * 3 + 2];
        __syncthreads();
      }
    }
    if (moved) {
      const float* A = motion + (int64_t)t * 12;
      const float a = affine_row(A, x, y, z), b = affine_row(A + 4, x, y, z), c = affine_row(A + 8, x, y, z);
      x = a;
      y = b;
      z = c;
    }
    if (pose) {
      const float* P = pose + (int64_t)t * 12;
      const float cx = affine_row(P, x, y, z), cy = affine_row(P + 4, x, y, z), cz = affine_row(P + 8, x, y, z);
      const float h0 = linear_row(intr, cx, cy, cz), h1 = linear_row(intr + 3, cx, cy, cz), h2 = linear_row(intr + 6, cx, cy, cz);
      x = h0 / h2;
      y = h1 / h2;
      z = cz;
    }
    x = x * scale_u;
    y = y * scale_v;
    stage[tid * 3] = x;
    stage[tid * 3 + 1] = y;
    stage[tid * 3 + 2] = z;
    __syncthreads();
    float* o = out + ((int64_t)t * M + p0) * 3;
    for (int k = tid; k < words; k += MO_THREADS) o[k] = stage[k];
    __syncthreads();
  }
}

template <typename TIn>
__device__ __forceinline__ void load_point_f64(const void* p, int64_t i, double& x, double& y, double& z) {
  const TIn* q = reinterpret_cast<const TIn*>(p) + i * 3;
  x = (double)q[0];
  y = (double)q[1];
  z = (double)q[2];
}

__device__ __forceinline__ double linear_row_f64(const double* __restrict__ A, double x, double y, double z) {
  return __builtin_fma(A[2], z, __builtin_fma(A[1], y, A[0] * x));
}

// s2w_vggt: world = Rinv ((Kinv (u, v, 1)) z - t) where z > 0, else (0, 0, 0)
template <typename TIo>
__global__ __launch_bounds__(MO_THREADS) void motion_unproject_f64_kernel(const void* __restrict__ pts, int64_t N, const double* __restrict__ kinv,
                                                                          const double* __restrict__ rinv, const double* __restrict__ tvec,
                                                                          void* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (n >= N) return;
  const int t = blockIdx.y;
  const int64_t i = (int64_t)t * N + n;
  double u, v, z;
  load_point_f64<TIo>(pts, i, u, v, z);
  const double *K = kinv + (int64_t)t * 9, *R = rinv + (int64_t)t * 9, *tv = tvec + (int64_t)t * 3;
  const double d0 = (__builtin_fma(K[1], v, K[0] * u) + K[2]) * z - tv[0];
  const double d1 = (__builtin_fma(K[4], v, K[3] * u) + K[5]) * z - tv[1];
  const double d2 = (__builtin_fma(K[7], v, K[6] * u) + K[8]) * z - tv[2];
  const bool valid = z > 0.0;
  TIo* o = reinterpret_cast<TIo*>(out) + i * 3;
  o[0] = valid ? (TIo)linear_row_f64(R, d0, d1, d2) : (TIo)0;
  o[1] = valid ? (TIo)linear_row_f64(R + 3, d0, d1, d2) : (TIo)0;
  o[2] = valid ? (TIo)linear_row_f64(R + 6, d0, d1, d2) : (TIo)0;
}

// w2s_vggt: c = P (x, y, z, 1); (u, v) = K (c / (c_z + 1e-10)); (u, v, c_z) where c_z > 0, else (0, 0, 0)
template <typename TIn>
__global__ __launch_bounds__(MO_THREADS) void motion_project_f64_kernel(const void* __restrict__ pts, int64_t N, const double* __restrict__ pose,
                                                                        const double* __restrict__ intr, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (n >= N) return;
  const int t = blockIdx.y;
  const int64_t i = (int64_t)t * N + n;
  double x, y, z;
  load_point_f64<TIn>(pts, i, x, y, z);
  const double *P = pose + (int64_t)t * 12, *K = intr + (int64_t)t * 9;
  const double c0 = linear_row_f64(P, x, y, z) + P[3], c1 = linear_row_f64(P + 4, x, y, z) + P[7], c2 = linear_row_f64(P + 8, x, y, z) + P[11];
  const double den = c2 + 1e-10;
  const double n0 = c0 / den, n1 = c1 / den, n2 = c2 / den;
  const bool valid = c2 > 0.0;
  double* o = out + i * 3;
  o[0] = valid ? linear_row_f64(K, n0, n1, n2) : 0.0;
  o[1] = valid ? linear_row_f64(K + 3, n0, n1, n2) : 0.0;
  o[2] = valid ? c2 : 0.0;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int64_t chunks(int64_t N) { return (N + MO_CHUNK - 1) / MO_CHUNK; }

int select_launch(bool pixels, const float* points, int64_t N, const unsigned char* mask, int Hm, int Wm, unsigned char* flags, double* ws,
                  int64_t ws_bytes, double* sums, void* stream, const char* who) {
  FX_REQUIRE(points && mask && flags && ws && sums, FLEXAM_E_ARG, "%s: null pointer", who);
  FX_REQUIRE(aligned(points, 4) && aligned(ws, 8) && aligned(sums, 8), FLEXAM_E_ARG, "%s: points need 4-byte, ws and sums 8-byte alignment", who);
  FX_REQUIRE(N > 0 && N <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "%s: N=%lld (1 .. 2^31 - 1)", who, (long long)N);
  FX_REQUIRE(!pixels || (Hm > 0 && Wm > 0), FLEXAM_E_SHAPE, "%s: mask %d x %d", who, Hm, Wm);
  const int64_t nblk = chunks(N);
  FX_REQUIRE(ws_bytes >= nblk * 32, FLEXAM_E_ARG, "%s: workspace of %lld bytes, %lld needed (32 per %d points)", who, (long long)ws_bytes,
             (long long)(nblk * 32), MO_CHUNK);
  if (pixels)
    hipLaunchKernelGGL(motion_select_kernel<true>, dim3((unsigned)nblk), dim3(MO_THREADS), 0, (hipStream_t)stream, points, N, mask, Hm, Wm, flags, ws);
  else
    hipLaunchKernelGGL(motion_select_kernel<false>, dim3((unsigned)nblk), dim3(MO_THREADS), 0, (hipStream_t)stream, points, N, mask, 0, 0, flags, ws);
  hipLaunchKernelGGL(motion_select_combine_kernel, dim3(1), dim3(MO_THREADS), 0, (hipStream_t)stream, ws, nblk, sums);
  return flexam_check_launch(who);
}

}  // namespace

extern "C" int flexam_motion_select_map(const float* points, int64_t N, const unsigned char* mask, unsigned char* flags, double* ws,
                                        int64_t ws_bytes, double* sums, void* stream) {
  return select_launch(false, points, N, mask, 0, 0, flags, ws, ws_bytes, sums, stream, "flexam_motion_select_map");
}

extern "C" int flexam_motion_select_pixels(const float* points, int64_t N, const unsigned char* mask, int mask_h, int mask_w,
                                           unsigned char* flags, double* ws, int64_t ws_bytes, double* sums, void* stream) {
  return select_launch(true, points, N, mask, mask_h, mask_w, flags, ws, ws_bytes, sums, stream, "flexam_motion_select_pixels");
}

extern "C" int flexam_motion_compact(const unsigned char* mask, int64_t N, int* index, int* count, int* ws, int64_t ws_bytes, void* stream) {
  FX_REQUIRE(mask && index && count && ws, FLEXAM_E_ARG, "motion_compact: null pointer");
  FX_REQUIRE(aligned(index, 4) && aligned(count, 4) && aligned(ws, 4), FLEXAM_E_ARG, "motion_compact: index, count and ws need 4-byte alignment");
  FX_REQUIRE(N > 0 && N <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "motion_compact: N=%lld (1 .. 2^31 - 1)", (long long)N);
  const int64_t nblk = chunks(N);
  FX_REQUIRE(ws_bytes >= nblk * 4, FLEXAM_E_ARG, "motion_compact: workspace of %lld bytes, %lld needed (4 per %d positions)", (long long)ws_bytes,
             (long long)(nblk * 4), MO_CHUNK);
  hipLaunchKernelGGL(motion_compact_count_kernel, dim3((unsigned)nblk), dim3(MO_THREADS), 0, (hipStream_t)stream, mask, N, ws);
  hipLaunchKernelGGL(motion_compact_scan_kernel, dim3(1), dim3(MO_THREADS), 0, (hipStream_t)stream, ws, nblk, count);
  hipLaunchKernelGGL(motion_compact_write_kernel, dim3((unsigned)nblk), dim3(MO_THREADS), 0, (hipStream_t)stream, mask, N, ws, index);
  return flexam_check_launch("flexam_motion_compact");
}

extern "C" int flexam_motion_transform_f32(const float* src, int64_t src_frame_stride, int T, int64_t N, const unsigned char* flags,
                                           const float* motion, const float* pose, const float* intr, float scale_u, float scale_v,
                                           const int* index, int64_t M, float* out, void* stream) {
  FX_REQUIRE(src && out, FLEXAM_E_ARG, "motion_transform_f32: null pointer");
  FX_REQUIRE((pose == nullptr) == (intr == nullptr), FLEXAM_E_ARG, "motion_transform_f32: pose and intr come together");
  FX_REQUIRE(!flags || motion, FLEXAM_E_ARG, "motion_transform_f32: flags without motion matrices");
  FX_REQUIRE(aligned(src, 4) && aligned(out, 4) && aligned(motion, 4) && aligned(pose, 4) && aligned(intr, 4) && aligned(index, 4), FLEXAM_E_ARG,
             "motion_transform_f32: float and int pointers need 4-byte alignment");
  FX_REQUIRE(T > 0 && N > 0 && M > 0, FLEXAM_E_SHAPE, "motion_transform_f32: T=%d N=%lld M=%lld", T, (long long)N, (long long)M);
  FX_REQUIRE(index ? M <= N : M == N, FLEXAM_E_SHAPE, "motion_transform_f32: M=%lld output points from N=%lld (%s)", (long long)M, (long long)N,
             index ? "M <= N with an index list" : "M == N without one");
  FX_REQUIRE(src_frame_stride == 0 || src_frame_stride >= N * 3, FLEXAM_E_SHAPE, "motion_transform_f32: frame stride %lld (0 or >= 3 N)",
             (long long)src_frame_stride);
  const int strip = src_frame_stride == 0 ? MO_STRIP : 1;
  const int64_t gx = (M + MO_THREADS - 1) / MO_THREADS, gy = (T + strip - 1) / strip;
  FX_REQUIRE(gx <= 0x7FFFFFFF && gy <= 65535, FLEXAM_E_SHAPE, "motion_transform_f32: grid %lld x %lld", (long long)gx, (long long)gy);
  hipLaunchKernelGGL(motion_transform_f32_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(MO_THREADS), 0, (hipStream_t)stream, src, src_frame_stride,
                     T, flags, motion, pose, intr, scale_u, scale_v, index, M, out, strip);
  return flexam_check_launch("flexam_motion_transform_f32");
}

extern "C" int flexam_motion_unproject_f64(const void* points, int points_f32, int T, int64_t N, const double* kinv, const double* rinv,
                                           const double* tvec, void* out, void* stream) {
  FX_REQUIRE(points && kinv && rinv && tvec && out, FLEXAM_E_ARG, "motion_unproject_f64: null pointer");
  const uintptr_t a = points_f32 ? 4 : 8;
  FX_REQUIRE(aligned(points, a) && aligned(out, a) && aligned(kinv, 8) && aligned(rinv, 8) && aligned(tvec, 8), FLEXAM_E_ARG,
             "motion_unproject_f64: misaligned pointer");
  FX_REQUIRE(T > 0 && T <= 65535 && N > 0 && N <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "motion_unproject_f64: T=%d N=%lld", T, (long long)N);
  const dim3 grid((unsigned)((N + MO_THREADS - 1) / MO_THREADS), (unsigned)T);
  if (points_f32)
    hipLaunchKernelGGL(motion_unproject_f64_kernel<float>, grid, dim3(MO_THREADS), 0, (hipStream_t)stream, points, N, kinv, rinv, tvec, out);
  else
    hipLaunchKernelGGL(motion_unproject_f64_kernel<double>, grid, dim3(MO_THREADS), 0, (hipStream_t)stream, points, N, kinv, rinv, tvec, out);
  return flexam_check_launch("flexam_motion_unproject_f64");
}

extern "C" int flexam_motion_project_f64(const void* points, int points_f32, int T, int64_t N, const double* pose, const double* intr,
                                         double* out, void* stream) {
  FX_REQUIRE(points && pose && intr && out, FLEXAM_E_ARG, "motion_project_f64: null pointer");
  FX_REQUIRE(aligned(points, points_f32 ? 4 : 8) && aligned(out, 8) && aligned(pose, 8) && aligned(intr, 8), FLEXAM_E_ARG,
             "motion_project_f64: misaligned pointer");
  FX_REQUIRE(T > 0 && T <= 65535 && N > 0 && N <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "motion_project_f64: T=%d N=%lld", T, (long long)N);
  const dim3 grid((unsigned)((N + MO_THREADS - 1) / MO_THREADS), (unsigned)T);
  if (points_f32)
    hipLaunchKernelGGL(motion_project_f64_kernel<float>, grid, dim3(MO_THREADS), 0, (hipStream_t)stream, points, N, pose, intr, out);
  else
    hipLaunchKernelGGL(motion_project_f64_kernel<double>, grid, dim3(MO_THREADS), 0, (hipStream_t)stream, points, N, pose, intr, out);
  return flexam_check_launch("flexam_motion_project_f64");
}
