// flexam_amd/csrc/frames.hip -- pixels across the boundary: decoded frames in (resize + convert), the finished clip out (bytes).
//
// The reference resizes on the host, one frame at a time: torchvision `resize` of the float mask frames (bilinear, antialiased;
// FlexAM/utils/utils.py:473-517) and `F.interpolate(bilinear, align_corners=False)` of the ComfyUI streams followed by `.cpu().numpy()`,
// `* 255`, `/ 255` and a permute (utils.py:424-438); and it turns the decoded clip into bytes there too (utils.py:59-88).  Here:
//   flexam_frames_resize    out = sum_j wy[j] * sum_i wx[i] * src[t][c][y0 + j][x0 + i] in fp32, taps in ascending order, then
//                           * mul, / div, + add (each rounded on its own).  The tap tables -- first index, count, weights per output
//                           index and axis -- come from the host (flexam_amd/frames.py builds them in float32 the way torch's float
//                           path does); source (uint8 | float32) and destination are addressed by element strides, so one kernel
//                           reads [T, H, W, C] or [T, C, H, W] and writes [T, C, oh, ow] or [C, T, oh, ow].  One wave per output row
//                           segment: adjacent lanes take adjacent output columns, channels in register blocks of four, so the source
//                           rows of a tap window are read contiguously and the x weights once per block.  Loads are element-wide
//                           (byte loads for uint8: a [T, H, W, 3] row is 3 W bytes, aligned to nothing).
//   flexam_frames_to_bytes  [C, T, H, W] float32 | bf16 -> uint8 [T, H, W, C]: (x / 2 + 0.5 when signed) clamp to [0, 1], * 255,
//                           truncation; every step one float32 rounding (contraction off: a fused multiply-add changes bytes).
// Both are bandwidth kernels.
#include "common.h"
#include "flexam_hip.h"

namespace {

constexpr int RESIZE_ROWS = 4;            // waves (= output rows) per workgroup
constexpr int RESIZE_CB = 4;              // channels per register block
constexpr unsigned GRID_Y_MAX = 65535;

__device__ __forceinline__ float widen(unsigned char v) { return (float)v; }
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(bf16 v) { return bf2f(v); }

template <typename Src>
__global__ __launch_bounds__(64 * RESIZE_ROWS) void frames_resample_kernel(const Src* __restrict__ src, int64_t s_t, int64_t s_c,
                                                                          int64_t s_y, int64_t s_x, int T, int C, int H, int W,
                                                                          float* __restrict__ dst, int64_t d_t, int64_t d_c, int64_t d_y,
                                                                          int oh, int ow, const int* __restrict__ y_ix,
                                                                          const float* __restrict__ y_w, int ky, const int* __restrict__ x_ix,
                                                                          const float* __restrict__ x_w, int kx, float mul, float div,
                                                                          float add) {
#pragma clang fp contract(off)
  const int ox = blockIdx.x * 64 + threadIdx.x;
  if (ox >= ow) return;
  // every index is clamped into the source: a table that does not belong to these sizes gives wrong pixels, never a stray read
  const int x0 = min(max(x_ix[2 * ox], 0), W - 1), nx = min(min(x_ix[2 * ox + 1], kx), W - x0);
  const float* wx = x_w + (int64_t)ox * kx;
  const int64_t rows = (int64_t)T * oh;
  for (int64_t row = (int64_t)blockIdx.y * RESIZE_ROWS + threadIdx.y; row < rows; row += (int64_t)gridDim.y * RESIZE_ROWS) {
    const int t = (int)(row / oh), oy = (int)(row % oh);
    const int y0 = min(max(y_ix[2 * oy], 0), H - 1), ny = min(min(y_ix[2 * oy + 1], ky), H - y0);
    const float* wy = y_w + (int64_t)oy * ky;
    const Src* base = src + t * s_t + y0 * s_y + x0 * s_x;
    float* out = dst + t * d_t + oy * d_y + ox;
    for (int c0 = 0; c0 < C; c0 += RESIZE_CB) {
      const int nc = min(RESIZE_CB, C - c0);
      float acc[RESIZE_CB];
#pragma unroll
      for (int cc = 0; cc < RESIZE_CB; ++cc) acc[cc] = 0.f;
      for (int j = 0; j < ny; ++j) {
        const Src* p = base + j * s_y + c0 * s_c;
        float h[RESIZE_CB];
#pragma unroll
        for (int cc = 0; cc < RESIZE_CB; ++cc) h[cc] = 0.f;
        for (int i = 0; i < nx; ++i) {
          const float w = wx[i];
#pragma unroll
          for (int cc = 0; cc < RESIZE_CB; ++cc)
            if (cc < nc) h[cc] = __builtin_fmaf(w, widen(p[i * s_x + cc * s_c]), h[cc]);
        }
        const float v = wy[j];
#pragma unroll
        for (int cc = 0; cc < RESIZE_CB; ++cc) acc[cc] = __builtin_fmaf(v, h[cc], acc[cc]);
      }
#pragma unroll
      for (int cc = 0; cc < RESIZE_CB; ++cc)
        if (cc < nc) {
          float r = acc[cc];
          if (mul != 1.f) r = __fmul_rn(r, mul);
          if (div != 1.f) r = __fdiv_rn(r, div);        // IEEE division: `/ 255` is not `* (1 / 255)`
          if (add != 0.f) r = __fadd_rn(r, add);
          out[(c0 + cc) * d_c] = r;
        }
    }
  }
}

__device__ __forceinline__ unsigned to_byte(float x, int is_signed) {
#pragma clang fp contract(off)
  if (is_signed) x = __fadd_rn(__fmul_rn(x, 0.5f), 0.5f);       // x / 2 is x * 0.5 exactly; two roundings
  x = fminf(fmaxf(x, 0.f), 1.f);                                // NaN -> 0
  return (unsigned)(int)__fmul_rn(x, 255.f);
}

// one thread per pixel: C plane reads (coalesced per plane), C byte stores
template <typename Src>
__global__ __launch_bounds__(256) void frames_bytes_kernel(const Src* __restrict__ src, int C, int64_t n, int is_signed,
                                                           unsigned char* __restrict__ dst) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  for (int c = 0; c < C; ++c) dst[p * C + c] = (unsigned char)to_byte(widen(src[c * n + p]), is_signed);
}

// three channels, four pixels per thread: 12 bytes = three aligned dwords (n % 4 == 0 and dst 4-byte aligned: checked by the caller)
template <typename Src>
__global__ __launch_bounds__(256) void frames_bytes3_kernel(const Src* __restrict__ src, int64_t n, int is_signed,
                                                            unsigned* __restrict__ dst) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= n) return;
  unsigned b[12];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k * 3 + c] = to_byte(widen(src[c * n + q * 4 + k]), is_signed);
#pragma unroll
  for (int d = 0; d < 3; ++d) dst[q * 3 + d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
}

}  // namespace

extern "C" int flexam_frames_resize(const void* src, int src_is_u8, int64_t s_t, int64_t s_c, int64_t s_y, int64_t s_x, int T, int C, int H,
                                    int W, float* dst, int64_t d_t, int64_t d_c, int64_t d_y, int oh, int ow, const int* y_index,
                                    const float* y_weights, int ky, const int* x_index, const float* x_weights, int kx, float mul,
                                    float div, float add, void* stream) {
  FX_REQUIRE(src && dst && y_index && y_weights && x_index && x_weights, FLEXAM_E_ARG, "frames_resize: null pointer");
  FX_REQUIRE(T > 0 && C > 0 && H > 0 && W > 0 && oh > 0 && ow > 0, FLEXAM_E_SHAPE, "frames_resize: T=%d C=%d H=%d W=%d -> oh=%d ow=%d", T, C,
             H, W, oh, ow);
  FX_REQUIRE(ky >= 1 && ky <= FLEXAM_FRAMES_MAX_TAPS && kx >= 1 && kx <= FLEXAM_FRAMES_MAX_TAPS, FLEXAM_E_SHAPE,
             "frames_resize: tap table widths ky=%d kx=%d outside 1 .. %d", ky, kx, FLEXAM_FRAMES_MAX_TAPS);
  FX_REQUIRE(ky <= H && kx <= W, FLEXAM_E_SHAPE, "frames_resize: tap count over the axis: ky=%d H=%d kx=%d W=%d", ky, H, kx, W);
  FX_REQUIRE(s_t >= 0 && s_c >= 0 && s_y >= 0 && s_x >= 0 && d_t >= 0 && d_c >= 0 && d_y >= 0, FLEXAM_E_ARG, "frames_resize: negative stride");
  FX_REQUIRE(div != 0.f, FLEXAM_E_ARG, "frames_resize: div = 0");
  const int64_t groups = ((int64_t)T * oh + RESIZE_ROWS - 1) / RESIZE_ROWS;
  const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)(groups < GRID_Y_MAX ? groups : GRID_Y_MAX)), block(64, RESIZE_ROWS);
  if (src_is_u8)
    hipLaunchKernelGGL(frames_resample_kernel<unsigned char>, grid, block, 0, (hipStream_t)stream, (const unsigned char*)src, s_t, s_c, s_y,
                       s_x, T, C, H, W, dst, d_t, d_c, d_y, oh, ow, y_index, y_weights, ky, x_index, x_weights, kx, mul, div, add);
  else
    hipLaunchKernelGGL(frames_resample_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)src, s_t, s_c, s_y, s_x, T, C, H, W,
                       dst, d_t, d_c, d_y, oh, ow, y_index, y_weights, ky, x_index, x_weights, kx, mul, div, add);
  return flexam_check_launch("flexam_frames_resize");
}

extern "C" int flexam_frames_to_bytes(const void* src, int src_is_bf16, int C, int T, int H, int W, int is_signed, unsigned char* dst,
                                      void* stream) {
  FX_REQUIRE(src && dst, FLEXAM_E_ARG, "frames_to_bytes: null pointer");
  FX_REQUIRE(C > 0 && C <= 4 && T > 0 && H > 0 && W > 0, FLEXAM_E_SHAPE, "frames_to_bytes: C=%d (1 .. 4) T=%d H=%d W=%d", C, T, H, W);
  const int64_t n = (int64_t)T * H * W;
  FX_REQUIRE((n + 255) / 256 <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "frames_to_bytes: %lld pixels", (long long)n);
  const hipStream_t st = (hipStream_t)stream;
  if (C == 3 && n % 4 == 0 && ((uintptr_t)dst & 3) == 0) {
    const dim3 grid((unsigned)((n / 4 + 255) / 256));
    if (src_is_bf16)
      hipLaunchKernelGGL(frames_bytes3_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)src, n, is_signed, (unsigned*)dst);
    else
      hipLaunchKernelGGL(frames_bytes3_kernel<float>, grid, dim3(256), 0, st, (const float*)src, n, is_signed, (unsigned*)dst);
  } else {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (src_is_bf16)
      hipLaunchKernelGGL(frames_bytes_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)src, C, n, is_signed, dst);
    else
      hipLaunchKernelGGL(frames_bytes_kernel<float>, grid, dim3(256), 0, st, (const float*)src, C, n, is_signed, dst);
  }
  return flexam_check_launch("flexam_frames_to_bytes");
}
