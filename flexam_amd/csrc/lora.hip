// flexam_amd/csrc/lora.hip -- LoRA merge into stored weights (flexam_amd/lora_utils.py).
//
// The reference merges on the host or in torch: `weight.data += multiplier * alpha * torch.mm(up, down)` per layer
// (FlexAM/utils/lora_utils.py:480-485), which rounds the product, the scaled product and the sum to the working dtype.  Here:
//   flexam_lora_merge   W[n][k] <- round_to_W_dtype(float(W[n][k]) + s * sum_{j < r} U[n][j] * D[j][k])
// with every product and sum in fp32: acc = fma(U[n][j], D[j][k], acc) from acc = 0, j ascending; then fma(s, acc, W) and ONE
// rounding to the storage type (round to nearest even; e4m3 through the conversion of dit_rows.h, after a clamp to +-448: a result
// beyond the largest e4m3 value saturates, it does not become NaN; NaN stays NaN).  Unmerge is the same call with -s.
//
// Plain fp32 VALU: the bf16 MFMA would round U and D, and gfx950's fp32 MFMA runs at the vector rate.  A workgroup owns a 64 x 64
// tile of W, a thread a 4 x 4 patch of it (four rows, four adjacent columns); the rank is walked in chunks of LORA_RC, the chunk's
// U columns and D rows staged in LDS as fp32 (bf16 factors are widened on the way in: exact).  A tile that lies wholly inside W,
// with W's base and row stride aligned to four elements, moves its patch rows as single 4-element loads and stores; every other
// tile (ragged edges, odd strides) takes the guarded path, element by element.
// Measured (tools/lora_bench.py, rank 64 over 300 linears at 5B width, profiles/lora_bench.json): 17.9 ms, 21 % of copy bandwidth;
// U and D are staged with element-wide loads.
#include "dit_rows.h"
#include "flexam_hip.h"

namespace {

constexpr int LORA_T = 64;        // tile edge (rows and columns of W per workgroup)
constexpr int LORA_RC = 32;       // rank chunk staged in LDS
constexpr unsigned LORA_GRID_Y_MAX = 65535;

struct E4M3 { unsigned char b; };

__device__ __forceinline__ float lora_widen(float v) { return v; }
__device__ __forceinline__ float lora_widen(bf16 v) { return bf2f(v); }
__device__ __forceinline__ float lora_widen(E4M3 v) { return __builtin_amdgcn_cvt_f32_fp8((int)v.b, 0); }

__device__ __forceinline__ float e4m3_sat(float x) { return x != x ? x : fminf(fmaxf(x, -448.f), 448.f); }

__device__ __forceinline__ void lora_load4(const float* p, float* v) {
  const f32x4 t = *(const f32x4*)p;
  v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
}
__device__ __forceinline__ void lora_load4(const bf16* p, float* v) {
  const bf16x4 t = *(const bf16x4*)p;
  v[0] = bf2f(t[0]), v[1] = bf2f(t[1]), v[2] = bf2f(t[2]), v[3] = bf2f(t[3]);
}
__device__ __forceinline__ void lora_load4(const E4M3* p, float* v) {
  const int t = *(const int*)p;
  v[0] = __builtin_amdgcn_cvt_f32_fp8(t, 0), v[1] = __builtin_amdgcn_cvt_f32_fp8(t, 1);
  v[2] = __builtin_amdgcn_cvt_f32_fp8(t, 2), v[3] = __builtin_amdgcn_cvt_f32_fp8(t, 3);
}

__device__ __forceinline__ void lora_store4(float* p, const float* v) { *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void lora_store4(bf16* p, const float* v) {
  *(bf16x4*)p = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
}
__device__ __forceinline__ void lora_store4(E4M3* p, const float* v) {
  *(unsigned*)p = e4m3_pack4((f32x4){e4m3_sat(v[0]), e4m3_sat(v[1]), e4m3_sat(v[2]), e4m3_sat(v[3])}, 1.0f);
}
__device__ __forceinline__ void lora_store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void lora_store1(bf16* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void lora_store1(E4M3* p, float v) {
  p->b = (unsigned char)(e4m3_pack4((f32x4){e4m3_sat(v), 0.f, 0.f, 0.f}, 1.0f) & 0xFFu);
}

// grid: x = column tiles, y = row tiles (grid-stride: N / 64 may exceed the grid's y limit)
template <typename WT, typename FT>
__global__ __launch_bounds__(256) void lora_merge_kernel(WT* __restrict__ W, int64_t ldw, const FT* __restrict__ U, int64_t ldu,
                                                         const FT* __restrict__ D, int64_t ldd, int64_t N, int64_t K, int r, float s,
                                                         int aligned) {
  __shared__ __attribute__((aligned(16))) float Us[LORA_RC][LORA_T + 4];   // [j][row of the tile]; + 4: the transposing store below spreads over the banks
  __shared__ __attribute__((aligned(16))) float Ds[LORA_RC][LORA_T];       // [j][column of the tile]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t k0 = (int64_t)blockIdx.x * LORA_T;
  const int64_t row_tiles = (N + LORA_T - 1) / LORA_T;
  for (int64_t rt = blockIdx.y; rt < row_tiles; rt += gridDim.y) {
    const int64_t n0 = rt * LORA_T;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
    for (int j0 = 0; j0 < r; j0 += LORA_RC) {
      const int nj = min(LORA_RC, r - j0);
      __syncthreads();                       // the previous chunk (or row tile) has been read
      // U[n0 + row][j0 + j] -> Us[j][row]: adjacent threads take adjacent j of one row (the contiguous direction of U)
      for (int e = tid; e < LORA_T * LORA_RC; e += 256) {
        const int row = e / LORA_RC, j = e % LORA_RC;
        Us[j][row] = (j < nj && n0 + row < N) ? lora_widen(U[(n0 + row) * ldu + j0 + j]) : 0.f;
      }
      // D[j0 + j][k0 + col] -> Ds[j][col]: adjacent threads take adjacent columns
      for (int e = tid; e < LORA_T * LORA_RC; e += 256) {
        const int j = e / LORA_T, col = e % LORA_T;
        Ds[j][col] = (j < nj && k0 + col < K) ? lora_widen(D[(int64_t)(j0 + j) * ldd + k0 + col]) : 0.f;
      }
      __syncthreads();
      for (int j = 0; j < nj; ++j) {         // j ascending: the order the header states
        const f32x4 u = *(const f32x4*)&Us[j][ty * 4], d = *(const f32x4*)&Ds[j][tx * 4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[i][c] = __builtin_fmaf(u[i], d[c], acc[i][c]);
      }
    }
    const int64_t col = k0 + tx * 4;
    if (aligned && n0 + LORA_T <= N && k0 + LORA_T <= K) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        WT* p = W + (n0 + ty * 4 + i) * ldw + col;
        float w[4];
        lora_load4(p, w);
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = __builtin_fmaf(s, acc[i][c], w[c]);
        lora_store4(p, w);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t n = n0 + ty * 4 + i;
        if (n >= N) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (col + c >= K) continue;
          WT* p = W + n * ldw + col + c;
          lora_store1(p, __builtin_fmaf(s, acc[i][c], lora_widen(*p)));
        }
      }
    }
  }
}

template <typename WT, typename FT>
void lora_launch(void* W, int64_t ldw, const void* U, int64_t ldu, const void* D, int64_t ldd, int64_t N, int64_t K, int r, float s,
                 hipStream_t st) {
  const int64_t row_tiles = (N + LORA_T - 1) / LORA_T, col_tiles = (K + LORA_T - 1) / LORA_T;
  const int64_t quad = 4 * (int64_t)sizeof(WT);          // bytes of a 4-element load
  const int aligned = ((uintptr_t)W % quad == 0) && (ldw % 4 == 0);
  const dim3 grid((unsigned)col_tiles, (unsigned)(row_tiles < LORA_GRID_Y_MAX ? row_tiles : LORA_GRID_Y_MAX));
  hipLaunchKernelGGL((lora_merge_kernel<WT, FT>), grid, dim3(256), 0, st, (WT*)W, ldw, (const FT*)U, ldu, (const FT*)D, ldd, N, K, r, s,
                     aligned);
}

template <typename FT>
int lora_dispatch(void* W, int w_dtype, int64_t ldw, const void* U, int64_t ldu, const void* D, int64_t ldd, int64_t N, int64_t K, int r,
                  float s, hipStream_t st) {
  switch (w_dtype) {
    case FLEXAM_LORA_BF16: lora_launch<bf16, FT>(W, ldw, U, ldu, D, ldd, N, K, r, s, st); break;
    case FLEXAM_LORA_F32: lora_launch<float, FT>(W, ldw, U, ldu, D, ldd, N, K, r, s, st); break;
    default: lora_launch<E4M3, FT>(W, ldw, U, ldu, D, ldd, N, K, r, s, st); break;
  }
  return flexam_check_launch("flexam_lora_merge");
}

}  // namespace

extern "C" int flexam_lora_merge(void* W, int w_dtype, int64_t ldw, int64_t N, int64_t K, const void* U, int u_dtype, int64_t ldu,
                                 const void* D, int d_dtype, int64_t ldd, int r, float s, void* stream) {
  FX_REQUIRE(W && U && D, FLEXAM_E_ARG, "lora_merge: null pointer");
  FX_REQUIRE(w_dtype == FLEXAM_LORA_BF16 || w_dtype == FLEXAM_LORA_F32 || w_dtype == FLEXAM_LORA_E4M3, FLEXAM_E_ARG,
             "lora_merge: unknown storage code %d", w_dtype);
  FX_REQUIRE((u_dtype == FLEXAM_LORA_BF16 || u_dtype == FLEXAM_LORA_F32) && u_dtype == d_dtype, FLEXAM_E_ARG,
             "lora_merge: factors must both be bf16 or both fp32, got codes %d and %d", u_dtype, d_dtype);
  FX_REQUIRE(N >= 1 && K >= 1 && r >= 1, FLEXAM_E_SHAPE, "lora_merge: N=%lld K=%lld r=%d", (long long)N, (long long)K, r);
  FX_REQUIRE(ldw >= K && ldu >= r && ldd >= K, FLEXAM_E_SHAPE, "lora_merge: row strides ldw=%lld (K=%lld) ldu=%lld (r=%d) ldd=%lld",
             (long long)ldw, (long long)K, (long long)ldu, r, (long long)ldd);
  FX_REQUIRE((K + LORA_T - 1) / LORA_T <= 0x7FFFFFFF, FLEXAM_E_SHAPE, "lora_merge: K=%lld", (long long)K);
  const hipStream_t st = (hipStream_t)stream;
  return u_dtype == FLEXAM_LORA_F32 ? lora_dispatch<float>(W, w_dtype, ldw, U, ldu, D, ldd, N, K, r, s, st)
                                    : lora_dispatch<bf16>(W, w_dtype, ldw, U, ldu, D, ldd, N, K, r, s, st);
}
