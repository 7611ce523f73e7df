// flexam_amd/csrc/edit_mask.hip -- the foreground-edit mask refinement: binarised mask frames -> blurred, hull-filled, dilated
// masks (demo.py:33-96, generate_mask_fg_tracking_for_validation; copies in comfyui/wan2_2_fun_flexam/nodes.py:73-160).
//
// The reference runs, per frame and on the host, scipy.ndimage.gaussian_filter, cv2.findContours + convexHull + fillPoly and a
// cv2.dilate with a (2r+1)^2 elliptical element (r = 200 by default).  Here:
//   flexam_edit_mask_blur    two separable passes in fp64, in scipy's order of operations (correlate1d, symmetric kernel, mode
//                            'reflect'), a float32 result after each pass, then > 0.5.  One thread per pixel.
//   flexam_edit_mask_hull    one workgroup per frame: run-length encode the rows, label the 8-connected components of the runs
//                            (union-find with atomicMin: every component ends up rooted at its smallest run id, whatever the order
//                            of the unions), collect per component and row the leftmost and rightmost pixel, take the convex hull
//                            of those (its left and right chains, monotone chain in integers) and write, per component and row,
//                            the interval of pixels that lie in the closed hull or on the hull's edges drawn as 8-connected lines.
//                            Every run slot receives the interval of its (component, row).
//   flexam_edit_mask_dilate  one workgroup per output row: every interval of the rows y' within r grows by the element's half
//                            width at |y - y'| and is added to a difference array in LDS; a prefix sum gives the row.
// The union of the filled hulls of the 8-connected components equals the union of the filled hulls of the outer contours that
// cv2.RETR_EXTERNAL returns: a component inside another's hole lies inside that other's hull.  A component whose pixel centres
// are collinear contributes nothing (its CHAIN_APPROX_SIMPLE contour has fewer than 3 points, which the reference skips).
// Line pixels: along the major axis of an edge, the minor coordinate is floor(exact + 1/2) -- halves go to the larger coordinate.
// That tie rule is this library's choice; cv2's LINE_8 iterator may break ties the other way ("Foreground-edit masks").
#include "common.h"
#include "flexam_hip.h"

namespace {

constexpr int HULL_THREADS = 1024;
constexpr int HULL_MAX_H = 4096;          // rows per frame: one int per row in LDS
constexpr int EDIT_MAX_W = 16384;         // pixel columns fit 16 bits, and 2 * W * H products fit int32
constexpr unsigned IVL_EMPTY = 0x0000FFFFu;   // lo = 65535 > hi = 0

__device__ __forceinline__ int reflect_index(int i, int n) {     // scipy mode 'reflect': d c b a | a b c d | d c b a, repeated
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// out = sum_j w_j (x[i-j] + x[i+j]) in fp64 in scipy's order (NI_Correlate1D, symmetric branch), no fused multiply-adds
template <bool kRows>
__global__ __launch_bounds__(256) void edit_blur_kernel(const unsigned char* __restrict__ src, const float* __restrict__ tmp,
                                                        int64_t total, int H, int W, const double* __restrict__ w, int radius,
                                                        float* __restrict__ tmp_out, unsigned char* __restrict__ dst) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W);
  const int64_t fy = i / W;
  const int y = (int)(fy % H);
  if (kRows) {                              // axis 0: the input is the binarised frame (0 or 1)
    const unsigned char* col = src + (fy - y) * W + x;
    double acc = (double)col[(int64_t)y * W] * w[0];
    for (int j = radius; j >= 1; --j)
      acc += ((double)col[(int64_t)reflect_index(y - j, H) * W] + (double)col[(int64_t)reflect_index(y + j, H) * W]) * w[j];
    tmp_out[i] = (float)acc;
  } else {                                  // axis 1: the float32 result of axis 0, then the threshold
    const float* row = tmp + fy * W;
    double acc = (double)row[x] * w[0];
    for (int j = radius; j >= 1; --j) acc += ((double)row[reflect_index(x - j, W)] + (double)row[reflect_index(x + j, W)]) * w[j];
    dst[i] = (float)acc > 0.5f ? 1 : 0;
  }
}

__device__ __forceinline__ int floor_div(int a, int b) {        // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ int ceil_div(int a, int b) { return -floor_div(-a, b); }

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// union-find over the run ids of one frame: parents only ever point to smaller ids, so the root of a component is its smallest id
__device__ __forceinline__ int uf_find(const int* par, int x) {
  for (int p = ld_agent(par + x); p != x; p = ld_agent(par + x)) x = p;
  return x;
}
__device__ void uf_unite(int* par, int a, int b) {
  for (;;) {
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + b, a);
    if (old == b) return;                   // b was a root and now hangs below a
    b = old;                                // b was re-parented meanwhile: unite a with its new parent instead
  }
}

// global stores and atomics of this workgroup visible to all of its waves: the agent-scope fence drops the CU's stale L1 lines
__device__ __forceinline__ void phase_sync() {
  __threadfence();
  __syncthreads();
}

__device__ __forceinline__ int vy(int v) { return v >> 16; }
__device__ __forceinline__ int vx(int v) { return v & 0xFFFF; }

// x-range [lo, hi] of the pixels that the 8-connected line A -> B (A.y < B.y) puts in row y (A.y <= y <= B.y)
__device__ __forceinline__ void line_pixels(int a, int b, int y, int& lo, int& hi) {
  const int dy = vy(b) - vy(a), dx = vx(b) - vx(a), k = y - vy(a);
  if (abs(dx) <= dy) {                      // y-major: one pixel, x = floor(x(y) + 1/2)
    lo = hi = vx(a) + floor_div(2 * dx * k + dy, 2 * dy);
    return;
  }
  int ulo, uhi;                             // x-major: the columns u = x - A.x with floor(y(u) + 1/2) == y
  if (dx > 0) {
    ulo = max(ceil_div((2 * k - 1) * dx, 2 * dy), 0);
    uhi = min(ceil_div((2 * k + 1) * dx, 2 * dy) - 1, dx);
  } else {
    ulo = max(floor_div((2 * k + 1) * dx, 2 * dy) + 1, dx);
    uhi = min(floor_div((2 * k - 1) * dx, 2 * dy), 0);
  }
  lo = vx(a) + ulo;
  hi = vx(a) + uhi;
}

// Workspace per slot: 5 arrays of H * S ints (S = ceil(W / 2) = most runs a row can hold).
//   par   union-find parents, then component labels
//   cmp   at a root: the component's last row, then its offset into the per-(component, row) arrays
//   lo    per (component, row): leftmost pixel -> left hull chain (in place)
//   hi    per (component, row): rightmost pixel -> right hull chain (in place)
//   ivl   per (component, row): the filled interval
__global__ __launch_bounds__(HULL_THREADS) void edit_hull_kernel(const unsigned char* __restrict__ bin, int n, int H, int W,
                                                                 unsigned* __restrict__ runs_all, int* __restrict__ nruns_all,
                                                                 int* __restrict__ ws) {
  __shared__ int nr[HULL_MAX_H];
  __shared__ int next_off;
  const int S = (W + 1) / 2;
  const int64_t NS = (int64_t)H * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = HULL_THREADS / 64;
  int* par = ws + (int64_t)blockIdx.x * 5 * NS;
  int* cmp = par + NS;
  int* lo = cmp + NS;
  int* hi = lo + NS;
  int* ivl = hi + NS;
  const unsigned long long below = (1ull << lane) - 1;

  for (int f = blockIdx.x; f < n; f += gridDim.x) {
    const unsigned char* img = bin + (int64_t)f * H * W;
    unsigned* runs = runs_all + (int64_t)f * NS;
    unsigned short* run16 = reinterpret_cast<unsigned short*>(runs);   // run k of row y: [2 (y S + k)] = start, [+1] = end
    int* nruns = nruns_all + (int64_t)f * H;
    if (threadIdx.x == 0) next_off = 0;

    // 1. runs of every row (one wave per row), sorted by x
    for (int y = wave; y < H; y += NW) {
      const unsigned char* row = img + (int64_t)y * W;
      int ns = 0, ne = 0;
      for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool v = x < W && row[x];
        const bool st = v && (x == 0 || !row[x - 1]);
        const bool en = v && (x + 1 == W || !row[x + 1]);
        const unsigned long long ms = __ballot(st), me = __ballot(en);
        if (st) {
          const int k = ns + __popcll(ms & below);
          run16[2 * ((int64_t)y * S + k)] = (unsigned short)x;
          par[(int64_t)y * S + k] = y * S + k;
        }
        if (en) run16[2 * ((int64_t)y * S + ne + __popcll(me & below)) + 1] = (unsigned short)x;
        ns += __popcll(ms);
        ne += __popcll(me);
      }
      if (lane == 0) {
        nr[y] = ns;
        nruns[y] = ns;
      }
    }
    phase_sync();

    // 2. unite every run with the runs of the row above that touch it (8-connectivity: [s - 1, e + 1] overlaps)
    for (int y = 1 + wave; y < H; y += NW) {
      const int n0 = nr[y - 1];
      const unsigned* up = runs + (int64_t)(y - 1) * S;
      for (int k = lane; k < nr[y]; k += 64) {
        const unsigned r = runs[(int64_t)y * S + k];
        const int s = (int)(r & 0xFFFF), e = (int)(r >> 16);
        int a = 0, b = n0;                  // first run above whose end reaches s - 1
        while (a < b) {
          const int m = (a + b) >> 1;
          if ((int)(up[m] >> 16) < s - 1) a = m + 1; else b = m;
        }
        for (; a < n0 && (int)(up[a] & 0xFFFF) <= e + 1; ++a) uf_unite(par, (y - 1) * S + a, y * S + k);
      }
    }
    phase_sync();

    // 3. labels; a root starts its component's last row at its own
    for (int y = wave; y < H; y += NW)
      for (int k = lane; k < nr[y]; k += 64) {
        const int id = y * S + k, root = uf_find(par, id);
        __hip_atomic_store(par + id, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (root == id) cmp[id] = y;
      }
    phase_sync();
    for (int y = wave; y < H; y += NW)
      for (int k = lane; k < nr[y]; k += 64) atomicMax(cmp + par[y * S + k], y);
    phase_sync();

    // 4. per component: rows [y0, y1] get consecutive slots (every row of an 8-connected component holds one of its runs)
    for (int y = wave; y < H; y += NW)
      for (int k = lane; k < nr[y]; k += 64) {
        const int id = y * S + k;
        if (par[id] != id) continue;
        const int h = cmp[id] - y + 1, o = atomicAdd(&next_off, h);
        cmp[id] = o;
        ivl[o] = h;                         // read back by step 5 before it writes the row intervals
        for (int j = 0; j < h; ++j) {
          lo[o + j] = 0x7FFFFFFF;
          hi[o + j] = -1;
        }
      }
    phase_sync();
    for (int y = wave; y < H; y += NW)
      for (int k = lane; k < nr[y]; k += 64) {
        const int id = y * S + k, root = par[id];
        const int o = cmp[root] + y - root / S;
        const unsigned r = runs[id];
        atomicMin(lo + o, (int)(r & 0xFFFF));
        atomicMax(hi + o, (int)(r >> 16));
      }
    phase_sync();

    // 5. per component (one thread): hull chains, then the filled interval of every row
    for (int y = wave; y < H; y += NW)
      for (int k = lane; k < nr[y]; k += 64) {
        const int id = y * S + k;
        if (par[id] != id) continue;
        const int o = cmp[id];
        int* L = lo + o;                    // vertices (y << 16 | x), written over the rows already read
        int* R = hi + o;
        const int h = ivl[o];
        int nl = 0, nrt = 0;
        for (int j = 0; j < h; ++j) {
          const int xl = L[j], xr = R[j], yy = y + j;
          const int pl = (yy << 16) | xl, pr = (yy << 16) | xr;
          while (nl >= 2) {                 // left chain: keep only vertices strictly left of the line through their neighbours
            const int a = L[nl - 2], b = L[nl - 1];
            if ((vx(b) - vx(a)) * (yy - vy(a)) >= (xl - vx(a)) * (vy(b) - vy(a))) --nl; else break;
          }
          L[nl++] = pl;
          while (nrt >= 2) {
            const int a = R[nrt - 2], b = R[nrt - 1];
            if ((vx(b) - vx(a)) * (yy - vy(a)) <= (xr - vx(a)) * (vy(b) - vy(a))) --nrt; else break;
          }
          R[nrt++] = pr;
        }
        int* out = ivl + o;
        const bool collinear = h == 1 || (nl == 2 && nrt == 2 && L[0] == R[0] && L[1] == R[1]);
        int il = 0, ir = 0;
        for (int j = 0; j < h; ++j) {
          if (collinear) {
            out[j] = (int)IVL_EMPTY;
            continue;
          }
          const int yy = y + j;
          while (il < nl - 2 && vy(L[il + 1]) < yy) ++il;
          while (ir < nrt - 2 && vy(R[ir + 1]) < yy) ++ir;
          const int la = L[il], lb = L[il + 1], ra = R[ir], rb = R[ir + 1];
          int a = vx(la) + ceil_div((vx(lb) - vx(la)) * (yy - vy(la)), vy(lb) - vy(la));     // closed hull: ceil(left), floor(right)
          int b = vx(ra) + floor_div((vx(rb) - vx(ra)) * (yy - vy(ra)), vy(rb) - vy(ra));
          int p, q;
          line_pixels(la, lb, yy, p, q); a = min(a, p); b = max(b, q);
          line_pixels(ra, rb, yy, p, q); a = min(a, p); b = max(b, q);
          if (il + 2 < nl && vy(lb) == yy) { line_pixels(lb, L[il + 2], yy, p, q); a = min(a, p); b = max(b, q); }
          if (ir + 2 < nrt && vy(rb) == yy) { line_pixels(rb, R[ir + 2], yy, p, q); a = min(a, p); b = max(b, q); }
          out[j] = (int)((unsigned)max(a, 0) | ((unsigned)min(b, W - 1) << 16));
        }
      }
    phase_sync();

    // 6. every run slot: the interval of its (component, row)
    for (int y = wave; y < H; y += NW)
      for (int k = lane; k < nr[y]; k += 64) {
        const int id = y * S + k, root = par[id];
        runs[id] = (unsigned)ivl[cmp[root] + y - root / S];
      }
    phase_sync();
  }
}

// out[y][x] = 1 iff some interval [a, b] of a row y' with |y - y'| <= r has a - hw[|y - y'|] <= x <= b + hw[|y - y'|]
__global__ __launch_bounds__(256) void edit_dilate_kernel(const unsigned* __restrict__ runs_all, const int* __restrict__ nruns_all, int H,
                                                          int W, const int* __restrict__ hw, int radius, unsigned char* __restrict__ out) {
  extern __shared__ int diff[];             // W + 1 counters
  __shared__ int part[4];
  const int y = blockIdx.x, f = blockIdx.y, S = (W + 1) / 2;
  const unsigned* runs = runs_all + (int64_t)f * H * S;
  const int* nruns = nruns_all + (int64_t)f * H;
  for (int x = threadIdx.x; x <= W; x += 256) diff[x] = 0;
  __syncthreads();
  for (int j = threadIdx.x; j <= 2 * radius; j += 256) {
    const int yy = y - radius + j;
    if (yy < 0 || yy >= H) continue;
    const int grow = hw[abs(j - radius)], m = nruns[yy];
    const unsigned* row = runs + (int64_t)yy * S;
    for (int k = 0; k < m; ++k) {
      const unsigned v = row[k];
      const int a = (int)(v & 0xFFFF), b = (int)(v >> 16);
      if (a > b) continue;
      atomicAdd(&diff[max(a - grow, 0)], 1);
      atomicAdd(&diff[min(b + grow, W - 1) + 1], -1);
    }
  }
  __syncthreads();
  // prefix sum: thread t owns columns [t C, t C + C)
  const int C = (W + 255) / 256, x0 = threadIdx.x * C, x1 = min(x0 + C, W);
  int own = 0;
  for (int x = x0; x < x1; ++x) own += diff[x];
  int incl = own;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int run = incl - own;
  for (int w = 0; w < wave; ++w) run += part[w];
  unsigned char* o = out + ((int64_t)f * H + y) * W;
  for (int x = x0; x < x1; ++x) {
    run += diff[x];
    o[x] = run > 0 ? 1 : 0;
  }
}

}  // namespace

extern "C" int flexam_edit_mask_blur(const unsigned char* src, int n, int H, int W, const double* weights, int radius, float* tmp,
                                     unsigned char* dst, void* stream) {
  FX_REQUIRE(src && weights && tmp && dst, FLEXAM_E_ARG, "edit_mask_blur: null pointer");
  FX_REQUIRE(n > 0 && H > 0 && W > 0 && radius >= 0, FLEXAM_E_SHAPE, "edit_mask_blur: n=%d H=%d W=%d radius=%d", n, H, W, radius);
  const int64_t total = (int64_t)n * H * W;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(edit_blur_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, nullptr, total, H, W, weights, radius, tmp, nullptr);
  hipLaunchKernelGGL(edit_blur_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, nullptr, tmp, total, H, W, weights, radius, nullptr, dst);
  return flexam_check_launch("flexam_edit_mask_blur");
}

extern "C" int flexam_edit_mask_hull(const unsigned char* bin, int n, int H, int W, unsigned* runs, int* nruns, int* ws, int slots,
                                     void* stream) {
  FX_REQUIRE(bin && runs && nruns && ws, FLEXAM_E_ARG, "edit_mask_hull: null pointer");
  FX_REQUIRE(n > 0 && H > 0 && W > 0 && slots > 0, FLEXAM_E_SHAPE, "edit_mask_hull: n=%d H=%d W=%d slots=%d", n, H, W, slots);
  FX_REQUIRE(H <= HULL_MAX_H && W <= EDIT_MAX_W, FLEXAM_E_SHAPE, "edit_mask_hull: frames up to %d x %d, got %d x %d", HULL_MAX_H, EDIT_MAX_W, H, W);
  hipLaunchKernelGGL(edit_hull_kernel, dim3((unsigned)min(n, slots)), dim3(HULL_THREADS), 0, (hipStream_t)stream, bin, n, H, W, runs, nruns, ws);
  return flexam_check_launch("flexam_edit_mask_hull");
}

extern "C" int flexam_edit_mask_dilate(const unsigned* runs, const int* nruns, int n, int H, int W, const int* half_widths, int radius,
                                       unsigned char* out, void* stream) {
  FX_REQUIRE(runs && nruns && half_widths && out, FLEXAM_E_ARG, "edit_mask_dilate: null pointer");
  FX_REQUIRE(n > 0 && H > 0 && W > 0 && radius >= 0, FLEXAM_E_SHAPE, "edit_mask_dilate: n=%d H=%d W=%d radius=%d", n, H, W, radius);
  FX_REQUIRE(H <= HULL_MAX_H && W <= EDIT_MAX_W && n <= 65535, FLEXAM_E_SHAPE, "edit_mask_dilate: n=%d frames of %d x %d", n, H, W);
  hipLaunchKernelGGL(edit_dilate_kernel, dim3((unsigned)H, (unsigned)n), dim3(256), (size_t)(W + 1) * sizeof(int), (hipStream_t)stream, runs,
                     nruns, H, W, half_widths, radius, out);
  return flexam_check_launch("flexam_edit_mask_dilate");
}
