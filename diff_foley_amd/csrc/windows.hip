// Overlapped windows of a long fp32 NCHW tensor ("Videos longer than one window"): the copy that cuts K windows
// of Ww columns out of [B][rows][W] (rows = C * H), and the tent-weighted blend that puts K per-window results back together.
//   gather   win[b * K + k][row][j] = x[b][row][starts[k] + j]
//   blend    out[b][row][x] = (sum_k w(x - starts[k]) * win[b * K + k][row][x - starts[k]]) * inv_n[x],   w(j) = min(j + 1, Ww - j)
// over the windows that cover column x, in ascending k.  The blend is gather-form: one output element per thread, a loop over the
// covering windows k_first[x] .. k_first[x] + k_count[x] - 1 (starts ascend, so they are consecutive), one fma per window from a zero
// accumulator and one multiply by inv_n[x] = fp32(1 / n(x)), n(x) = sum_k w(x - starts[k]) an integer, the reciprocal taken in double
// on the host.  No atomics, no scatter, plain loads and stores: equal inputs give equal bits.  4-byte accesses throughout -- window
// starts are any integers, so no wider alignment is known; both kernels move at most a few MB beside a UNet step that moves GBs.
// The per-geometry tables (starts, k_first, k_count, inv_n) are built on the host once and kept on the device (window_tables).
#include <map>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int WN_THREADS = 256;
constexpr long WN_MAX_BLOCKS = 4096;

__global__ __launch_bounds__(WN_THREADS) void window_gather_kernel(const float* __restrict__ x, float* __restrict__ win,
                                                                   const int* __restrict__ starts, int K, long rows, int Ww, int W,
                                                                   long total) {
  for (long i = (long)blockIdx.x * WN_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * WN_THREADS) {
    const int j = (int)(i % Ww);
    const long r = i / Ww;               // (b * K + k) * rows + row
    const long row = r % rows;
    const long bk = r / rows;
    const int k = (int)(bk % K);
    const long b = bk / K;
    win[i] = x[(b * rows + row) * W + starts[k] + j];
  }
}

__global__ __launch_bounds__(WN_THREADS) void window_blend_kernel(const float* __restrict__ win, float* __restrict__ out,
                                                                  const int* __restrict__ starts, const int* __restrict__ k_first,
                                                                  const int* __restrict__ k_count, const float* __restrict__ inv_n,
                                                                  int K, long rows, int Ww, int W, long total) {
  for (long i = (long)blockIdx.x * WN_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * WN_THREADS) {
    const int col = (int)(i % W);
    const long r = i / W;                // b * rows + row
    const long row = r % rows;
    const long b = r / rows;
    const int k0 = k_first[col], k1 = k0 + k_count[col];
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) {
      const int j = col - starts[k];
      const float w = (float)min(j + 1, Ww - j);
      acc = __builtin_fmaf(w, win[((b * K + k) * rows + row) * Ww + j], acc);
    }
    out[i] = acc * inv_n[col];
  }
}

struct Geometry {
  int device, Ww, W;
  std::vector<int> starts;
  bool operator<(const Geometry& o) const {
    if (device != o.device) return device < o.device;
    if (Ww != o.Ww) return Ww < o.Ww;
    if (W != o.W) return W < o.W;
    return starts < o.starts;
  }
};

// one block per geometry: starts[K] | k_first[W] | k_count[W] | inv_n[W].  Reached through the C entries only, which hold the API lock
std::map<Geometry, int*> g_tables;
constexpr size_t WN_MAX_GEOMETRIES = 64;

unsigned blocks_for(long total) {
  const long b = (total + WN_THREADS - 1) / WN_THREADS;
  return (unsigned)(b < WN_MAX_BLOCKS ? b : WN_MAX_BLOCKS);
}

}  // namespace

bool window_geometry_ok(const int* starts, int K, int Ww, int W, const char** why) {
  const char* bad = nullptr;
  if (!starts || K < 1) bad = "at least one window";
  else if (Ww < 1 || W < Ww) bad = "1 <= window width <= total width";
  for (int k = 0; !bad && k < K; ++k) {
    if (starts[k] < 0) bad = "a window starts left of column 0";
    else if (starts[k] > W - Ww) bad = "a window ends right of the last column";
    else if (k && starts[k] < starts[k - 1]) bad = "window starts must ascend";
    else if (k && starts[k] > starts[k - 1] + Ww) bad = "a column between two windows is covered by none";
  }
  if (!bad && starts[0] != 0) bad = "column 0 is covered by no window";
  if (!bad && starts[K - 1] + Ww != W) bad = "the last column is covered by no window";
  if (why) *why = bad;
  return bad == nullptr;
}

hipError_t window_tables(const int* starts, int K, int Ww, int W, WindowTables* out) {
  if (!out || !window_geometry_ok(starts, K, Ww, W, nullptr)) return hipErrorInvalidValue;
  Geometry g;
  hipError_t e = hipGetDevice(&g.device);
  if (e != hipSuccess) return e;
  g.Ww = Ww;
  g.W = W;
  g.starts.assign(starts, starts + K);
  auto it = g_tables.find(g);
  if (it == g_tables.end()) {
    // a miss builds the tables on the host and uploads them with a blocking copy: once per geometry, never inside a step loop
    std::vector<int> host((size_t)K + 3 * (size_t)W);
    int* first = host.data() + K;
    int* count = first + W;
    float* inv = reinterpret_cast<float*>(count + W);
    for (int k = 0; k < K; ++k) host[k] = starts[k];
    for (int x = 0; x < W; ++x) {
      long n = 0;
      int k0 = -1, c = 0;
      for (int k = 0; k < K; ++k) {
        const int j = x - starts[k];
        if (j < 0 || j >= Ww) continue;
        if (k0 < 0) k0 = k;
        ++c;
        n += j + 1 < Ww - j ? j + 1 : Ww - j;
      }
      if (k0 < 0 || n <= 0) return hipErrorInvalidValue;      // window_geometry_ok rules it out
      first[x] = k0;
      count[x] = c;
      inv[x] = (float)(1.0 / (double)n);
    }
    if (g_tables.size() >= WN_MAX_GEOMETRIES) {      // hipFree waits for the device: nothing in flight reads a freed table
      for (auto& kv : g_tables) (void)hipFree(kv.second);
      g_tables.clear();
    }
    int* dev = nullptr;
    e = hipMalloc(&dev, host.size() * sizeof(int));
    if (e != hipSuccess) return e;
    e = hipMemcpy(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dev);
      return e;
    }
    it = g_tables.emplace(std::move(g), dev).first;
  }
  out->starts = it->second;
  out->k_first = it->second + K;
  out->k_count = out->k_first + W;
  out->inv_n = reinterpret_cast<const float*>(out->k_count + W);
  return hipSuccess;
}

hipError_t launch_window_gather(const float* x, float* win, const WindowTables& t, int B, int K, long rows, int Ww, int W,
                                hipStream_t s) {
  if (B <= 0 || K <= 0 || rows <= 0 || Ww <= 0 || W < Ww || !x || !win || !t.starts) return hipErrorInvalidValue;
  const long total = (long)B * K * rows * Ww;
  hipLaunchKernelGGL(window_gather_kernel, dim3(blocks_for(total)), dim3(WN_THREADS), 0, s, x, win, t.starts, K, rows, Ww, W, total);
  return hipGetLastError();
}

hipError_t launch_window_blend(const float* win, float* out, const WindowTables& t, int B, int K, long rows, int Ww, int W,
                               hipStream_t s) {
  if (B <= 0 || K <= 0 || rows <= 0 || Ww <= 0 || W < Ww || !win || !out || !t.starts || !t.k_first || !t.k_count || !t.inv_n)
    return hipErrorInvalidValue;
  const long total = (long)B * rows * W;
  hipLaunchKernelGGL(window_blend_kernel, dim3(blocks_for(total)), dim3(WN_THREADS), 0, s, win, out, t.starts, t.k_first, t.k_count,
                     t.inv_n, K, rows, Ww, W, total);
  return hipGetLastError();
}
