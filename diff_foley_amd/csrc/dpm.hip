// The two tensor operations of the DPM-Solver family that are not linear combinations (dpm_solver.py:386-399, 948-955): the data
// prediction x0 = (x - sigma eps) / alpha with Imagen's dynamic thresholding, and the error norm of the adaptive step-size solver.
// fp32 throughout, stateless like df_lincomb, no global atomics, no inline assembly: equal inputs give equal bits.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int DP_THREADS = 1024;      // thresholding: one block of 16 wavefronts per sample (n <= 64 Ki: at most 64 elements a lane a pass)
constexpr float DP_Q = 0.995f;        // the quantile of dpm_solver.py:395

__device__ __forceinline__ float dp_nan() { return __builtin_nanf(""); }

// The one expression every pass evaluates: an explicit fma and an IEEE division, so that no pass can contract it differently from
// another and the same element has the same bits in the histogram passes and in the store.
__device__ __forceinline__ float dp_x0(float x, float e, float sigma, float alpha) { return __builtin_fmaf(-sigma, e, x) / alpha; }

__global__ void data_prediction_plain_kernel(const float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ out,
                                             long total, float alpha, float sigma) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    out[i] = dp_x0(x[i], eps[i], sigma, alpha);
}

// s[b] = max(quantile_0.995(|x0[b]|), max_val); out[b] = clamp(x0[b], -s, s) / s.  The quantile is torch.quantile's 'linear' rule:
// rank = q (n - 1) in fp32, the order statistics k = floor(rank) and k + 1 of |x0| (ascending, 0-based) and
// lerp(v_k, v_k+1, rank - k).  v_k is SELECTED, not sorted for: the bit pattern of a non-negative float is monotone in its value, so
// four passes over the sample -- each a 256-bin LDS histogram of the next 8 bits among the elements that share the bits chosen so far
// -- fix the pattern of v_k from the top byte down.  Integer LDS atomics: the histogram does not depend on the order of arrival.
// The last histogram also says how many elements equal v_k; if rank k + 1 lies beyond them, v_k+1 is the smallest pattern above
// v_k's, found by one more pass (LDS atomicMin).  A NaN anywhere in the sample (pattern above +inf's) makes s and every output of that
// sample NaN, as torch.quantile does.  x0 is never stored between passes: dp_x0 is evaluated again.
__global__ __launch_bounds__(DP_THREADS) void data_prediction_threshold_kernel(const float* __restrict__ x,
                                                                              const float* __restrict__ eps, float* __restrict__ out,
                                                                              float* __restrict__ s_out, int n, float alpha, float sigma,
                                                                              float max_val) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[4];      // [0] chosen bin, [1] rank inside it, [2] its count, [3] NaN seen
  __shared__ unsigned above;       // smallest pattern > v_k's
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* xb = x + (long)b * n;
  const float* eb = eps + (long)b * n;
  float* ob = out + (long)b * n;

  const float rank = DP_Q * (float)(n - 1);
  int k_lo = (int)floorf(rank);
  if (k_lo > n - 1) k_lo = n - 1;
  const float frac = rank - (float)k_lo;
  const bool two = frac > 0.f && k_lo + 1 <= n - 1;

  if (tid < 4) sel[tid] = 0u;
  if (tid == 0) above = 0xffffffffu;
  unsigned prefix = 0u, mask = 0u, k = (unsigned)k_lo, eq = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += DP_THREADS) {
      const unsigned bits = __builtin_bit_cast(unsigned, dp_x0(xb[i], eb[i], sigma, alpha)) & 0x7fffffffu;
      if (pass == 0 && bits > 0x7f800000u) sel[3] = 1u;      // every writer writes the same value
      if ((bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {      // wavefront 0: lane l owns bins 4l .. 4l + 3; an inclusive scan of the lane totals finds the bin that holds rank k
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned mine = c0 + c1 + c2 + c3;
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o);
        if (tid >= o) incl += up;
      }
      const unsigned excl = incl - mine;
      if (k >= excl && k < incl) {      // exactly one lane: the elements that match the prefix number more than k
        unsigned r = k - excl, bin = 4u * tid, cnt = c0;
        if (r >= c0) {
          r -= c0; bin += 1; cnt = c1;
          if (r >= c1) {
            r -= c1; bin += 1; cnt = c2;
            if (r >= c2) { r -= c2; bin += 1; cnt = c3; }
          }
        }
        sel[0] = bin; sel[1] = r; sel[2] = cnt;
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 255u << shift;
    k = sel[1];
    eq = sel[2];
    // the next pass zeroes hist and meets a barrier before anyone writes sel again
  }
  // prefix is the pattern of v_k; k its rank among the eq elements equal to it
  unsigned hi_bits = prefix;
  if (two && k + 1 >= eq) {      // block-uniform: rank k + 1 is the first element above v_k
    for (int i = tid; i < n; i += DP_THREADS) {
      const unsigned bits = __builtin_bit_cast(unsigned, dp_x0(xb[i], eb[i], sigma, alpha)) & 0x7fffffffu;
      if (bits > prefix) atomicMin(&above, bits);
    }
    __syncthreads();
    hi_bits = above;      // n - 1 >= k + 1: such an element exists
  }
  const float v_lo = __builtin_bit_cast(float, prefix), v_hi = __builtin_bit_cast(float, hi_bits);
  float s = v_lo;
  if (two) {      // at::lerp
    const float d = v_hi - v_lo;
    s = frac < 0.5f ? v_lo + frac * d : v_hi - d * (1.f - frac);
  }
  s = fmaxf(s, max_val);
  if (sel[3] || max_val != max_val) s = dp_nan();
  if (tid == 0 && s_out) s_out[b] = s;
  if (s != s) {
    for (int i = tid; i < n; i += DP_THREADS) ob[i] = s;
    return;
  }
  for (int i = tid; i < n; i += DP_THREADS) {
    const float v = dp_x0(xb[i], eb[i], sigma, alpha);
    ob[i] = fminf(fmaxf(v, -s), s) / s;
  }
}

constexpr int AE_THREADS = 256;

// norm[b] = sqrt(mean_i(((hi - lo) / max(atol, rtol max(|lo|, |prev|)))^2)): one block per sample, per-lane sums in index order, a DPP
// tree per wavefront, the four wavefront totals added in slot order.
__global__ __launch_bounds__(AE_THREADS) void adaptive_error_sample_kernel(const float* __restrict__ hi, const float* __restrict__ lo,
                                                                          const float* __restrict__ prev, float* __restrict__ norm,
                                                                          long n, float atol, float rtol) {
  __shared__ __attribute__((aligned(16))) float red[16];
  const long off = (long)blockIdx.x * n;
  float acc = 0.f;
  for (long i = threadIdx.x; i < n; i += AE_THREADS) {
    const float l = lo[off + i];
    const float delta = fmaxf(atol, rtol * fmaxf(fabsf(l), fabsf(prev[off + i])));
    const float q = (hi[off + i] - l) / delta;
    acc += q * q;
  }
  const float total = block_sum_dpp_fresh(acc, red);
  if (threadIdx.x == 0) norm[blockIdx.x] = sqrtf(total / (float)n);
}

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? dp_nan() : fmaxf(a, b); }

// E = max_b norm[b], NaN if any is (torch's max): one wavefront, lane l takes samples l, l + 64, ...
__global__ __launch_bounds__(64) void adaptive_error_max_kernel(const float* __restrict__ norm, float* __restrict__ out, int B) {
  float m = -INFINITY;
  for (int b = threadIdx.x; b < B; b += 64) m = nan_max(m, norm[b]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o));
  if (threadIdx.x == 0) out[0] = m;
}

}  // namespace

hipError_t launch_dpm_data_prediction(const float* x, const float* eps, float* out, float* s_out, int B, long n, float alpha,
                                      float sigma, int thresholding, float max_val, hipStream_t s) {
  if (B <= 0 || n <= 0 || !x || !eps || !out) return hipErrorInvalidValue;
  if (!thresholding) {
    const long total = (long)B * n;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(data_prediction_plain_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, eps, out, total, alpha, sigma);
    return hipGetLastError();
  }
  if (n > (1L << 30)) return hipErrorInvalidValue;      // ranks and histogram counts are 32-bit
  hipLaunchKernelGGL(data_prediction_threshold_kernel, dim3((unsigned)B), dim3(DP_THREADS), 0, s, x, eps, out, s_out, (int)n, alpha,
                     sigma, max_val);
  return hipGetLastError();
}

hipError_t launch_dpm_adaptive_error(const float* x_hi, const float* x_lo, const float* x_prev, float* norm, float* out, int B, long n,
                                     float atol, float rtol, hipStream_t s) {
  if (B <= 0 || n <= 0 || !x_hi || !x_lo || !x_prev || !norm || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(adaptive_error_sample_kernel, dim3((unsigned)B), dim3(AE_THREADS), 0, s, x_hi, x_lo, x_prev, norm, n, atol, rtol);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(adaptive_error_max_kernel, dim3(1), dim3(64), 0, s, (const float*)norm, out, B);
  return hipGetLastError();
}
