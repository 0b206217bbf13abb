// The forward process and the denoising loss of LatentDiffusion at a PER-SAMPLE timestep (ddpm.py:279-297, 1046-1081; the samplers'
// stochastic_encode, ddim.py:400-413): q_sample and the reduction behind loss_dict.  fp32 throughout, no atomics, no inline assembly;
// the timestep vector stays on the device, so neither launch needs the host to know a timestep.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int QS_THREADS = 256;
constexpr int QS_MAX_CHUNKS = 64;      // blocks per sample at most: 64 x 256 float4 per pass, grid-stride beyond that

__device__ __forceinline__ float quiet_nan() { return __builtin_nanf(""); }

// out[b][:] = A[t[b]] * x0[b][:] + S[t[b]] * noise[b][:].  One sample per blockIdx.x / chunks, so the two table values are read once
// per thread through a wave-uniform address.  An index outside [0, T) reads nothing from the tables: both coefficients are NaN and so
// is every element of that sample's output (NaN * finite = NaN, NaN * 0 = NaN).
// Each sample is walked as head | body | tail: `head` scalar elements up to the first 16-byte boundary, `nv` float4, the rest scalar.
// base_mis = floats between a 16-byte boundary and x0's first element; aligned = 0 when the three tensors do not share that distance:
// the whole sample is then walked scalar.
__global__ __launch_bounds__(QS_THREADS) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                             const long long* __restrict__ t, const float* __restrict__ A,
                                                             const float* __restrict__ S, float* __restrict__ out, int B, long n,
                                                             int T, int chunks, int base_mis, int aligned) {
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  if (b >= B) return;
  const long long tb = t[b];
  const bool ok = tb >= 0 && tb < (long long)T;
  const float a = ok ? A[tb] : quiet_nan();
  const float s = ok ? S[tb] : quiet_nan();
  const long off = (long)b * n;
  const float* xb = x0 + off;
  const float* nb = noise + off;
  float* ob = out + off;
  long head = n, nv = 0;      // scalar everything unless the tensors share an alignment
  if (aligned) {
    const int mis = (int)(((long)base_mis + off) & 3);      // floats past a 16-byte boundary at this sample's first element
    head = (4 - mis) & 3;
    if (head > n) head = n;
    nv = (n - head) >> 2;
  }
  const long tail0 = head + 4 * nv;      // first element behind the float4 body; tail0 <= n
  const long stride = (long)chunks * QS_THREADS;
  const long tid = (long)chunk * QS_THREADS + threadIdx.x;
  for (long v = tid; v < nv; v += stride) {
    const float4 xv = *reinterpret_cast<const float4*>(xb + head + 4 * v);
    const float4 nz = *reinterpret_cast<const float4*>(nb + head + 4 * v);
    *reinterpret_cast<float4*>(ob + head + 4 * v) =
        make_float4(a * xv.x + s * nz.x, a * xv.y + s * nz.y, a * xv.z + s * nz.z, a * xv.w + s * nz.w);
  }
  for (long i = tid; i < head; i += stride) ob[i] = a * xb[i] + s * nb[i];
  for (long i = tail0 + tid; i < n; i += stride) ob[i] = a * xb[i] + s * nb[i];
}

constexpr int DL_THREADS = 256;      // four wavefronts per sample

// loss_simple[b] = mean over n of (target - pred)^2 (loss_type 0) or |target - pred| (1): one block per sample.  A lane adds its
// elements in index order, the 64 lanes of a wavefront meet in a DPP tree (wave_sum_dpp_bcast: no LDS pipe), the four wavefront
// totals meet in LDS and are added in slot order -- the same order in every run, so the result is a pure function of the inputs.
// An out-of-range t[b] makes the sample's loss NaN (its terms are still only read from pred / target, never from a table).
__global__ __launch_bounds__(DL_THREADS) void diffusion_loss_sample_kernel(const float* __restrict__ pred,
                                                                          const float* __restrict__ target,
                                                                          const long long* __restrict__ t, float* __restrict__ loss_simple,
                                                                          long n, int T, int loss_type, int vec) {
  __shared__ __attribute__((aligned(16))) float red[16];
  const int b = blockIdx.x;
  const float* pb = pred + (long)b * n;
  const float* gb = target + (long)b * n;
  float acc = 0.f;
  const long nv = vec ? (n >> 2) : 0;
  if (loss_type == 0) {
    for (long v = threadIdx.x; v < nv; v += DL_THREADS) {
      const float4 p = *reinterpret_cast<const float4*>(pb + 4 * v), g = *reinterpret_cast<const float4*>(gb + 4 * v);
      const float d0 = g.x - p.x, d1 = g.y - p.y, d2 = g.z - p.z, d3 = g.w - p.w;
      acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
    }
    for (long i = 4 * nv + threadIdx.x; i < n; i += DL_THREADS) {
      const float d = gb[i] - pb[i];
      acc += d * d;
    }
  } else {
    for (long v = threadIdx.x; v < nv; v += DL_THREADS) {
      const float4 p = *reinterpret_cast<const float4*>(pb + 4 * v), g = *reinterpret_cast<const float4*>(gb + 4 * v);
      acc += fabsf(g.x - p.x); acc += fabsf(g.y - p.y); acc += fabsf(g.z - p.z); acc += fabsf(g.w - p.w);
    }
    for (long i = 4 * nv + threadIdx.x; i < n; i += DL_THREADS) acc += fabsf(gb[i] - pb[i]);
  }
  const float total = block_sum_dpp_fresh(acc, red);
  if (threadIdx.x == 0) {
    const long long tb = t[b];
    loss_simple[b] = (tb >= 0 && tb < (long long)T) ? total / (float)n : quiet_nan();
  }
}

// The five scalars of loss_dict (ddpm.py:1062-1079) from loss_simple[B]: ONE wavefront.  Lane l adds samples l, l + 64, ... in that
// order, then the DPP tree: a fixed-order sum over B.  out = { mean(loss_simple), mean(loss_simple / exp(logvar[t]) + logvar[t]),
// mean(lvlb_weights[t] * loss_simple), l_simple_weight * out[1] + original_elbo_weight * out[2], mean(logvar) over the table }.
// A sample with t outside [0, T) contributes NaN to the first four and reads neither table.
__global__ __launch_bounds__(64) void diffusion_loss_means_kernel(const float* __restrict__ loss_simple, const long long* __restrict__ t,
                                                                 const float* __restrict__ logvar, const float* __restrict__ lvlb,
                                                                 float* __restrict__ out, int B, int T, float l_simple_weight,
                                                                 float original_elbo_weight) {
  float s_simple = 0.f, s_gamma = 0.f, s_vlb = 0.f, s_lv = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    const long long tb = t[b];
    const bool ok = tb >= 0 && tb < (long long)T;
    const float ls = loss_simple[b];
    const float lv = ok ? logvar[tb] : quiet_nan();
    const float w = ok ? lvlb[tb] : quiet_nan();
    s_simple += ls;
    s_gamma += ls / expf(lv) + lv;
    s_vlb += w * ls;
  }
  for (int i = threadIdx.x; i < T; i += 64) s_lv += logvar[i];
  s_simple = wave_sum_dpp_bcast(s_simple);
  s_gamma = wave_sum_dpp_bcast(s_gamma);
  s_vlb = wave_sum_dpp_bcast(s_vlb);
  s_lv = wave_sum_dpp_bcast(s_lv);
  if (threadIdx.x == 0) {
    const float gamma = s_gamma / (float)B, vlb = s_vlb / (float)B;
    out[0] = s_simple / (float)B;
    out[1] = gamma;
    out[2] = vlb;
    out[3] = l_simple_weight * gamma + original_elbo_weight * vlb;
    out[4] = s_lv / (float)T;
  }
}

inline int mis_of(const void* p) { return (int)(((uintptr_t)p & 15) >> 2); }

}  // namespace

hipError_t launch_q_sample(const float* x0, const float* noise, const long long* t, const float* A, const float* S, float* out,
                           int B, long n, int T, hipStream_t s) {
  if (B <= 0 || n <= 0 || T <= 0 || !x0 || !noise || !t || !A || !S || !out) return hipErrorInvalidValue;
  if ((((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)out) & 3) != 0) return hipErrorInvalidValue;      // not even float-aligned
  // float4 body only where the three tensors sit at the same distance from a 16-byte boundary (then they do so in every sample)
  const int aligned = mis_of(x0) == mis_of(noise) && mis_of(x0) == mis_of(out);
  const long per = (n / 4 + QS_THREADS - 1) / QS_THREADS;
  const int chunks = (int)(per < 1 ? 1 : (per > QS_MAX_CHUNKS ? QS_MAX_CHUNKS : per));
  if ((long)B * chunks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(q_sample_kernel, dim3((unsigned)(B * chunks)), dim3(QS_THREADS), 0, s, x0, noise, t, A, S, out, B, n, T, chunks,
                     mis_of(x0), aligned);
  return hipGetLastError();
}

hipError_t launch_diffusion_loss(const float* pred, const float* target, const long long* t, const float* logvar, const float* lvlb,
                                 float* loss_simple, float* scalars, int B, long n, int T, int loss_type, float l_simple_weight,
                                 float original_elbo_weight, hipStream_t s) {
  if (B <= 0 || n <= 0 || T <= 0 || (loss_type != 0 && loss_type != 1) || !pred || !target || !t || !logvar || !lvlb || !loss_simple ||
      !scalars)
    return hipErrorInvalidValue;
  if ((((uintptr_t)pred | (uintptr_t)target) & 3) != 0) return hipErrorInvalidValue;
  // float4 loads where every sample of both tensors starts on a 16-byte boundary
  const int vec = (n % 4 == 0) && mis_of(pred) == 0 && mis_of(target) == 0;
  hipLaunchKernelGGL(diffusion_loss_sample_kernel, dim3((unsigned)B), dim3(DL_THREADS), 0, s, pred, target, t, loss_simple, n, T,
                     loss_type, vec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(diffusion_loss_means_kernel, dim3(1), dim3(64), 0, s, (const float*)loss_simple, t, logvar, lvlb, scalars, B, T,
                     l_simple_weight, original_elbo_weight);
  return hipGetLastError();
}
