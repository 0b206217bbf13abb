// CAVP spectrogram encoder (Cnn14): the kernels around the MFMA GEMMs of the audio tower, and the audio / video similarity.
// Activations are NHWC with H = time and W = mel: [B][T][n_mels][C], operand type (bf16/fp16) for GEMM inputs, fp32 for the
// second conv of every ConvBlock (the pool rounds once).  Reference semantics: inference/model/cavp_model.py:68-84
// (encode_spec), inference/model/cavp_modules.py:1440-1483 (ConvBlock), :1516-1546 (Cnn14.forward).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

// ---- spec_conv_in: input BatchNorm (per mel bin) -> zero padding -> 1 -> C1 3x3 conv -> folded bn1 -> ReLU -> operand type NHWC.
// spec is the caller's [B][NM][T] fp32: pixel (t, m) of the (B, 1, T, NM) image the reference forms by unsqueeze + permute is
// spec[b][m][t], so the permute is this address rule.  The input BN is applied BEFORE the padding: a border tap reads 0, not the BN
// shift (which is why that BN is not folded into the conv).  One block = a tile of SC_TT x SC_TM pixels; its (SC_TT+2) x (SC_TM+2)
// normalised input patch and the C1 x 9 folded weights live in LDS; every thread makes 8 channels of one pixel per pass.
constexpr int SC_TT = 32, SC_TM = 8, SC_MAXC = 256;

__global__ __launch_bounds__(256) void spec_conv_in_kernel(const float* __restrict__ spec, const float* __restrict__ g0,
                                                           const float* __restrict__ b0, const float* __restrict__ m0,
                                                           const float* __restrict__ v0, const float* __restrict__ w,
                                                           const float* __restrict__ g1, const float* __restrict__ b1,
                                                           const float* __restrict__ m1, const float* __restrict__ v1, float eps,
                                                           bf16_t* __restrict__ out, int ldo, int B, int NM, int T, int C1) {
  __shared__ float patch[SC_TM + 2][SC_TT + 2];      // [mel][time]: time is the contiguous axis of spec
  __shared__ __attribute__((aligned(16))) float wl[9][SC_MAXC];
  __shared__ __attribute__((aligned(16))) float bl[SC_MAXC];
  const int t0 = blockIdx.x * SC_TT, mm0 = blockIdx.y * SC_TM, b = blockIdx.z;
  for (int i = threadIdx.x; i < (SC_TM + 2) * (SC_TT + 2); i += 256) {
    const int pm = i / (SC_TT + 2), pt = i - pm * (SC_TT + 2);
    const int m = mm0 + pm - 1, t = t0 + pt - 1;
    float v = 0.f;
    if ((unsigned)m < (unsigned)NM && (unsigned)t < (unsigned)T) {
      const float sc = g0[m] / sqrtf(v0[m] + eps);
      v = (spec[((long)b * NM + m) * T + t] - m0[m]) * sc + b0[m];
    }
    patch[pm][pt] = v;
  }
  for (int i = threadIdx.x; i < C1; i += 256) {
    const float sc = g1[i] / sqrtf(v1[i] + eps);
#pragma unroll
    for (int k = 0; k < 9; ++k) wl[k][i] = w[i * 9 + k] * sc;      // weight [C1][1][ky = time][kx = mel]
    bl[i] = b1[i] - m1[i] * sc;
  }
  __syncthreads();
  const int C8 = C1 / 8;
  for (int e = threadIdx.x; e < SC_TT * SC_TM * C8; e += 256) {
    const int c8 = e % C8, px = e / C8;
    const int pm = px % SC_TM, pt = px / SC_TM;
    const int t = t0 + pt, m = mm0 + pm;
    if (t >= T || m >= NM) continue;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = bl[c8 * 8 + i];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float x = patch[pm + kx][pt + ky];
        const float4 wa = *reinterpret_cast<const float4*>(&wl[ky * 3 + kx][c8 * 8]);
        const float4 wb = *reinterpret_cast<const float4*>(&wl[ky * 3 + kx][c8 * 8 + 4]);
        acc[0] = fmaf(x, wa.x, acc[0]); acc[1] = fmaf(x, wa.y, acc[1]); acc[2] = fmaf(x, wa.z, acc[2]); acc[3] = fmaf(x, wa.w, acc[3]);
        acc[4] = fmaf(x, wb.x, acc[4]); acc[5] = fmaf(x, wb.y, acc[5]); acc[6] = fmaf(x, wb.z, acc[6]); acc[7] = fmaf(x, wb.w, acc[7]);
      }
    uint4 o;
    o.x = pack_bf2(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f));
    o.y = pack_bf2(fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
    o.z = pack_bf2(fmaxf(acc[4], 0.f), fmaxf(acc[5], 0.f));
    o.w = pack_bf2(fmaxf(acc[6], 0.f), fmaxf(acc[7], 0.f));
    *reinterpret_cast<uint4*>(out + (((long)b * T + t) * NM + m) * ldo + c8 * 8) = o;
  }
}

// ---- avgpool_nhwc: F.avg_pool2d(kernel (PH, PW)) of fp32 NHWC [B][H][W][ldx] -> operand type [B][H/PH][W/PW][ldo]: floor semantics (a
// last odd row / column is dropped), 8 channels per thread: two 16-byte loads per input pixel, one 16-byte store.
template <int PH, int PW>
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const float* __restrict__ x, int ldx, bf16_t* __restrict__ out, int ldo,
                                                           int B, int H, int W, int C) {
  const int OH = H / PH, OW = W / PW, C8 = C / 8;
  const long total = (long)B * OH * OW * C8;
  constexpr float inv = 1.0f / (PH * PW);
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(e % C8);
    const long px = e / C8;
    const int ox = (int)(px % OW), oy = (int)((px / OW) % OH), b = (int)(px / ((long)OW * OH));
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = 0.f;
#pragma unroll
    for (int dy = 0; dy < PH; ++dy)
#pragma unroll
      for (int dx = 0; dx < PW; ++dx) {
        const float* p = x + (((long)b * H + oy * PH + dy) * W + ox * PW + dx) * ldx + c8 * 8;
        const float4 a = *reinterpret_cast<const float4*>(p);
        const float4 c = *reinterpret_cast<const float4*>(p + 4);
        s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
        s[4] += c.x; s[5] += c.y; s[6] += c.z; s[7] += c.w;
      }
    uint4 o;
    o.x = pack_bf2(s[0] * inv, s[1] * inv);
    o.y = pack_bf2(s[2] * inv, s[3] * inv);
    o.z = pack_bf2(s[4] * inv, s[5] * inv);
    o.w = pack_bf2(s[6] * inv, s[7] * inv);
    *reinterpret_cast<uint4*>(out + px * ldo + c8 * 8) = o;
  }
}

// ---- spec_head_pool: Cnn14's head in front of fc1, one pass over block 6's fp32 output x [B][T][W][ldx]:
//   m[b][t][c] = mean_w x[b][t][w][c];  out[b*T + t][c] = max(m[t-1], m[t], m[t+1]) + (m[t-1] + m[t] + m[t+1]) / 3
// max_pool1d pads with -inf (a missing neighbour does not take part), avg_pool1d pads with zeros and always divides by 3; t - 1 and
// t + 1 stay inside clip b.  4 channels per thread (one 16-byte load per pixel), operand-type rows [B*T][ldo].
__device__ __forceinline__ float4 mel_mean4(const float* __restrict__ p, int W, int ldx) {
  float4 s = *reinterpret_cast<const float4*>(p);
  for (int w = 1; w < W; ++w) {
    const float4 v = *reinterpret_cast<const float4*>(p + (long)w * ldx);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float d = (float)W;
  return make_float4(s.x / d, s.y / d, s.z / d, s.w / d);
}

__global__ __launch_bounds__(256) void spec_head_pool_kernel(const float* __restrict__ x, int ldx, bf16_t* __restrict__ out, int ldo,
                                                             int B, int T, int W, int C) {
  const int C4 = C / 4;
  const long total = (long)B * T * C4;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(e % C4);
    const long row = e / C4;                       // b * T + t
    const int t = (int)(row % T);
    const float* p = x + row * W * ldx + c4 * 4;
    const float4 m = mel_mean4(p, W, ldx);
    float4 mx = m, sm = m;
    if (t > 0) {
      const float4 a = mel_mean4(p - (long)W * ldx, W, ldx);
      mx.x = fmaxf(mx.x, a.x); mx.y = fmaxf(mx.y, a.y); mx.z = fmaxf(mx.z, a.z); mx.w = fmaxf(mx.w, a.w);
      sm.x = a.x + sm.x; sm.y = a.y + sm.y; sm.z = a.z + sm.z; sm.w = a.w + sm.w;
    }
    if (t + 1 < T) {
      const float4 a = mel_mean4(p + (long)W * ldx, W, ldx);
      mx.x = fmaxf(mx.x, a.x); mx.y = fmaxf(mx.y, a.y); mx.z = fmaxf(mx.z, a.z); mx.w = fmaxf(mx.w, a.w);
      sm.x += a.x; sm.y += a.y; sm.z += a.z; sm.w += a.w;
    }
    uint2 o;
    o.x = pack_bf2(mx.x + sm.x / 3.0f, mx.y + sm.y / 3.0f);
    o.y = pack_bf2(mx.z + sm.z / 3.0f, mx.w + sm.w / 3.0f);
    *reinterpret_cast<uint2*>(out + row * ldo + c4 * 4) = o;
  }
}

// ---- cavp_similarity: out[i][j] = scale / T * sum_t <v[i][t][:], s[j][t][:]>, fp32.  One block of SIM_WAVES wavefronts per (i, j);
// wavefront w takes the frames t = w, w + SIM_WAVES, ...: its lanes walk D in 16-byte steps, the wavefront's total comes from a DPP
// row reduction, and the block's wavefront totals are added in wavefront order by one thread: no atomics, a pure function of the input.
constexpr int SIM_WAVES = 4;

__global__ __launch_bounds__(64 * SIM_WAVES) void cavp_similarity_kernel(const float* __restrict__ v, const float* __restrict__ s,
                                                                         float* __restrict__ out, int Bs, int T, int D, float scale) {
  __shared__ float part[SIM_WAVES];
  const int i = blockIdx.y, j = blockIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float acc = 0.f;
  for (int t = wv; t < T; t += SIM_WAVES) {
    const float* a = v + ((long)i * T + t) * D;
    const float* c = s + ((long)j * T + t) * D;
    for (int d = lane * 4; d < D; d += 256) {
      const float4 x = *reinterpret_cast<const float4*>(a + d);
      const float4 y = *reinterpret_cast<const float4*>(c + d);
      acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
    }
  }
  acc = wave_sum_dpp_bcast(acc);
  if (lane == 0) part[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < SIM_WAVES; ++k) tot += part[k];
    out[(long)i * Bs + j] = tot * (scale / (float)T);
  }
}

inline unsigned grid_1d(long n, int cap = 65535) {
  const long g = (n + 255) / 256;
  return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace

hipError_t launch_spec_conv_in(const float* spec, const float* const bn0[4], const float* w, const float* const bn1[4], float eps,
                               uint16_t* out, int ldo, int B, int NM, int T, int C1, hipStream_t s) {
  if (B <= 0 || B > 65535 || NM <= 0 || T <= 0 || C1 <= 0 || C1 % 8 || C1 > SC_MAXC || ldo < C1 || ldo % 8) return hipErrorInvalidValue;
  if ((NM + SC_TM - 1) / SC_TM > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_conv_in_kernel, dim3((T + SC_TT - 1) / SC_TT, (NM + SC_TM - 1) / SC_TM, B), dim3(256), 0, s, spec, bn0[0],
                     bn0[1], bn0[2], bn0[3], w, bn1[0], bn1[1], bn1[2], bn1[3], eps, out, ldo, B, NM, T, C1);
  return hipGetLastError();
}

hipError_t launch_avgpool_nhwc(const float* x, int ldx, uint16_t* out, int ldo, int B, int H, int W, int C, int ph, int pw,
                               hipStream_t s) {
  if (B <= 0 || C <= 0 || C % 8 || ldx < C || ldx % 4 || ldo < C || ldo % 8 || pw != 2 || (ph != 1 && ph != 2) || H < ph || W < pw)
    return hipErrorInvalidValue;
  const long n = (long)B * (H / ph) * (W / pw) * (C / 8);
  if (ph == 2)
    hipLaunchKernelGGL((avgpool_nhwc_kernel<2, 2>), dim3(grid_1d(n)), dim3(256), 0, s, x, ldx, out, ldo, B, H, W, C);
  else
    hipLaunchKernelGGL((avgpool_nhwc_kernel<1, 2>), dim3(grid_1d(n)), dim3(256), 0, s, x, ldx, out, ldo, B, H, W, C);
  return hipGetLastError();
}

hipError_t launch_spec_head_pool(const float* x, int ldx, uint16_t* out, int ldo, int B, int T, int W, int C, hipStream_t s) {
  if (B <= 0 || T <= 0 || W <= 0 || C <= 0 || C % 4 || ldx < C || ldx % 4 || ldo < C || ldo % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_head_pool_kernel, dim3(grid_1d((long)B * T * (C / 4))), dim3(256), 0, s, x, ldx, out, ldo, B, T, W, C);
  return hipGetLastError();
}

hipError_t launch_cavp_similarity(const float* v, const float* sf, float* out, int Bv, int Bs, int T, int D, float scale, hipStream_t s) {
  if (Bv <= 0 || Bv > 65535 || Bs <= 0 || T <= 0 || D <= 0 || D % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cavp_similarity_kernel, dim3(Bs, Bv), dim3(64 * SIM_WAVES), 0, s, v, sf, out, Bs, T, D, scale);
  return hipGetLastError();
}
