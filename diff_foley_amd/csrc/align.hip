// Align-Acc verdict (evaluation/align_acc.py:85-86): pred = torch.round(prob), correct += #(pred == label), total += B -- one launch,
// counters that stay on the device between the batches of a dataset loop.
#include "kernels.h"

namespace {
// One block of 256 threads (four wavefronts).  pred[b] = prob[b] rounded half to even (rintf under the default rounding mode is
// v_rndne_f32: 0.5 -> 0, 1.5 -> 2, what torch.round computes); a NaN probability equals no label.  The matches are summed inside each
// wavefront by shuffles, the four partial sums meet in LDS, and thread 0 alone reads, adds to and writes the two counters: no
// atomics, and the accumulation over calls is ordered by the stream the launches share.
__global__ __launch_bounds__(256) void align_verdict_kernel(const float* __restrict__ prob, const float* __restrict__ labels,
                                                            float* __restrict__ pred, long long* __restrict__ counts, int B) {
  __shared__ int part[4];
  int hit = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float r = rintf(prob[b]);
    pred[b] = r;
    hit += (r == (labels ? labels[b] : 1.0f)) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) hit += __shfl_down(hit, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = hit;
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] = counts[0] + (long long)(part[0] + part[1] + part[2] + part[3]);
    counts[1] = counts[1] + (long long)B;
  }
}
}  // namespace

hipError_t launch_align_verdict(const float* prob, const float* labels, float* pred, long long* counts, int B, hipStream_t s) {
  if (B <= 0 || !prob || !pred || !counts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(align_verdict_kernel, dim3(1), dim3(256), 0, s, prob, labels, pred, counts, B);
  return hipGetLastError();
}
