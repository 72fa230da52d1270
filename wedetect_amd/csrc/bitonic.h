// Bitonic sort network pieces shared by the top-k sort (postprocess.hip) and the box-mAP sort (det_eval.hip).
// Both cut the network the same way: chunks of the array sorted / merged in LDS by one workgroup each, and the
// strides wider than a chunk as one global-memory compare-exchange launch per stride.  The element type only needs
// wd_bitonic_greater(a, b), a strict order with no equal elements (every key is unique), so the result is the
// ascending order whatever the network.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ bool wd_bitonic_greater(unsigned long long a, unsigned long long b) { return a > b; }

// one compare-exchange pass of stride jj over an LDS chunk of `chunk` elements starting at global position `base`;
// pairs of a merge of width dir_bit sort ascending where (position & dir_bit) == 0.  STEP = the workgroup size.
template <int STEP, typename T, typename P>
__device__ __forceinline__ void wd_lds_bitonic_pass(T* s, int chunk, P base, int jj, P dir_bit) {
  for (int i = threadIdx.x; i < chunk; i += STEP) {
    const int p = i ^ jj;
    if (p > i) {
      const T a = s[i], c = s[p];
      const bool up = ((base + i) & dir_bit) == 0;
      if (wd_bitonic_greater(a, c) == up) { s[i] = c; s[p] = a; }
    }
  }
  __syncthreads();
}

// the same compare-exchange on element i of a global array (stride j, merge width size)
template <typename T, typename P>
__device__ __forceinline__ void wd_global_bitonic_step(T* k, P i, P j, P size) {
  const P p = i ^ j;
  if (p > i) {
    const T a = k[i], c = k[p];
    const bool up = (i & size) == 0;
    if (wd_bitonic_greater(a, c) == up) { k[i] = c; k[p] = a; }
  }
}
