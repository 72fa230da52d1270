// topn_key.h — the key merge of include/wedetect_hip_topn.h, shared by the fused epilogue (split_gemm_p8.hip: p8_topn_epilogue) and
// the row kernel (topn.hip): row r owns n_top 64-bit words, slot j ends as the (j + 1)-th largest key offered to the row.
#pragma once
#include "common.h"

// the row affine of the retrieval scripts on a raw logit: ONE function for both producers, so the same bits
__device__ __forceinline__ float wd_topn_affine_score(float logit, float escale, float bias) {
  return wd_sigmoid_fast(fmaf(logit, escale, bias));           // explicit fma, as the GEMM epilogues
}

// A lower bound of the row's last slot: slots only grow, so any value read after the step's memset is one (device scope: the
// other producers of the step run on other CUs and XCDs).
__device__ __forceinline__ unsigned long long wd_topn_bound(const unsigned long long* slot, int n_top) {
  return __hip_atomic_load(slot + (n_top - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Offers key k to a row, entering the cascade at slot `first`: a slot keeps the larger of (its value, the carry) and hands the
// smaller down.  `first` = the number of LARGER keys the same producer offers to this row in this step (its own t-th largest
// enters at slot t: a key with t larger ones is at best the (t + 1)-th of the row, so no slot above t can be its place, and the
// final slots are the same as if every key entered at slot 0 — slot j ends as the maximum of what reached it, by induction over
// j).  A carry not above `bound` (<= the last slot <= every slot) changes nothing below and is dropped.
__device__ __forceinline__ void wd_topn_offer(unsigned long long* slot, int n_top, int first, unsigned long long k,
                                              unsigned long long bound) {
  unsigned long long carry = k;
  for (int j = first; j < n_top && carry > bound; ++j) {
    const unsigned long long old = atomicMax(slot + j, carry);
    carry = old < carry ? old : carry;
  }
}
