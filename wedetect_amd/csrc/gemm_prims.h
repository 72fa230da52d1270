// gemm_prims.h — the small building blocks that every GEMM / implicit-GEMM kernel source of this library shares, each written
// once: the XCD tile remap, the LDS-DMA instruction wrappers, the fenced workgroup barrier, the activation dispatch and the
// host-side vector flags of the epilogues.  (The epilogues themselves and the store tail built from them: split_gemm_impl.h.)
#pragma once
#include "common.h"

// Workgroup b runs on XCD b % 8 (round-robin dispatch; observed, and only locality depends on it), and every XCD has its own
// L2.  Give XCD x the CONTIGUOUS tile range [start(x), start(x + 1)) instead of every eighth tile, so that neighbouring tiles —
// which share operand panels, or halo rows — meet in one L2: bijective for any grid size nwg.
__device__ __forceinline__ int wd_xcd_tile(int tile, int nwg) {
  const int xcd = tile & 7, idx = tile >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---------------------------------------------------------------------------------------
// LDS-DMA: one global_load_lds_dwordx4 = 64 lanes x 16 B from per-lane global addresses to the 1 KB of LDS at [lds_addr, + 1024)
// (lane-linear).  M0 carries the wave-uniform LDS address and is written in the SAME statement that reads it (hipcc does not
// preserve M0 around a statement).  Inline asm, not the builtin: hipcc waits vmcnt(0) for a builtin DMA before the next ds_read;
// these are retired by the kernels' own counted s_waitcnt vmcnt(N), then a barrier, then the reads.  Three instruction forms:
//
//   wd_lds_dma_sbase<false>  scalar base + 32-bit VGPR offset, s_nop 0.  The kernels whose operands fit 32-bit offsets from their
//                            bases (wd_dma32_fits: the 256 x 256 and 128 x 256 kernels, the fused block MLPs): one VGPR per lane
//                            address instead of two, the row advance is scalar arithmetic.
//   wd_lds_dma_sbase<true>   the same with s_nop 4: the persistent wide block MLP only, whose piece loop makes hipcc restore spilled
//                            SGPRs with v_readlane right in front of the statement — a VALU write of an SGPR needs 5 wait states
//                            before a VMEM instruction reads it as its base (split_gemm_mlpw.hip; every other build is held to
//                            that distance by scripts/check_sgpr_vmem_hazard.py instead).
//   wd_lds_dma_vaddr_nop     64-bit VGPR address, `off`, s_nop 0: the depthwise 7 x 7 halo loader (elementwise.hip).
//   wd_lds_dma_vaddr         64-bit VGPR address, `off`, NO nop: the ping-pong, implicit-GEMM and 3 x 3 kernels and the probe,
//                            whose lanes address rows of several operands (or the zero page) and keep full pointers.
//
// Which form takes which nop: s_mov_b32 m0 needs ONE wait state before the DMA instruction reads M0 — the s_nop 0 of the
// forms above (split_gemm_mlpw.hip; the programming guide's LDS-DMA recipe has the same s_nop 0 between the two).  The last
// form was written without it and has run so on every shipped build; it is kept as it is, character for character, because
// adding the nop changes those kernels' instruction streams.
// ---------------------------------------------------------------------------------------
template <bool SAFE = false>
__device__ __forceinline__ void wd_lds_dma_sbase(unsigned lds_addr, unsigned voff, const unsigned char* base) {
  if constexpr (SAFE)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(base) : "memory", "m0");
  else
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(base) : "memory", "m0");
}
__device__ __forceinline__ void wd_lds_dma_vaddr_nop(unsigned lds_addr, const void* src) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_addr), "v"(src) : "memory", "m0");
}
__device__ __forceinline__ void wd_lds_dma_vaddr(unsigned lds_addr, const void* src) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_addr), "v"(src) : "memory", "m0");
}

// Workgroup barrier that nothing crosses: neither the compiler's scheduler (an MFMA touches no memory and would otherwise move)
// nor its memory accesses.  The kernels that use it have retired their own LDS reads and DMAs by counted waits before it.
#define WD_WG_BARRIER()                       \
  do {                                        \
    __builtin_amdgcn_sched_barrier(0);        \
    asm volatile("" ::: "memory");            \
    __builtin_amdgcn_s_barrier();             \
    asm volatile("" ::: "memory");            \
    __builtin_amdgcn_sched_barrier(0);        \
  } while (0)

// One `switch` over the four activations: every arm defines `constexpr int ACT` and expands the statement, which names ACT as a
// template argument — on the device (epilogue templates) and on the host (launchers of kernels templated on the activation).
// A macro on purpose: a generic lambda over std::integral_constant gave the same registers and code size but moved the
// epilogues' basic blocks around.
#define WD_ACT_DISPATCH(act, ...)                                                 \
  do {                                                                            \
    switch (act) {                                                                \
      case WD_ACT_RELU: { constexpr int ACT = WD_ACT_RELU; __VA_ARGS__; } break;  \
      case WD_ACT_SILU: { constexpr int ACT = WD_ACT_SILU; __VA_ARGS__; } break;  \
      case WD_ACT_GELU: { constexpr int ACT = WD_ACT_GELU; __VA_ARGS__; } break;  \
      default: { constexpr int ACT = WD_ACT_NONE; __VA_ARGS__; } break;           \
    }                                                                             \
  } while (0)

// Host side: may the epilogue move C / the residual / the bias as 16-byte vectors?  (Kernel arguments vec_c, vec_res, vec_bias.)
// strict: the kernel also writes the 2 x 2 deconvolution scatter, whose quads stay inside one tap only when n % 16 == 0.
struct WdEpiVecFlags { int c, res, bias; };
static inline WdEpiVecFlags wd_epi_vec_flags(const WdConvGemm& p, bool strict) {
  return {(p.ldc % 4 == 0) && wd_aligned16(p.c) && (!strict || p.out_mode == WD_OUT_ROWS || (p.n % 16 == 0)),
          p.res ? ((p.ldres % 4 == 0) && wd_aligned16(p.res)) : 0, p.bias ? wd_aligned16(p.bias) : 0};
}
