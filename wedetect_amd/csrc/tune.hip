// tune.hip — bank tuning (include/wedetect_hip_tune.h): the class bank learned from labelled boxes, towers frozen.
//   wd_tune_targets   one workgroup per image: the selected slots of wd_exemplar_assign -> per-anchor (class, IoU) targets
//   wd_tune_grad      one workgroup per (class block of 32, row split): S = E·Tᵀ tile by tile on fp32-input MFMA, sigmoid and
//                     sparse target in registers, dtᵀ += gᵀ·E into 96 accumulator registers kept for the whole sweep; the
//                     [rows, K] matrix is never written; partial sums go to slabs, in a fixed order
//   wd_tune_update    one workgroup per class row: slab sum, projection through the normalisation, Adam, renormalisation
#include "common.h"
#include "wedetect_hip_tune.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int D = WD_TUNE_DIM, CB = WD_TUNE_CLASS_BLOCK, RT = WD_TUNE_ROW_TILE;
constexpr int TLD = D + 4;                        // row stride of the t block in LDS: 772 % 64 == 4, so 16 lanes' b128 reads tile the banks
constexpr int GRAD_LDS_FLOATS = CB * TLD + RT * CB + RT * 4 + 4;
constexpr int GRAD_LDS = GRAD_LDS_FLOATS * 4;     // 96.5 KiB of t, 16 KiB of a * g, 2 KiB of row constants
constexpr int MAX_SLOTS = 64 * 8;                 // WD_EXEMPLAR_MAX_EX * WD_EXEMPLAR_MAX_M

// ------------------------------------------------------------------------------------------------------------- targets
__global__ void __launch_bounds__(256) tune_targets_kernel(const int* __restrict__ sel_anchors, const float* __restrict__ sel_iou,
                                                           const int* __restrict__ ex_cls, int max_ex, int m, int n_anchor,
                                                           int* __restrict__ pos_cls, float* __restrict__ pos_y) {
  __shared__ int s_anchor[MAX_SLOTS];
  __shared__ float s_iou[MAX_SLOTS];
  const int b = blockIdx.x, tid = threadIdx.x, slots = max_ex * m;
  const long long slot0 = (long long)b * slots, row0 = (long long)b * n_anchor;
  for (int i = tid; i < slots; i += 256) {
    const int a = sel_anchors[slot0 + i];
    s_anchor[i] = (a >= 0 && a < n_anchor) ? a : -1;
    s_iou[i] = sel_iou[slot0 + i];
  }
  for (int n = tid; n < n_anchor; n += 256) { pos_cls[row0 + n] = -1; pos_y[row0 + n] = 0.f; }
  __syncthreads();                                                 // the slots are in LDS and the image's rows hold (-1, 0)
  for (int i = tid; i < slots; i += 256) {
    const int a = s_anchor[i];
    if (a < 0) continue;
    const float iou = s_iou[i];
    bool wins = true;
    for (int j = 0; j < slots; ++j) {                              // slot against slot: at most 512 x 512 per image
      const float o = s_iou[j];
      if (j != i && s_anchor[j] == a && (o > iou || (o == iou && j < i))) wins = false;
    }
    if (wins) {                                                    // exactly one slot per claimed anchor
      pos_cls[row0 + a] = ex_cls[(long long)b * max_ex + i / m];
      pos_y[row0 + a] = iou;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- grad
__global__ void __launch_bounds__(256) tune_grad_kernel(const float* __restrict__ embed, int rows, int n_anchor, int off1, int off2,
                                                        float s0, float s1, float s2, float b0, float b1, float b2,
                                                        const int* __restrict__ pos_cls, const float* __restrict__ pos_y,
                                                        const float* __restrict__ bank, int n_cls, float inv_norm, int n_split,
                                                        float* __restrict__ slabs, float* __restrict__ loss_parts) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* tl = lds;                                                 // [CB][TLD]   the class block's unit rows
  float* gl = tl + CB * TLD;                                       // [RT][CB]    a * g of the tile in flight
  f32x4* info = reinterpret_cast<f32x4*>(gl + RT * CB);            // [RT]        a, b, class (bits), y of the tile's rows
  float* red = reinterpret_cast<float*>(info + RT);                // [4]
  const int cblk = blockIdx.x, sp = blockIdx.y, n_cblk = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
  const int k0 = cblk * CB, my_cls = k0 + col;
  const bool cls_ok = my_cls < n_cls;

  for (int i = tid; i < CB * (D / 4); i += 256) {                  // rows of classes past n_cls are zero
    const int c = i / (D / 4), q = i - c * (D / 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k0 + c < n_cls) v = *reinterpret_cast<const f32x4*>(bank + (size_t)(k0 + c) * D + q * 4);
    *reinterpret_cast<f32x4*>(tl + c * TLD + q * 4) = v;
  }

  const int nt = (rows + RT - 1) / RT;
  const int t_lo = (int)((long long)sp * nt / n_split), t_hi = (int)((long long)(sp + 1) * nt / n_split);
  f32x16 acc[6];
#pragma unroll
  for (int u = 0; u < 6; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
  float loss = 0.f;

  for (int t = t_lo; t < t_hi; ++t) {                              // block-uniform control flow throughout
    const int r0 = t * RT;
    if (tid < RT) {                                                // the previous tile's readers of info are past its second barrier
      const int r = r0 + tid;
      f32x4 v = {0.f, 0.f, __int_as_float(-1), 0.f};               // past the last row: masked below
      if (r < rows) {
        const int a = r % n_anchor, l = (a >= off1) + (a >= off2);
        v[0] = l == 0 ? s0 : (l == 1 ? s1 : s2);
        v[1] = l == 0 ? b0 : (l == 1 ? b1 : b2);
        v[2] = __int_as_float(pos_cls[r]);
        v[3] = pos_y[r];
      }
      info[tid] = v;
    }
    __syncthreads();

    // S[row][class] of this wave's 32 rows: the row on the A lane, the class on the B lane, both operands 8 consecutive
    // dimensions per lane half and chunk of 16 (k order within a chunk: j, 8 + j).  Chunk c goes to accumulator c % 8, so an
    // element is eight fmaf chains of 96 terms joined by one fixed tree: an eighth of the chain length of a single accumulator,
    // and eight independent MFMA chains in flight — the same order for every class and row
    f32x16 sa[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[u][r] = 0.f;
    {
      // a row past the last one reads the last row instead: its S is discarded below.  The 16 loads of the next eight chunks are
      // issued before the 64 MFMAs of the current eight (one wave per SIMD: nothing else hides the latency)
      const int rr = r0 + 32 * wave + col;
      const float* ep = embed + (size_t)(rr < rows ? rr : rows - 1) * D + 8 * h;
      const float* tp = tl + col * TLD + 8 * h;
      f32x4 cur[16], nxt[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) cur[u] = *reinterpret_cast<const f32x4*>(ep + 16 * (u >> 1) + 4 * (u & 1));
#pragma unroll
      for (int c8 = 0; c8 < D / 16; c8 += 8) {
        if (c8 + 8 < D / 16) {
#pragma unroll
          for (int u = 0; u < 16; ++u) nxt[u] = *reinterpret_cast<const f32x4*>(ep + 16 * (c8 + 8 + (u >> 1)) + 4 * (u & 1));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int c = c8 + u;
          const f32x4 e0 = cur[2 * u], e1 = cur[2 * u + 1];
          const f32x4 t0 = *reinterpret_cast<const f32x4*>(tp + 16 * c), t1 = *reinterpret_cast<const f32x4*>(tp + 16 * c + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) sa[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(e0[j], t0[j], sa[u], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 4; ++j) sa[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(e1[j], t1[j], sa[u], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) cur[u] = nxt[u];
      }
    }
    const f32x16 s = ((sa[0] + sa[1]) + (sa[2] + sa[3])) + ((sa[4] + sa[5]) + (sa[6] + sa[7]));
    // scale, bias, sigmoid, the sparse target: register r of the tile is row (r & 3) + 8 (r >> 2) + 4 h, the lane's class
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
      const f32x4 v = info[lr];
      const int pc = __float_as_int(v[2]);
      const bool valid = cls_ok && r0 + lr < rows;
      const float y = pc == my_cls ? v[3] : 0.f;
      const float z = v[0] * s[r] + v[1];
      const float e = expf(-fabsf(z));
      const float inv = 1.0f / (1.0f + e);
      const float p = z >= 0.f ? inv : e * inv;                    // overflow-free in both halves
      const float bce = fmaxf(z, 0.f) - z * y + log1pf(e);
      loss += valid ? bce : 0.f;
      gl[lr * CB + col] = valid ? (p - y) * inv_norm * v[0] : 0.f;
    }
    __syncthreads();

    // dt[class][d] += sum over the tile's rows of (a g)[row][class] * E[row][d]: the class on the A lane, two rows per step;
    // this wave owns d in [192 wave, 192 wave + 192): tile 2 u + e holds d = 192 wave + 64 u + 2 col + e
    // (a row past the last one reads the last row: its g is zero.)  Eight steps' loads are issued before the previous eight's MFMAs
    {
      const float* eb = embed + 192 * wave + 2 * col;
      const int last = rows - 1 - r0;                               // >= 0: the tile holds at least one row
      f32x2 cur[24], nxt[24];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int lr = 2 * q + h;
        const float* ep = eb + (size_t)(r0 + (lr < last ? lr : last)) * D;
#pragma unroll
        for (int u = 0; u < 3; ++u) cur[3 * q + u] = *reinterpret_cast<const f32x2*>(ep + 64 * u);
      }
#pragma unroll
      for (int k8 = 0; k8 < RT / 2; k8 += 8) {
        if (k8 + 8 < RT / 2) {
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int lr = 2 * (k8 + 8 + q) + h;
            const float* ep = eb + (size_t)(r0 + (lr < last ? lr : last)) * D;
#pragma unroll
            for (int u = 0; u < 3; ++u) nxt[3 * q + u] = *reinterpret_cast<const f32x2*>(ep + 64 * u);
          }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float g = gl[(2 * (k8 + q) + h) * CB + col];
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            acc[2 * u] = __builtin_amdgcn_mfma_f32_32x32x2f32(g, cur[3 * q + u][0], acc[2 * u], 0, 0, 0);
            acc[2 * u + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g, cur[3 * q + u][1], acc[2 * u + 1], 0, 0, 0);
          }
        }
#pragma unroll
        for (int u = 0; u < 24; ++u) cur[u] = nxt[u];
      }
    }
  }

  // the whole 32 x 768 block of the slab, padded classes (exact zeros) included
  const size_t k_pad = (size_t)n_cblk * CB;
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
      float* dst = slabs + ((size_t)sp * k_pad + k0 + i) * D + 192 * wave + 64 * u + 2 * col;
      *reinterpret_cast<f32x2*>(dst) = f32x2{acc[2 * u][r], acc[2 * u + 1][r]};
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o, 64);
  if (lane == 0) red[wave] = loss;
  __syncthreads();
  if (tid == 0) loss_parts[(size_t)sp * n_cblk + cblk] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_norm;
}

// -------------------------------------------------------------------------------------------------------------- update
// sum over the workgroup of one float per lane: butterfly inside the wave, then the four wave sums in a fixed order; every
// call of a kernel uses words of its own, so one barrier per reduction is enough
__device__ __forceinline__ float block_sum(float v, float* part, int lane, int wave) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) part[wave] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void __launch_bounds__(256) tune_update_kernel(const float* __restrict__ slabs, int n_slab, const float* __restrict__ loss_parts,
                                                          int n_loss, int n_cls, int k_pad, float* __restrict__ w, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ bank,
                                                          const unsigned char* __restrict__ trainable, float lr, float beta1, float beta2,
                                                          float eps, float bc1, float bc2, float* __restrict__ loss_out, int step,
                                                          unsigned* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ float part[4][4];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (k == 0) {                                                    // block-uniform
    float ls = 0.f;
    for (int i = tid; i < n_loss; i += 256) ls += loss_parts[i];
    ls = block_sum(ls, part[3], lane, wave);
    if (tid == 0) loss_out[step] = ls;
  }
  if (!trainable[k]) return;                                       // block-uniform: a frozen row is not touched
  float dt[3] = {0.f, 0.f, 0.f}, tk[3], wk[3];
  const size_t row = (size_t)k * D;
  for (int i = 0; i < n_slab; ++i) {                               // slab order
    const float* sl = slabs + ((size_t)i * k_pad + k) * D;
#pragma unroll
    for (int j = 0; j < 3; ++j) dt[j] += sl[tid + 256 * j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { tk[j] = bank[row + tid + 256 * j]; wk[j] = w[row + tid + 256 * j]; }
  const float dot = block_sum((dt[0] * tk[0] + dt[1] * tk[1]) + dt[2] * tk[2], part[0], lane, wave);
  const float nrm = sqrtf(block_sum((wk[0] * wk[0] + wk[1] * wk[1]) + wk[2] * wk[2], part[1], lane, wave));
  float mn[3], vn[3], wn[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float dw = (dt[j] - dot * tk[j]) / nrm;
    mn[j] = beta1 * m[row + tid + 256 * j] + (1.0f - beta1) * dw;
    vn[j] = beta2 * v[row + tid + 256 * j] + (1.0f - beta2) * (dw * dw);
    wn[j] = wk[j] - lr * (mn[j] / bc1) / (sqrtf(vn[j] / bc2) + eps);
  }
  const float nrm2 = sqrtf(block_sum((wn[0] * wn[0] + wn[1] * wn[1]) + wn[2] * wn[2], part[2], lane, wave));
  const float inf = __builtin_inff();
  const bool ok = nrm > 0.f && nrm < inf && nrm2 > 0.f && nrm2 < inf;   // a NaN fails the comparisons
  if (!ok) {
    if (tid == 0) *status = 1u;                                    // a plain store of the constant: every bad row stores the same word
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const size_t o = row + tid + 256 * j;
    w[o] = wn[j]; m[o] = mn[j]; v[o] = vn[j]; bank[o] = wn[j] / nrm2;
  }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool is_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }

}  // namespace

extern "C" int wd_tune_abi_version(void) { return 1; }

extern "C" int32_t wd_tune_plan(int64_t rows, int32_t n_cls) {
  if (rows <= 0 || n_cls <= 0) return 0;
  const int64_t nt = (rows + RT - 1) / RT;
  const int64_t n_cblk = ((int64_t)n_cls + CB - 1) / CB;
  int64_t s = WD_TUNE_MAX_SPLIT / n_cblk;                          // one workgroup per CU: 117 KiB of LDS each
  if (s < 1) s = 1;
  return (int32_t)(s < nt ? s : nt);
}

extern "C" int wd_tune_targets(const int32_t* sel_anchors, const float* sel_iou, const int32_t* ex_cls, int32_t max_ex, int32_t m,
                               int32_t batch, int32_t n_anchor, int32_t* pos_cls, float* pos_y, void* stream) {
  if (!sel_anchors || !sel_iou || !ex_cls || !pos_cls || !pos_y) return WD_ERR_BAD_ARG;
  if (batch <= 0 || n_anchor <= 0 || max_ex < 1 || max_ex > 64 || m < 1 || m > 8) return WD_ERR_BAD_ARG;
  if (!aligned4(sel_anchors) || !aligned4(sel_iou) || !aligned4(ex_cls) || !aligned4(pos_cls) || !aligned4(pos_y)) return WD_ERR_BAD_ARG;
  if (batch > 65535 || (long long)batch * n_anchor > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(tune_targets_kernel, dim3((unsigned)batch), dim3(256), 0, static_cast<hipStream_t>(stream), sel_anchors, sel_iou,
                     ex_cls, max_ex, m, n_anchor, pos_cls, pos_y);
  return wd_launch_status();
}

extern "C" int wd_tune_grad(const float* embed, int32_t rows, int32_t dim, int32_t n_anchor, int32_t off1, int32_t off2, float scale0,
                            float scale1, float scale2, float bias0, float bias1, float bias2, const int32_t* pos_cls,
                            const float* pos_y, const float* bank, int32_t n_cls, float inv_norm, int32_t n_split, float* slabs,
                            float* loss_parts, void* stream) {
  if (!embed || !pos_cls || !pos_y || !bank || !slabs || !loss_parts) return WD_ERR_BAD_ARG;
  if (dim != D || rows <= 0 || n_anchor <= 0 || n_cls <= 0 || !(0 < off1 && off1 < off2 && off2 <= n_anchor)) return WD_ERR_BAD_ARG;
  if (!is_finite(scale0) || !is_finite(scale1) || !is_finite(scale2) || !is_finite(bias0) || !is_finite(bias1) || !is_finite(bias2)) return WD_ERR_BAD_ARG;
  if (!is_finite(inv_norm) || !(inv_norm > 0.f) || n_split < 1 || n_split > WD_TUNE_MAX_SPLIT) return WD_ERR_BAD_ARG;
  if (!wd_aligned16(embed) || !wd_aligned16(bank) || !wd_aligned16(slabs) || !aligned4(pos_cls) || !aligned4(pos_y) || !aligned4(loss_parts))
    return WD_ERR_BAD_ARG;
  if ((long long)rows * D > 0x7ffffff0LL || n_cls > 65535 * CB) return WD_ERR_BAD_ARG;
  const long long n_cblk = ((long long)n_cls + CB - 1) / CB;
  if (n_split * n_cblk * CB * D >= (1LL << 40)) return WD_ERR_BAD_ARG;
  static WdAttrOnce attr;
  if (wd_set_max_lds(attr, reinterpret_cast<const void*>(tune_grad_kernel), GRAD_LDS) != WD_OK) return WD_ERR_LAUNCH;
  hipLaunchKernelGGL(tune_grad_kernel, dim3((unsigned)n_cblk, (unsigned)n_split), dim3(256), GRAD_LDS, static_cast<hipStream_t>(stream),
                     embed, rows, n_anchor, off1, off2, scale0, scale1, scale2, bias0, bias1, bias2, pos_cls, pos_y, bank, n_cls, inv_norm,
                     n_split, slabs, loss_parts);
  return wd_launch_status();
}

extern "C" int wd_tune_update(const float* slabs, int32_t n_slab, const float* loss_parts, int32_t n_cls, int32_t dim, float* w, float* m,
                              float* v, float* bank, const uint8_t* trainable, float lr, float beta1, float beta2, float eps, float bc1,
                              float bc2, float* loss_out, int32_t step, uint32_t* status, void* stream) {
  if (!slabs || !loss_parts || !w || !m || !v || !bank || !trainable || !loss_out || !status) return WD_ERR_BAD_ARG;
  if (dim != D || n_slab <= 0 || n_cls <= 0 || step < 0) return WD_ERR_BAD_ARG;
  if (!is_finite(lr) || !(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !is_finite(eps) || !(eps > 0.f))
    return WD_ERR_BAD_ARG;
  if (!(bc1 > 0.f && bc1 <= 1.f) || !(bc2 > 0.f && bc2 <= 1.f)) return WD_ERR_BAD_ARG;
  if (!wd_aligned16(slabs) || !aligned4(loss_parts) || !aligned4(w) || !aligned4(m) || !aligned4(v) || !aligned4(bank) ||
      !aligned4(loss_out) || !aligned4(status))
    return WD_ERR_BAD_ARG;
  if (n_cls > 65535 * CB) return WD_ERR_BAD_ARG;
  const long long n_cblk = ((long long)n_cls + CB - 1) / CB;
  if (n_slab * n_cblk * CB * D >= (1LL << 40) || n_slab * n_cblk > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(tune_update_kernel, dim3((unsigned)n_cls), dim3(256), 0, static_cast<hipStream_t>(stream), slabs, n_slab,
                     loss_parts, (int)(n_slab * n_cblk), n_cls, (int)(n_cblk * CB), w, m, v, bank, trainable, lr, beta1, beta2, eps, bc1,
                     bc2, loss_out, step, status);
  return wd_launch_status();
}
