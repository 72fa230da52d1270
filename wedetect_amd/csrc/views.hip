// views.hip — test-time augmentation (include/wedetect_hip_views.h): flipped views of a batch in one launch, and the rows of
// all views of every image merged into one list per image on the device.
//   flip   image = blockIdx.y; each lane produces FOUR consecutive pixels of a destination row = 12 bytes.  With w % 4 == 0 a row
//          is a multiple of 12 bytes and so is every group's offset in it: source and destination groups are three aligned dwords
//          when both pointers are 4-byte aligned.  A horizontal flip reverses the four pixels of the mirrored source group (bytes
//          permuted in registers, channels in place); a vertical flip only picks another row.  Otherwise the same lanes move bytes.
//   merge  ONE workgroup per image: filter (count, label) + un-flip + 64-bit keys (~score bits << 32 | slot) straight into LDS,
//          the bitonic network of bitonic.h over the n2 <= 4096 keys (32 KB), then the candidate list wd_nms_gather reads (flat
//          index = slot * n_cls + label).  The existing NMS runs on `batch` images of n_view * max_in anchors with identity metadata
//          {0, 0, 0, 1, 1, W, H, 1}: (x - 0) / 1 is exact, so the rows that come out are the un-flipped boxes.  View v is the
//          outer loop of the key phase, so view_flip[v], counts[v, b] and img_wh[b] are uniform (scalar) loads.
// No inline asm, no scratch (build.py NO_SCRATCH).
#include "bitonic.h"
#include "common.h"
#include "wedetect_hip_views.h"

#pragma clang fp contract(off)

namespace {

constexpr int kViewsAbi = 1;
constexpr int kPx = 4;                         // pixels per lane
constexpr int VM_MAX_VIEWS = 8, VM_MAX_ROWS = 4096, VM_MAX_OUT = 1024, VM_THREADS = 256;

struct alignas(4) Px4 { unsigned int d[3]; };

__global__ void __launch_bounds__(256) flip_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h,
                                                      int w, int dir, int vec) {
  const int groups = (w + kPx - 1) / kPx;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)h * groups) return;
  const int Y = (int)(idx / groups), x = (int)(idx % groups) * kPx;
  const int sy = (dir & 2) ? h - 1 - Y : Y;
  const size_t img = (size_t)blockIdx.y * h * w * 3;
  const unsigned char* srow = src + img + (size_t)sy * w * 3;
  unsigned char* o = dst + img + ((size_t)Y * w + (size_t)x) * 3;
  if (vec) {                                             // w % 4 == 0: the group is whole, its mirror starts at pixel w - 4 - x
    const int sx = (dir & 1) ? w - kPx - x : x;
    const unsigned* q = reinterpret_cast<const unsigned*>(srow + (size_t)sx * 3);
    const unsigned q0 = q[0], q1 = q[1], q2 = q[2];      // bytes b0 .. b11 = pixels p0 p1 p2 p3
    Px4 v;
    if (dir & 1) {                                       // p3 p2 p1 p0: out byte 3i + c = b[3(3 - i) + c]
      v.d[0] = (q2 >> 8) | ((q1 & 0x00FF0000u) << 8);                                         // b9 b10 b11 b6
      v.d[1] = (q1 >> 24) | ((q2 & 255u) << 8) | ((q0 >> 24) << 16) | ((q1 & 255u) << 24);    // b7 b8 b3 b4
      v.d[2] = ((q1 >> 8) & 255u) | (q0 << 8);                                                // b5 b0 b1 b2
    } else {
      v.d[0] = q0; v.d[1] = q1; v.d[2] = q2;
    }
    *reinterpret_cast<Px4*>(o) = v;
  } else {
    const int left = w - x < kPx ? w - x : kPx;          // pixels of this group inside the row
#pragma unroll
    for (int i = 0; i < kPx; ++i)
      if (i < left) {
        const unsigned char* p = srow + (size_t)((dir & 1) ? w - 1 - (x + i) : x + i) * 3;
        const unsigned char c0 = p[0], c1 = p[1], c2 = p[2];
        o[3 * i] = c0; o[3 * i + 1] = c1; o[3 * i + 2] = c2;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
struct ViewsLayout { size_t cand_count, guard, meta, bounds, boxes, cand_idx, cand_score, total; int n, n2; };

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

ViewsLayout views_layout(int n_view, int batch, int max_in) {
  ViewsLayout L;
  L.n = n_view * max_in;
  L.n2 = 1;
  while (L.n2 < L.n) L.n2 <<= 1;
  const size_t rows = (size_t)batch * L.n;
  size_t off = 0;
  L.cand_count = off; off = align256(off + (size_t)batch * 4);      // what the NMS reads: 0 under the guard
  L.guard = off; off = align256(off + (size_t)batch * 4);           // != 0: a view of this image reported count < 0
  L.meta = off; off = align256(off + (size_t)batch * 32);           // {0, 0, 0, 1, 1, W, H, 1} per image
  L.bounds = off; off = align256(off + (size_t)wd_nms_workspace_bytes(batch));   // wd_nms_gather's own workspace
  L.boxes = off; off = align256(off + rows * 16);
  L.cand_idx = off; off = align256(off + rows * 4);
  L.cand_score = off; off = align256(off + rows * 4);
  L.total = off;
  return L;
}

// image = blockIdx.x; slot = view * max_in + row.  Every slot of [0, n) gets a box (zeros when it is no candidate: the NMS never
// reads it, the workspace holds no stale bits) and every LDS position of [0, n2) a key (~0 = not a candidate, padding of the
// power-of-two network included: sorts last, and only the first `count` positions are ever unpacked).
__global__ void __launch_bounds__(VM_THREADS) views_sort_kernel(const f32x4* __restrict__ boxes, const float* __restrict__ scores,
                                                                const int* __restrict__ labels, const int* __restrict__ counts,
                                                                const int* __restrict__ view_flip, const float* __restrict__ img_wh,
                                                                int n_view, int batch, int max_in, int n_cls, int n, int n2,
                                                                int* __restrict__ cand_count, int* __restrict__ guard,
                                                                float* __restrict__ meta, f32x4* __restrict__ out_boxes,
                                                                int* __restrict__ cand_idx, float* __restrict__ cand_score) {
#pragma clang fp contract(off)
  __shared__ unsigned long long sk[VM_MAX_ROWS];
  __shared__ unsigned s_count, s_guard;
  const int b = blockIdx.x, t = threadIdx.x;
  if (t == 0) { s_count = 0u; s_guard = 0u; }
  for (int i = n + t; i < n2; i += VM_THREADS) sk[i] = ~0ull;
  __syncthreads();
  const float W = img_wh[2 * b], H = img_wh[2 * b + 1];
  f32x4* ob = out_boxes + (size_t)b * n;
  for (int v = 0; v < n_view; ++v) {
    const int flip = view_flip[v];
    const int cnt = counts[v * batch + b];
    if (cnt < 0 && t == 0) s_guard = 1u;
    const size_t base = ((size_t)v * batch + b) * max_in;
    for (int r0 = 0; r0 < max_in; r0 += VM_THREADS) {
      const int r = r0 + t;
      bool valid = false;
      if (r < max_in) {
        f32x4 bx = {0.f, 0.f, 0.f, 0.f};
        unsigned sbits = 0u;
        if (r < cnt) {
          const int lb = labels[base + r];
          valid = lb >= 0 && lb < n_cls;
          if (valid) {
            bx = boxes[base + r];
            sbits = __float_as_uint(scores[base + r]);
            if (flip & 1) { const float x1 = W - bx[2], x2 = W - bx[0]; bx[0] = x1; bx[2] = x2; }
            if (flip & 2) { const float y1 = H - bx[3], y2 = H - bx[1]; bx[1] = y1; bx[3] = y2; }
          }
        }
        const int slot = v * max_in + r;
        ob[slot] = bx;
        sk[slot] = valid ? ((unsigned long long)(~sbits) << 32) | (unsigned long long)(unsigned)slot : ~0ull;
      }
      const unsigned long long mask = __ballot(valid);
      if ((t & 63) == 0 && mask) atomicAdd(&s_count, (unsigned)__popcll(mask));
    }
  }
  __syncthreads();
  for (int sz = 2; sz <= n2; sz <<= 1)
    for (int jj = sz >> 1; jj > 0; jj >>= 1) wd_lds_bitonic_pass<VM_THREADS>(sk, n2, 0, jj, sz);
  const int count = (int)s_count;
  int* ci = cand_idx + (size_t)b * n;
  float* cs = cand_score + (size_t)b * n;
  for (int i = t; i < n; i += VM_THREADS) {              // every entry written: -1 / 0 from the count on
    if (i < count) {
      const unsigned long long ck = sk[i];
      const int slot = (int)(unsigned)(ck & 0xFFFFFFFFull);
      const int v = slot / max_in, r = slot - v * max_in;
      ci[i] = slot * n_cls + labels[((size_t)v * batch + b) * max_in + r];
      cs[i] = __uint_as_float(~(unsigned)(ck >> 32));
    } else {
      ci[i] = -1;
      cs[i] = 0.f;
    }
  }
  if (t < 8) {
    const float m = (t == 3 || t == 4 || t == 7) ? 1.f : t == 5 ? W : t == 6 ? H : 0.f;
    meta[(size_t)b * 8 + t] = m;
  }
  if (t == 0) {
    guard[b] = (int)s_guard;
    cand_count[b] = s_guard ? 0 : count;
  }
}

__global__ void __launch_bounds__(256) views_guard_kernel(const int* __restrict__ guard, int batch, int* __restrict__ out_count) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < batch && guard[b]) out_count[b] = -1;
}

}  // namespace

extern "C" int wd_views_abi_version(void) { return kViewsAbi; }

extern "C" int wd_flip_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t direction, void* stream) {
  if (!src || !dst || n <= 0 || n > 65535 || h <= 0 || w <= 0 || direction < 1 || direction > 3) return WD_ERR_BAD_ARG;
  const unsigned long long bytes = (unsigned long long)n * (unsigned long long)h * (unsigned long long)w * 3ull;
  const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
  if (s < d + bytes && d < s + bytes) return WD_ERR_BAD_ARG;
  const long long work = (long long)h * ((w + kPx - 1) / kPx);
  if (work > 0x7fffffffLL * 256) return WD_ERR_BAD_ARG;
  const int vec = (w % kPx == 0 && ((s | d) & 3u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(flip_u8_kernel, dim3((unsigned)((work + 255) / 256), (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream),
                     src, dst, h, w, direction, vec);
  return wd_launch_status();
}

extern "C" int64_t wd_views_merge_workspace_bytes(int32_t n_view, int32_t batch, int32_t max_in) {
  if (n_view <= 0 || n_view > VM_MAX_VIEWS || batch <= 0 || batch > 65535 || max_in <= 0 || (long long)n_view * max_in > VM_MAX_ROWS)
    return 0;
  return (int64_t)views_layout(n_view, batch, max_in).total;
}

extern "C" int wd_views_merge(const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts,
                              const int32_t* view_flip, const float* img_wh, int32_t n_view, int32_t batch, int32_t max_in,
                              int32_t n_cls, float iou_thr, int32_t split_thr, int32_t max_out, float* out_boxes, float* out_scores,
                              int32_t* out_labels, int32_t* out_src, int32_t* out_count, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  if (!boxes || !scores || !labels || !counts || !view_flip || !img_wh || !out_boxes || !out_scores || !out_labels || !out_src ||
      !out_count || !workspace)
    return WD_ERR_BAD_ARG;
  if (n_view < 1 || n_view > VM_MAX_VIEWS) return WD_ERR_UNSUPPORTED;
  if (batch <= 0 || batch > 65535 || max_in <= 0 || n_cls <= 0 || max_out <= 0 || !(fabsf(iou_thr) < INFINITY)) return WD_ERR_BAD_ARG;
  if ((long long)n_view * max_in > VM_MAX_ROWS || max_out > VM_MAX_OUT || (long long)n_view * max_in * n_cls >= 0x80000000LL)
    return WD_ERR_UNSUPPORTED;
  if (!wd_aligned16(boxes) || !wd_aligned16(out_boxes) || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return WD_ERR_BAD_ARG;
  const ViewsLayout L = views_layout(n_view, batch, max_in);
  if (workspace_bytes < 0 || (size_t)workspace_bytes < L.total) return WD_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  int* cand_count = reinterpret_cast<int*>(ws + L.cand_count);
  int* guard = reinterpret_cast<int*>(ws + L.guard);
  float* meta = reinterpret_cast<float*>(ws + L.meta);
  f32x4* ub = reinterpret_cast<f32x4*>(ws + L.boxes);
  int* cand_idx = reinterpret_cast<int*>(ws + L.cand_idx);
  float* cand_score = reinterpret_cast<float*>(ws + L.cand_score);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(views_sort_kernel, dim3((unsigned)batch), dim3(VM_THREADS), 0, s, reinterpret_cast<const f32x4*>(boxes), scores,
                     labels, counts, view_flip, img_wh, n_view, batch, max_in, n_cls, L.n, L.n2, cand_count, guard, meta, ub, cand_idx,
                     cand_score);
  if (wd_launch_status() != WD_OK) return WD_ERR_LAUNCH;
  const int rc = wd_nms_gather(cand_idx, cand_score, cand_count, L.n, reinterpret_cast<const float*>(ub), L.n, n_cls, meta, iou_thr,
                               max_out, WD_NMS_MMCV, split_thr, nullptr, 0, out_boxes, out_scores, out_labels, out_src, out_count,
                               nullptr, batch, ws + L.bounds, wd_nms_workspace_bytes(batch), s);
  if (rc != WD_OK) return rc;
  hipLaunchKernelGGL(views_guard_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, guard, batch, out_count);
  return wd_launch_status();
}
