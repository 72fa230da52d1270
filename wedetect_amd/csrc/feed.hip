// feed.hip — batched ragged pre-processing (include/wedetect_hip_feed.h): a whole batch of decoded uint8 HWC images of
// different sizes is resampled and padded into the tower's [B, H, W, 3] canvas in at most two launches.  The arithmetic of
// every mode restates the per-image kernels of preprocess.hip operation for operation (bit-identical output); what changes
// is the shape of the work:
//   - one launch covers all images: image = blockIdx.y, its descriptor is read through uniform (scalar) loads, so the mode
//     switch is per workgroup, never per lane;
//   - each lane produces FOUR consecutive pixels of a row = 12 bytes = three dwords, stored as one 12-byte access: a wave
//     writes 768 contiguous bytes per store instead of 3 x 64 strided bytes (HBM-bound byte work: the stores are the cost);
//   - channel order (swap_rb) is applied while packing, so no CHW round trip follows.
// No LDS, no inline asm, no scratch (build.py NO_SCRATCH).
#include "common.h"
#include "wedetect_hip_feed.h"

namespace {

constexpr int kFeedAbi = 1;
constexpr int kPrecisionBits = 32 - 8 - 2;     // Pillow's 8 bpc coefficient precision
constexpr int kPx = 4;                         // pixels per lane

__host__ __device__ __forceinline__ long long tmp_pitch(int new_w) {      // bytes, multiple of 16 (and of the 12-byte groups' need)
  return ((long long)((new_w + kPx - 1) / kPx) * (kPx * 3) + 15) / 16 * 16;
}

__device__ __forceinline__ unsigned char clip8(int v) {
  v >>= kPrecisionBits;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ unsigned char sat_round_u8(float v) {
  const int r = __float2int_rn(v);                      // cvRound: half to even
  return (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

struct alignas(4) Px4 { unsigned int d[3]; };

// 12 bytes (4 pixels x 3 channels) -> dst: one 12-byte store, or the first `n` pixels byte by byte
__device__ __forceinline__ void store_px4(unsigned char* o, const unsigned char (&px)[kPx * 3], bool vec, int n) {
  if (vec) {
    Px4 v;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      v.d[i] = (unsigned)px[4 * i] | ((unsigned)px[4 * i + 1] << 8) | ((unsigned)px[4 * i + 2] << 16) | ((unsigned)px[4 * i + 3] << 24);
    *reinterpret_cast<Px4*>(o) = v;
  } else {
#pragma unroll
    for (int i = 0; i < kPx; ++i)
      if (i < n) { o[3 * i] = px[3 * i]; o[3 * i + 1] = px[3 * i + 1]; o[3 * i + 2] = px[3 * i + 2]; }
  }
}

// ---- ragged horizontal pass of the PILLOW images: tmp[y][xx][c] = clip8(2^21 + sum_x src[y][xmin + x][c] * k[xx][x]) ----
__global__ void __launch_bounds__(256) feed_resample_h_kernel(const unsigned char* __restrict__ src, const WdFeedImage* __restrict__ images,
                                                              const int* __restrict__ tables, unsigned char* __restrict__ tmp) {
  const WdFeedImage& d = images[blockIdx.y];
  if (d.mode != WD_FEED_PILLOW) return;
  const int groups = (d.new_w + kPx - 1) / kPx;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)d.sh * groups) return;
  const int y = (int)(idx / groups), g = (int)(idx % groups);
  const int* __restrict__ bounds = tables + d.xa;
  const int* __restrict__ kk = tables + d.xidx;
  const unsigned char* __restrict__ row = src + d.src_off + (size_t)y * d.sw * 3;
  unsigned char px[kPx * 3];
#pragma unroll
  for (int i = 0; i < kPx; ++i) {
    const int xx = g * kPx + i;
    int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
    if (xx < d.new_w) {
      const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
      const int* k = kk + (size_t)xx * d.ksize_h;
      const unsigned char* p = row + (size_t)xmin * 3;
      for (int x = 0; x < n; ++x) {
        const int kv = k[x];
        s0 += p[3 * x] * kv;
        s1 += p[3 * x + 1] * kv;
        s2 += p[3 * x + 2] * kv;
      }
    }
    px[3 * i] = clip8(s0); px[3 * i + 1] = clip8(s1); px[3 * i + 2] = clip8(s2);
  }
  // tmp rows have a 16-byte pitch that holds whole groups: the padding pixels of the last group are written too
  store_px4(tmp + d.tmp_off + (size_t)y * tmp_pitch(d.new_w) + (size_t)g * (kPx * 3), px, true, kPx);
}

// ---- one resampled pixel (dy, dx) of an image, per mode; results in source channel order ----
__device__ __forceinline__ void px_copy(const WdFeedImage& d, const unsigned char* __restrict__ s0, int dy, int dx, unsigned char* r) {
  const unsigned char* s = s0 + ((size_t)dy * d.sw + dx) * 3;
  r[0] = s[0]; r[1] = s[1]; r[2] = s[2];
}

__device__ __forceinline__ void px_area_fast(const WdFeedImage& d, const unsigned char* __restrict__ src, int dy, int dx, unsigned char* r) {
#pragma clang fp contract(off)
  const int isx = d.p0, isy = d.p1;
  int s0 = 0, s1 = 0, s2 = 0;
  for (int y = 0; y < isy; ++y) {
    const unsigned char* s = src + ((size_t)(dy * isy + y) * d.sw + (size_t)dx * isx) * 3;
    for (int x = 0; x < isx; ++x) { s0 += s[3 * x]; s1 += s[3 * x + 1]; s2 += s[3 * x + 2]; }
  }
  if (isx == 2 && isy == 2) {
    r[0] = (unsigned char)((s0 + 2) >> 2); r[1] = (unsigned char)((s1 + 2) >> 2); r[2] = (unsigned char)((s2 + 2) >> 2);
  } else {
    r[0] = sat_round_u8((float)s0 * d.p2); r[1] = sat_round_u8((float)s1 * d.p2); r[2] = sat_round_u8((float)s2 * d.p2);
  }
}

// OpenCV's operation order (per source row: buf = sum_k S*alpha left to right; sum = beta*buf, then sum += beta*buf), multiply
// and add rounded separately
__device__ __forceinline__ void px_area(const WdFeedImage& d, const unsigned char* __restrict__ src, const int* __restrict__ tables,
                                        int dy, int dx, unsigned char* r) {
#pragma clang fp contract(off)
  const int* xa = tables + d.xa; const int* xidx = tables + d.xidx;
  const float* xw = reinterpret_cast<const float*>(tables) + d.xw;
  const int* ya = tables + d.ya; const int* yidx = tables + d.yidx;
  const float* yw = reinterpret_cast<const float*>(tables) + d.yw;
  const int xs = xa[2 * dx], xn = xa[2 * dx + 1];
  const int ys = ya[2 * dy], yn = ya[2 * dy + 1];
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  for (int j = 0; j < yn; ++j) {
    const unsigned char* row = src + (size_t)yidx[ys + j] * d.sw * 3;
    const float beta = yw[ys + j];
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    for (int k = 0; k < xn; ++k) {
      const unsigned char* s = row + (size_t)xidx[xs + k] * 3;
      const float al = xw[xs + k];
      b0 = b0 + (float)s[0] * al; b1 = b1 + (float)s[1] * al; b2 = b2 + (float)s[2] * al;
    }
    if (j == 0) { t0 = beta * b0; t1 = beta * b1; t2 = beta * b2; }
    else { t0 = t0 + beta * b0; t1 = t1 + beta * b1; t2 = t2 + beta * b2; }
  }
  r[0] = sat_round_u8(t0); r[1] = sat_round_u8(t1); r[2] = sat_round_u8(t2);
}

__device__ __forceinline__ void px_linear(const WdFeedImage& d, const unsigned char* __restrict__ src, const int* __restrict__ tables,
                                          int dy, int dx, unsigned char* r) {
  const int* xa = tables + d.xa; const int* xidx = tables + d.xidx;
  const int* ya = tables + d.ya; const int* yidx = tables + d.yidx;
  const int sx = xidx[dx], a0 = xa[2 * dx], a1 = xa[2 * dx + 1];
  const bool two = dx < d.p0;                            // p0 = xmax: from there on single tap * 2048
  int sy0 = yidx[dy], sy1 = sy0 + 1;
  sy0 = sy0 < 0 ? 0 : (sy0 < d.sh ? sy0 : d.sh - 1);
  sy1 = sy1 < 0 ? 0 : (sy1 < d.sh ? sy1 : d.sh - 1);
  const int b0 = ya[2 * dy], b1 = ya[2 * dy + 1];
  const unsigned char* p = src + ((size_t)sy0 * d.sw + sx) * 3;
  const unsigned char* q = src + ((size_t)sy1 * d.sw + sx) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = two ? p[c] * a0 + p[c + 3] * a1 : p[c] * 2048;
    const int h1 = two ? q[c] * a0 + q[c + 3] * a1 : q[c] * 2048;
    r[c] = (unsigned char)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
  }
}

// vertical pass of the PILLOW family over the horizontal pass's tmp
__device__ __forceinline__ void px_pillow_v(const WdFeedImage& d, const unsigned char* __restrict__ tmp, const int* __restrict__ tables,
                                            int dy, int dx, unsigned char* r) {
  const int* bounds = tables + d.ya;
  const int ymin = bounds[2 * dy], n = bounds[2 * dy + 1];
  const int* k = tables + d.yidx + (size_t)dy * d.ksize_v;
  const size_t pitch = (size_t)tmp_pitch(d.new_w);
  const unsigned char* col = tmp + d.tmp_off + (size_t)ymin * pitch + (size_t)dx * 3;
  int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
  for (int y = 0; y < n; ++y) {
    const int kv = k[y];
    const unsigned char* px = col + (size_t)y * pitch;
    s0 += px[0] * kv;
    s1 += px[1] * kv;
    s2 += px[2] * kv;
  }
  r[0] = clip8(s0); r[1] = clip8(s1); r[2] = clip8(s2);
}

// ---- canvas pass: image = blockIdx.y, lane = four pixels of one canvas row ----
template <int MODE>
__device__ __forceinline__ void feed_canvas_rows(const WdFeedImage& d, const unsigned char* __restrict__ src,
                                                 const int* __restrict__ tables, const unsigned char* __restrict__ tmp,
                                                 unsigned char* __restrict__ dst, int dst_h, int dst_w, bool vec) {
  const int groups = (dst_w + kPx - 1) / kPx;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)dst_h * groups) return;
  const int Y = (int)(idx / groups), g = (int)(idx % groups);
  const int dy = Y - d.top;
  const bool row_in = (unsigned)dy < (unsigned)d.new_h;
  const unsigned char* s = src + d.src_off;
  const unsigned char f0 = (unsigned char)(d.fill & 255), f1 = (unsigned char)((d.fill >> 8) & 255), f2 = (unsigned char)((d.fill >> 16) & 255);
  unsigned char px[kPx * 3];
#pragma unroll
  for (int i = 0; i < kPx; ++i) {
    const int dx = g * kPx + i - d.left;
    if (!row_in || (unsigned)dx >= (unsigned)d.new_w) {
      px[3 * i] = f0; px[3 * i + 1] = f1; px[3 * i + 2] = f2;
      continue;
    }
    unsigned char r[3];
    if (MODE == WD_CVRESIZE_COPY) px_copy(d, s, dy, dx, r);
    else if (MODE == WD_CVRESIZE_AREA_FAST) px_area_fast(d, s, dy, dx, r);
    else if (MODE == WD_CVRESIZE_AREA) px_area(d, s, tables, dy, dx, r);
    else if (MODE == WD_CVRESIZE_LINEAR) px_linear(d, s, tables, dy, dx, r);
    else px_pillow_v(d, tmp, tables, dy, dx, r);
    if (d.swap_rb) { px[3 * i] = r[2]; px[3 * i + 1] = r[1]; px[3 * i + 2] = r[0]; }
    else { px[3 * i] = r[0]; px[3 * i + 1] = r[1]; px[3 * i + 2] = r[2]; }
  }
  const int left_px = dst_w - g * kPx;                   // pixels of this group inside the row (< 4 only when dst_w % 4 != 0)
  unsigned char* o = dst + ((size_t)blockIdx.y * dst_h * dst_w + (size_t)Y * dst_w + (size_t)g * kPx) * 3;
  store_px4(o, px, vec, left_px < kPx ? left_px : kPx);
}

__global__ void __launch_bounds__(256) feed_canvas_kernel(const unsigned char* __restrict__ src, const WdFeedImage* __restrict__ images,
                                                          const int* __restrict__ tables, const unsigned char* __restrict__ tmp,
                                                          unsigned char* __restrict__ dst, int dst_h, int dst_w, int vec) {
  const WdFeedImage& d = images[blockIdx.y];
  switch (d.mode) {                                      // uniform per workgroup
    case WD_CVRESIZE_COPY: feed_canvas_rows<WD_CVRESIZE_COPY>(d, src, tables, tmp, dst, dst_h, dst_w, vec != 0); break;
    case WD_CVRESIZE_AREA_FAST: feed_canvas_rows<WD_CVRESIZE_AREA_FAST>(d, src, tables, tmp, dst, dst_h, dst_w, vec != 0); break;
    case WD_CVRESIZE_AREA: feed_canvas_rows<WD_CVRESIZE_AREA>(d, src, tables, tmp, dst, dst_h, dst_w, vec != 0); break;
    case WD_CVRESIZE_LINEAR: feed_canvas_rows<WD_CVRESIZE_LINEAR>(d, src, tables, tmp, dst, dst_h, dst_w, vec != 0); break;
    default: feed_canvas_rows<WD_FEED_PILLOW>(d, src, tables, tmp, dst, dst_h, dst_w, vec != 0); break;
  }
}

// a table of `len` elements at element offset `off` lies inside the arena
inline bool table_ok(int32_t off, long long len, int64_t table_elems) {
  return off >= 0 && len >= 0 && (long long)off + len <= (long long)table_elems;
}

}  // namespace

extern "C" int wd_feed_abi_version(void) { return kFeedAbi; }

extern "C" int32_t wd_feed_sizeof_image(void) { return (int32_t)sizeof(WdFeedImage); }

extern "C" int64_t wd_feed_tmp_bytes(int32_t sh, int32_t new_w) {
  if (sh <= 0 || new_w <= 0) return 0;
  return ((long long)sh * tmp_pitch(new_w) + 255) / 256 * 256;
}

extern "C" int wd_feed_batch_u8(const uint8_t* src, int64_t src_bytes, const WdFeedImage* images, const WdFeedImage* images_host,
                                int32_t batch, const void* tables, int64_t table_elems, uint8_t* tmp, int64_t tmp_bytes,
                                uint8_t* dst, int32_t dst_h, int32_t dst_w, void* stream) {
  if (!src || !images || !images_host || !dst || batch <= 0 || batch > 65535 || dst_h <= 0 || dst_w <= 0 || src_bytes <= 0)
    return WD_ERR_BAD_ARG;
  if (table_elems < 0 || tmp_bytes < 0 || (!tables && table_elems) || (!tmp && tmp_bytes)) return WD_ERR_BAD_ARG;
  if (tables && (reinterpret_cast<uintptr_t>(tables) & 3u)) return WD_ERR_BAD_ARG;
  long long h_work = 0;                                  // lanes of the largest PILLOW image's horizontal pass
  for (int b = 0; b < batch; ++b) {
    const WdFeedImage& d = images_host[b];
    if (d.sh <= 0 || d.sw <= 0 || d.new_h <= 0 || d.new_w <= 0) return WD_ERR_BAD_ARG;
    if (d.left < 0 || d.top < 0 || (long long)d.left + d.new_w > dst_w || (long long)d.top + d.new_h > dst_h) return WD_ERR_BAD_ARG;
    if (d.fill < 0 || d.fill > 0xffffff) return WD_ERR_BAD_ARG;
    if (d.src_off < 0 || d.src_off + (long long)d.sh * d.sw * 3 > src_bytes) return WD_ERR_BAD_ARG;
    switch (d.mode) {
      case WD_CVRESIZE_COPY:
        if (d.new_h != d.sh || d.new_w != d.sw) return WD_ERR_BAD_ARG;
        break;
      case WD_CVRESIZE_AREA_FAST:
        if (d.p0 < 1 || d.p1 < 1 || (long long)d.new_w * d.p0 > d.sw || (long long)d.new_h * d.p1 > d.sh) return WD_ERR_BAD_ARG;
        break;
      case WD_CVRESIZE_AREA:                             // tap arrays: their length is what the ranges in xa / ya name
        if (!table_ok(d.xa, 2LL * d.new_w, table_elems) || !table_ok(d.ya, 2LL * d.new_h, table_elems) ||
            !table_ok(d.xidx, 1, table_elems) || !table_ok(d.xw, 1, table_elems) || !table_ok(d.yidx, 1, table_elems) ||
            !table_ok(d.yw, 1, table_elems))
          return WD_ERR_BAD_ARG;
        break;
      case WD_CVRESIZE_LINEAR:
        if (!table_ok(d.xa, 2LL * d.new_w, table_elems) || !table_ok(d.ya, 2LL * d.new_h, table_elems) ||
            !table_ok(d.xidx, d.new_w, table_elems) || !table_ok(d.yidx, d.new_h, table_elems) || d.p0 < 0 || d.p0 > d.new_w)
          return WD_ERR_BAD_ARG;
        break;
      case WD_FEED_PILLOW: {
        if (d.ksize_h <= 0 || d.ksize_v <= 0) return WD_ERR_BAD_ARG;
        if (!table_ok(d.xa, 2LL * d.new_w, table_elems) || !table_ok(d.ya, 2LL * d.new_h, table_elems) ||
            !table_ok(d.xidx, (long long)d.new_w * d.ksize_h, table_elems) ||
            !table_ok(d.yidx, (long long)d.new_h * d.ksize_v, table_elems))
          return WD_ERR_BAD_ARG;
        if (d.tmp_off < 0 || d.tmp_off + wd_feed_tmp_bytes(d.sh, d.new_w) > tmp_bytes || (d.tmp_off & 15)) return WD_ERR_BAD_ARG;
        const long long w = (long long)d.sh * ((d.new_w + kPx - 1) / kPx);
        h_work = w > h_work ? w : h_work;
        break;
      }
      default:
        return WD_ERR_BAD_ARG;
    }
  }
  if (h_work && (reinterpret_cast<uintptr_t>(tmp) & 15u)) return WD_ERR_BAD_ARG;
  const long long c_work = (long long)dst_h * ((dst_w + kPx - 1) / kPx);
  if (h_work > 0x7fffffffLL * 256 || c_work > 0x7fffffffLL * 256) return WD_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int* tab = static_cast<const int*>(tables);
  if (h_work)
    hipLaunchKernelGGL(feed_resample_h_kernel, dim3((unsigned)((h_work + 255) / 256), (unsigned)batch), dim3(256), 0, st, src,
                       images, tab, tmp);
  const int vec = (dst_w % kPx == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(feed_canvas_kernel, dim3((unsigned)((c_work + 255) / 256), (unsigned)batch), dim3(256), 0, st, src, images,
                     tab, tmp, dst, dst_h, dst_w, vec);
  return wd_launch_status();
}
