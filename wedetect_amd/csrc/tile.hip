// tile.hip — tiled inference (include/wedetect_hip_tile.h): one large image cut into overlapping network-sized tiles in one
// launch, and the per-tile results merged into one list on the device.
//   cut    tile = blockIdx.y, its descriptor read through uniform (scalar) loads; each lane produces FOUR consecutive pixels
//          of a tile row = 12 bytes = three dwords, stored as one 12-byte access (as feed.hip).  A crop's source rows start at
//          arbitrary byte offsets (x0 * 3, any pitch): the 12 bytes are fetched as the four aligned dwords that hold them and
//          shifted into place — only where all four lie inside the image's bytes, byte loads otherwise (the image's first and
//          last bytes, the group that straddles the valid width).
//   merge  filter (count, border drop) + translate + 64-bit keys (~score bits << 32 | slot) in one kernel, the bitonic sort
//          of bitonic.h, an unpack into the candidate list wd_nms_gather reads (flat index = slot * n_cls + label), then the
//          existing NMS on ONE image of n_tile * max_in anchors with identity metadata {0, 0, 0, 1, 1, W, H, 1}: (x - 0) / 1
//          is exact, so the rows that come out are the translated boxes.
// No LDS in the cut, no inline asm, no scratch (build.py NO_SCRATCH).
#include "bitonic.h"
#include "common.h"
#include "wedetect_hip_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTileAbi = 1;
constexpr int kPx = 4;                         // pixels per lane
constexpr int MERGE_MAX_ROWS = 32768, MERGE_MAX_OUT = 1024;
constexpr int SORT_CHUNK = 8192;               // keys sorted per LDS visit (64 KB)

struct alignas(4) Px4 { unsigned int d[3]; };

__global__ void __launch_bounds__(256) tile_cut_kernel(const unsigned char* __restrict__ img, long long img_bytes, long long pitch,
                                                       const WdTile* __restrict__ tiles, int th, int tw, int fill, int swap_rb,
                                                       unsigned char* __restrict__ dst, int vec) {
  const WdTile& d = tiles[blockIdx.y];
  if (d.kind == WD_TILE_OVERVIEW) return;                // the caller's resize kernels own that slot
  const int groups = (tw + kPx - 1) / kPx;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)th * groups) return;
  const int Y = (int)(idx / groups), g = (int)(idx % groups);
  const int x = g * kPx;
  const unsigned f = (unsigned)fill & 255u;
  const unsigned f4 = f | f << 8 | f << 16 | f << 24;
  unsigned w3[3] = {f4, f4, f4};                         // the lane's 12 bytes
  if (d.kind == WD_TILE_CROP && Y < d.h && x < d.w) {
    const int nv = d.w - x < kPx ? d.w - x : kPx;        // valid pixels of this group
    const long long off = (long long)(d.y0 + Y) * pitch + (long long)(d.x0 + x) * 3;
    const unsigned char* p = img + off;
    const int sh = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
    const long long a = off - sh;                        // byte offset of the aligned dword that holds p[0]
    if (nv == kPx && a >= 0 && a + 16 <= img_bytes) {
      const unsigned* q = reinterpret_cast<const unsigned*>(p - sh);
      const unsigned q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      w3[0] = __builtin_amdgcn_alignbyte(q1, q0, (unsigned)sh);
      w3[1] = __builtin_amdgcn_alignbyte(q2, q1, (unsigned)sh);
      w3[2] = __builtin_amdgcn_alignbyte(q3, q2, (unsigned)sh);
    } else {
#pragma unroll
      for (int i = 0; i < kPx * 3; ++i)
        if (i < nv * 3) {
          const unsigned v = p[i];
          w3[i >> 2] = (w3[i >> 2] & ~(255u << (8 * (i & 3)))) | v << (8 * (i & 3));
        }
    }
    if (swap_rb) {                                       // bytes 3i <-> 3i + 2 of the valid pixels
      unsigned o3[3] = {w3[0], w3[1], w3[2]};
#pragma unroll
      for (int i = 0; i < kPx; ++i)
        if (i < nv) {
          const int b0 = 3 * i, b2 = 3 * i + 2;
          const unsigned v0 = (w3[b0 >> 2] >> (8 * (b0 & 3))) & 255u, v2 = (w3[b2 >> 2] >> (8 * (b2 & 3))) & 255u;
          o3[b0 >> 2] = (o3[b0 >> 2] & ~(255u << (8 * (b0 & 3)))) | v2 << (8 * (b0 & 3));
          o3[b2 >> 2] = (o3[b2 >> 2] & ~(255u << (8 * (b2 & 3)))) | v0 << (8 * (b2 & 3));
        }
      w3[0] = o3[0]; w3[1] = o3[1]; w3[2] = o3[2];
    }
  }
  unsigned char* o = dst + ((size_t)blockIdx.y * th * tw + (size_t)Y * tw + (size_t)x) * 3;
  if (vec) {
    Px4 v;
    v.d[0] = w3[0]; v.d[1] = w3[1]; v.d[2] = w3[2];
    *reinterpret_cast<Px4*>(o) = v;
  } else {
    const int left = tw - x < kPx ? tw - x : kPx;        // pixels of this group inside the row
#pragma unroll
    for (int i = 0; i < kPx * 3; ++i)
      if (i < left * 3) o[i] = (unsigned char)((w3[i >> 2] >> (8 * (i & 3))) & 255u);
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
struct MergeState {                            // 256 bytes at the head of the workspace
  unsigned count;                              // survivors of the filter
  unsigned guard;                              // != 0: a non-blank tile reported count < 0
  int cand_count;                              // what the NMS reads: 0 under the guard
  unsigned pad0;
  unsigned pad1[4];
  float meta[8];                               // {0, 0, 0, 1, 1, W, H, 1}
  unsigned pad2[48];
};
static_assert(sizeof(MergeState) == 256, "MergeState is one 256-byte block");

struct MergeLayout { size_t state, bounds, keys, boxes, cand_idx, cand_score, total; int n, n2; };

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

MergeLayout merge_layout(int n_tile, int max_in) {
  MergeLayout L;
  L.n = n_tile * max_in;
  L.n2 = 1;
  while (L.n2 < L.n) L.n2 <<= 1;
  size_t off = 0;
  L.state = off; off = align256(off + sizeof(MergeState));
  L.bounds = off; off = align256(off + (size_t)wd_nms_workspace_bytes(1));      // wd_nms_gather's own workspace (one image)
  L.keys = off; off = align256(off + (size_t)L.n2 * 8);
  L.boxes = off; off = align256(off + (size_t)L.n * 16);
  L.cand_idx = off; off = align256(off + (size_t)L.n * 4);
  L.cand_score = off; off = align256(off + (size_t)L.n * 4);
  L.total = off;
  return L;
}

__global__ void __launch_bounds__(64) merge_init_kernel(MergeState* __restrict__ st, const WdTile* __restrict__ tiles) {
  const int t = threadIdx.x;
  unsigned* w = reinterpret_cast<unsigned*>(st);
  w[t] = 0u;                                             // 64 lanes x 4 bytes: the whole block
  __syncthreads();
  if (t == 0) {
    st->meta[3] = 1.f; st->meta[4] = 1.f; st->meta[7] = 1.f;
    st->meta[5] = (float)tiles[0].img_w; st->meta[6] = (float)tiles[0].img_h;
  }
}

// slot i = tile * max_in + row: filter, translate, key.  Every slot of [0, n2) gets a key (~0 = not a candidate: sorts last)
// and every slot of [0, n) a box (zeros when it is no candidate: the NMS never reads it, the workspace holds no stale bits).
__global__ void __launch_bounds__(256) merge_keys_kernel(const f32x4* __restrict__ boxes, const float* __restrict__ scores,
                                                         const int* __restrict__ labels, const int* __restrict__ counts,
                                                         const WdTile* __restrict__ tiles, int n, int n2, int max_in, int n_cls,
                                                         float margin, MergeState* __restrict__ st,
                                                         unsigned long long* __restrict__ keys, f32x4* __restrict__ out_boxes) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n2) return;
  bool valid = false;
  f32x4 bx = {0.f, 0.f, 0.f, 0.f};
  unsigned sbits = 0;
  if (i < n) {
    const int t = i / max_in, r = i - t * max_in;
    const WdTile d = tiles[t];
    if (d.kind != WD_TILE_BLANK) {
      const int cnt = counts[t];
      if (cnt < 0 && r == 0) st->guard = 1u;             // sticky, benign race
      if (r < cnt) {
        const int lb = labels[i];
        valid = lb >= 0 && lb < n_cls;
        if (valid) {
          bx = boxes[i];
          sbits = __float_as_uint(scores[i]);
          if (d.kind == WD_TILE_CROP) {
            if (margin > 0.f) {
              const float w = (float)d.w, h = (float)d.h;
              const int m = d.interior_mask;
              if (((m & 1) && bx[0] < margin) || ((m & 2) && bx[1] < margin) || ((m & 4) && bx[2] > w - margin) ||
                  ((m & 8) && bx[3] > h - margin))
                valid = false;
            }
            const float fx = (float)d.x0, fy = (float)d.y0;
            bx[0] = bx[0] + fx; bx[1] = bx[1] + fy; bx[2] = bx[2] + fx; bx[3] = bx[3] + fy;
          }
          if (!valid) bx = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    out_boxes[i] = bx;
  }
  keys[i] = valid ? ((unsigned long long)(~sbits) << 32) | (unsigned long long)(unsigned)i : ~0ull;
  const unsigned long long mask = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&st->count, (unsigned)__popcll(mask));
}

// size == 0: full local sort of each chunk; size > chunk: the strides below a chunk of the merge of width `size`
__global__ void __launch_bounds__(1024) merge_sort_chunk_kernel(unsigned long long* __restrict__ keys, int n2, int size) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
  const int t = threadIdx.x;
  const int chunk = n2 < SORT_CHUNK ? n2 : SORT_CHUNK;
  const int base = blockIdx.x * SORT_CHUNK;
  if (base >= n2) return;
  unsigned long long* k = keys + base;
  for (int i = t; i < chunk; i += 1024) sk[i] = k[i];
  __syncthreads();
  if (size == 0) {
    for (int sz = 2; sz <= chunk; sz <<= 1)
      for (int jj = sz >> 1; jj > 0; jj >>= 1) wd_lds_bitonic_pass<1024>(sk, chunk, base, jj, sz);
  } else {
    for (int jj = chunk >> 1; jj > 0; jj >>= 1) wd_lds_bitonic_pass<1024>(sk, chunk, base, jj, size);
  }
  for (int i = t; i < chunk; i += 1024) k[i] = sk[i];
}

__global__ void __launch_bounds__(256) merge_sort_global_kernel(unsigned long long* __restrict__ keys, int n2, int size, int j) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n2) return;
  wd_global_bitonic_step(keys, i, j, size);
}

// sorted keys -> the candidate list of the NMS (every entry of [0, n) written: -1 / 0 from the count on)
__global__ void __launch_bounds__(256) merge_unpack_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ labels,
                                                           int n, int n_cls, MergeState* __restrict__ st,
                                                           int* __restrict__ cand_idx, float* __restrict__ cand_score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned count = st->count;
  if (i < n) {
    if (i < (int)count) {
      const unsigned long long ck = keys[i];
      const int slot = (int)(unsigned)(ck & 0xFFFFFFFFull);
      cand_idx[i] = slot * n_cls + labels[slot];
      cand_score[i] = __uint_as_float(~(unsigned)(ck >> 32));
    } else {
      cand_idx[i] = -1;
      cand_score[i] = 0.f;
    }
  }
  if (i == 0) st->cand_count = st->guard ? 0 : (int)count;
}

__global__ void __launch_bounds__(64) merge_guard_kernel(const MergeState* __restrict__ st, int* __restrict__ out_count) {
  if (threadIdx.x == 0 && st->guard) out_count[0] = -1;
}

}  // namespace

extern "C" int wd_tile_abi_version(void) { return kTileAbi; }

extern "C" int32_t wd_tile_sizeof_tile(void) { return (int32_t)sizeof(WdTile); }

extern "C" int wd_tile_cut_u8(const uint8_t* img, int32_t h, int32_t w, int64_t row_pitch_bytes, const WdTile* tiles,
                              const WdTile* tiles_host, int32_t n_tile, int32_t th, int32_t tw, int32_t fill, int32_t swap_rb,
                              uint8_t* dst, void* stream) {
  if (!img || !tiles || !tiles_host || !dst || n_tile <= 0 || n_tile > 65535 || h <= 0 || w <= 0 || th <= 0 || tw <= 0)
    return WD_ERR_BAD_ARG;
  if (fill < 0 || fill > 255 || row_pitch_bytes < (long long)w * 3) return WD_ERR_BAD_ARG;
  for (int t = 0; t < n_tile; ++t) {
    const WdTile& d = tiles_host[t];
    if (d.kind == WD_TILE_OVERVIEW || d.kind == WD_TILE_BLANK) continue;
    if (d.kind != WD_TILE_CROP) return WD_ERR_BAD_ARG;
    if (d.w <= 0 || d.h <= 0 || d.w > tw || d.h > th || d.x0 < 0 || d.y0 < 0 || (long long)d.x0 + d.w > w ||
        (long long)d.y0 + d.h > h)
      return WD_ERR_BAD_ARG;
  }
  const long long work = (long long)th * ((tw + kPx - 1) / kPx);
  if (work > 0x7fffffffLL * 256) return WD_ERR_BAD_ARG;
  const long long img_bytes = (long long)(h - 1) * row_pitch_bytes + (long long)w * 3;   // one past the last pixel byte
  const int vec = (tw % kPx == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(tile_cut_kernel, dim3((unsigned)((work + 255) / 256), (unsigned)n_tile), dim3(256), 0,
                     static_cast<hipStream_t>(stream), img, img_bytes, (long long)row_pitch_bytes, tiles, th, tw, fill, swap_rb, dst, vec);
  return wd_launch_status();
}

extern "C" int64_t wd_tile_merge_workspace_bytes(int32_t n_tile, int32_t max_in) {
  if (n_tile <= 0 || max_in <= 0 || (long long)n_tile * max_in > MERGE_MAX_ROWS) return 0;
  return (int64_t)merge_layout(n_tile, max_in).total;
}

extern "C" int wd_tile_merge(const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts,
                             const WdTile* tiles, int32_t n_tile, int32_t max_in, int32_t n_cls, float edge_margin, float iou_thr,
                             int32_t split_thr, int32_t max_out, float* out_boxes, float* out_scores, int32_t* out_labels,
                             int32_t* out_src, int32_t* out_count, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!boxes || !scores || !labels || !counts || !tiles || !out_boxes || !out_scores || !out_labels || !out_src || !out_count ||
      !workspace)
    return WD_ERR_BAD_ARG;
  if (n_tile <= 0 || max_in <= 0 || n_cls <= 0 || max_out <= 0 || !(edge_margin >= 0.f) || !(edge_margin < INFINITY))
    return WD_ERR_BAD_ARG;
  if ((long long)n_tile * max_in > MERGE_MAX_ROWS || max_out > MERGE_MAX_OUT ||
      (long long)n_tile * max_in * n_cls >= 0x80000000LL)
    return WD_ERR_UNSUPPORTED;
  if (!wd_aligned16(boxes) || !wd_aligned16(out_boxes) || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return WD_ERR_BAD_ARG;
  const MergeLayout L = merge_layout(n_tile, max_in);
  if ((size_t)workspace_bytes < L.total) return WD_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  MergeState* st = reinterpret_cast<MergeState*>(ws + L.state);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.keys);
  f32x4* tb = reinterpret_cast<f32x4*>(ws + L.boxes);
  int* cand_idx = reinterpret_cast<int*>(ws + L.cand_idx);
  float* cand_score = reinterpret_cast<float*>(ws + L.cand_score);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(merge_init_kernel, dim3(1), dim3(64), 0, s, st, tiles);
  hipLaunchKernelGGL(merge_keys_kernel, dim3((L.n2 + 255) / 256), dim3(256), 0, s, reinterpret_cast<const f32x4*>(boxes), scores,
                     labels, counts, tiles, L.n, L.n2, max_in, n_cls, edge_margin, st, keys, tb);
  {
    const int chunk = L.n2 < SORT_CHUNK ? L.n2 : SORT_CHUNK;
    const dim3 gch((L.n2 + SORT_CHUNK - 1) / SORT_CHUNK), gel((L.n2 + 255) / 256);
    hipLaunchKernelGGL(merge_sort_chunk_kernel, gch, dim3(1024), (size_t)chunk * 8, s, keys, L.n2, 0);
    for (int size = 2 * SORT_CHUNK; size <= L.n2; size <<= 1) {
      for (int j = size >> 1; j >= SORT_CHUNK; j >>= 1)
        hipLaunchKernelGGL(merge_sort_global_kernel, gel, dim3(256), 0, s, keys, L.n2, size, j);
      hipLaunchKernelGGL(merge_sort_chunk_kernel, gch, dim3(1024), (size_t)chunk * 8, s, keys, L.n2, size);
    }
  }
  hipLaunchKernelGGL(merge_unpack_kernel, dim3((L.n + 255) / 256), dim3(256), 0, s, keys, labels, L.n, n_cls, st, cand_idx, cand_score);
  if (wd_launch_status() != WD_OK) return WD_ERR_LAUNCH;
  const int rc = wd_nms_gather(cand_idx, cand_score, &st->cand_count, L.n, reinterpret_cast<const float*>(tb), L.n, n_cls, st->meta,
                               iou_thr, max_out, WD_NMS_MMCV, split_thr, nullptr, 0, out_boxes, out_scores, out_labels, out_src,
                               out_count, nullptr, 1, ws + L.bounds, wd_nms_workspace_bytes(1), s);
  if (rc != WD_OK) return rc;
  hipLaunchKernelGGL(merge_guard_kernel, dim3(1), dim3(64), 0, s, st, out_count);
  return wd_launch_status();
}
