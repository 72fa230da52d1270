// similarity_grouped.hip — region x text similarity with ONE TEXT BANK PER IMAGE (wd_similarity_grouped, ABI 15).
//
//   out[b, n, c] = c < count[b] ? (sigmoid)( <embed[b, n, :], bank[b, c, :]> * seg_scale[lvl(n)] + seg_bias[lvl(n)] ) : +0.0f
//
// The reference takes the class list per image (yolo_world.py:94-96) and contracts 'bchw,bkc->bkhw' with a [B, K, 768]
// bank (yolo_world_head.py:90-108); the shared-bank launch of wd_conv_gemm has one B operand for all rows.  This kernel is
// that launch with the operand chosen per workgroup: the main loop is conv_gemm.hip's (gemm_core.h: fp32 MFMA 16x16x4,
// channels in ascending K steps), the epilogue is the `seg` expression of its SPECIAL epilogue, so a valid element has the
// bits ImageTower.similarity gives for that image with its own count[b]-row bank, whatever tile either launch runs.
//
// Tile mapping: 64 x 80 tiles of 4 waves, K step 32, pinned order — the shared path's tile for K = 80.  One 1-D grid of
// B * ceil(N / 64) * ceil(k_max / 80) workgroups, column tile fastest, then row tile, then image: a row tile belongs to one
// image (N = 8400 leaves a partial last tile of 16 rows per image, 132 tiles instead of 131.25), and at B = 32 the grid is
// 4224 workgroups per column tile — 16 per CU.  XCD renumbering as in conv_gemm.hip: an XCD walks a contiguous tile range.
//
// Ragged counts: count[b] is read on the device (a scalar LOAD; no host round trip in the step).  A column tile that lies
// wholly at or above count[b] issues no operand load, no LDS traffic and no MFMA: its threads store zeros and leave before
// the first barrier (the branch is uniform over the workgroup).  A partly valid tile reads zeros for the bank rows
// >= count[b] (gemm_mainloop's n < N guard) and masks them in the epilogue.  The filler is +0.0f by contract:
// wd_topk_candidates keeps score > thr with thr >= 0 and orders scores by bit pattern, so padding never becomes a candidate.
// All stores are vector stores from VGPRs (16 bytes where ldo and the pointer allow it, 4 bytes otherwise).
#include "gemm_prims.h"
#include "gemm_loader.h"
#include "gemm_core.h"

namespace {

struct SimGroupedArgs {
  const float* embed;      // [n_img][rows][dim]
  const float* bank;       // [n_img][k_max][dim]
  const int32_t* count;    // [n_img] or nullptr (= k_max everywhere)
  float* out;              // [n_img][rows][ldo]
  int n_img, rows, k_max, dim, ldo;
  int seg_end0, seg_end1;
  float seg_scale[3], seg_bias[3];
  int sigmoid;
  int nbm, nbn;            // row / column tiles per image
  int vec_c;               // 16-byte stores allowed (ldo % 4 == 0, out 16-byte aligned)
};

// Rows [m0, m0 + BM) of ONE image's embedding block; rows >= rows_per_img and the K tail read the zero block.
template <int A_PT, int RSTEP>
struct ImageRowLoader {
  const float* base;
  int dim;
  int row[A_PT];
  bool ok[A_PT];
  __device__ __forceinline__ void init(const float* e_img, int rows, int dim_, int m0, int r0) {
    base = e_img; dim = dim_;
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int m = m0 + r0 + i * RSTEP;
      ok[i] = m < rows;
      row[i] = ok[i] ? m : 0;
    }
  }
  template <int BKS>
  __device__ __forceinline__ void load(int kbase, int kc4, f32x4 (&reg)[A_PT]) const {
    const int k = kbase + kc4;
    const bool kok = k < dim;
#pragma unroll
    for (int i = 0; i < A_PT; ++i)
      reg[i] = *reinterpret_cast<const f32x4*>((ok[i] && kok) ? base + (size_t)row[i] * dim + k : g_zero4);
  }
};

template <int TM, int TN, int WM, int WN, int BKT, int VAR>
__global__ void __launch_bounds__(64 * WM * WN, 5) similarity_grouped_kernel(const SimGroupedArgs a) {
  using T = Tile<TM, TN, WM, WN, BKT>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tile = (VAR & VAR_XCD) ? wd_xcd_tile(blockIdx.x, gridDim.x) : blockIdx.x;
  const int bn = tile % a.nbn;
  const int rest = tile / a.nbn;
  const int bm = rest % a.nbm, img = rest / a.nbm;      // img < n_img: the grid is exactly n_img * nbm * nbn workgroups
  const int m0 = bm * T::BM, n0 = bn * T::BN;
  int cnt = a.count ? a.count[img] : a.k_max;
  cnt = cnt < 0 ? 0 : cnt > a.k_max ? a.k_max : cnt;    // never read a bank row or write a column outside [0, k_max)
  float* outb = a.out + (size_t)img * a.rows * a.ldo;

  if (n0 >= cnt) {
    // a column tile without a valid class: zero fill only (rows < rows_per_img, columns < k_max)
    constexpr int C4 = T::BN / 4;
    for (int idx = t; idx < T::BM * C4; idx += T::NT) {
      const int m = m0 + idx / C4, n = n0 + 4 * (idx % C4);
      if (m >= a.rows || n >= a.k_max) continue;
      float* cp = outb + (size_t)m * a.ldo + n;
      if (a.vec_c && n + 3 < a.k_max) {
        *reinterpret_cast<f32x4*>(cp) = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n + r < a.k_max) cp[r] = 0.0f;
      }
    }
    return;
  }

  ImageRowLoader<T::A_PT, T::RSTEP> al;
  al.init(a.embed + (size_t)img * a.rows * a.dim, a.rows, a.dim, m0, t / T::KCH);
  f32x4 acc[TM][TN];
  gemm_mainloop<T, TM, TN, WN, VAR>(al, a.bank + (size_t)img * a.k_max * a.dim, n0, cnt, a.dim, acc, smem, [] {});

  // ---- epilogue: conv_gemm.hip's SPECIAL epilogue with seg_rows = rows_per_img, no bias / residual / activation
  // (the same expression, term for term: v + 0, * scale + bias, fast sigmoid), columns >= count[b] replaced by +0
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int m = m0 + (wm * TM + tm) * 16 + (lane & 15);
    if (m >= a.rows) continue;
    const int lvl = (m >= a.seg_end0) + (m >= a.seg_end1);
    const float oscale = lvl == 0 ? a.seg_scale[0] : lvl == 1 ? a.seg_scale[1] : a.seg_scale[2];
    const float obias = lvl == 0 ? a.seg_bias[0] : lvl == 1 ? a.seg_bias[1] : a.seg_bias[2];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int n = n0 + (wn * TN + tn) * 16 + 4 * (lane >> 4);
      if (n >= a.k_max) continue;
      const f32x4 v = acc[tm][tn];
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = v[r] + 0.0f;
        x = x * oscale + obias;
        if (a.sigmoid) x = wd_sigmoid_fast(x);
        o[r] = (n + r < cnt) ? x : 0.0f;
      }
      float* cp = outb + (size_t)m * a.ldo + n;
      if (a.vec_c && n + 3 < a.k_max) {
        *reinterpret_cast<f32x4*>(cp) = f32x4{o[0], o[1], o[2], o[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n + r < a.k_max) cp[r] = o[r];
      }
    }
  }
}

}  // namespace

extern "C" int wd_similarity_grouped(const float* embed, const float* bank, const int32_t* count, float* out, int32_t n_img,
                                     int32_t rows_per_img, int32_t k_max, int32_t dim, int32_t ldo, int32_t seg_end0,
                                     int32_t seg_end1, const float* seg_scale, const float* seg_bias, int32_t sigmoid,
                                     void* stream) {
  constexpr int TM = 1, TN = 5, WM = 4, WN = 1, BKT = 32, VAR = VAR_XCD | VAR_PIN;     // 64 x 80 x 32, 4 waves
  using T = Tile<TM, TN, WM, WN, BKT>;
  if (!embed || !bank || !out || !seg_scale || !seg_bias) return WD_ERR_BAD_ARG;
  if (n_img <= 0 || rows_per_img <= 0 || k_max <= 0 || dim <= 0 || dim % 4 || ldo < k_max) return WD_ERR_BAD_ARG;
  if (!(0 <= seg_end0 && seg_end0 <= seg_end1 && seg_end1 <= rows_per_img)) return WD_ERR_BAD_ARG;
  if (!wd_aligned16(embed) || !wd_aligned16(bank)) return WD_ERR_BAD_ARG;
  SimGroupedArgs a{};
  a.embed = embed; a.bank = bank; a.count = count; a.out = out;
  a.n_img = n_img; a.rows = rows_per_img; a.k_max = k_max; a.dim = dim; a.ldo = ldo;
  a.seg_end0 = seg_end0; a.seg_end1 = seg_end1;
  for (int i = 0; i < 3; ++i) { a.seg_scale[i] = seg_scale[i]; a.seg_bias[i] = seg_bias[i]; }
  a.sigmoid = sigmoid ? 1 : 0;
  a.nbm = (rows_per_img + T::BM - 1) / T::BM;
  a.nbn = (k_max + T::BN - 1) / T::BN;
  a.vec_c = (ldo % 4 == 0) && wd_aligned16(out);
  const long long nblk = (long long)n_img * a.nbm * a.nbn;
  if (nblk > 0x7fffffffLL) return WD_ERR_BAD_ARG;
  auto k = similarity_grouped_kernel<TM, TN, WM, WN, BKT, VAR>;
  static WdAttrOnce attr;
  if (wd_set_max_lds(attr, reinterpret_cast<const void*>(k), T::LDS_BYTES) != WD_OK) return WD_ERR_LAUNCH;
  WD_LAUNCH_GEMM(k, dim3((unsigned)nblk), dim3(T::NT), T::LDS_BYTES, static_cast<hipStream_t>(stream), a);
  return wd_launch_status();
}
