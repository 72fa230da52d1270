// track_walk.h — the BODY of a tracker step kernel, included as text between the braces of track_step_kernel<NC> (track.hip) and
// of track_step_optimal_kernel<NC> (assign.hip): one walk for both, and — unlike a function template the kernels would call, which
// hipcc schedules differently — the greedy kernel's instructions stay exactly what they were.  Not a header in its own right.
//
// The includer provides, after track_frame.h:
//   the kernel's parameters under these names: state, workspace, boxes, scores, labels, count, embed, n_frame, max_out,
//       max_tracks, dim, P (StepParams), track_ids, track_hits;  NC as a template parameter
//   WD_TRACK_SHARED   the type of the kernel's LDS object ``sh``: Shared, or a struct derived from it
//   WD_TRACK_ASSOCIATE(cand, rows, n_rows, round, thr)   a statement run by all 256 lanes with block-uniform arguments, after a
//       barrier: cand[j * sh.n_live + i] is the value of row rows[j] with live slot sh.live[i], 0 = no candidate, a candidate is
//       >= thr > 0.  For every pair (i, j) it takes it sets sh.match[sh.live[i]] = rows[j] | round << 16 and
//       sh.row_slot[rows[j]] = sh.live[i] + 1.  It sees tid, lane, wave and flip (which of the two sh.part sets block_max_key
//       uses next) and may return without a barrier: the walk places one before it reads the matches.
#pragma clang fp contract(off)
  __shared__ WD_TRACK_SHARED sh;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Layout L{max_tracks, dim};
  float* st = state + (long long)s * L.words();
  int* sti = reinterpret_cast<int*>(st);
  float* temb = st + L.embed();                                    // [max_tracks][dim], read and written between barriers
  float* ws = workspace + (long long)s * max_tracks * max_out;
  int flip = 0;

  // the slots' scalars into LDS; lanes past max_tracks hold free slots
  {
    const bool in = tid < max_tracks;
    sh.id[tid] = in ? sti[L.id() + tid] : 0;
    sh.label[tid] = in ? sti[L.label() + tid] : 0;
    sh.score[tid] = in ? st[L.score() + tid] : 0.f;
    sh.hits[tid] = in ? sti[L.hits() + tid] : 0;
    sh.miss[tid] = in ? sti[L.miss() + tid] : 0;
    sh.has[tid] = in ? sti[L.has() + tid] : 0;
    f32x4 bx = {0.f, 0.f, 0.f, 0.f}, vl = {0.f, 0.f, 0.f, 0.f};
    if (in) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { bx[k] = st[L.box() + tid * 4 + k]; vl[k] = st[L.vel() + tid * 4 + k]; }
    }
    sh.box[tid] = bx;
    sh.vel[tid] = vl;
    if (tid == 0) { sh.next_id = sti[0]; sh.status = sti[1]; }
  }
  __syncthreads();

  for (int f = 0; f < n_frame; ++f) {
    const long long b = (long long)s * n_frame + f;
    int cnt = count[b];                                            // uniform
    if (cnt < 0) {
      if (tid == 0) sh.status |= WD_TRACK_STATUS_BAD_COUNT;
      cnt = 0;
    }
    cnt = cnt > max_out ? max_out : cnt;
    const f32x4* fbox = reinterpret_cast<const f32x4*>(boxes) + b * max_out;
    const float* fscore = scores + b * max_out;
    const int* flabel = labels + b * max_out;
    const float* fembed = embed + b * max_out * dim;

    // ---- predict; the live slots and the two row lists, each ascending (ballot + prefix)
    {
      const bool lv = sh.id[tid] > 0;
      if (lv) sh.pred[tid] = sh.box[tid] + sh.vel[tid];
      sh.match[tid] = -1;
      const u64 m = __ballot(lv);
      if (lane == 0) sh.wcnt[0][wave] = __popcll(m);
      __syncthreads();
      int off = 0;
      for (int w = 0; w < wave; ++w) off += sh.wcnt[0][w];
      if (lv) sh.live[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)tid;
      if (tid == 0) { sh.n_live = sh.wcnt[0][0] + sh.wcnt[0][1] + sh.wcnt[0][2] + sh.wcnt[0][3]; sh.n_born = 0; }
      int n_hi = 0, n_lo = 0;
      for (int r0 = 0; r0 < cnt; r0 += 256) {                      // uniform trip count
        const int r = r0 + tid;
        const float sc = r < cnt ? fscore[r] : -1.f;
        const bool hi = r < cnt && sc >= P.high_thr, lo = r < cnt && sc >= P.low_thr && sc < P.high_thr;
        if (r < cnt) { sh.row_slot[r] = 0; sh.starts[r] = sc >= P.new_thr; }
        const u64 mh = __ballot(hi), ml = __ballot(lo);
        if (lane == 0) { sh.wcnt[1][wave] = __popcll(mh); sh.wcnt[2][wave] = __popcll(ml); }
        __syncthreads();
        int oh = n_hi, ol = n_lo;
        for (int w = 0; w < wave; ++w) { oh += sh.wcnt[1][w]; ol += sh.wcnt[2][w]; }
        if (hi) sh.hi_rows[oh + __popcll(mh & ((1ull << lane) - 1ull))] = (unsigned short)r;
        if (lo) sh.lo_rows[ol + __popcll(ml & ((1ull << lane) - 1ull))] = (unsigned short)r;
        n_hi += sh.wcnt[1][0] + sh.wcnt[1][1] + sh.wcnt[1][2] + sh.wcnt[1][3];
        n_lo += sh.wcnt[2][0] + sh.wcnt[2][1] + sh.wcnt[2][2] + sh.wcnt[2][3];
        __syncthreads();
      }
      if (tid == 0) { sh.n_hi = n_hi; sh.n_lo = n_lo; }
      __syncthreads();
    }
    const int n_live = sh.n_live, n_hi = sh.n_hi, n_lo = sh.n_lo;

    // ---- round 1: the high-score rows against all live slots
    {
      float* cand = n_live * n_hi <= TILE ? sh.tile : ws;
      // appearance: cand[j * n_live + i] = max(cos, 0) of row j with live slot i.  A wave holds TWO rows in registers and
      // streams the slots past them eight at a time: 24 loads of 16 bytes in flight per lane, sixteen independent sums
      for (int j0 = wave * 2; j0 < n_hi; j0 += 8) {
        const bool two = j0 + 1 < n_hi;                            // wave-uniform
        const int r0 = sh.hi_rows[j0], r1 = sh.hi_rows[two ? j0 + 1 : j0];
        f32x4 e0[NC], e1[NC];
        load_row<NC>(e0, fembed + (long long)r0 * dim, dim, lane);
        load_row<NC>(e1, fembed + (long long)r1 * dim, dim, lane);
        const float ss0 = tree_dot<NC>(e0, e0), ss1 = tree_dot<NC>(e1, e1);
        const bool ok0 = usable_norm(ss0), ok1 = usable_norm(ss1);
        const float inv0 = ok0 ? 1.0f / sqrtf(ss0) : 0.f, inv1 = ok1 ? 1.0f / sqrtf(ss1) : 0.f;
        if (lane == 0) { sh.inv_e[r0] = inv0; sh.inv_e[r1] = inv1; }
        for (int i0 = 0; i0 < n_live; i0 += 8) {
          int t[8];
          f32x4 tv[8][NC];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            t[u] = sh.live[i0 + u < n_live ? i0 + u : n_live - 1];
            load_row<NC>(tv[u], temb + (long long)t[u] * dim, dim, lane);   // read whether the slot has one or not: inside the state
          }
          float mine = 0.f;                                        // lane u keeps row 0's value of slot i0 + u, lane 8 + u row 1's
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const bool has = sh.has[t[u]] != 0;
            const float c0 = tree_dot<NC>(tv[u], e0) * inv0, c1 = tree_dot<NC>(tv[u], e1) * inv1;
            const float v0 = (ok0 && has) ? fmaxf(c0, 0.f) : 0.f, v1 = (ok1 && has) ? fmaxf(c1, 0.f) : 0.f;
            mine = lane == u ? v0 : (lane == 8 + u ? v1 : mine);
          }
          const int u = lane & 7;
          if (lane < 16 && i0 + u < n_live && (lane < 8 || two)) cand[(long long)(j0 + (lane >> 3)) * n_live + i0 + u] = mine;
        }
      }
      __syncthreads();
      // sim = w_iou * iou + w_app * max(cos, 0), one pair per lane; 0 where the pair is no candidate
#pragma unroll 2
      for (int idx = tid; idx < n_live * n_hi; idx += 256) {
        const int i = idx % n_live, j = idx / n_live;
        const int t = sh.live[i], r = sh.hi_rows[j];
        const float iou = track_iou(sh.pred[t], fbox[r]);
        const float sim = P.w_iou * iou + P.w_app * cand[idx];
        const bool ok = sim >= P.match_thr && (!P.match_labels || sh.label[t] == flabel[r]);
        cand[idx] = ok ? sim : 0.f;
      }
      __syncthreads();
      if (n_live > 0 && n_hi > 0) WD_TRACK_ASSOCIATE(cand, sh.hi_rows, n_hi, 1, P.match_thr);
    }

    // ---- round 2: IoU only, the low-score rows against the unmatched slots seen in the previous frame
    if (n_live > 0 && n_lo > 0) {                                  // block-uniform
      float* cand = n_live * n_lo <= TILE ? sh.tile : ws;
      __syncthreads();                                             // the last reads of round 1's values are done
      for (int idx = tid; idx < n_live * n_lo; idx += 256) {
        const int i = idx % n_live, j = idx / n_live;
        const int t = sh.live[i], r = sh.lo_rows[j];
        float v = 0.f;
        if (sh.match[t] < 0 && sh.miss[t] == 0 && (!P.match_labels || sh.label[t] == flabel[r])) {
          const float iou = track_iou(sh.pred[t], fbox[r]);
          v = iou >= P.iou2_thr ? iou : 0.f;
        }
        cand[idx] = v;
      }
      __syncthreads();
      WD_TRACK_ASSOCIATE(cand, sh.lo_rows, n_lo, 2, P.iou2_thr);
    }
    __syncthreads();

    // ---- update: the slots' scalars, one lane per slot
    if (sh.id[tid] > 0) {
      const int m = sh.match[tid];
      if (m >= 0) {
        const int r = m & 0xFFFF;
        const f32x4 det = fbox[r], bx = sh.box[tid], vl = sh.vel[tid];
        f32x4 nv;
#pragma unroll
        for (int k = 0; k < 4; ++k) nv[k] = P.ema_vel * vl[k] + P.w_vel * (det[k] - bx[k]);
        sh.vel[tid] = nv;
        sh.box[tid] = det;
        sh.label[tid] = flabel[r];
        sh.score[tid] = fscore[r];
        sh.hits[tid] += 1;
        sh.miss[tid] = 0;
      } else {
        sh.box[tid] = sh.pred[tid];
        sh.miss[tid] += 1;
        if (sh.miss[tid] > P.max_age) sh.id[tid] = 0;
      }
    }
    // the embeddings of the round-1 matches, one wave per slot (has / match are not touched by the lanes above)
    for (int i = wave; i < n_live; i += 4) {
      const int t = sh.live[i], m = sh.match[t];
      if (m < 0 || (m >> 16) != 1) continue;                       // wave-uniform
      const int r = m & 0xFFFF;
      const float inv = sh.inv_e[r];
      if (!(inv > 0.f)) continue;
      f32x4 e[NC], v[NC];
      load_row<NC>(e, fembed + (long long)r * dim, dim, lane);
      float* trow = temb + (long long)t * dim;
      if (sh.has[t]) {
        load_row<NC>(v, trow, dim, lane);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = P.ema_embed * v[c][k] + P.w_embed * (e[c][k] * inv);
        const float ss = tree_dot<NC>(v, v);
        if (usable_norm(ss)) {
          const float vi = 1.0f / sqrtf(ss);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = v[c][k] * vi;
          store_row<NC>(v, trow, dim, lane);
        }
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = e[c][k] * inv;
        store_row<NC>(v, trow, dim, lane);
        if (lane == 0) sh.has[t] = 1;
      }
    }
    __syncthreads();

    // ---- births: in row order, each into the lowest free slot — a serial rule, one lane
    if (tid == 0) {
      int fs = 0, nb = 0;
      for (int j = 0; j < n_hi; ++j) {
        const int r = sh.hi_rows[j];
        if (sh.row_slot[r] != 0 || !sh.starts[r]) continue;
        while (fs < max_tracks && sh.id[fs] > 0) ++fs;
        if (fs >= max_tracks) { sh.status |= WD_TRACK_STATUS_FULL; break; }   // every later row would find none either
        sh.id[fs] = sh.next_id++;
        sh.label[fs] = flabel[r];
        sh.score[fs] = fscore[r];
        sh.box[fs] = fbox[r];
        sh.vel[fs] = f32x4{0.f, 0.f, 0.f, 0.f};
        sh.hits[fs] = 1;
        sh.miss[fs] = 0;
        sh.has[fs] = 0;
        sh.match[fs] = r | (3 << 16);
        sh.row_slot[r] = (unsigned short)(fs + 1);
        sh.live[nb++] = (unsigned short)fs;
      }
      sh.n_born = nb;
    }
    __syncthreads();
    const int n_born = sh.n_born;
    for (int k = wave; k < n_born; k += 4) {
      const int t = sh.live[k], r = sh.match[t] & 0xFFFF;
      const float inv = sh.inv_e[r];
      if (!(inv > 0.f)) continue;                                  // wave-uniform
      f32x4 e[NC];
      load_row<NC>(e, fembed + (long long)r * dim, dim, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) e[c][q] = e[c][q] * inv;
      store_row<NC>(e, temb + (long long)t * dim, dim, lane);
      if (lane == 0) sh.has[t] = 1;
    }
    for (int r = tid; r < max_out; r += 256) {
      const int sl = r < cnt ? sh.row_slot[r] : 0;
      track_ids[b * max_out + r] = sl ? sh.id[sl - 1] : 0;
      track_hits[b * max_out + r] = sl ? sh.hits[sl - 1] : 0;
    }
    __syncthreads();                                               // the frame's LDS and embedding writes, before the next frame
  }

  if (tid < max_tracks) {
    sti[L.id() + tid] = sh.id[tid];
    sti[L.label() + tid] = sh.label[tid];
    st[L.score() + tid] = sh.score[tid];
    sti[L.hits() + tid] = sh.hits[tid];
    sti[L.miss() + tid] = sh.miss[tid];
    sti[L.has() + tid] = sh.has[tid];
    const f32x4 bx = sh.box[tid], vl = sh.vel[tid];
#pragma unroll
    for (int k = 0; k < 4; ++k) { st[L.box() + tid * 4 + k] = bx[k]; st[L.vel() + tid * 4 + k] = vl[k]; }
  }
  if (tid == 0) { sti[0] = sh.next_id; sti[1] = sh.status; }
