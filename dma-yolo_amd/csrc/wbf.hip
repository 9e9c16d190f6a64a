// Weighted boxes fusion on gfx950: ensemble_boxes.weighted_boxes_fusion (conf_type 'avg', allows_overflow False), the
// fusion step of the reference's multi-model evaluation (wbf.py:67), over the padded NMS output of M models.
//
// Bit-exact contract with the host restatement (tests/wbf_ref.py): every step is IEEE fp64, one rounding per operation
// (no FMA contraction in this translation unit), the divisions are the compiler's correctly rounded fp64 sequence.
//   1. prefilter  one thread per (model t, row j): score >= skip_box_thr, xyxy / (W, H), swap, clamp to [0, 1], drop
//                 zero area; record key = (label, s = score * w[t] descending, i = t * R + j).
//   2. order      counting rank sort: a record's rank is the number of records whose key precedes its own.  The key is
//                 a total order, so the ranks are a permutation and no two threads write one slot.  Equal labels are
//                 then contiguous: one segment per label, in score order.
//   3. cluster    one block per segment, sequential over its records: block-wide IoU against the live clusters'
//                 fused boxes, first-maximum reduction, thread 0 applies the running-sum update.  The cluster state
//                 lives in the workspace at (segment start + creation index).
//   4. output     the same rank sort over the cluster scores (ties: position = label, then creation index) scatters the
//                 rows; the thread of position 0 counts them into nout.
// No atomics anywhere.  Capacity: M * R <= dmy_wbf_max_rows() records per image, any int32 label, any label count.
#include "launch.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kMaxRows = 16384;  // records per image (M * R): the rank sorts are O(rows^2) per image
constexpr int kMaxImages = 65535;  // grid.y
constexpr int kSegBlocks = 256;  // cluster blocks per image; block x takes the segments that start at x, x + 256, ...
constexpr u64 kPad = ~0ull;  // cluster-score key of a position that holds no cluster
constexpr u64 kDropped = 1ull << 32;  // record label key of a row the prefilter dropped: after every real label

// per-image arrays of N = M * R entries, image b at offset b * N.  r*: by record index i = t * R + j; order and c*: by
// sorted position
struct WbfWs {
  u64 *rk0, *rk1;  // record key: biased label (kDropped when dropped), descending-score key
  u64* ckey;  // descending cluster-score key, kPad where no cluster
  double *rbox, *rs;  // record box [4] (normalised), s = score * w[t]
  double *cbox, *cS, *cconf, *cscore;  // cluster: fused box [4], sum of s * box [4], sum of s, final score
  int *order, *cn, *clabel;  // record index at each sorted position; cluster member count, label
};

// ascending unsigned order of the result == descending order of x; -0.0 sorts as +0.0 (they compare equal)
DEV u64 desc_key(double x) {
  const u64 b = (u64)__double_as_longlong(x + 0.0);
  return ~((b >> 63) ? ~b : (b | (1ull << 63)));
}

__global__ void __launch_bounds__(256) wbf_prefilter_kernel(const float* __restrict__ det, const int* __restrict__ counts,
                                                            const float* __restrict__ wh,
                                                            const double* __restrict__ weights, int M, int nimg, int R,
                                                            double skip_thr, WbfWs ws) {
  const int b = blockIdx.y, N = M * R;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int t = i / R, j = i - t * R;
  const long p = (long)b * N + i;
  u64 k0 = kDropped, k1 = 0ull;
  const int cnt = min(max(counts[t * nimg + b], 0), R);
  if (j < cnt) {
    const float* row = det + (((long)t * nimg + b) * R + j) * 6;
    const double score = (double)row[4];
    if (!(score < skip_thr)) {
      const double W = (double)wh[b * 2], H = (double)wh[b * 2 + 1];
      double x1 = (double)row[0] / W, y1 = (double)row[1] / H, x2 = (double)row[2] / W, y2 = (double)row[3] / H;
      if (x2 < x1) { const double v = x1; x1 = x2; x2 = v; }
      if (y2 < y1) { const double v = y1; y1 = y2; y2 = v; }
      double c[4] = {x1, y1, x2, y2};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (c[q] < 0.0) c[q] = 0.0;
        if (c[q] > 1.0) c[q] = 1.0;
      }
      if (!((c[2] - c[0]) * (c[3] - c[1]) == 0.0)) {
        const double s = score * weights[t];
        k0 = (u64)((unsigned)(int)row[5] ^ 0x80000000u);
        k1 = desc_key(s);
#pragma unroll
        for (int q = 0; q < 4; ++q) ws.rbox[p * 4 + q] = c[q];
        ws.rs[p] = s;
      }
    }
  }
  ws.rk0[p] = k0;
  ws.rk1[p] = k1;
}

// the number of entries of the image whose key (K0, K1, index) precedes entry i's; every thread of the block calls it
// (barriers).  K1 null: a one-word key.  *live (if given) receives the number of entries with K0 != kPad
DEV int rank_of(const u64* __restrict__ K0, const u64* __restrict__ K1, int N, int i, int* live) {
  __shared__ u64 s0[256], s1[256];
  const u64 a0 = i < N ? K0[i] : 0ull, a1 = (i < N && K1) ? K1[i] : 0ull;
  int rank = 0, nlive = 0;
  for (int base = 0; base < N; base += 256) {
    const int j = base + threadIdx.x;
    __syncthreads();
    if (j < N) {
      s0[threadIdx.x] = K0[j];
      s1[threadIdx.x] = K1 ? K1[j] : 0ull;
    }
    __syncthreads();
    const int lim = min(256, N - base);
    for (int q = 0; q < lim; ++q) {
      const u64 c0 = s0[q], c1 = s1[q];
      rank += (c0 < a0 || (c0 == a0 && (c1 < a1 || (c1 == a1 && base + q < i)))) ? 1 : 0;
      nlive += c0 != kPad ? 1 : 0;
    }
  }
  if (live) *live = nlive;
  return rank;
}

__global__ void __launch_bounds__(256) wbf_order_kernel(int N, WbfWs ws) {
  const long o = (long)blockIdx.y * N;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int rank = rank_of(ws.rk0 + o, ws.rk1 + o, N, i, nullptr);
  if (i < N) {
    ws.order[o + rank] = i;
    ws.ckey[o + rank] = kPad;  // every position once: the cluster kernel overwrites those that hold a cluster
  }
}

__global__ void __launch_bounds__(256) wbf_cluster_kernel(const double* __restrict__ weights, int M, int N,
                                                          double iou_thr, WbfWs ws) {
  __shared__ double riou[4];
  __shared__ int ridx[4];
  const long o = (long)blockIdx.y * N;
  const int tid = threadIdx.x, wave = tid >> 6;
  double sumw = 0.0;
  for (int t = 0; t < M; ++t) sumw = sumw + weights[t];
  for (int p0 = blockIdx.x; p0 < N; p0 += gridDim.x) {
    const u64 lab = ws.rk0[o + ws.order[o + p0]];
    if (lab == kDropped) break;  // dropped rows sort last: no segment starts at or after this position
    if (p0 > 0 && ws.rk0[o + ws.order[o + p0 - 1]] == lab) continue;  // not the first record of its label
    int ncl = 0;
    for (int r = p0; r < N; ++r) {
      const long ri = o + ws.order[o + r];
      if (ws.rk0[ri] != lab) break;
      const double x1 = ws.rbox[ri * 4], y1 = ws.rbox[ri * 4 + 1], x2 = ws.rbox[ri * 4 + 2], y2 = ws.rbox[ri * 4 + 3];
      const double s = ws.rs[ri];
      const double areaB = (x2 - x1) * (y2 - y1);
      double best = -1.0;
      int bi = 0x7fffffff;
      for (int c = tid; c < ncl; c += 256) {
        const double* cb = ws.cbox + (o + p0 + c) * 4;
        const double iw = fmax(fmin(cb[2], x2) - fmax(cb[0], x1), 0.0);
        const double ih = fmax(fmin(cb[3], y2) - fmax(cb[1], y1), 0.0);
        const double inter = iw * ih;
        const double areaA = (cb[2] - cb[0]) * (cb[3] - cb[1]);
        const double iou = inter / (areaA + areaB - inter);
        if (iou > best) { best = iou; bi = c; }
      }
      // first maximum over the block: the larger IoU, on a tie the lower cluster index
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) {
        const double ob = __shfl_xor(best, sh, 64);
        const int oi = __shfl_xor(bi, sh, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if ((tid & 63) == 0) { riou[wave] = best; ridx[wave] = bi; }
      __syncthreads();
      best = riou[0];
      bi = ridx[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const double ob = riou[w];
        const int oi = ridx[w];
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      const bool join = best > iou_thr;
      if (tid == 0) {
        const long pc = o + p0 + (join ? bi : ncl);
        const double bx[4] = {x1, y1, x2, y2};
        if (join) {
          const double conf = ws.cconf[pc] + s;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double S = ws.cS[pc * 4 + q] + s * bx[q];
            ws.cS[pc * 4 + q] = S;
            ws.cbox[pc * 4 + q] = S / conf;
          }
          ws.cconf[pc] = conf;
          ws.cn[pc] = ws.cn[pc] + 1;
        } else {  // a new cluster's fused box is the record's own box
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            ws.cS[pc * 4 + q] = s * bx[q];
            ws.cbox[pc * 4 + q] = bx[q];
          }
          ws.cconf[pc] = s;
          ws.cn[pc] = 1;
        }
      }
      ncl += join ? 0 : 1;
      __syncthreads();  // the update is visible to the block; riou / ridx are free again
    }
    for (int c = tid; c < ncl; c += 256) {
      const long pc = o + p0 + c;
      const double n = (double)ws.cn[pc];
      const double score = ws.cconf[pc] / n * fmin(n, sumw) / sumw;
      ws.cscore[pc] = score;
      ws.ckey[pc] = desc_key(score);
      ws.clabel[pc] = (int)((unsigned)lab ^ 0x80000000u);
    }
  }
}

__global__ void __launch_bounds__(256) wbf_output_kernel(const float* __restrict__ wh, int N, WbfWs ws,
                                                         float* __restrict__ out, int* __restrict__ nout) {
  const int b = blockIdx.y;
  const long o = (long)b * N;
  const int i = blockIdx.x * 256 + threadIdx.x;
  int live;
  const int rank = rank_of(ws.ckey + o, nullptr, N, i, &live);
  if (i == 0) nout[b] = live;
  if (i >= N || ws.ckey[o + i] == kPad) return;
  const double W = (double)wh[b * 2], H = (double)wh[b * 2 + 1];
  const double* cb = ws.cbox + (o + i) * 4;
  float* row = out + (o + rank) * 6;
  row[0] = (float)(cb[0] * W);
  row[1] = (float)(cb[1] * H);
  row[2] = (float)(cb[2] * W);
  row[3] = (float)(cb[3] * H);
  row[4] = (float)ws.cscore[o + i];
  row[5] = (float)ws.clabel[o + i];
}

constexpr long kWords = 18, kInts = 3;  // 8-byte and 4-byte workspace entries per position (WbfWs)

}  // namespace

DMY_API int dmy_wbf_max_rows(void) { return kMaxRows; }

DMY_API long dmy_wbf_workspace_bytes(int nimg, int rows) {
  return (long)nimg * rows * (kWords * 8 + kInts * 4);
}

DMY_API int dmy_wbf(const float* det, const int* counts, const float* wh, const double* weights, int M, int nimg, int R,
                    double iou_thr, double skip_box_thr, void* ws, float* out, int* nout, void* stream) {
  if (M <= 0 || nimg <= 0 || R <= 0 || nimg > kMaxImages || (long)M * R > kMaxRows) return kInvalid;
  if (!det || !counts || !wh || !weights || !ws || !out || !nout || (((uintptr_t)ws) & 7)) return kInvalid;
  const int N = M * R;
  const long n = (long)nimg * N;
  u64* w8 = (u64*)ws;
  double* d8 = (double*)(w8 + 3 * n);
  int* i4 = (int*)(w8 + kWords * n);
  const WbfWs s{w8, w8 + n, w8 + 2 * n, d8, d8 + 4 * n, d8 + 5 * n, d8 + 9 * n, d8 + 13 * n, d8 + 14 * n,
                i4, i4 + n, i4 + 2 * n};
  const dim3 grid(ceil_div(N, 256), nimg);
  int rc = launch(wbf_prefilter_kernel, grid, stream, det, counts, wh, weights, M, nimg, R, skip_box_thr, s);
  if (rc) return rc;
  if ((rc = launch(wbf_order_kernel, grid, stream, N, s))) return rc;
  if ((rc = launch(wbf_cluster_kernel, dim3(N < kSegBlocks ? N : kSegBlocks, nimg), stream, weights, M, N, iou_thr, s)))
    return rc;
  return launch(wbf_output_kernel, grid, stream, wh, N, s, out, nout);
}
