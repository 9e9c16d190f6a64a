// Batched non_max_suppression on gfx950 (utils/general.py:633-725 + torchvision.ops.nms).
//
// Bit-exact contract with the reference CPU path:
//   * candidates: obj > conf; cls' = cls * obj (fp32); multi-label rows (r, j) with cls' > conf in
//     row-major order, or best class = FIRST max; optional class filter.
//   * order: stable descending score == ascending 64-bit key (~score_bits << 32 | r*nc + j); the
//     max_nms cut and torchvision's own stable sort both reduce to this one total order.
//   * suppression: greedy over that order, IoU(i, j) = inter / (area_i + area_j - inter) with
//     boxes offset by cls * 4096 (fp32 adds), suppress iff IoU > thr; every product/sum uses
//     explicit round-to-nearest intrinsics so no FMA contraction changes a bit.
//   * lazy IoU rows: only rows that are KEPT compute IoU against the rest, and the scan stops at
//     max_det kept rows, so work is O(n * kept) instead of the O(n^2) mask.
//
// The modes beyond that default, each through its own C entry (the default entries run as before):
//   * apriori label rows (general.py:663-670): row index A + k is label k of the image, read from a packed label
//     table by the same row helpers (row_xywh, label_cand) -- box = the label's xywh, obj = 1, one-hot class, so the
//     score is 1.0 * 1.0 and the candidate enters the one total order like any other.
//   * criterion NMS (general.py:727-761 over bbox_iou, general.py:764-824): KIND picks GIoU / DIoU / CIoU of
//     (box1 = the kept, earlier box, box2 = the later one), j suppressed iff !(value <= thr), a NaN suppresses.
//   * merge-NMS (general.py:712-718): nms_merge_kernel / nms_compact_kernel after the keep list is cut to max_det.
#include "launch.h"

namespace {

constexpr unsigned long long PADKEY = 0xFFFFFFFFFFFFFFFFull;

struct NmsCfg {
  int A, no, nc;          // anchors per image, row width, classes
  float conf, iou;
  int multi, agnostic, max_det, max_nms;
  const unsigned char* cls_ok;  // nullable [nc] class filter
  const float* lab;             // nullable packed apriori labels [sum n_i, 5] = (cls, x, y, w, h) in pixels
  const int* lab_off;           // [nimg + 1] offsets of each image's labels in lab (with lab)
};

// score recomputation shared by candidate and gather kernels (identical fp32 ops)
DEV float cand_score(const float* row, int j) { return __fmul_rn(row[5 + j], row[4]); }

DEV int best_class(const float* row, int nc, float* sc) {
  int bj = 0;
  float bv = cand_score(row, 0);
  for (int j = 1; j < nc; ++j) {
    const float v = cand_score(row, j);
    if (v > bv) { bv = v; bj = j; }
  }
  *sc = bv;
  return bj;
}

// the (x, y, w, h) of row r of image b: prediction row r, or for r >= A label r - A of the image (general.py:667;
// only a launch with a label table makes such row indices)
DEV const float* row_xywh(const float* pred, const NmsCfg& cfg, int b, int r) {
  if (r >= cfg.A) return cfg.lab + ((long)cfg.lab_off[b] + (r - cfg.A)) * 5 + 1;
  return pred + ((long)b * cfg.A + r) * cfg.no;
}

// the score recomputation of a label row (general.py:668-669, 677): obj = 1, the class vector one-hot, so class
// (long)cls scores 1.0 * 1.0 and every other class 0, which passes no threshold: the row is one candidate with or
// without multi_label.  False for a class outside [0, nc) (the reference's indexing raises there; such a row is dropped)
DEV bool label_cand(const NmsCfg& cfg, int b, int r, int* j, float* s) {
  const float c = cfg.lab[((long)cfg.lab_off[b] + (r - cfg.A)) * 5];
  if (!(c > -1.f && c < (float)cfg.nc)) return false;
  *j = (int)c;
  *s = __fmul_rn(1.f, 1.f);
  return true;
}

// LAB: the image's label rows follow its A prediction rows (cfg.lab, cfg.lab_off)
template <bool LAB>
__global__ void nms_candidates_kernel(const float* __restrict__ pred, NmsCfg cfg, unsigned long long* __restrict__ keys,
                                      long cap, int* __restrict__ counts) {
  const int b = blockIdx.y;
  const float* P = pred + (long)b * cfg.A * cfg.no;
  int rows = cfg.A;
  if constexpr (LAB) rows += cfg.lab_off[b + 1] - cfg.lab_off[b];
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
    if (LAB && r >= cfg.A) {  // a label row: after every prediction row in the index order
      int j;
      float s;
      if (label_cand(cfg, b, r, &j, &s) && s > cfg.conf && (!cfg.cls_ok || cfg.cls_ok[j])) {
        const int slot = atomicAdd(counts + b, 1);
        if (slot < cap)
          keys[(long)b * cap + slot] = ((unsigned long long)(~__float_as_uint(s)) << 32) | (unsigned)(r * cfg.nc + j);
      }
      continue;
    }
    const float* row = P + (long)r * cfg.no;
    if (!(row[4] > cfg.conf)) continue;
    if (cfg.multi) {
      for (int j = 0; j < cfg.nc; ++j) {
        const float s = cand_score(row, j);
        if (s > cfg.conf && (!cfg.cls_ok || cfg.cls_ok[j])) {
          const int slot = atomicAdd(counts + b, 1);
          if (slot < cap)
            keys[(long)b * cap + slot] = ((unsigned long long)(~__float_as_uint(s)) << 32) | (unsigned)(r * cfg.nc + j);
        }
      }
    } else {
      float s;
      const int j = best_class(row, cfg.nc, &s);
      if (s > cfg.conf && (!cfg.cls_ok || cfg.cls_ok[j])) {
        const int slot = atomicAdd(counts + b, 1);
        if (slot < cap)
          keys[(long)b * cap + slot] = ((unsigned long long)(~__float_as_uint(s)) << 32) | (unsigned)(r * cfg.nc + j);
      }
    }
  }
}

__global__ void pad_keys_kernel(unsigned long long* keys, long cap, const int* counts, int nimg) {
  const int b = blockIdx.y;
  const int n = min((long)counts[b], cap);
  for (long i = n + blockIdx.x * (long)blockDim.x + threadIdx.x; i < cap; i += (long)gridDim.x * blockDim.x)
    keys[(long)b * cap + i] = PADKEY;
}

// ---- bitonic sort of each image's segment (length cap = power of two)
__global__ void bitonic_global_kernel(unsigned long long* keys, long cap, long k, long j) {
  const int b = blockIdx.y;
  unsigned long long* K = keys + (long)b * cap;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < cap; i += (long)gridDim.x * blockDim.x) {
    const long l = i ^ j;
    if (l > i) {
      const unsigned long long a = K[i], c = K[l];
      const bool up = (i & k) == 0;
      if ((a > c) == up) { K[i] = c; K[l] = a; }
    }
  }
}

// all passes with j < 1024 for a 2048-element tile in LDS.  In the first call (k_begin 2: no global pass has moved a key
// between tiles yet) a tile wholly past the image's candidate count holds only pad keys (pad_keys_kernel), sorted in
// either direction: it is skipped -- later calls may not skip, a descending merge carries real keys to a block's end.
// When the whole segment is one tile (cap 2048), only the first P = pow2 >= count keys are sorted: the rest are pad
// keys (written here as the tile is loaded), so the network over the prefix leaves the segment ascending (batch-1 detect at random init:
// ~0 candidates, 27 us -> a few)
__global__ void __launch_bounds__(1024) bitonic_local_kernel(unsigned long long* keys, long cap, long k_begin, long k_end,
                                                             const int* counts) {
  __shared__ unsigned long long s[2048];
  const int b = blockIdx.y;
  unsigned long long* K = keys + (long)b * cap + (long)blockIdx.x * 2048;
  const long g0 = (long)blockIdx.x * 2048;
  const long n = min((long)counts[b], cap);
  if (k_begin == 2 && g0 >= n && cap > 2048) return;  // (one tile: still writes its pads)
  int P = 2048;
  const bool one = cap == 2048 && k_begin == 2;
  if (one) {
    P = 2;
    while (P < n) P <<= 1;
    k_end = P;
  }
  // one tile: the pad keys past the count are made here (dmy_nms_sort launches no pad_keys_kernel for cap 2048)
  s[threadIdx.x] = one && threadIdx.x >= n ? PADKEY : K[threadIdx.x];
  s[threadIdx.x + 1024] = one && threadIdx.x + 1024 >= n ? PADKEY : K[threadIdx.x + 1024];
  __syncthreads();
  for (long k = k_begin; k <= k_end; k <<= 1) {
    for (long j = (k >> 1) < 1024 ? (k >> 1) : 1024; j > 0; j >>= 1) {
      if (j >= 2048) continue;
      for (int t = threadIdx.x; t < P; t += 1024) {
        const int l = t ^ (int)j;
        if (l > t) {
          const unsigned long long a = s[t], c = s[l];
          const bool up = ((g0 + t) & k) == 0;
          if ((a > c) == up) { s[t] = c; s[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  K[threadIdx.x] = s[threadIdx.x];
  K[threadIdx.x + 1024] = s[threadIdx.x + 1024];
}

// ---- greedy NMS, one block per image, lazy IoU rows
DEV void cand_box(const float* pred, const NmsCfg& cfg, int b, unsigned long long key, float* bx, float* score,
                  float* cls) {
  const unsigned rj = (unsigned)(key & 0xFFFFFFFFull);
  const int r = rj / cfg.nc, j = rj % cfg.nc;
  const float* row = row_xywh(pred, cfg, b, r);
  // xywh2xyxy (general.py:539-546)
  const float hw = row[2] / 2.f, hh = row[3] / 2.f;
  bx[0] = __fsub_rn(row[0], hw);
  bx[1] = __fsub_rn(row[1], hh);
  bx[2] = __fadd_rn(row[0], hw);
  bx[3] = __fadd_rn(row[1], hh);
  *score = __uint_as_float(~(unsigned)(key >> 32));
  *cls = (float)j;
}

// The HIP headers' __fmul_rn & co. are plain operators compiled under the build's contraction setting, so a product
// that feeds a sum can still become an FMA (one rounding instead of two).  The default path's formulas keep them as
// they always ran; the criteria below need every rounding of the reference, so their products go through mul_rn: the
// empty asm makes the rounded product an opaque value that no later pass can fuse into its consumer.  (`#pragma clang
// fp contract(off)` in these functions does not do it: under the build's explicit -ffp-contract=fast the inlined
// products were still fused, seen in the ISA; sums, differences and quotients need nothing, only a product can fuse)
DEV float mul_rn(float a, float b) {
  float r = a * b;
  asm("" : "+v"(r));
  return r;
}

// bbox_iou(box1, box2, x1y1x2y2=True, <KIND>) of general.py:764-824 in plain fp32, the reference's operation order,
// one rounding per operation (mul_rn & co.): p = box1 = the kept, earlier box, q = box2 = the later
// one.  eps = 1e-7 sits on h1, h2, union, c2 and c_area; x ** 2 is x * x; / 4 a division; 4 / pi ** 2 and 1 + eps
// python doubles rounded once to fp32.  (csrc/iou.h holds the same formulas in dual numbers for the loss.)
template <int KIND> DEV float box_criterion(const float* p, const float* q) {
  static_assert(KIND == DMY_IOU_GIOU || KIND == DMY_IOU_DIOU || KIND == DMY_IOU_CIOU, "criterion of NMS()");
  const float eps = 1e-7f;
  const float iw = fmaxf(__fsub_rn(fminf(p[2], q[2]), fmaxf(p[0], q[0])), 0.f);
  const float ih = fmaxf(__fsub_rn(fminf(p[3], q[3]), fmaxf(p[1], q[1])), 0.f);
  const float inter = mul_rn(iw, ih);
  const float w1 = __fsub_rn(p[2], p[0]), h1 = __fadd_rn(__fsub_rn(p[3], p[1]), eps);
  const float w2 = __fsub_rn(q[2], q[0]), h2 = __fadd_rn(__fsub_rn(q[3], q[1]), eps);
  const float uni = __fadd_rn(__fsub_rn(__fadd_rn(mul_rn(w1, h1), mul_rn(w2, h2)), inter), eps);
  const float iou = __fdiv_rn(inter, uni);
  const float cw = __fsub_rn(fmaxf(p[2], q[2]), fminf(p[0], q[0]));  // convex (smallest enclosing box) width, height
  const float ch = __fsub_rn(fmaxf(p[3], q[3]), fminf(p[1], q[1]));
  if constexpr (KIND == DMY_IOU_GIOU) {
    const float c_area = __fadd_rn(mul_rn(cw, ch), eps);
    return __fsub_rn(iou, __fdiv_rn(__fsub_rn(c_area, uni), c_area));
  } else {
    const float c2 = __fadd_rn(__fadd_rn(mul_rn(cw, cw), mul_rn(ch, ch)), eps);  // convex diagonal squared
    const float dx = __fsub_rn(__fsub_rn(__fadd_rn(q[0], q[2]), p[0]), p[2]);
    const float dy = __fsub_rn(__fsub_rn(__fadd_rn(q[1], q[3]), p[1]), p[3]);
    const float rho2 = __fdiv_rn(__fadd_rn(mul_rn(dx, dx), mul_rn(dy, dy)), 4.f);  // centre distance squared
    if constexpr (KIND == DMY_IOU_DIOU) {
      return __fsub_rn(iou, __fdiv_rn(rho2, c2));
    } else {
      const float k = (float)(4.0 / (M_PI * M_PI));
      const float da = __fsub_rn(atanf(__fdiv_rn(w2, h2)), atanf(__fdiv_rn(w1, h1)));
      const float v = mul_rn(k, mul_rn(da, da));
      const float alpha = __fdiv_rn(v, __fadd_rn(__fsub_rn(v, iou), (float)(1.0 + 1e-7)));
      return __fsub_rn(iou, __fadd_rn(__fdiv_rn(rho2, c2), mul_rn(v, alpha)));
    }
  }
}

// j (offset box + area c) is suppressed by the kept, earlier candidate (offset box + area p)?  DMY_IOU_PLAIN is
// torchvision.ops.nms's test, the default path's; the other kinds are NMS()'s `iou <= iou_thres` keeps, negated
template <int KIND> DEV bool suppresses(const float* p, const float* c, float thr) {
  if constexpr (KIND == DMY_IOU_PLAIN) {
    const float iw = fmaxf(__fsub_rn(fminf(p[2], c[2]), fmaxf(p[0], c[0])), 0.f);
    const float ih = fmaxf(__fsub_rn(fminf(p[3], c[3]), fmaxf(p[1], c[1])), 0.f);
    const float inter = __fmul_rn(iw, ih);
    const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(p[4], c[4]), inter));
    return iou > thr;
  } else {
    return !(box_criterion<KIND>(p, c) <= thr);
  }
}

template <int KIND>
__global__ void __launch_bounds__(1024) nms_greedy_kernel(const float* __restrict__ pred, NmsCfg cfg,
                                                         const unsigned long long* __restrict__ keys, long cap,
                                                         int* __restrict__ counts, float* __restrict__ boxes,
                                                         float* __restrict__ out, int* __restrict__ nkeep,
                                                         int* __restrict__ ncand) {
  extern __shared__ unsigned long long dead[];  // ceil(n/64) words
  const int b = blockIdx.x;
  const int n = min(min(counts[b], (int)cap), cfg.max_nms);
  const int nw = (n + 63) / 64;
  float* B = boxes + (long)b * cfg.max_nms * 5;  // offset boxes + area, sorted order
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float bx[4], sc, cl;
    cand_box(pred, cfg, b, keys[(long)b * cap + i], bx, &sc, &cl);
    const float off = cfg.agnostic ? 0.f : __fmul_rn(cl, 4096.f);
    for (int q = 0; q < 4; ++q) B[i * 5 + q] = __fadd_rn(bx[q], off);
    B[i * 5 + 4] = __fmul_rn(__fsub_rn(B[i * 5 + 2], B[i * 5 + 0]), __fsub_rn(B[i * 5 + 3], B[i * 5 + 1]));
  }
  for (int w = threadIdx.x; w < nw; w += blockDim.x) dead[w] = 0ull;
  __syncthreads();
  __shared__ int kept;
  if (threadIdx.x == 0) kept = 0;
  __syncthreads();
  for (int w = 0; w < nw && kept < cfg.max_det; ++w) {
    while (true) {
      __syncthreads();
      const unsigned long long valid = (w == nw - 1 && (n & 63)) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
      const unsigned long long alive = ~dead[w] & valid;
      if (alive == 0ull || kept >= cfg.max_det) break;
      const int i = w * 64 + __ffsll((long long)alive) - 1;
      __syncthreads();
      if (threadIdx.x == 0) {
        float bx[4], sc, cl;
        cand_box(pred, cfg, b, keys[(long)b * cap + i], bx, &sc, &cl);
        float* o = out + ((long)b * cfg.max_det + kept) * 6;
        o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3]; o[4] = sc; o[5] = cl;
        atomicOr(&dead[w], 1ull << (i & 63));
        kept = kept + 1;
      }
      const float bi[5] = {B[i * 5], B[i * 5 + 1], B[i * 5 + 2], B[i * 5 + 3], B[i * 5 + 4]};  // box1: the kept one
      for (int jj = i + 1 + threadIdx.x; jj < n; jj += blockDim.x)
        if (suppresses<KIND>(bi, B + jj * 5, cfg.iou)) atomicOr(&dead[jj >> 6], 1ull << (jj & 63));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nkeep[b] = kept;
    if (ncand != nullptr) {  // the count leaves through ncand; the counter is zero again for the next call
      ncand[b] = counts[b];
      counts[b] = 0;
    }
  }
}


// ---- bitmask NMS for capacities <= kMaskCap (one IoU bitmask row per sorted candidate, then a one-wave scan).
// The lazy kernel above walks kept boxes one at a time with block barriers and global box reads per step (~3 us each:
// ~1 ms for 2,000 candidates). Here nms_mask_kernel computes every IoU(i, j > i) > thr bit in parallel with the lazy
// kernel's exact fp32 operations (IoU is symmetric in its rounding: the adds / min / max commute), and nms_scan_kernel
// resolves the greedy order per 64-row block: the diagonal word sequentially in scalar registers, then the kept rows'
// mask words ORed into the later blocks' removed words in parallel (one word per lane). Same keep set and order.
constexpr int kMaskCap = 4096;

// the offset box + area of sorted candidate i (nms_boxes_kernel's arithmetic)
DEV void offset_box(const float* pred, const NmsCfg& cfg, int b, unsigned long long key, float* o) {
  float bx[4], sc, cl;
  cand_box(pred, cfg, b, key, bx, &sc, &cl);
  const float off = cfg.agnostic ? 0.f : __fmul_rn(cl, 4096.f);
  for (int q = 0; q < 4; ++q) o[q] = __fadd_rn(bx[q], off);
  o[4] = __fmul_rn(__fsub_rn(o[2], o[0]), __fsub_rn(o[3], o[1]));
}

// grid (cap/64 row blocks, cap/64 column blocks, nimg), 64 threads: mask[b][i][cb] bit c = IoU(i, 64 cb + c) > thr, j > i.
// The boxes come straight from the sorted keys (offset_box): no separate boxes launch.  KIND: the suppression test
// (suppresses<KIND>); for the kinds that are not symmetric the bit's row i is box1, as in the lazy kernel
template <int KIND>
__global__ void __launch_bounds__(64) nms_mask_kernel(const float* __restrict__ pred, NmsCfg cfg,
                                                      const unsigned long long* __restrict__ keys, long cap,
                                                      const int* __restrict__ counts,
                                                      unsigned long long* __restrict__ mask) {
  const int rb = blockIdx.x, cb = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  if (cb < rb) return;
  const int n = min(min(counts[b], (int)cap), cfg.max_nms);
  if (rb * 64 >= n) return;
  __shared__ float cbx[64][5];
  const int j0 = cb * 64;
  if (j0 + t < n) offset_box(pred, cfg, b, keys[(long)b * cap + j0 + t], cbx[t]);
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= n) return;
  float rbx[5];
  offset_box(pred, cfg, b, keys[(long)b * cap + i], rbx);
  unsigned long long bits = 0ull;
  const int cend = min(64, n - j0);
  for (int c = 0; c < cend; ++c) {
    if (j0 + c <= i) continue;
    if (suppresses<KIND>(rbx, cbx[c], cfg.iou)) bits |= 1ull << c;  // box1 = row i, the earlier one: bit (i, j > i)
  }
  mask[((long)b * cap + i) * (cap / 64) + cb] = bits;
}

DEV unsigned long long readlane64(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// one wave per image; lane w holds the removed-bits word of candidates [64 w, 64 w + 64)
__global__ void __launch_bounds__(64) nms_scan_kernel(const float* __restrict__ pred, NmsCfg cfg,
                                                      const unsigned long long* __restrict__ keys, long cap,
                                                      int* __restrict__ counts,
                                                      const unsigned long long* __restrict__ mask,
                                                      float* __restrict__ out, int* __restrict__ nkeep,
                                                      int* __restrict__ ncand) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(min(counts[b], (int)cap), cfg.max_nms);
  const int nw = (n + 63) / 64, W = (int)(cap / 64);
  const unsigned long long* Mb = mask + (long)b * cap * W;
  unsigned long long removed = 0ull;
  int kept = 0;
  for (int rb = 0; rb < nw && kept < cfg.max_det; ++rb) {
    const int i = rb * 64 + lane;
    const unsigned long long diag = i < n ? Mb[(long)i * W + rb] : 0ull;
    const unsigned long long valid = (rb == nw - 1 && (n & 63)) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
    unsigned long long alive = ~readlane64(removed, rb) & valid;
    unsigned long long keepm = 0ull;
    const int kbase = kept;
    while (alive != 0ull && kept < cfg.max_det) {
      const int t = __builtin_amdgcn_readfirstlane(__ffsll((long long)alive) - 1);
      keepm |= 1ull << t;
      ++kept;
      alive &= ~(readlane64(diag, t) | (1ull << t));
    }
    if ((keepm >> lane) & 1ull) {
      float bx[4], sc, cl;
      cand_box(pred, cfg, b, keys[(long)b * cap + i], bx, &sc, &cl);
      const int idx = kbase + __popcll(keepm & ((1ull << lane) - 1ull));
      float* o = out + ((long)b * cfg.max_det + idx) * 6;
      o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3]; o[4] = sc; o[5] = cl;
    }
    if (lane > rb && lane < nw) {
      unsigned long long km = keepm;
      while (km != 0ull) {
        const int t = __ffsll((long long)km) - 1;
        km &= km - 1ull;
        removed |= Mb[(long)(rb * 64 + t) * W + lane];
      }
    }
  }
  if (lane == 0) {
    nkeep[b] = kept;
    if (ncand != nullptr) {  // the count leaves through ncand; the counter is zero again for the next call
      ncand[b] = counts[b];
      counts[b] = 0;
    }
  }
}

// ---- merge-NMS (general.py:712-718), after the keep list is cut to max_det: the image's n candidates (before the
// max_nms cut) with 1 < n < 3000, else the rows stay as they are (n <= cap: an overflowing launch is rerun anyway)
DEV bool merge_applies(int n, long cap) { return n > 1 && n < 3000 && n <= cap; }

// box_iou (utils/metrics.py:254-276) of two offset boxes + areas: inter / (area1 + area2 - inter), one rounding each
DEV float plain_iou(const float* p, const float* c) {
  const float iw = fmaxf(__fsub_rn(fminf(p[2], c[2]), fmaxf(p[0], c[0])), 0.f);
  const float ih = fmaxf(__fsub_rn(fminf(p[3], c[3]), fmaxf(p[1], c[1])), 0.f);
  const float inter = mul_rn(iw, ih);
  return __fdiv_rn(inter, __fsub_rn(__fadd_rn(p[4], c[4]), inter));
}

// grid (max_det, nimg), 256 threads: block (k, b) merges kept row k of image b.  hit[j] = box_iou(offset box of the
// kept row, offset box j) > thr over ALL n sorted candidates (itself and earlier ones included), w[j] = hit[j] *
// score[j], merged box = sum w[j] xyxy[j] / sum w[j] over the un-offset boxes: the five sums in fp64 (every product
// of two fp32 values is exact there), one division and one rounding to fp32 per coordinate.  The kept row's offset box
// is remade from its output row (xyxy + cls * 4096, offset_box's own adds).  merged: the new rows, hits: each row's
// hit count (the `redundant` filter reads it); `out` is only read here, nms_compact_kernel rewrites it
__global__ void __launch_bounds__(256) nms_merge_kernel(const float* __restrict__ pred, NmsCfg cfg,
                                                        const unsigned long long* __restrict__ keys, long cap,
                                                        const int* __restrict__ counts, const float* __restrict__ out,
                                                        const int* __restrict__ nk, float* __restrict__ merged,
                                                        int* __restrict__ hits) {
  const int k = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int n = counts[b];
  if (k >= min(nk[b], cfg.max_det) || !merge_applies(n, cap)) return;
  const float* o = out + ((long)b * cfg.max_det + k) * 6;
  float bi[5];
  {
    const float off = cfg.agnostic ? 0.f : __fmul_rn(o[5], 4096.f);
    for (int q = 0; q < 4; ++q) bi[q] = __fadd_rn(o[q], off);
    bi[4] = mul_rn(__fsub_rn(bi[2], bi[0]), __fsub_rn(bi[3], bi[1]));
  }
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int hc = 0;
  for (int j = t; j < n; j += 256) {
    float bx[4], sc, cl, c[5];
    cand_box(pred, cfg, b, keys[(long)b * cap + j], bx, &sc, &cl);
    const float off = cfg.agnostic ? 0.f : __fmul_rn(cl, 4096.f);
    for (int q = 0; q < 4; ++q) c[q] = __fadd_rn(bx[q], off);
    c[4] = mul_rn(__fsub_rn(c[2], c[0]), __fsub_rn(c[3], c[1]));
    if (plain_iou(bi, c) > cfg.iou) {
      for (int q = 0; q < 4; ++q) s[q] += (double)sc * (double)bx[q];
      s[4] += (double)sc;
      ++hc;
    }
  }
  for (int sh = 32; sh > 0; sh >>= 1) {
    for (int q = 0; q < 5; ++q) s[q] += __shfl_xor(s[q], sh, 64);
    hc += __shfl_xor(hc, sh, 64);
  }
  __shared__ double ws[4][5];
  __shared__ int wh[4];
  if ((t & 63) == 0) {
    for (int q = 0; q < 5; ++q) ws[t >> 6][q] = s[q];
    wh[t >> 6] = hc;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) {
      for (int q = 0; q < 5; ++q) s[q] += ws[w][q];
      hc += wh[w];
    }
    float* m = merged + ((long)b * cfg.max_det + k) * 6;
    for (int q = 0; q < 4; ++q) m[q] = (float)(s[q] / s[4]);
    m[4] = o[4];
    m[5] = o[5];
    hits[(long)b * cfg.max_det + k] = hc;
  }
}

// one wave per image: the merged rows back into `out` in keep order, with `redundant` only those whose hit count is
// above 1 (general.py:717-718), and the keep count where nms_finish reads it.  The greedy launch before a merge left
// the candidate counter alone (its ncand was null), so the hand-over to ncand and the re-zeroing happen here
__global__ void __launch_bounds__(64) nms_compact_kernel(NmsCfg cfg, long cap, int redundant, int* __restrict__ counts,
                                                         const int* __restrict__ nk, const float* __restrict__ merged,
                                                         const int* __restrict__ hits, float* __restrict__ out,
                                                         int* __restrict__ nkeep, int* __restrict__ ncand) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = counts[b], kn = min(nk[b], cfg.max_det);
  int kept = kn;
  if (merge_applies(n, cap)) {
    kept = 0;
    for (int k0 = 0; k0 < kn; k0 += 64) {
      const int k = k0 + lane;
      const bool on = k < kn && (!redundant || hits[(long)b * cfg.max_det + k] > 1);
      const unsigned long long m = __ballot(on);
      if (on) {
        const float* src = merged + ((long)b * cfg.max_det + k) * 6;
        float* dst = out + ((long)b * cfg.max_det + kept + __popcll(m & ((1ull << lane) - 1ull))) * 6;
        for (int q = 0; q < 6; ++q) dst[q] = src[q];
      }
      kept += __popcll(m);
    }
  }
  if (lane == 0) {
    nkeep[b] = kept;
    if (ncand != nullptr) {
      ncand[b] = counts[b];
      counts[b] = 0;
    }
  }
}

}  // namespace

DMY_API int dmy_nms_candidates(const float* pred, int nimg, int A, int no, float conf, int multi,
                               const unsigned char* cls_ok, unsigned long long* keys, long cap, int* counts,
                               void* stream) {
  NmsCfg cfg{A, no, no - 5, conf, 0.f, multi, 0, 0, 0, cls_ok};
  dim3 grid(grid_cap(ceil_div(A, 256), 256), nimg);
  return launch(nms_candidates_kernel<false>, grid, stream, pred, cfg, keys, cap, counts);
}

// cap must be a power of two >= 2048; sorts each image's [0, cap) key segment ascending
DMY_API int dmy_nms_sort(unsigned long long* keys, long cap, const int* counts, int nimg, void* stream) {
  dim3 gp(grid_cap(ceil_div(cap, 256), 1024), nimg);
  if (cap > 2048) {  // cap 2048: bitonic_local pads
    if (int e = launch(pad_keys_kernel, gp, stream, keys, cap, counts, nimg)) return e;
  }
  dim3 gl((unsigned)(cap / 2048), nimg);
  if (int e = launch(bitonic_local_kernel, gl, 1024, 0, stream, keys, cap, 2, 2048, counts)) return e;
  for (long k = 4096; k <= cap; k <<= 1) {
    for (long j = k >> 1; j >= 2048; j >>= 1)
      if (int e = launch(bitonic_global_kernel, gp, stream, keys, cap, k, j)) return e;
    if (int e = launch(bitonic_local_kernel, gl, 1024, 0, stream, keys, cap, k, k, counts)) return e;
  }
  return 0;
}

DMY_API int dmy_nms_greedy(const float* pred, int nimg, int A, int no, float iou, int agnostic, int max_det,
                           int max_nms, const unsigned long long* keys, long cap, int* counts, float* boxes,
                           float* out, int* nkeep, int* ncand, void* stream) {
  NmsCfg cfg{A, no, no - 5, 0.f, iou, 0, agnostic, max_det, max_nms, nullptr};
  const size_t lds = sizeof(unsigned long long) * (size_t)((max_nms + 63) / 64);
  return launch(nms_greedy_kernel<DMY_IOU_PLAIN>, nimg, 1024, lds, stream, pred, cfg, keys, cap, counts, boxes, out, nkeep,
                ncand);
}

DMY_API int dmy_nms_mask_rows() { return kMaskCap; }

// the bitmask path: cap (the sort capacity) <= dmy_nms_mask_rows(); mask holds nimg * cap * cap / 64 words
DMY_API int dmy_nms_greedy_mask(const float* pred, int nimg, int A, int no, float iou, int agnostic, int max_det,
                                int max_nms, const unsigned long long* keys, long cap, int* counts, float* boxes,
                                unsigned long long* mask, float* out, int* nkeep, int* ncand, void* stream) {
  if (cap > kMaskCap || cap % 64 != 0) return kInvalid;
  NmsCfg cfg{A, no, no - 5, 0.f, iou, 0, agnostic, max_det, max_nms, nullptr};
  (void)boxes;  // the mask kernel makes its boxes from the keys (the lazy path's scratch; kept in the ABI)
  const dim3 gm((unsigned)(cap / 64), (unsigned)(cap / 64), nimg);
  if (int e = launch(nms_mask_kernel<DMY_IOU_PLAIN>, gm, 64, 0, stream, pred, cfg, keys, cap, counts, mask)) return e;
  return launch(nms_scan_kernel, nimg, 64, 0, stream, pred, cfg, keys, cap, counts, mask, out, nkeep, ncand);
}

// ---- the modes beyond the default call: label rows, criterion NMS, merge-NMS

// dmy_nms_candidates with the apriori label rows of general.py:663-670: labels [sum n_i, 5] = (cls, x, y, w, h) in
// pixels, packed image after image, label_off [nimg + 1] their offsets; label k of an image is row A + k
DMY_API int dmy_nms_candidates_labels(const float* pred, const float* labels, const int* label_off, int nimg, int A,
                                      int no, float conf, int multi, const unsigned char* cls_ok,
                                      unsigned long long* keys, long cap, int* counts, void* stream) {
  if (labels == nullptr || label_off == nullptr) return kInvalid;
  NmsCfg cfg{A, no, no - 5, conf, 0.f, multi, 0, 0, 0, cls_ok, labels, label_off};
  // a grid for the A prediction rows and one more block: the kernel's grid-stride loop walks label lists past it
  dim3 grid(grid_cap(ceil_div(A + 256, 256), 256), nimg);
  return launch(nms_candidates_kernel<true>, grid, stream, pred, cfg, keys, cap, counts);
}

// a label table goes with its offsets, or neither is given
static bool labels_ok(const float* labels, const int* label_off) { return (labels == nullptr) == (label_off == nullptr); }

// dmy_nms_greedy with the suppression criterion chosen (iou_kind: DMY_IOU_PLAIN, _GIOU, _DIOU or _CIOU; DMY_IOU_SIOU
// and anything else is refused) and row indices >= A read from the label table (labels / label_off nullable)
DMY_API int dmy_nms_greedy_kind(int iou_kind, const float* pred, const float* labels, const int* label_off, int nimg,
                                int A, int no, float iou, int agnostic, int max_det, int max_nms,
                                const unsigned long long* keys, long cap, int* counts, float* boxes, float* out,
                                int* nkeep, int* ncand, void* stream) {
  if (!labels_ok(labels, label_off)) return kInvalid;
  NmsCfg cfg{A, no, no - 5, 0.f, iou, 0, agnostic, max_det, max_nms, nullptr, labels, label_off};
  const size_t lds = sizeof(unsigned long long) * (size_t)((max_nms + 63) / 64);
  return by_int<DMY_IOU_PLAIN, DMY_IOU_GIOU, DMY_IOU_DIOU, DMY_IOU_CIOU>(iou_kind, kInvalid, [&](auto kind) {
    return launch(nms_greedy_kernel<decltype(kind)::value>, nimg, 1024, lds, stream, pred, cfg, keys, cap, counts, boxes,
                  out, nkeep, ncand);
  });
}

// dmy_nms_greedy_mask likewise (cap <= dmy_nms_mask_rows(); no boxes scratch: the mask kernel makes each box from its key)
DMY_API int dmy_nms_greedy_mask_kind(int iou_kind, const float* pred, const float* labels, const int* label_off,
                                     int nimg, int A, int no, float iou, int agnostic, int max_det, int max_nms,
                                     const unsigned long long* keys, long cap, int* counts, unsigned long long* mask,
                                     float* out, int* nkeep, int* ncand, void* stream) {
  if (cap > kMaskCap || cap % 64 != 0 || !labels_ok(labels, label_off)) return kInvalid;
  NmsCfg cfg{A, no, no - 5, 0.f, iou, 0, agnostic, max_det, max_nms, nullptr, labels, label_off};
  const dim3 gm((unsigned)(cap / 64), (unsigned)(cap / 64), nimg);
  return by_int<DMY_IOU_PLAIN, DMY_IOU_GIOU, DMY_IOU_DIOU, DMY_IOU_CIOU>(iou_kind, kInvalid, [&](auto kind) {
    if (int e = launch(nms_mask_kernel<decltype(kind)::value>, gm, 64, 0, stream, pred, cfg, keys, cap, counts, mask))
      return e;
    return launch(nms_scan_kernel, nimg, 64, 0, stream, pred, cfg, keys, cap, counts, mask, out, nkeep, ncand);
  });
}

// merge-NMS over the rows a greedy launch left in `out` (that launch with ncand null and its keep counts in nk, a
// device vector: counts still holds the candidate counts).  merged [nimg, max_det, 6] and hits [nimg, max_det] are
// scratch.  Rewrites `out`, stores the final keep counts in nkeep and hands counts to ncand as the greedy entries do
DMY_API int dmy_nms_merge(const float* pred, const float* labels, const int* label_off, int nimg, int A, int no,
                          float iou, int agnostic, int max_det, int redundant, const unsigned long long* keys, long cap,
                          int* counts, const int* nk, float* merged, int* hits, float* out, int* nkeep, int* ncand,
                          void* stream) {
  if (!labels_ok(labels, label_off) || max_det < 0) return kInvalid;
  NmsCfg cfg{A, no, no - 5, 0.f, iou, 0, agnostic, max_det, 0, nullptr, labels, label_off};
  if (max_det > 0) {  // max_det 0 keeps nothing: only the counts are handed over
    if (int e = launch(nms_merge_kernel, dim3(max_det, nimg), 256, 0, stream, pred, cfg, keys, cap, counts, out, nk,
                       merged, hits))
      return e;
  }
  return launch(nms_compact_kernel, nimg, 64, 0, stream, cfg, cap, redundant, counts, nk, merged, hits, out, nkeep,
                ncand);
}
