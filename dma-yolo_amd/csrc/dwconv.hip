// Depthwise convolution (groups == C_in == C_out, one k x k filter per channel) for gfx950: forward with the BN
// partial sums or the one-launch inference epilogue, data-grad as a gather, weight-grad through per-block partial
// rows summed in row order.  Replaces nn.Conv2d(groups=c) in DWConv / GhostConv.cv2 (models/common.py:79-82, 666-699)
// and the biased 7 x 7 of get_dwconv in GnConv (:1329, 1361-1362), whose bias gradient rides on the weight-grad launch.
//
// There is no reduction over channels, so no MFMA: these are streaming kernels over NHWC.  A thread owns one 16-byte
// channel vector (weight-grad: 4 channels) of a strip of kTW consecutive output pixels along W, so the (kTW - 1) * S + K
// input columns of a filter row are loaded once for kTW outputs instead of K times each.  Threads of a block are laid
// out (channel unit fastest, strip slot next): a tile of TC channel units (a power of two <= 32, blockIdx.y picks the
// tile) by 256 / TC strips; blocks walk the strip groups with a grid stride, so the number of partial rows is bounded.
//
// Bounds: every address is formed from an in-range (row, column) -- an out-of-range column is clamped to column 0 of
// the same valid row and its value replaced by zero, an out-of-range row is skipped -- and every store is predicated
// on its own pixel and channel unit.  Plain global loads, no buffer descriptors.
//
// Reductions (BN partials, weight-grad partials) go lane -> wave (xor shuffles over the lanes that share a channel
// unit) -> block (the four waves through LDS, summed in wave order) -> one row per block; no atomics anywhere, so the
// results are run-to-run bit-identical.
#include "launch.h"
#include "tile.h"

namespace {

constexpr int kTW = 4;            // output pixels per thread along W
constexpr int kFwdRowCap = 1024;  // BN partial rows (== gridDim.x of the forward)
constexpr int kWgRowCap = 512;    // weight-grad partial rows (== gridDim.x of the weight-grad)
constexpr int kWgC = 4;           // channels per thread in the weight-grad (K * K * 4 accumulators; K = 7: K * 4)

struct Strip {
  int n, oh, ow0;
};
DEV Strip strip_of(long st, int OH, int SW) {
  Strip s;
  s.ow0 = (int)(st % SW) * kTW;
  const long t = st / SW;
  s.oh = (int)(t % OH);
  s.n = (int)(t / OH);
  return s;
}

enum { EPI_STATS = 0, EPI_ACT = 1, EPI_ACC = 2, EPI_ACTBN = 3 };

// out[n, oh, ow, c] = sum_ij in[n, oh * S - P + i, ow * S - P + j, c] * w[i][j][c], P = K / 2; FLIP reads w[K-1-i][K-1-j]
// (the stride-1 data-grad is this correlation of dz with the flipped filter).
//   EPI_STATS: y = T(acc + bias); psum / psq (nullable): per-block sums of the stored values and their squares
//   EPI_ACT:   y = act(T(acc + bias) * scale + shift) (+ res)     (scale / shift nullable together)
//   EPI_ACC:   y = (accumulate ? y : 0) + acc
template <typename T, int K, int S, bool FLIP, int EPI>
__global__ void __launch_bounds__(256)
dw_conv_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
               float* __restrict__ psum, float* __restrict__ psq, int N, int IH, int IW, int C, long ips, int OH, int OW,
               long ops, int tcl, const float* __restrict__ scale, const float* __restrict__ shift, int act,
               const T* __restrict__ res, long rps, int accumulate) {
  constexpr int VW = Traits<T>::VW, P = K / 2, NC = (kTW - 1) * S + K;
  const int TC = 1 << tcl, cu = threadIdx.x & (TC - 1), slot = threadIdx.x >> tcl, PIX = 256 >> tcl;
  const int cv = blockIdx.y * TC + cu;
  const bool cok = cv < C / VW;
  const int c0 = cok ? cv * VW : 0;
  const int SW = (OW + kTW - 1) / kTW;
  const long nstrips = (long)N * OH * SW, ngroups = (nstrips + PIX - 1) / PIX;
  float s1[VW], s2[VW], bs[VW], sc[VW], sh[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) { s1[e] = 0.f; s2[e] = 0.f; bs[e] = 0.f; sc[e] = 1.f; sh[e] = 0.f; }
  if (EPI != EPI_ACC && bias && cok) ldf<VW>(bias + c0, bs);
  if (EPI == EPI_ACT && scale && cok) {
    ldf<VW>(scale + c0, sc);
    ldf<VW>(shift + c0, sh);
  }
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long st = g * PIX + slot;
    if (!cok || st >= nstrips) continue;
    const Strip sp = strip_of(st, OH, SW);
    float acc[kTW][VW];
#pragma unroll
    for (int b = 0; b < kTW; ++b)
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[b][e] = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int ih = sp.oh * S - P + i;
      if (ih < 0 || ih >= IH) continue;
      float wr[K][VW];
#pragma unroll
      for (int j = 0; j < K; ++j) load_vec<T>(w + (long)((FLIP ? K - 1 - i : i) * K + (FLIP ? K - 1 - j : j)) * C + c0, wr[j]);
      const T* xr = x + ((long)sp.n * IH + ih) * IW * ips + c0;
#pragma unroll
      for (int jj = 0; jj < NC; ++jj) {
        const int iw = sp.ow0 * S - P + jj;
        const bool ok = iw >= 0 && iw < IW;
        float xv[VW];
        load_vec<T>(xr + (long)(ok ? iw : 0) * ips, xv);
#pragma unroll
        for (int b = 0; b < kTW; ++b) {
          const int j = jj - b * S;
          if (j >= 0 && j < K) {
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[b][e] += (ok ? xv[e] : 0.f) * wr[j][e];
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < kTW; ++b) {
      const int ow = sp.ow0 + b;
      if (ow >= OW) continue;
      const long pix = ((long)sp.n * OH + sp.oh) * OW + ow;
      T* yp = y + pix * ops + c0;
      float f[VW];
      if (EPI == EPI_ACC) {
        if (accumulate) {
          load_vec<T>(yp, f);
#pragma unroll
          for (int e = 0; e < VW; ++e) f[e] += acc[b][e];
        } else {
#pragma unroll
          for (int e = 0; e < VW; ++e) f[e] = acc[b][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) f[e] = to_f(from_f<T>(acc[b][e] + bs[e]));  // the value as stored
        if (EPI == EPI_STATS) {
#pragma unroll
          for (int e = 0; e < VW; ++e) { s1[e] += f[e]; s2[e] += f[e] * f[e]; }
        } else {
          if (scale) {
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] = f[e] * sc[e] + sh[e];
          }
          act_fwd_n<VW>(act, f);
          if (res) {
            float r[VW];
            load_vec<T>(res + pix * rps + c0, r);
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] += r[e];
          }
        }
      }
      *reinterpret_cast<uint4*>(yp) = pack<T>(f);
    }
  }
  // tile.h's write_rows, inline: through the helper the bf16 instantiations compile to one SGPR fewer (usage is pinned)
  if (EPI == EPI_STATS && psum) {  // block-uniform: every thread reaches the barrier
    __shared__ float red[4][2 * 32 * VW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const float a = unit_sum(s1[e], tcl), q = unit_sum(s2[e], tcl);
      if (lane < TC) {
        red[wave][lane * VW + e] = a;
        red[wave][32 * VW + lane * VW + e] = q;
      }
    }
    __syncthreads();
    const int nch = TC * VW;
    for (int idx = threadIdx.x; idx < 2 * nch; idx += 256) {
      const int half = idx >= nch, cc = idx - half * nch, ch = blockIdx.y * nch + cc;
      if (ch < C) {
        const int o = half * 32 * VW + cc;
        (half ? psq : psum)[(long)blockIdx.x * C + ch] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
      }
    }
  }
}

// stride-2 data-grad as a gather: dx[n, h, w, c] = sum over the taps (i, j) with (h + P - i) and (w + P - j) even and
// the dz pixel ((h + P - i) / 2, (w + P - j) / 2) in range of dz * w[i][j][c].  A strip starts at a multiple of kTW (even)
// column, so the tap of (dx column b, dz column w0 / 2 + q) is the compile-time j = b + P - 2 q.
template <typename T, int K>
__global__ void __launch_bounds__(256)
dw_dgrad_s2_kernel(const T* __restrict__ dz, const T* __restrict__ w, T* __restrict__ dx, int accumulate, int N, int H,
                   int W, int C, long xps, int OH, int OW, long zps, int tcl) {
  constexpr int VW = Traits<T>::VW, P = K / 2, QLO = -(P / 2), QHI = (kTW - 1 + P) / 2;
  static_assert(kTW % 2 == 0, "strips must start on an even column");
  const int TC = 1 << tcl, cu = threadIdx.x & (TC - 1), slot = threadIdx.x >> tcl, PIX = 256 >> tcl;
  const int cv = blockIdx.y * TC + cu;
  if (cv >= C / VW) return;
  const int c0 = cv * VW;
  const int SW = (W + kTW - 1) / kTW;
  const long nstrips = (long)N * H * SW, ngroups = (nstrips + PIX - 1) / PIX;
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long st = g * PIX + slot;
    if (st >= nstrips) continue;
    const Strip sp = strip_of(st, H, SW);  // (n, h, w0)
    float acc[kTW][VW];
#pragma unroll
    for (int b = 0; b < kTW; ++b)
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[b][e] = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int r = sp.oh + P - i;
      if (r < 0 || (r & 1) || (r >> 1) >= OH) continue;
      float wr[K][VW];
#pragma unroll
      for (int j = 0; j < K; ++j) load_vec<T>(w + (long)(i * K + j) * C + c0, wr[j]);
      const T* zr = dz + ((long)sp.n * OH + (r >> 1)) * OW * zps + c0;
#pragma unroll
      for (int qq = QLO; qq <= QHI; ++qq) {
        const int q = (sp.ow0 >> 1) + qq;
        const bool ok = q >= 0 && q < OW;
        float zv[VW];
        load_vec<T>(zr + (long)(ok ? q : 0) * zps, zv);
#pragma unroll
        for (int b = 0; b < kTW; ++b) {
          const int j = b + P - 2 * qq;
          if (j >= 0 && j < K) {
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[b][e] += (ok ? zv[e] : 0.f) * wr[j][e];
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < kTW; ++b) {
      const int wc = sp.ow0 + b;
      if (wc >= W) continue;
      T* xp = dx + (((long)sp.n * H + sp.oh) * W + wc) * xps + c0;
      float f[VW];
      if (accumulate) {
        load_vec<T>(xp, f);
#pragma unroll
        for (int e = 0; e < VW; ++e) f[e] += acc[b][e];
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) f[e] = acc[b][e];
      }
      *reinterpret_cast<uint4*>(xp) = pack<T>(f);
    }
  }
}

// weight-grad partials: part[blockIdx.x][(i * K + j) * C + c] = sum over this block's dz pixels of
// x[n, oh * S - P + i, ow * S - P + j, c] * dz[n, oh, ow, c].  Every block writes its whole row slice (zeros without work).
template <typename T, int K, int S>
__global__ void __launch_bounds__(256)
dw_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dz, float* __restrict__ part, int N, int H, int W, int C,
                long xps, int OH, int OW, long zps, int tcl) {
  constexpr int P = K / 2, NC = (kTW - 1) * S + K;
  const int TC = 1 << tcl, cu = threadIdx.x & (TC - 1), slot = threadIdx.x >> tcl, PIX = 256 >> tcl;
  const int c4 = blockIdx.y * TC + cu;
  const bool cok = c4 < C / kWgC;
  const int c0 = cok ? c4 * kWgC : 0;
  const int SW = (OW + kTW - 1) / kTW;
  const long nstrips = (long)N * OH * SW, ngroups = (nstrips + PIX - 1) / PIX;
  float acc[K][K][kWgC];
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int e = 0; e < kWgC; ++e) acc[i][j][e] = 0.f;
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long st = g * PIX + slot;
    if (!cok || st >= nstrips) continue;
    const Strip sp = strip_of(st, OH, SW);
    float zv[kTW][kWgC];
    const T* zr = dz + ((long)sp.n * OH + sp.oh) * OW * zps + c0;
#pragma unroll
    for (int b = 0; b < kTW; ++b) {
      const bool ok = sp.ow0 + b < OW;
      load4(zr + (long)(ok ? sp.ow0 + b : sp.ow0) * zps, zv[b]);
#pragma unroll
      for (int e = 0; e < kWgC; ++e) zv[b][e] = ok ? zv[b][e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int ih = sp.oh * S - P + i;
      if (ih < 0 || ih >= H) continue;
      const T* xr = x + ((long)sp.n * H + ih) * W * xps + c0;
#pragma unroll
      for (int jj = 0; jj < NC; ++jj) {
        const int iw = sp.ow0 * S - P + jj;
        const bool ok = iw >= 0 && iw < W;
        float xv[kWgC];
        load4(xr + (long)(ok ? iw : 0) * xps, xv);
#pragma unroll
        for (int b = 0; b < kTW; ++b) {
          const int j = jj - b * S;
          if (j >= 0 && j < K) {
#pragma unroll
            for (int e = 0; e < kWgC; ++e) acc[i][j][e] += (ok ? xv[e] : 0.f) * zv[b][e];
          }
        }
      }
    }
  }
  __shared__ float red[4][32 * kWgC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = TC * kWgC;
  float* row = part + (long)blockIdx.x * K * K * C;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
      for (int e = 0; e < kWgC; ++e) {
        const float a = unit_sum(acc[i][j][e], tcl);
        if (lane < TC) red[wave][lane * kWgC + e] = a;
      }
      __syncthreads();
      if ((int)threadIdx.x < nch) {
        const int ch = blockIdx.y * nch + threadIdx.x;
        if (ch < C) row[(long)(i * K + j) * C + ch] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
      }
      __syncthreads();
    }
  }
}

// The weight-grad of a wide filter (K = 7), one filter row per blockIdx.z: K * kWgC accumulators per thread instead of
// K * K * kWgC (196 at K = 7, which would not stay in registers).  Same partial rows as dw_wgrad_kernel, RL floats apart:
// part[blockIdx.x][(i * K + j) * C + c] for i = blockIdx.z.  bias != 0: the blocks of filter row 0 also write the bias
// gradient's share part[blockIdx.x][K * K * C + c] = sum over this block's dz pixels of dz[n, oh, ow, c] (RL >= (K * K + 1) * C).
template <typename T, int K, int S>
__global__ void __launch_bounds__(256)
dw_wgrad_row_kernel(const T* __restrict__ x, const T* __restrict__ dz, float* __restrict__ part, long RL, int bias, int N,
                    int H, int W, int C, long xps, int OH, int OW, long zps, int tcl) {
  constexpr int P = K / 2, NC = (kTW - 1) * S + K;
  const int TC = 1 << tcl, cu = threadIdx.x & (TC - 1), slot = threadIdx.x >> tcl, PIX = 256 >> tcl;
  const int c4 = blockIdx.y * TC + cu, i = blockIdx.z;
  const bool cok = c4 < C / kWgC, bsum = bias && i == 0;  // bsum is block-uniform
  const int c0 = cok ? c4 * kWgC : 0;
  const int SW = (OW + kTW - 1) / kTW;
  const long nstrips = (long)N * OH * SW, ngroups = (nstrips + PIX - 1) / PIX;
  float acc[K][kWgC], bacc[kWgC];
#pragma unroll
  for (int e = 0; e < kWgC; ++e) {
    bacc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j][e] = 0.f;
  }
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long st = g * PIX + slot;
    if (!cok || st >= nstrips) continue;
    const Strip sp = strip_of(st, OH, SW);
    float zv[kTW][kWgC];
    const T* zr = dz + ((long)sp.n * OH + sp.oh) * OW * zps + c0;
#pragma unroll
    for (int b = 0; b < kTW; ++b) {
      const bool ok = sp.ow0 + b < OW;
      load4(zr + (long)(ok ? sp.ow0 + b : sp.ow0) * zps, zv[b]);
#pragma unroll
      for (int e = 0; e < kWgC; ++e) zv[b][e] = ok ? zv[b][e] : 0.f;
    }
    if (bsum) {
#pragma unroll
      for (int b = 0; b < kTW; ++b)
#pragma unroll
        for (int e = 0; e < kWgC; ++e) bacc[e] += zv[b][e];
    }
    const int ih = sp.oh * S - P + i;
    if (ih < 0 || ih >= H) continue;
    const T* xr = x + ((long)sp.n * H + ih) * W * xps + c0;
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) {
      const int iw = sp.ow0 * S - P + jj;
      const bool ok = iw >= 0 && iw < W;
      float xv[kWgC];
      load4(xr + (long)(ok ? iw : 0) * xps, xv);
#pragma unroll
      for (int b = 0; b < kTW; ++b) {
        const int j = jj - b * S;
        if (j >= 0 && j < K) {
#pragma unroll
          for (int e = 0; e < kWgC; ++e) acc[j][e] += (ok ? xv[e] : 0.f) * zv[b][e];
        }
      }
    }
  }
  __shared__ float red[4][32 * kWgC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = TC * kWgC;
  float* row = part + (long)blockIdx.x * RL;
#pragma unroll
  for (int j = 0; j <= K; ++j) {
    if (j == K && !bsum) break;
#pragma unroll
    for (int e = 0; e < kWgC; ++e) {
      const float a = unit_sum(j < K ? acc[j % K][e] : bacc[e], tcl);  // j == K: the bias share
      if (lane < TC) red[wave][lane * kWgC + e] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < nch) {
      const int ch = blockIdx.y * nch + threadIdx.x;
      if (ch < C) row[(long)(j < K ? i * K + j : K * K) * C + ch] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- 9 x 9, stride 1, padding 4 (ConvMix, models/cspcm.py:29)
// The K <= 7 kernels hold a whole filter row (K vectors) next to the kTW accumulators; at K = 7 in bf16 that already
// takes every VGPR.  The 9 x 9 bodies load the filter per column instead: the input columns of a filter row are walked
// once, column jj loads the one new filter vector w[i][jj] into a ring of kTW vectors (the taps jj - kTW + 1 .. jj are
// all an output of the strip still needs), and the filter rows are a real loop, not unrolled code.  Live per thread:
// kTW accumulators + kTW filter vectors + one input vector.  No LDS, no barrier in the main loop ("Depthwise
// 9 x 9").  Bounds as above: rows out of range are skipped, columns clamped to column 0 and zeroed, stores predicated.
//   EPI_STATS / EPI_ACT / EPI_ACC: as dw_conv_kernel
//   EPI_ACTBN: y = act(T(acc + bias)) * scale + shift (+ res)     (scale / shift nullable together)
template <typename T, bool FLIP, int EPI>
__global__ void __launch_bounds__(256)
dw9_conv_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
                float* __restrict__ psum, float* __restrict__ psq, int N, int IH, int IW, int C, long ips, int OH, int OW,
                long ops, int tcl, const float* __restrict__ scale, const float* __restrict__ shift, int act,
                const T* __restrict__ res, long rps, int accumulate) {
  constexpr int VW = Traits<T>::VW, K = 9, P = 4, NC = kTW - 1 + K;
  const int TC = 1 << tcl, cu = threadIdx.x & (TC - 1), slot = threadIdx.x >> tcl, PIX = 256 >> tcl;
  const int cv = blockIdx.y * TC + cu;
  const bool cok = cv < C / VW;
  const int c0 = cok ? cv * VW : 0;
  const int SW = (OW + kTW - 1) / kTW;
  const long nstrips = (long)N * OH * SW, ngroups = (nstrips + PIX - 1) / PIX;
  float s1[VW], s2[VW], bs[VW], sc[VW], sh[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) { s1[e] = 0.f; s2[e] = 0.f; bs[e] = 0.f; sc[e] = 1.f; sh[e] = 0.f; }
  if (EPI != EPI_ACC && bias && cok) ldf<VW>(bias + c0, bs);
  if ((EPI == EPI_ACT || EPI == EPI_ACTBN) && scale && cok) {
    ldf<VW>(scale + c0, sc);
    ldf<VW>(shift + c0, sh);
  }
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long st = g * PIX + slot;
    if (!cok || st >= nstrips) continue;
    const Strip sp = strip_of(st, OH, SW);
    float acc[kTW][VW];
#pragma unroll
    for (int b = 0; b < kTW; ++b)
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[b][e] = 0.f;
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
      const int ih = sp.oh - P + i;
      if (ih < 0 || ih >= IH) continue;
      const T* wr = w + (long)((FLIP ? K - 1 - i : i) * K) * C + c0;
      const T* xr = x + ((long)sp.n * IH + ih) * IW * ips + c0;
      float ring[kTW][VW];  // ring[j % kTW] = w[i][j] for the taps j of the last kTW columns
#pragma unroll
      for (int jj = 0; jj < NC; ++jj) {
        const int iw = sp.ow0 - P + jj;
        const bool ok = iw >= 0 && iw < IW;
        float xv[VW];
        load_vec<T>(xr + (long)(ok ? iw : 0) * ips, xv);
        if (jj < K) load_vec<T>(wr + (long)(FLIP ? K - 1 - jj : jj) * C, ring[jj % kTW]);
#pragma unroll
        for (int e = 0; e < VW; ++e) xv[e] = ok ? xv[e] : 0.f;
#pragma unroll
        for (int b = 0; b < kTW; ++b) {
          const int j = jj - b;
          if (j >= 0 && j < K) {
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[b][e] += xv[e] * ring[j % kTW][e];
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < kTW; ++b) {
      const int ow = sp.ow0 + b;
      if (ow >= OW) continue;
      const long pix = ((long)sp.n * OH + sp.oh) * OW + ow;
      T* yp = y + pix * ops + c0;
      float f[VW];
      if (EPI == EPI_ACC) {
        if (accumulate) {
          load_vec<T>(yp, f);
#pragma unroll
          for (int e = 0; e < VW; ++e) f[e] += acc[b][e];
        } else {
#pragma unroll
          for (int e = 0; e < VW; ++e) f[e] = acc[b][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) f[e] = to_f(from_f<T>(acc[b][e] + bs[e]));  // the value as stored
        if (EPI == EPI_STATS) {
#pragma unroll
          for (int e = 0; e < VW; ++e) { s1[e] += f[e]; s2[e] += f[e] * f[e]; }
        } else {
          if (EPI == EPI_ACTBN) act_fwd_n<VW>(act, f);
          if (scale) {
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] = f[e] * sc[e] + sh[e];
          }
          if (EPI == EPI_ACT) act_fwd_n<VW>(act, f);
          if (res) {
            float r[VW];
            load_vec<T>(res + pix * rps + c0, r);
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] += r[e];
          }
        }
      }
      *reinterpret_cast<uint4*>(yp) = pack<T>(f);
    }
  }
  if (EPI == EPI_STATS && psum) write_rows<VW>(s1, s2, tcl, C, psum, psq);  // block-uniform
}

// 9 x 9 weight-grad partials, one filter row per blockIdx.z and one 16-byte channel vector per thread: 9 * VW
// accumulators.  The strip's kTW dz vectors stay in registers while the kTW + 8 input columns of the row stream past;
// part[blockIdx.x][(i * 9 + j) * C + c] for i = blockIdx.z, rows 81 * C floats apart.  Every block writes its whole row
// slice (zeros without work), the rows are summed in row order by dw_wgrad_finalize_kernel.
template <typename T>
__global__ void __launch_bounds__(256)
dw9_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dz, float* __restrict__ part, int N, int H, int W, int C,
                 long xps, int OH, int OW, long zps, int tcl) {
  constexpr int VW = Traits<T>::VW, K = 9, P = 4, NC = kTW - 1 + K;
  const int TC = 1 << tcl, cu = threadIdx.x & (TC - 1), slot = threadIdx.x >> tcl, PIX = 256 >> tcl;
  const int cv = blockIdx.y * TC + cu, i = blockIdx.z;
  const bool cok = cv < C / VW;
  const int c0 = cok ? cv * VW : 0;
  const int SW = (OW + kTW - 1) / kTW;
  const long nstrips = (long)N * OH * SW, ngroups = (nstrips + PIX - 1) / PIX;
  float acc[K][VW];
#pragma unroll
  for (int j = 0; j < K; ++j)
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[j][e] = 0.f;
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long st = g * PIX + slot;
    if (!cok || st >= nstrips) continue;
    const Strip sp = strip_of(st, OH, SW);
    const int ih = sp.oh - P + i;
    if (ih < 0 || ih >= H) continue;
    float zv[kTW][VW];
    const T* zr = dz + ((long)sp.n * OH + sp.oh) * OW * zps + c0;
#pragma unroll
    for (int b = 0; b < kTW; ++b) {
      const bool ok = sp.ow0 + b < OW;
      load_vec<T>(zr + (long)(ok ? sp.ow0 + b : sp.ow0) * zps, zv[b]);
#pragma unroll
      for (int e = 0; e < VW; ++e) zv[b][e] = ok ? zv[b][e] : 0.f;
    }
    const T* xr = x + ((long)sp.n * H + ih) * W * xps + c0;
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) {
      const int iw = sp.ow0 - P + jj;
      const bool ok = iw >= 0 && iw < W;
      float xv[VW];
      load_vec<T>(xr + (long)(ok ? iw : 0) * xps, xv);
#pragma unroll
      for (int e = 0; e < VW; ++e) xv[e] = ok ? xv[e] : 0.f;
#pragma unroll
      for (int b = 0; b < kTW; ++b) {
        const int j = jj - b;
        if (j >= 0 && j < K) {
#pragma unroll
          for (int e = 0; e < VW; ++e) acc[j][e] += xv[e] * zv[b][e];
        }
      }
    }
  }
  __shared__ float red[4][32 * VW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = TC * VW;
  float* row = part + (long)blockIdx.x * K * K * C;
#pragma unroll
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const float a = unit_sum(acc[j][e], tcl);
      if (lane < TC) red[wave][lane * VW + e] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < nch) {
      const int ch = blockIdx.y * nch + threadIdx.x;
      if (ch < C) row[(long)(i * K + j) * C + ch] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
    __syncthreads();
  }
}

// dw[c][tap] (torch OIHW of a (C, 1, K, K) weight) = (accumulate ? dw : 0) + the partial rows (RL floats apart) summed
// in row order; db (nullable): the same for the bias gradient, whose share of a row follows its KK * C filter taps
__global__ void __launch_bounds__(256)
dw_wgrad_finalize_kernel(const float* __restrict__ part, int rows, int C, int KK, long RL, float* __restrict__ dw,
                         int accumulate, float* __restrict__ db, int db_accumulate) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= (KK + (db ? 1 : 0)) * C) return;
  const int tap = e / C, c = e - tap * C;
  float s = 0.f;
  for (int p = 0; p < rows; ++p) s += part[(long)p * RL + e];
  if (tap == KK) {
    db[c] = db_accumulate ? db[c] + s : s;
    return;
  }
  const long o = (long)c * KK + tap;
  dw[o] = accumulate ? dw[o] + s : s;
}

bool geom_ok(int dtype, int N, int H, int W, int C, long xps, int KH, int KW, int S, int P, int OH, int OW, long zps) {
  if (dtype != 0 && dtype != 1) return false;
  if (N < 1 || H < 1 || W < 1 || C < vec_width(dtype) || !rows_fit(C, {xps, zps})) return false;
  if (KH != KW || (KH != 3 && KH != 5 && KH != 7 && KH != 9) || (S != 1 && S != 2) || (KH >= 7 && S != 1) || P != KH / 2) return false;
  if (OH != (H + 2 * P - KH) / S + 1 || OW != (W + 2 * P - KW) / S + 1 || OH < 1 || OW < 1) return false;
  if ((long)N * H * W >= (1L << 31) || (long)N * OH * OW >= (1L << 31)) return false;
  return true;
}

// f(Int<K>{}, Int<S>{}) for the (K, S) pairs geom_ok admits (K = 7 / 9 are stride 1 only), -1 for any other.  f is a
// generic lambda that holds the launch and returns the entry's int.
template <typename F> int by_k_s(int K, int S, F&& f) {
  return by_int<3, 5, 7, 9>(K, -1, [&](auto k) {
    if constexpr (decltype(k)::value >= 7) return by_int<1>(S, -1, [&](auto s) { return f(k, s); });
    else return by_int<1, 2>(S, -1, [&](auto s) { return f(k, s); });
  });
}

// the correlation kernel of (K, S): the 9 x 9 has a body of its own
template <typename T, int K, int S, bool FLIP, int EPI> constexpr auto conv_kernel() {
  if constexpr (K == 9) return &dw9_conv_kernel<T, FLIP, EPI>;
  else return &dw_conv_kernel<T, K, S, FLIP, EPI>;
}

template <typename T, int EPI>
int launch_fwd(const T* x, const T* w, const float* bias, T* y, float* psum, float* psq, int N, int H, int W, int C,
               long xps, int KH, int S, int OH, int OW, long yps, const float* scale, const float* shift, int act,
               const T* res, long rps, hipStream_t st) {
  constexpr int VW = Traits<T>::VW;
  const int tcl = tile_log2(C / VW);
  const dim3 grid = tile_grid(part_rows((long)N * OH * OW, kFwdRowCap), C / VW, tcl);
  return by_k_s(KH, S, [&](auto k, auto s) {
    constexpr int K = decltype(k)::value, S_ = decltype(s)::value;
    if constexpr (EPI == EPI_ACTBN && K != 9) {  // the act-then-BN epilogue exists for the 9 x 9 only
      return -1;
    } else {
      return launch(conv_kernel<T, K, S_, false, EPI>(), grid, st, x, w, bias, y, psum, psq, N, H, W, C, xps, OH, OW, yps,
                    tcl, scale, shift, act, res, rps, 0);
    }
  });
}

template <typename T>
int launch_dgrad(const T* dz, const T* w, T* dx, int accumulate, int N, int H, int W, int C, long xps, int KH, int S,
                 int OH, int OW, long zps, hipStream_t st) {
  constexpr int VW = Traits<T>::VW;
  const int tcl = tile_log2(C / VW);
  const dim3 grid = tile_grid(part_rows((long)N * H * W, kFwdRowCap), C / VW, tcl);
  return by_k_s(KH, S, [&](auto k, auto s) {
    constexpr int K = decltype(k)::value, S_ = decltype(s)::value;
    if constexpr (S_ == 1) {
      // correlation of dz (OH x OW) with the flipped filter, same padding (P = K / 2, K odd), output H x W
      return launch(conv_kernel<T, K, 1, true, EPI_ACC>(), grid, st, dz, w, nullptr, dx, nullptr, nullptr, N, OH, OW, C,
                    zps, H, W, xps, tcl, nullptr, nullptr, 0, nullptr, 0, accumulate);
    } else {
      return launch(dw_dgrad_s2_kernel<T, K>, grid, st, dz, w, dx, accumulate, N, H, W, C, xps, OH, OW, zps, tcl);
    }
  });
}

// RL: floats between partial rows; bias: the rows also carry the bias gradient's share (K = 7 only, checked by wgrad)
template <typename T>
int launch_wgrad(const T* x, const T* dz, float* part, long RL, int bias, int N, int H, int W, int C, long xps, int KH,
                 int S, int OH, int OW, long zps, hipStream_t st) {
  const int rows = part_rows((long)N * OH * OW, kWgRowCap);
  return by_k_s(KH, S, [&](auto k, auto s) {
    constexpr int K = decltype(k)::value, S_ = decltype(s)::value;
    constexpr int CU = K == 9 ? Traits<T>::VW : kWgC;  // channels per thread
    const int tcl = tile_log2(C / CU);
    const dim3 grid = tile_grid(rows, C / CU, tcl, K >= 7 ? K : 1);  // K >= 7: one filter row per blockIdx.z
    if constexpr (K == 9) {
      return launch(dw9_wgrad_kernel<T>, grid, st, x, dz, part, N, H, W, C, xps, OH, OW, zps, tcl);
    } else if constexpr (K == 7) {
      return launch(dw_wgrad_row_kernel<T, 7, 1>, grid, st, x, dz, part, RL, bias, N, H, W, C, xps, OH, OW, zps, tcl);
    } else {
      return launch(dw_wgrad_kernel<T, K, S_>, grid, st, x, dz, part, N, H, W, C, xps, OH, OW, zps, tcl);
    }
  });
}

// the one-launch inference forwards: EPI_ACT, or EPI_ACTBN (9 x 9 only)
template <int EPI>
int fwd_epilogue(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int C, long xps,
                 int KH, int KW, int S, int P, int OH, int OW, long yps, const float* scale, const float* shift, int act,
                 const void* res, long rps, void* stream) {
  if ((EPI == EPI_ACTBN && KH != 9) || !dmy_dwconv_ok(dtype, x, w, y, N, H, W, C, C, C, xps, KH, KW, S, P, OH, OW, yps) ||
      (scale == nullptr) != (shift == nullptr) || (res && (!vec_ok(vec_width(dtype), C, {rps}, {res}) || rps < C)))
    return -1;
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch_fwd<T, EPI>((const T*)x, (const T*)w, bias, (T*)y, nullptr, nullptr, N, H, W, C, xps, KH, S, OH, OW, yps,
                              scale, shift, act, (const T*)res, rps, (hipStream_t)stream);
  });
}

int wgrad(int dtype, const void* x, const void* dz, float* part, int bias, int N, int H, int W, int C, long xps, int KH,
          int KW, int S, int P, int OH, int OW, long zps, void* stream) {
  if ((bias && KH != 7) || !dmy_dwconv_ok(dtype, x, part, dz, N, H, W, C, C, C, xps, KH, KW, S, P, OH, OW, zps)) return -1;
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch_wgrad<T>((const T*)x, (const T*)dz, part, ((long)KH * KW + bias) * C, bias, N, H, W, C, xps, KH, S, OH, OW,
                           zps, (hipStream_t)stream);
  });
}

}  // namespace

// the bases are checked for alignment only: a null base passes this query
DMY_API int dmy_dwconv_ok(int dtype, const void* x, const void* w, const void* z, int N, int H, int W, int C, int K,
                          int groups, long xps, int KH, int KW, int S, int P, int OH, int OW, long zps) {
  if (groups != C || K != C || !vec_ok(vec_width(dtype), C, {xps, zps}, {}, {x, w, z})) return 0;
  return geom_ok(dtype, N, H, W, C, xps, KH, KW, S, P, OH, OW, zps) ? 1 : 0;
}

DMY_API int dmy_dwconv_fwd_rows(long M, int C) {
  (void)C;
  return part_rows(M, kFwdRowCap);
}

DMY_API int dmy_dwconv_fwd(int dtype, const void* x, const void* w, const float* bias, void* z, float* psum, float* psq,
                           int N, int H, int W, int C, long xps, int KH, int KW, int S, int P, int OH, int OW, long zps,
                           void* stream) {
  if (!dmy_dwconv_ok(dtype, x, w, z, N, H, W, C, C, C, xps, KH, KW, S, P, OH, OW, zps) || (psum == nullptr) != (psq == nullptr))
    return -1;
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch_fwd<T, EPI_STATS>((const T*)x, (const T*)w, bias, (T*)z, psum, psq, N, H, W, C, xps, KH, S, OH, OW, zps,
                                    nullptr, nullptr, 0, nullptr, 0, (hipStream_t)stream);
  });
}

DMY_API int dmy_dwconv_fwd_act(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W,
                               int C, long xps, int KH, int KW, int S, int P, int OH, int OW, long yps, const float* scale,
                               const float* shift, int act, const void* res, long rps, void* stream) {
  return fwd_epilogue<EPI_ACT>(dtype, x, w, bias, y, N, H, W, C, xps, KH, KW, S, P, OH, OW, yps, scale, shift, act, res, rps,
                               stream);
}

DMY_API int dmy_dwconv_fwd_actbn(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W,
                                 int C, long xps, int KH, int KW, int S, int P, int OH, int OW, long yps,
                                 const float* scale, const float* shift, int act, const void* res, long rps,
                                 void* stream) {
  return fwd_epilogue<EPI_ACTBN>(dtype, x, w, bias, y, N, H, W, C, xps, KH, KW, S, P, OH, OW, yps, scale, shift, act, res,
                                 rps, stream);
}

DMY_API int dmy_dwconv_dgrad(int dtype, const void* dz, const void* w, void* dx, int accumulate, int N, int H, int W,
                             int C, long xps, int KH, int KW, int S, int P, int OH, int OW, long zps, void* stream) {
  if (!dmy_dwconv_ok(dtype, dx, w, dz, N, H, W, C, C, C, xps, KH, KW, S, P, OH, OW, zps)) return -1;
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch_dgrad<T>((const T*)dz, (const T*)w, (T*)dx, accumulate, N, H, W, C, xps, KH, S, OH, OW, zps,
                           (hipStream_t)stream);
  });
}

DMY_API int dmy_dwconv_wgrad_rows(long M, int C) {
  (void)C;
  return part_rows(M, kWgRowCap);
}

DMY_API int dmy_dwconv_wgrad(int dtype, const void* x, const void* dz, float* part, int N, int H, int W, int C, long xps,
                             int KH, int KW, int S, int P, int OH, int OW, long zps, void* stream) {
  return wgrad(dtype, x, dz, part, 0, N, H, W, C, xps, KH, KW, S, P, OH, OW, zps, stream);
}

DMY_API int dmy_dwconv_wgrad_bias(int dtype, const void* x, const void* dz, float* part, int N, int H, int W, int C,
                                  long xps, int KH, int KW, int S, int P, int OH, int OW, long zps, void* stream) {
  return wgrad(dtype, x, dz, part, 1, N, H, W, C, xps, KH, KW, S, P, OH, OW, zps, stream);
}

DMY_API int dmy_dwconv_wgrad_finalize(const float* part, int rows, int C, int KH, int KW, float* dw, int accumulate,
                                      void* stream) {
  if (rows < 1 || C < 1 || KH < 1 || KW < 1) return -1;
  const int KK = KH * KW;
  return launch(dw_wgrad_finalize_kernel, ceil_div((long)KK * C, 256), stream, part, rows, C, KK, (long)KK * C, dw,
                accumulate, nullptr, 0);
}

DMY_API int dmy_dwconv_wgrad_bias_finalize(const float* part, int rows, int C, int KH, int KW, float* dw, int accumulate,
                                           float* dbias, int bias_accumulate, void* stream) {
  if (rows < 1 || C < 1 || KH < 1 || KW < 1 || !dbias) return -1;
  const int KK = KH * KW;
  return launch(dw_wgrad_finalize_kernel, ceil_div((long)(KK + 1) * C, 256), stream, part, rows, C, KK,
                (long)(KK + 1) * C, dw, accumulate, dbias, bias_accumulate);
}

