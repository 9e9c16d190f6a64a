// Implicit-GEMM weight-grad for gfx950 and the weight layout passes (OIHW fp32 masters <-> the GEMM operand copies),
// NHWC activations.  Forward and data-grad are conv.hip; conv_core.h has the device primitives and conv_plan.h the
// host code (geometry, kernel codes, plan records) that both files use.
//
//   wgrad: C[m=cout][n=(kh,kw,ci)] = sum_pix dY[pix][m] * X[pix shifted][ci]       split-K over pixels
// v2 staging: global -> registers -> LDS, two stages, one barrier per BK-deep step; "k-major" tiles ([k][row], as
//   loaded from NHWC) are read with ds_read_b64_tr_b16, the 16-B chunks XOR-swizzled per k-row so the transposed reads
//   are bank-conflict free (kmaj_off).  The LDS-DMA kernels (v3, v3n, v4, tap-fused) fill the same images.
// Epilogues go through LDS: every fp32 atomic (or deterministic workspace store) is part of a 256-B wave segment.
#include "conv_plan.h"
#include <cmath>

namespace {

// weight-grad epilogue store: deterministic workspace slot of this split, or an fp32 atomic into dw
DEV void wgrad_out(const Geom& g, float* dw, int split, long idx, float v) {
  if (g.dws != nullptr) g.dws[(long)split * g.dws_slab + idx] = v;
  else atomicAdd(dw + idx, v);
}

// weight-grad GEMM column n = (kh * KW + kw) * C + c -> its offset inside one output row of dw
DEV long wgrad_col(const Geom& g, int n) {
  if (!g.oihw) return n;
  const int taps = g.KH * g.KW;
  return (long)(n % g.C) * taps + n / g.C;
}

// ---------------------------------------------------------------- weight-grad loader (k-major A and B)
// A[k=pix][m=co] = dy[pix][co];  B[k=pix][n=(kh,kw,ci)] = x[pix shifted by (kh,kw)][ci]
template <typename T, int BM, int BN, bool VECA, bool VECB> struct WgradLoader {
  using TT = Tile<T, BM, BN, true, true>;
  static constexpr int BK = TT::BK, VW = TT::VW;
  static constexpr int AV = BM / VW, BV = BN / VW;  // vectors per pixel row
  static constexpr int CA = BK * AV / NT, CB = BK * BV / NT;
  const T* x; const T* dy; Geom g; long NP; int Ntot, m0, n0;
  // the n -> (kh, kw, ci) decomposition is fixed per thread across K-steps
  int b_kh[CB], b_kw[CB], b_ci[CB];
  bool b_ok[CB];
  DEV WgradLoader(const T* x_, const T* dy_, const Geom& g_, int m0_, int n0_) : x(x_), dy(dy_), g(g_), m0(m0_), n0(n0_) {
    NP = (long)g.N * g.OH * g.OW;
    Ntot = g.KH * g.KW * g.C;
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      const int c = threadIdx.x + i * NT;
      const int n = n0 + (c % BV) * VW;
      b_ok[i] = n < Ntot;
      b_ci[i] = n % g.C;
      const int u = n / g.C;
      b_kw[i] = u % g.KW;
      b_kh[i] = u / g.KW;
    }
  }
  DEV T ld_b1(long pix, int n) const {
    if (pix >= NP || n >= Ntot) return from_f<T>(0.f);
    const int ow = (int)(pix % g.OW);
    const long t = pix / g.OW;
    const int oh = (int)(t % g.OH), b = (int)(t / g.OH);
    const int ci = n % g.C, u = n / g.C, kw = u % g.KW, kh = u / g.KW;
    const int ih = oh * g.S - g.P + kh, iw = ow * g.S - g.P + kw;
    if (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) return from_f<T>(0.f);
    return x[(((long)b * g.H + ih) * g.W + iw) * g.xps + ci];
  }
  DEV void load(int kt, uint4* ra, uint4* rb) const {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int c = threadIdx.x + i * NT;
      const long pix = (long)kt * BK + c / AV;
      const int co = m0 + (c % AV) * VW;
      if (VECA) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pix < NP && co < g.K) v = *reinterpret_cast<const uint4*>(dy + pix * g.yps + co);
        ra[i] = v;
      } else {
        T* e = reinterpret_cast<T*>(&ra[i]);
#pragma unroll
        for (int j = 0; j < VW; ++j) e[j] = (pix < NP && co + j < g.K) ? dy[pix * g.yps + co + j] : from_f<T>(0.f);
      }
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      const int c = threadIdx.x + i * NT;
      const long pix = (long)kt * BK + c / BV;
      if (VECB) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pix < NP && b_ok[i]) {
          const int ow = (int)(pix % g.OW);
          const long t = pix / g.OW;
          const int oh = (int)(t % g.OH), b = (int)(t / g.OH);
          const int ih = oh * g.S - g.P + b_kh[i], iw = ow * g.S - g.P + b_kw[i];
          if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
            v = *reinterpret_cast<const uint4*>(x + (((long)b * g.H + ih) * g.W + iw) * g.xps + b_ci[i]);
        }
        rb[i] = v;
      } else {
        T* e = reinterpret_cast<T*>(&rb[i]);
        const int n = n0 + (c % BV) * VW;
#pragma unroll
        for (int j = 0; j < VW; ++j) e[j] = ld_b1(pix, n + j);
      }
    }
  }
  DEV void store(T* As, T* Bs, const uint4* ra, const uint4* rb) const {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int c = threadIdx.x + i * NT;
      st_k<T, BM>(As, c / AV, (c % AV) * VW, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      const int c = threadIdx.x + i * NT;
      st_k<T, BN>(Bs, c / BV, (c % BV) * VW, rb[i]);
    }
  }
};

template <typename T, int BM, int BN, bool VECA, bool VECB>
__global__ void __launch_bounds__(NT) conv_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                        float* __restrict__ dw, int kt_per_split, Geom g, int gm,
                                                        int gn) {
  using TT = Tile<T, BM, BN, true, true>;
  __shared__ __attribute__((aligned(16))) char smem[TT::LDS_BYTES];
  T* lds = reinterpret_cast<T*>(smem);
  // (tile, split) from the linear dispatch id: consecutive logical ids share an XCD, so all tiles of
  // a split (which read the same pixel chunk) run on one XCD and share its L2
  const int lin = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int tile = lin % (gm * gn), split = lin / (gm * gn);
  const int tm = tile / gn, tn = tile % gn;
  const int m0 = tm * BM, n0 = tn * BN;
  WgradLoader<T, BM, BN, VECA, VECB> ld(x, dy, g, m0, n0);
  const long NP = (long)g.N * g.OH * g.OW;
  const int nk = (int)((NP + TT::BK - 1) / TT::BK);
  const int kt0 = split * kt_per_split;
  const int kt1 = min(nk, kt0 + kt_per_split);
  f32x4 acc[TT::TM][TT::TN];
  zero_acc<BM, BN>(acc);
  mainloop<T, BM, BN, true, true>(ld, kt0, kt1, lds, acc);
  __syncthreads();
  // stage the fp32 partial tile in LDS, then atomics in contiguous 256-B wave segments
  float* ct = reinterpret_cast<float*>(smem);
  constexpr int RS = BN + 4;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid >> 1, wn = wid & 1;
#pragma unroll
  for (int i = 0; i < TT::TM; ++i)
#pragma unroll
    for (int j = 0; j < TT::TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(wm * (BM / 2) + i * 16 + 4 * (lane >> 4) + r) * RS + wn * (BN / 2) + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  const int Ntot = g.KH * g.KW * g.C;
  static_assert((NT) % BN == 0, "epilogue column must be fixed per thread");
  const int c = threadIdx.x % BN, n = n0 + c;
  const long coff = wgrad_col(g, n);
  for (int e = threadIdx.x; e < BM * BN; e += NT) {
    const int row = e / BN, m = m0 + row;
    if (m < g.K && n < Ntot) wgrad_out(g, dw, split, (long)m * Ntot + coff, ct[row * RS + c]);
  }
}

// OIHW fp32 master weights -> T OHWI (forward B operand, input channels padded to Cp with zeros)
// and T IHWO (data-grad B operand).
template <typename T>
__global__ void wprep_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wt, int K, int C, int Cp,
                             int KH, int KW) {
  const long total = (long)K * Cp * KH * KW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cp);
    long t = i / Cp;
    const int kw = (int)(t % KW);
    t /= KW;
    const int kh = (int)(t % KH);
    const int k = (int)(t / KH);
    const float v = c < C ? w[(((long)k * C + c) * KH + kh) * KW + kw] : 0.f;
    if (wf) wf[i] = from_f<T>(v);
    if (wt && c < C) wt[(((long)c * KH + kh) * KW + kw) * K + k] = from_f<T>(v);
  }
}

// Every conv weight of a model in one launch (training forward: the fp32 masters change every step):
// blockIdx.y = layer, blocks grid-stride over that layer's K*KH*KW*C elements (no channel padding).
struct WprepDesc {
  const float* w;
  void* wf;
  void* wt;
  int K, C, KH, KW;
};
// 32 (K) x 32 (C) x taps tiles through LDS: the OIHW rows are read contiguously (32 x 32 x taps floats) and both
// copies are written 32 consecutive elements at a time (OHWI along C, IHWO along K).  The elementwise form it
// replaces wrote the IHWO copy with a K-strided 2-byte scatter (1.59 ms per DMA-1536 step for 46 M weights).
// Kernels with more than 9 taps (the 6 x 6 stem) take the elementwise loop.
constexpr int kWpT = 9, kWpPitch = 32 * kWpT + 1;  // LDS row pitch (floats): odd, so the K-major reads are conflict-free
template <typename T>
__global__ void __launch_bounds__(256) wprep_multi_kernel(const WprepDesc* __restrict__ d) {
  const WprepDesc L = d[blockIdx.y];
  T* wf = reinterpret_cast<T*>(L.wf);
  T* wt = reinterpret_cast<T*>(L.wt);
  const int taps = L.KH * L.KW;
  if (taps > kWpT) {
    const long total = (long)L.K * L.C * taps;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const int c = (int)(i % L.C);
      const long t = i / L.C;
      const int tap = (int)(t % taps), k = (int)(t / taps);
      const float v = L.w[((long)k * L.C + c) * taps + tap];
      wf[i] = from_f<T>(v);
      if (wt) wt[((long)c * taps + tap) * L.K + k] = from_f<T>(v);
    }
    return;
  }
  __shared__ float s[32 * kWpPitch];  // [k][c * taps + tap]
  const int tc = (L.C + 31) / 32, nt = ((L.K + 31) / 32) * tc, row = 32 * taps;
  for (int tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const int k0 = (tile / tc) * 32, c0 = (tile % tc) * 32;
    const int nrow = min(32, L.C - c0) * taps;
    for (int e = threadIdx.x; e < 32 * row; e += 256) {
      const int kk = e / row, r = e - kk * row, k = k0 + kk;
      s[kk * kWpPitch + r] = (k < L.K && r < nrow) ? L.w[((long)k * L.C + c0) * taps + r] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * row; e += 256) {  // OHWI: (k, tap, c), c fastest
      const int cc = e & 31, t = e >> 5, tap = t % taps, kk = t / taps, k = k0 + kk, c = c0 + cc;
      if (k < L.K && c < L.C) wf[((long)k * taps + tap) * L.C + c] = from_f<T>(s[kk * kWpPitch + cc * taps + tap]);
    }
    if (wt) {
      for (int e = threadIdx.x; e < 32 * row; e += 256) {  // IHWO: (c, tap, k), k fastest
        const int kk = e & 31, t = e >> 5, tap = t % taps, cc = t / taps, k = k0 + kk, c = c0 + cc;
        if (k < L.K && c < L.C) wt[((long)c * taps + tap) * L.K + k] = from_f<T>(s[kk * kWpPitch + cc * taps + tap]);
      }
    }
    __syncthreads();
  }
}

// Stem k6 s2 p2 weights as the equivalent k3 s1 p1 conv over the space-to-depth image (dmy_image_s2d):
// ws[k][ky][kx][(dy * 2 + dx) * C + c] = w[k][c][2 ky + dy][2 kx + dx], channels [4C, Cs) zero
template <typename T>
__global__ void wprep_s2d_kernel(const float* __restrict__ w, T* __restrict__ ws, int K, int C, int Cs) {
  const long total = (long)K * 9 * Cs;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % Cs);
    const long t = i / Cs;
    const int tap = (int)(t % 9), k = (int)(t / 9);
    const int ky = tap / 3, kx = tap % 3;
    float v = 0.f;
    if (ch < 4 * C) {
      const int q = ch / C, c = ch - q * C;
      v = w[(((long)k * C + c) * 6 + 2 * ky + (q >> 1)) * 6 + 2 * kx + (q & 1)];
    }
    ws[i] = from_f<T>(v);
  }
}

// weight-grad of the s2d view [K][3][3][Cs] (GEMM order) -> the stem's OIHW [K][C][6][6] gradient
__global__ void wgrad_s2d_to_oihw_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int C, int Cs) {
  const long total = (long)K * C * 36;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int kw = (int)(i % 6), kh = (int)(i / 6 % 6), c = (int)(i / 36 % C), k = (int)(i / (36L * C));
    const int tap = (kh >> 1) * 3 + (kw >> 1), q = (kh & 1) * 2 + (kw & 1);
    dst[i] = src[((long)k * 9 + tap) * Cs + q * C + c];
  }
}

// OHWI fp32 grad accumulator (input channels padded to Cp) -> OIHW param-shaped gradient
__global__ void wgrad_to_oihw_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int C, int Cp,
                                     int KH, int KW) {
  const long total = (long)K * C * KH * KW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int kw = (int)(i % KW);
    long t = i / KW;
    int kh = (int)(t % KH);
    t /= KH;
    int c = (int)(t % C);
    int k = (int)(t / C);
    dst[i] = src[(((long)k * KH + kh) * KW + kw) * Cp + c];
  }
}

namespace v3 {
// Weight-grad: rows m = output channel, columns n = (kh, kw, ci), reduction over pixels (split-K).
// Both operands are k-major ([64 pixels][128 channels], 256-B pixel rows) in the kmaj_off layout of
// the v2 kernel (16-B chunks XOR-swizzled per pixel row, read with ds_read_b64_tr_b16).  One 1-KiB
// LDS-DMA piece = 4 pixel rows; lane l fills pixel row 4i + (l >> 4), slot l & 15, i.e. logical chunk
// (l & 15) ^ key(row), key(row) = 2 ((row & 3) | ((row >> 3) & 1) << 2): two chunk values per lane.
template <int NS>
struct WgradLds {
  static constexpr int BM = 128, BN = 128, PPW = 4;  // pieces per wave per operand (4 waves)
  const bf16* x; const bf16* dy; Geom g; long NP; int Ntot, m0, n0;
  int cA[2], cB[2];                 // logical chunk for key bit 3 = 0 / 1
  bool bok[2]; int bkh[2], bkw[2], bci[2];
  long pix[PPW]; int pb[PPW], poh[PPW], pow_[PPW];  // this lane's pixel per piece (advanced by 64 per step)
  DEV WgradLds(const bf16* x_, const bf16* dy_, const Geom& g_, int m0_, int n0_, int kt0, int wid, int lane)
      : x(x_), dy(dy_), g(g_), m0(m0_), n0(n0_) {
    NP = (long)g.N * g.OH * g.OW;
    Ntot = g.KH * g.KW * g.C;
    const int q = lane >> 4, sl = lane & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = sl ^ (2 * (q | (h << 2)));
      cA[h] = c;
      cB[h] = c;
      const int n = n0 + c * 8;
      bok[h] = n < Ntot;
      bci[h] = n % g.C;
      const int t = n / g.C;
      bkw[h] = t % g.KW;
      bkh[h] = t / g.KW;
    }
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      pix[j] = (long)kt0 * 64 + (wid * PPW + j) * 4 + q;
      const long pp = pix[j] < NP ? pix[j] : 0;
      pow_[j] = (int)(pp % g.OW);
      const long t = pp / g.OW;
      poh[j] = (int)(t % g.OH);
      pb[j] = (int)(t / g.OH);
    }
  }
  DEV void issue(char* stage, int wid) {
    const bf16* zero = reinterpret_cast<const bf16*>(g_zero_page);
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int piece = wid * PPW + j;
      const int h = (piece >> 1) & 1;  // bit 3 of the pixel row (rows 4 piece .. 4 piece + 3)
      const bool pin = pix[j] < NP;
      const int co = m0 + cA[h] * 8;
      const bf16* sa = (pin && co < g.K) ? dy + pix[j] * g.yps + co : zero;
      glds16(sa, stage + piece * 1024);
      const int ih = poh[j] * g.S - g.P + bkh[h], iw = pow_[j] * g.S - g.P + bkw[h];
      const bool okb = pin && bok[h] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
      const bf16* sb = okb ? x + (((long)pb[j] * g.H + ih) * g.W + iw) * g.xps + bci[h] : zero;
      glds16(sb, stage + 16384 + piece * 1024);
      // advance this piece's pixel by one K step (64 pixels)
      pix[j] += 64;
      pow_[j] += 64;
      while (pow_[j] >= g.OW) {
        pow_[j] -= g.OW;
        if (++poh[j] == g.OH) { poh[j] = 0; ++pb[j]; }
      }
    }
  }
};

// Buffer-descriptor form of WgradLds: every address is a 32-bit element offset advanced by adds only
// (the per-pixel 64-bit products of WgradLds cost 32 quarter-rate v_mul_lo_u32 per K step).  Per
// piece the lane tracks its pixel (pix, oh, ow), ih/iw = oh*S - P / ow*S - P and the element bases
// dyb = pix * yps and xb = ((b H + ih) W + iw) xps; a 64-pixel step adds fixed deltas and walks the
// row / image wraps.  Invalid sources get kBufOob (range-checked to zero by the hardware).
struct WgradLdsB {
  static constexpr int PPW = 4;
  __amdgpu_buffer_rsrc_t rx, rdy;
  int NP, OW, OH, H, W, S;
  int dyStep, xStep, xWrapOW, xRow, xImg;   // uniform element deltas
  int co[2], tap[2], bkh[2], bkw[2];        // per lane half: dy column / x tap offset, tap
  bool cok[2], bok[2];
  int pix[PPW], oh[PPW], ow[PPW], ih[PPW], iw[PPW], dyb[PPW], xb[PPW];
  DEV WgradLdsB(const bf16* x, const bf16* dy, const Geom& g, int m0, int n0, int kt0, int wid, int lane,
                unsigned xbytes, unsigned dybytes)
      : OW(g.OW), OH(g.OH), H(g.H), W(g.W), S(g.S) {
    rx = make_rsrc(x, xbytes);
    rdy = make_rsrc(dy, dybytes);
    NP = g.N * g.OH * g.OW;
    const int Ntot = g.KH * g.KW * g.C, xps = (int)g.xps, yps = (int)g.yps;
    dyStep = 64 * yps;
    xStep = 64 * g.S * xps;
    xWrapOW = g.OW * g.S * xps;
    xRow = g.S * g.W * xps;
    xImg = (g.H - g.OH * g.S) * g.W * xps;
    const int q = lane >> 4, sl = lane & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = sl ^ (2 * (q | (h << 2)));
      co[h] = m0 + c * 8;
      cok[h] = co[h] < g.K;
      const int n = n0 + c * 8;
      bok[h] = n < Ntot;
      const int nn = bok[h] ? n : 0;
      const int ci = nn % g.C, t = nn / g.C;
      bkw[h] = t % g.KW;
      bkh[h] = t / g.KW;
      tap[h] = (bkh[h] * g.W + bkw[h]) * xps + ci;
    }
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      pix[j] = kt0 * 64 + (wid * PPW + j) * 4 + q;
      const int pp = pix[j] < NP ? pix[j] : 0;
      ow[j] = pp % g.OW;
      const int t = pp / g.OW;
      oh[j] = t % g.OH;
      const int b = t / g.OH;
      ih[j] = oh[j] * g.S - g.P;
      iw[j] = ow[j] * g.S - g.P;
      dyb[j] = pix[j] * yps;
      xb[j] = ((b * g.H + ih[j]) * g.W + iw[j]) * xps;
    }
  }
  DEV void issue(char* stage, int wid) {
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int piece = wid * PPW + j;
      const int h = (j >> 1) & 1;  // bit 3 of the pixel row 4 piece + q (wid * PPW is a multiple of 4)
      const bool pin = pix[j] < NP;
      blds16(rdy, (pin && cok[h]) ? (unsigned)(dyb[j] + co[h]) * 2u : kBufOob, stage + piece * 1024);
      const bool okb = pin && bok[h] && (unsigned)(ih[j] + bkh[h]) < (unsigned)H && (unsigned)(iw[j] + bkw[h]) < (unsigned)W;
      blds16(rx, okb ? (unsigned)(xb[j] + tap[h]) * 2u : kBufOob, stage + 16384 + piece * 1024);
      pix[j] += 64;
      dyb[j] += dyStep;
      ow[j] += 64;
      iw[j] += 64 * S;
      xb[j] += xStep;
      while (ow[j] >= OW) {
        ow[j] -= OW;
        iw[j] -= OW * S;
        xb[j] += xRow - xWrapOW;
        ih[j] += S;
        if (++oh[j] == OH) {
          oh[j] = 0;
          ih[j] -= OH * S;
          xb[j] += xImg;
        }
      }
    }
  }
};

template <int NS, int BUF>
__global__ void __launch_bounds__(256) conv_wgrad_v3(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                     float* __restrict__ dw, int kt_per_split, Geom g, int gm, int gn,
                                                     unsigned xbytes, unsigned dybytes) {
  constexpr int BM = 128, BN = 128, STAGE = 32768;
  constexpr int LDS = NS * STAGE > BM * (BN + 4) * 4 ? NS * STAGE : BM * (BN + 4) * 4;
  __shared__ __attribute__((aligned(1024))) char smem[LDS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  // (tile, split) from the linear dispatch id: consecutive logical ids share an XCD, so all tiles of
  // a split (which read the same pixel chunk) run on one XCD and share its L2
  const int lin = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int tile = lin % (gm * gn), split = lin / (gm * gn);
  const int tm = tile / gn, tn = tile % gn;
  const int m0 = tm * BM, n0 = tn * BN;
  const long NP = (long)g.N * g.OH * g.OW;
  const int nk_all = (int)((NP + 63) / 64);
  const int kt0 = split * kt_per_split;
  const int nk = min(nk_all, kt0 + kt_per_split) - kt0;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0 && BUF > 0) {
    // fragments of the whole step first, then the next stage's DMA while they land, then 32 MFMAs
    WgradLdsB ld(x, dy, g, m0, n0, kt0, wid, lane, xbytes, dybytes);
    ld.issue(smem, wid);
    if (NS == 3 && nk > 1) ld.issue(smem + STAGE, wid);
    for (int kt = 0; kt < nk; ++kt) {
      if (NS == 3 && kt + 1 < nk) vm_wait<8>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      const bf16* As = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE);
      const bf16* Bs = As + 64 * BM;
      bf16x8 a[2][4], b[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[h][i] = frag_k<BM>(As, wm * 64 + i * 16, h * 32, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = frag_k<BN>(Bs, wn * 64 + j * 16, h * 32, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (BUF == 1 && kt + NS - 1 < nk) ld.issue(smem + ((kt + NS - 1) % NS) * STAGE, wid);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][i], b[h][j], acc[i][j], 0, 0, 0);
    }
  } else if (nk > 0) {
    WgradLds<NS> ld(x, dy, g, m0, n0, kt0, wid, lane);
    ld.issue(smem, wid);
    if (NS == 3 && nk > 1) ld.issue(smem + STAGE, wid);
    for (int kt = 0; kt < nk; ++kt) {
      if (NS == 3 && kt + 1 < nk) vm_wait<8>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + NS - 1 < nk) ld.issue(smem + ((kt + NS - 1) % NS) * STAGE, wid);
      const bf16* As = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE);
      const bf16* Bs = As + 64 * BM;
#pragma unroll
      for (int ks = 0; ks < 64; ks += 32) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = frag_k<BM>(As, wm * 64 + i * 16, ks, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = frag_k<BN>(Bs, wn * 64 + j * 16, ks, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  float* ct = reinterpret_cast<float*>(smem);
  constexpr int RS = BN + 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(wm * 64 + i * 16 + 4 * (lane >> 4) + r) * RS + wn * 64 + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  const int Ntot = g.KH * g.KW * g.C;
  static_assert((256) % BN == 0, "epilogue column must be fixed per thread");
  const int c = threadIdx.x % BN, n = n0 + c;
  const long coff = wgrad_col(g, n);
  for (int e = threadIdx.x; e < BM * BN; e += 256) {
    const int row = e / BN, m = m0 + row;
    if (m < g.K && n < Ntot) wgrad_out(g, dw, split, (long)m * Ntot + coff, ct[row * RS + c]);
  }
}
// Narrow-layer weight-grad (out channels <= 64): block tile BM (out channels, 32 or 64) x BN
// ((kh, kw, ci) columns, 128 or 256), NW = BN / 64 waves side by side, each BM x 64.  Same k-major
// swizzled LDS images as conv_wgrad_v3 (kmaj_off<BM> / kmaj_off<BN>), filled by LDS-DMA: a 1-KiB
// piece covers 1024 / rowbytes pixel rows, lane l writes row (l / slots), physical slot (l % slots),
// i.e. the logical chunk (slot ^ key(row)) & (slots - 1).
template <int BM, int BN>
struct WgradLdsN {
  static constexpr int NW = BN / 64;
  static constexpr int RA = BM * 2, RB = BN * 2;
  static constexpr int SA = RA / 16, SB = RB / 16;
  static constexpr int PAW = 64 * RA / 1024 / NW, PBW = 64 * RB / 1024 / NW;
  static constexpr int RPA = 1024 / RA, RPB = 1024 / RB;
  static constexpr int A_BYTES = 64 * RA, STAGE = 64 * (RA + RB);
  static_assert(PAW >= 1 && PBW >= 1 && PAW * NW * 1024 == A_BYTES, "tile");
  const bf16* x; const bf16* dy; Geom g; long NP;
  long apix[PAW]; int aco[PAW];
  long bpix[PBW]; int bb[PBW], boh[PBW], bow[PBW], bkh[PBW], bkw[PBW], bci[PBW]; bool bok[PBW];
  DEV WgradLdsN(const bf16* x_, const bf16* dy_, const Geom& g_, int m0, int n0, int kt0, int wid, int lane)
      : x(x_), dy(dy_), g(g_) {
    NP = (long)g.N * g.OH * g.OW;
    const int Ntot = g.KH * g.KW * g.C;
#pragma unroll
    for (int j = 0; j < PAW; ++j) {
      const int r = (wid * PAW + j) * RPA + lane / SA;
      apix[j] = (long)kt0 * 64 + r;
      const int co = m0 + 8 * kmaj_chunk<BM>(r, lane % SA);
      aco[j] = co < g.K ? co : -1;
    }
#pragma unroll
    for (int j = 0; j < PBW; ++j) {
      const int r = (wid * PBW + j) * RPB + lane / SB;
      bpix[j] = (long)kt0 * 64 + r;
      const long pp = bpix[j] < NP ? bpix[j] : 0;
      bow[j] = (int)(pp % g.OW);
      const long t = pp / g.OW;
      boh[j] = (int)(t % g.OH);
      bb[j] = (int)(t / g.OH);
      const int n = n0 + 8 * kmaj_chunk<BN>(r, lane % SB);
      bok[j] = n < Ntot;
      bci[j] = n % g.C;
      const int u = n / g.C;
      bkw[j] = u % g.KW;
      bkh[j] = u / g.KW;
    }
  }
  DEV void issue(char* stage, int wid) {
    const bf16* zero = reinterpret_cast<const bf16*>(g_zero_page);
#pragma unroll
    for (int j = 0; j < PAW; ++j) {
      const bf16* sa = (apix[j] < NP && aco[j] >= 0) ? dy + apix[j] * g.yps + aco[j] : zero;
      glds16(sa, stage + (wid * PAW + j) * 1024);
      apix[j] += 64;
    }
#pragma unroll
    for (int j = 0; j < PBW; ++j) {
      const int ih = boh[j] * g.S - g.P + bkh[j], iw = bow[j] * g.S - g.P + bkw[j];
      const bool ok = bpix[j] < NP && bok[j] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
      const bf16* sb = ok ? x + (((long)bb[j] * g.H + ih) * g.W + iw) * g.xps + bci[j] : zero;
      glds16(sb, stage + A_BYTES + (wid * PBW + j) * 1024);
      bpix[j] += 64;
      bow[j] += 64;
      while (bow[j] >= g.OW) {
        bow[j] -= g.OW;
        if (++boh[j] == g.OH) { boh[j] = 0; ++bb[j]; }
      }
    }
  }
};

// Buffer-descriptor form of WgradLdsN (same LDS images): 32-bit element offsets advanced by adds
// (see WgradLdsB).  A piece j: pixel row r, dy column co; B piece j: pixel row r, column n -> tap.
template <int BM, int BN, int NWV = BN / 64>
struct WgradLdsNB {
  using L = WgradLdsN<BM, BN>;  // LDS image layout (row bytes, slots, rows per piece); NWV waves share the pieces
  static constexpr int PAW = 64 * L::RA / 1024 / NWV, PBW = 64 * L::RB / 1024 / NWV, A_BYTES = L::A_BYTES;
  static_assert(PAW >= 1 && PBW >= 1 && PAW * NWV * 1024 == A_BYTES, "pieces");
  __amdgpu_buffer_rsrc_t rx, rdy;
  int NP, OW, OH, H, W, S, dyStep, xStep, xWrapOW, xRow, xImg;
  int apix[PAW], adyb[PAW];
  int bpix[PBW], boh[PBW], bow[PBW], bih[PBW], biw[PBW], bxb[PBW], bkh[PBW], bkw[PBW], btap[PBW];
  DEV WgradLdsNB(const bf16* x, const bf16* dy, const Geom& g, int m0, int n0, int kt0, int wid, int lane,
                 unsigned xbytes, unsigned dybytes)
      : OW(g.OW), OH(g.OH), H(g.H), W(g.W), S(g.S) {
    rx = make_rsrc(x, xbytes);
    rdy = make_rsrc(dy, dybytes);
    NP = g.N * g.OH * g.OW;
    const int Ntot = g.KH * g.KW * g.C, xps = (int)g.xps, yps = (int)g.yps;
    dyStep = 64 * yps;
    xStep = 64 * g.S * xps;
    xWrapOW = g.OW * g.S * xps;
    xRow = g.S * g.W * xps;
    xImg = (g.H - g.OH * g.S) * g.W * xps;
#pragma unroll
    for (int j = 0; j < PAW; ++j) {
      const int r = (wid * PAW + j) * L::RPA + lane / L::SA;
      apix[j] = kt0 * 64 + r;
      const int co = m0 + 8 * kmaj_chunk<BM>(r, lane % L::SA);
      // an out-of-range column never becomes valid: fold it into the pixel bound
      adyb[j] = apix[j] * yps + co;
      if (co >= g.K) apix[j] = 0x40000000;
    }
#pragma unroll
    for (int j = 0; j < PBW; ++j) {
      const int r = (wid * PBW + j) * L::RPB + lane / L::SB;
      bpix[j] = kt0 * 64 + r;
      const int pp = bpix[j] < NP ? bpix[j] : 0;
      bow[j] = pp % g.OW;
      const int t = pp / g.OW;
      boh[j] = t % g.OH;
      const int b = t / g.OH;
      bih[j] = boh[j] * g.S - g.P;
      biw[j] = bow[j] * g.S - g.P;
      bxb[j] = ((b * g.H + bih[j]) * g.W + biw[j]) * xps;
      const int n = n0 + 8 * kmaj_chunk<BN>(r, lane % L::SB);
      const int nn = n < Ntot ? n : 0;
      const int ci = nn % g.C, u = nn / g.C;
      bkw[j] = u % g.KW;
      bkh[j] = u / g.KW;
      btap[j] = (bkh[j] * g.W + bkw[j]) * xps + ci;
      if (n >= Ntot) bkh[j] = 0x40000000;  // never in-image
    }
  }
  DEV void issue(char* stage, int wid) {
#pragma unroll
    for (int j = 0; j < PAW; ++j) {
      blds16(rdy, apix[j] < NP ? (unsigned)adyb[j] * 2u : kBufOob, stage + (wid * PAW + j) * 1024);
      apix[j] += 64;
      adyb[j] += dyStep;
    }
#pragma unroll
    for (int j = 0; j < PBW; ++j) {
      const bool ok = bpix[j] < NP && (unsigned)(bih[j] + bkh[j]) < (unsigned)H && (unsigned)(biw[j] + bkw[j]) < (unsigned)W;
      blds16(rx, ok ? (unsigned)(bxb[j] + btap[j]) * 2u : kBufOob, stage + A_BYTES + (wid * PBW + j) * 1024);
      bpix[j] += 64;
      bow[j] += 64;
      biw[j] += 64 * S;
      bxb[j] += xStep;
      while (bow[j] >= OW) {
        bow[j] -= OW;
        biw[j] -= OW * S;
        bxb[j] += xRow - xWrapOW;
        bih[j] += S;
        if (++boh[j] == OH) {
          boh[j] = 0;
          bih[j] -= OH * S;
          bxb[j] += xImg;
        }
      }
    }
  }
};

template <int BM, int BN, int NS, bool BUF>
__global__ void __launch_bounds__(BN) conv_wgrad_v3n(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                    float* __restrict__ dw, int kt_per_split, Geom g, int gm, int gn,
                                                    unsigned xbytes, unsigned dybytes) {
  using LD = WgradLdsN<BM, BN>;
  constexpr int STAGE = LD::STAGE, TM = BM / 16, PER = LD::PAW + LD::PBW;
  constexpr int LDSB = NS * STAGE > BM * (BN + 4) * 4 ? NS * STAGE : BM * (BN + 4) * 4;
  __shared__ __attribute__((aligned(1024))) char smem[LDSB];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // (tile, split) from the linear dispatch id: consecutive logical ids share an XCD, so all tiles of
  // a split (which read the same pixel chunk) run on one XCD and share its L2
  const int lin = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int tile = lin % (gm * gn), split = lin / (gm * gn);
  const int tm = tile / gn, tn = tile % gn;
  const int m0 = tm * BM, n0 = tn * BN;
  const long NP = (long)g.N * g.OH * g.OW;
  const int nk_all = (int)((NP + 63) / 64);
  const int kt0 = split * kt_per_split;
  const int nk = min(nk_all, kt0 + kt_per_split) - kt0;
  f32x4 acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0 && BUF) {
    WgradLdsNB<BM, BN> ld(x, dy, g, m0, n0, kt0, wid, lane, xbytes, dybytes);
    ld.issue(smem, wid);
    if (NS == 3 && nk > 1) ld.issue(smem + STAGE, wid);
    for (int kt = 0; kt < nk; ++kt) {
      if (NS == 3 && kt + 1 < nk) vm_wait<PER>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      const bf16* As = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE);
      const bf16* Bs = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE + LD::A_BYTES);
      bf16x8 a[2][TM], b[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a[h][i] = frag_k<BM>(As, i * 16, h * 32, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = frag_k<BN>(Bs, wid * 64 + j * 16, h * 32, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kt + NS - 1 < nk) ld.issue(smem + ((kt + NS - 1) % NS) * STAGE, wid);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][i], b[h][j], acc[i][j], 0, 0, 0);
    }
  } else if (nk > 0) {
    LD ld(x, dy, g, m0, n0, kt0, wid, lane);
    ld.issue(smem, wid);
    if (NS == 3 && nk > 1) ld.issue(smem + STAGE, wid);
    for (int kt = 0; kt < nk; ++kt) {
      if (NS == 3 && kt + 1 < nk) vm_wait<PER>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + NS - 1 < nk) ld.issue(smem + ((kt + NS - 1) % NS) * STAGE, wid);
      const bf16* As = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE);
      const bf16* Bs = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE + LD::A_BYTES);
#pragma unroll
      for (int ks = 0; ks < 64; ks += 32) {
        bf16x8 a[TM], b[4];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = frag_k<BM>(As, i * 16, ks, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = frag_k<BN>(Bs, wid * 64 + j * 16, ks, lane);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  float* ct = reinterpret_cast<float*>(smem);
  constexpr int RS = BN + 4;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(i * 16 + 4 * (lane >> 4) + r) * RS + wid * 64 + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  const int Ntot = g.KH * g.KW * g.C;
  static_assert((BN) % BN == 0, "epilogue column must be fixed per thread");
  const int c = threadIdx.x % BN, n = n0 + c;
  const long coff = wgrad_col(g, n);
  for (int e = threadIdx.x; e < BM * BN; e += BN) {
    const int row = e / BN, m = m0 + row;
    if (m < g.K && n < Ntot) wgrad_out(g, dw, split, (long)m * Ntot + coff, ct[row * RS + c]);
  }
}
// Weight-grad v4: 8 waves (BM / 64 x BN / 64, each 64 x 64), BM x BN = 128 x 256 or 256 x 128, a
// 3-stage LDS-DMA ring (48 KiB stages, one block per CU, 2 waves per SIMD) with a counted
// vmcnt(pieces per wave) so one stage stays in flight across each barrier -- the forward kernel's
// structure; the narrow-tile buffer loader with the pieces shared by all 8 waves.
template <int BM, int BN>
__global__ void __launch_bounds__(512) conv_wgrad_v4(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                     float* __restrict__ dw, int kt_per_split, Geom g, int gm, int gn,
                                                     unsigned xbytes, unsigned dybytes) {
  constexpr int WM = BM / 64, NS = 3;
  static_assert(WM * (BN / 64) == 8, "8 waves");
  using LD = WgradLdsNB<BM, BN, 8>;
  constexpr int STAGE = WgradLdsN<BM, BN>::STAGE, PER = LD::PAW + LD::PBW;
  constexpr int CT = BM * (BN + 4) * 4;
  constexpr int LDSB = NS * STAGE > CT ? NS * STAGE : CT;
  __shared__ __attribute__((aligned(1024))) char smem[LDSB];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid % WM, wn = wid / WM;
  const int lin = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int tile = lin % (gm * gn), split = lin / (gm * gn);
  const int tm = tile / gn, tn = tile % gn;
  const int m0 = tm * BM, n0 = tn * BN;
  const long NP = (long)g.N * g.OH * g.OW;
  const int nk_all = (int)((NP + 63) / 64);
  const int kt0 = split * kt_per_split;
  const int nk = min(nk_all, kt0 + kt_per_split) - kt0;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0) {
    LD ld(x, dy, g, m0, n0, kt0, wid, lane, xbytes, dybytes);
    ld.issue(smem, wid);
    if (nk > 1) ld.issue(smem + STAGE, wid);
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) vm_wait<PER>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      const bf16* As = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE);
      const bf16* Bs = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE + LD::A_BYTES);
      bf16x8 a[2][4], b[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[h][i] = frag_k<BM>(As, wm * 64 + i * 16, h * 32, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = frag_k<BN>(Bs, wn * 64 + j * 16, h * 32, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kt + NS - 1 < nk) ld.issue(smem + ((kt + NS - 1) % NS) * STAGE, wid);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][i], b[h][j], acc[i][j], 0, 0, 0);
    }
  }
  vm_wait<0>();
  __syncthreads();
  float* ct = reinterpret_cast<float*>(smem);
  constexpr int RS = BN + 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(wm * 64 + i * 16 + 4 * (lane >> 4) + r) * RS + wn * 64 + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  const int Ntot = g.KH * g.KW * g.C;
  static_assert((512) % BN == 0, "epilogue column must be fixed per thread");
  const int c = threadIdx.x % BN, n = n0 + c;
  const long coff = wgrad_col(g, n);
  for (int e = threadIdx.x; e < BM * BN; e += 512) {
    const int row = e / BN, m = m0 + row;
    if (m < g.K && n < Ntot) wgrad_out(g, dw, split, (long)m * Ntot + coff, ct[row * RS + c]);
  }
}

// ---------------------------------------------------------------- tap-fused 3x3 stride-1 weight-grad
// C[m = out channel][n = (tap, ci)] = sum over output pixels p of dy[p][m] * x[p + tap shift][ci], for a block tile
// of 128 out channels x (all 9 taps x 32 input channels) = 288 columns.  The reduction walks 8 x 8 output-pixel
// patches (64 pixels per K step): the x operand is the patch's 10 x 10 halo (32 channels) loaded ONCE and read by
// all 9 taps through shifted LDS addresses, so x is fetched ~1.6x per (out-channel tile) and dy once per 32-channel
// group -- vs 9x / 18x for the (tap, channel)-column tiles of conv_wgrad_v3/v4.
//   A (dy): [64 pixel rows][BM ch] k-major, the kmaj_off<BM> swizzle, frag_k<BM> (as conv_wgrad_v3 / v3n);
//   BM = 128, or 64 for layers with <= 64 output channels.
//   B (x halo): 10 rows of pitch 12 pixels x 32 ch (64-B rows), chunk ^ 2 (halo row y & 1): the 8 rows one
//   ds_read_b64_tr_b16 group touches ((y, x .. x + 3), (y + 1, x .. x + 3)) then hit 64 distinct banks.
//   Stages: BM/8 KiB A + 8 KiB B (120 of 128 halo rows used), 3-stage LDS-DMA ring, a counted vmcnt keeps one
//   stage in flight across each barrier.  4 waves = 2 (m) x 2 (n), wave tile BM/2 x 144 (BM/32 x 9 MFMA frags).
// Valid for KH = KW = 3, S = 1, P = 1, OH = H, OW = W, C % 16 == 0 (host-checked; a
// 16-channel plane half loads zeros).  Split-K over patches; the
// (tile, split) -> linear id mapping keeps a split's tiles on one XCD (they read the same patches).
template <int BM, int NP = 1>  // NP halo planes of 32 input channels each (2: a block owns 64 input channels)
struct WgradTapLds {
  static constexpr int BC = 32, PH = 8, PW = 8, HP = 12;  // halo pitch 12 (10 used)
  static constexpr int A_BYTES = 64 * BM * 2, B_BYTES = NP * 8 * 1024, STAGE = A_BYTES + B_BYTES;
  static constexpr int APW = A_BYTES / 1024 / 4;           // dy pieces per wave (4 waves)
  static constexpr int SLOTS = BM / 8, RPP = 64 / SLOTS;   // 16-B slots per pixel row, pixel rows per piece
  __amdgpu_buffer_rsrc_t rx, rdy;
  int OH, OW, H, W, npw, nph;
  int pb, py, px;                    // patch cursor (uniform)
  int arel[APW], ar[APW], ac[APW];   // dy: per piece pixel (r, c) in the patch and element offset rel. to the patch
  int acol[APW];                     // dy column (element) this lane loads for the piece
  bool aok[APW];
  int brel[2], by[2], bx[2];         // x halo: per piece halo (y, x) and element offset rel. to the halo origin
  int bcol[2];
  bool bok[2];
  int yps, xps, cmax;
  DEV WgradTapLds(const bf16* x, const bf16* dy, const Geom& g, int m0, int c0, int kt0, int wid, int lane,
                  unsigned xbytes, unsigned dybytes)
      : OH(g.OH), OW(g.OW), H(g.H), W(g.W) {
    cmax = g.C;  // C % 32 == 16 (the 16-channel space-to-depth stem): the plane's chunks past C load zeros
    rx = make_rsrc(x, xbytes);
    rdy = make_rsrc(dy, dybytes);
    yps = (int)g.yps;
    xps = (int)g.xps;
    npw = (g.OW + PW - 1) / PW;
    nph = (g.OH + PH - 1) / PH;
    px = kt0 % npw;
    const int t = kt0 / npw;
    py = t % nph;
    pb = t / nph;
#pragma unroll
    for (int j = 0; j < APW; ++j) {  // piece wid * APW + j: pixel rows RPP * piece + lane / SLOTS
      const int row = (wid * APW + j) * RPP + lane / SLOTS;
      const int slot = lane % SLOTS;
      // physical slot -> logical chunk under the kmaj_off<BM> key of this pixel row
      const int key = (2 * BM >= 256) ? 2 * ((row & 3) | (((row >> 3) & 1) << 2))
                                      : 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
      const int chunk = (slot ^ key) & (SLOTS - 1);
      acol[j] = m0 + chunk * 8;
      aok[j] = acol[j] < g.K;
      ar[j] = row >> 3;
      ac[j] = row & 7;
      arel[j] = (ar[j] * g.OW + ac[j]) * yps;
    }
    // halo: 8 pieces x 16 rows of 64 B; this wave fills pieces wid * 2 + j; lane: row (lane >> 2), slot lane & 3
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = (wid * 2 + j) * 16 + (lane >> 2);
      by[j] = row / HP;
      bx[j] = row % HP;
      const int chunk = (lane & 3) ^ (2 * (by[j] & 1));
      bok[j] = row < 10 * HP && bx[j] < 10;
      brel[j] = (by[j] * g.W + bx[j]) * xps;
      bcol[j] = c0 + chunk * 8;
    }
  }
  DEV void issue(char* stage, int wid) {
    const int oy0 = py * PH, ox0 = px * PW;
    const int abase = ((pb * OH + oy0) * OW + ox0) * yps;
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      const bool ok = aok[j] && oy0 + ar[j] < OH && ox0 + ac[j] < OW;
      blds16(rdy, ok ? (unsigned)(abase + arel[j] + acol[j]) * 2u : kBufOob, stage + (wid * APW + j) * 1024);
    }
    const int xbase = ((pb * H + oy0 - 1) * W + ox0 - 1) * xps;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool ok = bok[j] && (unsigned)(oy0 - 1 + by[j]) < (unsigned)H && (unsigned)(ox0 - 1 + bx[j]) < (unsigned)W;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        blds16(rx, ok && bcol[j] + 32 * pl < cmax ? (unsigned)(xbase + brel[j] + bcol[j] + 32 * pl) * 2u : kBufOob,
               stage + A_BYTES + pl * 8192 + (wid * 2 + j) * 1024);
    }
    if (++px == npw) {
      px = 0;
      if (++py == nph) { py = 0; ++pb; }
    }
  }
};

// B fragment of tap (kh, kw), 16 channels from ch0, pixels k0 .. k0 + 31 of the patch (frag_k's lane mapping with
// pixel k -> halo row ((k >> 3) + kh, (k & 7) + kw))
DEV bf16x8 frag_halo(const bf16* Bs, int kh, int kw, int ch0, int k0, int lane) {
  typedef short s4 __attribute__((ext_vector_type(4)));
  const int g = lane >> 4, il = lane & 15, q = il >> 2, p = il & 3;
  const int ch = ch0 + 4 * p;
  const int y = (k0 >> 3) + g + kh;
  const int chunk = (ch >> 3) ^ (2 * (y & 1));
  const int off = (y * WgradTapLds<128>::HP + q + kw) * 32 + ((chunk & 3) << 3) + (ch & 7);
  s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(Bs + off));
  s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(Bs + off + 4 * 32));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// NP = 2 (layers with <= 64 output channels, BM = 64): a block owns 64 input channels (two halo planes) and its 4
// waves are 1 (m) x 4 (n), wave tile BM x 144 (4 A + 9 B fragments per 36 MFMAs instead of 2 + 9 per 18): the
// halo fragment reads, which bound the 64-channel layers on the LDS port, are amortised over twice the rows
template <int BM, int NP = 1>
__global__ void __launch_bounds__(256, 2) conv_wgrad_tap(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                         float* __restrict__ dw, int kt_per_split, Geom g, int gm,
                                                         int gn, int nk_all, unsigned xbytes, unsigned dybytes) {
  using LD = WgradTapLds<BM, NP>;
  constexpr int NS = 3, STAGE = LD::STAGE;
  constexpr int TM = NP == 2 ? BM / 16 : BM / 32;           // NP 1: 2 (m) x 2 (n) waves; NP 2: 1 x 4
  constexpr int NCOL = 288 * NP;                            // tile columns: NP planes x 9 taps x 32 channels
  constexpr int NPASS = (BM == 128 && NP == 2) ? 4 : 2;    // epilogue: the tile staged in NPASS row slices
  constexpr int CTR = BM / NPASS, CTS = NCOL + 4;
  constexpr int LDSB = NS * STAGE > CTR * CTS * 4 ? NS * STAGE : CTR * CTS * 4;
  __shared__ __attribute__((aligned(1024))) char smem[LDSB];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = NP == 2 ? 0 : wid >> 1, wn = NP == 2 ? (wid & 1) : wid & 1, wpl = NP == 2 ? wid >> 1 : 0;
  const int lin = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int tile = lin % (gm * gn), split = lin / (gm * gn);
  const int tm = tile % gm, tc = tile / gm;  // out-channel tiles of one channel group adjacent (share the x halo)
  const int m0 = tm * BM, c0 = tc * LD::BC * NP;
  const int kt0 = split * kt_per_split;
  const int nk = min(nk_all, kt0 + kt_per_split) - kt0;
  f32x4 acc[TM][9];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0) {
    LD ld(x, dy, g, m0, c0, kt0, wid, lane, xbytes, dybytes);
    ld.issue(smem, wid);
    if (nk > 1) ld.issue(smem + STAGE, wid);
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) vm_wait<LD::APW + 2 * NP>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + NS - 1 < nk) ld.issue(smem + ((kt + NS - 1) % NS) * STAGE, wid);
      const bf16* As = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE);
      const bf16* Bs = reinterpret_cast<const bf16*>(smem + (kt % NS) * STAGE + LD::A_BYTES + wpl * 8192);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bf16x8 a[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = frag_k<BM>(As, wm * (BM / 2) + i * 16, h * 32, lane);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const int f = wn * 9 + j, tap = f >> 1;
          const bf16x8 b = frag_halo(Bs, tap / 3, tap % 3, (f & 1) * 16, h * 32, lane);
#pragma unroll
          for (int i = 0; i < TM; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b, acc[i][j], 0, 0, 0);
        }
      }
    }
  }
  vm_wait<0>();
  const int Ntot = 9 * g.C;
  float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int half = 0; half < NPASS; ++half) {
    __syncthreads();
    if (NP == 2 || wm == half) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = NP == 2 ? i * 16 - half * CTR : i * 16;  // row of the staged half
        if (NP == 2 && (row < 0 || row >= CTR)) continue;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ct[(row + 4 * (lane >> 4) + r) * CTS + wpl * 288 + (wn * 9 + j) * 16 + (lane & 15)] = acc[i][j][r];
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CTR * NCOL; e += 256) {
      const int row = e / NCOL, col = e % NCOL, m = m0 + half * CTR + row;
      const int pl = col / 288, cc = col % 288;
      const int ci = c0 + pl * 32 + (cc & 31), n = (cc >> 5) * g.C + ci;  // cc = tap * 32 + ci
      if (m < g.K && ci < g.C) wgrad_out(g, dw, split, (long)m * Ntot + wgrad_col(g, n), ct[row * CTS + col]);
    }
  }
}
}  // namespace v3

// dw[i] += sum over splits s = 0, 1, ... of ws[s][i], in that order (the deterministic split-K reduction)
__global__ void wgrad_split_reduce(const float* __restrict__ ws, float* __restrict__ dw, long slab, int splits) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < slab; i += (long)gridDim.x * blockDim.x) {
    float acc = ws[i];
    for (int k = 1; k < splits; ++k) acc += ws[(long)k * slab + i];
    dw[i] += acc;
  }
}

// Split-K of a weight-grad over its nk K steps (pixels) for a grid of `tiles` output tiles: {splits, per} with per K
// steps a split.  At least 8 steps per split; the sweep takes the first minimum of the cost model
//   rounds(tiles * s / R) * (K steps per split) * t_step + tiles * s * t_atomic   [us]
// with R resident blocks on the chip, t_step per K step of a block and t_atomic for a block's fp32 atomics.  Each
// caller keeps the source of its three constants.
inline WPlan wgrad_split(Kern k, int tiles, int nk, double R, double t_step, double t_atomic) {
  int maxs = nk / 8;
  if (maxs < 1) maxs = 1;
  int splits = 1;
  double best = 1e300;
  for (int sp = 1; sp <= maxs; sp += (sp < 16 ? 1 : sp / 16)) {
    const double blocks = (double)tiles * sp;
    const double t = ceil(blocks / R) * ceil_div(nk, sp) * t_step + blocks * t_atomic;
    if (t < best) { best = t; splits = sp; }
  }
  const int per = ceil_div(nk, splits);
  return WPlan{k, ceil_div(nk, per), per};
}
// the v2 (register-staged) weight-grad's rule: aim for ~2048 blocks, >= 8 K-tiles per split
inline WPlan wgrad_split_v2(Kern k, int tiles, int nk) {
  int splits = 2048 / tiles;
  if (splits < 1) splits = 1;
  int maxs = nk / 8;
  if (maxs < 1) maxs = 1;
  if (splits > maxs) splits = maxs;
  const int per = ceil_div(nk, splits);
  return WPlan{k, ceil_div(nk, per), per};
}

template <typename T, int BM, int BN>
int launch_wgrad(const void* x, const void* dy, float* dw, const Geom& g, hipStream_t st, const WPlan& pl) {
  constexpr int VW = Traits<T>::VW;
  const int gm = ceil_div(g.K, BM), gn = ceil_div(g.KH * g.KW * g.C, BN);
  return by_flags(vec_ok(VW, g.K, {g.yps}, {}, {dy}), vec_ok(VW, g.C, {g.xps}, {}, {x}), [&](auto VA, auto VB) {
    return launch(conv_wgrad_kernel<T, BM, BN, VA.value, VB.value>, dim3((unsigned)gm * gn, pl.splits), NT, 0, st, x,
                  dy, dw, pl.per, g, gm, gn);
  });
}

// ---------------------------------------------------------------- weight-grad
// tap-fused 3x3 s1 weight-grad (v3::conv_wgrad_tap) where it applies
inline bool wgrad_tap_ok(const Geom& g, const void* x, const void* dy) {
  if (g.KH != 3 || g.KW != 3 || g.S != 1 || g.P != 1 || g.OH != g.H || g.OW != g.W) return false;
  if (g.C % 16 != 0 || !vec_ok(8, g.C, {g.xps, g.K, g.yps}, {}, {x, dy})) return false;
  // C % 32 == 16 (the space-to-depth stem, 16 channels) included: the upper half of the halo plane loads zeros
  // (yolov5s 3845 -> 3876 img/s against the v3n column tiles, profiles/r05/wgrad_tap16_ab.log)
  if (!fits_buf(x_bytes(g)) || !fits_buf(y_bytes(g))) return false;
  // enough (patch, tile) work units that the per-block fp32 atomics of the 288-column tile stay a small share
  // (tools/gpu/tune_conv.py: 20^2 / 40^2 / 80^2 yolov5s layers are faster on the v3 / v4 column tiles)
  const long units = (long)g.N * ceil_div(g.OH, 8) * ceil_div(g.OW, 8) * ceil_div(g.K, 128) * ceil_div(g.C, 32);
  // 10000: the yolov5s 64-channel @80^2 layers (12800 units) measured 96 -> 79 us on the tap kernel, the 256-channel
  // @20^2 ones (9216) 70 -> 106 us (profiles/r02/ab_wgrad_v5s.log); lower thresholds were slower on yolov5s
  // (profiles/r05/wgrad_tap_units_ab.log)
  return units >= 10000;
}
// weight-grad of layers with <= 64 output channels: 1 = the narrow LDS-DMA tiles (BM 32/64) past 8 M pixels at
// K = 64, 2 = the 128 x 128 LDS-DMA tile (half its rows idle at K = 64) otherwise (tools/gpu/ab_conv.sh: 64 ch @768^2
// x 32 narrow 483 / 128-tile 394 / v2 257 TFLOP/s; @384^2 280 / 384 / 261; yolov5s layers 128-tile best)
inline int wgrad_narrow_for(const Geom& g, long NP) { return (g.K == 64 && NP >= 8L * 1024 * 1024) ? 1 : 2; }

// The weight-grad's plan: the kernel and its split-K (T = the storage type; the LDS-DMA kernels are bf16 only).
// conv_wgrad_t executes it and dmy_conv_wgrad_ws_elems reads the split count off it.
template <typename T>
WPlan plan_wgrad(const Geom& g, const void* x, const void* dy) {
  const long NP = (long)g.N * g.OH * g.OW;
  const int Ntot = g.KH * g.KW * g.C;
  if constexpr (sizeof(T) == 2) {
    const bool vec = vec_ok(8, g.C, {g.xps, g.K, g.yps}, {}, {x, dy});
    const int nm = wgrad_narrow_for(g, NP);
    const int nk = ceil_div(NP, 64);  // K steps of the column-tile kernels: 64 pixels
    const double NC = num_cus();
    if (wgrad_tap_ok(g, x, dy)) {
      // 128 output rows a tile above 64 output channels.  The <= 64-output-channel layers with C % 64 == 0 run the
      // two-plane tile (a block owns 64 input channels: 13 fragment reads per 36 MFMAs instead of 11 per 18; DMA-1536
      // 158.4 -> 159.1 img/s, profiles/r05/wgrad_tap_np2_ab.log); the same for the 128-row tile needs 288 accumulators,
      // one block per CU, and measured 2 % slower (profiles/r05/wgrad_tap_np128_ab.log)
      const Kern k = g.K > 64 ? Kern::W_TAP128 : g.C % 64 == 0 ? Kern::W_TAP64X2 : Kern::W_TAP64;
      const int BM = g.K > 64 ? 128 : 64, planes = k == Kern::W_TAP64X2 ? 2 : 1;
      const int np = g.N * ceil_div(g.OH, 8) * ceil_div(g.OW, 8);  // K steps: 8 x 8 patches
      // two resident blocks per CU; ~1.1 us per patch step of the 128-row tile (288 MFMA per wave pair at ~45 % of
      // peak) and its 147 KiB fp32 tile of atomics per block at 1.3 TB/s (MI355X_MICROARCH.md §Global float atomics);
      // the 64-row tile halves both
      const double f = BM / 128.0 * planes;
      return wgrad_split(k, ceil_div(g.K, BM) * ceil_div(g.C, 32 * planes), np, 2.0 * NC, 1.1 * f, 0.113 * f);
    }
    // wgrad v4 tile 256 x 128 for K_out >= 256, else the v3 128 x 128 kernel (tools/gpu/ab_conv.sh,
    // profiles/r01/ab_wgrad_v4.log: +7-11 % at K_out >= 256, the 256-row tile is half idle and a 128 x 256 one no
    // faster at K_out = 128).  The v3 model below with one resident block per CU, twice the tile per K step and atomics
    if (vec && g.K >= 256 && Ntot >= 128 && NP >= 16384 && fits_buf(x_bytes(g)) && fits_buf(y_bytes(g)))
      return wgrad_split(Kern::W_V4, ceil_div(g.K, 256) * ceil_div(Ntot, 128), nk, NC, 1.9 * 2 * 0.5, 0.0504 * 2);
    // v3 128 x 128 tile.  Cost model (calibrated on MI355X): resident blocks R = 2 per CU; 1.9 us a K step; 64 KiB of
    // fp32 atomics a block at 1.3 TB/s.  It beat fixed 512 / 768-block targets on DMA-1536 (152.15 vs 150.76 / 147.91
    // img/s, profiles/r04/wgrad_target_ab.log)
    if (vec && (g.K > 64 || nm == 2) && Ntot >= 64 && NP >= 16384)
      return wgrad_split(Kern::W_V3, ceil_div(g.K, 128) * ceil_div(Ntot, 128), nk, 2.0 * NC, 1.9, 0.0504);
    if (vec && g.K <= 64 && Ntot >= 128 && NP >= 16384 && nm == 1) {
      // narrow layers: BM = 32 / 64 out-channel tiles, BN = 128 / 256 column tiles.  One 256-column tile also for
      // 128 < Ntot < 256 (the 144-column space-to-depth stem view: on 128-column tiles the second tile re-read every
      // dy row for 16 columns of work; profiles/r04/stem_wgrad_ab.log 1638 -> 1276 us)
      const bool wide = Ntot >= 512 || Ntot % 256 == 0 || (Ntot > 128 && Ntot < 256);
      const int BM = g.K <= 32 ? 32 : 64, BN = wide ? 256 : 128;
      // the v3 model with the tile's share of a 128 x 128 step and atomics
      const double R = 2.0 * NC * (128.0 * 128.0) / (BM * BN) * 0.5;
      const double step = 1.9 * (BM * BN) / (128.0 * 128.0) + 0.25;
      return wgrad_split(wide ? Kern::W_V3N256 : Kern::W_V3N128, ceil_div(g.K, BM) * ceil_div(Ntot, BN), nk, R, step,
                         0.0504 * (BM * BN) / (128.0 * 128.0));
    }
  }
  const int nk = ceil_div(NP, Cfg<T>::BK);
  if (g.K > 64 && Ntot > 64) return wgrad_split_v2(Kern::W_V2_128, ceil_div(g.K, 128) * ceil_div(Ntot, 128), nk);
  return wgrad_split_v2(Kern::W_V2_64, ceil_div(g.K, 64) * ceil_div(Ntot, 64), nk);
}

// The LDS-DMA weight-grads read x and dy through buffer descriptors of xb / db bytes; v3 and v3n keep a plain-pointer
// form (BUF off, extents 0) for tensors past the descriptor range
inline int launch_wgrad_v3(const void* x, const void* dy, float* dw, const Geom& g, hipStream_t st, const WPlan& pl) {
  const int gm = ceil_div(g.K, 128), gn = ceil_div(g.KH * g.KW * g.C, 128);
  const bool buf = fits_buf(x_bytes(g)) && fits_buf(y_bytes(g));
  return by_flags(buf, [&](auto BUF) {
    return launch(v3::conv_wgrad_v3<2, BUF.value>, dim3((unsigned)gm * gn, pl.splits), 256, 0, st, x, dy, dw, pl.per, g,
                  gm, gn, buf ? (unsigned)x_bytes(g) : 0u, buf ? (unsigned)y_bytes(g) : 0u);
  });
}

inline int launch_wgrad_v4(const void* x, const void* dy, float* dw, const Geom& g, hipStream_t st, const WPlan& pl) {
  const int gm = ceil_div(g.K, 256), gn = ceil_div(g.KH * g.KW * g.C, 128);
  return launch(v3::conv_wgrad_v4<256, 128>, dim3((unsigned)gm * gn, pl.splits), 512, 0, st, x, dy, dw, pl.per, g, gm,
                gn, (unsigned)x_bytes(g), (unsigned)y_bytes(g));
}

template <int BM, int NP = 1>
int launch_wgrad_tap(const void* x, const void* dy, float* dw, const Geom& g, hipStream_t st, const WPlan& pl) {
  const int gm = ceil_div(g.K, BM), gn = ceil_div(g.C, 32 * NP);
  const int nk = g.N * ceil_div(g.OH, 8) * ceil_div(g.OW, 8);  // 8 x 8 patches
  return launch(v3::conv_wgrad_tap<BM, NP>, dim3((unsigned)gm * gn, pl.splits), 256, 0, st, x, dy, dw, pl.per, g, gm,
                gn, nk, (unsigned)x_bytes(g), (unsigned)y_bytes(g));
}

template <int BM, int BN>
int launch_wgrad_v3n(const void* x, const void* dy, float* dw, const Geom& g, hipStream_t st, const WPlan& pl) {
  const int gm = ceil_div(g.K, BM), gn = ceil_div(g.KH * g.KW * g.C, BN);
  constexpr int NS = 3 * v3::WgradLdsN<BM, BN>::STAGE <= 80 * 1024 ? 3 : 2;  // keep 2 blocks per CU
  const bool buf = fits_buf(x_bytes(g)) && fits_buf(y_bytes(g));
  return by_flags(buf, [&](auto BUF) {
    return launch(v3::conv_wgrad_v3n<BM, BN, NS, BUF.value>, dim3((unsigned)gm * gn, pl.splits), BN, 0, st, x, dy, dw,
                  pl.per, g, gm, gn, buf ? (unsigned)x_bytes(g) : 0u, buf ? (unsigned)y_bytes(g) : 0u);
  });
}

template <typename T>
int conv_wgrad_t(const void* x, const void* dy, float* dw, Geom g, hipStream_t st) {
  const WPlan pl = plan_wgrad<T>(g, x, dy);
  // deterministic mode with one split keeps the single atomic per element (exact: it adds to a zero or to an earlier
  // stream-ordered launch's value), so the workspace is dropped
  if (pl.splits <= 1) g.dws = nullptr;
  if (!g.zeroed) (void)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)g.K * g.KH * g.KW * g.C, st);
  const bool k32 = g.K <= 32;
  int rc;
  switch (sizeof(T) == 2 ? pl.k : Kern::V2) {
    case Kern::W_TAP128: rc = launch_wgrad_tap<128>(x, dy, dw, g, st, pl); break;
    case Kern::W_TAP64X2: rc = launch_wgrad_tap<64, 2>(x, dy, dw, g, st, pl); break;
    case Kern::W_TAP64: rc = launch_wgrad_tap<64>(x, dy, dw, g, st, pl); break;
    case Kern::W_V4: rc = launch_wgrad_v4(x, dy, dw, g, st, pl); break;
    case Kern::W_V3: rc = launch_wgrad_v3(x, dy, dw, g, st, pl); break;
    case Kern::W_V3N256:
      rc = k32 ? launch_wgrad_v3n<32, 256>(x, dy, dw, g, st, pl) : launch_wgrad_v3n<64, 256>(x, dy, dw, g, st, pl);
      break;
    case Kern::W_V3N128:
      rc = k32 ? launch_wgrad_v3n<32, 128>(x, dy, dw, g, st, pl) : launch_wgrad_v3n<64, 128>(x, dy, dw, g, st, pl);
      break;
    default:
      rc = pl.k == Kern::W_V2_128 ? launch_wgrad<T, 128, 128>(x, dy, dw, g, st, pl)
                                  : launch_wgrad<T, 64, 64>(x, dy, dw, g, st, pl);
  }
  if (rc != 0 || g.dws == nullptr) return rc;
  // deterministic mode: sum the splits' workspace slabs into dw, in split order
  return launch(wgrad_split_reduce, grid_cap(ceil_div(g.dws_slab, 256), 2048), st, g.dws, dw, g.dws_slab, pl.splits);
}

}  // namespace

// ================================================================ C ABI (include/dmayolo.h)
// A dtype other than 0 (fp32) or 1 (bf16) is refused with hipErrorInvalidValue before anything else is looked at.
// fp32 OIHW weight -> e4m3 OHWI [K][KH][KW][C] with a per-output-channel scale wscale[k] = amax_k / 448
__global__ void __launch_bounds__(256) wprep_fp8_kernel(const float* __restrict__ w, unsigned char* __restrict__ w8,
                                                        float* __restrict__ wscale, int C, int KH, int KW) {
  __shared__ float red[4];
  const int k = blockIdx.x, n = C * KH * KW;
  const float* src = w + (long)k * n;
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(src[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float inv = m > 0.f ? 448.f / m : 1.f;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {  // C % 128 == 0: 4 consecutive channels share (kh, kw)
    const int c = i % C, t = i / C, kw = t % KW, kh = t / KW;
    const float* s0 = src + ((long)c * KH + kh) * KW + kw;
    const long cs = (long)KH * KW;
    *reinterpret_cast<unsigned*>(w8 + (long)k * n + i) =
        pack4_e4m3(s0[0] * inv, s0[cs] * inv, s0[2 * cs] * inv, s0[3 * cs] * inv);
  }
  if (threadIdx.x == 0) wscale[k] = m > 0.f ? m / 448.f : 1.f;
}

// dmy_conv_route's weight-grad branch (declared in conv_plan.h)
int conv_wgrad_route(int dtype, const void* x, const void* dy, int N, int H, int W, int C, long xps, int K, int KH,
                     int KW, int S, int P, int OH, int OW, long yps) {
  const Geom g = make_geom(N, H, W, C, xps, K, KH, KW, S, P, OH, OW, yps);
  return by_dtype(dtype, -1, [&](auto tag) { return (int)plan_wgrad<typename decltype(tag)::type>(g, x, dy).k; });
}

DMY_API int dmy_conv_wprep_fp8(const float* w_oihw, void* w8, float* wscale, int K, int C, int KH, int KW,
                               void* stream) {
  if (C % 4 != 0) return (int)hipErrorInvalidValue;
  return launch(wprep_fp8_kernel, K, stream, w_oihw, w8, wscale, C, KH, KW);
}

// the weight-grad entries' body: g carries the flags; det = deterministic mode, whose splits (when more than one)
// store to the workspace ws of ws_elems floats instead of fp32 atomics
static int wgrad_entry(int dtype, const void* x, const void* dy, float* dw, Geom g, void* stream, bool det = false,
                       float* ws = nullptr, long ws_elems = 0) {
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const long slab = (long)g.K * g.KH * g.KW * g.C;
    if (const int splits = det ? plan_wgrad<T>(g, x, dy).splits : 1; splits > 1) {
      if (ws == nullptr || ws_elems < splits * slab) return kInvalid;
      g.dws = ws;
      g.dws_slab = slab;
    }
    return conv_wgrad_t<T>(x, dy, dw, g, (hipStream_t)stream);
  });
}

DMY_API int dmy_conv_wgrad(int dtype, const void* x, const void* dy, float* dw_ohwi, int N, int H, int W, int C,
                           long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, void* stream) {
  return wgrad_entry(dtype, x, dy, dw_ohwi, make_geom(N, H, W, C, xps, K, KH, KW, S, P, OH, OW, yps), stream);
}

DMY_API int dmy_conv_wgrad_ex(int dtype, const void* x, const void* dy, float* dw, int N, int H, int W, int C,
                              long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, int flags,
                              void* stream) {
  return wgrad_entry(dtype, x, dy, dw, make_geom(N, H, W, C, xps, K, KH, KW, S, P, OH, OW, yps, flags), stream);
}

// deterministic weight-grad: fp32 workspace elements it needs (0 = the dispatch uses one split: no workspace; 0 also
// for a dtype outside {0, 1})
DMY_API long dmy_conv_wgrad_ws_elems(int dtype, const void* x, const void* dy, int N, int H, int W, int C, long xps,
                                     int K, int KH, int KW, int S, int P, int OH, int OW, long yps, int flags) {
  (void)flags;  // the output layout and the memset do not change the split
  const Geom g = make_geom(N, H, W, C, xps, K, KH, KW, S, P, OH, OW, yps);
  const int splits = by_dtype(dtype, 0, [&](auto tag) { return plan_wgrad<typename decltype(tag)::type>(g, x, dy).splits; });
  return splits > 1 ? (long)splits * K * KH * KW * C : 0;
}

DMY_API int dmy_conv_wgrad_det(int dtype, const void* x, const void* dy, float* dw, int N, int H, int W, int C,
                               long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps, int flags,
                               float* ws, long ws_elems, void* stream) {
  return wgrad_entry(dtype, x, dy, dw, make_geom(N, H, W, C, xps, K, KH, KW, S, P, OH, OW, yps, flags), stream, true,
                     ws, ws_elems);
}

DMY_API int dmy_conv_wprep(int dtype, const float* w_oihw, void* w_ohwi, void* w_ihwo, int K, int C, int Cp, int KH,
                           int KW, void* stream) {
  const long total = (long)K * Cp * KH * KW;
  const int grid = grid_cap(ceil_div(total, 256), 1024);
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(wprep_kernel<T>, grid, stream, w_oihw, w_ohwi, w_ihwo, K, C, Cp, KH, KW);
  });
}

// descs: device array of n WprepDesc {w, wf, wt (nullable), K, C, KH, KW} (40 bytes each, include/dmayolo.h)
DMY_API int dmy_conv_wprep_multi(int dtype, const void* descs, int n, void* stream) {
  static_assert(sizeof(WprepDesc) == 40, "WprepDesc layout is part of the C ABI");
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return n <= 0 ? 0 : launch(wprep_multi_kernel<T>, dim3(128, n), stream, descs);
  });
}

DMY_API int dmy_conv_wprep_s2d(int dtype, const float* w_oihw, void* w_s2d, int K, int C, int Cs, void* stream) {
  const int grid = grid_cap(ceil_div((long)K * 9 * Cs, 256), 1024);
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(wprep_s2d_kernel<T>, grid, stream, w_oihw, w_s2d, K, C, Cs);
  });
}

DMY_API int dmy_conv_wgrad_s2d_to_oihw(const float* dw_s2d, float* dw_oihw, int K, int C, int Cs, void* stream) {
  return launch(wgrad_s2d_to_oihw_kernel, grid_cap(ceil_div((long)K * C * 36, 256), 1024), stream, dw_s2d, dw_oihw, K, C,
                Cs);
}

DMY_API int dmy_conv_wgrad_to_oihw(const float* dw_ohwi, float* dw_oihw, int K, int C, int Cp, int KH, int KW,
                                   void* stream) {
  const long total = (long)K * C * KH * KW;
  return launch(wgrad_to_oihw_kernel, grid_cap(ceil_div(total, 256), 1024), stream, dw_ohwi, dw_oihw, K, C, Cp, KH, KW);
}
