// Device primitives shared by the convolution translation units conv.hip (forward, data-grad, fp8) and
// conv_wgrad.hip (weight-grad, weight prep): the tile shapes, the LDS placement of m-major and k-major tiles, the MFMA
// fragment reads, the register-staged (v2) pipelined main loop, the launch geometry, the XCD tile order and the basics
// of the LDS-DMA (v3) kernels.  Header code with internal linkage: the build has no relocatable device code, so a
// kernel and every device function it calls live in one translation unit, and each unit gets its own copy of these
// (and of g_zero_page).  What only one pass uses (loaders, epilogues, kernels, routing) is in that pass's .hip file.
#pragma once
#include "common.h"

namespace {

constexpr int NT = 256;  // 4 waves, 2x2 over the block tile

template <typename T> struct Cfg;
template <> struct Cfg<bf16> {
  static constexpr int BK = 64, PADM = 8, PADK = 0;  // m-major rows 144 B; k-major rows unpadded (swizzled)
};
template <> struct Cfg<float> {
  static constexpr int BK = 32, PADM = 4, PADK = 16;
};

template <typename T, int BM, int BN, bool AK, bool BKM> struct Tile {
  static constexpr int BK = Cfg<T>::BK, VW = Traits<T>::VW;
  static constexpr int RSM = BK + Cfg<T>::PADM;  // m-major row stride (elements)
  static constexpr int A_ELEMS = AK ? BK * (BM + Cfg<T>::PADK) : BM * RSM;
  static constexpr int B_ELEMS = BKM ? BK * (BN + Cfg<T>::PADK) : BN * RSM;
  static constexpr int STAGE = A_ELEMS + B_ELEMS;
  static constexpr int TM = BM / 32, TN = BN / 32;
  static constexpr int STAGE_BYTES = 2 * STAGE * (int)sizeof(T);
  static constexpr int CT_BYTES = BM * (BN + 8) * 4;  // C tile (largest epilogue use, fp32 worst case)
  static constexpr int LDS_BYTES = STAGE_BYTES > CT_BYTES ? STAGE_BYTES : CT_BYTES;
};

// ---------------------------------------------------------------- LDS placement helpers
// k-major tile [k][ROW] with ROW = BM (or BN) elements; bf16 16-B chunks XOR-swizzled per k-row
template <typename T, int ROW> DEV int kmaj_off(int k, int row) {
  if constexpr (sizeof(T) == 2) {
    constexpr int RB = ROW * 2;  // bytes per k-row
    const int c = row >> 3, w = row & 7;
    int key;
    if constexpr (RB >= 256) key = 2 * ((k & 3) | (((k >> 3) & 1) << 2));
    else key = 2 * (((k >> 1) & 1) | (((k >> 3) & 1) << 1));
    return k * ROW + (((c ^ key) & (ROW / 8 - 1)) << 3) + w;
  } else {
    return k * (ROW + Cfg<float>::PADK) + row;
  }
}
// the inverse on a pixel row of the LDS-DMA image: physical 16-B slot `slot` of k-row `row` holds the logical chunk
// (slot ^ key(row)) & (slots - 1), key as in kmaj_off<bf16, ROW>
template <int ROW> DEV int kmaj_chunk(int row, int slot) {
  constexpr int RB = ROW * 2;
  int key;
  if constexpr (RB >= 256) key = 2 * ((row & 3) | (((row >> 3) & 1) << 2));
  else key = 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
  return (slot ^ key) & (ROW / 8 - 1);
}

// ---------------------------------------------------------------- fragment reads + MFMA
// bf16: A frag lane l = A[m0 + (l&15)][8(l>>4) .. +8)
template <int RSM> DEV bf16x8 frag_m(const bf16* base, int r0, int k0, int lane) {
  return *reinterpret_cast<const bf16x8*>(base + (r0 + (lane & 15)) * RSM + k0 + 8 * (lane >> 4));
}
template <int ROW> DEV bf16x8 frag_k(const bf16* base, int r0, int k0, int lane) {
  typedef short s4 __attribute__((ext_vector_type(4)));
  const int g = lane >> 4, il = lane & 15, q = il >> 2, p = il & 3;
  const bf16* a0 = base + kmaj_off<bf16, ROW>(k0 + 8 * g + q, r0 + 4 * p);
  const bf16* a1 = base + kmaj_off<bf16, ROW>(k0 + 8 * g + 4 + q, r0 + 4 * p);
  s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a0));
  s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a1));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

template <int BM, int BN, bool AK, bool BKM>
DEV void mma_step(const bf16* As, const bf16* Bs, f32x4 (&acc)[BM / 32][BN / 32], int wm, int wn, int lane) {
  using TT = Tile<bf16, BM, BN, AK, BKM>;
  constexpr int TM = TT::TM, TN = TT::TN;
#pragma unroll
  for (int ks = 0; ks < TT::BK; ks += 32) {
    bf16x8 a[TM], b[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r0 = wm * (BM / 2) + i * 16;
      a[i] = AK ? frag_k<BM>(As, r0, ks, lane) : frag_m<TT::RSM>(As, r0, ks, lane);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int r0 = wn * (BN / 2) + j * 16;
      b[j] = BKM ? frag_k<BN>(Bs, r0, ks, lane) : frag_m<TT::RSM>(Bs, r0, ks, lane);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

template <int BM, int BN, bool AK, bool BKM>
DEV void mma_step(const float* As, const float* Bs, f32x4 (&acc)[BM / 32][BN / 32], int wm, int wn, int lane) {
  using TT = Tile<float, BM, BN, AK, BKM>;
  constexpr int TM = TT::TM, TN = TT::TN;
#pragma unroll
  for (int kk = 0; kk < TT::BK / 4; ++kk) {
    const int k = 4 * kk + (lane >> 4);
    float a[TM], b[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r = wm * (BM / 2) + i * 16 + (lane & 15);
      a[i] = AK ? As[kmaj_off<float, BM>(k, r)] : As[r * TT::RSM + k];
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int r = wn * (BN / 2) + j * 16 + (lane & 15);
      b[j] = BKM ? Bs[kmaj_off<float, BN>(k, r)] : Bs[r * TT::RSM + k];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// ---------------------------------------------------------------- pipelined main loop
// Loader contract: load(kt, ra, rb) issues the global loads of K-tile kt into registers;
//                  store(As, Bs, ra, rb) writes them into one LDS stage.
template <typename T, int BM, int BN, bool AK, bool BKM, class L>
DEV void mainloop(L& ld, int kt0, int kt1, T* lds, f32x4 (&acc)[BM / 32][BN / 32]) {
  using TT = Tile<T, BM, BN, AK, BKM>;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  uint4 ra[L::CA], rb[L::CB];
  if (kt0 >= kt1) return;
  ld.load(kt0, ra, rb);
  int buf = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    T* As = lds + buf * TT::STAGE;
    T* Bs = As + TT::A_ELEMS;
    ld.store(As, Bs, ra, rb);
    __syncthreads();
    if (kt + 1 < kt1) ld.load(kt + 1, ra, rb);
    mma_step<BM, BN, AK, BKM>(As, Bs, acc, wm, wn, lane);
    buf ^= 1;
  }
}

template <typename T, int RSM> DEV void st_m(T* base, int row, int col, const uint4& v) {
  *reinterpret_cast<uint4*>(base + row * RSM + col) = v;
}
template <typename T, int ROW> DEV void st_k(T* base, int k, int row0, const uint4& v) {
  *reinterpret_cast<uint4*>(base + kmaj_off<T, ROW>(k, row0)) = v;
}

struct Geom {
  int N, H, W, C;       // input activation (forward sense)
  int K, KH, KW, S, P;  // out channels, kernel, stride, pad
  int OH, OW;           // output spatial
  long xps, yps;        // pixel strides of x and y (elements)
  int oihw;             // weight-grad: write [K][C][KH][KW] (torch OIHW) instead of the GEMM view [K][KH][KW][C]
  int zeroed;           // weight-grad: the output is already zero (caller-cleared arena): no memset
  // weight-grad deterministic mode: split s stores its partial tile to dws[s * dws_slab + idx] (no atomics) and
  // wgrad_split_reduce sums the splits in index order; null = fp32 atomics into dw
  float* dws;
  long dws_slab;
};

// ---------------------------------------------------------------- XCD-aware tile order
// Linear block id -> logical tile id such that each XCD (block id mod 8 under round-robin
// dispatch) walks a contiguous range of logical tiles; n-tiles of one m-panel are adjacent.
// Speed only: any placement is correct.  Bijective for every grid size.
DEV int xcd_remap(int id, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = id % 8, loc = id / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

template <int BM, int BN> DEV void zero_acc(f32x4 (&acc)[BM / 32][BN / 32]) {
#pragma unroll
  for (int i = 0; i < BM / 32; ++i)
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------- LDS-DMA (v3) basics
// The pointer-form loaders (FwdLds, WgradLds, WgradLdsN) point out-of-image taps / rows past M / channels past K at a
// zero page; one internal-linkage copy per translation unit.
__device__ __attribute__((aligned(64))) uint4 g_zero_page[4] = {};

namespace v3 {
constexpr int BK = 64;

DEV void glds16(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// swizzled fragment read: rows of 64 bf16, lane gets X[r0 + (l&15)][k0 + 8(l>>4) .. +8)
DEV bf16x8 frag_sw(const bf16* X, int r0, int k0, int lane) {
  const int row = r0 + (lane & 15);
  const int chunk = (k0 >> 3) + (lane >> 4);
  return *reinterpret_cast<const bf16x8*>(X + row * 64 + ((chunk ^ (row & 6)) << 3));
}

// The buffer-descriptor loaders give an out-of-image tap, a row past M or a column past K an offset beyond the
// descriptor's record count, and the hardware's range check returns zeros.
constexpr unsigned kBufOob = 0xFFFFFFF0u;  // >= every record count used (checked on the host)

DEV __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
DEV void blds16(__amdgpu_buffer_rsrc_t r, unsigned off, char* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, off, 0, 0, 0);
}

template <int N> DEV void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
}  // namespace v3

}  // namespace
