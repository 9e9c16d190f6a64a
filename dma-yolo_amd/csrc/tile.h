// The channel tile of the streaming NHWC kernels that reduce over pixels (dwconv.hip, convmix.hip): a thread owns one
// channel unit (a 16-byte vector, or 4 channels), a block of 256 threads covers a tile of TC = 1 << tcl units (a power of
// two <= 32, blockIdx.y picks the tile) by 256 / TC pixel slots.  Reductions go lane -> wave (xor shuffles over the lanes
// that share a unit) -> block (the four waves through LDS, summed in wave order) -> one row per block: no atomics.
#pragma once
#include "common.h"

// channel units per block tile: the next power of two for <= 32 units, else the one of 32 / 16 / 8 that pads least
inline int tile_log2(int units) {
  if (units <= 32) {
    int l = 0;
    while ((1 << l) < units) ++l;
    return l;
  }
  int best = 5;
  long pad = (long)ceil_div(units, 32) * 32;
  for (int l = 4; l >= 3; --l) {
    const long p = (long)ceil_div(units, 1 << l) * (1 << l);
    if (p < pad) { pad = p; best = l; }
  }
  return best;
}

template <typename T> DEV void load_vec(const T* p, float* f) { unpack<T>(*reinterpret_cast<const uint4*>(p), f); }

DEV void load4(const float* p, float* f) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}
DEV void load4(const bf16* p, float* f) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  const bf16* e = reinterpret_cast<const bf16*>(&v);
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = to_f(e[i]);
}

// sum over the lanes of a wave that share a channel unit (lane % TC), TC = 1 << tcl <= 32
DEV float unit_sum(float v, int tcl) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
    if (o >= (1 << tcl)) v += __shfl_xor(v, o, 64);
  return v;
}

// the thread's place in a tile of 16-byte vectors: first channel c0 (0 when the unit is past C: cok false), pixel slot
// rr of PIX per block
struct Tile {
  int c0, rr, PIX;
  bool cok;
  DEV Tile(int tcl, int C, int VW) {
    const int TC = 1 << tcl, cv = blockIdx.y * TC + (threadIdx.x & (TC - 1));
    cok = cv < C / VW;
    c0 = cok ? cv * VW : 0;
    rr = threadIdx.x >> tcl;
    PIX = 256 >> tcl;
  }
};

// this block's row of two [rows][C] partial arrays from the per-thread sums a, b; pb may be null (block-uniform).
// Every thread of the block must call it.
template <int VW>
DEV void write_rows(const float* a, const float* b, int tcl, int C, float* __restrict__ pa, float* __restrict__ pb) {
  __shared__ float red[4][2 * 32 * VW];
  const int TC = 1 << tcl, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < VW; ++e) {
    const float s = unit_sum(a[e], tcl), q = unit_sum(b[e], tcl);
    if (lane < TC) {
      red[wave][lane * VW + e] = s;
      red[wave][32 * VW + lane * VW + e] = q;
    }
  }
  __syncthreads();
  const int nch = TC * VW;
  for (int idx = threadIdx.x; idx < 2 * nch; idx += 256) {
    const int half = idx >= nch, cc = idx - half * nch, ch = blockIdx.y * nch + cc;
    if (ch < C && (half ? pb : pa)) {
      const int o = half * 32 * VW + cc;
      (half ? pb : pa)[(long)blockIdx.x * C + ch] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    }
  }
}
