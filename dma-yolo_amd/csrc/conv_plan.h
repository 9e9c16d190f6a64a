// Host code shared by conv.hip and conv_wgrad.hip: the launch geometry, the buffer-descriptor extents, the kernel
// codes and plan records of the routing, and the declaration of the one host function that crosses the two units.
#pragma once
#include "conv_core.h"
#include "launch.h"

namespace {

#define DMY_WGRAD_OIHW 1
#define DMY_WGRAD_ZEROED 2
// flags: the weight-grad's DMY_WGRAD_* bits (output layout, caller-cleared output)
Geom make_geom(int N, int H, int W, int C, long xps, int K, int KH, int KW, int S, int P, int OH, int OW, long yps,
               int flags = 0) {
  Geom g;
  g.N = N; g.H = H; g.W = W; g.C = C; g.K = K; g.KH = KH; g.KW = KW; g.S = S; g.P = P;
  g.OH = OH; g.OW = OW; g.xps = xps; g.yps = yps;
  g.oihw = flags & DMY_WGRAD_OIHW ? 1 : 0;
  g.zeroed = flags & DMY_WGRAD_ZEROED ? 1 : 0;
  g.dws = nullptr; g.dws_slab = 0;
  return g;
}
inline int num_cus() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

inline bool is_p1(const Geom& g) { return g.KH == 1 && g.KW == 1 && g.S == 1 && g.P == 0; }
// byte extents of the bf16 operands of g (H x W x C gather tensor, OH x OW x K output, K x KH x KW x C weights): the
// num_records of their buffer descriptors, which must stay below the out-of-range offset v3::kBufOob
inline double x_bytes(const Geom& g) { return 2.0 * ((double)g.N * g.H * g.W * g.xps); }
inline double y_bytes(const Geom& g) { return 2.0 * ((double)g.N * g.OH * g.OW * g.yps); }
inline double w_bytes(const Geom& g) { return 2.0 * g.K * g.KH * g.KW * g.C; }
inline bool fits_buf(double bytes) { return bytes < (double)v3::kBufOob; }

// ---------------------------------------------------------------- routing plans
// One function decides which kernel a bf16 implicit-GEMM launch takes; the launch executes that plan and
// dmy_conv_fwd_bn_rows reads the BN partial-row count off the same plan, so the two cannot drift.
// The values are the DMY_KERN_* codes of include/dmayolo.h (dmy_conv_route): append, never renumber.
enum class Kern {
  // forward, and the stride-1 data-grad as a forward over its GEMM view (V2 = the 64 x 64 register-staged tile)
  HALO, SPLITK, P1S, STEM, P1P, PIPE8, WIDE, WIDE288, TALL, V3, V2,
  // data-grad: v2 128 x 128 tile; stride 2 as one GEMM (32 / 64-128 channels), four classes merged, one launch a class
  V2_BIG, S2_Q2S, S2_Q2, S2_MERGED, S2_CLASS,
  // weight-grad: tap-fused 128 / 64 / 64-row two-plane tiles, v4, v3, v3n with 128 / 256 columns, v2 128 / 64 tiles
  W_TAP128, W_TAP64, W_TAP64X2, W_V4, W_V3, W_V3N128, W_V3N256, W_V2_128, W_V2_64
};
struct Plan {
  Kern k;
  bool buf;   // buffer-descriptor loader (C % 64 == 0, byte offsets < 4 GiB)
  bool lane;  // P1P: per-lane BN partials, one row per wave of the persistent grid
  long rows;  // BN partial rows the launch writes (when it writes them)
};
struct WPlan {
  Kern k;
  int splits, per;  // split-K over pixels: splits launches' worth of grid.y, per K steps each
};

}  // namespace

// The weight-grad's DMY_KERN_* code for dmy_conv_route (conv.hip), defined in conv_wgrad.hip next to plan_wgrad:
// the only function that crosses the two units.  It takes dmy_conv_wgrad's geometry arguments, not a Geom: Geom lives
// in each unit's anonymous namespace (as the kernels that take it by value do), so it cannot type an external function.
// -1 for a dtype outside {0, 1}.
__attribute__((visibility("hidden"))) int conv_wgrad_route(int dtype, const void* x, const void* dy, int N, int H,
                                                           int W, int C, long xps, int K, int KH, int KW, int S, int P,
                                                           int OH, int OW, long yps);
