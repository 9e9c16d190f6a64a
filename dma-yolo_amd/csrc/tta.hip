// Test-time augmentation input (models/yolo.py:194-209 with utils/torch_utils.py:264-274): one pass's
// x.flip -> F.interpolate(bilinear, align_corners=False) -> F.pad(0.447) -> stem layout -> act dtype in one launch.
//
// One thread produces one output pixel vector: a whole space-to-depth pixel (2x2 image pixels x C, the layout of
// dmy_image_s2d) or one channel-padded NHWC pixel (the layout of dmy_nchw_to_nhwc).  Neighbouring threads take
// neighbouring output columns, so the four taps of a channel plane read (nearly) consecutive addresses across the
// wave and every store is a 16-byte vector.  The flip is folded into the tap index; the image is normalised
// (uint8 * scale) per tap, combined in fp32 and rounded once to T.
#include "launch.h"

namespace {

struct Tap {
  int i0, i1;
  float l0, l1;
};

// torch's area_pixel_compute_source_index (align_corners=False) + guard_index_and_lambda; `flip` mirrors the taps
DEV Tap tap_of(int dst, float ratio, int in, bool flip) {
  const float src = fmaxf(0.f, ratio * ((float)dst + 0.5f) - 0.5f);
  Tap t;
  t.i0 = min((int)src, in - 1);
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  if (flip) {
    t.i0 = in - 1 - t.i0;
    t.i1 = in - 1 - t.i1;
  }
  return t;
}

// P = 2: space-to-depth [N][OHp/2][OWp/2][Cs], channel (dy*2+dx)*C+c;  P = 1: [N][OHp][OWp][Cs], channel c
template <typename S, typename T, int P>
__global__ void tta_image_kernel(const S* __restrict__ x, T* __restrict__ y, int N, int C, int H, int W, int Cs,
                                 float scale, int flip, int OH, int OW, int OHp, int OWp, float pad_value) {
  constexpr int VW = Traits<T>::VW;
  const int H2 = OHp / P, W2 = OWp / P;
  const long HW = (long)H * W, total = (long)N * H2 * W2;
  const float rh = (float)H / (float)OH, rw = (float)W / (float)OW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % W2);
    const long t = i / W2;
    const int oy = (int)(t % H2);
    const long b = t / H2;
    Tap ty[P], tx[P];
#pragma unroll
    for (int d = 0; d < P; ++d) {
      ty[d] = tap_of(min(P * oy + d, OH - 1), rh, H, flip == 2);
      tx[d] = tap_of(min(P * ox + d, OW - 1), rw, W, flip == 3);
    }
    const S* img = x + b * C * HW;
    T* dst = y + i * Cs;
    for (int c0 = 0; c0 < Cs; c0 += VW) {
      float f[VW];
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const int ch = c0 + j;
        if (ch >= P * P * C) {
          f[j] = 0.f;
          continue;
        }
        const int q = ch / C, c = ch - q * C;  // q = dy * P + dx
        const int dy = P == 2 ? (q >> 1) : 0, dx = P == 2 ? (q & 1) : 0;
        if (P * oy + dy >= OH || P * ox + dx >= OW) {
          f[j] = pad_value;
          continue;
        }
        const Tap a = dy ? ty[P - 1] : ty[0], e = dx ? tx[P - 1] : tx[0];  // selects, not indexed registers
        const S* pl = img + (long)c * HW;
        const float p00 = (float)pl[(long)a.i0 * W + e.i0] * scale, p01 = (float)pl[(long)a.i0 * W + e.i1] * scale;
        const float p10 = (float)pl[(long)a.i1 * W + e.i0] * scale, p11 = (float)pl[(long)a.i1 * W + e.i1] * scale;
        f[j] = a.l0 * (e.l0 * p00 + e.l1 * p01) + a.l1 * (e.l0 * p10 + e.l1 * p11);
      }
      *reinterpret_cast<uint4*>(dst + c0) = pack<T>(f);
    }
  }
}

template <typename S, int P>
int tta_launch(int dtype, const void* x, void* y, int N, int C, int H, int W, int Cs, float scale, int flip, int OH,
               int OW, int OHp, int OWp, float pad_value, void* stream) {
  const long n = (long)N * (OHp / P) * (OWp / P);
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    return launch(tta_image_kernel<S, typename decltype(tag)::type, P>, grid_cap(ceil_div(n, 256), 8192), stream, x, y,
                  N, C, H, W, Cs, scale, flip, OH, OW, OHp, OWp, pad_value);
  });
}

}  // namespace

// src_kind: 0 = uint8, 1 = fp32 (times scale, as dmy_image_s2d).  s2d: 1 = space-to-depth layout (OHp, OWp even,
// Cs >= 4C), 0 = channel-padded NHWC (Cs >= C); Cs a multiple of the 16-byte vector.  flip: 0 none, 2 up-down,
// 3 left-right.  Pixels outside OH x OW hold pad_value, channels past the image's hold zero.
DMY_API int dmy_tta_image(int dtype, int src_kind, const void* x, void* y, int N, int C, int H, int W, int s2d, int Cs,
                          float scale, int flip, int OH, int OW, int OHp, int OWp, float pad_value, void* stream) {
  if (dtype != 0 && dtype != 1) return kInvalid;
  const int P = s2d ? 2 : 1;
  if (N < 1 || C < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || OH > OHp || OW > OWp) return kInvalid;
  if (flip != 0 && flip != 2 && flip != 3) return kInvalid;
  if (s2d && ((OHp | OWp) & 1)) return kInvalid;
  if (!vec_ok(vec_width(dtype), Cs, {}, {}, {y}) || Cs < P * P * C) return kInvalid;
  if (src_kind == 0)
    return s2d ? tta_launch<uint8_t, 2>(dtype, x, y, N, C, H, W, Cs, scale, flip, OH, OW, OHp, OWp, pad_value, stream)
               : tta_launch<uint8_t, 1>(dtype, x, y, N, C, H, W, Cs, scale, flip, OH, OW, OHp, OWp, pad_value, stream);
  return s2d ? tta_launch<float, 2>(dtype, x, y, N, C, H, W, Cs, scale, flip, OH, OW, OHp, OWp, pad_value, stream)
             : tta_launch<float, 1>(dtype, x, y, N, C, H, W, Cs, scale, flip, OH, OW, OHp, OWp, pad_value, stream);
}
