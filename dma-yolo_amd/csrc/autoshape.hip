// AutoShape's two ends on the GPU (models/common.py:701-808).
//
// dmy_letterbox_batch: for a batch of decoded images of different sizes, one launch does what AutoShape.forward
// lines 775-778 do per image on the host -- letterbox(im, new_shape=shape1, auto=False) (cv2.resize INTER_LINEAR +
// the 114 border), stack, BHWC -> BCHW, / 255, cast -- and writes what Model.to_input would make of that batch: the
// stem's input in the activation dtype, space-to-depth (the layout of dmy_image_s2d) or channel-padded NHWC (the
// layout of dmy_nchw_to_nhwc).  The resize is mosaic_compose_kernel's (augment.hip): the 11-bit fixed-point
// horizontal and vertical passes from host-built per-axis tables, (v + 2^21) >> 22, saturated, so the uint8 level
// equals data.letterbox's bit for bit; the level times `scale` is the same single fp32 product the two layout
// kernels form.  The padded uint8 image is never stored.  One thread produces one output pixel vector (a whole
// space-to-depth pixel = 2 x 2 image pixels, or one padded NHWC pixel) and stores it as whole 16-byte vectors;
// neighbouring threads take neighbouring columns, so the taps of a wave fall on a few source rows (a gather of
// 4 taps x 3 bytes per image pixel, served by L2).
//
// dmy_scale_boxes: scale_coords (utils/general.py:605-617) over the padded NMS output of the whole batch, plus the
// Detections conversions (common.py:805-808: xyxy2xywh and the two divisions by the image size), one thread per kept
// row.  fp32 in the reference's order with IEEE divisions, so the rows equal torch's CPU result bit for bit.
#include "launch.h"

// no contraction: every sum, difference and quotient below rounds on its own, as the torch ops they replace do
#pragma clang fp contract(off)

namespace {

// Host-built descriptor, one per image (C ABI: 8-byte fields first; dmayolo/models/common.py LETTERBOX_DESC)
struct LetterboxDesc {
  const unsigned char* src;  // decoded image, HWC uint8, 3 channels, H0 x W0
  const int* xt;             // [4][w]: x0, x1, a0, a1 of the resized columns (augment._resize_table)
  const int* yt;             // [4][h]: y0, y1, b0, b1 of the resized rows
  int H0, W0, h, w;          // source size, unpadded (resized) size
  int top, left;             // where the resized image starts on the OH x OW canvas
  int swap;                  // 1: the source is BGR (data._read_bgr), the output RGB
  int pad_;
};
static_assert(sizeof(LetterboxDesc) == 56, "LetterboxDesc layout is part of the C ABI");

DEV int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the letterboxed uint8 levels (RGB order of the output) of canvas pixel (yy, xx), times scale
DEV void canvas_px(const LetterboxDesc& d, int yy, int xx, float scale, float* o) {
  const int yr = yy - d.top, xr = xx - d.left;
  if ((unsigned)yr >= (unsigned)d.h || (unsigned)xr >= (unsigned)d.w) {
    o[0] = o[1] = o[2] = 114.f * scale;
    return;
  }
  // table indices are clamped to the source: a bad table reads a wrong pixel, never outside the image
  const int x0 = clampi(d.xt[xr], d.W0 - 1), x1 = clampi(d.xt[d.w + xr], d.W0 - 1);
  const int a0 = d.xt[2 * d.w + xr], a1 = d.xt[3 * d.w + xr];
  const int y0 = clampi(d.yt[yr], d.H0 - 1), y1 = clampi(d.yt[d.h + yr], d.H0 - 1);
  const int b0 = d.yt[2 * d.h + yr], b1 = d.yt[3 * d.h + yr];
  const unsigned char* r0 = d.src + (long)y0 * d.W0 * 3;
  const unsigned char* r1 = d.src + (long)y1 * d.W0 * 3;
  const unsigned char *p00 = r0 + x0 * 3, *p01 = r0 + x1 * 3, *p10 = r1 + x0 * 3, *p11 = r1 + x1 * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cs = d.swap ? 2 - c : c;
    // a0 + a1 and b0 + b1 are 2048 (+- 1 of rounding): 255 * 2049 * 2049 + 2^21 < 2^31, int32 holds every step
    const int h0 = (int)p00[cs] * a0 + (int)p01[cs] * a1;
    const int h1 = (int)p10[cs] * a0 + (int)p11[cs] * a1;
    const int v = (h0 * b0 + h1 * b1 + (1 << 21)) >> 22;
    o[c] = (float)(v < 0 ? 0 : (v > 255 ? 255 : v)) * scale;
  }
}

// P = 2: space-to-depth [N][OH/2][OW/2][Cs], channel (dy * 2 + dx) * 3 + c;  P = 1: [N][OH][OW][Cs], channel c;
// channels past the image's are zero.  blockIdx.y = image
template <typename T, int P>
__global__ void __launch_bounds__(256) letterbox_batch_kernel(const LetterboxDesc* __restrict__ descs,
                                                              T* __restrict__ y, int OH, int OW, int Cs, float scale) {
  constexpr int VW = Traits<T>::VW, NV = P * P * 3, NVEC = (NV + VW - 1) / VW;
  const LetterboxDesc d = descs[blockIdx.y];
  const int H2 = OH / P, W2 = OW / P;
  const long total = (long)H2 * W2;
  T* img = y + (long)blockIdx.y * total * Cs;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int oy = (int)(i / W2), ox = (int)(i - (long)oy * W2);
    float v[NVEC * VW];
#pragma unroll
    for (int q = 0; q < P * P; ++q) canvas_px(d, P * oy + (q >> 1), P * ox + (q & 1), scale, v + q * 3);
#pragma unroll
    for (int j = NV; j < NVEC * VW; ++j) v[j] = 0.f;
    T* dst = img + i * Cs;
#pragma unroll
    for (int k = 0; k < NVEC; ++k) *reinterpret_cast<uint4*>(dst + k * VW) = pack<T>(v + k * VW);
    const float z[VW] = {};
    for (int c0 = NVEC * VW; c0 < Cs; c0 += VW) *reinterpret_cast<uint4*>(dst + c0) = pack<T>(z);
  }
}

template <int P>
int launch_letterbox(int dtype, const void* descs, int n, void* y, int OH, int OW, int Cs, float scale, void* stream) {
  const dim3 grid((unsigned)grid_cap(ceil_div((long)(OH / P) * (OW / P), 256), 8192), (unsigned)n);
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(letterbox_batch_kernel<T, P>, grid, stream, descs, y, OH, OW, Cs, scale);
  });
}

// one thread per row of the padded NMS output [nimg][max_det][6] = (x1, y1, x2, y2, conf, cls)
__global__ void __launch_bounds__(256) scale_boxes_kernel(float* __restrict__ det, const int* __restrict__ counts,
                                                          const float* __restrict__ geom, float* __restrict__ xywh,
                                                          float* __restrict__ xyxyn, float* __restrict__ xywhn,
                                                          int nimg, int max_det) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)nimg * max_det) return;
  const int b = (int)(i / max_det), r = (int)(i - (long)b * max_det);
  if (r >= counts[b]) return;  // rows at or past the keep count are not touched
  const float gain = geom[b * 5], px = geom[b * 5 + 1], py = geom[b * 5 + 2], w0 = geom[b * 5 + 3], h0 = geom[b * 5 + 4];
  float* p = det + i * 6;
  // scale_coords: subtract the pad, divide by the gain, clamp (clip_coords)
  const float x1 = fminf(fmaxf(__fdiv_rn(p[0] - px, gain), 0.f), w0), y1 = fminf(fmaxf(__fdiv_rn(p[1] - py, gain), 0.f), h0);
  const float x2 = fminf(fmaxf(__fdiv_rn(p[2] - px, gain), 0.f), w0), y2 = fminf(fmaxf(__fdiv_rn(p[3] - py, gain), 0.f), h0);
  const float conf = p[4], cls = p[5];
  // xyxy2xywh
  const float cx = __fdiv_rn(x1 + x2, 2.f), cy = __fdiv_rn(y1 + y2, 2.f), bw = x2 - x1, bh = y2 - y1;
  const float a[6] = {x1, y1, x2, y2, conf, cls};
  const float c[6] = {cx, cy, bw, bh, conf, cls};
  const float an[6] = {__fdiv_rn(x1, w0), __fdiv_rn(y1, h0), __fdiv_rn(x2, w0), __fdiv_rn(y2, h0), conf, cls};
  const float cn[6] = {__fdiv_rn(cx, w0), __fdiv_rn(cy, h0), __fdiv_rn(bw, w0), __fdiv_rn(bh, h0), conf, cls};
#pragma unroll
  for (int k = 0; k < 6; k += 2) {  // rows of 24 bytes: 8-byte aligned pairs
    *reinterpret_cast<float2*>(p + k) = make_float2(a[k], a[k + 1]);
    *reinterpret_cast<float2*>(xywh + i * 6 + k) = make_float2(c[k], c[k + 1]);
    *reinterpret_cast<float2*>(xyxyn + i * 6 + k) = make_float2(an[k], an[k + 1]);
    *reinterpret_cast<float2*>(xywhn + i * 6 + k) = make_float2(cn[k], cn[k + 1]);
  }
}

}  // namespace

DMY_API long dmy_letterbox_desc_bytes() { return (long)sizeof(LetterboxDesc); }

// descs: device array of n LetterboxDesc; host_descs: the host copy the device array was uploaded from, read here
// for the geometry checks (the kernel never sees it).  y: the stem input of the whole batch, dtype 0 fp32 / 1 bf16,
// s2d = 1 [n][OH/2][OW/2][Cs] (Cs >= 12) or s2d = 0 [n][OH][OW][Cs] (Cs >= 3), Cs whole 16-byte vectors.
// hipErrorInvalidValue before any launch for odd OH / OW with s2d, a resized rectangle outside the canvas, an empty
// image, a Cs that is not a vector multiple or an unaligned y.
DMY_API int dmy_letterbox_batch(int dtype, const void* descs, const void* host_descs, int n, void* y, int OH, int OW,
                                int s2d, int Cs, float scale, void* stream) {
  if (n <= 0) return 0;
  if (!descs || !host_descs || OH < 1 || OW < 1 || (dtype != 0 && dtype != 1)) return kInvalid;
  if (s2d && ((OH | OW) & 1)) return kInvalid;
  if (Cs < (s2d ? 12 : 3) || !vec_ok(vec_width(dtype), Cs, {}, {y})) return kInvalid;
  const LetterboxDesc* h = (const LetterboxDesc*)host_descs;
  for (int k = 0; k < n; ++k) {
    const LetterboxDesc& d = h[k];
    if (!d.src || !d.xt || !d.yt || d.H0 < 1 || d.W0 < 1 || d.h < 1 || d.w < 1) return kInvalid;
    if (d.top < 0 || d.left < 0 || d.top > OH - d.h || d.left > OW - d.w) return kInvalid;
  }
  return s2d ? launch_letterbox<2>(dtype, descs, n, y, OH, OW, Cs, scale, stream)
             : launch_letterbox<1>(dtype, descs, n, y, OH, OW, Cs, scale, stream);
}

// det: fp32 [nimg][max_det][6] rows of non_max_suppression, rewritten in place; counts: int32 [nimg] keep counts
// (device-readable); geom: fp32 [nimg][5] = gain, pad_x, pad_y, w0, h0; xywh / xyxyn / xywhn: fp32 buffers of det's
// shape, written for the kept rows only
DMY_API int dmy_scale_boxes(void* det, const void* counts, const void* geom, void* xywh, void* xyxyn, void* xywhn,
                            int nimg, int max_det, void* stream) {
  if (nimg <= 0 || max_det <= 0) return 0;
  if (!det || !counts || !geom || !xywh || !xyxyn || !xywhn) return kInvalid;
  for (const void* p : {(const void*)det, (const void*)xywh, (const void*)xyxyn, (const void*)xywhn})
    if (((uintptr_t)p) & 7) return kInvalid;
  return launch(scale_boxes_kernel, dim3(ceil_div((long)nimg * max_det, 256)), stream, det, counts, geom, xywh, xyxyn,
                xywhn, nimg, max_det);
}
