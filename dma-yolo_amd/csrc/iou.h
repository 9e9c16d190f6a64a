// bbox_iou (utils/metrics.py:192-252) in forward-mode duals: every criterion the reference's keywords select, with
// box 1 carrying the four derivatives and box 2 constant.  One prelude (corners, intersection, union, convex width
// and height; metrics.py:197-218) feeds the five tails:
//   kIouSIoU   metrics.py:219-235   iou - (distance_cost + shape_cost) / 2
//   kIouCIoU   metrics.py:238-247   iou - (rho2 / c2 + v alpha), alpha = v / (v - iou + (1 + eps)) a CONSTANT (the
//                                   reference computes it under no_grad): only v and iou carry derivatives
//   kIouDIoU   metrics.py:238-242   iou - rho2 / c2
//   kIouGIoU   metrics.py:248-250   iou - (c_area - union) / c_area
//   kIouPlain  metrics.py:215, 252  iou
// eps = 1e-7 sits where the reference adds it (h1, h2, union, c2, c_area); rho2 is the sum of squares / 4.  Ties follow
// dual.h: dmin / dmax split the derivative, dclamp0 passes it at 0, which is what torch.min / max / clamp(0) do.
// XYXY = false: box 1 is (x, y, w, h) and the seeds sit on those (the loss's form, x1y1x2y2=False); XYXY = true: the
// four corners are used as given and carry the seeds.  The numbering is the C ABI's DMY_IOU_* (include/dmayolo.h).
#pragma once
#include "dual.h"

constexpr int kIouSIoU = DMY_IOU_SIOU, kIouCIoU = DMY_IOU_CIOU, kIouDIoU = DMY_IOU_DIOU, kIouGIoU = DMY_IOU_GIOU,
              kIouPlain = DMY_IOU_PLAIN;

template <int KIND, bool XYXY>
DEV D4 bbox_iou_d4(D4 p0, D4 p1, D4 p2, D4 p3, float q0, float q1, float q2, float q3) {
  const float eps = 1e-7f;
  D4 b1x1, b1x2, b1y1, b1y2, b2x1, b2x2, b2y1, b2y2;
  if constexpr (XYXY) {
    b1x1 = p0; b1y1 = p1; b1x2 = p2; b1y2 = p3;
    b2x1 = dc(q0); b2y1 = dc(q1); b2x2 = dc(q2); b2y2 = dc(q3);
  } else {
    b1x1 = p0 - scal(p2, 0.5f); b1x2 = p0 + scal(p2, 0.5f);
    b1y1 = p1 - scal(p3, 0.5f); b1y2 = p1 + scal(p3, 0.5f);
    b2x1 = dc(q0 - q2 / 2); b2x2 = dc(q0 + q2 / 2);
    b2y1 = dc(q1 - q3 / 2); b2y2 = dc(q1 + q3 / 2);
  }
  D4 inter = dclamp0(dmin(b1x2, b2x2) - dmax(b1x1, b2x1)) * dclamp0(dmin(b1y2, b2y2) - dmax(b1y1, b2y1));
  D4 w1 = b1x2 - b1x1, h1 = b1y2 - b1y1 + dc(eps);
  D4 w2 = b2x2 - b2x1, h2 = b2y2 - b2y1 + dc(eps);
  D4 uni = w1 * h1 + w2 * h2 - inter + dc(eps);
  D4 iou = inter / uni;
  D4 cw = dmax(b1x2, b2x2) - dmin(b1x1, b2x1);  // convex (smallest enclosing box) width and height: every kind but
  D4 ch = dmax(b1y2, b2y2) - dmin(b1y1, b2y1);  // the plain IoU, where they are dead code
  if constexpr (KIND == kIouPlain) {
    return iou;
  } else if constexpr (KIND == kIouSIoU) {
    D4 scw = scal(b2x1 + b2x2 - b1x1 - b1x2, 0.5f);
    D4 sch = scal(b2y1 + b2y2 - b1y1 - b1y2, 0.5f);
    D4 sigma = dsqrt(dsq(scw) + dsq(sch));
    D4 sa1 = dabs(scw) / sigma, sa2 = dabs(sch) / sigma;
    const float thr = 0.70710678118654757f;  // pow(2, 0.5) / 2 (python double -> fp32 compare)
    D4 sa = sa1.v > thr ? sa2 : sa1;
    D4 ang = dcos(scal(dasin(sa), 2.f) - dc(1.5707963267948966f));
    D4 rx = dsq(scw / cw), ry = dsq(sch / ch);
    D4 gam = ang - dc(2.f);
    D4 dist = dc(2.f) - dexp(gam * rx) - dexp(gam * ry);
    D4 ow = dabs(w1 - w2) / dmax(w1, w2);
    D4 oh = dabs(h1 - h2) / dmax(h1, h2);
    D4 shape = dpow4(dc(1.f) - dexp(scal(ow, -1.f))) + dpow4(dc(1.f) - dexp(scal(oh, -1.f)));
    return iou - scal(dist + shape, 0.5f);
  } else if constexpr (KIND == kIouCIoU || KIND == kIouDIoU) {
    D4 c2 = dsq(cw) + dsq(ch) + dc(eps);  // convex diagonal squared
    D4 rho2 = scal(dsq(b2x1 + b2x2 - b1x1 - b1x2) + dsq(b2y1 + b2y2 - b1y1 - b1y2), 0.25f);  // centre distance squared
    if constexpr (KIND == kIouDIoU) {
      return iou - rho2 / c2;
    } else {
      const float k = (float)(4.0 / (M_PI * M_PI));  // python double -> fp32 scalar
      D4 v = scal(dsq(datan(w2 / h2) - datan(w1 / h1)), k);
      const float alpha = v.v / (v.v - iou.v + (float)(1.0 + 1e-7));  // no_grad: a constant
      return iou - (rho2 / c2 + scal(v, alpha));
    }
  } else {
    static_assert(KIND == kIouGIoU, "unknown IoU kind");
    D4 c_area = cw * ch + dc(eps);  // convex area
    return iou - (c_area - uni) / c_area;
  }
}
