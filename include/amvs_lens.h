/* amvs_lens.h -- lens undistortion of libamvs.so (csrc/amvs_undistort.hip) for views uploaded as raw 8-bit images.
 *
 * Why a header of its own: existing tests hold include/amvs.h to the 92 entry points of _lib.SIGNATURES and
 * include/amvs_depth.h to the one of _lib.DEPTH_SIGNATURES, and existing tests do not change.  What is declared here is
 * bound from a third table, _lib.LENS_SIGNATURES; _lib.load() binds all three.  The library, the context and the error
 * codes are those of amvs.h.
 *
 * ---- the definition -----------------------------------------------------------------------------------------------------
 * An image taken through a lens with the Brown-Conrady model (radial k1 .. k6, tangential p1, p2) is resampled into the
 * image a pinhole camera with the same K would have taken.  The definition is modelled on OpenCV's cv.undistort with its
 * defaults (new camera matrix = K, bilinear, constant border 0): a float64 map, source coordinates quantised to 5-bit
 * fractions, zero outside the image.  OpenCV is not a dependency of this library, so the text below IS the definition;
 * parity with cv2 itself is UNPINNED, as it is for the resize of amvs_set_view_bgr8.  It is judged
 * against tests/undistort_restatement.py, written from this text, byte for byte.
 *
 * Inputs.  src: [h][w][3] uint8.  K[9]: float64, row-major; fx = K[0], cx = K[2], fy = K[4], cy = K[5] are read, the
 * other entries must be 0, 0, 0, 0 and 1 (K[1], K[3], K[6], K[7] and K[8]).  dist[n_dist]: float64 with n_dist 4, 5 or 8,
 * in the order k1, k2, p1, p2, k3, k4, k5, k6; absent coefficients are 0.
 *
 * Arithmetic.  All float64: one rounding per operation, nothing contracted, in exactly the written order.  Division and
 * rint are correctly rounded; rint rounds halves to even.  Integers are converted exactly.
 *
 * For the destination pixel at column j and row i:
 *     x = (j - cx) / fx            y = (i - cy) / fy
 *     x2 = x*x    y2 = y*y    r2 = x2 + y2    xy2 = (2*x)*y
 *     num = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *     den = 1 + ((k6*r2 + k5)*r2 + k4)*r2
 *     kr  = num / den
 *     xd = (x*kr + p1*xy2) + p2*(r2 + 2*x2)
 *     yd = (y*kr + p1*(r2 + 2*y2)) + p2*xy2
 *     u = fx*xd + cx               v = fy*yd + cy
 *     fu = rint(u*32)              fv = rint(v*32)
 *
 * Outside pixels.  The pixel is OUTSIDE unless -32 <= fu < 32*w and -32 <= fv < 32*h, compared in float64 before any
 * integer conversion; NaN and +-inf fail.  An OUTSIDE pixel is written as 0, 0, 0.
 *
 * Inside pixels.  iu = (int)fu, sx = iu >> 5 (arithmetic shift: the floor), ax = iu & 31; the same gives sy and ay from
 * fv.  The four taps are (sx, sy), (sx+1, sy), (sx, sy+1) and (sx+1, sy+1) with the integer weights (32-ax)(32-ay),
 * ax(32-ay), (32-ax)ay and ax*ay, which sum to 1024.  A tap outside [0, w) x [0, h) contributes 0; its address is never
 * formed.  Per channel out = (sum of weight * byte + 512) >> 10.
 *
 * n_outside is the number of OUTSIDE pixels.
 *
 * Black border.  OUTSIDE pixels are zero and enter the sweeps' NCC as texture-less pixels, as they do after cv.undistort
 * in the reference's loader.  Masking them is out of scope.
 *
 * Errors (AMVS_EINVAL before anything is allocated): a NULL required pointer; h or w < 1 or > 2^24; n_dist not 4, 5 or
 * 8; a K entry or a coefficient that is not finite; fx or fy <= 0; a K entry that must be 0 or 1 and is not.
 *
 * amvs_undistort_bgr8: host image in, host image out ([h][w][3] each; they may not overlap); n_outside may be NULL.  It
 * touches no view of the context (the staging blocks of the uploads are used) and synchronises.  amvs_get_timing then
 * returns the device times of its three parts: init_ms the upload, sweep_ms the kernel, confidence_ms the download.
 *
 * amvs_set_view_bgr8_undistorted: amvs_set_view_bgr8 with the undistortion between the upload and the resize -- the raw
 * image is uploaded as it is, undistorted at source resolution into a second staging block of the context, and that block
 * is handed to the resize and gray kernels of amvs_set_view_bgr8, unchanged.  K_src is the calibration's own matrix at the
 * SOURCE resolution, not the context's scaled K.  Everything else (view, R, t, scaled_bgr_out, errors, synchronisation) is
 * amvs_set_view_bgr8's.                                                                                                   */
#ifndef AMVS_LENS_H
#define AMVS_LENS_H

#include "amvs.h"

#ifdef __cplusplus
extern "C" {
#endif

int amvs_undistort_bgr8(amvs_ctx *ctx, const uint8_t *bgr_host, int h, int w,
                        const double K[9], const double *dist, int n_dist,
                        uint8_t *out_host, int64_t *n_outside);

int amvs_set_view_bgr8_undistorted(amvs_ctx *ctx, int view, const uint8_t *bgr_host,
                                   int src_h, int src_w, const double K_src[9],
                                   const double *dist, int n_dist,
                                   const float R[9], const float t[3], uint8_t *scaled_bgr_out);

#ifdef __cplusplus
}
#endif

#endif
