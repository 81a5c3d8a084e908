/*
 * lqr_coldepth.h -- liblqr-1's colour-depth surface: carvers on 16-bit integer, float and double pixels.
 *
 * liblqr 0.4 takes pixels of four depths through lqr_carver_new_ext and hands them back through
 * lqr_carver_scan_ext / lqr_carver_scan_line_ext; ImageMagick's -liquid-rescale is such a caller
 * (32F, with lqr_carver_set_preserve_input_image).  This header adds exactly that surface on top of
 * lqr.h, with liblqr's prototypes and enum values, and leaves lqr.h (the plug-in's surface) as it is.
 *
 * Depths and pixel layout.  A pixel is `channels` values of one depth, interleaved:
 *   LQR_COLDEPTH_8I   unsigned char    energy reads v / 255
 *   LQR_COLDEPTH_16I  unsigned short   energy reads v / 65535
 *   LQR_COLDEPTH_32F  float            energy reads (double) v
 *   LQR_COLDEPTH_64F  double           energy reads v
 * channels is 1 .. 4 (grey, grey + alpha, RGB, RGBA) by default; lqr_imagetype.h raises that limit
 * (lqrx_set_max_channels: CMYKA and custom layouts of up to 64 channels) and sets what the channels
 * mean (CMY, CMYK, ...).  More channels than the limit in force, or a depth outside the enum, make
 * lqr_carver_new_ext return NULL with one line on stderr.  lqr_carver_new_ext(..., LQR_COLDEPTH_8I)
 * is lqr_carver_new.  Float values outside [0, 1] and negative ones are carved as they are.
 *
 * Buffer ownership (as liblqr): the carver owns `buffer` and free()s it at lqr_carver_destroy,
 * unless lqr_carver_set_preserve_input_image was called before the first resize; then the buffer is
 * never written and never freed, and the caller frees it after lqr_carver_destroy.
 *
 * Bias and rigidity masks stay 8-bit (lqr_carver_bias_add_rgb_area, lqr_carver_rigmask_add_rgb_area
 * take guchar masks whatever the carver's depth).  An attached carver may have a depth of its own.
 *
 * Read-out.  lqr_carver_scan_ext visits the pixels of the current image one by one in the order
 * liblqr visits them (rows of the carver frame: image columns when the carver is transposed) and
 * gives their image (x, y); lqr_carver_scan_line_ext gives a line at a time.  The pointer handed out
 * holds channels values of the carver's depth per pixel; it stays valid until the next scan call.
 * (lqr_carver_get_bpp is, as in liblqr, the deprecated name of lqr_carver_get_channels.)
 * lqr_carver_scan and lqr_carver_scan_line are the 8-bit forms: on a carver of another depth they
 * return FALSE.
 *
 * Extensions of lqr.h (lqrx_carver_read_image, lqrx_carver_read_image_device,
 * lqrx_carver_reload_device_batch) move w x h x channels x bytes-per-channel bytes per image on a
 * carver of any depth.
 */
#ifndef __LQR_COLDEPTH_H__
#define __LQR_COLDEPTH_H__

#include "lqr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum _LqrColDepth {
    LQR_COLDEPTH_8I = 0,
    LQR_COLDEPTH_16I = 1,
    LQR_COLDEPTH_32F = 2,
    LQR_COLDEPTH_64F = 3
} LqrColDepth;

typedef enum _LqrImageType {
    LQR_RGB_IMAGE = 0,
    LQR_RGBA_IMAGE = 1,
    LQR_GREY_IMAGE = 2,
    LQR_GREYA_IMAGE = 3,
    LQR_CMY_IMAGE = 4,
    LQR_CMYK_IMAGE = 5,
    LQR_CMYKA_IMAGE = 6,
    LQR_CUSTOM_IMAGE = 7
} LqrImageType;

LqrCarver *lqr_carver_new_ext(void *buffer, gint width, gint height, gint channels, LqrColDepth colour_depth);
void lqr_carver_set_preserve_input_image(LqrCarver *r);

gboolean lqr_carver_scan(LqrCarver *r, gint *x, gint *y, guchar **rgb);
gboolean lqr_carver_scan_ext(LqrCarver *r, gint *x, gint *y, void **rgb);
gboolean lqr_carver_scan_line_ext(LqrCarver *r, gint *n, void **rgb);

LqrColDepth lqr_carver_get_col_depth(LqrCarver *r);
LqrImageType lqr_carver_get_image_type(LqrCarver *r);
gint lqr_carver_get_bpp(LqrCarver *r);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_COLDEPTH_H__ */
