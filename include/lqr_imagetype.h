/*
 * lqr_imagetype.h -- liblqr-1's image types: carvers on CMY, CMYK, CMYKA and custom-channel pixels.
 *
 * Next to the colour depth (lqr_coldepth.h) liblqr 0.4 has a second axis, the image type: what the
 * channels of a pixel mean, and therefore which value the energy functions read.  A caller such as
 * ImageMagick's -liquid-rescale hands over every pixel channel of its image; this header adds the three
 * liblqr calls that say what they are, with liblqr's prototypes, and one extension that lifts the
 * channel limit.  lqr.h and lqr_coldepth.h stay as they are.
 *
 * Default type by channel count (lqr_carver_get_image_type): 1 GREY, 2 GREYA, 3 RGB, 4 RGBA, 5 CMYKA,
 * 6 and more CUSTOM with neither an alpha nor a black channel.
 *
 * lqr_carver_set_image_type: a type whose channel count differs from the carver's (GREY 1, GREYA 2,
 * RGB and CMY 3, RGBA and CMYK 4, CMYKA 5; CUSTOM any) returns LQR_ERROR and changes nothing.  A matching
 * one returns LQR_OK and sets the alpha / black channel indices to GREYA 1 / none, RGBA 3 / none,
 * CMYK none / 3, CMYKA 4 / 3, every other type none / none.
 * lqr_carver_set_alpha_channel, lqr_carver_set_black_channel: an index >= channels returns LQR_ERROR; a
 * negative one clears the role.  An accepted call turns the type into CUSTOM; giving one role the index
 * the other holds clears the other.
 *
 * What the energy reads.  n[k] is channel k normalised by the depth (lqr_coldepth.h); every operation
 * is rounded individually in double:
 *   GREY, GREYA   b = n[0]
 *   RGB, RGBA     (r, g, bl) = n[0 .. 2]
 *   CMY           (r, g, bl) = 1 - n[0 .. 2]
 *   CMYK, CMYKA   (r, g, bl) = (1 - n[0 .. 2]) * (1 - n[3])
 *                 brightness ((r + g) + bl) / 3, luma (0.2126 r + 0.7152 g) + 0.0722 bl
 *   CUSTOM        bf = n[black] (0 without a black channel); s = the sum over the channels k other than
 *                 alpha and black, ascending, of 1 - (1 - n[k]) (1 - bf), divided by their number;
 *                 b = 1 - s with a black channel, s without; the luma energies read the same value
 *   and b = b * n[alpha] where there is an alpha channel.
 * A CUSTOM layout that leaves no colour channel (one channel that is also the alpha channel) divides
 * zero by zero: the calls are accepted as liblqr accepts them, the result is unspecified.
 *
 * The calls may be made at any point between resizes, on a root carver or an attached one (where they
 * change only what lqr_carver_get_image_type reports: an attached carver's pixels are never read by an
 * energy function).  A call that changes what the energy reads makes the next resize lay the working
 * planes out again from the visible pixels, as a change of energy function between brightness and luma
 * does.  Pixels created by an enlargement average every channel alike, alpha and black included.
 * Bias and rigidity masks stay 8-bit guchar masks of one to four channels on a carver of any type.
 *
 * lqrx_set_max_channels (extension): the process-wide limit on `channels` of lqr_carver_new and
 * lqr_carver_new_ext.  It is 4 when the library is loaded (what gimp-lqr-plugin needs, and what
 * lqr_coldepth.h promised); a caller that hands over CMYKA or multi-channel pixels raises it once after
 * loading.  Values outside 4 .. 64 are refused (the limit stays); the previous limit is returned either
 * way.  A carver that is refused for its channel count says so on stderr, naming the limit in force.
 */
#ifndef __LQR_IMAGETYPE_H__
#define __LQR_IMAGETYPE_H__

#include "lqr_coldepth.h"

#ifdef __cplusplus
extern "C" {
#endif

LqrRetVal lqr_carver_set_image_type(LqrCarver *r, LqrImageType image_type);
LqrRetVal lqr_carver_set_alpha_channel(LqrCarver *r, gint channel_index);
LqrRetVal lqr_carver_set_black_channel(LqrCarver *r, gint channel_index);

gint lqrx_set_max_channels(gint n);

#ifdef __cplusplus
}
#endif

#endif /* __LQR_IMAGETYPE_H__ */
