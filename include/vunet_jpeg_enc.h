/*
 * vunet_jpeg_enc.h -- C ABI of the baseline JPEG encoder, csrc/jpeg_enc.hip (device) and csrc/jpeg_huff_enc.h (host): the uint8 RGB
 * (or gray) stack [Nslots][Hmax][Wmax][3 or 1] that every video call of the package ends in -> JFIF byte streams, byte for byte what
 * libjpeg-turbo's default encoder (RGB -> YCbCr, box down-sampling, the "islow" integer forward DCT, the Annex K tables scaled by a
 * quality, the Annex K Huffman tables) and so Pillow's Image.save(.., "JPEG", quality=q, subsampling=s) write.  The mirror image of
 * vunet_jpeg.h, whose vunet_jpeg_info / vunet_jpeg_img rows, coefficient layout and error conventions it shares.  Part of
 * libvunet_hip.so; additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root): the
 * cv2.VideoWriter / cv2.imwrite calls at the end of every video and grid of lib/logging.py, lib/figures.py and data/*.py.
 *
 * The split.  Everything up to the quantised coefficients is regular arithmetic and runs on the GPU, one launch per stage for a
 * whole batch of images of mixed sizes and samplings: vunet_jpeg_from_rgb and vunet_jpeg_fdct.  The entropy coder is a serial bit
 * walk and stays on the host: vunet_jpeg_encode_info, vunet_jpeg_quant_tables, vunet_jpeg_encode_bound and
 * vunet_jpeg_entropy_encode are pure host functions (no HIP call; they never initialise the GPU).
 *
 * Host.
 * vunet_jpeg_encode_info    the vunet_jpeg_info of an image: height, width >= 1 and <= 65535, ncomp 1 (hsamp = vsamp = 1) or 3 with
 *                           hsamp x vsamp of 1x1, 2x1 or 2x2 (4:4:4, 4:2:2, 4:2:0); restart = 0.
 * vunet_jpeg_quant_tables   qtab [2][64] uint16, natural order, table 0 for luma and 1 for chroma: the Annex K tables under libjpeg's
 *                           jpeg_quality_scaling (quality clamped to 1 .. 100; scale = 5000 / q below 50, else 200 - 2 q), each entry
 *                           clamp((base * scale + 50) / 100, 1, 255).
 * vunet_jpeg_encode_bound   *bytes = a size no stream of this info exceeds (1024 + 416 per block: every coefficient at its longest
 *                           code and every byte stuffed).
 * vunet_jpeg_entropy_encode coef in the decoder's layout (int16 [component][block row][block column][64], natural order, MCU-padded)
 *                           and qtab [ncomp][64] (entries 1 .. 255; component 2's table must equal component 1's) -> the whole
 *                           stream in out[0 .. *len): SOI; APP0 "JFIF" 1.01, no density unit, 1:1; one DQT per table (zigzag order);
 *                           SOF0 (component ids 1, 2, 3; sampling hsamp << 4 | vsamp, 0x11, 0x11; tables 0, 1, 1); the Annex K
 *                           Huffman tables, one DHT each, DC0 AC0 DC1 AC1 (one component: DC0 AC0 and one DQT); SOS; the interleaved
 *                           scan (MCUs left to right, top to bottom; per MCU the blocks component by component, row-major; DC as a
 *                           difference per component; AC as zero runs with ZRL and EOB; a zero byte stuffed after every 0xFF; the
 *                           last byte padded with 1-bits); EOI.  Nothing is written at or beyond out + cap.  *len is always the
 *                           length of the whole stream: with VUNET_JPEG_ERR_CAPACITY it says what `cap` has to be.  A DC difference
 *                           of more than 11 bits or an AC term of more than 10 is VUNET_JPEG_ERR_RANGE (*len is then 0).
 *                           VUNET_ERR_ARG: a NULL pointer, cap < 0, an info that vunet_jpeg_encode_info would not give, a table
 *                           entry outside 1 .. 255.
 *
 * Device.  One vunet_jpeg_img row per image, as for the decoder: coef_off in int16 elements (a multiple of 64) into `coef`, q_off in
 * uint16 elements (a multiple of 8) into `qtab` ([ncomp][64] there), plane_off in bytes (a multiple of 16) into `planes`, block0 the
 * number of blocks of all earlier images, slot the image's index in the input stack; bw0 / bh0 / bw1 / bh1 exactly the info's.  The
 * caller hands both copies of the rows: `imgs_host` is checked against the buffer sizes before anything is launched (VUNET_ERR_ARG),
 * `imgs` is what the kernels read.  An image's planes lie one after the other at plane_off, component c as [bh_c * 8][bw_c * 8] bytes.
 *
 * vunet_jpeg_from_rgb  frames [Nslots][Hmax][Wmax][channels], channels 3 (every row ncomp 3) or 1 (every row ncomp 1, Y = the
 *                      sample) -> level-unshifted planes.  jccolor.c's tables, FIX(x) = (int)(x * 65536 + 0.5):
 *                        Y  = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16
 *                        Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16
 *                        Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
 *                      Down-sampling (jcsample.c): h2v2 (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, .. along the output
 *                      columns, h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1, ...  Padding: every full-resolution read is clamped
 *                      to the last column (the row is edge-replicated BEFORE it is down-sampled); vertically the full-resolution
 *                      rows are replicated only up to a multiple of vsamp, and the DOWN-SAMPLED last row, ceil(height / vsamp) - 1,
 *                      is replicated below that.  Luma is edge-replicated both ways.  Every byte of every plane is written.  One
 *                      thread per 4 x 2 pixels: 24 bytes in, its luma and its chroma samples out, no second pass.
 * vunet_jpeg_fdct      level shift - 128, jfdctint.c's jpeg_fdct_islow in 32-bit integers (CONST_BITS 13, PASS1_BITS 2; the row
 *                      pass first, its outputs 0 and 4 shifted left by 2 and the others descaled by 11; the column pass descales 0
 *                      and 4 by 2 and the others by 15) and the quantiser sign(c) * ((|c| + (d >> 1)) / d), d = 8 q, an exact
 *                      integer division.  One launch over all blocks of the batch: eight threads per block, one row then one
 *                      column each through LDS, 16-byte stores of coefficient rows.  DUMMY BLOCKS -- MCU padding beyond a
 *                      component's real extent wb = ceil(ceil(width * hs_c / hsamp) / 8) x hb (likewise) -- are not transformed:
 *                      their 63 AC terms are 0 and their DC is the DC of a real block, (hb - 1, min((bx / hs_c) * hs_c + hs_c - 1,
 *                      wb - 1)) for by >= hb, else (by, wb - 1) (jccoefct.c's chain in closed form; hs_c the component's blocks per
 *                      MCU row); the dummy's eight threads transform that block again and keep its DC.
 * Both: no allocation, no synchronisation, no atomics (recordable in a hipGraph).  1 <= N, Nslots, Hmax, Wmax <= 65535.
 */
#ifndef VUNET_JPEG_ENC_H
#define VUNET_JPEG_ENC_H
#include <stddef.h>
#include <stdint.h>

#include "vunet_jpeg.h"

#define VUNET_JPEG_ERR_CAPACITY (-120)   /* the stream is longer than the output buffer; nothing was written past it */
#define VUNET_JPEG_ERR_RANGE (-121)      /* a DC difference of more than 11 bits or an AC coefficient of more than 10 */

#ifdef __cplusplus
extern "C" {
#endif

int vunet_jpeg_encode_info(int32_t height, int32_t width, int32_t ncomp, int32_t hsamp, int32_t vsamp, vunet_jpeg_info* info);
int vunet_jpeg_quant_tables(int32_t quality, uint16_t* qtab);
int vunet_jpeg_encode_bound(const vunet_jpeg_info* info, int64_t* bytes);
int vunet_jpeg_entropy_encode(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab, uint8_t* out, int64_t cap,
                              int64_t* len);

int vunet_jpeg_from_rgb(const uint8_t* frames, int32_t Nslots, int32_t Hmax, int32_t Wmax, int32_t channels,
                        const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N, uint8_t* planes, int64_t planes_bytes,
                        void* stream);
int vunet_jpeg_fdct(const uint8_t* planes, int64_t planes_bytes, const uint16_t* qtab, int64_t qtab_count, const vunet_jpeg_img* imgs,
                    const vunet_jpeg_img* imgs_host, int32_t N, int16_t* coef, int64_t coef_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
