/*
 * vunet_jpeg.h -- C ABI of the baseline JPEG decoder, csrc/jpeg_entropy.h (host) and csrc/jpeg.hip (device): encoded byte streams
 * -> the uint8 RGB stack [N][Hmax][Wmax][3] that vunet_image_input.h takes, bit for bit what libjpeg-turbo's default pipeline
 * (islow inverse DCT, "fancy" up-sampling, YCbCr -> RGB) and so Pillow's Image.open(..).convert("RGB") give.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned buffers, `stream` = hipStream_t as void*,
 * 0 or a negative code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root): the
 * cv2.imread of every img_%06d.jpg (data/base_dataset.py), frames that data/process.py wrote as baseline JPEGs.
 *
 * The split.  The entropy decode is a serial bit walk and stays on the host: vunet_jpeg_parse and vunet_jpeg_entropy_decode are
 * pure host functions (no HIP call; they never initialise the GPU) and read nothing past `len`.  Everything after it is regular
 * arithmetic on 8 x 8 blocks and runs on the GPU, one launch per stage for a whole batch of images of mixed sizes:
 * vunet_jpeg_idct and vunet_jpeg_to_rgb.
 *
 * Supported: baseline sequential (SOF0), 8-bit samples, 8-bit quantisation tables, 1 or 3 components, the first component sampled
 * 1x1, 2x1 or 2x2 against 1x1 chroma (4:4:4, 4:2:2, 4:2:0), one interleaved scan, restart intervals.  APPn, COM and other
 * segments with a length are skipped (EXIF orientation is ignored).  A one-component image is decoded as one block per MCU
 * whatever its sampling factors say, as the standard has it.
 *
 * Errors.  VUNET_JPEG_ERR_* below; -100 .. -109 say the stream is corrupt or truncated, -110 .. -119 that it is well-formed but
 * outside the supported subset.  VUNET_ERR_ARG: a NULL pointer, len < 0, or an info that is not the stream's.
 *
 * Coefficient layout.  Component c has bw_c x bh_c blocks, padded to whole MCUs: bw_0 = mcu_cols * hsamp, bh_0 = mcu_rows * vsamp,
 * bw_c = mcu_cols, bh_c = mcu_rows for chroma.  coef is int16 [component][block row][block column][64]: every block's 64
 * coefficients in natural (row-major) order, not yet multiplied by the quantisation table, the DC prediction undone; ncoef of
 * them in all, every one written.  qtab is uint16 [ncomp][64]: each component's table in natural order.
 *
 * Device stages.  One vunet_jpeg_img row per image tells both kernels where its data lies; the caller fills the rows on the host
 * and uploads them, and hands BOTH copies to the entry points: `imgs_host` is checked against the buffer sizes before anything is
 * launched (VUNET_ERR_ARG), `imgs` is what the kernels read.  Offsets: coef_off in int16 elements (a multiple of 64) into `coef`,
 * q_off in uint16 elements into `qtab`, plane_off in bytes (a multiple of 16) into `planes`, block0 the number of blocks of all
 * earlier images, slot the image's index in the output stack.  An image's planes lie one after the other at plane_off,
 * component c as [bh_c * 8][bw_c * 8] bytes.
 *
 * vunet_jpeg_idct    dequantise and jidctint.c's jpeg_idct_islow in 64-bit integers (CONST_BITS 13, PASS1_BITS 2; the column pass
 *                    descaled by 11, the row pass by 18), + 128, clamped to 0 .. 255.  One launch over all `nblocks` blocks of the
 *                    batch: eight threads per block, 16-byte coefficient loads, one column then one row each through LDS.
 * vunet_jpeg_to_rgb  up-sampling on the real down-sampled extent ceil(width / hsamp) x ceil(height / vsamp), edges replicated,
 *                    and the colour conversion, one thread per pixel, into out [Nslots][Hmax][Wmax][3] at the image's `slot`
 *                    (N <= Nslots: a caller may fill other slots by other means); bytes outside an image's height x width are
 *                    not written.  With cw the down-sampled width, i = x >> 1, s the sample row (h2v1) or
 *                    s = 3 near + far of two rows (h2v2; far = the row above for even y, below for odd y):
 *                      h2v1: even x (3 s[i] + s[i-1] + 1) >> 2, odd x (3 s[i] + s[i+1] + 2) >> 2, x = 0 and i = cw - 1 copy s[i];
 *                      h2v2: even x (3 s[i] + s[i-1] + 8) >> 4, odd x (3 s[i] + s[i+1] + 7) >> 4, x = 0 (4 s[i] + 8) >> 4,
 *                            odd x with i = cw - 1 (4 s[i] + 7) >> 4;
 *                      cw <= 2: libjpeg does not use these filters -- every chroma sample is repeated hsamp x vsamp times.
 *                    cb, cr centred at 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *                    B = Y + ((116130 cb + 32768) >> 16), arithmetic shifts, clamped.  One component: R = G = B = Y.
 * Both: no allocation, no synchronisation, no atomics (recordable in a hipGraph).  1 <= N, Hmax, Wmax <= 65535.
 */
#ifndef VUNET_JPEG_H
#define VUNET_JPEG_H
#include <stddef.h>
#include <stdint.h>

#define VUNET_JPEG_ERR_TRUNCATED (-100)   /* the stream ends inside a segment, a table or the scan, or before EOI */
#define VUNET_JPEG_ERR_MARKER (-101)      /* no SOI, a marker out of place, a malformed segment, a missing table */
#define VUNET_JPEG_ERR_HUFFMAN (-102)     /* a code that is in no table, or a coefficient index past 63 */
#define VUNET_JPEG_ERR_RESTART (-103)     /* a restart marker is missing or out of sequence */
#define VUNET_JPEG_ERR_SOF (-110)         /* progressive, extended, lossless or arithmetic-coded (any SOF but SOF0) */
#define VUNET_JPEG_ERR_PRECISION (-111)   /* 16-bit quantisation tables, or samples that are not 8-bit */
#define VUNET_JPEG_ERR_COMPONENTS (-112)  /* 4 components (CMYK / YCCK), an Adobe transform other than YCbCr, RGB components */
#define VUNET_JPEG_ERR_SAMPLING (-113)    /* sampling factors other than 1x1, 2x1, 2x2 luma against 1x1 chroma */
#define VUNET_JPEG_ERR_SCANS (-114)       /* more than one scan */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vunet_jpeg_info {
  int32_t height, width, ncomp, hsamp, vsamp;   /* hsamp, vsamp: of component 0 (1, 1 for one component) */
  int32_t mcu_cols, mcu_rows, restart;          /* restart: MCUs per restart interval, 0 = none */
  int32_t bw0, bh0, bw1, bh1;                   /* blocks per row / column of component 0 and of each chroma component (0 if none) */
  int32_t nblocks, ncoef;                       /* ncoef = 64 * nblocks */
} vunet_jpeg_info;

typedef struct vunet_jpeg_img {
  int64_t coef_off, plane_off;
  int32_t q_off, block0;
  int32_t height, width, ncomp, hsamp, vsamp, bw0, bh0, bw1, bh1;
  int32_t slot;   /* the image's index in the output stack */
} vunet_jpeg_img;

int vunet_jpeg_parse(const uint8_t* bytes, int64_t len, vunet_jpeg_info* info);
int vunet_jpeg_entropy_decode(const uint8_t* bytes, int64_t len, const vunet_jpeg_info* info, int16_t* coef, uint16_t* qtab);

int vunet_jpeg_idct(const int16_t* coef, int64_t coef_count, const uint16_t* qtab, int64_t qtab_count, const vunet_jpeg_img* imgs,
                    const vunet_jpeg_img* imgs_host, int32_t N, uint8_t* planes, int64_t planes_bytes, void* stream);
int vunet_jpeg_to_rgb(const uint8_t* planes, int64_t planes_bytes, const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host,
                      int32_t N, int32_t Nslots, int32_t Hmax, int32_t Wmax, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
