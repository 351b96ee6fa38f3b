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
 * walk on the host by default: vunet_jpeg_encode_info, vunet_jpeg_quant_tables, vunet_jpeg_encode_bound, vunet_jpeg_entropy_encode
 * and the optimised-table functions are pure host functions (no HIP call; they never initialise the GPU).  The same coder as
 * launches per stage, for callers that want only the streams' bytes to cross to the host: vunet_jpeg_huff_*, at the end.
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
 * Optimised Huffman tables (libjpeg's optimize_coding, Pillow's optimize=True): a pass over the coefficients that counts, the table
 * builder, and the stream writer with the caller's tables.  Tables travel as two plain arrays in DHT order DC0, AC0, DC1, AC1:
 * counts uint8 [4][16] (codes per length 1 .. 16) and symbols uint8 [4][256] (the first sum(counts) of a row count); an image of
 * one component reads the first two rows of each.
 * vunet_jpeg_symbol_histogram      hist uint32 [4][256], same order (one component: rows 2 and 3 stay 0): how often the coder emits
 *                                  each symbol -- per block in scan order the bit length of its DC difference; one 0xF0 per 16
 *                                  zeros of a run, (run << 4) | size per non-zero AC term, 0x00 where the block does not end at
 *                                  position 63.  VUNET_JPEG_ERR_RANGE as the coder gives it.
 * vunet_jpeg_optimal_table         freq uint32 [256] -> counts [16], symbols [256] (the first *nsym are set): jchuff.c's
 *                                  jpeg_gen_optimal_table.  A reserved symbol 256 of frequency 1 keeps every code from being all
 *                                  ones; the two smallest non-zero frequencies are merged, ties going to the larger index, until
 *                                  one is left; lengths above 16 are shortened pairwise from 32 down (a code longer than 32 before
 *                                  that is VUNET_ERR_ARG, libjpeg's own limit); the reserved code leaves the longest length in
 *                                  use; symbols are ordered by length, then by value.
 * vunet_jpeg_optimal_tables        a batch at once, what stands between the device coder's histogram and its other launches: hist
 *                                  [N][4][256] -> counts [N][4][16], symbols [N][4][256], codes [N][4][256] (vunet_jpeg_code_words'
 *                                  form); the first ntab (2 or 4) tables of every image are built, the others are empty.  Returns
 *                                  the first code that is not VUNET_OK with *failed the image's index (-1: none).
 * vunet_jpeg_entropy_encode_tables vunet_jpeg_entropy_encode with the DHT segments and codes of `counts` / `symbols`; both NULL:
 *                                  Annex K's, byte for byte vunet_jpeg_entropy_encode.  VUNET_ERR_ARG besides: only one of the two
 *                                  NULL, counts that are no prefix code's (more codes of a length than fit) or sum to more than
 *                                  256, a symbol listed twice, a symbol the coefficients need and its table lacks (*len is 0).
 * vunet_jpeg_write_header          SOI .. SOS of that stream alone into out[0 .. *len), same capacity rule: what the host puts in
 *                                  front of scan bytes coded on the device.
 * vunet_jpeg_code_words            codes uint32 [4][256], len << 16 | code, 0 = no such symbol: the tables as the device coder
 *                                  reads them (both NULL: Annex K's).  All four rows are read and written.
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
 *
 * The entropy coder on the device (csrc/jpeg_huff.hip): the coefficients vunet_jpeg_fdct left, under the same rows, -> the scans'
 * bytes, stuffed, the batch's images end to end; the host writes vunet_jpeg_write_header in front of each and FF D9 behind.  One
 * thread per 8 x 8 block walks it as the host coder does; bit offsets come from prefix sums; every stage is its own launch and
 * nothing inside a launch waits for another workgroup.  Integer atomic add (histogram) and OR (words two blocks share), both on
 * memory the entry point zeroes first: no result depends on the dispatch order.  `codes` uint32 [code_rows][4][256] as
 * vunet_jpeg_code_words gives them; tab_row[n] is image n's row (one row of Annex K's serves a whole batch).  All device pointers
 * 16-byte aligned.  Every `*_host` array is the host copy of the device array before it and is what is checked before anything is
 * launched (VUNET_ERR_ARG: a row outside the coefficients, a table row >= code_rows, a capacity too small).
 * vunet_jpeg_huff_count    hist uint32 [N][4][256] (hist_count >= 1024 N): vunet_jpeg_symbol_histogram of every image.  Blocks out
 *                          of range are counted up to the offending term; vunet_jpeg_huff_lengths reports them.
 * vunet_jpeg_huff_lengths  bits [bits_count >= the batch's blocks]: at block0 + s the bit offset of the image's block s in scan
 *                          order (an exclusive prefix sum per image: two launches).  totals [totals_count >= round_up(N, 4) +
 *                          round_up(2 N, 4)]: totals[n] the image's bits; from totals[round_up(N, 4)] on, two status words per
 *                          image, non-zero where a coefficient is out of baseline's range (VUNET_JPEG_ERR_RANGE on the host
 *                          route) and where a needed symbol has no code.  Offsets are 32-bit: the caller keeps images whose
 *                          blocks x 1664 bits do not fit away.
 * vunet_jpeg_huff_pack     spans int64 [N][2]: (byte offset of the image's unstuffed scan in `raw`, its bits as totals[n] said).
 *                          The images lie one after the other, each from a multiple of 1024 bytes; raw_bytes covers them.  The
 *                          last byte of a scan is padded with 1-bits.
 * vunet_jpeg_huff_stuff    -> out[img_start[n] .. img_start[n + 1]): image n's scan with a zero byte after every 0xFF; img_start
 *                          uint32 [N + 1].  chunk_off: scratch, one word per 1024 bytes of `raw` in use; out_cap >= two bytes per
 *                          unstuffed byte (and < 2^32).  Three launches.
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
int vunet_jpeg_symbol_histogram(const int16_t* coef, const vunet_jpeg_info* info, uint32_t* hist);
int vunet_jpeg_optimal_table(const uint32_t* freq, uint8_t* counts, uint8_t* symbols, int32_t* nsym);
int vunet_jpeg_optimal_tables(const uint32_t* hist, int32_t N, int32_t ntab, uint8_t* counts, uint8_t* symbols, uint32_t* codes,
                              int32_t* failed);
int vunet_jpeg_entropy_encode_tables(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab, const uint8_t* counts,
                                     const uint8_t* symbols, uint8_t* out, int64_t cap, int64_t* len);
int vunet_jpeg_write_header(const vunet_jpeg_info* info, const uint16_t* qtab, const uint8_t* counts, const uint8_t* symbols,
                            uint8_t* out, int64_t cap, int64_t* len);
int vunet_jpeg_code_words(const uint8_t* counts, const uint8_t* symbols, uint32_t* codes);

int vunet_jpeg_from_rgb(const uint8_t* frames, int32_t Nslots, int32_t Hmax, int32_t Wmax, int32_t channels,
                        const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N, uint8_t* planes, int64_t planes_bytes,
                        void* stream);
int vunet_jpeg_fdct(const uint8_t* planes, int64_t planes_bytes, const uint16_t* qtab, int64_t qtab_count, const vunet_jpeg_img* imgs,
                    const vunet_jpeg_img* imgs_host, int32_t N, int16_t* coef, int64_t coef_count, void* stream);

int vunet_jpeg_huff_count(const int16_t* coef, int64_t coef_count, const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host,
                          int32_t N, uint32_t* hist, int64_t hist_count, void* stream);
int vunet_jpeg_huff_lengths(const int16_t* coef, int64_t coef_count, const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host,
                            int32_t N, const uint32_t* codes, int64_t code_rows, const int32_t* tab_row, const int32_t* tab_row_host,
                            uint32_t* bits, int64_t bits_count, uint32_t* totals, int64_t totals_count, void* stream);
int vunet_jpeg_huff_pack(const int16_t* coef, int64_t coef_count, const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host,
                         int32_t N, const uint32_t* codes, int64_t code_rows, const int32_t* tab_row, const int32_t* tab_row_host,
                         const uint32_t* bitoff, int64_t bits_count, const int64_t* spans, const int64_t* spans_host, uint8_t* raw,
                         int64_t raw_bytes, void* stream);
int vunet_jpeg_huff_stuff(const uint8_t* raw, int64_t raw_bytes, const vunet_jpeg_img* imgs_host, const int64_t* spans,
                          const int64_t* spans_host, int32_t N, uint32_t* chunk_off, int64_t chunk_count, uint8_t* out,
                          int64_t out_cap, uint32_t* img_start, void* stream);

#ifdef __cplusplus
}
#endif
#endif
