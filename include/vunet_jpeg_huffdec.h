/*
 * vunet_jpeg_huffdec.h -- C ABI of the device entropy decoder of the baseline JPEG decoder: csrc/jpeg_sync.h (the walk, shared by
 * host and device), csrc/jpeg_entropy.h (the marker scan) and csrc/jpeg_huff_dec.hip (the kernels).  Encoded scans -> exactly the
 * `coef` that vunet_jpeg_entropy_decode writes (vunet_jpeg.h's layout), so vunet_jpeg_idct and vunet_jpeg_to_rgb run unchanged
 * behind it.  Part of libvunet_hip.so; additive entry points within ABI 12; conventions of vunet_jpeg_enc.h's vunet_jpeg_huff_*:
 * host and device copies of every descriptor row, the host copy checked against every buffer size before anything is launched
 * (VUNET_ERR_ARG otherwise), `stream` = hipStream_t as void*.
 *
 * The scheme (Weissenberger & Schmidt, "Accelerating JPEG decompression on GPUs"): Huffman codes self-synchronise, so a scan is cut
 * into subsequences of VUNET_JPEG_SUBSEQ_BYTES, one thread each; every thread walks its subsequence from a guessed parser state and
 * proposes the entry state of the next one, round after round, until no state changes.  Then the states are the true ones.
 *
 * vunet_jpeg_scan_segments  HOST only, no bit walk: the marker scan of one stream.  Finds the end of the entropy-coded data and
 *     splits it at RSTn markers: segs[i] = (byte begin, byte end, first MCU), offsets into `bytes`; one segment without restart
 *     intervals.  Writes the stream's quantisation tables (as vunet_jpeg_entropy_decode does) and its table row `tab`
 *     (VUNET_JPEG_HUFFDEC_TAB_BYTES: the decoding tables flattened, the component-to-table map, the MCU's shape).  Returns 0, a
 *     VUNET_JPEG_ERR_* of the header, VUNET_ERR_ARG (NULL, an info that is not the stream's, seg_cap below the expected count:
 *     ceil(MCUs / restart), or 1), or VUNET_JPEG_HUFFDEC_IRREGULAR -- not an error: a marker out of sequence, fill bytes, an FF at
 *     the end of the data, no EOI, a segment count that does not match `restart`, an empty segment, or more than two DC or two AC
 *     tables in use.  Such a stream goes to vunet_jpeg_entropy_decode, which decodes it or names its error.  Reads nothing past len.
 * vunet_jpeg_huffdec_rows   HOST only: the subsequence rows of one stream from its segments.  `byte_off`: where the stream's byte
 *     0 lies in the batch's `bytes` buffer (may be negative: only [segs[0].begin, segs[last].end) has to be there); `row0`: the index
 *     of rows[0] in the batch (a multiple of VUNET_JPEG_HUFFDEC_GROUP).  Rows are padded with PAD rows to a multiple of the group,
 *     so that a workgroup's subsequences belong to one image.  *nrows: rows written; VUNET_ERR_ARG if row_cap is too small.
 *
 * Device stages, each one launch (plus memsets), none waits for another workgroup inside a launch:
 * vunet_jpeg_huffdec_sync   `launches` Jacobi rounds, numbered first .. first + launches - 1 from 0.  Round L reads the exit states
 *     of round L - 1 and writes its own (two buffers in `state`, so the result does not depend on the dispatch order); inside a
 *     workgroup the rounds repeat in LDS until none of its states changes.  A thread whose entry state did not change does nothing.
 *     counters[L] (zeroed here) = exit states that changed in round L: zero means every state is final.  The caller reads the
 *     counters back every few launches; rounds <= workgroups of the longest image + 1 always suffice.
 * vunet_jpeg_huffdec_blocks per image an exclusive prefix sum of the blocks-begun counts, restarted at every segment: every
 *     subsequence's first block ordinal.  flags[n] (zeroed here) |= VUNET_JPEG_HUFFDEC_SHORT where a segment's total differs from
 *     its MCUs' blocks (the image's last segment may hold more: leftover data is tolerated there as on the host).
 * vunet_jpeg_huffdec_write  zeroes coef[0 .. coef_count), then every thread walks again from its true entry state and stores the AC
 *     terms and the DC differences.  flags[n] |= VUNET_JPEG_HUFFDEC_ERROR for what the host decoder would refuse.
 * vunet_jpeg_huffdec_dc     the running sum of the DC differences per component in scan order, reset at every restart interval,
 *     modular and truncated to int16 as on the host.
 * `rounds_final` of blocks / write: the number of sync rounds run so far (it names the buffer that holds the final states).
 *
 * state: uint32 [VUNET_JPEG_HUFFDEC_STATE_WORDS * nsub] (two exit-state buffers, the entry states walked from, the counts, the prefix sums and the ordinals).
 * A flagged image's coefficients are undefined: the caller decodes it with vunet_jpeg_entropy_decode.
 */
#ifndef VUNET_JPEG_HUFFDEC_H
#define VUNET_JPEG_HUFFDEC_H
#include <stddef.h>
#include <stdint.h>

#include "vunet_jpeg.h"

#define VUNET_JPEG_SUBSEQ_BYTES 128          /* bytes of a segment that one thread walks */
#define VUNET_JPEG_HUFFDEC_GROUP 256         /* threads of a workgroup: rows of one image come in multiples of it */
#define VUNET_JPEG_HUFFDEC_TAB_BYTES 5720    /* one image's table row (csrc/jpeg_sync.h's Tables) */
#define VUNET_JPEG_HUFFDEC_STATE_WORDS 9     /* uint32 words of `state` per subsequence row */
#define VUNET_JPEG_HUFFDEC_MAX_BYTES (1 << 28)   /* of one batch's `bytes`: bit positions are 32-bit */
#define VUNET_JPEG_HUFFDEC_IRREGULAR 1       /* vunet_jpeg_scan_segments: not a clean scan; decode it on the host */

#define VUNET_JPEG_SUBSEQ_FIRST 1            /* the first subsequence of its segment: its entry state is known */
#define VUNET_JPEG_SUBSEQ_LAST 2             /* the last subsequence of its segment */
#define VUNET_JPEG_SUBSEQ_TAIL 4             /* its segment is the image's last */
#define VUNET_JPEG_SUBSEQ_PAD 8              /* no subsequence: fills the workgroup */

#define VUNET_JPEG_HUFFDEC_SHORT 1           /* flags: a segment's blocks differ from its MCUs' */
#define VUNET_JPEG_HUFFDEC_ERROR 2           /* flags: a code in no table, an index past 63, a block cut short, bits left in front of RSTn */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vunet_jpeg_subseq {
  int32_t img;                       /* the image's row in imgs, tabs, spans and flags */
  int32_t seg_begin, seg_end;        /* the segment's bytes in `bytes` */
  int32_t begin, end;                /* the subsequence's: seg_begin <= begin < end <= seg_end, end - begin <= VUNET_JPEG_SUBSEQ_BYTES */
  int32_t first_block, seg_blocks;   /* the segment's block ordinals (scan order in the image): first MCU x blocks per MCU, and how many */
  int32_t seg_row;                   /* the batch index of the segment's first row */
  int32_t flags, reserved;
} vunet_jpeg_subseq;

int vunet_jpeg_scan_segments(const uint8_t* bytes, int64_t len, const vunet_jpeg_info* info, int64_t* segs, int64_t seg_cap,
                             int64_t* nseg, uint16_t* qtab, uint8_t* tab);
int vunet_jpeg_huffdec_rows(const int64_t* segs, int64_t nseg, const vunet_jpeg_info* info, int32_t img, int64_t byte_off, int64_t row0,
                            vunet_jpeg_subseq* rows, int64_t row_cap, int64_t* nrows);

/* spans: int32 [N][2] = (first row, row count) of every image; tabs: N table rows */
int vunet_jpeg_huffdec_sync(const uint8_t* bytes, int64_t bytes_count, const vunet_jpeg_subseq* rows, const vunet_jpeg_subseq* rows_host,
                            int64_t nsub, const uint8_t* tabs, const uint8_t* tabs_host, const vunet_jpeg_img* imgs_host, int32_t N,
                            uint32_t* state, int64_t state_count, uint32_t* counters, int64_t counters_count, int32_t first,
                            int32_t launches, void* stream);
int vunet_jpeg_huffdec_blocks(const vunet_jpeg_subseq* rows, const vunet_jpeg_subseq* rows_host, int64_t nsub, const int32_t* spans,
                              const int32_t* spans_host, const vunet_jpeg_img* imgs_host, int32_t N, uint32_t* state, int64_t state_count,
                              uint32_t* flags, int64_t flags_count, void* stream);
int vunet_jpeg_huffdec_write(const uint8_t* bytes, int64_t bytes_count, const vunet_jpeg_subseq* rows, const vunet_jpeg_subseq* rows_host,
                             int64_t nsub, const uint8_t* tabs, const uint8_t* tabs_host, const vunet_jpeg_img* imgs,
                             const vunet_jpeg_img* imgs_host, int32_t N, const uint32_t* state, int64_t state_count, int32_t rounds_final,
                             int16_t* coef, int64_t coef_count, uint32_t* flags, int64_t flags_count, void* stream);
int vunet_jpeg_huffdec_dc(const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, const uint8_t* tabs, const uint8_t* tabs_host,
                          int32_t N, int16_t* coef, int64_t coef_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
