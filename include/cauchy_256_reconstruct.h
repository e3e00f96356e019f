/*
 * cauchy_256_reconstruct.h -- repair: rebuild chosen rows of a stripe's codeword out of place.
 *
 * Not part of the reference API.  A stripe's codeword has k + m rows: rows 0 .. k - 1 are the data
 * blocks, row k + r is recovery block r of cauchy_256_encode.  From any k of them (the survivors,
 * in the reference's Block[] order with their Block.row bytes) every other row is a GF(256)-linear
 * combination
 *     out_j = sum_slot B(C[j][slot]) block_slot      (slot over the k survivors)
 * (B(c) the 8 x 8 bit matrix of the multiplication by c over the block's 8 sub-blocks).  The call
 * reads the k survivors of each stripe once per tile of four wanted rows and writes only the wanted
 * rows, to a place of the caller's: unlike cauchy_256_decode_batch it leaves the survivors and their
 * rows as they are, and it rebuilds recovery rows as well as data rows.  Device pointers, strides
 * in bytes, `stream` and the return codes (0 ok, -1 invalid parameters, -2 no device, -3 HIP
 * error) as in cauchy_256_batch.h; all work runs on the GPU.
 *
 * Both calls return -1 with nothing done when k < 1, m < 1, k > 256, m > 256, block_bytes <= 0,
 * stripes < 0, want < 1, want * k > 2^31 - 1, k + m > 255 (a row is one byte and 0xFF is reserved), k > 1 and m > 1 and
 * block_bytes % 8 != 0, a stride is smaller than its blocks (blocks_stride < k * block_bytes,
 * out_stride < want * block_bytes), or the blocks, rows, want-rows or out argument is NULL when
 * stripes > 0.  stripes == 0: nothing to do, 0.  m == 1 or k == 1 take any block size: for m == 1
 * the absent row is the XOR of the k survivors, for k == 1 every row is a copy of the one survivor.
 */
#ifndef LONGHAIR_AMD_CAUCHY_256_RECONSTRUCT_H
#define LONGHAIR_AMD_CAUCHY_256_RECONSTRUCT_H

#ifdef __cplusplus
extern "C" {
#endif

/* Rebuild `want` rows of every stripe from its k survivors.
 *   survivor slot i of stripe s   d_blocks + s * blocks_stride + i * block_bytes
 *   d_rows[s * k + i]             the row (Block.row) of that slot, in [0, k + m), no row twice
 *   d_want_rows[s * want + j]     the row wanted as out block j: in [0, k + m), or 0xFF for
 *                                 "nothing wanted here"; a row may repeat, and a row that is
 *                                 among the survivors is copied
 *   out block j of stripe s       d_out + s * out_stride + j * block_bytes
 *   d_status[s]                   0, or -1: a survivor row is >= k + m or repeats, or a wanted row
 *                                 lies in [k + m, 0xFE] (for every m, m == 1 included)
 * Out block j receives row w = d_want_rows[s * want + j] of the stripe's codeword: data block w
 * for w < k, else byte for byte what cauchy_256_encode_batch writes as recovery row w - k for the
 * stripe's data.  The out block of a 0xFF entry is not written, and a stripe with status -1
 * writes none of its out blocks.  d_status may be NULL.  d_blocks, d_rows and d_want_rows are
 * only read; the only bytes written are the wanted out blocks and `stripes` status bytes.  The out
 * blocks must not overlap the survivors, the rows or the wanted rows (not checked).
 * Asynchronous on `stream`; 0, -1, -2, -3 as the other batch calls.  Never allocates while
 * `stream` is being captured: it returns -3 then unless an uncaptured call with the same
 * (k, m, block_bytes, stripes, want) went first on that stream. */
int cauchy_256_reconstruct_batch(int k, int m, int block_bytes, int stripes,
                                 const void *d_blocks, long long blocks_stride,
                                 const unsigned char *d_rows,
                                 int want, const unsigned char *d_want_rows,
                                 void *d_out, long long out_stride,
                                 signed char *d_status, void *stream);
/* The same over pointer tables: survivor slot i of stripe s at d_block_ptrs[s * k + i], out block
 * j at d_out_ptrs[s * want + j]; any alignment.  The out pointer of a 0xFF entry is not read. */
int cauchy_256_reconstruct_batch_ptrs(int k, int m, int block_bytes, int stripes,
                                      const void *const *d_block_ptrs, const unsigned char *d_rows,
                                      int want, const unsigned char *d_want_rows,
                                      void *const *d_out_ptrs,
                                      signed char *d_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LONGHAIR_AMD_CAUCHY_256_RECONSTRUCT_H */
