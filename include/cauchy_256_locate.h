/*
 * cauchy_256_locate.h -- after the scrub: which block of a bad stripe is the corrupt one?
 *
 * Not part of the reference API.  cauchy_256_verify_batch says that a stripe's recovery blocks no
 * longer belong to its data; a flipped data bit marks every row there, so the caller knows that
 * something is wrong and not what.  These calls end in a row number cauchy_256_reconstruct_batch
 * takes as it is.  Device pointers, strides in bytes, `stream` and the return codes (0 ok, -1
 * invalid parameters, -2 no device, -3 HIP error) as in cauchy_256_batch.h; all work runs on the GPU.
 *
 * The contract.  A stripe's stored word is its k data blocks followed by its m recovery blocks,
 * rows 0 .. k + m - 1 as everywhere else (row x < k: data block x; row k + r: recovery block r).
 *   d_status[s] = 0, d_rows[s] = 0xFF   every recovery block is what cauchy_256_encode_batch writes
 *                                       for the stored data (the status 0 of verify).
 *   d_status[s] = 1, d_rows[s] = x      the stripe is not clean, and replacing block x ALONE can make
 *                                       it clean: block x is corrupt, in any number of its bytes.
 *   d_status[s] = 2, d_rows[s] = 0xFF   the stripe is not clean and no single block explains it:
 *                                       more than one block is corrupt, or m == 1 (one parity shows
 *                                       that something is wrong and cannot attribute it).
 * 0xFF is "no row", as in the want_rows of cauchy_256_reconstruct_batch: d_rows, read as
 * [stripes][1], is a valid want_rows.
 *
 * For m >= 2 the row of status 1 is unique.  The code is MDS, so two different codewords differ in
 * at least m + 1 blocks.  If replacing block x alone and replacing block y != x alone both gave a
 * codeword, those two codewords would differ in at most the 2 blocks x and y, and 2 < m + 1.
 *
 * What follows from the definition:
 *   - one corrupt block (data or recovery, any bytes of it) is always located: status 1, its row;
 *   - c corrupt blocks, 2 <= c <= m - 1: always status 2, never a wrong row (a codeword within one
 *     block of the stored word would be within c + 1 <= m blocks of the original codeword);
 *   - c >= m corrupt blocks: whatever the definition gives.  That can be a single row, and a wrong
 *     one, when the damage happens to lie within one block of another codeword -- as for every MDS
 *     code beyond its distance; no decoder can tell.
 *
 * In terms of the syndromes s_r = recovery_r ^ sum_j B(G[r][j]) data_j of cauchy_256_verify.h (row 0
 * of G is all ones): status 0 iff every s_r is zero; recovery block r alone explains the stripe iff
 * s_r is the only non-zero syndrome; data block x alone iff s_r == B(G[r][x]) s_0 for every r.  No
 * entry of G is zero, so a corrupt data block makes every row bad wherever it makes one bad.  Hence
 * (m >= 2) exactly one bad row r is recovery block r with no further arithmetic (a data block would
 * have made all m >= 2 rows bad, and another recovery row is not bad), and a number of bad rows
 * from 2 to m - 1 is status 2; only a stripe whose m rows are all bad is searched for its column.
 *
 * Both calls return -1 with nothing done when k < 1, m < 1, k > 256, m > 256, block_bytes <= 0,
 * stripes < 0, m > 1 and k > 1 and block_bytes % 8 != 0, m >= 2 and k + m > 255 (row 255 would
 * collide with "no row"), a stride is smaller than its blocks (data_stride < k * block_bytes,
 * recovery_stride < m * block_bytes), either output is NULL, or the data or recovery argument is
 * NULL when stripes > 0.  stripes == 0: nothing to do, 0.  m == 1 (any block size, k <= 256):
 * status 0 or 2 only.  k == 1, m >= 2 (any block size): every coefficient is 1, the recovery blocks
 * are copies of the data block.
 */
#ifndef LONGHAIR_AMD_CAUCHY_256_LOCATE_H
#define LONGHAIR_AMD_CAUCHY_256_LOCATE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Scrub every stripe and name the one block that explains a bad one.
 *   data block j of stripe s      d_data + s * data_stride + j * block_bytes
 *   recovery block r of stripe s  d_recovery + s * recovery_stride + r * block_bytes
 *   d_status[s], d_rows[s]        as above; both outputs are required
 * Exactly `stripes` bytes of d_status and of d_rows are written and nothing else; data and recovery
 * are only read.  Asynchronous on `stream`; 0, -1, -2, -3 as the other batch calls.
 * cauchy_256_last_launch reports, in order,
 *     lh_verify_kernel; lh_locate_kernel; lh_locate_finish_kernel
 * (the first two with the suffix "(pointer table)" from cauchy_256_locate_batch_ptrs), and for
 * m == 1, where there is nothing to search, lh_verify_kernel; lh_locate_finish_kernel.
 * Never allocates while `stream` is being captured: it returns -3, with nothing enqueued, if the
 * shape's generator is not on the device yet, or the zero page or the stream's workspace would
 * have to grow.  An uncaptured call of the same (k, m, block_bytes, stripes) on that stream first
 * provides all three. */
int cauchy_256_locate_batch(int k, int m, int block_bytes, int stripes,
                            const void *d_data, long long data_stride,
                            const void *d_recovery, long long recovery_stride,
                            signed char *d_status, unsigned char *d_rows, void *stream);
/* The same over pointer tables: d_data_ptrs [s * k + j], d_recovery_ptrs [s * m + r]; any
 * alignment. */
int cauchy_256_locate_batch_ptrs(int k, int m, int block_bytes, int stripes,
                                 const void *const *d_data_ptrs, const void *const *d_recovery_ptrs,
                                 signed char *d_status, unsigned char *d_rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LONGHAIR_AMD_CAUCHY_256_LOCATE_H */
