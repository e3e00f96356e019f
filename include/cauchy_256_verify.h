/*
 * cauchy_256_verify.h -- scrubbing stored stripes: do the recovery blocks still belong to the data?
 *
 * Not part of the reference API.  Recovery row r of a stripe is intact exactly when its syndrome
 *     recovery_r ^ sum_j B(G[r][j]) data_j          (j over all k data blocks)
 * is zero (G the generator of cauchy_256_encode, B(c) the 8 x 8 bit matrix of the multiplication
 * by c over the block's 8 sub-blocks).  One kernel reads the k + m blocks of each stripe once and
 * writes 1 + m bytes per stripe; no scratch the size of the recovery blocks, no second pass to
 * compare.  Device pointers, strides in bytes, `stream` and the return codes (0 ok, -1 invalid
 * parameters, -2 no device, -3 HIP error) as in cauchy_256_batch.h; all work runs on the GPU.
 *
 * Both calls return -1 with nothing done when k < 1, m < 1, k > 256, m > 256, block_bytes <= 0,
 * stripes < 0, m > 1 and k > 1 and (k + m > 256 or block_bytes % 8 != 0), a stride is smaller
 * than its blocks (data_stride < k * block_bytes, recovery_stride < m * block_bytes), both
 * outputs are NULL, or the data or recovery argument is NULL when stripes > 0.  stripes == 0:
 * nothing to do, 0.  m == 1 or k == 1 (any block size): row r is intact iff recovery_r equals the
 * XOR of the data blocks (for k == 1, a copy of the data block).
 */
#ifndef LONGHAIR_AMD_CAUCHY_256_VERIFY_H
#define LONGHAIR_AMD_CAUCHY_256_VERIFY_H

#ifdef __cplusplus
extern "C" {
#endif

/* Check the m stored recovery blocks of every stripe against its stored data.
 *   data block j of stripe s      d_data + s * data_stride + j * block_bytes
 *   recovery block r of stripe s  d_recovery + s * recovery_stride + r * block_bytes
 *   d_status[s]                   0: every recovery block equals, byte for byte, what
 *                                 cauchy_256_encode_batch writes for the stored data; else 1
 *                                 (not -1: a verify has no per-stripe input that can be invalid)
 *   d_bad_rows[s * m + r]         1 when recovery row r of stripe s differs, else 0
 * Either output may be NULL, not both.  Exactly `stripes` bytes of d_status and stripes * m bytes
 * of d_bad_rows are written and nothing else; data and recovery are only read.  A flipped
 * recovery bit marks its own row; a flipped data bit marks every row (no generator entry is
 * zero).  Asynchronous on `stream`; 0, -1, -2, -3 as the other batch calls.  Never allocates
 * while `stream` is being captured: it returns -3 if the shape's generator is not on the device
 * yet or the zero page the outputs are cleared from is smaller than stripes * m bytes (an
 * uncaptured call of the same size first, or cauchy_256_batch_prepare_stream where stripes * m
 * <= block_bytes, provides both). */
int cauchy_256_verify_batch(int k, int m, int block_bytes, int stripes,
                            const void *d_data, long long data_stride,
                            const void *d_recovery, long long recovery_stride,
                            signed char *d_status, unsigned char *d_bad_rows, void *stream);
/* The same over pointer tables: d_data_ptrs [s * k + j], d_recovery_ptrs [s * m + r]; any
 * alignment. */
int cauchy_256_verify_batch_ptrs(int k, int m, int block_bytes, int stripes,
                                 const void *const *d_data_ptrs, const void *const *d_recovery_ptrs,
                                 signed char *d_status, unsigned char *d_bad_rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LONGHAIR_AMD_CAUCHY_256_VERIFY_H */
