/*
 * cauchy_256_update.h -- patching the recovery blocks of already-encoded stripes.
 *
 * Not part of the reference API.  The code is linear, so when a few data blocks of a stripe
 * change its recovery blocks follow by
 *     recovery'[r] = recovery[r] ^ B(G[r][x]) (old_x ^ new_x)
 * (G the generator of cauchy_256_encode, B(c) the 8 x 8 bit matrix of the multiplication by c
 * over the block's 8 sub-blocks): one changed block moves 2 + 2 m blocks where a re-encode
 * moves k + m.  Device pointers, strides in bytes, `stream` and the return codes (0 ok, -1
 * invalid parameters, -2 no device, -3 HIP error) as in cauchy_256_batch.h; all work runs on
 * the GPU.
 *
 * Both calls return -1 with nothing done when k < 1, k > 255 (a column is one byte and 0xFF
 * is reserved), m < 1, block_bytes <= 0, stripes < 0, changes < 0 or > 255, a stride is
 * smaller than its blocks (old_stride, and new_stride when d_new is given, < changes *
 * block_bytes; recovery_stride < m * block_bytes), or m > 1 and (k + m > 256 or
 * block_bytes % 8 != 0); also for a NULL cols, old or recovery argument when there is work.
 * stripes == 0 or changes == 0: nothing to do, 0.  m == 1 (any block size) and k == 1: every
 * recovery block takes the plain XOR of the deltas.
 */
#ifndef LONGHAIR_AMD_CAUCHY_256_UPDATE_H
#define LONGHAIR_AMD_CAUCHY_256_UPDATE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Patch the recovery blocks of already-encoded stripes after `changes` data blocks per
 * stripe changed: recovery_r ^= sum_j B(G[r][col_j]) (old_j ^ new_j), exactly what
 * cauchy_256_encode_batch would write for the patched data.
 *   d_cols[s * changes + j]  data index of change j of stripe s; 0xFF = no change in this
 *                            entry (stripes may differ in how many blocks changed)
 *   change j of stripe s     d_old + s * old_stride + j * block_bytes, likewise d_new
 *   d_new == NULL            d_old holds the deltas (old ^ new) themselves
 *   d_status (optional)      one signed byte per stripe: 0 ok, -1 = some col is in [k, 0xFE];
 *                            such a stripe's recovery is left untouched
 * A column may repeat within a stripe; its deltas accumulate (linearity).  The recovery blocks
 * must not overlap d_old / d_new.  Asynchronous on `stream`; 0, -1, -2, -3 as the other batch
 * calls.  Never allocates while `stream` is being captured (returns -3 if it would have to). */
int cauchy_256_update_batch(int k, int m, int block_bytes, int stripes, int changes,
                            const unsigned char *d_cols,
                            const void *d_old, long long old_stride,
                            const void *d_new, long long new_stride,
                            void *d_recovery, long long recovery_stride,
                            signed char *d_status, void *stream);
/* The same over pointer tables: d_old_ptrs / d_new_ptrs [s * changes + j] (entries of 0xFF
 * columns are not read; d_new_ptrs NULL = deltas), d_recovery_ptrs [s * m + r]; any alignment. */
int cauchy_256_update_batch_ptrs(int k, int m, int block_bytes, int stripes, int changes,
                                 const unsigned char *d_cols,
                                 const void *const *d_old_ptrs, const void *const *d_new_ptrs,
                                 void *const *d_recovery_ptrs, signed char *d_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LONGHAIR_AMD_CAUCHY_256_UPDATE_H */
