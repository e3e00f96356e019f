// kernels.hpp -- argument blocks and launchers shared by the host code and kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lh {

constexpr int kGenericTileOut = 4;  // outputs per lane in lh_apply_generic_kernel

// Per-stripe decode plan record (written by lh_plan_kernel):
//   [0] e (erasures to recover)   [1] status (int8)   [2..15] reserved
//   [16]                     out_slot[e_max]   slot receiving the i-th recovered original
//   [16+e_max]               src_slot[k]       slot of original x, 0xFF if erased
//   [16+e_max+k]             rec_slot[m]       slot of recovery row r, 0xFF if absent
//   [16+e_max+k+m]           coef[e_max][m]    A^-1 over recovery rows (0 = unused row)
//   [16+e_max+k+m+e_max*m]   w[e_max][k]       per-slot coefficients of the recovered
//                                              originals (single-pass form)
struct PlanView {
    uint8_t *p;
    int k, m, e_max;
    __host__ __device__ PlanView(uint8_t *p_, int k_, int m_, int e_max_) : p(p_), k(k_), m(m_), e_max(e_max_) {}
    __host__ __device__ PlanView(const uint8_t *p_, int k_, int m_, int e_max_)
        : p(const_cast<uint8_t *>(p_)), k(k_), m(m_), e_max(e_max_) {}
    __host__ __device__ static long long bytes(int k, int m, int e_max) {
        long long n = 16 + e_max + k + m + (long long)e_max * m + (long long)e_max * k;
        return (n + 15) / 16 * 16;
    }
    __host__ __device__ int e() const { return p[0]; }
    __host__ __device__ int out_slot(int i) const { return p[16 + i]; }
    __host__ __device__ void set_out_slot(int i, uint8_t v) { p[16 + i] = v; }
    __host__ __device__ int src_slot(int x) const { return p[16 + e_max + x]; }
    __host__ __device__ void set_src_slot(int x, uint8_t v) { p[16 + e_max + x] = v; }
    __host__ __device__ int rec_slot(int r) const { return p[16 + e_max + k + r]; }
    __host__ __device__ void set_rec_slot(int r, uint8_t v) { p[16 + e_max + k + r] = v; }
    __host__ __device__ uint8_t *coef_ptr() const { return p + 16 + e_max + k + m; }
    __host__ __device__ void set_coef(int i, int r, uint8_t v) { coef_ptr()[i * m + r] = v; }
    __host__ __device__ uint8_t *w_ptr() const { return p + 16 + e_max + k + m + e_max * m; }
    __host__ __device__ void set_w(int i, int slot, uint8_t v) { w_ptr()[i * k + slot] = v; }
    __host__ __device__ static long long w_offset(int k, int m, int e_max) {
        return 16 + e_max + k + m + (long long)e_max * m;
    }
};

struct ApplyArgs {
    const uint8_t *in;            // stripe s, input j: in + s*in_stride + j*bytes
    long long in_stride;
    uint8_t *out;                 // stripe s, output i: out + s*out_stride + i*bytes
    long long out_stride;
    const uint8_t *coef;          // coef[s*coef_stride + i*n_in + j]  (stride 0: shared)
    long long coef_stride;
    const uint8_t *nout_per_stripe;  // optional: valid outputs of stripe s at [s*nout_stride]
    long long nout_stride;
    int n_in, n_out, bytes, sub, stripes, nch;
};

// Generic apply through the phase-B jump table (lh_apply_jump_kernel): out_i = sum_j
// B(W[i][j]) in_j for any coefficient matrix, at the nibble-table cost (22 XORs per input
// column and lane, then one XOR3 per output sub-row) instead of lh_apply_generic_kernel's 64
// masked XORs per output and column.  Dword lanes (sub >= 4), up to 8 outputs per wave and
// ceil(n_out / 8) waves per workgroup (at most 16; more outputs take further rounds).
//  per_stripe = 0 (encode: one coefficient matrix for every stripe): lanes run flat over
//    (stripe, dword chunk), so small blocks fill whole waves;
//  per_stripe = 1 (decode: the plan's per-stripe W over the k slots): a workgroup codes one
//    stripe's 64-lane chunk; the outputs go in place to the plan's output slots (count e =
//    plan[0]) after a workgroup barrier, so no wave still reads a slot another overwrites.
struct JumpApplyArgs {
    const uint8_t *in;            // stripe s, input j: in + s*in_stride + j*bytes
    long long in_stride;
    uint8_t *out;                 // per_stripe 0: stripe s, output i at out + s*out_stride + i*bytes
    long long out_stride;
    const uint8_t *coef;          // W[i][j] at coef + s*coef_stride + i*n_in + j (stride 0: shared)
    long long coef_stride;
    const uint8_t *plan;          // per_stripe 1: e and the output slots (PlanView), in place
    long long plan_stride;
    int n_in, n_out, bytes, sub, nch, stripes;
    int per_stripe, wps;          // wps: workgroups per stripe (per_stripe 1) = ceil(nch / 64)
    uint8_t *const *in_ptrs;      // pointer tables (cauchy_256_*_batch_ptrs), else NULL: input j of
    uint8_t *const *out_ptrs;     // stripe s at in_ptrs[s*in_n + j], output i (or, per_stripe 1, the
    int in_n, out_n;              // plan's slot i) at out_ptrs[s*out_n + i] (in, out, strides unused)
    int *order;                   // per_stripe 1: scratch of `stripes` ints, the stripes by e, largest
                                  // first (written by launch_apply_jump), or NULL: stripe order
    int dw;                       // bytes per lane per sub-block / 4: 1 (nch = ceil(sub / 4)) or
                                  // 2 (nch = ceil(sub / 8), the two-dword table, sub >= 8)
    int jump_fallback;            // dw 1: the in-asm table (set by launch_apply_jump from
                                  // LONGHAIR_AMD_INV_FALLBACK, tests), as a straddling table would
};

struct XorArgs {
    const uint8_t *in;            // stripe s, input j: in + s*in_stride + j*bytes
    long long in_stride;
    uint8_t *out;                 // stripe s: out + s*out_stride (+ out_slot*bytes with plan)
    long long out_stride;
    const uint8_t *plan;          // optional (decode m == 1): output slot from the plan
    long long plan_stride;
    int k, m, e_max;
    int n_in, n_rep, bytes, stripes, nch;
};

struct ScatterArgs {
    const uint8_t *work;
    long long work_stride;
    uint8_t *blocks;
    long long blocks_stride;
    const uint8_t *plan;
    long long plan_stride;
    int k, m, e_max, bytes, stripes;
};

struct PlanArgs {
    uint8_t *rows;                // stripes x k, rewritten
    int8_t *status;               // optional, stripes
    uint8_t *plan;
    long long plan_stride;
    const uint8_t *G;             // m x k generator (row 0 = ones)
    const uint8_t *points;        // Cauchy points X'[k], Y'[m] of G, or null (no closed form)
    const uint8_t *gf_exp;        // 512
    const int16_t *gf_log;        // 256
    int k, m, e_max, stripes;
    int want_w;                   // emit the single-pass coefficients (generic path)
};

struct FrameArgs {
    const uint8_t *data;          // frame: data blocks (stripe stride data_stride)
    long long data_stride;
    const uint8_t *rec;           // frame: recovery blocks
    long long rec_stride;
    uint8_t *packets;             // [stripe][packet i][row byte + block]
    long long packet_stride;
    uint8_t *blocks;              // unframe: decode slots
    long long blocks_stride;
    uint8_t *rows;                // unframe: Block.row bytes, stripes x k
    int k, m, bytes, stripes, npk, unframe;
};

// Phase B of the large-m decode (after the windowed phase-A kernel replaced every present
// recovery block R_r by V_r in place): D_{E_i} = sum_r B(coef[i][r]) V_r into out_slot(i).
struct InverseArgs {
    uint8_t *blocks;              // stripe s, slot j: blocks + s*stride + j*bytes
    long long stride;
    const uint8_t *plan;          // PlanView records
    long long plan_stride;
    int k, m, e_max, bytes, stripes;
    int pack;                     // lh_inverse_gt_kernel: 8 consecutive outputs per wave
    int jump_fallback;            // lh_inverse_gt_kernel: take the in-asm table (tests)
    int chunks_per_wg;            // lh_inverse_gt_kernel: consecutive 2 KiB chunks per workgroup (>= 1)
    uint8_t *const *ptrs;         // pointer-table batches: slot j of stripe s at ptrs[s*k + j]
                                  // (blocks and stride unused), else NULL
    int *order;                   // scratch of `stripes` ints: the stripes by e, largest first
                                  // (written by launch_inverse; NULL: launch order = stripe order)
};

hipError_t launch_inverse(const InverseArgs &a, hipStream_t st);

// Pinned-host decode pipeline: write every slot that held a recovery block before the
// decode (rows_orig >= k: the only slots decode writes) straight into the caller's pinned
// host buffer (device-mapped pointer), so only the recovered blocks cross PCIe back.
struct WritebackArgs {
    const uint8_t *blocks;        // device chunk: stripe s, slot j at blocks + s*stride + j*bytes
    long long stride;
    uint8_t *host;                // device-mapped pinned host buffer of the chunk
    long long host_stride;
    const uint8_t *rows_orig;     // the chunk's Block.row bytes before the decode, stripes x k
    int k, bytes, stripes;
};

// Pointer-table batches (cauchy_256_*_batch_ptrs) on the paths without a pointer form:
// block j of stripe s lives at ptrs[s * n + j].  gather: into a contiguous chunk (stripe s,
// block j at chunk + s * stride + j * bytes); scatter: back from it, only the blocks the
// decode may have changed when sel is set (sel = the chunk's rows before the decode):
// the slots with sel[s * n + j] >= sel_min (k, m > 1: the slots that held recovery rows), or
// with m1 the one output slot of cauchy_decode_m1 (the last slot with a row >= k, else slot 0,
// cauchy_256.cpp:487-535); and never a stripe whose status (when given) is non-zero (invalid
// rows: the decode left it untouched).  Only the first ncopy blocks of each stripe are copied.
struct PtrCopyArgs {
    uint8_t *const *ptrs;         // [stripe][n]
    uint8_t *chunk;
    long long stride;
    const uint8_t *sel;           // [stripe][n] or NULL
    const int8_t *status;         // [stripe] or NULL (scatter)
    int sel_min, m1;
    int n, ncopy, bytes, stripes, scatter;
};

// Recovery patch (cauchy_256_update_batch, lh_update_kernel): recovery_r ^= sum_j
// B(G[r][cols[j]]) delta_j over the stripe's `changes` entries, delta_j = old_j ^ new_j (or
// old_j alone without `new`).  An entry with column 0xFF is skipped; a column in [k, 0xFE]
// invalidates the stripe (status -1, nothing written).
struct UpdateArgs {
    const uint8_t *cols;          // cols[s*changes + j]
    const uint8_t *old_blocks;    // change j of stripe s: old_blocks + s*old_stride + j*bytes
    long long old_stride;
    const uint8_t *new_blocks;    // likewise, or NULL: old_blocks holds the deltas
    long long new_stride;
    uint8_t *rec;                 // recovery block r of stripe s: rec + s*rec_stride + r*bytes
    long long rec_stride;
    // table != 0: pointer tables (cauchy_256_update_batch_ptrs; the strided fields unused):
    // change j of stripe s at old_ptrs[s*changes + j] (new_ptrs likewise, or NULL), recovery
    // block r at rec_ptrs[s*m + r]
    int table;
    const uint8_t *const *old_ptrs;
    const uint8_t *const *new_ptrs;
    uint8_t *const *rec_ptrs;
    int8_t *status;               // optional, stripes
    const uint8_t *G;             // m x k generator (row 0 = ones); unused when `flat`
    int k, m, changes, bytes, stripes;
    int flat;                     // m == 1 or k == 1: every coefficient is 1, lanes over the block's bytes
    int span, nch;                // set by launch_update: bytes a lane column runs over (bytes / 8 of each
                                  // sub-block, or the whole block when flat) and lanes per stripe
};

// Which lane owns which bytes in the scrub, locate and repair kernels: derived by the launcher
// (lane_grid in kernels.hip, which sets all but `flat`), read by the kernel (lh_chunk_of,
// lh_lane_at).  The lanes are lh_update_kernel's, the tiles lh_verify_kernel's; see there.
struct LaneGrid {
    int flat;                     // m == 1 or k == 1 (set by the caller): every coefficient is 0 or 1,
                                  // 16-byte lanes over the block's bytes, any block size
    int span;                     // bytes a lane column runs over: bytes / 8 of each sub-block, or the
                                  // whole block when flat
    int nch;                      // lanes per stripe
    int tiles;                    // row tiles on the grid (1: none)
};

// Recovery scrub (cauchy_256_verify_batch, lh_verify_kernel): row r of stripe s is bad iff
// recovery_r ^ sum_j B(G[r][j]) data_j != 0 over all k data blocks.  Reads only; stores the byte 1
// to bad_rows[s*m + r] and status[s] of a bad row (launch_verify zeroes both outputs first).
struct VerifyArgs {
    const uint8_t *data;          // data block j of stripe s: data + s*data_stride + j*bytes
    long long data_stride;
    const uint8_t *rec;           // recovery block r of stripe s: rec + s*rec_stride + r*bytes
    long long rec_stride;
    // table != 0: pointer tables (cauchy_256_verify_batch_ptrs; the strided fields unused): data
    // block j of stripe s at data_ptrs[s*k + j], recovery block r at rec_ptrs[s*m + r]
    int table;
    const uint8_t *const *data_ptrs;
    const uint8_t *const *rec_ptrs;
    int8_t *status;               // optional, stripes (at least one of the two outputs is given)
    uint8_t *bad_rows;            // optional, stripes x m
    const uint8_t *zero;          // device zeros, at least stripes * m bytes (stripes without bad_rows)
    const uint8_t *G;             // m x k generator (row 0 = ones); unused when `flat`
    int k, m, bytes, stripes;
    LaneGrid grid;                // tiles: the row tiles
};

// Locate (cauchy_256_locate_batch): the scrub of `v` into the workspace's bad_rows (v.status NULL,
// v.bad_rows [stripes][m]), then lh_locate_kernel over the same lanes for the stripes whose m rows
// are all bad -- each lane with a non-zero syndrome votes for the one data column that explains it,
// or for "none", into votes[s] -- then lh_locate_finish_kernel, a thread per stripe, which writes
// the two output bytes from the stripe's bad rows and its vote.
// votes[s]: 0 no vote yet (cleared from the zero page), j + 1 every vote so far is column j,
// kLocateConflict two lanes disagreed or one found no column.
constexpr uint32_t kLocateConflict = 0xFFFFFFFFu;
struct LocateArgs {
    VerifyArgs v;                 // data, recovery, G, shape and the scrub's lane grid (launch_locate: tiles 1)
    uint32_t *votes;              // workspace, stripes words
    int8_t *status;               // stripes: 0 clean, 1 rows[s] is the corrupt block, 2 no single block
    uint8_t *rows;                // stripes: the row (data x, recovery k + r), else 0xFF
};

// Repair (cauchy_256_reconstruct_batch): out_j = sum_slot B(C[j][slot]) block_slot over the k
// survivor slots of a stripe, for its `want` wanted rows.  lh_reconstruct_coef_kernel validates
// the stripe (survivor rows distinct and < k + m, wanted rows < k + m or 0xFF), writes status[s],
// valid[s] and C[s][want][k] (from the planner's single-pass W, PlanView::w_ptr; all 0 / 1 when
// `flat`); lh_reconstruct_kernel applies C and stores the wanted out blocks of the valid stripes.
struct ReconstructArgs {
    const uint8_t *blocks;        // survivor slot i of stripe s: blocks + s*blocks_stride + i*bytes
    long long blocks_stride;
    uint8_t *out;                 // out block j of stripe s: out + s*out_stride + j*bytes
    long long out_stride;
    // table != 0: pointer tables (cauchy_256_reconstruct_batch_ptrs; the strided fields unused):
    // slot i of stripe s at block_ptrs[s*k + i], out block j at out_ptrs[s*want + j] (not read
    // where the entry is 0xFF)
    int table;
    const uint8_t *const *block_ptrs;
    uint8_t *const *out_ptrs;
    const uint8_t *rows;          // the caller's rows[s*k + i] (the planner ran on a copy)
    const uint8_t *want_rows;     // want_rows[s*want + j]
    int8_t *status;               // optional, stripes
    const uint8_t *plan;          // PlanView records of the rows' copy (want_w), e_max = min(k, m); unused when `flat`
    long long plan_stride;
    uint8_t *coef;                // workspace: C[s][j][slot] at coef[(s*want + j)*k + slot]
    uint8_t *valid;               // workspace: valid[s] = 1, or 0: the stripe stores nothing
    const uint8_t *G;             // m x k generator (row 0 = ones); unused when `flat`
    const uint8_t *gf_exp;        // 512
    const int16_t *gf_log;        // 256
    int k, m, want, bytes, stripes;
    LaneGrid grid;                // tiles: the wanted-row tiles
};

// Launch trace (codec.cpp): every launch site records the kernel it enqueued, so the
// calling thread can ask which kernels its last batch call ran (cauchy_256_last_launch).
void note_launch(const char *kernel);

hipError_t launch_writeback(const WritebackArgs &a, hipStream_t st);
hipError_t launch_apply_generic(const ApplyArgs &a, int W, hipStream_t st);
hipError_t launch_apply_jump(const JumpApplyArgs &a, hipStream_t st);
// lh_inv_gtab2 lies within one 4 GiB page on `device` (probed once; dw 2 only then)
bool jump_table2_usable(int device);
// LONGHAIR_AMD_INV_FALLBACK is set and non-zero (tests): phase B and the one-dword jump apply
// take the in-asm table, and no batch takes two-dword lanes
bool inv_fallback_forced();
hipError_t launch_frame(const FrameArgs &a, hipStream_t st);
hipError_t launch_xor_reduce(const XorArgs &a, hipStream_t st);
hipError_t launch_scatter(const ScatterArgs &a, hipStream_t st);
hipError_t launch_plan(const PlanArgs &a, hipStream_t st);
hipError_t launch_ptr_copy(const PtrCopyArgs &a, hipStream_t st);
hipError_t launch_update(const UpdateArgs &a, hipStream_t st);
hipError_t launch_verify(const VerifyArgs &a, hipStream_t st);
hipError_t launch_locate(const LocateArgs &a, hipStream_t st);
hipError_t launch_reconstruct(const ReconstructArgs &a, hipStream_t st);

}  // namespace lh
