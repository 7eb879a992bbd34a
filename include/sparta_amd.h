/*
 * sparta_amd.h -- C-ABI of the MI355X-native block-sparse SpMM path
 * (Jaccard row-clustering reorder -> VBS build -> VBS A x dense B on gfx950).
 *
 * This is the drop-in boundary for the ONE hot path of HicrestLaboratory/SPARTA.  Every entry
 * point below cites the reference interface it replaces (paths relative to the reference tree).
 * Plain pointers and sizes only; no C++/torch types; no exceptions cross the boundary.
 * All functions return SPARTA_OK (0) or a negative status; sparta_last_error() returns a
 * thread-local message for the last failure on the calling thread.
 *
 * Conventions kept from the reference:
 *   - `intT` is 64-bit (include/definitions.h:4) -> every VBS index array is int64_t here.
 *   - A VBS block is column-major h x w, blocks of a block-row are consecutive, block-rows are
 *     consecutive (include/matrices.h:95-104).
 *   - B is column-major cols x N with ld = cols, C is column-major rows x N with ld = rows, the
 *     rows of C are in REORDERED order, and C is accumulated into (src/general/vbr.cpp:323-372).
 *     Both layouts and the accumulate flag are explicit arguments here.
 *   - `dt` is the device time of the multiply only, in milliseconds, excluding host<->device
 *     copies (src/cuda/cuda_utilities.cpp:828,872-875).
 */
#ifndef SPARTA_AMD_H
#define SPARTA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define SPARTA_OK               0
#define SPARTA_ERR_INVALID     -1   /* bad argument (null pointer, negative size, unsorted row, ...) */
#define SPARTA_ERR_ALLOC       -2   /* host or device allocation failed */
#define SPARTA_ERR_HIP         -3   /* a HIP runtime call failed (message has the HIP error string) */
#define SPARTA_ERR_UNSUPPORTED -4   /* valid request this build does not implement */
#define SPARTA_ERR_IO          -5   /* file could not be read / parsed */
#define SPARTA_ERR_NO_DEVICE   -6   /* no gfx950 device visible: the product path has NO CPU fallback */

/* ---- enums -------------------------------------------------------------------------------- */
/* storage/compute type of the VBS values on the device; accumulation is always fp32 */
#define SPARTA_F32  0
#define SPARTA_F16  1
#define SPARTA_BF16 2

#define SPARTA_COL_MAJOR 0          /* the reference's layout for B and C */
#define SPARTA_ROW_MAJOR 1

#define SPARTA_PTR_HOST   0         /* B and C are host buffers: copied in/out, dt excludes the copies */
#define SPARTA_PTR_DEVICE 1         /* B and C are device buffers: stream-ordered, nothing is copied */

/* BlockingType of the reference, same numeric values (include/definitions.h:17; flag -a) */
#define SPARTA_BLOCKING_ITERATIVE            0
#define SPARTA_BLOCKING_ITERATIVE_STRUCTURED 1   /* m:n structured variant (IterativeBlockingPatternMN, blocking.cpp:19-87) */
#define SPARTA_BLOCKING_FIXED_SIZE           2
#define SPARTA_BLOCKING_ITERATIVE_CLOCKED    3   /* the reference's default (include/input.h:27) */
#define SPARTA_BLOCKING_ITERATIVE_QUEUE      4
#define SPARTA_BLOCKING_ITERATIVE_MAX_SIZE   5   /* dispatches to IterativeBlockingKeeper (blocking.cpp:655) */
#define SPARTA_BLOCKING_SCRAMBLE             6
#define SPARTA_BLOCKING_MINHASH              7   /* EXTENSION (not in the reference): LSH-bucketed clustering with the same merge rule, for inputs
                                                   the quadratic scans cannot handle (approximate: see sparta_amd/csrc/reorder.cpp) */

/* similarity measure, flag -m (include/input.h:29, src/general/blocking.cpp:699-717) */
#define SPARTA_SIM_HAMMING 0
#define SPARTA_SIM_JACCARD 1

/* kernel selection for sparta_vbs_spmm (`algo` argument).  Within SPARTA_SPMM_MFMA the library picks between its
 * product paths by measuring them once per (n_cols, layouts) on the handle; env SPARTA_PATH=stream|class|generic forces one. */
#define SPARTA_SPMM_MFMA  0   /* hand-written MFMA kernels (the product path) */
#define SPARTA_SPMM_EXACT 1   /* fp32 only: unfused mul+add in the reference's summation order,
                                 bit-identical to VBR::multiply on finite inputs (slow; for parity) */

/* ---- reorder (host-side C++) -------------------------------------------------------------- */
/* replaces the configuration fields of class BlockingEngine (include/blocking.h:12-23) as filled
 * from the command line by BlockingEngine(CLineReader&) (src/general/blocking.cpp:678-688). */
typedef struct sparta_reorder_cfg {
    int32_t blocking_algo;     /* SPARTA_BLOCKING_*            (-a, default 3)    */
    int32_t sim_measure;       /* SPARTA_SIM_*                 (-m, default 1)    */
    float   tau;               /* merge threshold, dist <= tau (-t, default 0.1)  */
    int32_t use_groups;        /* weight distances by cluster size (-g, default 0)*/
    int64_t col_block_size;    /* w                            (-b, default 3)    */
    int64_t row_block_size;    /* max / fixed block-row height (-B, default 3)    */
    int32_t use_pattern;       /* merge rows into the pattern  (-p, default 1)    */
    int32_t force_fixed_size;  /* re-chunk into equal heights  (-F, default 0)    */
    int32_t structured_m;      /* blocking_algo 1 only: at most m hits per column ... (include/blocking.h:20, default 2) */
    int32_t structured_n;      /* ... inside every run of n merged rows               (include/blocking.h:21, default 4) */
    int32_t minhash_bands;     /* blocking_algo 7 only: LSH bands (0 = 16) ...                                              */
    int32_t minhash_rows;      /* ... minhash values per band (0 = from tau), ...                                            */
    int32_t minhash_max_eval;  /* ... exact comparisons per seed at most (0 = 512), ...                                       */
    int32_t minhash_max_rows;  /* ... a cluster never grows beyond this many rows (0 = unlimited); only a seed's own identical copies can exceed it */
} sparta_reorder_cfg;

/* replaces the measuring fields of BlockingEngine (include/blocking.h:28-42) */
typedef struct sparta_reorder_stats {
    int64_t comparison_counter;
    int64_t merge_counter;
    float   average_row_distance;
    float   average_merge_tau;
    float   timer_total;        /* microseconds, as in the reference (blocking.cpp:236-238) */
    float   timer_comparisons;
    float   timer_merges;
    int32_t reserved;
} sparta_reorder_stats;

/* fills *cfg with the reference's command-line defaults (include/input.h:15-42) */
void sparta_reorder_cfg_default(sparta_reorder_cfg* cfg);

/* replaces std::vector<intT> BlockingEngine::GetGrouping(const CSR&)  (include/blocking.h:47,
 * src/general/blocking.cpp:633-676).  The CSR is flat: rowptr[rows+1], colidx ascending within each
 * row.  grouping_out[rows] receives one group id per row (the reference's convention: the id is the
 * seed row; algo 5 numbers incomplete clusters seed+rows).  stats may be NULL. */
int sparta_reorder(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx,
                   const sparta_reorder_cfg* cfg, int64_t* grouping_out, sparta_reorder_stats* stats);

/* replaces get_permutation / get_partition / get_fixed_size_grouping (src/general/utilities.cpp:8-54).
 * perm_out[new_row] = old_row.  part_out needs room for n+1 entries; *n_part_out receives the count
 * (block_rows + 1). */
int sparta_get_permutation(const int64_t* grouping, int64_t n, int64_t* perm_out);
int sparta_get_partition(const int64_t* grouping, int64_t n, int64_t* part_out, int64_t* n_part_out);
int sparta_get_fixed_size_grouping(const int64_t* grouping, int64_t n, int64_t row_block_size, int64_t* grouping_out);

/* replaces HammingDistanceGroup / JaccardDistanceGroup (src/general/blocking.cpp:859-994): distance
 * between a cluster pattern row_a (column ids, weight group_a) and a row row_b (weight group_b) on
 * column blocks of width block_size. */
int sparta_row_distance(int32_t sim_measure, const int64_t* row_a, int64_t size_a, int64_t group_a,
                        const int64_t* row_b, int64_t size_b, int64_t group_b, int64_t block_size, float* dist_out);

/* replaces merge_rows (src/general/utilities.cpp:145-173), including its lossy behaviour.
 * out needs room for size_a + size_b entries. */
int sparta_merge_rows(const int64_t* row_a, int64_t size_a, const int64_t* row_b, int64_t size_b,
                      int64_t* out, int64_t* size_out);

/* ---- on-disk formats either side of the path (host-side C++, sparta_amd/csrc/io.cpp) ------- */
#define SPARTA_FMT_EL  0            /* MatrixFormat::el  (include/definitions.h:15; flag -R 0) */
#define SPARTA_FMT_MTX 1            /* MatrixFormat::mtx (flag -R 1) */
#define SPARTA_IO_COMPAT 0          /* what the reference's readers do, quirks included */
#define SPARTA_IO_STRICT 1          /* the formats as documented: no dropped line, MatrixMarket banner/values/symmetry honoured */

/* a CSR in flat arrays, owned by the library (release with sparta_csr_host_free) */
typedef struct sparta_csr_host {
    int64_t rows, cols, nnz;
    int32_t pattern_only;         /* 1: vals == NULL, every stored entry counts as 1 (include/matrices.h:28) */
    int64_t* rowptr;              /* [rows + 1] */
    int32_t* colidx;              /* [nnz], in file order inside a row (the reference never sorts a row) */
    float*   vals;                /* [nnz] or NULL */
} sparta_csr_host;

/* replaces CSR::read_from_edgelist(infile, delimiter, pattern_only, mat_fmt, symmetrize)
 * (include/matrices.h:63, src/general/csr.cpp:183-365).  SPARTA_IO_COMPAT: `.el` -- leading '#'/'%' lines skipped, THE
 * FIRST REMAINING LINE IS DISCARDED (csr.cpp:213), "row<delim>col[<delim>value]" per line, row ids non-decreasing, rows =
 * last row id + 1, cols = largest column id + 1, symmetrize mirrors an upper-triangular pattern-only input; `.mtx` -- always
 * pattern-only, one line after the size line is skipped, symmetry ignored (csr.cpp:309-365).  Inputs on which the
 * reference throws or runs into undefined behaviour return SPARTA_ERR_IO.  SPARTA_IO_STRICT reads the documented formats. */
int sparta_csr_read(const char* path, const char* delimiter, int32_t pattern_only, int32_t mat_fmt, int32_t symmetrize, int32_t mode,
                    sparta_csr_host* out);
/* the same readers on a text already in memory (what is left in the std::ifstream the reference's CSR constructor is handed,
 * include/matrices.h:58-63) */
int sparta_csr_read_buffer(const char* text, int64_t len, const char* delimiter, int32_t pattern_only, int32_t mat_fmt, int32_t symmetrize,
                           int32_t mode, sparta_csr_host* out);
void sparta_csr_host_free(sparta_csr_host* m);

/* replaces CSR::save_to_edgelist (src/general/csr.cpp:169-179): "i<delim>j" per entry (el) / "j<delim>i" (mtx flavour) */
int sparta_csr_write_edgelist(const char* path, int64_t rows, const int64_t* rowptr, const int32_t* colidx, const char* delimiter,
                              int32_t mat_fmt);

/* the grouping file `<outfile>.g` that save_blocking_data writes (src/general/utilities.cpp:239-243): one group id per line */
int sparta_grouping_write(const char* path, const int64_t* grouping, int64_t n);
/* replaces read_grouping_file + the count-line rule of test/general/Matrix_Analysis.cpp:10-32,77-78: lines that do not start
 * with a number are skipped; a file with expected_rows + 1 numbers has a leading count, which is dropped.  expected_rows < 0:
 * no check.  *n_out = number of ids found (also on SPARTA_ERR_IO when it does not match expected_rows). */
int sparta_grouping_read(const char* path, int64_t expected_rows, int64_t* out, int64_t capacity, int64_t* n_out);

/* the reference's 32-column statistics row (src/general/utilities.cpp:175-236): one header line and one value line, every field
 * followed by ','; floats print as std::to_string(float) ("%f").  Field names are the reference's CSV column names. */
typedef struct sparta_csv_fields {
    const char* matrix;           /* CLineReader::filename_ */
    int64_t rows, cols, nonzeros;
    int32_t symmetrize, blocking_algo;
    float   tau;
    int32_t row_block_size, col_block_size, use_pattern, sim_use_groups, sim_measure, reorder;
    const char* exp_name;
    int32_t b_cols, warmup, exp_repetitions, multiplication_algo, n_streams;
    float   time_to_block, time_to_merge, time_to_compare;          /* microseconds (sparta_reorder_stats) */
    int64_t vbr_nzcount, vbr_nzblocks_count;                        /* sparta_blocking_info */
    float   vbr_average_height;
    int64_t vbr_longest_row, merge_counter, comparison_counter;
    float   average_merge_tau, average_row_distance;
    float   avg_time_multiply, std_time_multiply;                   /* milliseconds */
} sparta_csv_fields;
int sparta_blocking_csv_row(const sparta_csv_fields* f, char* header_out, int64_t header_cap, char* values_out, int64_t values_cap);

/* the row permutation of CSR::reorder_by_degree (src/general/csr.cpp:123-155; flag -r -1 / 1): perm_out[k] = old index of
 * the row that moves to position k (apply with CSR::permute_rows semantics, utilities.h:95-107) */
int sparta_degree_permutation(int64_t rows, const int64_t* rowptr, int32_t descending, int64_t* perm_out);

/* ---- VBS build (host-side C++) ------------------------------------------------------------- */
/* the five arrays + scalars of struct VBR (include/matrices.h:93-104), owned by the library */
typedef struct sparta_vbs_host {
    int64_t rows, cols;           /* padded up to block multiples when force_fixed_size */
    int64_t block_rows, block_cols;
    int64_t block_col_size;
    int64_t nztot;                /* number of stored values = sum h*w over nonzero blocks */
    int64_t nblocks;              /* number of nonzero blocks = sum nzcount */
    int64_t* row_part;            /* [block_rows + 1] */
    int64_t* nzcount;             /* [block_rows]     */
    int64_t* jab;                 /* [nblocks]        */
    float*   mab;                 /* [nztot]          */
} sparta_vbs_host;

/* replaces VBR::fill_from_CSR_inplace(cmat, grouping, col_block_size, row_block_size, force_fixed_size)
 * (include/matrices.h:118, src/general/vbr.cpp:135-237).  vals == NULL means pattern-only (every
 * stored nonzero is 1, vbr.cpp:217).  The caller releases *out with sparta_vbs_host_free. */
int sparta_vbs_build(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                     const int64_t* grouping, int64_t col_block_size, int64_t row_block_size, int32_t force_fixed_size,
                     sparta_vbs_host* out);
void sparta_vbs_host_free(sparta_vbs_host* v);

/* replaces VBR::fill_from_CSR(cmat, row_partition, block_size) (include/matrices.h:117, src/general/vbr.cpp:239-321): the rows
 * keep their order, block-row ib = rows [row_partition[ib], row_partition[ib+1]); repeated entries give block-rows of height 0
 * with nzcount 0, as in the reference.  Where the reference prints "PARTITION CHECK ERROR" and continues (vbr.cpp:253-257) this
 * returns SPARTA_ERR_INVALID. */
int sparta_vbs_build_partition(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                               const int64_t* row_partition, int64_t n_part, int64_t block_size, sparta_vbs_host* out);
/* replaces VBR::partition_check(candidate_part) (src/general/vbr.cpp:108-118): 0 = valid, 1 = empty, 2 = last entry != rows,
 * 3 = decreasing.  (A status of the partition, not a SPARTA_* code.) */
int sparta_vbs_partition_check(const int64_t* part, int64_t n_part, int64_t rows);

/* Binary VBS container ("SPARTAVB", little-endian, 96-byte header + the four arrays, FNV-1a checksum; layout in
 * sparta_amd/csrc/io.cpp): the reorder + build cost is paid once.  sparta_vbs_load verifies magic, sizes, checksum and the
 * structural invariants and fills *out (release with sparta_vbs_host_free).  No reference counterpart. */
int sparta_vbs_save(const char* path, const sparta_vbs_host* v);
int sparta_vbs_load(const char* path, sparta_vbs_host* out);

/* Blocked-ELL view of a fixed-square-block VBS: replaces prepare_cusparse_BLOCKEDELLPACK(VBR*, int* ell_blocksize, int* ellValue_cols,
 * int* ellColInd_rows, int* ellColInd_cols, int* num_blocks, intT** ellColInd, DataT_C** ellValues)
 * (src/cuda/cuda_utilities.cpp:1656-1710) -- the arrays the reference hands to cusparseCreateBlockedEll.  ell_blocksize =
 * block_col_size; *ell_cols_out = most blocks in a block-row; ell_col_ind: (rows / bs) x ell_cols, -1 = padding block;
 * ell_values: rows x (ell_cols * bs), row-major.  Call with ell_col_ind = ell_values = NULL to get ell_cols first.
 * SPARTA_ERR_INVALID where the reference exits (rows or cols not a multiple of the block size) and where its silent
 * assumption fails (a block-row that is not bs rows tall). */
int sparta_vbs_to_blocked_ell(const sparta_vbs_host* v, int64_t* ell_cols_out, int64_t* ell_col_ind, float* ell_values);

/* replaces BlockingEngine::CollectBlockingInfo (src/general/blocking.cpp:576-631): statistics of
 * the VBS a grouping would give, without building it. info_out: [VBR_nzcount, VBR_nzblocks_count,
 * VBR_longest_row]; avg_height_out: VBR_average_height. */
int sparta_blocking_info(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx,
                         const int64_t* grouping, int64_t col_block_size, int64_t* info_out, float* avg_height_out);

/* ---- device: VBS A x dense B (hand-written HIP, gfx950) ---------------------------------------- */
typedef struct sparta_vbs sparta_vbs_t;   /* opaque; owns the device image of A and the launch plan */

/* Uploads a VBS matrix (the reference's arrays, host pointers) to `device` once and builds the tile
 * plan.  Replaces the per-call cudaMalloc + H2D of A that every reference back-end performs
 * (src/cuda/cuda_utilities.cpp:779-789).  dtype SPARTA_F16 / SPARTA_BF16: the values are rounded (nearest even) and
 * re-laid-out for the 16-bit MFMA here, once (needs block_col_size % 32 == 0); products are accumulated in fp32. */
int sparta_vbs_create(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size,
                      const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, const float* mab,
                      int32_t dtype, int32_t device);

/* Same, restricted to block-rows [block_row_begin, block_row_end): the row-range partition used for
 * multi-GPU runs.  C of the resulting handle has row_part[end]-row_part[begin] rows (local numbering). */
int sparta_vbs_create_range(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size,
                            const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, const float* mab,
                            int64_t block_row_begin, int64_t block_row_end, int32_t dtype, int32_t device);

/* sparta_vbs_create_range with creation flags.  flags = 0 is sparta_vbs_create_range exactly (that entry calls this one).
 * SPARTA_CREATE_UPDATABLE: the handle can take new values for the same block pattern through sparta_vbs_set_values.  Such a handle keeps
 * every block-row in its dense-block images (no block-row moves to the sparse-row kernels, whose image holds only what was non-zero at
 * creation) and, for 16-bit handles, 32 bytes per 2-8 KB slice that say where in mab the slice came from.  Everything else -- plans,
 * kernels, products -- is as for flags = 0.  Unknown bits (flags & ~3): SPARTA_ERR_INVALID.
 * SPARTA_CREATE_TRANSPOSE: the handle also takes sparta_vbs_spmm_t (Ct = A^T * X on its own stored blocks).  It holds a block-column index
 * (16 bytes per block + 16 per block column and 32-column panel) and an image that product can read: an fp32 handle KEEPS its
 * reference-layout image (plain handles shed that second fp32 image after the first product; on the benchmark's headline handle this
 * costs about 90 MB), a 16-bit handle gets a second 16-bit image of about nztot * 2 bytes (counted in info[10]).  The forward product --
 * plans, kernels, which block-rows go to the sparse-row kernels -- is that of a handle without the bit.  Combines with
 * SPARTA_CREATE_UPDATABLE: sparta_vbs_set_values then rewrites what the transposed product reads, too. */
#define SPARTA_CREATE_UPDATABLE 1
#define SPARTA_CREATE_TRANSPOSE 2
int sparta_vbs_create_range_ex(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size,
                               const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, const float* mab,
                               int64_t block_row_begin, int64_t block_row_end, int32_t dtype, int32_t device, int32_t flags);
/* the flags a handle was created with (0 for sparta_vbs_create, _create_range, _create_from_csr, _create_transposed) */
int sparta_vbs_flags(const sparta_vbs_t* A, int32_t* flags_out);

/* Device handle straight from the CSR and a grouping, for matrices whose VBS image is mostly zeros (clustered power-law graphs:
 * 98 % of the stored area): does what sparta_vbs_build + sparta_vbs_create do, except that the block-rows the sparse-row
 * kernels will take anyway are never expanded into dense blocks -- neither on the host nor on the device.  Same product as a
 * handle made the two-step way (same decisions, same kernels, same data).  Columns must be strictly ascending within a row.
 * SPARTA_SPMM_EXACT is not available on such a handle.  No reference counterpart (the reference always expands:
 * src/general/vbr.cpp:205-228). */
int sparta_vbs_create_from_csr(sparta_vbs_t** out, int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                               const int64_t* grouping, int64_t col_block_size, int64_t row_block_size, int32_t force_fixed_size,
                               int32_t dtype, int32_t device);

/* What sparta_vbs_create_from_csr WOULD build for this grouping, without building or uploading anything (no GPU needed): the same
 * per-block decisions (well-filled blocks -> dense MFMA tiles, the nonzeros of the others -> rows of (column, value) for the sparse-row
 * kernels).  stats[8] = {tile blocks, stored elements of the tiles, MFMA steps of the tiles, sparse nonzeros, sparse rows, block-rows,
 * rows, 0}.  Lets a caller compare two blockings of one matrix -- the clustering of sparta_reorder against the fixed grid of the
 * reference's `-a 2 -F 1` arm (src/scripts/run_multiplication_experiments_fixed_cluster.sh:14-16) -- before paying for either handle. */
int sparta_vbs_plan_stats(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* grouping,
                          int64_t col_block_size, int64_t row_block_size, int32_t force_fixed_size, int32_t dtype, int64_t* stats);

/* C (+)= A * B.  Replaces VBR::multiply(B, B_cols, C) (include/matrices.h:121) and the GPU back-ends
 *   cublas_fixed_blocks_multiply / cublas_blockmat_batched / cutlas_* (const VBR&, DataT* B, int B_cols,
 *   DataT_C* C, float& dt[, int n_streams])            (include/cuda_utilities.h:38-44,
 *                                                        include/cutlass_bellpack_lib.h:19-25).
 * B: `cols` x n_cols, C: `rows` x n_cols (rows of this handle).  fp32 handles: fp32 B and C, any layout, any n_cols.
 * 16-bit handles: C is fp32; with SPARTA_PTR_DEVICE B is in the handle's 16-bit type, column-major, ldb even; any n_cols (the
 * reference's `-c` is arbitrary, include/input.h:15-42): whole 128-column slabs go through the kernels as they are, the last
 * n_cols % 128 columns through a zero-padded slab in per-handle scratch (128 columns of B and of C); with SPARTA_PTR_HOST B is fp32
 * like in the reference and is rounded on the device.  Tolerance of the 16-bit path: exact products of the ROUNDED inputs, fp32 accumulation -- the same bound
 * as the fp32 MFMA path relative to the reference's multiply run on the rounded inputs.  accumulate = 1 is the reference's
 * semantics (C += A*B); 0 overwrites C (every row of C is written).  ptr_space HOST: buffers are
 * copied to/from the device around the kernel and *dt_ms (may be NULL) covers the kernel only;
 * DEVICE: launched on `stream` (a hipStream_t, NULL = default stream); if dt_ms != NULL the call
 * records events and synchronises on them, otherwise it returns without synchronising.
 * Leading dimensions: the stream kernels address B and C with 32-bit byte offsets inside a column slab.  fp32 handles take the 64-bit
 * per-class kernels beyond ldb, ldc ~ 4.2 M elements (column-major; correct, slower); 16-bit handles run up to ldb < 34 M (16 M for SPARTA_H16_WIDE plans), ldc < 17 M elements
 * and return SPARTA_ERR_UNSUPPORTED beyond (a gathered B has the slab height as its leading dimension).
 * A handle carries per-handle scratch (split-tile workspace, layout copies of B, step lists of a gathered B): it must not run on two
 * streams at once.  The FIRST call of a shape (n_cols, layouts, shard_rows) on a handle may allocate that scratch, and on fp32 handles
 * times its two product paths once; every later call of the shape is kernel launches only and can be captured into a hipGraph.  A call
 * that would have to allocate or time while its stream is being captured returns SPARTA_ERR_UNSUPPORTED (and leaves the capture
 * intact): run it once outside the capture first.
 * A CAPTURED GRAPH STAYS VALID FOR AS LONG AS THE HANDLE LIVES: a graph captured from any call on a handle replays with the result of the eager call
 * it was captured from, whatever other calls (other n_cols, leading dimensions, layouts, slab heights, SPARTA_PTR_HOST calls) are made on the handle
 * between replays, on the same stream.  The cost: once a call on the handle has been captured, scratch that a later, larger shape outgrows is kept
 * until sparta_vbs_destroy instead of being freed (each retired buffer is smaller than its successor, so at most as much again as the largest);
 * every slab height of a gathered B keeps step lists of its own (captured or not); and an fp32 handle that would drop its reference-layout image of
 * A once the no-barrier kernel carries its products keeps both images.  sparta_debug_device_allocs counts all of it; a handle that is never captured
 * frees and reallocates as before.
 *
 * WHERE A DEVICE OPERAND MAY START (SPARTA_PTR_DEVICE; tests/test_footprint_gpu.py runs the products at offset bases inside guarded arenas).
 *   fp32 operands -- B, C, X, Y, G, Ct and mab of sparta_vbs_spmm, _gathered, _gathered_ld, _prepared, sparta_vbs_prepare_b, sparta_vbs_sddmm,
 *   sparta_vbs_spmm_t and sparta_vbs_set_values -- may start on ANY 4-byte boundary and have any leading dimension the entry accepts: a slice of a
 *   larger buffer is a valid operand.  Wider alignment only selects faster code (non-temporal stores of C when ldc % 32 == 0 and C is 128-byte aligned,
 *   16-byte vectors in the resident-column and sparse-row kernels, a row-major B read in place by the column-compacted tiles when its rows are 16-byte
 *   aligned); the result has the same bits either way, and nothing outside the defined elements of an output is written.
 *   16-bit operands -- B of sparta_vbs_spmm, _gathered, _gathered_ld and sparta_vbs_prepare_b, X and Y of sparta_vbs_sddmm, X of sparta_vbs_spmm_t --
 *   must start on a 4-byte boundary (an EVEN element), as their leading dimensions must be even: the forward kernels read B a dword and more at a time,
 *   some straight into LDS.  A base on an odd element is refused before anything is launched, with the code the entry uses for an odd leading dimension
 *   (SPARTA_ERR_UNSUPPORTED from the forward products and sparta_vbs_prepare_b, SPARTA_ERR_INVALID from sparta_vbs_sddmm and sparta_vbs_spmm_t); the
 *   outputs keep every bit.  The one exception is sparta_vbs_sddmm_block_ssq: its X and Y may start on ANY element (2-byte boundary) -- its kernel reads X
 *   one element at a time and tests the address of Y itself before it takes 16-byte loads (tests/test_sddmm_score_gpu.py: test_operand_placement holds it
 *   to the bits of the aligned call).
 *
 * WHAT AN OUTPUT ELEMENT DEPENDS ON (non-finite operands included: Inf and NaN are ordinary data, and 0 * Inf is NaN, so "multiplied by a zero"
 * is not "not read"; tests/test_poison_gpu.py).
 *   Forward products (sparta_vbs_spmm, _gathered, _gathered_ld, _prepared, SPARTA_SPMM_EXACT, sparta_vbs_spmm_ba on B^T): C[i, j] depends only on
 *   column j of B, and there only on the rows k that lie inside a block column which the block-row of row i stores -- for a handle from
 *   sparta_vbs_create_from_csr: a block column of the grouping's w-grid in which the block-row has a nonzero.  Stored positions past `cols`, the padding
 *   of a leading dimension and the gap between two slabs of a gathered B take no part.  However a planner groups block-rows into tiles (pair tiles, hub
 *   group tiles, union tiles), a block column that only a neighbour in the tile stores does not reach the rows of this block-row: a NaN in one row of B
 *   makes non-finite exactly the rows of C whose block-rows store that row's block column.
 *   Stored zeros: whether a stored 0.0 of A times a non-finite element of B gives NaN (the reference's VBR::multiply, the MFMA tiles) or is skipped (the
 *   sparse-row kernels, the fp32 k-compaction, create_from_csr dropping zeros) is NOT specified: such an element of C may be either.
 *   sparta_vbs_spmm_t: Ct[c, j] depends only on column j of X, and there only on the rows of the block-rows that store the block column of c.
 *   sparta_vbs_sddmm: the values of G in block (ib, jb) depend only on X's rows of block-row ib and Y's rows of block column jb (G[off + q * h + i]: row i
 *   of the block-row, row jb * w + q of Y), and with accumulate = 1 on their own previous value.
 *   sparta_vbs_set_values: a non-finite value in a stored block reaches only rows of C of that block's block-row (and, through spmm_t, rows of Ct of its
 *   block column); the next set_values replaces it completely.
 *   Overwriting calls (accumulate = 0) do not depend on the previous content of the output, NaN included.
 *   WITH A LIVE-BLOCK SET INSTALLED (sparta_vbs_set_live_blocks; a block is dead when its byte of the snapshot is 0):
 *   sparta_vbs_sddmm: the elements of G in a live block have the same bits as the same call without a live set.  A dead block depends on nothing: neither
 *   X's rows of its block-row nor Y's rows of its block column are read on its behalf.  accumulate = 0: all n_all elements of a dead block are +0.0f, the
 *   positions past `cols` included.  accumulate = 1: its elements are neither read nor written -- a -0.0f, a NaN or any other bits there stay.
 *   sparta_vbs_spmm_t: Ct[c, j] is the sum over the LIVE blocks of c's block column only, in block-row order: still one wave, one fixed order, no atomics.
 *   accumulate = 0 still writes all cols x n_cols elements, zeros where no live block covers a column.  Rows of X that reach a block column only through
 *   dead blocks are not read for it.  Dropping a block removes whole MFMA passes (a pass covers rows of one block only): with finite X the result equals,
 *   up to the sign of a zero, the product without a live set on values whose dead blocks are zero.
 *   Everything else ignores the live set: the forward products (unless live forward is on, below), sparta_vbs_set_values, the steps (unless live steps are on, below), sparta_vbs_block_ssq,
 *   sparta_vbs_mask_blocks.  Keeping the VALUES of dead blocks at zero stays the caller's job.
 *   WITH A LIVE-BLOCK SET INSTALLED AND LIVE STEPS ON (sparta_vbs_set_live_steps), for sparta_vbs_sgd_step, sparta_vbs_adam_step and both _ctl forms, in the
 *   fused and in the two-pass form:
 *   Live blocks: every element gets the pinned arithmetic of the plain step and the same bits.
 *   Dead blocks: G, M and V are neither read nor written -- all n_all elements, the positions past `cols` included -- and W is not written.  Every image the
 *   step's own kernel writes holds +0.0 for them.  PRECONDITION: W holds +0.0 there, as sparta_vbs_mask_blocks leaves it; the images written by the set_values
 *   launches that follow the step's kernel (the two-pass form; the image of sparta_vbs_spmm_t of a 16-bit handle) come from W as it stands.  If the
 *   precondition is broken W, M and V are still untouched, and those images hold whatever W held, rounded.
 *   The Adam step state: the tick and S are unchanged; a skipped step (R[skip]) behaves as without live steps (W, M, V, S keep their bits; the fused kernel
 *   still writes +0.0 for dead blocks into its image).
 *   Equivalence: on tensors whose dead blocks are +0 in W, M, V and G a live step leaves W, M, V, S and every product of the handle bit-identical to the
 *   plain step (which computes +0 for them: "A zero block stays zero", below).
 *   WITH A LIVE-BLOCK SET INSTALLED AND LIVE FORWARD ON (sparta_vbs_set_live_forward), for sparta_vbs_spmm on a 16-bit handle that takes the live form
 *   (sparta_vbs_live_forward_info word 1; every other handle and launch keeps the text above):
 *   A dead block contributes nothing to C, whatever the image holds for it, NaN included.  Neither its slice of A nor, on its behalf, the rows of B is read:
 *   its steps are not in a worker's live range, and what is kept of them (the dead half of a pair-tile step whose other half is live, the one step that
 *   carries the epilogue of a tile piece without a live block) loads through descriptors of zero records and meets B fragments ANDed with 0.  (The load
 *   pipeline still runs three records past the end of a live range, as it runs past the end of a plain one: those loads are issued and never used.)
 *   Rows of C reached only through dead blocks are +0.0, or unchanged under accumulate = 1.
 *   Equivalence: on values whose dead blocks are zero, C equals the plain product element for element, the sign of a zero aside -- whole steps of exact zero
 *   products are dropped and the order of the rest is kept. */
int sparta_vbs_spmm(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int32_t n_cols,
                    void* C, int64_t ldc, int32_t c_layout, int32_t accumulate,
                    int32_t ptr_space, void* stream, int32_t algo, float* dt_ms);

/* Multi-GPU entry point: B_gathered is what ONE ncclAllGather (RCCL) of the ranks' row shards of B leaves on
 * every GPU: n_shards consecutive column-major slabs of shard_rows x n_cols (ld = shard_rows), slab s holding
 * rows [s*shard_rows, (s+1)*shard_rows) of B, consecutive slabs shard_stride elements apart.  shard_rows must
 * be a multiple of block_col_size (so that no B panel straddles two slabs) and cols == n_shards * shard_rows.
 * Device pointers only; 16-bit handles take the slabs in their 16-bit type (shard_rows and shard_stride even).
 * No reference counterpart (the reference is single-GPU: SURVEY.md section 2.1). */
int sparta_vbs_spmm_gathered(sparta_vbs_t* A, const void* B_gathered, int64_t shard_rows, int64_t shard_stride, int32_t n_cols,
                             void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, void* stream, int32_t algo, float* dt_ms);
/* the same with the columns of a slab `shard_ld` >= shard_rows elements apart (sparta_vbs_spmm_gathered: shard_ld = shard_rows; 16-bit handles: shard_ld even).
 * Why: a leading dimension that is a multiple of a large power of two -- 2^20 rows of a 16-bit B: columns exactly 2 MB apart -- maps the columns of a panel of B
 * onto the same cache sets and memory channels: the hub kernel of a 16-bit handle measured 0.80 PFLOP/s with such a B and 1.05 with 64 elements of padding per
 * column (MI355X).  Pad the ranks' shard buffers before the all-gather (bench_parts.py does); for sparta_vbs_spmm the same advice holds for
 * ldb.  No reference counterpart (single-GPU). */
int sparta_vbs_spmm_gathered_ld(sparta_vbs_t* A, const void* B_gathered, int64_t shard_rows, int64_t shard_ld, int64_t shard_stride, int32_t n_cols,
                                void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, void* stream, int32_t algo, float* dt_ms);

/* Multi-GPU, sparsity-aware exchange: gathers chunks of `block_bytes` bytes (a multiple of 16; one chunk = one
 * block_col_size x n_cols tile of B in the row-block-tiled layout) from `src` into consecutive chunks of `dst`:
 * dst chunk i = src chunk ids_dev[i].  All pointers are device pointers (16-byte aligned); stream-ordered.  A rank uses it
 * to assemble the send buffer of the ONE all-to-all that ships to every other rank exactly the row-blocks of B that rank's
 * slab of A touches (sparta_amd/dist.py: RowBlockExchange); the receive buffer is then read in place by
 * sparta_vbs_spmm_gathered(shard_rows = block_col_size, shard_stride = block_col_size * n_cols).
 * No reference counterpart (single-GPU). */
int sparta_pack_blocks(const void* src, int64_t block_bytes, const int32_t* ids_dev, int64_t n_blocks, void* dst, void* stream);

/* B * A (dense x VBS).  The reference's cublas_blockmat_multiplyBA(const VBR&, DataT* B, int B_rows, DataT_C* C, float& dt, int n_streams)
 * (include/cuda_utilities.h:40, src/cuda/cuda_utilities.cpp:553-721) is NOT a B * A (it offsets B by block_col_size * ib elements, uses
 * the first block-row's height for every block and sizes C as B_rows x A_rows: DESIGN.md section 8), so there is nothing to be identical
 * to; these two entries compute the product itself.  sparta_vbs_create_transposed uploads A^T (same VBS arrays as sparta_vbs_create);
 * sparta_vbs_spmm_ba: C (M x cols, column-major, ldc) (+)= B (M x rows, column-major, ldb) * A, rows of A in the VBS's (reordered) order.
 * fp32 tolerance as for sparta_vbs_spmm. */
int sparta_vbs_create_transposed(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size,
                                 const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, const float* mab,
                                 int32_t dtype, int32_t device);
int sparta_vbs_spmm_ba(sparta_vbs_t* At, const void* B, int64_t ldb, int32_t M, void* C, int64_t ldc, int32_t accumulate,
                       int32_t ptr_space, void* stream, float* dt_ms);

/* SDDMM on the stored blocks of A: G (+)= (X * Y^T) sampled on A's pattern, in the handle's mab layout -- the gradient of A's values for
 * C = A * B (X = dC, Y = B).  No reference counterpart (the reference only multiplies).
 * X: rows x k, column-major, ldx >= rows (the layout of C, rows in the VBS's reordered order; a force_fixed_size padding row is a row like
 * any other).  Y: cols x k, column-major, ldy >= cols (the layout of B).  G: nztot fp32 values laid out as sparta_vbs_host.mab (for a range
 * handle the slice of its block-rows, from 0): for block-row ib (rows r0 ..), its block b (block-column jb), in-block column c, row i:
 *   G[a_off + (b * w + c) * h + i] = sum_n X[r0 + i, n] * Y[jb * w + c, n];   positions with jb * w + c >= cols (ragged last block column) get 0.
 * accumulate = 0 writes all nztot values, 1 adds to them.  fp32 handles take fp32 X, Y; 16-bit handles take X, Y in the handle's type with
 * even ldx, ldy and accumulate in fp32 (exact products of the 16-bit inputs).  SPARTA_PTR_HOST: X, Y are fp32 host arrays (rounded on the
 * device for 16-bit handles), G is a host array, *dt_ms (may be NULL) covers the kernel only; SPARTA_PTR_DEVICE: stream and dt_ms as for
 * sparta_vbs_spmm.  Any k >= 1.  Offsets into X, Y and G are 64-bit; ldx * k and ldy * k must stay below 2^61 (else SPARTA_ERR_UNSUPPORTED).
 * SPARTA_ERR_UNSUPPORTED on a handle without the dense blocks of every block-row (made by sparta_vbs_create_from_csr, hence also
 * sparta_vbs_create_transposed).  The FIRST call on a handle builds and uploads the work list (and, for SPARTA_PTR_HOST, scratch); every
 * later device-pointer call is kernel launches only and can be captured into a hipGraph -- a call that would still have to allocate while
 * its stream is being captured returns SPARTA_ERR_UNSUPPORTED. */
int sparta_vbs_sddmm(sparta_vbs_t* A, const void* X, int64_t ldx, const void* Y, int64_t ldy, int32_t k, float* G, int32_t accumulate,
                     int32_t ptr_space, void* stream, float* dt_ms);

/* New values for the stored blocks of a handle made with SPARTA_CREATE_UPDATABLE, same block pattern: mab is nztot fp32 values laid out
 * as sparta_vbs_host.mab (for a range handle the slice of its block-rows, from 0) -- the layout of G of sparta_vbs_sddmm, so that
 * W -= lr * G on the caller's fp32 master copy followed by this call is one training step.  Every device image the handle holds is
 * rewritten on the device (fp32: the reference-layout image and the fragment image with its per-step k-compaction redone; 16-bit: the
 * slices of the stream plans and of the hub plan, rounded to nearest even exactly as creation rounds them); positions past `cols` in a
 * ragged last block column are stored as given.  After the call, in stream order, every entry behaves as if the handle had been created
 * from the new values; the plans and the autotune's choices stay as creation made them.
 * SPARTA_PTR_DEVICE: stream-ordered on `stream`, kernel launches only (no allocation, no synchronisation): it can be captured into a
 * hipGraph.  SPARTA_PTR_HOST: mab is a host array, staged through scratch the handle owns; the call returns when the copy is done.
 * *dt_ms (may be NULL) covers the kernels only and synchronises (refused with SPARTA_ERR_UNSUPPORTED while the stream is being captured).
 * SPARTA_ERR_UNSUPPORTED on a handle made without the flag (including sparta_vbs_create_from_csr and sparta_vbs_create_transposed);
 * SPARTA_ERR_INVALID on a NULL handle, or a NULL mab with nztot > 0. */
int sparta_vbs_set_values(sparta_vbs_t* A, const float* mab, int32_t ptr_space, void* stream, float* dt_ms);

/* One SGD step on the caller's fp32 master copy AND the update of the handle, in one pass: what `W -= lr * G; sparta_vbs_set_values(A, W)`
 * does, without reading W a second time.  Device pointers only.  W (the weights), G (the gradient, what sparta_vbs_sddmm writes) and M (the
 * momentum buffer) hold nztot floats each in the layout of sparta_vbs_host.mab (a range handle: the slice of its block-rows, from 0); they may
 * start on any 4-byte boundary and must not overlap.  M may be NULL exactly when cfg->momentum == 0 (it is then neither read nor written).
 * Per stored element i, every operation rounded once to fp32 in this order, never contracted into an FMA:
 *     g = G[i]
 *     if (grad_scale   != 1) g = g * grad_scale
 *     if (weight_decay != 0) g = g + (weight_decay * W[i])
 *     if (momentum     != 0) { m = (momentum * M[i]) + g;  M[i] = m;  g = m; }
 *     W[i] = W[i] - (lr * g)
 * -- torch.optim.SGD with dampening 0, no Nesterov, M starting as zeros; a float32 restatement on the host reproduces W and M bit for bit.
 * Each of the nztot elements is updated exactly once; positions past `cols` in a ragged last block column are elements like any other.
 * After the call, in stream order, every entry of the handle behaves exactly as if sparta_vbs_set_values(A, W_new) had run: the fp32 fragment
 * image (k-compaction redone from the zero pattern of the NEW values), the reference-layout image if held, the 16-bit stream, pair and hub
 * slices (rounded as creation rounds), the image of sparta_vbs_spmm_t.
 * Two forms, same results.  Where ONE image of the handle holds every stored element exactly once, the kernel that writes that image can do the
 * arithmetic in its registers (fp32: the fragment image of a handle without 33..64-row tiles; 16-bit: the slices of the only non-empty stream plan
 * of a handle without a hub plan, the pair tiles of 32-wide blocks among them); the remaining images are then written from the new W.  Otherwise one
 * elementwise kernel does the arithmetic and the launches of sparta_vbs_set_values follow.  Every step takes the first form where the handle allows
 * it (it measured faster); the environment variable SPARTA_SGD_FUSE=0, read at every call, asks for the second form on every
 * step.  sparta_vbs_step_info says which form the last step took.
 * Kernel launches only: no allocation, no synchronisation, capturable into a hipGraph from the first call.  *dt_ms (may be NULL) covers the
 * kernels and synchronises (SPARTA_ERR_UNSUPPORTED while the stream is being captured).
 * SPARTA_ERR_UNSUPPORTED on a handle made without SPARTA_CREATE_UPDATABLE (including sparta_vbs_create_from_csr and
 * sparta_vbs_create_transposed); SPARTA_ERR_INVALID on a NULL handle, a NULL W, G or cfg with nztot > 0, a NULL M with momentum != 0. */
typedef struct sparta_sgd_cfg { float lr, momentum, weight_decay, grad_scale; } sparta_sgd_cfg;
int sparta_vbs_sgd_step(sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, void* stream, float* dt_ms);

/* One Adam / AdamW step on the caller's fp32 master copy AND the update of the handle, in one pass.  Device pointers only.  W (the weights), G (the
 * gradient), M (exp_avg) and V (exp_avg_sq) hold nztot floats each in the layout of sparta_vbs_host.mab (a range handle: the slice of its
 * block-rows, from 0); they may start on any 4-byte boundary and must not overlap.  M and V are zeros before the first step.
 * S is the step state: 32 bytes of caller-owned device memory on a 4-byte boundary (checkpointing it is the caller's copy), zero-filled for a
 * fresh optimizer:
 *     S[0] int32  steps done, t            S[3] fp32  step_size of the last step
 *     S[1] fp32   running product of beta1 S[4] fp32  d of the last step
 *     S[2] fp32   running product of beta2 S[5..7]    written as zero
 * Every operation is rounded once to fp32 in the order written, never contracted into an FMA; division and square root are IEEE correctly
 * rounded.  Once per step, on the device, before any element is touched:
 *     if (t == 0) { p1 = beta1; p2 = beta2; } else { p1 = p1 * beta1; p2 = p2 * beta2; }
 *     t = t + 1
 *     bc1 = 1 - p1;  bc2 = 1 - p2;  step_size = lr / bc1;  d = sqrt(bc2)
 * Per stored element i, with omb1 = 1.0f - beta1, omb2 = 1.0f - beta2, dk = 1.0f - (lr * weight_decay) taken in fp32 on the host:
 *     g = G[i];                       if (grad_scale != 1) g = g * grad_scale
 *     if (weight_decay != 0 &&  decoupled) w = W[i] * dk        else w = W[i]
 *     if (weight_decay != 0 && !decoupled) g = g + (weight_decay * w)
 *     m = (beta1 * M[i]) + (omb1 * g);          M[i] = m
 *     v = (beta2 * V[i]) + (omb2 * (g * g));    V[i] = v
 *     den = (sqrt(v) / d) + eps
 *     W[i] = w - (step_size * (m / den))
 * decoupled = 1 is torch.optim.AdamW, decoupled = 0 torch.optim.Adam with L2 weight decay, both without amsgrad and without maximize; the running
 * products differ from torch's beta ** step by roundings only.  A float32 restatement on the host reproduces W, M, V and S bit for bit.
 * Each of the nztot elements is updated exactly once (positions past `cols` in a ragged last block column are elements like any other), and
 * after the call, in stream order, every entry of the handle behaves exactly as after sparta_vbs_set_values(A, W_new): every image
 * sparta_vbs_sgd_step lists.  The two forms are those of sparta_vbs_sgd_step, chosen by the same rule, each behind a one-wave kernel that advances
 * S; the environment variable SPARTA_ADAM_FUSE=0|1, read at every call, asks for the two-pass form on every step / for the image kernel wherever
 * the handle has one (the default is the form that measured faster).  sparta_vbs_step_info reports the form taken.
 * The step count is read and advanced on the device: the call can be captured into a hipGraph from the first call, and a replay advances t as
 * an eager call does.  lr and the other fields of cfg are call arguments and are BAKED INTO a capture (as sparta_vbs_sgd_step bakes its own): a
 * learning-rate schedule under capture needs a re-capture.
 * Kernel launches only: no allocation, no synchronisation.  *dt_ms (may be NULL) covers the kernels and synchronises (SPARTA_ERR_UNSUPPORTED
 * while the stream is being captured).
 * SPARTA_ERR_UNSUPPORTED on a handle made without SPARTA_CREATE_UPDATABLE; SPARTA_ERR_INVALID, with nothing launched, on a NULL handle, a NULL
 * W, G, M, V, S or cfg with nztot > 0, beta1 or beta2 outside [0, 1), eps <= 0, reserved != 0. */
typedef struct sparta_adam_cfg { float lr, beta1, beta2, eps, weight_decay, grad_scale; int32_t decoupled; int32_t reserved; } sparta_adam_cfg;
int sparta_vbs_adam_step(sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S,
                         const sparta_adam_cfg* cfg, void* stream, float* dt_ms);
/* info_out[4] = {1 if the last sparta_vbs_sgd_step / sparta_vbs_adam_step on the handle did the arithmetic inside an image kernel, 0 if it took
 * the two-pass form, -1 if no step has run yet; kernel launches of that step (an Adam step counts its tick); 1 if that step skipped dead blocks
 * (sparta_vbs_set_live_steps), else 0; 0}. */
int sparta_vbs_step_info(const sparta_vbs_t* A, int64_t* info_out);

/* Global-norm gradient clipping and loss scaling with skip-on-overflow, decided on the device: between backward and step nothing comes back to the
 * host, and the sequence [sparta_grad_stats ..., sparta_grad_ctl_finish, sparta_vbs_*_step_ctl ...] is kernel launches only, capturable into a hipGraph
 * from the first call; a replay reads the gradients and the record afresh (one whose gradient has become non-finite skips).
 * R, the control record: SPARTA_GRAD_CTL_BYTES of caller-owned device memory on an 8-byte boundary, zero-filled for a fresh run (checkpointing words
 * 4, 5 and 9 is the caller's copy).  The first 64 bytes, as 32-bit words:
 *     0-1  fp64   ssq: sum of squares of the FINITE gradient elements folded in so far
 *     2    int32  nonfinite: number of Inf / NaN elements folded in, saturating at 2^31 - 1
 *     3           zero
 *     4    fp32   loss_scale (a zero word means 1.0f)          7  fp32   coef the steps multiply G by
 *     5    int32  growth_tracker                               8  int32  skip (0 / 1)
 *     6    fp32   norm of the last finish (unscaled)           9  int32  skipped_total
 *     10-15       written as zero by sparta_grad_ctl_finish
 * The rest is scratch of the reduction (the partial sums of its largest grid) with unspecified content: no call allocates.
 *
 * sparta_grad_stats folds the n floats of G (device memory, any 4-byte boundary; NULL allowed when n == 0) into words 0-2: accumulate = 0 overwrites
 * them (also with n == 0: zeros), 1 adds to them.  Handle-free, as sparta_pack_blocks: a global norm spans the dense parameters of a model too.  Each
 * finite element is widened to fp64 and squared there (exact), and the squares are summed in fp64; an Inf or NaN is counted and adds nothing to ssq.
 * The grid is a function of n alone -- one workgroup per SPARTA_GRAD_STATS_CHUNK elements, at most SPARTA_GRAD_STATS_MAX_GRID, which walk the chunks
 * round-robin -- the partials are summed in a fixed order by a second, one-workgroup launch, and no floating-point atomic is used: the three words are
 * bit-identical from run to run and between an eager call and a replay (for the same n and the same alignment of G modulo 16 bytes), and ssq differs from
 * the exact sum of the squares by at most n * 2^-53 * ssq.  Kernel launches only (on the current device); *dt_ms (may be NULL) covers them and
 * synchronises (SPARTA_ERR_UNSUPPORTED while the stream is being captured).  SPARTA_ERR_INVALID for a NULL or misaligned R, a NULL G with n > 0, n < 0.
 *
 * sparta_grad_ctl_finish turns the statistics into the coefficient and the skip flag and moves the loss scale -- clip_grad_norm_'s coefficient and
 * GradScaler.update()'s rule -- in a one-wave kernel.  Every fp32 operation is rounded once, in this order, never contracted into an FMA; division and
 * square root are IEEE correctly rounded:
 *     s = loss_scale (1.0f if the word is 0);  inv = 1.0f / s
 *     bad  = nonfinite != 0
 *     root = (float) sqrt(ssq)                  -- fp64 square root, then rounded to fp32; may be +Inf
 *     norm = root * inv;                        if (!isfinite(norm)) bad = 1
 *     coef = inv
 *     if (!bad && max_norm > 0) { c = max_norm / (norm + 1e-6f);  if (c < 1.0f) coef = inv * c; }
 *     if (bad) coef = 0.0f
 *     skip = bad;  skipped_total += skip
 *     if (growth_interval > 0) {
 *         if (skip) { s = s * backoff_factor;  growth_tracker = 0; }
 *         else { growth_tracker += 1;
 *                if (growth_tracker >= growth_interval) { s2 = s * growth_factor;  if (isfinite(s2)) s = s2;  growth_tracker = 0; } }
 *     }
 *     write loss_scale = s, growth_tracker, norm, coef, skip, skipped_total; words 10..15 = 0
 * coef is taken with the scale the gradients were produced under; the scale moves afterwards.  max_norm = 0: no clipping; growth_interval = 0: the loss
 * scale stays.  SPARTA_ERR_INVALID, with nothing launched, for a NULL or misaligned R, a NULL cfg, max_norm negative or NaN, growth_interval < 0, with
 * growth_interval > 0 a growth_factor < 1 or a backoff_factor outside (0, 1], any non-zero reserved word.
 *
 * sparta_vbs_sgd_step_ctl / sparta_vbs_adam_step_ctl are sparta_vbs_sgd_step / sparta_vbs_adam_step with the record R in front of `stream`.  R == NULL
 * is the plain entry exactly (which calls these with NULL).  With R != NULL the kernels of the step read coef and skip from R on the device, at every
 * launch and replay:
 *     per element, after the optional g = g * grad_scale:   g = g * coef     (always, one rounding; the rest of the pinned order is unchanged)
 * so a float32 restatement given the coef read back from R reproduces W, M, V and S bit for bit.  With skip != 0: W, M, V and S keep their bits (the
 * Adam step count does not advance), and every image of the handle is still written, from W: afterwards the handle behaves as after
 * sparta_vbs_set_values(A, W), whatever values it held before.  The flag selects -- G is not read, nothing is multiplied by zero -- so nothing
 * non-finite in G reaches W, M, V or an image.  Both forms of a step honour it; the routing rule, SPARTA_SGD_FUSE / SPARTA_ADAM_FUSE and
 * sparta_vbs_step_info are those of the plain entries, launch counts included.  A misaligned R: SPARTA_ERR_INVALID with nothing launched. */
#define SPARTA_GRAD_CTL_BYTES 16448
#define SPARTA_GRAD_STATS_CHUNK 4096
#define SPARTA_GRAD_STATS_MAX_GRID 1024
typedef struct sparta_grad_ctl_cfg {
    float max_norm, growth_factor, backoff_factor;
    int32_t growth_interval;
    int32_t reserved[4];
} sparta_grad_ctl_cfg;
int sparta_grad_stats(const float* G, int64_t n, void* R, int32_t accumulate, void* stream, float* dt_ms);
int sparta_grad_ctl_finish(void* R, const sparta_grad_ctl_cfg* cfg, void* stream);
int sparta_vbs_sgd_step_ctl(sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, const void* R, void* stream, float* dt_ms);
int sparta_vbs_adam_step_ctl(sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S,
                             const sparta_adam_cfg* cfg, const void* R, void* stream, float* dt_ms);

/* The epilogue of a block-sparse linear layer: bias, activation and the output type in ONE pass behind the forward product (sparta_epilogue_fwd), and in ONE
 * pass in front of the two backward products (sparta_epilogue_bwd), which writes their operand dZ in the handle's type and the bias gradient.  Handle-free,
 * as sparta_grad_stats: device pointers only, on the current device.  Every operand is a column-major rows x n_cols matrix with a leading dimension
 * (element (i, j) at j * ld + i) -- the layout of C of sparta_vbs_spmm and of X of sparta_vbs_spmm_t / sparta_vbs_sddmm; Z is fp32, y_dtype / dy_dtype /
 * dz_dtype are SPARTA_F32, SPARTA_F16 or SPARTA_BF16; bias (rows floats, may be NULL) is indexed by the row.  Bases and leading dimensions are arbitrary
 * (aligned to the element size, ld >= rows); offsets are 64-bit.  Where every operand is 16-byte aligned at the same row of every column (the bases agree
 * modulo four elements and every ld is a multiple of 4) a lane takes four consecutive rows per access, the rows in front and behind one by one; otherwise all
 * rows go one by one.  The results do not depend on which.
 *
 * THE ARITHMETIC, per element, every fp32 operation rounded once in the order written, nothing contracted into an FMA; 16-bit inputs are widened exactly and
 * 16-bit outputs rounded to nearest even (a bf16 NaN keeps its sign and gets the quiet bit):
 *     u = Z[i,j] + bias[i]                      (u = Z[i,j] when bias == NULL: no addition)
 *     SPARTA_ACT_NONE   y = u                                            dz = dy
 *     SPARTA_ACT_RELU   y = (u <= 0) ? +0.0f : u   (a NaN passes)        dz = (u <= 0) ? +0.0f : dy     (a select: a NaN in dy under a masked position is dropped)
 *     SPARTA_ACT_GELU   e = erff(u * 0.70710678f)                        (the erf form, torch's default)
 *                       y = (0.5f * u) * (1.0f + e)
 *                       dz = dy * (0.5f * (1.0f + e) + (u * expf((-0.5f * u) * u)) * 0.39894228f)
 * erff and expf are the device library's; everything else can be restated in numpy float32 bit for bit (tests/_epilogue.py).
 * THE BIAS GRADIENT: dbias[i] = the sum over j of the fp32 dz[i,j] BEFORE its rounding to dz_dtype, each widened to fp64.  The order is fixed: the columns go
 * in consecutive runs of SPARTA_EPILOGUE_RUN; inside a run the sum is sequential in fp64, j ascending, starting from 0.0; the run sums are added
 * sequentially in ascending run order; the result is rounded once to fp32.  No floating-point atomic, no shuffle tree: dbias is a function of (rows, n_cols,
 * data) alone -- not of the grid, the device, the alignment of the operands, eager or replayed.  With more than one run the run sums pass through `scratch`
 * (sparta_epilogue_scratch_bytes(rows, n_cols) bytes of caller-owned device memory on an 8-byte boundary, content unspecified before and after; 0 bytes when
 * one run covers n_cols) and a second, fixed-order launch adds them.  dbias == NULL skips the sums, and scratch is then unused.
 *
 * WHAT AN OUTPUT ELEMENT DEPENDS ON (Inf and NaN are ordinary data):
 *   Y[i,j] depends on Z[i,j] and bias[i] only.
 *   dZ[i,j] depends on dY[i,j], Z[i,j] and bias[i] only (with SPARTA_ACT_NONE on dY[i,j] only: Z may be NULL then, and neither Z nor bias is read).
 *   dbias[i] depends on row i of dY, Z and on bias[i] only; nothing accumulates into the previous content of dbias or scratch.
 *   The elements [rows, ld) of a column of any operand are neither read into a result nor written.
 * IN PLACE: Y == Z is allowed with y_dtype == SPARTA_F32 and ldy == ldz; dZ == dY with dz_dtype == dy_dtype and lddz == lddy.  Any other overlap of an
 * output with an operand is undefined.
 * The entries launch kernels only -- no allocation, no synchronisation -- and can be captured into a hipGraph from the first call.  *dt_ms (may be NULL)
 * covers the kernels and synchronises (SPARTA_ERR_UNSUPPORTED while the stream is being captured).  rows == 0 or n_cols == 0 returns SPARTA_OK; with
 * n_cols == 0 and dbias != NULL, dbias gets rows times +0.0f.  SPARTA_ERR_INVALID, with nothing launched and a message that names the entry, for a negative
 * size, an unknown act or dtype, ld < rows, a NULL Z (unless SPARTA_ACT_NONE in backward), Y, dY or dZ with rows and n_cols > 0, a pointer not aligned to
 * its element size, a NULL (or not 8-byte aligned) scratch when sparta_epilogue_scratch_bytes > 0 and dbias != NULL. */
#define SPARTA_ACT_NONE 0
#define SPARTA_ACT_RELU 1
#define SPARTA_ACT_GELU 2
#define SPARTA_EPILOGUE_RUN 32
int sparta_epilogue_fwd(const float* Z, int64_t ldz, const float* bias, int32_t act,
                        void* Y, int64_t ldy, int32_t y_dtype, int64_t rows, int64_t n_cols, void* stream, float* dt_ms);
int sparta_epilogue_scratch_bytes(int64_t rows, int64_t n_cols, int64_t* bytes_out);   /* may be 0 */
int sparta_epilogue_bwd(const void* dY, int64_t lddy, int32_t dy_dtype, const float* Z, int64_t ldz, const float* bias, int32_t act,
                        void* dZ, int64_t lddz, int32_t dz_dtype, float* dbias, void* scratch,
                        int64_t rows, int64_t n_cols, void* stream, float* dt_ms);

/* Block pruning: a score per stored block, and chosen blocks made zero -- and kept zero -- in the weights, the optimizer state and the gradient.
 * The stored blocks of the block-rows [block_row_begin, block_row_end) are numbered in mab order: block-row by block-row, inside a block-row in jab order.
 * sparta_vbs_block_table_host (pure host code, no GPU) writes four words per block:
 *     [0] the element offset of the block into the range's slice of mab
 *     [1] n_in  = h * min(w, cols - jb * w): the elements inside the matrix -- a block is column-major h x w, so these are its FIRST n_in elements
 *     [2] n_all = h * w
 *     [3] (ib - block_row_begin) << 32 | jb: the block-row, numbered from the start of the range, and the block column
 * Blocks of a block-row of height 0 are listed, with n_in = n_all = 0: block b is entry b of the range's jab.  table_out == NULL only counts.  The table a
 * handle uploads for the two device entries below is built by the function behind this entry.  sparta_vbs_block_count: the blocks of a handle.
 *
 * sparta_vbs_block_ssq / sparta_vbs_mask_blocks: device pointers only.  W and T0..T3 hold nztot floats each in the layout of sparta_vbs_host.mab (a range
 * handle: the slice of its block-rows, from 0) and may start on any 4-byte boundary; ssq_out holds n_blocks fp64 values (8-byte aligned), keep n_blocks
 * bytes.  Every handle made from VBS arrays takes them (sparta_vbs_create, _create_range, _create_range_ex with any flags, all three dtypes); neither reads
 * or writes an image of the handle -- to make a handle multiply with masked values, follow with sparta_vbs_set_values or a step.  Handles of
 * sparta_vbs_create_from_csr / sparta_vbs_create_transposed: SPARTA_ERR_UNSUPPORTED.  SPARTA_ERR_INVALID, with nothing launched, for a NULL handle, a NULL
 * ssq_out or keep with n_blocks > 0, a NULL W with nztot > 0, a misaligned pointer.  n_blocks == 0 succeeds and launches nothing.  The FIRST call of either
 * entry on a handle builds and uploads the table (16 bytes per block); every later call is one kernel launch, no allocation, no synchronisation, and can
 * be captured into a hipGraph -- a first call while the stream is being captured returns SPARTA_ERR_UNSUPPORTED, as does *dt_ms != NULL under capture
 * (dt_ms covers the kernel and synchronises).  Blocks of 2^31 or more elements: SPARTA_ERR_UNSUPPORTED.
 *
 * block_ssq: ssq_out[b] = the sum of the squares of the block's first n_in elements of W; stored positions past `cols` in a ragged last block column take
 * no part, whatever they hold.  Each element is widened to fp64 and squared there (exact), the squares are summed in fp64 by ONE wave per block in a fixed
 * order (per lane a head up to the block's first 16-byte boundary, 16-byte loads, a tail; lanes by xor-shuffle), no atomics, one launch: bit-identical from
 * run to run and between an eager call and a replay for the same alignment of W modulo 16 bytes, and within n_in * 2^-53 * ssq of the exact sum -- the bound
 * of any order of additions of non-negative terms, valid for n_in < 2^26 (n_in * 2^-53 must stay far below 1 for the first-order bound to hold).  Plain IEEE
 * arithmetic: an Inf or NaN inside the matrix gives that block a non-finite score.  n_in == 0 gives 0.0.
 *
 * mask_blocks: for every block with keep[b] == 0, all n_all elements (the positions past `cols` included) are stored as +0.0f in each non-NULL T; the old
 * content is not read (an Inf or NaN there is gone).  Blocks with keep[b] != 0 are neither read nor written: their bits, and every byte outside the
 * tensors, stay.  All four T NULL: valid, nothing launched.  The tensors must not overlap each other or keep.
 * A zero block stays zero under sparta_vbs_sgd_step / sparta_vbs_adam_step when its gradient is masked too: with W = M = V = +0 and g = +-0 the pinned
 * arithmetic above gives W = +0 again, with or without momentum and either kind of weight decay. */
int sparta_vbs_block_table_host(int64_t cols, int64_t block_rows, int64_t block_col_size, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab,
                                int64_t block_row_begin, int64_t block_row_end, int64_t* table_out /* [n_blocks][4] */, int64_t* n_blocks_out);
int sparta_vbs_block_count(const sparta_vbs_t* A, int64_t* n_blocks_out);
int sparta_vbs_block_ssq(sparta_vbs_t* A, const float* W, double* ssq_out, void* stream, float* dt_ms);
int sparta_vbs_mask_blocks(sparta_vbs_t* A, const uint8_t* keep, float* T0, float* T1, float* T2, float* T3, void* stream, float* dt_ms);

/* The live-block set of a handle: which of its stored blocks the two backward products (sparta_vbs_sddmm, sparta_vbs_spmm_t) still compute.  The pattern, the
 * images and every other entry stay as they are (the contract: "WITH A LIVE-BLOCK SET INSTALLED" above).
 *
 * sparta_vbs_set_live_blocks: keep = n_blocks device bytes in the numbering of sparta_vbs_mask_blocks (mab order, blocks of block-rows of height 0 included,
 * a range handle: the numbering of its range); keep[b] == 0: block b is dead.  The handle takes a snapshot in stream order: later writes to the caller's keep
 * have no effect until the next call.  keep == NULL removes the live set (host state only, nothing launched): from then on the handle launches the kernels
 * and lists it launched before one was installed.  Takes every handle sparta_vbs_mask_blocks takes (others: SPARTA_ERR_UNSUPPORTED); without
 * SPARTA_CREATE_TRANSPOSE only the SDDMM half is built.  The FIRST call with keep != NULL builds and uploads pattern-only helper arrays (the block table, the
 * map from positions of the block-column index to block numbers, about 40 bytes per block) and returns SPARTA_ERR_UNSUPPORTED while the stream is being
 * captured; every later call is two kernel launches (one without SPARTA_CREATE_TRANSPOSE), no allocation, no synchronisation, capturable -- a replay reads
 * keep again.  WHETHER a live set is installed is host state, decided when sparta_vbs_sddmm / _spmm_t is called (or captured); its CONTENT is device state in
 * stream order, as the values after sparta_vbs_set_values are.  With a live set sparta_vbs_sddmm with accumulate = 0 is two launches (the zeros of the dead
 * blocks, then the product).  sparta_vbs_destroy frees everything.
 *
 * The lists (written by stable compaction -- ballot and prefix count, one wave per block-row / block column, no atomics: a function of keep alone):
 *   sd_groups[SDDMM groups], sd_count[block_rows]: group g of a block-row is its stored columns 32 g .. 32 g + 31 (mab order, nb * w of them; a block-row of
 *     height 0 has no groups); it is live iff one of the blocks it overlaps is.  Block-row ib owns the slice of sd_groups that starts at the sum of the group
 *     counts of the block-rows before it: its live group numbers in ascending order, sd_count[ib] of them, then -1.  Work item (block-row, tile of rows, g0)
 *     of sparta_vbs_sddmm takes positions g0 .. g0 + 15 of the slice.
 *   t_blocks[spmm_t list entries], t_count[block columns]: the list of block column jb is its blocks of height > 0 in block-row order; its slice starts at
 *     the sum of the list lengths of the block columns before it and holds the block numbers of its live blocks in that order, t_count[jb] of them, then -1.
 * sparta_vbs_live_info: info_out[8] = {installed, n_blocks, live blocks, SDDMM groups, live SDDMM groups, spmm_t list entries, live spmm_t list entries, the
 * live-steps switch}, the live counts read back from the device (words 2..6 are 0 when no live set is installed, words 5, 6 without SPARTA_CREATE_TRANSPOSE).
 * sparta_vbs_live_lists_get: the lists the kernels walk, downloaded (host pointers; any of the four may be NULL); SPARTA_ERR_INVALID without a live set.  Both
 * synchronise the stream and are refused under capture; they are for tests and records.
 * sparta_vbs_live_lists_host: the same rule as host code (no GPU) on VBS arrays and a host keep, arguments as sparta_vbs_block_table_host; any of the four
 * outputs may be NULL (info_out[3] and [5] give the sizes). */
int sparta_vbs_set_live_blocks(sparta_vbs_t* A, const uint8_t* keep, void* stream);
/* sparta_vbs_sddmm_block_ssq: the block scores of X * Y^T on the stored blocks, without G -- what sparta_vbs_block_ssq would give on the G of
 * sparta_vbs_sddmm, for the blocks `sel` selects, in one pass that writes one fp64 partial per (32-row tile, stored column) instead of nztot floats.  Device
 * pointers only.  X, ldx, Y, ldy, k: the operands of sparta_vbs_sddmm; sel: n_blocks device bytes in the numbering of sparta_vbs_block_ssq / _mask_blocks (mab
 * order, blocks of block-rows of height 0 included, a range handle: the numbering of its range), or NULL = every block; ssq_out: n_blocks doubles.  Takes every
 * handle that both sparta_vbs_sddmm and sparta_vbs_block_ssq take, all three types, any creation flags (handles of sparta_vbs_create_from_csr / _transposed:
 * SPARTA_ERR_UNSUPPORTED).  SPARTA_ERR_INVALID, nothing launched: a NULL handle; X, Y or ssq_out NULL with n_blocks > 0; k <= 0; ssq_out not 8-byte aligned;
 * ldx < rows, ldy < cols, an odd ldx or ldy on a 16-bit handle.  n_blocks == 0 succeeds and launches nothing.  THE CONTRACT:
 *   - a SELECTED block (sel == NULL or sel[b] != 0): ssq_out[b] = the fp64 sum of the exact fp64 squares of the block's n_in elements inside the matrix, the
 *     elements being exactly the fp32 values sparta_vbs_sddmm(accumulate = 0) stores for the block on a handle without a live set (the same kernel body: the
 *     same MFMA sequence over k, the same accumulator bits).  Positions past `cols` contribute nothing.  The order of the sum is fixed per handle and sel: rows
 *     of a tile by xor-shuffle, then the block's (tile, column) partials 64 apart per lane in tile-major order, then the lanes by xor-shuffle.  Bit-identical
 *     from run to run, no atomics, plain IEEE: an Inf or NaN inside the block makes that block's score non-finite and no other;
 *   - an UNSELECTED block: ssq_out[b] = +0.0, written on every call.  Neither Y's rows nor, on its behalf alone, X's rows are read for it: the dependency rule
 *     of a dead block of the live SDDMM ("WITH A LIVE-BLOCK SET INSTALLED" above);
 *   - blocks of a block-row of height 0 score +0.0;
 *   - the result does not depend on whether a live set is installed or on what it holds, and the call changes neither the live set, the live-steps switch, the
 *     live-forward switch nor any image: it walks lists of its own, written from sel by the kernel of sparta_vbs_set_live_blocks;
 *   - the FIRST call on a handle builds and uploads pattern-only helpers (those of the live set, a slot offset per block-row, 24 bytes per block) and allocates
 *     its scratch (8 bytes per (32-row tile, stored column) of the pattern); under capture it returns SPARTA_ERR_UNSUPPORTED.  Every later call is three
 *     launches (the lists of sel, the product, one wave per block for the final sums): no allocation, no synchronisation, capturable; a replay reads X, Y and
 *     sel again.  dt_ms spans all three (and synchronises: refused under capture). */
int sparta_vbs_sddmm_block_ssq(sparta_vbs_t* A, const void* X, int64_t ldx, const void* Y, int64_t ldy, int32_t k, const uint8_t* sel, double* ssq_out, void* stream,
                               float* dt_ms);
/* Live steps: with enable != 0 and a live set installed, sparta_vbs_sgd_step / _adam_step and their _ctl forms skip the dead blocks (the contract: "WITH A
 * LIVE-BLOCK SET INSTALLED AND LIVE STEPS ON" above).  Opt-in, off at creation.  The switch is host state, read when a step is called (or captured); it has an
 * effect only while a live set is installed: sparta_vbs_set_live_blocks(A, NULL, ...) puts the steps back on the plain kernels without clearing it, and the
 * next live set switches them over again.  sparta_vbs_step_info word 2 says what the last step did, sparta_vbs_live_info word 7 is the switch.
 * On a set that prunes nothing a live step moves the bytes of the plain one: it measured the same, there is nothing to gain.
 * The FIRST enabling call builds and uploads pattern-only helper arrays (the arrays of the live set if no set was ever installed; on a handle with a fused
 * image one 32-bit map entry and one 32-bit word per step of the fp32 one-tile plan / two per 16-bit slice) and returns SPARTA_ERR_UNSUPPORTED while the
 * stream is being captured.  If a set is installed the call launches, on `stream`, the kernel that derives the image kernel's words from the snapshot; from then
 * on every sparta_vbs_set_live_blocks adds that one launch (none on a handle without a fused image: the two-pass form walks the block table with the snapshot
 * itself).  No allocation, no synchronisation, capturable after the first call; a replay of set_live_blocks re-reads keep.  enable == 0: host state only.
 * SPARTA_ERR_UNSUPPORTED on a handle made without SPARTA_CREATE_UPDATABLE and on every handle sparta_vbs_set_live_blocks refuses; SPARTA_ERR_INVALID on NULL. */
int sparta_vbs_set_live_steps(sparta_vbs_t* A, int32_t enable, void* stream);
/* Live forward: with enable != 0 and a live set installed, the 16-bit forward product walks only the steps of live blocks (the contract: "WITH A LIVE-BLOCK
 * SET INSTALLED AND LIVE FORWARD ON" above).  Opt-in, off at creation; the plain kernels and the plain records are untouched.  The switch is host state, read
 * when sparta_vbs_spmm is called (or captured), and acts only while a live set is installed.  Needs SPARTA_CREATE_UPDATABLE (the map from steps to blocks is
 * the one of the live steps): SPARTA_ERR_UNSUPPORTED otherwise, and on every handle sparta_vbs_set_live_blocks refuses.
 * Which handles take the live form: 16-bit handles with ONE stream image and no hub plan whose block width is a multiple of 32 (the handles with a fused step
 * image).  fp32 handles (their forward product follows sparta_vbs_set_values by itself), handles with a hub plan or two stream images and other block widths
 * accept the switch and keep the plain kernels; so do, on a handle that qualifies, a gathered B, SPARTA_H16_AHEAD=7 and SPARTA_H16_PATH=lds.  Word 1 and
 * words 2, 3 of sparta_vbs_live_forward_info say so.
 * The FIRST enabling call builds and uploads pattern-only helper arrays (those of the live set and the word map if they do not exist yet; a second copy of
 * the stream image's step records, 32 bytes per step, a second range array and 4 bytes per step that say where its tile piece ends) and returns
 * SPARTA_ERR_UNSUPPORTED while the stream is being captured.  If a set is installed the call launches, on `stream`, the word kernel and the compaction kernel;
 * from then on every sparta_vbs_set_live_blocks adds those launches.  No allocation, no synchronisation, capturable after the first call.
 * The rule (one wave per worker range, ballot and prefix count, no atomics: a function of the snapshot alone; sparta_live_forward_compact is the same rule
 * as host code on arrays): a SEGMENT is the run of records of a range up to and including the next STEP_LAST record -- what one worker owns of a tile.  A
 * step is live iff a present half of it (rows 0..31 / 32..63 of its slice) lies in a live block.  Per range, over the same positions: the kept steps first,
 * in order -- every live step, and the first step of a segment without one -- then the dropped steps, unchanged and in order; the live range is (begin,
 * begin + kept).  A kept record keeps its slice offset, its rows of B and its tail flag; the first kept step of a segment carries STEP_FIRST, the last one
 * STEP_LAST and the segment's epilogue fields (split flag, slot, first row of C, tile rows); a dead half gets its absent flag, the kept step of a segment
 * without a live step is marked dead as a whole (one-tile records: the lower absent flag, pair tiles: both) -- its epilogue still runs and writes zeros.
 * Ranges stay as creation balanced them: the worker with the most kept steps bounds the kernel.
 * sparta_vbs_live_forward_info: info_out[8] = {the switch, which stream image has the live form (0: none, 1: the <= 32-row tiles, 2: the 64-row / pair tiles), the form the last 16-bit product ran on the
 * image of <= 32-row tiles and on the image of 64-row / pair tiles (0: none yet, 1: plain, 2: live), steps of the image with the live form, kept steps (read
 * back; 0 without a live set or before the first enabling call), split tiles, ranges}.
 * sparta_vbs_live_forward_lists_get: host pointers, any may be NULL -- the plain records [steps][32 bytes] and ranges [ranges][2], the two live bits of every
 * step [steps][2], the compacted records and the live ranges.  SPARTA_ERR_INVALID without a live set, SPARTA_ERR_UNSUPPORTED on a handle without the lists.
 * Both synchronise the stream and are refused under capture; they are for tests and records.
 * sparta_live_forward_compact: `steps` = n_steps records of 32 bytes {int64 a_off; int32 b_row, h, c_row, mt_flags, slot, pad}, ranges = n_ranges disjoint
 * (begin, end) pairs, pair_image != 0: the records are 64-row / pair tiles (two halves, absent flags 1 << 27 / 1 << 28), else one-tile records (live[2 q]
 * alone counts); info_out[8] = {steps in ranges, kept, segments, segments without a live step, most kept steps of a range, fewest, 0, 0}. */
int sparta_vbs_set_live_forward(sparta_vbs_t* A, int32_t enable, void* stream);
int sparta_vbs_live_forward_info(sparta_vbs_t* A, int64_t* info_out /* [8] */, void* stream);
int sparta_vbs_live_forward_lists_get(sparta_vbs_t* A, void* steps_plain, int32_t* ranges_plain, uint8_t* live_bits, void* steps_live, int32_t* ranges_live,
                                      void* stream);
int sparta_live_forward_compact(const void* steps, int64_t n_steps, const int32_t* ranges, int64_t n_ranges, int32_t pair_image, const uint8_t* live /* [n_steps][2] */,
                                void* steps_out, int32_t* ranges_out, int64_t* info_out /* [8] */);
/* THE FP8 WEIGHT IMAGE (sparta_vbs_set_forward_a8): with the switch on, sparta_vbs_spmm on a 16-bit handle multiplies with an OCP e4m3 image of A -- one byte
 * per stored element and one power-of-two scale per group -- widened to the handle's 16-bit type in registers (v_cvt_scalef32_pk_{f16,bf16}_fp8), right in
 * front of the MFMAs the plain kernel issues.  Plans, records, B, accumulation order and epilogue are those of the plain product.  Everything else -- spmm_t,
 * sddmm, block_ssq, the live set, the steps -- keeps reading the 16-bit image: a forward under the switch with a backward on the 16-bit image of the same
 * values is quantisation-aware training, straight-through.  Opt-in, off at creation; with the switch off launches and results are what they were.
 * THE RULE.  A GROUP is one half of one slice of the stream image: the <= 32 rows x KP (32 or 64) values of a stored block that one step multiplies.  Every
 * stored element lies in exactly one group; image positions no stored element maps to hold code 0 and belong to no group.  For a group with fp32 values v:
 *   amax = the largest |v| over the FINITE elements (0 for a group of zeros or of nothing finite);
 *   e    = 0 if amax == 0; else with amax = m * 2^x, m in [0.5, 1): e = x - 9 if m <= 0.875, else x - 8 -- the smallest e with amax * 2^-e <= 448 -- clamped
 *          to [-126, 127] (no finite fp32 reaches the upper clamp); the scale is the fp32 2^e;
 *   code = v * 2^-e (one fp32 multiplication, exact) rounded to nearest even to e4m3fn: subnormals and the sign of zero kept, nothing exceeds 448 by
 *          construction; NaN and +-Inf become the NaN code with their sign (0x7F / 0xFF) -- e4m3fn has no Inf, AN Inf WEIGHT BECOMES NaN UNDER THE SWITCH;
 *   the value the product multiplies = code x 2^e in the handle's type as the conversion instruction gives it: exact whenever representable -- bf16 always,
 *          outside bf16 subnormals; f16 for -15 <= e <= 7 -- and the instruction's rounding otherwise.
 * The rounding is integer code on both sides; sparta_a8_quantize_group is the rule on the host for one group: v[k * ld + r] = row r < rows <= 32 of column
 * k < kcols (32 or 64), codes[k * rows + r], *e_out = e.  It needs no device.
 * sparta_vbs_set_forward_a8: the handle must be 16-bit, made with SPARTA_CREATE_UPDATABLE, and hold every stored element exactly once in ONE stream image (no
 * hub plan, no second image, a block width that is a multiple of 32: the handles that take the live forward form); every other handle -- fp32, not updatable,
 * made by sparta_vbs_create_from_csr / sparta_vbs_create_transposed -- gets SPARTA_ERR_UNSUPPORTED: the switch is never accepted and ignored.  Live forward
 * and the fp8 image do not combine: enabling one while the other is on is SPARTA_ERR_UNSUPPORTED.  The FIRST enabling call allocates the image (half the bytes
 * of the 16-bit image) and a private copy of the image's step records (32 bytes per step; the group exponents live in their last word) and is refused while
 * the stream is being captured; later calls are host state.  The image is INVALID until the next write of values: while the switch is on
 * sparta_vbs_set_values, sparta_vbs_sgd_step and sparta_vbs_adam_step (fused and two-pass forms, with and without a control record; a skipped step too) each
 * append ONE launch of the quantise kernel on the W / mab they were given, in stream order -- no allocation, capturable, a replay requantises -- so a valid
 * image is always the rule applied to the current values.  With a valid image sparta_vbs_spmm takes the a8 kernels (any n_cols, either layout of C); with an
 * invalid one, a gathered B, SPARTA_H16_AHEAD=7 or SPARTA_H16_PATH=lds it takes the plain kernels on the 16-bit image.  Switching off invalidates the image.
 * sparta_vbs_a8_info: info_out[8] = {the switch, the image is valid, which stream image has the form (0: none, 1: the <= 32-row tiles, 2: the 64-row / pair
 * tiles), the form the last 16-bit product ran on the image of <= 32-row tiles and on the image of 64-row / pair tiles (0: none yet, 1: plain, 2: live,
 * 3: a8, 4: a8 on the live records, sparta_vbs_set_a8_live), groups (one per 32-row slice, two per 64-row slice), bytes of the fp8 image (0 before the first enabling call), quantise launches so far}.
 * sparta_vbs_a8_get: host pointers to nztot elements each in mab order, any may be NULL -- the code of every stored element, its group's exponent, its group's
 * number (pattern only).  Synchronises the stream, refused under capture, SPARTA_ERR_UNSUPPORTED before the first enabling call; for tests and records. */
int sparta_vbs_set_forward_a8(sparta_vbs_t* A, int32_t enable, void* stream);
int sparta_vbs_a8_info(sparta_vbs_t* A, int64_t* info_out /* [8] */, void* stream);
int sparta_vbs_a8_get(sparta_vbs_t* A, uint8_t* codes, int32_t* exps, int32_t* group, void* stream);
int sparta_a8_quantize_group(const float* v, int64_t ld, int32_t rows, int32_t kcols, uint8_t* codes, int32_t* e_out);
/* THE FP8 IMAGE WITH A LIVE-BLOCK SET (sparta_vbs_set_a8_live): a third switch, for the combination the two above refuse.  sparta_vbs_set_live_forward governs
 * the product on the 16-bit image, sparta_vbs_set_forward_a8 selects the fp8 image, and this switch says that the product on the fp8 image skips dead blocks.
 * With the fp8 switch on and its image valid, this switch on and a live set installed, sparta_vbs_spmm walks the compacted records and live ranges of live
 * forward (the rule under sparta_vbs_set_live_forward) on the e4m3 image:
 *   a dead block contributes nothing to C, whatever W, the codes or the exponents hold for it; neither its codes nor, on its behalf, the rows of B are read;
 *   rows of C reached only through dead blocks are +0.0 (accumulate: unchanged);
 *   C equals bit for bit the live forward product of a plain handle with the same live set that was given the dequantised values, and -- the sign of a zero
 *   aside -- the product under sparta_vbs_set_forward_a8 alone on values whose dead blocks are zero.
 * Enabling needs the fp8 switch ON: SPARTA_ERR_UNSUPPORTED otherwise (so on every handle sparta_vbs_set_forward_a8 refuses).  The handles are those of the fp8
 * image, which are those of the live forward form: no new class.  The FIRST enabling call builds what live forward's first call builds, where it does not exist
 * yet (the word map, the segment ends, the second record and range arrays -- the same arrays), and is refused while the stream is being captured; later calls
 * are host state plus launches.  If a set is installed the call launches the word kernel, the compaction kernel and the scale-placement kernel, so that the
 * next product is right.  While the switch is on, ONE launch of the scale-placement kernel follows every compaction (sparta_vbs_set_live_blocks) and every
 * quantise launch (every write of values): position p of the compacted records then holds, in its last word, the exponents of the slice its a_off names.  No
 * allocation, no synchronisation, capturable.  The quantise kernel keeps covering every slice, dead ones included: switching off leaves a complete fp8 image.
 * Off at creation.  sparta_vbs_set_forward_a8(A, 0) clears this switch too.  sparta_vbs_set_live_forward(A, 1) stays refused while the fp8 switch is on,
 * whatever this switch says.  The product takes the plain kernels on the 16-bit image with an invalid fp8 image, a gathered B, SPARTA_H16_AHEAD=7 or
 * SPARTA_H16_PATH=lds, and the a8 kernels on every block without a live set; with this switch off launches and results are what they were.  The form fields
 * of sparta_vbs_a8_info and sparta_vbs_live_forward_info say 4 for this form.
 * sparta_vbs_a8_live_info: info_out[8] = {the switch, active (fp8 switch on and image valid, this switch on, a live set installed), which stream image has the
 * form (0: none, 1: the <= 32-row tiles, 2: the 64-row / pair tiles), its steps, kept steps (read back: synchronises the stream and is refused under capture
 * when a set is installed and the lists exist; else 0), launches of the scale-placement kernel so far, 0, 0}. */
int sparta_vbs_set_a8_live(sparta_vbs_t* A, int32_t enable, void* stream);
int sparta_vbs_a8_live_info(sparta_vbs_t* A, int64_t* info_out /* [8] */, void* stream);
int sparta_vbs_live_info(sparta_vbs_t* A, int64_t* info_out /* [8] */, void* stream);
int sparta_vbs_live_lists_get(sparta_vbs_t* A, int32_t* sd_groups, int32_t* sd_count, int32_t* t_blocks, int32_t* t_count, void* stream);
int sparta_vbs_live_lists_host(int64_t cols, int64_t block_rows, int64_t block_col_size, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab,
                               int64_t block_row_begin, int64_t block_row_end, const uint8_t* keep, int32_t* sd_groups, int32_t* sd_count, int32_t* t_blocks,
                               int32_t* t_count, int64_t* info_out /* [8] */);

/* ---- repattern: a trained layer moved onto a new block pattern (k_repattern.hip) ------------------------------------------------------------------
 * The new pattern is the old one minus dropped blocks plus added ones; the new handle is an ordinary handle created from the new arrays, and the values and
 * the optimizer state are moved from the old mab layout to the new one on the device.
 *
 * sparta_vbs_repattern_host (pure host code, no GPU): the pattern rule.  cols .. block_row_end as for sparta_vbs_block_table_host.  keep: host bytes, one per
 * stored block of the range in the numbering of sparta_vbs_mask_blocks (0 = drop); NULL keeps all.  add: n_add pairs of int64 (block-row, block column); the
 * block-row is numbered over the WHOLE matrix and must lie in [block_row_begin, block_row_end).
 *   nzcount_out[block_rows], jab_out[new nblocks]: the arrays of the WHOLE matrix; block-rows outside the range keep their blocks as they are (their jab
 *     entries are copied, not looked at).  row_part and block_col_size do not change.
 *   map_out[new blocks of the range], int32: per block of the range in the NEW numbering the old block number in the range, or -1 for an added block.
 *   counts_out[4] = {new nblocks, new nztot, new blocks in the range, new nztot of the range}.
 * Inside each block-row of the range the new blocks are the kept old blocks plus the added ones, in strictly ascending block column.  Blocks of block-rows of
 * height 0 are carried (and added) like any other: they have n_all = 0.  With jab_out == NULL and map_out == NULL the call only counts (nzcount_out may be
 * NULL as well; it is written whenever it is given).
 * SPARTA_ERR_INVALID, with NOTHING written: bad dimensions or range; the old jab not strictly ascending inside a block-row of the range, or an entry outside
 * [0, block_cols); an added pair outside the range or with a block column >= block_cols (or negative); an added pair given twice; an added pair that names
 * a block the old pattern stores, kept or not (a stored dead block comes back through keep, not through add); a NULL pointer whose count is above 0 (jab,
 * keep excepted, add; of jab_out and map_out exactly one NULL while its count is above 0; counts_out always).  More than 2^31 - 1 blocks in the new range:
 * SPARTA_ERR_UNSUPPORTED.
 *
 * sparta_vbs_move_blocks: S0..S3 are device tensors in src's mab layout (nztot(src) floats: a range handle's slice from 0), D0..D3 device tensors in dst's;
 * any 4-byte alignment.  A pair with both pointers NULL is skipped; exactly one NULL: SPARTA_ERR_INVALID.  map: HOST, n_blocks(dst) int32.
 *   every dst block b with map[b] >= 0 receives all n_all elements of src block map[b] bit for bit -- positions past cols, NaN payloads and -0.0 included;
 *   every dst block b with map[b] == -1 receives n_all stores of +0.0f and nothing is read for it;
 *   every element of a D belongs to exactly one block, so D may be uninitialised; no byte outside the tensors is written and no S is written.
 * Validated on the host before anything is launched: both handles made from VBS arrays (others: SPARTA_ERR_UNSUPPORTED, as sparta_vbs_mask_blocks) and on the
 * same device; every map entry in [-1, n_blocks(src)); mapped blocks of equal n_all (the handles need not come from sparta_vbs_repattern_host: any two
 * patterns whose mapped blocks agree in size will do; a block of 2^31 or more elements: SPARTA_ERR_UNSUPPORTED); no D overlaps an S or another D; 4-byte
 * alignment.  The call builds one 24-byte record per dst block (source offset, destination offset, n_all, moved or new), uploads them into storage the dst
 * handle owns (grown when needed, freed by sparta_vbs_destroy) and launches ONE kernel for up to four pairs: one wave per dst block, a block's record read
 * once, 16-byte stores on the destination's 16-byte grid, 16-byte loads where source and destination agree modulo 16 bytes and 4-byte loads elsewhere.
 * It is a rare operation: it synchronises the stream (the records of an earlier call may still be read) and returns SPARTA_ERR_UNSUPPORTED while the stream is
 * being captured.  dt_ms covers the kernel only.  n_blocks(dst) == 0, nztot(dst) == 0 or four skipped pairs: success, nothing launched.  src is not changed. */
int sparta_vbs_repattern_host(int64_t cols, int64_t block_rows, int64_t block_col_size, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab,
                              int64_t block_row_begin, int64_t block_row_end, const uint8_t* keep, const int64_t* add /* [n_add][2] */, int64_t n_add,
                              int64_t* nzcount_out, int64_t* jab_out, int32_t* map_out, int64_t* counts_out /* [4] */);
int sparta_vbs_move_blocks(sparta_vbs_t* dst, const sparta_vbs_t* src, const int32_t* map /* host, n_blocks(dst) */,
                           const float* S0, float* D0, const float* S1, float* D1, const float* S2, float* D2, const float* S3, float* D3,
                           void* stream, float* dt_ms);

/* ---- DENSE <-> BLOCKS: a dense matrix on the device scored, sampled into the mab layout of a handle and written back (k_dense.hip) ---------------------
 * The way into the block-sparse stack from a dense weight matrix, and the way back out.  Device pointers only, all three entries.
 *
 * D: a dense rows x cols matrix in SPARTA_ROW_MAJOR (element (r, c) at D[r * ldd + c], ldd >= cols) or SPARTA_COL_MAJOR (D[c * ldd + r], ldd >= rows) of
 * d_dtype SPARTA_F32, SPARTA_F16 or SPARTA_BF16 -- independent of a handle's storage type.  It may start on any element boundary (2 bytes for the 16-bit
 * types, 4 for fp32).  For a handle, rows and cols are the handle's: a range handle has the rows of its block-rows, and row 0 of D is the first row of the
 * range (as its slice of mab counts "from 0").  T: nztot floats in the layout of sparta_vbs_host.mab on any 4-byte boundary: element i of stored column q of
 * a block is T[off + q * h + i] (off, h, jb: sparta_vbs_block_table_host).  No kernel dereferences a misaligned vector pointer: accesses are 16 bytes wide
 * where base, leading dimension, block height and width allow it for a whole tile, one element wide elsewhere.
 *
 * sparta_vbs_gather_dense: for every stored block T[off + q * h + i] = D[r0 + i, jb * w + q] for the columns inside the matrix; the stored positions past
 * `cols` of a ragged last block column get +0.0f.  Every element of T is written (T may be uninitialised); nothing of D outside the stored blocks is read.
 * fp32 D travels as 32-bit words: NaN payloads, -0.0 and denormals arrive bit for bit.  bf16 is widened by a 16-bit shift, bit for bit.  fp16 is widened
 * exactly; a NaN stays a NaN, its payload is not specified.
 *
 * sparta_vbs_scatter_dense: the inverse, D[r0 + i, jb * w + q] = T[off + q * h + i] for the columns inside the matrix; positions of T past `cols` are not
 * read.  A 16-bit D receives the value rounded to nearest even exactly as sparta_vbs_create rounds a 16-bit handle's values and as every image is rounded
 * (bf16 keeps a NaN a NaN, Inf stays Inf; a finite fp32 above the fp16 range becomes Inf).  fill == 0: every element of D outside the stored blocks keeps
 * its bits.  fill != 0: every element of the rows x cols region outside the stored blocks becomes +0 of D's type (one launch that stores the region as +0,
 * in front of the scatter; with an empty pattern it runs alone).  The ldd padding is never written.  A handle that stores the same block column twice in
 * one block-row is refused with SPARTA_ERR_UNSUPPORTED (two blocks would write the same elements of D; gather takes it): found when the table is built.
 *
 * Handles: every handle made from VBS arrays (sparta_vbs_create, _create_range, _create_range_ex with any flags, all three dtypes -- the handles of
 * sparta_vbs_block_ssq); those of sparta_vbs_create_from_csr / _create_transposed: SPARTA_ERR_UNSUPPORTED.  Neither entry reads or writes an image of the
 * handle: to make a handle multiply with gathered values, follow with sparta_vbs_set_values.  The FIRST call of either entry on a handle builds and uploads
 * one 32-byte record per chunk of at most 64 rows of a stored block (offset, first row, first column, height, the chunk's rows, columns inside the matrix --
 * from the block table of sparta_vbs_block_table_host over the handle's own arrays; a block 257 rows tall is five work items, a block of height 0 none) into
 * storage the handle owns, and returns SPARTA_ERR_UNSUPPORTED while the stream is being captured.  Every later call is launches only (one, or two with
 * fill), no allocation, no synchronisation, and can be captured; a replay reads D / T again.  *dt_ms != NULL under capture: SPARTA_ERR_UNSUPPORTED.
 *
 * sparta_dense_block_ssq (no handle): ssq_out[ib * block_cols + jb], block_cols = (cols - 1) / block_col_size + 1, is the fp64 sum of the exact fp64 squares of
 * the elements of grid block (ib, jb) -- rows row_part[ib] .. row_part[ib + 1] - 1, columns jb * w .. -- that lie inside the matrix: the definition of
 * sparta_vbs_block_ssq, so a handle that stores the block and holds the gathered values scores it alike up to the order of the additions.  row_part:
 * DEVICE, block_rows + 1 int64, non-decreasing from 0 to at most rows (it is read by the kernel only, which clamps it into [0, rows]: nothing outside D is
 * read whatever it holds).  One wave per grid block, its runs (rows of the block in row-major, columns in column-major) in a fixed order with fma(d, d, acc)
 * into four accumulators per lane, lanes by xor-shuffle, no atomics, one launch: the score depends on the block's elements and shape alone, is bit-identical
 * from run to run and between an eager call and a replay, and lies within n_in * 2^-53 * ssq of the exact sum (the bound of sparta_vbs_block_ssq).  A block
 * of a block-row of height 0 scores 0.0 (also when rows == 0: the scores are stored, D is not read); an Inf or NaN makes exactly its own block's score
 * non-finite.  Launches only: capturable from the first call.
 *
 * SPARTA_ERR_INVALID, with nothing launched and no output touched: a NULL handle; NULL D, T, ssq_out with work to do; a layout or dtype code that is none of
 * the above; ldd too small; D not aligned to its element, T to 4 bytes, row_part / ssq_out to 8; negative dimensions or block_col_size <= 0; row_part NULL
 * with block_rows > 0.  2^31 or more rows or columns, a block of 2^31 or more elements, more than 2^31 - 1 grid blocks: SPARTA_ERR_UNSUPPORTED.  Empty work
 * (nztot == 0; no grid block) succeeds and launches nothing -- except that fill on an empty pattern still fills. */
int sparta_dense_block_ssq(const void* D, int64_t ldd, int32_t d_layout, int32_t d_dtype, int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size,
                           const int64_t* row_part /* device, block_rows + 1 */, double* ssq_out /* device, [block_rows][block_cols] */, void* stream, float* dt_ms);
int sparta_vbs_gather_dense(sparta_vbs_t* A, const void* D, int64_t ldd, int32_t d_layout, int32_t d_dtype, float* T, void* stream, float* dt_ms);
int sparta_vbs_scatter_dense(sparta_vbs_t* A, const float* T, void* D, int64_t ldd, int32_t d_layout, int32_t d_dtype, int32_t fill, void* stream, float* dt_ms);

/* Ct (+)= A^T * X on the stored blocks of A: the gradient of the dense operand of C = A * B (X = dC, Ct = dB), on the handle itself, so that
 * it follows sparta_vbs_set_values in stream order.  Only handles made with SPARTA_CREATE_TRANSPOSE take the call; every other handle
 * (flags without the bit, sparta_vbs_create, _create_range, _create_from_csr, _create_transposed): SPARTA_ERR_UNSUPPORTED.
 * X : rows x n_cols, column-major, ldx >= rows -- the layout of C of sparta_vbs_spmm (rows in the VBS's reordered order; a range handle:
 *     its own rows, local numbering; a force_fixed_size padding row is a row like any other).
 * Ct: cols x n_cols, column-major, ldo >= cols -- the layout of B of sparta_vbs_spmm; always fp32.
 * fp32 handles: fp32 X.  16-bit handles: X in the handle's type with even ldx (SPARTA_PTR_DEVICE) or fp32 rounded on the device
 * (SPARTA_PTR_HOST); products of the 16-bit values, fp32 accumulation.
 * accumulate = 0 writes every one of the cols x n_cols elements (zeros for columns of A that no stored block covers), 1 adds.  Nothing is
 * written at or beyond row `cols` of a column of Ct: the positions of a ragged last block column that lie past `cols` take no part.
 * Any n_cols >= 1.  Offsets are 64-bit; ldx * n_cols and ldo * n_cols must stay below 2^61 (else SPARTA_ERR_UNSUPPORTED).
 * Deterministic: every element of Ct is summed by one wave in one fixed order (no atomics).  ptr_space / stream / dt_ms as for
 * sparta_vbs_sddmm.  The block-column index and the image are built at creation: a device-pointer call is kernel launches only and can
 * be captured into a hipGraph; SPARTA_PTR_HOST calls stage X and Ct in scratch the handle owns. */
int sparta_vbs_spmm_t(sparta_vbs_t* A, const void* X, int64_t ldx, int32_t n_cols, float* Ct, int64_t ldo, int32_t accumulate,
                      int32_t ptr_space, void* stream, float* dt_ms);
/* The block-column index of sparta_vbs_spmm_t for the CPU suite (no GPU; not a product path): builds the index create builds for the
 * block-rows [block_row_begin, block_row_end) and walks it for one vector: y[cols] = A^T x (x: the range's rows, local numbering).
 * info_out[8] = {block columns with at least one block, work items, longest list of blocks of one item, segments of split columns (0:
 * a block column is never split between workgroups), 0, 0, 0, 0}. */
int sparta_spmm_t_host_check(int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size, const int64_t* row_part,
                             const int64_t* nzcount, const int64_t* jab, const float* mab, int64_t block_row_begin, int64_t block_row_end,
                             const float* x, double* y, int64_t* info_out);
/* The k-compaction rule of the fp32 fragment image, for the CPU suite (no GPU): nonempty[k] != 0 says column k of a step's 32-deep slice
 * has a non-zero; pos[k] is its fragment position (a permutation of 0..31, non-empty columns first: compact index c at (c >> 1) + 16 (c & 1)),
 * *pairs the MFMA pairs the step issues.  The host packer and the update kernel both call the function behind this entry. */
int sparta_frag_positions(const uint8_t* nonempty, uint8_t* pos, int32_t* pairs);
/* The packing rule of the packed fp32 plan, for the CPU suite (no GPU).  A block of a tile is cut into its eight aligned groups of four columns;
 * bit m of group_masks[b] says group m of block b has a non-zero.  Whole blocks are packed into steps of at most 8 slots (one slot per non-empty
 * group), first-fit decreasing by group count, ties in ascending block order.  step_of_block[b] / slot0_of_block[b]: the block's step and the slot
 * of its first non-empty group (the others follow); *n_steps the steps used.  A function of the masks alone. */
int sparta_f32_pack_blocks(int32_t n_blocks, const uint8_t* group_masks, int32_t* step_of_block, int32_t* slot0_of_block, int32_t* n_steps);
/* The packed plan of an fp32 handle: info_out[0] = 1 if its tiles of <= 32 rows run on packed steps (the partly empty blocks of a tile share a
 * step; chosen at creation for handles made without creation flags, by a rule of the handle's own block-rows -- at least 4096 such steps of which
 * packing removes at least 5 % -- never by a timing; SPARTA_F32_PLAN=packed|direct forces it), [1] packed steps, [2] slots (= MFMA pairs),
 * [3] steps of the one-tile plan they replace.  Four values.  A block_row_range handle decides for its own range: where it decides differently from
 * the whole handle the two agree within the fp32 bound, not bit for bit.  (A separate entry because sparta_vbs_info fills exactly 16 values.) */
int sparta_vbs_packed_info(const sparta_vbs_t* A, int64_t* info_out);

/* A dense operand that does NOT change between products, prepared once.  The reference's drivers multiply the same B `-x` times
 * (test/cuda/cuda_multiply.cpp:250-269); the sparse-row kernels of a handle read B row-major, so a column-major (the reference's layout)
 * or gathered B is otherwise transposed into per-handle scratch on EVERY product (11 % of a power-law product).
 * sparta_vbs_prepare_b makes that copy once, on `stream`, into memory the returned object owns; B itself is not copied and must stay
 * valid and unchanged while the object is used.  shard_rows = 0: B is column-major cols x n_cols with leading dimension ldb; shard_rows >
 * 0: the gathered layout of sparta_vbs_spmm_gathered_ld with ldb = the column stride inside a slab (shard_ld; 0 = unpadded = shard_rows).  Device pointers only.  sparta_vbs_spmm_prepared is sparta_vbs_spmm /
 * sparta_vbs_spmm_gathered on that B (SPARTA_SPMM_MFMA; the exception state of a failed call is a plain status code: the handle is usable
 * again).  The implicit per-call transpose of sparta_vbs_spmm stays the default: nothing changes for a caller that never prepares. */
typedef struct sparta_b sparta_b_t;
int sparta_vbs_prepare_b(sparta_vbs_t* A, const void* B, int64_t ldb, int64_t shard_rows, int64_t shard_stride, int32_t n_cols, void* stream,
                         sparta_b_t** out);
int sparta_vbs_spmm_prepared(sparta_vbs_t* A, const sparta_b_t* Bp, void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, void* stream,
                             float* dt_ms);
int sparta_b_destroy(sparta_b_t* Bp);

/* Per-tile-class device timing for roofline reports: when enabled, sparta_vbs_spmm brackets each class
 * launch with HIP events on the launch stream; sparta_vbs_class_times waits for them and writes the last
 * call's milliseconds into ms_out[4]: stream path -> {stream kernel, fix-up kernel, 0, 0};
 * per-class / generic path -> {<=16-row class, <=32-row class, <=64-row class, sparse-row kernels}.
 * (Block-rows whose blocks are nearly empty are multiplied as sparse rows, HBM-bound, instead of as MFMA tiles: see
 * sparta_amd/csrc/vbs_spmm.hip "sparse-row path"; env SPARTA_SPARSE_K=0 keeps everything on the MFMA kernels.) */
int sparta_vbs_set_class_timing(sparta_vbs_t* A, int32_t enable);
int sparta_vbs_class_times(sparta_vbs_t* A, float* ms_out);

/* Shader clock of the last timed call, per launch slot as in sparta_vbs_class_times (mhz_out[4], 0 where no probe ran).
 * With class timing enabled, workgroup 0 of each product kernel reads s_memtime (shader-clock cycles) and s_memrealtime
 * (constant 100 MHz) at entry and exit; the ratio is the clock the MFMA pipes really ran at.  Under a dense fp32 MFMA
 * load on random data MI355X settles well below its 2.4 GHz peak clock (power limit), which scales the attainable
 * fraction of the 157.3 TFLOP/s fp32 matrix peak: bench.py reports it next to the roofline.  No reference counterpart. */
int sparta_vbs_clock_mhz(sparta_vbs_t* A, double* mhz_out);

/* Developer aid: the device allocations the library holds right now, process-wide -- how many, and their bytes as asked of hipMalloc.  Every array of a
 * handle (scratch included) and every prepared B counts; a destroyed handle gives back exactly what it took.  Either pointer may be NULL. */
int sparta_debug_device_allocs(int64_t* live_count, int64_t* live_bytes);

int sparta_vbs_destroy(sparta_vbs_t* A);

/* plan / roofline introspection. info_out (int64[16]):
 *  [0] rows [1] cols [2] block_rows [3] block_col_size [4] nblocks [5] nztot (area)
 *  [6] tiles of <=16 rows [7] <=32 rows [8] <=64 rows [9] 0 [10] device bytes of A
 *  [11] padded MFMA rows summed over (tile, block) pairs x w (executed area)
 *  [12] steps of the stream plan [13] stream workers [14] split tiles
 *  [15] kernel path of the last sparta_vbs_spmm: 1 stream, 2 per-class, 3 generic */
int sparta_vbs_info(const sparta_vbs_t* A, int64_t* info_out);

/* the sparse-row part of the plan. info_out (int64[4]): [0] rows [1] nonzeros kept as (column, value) pairs
 * [2] rows handled one wave each [3] hub rows (cut into segments) */
int sparta_vbs_sparse_info(const sparta_vbs_t* A, int64_t* info_out);

/* the resident-column image of a small fp32 handle (no reference counterpart: the reference multiplies every matrix block by block, vbr.cpp:323-372; this is the
 * product path of its real matrices -- 8-22 k rows, no dense blocks at any block size it sweeps -- at its operand widths B_COLs = 1024 / 8192,
 * scripts/run_multiplication_experiments_fixed_cluster.sh:6-7).  Built when at least half the rows of the handle are on the sparse-row path -- the launches of its MFMA
 * tiles, if it has any, come first; the sparse part of a mixed block-row ADDS to what they stored -- and a column of B and of C fits LDS (rows, columns <= 40 960); taken by sparta_vbs_spmm when B and C are column-major (the reference's layouts) device or host pointers: NC columns of
 * B are copied into LDS, A (length-sorted rows, 64 to a slice, long rows cut into chunks) streams past them from L2, one launch, B and C cross HBM once; a row's
 * nonzeros are added in ascending column order as in CSR::multiply (csr.cpp:49-65).  SPARTA_COLRES=0 at create time: not built (the row gather takes the product).
 * info_out (int64[12]): [0] slices of 64 slots of the part with most (0: no image) [1] stored entries, padding included [2] rows cut into chunks [3] cells a column set
 * needs in LDS (the largest range of B + 4, or the largest staging image: rows + extra cells of the chunks) [4] longest slot [5] columns per workgroup of the last product on this path (0: the last product took another path)
 * [6] nonzeros [7] 1: every stored value is 1.0f and the image holds columns only (the reference's pattern-only runs, -P 1)
 * [8] parts the rows of C are cut into, [9] K ranges the columns of A are cut into (1, 1: a column of B and of C fits LDS whole; up to 4 x 4: rows, columns <= 163 k --
 * the workgroup of a part walks the ranges one after the other with its sums in registers, B is read once per part)
 * [10] parts of the SECOND image a handle keeps for products of few column sets (4; 0: none -- fewer than 2048 rows, or SPARTA_COLRES_SMALL=0): with at most 64 column sets the
 * product is one round of 4 x the workgroups, each streaming a quarter of A; [11] 1: the last product used it */
int sparta_vbs_colres_info(const sparta_vbs_t* A, int64_t* info_out);
/* HOST-side walk of that image for one column x of B (y = A x; rows of C through crow, NULL = identity; crow[i] + 2^31: row i ADDS to y -- the sparse part of a mixed block-row --,
 * crow[i] = -1: CSR row i is not a sparse row and y[i] is left alone -- a block-row of tiles; info_out as above, [0] = 0 and y untouched when the matrix
 * gets no image): slots in slice order, a slot's entries in order, the chunks of a long row added in chunk order -- the arithmetic of the kernel, for the CPU suite
 * to check the builder with.  Not a product path (and not a fallback: sparta_vbs_spmm never calls it). */
int sparta_colres_host_check(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* crow, const float* x,
                             float* y, int64_t* info_out);
/* HOST-side walk of the sparse-row device form (what the sparse-row kernels read: the list of short rows, the long rows' records and segments, the column windows and the
 * eight per-XCD streams) of a CSR matrix for one column x of B; rows, crow and y as for sparta_colres_host_check.  The short rows come from the list, a long row from its record:
 * its segments in row order, one partial per segment, the partials added in that order.  SPARTA_ERR_INVALID with a message if the form is broken: a nonzero covered not exactly
 * once, a row's segments not contiguous and in order, the partials' places not a permutation, the segments not in window order (one list), or the streams not monotone, a window
 * split across streams, a stream's windows not in column order (XCD order).  The SPARTA_SPARSE_SEG / SPARTA_SP_* switches apply as at creation.
 * info_out (12 words): [0] sparse rows [1] short rows [2] long rows [3] segments [4] window width in columns (0: no windows) [5] streams that hold segments (0: one list)
 * [6] base segment length [7] longest short row [8] nonzeros a segment holds before a window boundary ends it.  For the CPU suite; not a product path. */
int sparta_sparse_rows_host_check(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* crow, const float* x,
                                  float* y, int64_t* info_out);

/* the column-compacted ("union-pattern") tiles of a handle made by sparta_vbs_create_from_csr (fp32, and since the round's second half fp16 / bf16 storage: the same tiles through the 16-bit matrix instruction).  They replace what the reference's builder stores for a cluster at
 * SMALL block widths -- VBR::fill_from_CSR_inplace flags, per block-row, exactly the column blocks its rows touch and stores them back to back
 * (src/general/vbr.cpp:177-228; at -b 1 that is a dense rows x |union| tile plus the ascending column list, the ids its Jaccard distance is defined on,
 * src/general/blocking.cpp:923-994) -- and what VBR::multiply does with it (vbr.cpp:323-372): a block-row whose rows share columns but whose w-wide blocks would be
 * nearly empty is kept as tiles of <= 64 consecutive reordered rows x the columns at least 2-3 of those rows use, multiplied on the matrix cores against the
 * gathered rows of a row-major B (k_union.hip; a column-major B is transposed once per product, or once per sparta_vbs_prepare_b); the nonzeros of the other
 * columns are sparse rows that add.  SPARTA_UNION=0 at create time: not built.  SPARTA_SPMM_EXACT is not available on such a handle (as for any handle with sparse rows).
 * A row's nonzeros in columns too thinly used for the list ride in the tile's TAIL (at most SPARTA_UNION_TAIL = 16 per row) and are added in the tile's epilogue; only what
 * exceeds that is left to the sparse-row kernels.
 * The matrix instruction works on row tiles of 16 rows (fp32 handles: v_mfma_f32_16x16x4_f32) or 32 rows (16-bit handles): a tile of mt rows is multiplied as ceil(mt / 16) resp.
 * ceil(mt / 32) row tiles.
 * info_out (int64[12]): [0] tiles of <= 32 rows [1] tiles of 33..64 rows [2], [3] their 32-deep steps [4] stored elements (tile rows x list entries)
 * [5] list entries [6] nonzeros the tiles hold (lists + tails) [7] persistent workgroups of the launch [8] rows of C the tiles own [9] nonzeros in the tails
 * [10] elements the kernel multiplies (steps x 32 x the tile's rows rounded up to whole row tiles) [11] rows per row tile (16 or 32; 0: no tiles) */
int sparta_vbs_union_info(const sparta_vbs_t* A, int64_t* info_out);
/* HOST-side check of that builder and its device plan for the CPU suite (no GPU; not a product path, and not a fallback: sparta_vbs_spmm never calls it): the hybrid
 * image of the CSR matrix under `grouping` -- w-wide tiles, column-compacted tiles, sparse rows, decided as sparta_vbs_create_from_csr decides them for an fp32 handle --
 * multiplied with ONE column x; the column-compacted tiles are walked in their DEVICE form (step records, list entries, MFMA-fragment-order slices, dealt to
 * `max_workers` workers).  y (double, [rows padded as force_fixed_size pads them], reordered order).  info_out (int64[14]): [0..6] as sparta_vbs_union_info,
 * [7] nonzeros left to the sparse rows [8] stored elements of the w-wide tiles [9] padded rows [10], [11] workers of the two step lists [12] nonzeros in the tails [13] rows the tiles own */
int sparta_union_host_check(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* grouping, int64_t col_block_size,
                            int64_t row_block_size, int32_t force_fixed_size, int32_t max_workers, const float* x, double* y, int64_t* info_out);

/* the hub part of the plan of a 16-bit handle of 64-wide blocks (no reference counterpart: the reference multiplies every block-row the same way,
 * vbr.cpp:323-372 / cuda_utilities.cpp:828-875).  The long tiles of 33..64 rows -- the dense hub of a power-law matrix under the fixed 64 x 64 grid -- are grouped
 * by the Jaccard similarity of their block-column sets into group tiles of 2 or 4 and multiplied by a GEMM-shaped kernel that stages A and B once per workgroup.
 * info_out (int64[10]): [0] steps (one 64-deep k slice of one group tile) [1] 64-row tiles in the hub plan [2] group tiles [3] tiles per group tile (2 or 4; 0: no
 * hub plan) [4] stored elements of those tiles [5] elements the kernel multiplies (the union of a group's block columns x its tiles) [6] workers [7] K chunks of
 * the step order [8] segments (runs of one group tile on one worker: each one that is not a whole tile leaves partial images for the fix-up) [9] 0.
 * SPARTA_HUB=0 switches the hub plan off (every tile then runs on the 64-row plan as before). */
int sparta_vbs_hub_info(const sparta_vbs_t* A, int64_t* info_out);

/* number of visible HIP devices (0 when none); never initialises a device context */
int sparta_device_count(void);

const char* sparta_last_error(void);
const char* sparta_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPARTA_AMD_H */
