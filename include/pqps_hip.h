/* pqps_hip.h -- thin C-ABI shim over the hand-written gfx950 kernels.
 *
 * This is the lowest drop-in boundary of the HIP backend: plain pointers and
 * sizes, no C++ / torch types.  Everything behind it lives in ONE hipcc
 * translation unit (csrc/pqps_hip.hip).  The C11 engine
 * (engine/hip/executeEngine-hip.c) and the Python harness (ctypes) are its
 * only callers.
 *
 * What each entry point replaces in the reference (Jairik/Parallel-Query-
 * Processing-System, paths relative to its root):
 *
 *   pqps_filter_scan    linearSearchRecords over engine->all_records
 *                       (engine/serial/executeEngine-serial.c:854-878, called
 *                       from :466) with evaluateWhereClause :292-316 /
 *                       checkCondition :251-289 / CMP_* :18-123 fused in.
 *   pqps_filter_gather  linearSearchRecords over the index candidates
 *                       (executeEngine-serial.c:471) -- order preserving.
 *   pqps_filter_count   COUNT(*): resultSetS.numRecords without the ID list
 *                       (MPI shape: MPI_Allreduce at engine/mpi/executeEngine-mpi.c:745).
 *   pqps_filter_flags   the per-row flag array of DELETE
 *                       (engine/omp/executeEngine-omp.c:708-732, mpi :726-741).
 *   pqps_index_build    loadIntoBplusTree (engine/serial/buildEngine-serial.c:41-62)
 *                       -- as a permutation sorted (key asc, row desc), the
 *                       leaf order of engine/bplus.c:282-314,471-490.
 *   pqps_index_probe    findLeaf + the leaf walk of findRange (bplus.c:282-358).
 *   pqps_index_select   one probe of executeQuerySelectSerial, whole (executeEngine-serial.c:358-448).
 *   pqps_partition      the block partition of engine/mpi/executeEngine-mpi.c:703-715.
 *   pqps_exchange_*     the per-query exchange of the MPI engine (executeEngine-mpi.c:717-768:
 *                       local scan of the rank's rows, MPI_Allgather of the sizes + MPI_Allgatherv of
 *                       the IDs; :745 MPI_Allreduce for counts) over RCCL, same shape.
 *   pqps_merge_slots    the displacement arithmetic + placement of MPI_Allgatherv (:758-765) for
 *                       equal-size slots (index mode across processes).
 *   pqps_compact_rows   the survivor compaction of DELETE (executeEngine-serial.c:646-680).
 *   pqps_bump_codes     (no counterpart: keeps dictionary codes order-preserving on INSERT).
 *   pqps_member_flags   (no counterpart: LIKE / IN as a set of dictionary codes or values).
 *   pqps_filter_assign  (no counterpart: UPDATE SET ... WHERE, constants written in place).
 *   pqps_remap_codes    (no counterpart: batch INSERT, every code of a column to its place in a merged dictionary).
 *
 * All functions return 0 on success or a negative PQPS_E* code; the text of
 * the last error of the calling thread is at pqps_last_error().
 * Device pointers are plain `void *` (hipMalloc / torch tensor data_ptr).
 * `stream` is a hipStream_t passed as void*; NULL = the context's own stream.
 */
#ifndef PQPS_HIP_H
#define PQPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQPS_OK            0
#define PQPS_EINVAL       -1   /* bad argument (shape, width, alignment, capacity) */
#define PQPS_EHIP         -2   /* a HIP runtime call failed                        */
#define PQPS_ENOMEM       -3
#define PQPS_ENODEVICE    -4   /* no gfx950 device visible                         */
#define PQPS_EOVERFLOW    -5   /* out_ids capacity too small for the matches       */
#define PQPS_ETIMEOUT     -6   /* a bounded host wait of the exchange ran out: the communicator was aborted, the exchange is dead */

#define PQPS_MAX_COLUMNS  12   /* columns of `record` (include/logType.h)          */
#define PQPS_MAX_LEAVES   32   /* leaf comparisons in one WHERE tree               */
#define PQPS_TT_LEAVES     6   /* <= 6 leaves: 64-entry truth table path           */
#define PQPS_TILE_ROWS  4096   /* column buffers are padded to a multiple of this  */

/* One device-resident column.  `width` in {1,2,4,8} bytes per row; values are
 * compared as unsigned after the host has biased signed columns (see
 * pqps_leaf).  `data` must be 16-byte aligned.
 *
 * width == PQPS_WIDTH_BITS: a BIT PLANE of a boolean column -- row r is bit (r & 7) of byte r >> 3, LSB first, each
 * row's value 0 or 1 (pqps_pack_bits makes one from a byte column).  `data` 16-byte aligned, readable up to the padded
 * row count as for byte columns (n_rows rounded up to PQPS_STEP_ROWS rows = a multiple of 128 bytes).  Accepted by the
 * scan entry points (pqps_filter_scan / _count / _flags, pqps_qstream_*, pqps_exchange_select / _count); every other
 * entry point taking a pqps_column returns PQPS_EINVAL for one.
 *
 * width == PQPS_WIDTH_P12: a 12-BIT PACKED copy of a u16 column whose values are below 4096 (dictionary codes) -- row r is
 * the 12 bits at bit offset 12 r of the buffer, little-endian, so 8 rows are exactly 3 dwords and a row costs 1.5 bytes
 * (pqps_pack12 makes one).  `data` 16-byte aligned, readable up to n_rows rounded up to PQPS_STEP_ROWS rows, times 3/2
 * bytes; the fields of rows at and past n_rows are zero.  Its values compare as the u16 column's do.  Accepted by the
 * same scan entry points as a bit plane, and only as the FIRST column of a one-column predicate or of a two-column
 * predicate whose second column is a bit plane, with at most PQPS_TT_LEAVES leaves: the shapes (P) and (P,B).  Any other
 * position or entry point returns PQPS_EINVAL.
 * Measured at 100 M rows on MI355X ("Round 6"): `sudo_used = FALSE AND user_name = "..."` reads 1.625 B/row
 * instead of 2.125; ONE launch at a time takes what the u16 column takes (IDs 46.9 against 47.1 us, COUNT 40.8 against
 * 40.7), a stream of overlapping launches through the engine 40.4 - 41.7 us per query against 42.5 - 46.3. */
#define PQPS_WIDTH_BITS 0x81u
#define PQPS_WIDTH_P12  0x8Cu
typedef struct pqps_column {
    const void *data;
    uint32_t width;
    uint32_t reserved;
} pqps_column;

/* One leaf comparison, normalised by the host to an unsigned window test
 *      hit = ((value - lo) <= span) XOR negate
 * in 32-bit arithmetic (value zero-extended, lo and span taken mod 2^32) for columns of width 1, 2 and 4 and for bit
 * planes, and in 64-bit arithmetic for width 8 -- NOT in the column's own width: on a 1-byte column lo = 256 selects
 * no value, where 8-bit arithmetic would read it as lo = 0.  The host compiler relies on this (a comparison past the
 * last value of a full 256- or 65536-entry dictionary).  Covers =, !=, <, <=, >, >= on u64 / i32 / bool / dictionary
 * codes (signed i32 windows work unchanged in two's complement). */
typedef struct pqps_leaf {
    uint32_t column;          /* index into the pqps_column array of the call */
    uint32_t negate;          /* 0 or 1                                       */
    uint64_t lo;
    uint64_t span;
} pqps_leaf;

/* Jump-table form of the short-circuit evaluation of the WHERE tree
 * (executeEngine-serial.c:292-316): after leaf k, go to on_true[k] /
 * on_false[k]; targets are a later leaf index, PQPS_ACCEPT or PQPS_REJECT. */
#define PQPS_ACCEPT 0xFE
#define PQPS_REJECT 0xFF

typedef struct pqps_predicate {
    uint32_t n_leaves;                       /* 0: constant predicate (truth bit 0) */
    uint32_t n_columns;                      /* columns referenced, <= 12            */
    uint64_t truth;                          /* truth table over leaf bits, n<=6     */
    pqps_leaf leaf[PQPS_MAX_LEAVES];         /* sorted by `column`                   */
    uint8_t on_true[PQPS_MAX_LEAVES];        /* in ORIGINAL evaluation order ...     */
    uint8_t on_false[PQPS_MAX_LEAVES];
    uint8_t order[PQPS_MAX_LEAVES];          /* ... order[i] = leaf slot of step i   */
} pqps_predicate;

typedef struct pqps_ctx pqps_ctx;

const char *pqps_last_error(void);
/* The kernel instantiation the calling thread's last filter call chose, as rocprofv3 would name it
 * (e.g. "eval_chain_kernel<MODE_IDS, W0=2, W1=1, W2=0, S=1, NT=true, VC=false>"): what bench.py reports. */
const char *pqps_last_kernel(void);

/* Context = device ordinal + stream + filter scratch (match bits, step / group / supergroup
 * counts; grown on demand).  One query at a time per context; use one context per host thread. */
int  pqps_ctx_create(int device, pqps_ctx **out);
void pqps_ctx_destroy(pqps_ctx *ctx);
/* Allocates the filter scratch for tables of up to n_rows now (otherwise the first query does it:
 * half a dozen device allocations, several ms). */
int  pqps_ctx_reserve(pqps_ctx *ctx, uint64_t n_rows);
int  pqps_ctx_sync(pqps_ctx *ctx, void *stream);
/* Launch parameters of this context's ID queries (tests, A/B runs inside one process): "list16" 0 / 1 (the list area),
 * "list16_min" / "list16_min_u8" (a step with more matches leaves a 16-bit list), "list_max" (a step with at
 * most this many matches leaves 16-bit entries in its slot; 0 .. 128), "tiny_max" (... in its tiny word; 0 .. 3),
 * "expand_lag" / "sum_lag" (groups),
 * "tune" (bits), "steps" (chain scans, ID output and COUNT: 0 = one step per wave, 1 = two adjacent steps per wave where
 * the shape has such a kernel -- a lone byte column, a 12-bit packed column alone or with a plane);
 * value < 0 restores the default. */
int  pqps_ctx_set_option(pqps_ctx *ctx, const char *name, long value);
int  pqps_device_count(void);
int  pqps_ctx_device(pqps_ctx *ctx);
/* Per-launch HIP-event timing of the filter (up to 4096 launches per reset).
 * The scan kernel carries its own begin / end events on the dispatch packet, i.e. the timestamps rocprofv3
 * --kernel-trace reports.  pqps_ctx_kernel_time waits for the recorded launches and returns: *eval_ms = sum of
 * the scan-kernel durations, *total_ms = sum over the whole query, and their number; it then resets the recorder.
 * An ID query is ONE launch (scan tiles + expanders): eval_ms == total_ms; COUNT(*) / flags add the
 * one-workgroup reduction behind the scan.  While timing is on, pqps_qstream_scan / pqps_exchange_select run
 * each query whole on the caller's stream with the context's own scratch (so that the events mean the above):
 * issue them on ONE stream then. */
int  pqps_ctx_set_timing(pqps_ctx *ctx, int enable);
int  pqps_ctx_kernel_time(pqps_ctx *ctx, double *eval_ms, double *total_ms, int *launches);
/* Fills name (<=63 chars), CU count and total HBM bytes of the ctx device. */
int  pqps_device_info(pqps_ctx *ctx, char *name64, int *compute_units, uint64_t *hbm_bytes);

/* Plain device memory helpers so a C host needs no HIP headers. */
int  pqps_malloc(pqps_ctx *ctx, size_t bytes, void **dptr);
int  pqps_free(pqps_ctx *ctx, void *dptr);
/* Pinned host memory that the device addresses as well (zeroed): a kernel's few result words -- a match count --
 * written there are on the host when the query's completion event has fired, no download call (~20 us of host
 * time each) in between. */
int  pqps_malloc_mapped(pqps_ctx *ctx, size_t bytes, void **host_ptr, void **dev_ptr);
int  pqps_free_mapped(pqps_ctx *ctx, void *host_ptr);
int  pqps_memset(pqps_ctx *ctx, void *dptr, int value, size_t bytes, void *stream);
int  pqps_upload(pqps_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes, void *stream);
int  pqps_download(pqps_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes, void *stream);
/* Device-to-device copy between the devices of two contexts (or inside one), asynchronous on `stream` of the
 * DESTINATION context (NULL: its own stream): what the one-process engine gathers its shards' results with
 * (peer DMA over xGMI -- the one-process counterpart of the send / recv pairs of pqps_exchange, which in turn
 * stand for MPI_Allgatherv, engine/mpi/executeEngine-mpi.c:765). */
int  pqps_copy_peer(pqps_ctx *dst_ctx, void *dst, pqps_ctx *src_ctx, const void *src, size_t bytes, void *stream);

/* codes[i] += 1 for every i < n_rows with codes[i] >= threshold (`width` 1, 2 or 4 bytes).
 * Keeps the dictionary codes of a string column order-preserving when INSERT adds a value
 * at rank `threshold`. */
int pqps_bump_codes(pqps_ctx *ctx, void *codes, uint32_t width, uint64_t n_rows, uint32_t threshold, void *stream);

/* Bit plane of a byte column (a PQPS_WIDTH_BITS column): writes plane bytes [first_byte, plane_bytes), bit r = (bytes[r] != 0)
 * for r < n_rows and 0 past it.  Reads bytes[r] for r < n_rows only.  `plane` 16-byte aligned.  Asynchronous on `stream`. */
int pqps_pack_bits(pqps_ctx *ctx, const uint8_t *bytes, uint64_t n_rows, uint8_t *plane, uint64_t first_byte, uint64_t plane_bytes,
                   void *stream);

/* 12-bit packed copy of a u16 column (a PQPS_WIDTH_P12 column): writes the fields of rows [first_row rounded down to 8,
 * padded_rows) -- codes[r] & 0xFFF for r < n_rows, 0 past it -- and nothing in front of them.  The caller guarantees codes
 * below 4096.  `padded_rows` a multiple of 8 (the column's rows rounded up to PQPS_STEP_ROWS); `packed` holds
 * padded_rows * 3 / 2 bytes.  Reads codes[r] for r < n_rows only.  `codes` and `packed` 16-byte aligned.  Asynchronous on
 * `stream`. */
int pqps_pack12(pqps_ctx *ctx, const uint16_t *codes, uint64_t n_rows, void *packed, uint64_t first_row, uint64_t padded_rows,
                void *stream);

/* Set membership of one column, row by row (the member pass of a WHERE with LIKE / IN: include/hipPredicate.h).  `col` 1, 2,
 * 4 or 8 bytes wide; a bit plane, or an 8-byte column with the bitmap form, is PQPS_EINVAL.
 *   PQPS_MEMBER_BITMAP: idx = value - base in 32-bit arithmetic; the row is a member iff idx < n_bits and bit idx of
 *     bitmap_dev (u32 words, LSB first; n_bits <= 2^32) is set.  A bitmap of up to PQPS_MEMBER_LDS_BITS bits is staged into
 *     LDS by every workgroup, a larger one is read from global memory (it stays in L2).
 *   PQPS_MEMBER_LIST: the row is a member iff its value, zero-extended to u64, is in list_dev[0 .. n_list), ascending and
 *     duplicate-free (binary search).  An i32 column takes part as its u32 bit pattern.
 * OUTPUT.  PQPS_MEMBER_BYTES: out[r] = 0 / 1 for r < n_rows, as pqps_filter_flags writes; PQPS_MEMBER_PLANE: a
 * PQPS_WIDTH_BITS plane as pqps_pack_bits writes, bytes [0, n_rows rounded up to PQPS_STEP_ROWS, / 8), the bits of rows at
 * and past n_rows 0.  `out` 16-byte aligned.  *out_count (device, may be NULL) = the member rows.  `col` is read up to n_rows
 * rounded up to PQPS_STEP_ROWS, as a scan reads it.  n_rows == 0 launches nothing (count 0).  Asynchronous on `stream`. */
#define PQPS_MEMBER_BITMAP 0
#define PQPS_MEMBER_LIST   1
#define PQPS_MEMBER_BYTES  0
#define PQPS_MEMBER_PLANE  1
#define PQPS_MEMBER_LDS_BITS (1u << 18)   /* 32 KiB of LDS per workgroup: five workgroups fit a CU's 160 KiB */
int pqps_member_flags(pqps_ctx *ctx, const pqps_column *col, uint64_t n_rows, int form, uint32_t base, uint64_t n_bits,
                      const uint32_t *bitmap_dev, const uint64_t *list_dev, uint32_t n_list, int out_form, void *out,
                      uint64_t *out_count, void *stream);

/* Scan mode.  Evaluates `pred` on rows [0, n_rows) of `cols` and writes the
 * matching row IDs (row + id_base, u32) in ASCENDING row order to out_ids and
 * their number to *out_count (device u64).  Asynchronous on `stream`.  One launch.
 * Columns must be readable up to n_rows rounded up to PQPS_STEP_ROWS (1024) rows: the last, partial step is
 * loaded whole and masked.  A launch whose bounded internal waits ran out (never seen with in-order
 * dispatch) sets the context's sticky status word: pqps_ctx_sync then fails with PQPS_EHIP. */
#define PQPS_STEP_ROWS 1024
int pqps_filter_scan(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols,
                     uint64_t n_rows, uint32_t id_base, const pqps_predicate *pred,
                     uint32_t *out_ids, uint64_t out_capacity, uint64_t *out_count,
                     void *stream);

/* COUNT(*) only: no ID list, one u64. */
int pqps_filter_count(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols,
                      uint64_t n_rows, const pqps_predicate *pred,
                      uint64_t *out_count, void *stream);

/* Per-row byte flags (1 = match), the DELETE / MPI_Allgatherv shape. */
int pqps_filter_flags(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols,
                      uint64_t n_rows, const pqps_predicate *pred,
                      uint8_t *out_flags, uint64_t *out_count, void *stream);

/* Index mode.  Candidates are cand[range[0] .. range[1]) (device u32 row
 * numbers, `range` = 2 device u64 as written by pqps_index_probe); rows that
 * satisfy `pred` are APPENDED, candidate order preserved, at
 * out_ids[*out_count ...], and *out_count (device u64) is advanced -- several
 * probes concatenate without a host round trip (executeEngine-serial.c:444-448).
 * Only out_ids[0 .. out_capacity) is ever written: an ID whose place is at or past out_capacity is dropped, and
 * *out_count still advances by every row that passed (a count above out_capacity says the list was cut), also
 * when it was at or above out_capacity before the call.  IDs are row + id_base in 32-bit arithmetic. */
int pqps_filter_gather(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols,
                       const uint32_t *cand, const uint64_t *range, uint64_t max_candidates,
                       uint32_t id_base, const pqps_predicate *pred,
                       uint32_t *out_ids, uint64_t out_capacity, uint64_t *out_count,
                       void *stream);

/* Builds perm[0..n) = row numbers sorted by (key ascending, row DESCENDING)
 * and sorted_keys[0..n) (same width as the column).  key_kind: 0 = unsigned,
 * 1 = signed i32.  Nothing behind perm[n - 1] / sorted_keys[n - 1] is written; n_rows == 0
 * returns PQPS_OK and writes nothing.  Synchronises the stream. */
int pqps_index_build(pqps_ctx *ctx, const pqps_column *col, uint64_t n_rows, int key_kind,
                     uint32_t *perm, void *sorted_keys, void *stream);

/* range[0] = first position with key >= key_lo, range[1] = first position with
 * key > key_hi (inclusive window, findRange semantics); keys as raw 64-bit
 * patterns, compared signed when key_kind == 1.  The key is the low `width` bytes of
 * its pattern (an i32 key may come zero- or sign-extended).  range[1] is never below
 * range[0]: key_lo > key_hi gives the empty range at range[0].  n_rows == 0 gives (0, 0). */
int pqps_index_probe(pqps_ctx *ctx, const void *sorted_keys, uint32_t width, int key_kind,
                     uint64_t n_rows, uint64_t key_lo, uint64_t key_hi,
                     uint64_t *range, void *stream);

/* One index probe of a query, whole: pqps_index_probe into `range`, then the probe's rows that satisfy `pred` appended
 * as pqps_filter_gather does (executeEngine-serial.c:358-448: findRange, then the complete WHERE on every row found).
 * `index_column` = the column the index (perm / sorted_keys) was built on.  When `pred` is nothing but the probed
 * comparison itself -- ONE leaf on the indexed column whose window is [key_lo, key_hi], accepted when it holds (the
 * reference's `risk_level > 3` with an index on risk_level) -- every row found passes, and the rows are copied in
 * index order instead of evaluated (PQPS_INDEX_COPY=0, tests: always evaluate; same result) -- cut at out_capacity
 * and counted exactly as pqps_filter_gather does. */
int pqps_index_select(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, const pqps_column *index_column,
                      const uint32_t *perm, const void *sorted_keys, int key_kind, uint64_t n_rows,
                      uint64_t key_lo, uint64_t key_hi, uint32_t id_base, const pqps_predicate *pred,
                      uint64_t *range, uint32_t *out_ids, uint64_t out_capacity, uint64_t *out_count, void *stream);

/* DELETE on the device (engine/serial/executeEngine-serial.c:646-680 removes the matching rows and
 * keeps the survivors in order): `delete_flags` is what pqps_filter_flags produced (1 = row goes).
 * Every column is compacted in place to the surviving rows, order preserved; *kept_out = survivors.
 * Synchronises the stream.  Dictionary codes stay valid: a code nobody carries any more is harmless. */
int pqps_compact_rows(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows,
                      const uint8_t *delete_flags, uint64_t *kept_out, void *stream);

/* Projection on the device (the gather half of executeEngine-serial.c:504-515): out[i] = the column's
 * value (numeric, or the dictionary code of a string column) of result row ids[i], for the first
 * min(*count_dev, capacity) rows; `out` has the column's width.  Works for any ID order (scan or index
 * mode).  A caller that wants text materialises it from these values only for the rows it shows. */
int pqps_project_column(pqps_ctx *ctx, const pqps_column *col, const uint32_t *ids, const uint64_t *count_dev,
                        uint64_t capacity, uint32_t id_base, void *out, void *stream);

/* Index mode across shards (no counterpart in the reference: its MPI engine replicates the table).
 * A shard's index-mode result is ordered (key asc, row desc) within the shard; rows of a higher rank
 * are higher rows, so the table-wide leaf order of engine/bplus.c:282-358 is the sort of the union by
 * (key ascending, row descending).  pqps_gather_keys produces, for a result list, the order-preserving
 * u64 image of each row's key (count read on the device, e.g. a slot header; signed i32 keys biased);
 * pqps_merge_index_slots takes the all-gathered [count | ids] slots and the parallel key slots
 * (`world` x (slot_stride - PQPS_SLOT_HEADER_WORDS) u64) and writes the merged order.  One probed
 * condition per call; a query with several probed conditions (whose results the serial engine
 * concatenates, duplicates included) merges each condition's segment with its own call.
 * Synchronises the stream (the sort needs the total on the host).
 *   pqps_gather_keys: keys_out[i] for i < min(*count_dev, capacity), row = ids[i] - id_base in 32-bit arithmetic; nothing
 *     behind that is written.  pqps_project_column stops at the same place.
 *   pqps_merge_index_slots: the slots are those of pqps_merge_slots (a slot that reports more than slot_stride -
 *     PQPS_SLOT_HEADER_WORDS IDs holds that many).  Rank r's keys begin at key_slots[r * (slot_stride -
 *     PQPS_SLOT_HEADER_WORDS)] -- the key slots are that far apart, NOT slot_stride -- key i going with ID i of the slot.
 *     The call sorts the union, so the IDs of a slot may come in any order (the engine delivers leaf order).  `totals`
 *     must not be NULL (PQPS_EINVAL): totals[0] = IDs held by the slots, totals[1] = the sum of the reported counts.
 *     totals[0] > merged_capacity: PQPS_EOVERFLOW, both totals written, `merged` untouched.  Otherwise merged[0 .. totals[0])
 *     is written and nothing behind it. */
int pqps_gather_keys(pqps_ctx *ctx, const pqps_column *col, int key_kind, const uint32_t *ids, const uint64_t *count_dev,
                     uint64_t capacity, uint32_t id_base, uint64_t *keys_out, void *stream);
int pqps_merge_index_slots(pqps_ctx *ctx, const uint32_t *slots, const uint64_t *key_slots, uint32_t world,
                           uint64_t slot_stride, uint32_t *merged, uint64_t merged_capacity, uint64_t *totals, void *stream);

/* Tail of the all-gatherv merge.  A slot is what one rank's pqps_filter_scan produced when
 * given out_count = slot and out_ids = slot + PQPS_SLOT_HEADER_WORDS:
 *     [u64 match count][u64 reserved][u32 row IDs ...]
 * `slots` holds `world` such slots, `slot_stride` u32 apart -- what ONE equal-size RCCL
 * all-gather delivers (the count travels with the payload, so MPI_Allgather of the sizes +
 * MPI_Allgatherv of the data, engine/mpi/executeEngine-mpi.c:753-765, become a single
 * collective).  Writes the rank-order concatenation of the ID lists to `merged` and, if
 * `totals` != NULL, totals[0] = IDs merged, totals[1] = sum of the reported counts (larger
 * => a slot overflowed).  A slot that reports more than slot_stride - PQPS_SLOT_HEADER_WORDS IDs
 * holds that many; what a slot holds behind its count is never read into `merged`.
 * merged_capacity below totals[0]: the call still returns PQPS_OK, `merged` holds the first
 * merged_capacity IDs of the concatenation, nothing behind them is written, and totals[0] says
 * what there was (the caller compares).  Everything stays on the device. */
#define PQPS_SLOT_HEADER_WORDS 4
int pqps_merge_slots(pqps_ctx *ctx, const uint32_t *slots, uint32_t world, uint64_t slot_stride,
                     uint32_t *merged, uint64_t merged_capacity, uint64_t *totals, void *stream);

/* ---- a stream of queries on one GPU ------------------------------------------------------------------
 * An ID query is one launch: scan tiles that read the table at HBM speed, and behind the last of them a tail
 * in which the last tiles drain and the expanders wait for sums and hand out the last IDs -- 7 us (sparse
 * answer) to 25 us (dense) of a 100 M-row query in which most of the chip idles.  pqps_qstream_scan is
 * pqps_filter_scan with TWO queries in flight: each runs whole on one of two HIP streams of the query stream's
 * own (with a scratch of its own), so the dispatcher fills the slots one query's tail leaves free with the
 * next query's scan tiles (the reference's OpenMP driver issues its queries concurrently too,
 * QPEOMP.c:234-291).  `scan_stream` only orders the beginning: the first query after create / sync waits for
 * what that stream holds at that moment.  Results are complete after pqps_qstream_sync() (or a device
 * synchronise); the caller keeps a ring of `depth` out_ids / out_count pairs, the call for query k uses pair
 * k % depth and blocks on the host only until query k - depth has finished.
 * The two streams must sit on different hardware queues of the runtime (two streams that share one run their
 * launches one after the other): they are created at the highest stream priority, both the same -- the runtime
 * keeps a pool of hardware queues per priority, so they get two queues of their own however many streams the
 * rest of the process has created. */
typedef struct pqps_qstream pqps_qstream;
int pqps_qstream_create(pqps_ctx *ctx, uint32_t depth, pqps_qstream **out);
int pqps_qstream_scan(pqps_qstream *q, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, uint32_t id_base,
                      const pqps_predicate *pred, uint32_t *out_ids, uint64_t out_capacity, uint64_t *out_count,
                      void *scan_stream);
/* COUNT(*) through the same two lanes: pqps_filter_count with two queries in flight; the caller keeps a ring of
 * `depth` out_count words. */
int pqps_qstream_count(pqps_qstream *q, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows,
                       const pqps_predicate *pred, uint64_t *out_count, void *scan_stream);
int pqps_qstream_sync(pqps_qstream *q);
/* What the last answer looked like (the caller knows once it has a count: the engine at awaitQueryHIP).  While
 * answers hold a quarter of the rows or more, ID queries go to ONE lane: two dense expansions side by side get in each
 * other's way (`risk_level > 1`, 43 % of 100 M rows: 124 us one at a time, 140 - 147 per query with two in flight), a
 * sparse answer's end hides under the next query's scan.  Thread-safe against the issuing calls. */
void pqps_qstream_hint_answer(pqps_qstream *q, uint64_t matches, uint64_t n_rows);
/* Host time (ns) pqps_qstream_scan has spent waiting for an output pair to come free -- as opposed to time inside
 * runtime calls; `reset` != 0 clears the counter. */
uint64_t pqps_qstream_wait_ns(pqps_qstream *q, int reset);
int pqps_qstream_destroy(pqps_qstream *q);

/* The same with the SLOT named by the caller (0 .. depth-1) instead of call number % depth: what an engine with
 * several host threads needs -- a thread takes a free slot, issues, waits for THAT slot and reads its result, while
 * other threads do the same on other slots (the reference's OpenMP driver, QPEOMP.c:234-291).  Issuing calls on one
 * query stream must not overlap (the caller serialises them, e.g. under a mutex: they take microseconds);
 * pqps_qstream_wait may run concurrently with anything.  A slot is reused only after its query has been waited for.
 * Tables of 537 M rows and more use ONE lane (their launches keep expanders among the scan tiles, the tail is a few
 * percent of the launch, and two launches side by side lose more than the overlap gains). */
int pqps_qstream_scan_slot(pqps_qstream *q, uint32_t slot, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, uint32_t id_base,
                           const pqps_predicate *pred, uint32_t *out_ids, uint64_t out_capacity, uint64_t *out_count, void *scan_stream);
int pqps_qstream_count_slot(pqps_qstream *q, uint32_t slot, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows,
                            const pqps_predicate *pred, uint64_t *out_count, void *scan_stream);
/* Host wait for the query of ONE slot; reports (once) a launch OF THIS SLOT whose bounded waits ran out (the launches are
 * told apart by their epochs: two slots' queries may have run on the same lane). */
int pqps_qstream_wait(pqps_qstream *q, uint32_t slot);
/* A query that is more than one filter call (index probes + gather filters, flag passes in front of the last pass):
 * pqps_qstream_lane hands out the lane context + HIP stream the slot's query is to run on (call the pqps_filter_* /
 * pqps_index_probe functions with them), pqps_qstream_mark records its end on that stream. */
int pqps_qstream_lane(pqps_qstream *q, uint32_t slot, uint64_t n_rows, void *scan_stream, pqps_ctx **lane_ctx, void **lane_stream);
int pqps_qstream_mark(pqps_qstream *q, uint32_t slot);
/* Takes the lanes' scratch (hand-off words, slots, the 2-bytes-per-row list area of ID scans) for tables of up to n_rows rows
 * now rather than inside the first queries. */
int pqps_qstream_reserve(pqps_qstream *q, uint64_t n_rows);
/* Test hook: marks the slot's ID launch as one whose bounded waits ran out, the way the kernel does (its epoch in the lane's
 * status words).  pqps_qstream_wait(slot) must report it -- once -- and no other slot's wait may. */
int pqps_qstream_test_fail_slot(pqps_qstream *q, uint32_t slot);
/* Per-launch timing of the queries AS THEY RUN IN THE STREAM (two in flight): the lanes' own recorders, events on
 * the dispatch packets (recording does not change how the launches overlap).  pqps_qstream_kernel_time = the sums of
 * pqps_ctx_kernel_time over the lanes. */
int pqps_qstream_set_timing(pqps_qstream *q, int enable);
int pqps_qstream_kernel_time(pqps_qstream *q, double *eval_ms, double *total_ms, int *launches);

/* ---- multi-GPU SELECT: shard scan + all-gatherv of the matching row IDs over RCCL, one host call per query ----
 * Replaces the exchange step of engine/mpi/executeEngine-mpi.c:717-768 and keeps its shape: local scan of
 * the rank's row range, MPI_Allgather of the sizes (:753), displacements = exclusive prefix (:758-762),
 * MPI_Allgatherv of the payload (:765).  RCCL has no all-gatherv: the sizes travel in an 8-byte-per-rank
 * ncclAllGather, the payload as ONE group of ncclSend / ncclRecv of exactly count[r] IDs between every pair of
 * ranks, landing at its displacement -- nothing padded on the wire, no compaction pass, and no receive buffer
 * that could be too small (the gathered list is grown to the sizes before the payload moves).
 * WIRE FORM.  An answer of 32 768 matches and more (below that latency, not bytes, is the cost -- PQPS_WIRE_MIN_IDS moves the
 * floor) and of more than ~2 matches per 65 536 rows travels in compact form: the low 16 bits of every row number
 * (relative to the shard's first row) + one u32 per 65 536-row group saying where the group's entries begin -- 2 bytes per
 * match + 4 per group instead of 4 per match; the receiving GPU rebuilds the u32 IDs at the displacement (one copy kernel
 * for all the peers of a query).
 * The sender decides from its own count; the 32-byte-per-rank sizes all-gather carries (reported count, rows, first row,
 * form), so every receiver sizes its receives alike.  PQPS_EXCHANGE_COMPACT=0: always u32 (A/B runs, tests).
 * BOUNDED WAITS.  Every host wait of the exchange (a ring slot, the sizes, a result, pqps_exchange_sync) ends after
 * PQPS_EXCHANGE_TIMEOUT_S seconds (default 30; 0 = unbounded): the communicator is aborted (ncclCommAbort -- which also
 * ends the peers' matching calls), the call returns PQPS_ETIMEOUT and so does every later call on this exchange; the host
 * falls back to another exchange path or tears down.  Nothing of this re-starts a process that holds the GPU.
 * One process per GPU; every rank makes the same calls in the same order.  RCCL is loaded at run time from
 * `rccl_library` (e.g. the librccl.so of the process's torch build, or /opt/rocm/lib/librccl.so); the
 * 128-byte id is produced on rank 0 and handed to the other ranks by whatever bootstrap the host has
 * (torch.distributed broadcast, MPI_Bcast, a file).
 *
 * Bring-up in two steps so that a rank that fails locally cannot leave the others blocked:
 *   pqps_exchange_prepare   everything local (library, stream, buffers, scratch contexts); no communication
 *   (the host's bootstrap agrees that every rank prepared)
 *   pqps_exchange_connect   ncclCommInitRank -- returns once every rank of the world has called it
 * pqps_exchange_create = prepare + connect, for a host that has no such agreement step.
 *
 * pqps_exchange_select(x, ..., slot, scan_stream) enqueues, without blocking on the device:
 *   scan_stream     : the filter launch, writing [count | IDs] into ring slot `slot` (`slot_capacity` IDs: give it
 *                     the shard's row count and it can never be too small)
 *   exchange stream : (behind an event) the all-gather of the sizes and their copy to the host
 * -- after it has finished an EARLIER query: waited on the host for that query's sizes and enqueued its send /
 * recv group.  With a ring of 5 or more slots that is the query three calls back, whose scan ended while the two
 * scans in flight ran: the call does not block and both scan lanes stay supplied (a ring of 4 finishes the query
 * two calls back, a shorter one the previous query -- each step shorter makes the call wait for a scan that is
 * still running).  A slot may be reused after `ring` further calls; reuse waits on the host for the earlier
 * exchange.  pqps_exchange_result() finishes the slot if need be, waits for it and returns
 * the device pointer of the gathered ascending ID list (identical on every rank; valid until the slot is used
 * again), totals[0] = IDs gathered, totals[1] = IDs reported; PQPS_EOVERFLOW if a rank's own slot was too small. */
typedef struct { char internal[128]; } pqps_rccl_id;     /* = ncclUniqueId */
typedef struct pqps_exchange pqps_exchange;
int pqps_exchange_unique_id(const char *rccl_library, pqps_rccl_id *id);
int pqps_exchange_prepare(pqps_ctx *ctx, const char *rccl_library, uint32_t world, uint32_t rank,
                          uint64_t slot_capacity, uint32_t ring, pqps_exchange **out);
int pqps_exchange_connect(pqps_exchange *x, const pqps_rccl_id *id);
int pqps_exchange_create(pqps_ctx *ctx, const char *rccl_library, const pqps_rccl_id *id, uint32_t world,
                         uint32_t rank, uint64_t slot_capacity, uint32_t ring, pqps_exchange **out);
int pqps_exchange_select(pqps_exchange *x, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows,
                         uint32_t id_base, const pqps_predicate *pred, uint32_t slot, void *scan_stream);
/* COUNT(*) across the shards: local count kernel + ncclAllReduce(sum, 1 x u64)
 * (engine/mpi/executeEngine-mpi.c:745).  pqps_exchange_result() then reports totals[0] = the global
 * count, *local_count = this rank's; the merged pointer is meaningless for such a slot. */
int pqps_exchange_count(pqps_exchange *x, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows,
                        const pqps_predicate *pred, uint32_t slot, void *scan_stream);
int pqps_exchange_result(pqps_exchange *x, uint32_t slot, const uint32_t **merged_dev, uint64_t *local_count,
                         uint64_t totals[2]);
/* Finishes every query handed in so far (enqueues the payload groups still held back) and waits for the
 * exchange stream: call it before stopping a clock or tearing down. */
int pqps_exchange_sync(pqps_exchange *x);
/* Host time (ns) spent waiting -- for a ring slot to come free or for the sizes of a query -- as opposed to
 * time inside runtime / RCCL calls; `reset` != 0 clears the counter. */
uint64_t pqps_exchange_wait_ns(pqps_exchange *x, int reset);
/* The compact wire form by itself, for a host that moves the payload with its own collectives (merge.py over
 * torch.distributed): pqps_wire_pack reads a slot as the filter left it ([u64 count][u64][u32 IDs ...], `capacity` IDs), writes
 * this rank's four header words (reported count, rows, first row, form: 1 = compact) to header_dev and -- if `enabled` and
 * the compact form pays (pqps_wire_pays: >= 32 768 IDs and fewer bytes) -- the payload [u32 goff[groups + 1], padded to 16 bytes][u16 low[n]] to
 * `wire` (room for pqps_wire_bytes(n_rows, min(capacity, n_rows))); pqps_wire_expand turns a received payload into u32 IDs
 * at out_ids (the list's displacement in the gathered list). */
uint64_t pqps_wire_bytes(uint64_t n_rows, uint64_t n_ids);
int pqps_wire_pays(uint64_t n_rows, uint64_t n_ids);
int pqps_wire_pack(pqps_ctx *ctx, const uint32_t *slot, uint64_t capacity, uint64_t n_rows, uint32_t id_base, int enabled,
                   uint64_t *header_dev, void *wire, void *stream);
int pqps_wire_expand(pqps_ctx *ctx, const void *wire, uint64_t n_rows, uint32_t id_base, uint32_t *out_ids, void *stream);
/* Payload bytes this rank has RECEIVED from its peers so far: out[0] as they travelled (compact or u32), out[1] what the
 * same lists are as u32 IDs; `reset` != 0 clears both. */
void pqps_exchange_wire_bytes(pqps_exchange *x, uint64_t out[2], int reset);
/* SMALL ANSWERS IN ONE COLLECTIVE.  Behind each rank's 32-byte header the sizes all-gather of a SELECT has room for
 * PQPS_EXCHANGE_EAGER_IDS row numbers (default 16 384 = 64 KB per rank; 0: none; the smallest setting and the smallest slot of
 * the world win, agreed at connect; at most 4 MB gathered per query): a rank whose list fits puts it there, and when EVERY
 * rank's list fits the answer is complete after that one all-gather and one copy kernel -- no send / recv group, no size on
 * the host first.  When a list does not fit the query takes the two steps described above, and the next SELECT gathers bare
 * headers again until an answer that would have fitted has been seen (every rank reads the same sizes at the same point of its
 * call sequence, so all take the same turn).  out[0] = SELECTs that finished in the one collective, out[1] = SELECTs
 * finished, out[2] = the room agreed on (IDs per rank; 0 = off). */
void pqps_exchange_eager(pqps_exchange *x, uint64_t out[3], int reset);
int pqps_exchange_destroy(pqps_exchange *x);

/* ---- grouped COUNT(*): how many matching rows carry each value of one column ----------------------------------------
 * No counterpart in the reference (its engines have no aggregates).  The BIN of a row is (value - bin_base) in 32-bit
 * arithmetic: the dictionary code of a string column (bin_base 0), the value minus the column's minimum for an i32 column,
 * 0 / 1 for a boolean column.  bins[0 .. n_bins) are u32 device words; rows whose bin is >= n_bins are not counted.  All three
 * calls are asynchronous on `stream`; n_bins above 65 536 (or 0) returns PQPS_EINVAL.
 *
 * pqps_filter_group: COUNT(*) of `pred` over rows [0, n_rows) of `cols`, grouped by `group_col` -- ONE scan that evaluates the
 *   WHERE and builds the histogram (the group column is read only in steps of 1024 rows that hold a match).  `group_col`
 *   1, 2 or 4 bytes wide or a bit plane (PQPS_WIDTH_BITS).  The bins are zeroed by the call.  The readable-padding rule of
 *   pqps_filter_scan applies to the predicate columns AND to `group_col`.  D <= 16 bins: per-lane counters; D <= 16 384: a
 *   histogram in LDS; up to 65 536: atomics straight into the bins (slow: a path for correctness at high cardinality).
 *   The context's timing recorder (pqps_ctx_set_timing) records the launch like a COUNT's.
 * pqps_group_list: the same bins over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base < n_rows --
 *   by gathering `group_col` (1, 2 or 4 bytes wide, no bit plane).  The bins are zeroed by the call.
 * pqps_column_bounds: out_dev[0] = minimum, out_dev[1] = maximum of rows [0, n_rows) of a 4-byte column read as signed i32
 *   (device memory, two words; INT32_MAX / INT32_MIN for no rows). */
int pqps_filter_group(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                      const pqps_column *group_col, uint32_t bin_base, uint32_t n_bins, uint32_t *bins, void *stream);
int pqps_group_list(pqps_ctx *ctx, const pqps_column *group_col, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                    uint64_t capacity, uint32_t id_base, uint32_t bin_base, uint32_t n_bins, uint32_t *bins, void *stream);
int pqps_column_bounds(pqps_ctx *ctx, const pqps_column *col, uint64_t n_rows, int32_t *out_dev, void *stream);

/* ---- COUNT / SUM / MIN / MAX of a value column, overall or per group ------------------------------------------------
 * No counterpart in the reference.  `value_col`: 4 bytes (read as signed i32) or 8 bytes (read as u64); a bit plane or a
 * byte column is never a value.  OUTPUT per call (one shard): out[4 * n_bins] u64 device words, field-major --
 *   out[0 * n_bins + b]  count of the matching rows of bin b
 *   out[1 * n_bins + b]  sum of their values, sign-extended (i32) or as is (u64), mod 2^64
 *   out[2 * n_bins + b]  minimum of their IMAGES, out[3 * n_bins + b] maximum: the image of an i32 value v is
 *                        (uint64_t)(int64_t)v ^ 2^63, of a u64 value the value itself (unsigned order either way)
 * A bin without rows reads count 0, sum 0, min image UINT64_MAX, max image 0.  The bins are those of pqps_filter_group
 * ((value - bin_base) in 32-bit arithmetic, rows whose bin is >= n_bins are left out); `group_col` NULL means no GROUP BY:
 * n_bins must be 1 and every matching row is bin 0.  The calls initialise `out` themselves and are asynchronous on `stream`.
 *
 * pqps_filter_aggregate: ONE scan of `pred` over rows [0, n_rows) of `cols` (the value column, and the group column, are
 *   read only in steps of 1024 rows that hold a match).  `group_col` 1, 2 or 4 bytes wide or a bit plane.  The readable-
 *   padding rule of pqps_filter_scan applies to the predicate columns, `value_col` and `group_col`.  No GROUP BY: per-lane
 *   registers; D <= 2304 bins: a table in LDS; up to 65 536: atomics straight into `out` (slow: a correctness path).  The
 *   context's timing recorder records the launch like a COUNT's.
 * pqps_aggregate_list: the same over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base < n_rows --
 *   gathering `value_col` and `group_col` (1, 2 or 4 bytes wide, no bit plane) per listed row. */
int pqps_filter_aggregate(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                          const pqps_column *value_col, const pqps_column *group_col, uint32_t bin_base, uint32_t n_bins,
                          uint64_t *out, void *stream);
int pqps_aggregate_list(pqps_ctx *ctx, const pqps_column *value_col, const pqps_column *group_col, uint64_t n_rows,
                        const uint32_t *ids, const uint64_t *count_dev, uint64_t capacity, uint32_t id_base, uint32_t bin_base,
                        uint32_t n_bins, uint64_t *out, void *stream);

/* ---- GROUP BY buckets: COUNT(*) and COUNT / SUM / MIN / MAX per run of bins -------------------------------------------
 * No counterpart in the reference.  A BUCKET is a contiguous run of the bins of pqps_filter_group ((value - bin_base) in
 * 32-bit arithmetic): the codes of the strings that share a prefix, the values of one range of an i32 column.  `bounds_dev`
 * holds n_buckets + 1 u32 device words, the ascending run starts in bin space: bounds[0] == 0, strictly ascending,
 * bounds[n_buckets] == `domain` (hipBucketBounds makes them).  The bucket of a row with bin b is
 *     (number of entries of bounds[0 .. n_buckets] that are <= b) - 1,
 * and a row whose bucket is >= n_buckets is left out: exactly the rows with b >= domain.  Whatever `bounds_dev` holds,
 * nothing outside the output is written.  The four calls are asynchronous on `stream`, initialise their output themselves
 * and return PQPS_EINVAL for n_buckets 0 or above 65 536, a NULL `bounds_dev`, and `domain` 0 or below n_buckets.
 *
 * pqps_filter_group_buckets: pqps_filter_group per bucket -- ONE scan; `group_col` 1, 2 or 4 bytes wide (no bit plane), read
 *   only in steps that hold a match; bins[0 .. n_buckets) u32 device words.  The readable-padding rule of pqps_filter_scan
 *   applies to the predicate columns and `group_col`.  The bounds sit in LDS while they fit beside the bins (a workgroup
 *   takes at most 64 KiB); n_buckets <= 16: per-lane counters; <= 8191: a histogram in LDS; up to 65 536: atomics straight
 *   into the bins (a correctness path), with the bounds in LDS up to 16 383 buckets and read from global memory above.
 * pqps_group_buckets_list: the same over an ID list, as pqps_group_list.
 * pqps_filter_aggregate_buckets: pqps_filter_aggregate per bucket; `value_col` 4 bytes (signed i32) or 8 bytes (u64);
 *   out[4 * n_buckets] u64 device words in that call's field-major layout, images and empty-bin values (0, 0, UINT64_MAX,
 *   0).  n_buckets <= 2047: a table in LDS beside the bounds; above: atomics straight into `out`, bounds as above.
 * pqps_aggregate_buckets_list: the same over an ID list, as pqps_aggregate_list. */
int pqps_filter_group_buckets(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                              const pqps_column *group_col, uint32_t bin_base, const uint32_t *bounds_dev, uint32_t n_buckets,
                              uint32_t domain, uint32_t *bins, void *stream);
int pqps_group_buckets_list(pqps_ctx *ctx, const pqps_column *group_col, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                            uint64_t capacity, uint32_t id_base, uint32_t bin_base, const uint32_t *bounds_dev, uint32_t n_buckets,
                            uint32_t domain, uint32_t *bins, void *stream);
int pqps_filter_aggregate_buckets(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                                  const pqps_column *value_col, const pqps_column *group_col, uint32_t bin_base,
                                  const uint32_t *bounds_dev, uint32_t n_buckets, uint32_t domain, uint64_t *out, void *stream);
int pqps_aggregate_buckets_list(pqps_ctx *ctx, const pqps_column *value_col, const pqps_column *group_col, uint64_t n_rows,
                                const uint32_t *ids, const uint64_t *count_dev, uint64_t capacity, uint32_t id_base, uint32_t bin_base,
                                const uint32_t *bounds_dev, uint32_t n_buckets, uint32_t domain, uint64_t *out, void *stream);

/* ---- ORDER BY column [DESC] LIMIT K ------------------------------------------------------------------------------
 * No counterpart in the reference (it parses ORDER BY and executes none).  KEYS: every row is one composite key whose
 * ascending unsigned order is the answer's order -- the column's order-preserving image ascending (descending with
 * `descending`), ties by ascending table-wide row number (row_base / id_base + local row):
 *   key_col 1, 2 or 4 bytes wide, or a bit plane: one u64 per key, (img ^ x) << 32 | row, img = v ^ 2^31 when key_signed
 *     (i32), the value itself otherwise (dictionary codes, the bool byte or bit), x = 0xFFFFFFFF when descending, else 0
 *   key_col 8 bytes wide (command_id, unsigned): two u64 per key, (v ^ x, row), x = ~0 when descending, else 0
 *   key_col NULL: every value 0 (a single-valued column), the order is the row order.
 * OUTPUT (pqps_filter_topk / pqps_topk_list): out[0 .. k) keys (k or 2 k u64 words), ascending; of M candidates only the
 * first min(k, M) are real, the rest read all ones.  K = 1 .. PQPS_TOPK_MAX (PQPS_TOPK_MAX_WIDE for 8-byte keys).  Row
 * numbers stay below 2^32 - 1.  `scratch`: device memory of at least pqps_topk_scratch_bytes(ctx, n, k, wide, fused)
 * bytes (n = n_rows of the fused scan, the list length otherwise) that nothing else uses until the call's work is done --
 * the engine allocates it per query, so no two queries ever share it.  Asynchronous on `stream`.
 *
 * pqps_filter_topk: ONE scan of `pred` over rows [0, n_rows) (the key column read only in steps of 1024 rows that hold a
 *   match; the readable-padding rule of pqps_filter_scan applies to it), each wave keeping its K best in LDS, then a few
 *   small rounds that reduce the waves' partial rows to K.  *count (device) = the matching rows.  Recorded by the
 *   context's timing recorder like a COUNT (the scan's start to the last round's end).
 * pqps_topk_list: the same selection over ids[0 .. n) (table-wide rows, local row = id - id_base), keys gathered per
 *   entry -- an entry listed twice is a candidate twice.  key_col 1, 2, 4 or 8 bytes wide (no bit plane).
 * pqps_sort_list: the whole list in that order: out_ids[0 .. n) the rows, out_keys[0 .. n) (may be NULL) their sort keys
 *   as u64 (narrow: (img ^ x) zero-extended; wide: v ^ x).  Two stable radix sorts (rows, then keys).  Synchronous. */
#define PQPS_TOPK_MAX 1024u
#define PQPS_TOPK_MAX_WIDE 512u
uint64_t pqps_topk_scratch_bytes(pqps_ctx *ctx, uint64_t n, uint32_t k, int wide, int fused);
int pqps_filter_topk(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                     const pqps_column *key_col, int key_signed, int descending, uint32_t row_base, uint32_t k,
                     void *scratch, uint64_t scratch_bytes, uint64_t *out, uint64_t *count, void *stream);
int pqps_topk_list(pqps_ctx *ctx, const pqps_column *key_col, int key_signed, int descending, const uint32_t *ids, uint64_t n,
                   uint32_t id_base, uint32_t k, void *scratch, uint64_t scratch_bytes, uint64_t *out, void *stream);
int pqps_sort_list(pqps_ctx *ctx, const pqps_column *key_col, int key_signed, int descending, const uint32_t *ids, uint64_t n,
                   uint32_t id_base, uint32_t *out_ids, uint64_t *out_keys, void *stream);

/* ---- ORDER BY k1 [DESC], ... , kN [DESC] LIMIT K: several columns packed into one key ------------------------------
 * Field j (j = 0 the most significant) of a row whose column holds v:
 *     bin = v - base (32-bit arithmetic)     field = min(bin, 2^bits - 1) ^ (descending ? 2^bits - 1 : 0)
 *     packed = OR of field_j << shift_j
 * The caller chooses base and bits so that every bin fits (base = the column's lowest value as u32 for an i32 column, else
 * 0; bits = ceil(log2(domain))) and the shifts so that the fields do not overlap and earlier fields lie higher; a value
 * outside its domain is clamped into its own field.  T = the highest bit any field reaches (max of shift + bits):
 *     T <= 32   narrow keys, one u64: packed << 32 | row          K = 1 .. PQPS_TOPK_MAX
 *     T <= 64   wide keys, two u64: (packed, row)                 K = 1 .. PQPS_TOPK_MAX_WIDE
 * exactly the key forms, outputs and scratch rule (pqps_topk_scratch_bytes, wide = T > 32) of the one-column calls above;
 * ties in every field go to the ascending row number.  Field columns are 1, 2 or 4 bytes wide; pqps_filter_topk_multi also
 * takes bit planes.  PQPS_EINVAL: n_fields outside 1 .. PQPS_ORDER_MAX_FIELDS, a field of more than 32 bits, a field that
 * ends past bit 64 (so T > 64), overlapping fields, K over the form's bound, a bit plane in a list call.
 * pqps_filter_topk_multi: as pqps_filter_topk, every field's column read in the steps that hold a match.
 * pqps_topk_list_multi:   the selection of pqps_topk_list, but SYNCHRONOUS: the keys of the list are packed into a temporary
 *   of n keys that the call allocates, waits for and frees (one hipMalloc, one stream synchronize, one hipFree per call).
 * pqps_sort_list_multi:   as pqps_sort_list; out_keys (may be NULL) = the packed word of every row as u64.
 * pqps_sort_list_chain:   the order of 1 .. PQPS_ORDER_MAX_FIELDS whole one-column keys (as pqps_sort_list takes them: 1, 2, 4
 *   or 8 bytes wide), for key lists that fit no packed key: one stable radix sort by row, then one per key from the last
 *   to the first.  out_keys (may be NULL): n_keys arrays of n u64, array j = key j's image (pqps_sort_list's) of every
 *   row of out_ids -- ascending (image 0, ..., image N-1, row) is the answer's order.  Synchronous. */
#define PQPS_ORDER_MAX_FIELDS 4u
typedef struct pqps_order_field {
    pqps_column col;
    uint32_t base, bits, shift;
    int descending;
} pqps_order_field;
int pqps_filter_topk_multi(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                           const pqps_order_field *fields, uint32_t n_fields, uint32_t row_base, uint32_t k,
                           void *scratch, uint64_t scratch_bytes, uint64_t *out, uint64_t *count, void *stream);
int pqps_topk_list_multi(pqps_ctx *ctx, const pqps_order_field *fields, uint32_t n_fields, const uint32_t *ids, uint64_t n,
                         uint32_t id_base, uint32_t k, void *scratch, uint64_t scratch_bytes, uint64_t *out, void *stream);
int pqps_sort_list_multi(pqps_ctx *ctx, const pqps_order_field *fields, uint32_t n_fields, const uint32_t *ids, uint64_t n,
                         uint32_t id_base, uint32_t *out_ids, uint64_t *out_keys, void *stream);
int pqps_sort_list_chain(pqps_ctx *ctx, const pqps_column *key_cols, const int *key_signed, const int *descending, uint32_t n_keys,
                         const uint32_t *ids, uint64_t n, uint32_t id_base, uint32_t *out_ids, uint64_t *out_keys, void *stream);

/* ---- the first row of every group: per bin, the matching row that comes first in the order of a key column -------------
 * No counterpart in the reference (SQL: DISTINCT ON, ROW_NUMBER() OVER (PARTITION BY g ORDER BY k) = 1, argMin / argMax).
 * BINS: those of pqps_filter_group ((value - bin_base) in 32-bit arithmetic; rows whose bin is >= n_bins are left out);
 * `group_col` NULL means no GROUP BY: n_bins must be 1 and every matching row is bin 0.  n_bins 1 .. 65 536.
 * ORDER: that of the top-K family above -- the key column's image ascending (descending with `descending`), ties by
 * ascending table-wide row number (row_base / id_base + local row) in BOTH directions.  Row numbers stay below 2^32 - 1.
 * WORDS: out[0 .. n_bins) u64 device words, one per bin; all ones = the bin has no row.
 *   key_col 1, 2 or 4 bytes wide, or a bit plane: out[b] = the MINIMUM over the bin's rows of the top-K key
 *     (img ^ x) << 32 | row, img = v ^ 2^31 when key_signed (i32), the value itself otherwise, x = 0xFFFFFFFF when
 *     descending, else 0 (hipFirstKeyDecode of hipPredicate.h undoes it); `best` is not used and may be NULL
 *   key_col NULL: every value 0 (a single-valued column): out[b] = the lowest matching row of the bin
 *   key_col 8 bytes wide (command_id, unsigned): 96 bits do not fit one atomic, so the call runs TWO passes over the rows
 *     (two scans of the WHERE): best[b] = the minimum of v ^ x (x = ~0 when descending, else 0), then out[b] = the lowest
 *     row among the bin's rows whose v ^ x equals best[b].  `best` (n_bins u64 device words) is required; best[b] means
 *     something only where out[b] is not all ones.
 * The calls initialise `out`, `best` and `*count` themselves and are asynchronous on `stream`.  No scratch argument: the
 * partial rows of the fused scan live in the context's fused-scan scratch, which the call grows as pqps_filter_aggregate
 * does (one fused query at a time per context, as for its siblings).
 *
 * pqps_filter_group_first: ONE scan of `pred` over rows [0, n_rows) of `cols` (two for an 8-byte key); the key column and the
 *   group column are read only in steps of 1024 rows that hold a match, and every matching row costs ONE 64-bit unsigned
 *   atomic min.  `group_col` 1, 2 or 4 bytes wide or a bit plane.  The readable-padding rule of pqps_filter_scan applies to
 *   the predicate columns, `key_col` and `group_col`.  No GROUP BY: per-lane minima; D <= 8192 bins: a table of 8 B per bin
 *   in LDS; up to 65 536: atomics straight into `out` (slow: a correctness path).  *count (device) = the matching rows,
 *   those of bins >= n_bins included.  The context's timing recorder records the launch like a COUNT's (an 8-byte key: two
 *   records).
 * pqps_group_first_list: the same words over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base <
 *   n_rows -- gathering `key_col` (1, 2, 4 or 8 bytes wide, no bit plane) and `group_col` (1, 2 or 4 bytes wide, no bit
 *   plane) per listed row; an id listed twice changes nothing.  capacity or n_rows 0: `out` all ones, nothing launched. */
int pqps_filter_group_first(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                            const pqps_column *key_col, int key_signed, int descending, uint32_t row_base,
                            const pqps_column *group_col, uint32_t bin_base, uint32_t n_bins, uint64_t *out, uint64_t *best,
                            uint64_t *count, void *stream);
int pqps_group_first_list(pqps_ctx *ctx, const pqps_column *key_col, int key_signed, int descending, const pqps_column *group_col,
                          uint32_t bin_base, uint32_t n_bins, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                          uint64_t capacity, uint32_t id_base, uint64_t *out, uint64_t *best, void *stream);

/* ---- the first N rows of every group: per bin, the N matching rows that come first in the order of a key column --------
 * No counterpart in the reference (SQL: ROW_NUMBER() OVER (PARTITION BY g ORDER BY k [DESC]) <= n).  BINS, ORDER and WORDS
 * are those of the first-row calls above.  A row's word is unique, so the r-th row of a bin is the minimum word strictly
 * above the bin's (r-1)-th word: the calls run `n_rounds` ROUNDS, round 0 the first-row call itself, round r >= 1 the same
 * scan with one more test per matching row (word > the bin's word of round r-1).
 * WORDS: out[n_rounds][n_bins] u64 device words, row r being round r: out[r][b] = the word of the bin's (r+1)-th row; all
 *   ones = the bin has fewer than r + 1 rows (and then every later round reads all ones too).  `best` has the same shape
 *   for an 8-byte key (command_id), else it is not used and may be NULL: each round of an 8-byte key is the two passes of
 *   the first-row call, with the floor the pair (best[r-1][b], out[r-1][b]).
 * n_rounds 1 .. PQPS_HEAD_ROUNDS_MAX.  The calls initialise `out`, `best` and `*count` and are asynchronous on `stream`:
 * ALL rounds are issued without a host wait, each round reading the previous one's words from device memory.
 *
 * pqps_filter_group_head: n_rounds scans of `pred` (twice that for an 8-byte key), columns, padding rule and scratch as
 *   pqps_filter_group_first.  The floor is one register without GROUP BY; for D <= 4096 bins of a narrow key it lies in
 *   LDS beside the min table (16 B per bin); otherwise it is read from device memory per matching row (D <= 8192: the min
 *   table alone in LDS; above: atomics straight into `out`).  *count (device) is written by round 0 only.  Every round is
 *   recorded by the context's timing recorder like a COUNT (an 8-byte key: two records per round).
 * pqps_group_head_list: the same words over an ID list, arguments as pqps_group_first_list; an id listed twice is ONE
 *   candidate in every round (the test is a strict >).
 *
 * The SORT form, for an N above the round cap, over a selection sorted by (group, key, row):
 * pqps_runs_head_flags: keep[i] = (i < limit) || (sorted_keys[i - limit] != sorted_keys[i]) for i < n: in a sorted array an
 *   entry has rank >= limit inside its run of equal keys exactly when the entry `limit` places before it is in the same
 *   run.  limit >= 1; n = 0 launches nothing.  Asynchronous.
 * pqps_group_head_sort: the whole sort form over ids[0 .. n) (table-wide rows, local row = id - id_base): the list sorted
 *   by (group image, key image [descending], row) (pqps_sort_list_chain; pqps_sort_list where a column is NULL = every
 *   value 0), ids listed twice removed where `repeats` says the list may hold some (adjacent after the sort), the first
 *   `limit` entries of every run of equal group images flagged (pqps_runs_head_flags), and the kept entries compacted in
 *   order by the scan's compaction, as pqps_compact_rows builds DELETE's keep list.  out_ids[0 .. *kept_out) = the rows,
 *   out_keys[0 .. *kept_out) = their group images and out_keys[n .. n + *kept_out) their key images (pqps_sort_list's
 *   u64 images; `group_signed` / `key_signed`: i32 columns).  out_ids holds n entries, out_keys 2 n.  Columns 1, 2, 4 bytes
 *   wide, the key column also 8.  Synchronous. */
#define PQPS_HEAD_ROUNDS_MAX 16u
int pqps_filter_group_head(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                           const pqps_column *key_col, int key_signed, int descending, uint32_t row_base,
                           const pqps_column *group_col, uint32_t bin_base, uint32_t n_bins, uint32_t n_rounds, uint64_t *out,
                           uint64_t *best, uint64_t *count, void *stream);
int pqps_group_head_list(pqps_ctx *ctx, const pqps_column *key_col, int key_signed, int descending, const pqps_column *group_col,
                         uint32_t bin_base, uint32_t n_bins, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                         uint64_t capacity, uint32_t id_base, uint32_t n_rounds, uint64_t *out, uint64_t *best, void *stream);
int pqps_runs_head_flags(pqps_ctx *ctx, const uint64_t *sorted_keys, uint64_t n, uint64_t limit, uint8_t *keep, void *stream);
int pqps_group_head_sort(pqps_ctx *ctx, const pqps_column *key_col, int key_signed, int descending, const pqps_column *group_col,
                         int group_signed, const uint32_t *ids, uint64_t n, uint32_t id_base, uint64_t limit, int repeats,
                         uint32_t *out_ids, uint64_t *out_keys, uint64_t *kept_out, void *stream);

/* ---- one pass of a radix select: per group, the histogram of one digit of a key under a prefix --------------------------
 * No counterpart in the reference.  What exact percentiles (SQL: PERCENTILE_DISC) are made of: a few counting scans instead
 * of a sort.  KEY IMAGE of a row: (uint32_t)(v - key_base) for a key column of 1, 2 or 4 bytes or a bit plane (key_wide 0;
 * the 32-bit wrap-around makes an i32 value minus the column's minimum monotone), v - key_base in 64 bits for an 8-byte
 * column (key_wide 1).  The caller promises image < 2^key_bits (key_bits 1 .. 32, or .. 64 when key_wide); a row whose image
 * has a bit at or above key_bits is left out and never indexes anything.
 * GROUPS: the bins of pqps_filter_group ((value - bin_base) in 32-bit arithmetic; rows whose bin is >= n_bins are left out, so
 * bin_base / n_bins is also a window onto a longer run of bins); `group_col` NULL means no GROUP BY: n_bins must be 1.
 * DIGIT: bits [shift, shift + digit_bits) of the image, digit_bits 1 .. PQPS_DIGIT_BITS_MAX, shift + digit_bits <= key_bits.
 * PREFIXES: prefix_dev NULL (the first pass): `slots` must be 1 and the table of a row is its group bin.  Otherwise
 *   prefix_dev[(bin * slots) + j], j < slots (1 .. PQPS_DIGIT_SLOTS_MAX), are u64 device words: the row counts into table
 *   t = bin * slots + j of the slot whose word equals image >> (shift + digit_bits), and is left out when none does.  All
 *   ones marks an unused slot; the slots of one group hold distinct words.
 * OUTPUT: tables_dev[n_bins * slots][2^digit_bits] u32 device counts, at most PQPS_DIGIT_WORDS_MAX words in all, zeroed by the
 *   call: tables_dev[t * 2^digit_bits + digit] = the matching rows of table t with that digit.  Asynchronous on `stream`.
 *
 * pqps_filter_digit_hist: ONE scan of `pred` over rows [0, n_rows) of `cols`; the key column and the group column are read
 *   only in steps of 1024 rows that hold a match (the readable-padding rule of pqps_filter_scan applies to both; `group_col`
 *   1, 2 or 4 bytes wide or a bit plane).  Up to 16 384 counts (8 tables of 11 bits, 64 of 8 bits): tables in LDS, a partial
 *   row per workgroup, summed by a second launch; above: one global atomic per matching row.  Scratch as
 *   pqps_filter_group_first; the context's timing recorder records the launch like a COUNT's.
 * pqps_digit_hist_list: the same tables over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base < n_rows
 *   -- gathering `key_col` (1, 2, 4 or 8 bytes wide) and `group_col` (1, 2 or 4 bytes wide) per listed row, no bit planes; an
 *   id listed twice is counted twice.  capacity or n_rows 0: the tables zeroed, nothing launched. */
#define PQPS_DIGIT_BITS_MAX 11u
#define PQPS_DIGIT_SLOTS_MAX 16u
#define PQPS_DIGIT_WORDS_MAX (1u << 22)
int pqps_filter_digit_hist(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                           const pqps_column *key_col, int key_wide, uint64_t key_base, uint32_t key_bits, const pqps_column *group_col,
                           uint32_t bin_base, uint32_t n_bins, uint32_t slots, const uint64_t *prefix_dev, uint32_t shift,
                           uint32_t digit_bits, uint32_t *tables_dev, void *stream);
int pqps_digit_hist_list(pqps_ctx *ctx, const pqps_column *key_col, int key_wide, uint64_t key_base, uint32_t key_bits,
                         const pqps_column *group_col, uint32_t bin_base, uint32_t n_bins, uint32_t slots, const uint64_t *prefix_dev,
                         uint32_t shift, uint32_t digit_bits, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                         uint64_t capacity, uint32_t id_base, uint32_t *tables_dev, void *stream);

/* ---- COUNT(DISTINCT value column), overall or per group ---------------------------------------------------------------
 * No counterpart in the reference.  BINS: a value bin is (value - v_base) in 32-bit arithmetic (dictionary codes with
 * v_base 0, an i32 value minus the column's minimum, the bool byte or bit), a group bin (value - g_base) likewise;
 * `group_col` NULL means no GROUP BY (n_groups must be 1, every matching row is group 0).  Rows whose value bin is >=
 * n_values or whose group bin is >= n_groups are left out.  BITMAP (device, u32 words): n_groups rows of
 * W = ceil(n_values / 32) words, pqps_distinct_bitmap_words(n_values, n_groups) in all; bit v of row g set iff a matching
 * row has group bin g and value bin v.  The bitmap forms take n_groups x W x 32 <= 2^30 bits (128 MiB) -- wider domains
 * go through pqps_distinct_sort.  `distinct` (device, n_groups u64; may be NULL where noted): the popcount of every row.
 * The calls initialise their outputs themselves.
 *
 * pqps_filter_distinct: ONE scan of `pred` over rows [0, n_rows) of `cols` (the value and group columns read only in steps
 *   of 1024 rows that hold a match; 1, 2, 4 bytes wide or a bit plane; the readable-padding rule of pqps_filter_scan
 *   applies to both).  n_groups x n_values <= 64: per-lane registers; a bitmap of up to 16 384 words: dynamic LDS; larger:
 *   test-before-set atomics on `bitmap` (a correctness path).  *total (device) = the matching rows.  `distinct` non-NULL:
 *   the popcount pass too.  Asynchronous on `stream`; the context's timing recorder records it like a COUNT's (the scan's
 *   start to the last launch's end).
 * pqps_distinct_list: the same bitmap over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base < n_rows --
 *   gathering both columns (1, 2 or 4 bytes wide, no bit plane) per listed row.  Asynchronous.
 * pqps_distinct_count: distinct[g] = the popcount of row g of a bitmap (e.g. the OR of several shards').  Asynchronous.
 * pqps_distinct_sort: the sort form for any domain, command_id (8 bytes, unsigned) included: the listed rows' (group,
 *   value) keys sorted by the stable LSD radix sort, distinct[g] = the keys of group g that differ from their predecessor.
 *   `out_keys` (may be NULL) receives the sorted keys -- narrow values: n u64 (group bin << 32 | value bin); 8-byte values:
 *   n u64 values followed by n u32 group bins (group-major, values ascending within a group).  A listed row whose group bin
 *   is >= n_groups is not counted; in `out_keys` it carries a group bin >= n_groups and sorts behind the rows of every group.
 *   Its scratch is allocated and freed by the call.  Synchronous. */
uint64_t pqps_distinct_bitmap_words(uint32_t n_values, uint32_t n_groups);
int pqps_filter_distinct(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                         const pqps_column *value_col, uint32_t v_base, uint32_t n_values, const pqps_column *group_col,
                         uint32_t g_base, uint32_t n_groups, uint32_t *bitmap, uint64_t *total, uint64_t *distinct, void *stream);
int pqps_distinct_list(pqps_ctx *ctx, const pqps_column *value_col, uint32_t v_base, uint32_t n_values, const pqps_column *group_col,
                       uint32_t g_base, uint32_t n_groups, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                       uint64_t capacity, uint32_t id_base, uint32_t *bitmap, uint64_t *distinct, void *stream);
int pqps_distinct_count(pqps_ctx *ctx, const uint32_t *bitmap, uint32_t n_values, uint32_t n_groups, uint64_t *distinct, void *stream);
int pqps_distinct_sort(pqps_ctx *ctx, const pqps_column *value_col, uint32_t v_base, const pqps_column *group_col, uint32_t g_base,
                       uint32_t n_groups, const uint32_t *ids, uint64_t n, uint32_t id_base, uint64_t *distinct, uint64_t *out_keys,
                       void *stream);

/* ---- GROUP BY two columns: COUNT(*), or COUNT / SUM / MIN / MAX of a value column, per pair of values ---------------------
 * No counterpart in the reference.  BINS: each group column has the bins of pqps_filter_group -- bin_a = (value of A - a_base),
 * bin_b = (value of B - b_base) in 32-bit arithmetic, n_a and n_b of them (1 .. 65 536 each); a row whose bin_a >= n_a or
 * bin_b >= n_b is left out.  The bin of a row is bin_a * n_b + bin_b, D = n_a x n_b bins in all -- a 64-bit product: the
 * two dense calls take D = 1 .. 65 536 and return PQPS_EINVAL for anything else (n_a or n_b 0 included), the sort call
 * takes any D.  `value_col` NULL: COUNT(*) only; otherwise 4 bytes (signed i32) or 8 bytes (u64), as pqps_filter_aggregate.
 * DENSE OUTPUT (`out`, device): without a value column D u32 counts, as pqps_filter_group's bins; with one the [4][D] u64
 * fields of pqps_filter_aggregate (counts, sums, min images, max images; a bin without rows reads 0, 0, UINT64_MAX, 0).  The
 * calls initialise `out` themselves and are asynchronous on `stream`.
 *
 * pqps_filter_group_pair: ONE scan of `pred` over rows [0, n_rows) of `cols`; A, B and the value column are read only in
 *   steps of 1024 rows that hold a match.  `a_col` / `b_col` 1, 2 or 4 bytes wide or a bit plane each; the readable-padding
 *   rule of pqps_filter_scan applies to the predicate columns, A, B and `value_col`.  COUNT(*): a u32 histogram in LDS for
 *   D <= 16 384, atomics straight into the bins above (slow: a correctness path).  With a value: the 28-byte-per-bin table
 *   in LDS for D <= 2304, four global 64-bit atomics per matching row above.  The context's timing recorder records the
 *   launch like a COUNT's.
 * pqps_group_pair_list: the same bins over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base; a row
 *   >= n_rows is skipped -- gathering A, B (1, 2 or 4 bytes wide, no bit plane) and the value per listed row.
 * pqps_group_pair_sort: the sparse form for any D, over ids[0 .. n) (n below 2^32 - 1): one u64 key per listed row,
 *   bin_a << 32 | bin_b (rows outside the bins or the table are left out), sorted with the row numbers by the stable LSD
 *   radix sort over the bytes in which the keys differ, then reduced run by run.  OUTPUT: *n_runs (host) = the pairs that
 *   occur, *runs_dev = device memory the call allocates (NULL for no runs; the caller frees it with pqps_free), compact and
 *   field-major, *n_runs u64 entries per field, ascending by key: keys, counts, and with a value column sums, min images,
 *   max images.  Its scratch is allocated and freed by the call.  Synchronous. */
int pqps_filter_group_pair(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                           const pqps_column *a_col, uint32_t a_base, uint32_t n_a, const pqps_column *b_col, uint32_t b_base,
                           uint32_t n_b, const pqps_column *value_col, void *out, void *stream);
int pqps_group_pair_list(pqps_ctx *ctx, const pqps_column *a_col, uint32_t a_base, uint32_t n_a, const pqps_column *b_col, uint32_t b_base,
                         uint32_t n_b, const pqps_column *value_col, uint64_t n_rows, const uint32_t *ids, const uint64_t *count_dev,
                         uint64_t capacity, uint32_t id_base, void *out, void *stream);
int pqps_group_pair_sort(pqps_ctx *ctx, const pqps_column *a_col, uint32_t a_base, uint32_t n_a, const pqps_column *b_col, uint32_t b_base,
                         uint32_t n_b, const pqps_column *value_col, uint64_t n_rows, const uint32_t *ids, uint64_t n, uint32_t id_base,
                         uint64_t **runs_dev, uint64_t *n_runs, void *stream);

/* ---- GROUP BY one column of any size: the wide bins, their compaction, and the sort form ------------------------------------
 * No counterpart in the reference.  What the top-N groups query runs above the 65 536 bins of pqps_filter_group and
 * pqps_filter_aggregate; those calls keep their limit.  BINS as theirs: (value - bin_base) in 32-bit arithmetic, a row whose
 * bin is not below n_bins is left out, and whatever the column holds nothing is indexed out of range.  `group_col` 1, 2 or 4
 * bytes wide (no bit plane); `value_col` NULL: COUNT(*) only, else 4 bytes (signed i32) or 8 bytes (u64).
 * DENSE OUTPUT (`out`, device, the caller's): without a value column n_bins u32 counts, with one the [4][n_bins] u64 fields of
 * pqps_filter_aggregate (counts, sums, min images, max images; a bin without rows reads 0, 0, UINT64_MAX, 0).
 * RUN FORMAT (pqps_bins_compact, pqps_group_sort): that of pqps_group_pair_sort with key = the bin -- *n_runs (host) = the bins
 *   that have rows, *runs_dev = device memory the call allocates (NULL for no runs; the caller frees it with pqps_free),
 *   field-major, *n_runs u64 entries per field, ascending by key: keys, counts, and with a value sums, min images, max images.
 *
 * pqps_filter_group_wide: ONE scan of `pred` over rows [0, n_rows) of `cols` into `out`, any n_bins >= 1; the group and the
 *   value column are read only in steps of 1024 rows that hold a match, the readable-padding rule of pqps_filter_scan applies
 *   to them (16-byte aligned).  Every workgroup keeps a write-combining FRONT in LDS before the global atomics: a direct-mapped
 *   table of PQPS_WIDE_COUNT_SLOTS (COUNT(*)) or PQPS_WIDE_VALUE_SLOTS slots, slot = bin mod slots, each a tag and an
 *   accumulator.  A row whose slot is free or holds its bin is added in LDS; any other row goes to `out` with one global
 *   atomic per field.  The first bin to arrive keeps its slot (no eviction); the workgroup ends by adding every claimed slot
 *   to `out`.  pqps_ctx_set_option(ctx, "wide_front", 0) runs without the front (global atomics alone; < 0: the default, on).
 *   The call initialises `out` and is asynchronous on `stream`; the timing recorder records the launch like a COUNT's.
 * pqps_group_wide_list: the same over an ID list -- ids[0 .. min(*count_dev, capacity)), row = id - id_base; a row >= n_rows
 *   is skipped -- gathering the columns per listed row (any alignment of `group_col`).
 * pqps_bins_compact: dense bins (`valued` != 0: the [4][n_bins] fields) into the run format, in two launches of waves that
 *   each take tiles of PQPS_COMPACT_TILE bins -- the bins with rows per tile, an exclusive scan, the writes; no workgroup
 *   waits for another.  Synchronous.
 * pqps_group_sort: the one-column form of pqps_group_pair_sort over ids[0 .. n) (n below 2^32 - 1), n_bins = 1 .. 2^32 as a
 *   64-bit count: one key per listed row (its bin; rows outside the bins or the table are left out), the same sort and the
 *   same run reduction.  Its runs equal pqps_bins_compact's of the same rows.  Synchronous. */
#define PQPS_COMPACT_TILE      1024u
#define PQPS_WIDE_COUNT_SLOTS  8192u
#define PQPS_WIDE_VALUE_SLOTS  2048u
int pqps_filter_group_wide(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                           const pqps_column *value_col, const pqps_column *group_col, uint32_t bin_base, uint32_t n_bins,
                           void *out, void *stream);
int pqps_group_wide_list(pqps_ctx *ctx, const pqps_column *value_col, const pqps_column *group_col, uint64_t n_rows,
                         const uint32_t *ids, const uint64_t *count_dev, uint64_t capacity, uint32_t id_base, uint32_t bin_base,
                         uint32_t n_bins, void *out, void *stream);
int pqps_bins_compact(pqps_ctx *ctx, const void *bins, uint32_t n_bins, int valued, uint64_t **runs_dev, uint64_t *n_runs, void *stream);
int pqps_group_sort(pqps_ctx *ctx, const pqps_column *group_col, uint32_t bin_base, uint64_t n_bins, const pqps_column *value_col,
                    uint64_t n_rows, const uint32_t *ids, uint64_t n, uint32_t id_base, uint64_t **runs_dev, uint64_t *n_runs, void *stream);

/* ---- HAVING: dense bins into the presence bitmap of a value set -------------------------------------------------------------
 * No counterpart in the reference.  pqps_bins_having turns the dense bins of a grouped scan into the bitmap pqps_member_flags
 * reads (PQPS_MEMBER_BITMAP with n_bits = n_bins), all on the device.
 * INPUT   `bins` (device): `valued` 0 -- the n_bins u32 counts of pqps_filter_group / pqps_filter_group_wide (`field` must be
 *         PQPS_HAVING_COUNT); otherwise the field-major [4][n_bins] u64 of pqps_filter_aggregate (counts, sums, min images,
 *         max images).  `field` PQPS_HAVING_COUNT / _SUM / _MIN / _MAX picks the compared row, `op` PQPS_HAVING_EQ .. _GE the
 *         comparison with `constant`: counts unsigned; sums as int64 when `value_signed`, else unsigned; MIN and MAX unsigned on
 *         IMAGES (the caller passes the constant as an image: (u64)(i64)v ^ 2^63 for an i32 value, v itself for command_id).
 * OUTPUT  bit b of `bitmap` (device, 8-byte aligned, u32 words, LSB first) = count[b] != 0 && field[b] OP constant: a bin
 *         without rows is never set.  All (n_bins + 31) / 32 words are written in full, the tail bits of the last word 0,
 *         nothing past them.  *members (device, may be NULL; the call zeroes it first) = the popcount.
 * Wave64, one bin per lane per round: streaming loads of the count and of the compared field alone, one ballot and one 8-byte
 * store per wave and round, a persistent grid, one atomic add per workgroup for `members`; no workgroup waits for another.
 * Asynchronous on `stream`.  PQPS_EINVAL before any launch: a NULL ctx / bins / bitmap, a bitmap that is not 8-byte aligned,
 * n_bins 0, a field or op outside the enums, `valued` 0 with a field other than PQPS_HAVING_COUNT.
 * pqps_bins_rows: *rows (device; zeroed by the call) = the sum of the counts of the same bins -- the rows a fused grouped scan
 * matched, which that scan does not report.  Asynchronous; PQPS_EINVAL for a NULL argument or n_bins 0. */
enum { PQPS_HAVING_COUNT = 0, PQPS_HAVING_SUM = 1, PQPS_HAVING_MIN = 2, PQPS_HAVING_MAX = 3 };
enum { PQPS_HAVING_EQ = 0, PQPS_HAVING_NE = 1, PQPS_HAVING_LT = 2, PQPS_HAVING_GT = 3, PQPS_HAVING_LE = 4, PQPS_HAVING_GE = 5 };
int pqps_bins_having(pqps_ctx *ctx, const void *bins, uint32_t n_bins, int valued, int field, int op, uint64_t constant,
                     int value_signed, uint32_t *bitmap, uint64_t *members, void *stream);
int pqps_bins_rows(pqps_ctx *ctx, const void *bins, uint32_t n_bins, int valued, uint64_t *rows, void *stream);

/* ---- UPDATE SET ... WHERE: constants assigned in place to the rows a WHERE selects -----------------------------------------
 * No counterpart in the reference (its parser knows no UPDATE).  A TARGET is a column and the value every selected row of it
 * receives: `data` 16-byte aligned and WRITABLE up to n_rows rounded up to PQPS_STEP_ROWS rows, `width` 1, 2, 4 or 8 bytes
 * (never a bit plane: a boolean column is assigned in its byte column and the plane repacked with pqps_pack_bits), `value`
 * the new value's low `width` bytes.  1 .. PQPS_MAX_COLUMNS targets per call, no column twice.  Rows that are not selected,
 * and every row at or past n_rows (the padding included), keep their bits.  Row r is read and written by one lane only, and
 * the WHERE of a row is evaluated before the row is written: a target may be one of the predicate's columns, the WHERE
 * sees its old values.  Asynchronous on `stream`; n_rows == 0 launches nothing.
 *
 * pqps_filter_assign: ONE scan of `pred` over rows [0, n_rows) of `cols` (as pqps_filter_count takes them, bit planes
 *   included) that stores into the targets as it goes; a 1024-row step without a match stores nothing and loads nothing
 *   beyond the predicate's columns.  *matched_dev (device, may be NULL) = the rows selected.  The context's timing recorder
 *   records the launch like a COUNT's.
 * pqps_assign_flags: the same stores for the rows r < n_rows with flags[r] != 0 -- the byte flags pqps_filter_flags or
 *   pqps_member_flags (PQPS_MEMBER_BYTES) wrote.  `flags` 16-byte aligned, read for r < n_rows only. */
typedef struct { void *data; uint32_t width; uint64_t value; } pqps_assign_target;
int pqps_filter_assign(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows, const pqps_predicate *pred,
                       const pqps_assign_target *targets, uint32_t n_targets, uint64_t *matched_dev, void *stream);
int pqps_assign_flags(pqps_ctx *ctx, const uint8_t *flags, uint64_t n_rows, const pqps_assign_target *targets, uint32_t n_targets,
                      void *stream);

/* ---- several COUNT(*) WHEREs answered by one scan -------------------------------------------------------------------------
 * No counterpart in the reference (SQL: SELECT COUNT(*) FILTER (WHERE a), COUNT(*) FILTER (WHERE b), ...).  ONE scan of rows
 * [0, n_rows) of `cols` -- the union of the queries' columns, each loaded once per 1024-row step -- answers up to
 * PQPS_COUNT_MANY_MAX queries: counts_dev[i] (device, n_queries u64, written whole by the call: no zeroing by the caller)
 * = the exact number of rows query i accepts.
 *   leaf[0 .. n_leaves)    the DISTINCT window tests of all queries, sorted by `column`, `negate` 0 (pqps_leaf arithmetic);
 *                          each is evaluated once per row whatever the number of queries that use it
 *   query[i]               a jump program as pqps_predicate carries it, in evaluation order: step s tests leaf slot leaf[s]
 *                          and goes to on_true[s] / on_false[s] -- a LATER step, PQPS_ACCEPT or PQPS_REJECT.  A negated
 *                          comparison is a step with the two targets swapped.  n_steps == 0: the constant `constant` (0 / 1).
 * Columns: 1, 2, 4 or 8 bytes or a bit plane, 16-byte aligned, readable up to n_rows rounded up to PQPS_STEP_ROWS as
 * pqps_filter_scan reads them; a PQPS_WIDTH_P12 column is PQPS_EINVAL (that form stays the one-query scan's).
 * PQPS_EINVAL, nothing launched: a NULL argument; n_queries 0 or above PQPS_COUNT_MANY_MAX; n_leaves above PQPS_MAX_LEAVES;
 * n_columns != n_cols or above PQPS_MAX_COLUMNS; a leaf whose column is out of range, leaves not sorted by column, a leaf
 * with `negate` set; n_steps above PQPS_TT_LEAVES; a step's leaf slot out of range; a jump target that is neither a later
 * step of the query nor accept / reject; `constant` above 1.
 * One scan launch (count_many_scan_kernel, the persistent grid of the fused scans) and, behind it, the one-workgroup
 * reduction of the workgroups' totals, as a COUNT has; n_rows == 0 launches the reduction only.  Asynchronous on `stream`.
 * The context's timing recorder records the call like a COUNT's: ONE record per call. */
#define PQPS_COUNT_MANY_MAX 16u
typedef struct pqps_count_query {
    uint32_t n_steps;
    uint8_t leaf[PQPS_TT_LEAVES], on_true[PQPS_TT_LEAVES], on_false[PQPS_TT_LEAVES];
    uint8_t constant;
} pqps_count_query;
typedef struct pqps_count_many {
    uint32_t n_queries, n_leaves, n_columns;
    pqps_leaf leaf[PQPS_MAX_LEAVES];
    pqps_count_query query[PQPS_COUNT_MANY_MAX];
} pqps_count_many;
int pqps_filter_count_many(pqps_ctx *ctx, const pqps_column *cols, uint32_t n_cols, uint64_t n_rows,
                           const pqps_count_many *prog, uint64_t *counts_dev /* n_queries u64 */, void *stream);

/* ---- batch INSERT: dictionary codes through a lookup table ----------------------------------------------------------------
 * No counterpart in the reference.  dst[i] = lut[src[i]] for i < n: what is left for the device when a batch of rows merges
 * its dictionary into a column's -- ONE pass per column and shard whatever the number of new strings (pqps_bump_codes is one
 * pass per string).  `src_width`, `dst_width` 1, 2 or 4 bytes, dst_width >= src_width: the same call widens a column whose
 * dictionary has outgrown its codes.  dst == src is legal exactly when the widths are equal (a lane reads and writes only
 * its own elements); otherwise the two ranges must not overlap.  `src` is read for i < n only.  No byte of `dst` at or past
 * n * dst_width changes; the dword the end cuts through is read and written back, so `dst` is readable and writable up to
 * n * dst_width rounded up to 4 bytes.  A code >= lut_count never indexes the table: it is stored as 0 and counted into
 * *bad_dev (device, may be NULL; zeroed by the call; one 64-bit atomic add per workgroup).  `lut_dev`: lut_count u32 words.
 * FORMS, chosen by the caller (pqps_remap_form: the form the engine takes for a table of lut_count entries):
 *   PQPS_REMAP_LDS     every workgroup stages the table into LDS once; lut_count <= PQPS_REMAP_LDS_CODES (16 KiB: the 8
 *                      workgroups per CU of the persistent grid fit a CU's 160 KiB -- with fewer the pass waits on its
 *                      loads)
 *   PQPS_REMAP_GLOBAL  lookups go to memory: a full 2-byte dictionary's table is 256 KiB and lives in L2
 * PQPS_EINVAL, nothing launched: a NULL pointer; `src` or `dst` not 16-byte aligned; a width pair outside the six; dst == src
 * with different widths or a partial overlap; an unknown form, or the LDS form with a larger table; lut_count 0, or a
 * lut_count whose largest position (lut_count - 1) does not fit dst_width.  n == 0 launches nothing.  Asynchronous on
 * `stream`.  Traffic: src_width + dst_width bytes per row. */
#define PQPS_REMAP_LDS    0
#define PQPS_REMAP_GLOBAL 1
#define PQPS_REMAP_LDS_CODES 4096u
int pqps_remap_codes(pqps_ctx *ctx, const void *src, uint32_t src_width, void *dst, uint32_t dst_width, uint64_t n,
                     const uint32_t *lut_dev, uint32_t lut_count, int form, uint64_t *bad_dev, void *stream);
int pqps_remap_form(uint32_t lut_count);

/* Checksums of a device-resident ID list: out[0] = sum of ids[i], out[1] = sum of ids[i] * (2 i + 1), both mod 2^64 (the
 * second depends on the order).  Synchronous; what a bench or a test compares two lists with without downloading them. */
int pqps_ids_checksum(pqps_ctx *ctx, const uint32_t *ids, uint64_t count, uint64_t out[2], void *stream);

/* Row-range block partition of engine/mpi/executeEngine-mpi.c:703-715. */
void pqps_partition(uint64_t n_rows, int world, int rank, uint64_t *start, uint64_t *count);

/* Seeded on-device generator of the commands_* schema (SURVEY.md App. B /
 * generate_commands.py distributions); rows [row0, row0+n) of the global
 * table.  Any output pointer may be NULL.  `user_cdf` = 2000 u32 thresholds,
 * `user_shell` = 2000 u8 (both device), built by pqps_synth_user_tables. */
typedef struct pqps_synth_cols {
    uint64_t *command_id;
    int32_t  *exit_code;
    int32_t  *user_id;
    int32_t  *risk_level;
    uint8_t  *sudo_used;
    uint8_t  *shell_code;     /* rank in {"bash","fish","sh","zsh"}        */
    uint16_t *user_code;      /* rank of "student<id>" == user_id - 1000   */
    uint8_t  *host_code;      /* rank among the 16 host names              */
    uint8_t  *base_code;      /* rank among 111 base commands (uniform)    */
} pqps_synth_cols;

#define PQPS_SYNTH_USERS 2000
void pqps_synth_user_tables(uint64_t seed, uint32_t *cdf_host, uint8_t *shell_host);
int  pqps_synth_generate(pqps_ctx *ctx, uint64_t seed, uint64_t row0, uint64_t n,
                         const uint32_t *user_cdf_dev, const uint8_t *user_shell_dev,
                         const pqps_synth_cols *out, void *stream);
/* CPU twin of the generator (same bits), used by tests and the CPU baseline. */
void pqps_synth_generate_host(uint64_t seed, uint64_t row0, uint64_t n,
                              const uint32_t *user_cdf, const uint8_t *user_shell,
                              const pqps_synth_cols *out);

#ifdef __cplusplus
}
#endif
#endif /* PQPS_HIP_H */
