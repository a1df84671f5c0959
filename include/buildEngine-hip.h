/* buildEngine-hip.h -- load step of the HIP engine: CSV -> rows -> per-column
 * device buffers (+ order-preserving dictionaries for the 7 string columns).
 *
 * Same role and naming as the reference's include/buildEngine-omp.h:30-35;
 * CSV rules follow engine/serial/buildEngine-serial.c:70-221 exactly
 * (SURVEY.md App. A.5): header line skipped, 1024-byte fgets window, quoted
 * fields with "" escape, missing trailing fields stay zero.
 */
#ifndef BUILDENGINE_HIP_H
#define BUILDENGINE_HIP_H

#include "bplus.h"
#include "executeEngine-hip.h"
#include "logType.h"
#include "recordSchema.h"
#include "pqps_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Column order of `record` / the CSV. */
enum {
    HIPCOL_COMMAND_ID = 0, HIPCOL_RAW_COMMAND, HIPCOL_BASE_COMMAND, HIPCOL_SHELL_TYPE,
    HIPCOL_EXIT_CODE, HIPCOL_TIMESTAMP, HIPCOL_SUDO_USED, HIPCOL_WORKING_DIRECTORY,
    HIPCOL_USER_ID, HIPCOL_USER_NAME, HIPCOL_HOST_NAME, HIPCOL_RISK_LEVEL,
    HIPCOL_COUNT
};

/* Sorted (strcmp byte order) distinct values of one string column. */
struct hipDictionary {
    int count;
    const char **values;     /* `count` strings, ascending; into `storage` or (after INSERT) strdup'd */
    char *storage;
    size_t storage_bytes;
};

/* One B+-tree replacement: device permutation + sorted keys. */
struct hipIndex {
    int column;              /* HIPCOL_*                                   */
    int key_kind;            /* 0 unsigned, 1 signed                       */
    uint32_t *perm_dev;      /* n rows, (key asc, row desc)                */
    void *keys_dev;          /* n keys, column width                       */
};

/* Locks of one engine (engine/hip/buildEngine-hip.c).  The OpenMP driver of the reference calls the engine
 * from several threads at once (QPEOMP.c:234-291).  SELECT / COUNT are READERS: each takes one of the table's
 * query LANES (result buffers of its own on every shard + a slot of the shards' query streams, pqps_qstream),
 * so several of them are on the device at once and none waits for another's result download; INSERT / DELETE /
 * index creation are WRITERS and run alone.  A reader may be finished by another thread than the one that began
 * it (asynchronous tickets), hence a counting gate and not a pthread rwlock. */
struct hipLocks;

/* Result buffers of one query in flight on one shard. */
struct hipLane {
    uint32_t *ids_dev;                           /* row numbers of the result, capacity_ids u32                 */
    uint64_t capacity_ids;
    uint64_t *count_dev;                         /* 8 x u64: count, spare, range[2], flag-pass count, spare ... */
    volatile uint64_t *count_host;               /* the same words as the host sees them (pinned, mapped): read after the
                                                    query's completion event, no download; NULL: count_dev is device memory */
    pqps_ctx *copy;                              /* context (stream) for this lane's downloads / gathers; NULL: the table's */
    uint32_t *merged_dev;                        /* shard 0 only, several shards: the gathered list of all shards */
    uint64_t merged_cap;
};

#define HIP_MAX_LANES 8

/* Device-resident table; hangs off engineS.record_block (same address for the engine's life). */
struct hipTable {
    pqps_ctx *ctx;
    uint64_t n_rows;
    uint64_t capacity_rows;                      /* allocation, multiple of PQPS_TILE_ROWS */
    pqps_column col[HIPCOL_COUNT];               /* device buffers; a dictionary column with ONE value may have none
                                                    (data NULL, width 0): every row carries code 0                  */
    struct hipDictionary dict[HIPCOL_COUNT];     /* string columns only                    */
    struct hipIndex *index;                      /* engine->num_indexes entries            */
    struct hipLane own;                          /* the table's own result buffers: writers, ad-hoc tables          */
    pqps_qstream *qs;                            /* engine tables: this shard's query stream, n_lanes slots         */
    int n_lanes;
    struct hipLane lane[HIP_MAX_LANES];
    record *row_block;                           /* contiguous host rows (all_records[i] point in); NULL: device only */
    size_t row_capacity;                         /* rows row_block / all_records have room for      */
    int device_only;                             /* the engine has no host rows (initializeEngineColumnsHIP / SyntheticHIP) */
    int probe_bool;                              /* index mode probes BOOL indexes too (hipEngineProbeBoolIndexes) */
    struct hipLocks *locks;                      /* engine tables only; NULL for ad-hoc tables      */
    /* Several devices in one process (PQPS_DEVICES=0,1,...): the engine's rows are split into contiguous
     * shards by the reference's block partition (executeEngine-mpi.c:703-715), one device table each.
     * shard[0] is this table; it alone owns the dictionaries (codes are global), the host rows and the
     * locks.  A table without shards (n_shards 0) is its own single shard. */
    int n_shards;
    struct hipTable **shard;
    uint64_t row0;                               /* engine row number of this shard's first row    */
    /* One process per GPU (hipEngineJoinRanksHIP): this process holds rows [row0, row0 + n_rows) of a table that `world`
     * processes hold between them; scan-mode SELECT / COUNT go through the exchange (pqps_exchange_*: the shard's scan +
     * all-gatherv of the row numbers / all-reduce of the counts over RCCL, engine/mpi/executeEngine-mpi.c:745-765), whose
     * ring slots are the table's lanes. */
    pqps_exchange *xch;
    int world, rank;
    uint64_t rows_total;
    /* Bit plane of HIPCOL_SUDO_USED (width PQPS_WIDTH_BITS, capacity_rows / 8 bytes; data NULL without a byte column): what
     * the scans read in place of the byte column.  Packed from the byte column wherever that is written (load, INSERT,
     * DELETE) by the writer that wrote it; index builds, gathers, projection and compaction keep using the byte column. */
    pqps_column sudo_bits;
    /* 12-bit packed copies (width PQPS_WIDTH_P12, capacity_rows * 3 / 2 bytes; data NULL: none) of the dictionary columns
     * stored as u16 whose dictionary has at most 4096 entries: what a scan of that column alone, or of it and the plane of
     * sudo_used, reads in place of the u16 column (1.5 bytes per row).  Every writer that changes a row or the codes of
     * such a column repacks its copy WHOLE before it returns; a dictionary that outgrows 4096 entries, or a column whose
     * width changes, drops the copy for good.  Everything but those scans keeps using the u16 column. */
    pqps_column packed12[HIPCOL_COUNT];
    /* Value range of the i32 columns a grouped COUNT has grouped on (executeQueryGroupCountHIP), over every shard's rows;
     * shard 0 only, computed on first use.  INSERT widens a known range; DELETE leaves it (then possibly wider than the data). */
    int bounds_known[HIPCOL_COUNT];
    int32_t bounds_lo[HIPCOL_COUNT], bounds_hi[HIPCOL_COUNT];
    /* The value sets of the engine (hipEngineCreateSetHIP; engine/hip/executeEngine-hip.c owns the type): shard 0 only, made
     * with the first set, kept across a rebuild like the locks, freed by destroyEngineHIP. */
    struct hipValueSets *sets;
};

#define HIP_MAX_SHARDS 16
static inline int hipTableShards(const struct hipTable *t) { return t->n_shards > 1 ? t->n_shards : 1; }
static inline struct hipTable *hipTableShard(struct hipTable *t, int s) { return t->n_shards > 1 ? t->shard[s] : t; }

/* No-ops on a table without locks.  hipTableLockExclusive returns -1 (and takes nothing) when the calling thread holds a
 * query lane -- a ticket of its own it has not released: the writer would wait for that ticket for ever. */
void hipTableLockShared(struct hipTable *t);
void hipTableUnlockShared(struct hipTable *t);
int  hipTableLockExclusive(struct hipTable *t);
void hipTableUnlockExclusive(struct hipTable *t);
/* A free query lane of the table; -1 on a table without lanes (the query then uses the table's own buffers).  Waits while
 * all lanes are taken, but never for ever: HIP_LANE_REFUSED at once when the calling thread itself holds every lane, or
 * after PQPS_LANE_WAIT_MS (default 10 000) without a lane coming free; the reason is on stderr. */
#define HIP_LANE_REFUSED (-2)
int  hipTableAcquireLane(struct hipTable *t);
void hipTableReleaseLane(struct hipTable *t, int lane);
int  hipTableLaneCount(const struct hipTable *t);
/* test hooks: the gate alone on a table that has nothing else (tests/c/locks_test.c) */
void hipTableLocksCreate(struct hipTable *t, int n_lanes);
void hipTableLocksDestroy(struct hipTable *t);
/* Issuing calls on the shards' query streams are serialised (they take microseconds). */
void hipTableLockIssue(struct hipTable *t);
void hipTableUnlockIssue(struct hipTable *t);

/* CSV -> contiguous block of records + pointer array (reference signature of
 * getAllRecordsFromFileOMP, buildEngine-omp.h:31). */
record **getAllRecordsFromFileHIP(const char *filepath, int *num_records, void **record_block_out);
/* Parses one CSV line into a freshly calloc'd record (buildEngine-serial.c:159). */
record *getRecordFromLineHIP(char *line);
/* Same, into caller storage (zeroed first). */
void fillRecordFromLineHIP(record *dst, const char *line);
FieldType mapAttributeTypeHIP(int attributeType);
/* Builds the device index for one attribute and appends it to the engine. */
bool makeIndexHIP(struct engineS *engine, const char *indexName, int attributeType);

/* rows -> columns -> device.  Replaces engine->record_block (the row block
 * returned by getAllRecordsFromFileHIP) by the struct hipTable that owns it. */
bool buildDeviceTableHIP(struct engineS *engine);
/* Same, with the device context coming from a start-up begun earlier (hipBeginContextHIP runs
 * pqps_ctx_create on a background thread: the HIP runtime needs ~0.2 s, the CSV parse can use them). */
struct hipContextFuture;
struct hipContextFuture *hipBeginContextHIP(void);
bool buildDeviceTableOnHIP(struct engineS *engine, struct hipContextFuture *future);
/* Re-creates columns, dictionaries and indexes from engine->all_records
 * (after INSERT / DELETE changed the host rows). */
void rebuildDeviceTableHIP(struct engineS *engine);
/* INSERT: appends `r` (row number engine->num_records - 1) to the device table (its last shard) in place; false
 * when that needs a rebuild which a device-only engine cannot do (a dictionary outgrowing its code width). */
bool appendRowDeviceTableHIP(struct engineS *engine, const record *r);
/* DELETE: `delete_flags_dev[s]` (1 = row goes, from pqps_filter_flags on shard s) compacts that shard's
 * device columns in place; `expected_rows` = survivors counted on the host over all shards (cross-check). */
void compactDeviceTableHIP(struct engineS *engine, uint8_t *const *delete_flags_dev, size_t expected_rows);
/* UPDATE (executeQueryUpdateHIP), device side, in the order the engine calls them under the exclusive lock; `a` = the n
 * assignments hipCompileAssignments made against the table's schema.
 *   updateNeedsRebuildHIP       true when an assignment cannot be made in place: a string new to a dictionary that is full
 *                               for its code width, or another value for a single-valued column without a buffer.
 *   updateInsertStringsHIP      every string that is new goes into its dictionary at its rank, the codes at and above it are
 *                               bumped on every shard (pqps_bump_codes, as INSERT); bit c of the result: column c was bumped.
 *   updateTargetsHIP            the shard's targets of pqps_filter_assign / pqps_assign_flags (a single-valued column assigned
 *                               its own value has none); returns their number.
 *   finishUpdateDeviceTableHIP  matched[s] = rows shard s changed: repacks the sudo_used plane, widens the cached bounds of
 *                               an i32 target, rebuilds the indexes on assigned columns (shards with a match) and on bumped
 *                               columns (every shard). */
struct hipAssignment;
bool updateNeedsRebuildHIP(struct engineS *engine, const struct hipAssignment *a, int n);
uint32_t updateInsertStringsHIP(struct engineS *engine, const struct hipAssignment *a, int n);
int updateTargetsHIP(const struct hipTable *sh, const struct hipAssignment *a, int n, pqps_assign_target *targets);
void finishUpdateDeviceTableHIP(struct engineS *engine, const struct hipAssignment *a, int n, const uint64_t *matched, uint32_t bumped);
/* Batch INSERT (executeQueryInsertColumnsHIP / executeQueryInsertRowsHIP), device side, under the exclusive lock, in two steps
 * so that everything that can be refused is decided before a row, a file or a dictionary changes:
 *   prepareAppendColumnsHIP  checks the batch (shapes, widths, the dictionary merges of hipMergeDictionaries, INT_MAX rows), stages
 *                            it on the last shard's device -- host arrays uploaded, device arrays copied -- and translates its
 *                            codes into staging buffers of the column's final width (pqps_remap_codes with lut_new, whose count
 *                            of out-of-range codes is the code check); command_id != 0 and sudo_used <= 1 are checked on the
 *                            host.  NULL = refused (reason on stderr), nothing changed.  The caller's dictionaries must stay
 *                            valid until the commit.
 *   prepareAppendRowsHIP     the same from records: the batch's dictionaries and codes built on the host first.
 *   commitAppendHIP          grows the last shard when its head-room is used up (shard_alloc's capacity for the new count);
 *                            per string column whose merge is no identity or whose union needs wider codes ONE
 *                            pqps_remap_codes with lut_old per shard (in place, or into a buffer of the next width that fits;
 *                            a single-valued column gets its buffer); copies the staged columns behind the last row; packs
 *                            the plane from the first new row; widens cached bounds; installs the unions as dictionaries;
 *                            rebuilds the last shard's indexes and, on the other shards, those whose codes changed;
 *                            advances engine->num_records; frees the batch.  A device failure here is fatal, as in INSERT.
 *   discardAppendHIP         frees a prepared batch that is not committed. */
struct hipAppend;
struct hipColumnData;
struct hipAppend *prepareAppendColumnsHIP(struct engineS *engine, unsigned long long num_rows, const struct hipColumnData *columns);
struct hipAppend *prepareAppendRowsHIP(struct engineS *engine, const record *rows, unsigned long long num_rows);
void commitAppendHIP(struct engineS *engine, struct hipAppend *batch);
void discardAppendHIP(struct engineS *engine, struct hipAppend *batch);
void destroyDeviceTableHIP(struct engineS *engine);

/* Engines over device-resident columns (no host rows): see initializeEngineColumnsHIP / initializeEngineSyntheticHIP
 * in executeEngine-hip.h.  `columns` describes all 12 columns of `record`. */
struct hipColumnData;
bool buildDeviceTableFromColumnsHIP(struct engineS *engine, unsigned long long num_rows, const struct hipColumnData *columns);
bool buildSyntheticDeviceTableHIP(struct engineS *engine, unsigned long long num_rows, unsigned long long seed);
/* rows [first_row, first_row + num_rows) of the seeded table, as ONE shard whose row numbers start at first_row (a rank's
 * part of a table spread over several processes); `min_lanes`: at least that many query lanes */
bool buildSyntheticShardDeviceTableHIP(struct engineS *engine, unsigned long long num_rows, unsigned long long seed,
                                       unsigned long long first_row, int min_lanes);
/* Dictionary of a string column of the synthetic table (ascending strcmp order): the values behind the codes
 * pqps_synth_generate produces; NULL for a numeric column. */
const char *const *hipSyntheticDictionary(int column, int *count);

/* Lower-level pieces (also used for ad-hoc tables over caller-supplied rows,
 * see linearSearchRecords / evaluateWhereClause in executeEngine-hip.c). */
struct hipSchema;
struct hipTable *hipTableFromRows(pqps_ctx *ctx, record *const *rows, size_t n);
void hipTableFree(struct hipTable *t, int n_indexes);
void hipSchemaOfTable(const struct hipTable *t, struct hipSchema *s);

#ifdef __cplusplus
}
#endif
#endif /* BUILDENGINE_HIP_H */
