/* executeEngine-hip.h -- MI355X (gfx950) execute engine.
 *
 * Drop-in for the reference's OpenMP / MPI engines: same shape as
 * include/executeEngine-omp.h:8-51 with the suffix HIP, same structs
 * (executeEngine-serial.h), same ownership and error behaviour as the serial
 * engine that defines the results (engine/serial/executeEngine-serial.c):
 *
 *   executeQuerySelectHIP   replaces executeQuerySelectSerial :328-528
 *                           (and executeQuerySelectOMP omp:333, ...MPI mpi:332)
 *   initializeEngineHIP     replaces initializeEngineSerial :727-771
 *   destroyEngineHIP        replaces destroyEngineSerial :774-814
 *   addAttributeIndexHIP    replaces addAttributeIndexSerial :825-841
 *   executeQueryDeleteHIP   replaces executeQueryDeleteSerial :627-715
 *   executeQueryInsertHIP   replaces executeQueryInsertSerial :538-617
 *
 * Results are bit-exact with QPESeq (the serial engine): scan mode returns
 * ascending row order; index mode returns (key asc, row desc) per probed
 * top-level condition, concatenated, then re-filtered.
 * There is no CPU fallback: without a gfx950 device / the HIP runtime
 * initializeEngineHIP prints the reason and exits, like the reference's engines on a failed start-up
 * allocation.  A query that fails later (a WHERE that cannot be compiled, a device error) prints the reason
 * and reports failure -- success = false / -1 -- and the engine stays usable.  (A device step that fails in
 * the middle of an INSERT / DELETE -- after the CSV and the host rows have changed -- is still fatal: the device
 * table could not be trusted afterwards.)
 */
#ifndef EXECUTE_ENGINE_HIP_H
#define EXECUTE_ENGINE_HIP_H

#include "executeEngine-serial.h"

#ifdef __cplusplus
extern "C" {
#endif

struct resultSetS *executeQuerySelectHIP(
    struct engineS *engine,
    const char **selectItems,        /* NULL / 0 items: all 12 columns            */
    int numSelectItems,
    const char *tableName,           /* ignored, as in the reference              */
    struct whereClauseS *whereClause /* NULL: every row                           */
);

bool executeQueryInsertHIP(struct engineS *engine, const char *tableName, const record *r);

struct resultSetS *executeQueryDeleteHIP(
    struct engineS *engine, const char *tableName, struct whereClauseS *whereClause);

struct engineS *initializeEngineHIP(
    int num_indexes,
    const char *indexed_attributes[],
    const int attribute_types[],     /* 0 = u64, 1 = int, 2 = string, 3 = bool    */
    const char *datafile,
    const char *tableName
);

void destroyEngineHIP(struct engineS *engine);

bool addAttributeIndexHIP(struct engineS *engine, const char *tableName,
                          const char *attributeName, int attributeType);

/* ---- HIP-engine extensions (not in the reference API) ------------------- */

/* The filter without the string projection: matching row numbers (the index
 * into engine->all_records) in QPESeq result order.  Returns the number of
 * matches, or -1 on error; *ids is malloc'd (caller frees).  This is what
 * executeQuerySelectHIP projects from, and what COUNT(*) reads. */
long long executeQuerySelectIdsHIP(struct engineS *engine,
                                   struct whereClauseS *whereClause,
                                   unsigned int **ids, double *queryTime);

/* Columnar SELECT: the scalable form of resultSetS (executeEngine-serial.h:30-38, whose rows x columns
 * heap strings are the right shape for 50 k rows, not for 10^8).  Same row selection and order as
 * executeQuerySelectHIP; the selected columns are gathered ON THE DEVICE for the result rows
 * (pqps_project_column) and come back as typed arrays; text exists only for the cells someone asks for
 * (hipColumnarCellText, hipColumnarHead -> printTable), formatted exactly as get_attribute_string_value
 * (serial:216-248) would. */
struct hipColumnarResult {
    int numRecords;
    int numColumns;
    char **columnNames;
    int *columnKinds;                  /* HIPKIND_U64 / _I32 / _BOOL / _DICT (hipPredicate.h); -1 = unknown column ("NULL" cells) */
    void **values;                     /* per column, numRecords entries: uint64_t / int32_t / uint8_t / uint32_t dictionary code */
    const char *const **dictionaries;  /* per column: code -> C string for _DICT columns, else NULL.  Owned by the result: the
                                          codes are numbered 0 .. dictionarySizes[col]-1 over the distinct values this result
                                          holds, ascending in strcmp order */
    int *dictionarySizes;
    double queryTime;                  /* selection + device gather + download */
    bool success;
};
struct hipColumnarResult *executeQuerySelectColumnarHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                        struct whereClauseS *whereClause);
void freeColumnarResultHIP(struct hipColumnarResult *result);
/* malloc'd text of one cell. */
char *hipColumnarCellText(const struct hipColumnarResult *result, int row, int column);
/* The first `limit` rows (all if limit <= 0, printTable's own convention) as an ordinary result set, e.g. for printTable; numRecords of the
 * returned set is the FULL count, as printTable's footer reports it, and only `limit` rows of data exist --
 * free it with freeResultSetHead. */
struct resultSetS *hipColumnarHead(const struct hipColumnarResult *result, int limit);
void freeResultSetHead(struct resultSetS *head, int rows);

/* ---- engines over device-resident columns: tables of 10^8 - 10^9 rows behind struct engineS --------------------
 * initializeEngineHIP builds the device table from 1040-byte host rows (the reference's `record`); a 1 G-row table
 * is 1.04 TB in that form and 26 GB as columns.  These two constructors build the SAME engine -- same query API,
 * same results -- without host rows: engine->all_records is NULL, engine->datafile is "" (INSERT / DELETE change
 * the device table only, no CSV is kept in step), and executeQuerySelectHIP produces its strings from values
 * gathered on the device.
 *
 * initializeEngineColumnsHIP: the caller hands over the 12 columns of `record` (include/logType.h:11-24) as arrays:
 *   numeric columns   command_id u64, exit_code / user_id / risk_level i32, sudo_used u8 (0 / 1)
 *   string columns    order-preserving dictionary codes (u8 / u16 / u32 by `width`) + the dictionary, ascending in
 *                     strcmp order, no duplicates; a column whose dictionary has ONE value needs no array
 *   values            host memory, or (on_device != 0) device memory of the engine's device -- copied either way,
 *                     the engine owns padded buffers with head-room for INSERT.
 * initializeEngineSyntheticHIP: the seeded synthetic table of the commands_* schema (pqps_synth_generate,
 * SURVEY.md App. B distributions), generated in place on the device(s); raw_command, timestamp and
 * working_directory are single-valued columns.  With PQPS_DEVICES=0,1,... the rows are sharded like any engine's. */
struct hipColumnData {
    const void *values;                /* num_rows entries of `width` bytes; NULL for a single-valued string column */
    unsigned int width;                /* bytes per entry: 8 / 4 / 1 as the column's type says; codes: 1, 2 or 4      */
    int on_device;                     /* values is device memory (of the engine's first device)                      */
    const char *const *dictionary;     /* string columns: `dictionary_count` C strings, ascending strcmp order         */
    int dictionary_count;
};
struct engineS *initializeEngineColumnsHIP(unsigned long long num_rows, const struct hipColumnData columns[12],
                                           int num_indexes, const char *indexed_attributes[], const int attribute_types[],
                                           const char *tableName);
struct engineS *initializeEngineSyntheticHIP(unsigned long long num_rows, unsigned long long seed,
                                             int num_indexes, const char *indexed_attributes[], const int attribute_types[],
                                             const char *tableName);

/* ---- set predicates in WHERE: LIKE and IN --------------------------------------------------------------------------
 * Beyond the reference's six comparisons a `struct whereClauseS` node may carry one of four operators, written exactly
 * so: "LIKE", "NOT LIKE", "IN", "NOT IN".  They are reached through this API only (the reference's tokenizer and
 * connectEngine never produce them); any other unknown operator stays "never true".
 *   LIKE / NOT LIKE   string columns.  `value` is the pattern: `%` any run of bytes (none included), `_` exactly one byte,
 *                     `\%` `\_` `\\` literals, a backslash anywhere else itself; byte-wise, case-sensitive, the whole
 *                     string has to match.  On a numeric or boolean column the WHERE is refused.
 *   IN / NOT IN       any column.  `value` is `( item, item, ... )`: a single-quoted string ('' = a quote inside it) or a
 *                     bare token trimmed of white space, each typed by the column exactly as the literal of `=` is.
 *                     `()` is legal (IN: never true).  Duplicates and strings no row carries are harmless.  Refused: no
 *                     parentheses, an unterminated quote, an empty item, more than 65 536 items.
 * A refused WHERE fails like any WHERE that cannot be compiled (message on stderr, the query reports failure).  Set
 * conditions are never index probes: in index mode they are part of the re-filter of the probed rows.  A set of up to four
 * runs of values costs nothing extra (it is window comparisons of the one fused scan, and crosses ranks like any other);
 * a more fragmented one is a pass of its own in front of the scan (include/hipPredicate.h), which every query form and
 * DELETE take in their stride -- the aggregates by their selection-then-list route -- and which an engine joined across
 * ranks refuses, as it refuses every WHERE of several passes. */

/* ---- batch INSERT: any number of rows appended in one call ----------------------------------------------------------------
 * executeQueryInsertHIP takes one `record` per call and pays, per call, twelve small uploads, a rebuild of the last shard's
 * indexes and -- for every string new to its dictionary -- a pass over that column on every shard (pqps_bump_codes) and a
 * rebuild of every shard's indexes; on an engine without host rows it gives up when the head-room is used up or a dictionary
 * outgrows its code width.  These two calls append a whole batch: ONE dictionary merge per string column on the host
 * (hipMergeDictionaries), at most ONE remap pass per string column and shard on the device (pqps_remap_codes) whatever the
 * number of new strings, ONE rebuild of the indexes; a column whose union outgrows its codes is widened 1 -> 2 -> 4 bytes, a
 * single-valued column that receives a second string gets its buffer, and the last shard grows when its head-room is used up.
 * executeQueryInsertHIP itself is unchanged.
 * RESULT.  The engine answers every query form exactly as a fresh engine built from the old rows followed by the batch's rows
 * in order: dictionaries are the sorted unions (a batch string no row carries still enters: harmless, as after DELETE), old
 * rows keep their numbers, the new ones are n .. n + num_rows - 1 on the last shard (no re-balancing, as INSERT).
 * Both return the rows appended, or -1 (reason on stderr) with NOTHING changed; num_rows == 0 returns 0.  Writers like INSERT,
 * DELETE and UPDATE: the exclusive lock, refused from a thread that holds a ticket and on an engine joined across ranks.
 *   executeQueryInsertColumnsHIP  the input of initializeEngineColumnsHIP: the batch's own ascending dictionaries, codes of 1, 2
 *       or 4 bytes whatever the table's width, `values` NULL with a one-string dictionary for a single-valued column,
 *       `on_device` honoured.  For engines WITHOUT host rows; an engine over a CSV refuses it (it has rows and a file to keep
 *       in step).
 *   executeQueryInsertRowsHIP     records; the batch's dictionaries and codes are built from them, then the same device route.  On
 *       an engine with host rows the row store grows once, the batch goes to the CSV in one fopen("a") (the bytes B single
 *       INSERTs leave) and the rows are copied, all after the batch has been accepted.
 * REFUSED before anything changes: a dictionary list that is not strictly ascending, an empty or over-long string (the merge's
 * refusals); a width outside 8 / 4 / 1 for the numeric columns or 1 / 2 / 4 for codes; values NULL with a dictionary of more
 * than one string; command_id 0 or sudo_used > 1 in any batch row; a batch code >= its dictionary_count; more than INT_MAX
 * rows in all.  `queryTime` may be NULL. */
long long executeQueryInsertColumnsHIP(struct engineS *engine, const char *tableName, unsigned long long num_rows,
                                       const struct hipColumnData columns[12], double *queryTime);
long long executeQueryInsertRowsHIP(struct engineS *engine, const char *tableName, const record *rows, unsigned long long num_rows,
                                    double *queryTime);

/* ---- UPDATE table SET column = value [, ...] [WHERE ...] ---------------------------------------------------------------
 * No counterpart in the reference (its parser answers UPDATE with CMD_UNKNOWN); reached through this API only.
 * `setColumns[i] = setValues[i]` for i < numSet (1 .. 12, no column twice); each value text is typed by its column exactly
 * as the literal of `=` is typed in a WHERE (strtoull for command_id, atoi for the i32 columns, "true" in any case or "1"
 * for sudo_used and anything else false, the string itself for a string column).  Returns the number of rows the WHERE
 * selects -- a row that already carries the new value counts -- or -1 on refusal or error (reason on stderr).
 *   ROWS        the rows for which the WHERE is true, each once: scan semantics, also on an engine with indexes, as DELETE
 *               has.  NULL: every row.  LIKE / IN work as in any WHERE.
 *   OLD VALUES  the WHERE reads the values from before the update, also of columns that are assigned.
 *   STABILITY   row numbers, row order and every other column stay as they are.
 *   WRITER      UPDATE runs alone like INSERT / DELETE: it waits until every ticket is released and is refused (-1) when
 *               called from a thread that holds one.
 *   REFUSED     (-1, table unchanged) what hipCompileAssignments refuses (include/hipPredicate.h: unknown column, a column
 *               twice, numSet outside 1 .. 12, an empty or over-long string, command_id 0); a WHERE that cannot be compiled;
 *               an engine joined across ranks; and, on an engine without host rows, an assignment that only a rebuild of the
 *               table could make: a string new to a dictionary that is full for its code width (256 / 65 536 values), or
 *               another value for a single-valued string column that has no device buffer (assigning that column its own
 *               value is legal and changes nothing).  The engine decides this before it changes anything.
 * A string that is new to its column's dictionary is inserted at its rank first and the codes at and above it are bumped on
 * every shard (as INSERT does); when the WHERE then fails to compile or selects no row the dictionary keeps a value no
 * row carries -- harmless, as after DELETE.
 * Engines without host rows: a WHERE that is one scan pass is ONE fused launch per shard (pqps_filter_assign: the WHERE
 * and the stores); any other WHERE leaves byte flags as for DELETE and pqps_assign_flags stores by them.  Engines with host
 * rows and a CSV always take the flags: the flags come to the host, the matching host rows are changed and the CSV is
 * rewritten as after DELETE (not at all when no row matches); the device stores by the same flags, or the table is
 * rebuilt from the host rows where the assignment needs it.  Afterwards the sudo_used bit plane, the cached i32 bounds and
 * the indexes on assigned or bumped columns are brought up to date. */
long long executeQueryUpdateHIP(struct engineS *engine, const char *tableName,
                                const char *const *setColumns, const char *const *setValues, int numSet,
                                struct whereClauseS *whereClause, double *queryTime /* may be NULL */);

/* ---- asynchronous queries: several in flight, results left on the device -----------------------------------------
 * The engine's table has LANES (default 4, PQPS_ENGINE_LANES): result buffers + a slot of the table's query stream
 * (pqps_qstream: two launches in flight on two HIP streams, one for tables of 537 M rows and more).  Every SELECT /
 * COUNT takes a lane for its device phase -- concurrent callers of the synchronous functions (the reference's OpenMP
 * driver, QPEOMP.c:234-291) therefore overlap on the device -- and a caller can keep several queries in flight itself:
 *   t = executeQuerySelectAsyncHIP(engine, where)     enqueues the query (blocks only while every lane is taken)
 *   n = awaitQueryHIP(t, &result)                     waits for it: number of matching rows, -1 on error
 *   ...                                               result.ids_dev: the row numbers in QPESeq order, ON THE DEVICE
 *   releaseQueryHIP(t)                                the lane is free again, result.ids_dev is no longer valid
 * With several shards the shards' lists are gathered on shard 0's device by peer copies (the one-process form of
 * MPI_Allgather of the sizes + MPI_Allgatherv of the payload, engine/mpi/executeEngine-mpi.c:753-765; index mode:
 * merged by key on the device).  executeQueryCountAsyncHIP: COUNT(*), no list.  A ticket must be released. */
struct hipQueryTicket;
struct hipDeviceResult {
    long long count;                   /* matching rows (COUNT: the only field that means anything)     */
    const unsigned int *ids_dev;       /* `count` row numbers, device memory of device `device`         */
    int device;
    int n_shards;
    unsigned long long shard_count[16];/* matches found by each shard                                    */
};
/* Limits, so that no caller can wait for itself (the engine refuses instead of hanging a process that holds the GPU):
 *   - a thread may hold at most hipEngineLanes(engine) unreleased tickets of one engine; asking for one more returns NULL at
 *     once (reason on stderr).  Tickets held by SEVERAL threads can still add up to all lanes: a further request then waits
 *     for a release, at most PQPS_LANE_WAIT_MS (default 10 000), and returns NULL after that;
 *   - INSERT / DELETE / UPDATE / addAttributeIndexHIP / hipEngineProbeBoolIndexes / hipEngineKernelTiming wait until every ticket is
 *     released; called from a thread that holds a ticket itself they are refused (false / success = false / -1).  While such
 *     a call waits, threads that hold no ticket wait behind it with new queries; a thread that holds one may take more. */
int hipEngineLanes(struct engineS *engine);
struct hipQueryTicket *executeQuerySelectAsyncHIP(struct engineS *engine, struct whereClauseS *whereClause);
struct hipQueryTicket *executeQueryCountAsyncHIP(struct engineS *engine, struct whereClauseS *whereClause);
long long awaitQueryHIP(struct hipQueryTicket *ticket, struct hipDeviceResult *result /* may be NULL */);
void releaseQueryHIP(struct hipQueryTicket *ticket);
/* out[0] = sum of the answer's row numbers, out[1] = sum of id[i] * (2 i + 1), mod 2^64 -- computed where the list lies,
 * on the device; awaits the ticket first.  0, or -1 (a failed query, a COUNT ticket). */
int hipQueryChecksumHIP(struct hipQueryTicket *ticket, unsigned long long out[2]);

/* ---- one process per GPU: the reference's QPEMPI shape (QPEMPI.c:145-155: a C driver, one process per rank; the row
 * partition and the exchange of engine/mpi/executeEngine-mpi.c:703-768) ----------------------------------------------
 * Every process builds ITS rows of the table -- initializeEngineSyntheticRankHIP: rows [start, start + count) of the
 * seeded table by the reference's block partition, row numbers table-wide -- on its own GPU (PQPS_DEVICE), then joins the
 * others: rank 0 makes a 128-byte RCCL id (hipEngineRcclIdHIP) and hands it to the other ranks by whatever the host has (a
 * file, MPI_Bcast, torch.distributed), every rank calls hipEngineJoinRanksHIP -- or its two halves with an agreement of
 * the ranks in between, so that a rank that fails locally cannot leave the others inside the communicator's bring-up.
 * From then on the engine's SELECT / COUNT are the TABLE's: executeQuerySelectAsyncHIP enqueues the shard's scan and the
 * all-gatherv of the matching row numbers over RCCL (sizes, then exactly-sized payload at displacements, compact on the
 * wire: pqps_exchange_select), awaitQueryHIP hands EVERY rank the whole ascending list on its device (count = matches in
 * the table, shard_count[0] = this rank's); COUNT is the all-reduced count (mpi:745).  Rules: every rank issues the same
 * queries in the same order (one issuing thread per process, or an order the host guarantees); scan-mode queries of one
 * pass only (no index probes: the rank engines have no indexes); INSERT / DELETE are not exchanged.  `rccl_library`: the
 * librccl.so to load (e.g. /opt/rocm/lib/librccl.so).  Every host wait of the exchange is bounded
 * (PQPS_EXCHANGE_TIMEOUT_S): a query that cannot finish fails -- awaitQueryHIP returns -1 -- it never hangs. */
struct engineS *initializeEngineSyntheticRankHIP(unsigned long long rows_total, unsigned long long seed, int world, int rank,
                                                 const char *tableName);
int hipEngineRcclIdHIP(const char *rccl_library, void *id128);
int hipEngineJoinRanksHIP(struct engineS *engine, const char *rccl_library, const void *id128);
int hipEngineJoinPrepareHIP(struct engineS *engine, const char *rccl_library);
int hipEngineJoinConnectHIP(struct engineS *engine, const void *id128);
int hipEngineLeaveRanksHIP(struct engineS *engine);
/* payload bytes this rank has received: out[0] as they travelled, out[1] as u32 row numbers would have */
int hipEngineWireBytesHIP(struct engineS *engine, unsigned long long out[2], int reset);
/* out[0] = SELECTs whose answer arrived with the sizes (one collective, pqps_exchange_eager), out[1] = SELECTs finished,
 * out[2] = row numbers a rank's block has room for (0: off) */
int hipEngineEagerQueriesHIP(struct engineS *engine, unsigned long long out[3], int reset);

/* Device time of the engine's queries AS THEY RUN on the lanes (several in flight): the recorders of the shards' query
 * streams (pqps_qstream_set_timing), events on the dispatch packets.  hipEngineKernelTime sums over the launches
 * recorded since the last call: scan_ms = the filter launches alone, query_ms = whole queries (COUNT: + the
 * one-workgroup reduction).  Up to 4096 launches per lane between two calls. */
int hipEngineKernelTiming(struct engineS *engine, int enable);
int hipEngineKernelTime(struct engineS *engine, double *scan_ms, double *query_ms, int *launches);

/* Which of the reference's two SELECT row selections index mode follows.  Off (the default): QPESeq's -- only
 * u64 / int indexes are probed (engine/serial/executeEngine-serial.c:377-433).  On: QPEOMP's / QPEMPI's -- BOOL indexes
 * are probed as well (engine/omp/executeEngine-omp.c:424-459, same block in engine/mpi), which changes the answers of
 * queries with a top-level condition on an indexed BOOL column: rows come back in the index's order (key ascending, row
 * descending), a row once per probe that finds it, and an OR beside the probed condition loses its other side.  The
 * one-thread order of that engine is reproduced (its append order across threads is a race).  Also switched on for a
 * new engine by PQPS_PROBE_BOOL=1.  Returns the previous setting, -1 on a NULL engine. */
int hipEngineProbeBoolIndexes(struct engineS *engine, int enable);

/* Number of device shards the engine's table is split into (1 unless PQPS_DEVICES names several devices);
 * `rows` (may be NULL, room for that many entries) receives the rows each shard holds. */
int hipEngineShards(struct engineS *engine, unsigned long long *rows, int capacity);

/* Grouped COUNT(*): how many matching rows carry each value of one column (no aggregates in the reference; the SQL layer
 * stays the reference's, so this is reached through the C API and the Python package only).
 * SEMANTICS: the counts are the rows executeQuerySelectIdsHIP(engine, whereClause) returns, grouped by the value of
 * `groupColumn` -- in index mode too, rows that several probed conditions return more than once included; `total` equals
 * that call's count.  A NULL WHERE groups the whole table; a WHERE that matches nothing gives numGroups = 0, success = true.
 * Groups with at least one row only, in ascending key order: numeric order for i32 columns, false before true, the
 * dictionary's strcmp order for string columns.  keys: the i32 value, 0 / 1, or the dictionary code at the time of the query;
 * keyText: as get_attribute_string_value (serial:216-248) formats the value (%d, true / false, the string).
 * REFUSED (success = false, the reason on stderr): command_id (u64 and unique: grouping on it is the SELECT itself), an
 * unknown column, more than 65 536 groups in the column's range (e.g. timestamp on a 1 M-row CSV), an engine joined across
 * ranks (hipEngineJoinRanksHIP).  A reader like COUNT: it takes a query lane, so the lane rules above apply (a thread that
 * holds every lane is refused at once).  Execution: a single-pass scan-mode WHERE runs ONE fused filter-and-histogram launch
 * per shard (pqps_filter_group); index probes and WHERE lists of several passes run the selection and then
 * pqps_group_list over each shard's list; the shards' bins are summed on the host.  i32 columns: the value range is found
 * on first use (pqps_column_bounds) and cached with the table. */
struct hipGroupResult {
    int column;                        /* HIPCOL_* of the group column                                   */
    int kind;                          /* HIPKIND_I32 / _BOOL / _DICT                                    */
    int numGroups;                     /* groups with at least one row, ascending key order              */
    long long total;                   /* sum of counts                                                  */
    long long *keys;                   /* i32 value, 0/1, or dictionary code at the time of the query    */
    char **keyText;                    /* owned copies, formatted as get_attribute_string_value would    */
    unsigned long long *counts;
    double queryTime;
    bool success;
};
struct hipGroupResult *executeQueryGroupCountHIP(struct engineS *engine, const char *groupColumn,
                                                 struct whereClauseS *whereClause);
void freeGroupResultHIP(struct hipGroupResult *result);

/* COUNT, SUM, MIN and MAX of one numeric column, overall or per group (no aggregates in the reference; reached through the
 * C API and the Python package only, like the grouped COUNT above).
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns -- in index mode too, so a row several probed
 * conditions return more than once is counted and added that many times, as in executeQueryGroupCountHIP; `total` equals
 * that call's count.
 * NO GROUP BY (groupColumn == NULL): one group over all those rows -- numGroups is 1 if any row matches and 0 otherwise;
 * keys and keyText are NULL, groupColumn and groupKind are -1.
 * GROUP BY: the groups, keys, key text and key order of executeQueryGroupCountHIP for the same column and WHERE, and
 * counts[g] equals its count.
 * VALUES: exit_code, user_id, risk_level (HIPKIND_I32): sums exact in int64 (no overflow below 2^32 rows), min / max signed.
 * command_id (HIPKIND_U64): the sum is modulo 2^64, min / max unsigned, all three returned as the u64 bits in the long long
 * fields (valueKind says which).  There is no AVG on the device: AVG is sums[g] / counts[g].
 * REFUSED (success = false, the reason on stderr): a dictionary or boolean value column, an unknown value or group column,
 * and every group-column refusal of executeQueryGroupCountHIP (command_id, more than 65 536 groups, an engine joined across
 * ranks -- with or without GROUP BY).  A reader like COUNT: shared lock and one query lane; the lane rules above apply.
 * Execution: as executeQueryGroupCountHIP -- a single-pass scan-mode WHERE runs ONE fused filter-and-aggregate launch per
 * shard (pqps_filter_aggregate), everything else the selection and then pqps_aggregate_list over each shard's list; shards
 * are combined on the host.  An empty table, or a WHERE that matches nothing, gives numGroups = 0 with success = true. */
struct hipAggregateResult {
    int valueColumn, valueKind;        /* HIPCOL_*, HIPKIND_I32 / HIPKIND_U64                            */
    int groupColumn, groupKind;        /* HIPCOL_*, HIPKIND_*; -1 / -1 without GROUP BY                  */
    int numGroups;
    long long total;                   /* sum of counts = executeQuerySelectIdsHIP's count               */
    long long *keys;                   /* as hipGroupResult; NULL without GROUP BY                       */
    char **keyText;                    /* as hipGroupResult; NULL without GROUP BY                       */
    unsigned long long *counts;
    long long *sums, *mins, *maxs;     /* u64 bits when valueKind == HIPKIND_U64                         */
    double queryTime;
    bool success;
};
struct hipAggregateResult *executeQueryAggregateHIP(struct engineS *engine, const char *valueColumn, const char *groupColumn,
                                                    struct whereClauseS *whereClause);
void freeAggregateResultHIP(struct hipAggregateResult *result);

/* GROUP BY buckets: COUNT(*), or COUNT / SUM / MIN / MAX of one numeric column, per PREFIX of a string column or per RANGE
 * of an i32 column -- "how many per hour / per day" of the ISO-8601 `timestamp` (prefix 13 is an hour, 10 a day, 7 a month),
 * user_id in ranges of 100 (no aggregates in the reference; reached through the C API and the Python package only, like the
 * grouped COUNT above).
 * BUCKETS: HIPBUCKET_PREFIX, bucketArg = k >= 1, a string column: the bucket of a row is the first min(k, strlen) bytes of
 * its string; keys[g] is the lowest dictionary code of the bucket at the time of the query, keyText[g] the truncated string.
 * HIPBUCKET_WIDTH, bucketArg = w >= 1, an i32 column: the bucket is floor(value / w), floor towards minus infinity;
 * keys[g] is its lower bound floor(value / w) * w (it may lie below INT_MIN), keyText[g] is %lld of it.
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns -- in index mode too, so a row several probed
 * conditions return more than once counts that many times; `total` equals that call's count.  Only buckets with at least one
 * row are listed, in ascending key order (strcmp order of the prefixes, numeric order of the lower bounds).
 * VALUES (valueColumn != NULL): as executeQueryAggregateHIP -- i32 sums exact in int64, command_id sums modulo 2^64 with
 * unsigned min / max, returned as the u64 bits (valueKind says which).  Without a value column sums, mins and maxs are NULL.
 * MARGINALS: for every WHERE, adding executeQueryGroupCountHIP's counts over the values of a bucket gives that bucket's
 * count; a prefix longer than every string (and a width of 1) gives exactly executeQueryGroupCountHIP's groups.
 * SPECIAL CASES: a NULL WHERE groups the whole table; no match, or an empty table, gives numGroups = 0 with success = true;
 * a single-valued dictionary column (no device buffer) gives one bucket from the selection, with no bucket kernel -- with a
 * value column the ungrouped aggregate.
 * REFUSED (success = false, the reason on stderr): everything hipBucketBounds refuses (k < 1 or w < 1, PREFIX on a numeric
 * or boolean column, WIDTH on a string or boolean column, command_id, an unknown column, more than 65 536 buckets), an
 * unknown value column, a dictionary or boolean value column, an engine joined across ranks.  NOT refused: a dictionary of
 * any size (timestamp on a 1 M-row CSV) or an i32 column spanning more than 65 536 values, while the BUCKETS are at most
 * 65 536.  A reader like COUNT: shared lock and one query lane; the lane rules above apply.
 * Execution: the bounds (the ascending run starts of the buckets in bin space, hipBucketBounds) are built once per query on
 * the host and uploaded once per shard into scratch of the query's own, freed with it.  A single-pass scan-mode WHERE runs
 * ONE fused launch per shard (pqps_filter_group_buckets / pqps_filter_aggregate_buckets); index probes, WHEREs of several
 * passes and fragmented LIKE / IN sets run the selection and then pqps_group_buckets_list / pqps_aggregate_buckets_list over
 * each shard's list; shards' buckets are added or merged on the host.  The i32 range is the table's cached one (it may be
 * wider than the data after a DELETE: empty buckets are never listed). */
enum { HIPBUCKET_PREFIX = 1, HIPBUCKET_WIDTH = 2 };
struct hipBucketResult {
    int groupColumn, groupKind;        /* HIPCOL_*, HIPKIND_DICT / HIPKIND_I32                           */
    int bucketMode;                    /* HIPBUCKET_*                                                    */
    long long bucketArg;               /* k or w                                                         */
    int valueColumn, valueKind;        /* -1 / -1: no value column, COUNT(*) per bucket only             */
    int numGroups;                     /* buckets with at least one row, ascending key order             */
    long long total;                   /* sum of counts = executeQuerySelectIdsHIP's count               */
    long long *keys;                   /* lowest code of the prefix's run / lower bound of the range     */
    char **keyText;                    /* owned: the truncated string / %lld of the lower bound          */
    unsigned long long *counts;
    long long *sums, *mins, *maxs;     /* NULL without a value column; u64 bits for command_id           */
    double queryTime;
    bool success;
};
struct hipBucketResult *executeQueryGroupBucketsHIP(struct engineS *engine, const char *groupColumn, int bucketMode,
                                                    long long bucketArg, const char *valueColumn /* may be NULL */,
                                                    struct whereClauseS *whereClause);
void freeBucketResultHIP(struct hipBucketResult *result);

/* COUNT(DISTINCT one column), overall or per group (no aggregates in the reference; reached through the C API and the
 * Python package only, like the grouped COUNT above -- the SQL driver has no COUNT(DISTINCT ...), so its output stays that
 * of QPESeq).
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns.  In index mode a row several probed
 * conditions return more than once is a duplicate: it changes no distinct count, but it counts in `total`, which equals
 * that call's count.
 * DISTINCT: the number of different values of `valueColumn` among those rows.  exit_code, user_id, risk_level compare by
 * signed value, command_id as u64, sudo_used as a bool, string columns by string equality (code equality: a dictionary
 * holds each string once); a single-valued string column (no device buffer) gives 1 for every group with rows, with no
 * kernel.  Every one of the 12 columns may be the value column, the group column too (then every group gives 1).
 * NO GROUP BY (groupColumn == NULL): numGroups is 1 if any row matches and 0 otherwise; keys and keyText are NULL,
 * groupColumn and groupKind are -1, as in hipAggregateResult.
 * GROUP BY: the groups, keys, key text and key order of executeQueryGroupCountHIP for the same column and WHERE; a group is
 * listed iff it has a matching row, i.e. iff distinct[g] >= 1.
 * REFUSED (success = false, the reason on stderr): an unknown value or group column, and every group-column refusal of
 * executeQueryGroupCountHIP (command_id, more than 65 536 groups, an engine joined across ranks -- with or without GROUP
 * BY).  Nothing is refused for the size of the value domain.  A reader like COUNT: shared lock and one query lane; the
 * lane rules above apply.
 * Execution: value bins are dictionary codes, 0 / 1, or value - min for an i32 column (the range cached with the table and
 * widened by INSERT).  With G groups and W = ceil(bins / 32) words, a presence bitmap of G x W x 32 <= 2^30 bits per shard:
 * a single-pass scan-mode WHERE runs ONE fused filter-and-bitmap launch per shard (pqps_filter_distinct), everything else
 * the selection and then pqps_distinct_list over each shard's list; shards' bitmaps are OR-ed before the popcount.
 * command_id, or a bitmap over the cap: the selection, a radix sort of the (group, value) keys of each shard's list
 * (pqps_distinct_sort), several shards merged on the host with duplicates dropped -- shard counts are never added.  An empty
 * table, or a WHERE that matches nothing, gives numGroups = 0 with success = true. */
struct hipDistinctResult {
    int valueColumn, valueKind;        /* HIPCOL_*, HIPKIND_*                                              */
    int groupColumn, groupKind;        /* HIPCOL_*, HIPKIND_*; -1 / -1 without GROUP BY                    */
    int numGroups;
    long long total;                   /* executeQuerySelectIdsHIP's count                                  */
    long long *keys;                   /* as hipGroupResult; NULL without GROUP BY                         */
    char **keyText;                    /* as hipGroupResult; NULL without GROUP BY                         */
    unsigned long long *distinct;      /* distinct values per group, >= 1                                  */
    double queryTime;
    bool success;
};
struct hipDistinctResult *executeQueryCountDistinctHIP(struct engineS *engine, const char *valueColumn, const char *groupColumn,
                                                       struct whereClauseS *whereClause);
void freeDistinctResultHIP(struct hipDistinctResult *result);

/* GROUP BY two columns: COUNT(*), or COUNT / SUM / MIN / MAX of one numeric column, per pair of values (no aggregates in the
 * reference; reached through the C API and the Python package only, like the grouped COUNT above).
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns -- in index mode too, so a row several probed
 * conditions return more than once is counted and added that many times, as in executeQueryGroupCountHIP and
 * executeQueryAggregateHIP; `total` equals that call's count.
 * GROUPS: a group is a pair (value of A, value of B) that at least one of those rows carries.  Pairs come in ascending
 * lexicographic order: A's key order first, then B's, each column in executeQueryGroupCountHIP's key order (numeric for
 * i32, false before true, the dictionary's strcmp order); keys[j] and keyText[j] per column are exactly that call's.
 * VALUES (valueColumn != NULL): as executeQueryAggregateHIP -- i32 sums exact in int64, command_id sums modulo 2^64 with
 * unsigned min / max, returned as the u64 bits (valueKind says which).  Without a value column sums, mins and maxs are NULL.
 * There is no AVG on the device.
 * MARGINALS: for every WHERE, summing counts over B for a fixed A gives executeQueryGroupCountHIP(A)'s count; summing sums
 * and taking the min of mins and the max of maxs over B gives executeQueryAggregateHIP(value, A).
 * SPECIAL CASES: a NULL WHERE groups the whole table; no match, or an empty table, gives numGroups = 0 with success = true;
 * A == B is allowed (only diagonal pairs occur); a single-valued dictionary column (no device buffer) as A or B contributes
 * its one key to every pair -- the query then runs as the one-column form on the other column, and as one group from the
 * selection when both are single-valued.
 * REFUSED (success = false, the reason on stderr): an unknown group or value column, a dictionary or boolean value column,
 * and for either group column alone everything executeQueryGroupCountHIP refuses (command_id, an i32 column spanning more
 * than 65 536 values, an engine joined across ranks).  NOTHING is refused for the size of the product: two columns of
 * 65 536 bins each are a legal query.  A reader like COUNT: shared lock and one query lane; the lane rules above apply.
 * Execution: with D = bins of A x bins of B (a 64-bit product).  D <= 65 536: a single-pass scan-mode WHERE runs ONE fused
 * launch per shard (pqps_filter_group_pair), everything else the selection and then pqps_group_pair_list over each shard's
 * list; shards' bins are added on the host.  D > 65 536, on any WHERE: the selection, then per shard a radix sort of the
 * listed rows' composite keys and a run reduction on the device (pqps_group_pair_sort); the download is one entry per pair
 * that occurs, and shards' runs are merged by key on the host (counts and sums added, min / max taken). */
struct hipGroupPairResult {
    int groupColumn[2], groupKind[2];   /* HIPCOL_*, HIPKIND_I32 / _BOOL / _DICT                          */
    int valueColumn, valueKind;         /* -1 / -1: no value column, COUNT(*) per pair only                */
    int numGroups;                      /* pairs with at least one row                                     */
    long long total;                    /* sum of counts = executeQuerySelectIdsHIP's count                */
    long long *keys[2];                 /* per pair, as hipGroupResult.keys for that column                */
    char **keyText[2];                  /* per pair, owned copies, as get_attribute_string_value formats   */
    unsigned long long *counts;
    long long *sums, *mins, *maxs;      /* NULL without a value column; u64 bits for command_id            */
    double queryTime;
    bool success;
};
struct hipGroupPairResult *executeQueryGroupPairHIP(struct engineS *engine, const char *groupColumnA, const char *groupColumnB,
                                                    const char *valueColumn /* may be NULL */, struct whereClauseS *whereClause);
void freeGroupPairResultHIP(struct hipGroupPairResult *result);

/* ORDER BY one column [ASC | DESC] with LIMIT (the reference parses ORDER BY into ParsedSQL.order_by / order_desc and
 * executes it nowhere; reached through the C API and the Python package only -- the SQL driver still ignores it, so its
 * output stays that of QPESeq).
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns -- in index mode too, so a row several
 * probed conditions return appears that many times, as in executeQueryGroupCountHIP / executeQueryAggregateHIP; *matches
 * equals that call's count.
 * ORDER: by the key of `orderColumn`, ascending, or descending with `descending`; TIES BY ASCENDING ROW NUMBER in both
 * directions (copies of a row in index mode are adjacent: they share key and row).  The order is total and the same for
 * every shard layout and every path.  exit_code, user_id, risk_level: signed.  command_id: unsigned 64-bit.  sudo_used:
 * false before true.  String columns: the dictionary's strcmp order (the order-preserving codes); a single-valued string
 * column makes every key equal, so the answer is the first rows by row number.  Every one of the 12 columns can be an
 * order column.
 * LIMIT: limit > 0 gives the first min(limit, matches) rows of that order, limit <= 0 all of them (a full ORDER BY).
 * REFUSED (-1 / success = false, the reason on stderr): an unknown order column, and an engine joined across ranks.
 * A reader like COUNT: shared lock and one query lane, the lane rules above apply; the device scratch of a query is
 * allocated for it and freed with it, so two lanes never share any.
 * Execution: a single-pass scan-mode WHERE with 0 < limit <= 1024 (512 for command_id) runs ONE fused filter-and-top-K
 * launch per shard (pqps_filter_topk) and small rounds that reduce its waves' partial rows; everything else runs the
 * selection, then per shard the same top-K selection over its list (pqps_topk_list) or, for limit <= 0 or above those
 * bounds, a stable radix sort of the list (pqps_sort_list).  Shards are merged on the host.  An empty table, or a WHERE
 * that matches nothing, gives 0 rows with matches = 0 and success. */
/* Row numbers of the first `limit` rows (all if limit <= 0) in that order; returns how many were written to *ids
 * (malloc'd, caller frees), -1 on error or refusal.  *matches (may be NULL) = executeQuerySelectIdsHIP's count. */
long long executeQueryOrderIdsHIP(struct engineS *engine, struct whereClauseS *whereClause, const char *orderColumn,
                                  bool descending, long long limit, unsigned int **ids, long long *matches, double *queryTime);
/* The same rows, projected: a hipColumnarResult whose numRecords rows are in that order (cells exactly as
 * executeQuerySelectColumnarHIP makes them; hipColumnarHead / hipColumnarCellText work on it unchanged).  *matches (may
 * be NULL) as above. */
struct hipColumnarResult *executeQuerySelectOrderedHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                       struct whereClauseS *whereClause, const char *orderColumn,
                                                       bool descending, long long limit, long long *matches);

/* ORDER BY k1 [DESC], ... , kN [DESC] LIMIT: 1 <= numKeys <= HIP_ORDER_MAX_KEYS (hipPredicate.h).  The rows and *matches are
 * those of the one-column calls; the order is lexicographic by the keys, each in its column's order above and reversed by its
 * own `descending`; rows equal in ALL keys come in ascending row number, whatever the directions.  A column named a second
 * time and a single-valued string column carry no information and are ignored: with one key left the query IS the
 * one-column query, with none the answer is the row order.  Otherwise the keys are packed into one number per row
 * (hipOrderKeyPlan: ceil(log2 domain) bits per key from the dictionary counts and the table-wide i32 bounds) and the three
 * paths above run on it: up to 32 bits as the narrow key (limit <= 1024 for the top-K paths), up to 64 as the wide key
 * (limit <= 512); more than 64 bits, or command_id among several keys, takes one stable radix sort per key
 * (pqps_sort_list_chain) whatever the limit.  Refused (-1 / success = false, reason on stderr): numKeys outside 1 .. 4, a NULL
 * or unknown column, an engine joined across ranks. */
struct hipOrderKey { const char *column; bool descending; };
long long executeQueryOrderIdsByHIP(struct engineS *engine, struct whereClauseS *whereClause, const struct hipOrderKey *keys,
                                    int numKeys, long long limit, unsigned int **ids, long long *matches, double *queryTime);
struct hipColumnarResult *executeQuerySelectOrderedByHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                         struct whereClauseS *whereClause, const struct hipOrderKey *keys, int numKeys,
                                                         long long limit, long long *matches);

/* The first row of every group: per value of `groupColumn`, the matching row that comes first in the order of `orderColumn`
 * -- "the latest command of every user", "the first sudo on every host" (SQL: DISTINCT ON, ROW_NUMBER() OVER (PARTITION BY
 * g ORDER BY k) = 1, argMin / argMax; no counterpart in the reference, reached through the C API and the Python package only
 * -- the SQL driver has no GROUP BY, so its output stays that of QPESeq).
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns.  In index mode a row several probed
 * conditions return more than once changes nothing except `total`, which equals that call's count.
 * GROUPS: the groups, keys, key text and key order of executeQueryGroupCountHIP for the same column and WHERE; a group is
 * listed iff it has a matching row.  groupColumn == NULL: one group over all those rows -- numGroups is 1 if any row matches
 * and 0 otherwise, keys and keyText are NULL, groupColumn and groupKind are -1, as in hipAggregateResult.
 * ORDER: exactly executeQueryOrderIdsHIP's -- exit_code, user_id, risk_level signed, command_id unsigned 64-bit, false before
 * true, string columns in the dictionary's strcmp order (the codes); ascending, or descending with `descending`; TIES GO TO
 * THE LOWEST ROW NUMBER IN BOTH DIRECTIONS.  Every one of the 12 columns can be the order column; a single-valued string
 * column (no device buffer) makes every key equal, so the answer is the lowest matching row of each group.  Group column ==
 * order column is legal.
 * CONSEQUENCE: for every WHERE, rows[g] equals the first row of executeQueryOrderIdsHIP(whereClause AND groupColumn =
 * keyText[g], orderColumn, descending, limit 1); with groupColumn == NULL it equals that call's for whereClause itself.
 * REFUSED (success = false, the reason on stderr): an unknown group or order column, and every group-column refusal of
 * executeQueryGroupCountHIP (command_id as the group column, more than 65 536 groups, an engine joined across ranks -- with
 * or without GROUP BY).  NOTHING is refused for the size of the order column's domain: timestamp with 4-byte codes on a
 * 1 M-row CSV is a legal order column.  A reader like COUNT: shared lock and one query lane, the lane rules above apply; the
 * device buffers of a query are allocated for it and freed with it.
 * Execution: as executeQueryAggregateHIP -- a single-pass scan-mode WHERE runs ONE fused launch per shard
 * (pqps_filter_group_first: one 64-bit atomic min per matching row; two launches, i.e. two scans of the WHERE, for
 * command_id, whose keys need 96 bits), everything else the selection and then pqps_group_first_list over each shard's list.
 * Shards are merged on the host by the minimum word per bin (rows are table-wide; command_id compares (key, row)).  A
 * single-valued group column gives one group from the ungrouped form.  An empty table, or a WHERE that matches nothing,
 * gives numGroups = 0 with success = true. */
struct hipGroupFirstResult {
    int groupColumn, groupKind;        /* HIPCOL_*, HIPKIND_*; -1 / -1 without GROUP BY                    */
    int orderColumn, orderKind;        /* HIPCOL_*, HIPKIND_*                                              */
    bool descending;
    int numGroups;
    long long total;                   /* executeQuerySelectIdsHIP's count                                  */
    long long *keys;                   /* as hipGroupResult; NULL without GROUP BY                         */
    char **keyText;                    /* as hipGroupResult; NULL without GROUP BY                         */
    unsigned int *rows;                /* table-wide row number of each group's first row                  */
    long long *orderKeys;              /* that row's order key: i32 value, 0 / 1, dictionary code at the time of the query,
                                          the u64 bits for command_id                                      */
    char **orderText;                  /* owned: as get_attribute_string_value formats the order column's cell */
    double queryTime;
    bool success;
};
struct hipGroupFirstResult *executeQueryGroupFirstHIP(struct engineS *engine, const char *groupColumn /* may be NULL */,
                                                      const char *orderColumn, bool descending, struct whereClauseS *whereClause);
void freeGroupFirstResultHIP(struct hipGroupFirstResult *result);
/* The same rows, projected: a hipColumnarResult whose numRecords = numGroups rows are those first rows in group key order
 * (cells exactly as executeQuerySelectColumnarHIP makes them; the device gather executeQuerySelectOrderedHIP uses).
 * *matches (may be NULL) = executeQuerySelectIdsHIP's count. */
struct hipColumnarResult *executeQuerySelectGroupFirstHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                          struct whereClauseS *whereClause, const char *groupColumn /* may be NULL */,
                                                          const char *orderColumn, bool descending, long long *matches);

/* THE FIRST N ROWS OF EVERY GROUP: per value of `groupColumn`, the n matching rows that come first in the order of
 * `orderColumn` -- "the n latest commands of every user", "the three riskiest commands per host" (SQL: ROW_NUMBER() OVER
 * (PARTITION BY g ORDER BY k [DESC]) <= n; no counterpart in the reference, reached through the C API and the Python package
 * only, as every grouped form is).
 * ROWS: exactly the rows executeQuerySelectIdsHIP returns, each row at most once.  An index-mode duplicate changes nothing
 * but `total`.
 * GROUPS: the groups, keys, key text and key order of executeQueryGroupFirstHIP.  groupColumn == NULL means one group.
 * ORDER: exactly executeQueryOrderIdsHIP's.  Ties go to the lowest row number in both directions.  Every one of the 12
 * columns is a legal order column, command_id included.  Single-valued columns are legal.  The order column may equal the
 * group column.
 * ANSWER: for each group that has a matching row, its first min(n, rows of the group) rows in that order.  Groups come in
 * key order, and rows in order inside each group: group g's rows are entries offsets[g] .. offsets[g + 1] of rows /
 * orderKeys / orderText.
 * CONSEQUENCE: the rows of group g are executeQueryOrderIdsHIP(orderColumn, whereClause AND groupColumn = keyText[g],
 * descending, limit n) with repeated ids removed.  With n = 1 the answer is executeQueryGroupFirstHIP's.
 * N: any n >= 1 is legal.  Nothing is refused for the size of n or of the order column's domain.
 * REFUSED (success = false, the reason on stderr): n < 1, unknown columns, and every group-column refusal of
 * executeQueryGroupFirstHIP: command_id as the group column, more than 65 536 bins, an engine joined across ranks.
 * CONCURRENCY: a reader like COUNT: shared lock, one lane, and its device buffers live and die with the query.
 * An empty table, or a WHERE that matches nothing, gives numGroups = 0 with success = true.
 * Execution: routed as executeQueryGroupFirstHIP.  n up to the round cap (PQPS_HEAD_ROUNDS_MAX of pqps_hip.h; the
 * environment variable PQPS_HEAD_ROUNDS, read per query, lowers it -- 0: never -- for the bench): the ROUNDS form, a
 * single-pass scan-mode WHERE by pqps_filter_group_head (n scans issued back to back, no host wait between them), everything
 * else by the selection and pqps_group_head_list.  Above the cap both routes take the selection and the SORT form
 * (pqps_group_head_sort: one sort by (group, key, row), repeated ids out, the first n of every run kept by one flag pass
 * and a compaction).  Either way a shard hands at most n entries per bin, and hipHeadMerge (hipPredicate.h) keeps the n
 * smallest per bin of the shards' union. */
struct hipGroupHeadResult {
    int groupColumn, groupKind;        /* as hipGroupFirstResult                                            */
    int orderColumn, orderKind;
    bool descending;
    int limit;                         /* n                                                                 */
    int numGroups;
    long long total;                   /* executeQuerySelectIdsHIP's count                                  */
    long long *keys;                   /* as hipGroupFirstResult; NULL without GROUP BY                     */
    char **keyText;
    long long *offsets;                /* numGroups + 1 entries: group g's rows are offsets[g] .. offsets[g + 1] */
    unsigned int *rows;                /* offsets[numGroups] entries each, group by group, in order:         */
    long long *orderKeys;              /*   as hipGroupFirstResult's                                         */
    char **orderText;
    double queryTime;
    bool success;
};
struct hipGroupHeadResult *executeQueryGroupHeadHIP(struct engineS *engine, const char *groupColumn /* may be NULL */,
                                                    const char *orderColumn, bool descending, long long n,
                                                    struct whereClauseS *whereClause);
void freeGroupHeadResultHIP(struct hipGroupHeadResult *result);
/* The same rows, projected in answer order (cells exactly as executeQuerySelectColumnarHIP makes them).  *matches (may be
 * NULL) = executeQuerySelectIdsHIP's count; *offsets (may be NULL) = a malloc'd array of numGroups + 1 entries, as above
 * (the caller frees it; NULL after a refusal). */
struct hipColumnarResult *executeQuerySelectGroupHeadHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                         struct whereClauseS *whereClause, const char *groupColumn /* may be NULL */,
                                                         const char *orderColumn, bool descending, long long n, long long *matches,
                                                         long long **offsets);

/* EXACT PERCENTILES, overall or per group: "the median and p95 exit_code per host", "the timestamp by which half of each
 * user's risk-5 commands had happened" (SQL: PERCENTILE_DISC(p) WITHIN GROUP (ORDER BY valueColumn); no counterpart in the
 * reference, reached through the C API and the Python package only, as every grouped form is).  Exact: no tolerance, no
 * sketch, and no floating point anywhere in the choice of a row.
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns; as in executeQueryGroupCountHIP a row that
 * several probed conditions return more than once counts that many times.  `total` equals that call's count.
 * GROUPS: the groups, keys, key text and key order of executeQueryGroupCountHIP for the same column and WHERE, only groups
 * with a row; counts[g] equals its count.  groupColumn == NULL: one group over all those rows -- numGroups is 1 if any row
 * matches and 0 otherwise, keyText is NULL, groupColumn and groupKind are -1.
 * VALUE COLUMN: any of the 12 columns, in executeQueryOrderIdsHIP's ascending order: strings in dictionary (strcmp) order,
 * exit_code / user_id / risk_level signed, command_id unsigned 64-bit, false before true.
 * FRACTIONS: ppm[0 .. numFractions), 1 .. 16 of them, exact integers in PARTS PER MILLION, 0 .. 1 000 000, in any order,
 * repeats allowed.  For a group of n rows the answer for p is the element at 0-based rank max(ceil(p n / 10^6) - 1, 0) of the
 * group's ascending sort (hipQuantileRank, 64-bit integers): p = 0 the minimum, 1 000 000 the maximum, 500 000 the lower
 * median.  There is no PERCENTILE_CONT: interpolation needs the neighbouring rank too and means nothing for strings.
 * ANSWER: values[g * numFractions + f] = group g's value for ppm[f]: the i32 value, the u64 bits of command_id, 0 / 1, or the
 * dictionary code at the time of the query; for a string column valueText[g * numFractions + f] is its (owned) text, for
 * every other kind valueText is NULL.
 * REFUSED (success = false, the reason on stderr): an unknown value or group column, numFractions outside 1 .. 16, a ppm
 * above 1 000 000, and every group-column refusal of executeQueryGroupCountHIP (command_id as the group column, more than
 * 65 536 groups, an engine joined across ranks -- with or without GROUP BY).  NOTHING is refused for the size of the value
 * column's domain.  A reader like COUNT: shared lock and one query lane, the lane rules above apply; bounds and dictionaries
 * are read under the lock; the device buffers of a query are allocated for it and freed with it.
 * Execution: a radix select over the value column's order-preserving key image (dictionary code, i32 value minus the
 * table-wide minimum, the bool, command_id minus the selection's minimum -- one MIN / MAX aggregate first), B key bits planned
 * from the dictionary size or the bounds.  B is split into digits from the top (hipQuantileDigitBits: 11 bits while a launch
 * counts at most 8 tables, else 8; a domain of at most 2048 values is ONE pass); every pass is one counting scan per shard --
 * pqps_filter_digit_hist for a single-pass scan-mode WHERE, otherwise the selection ONCE and pqps_digit_hist_list over each
 * shard's list per pass -- whose tables are downloaded and summed over the shards on the host (a histogram is decomposable
 * where a quantile is not), and hipQuantilePick narrows every pending fraction by one digit.  Pass 0 also gives every
 * group's row count.  A launch counts at most 2^22 words (16 MiB per shard and pass): more groups than that run in batches of
 * consecutive bins (the environment variable PQPS_QUANTILE_WORDS, read per query, lowers the cap -- for the tests).  An
 * empty table, or a WHERE that matches nothing, gives numGroups = 0 with success = true. */
struct hipQuantileResult {
    int valueColumn, valueKind;        /* HIPCOL_*, HIPKIND_*                                               */
    int groupColumn, groupKind;        /* HIPCOL_*, HIPKIND_*; -1 / -1 without GROUP BY                     */
    int numGroups, numFractions;
    int passes;                        /* counting scans per shard the select took (batches counted)         */
    long long total;                   /* sum of counts = executeQuerySelectIdsHIP's count                   */
    char **keyText;                    /* as hipGroupResult; NULL without GROUP BY                           */
    unsigned long long *counts;        /* numGroups: the rows of every group                                 */
    long long *values;                 /* [numGroups * numFractions]: i32 value, u64 bits, code, or 0 / 1     */
    char **valueText;                  /* strings only, else NULL: [numGroups * numFractions] owned texts     */
    double queryTime;
    bool success;
};
struct hipQuantileResult *executeQueryQuantilesHIP(struct engineS *engine, const char *valueColumn, const char *groupColumn /* may be NULL */,
                                                   const unsigned *ppm, int numFractions, struct whereClauseS *whereClause);
void freeQuantileResultHIP(struct hipQuantileResult *result);

/* THE TOP N GROUPS: GROUP BY one column of ANY size, ORDER BY an aggregate [DESC], LIMIT n -- "the 20 most frequent commands",
 * "the 10 users with the highest summed risk" (no aggregates in the reference; reached through the C API and the Python
 * package only, like the grouped COUNT above).
 * ROWS: exactly the rows executeQuerySelectIdsHIP(engine, whereClause) returns -- in index mode a row several probed conditions
 * return counts that many times, as in executeQueryGroupCountHIP.
 * GROUPS: the keys, key text and key order of executeQueryGroupCountHIP, but NOTHING is refused for the size of the column's
 * domain: any dictionary (raw_command, timestamp of a large CSV) and any i32 span, INT_MIN .. INT_MAX (2^32 bins) included.
 * VALUES (valueColumn, may be NULL: COUNT(*) only): as executeQueryAggregateHIP -- i32 sums exact in int64, command_id sums
 * modulo 2^64 and its min / max unsigned, returned as the u64 bits.
 * ORDER: by the aggregate `orderBy` names -- COUNT compares unsigned; SUM / MIN / MAX signed for an i32 value column and
 * unsigned on the u64 bits for command_id -- ascending, or reversed when `descending`.  Groups whose aggregate is equal come
 * in ascending key order in BOTH directions: the order is total, and the same for every shard layout and every path.
 * HIPTOP_BY_KEY is the key order, or its reverse.  (hipGroupTopOrder of hipPredicate.h is the rule, as host code.)
 * LIMIT: limit > 0 lists the first min(limit, groupsTotal) groups of that order, limit <= 0 all of them; `total` and
 * `groupsTotal` describe the whole answer either way.
 * A NULL WHERE groups the whole table; an empty table, or a WHERE that matches nothing, gives 0 groups with success = true; a
 * single-valued string column gives one group from the selection, with no kernel.
 * REFUSED (success = false, the reason on stderr): an unknown group or value column, command_id as the group column, a
 * dictionary or boolean value column, orderBy outside the enum, HIPTOP_BY_SUM / _MIN / _MAX without a value column, an engine
 * joined across ranks, a listing of more than INT_MAX groups (numGroups is an int: such an answer needs a LIMIT).  A reader
 * like COUNT: shared lock and one query lane, the lane rules above apply; device buffers are
 * allocated for the query and freed with it.
 * Execution, per shard.  Up to 65 536 bins: the dense bins of executeQueryGroupCountHIP / executeQueryAggregateHIP.  Above,
 * while the shard's bins (4 B each, 32 B with a value column) fit HIP_TOP_BINS_BUDGET: the wide bins in device memory behind
 * an LDS front -- ONE fused launch for a single-pass scan-mode WHERE (pqps_filter_group_wide), otherwise the selection and
 * pqps_group_wide_list over the shard's list -- compacted on the device to one entry per group that occurs
 * (pqps_bins_compact), which is all that is downloaded.  Above the budget: the selection's list sorted by bin and reduced run
 * by run (pqps_group_sort), the same compact format.  The shards' runs are merged
 * by key on the host (counts and sums added, min and max taken), ordered by hipGroupTopOrder, and only the listed groups get
 * their key text. */
enum { HIPTOP_BY_KEY = 0, HIPTOP_BY_COUNT = 1, HIPTOP_BY_SUM = 2, HIPTOP_BY_MIN = 3, HIPTOP_BY_MAX = 4 };
#define HIP_TOP_BINS_BUDGET (256ull << 20)   /* bytes of bins per shard: the part's 256 MiB of Infinity Cache */
struct hipGroupTopResult {
    int groupColumn, groupKind;        /* HIPCOL_*, HIPKIND_I32 / _BOOL / _DICT                            */
    int valueColumn, valueKind;        /* HIPCOL_*, HIPKIND_I32 / HIPKIND_U64; -1 / -1: COUNT(*) only      */
    int orderBy;                       /* HIPTOP_BY_*                                                      */
    bool descending;
    long long limit;
    int numGroups;                     /* groups listed: min(limit, groupsTotal), all when limit <= 0      */
    long long groupsTotal;             /* groups with at least one matching row                            */
    long long total;                   /* executeQuerySelectIdsHIP's count, over ALL groups                */
    long long *keys;                   /* as hipGroupResult, in the order asked for                        */
    char **keyText;                    /* as hipGroupResult                                                */
    unsigned long long *counts;
    long long *sums, *mins, *maxs;     /* NULL without a value column; u64 bits for command_id             */
    double queryTime;
    bool success;
};
struct hipGroupTopResult *executeQueryGroupTopHIP(struct engineS *engine, const char *groupColumn,
                                                  const char *valueColumn /* may be NULL */, int orderBy, bool descending,
                                                  long long limit, struct whereClauseS *whereClause);
void freeGroupTopResultHIP(struct hipGroupTopResult *result);

/* VALUE SETS: column IN (SELECT column FROM table WHERE ... [GROUP BY column HAVING agg op n]) -- a self semi-join whose set
 * stays on the device (no counterpart in the reference; reached through the C API and the Python package only).
 * A VALUE SET S belongs to one engine and one column B (`column`).  It is made from an inner WHERE chain (NULL: every row) and
 * an optional HAVING `aggregate op constant`.
 * INNER ROWS: the rows for which the inner WHERE is true, each row ONCE -- scan semantics also on an engine with indexes, as
 *   UPDATE and DELETE have them.  The chain may hold LIKE / IN and the IN SET nodes of sets made earlier.
 * WITHOUT HAVING S is the set of values of B that at least one inner row carries.  WITH HAVING S is the set of values v of B
 *   that at least one inner row carries AND whose aggregate over the inner rows carrying v satisfies `op constant`.  A value
 *   without inner rows is never in S: COUNT(*) < 5 and SUM(x) = 0 do not select it.
 *   aggregate: HIPTOP_BY_COUNT (COUNT(*); valueColumn is not read), HIPTOP_BY_SUM / _MIN / _MAX of valueColumn, a numeric
 *   column, with the arithmetic of executeQueryAggregateHIP: an i32 sum is an int64 compared signed, a command_id sum is taken
 *   mod 2^64 and compared unsigned, MIN and MAX are compared in value order.  op: "=", "!=", "<", ">", "<=", ">=".  constant:
 *   decimal text -- strtoll for the aggregates of an i32 column, strtoull for those of command_id and for COUNT; a negative
 *   constant where the number is unsigned, trailing garbage, an empty text or a value out of range is refused
 *   (hipCompileHaving of hipPredicate.h is that rule, as host code).  AVG is a follow-up.
 * OUTER USE: the whereClauseS node {attribute = A, operator = "IN SET" | "NOT IN SET", value = "<id>"} (the id in decimal) is
 *   true for a row iff its value of A is (is not) in S.  Like the other set operators it is reached through this API only, is
 *   never an index probe (in index mode it is part of the re-filter), and works in every call that takes a WHERE -- every
 *   reader form, DELETE and UPDATE -- as a member pass (pqps_member_flags) that reads the set's bitmap where the build left it.
 *   A string column A only with B = A; any i32 column A with any i32 column B (values of A outside B's range are no members);
 *   command_id and sudo_used neither as A nor as B.
 * LIFETIME: every successful writer (single and batch INSERT, DELETE, UPDATE -- and an UPDATE that put a new string into a
 *   dictionary, whatever became of its rows) makes every set of the engine STALE, because the codes may have moved, and gives
 *   their device memory back; a WHERE that names a stale set, a freed set or an unknown id is refused at compile, saying which.
 *   At most HIP_MAX_VALUE_SETS sets per engine that are not freed.  Creating a set is a READER: shared lock and one lane,
 *   legal from a thread that holds tickets, under the lane rules above.  hipEngineFreeSetHIP waits like a WRITER and is refused
 *   (-1, nothing freed) from a thread that holds a ticket.  destroyEngineHIP frees what is left.
 * REFUSED (success = false, the reason on stderr, nothing changed): an unknown column; command_id or sudo_used as B; a
 *   dictionary or boolean value column; SUM / MIN / MAX without a value column; an aggregate outside COUNT .. MAX; a bad op or
 *   constant; a domain that fits no route; an engine joined across ranks; one set too many; a WHERE that does not compile.
 * ROUTES, by the domain D of B (dictionary codes, or value - lo over the column's range), per shard:
 *   no HAVING, D <= PQPS_MEMBER_MAX_BITS: the presence bitmap of pqps_filter_distinct (a single-pass WHERE: ONE fused scan) or
 *     of pqps_distinct_list over the selection; the popcount is pqps_distinct_count's.
 *   HAVING, D <= 65 536: the dense bins of pqps_filter_group / pqps_filter_aggregate (or their list forms), then
 *     pqps_bins_having.  HAVING, D above, the bins (4 B for COUNT, 32 B with a value) within HIP_TOP_BINS_BUDGET: the wide bins
 *     of pqps_filter_group_wide / pqps_group_wide_list, then pqps_bins_having.  Anything larger is refused (follow-up: the runs
 *     of the sort form into a list set).
 *   ONE SHARD: neither bins nor bitmap leave the device; only `rows` and `members` come to the host, and the member pass of
 *   every later query reads the buffer the build wrote.  SEVERAL SHARDS: the shards' bitmaps are ORed, or their bins combined
 *   as the grouped queries combine them, on the host; the combined bins go to shard 0 for the same pqps_bins_having (the
 *   comparison exists once, in the kernel), and the resulting bitmap is placed on every shard.
 * hipEngineSetKeysHIP downloads the bitmap and decodes it as the grouped queries decode bins: the members' keys and key text
 * in key order (refused for a stale or freed set). */
#define HIP_MAX_VALUE_SETS 64
struct hipSetHaving {
    int aggregate;                     /* HIPTOP_BY_COUNT .. HIPTOP_BY_MAX                                  */
    const char *valueColumn;           /* SUM / MIN / MAX: a numeric column; COUNT: not read, may be NULL   */
    const char *op;
    const char *constant;
};
struct hipValueSet {
    bool success;
    unsigned int id;                   /* what an IN SET node names, in decimal; never 0 for a set that was made */
    int column, kind;                  /* B: HIPCOL_*, HIPKIND_DICT / HIPKIND_I32                           */
    unsigned long long members;        /* values in S                                                      */
    unsigned long long rows;           /* the inner rows                                                   */
    double queryTime;
};
struct hipSetKeys {
    bool success;
    int column, kind;
    int numKeys;
    long long *keys;                   /* as hipGroupResult: dictionary codes, or the i32 values            */
    char **keyText;                    /* as hipGroupResult                                                */
};
struct hipValueSet *hipEngineCreateSetHIP(struct engineS *engine, const char *column, struct whereClauseS *whereClause,
                                          const struct hipSetHaving *having /* may be NULL */);
struct hipSetKeys *hipEngineSetKeysHIP(struct engineS *engine, const struct hipValueSet *set);
void freeSetKeysHIP(struct hipSetKeys *keys);
/* Frees the set on the device and `set` itself: 0, or -1 (nothing freed) from a thread that holds a ticket.  A `set` that was
 * refused (success = false) is just freed. */
int hipEngineFreeSetHIP(struct engineS *engine, struct hipValueSet *set);

/* COUNT(*) through the backend API (the reference parser cannot express it,
 * SURVEY.md fact 10): scan-mode count of matching rows, no ID list. */
long long executeQueryCountHIP(struct engineS *engine, struct whereClauseS *whereClause);

/* SEVERAL COUNT(*) OVER ONE TABLE STATE, AS FEW SCANS AS THEY NEED (SQL: SELECT COUNT(*) FILTER (WHERE a), COUNT(*) FILTER
 * (WHERE b), ...; no counterpart in the reference).  counts[i] is exactly what executeQueryCountHIP(engine, whereClauses[i])
 * returns on the same table state, for every clause the engine accepts, a NULL clause (every row) included.
 *   FUSED   a clause that binds to ONE scan pass of at most PQPS_TT_LEAVES comparisons: hipCountManyPack (hipPredicate.h) packs
 *           these, in the caller's order, into batches of up to HIP_COUNT_MANY_BATCH clauses that share their comparisons and
 *           columns, and every batch is one pqps_filter_count_many launch per shard -- each column of the batch read once.
 *   CONSTANT  a clause that folds to true or false (a single-valued column, an empty IN list): answered from the row count,
 *           no launch.
 *   ALONE   every other clause -- more passes (over 32 comparisons, a fragmented LIKE / IN, IN SET) or 7 and more
 *           comparisons -- runs through the COUNT path of executeQueryCountHIP, one after the other on the call's lane.
 * (COUNT(*) is the scan-mode count whatever indexes the engine has -- executeQueryCountHIP never probes one -- so an indexed
 * attribute does not keep a clause out of a batch.)  Nothing is refused for its shape.
 * A reader like COUNT: the table locked shared, ONE lane, one bind per clause; the batches of all shards are issued under the
 * issue lock before the first wait, the shards' counts summed on the host.  From a thread that holds a ticket it behaves as
 * the other readers do.
 * Returns numQueries (0 for an empty list, `counts` not read), or -1 with `counts` untouched and the reason on stderr for: a
 * NULL engine or `counts`, numQueries < 0, a NULL `whereClauses` with numQueries > 0, a clause that fails to compile (a
 * malformed IN list, a stale set), an engine joined across ranks (as the grouped calls refuse it), a refused lane, a failed
 * device call. */
#define HIP_COUNT_MANY_BATCH 16
#define HIP_COUNT_MANY_MIN_BATCH 2      /* a batch of fewer clauses runs them ALONE: one clause is faster through COUNT's specialised kernels */
long long executeQueryCountManyHIP(struct engineS *engine, struct whereClauseS *const *whereClauses, int numQueries, long long *counts);

#ifdef __cplusplus
}
#endif
#endif /* EXECUTE_ENGINE_HIP_H */
