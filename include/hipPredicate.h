/* hipPredicate.h -- WHERE list -> device predicate program.
 *
 * Host-side compiler of the HIP engine.  It turns the reference's
 * `struct whereClauseS` list (include/executeEngine-serial.h) into the
 * pqps_predicate the filter kernel executes, with exactly the semantics of
 * the serial engine:
 *   evaluateWhereClause  engine/serial/executeEngine-serial.c:292-316
 *                        (right-recursive AND/OR, no precedence, nesting via sub)
 *   checkCondition       :251-289  (literal typed by the COLUMN: strtoull / atoi /
 *                        "true"|"1" / raw text; unknown attribute or operator = false)
 *   CMP_NUM / CMP_STR    :18-123   (strcmp byte order for the 7 string columns)
 * Strings never reach the GPU: a string column is stored as order-preserving
 * dictionary codes (rank in strcmp order), so `col OP "literal"` becomes a
 * window on the code -- decided on the host by two binary searches.
 */
#ifndef HIP_PREDICATE_H
#define HIP_PREDICATE_H

#include <stddef.h>
#include <stdint.h>
#include "executeEngine-serial.h"
#include "executeEngine-hip.h"
#include "pqps_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HIPKIND_U64 = 0, HIPKIND_I32 = 1, HIPKIND_BOOL = 2, HIPKIND_DICT = 3 };

/* What the compiler needs to know about one column of `record`. */
struct hipColumnInfo {
    int present;                 /* 0: column not materialised on the device       */
    int kind;                    /* HIPKIND_*                                      */
    uint32_t width;              /* bytes per row on the device: 1, 2, 4 or 8      */
    int dict_count;              /* HIPKIND_DICT: number of distinct values        */
    const char *const *dict;     /* ... ascending in strcmp order                  */
};

/* Indexed by HIPCOL_* (buildEngine-hip.h): the 12 columns in `record` order. */
struct hipSchema {
    struct hipColumnInfo col[PQPS_MAX_COLUMNS];
};

/* Compiles `where` (NULL = every row).  On success returns 0, fills *pred and
 * column_ids[0 .. pred->n_columns) with the HIPCOL_* id bound to each column
 * slot of the predicate.  Returns -1 and a message in err when the clause
 * cannot be expressed (more than PQPS_MAX_LEAVES reachable leaves, or a leaf
 * on a column that is not materialised). */
int hipCompileWhere(const struct hipSchema *schema, const struct whereClauseS *where,
                    pqps_predicate *pred, int column_ids[PQPS_MAX_COLUMNS],
                    char *err, size_t errlen);

/* A WHERE of any size as a sequence of passes.  Pass k < n_passes - 1 is evaluated into one flag byte per row
 * (pqps_filter_flags); a later pass reads those flags as a 1-byte column: column id PQPS_MAX_COLUMNS + k in its
 * column_ids.  The last pass yields the query's result.  Nearly every clause is a single pass; a clause with
 * more than PQPS_MAX_LEAVES reachable comparisons (or more than PQPS_MAX_COLUMNS columns once flags are
 * counted) is split along the reference's own evaluation order (evaluateWhereClause, serial:292-316). */
struct hipPass {
    pqps_predicate pred;
    int column_ids[PQPS_MAX_COLUMNS];
    /* a member pass (see below) instead of a filter pass: pred and column_ids are unused */
    int member;                  /* 0: filter pass, 1: member pass                              */
    int member_column;           /* HIPCOL_* id of the table column it reads                    */
    int member_form;             /* PQPS_MEMBER_BITMAP / PQPS_MEMBER_LIST                       */
    uint32_t member_base;        /* bitmap: bit i stands for the value member_base + i (mod 2^32) */
    uint64_t member_bits;        /* bitmap: number of bits                                      */
    uint32_t *member_bitmap;     /* (member_bits + 31) / 32 words, LSB first; malloc'd          */
    uint64_t *member_list;       /* list: ascending, duplicate-free values; malloc'd            */
    uint32_t member_count;       /* list: number of values                                      */
    uint32_t member_set;         /* a value set (IN SET, below): its id, and member_bitmap is NULL -- the bitmap is the
                                    set's own, on the device; 0: none                            */
};
struct hipPlan {
    int n_passes;
    struct hipPass *pass;        /* malloc'd; hipPlanFree */
};
/* SET PREDICATES.  Four operators beyond the reference's six: "LIKE", "NOT LIKE" (string columns; `%` any run of bytes,
 * `_` one byte, `\%` `\_` `\\` literals, byte-wise, the whole string) and "IN", "NOT IN" (any column; value = a
 * parenthesised list of single-quoted strings or bare tokens, each typed by the column as the literal of `=` is).  The host
 * decides them once per distinct value -- on the dictionary of a string column -- into sorted runs of codes / values:
 *   no run, or the whole domain: a constant;
 *   up to PQPS_MEMBER_MAX_RUNS runs (else: so many runs of the complement within the column's domain): that many window
 *     leaves, an OR ladder (an AND ladder of negated windows for the NOT form / the complement) -- `a IN (x, y)` compiles
 *     to the very predicate of `a = x OR a = y`;
 *   anything more fragmented: a MEMBER PASS of the plan, numbered like the other passes and in front of them, which
 *     pqps_member_flags evaluates into the flag column PQPS_MAX_COLUMNS + pass; the node itself is the leaf `flags = 1`
 *     (negated for the NOT form).  Dictionary codes and bool: a bitmap over [first, last] selected code; an i32 column: a
 *     bitmap over [min, max] of the list when that is at most PQPS_MEMBER_MAX_BITS values, else the sorted list of u32 bit
 *     patterns; command_id: the sorted list.
 * LIKE on a numeric or boolean column and a malformed IN list (no parentheses, an unterminated quote, an empty item, more
 * than PQPS_MEMBER_MAX_ITEMS items) fail the compile.  hipCompileWhere fails for a WHERE that needs a member pass. */
#define PQPS_MEMBER_MAX_RUNS  4
#define PQPS_MEMBER_MAX_ITEMS 65536
#define PQPS_MEMBER_MAX_BITS  (1ull << 27)
int hipCompileWherePlan(const struct hipSchema *schema, const struct whereClauseS *where,
                        struct hipPlan *plan, char *err, size_t errlen);
void hipPlanFree(struct hipPlan *plan);

/* VALUE SETS.  Two more set operators, "IN SET" and "NOT IN SET": the node {attribute = A, value = "<id>"} is true for a row
 * iff its value of A is (is not) in the value set whose id the value text is, in decimal (hipEngineCreateSetHIP of
 * executeEngine-hip.h makes such sets and keeps their bitmaps on the device).  The compiler sees a set as a hipSetInfo:
 *   id       never 0
 *   column   HIPCOL_* id of the column B the set was made over
 *   kind     HIPKIND_DICT or HIPKIND_I32 (nothing else has sets)
 *   base, n_bits   bit i of the set's bitmap stands for the code i (base 0) or the i32 value base + i (mod 2^32)
 *   members  the number of set bits
 *   stale    the table was written after the set was made: its codes may have moved
 * Which A for which B: a string column only with itself (the codes of two dictionaries do not compare); any i32 column with
 * any i32 column (a value of A outside [base, base + n_bits) is no member); command_id and sudo_used never.
 * The node compiles to a MEMBER PASS with member_form = PQPS_MEMBER_BITMAP, member_base = base, member_bits = n_bits,
 * member_bitmap = NULL and member_set = id, read as the leaf `flags = 1` (negated for NOT IN SET) like every other member pass.
 * FOLDED TO A CONSTANT, no pass: a set without members (IN SET false, NOT IN SET true), and a string column's set that holds
 * the whole dictionary (IN SET true, NOT IN SET false) -- which is also how a single-valued column without a device buffer
 * is decided.  The compile FAILS, saying so in err, for: a value that is no decimal id, an id the table does not hold (never
 * made, or freed), a stale set, a pair of columns outside the rule above.
 * hipCompileWherePlanSets is hipCompileWherePlan given the table sets[0 .. n_sets) (NULL with 0); hipCompileWherePlan is that
 * call with no sets.  It and hipCompileWhere therefore refuse every chain that names a set. */
struct hipSetInfo {
    uint32_t id;
    int column;
    int kind;
    uint32_t base;
    uint64_t n_bits;
    uint64_t members;
    int stale;
};
int hipCompileWherePlanSets(const struct hipSchema *schema, const struct whereClauseS *where, const struct hipSetInfo *sets,
                            int n_sets, struct hipPlan *plan, char *err, size_t errlen);

/* THE HAVING OF A VALUE SET, `aggregate op constant`, as pqps_bins_having takes it; pure host code.
 *   aggregate   HIPTOP_BY_COUNT / _SUM / _MIN / _MAX (executeEngine-hip.h) -> field PQPS_HAVING_COUNT / _SUM / _MIN / _MAX
 *   value_kind  HIPKIND_I32 or HIPKIND_U64 for SUM / MIN / MAX (the value column's kind); not read for COUNT
 *   op          "=", "!=", "<", ">", "<=", ">=" (exactly so written) -> PQPS_HAVING_EQ .. _GE
 *   constant    decimal text, optional white space and sign in front, nothing behind the digits: strtoll for the aggregates of
 *               an i32 column, strtoull (no '-') for those of command_id and for COUNT.  SUM and COUNT keep the number's bits;
 *               MIN and MAX get its IMAGE: (u64)c ^ 2^63 for an i32 column (any int64 c: one outside the i32 range compares as
 *               it should), c itself for command_id.
 *   value_signed  1 for the SUM of an i32 column (compared as int64), else 0
 * Returns 0, or -1 with the reason on stderr and *out untouched for: a NULL argument, an aggregate outside COUNT .. MAX, a
 * value_kind that is no number where one is read, an unknown op, an empty constant, one without digits, trailing garbage, a
 * negative number where it is unsigned, a value out of the range of int64 / uint64. */
struct hipHaving {
    int field, op;
    uint64_t constant;
    int value_signed;
};
int hipCompileHaving(int aggregate, int value_kind, const char *op, const char *constant, struct hipHaving *out);

/* 1 for "LIKE", "NOT LIKE", "IN", "NOT IN", "IN SET", "NOT IN SET" (exactly so written), else 0. */
int hipIsSetOperator(const char *op);

/* THE SET LIST OF AN UPDATE.  One assignment `column = value`, its value text typed by the column exactly as the literal of
 * `=` is typed in a WHERE (checkCondition, serial:251-289): strtoull for command_id, atoi for the three i32 columns, "true"
 * (any case) or "1" for sudo_used and anything else false, the string itself for a string column. */
struct hipAssignment {
    int column;                  /* HIPCOL_* id                                                                   */
    int kind;                    /* HIPKIND_*                                                                     */
    uint64_t value;              /* U64: the value; I32: its u32 bit pattern; BOOL: 0 / 1; DICT: `rank`           */
    int present;                 /* DICT: 1 when the string is in the dictionary (numeric columns: 1)             */
    uint32_t rank;               /* DICT: number of dictionary values below the string -- its code when present,
                                    the rank it is inserted at otherwise                                         */
    const char *text;            /* DICT: the caller's string (not copied); NULL otherwise                        */
};
/* Compiles n assignments into out[0 .. n); pure host code.  Returns 0, or -1 with the reason on stderr and `out` untouched
 * for: an unknown column or one the schema does not hold, the same column twice, n < 1 or n > PQPS_MAX_COLUMNS, a NULL
 * value, an empty string for a string column, a string that does not fit its field of `record` with its NUL
 * (include/logType.h), command_id 0 (the last two are INSERT's own rules, serial:544-551). */
int hipCompileAssignments(const struct hipSchema *schema, const char *const *columns, const char *const *values, int n,
                          struct hipAssignment *out);

/* THE DICTIONARY MERGE OF A BATCH INSERT.  Two ascending, duplicate-free string lists -- a column's dictionary and the
 * dictionary of a batch of rows -- into their sorted union in strcmp order; pure host code.
 *   merged[0 .. *merged_count)   the union; the pointers are the inputs' own (nothing is copied), room for old_count +
 *                                new_count of them
 *   lut_old[old_count], lut_new[new_count]   the position of every input string in the union: what pqps_remap_codes sends the
 *                                table's and the batch's codes through
 *   *identity                    1 when lut_old[i] == i for every i -- every new string sorts behind every old one, or nothing
 *                                is new: the table's codes stay as they are
 * `column` (HIPCOL_* id of a string column) names the field of `record` the strings have to fit.  Returns 0, or -1 with the
 * reason on stderr and every output untouched for: a NULL pointer (a list may be NULL when its count is 0), a negative
 * count, a column that is no string column, a list that is not strictly ascending, an empty string (INSERT's rule,
 * serial:544-551), a string that does not fit its field with its NUL (the limit hipCompileAssignments enforces). */
int hipMergeDictionaries(const char *const *old_values, int old_count, const char *const *new_values, int new_count, int column,
                         const char **merged, int *merged_count, uint32_t *lut_old, uint32_t *lut_new, int *identity);

/* THE BUCKETS OF GROUP BY PREFIX(k) / WIDTH(w).  Dictionary codes are ranks in strcmp order and truncation to k bytes is
 * monotone under strcmp, so the strings of one prefix are one run of codes; the values of one width bucket are one run of
 * value - lo.  Both are therefore a short ascending list of run starts in bin space (code, or value - lo); pure host code.
 *   PREFIX (arg = k >= 1, a string column: dict[0 .. dict_count) ascending; lo / hi unused)
 *       bucket of a string = its first min(k, strlen) bytes; a bucket starts at every entry whose truncation differs from
 *       its predecessor's; key = the lowest code of the run (the key text is dict[key] cut to k bytes)
 *   WIDTH  (arg = w >= 1, an i32 column whose values lie in [lo, hi]; dict unused)
 *       bucket = floor(value / w) towards minus infinity; key = its lower bound floor(value / w) * w, which may lie below
 *       INT_MIN (the key text is %lld of it); run start j = max(lower bound j, lo) - lo; floor(hi / w) - floor(lo / w) + 1
 *       buckets
 *   (*bounds)[0 .. *n_buckets]   the run starts and, last, the sentinel: [0] == 0, strictly ascending, [*n_buckets] == the
 *                                domain (dict_count, or hi - lo + 1) -- what pqps_filter_group_buckets takes
 *   (*keys)[0 .. *n_buckets)     the key of every bucket
 * Both are malloc'd; the caller frees them.  Returns 0, or -1 with the reason on stderr and every output untouched for: a
 * NULL output, an unknown column, command_id, arg < 1, PREFIX on a numeric or boolean column, WIDTH on a string or boolean
 * column, an empty dictionary or range, a range of 2^32 values (no u32 holds its sentinel), more than HIPBUCKET_MAX
 * buckets. */
#define HIPBUCKET_MAX 65536u     /* mode: HIPBUCKET_PREFIX / HIPBUCKET_WIDTH of executeEngine-hip.h */
int hipBucketBounds(const char *column, const char *const *dict, int dict_count, int lo, int hi, int mode, long long arg,
                    uint32_t **bounds, long long **keys, uint32_t *n_buckets);

/* THE WORD OF "THE FIRST ROW OF EVERY GROUP".  pqps_filter_group_first / pqps_group_first_list leave one u64 per bin for a
 * narrow order column: (img ^ x) << 32 | row, img = v ^ 2^31 for an i32 column and the dictionary code or the bool otherwise,
 * x = 0xFFFFFFFF when descending and 0 otherwise; all ones = no row.  Pure host code.  Returns 0 for the empty word (*key and
 * *row untouched), -1 for a kind that has no such word (HIPKIND_U64: command_id takes the two-pass form), otherwise 1 with
 * *key = the i32 value, 0 / 1, or the dictionary code, and *row = the table-wide row number (either may be NULL). */
int hipFirstKeyDecode(int kind, int descending, unsigned long long word, long long *key, unsigned int *row);

/* THE SHARD MERGE OF "THE FIRST N ROWS OF EVERY GROUP" (executeQueryGroupHeadHIP).  Every shard hands its candidates -- at
 * most `limit` per bin -- as ONE list of n entries in ascending (bin, word) order: words[i] is the word of
 * pqps_filter_group_head for a narrow order column, (img ^ x) << 32 | row; for command_id best[i] = v ^ x and words[i] = the
 * row, in ascending (bin, best, word) order, and `best` is NULL otherwise.  Both forms of the query (the rounds and the sort)
 * hand this shape.  Rows are table-wide, so the words of different shards compare directly: per bin the merge keeps the
 * `limit` smallest entries of the union, command_id comparing (best, row); an entry equal in everything (the same row) on
 * two shards cannot happen and would be kept twice.  Pure host code, one pass over the lists.
 *   OUTPUT  out_bins / out_words / out_best (NULL unless the lists carry best) [0 .. return value): the kept entries in
 *           ascending (bin, [best,] word) order; each has room for the sum of the lists' n.
 * Returns -1 with the reason on stderr for limit < 1, a NULL list or output that is needed, lists with and without best
 * mixed, out of memory. */
struct hipHeadList { uint64_t n; const uint32_t *bins; const uint64_t *words; const uint64_t *best; };
long long hipHeadMerge(const struct hipHeadList *shards, int n_shards, long long limit, uint32_t *out_bins, uint64_t *out_words,
                       uint64_t *out_best);

/* THE PACKED KEY OF ORDER BY k1 [DESC], ... , kN [DESC].  Turns a key list into the fields of one unsigned number whose
 * ascending order is the lexicographic order of the keys, each in its own direction; pure host code.
 *   INPUT   columns[0 .. n_keys) / descending[0 .. n_keys): the key list, 1 <= n_keys <= HIP_ORDER_MAX_KEYS;
 *           dict_counts[c], lo[c], hi[c] (c = HIPCOL_* id, PQPS_MAX_COLUMNS entries each): the dictionary count of every
 *           string column and the table-wide [lo, hi] of every i32 column (lo > hi: no rows); other entries are not read.
 *   KEY LIST  a column named a second time is ignored at its later positions; a string column of at most one value is
 *           ignored; what remains are the fields, field 0 the most significant.
 *   FIELD   domain D = the dictionary count, 2 for sudo_used, hi - lo + 1 for an i32 column (2^64 for command_id);
 *           bits = ceil(log2 D) (0 for D <= 1, 32 for an i32 column over more than 2^31 values, 64 for command_id);
 *           base = lo as u32 for an i32 column, else 0; shift = the bits of all later fields (0 in the CHAIN form);
 *           a row's field = min(value - base, 2^bits - 1) ^ (descending ? 2^bits - 1 : 0), value - base in 32-bit arithmetic
 *   FORM    HIPORDER_ROWS    no field remains: the answer is the row order
 *           HIPORDER_ONE     one field remains: the one-column ORDER BY of field[0]
 *           HIPORDER_PACK32  T = total_bits <= 32: one u64 per row, packed << 32 | row
 *           HIPORDER_PACK64  32 < T <= 64: the pair (packed, row)
 *           HIPORDER_CHAIN   T > 64, or command_id among two or more fields: no packed key, one stable sort per field
 * Returns 0, or -1 with the reason on stderr and *plan untouched for: a NULL argument, n_keys outside
 * 1 .. HIP_ORDER_MAX_KEYS, a NULL or unknown column. */
#define HIP_ORDER_MAX_KEYS 4
enum { HIPORDER_ROWS = 0, HIPORDER_ONE = 1, HIPORDER_PACK32 = 2, HIPORDER_PACK64 = 3, HIPORDER_CHAIN = 4 };
struct hipOrderField {
    int column;                  /* HIPCOL_* id                                                                   */
    int kind;                    /* HIPKIND_*                                                                     */
    int descending;
    uint32_t base, bits, shift;
};
struct hipOrderKeyPlan {
    int form;                    /* HIPORDER_*                                                                    */
    int n_fields;
    uint32_t total_bits;         /* T                                                                             */
    struct hipOrderField field[HIP_ORDER_MAX_KEYS];
};
int hipOrderKeyPlan(const char *const *columns, const int *descending, int n_keys, const int *dict_counts,
                    const int *lo, const int *hi, struct hipOrderKeyPlan *plan);

/* THE ORDER OF "THE TOP N GROUPS" (executeQueryGroupTopHIP).  Orders the merged groups of a grouped answer by one of their
 * aggregates and lists the first `limit` of them; pure host code.
 *   INPUT   bins[0 .. n_groups): the groups' keys in bin space, all different (any order); counts; and, where order_by is
 *           HIPTOP_BY_SUM / _MIN / _MAX, sums (the i32 sums as two's-complement int64 bits, command_id's mod 2^64), min_images,
 *           max_images -- the u64 IMAGES of pqps_filter_aggregate, (u64)(i64)v ^ 2^63 for an i32 value and v itself for
 *           command_id -- with value_kind = HIPKIND_I32 or HIPKIND_U64.  Arrays the order does not read may be NULL.
 *   ORDER   HIPTOP_BY_KEY: the bin.  _COUNT: unsigned.  _SUM: signed for HIPKIND_I32, unsigned for HIPKIND_U64.  _MIN / _MAX:
 *           the images, unsigned (that IS the signed order of i32 values).  Ascending, or reversed when `descending`; groups
 *           that compare equal come in ascending bin order in BOTH directions, so the order is total.
 *   OUTPUT  order[0 .. return value): indices into the input arrays, the listed groups in order; the return value is
 *           min(limit, n_groups) for limit > 0 and n_groups for limit <= 0, and `order` has room for that many.
 * A partial selection: a heap of `limit` entries over one pass when limit < n_groups, a sort otherwise.  Returns -1 with the
 * reason on stderr and `order` untouched for: order_by outside the enum, a NULL array the order reads, a value_kind that is
 * no number where sums are compared, out of memory.  (HIPTOP_BY_*: executeEngine-hip.h.) */
long long hipGroupTopOrder(const uint64_t *bins, const uint64_t *counts, const uint64_t *sums, const uint64_t *min_images,
                           const uint64_t *max_images, uint64_t n_groups, int value_kind, int order_by, int descending,
                           long long limit, uint64_t *order);

/* THE BATCHES OF "SEVERAL COUNTS, ONE SCAN" (executeQueryCountManyHIP).  Packs the one-pass predicates of n queries, in the
 * caller's order and greedily, into batches that pqps_filter_count_many takes one launch each; pure host code.
 *   INPUT   queries[i].pred / .column_ids: a filter pass as hipCompileWherePlan leaves it in a one-pass plan (leaves sorted
 *           by column slot, the jump program in evaluation order, column_ids[slot] = HIPCOL_* id).  max_queries: queries per
 *           batch, 1 .. PQPS_COUNT_MANY_MAX.
 *   LEAVES  a batch's leaves are the DISTINCT windows (column, lo, span) of its queries, sorted by (column slot, lo, span).
 *           Polarity is not part of a leaf's identity: `negate` is 0 in the batch, and a window and its complement -- again
 *           a window in the kernels' arithmetic, 64 bits for command_id and 32 for every other column -- are ONE leaf, the
 *           one with the smaller span (`risk_level > 3`, `risk_level <= 3` and a negated `risk_level <= 3` share it).  A
 *           comparison that is the complement of its leaf becomes a step with on_true and on_false swapped.
 *   PROGRAM query[p] of the batch: the predicate's steps in evaluation order, step s = (leaf slot of the batch, on_true,
 *           on_false), targets as in pqps_predicate.
 *   COLUMNS the union of the queries' columns, ascending HIPCOL_* id: batch.column_ids[slot], -1 behind n_columns.
 *   CAPS    a query that would take the open batch over max_queries queries, PQPS_MAX_LEAVES distinct leaves or
 *           PQPS_MAX_COLUMNS columns closes it and opens the next.
 *   PLACE   place[i].batch >= 0: query i is query[place[i].position] of batches[place[i].batch];
 *           HIPCOUNT_CONSTANT: n_leaves == 0, the answer is every row (place[i].constant = 1) or none (0), no launch;
 *           HIPCOUNT_ALONE: more than PQPS_TT_LEAVES leaves, the caller runs it by the one-query COUNT.
 *   `batches` has room for n entries (at least 1); *n_batches = the batches made.
 * Returns 0, or -1 with the reason on stderr and every output untouched for: a NULL argument (queries may be NULL when n is
 * 0), n < 0, max_queries outside 1 .. PQPS_COUNT_MANY_MAX, a query without pred or column_ids, more than PQPS_MAX_LEAVES
 * leaves or PQPS_MAX_COLUMNS columns, a leaf whose column or a step whose leaf slot is out of range, leaves not sorted by
 * column, a column slot without an id, a predicate whose jump targets do not go forward. */
enum { HIPCOUNT_CONSTANT = -1, HIPCOUNT_ALONE = -2 };
struct hipCountQuery { const pqps_predicate *pred; const int *column_ids; };
struct hipCountBatch { pqps_count_many prog; int column_ids[PQPS_MAX_COLUMNS]; };
struct hipCountPlace { int batch, position, constant; };
int hipCountManyPack(const struct hipCountQuery *queries, int n, int max_queries, struct hipCountBatch *batches, int *n_batches,
                     struct hipCountPlace *place);

/* THE HOST HALF OF EXACT PERCENTILES (executeQueryQuantilesHIP): a radix select over the order-preserving key image of the
 * value column, one digit per counting scan (pqps_filter_digit_hist), most significant digit first.  Pure host code, integer
 * arithmetic only -- no floating point takes part in choosing a rank.
 *
 * hipQuantileRank: the 0-based rank, in the ascending sort of n values, of the fraction `ppm` parts per million (SQL's
 *   PERCENTILE_DISC): max(ceil(ppm * n / 1 000 000) - 1, 0).  ppm above 1 000 000 counts as 1 000 000; n = 0 gives 0.
 * hipQuantileDigitBits: the width of the next digit when `bits_left` of the key's `key_bits` are still open and the launch
 *   counts `tables` tables: a key of at most 11 bits is ONE pass; otherwise 11 bits while tables <= 8 (the tables fit LDS),
 *   else 8 bits (64 tables fit LDS; more live in global memory), never more than bits_left.  0 when nothing is left.
 * hipQuantilePick: one group after one pass.  tables[n_slots][2^digit_bits]: the group's counts, summed over the shards;
 *   prefixes[n_slots]: the prefix every slot stands for (NULL: one slot, prefix 0 -- the first pass); entry i < n_entries is a
 *   pending fraction: ranks[i] = its rank among the rows of table slots[i].  Per entry: digits[i] = the digit whose bucket
 *   holds the rank (the first d with ranks[i] < counts[0] + .. + counts[d]), ranks_in[i] = the rank inside that bucket.
 *   next_prefixes[0 .. *n_next): the distinct values of (prefix << digit_bits | digit) over the entries, ascending -- the
 *   next pass's slots; next_slots[i]: the one entry i follows.  Every output has room for n_entries.  Returns 0, or -1 with
 *   the reason on stderr for a NULL argument, digit_bits outside 1 .. 16, n_slots or n_entries above
 *   HIPQUANTILE_MAX_FRACTIONS, a slot out of range, a rank at or above its table's total. */
#define HIPQUANTILE_PPM 1000000ull
#define HIPQUANTILE_MAX_FRACTIONS 16
#define HIPQUANTILE_DIGIT_LDS 11u        /* = PQPS_DIGIT_BITS_MAX */
#define HIPQUANTILE_DIGIT_WIDE 8u
#define HIPQUANTILE_TABLES_LDS 8u
unsigned long long hipQuantileRank(unsigned long long n, unsigned int ppm);
unsigned int hipQuantileDigitBits(unsigned int bits_left, unsigned int key_bits, unsigned long long tables);
int hipQuantilePick(const uint64_t *tables, unsigned int digit_bits, const uint64_t *prefixes, int n_slots, const uint64_t *ranks,
                    const int *slots, int n_entries, unsigned int *digits, uint64_t *ranks_in, uint64_t *next_prefixes,
                    int *next_slots, int *n_next);

/* The number of values[0 .. count) (ascending in strcmp order) below `text`: its code when it is in the dictionary
 * (*present = 1), the rank it is inserted at otherwise (*present = 0). */
int hipDictionaryRank(const char *const *values, int count, const char *text, int *present);

/* Column name -> HIPCOL_* id, -1 if unknown. */
int hipColumnId(const char *name);

#ifdef __cplusplus
}
#endif
#endif /* HIP_PREDICATE_H */
