/* executeEngine-hip.c -- MI355X execute engine (see include/executeEngine-hip.h).
 *
 * Host orchestration in C11; every row predicate runs in the HIP filter
 * kernel behind include/pqps_hip.h.  There is no CPU evaluation path: if the
 * device or the shim is unavailable the engine prints the reason and exits.
 *
 * Reference being replaced: engine/serial/executeEngine-serial.c ("S"):
 *   executeQuerySelectSerial S:328-528, linearSearchRecords S:854-878,
 *   evaluateWhereClause S:292-316, executeQueryInsertSerial S:538-617,
 *   executeQueryDeleteSerial S:627-715, initialize/destroy S:727-814.
 */
#define _POSIX_C_SOURCE 200809L
#include "executeEngine-hip.h"
#include "buildEngine-hip.h"
#include "hipPredicate.h"

#include <limits.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include <unistd.h>

static double now_seconds(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* PQPS_TRACE=1: phase timings of every engine call on stderr. */
static int trace_on(void) {
    static int on = -1;
    if (on < 0) { const char *e = getenv("PQPS_TRACE"); on = e && atoi(e) != 0; }
    return on;
}
#define TRACE(...) do { if (trace_on()) fprintf(stderr, "[pqps] " __VA_ARGS__); } while (0)

/* A device call failed inside a query: the reason goes to stderr (like every diagnostic of the reference's
 * engines) and the query reports failure to its caller -- the process, and the engine, carry on. */
static int engine_error(const char *what) {
    fprintf(stderr, "HIP engine: %s: %s\n", what, pqps_last_error());
    return -1;
}

static int oom(void) {
    fprintf(stderr, "HIP engine: out of memory\n");
    return -1;
}

#define TRY(call, what) do { if ((call) != PQPS_OK) return engine_error(what); } while (0)

/* ---- predicate binding --------------------------------------------------------- */

/* The value sets of one engine (include/executeEngine-hip.h): what an IN SET node of a WHERE names.  The registry hangs off
 * the engine's table; `set[i].id` 0 is a free entry.  Sets are made by readers (several at once) and freed or made stale by
 * writers (alone): g_sets_lock guards the entries themselves, the table's locks keep a bitmap where a query in flight reads it. */
struct value_set {
    uint32_t id;
    int column, kind;                    /* B: HIPCOL_*, HIPKIND_DICT / HIPKIND_I32                                   */
    uint64_t version;                    /* the registry's when the set was made                                     */
    bool stale;                          /* a writer came after it: no device memory any more                        */
    uint32_t base;                       /* bit i of the bitmap: the code i, or the i32 value base + i               */
    int32_t lo;
    uint64_t n_bits, members, rows;
    uint32_t *bitmap[HIP_MAX_SHARDS];    /* one copy per shard, on its device                                        */
};
struct hipValueSets {
    uint64_t version;                    /* bumped by every successful writer                                        */
    uint32_t next_id;
    struct value_set set[HIP_MAX_VALUE_SETS];
};
static pthread_mutex_t g_sets_lock = PTHREAD_MUTEX_INITIALIZER;

/* (g_sets_lock held) the entry of set `id`, NULL if there is none */
static struct value_set *value_set_find(const struct hipTable *t, uint32_t id) {
    for (int i = 0; t->sets && id && i < HIP_MAX_VALUE_SETS; i++)
        if (t->sets->set[i].id == id) return &t->sets->set[i];
    return NULL;
}

/* What the WHERE compiler may know of the table's sets: infos[HIP_MAX_VALUE_SETS], the number filled in returned. */
static int value_set_infos(const struct hipTable *t, struct hipSetInfo *infos) {
    int n = 0;
    pthread_mutex_lock(&g_sets_lock);
    for (int i = 0; t->sets && i < HIP_MAX_VALUE_SETS; i++) {
        const struct value_set *vs = &t->sets->set[i];
        if (!vs->id) continue;
        infos[n++] = (struct hipSetInfo){ .id = vs->id, .column = vs->column, .kind = vs->kind, .base = vs->base, .n_bits = vs->n_bits,
                                          .members = vs->members, .stale = vs->stale };
    }
    pthread_mutex_unlock(&g_sets_lock);
    return n;
}

/* The bitmap of set `id` on shard s: the set's own buffer, which the caller does not own (NULL: no such set). */
static const uint32_t *value_set_bitmap(const struct hipTable *t, uint32_t id, int s) {
    pthread_mutex_lock(&g_sets_lock);
    const struct value_set *vs = value_set_find(t, id);
    const uint32_t *bitmap = vs && !vs->stale ? vs->bitmap[s] : NULL;
    pthread_mutex_unlock(&g_sets_lock);
    return bitmap;
}

/* (g_sets_lock held, no query in flight) gives back the device memory of a set */
static void value_set_release(struct hipTable *t, struct value_set *vs) {
    for (int s = 0; s < hipTableShards(t) && s < HIP_MAX_SHARDS; s++) {
        if (vs->bitmap[s]) pqps_free(hipTableShard(t, s)->ctx, vs->bitmap[s]);
        vs->bitmap[s] = NULL;
    }
}

/* A writer succeeded (the caller holds the table exclusively): the codes may have moved, every set is stale from now on. */
static void value_sets_invalidate(struct hipTable *t) {
    if (!t || !t->sets) return;
    pthread_mutex_lock(&g_sets_lock);
    t->sets->version++;
    for (int i = 0; i < HIP_MAX_VALUE_SETS; i++) {
        struct value_set *vs = &t->sets->set[i];
        if (!vs->id || vs->stale) continue;
        vs->stale = true;
        value_set_release(t, vs);
    }
    pthread_mutex_unlock(&g_sets_lock);
}

/* destroyEngineHIP: whatever is left, before the contexts go */
static void value_sets_destroy(struct hipTable *t) {
    if (!t || !t->sets) return;
    pthread_mutex_lock(&g_sets_lock);
    for (int i = 0; i < HIP_MAX_VALUE_SETS; i++) if (t->sets->set[i].id) value_set_release(t, &t->sets->set[i]);
    free(t->sets);
    t->sets = NULL;
    pthread_mutex_unlock(&g_sets_lock);
}

/* The compiled WHERE of one query: usually one pass; see hipCompileWherePlan.  An IN SET node names a set of the table. */
static int bind_where(const struct hipTable *t, const struct whereClauseS *where, struct hipPlan *plan) {
    struct hipSchema schema;
    struct hipSetInfo infos[HIP_MAX_VALUE_SETS];
    char err[160];
    hipSchemaOfTable(t, &schema);
    if (hipCompileWherePlanSets(&schema, where, infos, value_set_infos(t, infos), plan, err, sizeof err) != 0) {
        fprintf(stderr, "HIP engine: cannot compile WHERE clause: %s\n", err);
        return -1;
    }
    return 0;
}

/* One shard's side of a plan: the flag buffers of the passes before the last, and the last pass's columns. */
struct shard_pred {
    const pqps_predicate *pred;
    pqps_column cols[PQPS_MAX_COLUMNS];
    uint32_t n_cols;
    uint8_t **flags;                 /* n_passes - 1 device buffers (NULL for a single pass) */
    void **member;                   /* ... and the bitmap or list of each member pass among them, on the device */
    bool *plane;                     /* ... flags[k] is a bit plane (a member pass all of whose readers are scans) */
    int n_flags;
};

static void shard_pred_free(struct hipTable *sh, struct shard_pred *sp) {
    for (int k = 0; k < sp->n_flags; k++) {
        if (sp->flags[k]) pqps_free(sh->ctx, sp->flags[k]);
        if (sp->member[k]) pqps_free(sh->ctx, sp->member[k]);
    }
    free(sp->flags);
    free(sp->member);
    free(sp->plane);
    sp->flags = NULL;
    sp->member = NULL;
    sp->plane = NULL;
    sp->n_flags = 0;
}

/* Where a scan reads a 0 / 1 column from a bit plane: the plane is the pass's last column (the width-specialised kernels'
 * shapes: widths non-increasing, the plane last) or the pass takes the generic kernel anyway (more than 3 columns or more
 * than 6 comparisons).  A lone bool column keeps its bytes: its scan time is all output, not input. */
static bool plane_slot(const struct hipPass *pass, uint32_t i) {
    const uint32_t n = pass->pred.n_columns;
    const bool generic = n > 3 || pass->pred.n_leaves > PQPS_TT_LEAVES;
    return n > 1 && (i == n - 1 || generic);
}

/* PQPS_PACK12=0 (read once): no scan reads a 12-bit packed copy (A/B runs, tests). */
static bool packed12_enabled(void) {
    static int on = -1;
    if (on < 0) { const char *e = getenv("PQPS_PACK12"); on = !e || atoi(e) != 0; }
    return on != 0;
}

/* `scan`: the columns go to a scan (pqps_filter_scan / _count / _flags, query stream, exchange, the fused scans), which
 * reads sudo_used from its bit plane where plane_slot allows.  Index-mode gathers always get the byte column.  `plain`:
 * the scan is an ID, COUNT or flag scan -- those read a u16 dictionary column from its 12-bit packed copy where the pass
 * is that column alone, or that column and the plane of sudo_used, with at most 6 comparisons: the two shapes the
 * specialised kernels have for a copy.  `sp`: the shard's flag buffers (NULL for a plan of one pass); the flags of a
 * member pass are a plane where head_pass wrote one. */
static void pass_columns(const struct hipTable *sh, const struct hipPass *pass, const struct shard_pred *sp, bool scan, bool plain, pqps_column *cols) {
    const uint32_t n = pass->pred.n_columns;
    for (uint32_t i = 0; i < n; i++) {
        const int id = pass->column_ids[i];
        if (id >= PQPS_MAX_COLUMNS) {
            cols[i].data = sp->flags[id - PQPS_MAX_COLUMNS];
            cols[i].width = sp->plane[id - PQPS_MAX_COLUMNS] ? PQPS_WIDTH_BITS : 1;
            cols[i].reserved = 0;
        }
        else if (scan && id == HIPCOL_SUDO_USED && sh->sudo_bits.data && plane_slot(pass, i)) cols[i] = sh->sudo_bits;
        else cols[i] = sh->col[id];
    }
    /* (n < 1 first: a pass without columns -- no WHERE -- has filled in nothing of `cols`, which may be the caller's bare stack array) */
    if (!scan || !plain || n < 1 || n > 2 || pass->pred.n_leaves < 1 || pass->pred.n_leaves > PQPS_TT_LEAVES || !packed12_enabled()) return;
    const int first = pass->column_ids[0];
    if (first >= PQPS_MAX_COLUMNS || !sh->packed12[first].data || cols[0].width != 2) return;
    if (n == 2 && !(pass->column_ids[1] == HIPCOL_SUDO_USED && cols[1].width == PQPS_WIDTH_BITS)) return;
    cols[0] = sh->packed12[first];
}

/* A member pass writes a plane when every reader of its flag column is a scan that takes a plane in that slot
 * (`scan_last`: the plan's last pass is a scan, not index-mode gathers). */
static bool member_writes_plane(const struct hipPlan *plan, int k, bool scan_last) {
    bool read = false;
    for (int j = k + 1; j < plan->n_passes; j++) {
        const struct hipPass *p = &plan->pass[j];
        for (uint32_t i = 0; !p->member && i < p->pred.n_columns; i++) {
            if (p->column_ids[i] != PQPS_MAX_COLUMNS + k) continue;
            if (!(j < plan->n_passes - 1 || scan_last) || !plane_slot(p, i)) return false;
            read = true;
        }
    }
    return read;
}

/* The passes in front of the last on one shard, on (ctx, stream): each leaves one flag per row -- a filter pass through
 * pqps_filter_flags, a member pass (a LIKE / IN set as a bitmap or list, uploaded here, owned by `sp`; or the bitmap of a
 * value set of table `t`, which stays the set's) through pqps_member_flags on shard s.  `count_dev`: a device word for the counts nobody reads. */
static int head_passes(const struct hipPlan *plan, const struct hipTable *t, int s, struct shard_pred *sp, pqps_ctx *ctx, void *stream,
                       uint64_t *count_dev, bool scan_last) {
    struct hipTable *sh = hipTableShard((struct hipTable *)t, s);
    if (plan->n_passes < 2) return 0;
    const size_t n = (size_t)plan->n_passes - 1;
    sp->flags = calloc(n, sizeof *sp->flags);
    sp->member = calloc(n, sizeof *sp->member);
    sp->plane = calloc(n, sizeof *sp->plane);
    if (!sp->flags || !sp->member || !sp->plane) {
        free(sp->flags); free(sp->member); free(sp->plane);
        sp->flags = NULL; sp->member = NULL; sp->plane = NULL;
        return oom();
    }
    sp->n_flags = (int)n;
    for (int k = 0; k < sp->n_flags; k++) {
        const struct hipPass *pass = &plan->pass[k];
        TRY(pqps_malloc(sh->ctx, sh->capacity_rows, (void **)&sp->flags[k]), "flag allocation");
        if (!pass->member) {
            pqps_column cols[PQPS_MAX_COLUMNS];
            pass_columns(sh, pass, sp, true, true, cols);
            TRY(pqps_filter_flags(ctx, cols, pass->pred.n_columns, sh->n_rows, &pass->pred, sp->flags[k], count_dev, stream), "flag filter");
            continue;
        }
        const bool bitmap = pass->member_form == PQPS_MEMBER_BITMAP;
        const void *host = bitmap ? (const void *)pass->member_bitmap : (const void *)pass->member_list;
        const size_t bytes = bitmap ? (size_t)((pass->member_bits + 31) / 32) * sizeof(uint32_t) : (size_t)pass->member_count * sizeof(uint64_t);
        const void *set = NULL;
        if (pass->member_set) {
            /* a value set: its bitmap is on this device already, where the build left it, and stays the set's */
            set = value_set_bitmap(t, pass->member_set, s);
            if (!set) { fprintf(stderr, "HIP engine: value set %u has no bitmap on shard %d\n", pass->member_set, s); return -1; }
        } else if (bytes) {
            TRY(pqps_malloc(sh->ctx, bytes, &sp->member[k]), "member set allocation");
            TRY(pqps_upload(ctx, sp->member[k], host, bytes, stream), "member set upload");
            set = sp->member[k];
        }
        sp->plane[k] = member_writes_plane(plan, k, scan_last);
        TRY(pqps_member_flags(ctx, &sh->col[pass->member_column], sh->n_rows, pass->member_form, pass->member_base, pass->member_bits,
                              bitmap ? set : NULL, bitmap ? NULL : set, pass->member_count,
                              sp->plane[k] ? PQPS_MEMBER_PLANE : PQPS_MEMBER_BYTES, sp->flags[k], count_dev, stream), "member flags");
    }
    return 0;
}

/* Inclusive key window of an indexed top-level condition, S:377-424.
 * v + 1 / v - 1 wrap the way the reference's machine arithmetic does. */
static void key_window_u64(const char *op, const char *value, uint64_t *lo, uint64_t *hi) {
    const uint64_t v = strtoull(value, NULL, 10);
    *lo = 0; *hi = UINT64_MAX;
    if (strcmp(op, "=") == 0) { *lo = v; *hi = v; }
    else if (strcmp(op, ">") == 0) *lo = v + 1;
    else if (strcmp(op, ">=") == 0) *lo = v;
    else if (strcmp(op, "<") == 0) *hi = v - 1;
    else if (strcmp(op, "<=") == 0) *hi = v;
}

static void key_window_i32(const char *op, const char *value, uint64_t *lo, uint64_t *hi) {
    const int v = atoi(value);
    int l = INT_MIN, h = INT_MAX;
    if (strcmp(op, "=") == 0) { l = v; h = v; }
    else if (strcmp(op, ">") == 0) l = (int)((unsigned)v + 1u);
    else if (strcmp(op, ">=") == 0) l = v;
    else if (strcmp(op, "<") == 0) h = (int)((unsigned)v - 1u);
    else if (strcmp(op, "<=") == 0) h = v;
    *lo = (uint64_t)(uint32_t)l;
    *hi = (uint64_t)(uint32_t)h;
}

/* The keys a condition on a BOOL index admits in the OpenMP / MPI engines (omp:424-459): = / != one key, the ordered
 * operators what they admit; `> true` and `< false` admit none (lo > hi: the probe finds nothing, but it counts as a
 * probe -- the query stays in index mode and comes back empty). */
static void key_window_bool(const char *op, const char *value, uint64_t *lo, uint64_t *hi) {
    const int val = (strcasecmp(value, "true") == 0 || strcmp(value, "1") == 0) ? 1 : 0;
    int l = 0, h = 1;
    if (strcmp(op, "=") == 0) { l = val; h = val; }
    else if (strcmp(op, "!=") == 0) { l = !val; h = !val; }
    else if (strcmp(op, ">") == 0) { l = 1; h = val ? 0 : 1; }
    else if (strcmp(op, ">=") == 0) { l = val; h = 1; }
    else if (strcmp(op, "<") == 0) { l = val ? 0 : 1; h = 0; }
    else if (strcmp(op, "<=") == 0) { l = 0; h = val; }
    *lo = (uint64_t)l;
    *hi = (uint64_t)h;
}

/* One index probe the serial engine would make for this WHERE (S:358-433), in its order (with probe_bool: the
 * OpenMP / MPI engines' one-thread order, omp:362-494 -- the same walk with BOOL indexes included). */
struct probe { int index; uint64_t lo, hi; };

static int list_probes(struct engineS *engine, const struct hipTable *t, struct whereClauseS *where, struct probe **out) {
    int n = 0, cap = 0;
    struct probe *pr = NULL;
    for (struct whereClauseS *wc = where; wc; wc = wc->next) {
        if (wc->attribute == NULL) continue;                           /* nested node, S:361-364 */
        if (hipIsSetOperator(wc->operator)) continue;                  /* LIKE / IN: never a probe, part of the re-filter */
        for (int i = 0; i < engine->num_indexes; i++) {
            if (strcmp(wc->attribute, engine->indexed_attributes[i]) != 0) continue;
            const struct hipIndex *ix = &t->index[i];
            if (ix->column < 0 || wc->operator == NULL || wc->value == NULL) continue;
            uint64_t lo, hi;
            /* only u64 / int indexes are probed by the serial engine, S:377-433 */
            if (engine->attribute_types[i] == FIELD_UINT64 && t->col[ix->column].width == 8 && ix->key_kind == 0)
                key_window_u64(wc->operator, wc->value, &lo, &hi);
            else if (engine->attribute_types[i] == FIELD_INT && ix->key_kind == 1)
                key_window_i32(wc->operator, wc->value, &lo, &hi);
            else if (t->probe_bool && engine->attribute_types[i] == FIELD_BOOL && t->col[ix->column].width == 1 && ix->key_kind == 0)
                key_window_bool(wc->operator, wc->value, &lo, &hi);
            else
                continue;
            if (n == cap) {
                cap = cap ? 2 * cap : 8;
                struct probe *grown = realloc(pr, (size_t)cap * sizeof *grown);
                if (!grown) { free(pr); return -1; }
                pr = grown;
            }
            pr[n++] = (struct probe){ i, lo, hi };
        }
    }
    *out = pr;
    return n;
}

/* ---- one query on the device(s) -------------------------------------------------------------------------
 * Row selection of executeQuerySelectSerial, S:358-474.  A query is ISSUED -- everything it needs is enqueued on
 * every shard, nothing is waited for -- and later AWAITED.  Engine tables give it a lane: result buffers of its own
 * on every shard and a slot of the shards' query streams (so several queries are on the device at once); a table
 * without lanes (ad-hoc tables over caller-supplied rows) runs it on the table's own context and buffers.
 *
 * Result.  Scan mode: shard s holds count[s] ascending engine row numbers; the answer is their concatenation in
 * shard order.  Index mode: per probe, each shard appended its rows in (key asc, row desc) order; several shards
 * are merged by key on shard 0's device.  `ids_dev` = the whole answer on shard 0's device (one shard: its lane's
 * buffer as it stands; several: the gathered list). */
struct query {
    struct engineS *engine;
    struct hipTable *t;
    int lane;                            /* -1: the table's own buffers */
    int n_shards;
    bool count_only;
    struct hipPlan plan;
    bool have_plan;
    struct probe *probes;
    int n_probes;
    struct shard_pred sp[HIP_MAX_SHARDS];
    uint64_t *seg_dev[HIP_MAX_SHARDS];   /* index mode, several shards: running count after each probe */
    /* after await */
    uint64_t total;
    uint64_t count[HIP_MAX_SHARDS];
    const uint32_t *ids_dev;
    pqps_ctx *ids_ctx;                   /* a context of the device ids_dev lives on (downloads) */
    bool exchanged;                      /* issued through the ranks' exchange: the answer is the exchange slot's */
    bool per_shard;                      /* several shards: leave each shard's list on its device (grouped COUNT) */
    bool keep_lists, listed;             /* a query that makes several shard_reduces over ONE selection (the percentiles'
                                            passes) sets keep_lists; listed: query_lists() has run, the lists stand   */
};

static struct hipLane *query_lane(const struct query *q, int s) {
    struct hipTable *sh = hipTableShard(q->t, s);
    return q->lane >= 0 ? &sh->lane[q->lane] : &sh->own;
}

/* context for the lane's own copies / gathers (never the stream the scans run on) */
static pqps_ctx *lane_copy_ctx(const struct query *q, int s) {
    struct hipLane *L = query_lane(q, s);
    return L->copy ? L->copy : hipTableShard(q->t, s)->ctx;
}

static void query_init(struct query *q, struct engineS *engine, struct hipTable *t, int lane, bool count_only) {
    memset(q, 0, sizeof *q);
    q->engine = engine;
    q->t = t;
    q->lane = lane;
    q->n_shards = hipTableShards(t);
    q->count_only = count_only;
}

static void query_free(struct query *q) {
    for (int s = 0; s < q->n_shards; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        shard_pred_free(sh, &q->sp[s]);
        if (q->seg_dev[s]) { pqps_free(sh->ctx, q->seg_dev[s]); q->seg_dev[s] = NULL; }
    }
    free(q->probes);
    q->probes = NULL;
    if (q->have_plan) { hipPlanFree(&q->plan); q->have_plan = false; }
}

/* The filter calls of the query on shard s, on (ctx, stream): flag passes, then the count, the probes + gather
 * filters, or the scan. */
static int issue_calls(struct query *q, int s, pqps_ctx *ctx, void *stream) {
    struct hipTable *sh = hipTableShard(q->t, s);
    struct hipLane *L = query_lane(q, s);
    struct shard_pred *sp = &q->sp[s];
    const struct hipPlan *plan = &q->plan;
    const struct hipPass *last = &plan->pass[plan->n_passes - 1];
    /* the passes before the last: one flag per row each */
    const bool scan_last = q->count_only || q->n_probes == 0;
    if (head_passes(plan, q->t, s, sp, ctx, stream, L->count_dev + 4, scan_last) != 0) return -1;
    sp->pred = &last->pred;
    sp->n_cols = last->pred.n_columns;
    pass_columns(sh, last, sp, scan_last, true, sp->cols);
    if (q->count_only) {
        TRY(pqps_filter_count(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, L->count_dev, stream), "count filter");
    } else if (q->n_probes > 0) {
        TRY(pqps_memset(ctx, L->count_dev, 0, sizeof(uint64_t), stream), "counter reset");
        if (q->n_shards > 1 && !q->seg_dev[s]) TRY(pqps_malloc(sh->ctx, (size_t)q->n_probes * sizeof(uint64_t), (void **)&q->seg_dev[s]), "segment counters");
        for (int k = 0; k < q->n_probes; k++) {
            const struct hipIndex *ix = &sh->index[q->probes[k].index];
            uint64_t *range_dev = L->count_dev + 2;
            /* the probe, then its rows that pass the complete WHERE appended, leaf order kept (S:441-448 + S:471) -- copied
             * when the WHERE is the probed comparison itself (the shim looks at the compiled predicate) */
            TRY(pqps_index_select(ctx, sp->cols, sp->n_cols, &sh->col[ix->column], ix->perm_dev, ix->keys_dev, ix->key_kind, sh->n_rows,
                                  q->probes[k].lo, q->probes[k].hi, (uint32_t)sh->row0, sp->pred, range_dev,
                                  L->ids_dev, L->capacity_ids, L->count_dev, stream), "index probe + filter");
            if (q->seg_dev[s])                                     /* where this probe's rows end on this shard */
                TRY(pqps_copy_peer(ctx, q->seg_dev[s] + k, ctx, L->count_dev, sizeof(uint64_t), stream), "segment counter");
        }
    } else {
        TRY(pqps_filter_scan(ctx, sp->cols, sp->n_cols, sh->n_rows, (uint32_t)sh->row0, sp->pred, L->ids_dev, L->capacity_ids,
                             L->count_dev, stream), "scan filter");
    }
    return 0;
}

/* Everything of the query that runs on shard s.  A single-pass scan or count on a lane is ONE call into the shard's
 * query stream, whose completion event rides on the launch itself. */
static int issue_on_shard(struct query *q, int s) {
    struct hipTable *sh = hipTableShard(q->t, s);
    struct hipLane *L = query_lane(q, s);
    struct shard_pred *sp = &q->sp[s];
    memset(sp, 0, sizeof *sp);
    const struct hipPlan *plan = &q->plan;
    const struct hipPass *last = &plan->pass[plan->n_passes - 1];
    const bool single = plan->n_passes == 1 && q->n_probes == 0;
    if (q->t->xch) {
        /* one process per GPU: the shard's scan + the exchange with the other ranks, one call (mpi:717-768).  Every rank has
         * to issue the same queries in the same order; index probes and WHERE lists of several passes stay local matters */
        if (!single || q->lane < 0) {
            fprintf(stderr, "HIP engine: across ranks only scan-mode queries of one pass are exchanged (no index probes, at most %d comparisons)\n", PQPS_MAX_LEAVES);
            return -1;
        }
        sp->pred = &last->pred;
        sp->n_cols = last->pred.n_columns;
        pass_columns(sh, last, NULL, true, true, sp->cols);
        if (q->count_only)
            TRY(pqps_exchange_count(q->t->xch, sp->cols, sp->n_cols, sh->n_rows, sp->pred, (uint32_t)q->lane, NULL), "count exchange");
        else
            TRY(pqps_exchange_select(q->t->xch, sp->cols, sp->n_cols, sh->n_rows, (uint32_t)sh->row0, sp->pred, (uint32_t)q->lane, NULL), "scan exchange");
        q->exchanged = true;
        return 0;
    }
    if (q->lane >= 0 && single) {
        sp->pred = &last->pred;
        sp->n_cols = last->pred.n_columns;
        pass_columns(sh, last, NULL, true, true, sp->cols);
        if (q->count_only)
            TRY(pqps_qstream_count_slot(sh->qs, (uint32_t)q->lane, sp->cols, sp->n_cols, sh->n_rows, sp->pred, L->count_dev, NULL), "count filter");
        else
            TRY(pqps_qstream_scan_slot(sh->qs, (uint32_t)q->lane, sp->cols, sp->n_cols, sh->n_rows, (uint32_t)sh->row0, sp->pred,
                                       L->ids_dev, L->capacity_ids, L->count_dev, NULL), "scan filter");
        return 0;
    }
    pqps_ctx *ctx = sh->ctx;
    void *stream = NULL;
    if (q->lane >= 0) TRY(pqps_qstream_lane(sh->qs, (uint32_t)q->lane, sh->n_rows, NULL, &ctx, &stream), "query lane");
    const int rc = issue_calls(q, s, ctx, stream);
    /* the end of whatever reached the lane's stream is marked even if a call failed half-way: the lane's buffers must
     * not be handed to another query while a launch of this one still runs */
    if (q->lane >= 0 && pqps_qstream_mark(sh->qs, (uint32_t)q->lane) != PQPS_OK && rc == 0) return engine_error("query lane");
    return rc;
}

static int query_issue_all(struct query *q) {
    int rc = 0;
    hipTableLockIssue(q->t);
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        shard_pred_free(hipTableShard(q->t, s), &q->sp[s]);            /* (a re-issue after a result buffer had to grow) */
        rc = issue_on_shard(q, s);
    }
    hipTableUnlockIssue(q->t);
    return rc;
}

/* Compiles the WHERE, lists the probes, enqueues the query on every shard. */
static int query_issue(struct query *q, struct whereClauseS *where) {
    if (bind_where(q->t, where, &q->plan) != 0) return -1;
    q->have_plan = true;
    if (!q->count_only) {
        q->n_probes = list_probes(q->engine, q->t, where, &q->probes);     /* COUNT(*) is the scan-mode count */
        if (q->n_probes < 0) { q->n_probes = 0; return -1; }
    }
    return query_issue_all(q);
}

static int wait_shard(struct query *q, int s) {
    struct hipTable *sh = hipTableShard(q->t, s);
    if (q->exchanged || (q->t->xch && q->lane >= 0)) return 0;      /* (the exchange's own slot waits cover it) */
    if (q->lane >= 0) TRY(pqps_qstream_wait(sh->qs, (uint32_t)q->lane), "filter execution");
    else TRY(pqps_ctx_sync(sh->ctx, NULL), "filter execution");
    return 0;
}

static int grow_lane_ids(struct hipTable *sh, struct hipLane *L, uint64_t need) {
    if (need <= L->capacity_ids) return 0;
    pqps_free(sh->ctx, L->ids_dev);
    L->ids_dev = NULL;
    L->capacity_ids = 0;
    const uint64_t cap = need + need / 8 + 1024;
    TRY(pqps_malloc(sh->ctx, cap * sizeof(uint32_t), (void **)&L->ids_dev), "result allocation");
    L->capacity_ids = cap;
    return 0;
}

/* Several shards: the answer in one piece on shard 0's device.  Scan mode = the concatenation of the shards' lists in
 * shard order, placed by peer copies at the displacements the counts give (MPI_Allgather of the sizes, exclusive prefix,
 * MPI_Allgatherv: mpi:753-765).  Index mode = per probe the union of the shards' segments sorted by (key asc, row
 * desc) -- every segment is in that order already and a later shard holds later rows, so this is the table-wide
 * leaf order of the reference's tree: keys gathered on each shard, segments and keys copied over, merged by the
 * device sort behind pqps_merge_index_slots. */
static int gather_shards(struct query *q) {
    struct hipTable *t = q->t;
    struct hipLane *L0 = query_lane(q, 0);
    pqps_ctx *c0 = lane_copy_ctx(q, 0);
    if (q->total > L0->merged_cap) {
        if (L0->merged_dev) pqps_free(t->ctx, L0->merged_dev);
        L0->merged_dev = NULL;
        L0->merged_cap = 0;
        const uint64_t cap = q->total + q->total / 8 + 1024;
        TRY(pqps_malloc(t->ctx, cap * sizeof(uint32_t), (void **)&L0->merged_dev), "gathered list allocation");
        L0->merged_cap = cap;
    }
    q->ids_dev = L0->merged_dev;
    q->ids_ctx = c0;
    if (q->total == 0) return 0;
    if (q->n_probes == 0) {
        uint64_t at = 0;
        for (int s = 0; s < q->n_shards; s++) {
            TRY(pqps_copy_peer(c0, L0->merged_dev + at, lane_copy_ctx(q, s), query_lane(q, s)->ids_dev, q->count[s] * sizeof(uint32_t), NULL), "peer copy");
            at += q->count[s];
        }
        TRY(pqps_ctx_sync(c0, NULL), "peer copy");
        return 0;
    }
    /* index mode */
    uint64_t *ends = malloc((size_t)q->n_probes * (size_t)q->n_shards * sizeof *ends);       /* [shard][probe] */
    if (!ends) return -1;
    int rc = 0;
#define RUN(call, what) do { if (rc == 0 && (call) != PQPS_OK) rc = engine_error(what); } while (0)
    for (int s = 0; s < q->n_shards; s++)
        RUN(pqps_download(lane_copy_ctx(q, s), ends + (size_t)s * (size_t)q->n_probes, q->seg_dev[s], (size_t)q->n_probes * sizeof *ends, NULL), "segment counters");
    uint64_t out_at = 0;
    for (int k = 0; k < q->n_probes && rc == 0; k++) {
        uint64_t seg_total = 0, seg_len[HIP_MAX_SHARDS], seg_begin[HIP_MAX_SHARDS];
        for (int s = 0; s < q->n_shards; s++) {
            const uint64_t *e = ends + (size_t)s * (size_t)q->n_probes;
            seg_begin[s] = k ? e[k - 1] : 0;
            seg_len[s] = e[k] - seg_begin[s];
            seg_total += seg_len[s];
        }
        if (seg_total == 0) continue;
        const uint64_t stride = ((seg_total + 1) & ~1ull) + PQPS_SLOT_HEADER_WORDS;
        uint32_t *slots = NULL;
        uint64_t *keys = NULL, *totals_dev = NULL;
        RUN(pqps_malloc(t->ctx, stride * sizeof(uint32_t), (void **)&slots), "merge buffer");
        RUN(pqps_malloc(t->ctx, (stride - PQPS_SLOT_HEADER_WORDS) * sizeof(uint64_t), (void **)&keys), "merge buffer");
        RUN(pqps_malloc(t->ctx, 2 * sizeof(uint64_t), (void **)&totals_dev), "merge buffer");
        const uint64_t header[2] = { seg_total, 0 };
        RUN(pqps_upload(c0, slots, header, sizeof header, NULL), "merge header");
        uint64_t at = 0;
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            if (seg_len[s] == 0) continue;
            struct hipTable *sh = hipTableShard(t, s);
            struct hipLane *L = query_lane(q, s);
            pqps_ctx *cs = lane_copy_ctx(q, s);
            const struct hipIndex *ix = &sh->index[q->probes[k].index];
            uint64_t *keys_s = NULL;
            RUN(pqps_malloc(sh->ctx, seg_len[s] * sizeof(uint64_t), (void **)&keys_s), "key buffer");
            /* (the count word on the device is the shard's total >= the segment's length: the capacity argument bounds the gather) */
            RUN(pqps_gather_keys(cs, &sh->col[ix->column], ix->key_kind, L->ids_dev + seg_begin[s], L->count_dev, seg_len[s], (uint32_t)sh->row0, keys_s, NULL), "key gather");
            RUN(pqps_ctx_sync(cs, NULL), "key gather");
            RUN(pqps_copy_peer(c0, slots + PQPS_SLOT_HEADER_WORDS + at, cs, L->ids_dev + seg_begin[s], seg_len[s] * sizeof(uint32_t), NULL), "peer copy");
            RUN(pqps_copy_peer(c0, keys + at, cs, keys_s, seg_len[s] * sizeof(uint64_t), NULL), "peer copy");
            RUN(pqps_ctx_sync(c0, NULL), "peer copy");
            if (keys_s) pqps_free(sh->ctx, keys_s);
            at += seg_len[s];
        }
        RUN(pqps_merge_index_slots(c0, slots, keys, 1, stride, L0->merged_dev + out_at, L0->merged_cap - out_at, totals_dev, NULL), "index merge");
        out_at += seg_total;
        if (slots) pqps_free(t->ctx, slots);
        if (keys) pqps_free(t->ctx, keys);
        if (totals_dev) pqps_free(t->ctx, totals_dev);
    }
#undef RUN
    free(ends);
    return rc;
}

/* Waits for the query; a result buffer that turned out too small (index-mode duplicates can exceed the table's rows)
 * is grown and the query issued again. */
static int query_await(struct query *q) {
    if (q->exchanged) {
        /* every rank holds the whole answer: the shards' lists gathered in rank order (= ascending row numbers) */
        const uint32_t *merged = NULL;
        uint64_t local = 0, totals[2] = { 0, 0 };
        TRY(pqps_exchange_result(q->t->xch, (uint32_t)q->lane, q->count_only ? NULL : &merged, &local, totals), "exchange result");
        q->total = totals[0];
        q->count[0] = local;
        q->ids_dev = merged;
        q->ids_ctx = lane_copy_ctx(q, 0);
        return 0;
    }
    for (;;) {
        bool again = false;
        int rc = 0;
        q->total = 0;
        for (int s = 0; s < q->n_shards; s++) {
            struct hipTable *sh = hipTableShard(q->t, s);
            struct hipLane *L = query_lane(q, s);
            if (rc == 0) rc = wait_shard(q, s);
            if (rc == 0 && L->count_host) q->count[s] = L->count_host[0];         /* written by the launch itself, on the host with its completion event */
            else if (rc == 0 && pqps_download(lane_copy_ctx(q, s), &q->count[s], L->count_dev, sizeof(uint64_t), NULL) != PQPS_OK) rc = engine_error("count download");
            if (rc == 0 && !q->count_only && q->count[s] > L->capacity_ids) {
                rc = grow_lane_ids(sh, L, q->count[s]);
                again = true;
            }
            q->total += q->count[s];
            if (rc == 0 && !q->count_only && q->n_probes == 0 && q->lane >= 0 && sh->qs) pqps_qstream_hint_answer(sh->qs, q->count[s], sh->n_rows);
        }
        if (rc != 0) return rc;
        if (!again) break;
        if (query_issue_all(q) != 0) return -1;
    }
    if (q->count_only) return 0;
    if (q->n_shards == 1 || q->per_shard) {
        q->ids_dev = query_lane(q, 0)->ids_dev;
        q->ids_ctx = lane_copy_ctx(q, 0);
        return 0;
    }
    return gather_shards(q);
}

/* ---- asynchronous tickets (include/executeEngine-hip.h) ------------------------------------------------ */

struct hipQueryTicket {
    struct query q;
    double t0;
    int state;                       /* 0 issued, 1 awaited, -1 failed */
};

static struct hipQueryTicket *ticket_begin(struct engineS *engine, struct whereClauseS *where, bool count_only) {
    if (!engine || !engine->record_block) return NULL;
    struct hipTable *t = engine->record_block;
    struct hipQueryTicket *tk = calloc(1, sizeof *tk);
    if (!tk) { oom(); return NULL; }
    tk->t0 = now_seconds();
    hipTableLockShared(t);                                            /* until releaseQueryHIP: no writer meanwhile */
    const int lane = hipTableAcquireLane(t);
    if (lane == HIP_LANE_REFUSED) {                                   /* reason on stderr: the caller holds every lane itself, or none came free in time */
        hipTableUnlockShared(t);
        free(tk);
        return NULL;
    }
    query_init(&tk->q, engine, t, lane, count_only);
    if (query_issue(&tk->q, where) != 0) tk->state = -1;            /* reason on stderr; awaitQueryHIP reports -1 */
    return tk;
}

struct hipQueryTicket *executeQuerySelectAsyncHIP(struct engineS *engine, struct whereClauseS *whereClause) {
    return ticket_begin(engine, whereClause, false);
}

struct hipQueryTicket *executeQueryCountAsyncHIP(struct engineS *engine, struct whereClauseS *whereClause) {
    return ticket_begin(engine, whereClause, true);
}

long long awaitQueryHIP(struct hipQueryTicket *tk, struct hipDeviceResult *result) {
    if (result) memset(result, 0, sizeof *result);
    if (!tk) return -1;
    if (tk->state == 0) tk->state = query_await(&tk->q) == 0 ? 1 : -1;
    if (tk->state < 0) { if (result) result->count = -1; return -1; }
    if (result) {
        result->count = (long long)tk->q.total;
        result->ids_dev = tk->q.count_only ? NULL : tk->q.ids_dev;
        result->device = pqps_ctx_device(tk->q.t->ctx);
        result->n_shards = tk->q.n_shards;
        for (int s = 0; s < tk->q.n_shards && s < 16; s++) result->shard_count[s] = tk->q.count[s];
    }
    return (long long)tk->q.total;
}

/* Checksums of the answer's ID list where it lies, on the device (pqps_ids_checksum): what a driver compares the list of
 * a timed query with -- against another path's list, or against numpy over the oracle's -- without moving it. */
int hipQueryChecksumHIP(struct hipQueryTicket *tk, unsigned long long out[2]) {
    if (!tk || !out) return -1;
    const long long count = awaitQueryHIP(tk, NULL);
    if (count < 0 || tk->q.count_only) return -1;
    uint64_t sums[2] = { 0, 0 };
    if (count > 0 && pqps_ids_checksum(tk->q.ids_ctx, tk->q.ids_dev, (uint64_t)count, sums, NULL) != PQPS_OK) return engine_error("ID checksum");
    out[0] = sums[0];
    out[1] = sums[1];
    return 0;
}

/* ---- one process per GPU ----------------------------------------------------------------------------------- */
static struct engineS *engine_shell(unsigned long long num_rows, const char *tableName);
static void probe_mode_from_env(struct engineS *engine);

struct engineS *initializeEngineSyntheticRankHIP(unsigned long long rows_total, unsigned long long seed, int world, int rank,
                                                 const char *tableName) {
    if (world < 1 || rank < 0 || rank >= world) { fprintf(stderr, "HIP engine: rank %d of %d\n", rank, world); return NULL; }
    if (rows_total > 0xFFFFFFFFull) { fprintf(stderr, "HIP engine: row numbers are 32 bits wide: %llu rows\n", rows_total); return NULL; }
    uint64_t start = 0, count = 0;
    pqps_partition(rows_total, world, rank, &start, &count);       /* mpi:703-715 */
    struct engineS *engine = engine_shell(count, tableName);
    if (!engine) return NULL;
    /* six lanes: the exchange holds the payload of two queries back behind the scans in flight (pqps_exchange_select) */
    buildSyntheticShardDeviceTableHIP(engine, count, seed, start, 6);
    struct hipTable *t = engine->record_block;
    t->world = world;
    t->rank = rank;
    t->rows_total = rows_total;
    probe_mode_from_env(engine);
    return engine;
}

int hipEngineRcclIdHIP(const char *rccl_library, void *id128) {
    if (!id128) return -1;
    if (pqps_exchange_unique_id(rccl_library, (pqps_rccl_id *)id128) != PQPS_OK) return engine_error("RCCL id");
    return 0;
}

int hipEngineJoinPrepareHIP(struct engineS *engine, const char *rccl_library) {
    if (!engine || !engine->record_block) return -1;
    struct hipTable *t = engine->record_block;
    if (t->world < 1 || hipTableShards(t) != 1 || t->xch) { fprintf(stderr, "HIP engine: not a rank's engine, or joined already\n"); return -1; }
    if (hipTableLockExclusive(t) != 0) return -1;
    const int rc = pqps_exchange_prepare(t->ctx, rccl_library, (uint32_t)t->world, (uint32_t)t->rank, t->capacity_rows, (uint32_t)t->n_lanes, &t->xch);
    hipTableUnlockExclusive(t);
    if (rc != PQPS_OK) { t->xch = NULL; return engine_error("exchange set-up"); }
    return 0;
}

int hipEngineJoinConnectHIP(struct engineS *engine, const void *id128) {
    if (!engine || !engine->record_block || !id128) return -1;
    struct hipTable *t = engine->record_block;
    if (!t->xch) return -1;
    if (pqps_exchange_connect(t->xch, (const pqps_rccl_id *)id128) != PQPS_OK) {
        engine_error("communicator");
        pqps_exchange_destroy(t->xch);
        t->xch = NULL;
        return -1;
    }
    return 0;
}

int hipEngineJoinRanksHIP(struct engineS *engine, const char *rccl_library, const void *id128) {
    if (hipEngineJoinPrepareHIP(engine, rccl_library) != 0) return -1;
    return hipEngineJoinConnectHIP(engine, id128);
}

int hipEngineLeaveRanksHIP(struct engineS *engine) {
    if (!engine || !engine->record_block) return -1;
    struct hipTable *t = engine->record_block;
    if (hipTableLockExclusive(t) != 0) return -1;                   /* every ticket is released */
    if (t->xch) { pqps_exchange_destroy(t->xch); t->xch = NULL; }
    hipTableUnlockExclusive(t);
    return 0;
}

int hipEngineWireBytesHIP(struct engineS *engine, unsigned long long out[2], int reset) {
    if (!engine || !engine->record_block || !out) return -1;
    struct hipTable *t = engine->record_block;
    uint64_t b[2] = { 0, 0 };
    if (t->xch) pqps_exchange_wire_bytes(t->xch, b, reset);
    out[0] = b[0];
    out[1] = b[1];
    return 0;
}

int hipEngineEagerQueriesHIP(struct engineS *engine, unsigned long long out[3], int reset) {
    if (!engine || !engine->record_block || !out) return -1;
    struct hipTable *t = engine->record_block;
    uint64_t b[3] = { 0, 0, 0 };
    if (t->xch) pqps_exchange_eager(t->xch, b, reset);
    out[0] = b[0];
    out[1] = b[1];
    out[2] = b[2];
    return 0;
}

int hipEngineLanes(struct engineS *engine) {
    if (!engine || !engine->record_block) return -1;
    return hipTableLaneCount(engine->record_block);
}

/* The lane goes back (its device buffers are no longer this query's); the table stays locked shared. */
static void ticket_release_lane(struct hipQueryTicket *tk) {
    if (tk->state == 2) return;
    /* never leave a launch behind that writes into a freed lane */
    if (tk->state == 0) (void)query_await(&tk->q);
    else if (tk->state < 0) for (int sx = 0; sx < tk->q.n_shards; sx++) (void)wait_shard(&tk->q, sx);
    query_free(&tk->q);
    hipTableReleaseLane(tk->q.t, tk->q.lane);
    tk->state = 2;
}

void releaseQueryHIP(struct hipQueryTicket *tk) {
    if (!tk) return;
    struct hipTable *t = tk->q.t;
    ticket_release_lane(tk);
    hipTableUnlockShared(t);
    free(tk);
}

/* The answer's row numbers on the host (malloc'd); -1 on error. */
static long long ticket_download_ids(struct hipQueryTicket *tk, unsigned int **ids) {
    *ids = NULL;
    long long count = awaitQueryHIP(tk, NULL);
    if (count < 0) return -1;
    unsigned int *out = malloc((count ? (size_t)count : 1) * sizeof *out);
    if (!out) { fprintf(stderr, "HIP engine: out of memory for %lld result IDs\n", count); return -1; }
    if (count && pqps_download(tk->q.ids_ctx, out, tk->q.ids_dev, (size_t)count * sizeof *out, NULL) != PQPS_OK) {
        engine_error("ID download");
        free(out);
        return -1;
    }
    *ids = out;
    return count;
}

/* The filter without the projection: the row numbers on the host. */
long long executeQuerySelectIdsHIP(struct engineS *engine, struct whereClauseS *whereClause,
                                   unsigned int **ids, double *queryTime) {
    if (!engine || !engine->record_block || !ids) return -1;
    *ids = NULL;
    const double t0 = now_seconds();
    struct hipQueryTicket *tk = executeQuerySelectAsyncHIP(engine, whereClause);
    const long long count = tk ? ticket_download_ids(tk, ids) : -1;
    releaseQueryHIP(tk);
    if (queryTime) *queryTime = now_seconds() - t0;
    return count;
}

long long executeQueryCountHIP(struct engineS *engine, struct whereClauseS *whereClause) {
    if (!engine || !engine->record_block) return -1;
    struct hipQueryTicket *tk = executeQueryCountAsyncHIP(engine, whereClause);
    const long long count = awaitQueryHIP(tk, NULL);
    releaseQueryHIP(tk);
    return count;
}

/* ---- what grouped COUNT, the aggregates, COUNT(DISTINCT) and ORDER BY share --------------------------------------- */

/* The table locked shared, a lane taken and q ready for a query; false where the lane is refused (reason on stderr,
 * nothing held).  query_close() gives all of it back. */
static bool query_open(struct engineS *engine, struct query *q) {
    struct hipTable *t = engine->record_block;
    hipTableLockShared(t);
    const int lane = hipTableAcquireLane(t);
    if (lane == HIP_LANE_REFUSED) { hipTableUnlockShared(t); return false; }
    query_init(q, engine, t, lane, false);
    return true;
}

static void query_close(struct query *q) {
    query_free(q);
    hipTableReleaseLane(q->t, q->lane);
    hipTableUnlockShared(q->t);
}

/* The selection, every shard's list left on its own device (q->count[s] rows in query_lane(q, s)); q->total of them. */
static int query_lists(struct query *q) {
    if (q->listed) return 0;
    q->per_shard = true;
    int rc = query_issue_all(q);
    if (rc == 0) rc = query_await(q);
    if (rc == 0 && q->keep_lists) q->listed = true;
    return rc;
}


/* A fused query (single-pass scan-mode WHERE): under the issue lock `call` makes the ONE shim call of every non-empty
 * shard s, on (ctx, stream) of the query's lane with q->sp[s] holding the pass's predicate and columns, and returns 0 or
 * the engine_error; then every shard is waited for, also after an error. */
typedef int (*fused_call)(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg);

static int fused_issue(struct query *q, fused_call call, void *arg) {
    const struct hipPass *last = &q->plan.pass[0];
    int rc = 0;
    hipTableLockIssue(q->t);
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        struct shard_pred *sp = &q->sp[s];
        pqps_ctx *ctx = sh->ctx;
        void *stream = NULL;
        if (sh->n_rows == 0) continue;
        if (q->lane >= 0 && pqps_qstream_lane(sh->qs, (uint32_t)q->lane, sh->n_rows, NULL, &ctx, &stream) != PQPS_OK) { rc = engine_error("query lane"); break; }
        sp->pred = &last->pred;
        sp->n_cols = last->pred.n_columns;
        pass_columns(sh, last, NULL, true, false, sp->cols);
        rc = call(q, s, ctx, stream, arg);
        /* marked even after a failed call: the lane must not be handed on while a launch of this query runs */
        if (q->lane >= 0 && pqps_qstream_mark(sh->qs, (uint32_t)q->lane) != PQPS_OK && rc == 0) rc = engine_error("query lane");
    }
    hipTableUnlockIssue(q->t);
    for (int s = 0; s < q->n_shards; s++) if (wait_shard(q, s) != 0 && rc == 0) rc = -1;
    return rc;
}

/* The query on every shard, reduced on the host: what the dense bins of grouped COUNT, the aggregates, the buckets, the
 * pairs and the first rows do.  Every shard with rows gets one device buffer of the query's own, [head][out]: `head_bytes`
 * uploaded from `head` before anything is issued (the out part starts on the next 16 bytes), `bytes` of output.  Then
 * either `fused` makes the one launch per shard (fused_issue), or the selection is left per shard (query_lists) and `list`
 * runs over every shard's list that has rows, on the lane's copy context, writes `out` and returns the shim's status.
 * After the waits a shard's out part is downloaded and handed to `combine`; or, where the answer is no buffer of a fixed
 * size, `post` takes the out part on its device instead (on the lane's copy context; it returns 0 or its engine_error), and
 * `bytes` may be 0: no buffer, out is NULL.  `list` may be NULL when `post` does the list's work.  No callback sees a shard
 * without rows. */
struct shard_reduce {
    const char *what;                    /* the query's word in the messages of a failed device call */
    const void *head;
    size_t head_bytes, bytes;
    fused_call fused;
    int (*list)(struct query *q, int s, pqps_ctx *cs, const struct hipLane *L, void *out, void *arg);
    void (*combine)(void *arg, const void *host);
    int (*post)(struct query *q, int s, pqps_ctx *cs, void *out, void *arg);
};

static size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

/* buf[0 .. n_shards): filled with the shards' buffers for the callbacks (which find it through `arg`), freed on return. */
static int shard_reduce(struct query *q, bool fused, const struct shard_reduce *r, void **buf, void *arg) {
    const size_t head = pad16(r->head_bytes);
    void *host = r->post ? NULL : malloc(r->bytes);
    int rc = host || r->post ? 0 : oom();
    for (int s = 0; s < q->n_shards; s++) buf[s] = NULL;
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        if (sh->n_rows == 0 || head + r->bytes == 0) continue;
        if (pqps_malloc(sh->ctx, head + r->bytes, &buf[s]) != PQPS_OK ||
            (r->head_bytes && pqps_upload(lane_copy_ctx(q, s), buf[s], r->head, r->head_bytes, NULL) != PQPS_OK))
            rc = engine_error(r->what);
    }
    if (rc == 0) rc = fused ? fused_issue(q, r->fused, arg) : query_lists(q);
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        if (hipTableShard(q->t, s)->n_rows == 0 || (!fused && q->count[s] == 0)) continue;
        pqps_ctx *cs = lane_copy_ctx(q, s);
        void *out = buf[s] ? (char *)buf[s] + head : NULL;
        if (!fused && r->list && r->list(q, s, cs, query_lane(q, s), out, arg) != PQPS_OK) rc = engine_error(r->what);
        else if (r->post) rc = r->post(q, s, cs, out, arg);
        else if (pqps_download(cs, host, out, r->bytes, NULL) != PQPS_OK) rc = engine_error(r->what);
        else r->combine(arg, host);
    }
    for (int s = 0; s < q->n_shards; s++) if (buf[s]) pqps_free(hipTableShard(q->t, s)->ctx, buf[s]);
    free(host);
    return rc;
}

/* ---- several COUNT(*) in as few scans as they need (include/executeEngine-hip.h) ---------------------------------- */

/* The batches of one call: batch b is `pass[b]` to pass_columns (its columns; more comparisons than the specialised shapes
 * take, so that sudo_used is read from its plane in every slot but a lone one) and one launch into buf[s] + b * 16. */
struct count_many_call {
    const struct hipCountBatch *batch;
    const struct hipPass *pass;
    int n_batches;
    uint64_t *buf[HIP_MAX_SHARDS];
};

static int count_many_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct count_many_call *c = arg;
    const struct hipTable *sh = hipTableShard(q->t, s);
    for (int b = 0; b < c->n_batches; b++) {
        pqps_column cols[PQPS_MAX_COLUMNS];
        if (c->batch[b].prog.n_queries < HIP_COUNT_MANY_MIN_BATCH) continue;       /* (its clauses run alone) */
        pass_columns(sh, &c->pass[b], NULL, true, false, cols);
        TRY(pqps_filter_count_many(ctx, cols, c->batch[b].prog.n_columns, sh->n_rows, &c->batch[b].prog,
                                   c->buf[s] + (size_t)b * PQPS_COUNT_MANY_MAX, stream), "count many");
    }
    return 0;
}

long long executeQueryCountManyHIP(struct engineS *engine, struct whereClauseS *const *whereClauses, int numQueries, long long *counts) {
    if (!engine || !engine->record_block || !counts || numQueries < 0 || (numQueries && !whereClauses)) {
        fprintf(stderr, "HIP engine: count many: NULL engine, clauses or counts, or a negative number of clauses\n");
        return -1;
    }
    if (numQueries == 0) return 0;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: several counts in one scan are not exchanged across ranks\n"); return -1; }
    struct query qs, *q = &qs;
    if (!query_open(engine, q)) return -1;
    const size_t n = (size_t)numQueries;
    struct hipPlan *plans = calloc(n, sizeof *plans);
    bool *bound = calloc(n, sizeof *bound);
    int *fused_of = malloc(n * sizeof *fused_of);                   /* clause i is queries[fused_of[i]] of the packer, or -1: alone */
    struct hipCountQuery *queries = malloc(n * sizeof *queries);
    struct hipCountPlace *place = malloc(n * sizeof *place);
    struct hipCountBatch *batches = malloc(n * sizeof *batches);
    long long *answer = malloc(n * sizeof *answer);
    struct hipPass *passes = NULL;
    struct count_many_call call;
    memset(&call, 0, sizeof call);
    int rc = plans && bound && fused_of && queries && place && batches && answer ? 0 : oom();
    int n_fused = 0, n_batches = 0;
    for (size_t i = 0; i < n && rc == 0; i++) {                     /* one bind per clause */
        if (bind_where(t, whereClauses[i], &plans[i]) != 0) { rc = -1; break; }
        bound[i] = true;
        fused_of[i] = -1;
        if (plans[i].n_passes != 1 || plans[i].pass[0].member) continue;
        queries[n_fused].pred = &plans[i].pass[0].pred;
        queries[n_fused].column_ids = plans[i].pass[0].column_ids;
        fused_of[i] = n_fused++;
    }
    if (rc == 0 && hipCountManyPack(queries, n_fused, HIP_COUNT_MANY_BATCH, batches, &n_batches, place) != 0) rc = -1;
    uint64_t rows = 0;
    for (int s = 0; s < q->n_shards; s++) rows += hipTableShard(t, s)->n_rows;
    if (rc == 0 && n_batches) {
        passes = calloc((size_t)n_batches, sizeof *passes);
        if (!passes) rc = oom();
        for (int b = 0; b < n_batches && rc == 0; b++) {
            passes[b].pred.n_columns = batches[b].prog.n_columns;
            passes[b].pred.n_leaves = PQPS_MAX_LEAVES;
            memcpy(passes[b].column_ids, batches[b].column_ids, sizeof passes[b].column_ids);
        }
        call.batch = batches;
        call.pass = passes;
        call.n_batches = n_batches;
        const size_t bytes = (size_t)n_batches * PQPS_COUNT_MANY_MAX * sizeof(uint64_t);
        for (int s = 0; s < q->n_shards && rc == 0; s++)
            if (hipTableShard(t, s)->n_rows && pqps_malloc(hipTableShard(t, s)->ctx, bytes, (void **)&call.buf[s]) != PQPS_OK) rc = engine_error("count many buffer");
        if (rc == 0) {
            q->plan.n_passes = 1;                                   /* (fused_issue: the first batch as the pass; it fills q->sp, the call takes its own columns) */
            q->plan.pass = passes;
            rc = fused_issue(q, count_many_fused_call, &call);
            q->plan.n_passes = 0;
            q->plan.pass = NULL;
        }
    }
    for (size_t i = 0; i < n && rc == 0; i++) answer[i] = 0;
    uint64_t *host = rc == 0 && n_batches ? malloc((size_t)n_batches * PQPS_COUNT_MANY_MAX * sizeof *host) : NULL;
    if (rc == 0 && n_batches && !host) rc = oom();
    for (int s = 0; s < q->n_shards && rc == 0 && n_batches; s++) {
        if (!call.buf[s]) continue;
        if (pqps_download(lane_copy_ctx(q, s), host, call.buf[s], (size_t)n_batches * PQPS_COUNT_MANY_MAX * sizeof *host, NULL) != PQPS_OK) { rc = engine_error("count many download"); break; }
        for (size_t i = 0; i < n; i++) {
            if (fused_of[i] < 0 || place[fused_of[i]].batch < 0 || batches[place[fused_of[i]].batch].prog.n_queries < HIP_COUNT_MANY_MIN_BATCH) continue;
            answer[i] += (long long)host[(size_t)place[fused_of[i]].batch * PQPS_COUNT_MANY_MAX + (size_t)place[fused_of[i]].position];
        }
    }
    free(host);
    for (size_t i = 0; i < n && rc == 0; i++) {
        const int f = fused_of[i];
        if (f >= 0 && place[f].batch >= 0 && batches[place[f].batch].prog.n_queries >= HIP_COUNT_MANY_MIN_BATCH) continue;
        if (f >= 0 && place[f].batch == HIPCOUNT_CONSTANT) { answer[i] = place[f].constant ? (long long)rows : 0; continue; }
        /* alone, or in a batch too small to pay: the COUNT of executeQueryCountHIP with the plan bound above, on this call's lane */
        struct query one;
        query_init(&one, engine, t, q->lane, true);
        one.plan = plans[i];
        one.have_plan = true;
        bound[i] = false;                                           /* (query_free frees the plan) */
        if (query_issue_all(&one) != 0) { rc = -1; for (int s = 0; s < one.n_shards; s++) (void)wait_shard(&one, s); }
        else if (query_await(&one) != 0) rc = -1;
        answer[i] = (long long)one.total;
        query_free(&one);
    }
    for (int s = 0; s < q->n_shards; s++) if (call.buf[s]) pqps_free(hipTableShard(t, s)->ctx, call.buf[s]);
    for (size_t i = 0; plans && bound && i < n; i++) if (bound[i]) hipPlanFree(&plans[i]);
    if (rc == 0) memcpy(counts, answer, n * sizeof *counts);
    free(plans); free(bound); free(fused_of); free(queries); free(place); free(batches); free(answer); free(passes);
    query_close(q);
    return rc == 0 ? (long long)numQueries : -1;
}

/* ---- grouped COUNT(*) (include/executeEngine-hip.h) --------------------------------------------------------------- */

static const int k_group_kind[HIPCOL_COUNT] = {
    HIPKIND_U64, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_I32, HIPKIND_DICT,
    HIPKIND_BOOL, HIPKIND_DICT, HIPKIND_I32, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_I32
};
#define HIP_GROUP_MAX_BINS 65536ull

/* [lo, hi] of an i32 column over every shard, computed once (pqps_column_bounds on each shard) and cached with the table.
 * Readers hold the table shared: two of them may come here at once. */
static pthread_mutex_t g_bounds_lock = PTHREAD_MUTEX_INITIALIZER;

static int column_bounds(struct query *q, int c, int32_t *lo, int32_t *hi) {
    struct hipTable *t = q->t;
    int rc = 0;
    pthread_mutex_lock(&g_bounds_lock);
    if (!t->bounds_known[c]) {
        int32_t l = INT_MAX, h = INT_MIN;
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            struct hipTable *sh = hipTableShard(t, s);
            if (sh->n_rows == 0) continue;
            pqps_ctx *cs = lane_copy_ctx(q, s);
            int32_t *out_dev = NULL, out[2];
            if (pqps_malloc(sh->ctx, 2 * sizeof(int32_t), (void **)&out_dev) != PQPS_OK) { rc = engine_error("bounds buffer"); break; }
            if (pqps_column_bounds(cs, &sh->col[c], sh->n_rows, out_dev, NULL) != PQPS_OK ||
                pqps_download(cs, out, out_dev, sizeof out, NULL) != PQPS_OK)
                rc = engine_error("column bounds");
            pqps_free(sh->ctx, out_dev);
            if (rc == 0) { if (out[0] < l) l = out[0]; if (out[1] > h) h = out[1]; }
        }
        if (rc == 0) { t->bounds_lo[c] = l; t->bounds_hi[c] = h; t->bounds_known[c] = 1; }
    }
    *lo = t->bounds_lo[c];
    *hi = t->bounds_hi[c];
    pthread_mutex_unlock(&g_bounds_lock);
    return rc;
}

/* How a grouped query bins its rows (shared by grouped COUNT and the aggregates). */
struct group_plan {
    int c;                               /* HIPCOL_* of the group column, -1 without GROUP BY                        */
    int kind;                            /* k_group_kind[c], -1 without GROUP BY                                     */
    uint32_t n_bins, bin_base;           /* 1 / 0 without GROUP BY                                                   */
    uint64_t span;                       /* the bins as a 64-bit count: n_bins, but 2^32 for an i32 column that holds
                                            INT_MIN and INT_MAX (n_bins is then 2^32 - 1; only the top groups ask)   */
    int32_t lo;                          /* i32 group column: the key of bin 0                                       */
    bool single;                         /* a single-valued dictionary column (no buffer): every row is bin 0        */
    bool empty;                          /* no rows in the table: no groups, nothing to launch                      */
    bool fused;                          /* single-pass scan-mode WHERE: one fused launch per shard                 */
    pqps_column gcol[HIP_MAX_SHARDS];    /* shard s's group column (sudo_used: its bit plane on the fused path)      */
};

/* The HIPCOL_* of a group column, or -1 with the reason on stderr (`what`: the query's name in the message). */
static int group_column_id(const char *what, const char *column) {
    const int c = hipColumnId(column);
    if (c < 0) { fprintf(stderr, "HIP engine: %s: unknown column '%s'\n", what, column); return -1; }
    if (c == HIPCOL_COMMAND_ID) { fprintf(stderr, "HIP engine: %s: command_id is unique -- grouping on it is the SELECT\n", what); return -1; }
    return c;
}

/* The HIPCOL_* of a value column (a number: i32 or command_id), or -1 with the reason on stderr. */
static int value_column_id(const char *what, const char *column) {
    const int v = hipColumnId(column);
    if (v < 0) { fprintf(stderr, "HIP engine: %s: unknown value column '%s'\n", what, column); return -1; }
    if (k_group_kind[v] != HIPKIND_I32 && k_group_kind[v] != HIPKIND_U64) {
        fprintf(stderr, "HIP engine: %s: %s is a %s column, not a number\n", what, column, k_group_kind[v] == HIPKIND_BOOL ? "boolean" : "dictionary");
        return -1;
    }
    return v;
}

/* Binds the WHERE into q: the plan and the index probes. */
static int query_bind(struct engineS *engine, struct whereClauseS *whereClause, struct query *q) {
    int rc = bind_where(q->t, whereClause, &q->plan);
    q->have_plan = rc == 0;
    if (rc == 0) {
        q->n_probes = list_probes(engine, q->t, whereClause, &q->probes);
        if (q->n_probes < 0) { q->n_probes = 0; rc = -1; }
    }
    return rc;
}

/* The bins of group column c (-1: none) of a bound query: codes of a dictionary (none for a single-valued column: every row
 * is bin 0), 0 / 1, or the i32 range.  `column`: its name, `what`: the query's, for the messages.  `any_span`: the caller
 * takes an i32 range of any size (the top groups); every other caller refuses one above HIP_GROUP_MAX_BINS here. */
static int group_plan_bins(struct query *q, int c, const char *column, const char *what, bool any_span, struct group_plan *gp) {
    struct hipTable *t = q->t;
    int rc = 0;
    int32_t hi = -1;
    uint64_t rows = 0;
    for (int s = 0; s < q->n_shards; s++) rows += hipTableShard(t, s)->n_rows;
    if (rows == 0) gp->empty = true;                                     /* an empty table: no groups */
    else if (c >= 0) {
        if (gp->kind == HIPKIND_DICT) {
            gp->n_bins = t->dict[c].count > 0 ? (uint32_t)t->dict[c].count : 1u;
            gp->single = t->col[c].width == 0;
        } else if (gp->kind == HIPKIND_BOOL) {
            gp->n_bins = 2;
        } else if ((rc = column_bounds(q, c, &gp->lo, &hi)) == 0) {
            if (gp->lo > hi) gp->empty = true;                           /* no rows at all */
            else if (!any_span && (uint64_t)((int64_t)hi - (int64_t)gp->lo) + 1u > HIP_GROUP_MAX_BINS) {
                fprintf(stderr, "HIP engine: %s: %s spans %lld values, more than %llu groups\n", what, column,
                        (long long)hi - (long long)gp->lo + 1, HIP_GROUP_MAX_BINS);
                rc = -1;
            } else {
                gp->span = (uint64_t)((int64_t)hi - (int64_t)gp->lo) + 1u;
                gp->n_bins = gp->span > UINT32_MAX ? UINT32_MAX : (uint32_t)gp->span;
                gp->bin_base = (uint32_t)gp->lo;
            }
        }
    }
    if (gp->kind != HIPKIND_I32) gp->span = gp->n_bins;
    return rc;
}

/* The plan of group column c (-1: none) of a query whose WHERE is bound (`bound` == 0; otherwise only the fields that need
 * no table are set, and `bound` is returned): its bins, whether the query is fused, and every shard's group column. */
static int group_plan_column_span(struct query *q, int bound, int c, const char *column, const char *what, bool any_span, struct group_plan *gp) {
    memset(gp, 0, sizeof *gp);
    gp->c = c;
    gp->kind = c >= 0 ? k_group_kind[c] : -1;
    gp->n_bins = 1;
    gp->span = 1;
    const int rc = bound == 0 ? group_plan_bins(q, c, column, what, any_span, gp) : bound;
    gp->fused = q->plan.n_passes == 1 && q->n_probes == 0;
    for (int s = 0; s < q->n_shards && c >= 0; s++) {
        const struct hipTable *sh = hipTableShard(q->t, s);
        gp->gcol[s] = gp->fused && c == HIPCOL_SUDO_USED && sh->sudo_bits.data ? sh->sudo_bits : sh->col[c];
    }
    return rc;
}

static int group_plan_column(struct query *q, int bound, int c, const char *column, const char *what, struct group_plan *gp) {
    return group_plan_column_span(q, bound, c, column, what, false, gp);
}

/* Binds the WHERE into q (query_bind) and decides the bins of group column c (group_plan_column). */
static int group_plan_init(struct engineS *engine, struct whereClauseS *whereClause, struct query *q, int c, const char *column,
                           const char *what, struct group_plan *gp) {
    return group_plan_column(q, query_bind(engine, whereClause, q), c, column, what, gp);
}

/* The host accumulator of n > 0 dense bins: n counts (COUNT(DISTINCT)'s per-group answers too), or with a value column the
 * [4][n] u64 fields of pqps_filter_aggregate (count, sum, min image, max image) with the min images all ones.  NULL, said
 * on stderr: out of memory. */
static uint64_t *bins_alloc(uint64_t n, bool valued) {
    uint64_t *acc = calloc((size_t)(valued ? 4 : 1) * n, sizeof *acc);
    if (!acc) oom();
    for (uint64_t k = 0; acc && valued && k < n; k++) acc[2 * n + k] = UINT64_MAX;
    return acc;
}

static size_t bins_bytes(uint32_t n, int vc) { return vc < 0 ? (size_t)n * sizeof(uint32_t) : (size_t)n * 4 * sizeof(uint64_t); }

/* What the dense bins are added into: first in the arg of every shard_reduce whose combine is group_combine. */
struct bins_acc { uint64_t *acc; uint32_t n_bins; int vc; };

/* One shard's result added into the host accumulator: COUNT (vc < 0) u32 bins into acc[0 .. n_bins); an aggregate the
 * [4][n_bins] u64 fields into acc[4 * n_bins] (counts and sums added, min / max images taken). */
static void group_combine(void *arg, const void *host) {
    const struct bins_acc *b = arg;
    const uint32_t n_bins = b->n_bins;
    uint64_t *acc = b->acc;
    if (b->vc < 0) {
        for (uint32_t k = 0; k < n_bins; k++) acc[k] += ((const uint32_t *)host)[k];
        return;
    }
    const uint64_t *h = host;
    for (uint32_t k = 0; k < 2 * n_bins; k++) acc[k] += h[k];
    for (uint32_t k = 2 * n_bins; k < 3 * n_bins; k++) if (h[k] < acc[k]) acc[k] = h[k];
    for (uint32_t k = 3 * n_bins; k < 4 * n_bins; k++) if (h[k] > acc[k]) acc[k] = h[k];
}

/* The bins of the query on every shard, combined on the host (shard_reduce, group_combine).  vc < 0: grouped COUNT
 * (pqps_filter_group / pqps_group_list); otherwise the aggregates of value column vc (pqps_filter_aggregate /
 * pqps_aggregate_list; no group column without GROUP BY or for a single-valued one). */
struct group_call { struct bins_acc into; const struct group_plan *gp; void **bins_dev; };

static int group_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct group_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const bool grouped = gp->c >= 0 && !gp->single;
    const int vc = a->into.vc;
    const int rc = vc < 0 ? pqps_filter_group(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &gp->gcol[s], gp->bin_base, gp->n_bins, a->bins_dev[s], stream)
                          : pqps_filter_aggregate(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &sh->col[vc], grouped ? &gp->gcol[s] : NULL,
                                                  gp->bin_base, gp->n_bins, a->bins_dev[s], stream);
    return rc == PQPS_OK ? 0 : engine_error("group filter");
}

static int group_list_call(struct query *q, int s, pqps_ctx *cs, const struct hipLane *L, void *out, void *arg) {
    const struct group_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const bool grouped = gp->c >= 0 && !gp->single;
    const int vc = a->into.vc;
    return vc < 0 ? pqps_group_list(cs, &gp->gcol[s], sh->n_rows, L->ids_dev, L->count_dev, q->count[s], (uint32_t)sh->row0, gp->bin_base, gp->n_bins, out, NULL)
                  : pqps_aggregate_list(cs, &sh->col[vc], grouped ? &gp->gcol[s] : NULL, sh->n_rows, L->ids_dev, L->count_dev, q->count[s],
                                        (uint32_t)sh->row0, gp->bin_base, gp->n_bins, out, NULL);
}

static int group_bins(struct query *q, const struct group_plan *gp, int vc, uint64_t *acc) {
    void *bins_dev[HIP_MAX_SHARDS];
    const struct shard_reduce r = { .what = "group bins", .bytes = bins_bytes(gp->n_bins, vc), .fused = group_fused_call,
                                    .list = group_list_call, .combine = group_combine };
    return shard_reduce(q, gp->fused, &r, bins_dev, &(struct group_call){ { acc, gp->n_bins, vc }, gp, bins_dev });
}

/* The rows of every group (counts[0 .. n_bins)), as grouped COUNT finds them (COUNT(DISTINCT) of a single-valued column too). */
static int group_counts(struct query *q, const struct group_plan *gp, uint64_t *counts) {
    if (!gp->single && gp->c >= 0) return group_bins(q, gp, -1, counts);
    /* one group: the number of rows the selection returns (scan mode: the count, no list) */
    q->count_only = q->n_probes == 0;
    int rc = query_issue_all(q);
    if (rc == 0) rc = query_await(q);
    if (rc == 0) counts[0] = q->total;
    return rc;
}

/* The key and key text of bin k of group column c (kind `kind`); text points into buf or the dictionary. */
static const char *group_key(const struct hipTable *t, int c, int kind, uint32_t k, int32_t lo, long long *key, char *buf, size_t len) {
    if (kind == HIPKIND_I32) { *key = (long long)lo + (long long)k; snprintf(buf, len, "%d", (int)*key); return buf; }
    *key = k;
    if (kind == HIPKIND_BOOL) return k ? "true" : "false";
    return t->dict[c].values[k];
}

/* The groups of a result: the bins k of 0 .. n_bins with nonzero[k], in bin order.  *numGroups = how many; with a group
 * column (column >= 0) *keys and *keyText get their keys and owned texts (one spare entry each).  -1 when out of memory:
 * *numGroups then counts the texts made, so that free_group_keys() frees what there is. */
static int group_keys_fill(const struct hipTable *t, int column, int kind, int32_t lo, const uint64_t *nonzero, uint32_t n_bins,
                           long long **keys, char ***keyText, int *numGroups) {
    int n = 0;
    for (uint32_t k = 0; k < n_bins; k++) n += nonzero[k] != 0;
    *numGroups = column >= 0 ? 0 : n;
    if (column < 0) return 0;
    *keys = calloc((size_t)n + 1, sizeof **keys);
    *keyText = calloc((size_t)n + 1, sizeof **keyText);
    for (uint32_t k = 0; k < n_bins && *keys && *keyText; k++) {
        if (!nonzero[k]) continue;
        char buf[32];
        if (!((*keyText)[*numGroups] = strdup(group_key(t, column, kind, k, lo, &(*keys)[*numGroups], buf, sizeof buf)))) break;
        ++*numGroups;
    }
    if (*keys && *keyText && *numGroups == n) return 0;
    return oom();
}

static void free_group_keys(long long *keys, char **keyText, int numGroups) {
    for (int g = 0; g < numGroups && keyText; g++) free(keyText[g]);
    free(keyText);
    free(keys);
}

/* The per-group arrays of a result with n groups: counts and, with a value column, sums / mins / maxs; n + 1 entries each. */
static int group_arrays_alloc(size_t n, bool valued, unsigned long long **counts, long long **sums, long long **mins, long long **maxs) {
    *counts = calloc(n + 1, sizeof **counts);
    if (valued) {
        *sums = calloc(n + 1, sizeof **sums);
        *mins = calloc(n + 1, sizeof **mins);
        *maxs = calloc(n + 1, sizeof **maxs);
    }
    return *counts && (!valued || (*sums && *mins && *maxs)) ? 0 : oom();
}

/* Group g of those arrays (sums == NULL: its count alone) from the accumulated fields.  The image of an i32 value is
 * (u64)(i64)v ^ 2^63, of a u64 value the value itself. */
static void group_arrays_set(unsigned long long *counts, long long *sums, long long *mins, long long *maxs, size_t g,
                             uint64_t count, uint64_t sum, uint64_t min_image, uint64_t max_image, int valueKind) {
    const uint64_t flip = valueKind == HIPKIND_I32 ? 0x8000000000000000ull : 0;
    counts[g] = count;
    if (!sums) return;
    sums[g] = (long long)sum;
    mins[g] = (long long)(min_image ^ flip);
    maxs[g] = (long long)(max_image ^ flip);
}

static void group_arrays_free(unsigned long long *counts, long long *sums, long long *mins, long long *maxs) {
    free(counts);
    free(sums);
    free(mins);
    free(maxs);
}

static int group_result_fill(struct hipGroupResult *res, const struct hipTable *t, const uint64_t *counts, uint32_t n_bins, int32_t lo) {
    if (group_keys_fill(t, res->column, res->kind, lo, counts, n_bins, &res->keys, &res->keyText, &res->numGroups) != 0) return -1;
    res->counts = calloc((size_t)res->numGroups + 1, sizeof *res->counts);
    if (!res->counts) return oom();
    int g = 0;
    for (uint32_t k = 0; k < n_bins; k++) {
        if (!counts[k]) continue;
        res->counts[g++] = counts[k];
        res->total += (long long)counts[k];
    }
    return 0;
}

struct hipGroupResult *executeQueryGroupCountHIP(struct engineS *engine, const char *groupColumn, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipGroupResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->column = -1;
    res->kind = -1;
    if (!engine || !engine->record_block || !groupColumn) { fprintf(stderr, "HIP engine: grouped COUNT without an engine or a column\n"); return res; }
    const int c = group_column_id("grouped COUNT", groupColumn);
    if (c < 0) return res;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: grouped COUNT is not exchanged across ranks\n"); return res; }
    res->column = c;
    res->kind = k_group_kind[c];
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    uint64_t *counts = NULL;
    struct group_plan gp;
    int rc = group_plan_init(engine, whereClause, &q, c, groupColumn, "grouped COUNT", &gp);
    if (rc == 0 && !gp.empty && !(counts = bins_alloc(gp.n_bins, false))) rc = -1;
    if (rc == 0 && !gp.empty) rc = group_counts(&q, &gp, counts);
    if (rc == 0 && group_result_fill(res, t, counts ? counts : (uint64_t[1]){ 0 }, gp.empty ? 0u : gp.n_bins, gp.lo) == 0) res->success = true;
    free(counts);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeGroupResultHIP(struct hipGroupResult *res) {
    if (!res) return;
    free_group_keys(res->keys, res->keyText, res->numGroups);
    free(res->counts);
    free(res);
}

/* ---- COUNT / SUM / MIN / MAX of a value column (include/executeEngine-hip.h) ---------------------------------------- */

/* acc[4][n_bins] (count, sum, min image, max image: pqps_filter_aggregate's layout) into the result, groups with rows only */
static int aggregate_result_fill(struct hipAggregateResult *res, const struct hipTable *t, const uint64_t *acc, uint32_t n_bins, int32_t lo) {
    if (group_keys_fill(t, res->groupColumn, res->groupKind, lo, acc, n_bins, &res->keys, &res->keyText, &res->numGroups) != 0) return -1;
    if (group_arrays_alloc((size_t)res->numGroups, true, &res->counts, &res->sums, &res->mins, &res->maxs) != 0) return -1;
    size_t g = 0;
    for (uint32_t k = 0; k < n_bins; k++) {
        if (!acc[k]) continue;
        group_arrays_set(res->counts, res->sums, res->mins, res->maxs, g++, acc[k], acc[n_bins + k], acc[2 * n_bins + k], acc[3 * n_bins + k], res->valueKind);
        res->total += (long long)acc[k];
    }
    return 0;
}

struct hipAggregateResult *executeQueryAggregateHIP(struct engineS *engine, const char *valueColumn, const char *groupColumn,
                                                    struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipAggregateResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->valueColumn = res->valueKind = res->groupColumn = res->groupKind = -1;
    if (!engine || !engine->record_block || !valueColumn) { fprintf(stderr, "HIP engine: aggregate without an engine or a value column\n"); return res; }
    const int v = value_column_id("aggregate", valueColumn);
    if (v < 0) return res;
    const int c = groupColumn ? group_column_id("aggregate", groupColumn) : -1;
    if (groupColumn && c < 0) return res;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: aggregates are not exchanged across ranks\n"); return res; }
    res->valueColumn = v;
    res->valueKind = k_group_kind[v];
    res->groupColumn = c;
    res->groupKind = c >= 0 ? k_group_kind[c] : -1;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    uint64_t *acc = NULL;
    struct group_plan gp;
    int rc = group_plan_init(engine, whereClause, &q, c, groupColumn, "aggregate", &gp);
    if (rc == 0 && !gp.empty && !(acc = bins_alloc(gp.n_bins, true))) rc = -1;
    if (rc == 0 && !gp.empty) rc = group_bins(&q, &gp, v, acc);
    if (rc == 0 && aggregate_result_fill(res, t, acc ? acc : (uint64_t[4]){ 0 }, gp.empty ? 0u : gp.n_bins, gp.lo) == 0) res->success = true;
    free(acc);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeAggregateResultHIP(struct hipAggregateResult *res) {
    if (!res) return;
    free_group_keys(res->keys, res->keyText, res->numGroups);
    group_arrays_free(res->counts, res->sums, res->mins, res->maxs);
    free(res);
}

/* ---- exact percentiles, overall or per group (include/executeEngine-hip.h) ------------------------------------------ */

/* The value column as a radix select sees it: an order-preserving key image of key_bits bits (image = value - key_base in
 * the kernels' arithmetic), and every shard's key column. */
struct quantile_plan {
    int v, kind;
    bool wide;                           /* command_id: 64-bit images                                                */
    bool no_key;                         /* a single-valued string column (no buffer): every value is code 0         */
    bool empty;                          /* no row can match (an i32 column without rows, a selection without rows)  */
    uint64_t key_base;
    uint32_t key_bits;
    pqps_column kcol[HIP_MAX_SHARDS];    /* shard s's key column (sudo_used on the fused path: its bit plane)        */
};

/* the bits an image up to `top` needs, at least 1 */
static uint32_t quantile_bits(uint64_t top) {
    uint32_t bits = 1;
    while (bits < 64 && (top >> bits) != 0) bits++;
    return bits;
}

/* The key plan of value column v of a bound query whose group plan is gp: the dictionary size, 0 / 1, the table-wide i32
 * bounds (column_bounds: cached with the table, kept by the writers), or for command_id the minimum and maximum over the
 * SELECTION -- one aggregate through the grouped queries' driver, which also leaves the lists of a query that has some. */
static int quantile_plan_init(struct query *q, const struct group_plan *gp, int v, struct quantile_plan *qp) {
    struct hipTable *t = q->t;
    int rc = 0;
    memset(qp, 0, sizeof *qp);
    qp->v = v;
    qp->kind = k_group_kind[v];
    qp->wide = qp->kind == HIPKIND_U64;
    qp->key_bits = 1;
    if (qp->kind == HIPKIND_DICT) {
        qp->no_key = t->col[v].width == 0;
        qp->key_bits = quantile_bits(t->dict[v].count > 1 ? (uint64_t)t->dict[v].count - 1 : 0);
    } else if (qp->kind == HIPKIND_I32) {
        int32_t lo, hi;
        if ((rc = column_bounds(q, v, &lo, &hi)) == 0) {
            if (lo > hi) qp->empty = true;
            else { qp->key_base = (uint32_t)lo; qp->key_bits = quantile_bits((uint64_t)((int64_t)hi - (int64_t)lo)); }
        }
    } else if (qp->kind == HIPKIND_U64) {
        struct group_plan one;
        uint64_t acc[4] = { 0, 0, UINT64_MAX, 0 };
        group_plan_column(q, 0, -1, NULL, "percentiles", &one);
        if ((rc = group_bins(q, &one, v, acc)) == 0) {
            if (acc[0] == 0) qp->empty = true;
            else { qp->key_base = acc[2]; qp->key_bits = quantile_bits(acc[3] - acc[2]); }
        }
    }
    for (int s = 0; s < q->n_shards; s++) {
        const struct hipTable *sh = hipTableShard(t, s);
        qp->kcol[s] = gp->fused && v == HIPCOL_SUDO_USED && sh->sudo_bits.data ? sh->sudo_bits : sh->col[v];
    }
    return rc;
}

/* The words one launch may count: PQPS_DIGIT_WORDS_MAX, or what PQPS_QUANTILE_WORDS (read per query; the tests' knob) lowers
 * it to -- never below one group's 16 slots of 11 bits. */
static uint32_t quantile_words_cap(void) {
    const char *env = getenv("PQPS_QUANTILE_WORDS");
    const long long w = env ? atoll(env) : 0;
    const long long least = (long long)HIPQUANTILE_MAX_FRACTIONS << HIPQUANTILE_DIGIT_LDS;
    return w >= least && w < (long long)PQPS_DIGIT_WORDS_MAX ? (uint32_t)w : PQPS_DIGIT_WORDS_MAX;
}

/* One launch per shard of one pass: the tables of the group bins [bin0, bin0 + n_bins) of gp, `slots` per bin, summed over
 * the shards into acc[n_bins * slots << d] (shard_reduce).  A shard's buffer is [prefixes: n_bins * slots u64][tables]. */
struct digit_call {
    uint64_t *acc; size_t words;         /* first: what digit_combine adds into                                      */
    const struct group_plan *gp; const struct quantile_plan *qp; void **buf;
    uint32_t bin0, n_bins, slots, shift, d;
    bool prefixed; size_t head;
};

static void digit_combine(void *arg, const void *host) {
    const struct digit_call *a = arg;
    const uint32_t *h = host;
    for (size_t k = 0; k < a->words; k++) a->acc[k] += h[k];
}

static int digit_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct digit_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct quantile_plan *qp = a->qp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const bool grouped = gp->c >= 0 && !gp->single;
    if (pqps_filter_digit_hist(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &qp->kcol[s], qp->wide, qp->key_base, qp->key_bits,
                               grouped ? &gp->gcol[s] : NULL, gp->bin_base + a->bin0, a->n_bins, a->slots, a->prefixed ? a->buf[s] : NULL,
                               a->shift, a->d, (uint32_t *)((char *)a->buf[s] + a->head), stream) != PQPS_OK)
        return engine_error("percentile filter");
    return 0;
}

static int digit_list_call(struct query *q, int s, pqps_ctx *cs, const struct hipLane *L, void *out, void *arg) {
    const struct digit_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct quantile_plan *qp = a->qp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const bool grouped = gp->c >= 0 && !gp->single;
    return pqps_digit_hist_list(cs, &qp->kcol[s], qp->wide, qp->key_base, qp->key_bits, grouped ? &gp->gcol[s] : NULL, gp->bin_base + a->bin0,
                                a->n_bins, a->slots, a->prefixed ? a->buf[s] : NULL, a->shift, a->d, sh->n_rows, L->ids_dev, L->count_dev,
                                q->count[s], (uint32_t)sh->row0, out, NULL);
}

/* The select's state: per group bin its rows, its prefix slots (ascending, distinct) and, per fraction, the slot it
 * follows and its rank among that slot's rows. */
struct quantile_state {
    int n_fractions;
    uint64_t *counts;                    /* [n_bins]                                                                 */
    uint64_t *prefix;                    /* [n_bins][HIPQUANTILE_MAX_FRACTIONS]                                      */
    int *n_slots;                        /* [n_bins]; 0: no rows                                                     */
    int *slot;                           /* [n_bins][n_fractions]                                                    */
    uint64_t *rank;                      /* [n_bins][n_fractions]                                                    */
};

static void quantile_state_free(struct quantile_state *st) {
    free(st->counts); free(st->prefix); free(st->n_slots); free(st->slot); free(st->rank);
}

static int quantile_state_alloc(struct quantile_state *st, uint32_t n_bins, int n_fractions) {
    memset(st, 0, sizeof *st);
    st->n_fractions = n_fractions;
    st->counts = calloc(n_bins, sizeof *st->counts);
    st->prefix = calloc((size_t)n_bins * HIPQUANTILE_MAX_FRACTIONS, sizeof *st->prefix);
    st->n_slots = calloc(n_bins, sizeof *st->n_slots);
    st->slot = calloc((size_t)n_bins * (size_t)n_fractions, sizeof *st->slot);
    st->rank = calloc((size_t)n_bins * (size_t)n_fractions, sizeof *st->rank);
    return st->counts && st->prefix && st->n_slots && st->slot && st->rank ? 0 : oom();
}

/* The radix select (caller holds the table shared and the query's lane; the WHERE is bound, gp and qp are planned): pass by
 * pass from the top digit, each pass in batches of consecutive group bins that keep a launch within the words cap.  Pass 0
 * leaves every group's rows in st->counts; at the end st->prefix[b][st->slot[b][f]] is the image of fraction f of group b. */
static int quantile_select(struct query *q, const struct group_plan *gp, const struct quantile_plan *qp, const unsigned *ppm,
                           struct quantile_state *st, int *passes) {
    const uint32_t G = gp->n_bins, cap = quantile_words_cap();
    const int F = st->n_fractions;
    void *buf[HIP_MAX_SHARDS];
    uint64_t *acc = NULL, *head = NULL;
    int rc = 0;
    q->keep_lists = true;
    for (uint32_t left = qp->key_bits; left > 0 && rc == 0; ) {
        const bool first = left == qp->key_bits;
        uint32_t slots = 1;
        for (uint32_t b = 0; b < G && !first; b++) if ((uint32_t)st->n_slots[b] > slots) slots = (uint32_t)st->n_slots[b];
        const uint32_t d = hipQuantileDigitBits(left, qp->key_bits, (uint64_t)G * slots), shift = left - d;
        uint32_t per = (cap >> d) / slots;                               /* group bins per launch */
        if (per > G) per = G;
        const size_t words = ((size_t)per * slots) << d, head_words = first ? 0 : (size_t)per * slots;
        acc = malloc(words * sizeof *acc);
        head = malloc((head_words + 1) * sizeof *head);
        if (!acc || !head) rc = oom();
        for (uint32_t b0 = 0; b0 < G && rc == 0; b0 += per) {
            const uint32_t nb = G - b0 < per ? G - b0 : per;
            bool pending = first;
            for (uint32_t b = b0; b < b0 + nb && !pending; b++) pending = st->n_slots[b] > 0;
            if (!pending) continue;                                      /* no group of the window has rows */
            for (size_t k = 0; k < (size_t)nb * slots && !first; k++) {
                const uint32_t b = b0 + (uint32_t)(k / slots), j = (uint32_t)(k % slots);
                head[k] = j < (uint32_t)st->n_slots[b] ? st->prefix[(size_t)b * HIPQUANTILE_MAX_FRACTIONS + j] : UINT64_MAX;
            }
            struct digit_call a = { .acc = acc, .words = ((size_t)nb * slots) << d, .gp = gp, .qp = qp, .buf = buf, .bin0 = b0, .n_bins = nb,
                                    .slots = slots, .shift = shift, .d = d, .prefixed = !first, .head = pad16((size_t)nb * slots * (first ? 0 : 8)) };
            const struct shard_reduce r = { .what = "percentile tables", .head = head, .head_bytes = first ? 0 : (size_t)nb * slots * sizeof *head,
                                            .bytes = a.words * sizeof(uint32_t), .fused = digit_fused_call, .list = digit_list_call,
                                            .combine = digit_combine };
            memset(acc, 0, a.words * sizeof *acc);
            rc = shard_reduce(q, gp->fused, &r, buf, &a);
            ++*passes;
            for (uint32_t b = b0; b < b0 + nb && rc == 0; b++) {
                const uint64_t *tables = acc + (((size_t)(b - b0) * slots) << d);
                uint64_t *rank = st->rank + (size_t)b * (size_t)F, *prefix = st->prefix + (size_t)b * HIPQUANTILE_MAX_FRACTIONS;
                int *slot = st->slot + (size_t)b * (size_t)F;
                if (first) {
                    for (uint32_t k = 0; k < 1u << d; k++) st->counts[b] += tables[k];
                    if (st->counts[b] == 0) continue;
                    for (int f = 0; f < F; f++) rank[f] = hipQuantileRank(st->counts[b], ppm[f]);
                } else if (st->n_slots[b] == 0) continue;
                unsigned int digits[HIPQUANTILE_MAX_FRACTIONS];
                uint64_t ranks_in[HIPQUANTILE_MAX_FRACTIONS], next[HIPQUANTILE_MAX_FRACTIONS];
                int next_slot[HIPQUANTILE_MAX_FRACTIONS], n_next = 0;
                if (hipQuantilePick(tables, d, first ? NULL : prefix, first ? 1 : st->n_slots[b], rank, slot, F, digits, ranks_in, next, next_slot,
                                    &n_next) != 0) { rc = -1; break; }   /* (never: the ranks come from these very counts) */
                for (int f = 0; f < F; f++) { rank[f] = ranks_in[f]; slot[f] = next_slot[f]; }
                for (int j = 0; j < n_next; j++) prefix[j] = next[j];
                st->n_slots[b] = n_next;
            }
        }
        free(acc);
        free(head);
        acc = head = NULL;
        left = shift;
    }
    return rc;
}

/* The select's answer into the result: the groups with rows in bin order, their counts, and per fraction the value. */
static int quantile_result_fill(struct hipQuantileResult *res, const struct hipTable *t, const struct group_plan *gp,
                                const struct quantile_plan *qp, const struct quantile_state *st, uint32_t n_bins) {
    long long *keys = NULL;
    const int F = res->numFractions;
    const int rc = group_keys_fill(t, res->groupColumn, res->groupKind, gp->lo, st->counts, n_bins, &keys, &res->keyText, &res->numGroups);
    free(keys);
    if (rc != 0) return -1;
    const size_t n = (size_t)res->numGroups * (size_t)F;
    res->counts = calloc((size_t)res->numGroups + 1, sizeof *res->counts);
    res->values = calloc(n + 1, sizeof *res->values);
    res->valueText = qp->kind == HIPKIND_DICT ? calloc(n + 1, sizeof *res->valueText) : NULL;
    if (!res->counts || !res->values || (qp->kind == HIPKIND_DICT && !res->valueText)) return oom();
    size_t g = 0;
    for (uint32_t b = 0; b < n_bins; b++) {
        if (!st->counts[b]) continue;
        res->counts[g] = st->counts[b];
        res->total += (long long)st->counts[b];
        for (int f = 0; f < F; f++) {
            const uint64_t image = qp->no_key ? 0 : st->prefix[(size_t)b * HIPQUANTILE_MAX_FRACTIONS + (size_t)st->slot[(size_t)b * (size_t)F + (size_t)f]];
            long long *value = &res->values[g * (size_t)F + (size_t)f];
            if (qp->kind == HIPKIND_U64) *value = (long long)(image + qp->key_base);
            else if (qp->kind == HIPKIND_I32) *value = (int32_t)((uint32_t)image + (uint32_t)qp->key_base);
            else *value = (long long)image;
            if (qp->kind != HIPKIND_DICT) continue;
            if (image >= (uint64_t)t->dict[qp->v].count) { fprintf(stderr, "HIP engine: percentiles: code %llu outside the dictionary\n", (unsigned long long)image); return -1; }
            if (!(res->valueText[g * (size_t)F + (size_t)f] = strdup(t->dict[qp->v].values[image]))) return oom();
        }
        g++;
    }
    return 0;
}

struct hipQuantileResult *executeQueryQuantilesHIP(struct engineS *engine, const char *valueColumn, const char *groupColumn,
                                                   const unsigned *ppm, int numFractions, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipQuantileResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->valueColumn = res->valueKind = res->groupColumn = res->groupKind = -1;
    if (!engine || !engine->record_block || !valueColumn || !ppm) { fprintf(stderr, "HIP engine: percentiles without an engine, a value column or fractions\n"); return res; }
    if (numFractions < 1 || numFractions > HIPQUANTILE_MAX_FRACTIONS) {
        fprintf(stderr, "HIP engine: percentiles: %d fractions, not 1 .. %d\n", numFractions, HIPQUANTILE_MAX_FRACTIONS);
        return res;
    }
    for (int f = 0; f < numFractions; f++)
        if (ppm[f] > HIPQUANTILE_PPM) { fprintf(stderr, "HIP engine: percentiles: %u parts per million is above 1 000 000\n", ppm[f]); return res; }
    const int v = hipColumnId(valueColumn);
    if (v < 0) { fprintf(stderr, "HIP engine: percentiles: unknown value column '%s'\n", valueColumn); return res; }
    const int c = groupColumn ? group_column_id("percentiles", groupColumn) : -1;
    if (groupColumn && c < 0) return res;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: percentiles are not exchanged across ranks\n"); return res; }
    res->valueColumn = v;
    res->valueKind = k_group_kind[v];
    res->groupColumn = c;
    res->groupKind = c >= 0 ? k_group_kind[c] : -1;
    res->numFractions = numFractions;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    struct group_plan gp;
    struct quantile_plan qp;
    struct quantile_state st;
    memset(&st, 0, sizeof st);
    int rc = group_plan_init(engine, whereClause, &q, c, groupColumn, "percentiles", &gp);
    if (rc == 0 && !gp.empty) { q.keep_lists = true; rc = quantile_plan_init(&q, &gp, v, &qp); }
    const bool empty = rc != 0 || gp.empty || qp.empty;
    if (rc == 0 && !empty) rc = quantile_state_alloc(&st, gp.n_bins, numFractions);
    if (rc == 0 && !empty) rc = qp.no_key ? group_counts(&q, &gp, st.counts) : quantile_select(&q, &gp, &qp, ppm, &st, &res->passes);
    if (rc == 0 && !empty) rc = quantile_result_fill(res, t, &gp, &qp, &st, gp.n_bins);
    if (rc == 0) res->success = true;
    quantile_state_free(&st);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeQuantileResultHIP(struct hipQuantileResult *res) {
    if (!res) return;
    const size_t n = (size_t)res->numGroups * (size_t)res->numFractions;
    for (size_t i = 0; i < n && res->valueText; i++) free(res->valueText[i]);
    free(res->valueText);
    free_group_keys(NULL, res->keyText, res->numGroups);
    free(res->counts);
    free(res->values);
    free(res);
}

/* ---- GROUP BY buckets (include/executeEngine-hip.h) ---------------------------------------------------------------- */

/* How a bucketed query bins its rows: gp as the grouped queries use it (column, kind, fused, every shard's group column;
 * n_bins = the buckets), and the run starts of the buckets in bin space with their keys (hipBucketBounds; malloc'd). */
struct bucket_plan {
    struct group_plan gp;
    int mode;
    long long arg;
    uint32_t *bounds;                    /* n_bins + 1 run starts, the last one the domain */
    long long *keys;                     /* n_bins */
};

/* Binds the WHERE into q and decides the buckets of column c (valid for the mode: the caller has checked). */
static int bucket_plan_init(struct engineS *engine, struct whereClauseS *whereClause, struct query *q, int c, const char *column,
                            int mode, long long arg, struct bucket_plan *bp) {
    struct hipTable *t = q->t;
    struct group_plan *gp = &bp->gp;
    memset(bp, 0, sizeof *bp);
    bp->mode = mode;
    bp->arg = arg;
    gp->c = c;
    gp->kind = k_group_kind[c];
    gp->n_bins = 1;
    int rc = query_bind(engine, whereClause, q);
    gp->fused = q->plan.n_passes == 1 && q->n_probes == 0;
    for (int s = 0; s < q->n_shards; s++) gp->gcol[s] = hipTableShard(t, s)->col[c];
    if (rc != 0) return rc;
    uint64_t rows = 0;
    int32_t hi = -1;
    for (int s = 0; s < q->n_shards; s++) rows += hipTableShard(t, s)->n_rows;
    if (rows == 0 || (gp->kind == HIPKIND_DICT && t->dict[c].count < 1)) { gp->empty = true; return 0; }
    if (gp->kind == HIPKIND_DICT) gp->single = t->col[c].width == 0;
    else if ((rc = column_bounds(q, c, &gp->lo, &hi)) != 0) return rc;
    else if (gp->lo > hi) { gp->empty = true; return 0; }
    else gp->bin_base = (uint32_t)gp->lo;
    return hipBucketBounds(column, gp->kind == HIPKIND_DICT ? (const char *const *)t->dict[c].values : NULL,
                           gp->kind == HIPKIND_DICT ? (int)t->dict[c].count : 0, gp->lo, hi, mode, arg, &bp->bounds, &bp->keys, &gp->n_bins);
}

static void bucket_plan_free(struct bucket_plan *bp) {
    free(bp->bounds);
    free(bp->keys);
}

struct bucket_call { struct bins_acc into; const struct bucket_plan *bp; void **buf; size_t head; };

static int bucket_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct bucket_call *a = arg;
    const struct group_plan *gp = &a->bp->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const uint32_t *bounds_dev = a->buf[s];
    void *out = (char *)a->buf[s] + a->head;
    const uint32_t domain = a->bp->bounds[gp->n_bins];
    const int vc = a->into.vc;
    const int rc = vc < 0 ? pqps_filter_group_buckets(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &gp->gcol[s], gp->bin_base, bounds_dev,
                                                      gp->n_bins, domain, out, stream)
                          : pqps_filter_aggregate_buckets(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &sh->col[vc], &gp->gcol[s],
                                                          gp->bin_base, bounds_dev, gp->n_bins, domain, out, stream);
    return rc == PQPS_OK ? 0 : engine_error("bucket filter");
}

static int bucket_list_call(struct query *q, int s, pqps_ctx *cs, const struct hipLane *L, void *out, void *arg) {
    const struct bucket_call *a = arg;
    const struct group_plan *gp = &a->bp->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const uint32_t *bounds_dev = a->buf[s];
    const uint32_t domain = a->bp->bounds[gp->n_bins];
    const int vc = a->into.vc;
    return vc < 0 ? pqps_group_buckets_list(cs, &gp->gcol[s], sh->n_rows, L->ids_dev, L->count_dev, q->count[s], (uint32_t)sh->row0, gp->bin_base,
                                            bounds_dev, gp->n_bins, domain, out, NULL)
                  : pqps_aggregate_buckets_list(cs, &sh->col[vc], &gp->gcol[s], sh->n_rows, L->ids_dev, L->count_dev, q->count[s],
                                                (uint32_t)sh->row0, gp->bin_base, bounds_dev, gp->n_bins, domain, out, NULL);
}

/* The buckets of the query on every shard, combined on the host (shard_reduce, group_combine): vc < 0 the counts, otherwise
 * the aggregates of value column vc.  A shard's buffer is [bounds][bins], the bounds the head that is uploaded once. */
static int bucket_bins(struct query *q, const struct bucket_plan *bp, int vc, uint64_t *acc) {
    const uint32_t n_bins = bp->gp.n_bins;
    void *buf[HIP_MAX_SHARDS];
    const struct shard_reduce r = { .what = "buckets", .head = bp->bounds, .head_bytes = ((size_t)n_bins + 1) * sizeof(uint32_t),
                                    .bytes = bins_bytes(n_bins, vc), .fused = bucket_fused_call, .list = bucket_list_call, .combine = group_combine };
    return shard_reduce(q, bp->gp.fused, &r, buf, &(struct bucket_call){ { acc, n_bins, vc }, bp, buf, pad16(r.head_bytes) });
}

/* acc (counts, or the [4][n_bins] fields) into the result: buckets with rows only, with their keys and key texts */
static int bucket_result_fill(struct hipBucketResult *res, const struct hipTable *t, const struct bucket_plan *bp, const uint64_t *acc, uint32_t n_bins) {
    const bool valued = res->valueColumn >= 0;
    size_t n = 0;
    for (uint32_t k = 0; k < n_bins; k++) n += acc[k] != 0;
    res->keys = calloc(n + 1, sizeof *res->keys);
    res->keyText = calloc(n + 1, sizeof *res->keyText);
    if (!res->keys || !res->keyText) return oom();
    if (group_arrays_alloc(n, valued, &res->counts, &res->sums, &res->mins, &res->maxs) != 0) return -1;
    for (uint32_t k = 0; k < n_bins; k++) {
        if (!acc[k]) continue;
        const int g = res->numGroups;
        char buf[32];
        res->keys[g] = bp->keys[k];
        if (bp->mode == HIPBUCKET_WIDTH) {
            snprintf(buf, sizeof buf, "%lld", bp->keys[k]);
            res->keyText[g] = strdup(buf);
        } else {
            const char *text = t->dict[res->groupColumn].values[bp->keys[k]];
            const size_t len = strlen(text);
            res->keyText[g] = strndup(text, (unsigned long long)bp->arg < len ? (size_t)bp->arg : len);
        }
        if (!res->keyText[g]) return oom();
        group_arrays_set(res->counts, res->sums, res->mins, res->maxs, (size_t)g, acc[k], valued ? acc[n_bins + k] : 0,
                         valued ? acc[2 * n_bins + k] : 0, valued ? acc[3 * n_bins + k] : 0, res->valueKind);
        res->total += (long long)acc[k];
        res->numGroups++;
    }
    return 0;
}

struct hipBucketResult *executeQueryGroupBucketsHIP(struct engineS *engine, const char *groupColumn, int bucketMode, long long bucketArg,
                                                    const char *valueColumn, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipBucketResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->groupColumn = res->groupKind = res->valueColumn = res->valueKind = -1;
    res->bucketMode = bucketMode;
    res->bucketArg = bucketArg;
    if (!engine || !engine->record_block || !groupColumn) { fprintf(stderr, "HIP engine: GROUP BY buckets without an engine or a column\n"); return res; }
    /* column, mode and argument are checked by hipBucketBounds itself, on a one-value column: nothing of the table is needed */
    {
        static const char *const one[1] = { "" };
        uint32_t *b = NULL, n = 0;
        long long *k = NULL;
        if (hipBucketBounds(groupColumn, one, 1, 0, 0, bucketMode, bucketArg, &b, &k, &n) != 0) return res;
        free(b);
        free(k);
    }
    const int c = hipColumnId(groupColumn);
    const int v = valueColumn ? value_column_id("GROUP BY buckets", valueColumn) : -1;
    if (valueColumn && v < 0) return res;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: GROUP BY buckets is not exchanged across ranks\n"); return res; }
    res->groupColumn = c;
    res->groupKind = k_group_kind[c];
    res->valueColumn = v;
    res->valueKind = v >= 0 ? k_group_kind[v] : -1;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    uint64_t *acc = NULL;
    struct bucket_plan bp;
    int rc = bucket_plan_init(engine, whereClause, &q, c, groupColumn, bucketMode, bucketArg, &bp);
    const uint32_t n_bins = rc == 0 && !bp.gp.empty ? bp.gp.n_bins : 0u;
    if (n_bins && !(acc = bins_alloc(n_bins, v >= 0))) rc = -1;
    /* a single-valued column has no device buffer: one bucket from the selection (group_counts), or the ungrouped aggregate */
    if (rc == 0 && n_bins) rc = !bp.gp.single ? bucket_bins(&q, &bp, v, acc) : v < 0 ? group_counts(&q, &bp.gp, acc) : group_bins(&q, &bp.gp, v, acc);
    if (rc == 0 && bucket_result_fill(res, t, &bp, acc ? acc : (uint64_t[4]){ 0 }, n_bins) == 0) res->success = true;
    free(acc);
    bucket_plan_free(&bp);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeBucketResultHIP(struct hipBucketResult *res) {
    if (!res) return;
    free_group_keys(res->keys, res->keyText, res->numGroups);
    group_arrays_free(res->counts, res->sums, res->mins, res->maxs);
    free(res);
}

/* ---- COUNT(DISTINCT value column) (include/executeEngine-hip.h) ---------------------------------------------------- */

#define HIP_DISTINCT_MAX_BITS (1ull << 30)          /* the bitmap forms' cap per shard: 128 MiB */

/* How COUNT(DISTINCT) reads its value column. */
struct distinct_plan {
    int v;                               /* HIPCOL_* of the value column                                             */
    bool single;                         /* a single-valued dictionary column (no buffer): 1 per non-empty group    */
    bool sort;                           /* command_id, or a bitmap above the cap: the sort form                    */
    uint32_t v_base, n_values;           /* value bins: (value - v_base), n_values of them (the bitmap forms)        */
    pqps_column vcol[HIP_MAX_SHARDS];    /* shard s's value column (sudo_used on the fused path: its bit plane)      */
};

/* The value side of the plan (gp already made by group_plan_init, not empty). */
static int distinct_plan_init(struct query *q, const struct group_plan *gp, int v, struct distinct_plan *dp) {
    struct hipTable *t = q->t;
    memset(dp, 0, sizeof *dp);
    dp->v = v;
    dp->n_values = 1;
    const int kind = k_group_kind[v];
    uint64_t dv = 1;
    if (kind == HIPKIND_U64) dp->sort = true;
    else if (kind == HIPKIND_DICT) { dp->single = t->col[v].width == 0; dv = t->dict[v].count > 0 ? (uint64_t)t->dict[v].count : 1u; }
    else if (kind == HIPKIND_BOOL) dv = 2;
    else {
        int32_t lo = 0, hi = -1;
        const int rc = column_bounds(q, v, &lo, &hi);
        if (rc != 0) return rc;
        dv = lo > hi ? 1u : (uint64_t)((int64_t)hi - (int64_t)lo) + 1u;
        dp->v_base = (uint32_t)lo;
    }
    /* (dv <= 2^32: an i32 range over the cap goes to the sort form, whose value image is 32 bits) */
    if (!dp->sort && (uint64_t)gp->n_bins * ((dv + 31) / 32) * 32 > HIP_DISTINCT_MAX_BITS) dp->sort = true;
    if (!dp->sort) dp->n_values = (uint32_t)dv;
    for (int s = 0; s < q->n_shards; s++) {
        const struct hipTable *sh = hipTableShard(t, s);
        dp->vcol[s] = gp->fused && !dp->sort && v == HIPCOL_SUDO_USED && sh->sudo_bits.data ? sh->sudo_bits : sh->col[v];
    }
    return 0;
}

struct distinct_call { const struct group_plan *gp; const struct distinct_plan *dp; void **buf; size_t head; bool *filled; };

/* shard s's buffer buf[s] of the bitmap forms: [total][distinct][bitmap], the bitmap `head` bytes in */
#define DBUF_TOTAL(s) ((uint64_t *)buf[s])
#define DBUF_DISTINCT(s) ((uint64_t *)((char *)buf[s] + 16))
#define DBUF_BITMAP(s) ((uint32_t *)((char *)buf[s] + head))

static int distinct_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct distinct_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct distinct_plan *dp = a->dp;
    void **buf = a->buf;
    const size_t head = a->head;
    const struct shard_pred *sp = &q->sp[s];
    const bool grouped = gp->c >= 0 && !gp->single;
    if (pqps_filter_distinct(ctx, sp->cols, sp->n_cols, hipTableShard(q->t, s)->n_rows, sp->pred, &dp->vcol[s], dp->v_base, dp->n_values,
                             grouped ? &gp->gcol[s] : NULL, gp->bin_base, gp->n_bins, DBUF_BITMAP(s), DBUF_TOTAL(s),
                             q->n_shards > 1 ? NULL : DBUF_DISTINCT(s), stream) != PQPS_OK)
        return engine_error("COUNT(DISTINCT) filter");
    a->filled[s] = true;
    return 0;
}

/* The bitmap forms on every shard: one shard pops its bitmap on its device; several download theirs, OR them on the host
 * and pop the union on the first shard's device -- shard counts are never added.  distinct[0 .. n_bins), *total the rows. */
static int distinct_bitmap(struct query *q, const struct group_plan *gp, const struct distinct_plan *dp, uint64_t *distinct, uint64_t *total) {
    const uint32_t G = gp->n_bins, D = dp->n_values;
    const uint64_t words = pqps_distinct_bitmap_words(D, G);
    const size_t head = 16 + pad16((size_t)G * 8);   /* [total][distinct][bitmap] */
    const size_t bytes = head + words * 4;
    const bool grouped = gp->c >= 0 && !gp->single;
    const bool multi = q->n_shards > 1;
    void *buf[HIP_MAX_SHARDS] = { NULL };
    bool filled[HIP_MAX_SHARDS] = { false };
    int rc = 0;
    *total = 0;
    for (int s = 0; s < q->n_shards && rc == 0; s++)
        if (pqps_malloc(hipTableShard(q->t, s)->ctx, bytes, &buf[s]) != PQPS_OK) rc = engine_error("COUNT(DISTINCT) bitmap");
    if (rc == 0 && gp->fused) {
        rc = fused_issue(q, distinct_fused_call, &(struct distinct_call){ gp, dp, buf, head, filled });
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            uint64_t n = 0;
            if (!filled[s]) continue;
            if (pqps_download(lane_copy_ctx(q, s), &n, DBUF_TOTAL(s), sizeof n, NULL) != PQPS_OK) rc = engine_error("COUNT(DISTINCT) total");
            *total += n;
        }
    } else if (rc == 0) {
        rc = query_lists(q);
        if (rc == 0) *total = q->total;
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            const struct hipTable *sh = hipTableShard(q->t, s);
            struct hipLane *L = query_lane(q, s);
            if (q->count[s] == 0) continue;
            if (pqps_distinct_list(lane_copy_ctx(q, s), &dp->vcol[s], dp->v_base, D, grouped ? &gp->gcol[s] : NULL, gp->bin_base, G, sh->n_rows,
                                   L->ids_dev, L->count_dev, q->count[s], (uint32_t)sh->row0, DBUF_BITMAP(s), multi ? NULL : DBUF_DISTINCT(s), NULL) != PQPS_OK)
                rc = engine_error("COUNT(DISTINCT) list");
            else filled[s] = true;
        }
    }
    if (rc == 0 && !multi) {
        if (filled[0] && pqps_download(lane_copy_ctx(q, 0), distinct, DBUF_DISTINCT(0), (size_t)G * 8, NULL) != PQPS_OK) rc = engine_error("COUNT(DISTINCT) download");
    } else if (rc == 0) {
        uint32_t *merged = calloc(words, sizeof *merged), *part = malloc(words * sizeof *part);
        if (!merged || !part) rc = oom();
        bool any = false;
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            if (!filled[s]) continue;
            if (pqps_download(lane_copy_ctx(q, s), part, DBUF_BITMAP(s), words * 4, NULL) != PQPS_OK) { rc = engine_error("COUNT(DISTINCT) download"); break; }
            for (uint64_t i = 0; i < words; i++) merged[i] |= part[i];
            any = true;
        }
        pqps_ctx *c0 = lane_copy_ctx(q, 0);
        if (rc == 0 && any && (pqps_upload(c0, DBUF_BITMAP(0), merged, words * 4, NULL) != PQPS_OK ||
                               pqps_distinct_count(c0, DBUF_BITMAP(0), D, G, DBUF_DISTINCT(0), NULL) != PQPS_OK ||
                               pqps_download(c0, distinct, DBUF_DISTINCT(0), (size_t)G * 8, NULL) != PQPS_OK))
            rc = engine_error("COUNT(DISTINCT) merge");
        free(merged);
        free(part);
    }
#undef DBUF_TOTAL
#undef DBUF_DISTINCT
#undef DBUF_BITMAP
    for (int s = 0; s < q->n_shards; s++) if (buf[s]) pqps_free(hipTableShard(q->t, s)->ctx, buf[s]);
    return rc;
}

/* One shard's sorted keys on the host, as (group bin, value) pairs in ascending order. */
struct distinct_keys { const uint64_t *k; const uint32_t *g; uint64_t n, at; bool wide; };

static void distinct_key_at(const struct distinct_keys *d, uint64_t i, uint64_t *g, uint64_t *v) {
    if (d->wide) { *g = d->g[i]; *v = d->k[i]; }
    else { *g = d->k[i] >> 32; *v = d->k[i] & 0xFFFFFFFFull; }
}

/* The sort form: the selection, every shard's list sorted on its device (pqps_distinct_sort).  One shard counts on its
 * device; several download their sorted keys and are merged on the host with duplicates dropped. */
static int distinct_sort(struct query *q, const struct group_plan *gp, const struct distinct_plan *dp, uint64_t *distinct, uint64_t *total) {
    const uint32_t G = gp->n_bins;
    const bool grouped = gp->c >= 0 && !gp->single;
    const bool wide = dp->v == HIPCOL_COMMAND_ID;
    const bool multi = q->n_shards > 1;
    int rc = query_lists(q);
    if (rc != 0) return rc;
    *total = q->total;
    struct distinct_keys keys[HIP_MAX_SHARDS];
    void *host[HIP_MAX_SHARDS] = { NULL };
    memset(keys, 0, sizeof keys);
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        const uint64_t n = q->count[s];
        if (n == 0) continue;
        pqps_ctx *cs = lane_copy_ctx(q, s);
        const size_t key_bytes = (size_t)n * (wide ? 12 : 8);
        void *dev = NULL;
        if (pqps_malloc(sh->ctx, (size_t)G * 8 + (multi ? key_bytes : 0), &dev) != PQPS_OK) { rc = engine_error("COUNT(DISTINCT) buffers"); break; }
        uint64_t *keys_dev = multi ? (uint64_t *)((char *)dev + (size_t)G * 8) : NULL;
        if (pqps_distinct_sort(cs, &sh->col[dp->v], dp->v_base, grouped ? &sh->col[gp->c] : NULL, gp->bin_base, G, query_lane(q, s)->ids_dev, n,
                               (uint32_t)sh->row0, dev, keys_dev, NULL) != PQPS_OK) rc = engine_error("COUNT(DISTINCT) sort");
        else if (!multi) { if (pqps_download(cs, distinct, dev, (size_t)G * 8, NULL) != PQPS_OK) rc = engine_error("COUNT(DISTINCT) download"); }
        else if (!(host[s] = malloc(key_bytes))) rc = oom();
        else if (pqps_download(cs, host[s], keys_dev, key_bytes, NULL) != PQPS_OK) rc = engine_error("COUNT(DISTINCT) download");
        else keys[s] = (struct distinct_keys){ host[s], wide ? (const uint32_t *)((uint64_t *)host[s] + n) : NULL, n, 0, wide };
        pqps_free(sh->ctx, dev);
    }
    if (rc == 0 && multi) {                                              /* k-way merge by (group, value), each key once */
        bool have_last = false;
        uint64_t lg = 0, lv = 0;
        for (;;) {
            int best = -1;
            uint64_t bg = 0, bv = 0;
            for (int s = 0; s < q->n_shards; s++) {
                if (keys[s].at >= keys[s].n) continue;
                uint64_t g, v;
                distinct_key_at(&keys[s], keys[s].at, &g, &v);
                if (best < 0 || g < bg || (g == bg && v < bv)) { best = s; bg = g; bv = v; }
            }
            if (best < 0) break;
            keys[best].at++;
            if (have_last && bg == lg && bv == lv) continue;
            have_last = true;
            lg = bg;
            lv = bv;
            if (bg < G) distinct[bg]++;
        }
    }
    for (int s = 0; s < q->n_shards; s++) free(host[s]);
    return rc;
}

/* distinct[0 .. n_bins) into the result: the groups with rows, in bin order */
static int distinct_result_fill(struct hipDistinctResult *res, const struct hipTable *t, const uint64_t *distinct, uint32_t n_bins, int32_t lo) {
    if (group_keys_fill(t, res->groupColumn, res->groupKind, lo, distinct, n_bins, &res->keys, &res->keyText, &res->numGroups) != 0) return -1;
    res->distinct = calloc((size_t)res->numGroups + 1, sizeof *res->distinct);
    if (!res->distinct) return oom();
    int g = 0;
    for (uint32_t k = 0; k < n_bins; k++) if (distinct[k]) res->distinct[g++] = distinct[k];
    return 0;
}

struct hipDistinctResult *executeQueryCountDistinctHIP(struct engineS *engine, const char *valueColumn, const char *groupColumn,
                                                       struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipDistinctResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->valueColumn = res->valueKind = res->groupColumn = res->groupKind = -1;
    if (!engine || !engine->record_block || !valueColumn) { fprintf(stderr, "HIP engine: COUNT(DISTINCT) without an engine or a value column\n"); return res; }
    const int v = hipColumnId(valueColumn);
    if (v < 0) { fprintf(stderr, "HIP engine: COUNT(DISTINCT): unknown value column '%s'\n", valueColumn); return res; }
    const int c = groupColumn ? group_column_id("COUNT(DISTINCT)", groupColumn) : -1;
    if (groupColumn && c < 0) return res;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: COUNT(DISTINCT) is not exchanged across ranks\n"); return res; }
    res->valueColumn = v;
    res->valueKind = k_group_kind[v];
    res->groupColumn = c;
    res->groupKind = c >= 0 ? k_group_kind[c] : -1;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    uint64_t *distinct = NULL, total = 0;
    struct group_plan gp;
    struct distinct_plan dp;
    int rc = group_plan_init(engine, whereClause, &q, c, groupColumn, "COUNT(DISTINCT)", &gp);
    if (rc == 0 && !gp.empty && !(distinct = bins_alloc(gp.n_bins, false))) rc = -1;
    if (rc == 0 && !gp.empty) rc = distinct_plan_init(&q, &gp, v, &dp);
    if (rc == 0 && !gp.empty) {
        if (dp.single) {                                                 /* one value: 1 for every group with rows */
            rc = group_counts(&q, &gp, distinct);
            for (uint32_t k = 0; k < gp.n_bins && rc == 0; k++) { total += distinct[k]; distinct[k] = distinct[k] != 0; }
        } else if (dp.sort) {
            rc = distinct_sort(&q, &gp, &dp, distinct, &total);
        } else {
            rc = distinct_bitmap(&q, &gp, &dp, distinct, &total);
        }
    }
    res->total = (long long)total;
    if (rc == 0 && distinct_result_fill(res, t, distinct ? distinct : (uint64_t[1]){ 0 }, gp.empty ? 0u : gp.n_bins, gp.lo) == 0) res->success = true;
    free(distinct);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeDistinctResultHIP(struct hipDistinctResult *res) {
    if (!res) return;
    free_group_keys(res->keys, res->keyText, res->numGroups);
    free(res->distinct);
    free(res);
}

/* ---- GROUP BY two columns (include/executeEngine-hip.h) ------------------------------------------------------------- */

/* The pairs of an answer, ascending by key = bin of A << 32 | bin of B: counts, and with a value column sums and the min /
 * max images of pqps_filter_aggregate. */
struct pair_rows { uint64_t n; uint64_t *key, *cnt, *sum, *mn, *mx; };

static void pair_rows_free(struct pair_rows *pr) {
    free(pr->key); free(pr->cnt); free(pr->sum); free(pr->mn); free(pr->mx);
    memset(pr, 0, sizeof *pr);
}

static int pair_rows_alloc(struct pair_rows *pr, uint64_t n, bool valued) {
    memset(pr, 0, sizeof *pr);
    pr->key = calloc((size_t)n + 1, sizeof *pr->key);
    pr->cnt = calloc((size_t)n + 1, sizeof *pr->cnt);
    if (valued) {
        pr->sum = calloc((size_t)n + 1, sizeof *pr->sum);
        pr->mn = calloc((size_t)n + 1, sizeof *pr->mn);
        pr->mx = calloc((size_t)n + 1, sizeof *pr->mx);
    }
    if (pr->key && pr->cnt && (!valued || (pr->sum && pr->mn && pr->mx))) return 0;
    pair_rows_free(pr);
    return oom();
}

/* Dense bins (acc: D counts, or the [4][D] fields of group_combine) into pairs: bin k is the pair (k / n_b, k % n_b). */
static int pair_rows_from_bins(const uint64_t *acc, uint32_t D, uint32_t n_b, bool valued, struct pair_rows *pr) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < D; k++) n += acc[k] != 0;
    if (pair_rows_alloc(pr, n, valued) != 0) return -1;
    for (uint32_t k = 0; k < D; k++) {
        if (!acc[k]) continue;
        const uint64_t g = pr->n++;
        pr->key[g] = (uint64_t)(k / n_b) << 32 | (k % n_b);
        pr->cnt[g] = acc[k];
        if (valued) { pr->sum[g] = acc[D + k]; pr->mn[g] = acc[2 * (size_t)D + k]; pr->mx[g] = acc[3 * (size_t)D + k]; }
    }
    return 0;
}

struct pair_call { struct bins_acc into; const struct group_plan *a, *b; void **out_dev; };

static int pair_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct pair_call *p = arg;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const int vc = p->into.vc;
    const int rc = pqps_filter_group_pair(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &p->a->gcol[s], p->a->bin_base, p->a->n_bins,
                                          &p->b->gcol[s], p->b->bin_base, p->b->n_bins, vc >= 0 ? &sh->col[vc] : NULL, p->out_dev[s], stream);
    return rc == PQPS_OK ? 0 : engine_error("group pair filter");
}

/* (off the fused path gcol[s] is the shard's own column) */
static int pair_list_call(struct query *q, int s, pqps_ctx *cs, const struct hipLane *L, void *out, void *arg) {
    const struct pair_call *p = arg;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const int vc = p->into.vc;
    return pqps_group_pair_list(cs, &p->a->gcol[s], p->a->bin_base, p->a->n_bins, &p->b->gcol[s], p->b->bin_base, p->b->n_bins,
                                vc >= 0 ? &sh->col[vc] : NULL, sh->n_rows, L->ids_dev, L->count_dev, q->count[s], (uint32_t)sh->row0, out, NULL);
}

/* The dense bins (D = n_a x n_b <= 65 536) of the query on every shard, combined on the host (shard_reduce, group_combine):
 * pqps_filter_group_pair, or pqps_group_pair_list over every shard's list. */
static int pair_dense(struct query *q, const struct group_plan *a, const struct group_plan *b, int vc, uint64_t *acc) {
    const uint32_t D = a->n_bins * b->n_bins;
    void *out_dev[HIP_MAX_SHARDS];
    const struct shard_reduce r = { .what = "group pair bins", .bytes = bins_bytes(D, vc), .fused = pair_fused_call,
                                    .list = pair_list_call, .combine = group_combine };
    return shard_reduce(q, a->fused, &r, out_dev, &(struct pair_call){ { acc, D, vc }, a, b, out_dev });
}

/* The shards' compact runs (the run format of pqps_group_pair_sort: host[s] holds runs[s] entries per field, ascending by
 * key) merged by key into pr: counts and sums added, min / max images taken. */
static int runs_merge(int n_shards, uint64_t *const *host, const uint64_t *runs, bool valued, struct pair_rows *pr) {
    uint64_t at[HIP_MAX_SHARDS] = { 0 }, all = 0;
    for (int s = 0; s < n_shards; s++) all += runs[s];
    int rc = pair_rows_alloc(pr, all, valued);
    while (rc == 0) {                                                    /* k-way merge by key */
        int best = -1;
        for (int s = 0; s < n_shards; s++)
            if (at[s] < runs[s] && (best < 0 || host[s][at[s]] < host[best][at[best]])) best = s;
        if (best < 0) break;
        const uint64_t *h = host[best], r = runs[best], i = at[best]++;
        uint64_t g = pr->n;
        if (g && pr->key[g - 1] == h[i]) g--;                            /* the key of another shard's run */
        else { pr->n++; pr->key[g] = h[i]; if (valued) pr->mn[g] = UINT64_MAX; }
        pr->cnt[g] += h[r + i];
        if (valued) {
            pr->sum[g] += h[2 * r + i];
            if (h[3 * r + i] < pr->mn[g]) pr->mn[g] = h[3 * r + i];
            if (h[4 * r + i] > pr->mx[g]) pr->mx[g] = h[4 * r + i];
        }
    }
    return rc;
}

/* One shard's runs from its device to the host: *host = malloc'd, `fields` x n_runs u64 (NULL for no runs); runs_dev is freed. */
static int runs_fetch(pqps_ctx *cs, pqps_ctx *owner, uint64_t *runs_dev, uint64_t n_runs, bool valued, const char *what, uint64_t **host) {
    const size_t bytes = (valued ? 5 : 2) * (size_t)n_runs * 8;
    int rc = 0;
    if (n_runs && !(*host = malloc(bytes))) rc = oom();
    else if (n_runs && pqps_download(cs, *host, runs_dev, bytes, NULL) != PQPS_OK) rc = engine_error(what);
    if (runs_dev) pqps_free(owner, runs_dev);
    return rc;
}

/* The sparse form: the selection, every shard's list sorted and reduced to its runs on its device (pqps_group_pair_sort),
 * the compact runs downloaded and merged by key on the host (runs_merge). */
static int pair_sparse(struct query *q, const struct group_plan *a, const struct group_plan *b, int vc, struct pair_rows *pr) {
    const bool valued = vc >= 0;
    uint64_t *host[HIP_MAX_SHARDS] = { NULL };
    uint64_t runs[HIP_MAX_SHARDS] = { 0 };
    memset(pr, 0, sizeof *pr);
    int rc = query_lists(q);
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        pqps_ctx *cs = lane_copy_ctx(q, s);
        uint64_t *runs_dev = NULL;
        if (q->count[s] == 0) continue;
        if (pqps_group_pair_sort(cs, &sh->col[a->c], a->bin_base, a->n_bins, &sh->col[b->c], b->bin_base, b->n_bins, valued ? &sh->col[vc] : NULL,
                                 sh->n_rows, query_lane(q, s)->ids_dev, q->count[s], (uint32_t)sh->row0, &runs_dev, &runs[s], NULL) != PQPS_OK)
            rc = engine_error("group pair sort");
        if (rc == 0) rc = runs_fetch(cs, sh->ctx, runs_dev, runs[s], valued, "group pair download", &host[s]);
        else if (runs_dev) pqps_free(sh->ctx, runs_dev);
    }
    if (rc == 0) rc = runs_merge(q->n_shards, host, runs, valued, pr);
    for (int s = 0; s < q->n_shards; s++) free(host[s]);
    return rc;
}

static int pair_result_fill(struct hipGroupPairResult *res, const struct hipTable *t, const struct group_plan *gp[2], const struct pair_rows *pr) {
    const size_t n = (size_t)pr->n;
    const bool valued = res->valueColumn >= 0;
    for (int j = 0; j < 2; j++) {
        res->keys[j] = calloc(n + 1, sizeof **res->keys);
        res->keyText[j] = calloc(n + 1, sizeof **res->keyText);
    }
    if (!res->keys[0] || !res->keys[1] || !res->keyText[0] || !res->keyText[1]) return oom();
    if (group_arrays_alloc(n, valued, &res->counts, &res->sums, &res->mins, &res->maxs) != 0) return -1;
    for (size_t g = 0; g < n; g++) {
        const uint32_t bin[2] = { (uint32_t)(pr->key[g] >> 32), (uint32_t)pr->key[g] };
        res->numGroups = (int)g + 1;                                     /* (what freeGroupPairResultHIP frees) */
        for (int j = 0; j < 2; j++) {
            char buf[32];
            res->keyText[j][g] = strdup(group_key(t, gp[j]->c, gp[j]->kind, bin[j], gp[j]->lo, &res->keys[j][g], buf, sizeof buf));
            if (!res->keyText[j][g]) return oom();
        }
        group_arrays_set(res->counts, res->sums, res->mins, res->maxs, g, pr->cnt[g], valued ? pr->sum[g] : 0, valued ? pr->mn[g] : 0,
                         valued ? pr->mx[g] : 0, res->valueKind);
        res->total += (long long)pr->cnt[g];
    }
    return 0;
}

struct hipGroupPairResult *executeQueryGroupPairHIP(struct engineS *engine, const char *groupColumnA, const char *groupColumnB,
                                                    const char *valueColumn, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipGroupPairResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->groupColumn[0] = res->groupColumn[1] = res->groupKind[0] = res->groupKind[1] = res->valueColumn = res->valueKind = -1;
    if (!engine || !engine->record_block || !groupColumnA || !groupColumnB) { fprintf(stderr, "HIP engine: GROUP BY pair without an engine or two columns\n"); return res; }
    const char *names[2] = { groupColumnA, groupColumnB };
    int c[2], v = -1;
    for (int j = 0; j < 2; j++) if ((c[j] = group_column_id("GROUP BY pair", names[j])) < 0) return res;
    if (valueColumn && (v = value_column_id("GROUP BY pair", valueColumn)) < 0) return res;
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: GROUP BY pair is not exchanged across ranks\n"); return res; }
    for (int j = 0; j < 2; j++) { res->groupColumn[j] = c[j]; res->groupKind[j] = k_group_kind[c[j]]; }
    res->valueColumn = v;
    res->valueKind = v >= 0 ? k_group_kind[v] : -1;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    struct group_plan gp[2], none;
    struct pair_rows pr;
    memset(&pr, 0, sizeof pr);
    int rc = query_bind(engine, whereClause, &q);                        /* the WHERE is bound once */
    for (int j = 0; j < 2; j++) {
        const int r = group_plan_column(&q, rc, c[j], names[j], "GROUP BY pair", &gp[j]);
        if (rc == 0) rc = r;
    }
    if (rc == 0 && !gp[0].empty && !gp[1].empty) {
        /* a single-valued column contributes its one key to every pair: the query runs as the one-column form on the other
         * column (as one group when both are single-valued), through the one-column code */
        const struct group_plan *one = gp[0].single && gp[1].single ? NULL : gp[0].single ? &gp[1] : gp[1].single ? &gp[0] : NULL;
        const bool reduced = gp[0].single || gp[1].single;
        const uint64_t D = reduced ? (one ? one->n_bins : 1u) : (uint64_t)gp[0].n_bins * gp[1].n_bins;   /* 64 bits: 65 536 x 65 536 = 2^32 */
        if (!reduced && D > HIP_GROUP_MAX_BINS) rc = pair_sparse(&q, &gp[0], &gp[1], v, &pr);
        else {
            uint64_t *acc = bins_alloc(D, v >= 0);
            if (!acc) rc = -1;
            if (rc == 0 && !reduced) rc = pair_dense(&q, &gp[0], &gp[1], v, acc);
            else if (rc == 0) {
                if (!one) { (void)group_plan_column(&q, 0, -1, NULL, "GROUP BY pair", &none); one = &none; }
                rc = v < 0 ? group_counts(&q, one, acc) : group_bins(&q, one, v, acc);
            }
            /* bin k of a reduced query: (0, k) where A is the single-valued one, (k, 0) otherwise */
            if (rc == 0) rc = pair_rows_from_bins(acc, (uint32_t)D, !reduced ? gp[1].n_bins : gp[0].single ? (uint32_t)D : 1u, v >= 0, &pr);
            free(acc);
        }
    }
    if (rc == 0 && pair_result_fill(res, t, (const struct group_plan *[2]){ &gp[0], &gp[1] }, &pr) == 0) res->success = true;
    pair_rows_free(&pr);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeGroupPairResultHIP(struct hipGroupPairResult *res) {
    if (!res) return;
    for (int j = 0; j < 2; j++) free_group_keys(res->keys[j], res->keyText[j], res->numGroups);
    group_arrays_free(res->counts, res->sums, res->mins, res->maxs);
    free(res);
}

/* ---- the top N groups (include/executeEngine-hip.h) ------------------------------------------------------------------ */

/* Whether a shard's `span` wide bins fit the budget: 4 B a bin, 32 B with a value column; n_bins must fit a u32 count too. */
static bool top_bins_fit(uint64_t span, bool valued) {
    return span <= UINT32_MAX && span * (valued ? 4 * sizeof(uint64_t) : sizeof(uint32_t)) <= HIP_TOP_BINS_BUDGET;
}

struct top_call { const struct group_plan *gp; int vc; bool fit; void **bins_dev; uint64_t **host; uint64_t *runs; };

static int top_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct top_call *a = arg;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const int rc = pqps_filter_group_wide(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, a->vc >= 0 ? &sh->col[a->vc] : NULL, &sh->col[a->gp->c],
                                          a->gp->bin_base, a->gp->n_bins, a->bins_dev[s], stream);
    return rc == PQPS_OK ? 0 : engine_error("wide group filter");
}

/* A shard's bins (filled by the fused launch, or here from its list) compacted on its device; or, without bins (past the
 * budget), its list sorted and reduced.  Either way the shard hands over its runs only. */
static int top_post(struct query *q, int s, pqps_ctx *cs, void *out, void *arg) {
    const struct top_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct hipLane *L = query_lane(q, s);
    const bool valued = a->vc >= 0;
    const pqps_column *vcol = valued ? &sh->col[a->vc] : NULL;
    uint64_t *runs_dev = NULL;
    int rc = 0;
    if (!a->fit) {
        if (pqps_group_sort(cs, &sh->col[gp->c], gp->bin_base, gp->span, vcol, sh->n_rows, L->ids_dev, q->count[s], (uint32_t)sh->row0,
                            &runs_dev, &a->runs[s], NULL) != PQPS_OK)
            rc = engine_error("group sort");
    } else {
        if (!gp->fused && pqps_group_wide_list(cs, vcol, &sh->col[gp->c], sh->n_rows, L->ids_dev, L->count_dev, q->count[s], (uint32_t)sh->row0,
                                               gp->bin_base, gp->n_bins, out, NULL) != PQPS_OK)
            rc = engine_error("wide group list");
        if (rc == 0 && pqps_bins_compact(cs, out, gp->n_bins, valued, &runs_dev, &a->runs[s], NULL) != PQPS_OK) rc = engine_error("bins compaction");
    }
    if (rc == 0) return runs_fetch(cs, sh->ctx, runs_dev, a->runs[s], valued, "group runs download", &a->host[s]);
    if (runs_dev) pqps_free(sh->ctx, runs_dev);
    return rc;
}

/* The groups of a column of more than HIP_GROUP_MAX_BINS bins, merged over the shards into pr (key = the bin), through
 * shard_reduce with top_post as its post step.  Fused (a single-pass scan-mode WHERE whose bins fit the budget): one
 * pqps_filter_group_wide launch per shard.  Otherwise the selection, and per shard the wide bins over its list where they
 * fit the budget, the sort form where they do not (measured, DESIGN.md 7l: inside the budget the wide bins win down to a
 * list of 5 000 rows against 10^7 bins). */
static int top_wide(struct query *q, const struct group_plan *gp, int vc, struct pair_rows *pr) {
    const bool valued = vc >= 0, fit = top_bins_fit(gp->span, valued);
    void *bins_dev[HIP_MAX_SHARDS];
    uint64_t *host[HIP_MAX_SHARDS] = { NULL };
    uint64_t runs[HIP_MAX_SHARDS] = { 0 };
    const struct shard_reduce r = { .what = "wide group bins", .bytes = fit ? bins_bytes(gp->n_bins, vc) : 0, .fused = top_fused_call, .post = top_post };
    memset(pr, 0, sizeof *pr);
    int rc = shard_reduce(q, gp->fused && fit, &r, bins_dev, &(struct top_call){ gp, vc, fit, bins_dev, host, runs });
    if (rc == 0) rc = runs_merge(q->n_shards, host, runs, valued, pr);
    for (int s = 0; s < q->n_shards; s++) free(host[s]);
    return rc;
}

/* The listed groups into the result: pr holds every group (ascending by bin), order[0 .. n) the indices of the listed ones. */
static int top_result_fill(struct hipGroupTopResult *res, const struct hipTable *t, const struct group_plan *gp, const struct pair_rows *pr,
                           const uint64_t *order, size_t n) {
    const bool valued = res->valueColumn >= 0;
    res->keys = calloc(n + 1, sizeof *res->keys);
    res->keyText = calloc(n + 1, sizeof *res->keyText);
    if (!res->keys || !res->keyText) return oom();
    if (group_arrays_alloc(n, valued, &res->counts, &res->sums, &res->mins, &res->maxs) != 0) return -1;
    for (size_t g = 0; g < n; g++) {
        const uint64_t i = order[g];
        char buf[32];
        if (!(res->keyText[g] = strdup(group_key(t, gp->c, gp->kind, (uint32_t)pr->key[i], gp->lo, &res->keys[g], buf, sizeof buf)))) return oom();
        res->numGroups = (int)g + 1;                                     /* (what freeGroupTopResultHIP frees) */
        group_arrays_set(res->counts, res->sums, res->mins, res->maxs, g, pr->cnt[i], valued ? pr->sum[i] : 0, valued ? pr->mn[i] : 0,
                         valued ? pr->mx[i] : 0, res->valueKind);
    }
    return 0;
}

struct hipGroupTopResult *executeQueryGroupTopHIP(struct engineS *engine, const char *groupColumn, const char *valueColumn, int orderBy,
                                                  bool descending, long long limit, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipGroupTopResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->groupColumn = res->groupKind = res->valueColumn = res->valueKind = -1;
    res->orderBy = orderBy;
    res->descending = descending;
    res->limit = limit;
    if (!engine || !engine->record_block || !groupColumn) { fprintf(stderr, "HIP engine: top groups without an engine or a column\n"); return res; }
    const int c = group_column_id("top groups", groupColumn);
    if (c < 0) return res;
    int v = -1;
    if (valueColumn && (v = value_column_id("top groups", valueColumn)) < 0) return res;
    if (orderBy < HIPTOP_BY_KEY || orderBy > HIPTOP_BY_MAX) { fprintf(stderr, "HIP engine: top groups: order %d is none of HIPTOP_BY_*\n", orderBy); return res; }
    if (orderBy >= HIPTOP_BY_SUM && v < 0) { fprintf(stderr, "HIP engine: top groups: ordering by SUM / MIN / MAX needs a value column\n"); return res; }
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: top groups are not exchanged across ranks\n"); return res; }
    res->groupColumn = c;
    res->groupKind = k_group_kind[c];
    res->valueColumn = v;
    res->valueKind = v >= 0 ? k_group_kind[v] : -1;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    struct group_plan gp;
    struct pair_rows pr;
    uint64_t *order = NULL;
    long long listed = 0;
    memset(&pr, 0, sizeof pr);
    int rc = group_plan_column_span(&q, query_bind(engine, whereClause, &q), c, groupColumn, "top groups", true, &gp);
    if (rc == 0 && !gp.empty) {
        if (gp.span > HIP_GROUP_MAX_BINS && !gp.single) rc = top_wide(&q, &gp, v, &pr);
        else {                                                           /* the dense bins of the other grouped queries */
            uint64_t *acc = bins_alloc(gp.n_bins, v >= 0);
            if (!acc) rc = -1;
            if (rc == 0) rc = v < 0 ? group_counts(&q, &gp, acc) : group_bins(&q, &gp, v, acc);
            if (rc == 0) rc = pair_rows_from_bins(acc, gp.n_bins, UINT32_MAX, v >= 0, &pr);   /* n_b past every bin: key = bin */
            free(acc);
        }
    }
    for (uint64_t g = 0; g < pr.n; g++) res->total += (long long)pr.cnt[g];
    res->groupsTotal = (long long)pr.n;
    const uint64_t listing = limit > 0 && (uint64_t)limit < pr.n ? (uint64_t)limit : pr.n;
    if (rc == 0 && listing > INT_MAX) {                                  /* numGroups is an int */
        fprintf(stderr, "HIP engine: top groups: %llu groups to list, more than %d: give a LIMIT\n", (unsigned long long)listing, INT_MAX);
        rc = -1;
    }
    if (rc == 0 && pr.n && !(order = malloc((size_t)pr.n * sizeof *order))) rc = oom();
    if (rc == 0 && (listed = hipGroupTopOrder(pr.key, pr.cnt, pr.sum, pr.mn, pr.mx, pr.n, res->valueKind, orderBy, descending, limit, order)) < 0) rc = -1;
    if (rc == 0 && top_result_fill(res, t, &gp, &pr, order, (size_t)listed) == 0) res->success = true;
    free(order);
    pair_rows_free(&pr);
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeGroupTopResultHIP(struct hipGroupTopResult *res) {
    if (!res) return;
    free_group_keys(res->keys, res->keyText, res->numGroups);
    group_arrays_free(res->counts, res->sums, res->mins, res->maxs);
    free(res);
}

/* ---- value sets: IN (SELECT column ... [GROUP BY column HAVING agg op n]) (include/executeEngine-hip.h) ----------------- */

/* How one set is built on every shard: the bins of B (gp) and what is made of them. */
struct set_plan {
    const struct group_plan *gp;
    bool having;                         /* bins, then pqps_bins_having; otherwise the presence bitmap of the distinct calls */
    bool wide;                           /* more than HIP_GROUP_MAX_BINS bins: the wide bins                                 */
    int vc;                              /* the value column of the bins, -1: u32 counts                                     */
    struct hipHaving hv;
    size_t words;                        /* u32 words of the bitmap                                                          */
    void **work;                         /* shard s: its bins (having), or the words [total][distinct]                       */
    uint32_t **bitmap;                   /* shard s: the set's bitmap                                                        */
    bool *filled;                        /* shard s: a launch wrote work[s] / bitmap[s]                                      */
};

static int set_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct set_plan *p = arg;
    const struct group_plan *gp = p->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const pqps_column *vcol = p->vc >= 0 ? &sh->col[p->vc] : NULL;
    int rc;
    if (!p->having)
        rc = pqps_filter_distinct(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &gp->gcol[s], gp->bin_base, gp->n_bins, NULL, 0, 1,
                                  p->bitmap[s], (uint64_t *)p->work[s], q->n_shards > 1 ? NULL : (uint64_t *)p->work[s] + 1, stream);
    else if (p->wide)
        rc = pqps_filter_group_wide(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, vcol, &gp->gcol[s], gp->bin_base, gp->n_bins, p->work[s], stream);
    else if (vcol)
        rc = pqps_filter_aggregate(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, vcol, gp->single ? NULL : &gp->gcol[s], gp->bin_base,
                                   gp->n_bins, p->work[s], stream);
    else
        rc = pqps_filter_group(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, &gp->gcol[s], gp->bin_base, gp->n_bins, p->work[s], stream);
    if (rc != PQPS_OK) return engine_error("value set scan");
    p->filled[s] = true;
    return 0;
}

/* the same over shard s's list (query_lists), on the lane's copy context */
static int set_list_call(struct query *q, int s, const struct set_plan *p) {
    const struct group_plan *gp = p->gp;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct hipLane *L = query_lane(q, s);
    pqps_ctx *cs = lane_copy_ctx(q, s);
    const pqps_column *vcol = p->vc >= 0 ? &sh->col[p->vc] : NULL;
    const uint32_t row0 = (uint32_t)sh->row0;
    int rc;
    if (!p->having)
        rc = pqps_distinct_list(cs, &gp->gcol[s], gp->bin_base, gp->n_bins, NULL, 0, 1, sh->n_rows, L->ids_dev, L->count_dev, q->count[s], row0,
                                p->bitmap[s], q->n_shards > 1 ? NULL : (uint64_t *)p->work[s] + 1, NULL);
    else if (p->wide)
        rc = pqps_group_wide_list(cs, vcol, &gp->gcol[s], sh->n_rows, L->ids_dev, L->count_dev, q->count[s], row0, gp->bin_base, gp->n_bins, p->work[s], NULL);
    else if (vcol)
        rc = pqps_aggregate_list(cs, vcol, gp->single ? NULL : &gp->gcol[s], sh->n_rows, L->ids_dev, L->count_dev, q->count[s], row0, gp->bin_base,
                                 gp->n_bins, p->work[s], NULL);
    else
        rc = pqps_group_list(cs, &gp->gcol[s], sh->n_rows, L->ids_dev, L->count_dev, q->count[s], row0, gp->bin_base, gp->n_bins, p->work[s], NULL);
    if (rc != PQPS_OK) return engine_error("value set list");
    p->filled[s] = true;
    return 0;
}

/* The HAVING of bins on shard 0's device into the set's bitmap there: out[0] = the rows the bins hold, out[1] = the members.
 * This is the only place the comparison is made. */
static int set_having(pqps_ctx *c0, const struct set_plan *p, const void *bins, uint32_t *bitmap, uint64_t *cnt_dev, uint64_t out[2]) {
    const int valued = p->vc >= 0;
    if (pqps_bins_rows(c0, bins, p->gp->n_bins, valued, cnt_dev, NULL) != PQPS_OK ||
        pqps_bins_having(c0, bins, p->gp->n_bins, valued, p->hv.field, p->hv.op, p->hv.constant, p->hv.value_signed, bitmap, cnt_dev + 1, NULL) != PQPS_OK ||
        pqps_download(c0, out, cnt_dev, 2 * sizeof *out, NULL) != PQPS_OK)
        return engine_error("HAVING");
    return 0;
}

/* Builds the bitmap of vs on every shard (vs->bitmap[s]; on failure none is left) and fills vs->rows / vs->members. */
static int set_build(struct query *q, struct set_plan *p, struct value_set *vs) {
    const struct group_plan *gp = p->gp;
    const bool valued = p->vc >= 0, multi = q->n_shards > 1;
    const uint32_t n_bins = gp->n_bins;
    const size_t bm_bytes = (p->words + (p->words & 1u)) * sizeof(uint32_t);       /* whole 8-byte stores of pqps_bins_having */
    const size_t work_bytes = p->having ? bins_bytes(n_bins, p->vc) : 2 * sizeof(uint64_t);
    void *work[HIP_MAX_SHARDS] = { NULL };
    bool filled[HIP_MAX_SHARDS] = { false };
    uint64_t *cnt_dev = NULL, out[2] = { 0, 0 };
    void *host = NULL;
    int rc = 0;
    p->work = work; p->bitmap = vs->bitmap; p->filled = filled;
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        if (pqps_malloc(sh->ctx, bm_bytes, (void **)&vs->bitmap[s]) != PQPS_OK || pqps_malloc(sh->ctx, work_bytes, &work[s]) != PQPS_OK)
            rc = engine_error("value set buffers");
    }
    if (rc == 0 && pqps_malloc(hipTableShard(q->t, 0)->ctx, 2 * sizeof(uint64_t), (void **)&cnt_dev) != PQPS_OK) rc = engine_error("value set buffers");
    if (rc == 0 && gp->fused) rc = fused_issue(q, set_fused_call, p);
    else if (rc == 0) {
        rc = query_lists(q);
        for (int s = 0; s < q->n_shards && rc == 0; s++) if (q->count[s]) rc = set_list_call(q, s, p);
    }
    pqps_ctx *c0 = lane_copy_ctx(q, 0);
    if (rc == 0 && !multi) {
        /* one shard: neither bins nor bitmap leave the device, the two counts do */
        if (!filled[0]) {
            if (pqps_memset(c0, vs->bitmap[0], 0, bm_bytes, NULL) != PQPS_OK || pqps_ctx_sync(c0, NULL) != PQPS_OK) rc = engine_error("value set bitmap");
        } else if (p->having) rc = set_having(c0, p, work[0], vs->bitmap[0], cnt_dev, out);
        else {
            if (pqps_download(c0, out, work[0], sizeof out, NULL) != PQPS_OK) rc = engine_error("value set counts");
            if (!gp->fused) out[0] = q->total;                              /* (the list form leaves no total) */
        }
    } else if (rc == 0 && !p->having) {
        /* several shards: the OR of their bitmaps, placed on every shard; the popcount on shard 0 */
        uint32_t *merged = calloc(p->words, sizeof *merged);
        host = malloc(p->words * sizeof(uint32_t));
        if (!merged || !host) rc = oom();
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            uint64_t n = 0;
            if (!filled[s]) continue;
            pqps_ctx *cs = lane_copy_ctx(q, s);
            if (pqps_download(cs, host, vs->bitmap[s], p->words * sizeof(uint32_t), NULL) != PQPS_OK ||
                (gp->fused && pqps_download(cs, &n, work[s], sizeof n, NULL) != PQPS_OK)) { rc = engine_error("value set download"); break; }
            for (size_t i = 0; i < p->words; i++) merged[i] |= ((const uint32_t *)host)[i];
            out[0] += n;
        }
        if (rc == 0 && !gp->fused) out[0] = q->total;
        for (int s = 0; s < q->n_shards && rc == 0; s++)
            if (pqps_upload(lane_copy_ctx(q, s), vs->bitmap[s], merged, p->words * sizeof(uint32_t), NULL) != PQPS_OK) rc = engine_error("value set upload");
        if (rc == 0 && (pqps_distinct_count(c0, vs->bitmap[0], n_bins, 1, cnt_dev + 1, NULL) != PQPS_OK ||
                        pqps_download(c0, &out[1], cnt_dev + 1, sizeof out[1], NULL) != PQPS_OK))
            rc = engine_error("value set popcount");
        free(merged);
    } else if (rc == 0) {
        /* several shards: their bins combined as the grouped queries combine them, HAVING on shard 0, the bitmap to the others */
        uint64_t *acc = bins_alloc(n_bins, valued);
        host = malloc(work_bytes > p->words * sizeof(uint32_t) ? work_bytes : p->words * sizeof(uint32_t));
        if (!acc) rc = -1;
        else if (!host) rc = oom();
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            if (!filled[s]) continue;
            if (pqps_download(lane_copy_ctx(q, s), host, work[s], work_bytes, NULL) != PQPS_OK) rc = engine_error("value set download");
            else group_combine(&(struct bins_acc){ acc, n_bins, p->vc }, host);
        }
        if (rc == 0 && !valued) for (uint32_t k = 0; k < n_bins; k++) ((uint32_t *)host)[k] = (uint32_t)acc[k];   /* (a table has fewer than 2^31 rows) */
        if (rc == 0 && pqps_upload(c0, work[0], valued ? (const void *)acc : host, work_bytes, NULL) != PQPS_OK) rc = engine_error("value set upload");
        if (rc == 0) rc = set_having(c0, p, work[0], vs->bitmap[0], cnt_dev, out);
        if (rc == 0 && pqps_download(c0, host, vs->bitmap[0], p->words * sizeof(uint32_t), NULL) != PQPS_OK) rc = engine_error("value set download");
        for (int s = 1; s < q->n_shards && rc == 0; s++)
            if (pqps_upload(lane_copy_ctx(q, s), vs->bitmap[s], host, p->words * sizeof(uint32_t), NULL) != PQPS_OK) rc = engine_error("value set upload");
        free(acc);
    }
    free(host);
    for (int s = 0; s < q->n_shards; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        if (work[s]) pqps_free(sh->ctx, work[s]);
        if (rc != 0 && vs->bitmap[s]) { pqps_free(sh->ctx, vs->bitmap[s]); vs->bitmap[s] = NULL; }
    }
    if (cnt_dev) pqps_free(hipTableShard(q->t, 0)->ctx, cnt_dev);
    vs->rows = out[0];
    vs->members = out[1];
    return rc;
}

/* Enters vs into the table's registry under a new id; -1 (reason on stderr) when HIP_MAX_VALUE_SETS sets are there already. */
static int value_set_register(struct hipTable *t, struct value_set *vs) {
    int rc = -1;
    pthread_mutex_lock(&g_sets_lock);
    if (!t->sets && (t->sets = calloc(1, sizeof *t->sets))) t->sets->next_id = 1;
    for (int i = 0; t->sets && i < HIP_MAX_VALUE_SETS && rc != 0; i++) {
        if (t->sets->set[i].id) continue;
        vs->id = t->sets->next_id++;
        if (t->sets->next_id == 0) t->sets->next_id = 1;
        vs->version = t->sets->version;
        t->sets->set[i] = *vs;
        rc = 0;
    }
    pthread_mutex_unlock(&g_sets_lock);
    if (rc != 0) fprintf(stderr, "HIP engine: value set: %d sets are alive already (free one first)\n", HIP_MAX_VALUE_SETS);
    return rc;
}

static bool value_sets_full(const struct hipTable *t) {
    int n = 0;
    pthread_mutex_lock(&g_sets_lock);
    for (int i = 0; t->sets && i < HIP_MAX_VALUE_SETS; i++) n += t->sets->set[i].id != 0;
    pthread_mutex_unlock(&g_sets_lock);
    return n >= HIP_MAX_VALUE_SETS;
}

struct hipValueSet *hipEngineCreateSetHIP(struct engineS *engine, const char *column, struct whereClauseS *whereClause,
                                          const struct hipSetHaving *having) {
    const double t0 = now_seconds();
    struct hipValueSet *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->column = res->kind = -1;
    if (!engine || !engine->record_block || !column) { fprintf(stderr, "HIP engine: value set without an engine or a column\n"); return res; }
    const int c = hipColumnId(column);
    if (c < 0) { fprintf(stderr, "HIP engine: value set: unknown column '%s'\n", column); return res; }
    if (c == HIPCOL_COMMAND_ID || c == HIPCOL_SUDO_USED) {
        fprintf(stderr, "HIP engine: value set: %s takes no value set (sudo_used never needs one, command_id is a follow-up: the list form)\n", column);
        return res;
    }
    struct set_plan p;
    memset(&p, 0, sizeof p);
    p.vc = -1;
    if (having) {
        int v = -1;
        if (having->aggregate < HIPTOP_BY_COUNT || having->aggregate > HIPTOP_BY_MAX) {
            fprintf(stderr, "HIP engine: value set: HAVING aggregate %d is none of HIPTOP_BY_COUNT .. HIPTOP_BY_MAX\n", having->aggregate);
            return res;
        }
        if (having->aggregate != HIPTOP_BY_COUNT) {
            if (!having->valueColumn) { fprintf(stderr, "HIP engine: value set: HAVING SUM / MIN / MAX needs a value column\n"); return res; }
            if ((v = value_column_id("value set", having->valueColumn)) < 0) return res;
        }
        if (hipCompileHaving(having->aggregate, v >= 0 ? k_group_kind[v] : -1, having->op, having->constant, &p.hv) != 0) return res;
        p.having = true;
        p.vc = v;
    }
    struct hipTable *t = engine->record_block;
    if (t->xch) { fprintf(stderr, "HIP engine: value sets are not made on an engine joined across ranks\n"); return res; }
    if (value_sets_full(t)) { fprintf(stderr, "HIP engine: value set: %d sets are alive already (free one first)\n", HIP_MAX_VALUE_SETS); return res; }
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    struct group_plan gp;
    struct value_set vs;
    memset(&vs, 0, sizeof vs);
    /* scan semantics: the WHERE is bound without index probes, every inner row counts once */
    int rc = bind_where(t, whereClause, &q.plan);
    q.have_plan = rc == 0;
    rc = group_plan_column_span(&q, rc, c, column, "value set", true, &gp);
    if (rc == 0 && !gp.empty) {
        if (gp.single) {
            /* a single-valued string column has no buffer to group by: one bin over every inner row, `COUNT(*) != 0` without a HAVING */
            if (!p.having) p.hv = (struct hipHaving){ PQPS_HAVING_COUNT, PQPS_HAVING_NE, 0, 0 };
            p.having = true;
            if (p.vc < 0) p.vc = HIPCOL_COMMAND_ID;
        }
        p.wide = gp.span > HIP_GROUP_MAX_BINS;
        if (!p.having && gp.span > PQPS_MEMBER_MAX_BITS) {
            fprintf(stderr, "HIP engine: value set: %s spans %llu values, more than the %llu a set's bitmap takes\n", column,
                    (unsigned long long)gp.span, (unsigned long long)PQPS_MEMBER_MAX_BITS);
            rc = -1;
        } else if (p.having && p.wide && !top_bins_fit(gp.span, p.vc >= 0)) {
            fprintf(stderr, "HIP engine: value set: the %llu bins of %s (%d bytes each) do not fit the budget of %llu bytes\n",
                    (unsigned long long)gp.span, column, p.vc >= 0 ? 32 : 4, (unsigned long long)HIP_TOP_BINS_BUDGET);
            rc = -1;
        }
    }
    vs.column = c;
    vs.kind = k_group_kind[c];
    if (rc == 0 && !gp.empty) {
        p.gp = &gp;
        p.words = ((size_t)gp.n_bins + 31) / 32;
        vs.base = gp.bin_base;
        vs.lo = gp.lo;
        vs.n_bits = gp.n_bins;
        rc = set_build(&q, &p, &vs);
    }
    if (rc == 0 && value_set_register(t, &vs) != 0) {
        pthread_mutex_lock(&g_sets_lock);
        value_set_release(t, &vs);
        pthread_mutex_unlock(&g_sets_lock);
        rc = -1;
    }
    query_close(&q);
    if (rc == 0) {
        res->success = true;
        res->id = vs.id;
        res->column = c;
        res->kind = vs.kind;
        res->members = vs.members;
        res->rows = vs.rows;
    }
    res->queryTime = now_seconds() - t0;
    return res;
}

struct hipSetKeys *hipEngineSetKeysHIP(struct engineS *engine, const struct hipValueSet *set) {
    struct hipSetKeys *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    res->column = res->kind = -1;
    if (!engine || !engine->record_block || !set || !set->success) { fprintf(stderr, "HIP engine: set keys without an engine or a set\n"); return res; }
    struct hipTable *t = engine->record_block;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    struct value_set vs;
    pthread_mutex_lock(&g_sets_lock);
    const struct value_set *found = value_set_find(t, set->id);
    if (found) vs = *found;
    pthread_mutex_unlock(&g_sets_lock);
    int rc = 0;
    if (!found || vs.stale) {
        fprintf(stderr, "HIP engine: set keys: value set %u %s\n", set->id, found ? "is stale: the table was written after it was made" : "does not exist (freed)");
        rc = -1;
    }
    const size_t words = rc == 0 && vs.members ? (size_t)((vs.n_bits + 31) / 32) : 0;
    uint32_t *bits = NULL;
    if (rc == 0 && vs.members > INT_MAX) { fprintf(stderr, "HIP engine: set keys: more than %d keys\n", INT_MAX); rc = -1; }
    if (rc == 0 && words && !(bits = malloc(words * sizeof *bits))) rc = oom();
    if (rc == 0 && words && pqps_download(lane_copy_ctx(&q, 0), bits, vs.bitmap[0], words * sizeof *bits, NULL) != PQPS_OK) rc = engine_error("set keys download");
    if (rc == 0) {
        res->column = vs.column;
        res->kind = vs.kind;
        res->keys = calloc((size_t)vs.members + 1, sizeof *res->keys);
        res->keyText = calloc((size_t)vs.members + 1, sizeof *res->keyText);
        if (!res->keys || !res->keyText) rc = oom();
    }
    for (uint64_t k = 0; rc == 0 && words && k < vs.n_bits; k++) {
        if (!((bits[k >> 5] >> (k & 31)) & 1u)) continue;
        char buf[32];
        if ((uint64_t)res->numKeys >= vs.members) { fprintf(stderr, "HIP engine: set keys: the bitmap holds more than its %llu members\n", (unsigned long long)vs.members); rc = -1; break; }
        if (!(res->keyText[res->numKeys] = strdup(group_key(t, vs.column, vs.kind, (uint32_t)k, vs.lo, &res->keys[res->numKeys], buf, sizeof buf)))) rc = oom();
        else res->numKeys++;
    }
    free(bits);
    query_close(&q);
    res->success = rc == 0;
    return res;
}

void freeSetKeysHIP(struct hipSetKeys *keys) {
    if (!keys) return;
    free_group_keys(keys->keys, keys->keyText, keys->numKeys);
    free(keys);
}

int hipEngineFreeSetHIP(struct engineS *engine, struct hipValueSet *set) {
    if (!set) return 0;
    if (set->success && set->id && engine && engine->record_block) {
        struct hipTable *t = engine->record_block;
        if (hipTableLockExclusive(t) != 0) return -1;                    /* a thread that holds a ticket: refused, nothing freed */
        pthread_mutex_lock(&g_sets_lock);
        struct value_set *vs = value_set_find(t, set->id);
        if (vs) { value_set_release(t, vs); memset(vs, 0, sizeof *vs); }
        pthread_mutex_unlock(&g_sets_lock);
        hipTableUnlockExclusive(t);
    }
    free(set);
    return 0;
}

/* ---- projection ------------------------------------------------------------------ */

/* get_attribute_string_value, S:216-248, with the column resolved once per query
 * instead of one strcmp chain per cell. */
static char *cell_text(const record *r, const FieldInfo *fi) {
    char buf[32];
    if (!fi) return strdup("NULL");                            /* unknown column, S:244 */
    const char *p = (const char *)r + fi->offset;
    switch (fi->type) {
    case FIELD_UINT64: snprintf(buf, sizeof buf, "%llu", *(const unsigned long long *)p); return strdup(buf);
    case FIELD_INT: snprintf(buf, sizeof buf, "%d", *(const int *)p); return strdup(buf);
    case FIELD_BOOL: return strdup(*(const bool *)p ? "true" : "false");
    default: return strdup(p);
    }
}

static const char *const k_all_columns[12] = {
    "command_id", "raw_command", "base_command", "shell_type", "exit_code", "timestamp",
    "sudo_used", "working_directory", "user_id", "user_name", "host_name", "risk_level"
};

/* projection of a row range (one task per thread; malloc is thread safe) */
struct project_job {
    struct engineS *engine; const unsigned int *ids; char ***data; const FieldInfo *const *cols; int n_cols;
    size_t begin, end;
};

static void *project_rows(void *arg) {
    struct project_job *j = arg;
    for (size_t i = j->begin; i < j->end; i++) {
        const record *r = j->engine->all_records[j->ids[i]];
        char **row = malloc((size_t)j->n_cols * sizeof(char *));
        if (!row) { perror("Failed to allocate result row"); exit(EXIT_FAILURE); }
        for (int c = 0; c < j->n_cols; c++) row[c] = cell_text(r, j->cols[c]);
        j->data[i] = row;
    }
    return NULL;
}

static struct resultSetS *select_device_only(struct engineS *engine, const char **selectItems, int numSelectItems, struct whereClauseS *whereClause);

struct resultSetS *executeQuerySelectHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                         const char *tableName, struct whereClauseS *whereClause) {
    (void)tableName;                                   /* never checked by the reference either */
    if (engine && engine->record_block && ((struct hipTable *)engine->record_block)->device_only)
        return select_device_only(engine, selectItems, numSelectItems, whereClause);
    struct resultSetS *rs = malloc(sizeof *rs);
    if (!rs) { perror("Failed to allocate memory for result set"); exit(EXIT_FAILURE); }
    memset(rs, 0, sizeof *rs);

    unsigned int *ids = NULL;
    double qtime = 0.0;
    if (!engine || !engine->record_block) { rs->success = false; return rs; }
    const double t_sel = now_seconds();
    struct hipQueryTicket *tk = executeQuerySelectAsyncHIP(engine, whereClause);    /* holds the table shared: the projection below reads the host rows */
    const long long count = tk ? ticket_download_ids(tk, &ids) : -1;
    if (tk) ticket_release_lane(tk);                   /* the device side is done: the lane serves the next query while this one builds strings */
    qtime = now_seconds() - t_sel;
    if (count < 0) {                                   /* reason already on stderr */
        releaseQueryHIP(tk);
        rs->success = false;
        return rs;
    }

    rs->numRecords = (int)count;
    if (selectItems == NULL || numSelectItems == 0) {  /* SELECT *, S:490-492 */
        selectItems = (const char **)k_all_columns;
        rs->numColumns = 12;
    } else {
        rs->numColumns = numSelectItems;
    }
    rs->columnNames = malloc((size_t)rs->numColumns * sizeof(char *));
    const FieldInfo **cols = malloc((size_t)(rs->numColumns > 0 ? rs->numColumns : 1) * sizeof *cols);
    for (int j = 0; j < rs->numColumns; j++) {
        rs->columnNames[j] = strdup(selectItems[j]);
        cols[j] = get_field_info(selectItems[j]);
    }
    rs->data = malloc((count ? (size_t)count : 1) * sizeof(char **));

    /* S:504-515 -- rows x columns heap strings, the result-set contract of the reference */
    const double t_proj = now_seconds();
    int nt = 1;
    if (count >= 8192) {
        const char *env = getenv("PQPS_HOST_THREADS");
        long cpus = env ? atol(env) : sysconf(_SC_NPROCESSORS_ONLN);
        nt = cpus < 1 ? 1 : (cpus > 16 ? 16 : (int)cpus);
    }
    struct project_job job[16];
    pthread_t tid[16];
    for (int k = 0; k < nt; k++) {
        job[k] = (struct project_job){ engine, ids, rs->data, cols, rs->numColumns,
                                       (size_t)count * (size_t)k / (size_t)nt, (size_t)count * (size_t)(k + 1) / (size_t)nt };
        if (nt == 1 || pthread_create(&tid[k], NULL, project_rows, &job[k]) != 0) { project_rows(&job[k]); tid[k] = 0; }
    }
    for (int k = 0; k < nt; k++) if (nt > 1 && tid[k]) pthread_join(tid[k], NULL);
    releaseQueryHIP(tk);
    TRACE("SELECT: %lld rows x %d columns, selection %.3f ms, projection %.3f ms (%d threads)\n", count, rs->numColumns,
          qtime * 1e3, (now_seconds() - t_proj) * 1e3, nt);
    free(cols);
    free(ids);
    rs->columnTypes = calloc((size_t)rs->numColumns, sizeof(FieldType));   /* placeholder, S:524-525 */
    rs->queryTime = qtime;
    rs->success = true;
    return rs;
}

/* ---- columnar SELECT ------------------------------------------------------------------------------- */

/* Dictionary codes of a result column become self-contained: the codes are widened to u32 and re-numbered
 * 0..k-1 over the k distinct values the result holds (still ascending in strcmp order), and the result owns a
 * copy of those k strings -- it stays valid whatever INSERT / DELETE / destroy later do to the engine. */
static int own_dictionary(struct hipColumnarResult *res, int j, const struct hipDictionary *d, uint32_t w, uint64_t count) {
    void *raw = res->values[j];
    uint32_t *wide = w == 4 ? raw : malloc(count * sizeof *wide);
    uint32_t *local = calloc((size_t)(d->count > 0 ? d->count : 1), sizeof *local);
    if (!wide || !local) { if (wide != raw) free(wide); free(local); fprintf(stderr, "HIP engine: out of memory for the result set\n"); return -1; }
    if (w == 1) for (uint64_t i = 0; i < count; i++) wide[i] = ((const uint8_t *)raw)[i];
    else if (w == 2) for (uint64_t i = 0; i < count; i++) wide[i] = ((const uint16_t *)raw)[i];
    if (wide != raw) { free(raw); res->values[j] = wide; }
    for (uint64_t i = 0; i < count; i++) local[wide[i]] = 1;
    int k = 0;
    for (int v = 0; v < d->count; v++) if (local[v]) k++;
    char **values = malloc((size_t)(k ? k : 1) * sizeof *values);
    if (!values) { free(local); fprintf(stderr, "HIP engine: out of memory for the result set\n"); return -1; }
    k = 0;
    for (int v = 0; v < d->count; v++) {
        if (!local[v]) continue;
        values[k] = strdup(d->values[v]);
        if (!values[k]) {                                               /* hand over what exists: freeColumnarResultHIP frees it */
            free(local);
            res->dictionaries[j] = (const char *const *)values;
            res->dictionarySizes[j] = k;
            fprintf(stderr, "HIP engine: out of memory for the result set\n");
            return -1;
        }
        local[v] = (uint32_t)k++;
    }
    for (uint64_t i = 0; i < count; i++) wide[i] = local[wide[i]];
    free(local);
    res->dictionaries[j] = (const char *const *)values;
    res->dictionarySizes[j] = k;
    return 0;
}

/* Device gather of one column for the selected rows of every shard, into `raw` (result order).  `scattered`: the
 * shards' rows are interleaved in the result (index mode over several shards): shard s's k-th row goes to sub_pos[s][k]. */
static int project_column(struct query *q, int c, void *const *gathered, bool scattered, unsigned int *const *sub_pos, char *raw, char *tmp) {
    struct hipTable *t = q->t;
    const uint32_t w = t->col[c].width;
    uint64_t at = 0;
    for (int s = 0; s < q->n_shards; s++) {
        struct hipTable *sh = hipTableShard(t, s);
        struct hipLane *L = query_lane(q, s);
        pqps_ctx *cs = lane_copy_ctx(q, s);
        const uint64_t k = q->count[s];
        if (k == 0) continue;
        TRY(pqps_project_column(cs, &sh->col[c], L->ids_dev, L->count_dev, k, (uint32_t)sh->row0, gathered[s], NULL), "device projection");
        if (!scattered) {
            TRY(pqps_download(cs, raw + at * w, gathered[s], k * w, NULL), "projection download");
        } else {
            TRY(pqps_download(cs, tmp, gathered[s], k * w, NULL), "projection download");
            for (uint64_t i = 0; i < k; i++) memcpy(raw + (size_t)sub_pos[s][i] * w, tmp + i * w, w);
        }
        at += k;
    }
    return 0;
}

/* The columns of a columnar result for the `count` rows in the query's lanes (q->count[s] rows of shard s; `scattered`,
 * sub_pos and tmp as project_column's). */
static int project_result(struct query *q, const char **selectItems, int numSelectItems, uint64_t count, bool scattered,
                          unsigned int *const *sub_pos, char *tmp, struct hipColumnarResult *res) {
    struct hipTable *t = q->t;
    struct hipSchema schema;
    hipSchemaOfTable(t, &schema);
    void *gathered[HIP_MAX_SHARDS];
    memset(gathered, 0, sizeof gathered);
    int rc = 0;
    for (int s = 0; s < q->n_shards && rc == 0; s++)
        if (q->count[s] && pqps_malloc(hipTableShard(t, s)->ctx, q->count[s] * 8, &gathered[s]) != PQPS_OK) rc = engine_error("projection buffer");
    for (int j = 0; j < numSelectItems && rc == 0; j++) {
        res->columnNames[j] = strdup(selectItems[j]);
        const int c = hipColumnId(selectItems[j]);
        res->columnKinds[j] = c < 0 ? -1 : schema.col[c].kind;
        if (c < 0 || count == 0) continue;
        const uint32_t w = t->col[c].width;
        if (w == 0) {                                                    /* a single-valued string column: every row carries code 0 */
            res->values[j] = calloc(count, sizeof(uint32_t));
            if (!res->values[j]) { fprintf(stderr, "HIP engine: out of memory for the result set\n"); rc = -1; break; }
            rc = own_dictionary(res, j, &t->dict[c], 4, count);
            continue;
        }
        char *raw = malloc(count * w);
        if (!raw) { fprintf(stderr, "HIP engine: out of memory for the result set\n"); rc = -1; break; }
        res->values[j] = raw;
        rc = project_column(q, c, gathered, scattered, sub_pos, raw, tmp);
        if (rc == 0 && schema.col[c].kind == HIPKIND_DICT)
            rc = own_dictionary(res, j, &t->dict[c], w, count);
    }
    for (int s = 0; s < q->n_shards; s++) if (gathered[s]) pqps_free(hipTableShard(t, s)->ctx, gathered[s]);
    return rc;
}

/* Caller holds the table shared. */
static int select_columnar(struct engineS *engine, struct hipTable *t, const char **selectItems, int numSelectItems,
                           struct whereClauseS *whereClause, struct hipColumnarResult *res) {
    struct query q;
    const int lane = hipTableAcquireLane(t);
    if (lane == HIP_LANE_REFUSED) return -1;                        /* reason on stderr */
    query_init(&q, engine, t, lane, false);
    int rc = query_issue(&q, whereClause);
    if (rc == 0) rc = query_await(&q);
    else for (int s = 0; s < q.n_shards; s++) (void)wait_shard(&q, s);
    const int n_shards = q.n_shards;
    const uint64_t count = rc == 0 ? q.total : 0;
    unsigned int *sub_pos[HIP_MAX_SHARDS];
    memset(sub_pos, 0, sizeof sub_pos);
    char *tmp = NULL;
    const bool scattered = rc == 0 && n_shards > 1 && q.n_probes > 0 && count > 0;
    if (scattered) {
        /* index mode over several shards: each shard gathers for its own rows in merged order (its sub-list
         * replaces the shard-order list in its lane), the values are scattered to their merged positions */
        uint64_t fill[HIP_MAX_SHARDS], biggest = 0;
        memset(fill, 0, sizeof fill);
        unsigned int *sub_ids[HIP_MAX_SHARDS];
        memset(sub_ids, 0, sizeof sub_ids);
        unsigned int *merged = malloc(count * sizeof *merged);
        if (!merged) rc = -1;
        if (rc == 0 && pqps_download(q.ids_ctx, merged, q.ids_dev, count * sizeof *merged, NULL) != PQPS_OK) rc = engine_error("ID download");
        for (int s = 0; s < n_shards; s++) {
            sub_ids[s] = malloc((q.count[s] ? q.count[s] : 1) * sizeof **sub_ids);
            sub_pos[s] = malloc((q.count[s] ? q.count[s] : 1) * sizeof **sub_pos);
            if (!sub_ids[s] || !sub_pos[s]) rc = -1;
            if (q.count[s] > biggest) biggest = q.count[s];
        }
        for (uint64_t i = 0; i < count && rc == 0; i++) {
            const unsigned int id = merged[i];
            int s = n_shards - 1;
            while (s > 0 && id < hipTableShard(t, s)->row0) s--;
            sub_ids[s][fill[s]] = id;
            sub_pos[s][fill[s]++] = (unsigned int)i;
        }
        for (int s = 0; s < n_shards && rc == 0; s++)
            if (q.count[s] && pqps_upload(lane_copy_ctx(&q, s), query_lane(&q, s)->ids_dev, sub_ids[s], q.count[s] * sizeof **sub_ids, NULL) != PQPS_OK)
                rc = engine_error("ID upload");
        for (int s = 0; s < n_shards; s++) free(sub_ids[s]);
        free(merged);
        tmp = malloc((biggest ? biggest : 1) * 8);
        if (!tmp) rc = -1;
    }
    if (rc == 0) rc = project_result(&q, selectItems, numSelectItems, count, scattered, sub_pos, tmp, res);
    for (int s = 0; s < n_shards; s++) free(sub_pos[s]);
    free(tmp);
    res->numRecords = (int)count;
    query_free(&q);
    hipTableReleaseLane(t, q.lane);
    return rc;
}

/* The empty result of a columnar SELECT: the column arrays for *selectItems -- none: all 12 columns, and the two arguments
 * are set to that list -- or, without an engine, the bare result.  Out of memory ends the process, as the reference's
 * result sets do. */
static struct hipColumnarResult *columnar_shell(struct engineS *engine, const char ***selectItems, int *numSelectItems) {
    struct hipColumnarResult *res = calloc(1, sizeof *res);
    if (!res) { perror("Failed to allocate memory for result set"); exit(EXIT_FAILURE); }
    if (!engine || !engine->record_block) return res;
    if (*selectItems == NULL || *numSelectItems == 0) { *selectItems = (const char **)k_all_columns; *numSelectItems = 12; }
    const size_t n = (size_t)*numSelectItems;
    res->numColumns = *numSelectItems;
    res->columnNames = calloc(n, sizeof(char *));
    res->columnKinds = calloc(n, sizeof(int));
    res->values = calloc(n, sizeof(void *));
    res->dictionaries = calloc(n, sizeof(*res->dictionaries));
    res->dictionarySizes = calloc(n, sizeof(int));
    if (!res->columnNames || !res->columnKinds || !res->values || !res->dictionaries || !res->dictionarySizes) { perror("Failed to allocate memory for result set"); exit(EXIT_FAILURE); }
    return res;
}

struct hipColumnarResult *executeQuerySelectColumnarHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                        struct whereClauseS *whereClause) {
    struct hipColumnarResult *res = columnar_shell(engine, &selectItems, &numSelectItems);
    if (!engine || !engine->record_block) return res;
    struct hipTable *t = engine->record_block;

    const double t0 = now_seconds();
    hipTableLockShared(t);
    const int rc = select_columnar(engine, t, selectItems, numSelectItems, whereClause, res);
    hipTableUnlockShared(t);
    res->queryTime = now_seconds() - t0;
    res->success = rc == 0;
    if (rc != 0) res->numRecords = 0;
    TRACE("SELECT (columnar): %d rows x %d columns in %.3f ms\n", res->numRecords, res->numColumns, res->queryTime * 1e3);
    return res;
}

/* ---- ORDER BY column [DESC] LIMIT K (include/executeEngine-hip.h) -------------------------------------------------- */

/* One ordered row as the host merges the shards: narrow keys a = (img ^ x) << 32 | row, b = 0; command_id a = v ^ x,
 * b = row (pqps_filter_topk's keys) -- ascending (a, b) is the answer's order. */
struct order_key { uint64_t a, b; };

static int order_key_cmp(const void *x, const void *y) {
    const struct order_key *p = x, *r = y;
    if (p->a != r->a) return p->a < r->a ? -1 : 1;
    return p->b < r->b ? -1 : p->b > r->b;
}

static uint32_t order_key_row(const struct order_key *k, bool wide) { return (uint32_t)(wide ? k->b : k->a); }

/* How the rows of an ORDER BY are found and ordered. */
struct order_plan {
    int c;                               /* HIPCOL_* of the order column                                          */
    bool desc, wide, key_signed;         /* command_id: 128-bit keys; i32 columns: signed images                    */
    uint32_t k;                          /* the top-K paths: K = limit; 0: the full sort                            */
    bool fused;                          /* single-pass scan-mode WHERE and K > 0: one fused launch per shard       */
    pqps_column kcol[HIP_MAX_SHARDS];    /* shard s's key column (sudo_used on the fused path: its bit plane)       */
    bool no_key;                         /* a single-valued string column: every key 0                             */
    /* ORDER BY several columns (order_plan_keys): the one-column fields above describe field[0] where one key remains */
    bool rows_only;                      /* no key remains: every key 0, the answer is the row order               */
    bool multi;                          /* kp.form is PACK32, PACK64 or CHAIN                                      */
    struct hipOrderKeyPlan kp;           /* one plan for all shards: bounds and dictionaries are table-wide          */
    pqps_order_field fld[HIP_MAX_SHARDS][HIP_ORDER_MAX_KEYS];   /* PACK32 / PACK64: shard s's fields                */
    pqps_column ccol[HIP_MAX_SHARDS][HIP_ORDER_MAX_KEYS];       /* CHAIN: shard s's key columns ...                 */
    int csigned[HIP_ORDER_MAX_KEYS], cdesc[HIP_ORDER_MAX_KEYS]; /* ... and their images' rules                      */
};

static bool order_is_chain(const struct order_plan *op) { return op->multi && op->kp.form == HIPORDER_CHAIN; }
static bool order_is_packed(const struct order_plan *op) { return op->multi && op->kp.form != HIPORDER_CHAIN; }

/* Shard s's keys of the top-K paths (n of them, K words each, downloaded from `out` on `cs`) appended to keys[*n_keys]. */
static int order_collect(pqps_ctx *cs, const uint64_t *out_dev, uint64_t n, bool wide, struct order_key *keys, uint64_t *n_keys) {
    if (n == 0) return 0;
    uint64_t *h = malloc((size_t)n * (wide ? 16 : 8));
    if (!h) return oom();
    if (pqps_download(cs, h, out_dev, (size_t)n * (wide ? 16 : 8), NULL) != PQPS_OK) { free(h); return engine_error("ORDER BY download"); }
    for (uint64_t i = 0; i < n; i++) keys[*n_keys + i] = wide ? (struct order_key){ h[2 * i], h[2 * i + 1] } : (struct order_key){ h[i], 0 };
    *n_keys += n;
    free(h);
    return 0;
}

struct topk_call { const struct order_plan *op; void **buf; const size_t *scratch_bytes; size_t out_bytes; };

static int topk_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct topk_call *a = arg;
    const struct order_plan *op = a->op;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    char *b = a->buf[s];
    const int rc = order_is_packed(op)
        ? pqps_filter_topk_multi(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, op->fld[s], (uint32_t)op->kp.n_fields, (uint32_t)sh->row0,
                                 op->k, b + 16 + a->out_bytes, a->scratch_bytes[s], (uint64_t *)(b + 16), (uint64_t *)b, stream)
        : pqps_filter_topk(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, op->no_key ? NULL : &op->kcol[s], op->key_signed, op->desc,
                           (uint32_t)sh->row0, op->k, b + 16 + a->out_bytes, a->scratch_bytes[s], (uint64_t *)(b + 16), (uint64_t *)b, stream);
    if (rc != PQPS_OK) return engine_error("ORDER BY filter");
    return 0;
}

/* The top-K paths on every shard: each shard's K best (fused: pqps_filter_topk on the query's lane; otherwise the
 * selection, left per shard, and pqps_topk_list over every list) into keys[0 .. *n_keys), *matches the selection's rows. */
static int order_topk(struct query *q, const struct order_plan *op, struct order_key *keys, uint64_t *n_keys, uint64_t *matches) {
    const uint32_t k = op->k;
    const size_t out_bytes = ((size_t)k * (op->wide ? 16 : 8) + 15) & ~(size_t)15;
    void *buf[HIP_MAX_SHARDS] = { NULL };
    uint64_t got[HIP_MAX_SHARDS] = { 0 };
    size_t scratch_bytes[HIP_MAX_SHARDS] = { 0 };
    int rc = 0;
    *n_keys = 0;
    *matches = 0;
    if (!op->fused) {
        rc = query_lists(q);
        if (rc == 0) *matches = q->total;
    }
    /* per shard one buffer: [16 B count][out: K keys][scratch] */
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        const uint64_t n = op->fused ? sh->n_rows : q->count[s];
        if (n == 0) continue;
        scratch_bytes[s] = pqps_topk_scratch_bytes(sh->ctx, n, k, op->wide, op->fused);
        if (pqps_malloc(sh->ctx, 16 + out_bytes + scratch_bytes[s], &buf[s]) != PQPS_OK) rc = engine_error("ORDER BY scratch");
    }
    if (rc == 0 && op->fused) {
        rc = fused_issue(q, topk_fused_call, &(struct topk_call){ op, buf, scratch_bytes, out_bytes });
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            if (!buf[s]) continue;
            if (pqps_download(lane_copy_ctx(q, s), &got[s], buf[s], sizeof got[s], NULL) != PQPS_OK) rc = engine_error("ORDER BY count");
            *matches += got[s];
        }
    } else if (rc == 0) {
        for (int s = 0; s < q->n_shards && rc == 0; s++) {
            struct hipTable *sh = hipTableShard(q->t, s);
            if (!buf[s]) continue;
            char *b = buf[s];
            got[s] = q->count[s];
            const int lrc = order_is_packed(op)
                ? pqps_topk_list_multi(lane_copy_ctx(q, s), op->fld[s], (uint32_t)op->kp.n_fields, query_lane(q, s)->ids_dev, q->count[s],
                                       (uint32_t)sh->row0, k, b + 16 + out_bytes, scratch_bytes[s], (uint64_t *)(b + 16), NULL)
                : pqps_topk_list(lane_copy_ctx(q, s), op->no_key ? NULL : &op->kcol[s], op->key_signed, op->desc, query_lane(q, s)->ids_dev, q->count[s],
                                 (uint32_t)sh->row0, k, b + 16 + out_bytes, scratch_bytes[s], (uint64_t *)(b + 16), NULL);
            if (lrc != PQPS_OK) rc = engine_error("ORDER BY list");
        }
    }
    for (int s = 0; s < q->n_shards && rc == 0; s++)
        if (buf[s]) rc = order_collect(lane_copy_ctx(q, s), (const uint64_t *)((char *)buf[s] + 16), got[s] < k ? got[s] : k, op->wide, keys, n_keys);
    for (int s = 0; s < q->n_shards; s++) if (buf[s]) pqps_free(hipTableShard(q->t, s)->ctx, buf[s]);
    return rc;
}

/* Row i of shard x against row j of shard y in the CHAIN form: the per-key images (nk arrays of take rows each), then the row. */
static int order_chain_cmp(const uint64_t *kx, uint64_t tx, uint64_t i, uint32_t rx, const uint64_t *ky, uint64_t ty, uint64_t j, uint32_t ry, int nk) {
    for (int f = 0; f < nk; f++) {
        const uint64_t a = kx[(uint64_t)f * tx + i], b = ky[(uint64_t)f * ty + j];
        if (a != b) return a < b ? -1 : 1;
    }
    return rx < ry ? -1 : rx > ry;
}

/* The full sort: the selection, every shard's list sorted on its device (pqps_sort_list; several keys: pqps_sort_list_multi
 * by the packed key, or pqps_sort_list_chain key by key), the first `want` rows of each downloaded and the shards merged on
 * the host by (key, row), the CHAIN form by (key 0, ..., key N-1, row) -- one shard needs no keys. */
static int order_sort(struct query *q, const struct order_plan *op, uint64_t want, uint32_t **rows, uint64_t *n_rows, uint64_t *matches) {
    int rc = query_lists(q);
    if (rc != 0) return rc;
    *matches = q->total;
    const int n_shards = q->n_shards;
    const bool merge = n_shards > 1;
    const bool chain = order_is_chain(op);
    const int nk = chain ? op->kp.n_fields : 1;                          /* key arrays per shard */
    uint32_t *ids[HIP_MAX_SHARDS] = { NULL };
    uint64_t *keys[HIP_MAX_SHARDS] = { NULL }, take[HIP_MAX_SHARDS] = { 0 }, total = 0;
    for (int s = 0; s < n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        const uint64_t n = q->count[s];
        if (n == 0) continue;
        pqps_ctx *cs = lane_copy_ctx(q, s);
        take[s] = n < want ? n : want;
        uint32_t *ids_dev = NULL;
        uint64_t *keys_dev = NULL;
        ids[s] = malloc((size_t)take[s] * sizeof **ids);
        if (merge) keys[s] = malloc((size_t)take[s] * (size_t)nk * sizeof **keys);
        if (!ids[s] || (merge && !keys[s])) { rc = oom(); break; }
        if (pqps_malloc(sh->ctx, n * sizeof(uint32_t), (void **)&ids_dev) != PQPS_OK ||
            (merge && pqps_malloc(sh->ctx, n * (size_t)nk * sizeof(uint64_t), (void **)&keys_dev) != PQPS_OK)) rc = engine_error("ORDER BY buffers");
        else if ((chain ? pqps_sort_list_chain(cs, op->ccol[s], op->csigned, op->cdesc, (uint32_t)nk, query_lane(q, s)->ids_dev, n, (uint32_t)sh->row0,
                                               ids_dev, keys_dev, NULL)
                  : op->multi ? pqps_sort_list_multi(cs, op->fld[s], (uint32_t)op->kp.n_fields, query_lane(q, s)->ids_dev, n, (uint32_t)sh->row0,
                                                     ids_dev, keys_dev, NULL)
                  : pqps_sort_list(cs, op->no_key ? NULL : &op->kcol[s], op->key_signed, op->desc, query_lane(q, s)->ids_dev, n, (uint32_t)sh->row0,
                                   ids_dev, keys_dev, NULL)) != PQPS_OK) rc = engine_error("ORDER BY sort");
        else if (pqps_download(cs, ids[s], ids_dev, (size_t)take[s] * sizeof **ids, NULL) != PQPS_OK) rc = engine_error("ORDER BY download");
        for (int f = 0; f < nk && merge && rc == 0; f++)                 /* the first take[s] of every key array of n */
            if (pqps_download(cs, keys[s] + (size_t)f * take[s], keys_dev + (size_t)f * n, (size_t)take[s] * sizeof **keys, NULL) != PQPS_OK)
                rc = engine_error("ORDER BY download");
        if (ids_dev) pqps_free(sh->ctx, ids_dev);
        if (keys_dev) pqps_free(sh->ctx, keys_dev);
        total += take[s];
    }
    if (total > want) total = want;
    uint32_t *out = NULL;
    if (rc == 0 && !merge) { out = ids[0]; ids[0] = NULL; }
    else if (rc == 0) {
        out = malloc((size_t)(total ? total : 1) * sizeof *out);
        if (!out) rc = oom();
        uint64_t at[HIP_MAX_SHARDS] = { 0 };
        for (uint64_t i = 0; i < total && rc == 0; i++) {              /* (a later shard holds later rows: the keys decide) */
            int best = -1;
            struct order_key bk = { 0, 0 };
            for (int s = 0; s < n_shards; s++) {
                if (at[s] >= take[s]) continue;
                if (chain) {
                    if (best < 0 || order_chain_cmp(keys[s], take[s], at[s], ids[s][at[s]], keys[best], take[best], at[best], ids[best][at[best]], nk) < 0) best = s;
                    continue;
                }
                const struct order_key ks = { keys[s][at[s]], ids[s][at[s]] };
                if (best < 0 || order_key_cmp(&ks, &bk) < 0) { best = s; bk = ks; }
            }
            out[i] = ids[best][at[best]++];
        }
    }
    for (int s = 0; s < n_shards; s++) { free(ids[s]); free(keys[s]); }
    if (rc == 0) { *rows = out; *n_rows = total; }
    else free(out);
    return rc;
}

/* The rows of the ORDER BY (caller holds the table shared and the query's lane): *rows (malloc'd) in order, *n_rows of
 * them, *matches the selection's count. */
static int order_rows(struct engineS *engine, struct whereClauseS *whereClause, struct query *q, struct order_plan *op, long long limit,
                      uint32_t **rows, uint64_t *n_rows, uint64_t *matches) {
    struct hipTable *t = q->t;
    *rows = NULL;
    *n_rows = 0;
    *matches = 0;
    int rc = bind_where(t, whereClause, &q->plan);
    q->have_plan = rc == 0;
    if (rc == 0) {
        q->n_probes = list_probes(engine, t, whereClause, &q->probes);
        if (q->n_probes < 0) { q->n_probes = 0; rc = -1; }
    }
    if (rc != 0) return rc;
    uint64_t all = 0;
    for (int s = 0; s < q->n_shards; s++) all += hipTableShard(t, s)->n_rows;
    if (all == 0) { *rows = malloc(sizeof **rows); return *rows ? 0 : -1; }      /* an empty table: no rows */
    const uint32_t kmax = order_is_chain(op) ? 0 : op->wide ? PQPS_TOPK_MAX_WIDE : PQPS_TOPK_MAX;   /* CHAIN: the sort only */
    op->k = limit > 0 && limit <= (long long)kmax ? (uint32_t)limit : 0;
    op->fused = op->k > 0 && q->plan.n_passes == 1 && q->n_probes == 0;
    op->no_key = op->rows_only || t->col[op->c].width == 0;
    for (int s = 0; s < q->n_shards; s++) {
        const struct hipTable *sh = hipTableShard(t, s);
        op->kcol[s] = op->fused && op->c == HIPCOL_SUDO_USED && sh->sudo_bits.data ? sh->sudo_bits : sh->col[op->c];
        for (int j = 0; j < op->kp.n_fields && op->multi; j++) {
            const struct hipOrderField *f = &op->kp.field[j];
            op->ccol[s][j] = sh->col[f->column];
            op->fld[s][j] = (pqps_order_field){ op->fused && f->column == HIPCOL_SUDO_USED && sh->sudo_bits.data ? sh->sudo_bits : sh->col[f->column],
                                                f->base, f->bits, f->shift, f->descending };
        }
    }
    if (op->k == 0) return order_sort(q, op, limit > 0 ? (uint64_t)limit : UINT64_MAX, rows, n_rows, matches);
    struct order_key *keys = malloc((size_t)q->n_shards * op->k * sizeof *keys);
    uint64_t n_keys = 0;
    if (!keys) return oom();
    rc = order_topk(q, op, keys, &n_keys, matches);
    if (rc == 0) {
        qsort(keys, (size_t)n_keys, sizeof *keys, order_key_cmp);
        const uint64_t n = n_keys < op->k ? n_keys : op->k;
        *rows = malloc((size_t)(n ? n : 1) * sizeof **rows);
        if (!*rows) rc = oom();
        else {
            for (uint64_t i = 0; i < n; i++) (*rows)[i] = order_key_row(&keys[i], op->wide);
            *n_rows = n;
        }
    }
    free(keys);
    return rc;
}

/* The order column's plan, or -1 with the reason on stderr. */
static int order_plan_init(struct hipTable *t, const char *orderColumn, bool descending, struct order_plan *op) {
    memset(op, 0, sizeof *op);
    if (!orderColumn) { fprintf(stderr, "HIP engine: ORDER BY without a column\n"); return -1; }
    op->c = hipColumnId(orderColumn);
    if (op->c < 0) { fprintf(stderr, "HIP engine: ORDER BY: unknown column '%s'\n", orderColumn); return -1; }
    if (t->xch) { fprintf(stderr, "HIP engine: ORDER BY is not exchanged across ranks\n"); return -1; }
    op->desc = descending;
    op->wide = op->c == HIPCOL_COMMAND_ID;
    op->key_signed = k_group_kind[op->c] == HIPKIND_I32;
    return 0;
}

/* The plan of a key list (the query is open: the i32 bounds are the table's cached ones), or -1 with the reason on stderr.
 * One remaining key is the one-column plan; none is the row order. */
static int order_plan_keys(struct query *q, const struct hipOrderKey *keys, int numKeys, struct order_plan *op) {
    struct hipTable *t = q->t;
    memset(op, 0, sizeof *op);
    if (!keys) { fprintf(stderr, "HIP engine: ORDER BY without keys\n"); return -1; }
    if (numKeys < 1 || numKeys > HIP_ORDER_MAX_KEYS) { fprintf(stderr, "HIP engine: ORDER BY: %d keys, not 1 .. %d\n", numKeys, HIP_ORDER_MAX_KEYS); return -1; }
    if (t->xch) { fprintf(stderr, "HIP engine: ORDER BY is not exchanged across ranks\n"); return -1; }
    const char *names[HIP_ORDER_MAX_KEYS];
    int desc[HIP_ORDER_MAX_KEYS], counts[HIPCOL_COUNT] = { 0 }, lo[HIPCOL_COUNT] = { 0 }, hi[HIPCOL_COUNT] = { 0 };
    for (int i = 0; i < numKeys; i++) {
        names[i] = keys[i].column;
        desc[i] = keys[i].descending;
        const int c = names[i] ? hipColumnId(names[i]) : -1;
        if (c < 0) continue;                                             /* hipOrderKeyPlan refuses it */
        if (k_group_kind[c] == HIPKIND_DICT) counts[c] = t->col[c].width == 0 ? (t->dict[c].count > 0) : (int)t->dict[c].count;
    }
    /* which keys remain does not depend on the i32 bounds: they are asked for (a min / max pass on first use) only where
     * several keys remain, so a key list that comes down to one column costs what the one-column query costs */
    if (hipOrderKeyPlan(names, desc, numKeys, counts, lo, hi, &op->kp) != 0) return -1;
    if (op->kp.form >= HIPORDER_PACK32) {
        for (int j = 0; j < op->kp.n_fields; j++) {
            const int c = op->kp.field[j].column;
            int32_t l, h;
            if (k_group_kind[c] != HIPKIND_I32) continue;
            if (column_bounds(q, c, &l, &h) != 0) return -1;
            lo[c] = l;
            hi[c] = h;
        }
        if (hipOrderKeyPlan(names, desc, numKeys, counts, lo, hi, &op->kp) != 0) return -1;
    }
    op->rows_only = op->kp.form == HIPORDER_ROWS;
    op->multi = op->kp.form >= HIPORDER_PACK32;
    if (op->multi) {
        op->wide = op->kp.form == HIPORDER_PACK64;
        for (int j = 0; j < op->kp.n_fields; j++) {
            op->csigned[j] = op->kp.field[j].kind == HIPKIND_I32;
            op->cdesc[j] = op->kp.field[j].descending;
        }
    } else {
        op->c = op->rows_only ? HIPCOL_COMMAND_ID : op->kp.field[0].column;  /* (no key: the column is not read) */
        op->desc = !op->rows_only && op->kp.field[0].descending;
        op->wide = !op->rows_only && op->c == HIPCOL_COMMAND_ID;
        op->key_signed = k_group_kind[op->c] == HIPKIND_I32;
    }
    return 0;
}

/* What an ORDER BY entry point orders by: a key list, or (keys == NULL) one column. */
struct order_request { const struct hipOrderKey *keys; int numKeys; const char *column; bool descending; };

static int order_request_plan(struct query *q, const struct order_request *r, struct order_plan *op) {
    return r->keys || r->numKeys ? order_plan_keys(q, r->keys, r->numKeys, op) : order_plan_init(q->t, r->column, r->descending, op);
}

static long long order_ids_run(struct engineS *engine, struct whereClauseS *whereClause, const struct order_request *r, long long limit,
                               unsigned int **ids, long long *matches, double *queryTime) {
    const double t0 = now_seconds();
    if (matches) *matches = 0;
    if (!engine || !engine->record_block || !ids) { fprintf(stderr, "HIP engine: ORDER BY without an engine or a result\n"); return -1; }
    *ids = NULL;
    struct query q;
    if (!query_open(engine, &q)) return -1;                              /* reason on stderr */
    struct order_plan op;
    uint32_t *rows = NULL;
    uint64_t n = 0, m = 0;
    int rc = order_request_plan(&q, r, &op);
    if (rc == 0) rc = order_rows(engine, whereClause, &q, &op, limit, &rows, &n, &m);
    query_close(&q);
    if (queryTime) *queryTime = now_seconds() - t0;
    if (rc != 0) { free(rows); return -1; }
    *ids = rows;
    if (matches) *matches = (long long)m;
    return (long long)n;
}

long long executeQueryOrderIdsByHIP(struct engineS *engine, struct whereClauseS *whereClause, const struct hipOrderKey *keys,
                                    int numKeys, long long limit, unsigned int **ids, long long *matches, double *queryTime) {
    if (!keys && numKeys == 0) numKeys = -1;                             /* (a key list, though an empty one: refused) */
    return order_ids_run(engine, whereClause, &(struct order_request){ keys, numKeys, NULL, false }, limit, ids, matches, queryTime);
}

long long executeQueryOrderIdsHIP(struct engineS *engine, struct whereClauseS *whereClause, const char *orderColumn,
                                  bool descending, long long limit, unsigned int **ids, long long *matches, double *queryTime) {
    return order_ids_run(engine, whereClause, &(struct order_request){ NULL, 0, orderColumn, descending }, limit, ids, matches, queryTime);
}

/* rows[0 .. n) (table-wide, in the result's order) projected into res (caller holds the table shared and the query's lane):
 * they become every shard's list in its lane, and the device gather of the columnar SELECT runs over those. */
static int project_listed_rows(struct query *q, const uint32_t *rows, uint64_t n, const char **selectItems, int numSelectItems,
                               struct hipColumnarResult *res) {
    struct hipTable *t = q->t;
    int rc = 0;
    /* shard s's k-th row goes to position sub_pos[s][k] of the result */
    const int n_shards = q->n_shards;
    unsigned int *sub_pos[HIP_MAX_SHARDS] = { NULL };
    uint32_t *sub_ids[HIP_MAX_SHARDS] = { NULL };
    uint64_t biggest = 0;
    for (int s = 0; s < n_shards && rc == 0; s++) {
        sub_ids[s] = malloc((size_t)(n ? n : 1) * sizeof **sub_ids);
        sub_pos[s] = malloc((size_t)(n ? n : 1) * sizeof **sub_pos);
        if (!sub_ids[s] || !sub_pos[s]) rc = oom();
        q->count[s] = 0;
    }
    for (uint64_t i = 0; i < n && rc == 0; i++) {
        int s = n_shards - 1;
        while (s > 0 && rows[i] < hipTableShard(t, s)->row0) s--;
        sub_ids[s][q->count[s]] = rows[i];
        sub_pos[s][q->count[s]++] = (unsigned int)i;
    }
    for (int s = 0; s < n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(t, s);
        struct hipLane *L = query_lane(q, s);
        if (q->count[s] > biggest) biggest = q->count[s];
        if (q->count[s] == 0) continue;
        if (grow_lane_ids(sh, L, q->count[s]) != 0) rc = -1;
        else if (pqps_upload(lane_copy_ctx(q, s), L->ids_dev, sub_ids[s], q->count[s] * sizeof **sub_ids, NULL) != PQPS_OK ||
                 pqps_upload(lane_copy_ctx(q, s), L->count_dev, &q->count[s], sizeof(uint64_t), NULL) != PQPS_OK) rc = engine_error("ID upload");
    }
    char *tmp = rc == 0 && n_shards > 1 ? malloc((biggest ? biggest : 1) * 8) : NULL;
    if (rc == 0 && n_shards > 1 && !tmp) rc = -1;
    if (rc == 0) rc = project_result(q, selectItems, numSelectItems, n, n_shards > 1, sub_pos, tmp, res);
    for (int s = 0; s < n_shards; s++) { free(sub_ids[s]); free(sub_pos[s]); }
    free(tmp);
    return rc;
}

static struct hipColumnarResult *order_select_run(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                  struct whereClauseS *whereClause, const struct order_request *r, long long limit,
                                                  long long *matches) {
    if (matches) *matches = 0;
    struct hipColumnarResult *res = columnar_shell(engine, &selectItems, &numSelectItems);
    if (!engine || !engine->record_block) return res;
    const double t0 = now_seconds();
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    struct order_plan op;
    uint32_t *rows = NULL;
    uint64_t n = 0, m = 0;
    int rc = order_request_plan(&q, r, &op);
    if (rc == 0) rc = order_rows(engine, whereClause, &q, &op, limit, &rows, &n, &m);
    if (rc == 0) rc = project_listed_rows(&q, rows, n, selectItems, numSelectItems, res);
    free(rows);
    query_close(&q);
    res->numRecords = rc == 0 ? (int)n : 0;
    res->queryTime = now_seconds() - t0;
    res->success = rc == 0;
    if (rc == 0 && matches) *matches = (long long)m;
    return res;
}

struct hipColumnarResult *executeQuerySelectOrderedHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                       struct whereClauseS *whereClause, const char *orderColumn,
                                                       bool descending, long long limit, long long *matches) {
    return order_select_run(engine, selectItems, numSelectItems, whereClause, &(struct order_request){ NULL, 0, orderColumn, descending },
                            limit, matches);
}

struct hipColumnarResult *executeQuerySelectOrderedByHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                         struct whereClauseS *whereClause, const struct hipOrderKey *keys, int numKeys,
                                                         long long limit, long long *matches) {
    if (!keys && numKeys == 0) numKeys = -1;                             /* (a key list, though an empty one: refused) */
    return order_select_run(engine, selectItems, numSelectItems, whereClause, &(struct order_request){ keys, numKeys, NULL, false },
                            limit, matches);
}

/* ---- the first row and the first N rows of every group (include/executeEngine-hip.h) ------------------------------- */
/* One driver (head_reduce): the first row is one round of the first N; only what the host does with the words differs. */

/* Checks the two columns and the engine; fills the result's column fields and the order plan.  -1: refused, reason on stderr. */
static int group_first_begin(struct engineS *engine, const char *groupColumn, const char *orderColumn, bool descending,
                             struct hipGroupFirstResult *res, struct order_plan *op) {
    res->groupColumn = res->groupKind = res->orderColumn = res->orderKind = -1;
    res->descending = descending;
    if (!engine || !engine->record_block || !orderColumn) { fprintf(stderr, "HIP engine: first row per group without an engine or an order column\n"); return -1; }
    memset(op, 0, sizeof *op);
    op->c = hipColumnId(orderColumn);
    if (op->c < 0) { fprintf(stderr, "HIP engine: first row per group: unknown order column '%s'\n", orderColumn); return -1; }
    const int c = groupColumn ? group_column_id("first row per group", groupColumn) : -1;
    if (groupColumn && c < 0) return -1;
    if (((struct hipTable *)engine->record_block)->xch) { fprintf(stderr, "HIP engine: first row per group is not exchanged across ranks\n"); return -1; }
    op->desc = descending;
    op->wide = op->c == HIPCOL_COMMAND_ID;
    op->key_signed = k_group_kind[op->c] == HIPKIND_I32;
    res->groupColumn = c;
    res->groupKind = c >= 0 ? k_group_kind[c] : -1;
    res->orderColumn = op->c;
    res->orderKind = k_group_kind[op->c];
    return 0;
}

/* One shard's candidates on the host, in the shape hipHeadMerge takes: at most `limit` entries per bin, ascending. */
struct head_list { uint64_t n; uint32_t *bins; uint64_t *words, *best; };

static int head_list_alloc(struct head_list *l, uint64_t cap, bool wide) {
    l->n = 0;
    l->bins = malloc((size_t)(cap ? cap : 1) * sizeof *l->bins);
    l->words = malloc((size_t)(cap ? cap : 1) * sizeof *l->words);
    l->best = wide ? malloc((size_t)(cap ? cap : 1) * sizeof *l->best) : NULL;
    return l->bins && l->words && (!wide || l->best) ? 0 : oom();
}

static void head_list_free(struct head_list *l) { free(l->bins); free(l->words); free(l->best); }

/* The round cap of this query: PQPS_HEAD_ROUNDS_MAX, or what PQPS_HEAD_ROUNDS says below it (0: the sort form always). */
static uint32_t head_round_cap(void) {
    const char *e = getenv("PQPS_HEAD_ROUNDS");
    if (!e || !*e) return PQPS_HEAD_ROUNDS_MAX;
    const long v = strtol(e, NULL, 0);
    return v < 0 ? 0u : v > (long)PQPS_HEAD_ROUNDS_MAX ? PQPS_HEAD_ROUNDS_MAX : (uint32_t)v;
}

/* The rounds form: one shard's device buffer is [16 B: the matching rows][out: rounds x n_bins words][best: the same,
 * command_id only].  The sort form has no buffer (shard_reduce's post).  lists[0 .. *n_lists): what the shards handed
 * (the N-rows query); the first-row query hands no lists: its one round's words meet in out[n_bins] (best[n_bins]:
 * command_id), all ones before the first shard.  head_reduce() says who sets what. */
struct head_call {
    const struct group_plan *gp; const struct order_plan *op; void **buf;
    uint32_t rounds; uint64_t limit;
    struct head_list *lists; int *n_lists;
    uint64_t *out, *best;
    uint64_t *matches; bool fused; int rc;
};

static int head_fused_call(struct query *q, int s, pqps_ctx *ctx, void *stream, void *arg) {
    const struct head_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct order_plan *op = a->op;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const struct shard_pred *sp = &q->sp[s];
    const bool grouped = gp->c >= 0 && !gp->single;
    uint64_t *b = a->buf[s];
    const size_t words = (size_t)a->rounds * gp->n_bins;
    if (pqps_filter_group_head(ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, op->no_key ? NULL : &op->kcol[s], op->key_signed, op->desc,
                               (uint32_t)sh->row0, grouped ? &gp->gcol[s] : NULL, gp->bin_base, gp->n_bins, a->rounds, b + 2,
                               op->wide ? b + 2 + words : NULL, b, stream) != PQPS_OK)
        return engine_error(a->out ? "first-row filter" : "first-rows filter");   /* a->out: the first-row query */
    return 0;
}

static int head_list_call(struct query *q, int s, pqps_ctx *cs, const struct hipLane *L, void *out, void *arg) {
    const struct head_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct order_plan *op = a->op;
    const struct hipTable *sh = hipTableShard(q->t, s);
    const bool grouped = gp->c >= 0 && !gp->single;
    uint64_t *b = out;
    const size_t words = (size_t)a->rounds * gp->n_bins;
    return pqps_group_head_list(cs, op->no_key ? NULL : &op->kcol[s], op->key_signed, op->desc, grouped ? &gp->gcol[s] : NULL, gp->bin_base,
                                gp->n_bins, sh->n_rows, L->ids_dev, L->count_dev, q->count[s], (uint32_t)sh->row0, a->rounds, b + 2,
                                op->wide ? b + 2 + words : NULL, NULL);
}

/* One round: one shard's words merged into the host's.  Rows are table-wide, so the minimum word per bin is the answer;
 * command_id compares (best, row).  (Lists and hipHeadMerge give the same answer; with 40 000 bins they were measured
 * 4 % slower per query)  The match count in front of the words is added up on the fused path only: the
 * list call does not write it, and the total is the selection's there. */
static void first_combine(void *arg, const void *host) {
    const struct head_call *a = arg;
    const uint32_t n_bins = a->gp->n_bins;
    const uint64_t *h = (const uint64_t *)host + 2;
    uint64_t *out = a->out, *best = a->best;
    if (a->fused) *a->matches += *(const uint64_t *)host;
    for (uint32_t k = 0; k < n_bins; k++) {
        if (h[k] == UINT64_MAX) continue;
        if (!a->op->wide) { if (h[k] < out[k]) out[k] = h[k]; continue; }
        const uint64_t hb = h[n_bins + k];
        if (out[k] == UINT64_MAX || hb < best[k] || (hb == best[k] && h[k] < out[k])) { out[k] = h[k]; best[k] = hb; }
    }
}

/* Several rounds: one shard's [round][bin] words into a list: bin by bin, the rounds until the first all-ones word. */
static void head_combine(void *arg, const void *host) {
    struct head_call *a = arg;
    const uint32_t n_bins = a->gp->n_bins, rounds = a->rounds;
    const bool wide = a->op->wide;
    const uint64_t *h = (const uint64_t *)host + 2, *hb = h + (size_t)rounds * n_bins;
    if (a->fused) *a->matches += *(const uint64_t *)host;
    if (a->rc != 0) return;
    uint64_t cap = 0;
    for (size_t i = 0; i < (size_t)rounds * n_bins; i++) cap += h[i] != UINT64_MAX;
    struct head_list *l = &a->lists[(*a->n_lists)++];
    if ((a->rc = head_list_alloc(l, cap, wide)) != 0) return;
    for (uint32_t k = 0; k < n_bins; k++)
        for (uint32_t r = 0; r < rounds && h[(size_t)r * n_bins + k] != UINT64_MAX; r++) {
            l->bins[l->n] = k;
            l->words[l->n] = h[(size_t)r * n_bins + k];
            if (wide) l->best[l->n] = hb[(size_t)r * n_bins + k];
            l->n++;
        }
}

/* The sort form on one shard's list: pqps_group_head_sort, then the kept entries downloaded into a list. */
static int head_sort_post(struct query *q, int s, pqps_ctx *cs, void *out, void *arg) {
    (void)out;
    struct head_call *a = arg;
    const struct group_plan *gp = a->gp;
    const struct order_plan *op = a->op;
    struct hipTable *sh = hipTableShard(q->t, s);
    const bool grouped = gp->c >= 0 && !gp->single;
    const uint64_t n = q->count[s];
    uint32_t *ids_dev = NULL, *ids = NULL;
    uint64_t *keys_dev = NULL, *keys = NULL, kept = 0;
    int rc = 0;
    if (pqps_malloc(sh->ctx, n * sizeof(uint32_t), (void **)&ids_dev) != PQPS_OK ||
        pqps_malloc(sh->ctx, 2 * n * sizeof(uint64_t), (void **)&keys_dev) != PQPS_OK) rc = engine_error("first-rows sort buffers");
    else if (pqps_group_head_sort(cs, op->no_key ? NULL : &op->kcol[s], op->key_signed, op->desc, grouped ? &gp->gcol[s] : NULL,
                                  gp->kind == HIPKIND_I32, query_lane(q, s)->ids_dev, n, (uint32_t)sh->row0, a->limit, q->n_probes > 0,
                                  ids_dev, keys_dev, &kept, NULL) != PQPS_OK) rc = engine_error("first-rows sort");
    struct head_list *l = &a->lists[*a->n_lists];
    if (rc == 0) {
        ++*a->n_lists;
        rc = head_list_alloc(l, kept, op->wide);
        ids = malloc((size_t)(kept ? kept : 1) * sizeof *ids);
        keys = malloc((size_t)(kept ? kept : 1) * 2 * sizeof *keys);
        if (rc == 0 && (!ids || !keys)) rc = oom();
    }
    if (rc == 0 && kept > 0 &&
        (pqps_download(cs, ids, ids_dev, (size_t)kept * sizeof *ids, NULL) != PQPS_OK ||
         pqps_download(cs, keys, keys_dev, (size_t)kept * sizeof *keys, NULL) != PQPS_OK ||
         pqps_download(cs, keys + kept, keys_dev + n, (size_t)kept * sizeof *keys, NULL) != PQPS_OK)) rc = engine_error("first-rows download");
    for (uint64_t i = 0; i < kept && rc == 0; i++) {
        /* the images of pqps_sort_list: an i32 group's is v ^ 2^31; a key that is not read is 0 in every row */
        const uint32_t bin = (grouped ? (uint32_t)keys[i] ^ (gp->kind == HIPKIND_I32 ? 0x80000000u : 0u) : gp->bin_base) - gp->bin_base;
        const uint64_t img = op->no_key ? (op->desc ? 0xFFFFFFFFull : 0ull) : keys[kept + i];
        if (bin >= gp->n_bins) continue;
        l->bins[l->n] = bin;
        l->words[l->n] = op->wide ? (uint64_t)ids[i] : img << 32 | ids[i];
        if (op->wide) l->best[l->n] = img;
        l->n++;
    }
    free(ids);
    free(keys);
    if (ids_dev) pqps_free(sh->ctx, ids_dev);
    if (keys_dev) pqps_free(sh->ctx, keys_dev);
    return rc;
}

/* Checks n, the two columns and the engine (group_first_begin); fills the result's column fields and the order plan. */
static int group_head_begin(struct engineS *engine, const char *groupColumn, const char *orderColumn, bool descending, long long n,
                            struct hipGroupHeadResult *res, struct order_plan *op) {
    struct hipGroupFirstResult gf;
    memset(&gf, 0, sizeof gf);
    res->groupColumn = res->groupKind = res->orderColumn = res->orderKind = -1;
    res->descending = descending;
    if (n < 1) { fprintf(stderr, "HIP engine: first rows per group: n = %lld, not >= 1\n", n); return -1; }
    res->limit = n > INT_MAX ? INT_MAX : (int)n;
    const int rc = group_first_begin(engine, groupColumn, orderColumn, descending, &gf, op);
    res->groupColumn = gf.groupColumn; res->groupKind = gf.groupKind;
    res->orderColumn = gf.orderColumn; res->orderKind = gf.orderKind;
    return rc;
}

/* One word (and its `best`: command_id) into the row, the order key and the key's text as the order column's cell reads.
 * Inline: it runs once per answer row, and the fills pass it the same columns and kinds every time. */
static inline int first_word_decode(const struct hipTable *t, const char *what, int oc, int kind, bool desc, uint64_t word, uint64_t best,
                             unsigned int *row, long long *key, char **text) {
    char buf[32];
    const char *cell = buf;
    if (kind == HIPKIND_U64) {
        *row = (unsigned int)word;
        *key = (long long)(best ^ (desc ? UINT64_MAX : 0));
        snprintf(buf, sizeof buf, "%llu", (unsigned long long)*key);
    } else {
        hipFirstKeyDecode(kind, desc, word, key, row);
        if (kind == HIPKIND_I32) snprintf(buf, sizeof buf, "%d", (int)*key);
        else if (kind == HIPKIND_BOOL) cell = *key ? "true" : "false";
        else if (*key < (long long)t->dict[oc].count) cell = t->dict[oc].values[*key];
        else { fprintf(stderr, "HIP engine: %s: code %lld outside the dictionary\n", what, *key); return -1; }
    }
    return (*text = strdup(cell)) ? 0 : oom();
}

/* The merged entries (ascending bin, then order) into the result: groups with a row only, in bin order. */
static int group_head_fill(struct hipGroupHeadResult *res, const struct hipTable *t, const uint32_t *bins, const uint64_t *words,
                           const uint64_t *best, uint64_t n, uint32_t n_bins, int32_t lo) {
    uint64_t *present = calloc((size_t)n_bins + 1, sizeof *present);
    if (!present) return oom();
    for (uint64_t i = 0; i < n; i++) present[bins[i]]++;
    int rc = group_keys_fill(t, res->groupColumn, res->groupKind, lo, present, n_bins, &res->keys, &res->keyText, &res->numGroups);
    res->offsets = calloc((size_t)res->numGroups + 1, sizeof *res->offsets);
    res->rows = calloc((size_t)n + 1, sizeof *res->rows);
    res->orderKeys = calloc((size_t)n + 1, sizeof *res->orderKeys);
    res->orderText = calloc((size_t)n + 1, sizeof *res->orderText);
    if (rc == 0 && (!res->offsets || !res->rows || !res->orderKeys || !res->orderText)) rc = oom();
    int g = 0;
    for (uint32_t k = 0; k < n_bins && rc == 0; k++)
        if (present[k]) { res->offsets[g + 1] = res->offsets[g] + (long long)present[k]; g++; }
    free(present);
    for (uint64_t i = 0; i < n && rc == 0; i++)
        rc = first_word_decode(t, "first rows per group", res->orderColumn, res->orderKind, res->descending, words[i], best ? best[i] : 0,
                               &res->rows[i], &res->orderKeys[i], &res->orderText[i]);
    return rc;
}

/* One round's words, out[n_bins] (best[n_bins] for command_id), into the result: the bins with a row only, in bin order. */
static int group_first_fill(struct hipGroupFirstResult *res, const struct hipTable *t, const uint64_t *out, const uint64_t *best,
                            uint32_t n_bins, int32_t lo) {
    uint64_t *present = calloc((size_t)n_bins + 1, sizeof *present);
    if (!present) return oom();
    for (uint32_t k = 0; k < n_bins; k++) present[k] = out[k] != UINT64_MAX;
    int rc = group_keys_fill(t, res->groupColumn, res->groupKind, lo, present, n_bins, &res->keys, &res->keyText, &res->numGroups);
    free(present);
    if (rc != 0) return -1;
    const size_t n = (size_t)res->numGroups;
    res->rows = calloc(n + 1, sizeof *res->rows);
    res->orderKeys = calloc(n + 1, sizeof *res->orderKeys);
    res->orderText = calloc(n + 1, sizeof *res->orderText);
    if (!res->rows || !res->orderKeys || !res->orderText) return oom();
    size_t g = 0;
    for (uint32_t k = 0; k < n_bins && rc == 0; k++) {
        if (out[k] == UINT64_MAX) continue;
        rc = first_word_decode(t, "first row per group", res->orderColumn, res->orderKind, res->descending, out[k], best ? best[k] : 0,
                               &res->rows[g], &res->orderKeys[g], &res->orderText[g]);
        g++;
    }
    return rc;
}

/* The query on every shard (shard_reduce).  a->rounds: that many rounds of the scan; 0: the sort form.  With a->out the one
 * round's words meet per bin in a->out (first_combine); without it every shard hands a list into a->lists.  *a->matches =
 * the selection's rows.  The caller sets rounds, limit, out / best or lists / n_lists, and matches; the rest is set here. */
static int head_reduce(struct query *q, struct group_plan *gp, struct order_plan *op, struct head_call *a) {
    struct hipTable *t = q->t;
    void *buf[HIP_MAX_SHARDS];
    if (!a->rounds) {                                                    /* the sort form works on the selection's lists */
        gp->fused = false;
        for (int s = 0; s < q->n_shards && gp->c >= 0; s++) gp->gcol[s] = hipTableShard(t, s)->col[gp->c];
    }
    op->fused = gp->fused;
    op->no_key = t->col[op->c].width == 0;
    for (int s = 0; s < q->n_shards; s++) {
        const struct hipTable *sh = hipTableShard(t, s);
        op->kcol[s] = gp->fused && op->c == HIPCOL_SUDO_USED && sh->sudo_bits.data ? sh->sudo_bits : sh->col[op->c];
    }
    a->gp = gp; a->op = op; a->buf = buf; a->fused = gp->fused;
    const struct shard_reduce r = a->rounds
        ? (struct shard_reduce){ .what = a->out ? "first-row words" : "first-rows words", .bytes = 16 + (size_t)a->rounds * gp->n_bins * (op->wide ? 2 : 1) * sizeof(uint64_t),
                                 .fused = head_fused_call, .list = head_list_call, .combine = a->out ? first_combine : head_combine }
        : (struct shard_reduce){ .what = "first-rows sort", .post = head_sort_post };
    int rc = shard_reduce(q, gp->fused, &r, buf, a);
    if (rc == 0) rc = a->rc;
    if (rc == 0 && !gp->fused) *a->matches = q->total;
    return rc;
}

/* The first N rows of every group (caller holds the table shared and the query's lane, group_head_begin has passed).
 * `rounds`: the caller's choice of the rounds form; else the sort form. */
static int group_head_run(struct engineS *engine, struct query *q, const char *groupColumn, struct order_plan *op, long long n,
                          bool rounds, struct whereClauseS *whereClause, struct hipGroupHeadResult *res) {
    struct group_plan gp;
    struct head_list lists[HIP_MAX_SHARDS];
    struct hipHeadList in[HIP_MAX_SHARDS];
    int n_lists = 0;
    uint64_t matches = 0, total = 0;
    uint32_t *bins = NULL;
    uint64_t *words = NULL, *best = NULL;
    long long kept = 0;
    int rc = group_plan_init(engine, whereClause, q, res->groupColumn, groupColumn, "first rows per group", &gp);
    if (rc == 0 && !gp.empty) {
        rc = head_reduce(q, &gp, op, &(struct head_call){ .rounds = rounds ? (uint32_t)n : 0, .limit = (uint64_t)n, .lists = lists,
                                                          .n_lists = &n_lists, .matches = &matches });
        for (int s = 0; s < n_lists; s++) {
            in[s] = (struct hipHeadList){ lists[s].n, lists[s].bins, lists[s].words, lists[s].best };
            total += lists[s].n;
        }
        if (rc == 0 && total > 0) {
            bins = malloc((size_t)total * sizeof *bins);
            words = malloc((size_t)total * sizeof *words);
            best = op->wide ? malloc((size_t)total * sizeof *best) : NULL;
            if (!bins || !words || (op->wide && !best)) rc = oom();
            else if ((kept = hipHeadMerge(in, n_lists, n, bins, words, best)) < 0) rc = -1;
        }
    }
    if (rc == 0) rc = group_head_fill(res, q->t, bins, words, best, (uint64_t)kept, gp.empty ? 0u : gp.n_bins, gp.lo);
    if (rc == 0) res->total = (long long)matches;
    for (int s = 0; s < n_lists; s++) head_list_free(&lists[s]);
    free(bins);
    free(words);
    free(best);
    return rc;
}

/* The first row of every group: one round of the same scan, whatever PQPS_HEAD_ROUNDS says (that variable moves the switch
 * of the N-rows query only).  One word per bin, so the shards' words meet in a dense array and no list is built. */
static int group_first_run(struct engineS *engine, struct query *q, const char *groupColumn, struct order_plan *op,
                           struct whereClauseS *whereClause, struct hipGroupFirstResult *res) {
    struct group_plan gp;
    uint64_t *out = NULL, *best = NULL, matches = 0;
    int rc = group_plan_init(engine, whereClause, q, res->groupColumn, groupColumn, "first row per group", &gp);
    if (rc == 0 && !gp.empty) {
        out = malloc((size_t)gp.n_bins * sizeof *out);
        best = op->wide ? malloc((size_t)gp.n_bins * sizeof *best) : NULL;
        if (!out || (op->wide && !best)) rc = oom();
        else {
            memset(out, 0xFF, (size_t)gp.n_bins * sizeof *out);
            if (best) memset(best, 0xFF, (size_t)gp.n_bins * sizeof *best);
            rc = head_reduce(q, &gp, op, &(struct head_call){ .rounds = 1, .limit = 1, .out = out, .best = best, .matches = &matches });
        }
    }
    if (rc == 0) rc = group_first_fill(res, q->t, out, best, gp.empty ? 0u : gp.n_bins, gp.lo);
    if (rc == 0) res->total = (long long)matches;
    free(out);
    free(best);
    return rc;
}

static void group_head_clear(struct hipGroupHeadResult *res) {
    const long long n = res->offsets ? res->offsets[res->numGroups] : 0;
    free_group_keys(res->keys, res->keyText, res->numGroups);
    for (long long i = 0; i < n && res->orderText; i++) free(res->orderText[i]);
    free(res->orderText);
    free(res->orderKeys);
    free(res->rows);
    free(res->offsets);
}

static void group_first_clear(struct hipGroupFirstResult *res) {
    free_group_keys(res->keys, res->keyText, res->numGroups);
    for (int g = 0; g < res->numGroups && res->orderText; g++) free(res->orderText[g]);
    free(res->orderText);
    free(res->orderKeys);
    free(res->rows);
}

struct hipGroupFirstResult *executeQueryGroupFirstHIP(struct engineS *engine, const char *groupColumn, const char *orderColumn,
                                                      bool descending, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipGroupFirstResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    struct order_plan op;
    if (group_first_begin(engine, groupColumn, orderColumn, descending, res, &op) != 0) return res;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    if (group_first_run(engine, &q, groupColumn, &op, whereClause, res) == 0) res->success = true;
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeGroupFirstResultHIP(struct hipGroupFirstResult *res) {
    if (!res) return;
    group_first_clear(res);
    free(res);
}

struct hipColumnarResult *executeQuerySelectGroupFirstHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                          struct whereClauseS *whereClause, const char *groupColumn,
                                                          const char *orderColumn, bool descending, long long *matches) {
    if (matches) *matches = 0;
    struct hipColumnarResult *res = columnar_shell(engine, &selectItems, &numSelectItems);
    if (!engine || !engine->record_block) return res;
    const double t0 = now_seconds();
    struct hipGroupFirstResult gf;
    struct order_plan op;
    memset(&gf, 0, sizeof gf);
    if (group_first_begin(engine, groupColumn, orderColumn, descending, &gf, &op) != 0) return res;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    int rc = group_first_run(engine, &q, groupColumn, &op, whereClause, &gf);
    const uint64_t n = rc == 0 ? (uint64_t)gf.numGroups : 0;
    if (rc == 0) rc = project_listed_rows(&q, gf.rows, n, selectItems, numSelectItems, res);
    query_close(&q);
    res->numRecords = rc == 0 ? (int)n : 0;
    res->queryTime = now_seconds() - t0;
    res->success = rc == 0;
    if (rc == 0 && matches) *matches = gf.total;
    group_first_clear(&gf);
    return res;
}

struct hipGroupHeadResult *executeQueryGroupHeadHIP(struct engineS *engine, const char *groupColumn, const char *orderColumn,
                                                    bool descending, long long n, struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    struct hipGroupHeadResult *res = calloc(1, sizeof *res);
    if (!res) { oom(); return NULL; }
    struct order_plan op;
    if (group_head_begin(engine, groupColumn, orderColumn, descending, n, res, &op) != 0) return res;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    if (group_head_run(engine, &q, groupColumn, &op, n, (unsigned long long)n <= head_round_cap(), whereClause, res) == 0)
        res->success = true;
    query_close(&q);
    res->queryTime = now_seconds() - t0;
    return res;
}

void freeGroupHeadResultHIP(struct hipGroupHeadResult *res) {
    if (!res) return;
    group_head_clear(res);
    free(res);
}

struct hipColumnarResult *executeQuerySelectGroupHeadHIP(struct engineS *engine, const char **selectItems, int numSelectItems,
                                                         struct whereClauseS *whereClause, const char *groupColumn,
                                                         const char *orderColumn, bool descending, long long n, long long *matches,
                                                         long long **offsets) {
    if (matches) *matches = 0;
    if (offsets) *offsets = NULL;
    struct hipColumnarResult *res = columnar_shell(engine, &selectItems, &numSelectItems);
    if (!engine || !engine->record_block) return res;
    const double t0 = now_seconds();
    struct hipGroupHeadResult gh;
    struct order_plan op;
    memset(&gh, 0, sizeof gh);
    if (group_head_begin(engine, groupColumn, orderColumn, descending, n, &gh, &op) != 0) return res;
    struct query q;
    if (!query_open(engine, &q)) return res;                             /* reason on stderr */
    int rc = group_head_run(engine, &q, groupColumn, &op, n, (unsigned long long)n <= head_round_cap(), whereClause, &gh);
    const uint64_t rows = rc == 0 ? (uint64_t)gh.offsets[gh.numGroups] : 0;
    if (rc == 0) rc = project_listed_rows(&q, gh.rows, rows, selectItems, numSelectItems, res);
    query_close(&q);
    res->numRecords = rc == 0 ? (int)rows : 0;
    res->queryTime = now_seconds() - t0;
    res->success = rc == 0;
    if (rc == 0 && matches) *matches = gh.total;
    if (rc == 0 && offsets) {
        *offsets = malloc(((size_t)gh.numGroups + 1) * sizeof **offsets);
        if (*offsets) memcpy(*offsets, gh.offsets, ((size_t)gh.numGroups + 1) * sizeof **offsets);
        else { oom(); res->success = false; }
    }
    group_head_clear(&gh);
    return res;
}

void freeColumnarResultHIP(struct hipColumnarResult *res) {
    if (!res) return;
    for (int j = 0; j < res->numColumns; j++) {
        if (res->columnNames) free(res->columnNames[j]);
        if (res->values) free(res->values[j]);
        if (res->dictionaries && res->dictionaries[j]) {
            for (int v = 0; v < res->dictionarySizes[j]; v++) free((void *)res->dictionaries[j][v]);
            free((void *)res->dictionaries[j]);
        }
    }
    free(res->columnNames); free(res->columnKinds); free(res->values); free((void *)res->dictionaries); free(res->dictionarySizes);
    free(res);
}

char *hipColumnarCellText(const struct hipColumnarResult *res, int row, int col) {
    char buf[32];
    if (!res || row < 0 || row >= res->numRecords || col < 0 || col >= res->numColumns) return NULL;
    const void *v = res->values[col];
    switch (res->columnKinds[col]) {                                    /* get_attribute_string_value, S:216-248 */
    case HIPKIND_U64: snprintf(buf, sizeof buf, "%llu", (unsigned long long)((const uint64_t *)v)[row]); return strdup(buf);
    case HIPKIND_I32: snprintf(buf, sizeof buf, "%d", ((const int32_t *)v)[row]); return strdup(buf);
    case HIPKIND_BOOL: return strdup(((const uint8_t *)v)[row] ? "true" : "false");
    case HIPKIND_DICT: return strdup(res->dictionaries[col][((const uint32_t *)v)[row]]);
    default: return strdup("NULL");                                     /* unknown column, S:244 */
    }
}

struct resultSetS *hipColumnarHead(const struct hipColumnarResult *res, int limit) {
    struct resultSetS *rs = calloc(1, sizeof *rs);
    if (!rs || !res) { free(rs); return NULL; }
    const int rows = limit <= 0 || limit > res->numRecords ? res->numRecords : limit;   /* printTable: limit <= 0 = every row */
    rs->numRecords = res->numRecords;                                   /* the footer counts every record */
    rs->numColumns = res->numColumns;
    rs->columnNames = malloc((size_t)(res->numColumns > 0 ? res->numColumns : 1) * sizeof(char *));
    for (int j = 0; j < res->numColumns; j++) rs->columnNames[j] = strdup(res->columnNames[j]);
    rs->columnTypes = calloc((size_t)(res->numColumns > 0 ? res->numColumns : 1), sizeof(FieldType));
    rs->data = malloc((size_t)(rows > 0 ? rows : 1) * sizeof(char **));
    for (int i = 0; i < rows; i++) {
        rs->data[i] = malloc((size_t)(res->numColumns > 0 ? res->numColumns : 1) * sizeof(char *));
        for (int j = 0; j < res->numColumns; j++) rs->data[i][j] = hipColumnarCellText(res, i, j);
    }
    rs->queryTime = res->queryTime;
    rs->success = res->success;
    return rs;
}

void freeResultSetHead(struct resultSetS *head, int rows) {
    if (!head) return;
    const int full = head->numRecords;
    head->numRecords = rows <= 0 || rows > full ? full : rows;          /* only these rows were materialised */
    freeResultSet(head);
}

/* executeQuerySelectHIP on an engine without host rows: the same strings, made from values gathered on the device. */
static struct resultSetS *select_device_only(struct engineS *engine, const char **selectItems, int numSelectItems, struct whereClauseS *whereClause) {
    struct hipColumnarResult *res = executeQuerySelectColumnarHIP(engine, selectItems, numSelectItems, whereClause);
    struct resultSetS *rs = res && res->success ? hipColumnarHead(res, 0) : NULL;      /* every row */
    if (!rs) {
        rs = calloc(1, sizeof *rs);
        if (!rs) { perror("Failed to allocate memory for result set"); exit(EXIT_FAILURE); }
        rs->success = false;
    }
    if (res) freeColumnarResultHIP(res);
    return rs;
}

/* freeResultSet, S:881-908. */
void freeResultSet(struct resultSetS *result) {
    if (!result) return;
    const double t_free = now_seconds();
    const long long cells = (long long)result->numRecords * result->numColumns;
    if (result->columnNames) {
        for (int j = 0; j < result->numColumns; j++) free(result->columnNames[j]);
        free(result->columnNames);
    }
    free(result->columnTypes);
    if (result->data) {
        for (int i = 0; i < result->numRecords; i++) {
            if (!result->data[i]) continue;
            for (int j = 0; j < result->numColumns; j++) free(result->data[i][j]);
            free(result->data[i]);
        }
        free(result->data);
    }
    free(result);
    TRACE("freeResultSet: %lld cells, %.3f ms\n", cells, (now_seconds() - t_free) * 1e3);
}

int isAttributeIndexed(struct engineS *engine, const char *attributeName) {
    for (int i = 0; i < engine->num_indexes; i++)
        if (strcmp(engine->indexed_attributes[i], attributeName) == 0) return i;
    return -1;
}

/* ---- helpers over caller-supplied rows ---------------------------------------------- */

static pqps_ctx *g_adhoc_ctx;
static pthread_mutex_t g_adhoc_lock = PTHREAD_MUTEX_INITIALIZER;   /* one shared context: one ad-hoc filter at a time */

static pqps_ctx *adhoc_ctx(void) {
    if (!g_adhoc_ctx) {
        int device = 0;
        const char *env = getenv("PQPS_DEVICE");
        if (env) device = atoi(env);
        if (pqps_ctx_create(device, &g_adhoc_ctx) != PQPS_OK) { engine_error("cannot create a device context"); g_adhoc_ctx = NULL; }
    }
    return g_adhoc_ctx;
}

static int adhoc_search(struct hipTable *t, record **records, struct whereClauseS *whereClause, record ***out, int *matching) {
    struct engineS none;                                /* no indexes: always the scan path */
    memset(&none, 0, sizeof none);
    struct query q;
    query_init(&q, &none, t, -1, false);                /* a table without lanes: its own context and buffers */
    int rc = query_issue(&q, whereClause);
    if (rc == 0) rc = query_await(&q);
    const uint64_t count = rc == 0 ? q.total : 0;
    uint32_t *ids = malloc((count ? count : 1) * sizeof *ids);
    record **hit = malloc((count ? count : 1) * sizeof *hit);
    if (rc == 0 && (!ids || !hit)) { fprintf(stderr, "HIP engine: out of memory for results\n"); rc = -1; }
    if (rc == 0 && count && pqps_download(q.ids_ctx, ids, q.ids_dev, count * sizeof *ids, NULL) != PQPS_OK) rc = engine_error("ID download");
    query_free(&q);
    if (rc != 0) { free(ids); free(hit); return -1; }
    for (uint64_t i = 0; i < count; i++) hit[i] = records[ids[i]];
    free(ids);
    *out = hit;
    *matching = (int)count;
    return 0;
}

/* linearSearchRecords, S:854-878: the rows are columnarised, filtered on the
 * GPU (input order kept) and the surviving pointers returned.  NULL (and 0 matches) when the device or
 * the clause fails; the reason is on stderr. */
record **linearSearchRecords(record **records, int num_records, struct whereClauseS *whereClause,
                             int *matchingRecords) {
    *matchingRecords = 0;
    record **out = NULL;
    pthread_mutex_lock(&g_adhoc_lock);
    pqps_ctx *ctx = adhoc_ctx();
    if (ctx) {
        struct hipTable *t = hipTableFromRows(ctx, records, (size_t)(num_records > 0 ? num_records : 0));
        if (adhoc_search(t, records, whereClause, &out, matchingRecords) != 0) { out = NULL; *matchingRecords = 0; }
        hipTableFree(t, 0);
    }
    pthread_mutex_unlock(&g_adhoc_lock);
    return out;
}

/* evaluateWhereClause, S:292-316, for one row: a one-row table through the same kernel. */
bool evaluateWhereClause(record *r, struct whereClauseS *wc) {
    if (wc == NULL) return true;
    int n = 0;
    record *rows[1] = { r };
    record **hit = linearSearchRecords(rows, 1, wc, &n);
    free(hit);
    return n == 1;
}

/* ---- lifecycle ------------------------------------------------------------------------ */

/* PQPS_PROBE_BOOL=1: new engines follow the OpenMP / MPI engines' row selection (hipEngineProbeBoolIndexes) */
static void probe_mode_from_env(struct engineS *engine) {
    const char *env = getenv("PQPS_PROBE_BOOL");
    if (env && atoi(env) != 0 && engine->record_block) ((struct hipTable *)engine->record_block)->probe_bool = 1;
}

struct engineS *initializeEngineHIP(int num_indexes, const char *indexed_attributes[],
                                    const int attribute_types[], const char *datafile,
                                    const char *tableName) {
    struct engineS *engine = malloc(sizeof *engine);
    if (!engine) { perror("Failed to allocate memory for engine"); exit(EXIT_FAILURE); }
    memset(engine, 0, sizeof *engine);
    engine->tableName = strdup(tableName ? tableName : "");
    if (!datafile) datafile = "../data/commands_50k.csv";          /* S:757 */
    engine->datafile = strdup(datafile);
    const double t0 = now_seconds();
    struct hipContextFuture *device = hipBeginContextHIP();        /* HIP start-up runs beside the CSV parse */
    engine->all_records = getAllRecordsFromFileHIP(datafile, &engine->num_records, &engine->record_block);
    const double t1 = now_seconds();
    buildDeviceTableOnHIP(engine, device);                         /* exits loudly without a GPU */
    const double t2 = now_seconds();
    for (int i = 0; i < num_indexes; i++) {
        if (!makeIndexHIP(engine, indexed_attributes[i], attribute_types[i]))
            fprintf(stderr, "Failed to create index for attribute: %s\n", indexed_attributes[i]);
    }
    probe_mode_from_env(engine);
    TRACE("init: %d rows, CSV -> rows %.1f ms, rows -> device columns %.1f ms, %d indexes %.1f ms\n", engine->num_records,
          (t1 - t0) * 1e3, (t2 - t1) * 1e3, num_indexes, (now_seconds() - t2) * 1e3);
    return engine;
}

/* An engine without host rows: all_records NULL, datafile "" (no CSV is kept in step). */
static struct engineS *engine_shell(unsigned long long num_rows, const char *tableName) {
    if (num_rows > (unsigned long long)INT_MAX) {
        fprintf(stderr, "HIP engine: %llu rows: the engine API counts rows in int (include/executeEngine-serial.h:22)\n", num_rows);
        return NULL;
    }
    struct engineS *engine = malloc(sizeof *engine);
    if (!engine) { perror("Failed to allocate memory for engine"); exit(EXIT_FAILURE); }
    memset(engine, 0, sizeof *engine);
    engine->tableName = strdup(tableName ? tableName : "");
    engine->datafile = strdup("");
    engine->num_records = (int)num_rows;
    return engine;
}

static void engine_indexes(struct engineS *engine, int num_indexes, const char *indexed_attributes[], const int attribute_types[]) {
    for (int i = 0; i < num_indexes; i++)
        if (!makeIndexHIP(engine, indexed_attributes[i], attribute_types[i]))
            fprintf(stderr, "Failed to create index for attribute: %s\n", indexed_attributes[i]);
    probe_mode_from_env(engine);
}

struct engineS *initializeEngineColumnsHIP(unsigned long long num_rows, const struct hipColumnData columns[12],
                                           int num_indexes, const char *indexed_attributes[], const int attribute_types[],
                                           const char *tableName) {
    if (!columns) return NULL;
    struct engineS *engine = engine_shell(num_rows, tableName);
    if (!engine) return NULL;
    const double t0 = now_seconds();
    buildDeviceTableFromColumnsHIP(engine, num_rows, columns);      /* exits loudly without a GPU */
    const double t1 = now_seconds();
    engine_indexes(engine, num_indexes, indexed_attributes, attribute_types);
    TRACE("init (columns): %llu rows, device columns %.1f ms, %d indexes %.1f ms\n", num_rows, (t1 - t0) * 1e3, num_indexes, (now_seconds() - t1) * 1e3);
    return engine;
}

struct engineS *initializeEngineSyntheticHIP(unsigned long long num_rows, unsigned long long seed,
                                             int num_indexes, const char *indexed_attributes[], const int attribute_types[],
                                             const char *tableName) {
    struct engineS *engine = engine_shell(num_rows, tableName);
    if (!engine) return NULL;
    const double t0 = now_seconds();
    buildSyntheticDeviceTableHIP(engine, num_rows, seed);           /* exits loudly without a GPU */
    const double t1 = now_seconds();
    engine_indexes(engine, num_indexes, indexed_attributes, attribute_types);
    TRACE("init (synthetic): %llu rows, generation %.1f ms, %d indexes %.1f ms\n", num_rows, (t1 - t0) * 1e3, num_indexes, (now_seconds() - t1) * 1e3);
    return engine;
}

void destroyEngineHIP(struct engineS *engine) {
    if (!engine) { fprintf(stderr, "Attempted to destroy a NULL engine pointer\n"); return; }
    const double t_destroy = now_seconds();
    value_sets_destroy(engine->record_block);                      /* the sets nobody freed, while their contexts live */
    destroyDeviceTableHIP(engine);                                 /* frees the row block too */
    TRACE("destroy: device table + context %.3f ms\n", (now_seconds() - t_destroy) * 1e3);
    free(engine->bplus_tree_roots);
    if (engine->indexed_attributes) {
        for (int i = 0; i < engine->num_indexes; i++) free(engine->indexed_attributes[i]);
        free(engine->indexed_attributes);
    }
    free(engine->attribute_types);
    free(engine->all_records);
    free(engine->tableName);
    free(engine->datafile);
    free(engine);
}

bool addAttributeIndexHIP(struct engineS *engine, const char *tableName, const char *attributeName,
                          int attributeType) {
    (void)tableName;
    if (hipTableLockExclusive(engine->record_block) != 0) return false;
    const bool ok = makeIndexHIP(engine, attributeName, attributeType);
    hipTableUnlockExclusive(engine->record_block);
    return ok;
}

int hipEngineProbeBoolIndexes(struct engineS *engine, int enable) {
    if (!engine || !engine->record_block) return -1;
    struct hipTable *t = engine->record_block;
    if (hipTableLockExclusive(t) != 0) return -1;                   /* no query in flight while the mode changes */
    const int before = t->probe_bool;
    t->probe_bool = enable != 0;
    hipTableUnlockExclusive(t);
    return before;
}

int hipEngineKernelTiming(struct engineS *engine, int enable) {
    if (!engine || !engine->record_block) return -1;
    struct hipTable *t = engine->record_block;
    int rc = 0;
    if (hipTableLockExclusive(t) != 0) return -1;                   /* no query in flight while the recorders are switched */
    for (int s = 0; s < hipTableShards(t) && rc == 0; s++)
        if (hipTableShard(t, s)->qs && pqps_qstream_set_timing(hipTableShard(t, s)->qs, enable) != PQPS_OK) rc = engine_error("kernel timing");
    hipTableUnlockExclusive(t);
    return rc;
}

int hipEngineKernelTime(struct engineS *engine, double *scan_ms, double *query_ms, int *launches) {
    if (!engine || !engine->record_block || !scan_ms || !query_ms || !launches) return -1;
    struct hipTable *t = engine->record_block;
    *scan_ms = 0.0; *query_ms = 0.0; *launches = 0;
    int rc = 0;
    if (hipTableLockExclusive(t) != 0) return -1;
    for (int s = 0; s < hipTableShards(t) && rc == 0; s++) {
        double e = 0.0, q = 0.0;
        int k = 0;
        if (!hipTableShard(t, s)->qs) continue;
        if (pqps_qstream_kernel_time(hipTableShard(t, s)->qs, &e, &q, &k) != PQPS_OK) { rc = engine_error("kernel timing"); break; }
        *scan_ms += e; *query_ms += q; *launches += k;
    }
    hipTableUnlockExclusive(t);
    return rc;
}

int hipEngineShards(struct engineS *engine, unsigned long long *rows, int capacity) {
    if (!engine || !engine->record_block) return 0;
    struct hipTable *t = engine->record_block;
    hipTableLockShared(t);
    const int n = hipTableShards(t);
    for (int s = 0; rows && s < n && s < capacity; s++) rows[s] = hipTableShard(t, s)->n_rows;
    hipTableUnlockShared(t);
    return n;
}

/* ---- mutation (kept in step with the CSV like the reference) ------------------------------ */

static void write_csv_row(FILE *f, const record *r) {           /* S:562, S:687 */
    fprintf(f, "%llu,%s,%s,%s,%d,%s,%d,%s,%d,%s,%s,%d\n", r->command_id, r->raw_command, r->base_command,
            r->shell_type, r->exit_code, r->timestamp, r->sudo_used, r->working_directory, r->user_id,
            r->user_name, r->host_name, r->risk_level);
}

/* executeQueryInsertSerial, S:538-617. */
/* The whole table as CSV text, rows formatted exactly like write_csv_row (S:687-700), by host
 * threads into per-range buffers that are then written in order: the rewrite after a DELETE is
 * the reference's own file format and by far the longest phase of a DELETE on a large table. */
struct csv_job { const record *rows; size_t begin, end; char *buf; size_t len; };

static char *put_u64(char *p, unsigned long long v) {
    char tmp[24];
    int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) *p++ = tmp[--k];
    return p;
}

static char *put_i32(char *p, int v) {
    unsigned long long u = v < 0 ? (unsigned long long)(-(long long)v) : (unsigned long long)v;
    if (v < 0) *p++ = '-';
    return put_u64(p, u);
}

static char *put_str(char *p, const char *s) {
    const size_t k = strlen(s);
    memcpy(p, s, k);
    return p + k;
}

static void *csv_format_rows(void *arg) {
    struct csv_job *j = arg;
    /* exact room: the strings as "%s" would print them (a field filled to its last byte has no NUL
     * and runs on into the next one, in the reference's fprintf as well) + 5 numbers + separators */
    size_t room = 1;
    for (size_t i = j->begin; i < j->end; i++) {
        const record *r = &j->rows[i];
        room += strlen(r->raw_command) + strlen(r->base_command) + strlen(r->shell_type) + strlen(r->timestamp) +
                strlen(r->working_directory) + strlen(r->user_name) + strlen(r->host_name) + 5 * 21 + 12;
    }
    j->buf = malloc(room);
    if (!j->buf) { j->len = 0; return NULL; }
    char *p = j->buf;
    for (size_t i = j->begin; i < j->end; i++) {
        const record *r = &j->rows[i];
        p = put_u64(p, r->command_id); *p++ = ',';
        p = put_str(p, r->raw_command); *p++ = ',';
        p = put_str(p, r->base_command); *p++ = ',';
        p = put_str(p, r->shell_type); *p++ = ',';
        p = put_i32(p, r->exit_code); *p++ = ',';
        p = put_str(p, r->timestamp); *p++ = ',';
        p = put_i32(p, (int)r->sudo_used); *p++ = ',';
        p = put_str(p, r->working_directory); *p++ = ',';
        p = put_i32(p, r->user_id); *p++ = ',';
        p = put_str(p, r->user_name); *p++ = ',';
        p = put_str(p, r->host_name); *p++ = ',';
        p = put_i32(p, r->risk_level); *p++ = '\n';
    }
    j->len = (size_t)(p - j->buf);
    return NULL;
}

static void write_csv_table(FILE *f, const record *rows, size_t n) {
    enum { kMaxJobs = 16, kChunkRows = 65536 };
    for (size_t base = 0; base < n; ) {                         /* bounded memory: <= 16 chunks in flight */
        struct csv_job job[kMaxJobs];
        pthread_t tid[kMaxJobs];
        int nj = 0;
        while (nj < kMaxJobs && base < n) {
            const size_t end = base + kChunkRows < n ? base + kChunkRows : n;
            job[nj] = (struct csv_job){ rows, base, end, NULL, 0 };
            base = end;
            nj++;
        }
        for (int k = 0; k < nj; k++)
            if (nj == 1 || pthread_create(&tid[k], NULL, csv_format_rows, &job[k]) != 0) { csv_format_rows(&job[k]); tid[k] = 0; }
        for (int k = 0; k < nj; k++) {
            if (nj > 1 && tid[k]) pthread_join(tid[k], NULL);
            if (job[k].buf) fwrite(job[k].buf, 1, job[k].len, f);
            else for (size_t i = job[k].begin; i < job[k].end; i++) write_csv_row(f, &rows[i]);   /* out of memory: plain path */
            free(job[k].buf);
        }
    }
}

/* n rows into the engine's CSV, opened in `mode`: "a" behind the rows it holds, "w" in their place (S:683-701: no header
 * written).  false: the file cannot be opened. */
static bool csv_write_rows(const struct engineS *engine, const char *mode, const record *rows, size_t n) {
    FILE *f = fopen(engine->datafile, mode);
    if (!f) return false;
    write_csv_table(f, rows, n);
    fclose(f);
    return true;
}

/* Room for `total` host rows in row_block and all_records[], all_records[i] == &row_block[i] for the rows there are.  The
 * store grows geometrically; all_records[] is re-pointed only when the block moved, and at once: the table is whole even
 * when the second allocation fails (-1, as when the first does). */
static int host_rows_reserve(struct engineS *engine, struct hipTable *t, size_t total) {
    if (total <= t->row_capacity) return 0;
    const size_t n = (size_t)engine->num_records, cap = total + total / 8 + 64;
    record *block = realloc(t->row_block, cap * sizeof *block);
    if (!block) return -1;
    if (block != t->row_block) for (size_t i = 0; i < n; i++) engine->all_records[i] = &block[i];
    t->row_block = block;
    record **rows = realloc(engine->all_records, cap * sizeof *rows);
    if (!rows) return -1;
    engine->all_records = rows;
    t->row_capacity = cap;
    return 0;
}

/* A writer's flags (DELETE: the rows that go, UPDATE: the rows that change): per shard on the device, where row_flags()
 * allocates them, and for the whole table on the host -- on an engine with host rows. */
struct writer_flags { uint8_t *dev[HIP_MAX_SHARDS], *host; };

static int writer_flags_host(struct writer_flags *wf, const struct hipTable *t, size_t n, const char *writer) {
    if (t->device_only) return 0;
    wf->host = malloc(n ? n : 1);
    if (!wf->host) { fprintf(stderr, "HIP engine: out of memory for %zu %s flags\n", n, writer); return -1; }
    return 0;
}

static void writer_flags_free(struct writer_flags *wf, struct hipTable *t) {
    for (int s = 0; s < hipTableShards(t); s++) if (wf->dev[s]) pqps_free(hipTableShard(t, s)->ctx, wf->dev[s]);
    free(wf->host);
    memset(wf, 0, sizeof *wf);
}

bool executeQueryInsertHIP(struct engineS *engine, const char *tableName, const record *r) {
    (void)tableName;
    if (r->command_id == 0 || !r->raw_command[0] || !r->base_command[0] || !r->shell_type[0] ||
        !r->timestamp[0] || !r->working_directory[0] || !r->user_name[0] || !r->host_name[0])
        return false;                                              /* S:544-551 */
    struct hipTable *t = engine->record_block;
    const double t0 = now_seconds();
    if (hipTableLockExclusive(t) != 0) return false;
    const size_t n = (size_t)engine->num_records;
    if (t->device_only) {
        /* no host rows, no CSV: the row goes to the device table alone */
        if (n + 1 > (size_t)INT_MAX) { hipTableUnlockExclusive(t); return false; }
        engine->num_records = (int)(n + 1);
        const bool ok = appendRowDeviceTableHIP(engine, r);
        if (!ok) {
            engine->num_records = (int)n;
            fprintf(stderr, "HIP engine: INSERT needs a table rebuild (head-room used up or a dictionary outgrowing its code width), which an engine without host rows cannot do\n");
        }
        TRACE("INSERT (device only): %.3f ms\n", (now_seconds() - t0) * 1e3);
        if (ok) value_sets_invalidate(t);
        hipTableUnlockExclusive(t);
        return ok;
    }
    /* room for the row first: a failed allocation must not leave the CSV one row ahead of the engine */
    if (host_rows_reserve(engine, t, n + 1) != 0 || !csv_write_rows(engine, "a", r, 1)) { hipTableUnlockExclusive(t); return false; }
    t->row_block[n] = *r;
    engine->all_records[n] = &t->row_block[n];
    engine->num_records = (int)(n + 1);
    const double t1 = now_seconds();
    appendRowDeviceTableHIP(engine, engine->all_records[n]);
    TRACE("INSERT: CSV append + host row %.3f ms, device append + indexes %.3f ms\n", (t1 - t0) * 1e3, (now_seconds() - t1) * 1e3);
    value_sets_invalidate(t);
    hipTableUnlockExclusive(t);
    return true;
}

/* executeQueryDeleteSerial, S:627-715: the per-row decision is the GPU flag
 * kernel (the flag-array shape of engine/omp/executeEngine-omp.c:708-732). */
/* Flags of the rows the bound WHERE of a writer's query selects (DELETE: the rows that go, UPDATE: the rows that change), per
 * shard on the device; `flags` (may be NULL: an engine without host rows) receives them for the whole table, *deleted their
 * number, per_shard[s] (may be NULL) each shard's. */
static int row_flags(struct query *q, size_t n, uint8_t **flags_dev, uint8_t *flags, uint64_t *deleted, uint64_t *per_shard) {
    struct hipTable *t = q->t;
    *deleted = 0;
    int rc = 0;
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(t, s);
        /* the passes in front of the last as for any query, the last pass as flags instead of a count */
        struct hipPlan head = q->plan;
        struct shard_pred *sp = &q->sp[s];
        memset(sp, 0, sizeof *sp);
        const struct hipPass *last = &head.pass[head.n_passes - 1];
        rc = head_passes(&head, t, s, sp, sh->ctx, NULL, sh->own.count_dev + 4, true);
        if (rc != 0) break;
        sp->pred = &last->pred;
        sp->n_cols = last->pred.n_columns;
        pass_columns(sh, last, sp, true, true, sp->cols);
        if (rc == 0 && pqps_malloc(sh->ctx, sh->capacity_rows, (void **)&flags_dev[s]) != PQPS_OK) rc = engine_error("flag allocation");
        if (rc == 0 && pqps_filter_flags(sh->ctx, sp->cols, sp->n_cols, sh->n_rows, sp->pred, flags_dev[s], sh->own.count_dev, NULL) != PQPS_OK)
            rc = engine_error("flag filter");
    }
    for (int s = 0; s < q->n_shards; s++) {
        struct hipTable *sh = hipTableShard(t, s);
        uint64_t k = 0;
        if (rc == 0 && pqps_ctx_sync(sh->ctx, NULL) != PQPS_OK) rc = engine_error("filter execution");
        if (rc == 0 && pqps_download(sh->ctx, &k, sh->own.count_dev, sizeof k, NULL) != PQPS_OK) rc = engine_error("count download");
        *deleted += k;
        if (per_shard) per_shard[s] = k;
        if (rc == 0 && sh->row0 + sh->n_rows > n) { fprintf(stderr, "HIP engine: device shards hold more rows than the engine\n"); rc = -1; }
        if (rc == 0 && flags && sh->n_rows && pqps_download(sh->ctx, flags + sh->row0, flags_dev[s], sh->n_rows, NULL) != PQPS_OK) rc = engine_error("flag download");
    }
    return rc;
}

struct resultSetS *executeQueryDeleteHIP(struct engineS *engine, const char *tableName,
                                         struct whereClauseS *whereClause) {
    (void)tableName;
    struct resultSetS *rs = calloc(1, sizeof *rs);
    if (!rs) { perror("Failed to allocate memory for result set"); exit(EXIT_FAILURE); }
    const double t0 = now_seconds();
    struct hipTable *t = engine->record_block;
    if (hipTableLockExclusive(t) != 0) { memset(rs, 0, sizeof *rs); rs->success = false; return rs; }
    const size_t n = (size_t)engine->num_records;
    struct writer_flags wf;
    memset(&wf, 0, sizeof wf);
    uint64_t flagged = 0;
    int rc = writer_flags_host(&wf, t, n, "delete");
    if (rc == 0) {
        struct query q;
        query_init(&q, engine, t, -1, true);                        /* the writer is alone: the table's own context and buffers */
        rc = bind_where(t, whereClause, &q.plan);
        if (rc == 0) { q.have_plan = true; rc = row_flags(&q, n, wf.dev, wf.host, &flagged, NULL); }
        query_free(&q);
    }
    if (rc != 0) {
        writer_flags_free(&wf, t);
        hipTableUnlockExclusive(t);
        rs->success = false;                                       /* nothing was deleted */
        return rs;
    }
    const double t1 = now_seconds();

    size_t keep = 0, deleted = 0;
    if (t->device_only) {                                           /* no host rows, no CSV */
        deleted = (size_t)flagged;
        keep = n - deleted;
        engine->num_records = (int)keep;
    } else {
        record *block = t->row_block;
        for (size_t i = 0; i < n; i++) {
            if (wf.host[i]) { deleted++; continue; }
            if (keep != i) block[keep] = block[i];
            keep++;
        }
        for (size_t i = 0; i < keep; i++) engine->all_records[i] = &block[i];
        engine->num_records = (int)keep;
    }
    const double t2 = now_seconds();

    if (!t->device_only) (void)csv_write_rows(engine, "w", t->row_block, keep);     /* a file that cannot be opened is left */
    const double t3 = now_seconds();
    /* device side: the same flags compact the 12 columns of every shard in place (order kept); dictionaries
     * stay as they are (a code without rows is harmless), indexes are re-sorted */
    if (deleted) compactDeviceTableHIP(engine, wf.dev, keep);
    writer_flags_free(&wf, t);
    TRACE("DELETE: %zu of %zu rows, flags %.3f ms, host rows %.3f ms, CSV rewrite %.3f ms, device compaction + indexes %.3f ms\n",
          deleted, n, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (now_seconds() - t3) * 1e3);
    value_sets_invalidate(t);
    hipTableUnlockExclusive(t);
    rs->numRecords = (int)deleted;
    rs->queryTime = now_seconds() - t0;
    rs->success = true;
    return rs;
}

/* ---- UPDATE SET ... WHERE (include/executeEngine-hip.h) -------------------------------------------------------------- */

static void assign_host_row(record *r, const struct hipAssignment *a, int n) {
    for (int i = 0; i < n; i++) {
        switch (a[i].column) {
        case HIPCOL_COMMAND_ID: r->command_id = a[i].value; break;
        case HIPCOL_EXIT_CODE: r->exit_code = (int)(uint32_t)a[i].value; break;
        case HIPCOL_USER_ID: r->user_id = (int)(uint32_t)a[i].value; break;
        case HIPCOL_RISK_LEVEL: r->risk_level = (int)(uint32_t)a[i].value; break;
        case HIPCOL_SUDO_USED: r->sudo_used = a[i].value != 0; break;
        case HIPCOL_RAW_COMMAND: strncpy(r->raw_command, a[i].text, sizeof r->raw_command); break;
        case HIPCOL_BASE_COMMAND: strncpy(r->base_command, a[i].text, sizeof r->base_command); break;
        case HIPCOL_SHELL_TYPE: strncpy(r->shell_type, a[i].text, sizeof r->shell_type); break;
        case HIPCOL_TIMESTAMP: strncpy(r->timestamp, a[i].text, sizeof r->timestamp); break;
        case HIPCOL_WORKING_DIRECTORY: strncpy(r->working_directory, a[i].text, sizeof r->working_directory); break;
        case HIPCOL_USER_NAME: strncpy(r->user_name, a[i].text, sizeof r->user_name); break;
        case HIPCOL_HOST_NAME: strncpy(r->host_name, a[i].text, sizeof r->host_name); break;
        default: break;
        }
    }
}

/* The fused route: the WHERE of one scan pass and the stores, ONE launch per shard on the table's own context. */
static int update_fused(struct query *q, const struct hipAssignment *a, int n, uint64_t *matched) {
    const struct hipPass *pass = &q->plan.pass[0];
    int rc = 0;
    for (int s = 0; s < q->n_shards && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        pqps_column cols[PQPS_MAX_COLUMNS];
        pqps_assign_target targets[PQPS_MAX_COLUMNS];
        pass_columns(sh, pass, NULL, true, false, cols);
        const int k = updateTargetsHIP(sh, a, n, targets);
        if (k == 0) {                                               /* nothing to store: the rows are counted all the same */
            if (pqps_filter_count(sh->ctx, cols, pass->pred.n_columns, sh->n_rows, &pass->pred, sh->own.count_dev, NULL) != PQPS_OK)
                rc = engine_error("count filter");
        } else if (pqps_filter_assign(sh->ctx, cols, pass->pred.n_columns, sh->n_rows, &pass->pred, targets, (uint32_t)k, sh->own.count_dev,
                                      NULL) != PQPS_OK)
            rc = engine_error("filter and assign");
    }
    /* every shard that was launched on is waited for, whatever another one returned */
    for (int s = 0; s < q->n_shards; s++) {
        struct hipTable *sh = hipTableShard(q->t, s);
        if (pqps_ctx_sync(sh->ctx, NULL) != PQPS_OK && rc == 0) rc = engine_error("filter and assign");
        if (rc == 0 && pqps_download(sh->ctx, &matched[s], sh->own.count_dev, sizeof matched[s], NULL) != PQPS_OK) rc = engine_error("count download");
    }
    return rc;
}

/* The stores of the flags route, by the flags row_flags() left on every shard. */
static int update_by_flags(struct hipTable *t, const struct hipAssignment *a, int n, uint8_t *const *flags_dev, const uint64_t *matched) {
    int rc = 0;
    for (int s = 0; s < hipTableShards(t) && rc == 0; s++) {
        struct hipTable *sh = hipTableShard(t, s);
        pqps_assign_target targets[PQPS_MAX_COLUMNS];
        const int k = updateTargetsHIP(sh, a, n, targets);
        if (k && matched[s] && pqps_assign_flags(sh->ctx, flags_dev[s], sh->n_rows, targets, (uint32_t)k, NULL) != PQPS_OK)
            rc = engine_error("assign by flags");
    }
    for (int s = 0; s < hipTableShards(t); s++)
        if (pqps_ctx_sync(hipTableShard(t, s)->ctx, NULL) != PQPS_OK && rc == 0) rc = engine_error("assign by flags");
    return rc;
}

static long long update_locked(struct engineS *engine, struct hipTable *t, const char *const *setColumns, const char *const *setValues, int numSet,
                               struct whereClauseS *whereClause) {
    const double t0 = now_seconds();
    if (t->xch) {
        fprintf(stderr, "HIP engine: UPDATE is refused on an engine joined across ranks\n");
        return -1;
    }
    /* 1. the SET list, and whether it can be made in place */
    struct hipSchema schema;
    struct hipAssignment a[PQPS_MAX_COLUMNS];
    hipSchemaOfTable(t, &schema);
    if (hipCompileAssignments(&schema, setColumns, setValues, numSet, a) != 0) return -1;
    const bool rebuild = updateNeedsRebuildHIP(engine, a, numSet);
    if (rebuild && t->device_only) {
        fprintf(stderr, "HIP engine: UPDATE needs a table rebuild (a dictionary outgrowing its code width, or a second value for a column "
                        "without a device buffer), which an engine without host rows cannot do\n");
        return -1;
    }
    const size_t n = (size_t)engine->num_records;
    const int n_shards = hipTableShards(t);
    /* 2. new strings into their dictionaries, before the WHERE is bound: its constants are codes */
    const uint32_t bumped = rebuild ? 0u : updateInsertStringsHIP(engine, a, numSet);
    if (bumped) value_sets_invalidate(t);                            /* codes moved: the sets are stale whatever becomes of the rows */
    const double t1 = now_seconds();

    /* 3. the rows */
    uint64_t matched[HIP_MAX_SHARDS];
    struct writer_flags wf;
    memset(matched, 0, sizeof matched);
    memset(&wf, 0, sizeof wf);
    uint64_t total = 0;
    bool fused = false;
    struct query q;
    query_init(&q, engine, t, -1, true);                            /* the writer is alone: the table's own context and buffers */
    int rc = bind_where(t, whereClause, &q.plan);
    if (rc == 0) {
        q.have_plan = true;
        fused = t->device_only && q.plan.n_passes == 1;
        if (fused) {
            rc = update_fused(&q, a, numSet, matched);
            for (int s = 0; s < n_shards; s++) total += matched[s];
        } else {
            rc = writer_flags_host(&wf, t, n, "update");
            if (rc == 0) rc = row_flags(&q, n, wf.dev, wf.host, &total, matched);
        }
        TRACE("UPDATE: %s route, %llu of %zu rows\n", fused ? "fused" : "flags", (unsigned long long)total, n);
    }
    query_free(&q);
    const double t2 = now_seconds();
    if (rc != 0) memset(matched, 0, sizeof matched);               /* (nothing was stored: the flags route stores below) */

    /* host rows and the CSV, as after a DELETE */
    double t3 = t2;
    if (rc == 0 && !t->device_only && total) {
        for (size_t i = 0; i < n; i++)
            if (wf.host[i]) assign_host_row(&t->row_block[i], a, numSet);
        (void)csv_write_rows(engine, "w", t->row_block, n);        /* a file that cannot be opened is left */
        t3 = now_seconds();
    }

    /* the stores of the flags route, or the rebuild from the updated host rows.  A device step that fails after the host rows
     * and the CSV have changed is fatal, as in INSERT / DELETE. */
    if (rc == 0 && !fused && total && !rebuild && update_by_flags(t, a, numSet, wf.dev, matched) != 0) {
        if (!t->device_only) exit(EXIT_FAILURE);
        rc = -1;
    }
    writer_flags_free(&wf, t);
    /* 4. plane, bounds, indexes (bumped codes are keys of indexes whatever became of the WHERE) */
    if (rebuild) { if (rc == 0 && total) rebuildDeviceTableHIP(engine); }
    else finishUpdateDeviceTableHIP(engine, a, numSet, matched, bumped);
    TRACE("UPDATE: SET list + dictionaries %.3f ms, rows %.3f ms, host rows + CSV %.3f ms, device stores + plane + indexes %.3f ms\n",
          (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (now_seconds() - t3) * 1e3);
    return rc == 0 ? (long long)total : -1;
}

long long executeQueryUpdateHIP(struct engineS *engine, const char *tableName, const char *const *setColumns, const char *const *setValues,
                                int numSet, struct whereClauseS *whereClause, double *queryTime) {
    (void)tableName;
    if (!engine || !engine->record_block) return -1;
    const double t0 = now_seconds();
    struct hipTable *t = engine->record_block;
    if (hipTableLockExclusive(t) != 0) return -1;
    const long long k = update_locked(engine, t, setColumns, setValues, numSet, whereClause);
    if (k >= 0) value_sets_invalidate(t);
    hipTableUnlockExclusive(t);
    if (queryTime) *queryTime = now_seconds() - t0;
    return k;
}


/* ---- batch INSERT: any number of rows in one call (include/executeEngine-hip.h) --------------------------------------- */

/* the writer's gate of both forms: -1 with the lock NOT held */
static int insert_batch_enter(struct engineS *engine, struct hipTable **t_out) {
    if (!engine || !engine->record_block) return -1;
    struct hipTable *t = engine->record_block;
    if (hipTableLockExclusive(t) != 0) return -1;
    if (t->xch) {
        fprintf(stderr, "HIP engine: batch INSERT is refused on an engine joined across ranks\n");
        hipTableUnlockExclusive(t);
        return -1;
    }
    *t_out = t;
    return 0;
}

long long executeQueryInsertColumnsHIP(struct engineS *engine, const char *tableName, unsigned long long num_rows,
                                       const struct hipColumnData columns[12], double *queryTime) {
    (void)tableName;
    const double t0 = now_seconds();
    struct hipTable *t = NULL;
    if (insert_batch_enter(engine, &t) != 0) return -1;
    long long k = -1;
    if (!t->device_only) {
        fprintf(stderr, "HIP engine: batch INSERT of columns is for engines without host rows; this one keeps rows and a CSV in step: use the rows form\n");
    } else if (num_rows == 0) {
        k = 0;
    } else {
        struct hipAppend *b = prepareAppendColumnsHIP(engine, num_rows, columns);
        const double t1 = now_seconds();
        if (b) {
            commitAppendHIP(engine, b);
            k = (long long)num_rows;
            TRACE("INSERT of %llu rows: merge + staging %.3f ms, remap + append + indexes %.3f ms\n", num_rows, (t1 - t0) * 1e3, (now_seconds() - t1) * 1e3);
        }
    }
    if (k >= 0) value_sets_invalidate(t);
    hipTableUnlockExclusive(t);
    if (queryTime) *queryTime = now_seconds() - t0;
    return k;
}

long long executeQueryInsertRowsHIP(struct engineS *engine, const char *tableName, const record *rows, unsigned long long num_rows,
                                    double *queryTime) {
    (void)tableName;
    const double t0 = now_seconds();
    struct hipTable *t = NULL;
    if (insert_batch_enter(engine, &t) != 0) return -1;
    long long k = -1;
    struct hipAppend *b = NULL;
    if (num_rows == 0) k = 0;
    else if (!rows) fprintf(stderr, "HIP engine: batch INSERT: no rows\n");
    else b = prepareAppendRowsHIP(engine, rows, num_rows);
    if (b && !t->device_only) {
        /* the host rows and the CSV, as B single INSERTs leave them: room first, then the file, then the rows */
        const size_t n = (size_t)engine->num_records, total = n + (size_t)num_rows;
        if (host_rows_reserve(engine, t, total) != 0 || !csv_write_rows(engine, "a", rows, (size_t)num_rows)) {
            fprintf(stderr, "HIP engine: batch INSERT: no room for the host rows, or the CSV cannot be appended to\n");
            discardAppendHIP(engine, b);
            b = NULL;
        } else {
            memcpy(&t->row_block[n], rows, (size_t)num_rows * sizeof *rows);
            for (size_t i = n; i < total; i++) engine->all_records[i] = &t->row_block[i];
        }
    }
    if (b) {
        commitAppendHIP(engine, b);
        k = (long long)num_rows;
    }
    if (k >= 0) value_sets_invalidate(t);
    hipTableUnlockExclusive(t);
    if (queryTime) *queryTime = now_seconds() - t0;
    return k;
}
