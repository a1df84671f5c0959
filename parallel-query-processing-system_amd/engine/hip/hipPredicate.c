/* hipPredicate.c -- WHERE list -> pqps_predicate (see include/hipPredicate.h).
 *
 * Semantics follow the reference's serial evaluator
 * (engine/serial/executeEngine-serial.c, "S" below); nothing here touches the
 * GPU and nothing here evaluates rows: it only decides, per leaf, which
 * unsigned window of column values makes the leaf true.
 */
#define _POSIX_C_SOURCE 200809L
#include "hipPredicate.h"
#include "logType.h"

#include <errno.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#define T_ACCEPT (-1)
#define T_REJECT (-2)
#define MAX_RAW_STEPS 512

enum { ST_LEAF = 0, ST_FALSE = 1, ST_TRUE = 2 };

struct step {
    int kind;
    int col;                 /* HIPCOL id */
    uint64_t lo, span;
    int neg;
    int t, f;                /* raw step index, T_ACCEPT or T_REJECT */
};

static const char *const k_names[PQPS_MAX_COLUMNS] = {
    "command_id", "raw_command", "base_command", "shell_type", "exit_code", "timestamp",
    "sudo_used", "working_directory", "user_id", "user_name", "host_name", "risk_level"
};

int hipColumnId(const char *name) {
    if (!name) return -1;
    for (int i = 0; i < PQPS_MAX_COLUMNS; i++)
        if (strcmp(name, k_names[i]) == 0) return i;
    return -1;
}

/* S:131-136 */
static int op_code(const char *op) {
    if (!op) return -1;
    if (strcmp(op, "=") == 0) return 0;
    if (strcmp(op, "!=") == 0) return 1;
    if (strcmp(op, ">") == 0) return 2;
    if (strcmp(op, "<") == 0) return 3;
    if (strcmp(op, ">=") == 0) return 4;
    if (strcmp(op, "<=") == 0) return 5;
    return -1;
}

/* Window of an ordered unsigned domain [0, max] for `x OP v`. */
static void window_unsigned(struct step *s, int op, uint64_t v, uint64_t max) {
    s->kind = ST_LEAF;
    s->neg = 0;
    switch (op) {
    case 0: s->lo = v; s->span = 0; break;
    case 1: s->lo = v; s->span = 0; s->neg = 1; break;
    case 2: if (v >= max) s->kind = ST_FALSE; else { s->lo = v + 1; s->span = max - (v + 1); } break;
    case 3: if (v == 0) s->kind = ST_FALSE; else { s->lo = 0; s->span = v - 1; } break;
    case 4: if (v > max) s->kind = ST_FALSE; else { s->lo = v; s->span = max - v; } break;
    default: s->lo = 0; s->span = v > max ? max : v; break;
    }
}

/* Signed 32-bit column: windows on the two's-complement bit pattern, all
 * arithmetic mod 2^32 (the kernel tests (x - lo) <= span in u32). */
static void window_i32(struct step *s, int op, int v) {
    const uint32_t uv = (uint32_t)v, umin = 0x80000000u, umax = 0x7FFFFFFFu;
    s->kind = ST_LEAF;
    s->neg = 0;
    switch (op) {
    case 0: s->lo = uv; s->span = 0; break;
    case 1: s->lo = uv; s->span = 0; s->neg = 1; break;
    case 2: if (v == INT_MAX) s->kind = ST_FALSE; else { s->lo = uv + 1u; s->span = (uint32_t)(umax - (uv + 1u)); } break;
    case 3: if (v == INT_MIN) s->kind = ST_FALSE; else { s->lo = umin; s->span = (uint32_t)((uv - 1u) - umin); } break;
    case 4: s->lo = uv; s->span = (uint32_t)(umax - uv); break;
    default: s->lo = umin; s->span = (uint32_t)(uv - umin); break;
    }
    s->lo &= 0xFFFFFFFFull;
    s->span &= 0xFFFFFFFFull;
}

int hipDictionaryRank(const char *const *values, int count, const char *text, int *present) {
    int l = 0, r = count;
    while (l < r) { const int m = l + (r - l) / 2; if (strcmp(values[m], text) < 0) l = m + 1; else r = m; }
    *present = l < count && strcmp(values[l], text) == 0;
    return l;
}

/* String column as order-preserving codes: strcmp(field, lit) OP 0 (S:23-26)
 * rewritten on ranks.  lb = #values < lit, ub = #values <= lit. */
static void window_dict(struct step *s, int op, const char *lit, const struct hipColumnInfo *ci) {
    int present;
    const int lb = hipDictionaryRank(ci->dict, ci->dict_count, lit, &present), ub = lb + present;
    const uint64_t top = 0xFFFFFFFFull;
    s->kind = ST_LEAF;
    s->neg = 0;
    switch (op) {
    case 0: if (!present) s->kind = ST_FALSE; else { s->lo = (uint64_t)lb; s->span = 0; } break;
    case 1: if (!present) s->kind = ST_TRUE; else { s->lo = (uint64_t)lb; s->span = 0; s->neg = 1; } break;
    case 2: s->lo = (uint64_t)ub; s->span = top - (uint64_t)ub; break;                 /* code >= ub */
    case 3: if (lb == 0) s->kind = ST_FALSE; else { s->lo = 0; s->span = (uint64_t)lb - 1; } break;   /* code < lb */
    case 4: s->lo = (uint64_t)lb; s->span = top - (uint64_t)lb; break;                 /* code >= lb */
    default: if (ub == 0) s->kind = ST_FALSE; else { s->lo = 0; s->span = (uint64_t)ub - 1; } break;  /* code < ub */
    }
}

/* Result flags of an earlier pass of a multi-pass plan, bound like a 1-byte column: its column id is
 * PQPS_MAX_COLUMNS + pass number, its leaf is `flags = 1`.  The planner names it "\x01<pass>". */
#define FLAG_ATTRIBUTE '\x01'
static const struct hipColumnInfo k_flag_column = { 1, HIPKIND_BOOL, 1, 0, NULL };

static const struct hipColumnInfo *col_info(const struct hipSchema *schema, int col) {
    return col >= PQPS_MAX_COLUMNS ? &k_flag_column : &schema->col[col];
}

/* Flag leaves exist only inside hipCompileWherePlan: the planner makes them (make_flag_leaf: the name "\x01<pass>" AND
 * the mark in value_type), and only passes that exist can be named -- `flag_passes` = the passes emitted so far
 * while the planner runs on the calling thread, 0 otherwise.  A caller-supplied list that names "\x01<n>" (the engine
 * API takes whereClauseS lists from anybody) is an unknown attribute like any other, never an index into flag
 * buffers that do not exist. */
#define FLAG_MARK 0x7F1A6
static _Thread_local int flag_passes;

struct set_node;
static const struct set_node *find_set(const struct whereClauseS *c);
static int set_node_column(const struct set_node *sn);
static int set_node_leaves(const struct set_node *sn);

/* The column a leaf node reads: a table column, or the flags of an earlier pass -- for a flag leaf of the planner, and for
 * a set node that became a member pass. */
static int node_column(const struct whereClauseS *c) {
    if (c->attribute && c->attribute[0] == FLAG_ATTRIBUTE) {
        const int pass = atoi(c->attribute + 1);
        return c->value_type == FLAG_MARK && pass >= 0 && pass < flag_passes ? PQPS_MAX_COLUMNS + pass : -1;
    }
    const struct set_node *sn = find_set(c);
    if (sn) return set_node_column(sn);
    return hipColumnId(c->attribute);
}

/* comparisons a leaf node compiles to: a set node of several runs is that many window leaves */
static int node_leaves(const struct whereClauseS *c) {
    const struct set_node *sn = find_set(c);
    return sn ? set_node_leaves(sn) : 1;
}


/* ---- set predicates: LIKE / NOT LIKE / IN / NOT IN (no counterpart in the reference) -------------------------------
 * A set node is decided on the host, once per distinct value of its column, BEFORE leaves are counted and passes are
 * planned: resolve_sets leaves one entry per node in a side table, the sorted runs of codes / values the node selects.
 * A set of few runs becomes that many ordinary window leaves, anything more fragmented a member pass of the plan whose
 * flags the node reads as the leaf `flags = 1` (include/hipPredicate.h). */
enum { SET_LIKE = 0, SET_NOT_LIKE = 1, SET_IN = 2, SET_NOT_IN = 3, SET_IN_SET = 4, SET_NOT_IN_SET = 5 };
static int set_op_code(const char *op) {
    if (!op) return -1;
    if (strcmp(op, "LIKE") == 0) return SET_LIKE;
    if (strcmp(op, "NOT LIKE") == 0) return SET_NOT_LIKE;
    if (strcmp(op, "IN") == 0) return SET_IN;
    if (strcmp(op, "NOT IN") == 0) return SET_NOT_IN;
    if (strcmp(op, "IN SET") == 0) return SET_IN_SET;
    if (strcmp(op, "NOT IN SET") == 0) return SET_NOT_IN_SET;
    return -1;
}

int hipIsSetOperator(const char *op) { return set_op_code(op) >= 0; }

enum { SM_FALSE = 0, SM_TRUE = 1, SM_WINDOWS = 2, SM_MEMBER = 3, SM_ABSENT = 4 };
struct set_node {
    const char *attribute, *operator, *value;   /* the node's identity: what a copy of the node keeps (fit_chain copies) */
    int col, mode;
    int negate;                                  /* windows: every leaf negated (an AND ladder); member: the flag leaf negated */
    int n_runs;
    uint64_t lo[PQPS_MEMBER_MAX_RUNS], span[PQPS_MEMBER_MAX_RUNS];
    int pass;                                    /* SM_MEMBER: the pass that leaves the flags, -1 until it is emitted */
    int form;
    uint32_t base;
    uint64_t n_bits;
    uint32_t *bitmap;
    uint64_t *list;
    uint32_t n_list;
    uint32_t set_id;                             /* a value set (IN SET): its id; the bitmap is the set's own, on the device */
};
struct set_table { struct set_node *node; int n, cap; };
static _Thread_local const struct set_table *sets;   /* the table of the compile running on this thread */
/* ... and the value sets it may name (hipCompileWherePlanSets) */
static _Thread_local const struct hipSetInfo *value_sets;
static _Thread_local int n_value_sets;

static const struct set_node *find_set(const struct whereClauseS *c) {
    if (!sets || c->sub) return NULL;
    for (int i = 0; i < sets->n; i++) {
        const struct set_node *sn = &sets->node[i];
        if (sn->attribute == c->attribute && sn->operator == c->operator && sn->value == c->value) return sn;
    }
    return NULL;
}

static void set_table_free(struct set_table *T) {
    for (int i = 0; i < T->n; i++) { free(T->node[i].bitmap); free(T->node[i].list); }
    free(T->node);
    memset(T, 0, sizeof *T);
}

static int set_fail(char *err, size_t errlen, const char *attribute, const char *what) {
    if (err) snprintf(err, errlen, "%s: %s", attribute, what);
    return -1;
}

static int is_blank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

/* `( item, item, ... )` -> malloc'd strings.  An item is a single-quoted string ('' is a quote inside it) or a bare
 * token with the white space around it trimmed. */
static int parse_in_list(const char *attribute, const char *value, char ***items_out, int *n_out, char *err, size_t errlen) {
    *items_out = NULL; *n_out = 0;
    const char *q = value, *e = value + strlen(value);
    while (q < e && is_blank(*q)) q++;
    while (e > q && is_blank(e[-1])) e--;
    if (e - q < 2 || *q != '(' || e[-1] != ')') return set_fail(err, errlen, attribute, "IN needs a parenthesised list");
    q++; e--;
    char **items = NULL;
    int n = 0, cap = 0, rc = 0;
    char *buf = malloc((size_t)(e - q) + 1);
    if (!buf) return set_fail(err, errlen, attribute, "out of memory");
    while (q < e && is_blank(*q)) q++;
    while (q < e) {                                                    /* (an interior of blanks only: the empty list) */
        size_t len = 0;
        while (q < e && is_blank(*q)) q++;
        if (q < e && *q == '\'') {
            q++;
            for (;;) {
                if (q >= e) { rc = set_fail(err, errlen, attribute, "unterminated quote in IN list"); break; }
                if (*q == '\'') { if (q + 1 < e && q[1] == '\'') { buf[len++] = '\''; q += 2; continue; } q++; break; }
                buf[len++] = *q++;
            }
            if (rc) break;
            while (q < e && is_blank(*q)) q++;
            if (q < e && *q != ',') { rc = set_fail(err, errlen, attribute, "malformed IN list"); break; }
        } else {
            const char *start = q;
            while (q < e && *q != ',') q++;
            const char *stop = q;
            while (stop > start && is_blank(stop[-1])) stop--;
            if (stop == start) { rc = set_fail(err, errlen, attribute, "empty item in IN list"); break; }
            len = (size_t)(stop - start);
            memcpy(buf, start, len);
        }
        if (n == PQPS_MEMBER_MAX_ITEMS) { rc = set_fail(err, errlen, attribute, "IN list has more than 65536 items"); break; }
        if (n == cap) {
            cap = cap ? 2 * cap : 16;
            char **grown = realloc(items, (size_t)cap * sizeof *grown);
            if (!grown) { rc = set_fail(err, errlen, attribute, "out of memory"); break; }
            items = grown;
        }
        items[n] = malloc(len + 1);
        if (!items[n]) { rc = set_fail(err, errlen, attribute, "out of memory"); break; }
        memcpy(items[n], buf, len);
        items[n++][len] = '\0';
        if (q == e) break;
        q++;                                                          /* the comma: another item has to follow */
        if (q == e) { rc = set_fail(err, errlen, attribute, "empty item in IN list"); break; }
    }
    free(buf);
    if (rc) { for (int i = 0; i < n; i++) free(items[i]); free(items); return rc; }
    *items_out = items; *n_out = n;
    return 0;
}

/* LIKE pattern as tokens: kind 0 = the literal byte lit[i], 1 = `_`, 2 = `%`.  `\%`, `\_` and `\\` are literals; a
 * backslash in front of anything else, or at the end, is itself a literal backslash. */
static int like_tokens(const char *pat, uint8_t *kind, unsigned char *lit) {
    int m = 0;
    for (const unsigned char *p = (const unsigned char *)pat; *p; p++) {
        if (*p == '\\' && (p[1] == '%' || p[1] == '_' || p[1] == '\\')) { kind[m] = 0; lit[m++] = *++p; }
        else if (*p == '%') { kind[m] = 2; lit[m++] = 0; }
        else if (*p == '_') { kind[m] = 1; lit[m++] = 0; }
        else { kind[m] = 0; lit[m++] = *p; }
    }
    return m;
}

/* whole-string match, byte-wise; `%` backtracks to the latest one only (enough for this grammar) */
static int like_match(const unsigned char *s, const uint8_t *kind, const unsigned char *lit, int m) {
    int i = 0, star = -1;
    const unsigned char *resume = NULL;
    while (*s) {
        if (i < m && (kind[i] == 1 || (kind[i] == 0 && lit[i] == *s))) { i++; s++; }
        else if (i < m && kind[i] == 2) { star = i++; resume = s; }
        else if (star >= 0) { i = star + 1; s = ++resume; }
        else return 0;
    }
    while (i < m && kind[i] == 2) i++;
    return i == m;
}

struct runs { uint64_t *lo, *hi; size_t n, cap; };               /* ascending, disjoint, not adjacent; inclusive ends */
static int runs_add(struct runs *r, uint64_t v) {                 /* values arrive ascending (duplicates allowed) */
    if (r->n && (r->hi[r->n - 1] == v || r->hi[r->n - 1] + 1 == v)) { r->hi[r->n - 1] = v; return 0; }
    if (r->n == r->cap) {
        const size_t cap = r->cap ? 2 * r->cap : 16;
        uint64_t *lo = realloc(r->lo, cap * sizeof *lo);
        if (lo) r->lo = lo;
        uint64_t *hi = realloc(r->hi, cap * sizeof *hi);
        if (hi) r->hi = hi;
        if (!lo || !hi) return -1;
        r->cap = cap;
    }
    r->lo[r->n] = v; r->hi[r->n++] = v;
    return 0;
}

static int cmp_u64(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

/* rank of the first dictionary entry whose first `len` bytes are >= (upper == 0) or > (upper != 0) `prefix` */
static int prefix_bound(const struct hipColumnInfo *ci, const unsigned char *prefix, size_t len, int upper) {
    int l = 0, r = ci->dict_count;
    while (l < r) {
        const int m = l + (r - l) / 2;
        const int c = strncmp(ci->dict[m], (const char *)prefix, len);
        if (upper ? c <= 0 : c < 0) l = m + 1; else r = m;
    }
    return l;
}

/* Marks the codes a LIKE pattern selects.  The literal bytes in front of the first wildcard give a code window (the codes
 * are order-preserving: the strings with that prefix are neighbours); only its strings are matched, and none at all when
 * nothing but `%` follows the literal. */
static int like_marks(const struct hipColumnInfo *ci, const char *pattern, uint8_t *mark) {
    const size_t plen = strlen(pattern);
    uint8_t *kind = malloc(plen + 1);
    unsigned char *lit = malloc(plen + 1);
    if (!kind || !lit) { free(kind); free(lit); return -1; }
    const int m = like_tokens(pattern, kind, lit);
    int prefix = 0, rest_any = 1;
    while (prefix < m && kind[prefix] == 0) prefix++;
    for (int i = prefix; i < m; i++) if (kind[i] != 2) rest_any = 0;
    const int first = prefix_bound(ci, lit, (size_t)prefix, 0), end = prefix_bound(ci, lit, (size_t)prefix, 1);
    for (int c = first; c < end; c++) {
        if (prefix == m) mark[c] = strlen(ci->dict[c]) == (size_t)m;      /* no wildcard: the string itself */
        else mark[c] = rest_any ? 1 : (uint8_t)like_match((const unsigned char *)ci->dict[c], kind, lit, m);
    }
    free(kind); free(lit);
    return 0;
}

/* From the runs of the set S (keys in [0, dmax], an order-preserving image of the column's values; `unbias` turns a key
 * back into the pattern the kernels compare) to the node's form.  The set's own runs are taken when they are at most
 * PQPS_MEMBER_MAX_RUNS -- `a IN (x, y)` is then exactly `a = x OR a = y` -- else those of its complement in the domain. */
static int set_from_runs(struct set_node *sn, const struct runs *S, uint64_t dmax, uint64_t unbias, int not_form, int kind) {
    if (S->n == 0) { sn->mode = not_form ? SM_TRUE : SM_FALSE; return 0; }
    if (S->n == 1 && S->lo[0] == 0 && S->hi[0] == dmax) { sn->mode = not_form ? SM_FALSE : SM_TRUE; return 0; }
    const uint64_t mask = kind == HIPKIND_U64 ? UINT64_MAX : 0xFFFFFFFFull;
    const int head = S->lo[0] != 0, tail = S->hi[S->n - 1] != dmax;
    const size_t n_gaps = S->n - 1 + (size_t)head + (size_t)tail;
    if (S->n <= PQPS_MEMBER_MAX_RUNS) {
        sn->mode = SM_WINDOWS; sn->negate = not_form; sn->n_runs = (int)S->n;
        for (size_t i = 0; i < S->n; i++) { sn->lo[i] = (S->lo[i] ^ unbias) & mask; sn->span[i] = S->hi[i] - S->lo[i]; }
        return 0;
    }
    if (n_gaps <= PQPS_MEMBER_MAX_RUNS) {
        sn->mode = SM_WINDOWS; sn->negate = !not_form; sn->n_runs = 0;
        for (size_t i = 0; i <= S->n; i++) {
            if ((i == 0 && !head) || (i == S->n && !tail)) continue;
            const uint64_t lo = i == 0 ? 0 : S->hi[i - 1] + 1, hi = i == S->n ? dmax : S->lo[i] - 1;
            sn->lo[sn->n_runs] = (lo ^ unbias) & mask; sn->span[sn->n_runs++] = hi - lo;
        }
        return 0;
    }
    sn->mode = SM_MEMBER; sn->negate = not_form; sn->pass = -1;
    const uint64_t extent = S->hi[S->n - 1] - S->lo[0];                /* keys the bitmap would span, minus one */
    if (kind != HIPKIND_U64 && extent < PQPS_MEMBER_MAX_BITS) {
        sn->form = PQPS_MEMBER_BITMAP;
        sn->base = (uint32_t)(S->lo[0] ^ unbias);
        sn->n_bits = extent + 1;
        sn->bitmap = calloc((size_t)((sn->n_bits + 31) / 32), sizeof *sn->bitmap);
        if (!sn->bitmap) return -1;
        for (size_t i = 0; i < S->n; i++)
            for (uint64_t k = S->lo[i] - S->lo[0]; k <= S->hi[i] - S->lo[0]; k++) sn->bitmap[k >> 5] |= 1u << (k & 31);
        return 0;
    }
    sn->form = PQPS_MEMBER_LIST;                                        /* (numeric columns only: at most PQPS_MEMBER_MAX_ITEMS values) */
    size_t total = 0;
    for (size_t i = 0; i < S->n; i++) total += (size_t)(S->hi[i] - S->lo[i]) + 1;
    sn->list = malloc(total * sizeof *sn->list);
    if (!sn->list) return -1;
    sn->n_list = 0;
    for (size_t i = 0; i < S->n; i++)
        for (uint64_t k = S->lo[i]; ; k++) { sn->list[sn->n_list++] = (k ^ unbias) & mask; if (k == S->hi[i]) break; }
    qsort(sn->list, sn->n_list, sizeof *sn->list, cmp_u64);             /* an i32 column: by its u32 bit pattern, as the kernel searches */
    return 0;
}

/* IN SET / NOT IN SET: the node's value names a value set of the table (include/hipPredicate.h). */
static int resolve_value_set(const struct whereClauseS *c, int not_form, int col, int kind, struct set_node *sn, char *err, size_t errlen) {
    char *end = NULL;
    const unsigned long long id = c->value[0] >= '0' && c->value[0] <= '9' ? strtoull(c->value, &end, 10) : 0;
    if (!end || *end || id == 0 || id > 0xFFFFFFFFull) return set_fail(err, errlen, c->attribute, "IN SET needs the decimal id of a value set");
    const struct hipSetInfo *si = NULL;
    for (int i = 0; i < n_value_sets && !si; i++) if (value_sets[i].id == (uint32_t)id) si = &value_sets[i];
    if (!si) return set_fail(err, errlen, c->attribute, "IN SET names a value set that does not exist (never made, or freed)");
    if (si->stale) return set_fail(err, errlen, c->attribute, "IN SET names a stale value set: the table was written after the set was made");
    if (kind == HIPKIND_U64 || kind == HIPKIND_BOOL) return set_fail(err, errlen, c->attribute, "command_id and sudo_used take no value set");
    if (kind != si->kind || (kind == HIPKIND_DICT && col != si->column))
        return set_fail(err, errlen, c->attribute, "the value set is over another column: a string column takes only its own sets, an i32 column those of i32 columns");
    if (si->members == 0) { sn->mode = not_form ? SM_TRUE : SM_FALSE; return 0; }
    if (kind == HIPKIND_DICT && si->members == si->n_bits) { sn->mode = not_form ? SM_FALSE : SM_TRUE; return 0; }
    sn->mode = SM_MEMBER;
    sn->negate = not_form;
    sn->form = PQPS_MEMBER_BITMAP;
    sn->base = si->base;
    sn->n_bits = si->n_bits;
    sn->set_id = si->id;
    return 0;
}

static int resolve_one(const struct hipSchema *schema, const struct whereClauseS *c, int op, int col, struct set_node *sn,
                       char *err, size_t errlen) {
    const struct hipColumnInfo *ci = &schema->col[col];
    if (op == SET_IN_SET || op == SET_NOT_IN_SET) {
        const int k = col == 0 ? HIPKIND_U64 : (col == 4 || col == 8 || col == 11) ? HIPKIND_I32 : col == 6 ? HIPKIND_BOOL : HIPKIND_DICT;
        if (resolve_value_set(c, op == SET_NOT_IN_SET, col, k, sn, err, errlen) != 0) return -1;
        if (sn->mode == SM_MEMBER && !ci->present) sn->mode = SM_ABSENT;         /* no column for a pass to read */
        return 0;
    }
    const int not_form = op == SET_NOT_LIKE || op == SET_NOT_IN;
    const int is_like = op == SET_LIKE || op == SET_NOT_LIKE;
    /* typed by the column, as the literal of `=` is (make_leaf) */
    const int kind = col == 0 ? HIPKIND_U64 : (col == 4 || col == 8 || col == 11) ? HIPKIND_I32 : col == 6 ? HIPKIND_BOOL : HIPKIND_DICT;
    if (is_like && kind != HIPKIND_DICT) return set_fail(err, errlen, c->attribute, "LIKE needs a string column");
    char **items = NULL;
    int n_items = 0;
    if (!is_like && parse_in_list(c->attribute, c->value, &items, &n_items, err, errlen) != 0) return -1;
    struct runs S;
    memset(&S, 0, sizeof S);
    int rc = 0;
    uint64_t dmax = 0, unbias = 0;
    if (kind == HIPKIND_DICT) {
        if (!(ci->present && ci->kind == HIPKIND_DICT)) sn->mode = SM_ABSENT;      /* reported as absent if it can be reached */
        else {
            uint8_t *mark = calloc((size_t)ci->dict_count + 1, 1);
            if (!mark) rc = -1;
            else if (is_like) rc = like_marks(ci, c->value, mark);
            else for (int i = 0, present; i < n_items; i++) {
                const int l = hipDictionaryRank(ci->dict, ci->dict_count, items[i], &present);
                if (present) mark[l] = 1;
            }
            for (int k = 0; rc == 0 && k < ci->dict_count; k++) if (mark[k]) rc = runs_add(&S, (uint64_t)k);
            free(mark);
            dmax = ci->dict_count > 0 ? (uint64_t)ci->dict_count - 1 : 0;
        }
    } else {
        uint64_t *v = malloc(((size_t)n_items + 1) * sizeof *v);
        if (!v) rc = -1;
        else {
            for (int i = 0; i < n_items; i++) {
                if (kind == HIPKIND_U64) v[i] = strtoull(items[i], NULL, 10);
                else if (kind == HIPKIND_I32) v[i] = (uint64_t)((uint32_t)atoi(items[i]) ^ 0x80000000u);
                else v[i] = (strcasecmp(items[i], "true") == 0 || strcmp(items[i], "1") == 0);
            }
            qsort(v, (size_t)n_items, sizeof *v, cmp_u64);
            for (int i = 0; rc == 0 && i < n_items; i++) rc = runs_add(&S, v[i]);
            free(v);
        }
        dmax = kind == HIPKIND_U64 ? UINT64_MAX : kind == HIPKIND_I32 ? 0xFFFFFFFFull : 1;
        unbias = kind == HIPKIND_I32 ? 0x80000000ull : 0;
    }
    if (rc == 0 && sn->mode != SM_ABSENT) rc = set_from_runs(sn, &S, dmax, unbias, not_form, kind);
    if (rc == 0 && sn->mode == SM_MEMBER && !ci->present) {               /* no column for a pass to read */
        free(sn->bitmap); free(sn->list);
        sn->bitmap = NULL; sn->list = NULL;
        sn->mode = SM_ABSENT;
    }
    for (int i = 0; i < n_items; i++) free(items[i]);
    free(items); free(S.lo); free(S.hi);
    if (rc != 0 && err && errlen && !err[0]) snprintf(err, errlen, "out of memory");
    return rc;
}

/* One table entry per set node of the tree.  Fails (message in err) where the node cannot be compiled at all. */
static int resolve_sets(const struct hipSchema *schema, const struct whereClauseS *wc, struct set_table *T, char *err, size_t errlen) {
    for (; wc; wc = wc->next) {
        if (wc->sub) { if (resolve_sets(schema, wc->sub, T, err, errlen) != 0) return -1; continue; }
        const int op = set_op_code(wc->operator);
        const int col = wc->attribute ? hipColumnId(wc->attribute) : -1;
        if (op < 0 || col < 0 || wc->value == NULL) continue;             /* never true, like any unknown attribute */
        int known = 0;
        for (int i = 0; i < T->n; i++)
            if (T->node[i].attribute == wc->attribute && T->node[i].operator == wc->operator && T->node[i].value == wc->value) known = 1;
        if (known) continue;
        if (T->n == T->cap) {
            const int cap = T->cap ? 2 * T->cap : 8;
            struct set_node *grown = realloc(T->node, (size_t)cap * sizeof *grown);
            if (!grown) { if (err) snprintf(err, errlen, "out of memory"); return -1; }
            T->node = grown; T->cap = cap;
        }
        struct set_node *sn = &T->node[T->n];
        memset(sn, 0, sizeof *sn);
        sn->attribute = wc->attribute; sn->operator = wc->operator; sn->value = wc->value;
        sn->col = col; sn->pass = -1;
        T->n++;                                                            /* (set_table_free releases what a failed node holds) */
        if (resolve_one(schema, wc, op, col, sn, err, errlen) != 0) return -1;
    }
    return 0;
}

static int set_node_column(const struct set_node *sn) {
    return sn->mode == SM_MEMBER ? (sn->pass >= 0 ? PQPS_MAX_COLUMNS + sn->pass : -1) : sn->col;
}
static int set_node_leaves(const struct set_node *sn) { return sn->mode == SM_WINDOWS ? sn->n_runs : 1; }

struct builder {
    const struct hipSchema *schema;
    struct step st[MAX_RAW_STEPS];
    int n;
    char *err;
    size_t errlen;
    int failed;
};

static int count_leaves(const struct whereClauseS *wc) {
    int n = 0;
    for (; wc; wc = wc->next) n += wc->sub ? count_leaves(wc->sub) : node_leaves(wc);
    return n;
}

/* checkCondition S:251-289 + create_where_condition S:129-213 as a window. */
static void make_leaf(struct builder *b, struct step *s, const struct whereClauseS *c) {
    s->kind = ST_FALSE;
    s->col = -1;
    const int col = node_column(c);
    const struct set_node *sn = find_set(c);
    if (sn) {                                                    /* a set node that is one step: decided, or the flags of its member pass */
        if (sn->mode == SM_FALSE || col < 0) return;
        if (sn->mode == SM_TRUE) { s->kind = ST_TRUE; return; }
        s->kind = ST_LEAF; s->col = col; s->lo = 1; s->span = 0; s->neg = sn->negate;
        if (sn->mode == SM_ABSENT) {
            s->lo = 0; s->neg = 0;
            b->failed = 1;
            if (b->err) snprintf(b->err, b->errlen, "column '%s' is not materialised on the device", c->attribute);
        }
        return;
    }
    const int op = op_code(c->operator);
    if (col < 0 || op < 0 || c->value == NULL) return;          /* S:212, S:279: never true */
    const struct hipColumnInfo *ci = col_info(b->schema, col);
    s->col = col;
    if (col >= PQPS_MAX_COLUMNS) { s->kind = ST_LEAF; s->lo = 1; s->span = 0; s->neg = 0; return; }
    /* the literal is typed by the column, not by the token (S:256-276) */
    if (strcmp(c->attribute, "command_id") == 0) {
        window_unsigned(s, op, strtoull(c->value, NULL, 10), UINT64_MAX);
    } else if (strcmp(c->attribute, "risk_level") == 0 || strcmp(c->attribute, "exit_code") == 0 ||
               strcmp(c->attribute, "user_id") == 0) {
        window_i32(s, op, atoi(c->value));
    } else if (strcmp(c->attribute, "sudo_used") == 0) {
        const int lit = (strcasecmp(c->value, "true") == 0 || strcmp(c->value, "1") == 0);
        if (op == 0) { s->kind = ST_LEAF; s->lo = (uint64_t)lit; s->span = 0; s->neg = 0; }
        else if (op == 1) { s->kind = ST_LEAF; s->lo = (uint64_t)lit; s->span = 0; s->neg = 1; }
        else return;                                             /* S:207-210: no ordering comparators */
    } else {
        if (ci->present && ci->kind == HIPKIND_DICT) {
            window_dict(s, op, c->value, ci);
            /* a column with ONE value: every row carries code 0, the comparison is decided here and now (such a column
             * may have no device buffer at all: include/buildEngine-hip.h) */
            if (s->kind == ST_LEAF && ci->dict_count == 1) s->kind = ((s->lo == 0) != (s->neg != 0)) ? ST_TRUE : ST_FALSE;
        } else s->kind = ST_LEAF;                                /* reported as absent below */
    }
    if (s->kind == ST_LEAF && !ci->present) {
        b->failed = 1;
        if (b->err) snprintf(b->err, b->errlen, "column '%s' is not materialised on the device", c->attribute);
    }
}

/* Emits the steps of one chain starting at raw index `start`; T / F are the
 * targets of the whole chain.  evaluateWhereClause S:292-316:
 *   cur OR  rest  -> true: T,    false: rest
 *   cur AND rest  -> true: rest, false: F      (also any other / NULL logical_op, S:315)
 *   last          -> true: T,    false: F                                               */
static void emit_chain(struct builder *b, const struct whereClauseS *wc, int start, int T, int F) {
    for (; wc; wc = wc->next) {
        const int size = wc->sub ? count_leaves(wc->sub) : node_leaves(wc);
        const int next_start = start + size;
        int t = T, f = F;
        if (wc->next) {
            if (wc->logical_op && strcmp(wc->logical_op, "OR") == 0) f = next_start;
            else t = next_start;
        }
        const struct set_node *sn = wc->sub ? NULL : find_set(wc);
        if (wc->sub) {
            emit_chain(b, wc->sub, start, t, f);
        } else if (sn && sn->mode == SM_WINDOWS) {
            /* the runs as window leaves at the node's own targets: an OR ladder, or an AND ladder of negated windows */
            for (int i = 0; i < size; i++) {
                struct step *s = &b->st[start + i];
                const int more = i + 1 < size ? start + i + 1 : (sn->negate ? t : f);
                s->kind = ST_LEAF; s->col = sn->col; s->lo = sn->lo[i]; s->span = sn->span[i]; s->neg = sn->negate;
                s->t = sn->negate ? more : t;
                s->f = sn->negate ? f : more;
            }
            if (!b->schema->col[sn->col].present) {
                b->failed = 1;
                if (b->err) snprintf(b->err, b->errlen, "column '%s' is not materialised on the device", wc->attribute);
            }
        } else {
            struct step *s = &b->st[start];
            if (wc->attribute == NULL) { s->kind = ST_FALSE; s->col = -1; }   /* reference would crash; never true */
            else make_leaf(b, s, wc);
            s->t = t;
            s->f = f;
        }
        start = next_start;
    }
}

static int cmp_int(const void *a, const void *b) { return *(const int *)a - *(const int *)b; }

static int compile_pass(const struct hipSchema *schema, const struct whereClauseS *where,
                        pqps_predicate *pred, int column_ids[PQPS_MAX_COLUMNS],
                        char *err, size_t errlen) {
    memset(pred, 0, sizeof *pred);
    if (err && errlen) err[0] = '\0';
    for (int i = 0; i < PQPS_MAX_COLUMNS; i++) column_ids[i] = -1;
    if (where == NULL) { pred->truth = 1; return 0; }            /* S:864: no clause keeps every row */

    const int raw = count_leaves(where);
    if (raw > MAX_RAW_STEPS) {
        if (err) snprintf(err, errlen, "WHERE has %d leaves (limit %d)", raw, MAX_RAW_STEPS);
        return -1;
    }
    struct builder *b = calloc(1, sizeof *b);
    if (!b) { if (err) snprintf(err, errlen, "out of memory"); return -1; }
    b->schema = schema; b->n = raw; b->err = err; b->errlen = errlen;
    emit_chain(b, where, 0, T_ACCEPT, T_REJECT);

    /* fold constant leaves: alias[s] = where control really goes when it reaches s */
    int alias[MAX_RAW_STEPS];
    for (int s = raw - 1; s >= 0; s--) {
        struct step *st = &b->st[s];
        if (st->t >= 0) st->t = alias[st->t];
        if (st->f >= 0) st->f = alias[st->f];
        alias[s] = st->kind == ST_LEAF ? s : (st->kind == ST_TRUE ? st->t : st->f);
    }
    const int entry = alias[0];
    /* reachability (jumps only go forward) */
    char reach[MAX_RAW_STEPS];
    memset(reach, 0, sizeof reach);
    if (entry >= 0) reach[entry] = 1;
    for (int s = 0; s < raw; s++) {
        if (!reach[s]) continue;
        if (b->st[s].t >= 0) reach[b->st[s].t] = 1;
        if (b->st[s].f >= 0) reach[b->st[s].f] = 1;
    }
    int newidx[MAX_RAW_STEPS], n = 0;
    for (int s = 0; s < raw; s++) newidx[s] = reach[s] ? n++ : -1;

    /* only leaves that can actually be evaluated may name an absent column */
    int absent = 0;
    for (int s = 0; s < raw; s++)
        if (reach[s] && !col_info(schema, b->st[s].col)->present) absent = 1;
    if (b->failed && !absent) { b->failed = 0; if (err && errlen) err[0] = '\0'; }
    if (b->failed) { free(b); return -1; }

    if (entry < 0) {                                             /* constant predicate */
        pred->truth = (entry == T_ACCEPT) ? 1 : 0;
        free(b);
        return 0;
    }
    if (n > PQPS_MAX_LEAVES) {
        if (err) snprintf(err, errlen, "WHERE needs %d leaf comparisons (limit %d)", n, PQPS_MAX_LEAVES);
        free(b);
        return -1;
    }

    /* column slots: distinct columns of the reachable leaves, widest first (then
     * ascending HIPCOL id) -- the order the width-specialised kernels expect */
    int cols[PQPS_MAX_LEAVES], nc = 0;
    for (int s = 0; s < raw; s++) if (reach[s]) cols[nc++] = b->st[s].col;
    qsort(cols, (size_t)nc, sizeof cols[0], cmp_int);
    int n_cols = 0;
    for (int i = 0; i < nc; i++) {
        if (i != 0 && cols[i] == cols[i - 1]) continue;
        if (n_cols == PQPS_MAX_COLUMNS) {
            if (err) snprintf(err, errlen, "WHERE reads more than %d columns in one pass", PQPS_MAX_COLUMNS);
            free(b);
            return -1;
        }
        column_ids[n_cols++] = cols[i];
    }
    for (int i = 1; i < n_cols; i++) {                           /* stable insertion sort by width desc */
        const int c = column_ids[i];
        int j = i;
        while (j > 0 && col_info(schema, column_ids[j - 1])->width < col_info(schema, c)->width) { column_ids[j] = column_ids[j - 1]; j--; }
        column_ids[j] = c;
    }

    /* leaf slots sorted by column slot (stable in evaluation order) */
    int slot_of_step[PQPS_MAX_LEAVES];
    int k = 0;
    for (int c = 0; c < n_cols; c++) {
        for (int s = 0; s < raw; s++) {
            if (!reach[s] || b->st[s].col != column_ids[c]) continue;
            const struct step *st = &b->st[s];
            pred->leaf[k].column = (uint32_t)c;
            pred->leaf[k].negate = (uint32_t)st->neg;
            pred->leaf[k].lo = st->lo;
            pred->leaf[k].span = st->span;
            slot_of_step[newidx[s]] = k++;
        }
    }
    for (int s = 0; s < raw; s++) {
        if (!reach[s]) continue;
        const int i = newidx[s];
        const struct step *st = &b->st[s];
        pred->order[i] = (uint8_t)slot_of_step[i];
        pred->on_true[i] = st->t == T_ACCEPT ? PQPS_ACCEPT : st->t == T_REJECT ? PQPS_REJECT : (uint8_t)newidx[st->t];
        pred->on_false[i] = st->f == T_ACCEPT ? PQPS_ACCEPT : st->f == T_REJECT ? PQPS_REJECT : (uint8_t)newidx[st->f];
    }
    pred->n_leaves = (uint32_t)n;
    pred->n_columns = (uint32_t)n_cols;

    /* truth table over leaf SLOTS by walking the jump table for every assignment */
    if (n <= PQPS_TT_LEAVES) {
        uint64_t tt = 0;
        for (uint32_t m = 0; m < (1u << n); m++) {
            int s = 0;
            while (s < n) {
                const int r = (m >> pred->order[s]) & 1u;
                const uint8_t nx = r ? pred->on_true[s] : pred->on_false[s];
                if (nx >= PQPS_ACCEPT) { s = nx; break; }
                s = nx;
            }
            if (s == PQPS_ACCEPT) tt |= 1ull << m;
        }
        pred->truth = tt;
    }
    free(b);
    return 0;
}

int hipCompileWhere(const struct hipSchema *schema, const struct whereClauseS *where,
                    pqps_predicate *pred, int column_ids[PQPS_MAX_COLUMNS],
                    char *err, size_t errlen) {
    struct set_table T;
    memset(&T, 0, sizeof T);
    memset(pred, 0, sizeof *pred);
    if (err && errlen) err[0] = '\0';
    for (int i = 0; i < PQPS_MAX_COLUMNS; i++) column_ids[i] = -1;
    int rc = resolve_sets(schema, where, &T, err, errlen);
    for (int i = 0; rc == 0 && i < T.n; i++)
        if (T.node[i].mode == SM_MEMBER) {
            if (err) snprintf(err, errlen, "%s: the set needs a member pass (hipCompileWherePlan)", T.node[i].attribute);
            rc = -1;
        }
    if (rc == 0) {
        sets = &T;
        rc = compile_pass(schema, where, pred, column_ids, err, errlen);
        sets = NULL;
    }
    set_table_free(&T);
    return rc;
}

/* ---- multi-pass plans ----------------------------------------------------------------------------- */

struct planner {
    const struct hipSchema *schema;
    struct hipPlan *plan;
    int capacity;
    void **arena; int n_arena, cap_arena;
    char *err; size_t errlen;
};

static void *plan_alloc(struct planner *P, size_t bytes) {
    if (P->n_arena == P->cap_arena) {
        const int cap = P->cap_arena ? 2 * P->cap_arena : 16;
        void **grown = realloc(P->arena, (size_t)cap * sizeof *grown);
        if (!grown) return NULL;
        P->arena = grown; P->cap_arena = cap;
    }
    void *p = calloc(1, bytes ? bytes : 1);
    if (p) P->arena[P->n_arena++] = p;
    return p;
}

/* distinct columns a chain would bind: table columns once each, every flag column */
static void chain_columns(const struct whereClauseS *wc, uint32_t *table_mask, int *flag_columns) {
    for (; wc; wc = wc->next) {
        if (wc->sub) { chain_columns(wc->sub, table_mask, flag_columns); continue; }
        const int col = node_column(wc);
        if (col >= PQPS_MAX_COLUMNS) *flag_columns += 1;
        else if (col >= 0) *table_mask |= 1u << col;
    }
}

static int element_leaves(const struct whereClauseS *e) { return e->sub ? count_leaves(e->sub) : node_leaves(e); }

/* does [first, last] (elements of one array) fit one pass? */
static int span_fits(const struct whereClauseS *first, const struct whereClauseS *last) {
    int leaves = 0, flags = 0;
    uint32_t mask = 0;
    for (const struct whereClauseS *e = first; e <= last; e++) {
        leaves += element_leaves(e);
        if (e->sub) chain_columns(e->sub, &mask, &flags);
        else {
            const int col = node_column(e);
            if (col >= PQPS_MAX_COLUMNS) flags++; else if (col >= 0) mask |= 1u << col;
        }
    }
    return leaves <= PQPS_MAX_LEAVES && __builtin_popcount(mask) + flags <= PQPS_MAX_COLUMNS;
}

/* Compiles `chain` as the next pass; returns its number, -1 on failure. */
static struct hipPass *next_pass(struct planner *P) {
    struct hipPlan *plan = P->plan;
    if (plan->n_passes == P->capacity) {
        const int cap = P->capacity ? 2 * P->capacity : 4;
        struct hipPass *grown = realloc(plan->pass, (size_t)cap * sizeof *grown);
        if (!grown) { if (P->err) snprintf(P->err, P->errlen, "out of memory"); return NULL; }
        plan->pass = grown; P->capacity = cap;
    }
    struct hipPass *pass = &plan->pass[plan->n_passes];
    memset(pass, 0, sizeof *pass);
    return pass;
}

/* The member pass of a set node: takes the node's bitmap or list; the node reads its flags from now on. */
static int emit_member(struct planner *P, struct set_node *sn) {
    struct hipPass *pass = next_pass(P);
    if (!pass) return -1;
    for (int i = 0; i < PQPS_MAX_COLUMNS; i++) pass->column_ids[i] = -1;
    pass->member = 1;
    pass->member_column = sn->col;
    pass->member_form = sn->form;
    pass->member_base = sn->base;
    pass->member_bits = sn->n_bits;
    pass->member_bitmap = sn->bitmap; sn->bitmap = NULL;
    pass->member_list = sn->list; sn->list = NULL;
    pass->member_count = sn->n_list;
    pass->member_set = sn->set_id;
    sn->pass = P->plan->n_passes;
    return P->plan->n_passes++;
}

static int emit_pass(struct planner *P, const struct whereClauseS *chain) {
    struct hipPlan *plan = P->plan;
    struct hipPass *pass = next_pass(P);
    if (!pass) return -1;
    flag_passes = plan->n_passes;                                  /* this pass may read the flags of the passes before it */
    if (compile_pass(P->schema, chain, &pass->pred, pass->column_ids, P->err, P->errlen) != 0) return -1;
    flag_passes = plan->n_passes + 1;                              /* the planner may now name this pass's flags */
    return plan->n_passes++;
}

static int make_flag_leaf(struct planner *P, struct whereClauseS *e, int pass) {
    char *name = plan_alloc(P, 16);
    if (!name) { if (P->err) snprintf(P->err, P->errlen, "out of memory"); return -1; }
    snprintf(name, 16, "%c%d", FLAG_ATTRIBUTE, pass);
    e->attribute = name;
    e->operator = "=";
    e->value = "1";
    e->value_type = FLAG_MARK;
    e->sub = NULL;
    return 0;
}

/* A chain equivalent to `chain` that fits one pass; what does not fit is evaluated by earlier passes and
 * read back as flag leaves.  evaluateWhereClause (S:292-316) is right-recursive: `e AND rest` / `e OR rest`
 * only ever continue at the START of rest, so any suffix of the element list can be evaluated first and
 * replaced by one leaf; a parenthesised element is a value of its own and can be replaced likewise. */
static struct whereClauseS *fit_chain(struct planner *P, const struct whereClauseS *chain) {
    int n = 0;
    for (const struct whereClauseS *wc = chain; wc; wc = wc->next) n++;
    struct whereClauseS *el = plan_alloc(P, (size_t)n * sizeof *el);
    if (!el) { if (P->err) snprintf(P->err, P->errlen, "out of memory"); return NULL; }
    int i = 0;
    for (const struct whereClauseS *wc = chain; wc; wc = wc->next, i++) {
        el[i] = *wc;
        el[i].next = i + 1 < n ? &el[i + 1] : NULL;
    }
    for (i = 0; i < n; i++) {
        if (!el[i].sub || (span_fits(&el[i], &el[i]) && count_leaves(el[i].sub) < PQPS_MAX_LEAVES)) continue;
        struct whereClauseS *inner = fit_chain(P, el[i].sub);        /* too large for one pass even alone */
        const int pass = inner ? emit_pass(P, inner) : -1;
        if (pass < 0 || make_flag_leaf(P, &el[i], pass) != 0) return NULL;
    }
    while (!span_fits(&el[0], &el[n - 1])) {
        int first = n - 1;                                            /* longest suffix that fits a pass */
        while (first > 0 && span_fits(&el[first - 1], &el[n - 1])) first--;
        if (first == n - 1 && element_leaves(&el[n - 1]) == 1) {
            /* a lone leaf: replacing it gains nothing.  The element before it (a parenthesised one, or the
             * two would fit together) becomes a leaf first. */
            if (n < 2 || !el[n - 2].sub) { if (P->err) snprintf(P->err, P->errlen, "WHERE cannot be split into passes"); return NULL; }
            const int pass = emit_pass(P, el[n - 2].sub);
            if (pass < 0 || make_flag_leaf(P, &el[n - 2], pass) != 0) return NULL;
            continue;
        }
        const int pass = emit_pass(P, &el[first]);
        if (pass < 0 || make_flag_leaf(P, &el[first], pass) != 0) return NULL;
        el[first].next = NULL;
        el[first].logical_op = NULL;
        n = first + 1;
    }
    return el;
}

int hipCompileWherePlan(const struct hipSchema *schema, const struct whereClauseS *where,
                        struct hipPlan *plan, char *err, size_t errlen) {
    return hipCompileWherePlanSets(schema, where, NULL, 0, plan, err, errlen);
}

int hipCompileWherePlanSets(const struct hipSchema *schema, const struct whereClauseS *where, const struct hipSetInfo *value_set_table,
                            int n_sets, struct hipPlan *plan, char *err, size_t errlen) {
    memset(plan, 0, sizeof *plan);
    struct planner P;
    memset(&P, 0, sizeof P);
    P.schema = schema; P.plan = plan; P.err = err; P.errlen = errlen;
    if (err && errlen) err[0] = '\0';
    /* set nodes first: what each selects, and a member pass for every set too fragmented for window leaves */
    struct set_table T;
    memset(&T, 0, sizeof T);
    value_sets = value_set_table;
    n_value_sets = value_set_table && n_sets > 0 ? n_sets : 0;
    int last = resolve_sets(schema, where, &T, err, errlen);
    value_sets = NULL;
    n_value_sets = 0;
    sets = &T;
    flag_passes = 0;
    for (int i = 0; last == 0 && i < T.n; i++)
        if (T.node[i].mode == SM_MEMBER && emit_member(&P, &T.node[i]) < 0) last = -1;
    const int n_member = plan->n_passes;
    if (last == 0) {
        /* one further pass whenever the clause allows it (constant leaves are folded away first) */
        if (count_leaves(where) > MAX_RAW_STEPS || (last = emit_pass(&P, where)) < 0) {
            if (err && errlen) err[0] = '\0';
            plan->n_passes = n_member;
            struct whereClauseS *fitted = fit_chain(&P, where);
            last = fitted ? emit_pass(&P, fitted) : -1;
        }
    }
    flag_passes = 0;
    sets = NULL;
    set_table_free(&T);
    for (int i = 0; i < P.n_arena; i++) free(P.arena[i]);
    free(P.arena);
    if (last < 0) { hipPlanFree(plan); return -1; }
    return 0;
}

void hipPlanFree(struct hipPlan *plan) {
    if (!plan) return;
    for (int k = 0; k < plan->n_passes; k++) { free(plan->pass[k].member_bitmap); free(plan->pass[k].member_list); }
    free(plan->pass);
    plan->pass = NULL;
    plan->n_passes = 0;
}

/* ---- the HAVING of a value set ------------------------------------------------------------------------------------- */

static int having_fail(const char *what, const char *text) {
    fprintf(stderr, "HIP engine: HAVING: %s%s%s%s\n", what, text ? " '" : "", text ? text : "", text ? "'" : "");
    return -1;
}

int hipCompileHaving(int aggregate, int value_kind, const char *op, const char *constant, struct hipHaving *out) {
    static const char *const k_ops[6] = { "=", "!=", "<", ">", "<=", ">=" };    /* PQPS_HAVING_EQ .. _GE */
    if (!op || !constant || !out) return having_fail("NULL argument", NULL);
    if (aggregate < HIPTOP_BY_COUNT || aggregate > HIPTOP_BY_MAX) return having_fail("the aggregate is none of COUNT, SUM, MIN, MAX", NULL);
    const int counted = aggregate == HIPTOP_BY_COUNT;
    if (!counted && value_kind != HIPKIND_I32 && value_kind != HIPKIND_U64) return having_fail("SUM / MIN / MAX need a numeric value column", NULL);
    struct hipHaving h;
    memset(&h, 0, sizeof h);
    h.field = aggregate - HIPTOP_BY_COUNT;
    h.op = -1;
    for (int i = 0; i < 6; i++) if (strcmp(op, k_ops[i]) == 0) h.op = i;
    if (h.op < 0) return having_fail("unknown operator", op);
    const char *p = constant;
    while (is_blank(*p)) p++;
    const int is_signed = !counted && value_kind == HIPKIND_I32;
    const char *digits = p + (*p == '+' || *p == '-');
    if (*digits < '0' || *digits > '9') return having_fail("the constant is no decimal number", constant);
    if (*p == '-' && !is_signed) return having_fail("a negative constant for an unsigned aggregate", constant);
    char *end = NULL;
    errno = 0;
    if (is_signed) h.constant = (uint64_t)strtoll(p, &end, 10);
    else h.constant = strtoull(p, &end, 10);
    if (errno == ERANGE) return having_fail("the constant is out of range", constant);
    if (!end || *end) return having_fail("trailing garbage behind the constant", constant);
    if (is_signed && aggregate >= HIPTOP_BY_MIN) h.constant ^= 0x8000000000000000ull;      /* the image of pqps_filter_aggregate */
    h.value_signed = is_signed && aggregate == HIPTOP_BY_SUM;
    *out = h;
    return 0;
}

/* ---- the SET list of an UPDATE ------------------------------------------------------------------------------------ */

/* bytes of the `record` field of a string column (with its NUL), 0 for the others */
static size_t field_bytes(int col) {
    static const size_t k_bytes[PQPS_MAX_COLUMNS] = {
        0, sizeof(((record *)0)->raw_command), sizeof(((record *)0)->base_command), sizeof(((record *)0)->shell_type), 0,
        sizeof(((record *)0)->timestamp), 0, sizeof(((record *)0)->working_directory), 0, sizeof(((record *)0)->user_name),
        sizeof(((record *)0)->host_name), 0
    };
    return k_bytes[col];
}

static int assign_fail(const char *column, const char *what) {
    fprintf(stderr, "HIP engine: UPDATE SET %s: %s\n", column ? column : "(null)", what);
    return -1;
}

int hipCompileAssignments(const struct hipSchema *schema, const char *const *columns, const char *const *values, int n,
                          struct hipAssignment *out) {
    struct hipAssignment a[PQPS_MAX_COLUMNS];
    if (!schema || !columns || !values || !out) return assign_fail(NULL, "NULL argument");
    if (n < 1 || n > PQPS_MAX_COLUMNS) return assign_fail(NULL, "1 to 12 assignments");
    for (int i = 0; i < n; i++) {
        const int col = hipColumnId(columns[i]);
        if (col < 0) return assign_fail(columns[i], "unknown column");
        if (!values[i]) return assign_fail(columns[i], "no value");
        for (int k = 0; k < i; k++)
            if (a[k].column == col) return assign_fail(columns[i], "assigned twice");
        const struct hipColumnInfo *ci = &schema->col[col];
        if (!ci->present) return assign_fail(columns[i], "the column is not materialised on the device");
        a[i] = (struct hipAssignment){ col, ci->kind, 0, 1, 0, NULL };
        switch (ci->kind) {
        case HIPKIND_U64:
            a[i].value = strtoull(values[i], NULL, 10);
            if (a[i].value == 0) return assign_fail(columns[i], "command_id 0 is no row's id");
            break;
        case HIPKIND_I32:
            a[i].value = (uint64_t)(uint32_t)atoi(values[i]);
            break;
        case HIPKIND_BOOL:
            a[i].value = (strcasecmp(values[i], "true") == 0 || strcmp(values[i], "1") == 0) ? 1u : 0u;
            break;
        default: {
            if (!values[i][0]) return assign_fail(columns[i], "an empty string");
            if (strlen(values[i]) + 1 > field_bytes(col)) return assign_fail(columns[i], "the string does not fit the record's field");
            a[i].rank = (uint32_t)hipDictionaryRank(ci->dict, ci->dict_count, values[i], &a[i].present);
            a[i].value = a[i].rank;
            a[i].text = values[i];
            break;
        }
        }
    }
    memcpy(out, a, (size_t)n * sizeof *a);
    return 0;
}

/* ---- the dictionary merge of a batch INSERT ----------------------------------------------------------------------- */

static int merge_fail(int column, const char *what) {
    fprintf(stderr, "HIP engine: dictionary merge, column %d: %s\n", column, what);
    return -1;
}

/* 0 when the list is strictly ascending, free of empty strings and of strings longer than the field */
static int merge_check(const char *const *values, int count, size_t room, int column, const char *which) {
    for (int i = 0; i < count; i++) {
        if (!values[i]) return merge_fail(column, "a NULL string");
        if (!values[i][0]) return merge_fail(column, "an empty string");
        if (strlen(values[i]) + 1 > room) return merge_fail(column, "a string does not fit the record's field");
        if (i > 0 && strcmp(values[i - 1], values[i]) >= 0) return merge_fail(column, which);
    }
    return 0;
}

int hipMergeDictionaries(const char *const *old_values, int old_count, const char *const *new_values, int new_count, int column,
                         const char **merged, int *merged_count, uint32_t *lut_old, uint32_t *lut_new, int *identity) {
    if (!merged || !merged_count || !lut_old || !lut_new || !identity || (!old_values && old_count > 0) || (!new_values && new_count > 0))
        return merge_fail(column, "NULL argument");
    if (old_count < 0 || new_count < 0) return merge_fail(column, "a negative count");
    if (column < 0 || column >= PQPS_MAX_COLUMNS || field_bytes(column) == 0) return merge_fail(column, "not a string column");
    const size_t room = field_bytes(column);
    if (merge_check(old_values, old_count, room, column, "the old list is not strictly ascending") != 0 ||
        merge_check(new_values, new_count, room, column, "the new list is not strictly ascending") != 0)
        return -1;
    /* nothing is refused from here on: the outputs may be written */
    int i = 0, k = 0, m = 0, same = 1;
    while (i < old_count || k < new_count) {
        const int c = i >= old_count ? 1 : k >= new_count ? -1 : strcmp(old_values[i], new_values[k]);
        if (c <= 0) {
            merged[m] = old_values[i];
            if (m != i) same = 0;
            lut_old[i++] = (uint32_t)m;
            if (c == 0) lut_new[k++] = (uint32_t)m;
        } else {
            merged[m] = new_values[k];
            lut_new[k++] = (uint32_t)m;
        }
        m++;
    }
    *merged_count = m;
    *identity = same;
    return 0;
}

/* ---- the buckets of GROUP BY PREFIX(k) / WIDTH(w) ------------------------------------------------------------------ */

static const int k_bucket_kind[PQPS_MAX_COLUMNS] = {
    HIPKIND_U64, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_I32, HIPKIND_DICT,
    HIPKIND_BOOL, HIPKIND_DICT, HIPKIND_I32, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_I32
};

static int bucket_fail(const char *column, const char *what) {
    fprintf(stderr, "HIP engine: buckets of %s: %s\n", column ? column : "(null)", what);
    return -1;
}

/* floor(v / w) for w >= 1 */
static long long floor_div(long long v, long long w) {
    return v / w - (v % w < 0);
}

/* 1 when a and b differ within their first k bytes (either may end sooner) */
static int prefix_differs(const char *a, const char *b, long long k) {
    for (long long i = 0; i < k; i++) {
        if (a[i] != b[i]) return 1;
        if (!a[i]) return 0;
    }
    return 0;
}

int hipBucketBounds(const char *column, const char *const *dict, int dict_count, int lo, int hi, int mode, long long arg,
                    uint32_t **bounds, long long **keys, uint32_t *n_buckets) {
    if (!bounds || !keys || !n_buckets) return bucket_fail(column, "NULL argument");
    const int c = hipColumnId(column);
    if (c < 0) return bucket_fail(column, "unknown column");
    if (c == 0) return bucket_fail(column, "command_id is unique -- it has no buckets");
    if (mode != HIPBUCKET_PREFIX && mode != HIPBUCKET_WIDTH) return bucket_fail(column, "the mode is neither PREFIX nor WIDTH");
    const int kind = k_bucket_kind[c];
    if (arg < 1) return bucket_fail(column, mode == HIPBUCKET_PREFIX ? "a prefix of less than 1 byte" : "a width of less than 1");
    if (mode == HIPBUCKET_PREFIX && kind != HIPKIND_DICT) return bucket_fail(column, "PREFIX needs a string column");
    if (mode == HIPBUCKET_WIDTH && kind != HIPKIND_I32) return bucket_fail(column, "WIDTH needs an i32 column");
    uint64_t n = 0, domain;
    if (mode == HIPBUCKET_PREFIX) {
        if (!dict || dict_count < 1) return bucket_fail(column, "an empty dictionary");
        domain = (uint64_t)dict_count;
        for (int i = 0; i < dict_count; i++) {
            if (!dict[i]) return bucket_fail(column, "a NULL string");
            n += i == 0 || prefix_differs(dict[i - 1], dict[i], arg);
        }
    } else {
        if (lo > hi) return bucket_fail(column, "an empty range");
        domain = (uint64_t)((long long)hi - (long long)lo) + 1u;
        if (domain > UINT32_MAX) return bucket_fail(column, "the range spans 2^32 values: no u32 holds the sentinel");
        n = (uint64_t)(floor_div(hi, arg) - floor_div(lo, arg)) + 1u;
    }
    if (n > HIPBUCKET_MAX) {
        fprintf(stderr, "HIP engine: buckets of %s: %llu buckets, more than %u\n", column, (unsigned long long)n, HIPBUCKET_MAX);
        return -1;
    }
    uint32_t *b = malloc((size_t)(n + 1) * sizeof *b);
    long long *k = malloc((size_t)n * sizeof *k);
    if (!b || !k) { free(b); free(k); return bucket_fail(column, "out of memory"); }
    if (mode == HIPBUCKET_PREFIX) {
        uint64_t j = 0;
        for (int i = 0; i < dict_count; i++)
            if (i == 0 || prefix_differs(dict[i - 1], dict[i], arg)) { b[j] = (uint32_t)i; k[j++] = i; }
    } else {
        const long long q0 = floor_div(lo, arg);
        for (uint64_t j = 0; j < n; j++) {
            const long long lower = (q0 + (long long)j) * arg;
            k[j] = lower;
            b[j] = (uint32_t)((lower > lo ? lower : (long long)lo) - (long long)lo);
        }
    }
    b[n] = (uint32_t)domain;
    *bounds = b;
    *keys = k;
    *n_buckets = (uint32_t)n;
    return 0;
}

/* ---- the word of pqps_filter_group_first, undone --------------------------------------------------------------------- */

int hipFirstKeyDecode(int kind, int descending, unsigned long long word, long long *key, unsigned int *row) {
    if (kind != HIPKIND_I32 && kind != HIPKIND_BOOL && kind != HIPKIND_DICT) return -1;
    if (word == ~0ull) return 0;
    uint32_t img = (uint32_t)(word >> 32);
    if (descending) img = ~img;
    if (key) *key = kind == HIPKIND_I32 ? (long long)(int32_t)(img ^ 0x80000000u) : (long long)img;
    if (row) *row = (unsigned int)(word & 0xFFFFFFFFull);
    return 1;
}

/* ---- the shard merge of the first N rows of every group ----------------------------------------------------------------- */

/* Shard x's entry i against shard y's entry j: (bin, [best,] word). */
static int head_entry_cmp(const struct hipHeadList *x, uint64_t i, const struct hipHeadList *y, uint64_t j, bool wide) {
    if (x->bins[i] != y->bins[j]) return x->bins[i] < y->bins[j] ? -1 : 1;
    if (wide && x->best[i] != y->best[j]) return x->best[i] < y->best[j] ? -1 : 1;
    return x->words[i] < y->words[j] ? -1 : x->words[i] > y->words[j];
}

long long hipHeadMerge(const struct hipHeadList *shards, int n_shards, long long limit, uint32_t *out_bins, uint64_t *out_words,
                       uint64_t *out_best) {
    if (n_shards < 0 || (n_shards && !shards) || limit < 1) { fprintf(stderr, "hipHeadMerge: no shards, or limit %lld < 1\n", limit); return -1; }
    bool wide = false;
    uint64_t total = 0;
    for (int s = 0; s < n_shards; s++) {
        if (shards[s].n == 0) continue;
        if (!shards[s].bins || !shards[s].words) { fprintf(stderr, "hipHeadMerge: shard %d: a NULL list\n", s); return -1; }
        if (total && wide != (shards[s].best != NULL)) { fprintf(stderr, "hipHeadMerge: shard %d: narrow and wide lists mixed\n", s); return -1; }
        wide = shards[s].best != NULL;
        total += shards[s].n;
    }
    if (total && (!out_bins || !out_words || (wide && !out_best))) { fprintf(stderr, "hipHeadMerge: a NULL output\n"); return -1; }
    uint64_t *at = calloc((size_t)(n_shards ? n_shards : 1), sizeof *at);
    if (!at) { fprintf(stderr, "hipHeadMerge: out of memory\n"); return -1; }
    uint64_t n = 0, in_bin = 0;
    for (uint64_t step = 0; step < total; step++) {
        int b = -1;
        for (int s = 0; s < n_shards; s++)
            if (at[s] < shards[s].n && (b < 0 || head_entry_cmp(&shards[s], at[s], &shards[b], at[b], wide) < 0)) b = s;
        const uint64_t i = at[b]++;
        const uint32_t bin = shards[b].bins[i];
        if (n == 0 || out_bins[n - 1] != bin) in_bin = 0;
        if (in_bin >= (uint64_t)limit) continue;                        /* the bin has its rows: a later shard's surplus */
        out_bins[n] = bin;
        out_words[n] = shards[b].words[i];
        if (wide) out_best[n] = shards[b].best[i];
        n++;
        in_bin++;
    }
    free(at);
    return (long long)n;
}

/* ---- the order of the top N groups ------------------------------------------------------------------------------------- */

/* One group as the order sees it: `rank` ascends in the wanted order (complemented for a descending one), ties by bin. */
struct top_item { uint64_t rank, bin, index; };

static int top_before(const struct top_item *x, const struct top_item *y) {
    return x->rank != y->rank ? x->rank < y->rank : x->bin < y->bin;
}

static int top_item_cmp(const void *x, const void *y) {
    return top_before(x, y) ? -1 : top_before(y, x) ? 1 : 0;
}

/* h[0 .. n) is a heap whose root is the LAST of its entries in the order; the entry at i sinks to its place */
static void top_sift_down(struct top_item *h, uint64_t n, uint64_t i) {
    for (;;) {
        uint64_t last = i;
        const uint64_t l = 2 * i + 1, r = l + 1;
        if (l < n && top_before(&h[last], &h[l])) last = l;
        if (r < n && top_before(&h[last], &h[r])) last = r;
        if (last == i) return;
        const struct top_item t = h[i]; h[i] = h[last]; h[last] = t;
        i = last;
    }
}

long long hipGroupTopOrder(const uint64_t *bins, const uint64_t *counts, const uint64_t *sums, const uint64_t *min_images,
                           const uint64_t *max_images, uint64_t n_groups, int value_kind, int order_by, int descending,
                           long long limit, uint64_t *order) {
    const uint64_t *by = order_by == HIPTOP_BY_KEY ? bins : order_by == HIPTOP_BY_COUNT ? counts : order_by == HIPTOP_BY_SUM ? sums :
                         order_by == HIPTOP_BY_MIN ? min_images : max_images;
    uint64_t flip = 0;
    if (order_by < HIPTOP_BY_KEY || order_by > HIPTOP_BY_MAX) { fprintf(stderr, "HIP engine: top groups: order %d is none of HIPTOP_BY_*\n", order_by); return -1; }
    if (order_by == HIPTOP_BY_SUM) {
        if (value_kind != HIPKIND_I32 && value_kind != HIPKIND_U64) { fprintf(stderr, "HIP engine: top groups: sums of a column that is no number\n"); return -1; }
        if (value_kind == HIPKIND_I32) flip = 0x8000000000000000ull;     /* signed order as unsigned */
    }
    if (n_groups && (!bins || !by || !order)) { fprintf(stderr, "HIP engine: top groups: an array the order reads is NULL\n"); return -1; }
    const uint64_t k = limit > 0 && (uint64_t)limit < n_groups ? (uint64_t)limit : n_groups;
    if (k == 0) return 0;
    if (descending) flip = ~flip;
    struct top_item *h = malloc((size_t)k * sizeof *h);
    if (!h) { fprintf(stderr, "HIP engine: top groups: out of memory\n"); return -1; }
    for (uint64_t i = 0; i < n_groups; i++) {
        const struct top_item it = { by[i] ^ flip, bins[i], i };
        if (i < k) {
            h[i] = it;
            if (i + 1 == k && k < n_groups) for (uint64_t j = k / 2; j-- > 0;) top_sift_down(h, k, j);   /* the heap is made */
        } else if (top_before(&it, &h[0])) {                             /* replaces the last of the k kept */
            h[0] = it;
            top_sift_down(h, k, 0);
        }
    }
    qsort(h, (size_t)k, sizeof *h, top_item_cmp);
    for (uint64_t i = 0; i < k; i++) order[i] = h[i].index;
    free(h);
    return (long long)k;
}

/* ---- the packed key of ORDER BY several columns ---------------------------------------------------------------------- */

/* ceil(log2 d): the bits that hold 0 .. d - 1 */
static uint32_t domain_bits(uint64_t d) {
    uint32_t b = 0;
    while (b < 64 && (1ull << b) < d) b++;
    return b;
}

int hipOrderKeyPlan(const char *const *columns, const int *descending, int n_keys, const int *dict_counts,
                    const int *lo, const int *hi, struct hipOrderKeyPlan *plan) {
    if (!columns || !descending || !dict_counts || !lo || !hi || !plan) { fprintf(stderr, "HIP engine: ORDER BY: NULL argument\n"); return -1; }
    if (n_keys < 1 || n_keys > HIP_ORDER_MAX_KEYS) {
        fprintf(stderr, "HIP engine: ORDER BY: %d keys, not 1 .. %d\n", n_keys, HIP_ORDER_MAX_KEYS);
        return -1;
    }
    struct hipOrderKeyPlan p;
    memset(&p, 0, sizeof p);
    int seen[PQPS_MAX_COLUMNS] = { 0 };
    int has_u64 = 0;
    for (int i = 0; i < n_keys; i++) {
        if (!columns[i]) { fprintf(stderr, "HIP engine: ORDER BY: key %d without a column\n", i); return -1; }
        const int c = hipColumnId(columns[i]);
        if (c < 0) { fprintf(stderr, "HIP engine: ORDER BY: unknown column '%s'\n", columns[i]); return -1; }
        if (seen[c]) continue;                                           /* named before: no information */
        seen[c] = 1;
        const int kind = k_bucket_kind[c];
        if (kind == HIPKIND_DICT && dict_counts[c] <= 1) continue;       /* single-valued: no information */
        struct hipOrderField *f = &p.field[p.n_fields++];
        f->column = c;
        f->kind = kind;
        f->descending = descending[i] != 0;
        if (kind == HIPKIND_U64) { f->bits = 64; has_u64 = 1; }
        else if (kind == HIPKIND_DICT) f->bits = domain_bits((uint64_t)dict_counts[c]);
        else if (kind == HIPKIND_BOOL) f->bits = 1;
        else {
            f->base = (uint32_t)lo[c];
            f->bits = lo[c] > hi[c] ? 0 : domain_bits((uint64_t)((long long)hi[c] - (long long)lo[c]) + 1u);
        }
        p.total_bits += f->bits;
    }
    if (p.n_fields == 0) p.form = HIPORDER_ROWS;
    else if (p.n_fields == 1) p.form = HIPORDER_ONE;
    else if (has_u64 || p.total_bits > 64) p.form = HIPORDER_CHAIN;
    else p.form = p.total_bits <= 32 ? HIPORDER_PACK32 : HIPORDER_PACK64;
    if (p.form == HIPORDER_PACK32 || p.form == HIPORDER_PACK64) {
        uint32_t shift = 0;
        for (int j = p.n_fields - 1; j >= 0; j--) { p.field[j].shift = shift; shift += p.field[j].bits; }
    }
    *plan = p;
    return 0;
}

/* ---- the batches of several counts in one scan ------------------------------------------------------------------------ */

/* the batch being filled: columns and leaves in order of arrival, the programs' leaf slots index leaf[] */
struct count_open {
    int n_queries, n_leaves, n_cols;
    int col[PQPS_MAX_COLUMNS];                                   /* HIPCOL_* ids */
    struct count_leaf { int col; uint64_t lo, span; } leaf[PQPS_MAX_LEAVES];
    pqps_count_query query[PQPS_COUNT_MANY_MAX];
};

static int count_fail(int query, const char *what) {
    if (query >= 0) fprintf(stderr, "HIP engine: count many: query %d: %s\n", query, what);
    else fprintf(stderr, "HIP engine: count many: %s\n", what);
    return -1;
}

static int count_leaf_cmp(const struct count_leaf *a, const struct count_leaf *b) {
    if (a->col != b->col) return a->col < b->col ? -1 : 1;
    if (a->lo != b->lo) return a->lo < b->lo ? -1 : 1;
    if (a->span != b->span) return a->span < b->span ? -1 : 1;
    return 0;
}

static int count_find_leaf(const struct count_leaf *leaf, int n, const struct count_leaf *key) {
    for (int i = 0; i < n; i++) if (count_leaf_cmp(&leaf[i], key) == 0) return i;
    return -1;
}

/* The leaf a comparison becomes in a batch, and whether the comparison is its complement.  The window test is taken in the
 * arithmetic the kernels use -- 64 bits for command_id, 32 for every other column (pqps_leaf) -- where the complement of a
 * window is again a window: of the two, the one with the smaller span (then the smaller lo) names the leaf. */
static struct count_leaf count_canonical(int col, const pqps_leaf *l, int *negated) {
    const uint64_t mask = col >= 0 && col < PQPS_MAX_COLUMNS && k_bucket_kind[col] == HIPKIND_U64 ? ~0ull : 0xFFFFFFFFull;
    struct count_leaf c = { col, l->lo & mask, l->span & mask };
    *negated = l->negate != 0;
    if (c.span != mask) {                                        /* (the full window has no complement) */
        const uint64_t lo = (c.lo + c.span + 1) & mask, span = (mask - c.span - 1) & mask;
        if (span < c.span || (span == c.span && lo < c.lo)) { c.lo = lo; c.span = span; *negated = !*negated; }
    }
    return c;
}

static int count_find_col(const int *col, int n, int id) {
    for (int i = 0; i < n; i++) if (col[i] == id) return i;
    return -1;
}

/* the open batch, its columns ascending and its leaves sorted by (column slot, lo, span), into *out */
static void count_close(const struct count_open *o, struct hipCountBatch *out) {
    memset(out, 0, sizeof *out);
    int col[PQPS_MAX_COLUMNS];
    memcpy(col, o->col, sizeof col);
    qsort(col, (size_t)o->n_cols, sizeof col[0], cmp_int);
    for (int c = 0; c < PQPS_MAX_COLUMNS; c++) out->column_ids[c] = c < o->n_cols ? col[c] : -1;
    int by_rank[PQPS_MAX_LEAVES], slot_of[PQPS_MAX_LEAVES];
    for (int i = 0; i < o->n_leaves; i++) {                       /* insertion sort of the indices */
        int j = i;
        while (j > 0 && count_leaf_cmp(&o->leaf[by_rank[j - 1]], &o->leaf[i]) > 0) { by_rank[j] = by_rank[j - 1]; j--; }
        by_rank[j] = i;
    }
    for (int r = 0; r < o->n_leaves; r++) {
        const struct count_leaf *l = &o->leaf[by_rank[r]];
        slot_of[by_rank[r]] = r;
        out->prog.leaf[r].column = (uint32_t)count_find_col(col, o->n_cols, l->col);
        out->prog.leaf[r].negate = 0;
        out->prog.leaf[r].lo = l->lo;
        out->prog.leaf[r].span = l->span;
    }
    out->prog.n_queries = (uint32_t)o->n_queries;
    out->prog.n_leaves = (uint32_t)o->n_leaves;
    out->prog.n_columns = (uint32_t)o->n_cols;
    for (int q = 0; q < o->n_queries; q++) {
        out->prog.query[q] = o->query[q];
        for (uint32_t s = 0; s < o->query[q].n_steps; s++) out->prog.query[q].leaf[s] = (uint8_t)slot_of[o->query[q].leaf[s]];
    }
}

int hipCountManyPack(const struct hipCountQuery *queries, int n, int max_queries, struct hipCountBatch *batches, int *n_batches,
                     struct hipCountPlace *place) {
    if (n < 0) return count_fail(-1, "a negative number of queries");
    if ((n && !queries) || !batches || !n_batches || !place) return count_fail(-1, "NULL argument");
    if (max_queries < 1 || max_queries > (int)PQPS_COUNT_MANY_MAX) return count_fail(-1, "queries per batch outside 1 .. 16");
    for (int i = 0; i < n; i++) {
        const pqps_predicate *p = queries[i].pred;
        const int *ids = queries[i].column_ids;
        if (!p || !ids) return count_fail(i, "no predicate or no column ids");
        if (p->n_leaves > PQPS_MAX_LEAVES || p->n_columns > PQPS_MAX_COLUMNS) return count_fail(i, "too many leaves or columns");
        uint32_t prev = 0;
        for (uint32_t k = 0; k < p->n_leaves; k++) {
            if (p->leaf[k].column >= p->n_columns) return count_fail(i, "a leaf's column is out of range");
            if (p->leaf[k].column < prev) return count_fail(i, "leaves not sorted by column");
            prev = p->leaf[k].column;
            if (ids[p->leaf[k].column] < 0) return count_fail(i, "a column slot without an id");
        }
        for (uint32_t s = 0; s < p->n_leaves; s++) {
            const uint8_t t = p->on_true[s], f = p->on_false[s];
            if (p->order[s] >= p->n_leaves) return count_fail(i, "a step's leaf slot is out of range");
            if ((t < PQPS_ACCEPT && (t <= s || t >= p->n_leaves)) || (f < PQPS_ACCEPT && (f <= s || f >= p->n_leaves)))
                return count_fail(i, "jump targets must point forward");
        }
    }
    struct count_open *o = calloc(1, sizeof *o);
    if (!o) return count_fail(-1, "out of memory");
    int nb = 0;
    for (int i = 0; i < n; i++) {
        const pqps_predicate *p = queries[i].pred;
        const int *ids = queries[i].column_ids;
        place[i].position = 0;
        place[i].constant = 0;
        if (p->n_leaves == 0) { place[i].batch = HIPCOUNT_CONSTANT; place[i].constant = (int)(p->truth & 1u); continue; }
        if (p->n_leaves > PQPS_TT_LEAVES) { place[i].batch = HIPCOUNT_ALONE; continue; }
        for (;;) {
            /* what the query adds to the open batch */
            struct count_leaf add_leaf[PQPS_TT_LEAVES];
            int add_col[PQPS_TT_LEAVES], n_add_leaf = 0, n_add_col = 0;
            for (uint32_t k = 0; k < p->n_leaves; k++) {
                int negated;
                const struct count_leaf l = count_canonical(ids[p->leaf[k].column], &p->leaf[k], &negated);
                if (count_find_leaf(o->leaf, o->n_leaves, &l) < 0 && count_find_leaf(add_leaf, n_add_leaf, &l) < 0) add_leaf[n_add_leaf++] = l;
                if (count_find_col(o->col, o->n_cols, l.col) < 0 && count_find_col(add_col, n_add_col, l.col) < 0) add_col[n_add_col++] = l.col;
            }
            const int fits = o->n_queries < max_queries && o->n_leaves + n_add_leaf <= PQPS_MAX_LEAVES && o->n_cols + n_add_col <= PQPS_MAX_COLUMNS;
            if (!fits) {                                         /* (never an empty batch: six leaves fit every cap) */
                count_close(o, &batches[nb++]);
                memset(o, 0, sizeof *o);
                continue;
            }
            for (int k = 0; k < n_add_leaf; k++) o->leaf[o->n_leaves++] = add_leaf[k];
            for (int k = 0; k < n_add_col; k++) o->col[o->n_cols++] = add_col[k];
            break;
        }
        pqps_count_query *q = &o->query[o->n_queries];
        memset(q, 0, sizeof *q);
        q->n_steps = p->n_leaves;
        for (uint32_t s = 0; s < p->n_leaves; s++) {
            const pqps_leaf *pl = &p->leaf[p->order[s]];
            int negated;
            const struct count_leaf l = count_canonical(ids[pl->column], pl, &negated);
            q->leaf[s] = (uint8_t)count_find_leaf(o->leaf, o->n_leaves, &l);
            q->on_true[s] = negated ? p->on_false[s] : p->on_true[s];
            q->on_false[s] = negated ? p->on_true[s] : p->on_false[s];
        }
        place[i].batch = nb;
        place[i].position = o->n_queries++;
    }
    if (o->n_queries) count_close(o, &batches[nb++]);
    free(o);
    *n_batches = nb;
    return 0;
}

/* ---- exact percentiles: the host half of the radix select (include/hipPredicate.h) ----------------------------------- */

unsigned long long hipQuantileRank(unsigned long long n, unsigned int ppm) {
    const unsigned long long p = ppm > HIPQUANTILE_PPM ? HIPQUANTILE_PPM : ppm;
    const unsigned long long up = (p * n + HIPQUANTILE_PPM - 1) / HIPQUANTILE_PPM;      /* ceil(p n / 10^6): p n < 2^20 n */
    return up > 0 ? up - 1 : 0;
}

unsigned int hipQuantileDigitBits(unsigned int bits_left, unsigned int key_bits, unsigned long long tables) {
    if (bits_left == 0) return 0;
    if (bits_left == key_bits && key_bits <= HIPQUANTILE_DIGIT_LDS) return key_bits;     /* a small domain: one pass */
    const unsigned int d = tables <= HIPQUANTILE_TABLES_LDS ? HIPQUANTILE_DIGIT_LDS : HIPQUANTILE_DIGIT_WIDE;
    return bits_left < d ? bits_left : d;
}

int hipQuantilePick(const uint64_t *tables, unsigned int digit_bits, const uint64_t *prefixes, int n_slots, const uint64_t *ranks,
                    const int *slots, int n_entries, unsigned int *digits, uint64_t *ranks_in, uint64_t *next_prefixes,
                    int *next_slots, int *n_next) {
    if (!tables || !ranks || !slots || !digits || !ranks_in || !next_prefixes || !next_slots || !n_next) {
        fprintf(stderr, "HIP engine: quantile pick: NULL argument\n");
        return -1;
    }
    if (digit_bits < 1 || digit_bits > 16 || n_slots < 1 || n_slots > HIPQUANTILE_MAX_FRACTIONS || n_entries < 0 ||
        n_entries > HIPQUANTILE_MAX_FRACTIONS) {
        fprintf(stderr, "HIP engine: quantile pick: %u digit bits, %d slots, %d entries\n", digit_bits, n_slots, n_entries);
        return -1;
    }
    const uint64_t width = 1ull << digit_bits;
    uint64_t next[HIPQUANTILE_MAX_FRACTIONS];
    for (int i = 0; i < n_entries; i++) {
        if (slots[i] < 0 || slots[i] >= n_slots) { fprintf(stderr, "HIP engine: quantile pick: slot %d of %d\n", slots[i], n_slots); return -1; }
        const uint64_t *t = tables + (uint64_t)slots[i] * width;
        uint64_t below = 0, dg = 0;
        while (dg < width && ranks[i] >= below + t[dg]) below += t[dg++];
        if (dg == width) {
            fprintf(stderr, "HIP engine: quantile pick: rank %llu in a table of %llu rows\n", (unsigned long long)ranks[i], (unsigned long long)below);
            return -1;
        }
        digits[i] = (unsigned int)dg;
        ranks_in[i] = ranks[i] - below;
        next[i] = ((prefixes ? prefixes[slots[i]] : 0ull) << digit_bits) | dg;
    }
    /* the distinct next prefixes, ascending (at most 16: an insertion sort), and every entry's place among them */
    int n = 0;
    for (int i = 0; i < n_entries; i++) {
        int at = 0;
        while (at < n && next_prefixes[at] < next[i]) at++;
        if (at < n && next_prefixes[at] == next[i]) continue;
        for (int k = n; k > at; k--) next_prefixes[k] = next_prefixes[k - 1];
        next_prefixes[at] = next[i];
        n++;
    }
    for (int i = 0; i < n_entries; i++) {
        int at = 0;
        while (next_prefixes[at] != next[i]) at++;
        next_slots[i] = at;
    }
    *n_next = n;
    return 0;
}
