/* count_many_helpers_test.c -- hipCountManyPack, the batches of "several COUNT(*), one scan", without a device: predicates
 * compiled by hipCompileWherePlan are packed, every batch is evaluated row by row over a small table (the jump program as the
 * batch carries it, forwards) and compared with the predicate's own truth table; the caps, the places and the refusals.
 * Pure host code of engine/hip/hipPredicate.c, which is included.  Built with the host sanitizers by
 * tests/test_count_many_helpers.py; by hand, from the repository's root:
 *
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/c/count_many_helpers_test.c \
 *       -o count_many_helpers_test && ./count_many_helpers_test
 */
#include "../../parallel-query-processing-system_amd/engine/hip/hipPredicate.c"

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } else printf("ok   %s\n", what); } while (0)

static const char *const k_words[] = { "ann", "bob", "cy", "dee", "eve" };

static void schema_of(struct hipSchema *s) {
    memset(s, 0, sizeof *s);
    static const int kinds[12] = { HIPKIND_U64, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_I32, HIPKIND_DICT, HIPKIND_BOOL, HIPKIND_DICT,
                                   HIPKIND_I32, HIPKIND_DICT, HIPKIND_DICT, HIPKIND_I32 };
    static const uint32_t widths[12] = { 8, 1, 1, 1, 4, 1, 1, 1, 4, 1, 1, 4 };
    for (int c = 0; c < 12; c++) {
        s->col[c].present = 1;
        s->col[c].kind = kinds[c];
        s->col[c].width = widths[c];
        if (kinds[c] == HIPKIND_DICT) { s->col[c].dict_count = 5; s->col[c].dict = k_words; }
    }
}

/* row r of the table: the value of column c as the device holds it (u64 / the u32 bits of an i32 / 0, 1 / a code) */
static uint64_t cell(int c, int r) {
    switch (c) {
    case 0: return r == 0 ? UINT64_MAX : r == 1 ? 0 : (uint64_t)(r * 37 % 50);
    case 4: return (uint32_t)(r % 7 - 3);
    case 6: return (uint64_t)(r % 3 == 0);
    case 8: return (uint32_t)(1000 + r % 40);
    case 11: return (uint32_t)(r % 6);
    default: return (uint64_t)((r * (c + 3)) % 5);
    }
}
#define N_ROWS 210

static int window(int c, uint64_t lo, uint64_t span, int r) {
    if (c == 0) return cell(c, r) - lo <= span;
    return (uint32_t)((uint32_t)cell(c, r) - (uint32_t)lo) <= (uint32_t)span;
}

static int pred_row(const pqps_predicate *p, const int *ids, int r) {
    if (p->n_leaves == 0) return (int)(p->truth & 1u);
    uint32_t s = 0;
    while (s < PQPS_ACCEPT) {
        const pqps_leaf *l = &p->leaf[p->order[s]];
        const int hit = window(ids[l->column], l->lo, l->span, r) != (l->negate != 0);
        s = hit ? p->on_true[s] : p->on_false[s];
    }
    return s == PQPS_ACCEPT;
}

static int batch_row(const struct hipCountBatch *b, int pos, int r) {
    const pqps_count_query *q = &b->prog.query[pos];
    if (q->n_steps == 0) return q->constant;
    uint32_t s = 0;
    while (s < PQPS_ACCEPT) {
        const pqps_leaf *l = &b->prog.leaf[q->leaf[s]];
        s = window(b->column_ids[l->column], l->lo, l->span, r) ? q->on_true[s] : q->on_false[s];
    }
    return s == PQPS_ACCEPT;
}

#define MAX_Q 48
static struct hipPlan g_plan[MAX_Q];
static struct hipCountQuery g_query[MAX_Q];
static int g_n;

static void add(const struct hipSchema *s, struct whereClauseS *where) {
    char err[120];
    if (hipCompileWherePlan(s, where, &g_plan[g_n], err, sizeof err) != 0 || g_plan[g_n].n_passes != 1) { printf("FAIL compile: %s\n", err); failures++; return; }
    g_query[g_n].pred = &g_plan[g_n].pass[0].pred;
    g_query[g_n].column_ids = g_plan[g_n].pass[0].column_ids;
    g_n++;
}

static void reset(void) {
    for (int i = 0; i < g_n; i++) hipPlanFree(&g_plan[i]);
    g_n = 0;
}

/* packs g_query[0 .. g_n), checks every batch's shape and every placed query row by row; -> the number of batches, -1 */
static int pack_and_check(int cap, struct hipCountBatch *batches, struct hipCountPlace *place) {
    int nb = -1, ok = 1;
    if (hipCountManyPack(g_query, g_n, cap, batches, &nb, place) != 0) return -1;
    for (int b = 0; b < nb; b++) {
        const pqps_count_many *p = &batches[b].prog;
        ok = ok && p->n_queries >= 1 && p->n_queries <= (uint32_t)cap && p->n_leaves <= PQPS_MAX_LEAVES && p->n_columns <= PQPS_MAX_COLUMNS;
        for (uint32_t k = 0; k < p->n_leaves; k++) {
            ok = ok && p->leaf[k].negate == 0 && p->leaf[k].column < p->n_columns;
            if (k) ok = ok && (p->leaf[k - 1].column < p->leaf[k].column || (p->leaf[k - 1].column == p->leaf[k].column &&
                               (p->leaf[k - 1].lo < p->leaf[k].lo || (p->leaf[k - 1].lo == p->leaf[k].lo && p->leaf[k - 1].span < p->leaf[k].span))));
        }
        for (uint32_t c = 0; c < PQPS_MAX_COLUMNS; c++)
            ok = ok && (c < p->n_columns ? batches[b].column_ids[c] >= 0 && (c == 0 || batches[b].column_ids[c - 1] < batches[b].column_ids[c]) : batches[b].column_ids[c] == -1);
    }
    for (int i = 0; i < g_n && ok; i++) {
        const pqps_predicate *p = g_query[i].pred;
        if (p->n_leaves == 0) { ok = place[i].batch == HIPCOUNT_CONSTANT && place[i].constant == (int)(p->truth & 1u); continue; }
        if (p->n_leaves > PQPS_TT_LEAVES) { ok = place[i].batch == HIPCOUNT_ALONE; continue; }
        ok = place[i].batch >= 0 && place[i].batch < nb && place[i].position >= 0 && (uint32_t)place[i].position < batches[place[i].batch].prog.n_queries;
        for (int r = 0; r < N_ROWS && ok; r++) ok = batch_row(&batches[place[i].batch], place[i].position, r) == pred_row(p, g_query[i].column_ids, r);
    }
    return ok ? nb : -1;
}

static struct whereClauseS leaf(const char *a, const char *op, const char *v) {
    struct whereClauseS w = { .attribute = (char *)a, .operator = (char *)op, .value = (char *)v };
    return w;
}

static void packing(void) {
    struct hipSchema s;
    schema_of(&s);
    static struct hipCountBatch batches[MAX_Q];
    static struct hipCountPlace place[MAX_Q];

    struct whereClauseS gt = leaf("risk_level", ">", "3"), le = leaf("risk_level", "<=", "3"), ge = leaf("risk_level", ">=", "4");
    struct whereClauseS ex = leaf("exit_code", ">", "3");
    add(&s, &gt); add(&s, &le); add(&s, &ge); add(&s, &ex); add(&s, &gt);
    CHECK(pack_and_check(16, batches, place) == 1, "pack: five one-leaf queries, one batch, every row as the predicates say");
    CHECK(batches[0].prog.n_leaves == 2 && batches[0].prog.n_columns == 2 && batches[0].prog.n_queries == 5,
          "pack: > 3, <= 3 and >= 4 share a leaf; the same window on another column is a second leaf; a duplicate is a second query");
    CHECK(batches[0].prog.query[0].on_true[0] == batches[0].prog.query[1].on_false[0] && batches[0].prog.query[0].on_false[0] == batches[0].prog.query[1].on_true[0] &&
          batches[0].prog.query[0].leaf[0] == batches[0].prog.query[1].leaf[0], "pack: the complement is the same leaf with the targets swapped");
    CHECK(batches[0].column_ids[0] == 4 && batches[0].column_ids[1] == 11, "pack: the columns ascending by id");
    reset();

    /* (a AND b) OR (c AND NOT d) over four columns, an 8-byte one among them; a constant; no WHERE */
    struct whereClauseS d = leaf("command_id", "!=", "0"), c = leaf("sudo_used", "=", "TRUE"), b = leaf("user_name", ">=", "cy"), a = leaf("user_id", "<", "1020");
    a.next = &b; a.logical_op = "AND";
    c.next = &d; c.logical_op = "AND";
    struct whereClauseS left = { .sub = &a }, right = { .sub = &c };
    left.next = &right; left.logical_op = "OR";
    struct whereClauseS folded = leaf("user_name", "<", "ann"), wide = leaf("command_id", ">=", "18446744073709551615");
    add(&s, &left); add(&s, &folded); add(&s, NULL); add(&s, &wide);
    CHECK(pack_and_check(16, batches, place) == 1 && place[1].batch == HIPCOUNT_CONSTANT && place[1].constant == 0 && place[2].batch == HIPCOUNT_CONSTANT &&
          place[2].constant == 1 && place[0].batch == 0 && place[0].position == 0 && place[3].position == 1, "pack: a nested clause, both constants, a 64-bit window");
    CHECK(batches[0].prog.n_columns == 4 && batches[0].prog.query[0].n_steps == 4, "pack: four steps over four columns");
    reset();

    /* seventeen queries: the cap; with a cap of 4: five batches */
    struct whereClauseS one[17];
    char text[17][8];
    for (int i = 0; i < 17; i++) { snprintf(text[i], sizeof text[i], "%d", 1000 + i % 5); one[i] = leaf("user_id", "=", text[i]); add(&s, &one[i]); }
    CHECK(pack_and_check(16, batches, place) == 2 && batches[0].prog.n_queries == 16 && batches[1].prog.n_queries == 1 && place[16].batch == 1 && place[16].position == 0,
          "pack: the 17th query opens a batch");
    CHECK(pack_and_check(4, batches, place) == 5 && batches[4].prog.n_queries == 1 && place[7].batch == 1 && place[7].position == 3, "pack: a cap of four");
    CHECK(pack_and_check(1, batches, place) == 17, "pack: a cap of one");
    reset();

    /* three new windows per query: the eleventh brings the 33rd leaf; a 7-leaf query stays alone */
    struct whereClauseS or3[12][7];
    char val[12][7][8];
    for (int i = 0; i < 12; i++) {
        const int n = i == 11 ? 7 : 3;
        for (int k = 0; k < n; k++) {
            snprintf(val[i][k], sizeof val[i][k], "%d", 1000 + 3 * i + k);
            or3[i][k] = leaf("user_id", "=", val[i][k]);
            if (k) { or3[i][k - 1].next = &or3[i][k]; or3[i][k - 1].logical_op = "OR"; }
        }
        add(&s, &or3[i][0]);
    }
    CHECK(pack_and_check(16, batches, place) == 2 && batches[0].prog.n_leaves == 30 && batches[0].prog.n_queries == 10 && batches[1].prog.n_leaves == 3 &&
          place[10].batch == 1 && place[11].batch == HIPCOUNT_ALONE, "pack: the 33rd distinct leaf opens a batch; seven leaves are alone");
    reset();

    /* every column in one union */
    static const char *const cols[12] = { "command_id", "raw_command", "base_command", "shell_type", "exit_code", "timestamp", "sudo_used", "working_directory",
                                          "user_id", "user_name", "host_name", "risk_level" };
    struct whereClauseS each[12];
    for (int i = 0; i < 12; i++) { each[i] = leaf(cols[i], "!=", i == 6 ? "TRUE" : (s.col[i].kind == HIPKIND_DICT ? "bob" : "2")); add(&s, &each[i]); }
    CHECK(pack_and_check(16, batches, place) == 1 && batches[0].prog.n_columns == 12 && batches[0].prog.n_leaves == 12, "pack: twelve columns in one batch");
    reset();
    CHECK(hipCountManyPack(NULL, 0, 16, batches, &(int){ 9 }, place) == 0, "pack: no queries");
}

static void refusals(void) {
    struct hipSchema s;
    schema_of(&s);
    struct whereClauseS b = leaf("sudo_used", "=", "TRUE"), a = leaf("risk_level", ">", "3");
    a.next = &b; a.logical_op = "AND";
    add(&s, &a);
    static struct hipCountBatch batches[2];
    struct hipCountPlace place[2];
    int nb = 77;
    memset(batches, 0x5A, sizeof batches);
    memset(place, 0x5A, sizeof place);
    static struct hipCountBatch batches_before[2];
    struct hipCountPlace place_before[2];
    memcpy(batches_before, batches, sizeof batches);
    memcpy(place_before, place, sizeof place);
#define REFUSED(call, what) CHECK((call) == -1 && nb == 77 && memcmp(batches, batches_before, sizeof batches) == 0 && memcmp(place, place_before, sizeof place) == 0, what)
    REFUSED(hipCountManyPack(NULL, 1, 16, batches, &nb, place), "refused: no queries but n = 1");
    REFUSED(hipCountManyPack(g_query, 1, 16, NULL, &nb, place), "refused: no batches");
    REFUSED(hipCountManyPack(g_query, 1, 16, batches, NULL, place), "refused: no batch count");
    REFUSED(hipCountManyPack(g_query, 1, 16, batches, &nb, NULL), "refused: no places");
    REFUSED(hipCountManyPack(g_query, -1, 16, batches, &nb, place), "refused: n < 0");
    REFUSED(hipCountManyPack(g_query, 1, 0, batches, &nb, place), "refused: a cap of 0");
    REFUSED(hipCountManyPack(g_query, 1, 17, batches, &nb, place), "refused: a cap of 17");
    pqps_predicate bad;
    struct hipCountQuery q = { &bad, g_query[0].column_ids };
    static const struct { int field, step, value; const char *what; } k_bad[] = {
        { 0, 0, 0, "refused: on_true onto itself" }, { 1, 1, 0, "refused: on_false backwards" }, { 0, 0, 2, "refused: on_true past the last step" },
        { 1, 1, 1, "refused: on_false onto itself" }, { 2, 1, 2, "refused: a leaf slot out of range" },
    };
    for (size_t i = 0; i < sizeof k_bad / sizeof *k_bad; i++) {
        bad = *g_query[0].pred;
        (k_bad[i].field == 0 ? bad.on_true : k_bad[i].field == 1 ? bad.on_false : bad.order)[k_bad[i].step] = (uint8_t)k_bad[i].value;
        REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), k_bad[i].what);
    }
    bad = *g_query[0].pred; bad.leaf[1].column = 2;
    REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), "refused: a leaf's column out of range");
    bad = *g_query[0].pred; bad.leaf[0].column = 1; bad.leaf[1].column = 0;
    REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), "refused: leaves not sorted by column");
    bad = *g_query[0].pred; bad.n_leaves = PQPS_MAX_LEAVES + 1;
    REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), "refused: too many leaves");
    bad = *g_query[0].pred;
    int no_ids[PQPS_MAX_COLUMNS];
    for (int c = 0; c < PQPS_MAX_COLUMNS; c++) no_ids[c] = -1;
    q.column_ids = no_ids;
    REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), "refused: a column slot without an id");
    q.column_ids = NULL;
    REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), "refused: no column ids");
    q.pred = NULL; q.column_ids = g_query[0].column_ids;
    REFUSED(hipCountManyPack(&q, 1, 16, batches, &nb, place), "refused: no predicate");
    CHECK(hipCountManyPack(g_query, 1, 16, batches, &nb, place) == 0 && nb == 1 && place[0].batch == 0 && place[0].position == 0, "refused: and the good one goes through");
    reset();
}

int main(void) {
    packing();
    refusals();
    printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures ? 1 : 0;
}
