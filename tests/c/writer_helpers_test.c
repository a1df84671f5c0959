/* writer_helpers_test.c -- what INSERT, DELETE, UPDATE and batch INSERT share on the host, without a device: the rank of a
 * string in a dictionary (hipDictionaryRank), the host part of a dictionary insert (dictionary_insert), the cached range of
 * a column (bounds_cover), the codes of a width (code_limit against width_for_count) and the host row store
 * (host_rows_reserve).  All but the first are static functions of the engine, so the engine's sources are included; nothing
 * else of them is called, and the program is linked with their device calls left unresolved.  Meant for the sanitizers, from
 * the repository's root:
 *
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/c/writer_helpers_test.c \
 *       -o writer_helpers_test -lpthread -Wl,--unresolved-symbols=ignore-all && ./writer_helpers_test
 */
#include "../../parallel-query-processing-system_amd/engine/hip/buildEngine-hip.c"      /* (first: it asks for _DEFAULT_SOURCE) */
#include "../../parallel-query-processing-system_amd/engine/hip/hipPredicate.c"
#include "../../parallel-query-processing-system_amd/engine/hip/executeEngine-hip.c"

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } else printf("ok   %s\n", what); } while (0)

static void rank_is(const char *const *values, int count, const char *text, int rank, int present, const char *what) {
    int p = -1;
    const int r = hipDictionaryRank(values, count, text, &p);
    CHECK(r == rank && p == present, what);
}

static void dictionary_rank(void) {
    static const char *const v[] = { "bash", "fish", "zsh" };
    rank_is(v, 0, "bash", 0, 0, "rank: an empty dictionary");
    rank_is(v, 3, "ash", 0, 0, "rank: below the first value");
    rank_is(v, 3, "bash", 0, 1, "rank: the first value");
    rank_is(v, 3, "csh", 1, 0, "rank: between two values");
    rank_is(v, 3, "fish", 1, 1, "rank: a middle value");
    rank_is(v, 3, "zsh", 2, 1, "rank: the last value");
    rank_is(v, 3, "zshh", 3, 0, "rank: above the last value");
    rank_is(v, 3, "fis", 1, 0, "rank: a proper prefix of a value is absent, at that value's position");
    rank_is(v, 1, "bash", 0, 1, "rank: one value, present");
    rank_is(v, 1, "c", 1, 0, "rank: one value, above it");
}

static bool ascending(const struct hipDictionary *d) {
    for (int i = 1; i < d->count; i++) if (strcmp(d->values[i - 1], d->values[i]) >= 0) return false;
    return true;
}

/* `text` inserted at its rank: the dictionary one longer, still ascending, every earlier string still there, the copy its own */
static void insert_at_rank(struct hipDictionary *d, const char *text, int expect_pos) {
    const char *before[8];
    const int n = d->count;
    for (int i = 0; i < n; i++) before[i] = d->values[i];
    int present = -1;
    const int pos = hipDictionaryRank(d->values, d->count, text, &present);
    CHECK(pos == expect_pos && !present, "insert: the rank of a new string");
    dictionary_insert(d, (size_t)pos, text);
    CHECK(d->count == n + 1, "insert: count grew by one");
    bool kept = true;                                                    /* (pointers first: nothing below reads a slot that was not written) */
    for (int i = 0; i < n; i++) kept = kept && d->values[i < pos ? i : i + 1] == before[i];
    CHECK(kept, "insert: the earlier strings keep their order around the rank");
    if (!kept || d->count != n + 1) return;
    CHECK(d->values[pos] != text && strcmp(d->values[pos], text) == 0, "insert: an owned copy stands at the rank");
    CHECK(ascending(d), "insert: strictly ascending under strcmp");
    CHECK(hipDictionaryRank(d->values, d->count, text, &present) == pos && present, "insert: the string is found at its rank");
}

static void dictionary_inserts(void) {
    struct hipDictionary d;
    memset(&d, 0, sizeof d);
    d.values = malloc(sizeof *d.values);
    d.values[0] = strdup("m");
    d.count = 1;
    /* at 0, at count, in the middle (two strings move), at 0 again (all four move), at count again */
    static const struct { const char *text; int pos; } k_new[] = { { "c", 0 }, { "x", 2 }, { "h", 1 }, { "a", 0 }, { "z", 5 } };
    for (size_t i = 0; i < sizeof k_new / sizeof *k_new && !failures; i++) insert_at_rank(&d, k_new[i].text, k_new[i].pos);
    if (failures) return;                                                /* (the pointers may then not be the dictionary's own) */
    for (int i = 0; i < d.count; i++) free((char *)d.values[i]);
    free(d.values);
}

static void cached_range(void) {
    struct hipTable t;
    memset(&t, 0, sizeof t);
    const int c = HIPCOL_EXIT_CODE, other = HIPCOL_USER_ID;
    t.bounds_lo[c] = 5; t.bounds_hi[c] = 7;
    bounds_cover(&t, c, -100, 100);
    CHECK(!t.bounds_known[c] && t.bounds_lo[c] == 5 && t.bounds_hi[c] == 7, "range: unknown stays unknown, lo and hi untouched");
    t.bounds_known[c] = 1;
    bounds_cover(&t, c, 6, 6);
    CHECK(t.bounds_lo[c] == 5 && t.bounds_hi[c] == 7, "range: a value inside changes nothing");
    bounds_cover(&t, c, 5, 7);
    CHECK(t.bounds_lo[c] == 5 && t.bounds_hi[c] == 7, "range: the range itself changes nothing");
    bounds_cover(&t, c, 3, 6);
    CHECK(t.bounds_lo[c] == 3 && t.bounds_hi[c] == 7, "range: lo moves out, hi stays");
    bounds_cover(&t, c, 4, 9);
    CHECK(t.bounds_lo[c] == 3 && t.bounds_hi[c] == 9, "range: hi moves out, lo does not move in");
    bounds_cover(&t, c, 20, 20);
    CHECK(t.bounds_lo[c] == 3 && t.bounds_hi[c] == 20, "range: a value above moves hi only");
    bounds_cover(&t, c, -20, -20);
    CHECK(t.bounds_lo[c] == -20 && t.bounds_hi[c] == 20, "range: a value below moves lo only");
    bounds_cover(&t, c, INT_MIN, INT_MAX);
    CHECK(t.bounds_lo[c] == INT_MIN && t.bounds_hi[c] == INT_MAX, "range: INT_MIN and INT_MAX are taken");
    bounds_cover(&t, c, 0, 0);
    CHECK(t.bounds_lo[c] == INT_MIN && t.bounds_hi[c] == INT_MAX, "range: the full range stays");
    CHECK(!t.bounds_known[other] && t.bounds_lo[other] == 0 && t.bounds_hi[other] == 0, "range: another column is untouched");
}

static void code_limits(void) {
    static const uint64_t counts[] = { 1, 256, 257, 65536, 65537 };
    static const uint32_t widths[] = { 1, 2, 4 };
    for (size_t i = 0; i < sizeof counts / sizeof *counts; i++) {
        const uint32_t w = width_for_count(counts[i]);
        uint32_t narrowest = 0;
        for (int k = 2; k >= 0; k--) if (code_limit(widths[k]) >= counts[i]) narrowest = widths[k];
        CHECK(w == narrowest, "width_for_count: the narrowest width whose code_limit holds the count");
    }
    CHECK(code_limit(0) == 1 && code_limit(1) == 256 && code_limit(2) == 65536 && code_limit(4) == 0xFFFFFFFFull, "code_limit: 1, 2^8, 2^16, 2^32 - 1");
}

/* every row of the store carries its number; all_records[i] point at row i */
static bool rows_whole(const struct engineS *e, const struct hipTable *t) {
    for (int i = 0; i < e->num_records; i++) {
        const record *r = &t->row_block[i];
        if (e->all_records[i] != r || r->command_id != (unsigned long long)i + 1 || r->exit_code != -i || r->user_name[0] != (char)('a' + i % 26)) return false;
    }
    return true;
}

static void reserve_and_fill(struct engineS *e, struct hipTable *t, size_t total, const char *what) {
    CHECK(host_rows_reserve(e, t, total) == 0, what);
    CHECK(t->row_block && e->all_records && t->row_capacity >= total, "reserve: a block and pointers with room for the total");
    if (!t->row_block || !e->all_records || t->row_capacity < total) return;
    CHECK(rows_whole(e, t), "reserve: the earlier rows' bytes and pointers");
    for (size_t i = (size_t)e->num_records; i < total; i++) {           /* (the sanitizer sees a store past either allocation) */
        memset(&t->row_block[i], 0, sizeof(record));
        t->row_block[i].command_id = i + 1;
        t->row_block[i].exit_code = -(int)i;
        t->row_block[i].user_name[0] = (char)('a' + i % 26);
        e->all_records[i] = &t->row_block[i];
    }
    e->num_records = (int)total;
}

static void host_rows(void) {
    struct engineS e;
    struct hipTable t;
    memset(&e, 0, sizeof e);
    memset(&t, 0, sizeof t);
    reserve_and_fill(&e, &t, 1, "reserve: the first row of a table without a block");
    CHECK(t.row_block && e.all_records && t.row_capacity >= 1, "reserve: the block and the pointers exist");
    reserve_and_fill(&e, &t, t.row_capacity, "reserve: up to the capacity");
    const record *block = t.row_block;
    record **ptrs = e.all_records;
    const size_t cap = t.row_capacity;
    CHECK(host_rows_reserve(&e, &t, cap) == 0 && t.row_block == block && e.all_records == ptrs && t.row_capacity == cap,
          "reserve: total == capacity moves nothing");
    reserve_and_fill(&e, &t, cap + 1, "reserve: capacity + 1");
    CHECK(t.row_capacity > cap + 1, "reserve: ... grows by more than the one row");
    reserve_and_fill(&e, &t, (size_t)e.num_records + 70000, "reserve: a jump by 70 000 rows");
    /* a block that certainly moved: the store copied into a fresh, tight allocation, the pointers left at the old one */
    const size_t n = (size_t)e.num_records;
    if (failures) return;                                                /* (a store that is not whole is not built upon) */
    record *tight = malloc(n * sizeof *tight);
    memcpy(tight, t.row_block, n * sizeof *tight);
    record *old = t.row_block;
    t.row_block = tight;
    t.row_capacity = n;
    for (size_t i = 0; i < n; i++) e.all_records[i] = &tight[i];
    free(old);
    void *wedge = malloc(64);                                            /* (keeps the block from growing in place) */
    reserve_and_fill(&e, &t, n + 1, "reserve: one row more than a tight block");
    free(wedge);
    free(t.row_block);
    free(e.all_records);
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);                                    /* what was checked is on record whatever follows */
    dictionary_rank();
    dictionary_inserts();
    cached_range();
    code_limits();
    host_rows();
    printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures != 0;
}
