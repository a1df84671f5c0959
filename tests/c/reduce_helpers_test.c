/* reduce_helpers_test.c -- the host side of the grouped queries' reduction, without a device: the accumulator and the
 * result arrays (bins_alloc, group_arrays_alloc / _set / _free) and the two combines (group_combine, first_combine).  They
 * are static functions of the engine, so the engine's source is included; nothing else of it is called, and the program is
 * linked with its device calls left unresolved.  Meant for the sanitizers, from the repository's root:
 *
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/c/reduce_helpers_test.c \
 *       -o reduce_helpers_test -lpthread -Wl,--unresolved-symbols=ignore-all && ./reduce_helpers_test
 */
#include "../../parallel-query-processing-system_amd/engine/hip/executeEngine-hip.c"

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } else printf("ok   %s\n", what); } while (0)

#define FLIP 0x8000000000000000ull
static uint64_t image(int32_t v) { return (uint64_t)(int64_t)v ^ FLIP; }

/* n bins, accumulated from two shards' downloads and stored into result arrays of as many groups */
static void accumulate_and_store(uint32_t n, bool valued) {
    const int vc = valued ? HIPCOL_EXIT_CODE : -1;
    uint64_t *acc = bins_alloc(n, valued);
    CHECK(acc != NULL || n == 0, "accumulator");                        /* (the engine never asks for 0 bins) */
    for (uint32_t k = 0; k < n; k++) CHECK(acc[k] == 0 && (!valued || (acc[n + k] == 0 && acc[2 * n + k] == UINT64_MAX && acc[3 * n + k] == 0)), "accumulator starts empty");
    void *host = malloc(bins_bytes(n, vc) + 1);
    for (int shard = 0; shard < 2; shard++) {
        for (uint32_t k = 0; k < n; k++) {
            if (!valued) { ((uint32_t *)host)[k] = 3 + (uint32_t)shard; continue; }
            uint64_t *h = host;
            h[k] = 3 + (uint64_t)shard;
            h[n + k] = shard ? 7 : UINT64_MAX - 2;                      /* the sum wraps modulo 2^64 */
            h[2 * n + k] = image(shard ? INT_MIN : 5);
            h[3 * n + k] = image(shard ? -1 : -9);
        }
        group_combine(&(struct bins_acc){ acc, n, vc }, host);
    }
    unsigned long long *counts = NULL;
    long long *sums = NULL, *mins = NULL, *maxs = NULL;
    CHECK(group_arrays_alloc(n, valued, &counts, &sums, &mins, &maxs) == 0, "result arrays");
    CHECK(counts && (valued ? sums && mins && maxs : !sums && !mins && !maxs), "... those of the form");
    for (uint32_t k = 0; k < n; k++) {
        group_arrays_set(counts, sums, mins, maxs, k, acc[k], valued ? acc[n + k] : 0, valued ? acc[2 * n + k] : 0, valued ? acc[3 * n + k] : 0, HIPKIND_I32);
        CHECK(counts[k] == 7, "counts added");
        if (valued) CHECK(sums[k] == 4 && mins[k] == INT_MIN && maxs[k] == -1, "sum modulo 2^64, i32 minimum INT_MIN and maximum -1 through the flip");
    }
    CHECK(counts[n] == 0 && (!valued || (sums[n] == 0 && mins[n] == 0 && maxs[n] == 0)), "the spare entry");
    if (valued && n) {                                                   /* a u64 value column: no flip */
        group_arrays_set(counts, sums, mins, maxs, 0, 1, UINT64_MAX, 2, UINT64_MAX, HIPKIND_U64);
        CHECK(sums[0] == -1 && mins[0] == 2 && (unsigned long long)maxs[0] == UINT64_MAX, "command_id values are their own images");
    }
    group_arrays_free(counts, sums, mins, maxs);
    free(host);
    free(acc);
}

/* first_combine over one shard's buffer [16 B matches][out][best] */
static void first_rows(uint32_t n) {
    struct group_plan gp;
    struct order_plan op;
    memset(&gp, 0, sizeof gp);
    memset(&op, 0, sizeof op);
    gp.n_bins = n;
    uint64_t *out = malloc(((size_t)n + 1) * 8), *best = malloc(((size_t)n + 1) * 8), *h = malloc((2 + 2 * (size_t)n) * 8), matches = 0;
    for (int wide = 0; wide < 2; wide++) {
        for (int fused = 0; fused < 2; fused++) {
            op.wide = wide;
            memset(out, 0xFF, ((size_t)n + 1) * 8);
            memset(best, 0xFF, ((size_t)n + 1) * 8);
            memset(h, 0xFF, (2 + 2 * (size_t)n) * 8);
            matches = 0;
            struct head_call a = { .gp = &gp, .op = &op, .rounds = 1, .out = out, .best = best, .matches = &matches, .fused = fused };
            h[0] = 0;
            first_combine(&a, h);                                        /* words of all ones in every bin */
            int groups = 0;
            for (uint32_t k = 0; k < n; k++) groups += out[k] != UINT64_MAX;
            CHECK(groups == 0 && matches == 0, "all ones in every bin: no groups");
            if (!n) continue;
            h[0] = 11;                                                   /* (the list call leaves these bytes unwritten) */
            h[2] = 40; h[2 + n] = 9;
            first_combine(&a, h);
            h[2] = 30; h[2 + n] = 9;                                     /* equal best, lower row */
            first_combine(&a, h);
            h[2] = 35; h[2 + n] = 9;                                     /* equal best, higher row */
            first_combine(&a, h);
            CHECK(out[0] == 30 && (!wide || best[0] == 9), "equal best: the lower row wins");
            h[2] = 50; h[2 + n] = 8;
            first_combine(&a, h);
            CHECK(out[0] == (wide ? 50u : 30u), "command_id: a lower best wins over a lower row; otherwise the minimum word");
            CHECK(matches == (fused ? 44u : 0u), "the match count is added up on the fused path only");
        }
    }
    free(h);
    free(best);
    free(out);
}

int main(void) {
    for (uint32_t n = 0; n < 3; n++) {
        accumulate_and_store(n, false);
        accumulate_and_store(n, true);
        first_rows(n);
    }
    printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures != 0;
}
