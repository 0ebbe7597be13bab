/* example_compute.c -- sybl_table_compute through the sybl_* C ABI from plain C99: a request log with start and end times and a
 * status, two columns computed from them as a NEW resident table -- latency = end - start and is_error = status >= 500 --, and
 * the average latency grouped by is_error.  Rows whose end time is unknown keep an unpopulated latency.
 *
 *   gcc -std=c99 -Iinclude tools/example_compute.c -Lsybil_amd -lsybilgpu -Wl,-rpath,$PWD/sybil_amd -o example_compute
 *   ./example_compute
 */
#include <stdio.h>
#include <string.h>

#include "sybilgpu.h"

#define BLOCKS 3
#define BLOCK_N 1000

static int die(const char *what) {
    fprintf(stderr, "%s: %s\n", what, sybl_last_error());
    return 1;
}

int main(void) {
    sybl_ctx *ctx = NULL;
    if (sybl_init(0, &ctx)) return die("sybl_init");

    sybl_table *log = NULL;
    if (sybl_table_create(ctx, "requests", &log)) return die("sybl_table_create");
    if (sybl_table_add_column(log, "start", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(log, "end", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(log, "status", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    static int64_t start_v[BLOCK_N], end_v[BLOCK_N], status_v[BLOCK_N];
    static uint8_t end_p[BLOCK_N];
    for (int b = 0; b < BLOCKS; b++) {
        for (int i = 0; i < BLOCK_N; i++) {
            start_v[i] = 1700000000000LL + (int64_t)b * 60000 + i * 50;
            end_v[i] = start_v[i] + (i * 37 + b) % 500;
            end_p[i] = i % 97 != 0; /* a request that never finished */
            status_v[i] = i % 13 == 0 ? 503 : 200;
        }
        sybl_col_view cols[3];
        memset(cols, 0, sizeof(cols));
        cols[0].name = "start";
        cols[0].type = SYBL_INT_VAL;
        cols[0].ints = start_v;
        cols[1].name = "end";
        cols[1].type = SYBL_INT_VAL;
        cols[1].ints = end_v;
        cols[1].populated = end_p;
        cols[2].name = "status";
        cols[2].type = SYBL_INT_VAL;
        cols[2].ints = status_v;
        if (sybl_table_append_block(log, BLOCK_N, 3, cols)) return die("sybl_table_append_block");
    }
    if (sybl_table_compact(log)) return die("sybl_table_compact");

    sybl_compute_col exprs[2];
    exprs[0].name = "latency";
    exprs[0].expr = "end - start";
    exprs[1].name = "is_error";
    exprs[1].expr = "status >= 500";
    sybl_compute_desc d;
    memset(&d, 0, sizeof(d));
    d.n_exprs = 2;
    d.exprs = exprs;
    sybl_table *out = NULL;
    if (sybl_table_compute(log, &d, &out)) return die("sybl_table_compute");
    sybl_table_free(log); /* the output owns everything it shows */

    sybl_compute_stats st;
    if (sybl_table_compute_stats(out, &st)) return die("sybl_table_compute_stats");
    int32_t width = 0;
    int64_t base = 0;
    if (sybl_table_column_storage(out, "latency", &width, &base)) return die("sybl_table_column_storage");
    printf("%lld rows in %lld blocks, %d expressions of %d ops, %lld unpopulated results; latency is stored at %d byte(s)\n"
           "range %.3f ms, store %.3f ms, statistics %.3f ms\n",
           (long long)st.rows, (long long)st.blocks, (int)st.exprs, (int)st.ops, (long long)st.unpopulated, (int)width, st.range_ms,
           st.store_ms, st.stats_ms);

    /* average latency by is_error: a plain scan of the new table */
    const char *groups[1] = {"is_error"};
    const char *aggs[1] = {"latency"};
    sybl_query_desc q;
    memset(&q, 0, sizeof(q));
    q.n_groups = 1;
    q.groups = groups;
    q.n_aggs = 1;
    q.aggs = aggs;
    q.op = SYBL_AGG_AVG;
    sybl_query *query = NULL;
    sybl_result *res = NULL;
    if (sybl_query_prepare(out, &q, &query)) return die("sybl_query_prepare");
    if (sybl_query_scan(query)) return die("sybl_query_scan");
    if (sybl_query_finalize(query, &res)) return die("sybl_query_finalize");
    printf("%s\n", sybl_result_render(res, 0));

    sybl_result_free(res);
    sybl_query_free(query);
    sybl_table_free(out);
    sybl_shutdown(ctx);
    return 0;
}
