/* example_concat.c -- sybl_table_concat through the sybl_* C ABI from plain C99: two small resident tables in compact storage
 * whose host dictionaries overlap (in another id order) and whose latency ranges differ, joined end to end as a NEW
 * resident table; then what the call did (copies / transcodes), the merged dictionary, and a group-by over the result.
 *
 *   gcc -std=c99 -Iinclude tools/example_concat.c -Lsybil_amd -lsybilgpu -Wl,-rpath,$PWD/sybil_amd -o example_concat
 *   ./example_concat
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sybilgpu.h"

#define BLOCK_N 1000
#define NEW_N 700

static int die(const char *what) {
    fprintf(stderr, "%s: %s\n", what, sybl_last_error());
    return 1;
}

/* n rows from `time0` on: latency = lat0 + (i * 37) % lat_mod, host = hosts[i % 3] */
static int add_block(sybl_table *t, int n, int64_t time0, int64_t lat0, int64_t lat_mod, const char *const *hosts) {
    static int64_t time_v[BLOCK_N], lat_v[BLOCK_N];
    static int32_t host_v[BLOCK_N];
    for (int i = 0; i < n; i++) {
        time_v[i] = time0 + i;
        lat_v[i] = lat0 + ((int64_t)i * 37) % lat_mod;
        host_v[i] = i % 3;
    }
    sybl_col_view cols[3];
    memset(cols, 0, sizeof(cols));
    cols[0].name = "time";
    cols[0].type = SYBL_INT_VAL;
    cols[0].ints = time_v;
    cols[1].name = "latency";
    cols[1].type = SYBL_INT_VAL;
    cols[1].ints = lat_v;
    cols[2].name = "host";
    cols[2].type = SYBL_STR_VAL;
    cols[2].str_ids = host_v;
    cols[2].strings = hosts;
    cols[2].n_strings = 3;
    return sybl_table_append_block(t, n, 3, cols);
}

static int make_table(sybl_ctx *ctx, sybl_table **out) {
    if (sybl_table_create(ctx, "events", out)) return 1;
    if (sybl_table_add_column(*out, "time", SYBL_INT_VAL, 1, 0)) return 1;
    if (sybl_table_add_column(*out, "latency", SYBL_INT_VAL, 1, 0)) return 1;
    return sybl_table_add_column(*out, "host", SYBL_STR_VAL, 1, 0);
}

int main(void) {
    sybl_ctx *ctx = NULL;
    if (sybl_init(0, &ctx)) return die("sybl_init");
    const char *old_hosts[3] = {"web1", "web2", "db1"}, *new_hosts[3] = {"db1", "cache1", "web1"};
    sybl_table *main_t = NULL, *arrivals = NULL;
    if (make_table(ctx, &main_t) || make_table(ctx, &arrivals)) return die("sybl_table_create");
    /* the big table: latencies 0..199 fit a byte; the arrivals: 10000..69999 need two, from another base */
    if (add_block(main_t, BLOCK_N, 1700000000, 0, 200, old_hosts)) return die("sybl_table_append_block");
    if (add_block(main_t, BLOCK_N, 1700001000, 0, 200, old_hosts)) return die("sybl_table_append_block");
    if (add_block(arrivals, NEW_N, 1700002000, 10000, 60000, new_hosts)) return die("sybl_table_append_block");
    if (sybl_table_compact(main_t) || sybl_table_compact(arrivals)) return die("sybl_table_compact");

    sybl_table *both[2];
    both[0] = main_t;
    both[1] = arrivals;
    sybl_concat_desc d;
    memset(&d, 0, sizeof(d));
    d.n_tables = 2;
    d.tables = both;
    d.columns = NULL; /* the union of the sources' columns */
    sybl_table *all = NULL;
    if (sybl_table_concat(&d, &all)) return die("sybl_table_concat");
    sybl_table_free(main_t); /* the output owns everything it shows */
    sybl_table_free(arrivals);

    sybl_concat_stats st;
    if (sybl_table_concat_stats(all, &st)) return die("sybl_table_concat_stats");
    printf("concat: %lld rows in %lld blocks from %d tables, %d columns\n", (long long)st.rows, (long long)st.blocks, st.tables, st.columns);
    printf("pieces: %d copies, %d transcodes, %d through an id table\n", st.copies, st.transcodes, st.lut_transcodes);
    int32_t width = 0;
    int64_t base = 0;
    if (sybl_table_column_storage(all, "latency", &width, &base)) return die("sybl_table_column_storage");
    printf("latency: %d bytes from base %lld\n", width, (long long)base);
    const char *const *strings = NULL;
    int64_t n_strings = 0;
    if (sybl_table_column_dict(all, "host", &strings, &n_strings)) return die("sybl_table_column_dict");
    printf("hosts:");
    for (int64_t i = 0; i < n_strings; i++) printf(" %s", strings[i]);
    printf("\n");

    const char *groups[1] = {"host"}, *aggs[1] = {"latency"};
    sybl_query_desc qd;
    memset(&qd, 0, sizeof(qd));
    qd.n_groups = 1;
    qd.groups = groups;
    qd.n_aggs = 1;
    qd.aggs = aggs;
    qd.op = SYBL_AGG_AVG;
    qd.order_by = "$COUNT";
    sybl_query *q = NULL;
    if (sybl_query_prepare(all, &qd, &q)) return die("sybl_query_prepare");
    if (sybl_query_scan(q)) return die("sybl_query_scan");
    sybl_result *res = NULL;
    if (sybl_query_finalize(q, &res)) return die("sybl_query_finalize");
    const sybl_group_row *rows = NULL;
    int64_t n = 0;
    if (sybl_result_rows(res, 0, &rows, &n)) return die("sybl_result_rows");
    for (int64_t i = 0; i < n; i++)
        printf("group %s count %lld sum %lld\n", rows[i].group_by_key, (long long)rows[i].count, (long long)rows[i].aggs[0].sum);

    sybl_result_free(res);
    sybl_query_free(q);
    sybl_table_free(all);
    sybl_shutdown(ctx);
    return 0;
}
