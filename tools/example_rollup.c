/* example_rollup.c -- sybl_table_rollup through the sybl_* C ABI from plain C99: build a small resident table block by block,
 * roll it up by (hour, host) into a NEW resident table holding count, the n / sum / max of latency and its exact p50 / p99
 * (pre-aggregation: the raw table is freed, the rollup lives on), print its first rows, and save it in the reference's on-disk
 * format.
 *
 *   gcc -std=c99 -Iinclude tools/example_rollup.c -Lsybil_amd -lsybilgpu -Wl,-rpath,$PWD/sybil_amd -o example_rollup
 *   ./example_rollup <output dir>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sybilgpu.h"

#define BLOCKS 3
#define BLOCK_N 4000

static int die(const char *what) {
    fprintf(stderr, "%s: %s\n", what, sybl_last_error());
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <output dir>\n", argv[0]);
        return 2;
    }
    sybl_ctx *ctx = NULL;
    if (sybl_init(0, &ctx)) return die("sybl_init");
    sybl_table *tab = NULL;
    if (sybl_table_create(ctx, "events", &tab)) return die("sybl_table_create");
    if (sybl_table_add_column(tab, "time", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(tab, "latency", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(tab, "host", SYBL_STR_VAL, 1, 0)) return die("sybl_table_add_column");

    /* one row per second, three blocks of four thousand: a little over three hours */
    static int64_t time_v[BLOCK_N], lat_v[BLOCK_N];
    static int32_t host_v[BLOCK_N];
    const char *hosts[3] = {"web1", "web2", "db1"};
    for (int b = 0; b < BLOCKS; b++) {
        for (int i = 0; i < BLOCK_N; i++) {
            time_v[i] = 1700000000 + (int64_t)b * BLOCK_N + i;
            lat_v[i] = (i * 37 + b) % 500;
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
        if (sybl_table_append_block(tab, BLOCK_N, 3, cols)) return die("sybl_table_append_block");
    }

    const char *groups[1] = {"host"};
    sybl_rollup_agg agg;
    agg.col = "latency";
    agg.ops = "n,sum,max,p50,p99";
    sybl_rollup_desc d;
    memset(&d, 0, sizeof(d));
    d.n_groups = 1;
    d.groups = groups;
    d.n_aggs = 1;
    d.aggs = &agg;
    d.time_col = "time";
    d.time_bucket = 3600;
    d.count_name = NULL; /* "count" */
    d.block_rows = 0;    /* 65536 */

    sybl_table *hourly = NULL;
    if (sybl_table_rollup(tab, &d, &hourly)) return die("sybl_table_rollup");
    printf("source: %lld rows in %lld blocks\n", (long long)sybl_table_rows(tab), (long long)sybl_table_blocks(tab));
    sybl_table_free(tab); /* the rollup owns everything it shows */

    sybl_rollup_stats st;
    if (sybl_table_rollup_stats(hourly, &st)) return die("sybl_table_rollup_stats");
    printf("hourly by host: %lld groups of %lld matching rows in %lld blocks (path %d, %lld cells; accumulate %.3f ms, emit %.3f ms)\n",
           (long long)st.groups, (long long)st.rows_matched, (long long)st.blocks_out, (int)st.path, (long long)st.cells_or_slots,
           st.accumulate_ms, st.emit_ms);
    sybl_rollup_pct_stats ps;
    if (sybl_table_rollup_pct_stats(hourly, &ps)) return die("sybl_table_rollup_pct_stats");
    printf("percentiles: %d columns of %lld sorted values with keys of %d bits (keys %.3f ms, sort %.3f ms, pick %.3f ms)\n", (int)ps.percentiles,
           (long long)ps.items, (int)ps.key_bits_max, ps.keys_ms, ps.sort_ms, ps.pick_ms);
    const int64_t g = sybl_table_rows(hourly);
    int64_t *hour = malloc((size_t)g * sizeof(int64_t)), *count = malloc((size_t)g * sizeof(int64_t)), *sum = malloc((size_t)g * sizeof(int64_t));
    int64_t *p50 = malloc((size_t)g * sizeof(int64_t)), *p99 = malloc((size_t)g * sizeof(int64_t));
    if (!hour || !count || !sum || !p50 || !p99) return 1;
    if (sybl_table_read_int(hourly, "time", 0, g, hour) || sybl_table_read_int(hourly, "count", 0, g, count) ||
        sybl_table_read_int(hourly, "latency_sum", 0, g, sum) || sybl_table_read_int(hourly, "latency_p50", 0, g, p50) ||
        sybl_table_read_int(hourly, "latency_p99", 0, g, p99))
        return die("sybl_table_read_int");
    int64_t total = 0;
    for (int64_t i = 0; i < g; i++) {
        total += count[i];
        if (i < 6)
            printf("  hour %lld: count %lld, latency_sum %lld, latency_p50 %lld, latency_p99 %lld\n", (long long)hour[i], (long long)count[i],
                   (long long)sum[i], (long long)p50[i], (long long)p99[i]);
    }
    printf("counts add up to %lld\n", (long long)total);
    free(hour);
    free(count);
    free(sum);
    free(p50);
    free(p99);
    if (sybl_table_save(hourly, argv[1])) return die("sybl_table_save");
    printf("saved under %s/events\n", argv[1]);

    sybl_table_free(hourly);
    sybl_shutdown(ctx);
    return 0;
}
