/* example_select.c -- sybl_table_select through the sybl_* C ABI from plain C99: build a small resident table block by block,
 * keep the rows with `time > T` as a NEW resident table (retention: the old table is freed, the new one lives on), print its
 * rows and blocks, and save it in the reference's on-disk format (the subset export).
 *
 *   gcc -std=c99 -Iinclude tools/example_select.c -Lsybil_amd -lsybilgpu -Wl,-rpath,$PWD/sybil_amd -o example_select
 *   ./example_select <output dir> [<T>]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sybilgpu.h"

#define BLOCKS 3
#define BLOCK_N 1000

static int die(const char *what) {
    fprintf(stderr, "%s: %s\n", what, sybl_last_error());
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <output dir> [<T>]\n", argv[0]);
        return 2;
    }
    const int64_t T = argc > 2 ? atoll(argv[2]) : 1700001499;
    sybl_ctx *ctx = NULL;
    if (sybl_init(0, &ctx)) return die("sybl_init");
    sybl_table *tab = NULL;
    if (sybl_table_create(ctx, "events", &tab)) return die("sybl_table_create");
    if (sybl_table_add_column(tab, "time", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(tab, "latency", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(tab, "host", SYBL_STR_VAL, 1, 0)) return die("sybl_table_add_column");

    /* one row per second, three blocks of a thousand */
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

    sybl_filter filt;
    memset(&filt, 0, sizeof(filt));
    filt.col = "time";
    filt.op = SYBL_OP_GT;
    filt.int_value = T;
    sybl_select_desc d;
    memset(&d, 0, sizeof(d));
    d.n_filters = 1;
    d.filters = &filt;
    d.columns = NULL;   /* every column */
    d.block_rows = 512; /* 0 = 65536 */

    sybl_table *kept = NULL;
    if (sybl_table_select(tab, &d, &kept)) return die("sybl_table_select");
    printf("source: %lld rows in %lld blocks\n", (long long)sybl_table_rows(tab), (long long)sybl_table_blocks(tab));
    sybl_table_free(tab); /* the selected table owns everything it shows */

    sybl_select_stats st;
    if (sybl_table_select_stats(kept, &st)) return die("sybl_table_select_stats");
    printf("time > %lld: %lld rows in %lld blocks (filter %.3f ms, rows %.3f ms, gather %.3f ms)\n", (long long)T,
           (long long)sybl_table_rows(kept), (long long)sybl_table_blocks(kept), st.filter_ms, st.rows_ms, st.gather_ms);
    if (sybl_table_save(kept, argv[1])) return die("sybl_table_save");
    printf("saved under %s/events\n", argv[1]);

    sybl_table_free(kept);
    sybl_shutdown(ctx);
    return 0;
}
