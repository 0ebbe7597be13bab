/* example_samples.c -- `sybil query -samples` through the sybl_* C ABI from plain C99: open a table, ask for the newest
 * rows behind `-int-filter <v>:gt:<x>` (or, with a sort column, the rows with its largest values), walk the returned
 * columns, print the -json form.
 *
 *   gcc -std=c99 -Iinclude tools/example_samples.c -Lsybil_amd -lsybilgpu -Wl,-rpath,$PWD/sybil_amd -o example_samples
 *   ./example_samples db events pageload 100 5 [<sort column>]
 *
 * The table is freed BEFORE the result is read: a samples result owns everything it shows.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sybilgpu.h"

static int die(const char *what) {
    fprintf(stderr, "%s: %s\n", what, sybl_last_error());
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s <dir> <table> <int column> <greater-than> <limit> [<sort column>]\n", argv[0]);
        return 2;
    }
    sybl_ctx *ctx = NULL;
    if (sybl_init(0, &ctx)) return die("sybl_init");
    sybl_table *tab = NULL;
    /* every column becomes resident: samples return whole rows (LoadAllColumns) */
    if (sybl_table_open_flags(ctx, argv[1], argv[2], NULL, 0, 0, 1, SYBL_OPEN_COMPACT, &tab)) return die("sybl_table_open_flags");

    sybl_filter filt;
    memset(&filt, 0, sizeof(filt));
    filt.col = argv[3];
    filt.op = SYBL_OP_GT;
    filt.int_value = atoll(argv[4]);
    sybl_samples_desc d;
    memset(&d, 0, sizeof(d));
    d.n_filters = 1;
    d.filters = &filt;
    d.columns = NULL; /* every column */
    d.order_by = argc > 6 ? argv[6] : "$COUNT";
    d.order_asc = 0;
    d.limit = atoi(argv[5]);

    sybl_samples *smp = NULL;
    if (sybl_table_samples(tab, &d, &smp)) return die("sybl_table_samples");
    sybl_table_free(tab);

    sybl_samples_info info;
    if (sybl_samples_get_info(smp, &info)) return die("sybl_samples_get_info");
    printf("%lld rows of %lld matched in %lld of %lld blocks (filter %.3f ms over %lld blocks, select %.3f ms)\n", (long long)info.n_rows,
           (long long)info.matched, (long long)info.blocks_visited, (long long)info.blocks_total, info.filter_ms,
           (long long)info.blocks_filtered, info.select_ms);
    const int64_t *row_ids = NULL;
    if (sybl_samples_row_ids(smp, &row_ids)) return die("sybl_samples_row_ids");
    for (int64_t i = 0; i < info.n_rows; i++) {
        printf("row %lld:", (long long)row_ids[i]);
        for (int32_t c = 0; c < info.n_columns; c++) {
            sybl_samples_col col;
            if (sybl_samples_column(smp, c, &col)) return die("sybl_samples_column");
            if (!col.populated[i]) continue;
            if (col.type == SYBL_INT_VAL) {
                printf(" %s=%lld", col.name, (long long)col.ints[i]);
            } else if (col.type == SYBL_STR_VAL) {
                printf(" %s=%s", col.name, col.strings[i]);
            } else {
                printf(" %s=[", col.name);
                for (int64_t k = col.set_off[i]; k < col.set_off[i + 1]; k++) printf("%s%s", k > col.set_off[i] ? "," : "", col.set_strings[k]);
                printf("]");
            }
        }
        printf("\n");
    }
    const char *json = sybl_samples_render(smp);
    if (!json) return die("sybl_samples_render");
    printf("%s\n", json);

    sybl_samples_free(smp);
    sybl_shutdown(ctx);
    return 0;
}
