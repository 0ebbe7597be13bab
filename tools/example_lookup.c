/* example_lookup.c -- sybl_table_lookup through the sybl_* C ABI from plain C99: an event log keyed by host id, a small
 * second table that says which datacenter a host is in, the datacenter attached to every event as a NEW resident table, and
 * the average latency grouped by it.  Host 7 is in no datacenter: its events keep an unpopulated value (a left join).
 *
 *   gcc -std=c99 -Iinclude tools/example_lookup.c -Lsybil_amd -lsybilgpu -Wl,-rpath,$PWD/sybil_amd -o example_lookup
 *   ./example_lookup
 */
#include <stdio.h>
#include <string.h>

#include "sybilgpu.h"

#define BLOCKS 3
#define BLOCK_N 1000
#define HOSTS 8

static int die(const char *what) {
    fprintf(stderr, "%s: %s\n", what, sybl_last_error());
    return 1;
}

int main(void) {
    sybl_ctx *ctx = NULL;
    if (sybl_init(0, &ctx)) return die("sybl_init");

    /* the event log: host id, latency */
    sybl_table *events = NULL;
    if (sybl_table_create(ctx, "events", &events)) return die("sybl_table_create");
    if (sybl_table_add_column(events, "host", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(events, "latency", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    static int64_t host_v[BLOCK_N], lat_v[BLOCK_N];
    for (int b = 0; b < BLOCKS; b++) {
        for (int i = 0; i < BLOCK_N; i++) {
            host_v[i] = (i + b) % HOSTS;
            lat_v[i] = (i * 37 + b) % 500;
        }
        sybl_col_view cols[2];
        memset(cols, 0, sizeof(cols));
        cols[0].name = "host";
        cols[0].type = SYBL_INT_VAL;
        cols[0].ints = host_v;
        cols[1].name = "latency";
        cols[1].type = SYBL_INT_VAL;
        cols[1].ints = lat_v;
        if (sybl_table_append_block(events, BLOCK_N, 2, cols)) return die("sybl_table_append_block");
    }

    /* what a host id means: hosts 0..6, each in one of three datacenters */
    sybl_table *hosts = NULL;
    if (sybl_table_create(ctx, "hosts", &hosts)) return die("sybl_table_create");
    if (sybl_table_add_column(hosts, "host", SYBL_INT_VAL, 1, 0)) return die("sybl_table_add_column");
    if (sybl_table_add_column(hosts, "datacenter", SYBL_STR_VAL, 1, 0)) return die("sybl_table_add_column");
    {
        int64_t id_v[HOSTS - 1];
        int32_t dc_v[HOSTS - 1];
        const char *dcs[3] = {"ams", "fra", "sfo"};
        for (int i = 0; i < HOSTS - 1; i++) {
            id_v[i] = i;
            dc_v[i] = i % 3;
        }
        sybl_col_view cols[2];
        memset(cols, 0, sizeof(cols));
        cols[0].name = "host";
        cols[0].type = SYBL_INT_VAL;
        cols[0].ints = id_v;
        cols[1].name = "datacenter";
        cols[1].type = SYBL_STR_VAL;
        cols[1].str_ids = dc_v;
        cols[1].strings = dcs;
        cols[1].n_strings = 3;
        if (sybl_table_append_block(hosts, HOSTS - 1, 2, cols)) return die("sybl_table_append_block");
    }

    sybl_lookup_desc d;
    memset(&d, 0, sizeof(d));
    d.dim = hosts;
    d.key = "host";
    d.dim_key = NULL; /* the same name */
    d.columns = NULL; /* every column of hosts but the key */
    d.prefix = "host_";
    sybl_table *joined = NULL;
    if (sybl_table_lookup(events, &d, &joined)) return die("sybl_table_lookup");
    sybl_table_free(events); /* the output owns everything it shows */
    sybl_table_free(hosts);

    sybl_lookup_stats st;
    if (sybl_table_lookup_stats(joined, &st)) return die("sybl_table_lookup_stats");
    printf("%lld rows in %lld blocks, %lld matched one of %lld hosts (path %d; build %.3f ms, probe %.3f ms, gather %.3f ms)\n",
           (long long)st.rows, (long long)st.blocks, (long long)st.matched, (long long)st.dim_keys, (int)st.path, st.build_ms, st.probe_ms,
           st.gather_ms);

    /* average latency by datacenter: a plain scan of the new table */
    const char *groups[1] = {"host_datacenter"};
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
    if (sybl_query_prepare(joined, &q, &query)) return die("sybl_query_prepare");
    if (sybl_query_scan(query)) return die("sybl_query_scan");
    if (sybl_query_finalize(query, &res)) return die("sybl_query_finalize");
    printf("%s\n", sybl_result_render(res, 0));

    sybl_result_free(res);
    sybl_query_free(query);
    sybl_table_free(joined);
    sybl_shutdown(ctx);
    return 0;
}
